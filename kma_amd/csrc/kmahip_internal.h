// kmahip_internal.h -- shared between the host-side loader and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>
#include "../../include/kmahip.h"

#define KMAHIP_EMPTY_VI 0xFFFFFFFFu
#define KMAHIP_BUCKET_SLOTS 4
#define KMAHIP_N_COUNTERS 32
// slots of kmahip_ws::counters that scan.hip and api.hip both name: live strand items on the bare list, and as records
#define KMAHIP_C_NACT 8
#define KMAHIP_C_NREC 21
#define KMAHIP_C_NREPL 22      // records whose diagonal the prefilter replaced by a better one (counted with the statistics on)
// KMAHIP_C_NREC counts the items that took the record route; of them the prefilter WRITES the records of those it does not settle
// itself (DevDB::span), densely, by a counter of their own: what the first tier's launch over records reads as its item count
// while the route is on (with the route off nothing is added to it: every record item's record is written, and C_NREC is read)
#define KMAHIP_C_NWRIT 19
#define KMAHIP_C_NSET 20       // record items the prefilter settled (always counted)
// the scan's queue (counted with the statistics on): k-mer starts its lanes left to the queue round, and the (group, pass) rounds that had any
#define KMAHIP_C_QENT 30
#define KMAHIP_C_QWG 31
// stage 3a's class queues (align.hip, api.hip): [+0..3] entries of the classes wide, narrow, tiny, mid; [+4] pending
// tasks; [+5] hand-ons over the queues (tasks punted behind a queued problem, entries that found no room)
#define KMAHIP_C_ADQ 24
#define KMAHIP_KBITS_MUL 0x85EBCA6Bu      // device counter words per workspace
// The status word, counters[1] of a workspace (and of the chain finder's own counter block): the kernels raise it with atomicMax, so
// the largest code of a launch is what the host reads, and clears, once the stage is synchronised (pipeline_util.h: ws_status and the
// three retries; api.hip: ws_classify; assemble.hip keeps the pile-up's codes to itself). The traceback and the pile-up never run
// between two reads of the word, so they share the value 16.
enum KmaStatus : unsigned long long {
	KMAHIP_ST_POOL = 1,             // stage 2: the library's candidate pool ran out (kmahip_ws::pool_scale doubles, the scan is repeated)
	KMAHIP_ST_CALLER_CAP = 2,       // a capacity the caller chose is too small (T_cap, ops_cap, the chain finder's record room): the needed size is reported
	KMAHIP_ST_SEED_MEMS = 3,        // stage 3a: more MEMs between a read and a template than kmahip_ws::mem_scale gives slots for
	KMAHIP_ST_TRACE_RUNS = 4,       // traceback: a read's runs outgrew the lane's buffer
	KMAHIP_ST_TRACE_DP = 8,         // traceback: a DP problem outgrew the lane's scratch
	KMAHIP_ST_TRACE_MEMS = 16,      // traceback: as KMAHIP_ST_SEED_MEMS
	KMAHIP_ST_PILE_LDS_COLS = 16,   // pile-up: the LDS did not hold a template's (or a unit's) insertion columns
	KMAHIP_ST_PILE_NODES = 32,      // pile-up: the pool of insertion columns in HBM ran out
	KMAHIP_ST_CHAIN_CAP = 40,       // chain finder: a per-read capacity ran out (chains per read, depth of the tree of covered stretches)
	KMAHIP_ST_PILE_SEG_COLS = 64,   // pile-up: a segment's insertion columns outgrew its share of the LDS
	KMAHIP_ST_PILE_TURNS = 128      // pile-up: a read goes round a template cut into units too often
};

// Probe table in HBM: open hashing over 32-byte buckets of 4 (key, position)
// slots. bucket(key) = (key * GOLD) >> (32 - nb_log2); a key lives in the first
// bucket at or after its home bucket (cyclic) that had a free slot at build
// time, so a lookup stops at the first bucket holding either the key (hit) or
// an empty slot (miss). This replaces the reference's three dependent gathers
// exist[] -> key_index[] -> value_index[] (hashmapkma.c:149-178) by one 32-byte
// gather in the common case.
struct DevDB {
	uint32_t DB_size;
	uint32_t kmersize;
	uint32_t mlen;
	uint32_t nb_log2;
	uint32_t values_u16;          // 1: values16 valid, 0: values32
	const uint2 *slots;           // (1 << nb_log2) * 4 slots of (key, gpos): gpos = one position of the k-mer in `cat`
	const uint64_t *cat;          // all templates back to back, 2 bit per base (+ pad words)
	const uint32_t *vs_id;        // per position of `cat`: value-list offset of the k-mer starting there, or
	                              // KMAHIP_EMPTY_VI where no k-mer of one template starts (its last k-1 bases)
	const int64_t *cat_off;       // DB_size + 1: first position of template t in `cat` (cat_off[DB_size] = total bases)
	const uint16_t *values16;     // [cnt, t1..tcnt] lists, offsets = value_index of the index file
	const uint32_t *values32;
	const int32_t *tlen;          // DB_size, tlen[0] = kmerindex
	const uint64_t *tseq;         // 2-bit template store (.seq.b image + pad)
	const int64_t *tseq_off;      // DB_size + 1 word offsets
	// per-template position index (replaces the lazily built HashMapCCI,
	// hashmapcci.c:470-505): linear-probing table of (kmer, val) per template;
	// val > 0: the single 1-based position of the k-mer; val < 0: -(o + 1) where
	// tpos_dups[o] = count followed by the ascending 1-based positions; val == 0
	// empty. The poly-A k-mer 0 is never indexed (hashmapcci.c:414-417).
	// presence bits of the k-mers of the probe table (small databases only, else NULL): bit ((key * KBITS_MUL) >> kbits_shift).
	// 2 MiB at most, so it stays in the 4 MiB L2 of every XCD, where a gather costs a quarter of one into the 67 MB table;
	// consulted where a miss is the likely answer (wrong-strand prefilter probes)
	const uint32_t *kbits;
	uint32_t kbits_shift;
	const uint2 *tpos_slots;
	const int64_t *tpos_off;      // DB_size + 1 slot offsets
	const uint32_t *tpos_shift;   // DB_size: 32 - log2(table size)
	const int32_t *tpos_dups;
	// everything the seeding kernel needs to know about a template in one 32-byte record (two 16-byte gathers instead of four
	// scattered ones): x = {tseq_off lo, hi, tpos_off lo, hi}, y = {tlen, tpos_shift, 0, 0}
	const uint4 *tmeta;           // 2 * DB_size
	// decontamination (kmahip_db_open_decon): 1 = the value lists may hold the pseudo-template DB_size. Nothing above has an entry
	// for that id (tlen, cat_off, tseq_off, tpos_*, tmeta all end at DB_size - 1): stage 2 scores it by id alone and takes it out of
	// every list it hands on, and every entry point that would look a listed template up refuses such a database
	uint32_t decon;
	// The list table: a second probe table over the same k-mers whose value is the k-mer's value-list OFFSET (what vs_id holds at the
	// position `slots` answers with), for the lookups that want nothing but the list: one 32-byte gather where probe() + vs_id[] are
	// two dependent ones. Same hash, same buckets of four; (1 << lb_log2) buckets, twice the probe table's unless KMAHIP_LTAB_SHIFT=0.
	// Bit 31 of a bucket's fourth value (KMAHIP_LTAB_PASSED) is set when an insertion went past the (full) bucket, so a lookup of an
	// absent key ends at the first bucket that is not full OR that no insertion passed; list offsets stay below 2^31 - 1 (else no
	// table is built). NULL: none was built (KMAHIP_SCAN_LTAB=0, no memory, offsets too large) or the launch switched it off.
	const uint2 *lslots;
	uint32_t lb_log2;
	uint32_t lpass;               // OR-ed to a full bucket's fourth value before its flag is looked at: 0, or KMAHIP_LTAB_PASSED when the
	                              // flag is to be ignored (KMAHIP_LTAB_FLAG=0: a miss ends at a bucket that is not full, as in probe())
	// The span table: per position p of `cat` (and 64 entries behind it, as vs_id) what a read that lies on `cat` from p on without a
	// mismatch scores, as far as the database alone decides it. x = t0, the template p lies in; y = need | room << 8:
	//   room  k-mer starts from p on that lie inside t0 and have a value list that names t0 (a k-mer over a template's N has none, or
	//         another template's), capped at KMAHIP_SPAN_NEVER (0 where none starts at p);
	//   need  the smallest n >= 1 for which the value lists at p .. p + n - 1, all inside `room`, have no template but t0 in common;
	//         KMAHIP_SPAN_NEVER: no such n (or the builder gave up: always safe, the item is then scanned).
	// A read of npos k-mer starts with need <= npos <= room has t0 as its only best template (scan.hip: settle_allowed has the proof).
	// NULL: none was built (KMAHIP_SCAN_SPAN=0, no memory, no diagonals to look it up by) or the launch switched the route off.
	const uint2 *span;
};
#define KMAHIP_SPAN_NEVER 255u
#define KMAHIP_SPAN_LIST_MAX 32      // the builder keeps at most this many other templates of the list at p; a longer list: never
#define KMAHIP_SPAN_SCAN_MAX 256u    // a later list of more ids than this is passed over by the builder (need comes out later, or never)
#define KMAHIP_LTAB_PASSED 0x80000000u

struct kmahip_db {
	DevDB dev;                    // device pointers
	kmahip_db_info info;
	int device;
	std::vector<void *> allocs;   // device allocations owned by the db
	// host copies needed by host-side stages
	std::vector<int32_t> h_tlen;
	std::vector<int64_t> h_cat_off;
	std::string prefix;           // index prefix (the `.name` file is read on demand by the text writers)
	std::vector<std::string> h_names;
	std::vector<uint64_t> h_tseq;     // <prefix>.seq.b, read when the `.aln` writer first asks (pipeline.hip: load_tseq)
	std::vector<int64_t> h_tseq_off;
	bool decon = false;               // opened by kmahip_db_open_decon (dev.decon says the same to the kernels)
};

// per-call scratch, grown on demand
struct kmahip_ws {
	kmahip_db *db;
	int64_t cap_reads;
	// per strand item (2 per read)
	int32_t *item_score;
	int32_t *item_n;
	int64_t *item_off;
	// candidate pool
	int32_t *pool;
	int64_t pool_cap;
	int64_t pool_scale;       // pool = cap_reads * 16 (KMAHIP_SCAN_POOL_PER_READ) * pool_scale ints; doubled after an overflow (grow_pool)
	int mem_scale;            // MEM slots per (read, template) = the usual 64 (reads up to 1 kb) x this; raised by the runs when a read
	                          // full of repeats carries more (KMAHIP_ST_SEED_MEMS, KMAHIP_ST_TRACE_MEMS), 0 = 1
	// counters (KMAHIP_N_COUNTERS): [0] pool top, [1] status, [2] n_overflow, [3] probes, [4] value elems, [5] active strands,
	// [6] hash probes, [7] pair pool top, [8] live strand items on the bare list, [9] prefilter probes, [19] records written, [20] record items settled by the prefilter, [21] records, [22] replaced diagonals, [24..29] stage 3a's class queues (KMAHIP_C_ADQ),
	// [30] k-mer starts left to the scan's queue, [31] its rounds that had any
	unsigned long long *counters;
	int64_t *overflow_items;
	int64_t *active_items;    // strand items that passed the prefilter (device-wide compaction)
	uint64_t *recs;           // the live items the scan takes as 64-byte records (scan.hip: REC_WORDS), counters[21] of them
	int64_t rec_cap;          // records the prefilter may write: cap_reads, or KMAHIP_SCAN_REC_CAP if that is less
	int stats_on;
	int timing_on;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> *events;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> *events2;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> *events3;   // prefilter kernel
	std::vector<std::pair<hipEvent_t, hipEvent_t>> *events4;   // seeding kernel
	// paired input in the default mode (kmahip_ws_set_pe_chain): singly loaded reads of a paired stream go to the chain finder
	int pe_chain_on;
	kmahip_chain_params pe_chain;
	int ck;                   // kmahip_ws_set_count_kmers: stage 2 counts k-mers (scan_count_kernel) instead of scoring a pseudo-alignment
	// paired-end stage 2
	int32_t *pool_sc, *ppool;
	void *pe_rec;
	int64_t pe_cap;
	// align stage
	int32_t *a_s32;
	uint64_t *a_s64;
	int64_t a_lanes;
	int a_mem_cap, a_ncols;
	void *a_task;
	int64_t a_task_cap;
	int *a_xq;                    // spill queues of deferred DP problems (long reads), see align.hip
	size_t a_xq_bytes;
	hipStream_t a_side;           // the general kernel over the handed-on tasks runs here, beside the class queues (align.hip)
	hipEvent_t a_ev[2];           // fork / join of that stream
	void *a_priv;             // private copies of the ConClave vectors (reduce_reads_kernel)
	int64_t a_priv_cap;
	// trace stage (3c) scratch
	int32_t *t_s32;
	uint8_t *t_E;
	int64_t t_lanes;
	int32_t *t_queue;            // reads the first trace pass put off
	int64_t t_queue_cap;
	int t_max_len, t_mem_cap;
	// what the read filter dropped, kept on request (kmahip_ws_set_trace_drops): all NULL = off
	kmahip_trace_drops t_drops;
	// pile-up stage (3c) scratch and results
	uint32_t *p_counts;
	int32_t *p_chain, *p_seg, *p_vals;
	void *p_nodes;
	uint64_t *p_keys;
	int64_t *p_rank;
	int64_t p_total, p_node_cap, p_reads_cap, p_kept, p_nodes_used, p_ent_cap;
	// what the last kmahip_assemble2_dev left for kmahip_assemble_ef_dev (assemble.hip): 0 = no pile-up, else how its columns were called
	int ef_state, ef_bcd, ef_caller, ef_sig90;
	double ef_support, ef_qstar;
	// kmahip_matvcf_gather, around its kmahip_assemble_vcf_dev calls: the VCF rows test AD against this support instead of ef_support
	// (the reference's presets leave the two apart: kmahip_shard_opts.vcf_support)
	int ef_vcf_own;
	double ef_vcf_support;
	// long-read trace pipeline (longtrace.hip): per-wavefront MEM arrays, per-pass pools, queues, scratch, counters
	void *lt_buf[20];
	size_t lt_bytes[20];
	unsigned long long lt_stats[4];   // of the last call: DP problems, DP cells, MEMs chained, reads
	unsigned long long chain_route_counts[5]; // of the last kmahip_chain_device call: reads, marked by chain_anchor_kernel, given up by chain_fast_kernel,
	                                          // taken by the long-read route, taken by chain_kernel
	unsigned long long lt_class_counts[26];   // of the last call: problems per wavefront class 0..16, then per lane class 0..8
	// slow-path dense scratch
	int32_t *dense;
	int64_t dense_slots;
	// scan workspace for CSR offsets
	int64_t *blk_sums;
	int64_t blk_cap;
	// staging for host calls
	void *stage[8];
	size_t stage_bytes[8];
};

// an anchor of the default mode's chain finder (KmerAnker, kmeranker.h:25-34): a maximal run of k-mer starts with one value list.
// Built by chain_anchor_kernel (scan.hip) or by the lane-per-read kernel of chain.hip, chained and taken apart in chain.hip.
struct KmaAnk { int score, weight, score_len, len_len; unsigned start, end; uint32_t values; int descend; };

void kmahip_set_error(const char *fmt, ...);
// The QC accumulator (qc.hip; kmahip_qc_* of kmahip.h) as the two readers feed it, always in stream order.
//   kmahip_qc_add_seq     update_QCstat (qc.c:85-104) for one counted sequence
//   kmahip_qc_add_pass    the same for a run of counted sequences whose integer sums and length histogram (512 bins at len >> res)
//                         were reduced elsewhere (s1_qc_kernel): sp[i] is added to Eeq and binned by the host's log10, in order
//   kmahip_qc_add_read    what run_input* and the head of phredStat count: sequences read with their bases, records read / kept
//   kmahip_qc_end_reader  the phred scale a reader leaves behind (runinput.c:451, 590-592, 715-717)
struct KmaQcPair { double sp; int32_t len, pad_; };
void kmahip_qc_add_seq(kmahip_qc *qc, int len, int gc, int ns, double sp);
void kmahip_qc_add_pass(kmahip_qc *qc, uint64_t count, uint64_t bp, uint64_t gc, uint64_t ns, int maxlen, const uint32_t *hist, int res,
                        const KmaQcPair *pairs, size_t n_pairs);
void kmahip_qc_add_read(kmahip_qc *qc, uint64_t org_count, uint64_t org_bp, uint64_t org_frag, uint64_t frag);
void kmahip_qc_end_reader(kmahip_qc *qc, bool paired, int phred);
// <prefix>.comp.b as read from disk (db.hip: kmahip_comp_read): keys[i] is the i-th k-mer, vidx[i] the offset of its value list in
// `values` (u16 or u32 elements: count, then the sorted template ids); n_hdr is the header's n, n the k-mers actually there
struct KmaComp {
	uint32_t DB_size = 0, mlen = 0, prefix_len = 0, tail[2] = {0, 0};      // tail: kmersize, flag
	uint64_t prefix = 0, n_hdr = 0, n = 0, v_index = 0;
	bool mega = false, u16 = false;
	std::vector<uint8_t> values;
	std::vector<uint32_t> keys, vidx;
};
int kmahip_comp_read(const std::string &comp, bool allow_sparse, KmaComp *c);
int kmahip_cmp(bool t, bool q);          // conclave.hip: the reference's `cmp` (or / and / true, kmahip_set_cmp)
// The homology counts of a sparse index build (homology.hip; `kma index -Sparse ... -hq / -ht`, qualcheck.c:81-324), over the window
// keys of index_sparse_keys_kernel as they are before any template is renumbered. Rows and columns are templates in file order.
//   kmahip_hom_open    sorts the two views of the windows; slen[t]: the windows of template t, w: prefix_len + k, min_klen: MinKlen
//   kmahip_hom_pairs   pass 1: the pairs whose thisQ / thisT reach a threshold, whatever is kept
//   kmahip_hom_best    pass 2: every row's winners over the columns with kept[j] != 0
struct KmaHom;
struct KmaHomPair { uint32_t row, jf; };                        // jf: column * 4 + (thisQ >= homQ) + 2 * (thisT >= homT)
struct KmaHomRow { uint32_t tot, jQ, num, den, jT; };           // max Scores_tot and its template; Scores, ulen and template of the max thisT (ids 1 .., 0: none)
int kmahip_hom_open(const unsigned long long *d_keys, int64_t n_keys, const int64_t *d_off, const std::vector<uint32_t> &slen, int w, int64_t min_klen, KmaHom **out);
int kmahip_hom_pairs(KmaHom *h, double homQ, double homT, bool use_t, std::vector<KmaHomPair> &pairs);
int kmahip_hom_best(KmaHom *h, const std::vector<uint8_t> &kept, std::vector<KmaHomRow> &rows);
void kmahip_hom_close(KmaHom *h);
#define HIP_TRY(expr) do { hipError_t e__ = (expr); if(e__ != hipSuccess) { \
	kmahip_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); return KMAHIP_EDEVICE; } } while(0)
// the workspace's counter block, made (and zeroed) by whichever stage runs first
static inline int kmahip_ws_counters(kmahip_ws *ws) {
	if(ws->counters) return KMAHIP_OK;
	HIP_TRY(hipMalloc((void **) &ws->counters, KMAHIP_N_COUNTERS * sizeof(unsigned long long)));
	HIP_TRY(hipMemset(ws->counters, 0, KMAHIP_N_COUNTERS * sizeof(unsigned long long)));
	return KMAHIP_OK;
}

// Proximity matching (-proxi: kmahip_params.minFrac other than 1 and -1, kma.c:708) is built for the single-end -1t1 run, stages 2
// and 3a (getProxiMatch, update_Scores). Every other entry point refuses it by name: KMAHIP_EINVAL, `what` = what is not built.
int kmahip_mem_mode();          // pipeline.hip
static inline bool kmahip_proxi_on(const kmahip_params *p) { return p->minFrac != 1.0 && p->minFrac != -1.0; }
static inline int kmahip_refuse_proxi(const kmahip_params *p, const char *what) {
	if(!p || !kmahip_proxi_on(p)) return KMAHIP_OK;
	kmahip_set_error("proximity matching (minFrac %g) serves the single-end -1t1 run, not %s", p->minFrac, what);
	return KMAHIP_EINVAL;
}
// Forced pairing (kmahip_params.apm: 2 in bits 0-1, or 3 in bits 4-5) has its stage 2 only (kmahip_scan_pe): stage 3a would run
// penalty pairing on its couples, not alnFragsForcePE
static inline int kmahip_refuse_forced_pairing(const kmahip_params *p) {
	if(!p || ((p->apm & 3) != 2 && ((p->apm >> 4) & 3) != 3)) return KMAHIP_OK;
	kmahip_set_error("forced pairing (apm %d) is built for kmahip_scan_pe only: stage 3a (alnFragsForcePE) is not", (int) p->apm);
	return KMAHIP_EINVAL;
}
// Decontamination (a database opened by kmahip_db_open_decon) is built for stage 2 of the one-rank -1t1 runs, where the filter sits
// (scan.hip: decon_filter). Every other entry point that reads value lists refuses such a database by name: it would hand the
// pseudo-template DB_size on, or run without the filter
static inline int kmahip_refuse_decon(const kmahip_db *db, const char *what) {
	if(!db || !db->decon) return KMAHIP_OK;
	kmahip_set_error("decontamination (a database opened with its .decon.comp.b) serves the one-rank -1t1 runs, not %s", what);
	return KMAHIP_EINVAL;
}
#define KMAHIP_DECON_CHAIN "the default mode's chain finder (the reference's reads template_lengths[DB_size] there, past the array's end)"
#define KMAHIP_DECON_MEM "-mem_mode (the reference's reads template_lengths[DB_size] there, past the array's end)"
#define KMAHIP_DECON_MT1 "the -Mt1 run (it scans no k-mers)"
#define KMAHIP_DECON_SHARD "the sharded runs"
#define KMAHIP_PROXI_PE "paired reads (getSecondProxiPen, getF_Proxi / getR_Proxi and the minFrac branches of alnFragsUnionPE / alnFragsPenaltyPE are not built)"
#define KMAHIP_PROXI_CHAIN "the default mode's chain finder (getProxiChainTemplates is not built)"
#define KMAHIP_PROXI_MT1 "the -Mt1 run"
#define KMAHIP_PROXI_MEM "-mem_mode (the soft-proximity vector of the S2 stream is not built)"
#define KMAHIP_PROXI_SHARD "the sharded runs"

int kmahip_launch_scan_se(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads,
                          const kmahip_params *p, kmahip_cands *out, hipStream_t stream);
int kmahip_launch_align_se(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_cands *cands,
                           const kmahip_params *p, kmahip_hits *out, hipStream_t stream);
int kmahip_launch_trace(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *flag, const int32_t *tmpl,
                        const uint8_t *tmpl_ok, const kmahip_params *p, kmahip_traces *out, hipStream_t stream);
int kmahip_trace_reserve(kmahip_ws *ws, int max_len, int64_t n);          // align.hip: the traceback scratch, ahead of time
int kmahip_launch_longtrace(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *tmpl, int tmpl_all, const int32_t *rc_in,
                            const uint8_t *tmpl_ok, int one2one, const kmahip_params *p, kmahip_traces *out, int32_t *rc_out, hipStream_t stream, int score_mode = 0);
// anchors of every strand that passes the prefilter, for reads without N's and up to 288 k-mer starts (the others get slow[read] = 1):
// a_n[2 r + strand] anchors at pool + a_off[2 r + strand]; cnt[0] = anchors written (may exceed pool_cap: repeat with a larger pool)
// the fragment rows of a run whose items (reads, records, fragments) and headers are in HBM: ordered, measured and formatted on the
// device, compressed and written by the host's threads (session.hip)
int kmahip_frag_write_dev(kmahip_db *db, const kmahip_reads *W, const char *d_names, const int64_t *d_name_off, const int64_t *d_name_idx, const int32_t *d_rc,
                          const int32_t *d_tmpl, const int32_t *d_nhits, const int32_t *d_stats, const int64_t *d_rank, int64_t max_frag, const char *path,
                          int64_t text_chunk, char **pinned, int64_t *n_rows_out, int order = 0, struct KmaFragSink *sink = nullptr);
// a fragment file that stays open over several kmahip_frag_write_dev calls (each appends its rows; kmahip_frag_sink_close ends the file):
// the compressing threads go on with a call's text after the call has returned, in the caller's three pinned buffers (`pinned` is then
// required, and the same for every call)
struct KmaFragSink;
KmaFragSink *kmahip_frag_sink_open(const char *path);
int kmahip_frag_sink_close(KmaFragSink *sink);

// the SAM rows of a run whose items and headers are in HBM (samout.hip): classified, ordered, measured and formatted on the device, written
// to `fd` in order as the chunks of text come back. Everything in KmaSamIn is a DEVICE pointer; W->n_reads items.
struct KmaSamIn {
	const kmahip_reads *W;
	const char *d_names;
	const int64_t *d_name_off, *d_name_idx;          // d_name_idx (or NULL): the header an item carries
	const int32_t *d_rc, *d_tmpl, *d_nhits, *d_flag;
	const kmahip_traces *tr;
	const kmahip_trace_drops *drops;                 // NULL: no rows of class 3b
	const uint8_t *d_ok;                             // per template, NULL = all
	const int64_t *d_rank;                           // position among the filed items of the whole stream, NULL = counted here
	int64_t max_frag;
	int order, level;
};
int kmahip_sam_write_dev(kmahip_db *db, const KmaSamIn *in, int fd, int64_t text_chunk, char **pinned, int64_t *rows_out, int64_t class_rows[5]);
int kmahip_sam_open(const char *path, bool append);          // a descriptor for kmahip_sam_write_dev ("-": standard output), -1 on failure
int kmahip_sam_close(int fd);

// stage 2 of the default mode on a batch that is in HBM, its records as a batch of their own in stream order (pipeline.hip). The
// arrays live in a block of their own until kmahip_chain_records_free.
struct KmaChainRecs {
	int64_t m = 0, n_T = 0;
	kmahip_reads d{};              // the records: the read, or its reverse complement where the record prints that; q_start / q_end set
	kmahip_cands c{};              // their template lists
	int64_t *o_read = nullptr;     // the read of the batch a record comes from
	int32_t *o_emit = nullptr;     // 1 = the record holds the reverse complement
	void *block = nullptr;
};
int kmahip_chain_records_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *dR, const kmahip_params *p, const kmahip_chain_params *cp, KmaChainRecs *out);
void kmahip_chain_records_free(KmaChainRecs *r);

int kmahip_launch_chain_anchors(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p, KmaAnk *pool, int64_t pool_cap,
                                int64_t *a_off, int32_t *a_n, uint8_t *slow, unsigned long long *cnt, hipStream_t stream);
int kmahip_db_load_names(kmahip_db *db);       // fragout.hip: fills db->h_names from <prefix>.name
double kmahip_p_chisqr(long double q);      // stdstat.c:136-147 (conclave.hip)

// `-ConClave 2` (conclave.hip): the runs ask which version is set (kmahip_set_conclave_version) and, for 2, hand the records of their
// stream over in parts (the batches of a session; anything else is one part). Everything is a DEVICE pointer.
int kmahip_conclave_version();
int kmahip_refuse_conclave2(const char *what);          // KMAHIP_EINVAL by name where version 2 is set (the sharded runs), else KMAHIP_OK
struct KmaCC2Part {
	int pe;                                  // as CCArgs.pe: 0 single-end reads, 1 record slots of kmahip_align_pe_dev, 2 explicit records
	int64_t n;                               // slots
	const int32_t *len, *len2, *mate, *pe_kind;
	const int64_t *off;
	const kmahip_hits *hits;                 // n_hits, best_score, tmpl, start, end
	int32_t *o_tmpl, *o_start, *o_end;       // per slot
	const int32_t *seed;                     // per slot (kmahip_cc2_seeds)
};
// as / us: stage 3a's two vectors (read only); tot: the per-template outputs (w_scores is set, the others are added to)
int kmahip_conclave2_parts(kmahip_db *db, const KmaCC2Part *parts, int n_parts, const uint64_t *as, const uint64_t *us, const kmahip_conclave *tot,
                           double evalue, double scoreT, hipStream_t stream);
// seed[s] for slot s = read src[s * src_stride] (src NULL: read s; < 0: none) of batch a, or of b where the index is >= n0 (b NULL: a
// alone), reverse complemented where rc[s * rc_stride] & 1 (rc NULL: as stored)
int kmahip_cc2_seeds(const kmahip_reads *a, const kmahip_reads *b, int64_t n0, int64_t n_slots, const int32_t *src, int src_stride, const int32_t *rc, int rc_stride,
                     int32_t *seed, hipStream_t stream);
int kmahip_launch_scan_pe(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p,
                          kmahip_pe_recs *out, hipStream_t stream);
int kmahip_launch_align_pe(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_pe_recs *recs,
                           const kmahip_params *p, kmahip_hits *out, int32_t *pe_kind, hipStream_t stream);

// the paired run on a batch that is in HBM already (session.hip -> pipeline.hip): batch->reads holds DEVICE arrays (sizes and
// max_len as usual), batch->pair the host's mate flags; the headers and the fragment writer's pinned text buffers are these
struct KmaPeDev {
	const char *d_names;
	const int64_t *d_name_off;
	char **h_text;
	int64_t text_chunk;
	int64_t *frag_rows;       // out: rows written to the fragment file (may be NULL)
	int sam_level, sam_fd;    // SAM records of the filed fragments: the value of -sam (0: none) and the descriptor they go to
	struct KmaEfReq *ef;      // the extended features of the run (or NULL): filled behind the pile-up
	struct KmaMatVcf *mv;     // the count matrix and the VCF records of the run (or NULL): gathered behind the pile-up
};
// what a run gathers for the `.mapstat` file: HOST vectors of DB_size entries, ConClave's two counts and kmahip_assemble_ef_dev's figures
struct KmaEfReq {
	uint32_t *read_counts, *frag_counts;
	kmahip_assembly_ef *out;
};
// ... and what the writer of `.res` needs to write the file beside it, a row where it writes one (kmahip_write_res_fsa)
struct KmaMapstat {
	const char *path, *t_db, *cmdline;
	uint32_t fragments;          // `## fragmentCount`
	const uint32_t *read_counts, *frag_counts;
	const kmahip_assembly_ef *ef;
};
// the count matrix and the VCF file (-matrix, -vcf [n]): what a run gathers behind the pile-up for the templates whose `.res` row passes
// its gate (kmahip_matvcf_gather, pipeline.hip: kmahip_assemble_matrix_dev / kmahip_assemble_vcf_dev), and what the writer of `.res`
// needs to write <out>.mat.gz and <out>.vcf.gz from its own loop (kmahip_write_res_fsa)
struct KmaMatVcf {
	bool matrix = false;
	int vcf = 0;                 // the value of -vcf (0: no file, 2: the FILTER column is filled)
	std::string mat_path, vcf_path, t_db;
	double evalue = 0, support = 0, ID_t = 1.0, Depth_t = 0;
	int bcd = 1;
	std::vector<char> mat_text;          // the rows of template t: mat_text[mat_off[t] .. mat_off[t + 1])
	std::vector<int64_t> mat_off;
	std::vector<kmahip_vcf_rec> recs;    // the records of template t: recs[rec_off[t] .. rec_off[t + 1])
	std::vector<int64_t> rec_off;
};
int kmahip_matvcf_gather(kmahip_db *db, kmahip_ws *ws, const kmahip_res_row *rows, int64_t n_rows, const kmahip_assembly *a, KmaMatVcf *mv);
int kmahip_run_pe_resident(kmahip_db *db, kmahip_ws *ws, const kmahip_read_batch *batch, const KmaPeDev *pd, const kmahip_params *p, double evalue, int bcd,
                           int64_t max_frag, const char *frag_path, kmahip_run *out);
