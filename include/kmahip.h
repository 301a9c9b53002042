/* kmahip.h -- C ABI of libkmahip.so: the MI355X (gfx950) implementation of KMA's
 * seed-and-extend mapping core (stage 2 "k-mer scan" and stage 3a "alignment
 * score"), batched.  Plain C types only; every function returns 0 on success or
 * a negative KMAHIP_E* code (never exit()s; the reference's ERROR() ->
 * exit(errno) convention, pherror.h:27, is left to the calling host program).
 *
 * What each entry point replaces in the reference (file:line into KMA 1.5.1):
 *   kmahip_db_open            hashMapKMA_load           hashmapkma.c:275-455
 *                             load_DBs_KMA + seq_indexes runkma.c:160-220
 *                             alignLoad_fly/hashMapCCI_load (lazy per template)
 *                                                        hashmapcci.c:470-505,616
 *   kmahip_scan_se[_dev]      save_kmers_batch body:    kmers.h:22, kmers.c:51-290
 *                             worker loop save_kmers_threaded savekmers.c:94-271
 *                             with kmerScan = save_kmers (savekmers.h:50,
 *                             savekmers.c:2442-3065) and hashMap_get
 *                             (hashmapkma.h:59, hashmapkma.c:149-178); the
 *                             result arrays carry the S2 record fields that
 *                             print_ankers writes (ankers.c:30-50)
 *   kmahip_align_se[_dev]     alnFrags_threaded body (alnfrags.c:2150-2294) with
 *                             alnFragsSE (alnfrags.c:1052-1218): KMA_score
 *                             (align.h:33, align.c:509-748), chainSeeds
 *                             (chain.h:39, chain.c:79-260), NW_score /
 *                             NW_band_score (nw.h:62-63, nw.c:642-1188),
 *                             update_Scores (updatescores.c:203-298)
 *   kmahip_map_se             both of the above on one staged batch (host buffers)
 *   kmahip_allreduce_scores   (new) SUM of alignment_scores/uniq_alignment_scores
 *                             across read shards before runConClave
 *                             (runkma.c:563-594); see INTEGRATION.md
 *
 * Ownership: the caller owns every host and device buffer it passes in; the
 * library owns the database image in HBM and its private workspaces.
 * Threading: one kmahip_db may be used from several host threads as long as
 * each call uses its own kmahip_ws (workspace) and stream.
 */
#ifndef KMAHIP_H
#define KMAHIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMAHIP_OK            0
#define KMAHIP_EINVAL       -1  /* bad argument */
#define KMAHIP_EIO          -2  /* cannot read an index file */
#define KMAHIP_EFORMAT      -3  /* index variant not supported (megamap, k>16 keys, flag!=0) */
#define KMAHIP_ENOMEM       -4  /* host or device allocation failed */
#define KMAHIP_EDEVICE      -5  /* HIP runtime error (see kmahip_last_error) */
#define KMAHIP_EOVERFLOW    -6  /* an output capacity given by the caller was too small */

typedef struct kmahip_db kmahip_db;
typedef struct kmahip_ws kmahip_ws;

/* scoring constants: Penalties, penalties.h:22-33 (d is the 5x5 substitution
 * matrix built at kma.c:1307-1328) */
typedef struct kmahip_rewards {
	int32_t M, MM, U, W1, Wl, Mn, PE;
	int32_t d[5][5];
} kmahip_rewards;

/* run parameters (the subset of kma.c flags the path reads) */
typedef struct kmahip_params {
	kmahip_rewards rw;
	int32_t exhaustive;   /* -ex_mode */
	int32_t minlen;       /* -ml, default 16 */
	int32_t mq;           /* -mq, default 0 */
	double scoreT;        /* -mrs, default 0.5 */
	double mrc;           /* -mrc, default 0.0 */
	double minFrac;       /* -proxi, default 1.0 (1 and -1: off); -1 <= minFrac <= 1. Proximity matching in the single-end -1t1 run: stage 2 hands on every
	                       * template of a strand whose k-mer score reaches (int) (|minFrac| * best) (getProxiMatch savekmers.c:296-340), stage 3a keeps a hit
	                       * when aln_len * (|minFrac| * best normalised score) <= score or |minFrac| * best read score <= score and adds the best read
	                       * score (minFrac > 0) or the hit's own (minFrac < 0) to alignment_scores (update_Scores updatescores.c:235-272). Every other entry
	                       * point -- paired reads, kmahip_scan_chain and the chain runs, -Mt1, the sharded runs, anything under kmahip_set_mem_mode(1) --
	                       * returns KMAHIP_EINVAL for it */
	int32_t ts;           /* -ts, default 0: the traceback aligner trims this many bases off the front of every seed of the best chain but
	                       * the first one when that starts the read (trimSeeds chain.c:493-528, called by KMA() align.c:413; KMA_score
	                       * has no such step); at least one base of a seed remains */
	int32_t apm;          /* paired reads: 0 = the pairing penalty of -apm p (save_kmers_penaltyPair savekmers.c:3572, alnFragsPenaltyPE
	                       * alnfrags.c:1596), 1 = union, -apm u and what `-ipe` means without -apm (kma.c:206: save_kmers_unionPair
	                       * savekmers.c:3367 with getF_Best / getR_Best, alnFragsUnionPE alnfrags.c:1220). The reference can set the two
	                       * stages apart (-pm x: save_kmers_pair only, -fpm x: alnFragsPE only, kma.c:437-465): bits 0-1 = stage 2 as
	                       * above, bits 4-5 = stage 3a + 1 (0: the same as stage 2, 1: p, 2: u). Stage 2 also takes 2 = forced pairing
	                       * (-apm f / -pm f: save_kmers_forcePair savekmers.c:3779 with getFirstForce / getSecondBestForce -- a couple on the
	                       * templates both mates hit on opposite strands at the best summed score, or no record at all) -- for kmahip_scan_pe
	                       * only: stage 3a of forced pairing (alnFragsForcePE) is not built, and the paired stage-3a, run and session entry points return
	                       * KMAHIP_EINVAL for it (2 in bits 0-1, or 3 in bits 4-5) */
	int32_t ca;           /* -ca, default 0: circular alignments. 0 = the seeds of stage 3a and of every traceback are chained by chainSeeds
	                       * (chain.c:79), non-zero = by chainSeeds_circular (chain.c:262, chosen at kma.c:722): a chain may go on across the
	                       * template's origin, the alignment then ends before it starts (end < start in the fragment row). Stage 2 does not
	                       * read it */
} kmahip_params;

typedef struct kmahip_db_info {
	uint32_t DB_size;     /* templates + 1 (ids are 1-based) */
	uint32_t kmersize;
	uint64_t n_kmers;     /* distinct k-mers */
	uint64_t n_values;    /* elements in the value-list array */
	uint64_t hash_bytes;  /* bytes of the probe table in HBM */
	uint64_t total_bytes; /* all DB bytes resident in HBM */
	uint64_t tseq_words;  /* 2-bit template store, u64 words */
} kmahip_db_info;

/* A batch of 2-bit packed reads (CompDNA, compdna.h:23-30), CSR layout.
 * seq: u64 words, 32 bases per word MSB-first, N packed as A; each read is
 * followed by at least one readable pad word (getKmer_macro reads word+1,
 * stdnuc.h:27-30).  N: sorted N positions.  All pointers are HOST pointers for
 * the plain calls and DEVICE pointers for the *_dev calls. */
typedef struct kmahip_reads {
	int64_t n_reads;
	const uint64_t *seq;
	const int64_t *seq_off;   /* n_reads+1 word offsets */
	const int32_t *len;       /* n_reads */
	const int32_t *N;
	const int64_t *N_off;     /* n_reads+1 */
	int64_t seq_words;        /* total words in seq (host calls: bytes to stage) */
	int64_t N_total;
	int32_t max_len;          /* longest read in the batch (sizes the align scratch) */
	/* optional (NULL: whole reads): query bounds per read, [q_start[i], q_end[i]) in the coordinates of the read as stored --
	 * what a default-mode S2 record carries behind its header (qseqs.c:41-56). Stage 3a and the traceback look for seeds only
	 * from q_start on and let the last N-free stretch end at q_end (KMA_score align.c:534-540, KMA :249-254, anker_rc_comp
	 * :1029-1044; for a view of the reverse strand the bounds count from the other end, alnfrags.c:1113-1127). Same memory
	 * space as the other arrays of the call. */
	const int32_t *q_start;
	const int32_t *q_end;
} kmahip_reads;

/* Stage-2 result, one entry per read = the S2 record fields (ankers.c:30-50):
 * rc_flag = +-best k-mer score (negative: both strands tie), flag = 0 | 16
 * (16: the reverse-complemented read is the one passed on), T = candidate
 * template ids (negative id: reverse strand entry of a tie). Reads the
 * reference would not emit have T_off[i+1] == T_off[i]. */
typedef struct kmahip_cands {
	int32_t *rc_flag;     /* n_reads */
	int32_t *flag;        /* n_reads */
	int64_t *T_off;       /* n_reads + 1 */
	int32_t *T;           /* T_cap */
	int64_t T_cap;
} kmahip_cands;

/* Stage-3a result (what update_Scores keeps, updatescores.c:203-298 = one
 * frag_raw record per read).  Hits of read i are stored at
 * [T_off[i], T_off[i] + n_hits[i]) of tmpl/score/start/end, in candidate order,
 * so these arrays need the same capacity as kmahip_cands.T.  Reads whose two
 * strands tied in stage 2 (rc_flag < 0) get their strand per template from MEM
 * coverage (anker_rc_comp, align.c:993-1176); a negative tmpl = reverse strand.
 * alignment_scores / uniq_alignment_scores are the two u64[DB_size] ConClave
 * vectors (updatescores.c:228,276); the call ADDS into them (caller zeroes). */
typedef struct kmahip_hits {
	int32_t *n_hits;      /* n_reads */
	int32_t *best_score;  /* n_reads: best_read_score */
	int32_t *flag;        /* n_reads: stage-2 flag, |= 4 when unmapped after alignment */
	int32_t *tmpl;        /* signed template id */
	int32_t *score;
	int32_t *start;
	int32_t *end;
	uint64_t *alignment_scores;       /* DB_size, may be NULL */
	uint64_t *uniq_alignment_scores;  /* DB_size, may be NULL */
	int32_t *rc;          /* n_reads (records), may be NULL. bit 0: the fragment update_Scores* files for this record is the
	                       * reverse complement of the ORIGINAL read (single end: stage 2's flag & 16; paired: a pair with a
	                       * reverse-strand candidate is turned and only turned back, flag toggled, when its first kept template
	                       * is positive, alnfrags.c:1629-1643, 1807-1822 -- the flag alone does not tell). bit 1 (proper pairs):
	                       * the second slot's fragment is written first (alnfrags.c:1807-1812). Input of the stage-3c calls. */
} kmahip_hits;

/* Stage-2 result for paired reads (`-ipe ... -apm p`): two record slots per pair, in the order the
 * reference writes them to the S2 stream (printPair / deConPrintPtr, savekmers.c:3609-3737, ankers.c:150-160).
 * mate[r] = -1: slot not written; else 0/1 = which mate of the pair the record carries. rc[r] = 1: its
 * reverse complement is the sequence passed on. rc_flag / flag / T as in kmahip_cands; a properly paired
 * couple is "first record with an empty list (flag & 2), second record with the shared list". */
typedef struct kmahip_pe_recs {
	int32_t *mate;        /* 2 * n_pairs */
	int32_t *rc;
	int32_t *rc_flag;
	int32_t *flag;
	int64_t *R_off;       /* 2 * n_pairs + 1 */
	int32_t *T;
	int64_t T_cap;
} kmahip_pe_recs;

void kmahip_default_params(kmahip_params *p);
const char *kmahip_last_error(void);

/* device selection: one process per GPU (LOCAL_RANK), call before db_open */
int kmahip_init(int device);

int kmahip_db_open(const char *prefix, kmahip_db **out);
/* Decontamination (`kma ... -deCon`, kmers.c:76-80): the same database read from <prefix>.decon.comp.b (KMAHIP_EIO, naming the file,
 * when it is missing). Its value lists hold the pseudo-template DB_size where a k-mer is also the contamination's. Stage 2 scores it
 * like any template and then takes it out of every final list (deConPrint / deConPrintPair, ankers.c:74-148): a read whose list
 * empties has no record, and no list that leaves kmahip_scan_se[_dev] / kmahip_scan_pe[_dev] holds +-DB_size. Served by the one-rank
 * -1t1 entry points (single end, also with proximity matching; paired at apm p / u / f); the default mode's chain finder, -mem_mode,
 * the -Mt1 run and the sharded entry points refuse such a database with KMAHIP_EINVAL, by name. */
int kmahip_db_open_decon(const char *prefix, kmahip_db **out);
int kmahip_db_is_decon(const kmahip_db *db);          /* 1: opened by kmahip_db_open_decon, 0: not (or NULL) */
void kmahip_db_close(kmahip_db *db);
int kmahip_db_get_info(const kmahip_db *db, kmahip_db_info *info);

int kmahip_ws_create(kmahip_db *db, kmahip_ws **out);
void kmahip_ws_destroy(kmahip_ws *ws);

/* Stage 2, single-end `-1t1`.  Host buffers in, host buffers out (PCIe
 * inclusive).  Returns KMAHIP_EOVERFLOW if T_cap is too small; T_off[n] then
 * holds the needed capacity. */
int kmahip_scan_se(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads,
                   const kmahip_params *p, kmahip_cands *out);
/* Same with everything resident in HBM; asynchronous on `stream`
 * (a hipStream_t, NULL = default stream). */
int kmahip_scan_se_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads,
                       const kmahip_params *p, kmahip_cands *out, void *stream);
/* Stage 2, paired end with pairing penalty (`-apm p`): save_kmers_pair = save_kmers_penaltyPair
 * (savekmers.h:51, savekmers.c:3572-3777) with get_kmers_for_pair (:427-688). reads = mates interleaved
 * (read 2i = mate 1, 2i+1 = mate 2 of pair i). *_dev: device pointers, asynchronous on `stream`. */
int kmahip_scan_pe(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p, kmahip_pe_recs *out);
int kmahip_scan_pe_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p,
                       kmahip_pe_recs *out, void *stream);

/* Stage 3a for the records of kmahip_scan_pe_dev (device pointers): alnFragsPE = alnFragsPenaltyPE
 * (alnfrags.h:68, alnfrags.c:1596-1972) for proper couples (first record with an empty list, second with the
 * shared candidates), alnFragsSE for records written singly; update_Scores_pe / update_Scores_se
 * (updatescores.c:300-488). The per-record arrays of `out` have 2 * n_pairs entries; pe_kind[pair] = 0 records
 * handled singly / nothing, 1 proper pair, 2 unmated pair, 3 first record only, 4 second record only. Hits of a
 * couple are stored in the SECOND record's slice [R_off[2p+1], ...): kind 1: n_hits shared by both records;
 * kind 2: the first record's n_hits[2p] hits followed by the second's n_hits[2p+1]; kind 3/4: that record's. */
int kmahip_align_pe_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_pe_recs *recs,
                        const kmahip_params *p, kmahip_hits *out, int32_t *pe_kind, void *stream);
/* Stages 2 + 3a for paired reads with host buffers in and out. */
int kmahip_map_pe(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p,
                  kmahip_pe_recs *recs_out, kmahip_hits *hits_out, int32_t *pe_kind);

/* Stage 3a, single end: alignment score of every (read, candidate) pair,
 * per-read hit selection and ConClave accumulators.  `cands` is the output of
 * kmahip_scan_se_dev on the same `reads` (device pointers). */
int kmahip_align_se_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_cands *cands,
                        const kmahip_params *p, kmahip_hits *out, void *stream);
/* Stages 2 + 3a with host buffers in and out (reads staged once). */
int kmahip_map_se(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p,
                  kmahip_cands *cands_out, kmahip_hits *hits_out);

/* Stage 3b, ConClave (runConClave, conclave.c:43-215, `-ConClave 1`): ONE template per frag_raw record, chosen from the
 * templates the read aligned equally well to by (alignment_scores, alignment_scores / template_length,
 * uniq_alignment_scores, smaller id). Inputs are the outputs of kmahip_align_se_dev / kmahip_align_pe_dev (device
 * pointers; with several GPUs AFTER kmahip_allreduce_scores). Per record slot (SE: read i; PE: record slot r, a proper
 * pair being the record of its second slot): the chosen signed template (0 = nothing written for the slot), its start
 * and end. Per template, ADDED into caller-zeroed vectors: w_scores (the Score column of `.res`, conclave.c:147),
 * fragment / read counts (:148-151, 172-174) and the summed read lengths (Depth under `-sasm`, assembly.c:1280).
 * With several GPUs these four are summed over ranks afterwards (kmahip_allreduce_scores takes any
 * two u64 vectors). */
typedef struct kmahip_conclave {
	int32_t *tmpl;               /* n slots */
	int32_t *start;
	int32_t *end;
	uint64_t *w_scores;          /* DB_size */
	uint32_t *fragment_counts;   /* DB_size, may be NULL */
	uint32_t *read_counts;       /* DB_size, may be NULL */
	uint64_t *depth;             /* DB_size, may be NULL */
} kmahip_conclave;
int kmahip_conclave_se_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_cands *cands,
                           const kmahip_hits *hits, kmahip_conclave *out, void *stream);
int kmahip_conclave_pe_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_pe_recs *recs,
                           const kmahip_hits *hits, const int32_t *pe_kind, kmahip_conclave *out, void *stream);
/* the same with host buffers in and out (only reads->n_reads / len are used of `reads`; the per-template vectors of
 * `out` are read, added to and written back) */
int kmahip_conclave_se(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_cands *cands,
                       const kmahip_hits *hits, kmahip_conclave *out);
int kmahip_conclave_pe(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_pe_recs *recs,
                       const kmahip_hits *hits, const int32_t *pe_kind, kmahip_conclave *out);
/* The general form, host buffers: one entry per frag_raw record IN STREAM ORDER, exactly the fields runConClave reads
 * (conclave.c:59-70): hits->n_hits[r] listed templates at off[r] of tmpl / start / end, hits->best_score[r] = stats[2]
 * (negative: a pair record, the mate of length q_len2[r] follows), q_len[r]. off has n_records + 1 entries; q_len2 may be
 * NULL. For glue that merges single and paired results of one input stream: a record whose list is empty takes the first
 * listed hit of the record before it (the reference reads zero entries into buffers it does not clear). */
int kmahip_conclave_records(kmahip_db *db, kmahip_ws *ws, int64_t n_records, const int32_t *q_len, const int32_t *q_len2,
                            const int64_t *off, const kmahip_hits *hits, kmahip_conclave *out);
/* ... with DEVICE pointers, asynchronous on `stream`; `off` needs n_records entries only (a record with n_hits 0 and
 * score 0 is an unused slot: ConClave passes over it) */
int kmahip_conclave_records_dev(kmahip_db *db, kmahip_ws *ws, int64_t n_records, const int32_t *q_len, const int32_t *q_len2,
                                const int64_t *off, const kmahip_hits *hits, kmahip_conclave *out, void *stream);

/* The columns of a `.res` row that do not depend on the consensus (runkma.c:765-783, 809): Score, Expected (as printed,
 * (unsigned) expected), Template_length, q_value, p_value, and whether the template passes the reference's gate for
 * assembly / output (cmp_or(p <= evalue && score > expected, score >= scoreT * length), stdstat.c:23-27). One row per
 * template with w_scores > 0, in template order; w_scores is a HOST vector (summed over ranks). kma.c:312,319:
 * evalue = 0.05, scoreT = 0.5. Returns KMAHIP_EOVERFLOW with *n_rows = needed when cap is too small. */
typedef struct kmahip_res_row {
	int32_t template_id;
	int32_t template_length;
	uint64_t score;
	uint32_t expected;
	int32_t significant;
	double q_value;
	double p_value;
} kmahip_res_row;
/* How a template's p-value test and its score test combine into `significant` -- the reference's `cmp` pointer (stdstat.c:23-35,
 * kma.c:915-920): 0 = or (default), 1 = and (`-and`), 2 = always true (`-oa`, which also sets -ID and -md to 0). One setting per
 * process, read by kmahip_res_rows and by every run entry point (runkma.c:783, mt1.c:419). */
int kmahip_set_cmp(int mode);
/* `-lc` outside the chain finder: ConClavePtr = runConClave_lc (kma.c:694-701, conclave.c:215-385) -- among a read's equally good
 * templates the ConClave score per template base decides before the score itself. One setting per process; every ConClave entry
 * point reads it. (The chain finder's length-corrected helpers, kmeranker.c:37-55, 432-510, are not built: -lc needs -1t1.) */
int kmahip_set_conclave_lc(int on);
/* `-mem_mode` (runKMA_MEM instead of runKMA, kma.c:1619-1623, runkma.c:910-1250): ConClave is based on the template finder's own
 * scores -- a stage-2 record is the frag_raw record (its templates as the hits, each spanning its template, the k-mer score as the
 * read score; update_Scores_MEM updatescores.c:31-67), no alignment happens before ConClave; stage 3c aligns every read against the
 * template ConClave gave it as ever. A couple of a paired stream -- a first record without a list, then its mate with the templates --
 * is one record with both scores added up (update_Scores_pe_MEM :69-107, runkma.c:1090-1134). One setting per process, read by the
 * whole-run entry points (kmahip_run_se / _pe / _chain, the sessions, the sharded runs). */
int kmahip_set_mem_mode(int on);
/* `-ConClave n` (kma.c:493-501, runkma.c:588-594): 1 = runConClave (the default), 2 = runConClave2 / runConClave2_lc
 * (conclave.c:386-1110); anything else returns KMAHIP_EINVAL. One setting per process, read by the whole-run entry points of one rank
 * (kmahip_run_se / _pe / _chain, the sessions); the sharded runs return KMAHIP_EINVAL under version 2 (the vectors of its first and
 * third pass would have to be summed over the ranks). `-Mt1` runs no ConClave and ignores it. The stage entry points say which
 * scheme they are by their names: kmahip_conclave_* is version 1, kmahip_conclave2_* version 2, whatever is set here. */
int kmahip_set_conclave_version(int v);
/* Stage 3b, ConClave version 2 (runConClave2, conclave.c:386-747; with kmahip_set_conclave_lc, runConClave2_lc :749-1110), the general
 * record form of kmahip_conclave_records: the same records, and per record q_seed[r], the value of `rand` behind the seven-step loop
 * over the first and last seven bases of the record's first sequence (conclave.c:566-571; read only where q_len[r] >= 16). Four
 * passes: every record's best-of-list template collects its score (:404-466); templates that fail the test of `.res` on those sums
 * are dropped (:469-491, host arithmetic with evalue, scoreT and kmahip_set_cmp: one vector goes to the host and comes back); a record
 * with several templates of which one survived adds its score to that template's unique score (:493-532); a record with several
 * templates draws one in proportion to the unique scores, or takes the best of its list where they are all 0, the sequence is
 * shorter than 16 or nothing was drawn (:534-743). Outputs as kmahip_conclave_records, except that out->w_scores is SET, not
 * added to (:535); hits->uniq_alignment_scores is not changed (the third pass adds into a copy). A sum of unique scores that wraps
 * a 32-bit int negative is undefined in the reference (:580): nothing is claimed for it. */
int kmahip_conclave2_records(kmahip_db *db, kmahip_ws *ws, int64_t n_records, const int32_t *q_len, const int32_t *q_len2,
                             const int64_t *off, const int32_t *q_seed, const kmahip_hits *hits, double evalue, double scoreT,
                             kmahip_conclave *out);
/* ... with DEVICE pointers on `stream`; returns when the four passes are done (the host step in the middle waits for the first) */
int kmahip_conclave2_records_dev(kmahip_db *db, kmahip_ws *ws, int64_t n_records, const int32_t *q_len, const int32_t *q_len2,
                                 const int64_t *off, const int32_t *q_seed, const kmahip_hits *hits, double evalue, double scoreT,
                                 kmahip_conclave *out, void *stream);
int kmahip_res_rows(const kmahip_db *db, const uint64_t *w_scores, double evalue, double scoreT,
                    kmahip_res_row *rows, int64_t cap, int64_t *n_rows);

/* Stage 3c, per read: the traceback aligner KMA() (align.c:214-507 with NW / NW_band, nw.c:26-640) for every read that
 * ConClave filed under a template, followed by assemble_KMA's read filter (assembly.c:1931-1961: + Wl for an alignment
 * that starts at the first / ends at the last template base, minlen, mrc, scoreT). This is what the reference prints per
 * read in `.frag.gz` / SAM and feeds to alnToMat.
 *   rc[i]     kmahip_hits.rc of the read's record (bit 0: the filed fragment is the reverse complement of reads[i])
 *   tmpl[i]   kmahip_conclave.tmpl (signed; 0 = read has no template)
 *   tmpl_ok   per template, 1 = assemble (kmahip_res_row.significant); NULL = all
 * Out per read: stats[10 * i ..] = score, start, end, aln_len, clip_start, clip_end, match, tGaps, qGaps, mapQ (all 0: the
 * read was dropped); the alignment columns as n_ops[i] runs at ops[ops_off[i] ..], each (length << 2) | class with class
 * 0 '=' (match), 1 'X' (mismatch), 2 'I' (gap in template), 3 'D' (gap in read) -- the classes of makeCigar (sam.c:57-78).
 * The SAM CIGAR is clip_start 'S' + runs + clip_end 'S'; POS = start + 1; AS = score. Runs are appended in no particular
 * read order. KMAHIP_EOVERFLOW: ops_cap too small (kmahip_ws_status). Device pointers; asynchronous on `stream`. */
typedef struct kmahip_traces {
	int32_t *stats;     /* 10 * n_reads */
	int64_t *ops_off;   /* n_reads */
	int32_t *n_ops;     /* n_reads */
	uint32_t *ops;      /* ops_cap */
	int64_t ops_cap;
} kmahip_traces;
int kmahip_align_trace_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                           const uint8_t *tmpl_ok, const kmahip_params *p, kmahip_traces *out, void *stream);
/* the same with host buffers in and out; returns KMAHIP_EOVERFLOW with the needed run count in *ops_needed */
int kmahip_align_trace(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                       const uint8_t *tmpl_ok, const kmahip_params *p, kmahip_traces *out, int64_t *ops_needed);

/* What the read filter dropped, kept on request (the `-sam` rows of assembly.c:1995-2002: an alignment that fails the filter with a read
 * score other than 0 is still printed as an aligned record). With a record set on the workspace, every trace call on it (kmahip_align_trace_dev,
 * the sessions) fills, per read: stats[6 * i ..] = read_score (which may be negative), start, end, clip_start, clip_end, mapQ, and the read's
 * runs as n_ops[i] entries at ops_off[i] of the SAME run pool (kmahip_traces.ops; they count towards ops_cap) -- for a read with a template that
 * the filter dropped with read_score != 0; all zero for every other read. The read's kmahip_traces entry stays all zero either way, so the
 * pile-up and the fragment rows see no change. DEVICE pointers, n_reads entries as the traces'; NULL (the default) switches it off. */
typedef struct kmahip_trace_drops {
	int32_t *stats;     /* 6 * n_reads */
	int64_t *ops_off;   /* n_reads */
	int32_t *n_ops;     /* n_reads */
} kmahip_trace_drops;
int kmahip_ws_set_trace_drops(kmahip_ws *ws, const kmahip_trace_drops *drops);

/* `-Mt1 t` (runKMA_Mt1, mt1.c:86-500 -> assemble_KMA with read_score == 0, assembly.c:1917-1965): raw reads go straight to
 * stage 3c against ONE template, no stage 2 and no ConClave. Per read: anker_rc (align.c:780-991) seeds both strands against
 * the template's position index and keeps the strand with the larger MEM coverage (forward on equality; the forward strand is
 * only seeded when one of its every-k-th k-mers is in the index, preseed align.c:750-768, unless p->exhaustive), KMA() chains
 * its MEMs and joins them with traceback, then the read filter as in kmahip_align_trace_dev. one2one: `-1t1` was given too
 * (anker_rc's coverage gate, align.c:952). Out: kmahip_traces as above, and rc_out[i] (may be NULL) = 1 when the reverse
 * complement of read i is what was aligned -- pass it as `rc` and a vector of `tmpl` to kmahip_assemble2. Built as a pipeline
 * of kernels (seed + chain per read on a wavefront, DP problems batched by size); device pointers. */
int kmahip_align_trace_mt1_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, int32_t tmpl, int one2one, const kmahip_params *p,
                               kmahip_traces *out, int32_t *rc_out, void *stream);
/* the same with host buffers in and out; KMAHIP_EOVERFLOW with the needed run count in *ops_needed */
int kmahip_align_trace_mt1(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, int32_t tmpl, int one2one, const kmahip_params *p,
                           kmahip_traces *out, int32_t *rc_out, int64_t *ops_needed);

/* Stage 3c per template: pile-up of the traced reads (alnToMat, assembly.c:1317-1444: per template position the counts of
 * A C G T N and gap, insertion columns chained between positions) on the device, then callConsensus + baseCaller
 * (assembly.c:1499-1631, 162-179) in host arithmetic. Inputs: the reads, the rc / tmpl arrays given to
 * kmahip_align_trace and its output (all HOST buffers here). Reads of one template are piled up in the reference's order:
 * reverse stream order inside every chunk of max_frag filed fragments (conclave.c:164-166, 194; kma.c default 1000000;
 * <= 0 selects it) -- only the gap count a NEW insertion column starts with depends on it. bcd / evalue: `-bcd` (1) and
 * `-e` (0.05). Out, per template (DB_size entries, zero where nothing was piled up): cover = called positions equal to the
 * template base, aln_len = called columns, depth = summed depth of the called columns, asm_len = columns incl.
 * insertion columns (runkma.c:792-800 turns these into Template_Identity / Template_Coverage / Query_Identity /
 * Query_Coverage / Depth). Optionally the consensus line of every assembled template ("ACGTN-", lower case = call not
 * significant, '-' = no call), 0-terminated, at consensus + consensus_off[t]. */
typedef struct kmahip_assembly {
	int64_t *cover;
	int64_t *aln_len;
	int64_t *depth;
	int64_t *asm_len;
	char *consensus;          /* may be NULL */
	int64_t *consensus_off;   /* DB_size, may be NULL */
	int64_t consensus_cap;
	int64_t consensus_used;   /* in: 0; out: bytes written */
} kmahip_assembly;
int kmahip_assemble(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                    const kmahip_traces *traces, int64_t max_frag, int bcd, double evalue, kmahip_assembly *out);
/* kmahip_assemble with the per-read inputs already in HBM (reads, rc, tmpl and the traces are DEVICE pointers, e.g. the
 * outputs of kmahip_align_trace_dev); `out` is filled on the host as above. */
int kmahip_assemble_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                        const kmahip_traces *traces, int64_t max_frag, int bcd, double evalue, kmahip_assembly *out);

/* kmahip_assemble with the knobs of the other stage-3c flavours: order 1 = pile the reads up in stream order (what the single
 * reading thread of `-Mt1` does, assembly.c:1873-1965) instead of ConClave's per-template order; caller 1 = nanoCaller
 * (assembly.c:205-240) and sig90 1 = significantAnd90Nuc (assembly.c:147-149), the pair `-bcNano` selects (kma.c:762-766). */
typedef struct kmahip_assemble_opts {
	int64_t max_frag;   /* <= 0: 1000000 */
	double evalue;      /* -e, 0.05 */
	int32_t bcd;        /* -bcd, 1 */
	int32_t order;      /* 0 ConClave's order, 1 stream order */
	int32_t caller;     /* 0 baseCaller, 1 nanoCaller (-bcNano), 2 orgBaseCaller (-bcg), 3 refCaller (-ref_fsa), 4 refNanoCaller (-ref_fsa
	                     * -bcNano): assembly.c:162-270. + 8: insertion columns called as gaps -- which the reference trims from its alignment,
	                     * assembly.c:748-752 -- come out as '_' in the consensus string instead of '-' (for a writer that keeps the gaps of
	                     * template positions: -ref_fsa 0). + 16: alnToMatDense (-dense, assembly.c:1446-1497): template positions only, no
	                     * insertion columns. + 32: the character of EVERY insertion column carries bit 7 (what kmahip_aln_entry needs to tell
	                     * them from template positions; a reader of the string masks with 0x7F) */
	int32_t sig90;      /* 0 significantNuc, 1 significantAnd90Nuc (-bc90, -bcNano), 2 significantAndSupport (-bc x): `support` below */
	/* per read: how many filed fragments (ConClave template != 0) precede it in the WHOLE stream -- what the reference's
	 * chunks of max_frag records are counted in (conclave.c:166, 194). NULL: the batch is the whole stream and the
	 * positions are counted here. A rank that piles up the reads of its templates gathered from several read shards
	 * (kma_amd/dist.py) passes the positions the reads had in the global stream. Host pointer for kmahip_assemble2,
	 * device pointer for kmahip_assemble2_dev. */
	const int64_t *frag_rank;
	double support;     /* sig90 == 2: a base call needs support * depth of the column (assembly.c:151-160) */
} kmahip_assemble_opts;
int kmahip_assemble2(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                     const kmahip_traces *traces, const kmahip_assemble_opts *opts, kmahip_assembly *out);
int kmahip_assemble2_dev(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                         const kmahip_traces *traces, const kmahip_assemble_opts *opts, kmahip_assembly *out);

/* The whole single-end `-1t1` run on one batch, one call: reads uploaded ONCE, stage 2, stage 3a, ConClave, the `.res`
 * statistics, the traceback aligner and the pile-up all on what is already in HBM; only the per-template results (and, if
 * asked for, the per-read columns a `.frag.gz` / SAM writer needs) come back. Equivalent to kmahip_map_se +
 * kmahip_conclave_se + kmahip_res_rows + kmahip_align_trace + kmahip_assemble, minus four uploads of the reads and the
 * host round trips in between (runKMA, runkma.c:104-900, for one chunk of input). HOST buffers.
 *   rows / rows_cap / n_rows   as kmahip_res_rows (KMAHIP_EOVERFLOW with n_rows = needed)
 *   assembly                   as kmahip_assemble
 *   tmpl, n_hits, rc, trace_stats   optional per-read outputs (n_reads, n_reads, n_reads, 10 * n_reads), NULL to skip
 *   ms[6]                      wall time of: upload, stages 2 + 3a, ConClave + statistics, traceback, pile-up, consensus (host)
 *   caller, sig90              IN: nanoCaller / significantAnd90Nuc for the consensus (`-bcNano`, kma.c:762-766); zero = baseCaller */
typedef struct kmahip_run {
	kmahip_res_row *rows;
	int64_t rows_cap, n_rows;
	kmahip_assembly assembly;
	int32_t *tmpl, *n_hits, *rc, *trace_stats;
	double ms[6];
	int32_t caller, sig90;      /* IN, kmahip_run_se / _pe / _chain: the base caller as in kmahip_assemble_opts (`-bcNano` = 1, 1; 0, 0 = baseCaller) */
	double support;             /* IN: as kmahip_assemble_opts.support */
} kmahip_run;
int kmahip_run_se(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p, double evalue, int bcd,
                  int64_t max_frag, kmahip_run *out);

/* The `-Mt1 tmpl` run on one batch (runKMA_Mt1, mt1.c:86-500): raw reads uploaded once, kmahip_align_trace_mt1 per read, the
 * pile-up in stream order and the consensus, all on the device. HOST buffers. aopts: evalue, bcd, caller / sig90 (`-bcNano` = 1, 1);
 * order is stream order whatever aopts says. Out: rows[0] (n_rows = 1) = the `.res` figures of mt1.c:425-447: Score = summed KMA()
 * scores of the kept reads, Expected 0, q_value = Score, p_value = p_chisqr(Score), significant = the reference's gate for printing
 * the row with its identity columns; assembly as kmahip_assemble; tmpl[i] = tmpl for the reads that were kept, n_hits[i] = 1,
 * rc[i] = strand, trace_stats as kmahip_traces.stats -- what kmahip_frag_write2 (order 1) takes. */
int kmahip_run_mt1(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, int32_t tmpl, int one2one, const kmahip_params *p,
                   const kmahip_assemble_opts *aopts, kmahip_run *out);

/* One `.res` row exactly as runKMA prints it (runkma.c:809) from kmahip_res_rows + kmahip_assemble; returns the number of
 * characters written, 0 when the reference prints no row for the template (nothing covered, identity below -ID (1.0) or
 * depth below -md (0.0)). */
int kmahip_res_line(const char *template_name, const kmahip_res_row *row, int64_t cover, int64_t aln_len, int64_t depth_sum,
                    double ID_t, double Depth_t, char *line, int64_t cap);

/* ---- extended features (`-ef [n]`, kma.c:938-948; the `<out>.mapstat` file) -----------------------------------------------------
 * Per template, what the reference gathers beside the `.res` columns while it assembles (HOST vectors of DB_size entries each, zero
 * where nothing was piled up):
 *   depth_var            sum of depth^2 over the columns the consensus calls as something other than '-', insertion columns included
 *                        (callConsensus, assembly.c:1598-1601)
 *   snp_sum, deletion_sum   over the template positions: the bases that differ from the template's, the gaps (ef.c:94-96)
 *   insert_sum           the bases on the insertion columns (ef.c:97-99)
 *   max_depth            the deepest column, gaps counted (ef.c:101-105)
 *   nuc_high_var         the columns deeper than depth / t_len + 3 sqrt(var) (ef.c:65, 106-108)
 *   score_sum, read_count_aln, fragment_count_aln   over the reads the stage-3c filter kept (alnToMat, assembly.c:1334-1338): their
 *                        alignment scores without the end bonus, their number, and the number of those that are not the second mate of
 *                        a proper pair (`!(flag & 2) || (flag & 64)`), raised to half the reads (ef.c:71)
 *   var                  depth_var / t_len - (depth / t_len)^2 in long double, stored when it is not negative (assembly.c:2067-2081);
 *                        else fixVarOverflow's sum over the template positions (assembly.c:1633-1687)
 * Counts are read as the reference's 16-bit counters hold them. */
typedef struct kmahip_assembly_ef {
	uint64_t *depth_var;
	uint64_t *snp_sum, *insert_sum, *deletion_sum;
	uint32_t *max_depth, *nuc_high_var;
	uint64_t *score_sum;
	uint32_t *read_count_aln, *fragment_count_aln;
	double *var;
} kmahip_assembly_ef;
/* Valid directly after a kmahip_assemble2 / kmahip_assemble2_dev call on the same workspace, before anything else uses it: the sums
 * are made over the pile-up that call left in HBM, by kernels of their own behind it. n_reads, tmpl, traces (only `stats` is read)
 * and `assembly` are those of that call; flag: per read the frag_raw flag (kmahip_hits.flag; for the fragments of a paired run their
 * record's), NULL = every read is a fragment; p: rw.Wl, the end bonus the scores carry. KMAHIP_EINVAL with a message when the
 * pile-up is not there (no such call before, or its columns were called on the host: KMAHIP_HOST_CONSENSUS).
 * _dev: tmpl, traces->stats and flag are DEVICE pointers; the other form takes them on the host. `out` is the host's in both. */
int kmahip_assemble_ef_dev(kmahip_db *db, kmahip_ws *ws, int64_t n_reads, const int32_t *tmpl, const kmahip_traces *traces, const int32_t *flag,
                           const kmahip_params *p, const kmahip_assembly *assembly, kmahip_assembly_ef *out);
int kmahip_assemble_ef(kmahip_db *db, kmahip_ws *ws, int64_t n_reads, const int32_t *tmpl, const kmahip_traces *traces, const int32_t *flag,
                       const kmahip_params *p, const kmahip_assembly *assembly, kmahip_assembly_ef *out);

/* The text of `<out>.mapstat`. Header (initExtendedFeatures, ef.c:30-46): `## method`, `## version` (that of the reference whose file
 * this is: KMAHIP_MAPSTAT_VERSION), `## database` (t_db without its folder), `## fragmentCount` (the records stage 1 passed on, a couple
 * counting once: kmahip_read_batch.records summed; ankers.c:163-216), `## date`, `## command`, the column line. Returns the
 * characters written, 0 when cap is too small. */
#define KMAHIP_MAPSTAT_VERSION "1.5.1"
int64_t kmahip_mapstat_header(const char *t_db, uint32_t fragment_count, const char *cmdline, char *text, int64_t cap);
/* One row (printExtendedFeatures, ef.c:129-136), printed exactly where the `.res` row is (runkma.c:814-829): the first seven arguments
 * are kmahip_res_line's, and the result is 0 where that function's is. read_count / fragment_count: ConClave's (kmahip_conclave). */
typedef struct kmahip_mapstat_row {
	uint32_t read_count, fragment_count;
	uint64_t score_sum;
	double var;
	uint32_t nuc_high_var, max_depth;
	uint64_t snp_sum, insert_sum, deletion_sum;
	uint32_t read_count_aln, fragment_count_aln;
} kmahip_mapstat_row;
int kmahip_mapstat_line(const char *template_name, const kmahip_res_row *row, int64_t cover, int64_t aln_len, int64_t depth_sum,
                        double ID_t, double Depth_t, const kmahip_mapstat_row *ef, char *line, int64_t cap);

/* ---- the count matrix and the VCF file (`-matrix`, kma.c:667; `-vcf [n]`, kma.c:949-961: `<out>.mat.gz`, `<out>.vcf.gz`) ----------------
 * Both are made over the pile-up the last kmahip_assemble2 / kmahip_assemble2_dev call left in HBM, by kernels of their own behind it
 * (over consensus_kernel's segment list), for the templates `mask` names: HOST bytes, DB_size of them, 1 where the `.res` row of the
 * template passes its gate (kmahip_res_line gives a row). Valid directly after that call on the same workspace (kmahip_assemble_ef[_dev]
 * may come between: it leaves the pile-up as it is); KMAHIP_EINVAL with a message when the pile-up is not there or its columns were
 * called on the host (KMAHIP_HOST_CONSENSUS). Neither takes a per-read array, so there is no host-pointer form beside them.
 *
 * kmahip_assemble_matrix_dev replaces the row loop of updateMatrix (assembly.c:107-129; called at runkma.c:824, :1538, mt1.c:445): per
 * column in ring order (template position p, then the insertion columns in front of p + 1) the row
 * `<ref>\t%hu\t%hu\t%hu\t%hu\t%hu\t%hu\n`, <ref> the template's base or '-' at an insertion column, counts as the reference's 16-bit
 * counters hold them. The rows are formatted on the device and handed to `sink` in template order, whole rows only, in pieces of at most
 * chunk_bytes + 37 bytes (chunk_bytes <= 0: the value of KMAHIP_MAT_CHUNK, or 64 MiB); tmpl_bytes[t] (HOST, DB_size entries; filled
 * before the first call of `sink`) is the number of bytes of template t, so the caller can put `#name\n` in front of a template's
 * rows and the empty line behind them (assembly.c:100-105, 131-139). sink NULL: the sizes alone. A sink that returns non-zero ends the
 * call with KMAHIP_EIO. */
typedef int (*kmahip_text_sink)(void *user, const char *text, int64_t bytes);
int kmahip_assemble_matrix_dev(kmahip_db *db, kmahip_ws *ws, const uint8_t *mask, int64_t chunk_bytes, int64_t *tmpl_bytes, kmahip_text_sink sink, void *user);

/* kmahip_assemble_vcf_dev replaces the column loop of updateVcf (vcf.c:128-277; called at runkma.c:830, :1544, mt1.c:448) up to the
 * decision whether a column's row is printed: one record per printed row, in ring order, templates ascending. The gates are evaluated
 * on the device (vcf.c:195, and the all-zero row of a template position nothing was piled on, vcf.c:261-275); `evalue < P` is the test
 * of the consensus, Q < q* in IEEE double. The text is the host's (kmahip_vcf_line): no floating-point text is made on the device.
 *   pos          POS: the template position + 1, 0 at an insertion column
 *   ref          the template's base ('A', 'C', 'G', 'T'), '-' at an insertion column
 *   call         the called character ('.' in the all-zero row)
 *   best_score   bestScore as updateVcf leaves it behind its minor-call branch (vcf.c:143-178)
 *   counts       A, C, G, T, N, gaps, as the reference's 16-bit counters hold them
 * tmpl_rows[t] (HOST, DB_size entries): the records of template t. recs: room for `cap` records (HOST); *n_recs: the number there is.
 * recs NULL: the numbers alone; cap too small: KMAHIP_EOVERFLOW with *n_recs set. */
typedef struct kmahip_vcf_rec {
	int32_t tmpl, pos;
	uint8_t ref, call;
	uint16_t reserved;
	int32_t best_score;
	uint32_t counts[6];
} kmahip_vcf_rec;
int kmahip_assemble_vcf_dev(kmahip_db *db, kmahip_ws *ws, const uint8_t *mask, int64_t *tmpl_rows, kmahip_vcf_rec *recs, int64_t cap, int64_t *n_recs);

/* The text of `<out>.vcf.gz`. Header (initialiseVcf, vcf.c:46-95): kmaVersion is KMAHIP_MAPSTAT_VERSION, the last column t_db without
 * its folder. One row (vcf.c:180-275) from a record: AF, RAF and Q with %.2f, P = p_chisqr(Q) with %4.1e, QUAL from binP(DP, AD, 0.25)
 * (stdstat.c:149-202), PASS / LowQual / FAIL (vcf.c:202-208), `<->` for a gap on either side, all in the host's libm. evalue, support,
 * bcd: those of the run; filter: the value of -vcf (2 fills the FILTER column, else it is `.`). Both return the characters written,
 * 0 when cap is too small. */
int64_t kmahip_vcf_header(const char *t_db, char *text, int64_t cap);
int kmahip_vcf_line(const char *template_name, const kmahip_vcf_rec *rec, double evalue, double support, int bcd, int filter, char *line, int64_t cap);

/* ---- stage 2 of the DEFAULT mode (no -1t1) -------------------------------------------------------------------
 * kmerScan = save_kmers_chain (savekmers.c:5127-5945, the reference's default, savekmers.c:40) with the default helpers of
 * kmeranker.c:25-30. A read yields zero or more S2 records, one per accepted chain of anchors: rc_flag = the chain's score
 * (negative: both strands carry it and the reverse strand's templates follow as negative ids), emit_rc = 1 when the record
 * prints the reverse-complemented read (print_ankers with qseq_r), [q_start, q_end) = the query bounds insertKmerBound appends
 * to the header behind a NUL (qseqs.c:41-56; read back at alnfrags.c:1092-1099, conclave.c:137-145, assembly.c:1926-1933).
 * Records come back in stream order: reads ascending, the chains of a read in the order the reference prints them. HOST buffers;
 * KMAHIP_EOVERFLOW with n_recs / n_T = what is needed when rec_cap / T_cap are too small. Parameters: minlen (-ml, 16),
 * coverT (-mct, 0.1: how much of a chain may overlap what was taken before), mrs (-mrs, 0.5); NULL = those defaults.
 * One lane per read on per-lane scratch in HBM: the anchor search is this round's correct-first form. */
typedef struct kmahip_chain_params { int32_t minlen; int32_t pad_; double coverT, mrs; } kmahip_chain_params;
typedef struct kmahip_chain_recs {
	int64_t rec_cap, T_cap;   /* in: capacities of the arrays below (T_off: rec_cap + 1) */
	int64_t n_recs, n_T;      /* out */
	int64_t *read;            /* index of the read in the batch */
	int32_t *rc_flag, *emit_rc, *q_start, *q_end;
	int64_t *T_off;           /* templates of record i: T[T_off[i] .. T_off[i + 1]) */
	int32_t *T;
} kmahip_chain_recs;
int kmahip_scan_chain(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_params *p, const kmahip_chain_params *cp,
                      kmahip_chain_recs *out);
/* One place where the reference's own result is not a function of its input (savekmers.c:5447-5449): behind an N the chain finder
 * restarts the reverse strand's rolling k-mer k bases too far on, which for a read with an N among its first k - 1 bases lies
 * beyond the end of that read in a buffer the reference never clears -- zeros while no longer read came before it in the stream,
 * otherwise what the longer read left there (and with -t > 1 whichever read the thread's buffer held last). This library reads
 * zeros. kmahip_chain_unpinned_reads counts, on HOST arrays of a batch in stream order, the reads for which that matters: an N among
 * the first k - 1 bases and a longer read somewhere before (longest_before: the longest read of the batches before this one, 0 for
 * the first; *longest_after = what to pass with the next batch). Their records may differ from the reference's; a host that must
 * know says so (examples/kmahip_map prints the count). */
int kmahip_chain_unpinned_reads(const int32_t *len, const int32_t *N, const int64_t *N_off, int64_t n_reads, int k,
                                int32_t longest_before, int32_t *longest_after, int64_t *count);

/* ---- index build: `kma index -i <fasta ...> -o <prefix> [-k k]` ------------------------------------------------
 * Writes <prefix>.comp.b / .length.b / .seq.b / .name as the reference's index.c + makeindex.c:167-330 (makeDB) +
 * compress.c:83-614 (compressKMA_DB) do for the default options: the hashed index form, k <= 16, templates trimmed of leading /
 * trailing N's (their count goes into the name as " B<n>"), templates shorter than k skipped, k-mers that hold an N left out,
 * equal template lists stored once. Every k-mer start becomes a 64-bit key on the device (k-mer << 32 | template), sorted and
 * made unique there (rocPRIM); grouping, list sharing and the bucket directory are one pass on the host. The files hold the
 * same k-mer -> template-list mapping as the reference's (tests compare the two) and the reference maps against them with
 * identical results; bucket count, key order inside a bucket and list order are the builder's own. FASTA input, plain or .gz.
 * Not covered: minimizers (-m), homopolymer compression (-hc); -Sparse / prefixes have their own entry point,
 * kmahip_index_build_sparse below, and so has -t_db (kmahip_index_append); `-batch list` is the
 * host program's (examples/kmahip_index: the listed paths become fasta_paths). */
int kmahip_index_build(const char *const *fasta_paths, int n_files, const char *out_prefix, int kmersize);
/* `kma index ... -deCon <fasta ...>` (index.c:676-729, decon.c:77-227): the four files of kmahip_index_build, byte for byte, and
 * <prefix>.decon.comp.b beside them, the same mapping with the pseudo-template DB_size (one past the last template) appended to the
 * list of every database k-mer that occurs in a contamination record or in its reverse complement. A record counts when it is
 * longer than k; N's split it as they split a template. A k-mer that only the contamination holds is not added. decon_paths: FASTA,
 * plain or .gz; "--" (standard input) is refused with KMAHIP_EINVAL. Marking an index that exists: kmahip_index_append. */
int kmahip_index_build_decon(const char *const *fasta_paths, int n_files, const char *const *decon_paths, int n_decon,
                             const char *out_prefix, int kmersize);
/* `kma index ... -Sparse <prefix | -> [-ML n]` (index.c:451-474, 576-613; makeindex.c:46-48, 167-291; updateindex.c:79-199:
 * updateDBs_sparse, updateAnnots_sparse; qualcheck.c:31-79: lengthCheck; hashmap.c:120-187): the index `kma -Sparse` and
 * kmahip_sparse_open map against. A window is prefix_len + k bases of a trimmed template or of its reverse complement that hold no N
 * and start with the prefix; its k-mer, the last k bases, is indexed. prefix_text "-": no prefix, every N-free k-mer of either strand
 * (header fields prefix_len 0, prefix 1). A template stays when it is LONGER than MinLen = max(k, kmerindex), has MinKlen = 1
 * windows at least (without a prefix (length - k + 1) * 2 stands for the count) and one window in any case; a template that goes
 * gets no id, no name and no .seq.b words, and those behind it move up. min_len (-ML) > k + prefix_len + 1: MinLen = min_len,
 * MinKlen = 2 * (min_len - k - prefix_len + 1), divided by 4 once per prefix base; any other value (0: the default) is ignored,
 * as the reference ignores it. .length.b holds DB_size, lengths (slot 0: kmerindex), slengths (windows of both strands) and
 * ulengths (distinct window k-mers); .comp.b the same k-mer -> ascending template list mapping as the reference's, in the
 * builder's own bucket layout; .seq.b and .name as kmahip_index_build writes them, over the templates that stayed.
 * kmersize <= 0: 16. kmerindex <= 0: kmersize (what -k sets). KMAHIP_EINVAL, the reason in kmahip_last_error: k outside 4 ... 16,
 * a prefix of more than 16 bases, a null prefix, an empty one or one with a letter that is no A, C, G, T (IUPAC codes as the
 * reference folds them) -- "Invalid prefix." as the reference says. Not covered: -deCon on a sparse index; -ht / -hq and appending
 * (kmahip_index_append) have their own entry points below. */
int kmahip_index_build_sparse(const char *const *fasta_paths, int n_files, const char *out_prefix, int kmersize, int kmerindex,
                              const char *prefix_text, int min_len);
/* `kma index ... -Sparse <prefix | -> -hq x -ht y [-and]` (index.c:309-350, 607-613; qualcheck.c:81-324: queryCheck, templateCheck,
 * called from updateDBs_sparse alone, updateindex.c:103): homology reduction while the sparse index is built. Templates come in file
 * order; one that reaches the length gates is scored against the templates kept before it. For a kept template j, Scores_tot[j] =
 * the windows of the new template, repeats and all, whose k-mer j holds, Scores[j] = its distinct k-mers that j holds; thisQ =
 * 1.0 * Scores_tot[j] / thisKlen (its windows on both strands), thisT = 1.0 * Scores[j] / ulength[j]; bestQ, bestT their maxima, a tie
 * going to the template met first in the walk (forward strand, then the reverse complement; inside one value list the lower id).
 * hom_t < 1 selects templateCheck: the template stays iff cmp(bestT < hom_t, bestQ < hom_q), cmp = OR, AND when and_mode != 0.
 * Otherwise hom_q < 1 selects queryCheck: it stays iff bestQ < hom_q. Otherwise the build is kmahip_index_build_sparse's. A template
 * that goes gets no id, and the ids behind it move up. The pairs are counted on the device (homology.hip), the chain of decisions is
 * the host's; the files are those of kmahip_index_build_sparse over the templates that stayed.
 * report_path: the cluster lines the reference prints to standard output, one per template whose windows reach MinKlen, in file
 * order: queryCheck `name\t<its id, or templateQ when it goes>\t%f\t%d` (bestQ, templateQ), templateCheck six fields (`name`, its
 * id or -- when it goes -- templateQ if bestT < hom_t, else templateT; bestQ, templateQ, bestT, templateT). NULL: no report; "-":
 * standard output. The lines are written before an empty database is reported (KMAHIP_EFORMAT, "DB is empty"; hom_q = 0 keeps nothing).
 * KMAHIP_EINVAL besides kmahip_index_build_sparse's: a threshold below 0; hom_t < 1 with a min_len that takes effect (templateCheck
 * returns at qualcheck.c:287 without clearing its scores, so the reference's later answers rest on stale state).
 * KMAHIP_HOM_BLOCK (columns a workgroup sums at once) and KMAHIP_HOM_PAIRS (first capacity of the pair list) are test knobs. */
int kmahip_index_build_sparse_hom(const char *const *fasta_paths, int n_files, const char *out_prefix, int kmersize, int kmerindex,
                                  const char *prefix_text, int min_len, double hom_q, double hom_t, int and_mode, const char *report_path);
/* Test and timing hooks of the homology counts. kmahip_test_index_hom_rows runs the build up to the report and writes no file: out
 * takes seven words per candidate template (one longer than MinLen) in file order -- stays, thisKlen, max Scores_tot and its template,
 * Scores and ulength of the best thisT and its template, the templates numbered in file order from 1 (0: none) --, *n_rows how many
 * there are (KMAHIP_EINVAL with *n_rows set when cap_rows is too small). kmahip_test_index_hom_timing: what the last homology step of
 * this process took by the host's clock: ms of pass 1, of the host's chain of decisions, of pass 2, and the pairs pass 1 listed. */
int kmahip_test_index_hom_rows(const char *const *fasta_paths, int n_files, int kmersize, const char *prefix_text, int min_len, double hom_q,
                               double hom_t, int and_mode, uint32_t *out, int64_t cap_rows, int64_t *n_rows);
int kmahip_test_index_hom_timing(double *out4);
/* `kma index -t_db <prefix> [-i <fasta ...>] [-deCon <fasta ...>] [-o <out>]` (index.c:221-229, 529-557, 616-674, 676-732; load_DBs,
 * loadupdate.c:151-210; hashMapKMA_openChains, loadupdate.c:64-112): templates are added to an index that exists. The result is the
 * index a fresh build of the old templates followed by the new ones gives: byte for byte the files kmahip_index_build /
 * _build_sparse / _build_decon write for the concatenated input, and the reference's own append in mapping, header, lengths, names
 * and sequences. k and the sparse prefix are the old index's (a sparse index is appended sparsely); the new templates get the ids
 * from the old DB_size on and are parsed as in a fresh build (N trimming, " B<n>", the length gate, IUPAC folding). The k-mers of
 * the old templates come out of the old .comp.b, not out of .seq.b (which stores N as A): the k-mer -> value-list table is
 * expanded back into (k-mer << 32 | template) pairs on the device (one thread per k-mer counts, a scan, one lane per pair writes),
 * joins the keys of the new templates in the sort and goes through the host pass of a fresh build. The list width follows the new
 * DB_size (16 bits below 65535). The old index may be the reference's or ours, hashed or direct-address.
 * n_files == 0 with n_decon > 0: decontamination onto the index as it is; only <prefix>.decon.comp.b is written. With both, the
 * pseudo-template is the new DB_size. out_prefix NULL: in place. Every file is written as <out>.appending<ext> and renamed at the
 * end, so a failed in-place append leaves the old index whole; with an out_prefix of its own the old files are never touched. An
 * old <prefix>.decon.comp.b beside an index appended without decon_paths is left as it is, as in the reference: it is stale then.
 * Before any launch the old index is held to its header: every list inside the value array, not empty, ascending, ids 1 ..
 * DB_size - 1, .length.b / .name / .seq.b of the sizes DB_size and the lengths ask for; else KMAHIP_EFORMAT, "Wrong format of DB."
 * KMAHIP_EFORMAT by name also: k > 16, a minimizer / homopolymer flag. KMAHIP_EINVAL: a NULL db_prefix, neither input ("No inputfiles
 * defined."), "--" among decon_paths, decon_paths on a sparse index (deConNode_sparse). Not covered: -hq / -ht / -ML with an append. */
int kmahip_index_append(const char *db_prefix, const char *const *fasta_paths, int n_files, const char *const *decon_paths, int n_decon,
                        const char *out_prefix);
/* Test and timing hooks of the expansion. kmahip_test_index_expand: the pairs of <prefix>.comp.b (k-mer << 32 | template) as the
 * device wrote them, in the order of the file's k-mers; *n how many (KMAHIP_EINVAL with *n set when cap is too small); the file is
 * checked as kmahip_index_append checks it. kmahip_test_index_expand_timing: ms of the count kernel, the scan and the write pass of
 * the last expansion of this process, by device events. */
int kmahip_test_index_expand(const char *prefix, uint64_t *out_pairs, int64_t cap, int64_t *n);
int kmahip_test_index_expand_timing(double *out3);

/* ---- stage 1: FASTQ / FASTA ingest into packed read batches -------------------------------------------
 * Host code (zlib for .gz, plain files read as they are): the record parser of FileBuffgetFq / FileBuffgetFsa
 * (seqparse.c:241-403, 66-159) with the to2Bit table of kma.c:1440-1480 (IUPAC codes fold onto ACGT, N / X = 4), the
 * phred-scale guess of getPhredFileBuff (seqparse.c:551-589), the quality trimming of phredStat (runinput.c:127-313;
 * fsastat :315-368 for FASTA), the length gate of run_input / run_input_PE (runinput.c:370-606) and the 2-bit packing of
 * compDNA (compdna.c:99-127). What it yields is what the reference's stage 1 writes into the S1 stream (printFsa /
 * printFsa_pair, runinput.c:765-830), in the same order. */
typedef struct kmahip_trim {
	int32_t min_phred;    /* -mp  (20): 5' / 3' end bases below it are trimmed */
	int32_t min_q;        /* -eq  (0): minimum average quality, bi-directional trimming towards it */
	int32_t hardmask_q;   /* -mi  (0): bases below it become N */
	int32_t min_len;      /* -ml  (16) */
	int32_t max_len;      /* -xl  (2147483647) */
} kmahip_trim;
void kmahip_trim_default(kmahip_trim *t);

typedef struct kmahip_ingest kmahip_ingest;

/* One batch, owned by the reader and valid until the next call on it. `reads` holds HOST pointers in the layout every
 * kmahip_*_se / _pe call takes (each read followed by one pad word). pair[i]: 0 = single record, 1 = first mate of a
 * pair record (its second mate is read i + 1, pair 2). */
typedef struct kmahip_read_batch {
	kmahip_reads reads;
	const char *names;        /* header lines without '@' / '>', chomped, each NUL-terminated */
	const int64_t *name_off;  /* n_reads + 1 */
	const uint8_t *pair;      /* n_reads */
	int64_t records;          /* S1 records in the batch (a pair counts once) */
} kmahip_read_batch;

/* path2 == NULL: single end (run_input); otherwise the two mate files are read in lockstep (run_input_PE): both mates
 * long enough -> a pair record, one of them -> a single record, none -> dropped. */
int kmahip_ingest_open(const char *path1, const char *path2, const kmahip_trim *trim, kmahip_ingest **out);
/* `-int file` (run_input_INT, runinput.c:608-740): ONE file whose records are taken two at a time as the mates of a couple, trimmed
 * and gated like the two files of -ipe (both long enough -> a pair record, one -> a single record); the last record of a file with
 * an odd number of them meets an empty mate (FileBuffgetFq clears the length before it finds the end, seqparse.c:249) and is filed
 * singly. The batches are those of a paired reader (pair[] = 1 / 2 / 0). FASTQ only: for FASTA the reference cuts mate 2 with
 * mate 1's bounds (runinput.c:705), which may reach past what it read -- KMAHIP_EFORMAT. */
int kmahip_ingest_open_interleaved(const char *path, const kmahip_trim *trim, kmahip_ingest **out);
/* up to max_records further S1 records; batch->reads.n_reads == 0 at the end of the input. A record that does not start
 * with '@' ends the input like in the reference ("Malformed input.", seqparse.c:256-260): the records before it are
 * delivered, then one call returns KMAHIP_EFORMAT. */
int kmahip_ingest_next(kmahip_ingest *in, int64_t max_records, kmahip_read_batch *batch);
/* A second bound on the batches of kmahip_ingest_next, for inputs of long reads where a count of records says little about a batch's
 * size: a batch also closes once it holds about max_bases bases (checked between the stretches of input the reader cuts into records:
 * it may go over by one such stretch, tens of megabytes of text). 0 (the default): no such bound. */
int kmahip_ingest_set_batch_bases(kmahip_ingest *in, int64_t max_bases);
/* For a caller that took the whole input as one batch (max_records = INT64_MAX): KMAHIP_EIO / KMAHIP_EFORMAT when the input broke
 * off behind the records delivered (a truncated or corrupt .gz, a record that does not start with '@'; the reference ends with a
 * non-zero exit status there), 0 otherwise. Does not touch the batch -- another kmahip_ingest_next would, its arrays are reused. */
int kmahip_ingest_status(kmahip_ingest *in);
/* 33 or 64 (0: undeterminable, treated like the reference does); records read / kept so far */
int kmahip_ingest_phred_scale(const kmahip_ingest *in);
void kmahip_ingest_counts(const kmahip_ingest *in, int64_t *records_read, int64_t *records_kept);
void kmahip_ingest_close(kmahip_ingest *in);

/* ---- stage 1 on the device: the same batches, born in HBM ------------------------------------------------------------
 * A second reader for plain (uncompressed) FASTQ in regular files, single end or two mate files in lockstep: the host only
 * reads file bytes into pinned buffers and copies them up; locating the records (FileBuffgetFq, seqparse.c:241-403), quality
 * trimming and the length gate (phredStat runinput.c:127-313, run_input / run_input_PE :370-606) and the 2-bit packing
 * (compDNA, compdna.c:99-127) are HIP kernels. Read for read its batches are those of kmahip_ingest_next on the same
 * input; where a batch ends is the reader's own business (a batch never ends inside a couple). The first record that is
 * not four well-formed lines ends the device's part: from there on -- and for the bytes behind the last complete record
 * of the input -- the host reader above does the work inside this one, so odd files and "Malformed input." behave as ever.
 * NOT covered: .gz, FASTA, interleaved input, byte-range parts. kmahip_ingest_dev_open refuses those with KMAHIP_EFORMAT
 * (kmahip_last_error names the reason) before it makes any HIP call: take kmahip_ingest_open for them. */
typedef struct kmahip_ingest_dev kmahip_ingest_dev;
/* run_input / run_input_PE (runinput.c:370-606) over plain FASTQ; the device current at the call is the reader's */
int kmahip_ingest_dev_open(const char *path1, const char *path2, const kmahip_trim *trim, kmahip_ingest_dev **out);
/* up to max_records further S1 records (printFsa / printFsa_pair, runinput.c:765-830). batch->reads.*, names, name_off:
 * DEVICE pointers; batch->pair: HOST; the scalar fields filled. All valid until the next call on the reader. */
int kmahip_ingest_dev_next(kmahip_ingest_dev *in, int64_t max_records, kmahip_read_batch *batch);
/* as kmahip_ingest_status ("Malformed input.", seqparse.c:256-260), kmahip_ingest_phred_scale (getPhredFileBuff,
 * seqparse.c:551-589) and kmahip_ingest_counts */
int kmahip_ingest_dev_status(kmahip_ingest_dev *in);
int kmahip_ingest_dev_phred_scale(const kmahip_ingest_dev *in);
void kmahip_ingest_dev_counts(const kmahip_ingest_dev *in, int64_t *records_read, int64_t *records_kept);
/* bytes of input that were left to the host reader inside this one, from an odd record or the unfinished end of the input on
 * (0: the device delivered every record itself) */
int64_t kmahip_ingest_dev_handed_back(const kmahip_ingest_dev *in);
/* where the device part's time went so far, ms: [0] reading the files into pinned memory, [1] waiting for the copies,
 * [2] kernels, scans and the figures that come back; *bytes: input bytes copied up */
void kmahip_ingest_dev_timing(const kmahip_ingest_dev *in, double ms[3], int64_t *bytes);
/* for callers without a HIP runtime of their own (the Python binding): bytes of a batch's device arrays copied to host memory */
int kmahip_ingest_dev_copy_out(void *host_dst, const void *dev_src, size_t bytes);
void kmahip_ingest_dev_close(kmahip_ingest_dev *in);

/* ---- the QC report (`kma ... -qc`, `kma trim -qc`) and the trimmed reads as text (`kma trim`) ------------------------------------
 * An accumulator that the readers above feed while they trim: what init_QCstat / update_QCstat (qc.c:24-43, 85-104) keep and
 * print_QCstat (qc.c:167-262) prints. A reader with an accumulator trims by the reference's -qc rule (phredStat with a report,
 * runinput.c:133-136, 163, 303-312): every read goes through the summing loop whatever -eq and -mi are, and the figure held against
 * -ml is the trimmed length less its N's (hard-masked bases included) -- so a read with len >= ml > len - ns is kept without an
 * accumulator and dropped with one. A reader without one does exactly what it did before. */
typedef struct kmahip_qc kmahip_qc;
typedef struct kmahip_qc_stats {
	uint64_t fragcount, org_fragcount;   /* S1 records kept / read, a couple counting once (runinput.c:448-452, 587-593, 712-718) */
	uint64_t count, org_count;           /* sequences counted by update_QCstat (ml <= len - ns, per mate) / read (runinput.c:133-136) */
	uint64_t bpcount, org_bpcount;
	uint64_t totgc, totns;               /* C and G that were not hard-masked; N's and hard-masked bases */
	double Eeq;                          /* sum of every counted sequence's sum of 10^(-q/10), added up in stream order */
	int32_t maxlen, qresolution;         /* longest counted sequence; ldist bin = len >> qresolution (rescale_ldist, qc.c:50-65) */
	int32_t phred_scale, pad_;           /* runinput.c:451, 590-592, 715-717: the last single-end file's, a paired one's once Eeq != 0 */
	uint32_t qdist[256];                 /* bin (int) ceil(-10 * log10(sp / len)), decided by the host's log10 (qc.c:102) */
	uint32_t ldist[512];
} kmahip_qc_stats;
/* init_QCstat(0) / destroy_QCstat (qc.c:24-48) */
int kmahip_qc_open(kmahip_qc **out);
void kmahip_qc_close(kmahip_qc *qc);
/* Attach an accumulator to a reader, before its first _next (KMAHIP_EINVAL afterwards): from then on the reader trims by the -qc
 * rule and feeds it (phredStat, runinput.c:127-313; the counts of run_input / _PE / _INT, :448-452, 587-593, 712-718). Readers one
 * after the other feed one accumulator (`-i a b`; the host reader that the device reader hands odd records to takes it over by
 * itself). Refused by name, where the reference dies (runinput.c:359-361 with qc.c:102): FASTA input (KMAHIP_EFORMAT) and a
 * minimum length below 1 (KMAHIP_EINVAL). The accumulator must outlive the reader. */
int kmahip_ingest_set_qc(kmahip_ingest *in, kmahip_qc *qc);
int kmahip_ingest_dev_set_qc(kmahip_ingest_dev *in, kmahip_qc *qc);
/* the sums so far (a copy) */
int kmahip_qc_get(const kmahip_qc *qc, kmahip_qc_stats *out);
/* print_QCstat (qc.c:167-262) into `path`: `trim` as the options gave it ("End Trim Q" is -mp raised to -mi, kma.c:1555-1557 /
 * trim.c:432-434), clip5 / clip3 the -5p / -3p values, which are printed and read by nothing else. The four quality lines, E(Q) and
 * the Q distribution are left out while Eeq == 0. */
int kmahip_qc_write(const kmahip_qc *qc, const kmahip_trim *trim, int clip5, int clip3, const char *path);
/* `kma trim` (printTrimFsa / printTrimFsa_pair, trim.c:28-126): with on != 0, set before the first _next, every batch of the host
 * reader also carries its records as FASTQ text -- the chomped header line with its '@', the trimmed bases through to2Bit and
 * "ACGTN" (IUPAC and lower case become A / C / G / T, hard-masked bases N), "+", the trimmed qualities -- single records in stream 0
 * (<out>.fq), couples in stream 1 (<out>_int.fq), both in stream order. kmahip_ingest_text: the text of the batch delivered last,
 * valid until the next call on the reader. */
int kmahip_ingest_set_text(kmahip_ingest *in, int on);
int kmahip_ingest_text(const kmahip_ingest *in, int stream, const char **text, int64_t *bytes);
/* the same for the device reader: the text is written on the device (s1_fastq_kernel: a record's size from its trimmed span and its
 * name, the sizes scanned per stream, a group of lanes per record) and comes back with the batch -- `text` is HOST memory, valid until
 * the next call. The part of an odd file that the host reader takes is the host reader's text. */
int kmahip_ingest_dev_set_text(kmahip_ingest_dev *in, int on);
int kmahip_ingest_dev_text(const kmahip_ingest_dev *in, int stream, const char **text, int64_t *bytes);
/* what the report cost the device reader so far, ms: [0] fetching the counted sequences' (sp, len), [1] adding and binning them on the host */
void kmahip_ingest_dev_qc_timing(const kmahip_ingest_dev *in, double ms[2]);
/* trim_main (trim.c:149-472) over files: single-end files (run_input), then couples of mate files (run_input_PE), then interleaved
 * files (run_input_INT), FASTQ plain or .gz, into <out_prefix>.fq and -- when there are paired or interleaved files --
 * <out_prefix>_int.fq; with qc != NULL the report is fed (and written to <out_prefix>.json by the caller, kmahip_qc_write).
 * s1dev != 0: stage 1 and the text of the files the device reader covers (plain FASTQ, single end or mate files) are made on the
 * device current at the call, everything else -- .gz, interleaved files, odd records -- by the host reader, as ever.
 * *fragments: the records written, a couple counting once. FASTA input: KMAHIP_EFORMAT. */
int kmahip_trim_files(const char *const *se, int n_se, const char *const *pe, int n_pe, const char *const *il, int n_il,
                      const kmahip_trim *trim, kmahip_qc *qc, int s1dev, const char *out_prefix, int64_t *fragments);

/* `.frag.gz` (updateFrags, assembly.c:49-83): one row per read that passed the stage-3c filter -- the read as aligned, the
 * number of equally good templates, score, start, end, template name (from <prefix>.name), read header -- in the order a
 * single-threaded assemble_KMA writes them: templates ascending, inside a template the pile-up order (see kmahip_assemble).
 * HOST buffers: the reads, kmahip_hits.rc, kmahip_conclave.tmpl, the per-read tie count (kmahip_hits.n_hits), the stats
 * array of kmahip_align_trace and the read headers (kmahip_read_batch.names / name_off). A path ending in ".gz" is
 * gzip-compressed (level 1 as filebuff.c:189), anything else plain text. */
int kmahip_frag_write(const char *path, kmahip_db *db, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                      const int32_t *n_hits, const int32_t *trace_stats, int64_t max_frag, const char *read_names,
                      const int64_t *read_name_off, int64_t *rows);

/* kmahip_frag_write with the row order chosen: order 0 = as above, 1 = stream order inside a template (`-Mt1`) */
int kmahip_frag_write2(const char *path, kmahip_db *db, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                       const int32_t *n_hits, const int32_t *trace_stats, int64_t max_frag, int order, const char *read_names,
                       const int64_t *read_name_off, int64_t *rows);

/* kmahip_frag_write2 for a batch that is not the whole stream: frag_rank[i] = number of filed fragments before read i in
 * the whole stream (as kmahip_assemble_opts.frag_rank; NULL = count them in this batch). */
int kmahip_frag_write3(const char *path, kmahip_db *db, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl,
                       const int32_t *n_hits, const int32_t *trace_stats, int64_t max_frag, int order, const int64_t *frag_rank,
                       const char *read_names, const int64_t *read_name_off, int64_t *rows);

/* One gzip member as kmahip_frag_write* makes them for a path ending in ".gz": Huffman coding only (the reference deflates
 * at level 1, filebuff.c:189 -- what a reader inflates is the same). The writers compress blocks of rows on several threads
 * and concatenate the members (RFC 1952 2.2). Exposed for tests. */
int kmahip_gzip_member(const void *src, int64_t n, void *dst, int64_t cap, int64_t *out_bytes);

/* ---- SAM records (`-sam [n]`, kma.c:1005-1012; saminit / samwrite / makeCigar, sam.c:30-211) ------------------------------------------
 * One row per record: QNAME FLAG RNAME POS MAPQ CIGAR * 0 TLEN SEQ * ET:i:<equally good templates> AS:i:<score>, QNAME = the read header up
 * to its first TAB, MAPQ = min(254, mapQ), POS = start + 1, TLEN = end - POS, SEQ = the fragment as filed (N's restored). Which records, with
 * `level` = the option's value (1 for a bare -sam):
 *   1  reads stage 2 passed nothing on for (n_hits 0, tmpl 0, flag & 4 clear), only when level == 1 (kmers.c:70, savekmers.c:205-248):
 *      FLAG 20, RNAME *, POS 0, MAPQ 0, CIGAR *, TLEN 0, ET 0, AS 0, SEQ = the read as stage 1 packed it
 *   2  reads stage 3a rejected (tmpl 0, flag & 4), only when level == 1 (runkma.c:348, alnfrags.c:2262-2273): FLAG = flag, otherwise as
 *      above, SEQ = the read as stage 2 passed it on (rc bit 0)
 *   3  the filed fragments (tmpl != 0) of every template, templates ascending, in assemble_KMA's order (that of the fragment rows, counted
 *      over ALL filed fragments): 3a kept by the read filter (the rows of `.frag.gz`): FLAG = flag | 16 for a template of negative sign;
 *      3b dropped with read_score != 0 (kmahip_trace_drops): an aligned record all the same, AS = read_score; 3c / 3d everything else that
 *      was filed (read_score 0, nothing to align, or a template the significance gate skips: tmpl_ok 0): FLAG | 4, RNAME = the template,
 *      POS 0, MAPQ 0, CIGAR *, TLEN 0, AS 0. 3b - 3d only when !(level & 2096) (assembly.c:1995-2015; the reference's own test, kept).
 * Order: class 1 in stream order, class 2 in stream order, class 3 (the reference's stages 2 and 3a run beside each other under -sam and
 * interleave their rows differently from run to run; what it prints with a template name comes in this order every time).
 *
 * kmahip_sam_cigar: the CIGAR of one record (makeCigar: <clip_start>S, the runs as =XID, <clip_end>S), 0-terminated, into out[cap]; returns
 * its length or KMAHIP_EOVERFLOW. kmahip_sam_row_host: one whole row from host values (rname NULL = "*", runs NULL = CIGAR "*", seq = the
 * bases as text); returns its length (no terminator is written) or KMAHIP_EOVERFLOW. Pure host code: the checkers of the device's text. */
#define KMAHIP_VERSION "0.9.0"
const char *kmahip_version(void);
int64_t kmahip_sam_cigar(const uint32_t *runs, int64_t n, int32_t clip_start, int32_t clip_end, char *out, int64_t cap);
int64_t kmahip_sam_row_host(const char *header, int32_t flag, const char *rname, int32_t pos, int32_t mapq, const uint32_t *runs, int64_t n_runs,
                            int32_t clip_start, int32_t clip_end, int32_t tlen, const char *seq, int32_t et, int32_t as, char *out, int64_t cap);
/* The header (saminit): @HD, one @PG line ("@PG\tID:KMA\tPN:<program>\tVN:<KMAHIP_VERSION>\tCL:<cmdline>", CL left out for a NULL cmdline),
 * @SQ for every template in index order. path: a file (created or emptied), or "-" = standard output. */
int kmahip_sam_header(kmahip_db *db, const char *program, const char *cmdline, const char *path);
/* The rows of one batch that is the whole stream, APPENDED to path ("-" = standard output). HOST buffers in the mould of kmahip_frag_write3:
 * the reads, kmahip_hits.rc / kmahip_conclave.tmpl / kmahip_hits.n_hits / kmahip_hits.flag per read, the traces of kmahip_align_trace (stats,
 * ops_off, n_ops, and ops_cap entries of ops), the drop record with HOST arrays (NULL: no rows of class 3b), tmpl_ok per template (NULL =
 * all), frag_rank as in kmahip_assemble_opts, the read headers. Classified, ordered, measured and formatted on the device -- a lane per row,
 * or a wavefront per row for long reads (KMAHIP_SAM_GROUP=1 / 64 forces one) --, brought back as text a chunk at a time (KMAHIP_SAM_CHUNK
 * bytes, 64 MiB by default; a longer row gets a buffer of its own size) and written in order, uncompressed.
 * class_rows (may be NULL): rows of classes 1, 2, 3a, 3b, 3c + 3d. */
int kmahip_sam_write(const char *path, kmahip_db *db, const kmahip_reads *reads, const int32_t *rc, const int32_t *tmpl, const int32_t *n_hits,
                     const int32_t *flag, const kmahip_traces *traces, const kmahip_trace_drops *drops, const uint8_t *tmpl_ok, int64_t max_frag,
                     int order, const int64_t *frag_rank, const char *read_names, const int64_t *read_name_off, int level, int64_t *rows,
                     int64_t class_rows[5]);

/* The mapping quality the stage-3 kernels gate on with -mq (chainSeeds, chain.c:79-260: ceil(40 (1 - second / best) min(1, w / 10)
 * log(best)) in double, 0 for best <= 0), evaluated ON THE DEVICE by the one function all of those kernels call, for n triples in HOST
 * arrays. Exposed for tests: the device's log against the libm the reference links. */
int kmahip_test_mapq(const int32_t *best, const int32_t *second, const int32_t *w, int64_t n, uint32_t *out);
/* The list table (a second probe table whose value is a k-mer's value-list offset; the scan's queue and the wavefront-per-item kernels
 * look lists up in it): for n keys in a HOST array, one lane per key, out_list[i] = the list table's answer and out_via_pos[i] = the
 * list offset filed at the position the probe table answers with; 0xFFFFFFFF = not in the index. The two must agree for every key.
 * KMAHIP_LTAB_FLAG is honoured as in a scan launch. KMAHIP_EINVAL when the database has no list table. Exposed for tests. */
int kmahip_test_list_probe(kmahip_db *db, const uint32_t *keys, int64_t n, uint32_t *out_list, uint32_t *out_via_pos);
/* log2 of the list table's bucket count (the probe table's + 1, or the same with KMAHIP_LTAB_SHIFT=0 in the environment of the
 * open), 0: the database has none (KMAHIP_SCAN_LTAB=0 at the open, no memory for it, list offsets of 2^31 - 1 or more) */
int kmahip_db_list_table_log2(const kmahip_db *db);
/* The neighbour move of the cooperative DP sweep (a DPP row or wavefront shift in place of __shfl_down(x, 1, w)), on one wavefront:
 * out[l] = what lane l receives of in[0..64), w = 8, 16, 32 or 64 lanes per segment. What the last lane of a segment receives is
 * unspecified (the sweep never uses it). Exposed for tests. */
int kmahip_test_lane_down(const int32_t *in, int w, int32_t *out);

/* The single-end run in KMA's DEFAULT mode (no -1t1) on one batch: kmahip_scan_chain, then every S2 record -- a read, or its
 * reverse complement where the record prints that, with its query bounds -- goes through stage 3a, ConClave, the `.res`
 * statistics, the traceback and the pile-up like a read of kmahip_run_se (runKMA, runkma.c:104-900 with kmerScan =
 * save_kmers_chain). A chimeric read therefore counts once per chain. `names` / `name_off`: read headers for the `.frag(.gz)`
 * rows written to frag_path (both NULL to skip the file). out->tmpl / n_hits / rc / trace_stats are not filled (the records
 * are not the caller's reads); rows, assembly and ms are as in kmahip_run_se. */
int kmahip_run_chain(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const char *names, const int64_t *name_off,
                     const kmahip_params *p, const kmahip_chain_params *cp, double evalue, int bcd, int64_t max_frag,
                     const char *frag_path, kmahip_run *out);

/* The paired run (`-ipe r1 r2 -apm p -1t1`) on one batch as kmahip_ingest_next hands it over for two mate files: reads in
 * stream order, batch->pair[i] = 1 / 2 for the mates of a pair record, 0 for a record that lost its mate to the trimming.
 * Pairs go through kmahip_map_pe, single records through kmahip_map_se; their results are merged into frag_raw records in
 * stream order (alnFragsPenaltyPE's record forms: proper pair -- second slot first when the pair was swapped --, unmated,
 * one mate only, alnfrags.c:1777-1970), ConClave over the records, the `.res` statistics, the traceback aligner over the
 * fragments in record order and the pile-up. Fills out->rows / n_rows / assembly / ms (the per-read pointers of `out` are
 * not used: fragments are not in read order); frag_path != NULL also writes the `.frag.gz`. HOST buffers. */
int kmahip_run_pe(kmahip_db *db, kmahip_ws *ws, const kmahip_read_batch *batch, const kmahip_params *p, double evalue, int bcd,
                  int64_t max_frag, const char *frag_path, kmahip_run *out);

/* Paired input in KMA's DEFAULT mode (`-ipe r1 r2` without -1t1): the reference's batch loop hands a couple to save_kmers_pair
 * and a record that lost its mate to kmerScan (save_kmers_batch, savekmers.c:171-200), which without -1t1 is save_kmers_chain
 * (savekmers.c:40) -- the couples are mapped exactly as under -1t1 (one2one only guards a branch of anker_rc / anker_rc_comp no
 * seeded read reaches, align.c:964,1157), a single record yields the chain finder's records with their query bounds. With `cp`
 * set on the workspace every paired run on it (kmahip_run_pe, kmahip_run_pe_sharded, a session after kmahip_session_set_pe)
 * does that: each record of a single read is a unit of the stream where its read stood, and goes through stage 3a, ConClave,
 * the traceback and the `.frag.gz` like a record of kmahip_run_chain. NULL: back to -1t1 (single records through save_kmers). */
int kmahip_ws_set_pe_chain(kmahip_ws *ws, const kmahip_chain_params *cp);

/* -ck, "count k-mers over pseudo alignment" (kma.c:689), off on a new workspace. on != 0: stage 2 of every run on this workspace that
 * scans k-mers for the single-end -1t1 run or for pairs scores a template by ONE point per k-mer start of the read whose value list
 * holds it -- save_kmers_count (savekmers.c:3067-3365) in place of save_kmers (:2442-3065), get_kmers_for_pair_count (:690-824) in
 * place of get_kmers_for_pair (:427-688), chosen at kma.c:1272-1276 -- on the device by scan_count_kernel. A single-end record is
 * written when kmersize <= the best count of either strand (:3343); the pairing functions, kmahip_params::minFrac on single-end
 * input, the decon filter and every stage behind stage 2 are the same. Read by kmahip_scan_se* / kmahip_scan_pe* and everything
 * that runs them (kmahip_map_se / _pe, kmahip_run_se / _pe, the sessions, the sharded runs); kmahip_scan_chain and the chain runs
 * (the default mode on single-end input) and kmahip_run_mt1 do not read it, like the reference. The setting lives on the workspace
 * and not in kmahip_params, whose layout stays as it is. */
int kmahip_ws_set_count_kmers(kmahip_ws *ws, int on);

/* Multi-GPU (one process per GPU): in-place SUM over all ranks of the two ConClave
 * vectors on `stream`, through RCCL (ncclAllReduce, ncclUint64, ncclSum).
 * `nccl_comm` is an ncclComm_t the host program created (ncclCommInitRank);
 * librccl is resolved at run time, the library does not link against it. */
int kmahip_allreduce_scores(void *nccl_comm, uint64_t *alignment_scores, uint64_t *uniq_alignment_scores,
                            size_t DB_size, void *stream);

/* ---- several GPUs of one node: one process per GPU, the reads sharded over the ranks -----------------------------
 * The reference is one process (threads over pipes, kmapipe.c:55-146); these entries are what a read-sharded host needs between
 * its stages: the SUM of alignment_scores / uniq_alignment_scores before runConClave (runkma.c:563-594, updatescores.c:228,276),
 * the SUM of ConClave's per-template outputs before the `.res` statistics (conclave.c:147-151, runkma.c:608-613, 770-783), and the
 * exchange that brings every traced read to the rank that owns its template, in the order of the whole stream (the assembly
 * order of conclave.c:164-196 and assembly.c:1377-1424 is made of it).
 * A communicator is bootstrapped through a POSIX shared-memory segment named after `key` (every rank of one run passes the same
 * key, no two runs at a time the same one); backend "rccl": device data moves with ncclAllReduce / ncclSend / ncclRecv over xGMI
 * (one device per rank), "shm": staged through host memory (any number of ranks per device: rehearsals and tests). */
typedef struct kmahip_comm kmahip_comm;
int kmahip_comm_init(int rank, int world, const char *key, const char *backend, kmahip_comm **out);
void kmahip_comm_destroy(kmahip_comm *c);
int kmahip_comm_rank(const kmahip_comm *c);
int kmahip_comm_world(const kmahip_comm *c);
int kmahip_comm_is_rccl(const kmahip_comm *c);
/* One line about the communicator for a log or a JSON record: "backend=rccl rank=R world=W rccl_nranks=N rccl_rank=R
 * rccl_version=V allreduces=A alltoallvs=B" -- nranks / rank / version as RCCL itself reports them (ncclCommCount,
 * ncclCommUserRank, ncclGetVersion), A and B the exchanges that went through it so far --, or "backend=shm|none rank=R world=W".
 * Returns what snprintf returns. With KMAHIP_COMM_FORCE_RCCL=1 a ONE-rank communicator of backend "rccl" is a real RCCL
 * communicator too (kmahip_comm_init runs a SUM all-reduce and a grouped send / recv through it before it returns, as it does
 * for every RCCL communicator): the transport can be exercised on a box with a single device. */
int kmahip_comm_describe(const kmahip_comm *c, char *buf, size_t cap);
int kmahip_comm_barrier(kmahip_comm *c);
/* every rank posts `bytes` (at most 64 KiB) of HOST memory and gets all ranks' back in rank order */
int kmahip_comm_allgather(kmahip_comm *c, const void *mine, size_t bytes, void *all);
/* in-place SUM over the ranks of n u64 values in DEVICE memory */
int kmahip_comm_allreduce_u64(kmahip_comm *c, uint64_t *d_buf, size_t n, void *stream);
/* all-to-all of byte blocks: send_bytes[d] bytes for rank d back to back in `send`; recv_bytes[s] from rank s land back to back
 * in `recv` in rank order (the sizes are agreed on beforehand, e.g. through kmahip_comm_allgather). device != 0: DEVICE buffers. */
int kmahip_comm_alltoallv(kmahip_comm *c, const void *send, const int64_t *send_bytes, void *recv, const int64_t *recv_bytes,
                          int device, void *stream);

/* Stage 1 for one rank of a sharded run: the part `part` of `parts` of the input. FASTQ in a plain file (single end): the rank
 * parses only its byte range -- ranges are cut at record starts found by the reader's own guess (a line beginning with '@' whose
 * next line but one begins with '+'), the same on every rank, so the parts tile the file; *whole_input = 0. Anything else (.gz,
 * FASTA, two mate files): the reader delivers the whole input and *whole_input = 1 -- the caller keeps the records
 * [n part / parts, n (part + 1) / parts) of it. path2 == "" (the empty string) asks for the interleaved reader of
 * kmahip_ingest_open_interleaved on path1. */
int kmahip_ingest_open_part(const char *path1, const char *path2, const kmahip_trim *trim, int part, int parts, kmahip_ingest **out,
                            int *whole_input);

/* The single-end `-1t1` run of kmahip_run_se + the three writers, with the reads sharded over the ranks of `comm` (NULL or a
 * one-rank communicator: everything on this device). `batch`: this rank's contiguous part of the input stream, in stream order
 * over the ranks. Each rank maps its reads (stages 2, 3a), the score vectors are summed, ConClave runs per shard on the global
 * vectors, its per-template outputs are summed (every rank then computes the same `.res` statistics), the traceback runs on the
 * rank's own reads, and every kept read travels to the owner of its template (contiguous template ranges, balanced by filed
 * fragments) with its position among the filed fragments of the whole stream; the owners pile up, call the consensus and write
 * the rows of their templates to <out_prefix>.part<rank>.res, .fsa and .frag.gz. Rank 0 then concatenates the parts in
 * rank order (= template order; gzip members concatenate) into <out_prefix>.res / .fsa / .frag.gz -- byte for byte the files of
 * the one-device run (tests/test_shard_gpu.py). ms[8]: upload, stages 2 + 3a, exchange 1 + ConClave + exchange 2, traceback,
 * gather by owner, pile-up + consensus, writers, merge. */
typedef struct kmahip_shard_opts {
	double evalue;        /* -e, 0.05 */
	int32_t bcd;          /* -bcd, 1 */
	int32_t caller, sig90;/* -bcNano: 1, 1 */
	int64_t max_frag;     /* -mf, <= 0: 1000000 */
	double ID_t, Depth_t; /* -ID (1.0), -md (0.0) */
	double support;       /* -bc x with sig90 == 2 */
	int32_t ref_fsa;      /* the consensus file: 0 gap columns left out, 1 gaps as n (-ref_fsa), 2 as they are (-ref_fsa 0; printconsensus.c:38-60) */
	int32_t write_aln;    /* != 0: <prefix>.aln as well (printConsensus printconsensus.c:26-37; the reference writes it unless -na) */
	int32_t vcf_support_own; /* sessions with kmahip_session_set_vcf. 0: the `.vcf.gz` rows and their FILTER column test AD against support * DP
	                       * (vcf.c:195-204), as `-bc x` has it. != 0: against vcf_support * DP. The reference keeps the callers' threshold
	                       * (significantAndSupport's static, assembly.c:153) and the variable it hands updateVcf apart, and its presets -mint2 /
	                       * -mint3 set the first alone (kma.c:1092, 1112): vcf_support = 0 there unless a `-bc x` stands beside them */
	int32_t pad_;
	double vcf_support;
} kmahip_shard_opts;
/* One template's block of the `.aln` file: "# name", then per 60 alignment columns the lines "template:", the match line ('|' where
 * the call equals the template's base, '_' elsewhere) and "query:", of the alignment as assemble_KMA trims it (assembly.c:2094-2119:
 * without the insertion columns called as gaps). cons: the template's consensus string from kmahip_assemble2 / kmahip_run_* with
 * caller + 32. Returns the number of bytes written to out (no terminator), -1 on an error (cap too small: (columns / 60 + 2) * 224 +
 * strlen(name) + 16 always suffices). Host memory; reads <prefix>.seq.b the first time. */
int64_t kmahip_aln_entry(kmahip_db *db, int32_t tmpl, const char *name, const char *cons, char *out, int64_t cap);
int kmahip_run_se_sharded(kmahip_db *db, kmahip_ws *ws, kmahip_comm *comm, const kmahip_read_batch *batch, const kmahip_params *p,
                          const kmahip_shard_opts *opts, const char *out_prefix, double ms[8]);
/* The default mode (no -1t1; kmahip_run_chain) over read shards: stage 2 -- save_kmers_chain -- on the rank's reads, its records (a
 * read or its pieces with their query bounds) in stream order, and from there the stages and exchanges of kmahip_run_se_sharded on
 * records instead of reads; a fragment row carries the header of the read its record came from. cp: NULL = the defaults. */
int kmahip_run_chain_sharded(kmahip_db *db, kmahip_ws *ws, kmahip_comm *comm, const kmahip_read_batch *batch, const kmahip_params *p,
                             const kmahip_chain_params *cp, const kmahip_shard_opts *opts, const char *out_prefix, double ms[8]);
/* `-Mt1 tmpl [-bcNano]` (kmahip_run_mt1; runKMA_Mt1 mt1.c:86-500) over read shards: every rank traces its contiguous part of the stream
 * against the one template (the traceback is four fifths of that run), the Score and the number of kept reads are summed, and the kept
 * reads travel to the template's owner (rank 0) with their positions among the kept reads of the whole stream, where they are piled
 * up in stream order. Files as kmahip_run_se_sharded leaves them, identical to the one-process run. */
int kmahip_run_mt1_sharded(kmahip_db *db, kmahip_ws *ws, kmahip_comm *comm, const kmahip_read_batch *batch, int32_t tmpl, int one2one,
                           const kmahip_params *p, const kmahip_shard_opts *opts, const char *out_prefix, double ms[8]);
/* The paired run (`-ipe r1 r2 -apm p -1t1`, kmahip_run_pe) the same way. `batch`: this rank's contiguous part of the stream of
 * units (pairs and single records; a pair is never cut). On top of the three exchanges above, two things cross the shards because
 * runConClave walks ONE stream: a record whose hit list came out empty takes the first listed hit of the last record before it
 * that had one (conclave.c:123-127) -- the shards hand that hit on --, and the chunks of maxFrag filed fragments close one after
 * the other (conclave.c:164-196) -- the ranks count theirs in turn. */
int kmahip_run_pe_sharded(kmahip_db *db, kmahip_ws *ws, kmahip_comm *comm, const kmahip_read_batch *batch, const kmahip_params *p,
                          const kmahip_shard_opts *opts, const char *out_prefix, double ms[8]);

/* ---- the single-end `-1t1` run fed batch by batch: the host holds one batch at a time ------------------------------------------
 * The reference streams its input through pipes and spills the frag_raw records of stage 3a to a temporary file that ConClave
 * and the assembly read back once the input has ended (kmapipe.c:55-146, updatescores.c:283-295, runkma.c:563-594, 757-863). Here
 * HBM is that temporary file: kmahip_session_add uploads a batch of kmahip_ingest_next (reads, N positions, headers) behind the
 * batches before it, runs stages 2 and 3a on it and adds into the ConClave vectors -- the batch's host arrays may be reused when it
 * returns; kmahip_session_finish runs ConClave and the traceback per batch, one pile-up + consensus over everything, and writes
 * <out_prefix>.res, .fsa (write_fsa) and .frag.gz (write_frag) -- the fragment rows are ordered, measured and formatted on the
 * device and come back as text a chunk at a time for the host's threads to compress. Files byte for byte those of kmahip_run_se +
 * kmahip_frag_write (the .gz after inflating). opts: evalue, bcd, caller / sig90, max_frag, ID_t, Depth_t as in
 * kmahip_run_se_sharded; reads_hint: an estimate of the number of reads (0: none), sizes the device arrays up front.
 * ms[8]: uploads and stages 2 + 3a (each summed over the batches), ConClave + statistics, traceback, pile-up + consensus,
 * .res + .fsa, fragment rows. */
typedef struct kmahip_session kmahip_session;
int kmahip_session_open(kmahip_db *db, kmahip_ws *ws, const kmahip_params *p, const kmahip_shard_opts *opts, int64_t reads_hint, kmahip_session **out);
/* Paired input (`-ipe r1 r2 -apm p -1t1`; kmahip_run_pe) through the session: the batches of a paired reader (kmahip_ingest_open with
 * two files: batch->pair says which reads are mates; a batch never ends inside a couple) are uploaded behind each other like single-end
 * ones -- the host holds one batch at a time --, the first one is run through the stages once to pay for first launches and scratch
 * while stage 1 reads on, and kmahip_session_finish runs kmahip_run_pe's stages on everything and writes the files. Before the first
 * batch. */
int kmahip_session_set_pe(kmahip_session *s);
/* The reference's DEFAULT mode (no -1t1: kmahip_run_chain) through the same session: call once, before the first batch. A batch's
 * reads then go through the chain finder, and what the session keeps and maps are its records (a read, or its pieces, with their query
 * bounds); a fragment row carries the header of the read its record came from. cp: NULL = the defaults (kmahip_scan_chain). */
int kmahip_session_set_chain(kmahip_session *s, const kmahip_chain_params *cp);
/* `-Mt1 tmpl` (kmahip_run_mt1; runKMA_Mt1, mt1.c:86-500) through the same session: call once, before the first batch. There is no
 * stage 2 and no ConClave in this mode, and a read's traceback depends on nothing but the read: kmahip_session_map seeds and traces
 * the batch's reads against the template right away -- beside stage 1 of the next batch -- and keeps their figures and alignment runs
 * in HBM; kmahip_session_finish sums the `.res` row, piles everything up in stream order and writes the three files (those of
 * kmahip_run_mt1 + kmahip_frag_write2 with order 1). frag_path (or NULL): the fragment file -- its rows depend on nothing but their
 * reads either, so each batch's rows are formatted on the device and handed to the compressing threads as soon as the batch is traced;
 * kmahip_session_finish then only ends the file (its write_frag is ignored; with NULL here and write_frag set, the file is written at
 * the finish as <out_prefix>.frag.gz). ms[] of kmahip_session_finish: [1] the tracebacks, [3] nothing, [7] the fragment rows made
 * beside the batches. */
int kmahip_session_set_mt1(kmahip_session *s, int32_t tmpl, int one2one, const char *frag_path);
/* SAM records of the run (`-sam [n]`; kmahip_sam_write has the record classes and their order): call before the first batch. level = the
 * option's value (1 for a bare -sam), path = where header and rows go ("-" = standard output), program / cmdline = the @PG line's PN and CL.
 * The session then keeps every read's stage-3a flag, lets its traceback keep what the read filter drops (kmahip_trace_drops, when the level
 * prints such rows) and kmahip_session_finish writes the SAM beside `.res` / `.fsa` / `.frag.gz`, which stay byte for byte what they are
 * without it. Serves the single-end `-1t1` session at every level and the paired one (kmahip_session_set_pe) at levels other than 1: the
 * filed fragments of kmahip_run_pe's records, each with its record's flag, in the fragment rows' order. KMAHIP_EINVAL, naming the mode,
 * for a session in the default mode, `-Mt1`, or with paired input at level 1 (the unmapped-mate flags of stages 2 and 3a are not built). */
int kmahip_session_set_sam(kmahip_session *s, int level, const char *path, const char *program, const char *cmdline);
/* The extended-features file (`-ef`): call before the first batch. The session then asks ConClave for its read and fragment counts,
 * runs kmahip_assemble_ef_dev behind the pile-up and writes <out_prefix>.mapstat beside `.res`, from the same loop over the rows: a
 * template is in both files or in neither. cmdline: the `## command` line (NULL: empty). t_db: the `## database` value (NULL: the
 * prefix the index was opened with). Served by the -1t1 sessions (single end and paired) and the default mode; a -Mt1 session writes no
 * such file, as runKMA_Mt1 writes none (mt1.c:313, 378). */
int kmahip_session_set_ef(kmahip_session *s, const char *cmdline, const char *t_db);
/* ... its `## fragmentCount`: the records stage 1 passed on (kmahip_read_batch.records summed over the batches, a couple counting
 * once). Only the reader knows it, and only when the input has ended: call before kmahip_session_finish. */
int kmahip_session_set_ef_fragments(kmahip_session *s, int64_t records);
/* The count matrix (`-matrix`) and the VCF file (`-vcf [n]`): call before the first batch. The session then runs
 * kmahip_assemble_matrix_dev / kmahip_assemble_vcf_dev behind the pile-up, for the templates whose `.res` row passes its gate, and writes
 * <out_prefix>.mat.gz / <out_prefix>.vcf.gz from the loop that writes `.res`: a template is in all files or in none. level: the value of
 * -vcf (1, or 2 to fill the FILTER column); t_db: the last column of the header line (NULL: the prefix the index was opened with).
 * Served by every session: -1t1 single end and paired, the default mode, -Mt1 (runKMA_Mt1 writes both, mt1.c:445-450). */
int kmahip_session_set_matrix(kmahip_session *s);
int kmahip_session_set_vcf(kmahip_session *s, int level, const char *t_db);
int kmahip_session_add(kmahip_session *s, const kmahip_read_batch *batch);
/* kmahip_session_add in two steps, for a caller whose reader thread is to go on while the device works: _upload returns when the
 * batch's host arrays are free again, _map runs stages 2 and 3a on what has been uploaded since the last call */
int kmahip_session_upload(kmahip_session *s, const kmahip_read_batch *batch);
int kmahip_session_map(kmahip_session *s);
/* kmahip_session_upload for a batch that is on the device already (kmahip_ingest_dev_next: what the reference's stage 1 writes into
 * its pipe, kmapipe.c:55-146, never leaves HBM): device-to-device placement behind the batches before it; the batch's arrays are free
 * when it returns. For the `-1t1` single-end and paired sessions; KMAHIP_EINVAL for a session in the default mode or `-Mt1`, whose
 * hosts need the host arrays. A failing call leaves the session as it was. */
int kmahip_session_upload_dev(kmahip_session *s, const kmahip_read_batch *dev_batch);
int kmahip_session_finish(kmahip_session *s, const char *out_prefix, int write_fsa, int write_frag, int64_t *n_reads, int64_t *n_rows, double ms[8]);
void kmahip_session_close(kmahip_session *s);

/* Status of the *_dev calls issued on this workspace since the last query; synchronises `stream`. 0, or KMAHIP_EOVERFLOW
 * with kmahip_last_error() naming one of:
 *   - the library's own candidate pool ran out (stage 2): the pool has been doubled, repeat the scan call (and what
 *     followed it) -- no caller capacity is involved;
 *   - T_cap (kmahip_cands / kmahip_pe_recs) or ops_cap (kmahip_traces) too small: T_off[n] / R_off[2n] holds the needed
 *     size. A kmahip_align_*_dev call queued behind such a scan touches nothing beyond the capacities (it reports no hits),
 *     so scan_dev + align_dev may be chained on a stream without a status check in between;
 *   - more MEMs per (read, template) pair than the align scratch holds (a read full of repeats): the capacity has been raised
 *     fourfold, repeat the align (score vectors zeroed again) or trace call; the one-call runs (kmahip_run_*) do that themselves;
 *   - a DP problem beyond the trace scratch.
 * The status word is sticky until read here. */
int kmahip_ws_status(kmahip_ws *ws, void *stream);

/* Algorithmic work counters of the last scan on this workspace (read after a sync): probes = k-mer starts
 * whose value set was resolved (= hashMap_get calls of the reference), hash_probes = those that actually went
 * to the probe table (the rest were read off the template store while walking a match). */
typedef struct kmahip_scan_stats {
	uint64_t probes;
	uint64_t value_elems;
	uint64_t active_strands;
	uint64_t hash_probes;
	uint64_t prefilter_probes;   /* of probes / hash_probes: those issued by scan_prefilter_kernel */
} kmahip_scan_stats;
/* same for the last align call: template-index lookups, bases inside MEMs,
 * DP cells filled, (read, candidate) tasks aligned */
typedef struct kmahip_align_stats {
	uint64_t lookups;
	uint64_t mem_bases;
	uint64_t dp_cells;
	uint64_t tasks;
} kmahip_align_stats;
int kmahip_align_get_stats(kmahip_ws *ws, kmahip_align_stats *st, void *stream);
/* counting costs atomics in the kernel: off by default */
int kmahip_scan_set_stats(kmahip_ws *ws, int on);
int kmahip_scan_get_stats(kmahip_ws *ws, kmahip_scan_stats *st, void *stream);
/* How the last scan launch on this workspace handed its live strand items to the first tier: out[0] as self-contained
 * records (reads without N's of at most 192 bases, outside the exhaustive mode), out[1] as bare list entries (everything else,
 * and every item with KMAHIP_SCAN_REC=0 in the environment). Read it before another stage is launched on the workspace. */
int kmahip_ws_scan_routes(kmahip_ws *ws, void *stream, unsigned long long out[2]);
/* Strand items of the last scan launch whose candidates did not fit the first tier's table (out[0]: handed to the second tier, 64
 * slots) and not the second tier's either (out[1]: handed to scan_dense_kernel, a wavefront per item on tables as wide as the
 * database). Read it before another stage is launched on the workspace. */
int kmahip_ws_scan_overflow(kmahip_ws *ws, void *stream, unsigned long long out[2]);
/* Records of the last scan launch whose template diagonal the prefilter replaced: it counts the bases of the read that differ
 * from the template store along the diagonal of its first hit and, at two or more, looks up the read's k-mer that ends at the first
 * of them and files that hit's diagonal when fewer bases differ along it (KMAHIP_SCAN_REFINE=0 in the environment: never). Counted
 * only while kmahip_scan_set_stats is on; read it before another stage is launched on the workspace. */
int kmahip_ws_scan_diag_replaced(kmahip_ws *ws, void *stream, unsigned long long *out);
/* The queue round of the last scan launch: out[0] the k-mer starts that the lanes of the LDS tiers left to be looked up one by one
 * (behind a base off the diagonal, a miss or a cut walk), out[1] the rounds -- one per workgroup's group of strand items and pass of 136
 * starts -- that had any. Counted only while kmahip_scan_set_stats is on; read it before another stage is launched on the workspace. */
int kmahip_ws_scan_queue_counts(kmahip_ws *ws, void *stream, unsigned long long out[2]);
/* Record items of the last scan launch that the prefilter settled itself: the read lies on the template store along its diagonal
 * without a mismatch, and the span table (below) says that the k-mers of that stretch leave its template as the only best one. They
 * are counted among the records of kmahip_ws_scan_routes and never reach the first tier. Always counted. Off (0) outside the
 * best-templates mode of kmahip_launch_scan_se, under -proxi, -ex_mode, -ck, a decon database, a scoring scheme that is not
 * M > 0, MM < M, U <= 0, W1 <= 0, and with KMAHIP_PF_SETTLE=0 in the environment. Read it before another stage is launched. */
int kmahip_ws_scan_settled(kmahip_ws *ws, void *stream, unsigned long long *out);
/* The span table as it lies on the device, built by kmahip_db_open (KMAHIP_SCAN_SPAN=0: not built): for the first n positions p of
 * the concatenated templates (template 1 first; at most total bases + 64) t0 = the template p lies in, room = the k-mer starts from p
 * on inside t0 whose value lists name t0 (capped at 255), need = the fewest of them whose value lists have t0 alone in common (255: never); all 0 where no
 * k-mer starts. HOST arrays. Returns 1, 0 when the database has no table, or an error. Exposed for tests. */
int kmahip_test_span_table(kmahip_db *db, int64_t n, uint32_t *out_t0, uint8_t *out_need, uint8_t *out_room);
/* Stage 3a's device-wide queues after the last alignment launch on the workspace (the register-only route, which hands its DP
 * problems of 2..63 query columns to four class queues that one kernel sweeps): out[0..3] entries of the classes of 33..63,
 * 17..32, 9..16 and 2..8 columns, out[4] tasks that waited for queued problems (the last result to arrive finishes such a task),
 * out[5] hand-ons to the general kernel over the queues: tasks that gave up behind a problem they had queued, plus entries that
 * found no room (KMAHIP_ALIGN_DQ_CAP=<n> in the environment caps the entries per queue: tests and timing only). */
int kmahip_ws_align_queue_counts(kmahip_ws *ws, void *stream, unsigned long long out[6]);
/* The traceback of reads up to 1 kb settles in a first pass every read whose DP problems are provably ungapped and puts the others
 * off to a pass with move matrices: out[0] the reads the last such launch on the workspace put off, out[1] those of them that the pass
 * with the matrices in LDS (KMAHIP_TRACE_LDS=1 in the environment) put off once more. Both 0 after a launch of that kernel
 * in one pass (a scheme without the shortcut, KMAHIP_TRACE=lanes1); the long-read pipeline leaves them as they were. Read it before
 * another stage is launched on the workspace. */
int kmahip_ws_trace_put_off(kmahip_ws *ws, void *stream, unsigned long long out[2]);
/* The scoring schemes under which stage 3a and the traceback may take a DP problem's diagonal for its answer without the matrix: the
 * most mismatches between two seeds up to which they do, -1 for a scheme under which they never do (host arithmetic; both stages call
 * this one function). */
int kmahip_diag_gap_m_max(const kmahip_rewards *rw);

/* work figures of the last long-read trace call on this workspace (kmahip_align_trace_mt1*, kmahip_run_mt1, or the trace stage
 * on reads over 1 kb): DP problems solved, their cells (rows x columns; rows x (band + 1) for banded ones), MEMs of the chained
 * strands, reads */
typedef struct kmahip_trace_stats {
	uint64_t problems, dp_cells, mems, reads;
} kmahip_trace_stats;
int kmahip_trace_get_stats(kmahip_ws *ws, kmahip_trace_stats *st);
/* DP problems of the same call by the size class that solved them, summed over the call's passes: out[0..16] the wavefront classes
 * (0-3 lt_dp_kernel of 8 / 16 / 32 / 64 columns; 4-7 lt_dpx_kernel with the move matrix in LDS: full 2 / 4 columns a lane, banded
 * 2 / 4; 8 the one-lane kernel; 9-12 as 4-7 with the move matrix in HBM; 13, 14 unused; 15, 16 banded, 8 / 16 columns a lane),
 * out[17..25] the lane classes 0..8 (rows of 16 / 32 / 48 / 64 / 128 / 256 cells, bands of up to 72 / 96 / 144). Degenerate joins
 * (a pure insertion or deletion) are in no class. */
int kmahip_trace_get_class_counts(kmahip_ws *ws, unsigned long long out[26]);
/* which route the reads of the last default-mode stage 2 call on this workspace took (kmahip_scan_chain, or stage 2 of a whole run
 * without -1t1): out[0] reads of the call; out[1] reads chain_anchor_kernel handed over (N's, more than 288 k-mer starts, more than 32
 * anchors on a strand); out[2] reads chain_fast_kernel gave up (more candidate templates than its LDS table holds); out[3] reads the
 * long-read route took; out[4] reads chain_kernel took. out[1] + out[2] == out[3] + out[4]; with KMAHIP_CHAIN=slow out[4] == out[0]
 * and the rest is 0. */
int kmahip_chain_get_route_counts(kmahip_ws *ws, unsigned long long out[5]);

/* Kernel timing: when on, every *_dev call records a HIP event pair around its
 * main kernels (scan_prefilter_kernel, scan_se_kernel, seed_tasks_kernel, align_tasks_kernel) on the caller's stream; get_timing waits
 * for them, returns the summed milliseconds and launch count, and resets. */
int kmahip_ws_set_timing(kmahip_ws *ws, int on);
int kmahip_ws_get_timing(kmahip_ws *ws, int kernel /* 0 scan_se_kernel, 1 align_tasks_kernel, 2 scan_prefilter_kernel, 3 seed_tasks_kernel */,
                         double *total_ms, int64_t *launches);

/* ---- sparse mapping (`kma -Sparse`, sparse.c:338-797): no alignment; the k-mers of the reads that the index holds are counted, the
 * templates ranked on those counts and named one by one, a named template's k-mers withdrawn from all the others; one row per named
 * template in <out>.spa. A pipeline of its own beside the mapping one (sparse.hip): kmahip_db_open keeps refusing sparse indexes.
 *
 * kmahip_sparse_open reads <prefix>.comp.b (hashed or direct-address form; prefix_len / prefix from its header, `-Sparse -` gives
 * 0 / 1), <prefix>.length.b as load_DBs_Sparse does (sparse.c:133-177: the first array is skipped, then the lengths, then the unique
 * lengths) and <prefix>.name; no .seq.b. On the device: a probe table k-mer -> k-mer id (the 32-byte buckets of the mapping index),
 * the offset of every id's value list, the value lists, and one 32-bit count per id (the `int value` of HashMap_kmers,
 * hashmapkmers.h:24-28). Refused with KMAHIP_EFORMAT and the reason in kmahip_last_error: an index without a prefix, k > 16,
 * flag != 0 (minimizer / homopolymer indexes), a .length.b without unique lengths ("DB needs to sparse indexed, to run a sparse
 * mapping.", sparse.c:172). Not built: -Sparse with -deCon (collect_Kmers_deCon), several ranks, building sparse indexes. */
typedef struct kmahip_sparse kmahip_sparse;
typedef struct kmahip_sparse_info {
	uint32_t DB_size, kmersize, prefix_len, values_u16;
	uint64_t prefix, n_kmers /* k-mers held (= ids) */, n_hdr /* the header's n: templates->n of sparse.c:685 */, n_values, total_bytes;
} kmahip_sparse_info;
int kmahip_sparse_open(const char *prefix, kmahip_sparse **out);
void kmahip_sparse_close(kmahip_sparse *sdb);
int kmahip_sparse_get_info(const kmahip_sparse *sdb, kmahip_sparse_info *info);
/* template t's name (1 <= t < DB_size), its length and its unique length */
int kmahip_sparse_template(const kmahip_sparse *sdb, int32_t t, const char **name, uint32_t *len, uint32_t *ulen);

/* One batch of reads (host pointers; _dev: device pointers) added to the counts held by sdb: translateToKmersAndDump for flag == 0
 * (sparse.c:50-131) over both strands, branch for branch -- with a prefix per N-free stretch behind the strict gate
 * i < end - kmersize - prefix_len, the k-mer being the one that starts behind a prefix match; without one every k-mer of a stretch,
 * the walk resuming kmersize + 1 bases behind an N (:124) -- and save_kmers_sparse (:232-244): every k-mer produced counts into Ntot,
 * every one the index holds adds 1 to the count of its id. Undoes a collect: the scores are stale until the next one. */
int kmahip_sparse_count(kmahip_sparse *sdb, const kmahip_reads *reads);
int kmahip_sparse_count_dev(kmahip_sparse *sdb, const kmahip_reads *reads);
/* for tests: keys[i] / counts[i] of k-mer id i (n_kmers each; either may be NULL) and Ntot */
int kmahip_sparse_counts(kmahip_sparse *sdb, uint32_t *keys, uint32_t *counts, uint64_t *Ntot);
/* collect_Kmers (hashtable.c:54-120): every k-mer with a count > 0 becomes live and adds 1 / its count to Scores / Scores_tot of each
 * template of its list; Nhits.n / Nhits.tot. The working copies (w_Scores ...) start from these. */
int kmahip_sparse_collect(kmahip_sparse *sdb);
/* withDraw_Kmers (hashtable.c:224-270) on the working copies: every live k-mer whose list holds t by intpos_bin (:27-52, restated as
 * it stands) takes 1 / its count off every template of its list and dies */
int kmahip_sparse_withdraw(kmahip_sparse *sdb, int32_t t);
/* which: 0 = Scores / Scores_tot / Nhits of the last collect, 1 = the working copies. DB_size elements each; hits[2] = n, tot */
int kmahip_sparse_scores(kmahip_sparse *sdb, int which, uint32_t *scores, uint64_t *scores_tot, uint64_t hits[2]);

typedef struct kmahip_sparse_opts {
	double ID_t;       /* -ID (1.0) */
	double Depth_t;    /* -md (0.0) */
	double evalue;     /* -e / -p (0.05) */
	int32_t ss;        /* -ss: 'q', 'c' or 'd' */
	int32_t pad_;
} kmahip_sparse_opts;
void kmahip_sparse_default_opts(kmahip_sparse_opts *o);
/* one row of <out>.spa (sparse.c:766-774); ulen is what its Template_length column prints (:773) */
typedef struct kmahip_sparse_row {
	int32_t tmpl, expected;
	uint64_t score;
	uint32_t ulen, pad_;
	double query_cover, cover, depth, tot_query_cover, tot_cover, tot_depth, q_value, p_value;
} kmahip_sparse_row;
/* save_kmers_sparse_batch without decontamination (sparse.c:645-790): collect, then choose (host arithmetic in the host's libm on the
 * two downloaded vectors: the three -ss orders, the -ID / -md gates, p_chisqr, SearchList) and withdraw (a kernel) until nothing is
 * left. Up to cap rows are stored, *n_rows is their number (KMAHIP_EOVERFLOW when cap was too small). */
int kmahip_sparse_rows(kmahip_sparse *sdb, const kmahip_sparse_opts *opts, kmahip_sparse_row *rows, int64_t cap, int64_t *n_rows);
/* the rows as the reference prints them (header line, "%s\t%d\t%lu\t%d\t%d" and %8.2f columns, p_value %4.1e) into `path` */
int kmahip_sparse_write(kmahip_sparse *sdb, const kmahip_sparse_opts *opts, const char *path);
/* Timing and ablation. set_timing: event pairs around the kernels; get_timing sums them per kernel (0 count, 1 collect, 2 withdraw)
 * and resets. set_noadd(1): the counting kernel keeps its probes and drops its adds -- timing only, the counts are wrong by design. */
int kmahip_sparse_set_timing(kmahip_sparse *sdb, int on);
int kmahip_sparse_get_timing(kmahip_sparse *sdb, int kernel, double *total_ms, int64_t *launches);
int kmahip_sparse_set_noadd(kmahip_sparse *sdb, int on);

/* ---- template distances (`kma dist`, dist.c): for every pair of templates the k-mers they share, written as PHYLIP matrices under
 * thirteen measures. A pipeline of its own (tdist.hip) that reads nothing but <prefix>.comp.b and <prefix>.name and never looks at a
 * k-mer key, so it serves every form of index the reference writes: hashed and direct-address, k up to 32, sparse / prefix indexes,
 * minimizer and homopolymer flags -- the forms kmahip_db_open refuses included.
 *
 * kmahip_tdist_open reads the file as loadValues does (dist.c:38-162): the header; the direct-address array when size - 1 == mask,
 * else the bucket array is passed over; the values, 16-bit when DB_size < 65535, else 32-bit; for the hashed form the keys are passed
 * over (4 or 8 bytes each by mlen) and the n value indexes read; then the optional kmersize / flag. A short or inconsistent file:
 * KMAHIP_EFORMAT with `Wrong format of DB.` (the reference's words) in kmahip_last_error; so is a list that leaves the value array or
 * holds a template outside 1 .. DB_size - 1 (the reference walks them unchecked). Offsets beyond 32 bits are not served.
 * kmahip_tdist_open_lists is the same object over explicit arrays: offsets[n_kmers] are the per-k-mer entries (1 = none, as in the
 * file), values the [length, ids ...] lists with ids 1 .. n_templates, value_bytes 2 or 4; its templates are named by their ids. */
typedef struct kmahip_tdist kmahip_tdist;
typedef struct kmahip_tdist_info {
	uint32_t DB_size, mlen, kmersize, flag, prefix_len, direct /* 1: the direct-address form */, value_bytes, form /* of the last count: 0 rows, 1 pairs */;
	uint64_t n_kmers, n_lists /* distinct value lists */, n_values, name_bytes, total_bytes;
} kmahip_tdist_info;
int kmahip_tdist_open(const char *prefix, kmahip_tdist **out);
int kmahip_tdist_open_lists(uint32_t n_templates, uint64_t n_kmers, const uint32_t *offsets, const void *values, int value_bytes, uint64_t n_values,
                            kmahip_tdist **out);
void kmahip_tdist_close(kmahip_tdist *td);
int kmahip_tdist_get_info(const kmahip_tdist *td, kmahip_tdist_info *info);
/* the name of row t (0 <= t < DB_size - 1) */
int kmahip_tdist_name(const kmahip_tdist *td, uint32_t t, const char **name);
/* kmerSimilarity (dist.c:171-225): the per-k-mer entries are walked, entries equal to 1 passed over, the walk ends behind the n-th
 * live one; a list counts once per k-mer that points to it. N[t] = k-mers whose list holds template t + 1, D[hi][lo] (lower
 * triangle, hi > lo) = k-mers whose list holds both; int32 like the reference's int. A pair is (max, min) of the two ids.
 * KMAHIP_TDIST_FORM = rows | pairs chooses between the two forms of the pair sums (both give the same arrays). */
int kmahip_tdist_count(kmahip_tdist *td);
/* N (DB_size - 1 entries, may be NULL) and rows row_lo <= hi < row_hi of the triangle, row hi holding hi cells (D may be NULL) */
int kmahip_tdist_get_counts(kmahip_tdist *td, int32_t *N, int32_t *D, uint32_t row_lo, uint32_t row_hi);
/* the file of runDist / threadDist (dist.c:659-875): a matrix per bit of methods in the order 1, 2, 4 ... 4096, every cell 11 bytes
 * (`\t%10d`, `\t%10.6f`, `\t%.8f`), format & 1: names as they are (else `%-10.10s`), format & 4: a method line `# %-35s\n`; sizes as
 * getPhySize, the 11 NUL bytes behind each matrix with strict names included. The cells are formatted on the device in chunks of
 * KMAHIP_TDIST_CHUNK bytes (64 MiB). Where a requested measure would divide by zero -- a template with N = 0 under methods 4, 8, 256,
 * 512, 1024, 2048, two of them under 16, 32, 64, 128, 4096 -- KMAHIP_EINVAL, the template named (the reference prints -nan there, and its
 * chi-square dies of an integer division). */
int kmahip_tdist_write(kmahip_tdist *td, const char *path, int methods, int format);
/* test hook: n cells of `method` (one bit) from explicit triples, formatted on the device into 11 * n bytes */
int kmahip_test_tdist_cells(int method, const int32_t *Ni, const int32_t *Nj, const int32_t *D, int64_t n, char *out);
/* event pairs around the kernels; get_timing sums them per kernel (0 tdist_mult_kernel, 1 the inverted index with its scan, 2
 * tdist_rows_kernel, 3 tdist_pairs_kernel, 4 the write kernels) and resets */
#define KMAHIP_TDIST_KERNELS 5
int kmahip_tdist_set_timing(kmahip_tdist *td, int on);
int kmahip_tdist_get_timing(kmahip_tdist *td, int kernel, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
