// ingest_dev.hip -- stage 1 of KMA on the device (kmahip.h: kmahip_ingest_dev_*): FASTQ bytes -> trimmed, 2-bit packed read batches
// that are born in HBM. The spec is ingest.hip (locate_mem, pack_fastq, phred_stat, append_raw / append_read), which restates
// FileBuffgetFq (seqparse.c:241-403), run_input / run_input_PE (runinput.c:370-606), phredStat (:127-313) and compDNA
// (compdna.c:99-127); the batches here are, read for read, those of kmahip_ingest_next.
//
// Covered: FASTQ in plain regular files, single end and two mate files in lockstep, every field of kmahip_trim, phred 33 / 64, DOS
// line ends, N / IUPAC / lower case, reads of any length. NOT covered, and refused by kmahip_ingest_dev_open with KMAHIP_EFORMAT before
// any HIP call (the caller takes kmahip_ingest_open): .gz, FASTA, the interleaved reader, byte-range parts of sharded runs.
//
// The host reads file bytes into pinned buffers (parallel pread) and copies them up; everything per byte and per record is done here:
//   lines    a newline index of the chunk (count per block, scan, line starts). A chunk always begins at a record start, so record i is
//            lines 4 i .. 4 i + 3 whatever its quality line begins with;
//   shape    the first record that is not four well-formed lines (no '@', a quality line shorter than the sequence) ends the device's
//            part: from its byte offset on the host reader takes the rest of the input (kmahip_ingest_open_at), so that odd files and
//            "Malformed input" behave as they always did. The bytes behind the last complete record at the end of the input go the same way;
//   records  a thread per record index (it sees both mates): name span, end trimming or the -eq / -mi routine, length gate, pair flags;
//   scans    kept reads, packed words and name bytes -> where every read goes, in stream order;
//   pack     a group of lanes per read, a lane per 32-base word: the word, the N's it holds (scanned over the words -> N_off and the
//            N lists in a second pass), the header bytes.
#include "kmahip_internal.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <rocprim/rocprim.hpp>

// ingest.hip: the host reader from given byte offsets of its (plain, regular) files on, with the phred scale and the counts so far
int kmahip_ingest_open_at(const char *path1, size_t off1, const char *path2, size_t off2, const kmahip_trim *trim, int phred,
                          int64_t n_read, int64_t n_kept, kmahip_ingest **out);
// ... and its phred-scale guess (getPhredFileBuff), to2Bit table and 10^(-q/10) table: one copy of each for both readers
int kmahip_ingest_guess_phred(const uint8_t *buff, size_t bytes);
const uint8_t *kmahip_ingest_to2bit();
const double *kmahip_ingest_prob();

namespace {

constexpr size_t FIRST_CHUNK = 1048576;          // as ingest.hip: the phred scale is guessed from the first file buffer
constexpr int LINE_BYTES = 16, LINE_BLOCK = 256, LINE_TILE = LINE_BYTES * LINE_BLOCK;

struct TrimDev {
	int min_phred_raw;      // phred + -mp (raised to -eq / -mi)
	int min_q, hardmask_q, min_len, max_len;
	int plain, paired;
	double minP;
};

// what the records kernel makes of one (record, mate): where its trimmed bases, their qualities and its name lie in the chunk
struct Slot {
	int32_t seq_pos, qual_pos, len, name_pos, name_len;
	uint8_t pair, mate, keep, pad_;
};

// ---- lines --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned nl_mask16(const uint8_t *buf, int64_t at, int64_t bytes) {
	if(at >= bytes) return 0u;
	const uint4 v = *(const uint4 *) (buf + at);          // (the buffer is padded to whole tiles)
	const uint32_t w[4] = {v.x, v.y, v.z, v.w};
	unsigned m = 0;
#pragma unroll
	for(int k = 0; k < 4; ++k)
#pragma unroll
		for(int b = 0; b < 4; ++b) if(((w[k] >> (8 * b)) & 0xFFu) == (uint32_t) '\n') m |= 1u << (4 * k + b);
	const int64_t left = bytes - at;
	if(left < 16) m &= (1u << left) - 1u;
	return m;
}

// exclusive sum over the 256 threads of a block; *total = the block's sum
__device__ __forceinline__ int block_excl(int v, int *total) {
	__shared__ int wsum[LINE_BLOCK / 64];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	int inc = v;
#pragma unroll
	for(int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if(lane >= d) inc += o; }
	if(lane == 63) wsum[wv] = inc;
	__syncthreads();
	int base = 0, tot = 0;
#pragma unroll
	for(int k = 0; k < LINE_BLOCK / 64; ++k) { if(k < wv) base += wsum[k]; tot += wsum[k]; }
	*total = tot;
	return base + inc - v;
}

__global__ __launch_bounds__(LINE_BLOCK) void s1_lines_count_kernel(const uint8_t *buf, int64_t bytes, int64_t n_blocks, int64_t *block_cnt) {
	const int64_t at = ((int64_t) blockIdx.x * LINE_BLOCK + threadIdx.x) * LINE_BYTES;
	int tot;
	(void) block_excl(__popc(nl_mask16(buf, at, bytes)), &tot);
	if(threadIdx.x == 0) { block_cnt[blockIdx.x] = tot; if(blockIdx.x == 0) block_cnt[n_blocks] = 0; }
}

// lines[0] = 0, lines[j] = the byte behind the j-th newline
__global__ __launch_bounds__(LINE_BLOCK) void s1_lines_kernel(const uint8_t *buf, int64_t bytes, const int64_t *block_off, int32_t *lines) {
	const int64_t at = ((int64_t) blockIdx.x * LINE_BLOCK + threadIdx.x) * LINE_BYTES;
	unsigned m = nl_mask16(buf, at, bytes);
	int tot;
	int64_t j = block_off[blockIdx.x] + block_excl(__popc(m), &tot) + 1;
	if(blockIdx.x == 0 && threadIdx.x == 0) lines[0] = 0;
	while(m) { const int b = __ffs(m) - 1; m &= m - 1; lines[j++] = (int32_t) (at + b + 1); }
}

// the first record of the chunk that is not four well-formed lines
__global__ __launch_bounds__(256) void s1_shape_kernel(const uint8_t *buf, const int32_t *lines, int64_t n_rec, int *bad) {
	const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(r >= n_rec) return;
	const int32_t *l = lines + 4 * r;
	const int seq_len = l[2] - 1 - l[1], q_len = l[4] - 1 - l[3];
	if(buf[l[0]] != '@' || q_len < seq_len) atomicMin(bad, (int) r);
}

// ---- records ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

// phred_stat of ingest.hip (phredStat, runinput.c:127-313) on the -eq / -mi path; a base is N when the table says so or when its
// quality is below -mi (the host writes that into its copy of the read; here it is asked again). Sequential double arithmetic in the
// reference's order; no product feeds a sum, and contraction is off all the same: one fused rounding would break the byte parity
//
// QC: the routine with a report (phredStat's qcreport, runinput.c:133-136, 163, 303-312): C + G are counted beside the N's, through
// the -eq loop's segments as well, and *rep is what update_QCstat is given -- rep->len < 0 when the sequence is not counted.
struct QcSlot { double sp; int32_t len, gc, ns, org_len; };
#pragma clang fp contract(off)
template <bool QC>
__device__ int phred_stat_dev(const uint8_t *raw, const uint8_t *qual, int len, const uint8_t *T, const double *prob, const TrimDev P, int *START, int *END, QcSlot *rep = nullptr) {
	if constexpr(QC) { rep->sp = 0; rep->len = -1; rep->gc = 0; rep->ns = 0; rep->org_len = len; }
	if(P.max_len < len) { *START = 0; *END = 0; return 0; }
	const int minPhred = P.min_phred_raw;
	int start = 0, end = len;
	while(start < end && qual[start] < minPhred) ++start;
	while(start < end && qual[end - 1] < minPhred) --end;
	len = end - start;
	auto isN = [&](int i) { return T[raw[i]] == 4 || qual[i] < P.hardmask_q; };
	unsigned ns = 0, gc = 0;
	double sp = 0;
#define TALLY(p, n_, g_) do { if(isN(p)) ++n_; else if constexpr(QC) { const uint8_t c_ = T[raw[p]]; if(c_ == 1 || c_ == 2) ++g_; } } while(0)
	for(int i = start; i < end; ++i) { sp += prob[qual[i]]; TALLY(i, ns, gc); }
	const double minP = P.minP;
	if(P.min_len <= (int) (len - ns) && (minP * len) < sp) {
		unsigned ns5 = 0, ns3 = 0, gc5 = 0, gc3 = 0, l5 = 0, l3 = 0;
		double sp5 = 0, sp3 = 0;
		int p5 = start, p3 = end - 1;
#define GROW3() do { \
		while((int) l3 < len && minPhred <= qual[p3]) { sp3 += prob[qual[p3]]; ++l3; TALLY(p3, ns3, gc3); --p3; } \
		while((int) l3 < len && qual[p3] < minPhred) { sp3 += prob[qual[p3]]; ++l3; TALLY(p3, ns3, gc3); --p3; } } while(0)
#define GROW5() do { \
		while((int) l5 < len && minPhred <= qual[p5]) { sp5 += prob[qual[p5]]; ++l5; TALLY(p5, ns5, gc5); ++p5; } \
		while((int) l5 < len && qual[p5] < minPhred) { sp5 += prob[qual[p5]]; ++l5; TALLY(p5, ns5, gc5); ++p5; } } while(0)
		GROW3();
		while(P.min_len <= (int) (len - ns) && (minP * len) < sp) {
			if((sp5 * l3) < (sp3 * l5)) {
				end -= (int) l3; ns -= ns3; gc -= gc3; len -= (int) l3; sp -= sp3;
				ns3 = 0; gc3 = 0; l3 = 0; sp3 = 0;
				GROW3();
			} else {
				start += (int) l5; len -= (int) l5; ns -= ns5; gc -= gc5; sp -= sp5;
				ns5 = 0; gc5 = 0; l5 = 0; sp5 = 0;
				GROW5();
			}
		}
#undef GROW3
#undef GROW5
	}
#undef TALLY
	if constexpr(QC) if(P.min_len <= (int) (len - ns)) { rep->sp = sp; rep->len = len; rep->gc = (int32_t) gc; rep->ns = (int32_t) ns; }
	*START = start; *END = end;
	return len - (int) ns;
}

struct MateView { const uint8_t *buf; const int32_t *lines; int64_t first; };      // lines == NULL: the mate file has run out (empty mates)

// pack_fastq of ingest.hip for record index blockIdx * 256 + threadIdx of the pass: slots[mates * i + m], and per slot what it adds to
// the batch (kept reads, words with the pad word, name bytes with the NUL); entry [n_slots] of the three is 0 for the scans
//
// The -qc instantiation, s1_records_kernel<true, QcOut>: every read takes the routine with a report, never the plain path; per slot the
// report (qslots), whether update_QCstat counts it (counted, scanned like kept) and the longest counted sequence so far (*run_max:
// s1_qc_kernel bins by it). Its three outputs travel in a parameter pack, so that the plain instantiation, s1_records_kernel<false>, has
// the parameter list -- and the code -- of the kernel that knew no report.
struct QcOut { QcSlot *qslots; int64_t *counted; int *run_max; };
template <bool QC, class... Out>
__global__ __launch_bounds__(256) void s1_records_kernel(MateView M0, MateView M1, int64_t n, const TrimDev P, const uint8_t *tab, const double *prob,
                                                         Slot *slots, int64_t *kept, int64_t *words, int64_t *nbytes, unsigned long long *couples, Out... out) {
	static_assert(sizeof...(Out) == (QC ? 1 : 0), "the -qc instantiation takes one QcOut, the plain one nothing");
	__shared__ uint8_t T[256];
	T[threadIdx.x] = tab[threadIdx.x];
	__syncthreads();
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const int mates = P.paired ? 2 : 1;
	if(i == 0) { kept[n * mates] = 0; words[n * mates] = 0; nbytes[n * mates] = 0; }
	if constexpr(QC) if(i == 0) ((out.counted[n * mates] = 0), ...);
	if(i >= n) return;
	int len[2] = {0, 0};
	Slot S[2];
	QcSlot Q[2];
	for(int m = 0; m < mates; ++m) {
		const MateView &V = m ? M1 : M0;
		Slot &s = S[m];
		s.seq_pos = s.qual_pos = s.len = s.name_pos = s.name_len = 0; s.pair = 0; s.mate = (uint8_t) m; s.keep = 0; s.pad_ = 0;
		if constexpr(QC) { Q[m].sp = 0; Q[m].len = -1; Q[m].gc = 0; Q[m].ns = 0; Q[m].org_len = 0; }
		if(!V.lines) continue;
		const int32_t *l = V.lines + 4 * (V.first + i);
		const int l0 = l[0], l1 = l[1], l2 = l[2], l3 = l[3];
		{	// name: the header line without '@', chomped of trailing white space
			int h = l1 - 1;
			while(h > l0 && is_space(V.buf[h - 1])) --h;
			s.name_pos = l0 + 1; s.name_len = h > l0 ? h - l0 - 1 : 0;
		}
		const int L = l2 - 1 - l1;
		const uint8_t *q = V.buf + l3;
		int st = 0, en = 0;
		if constexpr(QC) len[m] = phred_stat_dev<true>(V.buf + l1, q, L, T, prob, P, &st, &en, &Q[m]);
		else if(P.plain) {
			if(P.max_len >= L) {
				en = L;
				while(st < en && q[st] < P.min_phred_raw) ++st;
				while(st < en && q[en - 1] < P.min_phred_raw) --en;
			}
			len[m] = en - st;
		} else len[m] = phred_stat_dev<false>(V.buf + l1, q, L, T, prob, P, &st, &en);
		s.seq_pos = l1 + st; s.qual_pos = l3 + st; s.len = en - st;
	}
	const bool ok0 = P.min_len <= len[0], ok1 = P.paired && P.min_len <= len[1];
	if(ok0 && ok1) { S[0].keep = 1; S[0].pair = 1; S[1].keep = 1; S[1].pair = 2; }
	else if(ok0) S[0].keep = 1;
	else if(ok1) S[1].keep = 1;
	{	// pair records of the pass (kept reads - couples = kept records), one atomic per wavefront
		const unsigned long long both = __ballot(ok0 && ok1);
		if(both && (threadIdx.x & 63) == __ffsll((long long) __ballot(1)) - 1) atomicAdd(couples, (unsigned long long) __popcll(both));
	}
	for(int m = 0; m < mates; ++m) {
		const int64_t o = i * mates + m;
		slots[o] = S[m];
		kept[o] = S[m].keep;
		words[o] = S[m].keep ? ((S[m].len + 31) >> 5) + 1 : 0;
		nbytes[o] = S[m].keep ? S[m].name_len + 1 : 0;
		if constexpr(QC) ((out.qslots[o] = Q[m], out.counted[o] = Q[m].len >= 0), ...);
	}
	if constexpr(QC) {	// the running maximum: an atomic only from a thread that still has something to raise (lanes behind the pass's
		// last record have left, so nothing is exchanged across the wave here)
		const int mx = max(Q[0].len, mates == 2 ? Q[1].len : -1);
		((mx > 0 && mx > *(volatile int *) out.run_max ? (void) atomicMax(out.run_max, mx) : (void) 0), ...);
	}
}

// ---- QC -----------------------------------------------------------------------------------------------------------------------
// One pass's share of update_QCstat (qc.c:85-104) for everything that does not depend on floating-point order: the integer sums
// (sequences counted, their bases, C + G, N's; the bases of every sequence read), the length histogram at len >> res, and the counted
// sequences' (sp, len) compacted in stream order behind the scan over `counted`. Per workgroup: the sums by wave reductions and one
// LDS word per wave, the histogram by LDS atomics, then one global atomic per sum and per bin that is not zero. res comes from the
// running maximum that the records kernel left behind (rescale_ldist, qc.c:50-65: the least res with maxlen >> res < 512), so every
// bin lies below 512; the host folds the bins of passes with different res together. Eeq and the quality bins are the host's: they
// depend on the order of the sum and on its log10.
// stat: [0] counted, [1] bases, [2] C + G, [3] N's, [4] bases read; then int res, int run_max (kept between the passes)
constexpr int QC_SUMS = 5, QC_BINS = 512;
struct QcStat { unsigned long long sum[QC_SUMS]; int res, run_max; uint32_t pad_[4]; uint32_t hist[QC_BINS]; };
__global__ __launch_bounds__(256) void s1_qc_kernel(int64_t n_slots, const QcSlot *qslots, const int64_t *counted_ex, QcStat *stat, KmaQcPair *pairs) {
	__shared__ uint32_t h[QC_BINS];
	__shared__ unsigned long long wsum[4][QC_SUMS];
	for(int b = threadIdx.x; b < QC_BINS; b += 256) h[b] = 0;
	const int run_max = stat->run_max;
	int res = 0;
	while(QC_BINS <= (run_max >> res)) ++res;
	__syncthreads();
	const int64_t o = (int64_t) blockIdx.x * 256 + threadIdx.x;
	unsigned long long v[QC_SUMS] = {0, 0, 0, 0, 0};
	if(o < n_slots) {
		const QcSlot q = qslots[o];
		v[4] = (unsigned long long) q.org_len;
		if(q.len >= 0) {
			v[0] = 1; v[1] = (unsigned long long) q.len; v[2] = (unsigned long long) q.gc; v[3] = (unsigned long long) q.ns;
			const int bin = q.len >> res;
			if(bin < QC_BINS) atomicAdd(&h[bin], 1u);
			KmaQcPair p;
			p.sp = q.sp; p.len = q.len; p.pad_ = 0;
			pairs[counted_ex[o]] = p;          // (16 bytes, 16-byte aligned: one store)
		}
	}
#pragma unroll
	for(int k = 0; k < QC_SUMS; ++k) {
#pragma unroll
		for(int d = 32; d > 0; d >>= 1) v[k] += __shfl_down(v[k], d, 64);
	}
	if((threadIdx.x & 63) == 0) for(int k = 0; k < QC_SUMS; ++k) wsum[threadIdx.x >> 6][k] = v[k];
	__syncthreads();
	if(threadIdx.x < QC_SUMS) {
		const unsigned long long t = wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
		if(t) atomicAdd(&stat->sum[threadIdx.x], t);
	}
	for(int b = threadIdx.x; b < QC_BINS; b += 256) if(h[b]) atomicAdd(&stat->hist[b], h[b]);
	if(blockIdx.x == 0 && threadIdx.x == 0) stat->res = res;
}

// ---- pack ---------------------------------------------------------------------------------------------------------------------
struct OutView {
	uint64_t *seq;
	int64_t *seq_off, *N_off, *name_off;
	int32_t *len, *N;
	char *names;
	uint8_t *pair;
	int64_t r0, w0, n0, c0;          // what the batch held before this pass: reads, words, N's, name bytes
};

// append_raw / append_read of ingest.hip: a group of G lanes per slot, a lane per 32-base word (and the pad word); codes above 4 are
// OR-ed in unmasked like there. wordN[w] = the N's of word w of the pass (scanned afterwards). Then the header bytes and the NUL.
__global__ __launch_bounds__(256) void s1_pack_kernel(const uint8_t *buf0, const uint8_t *buf1, int64_t n_slots, int G, const Slot *slots, const int64_t *kept_ex,
                                                      const int64_t *words_ex, const int64_t *nbytes_ex, int hardmask_q, const uint8_t *tab, OutView O, int64_t *wordN, int *max_len) {
	__shared__ uint8_t T[256];
	T[threadIdx.x] = tab[threadIdx.x];
	__syncthreads();
	const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t o = t / G;
	const int g = (int) (t % G);
	if(o >= n_slots) return;
	const Slot s = slots[o];
	if(!s.keep) return;
	const uint8_t *buf = s.mate ? buf1 : buf0;
	const int64_t r = O.r0 + kept_ex[o], wl = words_ex[o], c = O.c0 + nbytes_ex[o];
	const int L = s.len, nw = (L + 31) >> 5;
	if(g == 0) {
		O.len[r] = L; O.seq_off[r] = O.w0 + wl; O.name_off[r] = c; O.pair[r] = s.pair;
		if(L > *max_len) atomicMax(max_len, L);
	}
	const uint8_t *raw = buf + s.seq_pos, *q = buf + s.qual_pos;
	for(int w = g; w <= nw; w += G) {
		uint64_t x = 0;
		int nN = 0;
		if(w < nw) {
			const int i0 = w << 5, e = min(32, L - i0);
			for(int i = 0; i < e; ++i) {
				uint8_t code = T[raw[i0 + i]];
				if(hardmask_q && q[i0 + i] < hardmask_q) code = 4;
				if(code == 4) { x <<= 2; ++nN; }
				else x = (x << 2) | code;
			}
			if(e < 32) x <<= (64 - (e << 1));
		}
		O.seq[O.w0 + wl + w] = x;
		wordN[wl + w] = nN;
	}
	const uint8_t *nm = buf + s.name_pos;
	for(int k = g; k <= s.name_len; k += G) O.names[c + k] = k < s.name_len ? (char) nm[k] : '\0';
}

// the N lists: N_off of every read of the pass from the scan over its words, the positions word by word
__global__ __launch_bounds__(256) void s1_npos_kernel(const uint8_t *buf0, const uint8_t *buf1, int64_t n_slots, int G, const Slot *slots, const int64_t *kept_ex,
                                                      const int64_t *words_ex, const int64_t *wordN, const int64_t *wordN_ex, int hardmask_q, const uint8_t *tab, OutView O) {
	__shared__ uint8_t T[256];
	T[threadIdx.x] = tab[threadIdx.x];
	__syncthreads();
	const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t o = t / G;
	const int g = (int) (t % G);
	if(o >= n_slots) return;
	const Slot s = slots[o];
	if(!s.keep) return;
	const uint8_t *buf = s.mate ? buf1 : buf0;
	const int64_t wl = words_ex[o];
	if(g == 0) O.N_off[O.r0 + kept_ex[o]] = O.n0 + wordN_ex[wl];
	const int L = s.len, nw = (L + 31) >> 5;
	const uint8_t *raw = buf + s.seq_pos, *q = buf + s.qual_pos;
	for(int w = g; w < nw; w += G) {
		if(!wordN[wl + w]) continue;
		int32_t *out = O.N + O.n0 + wordN_ex[wl + w];
		const int i0 = w << 5, e = min(32, L - i0);
		for(int i = 0; i < e; ++i) if(T[raw[i0 + i]] == 4 || (hardmask_q && q[i0 + i] < hardmask_q)) *out++ = i0 + i;
	}
}

// the offsets behind the last read of the batch so far
__global__ void s1_ends_kernel(OutView O, int64_t r, int64_t w, int64_t n, int64_t c) {
	if(threadIdx.x == 0 && blockIdx.x == 0) { O.seq_off[r] = w; O.N_off[r] = n; O.name_off[r] = c; }
}

// ---- text ---------------------------------------------------------------------------------------------------------------------
// `kma trim` (printTrimFsa / printTrimFsa_pair, trim.c:28-126): every kept record as FASTQ text -- '@' and the chomped header line, the
// trimmed bases through to2Bit and "ACGTN" (a hard-masked base is an N), "+", the trimmed qualities -- single records in stream 0,
// couples in stream 1, both in stream order. A record's size follows from its Slot alone; the sizes are scanned per stream.
__device__ __forceinline__ int64_t fastq_bytes(const Slot &s) { return s.keep ? 2 * (int64_t) s.len + s.name_len + 6 : 0; }

__global__ __launch_bounds__(256) void s1_fastq_size_kernel(int64_t n_slots, const Slot *slots, int64_t *size0, int64_t *size1) {
	const int64_t o = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(o == 0) { size0[n_slots] = 0; size1[n_slots] = 0; }
	if(o >= n_slots) return;
	const Slot s = slots[o];
	const int64_t b = fastq_bytes(s);
	size0[o] = s.pair ? 0 : b;
	size1[o] = s.pair ? b : 0;
}

// A group of G lanes per slot. The record is a run of bytes at an arbitrary offset of its stream: the bytes before the first
// 16-byte boundary and behind the last one are stored one by one, everything between as whole 16-byte words, a word per lane and
// round -- each put together from the chunk (header and qualities as they are, bases through the table).
__global__ __launch_bounds__(256) void s1_fastq_kernel(const uint8_t *buf0, const uint8_t *buf1, int64_t n_slots, int G, const Slot *slots, const int64_t *off0,
                                                       const int64_t *off1, int hardmask_q, const uint8_t *tab, char *text0, char *text1) {
	__shared__ uint8_t T[256];
	T[threadIdx.x] = tab[threadIdx.x];
	__syncthreads();
	const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t o = t / G;
	const int g = (int) (t % G);
	if(o >= n_slots) return;
	const Slot s = slots[o];
	if(!s.keep) return;
	const uint8_t *buf = s.mate ? buf1 : buf0;
	const uint8_t *nm = buf + s.name_pos, *raw = buf + s.seq_pos, *q = buf + s.qual_pos;
	char *dst = s.pair ? text1 + off1[o] : text0 + off0[o];
	const int64_t L = s.len, nl = s.name_len, size = 2 * L + nl + 6;
	const int64_t b0 = nl + 2, b1 = b0 + L, q0 = b1 + 3, q1 = q0 + L;          // bases [b0, b1), "\n+\n", qualities [q0, q1), '\n'
	auto byte_at = [&](int64_t j) -> char {
		if(j >= q0) return j < q1 ? (char) q[j - q0] : '\n';
		if(j >= b1) return j == b1 + 1 ? '+' : '\n';
		if(j >= b0) {
			uint8_t code = T[raw[j - b0]];
			if(hardmask_q && q[j - b0] < hardmask_q) code = 4;
			return "ACGTN-"[code < 5 ? code : 5];
		}
		return j == 0 ? '@' : (j <= nl ? (char) nm[j - 1] : '\n');
	};
	// [0, head) single bytes, [head, head + 16 * words) aligned words, the rest single bytes
	const int64_t head = min(size, (int64_t) ((16 - ((uintptr_t) dst & 15)) & 15)), words = (size - head) >> 4, tail = head + (words << 4);
	for(int64_t j = g; j < head; j += G) dst[j] = byte_at(j);
	for(int64_t w = g; w < words; w += G) {
		const int64_t j0 = head + (w << 4);
		uint32_t x[4];
#pragma unroll
		for(int k = 0; k < 4; ++k) {
			x[k] = 0;
#pragma unroll
			for(int b = 0; b < 4; ++b) x[k] |= (uint32_t) (uint8_t) byte_at(j0 + 4 * k + b) << (8 * b);
		}
		*(uint4 *) (dst + j0) = make_uint4(x[0], x[1], x[2], x[3]);
	}
	for(int64_t j = tail + g; j < size; j += G) dst[j] = byte_at(j);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// a device array of the reader's own (never the process-wide block cache: it belongs to the device current at open). Growing one is
// hipMalloc + copy + hipFree on the reader's thread, and hipFree waits for the whole device -- also for what another thread is running
// on the batch before: that happens while the first batches size the arrays, not afterwards
struct DBuf {
	char *p = nullptr;
	size_t cap = 0;
	~DBuf() { if(p) (void) hipFree(p); }
	int ensure(size_t need, size_t used, hipStream_t s) {
		if(need <= cap && p) return KMAHIP_OK;
		const size_t want = std::max<size_t>(std::max(need, cap + cap / 2), 256);
		char *q = nullptr;
		if(hipMalloc((void **) &q, want) != hipSuccess) { kmahip_set_error("hipMalloc of %zu bytes failed", want); return KMAHIP_ENOMEM; }
		if(p) {
			if((used && hipMemcpyAsync(q, p, used, hipMemcpyDeviceToDevice, s) != hipSuccess) || hipStreamSynchronize(s) != hipSuccess) {
				(void) hipFree(q); kmahip_set_error("device copy failed"); return KMAHIP_EDEVICE;
			}
			(void) hipFree(p);
		}
		p = q; cap = want;
		return KMAHIP_OK;
	}
	template <class T> T *as() const { return (T *) p; }
};

struct MateIn {
	int fd = -1;
	size_t size = 0, off = 0;         // off: where the resident chunk starts in the file (always a record start)
	DBuf buf, lines;
	size_t bytes = 0;                 // of the resident chunk
	int64_t usable = 0, cur = 0;      // records of the chunk the device delivers, and how many of them it has
	size_t consumed = 0;              // bytes of the chunk those records take
	bool loaded = false, done = false, handback = false;
};

}  // namespace

struct kmahip_ingest_dev {
	MateIn m[2];
	int mates = 1;
	std::string path[2];
	kmahip_trim trim;
	TrimDev P;
	int phred = 33, device = 0, threads = 1;
	size_t chunk = 64u << 20, piece = 16u << 20;
	hipStream_t s = nullptr, cs = nullptr;          // kernels; copies
	static constexpr int NPIN = 3;
	uint8_t *pin[NPIN] = {nullptr, nullptr, nullptr};
	hipEvent_t pin_free[NPIN] = {nullptr, nullptr, nullptr};
	hipEvent_t pass_done = nullptr;
	bool dev_up = false;
	DBuf tab, prob, scan_tmp, small;
	int64_t *h_small = nullptr;          // pinned: the few figures that come back per pass
	// per pass
	DBuf slots, kept, words, nbytes, kept_ex, words_ex, nbytes_ex, wordN, wordN_ex, block_cnt, block_off;
	// the batch
	DBuf o_seq, o_seq_off, o_len, o_N, o_N_off, o_names, o_name_off, o_pair;
	std::vector<uint8_t> h_pair;
	int64_t n_read = 0, n_kept = 0, handed = 0;
	kmahip_ingest *host = nullptr;       // the host reader, once the rest of the input is its
	double ms_read = 0, ms_copy = 0, ms_kernel = 0;
	int64_t bytes_in = 0;
	// kmahip_ingest_dev_set_qc: the accumulator, the per-slot reports and their scan, the pass's sums + histogram (device and pinned
	// mirror) and the counted sequences' (sp, len) as they come back; where the report's own time went (KMAHIP_DEBUG_TIMING)
	// kmahip_ingest_dev_set_text: the per-slot sizes of the two streams and their scans, the batch's text on the device and as it
	// comes back
	bool text = false;
	DBuf tsize[2], tsize_ex[2], d_text[2];
	int64_t text_tot[2] = {0, 0};
	std::vector<char> h_text[2];
	kmahip_qc *qc = nullptr;
	bool started = false;
	DBuf qslots, counted, counted_ex, qpairs, qstat;
	QcStat *h_qstat = nullptr;
	std::vector<KmaQcPair> h_pairs;
	double ms_qc_copy = 0, ms_qc_bin = 0;
};

namespace {

using Reader = kmahip_ingest_dev;

int scan64(Reader *R, const int64_t *in, int64_t *out, size_t n) {
	size_t tmp = 0;
	if(rocprim::exclusive_scan(nullptr, tmp, in, out, (int64_t) 0, n, rocprim::plus<int64_t>(), R->s) != hipSuccess) { kmahip_set_error("rocprim::exclusive_scan (size query) failed"); return KMAHIP_EDEVICE; }
	int rc = R->scan_tmp.ensure(tmp + 16, 0, R->s);
	if(rc) return rc;
	if(rocprim::exclusive_scan(R->scan_tmp.p, tmp, in, out, (int64_t) 0, n, rocprim::plus<int64_t>(), R->s) != hipSuccess) { kmahip_set_error("rocprim::exclusive_scan failed"); return KMAHIP_EDEVICE; }
	return KMAHIP_OK;
}

// streams, pinned buffers, the tables: the first device work of the reader
int bring_up(Reader *R) {
	if(R->dev_up) return KMAHIP_OK;
	HIP_TRY(hipStreamCreateWithFlags(&R->s, hipStreamNonBlocking));
	HIP_TRY(hipStreamCreateWithFlags(&R->cs, hipStreamNonBlocking));
	for(int k = 0; k < Reader::NPIN; ++k) {
		HIP_TRY(hipHostMalloc((void **) &R->pin[k], R->piece, hipHostMallocDefault));
		HIP_TRY(hipEventCreateWithFlags(&R->pin_free[k], hipEventDisableTiming));
	}
	HIP_TRY(hipEventCreateWithFlags(&R->pass_done, hipEventDisableTiming));
	HIP_TRY(hipHostMalloc((void **) &R->h_small, 64 * sizeof(int64_t), hipHostMallocDefault));
	// ingest.hip's to2Bit table (kma.c:1440-1480) as it is, and its 10^(-q/10) table re-indexed by the raw quality byte
	const double *P = kmahip_ingest_prob();
	double pr[256];
	// (a quality byte below the scale's base has no entry in the reference's table either; it reads as quality 0 here)
	for(int raw = 0; raw < 256; ++raw) pr[raw] = P[std::min(255, std::max(0, raw - R->phred))];
	int rc;
	if((rc = R->tab.ensure(256, 0, R->s)) || (rc = R->prob.ensure(sizeof pr, 0, R->s)) || (rc = R->small.ensure(64 * 8, 0, R->s))) return rc;
	HIP_TRY(hipMemcpy(R->tab.p, kmahip_ingest_to2bit(), 256, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(R->prob.p, pr, sizeof pr, hipMemcpyHostToDevice));
	R->dev_up = true;
	return KMAHIP_OK;
}

double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }

// bytes [off, off + bytes) of the file into the mate's device buffer: parallel pread into pinned pieces, each copied up while the next
// one is read. One chunk per mate file is resident: the next one is fetched when its records have all been taken, so reading + copying
// and the kernels take turns (DESIGN.md 3.6a says what that costs and what a second chunk buffer would change)
int fetch(Reader *R, MateIn &M, size_t bytes) {
	const size_t padded = (bytes + LINE_TILE - 1) / LINE_TILE * LINE_TILE + LINE_TILE;
	int rc = M.buf.ensure(padded, 0, R->s);
	if(rc) return rc;
	// (the kernels of the last pass may still be reading the chunk this one replaces: the copies wait for them, the reads need not)
	HIP_TRY(hipEventRecord(R->pass_done, R->s));
	HIP_TRY(hipStreamWaitEvent(R->cs, R->pass_done, 0));
	size_t at = 0;
	int k = 0;
	std::atomic<bool> io_fail{false};
	while(at < bytes) {
		const size_t n = std::min(R->piece, bytes - at);
		HIP_TRY(hipEventSynchronize(R->pin_free[k]));
		const auto t0 = std::chrono::steady_clock::now();
		uint8_t *dst = R->pin[k];
		const int nt = (int) std::max<size_t>(1, std::min<size_t>((size_t) R->threads, n / (1u << 20)));
		auto rd = [&](int w) {
			size_t a = n * (size_t) w / (size_t) nt;
			const size_t b = n * (size_t) (w + 1) / (size_t) nt;
			while(a < b) {
				const ssize_t got = pread(M.fd, dst + a, b - a, (off_t) (M.off + at + a));
				if(got <= 0) { io_fail = true; return; }
				a += (size_t) got;
			}
		};
		{
			std::vector<std::thread> pool;
			for(int w = 1; w < nt; ++w) pool.emplace_back(rd, w);
			rd(0);
			for(std::thread &th : pool) th.join();
		}
		R->ms_read += ms_since(t0);
		if(io_fail) { kmahip_set_error("read error in %s", R->path[&M - R->m].c_str()); return KMAHIP_EIO; }
		HIP_TRY(hipMemcpyAsync(M.buf.p + at, dst, n, hipMemcpyHostToDevice, R->cs));
		HIP_TRY(hipEventRecord(R->pin_free[k], R->cs));
		at += n;
		k = (k + 1) % Reader::NPIN;
	}
	const auto t1 = std::chrono::steady_clock::now();
	HIP_TRY(hipStreamSynchronize(R->cs));
	R->ms_copy += ms_since(t1);
	R->bytes_in += (int64_t) bytes;
	return KMAHIP_OK;
}

// the next chunk of a mate file whose resident records have all been taken: fetched, its lines indexed, its shape checked.
// Afterwards the mate has usable records, or has run out (done), or the host reader has to take over at M.off (handback)
int next_chunk(Reader *R, MateIn &M) {
	M.off += M.consumed;
	M.consumed = 0; M.usable = 0; M.cur = 0; M.loaded = false;
	for(;;) {
		if(M.off >= M.size) { M.done = true; return KMAHIP_OK; }
		const size_t bytes = std::min(R->chunk, M.size - M.off);
		if(bytes > (size_t) INT_MAX - 2 * LINE_TILE) { M.handback = true; return KMAHIP_OK; }          // (a record of two gigabytes: the host reader's)
		int rc = fetch(R, M, bytes);
		if(rc) return rc;
		M.bytes = bytes;
		const int64_t nb = (int64_t) ((bytes + LINE_TILE - 1) / LINE_TILE);
		if((rc = R->block_cnt.ensure((size_t) (nb + 1) * 8, 0, R->s)) || (rc = R->block_off.ensure((size_t) (nb + 1) * 8, 0, R->s))) return rc;
		const uint8_t *buf = (const uint8_t *) M.buf.p;
		hipLaunchKernelGGL(s1_lines_count_kernel, dim3((unsigned) nb), dim3(LINE_BLOCK), 0, R->s, buf, (int64_t) bytes, nb, R->block_cnt.as<int64_t>());
		HIP_TRY(hipGetLastError());
		if((rc = scan64(R, R->block_cnt.as<int64_t>(), R->block_off.as<int64_t>(), (size_t) nb + 1))) return rc;
		HIP_TRY(hipMemcpyAsync(R->h_small, R->block_off.as<int64_t>() + nb, 8, hipMemcpyDeviceToHost, R->s));
		HIP_TRY(hipStreamSynchronize(R->s));
		const int64_t n_lines = R->h_small[0], n_rec = n_lines / 4;
		int bad = INT_MAX;
		if(n_rec > 0) {
			if((rc = M.lines.ensure((size_t) (n_lines + 2) * 4, 0, R->s))) return rc;
			hipLaunchKernelGGL(s1_lines_kernel, dim3((unsigned) nb), dim3(LINE_BLOCK), 0, R->s, buf, (int64_t) bytes, R->block_off.as<int64_t>(), M.lines.as<int32_t>());
			int *d_bad = R->small.as<int>();
			*(int *) (R->h_small + 1) = INT_MAX;
			HIP_TRY(hipMemcpyAsync(d_bad, R->h_small + 1, sizeof(int), hipMemcpyHostToDevice, R->s));
			hipLaunchKernelGGL(s1_shape_kernel, dim3((unsigned) ((n_rec + 255) / 256)), dim3(256), 0, R->s, buf, M.lines.as<int32_t>(), n_rec, d_bad);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(R->h_small, d_bad, sizeof(int), hipMemcpyDeviceToHost, R->s));
			HIP_TRY(hipStreamSynchronize(R->s));
			bad = *(const int *) R->h_small;
		}
		const int64_t usable = std::min<int64_t>(n_rec, bad);
		if(usable > 0) {
			HIP_TRY(hipMemcpyAsync(R->h_small, M.lines.as<int32_t>() + 4 * usable, 4, hipMemcpyDeviceToHost, R->s));
			HIP_TRY(hipStreamSynchronize(R->s));
			M.usable = usable; M.consumed = (size_t) *(const int32_t *) R->h_small; M.loaded = true;
			return KMAHIP_OK;
		}
		if(bad == 0 || M.off + bytes >= M.size) { M.handback = true; return KMAHIP_OK; }      // an odd record, or the bytes behind the last complete one
		R->chunk *= 2;                                                                         // a record longer than the chunk
	}
}

// records [cur, cur + take) of the resident chunks behind what the batch holds already
int run_pass(Reader *R, int64_t take, int64_t tot[4], int *d_max_len, int64_t *records) {
	const int mates = R->mates;
	const int64_t ns = take * mates;
	int rc;
	if((rc = R->slots.ensure((size_t) ns * sizeof(Slot), 0, R->s)) || (rc = R->kept.ensure((size_t) (ns + 1) * 8, 0, R->s)) || (rc = R->words.ensure((size_t) (ns + 1) * 8, 0, R->s)) ||
	   (rc = R->nbytes.ensure((size_t) (ns + 1) * 8, 0, R->s)) || (rc = R->kept_ex.ensure((size_t) (ns + 1) * 8, 0, R->s)) || (rc = R->words_ex.ensure((size_t) (ns + 1) * 8, 0, R->s)) ||
	   (rc = R->nbytes_ex.ensure((size_t) (ns + 1) * 8, 0, R->s))) return rc;
	if(R->qc && ((rc = R->qslots.ensure((size_t) ns * sizeof(QcSlot), 0, R->s)) || (rc = R->counted.ensure((size_t) (ns + 1) * 8, 0, R->s)) ||
	             (rc = R->counted_ex.ensure((size_t) (ns + 1) * 8, 0, R->s)) || (rc = R->qpairs.ensure((size_t) (ns + 1) * sizeof(KmaQcPair), 0, R->s)))) return rc;
	MateView V[2] = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
	size_t rec_bytes = 0;          // bytes per record of the chunks: long reads get a wavefront each, short ones eight lanes
	for(int m = 0; m < mates; ++m) if(!R->m[m].done) {
		V[m] = MateView{(const uint8_t *) R->m[m].buf.p, R->m[m].lines.as<int32_t>(), R->m[m].cur};
		rec_bytes = std::max(rec_bytes, R->m[m].consumed / (size_t) R->m[m].usable);
	}
	unsigned long long *d_couples = (unsigned long long *) (R->small.p + 64);
	HIP_TRY(hipMemsetAsync(d_couples, 0, 8, R->s));
	QcStat *d_stat = R->qstat.as<QcStat>();
	if(R->qc) {
		// (the sums and the bins start at zero with every pass; res and the running maximum stay)
		HIP_TRY(hipMemsetAsync(d_stat->sum, 0, sizeof d_stat->sum, R->s));
		HIP_TRY(hipMemsetAsync(d_stat->hist, 0, sizeof d_stat->hist, R->s));
		hipLaunchKernelGGL((s1_records_kernel<true, QcOut>), dim3((unsigned) ((take + 255) / 256)), dim3(256), 0, R->s, V[0], V[1], take, R->P, (const uint8_t *) R->tab.p, R->prob.as<double>(),
		                   R->slots.as<Slot>(), R->kept.as<int64_t>(), R->words.as<int64_t>(), R->nbytes.as<int64_t>(), d_couples,
		                   QcOut{R->qslots.as<QcSlot>(), R->counted.as<int64_t>(), &d_stat->run_max});
	} else
	hipLaunchKernelGGL(s1_records_kernel<false>, dim3((unsigned) ((take + 255) / 256)), dim3(256), 0, R->s, V[0], V[1], take, R->P, (const uint8_t *) R->tab.p, R->prob.as<double>(),
	                   R->slots.as<Slot>(), R->kept.as<int64_t>(), R->words.as<int64_t>(), R->nbytes.as<int64_t>(), d_couples);
	HIP_TRY(hipGetLastError());
	if(R->qc) {
		if((rc = scan64(R, R->counted.as<int64_t>(), R->counted_ex.as<int64_t>(), (size_t) ns + 1))) return rc;
		hipLaunchKernelGGL(s1_qc_kernel, dim3((unsigned) ((ns + 255) / 256)), dim3(256), 0, R->s, ns, R->qslots.as<QcSlot>(), R->counted_ex.as<int64_t>(), d_stat, R->qpairs.as<KmaQcPair>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(R->h_qstat, d_stat, sizeof(QcStat), hipMemcpyDeviceToHost, R->s));
	}
	if((rc = scan64(R, R->kept.as<int64_t>(), R->kept_ex.as<int64_t>(), (size_t) ns + 1)) || (rc = scan64(R, R->words.as<int64_t>(), R->words_ex.as<int64_t>(), (size_t) ns + 1)) ||
	   (rc = scan64(R, R->nbytes.as<int64_t>(), R->nbytes_ex.as<int64_t>(), (size_t) ns + 1))) return rc;
	HIP_TRY(hipMemcpyAsync(R->h_small + 0, R->kept_ex.as<int64_t>() + ns, 8, hipMemcpyDeviceToHost, R->s));
	HIP_TRY(hipMemcpyAsync(R->h_small + 1, R->words_ex.as<int64_t>() + ns, 8, hipMemcpyDeviceToHost, R->s));
	HIP_TRY(hipMemcpyAsync(R->h_small + 2, R->nbytes_ex.as<int64_t>() + ns, 8, hipMemcpyDeviceToHost, R->s));
	HIP_TRY(hipMemcpyAsync(R->h_small + 3, d_couples, 8, hipMemcpyDeviceToHost, R->s));
	HIP_TRY(hipStreamSynchronize(R->s));
	const int64_t nk = R->h_small[0], nw = R->h_small[1], nc = R->h_small[2];
	*records += nk - R->h_small[3];
	if(R->qc) {
		// the counted sequences' (sp, len) in stream order: Eeq is their sum in that order and the quality bin the decision of this
		// host's log10 (qc.hip), everything else of the pass was summed on the device
		const QcStat &H = *R->h_qstat;
		const size_t nq = (size_t) H.sum[0];
		const auto t0 = std::chrono::steady_clock::now();
		R->h_pairs.resize(nq);
		if(nq) {
			HIP_TRY(hipMemcpyAsync(R->h_pairs.data(), R->qpairs.p, nq * sizeof(KmaQcPair), hipMemcpyDeviceToHost, R->s));
			HIP_TRY(hipStreamSynchronize(R->s));
		}
		const auto t1 = std::chrono::steady_clock::now();
		kmahip_qc_add_pass(R->qc, H.sum[0], H.sum[1], H.sum[2], H.sum[3], H.run_max, H.hist, H.res, R->h_pairs.data(), nq);
		kmahip_qc_add_read(R->qc, (uint64_t) ns, H.sum[4], (uint64_t) take, (uint64_t) (nk - R->h_small[3]));
		R->ms_qc_copy += std::chrono::duration<double, std::milli>(t1 - t0).count();
		R->ms_qc_bin += ms_since(t1);
	}
	if(R->text && nk) {
		// the pass's records as text behind what the batch holds already: sizes, their scans, the bytes
		for(int k = 0; k < 2; ++k) if((rc = R->tsize[k].ensure((size_t) (ns + 1) * 8, 0, R->s)) || (rc = R->tsize_ex[k].ensure((size_t) (ns + 1) * 8, 0, R->s))) return rc;
		hipLaunchKernelGGL(s1_fastq_size_kernel, dim3((unsigned) ((ns + 255) / 256)), dim3(256), 0, R->s, ns, R->slots.as<Slot>(), R->tsize[0].as<int64_t>(), R->tsize[1].as<int64_t>());
		HIP_TRY(hipGetLastError());
		for(int k = 0; k < 2; ++k) {
			if((rc = scan64(R, R->tsize[k].as<int64_t>(), R->tsize_ex[k].as<int64_t>(), (size_t) ns + 1))) return rc;
			HIP_TRY(hipMemcpyAsync(R->h_small + 5 + k, R->tsize_ex[k].as<int64_t>() + ns, 8, hipMemcpyDeviceToHost, R->s));
		}
		HIP_TRY(hipStreamSynchronize(R->s));
		const int64_t nt[2] = {R->h_small[5], R->h_small[6]};
		for(int k = 0; k < 2; ++k) if((rc = R->d_text[k].ensure((size_t) (R->text_tot[k] + nt[k] + 16), (size_t) R->text_tot[k], R->s))) return rc;
		const int G = rec_bytes > 600 ? 64 : 8;
		const int64_t threads = ns * G;
		hipLaunchKernelGGL(s1_fastq_kernel, dim3((unsigned) ((threads + 255) / 256)), dim3(256), 0, R->s, (const uint8_t *) R->m[0].buf.p, (const uint8_t *) R->m[1].buf.p, ns, G, R->slots.as<Slot>(),
		                   R->tsize_ex[0].as<int64_t>(), R->tsize_ex[1].as<int64_t>(), R->P.hardmask_q, (const uint8_t *) R->tab.p, R->d_text[0].p + R->text_tot[0], R->d_text[1].p + R->text_tot[1]);
		HIP_TRY(hipGetLastError());
		R->text_tot[0] += nt[0]; R->text_tot[1] += nt[1];
	}
	if(nk) {
		if((rc = R->o_seq.ensure((size_t) (tot[1] + nw + 2) * 8, (size_t) tot[1] * 8, R->s)) || (rc = R->o_seq_off.ensure((size_t) (tot[0] + nk + 1) * 8, (size_t) tot[0] * 8, R->s)) ||
		   (rc = R->o_N_off.ensure((size_t) (tot[0] + nk + 1) * 8, (size_t) tot[0] * 8, R->s)) || (rc = R->o_name_off.ensure((size_t) (tot[0] + nk + 1) * 8, (size_t) tot[0] * 8, R->s)) ||
		   (rc = R->o_len.ensure((size_t) (tot[0] + nk + 1) * 4, (size_t) tot[0] * 4, R->s)) || (rc = R->o_pair.ensure((size_t) (tot[0] + nk + 1), (size_t) tot[0], R->s)) ||
		   (rc = R->o_names.ensure((size_t) (tot[3] + nc + 1), (size_t) tot[3], R->s)) || (rc = R->wordN.ensure((size_t) (nw + 1) * 8, 0, R->s)) ||
		   (rc = R->wordN_ex.ensure((size_t) (nw + 1) * 8, 0, R->s))) return rc;
		OutView O{R->o_seq.as<uint64_t>(), R->o_seq_off.as<int64_t>(), R->o_N_off.as<int64_t>(), R->o_name_off.as<int64_t>(), R->o_len.as<int32_t>(), R->o_N.as<int32_t>(),
		          R->o_names.p, (uint8_t *) R->o_pair.p, tot[0], tot[1], tot[2], tot[3]};
		const int G = rec_bytes > 600 ? 64 : 8;          // (eight lanes: reads of up to 224 bases, seven words and the pad word, in one round; any G is right)
		const int64_t threads = ns * G;
		const uint8_t *b0 = (const uint8_t *) R->m[0].buf.p, *b1 = (const uint8_t *) R->m[1].buf.p;
		HIP_TRY(hipMemsetAsync(R->wordN.p + (size_t) nw * 8, 0, 8, R->s));
		hipLaunchKernelGGL(s1_pack_kernel, dim3((unsigned) ((threads + 255) / 256)), dim3(256), 0, R->s, b0, b1, ns, G, R->slots.as<Slot>(), R->kept_ex.as<int64_t>(), R->words_ex.as<int64_t>(),
		                   R->nbytes_ex.as<int64_t>(), R->P.hardmask_q, (const uint8_t *) R->tab.p, O, R->wordN.as<int64_t>(), d_max_len);
		HIP_TRY(hipGetLastError());
		if((rc = scan64(R, R->wordN.as<int64_t>(), R->wordN_ex.as<int64_t>(), (size_t) nw + 1))) return rc;
		HIP_TRY(hipMemcpyAsync(R->h_small + 4, R->wordN_ex.as<int64_t>() + nw, 8, hipMemcpyDeviceToHost, R->s));
		HIP_TRY(hipStreamSynchronize(R->s));
		const int64_t nn = R->h_small[4];
		if((rc = R->o_N.ensure((size_t) (tot[2] + nn + 1) * 4, (size_t) tot[2] * 4, R->s))) return rc;
		O.N = R->o_N.as<int32_t>();
		hipLaunchKernelGGL(s1_npos_kernel, dim3((unsigned) ((threads + 255) / 256)), dim3(256), 0, R->s, b0, b1, ns, G, R->slots.as<Slot>(), R->kept_ex.as<int64_t>(), R->words_ex.as<int64_t>(),
		                   R->wordN.as<int64_t>(), R->wordN_ex.as<int64_t>(), R->P.hardmask_q, (const uint8_t *) R->tab.p, O);
		HIP_TRY(hipGetLastError());
		tot[0] += nk; tot[1] += nw; tot[2] += nn; tot[3] += nc;
	}
	for(int m = 0; m < mates; ++m) if(!R->m[m].done) R->m[m].cur += take;
	return KMAHIP_OK;
}

int min_out(Reader *R) {
	int rc;
	if((rc = R->o_seq.ensure(64, 0, R->s)) || (rc = R->o_seq_off.ensure(64, 0, R->s)) || (rc = R->o_N_off.ensure(64, 0, R->s)) || (rc = R->o_name_off.ensure(64, 0, R->s)) ||
	   (rc = R->o_len.ensure(64, 0, R->s)) || (rc = R->o_pair.ensure(64, 0, R->s)) || (rc = R->o_names.ensure(64, 0, R->s)) || (rc = R->o_N.ensure(64, 0, R->s))) return rc;
	return KMAHIP_OK;
}

// the rest of the input is the host reader's: from the record the device stopped at, in every mate file
int hand_back(Reader *R) {
	size_t off[2] = {0, 0};
	for(int m = 0; m < R->mates; ++m) {
		MateIn &M = R->m[m];
		off[m] = M.off;
		if(M.loaded && M.cur < M.usable) {
			if(M.cur > 0) {
				HIP_TRY(hipMemcpyAsync(R->h_small, M.lines.as<int32_t>() + 4 * M.cur, 4, hipMemcpyDeviceToHost, R->s));
				HIP_TRY(hipStreamSynchronize(R->s));
				off[m] += (size_t) *(const int32_t *) R->h_small;
			}
		} else if(M.loaded) off[m] += M.consumed;
		off[m] = std::min(off[m], M.size);
	}
	for(int m = 0; m < R->mates; ++m) R->handed += (int64_t) (R->m[m].size - off[m]);
	int rc = kmahip_ingest_open_at(R->path[0].c_str(), off[0], R->mates == 2 ? R->path[1].c_str() : nullptr, off[1], &R->trim, R->phred, R->n_read, R->n_kept, &R->host);
	if(!rc && R->text) rc = kmahip_ingest_set_text(R->host, 1);
	if(!rc && R->qc) rc = kmahip_ingest_set_qc(R->host, R->qc);          // (the same accumulator goes on, in stream order)
	return rc;
}

}  // namespace

// kmahip_ingest_open for the device reader (run_input / run_input_PE, runinput.c:370-606, over plain FASTQ files). An input it does not
// cover -- .gz, FASTA, anything that is no regular file -- is refused with KMAHIP_EFORMAT before the first HIP call.
extern "C" int kmahip_ingest_dev_open(const char *path1, const char *path2, const kmahip_trim *trim, kmahip_ingest_dev **out) {
	if(!path1 || !out) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	*out = nullptr;
	Reader *R = new Reader();
	if(trim) R->trim = *trim; else kmahip_trim_default(&R->trim);
	// kma.c:1555-1557, runinput.c:380-382
	if(R->trim.min_phred < R->trim.hardmask_q) R->trim.min_phred = R->trim.hardmask_q;
	if(R->trim.min_phred < R->trim.min_q) R->trim.min_phred = R->trim.min_q;
	R->mates = path2 ? 2 : 1;
	const char *paths[2] = {path1, path2};
	int kind[2] = {0, 0};
	std::vector<uint8_t> first[2];
	auto refuse = [&](int rc) { for(int m = 0; m < 2; ++m) if(R->m[m].fd >= 0) ::close(R->m[m].fd); delete R; return rc; };
	for(int m = 0; m < R->mates; ++m) {
		R->path[m] = paths[m];
		MateIn &M = R->m[m];
		M.fd = ::open(paths[m], O_RDONLY);
		if(M.fd < 0) { kmahip_set_error("cannot open %s", paths[m]); return refuse(KMAHIP_EIO); }
		struct stat sb;
		if(fstat(M.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { kmahip_set_error("%s is not a regular file: the device reader takes plain FASTQ files only", paths[m]); return refuse(KMAHIP_EFORMAT); }
		M.size = (size_t) sb.st_size;
		first[m].resize(std::min(M.size, FIRST_CHUNK));
		size_t got = 0;
		while(got < first[m].size()) {
			const ssize_t g = pread(M.fd, first[m].data() + got, first[m].size() - got, (off_t) got);
			if(g <= 0) { kmahip_set_error("cannot read %s", paths[m]); return refuse(KMAHIP_EIO); }
			got += (size_t) g;
		}
		if(got >= 2 && first[m][0] == 0x1f && first[m][1] == 0x8b) { kmahip_set_error("%s is gzip-compressed: the device reader takes plain FASTQ files only", paths[m]); return refuse(KMAHIP_EFORMAT); }
		const uint8_t c = got ? first[m][0] : 0;
		kind[m] = c == '@' ? 1 : (c == '>' ? 2 : 0);
		if(kind[m] == 2) { kmahip_set_error("%s is FASTA: the device reader takes plain FASTQ files only", paths[m]); return refuse(KMAHIP_EFORMAT); }
		if(got && !kind[m]) { kmahip_set_error("cannot determine format of file %s", paths[m]); return refuse(KMAHIP_EFORMAT); }
	}
	if(R->mates == 2 && kind[0] != kind[1]) { kmahip_set_error("%s and %s are in different formats", path1, path2); return refuse(KMAHIP_EFORMAT); }
	if(kind[0] == 1) {
		R->phred = kmahip_ingest_guess_phred(first[0].data(), first[0].size());
		if(R->mates == 2 && R->phred == 0) R->phred = kmahip_ingest_guess_phred(first[1].data(), first[1].size());
	}
	{	// threads that read the file (KMAHIP_INGEST_THREADS, else the hardware threads, at most 16: as ingest.hip)
		const char *e = getenv("KMAHIP_INGEST_THREADS");
		const int hw = (int) std::thread::hardware_concurrency();
		R->threads = e ? atoi(e) : std::min(16, hw > 0 ? hw : 1);
		R->threads = std::max(1, std::min(R->threads, 16));
	}
	// KMAHIP_INGEST_DEV_CHUNK: bytes of input per chunk (64 MiB; small ones make small test files cross chunk borders)
	if(const char *c = getenv("KMAHIP_INGEST_DEV_CHUNK")) R->chunk = (size_t) std::max(64, atoi(c));
	R->piece = std::min<size_t>(16u << 20, (R->chunk + 4095) / 4096 * 4096);
	TrimDev &P = R->P;
	P.min_phred_raw = R->phred + R->trim.min_phred; P.min_q = R->trim.min_q; P.hardmask_q = R->trim.hardmask_q;
	P.min_len = R->trim.min_len; P.max_len = R->trim.max_len;
	P.plain = !R->trim.min_q && !R->trim.hardmask_q; P.paired = R->mates == 2;
	P.minP = pow(10, (-0.1) * R->trim.min_q);
	// from here on the device: the one current now is the reader's
	if(hipGetDevice(&R->device) != hipSuccess) { kmahip_set_error("no HIP device"); return refuse(KMAHIP_EDEVICE); }
	const int rc = bring_up(R);
	if(rc) { kmahip_ingest_dev_close(R); return rc; }
	*out = R;
	return KMAHIP_OK;
}

// kmahip_ingest_next for the device reader: up to max_records further S1 records (printFsa / printFsa_pair order, runinput.c:765-830).
// The batch's arrays are device pointers, its pair flags host memory; all valid until the next call.
extern "C" int kmahip_ingest_dev_next(kmahip_ingest_dev *R, int64_t max_records, kmahip_read_batch *batch) {
	if(!R || !batch || max_records < 0) { kmahip_set_error("bad argument"); return KMAHIP_EINVAL; }
	HIP_TRY(hipSetDevice(R->device));
	int rc = min_out(R);
	if(rc) return rc;
	R->started = true;
	R->text_tot[0] = R->text_tot[1] = 0;
	R->h_text[0].clear(); R->h_text[1].clear();
	memset(batch, 0, sizeof *batch);
	int64_t tot[4] = {0, 0, 0, 0};
	int max_len = 0;
	R->h_pair.clear();
	if(R->host) {
		// the host reader's batch, placed on the device like the reader's own
		kmahip_read_batch hb;
		rc = kmahip_ingest_next(R->host, max_records, &hb);
		kmahip_ingest_counts(R->host, &R->n_read, &R->n_kept);
		const int64_t n = rc ? 0 : hb.reads.n_reads;
		if(n) {
			int rc2;
			if((rc2 = R->o_seq.ensure((size_t) (hb.reads.seq_words + 2) * 8, 0, R->s)) || (rc2 = R->o_seq_off.ensure((size_t) (n + 1) * 8, 0, R->s)) || (rc2 = R->o_N_off.ensure((size_t) (n + 1) * 8, 0, R->s)) ||
			   (rc2 = R->o_name_off.ensure((size_t) (n + 1) * 8, 0, R->s)) || (rc2 = R->o_len.ensure((size_t) (n + 1) * 4, 0, R->s)) || (rc2 = R->o_names.ensure((size_t) hb.name_off[n] + 1, 0, R->s)) ||
			   (rc2 = R->o_N.ensure((size_t) (hb.reads.N_total + 1) * 4, 0, R->s))) return rc2;
			HIP_TRY(hipMemcpyAsync(R->o_seq.p, hb.reads.seq, (size_t) hb.reads.seq_words * 8, hipMemcpyHostToDevice, R->s));
			HIP_TRY(hipMemcpyAsync(R->o_seq_off.p, hb.reads.seq_off, (size_t) (n + 1) * 8, hipMemcpyHostToDevice, R->s));
			HIP_TRY(hipMemcpyAsync(R->o_N_off.p, hb.reads.N_off, (size_t) (n + 1) * 8, hipMemcpyHostToDevice, R->s));
			HIP_TRY(hipMemcpyAsync(R->o_name_off.p, hb.name_off, (size_t) (n + 1) * 8, hipMemcpyHostToDevice, R->s));
			HIP_TRY(hipMemcpyAsync(R->o_len.p, hb.reads.len, (size_t) n * 4, hipMemcpyHostToDevice, R->s));
			if(hb.name_off[n]) HIP_TRY(hipMemcpyAsync(R->o_names.p, hb.names, (size_t) hb.name_off[n], hipMemcpyHostToDevice, R->s));
			if(hb.reads.N_total) HIP_TRY(hipMemcpyAsync(R->o_N.p, hb.reads.N, (size_t) hb.reads.N_total * 4, hipMemcpyHostToDevice, R->s));
			HIP_TRY(hipStreamSynchronize(R->s));
			R->h_pair.assign(hb.pair, hb.pair + n);
			tot[0] = n; tot[1] = hb.reads.seq_words; tot[2] = hb.reads.N_total; tot[3] = hb.name_off[n];
			max_len = hb.reads.max_len;
			batch->records = hb.records;
			for(int k = 0; k < 2 && R->text; ++k) {
				const char *tx = nullptr;
				int64_t nb = 0;
				if(!kmahip_ingest_text(R->host, k, &tx, &nb)) R->h_text[k].assign(tx, tx + nb);
			}
		}
		if(rc) return rc;
	} else {
		const auto t0 = std::chrono::steady_clock::now();
		const double io0 = R->ms_read + R->ms_copy;
		int *d_max_len = R->small.as<int>() + 4;
		HIP_TRY(hipMemsetAsync(d_max_len, 0, sizeof(int), R->s));
		int64_t records = 0;
		bool to_host = false;
		// (a batch of long reads also closes once it holds a quarter of a gigabase, checked between the chunks: HBM is the bound)
		while(records < max_records && tot[1] < (int64_t) (8 << 20)) {
			int64_t avail = INT64_MAX;
			bool all_done = true;
			for(int m = 0; m < R->mates && !to_host; ++m) {
				MateIn &M = R->m[m];
				if(!M.done && !M.handback && M.cur >= M.usable && (rc = next_chunk(R, M))) return rc;
				if(M.handback) to_host = true;
				if(!M.done) { all_done = false; avail = std::min(avail, M.usable - M.cur); }
			}
			if(to_host || all_done) break;
			// (as many input records as the batch still has room for kept ones, like kmahip_ingest_next)
			const int64_t take = std::min(avail, max_records - records);
			if((rc = run_pass(R, take, tot, d_max_len, &records))) return rc;
			R->n_read += take;
		}
		hipLaunchKernelGGL(s1_ends_kernel, dim3(1), dim3(64), 0, R->s,
		                   OutView{R->o_seq.as<uint64_t>(), R->o_seq_off.as<int64_t>(), R->o_N_off.as<int64_t>(), R->o_name_off.as<int64_t>(), nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0},
		                   tot[0], tot[1], tot[2], tot[3]);
		HIP_TRY(hipGetLastError());
		R->h_pair.resize((size_t) tot[0]);
		if(tot[0]) HIP_TRY(hipMemcpyAsync(R->h_pair.data(), R->o_pair.p, (size_t) tot[0], hipMemcpyDeviceToHost, R->s));
		HIP_TRY(hipMemcpyAsync(R->h_small + 8, d_max_len, sizeof(int), hipMemcpyDeviceToHost, R->s));
		for(int k = 0; k < 2 && R->text; ++k) {
			R->h_text[k].resize((size_t) R->text_tot[k]);
			if(R->text_tot[k]) HIP_TRY(hipMemcpyAsync(R->h_text[k].data(), R->d_text[k].p, (size_t) R->text_tot[k], hipMemcpyDeviceToHost, R->s));
		}
		HIP_TRY(hipStreamSynchronize(R->s));
		max_len = *(const int *) (R->h_small + 8);
		batch->records = records;
		R->n_kept += records;
		R->ms_kernel += ms_since(t0) - (R->ms_read + R->ms_copy - io0);
		if(R->qc) kmahip_qc_end_reader(R->qc, R->mates == 2, R->phred);
		if(to_host) {
			if((rc = hand_back(R))) return rc;
			// what the device made of the records before the odd one is this batch; with nothing in hand the host reader answers now
			if(tot[0] == 0) return kmahip_ingest_dev_next(R, max_records, batch);
		}
	}
	R->h_pair.reserve(1);
	batch->reads.n_reads = tot[0];
	batch->reads.seq = R->o_seq.as<uint64_t>(); batch->reads.seq_off = R->o_seq_off.as<int64_t>(); batch->reads.len = R->o_len.as<int32_t>();
	batch->reads.N = R->o_N.as<int32_t>(); batch->reads.N_off = R->o_N_off.as<int64_t>();
	batch->reads.seq_words = tot[1]; batch->reads.N_total = tot[2]; batch->reads.max_len = max_len;
	batch->names = R->o_names.p; batch->name_off = R->o_name_off.as<int64_t>(); batch->pair = R->h_pair.data();
	return KMAHIP_OK;
}

// kmahip_ingest_set_qc for the device reader: from now on the records kernel's -qc instantiation runs, s1_qc_kernel reduces every pass
// and the accumulator is fed pass by pass, in stream order; the host reader that takes over at an odd record is given it as well
extern "C" int kmahip_ingest_dev_set_qc(kmahip_ingest_dev *R, kmahip_qc *qc) {
	if(!R || !qc) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(R->started) { kmahip_set_error("a QC accumulator is attached before the first batch is read"); return KMAHIP_EINVAL; }
	if(R->trim.min_len < 1) { kmahip_set_error("a QC report needs a minimum length of 1 at least (the reference divides by the length of a kept read)"); return KMAHIP_EINVAL; }
	HIP_TRY(hipSetDevice(R->device));
	int rc = R->qstat.ensure(sizeof(QcStat), 0, R->s);
	if(rc) return rc;
	HIP_TRY(hipMemsetAsync(R->qstat.p, 0, sizeof(QcStat), R->s));
	HIP_TRY(hipStreamSynchronize(R->s));
	if(!R->h_qstat) HIP_TRY(hipHostMalloc((void **) &R->h_qstat, sizeof(QcStat), hipHostMallocDefault));
	R->qc = qc;
	kmahip_qc_end_reader(qc, R->mates == 2, R->phred);
	return KMAHIP_OK;
}

extern "C" void kmahip_ingest_dev_qc_timing(const kmahip_ingest_dev *R, double ms[2]) {
	if(ms) { ms[0] = R ? R->ms_qc_copy : 0; ms[1] = R ? R->ms_qc_bin : 0; }
}

// kmahip_ingest_set_text / kmahip_ingest_text for the device reader: s1_fastq_kernel writes the text of every pass, the batch's text
// comes back with the batch (HOST memory, valid until the next call); the host reader's part of an odd file is its own text
extern "C" int kmahip_ingest_dev_set_text(kmahip_ingest_dev *R, int on) {
	if(!R) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(R->started) { kmahip_set_error("the text sink is set before the first batch is read"); return KMAHIP_EINVAL; }
	R->text = on != 0;
	return KMAHIP_OK;
}

extern "C" int kmahip_ingest_dev_text(const kmahip_ingest_dev *R, int stream, const char **text, int64_t *bytes) {
	if(!R || !text || !bytes || stream < 0 || stream > 1) { kmahip_set_error("bad argument"); return KMAHIP_EINVAL; }
	*text = R->h_text[stream].empty() ? "" : R->h_text[stream].data();
	*bytes = (int64_t) R->h_text[stream].size();
	return KMAHIP_OK;
}

// kmahip_ingest_status for the device reader: only the host reader's part of an input can break off ("Malformed input.", seqparse.c:256-260)
extern "C" int kmahip_ingest_dev_status(kmahip_ingest_dev *R) {
	if(!R) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	return R->host ? kmahip_ingest_status(R->host) : KMAHIP_OK;
}

// getPhredFileBuff's answer (seqparse.c:551-589): 33, 64 or 0
extern "C" int kmahip_ingest_dev_phred_scale(const kmahip_ingest_dev *R) { return R ? R->phred : 0; }

// records read / kept so far (what run_input counts, runinput.c:404-424), the host reader's part included
extern "C" void kmahip_ingest_dev_counts(const kmahip_ingest_dev *R, int64_t *records_read, int64_t *records_kept) {
	if(records_read) *records_read = R ? R->n_read : 0;
	if(records_kept) *records_kept = R ? R->n_kept : 0;
}

// bytes of input that were left to the host reader (0: the device delivered every record itself)
extern "C" int64_t kmahip_ingest_dev_handed_back(const kmahip_ingest_dev *R) { return R ? R->handed : 0; }

// where the time of the device part went, in ms: reading the files into pinned memory, waiting for the copies, everything else
// (kernels, scans and the figures that come back), and the bytes of input that went up
extern "C" void kmahip_ingest_dev_timing(const kmahip_ingest_dev *R, double ms[3], int64_t *bytes) {
	if(ms) { ms[0] = R ? R->ms_read : 0; ms[1] = R ? R->ms_copy : 0; ms[2] = R ? R->ms_kernel : 0; }
	if(bytes) *bytes = R ? R->bytes_in : 0;
}

// for callers without a HIP runtime of their own (the Python binding, tests): bytes of a batch's device arrays copied to host memory
extern "C" int kmahip_ingest_dev_copy_out(void *host_dst, const void *dev_src, size_t bytes) {
	if(bytes && (!host_dst || !dev_src)) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(bytes) HIP_TRY(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
	return KMAHIP_OK;
}

extern "C" void kmahip_ingest_dev_close(kmahip_ingest_dev *R) {
	if(!R) return;
	if(R->host) kmahip_ingest_close(R->host);
	for(int m = 0; m < 2; ++m) if(R->m[m].fd >= 0) ::close(R->m[m].fd);
	if(R->dev_up || R->s || R->cs) {
		(void) hipSetDevice(R->device);
		if(R->s) (void) hipStreamSynchronize(R->s);
		if(R->cs) (void) hipStreamSynchronize(R->cs);
		for(int k = 0; k < kmahip_ingest_dev::NPIN; ++k) { if(R->pin[k]) (void) hipHostFree(R->pin[k]); if(R->pin_free[k]) (void) hipEventDestroy(R->pin_free[k]); }
		if(R->pass_done) (void) hipEventDestroy(R->pass_done);
		if(R->h_small) (void) hipHostFree(R->h_small);
		if(R->h_qstat) (void) hipHostFree(R->h_qstat);
		if(R->qc && getenv("KMAHIP_DEBUG_TIMING")) fprintf(stderr, "[kmahip] ingest_dev: QC report: %.1f ms fetching the counted sequences, %.1f ms summing and binning them on the host\n", R->ms_qc_copy, R->ms_qc_bin);
	}
	hipStream_t s = R->s, cs = R->cs;
	delete R;                                    // (the device arrays)
	if(s) (void) hipStreamDestroy(s);
	if(cs) (void) hipStreamDestroy(cs);
}
