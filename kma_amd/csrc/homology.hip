// homology.hip -- the counts behind `kma index -Sparse ... -hq x -ht y [-and]` (queryCheck / templateCheck, qualcheck.c:81-324) on the
// device. The reference looks every window of a new template up in the index of the templates kept so far and scores them; which
// templates are kept is a serial chain, but what a pair (new template i, earlier template j) scores depends on the two sequences alone:
//   Scores_tot[j]  windows of i, repeats and all, whose k-mer j holds          (updateScoreAndTemplate)
//   Scores[j]      distinct k-mers of i that j holds                            (addUscore behind hashMap_CountKmer)
//   first met      the walk position (forward strand, then the reverse complement) of i's first window whose k-mer j holds: the
//                  order of bestTemplates, which settles a tie (inside one value list the lower id comes first)
// So the rows are counted here under the ids of the file order, a workgroup per row in the spirit of tdist_rows_kernel, twice:
// pass 1 (hom_rows_kernel<false>) writes the pairs that can reject their row, as two flags from the reference's own double expressions;
// the host settles kept / rejected in file order (hom_resolve, index_host.h); pass 2 (hom_rows_kernel<true>) reduces every row over the
// kept columns to the winners the report names. Integers go back; the host forms the doubles it prints.
//
// Two sorted views of index_sparse_keys_kernel's windows feed the rows: `rows` = (template << 32 | k-mer) with the walk position as
// its value, a run of equal keys being one distinct k-mer of the row with its repeats; `lists` = the unique (k-mer << 32 | template),
// a k-mer's run being its value list over all candidates in ascending id.
#include "kmahip_internal.h"
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdlib>

struct KmaHom {
	int n_t = 0;
	int64_t n_keys = 0, min_klen = 1;
	size_t n_lists = 0;                          // unique (k-mer, template) pairs
	uint32_t cols = 0;
	unsigned long long *rows = nullptr, *lists = nullptr;
	uint32_t *pos = nullptr, *ulen = nullptr, *slen = nullptr;
	int64_t *row_start = nullptr;                // [n_t + 1] into rows / pos
	std::vector<void *> allocs;
};

namespace {

constexpr int HOM_BLOCK = 256;
constexpr uint32_t HOM_COLS_MAX = 4096;          // columns of a row summed at once: three words each, 48 KiB of LDS
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct SameKey { __device__ bool operator()(unsigned long long a, unsigned long long b) const { return a == b; } };

// a thread per key of index_sparse_keys_kernel (keys[2 p]: the forward window at base p, keys[2 p + 1]: the reverse strand's) -> the
// row view: template << 32 | k-mer, and where the reference's walk meets the window: p on the forward strand, behind it len + (len - w
// - p) on the reverse complement, whose walk runs down the forward coordinates
__global__ __launch_bounds__(256) void hom_row_keys_kernel(const unsigned long long *keys, int64_t n, const int64_t *t_off, int w, unsigned long long *rows, uint32_t *pos) {
	const int64_t q = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(q >= n) return;
	const unsigned long long key = keys[q];
	unsigned long long r = ~0ull;
	uint32_t at = 0;
	if(key != ~0ull) {
		const uint32_t id = (uint32_t) key;
		const int64_t a = t_off[id - 1], len = t_off[id] - a, p = (q >> 1) - a;
		at = (uint32_t) ((q & 1) ? len + (len - w - p) : p);
		r = ((unsigned long long) id << 32) | (key >> 32);
	}
	rows[q] = r;
	pos[q] = at;
}

// ulen[t] = the distinct window k-mers of template t: the heads of the runs of the row view
__global__ __launch_bounds__(256) void hom_ulen_kernel(const unsigned long long *rows, int64_t n, uint32_t *ulen) {
	const int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= n) return;
	const unsigned long long r = rows[e];
	if(r == ~0ull || (e && rows[e - 1] == r)) return;
	atomicAdd(&ulen[(uint32_t) (r >> 32) - 1], 1u);
}

struct Best { uint32_t tot, first, j; };                   // the winner by Scores_tot
struct BestT { uint32_t num, den, first, j; };              // the winner by Scores / ulen

__device__ __forceinline__ bool met_before(uint32_t fa, uint32_t ja, uint32_t fb, uint32_t jb) { return fa < fb || (fa == fb && ja < jb); }
// thisQ's share one denominator, so the integers order them; a strict `>` keeps the one met first
__device__ __forceinline__ void take(Best &b, uint32_t tot, uint32_t first, uint32_t j) {
	if(tot > b.tot || (tot == b.tot && tot && met_before(first, j, b.first, b.j))) b = Best{tot, first, j};
}
// thisT = 1.0 * Scores / ulen as the reference forms it, compared as doubles
__device__ __forceinline__ void take(BestT &b, uint32_t num, uint32_t den, uint32_t first, uint32_t j) {
	if(!num) return;
	const double v = 1.0 * num / den, w = b.num ? 1.0 * b.num / b.den : 0.0;
	if(v > w || (v == w && met_before(first, j, b.first, b.j))) b = BestT{num, den, first, j};
}

struct RowArgs {
	const unsigned long long *rows, *lists;
	const uint32_t *pos, *ulen, *slen;
	const int64_t *row_start;
	int64_t n_lists, min_klen;
	uint32_t cols;
	// pass 1
	double homQ, homT;
	int use_t;
	KmaHomPair *pairs;
	unsigned long long cap, *cursor;
	// pass 2
	const uint8_t *kept;
	KmaHomRow *out;
};

// Workgroup i takes row i: columns j < i in blocks of `cols`, three accumulators a column in LDS. A thread that holds the head of a run
// of the row view has a distinct k-mer, its repeats and its first walk position; it finds the k-mer's list from column c0 on by binary
// search and adds to every column of the block. BEST = false: the columns whose ratios reach a threshold go to the pair list (the
// cursor counts on past the capacity, so that a list that did not fit is known and by how much). BEST = true: the kept columns are
// reduced to the row's two winners
template <bool BEST>
__global__ __launch_bounds__(HOM_BLOCK) void hom_rows_kernel(const RowArgs A) {
	extern __shared__ __attribute__((aligned(16))) uint32_t hom_lds[];          // [cols] Scores_tot, [cols] Scores, [cols] first met
	__shared__ Best red_q[HOM_BLOCK];
	__shared__ BestT red_t[HOM_BLOCK];
	const uint32_t i = blockIdx.x;
	const int64_t a = A.row_start[i], b = A.row_start[i + 1];
	if(i == 0 || b - a < A.min_klen || b == a) return;          // (whole workgroups leave; the row's output stays zero)
	const uint32_t klen = A.slen[i];
	uint32_t *tot = hom_lds, *uniq = hom_lds + A.cols, *first = hom_lds + 2 * A.cols;
	Best bq{0, NONE, NONE};
	BestT bt{0, 1, NONE, NONE};
	for(uint32_t c0 = 0; c0 < i; c0 += A.cols) {
		const uint32_t w = min(A.cols, i - c0);
		for(uint32_t c = threadIdx.x; c < w; c += HOM_BLOCK) { tot[c] = 0; uniq[c] = 0; first[c] = NONE; }
		__syncthreads();
		for(int64_t e = a + threadIdx.x; e < b; e += HOM_BLOCK) {
			const unsigned long long r = A.rows[e];
			if(e > a && A.rows[e - 1] == r) continue;
			uint32_t cnt = 1, at = A.pos[e];
			for(int64_t f = e + 1; f < b && A.rows[f] == r; ++f) { ++cnt; at = min(at, A.pos[f]); }
			const unsigned long long km = r << 32, from = km | (unsigned long long) (c0 + 1);
			int64_t lo = 0, hi = A.n_lists;                   // first pair >= (k-mer, template c0 + 1)
			while(lo < hi) { const int64_t mid = (lo + hi) >> 1; if(A.lists[mid] < from) lo = mid + 1; else hi = mid; }
			for(; lo < A.n_lists; ++lo) {
				const unsigned long long u = A.lists[lo];
				if((u & 0xFFFFFFFF00000000ull) != km) break;
				const uint32_t c = (uint32_t) u - 1u - c0;          // (template ids are 1-based; c >= 0 by the search)
				if(c >= w) break;
				atomicAdd(&tot[c], cnt);
				atomicAdd(&uniq[c], 1u);
				atomicMin(&first[c], at);
			}
		}
		__syncthreads();
		for(uint32_t c = threadIdx.x; c < w; c += HOM_BLOCK) {
			if(!tot[c]) continue;
			const uint32_t j = c0 + c;
			if(BEST) {
				if(!A.kept[j]) continue;
				take(bq, tot[c], first[c], j);
				take(bt, uniq[c], A.ulen[j], first[c], j);
			} else {
				const bool fq = 1.0 * tot[c] / klen >= A.homQ;
				const bool ft = A.use_t && 1.0 * uniq[c] / A.ulen[j] >= A.homT;
				if(fq || ft) {
					const unsigned long long slot = atomicAdd(A.cursor, 1ull);
					if(slot < A.cap) A.pairs[slot] = KmaHomPair{i, (j << 2) | (uint32_t) fq | ((uint32_t) ft << 1)};
				}
			}
		}
		__syncthreads();
	}
	if(!BEST) return;
	red_q[threadIdx.x] = bq;
	red_t[threadIdx.x] = bt;
	__syncthreads();
	for(int s = HOM_BLOCK / 2; s > 0; s >>= 1) {
		if((int) threadIdx.x < s) {
			const Best q = red_q[threadIdx.x + s];
			const BestT t = red_t[threadIdx.x + s];
			take(red_q[threadIdx.x], q.tot, q.first, q.j);
			take(red_t[threadIdx.x], t.num, t.den, t.first, t.j);
		}
		__syncthreads();
	}
	if(threadIdx.x == 0) {
		const Best q = red_q[0];
		const BestT t = red_t[0];
		A.out[i] = KmaHomRow{q.tot, q.tot ? q.j + 1 : 0, t.num, t.num ? t.den : 0, t.num ? t.j + 1 : 0};
	}
}

template <class T>
int hom_room(KmaHom *h, size_t count, T **dst) {
	void *d = nullptr;
	const size_t bytes = (count ? count : 1) * sizeof(T);
	if(hipMalloc(&d, bytes) != hipSuccess) { (void) hipGetLastError(); kmahip_set_error("%zu bytes of device memory for the homology counts", bytes); return KMAHIP_ENOMEM; }
	h->allocs.push_back(d);
	*dst = (T *) d;
	return KMAHIP_OK;
}

void hom_fill(const KmaHom *h, RowArgs &A) {
	A = RowArgs{};
	A.rows = h->rows; A.lists = h->lists; A.pos = h->pos; A.ulen = h->ulen; A.slen = h->slen; A.row_start = h->row_start;
	A.n_lists = (int64_t) h->n_lists; A.min_klen = h->min_klen; A.cols = h->cols;
}

}  // namespace

void kmahip_hom_close(KmaHom *h) {
	if(!h) return;
	for(void *p : h->allocs) (void) hipFree(p);
	delete h;
}

int kmahip_hom_open(const unsigned long long *d_keys, int64_t n_keys, const int64_t *d_off, const std::vector<uint32_t> &slen, int w, int64_t min_klen, KmaHom **out) {
	*out = nullptr;
	const int n_t = (int) slen.size();
	if(n_t >= (1 << 30)) { kmahip_set_error("homology reduction: %d templates, below 2^30 served", n_t); return KMAHIP_EINVAL; }
	KmaHom *h = new KmaHom();
	struct Guard { KmaHom *h; ~Guard() { kmahip_hom_close(h); } } guard{h};
	h->n_t = n_t; h->n_keys = n_keys; h->min_klen = min_klen;
	// KMAHIP_HOM_BLOCK: the columns of a block, for the test of the block edges
	h->cols = HOM_COLS_MAX;
	if(const char *e = getenv("KMAHIP_HOM_BLOCK")) { const long c = atol(e); if(c >= 1 && (uint32_t) c < h->cols) h->cols = (uint32_t) c; }
	std::vector<int64_t> start((size_t) n_t + 1, 0);
	for(int t = 0; t < n_t; ++t) start[(size_t) t + 1] = start[(size_t) t] + slen[(size_t) t];
	const int64_t n_win = start[(size_t) n_t];
	unsigned long long *raw = nullptr, *sorted = nullptr;
	uint32_t *raw_pos = nullptr;
	size_t *d_count = nullptr;
	void *d_tmp = nullptr;
	int rc;
	if((rc = hom_room(h, (size_t) n_keys, &raw)) || (rc = hom_room(h, (size_t) n_keys, &raw_pos)) || (rc = hom_room(h, (size_t) n_keys, &h->rows)) ||
	   (rc = hom_room(h, (size_t) n_keys, &h->pos)) || (rc = hom_room(h, (size_t) n_keys, &sorted)) || (rc = hom_room(h, (size_t) n_keys, &h->lists)) ||
	   (rc = hom_room(h, (size_t) n_t, &h->ulen)) || (rc = hom_room(h, (size_t) n_t, &h->slen)) || (rc = hom_room(h, (size_t) n_t + 1, &h->row_start)) ||
	   (rc = hom_room(h, 1, &d_count))) return rc;
	HIP_TRY(hipMemcpy(h->slen, slen.data(), (size_t) n_t * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(h->row_start, start.data(), start.size() * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipMemset(h->ulen, 0, (size_t) n_t * 4));
	const unsigned blocks = (unsigned) ((n_keys + 255) / 256);
	hipLaunchKernelGGL(hom_row_keys_kernel, dim3(blocks), dim3(256), 0, 0, d_keys, n_keys, d_off, w, raw, raw_pos);
	HIP_TRY(hipGetLastError());
	size_t t1 = 0, t2 = 0, t3 = 0;
	if(rocprim::radix_sort_pairs(nullptr, t1, raw, h->rows, raw_pos, h->pos, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::radix_sort_keys(nullptr, t2, d_keys, sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(nullptr, t3, sorted, h->lists, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim size query failed"); return KMAHIP_EDEVICE; }
	size_t tmp_bytes = std::max(t1, std::max(t2, t3));
	if((rc = hom_room(h, tmp_bytes ? tmp_bytes : 16, (uint8_t **) &d_tmp))) return rc;
	if(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, raw, h->rows, raw_pos, h->pos, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::radix_sort_keys(d_tmp, tmp_bytes, d_keys, sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(d_tmp, tmp_bytes, sorted, h->lists, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim sort / unique failed"); return KMAHIP_EDEVICE; }
	HIP_TRY(hipMemcpy(&h->n_lists, d_count, sizeof h->n_lists, hipMemcpyDeviceToHost));
	if(h->n_lists > (size_t) n_keys) { kmahip_set_error("rocprim unique returned %zu of %lld keys", h->n_lists, (long long) n_keys); return KMAHIP_EDEVICE; }
	if(h->n_lists) {
		// the keys that hold no window sorted to the end, in both views
		unsigned long long last = 0;
		HIP_TRY(hipMemcpy(&last, h->lists + (h->n_lists - 1), 8, hipMemcpyDeviceToHost));
		if(last == ~0ull) --h->n_lists;
	}
	if(n_win) {
		hipLaunchKernelGGL(hom_ulen_kernel, dim3((unsigned) ((n_win + 255) / 256)), dim3(256), 0, 0, h->rows, n_win, h->ulen);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipDeviceSynchronize());
	guard.h = nullptr;
	*out = h;
	return KMAHIP_OK;
}

// pass 1 -> the pairs (row, column * 4 + flags: 1 = thisQ >= homQ, 2 = thisT >= homT; use_t false: queryCheck, which never forms
// thisT), in no order. The list starts at KMAHIP_HOM_PAIRS entries (the default: a million, or sixteen a row) and, when the cursor ran
// past it, is made again at the size the cursor reached: every row writes the same pairs again
int kmahip_hom_pairs(KmaHom *h, double homQ, double homT, bool use_t, std::vector<KmaHomPair> &pairs) {
	pairs.clear();
	if(h->n_t < 2) return KMAHIP_OK;
	unsigned long long cap = std::max<unsigned long long>(1ull << 20, 16ull * (unsigned long long) h->n_t);
	if(const char *e = getenv("KMAHIP_HOM_PAIRS")) { const long long c = atoll(e); if(c >= 1) cap = (unsigned long long) c; }
	unsigned long long *cursor = nullptr;
	int rc = hom_room(h, 1, &cursor);
	if(rc) return rc;
	const size_t shm = (size_t) h->cols * 12;
	for(int attempt = 0; attempt < 2; ++attempt) {
		KmaHomPair *d_pairs = nullptr;
		if(hipMalloc((void **) &d_pairs, (size_t) cap * sizeof(KmaHomPair)) != hipSuccess) { (void) hipGetLastError(); kmahip_set_error("%llu pairs of the homology list do not fit the device", cap); return KMAHIP_ENOMEM; }
		struct Free { void *p; ~Free() { (void) hipFree(p); } } fr{d_pairs};
		HIP_TRY(hipMemset(cursor, 0, 8));
		RowArgs A;
		hom_fill(h, A);
		A.homQ = homQ; A.homT = homT; A.use_t = use_t; A.pairs = d_pairs; A.cap = cap; A.cursor = cursor;
		hipLaunchKernelGGL(hom_rows_kernel<false>, dim3((unsigned) h->n_t), dim3(HOM_BLOCK), shm, 0, A);
		HIP_TRY(hipGetLastError());
		unsigned long long n = 0;
		HIP_TRY(hipMemcpy(&n, cursor, 8, hipMemcpyDeviceToHost));
		if(n <= cap) {
			pairs.resize((size_t) n);
			if(n) HIP_TRY(hipMemcpy(pairs.data(), d_pairs, (size_t) n * sizeof(KmaHomPair), hipMemcpyDeviceToHost));
			return KMAHIP_OK;
		}
		cap = n;
	}
	kmahip_set_error("the homology pair list outgrew the size its own count gave");
	return KMAHIP_EDEVICE;
}

// pass 2 -> per row the winners over the kept columns (ids of the file order, 1-based; 0: none met)
int kmahip_hom_best(KmaHom *h, const std::vector<uint8_t> &kept, std::vector<KmaHomRow> &rows) {
	rows.assign((size_t) h->n_t, KmaHomRow{0, 0, 0, 0, 0});
	if(h->n_t < 2) return KMAHIP_OK;
	uint8_t *d_kept = nullptr;
	KmaHomRow *d_out = nullptr;
	int rc;
	if((rc = hom_room(h, (size_t) h->n_t, &d_kept)) || (rc = hom_room(h, (size_t) h->n_t, &d_out))) return rc;
	HIP_TRY(hipMemcpy(d_kept, kept.data(), (size_t) h->n_t, hipMemcpyHostToDevice));
	HIP_TRY(hipMemset(d_out, 0, (size_t) h->n_t * sizeof(KmaHomRow)));
	RowArgs A;
	hom_fill(h, A);
	A.kept = d_kept; A.out = d_out;
	hipLaunchKernelGGL(hom_rows_kernel<true>, dim3((unsigned) h->n_t), dim3(HOM_BLOCK), (size_t) h->cols * 12, 0, A);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpy(rows.data(), d_out, (size_t) h->n_t * sizeof(KmaHomRow), hipMemcpyDeviceToHost));
	return KMAHIP_OK;
}
