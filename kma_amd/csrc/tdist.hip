// tdist.hip -- template distances (`kma dist`, dist.c) on the device: the reader of <db>.comp.b that loadValues is (:38-162; no key is
// read, so every form of index is served), kmerSimilarity (:171-225) as counting kernels over the distinct value lists, and the PHYLIP
// text of runDist / threadDist (:336-875) formatted a cell per thread. A pipeline of its own beside the mapping one, like sparse.hip.
//
// Counting. Many k-mers point to one value list: tdist_mult_kernel counts them per list, and a pair of a list then adds that
// multiplicity once. Two forms of the pair sums give the same arrays (integer sums do not depend on order): "rows" makes an inverted
// index template -> lists and sums each row of the triangle in LDS, stored with plain coalesced stores; "pairs" is the plain form, a
// wavefront per list with a global atomic add per pair. KMAHIP_TDIST_FORM chooses.
#include "kmahip_internal.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

struct kmahip_tdist {
	kmahip_tdist_info info{};
	uint32_t n = 0;                          // templates: DB_size - 1, the rows of the matrix
	std::vector<std::string> names;          // [n]
	std::vector<void *> allocs;
	// device
	const void *values = nullptr;            // the value array: [length, ids ...] lists, 16- or 32-bit
	uint32_t *entries = nullptr;             // [n_entries] the per-k-mer entries up to the n-th live one
	uint64_t n_entries = 0;
	uint32_t *list_off = nullptr;            // [n_lists] offsets of the distinct lists
	uint32_t *mult = nullptr;                // [n_values] k-mers that point to the list at this offset
	int32_t *N = nullptr, *D = nullptr;      // [n], [n (n - 1) / 2]
	uint32_t *inv_cnt = nullptr, *inv_cur = nullptr, *inv = nullptr;      // the inverted index: [n + 1] starts, [n] cursors, [sum of lengths] list numbers
	uint64_t n_elems = 0;                    // sum of the lengths of the distinct lists
	double *sq = nullptr;                    // [n] sqrt(N[t]) by the host's libm
	bool counted = false, sq_there = false;
	std::vector<int32_t> h_N;
	int timing = 0;
	double ms[KMAHIP_TDIST_KERNELS] = {0, 0, 0, 0, 0};
	int64_t launches[KMAHIP_TDIST_KERNELS] = {0, 0, 0, 0, 0};
};

namespace {

constexpr int WAVE = 64;
constexpr int ROWS_BLOCK = 256;
constexpr uint32_t ROW_COLS_MAX = 40000;     // ints of a row that one workgroup sums in LDS (160 000 of the 163 840 bytes); longer rows are split into column blocks
constexpr int CELLS = 256;                   // cells of a row per workgroup of the write kernels, one per thread
constexpr int CELL_BYTES = 11;               // `\t%10d`, `\t%10.6f`, `\t%.8f`

__device__ __forceinline__ int64_t td_tri(int64_t hi) { return hi * (hi - 1) / 2; }

// a lane per entry: the k-mers that point to each list (entries equal to 1 are the empty slots of the direct-address form)
__global__ __launch_bounds__(256) void tdist_mult_kernel(const uint32_t *entries, int64_t n_entries, uint32_t *mult) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n_entries) return;
	const uint32_t pos = entries[i];
	if(pos != 1u) atomicAdd(&mult[pos], 1u);
}

// the inverted index, a wavefront per list: FILL = false counts the lists of every template, FILL = true writes their numbers behind
// the scanned starts (the order inside a template's run is whatever the atomics give; the sums do not depend on it)
template <class V, bool FILL>
__global__ __launch_bounds__(256) void tdist_inv_kernel(const V *values, const uint32_t *list_off, int64_t n_lists, uint32_t *cnt, const uint32_t *start, uint32_t *inv) {
	const int lane = threadIdx.x & (WAVE - 1);
	const int64_t waves = (int64_t) gridDim.x * (blockDim.x / WAVE);
	for(int64_t l = (int64_t) blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; l < n_lists; l += waves) {
		const V *v = values + list_off[l];
		const uint32_t len = v[0];
		for(uint32_t e = lane; e < len; e += WAVE) {
			const uint32_t t = (uint32_t) v[1 + e] - 1u;
			const uint32_t slot = atomicAdd(&cnt[t], 1u);
			if(FILL) inv[start[t] + slot] = (uint32_t) l;
		}
	}
}

// kmerSimilarity by rows: workgroup (hi, column block) sums D[hi][c0 .. c0 + w) in LDS over the lists that hold hi, a wavefront per
// list, and stores the piece of the row; the first column block also sums N[hi]. Every cell of the triangle is stored.
template <class V>
__global__ __launch_bounds__(ROWS_BLOCK) void tdist_rows_kernel(const V *values, const uint32_t *list_off, const uint32_t *mult, const uint32_t *start, const uint32_t *inv,
                                                               uint32_t n, uint32_t cols, int32_t *N, int32_t *D) {
	extern __shared__ __attribute__((aligned(16))) int td_row[];          // [cols] and one word for N[hi]
	const uint32_t hi = blockIdx.x;
	const uint32_t c0 = blockIdx.y * cols;
	if(blockIdx.y && c0 >= hi) return;          // (whole workgroups leave)
	const uint32_t w = c0 < hi ? min(hi - c0, cols) : 0u;
	for(uint32_t c = threadIdx.x; c < w; c += ROWS_BLOCK) td_row[c] = 0;
	if(threadIdx.x == 0) td_row[cols] = 0;
	__syncthreads();
	const int lane = threadIdx.x & (WAVE - 1);
	const uint32_t a = start[hi], b = start[hi + 1];
	for(uint32_t li = a + threadIdx.x / WAVE; li < b; li += ROWS_BLOCK / WAVE) {
		const uint32_t o = list_off[inv[li]];
		const int m = (int) mult[o];
		const V *v = values + o;
		const uint32_t len = v[0];
		for(uint32_t e = lane; e < len; e += WAVE) {
			const uint32_t t = (uint32_t) v[1 + e] - 1u;
			if(t < hi && t - c0 < w) atomicAdd(&td_row[t - c0], m);          // (t < c0 wraps beyond w)
		}
		if(blockIdx.y == 0 && lane == 0) atomicAdd(&td_row[cols], m);
	}
	__syncthreads();
	int32_t *row = D + td_tri(hi) + c0;
	for(uint32_t c = threadIdx.x; c < w; c += ROWS_BLOCK) row[c] = td_row[c];
	if(blockIdx.y == 0 && threadIdx.x == 0) N[hi] = td_row[cols];
}

// kmerSimilarity, the plain form: a wavefront per list, for every member the lanes over the members before it, a global atomic add
// per pair. The pair is (max, min) of the two ids: nothing rests on the order inside a list. N and D start as zeros.
template <class V>
__global__ __launch_bounds__(256) void tdist_pairs_kernel(const V *values, const uint32_t *list_off, const uint32_t *mult, int64_t n_lists, int32_t *N, int32_t *D) {
	const int lane = threadIdx.x & (WAVE - 1);
	const int64_t waves = (int64_t) gridDim.x * (blockDim.x / WAVE);
	for(int64_t l = (int64_t) blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; l < n_lists; l += waves) {
		const uint32_t o = list_off[l];
		const int m = (int) mult[o];
		const V *v = values + o;
		const uint32_t len = v[0];
		for(uint32_t e = lane; e < len; e += WAVE) atomicAdd(&N[(uint32_t) v[1 + e] - 1u], m);
		for(uint32_t i = 1; i < len; ++i) {
			const uint32_t x = (uint32_t) v[1 + i] - 1u;
			for(uint32_t j = lane; j < i; j += WAVE) {
				const uint32_t y = (uint32_t) v[1 + j] - 1u;
				if(x != y) atomicAdd(&D[td_tri((int64_t) max(x, y)) + min(x, y)], m);
			}
		}
	}
}

// ---- a cell's text ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void td_put_int(char *o, int d) {
	// `\t%10d` of d >= 0
	unsigned u = (unsigned) d;
	o[0] = '\t';
	for(int i = 10; i >= 1; --i) {
		o[i] = (u || i == 10) ? (char) ('0' + u % 10u) : ' ';
		u /= 10u;
	}
}

// `\t%10.6f` (P = 10^6, three places before the point) or `\t%.8f` (P = 10^8, one place) of 0 <= d <= 100: the exact decimal rounding
// of the binary double that glibc's printf gives. d = M * 2^-s; M * P in 128 bits, shifted down by s, round-half-even on what leaves.
__device__ __forceinline__ void td_put_f(char *o, double d, bool eight) {
	const unsigned long long bits = (unsigned long long) __double_as_longlong(d);
	const int e = (int) ((bits >> 52) & 0x7FFull);
	const unsigned long long f = bits & ((1ull << 52) - 1ull);
	const unsigned long long M = e ? (f | (1ull << 52)) : f;
	const int s = e ? 1075 - e : 1074;          // 46 and up for d < 128
	const unsigned long long P = eight ? 100000000ull : 1000000ull;
	const unsigned long long lo = M * P, hi = __umul64hi(M, P);
	unsigned long long q;
	bool half, sticky;
	if(s <= 0) { q = lo; half = sticky = false; }          // (an integer beyond 2^52: not a value of these measures)
	else if(s < 64) { q = (hi << (64 - s)) | (lo >> s); half = (lo >> (s - 1)) & 1ull; sticky = (lo & ((1ull << (s - 1)) - 1ull)) != 0; }
	else if(s == 64) { q = hi; half = lo >> 63; sticky = (lo & ~(1ull << 63)) != 0; }
	else if(s < 128) { q = hi >> (s - 64); half = (hi >> (s - 65)) & 1ull; sticky = lo != 0 || (hi & ((1ull << (s - 65)) - 1ull)) != 0; }
	else { q = 0; half = sticky = false; }                  // (M * P < 2^80: below a half)
	if(half && (sticky || (q & 1ull))) ++q;
	unsigned long long ip = q / P, fp = q % P;
	o[0] = '\t';
	if(eight) {
		o[1] = (char) ('0' + ip % 10ull); o[2] = '.';
		for(int i = 10; i >= 3; --i) { o[i] = (char) ('0' + fp % 10ull); fp /= 10ull; }
	} else {
		for(int i = 3; i >= 1; --i) { o[i] = (ip || i == 3) ? (char) ('0' + ip % 10ull) : ' '; ip /= 10ull; }
		o[4] = '.';
		for(int i = 10; i >= 5; --i) { o[i] = (char) ('0' + fp % 10ull); fp /= 10ull; }
	}
}

// kmerDist, kmerShared, chi2dist (dist.c:321-334) with the `(d < 0 ? 0 : d)` of printIntLtdPhy
__device__ __forceinline__ int td_int_value(int method, int Ni, int Nj, int D) {
	if(method == 2) return D < 0 ? 0 : D;
	const int d = Ni + Nj - (D << 1);
	if(method == 1) return d < 0 ? 0 : d;
	long long c = (long long) d;
	c = c * c / (long long) (Ni + Nj);
	return c < 0 ? 0 : (int) c;
}

// the ten double measures (dist.c:428-476), the reference's own expressions in IEEE double; sNi, sNj: sqrt(Ni), sqrt(Nj) from the host's libm
__device__ __forceinline__ double td_f_value(int method, int Ni, int Nj, int D, double sNi, double sNj) {
#pragma clang fp contract(off)
	double d;
	switch(method) {
		case 4: d = 100.0 * D / Ni; break;
		case 8: d = 100.0 * D / Nj; break;
		case 16: d = 200.0 * D / (Ni + Nj); break;
		case 32: d = 100.0 - 200.0 * D / (Ni + Nj); break;
		case 64: d = 1.0 - (double) (D) / (Ni + Nj - D); break;
		case 128: d = (double) (D) / (Ni + Nj - D); break;
		case 256: d = 1.0 - (double) (D) / (sNi * sNj); break;
		case 512: d = (double) (D) / (sNi * sNj); break;
		case 1024: d = (double) (D) / (Ni < Nj ? Ni : Nj); break;
		default: d = 1.0 - (double) (D) / (Ni < Nj ? Ni : Nj); break;          // 2048
	}
	const double top = method < 64 ? 100.0 : 1.0;
	return (d < 0) ? 0.0 : ((top < d) ? top : d);
}

struct WriteArgs {
	int method, full;                // full: the asymmetric n x n matrices (4, 8)
	uint32_t n, r0;                  // rows of the matrix; the row of workgroup x = 0
	const int32_t *N, *D;
	const double *sq;
	const int64_t *row_off;          // [n + 1] where row i's `\n` stands in the matrix's text; [n]: the closing `\n`
	const int64_t *name_off;         // [n + 1] into names
	const char *names;
	int64_t w0, w1;                  // the window of the text this launch writes; w0 is a multiple of 16
	char *out;                       // the byte at w0
};

// one cell per thread: workgroup (row, block of CELLS cells) formats its cells into LDS, placed so that LDS and text agree modulo
// 16, and copies what lies inside the window out in 16-byte vectors (bytes at the edges); block 0 of a row writes `\n` and the name
template <bool F>
__device__ __forceinline__ void td_write_body(const WriteArgs &A) {
	__shared__ __attribute__((aligned(16))) char stage[16 + CELLS * CELL_BYTES + 16];
	const uint32_t i = A.r0 + blockIdx.x;
	const uint32_t cells = A.full ? A.n : i;
	const uint32_t c0 = blockIdx.y * CELLS;
	if(blockIdx.y && c0 >= cells) return;          // (whole workgroups leave)
	const int64_t nlen = A.name_off[i + 1] - A.name_off[i];
	const int64_t row = A.row_off[i];
	if(blockIdx.y == 0) {
		const char *nm = A.names + A.name_off[i];
		for(int64_t p = threadIdx.x; p < 1 + nlen; p += blockDim.x) {
			const int64_t at = row + p;
			if(at >= A.w0 && at < A.w1) A.out[at - A.w0] = p ? nm[p - 1] : '\n';
		}
	}
	const uint32_t mine = c0 < cells ? min((uint32_t) CELLS, cells - c0) : 0u;
	if(!mine) return;
	const int64_t a = row + 1 + nlen + (int64_t) CELL_BYTES * c0, b = a + (int64_t) CELL_BYTES * mine;
	if(b <= A.w0 || a >= A.w1) return;
	const int pad = (int) (a & 15);
	if(threadIdx.x < mine) {
		const uint32_t j = c0 + threadIdx.x;
		char *o = stage + pad + CELL_BYTES * threadIdx.x;
		if(F && j == i) td_put_f(o, 100.0, false);          // (only the full matrices have a diagonal)
		else {
			const uint32_t hi = max(i, j), lo = min(i, j);
			const int d = A.D[td_tri((int64_t) hi) + lo], Ni = A.N[i], Nj = A.N[j];
			if(F) td_put_f(o, td_f_value(A.method, Ni, Nj, d, A.sq[i], A.sq[j]), A.method >= 64);
			else td_put_int(o, td_int_value(A.method, Ni, Nj, d));
		}
	}
	__syncthreads();
	const int64_t lo = max(a, A.w0), hi = min(b, A.w1);
	const int64_t v0 = min((lo + 15) & ~(int64_t) 15, hi), v1 = max(hi & ~(int64_t) 15, v0);
	for(int64_t p = lo + threadIdx.x; p < v0; p += blockDim.x) A.out[p - A.w0] = stage[p - a + pad];
	for(int64_t p = v0 + 16 * (int64_t) threadIdx.x; p < v1; p += 16 * (int64_t) blockDim.x)
		*(uint4 *) (A.out + (p - A.w0)) = *(const uint4 *) (stage + (p - a + pad));
	for(int64_t p = v1 + threadIdx.x; p < hi; p += blockDim.x) A.out[p - A.w0] = stage[p - a + pad];
}

__global__ __launch_bounds__(CELLS) void tdist_write_int_kernel(const WriteArgs A) { td_write_body<false>(A); }
__global__ __launch_bounds__(CELLS) void tdist_write_f_kernel(const WriteArgs A) { td_write_body<true>(A); }

// the test hook: n cells from explicit triples
__global__ __launch_bounds__(256) void tdist_cells_kernel(int method, const int32_t *Ni, const int32_t *Nj, const int32_t *D, const double *sNi, const double *sNj, int64_t n, char *out) {
	for(int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
		char o[CELL_BYTES];
		if(method == 1 || method == 2 || method == 4096) td_put_int(o, td_int_value(method, Ni[i], Nj[i], D[i]));
		else td_put_f(o, td_f_value(method, Ni[i], Nj[i], D[i], sNi[i], sNj[i]), method >= 64);
		for(int c = 0; c < CELL_BYTES; ++c) out[i * CELL_BYTES + c] = o[c];
	}
}

struct Timer {
	kmahip_tdist *s; int which; hipEvent_t a = nullptr, b = nullptr;
	Timer(kmahip_tdist *s_, int w) : s(s_), which(w) {
		if(s->timing && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void) hipEventRecord(a, 0);
	}
	~Timer() {
		if(a && b) {
			float ms = 0;
			if(hipEventRecord(b, 0) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) { s->ms[which] += ms; ++s->launches[which]; }
		}
		if(a) (void) hipEventDestroy(a);
		if(b) (void) hipEventDestroy(b);
	}
};

template <class T>
int td_room(kmahip_tdist *s, size_t count, T **dst) {
	void *d = nullptr;
	const size_t bytes = (count ? count : 1) * sizeof(T);
	if(hipMalloc(&d, bytes) != hipSuccess) { (void) hipGetLastError(); kmahip_set_error("%zu bytes of device memory for the template distances", bytes); return KMAHIP_ENOMEM; }
	s->allocs.push_back(d);
	s->info.total_bytes += bytes;
	*dst = (T *) d;
	return KMAHIP_OK;
}

const struct { int bit; const char *name; } METHODS[13] = {
	{1, "k-mer distance"}, {2, "shared k-mers"}, {4, "Query k-mer coverage [%]"}, {8, "Template k-mer coverage [%]"}, {16, "Avg. k-mer coverage [%]"},
	{32, "Inverse Avg. k-mer coverage"}, {64, "Jaccard Distance"}, {128, "Jaccard Similarity"}, {256, "Cosine distance"}, {512, "Cosine similarity"},
	{1024, "Szymkiewicz\xe2\x80\x93Simpson similarity"}, {2048, "Szymkiewicz\xe2\x80\x93Simpson dissimilarity"}, {4096, "Chi-square distance"}};

int wrong_format(const char *why) {
	// (the reference's words first: `Wrong format of DB.`)
	kmahip_set_error("Wrong format of DB. (%s)", why);
	return KMAHIP_EFORMAT;
}

// the object over entries (per-k-mer list offsets, 1 = none) and a value array: every list is checked to lie inside the array and to
// hold ids 1 .. DB_size - 1 (the kernels walk them unchecked), the distinct lists are numbered, everything goes to the device
int td_build(kmahip_tdist *s, const uint32_t *entries, uint64_t n_entries, uint64_t n_live, const void *values, int vb, uint64_t n_values) {
	const uint32_t DB_size = s->info.DB_size;
	std::vector<uint8_t> seen((size_t) n_values + 1, 0);
	std::vector<uint32_t> lists;
	uint64_t elems = 0;
	for(uint64_t i = 0; i < n_entries; ++i) {
		const uint64_t o = entries[i];
		if(o == 1) continue;
		if(o >= n_values) return wrong_format("a k-mer's value list begins past the value array");
		if(seen[(size_t) o]) continue;
		seen[(size_t) o] = 1;
		const uint64_t len = vb == 2 ? ((const uint16_t *) values)[o] : ((const uint32_t *) values)[o];
		if(o + len >= n_values) return wrong_format("a k-mer's value list runs past the value array");
		for(uint64_t e = 1; e <= len; ++e) {
			const uint32_t t = vb == 2 ? ((const uint16_t *) values)[o + e] : ((const uint32_t *) values)[o + e];
			if(t < 1 || t >= DB_size) return wrong_format("a value list holds a template that is not in the database");
		}
		lists.push_back((uint32_t) o);
		elems += len;
	}
	if(lists.size() > 0x7FFFFFFFull || elems > 0xFFFFFFFFull) { kmahip_set_error("%zu value lists of %llu members: beyond what the inverted index addresses", lists.size(), (unsigned long long) elems); return KMAHIP_EFORMAT; }
	s->n_entries = n_entries; s->n_elems = elems;
	s->info.n_kmers = n_live; s->info.n_lists = lists.size(); s->info.n_values = n_values; s->info.value_bytes = (uint32_t) vb;
	const uint64_t n = s->n, tri = n * (n ? n - 1 : 0) / 2;
	uint8_t *vals = nullptr;
	int rc;
	if((rc = td_room(s, (size_t) n_values * vb + 16, &vals)) || (rc = td_room(s, (size_t) n_entries, &s->entries)) || (rc = td_room(s, lists.size(), &s->list_off)) ||
	   (rc = td_room(s, (size_t) n_values, &s->mult)) || (rc = td_room(s, (size_t) n, &s->N)) || (rc = td_room(s, (size_t) tri, &s->D)) ||
	   (rc = td_room(s, (size_t) n + 1, &s->inv_cnt)) || (rc = td_room(s, (size_t) n + 1, &s->inv_cur)) || (rc = td_room(s, (size_t) elems, &s->inv)) || (rc = td_room(s, (size_t) n, &s->sq))) return rc;
	s->values = vals;
	if(n_values) HIP_TRY(hipMemcpy(vals, values, (size_t) n_values * vb, hipMemcpyHostToDevice));
	if(n_entries) HIP_TRY(hipMemcpy(s->entries, entries, (size_t) n_entries * 4, hipMemcpyHostToDevice));
	if(!lists.empty()) HIP_TRY(hipMemcpy(s->list_off, lists.data(), lists.size() * 4, hipMemcpyHostToDevice));
	return KMAHIP_OK;
}

bool read_all(FILE *f, void *dst, size_t bytes) { return !bytes || fread(dst, 1, bytes, f) == bytes; }

}  // namespace

extern "C" void kmahip_tdist_close(kmahip_tdist *s) {
	if(!s) return;
	for(void *p : s->allocs) (void) hipFree(p);
	delete s;
}

extern "C" int kmahip_tdist_open(const char *prefix, kmahip_tdist **out) {
	if(!prefix || !out) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	*out = nullptr;
	const std::string base(prefix);
	FILE *f = fopen((base + ".comp.b").c_str(), "rb");
	if(!f) { kmahip_set_error("cannot open %s.comp.b", prefix); return KMAHIP_EIO; }
	struct Closer { FILE *f; ~Closer() { if(f) fclose(f); } } closer{f};
	fseek(f, 0, SEEK_END);
	const uint64_t fsize = (uint64_t) std::max(0l, ftell(f));
	rewind(f);
	// loadValues (dist.c:48-56): DB_size, mlen, prefix_len; prefix, size, n, v_index, null_index
	uint32_t h32[3];
	uint64_t h64[5];
	if(!read_all(f, h32, 12) || !read_all(f, h64, 40)) return wrong_format("no header");
	const uint32_t DB_size = h32[0], mlen = h32[1];
	const uint64_t size = h64[1], n = h64[2], v_index = h64[3];
	const uint64_t mask = mlen >= 32 ? ~0ull : mlen ? (1ull << (2 * mlen)) - 1ull : 0ull;
	if(size < n) return wrong_format("size below n: an old index");
	if(DB_size < 1) return wrong_format("DB_size 0");
	if(v_index >= 0xFFFFFFFFull || n > 0xFFFFFFFFull) { kmahip_set_error("%s.comp.b: %llu values, %llu k-mers: offsets beyond 32 bits are not served", prefix, (unsigned long long) v_index, (unsigned long long) n); return KMAHIP_EFORMAT; }
	const bool mega = size - 1 == mask;
	const int vb = DB_size < 65535u ? 2 : 4;
	uint64_t pos = 52;
	// (every piece is held against the file's length before room is made for it)
	auto fits = [&](uint64_t count, uint64_t each) { return count <= (fsize - pos) / each; };
	std::vector<uint32_t> exist;
	if(mega) {
		if(!fits(size, 4)) return wrong_format("the file ends inside the direct-address array");
		exist.resize((size_t) size);
		if(!read_all(f, exist.data(), (size_t) size * 4)) return wrong_format("the file ends inside the direct-address array");
		pos += size * 4;
	} else {
		if(!fits(size, 4)) return wrong_format("the file ends inside the bucket array");
		pos += size * 4;
		if(fseek(f, (long) pos, SEEK_SET)) return wrong_format("the file ends inside the bucket array");
	}
	if(!fits(v_index, (uint64_t) vb)) return wrong_format("the file ends inside the values");
	std::vector<uint8_t> values((size_t) v_index * vb + 8, 0);
	if(!read_all(f, values.data(), (size_t) v_index * vb)) return wrong_format("the file ends inside the values");
	pos += v_index * vb;
	if(!mega) {
		const uint64_t kb = mlen <= 16 ? 4 : 8;
		if(!fits(n + 1, kb)) return wrong_format("the file ends inside the keys");
		pos += (n + 1) * kb;
		if(fseek(f, (long) pos, SEEK_SET)) return wrong_format("the file ends inside the keys");
		if(!fits(n, 4)) return wrong_format("the file ends inside the value indexes");
		exist.resize((size_t) n);
		if(!read_all(f, exist.data(), (size_t) n * 4)) return wrong_format("the file ends inside the value indexes");
		pos += n * 4;
	}
	uint32_t tail[2] = {mlen, 0};
	if(fread(&tail[0], 4, 1, f) == 1) { if(fread(&tail[1], 4, 1, f) != 1) return wrong_format("a k-mer size without its flag"); }
	else tail[0] = mlen;
	// kmerSimilarity (:186-221): entries equal to 1 are passed over, the walk ends behind the n-th live one
	uint64_t live = 0, n_entries = 0;
	while(live < n && n_entries < exist.size()) live += exist[(size_t) n_entries++] != 1u;
	if(live < n) return wrong_format("fewer k-mers than the header counts");

	kmahip_tdist *s = new kmahip_tdist();
	s->info.DB_size = DB_size; s->info.mlen = mlen; s->info.kmersize = tail[0]; s->info.flag = tail[1]; s->info.prefix_len = h32[2]; s->info.direct = mega;
	s->n = DB_size - 1;
	{
		// nameLoad (runkma.c:107-128): a name ends at its newline; past the end of the file a name is empty
		FILE *g = fopen((base + ".name").c_str(), "rb");
		if(!g) { delete s; kmahip_set_error("cannot open %s.name", prefix); return KMAHIP_EIO; }
		s->names.assign(s->n, std::string());
		uint32_t t = 0;
		int c;
		while(t < s->n && (c = fgetc(g)) != EOF) { if(c == '\n') ++t; else s->names[t].push_back((char) c); }
		s->info.name_bytes = 0;
		fseek(g, 0, SEEK_END);
		s->info.name_bytes = (uint64_t) std::max(0l, ftell(g));
		fclose(g);
	}
	const int rc = td_build(s, exist.data(), n_entries, n, values.data(), vb, v_index);
	if(rc) { kmahip_tdist_close(s); return rc; }
	*out = s;
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_open_lists(uint32_t n_templates, uint64_t n_kmers, const uint32_t *offsets, const void *values, int value_bytes, uint64_t n_values, kmahip_tdist **out) {
	if(!out || (n_kmers && !offsets) || (n_values && !values) || (value_bytes != 2 && value_bytes != 4)) { kmahip_set_error("kmahip_tdist_open_lists: bad argument"); return KMAHIP_EINVAL; }
	*out = nullptr;
	if(n_templates >= 0xFFFFFFFEu || n_values >= 0xFFFFFFFFull || n_kmers > 0xFFFFFFFFull) { kmahip_set_error("kmahip_tdist_open_lists: sizes beyond 32 bits"); return KMAHIP_EINVAL; }
	if(value_bytes == 2 && n_templates + 1 >= 65535u) { kmahip_set_error("kmahip_tdist_open_lists: %u templates do not fit 16-bit values", n_templates); return KMAHIP_EINVAL; }
	kmahip_tdist *s = new kmahip_tdist();
	s->info.DB_size = n_templates + 1;
	s->n = n_templates;
	uint64_t live = 0;
	for(uint64_t i = 0; i < n_kmers; ++i) live += offsets[i] != 1u;
	s->names.resize(n_templates);
	for(uint32_t t = 0; t < n_templates; ++t) s->names[t] = std::to_string(t + 1);          // (no name file: a template is named by its id)
	for(const std::string &nm : s->names) s->info.name_bytes += nm.size() + 1;
	const int rc = td_build(s, offsets, n_kmers, live, values, value_bytes, n_values);
	if(rc) { kmahip_tdist_close(s); return rc; }
	*out = s;
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_get_info(const kmahip_tdist *s, kmahip_tdist_info *info) {
	if(!s || !info) return KMAHIP_EINVAL;
	*info = s->info;
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_name(const kmahip_tdist *s, uint32_t t, const char **name) {
	if(!s || !name || t >= s->n) { kmahip_set_error("template %u out of range", t); return KMAHIP_EINVAL; }
	*name = s->names[t].c_str();
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_count(kmahip_tdist *s) {
	if(!s) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	// KMAHIP_TDIST_FORM: "rows" (the default) or "pairs"; KMAHIP_TDIST_COLS: the ints of a row a workgroup
	// sums, for the test of the column blocks
	const char *form = getenv("KMAHIP_TDIST_FORM");
	const bool pairs = form && !strcmp(form, "pairs");
	if(form && !pairs && strcmp(form, "rows")) { kmahip_set_error("KMAHIP_TDIST_FORM=%s: rows or pairs", form); return KMAHIP_EINVAL; }
	const uint32_t n = s->n;
	const int64_t n_lists = (int64_t) s->info.n_lists;
	const uint64_t tri = (uint64_t) n * (n ? n - 1 : 0) / 2;
	const bool v16 = s->info.value_bytes == 2;
	const uint16_t *v2 = (const uint16_t *) s->values;
	const uint32_t *v4 = (const uint32_t *) s->values;
	s->counted = false; s->sq_there = false;
	HIP_TRY(hipMemsetAsync(s->mult, 0, std::max<size_t>(1, (size_t) s->info.n_values) * 4, 0));
	if(s->n_entries) {
		Timer tm(s, 0);
		hipLaunchKernelGGL(tdist_mult_kernel, dim3((unsigned) ((s->n_entries + 255) / 256)), dim3(256), 0, 0, s->entries, (int64_t) s->n_entries, s->mult);
	}
	HIP_TRY(hipGetLastError());
	const unsigned list_blocks = (unsigned) std::max<int64_t>(1, std::min<int64_t>(2048, (n_lists + 3) / 4));
	if(pairs) {
		HIP_TRY(hipMemsetAsync(s->N, 0, std::max<size_t>(1, n) * 4, 0));
		HIP_TRY(hipMemsetAsync(s->D, 0, std::max<size_t>(1, (size_t) tri) * 4, 0));
		if(n_lists) {
			Timer tm(s, 3);
			if(v16) hipLaunchKernelGGL(tdist_pairs_kernel<uint16_t>, dim3(list_blocks), dim3(256), 0, 0, v2, s->list_off, s->mult, n_lists, s->N, s->D);
			else hipLaunchKernelGGL(tdist_pairs_kernel<uint32_t>, dim3(list_blocks), dim3(256), 0, 0, v4, s->list_off, s->mult, n_lists, s->N, s->D);
		}
		HIP_TRY(hipGetLastError());
	} else if(n) {
		// the inverted index: count, scan (the host: DB_size words), fill
		std::vector<uint32_t> start((size_t) n + 1, 0);
		{
			Timer tm(s, 1);
			HIP_TRY(hipMemsetAsync(s->inv_cur, 0, ((size_t) n + 1) * 4, 0));
			if(n_lists) {
				if(v16) hipLaunchKernelGGL((tdist_inv_kernel<uint16_t, false>), dim3(list_blocks), dim3(256), 0, 0, v2, s->list_off, n_lists, s->inv_cur, (const uint32_t *) nullptr, (uint32_t *) nullptr);
				else hipLaunchKernelGGL((tdist_inv_kernel<uint32_t, false>), dim3(list_blocks), dim3(256), 0, 0, v4, s->list_off, n_lists, s->inv_cur, (const uint32_t *) nullptr, (uint32_t *) nullptr);
			}
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpy(start.data() + 1, s->inv_cur, (size_t) n * 4, hipMemcpyDeviceToHost));
			for(uint32_t t = 0; t < n; ++t) start[t + 1] += start[t];
			if(start[n] != s->n_elems) { kmahip_set_error("the inverted index counts %u members, the lists hold %llu", start[n], (unsigned long long) s->n_elems); return KMAHIP_EDEVICE; }
			HIP_TRY(hipMemcpy(s->inv_cnt, start.data(), ((size_t) n + 1) * 4, hipMemcpyHostToDevice));
			HIP_TRY(hipMemsetAsync(s->inv_cur, 0, ((size_t) n + 1) * 4, 0));
			if(n_lists) {
				if(v16) hipLaunchKernelGGL((tdist_inv_kernel<uint16_t, true>), dim3(list_blocks), dim3(256), 0, 0, v2, s->list_off, n_lists, s->inv_cur, s->inv_cnt, s->inv);
				else hipLaunchKernelGGL((tdist_inv_kernel<uint32_t, true>), dim3(list_blocks), dim3(256), 0, 0, v4, s->list_off, n_lists, s->inv_cur, s->inv_cnt, s->inv);
			}
			HIP_TRY(hipGetLastError());
		}
		uint32_t cols = std::min<uint32_t>(ROW_COLS_MAX, std::max<uint32_t>(1, n - 1));
		if(const char *e = getenv("KMAHIP_TDIST_COLS")) { const long c = atol(e); if(c >= 1 && (uint32_t) c < cols) cols = (uint32_t) c; }
		const size_t shm = ((size_t) cols + 4) * 4;
		const unsigned gy = (unsigned) ((std::max<uint32_t>(1, n - 1) + cols - 1) / cols);
		if(gy > 65535u) { kmahip_set_error("KMAHIP_TDIST_COLS=%u: more than 65535 column blocks", cols); return KMAHIP_EINVAL; }
		if(shm > 65536) {
			// (beyond 64 KiB the dynamic LDS of a kernel has to be asked for)
			if(v16) HIP_TRY(hipFuncSetAttribute((const void *) tdist_rows_kernel<uint16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) shm));
			else HIP_TRY(hipFuncSetAttribute((const void *) tdist_rows_kernel<uint32_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) shm));
		}
		{
			Timer tm(s, 2);
			if(v16) hipLaunchKernelGGL(tdist_rows_kernel<uint16_t>, dim3(n, gy), dim3(ROWS_BLOCK), shm, 0, v2, s->list_off, s->mult, s->inv_cnt, s->inv, n, cols, s->N, s->D);
			else hipLaunchKernelGGL(tdist_rows_kernel<uint32_t>, dim3(n, gy), dim3(ROWS_BLOCK), shm, 0, v4, s->list_off, s->mult, s->inv_cnt, s->inv, n, cols, s->N, s->D);
		}
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipDeviceSynchronize());
	s->h_N.assign(n, 0);
	if(n) HIP_TRY(hipMemcpy(s->h_N.data(), s->N, (size_t) n * 4, hipMemcpyDeviceToHost));
	s->info.form = pairs ? 1 : 0;
	s->counted = true;
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_get_counts(kmahip_tdist *s, int32_t *N, int32_t *D, uint32_t row_lo, uint32_t row_hi) {
	if(!s) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(!s->counted) { kmahip_set_error("kmahip_tdist_get_counts before kmahip_tdist_count"); return KMAHIP_EINVAL; }
	if(row_lo > row_hi || row_hi > s->n) { kmahip_set_error("rows %u .. %u of %u", row_lo, row_hi, s->n); return KMAHIP_EINVAL; }
	if(N && s->n) memcpy(N, s->h_N.data(), (size_t) s->n * 4);
	const uint64_t a = (uint64_t) row_lo * (row_lo ? row_lo - 1 : 0) / 2, b = (uint64_t) row_hi * (row_hi ? row_hi - 1 : 0) / 2;
	if(D && b > a) HIP_TRY(hipMemcpy(D, s->D + a, (size_t) (b - a) * 4, hipMemcpyDeviceToHost));
	return KMAHIP_OK;
}

// where a requested measure would divide by zero (the reference prints -nan there, and its chi-square dies of an integer division)
static int td_refuse_zero(const kmahip_tdist *s, int methods) {
	const uint32_t n = s->n;
	if(n < 2) return KMAHIP_OK;          // (no cell off the diagonal)
	int64_t first = -1, second = -1;
	for(uint32_t t = 0; t < n && second < 0; ++t) if(s->h_N[t] == 0) { if(first < 0) first = t; else second = t; }
	const int one = methods & (4 | 8 | 256 | 512 | 1024 | 2048), two = methods & (16 | 32 | 64 | 128 | 4096);          // (Ni + Nj, and the Jaccard pair's Ni + Nj - D, are 0 between two such templates)
	if(one && first >= 0) {
		kmahip_set_error("distance method %d divides by zero: template %lld (%s) holds no k-mer", one & -one, (long long) first + 1, s->names[(size_t) first].c_str());
		return KMAHIP_EINVAL;
	}
	if(two && second >= 0) {
		kmahip_set_error("distance method %d divides by zero: templates %lld (%s) and %lld (%s) hold no k-mer", two & -two, (long long) first + 1, s->names[(size_t) first].c_str(),
		                 (long long) second + 1, s->names[(size_t) second].c_str());
		return KMAHIP_EINVAL;
	}
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_write(kmahip_tdist *s, const char *path, int methods, int format) {
	if(!s || !path) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(!s->counted) { kmahip_set_error("kmahip_tdist_write before kmahip_tdist_count"); return KMAHIP_EINVAL; }
	int rc = td_refuse_zero(s, methods);
	if(rc) return rc;
	const uint32_t n = s->n;
	if((methods & (256 | 512)) && !s->sq_there && n) {
		// the cosine pair: sqrt(N[t]) as the host's libm gives it
		std::vector<double> sq(n);
		for(uint32_t t = 0; t < n; ++t) sq[t] = sqrt((double) s->h_N[t]);
		HIP_TRY(hipMemcpy(s->sq, sq.data(), (size_t) n * 8, hipMemcpyHostToDevice));
		s->sq_there = true;
	}
	// the names as the rows carry them: as they are (format & 1), else `%-10.10s`
	std::vector<int64_t> name_off((size_t) n + 1, 0);
	std::string blob;
	for(uint32_t t = 0; t < n; ++t) {
		std::string nm = s->names[t];
		if(!(format & 1)) { nm.resize(std::min<size_t>(nm.size(), 10)); nm.append(10 - nm.size(), ' '); }
		blob += nm;
		name_off[t + 1] = (int64_t) blob.size();
	}
	long long chunk = 0;
	if(const char *e = getenv("KMAHIP_TDIST_CHUNK")) chunk = atoll(e);
	if(chunk <= 0) chunk = 64ll << 20;
	chunk = std::max(256ll, (chunk + 15) & ~15ll);
	int64_t *d_row = nullptr, *d_name = nullptr;
	char *d_blob = nullptr, *d_out = nullptr;
	struct Rooms { std::vector<void *> v; ~Rooms() { for(void *p : v) (void) hipFree(p); } } rooms;
	auto room = [&](size_t bytes, void **dst) { if(hipMalloc(dst, std::max<size_t>(16, bytes)) != hipSuccess) { (void) hipGetLastError(); return false; } rooms.v.push_back(*dst); return true; };
	if(!room(((size_t) n + 1) * 8, (void **) &d_row) || !room(((size_t) n + 1) * 8, (void **) &d_name) || !room(blob.size(), (void **) &d_blob)) { kmahip_set_error("no device memory for the rows of the distance file"); return KMAHIP_ENOMEM; }
	HIP_TRY(hipMemcpy(d_name, name_off.data(), ((size_t) n + 1) * 8, hipMemcpyHostToDevice));
	if(!blob.empty()) HIP_TRY(hipMemcpy(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
	FILE *f = fopen(path, "wb");
	if(!f) { kmahip_set_error("cannot write %s", path); return KMAHIP_EIO; }
	struct Closer { FILE *f; ~Closer() { if(f) fclose(f); } } closer{f};
	std::vector<char> host;
	size_t out_room = 0;
	std::vector<int64_t> row_off((size_t) n + 1);
	for(const auto &M : METHODS) {
		if(!(methods & M.bit)) continue;
		const bool full = M.bit == 4 || M.bit == 8, dbl = !(M.bit == 1 || M.bit == 2 || M.bit == 4096);
		char head[64];
		int hl = 0;
		if(format & 4) hl += snprintf(head, sizeof head, "# %-35s\n", M.name);
		hl += snprintf(head + hl, sizeof head - (size_t) hl, "%10d", (int) n);
		// the row offsets: a prefix sum over the name lengths and the cells
		int64_t at = hl;
		for(uint32_t i = 0; i < n; ++i) { row_off[i] = at; at += 1 + (name_off[i + 1] - name_off[i]) + (int64_t) CELL_BYTES * (full ? n : i); }
		row_off[n] = at;
		const int64_t len = at + 1;
		HIP_TRY(hipMemcpy(d_row, row_off.data(), ((size_t) n + 1) * 8, hipMemcpyHostToDevice));
		for(int64_t w0 = 0; w0 < len; w0 += chunk) {
			const int64_t w1 = std::min<int64_t>(len, w0 + chunk);
			const size_t bytes = (size_t) (w1 - w0);
			if(out_room < bytes + 16) {
				if(!room(bytes + 16, (void **) &d_out)) { kmahip_set_error("no device memory for %zu bytes of distance text (KMAHIP_TDIST_CHUNK)", bytes); return KMAHIP_ENOMEM; }
				out_room = bytes + 16;
				host.resize(bytes);
			}
			// the rows that meet the window
			const int64_t *ro = row_off.data();
			const uint32_t r0 = (uint32_t) (std::max<int64_t>(1, std::upper_bound(ro, ro + n, w0) - ro) - 1);
			const uint32_t r1 = (uint32_t) (std::lower_bound(ro, ro + n, w1) - ro);          // one behind the last
			if(n && r1 > r0) {
				WriteArgs A;
				A.method = M.bit; A.full = full; A.n = n; A.r0 = r0; A.N = s->N; A.D = s->D; A.sq = s->sq; A.row_off = d_row; A.name_off = d_name; A.names = d_blob;
				A.w0 = w0; A.w1 = w1; A.out = d_out;
				const uint32_t most = full ? n : r1 - 1;
				const unsigned gy = std::max(1u, (most + CELLS - 1) / CELLS);
				if(gy > 65535u) { kmahip_set_error("rows of %u cells: beyond the write kernel's grid", most); return KMAHIP_EINVAL; }
				Timer tm(s, 4);
				if(dbl) hipLaunchKernelGGL(tdist_write_f_kernel, dim3(r1 - r0, gy), dim3(CELLS), 0, 0, A);
				else hipLaunchKernelGGL(tdist_write_int_kernel, dim3(r1 - r0, gy), dim3(CELLS), 0, 0, A);
			}
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpy(host.data(), d_out, bytes, hipMemcpyDeviceToHost));
			// the head of the matrix and its closing newline are the host's
			for(int64_t p = std::max<int64_t>(w0, 0); p < std::min<int64_t>(w1, hl); ++p) host[(size_t) (p - w0)] = head[p];
			if(row_off[n] >= w0 && row_off[n] < w1) host[(size_t) (row_off[n] - w0)] = '\n';
			if(fwrite(host.data(), 1, bytes, f) != bytes) { kmahip_set_error("writing %s failed", path); return KMAHIP_EIO; }
		}
		// getPhySize reserves DB_size * 11 name bytes with strict names and DB_size - 1 names are written: 11 bytes stay as the file was made
		if(!(format & 1)) { const char nul[CELL_BYTES] = {0}; if(fwrite(nul, 1, sizeof nul, f) != sizeof nul) { kmahip_set_error("writing %s failed", path); return KMAHIP_EIO; } }
	}
	const bool bad = ferror(f) != 0;
	closer.f = nullptr;
	if(fclose(f) || bad) { kmahip_set_error("writing %s failed", path); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

extern "C" int kmahip_test_tdist_cells(int method, const int32_t *Ni, const int32_t *Nj, const int32_t *D, int64_t n, char *out) {
	bool known = false;
	for(const auto &M : METHODS) known = known || M.bit == method;
	if(!known || n < 0 || (n && (!Ni || !Nj || !D || !out))) { kmahip_set_error("kmahip_test_tdist_cells: bad argument"); return KMAHIP_EINVAL; }
	if(!n) return KMAHIP_OK;
	std::vector<double> sq((size_t) 2 * n);
	for(int64_t i = 0; i < n; ++i) { sq[(size_t) i] = sqrt((double) Ni[i]); sq[(size_t) (n + i)] = sqrt((double) Nj[i]); }
	char *d = nullptr;
	const size_t ints = (size_t) n * 12, dbl = (size_t) n * 16;
	if(hipMalloc((void **) &d, dbl + ints + (size_t) n * CELL_BYTES) != hipSuccess) { (void) hipGetLastError(); kmahip_set_error("kmahip_test_tdist_cells: %lld cells do not fit", (long long) n); return KMAHIP_ENOMEM; }
	double *dq = (double *) d;
	int32_t *di = (int32_t *) (d + dbl);
	char *dout = d + dbl + ints;
	hipError_t e = hipMemcpy(dq, sq.data(), dbl, hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(di, Ni, (size_t) n * 4, hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(di + n, Nj, (size_t) n * 4, hipMemcpyHostToDevice);
	if(e == hipSuccess) e = hipMemcpy(di + 2 * n, D, (size_t) n * 4, hipMemcpyHostToDevice);
	if(e == hipSuccess) {
		const unsigned grid = (unsigned) std::min<int64_t>(4096, (n + 255) / 256);
		hipLaunchKernelGGL(tdist_cells_kernel, dim3(grid), dim3(256), 0, 0, method, di, di + n, di + 2 * n, dq, dq + n, n, dout);
		e = hipGetLastError();
	}
	if(e == hipSuccess) e = hipMemcpy(out, dout, (size_t) n * CELL_BYTES, hipMemcpyDeviceToHost);
	(void) hipFree(d);
	if(e != hipSuccess) { kmahip_set_error("kmahip_test_tdist_cells: %s", hipGetErrorString(e)); return KMAHIP_EDEVICE; }
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_set_timing(kmahip_tdist *s, int on) {
	if(!s) return KMAHIP_EINVAL;
	s->timing = on != 0;
	return KMAHIP_OK;
}

extern "C" int kmahip_tdist_get_timing(kmahip_tdist *s, int kernel, double *total_ms, int64_t *launches) {
	if(!s || kernel < 0 || kernel >= KMAHIP_TDIST_KERNELS) return KMAHIP_EINVAL;
	if(total_ms) *total_ms = s->ms[kernel];
	if(launches) *launches = s->launches[kernel];
	s->ms[kernel] = 0; s->launches[kernel] = 0;
	return KMAHIP_OK;
}
