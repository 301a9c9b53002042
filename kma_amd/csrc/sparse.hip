// sparse.hip -- sparse mapping (`kma -Sparse`, sparse.c:338-797) on the device: the loader of sparse indexes, the k-mer counting kernel
// (translateToKmersAndDump + save_kmers_sparse), collect_Kmers and withDraw_Kmers as kernels, and the choice of the templates as the
// reference's host arithmetic (save_kmers_sparse_batch without decontamination, :645-790). A pipeline of its own beside the mapping one.
#include "kmahip_internal.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

struct kmahip_sparse {
	kmahip_sparse_info info{};
	std::vector<void *> allocs;
	std::vector<uint32_t> h_keys, h_len, h_ulen;
	std::vector<char> names;              // <prefix>.name, newlines turned into NULs
	std::vector<const char *> name_of;    // [DB_size]; template 0 has none
	// device
	uint2 *slots = nullptr;               // (k-mer, id), KMAHIP_EMPTY_VI in .y for a free slot
	uint32_t nb_log2 = 0;
	uint32_t *voff = nullptr;             // [n] offset of id's value list
	const uint16_t *values16 = nullptr;
	const uint32_t *values32 = nullptr;
	uint32_t *counts = nullptr;           // [n]
	uint8_t *live = nullptr;              // [n] 1: in the reference's kmerList
	unsigned long long *ntot = nullptr;   // NTOT_SLOTS partial sums, a 128-byte line each: [0] Ntot, [1] probes that hit (the no-add variant's sink)
	uint32_t *scores = nullptr, *w_scores = nullptr;                  // [DB_size]
	unsigned long long *scores_tot = nullptr, *w_scores_tot = nullptr; // [DB_size]
	unsigned long long *hits = nullptr, *w_hits = nullptr;             // n, tot
	bool collected = false;
	int noadd = 0, timing = 0;
	double ms[3] = {0, 0, 0};
	int64_t launches[3] = {0, 0, 0};
	// staging of host batches
	void *stage[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	size_t stage_bytes[5] = {0, 0, 0, 0, 0};
};

namespace {

constexpr int WAVE = 64;
constexpr int COUNT_BLOCK = 256;          // four wavefronts, a read each
constexpr int NTOT_SLOTS = 256;           // partial sums of Ntot, NTOT_STRIDE words apart: a workgroup adds to the slot of its index
constexpr int NTOT_STRIDE = 16;
constexpr int COLLECT_BLOCKS = 512;       // workgroups of the collect kernel, each with its own copy of the score vectors in LDS
constexpr uint32_t LDS_SCORE_MAX = 4096;  // templates (DB_size) whose two vectors fit 48 KiB of LDS: 4 + 8 bytes each

__global__ __launch_bounds__(256) void sp_fill_kernel(unsigned long long *slots, int64_t n_slots) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n_slots) slots[i] = (unsigned long long) KMAHIP_EMPTY_VI << 32;
}

// a lane per k-mer: the first free slot at or behind its home bucket, taken with a 64-bit compare-and-swap (the scheme of db.hip with
// the k-mer's id where the mapping index keeps a position)
__global__ __launch_bounds__(256) void sp_insert_kernel(const uint32_t *keys, int64_t n, unsigned long long *slots, uint32_t nb_log2) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const uint32_t key = keys[i], nbm = (1u << nb_log2) - 1u;
	const unsigned long long empty = (unsigned long long) KMAHIP_EMPTY_VI << 32, mine = ((unsigned long long) (uint32_t) i << 32) | key;
	uint32_t b = (key * 0x9E3779B1u) >> (32u - nb_log2);
	for(;;) {
		unsigned long long *s = slots + (size_t) b * KMAHIP_BUCKET_SLOTS;
		for(int j = 0; j < KMAHIP_BUCKET_SLOTS; ++j) if(atomicCAS(&s[j], empty, mine) == empty) return;
		b = (b + 1u) & nbm;
	}
}

__device__ __forceinline__ bool sp_find(const uint2 *slots, uint32_t nb_log2, uint32_t km, uint32_t *id) {
	const uint32_t nbm = (1u << nb_log2) - 1u;
	uint32_t b = (km * 0x9E3779B1u) >> (32u - nb_log2);
	for(;;) {
		const uint4 *sl = (const uint4 *) (slots + (size_t) b * KMAHIP_BUCKET_SLOTS);
		const uint4 lo = sl[0], hi = sl[1];          // the bucket: 32 bytes
		if(lo.y == KMAHIP_EMPTY_VI) return false;
		if(lo.x == km) { *id = lo.y; return true; }
		if(lo.w == KMAHIP_EMPTY_VI) return false;
		if(lo.z == km) { *id = lo.w; return true; }
		if(hi.y == KMAHIP_EMPTY_VI) return false;
		if(hi.x == km) { *id = hi.y; return true; }
		if(hi.w == KMAHIP_EMPTY_VI) return false;
		if(hi.z == km) { *id = hi.w; return true; }
		b = (b + 1u) & nbm;
	}
}

// bases [pos, pos + len) of a packed read (32 per word from the top bits down), right-aligned; 1 <= len <= 32. Reads word + 1: every
// read is followed by a pad word
__device__ __forceinline__ uint64_t sp_mer(const uint64_t *w, int pos, int len) {
	const int ip = (pos & 31) << 1;
	uint64_t x = w[pos >> 5] << ip;
	if(ip) x |= w[(pos >> 5) + 1] >> (64 - ip);
	return x >> (64 - 2 * len);
}

// the reverse complement of a right-aligned len-mer
__device__ __forceinline__ uint64_t sp_revcomp(uint64_t x, int len) {
	x = ~x;
	x = __brevll(x);                                                           // bits reversed: the bases too, each with its two bits swapped
	x = ((x & 0x5555555555555555ull) << 1) | ((x >> 1) & 0x5555555555555555ull);
	return x >> (64 - 2 * len);
}

// bases [pos, pos + len) of strand rc of the read
__device__ __forceinline__ uint64_t sp_strand_mer(const uint64_t *w, int L, int rc, int pos, int len) {
	if(!rc) return sp_mer(w, pos, len);
	return sp_revcomp(sp_mer(w, L - pos - len, len), len);
}

// translateToKmersAndDump (sparse.c:50-131, flag == 0) and save_kmers_sparse (:232-244). A wavefront per read walks both strands: the
// stretches between N's are found by every lane alike (a read holds few N's), the positions of a stretch are spread over the lanes.
// ADD = false: the timing-only variant, the probes stay and the adds go.
template <bool ADD>
__global__ __launch_bounds__(COUNT_BLOCK) void sparse_count_kernel(const uint64_t *seq, const int64_t *seq_off, const int32_t *len, const int32_t *N, const int64_t *N_off,
                                                                   int64_t n_reads, const uint2 *slots, uint32_t nb_log2, int k, int p, uint64_t prefix,
                                                                   uint32_t *counts, unsigned long long *ntot) {
	const int lane = threadIdx.x & (WAVE - 1);
	const int64_t r = (int64_t) blockIdx.x * (COUNT_BLOCK / WAVE) + (threadIdx.x / WAVE);
	if(r >= n_reads) return;          // (whole wavefronts leave)
	const uint64_t *w = seq + seq_off[r];
	const int L = len[r];
	const int32_t *Nr = N + N_off[r];
	const int nN = (int) (N_off[r + 1] - N_off[r]);
	unsigned produced = 0, found = 0;
	for(int rc = 0; rc < 2; ++rc) {
		int i = 0, nx = 0;          // nx: N's (in this strand's order) that lie before i
		while(i < L) {
			// charpos(qseq, 4, i, seqlen): the first N at or behind i
			int end = L;
			while(nx < nN) {
				const int q = rc ? L - 1 - Nr[nN - 1 - nx] : Nr[nx];
				if(q >= i) { end = q; break; }
				++nx;
			}
			int first, last, next;          // starts of the windows of this stretch: [first, last)
			if(p) {
				if(i < end - k - p) { first = i; last = end - k - p + 1; next = end + 1; }
				else { first = last = 0; next = end + k + 1; }
			} else {
				first = i; last = end - k + 1; next = end + k + 1;      // (`end` is never reduced there: the walk resumes k + 1 bases behind the N)
			}
			for(int s = first + lane; s < last; s += WAVE) {
				if(p && sp_strand_mer(w, L, rc, s, p) != prefix) continue;
				const uint32_t km = (uint32_t) sp_strand_mer(w, L, rc, s + p, k);
				++produced;
				uint32_t id;
				if(sp_find(slots, nb_log2, km, &id)) {
					if(ADD) atomicAdd(&counts[id], 1u);          // (result unused: a plain global atomic add)
					else ++found;
				}
			}
			i = next;
		}
	}
	// Ntot: one add per wavefront, spread over NTOT_SLOTS lines (every wavefront adding to ONE address is what bounded this kernel:
	// 12.1 ms per 1 M reads whatever else it did, 24.0 ms with a second such counter)
	for(int o = WAVE / 2; o > 0; o >>= 1) { produced += __shfl_down(produced, o, WAVE); found += __shfl_down(found, o, WAVE); }
	if(lane == 0) {
		unsigned long long *mine = ntot + (size_t) (blockIdx.x & (NTOT_SLOTS - 1)) * NTOT_STRIDE;
		if(produced) atomicAdd(&mine[0], (unsigned long long) produced);
		if(!ADD && found) atomicAdd(&mine[1], (unsigned long long) found);
	}
}

template <class V>
__device__ __forceinline__ void sp_collect_body(const V *values, const uint32_t *voff, const uint32_t *counts, uint8_t *live, int64_t n, uint32_t DB_size, bool lds,
                                                uint32_t *l_sc, unsigned long long *l_tot, uint32_t *scores, unsigned long long *scores_tot, unsigned long long *hits) {
	unsigned long long hn = 0, ht = 0;
	for(int64_t id = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (int64_t) gridDim.x * blockDim.x) {
		const uint32_t c = counts[id];
		live[id] = c != 0;
		if(!c) continue;
		++hn; ht += (unsigned long long) (long long) (int) c;          // (node->value is an int, hashmapkmers.h:26)
		const V *v = values + voff[id];
		const uint32_t m = v[0];
		for(uint32_t j = 1; j <= m; ++j) {
			const uint32_t t = v[j];
			if(t >= DB_size) continue;
			if(lds) { atomicAdd(&l_sc[t], 1u); atomicAdd(&l_tot[t], (unsigned long long) (long long) (int) c); }
			else { atomicAdd(&scores[t], 1u); atomicAdd(&scores_tot[t], (unsigned long long) (long long) (int) c); }
		}
	}
	for(int o = WAVE / 2; o > 0; o >>= 1) { hn += __shfl_down(hn, o, WAVE); ht += __shfl_down(ht, o, WAVE); }
	if((threadIdx.x & (WAVE - 1)) == 0 && hn) { atomicAdd(&hits[0], hn); atomicAdd(&hits[1], ht); }
}

// collect_Kmers (hashtable.c:54-120): a lane per k-mer id. The scores are a few thousand hot addresses: each workgroup sums into its
// own copy in LDS and folds what is not zero into the global vectors at its end (lds), or, for a database whose vectors do not fit,
// adds to the global vectors directly.
template <class V>
__global__ __launch_bounds__(256) void sparse_collect_kernel(const V *values, const uint32_t *voff, const uint32_t *counts, uint8_t *live, int64_t n, uint32_t DB_size,
                                                             int lds, uint32_t *scores, unsigned long long *scores_tot, unsigned long long *hits) {
	extern __shared__ unsigned long long sp_lds[];
	unsigned long long *l_tot = sp_lds;
	uint32_t *l_sc = (uint32_t *) (sp_lds + (lds ? DB_size : 0));
	if(lds) {
		for(uint32_t t = threadIdx.x; t < DB_size; t += blockDim.x) { l_tot[t] = 0; l_sc[t] = 0; }
		__syncthreads();
	}
	sp_collect_body<V>(values, voff, counts, live, n, DB_size, lds != 0, l_sc, l_tot, scores, scores_tot, hits);
	if(lds) {
		__syncthreads();
		for(uint32_t t = threadIdx.x; t < DB_size; t += blockDim.x) if(l_sc[t]) { atomicAdd(&scores[t], l_sc[t]); atomicAdd(&scores_tot[t], l_tot[t]); }
	}
}

// intpos_bin (hashtable.c:27-52) as it stands: str1[0] is the list's length, and the last probe may land on it
template <class V>
__device__ __forceinline__ int sp_intpos_bin(const V *str1, int str2) {
	int upLim = (int) str1[0];
	if(upLim == 0) return -1;
	int downLim = 1;
	int pos = (upLim + downLim) >> 1;
	while(0 < (upLim - downLim)) {
		const int at = (int) str1[pos];
		if(at == str2) return pos;
		else if(at < str2) downLim = pos + 1;
		else upLim = pos - 1;
		pos = (upLim + downLim) >> 1;
	}
	if((int) str1[pos] == str2) return pos;
	return -1;
}

// withDraw_Kmers (hashtable.c:224-270): a plain pass over the live k-mers
template <class V>
__global__ __launch_bounds__(256) void sparse_withdraw_kernel(const V *values, const uint32_t *voff, const uint32_t *counts, uint8_t *live, int64_t n, uint32_t DB_size,
                                                              int tmpl, uint32_t *w_scores, unsigned long long *w_scores_tot, unsigned long long *w_hits) {
	unsigned long long hn = 0, ht = 0;
	const int64_t id = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(id < n && live[id]) {
		const V *v = values + voff[id];
		if(sp_intpos_bin<V>(v, tmpl) != -1) {
			const unsigned long long c = (unsigned long long) (long long) (int) counts[id];
			const uint32_t m = v[0];
			for(uint32_t j = 1; j <= m; ++j) {
				const uint32_t t = v[j];
				if(t >= DB_size) continue;
				atomicSub(&w_scores[t], 1u);
				atomicAdd(&w_scores_tot[t], 0ull - c);
			}
			live[id] = 0;
			hn = 1; ht = c;
		}
	}
	for(int o = WAVE / 2; o > 0; o >>= 1) { hn += __shfl_down(hn, o, WAVE); ht += __shfl_down(ht, o, WAVE); }
	if((threadIdx.x & (WAVE - 1)) == 0 && hn) { atomicAdd(&w_hits[0], 0ull - hn); atomicAdd(&w_hits[1], 0ull - ht); }
}

struct Timer {
	kmahip_sparse *s; int which; hipEvent_t a = nullptr, b = nullptr;
	Timer(kmahip_sparse *s_, int w) : s(s_), which(w) {
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
int sp_room(kmahip_sparse *s, size_t count, T **dst) {
	void *d = nullptr;
	const size_t bytes = (count ? count : 1) * sizeof(T);
	HIP_TRY(hipMalloc(&d, bytes));
	s->allocs.push_back(d);
	s->info.total_bytes += bytes;
	*dst = (T *) d;
	return KMAHIP_OK;
}

bool read_all(FILE *f, void *dst, size_t bytes) { return fread(dst, 1, bytes, f) == bytes; }

}  // namespace

extern "C" void kmahip_sparse_close(kmahip_sparse *s) {
	if(!s) return;
	for(void *p : s->allocs) (void) hipFree(p);
	for(void *p : s->stage) if(p) (void) hipFree(p);
	delete s;
}

extern "C" int kmahip_sparse_open(const char *prefix, kmahip_sparse **out) {
	if(!prefix || !out) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	*out = nullptr;
	const std::string base(prefix);
	KmaComp c;
	int rc = kmahip_comp_read(base + ".comp.b", true, &c);          // (refuses k > 16 and flag != 0 by name)
	if(rc) return rc;
	// what `kma index` without -Sparse writes: prefix_len 0 and prefix 0 (`-Sparse -` sets prefix 1, index.c)
	if(c.prefix_len == 0 && c.prefix == 0) { kmahip_set_error("%s.comp.b is not a sparse index (prefix length 0, prefix 0): DB needs to sparse indexed, to run a sparse mapping.", prefix); return KMAHIP_EFORMAT; }
	if(c.prefix_len > 32) { kmahip_set_error("prefix length %u", c.prefix_len); return KMAHIP_EFORMAT; }
	const uint32_t DB_size = c.DB_size, k = c.tail[0];
	const uint64_t n = c.n;

	// load_DBs_Sparse (sparse.c:133-177): the count, a first array that is skipped, the lengths, the unique lengths
	std::vector<uint32_t> h_len(DB_size), h_ulen(DB_size);
	{
		FILE *f = fopen((base + ".length.b").c_str(), "rb");
		if(!f) { kmahip_set_error("cannot open %s.length.b", prefix); return KMAHIP_EIO; }
		int32_t cnt = 0;
		if(!read_all(f, &cnt, 4) || (uint32_t) cnt != DB_size) { fclose(f); kmahip_set_error("bad %s.length.b", prefix); return KMAHIP_EIO; }
		size_t got = 0;
		if(fseek(f, (long) DB_size * 4, SEEK_CUR) == 0) {
			got = fread(h_len.data(), 4, DB_size, f);
			got += fread(h_ulen.data(), 4, DB_size, f);
		}
		fclose(f);
		if(got != (size_t) 2 * DB_size) { kmahip_set_error("%s.length.b holds no unique lengths: DB needs to sparse indexed, to run a sparse mapping.", prefix); return KMAHIP_EFORMAT; }
	}
	kmahip_sparse *s = new kmahip_sparse();
	s->h_len.swap(h_len); s->h_ulen.swap(h_ulen);
	{
		FILE *f = fopen((base + ".name").c_str(), "rb");
		if(!f) { delete s; kmahip_set_error("cannot open %s.name", prefix); return KMAHIP_EIO; }
		fseek(f, 0, SEEK_END);
		const long sz = ftell(f);
		rewind(f);
		s->names.assign((size_t) std::max(0l, sz) + 1, 0);
		if(sz > 0 && !read_all(f, s->names.data(), (size_t) sz)) { fclose(f); delete s; kmahip_set_error("cannot read %s.name", prefix); return KMAHIP_EIO; }
		fclose(f);
		// (template_names[0][file_size - 1] = 0; names[1] = the start, names[j] behind the (j - 1)-th newline, sparse.c:214-224)
		if(sz > 0) s->names[(size_t) sz - 1] = 0;
		s->name_of.assign(DB_size, "");
		uint32_t j = 2;
		if(DB_size > 1) s->name_of[1] = s->names.data();
		for(long i = 0; i < sz && j < DB_size; ++i) if(s->names[(size_t) i] == '\n') { s->names[(size_t) i] = 0; s->name_of[j++] = s->names.data() + i + 1; }
	}
	s->info.DB_size = DB_size; s->info.kmersize = k; s->info.prefix_len = c.prefix_len; s->info.prefix = c.prefix; s->info.values_u16 = c.u16;
	s->info.n_kmers = n; s->info.n_hdr = c.n_hdr; s->info.n_values = c.v_index;
	s->h_keys.assign(c.keys.begin(), c.keys.begin() + (size_t) n);

	// every list must lie inside the value array: the kernels walk them unchecked
	for(uint64_t i = 0; i < n; ++i) {
		const uint64_t o = c.vidx[i];
		uint64_t m = 0;
		bool ok = o < c.v_index;
		if(ok) { m = c.u16 ? ((const uint16_t *) c.values.data())[o] : ((const uint32_t *) c.values.data())[o]; ok = o + m < c.v_index + 1 && o + m >= o; }
		if(!ok) { delete s; kmahip_set_error("%s.comp.b: value list of k-mer %llu runs past the value array", prefix, (unsigned long long) i); return KMAHIP_EFORMAT; }
	}

	uint32_t nb_log2 = 4;
	while(((uint64_t) KMAHIP_BUCKET_SLOTS << nb_log2) < 2 * n) ++nb_log2;          // >= 2n slots, as the mapping index
	if(nb_log2 > 31) { delete s; kmahip_set_error("index too large"); return KMAHIP_EFORMAT; }
	s->nb_log2 = nb_log2;
	const size_t n_slots = ((size_t) 1 << nb_log2) * KMAHIP_BUCKET_SLOTS;
	uint32_t *d_keys = nullptr;
	uint8_t *vals = nullptr;
	const size_t vbytes = ((size_t) c.v_index + 8) * (c.u16 ? 2 : 4);
	if((rc = sp_room(s, n_slots, &s->slots)) || (rc = sp_room(s, (size_t) n, &s->voff)) || (rc = sp_room(s, (size_t) n, &s->counts)) || (rc = sp_room(s, (size_t) n, &s->live)) ||
	   (rc = sp_room(s, vbytes, &vals)) || (rc = sp_room(s, (size_t) NTOT_SLOTS * NTOT_STRIDE, &s->ntot)) || (rc = sp_room(s, DB_size, &s->scores)) || (rc = sp_room(s, DB_size, &s->w_scores)) ||
	   (rc = sp_room(s, DB_size, &s->scores_tot)) || (rc = sp_room(s, DB_size, &s->w_scores_tot)) || (rc = sp_room(s, 2, &s->hits)) || (rc = sp_room(s, 2, &s->w_hits))) {
		kmahip_sparse_close(s); return rc;
	}
	if(c.u16) s->values16 = (const uint16_t *) vals; else s->values32 = (const uint32_t *) vals;
	bool bad = hipMalloc((void **) &d_keys, ((size_t) n + 1) * 4) != hipSuccess;
	bad = bad || hipMemcpy(d_keys, c.keys.data(), (size_t) n * 4, hipMemcpyHostToDevice) != hipSuccess ||
	      hipMemcpy(s->voff, c.vidx.data(), (size_t) n * 4, hipMemcpyHostToDevice) != hipSuccess ||
	      hipMemcpy(vals, c.values.data(), std::min(vbytes, c.values.size()), hipMemcpyHostToDevice) != hipSuccess ||
	      hipMemset(s->counts, 0, std::max<size_t>(1, (size_t) n) * 4) != hipSuccess || hipMemset(s->live, 0, std::max<size_t>(1, (size_t) n)) != hipSuccess ||
	      hipMemset(s->ntot, 0, (size_t) NTOT_SLOTS * NTOT_STRIDE * 8) != hipSuccess;
	if(!bad) {
		hipLaunchKernelGGL(sp_fill_kernel, dim3((unsigned) ((n_slots + 255) / 256)), dim3(256), 0, 0, (unsigned long long *) s->slots, (int64_t) n_slots);
		if(n) hipLaunchKernelGGL(sp_insert_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, d_keys, (int64_t) n, (unsigned long long *) s->slots, nb_log2);
		bad = hipDeviceSynchronize() != hipSuccess;
	}
	if(d_keys) (void) hipFree(d_keys);
	if(bad) { kmahip_set_error("building the sparse probe table failed: %s", hipGetErrorString(hipGetLastError())); kmahip_sparse_close(s); return KMAHIP_EDEVICE; }
	*out = s;
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_get_info(const kmahip_sparse *s, kmahip_sparse_info *info) {
	if(!s || !info) return KMAHIP_EINVAL;
	*info = s->info;
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_template(const kmahip_sparse *s, int32_t t, const char **name, uint32_t *len, uint32_t *ulen) {
	if(!s || t < 0 || (uint32_t) t >= s->info.DB_size) { kmahip_set_error("template %d out of range", (int) t); return KMAHIP_EINVAL; }
	if(name) *name = s->name_of[(size_t) t];
	if(len) *len = s->h_len[(size_t) t];
	if(ulen) *ulen = s->h_ulen[(size_t) t];
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_count_dev(kmahip_sparse *s, const kmahip_reads *r) {
	if(!s || !r) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	s->collected = false;
	if(r->n_reads <= 0) return KMAHIP_OK;
	const int per = COUNT_BLOCK / WAVE;
	const int64_t blocks = (r->n_reads + per - 1) / per;
	if(blocks > 0x7FFFFFFFll) { kmahip_set_error("batch of %lld reads too large", (long long) r->n_reads); return KMAHIP_EINVAL; }
	{
		Timer tm(s, 0);
		if(s->noadd) hipLaunchKernelGGL(sparse_count_kernel<false>, dim3((unsigned) blocks), dim3(COUNT_BLOCK), 0, 0, r->seq, r->seq_off, r->len, r->N, r->N_off, r->n_reads,
		                                s->slots, s->nb_log2, (int) s->info.kmersize, (int) s->info.prefix_len, s->info.prefix, s->counts, s->ntot);
		else hipLaunchKernelGGL(sparse_count_kernel<true>, dim3((unsigned) blocks), dim3(COUNT_BLOCK), 0, 0, r->seq, r->seq_off, r->len, r->N, r->N_off, r->n_reads,
		                        s->slots, s->nb_log2, (int) s->info.kmersize, (int) s->info.prefix_len, s->info.prefix, s->counts, s->ntot);
	}
	HIP_TRY(hipGetLastError());
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_count(kmahip_sparse *s, const kmahip_reads *r) {
	if(!s || !r) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(r->n_reads <= 0) return KMAHIP_OK;
	const int64_t n = r->n_reads;
	const void *src[5] = {r->seq, r->seq_off, r->len, r->N, r->N_off};
	const size_t bytes[5] = {(size_t) r->seq_words * 8, (size_t) (n + 1) * 8, (size_t) n * 4, (size_t) std::max<int64_t>(1, r->N_total) * 4, (size_t) (n + 1) * 8};
	for(int a = 0; a < 5; ++a) {
		if(s->stage_bytes[a] < bytes[a] + 16) {
			if(s->stage[a]) (void) hipFree(s->stage[a]);
			s->stage[a] = nullptr; s->stage_bytes[a] = 0;
			HIP_TRY(hipMalloc(&s->stage[a], bytes[a] + 16));
			s->stage_bytes[a] = bytes[a] + 16;
		}
		if(a == 3 && r->N_total == 0) { HIP_TRY(hipMemset(s->stage[a], 0, 4)); continue; }
		HIP_TRY(hipMemcpy(s->stage[a], src[a], bytes[a], hipMemcpyHostToDevice));
	}
	// (the kernel reads the word behind a k-mer's first word: the words past the batch's last are staged as zero)
	HIP_TRY(hipMemset((char *) s->stage[0] + bytes[0], 0, 16));
	kmahip_reads d = *r;
	d.seq = (const uint64_t *) s->stage[0]; d.seq_off = (const int64_t *) s->stage[1]; d.len = (const int32_t *) s->stage[2];
	d.N = (const int32_t *) s->stage[3]; d.N_off = (const int64_t *) s->stage[4];
	const int rc = kmahip_sparse_count_dev(s, &d);
	if(rc) return rc;
	HIP_TRY(hipDeviceSynchronize());
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_counts(kmahip_sparse *s, uint32_t *keys, uint32_t *counts, uint64_t *Ntot) {
	if(!s) return KMAHIP_EINVAL;
	const size_t n = (size_t) s->info.n_kmers;
	if(keys && n) memcpy(keys, s->h_keys.data(), n * 4);
	if(counts && n) HIP_TRY(hipMemcpy(counts, s->counts, n * 4, hipMemcpyDeviceToHost));
	if(Ntot) {
		std::vector<unsigned long long> part((size_t) NTOT_SLOTS * NTOT_STRIDE);
		HIP_TRY(hipMemcpy(part.data(), s->ntot, part.size() * 8, hipMemcpyDeviceToHost));
		unsigned long long v = 0;
		for(int i = 0; i < NTOT_SLOTS; ++i) v += part[(size_t) i * NTOT_STRIDE];
		*Ntot = v;
	}
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_collect(kmahip_sparse *s) {
	if(!s) return KMAHIP_EINVAL;
	const uint32_t D = s->info.DB_size;
	const int64_t n = (int64_t) s->info.n_kmers;
	HIP_TRY(hipMemsetAsync(s->scores, 0, (size_t) D * 4, 0));
	HIP_TRY(hipMemsetAsync(s->scores_tot, 0, (size_t) D * 8, 0));
	HIP_TRY(hipMemsetAsync(s->hits, 0, 16, 0));
	if(n) {
		// KMAHIP_SPARSE_NO_LDS: the path of a database too large for the LDS copies, for the test that compares both
		const int lds = D <= LDS_SCORE_MAX && !getenv("KMAHIP_SPARSE_NO_LDS");
		const unsigned blocks = (unsigned) std::min<int64_t>(COLLECT_BLOCKS, (n + 255) / 256);
		const size_t shm = lds ? (size_t) D * 12 : 0;
		Timer tm(s, 1);
		if(s->values16) hipLaunchKernelGGL(sparse_collect_kernel<uint16_t>, dim3(blocks), dim3(256), shm, 0, s->values16, s->voff, s->counts, s->live, n, D, lds, s->scores, s->scores_tot, s->hits);
		else hipLaunchKernelGGL(sparse_collect_kernel<uint32_t>, dim3(blocks), dim3(256), shm, 0, s->values32, s->voff, s->counts, s->live, n, D, lds, s->scores, s->scores_tot, s->hits);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(s->w_scores, s->scores, (size_t) D * 4, hipMemcpyDeviceToDevice, 0));
	HIP_TRY(hipMemcpyAsync(s->w_scores_tot, s->scores_tot, (size_t) D * 8, hipMemcpyDeviceToDevice, 0));
	HIP_TRY(hipMemcpyAsync(s->w_hits, s->hits, 16, hipMemcpyDeviceToDevice, 0));
	HIP_TRY(hipDeviceSynchronize());
	s->collected = true;
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_withdraw(kmahip_sparse *s, int32_t t) {
	if(!s) return KMAHIP_EINVAL;
	if(!s->collected) { kmahip_set_error("kmahip_sparse_withdraw before kmahip_sparse_collect"); return KMAHIP_EINVAL; }
	if(t < 0 || (uint32_t) t >= s->info.DB_size) { kmahip_set_error("template %d out of range", (int) t); return KMAHIP_EINVAL; }
	const int64_t n = (int64_t) s->info.n_kmers;
	if(!n) return KMAHIP_OK;
	const unsigned blocks = (unsigned) ((n + 255) / 256);
	{
		Timer tm(s, 2);
		if(s->values16) hipLaunchKernelGGL(sparse_withdraw_kernel<uint16_t>, dim3(blocks), dim3(256), 0, 0, s->values16, s->voff, s->counts, s->live, n, s->info.DB_size, (int) t, s->w_scores, s->w_scores_tot, s->w_hits);
		else hipLaunchKernelGGL(sparse_withdraw_kernel<uint32_t>, dim3(blocks), dim3(256), 0, 0, s->values32, s->voff, s->counts, s->live, n, s->info.DB_size, (int) t, s->w_scores, s->w_scores_tot, s->w_hits);
	}
	HIP_TRY(hipGetLastError());
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_scores(kmahip_sparse *s, int which, uint32_t *scores, uint64_t *scores_tot, uint64_t hits[2]) {
	if(!s) return KMAHIP_EINVAL;
	if(!s->collected) { kmahip_set_error("kmahip_sparse_scores before kmahip_sparse_collect"); return KMAHIP_EINVAL; }
	const size_t D = s->info.DB_size;
	if(scores) HIP_TRY(hipMemcpy(scores, which ? s->w_scores : s->scores, D * 4, hipMemcpyDeviceToHost));
	if(scores_tot) HIP_TRY(hipMemcpy(scores_tot, which ? s->w_scores_tot : s->scores_tot, D * 8, hipMemcpyDeviceToHost));
	if(hits) HIP_TRY(hipMemcpy(hits, which ? s->w_hits : s->hits, 16, hipMemcpyDeviceToHost));
	return KMAHIP_OK;
}

extern "C" void kmahip_sparse_default_opts(kmahip_sparse_opts *o) {
	if(!o) return;
	o->ID_t = 1.0; o->Depth_t = 0.0; o->evalue = 0.05; o->ss = 'q'; o->pad_ = 0;      // kma.c:319-325
}

// save_kmers_sparse_batch, the branch without decontamination (sparse.c:645-790)
static int sparse_rows(kmahip_sparse *s, const kmahip_sparse_opts *opts, std::vector<kmahip_sparse_row> &rows) {
	int rc = kmahip_sparse_collect(s);
	if(rc) return rc;
	const int DB_size = (int) s->info.DB_size;
	const double ID_t = opts->ID_t, Depth_t = opts->Depth_t, evalue = opts->evalue;
	const char ss = (char) opts->ss;
	std::vector<uint32_t> Scores((size_t) DB_size), w_Scores((size_t) DB_size), SearchList((size_t) DB_size);
	std::vector<uint64_t> Scores_tot((size_t) DB_size), w_Scores_tot((size_t) DB_size);
	uint64_t Nhits[2], w_Nhits[2], Ntot = 0;
	if((rc = kmahip_sparse_scores(s, 0, Scores.data(), Scores_tot.data(), Nhits)) || (rc = kmahip_sparse_counts(s, nullptr, nullptr, &Ntot))) return rc;
	w_Scores = Scores; w_Scores_tot = Scores_tot;
	for(int i = 0; i < DB_size; ++i) SearchList[(size_t) i] = Scores[(size_t) i] != 0;
	const unsigned *template_lengths = s->h_len.data(), *template_ulengths = s->h_ulen.data();
	const long unsigned templates_n = s->info.n_hdr;
	const double etta = 1.0e-6;
	double expected = 0, q_value = 0, p_value = 0;
	int stop = Nhits[0] == 0;          // (kmerList == 0)
	while(!stop) {
		double depth = 0, cover = 0;
		long unsigned score = 0;
		int tmpl = 0;
		for(int i = 0; i < DB_size; ++i) {
			if(!SearchList[(size_t) i]) continue;
			if(ss == 'q' && !(w_Scores_tot[(size_t) i] >= score)) continue;
			const double tmp_cover = 100.0 * w_Scores[(size_t) i] / template_ulengths[i];
			const long unsigned tmp_score = w_Scores_tot[(size_t) i];
			const double tmp_depth = 1.0 * tmp_score / template_lengths[i];
			if(ID_t <= tmp_cover && Depth_t <= tmp_depth) {
				bool better;
				if(ss == 'q') better = tmp_score > score || (tmp_cover > cover || (tmp_cover == cover && (tmp_depth > depth || (tmp_depth == depth && template_ulengths[i] > template_ulengths[tmpl]))));
				else if(ss == 'd') better = tmp_depth > depth || (tmp_depth == depth && (tmp_cover > cover || (tmp_cover == cover && (tmp_score > score || (tmp_score == score && template_ulengths[i] > template_ulengths[tmpl])))));
				else better = tmp_cover > cover || (tmp_cover == cover && (tmp_depth > depth || (tmp_depth == depth && (tmp_score > score || (tmp_score == score && template_ulengths[i] > template_ulengths[tmpl])))));
				if(better) {
					const double tmp_expected = 1.0 * (Nhits[1] - w_Scores_tot[(size_t) i]) * template_ulengths[i] / (templates_n - template_ulengths[i] + etta);
					const double tmp_q = (tmp_score - tmp_expected) * (tmp_score - tmp_expected) / (tmp_score + tmp_expected);
					const double tmp_p = kmahip_p_chisqr(tmp_q);
					if(tmp_p <= evalue && tmp_score > tmp_expected) {
						score = tmp_score; cover = tmp_cover; depth = tmp_depth; tmpl = i;
						expected = tmp_expected; p_value = tmp_p; q_value = tmp_q;
					} else SearchList[(size_t) i] = 0;
				}
			} else SearchList[(size_t) i] = 0;
		}
		if(cover && ID_t <= cover && Depth_t <= depth) {
			kmahip_sparse_row row;
			memset(&row, 0, sizeof row);
			row.tmpl = tmpl; row.expected = (int) expected; row.score = score; row.ulen = template_ulengths[tmpl];
			row.query_cover = 100.0 * w_Scores_tot[(size_t) tmpl] / Ntot;
			row.cover = cover; row.depth = depth;
			row.tot_cover = 100.0 * Scores[(size_t) tmpl] / template_ulengths[tmpl];
			row.tot_depth = 1.0 * Scores_tot[(size_t) tmpl] / template_lengths[tmpl];
			row.tot_query_cover = 100.0 * Scores_tot[(size_t) tmpl] / Ntot;
			row.q_value = q_value; row.p_value = p_value;
			rows.push_back(row);
			if((rc = kmahip_sparse_withdraw(s, tmpl)) || (rc = kmahip_sparse_scores(s, 1, w_Scores.data(), w_Scores_tot.data(), w_Nhits))) return rc;
			SearchList[(size_t) tmpl] = 0;
			if(w_Nhits[0] == 0) stop = 1;          // (kmerList == 0)
		} else stop = 1;
	}
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_rows(kmahip_sparse *s, const kmahip_sparse_opts *opts, kmahip_sparse_row *rows, int64_t cap, int64_t *n_rows) {
	if(!s || !opts || !n_rows || (cap > 0 && !rows)) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(opts->ss != 'q' && opts->ss != 'c' && opts->ss != 'd') { kmahip_set_error("ss must be 'q', 'c' or 'd'"); return KMAHIP_EINVAL; }
	std::vector<kmahip_sparse_row> v;
	const int rc = sparse_rows(s, opts, v);
	if(rc) return rc;
	*n_rows = (int64_t) v.size();
	if((int64_t) v.size() > cap) { kmahip_set_error("%lld rows, room for %lld", (long long) v.size(), (long long) cap); return KMAHIP_EOVERFLOW; }
	if(!v.empty()) memcpy(rows, v.data(), v.size() * sizeof(kmahip_sparse_row));
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_write(kmahip_sparse *s, const kmahip_sparse_opts *opts, const char *path) {
	if(!s || !opts || !path) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(opts->ss != 'q' && opts->ss != 'c' && opts->ss != 'd') { kmahip_set_error("ss must be 'q', 'c' or 'd'"); return KMAHIP_EINVAL; }
	std::vector<kmahip_sparse_row> v;
	const int rc = sparse_rows(s, opts, v);
	if(rc) return rc;
	FILE *f = fopen(path, "w");
	if(!f) { kmahip_set_error("cannot write %s", path); return KMAHIP_EIO; }
	fprintf(f, "#Template\tNum\tScore\tExpected\tTemplate_length\tQuery_Coverage\tTemplate_Coverage\tDepth\ttot_query_Coverage\ttot_template_Coverage\ttot_depth\tq_value\tp_value\n");
	for(const kmahip_sparse_row &r : v)
		fprintf(f, "%s\t%d\t%lu\t%d\t%d\t%8.2f\t%8.2f\t%8.2f\t%8.2f\t%8.2f\t%8.2f\t%8.2f\t%4.1e\n", s->name_of[(size_t) r.tmpl], r.tmpl, (long unsigned) r.score, r.expected,
		        (int) r.ulen, r.query_cover, r.cover, r.depth, r.tot_query_cover, r.tot_cover, r.tot_depth, r.q_value, r.p_value);
	const bool bad = ferror(f) != 0;
	if(fclose(f) || bad) { kmahip_set_error("writing %s failed", path); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_set_timing(kmahip_sparse *s, int on) {
	if(!s) return KMAHIP_EINVAL;
	s->timing = on != 0;
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_get_timing(kmahip_sparse *s, int kernel, double *total_ms, int64_t *launches) {
	if(!s || kernel < 0 || kernel > 2) return KMAHIP_EINVAL;
	if(total_ms) *total_ms = s->ms[kernel];
	if(launches) *launches = s->launches[kernel];
	s->ms[kernel] = 0; s->launches[kernel] = 0;
	return KMAHIP_OK;
}

extern "C" int kmahip_sparse_set_noadd(kmahip_sparse *s, int on) {
	if(!s) return KMAHIP_EINVAL;
	s->noadd = on != 0;
	return KMAHIP_OK;
}
