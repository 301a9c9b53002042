// index.hip -- `kma index -i templates.fsa -o prefix [-k k]`: the four files the mapping path reads.
// What the reference does in index.c / makeindex.c:167-330 (makeDB: FileBuffgetFsa, compDNAref, lengthCheck, update_DB,
// updateAnnots) and compress.c:83-614 (compressKMA_DB: bucket directory, key / value-index arrays, value lists de-duplicated by
// valuesHash) restated around a device sort: every k-mer start of every template becomes a 64-bit key (k-mer << 32 | template),
// the keys are radix-sorted and made unique on the GPU, and what is left is one linear pass on the host (group by k-mer, share
// equal template lists, cut into buckets). The files hold the same k-mer -> template-list mapping as the reference's and load into
// it; bucket count, key order inside a bucket and the order of the shared lists are the builder's own (the reference's follow
// from the growth history of its in-memory hash table and carry no meaning for a reader).
// Covered: the default hashed form, k <= 16, no minimizers / homopolymer compression, no -batch.
// -Sparse (kmahip_index_build_sparse; index.c:451-474 / 576-613, updateindex.c:79-199, qualcheck.c:31-79): index_build_sparse below,
// with its host side in index_host.h. The plain build's kernel, host pass and files are as they were. With -hq / -ht
// (kmahip_index_build_sparse_hom; qualcheck.c:81-324) the templates too similar to those kept before go as well: the pairs are
// counted in homology.hip between the windows and the renumbering.
// -deCon (kmahip_index_build_decon; index.c:676-729, decon.c:77-227): every k-mer of either strand of the contamination records
// becomes a key of the pseudo-template DB_size and joins the same sort; the host pass runs twice over the sorted pairs, once
// without those keys (<prefix>.comp.b, as ever) and once with them (<prefix>.decon.comp.b), where a k-mer that only the
// contamination holds is dropped: decontamination marks k-mers of the database, it adds none.
// -t_db (kmahip_index_append; index.c:529-557, 616-674, loadupdate.c:64-210): the old .comp.b is expanded back into pairs on the
// device (index_expand_count_kernel, a scan, index_expand_pairs_kernel), the new templates' keys are made by the kernels of the fresh
// builds under ids from the old DB_size on, and everything joins one sort; the host pass and the writers are those of a fresh build.
#include "kmahip_internal.h"
#include <zlib.h>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

#include "index_host.h"          // Tmpl, RefTable (index.c:128-170), and the host side of the sparse build

namespace {

// one thread per base of the concatenated templates: the k-mer that starts there, if it lies inside one template and holds no N
__global__ __launch_bounds__(256) void index_kmers_kernel(const uint8_t *codes, const int64_t *t_off, int n_t, int64_t total, int k,
                                                            unsigned long long *keys) {
	const int64_t p = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(p >= total) return;
	int lo = 0, hi = n_t;                      // template holding p: last t with t_off[t] <= p
	while(hi - lo > 1) { const int mid = (lo + hi) >> 1; if(t_off[mid] <= p) lo = mid; else hi = mid; }
	unsigned long long key = ~0ull;
	if(p + k <= t_off[lo + 1]) {
		unsigned long long km = 0;
		bool ok = true;
		for(int i = 0; i < k; ++i) { const uint8_t c = codes[p + i]; ok = ok && c < 4; km = (km << 2) | (c & 3); }
		if(ok) key = (km << 32) | (unsigned long long) (lo + 1);
	}
	keys[p] = key;
}

// one thread per base of the concatenated contamination records: the k-mer that starts there and its reverse complement, both as keys
// of the pseudo-template `id` (deConNode on the record and on its comp_rc, decon.c:199-205); keys[2 p], keys[2 p + 1]
__global__ __launch_bounds__(256) void index_decon_kmers_kernel(const uint8_t *codes, const int64_t *r_off, int n_r, int64_t total, int k, uint32_t id,
                                                                  unsigned long long *keys) {
	const int64_t p = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(p >= total) return;
	int lo = 0, hi = n_r;                      // record holding p: last r with r_off[r] <= p
	while(hi - lo > 1) { const int mid = (lo + hi) >> 1; if(r_off[mid] <= p) lo = mid; else hi = mid; }
	unsigned long long fw = ~0ull, rc = ~0ull;
	if(p + k <= r_off[lo + 1]) {
		unsigned long long km = 0, rk = 0;
		bool ok = true;
		for(int i = 0; i < k; ++i) {
			const uint8_t c = codes[p + i];
			ok = ok && c < 4;
			km = (km << 2) | (c & 3);
			rk |= (unsigned long long) (3 - (c & 3)) << (2 * i);
		}
		if(ok) { fw = (km << 32) | id; rc = (rk << 32) | id; }
	}
	keys[2 * p] = fw;
	keys[2 * p + 1] = rc;
}

// -Sparse (updateDBs_sparse, updateindex.c:79-167). One thread per base p of the concatenated templates reads the prefix_len + k bases
// that start there, once, for both strands: when they lie inside one template and hold no N they are a window of the forward strand
// if their first prefix_len bases equal the prefix (its k-mer: the last k bases), and a window of the reverse strand if the reverse
// complement of their last prefix_len bases does (its k-mer: the reverse complement of the first k). keys[2 p], keys[2 p + 1]:
// k-mer << 32 | template in file order, 1 .. n_t, or ~0. slen[t] gains the template's windows: where a wavefront lies inside one
// template -- all but the few that hold a boundary -- it adds once, the population count of two ballots
__global__ __launch_bounds__(256) void index_sparse_keys_kernel(const uint8_t *codes, const int64_t *t_off, int n_t, int64_t total, int k, int prefix_len,
                                                                  unsigned long long prefix, unsigned long long *keys, unsigned *slen) {
	const int64_t p = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = p < total;
	int lo = 0;
	unsigned long long fw = ~0ull, rc = ~0ull;
	if(live) {
		int hi = n_t;                            // template holding p: last t with t_off[t] <= p
		while(hi - lo > 1) { const int mid = (lo + hi) >> 1; if(t_off[mid] <= p) lo = mid; else hi = mid; }
		const int w = prefix_len + k;            // <= 32 bases: one 64-bit word a strand
		if(p + w <= t_off[lo + 1]) {
			unsigned long long x = 0, y = 0;
			bool ok = true;
			for(int i = 0; i < w; ++i) {
				const uint8_t c = codes[p + i];
				ok = ok && c < 4;
				x = (x << 2) | (c & 3);
				y |= (unsigned long long) (3 - (c & 3)) << (2 * i);
			}
			if(ok) {
				const unsigned long long kmask = (1ull << (2 * k)) - 1, id = (unsigned long long) (lo + 1);
				if(prefix_len == 0 || (x >> (2 * k)) == prefix) fw = ((x & kmask) << 32) | id;
				if(prefix_len == 0 || (y >> (2 * k)) == prefix) rc = ((y & kmask) << 32) | id;
			}
		}
		keys[2 * p] = fw;
		keys[2 * p + 1] = rc;
	}
	// (no thread has left: lane 0 of a wavefront is live whenever any of its lanes is, p rises with the lane)
	const int lo0 = __builtin_amdgcn_readfirstlane(lo);
	const bool has_fw = fw != ~0ull, has_rc = rc != ~0ull;
	if(__all(!live || lo == lo0)) {
		const unsigned c = (unsigned) (__popcll(__ballot(has_fw)) + __popcll(__ballot(has_rc)));
		if((threadIdx.x & 63) == 0 && c) atomicAdd(&slen[lo0], c);
	} else if(has_fw || has_rc) atomicAdd(&slen[lo], (unsigned) has_fw + (unsigned) has_rc);
}

// the keys of the templates that are skipped go, the others take their template's id in the index: new_id[t - 1], 0 = skipped
__global__ __launch_bounds__(256) void index_sparse_remap_kernel(unsigned long long *keys, int64_t n, const uint32_t *new_id) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const unsigned long long key = keys[i];
	if(key == ~0ull) return;
	const uint32_t id = new_id[(uint32_t) key - 1];
	keys[i] = id ? (key & 0xFFFFFFFF00000000ull) | id : ~0ull;
}

// ulen[id] = the template's distinct window k-mers (what hashMap_add returned 1 for): its share of the unique (k-mer, id) pairs. The
// pairs are sorted by k-mer, so a wavefront seldom holds one id alone; where it does (a database of a template or two) it adds once
__global__ __launch_bounds__(256) void index_sparse_ulen_kernel(const unsigned long long *pairs, int64_t n, uint32_t DB_size, unsigned *ulen) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned long long key = i < n ? pairs[i] : ~0ull;
	const bool has = key != ~0ull && (uint32_t) key < DB_size;
	const uint32_t id = has ? (uint32_t) key : 0;
	const unsigned long long m = __ballot(has);
	if(m == 0) return;                           // (wave-uniform)
	const uint32_t id0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) __shfl((int) id, __ffsll((long long) m) - 1));
	if(__all(!has || id == id0)) {
		if((threadIdx.x & 63) == 0) atomicAdd(&ulen[id0], (unsigned) __popcll(m));
	} else if(has) atomicAdd(&ulen[id], 1u);
}

// An append (`kma index -t_db`): the k-mer -> value-list table of the old .comp.b back into (k-mer << 32 | template) pairs, what
// hashMapKMA_openChains (loadupdate.c:64-112) does chain by chain. One thread per stored k-mer: the length of its list, as a 64-bit
// count for the scan; cnt[n] = 0, so that the exclusive scan over n + 1 counts ends with the number of pairs
template <typename V>
__global__ __launch_bounds__(256) void index_expand_count_kernel(const V *values, const uint32_t *vidx, int64_t n, unsigned long long *cnt) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i > n) return;
	cnt[i] = i < n ? (unsigned long long) values[vidx[i]] : 0ull;
}

// One lane per pair j of the output, so that the stores are plain consecutive 8-byte ones whatever the lists' lengths: its k-mer is
// the last i with off[i] <= j (off: the scanned counts, n + 1 of them, strictly ascending since no list is empty), found by binary
// search as index_kmers_kernel finds its template -- over the k-mers of this block alone: the block's first and last lane search all
// n first and leave their answers in LDS, and lists of a few ids keep what lies between them to a few hundred entries
template <typename V>
__global__ __launch_bounds__(256) void index_expand_pairs_kernel(const V *values, const uint32_t *keys, const uint32_t *vidx, const unsigned long long *off, int64_t n,
                                                                  int64_t total, unsigned long long *pairs) {
	__shared__ int64_t range[2];
	const int64_t j0 = (int64_t) blockIdx.x * blockDim.x, j = j0 + threadIdx.x;
	if(threadIdx.x < 2) {
		const unsigned long long jj = (unsigned long long) (threadIdx.x == 0 ? j0 : (j0 + blockDim.x - 1 < total ? j0 + blockDim.x - 1 : total - 1));
		int64_t lo = 0, hi = n;
		while(hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if(off[mid] <= jj) lo = mid; else hi = mid; }
		range[threadIdx.x] = lo;
	}
	__syncthreads();
	if(j >= total) return;
	int64_t lo = range[0], hi = range[1] + 1;
	while(hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if(off[mid] <= (unsigned long long) j) lo = mid; else hi = mid; }
	const uint32_t id = (uint32_t) values[(uint64_t) vidx[lo] + 1 + ((unsigned long long) j - off[lo])];
	pairs[j] = ((unsigned long long) keys[lo] << 32) | id;
}

struct SameKey { __device__ bool operator()(unsigned long long a, unsigned long long b) const { return a == b; } };

int read_whole(const char *path, std::vector<uint8_t> &buf) {
	gzFile f = gzopen(path, "rb");
	if(!f) { kmahip_set_error("cannot open %s", path); return KMAHIP_EIO; }
	gzbuffer(f, 1 << 20);
	size_t n = buf.size();
	for(;;) {
		buf.resize(n + (8u << 20));
		const int got = gzread(f, buf.data() + n, 8u << 20);
		if(got <= 0) break;
		n += (size_t) got;
	}
	buf.resize(n);
	gzclose(f);
	return KMAHIP_OK;
}

// host pass over the sorted (k-mer << 32 | template) pairs and the .comp.b image of what it finds: group by k-mer, share equal
// lists (valuesHash, compress.c:218), lists laid out in the order they are first needed. with_decon = false: the pairs of the
// pseudo-template DB_size are passed over; true: they stay, but a k-mer that holds nothing else is dropped. prefix_len, prefix: the two
// header fields of a sparse index (hashMapKMA_dump), 0 and 0 in every other
int write_comp_b(const std::vector<unsigned long long> &pairs, uint32_t DB_size, int k, bool with_decon, const std::string &path, uint32_t prefix_len = 0,
                 uint64_t prefix = 0) {
	const bool u16 = DB_size < 65535;                               // hashmapkma.c:340-348
	std::vector<uint32_t> ukm, vi_of_key;
	std::vector<uint32_t> values;                                   // [cnt, t1 .. tcnt] per list
	std::unordered_map<uint64_t, std::vector<uint32_t>> by_sig;     // signature -> offsets of lists with it
	std::vector<uint32_t> list;
	for(size_t a = 0; a < pairs.size();) {
		size_t b = a;
		const uint32_t km = (uint32_t) (pairs[a] >> 32);
		list.clear();
		uint64_t sig = 0x9E3779B97F4A7C15ull;
		for(; b < pairs.size() && (uint32_t) (pairs[b] >> 32) == km; ++b) {
			const uint32_t t = (uint32_t) pairs[b];
			if(t == DB_size && (!with_decon || list.empty())) continue;      // (DB_size sorts behind every template of its k-mer)
			list.push_back(t);
			sig = (sig ^ t) * 0xBF58476D1CE4E5B9ull; sig ^= sig >> 29;
		}
		a = b;
		if(list.empty()) continue;
		uint32_t off = 0xFFFFFFFFu;
		std::vector<uint32_t> &cand = by_sig[sig];
		for(uint32_t o : cand) {
			if(values[o] == list.size() && !memcmp(&values[o + 1], list.data(), list.size() * 4)) { off = o; break; }
		}
		if(off == 0xFFFFFFFFu) {
			if(values.size() + list.size() + 1 >= 0xFFFFFFFFull) { kmahip_set_error("value lists exceed 32-bit offsets"); return KMAHIP_EFORMAT; }
			off = (uint32_t) values.size();
			values.push_back((uint32_t) list.size());
			values.insert(values.end(), list.begin(), list.end());
			cand.push_back(off);
		}
		ukm.push_back(km); vi_of_key.push_back(off);
	}
	const uint64_t n = ukm.size(), v_index = values.size();
	if(n == 0) { kmahip_set_error("the templates hold no k-mer"); return KMAHIP_EFORMAT; }
	// buckets: kpos = key & (size - 1) (hashMap_getGlobal, hashmapkma.c:149-178); never the direct-address form
	uint64_t size = 1u << 20;
	while(size < n) size <<= 1;
	const uint64_t kspace = 1ull << (2 * k);
	if(size >= kspace) size = kspace >> 1;
	if(size < 2 || n > 0xFFFFFFFFull) { kmahip_set_error("index shape not supported"); return KMAHIP_EFORMAT; }
	std::vector<uint32_t> exist(size, (uint32_t) n), fill(size + 1, 0);
	for(uint64_t i = 0; i < n; ++i) ++fill[(ukm[i] & (size - 1)) + 1];
	for(uint64_t b = 0; b < size; ++b) { if(fill[b + 1]) exist[b] = fill[b]; fill[b + 1] += fill[b]; }
	std::vector<uint32_t> key_index(n + 1), value_index(n);
	{
		std::vector<uint32_t> at(fill.begin(), fill.end() - 1);
		for(uint64_t i = 0; i < n; ++i) { const uint32_t s = at[ukm[i] & (size - 1)]++; key_index[s] = ukm[i]; value_index[s] = vi_of_key[i]; }
	}
	// the sentinel behind the last key ends the scan of the last bucket: any key of another bucket (compress.c:549-585)
	key_index[n] = (uint32_t) (((key_index[n - 1] & (size - 1)) + 1) & (size - 1));

	FILE *f = fopen(path.c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s", path.c_str()); return KMAHIP_EIO; }
	const uint32_t h32[3] = {DB_size, (uint32_t) k, prefix_len};          // (a sparse index: its prefix; 0 and 0 otherwise)
	const uint64_t h64[5] = {prefix, size, n, v_index, n};
	bool ok = fwrite(h32, 4, 3, f) == 3 && fwrite(h64, 8, 5, f) == 5 && fwrite(exist.data(), 4, size, f) == size;
	if(u16) {
		std::vector<uint16_t> v16(values.begin(), values.end());
		ok = ok && fwrite(v16.data(), 2, v16.size(), f) == v16.size();
	} else ok = ok && fwrite(values.data(), 4, values.size(), f) == values.size();
	const uint32_t tail[2] = {(uint32_t) k, 0};
	ok = ok && fwrite(key_index.data(), 4, n + 1, f) == n + 1 && fwrite(value_index.data(), 4, n, f) == n && fwrite(tail, 4, 2, f) == 2;
	ok = (fclose(f) == 0) && ok;
	if(!ok) { kmahip_set_error("writing %s failed", path.c_str()); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

// the contamination records of every file behind dcodes, d_roff[r] .. d_roff[r + 1] the bases of record r (d_roff comes in as {0})
int read_decon_records(const char *const *decon_paths, int n_decon, const RefTable &T, int k, std::vector<uint8_t> &dcodes, std::vector<int64_t> &d_roff) {
	for(int fi = 0; fi < n_decon; ++fi) {
		std::vector<uint8_t> raw;
		const int rc = read_whole(decon_paths[fi], raw);
		if(rc) return rc;
		if(raw.empty() || raw[0] != '>') { kmahip_set_error("%s is not a FASTA file", decon_paths[fi]); return KMAHIP_EFORMAT; }
		size_t p = 0;
		while(p < raw.size()) {
			while(p < raw.size() && raw[p] != '\n') ++p;
			if(p < raw.size()) ++p;
			const size_t at = dcodes.size();
			while(p < raw.size() && raw[p] != '>') { const uint8_t c = T.t[raw[p]]; if(c < 8) dcodes.push_back(c); ++p; }
			if((int64_t) (dcodes.size() - at) > k) d_roff.push_back((int64_t) dcodes.size());
			else dcodes.resize(at);
		}
	}
	return KMAHIP_OK;
}

// the build itself: n_decon = 0 is `kma index` without -deCon
int index_build(const char *const *fasta_paths, int n_files, const char *const *decon_paths, int n_decon, const char *out_prefix, int kmersize) {
	if(!fasta_paths || n_files <= 0 || !out_prefix) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	const int k = kmersize > 0 ? kmersize : 16;
	if(k < 4 || k > 16) { kmahip_set_error("k-mer length %d: 4 ... 16 supported", k); return KMAHIP_EINVAL; }
	static const RefTable T;
	std::vector<Tmpl> tm;
	std::vector<uint8_t> codes;
	for(int fi = 0; fi < n_files; ++fi) {
		std::vector<uint8_t> raw;
		const int rc = read_whole(fasta_paths[fi], raw);
		if(rc) return rc;
		size_t p = 0;
		if(raw.empty() || raw[0] != '>') { kmahip_set_error("%s is not a FASTA file", fasta_paths[fi]); return KMAHIP_EFORMAT; }
		while(p < raw.size()) {
			// header line, chomped (FileBuffgetFsa, seqparse.c:66-159); the sequence is every byte the table knows up to the next '>'
			size_t e = p;
			while(e < raw.size() && raw[e] != '\n') ++e;
			size_t h = e;
			while(h > p + 1 && isspace(raw[h - 1])) --h;
			std::string name((const char *) raw.data() + p + 1, h - p - 1);
			p = e < raw.size() ? e + 1 : e;
			const size_t at = codes.size();
			while(p < raw.size() && raw[p] != '>') { const uint8_t c = T.t[raw[p]]; if(c < 8) codes.push_back(c); ++p; }
			// compDNAref, compdna.c:129-147: leading and trailing N's go; the name says how many led (makeindex.c:229-233)
			size_t a = at, b = codes.size();
			while(a < b && codes[a] == 4) ++a;
			while(b > a && codes[b - 1] == 4) --b;
			const int bias = (int) (a - at);
			if(a > at) memmove(codes.data() + at, codes.data() + a, b - a);
			codes.resize(at + (b - a));
			const int len = (int) (b - a);
			if(len < k) { codes.resize(at); continue; }                  // lengthCheck, qualcheck.c:31-41: "# Skipped"
			if(bias > 0) name += " B" + std::to_string(bias);
			Tmpl t; t.name = name; t.at = at; t.len = len;
			tm.push_back(t);
		}
	}
	const int n_t = (int) tm.size();
	if(n_t == 0) { kmahip_set_error("no template of at least %d bases", k); return KMAHIP_EFORMAT; }
	const uint32_t DB_size = (uint32_t) n_t + 1;
	const int64_t total = (int64_t) codes.size();
	// the contamination records (deConDB, decon.c:161-227): the same parser and letter table; a record counts when it is LONGER than
	// k (:193), N's and all. Leading and trailing N's need no trimming here: no k-mer holds one
	std::vector<uint8_t> dcodes;
	std::vector<int64_t> d_roff(1, 0);
	if(const int rc = read_decon_records(decon_paths, n_decon, T, k, dcodes, d_roff)) return rc;
	const int64_t dtotal = (int64_t) dcodes.size();
	const int n_dr = (int) d_roff.size() - 1;
	const int64_t n_keys = total + 2 * dtotal;

	// device: keys, sort, unique
	std::vector<int64_t> t_off((size_t) n_t + 1);
	for(int t = 0; t < n_t; ++t) t_off[(size_t) t] = (int64_t) tm[(size_t) t].at;
	t_off[(size_t) n_t] = total;
	uint8_t *d_codes = nullptr; int64_t *d_off = nullptr;
	unsigned long long *d_keys = nullptr, *d_sorted = nullptr, *d_uniq = nullptr; size_t *d_count = nullptr; void *d_tmp = nullptr;
	auto release = [&] { (void) hipFree(d_codes); (void) hipFree(d_off); (void) hipFree(d_keys); (void) hipFree(d_sorted); (void) hipFree(d_uniq); (void) hipFree(d_count); (void) hipFree(d_tmp); };
	struct Guard { decltype(release) &r; ~Guard() { r(); } } guard{release};
	HIP_TRY(hipMalloc((void **) &d_codes, (size_t) total + 32));
	HIP_TRY(hipMalloc((void **) &d_off, t_off.size() * 8));
	HIP_TRY(hipMalloc((void **) &d_keys, (size_t) n_keys * 8));
	HIP_TRY(hipMalloc((void **) &d_sorted, (size_t) n_keys * 8));
	HIP_TRY(hipMalloc((void **) &d_uniq, (size_t) n_keys * 8));
	HIP_TRY(hipMalloc((void **) &d_count, sizeof(size_t)));
	HIP_TRY(hipMemcpy(d_codes, codes.data(), (size_t) total, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_off, t_off.data(), t_off.size() * 8, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(index_kmers_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, 0, d_codes, d_off, n_t, total, k, d_keys);
	HIP_TRY(hipGetLastError());
	if(dtotal > 0) {
		// the contamination's keys behind the templates': keys[total .. total + 2 * dtotal)
		uint8_t *d_dcodes = nullptr; int64_t *d_doff = nullptr;
		hipError_t e = hipMalloc((void **) &d_dcodes, (size_t) dtotal + 32);
		if(e == hipSuccess) e = hipMalloc((void **) &d_doff, d_roff.size() * 8);
		if(e == hipSuccess) e = hipMemcpy(d_dcodes, dcodes.data(), (size_t) dtotal, hipMemcpyHostToDevice);
		if(e == hipSuccess) e = hipMemcpy(d_doff, d_roff.data(), d_roff.size() * 8, hipMemcpyHostToDevice);
		if(e == hipSuccess) {
			hipLaunchKernelGGL(index_decon_kmers_kernel, dim3((unsigned) ((dtotal + 255) / 256)), dim3(256), 0, 0, d_dcodes, d_doff, n_dr, dtotal, k, DB_size, d_keys + total);
			e = hipGetLastError();
			if(e == hipSuccess) e = hipDeviceSynchronize();
		}
		(void) hipFree(d_dcodes); (void) hipFree(d_doff);
		if(e != hipSuccess) { kmahip_set_error("decontamination keys: %s", hipGetErrorString(e)); return KMAHIP_EDEVICE; }
	}
	size_t tmp_bytes = 0, tmp2 = 0;
	if(rocprim::radix_sort_keys(nullptr, tmp_bytes, d_keys, d_sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(nullptr, tmp2, d_sorted, d_uniq, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim size query failed"); return KMAHIP_EDEVICE; }
	tmp_bytes = std::max(tmp_bytes, tmp2);
	HIP_TRY(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16));
	if(rocprim::radix_sort_keys(d_tmp, tmp_bytes, d_keys, d_sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(d_tmp, tmp_bytes, d_sorted, d_uniq, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim sort / unique failed"); return KMAHIP_EDEVICE; }
	HIP_TRY(hipDeviceSynchronize());
	size_t n_pairs = 0;
	HIP_TRY(hipMemcpy(&n_pairs, d_count, sizeof n_pairs, hipMemcpyDeviceToHost));
	std::vector<unsigned long long> pairs(n_pairs);
	if(n_pairs) HIP_TRY(hipMemcpy(pairs.data(), d_uniq, n_pairs * 8, hipMemcpyDeviceToHost));
	if(n_pairs && pairs.back() == ~0ull) pairs.pop_back();         // the starts that hold no k-mer sorted to the end
	if(pairs.empty()) { kmahip_set_error("the templates hold no k-mer"); return KMAHIP_EFORMAT; }

	const std::string base(out_prefix);
	int rcw = write_comp_b(pairs, DB_size, k, false, base + ".comp.b");
	if(!rcw && n_decon > 0) rcw = write_comp_b(pairs, DB_size, k, true, base + ".decon.comp.b");
	if(rcw) return rcw;
	bool ok = true;
	// .length.b: DB_size, then the lengths with slot 0 = the k of the position index (makeindex.c:300-311)
	FILE *f = fopen((base + ".length.b").c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s.length.b", out_prefix); return KMAHIP_EIO; }
	std::vector<uint32_t> lens(DB_size);
	lens[0] = (uint32_t) k;
	for(int t = 0; t < n_t; ++t) lens[(size_t) t + 1] = (uint32_t) tm[(size_t) t].len;
	ok = fwrite(&DB_size, 4, 1, f) == 1 && fwrite(lens.data(), 4, DB_size, f) == DB_size && ok;
	ok = (fclose(f) == 0) && ok;
	// .seq.b: (len >> 5) + 1 words per template, 32 bases a word from the top, N as A (updateAnnots; read back at runkma.c:214-220)
	f = fopen((base + ".seq.b").c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s.seq.b", out_prefix); return KMAHIP_EIO; }
	std::vector<uint64_t> words;
	for(int t = 0; t < n_t; ++t) {
		const Tmpl &x = tm[(size_t) t];
		words.assign((size_t) (x.len >> 5) + 1, 0);
		for(int i = 0; i < x.len; ++i) words[(size_t) i >> 5] |= (uint64_t) (codes[x.at + (size_t) i] & 3) << (62 - ((i & 31) << 1));
		ok = fwrite(words.data(), 8, words.size(), f) == words.size() && ok;
	}
	ok = (fclose(f) == 0) && ok;
	f = fopen((base + ".name").c_str(), "wb");
	if(!f) { kmahip_set_error("cannot create %s.name", out_prefix); return KMAHIP_EIO; }
	for(int t = 0; t < n_t; ++t) ok = fprintf(f, "%s\n", tm[(size_t) t].name.c_str()) > 0 && ok;
	ok = (fclose(f) == 0) && ok;
	if(!ok) { kmahip_set_error("writing the index under %s failed", out_prefix); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

// `kma index -Sparse <prefix | -> [-ML n]`: which k-mers become keys, both strands, templates that go and the ids that move up behind
// them, two more arrays in .length.b and the prefix in the .comp.b header. The rule is index_host.h's; the device finds the windows
// under the ids of the file order (index_sparse_keys_kernel), the host picks the templates that stay from n_t window counts, the keys
// are renumbered where a template went (index_sparse_remap_kernel) and go through the plain build's sort and unique, and the unique
// pairs are counted per template (index_sparse_ulen_kernel)
double g_hom_ms[4] = {0, 0, 0, 0};          // the last homology step: pass 1, resolve, pass 2 in ms; pairs listed

// The homology step of a sparse build (QualCheck = queryCheck / templateCheck): the device counts the pairs (homology.hip), the host
// settles who stays and writes the line of every template that reaches the gate (index_host.h). report_path: NULL none, "-" standard
// output. capture (the test hook): seven words a candidate template: stays, thisKlen, then the row of pass 2 under file-order ids
int index_sparse_homology(const unsigned long long *d_keys, int64_t n_keys, const int64_t *d_off, const std::vector<Tmpl> &tm, const std::vector<uint32_t> &slen,
                          const SparseRule &rule, const HomRule &hom, const char *report_path, std::vector<uint8_t> &kept, std::vector<uint32_t> *capture) {
	KmaHom *h = nullptr;
	int rc = kmahip_hom_open(d_keys, n_keys, d_off, slen, rule.prefix_len + rule.k, rule.MinKlen, &h);
	if(rc) return rc;
	struct Guard { KmaHom *h; ~Guard() { kmahip_hom_close(h); } } guard{h};
	std::vector<KmaHomPair> pairs;
	std::vector<KmaHomRow> rows;
	// (each step ends with a copy to the host, so the host's clock times it: kmahip_test_index_hom_timing)
	const auto t0 = std::chrono::steady_clock::now();
	if((rc = kmahip_hom_pairs(h, hom.homQ, hom.homT, hom.mode() == 2, pairs))) return rc;
	const auto t1 = std::chrono::steady_clock::now();
	static_assert(sizeof(KmaHomPair) == 8, "a pair is two words");
	hom_resolve(slen, rule, hom, (const uint32_t *) pairs.data(), pairs.size(), kept);
	const auto t2 = std::chrono::steady_clock::now();
	if((rc = kmahip_hom_best(h, kept, rows))) return rc;
	const auto t3 = std::chrono::steady_clock::now();
	g_hom_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
	g_hom_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
	g_hom_ms[2] = std::chrono::duration<double, std::milli>(t3 - t2).count();
	g_hom_ms[3] = (double) pairs.size();
	FILE *f = nullptr;
	if(report_path && !(f = strcmp(report_path, "-") ? fopen(report_path, "wb") : stdout)) { kmahip_set_error("cannot create %s", report_path); return KMAHIP_EIO; }
	uint32_t next = 1;
	std::vector<uint32_t> id_of(tm.size(), 0);
	bool agree = true;
	if(capture) capture->assign(tm.size() * 7, 0);
	for(size_t t = 0; t < tm.size(); ++t) {
		if(kept[t]) id_of[t] = next++;
		const KmaHomRow &r = rows[t];
		if(capture) { uint32_t *c = capture->data() + 7 * t; c[0] = kept[t]; c[1] = slen[t]; c[2] = r.tot; c[3] = r.jQ; c[4] = r.num; c[5] = r.den; c[6] = r.jT; }
		if(!hom_eligible(slen[t], rule)) continue;
		agree = hom_report_line(f, hom, tm[t].name.substr(0, tm[t].head).c_str(), id_of[t], r.tot, slen[t], r.jQ ? id_of[r.jQ - 1] : 0, r.num, r.den, r.jT ? id_of[r.jT - 1] : 0) && agree;
	}
	bool ok = true;
	if(f) ok = (f == stdout ? fflush(f) == 0 : fclose(f) == 0) && !ferror(stdout);
	if(!ok) { kmahip_set_error("writing the homology report %s failed", report_path); return KMAHIP_EIO; }
	if(!agree) { kmahip_set_error("homology reduction: the winners of pass 2 contradict the flags of pass 1"); return KMAHIP_EDEVICE; }
	return KMAHIP_OK;
}

int index_build_sparse(const char *const *fasta_paths, int n_files, const char *out_prefix, int kmersize, int kmerindex, const char *prefix_text, int min_len,
                       const HomRule *hom = nullptr, const char *report_path = nullptr, std::vector<uint32_t> *capture = nullptr) {
	if(!fasta_paths || n_files <= 0 || (!out_prefix && !capture)) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	static const RefTable T;
	SparseRule rule;
	rule.k = kmersize > 0 ? kmersize : 16;
	rule.kmerindex = kmerindex > 0 ? kmerindex : rule.k;
	if(rule.k < 4 || rule.k > 16) { kmahip_set_error("k-mer length %d: 4 ... 16 supported", rule.k); return KMAHIP_EINVAL; }
	if(rule.kmerindex > 31) { kmahip_set_error("k-mer length of the position index %d: at most 31", rule.kmerindex); return KMAHIP_EINVAL; }
	int rc = sparse_parse_prefix(prefix_text, T, rule);
	if(rc) return rc;
	sparse_set_gates(min_len, rule);
	// templateCheck leaves at qualcheck.c:287 with its score arrays and found-k-mer set as they are when a template misses -ML's window
	// count, so what the reference answers afterwards depends on stale state: not a rule to restate
	if(hom && hom->mode() == 2 && rule.MinKlen > 1) { kmahip_set_error("sparse index: -ht with -ML is not built (templateCheck keeps stale scores behind a template below -ML)"); return KMAHIP_EINVAL; }
	const int k = rule.k;
	std::vector<Tmpl> tm;
	std::vector<uint8_t> codes;
	for(int fi = 0; fi < n_files; ++fi) {
		std::vector<uint8_t> raw;
		if((rc = read_whole(fasta_paths[fi], raw))) return rc;
		if((rc = sparse_parse_fasta(raw, fasta_paths[fi], T, rule.MinLen, codes, tm))) return rc;
	}
	const int n_t = (int) tm.size();
	if(n_t == 0) { kmahip_set_error("no template of more than %d bases", rule.MinLen); return KMAHIP_EFORMAT; }
	const int64_t total = (int64_t) codes.size(), n_keys = 2 * total;
	std::vector<int64_t> t_off((size_t) n_t + 1);
	for(int t = 0; t < n_t; ++t) t_off[(size_t) t] = (int64_t) tm[(size_t) t].at;
	t_off[(size_t) n_t] = total;

	uint8_t *d_codes = nullptr; int64_t *d_off = nullptr; unsigned *d_slen = nullptr, *d_ulen = nullptr; uint32_t *d_newid = nullptr;
	unsigned long long *d_keys = nullptr, *d_sorted = nullptr, *d_uniq = nullptr; size_t *d_count = nullptr; void *d_tmp = nullptr;
	auto release = [&] { (void) hipFree(d_codes); (void) hipFree(d_off); (void) hipFree(d_slen); (void) hipFree(d_ulen); (void) hipFree(d_newid); (void) hipFree(d_keys);
	                     (void) hipFree(d_sorted); (void) hipFree(d_uniq); (void) hipFree(d_count); (void) hipFree(d_tmp); };
	struct Guard { decltype(release) &r; ~Guard() { r(); } } guard{release};
	HIP_TRY(hipMalloc((void **) &d_codes, (size_t) total + 32));
	HIP_TRY(hipMalloc((void **) &d_off, t_off.size() * 8));
	HIP_TRY(hipMalloc((void **) &d_slen, (size_t) n_t * 4));
	HIP_TRY(hipMalloc((void **) &d_keys, (size_t) n_keys * 8));
	HIP_TRY(hipMemcpy(d_codes, codes.data(), (size_t) total, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_off, t_off.data(), t_off.size() * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipMemset(d_slen, 0, (size_t) n_t * 4));
	hipLaunchKernelGGL(index_sparse_keys_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, 0, d_codes, d_off, n_t, total, k, rule.prefix_len,
	                   (unsigned long long) rule.prefix, d_keys, d_slen);
	HIP_TRY(hipGetLastError());
	std::vector<uint32_t> slen((size_t) n_t), new_id;
	HIP_TRY(hipMemcpy(slen.data(), d_slen, (size_t) n_t * 4, hipMemcpyDeviceToHost));
	std::vector<uint8_t> kept;
	const bool homology = hom && hom->mode();
	if(homology) {
		if((rc = index_sparse_homology(d_keys, n_keys, d_off, tm, slen, rule, *hom, report_path, kept, capture))) return rc;
		if(!out_prefix) return KMAHIP_OK;
	}
	const uint32_t n_kept = sparse_assign_ids(tm, slen, rule, new_id, homology ? &kept : nullptr);
	if(n_kept == 0) { kmahip_set_error("DB is empty: no template holds a k-mer behind the prefix"); return KMAHIP_EFORMAT; }
	const uint32_t DB_size = n_kept + 1;
	if(n_kept != (uint32_t) n_t) {
		HIP_TRY(hipMalloc((void **) &d_newid, (size_t) n_t * 4));
		HIP_TRY(hipMemcpy(d_newid, new_id.data(), (size_t) n_t * 4, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(index_sparse_remap_kernel, dim3((unsigned) ((n_keys + 255) / 256)), dim3(256), 0, 0, d_keys, n_keys, d_newid);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMalloc((void **) &d_sorted, (size_t) n_keys * 8));
	HIP_TRY(hipMalloc((void **) &d_uniq, (size_t) n_keys * 8));
	HIP_TRY(hipMalloc((void **) &d_count, sizeof(size_t)));
	HIP_TRY(hipMalloc((void **) &d_ulen, (size_t) DB_size * 4));
	HIP_TRY(hipMemset(d_ulen, 0, (size_t) DB_size * 4));
	size_t tmp_bytes = 0, tmp2 = 0;
	if(rocprim::radix_sort_keys(nullptr, tmp_bytes, d_keys, d_sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(nullptr, tmp2, d_sorted, d_uniq, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim size query failed"); return KMAHIP_EDEVICE; }
	tmp_bytes = std::max(tmp_bytes, tmp2);
	HIP_TRY(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16));
	if(rocprim::radix_sort_keys(d_tmp, tmp_bytes, d_keys, d_sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(d_tmp, tmp_bytes, d_sorted, d_uniq, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim sort / unique failed"); return KMAHIP_EDEVICE; }
	size_t n_pairs = 0;
	HIP_TRY(hipMemcpy(&n_pairs, d_count, sizeof n_pairs, hipMemcpyDeviceToHost));
	if(n_pairs > (size_t) n_keys) { kmahip_set_error("rocprim unique returned %zu of %lld keys", n_pairs, (long long) n_keys); return KMAHIP_EDEVICE; }
	if(n_pairs) {
		hipLaunchKernelGGL(index_sparse_ulen_kernel, dim3((unsigned) ((n_pairs + 255) / 256)), dim3(256), 0, 0, d_uniq, (int64_t) n_pairs, DB_size, d_ulen);
		HIP_TRY(hipGetLastError());
	}
	std::vector<unsigned long long> pairs(n_pairs);
	if(n_pairs) HIP_TRY(hipMemcpy(pairs.data(), d_uniq, n_pairs * 8, hipMemcpyDeviceToHost));
	std::vector<uint32_t> ulen((size_t) DB_size);
	HIP_TRY(hipMemcpy(ulen.data(), d_ulen, (size_t) DB_size * 4, hipMemcpyDeviceToHost));
	if(n_pairs && pairs.back() == ~0ull) pairs.pop_back();         // the starts that hold no window sorted to the end
	if(pairs.empty()) { kmahip_set_error("DB is empty: no template holds a k-mer behind the prefix"); return KMAHIP_EFORMAT; }

	const std::string base(out_prefix);
	if((rc = write_comp_b(pairs, DB_size, k, false, base + ".comp.b", (uint32_t) rule.prefix_len, rule.prefix))) return rc;
	if((rc = sparse_write_length_b(base + ".length.b", tm, new_id, DB_size, rule.kmerindex, slen, ulen))) return rc;
	return sparse_write_seq_and_names(base, tm, new_id, codes);
}

// ---- `kma index -t_db <prefix>`: append to an index that exists ------------------------------------------------------------------
double g_expand_ms[3] = {0, 0, 0};          // the last expansion: count kernel, scan, pairs kernel in ms (device events)

// <prefix>.comp.b as an append takes it: read, and held to its own header before any of it reaches the device
struct OldIndex {
	KmaComp c;
	bool sparse = false;
	uint64_t n_pairs = 0;
};

int append_open(const std::string &base, OldIndex &o) {
	if(const int rc = kmahip_comp_read(base + ".comp.b", true, &o.c)) return rc;          // (refuses k > 16 and flag != 0 by name)
	o.sparse = !(o.c.prefix_len == 0 && o.c.prefix == 0);                                  // index.c:542-546
	if(o.c.prefix_len > 16 || (!o.c.mega && o.c.n != o.c.n_hdr)) { kmahip_set_error(KMAHIP_WRONG_DB " (prefix of %u bases)", o.c.prefix_len); return KMAHIP_EFORMAT; }
	return append_check_lists(o.c.keys.data(), o.c.vidx.data(), o.c.n, o.c.values.data(), o.c.u16, o.c.v_index, o.c.DB_size, (int) o.c.mlen, &o.n_pairs);
}

// the pairs of a checked index into d_pairs[0 .. o.n_pairs), in the order of the file's k-mers
int expand_on_device(const OldIndex &o, unsigned long long *d_pairs) {
	const KmaComp &c = o.c;
	const int64_t n = (int64_t) c.n;
	const size_t vbytes = (size_t) c.v_index * (c.u16 ? 2 : 4);
	void *d_values = nullptr, *d_tmp = nullptr; uint32_t *d_k = nullptr, *d_vi = nullptr; unsigned long long *d_cnt = nullptr, *d_off = nullptr;
	hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	auto release = [&] { (void) hipFree(d_values); (void) hipFree(d_tmp); (void) hipFree(d_k); (void) hipFree(d_vi); (void) hipFree(d_cnt); (void) hipFree(d_off);
	                     for(hipEvent_t e : ev) if(e) (void) hipEventDestroy(e); };
	struct Guard { decltype(release) &r; ~Guard() { r(); } } guard{release};
	HIP_TRY(hipMalloc(&d_values, vbytes));
	HIP_TRY(hipMalloc((void **) &d_k, (size_t) n * 4));
	HIP_TRY(hipMalloc((void **) &d_vi, (size_t) n * 4));
	HIP_TRY(hipMalloc((void **) &d_cnt, ((size_t) n + 1) * 8));
	HIP_TRY(hipMalloc((void **) &d_off, ((size_t) n + 1) * 8));
	HIP_TRY(hipMemcpy(d_values, c.values.data(), vbytes, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_k, c.keys.data(), (size_t) n * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_vi, c.vidx.data(), (size_t) n * 4, hipMemcpyHostToDevice));
	size_t tmp_bytes = 0;
	if(rocprim::exclusive_scan(nullptr, tmp_bytes, d_cnt, d_off, 0ull, (size_t) n + 1, rocprim::plus<unsigned long long>(), 0) != hipSuccess) { kmahip_set_error("rocprim size query failed"); return KMAHIP_EDEVICE; }
	HIP_TRY(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16));
	for(hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
	const dim3 g_cnt((unsigned) ((n + 1 + 255) / 256)), g_pairs((unsigned) ((o.n_pairs + 255) / 256));
	HIP_TRY(hipEventRecord(ev[0], 0));
	if(c.u16) hipLaunchKernelGGL(index_expand_count_kernel<uint16_t>, g_cnt, dim3(256), 0, 0, (const uint16_t *) d_values, d_vi, n, d_cnt);
	else hipLaunchKernelGGL(index_expand_count_kernel<uint32_t>, g_cnt, dim3(256), 0, 0, (const uint32_t *) d_values, d_vi, n, d_cnt);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(ev[1], 0));
	if(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_cnt, d_off, 0ull, (size_t) n + 1, rocprim::plus<unsigned long long>(), 0) != hipSuccess) { kmahip_set_error("rocprim scan failed"); return KMAHIP_EDEVICE; }
	HIP_TRY(hipEventRecord(ev[2], 0));
	// the write pass is sized by the host's count of the pairs: the scan must say the same before a lane derives an address from it
	unsigned long long total = 0;
	HIP_TRY(hipMemcpy(&total, d_off + n, 8, hipMemcpyDeviceToHost));
	if(total != o.n_pairs) { kmahip_set_error("index expansion: the scan counts %llu pairs, the host %llu", total, (unsigned long long) o.n_pairs); return KMAHIP_EDEVICE; }
	HIP_TRY(hipEventRecord(ev[3], 0));
	if(c.u16) hipLaunchKernelGGL(index_expand_pairs_kernel<uint16_t>, g_pairs, dim3(256), 0, 0, (const uint16_t *) d_values, d_k, d_vi, d_off, n, (int64_t) total, d_pairs);
	else hipLaunchKernelGGL(index_expand_pairs_kernel<uint32_t>, g_pairs, dim3(256), 0, 0, (const uint32_t *) d_values, d_k, d_vi, d_off, n, (int64_t) total, d_pairs);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(ev[4], 0));
	HIP_TRY(hipEventSynchronize(ev[4]));
	float ms[3] = {0, 0, 0};
	HIP_TRY(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
	HIP_TRY(hipEventElapsedTime(&ms[1], ev[1], ev[2]));
	HIP_TRY(hipEventElapsedTime(&ms[2], ev[3], ev[4]));
	for(int i = 0; i < 3; ++i) g_expand_ms[i] = ms[i];
	return KMAHIP_OK;
}

int index_append(const char *db_prefix, const char *const *fasta_paths, int n_files, const char *const *decon_paths, int n_decon, const char *out_prefix) {
	if(!db_prefix || n_files < 0 || n_decon < 0 || (n_files > 0 && !fasta_paths) || (n_decon > 0 && !decon_paths)) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(n_files == 0 && n_decon == 0) { kmahip_set_error("No inputfiles defined."); return KMAHIP_EINVAL; }
	for(int i = 0; i < n_files; ++i) if(!fasta_paths[i]) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	for(int i = 0; i < n_decon; ++i)
		if(!decon_paths[i] || !strcmp(decon_paths[i], "--")) { kmahip_set_error("decontamination from standard input (--) is not built: give a file"); return KMAHIP_EINVAL; }
	static const RefTable T;
	const std::string old_base(db_prefix), base(out_prefix ? out_prefix : db_prefix), tmp = base + ".appending";
	OldIndex o;
	int rc = append_open(old_base, o);
	if(rc) return rc;
	if(o.sparse && n_decon > 0) { kmahip_set_error("index append: -deCon on a sparse index is not built (deConNode_sparse)"); return KMAHIP_EINVAL; }
	const int k = (int) o.c.mlen;
	const uint32_t old_DB = o.c.DB_size;
	OldAnnots ann;
	if((rc = append_read_annots(old_base, old_DB, o.sparse, n_files > 0, ann))) return rc;

	// the new templates, parsed as a fresh build parses them; k and the prefix are the index's (index.c:535-546)
	SparseRule rule;
	rule.k = k; rule.kmerindex = o.sparse && ann.slen[0] ? (int) std::min<uint32_t>(ann.slen[0], 31) : k;          // load_DBs: kmerindex = slengths[0]
	rule.prefix_len = (int) o.c.prefix_len; rule.prefix = o.c.prefix;
	sparse_set_gates(0, rule);
	std::vector<Tmpl> tm;
	std::vector<uint8_t> codes;
	for(int fi = 0; fi < n_files; ++fi) {
		std::vector<uint8_t> raw;
		if((rc = read_whole(fasta_paths[fi], raw))) return rc;
		// (a plain build keeps a template of k bases: index_build's `len < k`)
		if((rc = sparse_parse_fasta(raw, fasta_paths[fi], T, o.sparse ? rule.MinLen : k - 1, codes, tm))) return rc;
	}
	const int n_t = (int) tm.size();
	if(n_files > 0 && n_t == 0) { kmahip_set_error("no template of at least %d bases", k); return KMAHIP_EFORMAT; }
	std::vector<uint8_t> dcodes;
	std::vector<int64_t> d_roff(1, 0);
	if((rc = read_decon_records(decon_paths, n_decon, T, k, dcodes, d_roff))) return rc;
	const int64_t total = (int64_t) codes.size(), dtotal = (int64_t) dcodes.size(), n_new = o.sparse ? 2 * total : total;
	const int n_dr = (int) d_roff.size() - 1;
	const int64_t n_old = (int64_t) o.n_pairs, n_keys = n_new + 2 * dtotal + n_old;
	std::vector<int64_t> t_off((size_t) n_t + 1);
	for(int t = 0; t < n_t; ++t) t_off[(size_t) t] = (int64_t) tm[(size_t) t].at;
	t_off[(size_t) n_t] = total;

	// device: keys[0 .. n_new) the new templates', [n_new .. + 2 dtotal) the contamination's, behind them the old index's pairs
	uint8_t *d_codes = nullptr, *d_dcodes = nullptr; int64_t *d_off = nullptr, *d_doff = nullptr; unsigned *d_slen = nullptr, *d_ulen = nullptr; uint32_t *d_newid = nullptr;
	unsigned long long *d_keys = nullptr, *d_sorted = nullptr, *d_uniq = nullptr; size_t *d_count = nullptr; void *d_tmp = nullptr;
	auto release = [&] { (void) hipFree(d_codes); (void) hipFree(d_dcodes); (void) hipFree(d_off); (void) hipFree(d_doff); (void) hipFree(d_slen); (void) hipFree(d_ulen);
	                     (void) hipFree(d_newid); (void) hipFree(d_keys); (void) hipFree(d_sorted); (void) hipFree(d_uniq); (void) hipFree(d_count); (void) hipFree(d_tmp); };
	struct Guard { decltype(release) &r; ~Guard() { r(); } } guard{release};
	HIP_TRY(hipMalloc((void **) &d_keys, (size_t) n_keys * 8));
	if((rc = expand_on_device(o, d_keys + n_new + 2 * dtotal))) return rc;
	std::vector<uint32_t> slen, new_id;
	uint32_t DB_size = old_DB;
	if(n_t > 0) {
		HIP_TRY(hipMalloc((void **) &d_codes, (size_t) total + 32));
		HIP_TRY(hipMalloc((void **) &d_off, t_off.size() * 8));
		HIP_TRY(hipMalloc((void **) &d_newid, (size_t) n_t * 4));
		HIP_TRY(hipMemcpy(d_codes, codes.data(), (size_t) total, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_off, t_off.data(), t_off.size() * 8, hipMemcpyHostToDevice));
		if(o.sparse) {
			HIP_TRY(hipMalloc((void **) &d_slen, (size_t) n_t * 4));
			HIP_TRY(hipMemset(d_slen, 0, (size_t) n_t * 4));
			hipLaunchKernelGGL(index_sparse_keys_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, 0, d_codes, d_off, n_t, total, k, rule.prefix_len,
			                   (unsigned long long) rule.prefix, d_keys, d_slen);
			HIP_TRY(hipGetLastError());
			slen.resize((size_t) n_t);
			HIP_TRY(hipMemcpy(slen.data(), d_slen, (size_t) n_t * 4, hipMemcpyDeviceToHost));
			if(sparse_assign_ids(tm, slen, rule, new_id) == 0) { kmahip_set_error("no new template holds a k-mer behind the prefix"); return KMAHIP_EFORMAT; }
		} else {
			hipLaunchKernelGGL(index_kmers_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, 0, d_codes, d_off, n_t, total, k, d_keys);
			HIP_TRY(hipGetLastError());
			new_id.resize((size_t) n_t);
			for(int t = 0; t < n_t; ++t) new_id[(size_t) t] = (uint32_t) t + 1;
		}
		// the ids of the new templates start at the old DB_size (update_DB with templates->DB_size, makeindex.c:225)
		if((uint64_t) old_DB + (uint64_t) n_t >= 0xFFFFFFFFull) { kmahip_set_error("more than 2^32 templates"); return KMAHIP_EFORMAT; }
		for(uint32_t &id : new_id) if(id) { id += old_DB - 1; DB_size = id + 1; }
		HIP_TRY(hipMemcpy(d_newid, new_id.data(), (size_t) n_t * 4, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(index_sparse_remap_kernel, dim3((unsigned) ((n_new + 255) / 256)), dim3(256), 0, 0, d_keys, n_new, d_newid);
		HIP_TRY(hipGetLastError());
	}
	if(dtotal > 0) {
		// the pseudo-template is the NEW DB_size (deConDB runs on the index as it stands after the append, index.c:676-696)
		HIP_TRY(hipMalloc((void **) &d_dcodes, (size_t) dtotal + 32));
		HIP_TRY(hipMalloc((void **) &d_doff, d_roff.size() * 8));
		HIP_TRY(hipMemcpy(d_dcodes, dcodes.data(), (size_t) dtotal, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_doff, d_roff.data(), d_roff.size() * 8, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(index_decon_kmers_kernel, dim3((unsigned) ((dtotal + 255) / 256)), dim3(256), 0, 0, d_dcodes, d_doff, n_dr, dtotal, k, DB_size, d_keys + n_new);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMalloc((void **) &d_sorted, (size_t) n_keys * 8));
	HIP_TRY(hipMalloc((void **) &d_uniq, (size_t) n_keys * 8));
	HIP_TRY(hipMalloc((void **) &d_count, sizeof(size_t)));
	size_t tmp_bytes = 0, tmp2 = 0;
	if(rocprim::radix_sort_keys(nullptr, tmp_bytes, d_keys, d_sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(nullptr, tmp2, d_sorted, d_uniq, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim size query failed"); return KMAHIP_EDEVICE; }
	tmp_bytes = std::max(tmp_bytes, tmp2);
	HIP_TRY(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 16));
	if(rocprim::radix_sort_keys(d_tmp, tmp_bytes, d_keys, d_sorted, (size_t) n_keys, 0, 64, 0) != hipSuccess ||
	   rocprim::unique(d_tmp, tmp_bytes, d_sorted, d_uniq, d_count, (size_t) n_keys, SameKey(), 0) != hipSuccess) { kmahip_set_error("rocprim sort / unique failed"); return KMAHIP_EDEVICE; }
	size_t n_pairs = 0;
	HIP_TRY(hipMemcpy(&n_pairs, d_count, sizeof n_pairs, hipMemcpyDeviceToHost));
	if(n_pairs > (size_t) n_keys) { kmahip_set_error("rocprim unique returned %zu of %lld keys", n_pairs, (long long) n_keys); return KMAHIP_EDEVICE; }
	std::vector<uint32_t> ulen;
	if(o.sparse && n_pairs) {
		// (the old templates keep the ulengths their file holds; the count of the new ones is their share of the unique pairs)
		HIP_TRY(hipMalloc((void **) &d_ulen, (size_t) DB_size * 4));
		HIP_TRY(hipMemset(d_ulen, 0, (size_t) DB_size * 4));
		hipLaunchKernelGGL(index_sparse_ulen_kernel, dim3((unsigned) ((n_pairs + 255) / 256)), dim3(256), 0, 0, d_uniq, (int64_t) n_pairs, DB_size, d_ulen);
		HIP_TRY(hipGetLastError());
		ulen.resize((size_t) DB_size);
		HIP_TRY(hipMemcpy(ulen.data(), d_ulen, (size_t) DB_size * 4, hipMemcpyDeviceToHost));
	}
	std::vector<unsigned long long> pairs(n_pairs);
	if(n_pairs) HIP_TRY(hipMemcpy(pairs.data(), d_uniq, n_pairs * 8, hipMemcpyDeviceToHost));
	if(n_pairs && pairs.back() == ~0ull) pairs.pop_back();         // the starts that hold no k-mer sorted to the end
	if(pairs.empty()) { kmahip_set_error("the templates hold no k-mer"); return KMAHIP_EFORMAT; }

	// every file under a name of its own beside its target, the names taken at the end: a failed append leaves the old index whole
	std::vector<const char *> exts;
	if(n_files > 0) {
		exts = {".comp.b", ".length.b", ".seq.b", ".name"};
		rc = write_comp_b(pairs, DB_size, k, false, tmp + ".comp.b", o.c.prefix_len, o.c.prefix);
		if(!rc) {
			std::vector<uint32_t> lens(ann.lens), sl(ann.slen), ul(ann.ulen);
			lens.resize(DB_size, 0);
			if(o.sparse) { sl.resize(DB_size, 0); ul.resize(DB_size, 0); }
			for(int t = 0; t < n_t; ++t) {
				const uint32_t id = new_id[(size_t) t];
				if(!id) continue;
				lens[id] = (uint32_t) tm[(size_t) t].len;
				if(o.sparse) { sl[id] = slen[(size_t) t]; ul[id] = ulen[id]; }
			}
			rc = append_write_length_b(tmp + ".length.b", DB_size, lens, o.sparse ? &sl : nullptr, o.sparse ? &ul : nullptr);
		}
		if(!rc) rc = sparse_write_seq_and_names(tmp, tm, new_id, codes, &ann.seq, &ann.names);
	}
	if(!rc && n_decon > 0) {
		exts.push_back(".decon.comp.b");
		rc = write_comp_b(pairs, DB_size, k, true, tmp + ".decon.comp.b", o.c.prefix_len, o.c.prefix);
	}
	const int rc2 = append_commit(tmp, base, exts, rc == KMAHIP_OK);
	return rc ? rc : rc2;
}

}  // namespace

extern "C" int kmahip_index_build_sparse(const char *const *fasta_paths, int n_files, const char *out_prefix, int kmersize, int kmerindex,
                                         const char *prefix_text, int min_len) {
	return index_build_sparse(fasta_paths, n_files, out_prefix, kmersize, kmerindex, prefix_text, min_len);
}

extern "C" int kmahip_index_build_sparse_hom(const char *const *fasta_paths, int n_files, const char *out_prefix, int kmersize, int kmerindex,
                                             const char *prefix_text, int min_len, double hom_q, double hom_t, int and_mode, const char *report_path) {
	if(!out_prefix) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	HomRule hom;
	hom.homQ = hom_q; hom.homT = hom_t; hom.and_mode = and_mode != 0;
	if(!(hom_q >= 0) || !(hom_t >= 0)) { kmahip_set_error("homology thresholds %g, %g: not below 0", hom_q, hom_t); return KMAHIP_EINVAL; }
	if(!hom.mode() && report_path && strcmp(report_path, "-")) {
		// lengthCheck prints nothing: the report is there and empty
		FILE *f = fopen(report_path, "wb");
		if(!f || fclose(f)) { kmahip_set_error("cannot create %s", report_path); return KMAHIP_EIO; }
	}
	return index_build_sparse(fasta_paths, n_files, out_prefix, kmersize, kmerindex, prefix_text, min_len, &hom, report_path);
}

// the test hook of the homology counts: no file is written; out: seven words a candidate template in file order (stays, thisKlen, max
// Scores_tot, its template, Scores and ulen of the max thisT, its template; templates by file order, 1 ..), *n_rows of them
extern "C" int kmahip_test_index_hom_rows(const char *const *fasta_paths, int n_files, int kmersize, const char *prefix_text, int min_len, double hom_q, double hom_t,
                                          int and_mode, uint32_t *out, int64_t cap_rows, int64_t *n_rows) {
	HomRule hom;
	hom.homQ = hom_q; hom.homT = hom_t; hom.and_mode = and_mode != 0;
	if(!hom.mode() || !out || !n_rows) { kmahip_set_error("kmahip_test_index_hom_rows: bad argument"); return KMAHIP_EINVAL; }
	std::vector<uint32_t> capture;
	const int rc = index_build_sparse(fasta_paths, n_files, nullptr, kmersize, kmersize, prefix_text, min_len, &hom, nullptr, &capture);
	if(rc) return rc;
	*n_rows = (int64_t) (capture.size() / 7);
	if(*n_rows > cap_rows) { kmahip_set_error("kmahip_test_index_hom_rows: %lld rows, room for %lld", (long long) *n_rows, (long long) cap_rows); return KMAHIP_EINVAL; }
	memcpy(out, capture.data(), capture.size() * 4);
	return KMAHIP_OK;
}

// what the last homology step of this process took: ms of pass 1 (with a regrown list: both launches), of the host's resolve and of
// pass 2, and the pairs pass 1 listed
extern "C" int kmahip_test_index_hom_timing(double *out4) {
	if(!out4) return KMAHIP_EINVAL;
	memcpy(out4, g_hom_ms, sizeof g_hom_ms);
	return KMAHIP_OK;
}

extern "C" int kmahip_index_append(const char *db_prefix, const char *const *fasta_paths, int n_files, const char *const *decon_paths, int n_decon,
                                   const char *out_prefix) {
	return index_append(db_prefix, fasta_paths, n_files, decon_paths, n_decon, out_prefix);
}

// the test hook of the expansion: the pairs of <prefix>.comp.b as the device wrote them, in the order of the file's k-mers
extern "C" int kmahip_test_index_expand(const char *prefix, uint64_t *out_pairs, int64_t cap, int64_t *n) {
	if(!prefix || !n || (!out_pairs && cap > 0)) { kmahip_set_error("kmahip_test_index_expand: bad argument"); return KMAHIP_EINVAL; }
	OldIndex o;
	int rc = append_open(std::string(prefix), o);
	if(rc) return rc;
	*n = (int64_t) o.n_pairs;
	if(*n > cap) { kmahip_set_error("kmahip_test_index_expand: %lld pairs, room for %lld", (long long) *n, (long long) cap); return KMAHIP_EINVAL; }
	unsigned long long *d_pairs = nullptr;
	HIP_TRY(hipMalloc((void **) &d_pairs, (size_t) o.n_pairs * 8));
	rc = expand_on_device(o, d_pairs);
	hipError_t e = hipSuccess;
	if(!rc) e = hipMemcpy(out_pairs, d_pairs, (size_t) o.n_pairs * 8, hipMemcpyDeviceToHost);
	(void) hipFree(d_pairs);
	if(e != hipSuccess) { kmahip_set_error("kmahip_test_index_expand: %s", hipGetErrorString(e)); return KMAHIP_EDEVICE; }
	return rc;
}

// what the last expansion of this process took on the device: ms of the count kernel, of the scan and of the write pass
extern "C" int kmahip_test_index_expand_timing(double *out3) {
	if(!out3) return KMAHIP_EINVAL;
	memcpy(out3, g_expand_ms, sizeof g_expand_ms);
	return KMAHIP_OK;
}

extern "C" int kmahip_index_build(const char *const *fasta_paths, int n_files, const char *out_prefix, int kmersize) {
	return index_build(fasta_paths, n_files, nullptr, 0, out_prefix, kmersize);
}

extern "C" int kmahip_index_build_decon(const char *const *fasta_paths, int n_files, const char *const *decon_paths, int n_decon,
                                        const char *out_prefix, int kmersize) {
	if(!decon_paths || n_decon <= 0) { kmahip_set_error("decontamination: no contamination file given"); return KMAHIP_EINVAL; }
	for(int i = 0; i < n_decon; ++i)
		if(!decon_paths[i] || !strcmp(decon_paths[i], "--")) { kmahip_set_error("decontamination from standard input (--) is not built: give a file"); return KMAHIP_EINVAL; }
	return index_build(fasta_paths, n_files, decon_paths, n_decon, out_prefix, kmersize);
}
