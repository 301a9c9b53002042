// samout.hip -- the SAM records of a run (`-sam [n]`; saminit / samwrite / makeCigar, sam.c:30-211), made where the data is: the reads, their
// headers, the traceback's figures and alignment runs are in HBM when a run ends, and a long read's CIGAR is thousands of runs.
//   sam_class_kernel   which record class an item falls in (kmahip.h: 1, 2, 3a - 3d, or none) and its sort key: class 1 in stream order,
//                      class 2 in stream order, class 3 by template and, inside a template, in the order assemble_KMA meets the filed
//                      fragments (conclave.c:164-166, 194: the key of the fragment rows, over ALL filed fragments)
//   sam_len_kernel     the width of a row: header up to its first TAB, decimal widths, names, bases, CIGAR text
//   sam_format_kernel  the text. Both take a group of G lanes per row: G = 1 for short reads, G = 64 (a wavefront) for long ones, where a
//                      shuffle prefix sum over the widths of the runs' texts gives each lane its place and the bases go out four per store
// rocPRIM sorts and scans; the text comes back a chunk at a time through pinned buffers and is written in order while the next chunk is made.
// kmahip_sam_cigar / kmahip_sam_row_host state the same row in host code: the checkers of the device's text.
#include "pipeline_util.h"
#include <cerrno>
#include <fcntl.h>
#include <unistd.h>

namespace {

enum { SC_NONE = 0, SC_S2 = 1, SC_S3A = 2, SC_KEPT = 3, SC_DROP = 4, SC_UNAL = 5 };

struct SamArgs {
	const uint64_t *seq;
	const int64_t *seq_off, *N_off, *name_off, *name_idx;
	const int32_t *len, *N, *rc, *tmpl, *n_hits, *flag, *stats;
	const int64_t *ops_off;
	const int32_t *n_ops;
	const uint32_t *ops;
	const int32_t *d_stats;          // the drop record (or NULL)
	const int64_t *d_ops_off;
	const int32_t *d_n_ops;
	const uint8_t *ok;
	const char *names, *tnames;
	const int64_t *tname_off;
	const uint8_t *cls;
	const int64_t *row_item;
	int64_t *row_off;
};

__global__ __launch_bounds__(256) void sam_filed_kernel(int64_t n, const int32_t *tmpl, int64_t *filed) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(i <= n) filed[i] = i < n && tmpl[i] != 0;
}

// class and key of every item; counts[c - 1] = items of class c (one atomic per wavefront and class)
__global__ __launch_bounds__(256) void sam_class_kernel(int64_t n, const SamArgs A, const int64_t *rank, int64_t max_frag, int order, int level, uint8_t *cls,
                                                        unsigned long long *keys, int64_t *vals, unsigned long long *counts) {
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	int c = SC_NONE;
	if(i < n) {
		const int tt = A.tmpl[i];
		if(tt == 0) {
			if(level == 1) c = (A.flag[i] & 4) ? SC_S3A : (A.n_hits[i] == 0 ? SC_S2 : SC_NONE);
		} else {
			const int t = abs(tt);
			if(A.stats[10 * i + 3] != 0) c = SC_KEPT;
			else if(!(level & 2096)) c = ((!A.ok || A.ok[t]) && A.d_stats && A.d_stats[6 * i] != 0) ? SC_DROP : SC_UNAL;
		}
		unsigned long long key = ~0ull;
		if(c == SC_S2) key = (unsigned long long) i;
		else if(c == SC_S3A) key = (1ull << 62) | (unsigned long long) i;
		else if(c != SC_NONE) {
			const unsigned long long rk = (unsigned long long) rank[i], mf = (unsigned long long) max_frag;
			const unsigned long long in = order == 1 ? rk : (rk / mf) * mf + (mf - 1ull - rk % mf);
			key = (2ull << 62) | ((unsigned long long) abs(tt) << 40) | in;
		}
		cls[i] = (uint8_t) c; keys[i] = key; vals[i] = i;
	}
	for(int x = SC_S2; x <= SC_UNAL; ++x) {
		const unsigned long long m = __ballot(c == x);
		if(m && (threadIdx.x & 63) == 0) atomicAdd(&counts[x - 1], (unsigned long long) __popcll(m));
	}
}

__device__ __forceinline__ int sam_udigits(unsigned u) {
	int d = 1;
	while(u >= 10u) { u /= 10u; ++d; }
	return d;
}
__device__ __forceinline__ int sam_digits(int v) { return v < 0 ? 1 + sam_udigits(0u - (unsigned) v) : sam_udigits((unsigned) v); }
// decimal text without a buffer of its own: the digits are written back to front into their place
__device__ __forceinline__ char *sam_put_uint(char *o, unsigned u) {
	const int nd = sam_udigits(u);
	for(int k = nd - 1; k >= 0; --k) { o[k] = (char) ('0' + u % 10u); u /= 10u; }
	return o + nd;
}
__device__ __forceinline__ char *sam_put_int(char *o, int v) {
	if(v < 0) { *o++ = '-'; return sam_put_uint(o, 0u - (unsigned) v); }
	return sam_put_uint(o, (unsigned) v);
}
__device__ __forceinline__ char *sam_put_str(char *o, const char *s, int n) {
	for(int x = 0; x < n; ++x) o[x] = s[x];
	return o + n;
}

// what a row prints, by class (samwrite, sam.c:160-182; assembly.c:1987-2015; alnfrags.c:2262-2273; savekmers.c:205-225)
struct SamRow {
	int flag, pos, mapq, tlen, et, as, cs, ce, n_ops, t;
	bool flip, star;
	const uint32_t *ops;
};
__device__ __forceinline__ SamRow sam_row(const SamArgs &A, int64_t i, int c) {
	SamRow R;
	const int tt = A.tmpl[i];
	R.t = c >= SC_KEPT ? abs(tt) : 0;
	R.pos = 0; R.mapq = 0; R.tlen = 0; R.et = 0; R.as = 0; R.cs = 0; R.ce = 0; R.n_ops = 0; R.ops = nullptr; R.star = true;
	if(c == SC_S2) { R.flag = 20; R.flip = false; return R; }
	if(c == SC_S3A) { R.flag = A.flag[i]; R.flip = (A.rc[i] & 1) != 0; return R; }
	R.flag = A.flag[i] | (tt < 0 ? 16 : 0);
	R.flip = ((A.rc[i] & 1) != 0) != (tt < 0);
	R.et = A.n_hits[i];
	if(c == SC_UNAL) { R.flag |= 4; return R; }
	R.star = false;
	unsigned mq;
	if(c == SC_KEPT) {
		const int32_t *st = A.stats + 10 * i;
		R.as = st[0]; R.pos = st[1] + 1; R.tlen = st[2] - R.pos; R.cs = st[4]; R.ce = st[5]; mq = (unsigned) st[9];
		R.ops = A.ops + A.ops_off[i]; R.n_ops = A.n_ops[i];
	} else {
		const int32_t *st = A.d_stats + 6 * i;
		R.as = st[0]; R.pos = st[1] + 1; R.tlen = st[2] - R.pos; R.cs = st[3]; R.ce = st[4]; mq = (unsigned) st[5];
		R.ops = A.ops + A.d_ops_off[i]; R.n_ops = A.d_n_ops[i];
	}
	R.mapq = mq > 254u ? 254 : (int) mq;
	return R;
}
// QNAME: the header up to its first TAB (samwrite cuts it there, sam.c:183-195)
__device__ __forceinline__ int sam_qname_len(const char *h, int n) {
	int x = 0;
	while(x < n && h[x] != '\t') ++x;
	return x;
}
template <int G> __device__ __forceinline__ int group_sum(int v) {
	if(G > 1) for(int d = G >> 1; d > 0; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// 12 TABs, RNEXT "*", PNEXT "0", QUAL "*", "ET:i:", "AS:i:", the newline
#define SAM_FIXED 26

template <int G>
__global__ __launch_bounds__(256) void sam_len_kernel(const SamArgs A, int64_t n_rows) {
	const int64_t r = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) / G;
	const int lane = (int) (threadIdx.x % G);
	if(r > n_rows) return;
	if(r == n_rows) { if(lane == 0) A.row_off[r] = 0; return; }
	const int64_t i = A.row_item[r];
	const SamRow R = sam_row(A, i, A.cls[i]);
	int cig = 0;
	for(int k = lane; k < R.n_ops; k += G) cig += sam_udigits(R.ops[k] >> 2) + 1;
	cig = group_sum<G>(cig);
	if(lane) return;
	if(R.star) cig = 1;
	else cig += (R.cs ? sam_digits(R.cs) + 1 : 0) + (R.ce ? sam_digits(R.ce) + 1 : 0);
	const int64_t ni = A.name_idx ? A.name_idx[i] : i;
	const int qn = sam_qname_len(A.names + A.name_off[ni], (int) (A.name_off[ni + 1] - A.name_off[ni] - 1));
	const int rn = R.t ? (int) (A.tname_off[R.t] - A.tname_off[R.t - 1]) : 1;
	A.row_off[r] = (int64_t) qn + sam_digits(R.flag) + rn + sam_digits(R.pos) + sam_digits(R.mapq) + cig + sam_digits(R.tlen) + A.len[i] + sam_digits(R.et) +
	               sam_digits(R.as) + SAM_FIXED;
}

// G lanes per row. Lane 0 writes the fields in front of the CIGAR; every lane takes every G-th run, its place from a prefix sum over the
// widths of the runs' texts; the field between CIGAR and SEQ, the bases (four per 32-bit store, then the N's) and the tags follow.
template <int G>
__global__ __launch_bounds__(256) void sam_format_kernel(const SamArgs A, int64_t r0, int64_t r1, int64_t text_base, char *text) {
	const int64_t r = r0 + ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) / G;
	const int lane = (int) (threadIdx.x % G);
	if(r >= r1) return;
	const int64_t i = A.row_item[r];
	const SamRow R = sam_row(A, i, A.cls[i]);
	char *p = text + (A.row_off[r] - text_base);
	const int64_t ni = A.name_idx ? A.name_idx[i] : i;
	const char *hd = A.names + A.name_off[ni];
	const int qn = sam_qname_len(hd, (int) (A.name_off[ni + 1] - A.name_off[ni] - 1));
	const int rn = R.t ? (int) (A.tname_off[R.t] - A.tname_off[R.t - 1]) : 1;
	if(lane == 0) {
		char *o = sam_put_str(p, hd, qn);
		*o++ = '\t'; o = sam_put_int(o, R.flag);
		*o++ = '\t';
		if(R.t) o = sam_put_str(o, A.tnames + A.tname_off[R.t - 1], rn); else *o++ = '*';
		*o++ = '\t'; o = sam_put_int(o, R.pos);
		*o++ = '\t'; o = sam_put_int(o, R.mapq);
		*o++ = '\t';
	}
	p += qn + sam_digits(R.flag) + rn + sam_digits(R.pos) + sam_digits(R.mapq) + 5;
	if(R.star) { if(lane == 0) *p = '*'; ++p; }
	else {
		if(R.cs) { if(lane == 0) *sam_put_int(p, R.cs) = 'S'; p += sam_digits(R.cs) + 1; }
		for(int b = 0; b < R.n_ops; b += G) {
			const int k = b + lane;
			const uint32_t e = k < R.n_ops ? R.ops[k] : 0u;
			const int w = k < R.n_ops ? sam_udigits(e >> 2) + 1 : 0;
			int incl = w;
			if(G > 1) for(int d = 1; d < G; d <<= 1) { const int v = __shfl_up(incl, d); if(lane >= d) incl += v; }
			if(w) *sam_put_uint(p + incl - w, e >> 2) = (char) ((0x4449583Du >> (8 * (e & 3u))) & 0xFFu);          // '=' 'X' 'I' 'D', low byte first
			p += G > 1 ? __shfl(incl, G - 1) : incl;
		}
		if(R.ce) { if(lane == 0) *sam_put_int(p, R.ce) = 'S'; p += sam_digits(R.ce) + 1; }
	}
	if(lane == (G > 1 ? 1 : 0)) {
		char *o = p;
		*o++ = '\t'; *o++ = '*'; *o++ = '\t'; *o++ = '0'; *o++ = '\t';
		o = sam_put_int(o, R.tlen);
		*o++ = '\t';
	}
	p += 6 + sam_digits(R.tlen);
	const int L = A.len[i];
	const uint64_t *w = A.seq + A.seq_off[i];
	const bool flip = R.flip;
	const uint32_t lut = 0x54474341u;          // 'A' 'C' 'G' 'T', low byte first
	for(int b = 4 * lane; b < L; b += 4 * G) {
		uint32_t four = 0;
#pragma unroll
		for(int x = 0; x < 4; ++x) {
			const int pos = b + x;
			int code = 0;
			if(pos < L) {
				const int src = flip ? L - 1 - pos : pos;
				code = (int) ((w[src >> 5] >> (62 - ((src & 31) << 1))) & 3ull);
				if(flip) code = 3 - code;
			}
			four |= ((lut >> (8 * code)) & 0xFFu) << (8 * x);
		}
		if(b + 4 <= L) memcpy(p + b, &four, 4);          // (unaligned: rows begin anywhere)
		else for(int x = 0; b + x < L; ++x) p[b + x] = (char) ((four >> (8 * x)) & 0xFFu);
	}
	// (the N's overwrite bases that another lane of the group may have stored: those stores first)
	if(G > 1) __threadfence();
	const int32_t *Np = A.N + A.N_off[i];
	const int nN = (int) (A.N_off[i + 1] - A.N_off[i]);
	for(int x = lane; x < nN; x += G) p[flip ? L - 1 - Np[x] : Np[x]] = 'N';
	p += L;
	if(lane == (G > 1 ? 2 : 0)) {
		char *o = p;
		*o++ = '\t'; *o++ = '*'; *o++ = '\t'; *o++ = 'E'; *o++ = 'T'; *o++ = ':'; *o++ = 'i'; *o++ = ':';
		o = sam_put_int(o, R.et);
		*o++ = '\t'; *o++ = 'A'; *o++ = 'S'; *o++ = ':'; *o++ = 'i'; *o++ = ':';
		o = sam_put_int(o, R.as);
		*o++ = '\n';
	}
}

__global__ __launch_bounds__(256) void sam_blocks_kernel(int64_t n_blocks, int64_t rows_per_block, int64_t n_rows, const int64_t *row_off, int64_t *block_off) {
	const int64_t b = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(b <= n_blocks) block_off[b] = row_off[b * rows_per_block < n_rows ? b * rows_per_block : n_rows];
}

int write_all(int fd, const char *p, size_t n) {
	while(n) {
		const ssize_t w = write(fd, p, n);
		if(w < 0) { if(errno == EINTR) continue; kmahip_set_error("writing the SAM records failed: %s", strerror(errno)); return KMAHIP_EIO; }
		p += w; n -= (size_t) w;
	}
	return KMAHIP_OK;
}

}  // namespace

int kmahip_sam_open(const char *path, bool append) {
	if(!strcmp(path, "-")) return STDOUT_FILENO;
	const int fd = open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0644);
	if(fd < 0) kmahip_set_error("cannot open %s: %s", path, strerror(errno));
	return fd;
}
int kmahip_sam_close(int fd) {
	if(fd < 0 || fd == STDOUT_FILENO) return KMAHIP_OK;
	if(close(fd)) { kmahip_set_error("closing the SAM file failed: %s", strerror(errno)); return KMAHIP_EIO; }
	return KMAHIP_OK;
}

int kmahip_sam_write_dev(kmahip_db *db, const KmaSamIn *in, int fd, int64_t text_chunk, char **pinned, int64_t *rows_out, int64_t class_rows[5]) {
	const kmahip_reads *W = in->W;
	const int64_t n = W->n_reads;
	const size_t D = db->info.DB_size;
	const int64_t mf = in->max_frag > 0 ? in->max_frag : 1000000;
	hipStream_t s = 0;
	int rc;
	auto t = std::chrono::steady_clock::now();
	if(rows_out) *rows_out = 0;
	if(class_rows) for(int x = 0; x < 5; ++x) class_rows[x] = 0;
	if(n <= 0) return KMAHIP_OK;
	if(D > ((size_t) 1 << 22)) { kmahip_set_error("SAM rows: more than 2^22 templates do not fit the sort key"); return KMAHIP_EINVAL; }
	if((rc = kmahip_db_load_names(db))) return rc;
	if(text_chunk <= 0) text_chunk = getenv("KMAHIP_SAM_CHUNK") ? std::max<int64_t>(64, atoll(getenv("KMAHIP_SAM_CHUNK"))) : (64ll << 20);
	DevBlock B;
	B.expect((size_t) n * 56 + (64u << 20));
	uint8_t *cls = nullptr;
	int64_t *filed = nullptr, *frank = nullptr, *vals = nullptr, *vals2 = nullptr, *row_len = nullptr, *row_off = nullptr;
	unsigned long long *keys = nullptr, *keys2 = nullptr, *counts = nullptr;
	if((rc = B.get((size_t) n + 1, &cls)) || (rc = B.get((size_t) n + 1, &keys)) || (rc = B.get((size_t) n + 1, &keys2)) || (rc = B.get((size_t) n + 1, &vals)) ||
	   (rc = B.get((size_t) n + 1, &vals2)) || (rc = B.get(8, &counts))) return rc;
	HIP_TRY(hipMemsetAsync(counts, 0, 64, s));
	const int64_t *use_rank = in->d_rank;
	if(!use_rank) {
		if((rc = B.get((size_t) n + 1, &filed)) || (rc = B.get((size_t) n + 1, &frank))) return rc;
		hipLaunchKernelGGL(sam_filed_kernel, dim3((unsigned) ((n + 256) / 256)), dim3(256), 0, s, n, in->d_tmpl, filed);
		HIP_TRY(hipGetLastError());
		if((rc = scan_i64(B, filed, frank, (size_t) n + 1, s))) return rc;
		use_rank = frank;
	}
	SamArgs A{};
	A.seq = W->seq; A.seq_off = W->seq_off; A.N_off = W->N_off; A.name_off = in->d_name_off; A.name_idx = in->d_name_idx; A.len = W->len; A.N = W->N;
	A.rc = in->d_rc; A.tmpl = in->d_tmpl; A.n_hits = in->d_nhits; A.flag = in->d_flag; A.stats = in->tr->stats; A.ops_off = in->tr->ops_off; A.n_ops = in->tr->n_ops;
	A.ops = in->tr->ops;
	if(in->drops && in->drops->stats) { A.d_stats = in->drops->stats; A.d_ops_off = in->drops->ops_off; A.d_n_ops = in->drops->n_ops; }
	A.ok = in->d_ok; A.names = in->d_names; A.cls = cls;
	hipLaunchKernelGGL(sam_class_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, n, A, use_rank, mf, in->order, in->level, cls, keys, vals, counts);
	HIP_TRY(hipGetLastError());
	unsigned long long h_counts[5] = {0, 0, 0, 0, 0};
	HIP_TRY(hipMemcpyAsync(h_counts, counts, sizeof h_counts, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	int64_t n_rows = 0;
	for(int x = 0; x < 5; ++x) { n_rows += (int64_t) h_counts[x]; if(class_rows) class_rows[x] = (int64_t) h_counts[x]; }
	if(rows_out) *rows_out = n_rows;
	if(n_rows == 0) return KMAHIP_OK;
	{
		size_t tmp_bytes = 0;
		if(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys2, vals, vals2, (size_t) n, 0, 64, s) != hipSuccess) { kmahip_set_error("rocprim::radix_sort_pairs (size query) failed"); return KMAHIP_EDEVICE; }
		char *tmp = nullptr;
		if((rc = B.get(tmp_bytes, &tmp))) return rc;
		if(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys2, vals, vals2, (size_t) n, 0, 64, s) != hipSuccess) { kmahip_set_error("rocprim::radix_sort_pairs failed"); return KMAHIP_EDEVICE; }
	}
	{	// template names on the device
		std::vector<int64_t> tn_off(D + 1, 0);
		std::string tn;
		for(size_t tt = 1; tt < D; ++tt) { if(tt - 1 < db->h_names.size()) tn += db->h_names[tt - 1]; tn_off[tt] = (int64_t) tn.size(); }
		tn_off[D] = (int64_t) tn.size();
		if((rc = B.up(tn.data(), tn.size(), 1, &A.tnames)) || (rc = B.up(tn_off.data(), D + 1, 0, &A.tname_off))) return rc;
	}
	if((rc = B.get((size_t) n_rows + 1, &row_len)) || (rc = B.get((size_t) n_rows + 1, &row_off))) return rc;
	// a lane per row, or a wavefront per row where the reads are long (s1_pack_kernel's choice, by the average length)
	int G = (W->seq_words > 0 ? W->seq_words * 32 / n : W->max_len) >= 512 ? 64 : 1;
	if(getenv("KMAHIP_SAM_GROUP")) G = atoi(getenv("KMAHIP_SAM_GROUP")) == 64 ? 64 : 1;
	A.row_item = vals2; A.row_off = row_len;
	const unsigned g_len = (unsigned) (((n_rows + 1) * G + 255) / 256);
	if(G == 64) hipLaunchKernelGGL(sam_len_kernel<64>, dim3(g_len), dim3(256), 0, s, A, n_rows);
	else hipLaunchKernelGGL(sam_len_kernel<1>, dim3(g_len), dim3(256), 0, s, A, n_rows);
	HIP_TRY(hipGetLastError());
	if((rc = scan_i64(B, row_len, row_off, (size_t) n_rows + 1, s))) return rc;
	A.row_off = row_off;
	int64_t text_bytes = 0;
	HIP_TRY(hipMemcpyAsync(&text_bytes, row_off + n_rows, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	// blocks of rows (a sixteenth of a chunk of text), chunks of whole blocks
	const int64_t avg = std::max<int64_t>(1, text_bytes / n_rows);
	const int64_t rows_per_block = std::max<int64_t>(1, std::min<int64_t>(1 << 16, text_chunk / 16 / avg));
	const int64_t n_blocks = (n_rows + rows_per_block - 1) / rows_per_block;
	int64_t *d_boff = nullptr;
	if((rc = B.get((size_t) n_blocks + 1, &d_boff))) return rc;
	hipLaunchKernelGGL(sam_blocks_kernel, dim3((unsigned) ((n_blocks + 256) / 256)), dim3(256), 0, s, n_blocks, rows_per_block, n_rows, row_off, d_boff);
	HIP_TRY(hipGetLastError());
	std::vector<int64_t> boff((size_t) n_blocks + 1);
	HIP_TRY(hipMemcpyAsync(boff.data(), d_boff, ((size_t) n_blocks + 1) * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	int64_t max_block = 0;
	for(int64_t b = 0; b < n_blocks; ++b) max_block = std::max(max_block, boff[(size_t) b + 1] - boff[(size_t) b]);
	const int64_t CHUNK = std::max<int64_t>(text_chunk, max_block);
	char *d_text[2] = {nullptr, nullptr}, *h_text[2] = {pinned ? pinned[0] : nullptr, pinned ? pinned[1] : nullptr}, *own[2] = {nullptr, nullptr};
	struct Own { char **o; ~Own() { for(int x = 0; x < 2; ++x) if(o[x]) (void) hipHostFree(o[x]); } } own_guard{own};
	for(int x = 0; x < 2; ++x) if((rc = B.get((size_t) CHUNK + 16, &d_text[x]))) return rc;
	if(!pinned || CHUNK > text_chunk) {          // (no buffers of the caller's, or a block of rows longer than they are)
		for(int x = 0; x < 2; ++x) { if(hipHostMalloc((void **) &own[x], (size_t) CHUNK + 16, hipHostMallocDefault) != hipSuccess) { own[x] = nullptr; kmahip_set_error("hipHostMalloc failed"); return KMAHIP_ENOMEM; } h_text[x] = own[x]; }
	}
	const double ms_prep = since(t);
	double ms_wait = 0, ms_write = 0;
	// chunk k is formatted and copied while chunk k - 1 is written
	struct Chunk { int64_t b0, b1; };
	auto next_chunk = [&](int64_t b0) { int64_t b1 = b0 + 1; while(b1 < n_blocks && boff[(size_t) b1 + 1] - boff[(size_t) b0] <= CHUNK) ++b1; return Chunk{b0, b1}; };
	auto launch = [&](const Chunk &c, int k) -> int {
		const int64_t ra = c.b0 * rows_per_block, rb = std::min(n_rows, c.b1 * rows_per_block);
		const unsigned g = (unsigned) (((rb - ra) * G + 255) / 256);
		if(G == 64) hipLaunchKernelGGL(sam_format_kernel<64>, dim3(g), dim3(256), 0, s, A, ra, rb, boff[(size_t) c.b0], d_text[k & 1]);
		else hipLaunchKernelGGL(sam_format_kernel<1>, dim3(g), dim3(256), 0, s, A, ra, rb, boff[(size_t) c.b0], d_text[k & 1]);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(h_text[k & 1], d_text[k & 1], (size_t) (boff[(size_t) c.b1] - boff[(size_t) c.b0]), hipMemcpyDeviceToHost, s));
		return KMAHIP_OK;
	};
	Chunk cur = next_chunk(0);
	int k = 0;
	if((rc = launch(cur, k))) return rc;
	for(;;) {
		HIP_TRY(hipStreamSynchronize(s));
		ms_wait += since(t);
		const Chunk done = cur;
		const int kd = k;
		const bool more = done.b1 < n_blocks;
		if(more) { cur = next_chunk(done.b1); ++k; if((rc = launch(cur, k))) return rc; }
		if((rc = write_all(fd, h_text[kd & 1], (size_t) (boff[(size_t) done.b1] - boff[(size_t) done.b0])))) { (void) hipStreamSynchronize(s); return rc; }
		ms_write += since(t);
		if(!more) break;
	}
	if(getenv("KMAHIP_DEBUG_TIMING"))
		fprintf(stderr, "[kmahip] SAM rows: %lld rows (classes 1, 2, 3a, 3b, 3c+3d: %llu %llu %llu %llu %llu), %lld bytes of text in %d chunks, %d lane(s) per row; classes + order + lengths %.1f ms, "
		                "waiting for the device %.1f, writing %.1f\n", (long long) n_rows, h_counts[0], h_counts[1], h_counts[2], h_counts[3], h_counts[4], (long long) text_bytes, k + 1, G, ms_prep, ms_wait, ms_write);
	return KMAHIP_OK;
}

// ---- the checkers: the same row in host code -------------------------------------------------------------------------------------
extern "C" const char *kmahip_version(void) { return KMAHIP_VERSION; }

extern "C" int64_t kmahip_sam_cigar(const uint32_t *runs, int64_t n, int32_t clip_start, int32_t clip_end, char *out, int64_t cap) {
	if(n < 0 || (n && !runs) || !out || cap < 1) { kmahip_set_error("bad arguments"); return KMAHIP_EINVAL; }
	int64_t len = 0;
	char buf[24];
	auto put = [&](long long v, char c) -> bool {
		const int w = snprintf(buf, sizeof buf, "%lld%c", v, c);
		if(len + w + 1 > cap) return false;
		memcpy(out + len, buf, (size_t) w);
		len += w;
		return true;
	};
	bool ok = true;
	if(clip_start) ok = put(clip_start, 'S');
	for(int64_t x = 0; ok && x < n; ++x) ok = put((long long) (runs[x] >> 2), "=XID"[runs[x] & 3u]);
	if(ok && clip_end) ok = put(clip_end, 'S');
	if(!ok) { kmahip_set_error("kmahip_sam_cigar: %lld bytes do not hold the CIGAR", (long long) cap); return KMAHIP_EOVERFLOW; }
	out[len] = 0;
	return len;
}

extern "C" int64_t kmahip_sam_row_host(const char *header, int32_t flag, const char *rname, int32_t pos, int32_t mapq, const uint32_t *runs, int64_t n_runs,
                                       int32_t clip_start, int32_t clip_end, int32_t tlen, const char *seq, int32_t et, int32_t as, char *out, int64_t cap) {
	if(!header || !seq || !out || cap < 1 || n_runs < 0) { kmahip_set_error("bad arguments"); return KMAHIP_EINVAL; }
	std::string row;
	const char *tab = strchr(header, '\t');
	row.append(header, tab ? (size_t) (tab - header) : strlen(header));
	row += '\t'; row += std::to_string(flag);
	row += '\t'; row += rname ? rname : "*";
	row += '\t'; row += std::to_string(pos);
	row += '\t'; row += std::to_string(mapq > 254 ? 254 : mapq);
	row += '\t';
	if(runs) {
		std::vector<char> cg((size_t) n_runs * 12 + 32);
		const int64_t l = kmahip_sam_cigar(runs, n_runs, clip_start, clip_end, cg.data(), (int64_t) cg.size());
		if(l < 0) return l;
		row.append(cg.data(), (size_t) l);
	} else row += '*';
	row += "\t*\t0\t"; row += std::to_string(tlen);
	row += '\t'; row += seq;
	row += "\t*\tET:i:"; row += std::to_string(et);
	row += "\tAS:i:"; row += std::to_string(as);
	row += '\n';
	if((int64_t) row.size() > cap) { kmahip_set_error("kmahip_sam_row_host: %lld bytes do not hold the row", (long long) cap); return KMAHIP_EOVERFLOW; }
	memcpy(out, row.data(), row.size());
	return (int64_t) row.size();
}

extern "C" int kmahip_sam_header(kmahip_db *db, const char *program, const char *cmdline, const char *path) {
	if(!db || !path) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	int rc;
	if((rc = kmahip_db_load_names(db))) return rc;
	std::string h = "@HD\tVN:1.6\tGO:reference\n@PG\tID:KMA\tPN:";
	h += program ? program : "kmahip";
	h += "\tVN:" KMAHIP_VERSION;
	if(cmdline) { h += "\tCL:"; h += cmdline; }
	h += '\n';
	for(size_t t = 1; t < db->info.DB_size; ++t) {
		h += "@SQ\tSN:";
		if(t - 1 < db->h_names.size()) h += db->h_names[t - 1];
		h += "\tLN:"; h += std::to_string(db->h_tlen[t]); h += '\n';
	}
	const int fd = kmahip_sam_open(path, false);
	if(fd < 0) return KMAHIP_EIO;
	rc = write_all(fd, h.data(), h.size());
	const int rc2 = kmahip_sam_close(fd);
	return rc ? rc : rc2;
}

// host buffers in: everything goes up once, the rows are made as for a session
extern "C" int kmahip_sam_write(const char *path, kmahip_db *db, const kmahip_reads *reads, const int32_t *rc_in, const int32_t *tmpl, const int32_t *n_hits,
                                const int32_t *flag, const kmahip_traces *traces, const kmahip_trace_drops *drops, const uint8_t *tmpl_ok, int64_t max_frag,
                                int order, const int64_t *frag_rank, const char *read_names, const int64_t *read_name_off, int level, int64_t *rows,
                                int64_t class_rows[5]) {
	if(!path || !db || !reads || !rc_in || !tmpl || !n_hits || !flag || !traces || !traces->stats || !traces->ops_off || !traces->n_ops || !read_names || !read_name_off ||
	   (traces->ops_cap > 0 && !traces->ops) || (drops && (!drops->stats || !drops->ops_off || !drops->n_ops))) { kmahip_set_error("null argument"); return KMAHIP_EINVAL; }
	if(level < 1) { kmahip_set_error("kmahip_sam_write: level %d (the value of -sam) must be positive", level); return KMAHIP_EINVAL; }
	const int64_t n = reads->n_reads;
	if(rows) *rows = 0;
	if(class_rows) for(int x = 0; x < 5; ++x) class_rows[x] = 0;
	if(n < 0 || reads->seq_words < 0 || reads->N_total < 0) { kmahip_set_error("negative size"); return KMAHIP_EINVAL; }
	// (every run a record points at lies inside what was given: checked before anything goes up or is opened)
	for(int64_t i = 0; i < n; ++i) {
		if(traces->n_ops[i] < 0 || traces->ops_off[i] < 0 || traces->ops_off[i] + traces->n_ops[i] > traces->ops_cap ||
		   (drops && (drops->n_ops[i] < 0 || drops->ops_off[i] < 0 || drops->ops_off[i] + drops->n_ops[i] > traces->ops_cap))) { kmahip_set_error("kmahip_sam_write: the runs of read %lld lie outside ops_cap", (long long) i); return KMAHIP_EINVAL; }
		if(abs(tmpl[i]) >= (int64_t) db->info.DB_size) { kmahip_set_error("kmahip_sam_write: template %d out of range", tmpl[i]); return KMAHIP_EINVAL; }
	}
	const int fd = kmahip_sam_open(path, true);
	if(fd < 0) return KMAHIP_EIO;
	struct Closer { int fd; ~Closer() { (void) kmahip_sam_close(fd); } } closer{fd};
	if(n == 0) return KMAHIP_OK;
	int rc;
	DevBlock B;
	kmahip_reads W;
	if((rc = upload_reads(B, *reads, &W))) return rc;
	KmaSamIn in{};
	kmahip_traces tr{};
	kmahip_trace_drops dr{};
	const int32_t *c32 = nullptr;
	const int64_t *c64 = nullptr;
	const uint32_t *cu32 = nullptr;
	const uint32_t uzero = 0;
	in.W = &W;
	if((rc = B.up(read_names, (size_t) read_name_off[n], 1, &in.d_names)) || (rc = B.up(read_name_off, (size_t) n + 1, 0, &in.d_name_off)) || (rc = B.up(rc_in, (size_t) n, 1, &in.d_rc)) ||
	   (rc = B.up(tmpl, (size_t) n, 1, &in.d_tmpl)) || (rc = B.up(n_hits, (size_t) n, 1, &in.d_nhits)) || (rc = B.up(flag, (size_t) n, 1, &in.d_flag))) return rc;
	if((rc = B.up(traces->stats, (size_t) n * 10, 10, &c32))) return rc;
	tr.stats = (int32_t *) c32;
	if((rc = B.up(traces->ops_off, (size_t) n, 1, &c64))) return rc;
	tr.ops_off = (int64_t *) c64;
	if((rc = B.up(traces->n_ops, (size_t) n, 1, &c32))) return rc;
	tr.n_ops = (int32_t *) c32;
	if((rc = B.up(traces->ops_cap > 0 ? traces->ops : &uzero, (size_t) std::max<int64_t>(1, traces->ops_cap), 0, &cu32))) return rc;
	tr.ops = (uint32_t *) cu32; tr.ops_cap = traces->ops_cap;
	in.tr = &tr;
	if(drops) {
		if((rc = B.up(drops->stats, (size_t) n * 6, 6, &c32))) return rc;
		dr.stats = (int32_t *) c32;
		if((rc = B.up(drops->ops_off, (size_t) n, 1, &c64))) return rc;
		dr.ops_off = (int64_t *) c64;
		if((rc = B.up(drops->n_ops, (size_t) n, 1, &c32))) return rc;
		dr.n_ops = (int32_t *) c32;
		in.drops = &dr;
	}
	if(tmpl_ok && (rc = B.up(tmpl_ok, (size_t) db->info.DB_size, 8, &in.d_ok))) return rc;
	if(frag_rank && (rc = B.up(frag_rank, (size_t) n, 1, &in.d_rank))) return rc;
	in.max_frag = max_frag; in.order = order; in.level = level;
	return kmahip_sam_write_dev(db, &in, fd, 0, nullptr, rows, class_rows);
}
