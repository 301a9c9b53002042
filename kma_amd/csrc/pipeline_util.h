// pipeline_util.h -- what the one-call runs (pipeline.hip) and the batched session (session.hip) share: device buffers carved out
// of slabs, the workspace's status word, an exclusive scan, the seed capacity that grows on demand.
#pragma once
#include "kmahip_internal.h"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <rocprim/rocprim.hpp>
#include <thread>
#include <vector>

// The large device blocks of a run, kept for the next one (pipeline.hip). A hipMalloc of gigabytes is 0.2 ms as a rule and 0.6-1.4 s now
// and then (tools/malloc_probe.py: one in five of 13 GB) -- the run pool of a million long reads is 13 GB, the reads 2.5 GB, and a run that
// asked for them anew each time took twice as long whenever the driver had to find the memory again.
void *kmahip_devcache_take(size_t bytes, size_t *got);      // a kept block of at least `bytes` (and not over twice that), or NULL
void kmahip_devcache_give(void *p, size_t bytes);           // keep it (or release it, when what is kept would exceed the cache's share)
void kmahip_devcache_flush();                               // release everything kept
// stage 3a of a single-end batch: kmahip_launch_align_se, or under -mem_mode (kmahip_set_mem_mode) the records of runKMA_MEM
int kmahip_stage3a_se(kmahip_db *db, kmahip_ws *ws, const kmahip_reads *reads, const kmahip_cands *cands, const kmahip_params *p, kmahip_hits *out, hipStream_t stream);
int kmahip_mem_mode();

namespace {

// Device buffers of one run, carved out of a few large allocations (a hipMalloc per array cost more than ConClave itself:
// thirty of them per run). When the run ends the small ones are released, the large ones kept for the next run.
struct DevBlock {
	std::vector<std::pair<void *, size_t>> owned;
	char *slab = nullptr;
	size_t slab_left = 0, slab_bytes = 256u << 20;
	~DevBlock() {
		// (hipFree waits for the device before it releases; a block that is kept must not be handed on before that either)
		bool any = false;
		for(auto &b : owned) any = any || b.second >= (64u << 20);
		if(any) (void) hipDeviceSynchronize();
		for(auto &b : owned) { if(b.second >= (64u << 20)) kmahip_devcache_give(b.first, b.second); else (void) hipFree(b.first); }
	}
	void expect(size_t bytes) { slab_bytes = std::max(slab_bytes, bytes); }
	static void *alloc(size_t want, size_t *got) {
		void *d = want >= (64u << 20) ? kmahip_devcache_take(want, got) : nullptr;
		if(d) return d;
		*got = want;
		if(hipMalloc(&d, want) == hipSuccess) return d;
		kmahip_devcache_flush();          // (what is kept may be what is missing)
		return hipMalloc(&d, want) == hipSuccess ? d : nullptr;
	}
	template <class T> int get(size_t n, T **dst, bool zero = false) {
		const size_t bytes = (((n ? n : 1) * sizeof(T)) + 255) & ~(size_t) 255;
		if(bytes > slab_left) {
			const size_t want = std::max(bytes, slab_bytes);
			size_t got = 0;
			void *d = alloc(want, &got);
			if(!d) {
				// (a smaller slab may still fit)
				if(want == bytes || !(d = alloc(bytes, &got))) { kmahip_set_error("hipMalloc of %zu bytes failed", bytes); return KMAHIP_ENOMEM; }
				owned.push_back({d, got});
				if(zero && hipMemsetAsync(d, 0, bytes, 0) != hipSuccess) { kmahip_set_error("hipMemset failed"); return KMAHIP_EDEVICE; }
				*dst = (T *) d;
				return KMAHIP_OK;
			}
			owned.push_back({d, got});
			slab = (char *) d; slab_left = got;
		}
		void *d = slab;
		slab += bytes; slab_left -= bytes;
		if(zero && hipMemsetAsync(d, 0, bytes, 0) != hipSuccess) { kmahip_set_error("hipMemset failed"); return KMAHIP_EDEVICE; }
		*dst = (T *) d;
		return KMAHIP_OK;
	}
	template <class T> int up(const T *src, size_t n, size_t pad, const T **dst) {
		T *d = nullptr;
		int rc = get(n + pad, &d);
		if(rc) return rc;
		if(pad && hipMemsetAsync(d + n, 0, pad * sizeof(T), 0) != hipSuccess) { kmahip_set_error("hipMemset failed"); return KMAHIP_EDEVICE; }
		if(n && hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { kmahip_set_error("hipMemcpy failed"); return KMAHIP_EDEVICE; }
		*dst = d;
		return KMAHIP_OK;
	}
};

double since(std::chrono::steady_clock::time_point &t) {
	const auto now = std::chrono::steady_clock::now();
	const double ms = std::chrono::duration<double, std::milli>(now - t).count();
	t = now;
	return ms;
}

// Host buffers for the per-read / per-fragment columns a run brings back: fresh from malloc their pages do not exist yet, and a copy
// that has to fault them in one by one runs at half speed. A thread writes every page once (an atomic OR of zero: it changes nothing,
// whatever has been copied there already) while the device is busy with the stages before the copy.
struct HostCols {
	std::vector<std::pair<char *, size_t>> bufs;
	std::thread th;
	template <class T> T *get(size_t n) {
		T *p = (T *) malloc((n ? n : 1) * sizeof(T));
		if(p) bufs.push_back({(char *) p, n * sizeof(T)});
		return p;
	}
	void start() {
		th = std::thread([this] { for(auto &b : bufs) for(size_t i = 0; i < b.second; i += 4096) __atomic_fetch_or(&b.first[i], 0, __ATOMIC_RELAXED); });
	}
	void wait() { if(th.joinable()) th.join(); }
	~HostCols() { wait(); for(auto &b : bufs) free(b.first); }
};

// status word of the workspace after a synchronised stage (KmaStatus, kmahip_internal.h), read and cleared, and the first counter
// (the pool / run top)
int ws_status(kmahip_ws *ws, unsigned long long *st, unsigned long long *c0) {
	unsigned long long c[2] = {0, 0};
	if(ws->counters) HIP_TRY(hipMemcpy(c, ws->counters, sizeof c, hipMemcpyDeviceToHost));          // (none yet: nothing has been launched)
	if(c[1]) HIP_TRY(hipMemset(ws->counters + 1, 0, sizeof(unsigned long long)));
	if(c0) *c0 = c[0];
	*st = c[1];
	return KMAHIP_OK;
}

// a read full of repeats can carry more MEMs against a template than the scratch holds slots for (64 for reads up to 1 kb;
// KMAHIP_ST_SEED_MEMS from stage 3a, KMAHIP_ST_TRACE_MEMS from the traceback): the capacity goes up fourfold and the stage is run again
bool grow_mem_cap(kmahip_ws *ws) {
	const int cur = ws->mem_scale > 0 ? ws->mem_scale : 1;
	if(cur >= 64) return false;
	ws->mem_scale = cur * 4;
	if(getenv("KMAHIP_DEBUG_TIMING")) fprintf(stderr, "[kmahip] seed (MEM) capacity per read and template raised to %d x the usual\n", ws->mem_scale);
	return true;
}

// KMAHIP_ST_POOL: the library's candidate pool (cap_reads x ints per read x pool_scale) doubles with the next scan launch
void grow_pool(kmahip_ws *ws) {
	ws->pool_scale *= 2; ws->cap_reads = 0;
	if(getenv("KMAHIP_DEBUG_TIMING")) fprintf(stderr, "[kmahip] candidate pool raised to %lld x its usual size\n", (long long) ws->pool_scale);
}

// ---- the three capacities a run cannot know in advance. Each helper launches, synchronises, reads the status word and repeats with
// more room: `launch` is the call site's launch (it returns a KMAHIP_* code), `alloc(cap)` makes room for `cap` entries and points
// the launch's arguments at it. The bounds are the same on every run path: four pool doublings, six list regrows, three run-pool
// regrows; MEM capacity up to 64 x (grow_mem_cap). KMAHIP_CAP_START=<n> replaces the starting guess of the lists and of the run pool
// (for the tests: the regrows at test size).
int64_t cap_start(int64_t guess) {
	const char *e = getenv("KMAHIP_CAP_START");
	return e ? std::max<int64_t>(1, atoll(e)) : guess;
}
void cap_note(const char *what, int64_t cap) {
	if(getenv("KMAHIP_DEBUG_TIMING")) fprintf(stderr, "[kmahip] %s raised to %lld entries\n", what, (long long) cap);
}

// candidate lists of stage 2: `start` entries, then what the scan says it needs (d_total: the last offset, on the device) + slack
template <class Alloc, class Launch>
int retry_cand_room(kmahip_ws *ws, hipStream_t s, int64_t start, int64_t slack, const int64_t *d_total, int64_t *total, Alloc alloc, Launch launch) {
	int64_t cap = cap_start(start);
	for(int doubled = 0, regrown = 0;;) {
		int rc;
		unsigned long long st = 0;
		if((rc = alloc(cap)) || (rc = launch())) return rc;
		HIP_TRY(hipStreamSynchronize(s));
		if((rc = ws_status(ws, &st, nullptr))) return rc;
		if(st == KMAHIP_ST_POOL) {
			if(doubled++ >= 4) { kmahip_set_error("internal candidate pool exhausted"); return KMAHIP_EOVERFLOW; }
			grow_pool(ws);
			continue;
		}
		HIP_TRY(hipMemcpy(total, d_total, sizeof *total, hipMemcpyDeviceToHost));
		if(*total <= cap) return KMAHIP_OK;
		if(regrown++ >= 6) { kmahip_set_error("candidate lists keep growing"); return KMAHIP_EOVERFLOW; }
		cap = *total + slack;
		cap_note("candidate lists", cap);
	}
}

// seed (MEM) room of stage 3a: the launch adds into the score vectors, so they are zeroed before every launch (`bytes` each; v1 may be NULL)
template <class Launch>
int retry_seed_room(kmahip_ws *ws, hipStream_t s, uint64_t *v0, uint64_t *v1, size_t bytes, Launch launch) {
	for(;;) {
		int rc;
		unsigned long long st = 0;
		HIP_TRY(hipMemsetAsync(v0, 0, bytes, s));
		if(v1) HIP_TRY(hipMemsetAsync(v1, 0, bytes, s));
		if((rc = launch())) return rc;
		HIP_TRY(hipStreamSynchronize(s));
		if((rc = ws_status(ws, &st, nullptr))) return rc;
		if(st != KMAHIP_ST_SEED_MEMS) return KMAHIP_OK;
		if(!grow_mem_cap(ws)) { kmahip_set_error("seed (MEM) capacity per read/template pair exceeded"); return KMAHIP_EOVERFLOW; }
	}
}

// run pool of a traceback: `start` runs, then what the kernels say they used + slack. mems: the launch can report KMAHIP_ST_TRACE_MEMS
// (kmahip_launch_trace; kmahip_launch_longtrace grows its MEM arrays itself), which costs no attempt
template <class Alloc, class Launch>
int retry_run_room(kmahip_ws *ws, hipStream_t s, int64_t start, int64_t slack, bool mems, unsigned long long *used, Alloc alloc, Launch launch) {
	int64_t cap = cap_start(start);
	for(int regrown = 0;;) {
		int rc;
		unsigned long long st = 0;
		if((rc = alloc(&cap)) || (rc = launch())) return rc;
		HIP_TRY(hipStreamSynchronize(s));
		if((rc = ws_status(ws, &st, used))) return rc;
		if(st == KMAHIP_ST_CALLER_CAP || (int64_t) *used > cap) {
			if(regrown++ >= 3) { kmahip_set_error("alignment run pool: %llu runs needed", *used); return KMAHIP_EOVERFLOW; }
			cap = (int64_t) *used + slack;
			cap_note("alignment run pool", cap);
			continue;
		}
		if(mems && st == KMAHIP_ST_TRACE_MEMS && grow_mem_cap(ws)) continue;
		if(st) { kmahip_set_error("trace stage: a read needs more scratch than the workspace holds (status %llu)", st); return KMAHIP_EDEVICE; }
		return KMAHIP_OK;
	}
}


int scan_i64(DevBlock &B, const int64_t *in, int64_t *out, size_t n, hipStream_t s) {
	size_t tmp_bytes = 0;
	if(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, (int64_t) 0, n, rocprim::plus<int64_t>(), s) != hipSuccess) {
		kmahip_set_error("rocprim::exclusive_scan (size query) failed"); return KMAHIP_EDEVICE;
	}
	char *tmp = nullptr;
	int rc = B.get(tmp_bytes, &tmp);
	if(rc) return rc;
	if(rocprim::exclusive_scan(tmp, tmp_bytes, in, out, (int64_t) 0, n, rocprim::plus<int64_t>(), s) != hipSuccess) {
		kmahip_set_error("rocprim::exclusive_scan failed"); return KMAHIP_EDEVICE;
	}
	return KMAHIP_OK;
}

// retry_run_room's `alloc` for a run pool that lives in a block
auto run_pool_in(DevBlock &B, kmahip_traces &tr) {
	return [&B, &tr](int64_t *cap) { tr.ops_cap = *cap; return B.get((size_t) *cap, &tr.ops); };
}

// a host batch's five read arrays in a block, padded the way the kernels read them (two words behind the bases, one entry behind the
// lengths and the N positions); *d is the batch with DEVICE arrays, without query bounds
int upload_reads(DevBlock &B, const kmahip_reads &reads, kmahip_reads *d) {
	const size_t n = (size_t) reads.n_reads;
	int rc;
	*d = reads;
	d->q_start = nullptr; d->q_end = nullptr;       // (host pointers, if any: the entry points that upload map whole reads)
	if((rc = B.up(reads.seq, (size_t) reads.seq_words, 2, &d->seq)) || (rc = B.up(reads.seq_off, n + 1, 0, &d->seq_off)) || (rc = B.up(reads.len, n, 1, &d->len)) ||
	   (rc = B.up(reads.N, (size_t) reads.N_total, 1, &d->N)) || (rc = B.up(reads.N_off, n + 1, 0, &d->N_off))) return rc;
	return KMAHIP_OK;
}

// stage 3a's outputs for n reads whose lists hold `total` entries: get(count, &array) makes a zeroed array (the two score vectors
// are the caller's)
template <class Get> int carve_hits(size_t n, size_t total, kmahip_hits *h, Get get) {
	int rc;
	for(int32_t **p : {&h->n_hits, &h->best_score, &h->flag, &h->rc}) if((rc = get(n + 1, p))) return rc;
	for(int32_t **p : {&h->tmpl, &h->score, &h->start, &h->end}) if((rc = get(total + 1, p))) return rc;
	return KMAHIP_OK;
}

}  // namespace
