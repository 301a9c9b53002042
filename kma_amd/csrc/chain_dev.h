// chain_dev.h -- the reference's seed chaining (chainSeeds / chainSeeds_circular, chain.c) and the three DP windows that follow it
// (leadTailAln, the link between two MEMs, trailTailAln; align.c), stated once for the aligners of align.hip and longtrace.hip: the
// chain rule for chain_seeds, the unrolled chain of kma_score_fast and lt_chain; the windows for lt_join (kma_score, kma_score_fast and
// kma_trace keep theirs written out: through these functions their kernels' spill counts move, DESIGN.md "One chaining rule"). Pure
// arithmetic on scalars passed by value -- no state, no memory. A caller keeps where its MEMs live, which DP it calls and what it does
// with the result.
// MEM coordinates are the reference's: template starts and ends 1-based (tS, tE), query 0-based, ends exclusive.
#pragma once
#include "dna_dev.h"

namespace {

// ---- the join: may MEM j follow MEM i, and with what chain score ------------------------------------------------------------------
// The reference walks the successors j left to right and accepts a join either on equality (`score <= g`: the later of equal joins
// wins) or strictly (`score < g`: the first wins); which of the two is a property of the branch.
enum { CJ_NONE = 0, CJ_STRICT = 1, CJ_EQ = 2 };
struct ChainJoin { int g, cls; };

// gap-open + extensions for a gap of n bases, nothing for none
__device__ __forceinline__ int chain_gap(int n, int U, int W1) { return n ? (n - 1) * U + W1 : 0; }

// MEM i: template start and end, query end, weight (covered bases x M). MEM j: its four ends and its chain score.
// chainSeeds, chain.c:79-260. CIRC (-ca, kma.c:722): chainSeeds_circular, chain.c:262-494 -- two more joins, both across the
// template's origin and both accepted strictly, and `<=` for the query-overlap join whose cut start lies behind tEnd (chain.c:412).
template <bool CIRC>
__device__ __forceinline__ ChainJoin chain_join(int tSi, int tEnd, int qEnd, int weight, int tSj, int tEj, int qSj, int qEj, int scj,
                                                int t_len, int k, int M, int MM, int U, int W1) {
	ChainJoin c = {0, CJ_NONE};
	if(qEnd < qSj) {
		if(tEnd < tSj) {
			// j lies behind i on both: a free join, gap + substitutions in between
			const int tGap = tSj - tEnd, qGap = qSj - qEnd;
			c.g = chain_gap(abs(tGap - qGap), U, W1) + weight + scj + mism_score(min(tGap, qGap), k, M, MM);
			c.cls = CJ_EQ;
		} else if(k <= tEj - tEnd) {
			// j overlaps i on the template and keeps a k-mer: the overlap is taken off j
			c.g = chain_gap(qSj - qEnd, U, W1) + weight + scj - (tSj - tEnd) * M;
			c.cls = CJ_STRICT;
		} else if(CIRC && tEj < tSi) {
			// circular join, chain.c:366-394: j ends in front of i, the template gap runs across the origin
			const int tGap = t_len - tEnd + tSj, qGap = qSj - qEnd;
			c.g = chain_gap(abs(tGap - qGap), U, W1) + weight + scj + mism_score(min(tGap, qGap), k, M, MM);
			c.cls = CJ_STRICT;
		}
	} else if(k <= qEj - qEnd) {
		// j overlaps i on the read and keeps a k-mer: its start is cut to qEnd
		int tStart = tSj + qEnd - qSj;
		if(tEnd < tStart) {
			c.g = chain_gap(tStart - tEnd, U, W1) + weight + scj - (tStart - tEnd) * M;
			c.cls = CIRC ? CJ_EQ : CJ_STRICT;        // (chain.c:412)
		} else if(CIRC) {
			// chain.c:416-437: the cut start across the origin
			if(t_len < tStart) tStart -= t_len;
			if(tStart != tEnd && tEj < tStart) {
				c.g = chain_gap(t_len - tEnd + tStart, U, W1) + weight + scj - (tEnd - tStart) * M;
				c.cls = CJ_STRICT;
			}
		}
	}
	return c;
}
// the serial chains' use of the class: does the join beat the running score
__device__ __forceinline__ bool chain_accepts(int score, ChainJoin c) {
	switch(c.cls) { case CJ_EQ: return score <= c.g; case CJ_STRICT: return score < c.g; default: return false; }
}

// ---- the two ends of a chain ----------------------------------------------------------------------------------------------------
// score of a MEM with nothing behind it: what is left of read and template as one gap or as substitutions, whichever is better
__device__ __forceinline__ int chain_tail_score(int weight, int tEnd, int qEnd, int t_len, int q_len, int k, int M, int MM, int U, int W1) {
	const int span = min(t_len - tEnd, q_len - qEnd);
	int gap = span - 1;
	gap = gap ? gap * U + W1 : W1;
	const int sub = mism_score(span, k, M, MM);
	return weight + (sub < gap ? gap : sub);
}
// the addition for the stretch in front of a MEM that starts a chain
__device__ __forceinline__ int chain_head_bonus(int tS, int qS, int k, int M, int MM, int U, int W1) {
	const int span = min(tS, qS);
	int gap = span - 1;
	if(0 < gap) gap = gap * U + W1; else if(gap == 0) gap = W1; else gap = 0;
	const int sub = mism_score(span, k, M, MM);
	return sub < gap ? gap : sub;
}
// best and second best chain start; nxt = the successor of MEM i. True: i is the new best.
__device__ __forceinline__ bool chain_rank(int &best, int &second, int &bestPos, int score, int i, int nxt) {
	if(best <= score) {
		if(nxt != bestPos) second = best;
		best = score; bestPos = i;
		return true;
	}
	if(second <= score && nxt != bestPos) second = best;
	return false;
}

// ---- the three windows -------------------------------------------------------------------------------------------------------------
// t_s / t_e 0-based template window, q_s / q_e query window, t_l template bases (a link across the origin: not t_e - t_s),
// k the mode handed to the DP, dp = there is a problem to solve
constexpr int CHAIN_BW = 64;
struct ChainWin { int t_s, t_e, q_s, q_e, t_l, k; bool dp; };

// band of a problem and whether the full matrix is taken anyway (NW_band_score's test)
__device__ __forceinline__ int dp_band(const ChainWin &w) { return abs(w.t_l - w.q_e + w.q_s) + CHAIN_BW; }
__device__ __forceinline__ bool dp_full(int t_l, int q_l, int band) { return q_l <= band || t_l <= band; }

// leading tail (leadTailAln, align.c:53-131) in front of a MEM that starts at (tS, qS): the longer side is cut to the shorter + band
__device__ __forceinline__ ChainWin lead_window(int tS, int qS) {
	const int bw = CHAIN_BW;
	ChainWin w = {0, tS - 1, 0, qS, 0, 0, false};
	const int t_e = w.t_e, q_e = qS;
	if(q_e) {
		if((q_e << 1) < t_e || (q_e + bw) < t_e) w.t_s = t_e - (q_e + (q_e < bw ? q_e : bw));
		else if((t_e << 1) < q_e || (t_e + bw) < q_e) w.q_s = q_e - (t_e + (t_e < bw ? t_e : bw));
		if(t_e - w.t_s > 0 && q_e - w.q_s > 0) { w.dp = true; w.t_l = t_e - w.t_s; w.k = -1 - (w.t_s == 0); }
	}
	return w;
}
// trailing tail (trailTailAln, align.c:140-212) behind a MEM that ends at (tE, qE)
__device__ __forceinline__ ChainWin trail_window(int tE, int qE, int t_len, int q_len) {
	const int bw = CHAIN_BW;
	const int t_s = tE - 1, q_s = qE;
	ChainWin w = {t_s, t_len, q_s, q_len, 0, 0, false};
	if(((q_len - q_s) << 1) < (t_len - t_s) || (q_len - q_s + bw) < (t_len - t_s)) {
		const int l = q_len - q_s; w.t_e = t_s + (l + (l < bw ? l : bw));
	} else if(((t_len - t_s) << 1) < (q_len - q_s) || (t_len - t_s + bw) < (q_len - q_s)) {
		const int l = t_len - t_s; w.q_e = q_s + (l + (l < bw ? l : bw));
	}
	if(w.t_e - t_s > 0 && w.q_e - q_s > 0) { w.dp = true; w.t_l = w.t_e - t_s; w.k = 1 + (w.t_e == t_len); }
	return w;
}
// link (KMA_score align.c:640-735, KMA :430-466) from the end (tEa, qEa) of MEM a to MEM b, which gives way where the two overlap:
// (tSn, qSn) is b's clipped start (w.q_e == qSn), reject the test of align.c:715
struct ChainLink { ChainWin w; int tSn, qSn; bool reject; };
__device__ __forceinline__ ChainLink link_window(int tEa, int qEa, int tSb, int tEb, int qSb, int t_len, int q_len, int U, int M) {
	const int q_s = qEa, t_s = tEa - 1;
	int qSn = qSb, tSn = tSb;
	if(qSn < q_s) { tSn += q_s - qSn; qSn = q_s; }
	int t_e = tSn - 1, t_l;
	if(t_e < t_s) {
		if(t_s <= tEb) { qSn += t_s - t_e; t_e = t_s; t_l = 0; }
		else t_l = t_len - t_s + t_e;
	} else t_l = t_e - t_s;
	const int q_e = qSn;
	ChainLink l;
	l.w.t_s = t_s; l.w.t_e = t_e; l.w.q_s = q_s; l.w.q_e = q_e; l.w.t_l = t_l; l.w.k = 0;
	l.tSn = tSn; l.qSn = qSn;
	l.reject = abs(t_l - q_e + q_s) * U > q_len * M || t_l > q_len || q_e - q_s > (q_len >> 1);
	l.w.dp = t_l > 0 || q_e - q_s > 0;
	return l;
}

} // namespace
