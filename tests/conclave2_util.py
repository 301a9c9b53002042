"""ConClave version 2 (`-ConClave 2`: runConClave2 / runConClave2_lc, conclave.c:386-1110) restated in plain Python over explicit frag_raw
records, for the tests of kmahip_conclave2_records and of the whole runs. No test lives here.

A record r of the stream: abs(n_hits[r]) listed templates at off[r] of tmpl / start / end (signed template: negative = the reverse strand),
score[r] (negative: a pair record, two reads), q_len[r] / q_len2[r] (the record's first sequence and its mate), seed[r] (below). A slot
with no template and score 0 is no record. Written from what the reference does, integer widths included:

  pass 1  every record's best-of-list template (a one-template record: that template; an empty list: the first listed template of the
          last record before it that had a list) collects abs(score) in a scratch vector w1
  pass 2  w1[t] is zeroed where template t fails `cmp(p_value <= evalue && score > expected, score >= scoreT * length)` on w1 itself
  pass 3  a record whose list is not of length 1 and holds exactly one template with w1 != 0 adds abs(score) to uniq2[that template]
          (uniq2 starts as a copy of the unique scores of stage 3a)
  pass 4  a record with one template takes it. Any other: tot = the sum of uniq2 over its list as a 32-bit int; with tot != 0 and a first
          sequence of 16 bases or more, one minimal-standard step on the seed gives rand, randScore = (unsigned) (rand / INT_MAX * tot), and
          the first entry at which the running sum of uniq2 exceeds randScore is taken; otherwise, or where none is, the best of the list.
          Template 0 (an empty list ends there): not filed.
"""
import math

import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
INT_MAX = 0x7fffffff

# fastp (stdstat.c:36-134): chi-square quantile -> p-value by table
_STEPS = [(114.5242, 1e-26), (109.9604, 1e-25), (105.3969, 1e-24), (100.8337, 1e-23), (96.27476, 1e-22), (91.71701, 1e-21), (87.16164, 1e-20),
          (82.60901, 1e-19), (78.05917, 1e-18), (73.51245, 1e-17), (68.96954, 1e-16), (64.43048, 1e-15), (59.89615, 1e-14), (55.36699, 1e-13),
          (50.84417, 1e-12), (46.32844, 1e-11), (41.82144, 1e-10), (37.32489, 1e-9), (32.84127, 1e-8), (28.37395, 1e-7), (23.92814, 1e-6),
          (19.51139, 1e-5), (15.13671, 1e-4), (10.82759, 1e-3), (6.634897, 0.01), (3.841443, 0.05), (2.705532, 0.1), (2.072251, 0.15),
          (1.642374, 0.2), (1.323304, 0.25), (1.074194, 0.3), (0.8734571, 0.35), (0.7083263, 0.4), (0.5706519, 0.45), (0.4549364, 0.5),
          (0.3573172, 0.55), (0.2749959, 0.6), (0.2059001, 0.65), (0.1484719, 0.7), (0.1015310, 0.75), (0.06418475, 0.8), (0.03576578, 0.85),
          (0.01579077, 0.9), (0.00393214, 0.95)]


def _fastp(q):
    for quantile, p in _STEPS:
        if q > quantile:
            return p
    return 1.0 if q >= 0 else 1.0 - _fastp(-q)


def p_chisqr(q):
    """stdstat.c:136-147; q a numpy longdouble"""
    if q < 0:
        return 1e-26
    if q > 49:
        return _fastp(q)
    return 1 - 1.772453850 * math.erf(math.sqrt(float(np.longdouble(0.5) * q))) / math.gamma(0.5)


def i32(x):
    """an integer stored into an `int`"""
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def seed_of(codes):
    """the `rand` of conclave.c:566-571 for a sequence of codes 0..4 (16 or more of them): its first seven and last seven bases"""
    c = [int(x) for x in codes]
    r, j = c[0], len(c)
    for i in range(7):
        j -= 1
        r = (((r << 2) | c[i]) << 2) | c[j]
    return i32(r)


def _cdiv(a, b):
    """C's integer division and remainder (towards zero)"""
    q = abs(a) // abs(b)
    q = q if (a < 0) == (b < 0) else -q
    return q, a - q * b


def _best(lst, AS, US, tlen, lc, best_tmpl):
    """the best-of-list rule with runConClave2's variables: best_read_score an int, bestNum a long unsigned -> index into lst or -1"""
    best_read_score, best_num, best_score, pick = 0, 0, 0.0, -1
    for i, x in enumerate(lst):
        t = abs(x)
        a, u = int(AS[t]), int(US[t])
        b = best_read_score & M64                    # (the int, sign-extended for the comparison with a long unsigned)
        sc = 1.0 * float(a) / float(int(tlen[t]))
        k1, k2 = ((sc, best_score), (a, b)) if lc else ((a, b), (sc, best_score))
        take = False
        if k1[0] > k1[1]:
            take = True
        elif k1[0] == k1[1]:
            if k2[0] > k2[1]:
                take = True
            elif k2[0] == k2[1]:
                take = u > best_num or (u == best_num and t < abs(best_tmpl))
        if take:
            pick, best_tmpl, best_read_score, best_score, best_num = i, x, i32(a), sc, u
    return pick


def significance(w1, tlen, evalue, scoreT, cmp_mode=0):
    """pass 2 (conclave.c:469-491) in place -> number of templates discarded"""
    D = len(tlen)
    nhits = sum(int(w1[t]) for t in range(1, D)) & M64
    tot_ulen = sum(int(tlen[t]) for t in range(1, D)) & M64
    gone = 0
    for t in range(D - 1, 0, -1):
        read_score = i32(int(w1[t]))
        if not read_score:
            continue
        t_len = int(tlen[t])
        rest = (tot_ulen - t_len) & M64
        expected = np.longdouble(t_len)
        expected /= np.longdouble(rest if 1 < rest else 1)
        expected *= np.longdouble((nhits - read_score) & M64)
        q = np.longdouble(read_score) - expected
        q /= (expected + np.longdouble(read_score))
        q *= np.longdouble(read_score) - expected
        p = p_chisqr(q)
        a, b = bool(p <= evalue and np.longdouble(read_score) > expected), bool(float(read_score) >= scoreT * t_len)
        keep = (a or b) if cmp_mode == 0 else ((a and b) if cmp_mode == 1 else True)
        if not keep:
            w1[t] = 0
            gone += 1
    return gone


def conclave2(n_hits, score, q_len, q_len2, off, seed, tmpl, start, end, AS, US, tlen, evalue=0.05, scoreT=0.5, lc=False, cmp_mode=0):
    """-> dict(tmpl, start, end per record; w_scores, fragment_counts, read_counts, depth per template; w1 (after pass 2), uniq2;
    counters = dict(draw, fallback, made_unique, discarded, empty))"""
    n, D = len(n_hits), len(tlen)
    nh = [abs(int(x)) for x in n_hits]
    written = [nh[r] > 0 or int(score[r]) != 0 for r in range(n)]
    lists = [[int(x) for x in tmpl[int(off[r]):int(off[r]) + nh[r]]] if written[r] else [] for r in range(n)]
    cnt = dict(draw=0, fallback=0, made_unique=0, discarded=0, empty=0)

    # pass 1
    w1 = [0] * D
    last_first = 0
    for r in range(n):
        if not written[r]:
            continue
        L = lists[r]
        if len(L) > 1:
            k = _best(L, AS, US, tlen, lc, -1)
            t = L[k] if k >= 0 else -1
        elif len(L) == 1:
            t = L[0]
        else:
            t = last_first
            cnt["empty"] += 1
        if L:
            last_first = L[0]
        w1[abs(t)] = (w1[abs(t)] + abs(int(score[r]))) & M64
    # pass 2
    cnt["discarded"] = significance(w1, tlen, evalue, scoreT, cmp_mode)
    # pass 3
    uniq2 = [int(x) for x in US]
    for r in range(n):
        if not written[r] or len(lists[r]) == 1:
            continue
        alive = [abs(x) for x in lists[r] if w1[abs(x)]]
        if len(alive) == 1:
            uniq2[alive[0]] = (uniq2[alive[0]] + abs(int(score[r]))) & M64
            cnt["made_unique"] += 1
    # pass 4
    o_t, o_s, o_e = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    w = np.zeros(D, np.uint64)
    fc, rcn, depth = np.zeros(D, np.uint32), np.zeros(D, np.uint32), np.zeros(D, np.uint64)
    for r in range(n):
        if not written[r]:
            continue
        L, o = lists[r], int(off[r])
        pick = -1
        if len(L) != 1:
            tot = 0
            for x in L:
                tot = i32(tot + uniq2[abs(x)])
            if tot and 16 <= int(q_len[r]):
                assert tot > 0, "a sum of unique scores that wraps negative: undefined in the reference, nothing to restate"
                rnd = int(seed[r])
                q, m = _cdiv(rnd, 127773)
                rnd = i32(16807 * m - 2836 * q)
                if rnd <= 0:
                    rnd += INT_MAX
                rand_score = int(float(rnd) / float(INT_MAX) * float(tot)) & M32
                run = 0
                for i, x in enumerate(L):
                    run = (run + uniq2[abs(x)]) & M64
                    if rand_score < run:
                        pick = i
                        break
                if pick >= 0:
                    cnt["draw"] += 1
            if pick < 0:
                pick = _best(L, AS, uniq2, tlen, lc, 0)
                if L:
                    cnt["fallback"] += 1
        else:
            pick = 0
        if pick < 0:
            continue
        t = L[pick]
        o_t[r], o_s[r], o_e[r] = t, int(start[o + pick]), int(end[o + pick])
        t = abs(t)
        if t == 0:
            continue
        w[t] += np.uint64(abs(int(score[r])))
        fc[t] += 1
        rcn[t] += 2 if int(score[r]) < 0 else 1
        depth[t] += np.uint64(int(q_len[r]) + (int(q_len2[r]) if int(score[r]) < 0 else 0))
    return dict(tmpl=o_t, start=o_s, end=o_e, w_scores=w, fragment_counts=fc, read_counts=rcn, depth=depth, w1=np.array(w1, np.uint64),
                uniq2=np.array(uniq2, np.uint64), counters=cnt)


def vectors_from_records(n_hits, score, off, tmpl, D):
    """the two ConClave vectors of stage 3a as they follow from the records (update_Scores, updatescores.c:283-295): every listed template
    gets the record's score, a one-template record adds to the unique vector too"""
    AS, US = np.zeros(D, np.uint64), np.zeros(D, np.uint64)
    for r in range(len(n_hits)):
        k, s, o = abs(int(n_hits[r])), abs(int(score[r])), int(off[r])
        for x in tmpl[o:o + k]:
            AS[abs(int(x))] += np.uint64(s)
        if k == 1:
            US[abs(int(tmpl[o]))] += np.uint64(s)
    return AS, US
