"""The counting template finder (`-ck`) restated in Python over a k-mer dictionary built from a fixture's FASTA: save_kmers_count
(savekmers.c:3067-3365) for single-end `-1t1` input, get_kmers_for_pair_count (:690-824) for one mate of a pair, and the pairing
functions that run over a pair's counted candidates, save_kmers_penaltyPair (:3572-3777) and save_kmers_unionPair (:3367-3570). Shared by
tests/test_ck_oracle.py (against the recorded taps), tests/test_ck_gpu.py (against the device) and tests/golden/make_golden_ck.py
(the intended outcomes of the hand-made reads). No test lives here.

A read is an array of codes 0-3 with 4 for N. Templates are numbered from 1 in file order; a value list ascends by template."""
import gzip

import numpy as np

LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    LUT[_c] = _i
    LUT[ord(chr(_c).lower())] = _i


def read_fasta(path):
    """-> (names, [codes]) of a FASTA file (gzip'd or plain)"""
    op = gzip.open if path.endswith(".gz") else open
    names, seqs, cur = [], [], []
    with op(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if names:
                    seqs.append(LUT[np.frombuffer(b"".join(cur), np.uint8)])
                names.append(line[1:].decode())
                cur = []
            elif line:
                cur.append(line)
    if names:
        seqs.append(LUT[np.frombuffer(b"".join(cur), np.uint8)])
    return names, seqs


def read_fastq(path):
    """-> (names, [codes]) of a FASTQ file (gzip'd or plain), four lines a record"""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        lines = f.read().split(b"\n")
    names = [lines[i][1:].split()[0].decode() for i in range(0, len(lines) - 3, 4)]
    reads = [LUT[np.frombuffer(lines[i + 1], np.uint8)] for i in range(0, len(lines) - 3, 4)]
    return names, reads


def _kmers(codes, k):
    """k-mer value of every start of an N-free code array (2 bits a base, first base highest)"""
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    v = np.zeros(n, np.uint64)
    c = codes.astype(np.uint64)
    for i in range(k):
        v = (v << np.uint64(2)) | c[i:i + n]
    return v


def kmer_dict(seqs, k=16):
    """k-mer -> tuple of the templates (1-based, ascending) that hold it on their forward strand; a window with an N holds none"""
    d = {}
    for t, s in enumerate(seqs, 1):
        ok = np.ones(max(0, len(s) - k + 1), bool)
        for p in np.flatnonzero(s > 3):
            ok[max(0, p - k + 1):p + 1] = False
        km = _kmers(np.where(s > 3, 0, s), k)
        for x in np.unique(km[ok]).tolist():
            d.setdefault(x, []).append(t)
    return {x: tuple(v) for x, v in d.items()}


def strands(read):
    """-> (forward codes with A at every N, its N positions, the reverse complement of THOSE codes -- T where the N's were, as
    rc_comp leaves them -- and the mirrored N positions)"""
    read = np.asarray(read, np.uint8)
    nf = np.flatnonzero(read > 3).tolist()
    fwd = np.where(read > 3, 0, read).astype(np.uint8)
    rev = (3 - fwd[::-1]).astype(np.uint8)
    L = len(read)
    return fwd, nf, rev, sorted(L - 1 - p for p in nf)


def quick_check(d, k, codes, n_list, exhaustive=False):
    """every k-th k-mer of every stretch between the positions of n_list (savekmers.c:3100-3114)"""
    if exhaustive:
        return True
    km = _kmers(codes, k).tolist()
    j = 0
    for end in list(n_list) + [len(codes)]:
        while j < end - k + 1:
            if km[j] in d:
                return True
            j += k
        j = end + 1
    return False


def count_walk(d, k, codes, bounds):
    """The counting walk (savekmers.c:3119-3183) over the stretches between the positions of `bounds`: -> (templates in first-seen
    order, {template: count}, hit starts)"""
    km = _kmers(codes, k).tolist()
    L, seqend = len(codes), len(codes) - k + 1
    order, score, hits = [], {}, 0
    j = 0
    for end in list(bounds) + [L]:
        if not j < seqend:
            break
        for e in range(j + k - 1, end):          # e = last base of the k-mer
            v = d.get(km[e - k + 1])
            if v is None:
                continue
            hits += 1
            for t in v:
                if t not in score:
                    score[t] = 0
                    order.append(t)
                score[t] += 1
        j = end + 1
    return order, score, hits


def get_match(order, score, min_frac=1.0):
    """getBestMatch (savekmers.c:273-294) or, min_frac != 1, getProxiMatch (:296-340) -> (best, kept templates in order)"""
    best = max(score[t] for t in order)
    if min_frac == 1.0:
        return best, [t for t in order if score[t] == best]
    thr = int(min_frac * best)
    return best, [t for t in order if thr <= score[t]]


def save_kmers_count(d, k, read, min_frac=1.0, exhaustive=False, mirrored=False):
    """-> None (no record) or (rc_flag, flag, T). mirrored=False is the reference: the reverse strand's walk takes its stretch bounds
    from the FORWARD strand's N list (savekmers.c:3250); mirrored=True is the "corrected" rule, kept as a foil for the tests."""
    if len(read) < k:
        return None
    fwd, nf, rev, nr = strands(read)
    best = [0, 0]
    T = [[], []]
    for s, (codes, own, bounds) in enumerate(((fwd, nf, nf), (rev, nr, nr if mirrored else nf))):
        if quick_check(d, k, codes, own, exhaustive):
            order, score, hits = count_walk(d, k, codes, bounds)
            if hits:
                best[s], T[s] = get_match(order, score, abs(min_frac))
    bs, br = best
    if (bs > 0 or br > 0) and (k <= bs or k <= br):
        if bs > br:
            return bs, 0, T[0]
        if bs < br:
            return br, 16, T[1]
        return -bs, 0, T[0] + [-t for t in T[1]]
    return None


def get_kmers_for_pair_count(d, k, read, exhaustive=False, forward_list=False):
    """one mate -> (the larger hit count of the two strands, [(template, count)] forward, the same for the reverse strand); both
    strands walk between their own N positions (comp_rc in place). forward_list=True is a foil for the tests: the reverse strand's
    walk bounded by the forward list, save_kmers_count's rule, which this function does not have"""
    if len(read) < k:
        return 0, [], []
    fwd, nf, rev, nr = strands(read)
    out, most = [], 0
    for codes, own in ((fwd, nf), (rev, nr)):
        lst = []
        if quick_check(d, k, codes, own, exhaustive):
            order, score, hits = count_walk(d, k, codes, nf if forward_list else own)
            lst = [(t, score[t]) for t in order]
            most = max(most, hits)
        out.append(lst)
    return most, out[0], out[1]


def scan_se(d, k, reads, **kw):
    """save_kmers_count over a batch -> (rc_flag, flag, T_off, T) as KmaHipDB.scan_se returns them"""
    rc_flag, flag, T_off, T = np.zeros(len(reads), np.int32), np.zeros(len(reads), np.int32), np.zeros(len(reads) + 1, np.int64), []
    for i, r in enumerate(reads):
        res = save_kmers_count(d, k, r, **kw)
        if res is not None:
            rc_flag[i], flag[i] = res[0], res[1]
            T += res[2]
        T_off[i + 1] = len(T)
    return rc_flag, flag, T_off, np.asarray(T, np.int32)


# ---- pairs: the pairing functions over the counted candidates ------------------------------------------------------------------------------
# save_kmers_penaltyPair (savekmers.c:3572-3777, with getFirstPen :1383, getSecondBestPen :1415, getF_Best :1648) and
# save_kmers_unionPair (:3367-3570, with getF_Best / getR_Best :1648-1762). `-ck` leaves them as they are and only swaps what they call
# for a mate's candidates (get_kmers_for_pair_ptr), so a candidate's score is its count and the hit count is the number of hit starts.
# A record is a dict(mate, rc, rc_flag, flag, T) in the order the reference prints them; a couple is two records, the first with an
# empty list. CompDNA.seqlen is unsigned, so the coverage tests wrap like 32-bit unsigned arithmetic.
def _u32(x):
    return x & 0xFFFFFFFF


def _find(lst, t):
    for tt, s in lst:
        if tt == t:
            return s
    return 0


def _best_of(F, R):
    """getF_Best: the best score over both strands' candidates and its templates in the order met, the forward strand's first"""
    best, out = 0, []
    for sign, lst in ((1, F), (-1, R)):
        for t, s in lst:
            if best < s:
                best, out = s, [sign * t]
            elif best == s:
                out.append(sign * t)
    return best, out


def _rec(mate, rc, score, flag, T):
    return dict(mate=mate, rc=rc, rc_flag=score, flag=flag, T=np.asarray(T, np.int32))


def pair_penalty(k, PE, len1, len2, c1, c2):
    """c = (hit count, forward [(template, count)], reverse [...]) of each mate -> records"""
    (hc1, F1, R1), (hc2, F2, R2) = c1, c2
    reg, best1 = [], 0                       # mate 1: getFirstPen, every candidate with its score, reverse ones negated
    if hc1:
        reg = [(t, s) for t, s in F1] + [(-t, s) for t, s in R1]
        best1 = max([s for _, s in reg] + [0])
    regT = [t for t, _ in reg]
    paired, best2, bT = False, 0, []
    if hc2:
        if 0 < best1:                        # getSecondBestPen
            bT = [t for t, _ in F2] + [-t for t, _ in R2]
            best2 = max([s for _, s in F2] + [s for _, s in R2] + [0])
            hits = []
            if best2:
                comp = max(0, best1 + best2 - PE)
                for t, s1 in reg:
                    sc = _find(R2, t) if t > 0 else _find(F2, -t)
                    if 0 < sc:
                        sc += s1
                        if comp < sc:
                            comp, hits = sc, [t]
                        elif comp == sc:
                            hits.append(t)
            if hits:
                paired, regT = True, hits
            else:
                regT = [t for t, s in reg if s == best1]
                bT = [t for t in bT if (best2 == _find(F2, t) if 0 < t else best2 <= _find(R2, -t))]
        else:                                # getF_Best on mate 2
            best2, regT = _best_of(F2, R2)
    o1, o2 = int(len1 >= k), int(len2 >= k)  # a scanned mate is left reverse-complemented by get_kmers_for_pair
    flag, flag_r = 65, 129
    out = []
    gate = lambda length, h: k <= h or _u32(length - h - k) < _u32(h * k)  # noqa: E731
    if 0 < best1 and 0 < best2:
        if paired:
            flag |= 2; flag_r |= 2
            comp = min(hc1 + hc2, best1 + best2)
            if k <= comp or _u32(len1 + len2 - comp - (k << 1)) < _u32(comp * k):
                if 0 < regT[0]:
                    flag |= 32; flag_r |= 16; o1 ^= 1
                    out = [_rec(0, o1, best1, flag, []), _rec(1, o2, best2, flag_r, regT)]
                else:
                    flag |= 16; flag_r |= 32; o2 ^= 1
                    out = [_rec(1, o2, best2, flag_r, []), _rec(0, o1, best1, flag, [-t for t in regT])]
        else:
            ok1, ok2 = gate(len1, min(hc1, best1)), gate(len2, min(hc2, best2))
            s1, s2 = best1, best2
            if ok1:
                if 0 < regT[0]:
                    o1 ^= 1
                    if regT[-1] < 0:
                        s1 = -s1
                else:
                    flag |= 16; flag_r |= 32
                    regT = [-t for t in regT]
            if ok2:
                if 0 < bT[0]:
                    o2 ^= 1
                    if bT[-1] < 0:
                        s2 = -s2
                else:
                    flag |= 32; flag_r |= 16
                    bT = [-t for t in bT]
            if ok1:
                out.append(_rec(0, o1, s1, flag, regT))
            if ok2:
                out.append(_rec(1, o2, s2, flag_r, bT))
    elif 0 < best1:
        if gate(len1, min(hc1, best1)):
            s1 = best1
            flag |= 8 | 32
            if 0 < regT[0]:
                o1 ^= 1
                if regT[-1] < 0:
                    s1 = -s1
            else:
                flag |= 16
                regT = [-t for t in regT]
            out = [_rec(0, o1, s1, flag, regT)]
    elif 0 < best2:
        if gate(len2, min(hc2, best2)):
            s2 = best2
            flag_r |= 8 | 32
            if 0 < regT[0]:
                o2 ^= 1
                if regT[-1] < 0:
                    s2 = -s2
            else:
                flag_r |= 16
                regT = [-t for t in regT]
            out = [_rec(1, o2, s2, flag_r, regT)]
    return out


def pair_union(k, len1, len2, c1, c2):
    (hc1, F1, R1), (hc2, F2, R2) = c1, c2
    regT, bT, best1, best2, paired = [], [], 0, 0, False
    if hc1:
        best1, regT = _best_of(F1, R1)
        if k < best1 and _u32(best1 * k) < _u32(len1 - best1):
            best1 = 0
    if hc2:
        if best1:
            best2, bT = _best_of(F2, R2)
            hits = 0
            if 0 < best2:
                # getR_Best leaves a score standing only for mate 2's best templates: those of mate 1's list that mate 2 holds on the
                # OTHER strand at its best score move to the front, in the order met
                for i in range(len(regT)):
                    rt = regT[i]
                    if (_find(R2, rt) if rt > 0 else _find(F2, -rt)) == best2:
                        regT[hits], regT[i] = rt, regT[hits]
                        hits += 1
            if hits:
                paired, regT = True, regT[:hits]
        else:
            best2, regT = _best_of(F2, R2)
        if k < best2 and _u32(best2 * k) < _u32(len2 - best2):
            best2, paired = 0, False
    o1, o2 = int(len1 >= k), int(len2 >= k)
    flag, flag_r = 65, 129
    if 0 < best1 and 0 < best2:
        if paired:
            flag |= 2; flag_r |= 2
            if 0 < regT[0]:
                flag |= 32; flag_r |= 16; o1 ^= 1
                return [_rec(0, o1, best1, flag, []), _rec(1, o2, best2, flag_r, regT)]
            flag |= 16; flag_r |= 32; o2 ^= 1
            return [_rec(1, o2, best2, flag_r, []), _rec(0, o1, best1, flag, [-t for t in regT])]
        s1, s2 = best1, best2
        if 0 < regT[0]:
            o1 ^= 1
            if regT[-1] < 0:
                s1 = -s1
        else:
            flag |= 16; flag_r |= 32
            regT = [-t for t in regT]
        if 0 < bT[0]:
            o2 ^= 1
            if bT[-1] < 0:
                s2 = -s2
        else:
            flag |= 32; flag_r |= 16
            bT = [-t for t in bT]
        return [_rec(0, o1, s1, flag, regT), _rec(1, o2, s2, flag_r, bT)]
    if best1:
        s1 = best1
        flag |= 8 | 32
        if 0 < regT[0]:
            o1 ^= 1
            if regT[-1] < 0:
                s1 = -s1
        else:
            flag |= 16
            regT = [-t for t in regT]
        return [_rec(0, o1, s1, flag, regT)]
    if best2:
        s2 = best2
        flag_r |= 8 | 32
        if 0 < regT[0]:
            o2 ^= 1
            if regT[-1] < 0:
                s2 = -s2
        else:
            flag_r |= 16
            regT = [-t for t in regT]
        return [_rec(1, o2, s2, flag_r, regT)]
    return []


def scan_pair(d, k, a, b, union=False, PE=7, exhaustive=False, forward_list=False):
    """one pair of reads (codes, 4 = N) -> its records. union: `-apm u` and what `-ipe` means without -apm; else `-apm p`.
    forward_list: the foil -- the candidates counted with save_kmers_count's forward-N-list rule, which pairs do NOT have"""
    c1 = get_kmers_for_pair_count(d, k, a, exhaustive, forward_list)
    c2 = get_kmers_for_pair_count(d, k, b, exhaustive, forward_list)
    return pair_union(k, len(a), len(b), c1, c2) if union else pair_penalty(k, PE, len(a), len(b), c1, c2)
