#!/usr/bin/env python3
"""Directed fixture for the long-read traceback's size classes (longtrace.hip: lt_class, lt_lane_class, the windows of chain_dev.h):
`kma -i reads.fq -o out -t_db db -Mt1 1 -t 1 -sam` on reads built so that each yields ONE DP problem of chosen mode, rows and
columns -- or none -- under the default scoring scheme and under a second, larger one.

A read is an exact copy of a stretch of the template except for one foreign piece: a join (T[p:p+tl] replaced by X, X differing from
the template at both its ends, so the two MEMs end where intended and neither tail is a problem) or a tail (the first / last n template
bases of the read de-seeded by a substitution every 12 bases, with foreign sequence in front of / behind them where the window has
to cut the query side). No 16-mer of a foreign piece may occur in the template on either strand, every 16-mer of an exact piece
occurs there once: then the chain is the intended one. The generator checks the intention on the CPU restatement (oracle/align.c logs
the problems it solves) and the fate of every read (mapped / dropped) on the reference's own output.

Inputs are seeded here; the outputs are the reference's: one out.<scheme>.sam.tsv.gz per scheme (qname, flag, rname, pos, mapq, cigar,
AS); schemes.tsv holds the schemes' values (mismatches all alike, N scores 0) and the lane kernels' 16-bit gate under each. cases.tsv names for every read its group, its case, its fate, the problem (mode k, query columns, template rows, band; 0 = full
matrix) and the class the problem falls into, per scheme (the lane classes depend on the scheme through the 16-bit gate lane_tq): lane =
the lane class with every lane class on and the default cap of 20000 turns on a lane's sweep (-1: none), lanefree = the same with the cap
lifted (KMAHIP_LT_LANE_TURNS), wave = the wavefront class. Only data is stored.

Edges of lt_lane_class that no input reaches, and which the fixture therefore does not straddle: the band classes' row caps (t_l < 192 /
256 / 512) and matrix caps -- q_l <= RQ and band + 3 <= R bound t_l by 148 / 220 / 332 and the matrix by 10434 / 20778 / 47290 bytes;
and, under the default turn cap, the width edge of lane class 8 (band + 3 <= 144, |t_l - q_l| = 76 / 77): its smallest problem, 141 x
217, takes 142 x 141 = 20022 turns. That edge is straddled with the cap lifted."""
import gzip
import lzma
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
OUT = os.path.join(HERE, "ltclass")

K = 16
T_LEN = 20000
TIE_ZONE = 14000          # tie regions (homopolymers, short repeats) live behind this; the other joins stay in front of it

# name -> (reward, transition = transversion, gapopen, gapextend) as the reference's options take them
SCHEMES = {"s1": (1, 2, 3, 1), "s2": (7, 18, 35, 9)}


def scheme_values(name):
    """M, MM, U, W1 and the 5 x 5 table as kma.c:1308-1327 builds them (Mn = 0)"""
    M, T, W1, U = SCHEMES[name]
    MM = -((2 * T + 1) // 2)                       # (Ts + Tv - 1) / 2, C division
    d = [[(M if i == j else -T) if i < 4 and j < 4 else 0 for j in range(5)] for i in range(5)]
    return M, MM, -U, -W1, d


def scheme_options(name):
    M, T, W1, U = SCHEMES[name]
    return ["-reward", str(M), "-penalty", str(T), "-transition", str(T), "-transversion", str(T), "-gapopen", str(W1), "-gapextend", str(U)]


# ---- longtrace.hip's classifier, restated: the fixture's expectations come from here -----------------------------------------------
CHAIN_BW, LT_E_WAVE, LT_TMAX, LT_XE_LDS, XE_CAP, LANE_TURNS = 64, 8192, 127, 32768, 2 << 20, 20000
LANE_GEOM = [(16, 16, 16, 16 * 256), (32, 32, 16, 32 * 256), (48, 48, 16, 48 * 256), (64, 64, 16, 64 * 256), (128, 128, 32, 128 * 256),
             (256, 256, 32, 256 * 256), (72, 144, 12, 72 * 192), (96, 192, 16, 96 * 256), (144, 256, 32, 65536)]      # R, RQ, TW, ecap


def lane_tq(name):
    M, MM, U, W1, d = scheme_values(name)
    mx = max([abs(M), abs(MM), abs(U), abs(W1)] + [abs(x) for row in d for x in row])
    return 32000 // (abs(MM + U + W1) + 2 * mx + 1)


def band_of(q_l, t_l):
    band = abs(t_l - q_l) + CHAIN_BW
    return 0 if q_l <= band or t_l <= band else band


def stale_scan(q_l, t_l, band, k):
    if band & 1:
        band += 1
    cfin = ((t_l + q_l) >> 1) - (t_l - 1)
    return bool(band) and k == -2 and not (cfin + (band >> 1) < q_l - 1)


def wave_class(q_l, t_l, band, k):
    if band == 0 and t_l <= LT_TMAX:
        cells = (q_l + 1) * (t_l + 1)
        for c, (w, cap) in enumerate(((8, LT_E_WAVE // 8), (16, LT_E_WAVE // 4), (32, LT_E_WAVE // 2), (64, LT_E_WAVE))):
            if q_l <= w and cells <= cap:
                return c
    stale = stale_scan(q_l, t_l, band, k)
    if band & 1:
        band += 1
    pitch = band + 2 if band else q_l + 1
    if q_l < 256 and not stale and pitch * (t_l + 1) <= XE_CAP:
        return (4 if pitch * (t_l + 1) <= LT_XE_LDS else 9) + (2 if band else 0) + (0 if q_l <= 128 else 1)
    if band and q_l < 1024 and not stale and pitch * (t_l + 1) <= XE_CAP:
        return 15 + (0 if q_l < 512 else 1)
    return 8


def lane_class(q_l, t_l, band, k, tq, turns=LANE_TURNS):
    if not tq or t_l + q_l > tq or t_l < 1 or q_l < 1:
        return -1
    if band == 0:
        e = (q_l + 1) * (t_l + 1) + 4
        for j in range(6):
            R, RQ, TW, ecap = LANE_GEOM[j]
            if q_l + 1 <= R and e <= ecap and t_l < 16 * TW:
                return j if (q_l + 1) * t_l <= turns else -1
        return -1
    if stale_scan(q_l, t_l, band, k):
        return -1
    if band & 1:
        band += 1
    e = (band + 2) * (t_l + 1) + 4
    for j in range(6, 9):
        R, RQ, TW, ecap = LANE_GEOM[j]
        if band + 3 <= R and q_l <= RQ and e <= ecap and t_l < 16 * TW:
            return j if (band + 2) * t_l <= turns else -1
    return -1


# ---- reads ---------------------------------------------------------------------------------------------------------------------------
class SeedClash(Exception):
    """a 16-mer of a read's foreign piece occurs in the template (either strand), or one of an exact piece twice: another place is drawn"""


class Builder:
    def __init__(self):
        self.rng = np.random.default_rng(20)
        self.T = self.rng.integers(0, 4, size=T_LEN, dtype=np.uint8)
        self.ties = {}
        self.rows = []          # dict per read
        self.reads = []
        self.next_tie = TIE_ZONE

    # -- the template's tie regions: edge + content + edge, the edges G so that a read's T edges differ
    def tie_region(self, key, content):
        at = self.next_tie
        seg = np.concatenate([[2], content, [2]]).astype(np.uint8)
        self.T[at:at + len(seg)] = seg
        # the bases around the region differ from its edges (the MEMs end at the edges, not before)
        self.ties[key] = (at, len(seg))
        self.next_tie += 450
        assert self.next_tie <= 17800, self.next_tie
        return at, len(seg)

    def freeze(self):
        T = self.T
        self.kpos = {}
        keys = kmers(T)
        for i, x in enumerate(keys):
            self.kpos.setdefault(int(x), []).append(i)

    def foreign(self, n, avoid_first=None, avoid_last=None):
        x = self.rng.integers(0, 4, size=n, dtype=np.uint8)
        if n and avoid_first is not None:
            while x[0] == avoid_first:
                x[0] = self.rng.integers(0, 4)
        if n and avoid_last is not None:
            while x[-1] == avoid_last or (n == 1 and x[0] == avoid_first):
                x[-1] = self.rng.integers(0, 4)
        return x

    def place(self, t_l, flank):
        """a join position p in front of the tie zone whose read stays inside [0, TIE_ZONE)"""
        return int(self.rng.integers(flank + 1, TIE_ZONE - t_l - flank - 1))

    def add(self, group, case, read, exact, rc, fate, dp):
        """exact: [(read start, read end, template start)] the pieces that are copies; dp: None or (k, q_l, t_l)"""
        read = np.ascontiguousarray(read, np.uint8)
        self.check_seeds(read, exact, (group, case))
        from kma_amd import synth
        self.rows.append(dict(group=group, case=case, strand="-" if rc else "+", fate=fate, dp=dp))
        self.reads.append(np.ascontiguousarray(synth.revcomp_codes(read)) if rc else read)

    def check_seeds(self, read, exact, what):
        """every 16-mer inside an exact piece occurs once in the template (there); no other 16-mer of the read, on either strand, occurs
        at all (the all-A 16-mer is key 0, which the reference never looks up)"""
        from kma_amd import synth
        inside = np.zeros(max(0, len(read) - K + 1), bool)
        want = np.full(len(inside), -1, np.int64)
        for a, b, ts in exact:
            assert np.array_equal(read[a:b], self.T[ts:ts + b - a]), what
            if b - a >= K:
                inside[a:b - K + 1] = True
                want[a:b - K + 1] = ts + np.arange(b - a - K + 1)
        keys = kmers(read)
        for i, x in enumerate(keys):
            if x < 0 or x == 0:
                continue
            hits = self.kpos.get(int(x), [])
            if inside[i]:
                if hits != [int(want[i])]:
                    raise SeedClash(what, "exact 16-mer not unique", i, hits)
            elif hits:
                raise SeedClash(what, "foreign 16-mer in the template", i, hits)
        for x in kmers(synth.revcomp_codes(read)):
            if x > 0 and int(x) in self.kpos:
                raise SeedClash(what, "16-mer of the other strand in the template")

    def retry(self, fn):
        for _ in range(200):
            try:
                return fn()
            except SeedClash:
                continue
        return fn()

    # -- a join: T[p:p+tl] replaced by X
    def join(self, group, case, q_l, t_l, rc, X=None, p=None, flank=None, fate="map", flanks=None):
        T = self.T
        if flank is None:
            flank = default_flank(q_l, t_l)
        if p is None:
            for _ in range(1000):
                p = self.place(t_l, flank)
                # a pure deletion: the bases around it must not let a MEM run on
                if q_l or (T[p] != T[p + t_l] and T[p - 1] != T[p + t_l - 1]):
                    break
            else:
                raise AssertionError("no place")
        if X is None:
            X = self.foreign(q_l, T[p], T[p + t_l - 1]) if t_l else self.foreign(q_l, T[p], T[p - 1])
        assert len(X) == q_l
        if q_l and t_l:
            assert X[0] != T[p] and X[-1] != T[p + t_l - 1]
        fa, fb = flanks if flanks else (flank, flank)
        a, b = p - fa, p + t_l + fb
        assert 0 < a and b < T_LEN
        read = np.concatenate([T[a:p], X, T[p + t_l:b]])
        exact = [(0, fa, a), (fa + q_l, fa + q_l + fb, p + t_l)]
        dp = (0, q_l, t_l) if q_l and t_l and fate == "map" else None
        self.add(group, case, read, exact, rc, fate, dp)

    def deseed(self, seg, anchor_last):
        """a substitution every 12 bases, one of them at the end that touches the exact piece"""
        seg = seg.copy()
        n = len(seg)
        pos = range(n - 1, -1, -12) if anchor_last else range(0, n, 12)
        for i in pos:
            seg[i] = (seg[i] + 1 + self.rng.integers(0, 3)) & 3
        return seg

    def lead_tail(self, group, case, n, junk, at_start, rc, body=500):
        """junk + de-seeded T[s:s+n] + exact T[s+n:s+n+body]"""
        T = self.T
        s = 0 if at_start else int(self.rng.integers(400 + junk, 6000))
        F = self.foreign(junk, None, None)
        read = np.concatenate([F, self.deseed(T[s:s + n], True), T[s + n:s + n + body]])
        t_e, q_e = s + n, junk + n
        t_s = q_s = 0
        if (q_e << 1) < t_e or q_e + 64 < t_e:
            t_s = t_e - (q_e + min(q_e, 64))
        elif (t_e << 1) < q_e or t_e + 64 < q_e:
            q_s = q_e - (t_e + min(t_e, 64))
        self.add(group, case, read, [(junk + n, junk + n + body, s + n)], rc, "map", (-1 - (t_s == 0), q_e - q_s, t_e - t_s))

    def trail_tail(self, group, case, n, junk, at_end, rc, body=500):
        """exact T[e-body:e] + de-seeded T[e:e+n] + junk"""
        T = self.T
        e = T_LEN - n if at_end else int(self.rng.integers(1000, 6000))
        F = self.foreign(junk, None, None)
        read = np.concatenate([T[e - body:e], self.deseed(T[e:e + n], False), F])
        q_rest, t_rest = n + junk, T_LEN - e
        t_l, q_l = t_rest, q_rest
        if (q_rest << 1) < t_rest or q_rest + 64 < t_rest:
            t_l = q_rest + min(q_rest, 64)
        elif (t_rest << 1) < q_rest or t_rest + 64 < q_rest:
            q_l = t_rest + min(t_rest, 64)
        self.add(group, case, read, [(0, body, e - body)], rc, "map", (1 + (t_l == t_rest), q_l, t_l))


def default_flank(q_l, t_l):
    """exact bases on either side of a join: the read is over twice as long as the join plus 400 (link_window's reject stays away) and
    still scores half a point per column (the read filter's scoreT) when every pair of the join is a mismatch"""
    return (2 * (abs(q_l - t_l) + 3) + 4 * min(q_l, t_l) + q_l + t_l + 100) // 2 + 150


def kmers(seq):
    """16-mer keys of a code array, -1 where the 16-mer holds an N"""
    seq = np.asarray(seq, np.int64)
    n = len(seq) - K + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    key = np.zeros(n, np.int64)
    bad = np.zeros(n, bool)
    for x in range(K):
        key = (key << 2) | (seq[x:x + n] & 3)
        bad |= seq[x:x + n] > 3
    key[bad] = -1
    return key


A_, C_, G_, T_ = 0, 1, 2, 3


def rep(unit, times):
    return np.tile(np.array(unit, np.uint8), times)


def make_inputs():
    B = Builder()
    # template content of the tie cases: read content, template content; edges of the read T, of the template G
    ties = [("A20_A27", rep([A_], 20), rep([A_], 27)), ("A27_A20", rep([A_], 27), rep([A_], 20)),
            ("AC7_AC5", rep([A_, C_], 7), rep([A_, C_], 5)), ("ACT5_ACT3", rep([A_, C_, T_], 5), rep([A_, C_, T_], 3)),
            ("A40sub_A40", np.concatenate([rep([A_], 20), [C_], rep([A_], 19)]), rep([A_], 40)),
            ("AC7sub_AC7", np.concatenate([rep([A_, C_], 3), [A_, G_], rep([A_, C_], 3)]), rep([A_, C_], 7)),
            ("A98_A58", rep([A_], 98), rep([A_], 58)), ("A100_A120", rep([A_], 100), rep([A_], 120))]
    for key, rd, tp in ties:
        B.tie_region(key, tp)
    B.freeze()

    both = (False, True)

    def pairs(group, points):
        for q_l, t_l in points:
            for rc in both:
                B.retry(lambda: B.join(group, f"q{q_l}_t{t_l}", q_l, t_l, rc))

    # full-matrix joins on both sides of the lane classes' row widths; 256 columns: no lane class and no dpx class (serial);
    # the lane classes' cap on the turns of a sweep (20000)
    pairs("rows", [(q, 20) for q in (15, 16, 31, 32, 47, 48, 63, 64, 127, 128, 129, 255)] + [(256, 20), (256, 100), (255, 100), (199, 100), (199, 101)])
    # the wavefront classes 0-3: columns, cells against 1024 / 2048 / 4096 / 8192, template rows against 127
    pairs("wave", [(8, 112), (8, 113), (9, 50), (16, 119), (16, 120), (17, 50), (32, 123), (32, 124), (33, 50), (64, 125), (64, 126), (65, 50),
                   (63, 127), (63, 128)])
    # the lane classes' matrix cap (R x 256 bytes) and row cap (16 x TW template rows)
    pairs("lanecap", [(15, 254), (15, 255), (7, 255), (7, 256), (31, 254), (31, 255), (63, 254), (63, 255), (7, 511), (7, 512)])
    # full matrix against band; the lane band classes' widths (band + 3 against 72 / 96, and against 144 at |t_l - q_l| = 76 / 77, which
    # the default turn cap keeps out of the lane classes: (150, 226) / (150, 227) and (230, 306) / (230, 307) straddle it with the cap
    # lifted) and query columns (144 / 192; 256 under the default cap with (256, 256) / (257, 257), with the cap lifted also with
    # (256, 300) / (257, 301)); the turn cap of a banded sweep ((band + 2) x t_l: 94 x 212 / 94 x 213); 128 / 129 columns between
    # the banded dpx forms of 2 and 4 columns a lane
    pairs("band", [(64, 64), (65, 65), (66, 66), (100, 82), (100, 83), (82, 100), (83, 100),
                   (140, 144), (140, 145), (170, 198), (170, 199), (230, 306), (230, 307), (150, 226), (150, 227),
                   (144, 148), (145, 149), (192, 212), (193, 213), (256, 300), (257, 301), (256, 256), (257, 257),
                   (184, 212), (185, 213), (128, 140), (129, 141)])
    # move matrix in LDS against HBM: full matrix classes 4 -> 9 and 5 -> 10, banded 7 -> 12
    pairs("hbm", [(100, 323), (100, 324), (255, 127), (255, 128), (255, 159), (169, 239), (170, 240), (250, 320)])
    # tails: banded and wide, at the template's ends (k = -2 / 2, trimmed) and inside it (k = -1 / 1)
    for n in (150, 300, 600, 1100):
        for rc in both:
            B.retry(lambda: B.lead_tail("tails", f"lead_start_n{n}", n, n + 70, True, rc))
            B.retry(lambda: B.trail_tail("tails", f"trail_end_n{n}", n, n + 70, True, rc))
            B.retry(lambda: B.lead_tail("tails", f"lead_inner_n{n}", n, 0, False, rc))
            B.retry(lambda: B.trail_tail("tails", f"trail_inner_n{n}", n, 0, False, rc))
    # 512 and 1024 query columns: between the banded classes 15 and 16, and between 16 and the one-lane kernel
    for n in (511, 512, 1023, 1024):
        for rc in both:
            B.retry(lambda: B.lead_tail("tails", f"lead_inner_n{n}", n, 0, False, rc))
    for rc in both:
        # a short full-matrix tail with junk hanging over the template's end; tails that end flush with it
        B.retry(lambda: B.lead_tail("tails", "lead_start_trim_n30", 30, 100, True, rc))
        B.retry(lambda: B.trail_tail("tails", "trail_end_trim_n30", 30, 100, True, rc))
        for n in (100, 150):
            B.retry(lambda: B.lead_tail("tails", f"lead_start_flush_n{n}", n, 0, True, rc))
            B.retry(lambda: B.trail_tail("tails", f"trail_end_flush_n{n}", n, 0, True, rc))
    # degenerate joins: a pure deletion; a pure insertion (a tandem duplication behind one foreign base: the MEMs overlap on the template)
    for tl in (1, 5, 40):
        for rc in both:
            B.retry(lambda: B.join("degen", f"del_t{tl}", 0, tl, rc))

    def dup(d, rc):
        T = B.T
        p = B.place(0, 300)
        x = B.foreign(1, T[p], None)
        while x[0] == T[p] or x[0] == T[p - d - 1]:
            x = B.foreign(1, T[p], None)
        a, b = p - 300, p + 300
        read = np.concatenate([T[a:p], x, T[p - d:b]])
        B.add("degen", f"ins_dup{d}", read, [(0, 300, a), (301, 301 + d + 300, p - d)], rc, "map", None)
    for d in (20, 41, 60):
        for rc in both:
            B.retry(lambda: dup(d, rc))
    # ties: the traceback's preference among equal moves decides
    for key, rd, tp in ties:
        at, L = B.ties[key]
        X = np.concatenate([[T_], rd, [T_]]).astype(np.uint8)
        for rc in both:
            B.join("ties", key, len(X), L, rc, X=X, p=at, flank=230)

    # N's inside a join, at its first, middle and last position, once per kernel family
    def with_N(q_l, t_l, rc):
        flank = default_flank(q_l, t_l)
        p = B.place(t_l, flank)
        X = B.foreign(q_l, B.T[p], B.T[p + t_l - 1])
        X[0] = X[q_l // 2] = X[-1] = 4
        B.join("N", f"N_q{q_l}_t{t_l}", q_l, t_l, rc, X=X, p=p, flank=flank)
    for q_l, t_l in ((30, 25), (100, 60), (200, 50), (140, 144), (230, 300), (256, 100), (100, 330)):
        for rc in both:
            B.retry(lambda: with_N(q_l, t_l, rc))

    # the reject of a link: q_l against q_len >> 1
    # (the join is a de-seeded copy: the read on the accepted side still passes the read filter)
    def reject(fb, fate, rc):
        p = B.place(200, 100)
        X = B.deseed(B.T[p:p + 200], False)
        X[-1] = (B.T[p + 199] + 1 + B.rng.integers(0, 3)) & 3
        B.join("reject", f"q200_of_{300 + fb}", 200, 200, rc, X=X, p=p, flanks=(100, fb), fate=fate)
    for rc in both:
        for fb, fate in ((100, "map"), (99, "drop")):
            B.retry(lambda: reject(fb, fate, rc))

    # the 16-bit gate under the second scheme: rows + columns = lane_tq and lane_tq + 1, all mismatches / one long gap
    tq = lane_tq("s2")
    assert 200 <= tq <= 400 and lane_tq("s1") > 2000, tq

    def gate(q_l, t_l, kind, rc):
        flank = default_flank(q_l, t_l)
        p = B.place(t_l, flank)
        X = B.foreign(q_l, B.T[p], B.T[p + t_l - 1])
        if kind == "mism":
            m = min(q_l, t_l)
            X[:m] = (B.T[p:p + m] + 1 + B.rng.integers(0, 3, size=m)) & 3
            X[-1] = (B.T[p + t_l - 1] + 1 + B.rng.integers(0, 3)) & 3
        B.join("gate", f"{kind}_q{q_l}_t{t_l}", q_l, t_l, rc, X=X, p=p, flank=flank)
    for q_l, t_l, kind in ((tq // 2, tq - tq // 2, "mism"), (tq // 2 + 1, tq - tq // 2, "mism"), (tq - 40, 40, "gap"), (tq - 39, 40, "gap")):
        for rc in both:
            B.retry(lambda: gate(q_l, t_l, kind, rc))
    return B


def check_on_oracle(B, prefix):
    """the intention of every read on the CPU restatement: the problems it solves are the one the read aims at"""
    import ctypes
    import oracle
    odb = oracle.OracleDB(prefix)
    al = oracle.OracleAligner(odb)
    log = (ctypes.c_int32 * 1024).in_dll(oracle.lib(), "orc_dp_log")
    n = ctypes.c_int32.in_dll(oracle.lib(), "orc_dp_n")
    for i, (row, rd) in enumerate(zip(B.rows, B.reads)):
        n.value = 0
        o, is_rc, _ = al.align_trace_mt1(rd, 1)
        got = [tuple(log[4 * x:4 * x + 4]) for x in range(n.value)]
        assert (o is not None) == (row["fate"] == "map"), (i, row, got)
        if o is not None:
            assert is_rc == (row["strand"] == "-"), (i, row)
        want = []
        if row["dp"]:
            k, q_l, t_l = row["dp"]
            want = [(k, t_l, q_l, band_of(q_l, t_l))]
        assert got == want, (i, row, got, want)


def main():
    from kma_amd import synth
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    os.makedirs(OUT, exist_ok=True)
    B = make_inputs()
    with tempfile.TemporaryDirectory() as tmp:
        fsa, fq, prefix = os.path.join(tmp, "t.fsa"), os.path.join(tmp, "reads.fq"), os.path.join(tmp, "db")
        synth.write_fasta(fsa, ["template20k"], [B.T])
        synth.write_fastq(fq, B.reads, prefix="lt", qual=b"5")
        subprocess.run([KMA, "index", "-i", fsa, "-o", prefix], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        check_on_oracle(B, prefix)
        for scheme in SCHEMES:
            sam = subprocess.run([KMA, "-i", fq, "-o", os.path.join(tmp, "out"), "-t_db", prefix, "-Mt1", "1", "-t", "1", "-sam"] + scheme_options(scheme),
                                 check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()
            rows = {}
            for line in sam.splitlines():
                if line.startswith("@"):
                    continue
                c = line.split("\t")
                AS = ([x for x in c[11:] if x.startswith("AS:i:")] or ["AS:i:0"])[0][5:]
                assert c[0] not in rows
                rows[c[0]] = "\t".join([c[0], c[1], c[2], c[3], c[4], c[5], AS])
            # the fate of every read is the intended one (an unmapped read has a record with cigar '*')
            for i, row in enumerate(B.rows):
                rec = rows.get(f"lt{i}")
                assert rec is not None, (scheme, i, row)
                assert (rec.split("\t")[5] != "*") == (row["fate"] == "map"), (scheme, i, row, rec)
            with gzip.GzipFile(os.path.join(OUT, f"out.{scheme}.sam.tsv.gz"), "wb", mtime=0) as g:
                g.write(("\n".join(rows[f"lt{i}"] for i in range(len(B.rows))) + "\n").encode())

        def gz(src, dst):
            with open(src, "rb") as f, gzip.GzipFile(dst, "wb", mtime=0) as g:
                g.write(f.read())
        gz(fq, os.path.join(OUT, "reads.fq.gz"))
        gz(fsa, os.path.join(OUT, "db.fsa.gz"))
        with open(prefix + ".comp.b", "rb") as f, lzma.open(os.path.join(OUT, "db.comp.b.xz"), "wb", preset=9) as g:
            shutil.copyfileobj(f, g)
        for ext in (".length.b", ".seq.b", ".name"):
            shutil.copy(prefix + ext, os.path.join(OUT, "db" + ext))
    with open(os.path.join(OUT, "schemes.tsv"), "w") as f:
        f.write("scheme\tM\tMM\tU\tW1\tlane_tq\n")
        for sname in SCHEMES:
            M, MM, U, W1, d = scheme_values(sname)
            f.write(f"{sname}\t{M}\t{MM}\t{U}\t{W1}\t{lane_tq(sname)}\n")
    with open(os.path.join(OUT, "cases.tsv"), "w") as f:
        f.write("name\tgroup\tcase\tstrand\tfate\tn_dp\tk\tq_l\tt_l\tband\t" + "\t".join(f"lane_{s}\tlanefree_{s}\twave_{s}" for s in SCHEMES) + "\n")
        for i, row in enumerate(B.rows):
            cols = [f"lt{i}", row["group"], row["case"], row["strand"], row["fate"]]
            if row["dp"]:
                k, q_l, t_l = row["dp"]
                band = band_of(q_l, t_l)
                cols += [1, k, q_l, t_l, band]
                for s in SCHEMES:
                    cols += [lane_class(q_l, t_l, band, k, lane_tq(s)), lane_class(q_l, t_l, band, k, lane_tq(s), 1 << 30), wave_class(q_l, t_l, band, k)]
            else:
                cols += [0, 0, 0, 0, 0] + [-1, -1, -1] * len(SCHEMES)
            f.write("\t".join(str(c) for c in cols) + "\n")
    print(len(B.reads), "reads,", sum(len(r) for r in B.reads), "bases, longest", max(len(r) for r in B.reads))


if __name__ == "__main__":
    main()
