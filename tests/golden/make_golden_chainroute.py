#!/usr/bin/env python3
"""tests/golden/chainroute: a directed fixture for the three routes of the default mode's stage 2 (kmahip_chain_device: fast, long-read,
lane-per-read) and the edges between them, recorded from the compiled reference (oracle/_ref/kma).

One hand-built database of 100 templates (24 to 700 bases, 21 kb in all), indexed at k = 16 and k = 12:
    U700                 a template of its own (lists of one; reads on either side of 288 and 144 k-mer starts, of k - 1 / k / k + 1 bases,
                         reads with one deletion / substitution / two substitutions: k - 1, k, k + 1 missed starts between two hits)
    LE LF                a SNP ladder: equal but for one substitution every 17 bases, so the value list alternates between {LE} and {LE, LF}
                         and a read of LE opens two anchors per 17 starts -- 31, 32, 33 anchors on one strand
    LA LB LA' LB'        the same with the reverse complements of both in the database: n anchors on both strands
    LC LD LC' LD'        as before, but LD' differs from LC' every 19 bases: one strand over the cap, the other under it
    F5 (5), S5 (5)       families whose members are IDENTICAL over a window and random elsewhere: F5 has windows shared by 5, 4, 3, 2 members
    F17 (17)             windows shared by 17, 16, 15 members; the 16 carry the template numbers whose LdsMap home slots are the highest
                         the database has, so the probe wraps round the table
    G10 (10), G7 (7)     windows of 10, 7, 6: 16 / 17 templates reached at a later anchor, in pieces glued together
    TA (9), TB (8)       TB holds the reverse complement of TA's windows (shared by 8 and 9): strand ties with 8 + 8 and 9 + 8 templates
    LG LH                a ladder of 13 bases: at k = 12 two anchors per 13 starts, so that 31 anchors leave room for a piece of U700 with a
                         substitution (k missed starts: the anchor goes on) or two (k + 1: a new one) -- 32 / 33 anchors by that rule alone,
                         the one place where it shows: a chain's score and bounds are the same either way
    26 short templates of random sequence (they give the others their numbers)

Every read is aimed (`aim` in cases.tsv: numbers of k-mer starts, anchors per strand, distinct templates, the route) and the aim is
checked here with the plain restatement of the anchor rule in tests/chainroute_util.py; the oracle (oracle/chain.c) must give the
reference's records for every read at both k, default and exhaustive.

Written: db.fsa.gz, db{16,12}.comp.b.xz / .length.b, db.seq.b / .name, reads.fq.gz, cases.tsv, s2_k{16,12}[x].bin.gz (`kma -s2 -t 1`, x:
-ex_mode), chain_k{16,12}.res / .fsa.gz / .frag.gz (the whole run without -1t1).
usage: python3 tests/golden/make_golden_chainroute.py (needs oracle/_ref/kma: make -C oracle ref)"""
import ctypes
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
import chainroute_util as cu  # noqa: E402
import oracle  # noqa: E402
from kma_amd import formats, synth  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
OUT = os.path.join(HERE, "chainroute")
N_T = 100
rng = np.random.default_rng(20261020)


class Fresh:
    """random sequence none of whose 12-mers (and so none of whose 16-mers) occurs anywhere else in what was made before, on either
    strand: what the reads hit is then what the database was built to share, at k = 12 too (at random a 12-mer of a read hits a
    database of 46 kb once in 200 starts)"""
    K = 12

    def __init__(self):
        self.seen = set()

    def note(self, seq):
        if len(seq) >= self.K:
            t = [int(x) for x in seq[-self.K:]]
            self.seen.add(tuple(t))
            self.seen.add(tuple(3 - x for x in reversed(t)))

    def extend(self, seq, n):
        for _ in range(n):
            order = [int(x) for x in rng.permutation(4)]
            pick = order[0]
            for b in order:
                if len(seq) < self.K - 1 or tuple([int(x) for x in seq[len(seq) - self.K + 1:]] + [b]) not in self.seen:
                    pick = b
                    break
            seq.append(pick)
            self.note(seq)
        return seq

    def paste(self, seq, w):
        for b in w:
            seq.append(int(b))
            self.note(seq)
        return seq


FRESH = Fresh()


def rnd(n):
    return np.array(FRESH.extend([], n), np.uint8)


def other(b):
    return np.uint8((int(b) + 1 + int(rng.integers(0, 3))) & 3)


def rc(s):
    return synth.revcomp_codes(np.asarray(s, np.uint8))


def home_slot(t):
    return ((t * 0x9E3779B1) & 0xFFFFFFFF) >> 28


def ladder(base, s, phase=8):
    out = base.copy()
    for p in range(phase, len(base), s):
        out[p] = other(base[p])
    return out


def make_db():
    """-> names, seqs (template number = index + 1), W: the windows by name"""
    W = {}
    groups = {}

    def family(name, n, windows, length=400):
        members = [FRESH.extend([], 25) for _ in range(n)]
        for wname, m, wl, preset in windows:
            w = preset if preset is not None else rnd(wl)
            W[f"{name}.{wname}"] = w
            for i in range(n):
                if i < m:
                    FRESH.paste(members[i], w)
                else:
                    FRESH.extend(members[i], len(w))
                FRESH.extend(members[i], 12)
        groups[name] = [(f"{name}_{i}", np.array(FRESH.extend(members[i], max(20, length - len(members[i]))), np.uint8)) for i in range(n)]
    # (no longer than their windows need: the two indexes are nine tenths of the fixture's bytes)
    family("F17", 17, [("A", 17, 80, None), ("B", 16, 80, None), ("C", 15, 80, None)], 320)
    family("G10", 10, [("A", 10, 80, None)], 160)
    family("G7", 7, [("A", 7, 80, None), ("B", 6, 80, None)], 230)
    family("F5", 5, [("w5", 5, 70, None), ("w4", 4, 70, None), ("w3", 3, 70, None), ("w2", 2, 70, None)], 370)
    family("S5", 5, [("A", 5, 80, None)], 160)
    family("TA", 9, [("W1", 8, 80, None), ("W2", 9, 80, None)], 230)
    family("TB", 8, [("W1", 8, 80, rc(W["TA.W1"])), ("W2", 8, 80, rc(W["TA.W2"]))], 230)
    W["U700"] = rnd(700)
    groups["U"] = [("U700", W["U700"])]
    W["LE"], W["LA"], W["LC"], W["LG"] = rnd(420), rnd(360), rnd(360), rnd(300)
    W["LH"] = ladder(W["LG"], 13)
    W["LF"], W["LB"], W["LD"] = ladder(W["LE"], 17), ladder(W["LA"], 17), ladder(W["LC"], 17)
    groups["L"] = [("LE", W["LE"]), ("LF", W["LF"]), ("LA", W["LA"]), ("LB", W["LB"]), ("LAr", rc(W["LA"])), ("LBr", rc(W["LB"])),
                   ("LC", W["LC"]), ("LD", W["LD"]), ("LCr", rc(W["LC"])), ("LDr", ladder(rc(W["LC"]), 19)),
                   ("LG", W["LG"]), ("LH", W["LH"])]
    groups["R"] = [(f"R_{i}", rnd(24)) for i in range(26)]
    # template numbers: the 16 members of F17 that share window B get the numbers with the highest home slots of LdsMap
    wrap = sorted(range(1, N_T + 1), key=lambda t: (-home_slot(t), t))[:16]
    rest = [t for t in range(1, N_T + 1) if t not in wrap]
    slots = {}
    for t, m in zip(sorted(wrap), groups["F17"][:16]):
        slots[t] = m
    later = groups["F17"][16:] + groups["G10"] + groups["G7"] + groups["F5"] + groups["S5"] + groups["TA"] + groups["TB"] + groups["U"] + groups["L"] + groups["R"]
    assert len(later) == len(rest), (len(later), len(rest))
    for t, m in zip(rest, later):
        slots[t] = m
    names = [slots[t][0] for t in range(1, N_T + 1)]
    seqs = [slots[t][1] for t in range(1, N_T + 1)]
    W["wrap_slots"] = sorted(home_slot(t) for t in wrap)
    return names, seqs, W


class Reads:
    def __init__(self, odb):
        self.odb = odb          # {k: OracleDB}
        self.rows = []
        self.reads = []

    def numbers(self, read, k, ex=0):
        a = cu.analyse(self.odb[k], read, ex)
        return dict(starts=a["starts"], aF=len(a["anchors"][0]), aR=len(a["anchors"][1]), nT=len(a["templates"]), route=cu.route_of(a),
                    last_open=max([x[0] for s in a["anchors"] for x in s] or [-1]))

    def retry(self, fn, tries=100):
        """fn draws a read and adds it; drawn again while a 12-mer that a cut, a joint or a substitution made hits by chance"""
        for _ in range(tries):
            n = len(self.rows)
            try:
                return fn()
            except AssertionError as e:
                err = e
                del self.rows[n:], self.reads[n:]
        raise err

    def add(self, group, case, read, aim, both=True):
        """aim: {k: {field: value}} on the read as given; with `both` the reverse complement follows, its strands swapped"""
        for flip in ((0, 1) if both else (0,)):
            rd = rc(read) if flip else np.asarray(read, np.uint8)
            aims = []
            for k, want in aim.items():
                got = self.numbers(rd, k)
                for f, v in want.items():
                    if flip:
                        f = {"aF": "aR", "aR": "aF"}.get(f, f)
                        if isinstance(v, str):
                            v = {"marked:aF": "marked:aR", "marked:aR": "marked:aF"}.get(v, v)
                    assert got[f] == v or (v == "marked" and got[f].startswith("marked:a")), (group, case, flip, k, f, v, got)
                    aims.append(f"k{k}:{f}={v}")
            # (an aim that holds at both k is written once, without the k)
            short = []
            for x in aims:
                kk, fv = x.split(":", 1)
                if all(f"k{k}:{fv}" in aims for k in cu.KS):
                    if fv not in short:
                        short.append(fv)
                else:
                    short.append(x)
            self.rows.append(dict(group=group, case=case + ("-" if flip else "+"), aim=";".join(short)))
            self.reads.append(rd)


def make_reads(R, W):
    U = W["U700"]

    def cut(w, n, lo=2):
        """n bases from inside a window, the place drawn"""
        o = int(rng.integers(lo, len(w) - n - lo + 1))
        return w[o:o + n]
    both_k = lambda **kw: {k: dict(kw) for k in cu.KS}          # noqa: E731
    # ---- k-mer starts: 288 / 289 and 143 / 144 / 145 at both k, reads of k - 1, k, k + 1 bases
    for L in (299, 300, 303, 304, 158, 159, 160, 154, 155, 156, 11, 12, 13, 15, 16, 17):
        aim = {}
        for k in cu.KS:
            st = max(L - k + 1, 0)
            aim[k] = dict(starts=st, route="none" if st <= 0 else "marked:starts" if st > 288 else "fast")
            if 0 < st <= 288:
                aim[k].update(aF=1, nT=1)
        R.retry(lambda: R.add("starts", f"L{L}", cut(U, L, 0), aim))
    # ---- k - 1, k, k + 1 missed starts between two hits of one list: the hit before in another lane of 9 starts, in the pass before
    for kind in ("del", "sub", "sub2"):
        for nh in (66, 70, 99, 100, 144, 145, 153, 156, 160, 171):          # (66, 70: across the pass border once the read is turned round)
            def gap_read():
                src = cut(U, 260, 0).copy()
                if kind == "del":
                    rd = np.concatenate([src[:nh], src[nh + 1:]])[:220]          # starts nh - k + 1 .. nh - 1 miss
                elif kind == "sub":
                    rd = src[:220]
                    rd[nh - 1] = other(rd[nh - 1])                              # starts nh - k .. nh - 1 miss
                else:
                    rd = src[:220]
                    rd[nh - 2], rd[nh - 1] = other(rd[nh - 2]), other(rd[nh - 1])          # starts nh - k - 1 .. nh - 1 miss
                for k in cu.KS:          # (a deleted base that equals its neighbour costs a start less)
                    A = cu.analyse(R.odb[k], rd)["anchors"][0]
                    assert kind == "sub" or A[1][0] - A[0][1] - 1 == (k - 1 if kind == "del" else k + 1)
                R.add("gaps", f"{kind}_next{nh}", rd, both_k(aF=1 if kind == "sub" else 2, nT=1, route="fast"))
            R.retry(gap_read)
    # ---- list lengths 1 .. 5 (the cached head of the list and the list itself, at both widths)
    for wname, n in (("F5.w5", 5), ("F5.w4", 4), ("F5.w3", 3), ("F5.w2", 2)):
        R.retry(lambda: R.add("lists", f"list{n}", cut(W[wname], 62), both_k(aF=1, nT=n, route="fast")))
        R.retry(lambda: R.add("lists", f"list{n}_short", cut(W[wname], 42), both_k(aF=1, nT=n, route="fast")))
    R.retry(lambda: R.add("lists", "list1_short", cut(U, 40), both_k(aF=1, nT=1, route="fast")))
    R.retry(lambda: R.add("lists", "lists_5_3_1_of_6", np.concatenate([cut(W["F5.w5"], 55), cut(W["F5.w3"], 55), cut(U, 60)]), both_k(aF=3, nT=6, route="fast")))
    # ---- candidate templates: 15 / 16 / 17 at the first anchor (the 16: home slots that wrap round the table)
    for wname, n in (("F17.C", 15), ("F17.B", 16), ("F17.A", 17)):
        R.retry(lambda: R.add("tmpl", f"one_anchor_{n}", cut(W[wname], 62), both_k(aF=1, nT=n, route="given_up" if n > 16 else "fast")))
    # 16 / 17 reached at a later anchor
    g10, g6, g7 = (lambda: cut(W["G10.A"], 60)), (lambda: cut(W["G7.B"], 60)), (lambda: cut(W["G7.A"], 60))
    for case, parts, n in (("10+6", [g10, g6], 16), ("10+7", [g10, g7], 17), ("6+10", [g6, g10], 16), ("7+10", [g7, g10], 17)):
        R.retry(lambda: R.add("tmpl", f"later_{case}", np.concatenate([p() for p in parts]), both_k(aF=2, nT=n, route="given_up" if n > 16 else "fast")))
    # three pieces, the middle one on the other strand: several records, 16 / 17 templates in all
    f5, s5 = (lambda: rc(cut(W["F5.w5"], 60))), (lambda: cut(W["S5.A"], 60))
    R.retry(lambda: R.add("tmpl", "chimeric_6+5+5", np.concatenate([g6(), f5(), s5()]), both_k(aF=2, aR=1, nT=16, route="fast")))
    R.retry(lambda: R.add("tmpl", "chimeric_7+5+5", np.concatenate([g7(), f5(), s5()]), both_k(aF=2, aR=1, nT=17, route="given_up")))
    R.retry(lambda: R.add("tmpl", "chimeric_10+6r", np.concatenate([g10(), rc(g6())]), both_k(aF=1, aR=1, nT=16, route="fast")))
    R.retry(lambda: R.add("tmpl", "chimeric_10+7r", np.concatenate([g10(), rc(g7())]), both_k(aF=1, aR=1, nT=17, route="given_up")))
    # strand ties: TA on one strand, TB on the other
    R.retry(lambda: R.add("tie", "tie_8+8", cut(W["TA.W1"], 62), both_k(aF=1, aR=1, nT=16, route="fast")))
    R.retry(lambda: R.add("tie", "tie_9+8", cut(W["TA.W2"], 62), both_k(aF=1, aR=1, nT=17, route="given_up")))
    R.retry(lambda: R.add("tie", "tie_8+8_and_more", np.concatenate([cut(W["TA.W1"], 62), cut(W["F5.w2"], 45)]), both_k(aF=2, aR=1, nT=18, route="given_up")))
    # ---- N's (behind base 20): chain_kernel takes them whatever else they are
    for case, src, pos in (("U150_N20", U[200:350], [20]), ("U150_N75", U[200:350], [75]), ("U150_Nlast", U[200:350], [149]), ("U150_N3", U[200:350], [30, 31, 90]),
                           ("U304_N", U[50:354], [200]), ("t17_N", W["F17.A"][8:70], [40]), ("t16_N", W["F17.B"][8:70], [25]), ("tie_N", W["TA.W1"][8:70], [30])):
        rd = src.copy()
        rd[pos] = 4
        R.add("N", case, rd, both_k(route="marked:N"), both=pos[-1] < len(rd) - 20)
    return R


def search_ladders(R, W):
    """31 / 32 / 33 anchors: offset and length searched with the restatement, per k"""
    memo = {}

    def find(src, k, want, extra=lambda n: True):
        for L in range(303 if k == 16 else 299, 200, -1):
            for o in range(0, len(src) - L + 1):
                key = (src.tobytes(), o, L, k)
                if key not in memo:
                    memo[key] = R.numbers(src[o:o + L], k)
                n = memo[key]
                if all(n[f] == v for f, v in want.items()) and extra(n):
                    return src[o:o + L]
        raise AssertionError(("no read for", k, want))
    for k in cu.KS:
        for n in (31, 32, 33):
            route = "marked:aF" if n > 32 else "fast"
            R.add("anchors", f"k{k}_one_strand_{n}", find(W["LE"], k, dict(aF=n, aR=0)), {k: dict(aF=n, aR=0, route=route)})
            R.add("anchors", f"k{k}_both_{n}", find(W["LA"], k, dict(aF=n, aR=n)), {k: dict(aF=n, aR=n, route="marked" if n > 32 else "fast")})
            # the n-th anchor opens at the last start of the read
            R.add("anchors", f"k{k}_opens_last_{n}", find(W["LE"], k, dict(aF=n, aR=0), lambda x: x["last_open"] == x["starts"] - 1), {k: dict(aF=n, aR=0, route=route)})
        # one strand over the cap, the other under it and already filed
        for f in (32, 33, 34):
            rd = find(W["LC"], k, dict(aF=f), lambda x: 20 <= x["aR"] <= 31)
            R.add("anchors", f"k{k}_F{f}_Rless", rd, {k: dict(aF=f, route="marked:aF" if f > 32 else "fast")})
        rd = find(W["LE"], k, dict(aR=0), lambda x: x["aF"] >= 35)
        R.add("anchors", f"k{k}_far_over", rd, {k: dict(aR=0, route="marked:aF")})
        if k == 12:
            # 32 / 33 anchors that hang on "exactly k missed starts go on, k + 1 open": ladder anchors, then U700 with one / two substitutions
            for kind, n in (("sub", 32), ("sub", 33), ("sub2", 32), ("sub2", 33)):
                def glued():
                    p = int(rng.integers(0, 600))
                    tail = W["U700"][p:p + 44].copy()
                    tail[20] = other(tail[20])
                    if kind == "sub2":
                        tail[21] = other(tail[21])
                    for La in range(150, 250):
                        rd = np.concatenate([W["LG"][3:3 + La], tail])
                        x = R.numbers(rd, k)
                        if x["aF"] == n and x["aR"] == 0:
                            A = cu.analyse(R.odb[k], rd)["anchors"][0]
                            assert len(A) - (1 if kind == "sub" else 2) == n - (1 if kind == "sub" else 2) and A[-1][1] - A[-1][0] >= (k if kind == "sub" else 0)
                            return R.add("anchors", f"k{k}_ladder+{kind}_{n}", rd, {k: dict(aF=n, aR=0, route="marked:aF" if n > 32 else "fast")})
                    raise AssertionError("no length")
                R.retry(glued)
        # a ladder read with N's and one with too many starts besides
        rd = find(W["LE"], k, dict(aF=33, aR=0)).copy()
        rd[100] = 4
        R.add("N", f"k{k}_ladder33_N", rd, {k: dict(route="marked:N")})


def search_tie_anchors(R, W):
    """a chain of two anchors (pieces of G10's window around a piece of another family) whose score a lone anchor inside it equals: the
    lone anchor's templates join the record (getTieAnkerScore). Searched on the oracle's own log."""
    log = (ctypes.c_int * 4).in_dll(oracle.lib(), "orc_chain_log")
    for k in cu.KS:
        for mid, n in ((W["G7.B"], 16), (W["S5.A"], 15), (W["G7.A"], 17)):
            found = 0
            for b in (64, 60, 56, 68):
                for a in range(k + 4, 45):
                    for c in range(k + 4, 45):
                        if found or a + 4 + c > 76:
                            continue
                        rd = np.concatenate([W["G10.A"][2:2 + a], mid[8:8 + b], W["G10.A"][2 + a + 4:2 + a + 4 + c]])
                        if a + c not in range(b - 8, b + 2):
                            continue
                        for i in range(4):
                            log[i] = 0
                        recs = R.odb[k].scan_chain(formats.pack_ragged([rd]))
                        if log[2] and len(recs[0]) == 1 and len(recs[0][0][4]) == n and R.numbers(rd, k)["aF"] == 3:
                            R.add("tieank", f"k{k}_tie_anchor_{n}", rd, {k: dict(aF=3, nT=n, route="given_up" if n > 16 else "fast")})
                            found = 1
            assert found, ("no tie anchor", k, n)


def nowhere(R):
    for L in (40, 150, 303, 304):
        R.add("nowhere", f"random{L}", rnd(L), {16: dict(aF=0, aR=0, route="none")}, both=False)
    rd = rnd(150)
    rd[60] = 4
    R.add("nowhere", "random150_N", rd, {16: dict(aF=0, aR=0, route="none")}, both=False)


def gz(src, dst):
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", 9, mtime=0) as g:
        g.write(f.read())


def main():
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    os.makedirs(OUT, exist_ok=True)
    names, seqs, W = make_db()
    with tempfile.TemporaryDirectory() as tmp:
        fsa, fq = os.path.join(tmp, "db.fsa"), os.path.join(tmp, "reads.fq")
        synth.write_fasta(fsa, names, seqs)
        prefix, odb = {}, {}
        for k in cu.KS:
            prefix[k] = os.path.join(tmp, f"db{k}")
            subprocess.run([KMA, "index", "-i", fsa, "-o", prefix[k], "-k", str(k)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            odb[k] = oracle.OracleDB(prefix[k])
            assert cu.kmersize(odb[k]) == k
        R = Reads(odb)
        make_reads(R, W)
        search_ladders(R, W)
        search_tie_anchors(R, W)
        nowhere(R)
        synth.write_fastq(fq, R.reads, prefix="cr", qual=b"5")
        names_r = [f"cr{i}" for i in range(len(R.reads))]
        batch = formats.pack_ragged(R.reads)
        cols = {}
        disagree = []
        for k in cu.KS:
            base = [KMA, "-i", fq, "-o", os.path.join(tmp, f"out{k}"), "-t_db", prefix[k], "-t", "1"]
            for ex in (0, 1):
                tapf = os.path.join(tmp, f"s2_{cu.cfg_name(k, ex)}.bin")
                with open(tapf, "wb") as f:
                    subprocess.run(base + ["-s2"] + (["-ex_mode"] if ex else []), check=True, stdout=f, stderr=subprocess.DEVNULL)
                gz(tapf, os.path.join(OUT, f"s2_{cu.cfg_name(k, ex)}.bin.gz"))
                tap, n_tap = formats.parse_s2(open(tapf, "rb").read())
                assert 0 < n_tap <= len(R.reads)          # (the terminator counts what stage 1 let through: not the reads shorter than k)
                by = cu.tap_by_read(tap)
                mine = odb[k].scan_chain(batch, exhaustive=ex)
                for i, recs in enumerate(mine):
                    want = [(qs, qe, rf, T) for qs, qe, rf, T, _ in by.get(names_r[i], [])]
                    got = [(qs, qe, rf, tuple(int(t) for t in T)) for rf, er, qs, qe, T in recs]
                    if got != want:
                        disagree.append((k, ex, i, R.rows[i], got, want))
                    cols.setdefault(i, {})[f"recs_{cu.cfg_name(k, ex)}"] = len(want)
                for i, rd in enumerate(R.reads):
                    n = R.numbers(rd, k, ex)
                    c = cols[i]
                    c[f"starts_k{k}"] = n["starts"]
                    for f in ("aF", "aR", "nT", "route"):
                        c[f"{f}_{cu.cfg_name(k, ex)}"] = n[f]
            subprocess.run(base, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            shutil.copy(os.path.join(tmp, f"out{k}.res"), os.path.join(OUT, f"chain_k{k}.res"))
            shutil.copy(os.path.join(tmp, f"out{k}.frag.gz"), os.path.join(OUT, f"chain_k{k}.frag.gz"))
            gz(os.path.join(tmp, f"out{k}.fsa"), os.path.join(OUT, f"chain_k{k}.fsa.gz"))
            with open(prefix[k] + ".comp.b", "rb") as f, lzma.open(os.path.join(OUT, f"db{k}.comp.b.xz"), "wb", preset=9 | lzma.PRESET_EXTREME) as g:
                shutil.copyfileobj(f, g)
        for d in disagree:
            print("oracle != reference:", d)
        assert not disagree
        for ext in (".seq.b", ".name"):          # (the same at both k)
            shutil.copy(prefix[16] + ext, os.path.join(OUT, "db" + ext))
            assert open(prefix[16] + ext, "rb").read() == open(prefix[12] + ext, "rb").read(), ext
        for k in cu.KS:
            shutil.copy(prefix[k] + ".length.b", os.path.join(OUT, f"db{k}.length.b"))
        gz(fq, os.path.join(OUT, "reads.fq.gz"))
        gz(fsa, os.path.join(OUT, "db.fsa.gz"))
    head = ["name", "group", "case", "len", "aim", "starts_k16", "starts_k12"]
    for k, ex in cu.CONFIGS:
        head += [f"{f}_{cu.cfg_name(k, ex)}" for f in ("aF", "aR", "nT", "route", "recs")]
    with open(os.path.join(OUT, "cases.tsv"), "w") as f:
        f.write("\t".join(head) + "\n")
        for i, row in enumerate(R.rows):
            c = dict(cols[i], name=names_r[i], group=row["group"], case=row["case"], len=len(R.reads[i]), aim=row["aim"] or "-")
            f.write("\t".join(str(c[h]) for h in head) + "\n")
    print(len(R.reads), "reads,", sum(len(r) for r in R.reads), "bases; home slots of the 16:", W["wrap_slots"])
    for k, ex in cu.CONFIGS:
        routes = [cols[i][f"route_{cu.cfg_name(k, ex)}"] for i in range(len(R.reads))]
        print(cu.cfg_name(k, ex), {r: routes.count(r) for r in sorted(set(routes))})


if __name__ == "__main__":
    main()
