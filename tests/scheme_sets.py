"""Scoring schemes and read recipes of the scheme tests (tests/test_oracle_schemes.py on the CPU, tests/test_schemes_gpu.py on the
device): schemes that stand on the edges of the inequalities behind the diagonal shortcuts of stage 3a and the traceback (nw_diagonal,
diag_emit: align.hip), and planted reads that sit exactly where those inequalities decide. Every recipe is seeded; the tests assert on
the oracle's output that each scheme still bites. No tests in here."""
import collections

import numpy as np

from kma_amd import synth

Scheme = collections.namedtuple("Scheme", "M Ts Tv W1 U Wl Mn PE")      # match, transition, transversion, gap open, gap extend, local open, N, pairing

SCHEMES = {
    "default": Scheme(1, -2, -2, -3, -1, -6, 0, 7),            # gap_m_max 2
    "cge": Scheme(1, -2, -2, -5, -1, -6, 0, 17),               # what -cge leaves behind (its MM = -3 does not survive kma.c:1308): gap_m_max 3
    "gmm1": Scheme(2, -3, -3, -4, -2, -6, 0, 7),               # gap_m_max 1
    "gmm6": Scheme(1, -1, -1, -6, -1, -6, 0, 7),               # gap_m_max 6
    "tie": Scheme(1, -2, -2, -4, -1, -6, 0, 7),                # 3 mismatches tie with one gap in each sequence: gap_m_max 2 by the `- 1` alone
    "edge_wu": Scheme(2, -2, -2, -3, -1, -6, 0, 7),            # MM - M == W1 + U: not plain
    "mm_eq_w1": Scheme(1, -3, -3, -3, -1, -6, 0, 7),           # MM == W1: not plain
    "wl2": Scheme(1, -2, -2, -3, -1, -2, 0, 7),                # a cheap local opening
    "tstv": Scheme(1, -1, -3, -3, -1, -6, 0, 7),               # MM = -2 is no entry of the table: not plain
    "mn1": Scheme(1, -2, -2, -3, -1, -6, -1, 7),               # N costs
    "pe20": Scheme(1, -2, -2, -3, -1, -6, 0, 20),              # the pairing reward, for the couples
}
PE_SCHEMES = ("pe20", "cge", "gmm1")       # the schemes the couples run under


def mm_of(s):
    """rewards->MM = (Ts + Tv - 1) / 2 with C's truncation (kma.c:1308)"""
    t = s.Ts + s.Tv - 1
    return -((-t) // 2) if t < 0 else t // 2


def apply(rw, s):
    """the scheme into a Rewards structure (the oracle's or the binding's), laid out as kma.c:1308-1327 and orc_default_rewards do"""
    rw.M, rw.MM, rw.U, rw.W1, rw.Wl, rw.Mn, rw.PE = s.M, mm_of(s), s.U, s.W1, s.Wl, s.Mn, s.PE
    for i in range(4):
        for j in range(4):
            rw.d[i][j] = s.Tv
        rw.d[i][4] = s.Mn
        rw.d[i][i ^ 2] = s.Ts
        rw.d[i][i] = s.M
    for j in range(5):
        rw.d[4][j] = s.Mn
    rw.d[4][4] = 0


def options(name):
    """the reference's command-line options for a scheme (kma.c:821-915 forces the signs itself)"""
    if name == "cge":
        return ["-cge"]
    s = SCHEMES[name]
    return ["-reward", str(s.M), "-transition", str(-s.Ts), "-transversion", str(-s.Tv), "-gapopen", str(-s.W1), "-gapextend", str(-s.U),
            "-localopen", str(-s.Wl), "-Npenalty", str(-s.Mn), "-per", str(s.PE)]


def is_plain(s):
    """the host's predicate in front of nw_diagonal and the traceback's first pass, restated: a plain match / mismatch table, and the
    penalties ordered as the proof at diag_emit needs them"""
    M, MM, W1, U = s.M, mm_of(s), s.W1, s.U
    return (M > 0 and MM < 0 and W1 < 0 and U < 0 and MM > W1 and MM - M > 2 * W1 and MM - M > W1 + U) and s.Ts == MM and s.Tv == MM


def gap_m_max(s):
    """most mismatches on a link's diagonal that still make it the only optimum: m (M - MM) < M - 2 W1; -1 where the scheme is not plain"""
    return (s.M - 2 * s.W1 - 1) // (s.M - mm_of(s)) if is_plain(s) else -1


LINK_M_MAX = max(gap_m_max(s) for s in SCHEMES.values()) + 2       # 8
RUN = 14                       # bases of the homopolymer and of the dinucleotide run
RUN_AT = (320, 654)            # where the two runs start in a run template
READ_LEN = 150


def templates():
    """20 random templates of 700 ... 900 bases, 6 copies of the first six with 2 % substitutions (couples whose mates prefer different
    templates), 4 templates with a run of 14 A and a run of (AC)7 at RUN_AT, and 3 of 3 000 bases for the long reads
    -> names, seqs, indexes of the run templates, indexes of the long templates"""
    rng = np.random.default_rng(1601)
    seqs = [rng.integers(0, 4, int(rng.integers(700, 901)), dtype=np.uint8) for _ in range(20)]
    names = ["t%d" % i for i in range(20)]
    for i in range(6):
        v = seqs[i].copy()
        x = rng.random(len(v)) < 0.02
        v[x] = (v[x] + rng.integers(1, 4, int(x.sum()), dtype=np.uint8)) & 3
        seqs.append(v)
        names.append("t%d_v" % i)
    runs = []
    for i in range(4):
        flank = [rng.integers(0, 4, 320, dtype=np.uint8) for _ in range(3)]
        # neither neighbour of a run carries on with its period: G in front of and behind both
        for f in flank:
            f[0] = f[1] = f[-1] = f[-2] = 2
        s = np.concatenate([flank[0], np.zeros(RUN, np.uint8), flank[1], np.tile(np.array([0, 1], np.uint8), RUN // 2), flank[2]])
        assert len(s) == 3 * 320 + 2 * RUN and not s[RUN_AT[0]:RUN_AT[0] + RUN].any() and s[RUN_AT[1]] == 0 and s[RUN_AT[1] + RUN - 1] == 1
        runs.append(len(seqs))
        seqs.append(np.ascontiguousarray(s))
        names.append("run%d" % i)
    longs = []
    for i in range(3):
        longs.append(len(seqs))
        seqs.append(rng.integers(0, 4, 3000, dtype=np.uint8))
        names.append("long%d" % i)
    return names, seqs, runs, longs


def _other(b, rng):
    return (int(b) + int(rng.integers(1, 4))) & 3


def _link(r, at, m, spacing, rng):
    for x in range(m):
        r[at + x * spacing] = _other(r[at + x * spacing], rng)
    return r


def _shift(r, spare, at, d, ins_first, rng):
    """a one-base deletion and a one-base insertion d bases further on (or the other way round); spare = the template base behind the
    window, which the deletion pulls in: the read keeps its length"""
    r = list(r) + [int(spare)]
    if ins_first:
        r.insert(at, _other(r[at], rng))
        del r[at + 1 + d]
    else:
        del r[at]
        r.insert(at + d, _other(r[at + d], rng))
    return np.array(r[:READ_LEN], np.uint8)


def short_set():
    """-> names, seqs, reads: reads = list of (kind, parameter tuple, codes). Kinds: link (m, spacing), shift (d, insertion first),
    indel (signed length), tail (offset from the end, trailing end?, mismatches), runtail (run, bases inside the run, trailing end?),
    over (bases over the end, over the template's end?), nlink (m). Odd reads are reverse-complemented."""
    names, seqs, runs, longs = templates()
    rng = np.random.default_rng(1602)
    out = []

    def window(L=READ_LEN, spare=1):
        t = int(rng.integers(0, 20))
        a = int(rng.integers(0, len(seqs[t]) - L - spare + 1))
        return seqs[t], a

    for m in range(1, LINK_M_MAX + 1):
        for spacing in (2, 5, 9):
            for _ in range(24):
                s, a = window()
                out.append(("link", (m, spacing), _link(s[a:a + READ_LEN].copy(), 60, m, spacing, rng)))
    for d in range(1, 11):
        for ins_first in (0, 1):
            for _ in range(20):
                s, a = window()
                out.append(("shift", (d, ins_first), _shift(s[a:a + READ_LEN], s[a + READ_LEN], 60, d, ins_first, rng)))
    for w in (-3, -2, -1, 1, 2, 3):
        for _ in range(24):
            s, a = window(spare=3)
            at = int(rng.integers(50, 101))
            r = s[a:a + READ_LEN + 3]
            r = np.concatenate([r[:at], r[at - w:]]) if w < 0 else np.concatenate([r[:at], rng.integers(0, 4, w, dtype=np.uint8), r[at:]])
            out.append(("indel", (w,), np.ascontiguousarray(r[:READ_LEN])))
    for off in range(1, 16):
        for trailing in (0, 1):
            for mism in (1, 2):
                for _ in range(8):
                    s, a = window()
                    r = s[a:a + READ_LEN].copy()
                    for o in (off, off + 3)[:mism]:
                        p = READ_LEN - 1 - o if trailing else o
                        r[p] = _other(r[p], rng)
                    out.append(("tail", (off, trailing, mism), r))
    # tails with a clean shifted diagonal: the read ends j bases inside a run and its base next to the run is changed into the one that
    # carries the run's period on. The diagonal then has one mismatch; the diagonal behind a gap of one (homopolymer) or two
    # (dinucleotide) has none.
    for run in (0, 1):
        p = RUN_AT[run]
        for j in range(1, 11):
            for trailing in (0, 1):
                for t in runs:
                    for _ in range(2):
                        s = seqs[t]
                        if trailing:
                            r = s[p + j - READ_LEN:p + j].copy()
                            r[READ_LEN - 1 - j] = s[p + 1] if run else 0          # (AC)n is preceded by C, A...A by A
                        else:
                            r = s[p + RUN - j:p + RUN - j + READ_LEN].copy()
                            r[j] = s[p] if run else 0                              # (AC)n is followed by A
                        out.append(("runtail", (run, j, trailing), r))
    for h in range(1, 21):
        for at_end in (0, 1):
            for _ in range(4):
                s = seqs[int(rng.integers(0, 20))]
                junk = rng.integers(0, 4, h, dtype=np.uint8)
                r = np.concatenate([s[len(s) - READ_LEN + h:], junk]) if at_end else np.concatenate([junk, s[:READ_LEN - h]])
                out.append(("over", (h, at_end), np.ascontiguousarray(r)))
    for m in (1, 2, 3):
        for _ in range(32):
            s, a = window()
            r = _link(s[a:a + READ_LEN].copy(), 60, m, 5, rng)
            r[62] = 4
            out.append(("nlink", (m,), r))
    reads = [(k, p, np.ascontiguousarray((synth.revcomp_codes(r) if i & 1 else r).astype(np.uint8))) for i, (k, p, r) in enumerate(out)]
    assert all(len(r) == READ_LEN for _, _, r in reads)
    return names, seqs, reads


def gpu_subset(reads):
    """two reads in five, every kind and parameter among them: what a device test runs per scheme"""
    return [i for i in range(len(reads)) if i % 5 in (0, 3)]


def long_set():
    """24 reads of 1 200 ... 2 500 bases off the long templates, a link (m = 1 ... LINK_M_MAX in turn, spacing 5) or a shift (d = 1 ... 10 in
    turn) every 150 bases -> reads (codes; odd ones reverse-complemented)"""
    names, seqs, runs, longs = templates()
    rng = np.random.default_rng(1603)
    out = []
    for i in range(24):
        s = seqs[longs[i % 3]]
        L = int(rng.integers(1200, 2501))
        a = int(rng.integers(0, len(s) - L - 1))
        parts = []
        for c, o in enumerate(range(0, L, READ_LEN)):
            w = s[a + o:a + min(o + READ_LEN, L)].copy()
            if len(w) == READ_LEN:
                if c & 1:
                    w = _shift(w, s[a + o + READ_LEN], 60, 1 + (c // 2 + i) % 10, (c >> 1) & 1, rng)
                else:
                    w = _link(w, 60, 1 + (c // 2 + i) % LINK_M_MAX, 5, rng)
            parts.append(w)
        r = np.concatenate(parts)
        out.append(np.ascontiguousarray((synth.revcomp_codes(r) if i & 1 else r).astype(np.uint8)))
    return out


def couples():
    """300 couples of 150-base mates made from the planted short reads: a planted read and, 60 ... 200 bases further on on the other strand,
    a clean mate -- of the same template, or for the reads off t0 ... t5 in two couples out of three of its 2 % copy, so that the mates
    prefer different templates and the pairing reward decides -> list of (mate 1, mate 2)"""
    names, seqs, reads = short_set()
    rng = np.random.default_rng(1604)
    out = []
    for t in range(300):
        src = t % 6 if t % 3 else int(rng.integers(6, 20))
        s = seqs[src]
        a = int(rng.integers(0, len(s) - 2 * READ_LEN - 200))
        kind = t % 4
        m1 = s[a:a + READ_LEN].copy()
        if kind == 1:
            m1 = _link(m1, 60, 1 + t % 4, 5, rng)
        elif kind == 2:
            m1 = _shift(m1, s[a + READ_LEN], 60, 1 + t % 10, t & 1, rng)
        b = a + READ_LEN + int(rng.integers(60, 201))
        other = seqs[20 + src] if src < 6 and t % 3 == 1 else s
        m2 = synth.revcomp_codes(other[b:b + READ_LEN])
        pair = (np.ascontiguousarray(m1.astype(np.uint8)), np.ascontiguousarray(m2.astype(np.uint8)))
        out.append(pair[::-1] if t & 8 else pair)
    return out


def cigar_has_gap(cigar):
    return "I" in cigar or "D" in cigar


MODES = ("1t1", "default")       # and "pe" for PE_SCHEMES


def write_inputs(tmp):
    """index and FASTQ files of the short set and the couples under the directory tmp -> dict(prefix, fq, r1, r2, names, seqs, reads)"""
    import os
    from kma_amd import formats
    names, seqs, reads = short_set()
    prefix = os.path.join(str(tmp), "db")
    formats.write_index(prefix, names, seqs)
    fq, r1, r2 = (os.path.join(str(tmp), f) for f in ("reads.fq", "r1.fq", "r2.fq"))
    synth.write_fastq(fq, [r for _, _, r in reads])
    cp = couples()
    synth.write_fastq(r1, [a for a, _ in cp])
    synth.write_fastq(r2, [b for _, b in cp])
    return dict(prefix=prefix, fq=fq, r1=r1, r2=r2, names=names, seqs=seqs, reads=reads, couples=cp)


def reference_rows(kma, inp, scheme, mode, out):
    """the compiled reference on the short set (mode "1t1" or "default") or on the couples ("pe": -1t1 -ipe ... -apm p) under a scheme
    -> its fragment rows reduced to (name, ties, score, start, end, template) as text, by read number (a couple's two rows in file order)"""
    import gzip
    import subprocess
    args = {"1t1": ["-i", inp["fq"], "-1t1"], "default": ["-i", inp["fq"]], "pe": ["-ipe", inp["r1"], inp["r2"], "-apm", "p", "-1t1"]}[mode]
    subprocess.run([kma] + args + ["-t_db", inp["prefix"], "-o", out, "-t", "1"] + options(scheme), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with gzip.open(out + ".frag.gz", "rt") as f:
        rows = [line.rstrip("\n").split("\t") for line in f]
    rows = [(c[6].split()[0], c[1], c[2], c[3], c[4], c[5]) for c in rows]
    return sorted(rows, key=lambda r: int(r[0][1:]))


def load_rows(scheme, mode):
    """tests/golden/schemes/<scheme>.<mode>.tsv.gz (make_golden_schemes.py) -> list of (name, ties, score, start, end, template)"""
    import gzip
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schemes", "%s.%s.tsv.gz" % (scheme, mode))
    with gzip.open(path, "rt") as f:
        return [tuple(line.rstrip("\n").split("\t")) for line in f]
