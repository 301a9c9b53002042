"""Databases, read sets and settings of the threshold tests (tests/test_oracle_thresholds.py on the CPU, tests/test_thresholds_gpu.py
on the device): inputs on which -mct / -mrs / -ml (the chain finder) and -mq (the mapQ gate) decide something. Every recipe is seeded;
the tests assert on the oracle's output that each setting still bites."""
import numpy as np

from kma_amd import synth

# (coverT, mrs, minlen) = (-mct, -mrs, -ml); the first entry of every list is the default setting
CHAIN_DEFAULT = (0.1, 0.5, 16)
CHIMERIC_SETTINGS = [CHAIN_DEFAULT, (0.5, 0.5, 16), (0.9, 0.5, 16), (1.0, 0.5, 16), (0.0, 0.5, 16), (0.1, 0.3, 16), (0.1, 0.8, 16), (0.1, 0.5, 40),
                     (0.5, 0.3, 60), (0.02, 0.9, 25)]
NOISY_SETTINGS = [CHAIN_DEFAULT, (0.1, 0.3, 16), (0.1, 0.8, 16), (0.5, 0.5, 16), (1.0, 0.2, 16), (0.0, 0.9, 16), (0.3, 0.65, 50)]
# (0.5, 0.5, 16) moves only a dozen reads of the noisy set: it is pinned to the binary on the CPU but not used as a device case
NOISY_GPU_SETTINGS = [s for s in NOISY_SETTINGS[1:] if s != (0.5, 0.5, 16)]
MODULE_SETTINGS = [CHAIN_DEFAULT] + [(c, 0.5, 16) for c in (0.0, 0.2, 0.35, 0.5, 0.75, 1.0)]
MODULE_GPU_SETTINGS = MODULE_SETTINGS[1:] + [(0.5, 0.3, 60)]
LONG_SETTINGS = [(0.5, 0.5, 16), (0.0, 0.9, 16), (1.0, 0.2, 40)]

# (mq, scoreT, mrc, minlen) of stage 3a and the traceback
ALIGN_SETTINGS = [(1, .5, 0, 16), (60, .5, 0, 16), (120, .5, 0, 16), (200, .5, 0, 16), (0, .8, 0, 16), (0, .95, 0, 16), (0, .2, 0, 16), (0, .5, .9, 16),
                  (0, .5, 0, 120), (60, .8, .9, 40)]


def _substitute(r, rate, rng):
    x = (rng.random(len(r)) < rate) & (r < 4)
    r[x] = (r[x] + rng.integers(1, 4, int(x.sum()), dtype=np.uint8)) & 3
    return r


def chimeric_set():
    """the database and reads of test_chain_finder_oracle_differential_against_reference_binary, seed 1"""
    from test_oracle_golden import _chimeric_reads
    names, seqs = synth.make_gene_db(25, 4, 300, 900, 0.05, seed=201)
    return names, seqs, _chimeric_reads(seqs, 3000, np.random.default_rng(101))


def noisy_set():
    """2 000 chimeric reads with a further 0 / 3 / 6 / 10 % substitutions per read (chains whose score falls on either side of
    mrs x length), and 40 reads glued from 2-5 pieces of 200+ bases of either strand at 8 % errors"""
    from test_oracle_golden import _chimeric_reads
    names, seqs = synth.make_gene_db(25, 4, 300, 900, 0.05, seed=202)
    rng = np.random.default_rng(102)
    reads = _chimeric_reads(seqs, 2000, rng)
    for i, r in enumerate(reads):
        _substitute(r, (0.0, 0.03, 0.06, 0.10)[i & 3], rng)
    for _ in range(40):
        parts = []
        for _ in range(int(rng.integers(2, 6))):
            s = seqs[int(rng.integers(0, len(seqs)))]
            L = int(rng.integers(200, min(400, len(s)) + 1))
            a = int(rng.integers(0, len(s) - L + 1))
            w = _substitute(s[a:a + L].copy(), 0.08, rng)
            parts.append(synth.revcomp_codes(w) if rng.random() < 0.5 else w)
        reads.append(np.ascontiguousarray(np.concatenate(parts).astype(np.uint8)))
    return names, seqs, reads


def shared_module_set():
    """40 random templates, each with one of five modules (30 ... 110 bases) inserted somewhere; a read runs through template X up to
    the end of the module and goes on in template Y behind Y's copy of it: the two chains overlap by the module, which is what
    coverT weighs"""
    rng = np.random.default_rng(207)
    modules = [rng.integers(0, 4, m, dtype=np.uint8) for m in (30, 45, 60, 80, 110)]
    seqs, where = [], []
    for t in range(40):
        body = rng.integers(0, 4, int(rng.integers(500, 1001)), dtype=np.uint8)
        mod = modules[t % 5]
        p = int(rng.integers(0, len(body) + 1))
        seqs.append(np.ascontiguousarray(np.concatenate([body[:p], mod, body[p:]])))
        where.append((t % 5, p))
    names = ["m%d_t%d" % (t % 5, t) for t in range(40)]
    reads = []
    while len(reads) < 2000:
        x, y = (int(v) for v in rng.integers(0, 40, 2))
        if x == y or where[x][0] != where[y][0]:
            continue
        m = len(modules[where[x][0]])
        p, q = where[x][1], where[y][1]
        La, Lb = (int(v) for v in rng.integers(40, 201, 2))
        if p - La < 0 or q + m + Lb > len(seqs[y]):
            continue
        r = _substitute(np.concatenate([seqs[x][p - La:p + m], seqs[y][q + m:q + m + Lb]]), 0.01, rng)
        if len(reads) & 1:
            r = synth.revcomp_codes(r)
        reads.append(np.ascontiguousarray(r.astype(np.uint8)))
    return names, seqs, reads


def repeat_rich_set():
    """24 templates: a flank, then 2-4 copies of a 180 ... 320-base unit, each copy diverged by 0 ... 8 % and followed by up to 40
    random bases. A 120-base read out of a copy has a second-best chain in the next copy: mapQ spreads from 0 to its maximum."""
    rng = np.random.default_rng(7)
    seqs = []
    for _ in range(24):
        unit = rng.integers(0, 4, int(rng.integers(180, 321)), dtype=np.uint8)
        parts = [rng.integers(0, 4, int(rng.integers(60, 200)), dtype=np.uint8)]
        for _ in range(int(rng.integers(2, 5))):
            parts.append(_substitute(unit.copy(), float(rng.choice([0.0, 0.005, 0.01, 0.02, 0.04, 0.08])), rng))
            parts.append(rng.integers(0, 4, int(rng.integers(0, 41)), dtype=np.uint8))
        seqs.append(np.ascontiguousarray(np.concatenate(parts)))
    names = ["rep%d" % t for t in range(24)]
    reads, *_ = synth.make_reads(seqs, 3000, read_len=120, sub_rate=0.01, random_frac=0.02, n_rate=0.0005, seed=3)
    return names, seqs, reads


LONG_ROUTE_MIN = 304        # N-free reads of more than 288 k-mer starts (k = 16) are what the chain finder's fast route leaves to the long-read kernels
N_LONG_ADDED = 260


def long_threshold_set(kind):
    """long_route_set(kind) of tests/test_chain_gpu.py, kept as it is, and behind it 40 templates of 4.6 ... 6.6 kb that carry one of five
    modules (100 ... 600 bases) with 260 N-free reads of 700 bases and more on them: 200 that run through a template into its module
    and go on behind another template's copy of it (the two chains overlap by 5 ... 65 % of the shorter one: coverT 0.0, 0.5 and 1.0 each
    draw the line elsewhere), at 1 % or 8 % substitutions, and 60 glued from 2-4 pieces of 300 ... 2 000 bases of either strand at
    0 ... 15 % (chains on either side of mrs 0.2, 0.5 and 0.9). -> names, seqs, reads, index of the first added read"""
    from test_chain_gpu import long_route_set
    names, seqs, reads = long_route_set(kind)
    names, seqs, reads = list(names), list(seqs), list(reads)
    first = len(reads)
    rng = np.random.default_rng(311)
    modules = [rng.integers(0, 4, m, dtype=np.uint8) for m in (100, 200, 300, 450, 600)]
    mine, where = [], []
    for t in range(40):
        body = rng.integers(0, 4, int(rng.integers(4500, 6001)), dtype=np.uint8)
        p = int(rng.integers(2000, len(body) - 2000 + 1))
        mine.append(np.ascontiguousarray(np.concatenate([body[:p], modules[t % 5], body[p:]])))
        where.append((t % 5, p))
    while len(reads) < first + 200:
        x, y = (int(v) for v in rng.integers(0, 40, 2))
        if x == y or where[x][0] != where[y][0]:
            continue
        m = len(modules[where[x][0]])
        p, q = where[x][1], where[y][1]
        La, Lb = (int(v) for v in rng.integers(300, 2001, 2))
        r = _substitute(np.concatenate([mine[x][p - La:p + m], mine[y][q + m:q + m + Lb]]), 0.08 if len(reads) % 4 == 3 else 0.01, rng)
        reads.append(np.ascontiguousarray((synth.revcomp_codes(r) if len(reads) & 1 else r).astype(np.uint8)))
    while len(reads) < first + N_LONG_ADDED:
        parts = []
        for _ in range(int(rng.integers(2, 5))):
            src = mine[int(rng.integers(0, 40))]
            L = int(rng.integers(300, 2001))
            a = int(rng.integers(0, len(src) - L + 1))
            w = _substitute(src[a:a + L].copy(), float(rng.choice([0.0, 0.04, 0.08, 0.12, 0.15])), rng)
            parts.append(synth.revcomp_codes(w) if rng.random() < 0.5 else w)
        reads.append(np.ascontiguousarray(np.concatenate(parts).astype(np.uint8)))
    return names + ["mod%d_t%d" % (t % 5, t) for t in range(40)], seqs + mine, reads, first


def flat_chain_records(per_read):
    """oracle.scan_chain's list per read -> (read, rc_flag, emit_rc, q_start, q_end, templates) in stream order"""
    return [(i, rf, er, qs, qe, tuple(int(t) for t in T)) for i, recs in enumerate(per_read) for rf, er, qs, qe, T in recs]


def reads_differing(a, b, n):
    """number of reads whose record lists differ between two flat record lists"""
    pa, pb = [[] for _ in range(n)], [[] for _ in range(n)]
    for r in a:
        pa[r[0]].append(r)
    for r in b:
        pb[r[0]].append(r)
    return sum(1 for x, y in zip(pa, pb) if x != y)
