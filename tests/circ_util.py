"""Shared by the tests of circular alignments (`-ca`, `-mint2`, `-mint3`): the seeded inputs whose reads span the origin of their
template, and the helpers that run examples/kmahip_map and the compiled reference (oracle/_ref/kma -t 1) on them. No test lives here."""
import gzip
import os
import subprocess

import numpy as np

from kma_amd import formats, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")
HEADER = os.path.join(ROOT, "include", "kmahip.h")
TIMEOUT = 120

# seeds of the inputs: (database, reads). A seed that misses a floor of test_circular_gpu.FLOORS is changed here, never the floor.
SEEDS = {"A": (301, 11), "P": (301, 12), "L": (302, 13), "O": (301, 18), "M": (302, 21)}
# wrapped rows (end < start in the inflated .frag.gz) the reference must file with -ca on each input
FLOORS = {"A": 300, "P": 60, "L": 40, "O": 40}
# input M: with -ca the deepest column of a template's count matrix must exceed the rows filed under it by at least this much (second
# turns are counted), and without -ca it must not exceed them at all
TURNS_FLOOR = 10


def db_short():
    """3 families x 3 variants of 600-900 bases, the variants 3 % apart"""
    return synth.make_gene_db(3, 3, 600, 900, 0.06, seed=SEEDS["A"][0])


def db_long():
    """2 templates of 6 000 bases, 5 % apart"""
    return synth.make_gene_db(1, 2, 6000, 6000, 0.05, seed=SEEDS["L"][0])


def _turn(s, start, n):
    """n bases of the circular template s from `start` on"""
    return s[(start + np.arange(n)) % len(s)].astype(np.uint8)


def _subst(r, rate, rng):
    x = rng.random(len(r)) < rate
    r = r.copy()
    r[x] = (r[x] + rng.integers(1, 4, int(x.sum()), dtype=np.uint8)) & 3
    return r


def _strand(r, rng):
    return np.ascontiguousarray(synth.revcomp_codes(r) if rng.random() < 0.5 else r)


def reads_a(seqs, n=3000):
    """150-base reads, both strands, 1 % substitutions, 30 % with one 2-base insertion or deletion; every other read starts 10..140
    bases before the end of its template and goes on at its first base"""
    rng = np.random.default_rng(SEEDS["A"][1])
    out = []
    for i in range(n):
        s = seqs[int(rng.integers(0, len(seqs)))]
        start = len(s) - int(rng.integers(10, 141)) if i & 1 else int(rng.integers(0, len(s) - 150 + 1))
        r = _turn(s, start, 152)
        if rng.random() < 0.3:
            at = int(rng.integers(20, 130))
            if rng.random() < 0.5:
                r = np.concatenate([r[:at], rng.integers(0, 4, 2, dtype=np.uint8), r[at:]])
            else:
                r = np.concatenate([r[:at], r[at + 2:]])
        out.append(_strand(_subst(r[:150], 0.01, rng), rng))
    return out


def pairs_p(seqs, n=1500):
    """pairs of 100-base mates from inserts of 220-320 bases, 60 % of the inserts across the origin -> (mates 1, mates 2)"""
    rng = np.random.default_rng(SEEDS["P"][1])
    m1, m2 = [], []
    for i in range(n):
        s = seqs[int(rng.integers(0, len(seqs)))]
        ins = int(rng.integers(220, 321))
        start = len(s) - int(rng.integers(10, ins - 9)) if rng.random() < 0.6 else int(rng.integers(0, len(s) - ins + 1))
        frag = _turn(s, start, ins)
        a, b = frag[:100], synth.revcomp_codes(frag[-100:])
        if rng.random() < 0.5:
            a, b = b, a
        m1.append(np.ascontiguousarray(_subst(a, 0.01, rng)))
        m2.append(np.ascontiguousarray(_subst(b, 0.01, rng)))
    return m1, m2


def reads_l(seqs, n=200):
    """reads of 1 500-4 000 bases at 5 % substitutions from anywhere on the circle, both strands: chains of more than 64 and more than
    128 MEMs, and the 128-successor window"""
    rng = np.random.default_rng(SEEDS["L"][1])
    out = []
    for _ in range(n):
        s = seqs[int(rng.integers(0, len(seqs)))]
        L = int(rng.integers(1500, 4001))
        out.append(_strand(_subst(_turn(s, int(rng.integers(0, len(s))), L), 0.05, rng), rng))
    return out


def reads_o(seqs, n=400):
    """reads of 0.9-1.6 template lengths at 2 % from anywhere on the circle: a whole turn and more"""
    rng = np.random.default_rng(SEEDS["O"][1])
    out = []
    for _ in range(n):
        s = seqs[int(rng.integers(0, len(seqs)))]
        L = int(len(s) * (0.9 + 0.7 * rng.random()))
        out.append(_strand(_subst(_turn(s, int(rng.integers(0, len(s))), L), 0.02, rng), rng))
    return out


def reads_m(seqs, n=60):
    """reads of 1.15-1.65 turns of a 6 000-base template (7-10 kb on a 6 kb plasmid), the templates in turn, 3 % substitutions, an
    insertion or a deletion of 1-3 bases every 150-500 bases, both strands: more than one turn of a template that the pile-up cuts
    into units"""
    rng = np.random.default_rng(SEEDS["M"][1])
    out = []
    for i in range(n):
        s = seqs[i % len(seqs)]
        L = int(len(s) * (1.15 + 0.5 * rng.random()))
        r = _subst(_turn(s, int(rng.integers(0, len(s))), L), 0.03, rng)
        parts, p = [], 0
        while p < len(r):
            q = min(len(r), p + int(rng.integers(150, 500)))
            parts.append(r[p:q])
            u = rng.random()
            if u < 0.4:
                parts.append(rng.integers(0, 4, int(rng.integers(1, 4)), dtype=np.uint8))
            elif u < 0.8:
                q = min(len(r), q + int(rng.integers(1, 4)))
            p = q
        out.append(_strand(np.concatenate(parts), rng))
    return out


def make_input(tmp, key):
    """index files and FASTQ of input `key` (A, P, L, O, M) in directory tmp -> dict(tmp, prefix, fq, fq2, reads, runs)"""
    names, seqs = db_long() if key in "LM" else db_short()
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    fq, fq2, rd = str(tmp / "reads.fq"), None, None
    if key == "P":
        m1, m2 = pairs_p(seqs)
        fq2 = str(tmp / "reads_2.fq")
        synth.write_fastq(fq, m1, lens=None)
        synth.write_fastq(fq2, m2, lens=None)
    else:
        rd = {"A": reads_a, "L": reads_l, "O": reads_o, "M": reads_m}[key](seqs)
        synth.write_fastq(fq, rd, lens=None)
    return dict(tmp=tmp, key=key, prefix=prefix, fq=fq, fq2=fq2, reads=rd, runs={}, names=names, seqs=seqs)


def build_map():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)


def _input_args(s):
    return ["-ipe", s["fq"], s["fq2"]] if s["fq2"] else ["-i", s["fq"]]


def ref(s, extra, stdout=False):
    """the reference on input s with `extra`, once per option set -> stem of its files (standard output in stem + '.out' when asked)"""
    key = " ".join(extra)
    if key not in s["runs"]:
        stem = str(s["tmp"] / ("ref%d" % len(s["runs"])))
        # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
        with open(stem + ".out", "wb") as so:
            p = subprocess.run([KMA] + _input_args(s) + ["-o", stem, "-t_db", s["prefix"], "-t", "1"] + extra, stdout=so if stdout else subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=TIMEOUT)
        assert p.returncode in (0, 2), p.returncode
        s["runs"][key] = stem
    return s["runs"][key]


def run_map(s, tag, extra, env=None, stdout=False):
    """examples/kmahip_map on input s with `extra` -> stem of its files (standard output in stem + '.out' when asked)"""
    stem = str(s["tmp"] / ("got_" + tag))
    e = dict(os.environ)
    e.update(env or {})
    with open(stem + ".out", "wb") as so:
        p = subprocess.run([MAP] + _input_args(s) + ["-t_db", s["prefix"], "-o", stem] + extra, stdout=so if stdout else subprocess.DEVNULL,
                           stderr=subprocess.PIPE, env=e, timeout=TIMEOUT)
    assert p.returncode == 0, (extra, p.returncode, p.stderr[-600:])
    return stem


def frag(stem):
    return gzip.open(stem + ".frag.gz", "rb").read()


def files(stem):
    return tuple(open(stem + ext, "rb").read() for ext in (".res", ".fsa", ".aln")) + (frag(stem),)


def frag_rows(raw):
    return [x.split(b"\t") for x in raw.split(b"\n") if x]


def wrapped(raw):
    """rows of an inflated .frag.gz whose alignment ends before it starts (columns 4 and 5) -> (wrapped, all)"""
    rows = frag_rows(raw)
    return sum(int(r[4]) < int(r[3]) for r in rows), len(rows)


def assert_same_files(got, want):
    g, r = files(got), files(want)
    for name, a, b in zip((".res", ".fsa", ".aln", ".frag.gz"), g, r):
        assert a == b, name
    return r


def mapstat(stem):
    return [x for x in open(stem + ".mapstat", "rb").read().split(b"\n") if not x.startswith(b"## date\t") and not x.startswith(b"## command\t")]


def gz(stem, ext):
    return gzip.open(stem + ext, "rb").read()


def matrix_blocks(raw):
    """an inflated .mat.gz -> {template name: its rows as bytes, each ended by a newline}"""
    out, name, rows = {}, None, []
    for ln in raw.split(b"\n"):
        if ln.startswith(b"#"):
            name, rows = ln[1:], []
            out[name] = rows
        elif ln:
            rows.append(ln)
    return {k: b"".join(r + b"\n" for r in v) for k, v in out.items()}


def deepest_column(block):
    return max(sum(int(x) for x in ln.split(b"\t")[1:7]) for ln in block.split(b"\n") if ln)
