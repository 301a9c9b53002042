"""Shared by the tests of proximity matching (`-proxi f`, `-ill`): the seeded inputs of the whole runs and the command lines that
examples/kmahip_map refuses. No test lives here."""
import os
import subprocess

import numpy as np

from kma_amd import formats, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")


def reads(seqs, n, rng):
    """the read generator of test_reference_binary_gpu.py (test_whole_run_equals_reference_binary), re-stated: substitutions, indels,
    unmappable and partly foreign reads, an N here and there, ragged lengths, both strands"""
    out = []
    for i in range(n):
        s = seqs[int(rng.integers(0, len(seqs)))]
        L = int(rng.integers(60, 251))
        a = int(rng.integers(0, max(1, len(s) - L)))
        r = s[a:a + L].copy()
        u = rng.random()
        if u < 0.03:                                   # unmappable
            r = rng.integers(0, 4, L, dtype=np.uint8)
        elif u < 0.08:                                 # foreign end (either side)
            j = rng.integers(0, 4, int(rng.integers(20, 140)), dtype=np.uint8)
            r = np.concatenate([r, j]) if rng.random() < 0.5 else np.concatenate([j, r])
        elif u < 0.16:                                 # an indel or two
            parts, p = [], 0
            while p < len(r):
                e = min(len(r), p + int(rng.integers(25, 110)))
                parts.append(r[p:e])
                v = rng.random()
                if v < 0.45:
                    parts.append(rng.integers(0, 4, int(rng.integers(1, 5)), dtype=np.uint8))
                elif v < 0.9:
                    e = min(len(r), e + int(rng.integers(1, 5)))
                p = e
            r = np.concatenate(parts)
        x = rng.random(len(r)) < 0.008
        r = r.copy()
        r[x] = (r[x] + rng.integers(1, 4, int(x.sum()), dtype=np.uint8)) & 3
        if rng.random() < 0.03:
            r[int(rng.integers(0, len(r)))] = 4        # an N
        if rng.random() < 0.5:
            r = synth.revcomp_codes(r)
        out.append(np.ascontiguousarray(r.astype(np.uint8)))
    return out


# the inputs of the whole runs: (families, variants, database seed, reads, read seed)
INPUTS = {
    "a": (12, 12, 102, 20000, 2),     # twelve variants per family: lists of up to twelve, the inline slots and the pool
    "b": (2, 80, 105, 4000, 5),       # eighty variants: lists of up to eighty, beyond the second tier (64 slots): the wavefront-per-item finish
    "c": (6, 24, 106, 6000, 6),       # twenty-four: lists of up to twenty, the second tier without overflow
}


def make_input(tmp, key):
    """index files and FASTQ of input `key` in directory tmp -> dict(tmp, prefix, fq)"""
    fam, var, db_seed, n, read_seed = INPUTS[key]
    names, seqs = synth.make_gene_db(fam, var, 500, 1300, 0.04, seed=db_seed)
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, reads(seqs, n, np.random.default_rng(read_seed)), lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=fq, runs={})


def refused_commands(tmp):
    """-> [(arguments behind `kmahip_map`, what the message must name)]: every combination proximity matching is not built for. The
    program refuses them before it opens a file or a device."""
    fq, r2, o, db = str(tmp / "r.fq"), str(tmp / "r2.fq"), str(tmp / "out"), str(tmp / "db")
    base = ["-t_db", db, "-o", o]
    se = ["-i", fq] + base
    return [
        (["-ipe", fq, r2] + base + ["-1t1", "-proxi", "0.9"], "paired input"),
        (["-ipe", fq, r2] + base + ["-ill"], "paired input"),
        (["-int", fq] + base + ["-1t1", "-proxi", "-0.9"], "interleaved input"),
        (se + ["-proxi", "0.9"], "without -1t1"),
        (se + ["-ill", "-Mt1", "1"], "-Mt1"),
        (se + ["-1t1", "-proxi", "0.9", "-mem_mode"], "-mem_mode"),
        (se + ["-ill", "-gpus", "2"], "-gpus N"),
        (se + ["-1t1", "-proxi", "0.9", "-s1dev"], "-s1dev"),
        (se + ["-ill", "-sam", "4"], "-sam n"),
    ]


def build_map():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
