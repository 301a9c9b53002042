"""The three capacity retries of the run paths (pipeline_util.h: retry_cand_room, retry_seed_room, retry_run_room), reached at test
size: examples/kmahip_map with KMAHIP_CAP_START=64 (the candidate lists and the run pool start at 64 entries) and
KMAHIP_SCAN_POOL_PER_READ=1 (the candidate pool starts at a sixteenth of its size), in every mode and on every run path. Each run
must say which capacities it raised (KMAHIP_DEBUG_TIMING) and still write the reference's files byte for byte.

Values used: synth.make_gene_db(n_families=30, variants=20, seed=3) and 600 reads of 150 bp (300 pairs for -ipe); for -Mt1, 40 reads
of 1.1-2.5 kb against genes of 1.5-3 kb. One pool int per read makes the pool overflow where one rank scans the 600 reads even with
five variants a family: the pool is 600 + 600/8 + 1024 = 1699 ints, and the inline slots of the 1200 strand items alone would take
2400. A rank of `-gpus 2` has 300 reads, 1361 ints and 1200 inline slots, which leaves 161 ints for the lists longer than two
entries: with five variants (0-4 % apart) too few reads tie three ways and the pool held (measured: no retry line), so the families
have 20 variants, a fifth of a percent apart, and most reads tie between several of them. The all-candidates scan of the pairs gives
every strand item a list. The doublings needed stay below the four allowed: four of them are today's size.
The default mode finds its templates with the chain finder, whose own retry is not among the three: its runs grow the run pool only,
and -Mt1 has no stage 2 at all."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from kma_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")

POOL = b"[kmahip] candidate pool raised to"
LISTS = b"[kmahip] candidate lists raised to"
RUNS = b"[kmahip] alignment run pool raised to"

# mode -> (switches, input, the retry lines its capacities print)
MODES = {
    "1t1": (["-1t1"], "se", (POOL, LISTS, RUNS)),
    "default": ([], "se", (RUNS,)),
    "pe_1t1": (["-1t1"], "pe", (POOL, LISTS, RUNS)),
    "Mt1": (["-Mt1", "1"], "long", (RUNS,)),
}
PATHS = {
    "session": ([], {}),
    "one_batch": ([], {"KMAHIP_MAP_ONE_BATCH": "1"}),
    "gpus2": (["-gpus", "2"], {"KMAHIP_COMM": "shm", "KMAHIP_SHARE_GPU": "1"}),
}
KNOBS = {"KMAHIP_CAP_START": "64", "KMAHIP_SCAN_POOL_PER_READ": "1", "KMAHIP_DEBUG_TIMING": "1"}


def _index(tmp, name, names, seqs):
    prefix = str(tmp / name)
    synth.write_fasta(prefix + ".fsa", names, seqs)
    subprocess.run([KMA, "index", "-i", prefix + ".fsa", "-o", prefix], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return prefix


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    tmp = tmp_path_factory.mktemp("capacity")
    names, seqs = synth.make_gene_db(n_families=30, variants=20, seed=3)
    short = _index(tmp, "db", names, seqs)
    reads, *_ = synth.make_reads(seqs, 600, read_len=150, sub_rate=0.01, seed=5)
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, [r for r in reads], prefix="q")
    m1, m2, _ = synth.make_pairs(seqs, 300, seed=9)
    r1, r2 = str(tmp / "r1.fq"), str(tmp / "r2.fq")
    synth.write_fastq(r1, list(m1), prefix="p")
    synth.write_fastq(r2, list(m2), prefix="p")
    rng = np.random.default_rng(13)
    lnames, lseqs = synth.make_gene_db(n_families=6, variants=3, len_lo=1500, len_hi=3000, seed=32)
    long_db = _index(tmp, "ldb", lnames, lseqs)
    lreads = []
    for i in range(40):          # (three in four out of template 1, the one -Mt1 names)
        g = lseqs[0 if i % 4 else int(rng.integers(0, len(lseqs)))]
        lreads.append(synth.make_long_reads(g, 1, read_len=int(rng.integers(1100, min(2500, len(g)))), seed=300 + i)[0])
    lfq = str(tmp / "long.fq")
    synth.write_fastq(lfq, lreads, prefix="l")
    return {"tmp": tmp, "se": (["-i", fq], short), "pe": (["-ipe", r1, r2], short), "long": (["-i", lfq], long_db), "ref": {}}


def _reference(inputs, mode):
    """the reference's files for a mode: made once, shared by the three run paths"""
    if mode not in inputs["ref"]:
        flags, kind, _ = MODES[mode]
        files, db = inputs[kind]
        out = str(inputs["tmp"] / ("ref_" + mode))
        subprocess.run([KMA] + files + ["-o", out, "-t_db", db, "-t", "1"] + flags, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        inputs["ref"][mode] = out
    return inputs["ref"][mode]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("mode", list(MODES))
def test_every_capacity_grows_from_a_small_start_and_the_files_equal_the_reference(inputs, mode, path):
    flags, kind, lines = MODES[mode]
    files, db = inputs[kind]
    more, env = PATHS[path]
    ref = _reference(inputs, mode)
    got = str(inputs["tmp"] / f"got_{mode}_{path}")
    e = dict(os.environ)
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    e.update(env)
    e.update(KNOBS)
    g = subprocess.run([MAP] + more + files + ["-t_db", db, "-o", got] + flags, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert g.returncode == 0, g.stderr.decode()[-2000:]
    for line in lines:
        assert line in g.stderr, (line, g.stderr.decode()[-2000:])          # (a run that never reaches the retry cannot pass)
    assert open(got + ".res", "rb").read() == open(ref + ".res", "rb").read()
    assert open(got + ".fsa", "rb").read() == open(ref + ".fsa", "rb").read()
    assert gzip.open(got + ".frag.gz").read() == gzip.open(ref + ".frag.gz").read()
