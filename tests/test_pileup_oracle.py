"""The plain reference of the pile-up, column by column (oracle/assembly.c: orc_assembly_columns, oracle.Assembly.columns / matrix_text)
and the builder of hand-made traces (pile_util), without a GPU. The columns are pinned on a file the reference itself wrote: set V of
the count-matrix tests, tests/golden/matvcf_v/ref.mat."""
import os

import numpy as np
import pytest

import oracle
import pile_util as pu
from kma_amd import formats
from matvcf_sets import v_reads, v_templates

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matvcf_v")


@pytest.fixture(scope="module")
def vdb(tmp_path_factory):
    names, seqs = v_templates()
    prefix = str(tmp_path_factory.mktemp("pile_v") / "db")
    formats.write_index(prefix, names, seqs)
    return oracle.OracleDB(prefix), names, seqs


def test_columns_equal_the_reference_matrix(vdb):
    """set V traced by the oracle's aligner, piled up in the reference's order (the last read first), read back and rendered: the
    reference's own `.mat.gz` of that input, byte for byte -- template rows, both chains of insertion columns, every count"""
    odb, names, seqs = vdb
    reads = v_reads(seqs)
    al = oracle.OracleAligner(odb)
    oa = oracle.Assembly(odb, 2, len(seqs[1]))
    for rd in reversed(reads):
        tr = al.align_trace(rd, 2)
        assert tr is not None
        oa.add(tr, rd)
    counts, ins = oa.columns()
    assert counts.shape == (oa.call()["asm_len"], 6) and int(ins.sum()) == 3 and len(counts) == 303
    text = oa.matrix_text(seqs[1])
    want = open(os.path.join(GOLDEN, "ref.mat"), "rb").read()
    assert b"#hand1\n" + text + b"\n" == want
    # the insertion columns stand where the reads put them: two behind position 80, one behind position 125
    assert list(np.nonzero(ins)[0]) == [81, 82, 128]
    assert b"\n-\t" in text


def test_columns_of_an_empty_ring(vdb):
    odb, _, seqs = vdb
    counts, ins = oracle.Assembly(odb, 1, 300).columns()
    assert counts.shape == (300, 6) and not counts.any() and not ins.any()


def test_stats_row_of_the_builder():
    st = pu.stats_of(100, 90, 3, [("=", 8), ("I", 2), ("X", 1), ("D", 4), ("=", 5)], q_len=3 + 16 + 7)
    #                score start end          aln clip clip match tGaps qGaps mapQ
    assert list(st) == [1, 90, 90 + 18 - 100, 20, 3, 7, 14, 2, 4, 0]
    assert list(pu.stats_of(64, 0, 0, [("=", 128)], 128))[1:4] == [0, 64, 128]
    assert pu.runs_of(pu.ops_of([("=", 8), ("I", 2), ("D", 70000)])) == [("=", 8), ("I", 2), ("D", 70000)]


def test_stats_row_round_trip_on_traced_reads(vdb):
    """the row rebuilt from start, clips and runs of the oracle aligner's own traces of set V is the aligner's row"""
    import itertools
    odb, _, seqs = vdb
    al = oracle.OracleAligner(odb)
    keys = ("score", "start", "end", "aln_len", "clip_start", "clip_end", "match", "tGaps", "qGaps", "mapQ")
    for rd in v_reads(seqs):
        tr = al.align_trace(rd, 2)
        runs = [(c, len(list(g))) for c, g in itertools.groupby(tr["cols"].decode())]
        assert {c for c, _ in runs} >= {"=", "X", "I", "D"} or len(runs) > 3
        assert list(pu.stats_of(300, tr["start"], tr["clip_start"], runs, len(rd), tr["score"], tr["mapQ"])) == [tr[k] for k in keys]


def test_trimming_of_gap_runs_at_the_ends():
    """assembly.c:1340-1354 as read_runs restates it: a leading D run moves the start, a leading I run the read position, gap runs
    behind the last aligned pair fall away, and the oracle piles up the trimmed trace exactly as the whole one"""
    assert pu.trimmed(10, [("D", 3), ("=", 5), ("I", 2)]) == (13, 0, [("=", 5)])
    assert pu.trimmed(10, [("I", 2), ("D", 1), ("X", 5), ("D", 2), ("I", 1)]) == (11, 2, [("X", 5)])
    assert pu.trimmed(10, [("D", 4)]) == (14, 0, [])


def test_trimmed_trace_piles_up_like_the_whole_one(vdb):
    odb, _, seqs = vdb
    rng = np.random.default_rng(5)
    whole = pu.make(seqs[0], 40, 2, [("I", 2), ("D", 3), ("=", 20), ("I", 1), ("X", 2), ("=", 9), ("D", 2), ("I", 3)], rng)
    start, skip, runs = pu.trimmed(40, pu.runs_of(whole["ops"]))
    assert (start, skip) == (43, 2)
    a, b = oracle.Assembly(odb, 1, 300), oracle.Assembly(odb, 1, 300)
    a.add(whole, whole["read"])
    cut = dict(cols="".join(c * n for c, n in runs).encode(), start=start, score=1, clip_start=0)
    b.add(cut, whole["read"][2 + skip:])
    (ca, ia), (cb, ib) = a.columns(), b.columns()
    assert np.array_equal(ca, cb) and np.array_equal(ia, ib)
    # columns 43 .. 73 hold one base each, the chain in front of column 63 one column
    assert ca.sum() == 31 + 1 and list(np.nonzero(ia)[0]) == [63] and not ca[:43].any()


def test_builder_reads_belong_to_their_runs(vdb):
    """the read `make` writes: template bases on `=`, other bases on X, an N where asked; stored reverse-complemented and filed with
    the rc flag or under the negative template id"""
    odb, _, seqs = vdb
    rng = np.random.default_rng(6)
    s = seqs[2]
    tr = pu.make(s, 290, 1, [("=", 12), ("X", 2), ("I", 2), ("=", 6)], rng, clip_end=2, n_at=(13,))
    rd = tr["read"][1:]
    assert np.array_equal(rd[:12], s[(290 + np.arange(12)) % 300]) and rd[12] != s[2] and rd[13] == 4
    assert np.array_equal(rd[16:22], s[4:10]) and len(tr["read"]) == 1 + 22 + 2 and tr["stats"][5] == 2
    b = pu.Batch([(3, tr, False), (3, tr, True), (3, tr, True)])
    assert list(b.tmpl) == [3, 3, -3] and list(b.rc) == [0, 1, 0]
    assert b.order(3, 0) == [2, 1, 0] and b.order(3, 2) == [1, 0, 2]
    assert list(b.ops_off) == [0, 4, 8] and len(b.ops) == 12


def test_second_turn_is_counted_by_the_ring_walk(vdb):
    """a trace of two turns and forty columns: every column twice, the first forty three times; an insertion run the second turn
    brings finds the depth the first turn left"""
    odb, _, seqs = vdb
    rng = np.random.default_rng(7)
    s = seqs[0]
    tr = pu.make(s, 250, 0, [("=", 350), ("I", 2), ("=", 290)], rng)
    oa = oracle.Assembly(odb, 1, 300)
    oa.add(tr, tr["read"])
    counts, ins = oa.columns()
    depth = counts.sum(axis=1)
    tpos = np.nonzero(~ins)[0]
    assert len(counts) == 302 and list(np.nonzero(ins)[0]) == [300, 301]          # in front of column 0 (250 + 350 = 2 * 300): printed behind column 299
    d = depth[tpos]
    want = np.full(300, 2)
    want[(250 + np.arange(40)) % 300] = 3
    assert np.array_equal(d, want)
    # the new columns start from min(depth of the site, depth in front - 1) = min(1, 2 - 1) gaps and hold the read's base
    assert list(depth[ins]) == [2, 2] and list(counts[ins][:, 5]) == [1, 1]
