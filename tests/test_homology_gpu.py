"""kmahip_index_build_sparse_hom (`kmahip_index -Sparse ... -hq / -ht / -and`, binding.index_build(..., hom_q=, hom_t=, hom_and=, report=))
against the reference's recorded reports and indexes of tests/golden/homology/: the report byte for byte and the index files as
test_sparse_index_gpu.py compares them, at every setting, also under a column block of 8 templates and a pair list of 4 entries; the
device's per-row integers against the restatement of tests/hom_util.py on a seeded synthetic database; the program's standard output;
the reference run live where it is built. Integers and the reference's own double expressions: no tolerance."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import hom_util as hu
import proxi_util
import sparse_index_util as siu
from kma_amd import binding, formats, synth

pytestmark = pytest.mark.gpu
EXTS = (".comp.b", ".length.b", ".name", ".seq.b")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("homology_gpu")


@pytest.fixture(scope="module")
def refs(tmp):
    """case -> prefix of the reference's recorded index, unpacked once"""
    return {case: siu.unpack(hu.GOLDEN, case, tmp) for case in hu.CASES}


def same_index(got, ref):
    """our files under prefix `got` against the reference's under `ref`"""
    for ext in (".length.b", ".name"):
        assert open(got + ext, "rb").read() == open(ref + ext, "rb").read(), ext
    a, b = formats.read_comp_b(got + ".comp.b"), formats.read_comp_b(ref + ".comp.b")
    assert (a.DB_size, a.mlen, a.kmersize, a.flag, a.n, a.prefix_len, a.prefix) == (b.DB_size, b.mlen, b.kmersize, b.flag, b.n, b.prefix_len, b.prefix)
    assert formats.comp_db_mapping(a) == formats.comp_db_mapping(b)
    assert a.v_index == b.v_index
    siu.seq_words_equal(got + ".seq.b", ref + ".seq.b", formats.read_lengths(ref)[1:])


def build_and_compare(case, refs, tmp, tag):
    got = str(tmp / ("%s_%s" % (tag, case)))
    binding.index_build(hu.INPUT, got, report=got + ".tsv", **hu.build_kwargs(case))
    assert open(got + ".tsv", "rb").read() == hu.report(case)
    same_index(got, refs[case])


@pytest.mark.parametrize("case", list(hu.CASES))
def test_report_and_index_equal_the_reference(case, refs, tmp):
    build_and_compare(case, refs, tmp, "got")
    assert sorted(f for f in os.listdir(tmp) if f.startswith("got_" + case + ".")) == sorted("got_%s%s" % (case, e) for e in EXTS + (".tsv",))


@pytest.mark.parametrize("knobs", [{"KMAHIP_HOM_BLOCK": "8"}, {"KMAHIP_HOM_PAIRS": "4"}, {"KMAHIP_HOM_BLOCK": "1", "KMAHIP_HOM_PAIRS": "1"}],
                         ids=["block_8", "pairs_4", "block_1_pairs_1"])
def test_column_blocks_and_a_regrown_pair_list(knobs, refs, tmp, monkeypatch):
    """40 templates in column blocks of 8 (rows that end inside a block, at its edge and behind it) and a pair list that starts at 4
    entries (every setting flags more pairs than that, so the list is made again at the counted size)"""
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    for case in hu.CASES:
        build_and_compare(case, refs, tmp, "knob")


def write_fasta(path, names, seqs):
    synth.write_fasta(path, names, seqs)
    return path


@pytest.mark.parametrize("sparse, kw, block", [("TG", dict(hom_q=0.7, hom_t=0.7), "64"), ("TG", dict(hom_q=0.8, hom_t=0.6, hom_and=True), None),
                                               ("-", dict(hom_q=0.75), "100")], ids=["TG_or_block64", "TG_and", "none_query_block100"])
def test_per_row_integers_equal_the_restatement(sparse, kw, block, tmp, monkeypatch):
    """300 templates, 50 families of 6 at 0 ... 4 % from their first member: kept flag, thisKlen, the winners' counts, ulen and ids of
    every row, before ids are given out"""
    if block:
        monkeypatch.setenv("KMAHIP_HOM_BLOCK", block)
    short = sparse == "-"
    names, seqs = synth.make_gene_db(50, 6, len_lo=200 if short else 600, len_hi=400 if short else 1500, seed=2026)
    fa = write_fasta(str(tmp / ("synth_%d.fsa" % short)), names, seqs)
    want = np.array(hu.Hom(fa, sparse, k=16, **kw).rows, np.uint32)
    got = binding.index_hom_rows(fa, k=16, sparse=sparse, **kw)
    assert want.shape == (300, 7) and 50 <= int(want[:, 0].sum()) < 300 and want[:, 2].any() and want[:, 4].any()
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:10]


@pytest.mark.parametrize("case", ["TG_hq06", "none_ht045_hq045_and", "TG_hq06_ML300"])
def test_the_program_prints_the_recorded_report(case, refs, tmp):
    proxi_util.build_map()
    out = str(tmp / ("prog_" + case))
    p = subprocess.run([hu.INDEX, "-i", hu.INPUT, "-o", out] + hu.kma_args(case), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout == hu.report(case)
    same_index(out, refs[case])


def test_everything_rejected_ends_like_the_empty_database(tmp):
    """-hq 0: every template gets its line and goes (qualcheck.c:181 with bestQ = 0), then `DB is empty`"""
    proxi_util.build_map()
    out = str(tmp / "empty")
    p = subprocess.run([hu.INDEX, "-i", hu.INPUT, "-o", out, "-Sparse", "TG", "-hq", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 1 and b"DB is empty" in p.stderr, (p.returncode, p.stderr)
    lines = p.stdout.split(b"\n")[:-1]
    assert len(lines) == 37 and all(l.endswith(b"\t0\t0.000000\t0") for l in lines) and lines[0] == b"gene_A\t0\t0.000000\t0"
    with pytest.raises(binding.KmaHipError, match="DB is empty"):
        binding.index_build(hu.INPUT, out, sparse="TG", hom_q=0.0)


def test_thresholds_of_one_give_the_plain_sparse_build(tmp):
    a, b = str(tmp / "plain"), str(tmp / "one")
    binding.index_build(hu.INPUT, a, sparse="TG")
    binding.index_build(hu.INPUT, b, sparse="TG", hom_q=1.0, hom_t=1.0, hom_and=True, report=b + ".tsv")
    for ext in EXTS:
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    assert open(b + ".tsv", "rb").read() == b""
    want = siu.Built(hu.INPUT, "TG", k=16)
    assert siu.Files(b).length_b == want.length_b() and want.DB_size == 38


def test_the_reference_run_live_agrees(tmp):
    """the fixture and a synthetic database of 300 templates through oracle/_ref/kma and through the program: the same standard output,
    the same index"""
    if not os.path.exists(hu.KMA):
        pytest.skip("oracle/_ref/kma not built")
    proxi_util.build_map()
    fix = str(tmp / "db.fsa")
    with open(fix, "wb") as f:
        f.write(gzip.open(hu.INPUT).read())
    names, seqs = synth.make_gene_db(50, 6, seed=77)
    syn = write_fasta(str(tmp / "live.fsa"), names, seqs)
    for tag, fa, args in (("fix", fix, ["-Sparse", "TG", "-ht", "0.7", "-hq", "0.3"]), ("syn_or", syn, ["-Sparse", "TG", "-hq", "0.9", "-ht", "0.9"]),
                          ("syn_and", syn, ["-Sparse", "-", "-hq", "0.9", "-ht", "0.9", "-and"]), ("syn_q", syn, ["-Sparse", "ATG", "-hq", "0.8", "-ML", "700"])):
        ref, got = str(tmp / ("ref_live_" + tag)), str(tmp / ("got_live_" + tag))
        r = subprocess.run([hu.KMA, "index", "-i", fa, "-o", ref] + args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120)
        p = subprocess.run([hu.INDEX, "-i", fa, "-o", got] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode in (0, 2) and p.returncode == 0, (tag, r.returncode, p.returncode, p.stderr)
        assert p.stdout == r.stdout and len(r.stdout.split(b"\n")) > 30, tag
        same_index(got, ref)
