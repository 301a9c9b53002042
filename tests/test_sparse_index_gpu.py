"""kmahip_index_build_sparse (`kmahip_index -Sparse`, binding.index_build(..., sparse=...)) against the reference's recorded indexes:
the files themselves for every case of tests/golden/sparse_index/, and what an index is for: SparseDB, `kmahip_map -Sparse` and the
reference binary map the fixture reads against an index we built and give the recorded `.spa` files. Integers only: no tolerance."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import proxi_util
import sparse_index_util as siu
import sparse_util as su
from kma_amd import binding, formats

pytestmark = pytest.mark.gpu
SE = {"TG": "se_TG", "none": "se_none", "ATG": "se_ATG"}          # index name under tests/golden/sparse/se -> case of sparse_util / sparse_index_util


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("sparse_index_gpu")


def same_index(got, ref, seq=True):
    """our files under prefix `got` against the reference's under `ref`"""
    for ext in (".length.b", ".name"):
        assert open(got + ext, "rb").read() == open(ref + ext, "rb").read(), ext
    a, b = formats.read_comp_b(got + ".comp.b"), formats.read_comp_b(ref + ".comp.b")
    assert (a.DB_size, a.mlen, a.kmersize, a.flag, a.n, a.prefix_len, a.prefix) == (b.DB_size, b.mlen, b.kmersize, b.flag, b.n, b.prefix_len, b.prefix)
    assert formats.comp_db_mapping(a) == formats.comp_db_mapping(b)
    assert a.v_index == b.v_index                                    # equal lists are stored once in both
    if seq:
        siu.seq_words_equal(got + ".seq.b", ref + ".seq.b", formats.read_lengths(ref)[1:])
    return a


@pytest.mark.parametrize("case", list(siu.CASES))
def test_build_equals_the_reference_files(case, tmp):
    k, sp, ml = siu.CASES[case]
    ref = siu.unpack(siu.GOLDEN, case, tmp)
    got = str(tmp / ("got_" + case))
    binding.index_build(siu.inputs(), got, k=k or 16, sparse=sp, min_len=ml)
    a = same_index(got, ref)
    assert (a.prefix_len, a.prefix) == ((0, 1) if sp == "-" else (len(sp), siu.encode(sp)))
    assert sorted(f for f in os.listdir(tmp) if f.startswith("got_" + case)) == ["got_%s%s" % (case, e) for e in (".comp.b", ".length.b", ".name", ".seq.b")]


def test_one_template_and_no_template(tmp):
    """a database of one template (every unique pair carries one id) against the restatement, with a prefix and without; and a
    database in which no template holds a window"""
    rng = np.random.default_rng(5)
    fa = str(tmp / "one.fsa")
    with open(fa, "w") as f:
        f.write(">only one\n%s\n" % "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 701)))
    for sp in ("TG", "-"):
        got = str(tmp / "one")
        binding.index_build(fa, got, sparse=sp)
        want, have = siu.Built(fa, sp, k=16), siu.Files(got)
        assert have.length_b == want.length_b() and have.name_file == want.name_file() and have.lists == want.lists
        assert (have.prefix_len, have.prefix) == (want.prefix_len, want.prefix) and want.ulengths[1] > (30 if sp == "TG" else 1300)
    with open(fa, "w") as f:
        f.write(">no window\n%s\n>nor here\n%s\n" % ("AG" * 40, "GGA" * 30))
    with pytest.raises(binding.KmaHipError, match="DB is empty"):
        binding.index_build(fa, str(tmp / "empty"), sparse="TG")


# ---- an index we built, in use --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ours(tmp):
    """index name -> prefix of the index examples/kmahip_index -Sparse built from tests/golden/se/db.fsa.gz"""
    proxi_util.build_map()
    made = {}

    def get(name):
        if name not in made:
            p = str(tmp / ("ours_" + name))
            arg = {"TG": ["TG"], "none": ["-"], "ATG": ["ATG"]}[name]
            subprocess.run([siu.INDEX, "-i", siu.OLD[SE[name]][2], "-o", p, "-k", "16", "-Sparse"] + arg, check=True, timeout=120)
            made[name] = p
        return made[name]
    return get


def counted(prefix, case):
    sdb = binding.SparseDB(prefix)
    for path in su.reads_path(case):
        with binding.Ingest(path) as ing:
            while True:
                got = ing.next(1 << 20)
                if got is None:
                    break
                sdb.count(got[0])
    return sdb


@pytest.mark.parametrize("name", list(SE))
def test_our_index_feeds_sparse_mapping(name, ours, tmp):
    case = SE[name]
    mine, ref = ours(name), su.unpack_index(case, tmp)
    same_index(mine, ref, seq=False)          # (the fixtures of sparse mapping hold no .seq.b: a sparse run reads none)
    idx = su.Index(mine)
    with counted(mine, case) as a, counted(ref, case) as b:
        (ka, ca, na), (kb, cb, nb) = a.counts(), b.counts()
        assert na == nb and dict(zip(ka.tolist(), ca.tolist())) == dict(zip(kb.tolist(), cb.tolist())) and ca.any()
        for ss in "qcd":
            want = su.golden(case, "spa_" + ss)
            assert su.spa_text(idx, a.rows(ss=ss)) == want
            out = str(tmp / ("mine_%s_%s" % (name, ss)))
            a.write(out + ".sdb.spa", ss=ss)
            assert open(out + ".sdb.spa").read() == want
            p = subprocess.run([su.MAP, "-i", su.reads_path(case)[0], "-o", out, "-t_db", mine, "-Sparse", "-ss", ss], stdout=subprocess.DEVNULL,
                               stderr=subprocess.PIPE, timeout=120)
            assert p.returncode == 0, p.stderr
            assert open(out + ".spa").read() == want and len(want.split("\n")) > 3


@pytest.mark.parametrize("name", list(SE))
def test_the_reference_reads_our_index(name, ours, tmp):
    if not os.path.exists(su.KMA):
        pytest.skip("oracle/_ref/kma not built")
    case = SE[name]
    fq = str(tmp / "reads.fq")
    with open(fq, "wb") as f:
        f.write(gzip.open(su.reads_path(case)[0]).read())
    for ss in "qcd":
        out = str(tmp / ("kma_%s_%s" % (name, ss)))
        p = subprocess.run([su.KMA, "-i", fq, "-o", out, "-t_db", ours(name), "-Sparse", "-ss", ss, "-t", "1"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=120)
        assert p.returncode in (0, 2)          # (the reference ORs errno into its exit status, kma.c:1630)
        assert open(out + ".spa").read() == su.golden(case, "spa_" + ss)
