"""The plain Python restatement of sparse mapping (tests/sparse_util.py) against the reference's own output, recorded under
tests/golden/sparse/ by tests/golden/make_golden_sparse.py: its k-mer tap (`kma -Sparse -s1`), its `# Total number of matches` line and
its `.spa` files for the three -ss orders. This pins the restatement the GPU tests compare the device with. No GPU."""
import numpy as np
import pytest

import sparse_util as su


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("sparse_oracle")


@pytest.mark.parametrize("case", list(su.CASES))
def test_kmer_walk_reproduces_the_tap(case, tmp):
    """translateToKmersAndDump: the k-mers of every read, both strands, as a multiset and in count"""
    idx, found, Ntot, kmers, _ = su.restated(case, tmp)
    want = su.golden(case, "kmers")
    assert Ntot == len(want)
    assert np.array_equal(np.sort(np.array(kmers, np.uint64)), want)


@pytest.mark.parametrize("case", list(su.CASES))
def test_matches_line(case, tmp):
    """Nhits.tot of collect_Kmers and Ntot, as the reference prints them"""
    idx, found, Ntot, _, _ = su.restated(case, tmp)
    st = su.State(idx, found)
    assert "# Total number of matches: %d of %d kmers\n" % (st.hits[1], Ntot) == su.golden(case, "matches")


@pytest.mark.parametrize("ss", ["q", "c", "d"])
@pytest.mark.parametrize("case", list(su.CASES))
def test_spa_byte_for_byte(case, ss, tmp):
    idx, found, Ntot, _, _ = su.restated(case, tmp)
    assert su.spa_text(idx, su.rows(idx, found, Ntot, ss=ss)) == su.golden(case, "spa_" + ss)


def test_the_fixtures_cover_what_they_are_for(tmp):
    """the three -ss orders differ on se/TG, a quarter of w's rows were changed by a withdrawal, the edge reads are all there"""
    q, c, d = (su.golden("se_TG", "spa_" + s) for s in "qcd")
    assert len({q, c, d}) == 3
    for ss in "qc":
        rows = [x.split("\t") for x in su.golden("w", "spa_" + ss).split("\n")[1:] if x]
        assert 4 * sum(1 for r in rows if r[5] != r[8]) >= len(rows)
    lens = sorted(len(r) for r in su.restated("e", tmp)[4])
    k, p = 16, 2
    for L in (k, k + p, k + p + 1, 33, 64, 65):
        assert L in lens
    idx = su.restated("se_none", tmp)[0]
    assert (idx.prefix_len, idx.prefix) == (0, 1)


def test_intpos_bin_reads_the_length_slot():
    """the reference's binary search as it stands: a list of two templates above 2 "holds" template 2, its own length"""
    assert su.intpos_bin([2, 5, 7], 2) == 0
    assert su.intpos_bin([2, 5, 7], 5) == 1 and su.intpos_bin([2, 5, 7], 7) == 2 and su.intpos_bin([2, 5, 7], 6) == -1
    assert su.intpos_bin([1, 9], 1) == -1 and su.intpos_bin([3, 4, 5, 6], 3) == -1
