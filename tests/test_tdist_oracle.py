"""The plain Python restatement of `kma dist` (tests/dist_util.py: reader, counts, thirteen measures, file layout) reproduces every file
the reference recorded under tests/golden/tdist/ byte for byte, over every form of index the fixtures hold. No GPU."""
import os

import numpy as np
import pytest

import dist_util as du

RUNS = [(case, tag) for case, (_, _, runs) in du.CASES.items() for tag in runs]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tdist_oracle")


@pytest.mark.parametrize("case,tag", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_restatement_reproduces_the_recorded_file(case, tag, tmp):
    v, N, D = du.restated(case, tmp)
    methods, fmt = du.run_flags(du.CASES[case][2][tag])
    want = du.golden(case, tag)
    got = du.phy(N, D, v.names, methods, fmt)
    assert len(got) == len(want) == du.phy_size(v.DB_size, os.path.getsize(os.path.join(du.GOLDEN, case + ".name")), methods, fmt)
    assert got == want


def test_fixtures_hold_what_they_are_there_for(tmp):
    v, N, D = du.restated("edge", tmp)
    lists = v.lists()
    lens = {len(ids) for ids, _ in lists.values()}
    assert {1, 2, 63, 64, 65} <= lens
    mults = [m for _, m in lists.values()]
    assert max(mults) >= 10 and 1 in mults
    assert N[69] == N[70] == D[70, 69] > 0 and D[71].sum() == 0 < N[71]
    assert all((np.diff(ids) > 0).all() for ids, _ in lists.values())          # the lists of an index ascend
    w = du.restated("wide", tmp)[0]
    assert 300 in {len(ids) for ids, _ in w.lists().values()}
    forms = {c: du.restated(c, tmp)[0] for c in ("edge_k20", "edge_TG", "edge_m12", "edge_mega")}
    assert forms["edge_k20"].mlen == 20 and forms["edge_TG"].prefix_len == 2 and forms["edge_m12"].flag != 0 and forms["edge_mega"].mega
    assert [du.restated(c, tmp)[0].DB_size for c in ("one", "two")] == [2, 3]


def test_a_short_file_is_the_wrong_format(tmp):
    p = du.unpack_index("two", tmp)
    raw = open(p + ".comp.b", "rb").read()
    q = str(tmp / "short")
    for cut in (20, 60, len(raw) - 200):
        with open(q + ".comp.b", "wb") as f:
            f.write(raw[:cut])
        with open(q + ".name", "wb") as f:
            f.write(b"a\nb\n")
        with pytest.raises(du.WrongFormat):
            du.Values(q)
