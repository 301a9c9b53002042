"""The Python restatement of homology reduction (tests/hom_util.py) against what the reference printed and wrote for every case of
tests/golden/homology/ (`kma index -Sparse ... -hq / -ht / -and`, recorded by tests/golden/make_golden_homology.py). No GPU. Strings and
integers; the ratios are the reference's own double expressions printed with %f, so the report is compared byte for byte."""
import pytest

import hom_util as hu
import sparse_index_util as siu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("homology_oracle")


@pytest.mark.parametrize("case", list(hu.CASES))
def test_restatement_gives_the_recorded_report_and_index(case, tmp):
    mine = hu.built(case)
    ref = siu.Files(siu.unpack(hu.GOLDEN, case, tmp, with_seq=False))
    assert mine.report == hu.report(case)
    assert mine.length_b() == ref.length_b and mine.name_file() == ref.name_file
    assert mine.lists == ref.lists and (mine.prefix_len, mine.prefix, mine.DB_size) == (ref.prefix_len, ref.prefix, ref.DB_size)
    k, sp, ml, hq, ht, a = hu.CASES[case]
    assert ref.k == k and len(mine.report.split(b"\n")[0].split(b"\t")) == (4 if ht is None else 6)


def test_the_fixture_holds_its_edges():
    """the edges the generator asserted, read back from the stored reports"""
    n6, n5, t9 = (hu.parse_report(hu.report(c)) for c in ("none_hq06", "none_hq05", "none_ht09"))
    assert n6["chimera_A_then_B"] == [3, 0.5, 1] and n6["chimera_B_then_A"] == [4, 0.5, 2]          # kept at -hq 0.6, the tie names the half met first
    assert n5["chimera_A_then_B"] == [1, 0.5, 1]                                                      # -hq 0.5 rejects exactly 0.5
    assert t9["copy_of_A_with_one_N"] == [1, 1.0, 1, 0.97265, 1]
    assert n6["read_of_S"][1] == 1.0 and "no_window_at_all" not in n6
    tg = hu.parse_report(hu.report("TG_hq06"))
    assert "no_TG_window" not in tg and "k_plus_one_bases" not in tg and "no_TG_window" in n6
    rows = hu.built("TG_ht08_hq08").rows
    assert len(rows) == 40 and sum(r[0] for r in rows) == 32 and any(r[3] != r[6] for r in rows if r[3])


def test_thresholds_of_one_are_the_plain_build():
    with pytest.raises(AssertionError):
        hu.Hom(hu.INPUT, "TG", k=16)
    plain = siu.Built(hu.INPUT, "TG", k=16)
    assert plain.DB_size == 38          # (40 candidates, three without a window behind TG; slot 0)
