"""The plain-C restatement of the long-read aligner (oracle/align.c: anker_rc, chainSeeds, the three windows, NW / NW_band with
traceback) on the directed fixture tests/golden/ltclass (make_golden_ltclass.py): every read yields one DP problem of a chosen mode, size
and band, or none, under two scoring schemes. Each read's record must be the reference's own SAM record, and the problems the restatement
solves on the way must be the ones cases.tsv names -- the class expectations of tests/test_ltclass_gpu.py stand on those."""
import ctypes

import pytest

import golden_util
import oracle


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return golden_util.load_ltclass(tmp_path_factory.mktemp("ltclass"))


def _band(q_l, t_l):
    band = abs(t_l - q_l) + 64
    return 0 if q_l <= band or t_l <= band else band


@pytest.mark.parametrize("scheme", ["s1", "s2"])
def test_oracle_reproduces_the_reference_sam_on_every_read(fx, scheme):
    """flag, POS, MAPQ (capped at 254), CIGAR and AS of every read; None exactly where the reference's CIGAR is '*'. The flag stays 0 on
    the reverse strand in this mode (anker_rc leaves it alone), so the strand is checked against the fixture's own note of it."""
    odb = oracle.OracleDB(fx["prefix"])
    golden_util.set_scheme(odb.rw, fx["schemes"][scheme])
    al = oracle.OracleAligner(odb)
    log = (ctypes.c_int32 * 1024).in_dll(oracle.lib(), "orc_dp_log")
    n_log = ctypes.c_int32.in_dll(oracle.lib(), "orc_dp_n")
    compared = mapped = 0
    for nm, rd, case in zip(fx["names"], fx["reads"], fx["cases"]):
        flag, rname, pos, mapq, cigar, AS = fx["sam"][scheme][nm]
        n_log.value = 0
        o, is_rc, _ = al.align_trace_mt1(rd, 1)
        problems = [tuple(log[4 * x:4 * x + 4]) for x in range(n_log.value)]
        compared += 1
        assert (case["fate"] == "map") == (cigar != "*"), nm
        if o is None:
            assert cigar == "*" and flag == 4, (nm, case["case"])
            assert not case["n_dp"] and not problems, (nm, case["case"], problems)
            continue
        mapped += 1
        assert (0, "template20k", o["start"] + 1, min(254, o["mapQ"]), o["cigar"], o["score"]) == (flag, rname, pos, mapq, cigar, AS), (nm, case["case"])
        assert is_rc == (case["strand"] == "-"), (nm, case["case"])
        # the one problem the read aims at: mode, template rows, query columns, band (0: full matrix)
        want = [(case["k"], case["t_l"], case["q_l"], case["band"])] if case["n_dp"] else []
        assert problems == want, (nm, case["case"], problems, want)
        if case["n_dp"]:
            assert case["band"] == _band(case["q_l"], case["t_l"]), nm
    assert compared == len(fx["names"]) == len(fx["cases"]) == 258
    assert mapped == sum(1 for c in fx["cases"] if c["fate"] == "map") == 256


def test_fixture_covers_what_it_is_meant_to(fx):
    """the fixture's own shape: both strands in every case, the modes of all three windows, degenerate joins, dropped reads, ties whose
    records differ from a plain diagonal, and the second scheme's 16-bit gate between 200 and 400"""
    cases = fx["cases"]
    by_case = {}
    for c in cases:
        by_case.setdefault((c["group"], c["case"]), set()).add(c["strand"])
    assert all(s == {"+", "-"} for s in by_case.values())
    assert {c["k"] for c in cases if c["n_dp"]} == {-2, -1, 0, 1, 2}
    assert sum(1 for c in cases if c["group"] == "degen" and not c["n_dp"]) == 12
    assert sum(1 for c in cases if c["fate"] == "drop") == 2
    assert 200 <= fx["schemes"]["s2"]["lane_tq"] <= 400 < fx["schemes"]["s1"]["lane_tq"]
    # rows + columns on either side of the gate: a lane class below it, none above it
    gate = [c for c in cases if c["group"] == "gate"]
    tq = fx["schemes"]["s2"]["lane_tq"]
    assert {c["q_l"] + c["t_l"] for c in gate} == {tq, tq + 1}
    # the edges of lane class 8: 256 / 257 query columns under the default turn cap, a band of 140 / 141 only with the cap lifted
    by_name = {c["case"]: c for c in cases if c["strand"] == "+"}
    assert (by_name["q256_t256"]["lane_s1"], by_name["q257_t257"]["lane_s1"]) == (8, -1)
    assert (by_name["q150_t226"]["lane_s1"], by_name["q150_t226"]["lanefree_s1"], by_name["q150_t227"]["lanefree_s1"]) == (-1, 8, -1)
    for c in gate:
        assert (c["lane_s2"] >= 0) == (c["q_l"] + c["t_l"] <= tq) and c["lane_s1"] >= 0, c
    # the ties: every one of them has a gap or a mismatch to place
    for c in cases:
        if c["group"] == "ties":
            cig = fx["sam"]["s1"][c["name"]][4]
            assert any(op in cig for op in "IDX"), (c["name"], cig)
