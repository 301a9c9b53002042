"""The plain-Python restatement of the QC report and of `kma trim` (tests/qc_util.py) against everything the reference recorded in
tests/golden/qc (made by tests/golden/make_golden_qc.py): the report byte for byte, the trimmed reads byte for byte. No GPU, no library:
this holds the checker itself to the reference, so that the other tests may use it on inputs made on the spot."""
import json

import pytest

import qc_util


@pytest.mark.parametrize("case", sorted(qc_util.CASES))
def test_restatement_matches_every_recorded_file(case):
    for setting in qc_util.SETTINGS:
        mine = qc_util.restate(case, setting)
        assert mine["json"].encode() == qc_util.gold(case, setting, "json"), (case, setting)
        assert mine["fq"] == qc_util.gold(case, setting, "fq"), (case, setting)
        paired = bool(qc_util.CASES[case][1] or qc_util.CASES[case][2])
        assert (qc_util.gold(case, setting, "int_fq") is not None) == paired
        if paired:
            assert mine["int_fq"] == qc_util.gold(case, setting, "int_fq"), (case, setting)


def test_the_set_holds_what_it_is_there_for():
    """the properties the generator asserted when it recorded the files, read back from the files themselves"""
    rep = {(c, s): json.loads(qc_util.gold(c, s, "json")) for c in qc_util.CASES for s in qc_util.SETTINGS}
    assert rep["long", "default"]["Length Resolution"] > 1
    assert {qc_util.restate(c, "default")["qc"].n50_branch() for c in ("long", "p33", "one")} == {"scaled", "plain", "maxlen"}
    q = rep["uni", "default"]["Q Distribution"]
    assert sum(q) == 66 and any(q[b] != 3 for b in range(20, 42))          # a uniform-quality read outside its nominal bin
    # a read kept by the plain rule and dropped under -qc: long enough as trimmed, too short without its N's
    plain = qc_util.restate("long", "default", report=False)["fq"].count(b"\n+\n")
    assert plain > rep["long", "default"]["Fragment Count"]
    assert rep["pe", "default"]["Fragment Count"] != rep["pe", "default"]["Sequence Count"] and qc_util.gold("pe", "default", "fq")
    assert sum(qc_util.restate(c, "eq25ml40")["both_ends"] for c in ("p33", "long")) > 0
    assert "Minimum Q" not in rep["p33", "ml1000"] and "E(Q)" not in rep["p33", "ml1000"] and "Minimum Q" in rep["long", "ml1000"]
    assert rep["p33+p64", "default"]["Phred Scale"] == 64                  # the last file's
    assert rep["p33", "mi25clip"]["End Trim Q"] == 25 and rep["p33", "mi25clip"]["5'-clip"] == 3 and rep["p33", "mi25clip"]["3'-clip"] == 2
