"""The plain-C restatement of the default mode's chain finder (oracle/chain.c) on the directed fixture tests/golden/chainroute
(make_golden_chainroute.py): reads aimed at the edges between the three device routes of stage 2 -- 288 / 289 k-mer starts, 32 / 33 anchors
on a strand, 16 / 17 candidate templates -- at k = 16 and k = 12. Every read's records must be the reference's own (`kma -s2`, default and
-ex_mode), and every row of cases.tsv must hold on the restatement of the anchor rule in tests/chainroute_util.py: the route counts that
tests/test_chainroute_gpu.py demands of the device stand on those rows."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chainroute_util as cu
import oracle
from kma_amd import formats, synth

KMA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "kma")


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = cu.load(tmp_path_factory.mktemp("chainroute"))
    f["odb"] = {k: oracle.OracleDB(f["prefix"][k]) for k in cu.KS}
    return f


@pytest.mark.parametrize("k,ex", cu.CONFIGS)
def test_oracle_reproduces_the_reference_tap_on_every_read(fx, k, ex):
    """bounds, score and templates of every record, in the reference's order, and the strand of the sequence it printed"""
    b = fx["batch"]
    by = cu.tap_by_read(fx["tap"][cu.cfg_name(k, ex)])
    mine = fx["odb"][k].scan_chain(b, exhaustive=ex)
    n_rec = 0
    for i, (nm, recs, case) in enumerate(zip(fx["names"], mine, fx["cases"])):
        want = by.get(nm, [])
        assert [(qs, qe, rf, tuple(int(t) for t in T)) for rf, er, qs, qe, T in recs] == [w[:4] for w in want], (nm, case["case"])
        assert len(want) == case[f"recs_{cu.cfg_name(k, ex)}"]
        L = int(b.length[i])
        for (rf, er, qs, qe, T), w in zip(recs, want):
            n_rec += 1
            seq = b.seq[b.seq_off[i]:b.seq_off[i] + ((L + 31) >> 5)]
            if er:
                seq, _ = oracle.rc_packed(seq, L, b.N[b.N_off[i]:b.N_off[i + 1]])
            assert np.array_equal(w[4], seq), nm
    assert n_rec == len(fx["tap"][cu.cfg_name(k, ex)]) > 200


def _aims(case, k):
    out = {}
    for a in case["aim"].split(";"):
        if a == "-":
            continue
        if a.startswith("k1") and ":" in a.split("=")[0]:
            kk, a = a.split(":", 1)
            if kk != f"k{k}":
                continue
        f, v = a.split("=")
        out[f] = int(v) if v.lstrip("-").isdigit() else v
    return out


@pytest.fixture(scope="module")
def analysed(fx):
    return {(k, ex): [cu.analyse(fx["odb"][k], rd, ex) for rd in fx["reads"]] for k, ex in cu.CONFIGS}


def test_every_row_of_the_case_table_holds_on_the_restated_anchor_rule(fx, analysed):
    """k-mer starts, anchors per strand, distinct templates and the route of every read at both k, default and exhaustive; and what the
    read was aimed at (its `aim`) in the default mode"""
    aimed = 0
    for (k, ex), rows in analysed.items():
        c = cu.cfg_name(k, ex)
        for case, a, rd in zip(fx["cases"], rows, fx["reads"]):
            got = dict(starts=a["starts"], aF=len(a["anchors"][0]), aR=len(a["anchors"][1]), nT=len(a["templates"]), route=cu.route_of(a))
            assert case["len"] == len(rd)
            assert (case[f"starts_k{k}"], case[f"aF_{c}"], case[f"aR_{c}"], case[f"nT_{c}"], case[f"route_{c}"]) == \
                (got["starts"], got["aF"], got["aR"], got["nT"], got["route"]), (case["name"], case["case"], c)
            if not ex:
                for f, v in _aims(case, k).items():
                    aimed += 1
                    assert got[f] == v or (v == "marked" and got[f].startswith("marked:a")), (case["name"], case["case"], c, f, v, got)
    assert aimed > 1000


def test_fixture_reaches_every_edge_it_is_meant_to(fx, analysed):
    """both sides of every limit of the fast route, every reason for a hand-over, and the bookkeeping next to the limits"""
    cases = fx["cases"]
    for k, ex in cu.CONFIGS:
        c = cu.cfg_name(k, ex)
        routes = {x[f"route_{c}"] for x in cases}
        assert routes == {"none", "fast", "marked:N", "marked:starts", "marked:aF", "marked:aR", "given_up"}, c
        fast = [x for x in cases if x[f"route_{c}"] == "fast"]
        # the limits themselves are reached from below, and passed by one
        assert max(x[f"starts_k{k}"] for x in fast) == cu.NPMAX
        assert cu.NPMAX + 1 in {x[f"starts_k{k}"] for x in cases if x[f"route_{c}"] == "marked:starts"}
        for s in ("aF", "aR"):
            assert {cu.AMAX - 1, cu.AMAX} <= {x[f"{s}_{c}"] for x in fast}
            assert cu.AMAX + 1 in {x[f"{s}_{c}"] for x in cases if x[f"route_{c}"] == "marked:" + s}
        assert any(x[f"aF_{c}"] == cu.AMAX and x[f"aR_{c}"] == cu.AMAX for x in fast)
        # one strand over the cap while the other has filed its anchors
        assert any(x[f"aF_{c}"] > cu.AMAX and 0 < x[f"aR_{c}"] <= cu.AMAX for x in cases)
        assert any(x[f"aR_{c}"] > cu.AMAX and 0 < x[f"aF_{c}"] <= cu.AMAX for x in cases)
        # the table of 16 templates: full at the first anchor and at a later one, on either strand, and exactly full
        given = [x for x in cases if x[f"route_{c}"] == "given_up"]
        assert all(x[f"nT_{c}"] > cu.TSLOTS for x in given) and all(x[f"nT_{c}"] <= cu.TSLOTS for x in fast)
        assert any(x[f"nT_{c}"] == cu.TSLOTS + 1 and x[f"aF_{c}"] + x[f"aR_{c}"] == 1 for x in given)
        assert any(x[f"nT_{c}"] == cu.TSLOTS + 1 and x[f"aF_{c}"] + x[f"aR_{c}"] > 1 for x in given)
        assert sum(x[f"nT_{c}"] == cu.TSLOTS for x in fast) >= 12
        assert {x[f"nT_{c}"] for x in fast} >= {1, 2, 3, 4, 5, 15, 16}
        # the pass border of 144 starts and reads of k - 1, k, k + 1 bases
        assert {143, 144, 145, 0, 1, 2} <= {x[f"starts_k{k}"] for x in cases}
    # the n-th anchor opens at the read's last start, n = 32 and 33
    for k in cu.KS:
        rows = analysed[(k, 0)]
        for n in (cu.AMAX, cu.AMAX + 1):
            assert any(len(s) == n and s[-1][0] == a["starts"] - 1 for a in rows for s in a["anchors"]), (k, n)
    # k - 1, k and k + 1 missed starts between two hits of one list, the hit before in the pass before (starts below 144) or not
    for k in cu.KS:
        seen = set()
        for case, a in zip(cases, analysed[(k, 0)]):
            if case["group"] != "gaps":
                continue
            A = [s for s in a["anchors"] if s][0]
            flip = not a["anchors"][0]
            if len(A) == 1:          # a substitution: exactly k missed starts, one anchor
                seen.add((k, None))
            else:
                missed = A[1][0] - A[0][1] - 1
                seen.add((missed, (A[0][1] < 144) != (A[1][0] < 144), flip))
        assert (k, None) in seen
        for missed in (k - 1, k + 1):
            for flip in (False, True):
                assert {(missed, True, flip), (missed, False, flip)} <= seen, (k, missed, flip, seen)
    # the 16 templates of F17's second window have the highest home slots of LdsMap the database offers: the probe wraps
    row = [x for x in cases if x["case"] == "one_anchor_16+"][0]
    a = analysed[(16, 0)][cases.index(row)]
    slots = sorted(((t * 0x9E3779B1) & 0xFFFFFFFF) >> 28 for t in a["templates"])
    assert len(slots) == 16 and slots[0] >= 13 and slots.count(15) >= 2
    # strand ties, tie anchors and reads cut into several records, from the oracle's own log
    log = (ctypes.c_int * 4).in_dll(oracle.lib(), "orc_chain_log")
    for k in cu.KS:
        for case_name, idx, least in (("tie_8+8+", 1, 1), ("tie_8+8-", 1, 1), (f"k{k}_tie_anchor_16+", 2, 1), (f"k{k}_tie_anchor_15-", 2, 1),
                                      ("chimeric_6+5+5+", 3, 1), ("chimeric_10+6r-", 3, 1)):
            i = [x["case"] for x in cases].index(case_name)
            for j in range(4):
                log[j] = 0
            recs = fx["odb"][k].scan_chain(formats.pack_ragged([fx["reads"][i]]))[0]
            assert log[idx] >= least, (k, case_name, list(log))
            if idx == 1:          # 8 + 8: the reverse strand's templates follow negated
                assert len(recs) == 1 and recs[0][0] < 0 and sum(t > 0 for t in recs[0][4]) == 8 and sum(t < 0 for t in recs[0][4]) == 8
            if idx == 2:
                assert len(recs) == 1 and len(recs[0][4]) == int(case_name.split("_")[-1][:2])


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    prefix = str(tmp_path_factory.mktemp("chainroute_wide") / "wide")
    return prefix, cu.wide_set(prefix)


@pytest.mark.parametrize("ex", [0, 1])
def test_oracle_equals_reference_binary_on_the_wide_database(wide, tmp_path, ex):
    """the reads of tests/test_chainroute_gpu.py's database with 32-bit value lists through `kma -s2` on the same index"""
    prefix, reads = wide
    odb = oracle.OracleDB(prefix)
    assert cu.is_u32(odb)
    b = formats.pack_ragged(reads)
    want = cu.flat(odb.scan_chain(b, exhaustive=ex))
    fq = str(tmp_path / "r.fq")
    synth.write_fastq(fq, reads)
    out = subprocess.run([KMA, "-i", fq, "-o", str(tmp_path / "o"), "-t_db", prefix, "-t", "1", "-s2"] + (["-ex_mode"] if ex else []), check=True,
                         stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    by = cu.tap_by_read(formats.parse_s2(out)[0])
    tap = [(i, rf, qs, qe, T) for i in range(b.n) for qs, qe, rf, T, _ in by.get(f"r{i}", [])]
    assert [(i, rf, qs, qe, T) for i, rf, er, qs, qe, T in want] == tap and len(tap) > 200
