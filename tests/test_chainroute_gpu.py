"""The three device routes of the default mode's stage 2 (kmahip_chain_device: prefilter + chain_anchor_kernel + chain_fast_kernel, the
long-read route, chain_kernel) on the directed fixture tests/golden/chainroute and on a database wide enough for 32-bit value lists. The
reads sit on either side of every limit of the fast route (288 k-mer starts, 32 anchors on a strand, 16 candidate templates) at k = 16 and
k = 12. Under every switch that moves reads between the routes the records must be the oracle's and the reference's own, and
kmahip_chain_get_route_counts must report exactly the routes cases.tsv names (tests/test_chainroute_oracle.py holds those rows to the
restated anchor rule without a GPU)."""
import gzip
import os

import numpy as np
import pytest

import chainroute_util as cu
import oracle
from kma_amd import binding, formats
from test_chain_gpu import _records, _run_both, _with_env

pytestmark = pytest.mark.gpu

SWITCHES = [{}, {"KMAHIP_CHAIN": "slow"}, {"KMAHIP_CHAIN_LONG": "0"}, {"KMAHIP_CHAIN_ORDER": "0"}, {"KMAHIP_CHAIN_CHUNK": "64"},
            {"KMAHIP_CHAIN_CHUNK": "64", "KMAHIP_CHAIN_OVERLAP": "0"}]
ROUTES = ("none", "fast", "marked:N", "marked:starts", "marked:aF", "marked:aR", "given_up")


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = cu.load(tmp_path_factory.mktemp("chainroute"))
    f["odb"] = {k: oracle.OracleDB(f["prefix"][k]) for k in cu.KS}
    f["has_N"] = [bool((rd == 4).any()) for rd in f["reads"]]
    return f


def _run(db, batch, ex, env):
    def call():
        return _records(db.scan_chain(batch, exhaustive=ex)), db.get_chain_route_counts()
    return _with_env(env, call)


def _check_all_switches(db, batch, ex, want, routes, has_N):
    for env in SWITCHES:
        got, counts = _run(db, batch, ex, env)
        assert got == want, (env, ex)
        assert counts == cu.counts_of(routes, has_N, env), (env, ex, counts)
        if env.get("KMAHIP_CHAIN") == "slow":          # (no read is handed over: chain_kernel takes them all as they come)
            assert counts == dict(reads=len(routes), marked=0, given_up=0, long=0, lane=len(routes))
        else:
            assert counts["marked"] + counts["given_up"] == counts["long"] + counts["lane"]


@pytest.mark.parametrize("k,ex", cu.CONFIGS)
def test_records_and_route_counts_under_every_switch(fx, k, ex):
    """same records, same order within a read, no read twice, whichever route takes the read; the counts of every call equal to what the
    case table names; and the reference's tap, record for record"""
    c = cu.cfg_name(k, ex)
    b = fx["batch"]
    routes = [x[f"route_{c}"] for x in fx["cases"]]
    want = cu.flat(fx["odb"][k].scan_chain(b, exhaustive=ex))
    by = cu.tap_by_read(fx["tap"][c])
    tap = [(i, rf, qs, qe, T) for i, nm in enumerate(fx["names"]) for qs, qe, rf, T, _ in by.get(nm, [])]
    assert [(i, rf, qs, qe, T) for i, rf, er, qs, qe, T in want] == tap and len(tap) > 200
    db = binding.KmaHipDB(fx["prefix"][k])
    try:
        _check_all_switches(db, b, ex, want, routes, fx["has_N"])
    finally:
        db.close()


@pytest.mark.parametrize("k", cu.KS)
def test_each_reason_for_a_hand_over_on_its_own(fx, k):
    """the reads of one route alone in a call: N's, starts, anchors on the forward and on the reverse strand, a table full at the first
    anchor and at a later one. The reads chain_fast_kernel gives up are the 17-template ones and none of the 16-template ones; a read
    given up leaves no record behind and is not lost. Last, a read of 288 starts alone among reads of under 60 bases."""
    cases, reads = fx["cases"], fx["reads"]
    c = cu.cfg_name(k, 0)
    groups = {r: [i for i, x in enumerate(cases) if x[f"route_{c}"] == r] for r in ROUTES}
    given = groups.pop("given_up")
    groups["given_up:first"] = [i for i in given if cases[i][f"aF_{c}"] + cases[i][f"aR_{c}"] == 1]
    groups["given_up:later"] = [i for i in given if cases[i][f"aF_{c}"] + cases[i][f"aR_{c}"] > 1]
    groups["exactly_16"] = [i for i, x in enumerate(cases) if x[f"route_{c}"] == "fast" and x[f"nT_{c}"] == cu.TSLOTS]
    groups["exactly_17"] = [i for i in given if cases[i][f"nT_{c}"] == cu.TSLOTS + 1]
    groups["given_up_among_fast"] = sorted(given + groups["fast"][:70])
    short = [i for i, x in enumerate(cases) if k <= x["len"] < 60 and x[f"route_{c}"] == "fast"]
    longest = [i for i, x in enumerate(cases) if x[f"starts_k{k}"] == cu.NPMAX and x[f"route_{c}"] == "fast"][:1]
    groups["one_long_among_short"] = short[:5] + longest + short[5:]
    db = binding.KmaHipDB(fx["prefix"][k])
    try:
        for name, idx in groups.items():
            assert len(idx) >= (6 if name == "one_long_among_short" else 2), name
            b = formats.pack_ragged([reads[i] for i in idx])
            routes = [cases[i][f"route_{c}"] for i in idx]
            want = cu.flat(fx["odb"][k].scan_chain(b))
            got, counts = _run(db, b, 0, {})
            assert got == want, name
            assert counts == cu.counts_of(routes, [fx["has_N"][i] for i in idx]), (name, counts)
            if name.startswith("marked"):
                assert counts["marked"] == len(idx) and counts["given_up"] == 0, name
            if name.startswith("given_up:") or name == "exactly_17":
                assert counts["given_up"] == counts["long"] == len(idx) and len({r[0] for r in got}) == len(idx), name
            if name in ("exactly_16", "fast", "none", "one_long_among_short"):
                assert counts["marked"] == counts["given_up"] == 0, name
    finally:
        db.close()


def test_a_lane_chains_a_read_behind_one_it_gave_up(fx):
    """chain_fast_kernel runs at most 262 144 lanes, each on every 262 144th read of its chunk: the fixture 1 300 times over gives 34 000
    lanes a second read, one in thirteen of them behind a read the lane gave up with its table full (what that read left in LdsMap must
    not reach the next one), as the reads come and ordered by their anchors. Every copy's records must be the first copy's."""
    k, times = 16, 1300
    b = fx["batch"]
    n, words, nN = b.n, len(b.seq), len(b.N)
    assert n * times > 262144 + 30000
    big = formats.ReadBatch(np.tile(b.seq, times), np.concatenate([(b.seq_off[:-1][None, :] + words * np.arange(times)[:, None]).reshape(-1), [words * times]]).astype(np.int64),
                            np.tile(b.length, times), np.tile(b.N, times),
                            np.concatenate([(b.N_off[:-1][None, :] + nN * np.arange(times)[:, None]).reshape(-1), [nN * times]]).astype(np.int64))
    routes = [x["route_k16"] for x in fx["cases"]]
    one = cu.counts_of(routes, fx["has_N"])
    want = cu.flat(fx["odb"][k].scan_chain(b))
    cols = [np.array([w[j] for w in want]) for j in range(5)]
    T = np.concatenate([np.array(w[5], np.int32) for w in want])
    db = binding.KmaHipDB(fx["prefix"][k])
    try:
        for env in ({"KMAHIP_CHAIN_ORDER": "0"}, {}):
            o, counts = _with_env(env, lambda: (db.scan_chain(big), db.get_chain_route_counts()))
            assert counts == {f: v * times for f, v in one.items()}, env
            assert len(o["read"]) == len(want) * times
            assert np.array_equal(o["read"], (cols[0][None, :] + n * np.arange(times)[:, None]).reshape(-1)), env
            for j, f in ((1, "rc_flag"), (2, "emit_rc"), (3, "q_start"), (4, "q_end")):
                assert np.array_equal(o[f], np.tile(cols[j], times)), (env, f)
            assert np.array_equal(o["T"], np.tile(T, times)), env
    finally:
        db.close()


@pytest.mark.parametrize("k", cu.KS)
def test_whole_default_mode_run_equals_reference_files(fx, tmp_path, k):
    """examples/kmahip_map -chain on the fixture's reads against the files the reference wrote without -1t1, in one piece and in batches of
    97 reads"""
    for env in ({}, {"KMAHIP_MAP_BATCH": "97"}):
        res, fsa, frag = _run_both(tmp_path, fx["prefix"][k], fx["fastq"], (), env)
        assert res == open(os.path.join(fx["dir"], f"chain_k{k}.res"), "rb").read(), env
        assert fsa == gzip.open(os.path.join(fx["dir"], f"chain_k{k}.fsa.gz")).read(), env
        assert frag == gzip.open(os.path.join(fx["dir"], f"chain_k{k}.frag.gz")).read(), env
        assert frag.count(b"\n") > 150


# ---- 32-bit value lists ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp("chainroute_wide") / "wide")
    reads = cu.wide_set(prefix)
    odb = oracle.OracleDB(prefix)
    assert cu.is_u32(odb)
    return dict(prefix=prefix, reads=reads, odb=odb, batch=formats.pack_ragged(reads), has_N=[bool((r == 4).any()) for r in reads])


@pytest.mark.parametrize("ex", [0, 1])
def test_wide_database_records_and_route_counts_under_every_switch(wide, ex):
    """the 32-bit branch of ank_n / ank_at and the 32-bit head chain_anchor_kernel stores, on all routes: lists of 1, 2, 3, 16 and 17
    templates, 31 / 32 / 33 anchors on either strand, N's, 289 starts"""
    b, odb = wide["batch"], wide["odb"]
    an = [cu.analyse(odb, rd, ex) for rd in wide["reads"]]
    routes = [cu.route_of(a) for a in an]
    assert set(routes) == set(ROUTES)
    fast = [a for a, r in zip(an, routes) if r == "fast"]
    assert {1, 2, 3, 16} <= {len(a["templates"]) for a in fast} and 17 in {len(a["templates"]) for a, r in zip(an, routes) if r == "given_up"}
    for s in (0, 1):
        assert {cu.AMAX - 1, cu.AMAX} <= {len(a["anchors"][s]) for a in fast}
        assert cu.AMAX + 1 in {len(a["anchors"][s]) for a, r in zip(an, routes) if r == ("marked:aR" if s else "marked:aF")}
    want = cu.flat(odb.scan_chain(b, exhaustive=ex))
    assert len(want) > 200
    db = binding.KmaHipDB(wide["prefix"])
    try:
        _check_all_switches(db, b, ex, want, routes, wide["has_N"])
    finally:
        db.close()
