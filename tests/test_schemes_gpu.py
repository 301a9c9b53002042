"""The device OFF the reference's default scoring scheme, kernel family by kernel family, through library calls, exact against the oracle
(which tests/test_oracle_schemes.py pins to the reference under the same schemes): stage 2 in both modes, stage 3a on both kernels with
the diagonal shortcut on and off, the traceback on its four routes and the long-read pipeline, the couples, and the -cge preset of the
host program. The schemes and the planted reads are those of tests/scheme_sets.py: links of gap_m_max and gap_m_max + 1 mismatches, the
tie scheme, tails whose shifted diagonal is clean, reads over template ends, an N in a link. `db.params.rw` and the oracle's Rewards are
filled by the same helper; the oracle's results are computed once per scheme."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import scheme_sets as ss
import threshold_sets as ts
from kma_amd import binding
from test_oracle_schemes import couple_records, couples_input, inputs, oracle_run, record_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("KMAHIP_ALIGN_FAST", "KMAHIP_ALIGN_DIAG", "KMAHIP_ALIGN_LONG", "KMAHIP_TRACE", "KMAHIP_TRACE_LDS", "KMAHIP_LT_LANE", "KMAHIP_CHAIN", "KMAHIP_CHAIN_LONG")


def _env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _open(inp, scheme):
    db = binding.KmaHipDB(inp["prefix"])
    ss.apply(db.params.rw, ss.SCHEMES[scheme])
    return db


# ---- stage 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", list(ss.SCHEMES))
def test_stage2_equals_the_oracle_under_every_scheme(tmp_path_factory, monkeypatch, scheme):
    """scan_se_kernel and what stands in front of it (-1t1), and the chain finder on its three routes (the default mode: bridge_same_set
    and the chain weights read M, MM, W1, U and Wl), record for record"""
    inp = inputs(tmp_path_factory)
    res = oracle_run(inp, scheme, "device")
    b = res["batch"]
    want = ts.flat_chain_records(res["odb"].scan_chain(b))
    assert len(want) >= b.n - 10
    db = _open(inp, scheme)
    try:
        _env(monkeypatch, {})
        got, _ = db.map_se(b)
        for a, c, nm in zip(res["scan"], got, ("rc_flag", "flag", "T_off", "T")):
            assert np.array_equal(a, c), (scheme, nm)
        for env in ({"KMAHIP_CHAIN": "slow"}, {"KMAHIP_CHAIN_LONG": "0"}, {}):
            _env(monkeypatch, env)
            o = db.scan_chain(b)
            have = [(int(o["read"][x]), int(o["rc_flag"][x]), int(o["emit_rc"][x]), int(o["q_start"][x]), int(o["q_end"][x]),
                     tuple(int(t) for t in o["T"][o["T_off"][x]:o["T_off"][x + 1]])) for x in range(len(o["read"]))]
            assert have == want, (scheme, env)
    finally:
        db.close()


# ---- stage 3a --------------------------------------------------------------------------------------------------------------------------
def _same_3a(res, got, what):
    (rc_flag, flag, T_off, T), h = got
    o = res["o"]
    for a, c in zip(res["scan"], (rc_flag, flag, T_off, T)):
        assert np.array_equal(a, c), what
    assert np.array_equal(o["n_hits"], h["n_hits"]), what
    assert np.array_equal(o["best_score"], h["best_score"]), what
    assert np.array_equal(o["out_flag"], h["flag"]), what
    for i in np.nonzero(o["n_hits"] > 0)[0]:
        s, c = int(T_off[i]), int(o["n_hits"][i])
        for key in ("tmpl", "start", "end", "score"):
            assert np.array_equal(o[key][s:s + c], h[key][s:s + c]), (what, int(i), key)
    assert np.array_equal(o["alignment_scores"], h["alignment_scores"]), what
    assert np.array_equal(o["uniq_alignment_scores"], h["uniq_alignment_scores"]), what


@pytest.mark.parametrize("scheme", list(ss.SCHEMES))
def test_stage3a_equals_the_oracle_with_and_without_the_diagonal_shortcut(tmp_path_factory, monkeypatch, scheme):
    """align_tasks_kernel (KMAHIP_ALIGN_FAST=0) and align_fast_kernel with its class queues, each with nw_diagonal as the host allows it
    and switched off (KMAHIP_ALIGN_DIAG=0): everything tests/test_align_gpu.py compares at the defaults. That the shortcut ran where the
    scheme allows it and nowhere else shows in the tasks left pending on the class queues: fewer with the shortcut under a plain scheme,
    the same number under one the predicate rejects."""
    inp = inputs(tmp_path_factory)
    res = oracle_run(inp, scheme, "device")
    s = ss.SCHEMES[scheme]
    db = _open(inp, scheme)
    counts = {}
    try:
        for fast in ("0", "1"):
            for diag in ("0", None):
                env = {"KMAHIP_ALIGN_FAST": fast}
                if diag is not None:
                    env["KMAHIP_ALIGN_DIAG"] = diag
                _env(monkeypatch, env)
                _same_3a(res, db.map_se(res["batch"]), (scheme, env))
                if fast == "1":
                    counts["off" if diag == "0" else "on"] = db.get_align_queue_counts()
    finally:
        db.close()
    print(scheme, "stage 3a class queues, shortcut on:", counts["on"], "off:", counts["off"])
    if ss.is_plain(s):
        assert counts["on"]["pending"] < counts["off"]["pending"], (scheme, counts)
    else:
        assert counts["on"]["pending"] == counts["off"]["pending"] > 0, (scheme, counts)
    # the restated predicate agrees with what the counts show, and its figure is the host's
    assert binding.diag_gap_m_max(_rw(s)) == ss.gap_m_max(s) and (ss.gap_m_max(s) >= 0) == ss.is_plain(s), scheme


def _rw(s):
    rw = binding.Rewards()
    ss.apply(rw, s)
    return rw


# ---- traceback -------------------------------------------------------------------------------------------------------------------------
_KEYS = ("score", "start", "end", "aln_len", "clip_start", "clip_end", "match", "tGaps", "qGaps", "mapQ")
TRACE_ROUTES = {"two_pass": {}, "lanes1": {"KMAHIP_TRACE": "lanes1"}, "lds": {"KMAHIP_TRACE_LDS": "1"}, "pipeline": {"KMAHIP_TRACE": "pipeline"}}


def _got(stats, off, nops, ops, i):
    st = stats[i]
    if not st.any():
        return None
    out = dict(zip(_KEYS, (int(x) for x in st)))
    out["cigar"] = binding.cigar_from_runs(ops[off[i]:off[i] + nops[i]], int(st[4]), int(st[5]))
    return out


def _want(o):
    if o is None:
        return None
    o = dict(o)
    o.pop("cols")
    return o


def _front(db, res, what):
    """stages 2 - 3b on the device, checked against the oracle's: what the traceback is then run on"""
    b = res["batch"]
    (rc_flag, flag, T_off, T), h = db.map_se(b)
    cc = db.conclave_se(b.length, T_off, h)
    assert np.array_equal(cc["tmpl"], res["cc"]["tmpl"]) and np.array_equal(cc["w_scores"], res["cc"]["w_scores"]), what
    ok = np.zeros(int(db.info.DB_size), np.uint8)
    for r in db.res_rows(cc["w_scores"]):
        ok[r.template_id] = r.significant
    assert np.array_equal(ok, res["ok"]), what
    return h, cc, ok


def _same_traces(res, traces, what):
    stats, off, nops, ops = traces
    kept = np.zeros(res["batch"].n, bool)
    for i, _, _ in res["filed"]:
        got = _got(stats, off, nops, ops, i)
        assert got == _want(res["trace"][i]), (what, i)
        kept[i] = got is not None
    assert not stats[~kept].any(), what
    return int(kept.sum())


@pytest.mark.parametrize("scheme", list(ss.SCHEMES))
def test_traceback_equals_the_oracle_on_every_route(tmp_path_factory, monkeypatch, scheme):
    """trace_kernel in two passes (the first settles the reads whose DP problems diag_emit's proof covers), in one pass
    (KMAHIP_TRACE=lanes1), with the LDS pass in between (KMAHIP_TRACE_LDS=1), and the long-read kernels on the short reads
    (KMAHIP_TRACE=pipeline): every figure, mapQ and the CIGAR of every read. Under a plain scheme the first pass puts off some reads and
    not all; under the others and in one pass it puts off none, because it does not run."""
    inp = inputs(tmp_path_factory)
    res = oracle_run(inp, scheme, "device")
    s = ss.SCHEMES[scheme]
    b = res["batch"]
    db = _open(inp, scheme)
    put_off = {}
    try:
        _env(monkeypatch, {})
        h, cc, ok = _front(db, res, scheme)
        for route, env in TRACE_ROUTES.items():
            _env(monkeypatch, env)
            traces = db.align_trace(b, h["rc"], cc["tmpl"], ok)
            put_off[route] = db.get_trace_put_off()
            assert _same_traces(res, traces, (scheme, route)) > 0.95 * b.n
    finally:
        db.close()
    print(scheme, "traceback, reads put off per route:", put_off, "of", b.n)
    for route in ("two_pass", "lds"):
        if ss.is_plain(s):
            assert 0 < put_off[route][0] < b.n, (scheme, put_off)
        else:
            assert put_off[route] == (0, 0), (scheme, put_off)
    assert put_off["lanes1"] == (0, 0) and put_off["two_pass"][1] == 0 and put_off["lds"][1] <= put_off["lds"][0]


@pytest.mark.parametrize("scheme", list(ss.SCHEMES))
def test_long_read_pipeline_equals_the_oracle_under_every_scheme(tmp_path_factory, monkeypatch, scheme):
    """reads of 1 200 ... 2 500 bases that carry the links and shifts every 150 bases: stages 2 and 3a, then the long-read traceback with
    its lane-per-problem classes (whose size limit the device derives from the scheme) and without them (KMAHIP_LT_LANE=0)"""
    inp = inputs(tmp_path_factory)
    res = oracle_run(inp, scheme, "long")
    b = res["batch"]
    assert b.n == 24 and int(b.length.min()) >= 1200
    gaps = sum(1 for tr in res["trace"].values() if tr is not None and ss.cigar_has_gap(tr["cigar"]))
    assert len(res["filed"]) == b.n and gaps >= 12, (scheme, len(res["filed"]), gaps)
    db = _open(inp, scheme)
    try:
        _env(monkeypatch, {})
        _same_3a(res, db.map_se(b), (scheme, "long"))
        h, cc, ok = _front(db, res, scheme)
        for env in ({}, {"KMAHIP_LT_LANE": "0"}):
            _env(monkeypatch, env)
            assert _same_traces(res, db.align_trace(b, h["rc"], cc["tmpl"], ok), (scheme, env)) == b.n
    finally:
        db.close()


# ---- couples ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ss.PE_SCHEMES)
def test_couples_equal_the_oracle_under_the_pairing_schemes(tmp_path_factory, monkeypatch, scheme):
    """the paired entry point (stage 2's pairing, alnFragsPenaltyPE on the device, which adds rw.PE to a proper pair) on 300 couples whose
    mates in part prefer different templates: the records in stream order and the two ConClave vectors"""
    import pe_util
    inp = inputs(tmp_path_factory)
    want = couple_records(inp, scheme)
    _env(monkeypatch, {})
    db = _open(inp, scheme)
    try:
        got = pe_util.hip_pe_conclave(db, couples_input(inp), records_only=True)
    finally:
        db.close()
    assert record_rows(got) == record_rows(want) and len(want["n_hits"]) >= 300
    assert np.array_equal(got["alignment_scores"], want["alignment_scores"]) and np.array_equal(got["uniq_alignment_scores"], want["uniq_alignment_scores"])


# ---- the -cge preset of the host program -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ss.MODES)
def test_cge_preset_of_the_host_program_writes_the_recorded_rows(tmp_path_factory, tmp_path, monkeypatch, mode):
    """examples/kmahip_map -cge derives its parameter block itself (M 1, W1 -5, U -1, PE 17; the preset's MM of -3 does not survive the
    table's construction in the reference, and must not here): run on the whole short set, its fragment rows are the ones the reference
    wrote under -cge, which differ from the default scheme's."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    inp = inputs(tmp_path_factory)
    _env(monkeypatch, {})
    out = str(tmp_path / "out")
    r = subprocess.run([os.path.join(ROOT, "examples", "kmahip_map"), "-i", inp["fq"], "-t_db", inp["prefix"], "-o", out, "-cge"] +
                       (["-1t1"] if mode == "1t1" else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    with gzip.open(out + ".frag.gz", "rt") as f:
        rows = [line.rstrip("\n").split("\t") for line in f]
    rows = sorted(((c[6].split()[0], c[1], c[2], c[3], c[4], c[5]) for c in rows), key=lambda x: int(x[0][1:]))
    assert rows == ss.load_rows("cge", mode) and rows != ss.load_rows("default", mode)
