"""The device's threshold gates OFF the reference's defaults, one kernel family per test, through library calls, exact against the oracle
(which tests/test_oracle_thresholds.py pins to the reference at the same settings): the mapQ function itself over every small triple,
the mq / scoreT / mrc / minlen lines of stage 3a on its three routes, of the paired records and of both traceback pipelines, the chain
finder's coverT / mrs / minlen tests on its three routes, and the `.res` statistics. Each test asserts on the oracle's output that its
settings decide something on its input."""
import itertools

import numpy as np
import pytest

import golden_util
import oracle
import threshold_sets as ts
from kma_amd import binding, formats, synth

pytestmark = pytest.mark.gpu


# ---- 1. the mapQ function: device log against the host libm ----------------------------------------------------------------------------
def _mapq_triples():
    W = np.arange(1, 13, dtype=np.int32)
    best = np.repeat(np.arange(1, 2049, dtype=np.int32), np.arange(2, 2050))
    start = np.cumsum(np.arange(2, 2050)) - np.arange(2, 2050)
    second = (np.arange(len(best), dtype=np.int64) - np.repeat(start, np.arange(2, 2050))).astype(np.int32)
    assert second.min() == 0 and np.all(second <= best) and len(best) == 2048 * 2049 // 2 + 2048
    pow2 = [1 << k for k in range(11, 22)]
    big = np.unique(np.concatenate([np.geomspace(2049, 1 << 21, 4000).astype(np.int64), pow2, [p - 1 for p in pow2], [p + 1 for p in pow2]]))
    big = big[(big > 2048) & (big <= 1 << 21)]
    rng = np.random.default_rng(2048)
    fixed = np.stack([np.zeros_like(big), np.ones_like(big), big // 3, big // 2, big - 2, big - 1, big], 1)
    sec_big = np.concatenate([fixed, (rng.random((len(big), 32)) * (big[:, None] + 1)).astype(np.int64)], 1)
    b2 = np.repeat(big, sec_big.shape[1]).astype(np.int32)
    s2 = sec_big.reshape(-1).astype(np.int32)
    b, s = np.concatenate([best, b2]), np.concatenate([second, s2])
    return np.tile(b, len(W)), np.tile(s, len(W)), np.repeat(W, len(b))


def test_device_mapq_equals_host_libm_on_every_small_triple():
    """kma_mapq -- the one function behind every `mapQ < mq` gate of align.hip and longtrace.hip -- evaluated on the device against
    orc_mapq, the expression of oracle/align.c compiled against the host libm as the reference's is: all (best, second, w) with best
    1 ... 2048, second 0 ... best, w 1 ... 12, and some 4 000 larger best values up to 2^21 (log-spaced, every 2^k and 2^k +- 1) with second
    at 0, 1, best/3, best/2, best-2, best-1, best and 32 random values. 27 million evaluations in one launch; not one may differ."""
    b, s, w = _mapq_triples()
    assert 2.6e7 < len(b) < 3e7
    want = oracle.mapq(b, s, w)
    got = binding.test_mapq(b, s, w)
    bad = np.nonzero(want != got)[0]
    print("mapQ: %d triples, %d distinct values up to %d, %d differ" % (len(b), len(np.unique(want)), int(want.max()), len(bad)))
    assert len(bad) == 0, [(int(b[i]), int(s[i]), int(w[i]), int(got[i]), int(want[i])) for i in bad[:20]]
    assert want.max() > 550 and want[(s == b)].max() == 0


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------
_cache = {}


def _synth_input(tmp_path_factory, name):
    """dict(prefix, batch, odb, scan = oracle.scan_se(batch), o = {setting: oracle.align_se}) of a synthetic stage-3a input"""
    if name not in _cache:
        names, seqs, reads = ts.repeat_rich_set()
        if name == "repeat320":        # reads the long-read pipeline takes at KMAHIP_ALIGN_LONG=300 (it leaves reads with N's to the lane kernel)
            reads, *_ = synth.make_reads(seqs, 600, read_len=320, sub_rate=0.01, random_frac=0.02, n_rate=0.0, seed=4)
        prefix = str(tmp_path_factory.mktemp("thr_" + name) / "db")
        formats.write_index(prefix, names, seqs)
        batch = formats.pack_fixed(reads)
        odb = oracle.OracleDB(prefix)
        _cache[name] = dict(prefix=prefix, batch=batch, odb=odb, scan=odb.scan_se(batch), o={})
    return _cache[name]


def _golden_input(g, name):
    if name not in _cache:
        odb = oracle.OracleDB(g["prefix"])
        _cache[name] = dict(prefix=g["prefix"], batch=g["batch"], odb=odb, scan=odb.scan_se(g["batch"]), o={})
    return _cache[name]


def _oracle_3a(inp, setting):
    if setting not in inp["o"]:
        mq, scoreT, mrc, minlen = setting
        inp["o"][setting] = inp["odb"].align_se(inp["batch"], *inp["scan"], minlen=minlen, mq=mq, scoreT=scoreT, mrc=mrc)
    return inp["o"][setting]


def _set_params(db, setting):
    db.params.mq, db.params.scoreT, db.params.mrc, db.params.minlen = setting[0], float(setting[1]), float(setting[2]), setting[3]


def _changed(inp, setting):
    """(reads mapped at the defaults, those of them that lose or change hits at `setting`, reads mapped at `setting`), by the oracle"""
    o0, o = _oracle_3a(inp, (0, .5, 0, 16)), _oracle_3a(inp, setting)
    T_off = inp["scan"][2]
    mapped = np.nonzero(o0["n_hits"] > 0)[0]
    ch = 0
    for i in mapped:
        s, c = int(T_off[i]), int(o0["n_hits"][i])
        ch += int(o["n_hits"][i]) != c or any(not np.array_equal(o[k][s:s + c], o0[k][s:s + c]) for k in ("tmpl", "start", "end", "score"))
    return len(mapped), ch, int((o["n_hits"] > 0).sum())


# ---- 2. stage 3a -------------------------------------------------------------------------------------------------------------------------
ROUTES = {"general": {"KMAHIP_ALIGN_FAST": "0"}, "default": {}, "long": {"KMAHIP_ALIGN_LONG": "300"}}


@pytest.mark.parametrize("route,name", list(itertools.product(ROUTES, ["repeat", "se"])) + [("long", "repeat320"), ("long", "long")])
def test_stage3a_gates_equal_the_oracle_off_the_defaults(tmp_path_factory, monkeypatch, golden_se, golden_long, route, name):
    """mapQ < mq and the scoreT / mrc / minlen acceptance lines of align_tasks_kernel (KMAHIP_ALIGN_FAST=0), of align_fast_kernel + what
    it hands on (the default) and of the long-read pipeline in score mode (lt_seed_kernel's gate and long_result_kernel; the pipeline
    takes reads of 300 bases on here, which the 120-base reads and the `se` fixture never reach: the repeat-rich database with 320-base
    reads and the `long` fixture are its inputs). Everything tests/test_align_gpu.py compares at the defaults, at ten settings."""
    for k in ("KMAHIP_ALIGN_FAST", "KMAHIP_ALIGN_LONG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    inp = _golden_input({"se": golden_se, "long": golden_long}[name], name) if name in ("se", "long") else _synth_input(tmp_path_factory, name)
    if name == "repeat":
        # the conditions that keep the mq settings from passing vacuously (on the oracle's output)
        for mq in (1, 60, 120):
            mapped, ch, _ = _changed(inp, (mq, .5, 0, 16))
            assert 0.1 * mapped <= ch <= 0.9 * mapped, (mq, mapped, ch)
        assert _changed(inp, (200, .5, 0, 16))[2] == 0
    if name == "repeat320":
        # 40 ln(320) = 231 bounds these reads' mapQ, a copy 0 ... 8 % away pulls it down: 60 and 120 lie inside the spread
        for mq in (60, 120):
            mapped, ch, _ = _changed(inp, (mq, .5, 0, 16))
            assert 0.1 * mapped <= ch <= 0.9 * mapped, (mq, mapped, ch)
    batch = inp["batch"]
    if route == "long":
        # what the long-read pipeline takes at KMAHIP_ALIGN_LONG=300: reads of 300 bases on without an N whose strands did not tie
        takes = (batch.length >= 300) & (np.diff(batch.N_off) == 0) & (inp["scan"][0] > 0)
        if name in ("repeat320", "long"):
            assert takes.mean() > 0.8, (name, float(takes.mean()))
        else:      # listed with this route all the same: here it is the default route once more
            assert not takes.any()
    db = binding.KmaHipDB(inp["prefix"])
    try:
        for setting in ts.ALIGN_SETTINGS:
            _set_params(db, setting)
            (rc_flag, flag, T_off, T), h = db.map_se(batch)
            for a, b in zip(inp["scan"], (rc_flag, flag, T_off, T)):
                assert np.array_equal(a, b), setting
            o = _oracle_3a(inp, setting)
            assert np.array_equal(o["n_hits"], h["n_hits"]), setting
            assert np.array_equal(o["best_score"], h["best_score"]), setting
            assert np.array_equal(o["out_flag"], h["flag"]), setting
            for i in np.nonzero(o["n_hits"] > 0)[0]:
                s, c = int(T_off[i]), int(o["n_hits"][i])
                for key in ("tmpl", "start", "end", "score"):
                    assert np.array_equal(o[key][s:s + c], h[key][s:s + c]), (setting, i, key)
            assert np.array_equal(o["alignment_scores"], h["alignment_scores"]), setting
            assert np.array_equal(o["uniq_alignment_scores"], h["uniq_alignment_scores"]), setting
    finally:
        db.close()


# ---- 3. traceback --------------------------------------------------------------------------------------------------------------------------
_KEYS = ("score", "start", "end", "aln_len", "clip_start", "clip_end", "match", "tGaps", "qGaps", "mapQ")


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


@pytest.mark.parametrize("name", ["se", "long"])
def test_traceback_gates_equal_the_oracle_and_the_fixture_mapq(golden_se, golden_long, name):
    """trace_kernel (and, for the reads of `long` over 1 kb, the long-read pipeline behind kmahip_align_trace): its mapQ gate and the read
    filter's minlen / mrc / scoreT lines. Stages 2 - 3b run at the defaults (they choose each read's template), the traceback at ten
    settings: every figure and the CIGAR against OracleAligner at the same setting, and for the settings that move mq alone against the
    reference's own SAM record -- a read is dropped exactly when its MAPQ there is below mq."""
    g = {"se": golden_se, "long": golden_long}[name]
    sam = golden_util.load_sam(name)
    b = g["batch"]
    odb = oracle.OracleDB(g["prefix"])
    db = binding.KmaHipDB(g["prefix"])
    try:
        (rc_flag, flag, T_off, T), h = db.map_se(b)
        cc = db.conclave_se(b.length, T_off, h)
        ok = np.zeros(int(db.info.DB_size), np.uint8)
        for r in db.res_rows(cc["w_scores"]):
            ok[r.template_id] = r.significant
        filed = []
        for i, r in enumerate(g["s1"]):
            tt = int(cc["tmpl"][i])
            if tt == 0 or not ok[abs(tt)]:
                continue
            read = g["reads"][i]
            if (int(h["flag"][i]) & 16 != 0) != (tt < 0):
                read = synth.revcomp_codes(read)
            filed.append((i, r["hdr"].rstrip(b"\0").decode(), read, abs(tt)))
        n_dropped = {}
        for setting in [(0, .5, 0, 16)] + ts.ALIGN_SETTINGS:
            _set_params(db, setting)
            stats, off, nops, ops = db.align_trace(b, h["rc"], cc["tmpl"], ok)
            al = oracle.OracleAligner(odb, mq=setting[0], scoreT=setting[1], mrc=setting[2], minlen=setting[3])
            kept = np.zeros(b.n, bool)
            for i, hd, read, t in filed:
                got = _got(stats, off, nops, ops, i)
                assert got == _want(al.align_trace(read, t)), (setting, hd)
                kept[i] = got is not None
                if setting[1:] == (.5, 0, 16):
                    assert (got is not None) == (hd in sam and sam[hd][0][3] >= setting[0]), (setting, hd)
            assert not stats[~kept].any(), setting
            n_dropped[setting] = len(sam) - int(kept.sum())
    finally:
        db.close()
    print(name, n_dropped)
    if name == "se":      # the other gates decide something on this fixture (mq: tests/test_oracle_thresholds.py)
        for setting in ((0, .8, 0, 16), (0, .95, 0, 16), (0, .5, .9, 16), (0, .5, 0, 120)):
            assert n_dropped[setting] >= 60, (setting, n_dropped)


def test_mt1_traceback_gates_equal_the_oracle_and_the_fixture_mapq(tmp_path):
    """the long-read trace pipeline of `-Mt1` (longtrace.hip: lt_seed_kernel's mapQ gate, the finish kernel's minlen / mrc / scoreT lines)
    on the raw reads of the mt1 fixture, as above"""
    g = golden_util.load_mt1(tmp_path / "mt1")
    sam = golden_util.load_sam("mt1")
    batch = formats.pack_ragged(g["reads"])
    odb = oracle.OracleDB(g["prefix"])
    db = binding.KmaHipDB(g["prefix"])
    try:
        for setting in [(0, .5, 0, 16)] + ts.ALIGN_SETTINGS:
            _set_params(db, setting)
            (stats, off, nops, ops), rc = db.align_trace_mt1(batch, 1)
            al = oracle.OracleAligner(odb, mq=setting[0], scoreT=setting[1], mrc=setting[2], minlen=setting[3])
            for i, (nm, rd) in enumerate(zip(g["names"], g["reads"])):
                o, is_rc, _ = al.align_trace_mt1(rd, 1)
                got = _got(stats, off, nops, ops, i)
                assert got == _want(o), (setting, nm)
                if got is not None:
                    assert int(rc[i]) == is_rc, (setting, nm)
                if setting[1:] == (.5, 0, 16):
                    flag_, rname, pos, mapq, cigar, AS = sam[nm][0]
                    assert (got is not None) == (cigar != "*" and mapq >= setting[0]), (setting, nm)
    finally:
        db.close()


# ---- 4. paired stage 3a ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mq,scoreT", [(60, .5), (0, .8)])
def test_paired_stage3a_gates_equal_the_oracle(golden_pe, mq, scoreT):
    """the acceptance lines of the paired records (alnFragsPenaltyPE on the device) and of the singly filed ones: the frag_raw records of
    the `pe` fixture in stream order -- hits, scores, lengths, templates, bounds -- and the two ConClave vectors against the oracle's at the
    same setting, record for record (a proper pair without a hit is a record too, and stands where it stood in the stream)."""
    import pe_util
    g = golden_pe
    base = pe_util.oracle_pe_conclave_records(g)
    want = pe_util.oracle_pe_conclave_records(g, mq=mq, scoreT=scoreT)
    db = binding.KmaHipDB(g["prefix"])
    try:
        db.params.mq, db.params.scoreT = mq, scoreT
        got = pe_util.hip_pe_conclave(db, g, records_only=True)
    finally:
        db.close()

    def rows(r):
        off = np.concatenate([r["off"], [len(r["tmpl"])]])
        return [(int(r["n_hits"][x]), int(r["score"][x]), int(r["q_len"][x]), int(r["q_len2"][x])) +
                tuple(tuple(int(v) for v in r[k][off[x]:off[x + 1]]) for k in ("tmpl", "start", "end")) for x in range(len(r["n_hits"]))]

    assert rows(got) == rows(want)
    assert np.array_equal(got["alignment_scores"], want["alignment_scores"]) and np.array_equal(got["uniq_alignment_scores"], want["uniq_alignment_scores"])
    # the setting decides something on this fixture (of the records with a hit at the defaults, 29 are gone or different at mq 60 and 66
    # at scoreT 0.8)
    moved = len(set(r for r in rows(base) if r[0]) - set(rows(want)))
    print("pe", mq, scoreT, moved)
    assert moved > 0


# ---- 5. the chain finder -----------------------------------------------------------------------------------------------------------------------
CHAIN_ROUTES = ({"KMAHIP_CHAIN": "slow"}, {"KMAHIP_CHAIN_LONG": "0"}, {})


def _chain_case(monkeypatch, prefix, reads, settings, min_differing, first=0):
    def dev(db, b, env, **kw):
        for k in ("KMAHIP_CHAIN", "KMAHIP_CHAIN_LONG"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        o = db.scan_chain(b, **kw)
        return [(int(o["read"][x]), int(o["rc_flag"][x]), int(o["emit_rc"][x]), int(o["q_start"][x]), int(o["q_end"][x]),
                 tuple(int(t) for t in o["T"][o["T_off"][x]:o["T_off"][x + 1]])) for x in range(len(o["read"]))]

    b = formats.pack_ragged(reads)
    odb = oracle.OracleDB(prefix)
    base = [r for r in ts.flat_chain_records(odb.scan_chain(b)) if r[0] >= first]
    db = binding.KmaHipDB(prefix)
    differing = {}
    try:
        for coverT, mrs, minlen in settings:
            for exhaustive in (0, 1):
                want = ts.flat_chain_records(odb.scan_chain(b, minlen=minlen, coverT=coverT, mrs=mrs, exhaustive=exhaustive))
                if not exhaustive:
                    differing[(coverT, mrs, minlen)] = ts.reads_differing([r for r in want if r[0] >= first], base, len(reads))
                    assert differing[(coverT, mrs, minlen)] >= min_differing, differing
                for env in CHAIN_ROUTES:
                    got = dev(db, b, env, minlen=minlen, coverT=coverT, mrs=mrs, exhaustive=exhaustive)
                    assert got == want, (coverT, mrs, minlen, exhaustive, env)
    finally:
        db.close()
    return differing


@pytest.mark.parametrize("name", ["noisy", "module"])
def test_chain_finder_gates_equal_the_oracle_off_the_defaults(tmp_path, monkeypatch, name):
    """chain_kernel (KMAHIP_CHAIN=slow), the fast route without and with the long-read kernels: the coverT / mrs / minlen tests and the
    early exit whose proof leans on coverT and minlen, on reads whose chains score around mrs x length (noisy) and whose chains overlap
    by a shared module of 30 ... 110 bases (module). Every setting changes the records of at least 60 reads of its set."""
    names, seqs, reads = (ts.noisy_set if name == "noisy" else ts.shared_module_set)()
    prefix = str(tmp_path / "db")
    formats.write_index(prefix, names, seqs)
    _chain_case(monkeypatch, prefix, reads, ts.NOISY_GPU_SETTINGS if name == "noisy" else ts.MODULE_GPU_SETTINGS, 60)


@pytest.mark.parametrize("kind", ["genome", "genes"])
def test_chain_finder_long_read_route_equals_the_oracle_off_the_defaults(tmp_path, monkeypatch, kind):
    """chain_long_anchor_kernel + chain_long_tail_kernel carry their own copies of the gates: the reads of
    test_long_read_route_equals_lane_kernel_and_oracle (232 of them, 15 ... 20 000 bases; a setting moves 1 ... 129 of those) and behind
    them 260 reads of 922 bases and more whose chains overlap by a shared module or score around mrs x length (ts.long_threshold_set).
    The added reads are N-free and longer than the fast route takes, so the long-read kernels chain them; every setting changes the
    records of at least 60 OF THEM."""
    names, seqs, reads, first = ts.long_threshold_set(kind)
    assert len(reads) - first == ts.N_LONG_ADDED and all(len(r) >= ts.LONG_ROUTE_MIN and int(r.max()) < 4 for r in reads[first:])
    prefix = str(tmp_path / "db")
    formats.write_index(prefix, names, seqs)
    print(kind, _chain_case(monkeypatch, prefix, reads, ts.LONG_SETTINGS, 60, first))


# ---- 6. `.res` statistics ----------------------------------------------------------------------------------------------------------------------
def test_res_statistics_equal_the_oracle_off_the_defaults(golden_se):
    """kmahip_res_rows (host arithmetic) at other -e and scoreT values than 0.05 and 0.5, on the `se` fixture's ConClave scores"""
    g = golden_se
    b = g["batch"]
    tlen = formats.read_lengths(g["prefix"])
    db = binding.KmaHipDB(g["prefix"])
    try:
        (rc_flag, flag, T_off, T), h = db.map_se(b)
        w = db.conclave_se(b.length, T_off, h)["w_scores"]
        sig = {}
        for evalue, scoreT in ((0.05, .5), (1e-6, .5), (.5, .5), (.05, .1), (.05, .9)):
            rows = db.res_rows(w, evalue, scoreT)
            want = oracle.res_stats(w, tlen, evalue, scoreT)
            assert [r.template_id for r in rows] == [t for t in range(1, len(tlen)) if w[t] > 0]
            for r in rows:
                t = r.template_id
                assert (r.score, r.template_length, float(r.expected), r.q_value, r.p_value, r.significant) == \
                       (int(w[t]), int(tlen[t]), want["expected"][t], want["q_value"][t], want["p_value"][t], want["significant"][t]), (evalue, scoreT, t)
            sig[(evalue, scoreT)] = int(want["significant"][w > 0].sum())
    finally:
        db.close()
    print(sig)
    assert len(set(sig.values())) >= 2      # (63 or 64 of the fixture's 65 templates pass: the settings hardly differ on it)
