"""Proximity matching (`-proxi f`) and the `-ill` preset on the single-end `-1t1` run.

Stage 2 (getProxiMatch, savekmers.c:296-340) against the reference's `-s2` taps recorded at `-proxi 0.9` and `-proxi 0.7`
(tests/golden/proxi, make_golden_proxi.py); whole runs of examples/kmahip_map against the compiled reference (oracle/_ref/kma -t 1)
run live on the same seeded input, `.res`, `.fsa`, `.aln` and the inflated `.frag.gz` byte for byte; the combinations that stay
refused, by name. The inputs (proxi_util.INPUTS) put most reads' candidate lists beyond the scan's first-tier table (16 slots), its
second tier (64) and the two inline result slots, so the overflow routes, the pool and the retry with a larger one carry the run."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_util
import proxi_util
from kma_amd import binding, formats, synth
from proxi_util import KMA, MAP

pytestmark = pytest.mark.gpu
GOLD = os.path.join(golden_util.GOLD, "proxi")
TIMEOUT = 120


# ---- stage 2 against the taps ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hipdb(golden_se):
    db = binding.KmaHipDB(golden_se["prefix"])
    yield db
    db.close()


@pytest.fixture(scope="module")
def taps():
    out = {}
    for f, name in ((0.9, "s2_p09.bin.gz"), (0.7, "s2_p07.bin.gz")):
        with gzip.open(os.path.join(GOLD, name), "rb") as g:
            out[f], _ = formats.parse_s2(g.read())
    return out


@pytest.fixture(scope="module")
def scan07(golden_se, hipdb):
    """the arrays at min_frac = 0.7 with every stage-2 switch at its default, computed once"""
    return hipdb.scan_se(golden_se["batch"], min_frac=0.7)


def _same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("f", [0.9, 0.7])
def test_scan_proxi_matches_reference_s2_tap(golden_se, hipdb, taps, f):
    rc_flag, flag, T_off, T = hipdb.scan_se(golden_se["batch"], min_frac=f)
    n = golden_util.check_scan_against_s2(golden_se["s1"], taps[f], rc_flag, flag, T_off, T)
    assert n > 800
    # the tap really differs from the plain one: longer lists, the same best scores
    plain = {r["hdr"]: r for r in golden_se["s2"]}
    longer = sum(len(r["T"]) > len(plain[r["hdr"]]["T"]) for r in taps[f])
    assert longer > 100, longer
    assert len(taps[f]) == len(plain) and all(r["rc_flag"] == plain[r["hdr"]]["rc_flag"] for r in taps[f])


def test_scan_proxi_takes_the_absolute_value(golden_se, hipdb):
    """the sign of -proxi is stage 3a's (kma.c:1605 hands stage 2 |minFrac|)"""
    assert _same_arrays(hipdb.scan_se(golden_se["batch"], min_frac=-0.9), hipdb.scan_se(golden_se["batch"], min_frac=0.9))


@pytest.mark.parametrize("switch", ["KMAHIP_SCAN_DIAG", "KMAHIP_SCAN_REC", "KMAHIP_SCAN_REFINE"])
def test_scan_proxi_same_with_every_stage2_switch_off(golden_se, hipdb, scan07, monkeypatch, switch):
    """a non-best template's exact score decides whether it is kept: the diagonal, record and refine routes must not change one"""
    monkeypatch.setenv(switch, "0")
    assert _same_arrays(hipdb.scan_se(golden_se["batch"], min_frac=0.7), scan07)


def test_scan_proxi_one_is_the_plain_scan(golden_se, hipdb):
    plain = hipdb.scan_se(golden_se["batch"])
    assert _same_arrays(hipdb.scan_se(golden_se["batch"], min_frac=-1.0), plain)
    golden_util.check_scan_against_s2(golden_se["s1"], golden_se["s2"], *plain)


# ---- whole runs against the binary -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    proxi_util.build_map()
    made = {}

    def get(key):
        if key not in made:
            made[key] = proxi_util.make_input(tmp_path_factory.mktemp("proxi_" + key), key)
        return made[key]
    return get


def _ref(s, extra):
    """the reference on input s with `extra`, once per option set -> stem of its files"""
    key = " ".join(extra)
    if key not in s["runs"]:
        stem = str(s["tmp"] / ("ref%d" % len(s["runs"])))
        # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
        p = subprocess.run([KMA, "-i", s["fq"], "-o", stem, "-t_db", s["prefix"], "-t", "1"] + extra, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL, timeout=TIMEOUT)
        assert p.returncode in (0, 2), p.returncode
        s["runs"][key] = stem
    return s["runs"][key]


def _map(s, tag, extra, env=None):
    stem = str(s["tmp"] / ("got_" + tag))
    e = dict(os.environ)
    e.update(env or {})
    subprocess.run([MAP, "-i", s["fq"], "-t_db", s["prefix"], "-o", stem] + extra, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                   env=e, timeout=TIMEOUT)
    return stem


def _files(stem):
    return tuple(open(stem + ext, "rb").read() for ext in (".res", ".fsa", ".aln")) + (gzip.open(stem + ".frag.gz", "rb").read(),)


def _assert_same_files(got, ref):
    g, r = _files(got), _files(ref)
    for name, a, b in zip((".res", ".fsa", ".aln", ".frag.gz"), g, r):
        assert a == b, name
    assert g[3].count(b"\n") > 1000
    return r


def _list_lengths(frag):
    """templates listed per row of an inflated .frag.gz (the second column)"""
    return np.array([int(x.split(b"\t")[1]) for x in frag.split(b"\n") if x])


@pytest.mark.parametrize("f", ["0.7", "-0.7"])
def test_whole_run_input_a(inputs, f):
    s = inputs("a")
    extra = ["-1t1", "-proxi", f]
    _assert_same_files(_map(s, "a" + f, extra), _ref(s, extra))
    # the sign is really exercised: what a kept hit adds to the ConClave scores moves the reference's own .res
    assert open(_ref(s, ["-1t1", "-proxi", "0.7"]) + ".res", "rb").read() != open(_ref(s, ["-1t1", "-proxi", "-0.7"]) + ".res", "rb").read()


@pytest.mark.parametrize("env", [{}, {"KMAHIP_MAP_BATCH": "1000"}, {"KMAHIP_ROW_GRAIN": "500"}], ids=["default", "batch1000", "grain500"])
def test_whole_run_input_b_long_lists(inputs, env):
    s = inputs("b")
    extra = ["-1t1", "-proxi", "0.7"]
    ref = _ref(s, extra)
    n = _list_lengths(gzip.open(ref + ".frag.gz", "rb").read())
    assert (n > 64).sum() >= 1000 and (n > 16).sum() >= 3000, ((n > 64).sum(), (n > 16).sum())
    _assert_same_files(_map(s, "b" + "".join(env), extra, env), ref)


def test_whole_run_input_c_second_tier(inputs):
    s = inputs("c")
    extra = ["-1t1", "-proxi", "0.9"]
    _assert_same_files(_map(s, "c", extra), _ref(s, extra))


@pytest.mark.parametrize("extra", [["-ill"], ["-ill", "-mrc", "0"], ["-ill", "-proxi", "0.7"], ["-proxi", "0.7", "-ill"]],
                         ids=["ill", "ill_mrc0", "ill_then_proxi", "proxi_then_ill"])
def test_whole_run_ill_preset(inputs, extra):
    """the preset; a later option that overrides one of its values; an earlier one that it overrides"""
    s = inputs("a")
    ref = _assert_same_files(_map(s, "".join(extra), extra), _ref(s, extra))
    if extra[-1] == "0.7":          # (-mrc 0 moves nothing on this input; the later -proxi does)
        assert ref != _files(_ref(s, ["-ill"]))
    if extra[0] == "-proxi":
        assert ref == _files(_ref(s, ["-ill"]))


def test_whole_run_ill_differs_from_its_parts_left_out(inputs):
    """(-ill is not the plain -1t1 run on this input: the preset's values reach the stages)"""
    s = inputs("a")
    assert _files(_ref(s, ["-ill"]))[0] != _files(_ref(s, ["-1t1"]))[0]


def test_whole_run_with_ef_matrix_vcf(inputs):
    s = inputs("c")
    extra = ["-1t1", "-proxi", "0.9", "-ef", "-matrix", "-vcf"]
    got, ref = _map(s, "emv", extra), _ref(s, extra)
    _assert_same_files(got, ref)
    keep = lambda raw: [x for x in raw.split(b"\n") if not x.startswith(b"## date\t") and not x.startswith(b"## command\t")]  # noqa: E731
    assert keep(open(got + ".mapstat", "rb").read()) == keep(open(ref + ".mapstat", "rb").read())
    for ext in (".mat.gz", ".vcf.gz"):
        assert gzip.open(got + ext, "rb").read() == gzip.open(ref + ext, "rb").read(), ext


@pytest.mark.parametrize("f", ["1", "-1"])
def test_proxi_one_leaves_the_run_as_it_is(inputs, f):
    s = inputs("c")
    if "plain" not in s:
        s["plain"] = _files(_map(s, "plain", ["-1t1"]))
    assert _files(_map(s, "one" + f, ["-1t1", "-proxi", f])) == s["plain"]
    assert s["plain"] == _files(_ref(s, ["-1t1"]))


@pytest.mark.parametrize("tail,msg", [(["-proxi", "1.5"], b"Invalid argument at \"-proxi\"."), (["-proxi", "x"], b"Invalid argument at \"-proxi\"."),
                                      (["-proxi"], b"Need argument at: \"-proxi\".")], ids=["above", "text", "bare"])
def test_proxi_bad_value_exits_1(inputs, tail, msg):
    s = inputs("c")
    p = subprocess.run([MAP, "-i", s["fq"], "-t_db", s["prefix"], "-o", str(s["tmp"] / "bad"), "-1t1"] + tail, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       timeout=TIMEOUT)
    assert p.returncode == 1 and msg in p.stderr, (p.returncode, p.stderr)
    assert not os.path.exists(str(s["tmp"] / "bad.res"))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_kmahip_map_refuses_by_name(tmp_path):
    proxi_util.build_map()
    cases = proxi_util.refused_commands(tmp_path)
    assert len(cases) >= 8
    for args, why in cases:
        p = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert p.returncode == 2, (args, p.returncode, p.stderr)
        assert why.encode() in p.stderr and b"proximity matching serves the single-end -1t1 run" in p.stderr, (args, p.stderr)
        assert not os.path.exists(str(tmp_path / "out.res"))


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("proxi_pe")
    names, seqs = synth.make_gene_db(n_families=4, variants=3, len_lo=500, len_hi=700, seed=11)
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    m1, m2, _ = synth.make_pairs(seqs, 64, read_len=100, seed=3)
    return prefix, formats.pack_ragged([x for ab in zip(m1, m2) for x in ab])


@pytest.mark.parametrize("call", ["scan_pe", "map_pe"])
def test_library_refuses_proximity_on_paired_entry_points(pairs, call):
    prefix, batch = pairs
    db = binding.KmaHipDB(prefix)
    try:
        db.params.minFrac = 0.9
        with pytest.raises(binding.KmaHipError, match=r"kmahip error -1: proximity matching .* serves the single-end -1t1 run, not paired reads"):
            getattr(db, call)(batch)
        db.params.minFrac = 1.0
        getattr(db, call)(batch)          # (and the same call is served without it)
    finally:
        db.close()


def test_library_refuses_forced_pairing_behind_stage_2(pairs):
    """kmahip_params.apm = 2: stage 2 (kmahip_scan_pe) is built; stage 3a would pair the couples by penalty, so kmahip_map_pe says no"""
    prefix, batch = pairs
    db = binding.KmaHipDB(prefix)
    try:
        db.params.apm = 2
        db.scan_pe(batch)
        with pytest.raises(binding.KmaHipError, match=r"kmahip error -1: forced pairing .* kmahip_scan_pe only"):
            db.map_pe(batch)
        db.params.apm = 0x30          # bits 4-5 = 3: forced pairing asked of stage 3a alone
        with pytest.raises(binding.KmaHipError, match=r"kmahip error -1: forced pairing"):
            db.map_pe(batch)
    finally:
        db.close()


def test_library_refuses_proximity_in_the_chain_finder_and_mem_mode(golden_se, hipdb):
    hipdb.params.minFrac = 0.9
    try:
        with pytest.raises(binding.KmaHipError, match=r"kmahip error -1: proximity matching .* chain finder"):
            hipdb.scan_chain(golden_se["batch"])
        binding.lib().kmahip_set_mem_mode(1)
        try:
            with pytest.raises(binding.KmaHipError, match=r"kmahip error -1: proximity matching .* -mem_mode"):
                hipdb.scan_se(golden_se["batch"])
        finally:
            binding.lib().kmahip_set_mem_mode(0)
    finally:
        hipdb.params.minFrac = 1.0
