"""Every DP size class of the long-read traceback (longtrace.hip) against the plain-C oracle and the reference's own SAM records, on
the directed fixture tests/golden/ltclass (make_golden_ltclass.py): each read yields ONE DP problem of a chosen mode, size and band -- or
none -- so that after a call kmahip_trace_get_class_counts must show exactly the group's reads in the classes cases.tsv names, and
nothing anywhere else. The groups walk the edges of lt_class / lt_lane_class (row widths, cell caps, template rows, full matrix against
band, band widths, LDS against HBM, the turn cap, the 16-bit gate; the generator's docstring names the few no input reaches), the modes of the three windows, degenerate joins, ties, N's and the
reject of a link; the arrangements move the same problems between the kernel families."""
import os

import pytest

import golden_util
import oracle
from kma_amd import binding, formats

pytestmark = pytest.mark.gpu

_KEYS = ("score", "start", "end", "aln_len", "clip_start", "clip_end", "match", "tGaps", "qGaps", "mapQ")
# the environment of an arrangement and where a problem with lane class j (every lane class on; -1: none) is counted under it:
# "lane" = in its lane class unless that is class 8, which is off by default; "all" = class 8 too; "free" = class 8 too and no cap on
# the turns of a lane's sweep (cases.tsv's lanefree columns); "wave" = in its wavefront class
ARRANGEMENTS = {
    "default": ({}, "lane"),
    "reg_off": ({"KMAHIP_LT_REG": "0"}, "lane"),
    "lane_off": ({"KMAHIP_LT_LANE": "0"}, "wave"),
    "score_table": ({"KMAHIP_LT_SCORE_TABLE": "1"}, "lane"),
    "passes_of_7": ({"KMAHIP_LT_PASS_READS": "7"}, "lane"),
    "lane_class_8_on": ({"KMAHIP_LT_LCLS": "0x1ff"}, "all"),
    "turn_cap_lifted": ({"KMAHIP_LT_LCLS": "0x1ff", "KMAHIP_LT_LANE_TURNS": "1000000"}, "free"),
}
# wavefront classes without a kernel (lt_class never returns them), and the one no input reaches
NOT_INSTANTIATED = {13: "no kernel: the full-matrix forms of 8 columns a lane were never built", 14: "no kernel: likewise, 16 columns a lane"}
UNREACHABLE = {11: "banded, q_l <= 128, move matrix over 32768 bytes: a band needs q_l > |t_l - q_l| + 64, so |t_l - q_l| < 64, t_l < 192 and "
                   "the matrix is at most (127 + 1 + 2) x 192 = 24960 bytes"}


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    g = golden_util.load_ltclass(tmp_path_factory.mktemp("ltclass"))
    odb = oracle.OracleDB(g["prefix"])
    g["oracle"] = {}
    for s, scheme in g["schemes"].items():
        golden_util.set_scheme(odb.rw, scheme)
        al = oracle.OracleAligner(odb)
        g["oracle"][s] = [al.align_trace_mt1(rd, 1)[:2] for rd in g["reads"]]
    g["groups"] = {}
    for i, c in enumerate(g["cases"]):
        g["groups"].setdefault(c["group"], []).append(i)
    g["db"] = binding.KmaHipDB(g["prefix"])
    yield g
    g["db"].close()


def _call(g, idx, scheme, env):
    """one align_trace_mt1 call on the reads idx under the scheme and the environment -> results, class counts"""
    db = g["db"]
    golden_util.set_scheme(db.params.rw, g["schemes"][scheme])
    batch = formats.pack_ragged([g["reads"][i] for i in idx])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        (stats, off, nops, ops), rc = db.align_trace_mt1(batch, 1)
        counts = db.get_trace_class_counts()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return (stats, off, nops, ops, rc), counts


def _expected_counts(g, idx, scheme, where):
    wave, lane = [0] * 17, [0] * 9
    for i in idx:
        c = g["cases"][i]
        if not c["n_dp"]:
            continue
        j = c[("lanefree_" if where == "free" else "lane_") + scheme]
        if where != "wave" and j >= 0 and (j != 8 or where in ("all", "free")):
            lane[j] += 1
        else:
            wave[c["wave_" + scheme]] += 1
    return dict(wave=wave, lane=lane)


def _check_reads(g, idx, scheme, res, what):
    stats, off, nops, ops, rc = res
    for x, i in enumerate(idx):
        nm, case = g["names"][i], g["cases"][i]
        o, is_rc = g["oracle"][scheme][i]
        flag, rname, pos, mapq, cigar, AS = g["sam"][scheme][nm]
        tag = (what, nm, case["case"])
        if not stats[x].any():
            assert o is None and cigar == "*", tag
            continue
        assert o is not None and cigar != "*", tag
        assert int(rc[x]) == is_rc == (case["strand"] == "-"), tag
        got = dict(zip(_KEYS, (int(v) for v in stats[x])))
        got["cigar"] = binding.cigar_from_runs(ops[off[x]:off[x] + nops[x]], int(stats[x, 4]), int(stats[x, 5]))
        want = {k: o[k] for k in _KEYS + ("cigar",)}
        assert got == want, tag + (got, want)
        assert (got["start"] + 1, min(254, got["mapQ"]), got["cigar"], got["score"]) == (pos, mapq, cigar, AS), tag


@pytest.mark.parametrize("scheme", ["s1", "s2"])
@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
def test_every_group_matches_oracle_and_reference_in_its_classes(fx, arrangement, scheme):
    env, where = ARRANGEMENTS[arrangement]
    for group, idx in fx["groups"].items():
        res, counts = _call(fx, idx, scheme, env)
        want = _expected_counts(fx, idx, scheme, where)
        print(arrangement, scheme, group, len(idx), "reads; wave", counts["wave"], "lane", counts["lane"])
        assert counts == want, (arrangement, scheme, group, counts, want)
        _check_reads(fx, idx, scheme, res, (arrangement, scheme, group))
        assert fx["db"].get_trace_stats().reads == len(idx)


def test_every_instantiated_class_is_reached(fx):
    """the whole fixture in one call each with the lane classes on, all nine on, all nine on without the turn cap, and off: every class
    with a kernel is counted at least once, the counts add up to the fixture's DP problems, and whatever stays empty has its reason here"""
    every = list(range(len(fx["reads"])))
    n_dp = sum(c["n_dp"] for c in fx["cases"])
    wave, lane = [0] * 17, [0] * 9
    for arrangement in ("default", "lane_class_8_on", "turn_cap_lifted", "lane_off"):
        env, where = ARRANGEMENTS[arrangement]
        res, counts = _call(fx, every, "s1", env)
        assert counts == _expected_counts(fx, every, "s1", where), arrangement
        assert sum(counts["wave"]) + sum(counts["lane"]) == n_dp == 244, (arrangement, counts)
        _check_reads(fx, every, "s1", res, (arrangement, "all"))
        wave = [a + b for a, b in zip(wave, counts["wave"])]
        lane = [a + b for a, b in zip(lane, counts["lane"])]
    print("wave", wave, "lane", lane)
    exempt = {**NOT_INSTANTIATED, **UNREACHABLE}
    assert set(exempt) == {11, 13, 14}
    for c in range(17):
        assert (wave[c] > 0) != (c in exempt), (c, wave[c], exempt.get(c))
    assert all(n > 0 for n in lane), lane
