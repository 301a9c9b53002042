"""Every route of the pile-up (pileup_device and its kernels, kma_amd/csrc/assemble.hip) against a plain walk over the ring of columns
(oracle/assembly.c), on hand-made traces (pile_util): the count matrix column by column, byte for byte, and the consensus figures.

Routes, each chosen by a switch the library reads and each shown taken by the line `pileup_device` prints per launch under
KMAHIP_DEBUG_TIMING: a template whole in half or in all of a CU's LDS, the same on HBM from the start or after an overflow, a template
longer than 5 741 columns cut into units of 64 .. 1 024 columns, with and without run checkpoints, units halved when one runs out of room
for insertion columns, both orders of max_frag. Cases (pile_util.case): reads that begin and end on the columns around a unit's bounds,
gaps and insertion runs on them, the origin of the ring, reads across it, reads that go round it more than once, reads of more runs than
a workgroup has threads, and a seeded mix of all of it on three templates at once. Nothing here needs the reference binary."""
import re

import numpy as np
import pytest

import oracle
import pile_util as pu
from kma_amd import binding, formats

pytestmark = pytest.mark.gpu

SWITCHES = ("KMAHIP_PILE_NO_LDS", "KMAHIP_PILE_LDS_NODES", "KMAHIP_PILE_FULL_LDS", "KMAHIP_PILE_SEG_COLS", "KMAHIP_PILE_NO_CKPT")
CASES = ("boundaries", "origin", "wrapped", "turns", "rounds", "mix1", "mix2")
# route: (switches, columns per unit, what the last launch's line must say). 6 000 columns make ceil(6 000 / S) units, the two short
# templates one each.
ROUTES = {
    "default": ({}, 1024, "8 units, 1024 columns per segment, half LDS, whole templates in LDS, run checkpoints"),
    "hbm": ({"KMAHIP_PILE_NO_LDS": "1"}, 1024, "8 units, 1024 columns per segment, full LDS, whole templates on HBM, run checkpoints"),
    "full_lds": ({"KMAHIP_PILE_FULL_LDS": "1"}, 1024, "8 units, 1024 columns per segment, full LDS, whole templates in LDS, run checkpoints"),
    "seg64": ({"KMAHIP_PILE_SEG_COLS": "64"}, 64, "96 units, 64 columns per segment, half LDS, whole templates in LDS, run checkpoints"),
    "seg256": ({"KMAHIP_PILE_SEG_COLS": "256"}, 256, "26 units, 256 columns per segment, half LDS, whole templates in LDS, run checkpoints"),
    "seg1024": ({"KMAHIP_PILE_SEG_COLS": "1024"}, 1024, "8 units, 1024 columns per segment, half LDS, whole templates in LDS, run checkpoints"),
    "no_ckpt": ({"KMAHIP_PILE_NO_CKPT": "1"}, 1024, "8 units, 1024 columns per segment, half LDS, whole templates in LDS, no run checkpoints"),
    "no_ckpt_seg256": ({"KMAHIP_PILE_NO_CKPT": "1", "KMAHIP_PILE_SEG_COLS": "256"}, 256,
                       "26 units, 256 columns per segment, half LDS, whole templates in LDS, no run checkpoints"),
}
LAUNCH = re.compile(r"\[kmahip\] pile-up: launch of (.*)")


@pytest.fixture(scope="module")
def ring(tmp_path_factory):
    names, seqs = pu.templates()
    prefix = str(tmp_path_factory.mktemp("pile_routes") / "db")
    formats.write_index(prefix, names, seqs)
    return dict(prefix=prefix, seqs=seqs, odb=oracle.OracleDB(prefix), want={})


def _want(ring, name, S, max_frag):
    """the case's batch and, per template with reads, the oracle's matrix text and call -- once per (case, unit length, max_frag)"""
    key = (name, S, max_frag)
    if key not in ring["want"]:
        b = pu.Batch(pu.case(name, ring["seqs"], S))
        per = {}
        for t, seq in enumerate(ring["seqs"], 1):
            if b.order(t, max_frag):
                oa = b.oracle(ring["odb"], t, len(seq), max_frag)
                per[t] = (oa.matrix_text(seq), oa.call())
        ring["want"][key] = (b, per)
    return ring["want"][key]


def _first_difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "column %d of %d / %d: device %r, ring walk %r" % (i, len(g) - 1, len(w) - 1, a, b)
    return "%d columns against %d" % (len(g) - 1, len(w) - 1)


def _pile_up(ring, monkeypatch, capfd, env, b, max_frag=0):
    """the batch through assemble + assemble_matrix of a fresh database handle with the route's switches -> (asm, {template: matrix text},
    the lines the launches printed)"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("KMAHIP_DEBUG_TIMING", "1")
    db = binding.KmaHipDB(ring["prefix"])
    try:
        D = int(db.info.DB_size)
        capfd.readouterr()
        asm = db.assemble(b.batch, b.rc, b.tmpl, b.traces, max_frag=max_frag, consensus=True)
        err = capfd.readouterr().err
        text = {}
        for t in range(1, D):
            mask = np.zeros(D, np.uint8)
            mask[t] = 1
            text[t] = db.assemble_matrix(mask)[0]
    finally:
        db.close()
    return asm, text, err


def _check(ring, b, per, asm, text):
    for t, (want_text, call) in per.items():
        assert text[t] == want_text, (t, _first_difference(text[t], want_text))
        assert (call["cover"], call["aln_len"], call["depth"], call["asm_len"]) == \
               (asm["cover"][t], asm["aln_len"][t], asm["depth"][t], asm["asm_len"][t]), t
        assert call["consensus"] == asm["consensus"][t], t


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_route(ring, monkeypatch, capfd, route, name):
    env, S, line = ROUTES[route]
    b, per = _want(ring, name, S, 0)
    assert pu.T_LONG in per
    asm, text, err = _pile_up(ring, monkeypatch, capfd, env, b)
    launches = LAUNCH.findall(err)
    assert launches == [line], err[-800:]               # one launch, on the route asked for; the long template in more than one unit
    _check(ring, b, per, asm, text)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("route", ["default", "seg256"])
def test_route_max_frag_5(ring, monkeypatch, capfd, route, name):
    """chunks of five reads, each back to front: another order of the same reads, so other depths under every new insertion column"""
    env, S, line = ROUTES[route]
    b, per = _want(ring, name, S, 5)
    if name not in ("rounds", "wrapped"):
        assert any(per[t][0] != _want(ring, name, S, 0)[1][t][0] for t in per)          # (the order is seen in the counts)
    asm, text, err = _pile_up(ring, monkeypatch, capfd, env, b, max_frag=5)
    assert LAUNCH.findall(err) == [line], err[-800:]
    _check(ring, b, per, asm, text)


def test_route_overflow_ladder(ring, monkeypatch, capfd):
    """KMAHIP_PILE_LDS_NODES=1 leaves a unit room for ONE insertion column. The long template's reads put one into every unit of 64
    columns, so every longer unit overflows: halved in half the LDS down to 256 columns, then all of the LDS, halved down to 64. The
    two whole templates need more than one column: their launch is repeated on HBM."""
    b, per = _want(ring, "ladder", 64, 0)
    asm, text, err = _pile_up(ring, monkeypatch, capfd, {"KMAHIP_PILE_LDS_NODES": "1"}, b)
    launches = LAUNCH.findall(err)
    want = ["8 units, 1024 columns per segment, half LDS, whole templates in LDS, run checkpoints",
            "14 units, 512 columns per segment, half LDS, whole templates in LDS, run checkpoints",
            "26 units, 256 columns per segment, half LDS, whole templates in LDS, run checkpoints",
            "26 units, 256 columns per segment, full LDS, whole templates in LDS, run checkpoints",
            "49 units, 128 columns per segment, full LDS, whole templates in LDS, run checkpoints",
            "96 units, 64 columns per segment, full LDS, whole templates in LDS, run checkpoints",
            "96 units, 64 columns per segment, full LDS, whole templates on HBM, run checkpoints"]
    assert launches == want, err[-1500:]
    for word in ("again with 512 columns", "again with 256 columns", "again with all of it", "again with 128 columns", "again with 64 columns",
                 "again with whole templates on HBM"):
        assert word in err, word
    _check(ring, b, per, asm, text)


@pytest.mark.parametrize("env", [{"KMAHIP_PILE_LDS_NODES": "1"}, {"KMAHIP_PILE_LDS_NODES": "1", "KMAHIP_PILE_FULL_LDS": "1"}], ids=["half", "full"])
@pytest.mark.parametrize("name", ["origin", "turns", "mix1"])
def test_whole_templates_after_an_overflow(ring, monkeypatch, capfd, name, env):
    """the reads of the two whole templates alone (one insertion column is all a cut template's unit could hold under this switch):
    LDS first, then HBM"""
    items = [x for x in pu.case(name, ring["seqs"], 1024) if x[0] != pu.T_LONG]
    b = pu.Batch(items)
    per = {}
    for t in (pu.T_MID, pu.T_SHORT):
        oa = b.oracle(ring["odb"], t, len(ring["seqs"][t - 1]))
        per[t] = (oa.matrix_text(ring["seqs"][t - 1]), oa.call())
    asm, text, err = _pile_up(ring, monkeypatch, capfd, env, b)
    launches = LAUNCH.findall(err)
    assert launches[-1].endswith("full LDS, whole templates on HBM, run checkpoints") and "whole templates in LDS" in launches[0], err[-800:]
    assert len(launches) == (2 if "KMAHIP_PILE_FULL_LDS" in env else 3)
    _check(ring, b, per, asm, text)


def test_sixteen_turns_and_the_refusal_of_more(ring, monkeypatch, capfd):
    """a cut template's sort key has room for sixteen turns of a read: sixteen are piled up (every column sixteen deep), one column
    more ends the call with KMAHIP_EINVAL and its own words -- alone in its batch, and with other reads beside it"""
    L = len(ring["seqs"][0])
    rng = np.random.default_rng(16)
    most = pu.make(ring["seqs"][0], 4321, 0, [("=", 16 * L)], rng)
    under = pu.make(ring["seqs"][0], 100, 0, pu.runs_from(300, I={150: 2}), rng)
    b = pu.Batch([(pu.T_LONG, under, False), (pu.T_LONG, most, True)])
    oa = b.oracle(ring["odb"], pu.T_LONG, L)
    counts, _ = oa.columns()
    assert int(counts.sum(axis=1).min()) == 16 and int(counts.sum(axis=1).max()) == 17
    asm, text, err = _pile_up(ring, monkeypatch, capfd, {}, b)
    _check(ring, b, {pu.T_LONG: (oa.matrix_text(ring["seqs"][0]), oa.call())}, asm, text)
    over = pu.make(ring["seqs"][0], 4321, 0, [("=", 16 * L + 1)], rng)
    for items in ([(pu.T_LONG, over, False)], [(pu.T_LONG, under, False), (pu.T_LONG, over, True), (pu.T_MID, pu.make(ring["seqs"][1], 5, 0, [("=", 90)], rng), False)]):
        bb = pu.Batch(items)
        db = binding.KmaHipDB(ring["prefix"])
        try:
            with pytest.raises(binding.KmaHipError) as e:
                db.assemble(bb.batch, bb.rc, bb.tmpl, bb.traces)
            assert "error -1" in str(e.value) and "more than 16 times" in str(e.value)
            # the handle is good for the next call
            asm = db.assemble(b.batch, b.rc, b.tmpl, b.traces, consensus=True)
            assert asm["asm_len"][pu.T_LONG] == L + 2
        finally:
            db.close()


def test_rounds_case_takes_the_run_loop_more_than_once(ring):
    b, _ = _want(ring, "rounds", 1024, 0)
    n = sorted(int(x) for x in b.n_ops)
    assert n[-1] > 6000 and sum(x > 2048 for x in n) >= 2 and sum(1024 < x <= 2048 for x in n) >= 2


def test_builder_round_trip_on_device_traces(golden_long):
    """fields 1-8 of the stats row of every read the device's own aligner kept, rebuilt from its start, clips and runs"""
    g = golden_long
    tlen = formats.read_lengths(g["prefix"])
    db = binding.KmaHipDB(g["prefix"])
    try:
        (_, _, T_off, _), h = db.map_se(g["batch"])
        cc = db.conclave_se(g["batch"].length, T_off, h)
        stats, off, nops, ops = db.align_trace(g["batch"], h["rc"], cc["tmpl"])
    finally:
        db.close()
    kept = np.nonzero(stats[:, 3])[0]
    assert len(kept) > 100
    classes = set()
    for i in kept:
        runs = pu.runs_of(ops[off[i]:off[i] + nops[i]])
        classes |= {c for c, _ in runs}
        t = abs(int(cc["tmpl"][i]))
        row = pu.stats_of(int(tlen[t]), int(stats[i, 1]), int(stats[i, 4]), runs, int(g["batch"].length[i]))
        assert list(row[1:9]) == [int(x) for x in stats[i, 1:9]], i
    assert classes == set("=XID")
