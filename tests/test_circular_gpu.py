"""Circular alignments (`-ca`: chainSeeds_circular, chain.c:262-494) and the presets `-mint2` / `-mint3` (kma.c:1069-1114).

Whole runs of examples/kmahip_map against the compiled reference (oracle/_ref/kma -t 1) run live on the same seeded input (circ_util:
reads that span the origin of their template), `.res`, `.fsa`, `.aln` and the inflated `.frag.gz` byte for byte, in every mode the
program serves; the side files; the library's `circular=` keyword. The reference's own output is checked first: it is deterministic,
files at least circ_util.FLOORS rows whose alignment ends before it starts with `-ca`, and none without."""
import os
import subprocess

import numpy as np
import pytest

import circ_util as cu
import golden_util
from kma_amd import binding, formats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    if not os.path.exists(cu.KMA):
        pytest.skip("oracle/_ref/kma not built")
    cu.build_map()
    made = {}

    def get(key):
        if key not in made:
            made[key] = cu.make_input(tmp_path_factory.mktemp("circ_" + key), key)
        return made[key]
    return get


def _same(s, tag, extra, env=None):
    """kmahip_map and the reference with the same options on input s: the four files agree; -> (reference's files, stem of ours)"""
    got = cu.run_map(s, tag, extra, env)
    return cu.assert_same_files(got, cu.ref(s, extra)), got


def _wraps(s, extra, plain):
    """the reference's run with `extra` (which holds -ca) drives the wrap paths: enough wrapped rows, none without the flag, another .res"""
    raw = cu.frag(cu.ref(s, extra))
    w, n = cu.wrapped(raw)
    assert w >= cu.FLOORS[s["key"]], (extra, w, n)
    w0, _ = cu.wrapped(cu.frag(cu.ref(s, plain)))
    assert w0 == 0, (plain, w0)
    assert cu.files(cu.ref(s, plain))[0] != cu.files(cu.ref(s, extra))[0]


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,extra", [("A", ["-1t1", "-ca"]), ("P", ["-1t1", "-ca"]), ("L", ["-Mt1", "1", "-ca"]), ("O", ["-1t1", "-ca"])],
                         ids=["A", "P", "L", "O"])
def test_reference_is_deterministic(inputs, key, extra):
    s = inputs(key)
    first = cu.files(cu.ref(s, extra))
    del s["runs"][" ".join(extra)]
    assert cu.files(cu.ref(s, extra)) == first


# ---- 1, 2: short reads ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KMAHIP_MAP_BATCH": "1000"}, {"KMAHIP_ALIGN_FAST": "0"}, {"KMAHIP_SEED_DIAG": "0"}],
                         ids=["default", "batch1000", "general_kernel", "seed_steps"])
def test_a_1t1(inputs, env):
    """the unrolled chain of align_fast_kernel, and (KMAHIP_ALIGN_FAST=0) the lane chain for every task"""
    s = inputs("A")
    _wraps(s, ["-1t1", "-ca"], ["-1t1"])
    _same(s, "a1t1" + "".join(env), ["-1t1", "-ca"], env)


def test_a_default_mode(inputs):
    s = inputs("A")
    _wraps(s, ["-ca"], [])
    _same(s, "adef", ["-ca"])


# ---- 3: pairs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["-1t1", "-ca"], ["-1t1", "-apm", "p", "-ca"], ["-ca"]], ids=["union", "penalty", "default_mode"])
def test_p_pairs(inputs, extra):
    s = inputs("P")
    _wraps(s, extra, [x for x in extra if x != "-ca"])
    _same(s, "p" + "".join(extra), extra)


# ---- 4: long reads ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["-Mt1", "1", "-ca"], ["-1t1", "-ca", "-bcNano"], ["-ca", "-bcNano"]], ids=["mt1", "1t1", "default_mode"])
def test_l_long_reads(inputs, extra):
    s = inputs("L")
    _wraps(s, extra, [x for x in extra if x != "-ca"])
    _same(s, "l" + "".join(extra), extra)


def test_l_long_reads_lane_chain(inputs):
    """the same reads with the long route off (KMAHIP_ALIGN_LONG=0): chain_seeds<true> of align_tasks_kernel on reads of many MEMs, its
    i + 128 window with the joins across the origin"""
    extra = ["-1t1", "-ca", "-bcNano"]
    _same(inputs("L"), "l1t1lane", extra, {"KMAHIP_ALIGN_LONG": "0"})


# ---- 5: reads as long as the template -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["-1t1", "-ca"], ["-Mt1", "2", "-ca"]], ids=["1t1", "mt1"])
def test_o_whole_turns(inputs, extra):
    s = inputs("O")
    _wraps(s, extra, [x for x in extra if x != "-ca"])
    _same(s, "o" + "".join(extra), extra)


# ---- 5b: more than one turn of a template the pile-up cuts into units ----------------------------------------------------------------------
M_RUNS = {"mt1": ["-Mt1", "1", "-ca", "-matrix", "-vcf", "-ef"], "1t1": ["-1t1", "-ca", "-bcNano", "-matrix"],
          "1t1_side": ["-1t1", "-ca", "-bcNano", "-matrix", "-vcf", "-ef"]}          # (the last one for a `.mapstat`: -Mt1 writes none)


def _rows_and_depths(stem):
    """-> {template name: (rows of .frag.gz filed under it, deepest column of its count matrix)}"""
    rows = {}
    for r in cu.frag_rows(cu.frag(stem)):
        rows[r[5]] = rows.get(r[5], 0) + 1
    blocks = cu.matrix_blocks(cu.gz(stem, ".mat.gz"))
    assert set(blocks) == set(rows)
    return {k: (rows[k], cu.deepest_column(blocks[k])) for k in rows}


@pytest.mark.parametrize("run", list(M_RUNS))
def test_m_reference_counts_the_second_turn(inputs, run):
    """the reference first: with -ca the reads of input M go round their template more than once and it counts every turn -- a column
    deeper than the template has reads, by TURNS_FLOOR at least; without -ca no column is deeper than the reads are many"""
    s = inputs("M")
    extra = M_RUNS[run]
    got = _rows_and_depths(cu.ref(s, extra))
    assert sum(n for n, _ in got.values()) == 60 and len(got) == (1 if run == "mt1" else 2)
    w, _ = cu.wrapped(cu.frag(cu.ref(s, extra)))
    assert w >= 20
    for name, (n, deepest) in got.items():
        print("input M %s %s: %d rows, deepest column %d" % (run, name.decode(), n, deepest))
        assert deepest >= n + cu.TURNS_FLOOR, (name, n, deepest)
    plain = _rows_and_depths(cu.ref(s, [x for x in extra if x != "-ca"]))
    for name, (n, deepest) in plain.items():
        assert deepest <= n, (name, n, deepest)


@pytest.mark.parametrize("env", [{}, {"KMAHIP_PILE_SEG_COLS": "256"}], ids=["default", "seg256"])
@pytest.mark.parametrize("run", list(M_RUNS))
def test_m_more_than_one_turn(inputs, run, env):
    """kmahip_map on input M: the pile-up takes a read that is longer than its cut template a turn at a time"""
    s = inputs("M")
    extra = M_RUNS[run]
    _, got = _same(s, "m" + run + "".join(env.values()), extra, env)
    want = cu.ref(s, extra)
    assert cu.gz(got, ".mat.gz") == cu.gz(want, ".mat.gz")
    if "-vcf" in extra:
        assert cu.gz(got, ".vcf.gz") == cu.gz(want, ".vcf.gz")
    if "-ef" in extra and "-Mt1" in extra:
        # (runKMA_Mt1 writes no extended-features file, mt1.c:313, 378: the option is taken and leaves none, on either side)
        assert not os.path.exists(got + ".mapstat") and not os.path.exists(want + ".mapstat")
    elif "-ef" in extra:
        assert cu.mapstat(got) == cu.mapstat(want)


def test_m_library_and_ring_walk(inputs):
    """the traces of align_trace_mt1(circular=True) on input M, piled up by the plain ring walk (oracle.Assembly) in stream order: the
    reference's own count matrix of its `-Mt1 1 -ca` run, whole turns and all; and the device's assemble + assemble_matrix on the same
    traces: the same text"""
    import oracle
    from kma_amd import synth
    s = inputs("M")
    want = cu.matrix_blocks(cu.gz(cu.ref(s, M_RUNS["mt1"]), ".mat.gz"))[s["names"][0].encode()]
    batch = formats.pack_ragged(s["reads"])
    tlen = formats.read_lengths(s["prefix"])
    db = binding.KmaHipDB(s["prefix"])
    try:
        (stats, off, nops, ops), rc = db.align_trace_mt1(batch, 1, circular=True)
        kept = stats[:, 3] != 0
        tmpl = kept.astype(np.int32)
        # stream order (`-Mt1`) through the ranks: the last read first in its chunk
        rank = np.arange(batch.n, dtype=np.int64)[::-1].copy()
        asm = db.assemble(batch, rc, tmpl, (stats, off, nops, ops), consensus=True, frag_rank=rank)
        mask = np.zeros(int(db.info.DB_size), np.uint8)
        mask[1] = 1
        text = db.assemble_matrix(mask)[0]
    finally:
        db.close()
    assert int(kept.sum()) == 60
    spans = stats[kept, 3] - stats[kept, 7]
    assert int((spans > tlen[1]).sum()) >= 20          # (reads of more than one turn, as traced)
    odb = oracle.OracleDB(s["prefix"])
    oa = oracle.Assembly(odb, 1, int(tlen[1]))
    for i in np.nonzero(kept)[0]:
        rd = synth.revcomp_codes(s["reads"][i]) if rc[i] & 1 else s["reads"][i]
        cols = "".join("=XID"[int(x) & 3] * (int(x) >> 2) for x in ops[off[i]:off[i] + nops[i]]).encode()
        oa.add(dict(cols=cols, start=int(stats[i, 1]), score=int(stats[i, 0]), clip_start=int(stats[i, 4])), rd)
    ring = oa.matrix_text(s["seqs"][0])
    assert ring == want
    assert text == want
    call = oa.call()
    assert (call["cover"], call["aln_len"], call["depth"], call["asm_len"]) == (asm["cover"][1], asm["aln_len"][1], asm["depth"][1], asm["asm_len"][1])
    assert call["consensus"] == asm["consensus"][1]


# ---- 6: the side outputs ------------------------------------------------------------------------------------------------------------------
def test_a_ef_matrix_vcf(inputs):
    s = inputs("A")
    extra = ["-1t1", "-ca", "-ef", "-matrix", "-vcf"]
    _, got = _same(s, "aemv", extra)
    want = cu.ref(s, extra)
    assert cu.mapstat(got) == cu.mapstat(want)
    for ext in (".mat.gz", ".vcf.gz"):
        assert cu.gz(got, ext) == cu.gz(want, ext), ext


def test_a_sam(inputs):
    s = inputs("A")
    extra = ["-1t1", "-ca", "-sam", "4"]
    got = cu.run_map(s, "asam", extra, stdout=True)
    want = cu.ref(s, extra, stdout=True)
    a, b = open(got + ".out", "rb").read(), open(want + ".out", "rb").read()
    body = lambda raw: [x for x in raw.split(b"\n") if x and not x.startswith(b"@PG")]  # noqa: E731
    assert body(a) == body(b)
    assert len(body(b)) > 2500
    cu.assert_same_files(got, want)


# ---- 7: the presets -----------------------------------------------------------------------------------------------------------------------
def _ref_preset(s, extra):
    want = cu.ref(s, extra)
    return cu.files(want) + (cu.gz(want, ".vcf.gz"),)


def _same_preset(s, extra):
    _, got = _same(s, "".join(extra), extra)
    want = cu.ref(s, extra)
    assert cu.mapstat(got) == cu.mapstat(want)
    assert cu.gz(got, ".vcf.gz") == cu.gz(want, ".vcf.gz")
    return _ref_preset(s, extra)


@pytest.mark.parametrize("extra", [["-mint2"], ["-mint3"], ["-mint3", "-bc", "0.9"], ["-bc", "0.9", "-mint3"]],
                         ids=["mint2", "mint3", "mint3_then_bc", "bc_then_mint3"])
def test_a_presets(inputs, extra):
    """the presets; a later option that overrides one of a preset's values; an earlier one. In the reference `-bc` and the presets
    share significantAndSupport's static threshold, which keeps the FIRST value it is given (assembly.c:153-157), while the `.vcf.gz`
    filter reads the variable only `-bc` sets (kma.c:747, vcf.c:195): a later `-bc 0.9` moves the VCF file and leaves the calls at the
    preset's 0.7, an earlier one decides the calls. Both orders must equal the reference's files, whatever they say."""
    s = inputs("A")
    w, _ = cu.wrapped(cu.frag(cu.ref(s, extra)))
    assert w >= cu.FLOORS["A"]
    ref = _same_preset(s, extra)
    if len(extra) > 1:
        assert ref != _ref_preset(s, ["-mint3"])          # (the other option reaches the run, before or behind the preset)


def test_a_mint2_is_not_mint3(inputs):
    s = inputs("A")
    assert cu.files(cu.ref(s, ["-mint2"]))[0] != cu.files(cu.ref(s, ["-mint3"]))[0]


# ---- 8: several ranks -----------------------------------------------------------------------------------------------------------------------
def test_a_two_ranks(inputs):
    s = inputs("A")
    extra = ["-1t1", "-ca"]
    got = cu.run_map(s, "aranks", ["-gpus", "2"] + extra, {"KMAHIP_COMM": "shm", "KMAHIP_SHARE_GPU": "1"})
    cu.assert_same_files(got, cu.ref(s, extra))


# ---- 9: -mem_mode, -proxi -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["-1t1", "-mem_mode", "-ca"], ["-1t1", "-ca", "-proxi", "0.9"]], ids=["mem_mode", "proxi"])
def test_a_mem_mode_and_proxi(inputs, extra):
    s = inputs("A")
    _wraps(s, extra, [x for x in extra if x != "-ca"])
    _same(s, "a" + "".join(extra), extra)


# ---- 10: the library ----------------------------------------------------------------------------------------------------------------------
def test_library_map_se_circular(inputs):
    """stage 3a by the library. A `.frag.gz` row holds the number of templates the read tied over and the one ConClave chose; its
    score, start and end are those of the stage-3c traceback, which seeds, chains and aligns like stage 3a and then adds Wl for an
    alignment that starts at the first or ends at the last template base (assembly.c:1931-1961). So stage 3a lists that template
    with that start and end, and the row's score is the read's best score plus those awards; run_se's traceback gives the row itself."""
    s = inputs("A")
    rows = {r[6]: r for r in cu.frag_rows(cu.frag(cu.ref(s, ["-1t1", "-ca"])))}
    ids = {n.encode(): x + 1 for x, n in enumerate(s["names"])}
    tlen = formats.read_lengths(s["prefix"])
    batch = formats.pack_ragged(s["reads"])
    db = binding.KmaHipDB(s["prefix"])
    try:
        assert db.params.ca == 0
        (_, _, T_off, _), h = db.map_se(batch, circular=True)
        assert db.params.ca == 0
        plain = db.map_se(batch)
        off = db.map_se(batch, circular=False)
        run = db.run_se(batch, circular=True)
        Wl = int(db.params.rw.Wl)
    finally:
        db.close()
    for a, b in zip(plain[0] + tuple(plain[1][k] for k in sorted(plain[1])), off[0] + tuple(off[1][k] for k in sorted(off[1]))):
        assert np.array_equal(a, b)
    assert not np.array_equal(plain[1]["best_score"], h["best_score"])
    seen = wrapped = 0
    bad = []
    for i in range(batch.n):
        r = rows.get(b"r%d" % i)
        if r is None:
            assert run["tmpl"][i] == 0 or run["trace_stats"][i, 3] == 0, i
            continue
        seen += 1
        n, t, score, start, end = int(r[1]), ids[r[5]], int(r[2]), int(r[3]), int(r[4])
        o = int(T_off[i])
        hit = [(abs(int(h["tmpl"][o + x])), int(h["start"][o + x]), int(h["end"][o + x])) for x in range(int(h["n_hits"][i]))]
        award = Wl * ((start == 0) + (end == tlen[t]))
        if not (int(h["n_hits"][i]) == n and (t, start, end) in hit and int(h["best_score"][i]) + award == score):
            bad.append((i, r[1:6], hit, int(h["best_score"][i])))
        st = run["trace_stats"][i]
        assert (abs(int(run["tmpl"][i])), int(run["n_hits"][i]), int(st[0]), int(st[1]), int(st[2])) == (t, n, score, start, end), (i, r[1:6], st)
        wrapped += end < start
    print("map_se(circular=True): %d rows, %d wrapped, %d differ from their row" % (seen, wrapped, len(bad)), bad[:5])
    assert not bad
    assert seen == len(rows) and seen > 2900 and wrapped >= cu.FLOORS["A"]


# ---- 11: inert where no read wraps --------------------------------------------------------------------------------------------------------
def test_golden_se_unmoved(inputs, tmp_path, golden_se):
    fq = os.path.join(golden_util.GOLD, "se", "reads.fq.gz")
    s = dict(tmp=tmp_path, key="se", prefix=golden_se["prefix"], fq=fq, fq2=None, runs={})
    extra = ["-1t1", "-ca"]
    r, _ = _same(s, "se", extra)
    assert r[3].count(b"\n") > 900
    assert cu.wrapped(r[3])[0] == 0
