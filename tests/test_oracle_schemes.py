"""The oracle OFF the reference's default scoring scheme, pinned to the reference on the CPU -- what tests/test_schemes_gpu.py then holds
the kernels against. The planted reads of tests/scheme_sets.py through the oracle's scan, stage 3a, ConClave and traceback under every
scheme of its table, against the fragment rows the compiled reference wrote under the same scheme (tests/golden/schemes, made by
tests/golden/make_golden_schemes.py); where oracle/_ref/kma is built the binary is run again and must still write those rows, and the
chain finder is compared with its `-s2` tap. The guards assert on the oracle's own output that the reads stand where the schemes decide."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle
import scheme_sets as ss
from kma_amd import formats, synth

_inputs = {}
_results = {}


def inputs(tmp_path_factory):
    """index, FASTQ files, reads and couples of the scheme tests, written once per session"""
    if not _inputs:
        inp = ss.write_inputs(tmp_path_factory.mktemp("schemes"))
        inp["codes"] = [r for _, _, r in inp["reads"]]
        inp["batch"] = formats.pack_ragged(inp["codes"])
        inp["tlen"] = formats.read_lengths(inp["prefix"])
        _inputs.update(inp)
    return _inputs


def _codes(inp, part):
    if part == "all":
        return inp["codes"]
    if part == "device":
        return [inp["codes"][i] for i in ss.gpu_subset(inp["reads"])]
    if "long" not in inp:
        inp["long"] = ss.long_set()
    return inp["long"]


def oracle_run(inp, scheme, part="all"):
    """scan -> stage 3a -> ConClave -> traceback by the oracle under a scheme, of all short reads, of the part of them the device tests
    run ("device": ss.gpu_subset) or of the long reads ("long"), computed once -> dict(odb, codes, batch, scan, o, cc, ok,
    filed = [(position in the batch, read as aligned, template)], trace = {position: result or None})"""
    key = (scheme, part)
    if key not in _results:
        odb = oracle.OracleDB(inp["prefix"])
        ss.apply(odb.rw, ss.SCHEMES[scheme])
        codes = _codes(inp, part)
        b = inp["batch"] if part == "all" else formats.pack_ragged(codes)
        scan = odb.scan_se(b)
        o = odb.align_se(b, *scan)
        tlen = inp["tlen"]
        cc = oracle.conclave(o["n_hits"], o["best_score"], b.length, np.zeros(b.n, np.int32), scan[2][:-1], o["tmpl"], o["start"], o["end"],
                             o["alignment_scores"], o["uniq_alignment_scores"], tlen)
        ok = np.asarray(oracle.res_stats(cc["w_scores"], tlen)["significant"], np.uint8)
        al = oracle.OracleAligner(odb)
        filed, trace = [], {}
        for i in range(b.n):
            tt = int(cc["tmpl"][i])
            if tt == 0 or not ok[abs(tt)]:
                continue
            rd = codes[i]
            if (int(o["out_flag"][i]) & 16 != 0) != (tt < 0):
                rd = synth.revcomp_codes(rd)
            filed.append((i, rd, abs(tt)))
            trace[i] = al.align_trace(rd, abs(tt))
        _results[key] = dict(odb=odb, codes=codes, batch=b, scan=scan, o=o, cc=cc, ok=ok, filed=filed, trace=trace)
    return _results[key]


def rows_of(inp, res):
    """the oracle's result as the reference's reduced fragment rows"""
    return [("r%d" % i, str(int(res["o"]["n_hits"][i])), str(tr["score"]), str(tr["start"]), str(tr["end"]), inp["names"][t - 1])
            for i, _, t in res["filed"] for tr in [res["trace"][i]] if tr is not None]


def figures(res, n):
    """(score, start, end) per read, None where the read yields no row"""
    return [None if res["trace"].get(i) is None else tuple(res["trace"][i][k] for k in ("score", "start", "end")) for i in range(n)]


@pytest.mark.parametrize("scheme", list(ss.SCHEMES))
def test_oracle_rows_equal_the_reference_under_every_scheme(tmp_path_factory, tmp_path, scheme):
    """-1t1: name, ties, score, start, end and template of every fragment row. The default mode: the chain finder hands every planted read
    on as one record, which stage 3a and the traceback then treat as -1t1 treats the read, so the recorded default-mode row of such a
    read must be the oracle's -1t1 row. Where oracle/_ref/kma is built it is run again in both modes and must write the recorded rows."""
    inp = inputs(tmp_path_factory)
    res = oracle_run(inp, scheme)
    want = ss.load_rows(scheme, "1t1")
    got = rows_of(inp, res)
    assert len(want) > 2000
    for g, w in zip(got, want):
        assert g == w, (scheme, g, w)
    assert len(got) == len(want)
    whole = {i for i, recs in enumerate(res["odb"].scan_chain(inp["batch"])) if len(recs) == 1}
    rec = {w[0]: w for w in ss.load_rows(scheme, "default")}
    same = 0
    for g in got:
        if int(g[0][1:]) in whole:
            assert rec.get(g[0]) == g, (scheme, g, rec.get(g[0]))
            same += 1
    print(scheme, "default mode:", same, "rows of reads handed on whole")
    assert same > 1500
    if os.path.exists(oracle.REF_KMA):
        for mode in ss.MODES:
            assert [tuple(r) for r in ss.reference_rows(oracle.REF_KMA, inp, scheme, mode, str(tmp_path / "out"))] == ss.load_rows(scheme, mode), (scheme, mode)


@pytest.mark.parametrize("scheme", list(ss.SCHEMES))
def test_oracle_chain_finder_equals_the_reference_under_every_scheme(tmp_path_factory, tmp_path, scheme):
    """`kma -s2` without -1t1 under the scheme's options against oracle.scan_chain with the scheme in its Rewards: the same records in the
    same order (one record per planted read: what the default-mode rows of the test above lean on). Skipped where oracle/_ref/kma has
    not been built."""
    if not os.path.exists(oracle.REF_KMA):
        pytest.skip("oracle/_ref/kma not built")
    inp = inputs(tmp_path_factory)
    res = oracle_run(inp, scheme)
    tap = subprocess.run([oracle.REF_KMA, "-i", inp["fq"], "-o", str(tmp_path / "o"), "-t_db", inp["prefix"], "-t", "1", "-s2"] + ss.options(scheme),
                         check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    want, _ = formats.parse_s2(tap)
    per_read = res["odb"].scan_chain(inp["batch"])
    flat = [(b"r%d" % i + bytes(2) + struct.pack("<2i", qs, qe), rf, tuple(int(t) for t in T)) for i, recs in enumerate(per_read) for rf, er, qs, qe, T in recs]
    ref = [(w["hdr"], w["rc_flag"], tuple(int(x) for x in w["T"])) for w in want]
    for x, (a, c) in enumerate(zip(flat, ref)):
        assert a == c, (scheme, x, a, c)
    assert len(flat) == len(ref) > 2000


def test_host_predicate_equals_its_restatement_under_every_scheme():
    """kmahip_diag_gap_m_max, the one host function in front of nw_diagonal and of the traceback's first pass, against ss.gap_m_max: the
    values 1, 2, 3 and 6, the tie that only the `- 1` keeps at 2, and -1 for the schemes at equality or with a table that is not plain"""
    from kma_amd import binding
    got = {}
    for name, s in ss.SCHEMES.items():
        rw = binding.Rewards()
        ss.apply(rw, s)
        got[name] = binding.diag_gap_m_max(rw)
        assert got[name] == ss.gap_m_max(s) and (got[name] >= 0) == ss.is_plain(s), (name, got[name])
    assert {got[k] for k in ("default", "cge", "gmm1", "gmm6", "tie")} == {1, 2, 3, 6} and got["tie"] == 2
    assert got["edge_wu"] == got["mm_eq_w1"] == got["tstv"] == -1


def _by_kind(inp, kind):
    return [(i, p) for i, (k, p, _) in enumerate(inp["reads"]) if k == kind]


def test_read_sets_stand_where_the_schemes_decide(tmp_path_factory):
    """what keeps tests/test_schemes_gpu.py from passing vacuously, asserted on the oracle's output alone: under every plain scheme at
    least 20 link reads with exactly gap_m_max mismatches, and 20 with one more, come out without a gap; at least 100 reads per scheme
    carry a gap; the tie scheme has 20 link reads with three mismatches; every scheme but the default moves score, start or end of at
    least 60 reads (the pairing reward: of 60 couples' records). The same must hold on the part of the set the device tests run."""
    inp = inputs(tmp_path_factory)
    n = len(inp["reads"])
    sub = ss.gpu_subset(inp["reads"])
    base = figures(oracle_run(inp, "default"), n)
    links = _by_kind(inp, "link")
    for scheme, s in ss.SCHEMES.items():
        res = oracle_run(inp, scheme)
        tr = res["trace"]
        for part, least in ((range(n), 20), (sub, 8)):
            part = set(part)
            gaps = sum(1 for i in part if tr.get(i) is not None and ss.cigar_has_gap(tr[i]["cigar"]))
            counts = {"gaps": gaps}
            if ss.is_plain(s):
                g = ss.gap_m_max(s)
                for m in (g, g + 1):
                    counts["m%d" % m] = sum(1 for i, p in links if i in part and p[0] == m and tr.get(i) is not None and not ss.cigar_has_gap(tr[i]["cigar"]))
                    assert counts["m%d" % m] >= least, (scheme, counts)
            if scheme == "tie":
                counts["m3"] = sum(1 for i, p in links if i in part and p[0] == 3 and tr.get(i) is not None and tr[i]["cigar"].count("X") == 3)
                assert counts["m3"] >= least, (scheme, counts)
            assert gaps >= (100 if least == 20 else 40), (scheme, counts)
            if scheme not in ("default", "pe20"):
                fig = figures(res, n)
                counts["moved"] = sum(1 for i in part if fig[i] != base[i])
                assert counts["moved"] >= (60 if least == 20 else 24), (scheme, counts)
            print(scheme, "all" if least == 20 else "device part", "plain" if ss.is_plain(s) else "not plain", "gap_m_max", ss.gap_m_max(s), counts)


def couples_input(inp):
    """the couples in the form of the paired fixtures (tests/pe_util.py): dict(prefix, s1, units)"""
    s1 = []
    for j, (a, b) in enumerate(inp["couples"]):
        for m in (a, b):
            pk = formats.pack_ragged([m])
            s1.append(dict(seq=np.asarray(pk.seq[:int(pk.seq_off[1]) if len(pk.seq_off) > 1 else len(pk.seq)]), seqlen=len(m),
                           N=np.asarray(pk.N, np.int32), hdr=b"r%d" % j, pair=1))
    return dict(prefix=inp["prefix"], s1=s1, units=[("pe", 2 * j, 2 * j + 1) for j in range(len(inp["couples"]))])


def couple_records(inp, scheme):
    import pe_util
    key = ("pe", scheme)
    if key not in _results:
        _results[key] = pe_util.oracle_pe_conclave_records(couples_input(inp), set_rewards=lambda rw: ss.apply(rw, ss.SCHEMES[scheme]))
    return _results[key]


def record_rows(r):
    off = np.concatenate([r["off"], [len(r["tmpl"])]])
    return [(int(r["n_hits"][x]), int(r["score"][x]), int(r["q_len"][x]), int(r["q_len2"][x])) +
            tuple(tuple(int(v) for v in r[k][off[x]:off[x + 1]]) for k in ("tmpl", "start", "end")) for x in range(len(r["n_hits"]))]


@pytest.mark.parametrize("scheme", ss.PE_SCHEMES)
def test_oracle_couples_equal_the_reference_under_the_pairing_schemes(tmp_path_factory, scheme):
    """`-1t1 -ipe ... -apm p`: the oracle's paired records (stage 2's pairing, alnFragsPenaltyPE) through ConClave against the recorded
    rows: the template and the number of equally good templates of every couple's rows. Every scheme moves at least 60 records
    relative to the default scheme."""
    inp = inputs(tmp_path_factory)
    r = couple_records(inp, scheme)
    tlen = inp["tlen"]
    cc = oracle.conclave(r["n_hits"], r["score"], r["q_len"], r["q_len2"], r["off"], r["tmpl"], r["start"], r["end"],
                         r["alignment_scores"], r["uniq_alignment_scores"], tlen)
    want = ss.load_rows(scheme, "pe")
    got = []
    for x in range(len(r["n_hits"])):
        tt = int(cc["tmpl"][x])
        if tt:
            got += [("r%d" % r["unit"][x], str(int(r["n_hits"][x])), inp["names"][abs(tt) - 1])] * (2 if r["q_len2"][x] else 1)
    # (mates filed under different templates: their rows stand in the file in the order of the templates, not of the mates)
    assert sorted(got) == sorted((w[0], w[1], w[5]) for w in want) and len(want) > 500
    moved = len(set(record_rows(couple_records(inp, "default"))) ^ set(record_rows(r))) // 2
    print(scheme, "couples' records moved:", moved)
    assert moved >= 60, (scheme, moved)
