"""The counting scan (`-ck`, kmahip_ws_set_count_kmers, scan_count_kernel) on the device: stage 2 against the reference's `-s2` taps of
`-ck` (tests/golden/ck, make_golden_ck.py) and against the Python restatement (tests/ck_util.py, which test_ck_oracle.py pins to the
same taps) array for array; both hand-ons of the LDS tiers; the pool's retry; a database with 32-bit value lists; whole runs of
examples/kmahip_map against the compiled reference (oracle/_ref/kma -t 1) live on the same input, `.res`, `.fsa`, `.aln` and the
inflated `.frag.gz` byte for byte; and the runs in which the option is taken without effect."""
import gzip
import lzma
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ck_util
import decon_util
import golden_util
import proxi_util
from kma_amd import binding, formats
from proxi_util import KMA, MAP

pytestmark = pytest.mark.gpu
CK = os.path.join(golden_util.GOLD, "ck")
K = 16
TIMEOUT = 120


def _same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _tap(name):
    with gzip.open(os.path.join(CK, name), "rb") as f:
        return formats.parse_s2(f.read())[0]


# ---- stage 2, single end: the taps on tests/golden/se ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hipdb(golden_se):
    db = binding.KmaHipDB(golden_se["prefix"])
    yield db
    db.close()


@pytest.fixture(scope="module")
def ck_scan(golden_se, hipdb):
    """count_kmers=True with everything else at its default, computed once"""
    return hipdb.scan_se(golden_se["batch"], count_kmers=True)


def test_scan_se_matches_the_ck_tap(golden_se, ck_scan):
    assert golden_util.check_scan_against_s2(golden_se["s1"], _tap("s2_ck.bin.gz"), *ck_scan) == 912


@pytest.mark.parametrize("name,kw", [("s2_ck_ex.bin.gz", dict(exhaustive=1)), ("s2_ck_p07.bin.gz", dict(min_frac=0.7))], ids=["ex_mode", "proxi07"])
def test_scan_se_matches_the_ck_taps_with_other_options(golden_se, hipdb, name, kw):
    got = hipdb.scan_se(golden_se["batch"], count_kmers=True, **kw)
    assert golden_util.check_scan_against_s2(golden_se["s1"], _tap(name), *got) > 900


def test_counts_are_not_the_plain_scan(golden_se, hipdb, ck_scan):
    plain = hipdb.scan_se(golden_se["batch"])
    golden_util.check_scan_against_s2(golden_se["s1"], golden_se["s2"], *plain)
    assert int((plain[0] != ck_scan[0]).sum()) > 200


def test_plain_path_untouched(golden_se, hipdb):
    """count_kmers=False is the call that never names the option, also after a counting call and after the setting was on and off"""
    never = hipdb.scan_se(golden_se["batch"])
    assert hipdb.count_kmers is False
    assert _same_arrays(hipdb.scan_se(golden_se["batch"], count_kmers=False), never)
    hipdb.scan_se(golden_se["batch"], count_kmers=True)
    assert hipdb.count_kmers is False and _same_arrays(hipdb.scan_se(golden_se["batch"]), never)
    hipdb.set_count_kmers(True)
    hipdb.set_count_kmers(False)
    assert _same_arrays(hipdb.scan_se(golden_se["batch"]), never)


def test_workspace_setting_is_the_keyword(golden_se, hipdb, ck_scan):
    hipdb.set_count_kmers(True)
    try:
        assert _same_arrays(hipdb.scan_se(golden_se["batch"]), ck_scan)
    finally:
        hipdb.set_count_kmers(False)


def test_scan_se_same_after_the_pool_retry(golden_se, ck_scan, monkeypatch):
    """one int of pool per read: the lists longer than the inline slots do not fit, the call is repeated with a larger pool"""
    monkeypatch.setenv("KMAHIP_SCAN_POOL_PER_READ", "1")
    db = binding.KmaHipDB(golden_se["prefix"])
    try:
        assert _same_arrays(db.scan_se(golden_se["batch"], count_kmers=True, min_frac=0.7),
                            ck_util.scan_se(_se_dict(golden_se), K, golden_se["reads"], min_frac=0.7))
        assert _same_arrays(db.scan_se(golden_se["batch"], count_kmers=True), ck_scan)
    finally:
        db.close()


_SE_DICT = {}


def _se_dict(golden_se):
    if "d" not in _SE_DICT:
        _SE_DICT["d"] = ck_util.kmer_dict(ck_util.read_fasta(os.path.join(golden_util.GOLD, "se", "db.fsa.gz"))[1], K)
    return _SE_DICT["d"]


def test_scan_se_equals_the_restatement(golden_se, ck_scan):
    assert _same_arrays(ck_scan, ck_util.scan_se(_se_dict(golden_se), K, golden_se["reads"]))


# ---- stage 2, single end: the edge set ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ck_edge")
    prefix = str(tmp / "edge")
    with lzma.open(os.path.join(CK, "edge.comp.b.xz"), "rb") as f, open(prefix + ".comp.b", "wb") as g:
        shutil.copyfileobj(f, g)
    for ext in (".length.b", ".seq.b", ".name"):
        shutil.copy(os.path.join(CK, "edge" + ext), prefix + ext)
    _, seqs = ck_util.read_fasta(os.path.join(CK, "edge.fsa.gz"))
    names, reads = ck_util.read_fastq(os.path.join(CK, "edge.fq.gz"))
    db = binding.KmaHipDB(prefix)
    yield dict(db=db, names=names, reads=reads, batch=formats.pack_ragged(reads), d=ck_util.kmer_dict(seqs, K), prefix=prefix, tmp=tmp)
    db.close()


@pytest.mark.parametrize("ex", [0, 1], ids=["ck", "ck_ex_mode"])
def test_edge_set_equals_the_restatement_and_the_tap(edge, ex):
    got = edge["db"].scan_se(edge["batch"], exhaustive=ex, count_kmers=True)
    assert _same_arrays(got, ck_util.scan_se(edge["d"], K, edge["reads"], exhaustive=bool(ex)))
    want = {r["hdr"].rstrip(b"\0").split()[0].decode(): r for r in _tap("s2_edge_ex.bin.gz" if ex else "s2_edge.bin.gz")}
    rc_flag, flag, T_off, T = got
    for i, n in enumerate(edge["names"]):
        lst = T[T_off[i]:T_off[i + 1]].tolist()
        if n in want:
            assert (int(rc_flag[i]), int(flag[i]), lst) == (want[n]["rc_flag"], want[n]["flag"], want[n]["T"].tolist()), n
        else:
            assert lst == [], n
    assert len(want) == (21 if ex else 20)          # (of 24 reads: exact30, len15 and len16 have no record, offstride only under -ex_mode)


def test_edge_set_takes_both_hand_ons(edge):
    """fam15 and fam62 do not fit the first tier's 14 places, fam63, fam80 and fam80_rev not the second tier's 62"""
    edge["db"].scan_se(edge["batch"], count_kmers=True)
    tier2, dense = edge["db"].get_scan_overflow()
    assert tier2 == 5 and dense == 3, (tier2, dense)


def test_edge_set_with_proximity_matching_equals_the_restatement(edge):
    for f in (0.5, 0.9):
        assert _same_arrays(edge["db"].scan_se(edge["batch"], min_frac=f, count_kmers=True), ck_util.scan_se(edge["d"], K, edge["reads"], min_frac=f))


def test_edge_set_same_after_the_pool_retry(edge, monkeypatch):
    monkeypatch.setenv("KMAHIP_SCAN_POOL_PER_READ", "1")
    db = binding.KmaHipDB(edge["prefix"])
    try:
        assert _same_arrays(db.scan_se(edge["batch"], count_kmers=True), ck_util.scan_se(edge["d"], K, edge["reads"]))
    finally:
        db.close()


@pytest.mark.parametrize("apm,tag", [(0, "p"), (1, "u")], ids=["apm_p", "apm_u"])
def test_edge_pairs_match_the_taps(edge, apm, tag):
    """four pairs (make_golden_ck.py): a couple, a pair with one mate unmapped, and two pairs on either side of best1 + best2 - PE
    against the summed count of the best common template -- `together` is a couple under the pairing penalty and two records under
    the union pairing. Every record of the tap in stream order: name, rc_flag, flag, list."""
    names, m1 = ck_util.read_fastq(os.path.join(CK, "edge_r1.fq.gz"))
    _, m2 = ck_util.read_fastq(os.path.join(CK, "edge_r2.fq.gz"))
    want = [(r["hdr"].rstrip(b"\0").decode(), int(r["rc_flag"]), int(r["flag"]), r["T"].tolist()) for r in _tap("s2_edge_pe_%s.bin.gz" % tag)]
    edge["db"].params.apm = apm
    try:
        mate, rc, rc_flag, flag, R_off, T = edge["db"].scan_pe(formats.pack_ragged([x for ab in zip(m1, m2) for x in ab]), count_kmers=True)
    finally:
        edge["db"].params.apm = 0
    got = [(names[x // 2], int(rc_flag[x]), int(flag[x]), T[R_off[x]:R_off[x + 1]].tolist()) for x in range(2 * len(names)) if mate[x] >= 0]
    assert got == want and len(want) == 7
    assert (("together", 85, 99, []) in want) == (tag == "p")
    # and array for array the restated pairing over the restated candidates (tests/ck_util.py), strands and mates included
    assert _pair_arrays(mate, rc, rc_flag, flag, R_off, T) == _restated_pairs(edge["d"], m1, m2, union=bool(apm))


def _pair_arrays(mate, rc, rc_flag, flag, R_off, T):
    """what scan_pe returned, slot by slot: (mate, rc, rc_flag, flag, list) or None for an empty slot"""
    return [(int(mate[x]), int(rc[x]), int(rc_flag[x]), int(flag[x]), T[R_off[x]:R_off[x + 1]].tolist()) if mate[x] >= 0 else None
            for x in range(len(mate))]


def _restated_pairs(d, m1, m2, union):
    """the same slots from the restatement: a pair's records in the order printed; a pair with one record keeps it in the mate's slot"""
    out = []
    for a, b in zip(m1, m2):
        recs = [(r["mate"], r["rc"], r["rc_flag"], r["flag"], r["T"].tolist()) for r in ck_util.scan_pair(d, K, a, b, union=union)]
        if len(recs) == 2:
            out += recs
        elif len(recs) == 1:
            out += [recs[0], None] if recs[0][0] == 0 else [None, recs[0]]
        else:
            out += [None, None]
    return out


@pytest.mark.parametrize("apm", [0, 1], ids=["apm_p", "apm_u"])
def test_scan_pe_equals_the_restated_pairing_on_the_paired_fixture(golden_pe, apm):
    """every pair of tests/golden/pe (135 of its mates hold an N): the device's slots against save_kmers_penaltyPair /
    save_kmers_unionPair restated over get_kmers_for_pair_count, which walks each strand between its own N positions"""
    g = golden_pe
    d = ck_util.kmer_dict(ck_util.read_fasta(os.path.join(golden_util.GOLD, "pe", "db.fsa.gz"))[1], K)
    pairs = [u for u in g["units"] if u[0] == "pe"]
    m1, m2 = [_codes(g["s1"][u[1]]) for u in pairs], [_codes(g["s1"][u[2]]) for u in pairs]
    db = binding.KmaHipDB(g["prefix"])
    try:
        db.params.apm = apm
        got = db.scan_pe(formats.pack_ragged([x for ab in zip(m1, m2) for x in ab]), count_kmers=True)
    finally:
        db.close()
    assert _pair_arrays(*got) == _restated_pairs(d, m1, m2, union=bool(apm))


# ---- stage 2, paired: the taps on tests/golden/pe ---------------------------------------------------------------------------------------------
def _codes(r):
    c = formats.unpack_words(r["seq"], r["seqlen"]).copy()
    if len(r["N"]):
        c[r["N"]] = 4
    return c


def _pe_device(g, db, singles_by_chain):
    pairs = [u for u in g["units"] if u[0] == "pe"]
    singles = [u for u in g["units"] if u[0] == "se"]
    pb = formats.pack_ragged([_codes(g["s1"][i]) for u in pairs for i in (u[1], u[2])])
    mate, rc, rc_flag, flag, R_off, T = db.scan_pe(pb, count_kmers=True)
    pair_res = {}
    for j, u in enumerate(pairs):
        pair_res[u[1]] = [dict(mate=int(mate[x]), rc=int(rc[x]), rc_flag=int(rc_flag[x]), flag=int(flag[x]), T=T[R_off[x]:R_off[x + 1]])
                          for x in (2 * j, 2 * j + 1) if mate[x] >= 0]
    sb = formats.pack_ragged([_codes(g["s1"][u[1]]) for u in singles])
    if singles_by_chain:
        return pair_res, db.scan_chain(sb), len(pairs)
    rf, fl, To, Ts = db.scan_se(sb, count_kmers=True)
    return pair_res, {u[1]: ((int(rf[j]), int(fl[j]), Ts[To[j]:To[j + 1]]) if To[j + 1] > To[j] else None) for j, u in enumerate(singles)}, len(pairs)


@pytest.mark.parametrize("apm,tap", [(0, "s2_ck_pe_p.bin.gz"), (1, "s2_ck_pe_u.bin.gz")], ids=["apm_p", "apm_u"])
def test_scan_pe_matches_the_ck_taps(golden_pe, apm, tap):
    import oracle
    g = golden_pe
    db = binding.KmaHipDB(g["prefix"])
    try:
        db.params.apm = apm
        pair_res, single_res, n_pairs = _pe_device(g, db, False)
    finally:
        db.close()
    idx = {id(r): i for i, r in enumerate(g["s1"])}
    got = golden_util.pe_stream_from(g, lambda a, b: pair_res[idx[id(a)]], lambda r: single_res[idx[id(r)]], oracle.rc_packed)
    want = gzip.open(os.path.join(CK, tap), "rb").read()
    assert n_pairs > 500 and got == want
    assert want != g["s2_bytes"]


def test_scan_pe_in_the_default_mode_matches_the_ck_tap(golden_pe):
    """`kma -ipe r1 r2 -ck` without -1t1: the couples by union pairing over the counted candidates, the records that lost their mate
    through the chain finder, which does not read the option"""
    import oracle
    g = golden_pe
    want = gzip.open(os.path.join(CK, "s2_ck_pe_default.bin.gz"), "rb").read()
    db = binding.KmaHipDB(g["prefix"])
    try:
        db.params.apm = 1
        pair_res, ch, _ = _pe_device(g, db, True)
    finally:
        db.close()
    by_single = {}
    for x in range(len(ch["read"])):
        by_single.setdefault(int(ch["read"][x]), []).append(x)
    out, j = b"", 0
    for u in g["units"]:
        if u[0] == "se":
            r = g["s1"][u[1]]
            for x in by_single.get(j, []):
                words, N = (oracle.rc_packed(r["seq"], r["seqlen"], r["N"]) if ch["emit_rc"][x] else (r["seq"], r["N"]))
                out += golden_util.s2_record_bytes(r["seqlen"], words, N, int(ch["rc_flag"][x]), ch["T"][ch["T_off"][x]:ch["T_off"][x + 1]],
                                                   r["hdr"] + b"\x00" + struct.pack("<2i", int(ch["q_start"][x]), int(ch["q_end"][x])), 0)
            j += 1
        else:
            a, b = g["s1"][u[1]], g["s1"][u[2]]
            for rec in pair_res[u[1]]:
                r = (a, b)[rec["mate"]]
                words, N = (oracle.rc_packed(r["seq"], r["seqlen"], r["N"]) if rec["rc"] else (r["seq"], r["N"]))
                out += golden_util.s2_record_bytes(r["seqlen"], words, N, int(rec["rc_flag"]), rec["T"], r["hdr"], int(rec["flag"]))
    out += struct.pack("<i", -len(g["units"]))
    assert out == want


def test_chain_finder_ignores_the_option(golden_se, hipdb):
    plain = hipdb.scan_chain(golden_se["batch"])
    hipdb.set_count_kmers(True)
    try:
        with_ck = hipdb.scan_chain(golden_se["batch"])
    finally:
        hipdb.set_count_kmers(False)
    assert all(np.array_equal(plain[k], with_ck[k]) for k in plain)


# ---- a database with 32-bit value lists ---------------------------------------------------------------------------------------------------------
def test_large_database_of_32_bit_value_lists(tmp_path):
    """66 000 templates of 40 bases, built by kmahip_index: DB_size >= 65535 switches the value lists to 32-bit elements. The last
    hundred templates repeat the first hundred, so the reads' lists name ids on both sides of 2^16."""
    rng = np.random.default_rng(66)
    D, L = 66000, 40
    seqs = rng.integers(0, 4, (D, L), dtype=np.uint8)
    seqs[D - 100:] = seqs[:100]
    fa = str(tmp_path / "wide.fsa")
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(fa, "wb") as f:
        f.write(b"".join(b">t%d\n" % i + lut[s].tobytes() + b"\n" for i, s in enumerate(seqs)))
    prefix = str(tmp_path / "wide")
    binding.index_build([fa], prefix)
    picks = [0, 1, 50, 99, 100, 101, 30000, 65533, 65534, 65535, 65536, 65899, 65900, 65950, 65999]
    reads = []
    for i, t in enumerate(picks):
        r = seqs[t].copy()
        if i % 3 == 1:
            r = (3 - r[::-1]).astype(np.uint8)
        if i % 4 == 2:
            r = np.concatenate([r, seqs[(t + 7) % D][:30]])          # a second template, fewer k-mers
        if i % 5 == 3:
            r[7] = 4
        reads.append(r)
    reads += [np.concatenate([seqs[5], seqs[65905][::-1]]), rng.integers(0, 4, 60, dtype=np.uint8), seqs[12][:30]]
    # the dictionary of the reads' k-mers alone: every template's k-mers in one array, looked up by value
    pw = (np.uint64(4) ** np.arange(K - 1, -1, -1, dtype=np.uint64))
    km = np.stack([(seqs[:, s:s + K].astype(np.uint64) * pw).sum(1) for s in range(L - K + 1)], 1)
    need = set()
    for r in reads:
        for codes in ck_util.strands(r)[0::2]:
            need.update(ck_util._kmers(codes, K).tolist())
    d = {}
    hit = np.isin(km, np.fromiter(need, np.uint64, len(need)))
    for t, s in zip(*np.nonzero(hit)):
        lst = d.setdefault(int(km[t, s]), [])
        if not lst or lst[-1] != t + 1:
            lst.append(int(t) + 1)
    d = {x: tuple(v) for x, v in d.items()}
    db = binding.KmaHipDB(prefix)
    try:
        got = db.scan_se(formats.pack_ragged(reads), count_kmers=True)
        want = ck_util.scan_se(d, K, reads)
        assert _same_arrays(got, want)
        assert int((want[0] != 0).sum()) >= 15 and int(want[3].max()) > 65536 and int(np.abs(want[3]).min()) < 100
        got = db.scan_se(formats.pack_ragged(reads), count_kmers=True, min_frac=0.5)
        assert _same_arrays(got, ck_util.scan_se(d, K, reads, min_frac=0.5))
    finally:
        db.close()


# ---- whole runs against the binary ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    proxi_util.build_map()
    tmp = tmp_path_factory.mktemp("ck_runs")
    s = proxi_util.make_input(tmp, "c")
    g = decon_util.unpack("m", tmp_path_factory.mktemp("ck_runs_m"))
    inter = str(tmp / "inter.fq")
    a, b = open(g["r1"], "rb").read().split(b"\n"), open(g["r2"], "rb").read().split(b"\n")
    with open(inter, "wb") as f:
        for i in range(0, len(a) - 3, 4):
            f.write(b"\n".join(a[i:i + 4]) + b"\n" + b"\n".join(b[i:i + 4]) + b"\n")
    return dict(tmp=tmp, se=(["-i", s["fq"]], s["prefix"]), m=g, inter=inter, n=0, cache={})


def _ref(r, inp, prefix, extra):
    key = " ".join(inp + [prefix] + extra)
    if key not in r["cache"]:
        r["n"] += 1
        stem = str(r["tmp"] / ("ref%d" % r["n"]))
        # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
        p = subprocess.run([KMA] + inp + ["-o", stem, "-t_db", prefix, "-t", "1"] + extra, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
        assert p.returncode in (0, 2), p.returncode
        r["cache"][key] = stem
    return r["cache"][key]


def _map(r, inp, prefix, extra, env=None):
    r["n"] += 1
    stem = str(r["tmp"] / ("got%d" % r["n"]))
    e = dict(os.environ)
    e.update(env or {})
    subprocess.run([MAP] + inp + ["-t_db", prefix, "-o", stem] + extra, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=e, timeout=TIMEOUT)
    return stem


def _files(stem):
    return [open(stem + ext, "rb").read() for ext in (".res", ".fsa", ".aln")] + [gzip.open(stem + ".frag.gz", "rb").read()]


def _same(got, ref, rows=500):
    for name, a, b in zip((".res", ".fsa", ".aln", ".frag.gz"), _files(got), _files(ref)):
        assert a == b, name
    assert gzip.open(got + ".frag.gz", "rb").read().count(b"\n") > rows


SE_RUNS = {
    "ck": (["-1t1", "-ck"], None),
    "ex_mode": (["-1t1", "-ck", "-ex_mode"], None),
    "mem_mode": (["-1t1", "-ck", "-mem_mode"], None),
    "proxi07": (["-1t1", "-ck", "-proxi", "0.7"], None),
    "s1dev": (["-1t1", "-ck", "-s1dev"], None),
    "gpus2": (["-1t1", "-ck", "-gpus", "2"], {"KMAHIP_COMM": "shm", "KMAHIP_SHARE_GPU": "1"}),
}


@pytest.mark.parametrize("tag", list(SE_RUNS))
def test_whole_run_single_end(runs, tag):
    extra, env = SE_RUNS[tag]
    inp, prefix = runs["se"]
    ref_extra = [x for x in extra if x not in ("-s1dev", "-gpus", "2")]          # (our own options: the reference's run is the plain one)
    ref = _ref(runs, inp, prefix, ref_extra)
    _same(_map(runs, inp, prefix, extra, env), ref)
    if tag == "ck":
        # the option moves the reference's own files
        assert _files(ref)[3] != _files(_ref(runs, inp, prefix, ["-1t1"]))[3]


def test_whole_run_with_ef_matrix_vcf(runs):
    inp, prefix = runs["se"]
    extra = ["-1t1", "-ck", "-ef", "-matrix", "-vcf"]
    got, ref = _map(runs, inp, prefix, extra), _ref(runs, inp, prefix, extra)
    _same(got, ref)
    keep = lambda raw: [x for x in raw.split(b"\n") if not x.startswith(b"## date\t") and not x.startswith(b"## command\t")]  # noqa: E731
    assert keep(open(got + ".mapstat", "rb").read()) == keep(open(ref + ".mapstat", "rb").read())
    for ext in (".mat.gz", ".vcf.gz"):
        assert gzip.open(got + ext, "rb").read() == gzip.open(ref + ext, "rb").read(), ext


@pytest.mark.parametrize("apm", [["-apm", "p"], ["-apm", "u"], []], ids=["p", "u", "none"])
def test_whole_run_paired(runs, apm):
    g = runs["m"]
    inp, extra = ["-ipe", g["r1"], g["r2"]], ["-1t1", "-ck"] + apm
    ref = _ref(runs, inp, g["prefix"], extra)
    _same(_map(runs, inp, g["prefix"], extra), ref)
    if not apm:
        assert _files(ref)[3] != _files(_ref(runs, inp, g["prefix"], ["-1t1"]))[3]


def test_whole_run_interleaved(runs):
    g = runs["m"]
    inp, extra = ["-int", runs["inter"]], ["-1t1", "-ck"]
    _same(_map(runs, inp, g["prefix"], extra), _ref(runs, inp, g["prefix"], extra))


def test_whole_run_paired_in_the_default_mode(runs):
    g = runs["m"]
    inp, extra = ["-ipe", g["r1"], g["r2"]], ["-ck"]
    _same(_map(runs, inp, g["prefix"], extra), _ref(runs, inp, g["prefix"], extra))


def test_whole_run_with_decontamination(runs):
    g = runs["m"]
    inp, extra = ["-i", g["reads"]], ["-1t1", "-ck", "-deCon"]
    ref = _ref(runs, inp, g["prefix"], extra)
    _same(_map(runs, inp, g["prefix"], extra), ref)
    assert open(ref + ".res", "rb").read() != open(_ref(runs, inp, g["prefix"], ["-1t1", "-ck"]) + ".res", "rb").read()


# ---- taken without effect -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["-Mt1", "1"]], ids=["default_mode", "Mt1"])
def test_option_without_effect_on_single_end_input(runs, extra):
    """single-end input without -1t1 (kma.c:1272: only a -1t1 run gets save_kmers_count) and -Mt1, which scans no k-mers"""
    inp, prefix = runs["se"]
    with_ck, without = _map(runs, inp, prefix, extra + ["-ck"]), _map(runs, inp, prefix, extra)
    assert _files(with_ck) == _files(without)
    if not extra:
        _same(with_ck, _ref(runs, inp, prefix, ["-ck"]))


def test_option_without_effect_in_sparse_mode(tmp_path):
    import sparse_util as su
    proxi_util.build_map()
    db = su.unpack_index("se_TG", tmp_path)
    fq = str(tmp_path / "a.fq")
    with open(fq, "wb") as f:
        f.write(gzip.open(su.reads_path("se_TG")[0]).read())
    out = str(tmp_path / "o")
    subprocess.run([MAP, "-i", fq, "-o", out, "-t_db", db, "-Sparse", "-ck"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
    assert open(out + ".spa").read() == su.golden("se_TG", "spa_q")
