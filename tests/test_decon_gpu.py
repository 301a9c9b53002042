"""Decontamination (`kma index -deCon`, `kma ... -deCon`) on the device.

The builder's `.decon.comp.b` against the reference's (committed under tests/golden/decon, and the live oracle/_ref/kma where it is built);
stage 2 -- single end, with proximity matching, paired at -apm p / u / f -- against the reference's `-s2 -deCon` taps, which lose records
and reorder one (deConPrint's swap, ankers.c:106-124); whole runs of examples/kmahip_map against the compiled reference, file by file;
and what the library refuses for a database opened with its decon table, entry point by entry point."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import decon_util
import golden_util
import proxi_util
from decon_util import INDEX, KMA, MAP
from kma_amd import binding, formats

pytestmark = pytest.mark.gpu
TIMEOUT = 120


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = decon_util.unpack(name, tmp_path_factory.mktemp("decon_" + name))
        return made[name]
    return get


@pytest.fixture(scope="module")
def m_reads():
    return decon_util.se_reads("m")


@pytest.fixture(scope="module")
def m_db(fx):
    db = binding.KmaHipDB(fx("m")["prefix"], decon=True)
    yield db
    db.close()


@pytest.fixture(scope="module")
def m_scan(m_db, m_reads):
    """stage 2 on fixture m with the decon table, every switch at its default, computed once"""
    return m_db.scan_se(m_reads[1])


# ---- the builder and the loader ----------------------------------------------------------------------------------------------------------
def _hosts(g):
    return [g[k] for k in sorted(g) if k.startswith("host")]


@pytest.fixture(scope="module")
def built(fx, tmp_path_factory):
    """our index of fixtures m and e, with and without -deCon"""
    out = {}
    for name in ("m", "e"):
        g, tmp = fx(name), tmp_path_factory.mktemp("decon_built_" + name)
        binding.index_build(g["db"], str(tmp / "plain"))
        binding.index_build(g["db"], str(tmp / "dec"), decon=_hosts(g))
        out[name] = (str(tmp / "plain"), str(tmp / "dec"))
    return out


@pytest.mark.parametrize("name", ["m", "e"])
def test_builder_decon_mapping_equals_the_references(fx, built, name, tmp_path):
    g = fx(name)
    ours = formats.comp_db_mapping(formats.read_comp_b(built[name][1] + ".decon.comp.b"))
    ref = formats.comp_db_mapping(formats.read_comp_b(g["prefix"] + ".decon.comp.b"))
    assert ours == ref
    D = int(formats.read_comp_b(g["prefix"] + ".decon.comp.b").DB_size)
    assert sum(D in v for v in ours.values()) >= (30 if name == "e" else 1000)
    if os.path.exists(KMA):
        subprocess.run([KMA, "index", "-i", g["db"], "-o", str(tmp_path / "live"), "-deCon"] + _hosts(g), check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=TIMEOUT)
        assert ours == formats.comp_db_mapping(formats.read_comp_b(str(tmp_path / "live") + ".decon.comp.b"))


def test_builder_edges_mark_what_each_record_is_there_for(fx, built):
    """fixture e record by record: exactly k bases mark nothing, k + 1 bases two k-mers, the N splits its record, lower case and IUPAC
    letters count, a reverse complement marks the forward k-mers, the second file is read too"""
    g = fx("e")
    seqs = {}
    for line in gzip.open(os.path.join(g["dir"], "db.fsa.gz"), "rt"):
        if line.startswith(">"):
            cur = line[1:].strip()
        else:
            seqs[cur] = seqs.get(cur, "") + line.strip()
    s = list(seqs.values())
    code = {c: i for i, c in enumerate("ACGT")}
    D = len(s) + 1
    m = formats.comp_db_mapping(formats.read_comp_b(built["e"][1] + ".decon.comp.b"))

    def marked(text):
        """how many of the k-mers of `text` carry the pseudo-template"""
        n = 0
        for i in range(len(text) - 15):
            km = 0
            for c in text[i:i + 16]:
                km = km << 2 | code[c]
            n += D in m[km]
        return n
    assert marked(s[0][10:26]) == 0                                   # exactly k
    assert marked(s[1][20:37]) == 2                                   # k + 1
    assert marked(s[2][30:50]) == 5 and marked(s[2][51:70]) == 4      # an N at 50: 20 and 19 bases either side
    assert marked(s[3][40:70]) == 15                                  # lower case
    assert marked(s[4][50:80]) == 15                                  # IUPAC
    assert marked(s[5][100:130]) == 15                                # reverse complement only
    assert marked(s[6][5:60]) == 40                                   # the second file, its record over two lines


@pytest.mark.parametrize("name", ["m", "e"])
def test_builder_other_files_are_those_of_a_build_without_decon(built, name):
    plain, dec = built[name]
    for ext in (".comp.b", ".seq.b", ".length.b", ".name"):
        assert open(plain + ext, "rb").read() == open(dec + ext, "rb").read(), ext
    assert not os.path.exists(plain + ".decon.comp.b")


def test_loader_opens_the_references_and_our_own_decon_file(fx, built, m_reads, m_scan):
    L = binding.lib()
    db = binding.KmaHipDB(built["m"][1], decon=True)
    try:
        assert L.kmahip_db_is_decon(db.h) == 1
        ours = db.scan_se(m_reads[1])
    finally:
        db.close()
    assert all(np.array_equal(a, b) for a, b in zip(ours, m_scan))
    plain = binding.KmaHipDB(fx("m")["prefix"])
    try:
        assert L.kmahip_db_is_decon(plain.h) == 0
    finally:
        plain.close()


def test_loader_names_the_missing_file(built):
    with pytest.raises(binding.KmaHipError, match=r"kmahip error -2: cannot open .*plain\.decon\.comp\.b"):
        binding.KmaHipDB(built["m"][0], decon=True)


# ---- stage 2, single end -----------------------------------------------------------------------------------------------------------------
def _coverage(plain, decon):
    by = {r["hdr"]: r for r in plain}
    reordered = [r for r in decon if sorted(r["T"].tolist()) == sorted(by[r["hdr"]]["T"].tolist()) and r["T"].tolist() != by[r["hdr"]]["T"].tolist()]
    return len(plain) - len(decon), reordered


def test_scan_se_matches_the_decon_tap(m_reads, m_scan):
    plain, decon = decon_util.tap("m", "s2_plain"), decon_util.tap("m", "s2_decon")
    gone, reordered = _coverage(plain, decon)
    assert gone * 10 >= len(plain) and len(reordered) >= 1
    n = golden_util.check_scan_against_s2(m_reads[0], decon, *m_scan)
    assert n == len(decon)
    # a dropped read is like a read without a hit
    rc_flag, flag, T_off, T = m_scan
    empty = np.diff(T_off) == 0
    assert empty.sum() >= gone and not rc_flag[empty].any() and not flag[empty].any()


@pytest.mark.parametrize("switch", ["KMAHIP_SCAN_DIAG", "KMAHIP_SCAN_REC", "KMAHIP_SCAN_REFINE"])
def test_scan_se_same_with_every_stage2_switch_off(m_db, m_reads, m_scan, monkeypatch, switch):
    monkeypatch.setenv(switch, "0")
    got = m_db.scan_se(m_reads[1])
    assert all(np.array_equal(a, b) for a, b in zip(got, m_scan))
    golden_util.check_scan_against_s2(m_reads[0], decon_util.tap("m", "s2_decon"), *got)


def test_scan_se_same_without_presence_bits(fx, m_reads, m_scan, monkeypatch):
    monkeypatch.setenv("KMAHIP_NO_KBITS", "1")          # (read when a database is opened)
    db = binding.KmaHipDB(fx("m")["prefix"], decon=True)
    try:
        got = db.scan_se(m_reads[1])
    finally:
        db.close()
    assert all(np.array_equal(a, b) for a, b in zip(got, m_scan))


def test_scan_se_wide_lists_take_the_second_tier_and_the_dense_kernel(fx):
    s1, batch = decon_util.se_reads("w")
    db = binding.KmaHipDB(fx("w")["prefix"], decon=True)
    try:
        got = db.scan_se(batch)
        tier2, dense = db.get_scan_overflow()
    finally:
        db.close()
    assert tier2 > 0 and dense > 0, (tier2, dense)
    decon = decon_util.tap("w", "s2_decon")
    assert golden_util.check_scan_against_s2(s1, decon, *got) == len(decon)
    assert 81 not in np.abs(got[3])


def test_scan_se_with_proximity_matching_matches_its_tap(m_db, m_reads):
    got = m_db.scan_se(m_reads[1], min_frac=0.8)
    tap = decon_util.tap("m", "s2_decon_p08")
    assert golden_util.check_scan_against_s2(m_reads[0], tap, *got) == len(tap)
    assert int(m_db.info.DB_size) not in np.abs(got[3])


def test_plain_database_is_unchanged(fx, m_reads):
    db = binding.KmaHipDB(fx("m")["prefix"])
    try:
        got = db.scan_se(m_reads[1])
    finally:
        db.close()
    plain = decon_util.tap("m", "s2_plain")
    assert golden_util.check_scan_against_s2(m_reads[0], plain, *got) == len(plain)


# ---- stage 2, paired ---------------------------------------------------------------------------------------------------------------------
def _codes(r):
    c = formats.unpack_words(r["seq"], r["seqlen"]).copy()
    if len(r["N"]):
        c[r["N"]] = 4
    return c


def _pe_stream(g, db):
    """the S2 stream of the paired fixture rebuilt from kmahip_scan_pe (and kmahip_scan_se for what stage 1 filed singly), as
    tests/test_pe_gpu.py rebuilds it"""
    import oracle
    pairs = [u for u in g["units"] if u[0] == "pe"]
    singles = [u for u in g["units"] if u[0] == "se"]
    pb = formats.pack_ragged([_codes(g["s1"][i]) for u in pairs for i in (u[1], u[2])])
    mate, rc, rc_flag, flag, R_off, T = db.scan_pe(pb)
    pair_res, single_res = {}, {}
    for j, u in enumerate(pairs):
        pair_res[u[1]] = [dict(mate=int(mate[x]), rc=int(rc[x]), rc_flag=int(rc_flag[x]), flag=int(flag[x]), T=T[R_off[x]:R_off[x + 1]])
                          for x in (2 * j, 2 * j + 1) if mate[x] >= 0]
    if singles:
        rf, fl, To, Ts = db.scan_se(formats.pack_ragged([_codes(g["s1"][u[1]]) for u in singles]))
        for j, u in enumerate(singles):
            single_res[u[1]] = (int(rf[j]), int(fl[j]), Ts[To[j]:To[j + 1]]) if To[j + 1] > To[j] else None
    idx = {id(r): i for i, r in enumerate(g["s1"])}
    stream = golden_util.pe_stream_from(g, lambda a, b: pair_res[idx[id(a)]], lambda r: single_res[idx[id(r)]], oracle.rc_packed)
    return stream, T


@pytest.mark.parametrize("apm,tag", [(0, "p"), (1, "u"), (2, "f")])
def test_scan_pe_matches_the_decon_tap(m_db, apm, tag):
    g = decon_util.pe_units("m")
    want = decon_util.gunzip(os.path.join(decon_util.GOLD, "m", "pe_s2_decon_%s.bin.gz" % tag))
    assert want != decon_util.gunzip(os.path.join(decon_util.GOLD, "m", "pe_s2_plain_%s.bin.gz" % tag))
    m_db.params.apm = apm
    try:
        got, T = _pe_stream(g, m_db)
    finally:
        m_db.params.apm = 0
    assert int(m_db.info.DB_size) not in np.abs(T)
    assert got == want


def test_no_single_end_output_holds_the_pseudo_template(m_db, m_scan):
    assert int(m_db.info.DB_size) == 61 and 61 not in np.abs(m_scan[3])


# ---- what the library refuses ------------------------------------------------------------------------------------------------------------
def test_library_refuses_by_name(m_db, m_reads):
    binding.lib()
    L = ctypes.CDLL(binding.LIB_PATH)          # (the same library through function objects of our own: the binding's keep their argument types)
    L.kmahip_last_error.restype = ctypes.c_char_p
    batch = m_reads[1]
    with pytest.raises(binding.KmaHipError, match="kmahip error -1: decontamination .* chain finder"):
        m_db.scan_chain(batch)
    with pytest.raises(binding.KmaHipError, match="kmahip error -1: decontamination .* -Mt1"):
        m_db.run_mt1(batch, 1)
    with pytest.raises(binding.KmaHipError, match="kmahip error -1: decontamination .* chain finder"):
        m_db.set_pe_chain(True)
    for mode, what in (("set_chain", "chain finder"), ("set_mt1", "-Mt1")):
        s = m_db.session()
        try:
            with pytest.raises(binding.KmaHipError, match="kmahip error -1: decontamination .* " + what):
                s.set_chain() if mode == "set_chain" else s.set_mt1(1)
        finally:
            s.close()
    L.kmahip_set_mem_mode.argtypes = [ctypes.c_int]
    assert L.kmahip_set_mem_mode(1) == 0
    try:
        with pytest.raises(binding.KmaHipError, match="kmahip error -1: decontamination .* -mem_mode"):
            m_db.scan_se(batch)
        with pytest.raises(binding.KmaHipError, match="kmahip error -1: decontamination .* -mem_mode"):
            m_db.scan_pe(batch)
    finally:
        assert L.kmahip_set_mem_mode(0) == 0
    # the sharded entry points: refused behind their argument checks, before anything is read
    p = binding.default_params()
    dummy = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 8)()
    for fn, args in (("kmahip_run_se_sharded", (m_db.h, m_db.ws, None, dummy, ctypes.byref(p), dummy, b"x", ms)),
                     ("kmahip_run_pe_sharded", (m_db.h, m_db.ws, None, dummy, ctypes.byref(p), dummy, b"x", ms)),
                     ("kmahip_run_chain_sharded", (m_db.h, m_db.ws, dummy, dummy, ctypes.byref(p), dummy, dummy, b"x", ms)),
                     ("kmahip_run_mt1_sharded", (m_db.h, m_db.ws, dummy, dummy, ctypes.c_int32(1), ctypes.c_int(0), ctypes.byref(p), dummy, b"x", ms))):
        f = getattr(L, fn)
        f.argtypes = None
        f.restype = ctypes.c_int
        assert f(*args) == -1, fn
        assert b"decontamination" in L.kmahip_last_error() and b"sharded" in L.kmahip_last_error(), (fn, L.kmahip_last_error())


# ---- whole runs against the binary -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(fx, tmp_path_factory):
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    proxi_util.build_map()
    g = dict(fx("m"))
    g["tmp"] = tmp_path_factory.mktemp("decon_runs")
    inter = str(g["tmp"] / "inter.fq")
    a, b = open(g["r1"], "rb").read().split(b"\n"), open(g["r2"], "rb").read().split(b"\n")
    with open(inter, "wb") as f:
        for i in range(0, len(a) - 3, 4):
            f.write(b"\n".join(a[i:i + 4]) + b"\n" + b"\n".join(b[i:i + 4]) + b"\n")
    g["inter"] = inter
    g["n"] = 0
    return g


def _ref(g, inp, extra, prefix=None):
    g["n"] += 1
    stem = str(g["tmp"] / ("ref%d" % g["n"]))
    # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
    p = subprocess.run([KMA] + inp + ["-o", stem, "-t_db", prefix or g["prefix"], "-t", "1"] + extra, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
    assert p.returncode in (0, 2), p.returncode
    return stem, p.stdout


def _map(g, inp, extra, env=None, prefix=None):
    g["n"] += 1
    stem = str(g["tmp"] / ("got%d" % g["n"]))
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([MAP] + inp + ["-t_db", prefix or g["prefix"], "-o", stem] + extra, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=e, timeout=TIMEOUT)
    return stem, p.stdout


def _files(stem, more=()):
    out = [open(stem + ext, "rb").read() for ext in (".res", ".fsa", ".aln")] + [gzip.open(stem + ".frag.gz", "rb").read()]
    for ext in more:
        out.append(gzip.open(stem + ext, "rb").read() if ext.endswith(".gz") else open(stem + ext, "rb").read())
    return out


def _same(got, ref, more=()):
    names = (".res", ".fsa", ".aln", ".frag.gz") + tuple(more)
    for name, a, b in zip(names, _files(got, more), _files(ref, more)):
        if name == ".mapstat":          # (its head names the program and the command line)
            a, b = [x for x in a.split(b"\n") if not x.startswith(b"## ")], [x for x in b.split(b"\n") if not x.startswith(b"## ")]
        if name == ".vcf.gz":
            a, b = [x for x in a.split(b"\n") if not x.startswith(b"##")], [x for x in b.split(b"\n") if not x.startswith(b"##")]
        assert a == b, name
    assert gzip.open(got + ".frag.gz", "rb").read().count(b"\n") > 500


@pytest.mark.parametrize("env", [None, {"KMAHIP_MAP_BATCH": "500"}], ids=["one_batch", "batches_of_500"])
def test_whole_run_single_end(runs, env):
    inp, extra = ["-i", runs["reads"]], ["-1t1", "-deCon"]
    ref, _ = _ref(runs, inp, extra)
    _same(_map(runs, inp, extra, env)[0], ref)
    # decontamination changes the result: the reference's own .res without it differs
    assert open(ref + ".res", "rb").read() != open(_ref(runs, inp, ["-1t1"])[0] + ".res", "rb").read()


@pytest.mark.parametrize("apm", [["-apm", "p"], ["-apm", "u"], []], ids=["p", "u", "none"])
def test_whole_run_paired(runs, apm):
    inp, extra = ["-ipe", runs["r1"], runs["r2"]], ["-1t1", "-deCon"] + apm
    _same(_map(runs, inp, extra)[0], _ref(runs, inp, extra)[0])


def test_whole_run_interleaved(runs):
    inp, extra = ["-int", runs["inter"]], ["-1t1", "-deCon"]
    _same(_map(runs, inp, extra)[0], _ref(runs, inp, extra)[0])


def test_whole_run_ill_preset(runs):
    inp, extra = ["-i", runs["reads"]], ["-ill", "-deCon"]
    _same(_map(runs, inp, extra)[0], _ref(runs, inp, extra)[0])


def test_whole_run_with_the_other_options(runs):
    inp, extra = ["-i", runs["reads"]], ["-1t1", "-deCon", "-ca", "-ConClave", "2", "-ef", "-matrix", "-vcf"]
    _same(_map(runs, inp, extra)[0], _ref(runs, inp, extra)[0], more=(".mapstat", ".mat.gz", ".vcf.gz"))


def test_whole_run_sam(runs):
    inp, extra = ["-i", runs["reads"]], ["-1t1", "-deCon", "-sam", "4"]
    (got, gsam), (ref, rsam) = _map(runs, inp, extra), _ref(runs, inp, extra)
    _same(got, ref)
    rows = lambda s: sorted(x for x in s.split(b"\n") if x and not x.startswith(b"@"))
    assert rows(gsam) == rows(rsam) and len(rows(gsam)) > 500


def test_whole_run_on_an_index_of_our_own_builder(runs):
    """kmahip_index -deCon and kma index -deCon: the same files from kmahip_map"""
    ours = str(runs["tmp"] / "ours")
    subprocess.run([INDEX, "-i", runs["db"], "-o", ours, "-deCon", runs["host"]], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
    inp, extra = ["-i", runs["reads"]], ["-1t1", "-deCon"]
    a, b = _map(runs, inp, extra, prefix=ours)[0], _map(runs, inp, extra)[0]
    for x, y in zip(_files(a), _files(b)):
        assert x == y
