"""ConClave version 2 (`-ConClave 2`, runConClave2 / runConClave2_lc) on the device.

kmahip_conclave2_records on hand-made and on seeded random records, every array exact against the plain Python restatement
(tests/conclave2_util.py, which test_conclave2_oracle.py holds against the reference's own files); whole runs of examples/kmahip_map
against the compiled reference (oracle/_ref/kma -t 1) run live on the same seeded inputs, `.res`, `.fsa`, `.aln` and the inflated
`.frag.gz` byte for byte; the refusal of the sharded runs. The setting is one per process: every test that sets version 2 puts version 1
back in a `finally`."""
import collections
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import conclave2_util as c2
import proxi_util
from kma_amd import binding, formats, synth
from proxi_util import KMA, MAP

pytestmark = pytest.mark.gpu
TIMEOUT = 120
INT_MAX = 0x7fffffff


def _db(tmp, lengths, seed):
    """an index of random templates of the given lengths -> (KmaHipDB, tlen with entry 0)"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, 4, int(n), dtype=np.uint8) for n in lengths]
    prefix = str(tmp / "db")
    formats.write_index(prefix, ["t%d" % i for i in range(len(seqs))], seqs)
    return binding.KmaHipDB(prefix), np.array([0] + [int(n) for n in lengths], np.int32)


def _fraction(seed):
    """rand / INT_MAX of a seed after its minimal-standard step (conclave.c:573-579)"""
    q, m = c2._cdiv(seed, 127773)
    r = c2.i32(16807 * m - 2836 * q)
    return (r + INT_MAX if r <= 0 else r) / INT_MAX


def _seed_with(lo, hi):
    """the first seed whose draw lands in [lo, hi) of the summed unique scores"""
    return next(s for s in range(1, 1 << 22) if lo <= _fraction(s) < hi)


def _arrays(recs):
    """recs: (list of signed templates, score, q_len, q_len2, seed) -> the arguments of conclave2_records / conclave2 but the vectors"""
    n_hits = np.array([len(r[0]) for r in recs], np.int32)
    off = np.concatenate([[0], np.cumsum(n_hits)]).astype(np.int64)
    tmpl = np.array([x for r in recs for x in r[0]] + [0], np.int32)
    # (start / end say which entry was taken: the entry's place in the flat list)
    start = np.arange(len(tmpl), dtype=np.int32) + 1000
    end = start + 5000
    col = lambda k: np.array([r[k] for r in recs], np.int32)
    return n_hits, col(1), col(2), col(3), off, col(4), tmpl, start, end


def _same(got, want):
    for k in ("tmpl", "start", "end", "w_scores", "fragment_counts", "read_counts", "depth"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0][:10])


def _both(db, recs, AS, US, tlen, lc):
    a = _arrays(recs)
    binding.lib().kmahip_set_conclave_lc(int(lc))
    try:
        got = db.conclave2_records(*a, AS, US)
    finally:
        binding.lib().kmahip_set_conclave_lc(0)
    want = c2.conclave2(*a, AS, US, tlen, lc=lc)
    _same(got, want)
    return got, want


def test_hand_made_records(tmp_path):
    """Eight templates of different lengths, forty-odd records; between them every case the four passes tell apart (named where they
    are made below), each reached according to the restatement's own counters and outputs.

    The `-lc` order (runConClave2_lc) is pinned HERE and nowhere else: on the seeded whole-run inputs the reference's files are the same
    with and without -lc under version 2, so no whole run tells the two orders apart. Records L1-L3 list two templates without a unique
    score, so the fourth pass takes the best of the list: L1 a template with the larger score but the smaller score per base against
    one with the reverse (the two orders disagree); L2 equal score per base with different totals; L3 equal totals with a different
    score per base (on these two the orders agree, by different tests)."""
    lengths = [400, 500, 600, 700, 800, 900, 1000, 450]
    db, tlen = _db(tmp_path, lengths, 5)
    try:
        D = len(tlen)
        AS, US = np.zeros(D, np.uint64), np.zeros(D, np.uint64)
        # the vectors are inputs of their own (stage 3a's): free to set. Templates 1-3 carry unique scores, 4-8 none.
        AS[1:] = [5000, 7000, 9000, 500, 1800, 2000, 2000, 900]          # 5: 1800 / 800 = 2.25 per base, 6: 2000 / 900 = 2.22; 7: 2000 / 1000 = 2.0 = 8: 900 / 450
        US[1:] = [3000, 1000, 2000, 0, 0, 0, 0, 0]
        first, last = _seed_with(0.0, 0.02), _seed_with(0.98, 1.0)
        recs = [
            ([], -150, 80, 80, 7),                     # 0  a pair record with an empty list at the very start of the stream: pass 1's carry is 0, not filed
            ([1], 300, 100, 0, 11),                    # 1  one hit
            ([-2], 350, 100, 0, 11),                   # 2  one hit on the reverse strand
            ([1, 2, 3], 400, 120, 0, first),           # 3  a draw that takes the first entry
            ([1, 2, 3], 400, 120, 0, last),            # 4  ... the last
            ([3, 2, 1], 400, 120, 0, first),           # 5  the same list in another order: the draw walks the list in order
            ([3, -2, 1], 400, 120, 0, _seed_with(0.45, 0.5)),      # 6  a reverse-strand template drawn
            ([5, 6], 500, 90, 0, 12345),               # 7  L1: all unique scores 0 -> best of list; the two orders disagree
            ([7, 8], 450, 90, 0, 12345),               # 8  L2: equal score per base, different totals
            ([6, 7], 450, 90, 0, 12345),               # 9  L3: equal totals, different score per base
            ([1, 3], 200, 15, 0, last),                # 10 fifteen bases: no draw (best of list: 3)
            ([1, 3], 200, 16, 0, first),               # 11 sixteen: a draw (the first entry: 1)
            ([], 0, 0, 0, 0),                          # 12 an unused slot
            ([4], 3, 60, 0, 5),                        # 13 template 4's only score in pass 1: below both gates, pass 2 discards it ...
            ([4, 3], 600, 100, 0, 99),                 # 14 ... so of this record's two templates one survives: pass 3 credits template 3
            ([2, 3], -700, 100, 90, first),            # 15 a pair record with a list: two reads, both lengths
            ([], -120, 70, 70, 3),                     # 16 a pair record with an empty list behind a record with one: pass 1 adds to template 2
            ([5, 3, 7, 8], 300, 100, 0, last),         # 17 a draw among templates of which only one has a unique score: whatever the seed, that one
        ]
        # enough further records with one template to carry templates 1-3 and 5-8 over the gates of pass 2
        for t, s in ((1, 400), (2, 450), (3, 500), (5, 700), (6, 800), (7, 900), (8, 400)):
            recs += [([t], s, 110, 0, 17), ([-t], s, 130, 0, 19), ([t], s, 64, 0, 23)]
        assert 35 <= len(recs) <= 45
        plain, want = _both(db, recs, AS, US, tlen, lc=False)
        with_lc, want_lc = _both(db, recs, AS, US, tlen, lc=True)
        cnt = want["counters"]
        assert cnt["empty"] == 2 and cnt["discarded"] >= 1 and cnt["made_unique"] >= 1 and cnt["draw"] >= 7 and cnt["fallback"] >= 4, cnt
        t = plain["tmpl"]
        assert t[0] == 0 and t[16] == 0 and t[12] == 0                      # empty lists and the unused slot: not filed
        assert want["w1"][4] == 0 and want["uniq2"][3] == 2000 + 600        # pass 2 discarded template 4, pass 3 credited 3
        assert want["w1"][2] >= 120 + 350                                   # the carry of record 16 went to the first listed template of record 15
        assert (t[1], t[2]) == (1, -2)
        assert (t[3], t[4], t[5]) == (1, 3, 3)                               # first / last entry; the other order
        assert t[6] == -2 and plain["start"][6] == 1000 + int(_arrays(recs)[4][6]) + 1
        assert (t[10], t[11]) == (3, 1)                                      # 15 bases: best of list; 16: the draw
        assert t[14] == 3 and t[17] == 3
        assert t[15] in (2, 3) and plain["read_counts"][abs(t[15])] >= 2
        # the two orders: L1 differs, L2 and L3 do not
        assert (t[7], with_lc["tmpl"][7]) == (6, 5), (t[7], with_lc["tmpl"][7])
        assert t[8] == with_lc["tmpl"][8] == 7 and t[9] == with_lc["tmpl"][9] == 6
        # uniq_alignment_scores is the caller's: unchanged
        assert US[3] == 2000
    finally:
        db.close()


@pytest.fixture(scope="module")
def random_records(tmp_path_factory):
    """2 000 records over 50 templates, lists of 1 to 80 entries on both strands, a tenth of them pair records (some with an empty list),
    a few unused slots, first sequences from 10 bases on -> (db, tlen, recs, AS, US); the vectors follow from the records"""
    rng = np.random.default_rng(20)
    db, tlen = _db(tmp_path_factory.mktemp("cc2_random"), rng.integers(300, 2000, 50), 21)
    recs = []
    for i in range(2000):
        pair = rng.random() < 0.1
        k = int(rng.integers(1, 81)) if rng.random() < 0.5 else int(rng.integers(1, 6))
        if pair and rng.random() < 0.2:
            k = 0
        if rng.random() < 0.01:
            recs.append(([], 0, 0, 0, 0))
            continue
        lst = [int(t) * (1 if rng.random() < 0.5 else -1) for t in rng.integers(1, 51, k)]
        s = int(rng.integers(20, 300))
        recs.append((lst, -s if pair else s, int(rng.integers(10, 200)), int(rng.integers(16, 200)) if pair else 0, int(rng.integers(0, 1 << 31))))
    a = _arrays(recs)
    AS, US = c2.vectors_from_records(a[0], a[1], a[4], a[6], len(tlen))
    yield db, tlen, recs, AS, US
    db.close()


@pytest.mark.parametrize("lc", [False, True], ids=["plain", "lc"])
def test_random_records(random_records, lc):
    db, tlen, recs, AS, US = random_records
    got, want = _both(db, recs, AS, US, tlen, lc)
    cnt = want["counters"]
    assert cnt["draw"] > 500 and cnt["fallback"] > 10 and cnt["empty"] > 10 and cnt["made_unique"] >= 0, cnt
    assert (got["tmpl"] < 0).sum() > 300 and len(got["tmpl"]) == 2000


# ---- whole runs against the binary -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    proxi_util.build_map()
    made = {}

    def get(key):
        if key in made:
            return made[key]
        tmp = tmp_path_factory.mktemp("cc2_" + key)
        fam, var, db_seed, _, _ = proxi_util.INPUTS["c"]
        if key == "c":
            s = proxi_util.make_input(tmp, "c")
            s["in"] = ["-i", s["fq"]]
        else:
            names, seqs = synth.make_gene_db(fam, var, 500, 1300, 0.04, seed=db_seed)
            s = dict(tmp=tmp, prefix=str(tmp / "db"), runs={})
            formats.write_index(s["prefix"], names, seqs)
            if key == "c400":
                s["fq"] = str(tmp / "reads.fq")
                synth.write_fastq(s["fq"], proxi_util.reads(seqs, 400, np.random.default_rng(7)), lens=None)
                s["in"] = ["-i", s["fq"]]
            else:
                m1, m2, _ = synth.make_pairs(seqs, 3000, read_len=100, seed=3)
                r1, r2 = str(tmp / "r1.fq"), str(tmp / "r2.fq")
                synth.write_fastq(r1, list(m1), prefix="p")
                synth.write_fastq(r2, list(m2), prefix="p")
                s["in"] = ["-ipe", r1, r2]
        made[key] = s
        return s
    return get


def _ref(s, extra):
    key = " ".join(extra)
    if key not in s["runs"]:
        stem = str(s["tmp"] / ("ref%d" % len(s["runs"])))
        # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
        p = subprocess.run([KMA] + s["in"] + ["-o", stem, "-t_db", s["prefix"], "-t", "1"] + extra, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
        assert p.returncode in (0, 2), p.returncode
        s["runs"][key] = stem
    return s["runs"][key]


def _map(s, tag, extra, env=None):
    stem = str(s["tmp"] / ("got_" + tag))
    e = dict(os.environ)
    e.update(env or {})
    subprocess.run([MAP] + s["in"] + ["-t_db", s["prefix"], "-o", stem] + extra, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=e, timeout=TIMEOUT)
    return stem


def _files(stem):
    return tuple(open(stem + ext, "rb").read() for ext in (".res", ".fsa", ".aln")) + (gzip.open(stem + ".frag.gz", "rb").read(),)


def _rows_moved(s, opts, floor):
    """on the reference alone: its version-2 fragment rows differ from its version-1 rows by at least `floor` (a run that silently stayed
    on version 1 cannot pass what follows)"""
    rows = lambda stem: collections.Counter(tuple(x.split(b"\t")[5:7]) for x in _files(stem)[3].split(b"\n") if x)          # (template, header)
    moved = sum((rows(_ref(s, opts + ["-ConClave", "2"])) - rows(_ref(s, opts))).values())
    assert moved >= floor, (moved, floor)


def _check(s, tag, opts, floor, env=None):
    _rows_moved(s, opts, floor)
    g, r = _files(_map(s, tag, opts + ["-ConClave", "2"], env)), _files(_ref(s, opts + ["-ConClave", "2"]))
    for name, a, b in zip((".res", ".fsa", ".aln", ".frag.gz"), g, r):
        assert a == b, name
    assert g[3].count(b"\n") > 100


@pytest.mark.parametrize("env", [{}, {"KMAHIP_MAP_BATCH": "1000"}, {"KMAHIP_MAP_ONE_BATCH": "1"}], ids=["default", "batch1000", "one_call"])
def test_whole_run_1t1(inputs, env):
    """(batches of 1000: the three loops over the batches of the session, the host step between the first and the second; one_call:
    kmahip_run_se on the whole input)"""
    _check(inputs("c"), "1t1" + "".join(env), ["-1t1"], 500, env)


def test_whole_run_default_mode(inputs):
    _check(inputs("c"), "chain", [], 500)


def test_whole_run_mem_mode(inputs):
    _check(inputs("c"), "mem", ["-1t1", "-mem_mode"], 500)


def test_whole_run_ill(inputs):
    _check(inputs("c"), "ill", ["-ill"], 500)


def test_whole_run_with_ef_matrix_vcf(inputs):
    s = inputs("c")
    opts = ["-1t1", "-ef", "-matrix", "-vcf"]
    _check(s, "emv", opts, 500)
    got, ref = str(s["tmp"] / "got_emv"), _ref(s, opts + ["-ConClave", "2"])
    keep = lambda raw: [x for x in raw.split(b"\n") if not x.startswith(b"## date\t") and not x.startswith(b"## command\t")]  # noqa: E731
    assert keep(open(got + ".mapstat", "rb").read()) == keep(open(ref + ".mapstat", "rb").read())
    for ext in (".mat.gz", ".vcf.gz"):
        assert gzip.open(got + ext, "rb").read() == gzip.open(ref + ext, "rb").read(), ext


def test_whole_run_few_reads_pass_2_decides_rows(inputs):
    s = inputs("c400")
    _check(s, "c400", ["-1t1"], 10)
    rows = lambda stem: open(stem + ".res", "rb").read().count(b"\n")
    assert rows(_ref(s, ["-1t1", "-ConClave", "2"])) > rows(_ref(s, ["-1t1"]))


@pytest.mark.parametrize("apm", [[], ["-apm", "p"]], ids=["union", "apm_p"])
def test_whole_run_pairs(inputs, apm):
    _check(inputs("pairs"), "pe" + "".join(apm), ["-1t1"] + apm, 300)


def test_whole_run_pairs_one_call(inputs):
    """(kmahip_run_pe on the whole input instead of the session)"""
    _check(inputs("pairs"), "pe_one", ["-1t1", "-apm", "p"], 300, {"KMAHIP_MAP_ONE_BATCH": "1"})


def test_version_1_is_the_run_without_the_option(inputs):
    s = inputs("c")
    assert _files(_map(s, "v1", ["-1t1", "-ConClave", "1"])) == _files(_map(s, "plain", ["-1t1"])) == _files(_ref(s, ["-1t1"]))


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_setter_takes_1_and_2_only():
    L = binding.lib()
    try:
        assert L.kmahip_set_conclave_version(2) == 0 and L.kmahip_set_conclave_version(1) == 0
        for v in (0, 3, -1):
            assert L.kmahip_set_conclave_version(v) == -1 and b"ConClave version" in L.kmahip_last_error()
    finally:
        binding.set_conclave_version(1)


def test_run_se_keyword_sets_and_restores(tmp_path):
    """KmaHipDB.run_se(conclave=2) against the restatement's view of the same batch: other templates than version 1 gives, and version 1
    again afterwards"""
    names, seqs = synth.make_gene_db(4, 12, 500, 900, 0.04, seed=31)
    prefix = str(tmp_path / "db")
    formats.write_index(prefix, names, seqs)
    batch = formats.pack_ragged(proxi_util.reads(seqs, 1500, np.random.default_rng(4)))
    db = binding.KmaHipDB(prefix)
    try:
        one = db.run_se(batch)
        two = db.run_se(batch, conclave=2)
        again = db.run_se(batch)
        assert binding._conclave_now == 1
        assert np.array_equal(one["tmpl"], again["tmpl"]) and (one["tmpl"] != two["tmpl"]).sum() > 50
        assert np.array_equal(one["tmpl"] != 0, two["tmpl"] != 0) or (two["tmpl"] != 0).sum() > 1000
    finally:
        binding.set_conclave_version(1)
        db.close()


def test_sharded_entry_point_refuses_version_2(tmp_path):
    """kmahip_run_se_sharded on a communicator of one rank: KMAHIP_EINVAL with the reason by name under version 2; served under version 1"""
    L = binding.lib()
    L.kmahip_comm_init.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    L.kmahip_comm_destroy.argtypes = [C.c_void_p]
    L.kmahip_run_se_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p]
    names, seqs = synth.make_gene_db(4, 3, 500, 700, 0.04, seed=11)
    prefix = str(tmp_path / "db")
    formats.write_index(prefix, names, seqs)
    reads = proxi_util.reads(seqs, 64, np.random.default_rng(2))
    batch = formats.pack_ragged(reads)
    seq = np.ascontiguousarray(batch.seq, np.uint64)
    Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
    rnames = [b"r%d" % i for i in range(batch.n)]
    blob = C.create_string_buffer(b"".join(x + b"\0" for x in rnames) + b"\0")
    noff = np.concatenate([[0], np.cumsum([len(x) + 1 for x in rnames])]).astype(np.int64)
    pair = np.zeros(batch.n, np.uint8)
    p = lambda a: a.ctypes.data
    rb = binding.ReadBatchC(binding.Reads(batch.n, p(seq), p(batch.seq_off), p(batch.length), p(Nn), p(batch.N_off), len(seq), len(batch.N), int(batch.length.max())),
                            C.cast(blob, C.c_void_p), p(noff), p(pair), batch.n)
    so = binding.ShardOpts(0.05, 1, 0, 0, 0, 1.0, 0.0, 0.0, 0, 1, 0, 0, 0.0)
    ms = (C.c_double * 8)()
    db = binding.KmaHipDB(prefix)
    comm = C.c_void_p()
    assert L.kmahip_comm_init(0, 1, b"cc2_%d" % os.getpid(), b"shm", C.byref(comm)) == 0, L.kmahip_last_error()
    try:
        par = binding.Params.from_buffer_copy(db.params)
        call = lambda stem: L.kmahip_run_se_sharded(db.h, db.ws, comm, C.addressof(rb), C.addressof(par), C.addressof(so), str(tmp_path / stem).encode(), C.addressof(ms))
        binding.set_conclave_version(2)
        assert call("two") == -1
        msg = L.kmahip_last_error()
        assert b"-ConClave 2" in msg and b"serves the runs of one rank" in msg and b"kmahip_run_se_sharded" in msg, msg
        assert not os.path.exists(str(tmp_path / "two.res"))
        binding.set_conclave_version(1)
        assert call("one") == 0, L.kmahip_last_error()
        assert os.path.getsize(str(tmp_path / "one.res")) > 100
    finally:
        binding.set_conclave_version(1)
        L.kmahip_comm_destroy(comm)
        db.close()
