"""Sparse mapping on the device (kma_amd.binding.SparseDB, `kmahip_map -Sparse`) against the plain Python restatement of
tests/sparse_util.py -- which test_sparse_oracle.py pins to the reference's own k-mer taps and `.spa` files -- against those `.spa` files
themselves, and, where oracle/_ref/kma is built, against whole runs of the reference. Everything is integers or host doubles: no tolerance."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import proxi_util
import sparse_util as su
from kma_amd import binding, synth

pytestmark = pytest.mark.gpu
CASES = list(su.CASES)
VARIANTS = {"ID99.5": dict(id_t=99.5), "md2": dict(depth_t=2.0), "md15": dict(depth_t=15.0), "e1e-30": dict(evalue=1e-30)}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("sparse_gpu")


def batches(case, max_records):
    """the reads of a case as the host's stage 1 hands them over, max_records at a time"""
    for path in su.reads_path(case):
        with binding.Ingest(path) as ing:
            while True:
                got = ing.next(max_records)
                if got is None:
                    break
                yield got[0]


_open = {}


@pytest.fixture(scope="module")
def counted(tmp):
    """case -> (SparseDB with every read counted in one batch per file, the restatement)"""
    def get(case):
        if case not in _open:
            idx, found, Ntot, _, _ = su.restated(case, tmp)
            sdb = binding.SparseDB(su.unpack_index(case, tmp))
            for b in batches(case, 1 << 20):
                sdb.count(b)
            _open[case] = (sdb, idx, found, Ntot)
        return _open[case]
    yield get
    for sdb, *_ in _open.values():
        sdb.close()
    _open.clear()


def as_dict(keys, cnt):
    nz = np.nonzero(cnt)[0]
    return {int(keys[i]): int(cnt[i]) for i in nz}


@pytest.mark.parametrize("case", CASES)
def test_counts_equal_the_restatement(case, counted):
    sdb, idx, found, Ntot = counted(case)
    assert (sdb.info.kmersize, sdb.info.prefix_len, sdb.info.prefix, sdb.info.n_kmers, sdb.info.DB_size) == (idx.k, idx.prefix_len, idx.prefix, len(idx.lists), idx.DB_size)
    keys, cnt, ntot = sdb.counts()
    assert sorted(keys.tolist()) == sorted(idx.lists)
    assert ntot == Ntot
    assert as_dict(keys, cnt) == dict(found)


@pytest.mark.parametrize("case", ["se_TG", "se_none", "e"])
@pytest.mark.parametrize("size", [1, 7])
def test_batching_does_not_change_the_state(case, size, counted, tmp):
    sdb, idx, found, Ntot = counted(case)
    want = sdb.counts()
    with binding.SparseDB(su.unpack_index(case, tmp)) as other:
        n = 0
        for b in batches(case, size):
            other.count(b)
            n += 1
        assert n > 3
        got = other.counts()
        assert got[2] == want[2] and np.array_equal(got[1], want[1])
        assert [np.array_equal(a, b) for a, b in zip(other.scores()[:2], sdb.scores()[:2])] == [True, True]


@pytest.mark.parametrize("case", CASES)
def test_scores_equal_the_restatement(case, counted):
    sdb, idx, found, Ntot = counted(case)
    st = su.State(idx, found)
    sc, tot, hits = sdb.scores()
    assert np.array_equal(sc, st.Scores) and np.array_equal(tot.astype(np.int64), st.Scores_tot) and hits == tuple(st.hits)


def test_collect_without_the_lds_copies(counted, monkeypatch):
    """the path of a database whose score vectors do not fit the LDS: global adds, the same vectors"""
    sdb, idx, found, Ntot = counted("w")
    sdb.collect()
    want = sdb.scores()
    monkeypatch.setenv("KMAHIP_SPARSE_NO_LDS", "1")
    sdb.collect()
    got = sdb.scores()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("ss", ["q", "c"])
def test_scores_before_and_after_each_withdrawal(ss, counted):
    """the w case: the templates the restatement names, withdrawn one by one on the device"""
    sdb, idx, found, Ntot = counted("w")
    trace = []
    rows = su.rows(idx, found, Ntot, ss=ss, trace=trace)
    assert len(trace) == len(rows) >= 10
    sdb.collect()
    st = su.State(idx, found)
    sc, tot, hits = sdb.scores(working=True)
    assert np.array_equal(sc, st.w_Scores) and np.array_equal(tot.astype(np.int64), st.w_Scores_tot) and hits == tuple(st.w_hits)
    for t, w_sc, w_tot, w_hits in trace:
        sdb.withdraw(t)
        sc, tot, hits = sdb.scores(working=True)
        assert np.array_equal(sc, w_sc), t
        assert np.array_equal(tot.astype(np.int64), w_tot), t
        assert hits == tuple(w_hits), t
    # the scores of the collect are untouched
    sc, tot, hits = sdb.scores()
    assert np.array_equal(sc, st.Scores) and hits == tuple(st.hits)


@pytest.mark.parametrize("ss", ["q", "c", "d"])
@pytest.mark.parametrize("case", CASES)
def test_rows_and_file_equal_the_reference(case, ss, counted, tmp):
    sdb, idx, found, Ntot = counted(case)
    want = su.golden(case, "spa_" + ss)
    rows = sdb.rows(ss=ss)
    assert su.spa_text(idx, rows) == want
    # the integers and the doubles themselves, not only their two decimals (p_value: libm's tgamma there, Python's own gamma here)
    assert [r[:11] for r in rows] == [r[:11] for r in su.rows(idx, found, Ntot, ss=ss)]
    path = str(tmp / ("%s.%s.spa" % (case, ss)))
    sdb.write(path, ss=ss)
    assert open(path).read() == want
    for r in rows:
        assert sdb.template(r[0]) == (idx.names[r[0]].encode(), int(idx.lengths[r[0]]), int(idx.ulengths[r[0]]))


@pytest.mark.parametrize("tag", list(VARIANTS))
@pytest.mark.parametrize("case", ["se_TG", "w"])
def test_gates_change_the_file_like_the_reference(case, tag, counted, tmp):
    """-ID 99.5, -md 2 (which leaves both files as they are, like the reference's), -md 15, -e 1e-30"""
    sdb, idx, found, Ntot = counted(case)
    want = su.golden(case, "spa_" + tag)
    path = str(tmp / ("%s.%s.spa" % (case, tag)))
    sdb.write(path, **VARIANTS[tag])
    assert open(path).read() == want
    assert su.spa_text(idx, sdb.rows(**VARIANTS[tag])) == want
    assert (want == su.golden(case, "spa_q")) == (tag == "md2")


def test_rows_can_be_asked_again_and_after_more_reads(counted, tmp):
    """rows() collects anew each time: asking twice gives the same rows, and reads counted afterwards are in the next answer"""
    case = "e"
    with binding.SparseDB(su.unpack_index(case, tmp)) as sdb:
        bs = list(batches(case, 1 << 20))
        sdb.count(bs[0])
        first = sdb.rows()
        assert sdb.rows() == first
        for b in bs[1:]:
            sdb.count(b)
        assert su.spa_text(su.restated(case, tmp)[0], sdb.rows()) == su.golden(case, "spa_q")


def test_count_on_device_resident_reads(counted, tmp):
    """kmahip_sparse_count_dev: the batch in HBM already (torch tensors), the same state as through the staging copy"""
    import torch
    sdb, idx, found, Ntot = counted("se_TG")
    want = sdb.counts()
    with binding.SparseDB(su.unpack_index("se_TG", tmp)) as other:
        for b in batches("se_TG", 700):
            dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).cuda()
                   for a in (b.seq, b.seq_off, b.length, b.N if len(b.N) else np.zeros(1, np.int32), b.N_off)]
            other.count_dev(*dev)
            other.counts()          # (a copy on the null stream: the kernel is done before the tensors go back to torch)
        got = other.counts()
        assert got[2] == want[2] and np.array_equal(got[1], want[1])


def test_noadd_variant_counts_nothing_but_ntot(counted, tmp):
    """the timing-only variant keeps the walk and the probes: Ntot as ever, no count touched"""
    with binding.SparseDB(su.unpack_index("se_TG", tmp)) as sdb:
        sdb.set_noadd(True)
        sdb.set_timing(True)
        for b in batches("se_TG", 1 << 20):
            sdb.count(b)
        keys, cnt, ntot = sdb.counts()
        assert ntot == counted("se_TG")[3] and not cnt.any()
        ms, launches = sdb.get_timing(0)
        assert launches == 1 and ms > 0


# ---- whole runs of examples/kmahip_map against the reference binary -------------------------------------------------------------
@pytest.fixture(scope="module")
def run_inputs(tmp):
    if not os.path.exists(su.KMA):
        pytest.skip("oracle/_ref/kma not built")
    proxi_util.build_map()
    a, b = str(tmp / "a.fq"), str(tmp / "b.fq")
    with open(a, "wb") as f:
        f.write(gzip.open(su.reads_path("se_TG")[0]).read())
    with open(b, "wb") as f:
        f.write(gzip.open(su.reads_path("w")[0]).read())
    return dict(a=a, b=b, gz=su.reads_path("se_TG")[0], fsa_gz=su.reads_path("e")[1], db=su.unpack_index("se_TG", tmp))


def both(tmp, tag, db, inputs, more):
    """the reference and kmahip_map on one command line -> (reference .spa, ours, our stderr, the files we wrote)"""
    ref_dir, got_dir = tmp / ("ref_" + tag), tmp / ("got_" + tag)
    os.makedirs(ref_dir); os.makedirs(got_dir)
    tail = ["-t_db", db, "-Sparse"] + more
    p = subprocess.run([su.KMA] + inputs + ["-o", str(ref_dir / "o"), "-t", "1"] + tail, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
    assert p.returncode in (0, 2)          # (the reference ORs errno into its exit status, kma.c:1630)
    q = subprocess.run([su.MAP] + inputs + ["-o", str(got_dir / "o")] + tail, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    assert q.returncode == 0, q.stderr
    return open(ref_dir / "o.spa").read(), open(got_dir / "o.spa").read(), q.stderr, sorted(os.listdir(got_dir))


RUNS = {
    "i": (lambda x: ["-i", x["a"]], [], None),
    "i_two_files": (lambda x: ["-i", x["a"], x["b"]], ["-ss", "c"], None),
    "ipe": (lambda x: ["-ipe", x["a"], x["b"]], [], b"Paired end information is not considered in Sparse mode.\n"),
    "int": (lambda x: ["-int", x["b"]], ["-ss", "d"], b"Interleaved information is not considered in Sparse mode.\n"),
    "gz_and_fasta": (lambda x: ["-i", x["gz"], x["fsa_gz"]], [], None),
    "trimming": (lambda x: ["-i", x["a"]], ["-mp", "30", "-ml", "100"], None),
    "one2one_ignored": (lambda x: ["-i", x["a"]], ["-1t1", "-ID", "50", "-e", "0.001"], None),
}


@pytest.mark.parametrize("tag", list(RUNS))
def test_whole_run_equals_reference_binary(tag, run_inputs, tmp):
    inputs, more, line = RUNS[tag]
    ref, got, err, files = both(tmp, tag, run_inputs["db"], inputs(run_inputs), more)
    assert got == ref and len(ref.split("\n")) > 3
    assert files == ["o.spa"]
    assert b"# Total number of matches: " in err
    assert line is None or line in err
    # the plain run is the fixture's; -mp 30 -ml 100 is not a run that happens to equal it
    if tag in ("i", "trimming"):
        assert (ref == su.golden("se_TG", "spa_q")) == (tag == "i")


def test_direct_address_index_written_by_kma_index(run_inputs, tmp):
    """The other .comp.b form than the fixtures': `kma index` starts from a table of 4^10 slots, so k = 10 is the largest k at which
    an index of this size is written direct-addressed (exist[] holds a list offset per possible k-mer, no key arrays); k = 11 is hashed.
    The whole run against it equals the reference's, and the loader finds the k-mers the restatement's reader finds."""
    names, seqs = synth.make_gene_db(12, 3, 500, 1300, 0.2, seed=7)
    fa = str(tmp / "mega.fsa")
    synth.write_fasta(fa, names, seqs)
    sizes = {}
    for k in (10, 11):
        db = str(tmp / ("mega%d" % k))
        subprocess.run([su.KMA, "index", "-i", fa, "-o", db, "-k", str(k), "-Sparse", "TG"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        sizes[k] = struct.unpack_from("<Q", open(db + ".comp.b", "rb").read(52), 20)[0]
    assert sizes[10] == 4 ** 10 and sizes[11] != 4 ** 11
    db = str(tmp / "mega10")
    ref, got, err, files = both(tmp, "mega", db, ["-i", run_inputs["b"]], [])
    assert got == ref and len(ref.split("\n")) > 5 and files == ["o.spa"]
    idx = su.Index(db)
    assert idx.mega
    with binding.SparseDB(db) as sdb:
        assert sorted(sdb.counts()[0].tolist()) == sorted(idx.lists)


def test_value_lists_of_32_bit_ids(counted, tmp):
    """DB_size >= 65535 switches the value lists to 32-bit elements (hashmapkma.c:340-348): the se/TG index rewritten by hand with 70000
    templates, the 69933 new ones without a k-mer. Counts, scores and rows equal the restatement on the rewritten index."""
    src = su.unpack_index("se_TG", tmp)
    old = su.Index(src)
    D = 70000
    p = str(tmp / "wide")
    keys = sorted(old.lists)
    values, vidx = [], []
    for key in keys:
        vidx.append(len(values)); values += old.lists[key]
    size = 1 << len(keys).bit_length()
    with open(p + ".comp.b", "wb") as f:
        f.write(struct.pack("<3I5Q", D, old.mlen, old.prefix_len, old.prefix, size, len(keys), len(values), 0))
        f.write(np.zeros(size, np.uint32).tobytes())                 # exist[]: the reference's bucket directory, not read here
        f.write(np.array(values, np.uint32).tobytes())
        f.write(np.array(keys + [0], np.uint32).tobytes())
        f.write(np.array(vidx, np.uint32).tobytes())
        f.write(struct.pack("<2I", old.k, 0))
    pad = np.ones(D - old.DB_size, np.uint32)
    with open(p + ".length.b", "wb") as f:
        f.write(struct.pack("<I", D))
        for arr in (old.lengths, old.lengths, old.ulengths):
            f.write(np.concatenate([arr.astype(np.uint32), pad]).tobytes())
    with open(p + ".name", "w") as f:
        f.write("".join(n + "\n" for n in old.names[1:]) + "".join("t%d\n" % i for i in range(old.DB_size, D)))
    idx = su.Index(p)
    assert idx.DB_size == D and idx.lists == old.lists
    _, _, found, Ntot = counted("se_TG")
    with binding.SparseDB(p) as sdb:
        assert sdb.info.values_u16 == 0
        for b in batches("se_TG", 1 << 20):
            sdb.count(b)
        keys_d, cnt, ntot = sdb.counts()
        assert ntot == Ntot and as_dict(keys_d, cnt) == dict(found)
        st = su.State(idx, found)
        sc, tot, hits = sdb.scores()
        assert np.array_equal(sc, st.Scores) and np.array_equal(tot.astype(np.int64), st.Scores_tot)
        assert su.spa_text(idx, sdb.rows(ss="c")) == su.golden("se_TG", "spa_c")
