"""Stage 2 with the list table: the scan's queue round (and the wavefront-per-item kernels) take the list of a k-mer start from
DevDB::lslots in one gather, not from the probe table's position and vs_id in two. The table is a shortcut to the same number: rc_flag,
flag, T_off and T of every read set must equal the oracle's with the table on, and the run with KMAHIP_SCAN_LTAB=0 bit for bit, in the
plain launch and in the counting one (kmahip_scan_set_stats), whose counts of resolved starts (C_PROBES) and of probe calls (C_HASH)
must not move either.

The index is ltab_util's (tests/test_list_table_gpu.py asserts what its buckets hold); the reads are built by hand, at most 64 a
batch, on both strands. The spills to the second tier and to scan_dense_kernel are forced as tests/test_scan_records_gpu.py forces
them: a family of 40 and of 90 variants."""
import numpy as np
import pytest

import ltab_util as U
from kma_amd import formats, synth
from test_scan_diag_route_gpu import _expect_pe, _scan_pe, _scan_se, _upload, both, strands, sub

pytestmark = pytest.mark.gpu

L = 150
SWITCHES = ("KMAHIP_SCAN_LTAB", "KMAHIP_LTAB_SHIFT", "KMAHIP_LTAB_FLAG", "KMAHIP_SCAN_REC")


def T_OF(f, v):
    return f * U.N_VAR + v


@pytest.fixture(scope="module")
def G(tmp_path_factory):
    import oracle
    from kma_amd import binding
    names, seqs, five = U.make_db()
    prefix = str(tmp_path_factory.mktemp("scan_ltab") / "db")
    formats.write_index(prefix, names, seqs, k=U.K)
    db = binding.KmaHipDB(prefix)
    assert db.list_table_log2() == 13
    yield dict(seqs=seqs, keys=U.kmers(seqs), odb=oracle.OracleDB(prefix), db=db)
    db.close()


def on_and_off(db, odb, reads, monkeypatch, paired=False, want_hits=1, env=()):
    """the batch with the table on and with KMAHIP_SCAN_LTAB=0, plain and counting: the oracle's result four times over, and the
    same counters on and off -> the counters"""
    batch = formats.pack_ragged(reads)
    assert batch.n <= 64
    expect = _expect_pe(odb, batch) if paired else odb.scan_se(batch)
    hits = sum(len(x) > 0 for x in expect) if paired else int((np.diff(expect[2]) > 0).sum())
    assert hits >= want_hits, hits
    d = _upload(batch)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    got, counts = {}, {}
    for ltab in ("1", "0"):
        monkeypatch.setenv("KMAHIP_SCAN_LTAB", ltab)
        for stats in (False, True):
            db.set_stats(stats)
            try:
                got[ltab, stats] = (_scan_pe(db, d, batch.n) if paired else _scan_se(db, d, batch.n))[0]
                if stats:
                    st = db.get_stats()
                    counts[ltab] = (int(st.probes), int(st.hash_probes), int(st.value_elems), int(st.prefilter_probes))
            finally:
                db.set_stats(False)
    for key, g in got.items():
        if paired:
            mate, rc, rc_flag, flag, R_off, T = g
            for j, exp in enumerate(expect):
                have = [(int(mate[x]), int(rc[x]), int(rc_flag[x]), int(flag[x]), T[R_off[x]:R_off[x + 1]].tolist())
                        for x in (2 * j, 2 * j + 1) if mate[x] >= 0]
                assert have == exp, (key, j, have, exp)
        else:
            for name, a, e in zip(("rc_flag", "flag", "T_off", "T"), g, expect):
                assert np.array_equal(a, e), (key, name)
        for a, b in zip(g, got["0", key[1]]):
            assert np.array_equal(a, b), key          # bit for bit what the run without the table gives
    assert counts["1"] == counts["0"], counts
    return counts["1"]


def _read(G, f, v, st=20, n=L):
    return G["seqs"][T_OF(f, v)][st:st + n].copy()


def test_exact_reads(G, monkeypatch):
    reads = [_read(G, i % U.N_FAM, i % U.N_VAR, st=7 * i) for i in range(30)]
    reads += [G["seqs"][-1].copy()]          # `wrap`: 80 bases, its five k-mers share the table's last bucket
    on_and_off(G["db"], G["odb"], strands(reads), monkeypatch, want_hits=len(reads))


def test_substitutions(G, monkeypatch):
    """one and three substitutions at the borders of the read's words, of the first and the last k-mer: every start that covers one
    goes through the queue, and misses"""
    at = (0, 15, 16, 31, 32, L - 16, L - 1)
    reads = []
    for v in (0, 3):
        r = _read(G, 1, v)
        reads += [sub(r, b) for b in at]
        reads += [sub(r, *t) for t in ((0, 15, 16), (16, 31, 32), (31, 32, L - 16), (32, L - 16, L - 1), (0, 31, L - 1), (15, 16, L - 1), (0, 16, 32))]
    probes, hash_probes, _, _ = on_and_off(G["db"], G["odb"], both(reads), monkeypatch, want_hits=2 * len(reads))
    assert hash_probes >= 2 * len(reads)          # the premise: every read left the queue a start (at least the one at its own end)


def test_reads_of_another_variant(G, monkeypatch):
    """error-free reads of the higher variants: the first stride k-mer is shared with a lower one, on whose diagonal the starts at
    the variant's own bases are dirty -- they are queued and HIT"""
    reads = [_read(G, f, v, st=st) for f in range(U.N_FAM) for v in (2, 3, 4) for st in (0, 60, 140)]
    on_and_off(G["db"], G["odb"], strands(reads), monkeypatch, want_hits=len(reads))


def test_indels(G, monkeypatch):
    reads = []
    for i, at in enumerate((20, 40, 75, 100, 130)):
        r = _read(G, i, 0, n=L + 1)
        reads += [np.delete(r, at)[:L], np.insert(r, at, (r[at] + 1) & 3)[:L], np.delete(r, [at, at + 1, at + 2])[:L]]
    on_and_off(G["db"], G["odb"], both(reads), monkeypatch, want_hits=2 * len(reads))


def test_reads_without_a_k_mer_of_the_index(G, monkeypatch):
    rng = np.random.default_rng(21)
    reads = [r for r in rng.integers(0, 4, (40, L), dtype=np.uint8)]
    for r in reads:
        both_strands = np.concatenate([U.kmers([r]), U.kmers([synth.revcomp_codes(r)])])
        assert not np.isin(both_strands, G["keys"]).any()
    reads += [_read(G, 2, 1), sub(_read(G, 3, 2), 70)]          # (and two that map, so that the scan runs at all)
    on_and_off(G["db"], G["odb"], reads, monkeypatch, want_hits=2)


def test_reads_with_N_a_long_read_and_no_records(G, monkeypatch):
    """the bare list: reads with N's, one read of 200 bases beside plain ones, and the whole batch with KMAHIP_SCAN_REC=0"""
    rng = np.random.default_rng(22)
    reads = []
    for i in range(40):
        r = sub(_read(G, i % U.N_FAM, i % U.N_VAR, st=3 * i), int(rng.integers(0, L)))
        if i % 2:
            r[rng.choice(L, size=1 + (i % 4), replace=False)] = 4
        reads.append(r)
    reads.append(sub(_read(G, 4, 1, st=50, n=200), 100))
    reads = strands(reads)
    on_and_off(G["db"], G["odb"], reads, monkeypatch, want_hits=38)
    assert G["db"].get_scan_routes()[1] >= 21
    on_and_off(G["db"], G["odb"], reads, monkeypatch, want_hits=38, env=(("KMAHIP_SCAN_REC", "0"),))
    assert G["db"].get_scan_routes()[0] == 0


def test_list_table_at_the_probe_tables_load_and_without_the_flag(G, monkeypatch):
    """KMAHIP_LTAB_FLAG=0 per launch on the default table"""
    reads = [sub(_read(G, i % U.N_FAM, i % U.N_VAR, st=5 * i), 10 + i, 60 + i) for i in range(32)]
    on_and_off(G["db"], G["odb"], strands(reads), monkeypatch, want_hits=32, env=(("KMAHIP_LTAB_FLAG", "0"),))


@pytest.mark.parametrize("variants", [40, 90])
def test_spill_to_the_later_tiers(tmp_path, monkeypatch, variants):
    """40 variants of a family do not fit the first tier's candidates, 90 not the second tier's either: the second tier's queue and
    scan_dense_kernel look their lists up in the table too; with -ck the counting twin of the dense kernel"""
    import oracle
    from kma_amd import binding
    names, seqs = synth.make_gene_db(n_families=6, variants=variants, len_lo=500, len_hi=900, max_div=0.03, seed=99)
    prefix = str(tmp_path / "red")
    formats.write_index(prefix, names, seqs)
    r, *_ = synth.make_reads(seqs, 64, read_len=L, sub_rate=0.01, seed=71)
    reads = [x.copy() for x in r]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    db = binding.KmaHipDB(prefix)
    try:
        assert db.list_table_log2() > 0
        on_and_off(db, oracle.OracleDB(prefix), reads, monkeypatch, want_hits=60)
        tier2, dense = db.get_scan_overflow()
        assert tier2 >= 16 and (dense >= 16 or variants == 40), (tier2, dense)
        batch = formats.pack_ragged(reads)
        ck = {}
        for ltab in ("1", "0"):
            monkeypatch.setenv("KMAHIP_SCAN_LTAB", ltab)
            ck[ltab] = db.scan_se(batch, count_kmers=True, t_cap=1 << 16)
            over = db.get_scan_overflow()
            assert over[0] >= 16 and (over[1] >= 16 or variants == 40), over
        for a, b in zip(ck["1"], ck["0"]):
            assert np.array_equal(a, b)
        assert len(ck["1"][3]) > 0
    finally:
        db.close()


def test_pairs_in_the_all_candidates_mode(G, monkeypatch):
    m1, m2, _ = synth.make_pairs(G["seqs"][:-1], 32, read_len=100, ins_lo=200, ins_hi=300, sub_rate=0.02, seed=82)
    reads = [x.copy() for a, b in zip(m1, m2) for x in (a, b)]
    on_and_off(G["db"], G["odb"], reads, monkeypatch, paired=True, want_hits=26)


def test_queue_counters(G, monkeypatch):
    """the counting launch's two words on the queue: error-free reads of a first variant leave it nothing; one substitution in the
    middle of a 150-base read leaves it the 16 starts that cover it"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    db = G["db"]
    clean = [_read(G, f, 0, st=10 * f) for f in range(U.N_FAM)]
    for reads, per_read in ((clean, 0), ([sub(r, 70) for r in clean], U.K)):
        d = _upload(formats.pack_ragged(reads))
        db.set_stats(True)
        try:
            _scan_se(db, d, len(reads))
            entries, rounds = db.get_scan_queue_counts()
        finally:
            db.set_stats(False)
        assert (entries, rounds) == (per_read * len(reads), 1 if per_read else 0)
