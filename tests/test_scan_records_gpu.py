"""Stage 2's record route (scan_prefilter_kernel hands every plain live strand item -- no N, at most 192 bases, not -ex_mode -- to
the first tier as a self-contained 64-byte record, KMAHIP_SCAN_REC unset) against the bare list (KMAHIP_SCAN_REC=0): rc_flag, flag,
T_off, T (paired: the record arrays) of every read set must equal the oracle under both settings, with the kernels that count
(stats launch) and with those that do not.

The read sets are the places where a record can go wrong: read lengths at the borders of the record's words, of the pass and of
the route itself, N's, groups that are not full, both strands of one read live, record items that overflow to the later tiers
(which read them again as bare items), pairs, and a record buffer that is too small. Every test asserts from
KmaHipDB.get_scan_routes() that its items took the route it is about, and on the oracle that its reads find a template at all."""
import numpy as np
import pytest

from kma_amd import formats, synth

pytestmark = pytest.mark.gpu

K = 16
SG = 8            # items of one scan workgroup (scan.hip: STHREADS / 16)
REC_MAX = 192     # longest read that gets a record ((SW - 1) * 32)
LENGTHS = (16, 17, 31, 32, 33, 63, 64, 65, 96, 128, 150, 151, 152, 160, 161, 191, 192, 193, 200, 320)


# ---- databases -----------------------------------------------------------------------------------------------------------------
def _make_db36():
    """36 templates of 400-700 bases in 12 families, and a 37th that holds its own reverse complement"""
    names, seqs = synth.make_gene_db(n_families=12, variants=3, len_lo=400, len_hi=700, max_div=0.03, seed=606)
    x = np.random.default_rng(607).integers(0, 4, 220, dtype=np.uint8)
    return names + ["palin"], list(seqs) + [np.concatenate([x, synth.revcomp_codes(x)])]


def _make_red(variants):
    return synth.make_gene_db(n_families=6, variants=variants, len_lo=500, len_hi=900, max_div=0.03, seed=99)


# ---- read sets (lists of uint8 code arrays, 4 = N) -----------------------------------------------------------------------------
def _reads(seqs, n, L, seed, sub_rate=0.01, random_frac=0.0):
    r, *_ = synth.make_reads([s for s in seqs if len(s) >= L], n, read_len=L, sub_rate=sub_rate, random_frac=random_frac, seed=seed)
    return [x.copy() for x in r]


def _with_N(reads, rng, how_many):
    for r in reads:
        r[rng.choice(len(r), size=how_many, replace=False)] = 4
    return reads


def _shuffle(reads, seed):
    return [reads[i] for i in np.random.default_rng(seed).permutation(len(reads))]


def set_lengths(seqs):
    reads = []
    for j, L in enumerate(LENGTHS):
        reads += _reads(seqs[:36], 24, L, seed=100 + j, sub_rate=0.006)
    return _shuffle(reads, 1)


def set_Ns(seqs):
    rng = np.random.default_rng(2)
    clean = _reads(seqs[:36], 131, 150, seed=21)
    one = _with_N(_reads(seqs[:36], 68, 150, seed=22), rng, 1)
    several = _with_N(_reads(seqs[:36], 61, 150, seed=23), rng, 4)
    return _shuffle(clean + one + several, 3)


def set_eligible(seqs):
    return _shuffle(_reads(seqs[:36], 150, 150, seed=31) + _reads(seqs[:36], 50, 77, seed=32), 4)


def set_ineligible(seqs):
    rng = np.random.default_rng(5)
    return _shuffle(_reads(seqs[:36], 60, 200, seed=41) + _reads(seqs[:36], 40, 320, seed=42) + _with_N(_reads(seqs[:36], 60, 150, seed=43), rng, 2), 6)


def set_forward_exact(seqs, n):
    """n error-free forward reads: their reverse strands hit nothing, so they are n live items"""
    r, *_ = synth.make_reads(seqs[:36], n, read_len=150, sub_rate=0.0, rc_frac=0.0, seed=50 + n)
    return [x.copy() for x in r]


def set_nohit(seqs):
    return [x for x in np.random.default_rng(7).integers(0, 4, (100, 150), dtype=np.uint8)]


def set_palin(seqs):
    """reads of the template that holds its own reverse complement: both strands of every read are live"""
    return _reads([seqs[36]], 40, 150, seed=61, sub_rate=0.004)


def set_overflow(seqs):
    rng = np.random.default_rng(8)
    return _shuffle(_reads(seqs, 260, 150, seed=71, random_frac=0.03) + _with_N(_reads(seqs, 40, 150, seed=72), rng, 1), 9)


def set_pairs(seqs, with_N):
    m1, m2, _ = synth.make_pairs(seqs[:36], 150, read_len=100, ins_lo=200, ins_hi=380, sub_rate=0.01, seed=81)
    rng = np.random.default_rng(10)
    reads = []
    for a, b in zip(m1, m2):
        a, b = a.copy(), b.copy()
        if rng.random() < 0.1:
            a = a[: int(rng.integers(12, 40))]
        if rng.random() < 0.1:
            b = rng.integers(0, 4, len(b), dtype=np.uint8)
        if with_N and rng.random() < 0.4:
            x = a if rng.random() < 0.5 else b
            x[rng.choice(len(x), size=int(rng.integers(1, 4)), replace=False)] = 4
        reads += [a, b]
    return reads


# ---- classes and premises, on the CPU ------------------------------------------------------------------------------------------
def classes(batch):
    """(reads that get a record when a strand of theirs is live, reads that go to the bare list then)"""
    nN = np.diff(batch.N_off)
    live = batch.length >= K
    el = live & (nN == 0) & (batch.length <= REC_MAX)
    return el, live & ~el


def premise(odb, batch, want_el=10, want_in=10):
    """the oracle's result, and how many reads of either class it gives a candidate"""
    e = odb.scan_se(batch)
    has = np.diff(e[2]) > 0
    el, inel = classes(batch)
    n_el, n_in = int((has & el).sum()), int((has & inel).sum())
    assert n_el >= want_el and n_in >= want_in, (n_el, n_in)
    return e, n_el, n_in


def candidates(seqs, reads):
    """per read, the most templates either of its strands shares a k-mer with: what the scan has to hold in a candidate table"""
    index = {}
    for t, s in enumerate(seqs):
        b = bytes(s)
        for i in range(len(b) - K + 1):
            index.setdefault(b[i:i + K], set()).add(t)
    out = []
    for r in reads:
        most = 0
        for x in (r, synth.revcomp_codes(r)):
            b, seen = bytes(x), set()
            for i in range(len(b) - K + 1):
                seen |= index.get(b[i:i + K], set())
            most = max(most, len(seen))
        out.append(most)
    return np.array(out)


# ---- the device ----------------------------------------------------------------------------------------------------------------
def _upload(batch):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(seq=t(np.concatenate([batch.seq, np.zeros(2, np.uint64)]).view(np.int64)), seq_off=t(batch.seq_off), length=t(batch.length),
                N_off=t(batch.N_off), N=t(batch.N if len(batch.N) else np.zeros(1, np.int32)), dev=dev)


def _scan_se(db, d, n):
    import torch
    rc_flag, flag = (torch.zeros(n, dtype=torch.int32, device=d["dev"]) for _ in range(2))
    T_off = torch.zeros(n + 1, dtype=torch.int64, device=d["dev"])
    T = torch.zeros(128 * n + 1024, dtype=torch.int32, device=d["dev"])
    db.scan_se_dev(d["seq"], d["seq_off"], d["length"], d["N"], d["N_off"], rc_flag, flag, T_off, T)
    routes = db.get_scan_routes()
    db.status()
    T_off = T_off.cpu().numpy()
    return (rc_flag.cpu().numpy(), flag.cpu().numpy(), T_off, T.cpu().numpy()[:T_off[n]]), routes


def _scan_pe(db, d, n):
    import torch
    mate, rc, rc_flag, flag = (torch.zeros(n, dtype=torch.int32, device=d["dev"]) for _ in range(4))
    R_off = torch.zeros(n + 1, dtype=torch.int64, device=d["dev"])
    T = torch.zeros(128 * n + 1024, dtype=torch.int32, device=d["dev"])
    db.scan_pe_dev(d["seq"], d["seq_off"], d["length"], d["N"], d["N_off"], mate, rc, rc_flag, flag, R_off, T)
    routes = db.get_scan_routes()
    db.status()
    return tuple(x.cpu().numpy() for x in (mate, rc, rc_flag, flag, R_off, T)), routes


def _expect_pe(odb, batch):
    out = []
    w = lambda i: batch.seq[batch.seq_off[i]:batch.seq_off[i + 1] - 1]
    Nn = lambda i: batch.N[batch.N_off[i]:batch.N_off[i + 1]]
    for j in range(batch.n // 2):
        _, recs = odb.scan_pe(w(2 * j), int(batch.length[2 * j]), Nn(2 * j), w(2 * j + 1), int(batch.length[2 * j + 1]), Nn(2 * j + 1))
        out.append([(r["mate"], r["rc"], r["rc_flag"], r["flag"], r["T"].tolist()) for r in recs])
    return out


def both_routes(db, batch, expect, n_el, n_in, monkeypatch, paired=False, cap=None):
    """The scan under both settings, counting and not, each result against `expect`; the routes' counts against the classes.
    -> (records, bare items) of the default setting"""
    d = _upload(batch)
    n = batch.n
    out = None
    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("KMAHIP_SCAN_REC", raising=False)
        else:
            monkeypatch.setenv("KMAHIP_SCAN_REC", setting)
        if cap is not None:
            monkeypatch.setenv("KMAHIP_SCAN_REC_CAP", str(cap))
        seen = []
        for stats in (False, True):
            db.set_stats(stats)
            try:
                got, (rec, bare) = (_scan_pe if paired else _scan_se)(db, d, n)
                active = int(db.get_stats().active_strands) if stats else None
            finally:
                db.set_stats(False)
            if paired:
                mate, rc, rc_flag, flag, R_off, T = got
                for j, exp in enumerate(expect):
                    have = [(int(mate[x]), int(rc[x]), int(rc_flag[x]), int(flag[x]), T[R_off[x]:R_off[x + 1]].tolist())
                            for x in (2 * j, 2 * j + 1) if mate[x] >= 0]
                    assert have == exp, (setting, stats, j, have, exp)
            else:
                for name, g, e in zip(("rc_flag", "flag", "T_off", "T"), got, expect):
                    assert np.array_equal(g, e), (setting, stats, name)
            if stats:
                assert rec + bare == active, (setting, rec, bare, active)
            seen.append((rec, bare))
        assert seen[0] == seen[1], seen
        rec, bare = seen[0]
        if setting is None:
            assert rec >= n_el and bare >= n_in, (rec, bare, n_el, n_in)
            if cap is not None:
                assert rec <= cap, (rec, cap)
            out = (rec, bare)
        else:
            assert rec == 0 and bare == sum(out), (rec, bare, out)
    return out


@pytest.fixture(scope="module")
def db36(tmp_path_factory):
    import oracle
    from kma_amd import binding
    names, seqs = _make_db36()
    prefix = str(tmp_path_factory.mktemp("scan_rec") / "db")
    formats.write_index(prefix, names, seqs)
    db = binding.KmaHipDB(prefix)
    yield dict(seqs=seqs, odb=oracle.OracleDB(prefix), db=db)
    db.close()


def test_lengths_at_the_borders_of_words_pass_and_route(db36, monkeypatch):
    """16 .. 192 bases go by record (the short ones take strand_win's branch for a window that starts before the read), 193 and
    more by the bare list, in one batch; 152 is the pass border (136 / 137 k-mer starts)"""
    batch = formats.pack_ragged(set_lengths(db36["seqs"]))
    e = db36["odb"].scan_se(batch)
    has = np.diff(e[2]) > 0
    for L in LENGTHS:
        assert int((has & (batch.length == L)).sum()) >= 10, L
    _, n_el, n_in = premise(db36["odb"], batch)
    rec, bare = both_routes(db36["db"], batch, e, n_el, n_in, monkeypatch)
    assert rec > 0 and bare > 0


def test_reads_with_N_between_plain_reads(db36, monkeypatch):
    batch = formats.pack_ragged(set_Ns(db36["seqs"]))
    e, n_el, n_in = premise(db36["odb"], batch)
    nN = np.diff(batch.N_off)
    has = np.diff(e[2]) > 0
    assert int((has & (nN == 1)).sum()) >= 10 and int((has & (nN > 1)).sum()) >= 10
    rec, bare = both_routes(db36["db"], batch, e, n_el, n_in, monkeypatch)
    assert rec % SG and bare % SG, (rec, bare)          # a last group that is not full, on either list


def test_only_plain_reads(db36, monkeypatch):
    batch = formats.pack_ragged(set_eligible(db36["seqs"]))
    e, n_el, _ = premise(db36["odb"], batch, want_in=0)
    rec, bare = both_routes(db36["db"], batch, e, n_el, 0, monkeypatch)
    assert bare == 0


def test_no_plain_read(db36, monkeypatch):
    batch = formats.pack_ragged(set_ineligible(db36["seqs"]))
    e, _, n_in = premise(db36["odb"], batch, want_el=0)
    rec, bare = both_routes(db36["db"], batch, e, 0, n_in, monkeypatch)
    assert rec == 0


@pytest.mark.parametrize("n", [1, SG - 1, SG, SG + 1])
def test_groups_around_one_workgroup(db36, monkeypatch, n):
    batch = formats.pack_ragged(set_forward_exact(db36["seqs"], n))
    e, n_el, _ = premise(db36["odb"], batch, want_el=n, want_in=0)
    rec, bare = both_routes(db36["db"], batch, e, n_el, 0, monkeypatch)
    assert (rec, bare) == (n, 0)


def test_reads_without_a_hit_and_an_empty_batch(db36, monkeypatch):
    batch = formats.pack_ragged(set_nohit(db36["seqs"]))
    e = db36["odb"].scan_se(batch)
    assert int(e[2][-1]) == 0
    assert both_routes(db36["db"], batch, e, 0, 0, monkeypatch) == (0, 0)
    empty = formats.pack_ragged([])
    nothing = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert both_routes(db36["db"], empty, nothing, 0, 0, monkeypatch) == (0, 0)


def test_both_strands_of_a_read_live(db36, monkeypatch):
    batch = formats.pack_ragged(set_palin(db36["seqs"]))
    e, n_el, _ = premise(db36["odb"], batch, want_in=0)
    rec, bare = both_routes(db36["db"], batch, e, n_el, 0, monkeypatch)
    assert (rec, bare) == (2 * batch.n, 0)          # one read, two records


@pytest.mark.parametrize("variants", [40, 90])
def test_record_items_that_overflow(tmp_path, monkeypatch, variants):
    """40 variants of a family do not fit the first tier's 14 candidates, 90 not the second tier's 62 either: the record items
    go on as bare items to the second tier and the dense kernel, which read the read arrays themselves"""
    import oracle
    from kma_amd import binding
    names, seqs = _make_red(variants)
    prefix = str(tmp_path / "red")
    formats.write_index(prefix, names, seqs)
    reads = set_overflow(seqs)
    batch = formats.pack_ragged(reads)
    odb = oracle.OracleDB(prefix)
    e, n_el, n_in = premise(odb, batch)
    assert np.diff(e[2]).max() >= 2
    # the case is what it claims to be: plain reads whose candidates do not fit the first tier's 14 slots (40 variants), nor the
    # second tier's 62 (90 variants)
    wide = candidates(seqs, reads) > (14 if variants == 40 else 62)
    assert int((wide & classes(batch)[0] & (np.diff(e[2]) > 0)).sum()) >= 100
    db = binding.KmaHipDB(prefix)
    try:
        both_routes(db, batch, e, n_el, n_in, monkeypatch)
    finally:
        db.close()


@pytest.mark.parametrize("with_N", [False, True])
def test_pairs(db36, monkeypatch, with_N):
    batch = formats.pack_ragged(set_pairs(db36["seqs"], with_N))
    _, n_el, n_in = premise(db36["odb"], batch, want_in=10 if with_N else 0)
    expect = _expect_pe(db36["odb"], batch)
    assert sum(len(x) > 0 for x in expect) >= 100
    rec, bare = both_routes(db36["db"], batch, expect, n_el, n_in if with_N else 0, monkeypatch, paired=True)
    assert rec > 0 and (bare > 0) == with_N


def test_record_buffer_too_small(db36, monkeypatch):
    """room for 8 records: the workgroup's other records are filed on the bare list, nothing is dropped"""
    batch = formats.pack_ragged(_reads(db36["seqs"][:36], 100, 150, seed=91))
    e, n_el, _ = premise(db36["odb"], batch, want_in=0)
    rec, bare = both_routes(db36["db"], batch, e, 0, 0, monkeypatch, cap=8)
    assert rec == 8 and bare >= n_el - 8
