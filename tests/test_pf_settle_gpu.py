"""The prefilter's settle route (scan_prefilter_kernel, DevDB::span): a record item whose read lies on the template store along its
final diagonal without a mismatch, with need <= npos <= room in the span table there, gets its result from the prefilter and no record.

Every test runs the scan with the route on and with KMAHIP_PF_SETTLE=0, each counting (set_stats) and not, compares rc_flag, flag,
T_off and T with the oracle, and asserts from KmaHipDB.get_scan_settled() that its items took, or did not take, the route. How many
items MUST be settled is worked out on the CPU from the numpy restatement of the table (tests/span_model.py, held to the oracle by
tests/test_span_table.py): a clean read of the FIRST template that holds its k-mers is filed along its own diagonal, so it is settled
exactly when the table says so; a clean read of a later variant is filed along an earlier one's diagonal and repaired once, so it may
be settled, never must."""
import numpy as np
import pytest

import scheme_sets as ss
import span_model
from kma_amd import formats, synth
from test_scan_records_gpu import _expect_pe, _scan_pe, _upload
from test_span_table import make_small_db

pytestmark = pytest.mark.gpu

K = 16
LENGTHS = (K, K + 1, 32, 33, 64, 65, 151, 152, 192, 193)


# ---- the database: families of variants, and hand-made templates for the borders ------------------------------------------------------
def make_db():
    """18 templates in 6 families of 3 variants (300 .. 420 bases); then
    x, y   share 90 bases in their middles (x[100:190] = y[60:150])
    u, v   share everything from a point to their ends (their last 200 bases)
    p, q   q holds the reverse complement of p[60:260]
    a, b   neighbours in the store: reads over the border between them
    the first template (a family's variant 0) and the last (b) are ones that reads lie on"""
    names, seqs = synth.make_gene_db(n_families=6, variants=3, len_lo=300, len_hi=420, max_div=0.03, seed=4242)
    rng = np.random.default_rng(4243)
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    x = rnd(330)
    y = np.concatenate([rnd(60), x[100:190], rnd(120)])
    y[59], y[150] = (x[99] + 1) & 3, (x[190] + 1) & 3
    tail = rnd(200)
    u, v = np.concatenate([rnd(110), tail]), np.concatenate([rnd(75), tail])
    p = rnd(320)
    q = np.concatenate([rnd(40), synth.revcomp_codes(p[60:260]), rnd(55)])
    a, b = rnd(260), rnd(250)
    extra = dict(x=x, y=y, u=u, v=v, p=p, q=q, a=a, b=b)
    return list(names) + list(extra), list(seqs) + list(extra.values())


class Fx:
    def __init__(self, tmp, names, seqs):
        import oracle
        from kma_amd import binding
        self.names, self.seqs = names, seqs
        self.prefix = str(tmp / "db")
        formats.write_index(self.prefix, names, seqs, k=K)
        self.db = binding.KmaHipDB(self.prefix)
        self.odb = oracle.OracleDB(self.prefix)
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
        self.cat = np.concatenate(list(seqs))
        self.table = span_model.span_table(seqs, formats.comp_db_mapping(formats.read_comp_b(self.prefix + ".comp.b")), K)

    def t(self, name):
        return self.names.index(name)

    def pos(self, name, i=0):
        return int(self.off[self.t(name)]) + i

    def read(self, p, L, rc=False):
        """the L bases of the store from position p on (over a template's end when it has to be), or their reverse complement"""
        r = self.cat[p:p + L].copy()
        return synth.revcomp_codes(r) if rc else r

    def says(self, p, L):
        """the table: is a clean read of L bases at p settled?"""
        _, need, room = self.table
        return L <= 192 and bool(span_model.settled(int(need[p]), int(room[p]), L - K + 1))

    def close(self):
        self.db.close()


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = Fx(tmp_path_factory.mktemp("pf_settle"), *make_db())
    yield f
    f.close()


def _scan(db, d, n, min_frac=1.0):
    import torch
    rc_flag, flag = (torch.zeros(n, dtype=torch.int32, device=d["dev"]) for _ in range(2))
    T_off = torch.zeros(n + 1, dtype=torch.int64, device=d["dev"])
    T = torch.zeros(128 * n + 1024, dtype=torch.int32, device=d["dev"])
    db.scan_se_dev(d["seq"], d["seq_off"], d["length"], d["N"], d["N_off"], rc_flag, flag, T_off, T, min_frac=min_frac)
    routes, settled = db.get_scan_routes(), db.get_scan_settled()
    active = int(db.get_stats().active_strands)
    db.status()
    T_off = T_off.cpu().numpy()
    return (rc_flag.cpu().numpy(), flag.cpu().numpy(), T_off, T.cpu().numpy()[:T_off[n]]), routes, settled, active


def both(db, odb, reads, monkeypatch, expect=None, cap=None):
    """The scan with the route on and off, counting and not, each against the oracle. -> (settled with the route on, its routes)"""
    batch = formats.pack_ragged(reads)
    e = expect if expect is not None else odb.scan_se(batch)
    d = _upload(batch)
    out = None
    if cap is not None:
        monkeypatch.setenv("KMAHIP_SCAN_REC_CAP", str(cap))
    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("KMAHIP_PF_SETTLE", raising=False)
        else:
            monkeypatch.setenv("KMAHIP_PF_SETTLE", setting)
        seen = []
        for stats in (False, True):
            db.set_stats(stats)
            try:
                got, (rec, bare), settled, active = _scan(db, d, batch.n)
            finally:
                db.set_stats(False)
            for name, g, x in zip(("rc_flag", "flag", "T_off", "T"), got, e):
                assert np.array_equal(g, x), (setting, stats, name, np.nonzero(g != x)[0][:5] if len(g) == len(x) else (len(g), len(x)))
            if stats:
                assert rec + bare == active, (setting, rec, bare, active)
            assert settled <= rec, (setting, settled, rec)
            seen.append((settled, rec, bare))
        # (under a cap, WHICH items get the record places is the order the prefilter's lanes claimed them in: it may differ from
        # launch to launch, and the settled count with it; the routes' counts may not)
        assert seen[0][1:] == seen[1][1:] and (cap is not None or seen[0] == seen[1]), seen
        if setting is None:
            out = seen[0]
        else:
            assert seen[0][0] == 0 and seen[0][1:] == out[1:], (seen, out)          # the routes' counts do not know about the settling
    monkeypatch.delenv("KMAHIP_PF_SETTLE", raising=False)
    return out[0], out[1:]


# ---- the table on the device ------------------------------------------------------------------------------------------------------------
def _same_table(db, table):
    got = db.test_span_table(len(table[0]))
    assert got is not None
    for name, g, w in zip(("t0", "need", "room"), got, table):
        assert np.array_equal(g, w), (name, np.nonzero(g != w)[0][:8])


def test_device_table_is_the_restatement(fx):
    _same_table(fx.db, fx.table)
    need, room = fx.table[1], fx.table[2]
    assert (need[room > 0] == 255).any() and (need[room > 0] == 1).any() and (room == 255).any() and (room[room > 0] < 20).any()


def test_device_table_small_databases(tmp_path, monkeypatch):
    """the database of tests/test_span_table.py (every entry held to the oracle there), a database of ONE template, and no table at all
    under KMAHIP_SCAN_SPAN=0: the reads are then scanned, none settled"""
    import oracle
    from kma_amd import binding
    for tag, (names, seqs) in (("small", make_small_db()), ("one", (["only"], [np.random.default_rng(5).integers(0, 4, 300, dtype=np.uint8)]))):
        prefix = str(tmp_path / tag)
        formats.write_index(prefix, names, seqs, k=K)
        table = span_model.span_table(seqs, formats.comp_db_mapping(formats.read_comp_b(prefix + ".comp.b")), K)
        db = binding.KmaHipDB(prefix)
        try:
            _same_table(db, table)
            if tag == "one":
                assert (table[1][table[2] > 0] == 1).all()
                reads = [seqs[0][i:i + L] for i, L in ((0, 150), (150, 150), (284, 16), (100, 192))]
                odb = oracle.OracleDB(prefix)
                settled, _ = both(db, odb, reads, monkeypatch)
                assert settled == len(reads)
        finally:
            db.close()
        if tag == "one":
            monkeypatch.setenv("KMAHIP_SCAN_SPAN", "0")
            db = binding.KmaHipDB(prefix)
            monkeypatch.delenv("KMAHIP_SCAN_SPAN")
            try:
                assert db.test_span_table(8) is None
                settled, (rec, _) = both(db, odb, reads, monkeypatch)
                assert settled == 0 and rec == len(reads)
            finally:
                db.close()


# ---- clean reads ------------------------------------------------------------------------------------------------------------------------
def test_clean_reads_on_every_variant_both_strands(fx, monkeypatch):
    reads, must, may = [], 0, 0
    for t in range(18):
        tl = len(fx.seqs[t])
        for j, L in enumerate(LENGTHS):
            for rc in (False, True):
                i = (37 * t + 11 * j + (5 if rc else 0)) % (tl - L + 1)
                p = int(fx.off[t]) + i
                reads.append(fx.read(p, L, rc))
                ok = fx.says(p, L)
                may += ok
                must += ok and t % 3 == 0          # variant 0 comes first in the store: filed along its own diagonal
    settled, (rec, bare) = both(fx.db, fx.odb, reads, monkeypatch)
    assert must >= 50 and must <= settled <= may, (must, settled, may)
    assert bare >= 18 * 2          # the reads of 193 bases are no records


def test_reads_on_the_first_and_the_last_template(fx, monkeypatch):
    first, last = 0, len(fx.seqs) - 1
    reads, must = [], 0
    for t in (first, last):
        tl = len(fx.seqs[t])
        for i, L in ((0, 150), (tl - 150, 150), (0, K), (tl - K, K), (tl - 192, 192)):
            for rc in (False, True):
                reads.append(fx.read(int(fx.off[t]) + i, L, rc))
                must += fx.says(int(fx.off[t]) + i, L)
    assert must >= 12
    settled, _ = both(fx.db, fx.odb, reads, monkeypatch)
    assert settled == must


# ---- the borders of need and room -------------------------------------------------------------------------------------------------------
def test_boundaries_of_need(fx, monkeypatch):
    """x[100:190] is y's too: a read that starts at x[100] needs 76 starts (75 shared ones and one more)"""
    p = fx.pos("x", 100)
    need = int(fx.table[1][p])
    assert need == 190 - 100 - K + 2
    reads = [fx.read(p, n + K - 1) for n in (need - 1, need, need + 1)]
    inside = [fx.read(fx.pos("x", 110), 60), fx.read(fx.pos("u", 120), 150), fx.read(fx.pos("v", 80), 150, rc=True)]          # never settled
    e = fx.odb.scan_se(formats.pack_ragged(reads + inside))
    assert np.diff(e[2]).tolist() == [2, 1, 1, 2, 2, 2]
    settled, _ = both(fx.db, fx.odb, reads + inside, monkeypatch, expect=e)
    assert settled == 2
    # each on its own: which ones were settled
    for r, want in zip(reads + inside, (0, 1, 1, 0, 0, 0)):
        assert both(fx.db, fx.odb, [r], monkeypatch)[0] == want


def test_boundaries_of_room(fx, monkeypatch):
    """a read that ends on a's last base is settled; the one that runs a base into b lies on the store without a mismatch, and is not"""
    end = fx.pos("b")          # = the position behind a's last base
    on_end, over = fx.read(end - 150, 150), fx.read(end - 149, 150)
    assert fx.says(end - 150, 150) and not fx.says(end - 149, 150)
    e = fx.odb.scan_se(formats.pack_ragged([on_end, over]))
    assert e[0][0] == K + 134 and 0 < e[0][1] < K + 134
    for rc in (False, True):
        conv = (lambda r: synth.revcomp_codes(r)) if rc else (lambda r: r)
        assert both(fx.db, fx.odb, [conv(on_end)], monkeypatch)[0] == 1
        assert both(fx.db, fx.odb, [conv(over)], monkeypatch)[0] == 0
    # over the end of the whole store: the last template's last bases and what lies behind them
    last = fx.read(len(fx.cat) - 150, 150)
    assert both(fx.db, fx.odb, [last], monkeypatch)[0] == 1


@pytest.mark.parametrize("where", [0, 31, 32, 63, 64, 149])
def test_one_mismatch_is_not_settled(fx, monkeypatch, where):
    reads = []
    for name in ("a", "p", "x"):
        for rc in (False, True):
            r = fx.read(fx.pos(name, 20), 150)
            r[where] = (r[where] + 1) & 3
            reads.append(synth.revcomp_codes(r) if rc else r)
    settled, (rec, _) = both(fx.db, fx.odb, reads, monkeypatch)
    assert settled == 0 and rec >= len(reads)


def test_repaired_diagonal_is_settled(fx, monkeypatch):
    """clean reads of the families' LAST variants: filed along variant 0's diagonal, which differs in two bases or more for most of
    them; the repair finds their own, and the table there settles them"""
    reads, may = [], 0
    for f in range(6):
        t = 3 * f + 2
        d = np.nonzero(fx.seqs[t] != fx.seqs[3 * f])[0]
        i = next(i for i in range(len(fx.seqs[t]) - 149) if ((d >= i) & (d < i + 150)).sum() >= 2)          # two differences in the window
        reads.append(fx.read(int(fx.off[t]) + i, 150))
        may += fx.says(int(fx.off[t]) + i, 150)
    fx.db.set_stats(True)
    try:
        _scan(fx.db, _upload(formats.pack_ragged(reads)), len(reads))
        replaced = fx.db.get_scan_diag_replaced()
    finally:
        fx.db.set_stats(False)
    settled, _ = both(fx.db, fx.odb, reads, monkeypatch)
    # (a repair may also land on the middle variant's diagonal, one base off: such a read is scanned)
    assert replaced >= 1 and 1 <= settled <= may, (replaced, settled, may)


def test_strand_tie(fx, monkeypatch):
    """p[60:260] forward is q reverse: both strand items of the read are settled, and the read's list is the oracle's merge"""
    reads = [fx.read(fx.pos("p", 80), 150), fx.read(fx.pos("p", 80), 150, rc=True)]
    e = fx.odb.scan_se(formats.pack_ragged(reads))
    assert np.diff(e[2]).tolist() == [2, 2] and (e[0] < 0).all()
    settled, _ = both(fx.db, fx.odb, reads, monkeypatch, expect=e)
    assert settled == 4


def test_template_with_an_N_under_a_clean_read(tmp_path, monkeypatch):
    """v0 carries an N where its sister v1 has a base: the store holds a base in the N's place, so the clean read lies on v0's
    diagonal without a mismatch, and the k-mers over that position are v1's alone. v1 differs from v0 once more, inside the read, so
    the lists before the N already leave v0 alone (need is small): only `room`, which ends where the lists stop naming v0, keeps the
    item out of the route. Found by tests/test_index_gpu.py on a first version whose room ran to the template's end."""
    import oracle
    from kma_amd import binding
    rng = np.random.default_rng(77)
    x = rng.integers(0, 4, 400, dtype=np.uint8)
    v1 = x.copy()
    v1[150] = (v1[150] + 1) & 3
    other = rng.integers(0, 4, 300, dtype=np.uint8)
    txt = lambda s: "".join("ACGT"[b] for b in s)
    v0_txt = txt(x)
    v0_txt = v0_txt[:200] + "N" + v0_txt[201:]
    fa = str(tmp_path / "n.fsa")
    with open(fa, "w") as f:
        f.write(f">v0\n{v0_txt}\n>v1\n{txt(v1)}\n>other\n{txt(other)}\n")
    prefix = str(tmp_path / "n")
    binding.index_build(fa, prefix, k=K)
    # the templates as the index stores them (the N as a base)
    lens = formats.read_lengths(prefix)[1:]
    words = np.fromfile(prefix + ".seq.b", np.uint64)
    seqs, o = [], 0
    for L in lens.tolist():
        seqs.append(formats.unpack_words(words[o:o + ((L + 31) >> 5)], L))
        o += (L >> 5) + 1
    assert [len(s) for s in seqs] == [400, 400, 300] and np.array_equal(seqs[1], v1)
    stored = seqs[0]
    assert np.array_equal(np.delete(stored, 200), np.delete(x, 200))
    table = span_model.span_table(seqs, formats.comp_db_mapping(formats.read_comp_b(prefix + ".comp.b")), K)
    # (whatever base stands for the N: a k-mer over it is v1's, or nobody's)
    assert int(table[1][130]) == 6 and int(table[2][130]) == 185 - 130 and int(table[1][140]) == 1
    db, odb = binding.KmaHipDB(prefix), oracle.OracleDB(prefix)
    try:
        _same_table(db, table)
        reads = [stored[130:280].copy(), synth.revcomp_codes(stored[130:280]), stored[130:184].copy(), stored[140:190].copy()]
        e = odb.scan_se(formats.pack_ragged(reads))
        assert abs(int(e[0][0])) < K + 134          # the read over the N does not have the full score on any template
        settled, (rec, _) = both(db, odb, reads, monkeypatch, expect=e)
        # the two reads over the N are scanned; the two that end before it (39 starts at need 6 / room 55; 35 at need 1 / room 45) are settled
        assert rec == 4 and settled == 2
    finally:
        db.close()


# ---- scoring schemes ----------------------------------------------------------------------------------------------------------------------
def _mixed(fx):
    reads = []
    for t in (0, 1, 2, 9, 10, 11, fx.t("x"), fx.t("a"), fx.t("p")):
        for i, rc in ((10, False), (60, True)):
            reads.append(fx.read(int(fx.off[t]) + i, 150, rc))
            r = fx.read(int(fx.off[t]) + i + 7, 120, rc)
            r[[40, 90]] = (r[[40, 90]] + 2) & 3
            reads.append(r)
    return reads


@pytest.mark.parametrize("scheme,rw,passes", [
    ("gmm1", None, True), ("gmm6", None, True),
    ("mm_is_m", dict(M=1, MM=1, U=-1, W1=-3), False), ("mm_above_m", dict(M=1, MM=2, U=-1, W1=-3), False),
    ("u_positive", dict(M=1, MM=-2, U=1, W1=-3), False), ("w1_positive", dict(M=1, MM=-2, U=-1, W1=1), False)])
def test_scoring_schemes(fx, monkeypatch, scheme, rw, passes):
    """a scheme that passes the sign test (M > 0, MM < M, U <= 0, W1 <= 0) settles and gives the oracle's scores; one that fails it
    settles nothing and gives the oracle's output all the same"""
    reads = _mixed(fx)
    try:
        for target in (fx.db.params.rw, fx.odb.rw):
            if rw is None:
                ss.apply(target, ss.SCHEMES[scheme])
            else:
                target.M, target.MM, target.U, target.W1 = rw["M"], rw["MM"], rw["U"], rw["W1"]
        settled, (rec, _) = both(fx.db, fx.odb, reads, monkeypatch)
    finally:
        for target in (fx.db.params.rw, fx.odb.rw):
            ss.apply(target, ss.SCHEMES["default"])
    assert rec >= len(reads)
    if passes:
        assert settled >= 6
    else:
        assert settled == 0


# ---- the records stay dense ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 40])
def test_record_capacity_with_settled_and_unsettled_items(fx, monkeypatch, cap):
    """room for `cap` records in a workgroup of 60 record items, 30 clean and 30 with one mismatch: `cap` take the record route, the
    others the bare list, nothing is dropped. Which items get the places is the order the lanes claim them in, so only what holds for
    ANY choice is asserted: of any 40 items at least 10 are clean and at least 10 are not, so settled and written records share the
    workgroup's places; of any 8 nothing can be said but settled <= 8."""
    reads = []
    for j in range(60):
        r = fx.read(fx.pos("a", (2 * j) % 160), 100)
        if j % 2:
            r[50] = (r[50] + 1) & 3
        reads.append(r)
    assert sum(fx.says(fx.pos("a", (2 * j) % 160), 100) for j in range(0, 60, 2)) == 30
    settled, (rec, bare) = both(fx.db, fx.odb, reads, monkeypatch, cap=cap)
    assert rec == cap and bare == 60 - cap
    assert max(0, cap - 30) <= settled <= min(cap, 30), (cap, settled)


def test_two_rounds_of_the_tail(fx, monkeypatch):
    """q holds the reverse complement of a stretch of p, so a database of p, q and their reverse complements makes BOTH strands of a
    read live: 230 reads are 460 record items in one prefilter workgroup, whose tail then runs two rounds; two in five carry a mismatch"""
    import oracle
    from kma_amd import binding
    p = fx.seqs[fx.t("p")]
    names, seqs = ["p", "prc"], [p, synth.revcomp_codes(p)]
    reads = []
    for j in range(230):
        r = p[j % 160:j % 160 + 150].copy()
        if j % 5 in (1, 3):
            r[(7 * j) % 150] = (r[(7 * j) % 150] + 1) & 3
        reads.append(r)
    tmp = str(fx.prefix) + "_two"
    formats.write_index(tmp, names, seqs, k=K)
    db, odb = binding.KmaHipDB(tmp), oracle.OracleDB(tmp)
    try:
        settled, (rec, bare) = both(db, odb, reads, monkeypatch)
        assert (rec, bare) == (460, 0)
        assert settled == 2 * sum(1 for j in range(230) if j % 5 not in (1, 3)), settled
    finally:
        db.close()


# ---- the route is off where it must be ----------------------------------------------------------------------------------------------------
def _route_off(db, scan, check, monkeypatch):
    """`scan()` with the route at its default and with KMAHIP_PF_SETTLE=0, counting and not: nothing settled, `check(result)` each time"""
    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("KMAHIP_PF_SETTLE", raising=False)
        else:
            monkeypatch.setenv("KMAHIP_PF_SETTLE", setting)
        for stats in (False, True):
            db.set_stats(stats)
            try:
                got = scan()
                assert db.get_scan_settled() == 0, (setting, stats)
            finally:
                db.set_stats(False)
            check(got)
    monkeypatch.delenv("KMAHIP_PF_SETTLE", raising=False)


def test_route_off_for_pairs(fx, monkeypatch):
    """the all-candidates mode, against the oracle; the same reads single-end are settled"""
    reads = []
    for j in range(40):
        t = (0, 3, fx.t("a"), fx.t("x"))[j % 4]
        reads += [fx.read(int(fx.off[t]) + j, 100), fx.read(int(fx.off[t]) + j + 130, 100, rc=True)]
    batch = formats.pack_ragged(reads)
    d = _upload(batch)
    assert both(fx.db, fx.odb, reads, monkeypatch)[0] >= 40
    expect = _expect_pe(fx.odb, batch)

    def check(got):
        mate, rc, rc_flag, flag, R_off, T = got[0]
        for j, exp in enumerate(expect):
            have = [(int(mate[x]), int(rc[x]), int(rc_flag[x]), int(flag[x]), T[R_off[x]:R_off[x + 1]].tolist()) for x in (2 * j, 2 * j + 1) if mate[x] >= 0]
            assert have == exp, j
    _route_off(fx.db, lambda: _scan_pe(fx.db, d, batch.n), check, monkeypatch)


def test_route_off_for_proxi_and_ck(golden_se, monkeypatch):
    """-proxi 0.9 and -ck on the golden single-end fixture, against the reference's own stage-2 records for those options; the plain
    scan of the same reads, against its records, settles items"""
    import gzip
    import os

    import golden_util
    from kma_amd import binding

    def tap(*path):
        with gzip.open(os.path.join(golden_util.GOLD, *path), "rb") as f:
            return formats.parse_s2(f.read())[0]
    db = binding.KmaHipDB(golden_se["prefix"])
    batch = golden_se["batch"]
    d = _upload(batch)          # (device arrays: a batch that also holds reads beyond 192 bases keeps its records for the others)

    def scan(min_frac=1.0, ck=False):
        db.set_count_kmers(ck)
        try:
            return _scan(db, d, batch.n, min_frac=min_frac)[0]
        finally:
            db.set_count_kmers(False)
    try:
        plain = scan()
        assert db.get_scan_routes()[0] > 500 and db.get_scan_settled() > 0, (db.get_scan_routes(), db.get_scan_settled())
        golden_util.check_scan_against_s2(golden_se["s1"], golden_se["s2"], *plain)
        for want, kw in ((tap("proxi", "s2_p09.bin.gz"), dict(min_frac=0.9)), (tap("ck", "s2_ck.bin.gz"), dict(ck=True))):
            _route_off(db, lambda: scan(**kw), lambda got: golden_util.check_scan_against_s2(golden_se["s1"], want, *got), monkeypatch)
    finally:
        db.close()


def test_route_off_for_a_decon_database(tmp_path, monkeypatch):
    """the decon fixture against the reference's `-deCon` stage-2 records; the same reads on the same templates settle without the table"""
    import decon_util
    import golden_util
    from kma_amd import binding
    g = decon_util.unpack("m", tmp_path)
    s1, batch = decon_util.se_reads("m")
    want = decon_util.tap("m", "s2_decon")
    plain, dec = binding.KmaHipDB(g["prefix"]), binding.KmaHipDB(g["prefix"], decon=True)
    try:
        got = plain.scan_se(batch)
        assert plain.get_scan_settled() > 0
        golden_util.check_scan_against_s2(s1, decon_util.tap("m", "s2_plain"), *got)
        assert dec.test_span_table(8) is not None

        def check(got):
            assert golden_util.check_scan_against_s2(s1, want, *got) == len(want)
        _route_off(dec, lambda: dec.scan_se(batch), check, monkeypatch)
    finally:
        plain.close()
        dec.close()
