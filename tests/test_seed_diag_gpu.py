"""seed_tasks_kernel's diagonal route (one compare per template diagonal with the read in registers, KMAHIP_SEED_DIAG=1, the default)
against the stepwise route (KMAHIP_SEED_DIAG=0): stage 2 + stage 3a of every read set must equal the oracle under both settings.

The read sets are the places where a mask over the whole diagonal can go wrong: read lengths at the borders of its 32-base words and
of the route itself, reads hanging off a template's ends, mismatches at the mask's edges, a second MEM on another diagonal, repeats,
and the views that must stay on the stepwise route. Each test works out from lengths, N counts and the template's place in the store
which route its tasks take (the rule of seed_view_diag), so that none passes on the other route alone."""
import numpy as np
import pytest

from kma_amd import formats, synth

pytestmark = pytest.mark.gpu

K = 16
MAXLEN = 160      # RR_MAXLEN
GPU = True        # False: only the arithmetic of the routes, on the CPU oracle (how the expected counts below were taken)


def _tandem(rng, n):
    """n bases with a 37-base unit four times in the middle: its k-mers are duplicated inside the template"""
    unit = rng.integers(0, 4, 37, dtype=np.uint8)
    rest = n - 4 * 37
    return np.concatenate([rng.integers(0, 4, rest // 2, dtype=np.uint8), unit, unit, unit, unit, rng.integers(0, 4, rest - rest // 2, dtype=np.uint8)])


@pytest.fixture(scope="module")
def dbx(tmp_path_factory):
    """36 templates of 300-600 bases. The first and the last three are fillers of which only the 'store ends' cases draw reads: at
    the ends of the store the route depends on the read's diagonal (_on_diag). Template 2 is 384 bases (a
    multiple of 32), template 3 one more, template 4 holds a tandem repeat."""
    import oracle
    rng = np.random.default_rng(2024)
    lens = [420, 384, 385, 500] + [int(x) for x in rng.integers(300, 601, 29)] + [333, 300, 310]
    seqs = [rng.integers(0, 4, n, dtype=np.uint8) for n in lens]
    seqs[3] = _tandem(rng, 500)
    names = ["t%d" % (i + 1) for i in range(len(seqs))]
    prefix = str(tmp_path_factory.mktemp("seed_diag") / "db")
    formats.write_index(prefix, names, seqs)
    return dict(prefix=prefix, seqs=seqs, odb=oracle.OracleDB(prefix))


def _draw(rng, s, start, L, rc=False):
    """L bases of template s from `start` on (bases off the template are random), optionally reverse complemented"""
    r = rng.integers(0, 4, L, dtype=np.uint8)
    a, b = max(start, 0), min(start + L, len(s))
    r[a - start:b - start] = s[a:b]
    return r, rc


def _sub(r, p):
    r[p] = (r[p] + 1) & 3


def _finish(reads):
    return formats.pack_ragged([synth.revcomp_codes(r) if rc else r for r, rc in reads])


def _store(seqs):
    """word offset of template t (1-based) in the template store and the store's word count, as db.hip lays it out"""
    tl = np.array([0] + [len(s) for s in seqs])
    off = np.zeros(len(tl) + 1, np.int64)
    for t in range(2, len(tl) + 1):
        off[t] = off[t - 1] + (tl[t - 1] >> 5) + 1
    return tl, off, int(off[len(tl)])


def _on_diag(store, t, L, n_N, d=None):
    """the rule of seed_walk_diag / seed_view_diag for one view: a read of 16..160 bases without N's, and the six words from the
    word of template position d on inside the store (which ends in two pad words). d = None: every diagonal the read can have on
    the template must agree (true of all templates but the first and the last), else the caller has to know the read's."""
    tl, off, words = store
    if not (K <= L <= MAXLEN and n_N == 0):
        return False
    ds = (K - L, int(tl[t]) - K) if d is None else (d,)
    ok = [off[t] + (x >> 5) >= 0 and off[t] + (x >> 5) + 5 <= words + 1 for x in ds]
    assert all(ok) or not any(ok), "the route depends on the read's diagonal: pass it"
    return ok[0]


def _routes(seqs, batch, rc_flag, T_off, T, diags=None):
    """(tasks on the diagonal route, tasks on the stepwise route) among the seeded tasks; diags: per read, the template diagonal
    it was drawn on (reads on the first and last template)"""
    store = _store(seqs)
    diag = step = 0
    for i in range(batch.n):
        if rc_flag[i] <= 0:
            continue
        for t in np.abs(T[T_off[i]:T_off[i + 1]]):
            ok = _on_diag(store, int(t), int(batch.length[i]), int(batch.N_off[i + 1] - batch.N_off[i]), None if diags is None else diags[i])
            diag, step = diag + ok, step + (not ok)
    return diag, step


def _routes_pe(seqs, pb, mate, rc_flag, R_off, T):
    """the same for paired records, by seed_tasks_kernel's choice of views: a couple (both mates kept, the candidates on the second
    record) has two views per task, any other record with a decided strand one"""
    store = _store(seqs)
    diag = step = couples = 0
    nN = lambda x: int(pb.N_off[x + 1] - pb.N_off[x])
    for p0 in range(0, pb.n, 2):
        r = p0 + 1
        if mate[p0] >= 0 and mate[r] >= 0 and R_off[p0 + 1] == R_off[p0]:
            views = [(p0 + int(mate[p0 + m]), t) for t in np.abs(T[R_off[r]:R_off[r + 1]]) for m in (0, 1)]
            couples += 1
        else:
            views = [(p0 + int(mate[x]), t) for x in (p0, r) if rc_flag[x] > 0 and mate[x] >= 0 for t in np.abs(T[R_off[x]:R_off[x + 1]])]
        for rd, t in views:
            ok = _on_diag(store, int(t), int(pb.length[rd]), nN(rd))
            diag, step = diag + ok, step + (not ok)
    return diag, step, couples


def _both(dbx, batch, monkeypatch, diags=None):
    """stage 2 + 3a under both settings, each against the oracle; -> (diagonal tasks, stepwise tasks, oracle result)"""
    odb = dbx["odb"]
    e = odb.scan_se(batch)
    o = odb.align_se(batch, *e)
    for setting in ("1", "0") if GPU else ():
        from kma_amd import binding
        monkeypatch.setenv("KMAHIP_SEED_DIAG", setting)
        db = binding.KmaHipDB(dbx["prefix"])
        try:
            (rc_flag, flag, T_off, T), h = db.map_se(batch)
        finally:
            db.close()
        for a, b in zip(e, (rc_flag, flag, T_off, T)):
            assert np.array_equal(a, b)
        assert np.array_equal(o["n_hits"], h["n_hits"]), setting
        assert np.array_equal(o["best_score"], h["best_score"]), setting
        for i in np.nonzero(o["n_hits"] > 0)[0]:
            s, c = int(T_off[i]), int(o["n_hits"][i])
            for key in ("tmpl", "score", "start", "end"):
                assert np.array_equal(o[key][s:s + c], h[key][s:s + c]), (setting, i, key)
    d, s = _routes(dbx["seqs"], batch, e[0], e[2], e[3], diags)
    return d, s, o


INNER = range(1, 33)      # templates (0-based) away from the ends of the store


def test_read_lengths_on_both_strands(dbx, monkeypatch):
    rng = np.random.default_rng(1)
    seqs = dbx["seqs"]
    for lengths, on_diag in (((16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160), True), ((161, 200), False)):
        reads = []
        for L in lengths:
            for n in range(24):
                s = seqs[INNER[int(rng.integers(len(INNER)))]]
                r, rc = _draw(rng, s, int(rng.integers(0, len(s) - L + 1)), L, rc=bool(n & 1))
                if n % 3 == 0 and L > 40:
                    _sub(r, int(rng.integers(L)))
                reads.append((r, rc))
        d, s, o = _both(dbx, _finish(reads), monkeypatch)
        # every read has one seeded task. Reads of 16 and 17 bases are seeded but too short to score a hit: they exercise the
        # kernel at those lengths for faults, not for values
        assert (d, s) == ((len(reads), 0) if on_diag else (0, len(reads))), (lengths, d, s)
        assert (o["n_hits"] > 0).sum() == len(reads) - (48 if on_diag else 0)


def test_reads_hanging_off_template_ends(dbx, monkeypatch):
    """template windows clipped at 0 and at t_len (templates 2 and 3: 384 and 385 bases). At the ends of the store the route is
    the diagonal's: the read hanging off the start of the first template, or lying in the last words of the last one (310 bases:
    diagonals from 224 on), has its six words outside the store and is left to the stepwise route; the other ends are served."""
    rng = np.random.default_rng(2)
    seqs = dbx["seqs"]
    hangs = (1, 2, 7, 15, 16, 17, 31, 32, 33, 40)
    lengths = (100, 128, 150, 160)
    inner = [(t, st) for t in (1, 2, 5, 9) for h in hangs for L in lengths for st in (-h, len(seqs[t]) - L + h)]
    inner_L = [L for t in (1, 2, 5, 9) for h in hangs for L in lengths for _ in (0, 1)]
    served = [(0, len(seqs[0]) - L + h, L) for h in hangs for L in lengths] + [(35, -h, L) for h in hangs for L in lengths] + \
             [(35, len(seqs[35]) - 160 + h, 160) for h in hangs]
    left = [(0, -h, L) for h in hangs for L in lengths] + [(35, len(seqs[35]) - 100 + h, 100) for h in hangs if h >= 15]
    for cases, on_diag in (([(t, st, L) for (t, st), L in zip(inner, inner_L)], True), (served, True), (left, False)):
        reads, diags = [], []
        for t, st, L in cases:
            for rc in (False, True):
                reads.append(_draw(rng, seqs[t], st, L, rc))
                diags.append(st)
        d, s, o = _both(dbx, _finish(reads), monkeypatch, diags)
        assert (d, s) == ((len(reads), 0) if on_diag else (0, len(reads))), (on_diag, d, s)
        assert (o["n_hits"] > 0).sum() == len(reads)


def test_substitutions_at_fixed_positions(dbx, monkeypatch):
    rng = np.random.default_rng(3)
    seqs = dbx["seqs"]
    reads = []
    for L in (150, 96, 160):
        singles = [(p,) for p in (0, 1, 15, 16, 17, L - 17, L - 16, L - 1)]
        doubles = [(p, p + g) for p in (0, 20, 31, 63, L - 40) for g in (1, 15, 16, 17)]
        for ps in singles + doubles:
            for rc in (False, True):
                s = seqs[INNER[int(rng.integers(len(INNER)))]]
                r, _ = _draw(rng, s, int(rng.integers(0, len(s) - L + 1)), L)
                for p in ps:
                    _sub(r, p)
                reads.append((r, rc))
    d, s, o = _both(dbx, _finish(reads), monkeypatch)
    assert (d, s) == (len(reads), 0), (d, s)      # one seeded task per read, all on the diagonal route
    assert (o["n_hits"] > 0).sum() == len(reads) - 2      # by the oracle: two reads of the set score no hit


def test_indels_and_more_errors_than_seeds(dbx, monkeypatch):
    rng = np.random.default_rng(4)
    seqs = dbx["seqs"]
    reads = []
    for n in range(1, 6):
        for at in (20, 47, 64, 75, 110):
            for rc in (False, True):
                s = seqs[INNER[int(rng.integers(len(INNER)))]]
                st = int(rng.integers(0, len(s) - 160))
                r, _ = _draw(rng, s, st, 150)
                reads.append((np.concatenate([r[:at], rng.integers(0, 4, n, dtype=np.uint8), r[at:150 - n]]), rc))      # insertion
                r, _ = _draw(rng, s, st, 150 + n)
                reads.append((np.concatenate([r[:at], r[at + n:]]), rc))                                                # deletion
    for errs in (4, 5, 6):      # MEMs = errors + 1 > SEEDS: handed on
        for n in range(20):
            s = seqs[INNER[int(rng.integers(len(INNER)))]]
            r, _ = _draw(rng, s, int(rng.integers(0, len(s) - 150 + 1)), 150)
            for p in np.linspace(18, 131, errs).astype(int):
                _sub(r, int(p))
            reads.append((r, bool(n & 1)))
    d, s, o = _both(dbx, _finish(reads), monkeypatch)
    assert (d, s) == (len(reads), 0), (d, s)
    assert (o["n_hits"] > 0).sum() == len(reads)


def test_repeats_and_kmers_found_elsewhere(dbx, monkeypatch):
    rng = np.random.default_rng(5)
    seqs = dbx["seqs"]
    reads = []
    s = seqs[3]      # the tandem repeat: duplicated k-mers, the task is handed on
    for st in range(60, 300, 3):
        for L in (80, 150):
            r, _ = _draw(rng, s, st, L)
            if st % 2:
                _sub(r, L // 2)
            reads.append((r, bool(st & 1)))
    for n in range(120):      # 16 read bases replaced by 16 bases from elsewhere in the template: a unique hit on another diagonal
        s = seqs[INNER[4 + n % 20]]
        st = int(rng.integers(0, len(s) - 150 + 1))
        r, _ = _draw(rng, s, st, 150)
        at = int(rng.integers(20, 110))
        src = (st + at + 200 + int(rng.integers(0, 40))) % (len(s) - 16)
        r[at:at + 16] = s[src:src + 16]
        reads.append((r, bool(n & 1)))
    d, s, o = _both(dbx, _finish(reads), monkeypatch)
    assert (d, s) == (len(reads), 0), (d, s)
    assert (o["n_hits"] > 0).sum() == 266      # by the oracle, of 280: the rest, reads inside the repeat, score no hit


def test_reads_with_n_stay_on_the_stepwise_route(dbx, monkeypatch):
    rng = np.random.default_rng(6)
    seqs = dbx["seqs"]
    reads = []
    for n in range(240):
        s = seqs[INNER[int(rng.integers(len(INNER)))]]
        L = (100, 150, 160)[n % 3]
        r, rc = _draw(rng, s, int(rng.integers(0, len(s) - L + 1)), L, rc=bool(n & 1))
        r[(0, L - 1, int(rng.integers(1, L - 1)))[(n // 3) % 3]] = 4
        reads.append((r, rc))
    d, s, o = _both(dbx, _finish(reads), monkeypatch)
    assert (d, s) == (0, len(reads)), (d, s)
    assert (o["n_hits"] > 0).sum() == len(reads)


def test_paired_records(dbx, monkeypatch):
    """2 x 100 nt through scan_pe_dev / align_pe_dev (kmahip_map_pe): seed_tasks_kernel serves couples through the same search, two
    slots per task. Both settings against the oracle's frag_raw lines, and against each other array for array. Every view is 100
    bases without N's on a template away from the ends of the store: all on the diagonal route, two per couple and candidate."""
    import pe_util
    from kma_amd import binding
    seqs = dbx["seqs"]
    m1, m2, _ = synth.make_pairs([seqs[i] for i in INNER], 300, read_len=100, ins_lo=180, ins_hi=300, sub_rate=0.01, seed=11)
    reads = [x for a, b in zip(m1, m2) for x in (a, b)]
    pb = formats.pack_ragged(reads)
    s1 = [dict(seqlen=len(r), seq=pb.seq[pb.seq_off[i]:pb.seq_off[i + 1] - 1], N=np.zeros(0, np.int32), hdr=b"r%d" % i) for i, r in enumerate(reads)]
    g = dict(prefix=dbx["prefix"], s1=s1, units=[("pe", 2 * j, 2 * j + 1) for j in range(len(m1))])
    exp, kinds = pe_util.oracle_pe_lines(g)
    assert kinds[1] > 200
    res = {}
    for setting in ("1", "0"):
        monkeypatch.setenv("KMAHIP_SEED_DIAG", setting)
        db = binding.KmaHipDB(dbx["prefix"])
        try:
            (mate, rc, rc_flag, flag, R_off, T), h = db.map_pe(pb)
        finally:
            db.close()
        got = []
        for j in range(len(m1)):
            r0, r1 = 2 * j, 2 * j + 1
            hdr = lambda x: s1[2 * j + int(mate[x])]["hdr"].decode()
            kind, o = int(h["kind"][j]), int(R_off[r1])
            if kind == 1:
                n = int(h["n_hits"][r1])
                row = (n, int(h["best_score"][r1]), h["start"][o:o + n].tolist(), h["end"][o:o + n].tolist(), h["tmpl"][o:o + n].tolist())
                got += [(hdr(r0),) + row, (hdr(r1),) + row]
            elif kind == 2:
                got += [(hdr(r0), None), (hdr(r1), None)]
            elif kind == 3:
                got.append((hdr(r0), None))
            elif kind == 4:
                got.append((hdr(r1), None))
            else:
                for x in (r0, r1):
                    nh, ox = int(h["n_hits"][x]), int(R_off[x])
                    if mate[x] >= 0 and nh > 0:
                        got.append((hdr(x), nh, int(h["best_score"][x]), h["start"][ox:ox + nh].tolist(), h["end"][ox:ox + nh].tolist(),
                                    h["tmpl"][ox:ox + nh].tolist()))
        assert len(got) == len(exp), setting
        pe_util.compare_lines(exp, got)
        assert int((h["kind"] == 1).sum()) == kinds[1]
        res[setting] = (mate, rc, rc_flag, flag, R_off, T, h)
        d, s, couples = _routes_pe(seqs, pb, mate, rc_flag, R_off, T)
        # every pair is a couple with one candidate: two views each, all of them on the diagonal route
        assert (d, s, couples) == (2 * len(m1), 0, len(m1)), (d, s, couples)
    for a, b in zip(res["1"][:6], res["0"][:6]):
        assert np.array_equal(a, b)
    for key in ("n_hits", "best_score", "flag", "kind", "alignment_scores", "uniq_alignment_scores"):
        assert np.array_equal(res["1"][6][key], res["0"][6][key]), key
