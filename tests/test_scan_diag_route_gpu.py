"""Stage 2 along the prefilter's diagonal: the prefilter counts a record's mismatches against the template store along the diagonal
of its first stride hit and tries ONE other diagonal (KMAHIP_SCAN_REFINE), and a lane of the scan's first tier settles every k-mer
start of its segment that lies on the diagonal from one issue of loads and queues the others. The diagonal is a hint: rc_flag,
flag, T_off and T of every read set must equal the oracle's with the defaults, with KMAHIP_SCAN_REFINE=0 and with
KMAHIP_SCAN_DIAG=0, counting and not.

The index is small and built here: one unrelated template first (it repeats a 16-mer of family 0, so that a repair probe can land
on a worse diagonal), then 6 families x 5 variants of 300-400 bases. The reads are built by hand, at most 64 a case, on both
strands. `DiagModel` restates the prefilter's rule in numpy (first occurrence in the store, one try, keep if fewer mismatches):
the count of replaced diagonals must equal it exactly, and it checks that a case holds the reads it claims to hold."""
import numpy as np
import pytest

import pe_util
from kma_amd import formats, synth

pytestmark = pytest.mark.gpu

K = 16
SG = 8            # items of one scan workgroup (scan.hip: STHREADS / 16)
REC_MAX = 192     # longest read that gets a record
N_FAM, N_VAR = 6, 5
SETTINGS = ((), (("KMAHIP_SCAN_REFINE", "0"),), (("KMAHIP_SCAN_DIAG", "0"),))


# ---- the index -----------------------------------------------------------------------------------------------------------------
def _make_db():
    """-> names, seqs, p: template 0 is unrelated to the families and carries the 16-mer of family 0's variant 2 that ends at
    base p of it, a base where variant 2 differs from variants 0 and 1 (the widest stretch without such a base lies before p)"""
    names, seqs = synth.make_gene_db(n_families=N_FAM, variants=N_VAR, len_lo=300, len_hi=400, max_div=0.04, seed=707)
    v0, v1, v2 = seqs[0], seqs[1], seqs[2]
    alld = np.nonzero(v2 != v0)[0]
    best = (-1, -1)
    for d in alld:
        if 60 <= d < len(v0) - 100 and v1[d] == v0[d]:
            before = alld[alld < d]
            best = max(best, (int(d - (before[-1] if len(before) else 0)), int(d)))
    assert best[0] >= 49          # (the reads of the case start up to 48 bases before p, on variant 0's diagonal)
    p = best[1]
    extra = np.random.default_rng(708).integers(0, 4, 350, dtype=np.uint8)
    extra[100:100 + K] = v2[p - K + 1:p + 1]
    return ["extra"] + names, [extra] + list(seqs), p


def T_OF(f, v):
    return 1 + f * N_VAR + v          # index into seqs


class DiagModel:
    """The prefilter's rule for the diagonal of a record, in numpy"""

    def __init__(self, seqs):
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
        self.total = int(self.off[-1])
        self.cat = np.concatenate(list(seqs) + [np.zeros(256, np.uint8)])          # (the store is zero behind its last base)
        self.first = {}
        for t, s in enumerate(seqs):
            b = bytes(s)
            for i in range(len(b) - K + 1):
                self.first.setdefault(b[i:i + K], int(self.off[t]) + i)

    def template_at(self, g):
        return int(np.searchsorted(self.off, g, side="right") - 1)

    def mismatches(self, s, a0):
        """bases of s that differ from the store along the diagonal that puts base 0 at a0; None: the span leaves the store"""
        nw = (len(s) + 31) >> 5
        if a0 < 0 or ((a0 + 32 * (nw - 1)) >> 5) > (self.total >> 5):
            return None
        return np.nonzero(self.cat[a0:a0 + len(s)] != s)[0]

    def item(self, s):
        """one strand of an N-free read -> None (no record) or what the prefilter does with its diagonal"""
        L = len(s)
        if L < K or L > REC_MAX:
            return None
        a0 = None
        for j in range(0, L - K + 1, K):
            gp = self.first.get(bytes(s[j:j + K]))
            if gp is not None:
                a0 = gp - j
                break
        if a0 is None:
            return None
        out = dict(a0=a0, m=None, probed=False, hit=False, a1=None, m1=None, replaced=False)
        d = self.mismatches(s, a0)
        if d is None:
            return out
        out["m"] = len(d)
        if len(d) < 2:
            return out
        st = min(max(0, int(d[0]) - K + 1), L - K)
        out["probed"] = True
        gp = self.first.get(bytes(s[st:st + K]))
        if gp is None:
            return out
        out["hit"], out["a1"] = True, gp - st
        d1 = self.mismatches(s, gp - st)
        if d1 is not None:
            out["m1"] = len(d1)
            out["replaced"] = len(d1) < len(d)
        return out

    def items(self, reads):
        out = []
        for r in reads:
            if (r == 4).any():
                continue
            out += [x for x in (self.item(r), self.item(synth.revcomp_codes(r))) if x is not None]
        return out


# ---- reads ---------------------------------------------------------------------------------------------------------------------
def sub(r, *pos):
    r = r.copy()
    for p in pos:
        r[p] = (r[p] + 1) & 3
    return r


def strands(reads, flip=0):
    """every other read as its reverse complement"""
    return [synth.revcomp_codes(r).copy() if (i + flip) & 1 else r for i, r in enumerate(reads)]


def both(reads):
    return [x for r in reads for x in (r, synth.revcomp_codes(r).copy())]


# ---- the device ----------------------------------------------------------------------------------------------------------------
def _upload(batch):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(seq=t(np.concatenate([batch.seq, np.zeros(2, np.uint64)]).view(np.int64)), seq_off=t(batch.seq_off), length=t(batch.length),
                N_off=t(batch.N_off), N=t(batch.N if len(batch.N) else np.zeros(1, np.int32)), dev=dev)


def _scan_se(db, d, n, t_cap=None):
    import torch
    rc_flag, flag = (torch.zeros(n, dtype=torch.int32, device=d["dev"]) for _ in range(2))
    T_off = torch.zeros(n + 1, dtype=torch.int64, device=d["dev"])
    T = torch.zeros(t_cap or 128 * n + 1024, dtype=torch.int32, device=d["dev"])
    db.scan_se_dev(d["seq"], d["seq_off"], d["length"], d["N"], d["N_off"], rc_flag, flag, T_off, T)
    replaced = db.get_scan_diag_replaced()
    db.status()
    T_off = T_off.cpu().numpy()
    return (rc_flag.cpu().numpy(), flag.cpu().numpy(), T_off, T.cpu().numpy()[:T_off[n]]), replaced


def _scan_pe(db, d, n):
    import torch
    mate, rc, rc_flag, flag = (torch.zeros(n, dtype=torch.int32, device=d["dev"]) for _ in range(4))
    R_off = torch.zeros(n + 1, dtype=torch.int64, device=d["dev"])
    T = torch.zeros(128 * n + 1024, dtype=torch.int32, device=d["dev"])
    db.scan_pe_dev(d["seq"], d["seq_off"], d["length"], d["N"], d["N_off"], mate, rc, rc_flag, flag, R_off, T)
    replaced = db.get_scan_diag_replaced()
    db.status()
    return tuple(x.cpu().numpy() for x in (mate, rc, rc_flag, flag, R_off, T)), replaced


def _expect_pe(odb, batch):
    out = []
    for j in range(batch.n // 2):
        w = [batch.seq[batch.seq_off[i]:batch.seq_off[i + 1] - 1] for i in (2 * j, 2 * j + 1)]
        N = [batch.N[batch.N_off[i]:batch.N_off[i + 1]] for i in (2 * j, 2 * j + 1)]
        # (the mates as the oracle's other entry points take them: codes -> words and N list, through the helper of the paired tests)
        for x in (0, 1):
            c = pe_util.codes_of(w[x], int(batch.length[2 * j + x]), N[x])
            assert np.array_equal(formats.pack_ragged([c]).seq[:-1], w[x])
        _, recs = odb.scan_pe(w[0], int(batch.length[2 * j]), N[0], w[1], int(batch.length[2 * j + 1]), N[1])
        out.append([(r["mate"], r["rc"], r["rc_flag"], r["flag"], r["T"].tolist()) for r in recs])
    return out


def three_settings(G, reads, monkeypatch, paired=False, want_hits=1, expect=None, batch=None, t_cap=None):
    """The scan with the defaults, with KMAHIP_SCAN_REFINE=0 and with KMAHIP_SCAN_DIAG=0, counting and not: every result against the
    oracle, the count of replaced diagonals against the model. -> the model's items"""
    if batch is None:
        batch = formats.pack_ragged(reads)
    if expect is None:
        expect = _expect_pe(G["odb"], batch) if paired else G["odb"].scan_se(batch)
    if paired:
        assert sum(len(x) > 0 for x in expect) >= want_hits
    else:
        assert int((np.diff(expect[2]) > 0).sum()) >= want_hits
    items = G["model"].items(reads) if reads is not None else None
    d = _upload(batch)
    for setting in SETTINGS:
        for name in ("KMAHIP_SCAN_REFINE", "KMAHIP_SCAN_DIAG"):
            monkeypatch.delenv(name, raising=False)
        for name, value in setting:
            monkeypatch.setenv(name, value)
        for stats in (False, True):
            G["db"].set_stats(stats)
            try:
                got, replaced = (_scan_pe(G["db"], d, batch.n) if paired else _scan_se(G["db"], d, batch.n, t_cap))
            finally:
                G["db"].set_stats(False)
            if paired:
                mate, rc, rc_flag, flag, R_off, T = got
                for j, exp in enumerate(expect):
                    have = [(int(mate[x]), int(rc[x]), int(rc_flag[x]), int(flag[x]), T[R_off[x]:R_off[x + 1]].tolist())
                            for x in (2 * j, 2 * j + 1) if mate[x] >= 0]
                    assert have == exp, (setting, stats, j, have, exp)
            else:
                for name, g, e in zip(("rc_flag", "flag", "T_off", "T"), got, expect):
                    assert np.array_equal(g, e), (setting, stats, name)
            if stats and items is not None:
                want = sum(x["replaced"] for x in items) if not setting else 0
                assert replaced == want, (setting, replaced, want)
    return items


@pytest.fixture(scope="module")
def G(tmp_path_factory):
    import oracle
    from kma_amd import binding
    names, seqs, p = _make_db()
    prefix = str(tmp_path_factory.mktemp("scan_diag") / "db")
    formats.write_index(prefix, names, seqs, k=K)
    db = binding.KmaHipDB(prefix)
    yield dict(seqs=seqs, p=p, odb=oracle.OracleDB(prefix), db=db, model=DiagModel(seqs))
    db.close()


# ---- substitutions at chosen bases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(N_VAR))
def test_substitutions_at_chosen_bases(G, monkeypatch, variant):
    """none, one and two substitutions in a 150-base read of every variant: at the borders of the read's words and of the read, at
    the k-mer starts where a lane's segment of 9 ends (8 | 9, 17 | 18) and at the last base of those starts, two closer than k and
    two exactly 16 and 17 apart (no / one clean start between them)"""
    L = 150
    s = G["seqs"][T_OF(1, variant)]
    r = s[20:20 + L].copy()
    reads = [r]
    reads += [sub(r, b) for b in (0, 15, 16, 31, 32, 63, 64, L - 17, L - 16, L - 1)]
    reads += [sub(r, b) for b in (8, 9, 17, 18, 8 + K - 1, 9 + K - 1, 17 + K - 1, 18 + K - 1)]
    reads += [sub(r, 40, 45), sub(r, 40, 56), sub(r, 40, 57), sub(r, 71, 72), sub(r, 8, 17)]
    items = three_settings(G, strands(reads, flip=variant), monkeypatch, want_hits=len(reads))
    assert len(items) >= len(reads)


# ---- read lengths --------------------------------------------------------------------------------------------------------------
def test_read_lengths(G, monkeypatch):
    """one start, two, a word's border, a record's last length and the first that goes by the bare list"""
    reads = []
    for j, L in enumerate((16, 17, 31, 32, 33, 64, 150, 151, 192, 193)):
        for v in (0, 2, 4):
            s = G["seqs"][T_OF(2 + (j & 1), v)]
            r = s[30 + j:30 + j + L].copy()
            reads += [r, synth.revcomp_codes(sub(r, L // 2) if L >= 64 else r).copy()]
    assert len(reads) <= 64
    items = three_settings(G, reads, monkeypatch, want_hits=len(reads))
    assert len(items) >= len(reads) - 6          # (the 193-base reads have no record)


# ---- the edges of the store ----------------------------------------------------------------------------------------------------
def test_reads_at_the_edges_of_the_store(G, monkeypatch):
    seqs, model = G["seqs"], G["model"]
    first, last = seqs[0], seqs[-1]
    reads = []
    for L in (16, 40, 150, 192):
        reads += [first[:L].copy(), last[len(last) - L:].copy()]
    # the diagonal comes from the second stride k-mer: base 0 of the first template, and one more case inside the store
    reads += [sub(first[:150], 3), sub(last[len(last) - 150:], 5), sub(last[len(last) - 150:], 149), sub(first[:150], 3, 149)]
    reads += [sub(seqs[T_OF(3, 0)][:150], 7)]
    reads = both(reads)
    items = three_settings(G, reads, monkeypatch, want_hits=len(reads))
    assert any(x["a0"] == 0 for x in items)
    at_end = model.mismatches(last[len(last) - 192:], model.total - 192)          # the bounds rule takes the very end of the store
    assert at_end is not None and len(at_end) == 0


# ---- chimeras ------------------------------------------------------------------------------------------------------------------
def test_chimeras_across_a_template_border(G, monkeypatch):
    """the end of one template and the start of its neighbour in the store: the bases agree along ONE diagonal, which crosses the
    k - 1 positions where no k-mer of the index starts"""
    seqs = G["seqs"]
    reads = []
    for t in (T_OF(0, 1), T_OF(2, 3), T_OF(0, 4), T_OF(3, 4), T_OF(4, 4)):          # (the last three: the neighbour is another family)
        a, b = seqs[t], seqs[t + 1]
        for na in (75, 20, 136, 8):
            reads.append(np.concatenate([a[len(a) - na:], b[:150 - na]]))
    reads += [sub(reads[0], 70), sub(reads[8], 80)]
    reads = both(reads)[:64]
    items = three_settings(G, reads, monkeypatch, want_hits=40)
    assert sum(x["m"] == 0 or x["m1"] == 0 for x in items) >= 8          # the whole read on one diagonal, border included


# ---- repair --------------------------------------------------------------------------------------------------------------------
def test_diagonals_that_repair(G, monkeypatch):
    """error-free reads of the higher variants: the first stride k-mer is shared with a lower variant, whose diagonal is filed,
    and the read's own differs from it in two places or more"""
    seqs = G["seqs"]
    reads = []
    for f in range(N_FAM):
        for v in (2, 3, 4):
            s = seqs[T_OF(f, v)]
            for st in (0, 60, len(s) - 150):
                reads.append(s[st:st + 150].copy())
    reads = strands(reads)[:64]
    items = three_settings(G, reads, monkeypatch, want_hits=len(reads))
    repaired = [x for x in items if x["replaced"]]
    assert len(repaired) >= 20 and all(x["m1"] < x["m"] for x in repaired)
    assert sum(x["m1"] == 0 for x in repaired) >= 10


def test_repair_probe_that_misses(G, monkeypatch):
    """two sequencing errors in a read of the FIRST variant: it lies on its own diagonal, and the k-mer that ends at the first
    error is in no template"""
    seqs = G["seqs"]
    reads = []
    for f in range(N_FAM):
        s = seqs[T_OF(f, 0)]
        for st, e1, e2 in ((10, 30, 90), (50, 5, 149), (100, 16, 17), (0, 0, 100), (20, 140, 145)):
            reads.append(sub(s[st:st + 150], e1, e2))
    reads = strands(reads)
    items = three_settings(G, reads, monkeypatch, want_hits=len(reads))
    assert sum(x["probed"] and not x["hit"] for x in items) >= 25
    assert not any(x["replaced"] for x in items)


def test_repair_probe_that_lands_on_the_planted_repeat(G, monkeypatch):
    """reads of family 0's variant 2 over base p: variant 0's diagonal is filed, the first mismatch is at p, and the k-mer that ends
    there occurs first on the unrelated template -- a worse diagonal, which is refused"""
    seqs, p, model = G["seqs"], G["p"], G["model"]
    v2 = seqs[T_OF(0, 2)]
    reads = []
    for before in (16, 20, 31, 32, 40, 48):
        st = p - before
        reads.append(v2[st:st + 150].copy())
    reads = both(reads)
    items = three_settings(G, reads, monkeypatch, want_hits=len(reads))
    planted = [x for x in items if x["hit"] and model.template_at(x["a1"] + 150) == 0 and model.template_at(x["a0"]) != 0]
    assert len(planted) >= 3 and not any(x["replaced"] for x in planted)
    assert all(x["m1"] is None or x["m1"] > x["m"] for x in planted)


# ---- queue overflow ------------------------------------------------------------------------------------------------------------
def test_queue_overflow_keeps_scattered_starts(G, monkeypatch):
    """one group of 8 reads with a substitution every 10th base: no start is on the diagonal but those between two substitutions
    16 apart -- there are none -- so every lane queues its whole segment, the queue of 512 entries overflows and the lanes behind
    keep theirs; with substitutions 20 apart a lane keeps starts that are not neighbours"""
    seqs = G["seqs"]
    reads = []
    for i in range(SG):
        s = seqs[T_OF(i % N_FAM, 0)]
        r = s[5 * i:5 * i + 150].copy()
        step = 10 if i < 5 else 20
        reads.append(sub(r, *range(i % 7, 150, step)))
    reads = strands(reads)
    # some starts must survive for the reads to be live at all: the stride k-mers are all broken at step 10, so a clean k-mer at a
    # stride position is spliced in at the read's end
    for i in range(SG):
        s = seqs[T_OF(i % N_FAM, 0)]
        tail = s[5 * i + 128:5 * i + 150]
        reads[i] = reads[i].copy()
        if i & 1:
            reads[i][:22] = synth.revcomp_codes(tail)
        else:
            reads[i][128:] = tail
    three_settings(G, reads, monkeypatch, want_hits=SG)


# ---- batch sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, SG - 1, SG, SG + 1])
def test_batches_around_one_workgroup(G, monkeypatch, n):
    seqs = G["seqs"]
    reads = [sub(seqs[T_OF(i % N_FAM, (2 * i) % N_VAR)][10 + i:160 + i], 40 + i) for i in range(n)]
    three_settings(G, reads, monkeypatch, want_hits=n)


# ---- N's -----------------------------------------------------------------------------------------------------------------------
def test_reads_with_N_between_plain_reads(G, monkeypatch):
    """the bare variant of the first tier (reads with N's: no diagonal is used) beside the record variant"""
    seqs = G["seqs"]
    rng = np.random.default_rng(11)
    reads = []
    for i in range(48):
        s = seqs[T_OF(i % N_FAM, i % N_VAR)]
        st = int(rng.integers(0, len(s) - 150))
        r = sub(s[st:st + 150], int(rng.integers(0, 150)))
        if i % 3 == 1:
            r[rng.choice(150, size=1 + (i % 4), replace=False)] = 4
        reads.append(r)
    reads = strands(reads)
    items = three_settings(G, reads, monkeypatch, want_hits=44)
    assert len(items) >= 32


# ---- the all-candidates mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_N", [False, True])
def test_pairs(G, monkeypatch, with_N):
    """-apm p: the first tier lists every candidate with its score and its count of hits, which the pairing reads"""
    m1, m2, _ = synth.make_pairs(G["seqs"][1:], 30, read_len=100, ins_lo=200, ins_hi=300, sub_rate=0.01, seed=81)
    rng = np.random.default_rng(12)
    reads = []
    for a, b in zip(m1, m2):
        a, b = a.copy(), b.copy()
        if with_N and rng.random() < 0.4:
            x = a if rng.random() < 0.5 else b
            x[rng.choice(len(x), size=int(rng.integers(1, 4)), replace=False)] = 4
        reads += [a, b]
    three_settings(G, reads, monkeypatch, paired=True, want_hits=25)


# ---- scan_blocks_kernel --------------------------------------------------------------------------------------------------------
def test_T_off_across_the_tiles_of_the_block_scan(G, monkeypatch):
    """3 x 1024 x 256 + 5 reads: the per-block totals cross the tile borders of scan_blocks_kernel. Reads of 16 random bases have no
    hit; every 997th read and the reads around the tile borders are 16-mers of the templates. T_off must be the running sum of the
    per-read counts, which the oracle gives for the reads that can hit."""
    seqs = G["seqs"]
    n = 3 * 1024 * 256 + 5
    rng = np.random.default_rng(13)
    codes = rng.integers(0, 4, (n, K), dtype=np.uint8)
    rows = set(range(0, n, 997))
    for tile in (1, 2, 3):
        rows |= {tile * 1024 * 256 + d for d in (-257, -256, -1, 0, 1, 255, 256)}
    rows |= {n - 1, n - 5, 255, 256}
    rows = np.array(sorted(r for r in rows if 0 <= r < n))
    for x, r in enumerate(rows):
        s = seqs[1 + x % (len(seqs) - 1)]
        st = (7 * x) % (len(s) - K)
        km = s[st:st + K]
        codes[r] = synth.revcomp_codes(km) if x % 3 == 0 else km
    # the reads that can hit: a 16-mer of the index on either strand
    w = (codes.astype(np.uint64) << (np.uint64(2) * np.arange(K - 1, -1, -1, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
    rcw = ((3 - codes[:, ::-1]).astype(np.uint64) << (np.uint64(2) * np.arange(K - 1, -1, -1, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
    index = np.unique(np.concatenate([np.lib.stride_tricks.sliding_window_view(s, K) for s in seqs]).astype(np.uint64)
                      @ (np.uint64(4) ** np.arange(K - 1, -1, -1, dtype=np.uint64)))
    can = np.nonzero(np.isin(w, index) | np.isin(rcw, index))[0]
    assert set(rows.tolist()) <= set(can.tolist())
    sub_e = G["odb"].scan_se(formats.pack_fixed(codes[can]))
    cnt = np.zeros(n, np.int64)
    cnt[can] = np.diff(sub_e[2])
    assert int((cnt[rows] > 0).sum()) == len(rows)
    rc_flag, flag = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc_flag[can], flag[can] = sub_e[0], sub_e[1]
    T_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    expect = (rc_flag, flag, T_off, sub_e[3])
    three_settings(G, None, monkeypatch, expect=expect, batch=formats.pack_fixed(codes), t_cap=int(T_off[-1]) + 1024, want_hits=len(rows))
