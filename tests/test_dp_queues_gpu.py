"""Stage 3a's device-wide DP queues (align.hip: dp_queues_kernel, one launch over the four width classes; the task is finished by
the problem that arrives last) against the CPU oracle, on reads whose DP problems are there by construction.

With k = 16 and the default penalties a tail with one mismatch is nw_diagonal's and so is a link with at most two; a tail with two
or more, or a link with three or more, is a DP problem as wide as the columns between the neighbouring MEMs or the read's end."""
import numpy as np
import pytest

from kma_amd import formats, synth

pytestmark = pytest.mark.gpu

L = 150
# offsets from the read's end of the mismatches of a trailing tail -> 7 (tiny), 13 (narrow), 25 (mid), 45 (wide) columns; a leading tail
# has them mirrored
TAILS = {"tiny": (7, 3), "narrow": (13, 4), "mid": (25, 13, 4), "wide": (45, 32, 19, 6)}
# first mismatch and spacing of a link's three -> 11 (narrow) and 25 (mid) columns; placed so that MEMs of 16 and more bases stand
# between it and the widest tails
LINKS = {"narrow": (66, 5), "mid": (62, 12)}


def _cut(rng, seqs, length=L):
    s = seqs[int(rng.integers(0, len(seqs)))]
    a = int(rng.integers(30, len(s) - length - 30))
    return s[a:a + length].copy()


def _plant(r, lead=None, link=None, trail=None, n=L):
    pos = []
    if lead:
        pos += [x - 1 for x in TAILS[lead]]
    if link:
        p, step = LINKS[link]
        pos += [p, p + step, p + 2 * step]
    if trail:
        pos += [n - x for x in TAILS[trail]]
    for p in pos:
        r[p] = (r[p] + 1) & 3
    return r


def _finish(rng, r):
    return np.ascontiguousarray(synth.revcomp_codes(r) if rng.random() < 0.5 else r).astype(np.uint8)


@pytest.fixture(scope="module")
def dbq(tmp_path_factory):
    rng = np.random.default_rng(2024)
    seqs = [rng.integers(0, 4, int(rng.integers(700, 901)), dtype=np.uint8) for _ in range(20)]
    prefix = str(tmp_path_factory.mktemp("dpq") / "db")
    formats.write_index(prefix, ["t%d" % i for i in range(len(seqs))], seqs)
    return dict(prefix=prefix, seqs=seqs, cache={})


def _batch(dbq, name):
    """the reads of a case and the oracle's results for them, made once"""
    if name in dbq["cache"]:
        return dbq["cache"][name]
    import oracle
    seqs = dbq["seqs"]
    reads = []
    if name == "alone":
        rng = np.random.default_rng(1)
        plans = [dict(trail=c) for c in TAILS] + [dict(lead=c) for c in TAILS] + [dict(link=c) for c in LINKS]
        for plan in plans:
            reads += [_finish(rng, _plant(_cut(rng, seqs), **plan)) for _ in range(200)]
    elif name == "several":
        rng = np.random.default_rng(2)
        for lead in (None,) + tuple(TAILS):
            for link in (None,) + tuple(LINKS):
                for trail in (None,) + tuple(TAILS):
                    if (lead is not None) + (link is not None) + (trail is not None) >= 2:
                        reads += [_finish(rng, _plant(_cut(rng, seqs), lead, link, trail)) for _ in range(24)]
    elif name == "punt":
        rng = np.random.default_rng(3)
        for i in range(900):
            if i % 3 == 0:      # a tiny leading tail (queued), 150 matching bases, then 80 foreign ones: a problem of 80 columns
                r = np.concatenate([_plant(_cut(rng, seqs, 157), lead="tiny", n=157), rng.integers(0, 4, 80, dtype=np.uint8)])
            else:
                r = _cut(rng, seqs)
            reads.append(_finish(rng, r))
    batch = formats.pack_ragged(reads)
    odb = oracle.OracleDB(dbq["prefix"])
    scan = odb.scan_se(batch)
    dbq["cache"][name] = (batch, scan, odb.align_se(batch, *scan))
    return dbq["cache"][name]


def _map(dbq, batch):
    from kma_amd import binding
    db = binding.KmaHipDB(dbq["prefix"])
    try:
        scan, h = db.map_se(batch)
        return scan, h, db.get_align_queue_counts()
    finally:
        db.close()


def _equal_oracle(scan, h, want_scan, o):
    for a, b in zip(want_scan, scan):
        assert np.array_equal(a, b)
    T_off = scan[2]
    assert np.array_equal(o["n_hits"], h["n_hits"])
    assert np.array_equal(o["best_score"], h["best_score"])
    assert np.array_equal(o["out_flag"], h["flag"])
    for i in np.nonzero(o["n_hits"] > 0)[0]:
        s, c = int(T_off[i]), int(o["n_hits"][i])
        for key in ("tmpl", "start", "end", "score"):
            assert np.array_equal(o[key][s:s + c], h[key][s:s + c]), (i, key)
    assert np.array_equal(o["alignment_scores"], h["alignment_scores"])
    assert np.array_equal(o["uniq_alignment_scores"], h["uniq_alignment_scores"])


def test_every_class_alone(dbq):
    batch, want_scan, o = _batch(dbq, "alone")
    scan, h, counts = _map(dbq, batch)
    print(counts)
    for c in ("wide", "mid", "narrow", "tiny"):
        assert counts[c] > 0, counts
    assert counts["pending"] > 0
    _equal_oracle(scan, h, want_scan, o)
    assert (o["n_hits"] > 0).sum() > 1900


def test_several_problems_per_task_in_different_classes(dbq):
    batch, want_scan, o = _batch(dbq, "several")
    scan, h, counts = _map(dbq, batch)
    print(counts)
    # two or three problems per read: the rows count more than one arrival
    assert counts["wide"] + counts["mid"] + counts["narrow"] + counts["tiny"] >= 2 * counts["pending"] > 0, counts
    _equal_oracle(scan, h, want_scan, o)


def test_queue_without_room(dbq, monkeypatch):
    monkeypatch.setenv("KMAHIP_ALIGN_DQ_CAP", "64")
    batch, want_scan, o = _batch(dbq, "alone")
    scan, h, counts = _map(dbq, batch)
    print(counts)
    assert counts["handed_on"] > 0, counts
    _equal_oracle(scan, h, want_scan, o)


def test_punt_behind_a_queued_problem(dbq):
    batch, want_scan, o = _batch(dbq, "punt")
    scan, h, counts = _map(dbq, batch)
    print(counts)
    _equal_oracle(scan, h, want_scan, o)


def test_couples(dbq):
    """the planted patterns on both mates of pairs through the paired entry point: one row and one count for both mates' problems"""
    import pe_util
    from kma_amd import binding
    rng = np.random.default_rng(5)
    seqs = dbq["seqs"]
    plans = [dict(trail=c) for c in TAILS] + [dict(lead=c) for c in TAILS] + [dict(link=c) for c in LINKS] + [dict(lead="tiny", link="mid", trail="wide")]
    s1, units = [], []
    for j in range(500):
        s = seqs[int(rng.integers(0, len(seqs)))]
        a = int(rng.integers(30, len(s) - 330))
        b = a + int(rng.integers(20, 150))
        m0 = _plant(s[a:a + L].copy(), **plans[j % len(plans)])
        m1 = synth.revcomp_codes(_plant(s[b:b + L].copy(), **plans[(j // len(plans) + j) % len(plans)]))
        if j & 1:
            m0, m1 = m1, m0
        for m in (m0, m1):
            pb = formats.pack_ragged([np.ascontiguousarray(m).astype(np.uint8)])
            s1.append(dict(seqlen=L, seq=pb.seq[:(L + 31) // 32].copy(), N=np.zeros(0, np.int32), hdr=b"p%d" % len(s1), pair=True))
        units.append(("pe", 2 * j, 2 * j + 1))
    g = dict(prefix=dbq["prefix"], s1=s1, units=units)
    want = pe_util.oracle_pe_conclave_records(g)
    db = binding.KmaHipDB(g["prefix"])
    try:
        got = pe_util.hip_pe_conclave(db, g, records_only=True)
    finally:
        db.close()
    assert len(want["n_hits"]) > 400
    for key in ("n_hits", "score", "q_len", "q_len2", "off", "tmpl", "start", "end", "alignment_scores", "uniq_alignment_scores"):
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("w", [8, 16, 32, 64])
def test_lane_moves(w):
    """the DPP moves of the sweep against __shfl_down(x, 1, w), on the lanes whose value nw_coop uses: all but a segment's last"""
    from kma_amd import binding
    x = np.random.default_rng(w).integers(-2 ** 31, 2 ** 31, 64, dtype=np.int64).astype(np.int32)
    got = binding.test_lane_down(x, w)
    lane = np.arange(64)
    want = np.where(lane % w == w - 1, x, np.roll(x, -1))      # numpy's __shfl_down(x, 1, w)
    used = lane % w != w - 1
    assert np.array_equal(got[used], want[used]), (w, got, want)


def test_determinism(dbq):
    batch, _, _ = _batch(dbq, "several")
    scan1, h1, _ = _map(dbq, batch)
    scan2, h2, _ = _map(dbq, batch)
    for a, b in zip(scan1, scan2):
        assert np.array_equal(a, b)
    assert sorted(h1) == sorted(h2)
    for key in h1:
        assert np.array_equal(h1[key], h2[key]), key
