"""The span table (DevDB::span) restated in numpy (tests/span_model.py) against the oracle, on the CPU: for EVERY position p of a
small database and EVERY number of k-mer starts npos that fits behind it, the read that is the exact substring of its template is
scanned by oracle.OracleDB.scan_se, and

    need[p] <= npos <= room[p]   <=>   the oracle returns t0[p] alone, with the score k*M + (npos - 1)*M.

Under the default scoring scheme and two others that pass the sign test of the prefilter's route (M > 0, MM < M, U <= 0, W1 <= 0).
The database holds families of close variants (need from 1 to "never"), a pair of templates that share a stretch in the middle and
a pair that share everything from a point to their ends (never settled there)."""
import numpy as np
import pytest

import scheme_sets as ss
import span_model
from kma_amd import formats, synth

K = 16


def make_small_db(seed=11):
    """(names, seqs): 2 families of 3 variants of 90 .. 120 bases; x / y share bases 30 .. 69 of x (40 bases) in their middles;
    u / v share their last 50 bases"""
    names, seqs = synth.make_gene_db(n_families=2, variants=3, len_lo=90, len_hi=120, max_div=0.05, seed=seed)
    rng = np.random.default_rng(seed + 1)
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    x = rnd(100)
    y = np.concatenate([rnd(25), x[30:70], rnd(30)])
    y[24], y[65] = (x[29] + 1) & 3, (x[70] + 1) & 3          # (the stretch ends where it is said to)
    tail = rnd(50)
    u, v = np.concatenate([rnd(45), tail]), np.concatenate([rnd(38), tail])
    return list(names) + ["x", "y", "u", "v"], list(seqs) + [x, y, u, v]


def table_of(prefix, seqs):
    return span_model.span_table(seqs, formats.comp_db_mapping(formats.read_comp_b(prefix + ".comp.b")), K)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    import oracle
    names, seqs = make_small_db()
    prefix = str(tmp_path_factory.mktemp("span") / "db")
    formats.write_index(prefix, names, seqs, k=K)
    t0, need, room = table_of(prefix, seqs)
    # every substring read: (position, npos)
    cases, reads = [], []
    g0 = 0
    for s in seqs:
        for i in range(len(s) - K + 1):
            assert room[g0 + i] == min(255, len(s) - K + 1 - i) and t0[g0 + i] > 0
            for npos in range(1, int(room[g0 + i]) + 1):
                cases.append((g0 + i, npos))
                reads.append(s[i:i + npos + K - 1])
        g0 += len(s)
    return dict(prefix=prefix, seqs=seqs, t0=t0, need=need, room=room, cases=np.array(cases), batch=formats.pack_ragged(reads),
                odb=oracle.OracleDB(prefix))


def test_the_table_has_every_kind_of_entry(small):
    t0, need, room = small["t0"], small["need"], small["room"]
    live = room > 0
    assert (need[live] == 1).any() and ((need[live] > 1) & (need[live] < 255)).any() and (need[live] == 255).any()
    assert (need[live] >= 1).all() and not live[-64:].any()
    # the stretch u and v share to their ends is never settled; the one in the middles of x and y is, once a read leaves it
    off = np.concatenate([[0], np.cumsum([len(s) for s in small["seqs"]])])
    iu, ix = len(small["seqs"]) - 2, len(small["seqs"]) - 4
    assert (need[off[iu] + 45:off[iu] + 95 - K + 1] == 255).all()
    assert need[off[ix] + 30] == 70 - 30 - K + 2          # the first start behind the shared stretch ends the tie
    assert t0[off[ix] + 30] == ix + 1


@pytest.mark.parametrize("scheme", ["default", "gmm1", "gmm6"])
def test_settled_is_what_the_oracle_finds(small, scheme):
    s = ss.SCHEMES[scheme]
    M, MM = s.M, ss.mm_of(s)
    assert M > 0 and MM < M and s.U <= 0 and s.W1 <= 0
    odb = small["odb"]
    ss.apply(odb.rw, s)
    try:
        rc_flag, flag, T_off, T = odb.scan_se(small["batch"])
    finally:
        ss.apply(odb.rw, ss.SCHEMES["default"])
    p, npos = small["cases"][:, 0], small["cases"][:, 1]
    want = span_model.settled(small["need"][p].astype(np.int64), small["room"][p].astype(np.int64), npos)
    n_t = np.diff(T_off)
    first = T[np.minimum(T_off[:-1], max(len(T) - 1, 0))]
    alone = (n_t == 1) & (first == small["t0"][p]) & (rc_flag == K * M + (npos - 1) * M)
    assert int(want.sum()) > 1000 and int((~want).sum()) > 1000
    bad = np.nonzero(alone != want)[0]
    assert len(bad) == 0, (scheme, [(int(p[i]), int(npos[i]), int(rc_flag[i]), T[T_off[i]:T_off[i + 1]].tolist()) for i in bad[:5]])
    # and a read that is not settled still finds its template, tied with others at the full score
    tied = ~want
    assert (n_t[tied] >= 2).all() and (np.abs(rc_flag[tied]) == K * M + (npos[tied] - 1) * M).all()
