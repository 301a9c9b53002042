"""Hand-made traces for the pile-up (stage 3c: pileup_device of kma_amd/csrc/assemble.hip), shared by its tests. No test lives here.

A trace is what the traceback aligner hands the pile-up about one read: the `stats` row and the runs `(length << 2) | class`, classes
= X I D (0 1 2 3: aligned and equal, aligned and different, bases the template lacks, template columns the read lacks). `make` turns
`(template, start, clip_start, runs)` into one, with the read such an alignment belongs to; `Batch` packs a list of them into what
binding.KmaHipDB.assemble takes and what oracle.Assembly.add takes, in the order the device piles them up."""
import numpy as np

from kma_amd import formats, synth

CLS = {"=": 0, "X": 1, "I": 2, "D": 3}


def stats_of(t_len, start, clip_start, runs, q_len, score=1, mapq=0):
    """the `stats` row of a trace: score, start, end, aln_len, clip_start, clip_end, match, tGaps, qGaps, mapQ. aln_len counts every
    column, tGaps the I columns, qGaps the D columns (pile_visits takes aln_len - tGaps, less the trimmed gap runs, as the template
    span); end = start + that span, folded into 1 .. t_len for an alignment that goes round the origin"""
    aln_len = sum(n for _, n in runs)
    t_gaps = sum(n for c, n in runs if c == "I")
    q_gaps = sum(n for c, n in runs if c == "D")
    match = sum(n for c, n in runs if c in "=X")          # (aligned pairs, equal or not)
    end = start + aln_len - t_gaps
    while end > t_len:
        end -= t_len
    q_used = aln_len - q_gaps
    return np.array([score, start, end, aln_len, clip_start, q_len - clip_start - q_used, match, t_gaps, q_gaps, mapq], np.int32)


def ops_of(runs):
    return np.array([(n << 2) | CLS[c] for c, n in runs], np.uint32)


def runs_of(ops):
    return [("=XID"[int(x) & 3], int(x) >> 2) for x in ops]


def trimmed(start, runs):
    """what read_runs / alnToMat (assembly.c:1340-1354) pile up of a trace: gap runs at either end are dropped, a leading D run moves
    the start, a leading I run the read position; column 0 is never dropped from behind -> (start, read bases skipped, runs)"""
    runs = list(runs)
    while len(runs) > 1 and runs[-1][0] in "ID":
        runs.pop()
    skip = 0
    while runs and runs[0][0] in "ID":
        c, n = runs.pop(0)
        if c == "D":
            start += n
        else:
            skip += n
    return start, skip, runs


def make(seq, start, clip_start, runs, rng, clip_end=0, n_at=(), score=1):
    """A trace on the ring `seq` (codes 0-3) and its read. runs: [(class, length)]; the read copies the template on `=`, differs on X,
    brings bases of its own on I and on the clips. n_at: indices into the ALIGNED part of the read that hold an N (they must lie on
    X or I columns, or the `=` would not be one). -> dict(stats, ops, cols, read (oriented like the template), start, score)"""
    t_len = len(seq)
    assert 0 <= start < t_len and all(n > 0 and c in CLS for c, n in runs)
    assert all(a[0] != b[0] for a, b in zip(runs, runs[1:])), "adjacent runs of one class are one run"
    parts, p = [rng.integers(0, 4, clip_start, dtype=np.uint8)], start
    for c, n in runs:
        if c in "=X":
            b = seq[(p + np.arange(n)) % t_len].astype(np.uint8)
            parts.append(b if c == "=" else (b + rng.integers(1, 4, n, dtype=np.uint8)) & 3)
        elif c == "I":
            parts.append(rng.integers(0, 4, n, dtype=np.uint8))
        if c != "I":
            p += n
    parts.append(rng.integers(0, 4, clip_end, dtype=np.uint8))
    read = np.concatenate(parts).astype(np.uint8)
    for i in n_at:
        read[clip_start + i] = 4
    cols = "".join(c * n for c, n in runs).encode()
    return dict(stats=stats_of(t_len, start, clip_start, runs, len(read), score), ops=ops_of(runs), cols=cols, read=read, start=start,
                score=score, clip_start=clip_start)


def dropped(rng, n=40):
    """a read the aligner dropped: a row of zeros, no runs"""
    return dict(stats=np.zeros(10, np.int32), ops=np.zeros(0, np.uint32), cols=b"", read=rng.integers(0, 4, n, dtype=np.uint8), start=0,
                score=0, clip_start=0)


class Batch:
    """traces [(template id (1-based), trace of make() or dropped(), stored reverse-complemented?)] -> the arrays of KmaHipDB.assemble.
    A read stored reverse-complemented is filed either with the rc flag set or under the negative template id, in turn."""

    def __init__(self, items):
        self.items = items
        n = len(items)
        stored, self.rc, self.tmpl = [], np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i, (t, tr, rev) in enumerate(items):
            stored.append(np.ascontiguousarray(synth.revcomp_codes(tr["read"]) if rev else tr["read"]))
            self.tmpl[i] = t
            if rev and i & 1:
                self.rc[i] = 1
            elif rev:
                self.tmpl[i] = -t
        self.batch = formats.pack_ragged(stored)
        self.stats = np.stack([tr["stats"] for _, tr, _ in items]).astype(np.int32)
        self.n_ops = np.array([len(tr["ops"]) for _, tr, _ in items], np.int32)
        self.ops_off = np.concatenate([[0], np.cumsum(self.n_ops)[:-1]]).astype(np.int64)
        self.ops = np.concatenate([tr["ops"] for _, tr, _ in items]).astype(np.uint32)

    @property
    def traces(self):
        return self.stats, self.ops_off, self.n_ops, self.ops

    def order(self, t, max_frag=0):
        """indices of template t's traces in the order the device piles them up: rank among the filed reads, back to front inside
        every chunk of max_frag (ConClave prepends to a per-template list, conclave.c:164-165)"""
        mf = max_frag if max_frag > 0 else 1000000
        idx = [i for i, (tt, tr, _) in enumerate(self.items) if tt == t and tr["stats"][3]]
        return sorted(idx, key=lambda i: (i // mf) * mf + (mf - 1 - i % mf))

    def oracle(self, odb, t, t_len, max_frag=0):
        """oracle.Assembly of template t with the traces added in that order"""
        import oracle
        oa = oracle.Assembly(odb, t, t_len)
        for i in self.order(t, max_frag):
            tr = self.items[i][1]
            oa.add(tr, tr["read"])
        return oa


def runs_from(span, I=None, D=None, X=()):
    """runs of an alignment over `span` template columns, counted from its first one: I {column: n} = n bases in front of that column,
    D {column: n} = the read lacks that column and the n - 1 behind it, X = columns with another base"""
    cols = np.full(span, ord("="), np.uint8)
    if len(X):
        cols[np.asarray(sorted(X), np.int64)] = ord("X")
    for c, n in (D or {}).items():
        cols[c:c + n] = ord("D")
    out, at = [], 0
    for c in sorted(I or {}):
        out += [cols[at:c].tobytes(), b"I" * I[c]]
        at = c
    out.append(cols[at:].tobytes())
    text = b"".join(out).decode()
    runs, i = [], 0
    while i < len(text):
        j = i
        while j < len(text) and text[j] == text[i]:
            j += 1
        runs.append((text[i], j - i))
        i = j
    return runs


# ---- the cases of tests/test_pileup_routes_gpu.py ---------------------------------------------------------------------------------------
T_LONG, T_MID, T_SHORT = 1, 2, 3          # templates of 6 000 (cut into units), 700 (whole, in LDS or on HBM) and 64 bases


def templates():
    rng = np.random.default_rng(4242)
    return ["cut into units", "whole", "tiny"], [rng.integers(0, 4, n, dtype=np.uint8) for n in (6000, 700, 64)]


class _Case:
    def __init__(self, seqs, seed):
        self.seqs, self.rng, self.items = seqs, np.random.default_rng(seed), []

    def add(self, t, start, span, I=None, D=None, x_rate=0.03, runs=None, n_rate=0.0):
        """one read over `span` columns of template t from `start` on; every third read carries clips, every other one is stored
        reverse-complemented"""
        rng, seq = self.rng, self.seqs[t - 1]
        if runs is None:
            X = set(int(c) for c in np.nonzero(rng.random(span) < x_rate)[0]) - {0, span - 1}
            runs = runs_from(span, I, D, X)
        k = len(self.items)
        tr = make(seq, start % len(seq), int(rng.integers(1, 6)) if k % 3 == 0 else 0, runs, rng, clip_end=int(rng.integers(0, 4)) if k % 3 == 0 else 0)
        if n_rate:
            # N on X columns only
            q, at = tr["clip_start"], []
            for c, n in runs:
                if c == "X":
                    at += [q + i for i in range(n) if rng.random() < n_rate]
                if c != "D":
                    q += n
            tr["read"][at] = 4
        self.items.append((t, tr, bool(k & 1)))
        return tr


def case(name, seqs, S):
    """the traces of one case for a route whose units are S columns long -> [(template, trace, stored reverse-complemented)]"""
    L, M, T = (len(s) for s in seqs)
    lo, hi = 2 * S, 3 * S                       # the unit the boundary cases stand on
    c = _Case(seqs, {"boundaries": 1, "origin": 2, "wrapped": 3, "turns": 4, "rounds": 5, "mix1": 61, "mix2": 62, "ladder": 7}[name])
    rng = c.rng
    if name == "boundaries":
        for _ in range(3):                      # something underneath, so that the depths differ from column to column
            c.add(T_LONG, lo - 250 + int(rng.integers(0, 100)), S + 400)
        c.add(T_LONG, lo, 300)                  # first column at lo, at lo - 1, at hi - 1
        c.add(T_LONG, lo - 1, 300)
        c.add(T_LONG, hi - 1, 300)
        c.add(T_LONG, hi - 300, 300)            # last column at hi - 1, at lo - 1
        c.add(T_LONG, lo - 300, 300)
        c.add(T_LONG, lo - 100, 300, D={98: 5})                 # a D run across lo, one across hi
        c.add(T_LONG, hi - 100, 300, D={97: 4})
        c.add(T_LONG, lo - 150, 400, I={150: 2})                # an I run whose site is lo: its chain hangs in front of the unit's first column
        c.add(T_LONG, hi - 200, 400, I={199: 3})                # ... whose site is hi - 1
        c.add(T_LONG, lo - 100, 300, I={99: 2, 100: 1})         # two I runs one aligned base apart: sites lo - 1 and lo
        c.add(T_LONG, lo - 100, 300, I={100: 1, 101: 2})        # ... sites lo and lo + 1
        c.add(T_LONG, hi - 100, 300, I={99: 1, 100: 3})         # ... sites hi - 1 and hi
        c.add(T_LONG, hi - 100, 300, I={98: 2, 99: 2, 100: 2, 101: 2})
        for site in (lo, hi - 1, hi, lo + 1, lo - 1):
            for n in (1, 3, 0, 2, 5, 0, 4):     # shorter then longer and the reverse; 0: a read that lacks the chain
                a = site - 60 - int(rng.integers(0, 40))
                c.add(T_LONG, a, 200, I={site - a: n} if n else None)
    elif name == "origin":
        for t, n, sp in ((T_LONG, L, 300), (T_MID, M, 300), (T_SHORT, T, 30)):
            c.add(t, n - sp, sp)                                # the last column is t_len - 1
            c.add(t, 0, sp)                                     # the first column is 0
            c.add(t, n - sp // 2, sp, I={sp // 2: 2})           # an I run in front of column 0: chained off column t_len - 1
            c.add(t, n - sp, sp)
            c.add(t, n - sp // 2, sp, I={sp // 2: 3})
            c.add(t, 0, sp, I={1: 1})
            c.add(t, n - sp, sp, I={sp - 1: 2})                 # site t_len - 1
            c.add(t, 0, 0, runs=[("I", 2), ("=", sp // 2), ("X", 1), ("=", sp // 3)])       # trimmed: the read position moves
            c.add(t, 0, 0, runs=[("D", 3), ("=", sp // 2), ("I", 1), ("=", sp // 3), ("D", 2), ("I", 2)])      # trimmed: the start moves
            c.add(t, n - sp // 2, sp)
    elif name == "wrapped":
        for over in (1, S - 1, S, S + 1):                       # across the origin by that many columns
            c.add(T_LONG, L - 300, 300 + over)
            c.add(T_LONG, L - 300, 300 + over, I={300: 2, 300 + over - 1: 1} if over > 2 else {300: 2})
        c.add(T_LONG, L - 100, 300, I={100: 2})                 # an I run whose site is column 0
        c.add(T_LONG, L - 100, 300, I={100: 1, 101: 1})
        c.add(T_LONG, L - 100, 300, D={98: 5})                  # a D run across the origin
        c.add(T_LONG, L - 100, 300, D={100: 3})
        c.add(T_LONG, L - 10, 500, I={10: 4})                   # starts inside the last unit
        c.add(T_LONG, L - S + 1, S + 200)
        c.add(T_LONG, 10, L - 5, I={700: 2, L - 10: 3})         # covers everything: the wrap's units reach the first one
        c.add(T_LONG, 3000, L, I={3000: 2})                     # exactly one turn
        c.add(T_LONG, 0, L)
        c.add(T_LONG, L - 50, 150, I={50: 1})
        for t, n in ((T_MID, M), (T_SHORT, T)):
            c.add(t, n - n // 3, n // 2, I={n // 3: 2})
            c.add(t, n // 2, n, I={n // 2: 1})
            c.add(t, n - n // 3, n // 2, D={n // 3 - 1: 3})
            c.add(t, n - 1, n - 1)
    elif name == "turns":
        for t, n, s in ((T_LONG, L, S), (T_MID, M, 64), (T_SHORT, T, 8)):
            q = n // 3
            c.add(t, q, n // 2, I={n // 4: 1})                  # reads of one turn underneath
            c.add(t, n - q, n // 2, I={q: 2, q + 5: 1})
            c.add(t, q, n + 1)                                  # one column more than a turn
            c.add(t, n - q, n + s, I={q: 2})                    # site column 0 in the first turn, passed again in the second
            c.add(t, q, n + n // 2, I={n + 7: 2})               # the second turn brings an I run where the first had none
            c.add(t, q + 9, n // 2, I={n // 4: 3})
            c.add(t, 2 * q, n + n // 2, I={11: 1, n + 11: 3})   # ... and where the first had a shorter one
            c.add(t, 2 * q, n + n // 2, I={13: 3, n + 13: 1}, D={n + 5: 2})
            c.add(t, 5, 2 * n)                                  # exactly two turns
            c.add(t, q, 2 * n, I={n: 2})                        # ... with an I run in front of the second turn's first column
            c.add(t, 2 * q, 2 * n + 40 if n > 100 else 2 * n + 5, I={n - 1: 1, n + 1: 2, 2 * n: 1}, D={n - 3 - q % 2: 2})
            c.add(t, n - 1, 2 * n + 2, I={1: 1, n + 1: 1, 2 * n + 1: 1})
            c.add(t, q, n // 2, I={n // 4: 2, n // 4 + 1: 1})   # one turn, on top
            c.add(t, 0, n, I={q: 1})
    elif name == "rounds":
        def jagged(span, every, start_with):
            # =1 X1 =1 X1 ..., an I or a D every `every` columns
            runs, k, col = [], 0, 0
            while col < span:
                runs.append(("=" if (col & 1) == 0 else "X", 1))
                col += 1
                if col % every == 0 and col < span - 2:
                    k += 1
                    if (k + start_with) & 1:
                        runs.append(("I", 1 + k % 3))
                    else:
                        runs.append(("D", 1 + k % 2))
                        col += 1 + k % 2
            return runs
        c.add(T_LONG, S + 17, 1500)
        r1, r2 = jagged(1300, 7, 0), jagged(2400, 9, 1)
        assert 1024 < len(r1) <= 2048 < len(r2)
        c.add(T_LONG, S - 100, 0, runs=r1)                      # more than 1 024 runs: two rounds of 1 024 threads, three of 512
        c.add(T_LONG, S + 300, 900, I={63: 2, 400: 1})
        c.add(T_LONG, 2 * S - 1000, 0, runs=r2)                 # more than 2 048
        c.add(T_LONG, L - 700, 0, runs=r1)                      # ... across the origin: no checkpoints, every unit scans from the first run
        c.add(T_LONG, 100, 0, runs=jagged(L + 500, 5, 0))       # ... and round the ring and on
        c.add(T_LONG, S, 2000, I={7: 1, 14: 1, 1024: 2})
    elif name in ("mix1", "mix2"):
        def indels(span, a, b):
            I, D, col = {}, {}, int(rng.integers(a, b))
            while col < span - 5:
                if rng.random() < 0.5:
                    I[col] = int(rng.integers(1, 4))
                else:
                    D[col] = int(rng.integers(1, 4))
                col += 4 + int(rng.integers(a, b))
            return I, D
        for k in range(300):
            u = rng.random()
            if k % 50 == 49:
                c.items.append((int(rng.integers(1, 4)), dropped(rng), bool(k & 1)))
                continue
            if u < 0.66:
                t, n = T_LONG, L
                v = rng.random()
                if v < 0.25:                    # on a unit boundary, either end
                    b = S * int(rng.integers(1, L // S + 1))
                    span = int(rng.integers(200, 1500))
                    start = (b - int(rng.integers(0, 3))) if rng.random() < 0.5 else (b - span - int(rng.integers(-1, 2)))
                elif v < 0.93:
                    span, start = int(rng.integers(200, 2600)), int(rng.integers(0, L))
                else:                           # more than one turn
                    span, start = int(L * (1.0 + 1.1 * rng.random())), int(rng.integers(0, L))
                I, D = indels(span, 30, 300)
            elif u < 0.86:
                t, n = T_MID, M
                span, start = int(rng.integers(100, 1200)), int(rng.integers(0, M))
                I, D = indels(span, 20, 150)
            else:
                t, n = T_SHORT, T
                span, start = int(rng.integers(20, 150)), int(rng.integers(0, T))
                I, D = indels(span, 8, 40)
            c.add(t, start % n, span, I=I, D=D, n_rate=0.2 if k % 7 == 0 else 0.0)
    elif name == "ladder":
        # one insertion column per unit of 64 columns and no more: with KMAHIP_PILE_LDS_NODES=1 every longer unit overflows
        sites = [64 * k + 10 for k in range(3, 40)]
        for k in range(12):
            a, span = 64 * 2 + 7 * k, 2400 + 11 * k
            c.add(T_LONG, a, span, I={s - a: 1 for s in sites if a < s < a + span - 1 and (k % 4 != 3 or s % 128 == 10)})
        # the whole templates need more than one: on to HBM
        c.add(T_MID, 100, 500, I={50: 2, 300: 1})
        c.add(T_MID, 600, 900, I={80: 1, 330: 3})
        c.add(T_SHORT, 60, 100, I={4: 2, 50: 1})
        c.add(T_SHORT, 3, 40, I={8: 1})
    else:
        raise KeyError(name)
    return c.items
