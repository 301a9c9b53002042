#!/usr/bin/env python3
"""CPU model of the diagonal that stage 2's prefilter files with a record, and of what the scan's lanes find along it
(DESIGN.md section 3.1, round 7). numpy only, seeded, reads nothing but the repository's own generators.

The rule modelled is the kernels': a slot of the probe table points at the FIRST occurrence of its k-mer in the concatenated
templates; the prefilter files the diagonal of its first stride hit; with repair tries, at two or more mismatching bases it looks up
the read's k-mer that ends at the first mismatching base it has not tried yet and keeps that hit's diagonal when fewer bases
differ along it. Counted per read, on the read's true strand: mismatches against the filed diagonal, the sequencing errors among
them, k-mer starts that fail on the diagonal, failing anchors of the 16 lanes (a lane owns 9 starts), starts of a failing lane
that are on the diagonal all the same, and the repair's table probes.

    python tools/diag_model.py [--families 1000] [--reads 20000] [--seed 1]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kma_amd import synth  # noqa: E402

K, L, SEG = 16, 150, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    _, seqs = synth.make_gene_db(a.families, 5, 600, 1500, 0.04, seed=12345)
    lens = np.array([len(s) for s in seqs], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    cat = np.concatenate(seqs + [np.zeros(64, np.uint8)])
    # every k-mer start inside a template, its key, and the first position of every key
    pos = np.concatenate([np.arange(off[t], off[t] + lens[t] - K + 1) for t in range(len(seqs))])
    key = np.zeros(len(pos), np.uint64)
    for i in range(K):
        key = (key << np.uint64(2)) | cat[pos + i].astype(np.uint64)
    order = np.lexsort((pos, key))
    ukey, first_i = np.unique(key[order], return_index=True)
    first = pos[order][first_i]

    def lookup(kmer):
        k = np.uint64(0)
        for b in kmer:
            k = (k << np.uint64(2)) | np.uint64(b)
        i = np.searchsorted(ukey, k)
        return int(first[i]) if i < len(ukey) and ukey[i] == k else None

    # round 11, the span table (DevDB::span): the templates of every k-mer, and `need` at a position -- the fewest k-mer starts from
    # there on, all inside its template, whose template sets have that template alone in common (None: never within the template)
    tmpl_sorted = (np.searchsorted(off, pos[order], side="right") - 1).astype(np.int64)
    bounds = np.concatenate([first_i, [len(order)]])

    def templates(p):
        k = np.uint64(0)
        for b in cat[p:p + K]:
            k = (k << np.uint64(2)) | np.uint64(b)
        i = np.searchsorted(ukey, k)
        return set(tmpl_sorted[bounds[i]:bounds[i + 1]].tolist())

    def need_at(p):
        t0 = int(np.searchsorted(off, p, side="right") - 1)
        room = int(off[t0] + lens[t0] - K + 1 - p)
        others = None
        for j in range(min(room, 254)):
            s = templates(p + j)
            others = s - {t0} if others is None else others & s
            if not others:
                return t0, j + 1, room
        return t0, None, room

    rng = np.random.default_rng(a.seed)
    ok = np.nonzero(lens >= L)[0]
    npos = L - K + 1
    tot = {tries: np.zeros(8) for tries in (0, 1, 2)}
    n = 0
    zero_mism = settled = own_template = 0
    needs = []
    for _ in range(a.reads):
        t = int(ok[rng.integers(0, len(ok))])
        st = int(rng.integers(0, lens[t] - L + 1))
        own = int(off[t]) + st
        r = cat[own:own + L].copy()
        err = rng.random(L) < 0.005
        r[err] = (r[err] + rng.integers(1, 4, int(err.sum()), dtype=np.uint8)) & 3
        a0 = None
        for j in range(0, npos, K):
            gp = lookup(r[j:j + K])
            if gp is not None:
                a0 = gp - j
                break
        if a0 is None:
            continue
        n += 1

        def mism(x):
            if x < 0 or x + L > len(cat):
                return None
            return np.nonzero(cat[x:x + L] != r)[0]

        for tries in (0, 1, 2):
            diag, d, probes, tried = a0, mism(a0), 0, set()
            for _try in range(tries):
                if d is None or len(d) < 2:
                    break
                cand = [int(b) for b in d if int(b) not in tried]
                if not cand:
                    break
                b = cand[0]
                tried.add(b)
                s0 = min(max(0, b - K + 1), L - K)
                probes += 1
                gp = lookup(r[s0:s0 + K])
                if gp is None:
                    continue
                d1 = mism(gp - s0)
                if d1 is not None and len(d1) < len(d):
                    diag, d = gp - s0, d1
            if tries == 1 and d is not None and len(d) == 0 and diag + L <= off[-1]:
                # the prefilter's settle route: no mismatch along the filed diagonal, and the table there says need <= npos <= room
                zero_mism += 1
                t0, nd, room = need_at(diag)
                if nd is not None and nd <= npos <= room:
                    settled += 1
                    needs.append(nd)
                    own_template += t0 == t
            bad = np.zeros(L, bool)
            if d is not None:
                bad[d] = True
            else:
                bad[:] = True
            fail = np.convolve(bad.astype(np.int32), np.ones(K, np.int32))[K - 1:K - 1 + npos] > 0
            anchors = np.arange(0, npos, SEG)
            behind = 0
            for j0 in anchors[fail[anchors]]:
                behind += int((~fail[j0:min(j0 + SEG, npos)]).sum())
            tot[tries] += (int(bad.sum()), int((bad & err).sum()), diag == own, int(fail.sum()), int(fail[anchors].sum()), behind, probes,
                           diag != a0)
    print(f"{n} live reads of {a.reads} ({5 * a.families} genes, k = {K}, {L} bases, 0.5 % substitutions)")
    head = ("mismatches", "of them errors", "own diagonal", "failing starts", "failing anchors", "clean behind a failing anchor",
            "repair probes", "diagonal replaced")
    print(f"{'per read':32s}" + "".join(f"{x:>12s}" for x in ("no repair", "one try", "two tries")))
    for i, h in enumerate(head):
        print(f"{h:32s}" + "".join(f"{tot[tries][i] / max(1, n):12.3f}" for tries in (0, 1, 2)))
    nd = np.array(needs if needs else [0])
    print(f"one try: {100 * zero_mism / max(1, n):.1f} % of the live reads have no mismatch on the filed diagonal; {100 * settled / max(1, n):.1f} % are settled "
          f"by the span table (need <= {npos} <= room), {own_template} of {settled} on their own template; need of the settled: mean {nd.mean():.1f}, "
          f"median {int(np.median(nd))}, 99th percentile {int(np.percentile(nd, 99))}")


if __name__ == "__main__":
    main()
