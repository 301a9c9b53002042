#!/usr/bin/env python3
"""Times of sparse mapping (sparse section): N reads of 150 bases against the `w`-shaped database of the tests
(synth.make_gene_db(families, 3, 500, 1300, 0.2)) scaled to ~5000 templates, indexed by `oracle/_ref/kma index -Sparse TG`.

Prints one JSON line with: the counting kernel's time with its adds and without them (kmahip_sparse_set_noadd), the collect kernel's
time, the withdraw kernel's time (sum and launches), the wall of `kmahip_map -Sparse` and of `oracle/_ref/kma -Sparse -t 1 / -t 16`
on the same host and files, and whether the two `.spa` files are identical.

    python tools/sparse_time.py [--reads 1000000] [--families 1667] [--dir /tmp/sparse_time] [--repeat 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kma_amd import binding, synth  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")


def wall(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    if p.returncode not in (0, 2):          # (the reference ORs errno into its exit status, kma.c:1630)
        raise SystemExit("%s -> %d" % (" ".join(cmd), p.returncode))
    return dt


def kernel_times(db, fq, repeat):
    """the counting kernel with its adds and without them, alternating, after one run of each that is not kept (code objects load on a
    first launch) -> ([with adds], [without]) of (count ms, collect ms, withdraw ms, withdraw launches, rows) per repeat"""
    out = ([], [])
    for it in range(2 * (repeat + 1)):
        noadd = it & 1
        with binding.SparseDB(db) as sdb:
            sdb.set_timing(True)
            sdb.set_noadd(noadd)
            with binding.Ingest(fq) as ing:
                while True:
                    got = ing.next(1 << 20)
                    if got is None:
                        break
                    sdb.count(got[0])
            rows = sdb.rows() if not noadd else []
            c, col, wd = sdb.get_timing(0), sdb.get_timing(1), sdb.get_timing(2)
            if it >= 2:
                out[noadd].append((c[0], col[0], wd[0], wd[1], len(rows)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--families", type=int, default=1667)
    ap.add_argument("--dir", default="/tmp/sparse_time")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: the sparse index is written by `kma index -Sparse`")
    os.makedirs(a.dir, exist_ok=True)
    fa, fq, db = (os.path.join(a.dir, x) for x in ("db.fsa", "reads.fq", "db"))
    names, seqs = synth.make_gene_db(a.families, 3, 500, 1300, 0.2, seed=7)
    synth.write_fasta(fa, names, seqs)
    reads, *_ = synth.make_reads(seqs, a.reads, read_len=150, sub_rate=0.005, n_rate=0.0002, seed=7)
    synth.write_fastq(fq, reads)
    del reads
    t_index = wall([KMA, "index", "-i", fa, "-o", db, "-Sparse", "TG"])
    with_adds, without = kernel_times(db, fq, a.repeat)
    best = lambda rows, i: min(r[i] for r in rows)
    res = dict(reads=a.reads, templates=len(seqs), index_s=round(t_index, 2),
               count_ms=round(best(with_adds, 0), 3), count_noadd_ms=round(best(without, 0), 3), collect_ms=round(best(with_adds, 1), 3),
               withdraw_ms_sum=round(best(with_adds, 2), 3), withdraw_launches=with_adds[0][3], rows=with_adds[0][4],
               count_ms_all=[round(r[0], 3) for r in with_adds], count_noadd_ms_all=[round(r[0], 3) for r in without])
    with binding.SparseDB(db) as sdb:
        res["index_kmers"] = int(sdb.info.n_kmers)
    walls = [round(wall([MAP, "-i", fq, "-t_db", db, "-o", os.path.join(a.dir, "got"), "-Sparse"]), 3) for _ in range(a.repeat + 1)][1:]
    res["kmahip_map_s"], res["kmahip_map_s_all"] = min(walls), walls
    res["kma_t1_s"] = round(wall([KMA, "-i", fq, "-t_db", db, "-o", os.path.join(a.dir, "ref"), "-Sparse", "-t", "1"]), 3)
    res["kma_t16_s"] = round(wall([KMA, "-i", fq, "-t_db", db, "-o", os.path.join(a.dir, "ref16"), "-Sparse", "-t", "16"]), 3)
    res["spa_identical"] = open(os.path.join(a.dir, "got.spa"), "rb").read() == open(os.path.join(a.dir, "ref.spa"), "rb").read()
    res["speedup_t1"] = round(res["kma_t1_s"] / res["kmahip_map_s"], 2)
    res["speedup_t16"] = round(res["kma_t16_s"] / res["kmahip_map_s"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
