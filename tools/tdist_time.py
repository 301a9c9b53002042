#!/usr/bin/env python3
"""Times of the template distances on one MI355X, against the 5 001-template database tools/sparse_time.py
builds (synth.make_gene_db(1667, 3, 500, 1300, 0.2, seed=7), indexed by `oracle/_ref/kma index -Sparse TG`). --dbs names more:
`plain` is the same FASTA indexed without -Sparse, `redundant` 50 families of 100 variants within 2 % of each other
(synth.make_gene_db(50, 100, 500, 1300, 0.02, seed=7), indexed without -Sparse): the database a curator would cluster, with value
lists up to 100 templates long.

Five kept runs each, after one that is not kept (code objects load on a first launch), with median and range: the counting kernels
under both forms (KMAHIP_TDIST_FORM = rows, pairs: tdist_mult_kernel, the inverted index with its scan, tdist_rows_kernel /
tdist_pairs_kernel; HIP events), the write kernels of `-d 8191` (HIP events, summed over the chunks), and the wall of the whole
`kmahip_dist` process for `-d 1` and `-d 8191` against `kma dist -t 1` and `-t 16` on the same host and files, with the files
compared byte for byte. Prints one JSON line, and puts its entries into the JSON object of --out.

    python tools/tdist_time.py [--dbs sparse_TG,plain,redundant] [--dir /tmp/tdist_time] [--repeat 5] [--out profiles/tdist_time.json]"""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kma_amd import binding, synth  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
DIST = os.path.join(ROOT, "examples", "kmahip_dist")


def wall(cmd, limit=300):
    """seconds of one process; `limit` ends a process that hangs (the longest here, `kma dist -d 8191 -t 1`, takes 12 s)"""
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=limit)
    dt = time.perf_counter() - t0
    print("[tdist_time] %.2f s  %s" % (dt, " ".join(cmd[:2] + cmd[-4:])), file=sys.stderr, flush=True)
    if p.returncode:
        raise SystemExit("%s -> %d %s" % (" ".join(cmd), p.returncode, p.stderr.decode()[-300:]))
    return dt


def summary(xs, digits=3):
    return dict(median=round(statistics.median(xs), digits), min=round(min(xs), digits), max=round(max(xs), digits), all=[round(x, digits) for x in xs])


def kernels(db, repeat, out):
    """-> per form the kernel times of `repeat` kept runs, the write kernels' under the default form, and whether both forms agree"""
    res = {f: dict(mult_ms=[], inverted_index_ms=[], pairs_or_rows_ms=[], count_wall_ms=[]) for f in ("rows", "pairs")}
    write_ms, write_launches, arrays = [], 0, {}
    for it in range(repeat + 1):
        for form in ("rows", "pairs"):
            os.environ["KMAHIP_TDIST_FORM"] = form
            with binding.TemplateDist(db) as td:
                td.set_timing(True)
                t0 = time.perf_counter()
                td.count()
                w = (time.perf_counter() - t0) * 1e3
                t = [td.get_timing(k)[0] for k in range(4)]
                if it == 0:
                    arrays[form] = td.counts()
                if form == "rows":
                    td.write(out, 8191, 1)
                    ms, n = td.get_timing(4)
                    if it:
                        write_ms.append(ms)
                        write_launches = n
                if it:
                    r = res[form]
                    r["mult_ms"].append(t[0]); r["inverted_index_ms"].append(t[1]); r["pairs_or_rows_ms"].append(t[3] if form == "pairs" else t[2]); r["count_wall_ms"].append(w)
                print("[tdist_time] run %d %s: count %.2f ms" % (it, form, w), file=sys.stderr, flush=True)
                info = dict(templates=td.n, kmers=int(td.info.n_kmers), lists=int(td.info.n_lists), values=int(td.info.n_values))
    del os.environ["KMAHIP_TDIST_FORM"]
    same = all((a == b).all() for a, b in zip(arrays["rows"], arrays["pairs"]))
    return dict(info, forms_agree=bool(same), rows={k: summary(v) for k, v in res["rows"].items()}, pairs={k: summary(v) for k, v in res["pairs"].items()},
                write_kernels_d8191_ms=summary(write_ms), write_kernel_launches=int(write_launches), d8191_bytes=os.path.getsize(out))


def processes(db, d, repeat, tmp):
    got, ref, ref16 = (os.path.join(tmp, x) for x in ("got.phy", "ref.phy", "ref16.phy"))
    res = {}
    for name, cmd in (("kmahip_dist_s", [DIST, "-t_db", db, "-o", got, "-d", str(d)]), ("kma_dist_t1_s", [KMA, "dist", "-t_db", db, "-o", ref, "-d", str(d), "-t", "1"]),
                      ("kma_dist_t16_s", [KMA, "dist", "-t_db", db, "-o", ref16, "-d", str(d), "-t", "16"])):
        res[name] = summary([wall(cmd) for _ in range(repeat + 1)][1:])
    res["files_identical"] = filecmp.cmp(got, ref, shallow=False) and filecmp.cmp(got, ref16, shallow=False)
    res["file_bytes"] = os.path.getsize(got)
    for f in (got, ref, ref16):
        os.remove(f)
    return res


def one_index(db, repeat, tmp):
    res = kernels(db, repeat, os.path.join(tmp, "k.phy"))
    os.remove(os.path.join(tmp, "k.phy"))
    res["d1"] = processes(db, 1, repeat, tmp)
    res["d8191"] = processes(db, 8191, repeat, tmp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dbs", default="sparse_TG")
    ap.add_argument("--dir", default="/tmp/tdist_time")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: the index is written by `kma index`, and `kma dist` is what the process is timed against")
    os.makedirs(a.dir, exist_ok=True)
    shapes = {"sparse_TG": ((1667, 3, 500, 1300, 0.2), ["-Sparse", "TG"]), "plain": ((1667, 3, 500, 1300, 0.2), []), "redundant": ((50, 100, 500, 1300, 0.02), [])}
    res = dict(repeat=a.repeat)
    for tag in a.dbs.split(","):
        shape, args = shapes[tag]
        fa = os.path.join(a.dir, tag + ".fsa")
        names, seqs = synth.make_gene_db(*shape, seed=7)
        synth.write_fasta(fa, names, seqs)
        db = os.path.join(a.dir, "db_" + tag)
        wall([KMA, "index", "-i", fa, "-o", db] + args)
        res[tag] = one_index(db, a.repeat, a.dir)
    print(json.dumps(res))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        old.update(res)
        with open(a.out, "w") as f:
            f.write(json.dumps(old) + "\n")


if __name__ == "__main__":
    main()
