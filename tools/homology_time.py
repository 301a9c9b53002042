#!/usr/bin/env python3
"""Times of homology reduction while a sparse index is built (`kmahip_index -Sparse TG -hq 0.9 -ht 0.9 -and`) on
one MI355X host, on two databases: `redundant`, 50 families of 100 variants within 2 % of each other (the shape tools/tdist_time.py
uses), and `genes`, the 5 001 templates of tools/sparse_time.py (synth.make_gene_db(1667, 3, 500, 1300, 0.2)). `--repeat` runs each
(5), median and range:

  * the two row passes and the host's chain of decisions between them, in the library (kmahip_test_index_hom_timing: the host's
    clock around each step, which ends with a copy to the host);
  * the whole process `kmahip_index -Sparse TG -hq 0.9 -ht 0.9 -and` against `oracle/_ref/kma index` with the same options;
  * `kmahip_index -Sparse TG` without the options against the same program of another build (`--parent <its examples/kmahip_index>`,
    e.g. the parent commit's, built in a checkout of its own), alternating so that both see the same machine.

It also checks what was timed: the report and the index equal the reference's. Writes one JSON document (`--out`).

    python tools/homology_time.py [--parent /path/to/parent/examples/kmahip_index] [--dir /tmp/homology_time] [--out profiles/homology_time.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kma_amd import binding, formats, synth  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
INDEX = os.path.join(ROOT, "examples", "kmahip_index")
OPTS = ["-hq", "0.9", "-ht", "0.9", "-and"]
SHAPES = {"redundant": (50, 100, 500, 1300, 0.02), "genes": (1667, 3, 500, 1300, 0.2)}


def wall(cmd, stdout=subprocess.DEVNULL):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=stdout, stderr=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    if p.returncode not in (0, 2):          # (the reference ORs errno into its exit status, kma.c:1630)
        raise SystemExit("%s -> %d" % (" ".join(cmd), p.returncode))
    return dt, p.stdout


def stats(xs, unit="s", digits=3):
    return {"median_" + unit: round(statistics.median(xs), digits), "min_" + unit: round(min(xs), digits), "max_" + unit: round(max(xs), digits),
            "all_" + unit: [round(x, digits) for x in xs]}


def overlap(a, b):
    return a["min_s"] <= b["max_s"] and b["min_s"] <= a["max_s"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dbs", default="redundant,genes")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent", default=None, help="examples/kmahip_index of the build to compare the build without the options with")
    ap.add_argument("--dir", default="/tmp/homology_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homology_time.json"))
    a = ap.parse_args()
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing")
    os.makedirs(a.dir, exist_ok=True)
    L = binding.lib()
    L.kmahip_test_index_hom_timing.argtypes = [C.POINTER(C.c_double)]
    res = dict(options=" ".join(["-Sparse", "TG"] + OPTS), repeat=a.repeat)
    for db in a.dbs.split(","):
        P = lambda x: os.path.join(a.dir, db + "_" + x)
        fa = P("db.fsa")
        names, seqs = synth.make_gene_db(*SHAPES[db], seed=7)
        synth.write_fasta(fa, names, seqs)
        r = dict(templates=len(seqs), bases=int(sum(len(s) for s in seqs)))
        # one run of each that is not kept: the page cache, and the device's first start in this session
        wall([INDEX, "-i", fa, "-o", P("ours"), "-Sparse", "TG"] + OPTS)
        wall([INDEX, "-i", fa, "-o", P("plain"), "-Sparse", "TG"])
        binding.index_build(fa, P("lib"), sparse="TG", hom_q=0.9, hom_t=0.9, hom_and=True, report=P("lib.tsv"))
        p1, host, p2, lib = [], [], [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            binding.index_build(fa, P("lib"), sparse="TG", hom_q=0.9, hom_t=0.9, hom_and=True, report=P("lib.tsv"))
            lib.append(time.perf_counter() - t0)
            ms = (C.c_double * 4)()
            L.kmahip_test_index_hom_timing(ms)
            p1.append(ms[0]); host.append(ms[1]); p2.append(ms[2])
            r["pairs_listed"] = int(ms[3])
        r["pass1"], r["resolve_on_host"], r["pass2"] = stats(p1, "ms"), stats(host, "ms"), stats(p2, "ms")
        r["library_call"] = stats(lib)
        ours, ref = [], []
        for _ in range(a.repeat):
            dt, mine = wall([INDEX, "-i", fa, "-o", P("ours"), "-Sparse", "TG"] + OPTS, stdout=subprocess.PIPE)
            ours.append(dt)
            dt, theirs = wall([KMA, "index", "-i", fa, "-o", P("ref"), "-Sparse", "TG"] + OPTS, stdout=subprocess.PIPE)
            ref.append(dt)
        r["kmahip_index_hom"], r["kma_index_hom"] = stats(ours), stats(ref)
        r["kma_over_kmahip_of_medians"] = round(statistics.median(ref) / statistics.median(ours), 2)
        plain, parent = [], []
        for _ in range(a.repeat):
            plain.append(wall([INDEX, "-i", fa, "-o", P("plain"), "-Sparse", "TG"])[0])
            if a.parent:
                parent.append(wall([a.parent, "-i", fa, "-o", P("parent"), "-Sparse", "TG"])[0])
        r["kmahip_index_sparse_without_the_options"] = stats(plain)
        if a.parent:
            r["parent_kmahip_index_sparse"] = stats(parent)
            r["ranges_overlap"] = overlap(r["kmahip_index_sparse_without_the_options"], r["parent_kmahip_index_sparse"])
            r["files_identical_to_parent"] = all(open(P("plain") + e, "rb").read() == open(P("parent") + e, "rb").read() for e in (".comp.b", ".length.b", ".seq.b", ".name"))
        # what was timed is the reference's answer
        x, y = formats.read_comp_b(P("ours.comp.b")), formats.read_comp_b(P("ref.comp.b"))
        r["templates_kept"] = int(x.DB_size) - 1
        r["report_lines"] = mine.count(b"\n")
        r["report_identical"] = mine == theirs and open(P("lib.tsv"), "rb").read() == theirs
        r["index_equal"] = bool((x.DB_size, x.n, x.prefix, x.prefix_len, x.v_index) == (y.DB_size, y.n, y.prefix, y.prefix_len, y.v_index) and
                                formats.comp_db_mapping(x) == formats.comp_db_mapping(y) and
                                all(open(P("ours") + e, "rb").read() == open(P("ref") + e, "rb").read() for e in (".length.b", ".name")))
        res[db] = r
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
