#!/usr/bin/env python3
"""Times of sparse index building, on the database tools/sparse_time.py makes (synth.make_gene_db(1667, 3, 500, 1300,
0.2): 5 001 templates) and its reads. Whole processes, `--repeat` runs each (5), median and range:

  * `kmahip_index -Sparse TG` against `oracle/_ref/kma index -Sparse TG` on the same host and file;
  * plain `kmahip_index` of this tree against the one of another build (`--parent <its examples/kmahip_index>`, e.g. the parent
    commit's, built in a checkout of its own), alternating so that both see the same machine.

It also checks what was timed: our sparse index holds the reference's mapping, .length.b and .name, and `kmahip_map -Sparse` writes the
same `.spa` from either index (`--reads`, 0 to leave the mapping out). Prints one JSON line.

    python tools/sparse_index_time.py [--parent /path/to/parent/examples/kmahip_index] [--reads 1000000] [--dir /tmp/sparse_index_time]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kma_amd import formats, synth  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
INDEX = os.path.join(ROOT, "examples", "kmahip_index")
MAP = os.path.join(ROOT, "examples", "kmahip_map")


def wall(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    if p.returncode not in (0, 2):          # (the reference ORs errno into its exit status, kma.c:1630)
        raise SystemExit("%s -> %d" % (" ".join(cmd), p.returncode))
    return dt


def stats(xs):
    return dict(median_s=round(statistics.median(xs), 3), min_s=round(min(xs), 3), max_s=round(max(xs), 3), all_s=[round(x, 3) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=1667)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent", default=None, help="examples/kmahip_index of the build to compare the plain index build with")
    ap.add_argument("--dir", default="/tmp/sparse_index_time")
    a = ap.parse_args()
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing")
    os.makedirs(a.dir, exist_ok=True)
    fa, fq = os.path.join(a.dir, "db.fsa"), os.path.join(a.dir, "reads.fq")
    names, seqs = synth.make_gene_db(a.families, 3, 500, 1300, 0.2, seed=7)
    synth.write_fasta(fa, names, seqs)
    P = lambda x: os.path.join(a.dir, x)
    res = dict(templates=len(seqs), bases=int(sum(len(s) for s in seqs)), repeat=a.repeat)
    # one run of each that is not kept: the page cache, and the device's first start in this session
    for cmd in ([INDEX, "-i", fa, "-o", P("ours"), "-Sparse", "TG"], [INDEX, "-i", fa, "-o", P("plain")]):
        wall(cmd)
    ours, ref = [], []
    for _ in range(a.repeat):
        ours.append(wall([INDEX, "-i", fa, "-o", P("ours"), "-Sparse", "TG"]))
        ref.append(wall([KMA, "index", "-i", fa, "-o", P("ref"), "-Sparse", "TG"]))
    res["kmahip_index_sparse"], res["kma_index_sparse"] = stats(ours), stats(ref)
    res["sparse_speedup_of_medians"] = round(statistics.median(ref) / statistics.median(ours), 2)
    plain, parent = [], []
    for _ in range(a.repeat):
        plain.append(wall([INDEX, "-i", fa, "-o", P("plain")]))
        if a.parent:
            parent.append(wall([a.parent, "-i", fa, "-o", P("parent")]))
    res["kmahip_index_plain"] = stats(plain)
    if a.parent:
        res["parent_kmahip_index_plain"] = stats(parent)
        res["plain_files_identical_to_parent"] = all(open(P("plain") + e, "rb").read() == open(P("parent") + e, "rb").read() for e in (".comp.b", ".length.b", ".seq.b", ".name"))
    # what was timed is the reference's index
    x, y = formats.read_comp_b(P("ours.comp.b")), formats.read_comp_b(P("ref.comp.b"))
    res["index_kmers"] = int(x.n)
    res["sparse_index_equal"] = bool((x.DB_size, x.n, x.prefix, x.prefix_len, x.v_index) == (y.DB_size, y.n, y.prefix, y.prefix_len, y.v_index) and
                                     formats.comp_db_mapping(x) == formats.comp_db_mapping(y) and
                                     all(open(P("ours") + e, "rb").read() == open(P("ref") + e, "rb").read() for e in (".length.b", ".name")))
    if a.reads:
        reads, *_ = synth.make_reads(seqs, a.reads, read_len=150, sub_rate=0.005, n_rate=0.0002, seed=7)
        synth.write_fastq(fq, reads)
        del reads
        res["reads"] = a.reads
        res["map_on_ours_s"] = round(wall([MAP, "-i", fq, "-t_db", P("ours"), "-o", P("got_ours"), "-Sparse"]), 3)
        res["map_on_ref_s"] = round(wall([MAP, "-i", fq, "-t_db", P("ref"), "-o", P("got_ref"), "-Sparse"]), 3)
        res["spa_identical"] = open(P("got_ours.spa"), "rb").read() == open(P("got_ref.spa"), "rb").read()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
