#!/usr/bin/env python3
"""Times of appending to an index (`kmahip_index -t_db`), on the database tools/sparse_time.py makes
(synth.make_gene_db(1667, 3, 500, 1300, 0.2): 5 001 templates, 4.5 M bases): the last 100 templates are appended to an index of the
first 4 901. A warm-up that is not kept, then `--repeat` runs each (5), median and range:

  * the two expansion kernels and the scan on their own, by device events around the launches (kmahip_test_index_expand_timing);
  * whole processes, alternating on one host: `kmahip_index -t_db` against `oracle/_ref/kma index -t_db`, and against `kmahip_index -i
    all.fsa` of another build (`--parent <its examples/kmahip_index>`: the parent commit's, the only way to the same index before);
  * the same three on 65 530 templates of 40 bases plus 10 (the 16- to 32-bit crossing; a table of 1.6 M k-mers the reference rebuilds);
  * plain `kmahip_index` and `kmahip_index -Sparse TG` of this tree against the parent's: identical files, times side by side.

It checks what was timed: every pair holds the same index. Prints one JSON line and, with --out, writes it.

    python tools/index_append_time.py [--parent /path/to/parent/examples/kmahip_index] [--out profiles/index_append_time.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import index_append_util as iau  # noqa: E402
from kma_amd import binding, synth  # noqa: E402

KMA, INDEX = iau.KMA, iau.INDEX
EXTS = (".comp.b", ".length.b", ".seq.b", ".name")


def wall(cmd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    if p.returncode not in (0, 2):          # (the reference ORs errno into its exit status)
        raise SystemExit("%s -> %d" % (" ".join(cmd), p.returncode))
    return dt


def stats(xs, unit="s", digits=3):
    return {"median_" + unit: round(statistics.median(xs), digits), "min_" + unit: round(min(xs), digits), "max_" + unit: round(max(xs), digits),
            "all_" + unit: [round(x, digits) for x in xs]}


def same(a, b):
    A, B = iau.Comp(a + ".comp.b"), iau.Comp(b + ".comp.b")
    return bool(A.header() == B.header() and A.v_index == B.v_index and np.array_equal(iau.expand(A), iau.expand(B)) and
                all(open(a + e, "rb").read() == open(b + e, "rb").read() for e in (".length.b", ".name")))


def identical(a, b):
    return all(open(a + e, "rb").read() == open(b + e, "rb").read() for e in EXTS)


def leg(P, tag, fa_old, fa_new, fa_all, repeat, parent):
    """one database: old index by each builder, then the three ways to the appended index, alternating"""
    res = {}
    wall([INDEX, "-i", fa_old, "-o", P(tag + "_old")])
    wall([KMA, "index", "-i", fa_old, "-o", P(tag + "_rold")])
    cmds = {"kmahip_index_t_db": [INDEX, "-t_db", P(tag + "_old"), "-i", fa_new, "-o", P(tag + "_got")],
            "kma_index_t_db": [KMA, "index", "-t_db", P(tag + "_rold"), "-i", fa_new, "-o", P(tag + "_rgot")],
            "kmahip_index_fresh": [INDEX, "-i", fa_all, "-o", P(tag + "_full")]}
    if parent:
        cmds["parent_kmahip_index_fresh"] = [parent, "-i", fa_all, "-o", P(tag + "_pfull")]
    for cmd in cmds.values():
        wall(cmd)          # not kept: the page cache, the device's first start
    times = {k: [] for k in cmds}
    for _ in range(repeat):
        for k, cmd in cmds.items():
            times[k].append(wall(cmd))
    for k, xs in times.items():
        res[k] = stats(xs)
    res["append_equals_the_reference_append"] = same(P(tag + "_got"), P(tag + "_rgot"))
    res["append_identical_to_our_fresh_build"] = identical(P(tag + "_got"), P(tag + "_full"))
    if parent:
        res["fresh_build_identical_to_parent"] = identical(P(tag + "_full"), P(tag + "_pfull"))
    # the expansion on its own
    binding.index_expand(P(tag + "_old"))
    ev = []
    for _ in range(repeat):
        pairs = binding.index_expand(P(tag + "_old"))
        ev.append(binding.index_expand_timing())
    c = iau.Comp(P(tag + "_old") + ".comp.b")
    res["old_index"] = dict(kmers=int(c.n), pairs=int(len(pairs)), value_elements=int(c.v_index), list_bits=16 if c.values.dtype == np.uint16 else 32)
    for i, name in enumerate(("expand_count_kernel", "expand_scan", "expand_pairs_kernel")):
        res[name] = stats([e[i] for e in ev], unit="ms", digits=4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=1667)
    ap.add_argument("--new", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent", default=None, help="examples/kmahip_index of the parent commit's build")
    ap.add_argument("--dir", default="/tmp/index_append_time")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing")
    os.makedirs(a.dir, exist_ok=True)
    P = lambda x: os.path.join(a.dir, x)
    names, seqs = synth.make_gene_db(a.families, 3, 500, 1300, 0.2, seed=7)
    cut = len(seqs) - a.new
    synth.write_fasta(P("old.fsa"), names[:cut], seqs[:cut])
    synth.write_fasta(P("new.fsa"), names[cut:], seqs[cut:])
    synth.write_fasta(P("all.fsa"), names, seqs)
    res = dict(repeat=a.repeat, genes=dict(templates=len(seqs), appended=a.new, bases=int(sum(len(s) for s in seqs))))
    res["genes"].update(leg(P, "g", P("old.fsa"), P("new.fsa"), P("all.fsa"), a.repeat, a.parent))
    rng = np.random.default_rng(65530)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (65540, 40))]
    for path, lo, hi in ((P("w_old.fsa"), 0, 65530), (P("w_new.fsa"), 65530, 65540), (P("w_all.fsa"), 0, 65540)):
        with open(path, "wb") as f:
            f.write(b"".join(b">t%d\n%s\n" % (i, rows[i].tobytes()) for i in range(lo, hi)))
    res["width_crossing"] = dict(templates=65540, appended=10, bases=65540 * 40)
    res["width_crossing"].update(leg(P, "w", P("w_old.fsa"), P("w_new.fsa"), P("w_all.fsa"), a.repeat, a.parent))
    if a.parent:          # plain builds against the parent's program
        for tag, more in (("plain", []), ("sparse_TG", ["-Sparse", "TG"])):
            mine, theirs = [], []
            for cmd in ([INDEX, "-i", P("all.fsa"), "-o", P("p_mine")] + more, [a.parent, "-i", P("all.fsa"), "-o", P("p_parent")] + more):
                wall(cmd)
            for _ in range(a.repeat):
                mine.append(wall([INDEX, "-i", P("all.fsa"), "-o", P("p_mine")] + more))
                theirs.append(wall([a.parent, "-i", P("all.fsa"), "-o", P("p_parent")] + more))
            res["build_" + tag] = dict(this_tree=stats(mine), parent=stats(theirs), files_identical=identical(P("p_mine"), P("p_parent")))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
