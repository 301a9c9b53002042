"""Records tests/golden/tdist/: hand-made FASTA, the reference's index files of them (`kma index`) and its distance files (`kma dist`).
Needs the compiled reference (oracle/_ref/kma). Every property a case is there for is asserted on the reference's own files.

    python tests/golden/make_golden_dist.py
"""
import gzip
import json
import lzma
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dist_util as du          # noqa: E402


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def edge():
    """72 templates. Blocks of 40 bases shared by 65, 64 and 63 of them (a list that long, pointed to by the 25 k-mers inside the
    block; their junctions add lists that one k-mer uses), a block in two templates, two identical templates under different
    names, one template that shares nothing with anyone; names shorter than, as long as and longer than 10 bytes"""
    rng = random.Random(20200101)
    B65, B64, B63, B2, same = (rnd(rng, 40) for _ in range(5))
    out = []
    for i in range(1, 73):
        s = rnd(rng, 36)
        if i <= 65:
            s += B65
        if 3 <= i <= 66:
            s += B64
        if 5 <= i <= 67:
            s += B63
        if i in (68, 69):
            s += B2
        if i in (70, 71):
            s = same
        name = ("s%d" % i) if i % 3 == 0 else ("name10_%03d" % i) if i % 3 == 1 else ("a_long_template_name_%d with a description" % i)
        out.append((name, s))
    return out


def wide():
    """330 templates, 300 of them with the same window of 40 bases: a list of 300, beyond a wavefront and a tile"""
    rng = random.Random(20200102)
    W, X = rnd(rng, 40), rnd(rng, 40)
    return [("w%d" % i, rnd(rng, 30) + (W if i <= 300 else X if i <= 310 else "")) for i in range(1, 331)]


def one():
    return [("only_one", rnd(random.Random(3), 60))]


def two():
    rng = random.Random(4)
    B = rnd(rng, 30)
    return [("first", rnd(rng, 30) + B), ("the second template", B + rnd(rng, 25))]


FASTA = {"edge": edge, "wide": wide, "one": one, "two": two}


def check(case, v, N, D):
    lists = v.lists()
    lens = {len(ids) for ids, _ in lists.values()}
    mults = [m for _, m in lists.values()]
    n = v.DB_size - 1
    if case.startswith("edge"):          # (a sparse index keeps no template without a window)
        assert 60 <= n <= 72 and max(lens) >= 60
    if case == "edge":
        assert n == 72
        assert {1, 2, 63, 64, 65} <= lens, sorted(lens)
        assert max(mults) >= 10 and 1 in mults
        assert N[69] == N[70] == D[70, 69] > 0                          # two identical templates
        assert D[71, :].sum() == 0 and N[71] > 0                          # one that shares nothing
        assert D[68, 67] > 0 and D[67, :67].sum() == 0
        assert {len(x) < 10 for x in v.names} == {True, False} and any(len(x) == 10 for x in v.names)
        assert (v.mlen, v.prefix_len, v.flag, v.mega) == (16, 0, 0, False)
    if case == "edge_k20":
        assert v.mlen == 20 and not v.mega
    if case == "edge_TG":
        assert v.prefix_len == 2 and v.mlen == 16 and not v.mega
    if case == "edge_m12":
        assert v.flag != 0, "no minimizer flag"
    if case == "edge_mega":
        assert v.mega and v.size == 4 ** 10
    if case == "wide":
        assert n == 330 and 300 in lens and (D[299, :299] > 0).all()
    if case == "one":
        assert n == 1
    if case == "two":
        assert n == 2 and D[1, 0] > 0


def main():
    assert os.path.exists(du.KMA), "build the reference first (oracle/Makefile, target ref)"
    os.makedirs(du.GOLDEN, exist_ok=True)
    for name, make in FASTA.items():
        with gzip.GzipFile(os.path.join(du.GOLDEN, name + ".fsa.gz"), "wb", mtime=0) as f:
            f.write("".join(">%s\n%s\n" % r for r in make()).encode())
    quiet = dict(stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for case, (fasta, index_args, runs) in du.CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "in.fsa")
            with open(fa, "wb") as f:
                f.write(gzip.open(os.path.join(du.GOLDEN, fasta + ".fsa.gz")).read())
            db = os.path.join(tmp, "td_" + case)
            subprocess.run([du.KMA, "index", "-i", fa, "-o", db] + index_args, check=True, **quiet)
            with open(db + ".comp.b", "rb") as f, lzma.open(os.path.join(du.GOLDEN, case + ".comp.b.xz"), "wb", preset=9) as g:
                g.write(f.read())
            with open(db + ".name", "rb") as f, open(os.path.join(du.GOLDEN, case + ".name"), "wb") as g:
                g.write(f.read())
            v = du.Values(db)
            N, D = du.counts(v.lists(), v.DB_size - 1)
            check(case, v, N, D)
            for tag, args in runs.items():
                out = os.path.join(tmp, tag + ".phy")
                subprocess.run([du.KMA, "dist", "-t_db", db, "-o", out] + args, check=True, **quiet)
                raw = open(out, "rb").read()
                methods, fmt = du.run_flags(args)
                assert len(raw) == du.phy_size(v.DB_size, os.path.getsize(db + ".name"), methods, fmt), (case, tag)
                if not fmt & 1:
                    assert raw.endswith(b"\n" + b"\0" * 11), (case, tag)
                with lzma.open(os.path.join(du.GOLDEN, "%s.%s.phy.xz" % (case, tag)), "wb", preset=9) as g:
                    g.write(raw)
            print(case, "n", v.DB_size - 1, "k-mers", v.n, "lists", len(v.lists()), "sum N", int(np.sum(N)))
    # the command line: texts and statuses of the runs that end before an index is read
    cli = []
    for args in du.CLI_CASES:
        p = subprocess.run([du.KMA, "dist"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        cli.append({"args": args, "status": p.returncode, "stdout": p.stdout.decode(), "stderr": p.stderr.decode()})
        assert p.returncode in (0, 1) and (p.stdout or p.stderr), args
    with open(os.path.join(du.GOLDEN, "cli.json"), "w") as f:
        json.dump(cli, f, indent=1, ensure_ascii=False)
        f.write("\n")


if __name__ == "__main__":
    main()
