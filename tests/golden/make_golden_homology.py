#!/usr/bin/env python3
"""Fixtures of homology reduction (`kma index -Sparse ... -hq x -ht y [-and]`) under tests/golden/homology/, made by oracle/_ref/kma.
Only data is stored: one hand-made FASTA file (db.fsa.gz) and, for every case of tests/hom_util.CASES, what the reference printed to
standard output (<case>.report.tsv) and its index (.comp.b as .xz, .length.b, .name, .seq.b).

The FASTA file holds some forty templates of 17-900 bases: unrelated genes, families of variants, chimeras, copies, a chain of
near-copies, templates with N's and templates that hold no window. Each edge they are made for is asserted on the reference's own
output further down; the script ends with an error when one does not occur."""
import gzip
import lzma
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hom_util as hu  # noqa: E402
import sparse_index_util as siu  # noqa: E402

LIMIT = 350_000          # bytes a stored file may have
K = 16
_COMP = str.maketrans("ACGT", "TGCA")


def need(cond, what):
    if not cond:
        raise SystemExit("edge not met on the reference's output: " + what)
    print("  ok: " + what)


def put(data, dst):
    with open(dst, "wb") as f:
        f.write(data)
    if os.path.getsize(dst) > LIMIT:
        raise SystemExit("%s: %d bytes" % (dst, os.path.getsize(dst)))


def templates(seed=20262):
    rng = np.random.default_rng(seed)
    acgt = lambda n: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))
    ag = lambda n: "".join("AG"[int(x)] for x in rng.integers(0, 2, n))

    def subs(seq, positions):
        s = list(seq)
        for p in positions:
            s[int(p)] = "ACGT"[("ACGT".index(s[int(p)]) + 1 + int(rng.integers(0, 3))) % 4]
        return "".join(s)

    def variant(seq, frac):
        return subs(seq, rng.choice(len(seq), max(1, int(round(frac * len(seq)))), replace=False))

    A, B = acgt(600), acgt(600)
    S = acgt(200)
    X = acgt(600)
    Y = subs(X, range(8, 200, 19))          # ten changes in the first third: thisQ against X near 0.73
    Z = subs(Y, range(208, 400, 19))        # ten more in the second: near 0.73 against Y, near 0.45 against X
    G, M = acgt(900), acgt(200)
    f1, f2, f3 = acgt(500), acgt(800), acgt(300)
    s1 = acgt(250)
    tg = [i for i in range(60, 440) if f1[i:i + 2] == "TG"]
    with_n = list(f1)
    with_n[tg[0] + 2] = "N"                 # right behind a prefix
    with_n[tg[len(tg) // 2]] = "N"          # the prefix's first base
    with_n[tg[-1] + 1] = "N"                # the prefix's second base
    recs = [   # (header, sequence as written, line width or 0)
        ("gene_A", A, 60),
        ("gene_B some description", B, 60),
        ("chimera_A_then_B", A[:300] + "N" + B[300:], 70),
        ("chimera_B_then_A", B[:300] + "N" + A[300:], 70),
        ("holds_S_first", acgt(200) + S + acgt(200), 0),
        ("holds_S_second", acgt(150) + S + acgt(250), 0),
        ("read_of_S", S, 0),
        ("copy_of_A", A, 0),
        ("revcomp_of_A", A.translate(_COMP)[::-1], 0),
        ("chain_X", X, 80),
        ("chain_Y", Y, 80),
        ("chain_Z", Z, 80),
        ("long_G", G, 60),
        ("short_M", M, 60),
        ("half_G_most_of_M", G[:500] + M[:150], 0),
        ("copy_of_A_with_one_N", A[:300] + "N" + A[301:], 0),
        ("fam1", f1, 0), ("fam1_v1", variant(f1, 0.01), 0), ("fam1_v3", variant(f1, 0.03), 0), ("fam1_v8", variant(f1, 0.08), 0),
        ("fam1_v20", variant(f1, 0.20), 0),
        ("fam2", f2, 100), ("fam2_v2", variant(f2, 0.02), 100), ("fam2_v5", variant(f2, 0.05), 100), ("fam2_v12", variant(f2, 0.12), 100),
        ("fam3", f3, 0), ("fam3_v1", variant(f3, 0.01), 0), ("fam3_v10", variant(f3, 0.10), 0),
        ("fam1_n_at_prefixes", "".join(with_n), 0),
        ("no_TG_window", ag(250), 0),
        ("no_window_at_all", ("ACGTACGTACGTAC" + "N") * 15, 0),
        ("k_plus_one_bases", "TG" + ag(15), 0),
        ("trailing_blanks_in_header  ", acgt(220), 0),
        ("leading_n", "NNN" + acgt(300) + "NN", 0),
        ("below_ml", s1, 0),
        ("below_ml_v2", variant(s1, 0.02), 0),
        ("below_ml_extended", s1 + acgt(150), 0),
        ("lone_350", acgt(350), 50),
        ("lone_201_lower", acgt(201).lower(), 67),
        ("fam2_v5_again", variant(f2, 0.05), 100),
    ]
    return recs, dict(X=X, Y=Y, Z=Z)


def fasta(recs):
    out = []
    for head, seq, width in recs:
        out.append(">" + head + "\n")
        w = width or len(seq)
        out += [seq[a:a + w] + "\n" for a in range(0, len(seq), w)]
    return "".join(out).encode()


def this_q(new, old, k, text):
    """thisQ of `new` against a database that holds `old` alone"""
    have = set(siu.windows(old, k, text))
    ws = siu.windows(new, k, text)
    return sum(w in have for w in ws) / len(ws)


def index(tmp, fa, case):
    db = os.path.join(tmp, case)
    p = subprocess.run([hu.KMA, "index", "-i", fa, "-o", db] + hu.kma_args(case), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode:
        raise SystemExit("kma index %s -> %d\n%s" % (case, p.returncode, p.stderr.decode()))
    return db, p.stdout


def check_edges(got, seqs):
    rep = {c: hu.parse_report(got[c][1]) for c in got}
    names = {c: [None] + got[c][0].name_file.decode().split("\n")[:-1] for c in got}
    at = {c: {n: i for i, n in enumerate(names[c]) if n} for c in got}
    for sp in ("none", "TG"):
        r6, a6 = rep[sp + "_hq06"], at[sp + "_hq06"]
        need(r6["copy_of_A"] == [a6["gene_A"], 1.0, a6["gene_A"]] and r6["revcomp_of_A"] == [a6["gene_A"], 1.0, a6["gene_A"]],
             sp + ": a copy and a reverse complement of A go at 1.000000 and name A")
        need(r6["read_of_S"][1:] == [1.0, a6["holds_S_first"]] and "holds_S_second" in a6 and a6["holds_S_second"] == a6["holds_S_first"] + 1,
             sp + ": a read of the segment two kept templates share names the lower id")
        need("chain_Y" not in a6 and r6["chain_Y"][2] == a6["chain_X"] and "chain_Z" in a6 and r6["chain_Z"][2] == a6["chain_X"],
             sp + ": of the chain X, Y, Z the middle one goes and the last one stays")
        text = "" if sp == "none" else "TG"
        need(this_q(seqs["Z"], seqs["Y"], K, text) >= 0.6 > this_q(seqs["Z"], seqs["X"], K, text), sp + ": ... only because Y is absent")
        fam = [n for n in r6 if n.startswith("fam")]
        need(any(n in a6 for n in fam if "_v" in n) and any(n not in a6 for n in fam), sp + ": variants on both sides of -hq 0.6")
        r8 = rep[sp + "_ht08_hq08"]
        need(len(r8["gene_A"]) == 5 and len(r6["gene_A"]) == 3, sp + ": six fields under templateCheck, four under queryCheck")
        need(r8["half_G_most_of_M"][2] != r8["half_G_most_of_M"][4] and 0 not in r8["half_G_most_of_M"][1:], sp + ": bestQ and bestT name different templates")
        need("fam1_n_at_prefixes" in r6, sp + ": N's in and next to a prefix")
        need("no_window_at_all" not in r6 and "no_window_at_all" not in a6, sp + ": a template without a window has no line and no id")
        need("leading_n" in r6 and "leading_n B3" in a6, sp + ": leading N's: B3 in the name file, not in the report")
        need("trailing_blanks_in_header" in r6, sp + ": a header loses its trailing blanks")
        for c in got:
            if c.startswith(sp):
                need(rep[c]["gene_A"][0] == 1 and not any(rep[c]["gene_A"][1:]) and rep[c]["gene_B some description"][0] == 2, c + ": the first templates meet nothing")
    n6, an6, n5, an5 = rep["none_hq06"], at["none_hq06"], rep["none_hq05"], at["none_hq05"]
    need(got["none_hq06"][1].count(b"\t0.500000\t") >= 2 and n6["chimera_A_then_B"][1:] == [0.5, an6["gene_A"]] and n6["chimera_B_then_A"][1:] == [0.5, an6["gene_B some description"]],
         "both chimeras tie at exactly 0.500000 and name the half met first")
    need("chimera_A_then_B" in an6 and "chimera_A_then_B" not in an5 and n5["chimera_A_then_B"] == [an5["gene_A"], 0.5, an5["gene_A"]],
         "-hq 0.5 rejects a bestQ of exactly 0.5 that -hq 0.6 lets pass")
    need(b"copy_of_A_with_one_N\t1\t1.000000\t1\t0.972650\t1\n" in got["none_ht09"][1], "a copy with one N: bestT 0.972650 beside bestQ 1.000000")
    t6, t5 = rep["TG_hq06"], rep["TG_hq05"]
    need("no_TG_window" not in t6 and "no_TG_window" in n6 and "k_plus_one_bases" not in t6 and "k_plus_one_bases" in n6,
         "no window behind the prefix, and k + 1 bases: a line without a prefix, none with it")
    need(at["TG_hq06"] != at["TG_hq05"] and at["TG_ht045_hq045_and"] != at["TG_ht08_hq08"], "the settings keep different templates")
    ml, aml = rep["TG_hq06_ML300"], at["TG_hq06_ML300"]
    need("below_ml" not in ml and "below_ml" in at["TG_hq06"] and "below_ml_extended" not in at["TG_hq06"] and "below_ml_extended" in aml,
         "-ML 300: a template stays that the plain case rejects for one that -ML skips")
    need(rep["k12_TG_hq06"] != t6, "-k 12 gives other ratios")
    need(all(len(v) == 5 for v in rep["TG_ht09"].values()) and at["TG_ht09"] != at["TG_ht08_hq08"], "-ht alone")


def main():
    if not os.path.exists(hu.KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    out = hu.GOLDEN
    os.makedirs(out, exist_ok=True)
    recs, seqs = templates()
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "db.fsa")
        put(fasta(recs), fa)
        with gzip.GzipFile(hu.INPUT, "wb", mtime=0) as g:
            g.write(fasta(recs))
        got = {}
        for case in hu.CASES:
            db, text = index(tmp, fa, case)
            got[case] = (siu.Files(db), text)
            print("%s: DB_size %d, %d k-mers, %d lines" % (case, got[case][0].DB_size, got[case][0].n, text.count(b"\n")))
        check_edges(got, seqs)
        for case in hu.CASES:
            db = os.path.join(tmp, case)
            put(got[case][1], os.path.join(out, case + ".report.tsv"))
            put(lzma.compress(open(db + ".comp.b", "rb").read(), preset=9), os.path.join(out, case + ".comp.b.xz"))
            for ext in (".length.b", ".name", ".seq.b"):
                shutil.copy(db + ext, os.path.join(out, case + ext))
            mine = hu.built(case, fa)
            need(mine.report == got[case][1] and mine.length_b() == got[case][0].length_b and mine.name_file() == got[case][0].name_file and mine.lists == got[case][0].lists,
                 case + ": the restatement of tests/hom_util.py gives the reference's report and index")
    print("homology fixtures written: %d bytes" % sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)))


if __name__ == "__main__":
    main()
