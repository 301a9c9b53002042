#!/usr/bin/env python3
"""Fixtures of sparse mapping (`kma index -Sparse`, `kma -Sparse`) under tests/golden/sparse/, made by oracle/_ref/kma. Only data is
stored: FASTA / FASTQ inputs, the reference's index files (.comp.b as .xz, .length.b, .name; a sparse run reads no .seq.b), its `.spa`
files for -ss q, c and d, its k-mer tap (`kma ... -Sparse -s1`, 8 bytes per k-mer; stored sorted, which keeps the multiset and lets it
compress) and its `# Total number of matches: X of Y kmers` line. For se/TG and w also the `.spa` of `-ID 99.5`, `-md 2`, `-md 15`
and `-e 1e-30` (-md 2 leaves both files as they are: every row's depth is above 12; -md 15 is the depth gate that bites).

  se  tests/golden/se's database (67 templates) and reads (1500 reads of 15-257 bases, 133 with an N), indexed three times:
      `-Sparse TG`, `-Sparse -` (no prefix: files named `none`) and `-Sparse ATG`.
  w   "withdrawal": 12 families of 3 variants at 20 % divergence, 3000 reads, prefix TG. Checked here on the reference's own output: at
      least a quarter of the rows have Query_Coverage != tot_query_Coverage -- the rows the withdrawal of an earlier template changed.
  e   "edges": a hand-made FASTQ and a FASTA file against a small database: read lengths k - 1, k, k + prefix_len, k + prefix_len + 1
      (the strict gate), 33, 64, 65; an N at the first base, at the last, right behind a prefix, two N's closer than k; a prefix whose
      k-mer would run past its stretch; one k-mer twice in a read and once more as its reverse complement; a palindromic k-mer."""
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kma_amd import synth  # noqa: E402
import proxi_util  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
K = 16
LIMIT = 350_000          # bytes: no fixture above the largest there was before


def run(cmd, **kw):
    # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
    p = subprocess.run(cmd, stdout=kw.get("stdout", subprocess.DEVNULL), stderr=kw.get("stderr", subprocess.DEVNULL))
    if p.returncode not in (0, 2):
        raise SystemExit("%s -> %d" % (" ".join(cmd), p.returncode))
    return p


def put(data, dst):
    with open(dst, "wb") as f:
        f.write(data)
    if os.path.getsize(dst) > LIMIT:
        raise SystemExit("%s: %d bytes" % (dst, os.path.getsize(dst)))


def put_gz(data, dst):
    with gzip.GzipFile(dst, "wb", mtime=0) as g:
        g.write(data)
    if os.path.getsize(dst) > LIMIT:
        raise SystemExit("%s: %d bytes" % (dst, os.path.getsize(dst)))


VARIANTS = (("ID99.5", ["-ID", "99.5"]), ("md2", ["-md", "2"]), ("md15", ["-md", "15"]), ("e1e-30", ["-e", "1e-30"]))


def store_case(outdir, name, tmp, fa, inputs, sparse_arg, variants=()):
    """index fa with `-Sparse sparse_arg`, map `inputs`, store everything of index `name` -> {ss: spa text}"""
    db = os.path.join(tmp, "idx_" + name)
    run([KMA, "index", "-i", fa, "-o", db, "-k", str(K), "-Sparse", sparse_arg])
    put(lzma.compress(open(db + ".comp.b", "rb").read(), preset=9), os.path.join(outdir, name + ".comp.b.xz"))
    for ext in (".length.b", ".name"):
        shutil.copy(db + ext, os.path.join(outdir, name + ext))
    out = os.path.join(tmp, "out_" + name)
    base = [KMA, "-i"] + inputs + ["-o", out, "-t_db", db, "-Sparse", "-t", "1"]
    spa = {}
    for ss in "qcd":
        p = run(base + ["-ss", ss], stderr=subprocess.PIPE)
        spa[ss] = open(out + ".spa").read()
        put(spa[ss].encode(), os.path.join(outdir, "%s.%s.spa" % (name, ss)))
        line = [x for x in p.stderr.decode().split("\n") if x.startswith("# Total number of matches")]
        assert len(line) == 1
        matches = line[0] + "\n"
    put(matches.encode(), os.path.join(outdir, name + ".matches.txt"))
    for tag, extra in variants:          # the gates off their defaults, -ss q
        run(base + extra)
        text = open(out + ".spa").read()
        print("%s/%s %s: %d rows, %s" % (os.path.basename(outdir), name, " ".join(extra), len(text.split("\n")) - 2, "as without" if text == spa["q"] else "changed"))
        put(text.encode(), os.path.join(outdir, "%s.%s.spa" % (name, tag)))
    tap = np.frombuffer(run(base + ["-s1"], stdout=subprocess.PIPE).stdout, np.uint64)
    put(lzma.compress(np.sort(tap).tobytes(), preset=9), os.path.join(outdir, name + ".kmers.bin.xz"))
    print("%s/%s: %s %d k-mers in the tap, rows q/c/d %s" % (os.path.basename(outdir), name, matches.strip(), len(tap),
                                                             "/".join(str(len(spa[s].split("\n")) - 2) for s in "qcd")))
    return spa


def gunzip_to(src, dst):
    with gzip.open(src, "rb") as f, open(dst, "wb") as g:
        g.write(f.read())


def make_se(outdir):
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        fa, fq = os.path.join(tmp, "db.fsa"), os.path.join(tmp, "reads.fq")
        gunzip_to(os.path.join(HERE, "se", "db.fsa.gz"), fa)
        gunzip_to(os.path.join(HERE, "se", "reads.fq.gz"), fq)
        shutil.copy(os.path.join(HERE, "se", "reads.fq.gz"), os.path.join(outdir, "reads.fq.gz"))
        for name, arg in (("TG", "TG"), ("none", "-"), ("ATG", "ATG")):
            store_case(outdir, name, tmp, fa, [fq], arg, VARIANTS if name == "TG" else ())


def changed_rows(spa):
    rows = [x.split("\t") for x in spa.split("\n")[1:] if x]
    return sum(1 for r in rows if r[5] != r[8]), len(rows)


def make_w(outdir, seed=7):
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        names, seqs = synth.make_gene_db(12, 3, 500, 1300, 0.2, seed=seed)
        fa, fq = os.path.join(tmp, "db.fsa"), os.path.join(tmp, "reads.fq")
        synth.write_fasta(fa, names, seqs)
        synth.write_fastq(fq, proxi_util.reads(seqs, 3000, np.random.default_rng(seed)), lens=None)
        spa = store_case(outdir, "TG", tmp, fa, [fq], "TG", VARIANTS)
        for ss in "qc":
            ch, n = changed_rows(spa[ss])
            print("w -ss %s: %d of %d rows changed by a withdrawal" % (ss, ch, n))
            if 4 * ch < n:
                raise SystemExit("w: fewer than a quarter of the rows changed; search another seed")
        put_gz(open(fq, "rb").read(), os.path.join(outdir, "reads.fq.gz"))


def make_e(outdir, seed=4501):
    os.makedirs(outdir, exist_ok=True)
    rng = np.random.default_rng(seed)
    B = synth.BASES
    txt = lambda s: B[np.asarray(s, np.uint8)].tobytes().decode()
    rc = lambda s: s.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    with tempfile.TemporaryDirectory() as tmp:
        names, seqs = synth.make_gene_db(3, 3, 200, 300, 0.03, seed)
        # a template with a palindromic k-mer behind a prefix, and a prefix behind it on the other strand
        pal = "ACGTACGTACGTACGT"
        assert rc(pal) == pal
        code = {c: i for i, c in enumerate("ACGT")}
        custom = txt(rng.integers(0, 4, 90)) + "TG" + pal + "CA" + txt(rng.integers(0, 4, 90))
        names = list(names) + ["palindrome"]
        seqs = list(seqs) + [np.array([code[c] for c in custom], np.uint8)]
        fa = os.path.join(tmp, "db.fsa")
        synth.write_fasta(fa, names, seqs)
        s = txt(seqs[0])
        tg = [i for i in range(40, len(s) - 80) if s[i:i + 2] == "TG"]
        a, b = tg[0], tg[len(tg) // 2]
        piece = s[b:b + 2 + K]
        t = txt(seqs[4])
        two_n = list(t[20:120]); two_n[30] = "N"; two_n[38] = "N"
        recs = [
            ("len_k_minus_1", s[a:a + K - 1]),
            ("len_k", s[a:a + K]),
            ("len_k_plus_p", s[a:a + K + 2]),
            ("len_k_plus_p_plus_1", s[a:a + K + 3]),
            ("len_33", s[a:a + 33]),
            ("len_64", s[a:a + 64]),
            ("len_65", s[a:a + 65]),
            ("n_first", "N" + s[a:a + 50]),
            ("n_last", s[a:a + 50] + "N"),
            ("n_behind_prefix", s[a:a + 2] + "N" + s[a + 3:a + 60]),
            ("two_n_closer_than_k", "".join(two_n)),
            ("prefix_at_the_end_of_a_stretch", s[a - 30:a + 10]),
            ("prefix_before_an_n", s[a - 30:a + 10] + "N" + s[a + 11:a + 50]),
            ("twice_and_reverse", piece + "A" + piece + "C" + rc(piece) + s[5:30]),
            ("palindrome", custom[70:130]),
            ("whole_template", txt(seqs[2])),
            ("whole_template_rc", rc(txt(seqs[7]))),
            ("lower_case", s[a:a + 60].lower()),
            ("no_match", txt(rng.integers(0, 4, 80))),
        ]
        fq = os.path.join(tmp, "reads.fq")
        with open(fq, "w") as f:
            for n, q in recs:
                f.write("@%s\n%s\n+\n%s\n" % (n, q, "I" * len(q)))
        u = txt(seqs[5])
        fsa = os.path.join(tmp, "reads.fsa")
        with open(fsa, "w") as f:
            f.write(">fasta_two_lines\n%s\n%s\n" % (u[10:60], u[60:100]))
            f.write(">fasta_n_at_both_ends\nNN%sN\n" % u[100:160])
            f.write(">fasta_n_inside\n%sN%s\n" % (u[20:50], u[51:110]))
        store_case(outdir, "TG", tmp, fa, [fq, fsa], "TG")
        put_gz(open(fa, "rb").read(), os.path.join(outdir, "db.fsa.gz"))
        put_gz(open(fq, "rb").read(), os.path.join(outdir, "reads.fq.gz"))
        put_gz(open(fsa, "rb").read(), os.path.join(outdir, "reads.fsa.gz"))


if __name__ == "__main__":
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    out = os.path.join(HERE, "sparse")
    make_se(os.path.join(out, "se"))
    make_w(os.path.join(out, "w"))
    make_e(os.path.join(out, "e"))
    print("sparse fixtures written")
