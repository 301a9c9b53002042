#!/usr/bin/env python3
"""Fixtures of sparse index building (`kma index -Sparse`) under tests/golden/sparse_index/, made by oracle/_ref/kma. Only data is
stored: two hand-made FASTA files and, for every case of tests/sparse_index_util.CASES, the reference's index (.comp.b as .xz,
.length.b, .name, .seq.b) and the names on its `# Skipped:` lines.

The FASTA files hold a few dozen templates of 16-300 bases built around the prefix TG and k = 16. Stretches called `ag` below are
random A / G: neither they nor their reverse complement (T / C) hold a TG, so every window of the hand-made templates is one that was
put there. Each edge the templates are made for is asserted on the reference's own output further down; the script ends with an error
when one does not occur."""
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
import sparse_index_util as siu  # noqa: E402

LIMIT = 350_000          # bytes: no fixture above the largest there was before
K, PL = 16, 2
PAL = "ACGTACGTACGTACGT"


def need(cond, what):
    if not cond:
        raise SystemExit("edge not met on the reference's output: " + what)
    print("  ok: " + what)


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


def templates(seed=20261):
    rng = np.random.default_rng(seed)
    ag = lambda n: "".join("AG"[int(x)] for x in rng.integers(0, 2, n))
    acgt = lambda n: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))
    shared = "TG" + ag(K)
    twice = "TG" + ag(K)
    gene = acgt(240)
    variant = list(gene)
    for p in rng.integers(0, 240, 6):
        variant[int(p)] = "ACGT"[("ACGT".index(variant[int(p)]) + 1) % 4]
    one = [   # (header, sequence as written, line width or 0)
        ("random_300_wrapped", acgt(300), 60),
        ("len_k_pl_minus_1", "TG" + ag(K - 1), 0),                                  # 17 bases: longer than k, no room for a window
        ("len_k_pl_prefix_at_0", "TG" + ag(K), 0),                                  # 18 bases: one window, at base 0
        ("len_k", acgt(K), 0),                                                      # 16 bases: the strict gate
        ("reverse_strand_only", ag(30) + ag(K) + "CA" + ag(30), 0),
        ("gene_a", gene, 70),
        ("no_window_in_the_middle", ag(60), 0),
        ("prefix_at_last_fit", ag(40) + "TG" + ag(K), 0),
        ("prefix_kmer_past_end", "TG" + ag(38) + "TG" + ag(K - 1), 0),
        ("n_inside_prefix", "TG" + ag(20) + "TNG" + ag(20) + "NTG" + ag(20), 0),  # ("NTG" reads ATG in two bits)
        ("n_behind_prefix", "TG" + ag(20) + "TGN" + ag(20), 0),
        ("n_inside_kmer", "TG" + ag(20) + "TG" + ag(8) + "N" + ag(20), 0),
        ("two_n_closer_than_k_pl", ag(5) + "TG" + ag(20) + "N" + "TG" + ag(10) + "N" + "TG" + ag(20), 0),
    ]
    two = [
        ("leading_and_trailing_n", "NNN" + "TG" + ag(30) + "NN", 0),
        ("palindrome_both_strands", ag(20) + "TG" + PAL + "CA" + ag(20), 0),
        ("one_kmer_twice", twice + ag(5) + twice + ag(10), 0),
        ("shares_a", ag(12) + shared + ag(9), 0),
        ("shares_b", ag(7) + shared + ag(21), 0),
        ("gene_a_variant", "".join(variant), 70),
        ("lower_case_and_iupac", ("tg" + ag(20)).lower() + "WK" + "RRKKSSVVDDMMRRKK" + "rkm" + ag(12).lower(), 0),
        ("trailing_blank_in_header  ", acgt(120), 0),
        ("random_200", acgt(200), 50),
        ("random_90", acgt(90), 0),
        ("ml_len_60", "".join("TG" + ag(3) for _ in range(12)), 0),               # nine windows; -ML 60 asks for more than 60 bases
        ("ml_len_61", "".join("TG" + ag(3) for _ in range(12)) + "A", 0),
        ("random_40_lower_wrapped", acgt(40).lower(), 13),
    ]
    return one, two


def fasta(recs):
    out = []
    for head, seq, width in recs:
        out.append(">" + head + "\n")
        w = width or len(seq)
        out += [seq[a:a + w] + "\n" for a in range(0, len(seq), w)]
    return "".join(out).encode()


def index(tmp, files, case):
    db = os.path.join(tmp, case)
    p = subprocess.run([siu.KMA, "index", "-i"] + files + ["-o", db] + siu.kma_args(case), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    if p.returncode:
        raise SystemExit("kma index %s -> %d\n%s" % (case, p.returncode, p.stderr.decode()))
    skipped = [x.split("\t", 1)[1].rstrip() for x in p.stderr.decode().split("\n") if x.startswith("# Skipped:")]
    return db, skipped


def check_edges(ref, skipped, ref_none, skipped_none, ref_ml, skipped_ml):
    """every edge, on the reference's files of `-k 16 -Sparse TG` (ref), `-Sparse -` and `-ML 60`"""
    names = [None] + ref.name_file.decode().split("\n")[:-1]
    at = {n: i for i, n in enumerate(names) if n}
    sl = lambda n: ref.slengths[at[n]]
    ul = lambda n: ref.ulengths[at[n]]
    need("len_k_pl_minus_1" in skipped and "len_k_pl_minus_1" not in at, "a template of k + pl - 1 bases is skipped")
    need(sl("len_k_pl_prefix_at_0") == 1 and ref.lengths[at["len_k_pl_prefix_at_0"]] == K + PL, "k + pl bases, the prefix at base 0: one window")
    need("len_k" in skipped and "len_k" in skipped_none, "a template of exactly k bases is skipped, with a prefix and without")
    need(sl("reverse_strand_only") == 1, "a template whose only window is on the reverse strand")
    need("no_window_in_the_middle" in skipped and at["prefix_at_last_fit"] == at["gene_a"] + 1, "a template without a window: no id, no name, the next one moves up")
    need(sl("prefix_at_last_fit") == 1, "a prefix at the last position that fits")
    need(sl("prefix_kmer_past_end") == 1, "a prefix whose k-mer would run past the end")
    need(sl("n_inside_prefix") == 2, "an N inside the prefix")
    need(sl("n_behind_prefix") == 1, "an N right behind the prefix")
    need(sl("n_inside_kmer") == 1, "an N inside the k-mer")
    need(sl("two_n_closer_than_k_pl") == 2, "two N closer than k + pl")
    need("leading_and_trailing_n B3" in at and sl("leading_and_trailing_n B3") == 1, "leading and trailing N: the name gains B3")
    need((sl("palindrome_both_strands"), ul("palindrome_both_strands")) == (2, 1), "a palindromic k-mer on both strands: slen 2, ulen 1")
    need(siu.encode(PAL) in ref.lists, "the palindromic k-mer is in the index")
    need((sl("one_kmer_twice"), ul("one_kmer_twice")) == (2, 1), "one k-mer twice in a template: slen 2, ulen 1")
    need([at["shares_a"], at["shares_b"]] in ref.lists.values(), "two templates share a k-mer")
    need(sl("lower_case_and_iupac") == 2, "lower case and IUPAC letters")
    need(sl("random_300_wrapped") > 10 and ref.lengths[at["random_300_wrapped"]] == 300, "wrapped lines")
    need("trailing_blank_in_header" in at, "a trailing blank in a header")
    need(at["leading_and_trailing_n B3"] > at["two_n_closer_than_k_pl"], "two input files, in order")
    kept_ml = set(ref_ml.name_file.decode().split("\n")[:-1])
    need(len(kept_ml) >= 3, "-ML 60 keeps templates")
    need("ml_len_61" in kept_ml and "ml_len_60" in at and "ml_len_60" in skipped_ml and sl("ml_len_60") == sl("ml_len_61") == 9,
         "-ML 60 skips on length (60 bases, not 61) what the plain case keeps")
    need(ref.lengths[at["reverse_strand_only"]] > 60 and "reverse_strand_only" in skipped_ml, "-ML 60 skips on window count what the plain case keeps")
    need(siu.gates(K, K, PL, 60)[1] >= 2, "-ML 60: MinKlen >= 2")
    need(ref_none.DB_size > ref.DB_size and (ref_none.prefix_len, ref_none.prefix) == (0, 1), "-Sparse -: more templates stay, header prefix 1")


def main():
    if not os.path.exists(siu.KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    out = siu.GOLDEN
    os.makedirs(out, exist_ok=True)
    one, two = templates()
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for name, recs in zip(siu.INPUTS, (one, two)):
            plain = os.path.join(tmp, name[:-3])
            put(fasta(recs), plain)
            put_gz(fasta(recs), os.path.join(out, name))
            files.append(plain)
        got = {}
        for case in siu.CASES:
            db, skipped = index(tmp, files, case)
            got[case] = (siu.Files(db), skipped)
            put(lzma.compress(open(db + ".comp.b", "rb").read(), preset=9), os.path.join(out, case + ".comp.b.xz"))
            for ext in (".length.b", ".name", ".seq.b"):
                shutil.copy(db + ext, os.path.join(out, case + ext))
            put("".join(s + "\n" for s in skipped).encode(), os.path.join(out, case + ".skipped.txt"))
            print("%s: DB_size %d, %d k-mers, %d skipped" % (case, got[case][0].DB_size, got[case][0].n, len(skipped)))
        check_edges(*got["k16_TG"], *got["k16_none"], *got["k16_TG_ML60"])
    print("sparse index fixtures written")


if __name__ == "__main__":
    main()
