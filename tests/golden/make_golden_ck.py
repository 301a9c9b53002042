#!/usr/bin/env python3
"""The fixtures of the counting template finder (`-ck`, save_kmers_count savekmers.c:3067-3365 and get_kmers_for_pair_count :690-824),
written to tests/golden/ck. Runs oracle/_ref/kma; only data is stored: gzip'd `-s2` taps, a FASTA and a FASTQ, the index files of
the hand-made database and cases.tsv.

  on tests/golden/se   s2_ck.bin.gz (-1t1 -ck), s2_ck_ex.bin.gz (+ -ex_mode), s2_ck_p07.bin.gz (+ -proxi 0.7)
  on tests/golden/pe   s2_ck_pe_p.bin.gz (-1t1 -apm p -ck), s2_ck_pe_u.bin.gz (-1t1 -apm u -ck), s2_ck_pe_default.bin.gz (-ck alone)
  the edge set, k = 16 edge.fsa.gz, edge.fq.gz, edge.{comp.b.xz,length.b,seq.b,name} (indexed by the reference),
                       s2_edge.bin.gz (-1t1 -ck), s2_edge_ex.bin.gz (+ -ex_mode), cases.tsv
                       edge_r1.fq.gz, edge_r2.fq.gz: four pairs; s2_edge_pe_p.bin.gz (-1t1 -apm p -ck), s2_edge_pe_u.bin.gz (-1t1 -apm u -ck)

cases.tsv names every read of the edge set with its intended outcome without and with -ex_mode (rc_flag 0 and an empty list: no
record); the outcome is asserted on the reference's taps below before anything is written.

    python3 tests/golden/make_golden_ck.py        (needs oracle/_ref/kma: `make -C oracle ref`)
"""
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
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
OUT = os.path.join(HERE, "ck")
K = 16

import ck_util  # noqa: E402
from kma_amd import formats  # noqa: E402


def put(name, data):
    with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as g:
        g.write(data)


def unpack_db(src, tmp):
    prefix = os.path.join(tmp, "db")
    with lzma.open(os.path.join(src, "db.comp.b.xz"), "rb") as f, open(prefix + ".comp.b", "wb") as g:
        shutil.copyfileobj(f, g)
    for ext in (".length.b", ".seq.b", ".name"):
        shutil.copy(os.path.join(src, "db" + ext), prefix + ext)
    return prefix


def tap(args):
    return subprocess.run([KMA] + args + ["-t", "1", "-s2"], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout


def text(codes):
    return "".join("ACGTN"[c] for c in codes)


def rc(codes):
    c = np.asarray(codes, np.uint8)[::-1]
    return np.where(c > 3, 4, 3 - c).astype(np.uint8)


def with_n(codes, *pos):
    c = np.array(codes, np.uint8)
    c[list(pos)] = 4
    return c


def edge_set():
    """-> (template names, template codes, [(read name, codes, note, expected, expected under -ex_mode)]); expected: None = no
    record, (rc_flag, flag, T), or "restated" = whatever tests/ck_util.py computes (asserted on the tap like the others)"""
    rng = np.random.default_rng(1603)
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)  # noqa: E731
    names, seqs = [], []

    def add(name, s):
        names.append(name)
        seqs.append(np.asarray(s, np.uint8))
        return len(names)

    t1 = rnd(400)
    add("plain", t1)
    unit = rnd(40)
    add("tandem", np.concatenate([rnd(30), unit, unit, rnd(30)]))
    x = rnd(60)
    add("palindrome", np.concatenate([x, rc(x)]))
    p = rnd(200)
    q = p.copy()
    q[100] = (q[100] + 1) & 3
    tp = add("rule_p", p)
    tq = add("rule_q", q)
    core = rnd(100)
    seg = {n: rnd(40) for n in (14, 15, 62, 63)}
    fam0 = len(names) + 1
    for i in range(80):
        add("fam%02d" % i, np.concatenate([core] + [seg[n] for n in (14, 15, 62, 63) if i < n] + [rnd(30)]))
    tl = rnd(12000)
    tlong = add("long", tl)

    fam = lambda n: list(range(fam0, fam0 + n))  # noqa: E731
    g = t1[150:250]
    R = "restated"
    offstride = np.concatenate([rnd(1), t1[100:130], rnd(2), t1[200:230]])
    long10k = tl[1500:11500].copy()
    long10k[[777, 5000, 9100]] = (long10k[[777, 5000, 9100]] + 1) & 3
    reads = [
        ("exact30", t1[50:80], "15 counted k-mers: below kmersize", None, None),
        ("exact31", t1[50:81], "16 counted k-mers: a record", (16, 0, [1]), (16, 0, [1])),
        ("len15", t1[10:25], "k - 1 bases", None, None),
        ("len16", t1[10:26], "k bases: one k-mer", None, None),
        ("offstride", offstride, "30 matching k-mers, none on the quick check's stride", None, (30, 0, [1])),
        ("tandem", np.concatenate([unit, unit]), "every k-mer of the unit counted twice", (65, 0, [2]), (65, 0, [2])),
        ("tie", x, "the template holds its own reverse complement", (-45, 0, [3, -3]), (-45, 0, [3, -3])),
        ("n_fwd", with_n(g, 20), "forward-best, one N", (69, 0, [1]), R),
        ("n_rev", with_n(rc(g), 20), "reverse-best, one N at an asymmetric position", R, R),
        ("n_ends_fwd", with_n(g, 0, 99), "N at base 0 and at the last base", (83, 0, [1]), R),
        ("n_ends_rev", with_n(rc(g), 0, 99), "the same, reverse-best", R, R),
        ("n_close_fwd", with_n(g, 30, 40), "two N's fewer than k apart", (59, 0, [1]), R),
        ("n_close_rev", with_n(rc(g), 30, 40), "the same, reverse-best", R, R),
        ("n_rule", with_n(rc(p[60:160]), 40), "reverse-best: the forward-N-list rule ties rule_p and rule_q, the mirrored rule would not", R, R),
        ("fam14", seg[14], "14 candidates: the first tier's table is full", (25, 0, fam(14)), (25, 0, fam(14))),
        ("fam15", seg[15], "15 candidates: the second tier", (25, 0, fam(15)), (25, 0, fam(15))),
        ("fam62", seg[62], "62 candidates: the second tier's table is full", (25, 0, fam(62)), (25, 0, fam(62))),
        ("fam63", seg[63], "63 candidates: the wavefront-per-item kernel", (25, 0, fam(63)), (25, 0, fam(63))),
        ("fam80", core[:60], "80 candidates", (45, 0, fam(80)), (45, 0, fam(80))),
        ("fam80_rev", rc(core[20:90]), "80 candidates on the reverse strand", (55, 16, fam(80)), (55, 16, fam(80))),
        ("len150", tl[0:150], "one pass of the scan", (135, 0, [tlong]), (135, 0, [tlong])),
        ("len193", tl[200:393], "beyond the 192 bases of a record", (178, 0, [tlong]), (178, 0, [tlong])),
        ("len1000", rc(tl[1000:2000]), "several passes, reverse strand", (985, 16, [tlong]), (985, 16, [tlong])),
        ("len10000", long10k, "many passes, three substitutions", (9985 - 48, 0, [tlong]), (9985 - 48, 0, [tlong])),
    ]
    assert tp == 4 and tq == 5
    # pairs: rule_p and rule_q differ in base 100. `apart`: mate 1 counts 85 on rule_p and 69 on rule_q, mate 2 the other way round:
    # the best common template sums to 154 < 85 + 85 - PE (7), each mate keeps its own best. `together`: mate 2 is shorter, 70 on
    # rule_q and 64 on rule_p: 85 + 64 = 149 > 85 + 70 - 7, the pairing penalty makes a couple on rule_p (the union pairing does not)
    pairs = [
        ("couple", tl[100:200], rc(tl[300:420])),
        ("lone", tl[100:200], rnd(100)),
        ("apart", p[20:120], rc(q[80:180])),
        ("together", p[20:120], rc(q[95:180])),
    ]
    return names, seqs, reads, pairs


def parse_tap(buf):
    recs, _ = formats.parse_s2(buf)
    return {r["hdr"].rstrip(b"\0").split()[0].decode(): (int(r["rc_flag"]), int(r["flag"]), [int(t) for t in r["T"]]) for r in recs}


def main():
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the committed single-end and paired fixtures
        se = unpack_db(os.path.join(HERE, "se"), os.path.join(tmp))
        fq = os.path.join(HERE, "se", "reads.fq.gz")
        base = ["-i", fq, "-o", os.path.join(tmp, "out"), "-t_db", se, "-1t1", "-ck"]
        for name, extra in (("s2_ck.bin.gz", []), ("s2_ck_ex.bin.gz", ["-ex_mode"]), ("s2_ck_p07.bin.gz", ["-proxi", "0.7"])):
            t = tap(base + extra)
            put(name, t)
            print(name, len(formats.parse_s2(t)[0]), "records")
        os.makedirs(os.path.join(tmp, "pe"))
        pe = unpack_db(os.path.join(HERE, "pe"), os.path.join(tmp, "pe"))
        base = ["-ipe", os.path.join(HERE, "pe", "r1.fq.gz"), os.path.join(HERE, "pe", "r2.fq.gz"), "-o", os.path.join(tmp, "out"), "-t_db", pe, "-ck"]
        for name, extra in (("s2_ck_pe_p.bin.gz", ["-1t1", "-apm", "p"]), ("s2_ck_pe_u.bin.gz", ["-1t1", "-apm", "u"]), ("s2_ck_pe_default.bin.gz", [])):
            t = tap(base + extra)
            put(name, t)
            print(name, len(t), "bytes")
        # ---- the edge set
        names, seqs, reads, pairs = edge_set()
        fsa = os.path.join(tmp, "edge.fsa")
        with open(fsa, "w") as f:
            for n, s in zip(names, seqs):
                f.write(">%s\n%s\n" % (n, text(s)))
        efq = os.path.join(tmp, "edge.fq")
        with open(efq, "w") as f:
            for n, c, *_ in reads:
                f.write("@%s\n%s\n+\n%s\n" % (n, text(c), "I" * len(c)))
        prefix = os.path.join(tmp, "edge")
        subprocess.run([KMA, "index", "-i", fsa, "-o", prefix, "-k", str(K)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        base = ["-i", efq, "-o", os.path.join(tmp, "out"), "-t_db", prefix, "-1t1", "-ck"]
        taps = [tap(base), tap(base + ["-ex_mode"])]
        got = [parse_tap(t) for t in taps]
        d = ck_util.kmer_dict(seqs, K)
        rows = []
        for n, c, note, *want in reads:
            row = [n, note]
            for ex in (0, 1):
                w = want[ex]
                if w == "restated":
                    w = ck_util.save_kmers_count(d, K, c, exhaustive=bool(ex))
                have = got[ex].get(n)
                assert have == (None if w is None else (w[0], w[1], list(w[2]))), (n, ex, w, have)
                row += ["0", "0", ""] if w is None else [str(w[0]), str(w[1]), ",".join(str(t) for t in w[2])]
            rows.append(row)
        # the read that pins the forward-N-list rule: the mirrored rule gives another list
        r = dict((n, c) for n, c, *_ in reads)["n_rule"]
        assert ck_util.save_kmers_count(d, K, r)[2] == [4, 5] and ck_util.save_kmers_count(d, K, r, mirrored=True)[2] == [4]
        with open(os.path.join(OUT, "cases.tsv"), "w") as f:
            f.write("name\tnote\trc_flag\tflag\tT\tex_rc_flag\tex_flag\tex_T\n")
            for row in rows:
                f.write("\t".join(row) + "\n")
        # the pairs
        for k in (1, 2):
            with open(os.path.join(tmp, "edge_r%d.fq" % k), "w") as f:
                for pr in pairs:
                    f.write("@%s\n%s\n+\n%s\n" % (pr[0], text(pr[k]), "I" * len(pr[k])))
            put("edge_r%d.fq.gz" % k, open(os.path.join(tmp, "edge_r%d.fq" % k), "rb").read())
        want = {
            "p": [("couple", 85, 99, []), ("couple", 105, 147, [86]), ("lone", 85, 105, [86]), ("apart", 85, 97, [4]), ("apart", 85, 145, [5]),
                  ("together", 85, 99, []), ("together", 70, 147, [4])],
            "u": [("couple", 85, 99, []), ("couple", 105, 147, [86]), ("lone", 85, 105, [86]), ("apart", 85, 97, [4]), ("apart", 85, 145, [5]),
                  ("together", 85, 97, [4]), ("together", 70, 145, [5])],
        }
        for apm in ("p", "u"):
            t = tap(["-ipe", os.path.join(tmp, "edge_r1.fq"), os.path.join(tmp, "edge_r2.fq"), "-o", os.path.join(tmp, "out"), "-t_db", prefix, "-1t1", "-ck", "-apm", apm])
            have = [(r["hdr"].rstrip(b"\0").decode(), int(r["rc_flag"]), int(r["flag"]), [int(x) for x in r["T"]]) for r in formats.parse_s2(t)[0]]
            assert have == want[apm], (apm, have)
            # the intended outcome above is also what the restated pairing computes from the counted candidates
            restated = [(pr[0], int(r["rc_flag"]), int(r["flag"]), [int(x) for x in r["T"]])
                        for pr in pairs for r in ck_util.scan_pair(d, K, pr[1], pr[2], union=apm == "u")]
            assert restated == want[apm], (apm, restated)
            put("s2_edge_pe_%s.bin.gz" % apm, t)
        put("edge.fsa.gz", open(fsa, "rb").read())
        put("edge.fq.gz", open(efq, "rb").read())
        put("s2_edge.bin.gz", taps[0])
        put("s2_edge_ex.bin.gz", taps[1])
        with open(prefix + ".comp.b", "rb") as f, lzma.open(os.path.join(OUT, "edge.comp.b.xz"), "wb", preset=9) as g:
            shutil.copyfileobj(f, g)
        for ext in (".length.b", ".seq.b", ".name"):
            shutil.copy(prefix + ext, os.path.join(OUT, "edge" + ext))
        print(len(reads), "edge reads,", len(names), "templates,", sum(os.path.getsize(os.path.join(OUT, x)) for x in os.listdir(OUT)), "bytes in all")


if __name__ == "__main__":
    main()
