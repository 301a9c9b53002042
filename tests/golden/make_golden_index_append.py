#!/usr/bin/env python3
"""Fixtures of appending to an index (`kma index -t_db`) under tests/golden/index_append/, made by oracle/_ref/kma. Only data is
stored: hand-made FASTA parts (a: the old database; b = b1 + b2: what is appended; c: contamination), the reference's old indexes
(tests/index_append_util.OLD) and its appended ones (.comp.b as .xz, .length.b, .name, .seq.b), its decontamination tables, and
cli.tsv: first line of stderr and status of the command lines that end before an index is read.

Every property the parts are made for is asserted on the reference's own output before anything is written; the script ends with an
error when one does not hold."""
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
import index_append_util as iau  # noqa: E402
import sparse_index_util as siu  # noqa: E402

LIMIT = 350_000          # bytes a stored file
FAMILY = 5               # the A templates that share one segment


def need(cond, what):
    if not cond:
        raise SystemExit("not met on the reference's output: " + what)
    print("  ok: " + what)


def put(data, dst):
    with open(dst, "wb") as f:
        f.write(data)
    if os.path.getsize(dst) > LIMIT:
        raise SystemExit("%s: %d bytes" % (dst, os.path.getsize(dst)))


def gz(data):
    import io
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as g:
        g.write(data)
    return buf.getvalue()


def revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def parts(seed=20262):
    rng = np.random.default_rng(seed)
    acgt = lambda n: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))
    seg = acgt(120)
    a = [("a_random_%02d" % i, acgt(int(rng.integers(80, 400))), (0, 60, 70)[i % 3]) for i in range(18)]
    a += [("a_family_%d" % i, acgt(50) + seg + acgt(40 + 5 * i), 0) for i in range(FAMILY)]
    a += [
        ("a_inner_n", acgt(100) + "N" + acgt(60) + "NN" + acgt(80), 80),
        ("a_inner_n_near_the_end", acgt(90) + "N" + acgt(20), 0),
        ("a_iupac", acgt(40) + "RYKMSWBDHV" + acgt(40) + "UuXx" + acgt(40), 0),          # (X reads as N)
        ("a_lower_case", acgt(150).lower(), 50),
    ]
    b = [
        ("b_copy_of_a_random_03", a[3][1], 0),
        ("b_reverse_complement_of_a_random_05", revcomp(a[5][1]), 60),
        ("b_shares_60_of_the_family_segment", acgt(45) + seg[30:90] + acgt(45), 0),
        ("b_nothing_in_common", acgt(200), 0),
        ("b_random_00", acgt(130), 0),
        ("b_three_leading_n", "NNN" + acgt(150), 0),
        ("b_shorter_than_k", acgt(8), 0),
        ("b_inner_n", acgt(70) + "N" + acgt(70), 0),
        ("b_random_01", acgt(310).lower(), 70),
        ("b_random_02", acgt(96), 0),          # (three full words of .seq.b and one more)
        ("b_variant_of_a_random_07", a[7][1][:60] + acgt(1) + a[7][1][61:], 0),
        ("b_random_03", acgt(64), 0),
    ]
    c = [
        ("c_piece_of_a_random_02", a[2][1][10:70], 0),
        ("c_piece_of_b_nothing_in_common_reversed", revcomp(b[3][1][20:120]), 0),
        ("c_k_bases", acgt(16), 0),
        ("c_with_n", a[9][1][:30] + "N" + a[9][1][31:60], 0),
        ("c_foreign", acgt(300), 60),
    ]
    return a, b, c, seg


def fasta(recs):
    out = []
    for head, seq, width in recs:
        out.append(">" + head + "\n")
        w = width or len(seq)
        out += [seq[x:x + w] + "\n" for x in range(0, len(seq), w)]
    return "".join(out).encode()


def kma_index(args):
    p = subprocess.run([iau.KMA, "index"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    if p.returncode:
        raise SystemExit("kma index %s -> %d\n%s" % (" ".join(args), p.returncode, p.stderr.decode()))


def copy_index(src, dst):
    for ext in (".comp.b", ".length.b", ".name", ".seq.b"):
        shutil.copy(src + ext, dst + ext)


def main():
    if not os.path.exists(iau.KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    out = iau.GOLDEN
    os.makedirs(out, exist_ok=True)
    a, b, c, seg = parts()
    half = 6
    text = {"a": fasta(a), "b": fasta(b), "b1": fasta(b[:half]), "b2": fasta(b[half:]), "c": fasta(c)}
    store = {}          # file name under the fixture folder -> bytes
    with tempfile.TemporaryDirectory() as tmp:
        fa = {}
        for name, data in text.items():
            fa[name] = os.path.join(tmp, name + ".fsa")
            put(data, fa[name])
            store[name + ".fsa.gz"] = gz(data)
        p = lambda name: os.path.join(tmp, name)
        for name, args in iau.OLD.items():
            kma_index(["-i", fa["a"], "-o", p(name)] + args)
        need(iau.Comp(p("A_k10") + ".comp.b").mega and not iau.Comp(p("A_k12") + ".comp.b").mega, "the k = 10 index is direct-address, the k = 12 one hashed")

        # the expansion cannot be replaced by a rebuild from .seq.b
        put(fasta([(h, s.replace("N", "A").replace("n", "A").replace("X", "A").replace("x", "A"), w) for h, s, w in a]), p("a_noN.fsa"))
        kma_index(["-i", p("a_noN.fsa"), "-o", p("A_noN"), "-k", "16"])
        n_with, n_without = iau.Comp(p("A_k16") + ".comp.b").n, iau.Comp(p("A_noN") + ".comp.b").n
        need(n_with != n_without and open(p("A_k16") + ".seq.b", "rb").read() == open(p("A_noN") + ".seq.b", "rb").read(),
             "N -> A changes the k-mers (%d, %d) and leaves .seq.b as it is" % (n_with, n_without))

        got = {}
        for case, d in iau.CASES.items():
            if d.get("fresh_is_the_oracle"):
                # the reference's own append onto a direct-address index is no oracle: at k = 10 it ends with a segmentation fault, at
                # k = 9 it writes a value array a thousand times the fresh build's. What an append has to give is the fresh build
                fresh = p("fresh_" + case)
                kma_index(["-i", fa["a"]] + [fa[x] for step in d["steps"] for x in step] + ["-o", fresh] + iau.OLD[d["old"]])
                q = subprocess.run([iau.KMA, "index", "-t_db", p(d["old"]), "-i", fa["b"], "-o", p("broken")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                need(q.returncode != 0, "%s: the reference's own append ends with status %d" % (case, q.returncode))
                got[case] = fresh
                continue
            cur = p("run_" + case)
            copy_index(p(d["old"]), cur)
            for si, step in enumerate(d["steps"]):
                last = si == len(d["steps"]) - 1
                nxt = cur if d.get("inplace") else "%s_%d" % (p("run_" + case), si)
                args = ["-t_db", cur] + (["-i"] + [fa[x] for x in step] if step else []) + ([] if d.get("inplace") else ["-o", nxt]) + d["line"]
                if d.get("decon") and last:
                    args += ["-deCon", fa["c"]]
                kma_index(args)
                if not step:          # decon onto the index: only the decon table is written
                    iau.files_equal(cur, p(d["old"]))
                    need(sorted(f for f in os.listdir(tmp) if f.startswith(os.path.basename(cur) + ".")) ==
                         sorted(os.path.basename(cur) + e for e in (".comp.b", ".decon.comp.b", ".length.b", ".name", ".seq.b")),
                         "%s: .decon.comp.b is written and the four files are left alone" % case)
                cur = nxt
            got[case] = cur
            # every appended index equals the reference's fresh build of the concatenation
            fresh = p("fresh_" + case)
            files = [fa["a"]] + [fa[x] for step in d["steps"] for x in step]
            kma_index(["-i"] + files + ["-o", fresh] + iau.OLD[d["old"]] + (["-deCon", fa["c"]] if d.get("decon") else []))
            iau.same_index(cur, fresh)
            if d.get("decon"):
                iau.same_comp(cur + ".decon.comp.b", fresh + ".decon.comp.b")
            print("  ok: %s equals the fresh build of the concatenation" % case)
        for case, d in iau.CASES.items():
            first = next(x for x, e in iau.CASES.items() if e["want"] == d["want"])
            iau.same_index(got[case], got[first])
        need(open(got["TG_with_the_option"] + ".comp.b", "rb").read() == open(got["TG_without_the_option"] + ".comp.b", "rb").read(),
             "a sparse index is appended sparsely with -Sparse TG on the line and without: the same bytes")
        k12 = iau.Comp(got["k12_with_k16_on_the_line"] + ".comp.b")
        need((k12.mlen, k12.kmersize) == (12, 12), "-k 16 beside -t_db is ignored")

        # the shared list that diverges
        names = open(got["k16"] + ".name").read().split("\n")[:-1]
        fam = tuple(i + 1 for i, n in enumerate(names) if n.startswith("a_family_"))
        bid = names.index("b_shares_60_of_the_family_segment") + 1
        before = [x for x in iau.Comp(p("A_k16") + ".comp.b").stored_lists() if x[:FAMILY] == fam]
        after = [x for x in iau.Comp(got["k16"] + ".comp.b").stored_lists() if x[:FAMILY] == fam]
        need(len(fam) == FAMILY and before == [fam] and sorted(after) == [fam, fam + (bid,)], "the family's list is stored once before the append and twice after")
        need("b_three_leading_n B3" in names and "b_shorter_than_k" not in names and len(names) == len(a) + len(b) - 1, "B3 in a name, the short template skipped")
        m = iau.Comp(got["k16"] + ".comp.b").mapping()
        need((names.index("a_random_03") + 1, names.index("b_copy_of_a_random_03") + 1) in m.values(), "the copy shares every k-mer with its original")
        noc = names.index("b_nothing_in_common") + 1
        need(all(ids == (noc,) for ids in m.values() if noc in ids), "a template with no k-mer in common with the old index")
        dd, da = iau.Comp(got["decon_onto_the_index"] + ".decon.comp.b"), iau.Comp(got["append_and_decon"] + ".decon.comp.b")
        need(any(ids[-1] == dd.DB_size for ids in dd.mapping().values()) and dd.DB_size == len(a) + 1, "decon onto the index marks k-mers with the old DB_size")
        need(any(ids == (noc, da.DB_size) for ids in da.mapping().values()) and da.DB_size == len(names) + 1, "append and decon marks k-mers of a new template with the new DB_size")

        for name in list(iau.OLD) + list(iau.RECORDED):
            src = p(name) if name in iau.OLD else got[next(x for x, e in iau.CASES.items() if e["want"] == name)]
            store[name + ".comp.b.xz"] = lzma.compress(open(src + ".comp.b", "rb").read(), preset=9)
            for ext in (".length.b", ".name", ".seq.b"):
                store[name + ext] = open(src + ext, "rb").read()
        for case, d in iau.CASES.items():
            if d.get("want_decon"):
                store[d["want_decon"] + ".decon.comp.b.xz"] = lzma.compress(open(got[case] + ".decon.comp.b", "rb").read(), preset=9)
        rows = []
        for args in iau.CLI_CASES:
            q = subprocess.run([iau.KMA, "index"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, cwd=tmp)
            rows.append("%s\t%d\t%s\n" % (" ".join(args), q.returncode, q.stderr.decode().split("\n")[0]))
        store["cli.tsv"] = "".join(rows).encode()
    for name, data in store.items():
        put(data, os.path.join(out, name))
    print("index append fixtures written: %d files, %d bytes" % (len(store), sum(len(x) for x in store.values())))


if __name__ == "__main__":
    main()
