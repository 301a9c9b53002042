#!/usr/bin/env python3
"""Expected files of the committed single-end and paired fixtures (tests/golden/se, tests/golden/pe) under `-ConClave 2` -- `kma -i
reads.fq.gz -t_db db -o out -1t1 -ConClave 2 -t 1` and `kma -ipe r1.fq.gz r2.fq.gz ... -1t1 -apm p -ConClave 2 -t 1`: runConClave2 on
the frag_raw records whose text taps (out.frag_raw.gz) are committed there -- written to tests/golden/conclave2 as se.res, se.frag.gz,
pe.res and pe.frag.gz (data only: the reference's result rows). Two more inputs are recorded with their taps (<tag>.frag_raw.gz, <tag>.res,
<tag>.frag.gz), each a few hundred reads (proxi_util.reads, seed 7) on a redundant seeded database (proxi_util.INPUTS; the database is
made again from its seed where it is needed): c400, 400 reads on "c" (6 families of 24 variants) -- few reads, so the second pass
decides rows: 66 templates instead of 58 -- and a200, 200 reads on "a" (12 x 12). On the golden inputs and on c400 every ambiguous read
draws its template; a200 holds reads none of whose templates has a unique score, which take the other route of the fourth pass (the
best of the list).

    python3 tests/golden/make_golden_conclave2.py        (needs oracle/_ref/kma: `make -C oracle ref`)
"""
import gzip
import lzma
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
OUT = os.path.join(HERE, "conclave2")


def record(name, inputs, extra):
    src = os.path.join(HERE, name)
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, "db")
        with lzma.open(os.path.join(src, "db.comp.b.xz"), "rb") as f, open(db + ".comp.b", "wb") as g:
            shutil.copyfileobj(f, g)
        for ext in (".length.b", ".seq.b", ".name"):
            shutil.copy(os.path.join(src, "db" + ext), db + ext)
        rows = {}
        for version in ("1", "2"):
            out = os.path.join(tmp, "out" + version)
            # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
            p = subprocess.run([KMA] + [os.path.join(src, x) if x.endswith(".gz") else x for x in inputs] + ["-o", out, "-t_db", db, "-1t1", "-t", "1",
                               "-ConClave", version] + extra, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            assert p.returncode in (0, 2), p.returncode
            rows[version] = gzip.open(out + ".frag.gz").read()
        shutil.copy(os.path.join(tmp, "out2.res"), os.path.join(OUT, name + ".res"))
        with gzip.GzipFile(os.path.join(OUT, name + ".frag.gz"), "wb", mtime=0) as g:
            g.write(rows["2"])
        tm = lambda raw: {x.split(b"\t")[6]: x.split(b"\t")[5] for x in raw.split(b"\n") if x}
        a, b = tm(rows["1"]), tm(rows["2"])
        print(name, open(os.path.join(tmp, "out2.res")).read().count("\n") - 1, "templates,", rows["2"].count(b"\n"), "fragment rows,",
              sum(a.get(h) != t for h, t in b.items()), "of them under another template than with -ConClave 1")


def record_seeded(tag, key, n_reads):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import proxi_util
    from kma_amd import formats, synth
    fam, var, db_seed, _, _ = proxi_util.INPUTS[key]
    names, seqs = synth.make_gene_db(fam, var, 500, 1300, 0.04, seed=db_seed)
    with tempfile.TemporaryDirectory() as tmp:
        db, fq = os.path.join(tmp, "db"), os.path.join(tmp, "reads.fq")
        formats.write_index(db, names, seqs)
        synth.write_fastq(fq, proxi_util.reads(seqs, n_reads, np.random.default_rng(7)), lens=None)
        base = [KMA, "-i", fq, "-t_db", db, "-1t1", "-t", "1"]
        for stem, extra in (("tap", ["-a"]), ("v1", []), ("v2", ["-ConClave", "2"])):
            p = subprocess.run(base + ["-o", os.path.join(tmp, stem)] + extra, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            assert p.returncode in (0, 2), p.returncode
        shutil.copy(os.path.join(tmp, "v2.res"), os.path.join(OUT, tag + ".res"))
        for name, src in ((tag + ".frag.gz", "v2.frag.gz"), (tag + ".frag_raw.gz", "tap.frag_raw.gz")):
            with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as g:
                g.write(gzip.open(os.path.join(tmp, src)).read())
        rows = lambda t: open(os.path.join(tmp, t + ".res")).read().count("\n") - 1
        print(tag, rows("v2"), "templates (", rows("v1"), "with -ConClave 1 ),", gzip.open(os.path.join(tmp, "v2.frag.gz")).read().count(b"\n"), "fragment rows")


def main():
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    os.makedirs(OUT, exist_ok=True)
    record("se", ["-i", "reads.fq.gz"], [])
    record("pe", ["-ipe", "r1.fq.gz", "r2.fq.gz"], ["-apm", "p"])
    record_seeded("c400", "c", 400)
    record_seeded("a200", "a", 200)


if __name__ == "__main__":
    main()
