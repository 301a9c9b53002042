#!/usr/bin/env python3
"""Fixtures of decontamination (`kma index -deCon`, `kma ... -deCon`) under tests/golden/decon/, made by oracle/_ref/kma from seeded
synthetic inputs. Only data is stored: FASTA / FASTQ inputs, the reference's index files and its `-s1` / `-s2` taps.

  m  "mosaic": 12 families of 5 variants (500-800 bases, up to 6 % divergence, k = 16); a host file of 10 records, eight of them
     mosaics of one family's variants (a switch of variant every 40-90 bases, between 150-base random flanks: their reads beat every
     single variant) and two a 300-base piece of one variant between 100-base flanks; 1000 + 1000 reads of 100 bases from genes and
     host, 500 + 500 pairs. The seeds are searched until the reference's own taps show that at least a tenth of the records is gone
     under -deCon and that at least one kept record changed the order of its templates (the swap of deConPrint, ankers.c:106-124).
  w  "wide": one family of 80 variants and a host mosaic of it, 300 reads: candidate lists beyond the scan's 14- and 62-entry tables.
  e  "edges": contamination records cut to hit known k-mers of a small database: exactly k bases (marks nothing), k + 1, an N in
     the middle, lower case, IUPAC letters, reverse complement only, no match, and a second file on the same -deCon."""
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
from kma_amd import formats, synth  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
K = 16


def run(cmd, stdout=None):
    # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
    p = subprocess.run(cmd, stdout=stdout, stderr=subprocess.DEVNULL)
    if p.returncode not in (0, 2):
        raise SystemExit("%s -> %d" % (" ".join(cmd), p.returncode))


def tap(cmd):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    if p.returncode not in (0, 2):
        raise SystemExit("%s -> %d" % (" ".join(cmd), p.returncode))
    return p.stdout


def put_gz(data, dst):
    with gzip.GzipFile(dst, "wb", mtime=0) as g:
        g.write(data)


def gz(src, dst):
    with open(src, "rb") as f:
        put_gz(f.read(), dst)


def xz(src, dst):
    with open(src, "rb") as f, lzma.open(dst, "wb", preset=9) as g:
        shutil.copyfileobj(f, g)


def mosaic(variants, rng, flank):
    """one family's variants, switching variant every 40-90 bases, between random flanks"""
    L = len(variants[0])
    parts, p = [rng.integers(0, 4, flank, dtype=np.uint8)], 0
    while p < L:
        e = min(L, p + int(rng.integers(40, 91)))
        parts.append(variants[int(rng.integers(0, len(variants)))][p:e])
        p = e
    parts.append(rng.integers(0, 4, flank, dtype=np.uint8))
    return np.concatenate(parts)


def host_records(seqs, n_var, rng, n_mosaic, n_piece):
    n_fam = len(seqs) // n_var
    names, recs = [], []
    for i in range(n_mosaic):
        f = int(rng.integers(0, n_fam))
        names.append("host_mosaic%d_fam%d" % (i, f)); recs.append(mosaic(seqs[f * n_var:(f + 1) * n_var], rng, 150))
    for i in range(n_piece):
        s = seqs[int(rng.integers(0, len(seqs)))]
        a = int(rng.integers(0, len(s) - 300))
        names.append("host_piece%d" % i)
        recs.append(np.concatenate([rng.integers(0, 4, 100, dtype=np.uint8), s[a:a + 300], rng.integers(0, 4, 100, dtype=np.uint8)]))
    return names, recs


def store_index(db, outdir):
    xz(db + ".comp.b", os.path.join(outdir, "db.comp.b.xz"))
    xz(db + ".decon.comp.b", os.path.join(outdir, "db.decon.comp.b.xz"))
    for ext in (".length.b", ".seq.b", ".name"):
        shutil.copy(db + ext, os.path.join(outdir, "db" + ext))


def try_m(tmp, seed):
    rng = np.random.default_rng(seed)
    names, seqs = synth.make_gene_db(12, 5, 500, 800, 0.06, seed)
    hn, hs = host_records(seqs, 5, rng, 8, 2)
    fa, ha = os.path.join(tmp, "db.fsa"), os.path.join(tmp, "host.fsa")
    synth.write_fasta(fa, names, seqs); synth.write_fasta(ha, hn, hs)
    g, *_ = synth.make_reads(seqs, 1000, read_len=100, sub_rate=0.005, seed=seed + 1)
    h, *_ = synth.make_reads(hs, 1000, read_len=100, sub_rate=0.005, seed=seed + 2)
    reads = list(g) + list(h)
    order = rng.permutation(len(reads))
    fq = os.path.join(tmp, "reads.fq")
    synth.write_fastq(fq, [reads[i] for i in order])
    a1, a2, _ = synth.make_pairs(seqs, 500, read_len=100, ins_lo=200, ins_hi=400, sub_rate=0.005, seed=seed + 3)
    b1, b2, _ = synth.make_pairs(hs, 500, read_len=100, ins_lo=200, ins_hi=400, sub_rate=0.005, seed=seed + 4)
    m1, m2 = list(a1) + list(b1), list(a2) + list(b2)
    order = rng.permutation(len(m1))
    fq1, fq2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
    synth.write_fastq(fq1, [m1[i] for i in order], prefix="p"); synth.write_fastq(fq2, [m2[i] for i in order], prefix="p")
    db = os.path.join(tmp, "db")
    run([KMA, "index", "-i", fa, "-o", db, "-k", str(K), "-deCon", ha])
    se = [KMA, "-i", fq, "-o", os.path.join(tmp, "out"), "-t_db", db, "-1t1", "-t", "1"]
    taps = dict(s1=tap(se + ["-s1"]), s2_plain=tap(se + ["-s2"]), s2_decon=tap(se + ["-s2", "-deCon"]))
    plain = {r["hdr"]: r for r in formats.parse_s2(taps["s2_plain"])[0]}
    kept = formats.parse_s2(taps["s2_decon"])[0]
    gone = len(plain) - len(kept)
    reordered = sum(1 for r in kept if sorted(r["T"].tolist()) == sorted(plain[r["hdr"]]["T"].tolist()) and r["T"].tolist() != plain[r["hdr"]]["T"].tolist())
    print("m seed %d: %d of %d records gone, %d kept records reordered" % (seed, gone, len(plain), reordered))
    if gone * 10 < len(plain) or reordered < 1:
        return None
    taps["s2_decon_p08"] = tap(se + ["-s2", "-deCon", "-proxi", "0.8"])
    pe = [KMA, "-ipe", fq1, fq2, "-o", os.path.join(tmp, "out"), "-t_db", db, "-1t1", "-t", "1"]
    taps["pe_s1"] = tap(pe + ["-s1"])
    for tag in "puf":
        taps["pe_s2_decon_" + tag] = tap(pe + ["-apm", tag, "-s2", "-deCon"])
        taps["pe_s2_plain_" + tag] = tap(pe + ["-apm", tag, "-s2"])
    return dict(db=db, files=dict(db=fa, host=ha, reads=fq, r1=fq1, r2=fq2), taps=taps)


def make_m(outdir):
    os.makedirs(outdir, exist_ok=True)
    for seed in range(4100, 4200):
        with tempfile.TemporaryDirectory() as tmp:
            got = try_m(tmp, seed)
            if got is None:
                continue
            store_index(got["db"], outdir)
            for name, path in got["files"].items():
                gz(path, os.path.join(outdir, name + (".fsa.gz" if name in ("db", "host") else ".fq.gz")))
            for name, data in got["taps"].items():
                put_gz(data, os.path.join(outdir, name + ".bin.gz"))
            with open(os.path.join(outdir, "seed.txt"), "w") as f:
                f.write("%d\n" % seed)
            return
    raise SystemExit("no seed gave the coverage conditions")


def make_w(outdir, seed=4301):
    os.makedirs(outdir, exist_ok=True)
    rng = np.random.default_rng(seed)
    with tempfile.TemporaryDirectory() as tmp:
        names, seqs = synth.make_gene_db(1, 80, 600, 800, 0.06, seed)
        hn, hs = host_records(seqs, 80, rng, 2, 0)
        fa, ha = os.path.join(tmp, "db.fsa"), os.path.join(tmp, "host.fsa")
        synth.write_fasta(fa, names, seqs); synth.write_fasta(ha, hn, hs)
        g, *_ = synth.make_reads(seqs, 150, read_len=100, sub_rate=0.005, seed=seed + 1)
        h, *_ = synth.make_reads(hs, 150, read_len=100, sub_rate=0.005, seed=seed + 2)
        fq = os.path.join(tmp, "reads.fq")
        synth.write_fastq(fq, list(g) + list(h))
        db = os.path.join(tmp, "db")
        run([KMA, "index", "-i", fa, "-o", db, "-k", str(K), "-deCon", ha])
        se = [KMA, "-i", fq, "-o", os.path.join(tmp, "out"), "-t_db", db, "-1t1", "-t", "1"]
        store_index(db, outdir)
        gz(fa, os.path.join(outdir, "db.fsa.gz")); gz(ha, os.path.join(outdir, "host.fsa.gz")); gz(fq, os.path.join(outdir, "reads.fq.gz"))
        put_gz(tap(se + ["-s1"]), os.path.join(outdir, "s1.bin.gz"))
        put_gz(tap(se + ["-s2"]), os.path.join(outdir, "s2_plain.bin.gz"))
        put_gz(tap(se + ["-s2", "-deCon"]), os.path.join(outdir, "s2_decon.bin.gz"))


def make_e(outdir, seed=4401):
    os.makedirs(outdir, exist_ok=True)
    rng = np.random.default_rng(seed + 7)          # (not the database's seed: the record that matches nothing would repeat family 0's first bases)
    B = synth.BASES
    with tempfile.TemporaryDirectory() as tmp:
        names, seqs = synth.make_gene_db(3, 3, 200, 300, 0.03, seed)
        fa = os.path.join(tmp, "db.fsa")
        synth.write_fasta(fa, names, seqs)
        txt = lambda s: B[s].tobytes()
        with_n = bytearray(txt(seqs[2][30:70])); with_n[20:21] = b"N"
        iupac = txt(seqs[4][50:80]).translate(bytes.maketrans(b"ACGT", b"RYSW"))      # (each folds back onto its base: index.c:128-170)
        recs1 = [
            (b"exactly_k", txt(seqs[0][10:10 + K])),
            (b"k_plus_1", txt(seqs[1][20:20 + K + 1])),
            (b"n_in_the_middle", bytes(with_n)),
            (b"lower_case", txt(seqs[3][40:70]).lower()),
            (b"iupac", iupac[:10] + txt(seqs[4][60:70]) + iupac[20:]),
            (b"reverse_complement_only", txt(synth.revcomp_codes(seqs[5][100:130]))),
            (b"no_match", txt(rng.integers(0, 4, 50, dtype=np.uint8))),
        ]
        recs2 = [(b"second_file", txt(seqs[6][5:45]) + b"\n" + txt(seqs[6][45:60]))]
        h1, h2 = os.path.join(tmp, "host1.fsa"), os.path.join(tmp, "host2.fsa")
        for path, recs in ((h1, recs1), (h2, recs2)):
            with open(path, "wb") as f:
                for n, s in recs:
                    f.write(b">" + n + b"\n" + s + b"\n")
        db = os.path.join(tmp, "db")
        run([KMA, "index", "-i", fa, "-o", db, "-k", str(K), "-deCon", h1, h2])
        store_index(db, outdir)
        gz(fa, os.path.join(outdir, "db.fsa.gz")); gz(h1, os.path.join(outdir, "host1.fsa.gz")); gz(h2, os.path.join(outdir, "host2.fsa.gz"))


if __name__ == "__main__":
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    out = os.path.join(HERE, "decon")
    make_m(os.path.join(out, "m"))
    make_w(os.path.join(out, "w"))
    make_e(os.path.join(out, "e"))
    print("decon fixtures written")
