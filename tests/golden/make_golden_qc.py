#!/usr/bin/env python3
"""Fixtures for the QC report (-qc) and the trimmed reads (`kma trim`): what the compiled reference (oracle/_ref/kma) writes for the
inputs of tests/golden/ingest and three new ones under the settings of make_golden_ingest.py plus `-mi 25 -5p 3 -3p 2` and `-ml 1000`.

    python3 tests/golden/make_golden_qc.py        (needs the reference binary: `make -C oracle ref`)

New inputs, in tests/golden/qc/: long.fq.gz (reads of 40 to 5 000 bases, among them 511, 512, 513, 1023, 1024 and 1025, ordered so that
the length histogram's resolution rises several times, and N-rich reads at the -ml gate), uni.fq (uniform quality 2..41 at three
lengths: where the quality bin is decided by the last bit of a log10) and one.fq (a single read). Recorded per case and setting, each
gzip-compressed: <case>.<setting>.json.gz (the report), .s1.gz (the S1 stream of `kma ... -s1 -qc`), .fq.gz and .int_fq.gz (the files of
`kma trim -o P`: P.fq and P_int.fq). The cases and settings are those of tests/qc_util.py."""
import gzip
import json
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
sys.path.insert(0, HERE)
import make_golden_ingest as mgi  # noqa: E402
import qc_util  # noqa: E402
from kma_amd import synth  # noqa: E402

KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
OUT = qc_util.QC


def write_long(path):
    rng = np.random.default_rng(11)
    lens = [int(x) for x in rng.integers(40, 300, 8)] + [511, 512, 513] + [int(x) for x in rng.integers(40, 300, 8)] + [1023, 1024, 1025]
    lens += [int(x) for x in rng.integers(40, 400, 8)] + [2500] + [int(x) for x in rng.integers(40, 300, 8)] + [5000] + [int(x) for x in rng.integers(40, 700, 12)]
    recs = []
    for i, L in enumerate(lens):
        recs.append((b"@l%d len=%d" % (i, L), mgi.rand_read(rng, L), mgi.rand_qual(rng, L)))
    # N-rich reads of good quality at the length gates (16, 40, 60): long enough as they stand, too short without their N's
    for i, (L, n) in enumerate(((40, 28), (40, 26), (44, 30), (50, 14), (52, 13), (70, 12), (72, 15), (41, 24))):
        s = bytearray(mgi.ALPHA[j] for j in rng.integers(0, 4, L))
        for p in rng.choice(np.arange(2, L - 2), n, replace=False):
            s[int(p)] = ord("N")
        recs.insert(5 + 7 * i, (b"@n%d N-rich" % i, bytes(s), bytes([33 + 38]) * L))
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        for h, s, q in recs:
            f.write(h + b"\n" + s + b"\n+\n" + q + b"\n")


def write_uni(path):
    rng = np.random.default_rng(12)
    with open(path, "wb") as f:
        for L in (36, 100, 151):
            for q in range(2, 42):
                f.write(b"@u%d_%d\n" % (L, q) + bytes(mgi.ALPHA[j] for j in rng.integers(0, 4, L)) + b"\n+\n" + bytes([33 + q]) * L + b"\n")


def write_one(path):
    rng = np.random.default_rng(13)
    with open(path, "wb") as f:
        f.write(b"@only one\n" + bytes(mgi.ALPHA[j] for j in rng.integers(0, 4, 100)) + b"\n+\n" + bytes([33 + 35]) * 100 + b"\n")


def inputs_of(case):
    se, pe, il = qc_util.CASES[case]
    args = []
    if se:
        args += ["-i"] + [qc_util.path_of(f) for f in se]
    if pe:
        args += ["-ipe"] + [qc_util.path_of(f) for f in pe]
    if il:
        args += ["-int"] + [qc_util.path_of(f) for f in il]
    return args


def put(case, setting, ext, data):
    with gzip.GzipFile(os.path.join(OUT, f"{case}.{setting}.{ext}.gz"), "wb", mtime=0) as g:
        g.write(data)


def main():
    if not os.path.exists(KMA):
        sys.exit("build the reference first: make -C oracle ref")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    write_long(os.path.join(OUT, "long.fq.gz"))
    write_uni(os.path.join(OUT, "uni.fq"))
    write_one(os.path.join(OUT, "one.fq"))
    seen = dict(branches=set(), both_ends=0)
    reports = {}
    with tempfile.TemporaryDirectory() as tmp:
        names, seqs = synth.make_gene_db(3, 2, 300, 400, 0.02, seed=5)
        fa = os.path.join(tmp, "db.fsa")
        synth.write_fasta(fa, names, seqs)
        db = os.path.join(tmp, "db")
        subprocess.run([KMA, "index", "-i", fa, "-o", db], check=True, stderr=subprocess.DEVNULL)
        for case in qc_util.CASES:
            for setting in qc_util.SETTINGS:
                flags = qc_util.ref_flags(setting)
                o = os.path.join(tmp, "t")
                for ext in (".fq", "_int.fq", ".json"):
                    if os.path.exists(o + ext):
                        os.remove(o + ext)
                subprocess.run([KMA, "trim"] + inputs_of(case) + ["-o", o, "-qc"] + flags, check=True, stderr=subprocess.DEVNULL)
                report = open(o + ".json", "rb").read()
                put(case, setting, "json", report)
                put(case, setting, "fq", open(o + ".fq", "rb").read())
                if os.path.exists(o + "_int.fq"):
                    put(case, setting, "int_fq", open(o + "_int.fq", "rb").read())
                m = os.path.join(tmp, "m")
                r = subprocess.run([KMA] + inputs_of(case) + ["-o", m, "-t_db", db, "-1t1", "-t", "1", "-s1", "-qc"] + flags, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
                put(case, setting, "s1", r.stdout)
                assert open(m + ".json", "rb").read() == report, "kma -qc and kma trim -qc write the same report"
                reports[case, setting] = json.loads(report)
                mine = qc_util.restate(case, setting)
                seen["branches"].add(mine["qc"].n50_branch())
                if "eq" in setting:
                    seen["both_ends"] += mine["both_ends"]
                print(case, setting, reports[case, setting]["Fragment Count"], "fragments,", reports[case, setting]["Sequence Count"], "sequences")
        # what the set has to hold, on the reference's own output
        assert reports["long", "default"]["Length Resolution"] > 1
        assert seen["branches"] == {"maxlen", "scaled", "plain"}, seen["branches"]
        q = reports["uni", "default"]["Q Distribution"]
        assert sum(q) == 66 and any(q[b] != 3 for b in range(20, 42)), "a read of uniform quality outside its nominal bin"
        o = os.path.join(tmp, "plain")
        r = subprocess.run([KMA, "trim"] + inputs_of("long") + ["-o", o], check=True, stderr=subprocess.PIPE)
        plain = int(r.stderr.decode().strip().splitlines()[-1].split("\t")[-1])
        assert plain > reports["long", "default"]["Fragment Count"], "a read dropped only under -qc"
        pe = reports["pe", "default"]
        assert pe["Fragment Count"] != pe["Sequence Count"] and qc_util.gold("pe", "default", "fq"), "a couple that loses one mate"
        assert seen["both_ends"] > 0, "a read that the -eq loop cuts at both ends"
        # (long.fq.gz holds reads of a thousand bases: there the block stays)
        assert all(("Minimum Q" in reports[c, "ml1000"]) == (c == "long") for c in qc_util.CASES), "the Q block absent under -ml 1000"
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("tests/golden/qc:", len(os.listdir(OUT)), "files,", total, "bytes, largest", max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)))


if __name__ == "__main__":
    main()
