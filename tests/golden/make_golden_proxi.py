#!/usr/bin/env python3
"""Add the stage-2 taps of proximity matching to the fixtures: `kma ... -1t1 -t 1 -s2 -proxi 0.9` and `-proxi 0.7` on the
database and reads already committed under tests/golden/se (getProxiMatch, savekmers.c:296-340, in place of getBestMatch).
Runs oracle/_ref/kma and stores the two S2 streams as proxi/s2_p09.bin.gz and proxi/s2_p07.bin.gz. Only data is stored."""
import gzip
import hashlib
import lzma
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")


def unpack(src, tmp):
    prefix = os.path.join(tmp, "db")
    with lzma.open(os.path.join(src, "db.comp.b.xz"), "rb") as f, open(prefix + ".comp.b", "wb") as g:
        shutil.copyfileobj(f, g)
    for ext in (".length.b", ".seq.b", ".name"):
        shutil.copy(os.path.join(src, "db" + ext), prefix + ext)
    fq = os.path.join(tmp, "reads.fq")
    with gzip.open(os.path.join(src, "reads.fq.gz"), "rb") as f, open(fq, "wb") as g:
        shutil.copyfileobj(f, g)
    return prefix, fq


def make(outdir):
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        prefix, fq = unpack(os.path.join(HERE, "se"), tmp)
        base = [KMA, "-i", fq, "-o", os.path.join(tmp, "out"), "-t_db", prefix, "-1t1", "-t", "1", "-s2"]
        for tag, f in (("p09", "0.9"), ("p07", "0.7")):
            tap = subprocess.run(base + ["-proxi", f], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
            with gzip.GzipFile(os.path.join(outdir, "s2_%s.bin.gz" % tag), "wb", mtime=0) as g:
                g.write(tap)
            print("-proxi", f, len(tap), "bytes, md5", hashlib.md5(tap).hexdigest())


if __name__ == "__main__":
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    make(os.path.join(HERE, "proxi"))
