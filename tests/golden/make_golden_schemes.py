#!/usr/bin/env python3
"""The reference under the scoring schemes of tests/scheme_sets.py: oracle/_ref/kma on the planted short reads with and without -1t1,
and on the couples (-1t1 -ipe ... -apm p) under the schemes the couples run under. Of every run the rows of `.frag.gz`, reduced to
name, number of equally good templates, score, start, end and template, are stored as schemes/<scheme>.<mode>.tsv.gz. Only data is
stored; the inputs are rebuilt from their seeds by whoever reads the rows."""
import gzip
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scheme_sets as ss      # noqa: E402

if __name__ == "__main__":
    if not os.path.exists(KMA):
        sys.exit("oracle/_ref/kma missing: run `make -C oracle ref` first")
    os.makedirs(os.path.join(HERE, "schemes"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        inp = ss.write_inputs(tmp)
        for scheme in ss.SCHEMES:
            for mode in ss.MODES + (("pe",) if scheme in ss.PE_SCHEMES else ()):
                rows = ss.reference_rows(KMA, inp, scheme, mode, os.path.join(tmp, "out"))
                path = os.path.join(HERE, "schemes", "%s.%s.tsv.gz" % (scheme, mode))
                with gzip.GzipFile(path, "wb", mtime=0) as g:
                    g.write("".join("\t".join(r) + "\n" for r in rows).encode())
                print(scheme, mode, len(rows), "rows,", os.path.getsize(path), "bytes")
