"""Shared by the tests of decontamination (`-deCon`): the committed fixtures (tests/golden/decon, make_golden_decon.py) unpacked into a
directory, and the command lines that examples/kmahip_map refuses. No test lives here."""
import gzip
import lzma
import os
import shutil

from kma_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "decon")
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")
INDEX = os.path.join(ROOT, "examples", "kmahip_index")


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def tap(name, which):
    """records of a committed S2 tap"""
    return formats.parse_s2(gunzip(os.path.join(GOLD, name, which + ".bin.gz")))[0]


def unpack(name, tmp):
    """fixture `name` (m, w, e) in directory tmp: the reference's index files (with the decon table) under tmp/db, every .fsa.gz / .fq.gz
    inflated beside them -> dict(dir, prefix, <file stem>: path)"""
    src = os.path.join(GOLD, name)
    tmp = str(tmp)
    prefix = os.path.join(tmp, "db")
    for ext in (".comp.b", ".decon.comp.b"):
        with lzma.open(os.path.join(src, "db" + ext + ".xz"), "rb") as f, open(prefix + ext, "wb") as g:
            shutil.copyfileobj(f, g)
    for ext in (".length.b", ".seq.b", ".name"):
        shutil.copy(os.path.join(src, "db" + ext), prefix + ext)
    out = dict(dir=src, prefix=prefix)
    for f in sorted(os.listdir(src)):
        if f.endswith(".fsa.gz") or f.endswith(".fq.gz"):
            path = os.path.join(tmp, f[:-3])
            with open(path, "wb") as g:
                g.write(gunzip(os.path.join(src, f)))
            out[f.split(".")[0]] = path
    return out


def se_reads(name):
    """the single-end reads of a fixture from its S1 tap -> (records, batch)"""
    import golden_util
    s1 = formats.parse_s1(gunzip(os.path.join(GOLD, name, "s1.bin.gz")))
    return s1, formats.pack_ragged(golden_util.reads_from_s1(s1))


def pe_units(name):
    """the paired stream of a fixture as golden_util.load_pe gives it: dict(s1, units)"""
    s1 = formats.parse_s1(gunzip(os.path.join(GOLD, name, "pe_s1.bin.gz")))
    units, i = [], 0
    while i < len(s1):
        if s1[i]["pair"]:
            units.append(("pe", i, i + 1)); i += 2
        else:
            units.append(("se", i)); i += 1
    return dict(s1=s1, units=units)


def refused_commands(tmp):
    """-> [(arguments behind `kmahip_map`, what the message must name)]: every combination decontamination is not built for. The
    program refuses them before it opens a file or a device."""
    fq, r2, o, db = str(tmp / "r.fq"), str(tmp / "r2.fq"), str(tmp / "out"), str(tmp / "db")
    base = ["-t_db", db, "-o", o, "-deCon"]
    se = ["-i", fq] + base
    return [
        (se, "without -1t1"),
        (["-ipe", fq, r2] + base, "without -1t1"),
        (["-int", fq] + base, "without -1t1"),
        (se + ["-1t1", "-mem_mode"], "-mem_mode"),
        (["-ipe", fq, r2] + base + ["-1t1", "-mem_mode"], "-mem_mode"),
        (se + ["-Mt1", "1"], "-Mt1"),
        (se + ["-1t1", "-gpus", "2"], "-gpus N"),
        (["-ipe", fq, r2] + base + ["-1t1", "-gpus", "2"], "-gpus N"),
    ]
