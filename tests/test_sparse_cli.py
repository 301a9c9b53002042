"""Sparse mapping (`-Sparse`) at the boundary, without a GPU: the entry points are declared and the header stays plain C99, what
examples/kmahip_map refuses it refuses by name with status 2 before a file or a device is opened, a wrong `-ss` gets the reference's
message, and kmahip_sparse_open refuses what it does not serve with the reason in kmahip_last_error, before any device call."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest

import golden_util
import proxi_util
import sparse_util as su
from sparse_util import KMA, MAP, ROOT

TIMEOUT = 60
SYMS = ("kmahip_sparse_open", "kmahip_sparse_close", "kmahip_sparse_get_info", "kmahip_sparse_template", "kmahip_sparse_count", "kmahip_sparse_count_dev",
        "kmahip_sparse_counts", "kmahip_sparse_collect", "kmahip_sparse_withdraw", "kmahip_sparse_scores", "kmahip_sparse_default_opts", "kmahip_sparse_rows",
        "kmahip_sparse_write", "kmahip_sparse_set_timing", "kmahip_sparse_get_timing", "kmahip_sparse_set_noadd")


@pytest.fixture(scope="module")
def built():
    proxi_util.build_map()


def test_entry_points_are_declared_and_the_header_is_c99(tmp_path):
    src = open(os.path.join(ROOT, "include", "kmahip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym
    c = tmp_path / "use.c"
    c.write_text('#include "kmahip.h"\n'
                 "int use(kmahip_sparse **s, const kmahip_reads *r, kmahip_sparse_row *rows, int64_t *n) {\n"
                 "\tkmahip_sparse_opts o;\n"
                 "\tkmahip_sparse_default_opts(&o);\n"
                 '\treturn kmahip_sparse_open("p", s) + kmahip_sparse_count(*s, r) + kmahip_sparse_rows(*s, &o, rows, 1, n) + kmahip_sparse_write(*s, &o, "x.spa");\n'
                 "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "kmahip_map.c")])


def _lib():
    from kma_amd import binding
    L = binding.lib()          # (builds the library when it is missing or older than its sources)
    L.kmahip_sparse_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    return L


def test_library_exports_the_entry_points():
    L = _lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    from kma_amd import binding
    o = binding.SparseOpts()
    L.kmahip_sparse_default_opts(ctypes.byref(o))
    assert (o.ID_t, o.Depth_t, o.evalue, chr(o.ss)) == (1.0, 0.0, 0.05, "q")


def _refused(L, prefix, *words):
    h = ctypes.c_void_p()
    rc = L.kmahip_sparse_open(str(prefix).encode(), ctypes.byref(h))
    err = L.kmahip_last_error()
    assert rc == -3 and h.value is None, (prefix, rc, err)
    for w in words:
        assert w in err, (prefix, err)


def test_open_refuses_what_it_does_not_serve(tmp_path):
    """a plain index, k = 20, a minimizer flag, a .length.b without unique lengths: KMAHIP_EFORMAT, the reason named, no device call
    (this test runs where there is no device)"""
    L = _lib()
    os.makedirs(tmp_path / "g")
    g = golden_util.load_se(tmp_path / "g")
    _refused(L, g["prefix"], b"not a sparse index", b"DB needs to sparse indexed, to run a sparse mapping.")
    sp = su.unpack_index("se_TG", tmp_path)

    def variant(name):
        p = str(tmp_path / name)
        for ext in (".comp.b", ".length.b", ".name"):
            shutil.copy(sp + ext, p + ext)
        return p
    k20 = variant("k20")
    with open(k20 + ".comp.b", "r+b") as f:          # mlen in the header
        f.seek(4); f.write(struct.pack("<I", 20))
    _refused(L, k20, b"k-mer length 20", b"64-bit keys")
    flag = variant("flag")
    with open(flag + ".comp.b", "r+b") as f:         # the file ends with kmersize, flag
        f.seek(-4, os.SEEK_END); f.write(struct.pack("<I", 1))
    _refused(L, flag, b"minimizer", b"flag 1")
    nolen = variant("nolen")
    D = struct.unpack("<I", open(sp + ".comp.b", "rb").read(4))[0]
    raw = open(sp + ".length.b", "rb").read()
    with open(nolen + ".length.b", "wb") as f:       # what `kma index` without -Sparse writes: one array behind the first
        f.write(raw[:4 + 2 * 4 * D])
    _refused(L, nolen, b"DB needs to sparse indexed, to run a sparse mapping.")
    if os.path.exists(KMA):          # and a k = 20 sparse index as the reference writes it
        fsa = tmp_path / "db.fsa"
        import gzip
        fsa.write_bytes(gzip.open(os.path.join(ROOT, "tests", "golden", "se", "db.fsa.gz")).read())
        subprocess.check_call([KMA, "index", "-i", str(fsa), "-o", str(tmp_path / "ref20"), "-k", "20", "-Sparse", "TG"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        _refused(L, tmp_path / "ref20", b"k-mer length 20")
    # kmahip_db_open keeps refusing the sparse index
    h = ctypes.c_void_p()
    assert L.kmahip_db_open(sp.encode(), ctypes.byref(h)) == -3 and b"sparse" in L.kmahip_last_error()


def refused_commands(tmp):
    fq, o, db = str(tmp / "r.fq"), str(tmp / "out"), str(tmp / "db")
    base = ["-i", fq, "-t_db", db, "-Sparse"]
    return [
        (base + ["-o", o, "-deCon"], "-deCon"),
        (base + ["-o", o, "-gpus", "2"], "-gpus N"),
        (base + ["-o", o, "-s1dev"], "-s1dev"),
        (base + ["-o", "--"], "-o --"),
        (["-Sparse", "-ss", "c"] + base[:4] + ["-o", o, "-deCon"], "-deCon"),
    ]


def test_every_combination_not_built_is_refused_by_name(built, tmp_path):
    for args, what in refused_commands(tmp_path):
        p = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert p.returncode == 2, (args, p.returncode, p.stderr)
        assert b"-Sparse is not built for" in p.stderr and what.encode() in p.stderr, (args, p.stderr)
        assert os.listdir(tmp_path) == [], (args, os.listdir(tmp_path))


def test_a_rank_of_a_sharded_run_refuses(built, tmp_path):
    env = dict(os.environ, KMAHIP_RANK="0", KMAHIP_WORLD="2", KMAHIP_KEY="sparse_cli")
    args = ["-i", str(tmp_path / "r.fq"), "-t_db", str(tmp_path / "db"), "-o", str(tmp_path / "out"), "-Sparse"]
    p = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT, env=env)
    assert p.returncode == 2 and b"-Sparse is not built for -gpus N" in p.stderr, (p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


def test_wrong_ss_gets_the_reference_message_and_the_default(built, tmp_path):
    """kma.c:724-735: the message, and the run goes on with -ss q -- here to the index that is not there (or the device that is not)"""
    args = ["-i", str(tmp_path / "r.fq"), "-t_db", str(tmp_path / "db"), "-o", str(tmp_path / "out"), "-Sparse", "-ss", "x"]
    p = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert b'Invalid argument parsed to option: "-ss", using default.\n' in p.stderr
    assert p.returncode == 1 and b"is not built" not in p.stderr, (p.returncode, p.stderr)
    for ok in "qcd":
        p = subprocess.run([MAP] + args[:-1] + [ok], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert b"Invalid argument" not in p.stderr and p.returncode == 1
    assert os.listdir(tmp_path) == []


def test_served_combinations_pass_the_command_line(built, tmp_path):
    """-i with a list, -ipe and -int with their stderr lines, and mapping options the sparse path never reads: no refusal"""
    fq = str(tmp_path / "r.fq")
    tail = ["-t_db", str(tmp_path / "db"), "-o", str(tmp_path / "out"), "-Sparse"]
    for head, more, line in ((["-i", fq, fq], [], None), (["-ipe", fq, fq], [], b"Paired end information is not considered in Sparse mode.\n"),
                             (["-int", fq], [], b"Interleaved information is not considered in Sparse mode.\n"),
                             (["-i", fq], ["-1t1", "-mem_mode", "-ca", "-ConClave", "2", "-ef", "-matrix", "-vcf", "-apm", "f", "-t", "4", "-ID", "50", "-md", "1", "-e", "0.01"], None)):
        p = subprocess.run([MAP] + head + tail + more, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert b"is not built" not in p.stderr and b"not one this program implements" not in p.stderr, (head, more, p.stderr)
        assert p.returncode == 1, (head, more, p.returncode, p.stderr)      # (no device, or no such index)
        assert line is None or line in p.stderr, (head, p.stderr)


def test_usage_names_the_option(built):
    p = subprocess.run([MAP, "-no_such_option"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert p.returncode == 2 and b"-Sparse [-ss q|c|d]" in p.stderr
