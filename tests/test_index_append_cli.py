"""Appending to an index (`kmahip_index -t_db`, kmahip_index_append) at the boundary, without a GPU: the entry point is declared in
plain C99 and exported, what is not built is refused by name with status 2 before a file or the device is opened, missing input ends
with the reference's recorded words and statuses, and an old index that contradicts its own header, or one this library does not
serve, is refused with the reason in kmahip_last_error before any device call."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest

import dist_util
import index_append_util as iau
import proxi_util
from index_append_util import INDEX, ROOT

TIMEOUT = 60
SYMS = ("kmahip_index_append", "kmahip_test_index_expand", "kmahip_test_index_expand_timing")


@pytest.fixture(scope="module")
def built():
    proxi_util.build_map()


def run(args, **kw):
    return subprocess.run([INDEX] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT, **kw)


def test_entry_point_is_declared_and_the_header_is_c99(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmahip.h")).read(), flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym
    assert "appending (-t_db)" not in open(os.path.join(ROOT, "include", "kmahip.h")).read()
    c = tmp_path / "use.c"
    c.write_text('#include "kmahip.h"\n'
                 "int use(const char *const *a, const char *const *d, uint64_t *pairs, int64_t *n) {\n"
                 '\treturn kmahip_index_append("p", a, 1, d, 1, (const char *) 0) + kmahip_index_append("p", a, 0, d, 1, "q") + kmahip_test_index_expand("p", pairs, 4, n);\n'
                 "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "kmahip_index.c")])


def _lib():
    from kma_amd import binding
    L = binding.lib()
    L.kmahip_index_append.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_char_p]
    L.kmahip_index_append.restype = ctypes.c_int
    return L


def _append(L, db, fasta, decon=(), out=None):
    fa = (ctypes.c_char_p * max(1, len(fasta)))(*[os.fsencode(str(x)) for x in fasta])
    da = (ctypes.c_char_p * max(1, len(decon)))(*[os.fsencode(str(x)) for x in decon])
    rc = L.kmahip_index_append(None if db is None else os.fsencode(str(db)), fa, len(fasta), da, len(decon), None if out is None else os.fsencode(str(out)))
    return rc, L.kmahip_last_error()


def test_library_exports_the_entry_point_and_null_arguments_are_invalid(tmp_path):
    L = _lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    assert _append(L, None, [iau.fasta("b")])[0] == -1
    assert L.kmahip_index_append(b"p", None, 1, None, 0, None) == -1
    assert L.kmahip_index_append(b"p", None, 0, None, 1, None) == -1
    rc, err = _append(L, tmp_path / "db", [])
    assert rc == -1 and b"No inputfiles defined." in err
    rc, err = _append(L, tmp_path / "db", [iau.fasta("b")], decon=["--"])
    assert rc == -1 and b"standard input" in err
    assert os.listdir(tmp_path) == []


def _copy(src, dst):
    for ext in (".comp.b", ".length.b", ".name", ".seq.b"):
        shutil.copy(src + ext, dst + ext)
    return dst


def test_an_index_that_contradicts_its_header_is_wrong_format(tmp_path):
    """hand-patched copies of the fixture's index: KMAHIP_EFORMAT and the reference's words, for the append and for the expansion's
    hook, and nothing written -- no device call is made on such a file (this test runs where there is no device)"""
    L = _lib()
    os.makedirs(tmp_path / "ref")
    good = iau.unpack("A_k16", tmp_path / "ref")
    c = iau.Comp(good + ".comp.b")
    o_values = 52 + 4 * c.size
    o_keys = o_values + 2 * c.v_index
    o_vidx = o_keys + 4 * (c.n + 1)
    first = int(c.vidx[0])
    two = next(int(v) for v in c.vidx.tolist() if c.values[v] >= 2)
    patches = {
        "vidx_past_v_index": (".comp.b", o_vidx, struct.pack("<I", c.v_index + 5)),
        "list_runs_past_v_index": (".comp.b", o_values + 2 * first, struct.pack("<H", 30000)),
        "empty_list": (".comp.b", o_values + 2 * first, struct.pack("<H", 0)),
        "id_of_DB_size": (".comp.b", o_values + 2 * (first + 1), struct.pack("<H", c.DB_size)),
        "id_0": (".comp.b", o_values + 2 * (first + 1), struct.pack("<H", 0)),
        "descending_list": (".comp.b", o_values + 2 * (two + 1), struct.pack("<2H", int(c.values[two + 2]), int(c.values[two + 1]))),
        "more_templates_in_length_b": (".length.b", 0, struct.pack("<I", c.DB_size + 1)),
    }
    os.makedirs(tmp_path / "w")
    for name, (ext, at, data) in patches.items():
        p = _copy(good, str(tmp_path / "w" / name))
        with open(p + ext, "r+b") as f:
            f.seek(at); f.write(data)
        before = {e: open(p + e, "rb").read() for e in (".comp.b", ".length.b", ".name", ".seq.b")}
        for out in (None, tmp_path / "w" / (name + "_out")):
            rc, err = _append(L, p, [iau.fasta("b")], out=out)
            assert rc == -3 and b"Wrong format of DB." in err, (name, rc, err)
        if ext == ".comp.b":
            n = ctypes.c_int64(0)
            buf = (ctypes.c_uint64 * 8)()
            L.kmahip_test_index_expand.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
            assert L.kmahip_test_index_expand(p.encode(), buf, 8, ctypes.byref(n)) == -3 and b"Wrong format of DB." in L.kmahip_last_error(), name
        assert before == {e: open(p + e, "rb").read() for e in before}, name
    short = _copy(good, str(tmp_path / "w" / "short_seq"))
    with open(short + ".seq.b", "r+b") as f:
        f.truncate(os.path.getsize(short + ".seq.b") - 8)
    rc, err = _append(L, short, [iau.fasta("b")])
    assert rc == -3 and b"Wrong format of DB." in err
    assert sorted(os.listdir(tmp_path / "w")) == sorted(n + e for n in list(patches) + ["short_seq"] for e in (".comp.b", ".length.b", ".name", ".seq.b"))


def test_what_is_not_served_is_refused_by_name(tmp_path):
    """the k = 20 index and the minimizer index of tests/golden/tdist, a sparse index with decon files, a missing index: the reason is
    named, before any device call"""
    L = _lib()
    for case, words in (("edge_k20", (b"k-mer length 20", b"64-bit keys")), ("edge_m12", (b"minimizer", b"flag"))):
        p = dist_util.unpack_index(case, tmp_path)
        rc, err = _append(L, p, [iau.fasta("b")])
        assert rc == -3 and all(w in err for w in words), (case, rc, err)
    os.makedirs(tmp_path / "ref")
    sp = iau.unpack("A_TG", tmp_path / "ref")
    for fasta in ([iau.fasta("b")], []):
        rc, err = _append(L, sp, fasta, decon=[iau.fasta("c")], out=tmp_path / "x")
        assert rc == -1 and b"sparse index" in err and b"deConNode_sparse" in err, (rc, err)
    rc, err = _append(L, tmp_path / "none", [iau.fasta("b")])
    assert rc == -2 and b"none.comp.b" in err
    assert sorted(os.listdir(tmp_path)) == sorted(["ref"] + ["td_%s%s" % (c, e) for c in ("edge_k20", "edge_m12") for e in (".comp.b", ".name")])


def test_every_combination_not_built_is_refused_by_name(built, tmp_path):
    db, fa, o = str(tmp_path / "db"), str(tmp_path / "b.fsa"), str(tmp_path / "out")
    for more, what in ((["-hq", "0.9"], b"-hq / -ht are not built with -t_db"), (["-ht", "0.9", "-and"], b"-hq / -ht are not built with -t_db"),
                       (["-Sparse", "TG", "-hq", "0.5", "-ht", "0.5"], b"-hq / -ht are not built with -t_db"), (["-ML", "100"], b"-ML is not built with -t_db"),
                       (["-Sparse", "TG", "-ML", "100"], b"-ML is not built with -t_db"), (["-deCon", "--"], b"standard input")):
        for io in (["-t_db", db, "-i", fa], ["-i", fa, "-o", o, "-t_db", db]):
            p = run(io + more)
            assert p.returncode == 2 and what in p.stderr and p.stdout == b"", (io, more, p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


def test_missing_input_ends_like_the_reference(built, tmp_path):
    for args, status, line in iau.cli_lines():
        p = run(args, cwd=str(tmp_path))
        assert p.returncode == status and p.stderr.split(b"\n")[0] == line.encode(), (args, p.returncode, p.stderr)
    p = run(["-t_db", "x", "-i", "b.fsa", "-Sparse", "TN"], cwd=str(tmp_path))          # a wrong prefix text is still a wrong prefix
    assert p.returncode == 1 and p.stderr == b"Invalid prefix.\n"
    assert os.listdir(tmp_path) == []


def test_served_command_lines_pass(built, tmp_path):
    """in place, decon onto an index, and -k / -Sparse beside -t_db: no refusal; the run ends at the device that is not there or at
    the index that is not"""
    x, y, b, c = (str(tmp_path / n) for n in ("x", "y", "b.fsa", "c.fsa"))
    for args in (["-t_db", x, "-i", b], ["-t_db", x, "-deCon", c], ["-t_db", x, "-i", b, "-o", y, "-k", "16", "-Sparse", "TG"],
                 ["-t_db", x, "-i", b, "-deCon", c, "-o", y], ["-t_db", x, "-Sparse", "TG", "-deCon", c], ["-t_db", x, "-i", b, "-and"]):
        p = run(args)
        assert p.returncode == 1 and p.stderr.startswith(b"kmahip_index: "), (args, p.returncode, p.stderr)
        assert b"is not built" not in p.stderr and b"are not built" not in p.stderr and b"usage" not in p.stderr, (args, p.stderr)
    assert os.listdir(tmp_path) == []


def test_usage_names_the_option(built):
    p = run(["-no_such_option"])
    assert p.returncode == 2 and b"usage: kmahip_index" in p.stderr and b"[-t_db <index to append to>" in p.stderr
