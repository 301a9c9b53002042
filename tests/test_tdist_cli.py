"""Template distances (`kma dist`) at the boundary, without a GPU: the entry points are declared and exported and the header and
examples/kmahip_dist.c stay plain C99; the texts and exit statuses of `kmahip_dist` for -dh, -fh, -h, missing and bad arguments,
unknown options and too few arguments are the reference's (recorded in tests/golden/tdist/cli.json, and the reference binary run live
where it is built), all before a device is opened; kmahip_tdist_open refuses a short file in the reference's words before any device
call."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import dist_util as du
from dist_util import DIST, KMA, ROOT

TIMEOUT = 60
SYMS = ("kmahip_tdist_open", "kmahip_tdist_open_lists", "kmahip_tdist_close", "kmahip_tdist_get_info", "kmahip_tdist_name", "kmahip_tdist_count",
        "kmahip_tdist_get_counts", "kmahip_tdist_write", "kmahip_test_tdist_cells", "kmahip_tdist_set_timing", "kmahip_tdist_get_timing")
CLI = json.load(open(os.path.join(du.GOLDEN, "cli.json")))


@pytest.fixture(scope="module")
def built():
    from kma_amd import binding
    binding.lib()          # (the program links against the library)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "kmahip_dist"], stdout=subprocess.DEVNULL)


def test_entry_points_are_declared_and_the_sources_are_c99(tmp_path):
    src = open(os.path.join(ROOT, "include", "kmahip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym
    c = tmp_path / "use.c"
    c.write_text('#include "kmahip.h"\n'
                 "int use(kmahip_tdist **td, int32_t *N, int32_t *D) {\n"
                 "\tkmahip_tdist_info info;\n"
                 '\treturn kmahip_tdist_open("p", td) + kmahip_tdist_get_info(*td, &info) + kmahip_tdist_count(*td) + kmahip_tdist_get_counts(*td, N, D, 0, 1)\n'
                 '\t       + kmahip_tdist_write(*td, "x.phy", 8191, 5);\n'
                 "}\n")
    flags = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(flags + [str(c)])
    subprocess.check_call(flags + [os.path.join(ROOT, "examples", "kmahip_dist.c")])


def _lib():
    from kma_amd import binding
    L = binding.lib()          # (builds the library when it is missing or older than its sources)
    L.kmahip_tdist_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    return L


def test_library_exports_the_entry_points():
    L = _lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym


@pytest.mark.parametrize("rec", CLI, ids=[" ".join(r["args"]) or "none" for r in CLI])
def test_texts_and_statuses_are_the_reference_s(built, rec, tmp_path):
    p = subprocess.run([DIST] + rec["args"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT, cwd=str(tmp_path))
    assert (p.returncode, p.stdout.decode(), p.stderr.decode()) == (rec["status"], rec["stdout"], rec["stderr"])
    assert os.listdir(tmp_path) == []
    if os.path.exists(KMA):
        r = subprocess.run([KMA, "dist"] + rec["args"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT, cwd=str(tmp_path))
        assert (r.returncode, r.stdout, r.stderr) == (p.returncode, p.stdout, p.stderr)


def test_the_recorded_command_lines_cover_what_they_should():
    got = {tuple(r["args"]) for r in CLI}
    assert got == {tuple(a) for a in du.CLI_CASES}
    err = "".join(r["stderr"] for r in CLI)
    for words in ("Too few arguments handed.", "Missing argument at", "Invalid value parsed at", "Unknown option:", "Unknown argument:"):
        assert words in err


def test_open_refuses_a_short_or_inconsistent_file_in_the_reference_s_words(tmp_path):
    """KMAHIP_EFORMAT with `Wrong format of DB.`, no device call (this test runs where there is no device)"""
    L = _lib()
    p = du.unpack_index("two", tmp_path)
    raw = open(p + ".comp.b", "rb").read()
    q = str(tmp_path / "bad")
    with open(q + ".name", "wb") as f:
        f.write(open(p + ".name", "rb").read())
    old = bytearray(raw)
    old[20:28] = (0).to_bytes(8, "little")          # size below n: what loadValues takes for an old index
    for body in (raw[:20], raw[:60], raw[:len(raw) - 200], raw[:len(raw) - 4], bytes(old)):
        with open(q + ".comp.b", "wb") as f:
            f.write(body)
        h = ctypes.c_void_p()
        rc = L.kmahip_tdist_open(q.encode(), ctypes.byref(h))
        assert rc == -3 and h.value is None and b"Wrong format of DB." in L.kmahip_last_error(), (len(body), rc, L.kmahip_last_error())
    h = ctypes.c_void_p()
    assert L.kmahip_tdist_open(str(tmp_path / "none").encode(), ctypes.byref(h)) == -2


def test_open_refuses_a_list_the_kernels_could_not_walk(tmp_path):
    """the reference walks the value lists unchecked; here a list that leaves the value array, or holds a template the database does
    not have, is the wrong format -- found on the host before any device call"""
    L = _lib()
    p = du.unpack_index("two", tmp_path)
    v = du.Values(p)
    raw = bytearray(open(p + ".comp.b", "rb").read())
    at = 52 + 4 * v.size          # the values of the hashed form, 16-bit
    first = int(v.exist[0])
    for word, what in ((0xFFF0, b"runs past the value array"), (None, b"not in the database")):
        bad = bytearray(raw)
        o = at + 2 * first if word is not None else at + 2 * (first + 1)
        bad[o:o + 2] = (word if word is not None else v.DB_size).to_bytes(2, "little")
        q = str(tmp_path / "badlist")
        with open(q + ".comp.b", "wb") as f:
            f.write(bytes(bad))
        with open(q + ".name", "wb") as f:
            f.write(open(p + ".name", "rb").read())
        h = ctypes.c_void_p()
        rc = L.kmahip_tdist_open(q.encode(), ctypes.byref(h))
        err = L.kmahip_last_error()
        assert rc == -3 and h.value is None and b"Wrong format of DB." in err and what in err, (rc, err)
