"""Sparse index building (`kmahip_index -Sparse`) at the boundary, without a GPU: the entry point is declared and exported, a wrong
prefix ends like the reference's (index.c:464-472), what is not built is refused by name before a file or the device is opened, and
kmahip_index_build_sparse refuses a wrong k or prefix with the reason in kmahip_last_error before any device call."""
import ctypes
import os
import re
import subprocess

import pytest

import proxi_util
from sparse_index_util import INDEX, ROOT

TIMEOUT = 60
SYM = "kmahip_index_build_sparse"


@pytest.fixture(scope="module")
def built():
    proxi_util.build_map()


def run(args):
    return subprocess.run([INDEX] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)


def test_entry_point_is_declared_and_the_header_is_c99(tmp_path):
    src = open(os.path.join(ROOT, "include", "kmahip.h")).read()
    cites = re.findall(r"/\*((?:(?!\*/).)*?)\*/\s*int %s\s*\(" % SYM, src, flags=re.S)
    assert len(cites) == 1
    for ref in ("index.c:451-474", "576-613", "makeindex.c", "updateindex.c:79-199", "qualcheck.c:31-79", "hashmap.c:120-187"):
        assert ref in cites[0], ref
    c = tmp_path / "use.c"
    c.write_text('#include "kmahip.h"\n'
                 "int use(const char *const *a) {\n"
                 '\treturn kmahip_index_build_sparse(a, 1, "p", 16, 16, "TG", 0);\n'
                 "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "kmahip_index.c")])


def _lib():
    from kma_amd import binding
    L = binding.lib()          # (builds the library when it is missing or older than its sources)
    assert hasattr(L, SYM)
    L.kmahip_index_build_sparse.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.kmahip_index_build_sparse.restype = ctypes.c_int
    L.kmahip_last_error.restype = ctypes.c_char_p
    return L


def test_library_refuses_a_wrong_k_or_prefix_before_any_file_or_device(tmp_path):
    L = _lib()
    arr = (ctypes.c_char_p * 1)(os.fsencode(str(tmp_path / "missing.fsa")))
    out = os.fsencode(str(tmp_path / "x"))
    for k, prefix, words in ((3, b"TG", (b"k-mer length 3",)), (17, b"TG", (b"k-mer length 17",)), (16, b"T" * 17, (b"17 bases", b"at most 16")),
                             (16, None, (b"null prefix",)), (16, b"", (b"Invalid prefix.",)), (16, b"TN", (b"Invalid prefix.",)), (16, b"T-", (b"Invalid prefix.",))):
        rc = L.kmahip_index_build_sparse(arr, 1, out, k, k, prefix, 0)
        err = L.kmahip_last_error()
        assert rc == -1, (k, prefix, rc, err)
        for w in words:
            assert w in err, (k, prefix, err)
    # a served combination gets as far as the file that is not there
    for prefix in (b"TG", b"-", b"rYkm", b"A" * 16):
        assert L.kmahip_index_build_sparse(arr, 1, out, 16, 16, prefix, 0) == -2 and b"missing.fsa" in L.kmahip_last_error()
    assert os.listdir(tmp_path) == []


def test_binding_keeps_the_modes_apart(tmp_path):
    from kma_amd import binding
    with pytest.raises(ValueError, match="decon"):
        binding.index_build(str(tmp_path / "a.fsa"), str(tmp_path / "x"), sparse="TG", decon=[str(tmp_path / "h.fsa")])
    with pytest.raises(ValueError, match="min_len"):
        binding.index_build(str(tmp_path / "a.fsa"), str(tmp_path / "x"), min_len=60)
    with pytest.raises(binding.KmaHipError, match="Invalid prefix"):
        binding.index_build(str(tmp_path / "a.fsa"), str(tmp_path / "x"), sparse="TN")
    assert os.listdir(tmp_path) == []


def test_invalid_prefix_ends_like_the_reference(built, tmp_path):
    io = ["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db")]
    for args in (io + ["-Sparse", "TN"], io + ["-Sparse", ""], ["-Sparse", "TN"] + io, io + ["-k", "12", "-Sparse", "T G"],
                 ["-i", str(tmp_path / "db.fsa"), "-Sparse", "-o", str(tmp_path / "db")]):          # (-Sparse takes the next argument whatever it is)
        p = run(args)
        assert p.returncode == 1 and p.stderr == b"Invalid prefix.\n", (args, p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


def test_sparse_with_decon_is_refused_by_name(built, tmp_path):
    host = tmp_path / "host.fsa"
    host.write_text(">h\nACGTACGTACGTACGTACGTACGTACGT\n")
    io = ["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db")]
    for args in (io + ["-Sparse", "TG", "-deCon", str(host)], io + ["-deCon", str(host), "-Sparse", "-"], io + ["-deCon", str(host), "-Sparse"]):
        p = run(args)
        assert p.returncode == 2, (args, p.returncode, p.stderr)
        assert b"-Sparse is not built for -deCon" in p.stderr, (args, p.stderr)
        assert os.listdir(tmp_path) == ["host.fsa"]


def test_plain_build_with_ml_is_refused_by_name(built, tmp_path):
    io = ["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db")]
    for args in (io + ["-ML", "60"], ["-ML", "60"] + io + ["-k", "12"], io + ["-ML", "60", "-deCon", str(tmp_path / "h.fsa")]):
        p = run(args)
        assert p.returncode == 2 and b"-ML is not built for" in p.stderr, (args, p.returncode, p.stderr)
    p = run(io + ["-Sparse", "TG", "-ML", "6x"])
    assert p.returncode == 1 and p.stderr == b"# Invalid minimum length parsed\n"
    assert os.listdir(tmp_path) == []


def test_served_command_lines_pass(built, tmp_path):
    """-Sparse with a prefix, with `-`, as the last argument, with -ML and -k: no refusal; the run ends at the device that is not there
    or at the FASTA file that is not"""
    io = ["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db")]
    for more in (["-Sparse", "TG"], ["-Sparse", "-"], ["-Sparse"], ["-Sparse", "atg", "-ML", "100", "-k", "12"], ["-ML", "0", "-Sparse", "TG"]):
        p = run(io + more)
        assert p.returncode == 1 and b"is not built" not in p.stderr and b"usage" not in p.stderr and b"Invalid prefix" not in p.stderr, (more, p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


def test_usage_names_the_options(built):
    p = run(["-no_such_option"])
    assert p.returncode == 2 and b"usage: kmahip_index" in p.stderr
    assert b"-Sparse [<prefix>|-]" in p.stderr and b"-ML <minimum length>" in p.stderr and b"-deCon" in p.stderr
