"""Homology reduction (`kmahip_index -Sparse ... -hq / -ht / -and`) at the boundary, without a GPU: the entry point is declared in plain
C99 and exported, the options are parsed with the reference's words and statuses (index.c:309-350), `-ht` with `-ML` is refused by name
before anything is opened, and what is served passes the command line (the run then ends at the missing input or device)."""
import os
import re
import subprocess

import pytest

import proxi_util
from hom_util import INDEX, ROOT

TIMEOUT = 60


@pytest.fixture(scope="module")
def built():
    proxi_util.build_map()


def run(args):
    return subprocess.run([INDEX] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)


def test_entry_point_is_declared_and_the_header_is_c99(tmp_path):
    text = open(os.path.join(ROOT, "include", "kmahip.h")).read()
    at = text.index("int kmahip_index_build_sparse_hom(")
    assert "qualcheck.c" in text[text.rindex("/*", 0, at):at]
    c = tmp_path / "use.c"
    c.write_text('#include "kmahip.h"\n'
                 "int use(const char *const *a) {\n"
                 '\treturn kmahip_index_build_sparse_hom(a, 1, "p", 16, 16, "TG", 0, 0.9, 0.9, 1, (const char *) 0);\n'
                 "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "kmahip_index.c")])


def test_library_exports_the_entry_point_and_refuses_bad_arguments(tmp_path):
    import ctypes
    from kma_amd import binding
    binding.lib()
    lib = ctypes.CDLL(binding.LIB_PATH)
    assert hasattr(lib, "kmahip_index_build_sparse_hom") and hasattr(lib, "kmahip_index_build_sparse")
    fa = tmp_path / "t.fsa"
    fa.write_text(">t\n" + "ACGTTGCA" * 40 + "\n")
    # (refused on the arguments alone, before a file or the device is opened)
    with pytest.raises(binding.KmaHipError, match="-ht with -ML"):
        binding.index_build(str(fa), str(tmp_path / "x"), sparse="TG", min_len=100, hom_t=0.9)
    with pytest.raises(binding.KmaHipError, match="not below 0"):
        binding.index_build(str(fa), str(tmp_path / "x"), sparse="TG", hom_q=-0.5)
    assert sorted(os.listdir(tmp_path)) == ["t.fsa"]


@pytest.mark.parametrize("opt", ["-hq", "-ht"])
def test_text_behind_the_number_ends_like_the_reference(built, tmp_path, opt):
    for value in ("0.5x", "x", "0.5,"):
        p = run(["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db"), "-Sparse", "TG", opt, value])
        assert p.returncode == 1 and p.stderr == ('Invalid argument at "%s".\n' % opt).encode() and p.stdout == b"", (value, p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("opt", ["-hq", "-ht"])
def test_a_negative_value_is_named_and_becomes_one(built, tmp_path, opt):
    """`Invalid -hq` for both options, as the reference says it; the value becomes 1 and the run goes on (here: to the missing -o)"""
    p = run(["-i", str(tmp_path / "db.fsa"), "-Sparse", "TG", opt, "-0.5"])
    assert p.returncode == 2 and p.stderr.startswith(b"Invalid -hq\n") and b"-i and -o are required" in p.stderr, (p.returncode, p.stderr)
    # -ht -1 is 1 afterwards: beside -ML it is no templateCheck, so nothing is refused
    p = run(["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db"), "-Sparse", "TG", "-ML", "300", opt, "-1"])
    assert p.returncode == 1 and p.stderr.startswith(b"Invalid -hq\n") and b"not built" not in p.stderr, (p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


def test_ht_with_ml_is_refused_by_name_and_hq_with_ml_is_served(built, tmp_path):
    base = ["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db"), "-Sparse", "TG", "-ML", "300"]
    for more in (["-ht", "0.9"], ["-ht", "0.9", "-hq", "0.9", "-and"], ["-hq", "0.5", "-ht", "0"]):
        p = run(base + more)
        assert p.returncode == 2 and b"-ht is not built with -ML" in p.stderr and b"qualcheck.c:287" in p.stderr, (more, p.returncode, p.stderr)
    for more in (["-hq", "0.9"], ["-hq", "0.9", "-and"], ["-ht", "1", "-hq", "0.9"]):
        p = run(base + more)
        assert p.returncode == 1 and b"not built" not in p.stderr and b"usage" not in p.stderr, (more, p.returncode, p.stderr)          # (no device, or no such file)
    p = run(["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db"), "-Sparse", "TG", "-hq", "0.9", "-deCon", str(tmp_path / "host.fsa")])
    assert p.returncode == 2 and b"-Sparse is not built for -deCon" in p.stderr
    assert os.listdir(tmp_path) == []


def test_without_sparse_the_options_are_taken_without_effect(built, tmp_path):
    for more in (["-hq", "0.5"], ["-ht", "0.5", "-and"], ["-and"], ["-hq"]):
        p = run(["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db")] + more)
        assert p.returncode == 1 and p.stderr.startswith(b"kmahip_index: ") and b"usage" not in p.stderr and p.stdout == b"", (more, p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


def test_usage_names_the_options(built):
    p = run(["-no_such_option"])
    assert p.returncode == 2 and all(w in p.stderr for w in (b"[-hq <", b"[-ht <", b"[-and]")), p.stderr
    assert re.search(rb"-Sparse \[<prefix>\|-\] \[-ML <minimum length>\] \[-hq", p.stderr)
