"""Decontamination (`-deCon`) at the boundary, without a GPU: the two entry points are declared and the header stays plain C99, what
examples/kmahip_map refuses it refuses by name before a file or a device is opened, and a bare `kmahip_index -deCon` ends like the
reference's (index.c:216-219)."""
import os
import re
import subprocess

import pytest

import decon_util
import proxi_util
from decon_util import INDEX, MAP, ROOT

TIMEOUT = 60


@pytest.fixture(scope="module")
def built():
    proxi_util.build_map()


def test_entry_points_are_declared_and_the_header_is_c99(tmp_path):
    src = open(os.path.join(ROOT, "include", "kmahip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in ("kmahip_index_build_decon", "kmahip_db_open_decon", "kmahip_db_is_decon"):
        assert re.search(r"\b%s\s*\(" % sym, src), sym
    c = tmp_path / "use.c"
    c.write_text('#include "kmahip.h"\n'
                 "int use(const char *const *a, const char *const *b, kmahip_db **db) {\n"
                 '\treturn kmahip_index_build_decon(a, 1, b, 1, "p", 16) + kmahip_db_open_decon("p", db) + kmahip_db_is_decon(*db);\n'
                 "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)])
    for prog in ("kmahip_index.c", "kmahip_map.c"):
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-fsyntax-only",
                               "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", prog)])


def test_library_exports_the_entry_points():
    import ctypes
    from kma_amd import binding
    binding.lib()          # (builds the library when it is missing or older than its sources)
    lib = ctypes.CDLL(binding.LIB_PATH)
    for sym in ("kmahip_index_build_decon", "kmahip_db_open_decon", "kmahip_db_is_decon"):
        assert hasattr(lib, sym), sym
    assert lib.kmahip_db_is_decon(None) == 0


def test_every_combination_not_built_is_refused_by_name(built, tmp_path):
    cases = decon_util.refused_commands(tmp_path)
    assert len(cases) == 8
    for args, what in cases:
        p = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert p.returncode == 2, (args, p.returncode, p.stderr)
        assert b"-deCon is not built for" in p.stderr and b"decontamination serves" in p.stderr and what.encode() in p.stderr, (args, p.stderr)
        assert os.listdir(tmp_path) == [], (args, os.listdir(tmp_path))


def test_a_rank_of_a_sharded_run_refuses(built, tmp_path):
    env = dict(os.environ, KMAHIP_RANK="0", KMAHIP_WORLD="2", KMAHIP_KEY="decon_cli")
    args = ["-i", str(tmp_path / "r.fq"), "-t_db", str(tmp_path / "db"), "-o", str(tmp_path / "out"), "-1t1", "-deCon"]
    p = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT, env=env)
    assert p.returncode == 2 and b"-deCon is not built for -gpus N" in p.stderr, (p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []


def test_served_combinations_pass_the_command_line(built, tmp_path):
    """-1t1 single end, -ipe at either pairing and -int, also beside -ca, -ConClave 2, -ill, -s1dev, -ef, -matrix, -vcf and -sam 4: no word
    about decontamination; the run ends at the missing index, which the message names with its decon file"""
    fq, r2 = str(tmp_path / "r.fq"), str(tmp_path / "r2.fq")
    for f in (fq, r2):
        with open(f, "w") as g:
            g.write("@r0\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n")
    tail = ["-t_db", str(tmp_path / "db"), "-o", str(tmp_path / "out"), "-1t1", "-deCon"]
    for head, more in ((["-i", fq], []), (["-ipe", fq, r2], ["-apm", "p"]), (["-ipe", fq, r2], ["-apm", "u"]), (["-ipe", fq, r2], []), (["-int", fq], []),
                       (["-i", fq], ["-ca", "-ConClave", "2", "-ef", "-matrix", "-vcf"]), (["-i", fq], ["-ill"]), (["-i", fq], ["-s1dev"]),
                       (["-i", fq], ["-sam", "4"])):
        p = subprocess.run([MAP] + head + tail + more, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert b"is not built" not in p.stderr and b"not one this program implements" not in p.stderr, (head, more, p.stderr)
        assert p.returncode == 1 and b"kmahip_map: open" in p.stderr, (head, more, p.returncode, p.stderr)      # (no device, or no such index)


def test_usage_names_the_option(built, tmp_path):
    p = subprocess.run([MAP, "-no_such_option"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert p.returncode == 2 and b"[-deCon]" in p.stderr


def test_bare_index_decon_exits_1_with_the_reference_message(built, tmp_path):
    for args in (["-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db"), "-deCon"], ["-deCon", "-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db")]):
        p = subprocess.run([INDEX] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
        assert p.returncode == 1 and p.stderr == b"No deCon file specified.\n", (args, p.returncode, p.stderr)
    p = subprocess.run([INDEX, "-i", str(tmp_path / "db.fsa"), "-o", str(tmp_path / "db"), "-deCon", "--"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert p.returncode == 2 and b"standard input" in p.stderr, (p.returncode, p.stderr)
    assert os.listdir(tmp_path) == []
