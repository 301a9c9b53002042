"""Counting k-mers (`-ck`): the workspace setting in the header, the binding and the command line (no GPU)."""
import ctypes
import inspect
import os
import re
import subprocess

import proxi_util
from proxi_util import MAP, ROOT

HEADER = os.path.join(ROOT, "include", "kmahip.h")


def _params_struct():
    return re.search(r"typedef struct kmahip_params \{(.*?)\} kmahip_params;", open(HEADER).read(), re.S).group(1)


def test_header_declares_the_workspace_setting_and_leaves_the_params_alone():
    src = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kmahip_ws_set_count_kmers\(kmahip_ws \*ws, int on\);", src, re.S)
    assert m, "kmahip_ws_set_count_kmers is declared with its comment"
    # the reference lines it replaces are cited
    for cite in ("kma.c:689", "savekmers.c:3067-3365", ":690-824", "kma.c:1272-1276"):
        assert cite in m.group(1), cite
    # the params structure is the one of before: its layout is shared with every caller
    body = re.sub(r"/\*.*?\*/", "", _params_struct(), flags=re.S)
    fields = re.findall(r"\b(?:int32_t|double|kmahip_rewards)\s+(\w+)\s*;", body)
    assert fields == ["rw", "exhaustive", "minlen", "mq", "scoreT", "mrc", "minFrac", "ts", "apm", "ca"]


def test_library_exports_the_setting_and_refuses_a_null_workspace():
    from kma_amd import binding
    L = binding.lib()
    L.kmahip_ws_set_count_kmers.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.kmahip_ws_set_count_kmers.restype = ctypes.c_int
    assert L.kmahip_ws_set_count_kmers(None, 1) == -1          # KMAHIP_EINVAL, before any device call
    assert [f[0] for f in binding.Params._fields_] == ["rw", "exhaustive", "minlen", "mq", "scoreT", "mrc", "minFrac", "ts", "apm", "ca"]


def test_keyword_on_every_entry_point():
    from kma_amd import binding
    for name in ("scan_se", "scan_pe", "map_se", "map_pe", "run_se", "run_pe", "session"):
        par = inspect.signature(getattr(binding.KmaHipDB, name)).parameters
        assert "count_kmers" in par and par["count_kmers"].default is False, name
    assert inspect.signature(binding.Session.__init__).parameters["count_kmers"].default is False
    assert inspect.signature(binding.KmaHipDB.set_count_kmers).parameters["on"].default is True


def test_kmahip_map_takes_the_option_where_it_stands():
    proxi_util.build_map()
    for args in (["-ck"], ["-1t1", "-ck"], ["-ck", "-Mt1", "1"], ["-ck", "-Sparse"], ["-ck", "-proxi", "0.7", "-1t1"]):
        p = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 2
        assert b"are required" in p.stderr and b"is not one this program implements" not in p.stderr, args


def test_usage_names_the_option():
    proxi_util.build_map()
    p = subprocess.run([MAP, "-no_such_option"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"is not one this program implements" in p.stderr
    assert b"[-ck]" in p.stderr and b"(-ck: count k-mers over pseudo alignment" in p.stderr


def test_no_new_refusal(tmp_path):
    """what is refused beside -ck is what is refused without it, in the same words"""
    proxi_util.build_map()
    for args, why in proxi_util.refused_commands(tmp_path):
        a = subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
        b = subprocess.run([MAP] + args + ["-ck"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
        assert a.returncode == b.returncode == 2 and a.stderr == b.stderr and why.encode() in b.stderr, args
