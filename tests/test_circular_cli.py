"""Circular alignments (`-ca`) and the presets `-mint2` / `-mint3`: the flag in the header, the binding and the command line (no GPU)."""
import ctypes
import re
import subprocess

import circ_util as cu


def _params_struct():
    src = open(cu.HEADER).read()
    return re.search(r"typedef struct kmahip_params \{(.*?)\} kmahip_params;", src, re.S).group(1)


def test_header_declares_the_field_last():
    body = re.sub(r"/\*.*?\*/", "", _params_struct(), flags=re.S)
    fields = re.findall(r"\b(?:int32_t|double|kmahip_rewards)\s+(\w+)\s*;", body)
    assert fields[-1] == "ca" and "int32_t ca;" in " ".join(body.split())
    # what it selects is cited
    assert "chain.c:262" in _params_struct() and "kma.c:722" in _params_struct()


def test_binding_mirrors_the_struct_and_defaults_to_plain_chaining():
    from kma_amd import binding
    assert binding.Params._fields_[-1] == ("ca", ctypes.c_int32)
    p = binding.default_params()
    assert p.ca == 0
    # the fields in front of it lie where they lay: the new one is appended
    assert [f[0] for f in binding.Params._fields_[:-1]] == ["rw", "exhaustive", "minlen", "mq", "scoreT", "mrc", "minFrac", "ts", "apm"]


def test_keyword_on_every_entry_point():
    import inspect
    from kma_amd import binding
    for name in ("map_se", "map_pe", "align_se_dev", "align_pe_dev", "align_trace", "align_trace_mt1", "run_se", "run_pe", "run_mt1"):
        par = inspect.signature(getattr(binding.KmaHipDB, name)).parameters
        assert "circular" in par and par["circular"].default is False, name


def test_kmahip_map_takes_the_three_options():
    cu.build_map()
    p = subprocess.run([cu.MAP, "-ca", "-mint2", "-mint3"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2
    assert b"are required" in p.stderr and b"is not one this program implements" not in p.stderr


def test_usage_names_the_three_options():
    cu.build_map()
    p = subprocess.run([cu.MAP, "-no_such_option"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 2 and b"is not one this program implements" in p.stderr
    for opt in (b"[-ca]", b"[-mint2]", b"[-mint3]", b"[-proxi f] [-ill]"):
        assert opt in p.stderr, opt
