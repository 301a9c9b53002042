"""The command line of proximity matching, as far as examples/kmahip_map goes without a device: the range check of `-proxi` with the
reference's messages (kma.c:702-721), and the combinations `-proxi` / `-ill` are not built for, each refused by name with status 2
before a file or a device is opened."""
import os
import subprocess

import pytest

import proxi_util
from proxi_util import MAP


@pytest.fixture(scope="module")
def built():
    proxi_util.build_map()


def _run(args):
    return subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)


@pytest.mark.parametrize("tail,msg", [(["-proxi", "1.5"], b"Invalid argument at \"-proxi\".\n"), (["-proxi", "-1.01"], b"Invalid argument at \"-proxi\".\n"),
                                      (["-proxi", "0.9x"], b"Invalid argument at \"-proxi\".\n"), (["-proxi"], b"Need argument at: \"-proxi\".\n")])
def test_proxi_value_is_checked_like_the_reference(built, tmp_path, tail, msg):
    p = _run(["-i", str(tmp_path / "r.fq"), "-t_db", str(tmp_path / "db"), "-o", str(tmp_path / "out"), "-1t1"] + tail)
    assert p.returncode == 1 and p.stderr == msg, (p.returncode, p.stderr)


def test_refused_combinations_name_their_reason(built, tmp_path):
    for args, why in proxi_util.refused_commands(tmp_path):
        p = _run(args)
        assert p.returncode == 2, (args, p.returncode, p.stderr)
        assert why.encode() in p.stderr and b"proximity matching serves the single-end -1t1 run" in p.stderr, (args, p.stderr)
    assert os.listdir(tmp_path) == []


def test_usage_lists_the_options(built):
    p = _run([])
    assert p.returncode == 2 and b"[-proxi f] [-ill]" in p.stderr
