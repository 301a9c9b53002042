"""`-ConClave n` on examples/kmahip_map's command line (kma.c:493-501): what is taken, what is refused and how, all before a file or a
device is opened (no GPU)."""
import os
import subprocess

import pytest

import proxi_util
from proxi_util import MAP

TIMEOUT = 60


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    proxi_util.build_map()
    tmp = tmp_path_factory.mktemp("cc2_cli")
    return tmp, ["-i", str(tmp / "r.fq"), "-t_db", str(tmp / "db"), "-o", str(tmp / "out")]


def _run(args):
    return subprocess.run([MAP] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)


@pytest.mark.parametrize("value", ["3", "x", "2x", "-1", "-1t1"], ids=["above", "text", "trailing_text", "negative", "an_option"])
def test_bad_version_exits_1_with_the_reference_message(base, value):
    """(the reference takes the next argument whatever it is: an option in its place is a bad value too)"""
    tmp, args = base
    p = _run(args + ["-1t1", "-ConClave", value])
    assert p.returncode == 1 and b" Invalid ConClave version specified.\n" in p.stderr, (p.returncode, p.stderr)
    assert not os.path.exists(str(tmp / "out.res"))


def test_version_0_is_refused_by_name(base):
    tmp, args = base
    p = _run(args + ["-1t1", "-ConClave", "0"])
    assert p.returncode == 2 and b"-ConClave 0" in p.stderr, (p.returncode, p.stderr)
    assert not os.path.exists(str(tmp / "out.res"))


@pytest.mark.parametrize("mode", [["-1t1"], [], ["-1t1", "-mem_mode"]], ids=["1t1", "default", "mem_mode"])
def test_version_2_with_several_ranks_is_refused_by_name(base, mode):
    tmp, args = base
    p = _run(args + mode + ["-ConClave", "2", "-gpus", "2"])
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert b"-ConClave 2" in p.stderr and b"serves the runs of one rank" in p.stderr and b"-gpus N" in p.stderr, p.stderr
    assert not os.path.exists(str(tmp / "out.res"))


def test_version_2_in_a_rank_of_a_sharded_run_is_refused(base):
    tmp, args = base
    env = dict(os.environ, KMAHIP_RANK="0", KMAHIP_WORLD="2", KMAHIP_KEY="cc2_cli")
    p = subprocess.run([MAP] + args + ["-1t1", "-ConClave", "2"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT, env=env)
    assert p.returncode == 2 and b"-ConClave 2" in p.stderr and b"serves the runs of one rank" in p.stderr, (p.returncode, p.stderr)


@pytest.mark.parametrize("tail", [["-ConClave"], ["-ConClave", "1"], ["-ConClave", "2"]], ids=["bare", "1", "2"])
def test_accepted_as_far_as_the_next_check(base, tail):
    """a trailing `-ConClave` without a value leaves version 1 (kma.c:495); 1 and 2 are taken: ConClave's own checks pass and a later one
    of the command line ends the run, before a file or a device is opened"""
    tmp, args = base
    if tail == ["-ConClave"]:
        # version 1 stays, so several ranks are no matter of ConClave's: the check that fires is -sam's own about them
        p = _run(args + ["-1t1", "-gpus", "2", "-sam", "4"] + tail)
        assert p.returncode == 2 and b"-sam is not built for -gpus N" in p.stderr and b"ConClave" not in p.stderr, (p.returncode, p.stderr)
    else:
        p = _run(args + ["-1t1"] + tail + ["-sam", "4", "-status"])
        assert p.returncode == 2 and b'"-sam" and "-status" cannot coincide.' in p.stderr and b"ConClave" not in p.stderr, (p.returncode, p.stderr)
    assert not os.path.exists(str(tmp / "out.res"))


def test_usage_names_the_option(base):
    tmp, args = base
    p = _run(args + ["-no_such_option"])
    assert p.returncode == 2 and b"-ConClave n" in p.stderr


def test_mt1_takes_version_2_and_ignores_it(base):
    """runKMA_Mt1 runs no ConClave: the option passes, several ranks or not (a later check of the command line ends the run)"""
    tmp, args = base
    p = _run(args + ["-Mt1", "1", "-ConClave", "2", "-gpus", "2", "-sam", "4", "-status"])
    assert p.returncode == 2 and b'"-sam" and "-status" cannot coincide.' in p.stderr and b"ConClave" not in p.stderr, (p.returncode, p.stderr)
