"""`kmahip_map -qc` and `kmahip_trim` on the command line, as far as no GPU is needed: option messages and statuses, every refusal by
name with nothing created, the usage texts, and kmahip_trim's host path whole against the recorded files."""
import os
import re
import subprocess

import pytest

import proxi_util
import qc_util
from proxi_util import MAP, ROOT

TRIM = os.path.join(ROOT, "examples", "kmahip_trim")
HEADER = os.path.join(ROOT, "include", "kmahip.h")
P33 = qc_util.path_of("p33.fq")
WRAP = os.path.join(qc_util.ING, "wrap.fa")


@pytest.fixture(scope="module", autouse=True)
def _built():
    proxi_util.build_map()


def _run(prog, args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("KMAHIP_RANK", "RANK", "KMAHIP_MAP_ONE_BATCH", "KMAHIP_COMM_FORCE_RCCL")}
    e.update(env or {})
    return subprocess.run([prog] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_header_declares_the_entry_points_with_the_lines_they_replace():
    src = open(HEADER).read()
    for name, cites in (("kmahip_qc_open", ("qc.c:24-48",)), ("kmahip_ingest_set_qc", ("runinput.c:127-313", "runinput.c:359-361")),
                        ("kmahip_ingest_dev_set_qc", ("runinput.c:127-313",)), ("kmahip_qc_write", ("qc.c:167-262", "kma.c:1555-1557")),
                        ("kmahip_ingest_set_text", ("trim.c:28-126",)), ("kmahip_trim_files", ("trim.c:149-472",))):
        at = src.index(name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        for c in cites:
            assert c in comment, (name, c)
    assert "typedef struct kmahip_qc_stats {" in src and "uint32_t ldist[512];" in src


# ---- kmahip_map -qc --------------------------------------------------------------------------------------------------------------------
def test_kmahip_map_takes_the_option_and_names_it_in_its_usage():
    for args in (["-qc"], ["-1t1", "-qc", "-5p", "3", "-3p", "2"], ["-qc", "-Sparse"]):
        p = _run(MAP, args)
        assert p.returncode == 2 and b"are required" in p.stderr and b"is not one this program implements" not in p.stderr, args
    p = _run(MAP, ["-no_such_option"])
    assert p.returncode == 2 and b"[-qc] [-5p n] [-3p n]" in p.stderr and b"(-qc: the QC report <output prefix>.json" in p.stderr


def test_kmahip_map_refuses_by_name_and_creates_nothing(tmp_path):
    out = str(tmp_path / "o")
    base = ["-t_db", str(tmp_path / "db"), "-o", out, "-1t1", "-qc"]
    cases = [
        (["-i", WRAP] + base, {}, "FASTA input"),
        (["-i", P33, WRAP] + base, {}, "FASTA input"),
        (["-i", P33, "-ml", "0"] + base, {}, "-ml below 1"),
        (["-i", P33] + base + ["-qc"], {}, "a second -qc"),
        (["-i", P33, "-gpus", "2"] + base, {}, "-gpus N"),
        (["-i", P33] + base, {"KMAHIP_RANK": "0", "KMAHIP_WORLD": "2"}, "-gpus N"),
        (["-i", P33] + base, {"RANK": "0", "WORLD_SIZE": "2"}, "-gpus N"),
        (["-i", P33] + base, {"KMAHIP_MAP_ONE_BATCH": "1"}, "KMAHIP_MAP_ONE_BATCH"),
        (["-i", "--"] + base, {}, "-i --"),
        (["-i", P33, "-Sparse"] + base + ["-qc"], {}, "a second -qc"),
        (["-i", WRAP, "-Sparse"] + base, {}, "FASTA input"),
    ]
    for args, env, why in cases:
        p = _run(MAP, args, env)
        assert p.returncode == 2, (args, p.returncode, p.stderr)
        assert b"kmahip_map: -qc is not built for " in p.stderr and why.encode() in p.stderr, (args, p.stderr)
        assert os.listdir(tmp_path) == [], args
    # without -qc the same command lines are what they were: not refused for any of these reasons
    p = _run(MAP, ["-i", P33, "-ml", "0", "-t_db", str(tmp_path / "db"), "-o", out, "-1t1", "-gpus", "1"])
    assert b"-qc" not in p.stderr


# ---- kmahip_trim -----------------------------------------------------------------------------------------------------------------------
def test_kmahip_trim_option_messages_and_statuses(tmp_path):
    out = ["-o", str(tmp_path / "o")]
    for args, status, msg in (
        (["-i"], 1, b"No files were specified.\n"),
        (["-ipe", P33], 1, b"Uneven number of paired end files.\n"),
        (["-ipe"], 1, b"No paired end files were specified.\n"),
        (["-int"], 1, b"No interleaved files were specified.\n"),
        (["-i", P33, "-ml", "1x"], 1, b"# Invalid minimum length parsed\n"),
        (["-i", P33, "-xl", "x"], 1, b"# Invalid minimum length parsed\n"),
        (["-i", P33, "-mp", "2.5"], 1, b"# Invalid minimum phred score parsed\n"),
        (["-i", P33, "-mi", "q"], 1, b"# Invalid internal minimum phred score parsed\n"),
        (["-i", P33, "-eq", "q"], 1, b"# Invalid average quality score parsed\n"),
        (["-i", P33, "-5p", "q"], 1, b"Invalid argument at \"-5p\".\n"),
        (["-i", P33, "-3p", "q"], 4, b"Invalid argument at \"-3p\".\n"),
    ):
        p = _run(TRIM, args + out)
        assert (p.returncode, p.stderr) == (status, msg), args
    p = _run(TRIM, ["-i", P33, "-bogus"] + out)
    assert p.returncode == 1 and p.stderr.startswith(b" Invalid option:\t-bogus\n Printing help message:\n#kmahip_trim trims sequences\n")
    h = _run(TRIM, ["-h"])
    assert h.returncode == 0 and h.stderr == b"" and h.stdout == p.stderr.split(b"Printing help message:\n", 1)[1]
    for opt in (b"-i", b"-ipe", b"-int", b"-o", b"-qc", b"-ml", b"-xl", b"-mp", b"-mi", b"-eq", b"-5p", b"-3p", b"-s1dev", b"-h"):
        assert re.search(rb"^# +" + re.escape(opt) + rb"\t", h.stdout, re.M), opt
    assert os.listdir(tmp_path) == []


def test_kmahip_trim_refuses_by_name_and_creates_nothing(tmp_path):
    out = ["-o", str(tmp_path / "o")]
    for args, env, why in (
        (["-i", WRAP] + out, {}, b"FASTA input"),
        (["-i", P33, "-ipe", P33, WRAP] + out, {}, b"FASTA input"),
        (["-i", P33], {}, b"a run without -o"),
        (["-i", "--"] + out, {}, b"-- (reads on standard input)"),
        (["-int", P33, "--"] + out, {}, b"-- (reads on standard input)"),
        (["-qc"] + out, {}, b"a run without input files"),
        (["-i", P33] + out, {"KMAHIP_RANK": "1"}, b"several ranks"),
        (["-i", P33] + out, {"RANK": "0"}, b"several ranks"),
        (["-i", P33, "-qc", "-qc"] + out, {}, b"a second -qc"),
        (["-i", P33, "-qc", "-ml", "0"] + out, {}, b"-ml below 1"),
    ):
        p = _run(TRIM, args, env)
        assert p.returncode == 2 and b"kmahip_trim: " in p.stderr and why in p.stderr, (args, p.returncode, p.stderr)
        assert os.listdir(tmp_path) == [], args


@pytest.mark.parametrize("case", sorted(qc_util.CASES))
def test_kmahip_trim_host_path_writes_the_recorded_files(case, tmp_path):
    se, pe, il = qc_util.CASES[case]
    args = (["-i"] + [qc_util.path_of(f) for f in se] if se else []) + (["-ipe"] + [qc_util.path_of(f) for f in pe] if pe else []) + (["-int"] + [qc_util.path_of(f) for f in il] if il else [])
    for setting in ("default", "eq15", "mi25clip", "ml1000"):
        out = str(tmp_path / setting)
        p = _run(TRIM, args + ["-o", out, "-qc"] + qc_util.ref_flags(setting))
        assert p.returncode == 0, p.stderr
        assert open(out + ".json", "rb").read() == qc_util.gold(case, setting, "json"), (case, setting)
        assert open(out + ".fq", "rb").read() == qc_util.gold(case, setting, "fq"), (case, setting)
        int_fq = qc_util.gold(case, setting, "int_fq")
        assert os.path.exists(out + "_int.fq") == (int_fq is not None)
        assert int_fq is None or open(out + "_int.fq", "rb").read() == int_fq
        frags = qc_util.stats_of_json(qc_util.gold(case, setting, "json"))["Fragment Count"]
        assert p.stderr == b"#\n# Total number of query fragment after trimming:\t%d\n" % frags
    # without -qc no report, and the plain trimming rule
    out = str(tmp_path / "plain")
    assert _run(TRIM, args + ["-o", out]).returncode == 0 and not os.path.exists(out + ".json")
    assert open(out + ".fq", "rb").read() == qc_util.restate(case, "default", report=False)["fq"]
