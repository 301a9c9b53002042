"""The QC report and the trimmed reads from the device's stage 1 (kmahip_ingest_dev_set_qc: the records kernel's -qc instantiation and
s1_qc_kernel) against what the reference recorded in tests/golden/qc, against the host reader field by field, and `kmahip_map -qc` /
`kmahip_trim -s1dev` whole against the reference binary run live."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import qc_util
from kma_amd import binding, formats, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")
TRIM = os.path.join(ROOT, "examples", "kmahip_trim")
# the cases whose files the device reader covers (plain FASTQ, single end or two mate files); long.fq.gz is unpacked first
DEV_CASES = ["p33", "dos", "p64", "pe", "long", "uni", "one", "p33+p64"]


def _plain(name, tmp_path):
    p = qc_util.path_of(name)
    if not p.endswith(".gz"):
        return p
    out = str(tmp_path / os.path.basename(p)[:-3])
    if not os.path.exists(out):
        with open(out, "wb") as f:
            f.write(gzip.open(p).read())
    return out


def _dev_run(case, setting, tmp_path, step):
    """-> (report bytes, batches, stats, bytes handed back) of the device reader over the case's files, `step` records per batch"""
    se, pe, _ = qc_util.CASES[case]
    files = [(_plain(f, tmp_path), None) for f in se] + [(_plain(a, tmp_path), _plain(b, tmp_path)) for a, b in zip(pe[0::2], pe[1::2])]
    batches, handed = [], 0
    with binding.QC() as qc:
        for p1, p2 in files:
            with binding.IngestDev(p1, p2, qc=qc, **qc_util.trim_kw(setting)) as ing:
                while True:
                    got = ing.next(step)
                    if got is None:
                        break
                    batches.append(got)
                ing.status()
                handed += ing.handed_back
        out = str(tmp_path / "dev.json")
        qc.write(out, **qc_util.SETTINGS[setting])
        return open(out, "rb").read(), batches, qc.stats(), handed


@pytest.mark.parametrize("case", DEV_CASES)
def test_device_reader_matches_every_recorded_report_and_stream(case, tmp_path):
    """seven records per batch: the accumulator spans many batches and many passes"""
    for setting in qc_util.SETTINGS:
        report, batches, stats, handed = _dev_run(case, setting, tmp_path, 7)
        assert handed == 0
        assert report == qc_util.gold(case, setting, "json"), (case, setting)
        qc_util.compare_s1(batches, formats.parse_s1(qc_util.gold(case, setting, "s1")))
        assert all(p[-1] != 1 for _, _, p in batches)


@pytest.mark.parametrize("chunk", [3000, 20000])
def test_input_cut_into_several_passes(chunk, tmp_path, monkeypatch):
    """chunks of a few kilobytes: a file is several passes of s1_qc_kernel whose histograms meet at different resolutions (`long` raises
    it four times), and one batch spans several of them"""
    monkeypatch.setenv("KMAHIP_INGEST_DEV_CHUNK", str(chunk))
    for case in ("p33", "pe", "long", "uni"):
        for setting in ("default", "eq25ml40", "mi25clip"):
            report, batches, _, handed = _dev_run(case, setting, tmp_path, 1 << 30)
            assert handed == 0
            assert report == qc_util.gold(case, setting, "json"), (case, setting, chunk)
            qc_util.compare_s1(batches, formats.parse_s1(qc_util.gold(case, setting, "s1")))


def _host_stats(p1, p2=None, **kw):
    with binding.QC() as qc, binding.Ingest(p1, p2, qc=qc, **kw) as ing:
        n = 0
        while True:
            g = ing.next(1 << 30)
            if g is None:
                break
            n += g[0].n
        return qc.stats(), n


def test_odd_record_hands_the_tail_and_the_accumulator_to_the_host_reader(tmp_path):
    recs = open(qc_util.path_of("p33.fq"), "rb").read().split(b"\n")
    head, tail = b"\n".join(recs[:4 * 150]) + b"\n", b"\n".join(recs[4 * 150:])
    odd = tmp_path / "odd.fq"
    # a record of five lines: its 26 qualities are twenty, a newline and five low ones that the end trimming takes off. The host reader
    # reads it as the reference does (as many quality bytes as bases, seqparse.c:330-380) and goes on; to the device it is odd
    odd.write_bytes(head + b"@odd\nACGTACGTACGTACGTACGTACGTAC\n+\n" + b"I" * 20 + b"\n" + b"#" * 5 + b"\n" + tail)
    for kw in ({}, dict(min_q=15), dict(hardmask_q=25, min_len=40)):
        want, n_want = _host_stats(str(odd), **kw)
        with binding.QC() as qc, binding.IngestDev(str(odd), qc=qc, **kw) as ing:
            n = 0
            while True:
                g = ing.next(11)
                if g is None:
                    break
                n += g[0].n
            assert ing.handed_back == os.path.getsize(odd) - len(head)
            got = qc.stats()
        assert qc_util.same_stats(want, got) == [] and n == n_want, (kw, qc_util.same_stats(want, got))
        assert got["org_count"] > 300 and got["count"] > 100


def test_device_against_host_stats_field_by_field(tmp_path):
    """a seeded file of a few thousand reads with every kind of quality line, and a mate file that runs out"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_ingest as mgi
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    mgi.write_fq(a, 3000, 31, lens=(30, 700))
    mgi.write_fq(b, 2500, 32, lens=(30, 300))
    for files in ((a, None), (a, b)):
        for kw in ({}, dict(min_q=20, min_len=30), dict(hardmask_q=15, max_len=500)):
            want, n_want = _host_stats(*files, **kw)
            with binding.QC() as qc, binding.IngestDev(*files, qc=qc, **kw) as ing:
                n = 0
                while True:
                    g = ing.next(1000)
                    if g is None:
                        break
                    n += g[0].n
                got = qc.stats()
            assert qc_util.same_stats(want, got) == [] and n == n_want, (files, kw, qc_util.same_stats(want, got))
            # (reads of up to 700 bases: the histogram's resolution rises, unless -xl 500 drops them)
            assert (got["qresolution"] >= 1) == ("max_len" not in kw) and got["org_count"] == (6000 if files[1] else 3000)


def test_device_reader_refusals():
    with binding.QC() as qc:
        with pytest.raises(binding.KmaHipError, match="minimum length of 1"):
            binding.IngestDev(qc_util.path_of("p33.fq"), min_len=0, qc=qc)
        with binding.IngestDev(qc_util.path_of("p33.fq")) as ing:
            ing.next(5)
            assert binding._qc_lib().kmahip_ingest_dev_set_qc(ing._h, qc._h) == -1          # KMAHIP_EINVAL: after the first batch
        assert qc.stats()["org_count"] == 0


# ---- whole runs against the reference binary, run live -------------------------------------------------------------------------------
def _write_fq(path, reads, rng, tag):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            L = len(r)
            q = rng.integers(24, 41, L)
            if rng.random() < 0.5:
                q[:int(rng.integers(1, 25))] = int(rng.integers(2, 22))
            if rng.random() < 0.5:
                q[-int(rng.integers(1, 30)):] = int(rng.integers(2, 22))
            if rng.random() < 0.3:
                x = int(rng.integers(0, L))
                q[x:x + int(rng.integers(1, 20))] = int(rng.integers(2, 18))
            f.write(b"@%s%d/x some text\n" % (tag, i) + bytes(b"ACGTN"[c] for c in r) + b"\n+\n" + bytes((q + 33).astype(np.uint8)) + b"\n")


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    import proxi_util
    proxi_util.build_map()
    tmp = tmp_path_factory.mktemp("qc_whole")
    names, seqs = synth.make_gene_db(6, 4, 500, 1300, 0.04, seed=41)
    fa = str(tmp / "db.fsa")
    synth.write_fasta(fa, names, seqs)
    prefix, sparse = str(tmp / "db"), str(tmp / "sp")
    subprocess.run([KMA, "index", "-i", fa, "-o", prefix], check=True, stderr=subprocess.DEVNULL)
    subprocess.run([KMA, "index", "-i", fa, "-o", sparse, "-Sparse", "TG"], check=True, stderr=subprocess.DEVNULL)
    rng = np.random.default_rng(42)
    fq, r1, r2 = str(tmp / "r.fq"), str(tmp / "r1.fq"), str(tmp / "r2.fq")
    _write_fq(fq, proxi_util.reads(seqs, 1500, rng), rng, b"s")
    _write_fq(r1, proxi_util.reads(seqs, 700, rng), rng, b"p")
    _write_fq(r2, proxi_util.reads(seqs, 700, rng), rng, b"p")
    subprocess.run(["gzip", "-1", "-k", fq], check=True)
    return dict(tmp=tmp, prefix=prefix, sparse=sparse, fq=fq, r1=r1, r2=r2)


RUNS = {
    "1t1": (["-i", "{fq}", "-1t1"], []),
    "default": (["-i", "{fq}"], []),
    "list": (["-i", "{fq}", "{r1}", "-1t1", "-mp", "25"], []),
    "ipe": (["-ipe", "{r1}", "{r2}", "-1t1", "-eq", "15"], []),
    "int": (["-int", "{fq}", "-1t1", "-mi", "12"], []),
    "gz": (["-i", "{fq}.gz", "-1t1", "-ml", "40"], []),
    "s1dev": (["-i", "{fq}", "-1t1", "-eq", "20", "-5p", "3"], ["-s1dev"]),
    "s1dev_pe": (["-ipe", "{r1}", "{r2}", "-1t1"], ["-s1dev"]),
    "Sparse": (["-i", "{fq}", "{r1}", "-Sparse"], []),
}


@pytest.mark.parametrize("run", sorted(RUNS))
def test_kmahip_map_qc_writes_the_files_of_the_reference(whole, run):
    args, ours_only = RUNS[run]
    args = [a.format(**whole) for a in args]
    db = whole["sparse"] if run == "Sparse" else whole["prefix"]
    ref, our = str(whole["tmp"] / f"{run}.ref"), str(whole["tmp"] / f"{run}.our")
    subprocess.run([KMA] + args + ["-t_db", db, "-o", ref, "-qc", "-t", "1"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    r = subprocess.run([MAP] + args + ours_only + ["-t_db", db, "-o", our, "-qc"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    exts = [".spa", ".json"] if run == "Sparse" else [".res", ".fsa", ".aln", ".frag.gz", ".json"]
    for ext in exts:
        a, b = open(ref + ext, "rb").read(), open(our + ext, "rb").read()
        if ext.endswith(".gz"):
            a, b = gzip.decompress(a), gzip.decompress(b)
        assert a == b and len(a) > 100, (run, ext)
    if ours_only:
        assert b"stage 1 on the device: " in r.stderr and b" 0 bytes of input left to the host reader" in r.stderr


def _trim_cli(case, setting, tmp_path, extra):
    import proxi_util
    proxi_util.build_map()
    se, pe, il = qc_util.CASES[case]
    args = (["-i"] + [_plain(f, tmp_path) for f in se] if se else []) + (["-ipe"] + [_plain(f, tmp_path) for f in pe] if pe else []) + (["-int"] + [qc_util.path_of(f) for f in il] if il else [])
    out = str(tmp_path / f"{case}.{setting}")
    r = subprocess.run([TRIM] + args + ["-o", out, "-qc"] + qc_util.ref_flags(setting) + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return out, r


@pytest.mark.parametrize("case", ["p33", "dos", "pe", "long", "intodd", "p33gz", "p33+p64"])
def test_kmahip_trim_s1dev_writes_the_recorded_files(case, tmp_path):
    for setting in ("default", "eq25ml40", "mi25clip", "ml1000"):
        out, r = _trim_cli(case, setting, tmp_path, ["-s1dev"])
        assert open(out + ".json", "rb").read() == qc_util.gold(case, setting, "json"), (case, setting)
        assert open(out + ".fq", "rb").read() == qc_util.gold(case, setting, "fq"), (case, setting)
        int_fq = qc_util.gold(case, setting, "int_fq")
        assert os.path.exists(out + "_int.fq") == (int_fq is not None)
        if int_fq is not None:
            assert open(out + "_int.fq", "rb").read() == int_fq, (case, setting)
        frags = qc_util.stats_of_json(qc_util.gold(case, setting, "json"))["Fragment Count"]
        assert r.stderr.decode().splitlines()[-1] == "# Total number of query fragment after trimming:\t%d" % frags
