"""The host reader with a QC accumulator (kmahip_ingest_set_qc, kmahip_qc_*) and its text sink (kmahip_ingest_set_text,
kmahip_trim_files) against what the reference recorded in tests/golden/qc: the report, the S1 stream under -qc and the trimmed reads,
byte for byte. No GPU. With one worker thread and with eight, with small chunks of input, and batch by batch."""
import os

import numpy as np
import pytest

import qc_util
from kma_amd import binding, formats


def _readers(case, qc, text=False, **kw):
    se, pe, il = qc_util.CASES[case]
    for f in se:
        yield binding.Ingest(qc_util.path_of(f), qc=qc, text=text, **kw)
    for a, b in zip(pe[0::2], pe[1::2]):
        yield binding.Ingest(qc_util.path_of(a), qc_util.path_of(b), qc=qc, text=text, **kw)
    for f in il:
        yield binding.Ingest(qc_util.path_of(f), interleaved=True, qc=qc, text=text, **kw)


def _run(case, setting, tmp_path, max_records=1 << 30):
    """-> (report bytes, batches, single text, couple text, stats) of the host reader over the case's files"""
    kw = qc_util.trim_kw(setting)
    batches, fq, int_fq = [], b"", b""
    with binding.QC() as qc:
        for ing in _readers(case, qc, text=True, **kw):
            with ing:
                while True:
                    got = ing.next(max_records)
                    if got is None:
                        break
                    batches.append(got)
                    a, b = ing.text()
                    fq += a
                    int_fq += b
                ing.status()
        out = str(tmp_path / "r.json")
        qc.write(out, **qc_util.SETTINGS[setting])
        return open(out, "rb").read(), batches, fq, int_fq, qc.stats()


def _hold(case, setting, got):
    report, batches, fq, int_fq, _ = got
    assert report == qc_util.gold(case, setting, "json"), (case, setting)
    qc_util.compare_s1(batches, formats.parse_s1(qc_util.gold(case, setting, "s1")))
    assert fq == qc_util.gold(case, setting, "fq"), (case, setting)
    assert int_fq == (qc_util.gold(case, setting, "int_fq") or b""), (case, setting)


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("case", sorted(qc_util.CASES))
def test_host_reader_matches_every_recorded_file(case, threads, tmp_path, monkeypatch):
    monkeypatch.setenv("KMAHIP_INGEST_THREADS", str(threads))
    for setting in qc_util.SETTINGS:
        _hold(case, setting, _run(case, setting, tmp_path))


@pytest.mark.parametrize("case", ["p33", "pe", "intodd", "p33gz", "long", "p33+p64"])
def test_small_chunks_and_small_batches(case, tmp_path, monkeypatch):
    """the input cut into chunks of a few kilobytes and regions of a few hundred bytes, the accumulator fed over many batches"""
    monkeypatch.setenv("KMAHIP_INGEST_CHUNK", "12000")
    monkeypatch.setenv("KMAHIP_INGEST_REGION", "700")
    monkeypatch.setenv("KMAHIP_INGEST_THREADS", "8")
    for setting in ("default", "eq25ml40", "mi25clip"):
        _hold(case, setting, _run(case, setting, tmp_path, max_records=7))


def test_threads_do_not_change_the_sums(tmp_path, monkeypatch):
    """enough records for the trimming to be shared among eight threads (2 048 per thread at least): Eeq to the last bit, every
    histogram and the text as with one thread -- and as the restatement has them"""
    big = str(tmp_path / "big.fq")
    p33 = open(qc_util.path_of("p33.fq"), "rb").read()
    uni = open(qc_util.path_of("qc/uni.fq"), "rb").read()
    with open(big, "wb") as f:
        f.write((p33 + uni) * 40)                                   # 20 800 records
    got = {}
    for threads in (1, 8):
        monkeypatch.setenv("KMAHIP_INGEST_THREADS", str(threads))
        with binding.QC() as qc, binding.Ingest(big, min_q=15, qc=qc, text=True) as ing:
            n = 0
            text = b""
            while True:
                g = ing.next(1 << 30)
                if g is None:
                    break
                n += g[0].n
                text += ing.text()[0]
            got[threads] = (qc.stats(), n, text)
    assert qc_util.same_stats(got[1][0], got[8][0]) == [] and got[1][1:] == got[8][1:]
    s = got[8][0]
    assert s["org_count"] == 20800 and s["fragcount"] == got[8][1] and s["Eeq"] > 0
    # one pass of the restatement over the two files gives the integer sums; Eeq is held above (equal for 1 and 8 threads)
    a = qc_util.QCStat()
    for name in ("p33.fq", "qc/uni.fq"):
        buf = qc_util.read_bytes(qc_util.path_of(name))
        for hdr, raw, qual in qc_util.read_fastq(buf):
            seq = [qc_util.TO2BIT[c] for c in raw]
            r = qc_util.phred_stat(seq, qual, 33, 20, 15, 0, 16, 2**31 - 1)
            if r["counted"]:
                a.update(r["len"], r["gc"], r["ns"], r["sp"])
    assert s["count"] == 40 * a.count and s["bpcount"] == 40 * a.bpcount and s["totgc"] == 40 * a.totgc and s["totns"] == 40 * a.totns
    assert np.array_equal(s["qdist"], 40 * np.array(a.qdist, np.uint32)) and np.array_equal(s["ldist"], 40 * np.array(a.ldist, np.uint32))


def test_a_reader_without_an_accumulator_is_the_reader_of_before():
    """`long` holds reads that only the -qc rule drops: without an accumulator they stay (the S1 stream of tests/golden/ingest is held by
    test_ingest.py; here the two rules are told apart on one file)"""
    with binding.Ingest(qc_util.path_of("qc/long.fq.gz")) as a:
        plain = a.next(1 << 30)[0].n
    with binding.QC() as qc, binding.Ingest(qc_util.path_of("qc/long.fq.gz"), qc=qc) as b:
        ruled = b.next(1 << 30)[0].n
        assert qc.stats()["fragcount"] == ruled
    assert plain > ruled


def test_trim_files_writes_the_three_files(tmp_path):
    se, pe, il = ["p33.fq"], ["m1.fq", "m2.fq"], ["ilvodd.fq"]
    out = str(tmp_path / "t")
    with binding.QC() as qc:
        n = binding.trim_files([qc_util.path_of(f) for f in se], out, paired=[qc_util.path_of(f) for f in pe], interleaved=[qc_util.path_of(f) for f in il], qc=qc, min_q=15)
        s = qc.stats()
    assert n == s["fragcount"]
    want = [qc_util.gold(c, "eq15", "fq") for c in ("p33", "pe", "intodd")]
    assert open(out + ".fq", "rb").read() == b"".join(want)
    assert open(out + "_int.fq", "rb").read() == qc_util.gold("pe", "eq15", "int_fq") + qc_util.gold("intodd", "eq15", "int_fq")
    # single-end files alone leave no _int.fq, like the reference
    out2 = str(tmp_path / "u")
    binding.trim_files([qc_util.path_of("p33.fq")], out2)
    assert os.path.exists(out2 + ".fq") and not os.path.exists(out2 + "_int.fq")
    assert open(out2 + ".fq", "rb").read() == qc_util.restate("p33", "default", report=False)["fq"]


def test_refusals_by_name():
    wrap = os.path.join(qc_util.ING, "wrap.fa")
    with binding.QC() as qc:
        with pytest.raises(binding.KmaHipError, match="FASTA input has no QC report"):
            binding.Ingest(wrap, qc=qc)
        with pytest.raises(binding.KmaHipError, match="minimum length of 1"):
            binding.Ingest(qc_util.path_of("p33.fq"), min_len=0, qc=qc)
        with pytest.raises(binding.KmaHipError, match="FASTA input is not written back"):
            binding.Ingest(wrap, text=True)
        with binding.Ingest(qc_util.path_of("p33.fq")) as ing:
            ing.next(5)
            L = binding._qc_lib()
            assert L.kmahip_ingest_set_qc(ing._h, qc._h) == -1          # KMAHIP_EINVAL: after the first batch
        assert qc.stats()["org_count"] == 0
