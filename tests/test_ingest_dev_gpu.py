"""The device stage-1 reader (kmahip_ingest_dev_*, kma_amd/csrc/ingest_dev.hip) on the GPU: against the S1 streams the compiled
reference wrote (tests/golden/ingest, the mapping fixtures), against the host reader on seeded files, across chunk borders, on inputs
whose odd records go back to the host reader, and through examples/kmahip_map -s1dev. Comparisons are those of tests/test_ingest.py."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from kma_amd import binding, formats, synth

import test_ingest as ti
from test_shard_gpu import _case, _same_files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ING = os.path.join(GOLD, "ingest")
MAP = os.path.join(ROOT, "examples", "kmahip_map")


def _all(reader, path1, path2=None, step=1 << 30, **kw):
    """test_ingest._all for either reader: (lengths, names, pair flags, (packed words, N list) per read), the error text, and for
    the device reader the bytes of input it left to the host reader"""
    out = ([], [], [], [])
    with reader(path1, path2 or None, **kw) as ing:
        err = None
        while True:
            try:
                g = ing.next(step)
            except binding.KmaHipError as e:
                err = str(e)
                continue
            if g is None:
                break
            b, names, pair = g
            assert pair[-1] != 1                      # a batch never ends inside a couple
            out[0].extend(int(x) for x in b.length)
            out[1].extend(names)
            out[2].extend(int(x) for x in pair)
            for i in range(b.n):
                L = int(b.length[i])
                w = b.seq[b.seq_off[i]:b.seq_off[i] + ((L + 31) >> 5) + 1]
                assert w[-1] == 0                     # the pad word
                out[3].append((bytes(w[:-1]), tuple(int(x) for x in b.N[b.N_off[i]:b.N_off[i + 1]])))
        counts = ing.counts()
        handed = ing.handed_back if reader is binding.IngestDev else None
    return (out, err, counts), handed


def _same(path1, path2=None, step=1 << 30, **kw):
    want, _ = _all(binding.Ingest, path1, path2, **kw)
    got, handed = _all(binding.IngestDev, path1, path2, step=step, **kw)
    assert got == want, (path1, path2, step, kw)
    return want, handed


# ---- 1. the reference's own S1 streams ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["p33", "dos", "p64", "pe"])
@pytest.mark.parametrize("setting", sorted(ti.SETTINGS))
def test_device_reader_matches_reference_s1(case, setting):
    f1, f2, phred = ti.CASES[case]
    s1 = formats.parse_s1(gzip.open(os.path.join(ING, f"{case}.{setting}.s1.gz")).read())
    with binding.IngestDev(os.path.join(ING, f1), os.path.join(ING, f2) if f2 else None, **ti.SETTINGS[setting]) as ing:
        assert ing.phred_scale == phred
        got = ing.next(1 << 30)
        assert got is not None
        ti._compare(*got, s1)
        assert ing.next(10) is None
        read, kept = ing.counts()
        assert kept == sum(1 for i in range(got[0].n) if got[2][i] != 2)
        assert ing.handed_back == 0                   # strict four-line files: the device delivers every record itself


@pytest.mark.parametrize("name,files", [("se", ("reads.fq.gz", None)), ("long", ("reads.fq.gz", None)), ("pe", ("r1.fq.gz", "r2.fq.gz"))])
def test_device_reader_matches_mapping_fixture_s1(tmp_path, name, files):
    src = os.path.join(GOLD, name)
    s1 = formats.parse_s1(gzip.open(os.path.join(src, "s1.bin.gz")).read())
    plain = []
    for f in files:
        if f:
            plain.append(str(tmp_path / f[:-3]))
            open(plain[-1], "wb").write(gzip.open(os.path.join(src, f)).read())
    with binding.IngestDev(plain[0], plain[1] if len(plain) > 1 else None) as ing:
        ti._compare(*ing.next(1 << 30), s1)
        assert ing.next(10) is None
        assert ing.handed_back == 0


# ---- 2. differential against the host reader -----------------------------------------------------------------------------------
def test_device_reader_differential_against_the_host_reader(tmp_path):
    sys.path.insert(0, os.path.join(GOLD))
    import make_golden_ingest as mk
    rng = np.random.default_rng(2024)
    kept_total = 0
    for case in range(30):
        fq, fq2 = str(tmp_path / f"c{case}.fq"), str(tmp_path / f"d{case}.fq")
        base = 64 if case % 5 == 4 else 33
        mk.write_fq(fq, int(rng.integers(1, 60)), 1000 + case, base=base, lens=(1, int(rng.integers(20, 400))))
        kw = dict(min_phred=int(rng.integers(0, 35)), min_q=int(rng.choice([0, 0, 10, 20, 28])), hardmask_q=int(rng.choice([0, 0, 5, 15])),
                  min_len=int(rng.integers(1, 80)), max_len=int(rng.choice([2**31 - 1, 150, 300])))
        mk.write_fq(fq2, int(rng.integers(1, 60)), 5000 + case, base=base, lens=(1, int(rng.integers(20, 400))))      # (its own record count)
        for step in (1 << 30, 101, 7):
            for p2 in (None, fq2):
                want, handed = _same(fq, p2, step=step, **kw)
                assert handed == 0, (case, step, p2)
                kept_total += len(want[0][0])
    assert kept_total > 3000


def test_device_reader_batches_and_empty_mates_on_larger_files(tmp_path):
    """files of several hundred records, so that max_records 101 and 7 both cut batches, as mate files of unequal record counts with
    the length gate open (-ml 0: the empty mates of the file that ran out are kept, as pair records with the other file's reads)"""
    sys.path.insert(0, os.path.join(GOLD))
    import make_golden_ingest as mk
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    mk.write_fq(a, 430, 77, lens=(1, 200))
    mk.write_fq(b, 260, 78, lens=(1, 200))
    for kw in (dict(min_len=0, min_phred=0), dict(min_len=0), dict(min_len=0, min_q=20, hardmask_q=5), dict(min_len=30)):
        for step in (1 << 30, 101, 7):
            for p1, p2 in ((a, None), (a, b), (b, a)):
                want, handed = _same(p1, p2, step=step, **kw)
                assert handed == 0
                if p2 and kw["min_len"] == 0:
                    assert len(want[0][0]) == 2 * 430 and want[0][0].count(0) >= 430 - 260      # every couple kept, empty mates among them


def test_session_upload_dev_refuses_the_modes_that_need_host_arrays(tmp_path):
    """kmahip_session_upload_dev on a default-mode and on a -Mt1 session: KMAHIP_EINVAL, and the session takes an ordinary batch afterwards"""
    import ctypes as C
    names, seqs = synth.make_gene_db(n_families=4, variants=2, seed=3)
    prefix = str(tmp_path / "db")
    formats.write_index(prefix, names, seqs)
    db = binding.KmaHipDB(prefix, device=0)
    L = binding.lib()
    L.kmahip_session_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    L.kmahip_session_set_chain.argtypes = [C.c_void_p, C.c_void_p]
    L.kmahip_session_set_mt1.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_char_p]
    L.kmahip_session_upload_dev.argtypes = [C.c_void_p, C.POINTER(binding.ReadBatchC)]
    L.kmahip_session_upload.argtypes = [C.c_void_p, C.POINTER(binding.ReadBatchC)]
    L.kmahip_session_close.argtypes = [C.c_void_p]
    L.kmahip_session_close.restype = None
    par = binding.default_params()
    for mode in ("chain", "mt1", "1t1"):
        opts = (C.c_char * 512)()
        ses = C.c_void_p()
        assert L.kmahip_session_open(db.h, db.ws, C.byref(par), opts, 1000, C.byref(ses)) == 0
        if mode == "chain":
            assert L.kmahip_session_set_chain(ses, None) == 0
        elif mode == "mt1":
            assert L.kmahip_session_set_mt1(ses, 1, 0, None) == 0
        with binding.IngestDev(os.path.join(ING, "p33.fq")) as ing:
            b = ing.next_dev(1 << 30)
            rc = L.kmahip_session_upload_dev(ses, C.byref(b))
            if mode == "1t1":
                assert rc == 0
            else:
                assert rc == -1 and b"-1t1" in L.kmahip_last_error()          # KMAHIP_EINVAL, by name
        if mode != "1t1":      # the refused session is as it was: a host batch goes up as ever
            t = binding.Trim(20, 0, 0, 16, 2**31 - 1)
            h = C.c_void_p()
            assert L.kmahip_ingest_open(os.path.join(ING, "p33.fq").encode(), None, C.byref(t), C.byref(h)) == 0
            hb = binding.ReadBatchC()
            assert L.kmahip_ingest_next(h, 1 << 30, C.byref(hb)) == 0 and hb.reads.n_reads > 0
            assert L.kmahip_session_upload(ses, C.byref(hb)) == 0
            L.kmahip_ingest_close(h)
        L.kmahip_session_close(ses)
    db.close()


# ---- 3. chunk borders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [64, 300, 4096, 100000])
def test_device_reader_chunk_borders(tmp_path, monkeypatch, chunk):
    rng = np.random.default_rng(5)
    rec = []
    for i in range(300):          # the hostile file of test_ingest_chunked_reader_equals_one_pass
        L = int(rng.choice([0, 1, 5, 30, 150, 700, 3000]))
        seq = "".join(rng.choice(list("ACGTN"), L))
        q = "".join(rng.choice(list("@+I5#"), L))
        rec.append(f"@{'r%d some text' % i if i % 7 else ''}\n{seq}\n+{'x' * int(rng.integers(0, 3))}\n{q}\n")
    hostile, nonl, trunc = tmp_path / "hostile.fq", tmp_path / "nonl.fq", tmp_path / "trunc.fq"
    hostile.write_text("".join(rec))
    nonl.write_text("".join(rec)[:-1])                     # last record without its final newline
    trunc.write_text("".join(rec)[:-40])                   # last record cut short
    files = [("p33.fq", None), ("dos.fq", None), ("m1.fq", "m2.fq"), (str(hostile), None), (str(nonl), None), (str(trunc), None)]
    monkeypatch.setenv("KMAHIP_INGEST_DEV_CHUNK", str(chunk))
    for f1, f2 in files:
        p1 = f1 if os.path.isabs(f1) else os.path.join(ING, f1)
        p2 = os.path.join(ING, f2) if f2 else None
        want, handed = _same(p1, p2, min_phred=0, min_len=0)
        assert len(want[0][0]) >= 150
        _same(p1, p2, step=7, min_phred=0, min_len=0)
        if f1 in ("p33.fq", "dos.fq", "m1.fq") or p1 == str(hostile):
            assert handed == 0, f1
        else:
            assert 0 < handed < 6200, f1              # only the bytes behind the last complete four-line record are the host reader's


# ---- 4. hand-back ----------------------------------------------------------------------------------------------------------------
def test_device_reader_hands_odd_records_back_to_the_host_reader(tmp_path):
    good = b"".join(b"@r%d\nACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIII\n" % i for i in range(200))
    short_q = tmp_path / "shortq.fq"
    short_q.write_bytes(good + b"@odd\nACGTACGTACGTACGTACGTACGTAC\n+\nIIIII\n" + good)
    bad = tmp_path / "bad.fq"
    bad.write_bytes(good + b"this is not a record\n" + good)
    for p in (short_q, bad):
        for step in (1 << 30, 100, 11):
            with binding.IngestDev(str(p)) as ing:
                first = ing.next(step)
                assert first is not None and first[0].n == min(step, 200) and first[1][0] == b"r0"
                if step < 200:
                    assert ing.handed_back == 0                        # nothing has gone to the host reader yet
            want, handed = _same(str(p), step=step)
            # exactly the bytes from the odd record on were left to the host reader: the 200 records before it came from the device
            assert handed == os.path.getsize(p) - len(good) and len(want[0][0]) >= 200
    want, _ = _same(str(bad))
    assert want[1] is not None and "malformed" in want[1] and len(want[0][0]) == 200
    # the file of test_ingest_reports_malformed_input_after_the_good_records: the same calls answer the same way
    tiny = tmp_path / "tiny.fq"
    tiny.write_bytes(b"@a\nACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIII\nthis is not a record\n@b\nACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIII\n")
    with binding.IngestDev(str(tiny)) as ing:
        got = ing.next(100)
        assert got is not None and got[0].n == 1 and got[1] == [b"a"]
        with pytest.raises(binding.KmaHipError):
            ing.next(100)
        assert ing.next(100) is None
    # a mate file that runs out, and one that breaks off inside a record
    short = tmp_path / "short.fq"
    short.write_bytes(good[:len(good) // 3 - 5])
    full = tmp_path / "full.fq"
    full.write_bytes(good)
    for a, b in ((full, short), (short, full)):
        want, _ = _same(str(a), str(b), step=13)
        assert len(want[0][0]) > 200


# ---- 5. whole runs through examples/kmahip_map -s1dev -----------------------------------------------------------------------------
def _run(args, env=None, ok=True):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([MAP] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r


def _s1dev_line(stderr):
    """(input records that went through the device reader, bytes it left to the host reader) as kmahip_map -s1dev reports them"""
    import re
    m = re.search(rb"stage 1 on the device: (\d+) input records, (\d+) bytes of input left to the host reader", stderr)
    assert m, stderr.decode()[-2000:]
    return int(m.group(1)), int(m.group(2))


def _pairs(tmp_path, n=2000):
    names, seqs = synth.make_gene_db(n_families=40, variants=5, seed=77)
    r1, r2 = [], []
    rng = np.random.default_rng(9)
    for k in range(n):
        g = seqs[int(rng.integers(0, len(seqs)))]
        a = int(rng.integers(0, max(1, len(g) - 300)))
        frag = g[a:a + 300]
        r1.append(frag[:120].copy())
        r2.append(synth.revcomp_codes(frag[-120:]))
    p1, p2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    synth.write_fastq(p1, r1, prefix="p")
    synth.write_fastq(p2, r2, prefix="p")
    return p1, p2


def test_kmahip_map_s1dev_writes_the_same_files(tmp_path):
    prefix, fq = _case(tmp_path)
    r1, r2 = _pairs(tmp_path)
    half = str(tmp_path / "half.fq")
    lines = open(fq, "rb").read().split(b"\n")
    open(half, "wb").write(b"\n".join(lines[:4 * 3000]) + b"\n")
    runs = {
        "se": ["-i", fq, "-1t1"],
        "pe_p": ["-ipe", r1, r2, "-apm", "p", "-1t1"],
        "pe_u": ["-ipe", r1, r2, "-1t1"],
        "list": ["-i", half, fq, "-1t1"],
        "trim": ["-i", fq, "-1t1", "-mp", "30", "-ml", "40", "-eq", "25", "-mf", "900"],
    }
    for name, args in runs.items():
        for batch in (None, "1000"):
            env = {"KMAHIP_MAP_BATCH": batch} if batch else {}
            a, b = str(tmp_path / f"{name}.host"), str(tmp_path / f"{name}.dev")
            _run(args + ["-t_db", prefix, "-o", a], env=env)
            r = _run(args + ["-t_db", prefix, "-o", b, "-s1dev"], env=env)
            _same_files(a, b)
            rec, left = _s1dev_line(r.stderr)
            assert rec >= 2000 and left == 0, (name, rec, left)          # every record came through the device reader
    # refused by name where the switch does not apply
    for args in (["-gpus", "2", "-i", fq, "-1t1"], ["-i", fq], ["-i", fq, "-Mt1", "1"]):
        r = _run(args + ["-t_db", prefix, "-o", str(tmp_path / "no"), "-s1dev"], ok=False)
        assert r.returncode != 0 and b"-s1dev" in r.stderr, args
    # a compressed input takes the host reader, silently
    subprocess.run(["gzip", "-1", "-k", fq], check=True, timeout=120)
    r = _run(["-i", fq + ".gz", "-1t1", "-t_db", prefix, "-o", str(tmp_path / "gz.dev"), "-s1dev"])
    assert _s1dev_line(r.stderr) == (0, 0)
    _same_files(str(tmp_path / "se.host"), str(tmp_path / "gz.dev"))
