"""SAM records (`-sam [n]`) made on the device: the formatter alone on hand-made traces against kmahip_sam_row_host, and whole
`-1t1` runs of examples/kmahip_map, single end and paired, against the compiled reference (oracle/_ref/kma -t 1) run live on the same
input. kmahip_map takes the level in full: its `-sam 1` is compared with the reference's bare `-sam`.

The reference runs stage 2 beside stage 3a under -sam, so its rows without a template (RNAME *) interleave differently from run to
run: those are compared as sorted lists; everything with a template name is compared byte for byte, in order."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from kma_amd import binding, formats, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")
LUT = np.frombuffer(b"ACGTN", dtype=np.uint8)
COMP = np.array([3, 2, 1, 0, 4], np.uint8)


def _text(codes, flip=False):
    return LUT[COMP[codes[::-1]] if flip else codes].tobytes()


# ---- 1. the formatter alone ---------------------------------------------------------------------------------------------------------
def _hand_made(rng, n_templates):
    """items of every record class with the figures the kernels must get right: run lengths at the digit boundaries, clips zero and
    not, a negative AS, mapQ 300, N's, reads of 20, 150 and 5 000 bases, headers with and without a TAB"""
    edges = (1, 9, 10, 99, 100, 99_999)
    items = []
    for i in range(640):
        L = (20, 150, 150, 150, 5000)[i % 5] if i % 97 else 5000
        codes = rng.integers(0, 4, L, dtype=np.uint8)
        if i % 3 == 0:
            codes[rng.integers(0, L, int(rng.integers(1, 4)))] = 4
        kind = ("s2", "s3a", "kept", "kept", "kept", "drop", "unal", "skip", "none")[int(rng.integers(0, 9))]
        it = dict(codes=codes, hdr=(b"read%d desc\tBX:Z:%d" % (i, i)) if i % 2 else b"read%d" % i, kind=kind, rc=int(rng.integers(0, 2)),
                  tmpl=0, n_hits=0, flag=0, st=np.zeros(10, np.int32), ds=np.zeros(6, np.int32), runs=[], druns=[])
        if kind == "s3a":
            it["flag"] = 4 | (16 if it["rc"] else 0)
        elif kind == "none":
            it["n_hits"] = 2          # (neither rejected nor filed: no record)
        elif kind != "s2":
            t = int(rng.integers(1, n_templates + 1))
            it["tmpl"] = -t if rng.random() < 0.3 else t
            it["n_hits"] = int(rng.integers(1, 12))
            it["flag"] = 16 if it["rc"] else 0
            n_runs = int(rng.integers(1, 9)) if L < 5000 else int(rng.integers(300, 1400))
            runs = [(int(edges[int(rng.integers(0, 6))] if rng.random() < 0.5 else rng.integers(1, 2000)) << 2) | int(rng.integers(0, 4)) for _ in range(n_runs)]
            cs, ce = (0 if rng.random() < 0.5 else int(rng.integers(1, 120))), (0 if rng.random() < 0.5 else int(rng.integers(1, 12000)))
            start, end = int(rng.integers(0, 900)), int(rng.integers(0, 1300))
            mapq = 300 if i % 7 == 0 else int(rng.integers(0, 255))
            if kind == "kept":
                it["st"][:] = [int(rng.integers(1, 5000)), start, end, 77, cs, ce, 70, 3, 4, mapq]
                it["runs"] = runs
            elif kind == "drop":
                it["ds"][:] = [-int(rng.integers(1, 400)) if rng.random() < 0.7 else int(rng.integers(1, 40)), start, end, cs, ce, mapq]
                it["druns"] = runs
        items.append(it)
    return items


def _expected_rows(items, names, ok, level, max_frag):
    rows1, rows2, rows3 = [], [], []
    rank = 0
    for it in items:
        k, tt = it["kind"], it["tmpl"]
        if k == "s2" and level == 1:
            rows1.append(binding.sam_row_host(it["hdr"], 20, None, 0, 0, None, 0, 0, 0, _text(it["codes"]), 0, 0))
        elif k == "s3a" and level == 1:
            rows2.append(binding.sam_row_host(it["hdr"], it["flag"], None, 0, 0, None, 0, 0, 0, _text(it["codes"], it["rc"] == 1), 0, 0))
        if tt == 0:
            continue
        t = abs(tt)
        key = (t, (rank // max_frag) * max_frag + (max_frag - 1 - rank % max_frag))
        rank += 1
        flag = it["flag"] | (16 if tt < 0 else 0)
        seq = _text(it["codes"], (it["rc"] == 1) != (tt < 0))
        if k == "kept":
            st = it["st"]
            rows3.append((key, binding.sam_row_host(it["hdr"], flag, names[t - 1], st[1] + 1, st[9], np.array(it["runs"], np.uint32), st[4], st[5],
                                                    st[2] - st[1] - 1, seq, it["n_hits"], st[0])))
        elif level & 2096:
            continue
        elif k == "drop" and ok[t]:
            ds = it["ds"]
            rows3.append((key, binding.sam_row_host(it["hdr"], flag, names[t - 1], ds[1] + 1, ds[5], np.array(it["druns"], np.uint32), ds[3], ds[4],
                                                    ds[2] - ds[1] - 1, seq, it["n_hits"], ds[0])))
        else:          # read_score 0, nothing to align, or a template the significance gate skips
            rows3.append((key, binding.sam_row_host(it["hdr"], flag | 4, names[t - 1], 0, 0, None, 0, 0, 0, seq, it["n_hits"], 0)))
    rows3.sort(key=lambda kr: kr[0])
    return rows1 + rows2 + [r for _, r in rows3]


@pytest.fixture(scope="module")
def hand_made(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sam_fmt")
    names, seqs = synth.make_gene_db(3, 3, 300, 500, 0.04, seed=5)
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    rng = np.random.default_rng(11)
    items = _hand_made(rng, len(seqs))
    ok = np.ones(len(seqs) + 1, np.uint8)
    ok[4] = 0          # a template the significance gate skips: its kept rows stay, everything else of it is class 3d
    for it in items:
        if abs(it["tmpl"]) == 4 and it["kind"] == "kept":
            it["kind"] = "skip"
            it["st"][:] = 0
            it["runs"] = []
    batch = formats.pack_ragged([it["codes"] for it in items])
    # the run pool: kept and dropped alignments interleaved, as the traceback leaves them
    ops, off, nops, doff, dnops = [0, 0, 0], [], [], [], []
    for it in items:
        off.append(len(ops)); nops.append(len(it["runs"])); ops += it["runs"]
        doff.append(len(ops)); dnops.append(len(it["druns"])); ops += it["druns"]
    arrays = dict(rc=np.array([it["rc"] for it in items], np.int32), tmpl=np.array([it["tmpl"] for it in items], np.int32),
                  n_hits=np.array([it["n_hits"] for it in items], np.int32), flag=np.array([it["flag"] for it in items], np.int32),
                  traces=(np.stack([it["st"] for it in items]), np.array(off, np.int64), np.array(nops, np.int32), np.array(ops, np.uint32)),
                  drops=(np.stack([it["ds"] for it in items]), np.array(doff, np.int64), np.array(dnops, np.int32)))
    tnames = [n.encode() if isinstance(n, str) else n for n in names]
    return dict(prefix=prefix, items=items, ok=ok, batch=batch, names=tnames, tmp=tmp, **arrays)


@pytest.mark.parametrize("group,chunk", [(None, None), ("1", "1024"), ("64", "1024"), ("64", None), ("1", "70000")])
@pytest.mark.parametrize("level", [1, 4, 16, 2096])
def test_formatter_equals_host_rows(hand_made, level, group, chunk, monkeypatch):
    """kmahip_sam_write on hand-made traces: rows of every class, each group size forced (and the one chosen by itself), text chunks
    shorter than a long read's row, so that such a row gets a buffer of its own, and chunks that hold a few rows"""
    h = hand_made
    for k, v in (("KMAHIP_SAM_GROUP", group), ("KMAHIP_SAM_CHUNK", chunk)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    max_frag = 7
    want = _expected_rows(h["items"], h["names"], h["ok"], level, max_frag)
    kinds = [it["kind"] for it in h["items"]]
    assert all(kinds.count(k) > 20 for k in ("s2", "s3a", "kept", "drop", "unal", "skip", "none"))
    path = h["tmp"] / f"rows_{level}_{group}_{chunk}.sam"
    db = binding.KmaHipDB(h["prefix"])
    try:
        db.sam_header(path, "test", "a b c")
        rows, per = db.sam_write(path, h["batch"], h["rc"], h["tmpl"], h["n_hits"], h["flag"], h["traces"], [it["hdr"] for it in h["items"]],
                                 drops=h["drops"], tmpl_ok=h["ok"], level=level, max_frag=max_frag)
    finally:
        db.close()
    got = open(path, "rb").read().split(b"\n")
    assert got[-1] == b""
    head, body = [x for x in got[:-1] if x.startswith(b"@")], [x + b"\n" for x in got[:-1] if not x.startswith(b"@")]
    lens = formats.read_lengths(h["prefix"])
    assert head == [b"@HD\tVN:1.6\tGO:reference", b"@PG\tID:KMA\tPN:test\tVN:" + binding.lib().kmahip_version() + b"\tCL:a b c"] + \
        [b"@SQ\tSN:" + n + b"\tLN:%d" % lens[t + 1] for t, n in enumerate(h["names"])]
    assert rows == len(want) == sum(per)
    assert len(body) == len(want)
    for r, (g, w) in enumerate(zip(body, want)):
        assert g == w, (r, g[:300], w[:300])
    if level == 1:
        assert all(p > 20 for p in per)
    if level == 16:
        assert per[0] == per[1] == per[3] == per[4] == 0 and per[2] > 100


# ---- whole runs against the reference ---------------------------------------------------------------------------------------------
def _split(out):
    lines = out.split(b"\n")
    assert lines[-1] == b""
    head = [x for x in lines[:-1] if x.startswith(b"@")]
    rows = [x for x in lines[:-1] if not x.startswith(b"@")]
    assert lines[:len(head)] == head          # (the header comes first)
    return head, rows


def _compare(got, ref):
    gh, gr = _split(got)
    rh, rr = _split(ref)
    assert [x for x in gh if not x.startswith(b"@PG")] == [x for x in rh if not x.startswith(b"@PG")]
    assert sum(x.startswith(b"@PG\tID:KMA\tPN:kmahip_map\tVN:") for x in gh) == 1
    named = lambda rows: [x for x in rows if x.split(b"\t")[2] != b"*"]  # noqa: E731
    star = lambda rows: sorted(x for x in rows if x.split(b"\t")[2] == b"*")  # noqa: E731
    g, r = named(gr), named(rr)
    for i, (a, b) in enumerate(zip(g, r)):
        assert a == b, (i, a[:400], b[:400])
    assert len(g) == len(r)
    assert star(gr) == star(rr)
    return rr


def _class_counts(rows, reads_by_name, frag_rows):
    """classes of the REFERENCE's rows: 1 / 2 by what SEQ holds (a stage-2 reject prints the read as it came, a stage-3a reject the
    strand stage 2 passed on, with FLAG 4 or 20), 3b = aligned rows beyond those of the fragment file, 3c + 3d = template but no CIGAR"""
    c = dict(c1=0, c2=0, aligned=0, c3cd=0, fwd=0, rev=0)
    for x in rows:
        f = x.split(b"\t")
        if f[2] == b"*":
            codes = reads_by_name[f[0]]
            if int(f[1]) == 20 and f[9] == _text(codes) and f[9] != _text(codes, True):
                c["c1"] += 1
            else:
                assert int(f[1]) in (4, 20)
                c["c2"] += 1
        elif f[5] == b"*":
            c["c3cd"] += 1
        else:
            c["aligned"] += 1
            c["rev" if int(f[1]) & 16 else "fwd"] += 1
    c["c3a"] = frag_rows
    c["c3b"] = c["aligned"] - frag_rows
    return c


def _run_ref(tmp, fq_args, prefix, tag, extra):
    out = subprocess.run([KMA] + fq_args + ["-o", str(tmp / f"ref_{tag}"), "-t_db", prefix, "-1t1", "-t", "1"] + extra, check=True, stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL).stdout
    return out


def _run_map(tmp, fq_args, prefix, tag, extra, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([MAP] + fq_args + ["-t_db", prefix, "-o", str(tmp / f"got_{tag}"), "-1t1"] + extra, check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, env=e).stdout


def _files(tmp, stem):
    return tuple(open(tmp / f"{stem}{ext}", "rb").read() for ext in (".res", ".fsa", ".aln")) + (gzip.open(tmp / f"{stem}.frag.gz", "rb").read(),)


def _need_binaries():
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)


def _make_se_set(tmp):
    """48 templates; 3 000 reads with all of test_reference_binary_gpu._reads' oddities over the first 40, one or two reads on each of
    the last 8 (templates the significance gate may skip), 400 short reads cut from a template's ends with 3 % substitutions (alignments
    the read filter drops), shuffled"""
    from test_reference_binary_gpu import _reads
    names, seqs = synth.make_gene_db(12, 4, 500, 1300, 0.04, seed=101)
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    rng = np.random.default_rng(2)
    reads = _reads(seqs[:40], 3000, rng)
    for s in seqs[40:]:
        for _ in range(int(rng.integers(1, 3))):
            a = int(rng.integers(0, len(s) - 150))
            reads.append(s[a:a + 150].copy())
    for _ in range(400):
        s = seqs[int(rng.integers(0, len(seqs)))]
        L = int(rng.integers(40, 110))
        r = (s[:L] if rng.random() < 0.5 else s[-L:]).copy()
        x = rng.random(L) < 0.03
        r[x] = (r[x] + rng.integers(1, 4, int(x.sum()), dtype=np.uint8)) & 3
        reads.append(synth.revcomp_codes(r).copy() if rng.random() < 0.5 else r)
    order = np.random.default_rng(2).permutation(len(reads))
    reads = [np.ascontiguousarray(reads[i]) for i in order]
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, reads, lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], by_name={b"r%d" % i: r for i, r in enumerate(reads)}, plain={})


def _plain_files(s, extra):
    """the four result files of the run WITHOUT -sam, once per set of the other options"""
    key = " ".join(extra)
    if key not in s["plain"]:
        tag = "plain" + str(len(s["plain"]))
        assert _run_map(s["tmp"], s["fq"], s["prefix"], tag, extra) == b""          # (nothing else goes to standard output)
        s["plain"][key] = _files(s["tmp"], "got_" + tag)
    return s["plain"][key]


@pytest.fixture(scope="module")
def se_set(tmp_path_factory):
    _need_binaries()
    return _make_se_set(tmp_path_factory.mktemp("sam_se"))


# (ours, the reference's: `-sam 1` is its bare `-sam`; -s1dev is ours alone)
SE_SETS = [
    ("sam", ["-sam", "1"], [], None),
    ("sam4", ["-sam", "4"], [], None),
    ("sam16", ["-sam", "16"], [], None),
    ("mrs", ["-sam", "1"], ["-mrs", "0.9", "-localopen", "12"], None),
    ("sam4mf", ["-sam", "4"], ["-mf", "7"], None),
    ("s1dev", ["-sam", "1", "-s1dev"], [], None),
    ("pipeline", ["-sam", "1"], [], {"KMAHIP_TRACE": "pipeline"}),
    ("sam4s1dev", ["-sam", "4", "-s1dev"], [], None),
    ("batches", ["-sam", "1"], [], {"KMAHIP_MAP_BATCH": "1000"}),          # (four batches: the per-read flags kept batch by batch)
]


def _ref_sam(sam):
    return [x for x in sam if x != "-s1dev" and not (x == "1" and sam[0] == "-sam")]


@pytest.mark.parametrize("tag,sam,extra,env", SE_SETS, ids=[x[0] for x in SE_SETS])
def test_single_end_run_equals_reference(se_set, tag, sam, extra, env):
    s = se_set
    ref = _run_ref(s["tmp"], s["fq"], s["prefix"], tag, _ref_sam(sam) + extra)
    level = int(sam[1])
    got = _run_map(s["tmp"], s["fq"], s["prefix"], tag, sam + extra, env)
    ref_rows = _compare(got, ref)
    # the other four files: those of the run without -sam, and the reference's
    mine = _files(s["tmp"], "got_" + tag)
    assert mine == _plain_files(s, extra)
    assert mine == _files(s["tmp"], "ref_" + tag)
    c = _class_counts(ref_rows, s["by_name"], mine[3].count(b"\n"))
    print(tag, c)
    assert c["c3a"] > 2000 and c["fwd"] > 500 and c["rev"] > 500
    if level == 1:
        assert c["c1"] >= 1 and c["c2"] >= 1
    else:
        assert c["c1"] == c["c2"] == 0
    if level & 2096:
        assert c["c3b"] == c["c3cd"] == 0
    else:
        # (a change of the generator must not empty a class silently)
        assert c["c3b"] >= 1 and c["c3cd"] >= 1


def _make_long_set(tmp):
    """6 templates of 8 - 9 kb; 40 reads of 3 kb with ONT-like errors on each of five, one on the sixth, five random 2.5 kb reads"""
    rng = np.random.default_rng(31)
    seqs = [rng.integers(0, 4, int(rng.integers(8000, 9001)), dtype=np.uint8) for _ in range(6)]
    names = ["long%d some description" % i for i in range(6)]
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    reads = []
    for t in range(5):
        reads += synth.make_long_reads(seqs[t], 40, read_len=3000, seed=40 + t)
    reads += synth.make_long_reads(seqs[5], 1, read_len=3000, seed=50)
    reads += [rng.integers(0, 4, 2500, dtype=np.uint8) for _ in range(5)]
    order = np.random.default_rng(3).permutation(len(reads))
    reads = [np.ascontiguousarray(reads[i].astype(np.uint8)) for i in order]
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, reads, lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], by_name={b"r%d" % i: r for i, r in enumerate(reads)}, plain={})


@pytest.fixture(scope="module")
def long_set(tmp_path_factory):
    _need_binaries()
    return _make_long_set(tmp_path_factory.mktemp("sam_long"))


@pytest.mark.parametrize("sam", [["-sam", "1"], ["-sam", "4"]], ids=["sam", "sam4"])
def test_long_reads_equal_reference(long_set, sam):
    """CIGARs of a thousand characters: the wavefront-per-row kernels, and lt_finish_kernel's records"""
    s = long_set
    tag = "l" + "".join(sam).replace("-", "")
    ref = _run_ref(s["tmp"], s["fq"], s["prefix"], tag, _ref_sam(sam))
    got = _run_map(s["tmp"], s["fq"], s["prefix"], tag, sam)
    ref_rows = _compare(got, ref)
    mine = _files(s["tmp"], "got_" + tag)
    assert mine == _plain_files(s, [])
    assert mine == _files(s["tmp"], "ref_" + tag)
    c = _class_counts(ref_rows, s["by_name"], mine[3].count(b"\n"))
    print(tag, c, max(len(x.split(b"\t")[5]) for x in ref_rows))
    assert c["c3a"] >= 150 and max(len(x.split(b"\t")[5]) for x in ref_rows) > 600
    assert c["c1"] == (5 if sam == ["-sam", "1"] else 0)


def _make_pe_set(tmp):
    """40 templates; 2 000 pairs on the first 32, 6 pairs on the other 8, a foreign mate in 150 pairs, both mates foreign in 60"""
    names, seqs = synth.make_gene_db(10, 4, 700, 1400, 0.04, seed=77)
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    rng = np.random.default_rng(5)
    a1, a2, _ = synth.make_pairs(seqs[:32], 2000, seed=9)
    b1, b2, _ = synth.make_pairs(seqs[32:], 6, seed=10)
    r1, r2 = [r.copy() for r in a1] + [r.copy() for r in b1], [r.copy() for r in a2] + [r.copy() for r in b2]
    odd = rng.choice(2000, 210, replace=False)
    for i in odd[:150]:
        (r1 if rng.random() < 0.5 else r2)[i] = rng.integers(0, 4, 150, dtype=np.uint8)
    for i in odd[150:]:
        r1[i], r2[i] = rng.integers(0, 4, 150, dtype=np.uint8), rng.integers(0, 4, 150, dtype=np.uint8)
    order = rng.permutation(len(r1))
    for path, rs, mate in ((tmp / "r1.fq", r1, b"/1"), (tmp / "r2.fq", r2, b"/2")):
        with open(path, "wb") as f:
            for k, i in enumerate(order):
                f.write(b"@p%d" % k + mate + b"\n" + LUT[rs[i]].tobytes() + b"\n+\n" + b"I" * len(rs[i]) + b"\n")
    return dict(tmp=tmp, prefix=prefix, fq=["-ipe", str(tmp / "r1.fq"), str(tmp / "r2.fq")], plain={})


@pytest.fixture(scope="module")
def pe_set(tmp_path_factory):
    _need_binaries()
    return _make_pe_set(tmp_path_factory.mktemp("sam_pe"))


PE_SETS = [("p4", ["-apm", "p"], ["-sam", "4"]), ("p16", ["-apm", "p"], ["-sam", "16"]), ("u4", [], ["-sam", "4"]), ("u16", [], ["-sam", "16"]),
           ("p4mrs", ["-apm", "p", "-mrs", "0.9", "-localopen", "12"], ["-sam", "4"])]


@pytest.mark.parametrize("tag,extra,sam", PE_SETS, ids=[x[0] for x in PE_SETS])
def test_paired_run_equals_reference(pe_set, tag, extra, sam):
    """couples, unmated pairs and single mates: the whole body byte for byte in the reference's order (n != 1 prints no row without a template)"""
    s = pe_set
    ref = _run_ref(s["tmp"], s["fq"], s["prefix"], tag, sam + extra)
    got = _run_map(s["tmp"], s["fq"], s["prefix"], tag, sam + extra)
    gh, gr = _split(got)
    rh, rr = _split(ref)
    assert [x for x in gh if not x.startswith(b"@PG")] == [x for x in rh if not x.startswith(b"@PG")]
    for i, (a, b) in enumerate(zip(gr, rr)):
        assert a == b, (i, a[:400], b[:400])
    assert len(gr) == len(rr)
    mine = _files(s["tmp"], "got_" + tag)
    assert mine == _plain_files(s, extra)
    assert mine == _files(s["tmp"], "ref_" + tag)
    aligned = sum(x.split(b"\t")[5] != b"*" for x in rr)
    unal = len(rr) - aligned
    print(tag, len(rr), aligned, unal, sorted({int(x.split(b"\t")[1]) for x in rr}))
    assert aligned > 3000 and all(x.split(b"\t")[2] != b"*" for x in rr)
    if sam[1] == "16":
        assert unal == 0 and aligned == mine[3].count(b"\n")
    else:
        assert unal >= 1          # (rows of classes 3c / 3d: the generator must not lose them silently)


def test_modes_without_sam_records_are_refused_by_name(se_set):
    """what -sam is not built for ends with status 2 and names the option: paired input at level 1, the default mode, -Mt1, interleaved
    input, -status beside it, and the option without its level"""
    s = se_set
    fq = s["fq"][1]
    for args in (["-ipe", fq, fq, "-1t1", "-sam"], ["-ipe", fq, fq, "-1t1", "-apm", "p", "-sam", "1"], ["-i", fq, "-sam", "4"], ["-i", fq, "-sam", "4", "-Mt1", "1"],
                 ["-int", fq, "-1t1", "-sam", "4"], ["-i", fq, "-1t1", "-sam", "4", "-status"], ["-i", fq, "-1t1", "-sam"]):
        p = subprocess.run([MAP] + args + ["-t_db", s["prefix"], "-o", str(s["tmp"] / "refused")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 2 and b"-sam" in p.stderr and p.stdout == b"", (args, p.returncode, p.stderr)


def test_sessions_of_other_modes_refuse_sam_by_name(se_set):
    """kmahip_session_set_sam: KMAHIP_EINVAL with a message that names the mode, whichever of the two is set first"""
    db = binding.KmaHipDB(se_set["prefix"])
    try:
        with db.session() as ses:          # (paired input at a level other than 1 is served, in either order)
            ses.set_pe()
            ses.set_sam(4, "-")
        with db.session() as ses:
            ses.set_sam(16, "-")
            ses.set_pe()
        for mode, word in (("set_chain", "default mode"), ("set_pe", "paired"), ("set_mt1", "-Mt1")):
            for sam_first in (False, True):
                with db.session() as ses:
                    first, second = (lambda: ses.set_sam(1, "-")), (lambda: getattr(ses, mode)(*([1] if mode == "set_mt1" else [])))
                    if not sam_first:
                        first, second = second, first
                    first()
                    with pytest.raises(binding.KmaHipError) as e:
                        second()
                    assert "error -1" in str(e.value) and word in str(e.value), (mode, sam_first, str(e.value))
    finally:
        db.close()
