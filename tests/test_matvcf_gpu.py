"""The count matrix and the VCF file (`-matrix`, `-vcf [n]`: `<out>.mat.gz`, `<out>.vcf.gz`) written from the device pile-up: whole runs
of examples/kmahip_map against the compiled reference (oracle/_ref/kma -t 1) run live on the same input and the same -t_db path. The two
files are compared inflated, whole, byte for byte (neither has a date line); in every case `.res`, `.fsa`, `.aln` and the inflated
`.frag.gz` are those of the same kmahip_map run without the two options.

Input sets (seeded):
  S  the single-end set of test_mapstat_gpu.py (templates of default_rng(2024), reads of default_rng(7))
  P  its couples (default_rng(8))
  V  by hand: three templates of 300 bases (default_rng(99)), 20 reads over positions 20 .. 171 of template 1; every read substitutes
     position 50 and deletes position 110, reads 0-7 substitute position 140, reads 0-13 insert two bases behind position 80, reads 14-16
     insert one base behind position 125; cut to 150 bases. The rows with an ALT are asserted literally (tests/golden/matvcf_v holds
     the reference's two files for the tests that run without the reference binary)
  B  saturation: 66 000 copies of template 1's bases 20 .. 169 (the 16-bit counters of the reference stop at 65 535)
  L  one template of 20 000 bases, 600 noisy reads spread over it, 40 exact reads over 8 100 .. 8 300 of which 30 insert two bases behind
     position 8 191: the last position of a segment of the column kernels, its chain of insertion columns hanging on the next one"""
import gzip
import os
import subprocess

import numpy as np
import pytest

from kma_amd import binding, formats, synth
from matvcf_sets import v_reads, v_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMA = os.path.join(ROOT, "oracle", "_ref", "kma")
MAP = os.path.join(ROOT, "examples", "kmahip_map")
GOLDEN = os.path.join(ROOT, "tests", "golden", "matvcf_v")
LUT = np.frombuffer(b"ACGTN", dtype=np.uint8)
OURS = ("-s1dev",)          # options of kmahip_map the reference does not know
TIMEOUT = 120


# ---- input sets (S and P: the generators of test_mapstat_gpu.py) ----------------------------------------------------------------------
def _noisy(rng, w, sub=0.02, dele=0.01, ins=0.01):
    w = w.copy()
    m = rng.random(len(w)) < sub
    w[m] = (w[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
    w = w[rng.random(len(w)) >= dele]
    ipos = np.nonzero(rng.random(len(w)) < ins)[0]
    if len(ipos):
        w = np.insert(w, ipos, rng.integers(0, 4, len(ipos), dtype=np.uint8))
    return np.ascontiguousarray(w)


def _templates():
    rng = np.random.default_rng(2024)
    seqs = [rng.integers(0, 4, int(rng.integers(600, 1201)) if i < 5 else 1200, dtype=np.uint8) for i in range(6)]
    return ["tmpl%d extended features" % i for i in range(6)], seqs


def _make_s(tmp):
    names, seqs = _templates()
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    rng = np.random.default_rng(7)
    reads = []
    for _ in range(1500):
        s = seqs[int(rng.integers(0, 5))]
        a = int(rng.integers(0, len(s) - 160))
        r = _noisy(rng, s[a:a + 160])[:150]
        reads.append(synth.revcomp_codes(r).copy() if rng.random() < 0.5 else r)
    s = seqs[5]
    for _ in range(300):
        a = int(rng.integers(0, len(s) - 150 + 1))
        reads.append(s[a:a + 150].copy())
    for _ in range(120):
        a = 200 + int(rng.integers(0, 20))
        reads.append(s[a:a + 100].copy())
    reads += [rng.integers(0, 4, 150, dtype=np.uint8) for _ in range(37)]
    reads += [rng.integers(0, 4, 8, dtype=np.uint8) for _ in range(5)]
    order = rng.permutation(len(reads))
    reads = [np.ascontiguousarray(reads[i]) for i in order]
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, reads, lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], plain={})


def _make_p(tmp):
    names, seqs = _templates()
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    rng = np.random.default_rng(8)
    m1, m2 = [], []
    for _ in range(600):
        s = seqs[int(rng.integers(0, 6))]
        a = int(rng.integers(0, len(s) - 350 + 1))
        frag = s[a:a + 350]
        x, y = _noisy(rng, frag[:130])[:120], _noisy(rng, synth.revcomp_codes(frag[-130:]))[:120]
        if rng.random() < 0.5:
            x, y = y, x
        m1.append(x); m2.append(y)
    m1[0], m2[0] = seqs[0][100:220].copy(), synth.revcomp_codes(seqs[0][330:450]).copy()
    paths = [str(tmp / "r1.fq"), str(tmp / "r2.fq"), str(tmp / "int.fq")]
    with open(paths[0], "wb") as f1, open(paths[1], "wb") as f2, open(paths[2], "wb") as fi:
        for k, (x, y) in enumerate(zip(m1, m2)):
            a = b"@p%d/1\n" % k + LUT[x].tobytes() + b"\n+\n" + b"I" * len(x) + b"\n"
            b = b"@p%d/2\n" % k + LUT[y].tobytes() + b"\n+\n" + b"I" * len(y) + b"\n"
            f1.write(a); f2.write(b); fi.write(a + b)
    return dict(tmp=tmp, prefix=prefix, fq=["-ipe", paths[0], paths[1]], fq_int=["-int", paths[2]], plain={})


def _make_v(tmp):
    names, seqs = v_templates()
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    reads = v_reads(seqs)
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, reads, lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], plain={}, seqs=seqs, reads=reads)


def _make_b(tmp):
    names, seqs = v_templates()
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    fq = str(tmp / "reads.fq")
    one = LUT[seqs[1][20:170]].tobytes()
    with open(fq, "wb") as f:
        f.write(b"".join(b"@b%d\n" % i + one + b"\n+\n" + b"I" * 150 + b"\n" for i in range(66000)))
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], plain={})


def _make_l(tmp):
    rng = np.random.default_rng(11)
    s = rng.integers(0, 4, 20000, dtype=np.uint8)
    prefix = str(tmp / "db")
    formats.write_index(prefix, ["long template"], [s])
    reads = []
    for _ in range(600):
        a = int(rng.integers(0, len(s) - 160))
        reads.append(_noisy(rng, s[a:a + 160])[:150])
    extra = np.array([(s[8192] + 1) & 3, (s[8192] + 2) & 3], np.uint8)
    for i in range(40):
        a = 8100 + int(rng.integers(0, 51))
        r = s[a:a + 150].copy()
        if i < 30:
            r = np.concatenate([s[a:8192], extra, s[8192:a + 150]])[:150]
        reads.append(np.ascontiguousarray(r))
    order = rng.permutation(len(reads))
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, [reads[i] for i in order], lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], plain={}, seq=s)


# ---- running both programs ----------------------------------------------------------------------------------------------------------
def _need_binaries():
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)


def _run_ref(tmp, fq_args, prefix, tag, extra):
    # (the reference ORs errno into its exit status, kma.c:1630: 2 with every output complete is an ENOENT left behind)
    p = subprocess.run([KMA] + fq_args + ["-o", str(tmp / f"ref_{tag}"), "-t_db", prefix, "-t", "1"] + [x for x in extra if x not in OURS],
                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
    assert p.returncode in (0, 2), p.returncode
    return p.stdout


def _run_map(tmp, fq_args, prefix, tag, extra, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([MAP] + fq_args + ["-t_db", prefix, "-o", str(tmp / f"got_{tag}")] + extra, check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, env=e, timeout=TIMEOUT).stdout


def _files(tmp, stem):
    return tuple(open(tmp / f"{stem}{ext}", "rb").read() for ext in (".res", ".fsa", ".aln")) + (gzip.open(tmp / f"{stem}.frag.gz", "rb").read(),)


def _without(extra):
    out, skip = [], False
    for i, x in enumerate(extra):
        if skip:
            skip = False
            continue
        if x == "-matrix":
            continue
        if x == "-vcf":
            skip = i + 1 < len(extra) and not extra[i + 1].startswith("-")
            continue
        out.append(x)
    return out


def _plain_files(s, fq, extra, env):
    """the four result files (and the standard output) of the same run WITHOUT -matrix / -vcf, once per set of the other options"""
    rest = _without(extra)
    key = " ".join(fq + rest) + repr(sorted((env or {}).items()))
    if key not in s["plain"]:
        tag = "plain" + str(len(s["plain"]))
        out = _run_map(s["tmp"], fq, s["prefix"], tag, rest, env)
        assert not os.path.exists(s["tmp"] / f"got_{tag}.mat.gz") and not os.path.exists(s["tmp"] / f"got_{tag}.vcf.gz")          # (no file without the options)
        s["plain"][key] = _files(s["tmp"], "got_" + tag) + (out,)
    return s["plain"][key]


def _inflate(path):
    return gzip.open(path, "rb").read()


def _case(s, tag, extra, env=None, fq=None):
    """both programs on the set with `extra`: the two files compared inflated, the other four against the run without the options.
    -> (matrix text or None, VCF text or None), the reference's"""
    fq = fq or s["fq"]
    _run_ref(s["tmp"], fq, s["prefix"], tag, extra)
    out = _run_map(s["tmp"], fq, s["prefix"], tag, extra, env)
    res = []
    for opt, ext in (("-matrix", ".mat.gz"), ("-vcf", ".vcf.gz")):
        gp, rp = s["tmp"] / f"got_{tag}{ext}", s["tmp"] / f"ref_{tag}{ext}"
        if opt not in extra:
            assert not os.path.exists(gp) and not os.path.exists(rp)
            res.append(None)
            continue
        got, ref = _inflate(gp), _inflate(rp)
        if got != ref:
            gl, rl = got.split(b"\n"), ref.split(b"\n")
            for i, (a, b) in enumerate(zip(gl, rl)):
                assert a == b, (tag, ext, i, a, b)
            assert len(gl) == len(rl), (tag, ext, len(gl), len(rl))
        res.append(ref)
    plain = _plain_files(s, fq, extra, env)
    assert _files(s["tmp"], "got_" + tag) == plain[:4]
    no_pg = lambda raw: [x for x in raw.split(b"\n") if not x.startswith(b"@PG")]  # noqa: E731   (the SAM text's @PG line names the run)
    assert no_pg(out) == no_pg(plain[4])
    return res


def _vcf_rows(vcf):
    return [x.split(b"\t") for x in vcf.split(b"\n") if x and not x.startswith(b"#")]


def _mat_templates(mat):
    return [x[1:] for x in mat.split(b"\n") if x.startswith(b"#")]


def _res_names(s, tag):
    return [x.split(b"\t")[0] for x in open(s["tmp"] / f"got_{tag}.res", "rb").read().split(b"\n")[1:-1]]


@pytest.fixture(scope="module")
def s_set(tmp_path_factory):
    _need_binaries()
    return _make_s(tmp_path_factory.mktemp("mv_s"))


@pytest.fixture(scope="module")
def p_set(tmp_path_factory):
    _need_binaries()
    return _make_p(tmp_path_factory.mktemp("mv_p"))


@pytest.fixture(scope="module")
def v_set(tmp_path_factory):
    _need_binaries()
    return _make_v(tmp_path_factory.mktemp("mv_v"))


BOTH = ["-matrix", "-vcf"]


# ---- set S ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,extra", [
    ("1t1", ["-1t1"] + BOTH),
    ("chain", BOTH),
    ("dense", ["-1t1", "-dense"] + BOTH),
    ("mem", ["-1t1", "-mem_mode"] + BOTH),
    ("bcbcg", ["-1t1", "-bc", "0.9", "-bcg"] + BOTH),
    ("mt1_6", ["-Mt1", "6"] + BOTH),
    ("mt1_2nano", ["-Mt1", "2", "-bcNano"] + BOTH),
    ("s1dev", ["-1t1", "-s1dev"] + BOTH),
], ids=["1t1", "default_mode", "dense", "mem_mode", "bc0.9_bcg", "Mt1_6", "Mt1_2_bcNano", "s1dev"])
def test_single_end(s_set, tag, extra):
    mat, vcf = _case(s_set, tag, extra)
    names = _res_names(s_set, tag)
    assert len(names) == (1 if "-Mt1" in extra else 6)
    # a template is in all files or in none
    assert [x.rstrip() for x in names] == [x.rstrip() for x in _mat_templates(mat)]
    assert set(r[0] for r in _vcf_rows(vcf)) <= set(x.rstrip() for x in names)
    assert all(r[6] == b"." for r in _vcf_rows(vcf))
    if tag == "dense":
        assert b"\n-\t" not in mat          # (no insertion columns)
    elif "-Mt1" not in extra:
        assert b"\n-\t" in mat and any(r[1] == b"0" for r in _vcf_rows(vcf))


def test_bcnano_prints_pass_rows(s_set):
    """-bcNano: the only S case in which the reference prints PASS rows"""
    mat, vcf = _case(s_set, "nano", ["-1t1", "-bcNano"] + BOTH)
    assert sum(r[9].endswith(b":PASS") for r in _vcf_rows(vcf)) == 47


def test_filter_column_filled(s_set):
    """-bcd 20 -vcf 2: the depth gate prints rows, the FILTER column holds what FT holds"""
    mat, vcf = _case(s_set, "bcd20", ["-1t1", "-bcd", "20", "-matrix", "-vcf", "2"])
    rows = _vcf_rows(vcf)
    assert len(rows) == 672
    assert all(r[6] != b"." and r[9].endswith(b":" + r[6]) for r in rows)


def test_matrix_alone(s_set):
    mat, vcf = _case(s_set, "matonly", ["-1t1", "-matrix"])
    assert vcf is None and len(_mat_templates(mat)) == 6


def test_vcf_alone(s_set):
    mat, vcf = _case(s_set, "vcfonly", ["-1t1", "-vcf"])
    assert mat is None and len(_vcf_rows(vcf)) > 0


def test_with_ef_and_sam(s_set):
    """-ef and -sam 4 beside the two: `.mapstat` and the SAM text are those of the run without -matrix -vcf (the date and command lines of
    `.mapstat`, and the @PG line, name the run)"""
    s = s_set
    _case(s, "efsam", ["-1t1", "-matrix", "-vcf", "-ef", "-sam", "4"])          # (the standard output is compared there, @PG line apart below)
    keep = lambda raw: [x for x in raw.split(b"\n") if not x.startswith(b"## date\t") and not x.startswith(b"## command\t")]  # noqa: E731
    key = [k for k in s["plain"] if "-ef -sam 4" in k]
    assert len(key) == 1
    tag = "plain%d" % list(s["plain"]).index(key[0])
    assert keep(open(s["tmp"] / "got_efsam.mapstat", "rb").read()) == keep(open(s["tmp"] / f"got_{tag}.mapstat", "rb").read())


def test_no_template_passes(s_set):
    """-md 100000: no `.res` row, the matrix inflates to nothing and the VCF to its header"""
    mat, vcf = _case(s_set, "md", ["-1t1", "-md", "100000"] + BOTH)
    assert mat == b"" and _vcf_rows(vcf) == [] and vcf.startswith(b"##fileformat=VCFv4.2\n") and vcf.endswith(b"\tdb\n")
    assert _res_names(s_set, "md") == []


# ---- set P ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,extra,which", [("ipe1t1", ["-1t1"] + BOTH, "fq"), ("int", ["-1t1"] + BOTH, "fq_int"), ("ipe", BOTH, "fq")],
                         ids=["ipe_1t1", "int_1t1", "ipe_default_mode"])
def test_pairs(p_set, tag, extra, which):
    mat, vcf = _case(p_set, tag, extra, fq=p_set[which])
    assert len(_mat_templates(mat)) == 6 and len(_vcf_rows(vcf)) > 0


# ---- set V ------------------------------------------------------------------------------------------------------------------------------
V_ROWS = [x.encode() for x in open(os.path.join(GOLDEN, "alt_rows.txt")).read().split("\n") if x] if os.path.exists(os.path.join(GOLDEN, "alt_rows.txt")) else None


def test_by_hand(v_set):
    """set V: the seven rows with an ALT, literally. The reference prints 156 rows for the set as described above -- an all-zero row for each of
    the 149 positions no read reaches (0 .. 19, 171 .. 299) and the seven --, the lookahead row at POS 81 among them"""
    mat, vcf = _case(v_set, "v", ["-1t1"] + BOTH)
    rows = _vcf_rows(vcf)
    assert len(rows) == 156          # (149 all-zero rows of the positions no read reaches, and the seven below)
    alt = [b"\t".join(r) for r in rows if r[4] != b"."]
    assert alt == V_ROWS and len(alt) == 7
    pos = [(r[1], r[3], r[4]) for r in rows if r[4] != b"."]
    assert pos == [(b"51", b"G", b"T"), (b"81", b"C", b"C"), (b"0", b"<->", b"g"), (b"0", b"<->", b"t"), (b"111", b"G", b"<->"), (b"141", b"A", b"a"), (b"171", b"A", b"a")]
    # the files the tests without the reference binary use are the reference's
    assert mat == open(os.path.join(GOLDEN, "ref.mat"), "rb").read() and vcf == open(os.path.join(GOLDEN, "ref.vcf"), "rb").read()


# ---- set B ------------------------------------------------------------------------------------------------------------------------------
def test_saturation(tmp_path_factory):
    _need_binaries()
    s = _make_b(tmp_path_factory.mktemp("mv_b"))
    mat, vcf = _case(s, "b", ["-1t1"] + BOTH)
    assert mat.count(b"65535") == 150


# ---- set L ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l_set(tmp_path_factory):
    _need_binaries()
    return _make_l(tmp_path_factory.mktemp("mv_l"))


@pytest.mark.parametrize("chunk", [None, "4096"], ids=["default_chunk", "chunk_4096"])
def test_segment_boundary(l_set, chunk):
    mat, vcf = _case(l_set, "l" + (chunk or ""), ["-1t1"] + BOTH, env={"KMAHIP_MAT_CHUNK": chunk} if chunk else None)
    lines = mat.split(b"\n")
    # the row of template position 8191 (line 0 is the name; the noisy reads leave insertion columns in front), then the two insertion columns
    s = l_set["seq"]
    at = [i for i, x in enumerate(lines) if i and x and not x.startswith(b"-")][8191]
    assert lines[at].startswith(LUT[s[8191]:s[8191] + 1].tobytes() + b"\t")
    assert lines[at + 1].startswith(b"-\t") and lines[at + 2].startswith(b"-\t") and sum(int(x) for x in lines[at + 1].split(b"\t")[1:5]) >= 30
    assert not lines[at + 3].startswith(b"-")
    assert len(mat) > 64 * 4096          # (the small chunk size makes more than sixty chunks)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_several_ranks_are_refused_by_name(s_set):
    s = s_set
    for opt in (["-matrix"], ["-vcf"]):
        for args, env, word in ((["-gpus", "2"], {}, b"-gpus"), ([], {"KMAHIP_MAP_ONE_BATCH": "1"}, b"KMAHIP_MAP_ONE_BATCH"),
                                ([], {"KMAHIP_COMM_FORCE_RCCL": "1"}, b"KMAHIP_COMM_FORCE_RCCL"), ([], {"KMAHIP_RANK": "0", "KMAHIP_WORLD": "2"}, b"-gpus")):
            e = dict(os.environ)
            e.update(env)
            p = subprocess.run([MAP] + s["fq"] + ["-1t1"] + opt + args + ["-t_db", s["prefix"], "-o", str(s["tmp"] / "refused")], stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, env=e, timeout=TIMEOUT)
            assert p.returncode == 2 and opt[0].encode() in p.stderr and word in p.stderr, (opt, args, p.returncode, p.stderr)
            assert not os.path.exists(s["tmp"] / "refused.mat.gz") and not os.path.exists(s["tmp"] / "refused.vcf.gz") and not os.path.exists(s["tmp"] / "refused.res")


def test_invalid_vcf_value(s_set):
    s = s_set
    p = subprocess.run([MAP] + s["fq"] + ["-1t1", "-vcf", "x2", "-t_db", s["prefix"], "-o", str(s["tmp"] / "invalid")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=TIMEOUT)
    assert p.returncode == 1 and p.stderr == b'Invalid argument at "-vcf".\n'
    q = subprocess.run([KMA] + s["fq"] + ["-1t1", "-vcf", "x2", "-t_db", s["prefix"], "-o", str(s["tmp"] / "invalid_ref")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=TIMEOUT)
    assert (q.returncode, q.stderr) == (p.returncode, p.stderr)


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_library_needs_the_pile_up(tmp_path):
    names, seqs = v_templates()
    prefix = str(tmp_path / "db")
    formats.write_index(prefix, names, seqs)
    db = binding.KmaHipDB(prefix)
    try:
        D = int(db.info.DB_size)
        for call, word in ((db.assemble_matrix, "count matrix"), (db.assemble_vcf, "VCF records")):
            with pytest.raises(binding.KmaHipError) as e:
                call(np.ones(D, np.uint8))
            assert "error -1" in str(e.value) and "pile-up" in str(e.value) and word in str(e.value)
    finally:
        db.close()


def test_library_against_recorded_files(tmp_path):
    """kmahip_assemble_matrix_dev / kmahip_assemble_vcf_dev behind kmahip_assemble2 through the stage entry points, on set V, against the
    reference's two files as recorded (no reference binary needed): every chunk size gives the same text, a mask of zeros gives nothing"""
    names, seqs = v_templates()
    prefix = str(tmp_path / "db")
    formats.write_index(prefix, names, seqs)
    batch = formats.pack_ragged(v_reads(seqs))
    ref_mat = open(os.path.join(GOLDEN, "ref.mat"), "rb").read()
    ref_vcf = open(os.path.join(GOLDEN, "ref.vcf"), "rb").read()
    db = binding.KmaHipDB(prefix)
    try:
        D = int(db.info.DB_size)
        got, hits = db.map_se(batch)
        cc = db.conclave_se(batch.length, got[2], hits)
        assert np.all(np.abs(cc["tmpl"]) == 2)
        traces = db.align_trace(batch, hits["rc"], cc["tmpl"])
        db.assemble(batch, hits["rc"], cc["tmpl"], traces)
        mask = np.zeros(D, np.uint8)
        mask[2] = 1
        for chunk in (0, 256, 1000):
            text, per = db.assemble_matrix(mask, chunk)
            assert b"#hand1\n" + text + b"\n" == ref_mat, chunk
            assert per[2] == len(text) and per.sum() == len(text)
        recs, per = db.assemble_vcf(mask)
        assert per[2] == len(recs) == 156 and per.sum() == 156
        lines = b"".join(db.vcf_line("hand1", r) for r in recs)
        assert binding.KmaHipDB.vcf_header(prefix) + lines == ref_vcf
        text, per = db.assemble_matrix(np.zeros(D, np.uint8))
        recs, per2 = db.assemble_vcf(np.zeros(D, np.uint8))
        assert text == b"" and per.sum() == 0 and len(recs) == 0 and per2.sum() == 0
    finally:
        db.close()
