"""The extended-features file (`-ef`, `<out>.mapstat`) written from the device pile-up: whole runs of examples/kmahip_map against the
compiled reference (oracle/_ref/kma -t 1) run live on the same input. The files are compared whole, byte for byte, except the `## date`
line and the `## command` line (which must be there and begin with the program's name); in every case `.res`, `.fsa`, `.aln` and the
inflated `.frag.gz` are those of the same kmahip_map run without `-ef`.

Input sets (seeded, the smallest that move every column):
  S  six templates of 600 - 1 200 bases; 1 500 reads of 150 bases over five of them with substitutions, deletions and insertions, half
     of them reverse complemented; on the sixth 300 exact reads plus 120 reads of 100 bases that start within 20 bases of position 200
     (a depth spike: nucHighDepthVariance > 0 there alone); 37 random reads and 5 reads of 8 bases (## fragmentCount is stage 1's count)
  P  600 couples from 350-base fragments of the same templates, mates of 120 bases, the same error model
  H  three templates of 300 bases, twelve reads of one template's bases 20 .. 169: nine exact, one substitution, one insertion of two
     bases, one deletion -- literal figures"""
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
COLS = ("refSequence", "readCount", "fragmentCount", "mapScoreSum", "refCoveredPositions", "refConsensusSum", "bpTotal", "depthVariance",
        "nucHighDepthVariance", "depthMax", "snpSum", "insertSum", "deletionSum", "readCountAln", "fragmentCountAln")
OURS = ("-s1dev",)          # options of kmahip_map the reference does not know


# ---- input sets ---------------------------------------------------------------------------------------------------------------------
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
    # (the sixth at full length: the spike must stand three standard deviations above a mean that 1 200 positions keep low)
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
    for _ in range(120):          # the spike
        a = 200 + int(rng.integers(0, 20))
        reads.append(s[a:a + 100].copy())
    reads += [rng.integers(0, 4, 150, dtype=np.uint8) for _ in range(37)]
    reads += [rng.integers(0, 4, 8, dtype=np.uint8) for _ in range(5)]
    order = rng.permutation(len(reads))
    reads = [np.ascontiguousarray(reads[i]) for i in order]
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, reads, lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], n_records=1500 + 300 + 120 + 37, plain={}, ref={}, got={})


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
    # the first couple is exact. A couple whose hit list comes out empty (-mrs 0.9 makes some) is filed where the last record with a list
    # was (conclave.c:123-127); in front of the first such record the reference reads a buffer ConClave has not filled yet -- what
    # stage 3a left there -- and files the couple by it. kmahip_map files such a couple nowhere; the set keeps clear of it.
    m1[0], m2[0] = seqs[0][100:220].copy(), synth.revcomp_codes(seqs[0][330:450]).copy()
    paths = [str(tmp / "r1.fq"), str(tmp / "r2.fq"), str(tmp / "int.fq")]
    with open(paths[0], "wb") as f1, open(paths[1], "wb") as f2, open(paths[2], "wb") as fi:
        for k, (x, y) in enumerate(zip(m1, m2)):
            a = b"@p%d/1\n" % k + LUT[x].tobytes() + b"\n+\n" + b"I" * len(x) + b"\n"
            b = b"@p%d/2\n" % k + LUT[y].tobytes() + b"\n+\n" + b"I" * len(y) + b"\n"
            f1.write(a); f2.write(b); fi.write(a + b)
    return dict(tmp=tmp, prefix=prefix, fq=["-ipe", paths[0], paths[1]], fq_int=["-int", paths[2]], n_records=600, plain={}, ref={}, got={})


def _h_reads(seqs):
    s = seqs[1]
    exact = s[20:170].copy()
    sub = exact.copy()
    sub[50] = (sub[50] + 1) & 3
    # two bases behind read position 60 that differ from what follows (so that the aligner cannot slide them), cut back to 150 bases
    extra = np.array([(s[81] + 1) & 3, (s[81] + 2) & 3], np.uint8)
    ins = np.concatenate([s[20:81], extra, s[81:170]])[:150]
    dele = np.concatenate([s[20:110], s[111:171]])
    return [exact.copy() for _ in range(9)] + [sub, np.ascontiguousarray(ins), np.ascontiguousarray(dele)]


def _h_templates():
    rng = np.random.default_rng(99)
    return ["hand%d" % i for i in range(3)], [rng.integers(0, 4, 300, dtype=np.uint8) for _ in range(3)]


def _make_h(tmp):
    names, seqs = _h_templates()
    prefix = str(tmp / "db")
    formats.write_index(prefix, names, seqs)
    reads = _h_reads(seqs)
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, reads, lens=None)
    return dict(tmp=tmp, prefix=prefix, fq=["-i", fq], n_records=12, plain={}, ref={}, got={}, seqs=seqs, reads=reads)


# ---- running both programs ----------------------------------------------------------------------------------------------------------
def _need_binaries():
    if not os.path.exists(KMA):
        pytest.skip("oracle/_ref/kma not built")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)


def _run_ref(tmp, fq_args, prefix, tag, extra):
    # (the reference ORs errno into its exit status, kma.c:1630: an ENOENT left behind on its -ef path makes that 2 although every
    # output is complete and closed; anything else is a failure)
    p = subprocess.run([KMA] + fq_args + ["-o", str(tmp / f"ref_{tag}"), "-t_db", prefix, "-t", "1"] + [x for x in extra if x not in OURS],
                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    assert p.returncode in (0, 2), p.returncode
    return p.stdout


def _run_map(tmp, fq_args, prefix, tag, extra, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([MAP] + fq_args + ["-t_db", prefix, "-o", str(tmp / f"got_{tag}")] + extra, check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, env=e).stdout


def _files(tmp, stem):
    return tuple(open(tmp / f"{stem}{ext}", "rb").read() for ext in (".res", ".fsa", ".aln")) + (gzip.open(tmp / f"{stem}.frag.gz", "rb").read(),)


def _without_ef(extra):
    out, skip = [], False
    for i, x in enumerate(extra):
        if skip:
            skip = False
            continue
        if x == "-ef":
            skip = i + 1 < len(extra) and not extra[i + 1].startswith("-")
            continue
        out.append(x)
    return out


def _plain_files(s, fq, extra, env):
    """the four result files of the same run WITHOUT -ef, once per set of the other options"""
    rest = _without_ef(extra)
    key = " ".join(fq + rest) + repr(sorted((env or {}).items()))
    if key not in s["plain"]:
        tag = "plain" + str(len(s["plain"]))
        _run_map(s["tmp"], fq, s["prefix"], tag, rest, env)
        assert not os.path.exists(s["tmp"] / f"got_{tag}.mapstat")          # (no file without the option)
        s["plain"][key] = _files(s["tmp"], "got_" + tag)
    return s["plain"][key]


def _parse(raw):
    """-> (header lines {key: value}, rows [dict])"""
    lines = raw.split(b"\n")
    assert lines[-1] == b""
    head = {}
    for x in lines[:6]:
        assert x.startswith(b"## "), x
        k, v = x[3:].split(b"\t", 1)
        head[k.decode()] = v
    assert lines[6] == ("# " + "\t".join(COLS)).encode()
    rows = []
    for x in lines[7:-1]:
        f = x.split(b"\t")
        assert len(f) == len(COLS), x
        rows.append({c: (v.decode() if c in ("refSequence", "depthVariance") else int(v)) for c, v in zip(COLS, f)})
    return head, rows


def _comparable(raw):
    return [x for x in raw.split(b"\n") if not x.startswith(b"## date\t") and not x.startswith(b"## command\t")]


def _case(s, tag, extra, env=None, fq=None):
    """both programs on the set with `extra`; the `.mapstat` files compared, the other four files against the run without -ef and
    against the reference's. -> (the reference's header, its rows)"""
    fq = fq or s["fq"]
    _run_ref(s["tmp"], fq, s["prefix"], tag, extra)
    assert _run_map(s["tmp"], fq, s["prefix"], tag, extra, env) == b""
    ref = open(s["tmp"] / f"ref_{tag}.mapstat", "rb").read()
    got = open(s["tmp"] / f"got_{tag}.mapstat", "rb").read()
    gl, rl = _comparable(got), _comparable(ref)
    for i, (a, b) in enumerate(zip(gl, rl)):
        assert a == b, (tag, i, a, b)
    assert len(gl) == len(rl)
    cmd = [x for x in got.split(b"\n") if x.startswith(b"## command\t")]
    assert len(cmd) == 1 and os.path.basename(cmd[0].split(b"\t", 1)[1].split(b" ")[0]) == b"kmahip_map", cmd
    assert sum(x.startswith(b"## date\t") for x in got.split(b"\n")) == 1
    mine = _files(s["tmp"], "got_" + tag)
    assert mine == _plain_files(s, fq, extra, env)
    assert mine == _files(s["tmp"], "ref_" + tag)
    head, rows = _parse(ref)
    # a row of the one file is a row of the other
    assert [r["refSequence"].encode() for r in rows] == [x.split(b"\t")[0].rstrip() for x in mine[0].split(b"\n")[1:-1]]
    assert int(head["fragmentCount"]) == s["n_records"]
    s["ref"][tag] = ref
    s["got"][tag] = got
    return head, rows


@pytest.fixture(scope="module")
def s_set(tmp_path_factory):
    _need_binaries()
    return _make_s(tmp_path_factory.mktemp("ef_s"))


@pytest.fixture(scope="module")
def p_set(tmp_path_factory):
    _need_binaries()
    return _make_p(tmp_path_factory.mktemp("ef_p"))


@pytest.fixture(scope="module")
def h_set(tmp_path_factory):
    _need_binaries()
    return _make_h(tmp_path_factory.mktemp("ef_h"))


def _s_properties(head, rows):
    """what set S is made for, read off the REFERENCE's file"""
    assert len(rows) == 6
    spike = [r for r in rows if r["nucHighDepthVariance"] > 0]
    assert [r["refSequence"] for r in spike] == ["tmpl5 extended features"] and spike[0]["depthMax"] > 150
    noisy = [r for r in rows if r["snpSum"] > 0 and r["insertSum"] > 0 and r["deletionSum"] > 0]
    assert len(noisy) >= 5
    assert int(head["fragmentCount"]) != sum(r["fragmentCount"] for r in rows)
    assert all(float(r["depthVariance"]) > 0 for r in rows)


# ---- cases 1 - 5, 8: single end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,extra,env", [("1t1", ["-1t1", "-ef"], None), ("s1dev", ["-1t1", "-ef", "-s1dev"], None),
                                           ("batches", ["-1t1", "-ef"], {"KMAHIP_MAP_BATCH": "500"})], ids=["1t1", "s1dev", "batches"])
def test_single_end_1t1(s_set, tag, extra, env):
    """case 1: -1t1 -ef, stage 1 on the host and on the device, and the counts summed over four batches"""
    head, rows = _case(s_set, tag, extra, env)
    _s_properties(head, rows)
    assert all(r["readCountAln"] == r["readCount"] == r["fragmentCount"] == r["fragmentCountAln"] for r in rows)


def test_read_filter_drops_reads(s_set):
    """case 2: -mrs 0.9 drops reads in stage 3c: readCountAln < readCount, and mapScoreSum is the kept reads' sum, not ConClave's"""
    head, rows = _case(s_set, "mrs", ["-1t1", "-ef", "-mrs", "0.9"])
    assert any(r["readCountAln"] != r["readCount"] for r in rows)
    res = {x.split(b"\t")[0].rstrip().decode(): int(x.split(b"\t")[1]) for x in open(s_set["tmp"] / "ref_mrs.res", "rb").read().split(b"\n")[1:-1]}
    assert any(res[r["refSequence"]] != r["mapScoreSum"] for r in rows)


def test_default_mode(s_set):
    """case 3a: -ef alone (the chain finder's records)"""
    head, rows = _case(s_set, "chain", ["-ef"])
    _s_properties(head, rows)


def test_dense(s_set):
    """case 3b: -dense has no insertion columns"""
    head, rows = _case(s_set, "dense", ["-1t1", "-ef", "-dense"])
    assert len(rows) == 6 and all(r["insertSum"] == 0 for r in rows) and any(r["deletionSum"] > 0 for r in rows)


@pytest.mark.parametrize("tag,extra", [("mem", ["-1t1", "-ef", "-mem_mode"]), ("ef2", ["-1t1", "-ef", "2"])], ids=["mem_mode", "ef2"])
def test_mem_mode_and_a_value(s_set, tag, extra):
    """case 4: -mem_mode, and -ef with a number behind it (kma.c:938-948), which gives the same file"""
    head, rows = _case(s_set, tag, extra)
    _s_properties(head, rows)
    if tag == "ef2":
        if "1t1" not in s_set["got"]:
            _case(s_set, "1t1", ["-1t1", "-ef"])
        assert _comparable(s_set["got"]["ef2"]) == _comparable(s_set["got"]["1t1"])


def test_identity_threshold_drops_rows(s_set):
    """case 5: -ID 99.5 leaves the rows `.res` has (the noisy templates' consensus misses a position here and there)"""
    head, rows = _case(s_set, "id", ["-1t1", "-ef", "-ID", "99.5"])
    if "1t1" not in s_set["ref"]:
        _case(s_set, "1t1", ["-1t1", "-ef"])
    assert len(rows) < len(_parse(s_set["ref"]["1t1"])[1])


def test_with_sam(s_set):
    """case 8: -sam 4 beside -ef: the same `.mapstat` as without it, the same SAM body as without -ef"""
    s = s_set
    if "1t1" not in s["got"]:
        _case(s, "1t1", ["-1t1", "-ef"])
    body = lambda out: [x for x in out.split(b"\n") if not x.startswith(b"@PG")]  # noqa: E731
    _run_ref(s["tmp"], s["fq"], s["prefix"], "sam", ["-1t1", "-ef", "-sam", "4"])
    both = _run_map(s["tmp"], s["fq"], s["prefix"], "sam", ["-1t1", "-ef", "-sam", "4"])
    alone = _run_map(s["tmp"], s["fq"], s["prefix"], "samonly", ["-1t1", "-sam", "4"])
    assert body(both) == body(alone) and len(body(both)) > 1500
    got = open(s["tmp"] / "got_sam.mapstat", "rb").read()
    assert _comparable(got) == _comparable(s["got"]["1t1"])
    assert _comparable(got) == _comparable(open(s["tmp"] / "ref_sam.mapstat", "rb").read())
    assert _files(s["tmp"], "got_sam") == _files(s["tmp"], "got_samonly") == _files(s["tmp"], "ref_sam")


# ---- case 6: pairs --------------------------------------------------------------------------------------------------------------------
def test_pairs_default_mode(p_set):
    """-ipe -ef: union pairing, the singly loaded records through the chain finder; a couple is one fragment and two reads"""
    head, rows = _case(p_set, "ipe", ["-ef"])
    assert len(rows) == 6
    assert all(1.8 * r["fragmentCount"] < r["readCount"] <= 2 * r["fragmentCount"] for r in rows)
    assert any(r["snpSum"] > 0 and r["insertSum"] > 0 and r["deletionSum"] > 0 for r in rows)


def test_pairs_1t1_apm_p(p_set):
    head, rows = _case(p_set, "apmp", ["-1t1", "-apm", "p", "-ef"])
    assert len(rows) == 6 and all(r["readCount"] > r["fragmentCount"] for r in rows)


def test_pairs_read_filter(p_set):
    """-mrs 0.9 on pairs: mates are dropped one by one, so the fix-up of ef.c:71 and the flag rule of alnToMat both show"""
    head, rows = _case(p_set, "apmpmrs", ["-1t1", "-apm", "p", "-ef", "-mrs", "0.9"])
    assert any(r["fragmentCountAln"] * 2 != r["readCountAln"] for r in rows)
    assert any(r["readCountAln"] != r["readCount"] for r in rows)


def test_pairs_interleaved(p_set):
    head, rows = _case(p_set, "int", ["-1t1", "-ef"], fq=p_set["fq_int"])
    assert len(rows) == 6 and all(r["readCount"] > r["fragmentCount"] for r in rows)


# ---- case 7: by hand ------------------------------------------------------------------------------------------------------------------
H_FIGURES = dict(snpSum=1, insertSum=2, deletionSum=1, depthMax=12, readCount=12, readCountAln=12, fragmentCount=12, fragmentCountAln=12)


def test_by_hand(h_set):
    head, rows = _case(h_set, "h", ["-1t1", "-ef"])
    _, mine = _parse(h_set["got"]["h"])
    for rr in (rows, mine):
        assert len(rr) == 1 and rr[0]["refSequence"] == "hand1"
        assert {k: rr[0][k] for k in H_FIGURES} == H_FIGURES, rr[0]


# ---- case 9: refusals ------------------------------------------------------------------------------------------------------------------
def test_several_ranks_are_refused_by_name(s_set):
    s = s_set
    for args, env, word in ((["-ef", "-gpus", "2"], {}, b"-gpus"), (["-ef"], {"KMAHIP_MAP_ONE_BATCH": "1"}, b"KMAHIP_MAP_ONE_BATCH"),
                            (["-ef"], {"KMAHIP_COMM_FORCE_RCCL": "1"}, b"KMAHIP_COMM_FORCE_RCCL")):
        e = dict(os.environ)
        e.update(env)
        p = subprocess.run([MAP] + s["fq"] + ["-1t1"] + args + ["-t_db", s["prefix"], "-o", str(s["tmp"] / "refused")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
        assert p.returncode == 2 and b"-ef" in p.stderr and word in p.stderr, (args, p.returncode, p.stderr)
        assert not os.path.exists(s["tmp"] / "refused.mapstat") and not os.path.exists(s["tmp"] / "refused.res")


def test_mt1_writes_no_mapstat(s_set):
    """runKMA_Mt1 writes no extended-features file (mt1.c:313, 378): -Mt1 1 -ef is accepted and leaves none, on either side"""
    s = s_set
    _run_ref(s["tmp"], s["fq"], s["prefix"], "mt1", ["-Mt1", "1", "-ef"])
    _run_map(s["tmp"], s["fq"], s["prefix"], "mt1", ["-Mt1", "1", "-ef"])
    assert not os.path.exists(s["tmp"] / "ref_mt1.mapstat") and not os.path.exists(s["tmp"] / "got_mt1.mapstat")
    assert _files(s["tmp"], "got_mt1") == _files(s["tmp"], "ref_mt1")


# ---- case 10: the library ---------------------------------------------------------------------------------------------------------------
def test_library_needs_the_pile_up(h_set):
    db = binding.KmaHipDB(h_set["prefix"])
    try:
        D = int(db.info.DB_size)
        with pytest.raises(binding.KmaHipError) as e:
            db.assemble_ef(np.zeros(1, np.int32), (np.zeros((1, 10), np.int32),), dict(depth=np.zeros(D, np.int64)))
        assert "error -1" in str(e.value) and "pile-up" in str(e.value)
    finally:
        db.close()


def test_library_figures_by_hand(h_set):
    """kmahip_assemble_ef behind kmahip_assemble2 through the stage entry points, on set H"""
    h = h_set
    batch = formats.pack_ragged(h["reads"])
    db = binding.KmaHipDB(h["prefix"])
    try:
        got, hits = db.map_se(batch)
        cc = db.conclave_se(batch.length, got[2], hits)
        assert np.all(np.abs(cc["tmpl"]) == 2)
        traces = db.align_trace(batch, hits["rc"], cc["tmpl"])
        asm = db.assemble(batch, hits["rc"], cc["tmpl"], traces)
        ef = db.assemble_ef(cc["tmpl"], traces, asm)
        t = 2
        assert (int(ef["snp_sum"][t]), int(ef["insert_sum"][t]), int(ef["deletion_sum"][t]), int(ef["max_depth"][t]), int(ef["read_count_aln"][t]),
                int(ef["fragment_count_aln"][t])) == (1, 2, 1, 12, 12, 12)
        # the called columns: 20 .. 167 twelve deep (the read with a base deleted has a gap there: counted), 168 and 169 eleven deep (the
        # read with two bases inserted ends two columns early), 170 one deep (the read with the deletion reaches it); the two insertion
        # columns, one base and eleven gaps each, are called '-' and count neither for the depth nor for its squares
        depth = int(asm["depth"][t])
        assert int(asm["aln_len"][t]) == 151 and depth == 148 * 12 + 2 * 11 + 1
        assert int(ef["depth_var"][t]) == 148 * 144 + 2 * 121 + 1
        assert abs(float(ef["var"][t]) - (int(ef["depth_var"][t]) / 300 - (depth / 300) ** 2)) < 1e-9
        assert int(ef["score_sum"][t]) > 0 and int(ef["nuc_high_var"][t]) == 0
        for x in (1, 3):
            assert all(int(ef[k][x]) == 0 for k in ("snp_sum", "insert_sum", "deletion_sum", "max_depth", "read_count_aln", "depth_var"))
    finally:
        db.close()
