"""kmahip_index_append (`kmahip_index -t_db`, binding.index_append) on the device: the expansion of an old .comp.b into pairs against
the restatement of tests/index_append_util.py; every recorded case of tests/golden/index_append/ against the reference's files and,
byte for byte, against our own fresh build of the concatenated FASTA; the 16- to 32-bit crossing of the value lists; and what an index
is for: kmahip_map and the reference binary map reads against an index we appended and against the reference's with one result.
Integers and bytes only: no tolerance.

The direct-address case is held to the reference's FRESH build of the concatenation: its own append onto such an index ends with a
segmentation fault at k = 10 (and at k = 9 writes a value array a thousand times the fresh build's), so it is no oracle there."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import dist_util
import index_append_util as iau
import proxi_util
import sparse_index_util as siu
from kma_amd import binding, formats, synth

pytestmark = pytest.mark.gpu
TIMEOUT = 120
EXTS = (".comp.b", ".length.b", ".name", ".seq.b")
BUILD = {"A_k16": dict(k=16), "A_k12": dict(k=12), "A_TG": dict(k=16, sparse="TG"), "A_none": dict(k=16, sparse="-"), "A_k10": dict(k=10)}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("index_append_gpu")


@pytest.fixture(scope="module")
def built():
    proxi_util.build_map()


@pytest.fixture(scope="module")
def ref(tmp):
    """name -> prefix of a recorded index of the reference (old or appended), unpacked once and never written to"""
    os.makedirs(tmp / "ref")
    out = {name: iau.unpack(name, tmp / "ref") for name in list(iau.OLD) + list(iau.RECORDED)}
    for name in ("decon_only", "append_decon"):
        out[name + ".decon"] = iau.unpack_decon(name, tmp / "ref")
    return out


@pytest.fixture(scope="module")
def fresh(tmp):
    """(old index, with b, with decon) -> prefix of OUR fresh build of the concatenated FASTA, built once"""
    made = {}
    os.makedirs(tmp / "fresh")

    def get(old, with_b=True, decon=False):
        key = (old, with_b, decon)
        if key not in made:
            p = str(tmp / "fresh" / ("%s_%d_%d" % key))
            binding.index_build([iau.fasta("a")] + ([iau.fasta("b")] if with_b else []), p, decon=[iau.fasta("c")] if decon else None, **BUILD[old])
            made[key] = p
        return made[key]
    return get


def snapshot(prefix, exts=EXTS):
    return {e: open(prefix + e, "rb").read() for e in exts}


# ---- the expansion alone --------------------------------------------------------------------------------------------------------
def expansion_equals(prefix):
    c = iau.Comp(prefix + ".comp.b")
    got = binding.index_expand(prefix)
    assert got.dtype == np.uint64 and len(got) == int(c.values.astype(np.int64)[c.vidx.astype(np.int64)].sum())
    # the device writes the pairs in the order of the file's k-mers, each list as the file holds it
    assert np.array_equal(got >> np.uint64(32), np.repeat(c.keys.astype(np.uint64), c.values.astype(np.int64)[c.vidx.astype(np.int64)]))
    assert np.array_equal(np.sort(got), iau.expand(c))
    return c, got


@pytest.mark.parametrize("name", ["A_k16", "A_TG", "A_none", "A_k10", "k16"])
def test_expansion_of_the_fixture_indexes(name, ref):
    c, got = expansion_equals(ref[name])
    assert c.mega == (name == "A_k10") and len(got) > 500


@pytest.mark.parametrize("case,longest,shared", [("edge", 65, 25), ("wide", 300, 1)])
def test_expansion_of_long_and_shared_lists(case, longest, shared, tmp):
    """tests/golden/tdist: lists of 1, 2, 63, 64 and 65 members and one list shared by 25 k-mers; a list of 300"""
    c, got = expansion_equals(dist_util.unpack_index(case, tmp))
    sizes = c.values.astype(np.int64)[c.vidx.astype(np.int64)]
    assert int(sizes.max()) == longest and int(np.bincount(c.vidx.astype(np.int64)).max()) >= shared
    if case == "edge":
        assert {1, 2, 63, 64, 65} <= set(sizes.tolist())


def test_expansion_of_32_bit_lists(tmp):
    rng = np.random.default_rng(11)
    seqs = [row for row in rng.integers(0, 4, (65540, 40), dtype=np.uint8)]
    prefix = str(tmp / "wide32")
    formats.write_index(prefix, ["t%d" % i for i in range(len(seqs))], seqs)
    c, got = expansion_equals(prefix)
    assert c.DB_size == 65541 and c.values.dtype == np.uint32 and int((got & np.uint64(0xFFFFFFFF)).max()) == 65540


# ---- every recorded case ---------------------------------------------------------------------------------------------------------
def append(how, db, parts, out, decon, line):
    files = [iau.fasta(x) for x in parts]
    if how == "binding":
        binding.index_append(db, files or None, out_prefix=out, decon=[iau.fasta("c")] if decon else None)
        return
    args = [iau.INDEX, "-t_db", db] + (["-i"] + files if files else []) + (["-o", out] if out else []) + line + (["-deCon", iau.fasta("c")] if decon else [])
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert p.returncode == 0 and p.stdout == b"", (args, p.returncode, p.stderr)


@pytest.mark.parametrize("how", ["binding", "cli"])
@pytest.mark.parametrize("case", list(iau.CASES))
def test_recorded_case(case, how, ref, fresh, built, tmp):
    d = iau.CASES[case]
    work = tmp / ("%s_%s" % (case, how))
    os.makedirs(work)
    cur = str(work / "db")
    for e in EXTS:
        shutil.copy(ref[d["old"]] + e, cur + e)
    for si, parts in enumerate(d["steps"]):
        out = None if d.get("inplace") else str(work / ("out%d" % si))
        before = snapshot(cur)
        append(how, cur, parts, out, bool(d.get("decon")) and si == len(d["steps"]) - 1, d["line"])
        if out:
            assert snapshot(cur) == before          # with an output prefix of its own the old index is not touched
            cur = out
        elif not parts:
            assert snapshot(cur) == before          # decon onto the index: the four files are left alone
    assert not [f for f in os.listdir(work) if "appending" in f]          # no temporary file is left
    want = ref[d["want"]]
    with_b = any(d["steps"])
    ours = fresh(d["old"], with_b=with_b, decon=bool(d.get("decon")))
    iau.same_index(cur, want)
    if with_b:
        iau.files_equal(cur, ours)          # byte for byte our own fresh build of a + b
        assert iau.Comp(cur + ".comp.b").DB_size == iau.Comp(ref[d["old"]] + ".comp.b").DB_size + 11
    if d.get("decon"):
        iau.same_comp(cur + ".decon.comp.b", ref[d["want_decon"] + ".decon"])
        iau.files_equal(cur, ours, exts=(".decon.comp.b",))
    stems = {f.split(".")[0] for f in os.listdir(work)}
    files = sorted(f for f in os.listdir(work) if f.startswith(os.path.basename(cur) + "."))
    assert files == sorted(os.path.basename(cur) + e for e in EXTS + ((".decon.comp.b",) if d.get("decon") else ())), files
    assert stems == {"db"} | {"out%d" % i for i in range(len(d["steps"])) if not d.get("inplace")}


def test_an_index_we_built_is_appended_like_the_reference_s(ref, fresh, tmp):
    """the old index from our builder, hashed where the reference's is direct-address too: the same bytes out"""
    for old in ("A_k16", "A_TG", "A_k10"):
        mine = fresh(old, with_b=False)
        out = str(tmp / ("ours_" + old))
        before = snapshot(mine)
        binding.index_append(mine, iau.fasta("b"), out_prefix=out)
        assert snapshot(mine) == before
        iau.files_equal(out, fresh(old))
        iau.same_index(out, ref[iau.CASES[{"A_k16": "k16", "A_TG": "TG_without_the_option", "A_k10": "direct_address"}[old]]["want"]])


def test_a_failed_append_leaves_the_old_index_whole(ref, tmp):
    work = tmp / "failed"
    os.makedirs(work)
    cur = str(work / "db")
    for e in EXTS:
        shutil.copy(ref["A_k16"] + e, cur + e)
    before = snapshot(cur)
    bad = str(work / "short.fsa")
    with open(bad, "w") as f:
        f.write(">too short\nACGTACGT\n")
    with pytest.raises(binding.KmaHipError, match="no template of at least 16 bases"):
        binding.index_append(cur, bad)
    with pytest.raises(binding.KmaHipError, match="cannot open"):
        binding.index_append(cur, str(work / "missing.fsa"))
    assert snapshot(cur) == before and sorted(os.listdir(work)) == sorted(["short.fsa"] + ["db" + e for e in EXTS])


# ---- the width of the value lists ------------------------------------------------------------------------------------------------
def same_big(a, b):
    """same_index on arrays: a mapping of 1.6 M k-mers as two Python dicts takes seconds, as sorted pairs it does not"""
    for ext in (".length.b", ".name"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    A, B = iau.Comp(a + ".comp.b"), iau.Comp(b + ".comp.b")
    assert A.header() == B.header() and A.v_index == B.v_index and A.values.dtype == B.values.dtype
    assert np.array_equal(iau.expand(A), iau.expand(B))
    return A


def test_crossing_from_16_to_32_bit_lists(tmp):
    """65 530 templates of 40 bases (DB_size 65 531: 16-bit lists) plus 10 (65 541: 32-bit lists)"""
    rng = np.random.default_rng(65530)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (65540, 40))]
    work = tmp / "cross"
    os.makedirs(work)
    fa, fb = str(work / "a.fsa"), str(work / "b.fsa")
    for path, lo, hi in ((fa, 0, 65530), (fb, 65530, 65540)):
        with open(path, "wb") as f:
            f.write(b"".join(b">t%d\n%s\n" % (i, rows[i].tobytes()) for i in range(lo, hi)))
    old, full, got = (str(work / n) for n in ("old", "full", "got"))
    binding.index_build(fa, old)
    binding.index_build([fa, fb], full)
    binding.index_append(old, fb, out_prefix=got)
    iau.files_equal(got, full)
    a, b = iau.Comp(old + ".comp.b"), iau.Comp(got + ".comp.b")
    assert (a.DB_size, a.values.dtype, b.DB_size, b.values.dtype) == (65531, np.uint16, 65541, np.uint32)
    if os.path.exists(iau.KMA):          # the reference's own append, run live: about a second a run
        r_old, r_got, mine = (str(work / n) for n in ("r_old", "r_got", "mine"))
        for args in (["-i", fa, "-o", r_old], ["-t_db", r_old, "-i", fb, "-o", r_got]):
            subprocess.run([iau.KMA, "index"] + args, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
        binding.index_append(r_old, fb, out_prefix=mine)
        iau.files_equal(mine, full)
        c = same_big(mine, r_got)
        assert c.DB_size == 65541 and c.n > 1_600_000


# ---- the index in use -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads(tmp):
    """2 000 reads of 50 ... 120 bases off the templates of a + b, a substitution in a hundred, half of them reverse-complemented"""
    rng = np.random.default_rng(2000)
    seqs = [np.array(["ACGTN".index(ch) for ch in seq], np.uint8) for part in ("a", "b") for _, seq, _ in siu.read_fasta(iau.fasta(part)) if len(seq) >= 50]
    out = []
    for _ in range(2000):
        s = seqs[int(rng.integers(0, len(seqs)))]
        L = min(len(s), int(rng.integers(50, 121)))
        at = int(rng.integers(0, len(s) - L + 1))
        r = s[at:at + L].copy()
        x = (rng.random(L) < 0.01) & (r < 4)
        r[x] = (r[x] + rng.integers(1, 4, int(x.sum()), dtype=np.uint8)) & 3
        out.append(synth.revcomp_codes(r) if rng.random() < 0.5 else r)
    fq = str(tmp / "reads.fq")
    synth.write_fastq(fq, out)
    return fq


def run_map(program, fq, prefix, stem, extra):
    args = [program, "-i", fq, "-o", stem, "-t_db", prefix] + extra + (["-t", "1"] if program == iau.KMA else [])
    p = subprocess.run(args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=TIMEOUT)
    # (the reference ORs errno into its exit status, kma.c:1630)
    assert p.returncode in ((0, 2) if program == iau.KMA else (0,)), (args, p.returncode, p.stderr)
    return stem


def mapped(stem):
    return open(stem + ".res", "rb").read(), gzip.open(stem + ".frag.gz", "rb").read()


def test_mapping_against_our_appended_index(reads, ref, built, tmp):
    mine = str(tmp / "use_k16")
    binding.index_append(ref["A_k16"], iau.fasta("b"), out_prefix=mine)
    a = mapped(run_map(iau.MAP, reads, mine, str(tmp / "map_mine"), ["-1t1"]))
    b = mapped(run_map(iau.MAP, reads, ref["k16"], str(tmp / "map_ref"), ["-1t1"]))
    assert a == b and a[1].count(b"\n") > 1500 and b"\nb_" in a[0]
    if os.path.exists(iau.KMA):
        assert mapped(run_map(iau.KMA, reads, mine, str(tmp / "kma_mine"), ["-1t1"])) == a


def test_sparse_mapping_against_our_appended_index(reads, ref, built, tmp):
    mine = str(tmp / "use_TG")
    binding.index_append(ref["A_TG"], iau.fasta("b"), out_prefix=mine)
    spa = lambda stem: open(stem + ".spa").read()
    a = spa(run_map(iau.MAP, reads, mine, str(tmp / "spa_mine"), ["-Sparse"]))
    assert a == spa(run_map(iau.MAP, reads, ref["TG"], str(tmp / "spa_ref"), ["-Sparse"])) and a.count("\n") > 10 and "\nb_" in a
    if os.path.exists(iau.KMA):
        assert spa(run_map(iau.KMA, reads, mine, str(tmp / "spa_kma"), ["-Sparse"])) == a


def test_decontaminated_mapping_against_our_appended_index(reads, ref, built, tmp):
    mine, theirs = str(tmp / "use_decon"), str(tmp / "ref_decon")
    binding.index_append(ref["A_k16"], iau.fasta("b"), out_prefix=mine, decon=iau.fasta("c"))
    for e in EXTS:
        shutil.copy(ref["k16"] + e, theirs + e)
    shutil.copy(ref["append_decon.decon"], theirs + ".decon.comp.b")
    a = mapped(run_map(iau.MAP, reads, mine, str(tmp / "dec_mine"), ["-1t1", "-deCon"]))
    assert a == mapped(run_map(iau.MAP, reads, theirs, str(tmp / "dec_ref"), ["-1t1", "-deCon"])) and a[1].count(b"\n") > 1500
