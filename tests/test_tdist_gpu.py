"""Template distances on the device (kma_amd.binding.TemplateDist, examples/kmahip_dist) against the plain Python restatement
(tests/dist_util.py) and the reference's recorded files (tests/golden/tdist/).

The cell test. `tdist_cells` is held to Python's %-formatting of the same double expression (correctly rounded, as glibc's printf):
every (Ni, Nj, D) with Ni, Nj <= 48 and D <= min(Ni, Nj); N = 2^k and 2^k +- 1 up to 2^30 with D = odd * 2^j, which makes the 7th or
9th decimal an exact tie wherever a power of two divides (5 / 512 among them; the test counts the ties it holds); 4 000 seeded large
triples; all ten double measures and the three integer ones. Left out: the triples a measure divides by zero on (write() refuses
those by name) and pairs with Ni + Nj >= 2^31, where the reference's int sum overflows (undefined there, beyond int32 counts here)."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dist_util as du
from kma_amd import binding

pytestmark = pytest.mark.gpu
TIMEOUT = 120
RUNS = [(case, tag) for case, (_, _, runs) in du.CASES.items() for tag in runs]
FORMS = ("rows", "pairs")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tdist_gpu")


@pytest.fixture(scope="module")
def built():
    binding.lib()          # (the program links against the library)
    subprocess.check_call(["make", "-C", os.path.join(du.ROOT, "examples"), "kmahip_dist"], stdout=subprocess.DEVNULL)


def _same_counts(td, N, D):
    gN, gD = td.counts()
    assert gN.dtype == gD.dtype == np.int32
    assert np.array_equal(gN, N) and np.array_equal(gD, du.tri(D))


# ---- counting -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(du.CASES))
def test_counts_equal_the_restatement(case, form, tmp, monkeypatch):
    v, N, D = du.restated(case, tmp)
    monkeypatch.setenv("KMAHIP_TDIST_FORM", form)
    with binding.TemplateDist(du.unpack_index(case, tmp)) as td:
        assert (td.info.DB_size, td.info.n_kmers, td.info.n_lists, td.info.direct) == (v.DB_size, v.n, len(v.lists()), int(v.mega))
        assert (td.info.mlen, td.info.prefix_len, td.info.flag, td.info.kmersize) == (v.mlen, v.prefix_len, v.flag, v.kmersize)
        assert td.count() == form
        _same_counts(td, N, D)
        assert [td.name(t) for t in range(td.n)] == v.names
        # a part of the triangle
        lo, hi = td.n // 3, td.n - td.n // 4
        assert np.array_equal(td.counts(lo, hi)[1], np.concatenate([D[i, :i] for i in range(lo, hi)] + [np.zeros(0, np.int64)]))


@pytest.mark.parametrize("case,cols", [("edge", 7), ("wide", 64), ("wide", 299), ("two", 1)])
def test_rows_split_into_column_blocks(case, cols, tmp, monkeypatch):
    """a row longer than what one workgroup sums in LDS is split: the same arrays at a width that cuts the fixtures' rows"""
    v, N, D = du.restated(case, tmp)
    monkeypatch.setenv("KMAHIP_TDIST_FORM", "rows")
    monkeypatch.setenv("KMAHIP_TDIST_COLS", str(cols))
    with binding.TemplateDist(du.unpack_index(case, tmp)) as td:
        td.count()
        _same_counts(td, N, D)


@pytest.mark.parametrize("form", FORMS)
def test_from_lists_16_and_32_bit_values_give_the_same_arrays(form, tmp, monkeypatch):
    v, N, D = du.restated("edge", tmp)
    off, val = v.exist.astype(np.uint32), v.values
    monkeypatch.setenv("KMAHIP_TDIST_FORM", form)
    got = []
    for vb in (2, 4):
        with binding.TemplateDist.from_lists(v.DB_size - 1, off, val, value_bytes=vb) as td:
            assert td.info.value_bytes == vb and td.info.n_lists == len(v.lists())
            td.count()
            _same_counts(td, N, D)
            got.append(td.counts())
    assert all(np.array_equal(a, b) for a, b in zip(*got))


@pytest.mark.parametrize("form", FORMS)
def test_nothing_rests_on_the_order_inside_a_list(form, tmp, monkeypatch):
    """every list of the edge fixture reversed in place: the pair is (max, min) of the two ids, the arrays stay"""
    v, N, D = du.restated("edge", tmp)
    val = v.values.astype(np.uint32).copy()
    for o in v.lists():
        m = int(val[o])
        val[o + 1:o + 1 + m] = val[o + 1:o + 1 + m][::-1].copy()
    monkeypatch.setenv("KMAHIP_TDIST_FORM", form)
    with binding.TemplateDist.from_lists(v.DB_size - 1, v.exist.astype(np.uint32), val, value_bytes=4) as td:
        td.count()
        _same_counts(td, N, D)


@pytest.mark.parametrize("n,form", [(17000, "rows"), (17000, "pairs"), (41000, "rows")])
def test_rows_wider_than_64_kib_of_lds_and_than_one_workgroup_sums(n, form, monkeypatch):
    """17 000 templates: the rows kernel asks for more dynamic LDS than a kernel gets unasked. 41 000: a workgroup sums the 40 000
    ints that are the most it takes (160 016 bytes of LDS), and the rows beyond are cut into two column blocks with nothing set to
    make them. Four lists, one of them beyond a wavefront, one used by five k-mers, one across column 40 000, and an entry equal to 1
    that is passed over. Every row that holds a count is compared cell by cell, and the last 20 rows whole."""
    rng = np.random.default_rng(5)
    lists = [([1, 5000, n - 1, n], 1), (sorted(rng.choice(np.arange(1, n + 1), 300, replace=False).tolist()), 5), ([16384, 16385, n], 2),
             ([n - 1002, n - 1001, n - 1000, n - 999, n - 3], 3)]
    if n > 40002:
        lists[3] = ([39999, 40000, 40001, 40002, n - 3], 3)
    val, off = [0, 0], []
    for ids, m in lists:
        off += [len(val)] * m
        val += [len(ids)] + ids
    off.insert(2, 1)
    want_N, want_D = np.zeros(n, np.int64), {}
    for ids, m in lists:
        for a in ids:
            want_N[a - 1] += m
        for i, a in enumerate(ids):
            for b in ids[:i]:
                want_D.setdefault(a - 1, {})
                want_D[a - 1][b - 1] = want_D[a - 1].get(b - 1, 0) + m
    monkeypatch.setenv("KMAHIP_TDIST_FORM", form)
    with binding.TemplateDist.from_lists(n, off, val, value_bytes=2) as td:
        assert td.info.n_kmers == 11 and td.info.n_lists == 4
        td.count()
        N, tail = td.counts(n - 20, n)
        assert np.array_equal(N, want_N)
        exp = np.zeros(len(tail), np.int64)
        base = (n - 20) * (n - 21) // 2
        for hi, row in want_D.items():
            for lo, c in row.items():
                if hi >= n - 20:
                    exp[hi * (hi - 1) // 2 + lo - base] = c
        assert np.array_equal(tail, exp) and exp.sum() > 0
        for hi, row in want_D.items():
            want = np.zeros(hi, np.int64)
            want[list(row)] = list(row.values())
            assert np.array_equal(td.counts(hi, hi + 1)[1], want), hi
        assert max(want_D) == n - 1 and any(lo >= 40000 for row in want_D.values() for lo in row) == (n > 40002)


# ---- the file -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counted(tmp):
    """a counted TemplateDist per case, opened once"""
    held = {}

    def get(case):
        if case not in held:
            td = binding.TemplateDist(du.unpack_index(case, tmp))
            td.count()
            held[case] = td
        return held[case]
    yield get
    for td in held.values():
        td.close()


@pytest.mark.parametrize("case,tag", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_write_equals_the_recorded_file(case, tag, counted, tmp):
    methods, fmt = du.run_flags(du.CASES[case][2][tag])
    out = str(tmp / ("w_%s_%s.phy" % (case, tag)))
    counted(case).write(out, methods, fmt)
    assert open(out, "rb").read() == du.golden(case, tag)


@pytest.mark.parametrize("case,tag,chunk", [("edge", "d8191_f5", 256), ("edge", "d3_f0", 256), ("edge", "d12_f4", 1000), ("wide", "d3", 256), ("wide", "d3", 4096),
                                            ("two", "d8191_f5", 256)])
def test_write_in_chunks_that_cut_rows(case, tag, chunk, counted, tmp, monkeypatch):
    """a chunk far smaller than a row of the matrix (72 cells are 792 bytes): windows begin and end inside names and cells"""
    methods, fmt = du.run_flags(du.CASES[case][2][tag])
    monkeypatch.setenv("KMAHIP_TDIST_CHUNK", str(chunk))
    out = str(tmp / ("c_%s_%s_%d.phy" % (case, tag, chunk)))
    counted(case).write(out, methods, fmt)
    assert open(out, "rb").read() == du.golden(case, tag)


def test_write_from_lists_names_the_templates_by_their_ids(tmp):
    v, N, D = du.restated("two", tmp)
    with binding.TemplateDist.from_lists(2, v.exist.astype(np.uint32), v.values) as td:
        td.count()
        out = str(tmp / "ids.phy")
        td.write(out, 8191, 4)
        assert open(out, "rb").read() == du.phy(N, D, [b"1", b"2"], 8191, 4)


def test_division_by_zero_is_refused_by_name(tmp):
    """template 2 of 4 is in no list, then templates 2 and 4: N = 0"""
    out = str(tmp / "zero.phy")
    with binding.TemplateDist.from_lists(4, [2, 2, 6], [0, 0, 3, 1, 3, 4, 2, 1, 3]) as td:
        td.count()
        N, D = td.counts()
        assert N.tolist() == [3, 0, 3, 2] and D.tolist() == [0, 3, 0, 2, 0, 2]
        for m in (4, 8, 256, 512, 1024, 2048, 8191, 4 | 1):
            with pytest.raises(binding.KmaHipError) as e:
                td.write(out, m, 1)
            assert "kmahip error -1" in str(e.value) and "divides by zero" in str(e.value) and "template 2 (2)" in str(e.value), str(e.value)
        served = 1 | 2 | 16 | 32 | 64 | 128 | 4096          # (one empty template: every sum of two is above zero)
        td.write(out, served, 5)
        Dm = np.zeros((4, 4), np.int64)
        Dm[np.tril_indices(4, -1)] = D
        assert open(out, "rb").read() == du.phy(N.astype(np.int64), Dm, [b"1", b"2", b"3", b"4"], served, 5)
    with binding.TemplateDist.from_lists(4, [2, 2], [0, 0, 2, 1, 3]) as td:
        td.count()
        for m in (16, 32, 64, 128, 4096, 64 | 1):
            with pytest.raises(binding.KmaHipError) as e:
                td.write(out, m, 1)
            assert "divides by zero" in str(e.value) and "templates 2 (2) and 4 (4)" in str(e.value), str(e.value)
        td.write(out, 3, 1)          # methods 1 and 2 are always served
        assert len(open(out, "rb").read()) == du.phy_size(5, 8, 3, 1)


# ---- the program --------------------------------------------------------------------------------------------------------------
CLI_RUNS = [("edge", "d8191_f5", []), ("edge", "d3_f0", ["-t", "4"]), ("edge", "default", []), ("wide", "d3", ["-t", "4"]), ("one", "d8191_f5", []),
            ("two", "default", []), ("edge_k20", "d8191_f5", []), ("edge_TG", "d8191_f5", ["-t", "4"]), ("edge_m12", "d8191_f5", []), ("edge_mega", "d8191_f5", [])]


@pytest.mark.parametrize("case,tag,more", CLI_RUNS, ids=["%s-%s" % r[:2] for r in CLI_RUNS])
def test_kmahip_dist_equals_the_recorded_file_and_the_reference_binary(case, tag, more, built, tmp):
    db = du.unpack_index(case, tmp)
    args = du.CASES[case][2][tag] + more
    out = str(tmp / ("p_%s_%s.phy" % (case, tag)))
    p = subprocess.run([du.DIST, "-t_db", db, "-o", out] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b""), p.stderr
    got = open(out, "rb").read()
    assert got == du.golden(case, tag)
    if os.path.exists(du.KMA):
        ref = out + ".ref"
        subprocess.run([du.KMA, "dist", "-t_db", db, "-o", ref] + args, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=TIMEOUT)
        assert open(ref, "rb").read() == got


def test_kmahip_dist_default_output_and_wrong_format(built, tmp_path):
    db = du.unpack_index("two", tmp_path)
    p = subprocess.run([du.DIST, "-t_db", db], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert p.returncode == 0 and open(db + ".phy", "rb").read() == du.golden("two", "default")
    with open(db + ".comp.b", "r+b") as f:
        f.truncate(60)
    p = subprocess.run([du.DIST, "-t_db", db, "-o", str(tmp_path / "o.phy")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT)
    assert p.returncode == 1 and p.stderr.startswith(b"Wrong format of DB.\n"), p.stderr


# ---- the cells ----------------------------------------------------------------------------------------------------------------
def _triples():
    small = [(a, b, d) for a in range(49) for b in range(49) for d in range(min(a, b) + 1)]
    pw = []
    odd = (1, 3, 5, 7, 125, 511)
    for k in range(1, 31):
        for a in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            for b in {a, 2 ** k, 2 ** (k - 1) + 1, 3, 2 ** 30 - 3, 2 ** 30 + 1}:
                if a + b >= 2 ** 31:
                    continue
                top = min(a, b)
                ds = {0, 1, top, top - 1} | {o << j for o in odd for j in range(0, k + 1)}
                pw += [(a, b, d) for d in sorted(ds) if 0 <= d <= top]
    rng = np.random.default_rng(20200103)
    big = []
    for _ in range(4000):
        a, b = (int(x) for x in rng.integers(1, 2 ** 30, 2))
        big.append((a, b, int(rng.integers(0, min(a, b) + 1))))
    return small, pw, big


def _divides_by_zero(method, a, b, d):
    if method in (4, 256, 512, 1024, 2048) and a == 0:
        return True
    if method in (8, 256, 512, 1024, 2048) and b == 0:
        return True
    if method in (16, 32, 4096) and a + b == 0:
        return True
    return method in (64, 128) and a + b - d == 0


@pytest.fixture(scope="module")
def triples():
    return _triples()


@pytest.mark.parametrize("method", list(du.METHODS))
def test_cells_equal_python_formatting_of_the_same_expression(method, triples):
    small, pw, big = triples
    t = [x for x in small + pw + big if not _divides_by_zero(method, *x)]
    a, b, d = (np.array(c, np.int64) for c in zip(*t))
    got = binding.tdist_cells(method, a, b, d)
    want = [du.cell(method, *x) for x in t]
    bad = [(x, g, w) for x, g, w in zip(t, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    kind = du.METHODS[method][1]
    if kind != "i":
        # the exact ties the set holds: value * 10^p is an integer and a half
        p = 10 ** (6 if kind == "f6" else 8)
        ties = sum(1 for x in pw if not _divides_by_zero(method, *x) and (Fraction(du.value(method, *x)) * p).denominator == 2)
        assert ties > 0, ties
        if method == 1024:
            assert (Fraction(du.value(1024, 512, 512, 5)) * p).denominator == 2 and (512, 512, 5) in pw          # 5 / 512


def test_cells_round_half_to_even_on_exact_ties():
    """5 / 512 = 0.009765625 and 3 / 512 = 0.005859375: the ninth decimal is a tie, the eighth even and odd"""
    assert binding.tdist_cells(1024, [512, 512], [512, 512], [5, 3]) == [b"\t0.00976562", b"\t0.00585938"]
    assert binding.tdist_cells(4, [512, 2048], [1, 1], [5, 1]) == [b"\t  0.976562", b"\t  0.048828"]
