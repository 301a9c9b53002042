"""The host's part of `<out>.vcf.gz`: kmahip_vcf_header and kmahip_vcf_line on records written by hand, against the rows the reference
printed for the hand set V of test_matvcf_gpu.py (tests/golden/matvcf_v, recorded from oracle/_ref/kma -1t1 -matrix -vcf). No GPU."""
import math
import os

from kma_amd import binding

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matvcf_v")
line = binding.KmaHipDB.vcf_line

# (pos, ref, call, bestScore, counts A C G T N -) of the seven rows of set V that carry an ALT, in the file's order
V_RECORDS = [
    (51, "G", "T", 20, (0, 0, 0, 20, 0, 0)),          # every read substitutes position 50
    (81, "C", "C", 20, (0, 20, 0, 0, 0, 0)),          # a matching column, printed because a kept insertion column follows
    (0, "-", "g", 14, (0, 0, 14, 0, 0, 6)),           # the two insertion columns of reads 0-13
    (0, "-", "t", 14, (0, 0, 0, 14, 0, 6)),
    (111, "G", "-", 20, (0, 0, 0, 0, 0, 20)),         # every read deletes position 110
    (141, "A", "a", 12, (12, 0, 8, 0, 0, 0)),         # reads 0-7 substitute position 140: not significant
    (171, "A", "a", 3, (3, 0, 0, 0, 0, 0)),           # three reads reach position 170
]
V_LITERAL = [
    b"hand1\t51\t.\tG\tT\t120\t.\tDP=20;AD=20;AF=1.00;RAF=1.00;DEL=0;AD6=0,0,0,20,0,0\tQ:P:FT\t20.00:7.7e-06:PASS\n",
    b"hand1\t81\t.\tC\tC\t120\t.\tDP=20;AD=20;AF=1.00;RAF=1.00;DEL=0;AD6=0,20,0,0,0,0\tQ:P:FT\t20.00:7.7e-06:PASS\n",
    b"hand1\t0\t.\t<->\tg\t45\t.\tDP=20;AD=14;AF=0.70;RAF=0.70;DEL=6;AD6=0,0,14,0,0,6\tQ:P:FT\t3.20:7.4e-02:LowQual\n",
    b"hand1\t0\t.\t<->\tt\t45\t.\tDP=20;AD=14;AF=0.70;RAF=0.70;DEL=6;AD6=0,0,0,14,0,6\tQ:P:FT\t3.20:7.4e-02:LowQual\n",
    b"hand1\t111\t.\tG\t<->\t120\t.\tDP=20;AD=20;AF=1.00;RAF=1.00;DEL=20;AD6=0,0,0,0,0,20\tQ:P:FT\t20.00:7.7e-06:PASS\n",
    b"hand1\t141\t.\tA\ta\t31\t.\tDP=20;AD=12;AF=0.60;RAF=0.60;DEL=0;AD6=12,0,8,0,0,0\tQ:P:FT\t0.80:3.7e-01:LowQual\n",
    b"hand1\t171\t.\tA\ta\t18\t.\tDP=3;AD=3;AF=1.00;RAF=1.00;DEL=0;AD6=3,0,0,0,0,0\tQ:P:FT\t3.00:8.3e-02:LowQual\n",
]


def test_rows_of_the_hand_set():
    got = [line("hand1", r) for r in V_RECORDS]
    assert got == V_LITERAL
    recorded = open(os.path.join(GOLDEN, "alt_rows.txt"), "rb").read()
    assert b"".join(got) == recorded
    vcf = open(os.path.join(GOLDEN, "ref.vcf"), "rb").read()
    assert all(x in vcf for x in got)


def test_header():
    vcf = open(os.path.join(GOLDEN, "ref.vcf"), "rb").read()
    head = b"".join(x + b"\n" for x in vcf.split(b"\n") if x.startswith(b"#"))
    assert binding.KmaHipDB.vcf_header("/some/folder/db") == head
    assert binding.KmaHipDB.vcf_header("db") == head
    assert head.count(b"\n") == 13 and b"##kmaVersion=1.5.1\n" in head and head.endswith(b"\tFORMAT\tdb\n")


def test_zero_row():
    """a template position nothing was piled on (vcf.c:261-275); the FILTER column is filled under -vcf 2"""
    vcf = open(os.path.join(GOLDEN, "ref.vcf"), "rb").read()
    zero = (1, "C", ".", 0, (0,) * 6)
    want = b"hand1\t1\t.\tC\t.\t0\t.\tDP=0;AD=0;AF=0.00;RAF=0.00;DEL=0;AD6=0,0,0,0,0,0\tQ:P:FT\t0.00:1.0e+00:FAIL\n"
    assert line("hand1", zero) == want and want in vcf
    assert line("hand1", zero, filter=2) == want.replace(b"\t0\t.\tDP", b"\t0\tFAIL\tDP")


def _qual(n, k):
    # binP(n, k, 0.25) at its two closed ends (stdstat.c:170-176), -10 / ln 10 times its logarithm, cut to an int
    p = 0.75 ** n if k == 0 else 0.25 ** n
    return int(-10 / math.log(10) * math.log(p))


def test_qual_at_the_ends():
    """AD == DP: binP is 0.25^DP; AD == 0 (a call of N over bases only: 'n' counts the N column): 0.75^DP"""
    full = line("t", (7, "A", "A", 40, (40, 0, 0, 0, 0, 0)), bcd=50)          # (printed for DP < bcd)
    assert full.split(b"\t")[5] == str(_qual(40, 40)).encode() == b"240"
    none = line("t", (7, "A", "n", 22, (20, 20, 0, 0, 0, 0)))
    f = none.split(b"\t")
    assert f[5] == str(_qual(40, 0)).encode() == b"49" and f[7].startswith(b"DP=40;AD=0;AF=0.00;RAF=0.55;")
    # between the ends: 20 of 40 at p = 0.25, the product form (stdstat.c:181-199)
    mid = line("t", (7, "A", "c", 20, (20, 20, 0, 0, 0, 0)))
    want = math.comb(40, 20) * 0.25 ** 20 * 0.75 ** 20
    assert abs(int(mid.split(b"\t")[5]) - (-10 * math.log10(want))) < 1


def test_qual_cap():
    """values above 3079 become 3079: 0.25^520 is a subnormal (3130), 0.25^6000 is 0 and binP gives its floor 1e-308 (3080); 0.25^500 stays"""
    for depth in (520, 6000):
        deep = line("t", (9, "C", "C", depth, (0, depth, 0, 0, 0, 0)), bcd=10000)
        assert deep.split(b"\t")[5] == b"3079"
    assert _qual(500, 500) == 3010
    below = line("t", (9, "C", "C", 500, (0, 500, 0, 0, 0, 0)), bcd=10000)
    assert below.split(b"\t")[5] == b"3010"


def test_filter_levels():
    """PASS / LowQual / FAIL (vcf.c:202-208), in the FILTER column only under -vcf 2; FT always"""
    rec = (141, "A", "a", 12, (12, 0, 8, 0, 0, 0))          # P = 0.37: not significant at 0.05
    for kw, ft in ((dict(bcd=1, support=0.0), b"LowQual"), (dict(bcd=30, support=0.7), b"FAIL"), (dict(bcd=1, support=0.0, evalue=0.5), b"PASS")):
        one, two = line("hand1", rec, filter=1, **kw), line("hand1", rec, filter=2, **kw)
        assert one.split(b"\t")[6] == b"." and two.split(b"\t")[6] == ft
        assert one.endswith(b":" + ft + b"\n") and two.endswith(b":" + ft + b"\n")
        assert one.replace(b"\t31\t.\t", b"\t31\t" + ft + b"\t") == two


def test_small_cap_gives_nothing():
    rec = V_RECORDS[0]
    full = line("hand1", rec)
    assert line("hand1", rec, cap=len(full)) == b""          # (no room for the NUL)
    assert line("hand1", rec, cap=len(full) + 1) == full
    assert line("hand1", (1, "C", ".", 0, (0,) * 6), cap=10) == b""
    buf_small = binding.C.create_string_buffer(16)
    assert binding.lib().kmahip_vcf_header(b"db", buf_small, 16) == 0
