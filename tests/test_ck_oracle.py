"""The Python restatement of the counting template finder (tests/ck_util.py: save_kmers_count, savekmers.c:3067-3365) held to the
reference's `-s2` taps of `-ck` (tests/golden/ck, make_golden_ck.py): every record of every single-end tap, the hand-made edge set
and its cases.tsv, and the literal forward-N-list rule of the reverse strand's walk against the "corrected" one; and the restated
pairing (save_kmers_penaltyPair, save_kmers_unionPair over get_kmers_for_pair_count) held to the five paired taps byte for byte or
record for record, with the forward-N-list rule as the foil there: pairs do not have it. No GPU."""
import gzip
import os

import numpy as np
import pytest

import ck_util
import golden_util
from kma_amd import formats

CK = os.path.join(golden_util.GOLD, "ck")
K = 16


def tap(name):
    with gzip.open(os.path.join(CK, name), "rb") as f:
        recs, _ = formats.parse_s2(f.read())
    out = {r["hdr"]: (int(r["rc_flag"]), int(r["flag"]), [int(t) for t in r["T"]]) for r in recs}
    assert len(out) == len(recs), "duplicate headers"
    return out


@pytest.fixture(scope="module")
def se():
    """tests/golden/se: its reads as stage 1 hands them on, and the k-mer dictionary of its FASTA"""
    with gzip.open(os.path.join(golden_util.GOLD, "se", "s1.bin.gz"), "rb") as f:
        s1 = formats.parse_s1(f.read())
    _, seqs = ck_util.read_fasta(os.path.join(golden_util.GOLD, "se", "db.fsa.gz"))
    return dict(hdr=[r["hdr"] for r in s1], reads=golden_util.reads_from_s1(s1), d=ck_util.kmer_dict(seqs, K))


@pytest.fixture(scope="module")
def edge():
    _, seqs = ck_util.read_fasta(os.path.join(CK, "edge.fsa.gz"))
    names, reads = ck_util.read_fastq(os.path.join(CK, "edge.fq.gz"))
    with open(os.path.join(CK, "cases.tsv")) as f:
        head = f.readline().rstrip("\n").split("\t")
        cases = [dict(zip(head, line.rstrip("\n").split("\t"))) for line in f]
    return dict(names=names, reads=reads, d=ck_util.kmer_dict(seqs, K), cases=cases)


def restated(d, hdr, reads, **kw):
    out = {}
    for h, r in zip(hdr, reads):
        res = ck_util.save_kmers_count(d, K, r, **kw)
        if res is not None:
            out[h] = res
    return out


@pytest.mark.parametrize("name,kw", [("s2_ck.bin.gz", {}), ("s2_ck_ex.bin.gz", dict(exhaustive=True)), ("s2_ck_p07.bin.gz", dict(min_frac=0.7))],
                         ids=["ck", "ck_ex_mode", "ck_proxi07"])
def test_restatement_matches_every_record_of_the_single_end_taps(se, name, kw):
    want = tap(name)
    assert len(want) > 900
    assert restated(se["d"], se["hdr"], se["reads"], **kw) == want


def test_counting_moves_the_tap(se):
    """the fixture is worth having: `-ck` keeps fewer records than the plain run and changes every rc_flag"""
    plain, _ = formats.parse_s2(gzip.open(os.path.join(golden_util.GOLD, "se", "s2.bin.gz"), "rb").read())
    plain = {r["hdr"]: int(r["rc_flag"]) for r in plain}
    ck = tap("s2_ck.bin.gz")
    assert len(ck) == 912 and len(plain) == 1178 and set(ck) <= set(plain)
    assert all(ck[h][0] != plain[h] for h in ck)
    longer = tap("s2_ck_p07.bin.gz")
    assert sum(len(longer[h][2]) > len(ck[h][2]) for h in ck) > 50


def test_mirrored_n_rule_fails_on_the_single_end_fixture(se):
    """the foil: with the reverse strand's walk bounded by its own, mirrored N list the restatement gets reads with N's wrong, and
    only those"""
    want = tap("s2_ck.bin.gz")
    wrong = [h for h, r in zip(se["hdr"], se["reads"]) if ck_util.save_kmers_count(se["d"], K, r, mirrored=True) != want.get(h)]
    assert len(wrong) >= 1
    has_n = {h for h, r in zip(se["hdr"], se["reads"]) if (np.asarray(r) > 3).any()}
    assert set(wrong) <= has_n


@pytest.mark.parametrize("name,ex", [("s2_edge.bin.gz", False), ("s2_edge_ex.bin.gz", True)], ids=["ck", "ck_ex_mode"])
def test_restatement_matches_the_edge_taps(edge, name, ex):
    want = {h.rstrip(b"\0").split()[0].decode(): v for h, v in tap(name).items()}
    assert restated(edge["d"], edge["names"], edge["reads"], exhaustive=ex) == want


def test_cases_tsv_matches_the_restatement(edge):
    assert [c["name"] for c in edge["cases"]] == edge["names"]
    for c, r in zip(edge["cases"], edge["reads"]):
        for pre, ex in (("", False), ("ex_", True)):
            res = ck_util.save_kmers_count(edge["d"], K, r, exhaustive=ex)
            want = None if c[pre + "rc_flag"] == "0" else (int(c[pre + "rc_flag"]), int(c[pre + "flag"]), [int(t) for t in c[pre + "T"].split(",")])
            assert res == want, (c["name"], pre, res, want)


def test_edge_cases_are_the_intended_ones(edge):
    by = {c["name"]: c for c in edge["cases"]}
    assert by["exact30"]["rc_flag"] == "0" and by["exact31"]["rc_flag"] == "16"
    assert by["len15"]["rc_flag"] == by["len16"]["rc_flag"] == "0"
    assert by["offstride"]["rc_flag"] == "0" and by["offstride"]["ex_rc_flag"] == "30"
    assert by["tandem"]["rc_flag"] == "65"                       # 80 bases, 65 starts: the unit's 25 k-mers twice, the junction's 15
    assert by["tie"]["rc_flag"] == "-45" and by["tie"]["T"] == "3,-3"
    assert [len(by["fam%d" % n]["T"].split(",")) for n in (14, 15, 62, 63, 80)] == [14, 15, 62, 63, 80]
    assert by["n_rev"]["flag"] == by["n_ends_rev"]["flag"] == by["n_close_rev"]["flag"] == by["n_rule"]["flag"] == "16"


def test_mirrored_n_rule_fails_on_the_edge_set(edge):
    """n_rule: the forward-N-list rule loses the k-mers over rule_q's one substitution and ties the two templates; the mirrored rule
    counts them and keeps rule_p alone"""
    r = dict(zip(edge["names"], edge["reads"]))["n_rule"]
    assert ck_util.save_kmers_count(edge["d"], K, r)[2] == [4, 5]
    assert ck_util.save_kmers_count(edge["d"], K, r, mirrored=True)[2] == [4]
    wrong = [n for n, r in zip(edge["names"], edge["reads"])
             if ck_util.save_kmers_count(edge["d"], K, r, mirrored=True) != ck_util.save_kmers_count(edge["d"], K, r)]
    assert "n_rule" in wrong and all(n.startswith("n_") for n in wrong)


def test_pair_candidates_use_each_strands_own_n_list(edge):
    """get_kmers_for_pair_count walks the reverse strand between its own N positions (comp_rc in place): on a reverse-best read with
    an N it counts what the mirrored rule counts"""
    r = dict(zip(edge["names"], edge["reads"]))["n_rev"]
    most, fw, rv = ck_util.get_kmers_for_pair_count(edge["d"], K, r)
    assert fw == [] and rv == [(1, 69)] and most == 69
    assert ck_util.save_kmers_count(edge["d"], K, r, mirrored=True) == (69, 16, [1])
    assert ck_util.save_kmers_count(edge["d"], K, r)[0] < 69


# ---- pairs -----------------------------------------------------------------------------------------------------------------------------------
def _codes(r):
    c = formats.unpack_words(r["seq"], r["seqlen"]).copy()
    if len(r["N"]):
        c[r["N"]] = 4
    return c


@pytest.fixture(scope="module")
def pe_dict():
    return ck_util.kmer_dict(ck_util.read_fasta(os.path.join(golden_util.GOLD, "pe", "db.fsa.gz"))[1], K)


def _pe_stream(g, d, union, forward_list=False, chain_db=None):
    """the S2 stream of the paired fixture from the restatement: couples and unmated records by the restated pairing; a record stage 1
    filed singly through save_kmers_count (-1t1) or, chain_db given, through the chain finder's oracle, which does not read the option"""
    import struct

    import oracle
    out = b""
    for u in g["units"]:
        if u[0] == "se":
            r = g["s1"][u[1]]
            if chain_db is None:
                res = ck_util.save_kmers_count(d, K, _codes(r))
                if res is not None:
                    words, N = oracle.rc_packed(r["seq"], r["seqlen"], r["N"]) if res[1] & 16 else (r["seq"], r["N"])
                    out += golden_util.s2_record_bytes(r["seqlen"], words, N, res[0], res[2], r["hdr"], res[1])
            else:
                for rc_flag, emit_rc, q_start, q_end, T in chain_db.scan_chain(formats.pack_ragged([_codes(r)]))[0]:
                    words, N = oracle.rc_packed(r["seq"], r["seqlen"], r["N"]) if emit_rc else (r["seq"], r["N"])
                    out += golden_util.s2_record_bytes(r["seqlen"], words, N, rc_flag, T, r["hdr"] + b"\x00" + struct.pack("<2i", q_start, q_end), 0)
        else:
            a, b = g["s1"][u[1]], g["s1"][u[2]]
            for rec in ck_util.scan_pair(d, K, _codes(a), _codes(b), union=union, forward_list=forward_list):
                r = (a, b)[rec["mate"]]
                words, N = oracle.rc_packed(r["seq"], r["seqlen"], r["N"]) if rec["rc"] else (r["seq"], r["N"])
                out += golden_util.s2_record_bytes(r["seqlen"], words, N, int(rec["rc_flag"]), rec["T"], r["hdr"], int(rec["flag"]))
    return out + struct.pack("<i", -len(g["units"]))


def _raw(name):
    with gzip.open(os.path.join(CK, name), "rb") as f:
        return f.read()


@pytest.mark.parametrize("union,name", [(False, "s2_ck_pe_p.bin.gz"), (True, "s2_ck_pe_u.bin.gz")], ids=["apm_p", "apm_u"])
def test_restated_pairing_matches_the_paired_taps_byte_for_byte(golden_pe, pe_dict, union, name):
    want = _raw(name)
    assert _pe_stream(golden_pe, pe_dict, union) == want
    assert want != golden_pe["s2_bytes"]          # (the option moves the paired tap)


def test_restated_pairing_matches_the_default_mode_tap_byte_for_byte(golden_pe, pe_dict):
    """`kma -ipe r1 r2 -ck` without -1t1: union pairing; the records that lost their mate go through the chain finder"""
    import oracle
    assert _pe_stream(golden_pe, pe_dict, True, chain_db=oracle.OracleDB(golden_pe["prefix"])) == _raw("s2_ck_pe_default.bin.gz")


@pytest.mark.parametrize("union,name", [(False, "s2_ck_pe_p.bin.gz"), (True, "s2_ck_pe_u.bin.gz")], ids=["apm_p", "apm_u"])
def test_forward_n_list_rule_fails_on_the_paired_fixture(golden_pe, pe_dict, union, name):
    """the foil for pairs: get_kmers_for_pair_count reverse-complements in place and walks each strand between its OWN N positions;
    with save_kmers_count's forward-N-list rule the restatement gets pairs with N's wrong"""
    g = golden_pe
    assert sum(1 for u in g["units"] if u[0] == "pe" for i in u[1:] if len(g["s1"][i]["N"])) > 50
    assert _pe_stream(g, pe_dict, union, forward_list=True) != _raw(name)
    for u in g["units"]:          # (and only those: a pair without an N comes out the same under either rule)
        if u[0] == "pe" and not len(g["s1"][u[1]]["N"]) and not len(g["s1"][u[2]]["N"]):
            a, b = _codes(g["s1"][u[1]]), _codes(g["s1"][u[2]])
            x, y = ck_util.scan_pair(pe_dict, K, a, b, union=union), ck_util.scan_pair(pe_dict, K, a, b, union=union, forward_list=True)
            assert [(r["mate"], r["rc_flag"], r["flag"], r["T"].tolist()) for r in x] == [(r["mate"], r["rc_flag"], r["flag"], r["T"].tolist()) for r in y]
            break


@pytest.mark.parametrize("union,name", [(False, "s2_edge_pe_p.bin.gz"), (True, "s2_edge_pe_u.bin.gz")], ids=["apm_p", "apm_u"])
def test_restated_pairing_matches_the_edge_pair_taps(edge, union, name):
    names, m1 = ck_util.read_fastq(os.path.join(CK, "edge_r1.fq.gz"))
    _, m2 = ck_util.read_fastq(os.path.join(CK, "edge_r2.fq.gz"))
    with gzip.open(os.path.join(CK, name), "rb") as f:
        recs, _ = formats.parse_s2(f.read())
    want = [(r["hdr"].rstrip(b"\0").decode(), int(r["rc_flag"]), int(r["flag"]), r["T"].tolist(), r["seq"].tolist()) for r in recs]
    got = []
    for n, a, b in zip(names, m1, m2):
        for rec in ck_util.scan_pair(edge["d"], K, a, b, union=union):
            r = (a, b)[rec["mate"]]
            if rec["rc"]:
                r = (3 - r[::-1]).astype(np.uint8)
            got.append((n, rec["rc_flag"], rec["flag"], rec["T"].tolist(), formats.pack_ragged([r]).seq[:(len(r) + 31) // 32].tolist()))
    assert got == want and len(want) == 7
    # both sides of best1 + best2 - PE: `apart` stays two records under either pairing, `together` is a couple under the penalty only
    assert [w[:3] for w in want if w[0] == "apart"] == [("apart", 85, 97), ("apart", 85, 145)]
    assert [w[2] for w in want if w[0] == "together"] == ([99, 147] if not union else [97, 145])
    assert [w[:4] for w in want if w[0] == "lone"] == [("lone", 85, 105, [86])]
