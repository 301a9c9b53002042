"""The plain Python restatement of ConClave version 2 (tests/conclave2_util.py) against the reference's own `-ConClave 2` outputs on the
committed golden inputs (tests/golden/conclave2, make_golden_conclave2.py): fed from the committed frag_raw taps of stage 3a
(tests/golden/se|pe/out.frag_raw.gz), it must name the template of every `.frag.gz` row and the Score of every `.res` row. This is
what makes the restatement a yardstick for the device's kernels (test_conclave2_gpu.py). No GPU."""
import gzip
import os

import numpy as np
import pytest

import conclave2_util as c2
import golden_util

GOLD = os.path.join(golden_util.GOLD, "conclave2")
SEEDED = {"c400": "c", "a200": "a"}          # (make_golden_conclave2.py: reads on a database of proxi_util.INPUTS, made again from its seed)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def _tap_lines(name):
    """the `-a` text tap in stream order: (sequence as written, n, score, starts, ends, templates, header)"""
    out = []
    path = os.path.join(GOLD, name + ".frag_raw.gz") if name in SEEDED else os.path.join(golden_util.GOLD, name, "out.frag_raw.gz")
    with gzip.open(path, "rt") as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            if len(c) == 7:
                out.append((c[0], int(c[1]), int(c[2]), [int(x) for x in c[3].split(",")], [int(x) for x in c[4].split(",")],
                            [int(x) for x in c[5].split(",")], c[6]))
    return out


def _records(name, g=None):
    """the frag_raw records behind the tap in stream order: (n, signed score, q_len, q_len2, starts, ends, templates, first sequence as
    written, header). Single end: one per line."""
    if name == "pe":
        return _pe_records(g)
    return [(a[1], a[2], len(a[0]), 0, a[3][:a[1]], a[4][:a[1]], a[5][:a[1]], a[0], a[6]) for a in _tap_lines(name)]


def _pe_records(g):
    """Paired: the tap prints one line per mate (updateAllFrag, alnfrags.c:2276-2283) with the FIRST mate's arrays on both, so the second
    record of an unmated couple is not in it (pe_util.compare_lines). The records are therefore the CPU oracle's (the walk of
    pe_util.oracle_pe_conclave_records, which the existing tests hold against this tap and against the reference's version-1 files);
    the tap is walked beside them, line for line as pe_util.oracle_pe_lines lays them out, for what the oracle's records do not
    carry: every record's first sequence as it was written, and its header. A proper pair is one record (score negated: two reads)
    whose first sequence is the second mate's where alnFragsPE swapped them (alnfrags.c:1807-1812)."""
    import oracle
    import pe_util
    from kma_amd import formats
    db = oracle.OracleDB(g["prefix"])
    al = oracle.OracleAligner(db)
    lines = _tap_lines("pe")
    recs, at = [], 0

    def se_record(r, rc, rc_flag, flag, T):
        nonlocal at
        words, N = pe_util.emitted(r, rc)
        b = formats.pack_ragged([pe_util.codes_of(words, r["seqlen"], N)])
        res = db.align_se(b, np.array([rc_flag], np.int32), np.array([flag & ~16], np.int32), np.array([0, len(T)], np.int64), np.asarray(T, np.int32))
        nh = int(res["n_hits"][0])
        if nh > 0:
            ln = lines[at]
            at += 1
            recs.append((nh, int(res["best_score"][0]), r["seqlen"], 0, res["start"][:nh].tolist(), res["end"][:nh].tolist(), res["tmpl"][:nh].tolist(), ln[0], ln[6]))

    for u in g["units"]:
        if u[0] == "se":
            r = g["s1"][u[1]]
            rf, fl, To, T = db.scan_se(formats.pack_ragged([pe_util.codes_of(r["seq"], r["seqlen"], r["N"])]))
            if To[1] > To[0]:
                se_record(r, int(fl[0]) & 16, int(rf[0]), int(fl[0]), T)
            continue
        a, b = g["s1"][u[1]], g["s1"][u[2]]
        _, rs = db.scan_pe(a["seq"], a["seqlen"], a["N"], b["seq"], b["seqlen"], b["N"])
        if len(rs) == 2 and len(rs[0]["T"]) == 0:
            ra, rb = (a, b)[rs[0]["mate"]], (a, b)[rs[1]["mate"]]
            wa, na = pe_util.emitted(ra, rs[0]["rc"])
            wb, nb = pe_util.emitted(rb, rs[1]["rc"])
            _, o = al.align_pe(np.asarray(wa), ra["seqlen"], np.asarray(na), rs[0]["flag"], np.asarray(wb), rb["seqlen"], np.asarray(nb), rs[1]["flag"], rs[1]["T"])
            n, nr = o["n_hits"], o["n_hits_r"]
            cut = lambda lo, hi: (o["start"][lo:hi].tolist(), o["end"][lo:hi].tolist(), o["tmpl"][lo:hi].tolist())
            if o["kind"] == 1:
                la, lb = lines[at], lines[at + 1]
                at += 2
                first, second = (lb, la) if o["swapped"] else (la, lb)
                recs.append((n, -o["best"], len(first[0]), len(second[0])) + cut(0, n) + (first[0], la[6]))
            elif o["kind"] == 2:
                la, lb = lines[at], lines[at + 1]
                at += 2
                if n:
                    recs.append((n, o["best"], ra["seqlen"], 0) + cut(0, n) + (la[0], la[6]))
                if nr:
                    recs.append((nr, o["best_r"], rb["seqlen"], 0) + cut(n, n + nr) + (lb[0], lb[6]))
            elif o["kind"] in (3, 4):
                ln = lines[at]
                at += 1
                if n:
                    recs.append((n, o["best"] if o["kind"] == 3 else o["best_r"], (ra if o["kind"] == 3 else rb)["seqlen"], 0) + cut(0, n) + (ln[0], ln[6]))
        else:
            for x in rs:
                se_record((a, b)[x["mate"]], x["rc"], x["rc_flag"], x["flag"], x["T"])
    assert at == len(lines), (at, len(lines))
    return recs


def _run(name, g=None):
    recs = _records(name, g)
    if name in SEEDED:
        import proxi_util
        from kma_amd import synth
        fam, var, db_seed, _, _ = proxi_util.INPUTS[SEEDED[name]]
        names, seqs = synth.make_gene_db(fam, var, 500, 1300, 0.04, seed=db_seed)
        tlen = np.array([0] + [len(x) for x in seqs], np.int32)
    else:
        names = golden_util.template_names(name)
        tlen = np.fromfile(os.path.join(golden_util.GOLD, name, "db.length.b"), np.int32)[1:].copy()
        tlen[0] = 0
    n_hits = np.array([r[0] for r in recs], np.int32)
    score = np.array([r[1] for r in recs], np.int32)
    off = np.concatenate([[0], np.cumsum(n_hits)]).astype(np.int64)
    flat = lambda k: np.array([x for r in recs for x in r[k]], np.int32)
    tmpl = flat(6)
    AS, US = c2.vectors_from_records(n_hits, score, off, tmpl, len(tlen))
    seed = np.array([c2.seed_of([CODE[ch] for ch in r[7]]) if len(r[7]) >= 16 else 0 for r in recs], np.int32)
    out = c2.conclave2(n_hits, score, [r[2] for r in recs], [r[3] for r in recs], off, seed, tmpl, flat(4), flat(5), AS, US, tlen)
    return recs, out, names


@pytest.mark.parametrize("name", ["se", "pe", "c400", "a200"])
def test_restatement_names_every_row_of_the_reference(name, golden_pe):
    recs, out, names = _run(name, golden_pe if name == "pe" else None)
    for r in recs:          # (the tap's sequences are the records': their lengths are)
        assert len(r[7]) == r[2], r
    # every row of the reference's `.frag.gz`: header -> template (the mates of a pair record are filed under one template)
    want = {}
    with gzip.open(os.path.join(GOLD, name + ".frag.gz"), "rt") as f:
        for line in f:
            c = line.rstrip("\n").split("\t")
            want.setdefault(c[6], []).append(c[5])
    got = {}
    for r, t in zip(recs, out["tmpl"]):
        if t:
            got.setdefault(r[8], []).extend([names[abs(int(t)) - 1]] * (2 if r[1] < 0 else 1))
    rows = 0
    for h, ts in want.items():          # (a filed fragment that stage 3c's read filter drops leaves no row: the rows are a part of what is filed)
        have = list(got.get(h, []))
        for t in ts:
            assert t in have, (h, got.get(h), ts)
            have.remove(t)
        rows += len(ts)
    assert rows > {"c400": 250, "a200": 100}.get(name, 900)
    # the Score column of every row of its `.res`
    res = 0
    with open(os.path.join(GOLD, name + ".res")) as f:
        for line in f:
            if line.startswith("#"):
                continue
            c = [x.strip() for x in line.split("\t")]
            assert int(out["w_scores"][names.index(c[0]) + 1]) == int(c[1]), c[:2]
            res += 1
    assert res > (30 if name == "a200" else 50)
    # both routes of the fourth pass are taken: every ambiguous read of the two golden inputs (and of c400, where few reads leave the
    # second pass much to discard) draws its template; a200 has reads none of whose templates has a unique score
    cnt = out["counters"]
    assert cnt["draw"] >= 1, cnt
    if name == "c400":
        assert cnt["discarded"] >= 50 and cnt["made_unique"] >= 1, cnt
    if name == "a200":
        assert cnt["fallback"] >= 1, cnt
    if name == "pe":
        assert cnt["empty"] >= 1, cnt


def test_version_2_moves_rows_of_the_golden_input():
    """(the fixture is not the version-1 result under another name)"""
    v1 = {c[6]: c[5] for c in (l.rstrip("\n").split("\t") for l in gzip.open(os.path.join(golden_util.GOLD, "se", "out.frag.gz"), "rt"))}
    v2 = {c[6]: c[5] for c in (l.rstrip("\n").split("\t") for l in gzip.open(os.path.join(GOLD, "se.frag.gz"), "rt"))}
    assert sum(v1.get(h) != t for h, t in v2.items()) >= 50
