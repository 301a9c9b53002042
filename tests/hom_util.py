"""Homology reduction of a sparse index (`kma index -Sparse ... -hq x -ht y [-and]`: index.c:309-350 / 607-613, updateindex.c:103,
queryCheck and templateCheck of qualcheck.c:81-324) restated in plain Python on strings, on top of sparse_index_util's windows, and the
fixture cases of tests/golden/homology/ (made by tests/golden/make_golden_homology.py). test_homology_oracle.py pins the restatement
to the reference's recorded reports and files. No test lives here.

The rule. Templates come in file order. One that is longer than MinLen and has thisKlen >= max(MinKlen, 1) windows (N's and all, with
a prefix or without) walks its windows, forward strand then reverse complement, through the index of the templates kept so far:
Scores_tot[j] += 1 for every kept j that holds the window's k-mer, Scores[j] += 1 the first time the k-mer is seen; a template joins
bestTemplates when it is first met, the members of one value list in ascending id. thisQ = 1.0 * Scores_tot[j] / thisKlen, thisT =
1.0 * Scores[j] / ulen[j]; the maxima are taken with a strict `>` in the order of bestTemplates. templateCheck (-ht < 1) keeps the
template iff cmp(bestT < homT, bestQ < homQ), cmp = or, and under -and; queryCheck (otherwise -hq < 1) iff bestQ < homQ; it prints
one line per template that reached the gate."""
import os

import sparse_index_util as siu

ROOT = siu.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "homology")
KMA = siu.KMA
INDEX = siu.INDEX
INPUT = os.path.join(GOLDEN, "db.fsa.gz")

# case -> (k, the argument of -Sparse, -ML or 0, -hq or None, -ht or None, -and)
CASES = {}
for _sp, _tag in (("TG", "TG"), ("-", "none")):
    CASES[_tag + "_hq06"] = (16, _sp, 0, 0.6, None, False)
    CASES[_tag + "_hq05"] = (16, _sp, 0, 0.5, None, False)
    CASES[_tag + "_ht045_hq045_and"] = (16, _sp, 0, 0.45, 0.45, True)
    CASES[_tag + "_ht08_hq08"] = (16, _sp, 0, 0.8, 0.8, False)
    CASES[_tag + "_ht09"] = (16, _sp, 0, None, 0.9, False)
CASES["TG_hq06_ML300"] = (16, "TG", 300, 0.6, None, False)
CASES["k12_TG_hq06"] = (12, "TG", 0, 0.6, None, False)
CASES["k12_TG_ht08_hq08"] = (12, "TG", 0, 0.8, 0.8, False)


def kma_args(case):
    k, sp, ml, hq, ht, a = CASES[case]
    return (["-k", str(k), "-Sparse", sp] + (["-ML", str(ml)] if ml else []) + (["-ht", repr(ht)] if ht is not None else [])
            + (["-hq", repr(hq)] if hq is not None else []) + (["-and"] if a else []))


def build_kwargs(case):
    k, sp, ml, hq, ht, a = CASES[case]
    return dict(k=k, sparse=sp, min_len=ml, hom_q=1.0 if hq is None else hq, hom_t=1.0 if ht is None else ht, hom_and=a)


class Hom(siu.Built):
    """siu.Built under the homology rule, and besides: report (the bytes on standard output) and rows: per candidate template (one
    longer than MinLen) in file order [stays, thisKlen, max Scores_tot, templateQ, Scores and ulen of the best thisT, templateT], the
    templates counted in file order over the candidates, 1 .. (0: none) -- what the device hands back before ids are given out"""

    def __init__(self, paths, sparse, k=None, min_len=0, hom_q=1.0, hom_t=1.0, hom_and=False):
        self.k = self.kmerindex = k or 16
        text = "" if sparse == "-" else "".join(siu._LETTERS[c] for c in sparse)
        self.prefix_len, self.prefix = len(text), (siu.encode(text) if text else 1)
        MinLen, MinKlen = siu.gates(self.k, self.kmerindex, len(text), min_len)
        mode = 2 if hom_t < 1 else 1 if hom_q < 1 else 0
        assert mode, "thresholds of 1: that is siu.Built"
        self.names, self.lengths, self.slengths, self.ulengths = [None], [self.kmerindex], [0], [0]
        self.lists, self.skipped, self.seqs = {}, [], [None]
        self.rows, report = [], []
        held = {}          # k-mer string -> candidates (file order, 1 ..) that stayed and hold it
        cand_id, cand_ulen = {}, {}          # candidate -> id in the index, ulen
        cand = 0
        for path in ([paths] if isinstance(paths, (str, bytes, os.PathLike)) else paths):
            for name, seq, lead in siu.read_fasta(path):
                if not MinLen < len(seq):
                    self.skipped.append(name)
                    continue
                cand += 1
                ws = siu.windows(seq, self.k, text)
                klen = len(ws)
                if klen == 0 or klen < MinKlen:
                    self.rows.append([0, klen, 0, 0, 0, 0, 0])
                    self.skipped.append(name)
                    continue
                tot, uniq, order, seen = {}, {}, [], set()
                for km in ws:
                    lst = held.get(km)
                    if not lst:
                        continue
                    for j in lst:
                        if j not in tot:
                            tot[j] = uniq[j] = 0
                            order.append(j)
                        tot[j] += 1
                    if km not in seen:
                        seen.add(km)
                        for j in lst:
                            uniq[j] += 1
                bestQ = bestT = 0.0
                tQ = tT = 0
                for j in order:
                    q = 1.0 * tot[j] / klen
                    if q > bestQ:
                        bestQ, tQ = q, j
                    t = 1.0 * uniq[j] / cand_ulen[j]
                    if t > bestT:
                        bestT, tT = t, j
                if mode == 1:
                    stays = bestQ < hom_q
                elif hom_and:
                    stays = bestT < hom_t and bestQ < hom_q
                else:
                    stays = bestT < hom_t or bestQ < hom_q
                idQ, idT = cand_id.get(tQ, 0), cand_id.get(tT, 0)
                tid = len(self.names)
                if mode == 1:
                    report.append("%s\t%d\t%f\t%d\n" % (name, tid if stays else idQ, bestQ, idQ))
                else:
                    report.append("%s\t%d\t%f\t%d\t%f\t%d\n" % (name, tid if stays else (idQ if bestT < hom_t else idT), bestQ, idQ, bestT, idT))
                self.rows.append([int(stays), klen, tot.get(tQ, 0), tQ, uniq.get(tT, 0), cand_ulen.get(tT, 0), tT])
                if not stays:
                    self.skipped.append(name)
                    continue
                u = set(ws)
                for km in u:
                    held.setdefault(km, []).append(cand)
                    self.lists.setdefault(siu.encode(km), []).append(tid)
                cand_id[cand], cand_ulen[cand] = tid, len(u)
                self.names.append(name + (" B%d" % lead if lead else ""))
                self.lengths.append(len(seq)); self.slengths.append(klen); self.ulengths.append(len(u))
                self.seqs.append(seq)
        self.DB_size = len(self.names)
        self.report = "".join(report).encode("latin-1")


def built(case, paths=None):
    k, sp, ml, hq, ht, a = CASES[case]
    return Hom(paths or INPUT, sp, k=k, min_len=ml, hom_q=1.0 if hq is None else hq, hom_t=1.0 if ht is None else ht, hom_and=a)


def report(case):
    return open(os.path.join(GOLDEN, case + ".report.tsv"), "rb").read()


def parse_report(data):
    """-> {name: fields behind it as numbers}"""
    out = {}
    for line in data.decode("latin-1").split("\n")[:-1]:
        f = line.split("\t")
        out[f[0]] = [float(x) if "." in x else int(x) for x in f[1:]]
    return out
