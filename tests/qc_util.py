"""The QC report and the trimmed reads of `kma ... -qc` / `kma trim`, restated in plain Python: phredStat's accounting with a report
(runinput.c:127-313), the counts of run_input / run_input_PE / run_input_INT (:370-730), update_QCstat and print_QCstat (qc.c:85-104,
167-262) and printTrimFsa / printTrimFsa_pair (trim.c:28-126). Slow and simple: the checker of tests/golden/qc (test_qc_oracle.py)
and the yardstick for inputs made on the spot. Also the table of fixture cases and settings that the generator and the tests share."""
import gzip
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ING = os.path.join(GOLD, "ingest")
QC = os.path.join(GOLD, "qc")

# name -> library keywords, and the -5p / -3p values that are only printed
SETTINGS = {
    "default": {},
    "mp25": dict(min_phred=25),
    "eq15": dict(min_q=15),
    "eq25ml40": dict(min_q=25, min_len=40),
    "mi12": dict(hardmask_q=12),
    "ml60xl130": dict(min_len=60, max_len=130),
    "mi25clip": dict(hardmask_q=25, clip5=3, clip3=2),
    "ml1000": dict(min_len=1000),
}
FLAGS = {"min_phred": "-mp", "min_q": "-eq", "hardmask_q": "-mi", "min_len": "-ml", "max_len": "-xl", "clip5": "-5p", "clip3": "-3p"}
# name -> (single-end files, mate files two by two, interleaved files); a name without a folder lies in golden/ingest
CASES = {
    "p33": (["p33.fq"], [], []),
    "dos": (["dos.fq"], [], []),
    "p64": (["p64.fq"], [], []),
    "pe": ([], ["m1.fq", "m2.fq"], []),
    "int": ([], [], ["ilv.fq"]),
    "intodd": ([], [], ["ilvodd.fq"]),
    "p33gz": (["p33gz.fq.gz"], [], []),
    "long": (["qc/long.fq.gz"], [], []),
    "uni": (["qc/uni.fq"], [], []),
    "one": (["qc/one.fq"], [], []),
    "p33+p64": (["p33.fq", "p64.fq"], [], []),
}


def path_of(name):
    return os.path.join(GOLD, name) if "/" in name else os.path.join(ING, name)


def ref_flags(setting):
    out = []
    for k, v in SETTINGS[setting].items():
        out += [FLAGS[k], str(v)]
    return out


def trim_kw(setting):
    return {k: v for k, v in SETTINGS[setting].items() if k not in ("clip5", "clip3")}


# ---- the tables -------------------------------------------------------------------------------------------------------------------
TO2BIT = [8] * 256
TO2BIT[ord("\n")] = 16
for _c, _chars in enumerate(("ARMDrmd", "CYBcyb", "GSKVgskv", "TWHUtwh", "NXnx")):
    for _ch in _chars:
        TO2BIT[ord(_ch)] = _c
TO2BIT[ord("a")] = 0
# kma.c:219 / trim.c:151: 10^(-q/10) as 32-decimal literals
PROB = [float("%.32f" % math.pow(10, -0.1 * q)) for q in range(256)]


def read_bytes(path):
    with open(path, "rb") as f:
        raw = f.read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def read_fastq(buf):
    """FileBuffgetFq (seqparse.c:241-403) over well-formed records: [(header line chomped, with its '@'; sequence line bytes; as many
    quality bytes)]. Every byte of the sequence line counts, also the '\\r' of a DOS file."""
    out, o = [], 0
    while o < len(buf):
        e = buf.index(b"\n", o)
        hdr = buf[o:e].rstrip(b" \t\r\n\v\f")
        o = e + 1
        e = buf.index(b"\n", o)
        seq = buf[o:e]
        o = buf.index(b"\n", e + 1) + 1
        qual = buf[o:o + len(seq)]
        e = buf.find(b"\n", o + len(seq))
        o = len(buf) if e < 0 else e + 1
        out.append((hdr, seq, qual))
    return out


def guess_phred(buf):
    """getPhredFileBuff (seqparse.c:551-589) over the first file buffer"""
    buf = buf[:1048576]
    avail, scale, maxlen, p = len(buf), 33, 0, 0
    while avail:
        seek = 3
        while seek:
            avail -= 1
            if not avail:
                break
            p += 1
            if buf[p] == 10:
                seek -= 1
        length, seek = 0, 1 if avail else 0
        while seek:
            avail -= 1
            if not avail:
                break
            p += 1
            c = buf[p]
            if c == 10:
                seek = 0
            elif c < 33:
                return 0
            elif 53 < c < 59:
                return 33
            elif 94 < c:
                scale = 64
            length += 1
        maxlen = max(maxlen, length)
    return scale if maxlen <= 301 else 33


# ---- phredStat with a report ------------------------------------------------------------------------------------------------------
def phred_stat(seq, qual, phred, min_phred, min_q, hardmask_q, min_len, max_len, report=True):
    """seq: list of codes, changed in place (hard masking); qual: raw bytes. -> dict(ret, start, end, counted, len, gc, ns, sp, cut5, cut3)
    (ret: the figure held against -ml). min_phred as the caller raised it (to -mi and -eq)."""
    L = len(seq)
    r = dict(ret=0, start=0, end=0, counted=False, len=0, gc=0, ns=0, sp=0.0, cut5=0, cut3=0)
    if max_len < L:
        return r
    mp = phred + min_phred
    start, end = 0, L
    while start < end and qual[start] < mp:
        start += 1
    while start < end and qual[end - 1] < mp:
        end -= 1
    ln = end - start
    if not min_q and not hardmask_q and not report:
        r.update(ret=ln, start=start, end=end)
        return r
    ns = gc = 0
    sp = 0.0
    hq = hardmask_q          # (compared with the raw byte, as the reference does: runinput.c:179)
    for i in range(start, end):
        q = qual[i]
        sp += PROB[q - phred] if q >= phred else PROB[0]
        if seq[i] == 4 or q < hq:
            seq[i] = 4
            ns += 1
        elif seq[i] in (1, 2):
            gc += 1
    minP = math.pow(10, -0.1 * min_q)

    def pr(q):
        return PROB[q - phred] if q >= phred else PROB[0]
    if min_len <= ln - ns and minP * ln < sp:
        ns5 = ns3 = gc5 = gc3 = l5 = l3 = 0
        sp5 = sp3 = 0.0
        p5, p3 = start, end - 1

        def grow(p, step, l, s, n, g):
            for good in (True, False):
                while l < ln and ((mp <= qual[p]) if good else (qual[p] < mp)):
                    s += pr(qual[p])
                    l += 1
                    if seq[p] in (1, 2):
                        g += 1
                    elif seq[p] == 4:
                        n += 1
                    p += step
            return p, l, s, n, g
        p3, l3, sp3, ns3, gc3 = grow(p3, -1, l3, sp3, ns3, gc3)
        while min_len <= ln - ns and minP * ln < sp:
            if sp5 * l3 < sp3 * l5:
                end -= l3; ns -= ns3; gc -= gc3; ln -= l3; sp -= sp3
                r["cut3"] += 1 if l3 else 0
                p3, l3, sp3, ns3, gc3 = grow(p3, -1, 0, 0.0, 0, 0)
            else:
                start += l5; ln -= l5; ns -= ns5; gc -= gc5; sp -= sp5
                r["cut5"] += 1 if l5 else 0
                p5, l5, sp5, ns5, gc5 = grow(p5, 1, 0, 0.0, 0, 0)
    r.update(ret=ln - ns, start=start, end=end, len=ln, gc=gc, ns=ns, sp=sp, counted=report and min_len <= ln - ns)
    return r


# ---- update_QCstat / print_QCstat -------------------------------------------------------------------------------------------------
class QCStat:
    def __init__(self):
        self.fragcount = self.org_fragcount = self.count = self.org_count = 0
        self.bpcount = self.org_bpcount = self.totgc = self.totns = 0
        self.Eeq = 0.0
        self.maxlen = self.qresolution = 0
        self.phred_scale = 0
        self.qdist = [0] * 256
        self.ldist = [0] * 512

    def update(self, ln, gc, ns, sp):
        self.count += 1
        self.bpcount += ln
        self.totgc += gc
        self.totns += ns
        self.Eeq += sp
        if self.maxlen < ln:
            if 512 <= (ln >> self.qresolution):
                new = self.qresolution + 1
                while 512 <= (ln >> new):
                    new += 1
                mask = new - self.qresolution
                for i in range(1, 512):
                    v, self.ldist[i] = self.ldist[i], 0
                    self.ldist[i >> mask] += v
                self.qresolution = new
            self.maxlen = ln
        self.qdist[int(math.ceil(-10 * math.log10(sp / ln)))] += 1
        self.ldist[ln >> self.qresolution] += 1

    def n50_branch(self):
        if not (self.maxlen << 1) < self.bpcount:
            return "maxlen"
        return "scaled" if self.qresolution else "plain"

    def stats(self):
        return dict(fragcount=self.fragcount, org_fragcount=self.org_fragcount, count=self.count, org_count=self.org_count,
                    bpcount=self.bpcount, org_bpcount=self.org_bpcount, totgc=self.totgc, totns=self.totns, Eeq=self.Eeq, maxlen=self.maxlen,
                    qresolution=self.qresolution, phred_scale=self.phred_scale, qdist=np.array(self.qdist, np.uint32), ldist=np.array(self.ldist, np.uint32))

    def json(self, min_phred=20, min_q=0, hardmask_q=0, min_len=16, max_len=2**31 - 1, clip5=0, clip3=0):
        o = ["{\n"]
        o.append('\t"Maximum Trim length": %d,\n' % max_len)
        o.append('\t"Minimum Trim length": %d,\n' % min_len)
        o.append('\t"5\'-clip": %d,\n' % clip5)
        o.append('\t"3\'-clip": %d,\n' % clip3)
        if self.Eeq:
            o.append('\t"Minimum Q": %d,\n' % min_q)
            o.append('\t"End Trim Q": %d,\n' % max(min_phred, hardmask_q))
            o.append('\t"Hard Mask Q": %d,\n' % hardmask_q)
            o.append('\t"Phred Scale": %d,\n' % self.phred_scale)
        for name, v in (("Fragment Count", self.fragcount), ("Org. Fragment Count", self.org_fragcount), ("Sequence Count", self.count),
                        ("Org. Sequence Count", self.org_count), ("Bp Count", self.bpcount), ("Org. Bp Count", self.org_bpcount)):
            o.append('\t"%s": %d,\n' % (name, v))
        o.append('\t"Mean Read Length": %f,\n' % (self.bpcount / self.count if self.count else 0))
        o.append('\t"Org. Mean Read Length": %f,\n' % (self.org_bpcount / self.org_count if self.org_count else 0))
        o.append('\t"GC Content": %f,\n' % (self.totgc / (self.bpcount - self.totns) if self.bpcount - self.totns else 0))
        o.append('\t"Max Sequence Length": %d,\n' % self.maxlen)
        dist, scale = self.ldist, 1 << self.qresolution
        if (self.maxlen << 1) < self.bpcount:
            n50, tot = 0, 0
            if self.qresolution:
                i = 0
                while i < 511:
                    if dist[i]:
                        p = dist[i + 1] / (dist[i] + dist[i + 1])
                        tot = int(tot + (n50 + p * scale) * dist[i])          # (an unsigned long takes a double sum)
                        if self.bpcount < (tot << 1):
                            n50 = int(n50 + p * scale)
                            i = 512
                        else:
                            n50 += scale
                    else:
                        n50 += scale
                    i += 1
            else:
                for i in range(512):
                    tot += (i * dist[i]) & 0xFFFFFFFF
                    if self.bpcount < (tot << 1):
                        n50 = i
                        break
        else:
            n50 = self.maxlen
        o.append('\t"N50": %d,\n' % n50)
        if self.Eeq:
            o.append('\t"E(Q)": %f,\n' % (-10 * math.log10(self.Eeq / self.bpcount)))
            o.append('\t"Q Distribution": [' + ", ".join(str(v) for v in self.qdist) + "],\n")
        o.append('\t"Length Resolution": %d,\n' % scale)
        o.append('\t"Length Distribution": [' + ", ".join(str(v) for v in dist) + "]\n")
        o.append("}\n")
        return "".join(o)


# ---- run_input / run_input_PE / run_input_INT with a report, and the trimmed text ----------------------------------------------------
def restate(case, setting, report=True):
    """-> dict(qc=QCStat, json=str, fq=bytes, int_fq=bytes, both_ends=int): what `kma trim -qc` with the setting's flags makes of the
    case's files; both_ends counts the reads that the -eq loop cut at their 5' and at their 3' end"""
    kw = dict(min_phred=20, min_q=0, hardmask_q=0, min_len=16, max_len=2**31 - 1, clip5=0, clip3=0)
    kw.update(SETTINGS[setting])
    mp = max(kw["min_phred"], kw["hardmask_q"], kw["min_q"])
    qc = QCStat()
    out = [bytearray(), bytearray()]
    both_ends = 0
    se, pe, il = CASES[case]

    def one(rec, phred):
        nonlocal both_ends
        hdr, raw, qual = rec
        seq = [TO2BIT[c] for c in raw]
        if report:
            qc.org_count += 1
            qc.org_bpcount += len(seq)
        r = phred_stat(seq, qual, phred, mp, kw["min_q"], kw["hardmask_q"], kw["min_len"], kw["max_len"], report)
        if r["counted"]:
            qc.update(r["len"], r["gc"], r["ns"], r["sp"])
        both_ends += 1 if r["cut5"] and r["cut3"] else 0
        text = hdr + b"\n" + bytes(b"ACGTN-"[min(c, 5)] for c in seq[r["start"]:r["end"]]) + b"\n+\n" + qual[r["start"]:r["end"]] + b"\n"
        return kw["min_len"] <= r["ret"], text

    def couples(recs1, recs2, phred):
        n = max(len(recs1), len(recs2))
        empty = (b"", b"", b"")
        for i in range(n):
            ok1, t1 = one(recs1[i] if i < len(recs1) else empty, phred)
            ok2, t2 = one(recs2[i] if i < len(recs2) else empty, phred)
            qc.org_fragcount += 1
            if ok1 and ok2:
                out[1] += t1 + t2
            elif ok1:
                out[0] += t1
            elif ok2:
                out[0] += t2
            if ok1 or ok2:
                qc.fragcount += 1
        if qc.Eeq:
            qc.phred_scale = phred
    for f in se:
        buf = read_bytes(path_of(f))
        phred = guess_phred(buf)
        for rec in read_fastq(buf):
            ok, text = one(rec, phred)
            qc.org_fragcount += 1
            if ok:
                out[0] += text
                qc.fragcount += 1
        qc.phred_scale = phred
    for a, b in zip(pe[0::2], pe[1::2]):
        b1, b2 = read_bytes(path_of(a)), read_bytes(path_of(b))
        phred = guess_phred(b1) or guess_phred(b2)
        couples(read_fastq(b1), read_fastq(b2), phred)
    for f in il:
        buf = read_bytes(path_of(f))
        recs = read_fastq(buf)
        couples(recs[0::2], recs[1::2], guess_phred(buf))
    jkw = {k: kw[k] for k in ("min_phred", "min_q", "hardmask_q", "min_len", "max_len", "clip5", "clip3")}
    return dict(qc=qc, json=qc.json(**jkw), fq=bytes(out[0]), int_fq=bytes(out[1]), both_ends=both_ends)


# ---- comparing ----------------------------------------------------------------------------------------------------------------------
def gold(case, setting, ext):
    """a recorded file of tests/golden/qc: ext = json | s1 | fq | int_fq (None: the reference wrote no such file)"""
    p = os.path.join(QC, f"{case}.{setting}.{ext}.gz")
    return gzip.open(p).read() if os.path.exists(p) else None


def stats_of_json(text):
    import json
    return json.loads(text)


def same_stats(a, b):
    """two stats() dicts field by field -> list of the names that differ"""
    bad = []
    for k in a:
        if isinstance(a[k], np.ndarray):
            if not np.array_equal(a[k], b[k]):
                bad.append(k)
        elif a[k] != b[k]:
            bad.append(k)
    return bad


def compare_s1(batches, s1):
    """the batches of a reader, [(ReadBatch, names, pair)], against parsed S1 records, read for read"""
    i = 0
    for batch, names, pair in batches:
        for j in range(batch.n):
            assert i < len(s1), "more reads than the reference wrote"
            r = s1[i]
            L = int(batch.length[j])
            assert L == r["seqlen"], (i, L, r["seqlen"])
            w = batch.seq[batch.seq_off[j]:batch.seq_off[j] + ((L + 31) >> 5)]
            assert np.array_equal(w, r["seq"]), i
            assert np.array_equal(batch.N[batch.N_off[j]:batch.N_off[j + 1]], r["N"]), i
            assert names[j] + b"\0" == r["hdr"], (i, names[j], r["hdr"])
            assert (pair[j] == 1) == r["pair"], i
            i += 1
    assert i == len(s1), (i, len(s1))
