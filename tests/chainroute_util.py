"""The anchor rule of the default mode's chain finder (save_kmers_chain, savekmers.c:5208-5452) restated in plain Python over the
oracle's hash lookup, and from it the route a read takes through kmahip_chain_device: what tests/golden/make_golden_chainroute.py aims
its reads with and what tests/test_chainroute_oracle.py and tests/test_chainroute_gpu.py hold cases.tsv and the route counts to.

An anchor opens at a k-mer start that hits the index unless the hit before it has the same value list and lies 0 or exactly k missed
starts back. Both strands are walked in FORWARD read coordinates; a strand is walked only when one of its every-k-th k-mers hits (or in
the exhaustive mode)."""
import ctypes as C
import gzip
import lzma
import os
import shutil

import numpy as np

import oracle
from kma_amd import formats, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "chainroute")

# the limits of the fast route (scan.hip: CA_NPMAX, CA_AMAX; chain.hip: CHAIN_LDS_TS)
NPMAX, AMAX, TSLOTS = 288, 32, 16
KS = (16, 12)
CONFIGS = [(k, ex) for k in KS for ex in (0, 1)]


def cfg_name(k, ex):
    return f"k{k}" + ("x" if ex else "")


class _OrcDB(C.Structure):          # the head of orc_db (oracle/kma_oracle.h)
    _fields_ = [("DB_size", C.c_uint32), ("mlen", C.c_uint32), ("prefix_len", C.c_uint32), ("kmersize", C.c_uint32), ("flag", C.c_uint32),
                ("prefix", C.c_uint64), ("size", C.c_uint64), ("n", C.c_uint64), ("v_index", C.c_uint64), ("null_index", C.c_uint64),
                ("exist", C.c_void_p), ("key32", C.c_void_p), ("key64", C.c_void_p), ("value_index", C.c_void_p),
                ("values16", C.POINTER(C.c_uint16)), ("values32", C.POINTER(C.c_uint32))]


def value_list(odb, v):
    """the templates of the value list at offset v"""
    d = C.cast(odb.h, C.POINTER(_OrcDB)).contents
    a = d.values16 if d.values16 else d.values32
    return [int(a[v + i]) for i in range(1, int(a[v]) + 1)]


def is_u32(odb):
    return not C.cast(odb.h, C.POINTER(_OrcDB)).contents.values16


def kmersize(odb):
    return int(C.cast(odb.h, C.POINTER(_OrcDB)).contents.kmersize)


def _strands(read):
    """the read as the reference packs it (N -> A) and its reverse complement, as code arrays, with their N positions"""
    read = np.asarray(read, np.uint8)
    L = len(read)
    N = np.flatnonzero(read == 4).astype(np.int32)
    fw = read.copy()
    fw[N] = 0
    b = formats.pack_ragged([read])
    words = np.zeros(((L + 31) >> 5) + 2, np.uint64)
    words[:(L + 31) >> 5] = b.seq[:(L + 31) >> 5]
    rwords, rN = oracle.rc_packed(words[:(L + 31) >> 5], L, N)
    rc = formats.unpack_words(np.asarray(rwords, np.uint64), L).copy()
    return fw, N.tolist(), rc, [int(x) for x in rN]


def _key(codes, pos, k):
    v = 0
    for c in codes[pos:pos + k]:
        v = (v << 2) | int(c)
    return v


def analyse(odb, read, exhaustive=0):
    """-> dict(starts, live=[F, R], anchors=[F, R] (each a list of (first start, last hit, value list offset)), templates = the distinct
    templates of the walked strands' anchors, has_N). Mirrors build_ankers of oracle/chain.c, N's and the reverse strand's restart behind
    an N included."""
    k = kmersize(odb)
    L = len(read)
    out = dict(starts=max(L - k + 1, 0), live=[False, False], anchors=[[], []], templates=set(), has_N=bool((np.asarray(read) == 4).any()))
    if L < k:
        return out
    fw, N, rc, rN = _strands(read)
    nN = len(N)
    cache = {}

    def get(codes, pos):
        key = _key(codes, pos, k)
        if key not in cache:
            cache[key] = odb.hash_get(key)
        return cache[key]
    for strand in (0, 1):
        s, Ns = (rc, rN) if strand else (fw, N)
        hit = bool(exhaustive)
        j = 0
        for i in range(nN + 1):
            segend = Ns[i] if i < nN else L
            while j < segend - k + 1 and not hit:
                hit = get(s, j) >= 0
                j += k
            j = segend + 1
        out["live"][strand] = hit
        if not hit:
            continue
        A = out["anchors"][strand]
        last, gaps, j, rcpos = -1, 0, 0, L - k
        for i in range(nN + 1):
            if j >= L - k + 1:
                break
            segend = N[i] if i < nN else L
            while j < segend - k + 1:
                if strand:
                    assert 0 <= rcpos <= L - k, "an N among the first k - 1 bases: the reference reads beyond the strand (DESIGN 3.1b)"
                    v = get(rc, rcpos)
                else:
                    v = get(fw, j)
                if v >= 0:
                    if v == last and gaps in (0, k):
                        A[-1][1] = j
                    else:
                        A.append([j, j, v])
                        last = v
                    gaps = 0
                else:
                    gaps += 1
                j += 1
                rcpos -= 1
            gaps += segend + 1 - j
            j = segend + 1
            rcpos = L - j
        for a in A:
            out["templates"].update(value_list(odb, a[2]))
    return out


def route_of(a):
    """the route of a read from its analysis: 'none' (too short, no strand walked or no anchor: nothing is chained), 'fast',
    'marked:N' / 'marked:starts' / 'marked:aF' / 'marked:aR' (chain_anchor_kernel hands it over; the first reason that applies), 'given_up'
    (chain_fast_kernel finds its table of 16 templates full)"""
    if a["starts"] <= 0 or not any(a["live"]):
        return "none"
    if a["has_N"]:
        return "marked:N"
    if a["starts"] > NPMAX:
        return "marked:starts"
    if len(a["anchors"][0]) > AMAX:
        return "marked:aF"
    if len(a["anchors"][1]) > AMAX:
        return "marked:aR"
    if not a["anchors"][0] and not a["anchors"][1]:
        return "none"
    return "given_up" if len(a["templates"]) > TSLOTS else "fast"


def counts_of(routes, has_N, env=None):
    """what kmahip_chain_get_route_counts must report for reads of these routes under the switches of `env`"""
    env = env or {}
    n = len(routes)
    if env.get("KMAHIP_CHAIN") == "slow":
        return dict(reads=n, marked=0, given_up=0, long=0, lane=n)
    marked = sum(r.startswith("marked") for r in routes)
    given = sum(r == "given_up" for r in routes)
    left = [hn for r, hn in zip(routes, has_N) if r.startswith("marked") or r == "given_up"]
    lane = len(left) if env.get("KMAHIP_CHAIN_LONG") == "0" else sum(left)
    return dict(reads=n, marked=marked, given_up=given, long=len(left) - lane, lane=lane)


def table(path):
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        return [{k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in zip(head, line.rstrip("\n").split("\t"))} for line in f]


def load(tmp):
    """tests/golden/chainroute unpacked into tmp: prefix = {16: ..., 12: ...}, the reads (codes 0-4, file order) with their names, cases
    (one dict per read, cases.tsv), tap = {'k16', 'k16x', 'k12', 'k12x': S2 records of the reference's `-s2` run, x: -ex_mode}, the paths of the FASTQ and of the whole-run files"""
    tmp = str(tmp)
    os.makedirs(tmp, exist_ok=True)
    prefix = {}
    for k in KS:
        prefix[k] = os.path.join(tmp, f"db{k}")
        with lzma.open(os.path.join(GOLD, f"db{k}.comp.b.xz"), "rb") as f, open(prefix[k] + ".comp.b", "wb") as g:
            shutil.copyfileobj(f, g)
        shutil.copy(os.path.join(GOLD, f"db{k}.length.b"), prefix[k] + ".length.b")
        for ext in (".seq.b", ".name"):
            shutil.copy(os.path.join(GOLD, "db" + ext), prefix[k] + ext)
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    names, reads = [], []
    with gzip.open(os.path.join(GOLD, "reads.fq.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    for i in range(0, len(lines) - 3, 4):
        names.append(lines[i][1:].decode())
        reads.append(lut[np.frombuffer(lines[i + 1], np.uint8)])
    fq = os.path.join(tmp, "reads.fq")
    with open(fq, "wb") as f:
        f.write(b"\n".join(lines))
    cases = table(os.path.join(GOLD, "cases.tsv"))
    assert [c["name"] for c in cases] == names
    tap = {}
    for k, ex in CONFIGS:
        with gzip.open(os.path.join(GOLD, f"s2_{cfg_name(k, ex)}.bin.gz"), "rb") as f:
            tap[cfg_name(k, ex)], _ = formats.parse_s2(f.read())
    return dict(dir=GOLD, prefix=prefix, names=names, reads=reads, cases=cases, tap=tap, fastq=fq, batch=formats.pack_ragged(reads))


def flat(per_read):
    """OracleDB.scan_chain's lists -> (read, rc_flag, emit_rc, q_start, q_end, templates) in stream order"""
    return [(i, rf, er, qs, qe, tuple(int(t) for t in T)) for i, recs in enumerate(per_read) for rf, er, qs, qe, T in recs]


def tap_by_read(tap):
    """the tap's records per read name: [(q_start, q_end, rc_flag, templates, packed sequence)]"""
    import struct
    out = {}
    for w in tap:
        h = w["hdr"]
        nm = h[:len(h) - 10].decode()          # (name, its NUL, a NUL, the two bounds)
        qs, qe = struct.unpack("<2i", h[-8:])
        out.setdefault(nm, []).append((qs, qe, int(w["rc_flag"]), tuple(int(t) for t in w["T"]), w["seq"]))
    return out


def wide_set(prefix):
    """66 000 short templates (tests/test_variants_gpu.py) and behind them a SNP ladder, a template of its own, a family with windows
    shared by 3 and 2 members and one with windows shared by 17 and 16: an anchor then carries ONE element of its list, ank_at reads
    the second from the list itself"""
    rng = np.random.default_rng(41)
    names, seqs = synth.make_gene_db(16500, 4, 48, 72, 0.05, seed=9)
    names, seqs = list(names), list(seqs)
    n_short = len(seqs)

    def rnd(n):
        return rng.integers(0, 4, n, dtype=np.uint8)
    LE = rnd(420)
    LF = LE.copy()
    LF[8::17] = (LF[8::17] + 1 + rng.integers(0, 3, len(LF[8::17]), dtype=np.uint8)) & 3
    U = rnd(400)
    w3, w2, w17, w16 = rnd(80), rnd(80), rnd(80), rnd(80)
    extra = [("LE", LE), ("LF", LF), ("U", U)]
    extra += [(f"F3_{i}", np.concatenate([rnd(30), w3, rnd(15), w2 if i < 2 else rnd(80), rnd(30)])) for i in range(3)]
    extra += [(f"F17_{i}", np.concatenate([rnd(30), w17, rnd(15), w16 if i < 16 else rnd(80), rnd(30)])) for i in range(17)]
    names += [n for n, _ in extra]
    seqs += [s for _, s in extra]
    formats.write_index(prefix, names, seqs)
    reads = []
    for _ in range(150):
        s = seqs[int(rng.integers(0, n_short))]
        L = int(rng.integers(30, len(s) + 1))
        st = int(rng.integers(0, len(s) - L + 1))
        r = s[st:st + L].copy()
        m = rng.random(L) < 0.01
        r[m] = (r[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
        reads.append(r)
    reads += [LE[5:5 + L] for L in range(262, 305)]          # 29 to 35 anchors; the last one 289 starts
    reads += [U[10:70], w3[8:70], w2[8:70], w16[8:70], w17[8:70], np.concatenate([w3[8:60], w16[8:70]]), np.concatenate([w2[8:60], w17[8:70]])]
    for src, pos in ((U[100:250], 40), (w17[8:70], 30), (LE[5:300], 150)):
        r = src.copy()
        r[pos] = 4
        reads.append(r)
    reads += [rnd(150), rnd(40), rnd(304)]
    return reads[:150] + [x for r in reads[150:] for x in (r, synth.revcomp_codes(r))]
