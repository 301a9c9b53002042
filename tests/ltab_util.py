"""Shared by the tests of the list table (DevDB::lslots, the second probe table whose value is a k-mer's value-list offset): the small
index they open and a host model of the table's buckets. No test lives here.

The index is the one of tests/test_scan_diag_route_gpu.py without its extra template -- 6 families x 5 variants of 300-400 bases,
4 475 distinct 16-mers -- and one template more, `wrap`: five 16-mers, found on the host, whose home is the LAST bucket of the list
table (and, their hash's leading bits being all ones, of every smaller table too), back to back. A bucket holds four, so the fifth is
stored in bucket 0. The 60 16-mers across the joints of `wrap` belong to the index like any other.

Which buckets end up full and which are passed by an insertion does not depend on the order of the insertions (bucketised linear
probing: a bucket passes on what its four slots do not hold), so `buckets()` gives what the device's table must look like."""
import numpy as np

from kma_amd import formats, synth

K = 16
GOLD = 0x9E3779B1
N_FAM, N_VAR = 6, 5
MISS = 0xFFFFFFFF


def home(keys, log2):
    return (((np.asarray(keys, np.uint64) * np.uint64(GOLD)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2)).astype(np.int64)


def kmers(seqs):
    return np.unique(formats._all_kmers(seqs, K)[0]).astype(np.uint64)


def codes_of_key(key):
    return np.array([(int(key) >> (2 * (K - 1 - i))) & 3 for i in range(K)], np.uint8)


def probe_log2(n):
    """log2 of the probe table's bucket count for n k-mers (db.hip: >= 2n slots in buckets of four, 16 buckets at least)"""
    lg = 4
    while (4 << lg) < 2 * n:
        lg += 1
    return lg


def make_db():
    """-> names, seqs, the five keys of `wrap`"""
    names, seqs = synth.make_gene_db(n_families=N_FAM, variants=N_VAR, len_lo=300, len_hi=400, max_div=0.04, seed=707)
    have = kmers(seqs)
    assert len(have) == 4475
    lg = probe_log2(len(have) + 65) + 1
    cand = np.random.default_rng(709).integers(0, 1 << 32, 1 << 20, dtype=np.uint64)
    cand = cand[(home(cand, lg) == (1 << lg) - 1) & ~np.isin(cand, have)]
    _, first = np.unique(cand, return_index=True)
    five = cand[np.sort(first)[:5]]
    assert len(five) == 5
    wrap = np.concatenate([codes_of_key(x) for x in five])
    return list(names) + ["wrap"], list(seqs) + [wrap], five


def buckets(keys, log2):
    """the table of 1 << log2 buckets of four over the distinct keys -> (occupied slots per bucket, bucket passed by an insertion)"""
    nb = 1 << log2
    arr = np.bincount(home(keys, log2), minlength=nb).astype(np.int64)
    occ = arr.copy()
    passed = np.zeros(nb, bool)
    carry = 0
    for _ in range(4):          # (laps: what the last bucket passes on arrives in bucket 0)
        for b in range(nb):
            tot = occ[b] + carry
            occ[b] = min(4, tot)
            carry = tot - occ[b]
            if carry:
                passed[b] = True
        if not carry:
            break
    assert carry == 0 and occ.sum() == len(keys)
    return occ, passed


def longest_chain(passed):
    nb = len(passed)
    run = best = 0
    for b in range(2 * nb):
        run = run + 1 if passed[b % nb] else 0
        best = max(best, min(run, nb))
    return best


def expected(comp, keys):
    """the list offset of every key by the index file's own arrays (formats.read_comp_b), MISS where the index has no such k-mer"""
    ik = np.asarray(comp.key_index[:comp.n], np.uint64)
    order = np.argsort(ik, kind="stable")
    ik, iv = ik[order], np.asarray(comp.value_index, np.uint64)[order]
    keys = np.asarray(keys, np.uint64)
    at = np.minimum(np.searchsorted(ik, keys), len(ik) - 1)
    return np.where(ik[at] == keys, iv[at], np.uint64(MISS)).astype(np.uint32)


def one_base_changed(keys, seed):
    """every key with one of its 16 bases replaced by another"""
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, np.uint64)
    sh = np.uint64(2) * rng.integers(0, K, len(keys)).astype(np.uint64)
    return keys ^ (rng.integers(1, 4, len(keys)).astype(np.uint64) << sh)
