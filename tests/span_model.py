"""The span table of kmahip_db_open (DevDB::span, db.hip: span_mine_kernel, span_build_kernel) restated in plain Python over numpy
arrays, for the tests (no tests in here). tools/diag_model.py has a lazy form of its own for the benchmark's database (need at one
position at a time, no give-up, templates without N's). Per position p of the concatenated templates (template 1 first):

  t0    the template p lies in (0 where no k-mer with a value list starts at p)
  room  the k-mer starts from p on that lie inside t0 and have a value list that names t0, capped at NEVER
  need  the fewest of them, >= 1, whose value lists have no template but t0 in common; NEVER when there is no such number below NEVER
        (or when the list at p names more than LIST_MAX other templates: the builder gives up there; a later list of more than
        SCAN_MAX ids is passed over, which can only make need larger)

A read of npos k-mer starts that lies on the templates from p on without a mismatch has t0 as its only best template, with the score
k*M + (npos - 1)*M, exactly when need <= npos <= room (scan.hip: settle_allowed has the proof and the scoring schemes it holds for)."""
import numpy as np

NEVER = 255
LIST_MAX = 32
SCAN_MAX = 256


def kmer_codes(seq, k):
    """the k-mers of a uint8 code array (0..3) as integers, first base in the highest bits"""
    L = len(seq)
    if L < k:
        return np.zeros(0, np.uint64)
    x = seq.astype(np.uint64)
    km = np.zeros(L - k + 1, np.uint64)
    for i in range(k):
        km = (km << np.uint64(2)) | x[i:L - k + 1 + i]
    return km


def span_table(seqs, mapping, k, list_max=LIST_MAX):
    """seqs: the templates (uint8 codes) in index order; mapping: {k-mer: tuple of template ids} as the index holds them
    (formats.comp_db_mapping). -> (t0 uint32, need uint8, room uint8), one entry per base of the concatenated templates + 64"""
    total = sum(len(s) for s in seqs)
    t0 = np.zeros(total + 64, np.uint32)
    need = np.zeros(total + 64, np.uint8)
    room = np.zeros(total + 64, np.uint8)
    g0 = 0
    for t, s in enumerate(seqs, start=1):
        lists = [mapping.get(int(x)) for x in kmer_codes(s, k)]
        ns = len(lists)
        # starts from i on up to the first one without a list
        # (a template with an N: the stored sequence holds a base in its place, and a k-mer over it is at best another template's)
        run = [0] * (ns + 1)
        for i in range(ns - 1, -1, -1):
            run[i] = 0 if lists[i] is None or t not in lists[i] else run[i + 1] + 1
        for i in range(ns):
            rm = min(NEVER, run[i])
            if rm == 0:
                continue
            nd = NEVER
            others = set(lists[i]) - {t}
            if len(others) <= list_max:
                for j in range(rm):
                    if j and lists[i + j] is not lists[i + j - 1] and len(lists[i + j]) <= SCAN_MAX:
                        others &= set(lists[i + j])
                    if not others:
                        if j + 1 < NEVER:
                            nd = j + 1
                        break
            t0[g0 + i], need[g0 + i], room[g0 + i] = t, nd, rm
        g0 += len(s)
    return t0, need, room


def settled(need, room, npos):
    return (need <= npos) & (npos <= room)
