"""The rule of a sparse index build as tests/sparse_index_util.py restates it, held to the reference's own files: the five cases of
tests/golden/sparse_index/ (N's, skipped templates, k = 12, -ML) and the four sparse indexes under tests/golden/sparse/ that have a
committed FASTA. The mapping, DB_size, the names, the three length arrays, the header's prefix and the skipped names are compared.
No GPU."""
import os

import numpy as np
import pytest

import sparse_index_util as siu

_built = {}


def built(case):
    if case not in _built:
        if case in siu.CASES:
            k, sp, ml = siu.CASES[case]
            _built[case] = siu.Built(siu.inputs(), sp, k=k, min_len=ml)
        else:
            _built[case] = siu.Built(siu.OLD[case][2], siu.OLD[case][3], k=16)
    return _built[case]


def reference(case, tmp_path):
    if case in siu.CASES:
        return siu.Files(siu.unpack(siu.GOLDEN, case, tmp_path))
    folder, name = siu.OLD[case][:2]
    return siu.Files(siu.unpack(os.path.join(siu.ROOT, "tests", "golden", "sparse", folder), name, tmp_path, with_seq=False))


@pytest.mark.parametrize("case", list(siu.CASES) + list(siu.OLD))
def test_restatement_equals_the_reference_index(case, tmp_path):
    want, got = reference(case, tmp_path), built(case)
    assert (got.DB_size, got.k, got.prefix_len, got.prefix) == (want.DB_size, want.k, want.prefix_len, want.prefix)
    assert want.mlen == want.k and want.flag == 0
    assert got.name_file() == want.name_file
    assert (got.lengths, got.slengths, got.ulengths) == (want.lengths, want.slengths, want.ulengths)
    assert got.length_b() == want.length_b
    assert got.lists == want.lists and len(want.lists) == want.n
    # ulengths are what the lists say: every id occurs in ulen lists
    occ = np.zeros(want.DB_size, np.int64)
    for ids in want.lists.values():
        occ[ids] += 1
    assert occ.tolist() == want.ulengths


@pytest.mark.parametrize("case", list(siu.CASES))
def test_skipped_names_and_sequence_words(case, tmp_path):
    got = built(case)
    assert got.skipped == siu.skipped(case)
    ref = np.fromfile(os.path.join(siu.GOLDEN, case + ".seq.b"), np.uint64)
    o = 0
    for L, words in zip(got.lengths[1:], got.seq_words()):
        assert ref[o:o + len(words)].tolist() == words
        o += (L >> 5) + 1
    assert o == len(ref)


def test_the_cases_differ_where_they_should():
    """no case is a copy of another: the gates and the prefix all bite"""
    tg, none, atg, nok, ml = (built(c) for c in siu.CASES)
    assert (nok.names, nok.lists, nok.lengths) == (tg.names, tg.lists, tg.lengths)          # -k 16 is the default
    assert none.DB_size > tg.DB_size > ml.DB_size > 2 and atg.k == 12 and atg.lengths[0] == 12
    assert siu.gates(16, 16, 2, 60) == (60, 5) and siu.gates(16, 16, 2, 19) == (16, 1) and siu.gates(16, 16, 2, 20) == (20, 0)
    assert set(ml.skipped) - set(tg.skipped) >= {"ml_len_60", "reverse_strand_only"}
