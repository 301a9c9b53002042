"""The list table (DevDB::lslots): for every 32-bit key, probe_list(key) == vs_id[probe(key)], or both miss -- through the hook
kmahip_test_list_probe, one lane per key -- and both equal the list offset the index file itself gives for the key.

The table is opened at twice the probe table's buckets (the default) and at as many (KMAHIP_LTAB_SHIFT=0), and looked up with the
passed flags honoured (the default) and ignored (KMAHIP_LTAB_FLAG=0): four combinations. What the flag is for -- a full bucket that no
insertion went past ends the lookup of an absent key -- what it must not break -- a key stored behind its home bucket, a chain of two
passed buckets, a key that wraps from the last bucket into bucket 0 -- are asserted of the fixture on the host, from the keys and the
hash alone (ltab_util.buckets), before the device is asked. The figures of this fixture (ltab_util.make_db: 4 540 distinct 16-mers):
8 192 buckets: 5 passed, 20 full, 15 full and not passed; 4 096 buckets: 22 passed, 108 full, 86 full and not passed, a chain of two."""
import os

import numpy as np
import pytest

import ltab_util as U
from kma_amd import formats, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("KMAHIP_SCAN_LTAB", "KMAHIP_LTAB_SHIFT", "KMAHIP_LTAB_FLAG")


def _open(prefix, shift, decon=False, **env):
    """the database opened with KMAHIP_LTAB_SHIFT=shift (and env) set for the time of the open only"""
    from kma_amd import binding
    env = dict(env, KMAHIP_LTAB_SHIFT=str(shift))
    was = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        return binding.KmaHipDB(prefix, decon=decon)
    finally:
        for k, v in was.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    names, seqs, five = U.make_db()
    prefix = str(tmp_path_factory.mktemp("ltab") / "db")
    formats.write_index(prefix, names, seqs, k=U.K)
    comp = formats.read_comp_b(prefix + ".comp.b")
    keys = np.sort(np.asarray(comp.key_index[:comp.n], np.uint64))
    assert np.array_equal(keys, U.kmers(seqs)) and len(keys) == 4540
    return dict(prefix=prefix, comp=comp, keys=keys, five=five)


def _absent(keys, log2, where, n, seed):
    """n keys that are not in the index and whose home bucket is one of `where`"""
    cand = np.random.default_rng(seed).integers(0, 1 << 32, 1 << 22, dtype=np.uint64)
    cand = np.unique(cand[np.isin(U.home(cand, log2), where) & ~np.isin(cand, keys)])
    assert len(cand) >= n, (len(cand), n)
    return cand[:n]


def _fixture_keys(small, shift):
    """the premise of the fixture at this bucket count, asserted on the host -> every key the device is asked for"""
    keys, five = small["keys"], small["five"]
    lg = U.probe_log2(len(keys)) + shift
    nb = 1 << lg
    occ, passed = U.buckets(keys, lg)
    full = occ == 4
    figures = (int(passed.sum()), int(full.sum()), int((full & ~passed).sum()), U.longest_chain(passed))
    assert figures == ((5, 20, 15, 1) if shift else (22, 108, 86, 2)), figures
    assert not (passed & ~full).any()
    # a key stored outside its home bucket: a passed bucket passed one on; the case the flag exists for: full, never passed
    assert passed.any() and (full & ~passed).any()
    # the wrap: the five keys of `wrap` share the last bucket, which holds four
    assert (U.home(five, lg) == nb - 1).all() and np.isin(five, keys).all() and passed[nb - 1] and occ[0] >= 1
    ask = [keys, U.one_base_changed(keys, 1), np.random.default_rng(2).integers(0, 1 << 32, 100_000, dtype=np.uint64),
           _absent(keys, lg, np.nonzero(full & ~passed)[0], 64, 3), _absent(keys, lg, np.nonzero(passed)[0], 16, 4),
           _absent(keys, lg, [nb - 1], 8, 5), np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE], np.uint64)]
    changed = np.isin(ask[1], keys)
    assert 0 < int(changed.sum()) < len(keys) // 2          # most are absent, some are a k-mer of another variant
    return lg, np.concatenate(ask).astype(np.uint32)


@pytest.mark.parametrize("shift", [1, 0])
def test_list_probe_equals_probe_and_vs_id(small, monkeypatch, shift):
    lg, ask = _fixture_keys(small, shift)
    want = U.expected(small["comp"], ask)
    assert int((want != U.MISS).sum()) >= len(small["keys"])
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    db = _open(small["prefix"], shift)
    try:
        assert db.list_table_log2() == lg
        for flag in ("1", "0"):
            monkeypatch.setenv("KMAHIP_LTAB_FLAG", flag)
            by_list, via_pos = db.test_list_probe(ask)
            bad = np.nonzero(by_list != via_pos)[0]
            assert len(bad) == 0, (shift, flag, ask[bad[:8]], by_list[bad[:8]], via_pos[bad[:8]])
            assert np.array_equal(by_list, want), (shift, flag)
    finally:
        db.close()


def test_no_list_table_when_switched_off_at_the_open(small, monkeypatch):
    """KMAHIP_SCAN_LTAB=0 at the open: none is built, the memory is not counted, and the hook says so"""
    from kma_amd import binding
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    on, off = _open(small["prefix"], 1), _open(small["prefix"], 1, KMAHIP_SCAN_LTAB="0")
    try:
        assert on.list_table_log2() == 13 and off.list_table_log2() == 0
        assert on.info.hash_bytes == off.info.hash_bytes == (1 << 12) * 32          # (the probe table's, with or without)
        assert on.info.total_bytes - off.info.total_bytes == (1 << 13) * 32
        with pytest.raises(binding.KmaHipError):
            off.test_list_probe(small["keys"][:4])
    finally:
        on.close()
        off.close()


def test_decon_index(tmp_path, monkeypatch):
    """the decon table of a committed fixture (the reference's own index files): its lists may hold the pseudo-template"""
    import decon_util
    fx = decon_util.unpack("m", tmp_path)
    comp = formats.read_comp_b(fx["prefix"] + ".decon.comp.b")
    keys = np.asarray(comp.key_index[:comp.n], np.uint64)
    ask = np.concatenate([keys, U.one_base_changed(keys, 6), np.random.default_rng(7).integers(0, 1 << 32, 100_000, dtype=np.uint64)]).astype(np.uint32)
    want = U.expected(comp, ask)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    db = _open(fx["prefix"], 1, decon=True)
    try:
        assert db.list_table_log2() == U.probe_log2(len(keys)) + 1
        by_list, via_pos = db.test_list_probe(ask)
        assert np.array_equal(by_list, via_pos) and np.array_equal(by_list, want)
    finally:
        db.close()


def test_index_with_32_bit_value_lists(tmp_path, monkeypatch):
    """66 000 templates (the builder of tests/test_variants_gpu.py): DB_size >= 65535, the lists hold 32-bit elements"""
    names, seqs = synth.make_gene_db(16500, 4, 48, 72, 0.05, seed=9)
    prefix = str(tmp_path / "wide")
    formats.write_index(prefix, names, seqs)
    comp = formats.read_comp_b(prefix + ".comp.b")
    assert comp.values.dtype == np.uint32
    keys = np.asarray(comp.key_index[:comp.n], np.uint64)
    ask = np.concatenate([keys, U.one_base_changed(keys, 8), np.random.default_rng(9).integers(0, 1 << 32, 100_000, dtype=np.uint64)]).astype(np.uint32)
    want = U.expected(comp, ask)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    db = _open(prefix, 1)
    try:
        assert db.list_table_log2() == U.probe_log2(len(keys)) + 1
        by_list, via_pos = db.test_list_probe(ask)
        assert np.array_equal(by_list, via_pos) and np.array_equal(by_list, want)
    finally:
        db.close()
