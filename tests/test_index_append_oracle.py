"""The restatement of `kma index -t_db` in tests/index_append_util.py against every file of tests/golden/index_append/ the reference
wrote: the old index expanded into pairs, the new templates' k-mers (plain windows, or sparse ones through sparse_index_util.windows)
merged in under the ids from the old DB_size on, and with -deCon the pseudo-template behind the lists of the marked k-mers. What
passes here is what the device is compared with in test_index_append_gpu.py. Integers and bytes only: no tolerance. No GPU."""
import numpy as np
import pytest

import index_append_util as iau
import sparse_index_util as siu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("index_append_oracle")


@pytest.fixture(scope="module")
def old(tmp):
    return {name: iau.unpack(name, tmp) for name in iau.OLD}


@pytest.fixture(scope="module")
def want(tmp):
    return {name: iau.unpack(name, tmp) for name in iau.RECORDED}


@pytest.mark.parametrize("name", list(iau.OLD) + list(iau.RECORDED))
def test_expand_holds_the_pairs_of_the_mapping(name, old, want):
    prefix = old.get(name) or want[name]
    c = iau.Comp(prefix + ".comp.b")
    pairs = iau.expand(prefix + ".comp.b")
    assert pairs.dtype == np.uint64 and np.all(pairs[1:] > pairs[:-1])
    assert len(pairs) == sum(len(ids) for ids in c.mapping().values())
    back = {}
    for x in pairs.tolist():
        back.setdefault(x >> 32, []).append(x & 0xFFFFFFFF)
    assert {km: tuple(ids) for km, ids in back.items()} == c.mapping()
    ids = pairs & np.uint64(0xFFFFFFFF)
    assert int(ids.min()) >= 1 and int(ids.max()) == c.DB_size - 1


@pytest.mark.parametrize("case", list(iau.CASES))
def test_the_restatement_gives_the_recorded_files(case, old, want, tmp):
    """(several appends in a row are restated as one: the rule has no state between them but the files)"""
    d = iau.CASES[case]
    paths = [iau.fasta(x) for step in d["steps"] for x in step]
    got = iau.Appended(old[d["old"]], paths, decon=[iau.fasta("c")] if d.get("decon") else ())
    ref = want.get(d["want"]) or old[d["want"]]
    wd = iau.unpack_decon(d["want_decon"], tmp) if d.get("want_decon") else None
    iau.held_to(got, ref, wd)
    if paths:
        assert got.skipped == ["b_shorter_than_k"] and got.DB_size == iau.Comp(old[d["old"]] + ".comp.b").DB_size + 11
        assert "b_three_leading_n B3" in got.names


def test_the_fixture_holds_what_it_is_made_for(old, want):
    a16, k16 = iau.Comp(old["A_k16"] + ".comp.b"), iau.Comp(want["k16"] + ".comp.b")
    names = open(want["k16"] + ".name").read().split("\n")[:-1]
    fam = tuple(i + 1 for i, n in enumerate(names) if n.startswith("a_family_"))
    bid = names.index("b_shares_60_of_the_family_segment") + 1
    assert [x for x in a16.stored_lists() if x[:5] == fam] == [fam]
    assert sorted(x for x in k16.stored_lists() if x[:5] == fam) == [fam, fam + (bid,)]
    assert iau.Comp(old["A_k10"] + ".comp.b").mega and not iau.Comp(old["A_k12"] + ".comp.b").mega
    # an N inside a template: its k-mers are not those of the N-as-A sequence .seq.b holds
    lens = np.fromfile(old["A_k16"] + ".length.b", np.uint32)[2:]
    words = np.fromfile(old["A_k16"] + ".seq.b", np.uint64)
    o, from_seq = 0, set()
    for L in lens.tolist():
        s = "".join("ACGT"[(int(words[o + (i >> 5)]) >> (62 - 2 * (i & 31))) & 3] for i in range(L))
        from_seq.update(siu.encode(km) for km in iau.plain_kmers(s, 16))
        o += (L >> 5) + 1
    assert from_seq > set(a16.mapping()) and len(from_seq) - a16.n > 30
    sp = iau.Comp(old["A_TG"] + ".comp.b")
    assert (sp.prefix_len, sp.prefix) == (2, siu.encode("TG")) and (iau.Comp(old["A_none"] + ".comp.b").prefix_len, iau.Comp(old["A_none"] + ".comp.b").prefix) == (0, 1)


def test_cli_lines_are_recorded():
    assert [(a, s) for a, s, _ in iau.cli_lines()] == [(a, 255 if "-t_db" in a else 0) for a in iau.CLI_CASES]
