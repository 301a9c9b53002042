"""The committed fixtures of decontamination (tests/golden/decon, make_golden_decon.py) hold what the GPU tests need them to hold: the
reference's own taps show records gone and a kept record reordered, the pseudo-template is in the decon table and in no tap. No GPU."""
import os

import numpy as np
import pytest

import decon_util
from kma_amd import formats


@pytest.fixture(scope="module")
def m_taps():
    return {w: decon_util.tap("m", w) for w in ("s2_plain", "s2_decon", "s2_decon_p08")}


def coverage(plain, decon):
    """(records of the plain tap that the decon tap lacks, kept records whose templates are the same set in another order)"""
    by = {r["hdr"]: r for r in plain}
    assert len(by) == len(plain) and all(r["hdr"] in by for r in decon)
    gone = len(plain) - len(decon)
    reordered = [r["hdr"] for r in decon if sorted(r["T"].tolist()) == sorted(by[r["hdr"]]["T"].tolist()) and r["T"].tolist() != by[r["hdr"]]["T"].tolist()]
    return gone, reordered


def test_mosaic_taps_hold_the_coverage_conditions(m_taps):
    gone, reordered = coverage(m_taps["s2_plain"], m_taps["s2_decon"])
    assert gone * 10 >= len(m_taps["s2_plain"]), (gone, len(m_taps["s2_plain"]))
    assert len(reordered) >= 1
    # the proximity tap keeps longer lists than the plain decon tap
    by = {r["hdr"]: r for r in m_taps["s2_decon"]}
    assert sum(len(r["T"]) > len(by[r["hdr"]]["T"]) for r in m_taps["s2_decon_p08"] if r["hdr"] in by) > 50


@pytest.mark.parametrize("name,taps", [("m", ["s2_decon", "s2_decon_p08", "pe_s2_decon_p", "pe_s2_decon_u", "pe_s2_decon_f"]), ("w", ["s2_decon"])])
def test_no_tap_holds_the_pseudo_template(tmp_path, name, taps):
    g = decon_util.unpack(name, tmp_path)
    D = int(formats.read_comp_b(g["prefix"] + ".decon.comp.b").DB_size)
    for w in taps:
        recs = decon_util.tap(name, w)
        assert len(recs) > 100
        assert all(D not in np.abs(r["T"]) for r in recs), w


def test_paired_taps_lose_records_under_decon():
    for tag in "puf":
        plain, decon = decon_util.tap("m", "pe_s2_plain_" + tag), decon_util.tap("m", "pe_s2_decon_" + tag)
        assert len(decon) * 10 <= len(plain) * 9, (tag, len(plain), len(decon))
    # the unmated branch loses one mate and keeps the other (savekmers.c:3509-3510): a header that is there once, twice in the plain tap
    for tag in "pu":
        def count(recs):
            c = {}
            for r in recs:
                c[r["hdr"]] = c.get(r["hdr"], 0) + 1
            return c
        plain, decon = count(decon_util.tap("m", "pe_s2_plain_" + tag)), count(decon_util.tap("m", "pe_s2_decon_" + tag))
        assert sum(1 for h, n in decon.items() if n == 1 and plain[h] == 2) >= 1, tag


@pytest.mark.parametrize("name", ["m", "w", "e"])
def test_decon_table_is_the_plain_table_plus_the_pseudo_template(tmp_path, name):
    g = decon_util.unpack(name, tmp_path)
    plain, decon = formats.read_comp_b(g["prefix"] + ".comp.b"), formats.read_comp_b(g["prefix"] + ".decon.comp.b")
    assert decon.DB_size == plain.DB_size and decon.kmersize == plain.kmersize
    a, b = formats.comp_db_mapping(plain), formats.comp_db_mapping(decon)
    D = int(plain.DB_size)
    assert a.keys() == b.keys()
    marked = [k for k in a if b[k] != a[k]]
    assert all(b[k] == a[k] + (D,) for k in marked)
    assert not any(D in v for v in a.values())
    assert len(marked) >= (30 if name == "e" else 1000), len(marked)


def test_wide_fixture_is_one_family_of_eighty(tmp_path):
    """(every read of it meets most of the 80 variants and the pseudo-template: more candidates than either LDS table of the scan holds;
    that the overflow routes really carried them is asserted on the device's counters, tests/test_decon_gpu.py)"""
    g = decon_util.unpack("w", tmp_path)
    assert formats.read_comp_b(g["prefix"] + ".decon.comp.b").DB_size == 81
    plain, decon = decon_util.tap("w", "s2_plain"), decon_util.tap("w", "s2_decon")
    assert len(plain) > 250 and len(decon) * 10 <= len(plain) * 9
