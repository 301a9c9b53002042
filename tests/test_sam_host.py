"""The host side of the SAM writer (no GPU): kmahip_sam_cigar and kmahip_sam_row_host, the checkers of the text the device makes
(makeCigar / samwrite, sam.c:30-211), and the exported symbols."""
import ctypes

import numpy as np
import pytest

from kma_amd import binding

DIGIT_EDGES = (1, 9, 10, 99, 100, 99_999)


def _runs(lengths, classes):
    return np.array([(int(n) << 2) | int(c) for n, c in zip(lengths, classes)], np.uint32)


@pytest.mark.parametrize("clip_start", [0, 7])
@pytest.mark.parametrize("clip_end", [0, 12345])
def test_cigar_equals_cigar_from_runs_at_the_digit_boundaries(clip_start, clip_end):
    # every run length at which the text gets a digit longer, in every class, next to each other
    lengths = [n for n in DIGIT_EDGES for _ in range(4)]
    classes = [c for _ in DIGIT_EDGES for c in range(4)]
    runs = _runs(lengths, classes)
    want = binding.cigar_from_runs(runs, clip_start, clip_end)
    assert binding.sam_cigar(runs, clip_start, clip_end) == want
    assert "99999=" in want and "1X" in want and "10I" in want and "100D" in want
    # one run at a time
    for n in DIGIT_EDGES:
        for c in range(4):
            r = _runs([n], [c])
            assert binding.sam_cigar(r, clip_start, clip_end) == binding.cigar_from_runs(r, clip_start, clip_end)


def test_cigar_of_an_empty_run_list():
    none = np.zeros(0, np.uint32)
    assert binding.sam_cigar(none) == binding.cigar_from_runs(none) == ""
    assert binding.sam_cigar(none, 5, 0) == binding.cigar_from_runs(none, 5, 0) == "5S"
    assert binding.sam_cigar(none, 0, 9) == "9S"
    assert binding.sam_cigar(none, 10, 100) == "10S100S"


def test_cigar_capacity():
    runs = _runs([10, 1, 99_999], [0, 1, 0])
    want = binding.cigar_from_runs(runs, 3, 4)          # 3S10=1X99999=4S: 15 characters
    assert len(want) == 15
    assert binding.sam_cigar(runs, 3, 4, cap=16) == want          # (the text and its terminator)
    for cap in (15, 14, 2, 1):
        with pytest.raises(binding.KmaHipError) as e:
            binding.sam_cigar(runs, 3, 4, cap=cap)
        assert "error -6" in str(e.value)          # KMAHIP_EOVERFLOW


def test_row_host_against_a_row_written_out():
    runs = _runs([20, 1, 3, 99, 2, 100], [0, 1, 0, 0, 3, 0])
    # QNAME ends at the header's first TAB; mapQ 300 prints as 254; a negative AS keeps its sign
    row = binding.sam_row_host(b"read7 extra\tBC:Z:ACGT\tmore", 16, b"geneA variant 2", 101, 300, runs, 4, 0, 222, "ACGTNACGT", 3, -12)
    assert row == b"read7 extra\t16\tgeneA variant 2\t101\t254\t4S20=1X3=99=2D100=\t*\t0\t222\tACGTNACGT\t*\tET:i:3\tAS:i:-12\n"
    # an unaligned record: no template, no CIGAR
    row = binding.sam_row_host(b"r1", 20, None, 0, 0, None, 0, 0, 0, "TTGCA", 0, 0)
    assert row == b"r1\t20\t*\t0\t0\t*\t*\t0\t0\tTTGCA\t*\tET:i:0\tAS:i:0\n"
    # filed but not aligned: the template's name, CIGAR "*"
    row = binding.sam_row_host(b"r2\t", 4, b"t9", 0, 0, None, 0, 0, 0, "A", 2, 0)
    assert row == b"r2\t4\tt9\t0\t0\t*\t*\t0\t0\tA\t*\tET:i:2\tAS:i:0\n"
    with pytest.raises(binding.KmaHipError) as e:
        binding.sam_row_host(b"r1", 20, None, 0, 0, None, 0, 0, 0, "TTGCA", 0, 0, cap=10)
    assert "error -6" in str(e.value)


def test_sam_symbols_are_exported():
    lib = ctypes.CDLL(binding.LIB_PATH)
    for s in ("kmahip_sam_cigar", "kmahip_sam_row_host", "kmahip_sam_header", "kmahip_sam_write", "kmahip_session_set_sam",
              "kmahip_ws_set_trace_drops", "kmahip_version"):
        assert hasattr(lib, s), s
    assert binding.lib().kmahip_version().decode().count(".") == 2
