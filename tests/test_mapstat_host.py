"""The formatters of the extended-features file (`<out>.mapstat`), no GPU: kmahip_mapstat_line against a Python %-format of the same
tuple (printExtendedFeatures, ef.c:129-136), kmahip_mapstat_header's fixed lines (initExtendedFeatures, ef.c:30-46), and the rule that
a row is written exactly where kmahip_res_line writes one (runkma.c:814-829)."""
import re

import pytest

from kma_amd import binding

HEADER_COLS = ("# refSequence\treadCount\tfragmentCount\tmapScoreSum\trefCoveredPositions\trefConsensusSum\tbpTotal\tdepthVariance\t"
               "nucHighDepthVariance\tdepthMax\tsnpSum\tinsertSum\tdeletionSum\treadCountAln\tfragmentCountAln")


def _row(t_len=1000, score=12345):
    return binding.ResRow(7, t_len, score, 3, 1, 12.5, 1e-5)


def _want(name, m, cover, aln_len, depth):
    return "%s\t%u\t%u\t%u\t%u\t%u\t%u\t%f\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n" % (
        name, m.read_count, m.fragment_count, m.score_sum, aln_len, cover, depth, m.var, m.nuc_high_var, m.max_depth, m.snp_sum, m.insert_sum,
        m.deletion_sum, m.read_count_aln, m.fragment_count_aln)


CASES = [
    # a variance that needs all six decimals; sums above 2^32
    (binding.MapstatRow(291, 291, 38230, 608.500223, 0, 92, 893, 396, 393, 291, 291), 733, 733, 43647),
    (binding.MapstatRow(4000000000, 2000000001, (1 << 40) + 17, 1277.385, 84, 65535 * 6, (1 << 33) + 1, (1 << 35) + 2, (1 << 34) + 3, 3999999999, 2000000000),
     998, 1000, (1 << 36) + 5),
    (binding.MapstatRow(1, 1, 150, 0.000001, 0, 1, 0, 0, 0, 1, 1), 150, 150, 150),
    (binding.MapstatRow(12, 12, 1788, 35.8899894444, 0, 12, 1, 2, 1, 12, 12), 151, 151, 1799),
    (binding.MapstatRow(5, 5, 700, 123456789.123456, 3, 70000, 9, 9, 9, 5, 5), 900, 950, 123456),
]


@pytest.mark.parametrize("m,cover,aln_len,depth", CASES, ids=[str(i) for i in range(len(CASES))])
def test_line_equals_the_reference_format(m, cover, aln_len, depth):
    name = "tmpl0 extended features"
    got = binding.KmaHipDB.mapstat_line(name, _row(), cover, aln_len, depth, m)
    assert got == _want(name, m, cover, aln_len, depth)
    assert len(got.split("\t")) == 15 and got.endswith("\n")


def test_no_row_where_res_has_none():
    """the gates of runkma.c:814: nothing covered, identity below -ID, depth below -md -- and a row in both files otherwise"""
    m = CASES[0][0]
    row = _row()
    for cover, aln_len, depth, ID_t, Depth_t in ((0, 10, 100, 1.0, 0.0), (500, 600, 6000, 99.5, 0.0), (900, 900, 4000, 1.0, 5.0), (900, 900, 9000, 1.0, 5.0),
                                                 (995, 995, 9000, 99.5, 0.0), (1, 1, 1, 1e-300, 0.0)):
        res = binding.KmaHipDB.res_line("x", row, cover, aln_len, depth, ID_t, Depth_t)
        got = binding.KmaHipDB.mapstat_line("x", row, cover, aln_len, depth, m, ID_t, Depth_t)
        assert (res is None) == (got is None), (cover, aln_len, depth, ID_t, Depth_t)
    assert binding.KmaHipDB.mapstat_line("x", row, 0, 10, 100, m) is None
    assert binding.KmaHipDB.mapstat_line("x", row, 900, 900, 9000, m) is not None


def test_header_lines():
    raw = binding.KmaHipDB.mapstat_header("/some/folder/db_name", 1957, "kmahip_map -i reads.fq -ef")
    lines = raw.decode().split("\n")
    assert lines[-1] == "" and len(lines) == 8
    assert lines[0] == "## method\tKMA"
    assert lines[1] == "## version\t1.5.1"
    assert lines[2] == "## database\tdb_name"
    assert lines[3] == "## fragmentCount\t1957"
    assert re.fullmatch(r"## date\t\d{4}-\d{2}-\d{2}", lines[4])
    assert lines[5] == "## command\tkmahip_map -i reads.fq -ef"
    assert lines[6] == HEADER_COLS
    # no folder in the name; a count above 2^31; no command line
    raw = binding.KmaHipDB.mapstat_header("db", 3000000000, None).decode().split("\n")
    assert raw[2] == "## database\tdb" and raw[3] == "## fragmentCount\t3000000000" and raw[5] == "## command\t"
