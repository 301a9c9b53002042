"""The oracle OFF the reference's default thresholds, pinned to the reference on the CPU -- what tests/test_thresholds_gpu.py then holds
the kernels against. The chain finder (oracle/chain.c) against the compiled reference's `-s2` tap at -mct / -mrs / -ml settings that
change which chains a read yields; the mapQ gate (-mq) of the traceback aligner against the MAPQ column of the reference's SAM
fixtures: a read is dropped exactly when its mapQ is below the threshold, and nothing else about it changes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import golden_util
import oracle
import threshold_sets as ts
from kma_amd import formats, synth

_SETS = {"chimeric": (ts.chimeric_set, ts.CHIMERIC_SETTINGS), "noisy": (ts.noisy_set, ts.NOISY_SETTINGS),
         "module": (ts.shared_module_set, ts.MODULE_SETTINGS + [(0.5, 0.3, 60)]),
         "long_genome": (lambda: ts.long_threshold_set("genome")[:3], [ts.CHAIN_DEFAULT] + ts.LONG_SETTINGS),
         "long_genes": (lambda: ts.long_threshold_set("genes")[:3], [ts.CHAIN_DEFAULT] + ts.LONG_SETTINGS)}
_built = {}


def _chain_set(tmp_path_factory, name):
    """index (by the reference's own indexer) + FASTQ of a read set, built once per session"""
    if name not in _built:
        names, seqs, reads = _SETS[name][0]()
        prefix = str(tmp_path_factory.mktemp("thr_" + name) / "db")
        synth.write_fasta(prefix + ".fsa", names, seqs)
        subprocess.run([oracle.REF_KMA, "index", "-i", prefix + ".fsa", "-o", prefix], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        synth.write_fastq(prefix + ".fq", reads)
        _built[name] = (prefix, formats.pack_ragged(reads), oracle.OracleDB(prefix))
    return _built[name]


@pytest.mark.parametrize("name,setting", [(n, s) for n, (_, settings) in _SETS.items() for s in settings])
def test_chain_finder_oracle_equals_reference_binary_off_the_defaults(tmp_path_factory, tmp_path, name, setting):
    """`kma -s2 -mct c -mrs m -ml l` (no -1t1, one thread) and oracle.scan_chain(minlen=l, coverT=c, mrs=m): the same records in the
    same order, on reads that map in pieces (chimeric), whose chains score on either side of mrs x length (noisy) and whose chains
    overlap by 30 ... 110 bases (module: the set on which -mct decides), and on the long reads the device's long-read route is run on
    (long_*: ts.long_threshold_set). Skipped where oracle/_ref/kma has not been built."""
    if not os.path.exists(oracle.REF_KMA):
        pytest.skip("oracle/_ref/kma not built")
    prefix, b, odb = _chain_set(tmp_path_factory, name)
    coverT, mrs, minlen = setting
    tap = subprocess.run([oracle.REF_KMA, "-i", prefix + ".fq", "-o", str(tmp_path / "o"), "-t_db", prefix, "-t", "1", "-s2",
                          "-mct", repr(coverT), "-mrs", repr(mrs), "-ml", str(minlen)], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    want, _ = formats.parse_s2(tap)
    got = ts.flat_chain_records(odb.scan_chain(b, minlen=minlen, coverT=coverT, mrs=mrs))
    flat = [(b"r%d" % i + bytes(2) + struct.pack("<2i", qs, qe), rf, T) for i, rf, er, qs, qe, T in got]
    ref = [(w["hdr"], w["rc_flag"], tuple(int(x) for x in w["T"])) for w in want]
    for x, (a, c) in enumerate(zip(flat, ref)):
        assert a == c, (x, a, c)
    assert len(flat) == len(ref) > (500 if name.startswith("long") else 2000)


def test_read_sets_keep_every_device_setting_biting(tmp_path):
    """what keeps tests/test_thresholds_gpu.py from passing vacuously, checked where no GPU is needed: every chain setting run on the
    device changes the record list of at least 60 reads of its set relative to the default setting"""
    for name, settings in (("noisy", ts.NOISY_GPU_SETTINGS), ("module", ts.MODULE_GPU_SETTINGS)):
        names, seqs, reads = _SETS[name][0]()
        prefix = str(tmp_path / name)
        formats.write_index(prefix, names, seqs)
        b = formats.pack_ragged(reads)
        odb = oracle.OracleDB(prefix)
        base = ts.flat_chain_records(odb.scan_chain(b))
        for coverT, mrs, minlen in settings:
            got = ts.flat_chain_records(odb.scan_chain(b, minlen=minlen, coverT=coverT, mrs=mrs))
            assert ts.reads_differing(got, base, len(reads)) >= 60, (name, coverT, mrs, minlen)
    # the long-read route's set: at least 60 of the reads added behind long_route_set, all of which that route takes
    for kind in ("genome", "genes"):
        names, seqs, reads, first = ts.long_threshold_set(kind)
        assert all(len(r) >= ts.LONG_ROUTE_MIN and int(r.max()) < 4 for r in reads[first:]) and len(reads) - first == ts.N_LONG_ADDED
        prefix = str(tmp_path / kind)
        formats.write_index(prefix, names, seqs)
        b = formats.pack_ragged(reads)
        odb = oracle.OracleDB(prefix)
        base = [r for r in ts.flat_chain_records(odb.scan_chain(b)) if r[0] >= first]
        for coverT, mrs, minlen in ts.LONG_SETTINGS:
            got = [r for r in ts.flat_chain_records(odb.scan_chain(b, minlen=minlen, coverT=coverT, mrs=mrs)) if r[0] >= first]
            assert ts.reads_differing(got, base, len(reads)) >= 60, (kind, coverT, mrs, minlen)


# ---- the mapQ gate against the MAPQ column of the reference's SAM fixtures ------------------------------------------------------------
MQ = (1, 150, 185)      # near the 0, 15 and 50 % points of the `se` fixture's mapQ distribution


def _filed_reads(g):
    """(header, read oriented like its template, template) of every read ConClave filed under a template the reference assembles"""
    from test_oracle_golden import _oracle_conclave_se
    res, cc, st, tlen = _oracle_conclave_se(g)
    out = []
    for i, r in enumerate(g["s1"]):
        tt = int(cc["tmpl"][i])
        if tt == 0 or not st["significant"][abs(tt)]:
            continue
        read = g["reads"][i]
        if int(res["out_flag"][i]) & 16:
            read = synth.revcomp_codes(read)
        if tt < 0:
            read = synth.revcomp_codes(read)
        out.append((r["hdr"].rstrip(b"\0").decode(), read, abs(tt)))
    return out


def _gate_case(g, name):
    sam = golden_util.load_sam(name)
    filed = _filed_reads(g)
    odb = oracle.OracleDB(g["prefix"])
    al = oracle.OracleAligner(odb)
    base = [al.align_trace(read, t) for _, read, t in filed]
    assert sum(o is not None for o in base) == len(sam)
    dropped = {}
    for m in MQ:
        alm = oracle.OracleAligner(odb, mq=m)
        dropped[m] = 0
        for (hd, read, t), o in zip(filed, base):
            got = alm.align_trace(read, t)
            if o is None or sam[hd][0][3] < m:
                assert got is None, (hd, m)
                dropped[m] += o is not None
            else:
                assert got == o, (hd, m)
    return dropped, len(sam)


def test_oracle_mapq_gate_drops_exactly_the_reads_below_it(golden_se):
    dropped, n = _gate_case(golden_se, "se")
    assert dropped[1] < 0.05 * n < dropped[150] < 0.3 * n < dropped[185] < 0.7 * n, (dropped, n)


def test_oracle_mapq_gate_drops_exactly_the_reads_below_it_long_reads(golden_long):
    _gate_case(golden_long, "long")


def test_oracle_mapq_gate_drops_exactly_the_reads_below_it_mt1(tmp_path):
    """`-Mt1 1`: anker_rc's strand, KMA() and the read filter per raw read (orc_align_trace_mt1)"""
    g = golden_util.load_mt1(tmp_path / "mt1")
    sam = golden_util.load_sam("mt1")
    odb = oracle.OracleDB(g["prefix"])
    al = oracle.OracleAligner(odb)
    base = [al.align_trace_mt1(rd, 1) for rd in g["reads"]]
    for m in MQ:
        alm = oracle.OracleAligner(odb, mq=m)
        for nm, rd, (o, is_rc, _) in zip(g["names"], g["reads"], base):
            got, got_rc, _ = alm.align_trace_mt1(rd, 1)
            if o is None or sam[nm][0][3] < m:
                assert got is None, (nm, m)
            else:
                assert got == o and got_rc == is_rc, (nm, m)
