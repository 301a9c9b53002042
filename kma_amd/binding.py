"""ctypes binding of libkmahip.so (include/kmahip.h) -- the only way Python
reaches the HIP path.  There is no CPU fallback: if the shared library is not
built (python -c 'import __graft_entry__ as g; g.build()') import fails loudly.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KMAHIP_LIB") or os.path.join(_HERE, "libkmahip.so")


class Rewards(C.Structure):
    _fields_ = [("M", C.c_int32), ("MM", C.c_int32), ("U", C.c_int32), ("W1", C.c_int32),
                ("Wl", C.c_int32), ("Mn", C.c_int32), ("PE", C.c_int32), ("d", (C.c_int32 * 5) * 5)]


class Params(C.Structure):
    _fields_ = [("rw", Rewards), ("exhaustive", C.c_int32), ("minlen", C.c_int32), ("mq", C.c_int32),
                ("scoreT", C.c_double), ("mrc", C.c_double), ("minFrac", C.c_double), ("ts", C.c_int32), ("apm", C.c_int32),
                ("ca", C.c_int32)]


class DBInfo(C.Structure):
    _fields_ = [("DB_size", C.c_uint32), ("kmersize", C.c_uint32), ("n_kmers", C.c_uint64),
                ("n_values", C.c_uint64), ("hash_bytes", C.c_uint64), ("total_bytes", C.c_uint64),
                ("tseq_words", C.c_uint64)]


class Reads(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("seq", C.c_void_p), ("seq_off", C.c_void_p), ("len", C.c_void_p),
                ("N", C.c_void_p), ("N_off", C.c_void_p), ("seq_words", C.c_int64), ("N_total", C.c_int64),
                ("max_len", C.c_int32), ("q_start", C.c_void_p), ("q_end", C.c_void_p)]


class Cands(C.Structure):
    _fields_ = [("rc_flag", C.c_void_p), ("flag", C.c_void_p), ("T_off", C.c_void_p), ("T", C.c_void_p),
                ("T_cap", C.c_int64)]


class Hits(C.Structure):
    _fields_ = [("n_hits", C.c_void_p), ("best_score", C.c_void_p), ("flag", C.c_void_p), ("tmpl", C.c_void_p),
                ("score", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p),
                ("alignment_scores", C.c_void_p), ("uniq_alignment_scores", C.c_void_p), ("rc", C.c_void_p)]


class PeRecs(C.Structure):
    _fields_ = [("mate", C.c_void_p), ("rc", C.c_void_p), ("rc_flag", C.c_void_p), ("flag", C.c_void_p),
                ("R_off", C.c_void_p), ("T", C.c_void_p), ("T_cap", C.c_int64)]


class Conclave(C.Structure):
    _fields_ = [("tmpl", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p), ("w_scores", C.c_void_p),
                ("fragment_counts", C.c_void_p), ("read_counts", C.c_void_p), ("depth", C.c_void_p)]


class ResRow(C.Structure):
    _fields_ = [("template_id", C.c_int32), ("template_length", C.c_int32), ("score", C.c_uint64), ("expected", C.c_uint32),
                ("significant", C.c_int32), ("q_value", C.c_double), ("p_value", C.c_double)]


class Traces(C.Structure):
    _fields_ = [("stats", C.c_void_p), ("ops_off", C.c_void_p), ("n_ops", C.c_void_p), ("ops", C.c_void_p), ("ops_cap", C.c_int64)]


class Assembly(C.Structure):
    _fields_ = [("cover", C.c_void_p), ("aln_len", C.c_void_p), ("depth", C.c_void_p), ("asm_len", C.c_void_p),
                ("consensus", C.c_void_p), ("consensus_off", C.c_void_p), ("consensus_cap", C.c_int64), ("consensus_used", C.c_int64)]


class AssemblyEf(C.Structure):
    _fields_ = [("depth_var", C.c_void_p), ("snp_sum", C.c_void_p), ("insert_sum", C.c_void_p), ("deletion_sum", C.c_void_p), ("max_depth", C.c_void_p),
                ("nuc_high_var", C.c_void_p), ("score_sum", C.c_void_p), ("read_count_aln", C.c_void_p), ("fragment_count_aln", C.c_void_p), ("var", C.c_void_p)]


class MapstatRow(C.Structure):
    _fields_ = [("read_count", C.c_uint32), ("fragment_count", C.c_uint32), ("score_sum", C.c_uint64), ("var", C.c_double), ("nuc_high_var", C.c_uint32),
                ("max_depth", C.c_uint32), ("snp_sum", C.c_uint64), ("insert_sum", C.c_uint64), ("deletion_sum", C.c_uint64), ("read_count_aln", C.c_uint32),
                ("fragment_count_aln", C.c_uint32)]


class VcfRec(C.Structure):
    _fields_ = [("tmpl", C.c_int32), ("pos", C.c_int32), ("ref", C.c_uint8), ("call", C.c_uint8), ("reserved", C.c_uint16), ("best_score", C.c_int32),
                ("counts", C.c_uint32 * 6)]


VCF_REC = np.dtype([("tmpl", np.int32), ("pos", np.int32), ("ref", np.uint8), ("call", np.uint8), ("reserved", np.uint16), ("best_score", np.int32),
                    ("counts", np.uint32, 6)])
TEXT_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)


class Trim(C.Structure):
    _fields_ = [("min_phred", C.c_int32), ("min_q", C.c_int32), ("hardmask_q", C.c_int32), ("min_len", C.c_int32),
                ("max_len", C.c_int32)]


class ReadBatchC(C.Structure):
    _fields_ = [("reads", Reads), ("names", C.c_void_p), ("name_off", C.c_void_p), ("pair", C.c_void_p), ("records", C.c_int64)]


class ChainParams(C.Structure):
    _fields_ = [("minlen", C.c_int32), ("pad_", C.c_int32), ("coverT", C.c_double), ("mrs", C.c_double)]


class ChainRecs(C.Structure):
    _fields_ = [("rec_cap", C.c_int64), ("T_cap", C.c_int64), ("n_recs", C.c_int64), ("n_T", C.c_int64), ("read", C.c_void_p),
                ("rc_flag", C.c_void_p), ("emit_rc", C.c_void_p), ("q_start", C.c_void_p), ("q_end", C.c_void_p), ("T_off", C.c_void_p),
                ("T", C.c_void_p)]


class AssembleOpts(C.Structure):
    _fields_ = [("max_frag", C.c_int64), ("evalue", C.c_double), ("bcd", C.c_int32), ("order", C.c_int32), ("caller", C.c_int32), ("sig90", C.c_int32),
                ("frag_rank", C.c_void_p), ("support", C.c_double)]


class Run(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("rows_cap", C.c_int64), ("n_rows", C.c_int64), ("assembly", Assembly),
                ("tmpl", C.c_void_p), ("n_hits", C.c_void_p), ("rc", C.c_void_p), ("trace_stats", C.c_void_p), ("ms", C.c_double * 6),
                ("caller", C.c_int32), ("sig90", C.c_int32), ("support", C.c_double)]


class ScanStats(C.Structure):
    _fields_ = [("probes", C.c_uint64), ("value_elems", C.c_uint64), ("active_strands", C.c_uint64),
                ("hash_probes", C.c_uint64), ("prefilter_probes", C.c_uint64)]


class AlignStats(C.Structure):
    _fields_ = [("lookups", C.c_uint64), ("mem_bases", C.c_uint64), ("dp_cells", C.c_uint64), ("tasks", C.c_uint64)]


class TraceStats(C.Structure):
    _fields_ = [("problems", C.c_uint64), ("dp_cells", C.c_uint64), ("mems", C.c_uint64), ("reads", C.c_uint64)]


class TraceDrops(C.Structure):
    _fields_ = [("stats", C.c_void_p), ("ops_off", C.c_void_p), ("n_ops", C.c_void_p)]


class ShardOpts(C.Structure):
    _fields_ = [("evalue", C.c_double), ("bcd", C.c_int32), ("caller", C.c_int32), ("sig90", C.c_int32), ("max_frag", C.c_int64),
                ("ID_t", C.c_double), ("Depth_t", C.c_double), ("support", C.c_double), ("ref_fsa", C.c_int32), ("write_aln", C.c_int32),
                ("vcf_support_own", C.c_int32), ("pad_", C.c_int32), ("vcf_support", C.c_double)]


class KmaHipError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if "KMAHIP_LIB" not in os.environ:
            # build on demand, also when a source is newer than the library (the .so is git-ignored but travels to the GPU box:
            # a stale one must never be what gets tested or benchmarked). `make -q` costs milliseconds when everything is current;
            # there is no other implementation to fall back to
            import shutil
            import subprocess
            csrc = os.path.join(_HERE, "csrc")
            stale = not os.path.exists(LIB_PATH)
            if not stale and shutil.which("make"):
                stale = subprocess.call(["make", "-q", "-C", csrc], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0
            if stale:
                # several ranks import this at the same moment (bench.py --gpus N, the dist tests): one builds, the others wait
                # for the lock and find the library current
                import fcntl
                with open(os.path.join(csrc, ".build.lock"), "w") as lock:
                    fcntl.flock(lock, fcntl.LOCK_EX)
                    try:
                        if not os.path.exists(LIB_PATH) or subprocess.call(["make", "-q", "-C", csrc], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0:
                            subprocess.check_call(["make", "-C", csrc, "-j4"], stdout=subprocess.DEVNULL)
                    except (OSError, subprocess.CalledProcessError) as e:
                        raise KmaHipError(f"{LIB_PATH} is missing or older than its sources and building it failed ({e}): run __graft_entry__.build()")
                    finally:
                        fcntl.flock(lock, fcntl.LOCK_UN)
        if not os.path.exists(LIB_PATH):
            raise KmaHipError(f"{LIB_PATH} is not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        L = C.CDLL(LIB_PATH)
        L.kmahip_last_error.restype = C.c_char_p
        L.kmahip_default_params.argtypes = [C.POINTER(Params)]
        L.kmahip_default_params.restype = None
        L.kmahip_init.argtypes = [C.c_int]
        L.kmahip_db_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        if hasattr(L, "kmahip_db_open_decon"):          # (KMAHIP_LIB may name an older library, for side-by-side timing)
            L.kmahip_db_open_decon.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
            L.kmahip_db_is_decon.argtypes = [C.c_void_p]
        L.kmahip_db_close.argtypes = [C.c_void_p]
        L.kmahip_db_close.restype = None
        L.kmahip_db_get_info.argtypes = [C.c_void_p, C.POINTER(DBInfo)]
        L.kmahip_ws_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.kmahip_ws_destroy.argtypes = [C.c_void_p]
        L.kmahip_ws_destroy.restype = None
        L.kmahip_scan_se.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(Cands)]
        L.kmahip_scan_se_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(Cands), C.c_void_p]
        L.kmahip_ws_status.argtypes = [C.c_void_p, C.c_void_p]
        L.kmahip_scan_set_stats.argtypes = [C.c_void_p, C.c_int]
        L.kmahip_scan_get_stats.argtypes = [C.c_void_p, C.POINTER(ScanStats), C.c_void_p]
        if hasattr(L, "kmahip_ws_scan_routes"):          # (KMAHIP_LIB may name an older library, for side-by-side timing)
            L.kmahip_ws_scan_routes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        if hasattr(L, "kmahip_ws_scan_diag_replaced"):
            L.kmahip_ws_scan_diag_replaced.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        if hasattr(L, "kmahip_ws_align_queue_counts"):
            L.kmahip_ws_align_queue_counts.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.kmahip_ws_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.kmahip_ws_get_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.kmahip_align_se_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Cands), C.POINTER(Params),
                                          C.POINTER(Hits), C.c_void_p]
        L.kmahip_align_get_stats.argtypes = [C.c_void_p, C.POINTER(AlignStats), C.c_void_p]
        L.kmahip_scan_pe.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(PeRecs)]
        L.kmahip_scan_pe_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(PeRecs), C.c_void_p]
        L.kmahip_align_pe_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(PeRecs), C.POINTER(Params), C.POINTER(Hits),
                                          C.c_void_p, C.c_void_p]
        L.kmahip_scan_pe_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(PeRecs), C.c_void_p]
        L.kmahip_map_pe.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(PeRecs),
                                    C.POINTER(Hits), C.c_void_p]
        L.kmahip_map_se.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(Cands), C.POINTER(Hits)]
        L.kmahip_conclave_se.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Cands), C.POINTER(Hits), C.POINTER(Conclave)]
        L.kmahip_conclave_pe.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(PeRecs), C.POINTER(Hits), C.c_void_p,
                                         C.POINTER(Conclave)]
        L.kmahip_conclave_se_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Cands), C.POINTER(Hits),
                                             C.POINTER(Conclave), C.c_void_p]
        L.kmahip_conclave2_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Hits),
                                               C.c_double, C.c_double, C.POINTER(Conclave)]
        L.kmahip_set_conclave_version.argtypes = [C.c_int]
        L.kmahip_conclave_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Hits),
                                              C.POINTER(Conclave)]
        L.kmahip_align_trace.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params),
                                         C.POINTER(Traces), C.POINTER(C.c_int64)]
        L.kmahip_align_trace_mt1.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.c_int32, C.c_int, C.POINTER(Params), C.POINTER(Traces),
                                             C.c_void_p, C.POINTER(C.c_int64)]
        L.kmahip_assemble.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.POINTER(Traces), C.c_int64,
                                      C.c_int, C.c_double, C.POINTER(Assembly)]
        L.kmahip_res_line.argtypes = [C.c_char_p, C.POINTER(ResRow), C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                      C.c_char_p, C.c_int64]
        L.kmahip_res_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.kmahip_frag_write.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.kmahip_run_se.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.c_double, C.c_int, C.c_int64, C.POINTER(Run)]
        L.kmahip_run_pe.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ReadBatchC), C.POINTER(Params), C.c_double, C.c_int, C.c_int64, C.c_char_p,
                                    C.POINTER(Run)]
        L.kmahip_run_mt1.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.c_int32, C.c_int, C.POINTER(Params), C.POINTER(AssembleOpts), C.POINTER(Run)]
        L.kmahip_ws_set_pe_chain.argtypes = [C.c_void_p, C.POINTER(ChainParams)]
        L.kmahip_assemble2.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.POINTER(Traces), C.POINTER(AssembleOpts),
                                       C.POINTER(Assembly)]
        L.kmahip_frag_write3.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.kmahip_frag_write2.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_int, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.kmahip_trace_get_stats.argtypes = [C.c_void_p, C.POINTER(TraceStats)]
        if hasattr(L, "kmahip_trace_get_class_counts"):          # (KMAHIP_LIB may name an older library, for side-by-side timing)
            L.kmahip_trace_get_class_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        if hasattr(L, "kmahip_chain_get_route_counts"):
            L.kmahip_chain_get_route_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.kmahip_trim_default.argtypes = [C.POINTER(Trim)]
        L.kmahip_trim_default.restype = None
        L.kmahip_ingest_open.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Trim), C.POINTER(C.c_void_p)]
        L.kmahip_ingest_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(ReadBatchC)]
        L.kmahip_ingest_phred_scale.argtypes = [C.c_void_p]
        L.kmahip_ingest_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.kmahip_ingest_counts.restype = None
        L.kmahip_ingest_close.argtypes = [C.c_void_p]
        L.kmahip_ingest_status.argtypes = [C.c_void_p]
        L.kmahip_ingest_set_batch_bases.argtypes = [C.c_void_p, C.c_int64]
        L.kmahip_ingest_close.restype = None
        L.kmahip_ingest_dev_open.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Trim), C.POINTER(C.c_void_p)]
        L.kmahip_ingest_dev_next.argtypes = [C.c_void_p, C.c_int64, C.POINTER(ReadBatchC)]
        L.kmahip_ingest_dev_status.argtypes = [C.c_void_p]
        L.kmahip_ingest_dev_phred_scale.argtypes = [C.c_void_p]
        L.kmahip_ingest_dev_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.kmahip_ingest_dev_counts.restype = None
        L.kmahip_ingest_dev_handed_back.argtypes = [C.c_void_p]
        L.kmahip_ingest_dev_handed_back.restype = C.c_int64
        L.kmahip_ingest_dev_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.kmahip_ingest_dev_timing.restype = None
        L.kmahip_ingest_dev_copy_out.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.kmahip_ingest_dev_close.argtypes = [C.c_void_p]
        L.kmahip_ingest_dev_close.restype = None
        L.kmahip_version.restype = C.c_char_p
        L.kmahip_sam_cigar.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
        L.kmahip_sam_cigar.restype = C.c_int64
        L.kmahip_sam_row_host.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_char_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
        L.kmahip_sam_row_host.restype = C.c_int64
        L.kmahip_sam_header.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
        L.kmahip_sam_write.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(Reads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Traces),
                                       C.POINTER(TraceDrops), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.kmahip_ws_set_trace_drops.argtypes = [C.c_void_p, C.POINTER(TraceDrops)]
        L.kmahip_session_open.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(ShardOpts), C.c_int64, C.POINTER(C.c_void_p)]
        L.kmahip_session_set_sam.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p]
        L.kmahip_session_set_chain.argtypes = [C.c_void_p, C.POINTER(ChainParams)]
        L.kmahip_session_set_mt1.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_char_p]
        L.kmahip_session_set_pe.argtypes = [C.c_void_p]
        L.kmahip_session_close.argtypes = [C.c_void_p]
        L.kmahip_session_close.restype = None
        if hasattr(L, "kmahip_assemble_ef"):          # (KMAHIP_LIB may name an older library, for side-by-side timing)
            L.kmahip_assemble_ef.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(Traces), C.c_void_p, C.POINTER(Params), C.POINTER(Assembly),
                                             C.POINTER(AssemblyEf)]
            L.kmahip_mapstat_header.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int64]
            L.kmahip_mapstat_header.restype = C.c_int64
            L.kmahip_mapstat_line.argtypes = [C.c_char_p, C.POINTER(ResRow), C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.POINTER(MapstatRow),
                                              C.c_char_p, C.c_int64]
            L.kmahip_session_set_ef.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
            L.kmahip_session_set_ef_fragments.argtypes = [C.c_void_p, C.c_int64]
        if hasattr(L, "kmahip_assemble_matrix_dev"):
            L.kmahip_assemble_matrix_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, TEXT_SINK, C.c_void_p]
            L.kmahip_assemble_vcf_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            L.kmahip_vcf_header.argtypes = [C.c_char_p, C.c_char_p, C.c_int64]
            L.kmahip_vcf_header.restype = C.c_int64
            L.kmahip_vcf_line.argtypes = [C.c_char_p, C.POINTER(VcfRec), C.c_double, C.c_double, C.c_int, C.c_int, C.c_char_p, C.c_int64]
            L.kmahip_session_set_matrix.argtypes = [C.c_void_p]
            L.kmahip_session_set_vcf.argtypes = [C.c_void_p, C.c_int, C.c_char_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise KmaHipError(f"kmahip error {rc}: {lib().kmahip_last_error().decode()}")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cigar_from_runs(runs, clip_start=0, clip_end=0):
    """SAM CIGAR (makeCigar, sam.c:30-98) of one read's runs"""
    out = [f"{clip_start}S"] if clip_start else []
    out += [f"{int(x) >> 2}{'=XID'[int(x) & 3]}" for x in runs]
    if clip_end:
        out.append(f"{clip_end}S")
    return "".join(out)


def sam_cigar(runs, clip_start=0, clip_end=0, cap=None):
    """kmahip_sam_cigar (host code): the CIGAR text of one record; KmaHipError (-6) when `cap` bytes do not hold it"""
    r = np.ascontiguousarray(runs, np.uint32)
    cap = int(cap) if cap is not None else 12 * len(r) + 32
    buf = C.create_string_buffer(max(1, cap))
    n = lib().kmahip_sam_cigar(_p(r) if len(r) else None, len(r), int(clip_start), int(clip_end), buf, cap)
    if n < 0:
        _check(int(n))
    return buf.raw[:n].decode()


def sam_row_host(header, flag, rname, pos, mapq, runs, clip_start, clip_end, tlen, seq, et, as_, cap=None):
    """kmahip_sam_row_host (host code): one SAM row from host values -> bytes. rname None = "*", runs None = CIGAR "*"."""
    r = None if runs is None else np.ascontiguousarray(runs, np.uint32)
    header, seq = (x.encode() if isinstance(x, str) else bytes(x) for x in (header, seq))
    rn = None if rname is None else (rname.encode() if isinstance(rname, str) else bytes(rname))
    cap = int(cap) if cap is not None else len(header) + len(seq) + (0 if r is None else 12 * len(r)) + 256 + (len(rn) if rn else 0)
    buf = C.create_string_buffer(max(1, cap))
    # (an empty run list is still a list: a pointer that is not NULL)
    keep = np.zeros(1, np.uint32) if r is not None and not len(r) else r
    n = lib().kmahip_sam_row_host(header, int(flag), rn, int(pos), int(mapq), None if keep is None else _p(keep), 0 if r is None else len(r),
                                  int(clip_start), int(clip_end), int(tlen), seq, int(et), int(as_), buf, cap)
    if n < 0:
        _check(int(n))
    return buf.raw[:n]


def test_mapq(best, second, w):
    """kmahip_test_mapq (a test hook): the device's mapQ function on arrays of (best, second, w) -> uint32 array"""
    b, s, ww = (np.ascontiguousarray(x, np.int32) for x in (best, second, w))
    assert b.shape == s.shape == ww.shape and b.ndim == 1
    out = np.zeros(len(b), np.uint32)
    L = lib()
    L.kmahip_test_mapq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.kmahip_test_mapq.restype = C.c_int
    _check(L.kmahip_test_mapq(_p(b), _p(s), _p(ww), len(b), _p(out)))
    return out


def diag_gap_m_max(rw):
    """kmahip_diag_gap_m_max (host arithmetic): the most mismatches on a link's diagonal up to which stage 3a and the traceback skip the
    DP matrix under the scoring scheme of a Rewards, -1 where they never do"""
    L = lib()
    L.kmahip_diag_gap_m_max.argtypes = [C.POINTER(Rewards)]
    L.kmahip_diag_gap_m_max.restype = C.c_int
    return int(L.kmahip_diag_gap_m_max(C.byref(rw)))


def test_lane_down(values, w):
    """kmahip_test_lane_down (a test hook): what each of a wavefront's 64 lanes receives from the sweep's neighbour move"""
    v = np.ascontiguousarray(values, np.int32)
    assert v.shape == (64,)
    out = np.zeros(64, np.int32)
    L = lib()
    L.kmahip_test_lane_down.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.kmahip_test_lane_down.restype = C.c_int
    _check(L.kmahip_test_lane_down(_p(v), int(w), _p(out)))
    return out


def index_build(fasta_paths, out_prefix, k=16, decon=None, sparse=None, min_len=0, hom_q=1.0, hom_t=1.0, hom_and=False, report=None):
    """kmahip_index_build: the four index files from FASTA file(s) (needs a GPU: the k-mers are sorted on the device).
    decon: contamination FASTA file(s) (`kma index -deCon`) -> kmahip_index_build_decon, which writes <out_prefix>.decon.comp.b too.
    sparse: a prefix such as "TG", or "-" for none (`kma index -Sparse`) -> kmahip_index_build_sparse, the index SparseDB maps against;
    min_len: its -ML (0: the default). A sparse decon index is not built, and -ML belongs to the sparse build alone.
    hom_q, hom_t, hom_and, report: `-hq`, `-ht`, `-and` of a sparse build (kmahip_index_build_sparse_hom) and the file that takes the
    cluster lines the reference prints to standard output; without sparse they have no effect, as in the reference."""
    paths = [os.fsencode(p) for p in ([fasta_paths] if isinstance(fasta_paths, (str, bytes)) else fasta_paths)]
    arr = (C.c_char_p * len(paths))(*paths)
    L = lib()
    if sparse is not None:
        if decon is not None:
            raise ValueError("index_build: sparse with decon is not built")
        L.kmahip_index_build_sparse.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.kmahip_index_build_sparse.restype = C.c_int
        if hom_q == 1.0 and hom_t == 1.0 and not hom_and and report is None:
            _check(L.kmahip_index_build_sparse(arr, len(paths), os.fsencode(out_prefix), int(k), int(k), os.fsencode(sparse), int(min_len)))
            return
        L.kmahip_index_build_sparse_hom.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_double,
                                                    C.c_int, C.c_char_p]
        L.kmahip_index_build_sparse_hom.restype = C.c_int
        _check(L.kmahip_index_build_sparse_hom(arr, len(paths), os.fsencode(out_prefix), int(k), int(k), os.fsencode(sparse), int(min_len), float(hom_q),
                                               float(hom_t), int(bool(hom_and)), None if report is None else os.fsencode(report)))
        return
    if min_len:
        raise ValueError("index_build: min_len (-ML) is built for sparse indexes only")
    if decon is not None:
        dpaths = [os.fsencode(p) for p in ([decon] if isinstance(decon, (str, bytes)) else decon)]
        darr = (C.c_char_p * max(1, len(dpaths)))(*dpaths)
        L.kmahip_index_build_decon.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int]
        L.kmahip_index_build_decon.restype = C.c_int
        _check(L.kmahip_index_build_decon(arr, len(paths), darr, len(dpaths), os.fsencode(out_prefix), int(k)))
        return
    L.kmahip_index_build.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int]
    L.kmahip_index_build.restype = C.c_int
    _check(L.kmahip_index_build(arr, len(paths), os.fsencode(out_prefix), int(k)))


def index_append(db_prefix, fasta_paths=None, out_prefix=None, decon=None):
    """kmahip_index_append (`kma index -t_db`): the templates of fasta_paths behind those of the index db_prefix, as a fresh build of
    all of them would index them; k and the sparse prefix are the index's. out_prefix None: in place. decon: contamination FASTA
    file(s); without fasta_paths only <prefix>.decon.comp.b is written, for the index as it is (needs a GPU)."""
    def arr(x):
        ps = [] if x is None else [os.fsencode(p) for p in ([x] if isinstance(x, (str, bytes)) else x)]
        return (C.c_char_p * max(1, len(ps)))(*ps), len(ps)
    L = lib()
    L.kmahip_index_append.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_char_p]
    L.kmahip_index_append.restype = C.c_int
    (fa, n_fa), (da, n_da) = arr(fasta_paths), arr(decon)
    _check(L.kmahip_index_append(os.fsencode(db_prefix), fa, n_fa, da, n_da, None if out_prefix is None else os.fsencode(out_prefix)))


def index_expand(prefix):
    """the test hook of an append's expansion (kmahip_test_index_expand): the (k-mer << 32 | template) pairs of <prefix>.comp.b as
    the device wrote them, uint64, in the order of the file's k-mers"""
    L = lib()
    L.kmahip_test_index_expand.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.kmahip_test_index_expand.restype = C.c_int
    cap = 1 << 16
    while True:
        out = np.zeros(cap, np.uint64)
        n = C.c_int64(0)
        rc = L.kmahip_test_index_expand(os.fsencode(prefix), _p(out), cap, C.byref(n))
        if rc and n.value > cap:
            cap = n.value
            continue
        _check(rc)
        return out[:n.value].copy()


def index_expand_timing():
    """ms of the count kernel, the scan and the write pass of this process's last expansion (kmahip_test_index_expand_timing)"""
    out = (C.c_double * 3)()
    L = lib()
    L.kmahip_test_index_expand_timing.argtypes = [C.POINTER(C.c_double)]
    _check(L.kmahip_test_index_expand_timing(out))
    return list(out)


def index_hom_rows(fasta_paths, k=16, sparse="-", min_len=0, hom_q=1.0, hom_t=1.0, hom_and=False):
    """the test hook of the homology counts (kmahip_test_index_hom_rows): [n candidate templates, 7] uint32 in file order -- stays, thisKlen,
    max Scores_tot, templateQ, Scores and ulen of the best thisT, templateT (templates by file order, 1 ..; 0: none). No file is written."""
    paths = [os.fsencode(p) for p in ([fasta_paths] if isinstance(fasta_paths, (str, bytes)) else fasta_paths)]
    arr = (C.c_char_p * len(paths))(*paths)
    L = lib()
    L.kmahip_test_index_hom_rows.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64,
                                             C.POINTER(C.c_int64)]
    L.kmahip_test_index_hom_rows.restype = C.c_int
    cap = 1 << 16
    while True:
        out = np.zeros((cap, 7), np.uint32)
        n = C.c_int64(0)
        rc = L.kmahip_test_index_hom_rows(arr, len(paths), int(k), os.fsencode(sparse), int(min_len), float(hom_q), float(hom_t), int(bool(hom_and)), _p(out), cap,
                                          C.byref(n))
        if rc and n.value > cap:
            cap = n.value
            continue
        _check(rc)
        return out[:n.value].copy()


class QCStats(C.Structure):
    _fields_ = [("fragcount", C.c_uint64), ("org_fragcount", C.c_uint64), ("count", C.c_uint64), ("org_count", C.c_uint64),
                ("bpcount", C.c_uint64), ("org_bpcount", C.c_uint64), ("totgc", C.c_uint64), ("totns", C.c_uint64), ("Eeq", C.c_double),
                ("maxlen", C.c_int32), ("qresolution", C.c_int32), ("phred_scale", C.c_int32), ("pad_", C.c_int32),
                ("qdist", C.c_uint32 * 256), ("ldist", C.c_uint32 * 512)]


def _qc_lib():
    L = lib()
    if not getattr(L, "_qc_ready", False):
        L.kmahip_qc_open.argtypes = [C.POINTER(C.c_void_p)]
        L.kmahip_qc_close.argtypes = [C.c_void_p]
        L.kmahip_qc_close.restype = None
        L.kmahip_qc_get.argtypes = [C.c_void_p, C.POINTER(QCStats)]
        L.kmahip_qc_write.argtypes = [C.c_void_p, C.POINTER(Trim), C.c_int, C.c_int, C.c_char_p]
        L.kmahip_ingest_set_qc.argtypes = [C.c_void_p, C.c_void_p]
        L.kmahip_ingest_dev_set_qc.argtypes = [C.c_void_p, C.c_void_p]
        L.kmahip_ingest_set_text.argtypes = [C.c_void_p, C.c_int]
        L.kmahip_ingest_text.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.kmahip_trim_files.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.c_int,
                                        C.POINTER(Trim), C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_int64)]
        L.kmahip_ingest_dev_set_text.argtypes = [C.c_void_p, C.c_int]
        L.kmahip_ingest_dev_text.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L._qc_ready = True
    return L


class QC:
    """The QC report of `kma ... -qc` / `kma trim -qc` (kmahip_qc_*): an accumulator that readers feed while they trim -- Ingest(..., qc=q),
    IngestDev(..., qc=q), several of them one after the other. A reader with one trims by the reference's -qc rule."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(_qc_lib().kmahip_qc_open(C.byref(self._h)))

    def stats(self):
        """-> dict of the counts, sums, the two histograms (numpy), the resolution and the phred scale"""
        s = QCStats()
        _check(_qc_lib().kmahip_qc_get(self._h, C.byref(s)))
        out = {n: getattr(s, n) for n, _ in QCStats._fields_ if n not in ("pad_", "qdist", "ldist")}
        out["qdist"] = np.array(s.qdist, np.uint32)
        out["ldist"] = np.array(s.ldist, np.uint32)
        return out

    def write(self, path, min_phred=20, min_q=0, hardmask_q=0, min_len=16, max_len=2**31 - 1, clip5=0, clip3=0):
        """print_QCstat: the JSON file; the trimming options as they were given, -5p / -3p only to be printed"""
        t = Trim(min_phred, min_q, hardmask_q, min_len, max_len)
        _check(_qc_lib().kmahip_qc_write(self._h, C.byref(t), int(clip5), int(clip3), os.fsencode(path)))

    def close(self):
        if self._h:
            _qc_lib().kmahip_qc_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def trim_files(paths, out_prefix, paired=(), interleaved=(), qc=None, s1dev=False, min_phred=20, min_q=0, hardmask_q=0, min_len=16, max_len=2**31 - 1):
    """`kma trim -i paths -ipe paired -int interleaved -o out_prefix` (kmahip_trim_files): <out_prefix>.fq and, with paired or interleaved
    files, <out_prefix>_int.fq; qc: a QC to feed (its write() makes <out_prefix>.json); s1dev: stage 1 and the text on the device for
    the files its reader covers. -> fragments written, a couple counting once"""
    def arr(xs):
        xs = [os.fsencode(x) for x in xs]
        return (C.c_char_p * max(1, len(xs)))(*xs), len(xs)
    se, n_se = arr(paths)
    pe, n_pe = arr(paired)
    il, n_il = arr(interleaved)
    t = Trim(min_phred, min_q, hardmask_q, min_len, max_len)
    n = C.c_int64()
    _check(_qc_lib().kmahip_trim_files(se, n_se, pe, n_pe, il, n_il, C.byref(t), qc._h if qc is not None else None, 1 if s1dev else 0, os.fsencode(out_prefix), C.byref(n)))
    return n.value


class Ingest:
    """Stage 1 on the host (kmahip_ingest_*): FASTQ / FASTA(.gz) -> trimmed, packed formats.ReadBatch batches, the
    records the reference's run_input / run_input_PE write into the S1 stream, in the same order."""

    def __init__(self, path1, path2=None, min_phred=20, min_q=0, hardmask_q=0, min_len=16, max_len=2**31 - 1, interleaved=False, qc=None, text=False):
        L = lib()
        t = Trim(min_phred, min_q, hardmask_q, min_len, max_len)
        self._h = C.c_void_p()
        if interleaved:          # `-int file`: the records of one file two at a time (run_input_INT)
            if path2:
                raise ValueError("interleaved input is one file")
            L.kmahip_ingest_open_interleaved.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_void_p)]
            _check(L.kmahip_ingest_open_interleaved(os.fsencode(path1), C.byref(t), C.byref(self._h)))
        else:
            _check(L.kmahip_ingest_open(os.fsencode(path1), os.fsencode(path2) if path2 else None, C.byref(t), C.byref(self._h)))
        try:
            if qc is not None:       # trim by the -qc rule and feed the accumulator (kmahip_ingest_set_qc)
                _check(_qc_lib().kmahip_ingest_set_qc(self._h, qc._h))
            if text:                 # the batches also as FASTQ text (kmahip_ingest_set_text): text() after every next()
                _check(_qc_lib().kmahip_ingest_set_text(self._h, 1))
        except Exception:
            self.close()
            raise

    def text(self):
        """-> (single records, couples) of the batch delivered last as FASTQ text (bytes), `kma trim`'s <out>.fq and <out>_int.fq"""
        out = []
        for k in range(2):
            p, n = C.c_void_p(), C.c_int64()
            _check(_qc_lib().kmahip_ingest_text(self._h, k, C.byref(p), C.byref(n)))
            out.append(C.string_at(p, n.value) if n.value else b"")
        return tuple(out)

    @property
    def phred_scale(self):
        return lib().kmahip_ingest_phred_scale(self._h)

    def counts(self):
        a, b = C.c_int64(), C.c_int64()
        lib().kmahip_ingest_counts(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def next(self, max_records=1 << 20):
        """-> (ReadBatch, names list[bytes], pair u8[n]) or None at the end of the input (copies out of the reader's buffers)"""
        from . import formats
        b = ReadBatchC()
        _check(lib().kmahip_ingest_next(self._h, max_records, C.byref(b)))
        n = b.reads.n_reads
        if n == 0:
            return None

        def arr(ptr, dt, m):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(m,)).copy() if m else np.zeros(0, dt)
        batch = formats.ReadBatch(seq=arr(b.reads.seq, C.c_uint64, b.reads.seq_words), seq_off=arr(b.reads.seq_off, C.c_int64, n + 1),
                                  length=arr(b.reads.len, C.c_int32, n), N=arr(b.reads.N, C.c_int32, max(1, b.reads.N_total)),
                                  N_off=arr(b.reads.N_off, C.c_int64, n + 1))
        noff = arr(b.name_off, C.c_int64, n + 1)
        raw = C.string_at(b.names, int(noff[-1]))
        names = [raw[noff[i]:noff[i + 1] - 1] for i in range(n)]
        return batch, names, arr(b.pair, C.c_uint8, n)

    def set_batch_bases(self, max_bases):
        """a batch of next() also closes once it holds about max_bases bases (0: no such bound)"""
        _check(lib().kmahip_ingest_set_batch_bases(self._h, int(max_bases)))

    def status(self):
        """raises when the input broke off behind the records delivered so far (for callers that take everything as one batch)"""
        _check(lib().kmahip_ingest_status(self._h))

    def close(self):
        if self._h:
            lib().kmahip_ingest_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class IngestDev:
    """Stage 1 on the device (kmahip_ingest_dev_*): plain FASTQ file(s) -> the batches of Ingest, made by HIP kernels and resident in HBM.
    Inputs it does not cover (.gz, FASTA) raise KmaHipError from the constructor, before any HIP call: use Ingest for them."""

    def __init__(self, path1, path2=None, min_phred=20, min_q=0, hardmask_q=0, min_len=16, max_len=2**31 - 1, qc=None, text=False):
        L = lib()
        t = Trim(min_phred, min_q, hardmask_q, min_len, max_len)
        self._h = C.c_void_p()
        _check(L.kmahip_ingest_dev_open(os.fsencode(path1), os.fsencode(path2) if path2 else None, C.byref(t), C.byref(self._h)))
        try:
            if qc is not None:       # the records kernel's -qc instantiation and s1_qc_kernel feed the accumulator (kmahip_ingest_dev_set_qc)
                _check(_qc_lib().kmahip_ingest_dev_set_qc(self._h, qc._h))
            if text:                 # s1_fastq_kernel writes the batches as FASTQ text as well (kmahip_ingest_dev_set_text): text() after every next()
                _check(_qc_lib().kmahip_ingest_dev_set_text(self._h, 1))
        except Exception:
            self.close()
            raise

    def text(self):
        """-> (single records, couples) of the batch delivered last as FASTQ text (bytes), written on the device"""
        out = []
        for k in range(2):
            p, n = C.c_void_p(), C.c_int64()
            _check(_qc_lib().kmahip_ingest_dev_text(self._h, k, C.byref(p), C.byref(n)))
            out.append(C.string_at(p, n.value) if n.value else b"")
        return tuple(out)

    @property
    def phred_scale(self):
        return lib().kmahip_ingest_dev_phred_scale(self._h)

    @property
    def handed_back(self):
        """bytes of input that were left to the host reader (0: the device delivered every record itself)"""
        return int(lib().kmahip_ingest_dev_handed_back(self._h))

    def counts(self):
        a, b = C.c_int64(), C.c_int64()
        lib().kmahip_ingest_dev_counts(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def timing(self):
        """-> (ms reading the files, ms waiting for the copies, ms kernels and scans, input bytes copied up)"""
        ms, n = (C.c_double * 3)(), C.c_int64()
        lib().kmahip_ingest_dev_timing(self._h, ms, C.byref(n))
        return ms[0], ms[1], ms[2], n.value

    def qc_timing(self):
        """-> (ms fetching the counted sequences' (sp, len), ms adding and binning them on the host) of a reader with a QC"""
        ms = (C.c_double * 2)()
        L = lib()
        L.kmahip_ingest_dev_qc_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.kmahip_ingest_dev_qc_timing.restype = None
        L.kmahip_ingest_dev_qc_timing(self._h, ms)
        return ms[0], ms[1]

    def next_dev(self, max_records=1 << 20):
        """the batch as the library hands it out (ReadBatchC with device pointers; valid until the next call), or None at the end"""
        b = ReadBatchC()
        _check(lib().kmahip_ingest_dev_next(self._h, max_records, C.byref(b)))
        return b if b.reads.n_reads else None

    def next(self, max_records=1 << 20):
        """-> (ReadBatch, names list[bytes], pair u8[n]) as Ingest.next, the arrays copied back from the device; None at the end"""
        from . import formats
        b = self.next_dev(max_records)
        if b is None:
            return None
        n = b.reads.n_reads

        def arr(ptr, dt, m):
            out = np.zeros(m, dt)
            if m:
                _check(lib().kmahip_ingest_dev_copy_out(out.ctypes.data_as(C.c_void_p), C.cast(ptr, C.c_void_p), out.nbytes))
            return out
        batch = formats.ReadBatch(seq=arr(b.reads.seq, np.uint64, b.reads.seq_words), seq_off=arr(b.reads.seq_off, np.int64, n + 1),
                                  length=arr(b.reads.len, np.int32, n), N=arr(b.reads.N, np.int32, max(1, b.reads.N_total)),
                                  N_off=arr(b.reads.N_off, np.int64, n + 1))
        noff = arr(b.name_off, np.int64, n + 1)
        raw = arr(b.names, np.uint8, int(noff[-1])).tobytes()
        names = [raw[noff[i]:noff[i + 1] - 1] for i in range(n)]
        pair = np.ctypeslib.as_array(C.cast(b.pair, C.POINTER(C.c_uint8)), shape=(n,)).copy()
        return batch, names, pair

    def status(self):
        _check(lib().kmahip_ingest_dev_status(self._h))

    def close(self):
        if self._h:
            lib().kmahip_ingest_dev_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Session:
    """A kmahip_session on a database, as far as choosing its mode goes: set_sam (kmahip_session_set_sam) beside set_chain / set_mt1 /
    set_pe, each before the first batch. Feeding batches and finishing the run is the host program's (examples/kmahip_map.c)."""

    def __init__(self, db, evalue=0.05, bcd=1, max_frag=0, reads_hint=0, conclave=1, count_kmers=False):
        self._db = db
        self._h = C.c_void_p()
        self._conclave_was = _conclave_now          # (-ConClave: one setting per process, read when the session finishes; close() puts it back)
        set_conclave_version(conclave)
        so = ShardOpts(evalue, bcd, 0, 0, int(max_frag), 1.0, 0.0, 0.0, 0, 1)
        p = Params.from_buffer_copy(db.params)
        self._ck_was = db.count_kmers          # (-ck: the counting scan in every run of the session that scans k-mers; close() puts it back)
        if count_kmers:
            db.set_count_kmers(True)
        try:
            _check(lib().kmahip_session_open(db.h, db.ws, C.byref(p), C.byref(so), int(reads_hint), C.byref(self._h)))
        except Exception:
            db.set_count_kmers(self._ck_was)          # (no session: the workspace and the process are left as they were found)
            set_conclave_version(self._conclave_was)
            raise

    def set_sam(self, level=1, path="-", program="kmahip", cmdline=None):
        _check(lib().kmahip_session_set_sam(self._h, int(level), os.fsencode(path), program.encode(), None if cmdline is None else cmdline.encode()))

    def set_ef(self, cmdline=None, t_db=None):
        _check(lib().kmahip_session_set_ef(self._h, None if cmdline is None else cmdline.encode(), None if t_db is None else os.fsencode(t_db)))

    def set_ef_fragments(self, records):
        _check(lib().kmahip_session_set_ef_fragments(self._h, int(records)))

    def set_matrix(self):
        _check(lib().kmahip_session_set_matrix(self._h))

    def set_vcf(self, level=1, t_db=None):
        _check(lib().kmahip_session_set_vcf(self._h, int(level), None if t_db is None else os.fsencode(t_db)))

    def set_chain(self):
        _check(lib().kmahip_session_set_chain(self._h, None))

    def set_mt1(self, tmpl, one2one=0, frag_path=None):
        _check(lib().kmahip_session_set_mt1(self._h, int(tmpl), int(one2one), None if frag_path is None else os.fsencode(frag_path)))

    def set_pe(self):
        _check(lib().kmahip_session_set_pe(self._h))

    def close(self):
        if self._h:
            lib().kmahip_session_close(self._h)
            self._h = C.c_void_p()
            set_conclave_version(self._conclave_was)
            self._db.set_count_kmers(self._ck_was)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


_conclave_now = 1


def set_conclave_version(v):
    """`-ConClave v` for the whole-run entry points of this process (kmahip_set_conclave_version): 1 runConClave, 2 runConClave2"""
    global _conclave_now
    _check(lib().kmahip_set_conclave_version(int(v)))
    _conclave_now = int(v)


@contextlib.contextmanager
def conclave_version(v):
    """set_conclave_version(v) for a block, the earlier value after it"""
    was = _conclave_now
    set_conclave_version(v)
    try:
        yield
    finally:
        set_conclave_version(was)


def default_params() -> Params:
    p = Params()
    lib().kmahip_default_params(C.byref(p))
    return p


class KmaHipDB:
    """An index resident in HBM + one workspace."""

    def __init__(self, prefix: str, device: int = 0, decon: bool = False):
        """decon: open <prefix>.decon.comp.b (kmahip_db_open_decon): stage 2 then drops what fits the contamination best"""
        L = lib()
        _check(L.kmahip_init(device))
        self.prefix = prefix
        self.decon = bool(decon)
        self.h = C.c_void_p()
        if decon:
            _check(L.kmahip_db_open_decon(prefix.encode(), C.byref(self.h)))
        else:
            _check(L.kmahip_db_open(prefix.encode(), C.byref(self.h)))
        self.ws = C.c_void_p()
        _check(L.kmahip_ws_create(self.h, C.byref(self.ws)))
        self.info = DBInfo()
        _check(L.kmahip_db_get_info(self.h, C.byref(self.info)))
        self.params = default_params()
        self.count_kmers = False

    def set_count_kmers(self, on=True):
        """`-ck` for every later stage-2 call on this workspace (kmahip_ws_set_count_kmers): a template scores one point per k-mer of the
        read it holds (save_kmers_count savekmers.c:3067, get_kmers_for_pair_count :690), not a pseudo-alignment. The chain finder and
        -Mt1 do not read it."""
        L = lib()
        L.kmahip_ws_set_count_kmers.argtypes = [C.c_void_p, C.c_int]
        L.kmahip_ws_set_count_kmers.restype = C.c_int
        _check(L.kmahip_ws_set_count_kmers(self.ws, 1 if on else 0))
        self.count_kmers = bool(on)

    @contextlib.contextmanager
    def _counting(self, on):
        """count_kmers=True of one call: the workspace's setting for its duration, the earlier one after it"""
        was = self.count_kmers
        if on and not was:
            self.set_count_kmers(True)
        try:
            yield
        finally:
            if self.count_kmers != was:
                self.set_count_kmers(was)

    def close(self):
        if getattr(self, "ws", None):
            lib().kmahip_ws_destroy(self.ws)
            self.ws = None
        if getattr(self, "h", None):
            lib().kmahip_db_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host buffers in / out ------------------------------------------------
    def scan_se(self, batch, exhaustive=0, t_cap=None, min_frac=1.0, count_kmers=False):
        """Stage 2 of the -1t1 run -> (rc_flag, flag, T_off, T). min_frac: proximity matching (-proxi): every template within that
        fraction of a strand's best k-mer score is handed on, not only the ties (stage 2 takes its absolute value). count_kmers (-ck):
        a template scores one point per k-mer of the read it holds (save_kmers_count), not a pseudo-alignment"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        rc_flag = np.zeros(max(n, 1), np.int32)
        flag = np.zeros(max(n, 1), np.int32)
        T_off = np.zeros(n + 1, np.int64)
        cap = t_cap or max(1024, 8 * n)
        p = Params.from_buffer_copy(self.params)
        p.exhaustive = exhaustive
        if min_frac != 1.0:
            p.minFrac = float(min_frac)
        for _ in range(8):
            T = np.zeros(cap, np.int32)
            out = Cands(_p(rc_flag), _p(flag), _p(T_off), _p(T), cap)
            with self._counting(count_kmers):
                rc = lib().kmahip_scan_se(self.h, self.ws, C.byref(r), C.byref(p), C.byref(out))
            if rc == -6:  # KMAHIP_EOVERFLOW
                cap = max(cap * 2, int(T_off[n]) + 16)
                continue
            _check(rc)
            return rc_flag[:n], flag[:n], T_off, T[:T_off[n]]
        raise KmaHipError("scan_se: output capacity kept overflowing")

    # -- device resident (torch tensors) -----------------------------------------
    def scan_chain(self, batch, minlen=16, coverT=0.1, mrs=0.5, exhaustive=0):
        """Stage 2 of the default mode (kmahip_scan_chain, no -1t1) -> dict(read, rc_flag, emit_rc, q_start, q_end, T_off, T):
        one entry per S2 record, in stream order"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        p = Params.from_buffer_copy(self.params)
        p.exhaustive = exhaustive
        cp = ChainParams(int(minlen), 0, float(coverT), float(mrs))
        L = lib()
        L.kmahip_scan_chain.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Reads), C.POINTER(Params), C.POINTER(ChainParams), C.POINTER(ChainRecs)]
        L.kmahip_scan_chain.restype = C.c_int
        rec_cap, T_cap = 2 * n + 1024, 16 * n + 4096
        for _ in range(4):
            o = dict(read=np.zeros(rec_cap, np.int64), rc_flag=np.zeros(rec_cap, np.int32), emit_rc=np.zeros(rec_cap, np.int32),
                     q_start=np.zeros(rec_cap, np.int32), q_end=np.zeros(rec_cap, np.int32), T_off=np.zeros(rec_cap + 1, np.int64),
                     T=np.zeros(T_cap, np.int32))
            out = ChainRecs(rec_cap, T_cap, 0, 0, _p(o["read"]), _p(o["rc_flag"]), _p(o["emit_rc"]), _p(o["q_start"]), _p(o["q_end"]),
                            _p(o["T_off"]), _p(o["T"]))
            rc = L.kmahip_scan_chain(self.h, self.ws, C.byref(r), C.byref(p), C.byref(cp), C.byref(out))
            if rc == -6 and (out.n_recs > rec_cap or out.n_T > T_cap):
                rec_cap, T_cap = max(rec_cap, out.n_recs + 16), max(T_cap, out.n_T + 16)
                continue
            _check(rc)
            m = out.n_recs
            for key in ("read", "rc_flag", "emit_rc", "q_start", "q_end"):
                o[key] = o[key][:m]
            o["T_off"] = o["T_off"][:m + 1]
            o["T"] = o["T"][:out.n_T]
            return o
        raise KmaHipError("scan_chain: output capacity kept overflowing")

    def scan_se_dev(self, seq, seq_off, length, N, N_off, rc_flag, flag, T_off, T, exhaustive=0, stream=None, min_frac=1.0):
        """All arguments are CUDA(HIP) torch tensors; asynchronous on `stream`. min_frac: as scan_se."""
        n = length.numel()
        r = Reads(n, seq.data_ptr(), seq_off.data_ptr(), length.data_ptr(), N.data_ptr(), N_off.data_ptr(),
                  seq.numel(), N.numel(), 0)
        out = Cands(rc_flag.data_ptr(), flag.data_ptr(), T_off.data_ptr(), T.data_ptr(), T.numel())
        p = Params.from_buffer_copy(self.params)
        p.exhaustive = exhaustive
        if min_frac != 1.0:
            p.minFrac = float(min_frac)
        _check(lib().kmahip_scan_se_dev(self.h, self.ws, C.byref(r), C.byref(p), C.byref(out), C.c_void_p(stream or 0)))

    def status(self, stream=None):
        _check(lib().kmahip_ws_status(self.ws, C.c_void_p(stream or 0)))

    def set_stats(self, on: bool):
        _check(lib().kmahip_scan_set_stats(self.ws, int(on)))

    def get_stats(self, stream=None) -> ScanStats:
        st = ScanStats()
        _check(lib().kmahip_scan_get_stats(self.ws, C.byref(st), C.c_void_p(stream or 0)))
        return st

    def get_scan_overflow(self, stream=None):
        """(items handed to the second tier, items handed to scan_dense_kernel) of the last scan launch"""
        out = (C.c_ulonglong * 2)()
        L = lib()
        L.kmahip_ws_scan_overflow.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        _check(L.kmahip_ws_scan_overflow(self.ws, C.c_void_p(stream or 0), out))
        return int(out[0]), int(out[1])

    def get_scan_routes(self, stream=None):
        """(items taken as records, items taken from the bare list) of the last scan launch"""
        out = (C.c_ulonglong * 2)()
        _check(lib().kmahip_ws_scan_routes(self.ws, C.c_void_p(stream or 0), out))
        return int(out[0]), int(out[1])

    def get_scan_diag_replaced(self, stream=None) -> int:
        """records of the last scan launch whose diagonal the prefilter replaced (counted with set_stats(True))"""
        out = C.c_ulonglong(0)
        _check(lib().kmahip_ws_scan_diag_replaced(self.ws, C.c_void_p(stream or 0), C.byref(out)))
        return int(out.value)

    def get_scan_queue_counts(self, stream=None):
        """(k-mer starts left to the queue round, rounds that had any) of the last scan launch (counted with set_stats(True))"""
        out = (C.c_ulonglong * 2)()
        L = lib()
        L.kmahip_ws_scan_queue_counts.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        _check(L.kmahip_ws_scan_queue_counts(self.ws, C.c_void_p(stream or 0), out))
        return int(out[0]), int(out[1])

    def get_scan_settled(self, stream=None) -> int:
        """record items of the last scan launch that the prefilter settled from the span table (always counted)"""
        out = C.c_ulonglong(0)
        L = lib()
        L.kmahip_ws_scan_settled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        _check(L.kmahip_ws_scan_settled(self.ws, C.c_void_p(stream or 0), C.byref(out)))
        return int(out.value)

    def test_span_table(self, n):
        """kmahip_test_span_table (a test hook): (t0, need, room) of the first n positions of the concatenated templates as the
        device holds them, or None when the database was opened without the table"""
        t0, need, room = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        L = lib()
        L.kmahip_test_span_table.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kmahip_test_span_table.restype = C.c_int
        rc = L.kmahip_test_span_table(self.h, n, _p(t0), _p(need), _p(room))
        if rc == 0:
            return None
        if rc < 0:
            _check(rc)
        return t0, need, room

    def list_table_log2(self) -> int:
        """log2 of the list table's bucket count, 0: the database was opened without one"""
        L = lib()
        L.kmahip_db_list_table_log2.argtypes = [C.c_void_p]
        L.kmahip_db_list_table_log2.restype = C.c_int
        return int(L.kmahip_db_list_table_log2(self.h))

    def test_list_probe(self, keys):
        """kmahip_test_list_probe (a test hook): for every 32-bit key (the list table's answer, the list offset by way of the probe
        table's position), 0xFFFFFFFF = not in the index -> two uint32 arrays"""
        k = np.ascontiguousarray(keys, np.uint32)
        assert k.ndim == 1
        out_list, out_via_pos = np.zeros(len(k), np.uint32), np.zeros(len(k), np.uint32)
        L = lib()
        L.kmahip_test_list_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.kmahip_test_list_probe.restype = C.c_int
        _check(L.kmahip_test_list_probe(self.h, _p(k), len(k), _p(out_list), _p(out_via_pos)))
        return out_list, out_via_pos

    def get_align_queue_counts(self, stream=None) -> dict:
        """stage 3a's class queues after the last alignment launch: entries per class, pending tasks, hand-ons over the queues"""
        out = (C.c_ulonglong * 6)()
        _check(lib().kmahip_ws_align_queue_counts(self.ws, C.c_void_p(stream or 0), out))
        return dict(zip(("wide", "mid", "narrow", "tiny", "pending", "handed_on"), (int(x) for x in out)))

    def get_trace_put_off(self, stream=None):
        """reads the first pass of the last two-pass traceback launch put off, and those the LDS pass (KMAHIP_TRACE_LDS=1) put off again"""
        out = (C.c_ulonglong * 2)()
        L = lib()
        L.kmahip_ws_trace_put_off.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        _check(L.kmahip_ws_trace_put_off(self.ws, C.c_void_p(stream or 0), out))
        return int(out[0]), int(out[1])

    def get_align_stats(self, stream=None) -> AlignStats:
        st = AlignStats()
        _check(lib().kmahip_align_get_stats(self.ws, C.byref(st), C.c_void_p(stream or 0)))
        return st

    def get_trace_stats(self) -> TraceStats:
        st = TraceStats()
        _check(lib().kmahip_trace_get_stats(self.ws, C.byref(st)))
        return st

    def get_trace_class_counts(self) -> dict:
        """DP problems of the last long-read trace call per size class: wave (17 wavefront classes), lane (9 lane classes)"""
        out = (C.c_ulonglong * 26)()
        _check(lib().kmahip_trace_get_class_counts(self.ws, out))
        return dict(wave=[int(x) for x in out[:17]], lane=[int(x) for x in out[17:]])

    def get_chain_route_counts(self) -> dict:
        """reads of the last scan_chain call by route: reads, marked (chain_anchor_kernel handed them over), given_up (chain_fast_kernel
        found its template table full), long (the long-read route took them), lane (chain_kernel took them)"""
        out = (C.c_ulonglong * 5)()
        _check(lib().kmahip_chain_get_route_counts(self.ws, out))
        return dict(zip(("reads", "marked", "given_up", "long", "lane"), (int(x) for x in out)))

    def set_timing(self, on: bool):
        _check(lib().kmahip_ws_set_timing(self.ws, int(on)))

    def get_timing(self, kernel=0):
        """kernel 0 = scan_se_kernel, 1 = align_tasks_kernel, 2 = scan_prefilter_kernel, 3 = seed_tasks_kernel -> (summed ms, launches)"""
        ms, n = C.c_double(), C.c_int64()
        _check(lib().kmahip_ws_get_timing(self.ws, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- stages 2 + 3a, host buffers ------------------------------------------
    def map_se(self, batch, exhaustive=0, t_cap=None, min_frac=1.0, circular=False, count_kmers=False):
        """-> (rc_flag, flag, T_off, T), hits dict (n_hits, best_score, flag, tmpl, score, start, end,
        alignment_scores, uniq_alignment_scores). min_frac: proximity matching (-proxi f) in stages 2 and 3a; its sign chooses what a
        kept hit adds to alignment_scores (positive: the read's best score, negative: the hit's own)"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        rc_flag = np.zeros(max(n, 1), np.int32)
        flag = np.zeros(max(n, 1), np.int32)
        T_off = np.zeros(n + 1, np.int64)
        cap = t_cap or max(1024, 8 * n)
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        p.exhaustive = exhaustive
        if min_frac != 1.0:
            p.minFrac = float(min_frac)
        D = int(self.info.DB_size)
        for _ in range(8):
            T = np.zeros(cap, np.int32)
            h = dict(n_hits=np.zeros(max(n, 1), np.int32), best_score=np.zeros(max(n, 1), np.int32),
                     flag=np.zeros(max(n, 1), np.int32), tmpl=np.zeros(cap, np.int32), score=np.zeros(cap, np.int32),
                     start=np.zeros(cap, np.int32), end=np.zeros(cap, np.int32),
                     alignment_scores=np.zeros(D, np.uint64), uniq_alignment_scores=np.zeros(D, np.uint64),
                     rc=np.zeros(max(n, 1), np.int32))
            out = Cands(_p(rc_flag), _p(flag), _p(T_off), _p(T), cap)
            hs = Hits(_p(h["n_hits"]), _p(h["best_score"]), _p(h["flag"]), _p(h["tmpl"]), _p(h["score"]), _p(h["start"]),
                      _p(h["end"]), _p(h["alignment_scores"]), _p(h["uniq_alignment_scores"]), _p(h["rc"]))
            with self._counting(count_kmers):
                rc = lib().kmahip_map_se(self.h, self.ws, C.byref(r), C.byref(p), C.byref(out), C.byref(hs))
            if rc == -6 and int(T_off[n]) > cap:
                cap = max(cap * 2, int(T_off[n]) + 16)
                continue
            if rc == -6 and b"candidate pool" in lib().kmahip_last_error():          # (the library has grown its pool: once more)
                continue
            _check(rc)
            for key in ("n_hits", "best_score", "flag", "rc"):
                h[key] = h[key][:n]
            return (rc_flag[:n], flag[:n], T_off, T[:T_off[n]]), h
        raise KmaHipError("map_se: output capacity kept overflowing")

    def align_se_dev(self, seq, seq_off, length, N, N_off, max_len, rc_flag, flag, T_off, T,
                     n_hits, best_score, out_flag, h_tmpl, h_score, h_start, h_end, aln_scores, uniq_scores, stream=None, min_frac=1.0, circular=False):
        """Stage 3a on device tensors (outputs of scan_se_dev); asynchronous on `stream`. min_frac: as map_se."""
        n = length.numel()
        r = Reads(n, seq.data_ptr(), seq_off.data_ptr(), length.data_ptr(), N.data_ptr(), N_off.data_ptr(),
                  seq.numel(), N.numel(), int(max_len))
        c = Cands(rc_flag.data_ptr(), flag.data_ptr(), T_off.data_ptr(), T.data_ptr(), T.numel())
        h = Hits(n_hits.data_ptr(), best_score.data_ptr(), out_flag.data_ptr(), h_tmpl.data_ptr(), h_score.data_ptr(),
                 h_start.data_ptr(), h_end.data_ptr(), aln_scores.data_ptr(), uniq_scores.data_ptr(), None)
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        if min_frac != 1.0:
            p.minFrac = float(min_frac)
        _check(lib().kmahip_align_se_dev(self.h, self.ws, C.byref(r), C.byref(c), C.byref(p), C.byref(h),
                                         C.c_void_p(stream or 0)))

    def scan_pe_dev(self, seq, seq_off, length, N, N_off, mate, rc, rc_flag, flag, R_off, T, exhaustive=0, stream=None):
        """Stage 2 for interleaved mates (`-apm p`) on device tensors; asynchronous on `stream`. mate / rc / rc_flag / flag: i32[2 pairs],
        R_off i64[2 pairs + 1], T i32[capacity]."""
        n = length.numel()
        r = Reads(n, seq.data_ptr(), seq_off.data_ptr(), length.data_ptr(), N.data_ptr(), N_off.data_ptr(), seq.numel(), N.numel(), 0)
        out = PeRecs(mate.data_ptr(), rc.data_ptr(), rc_flag.data_ptr(), flag.data_ptr(), R_off.data_ptr(), T.data_ptr(), T.numel())
        p = Params.from_buffer_copy(self.params)
        p.exhaustive = exhaustive
        _check(lib().kmahip_scan_pe_dev(self.h, self.ws, C.byref(r), C.byref(p), C.byref(out), C.c_void_p(stream or 0)))

    def align_pe_dev(self, seq, seq_off, length, N, N_off, max_len, mate, rc, rc_flag, flag, R_off, T,
                     n_hits, best_score, out_flag, h_tmpl, h_score, h_start, h_end, aln_scores, uniq_scores, out_rc, kind, stream=None, circular=False):
        """Stage 3a for the records of scan_pe_dev on device tensors; asynchronous on `stream`. kind: i32[pairs]."""
        n = length.numel()
        r = Reads(n, seq.data_ptr(), seq_off.data_ptr(), length.data_ptr(), N.data_ptr(), N_off.data_ptr(), seq.numel(), N.numel(), int(max_len))
        recs = PeRecs(mate.data_ptr(), rc.data_ptr(), rc_flag.data_ptr(), flag.data_ptr(), R_off.data_ptr(), T.data_ptr(), T.numel())
        h = Hits(n_hits.data_ptr(), best_score.data_ptr(), out_flag.data_ptr(), h_tmpl.data_ptr(), h_score.data_ptr(),
                 h_start.data_ptr(), h_end.data_ptr(), aln_scores.data_ptr(), uniq_scores.data_ptr(), out_rc.data_ptr())
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        _check(lib().kmahip_align_pe_dev(self.h, self.ws, C.byref(r), C.byref(recs), C.byref(p), C.byref(h), C.c_void_p(kind.data_ptr()),
                                         C.c_void_p(stream or 0)))

    # -- stage 3b (ConClave) -----------------------------------------------------------
    def _conclave_out(self, n):
        D = int(self.info.DB_size)
        o = dict(tmpl=np.zeros(max(n, 1), np.int32), start=np.zeros(max(n, 1), np.int32), end=np.zeros(max(n, 1), np.int32),
                 w_scores=np.zeros(D, np.uint64), fragment_counts=np.zeros(D, np.uint32), read_counts=np.zeros(D, np.uint32),
                 depth=np.zeros(D, np.uint64))
        return o, Conclave(_p(o["tmpl"]), _p(o["start"]), _p(o["end"]), _p(o["w_scores"]), _p(o["fragment_counts"]),
                           _p(o["read_counts"]), _p(o["depth"]))

    @staticmethod
    def _hits_struct(h):
        c = lambda a, t: np.ascontiguousarray(a if len(a) else np.zeros(1, t), t)
        keep = [c(h["n_hits"], np.int32), c(h["best_score"], np.int32), c(h["tmpl"], np.int32), c(h["start"], np.int32),
                c(h["end"], np.int32), c(h["alignment_scores"], np.uint64), c(h["uniq_alignment_scores"], np.uint64)]
        return keep, Hits(_p(keep[0]), _p(keep[1]), None, _p(keep[2]), None, _p(keep[3]), _p(keep[4]), _p(keep[5]), _p(keep[6]), None)

    def conclave_se(self, length, T_off, hits):
        """Stage 3b for the result of map_se (host arrays; `hits` may carry vectors summed over ranks) -> dict(tmpl, start,
        end per read; w_scores, fragment_counts, read_counts, depth per template)"""
        n = len(length)
        ln = np.ascontiguousarray(length, np.int32)
        to = np.ascontiguousarray(T_off, np.int64)
        r = Reads(n, None, None, _p(ln), None, None, 0, 0, 0)
        c = Cands(None, None, _p(to), None, 0)
        keep, hs = self._hits_struct(hits)
        o, oc = self._conclave_out(n)
        _check(lib().kmahip_conclave_se(self.h, self.ws, C.byref(r), C.byref(c), C.byref(hs), C.byref(oc)))
        for key in ("tmpl", "start", "end"):
            o[key] = o[key][:n]
        return o

    def conclave_pe(self, length, mate, R_off, hits):
        """Stage 3b for the result of map_pe (record slots; hits["kind"] per pair)"""
        n = len(length)
        ln = np.ascontiguousarray(length, np.int32)
        ro = np.ascontiguousarray(R_off, np.int64)
        mt = np.ascontiguousarray(mate if n else np.zeros(1, np.int32), np.int32)
        kd = np.ascontiguousarray(hits["kind"], np.int32)
        r = Reads(n, None, None, _p(ln), None, None, 0, 0, 0)
        pr = PeRecs(_p(mt), None, None, None, _p(ro), None, 0)
        keep, hs = self._hits_struct(hits)
        o, oc = self._conclave_out(n)
        _check(lib().kmahip_conclave_pe(self.h, self.ws, C.byref(r), C.byref(pr), C.byref(hs), _p(kd), C.byref(oc)))
        for key in ("tmpl", "start", "end"):
            o[key] = o[key][:n]
        return o

    def conclave_records(self, n_hits, score, q_len, q_len2, off, tmpl, start, end, alignment_scores, uniq_alignment_scores):
        """Stage 3b over explicit frag_raw records in stream order (score < 0: pair record)"""
        n = len(n_hits)
        ql = np.ascontiguousarray(q_len if n else np.zeros(1, np.int32), np.int32)
        ql2 = np.ascontiguousarray(q_len2 if n else np.zeros(1, np.int32), np.int32)
        of = np.ascontiguousarray(off, np.int64)
        assert len(of) == n + 1
        keep, hs = self._hits_struct(dict(n_hits=n_hits, best_score=score, tmpl=tmpl, start=start, end=end,
                                          alignment_scores=alignment_scores, uniq_alignment_scores=uniq_alignment_scores))
        o, oc = self._conclave_out(n)
        _check(lib().kmahip_conclave_records(self.h, self.ws, n, _p(ql), _p(ql2), _p(of), C.byref(hs), C.byref(oc)))
        for key in ("tmpl", "start", "end"):
            o[key] = o[key][:n]
        return o

    def conclave2_records(self, n_hits, score, q_len, q_len2, off, q_seed, tmpl, start, end, alignment_scores, uniq_alignment_scores,
                          evalue=0.05, scoreT=0.5):
        """Stage 3b, version 2 (runConClave2, kmahip_conclave2_records) over explicit frag_raw records in stream order; q_seed: per record
        the seed of its draw (conclave.c:566-571). The `-lc` order with kmahip_set_conclave_lc."""
        n = len(n_hits)
        ql = np.ascontiguousarray(q_len if n else np.zeros(1, np.int32), np.int32)
        ql2 = np.ascontiguousarray(q_len2 if n else np.zeros(1, np.int32), np.int32)
        sd = np.ascontiguousarray(q_seed if n else np.zeros(1, np.int32), np.int32)
        of = np.ascontiguousarray(off, np.int64)
        assert len(of) == n + 1 and len(sd) >= n
        keep, hs = self._hits_struct(dict(n_hits=n_hits, best_score=score, tmpl=tmpl, start=start, end=end,
                                          alignment_scores=alignment_scores, uniq_alignment_scores=uniq_alignment_scores))
        o, oc = self._conclave_out(n)
        _check(lib().kmahip_conclave2_records(self.h, self.ws, n, _p(ql), _p(ql2), _p(of), _p(sd), C.byref(hs), float(evalue), float(scoreT), C.byref(oc)))
        for key in ("tmpl", "start", "end"):
            o[key] = o[key][:n]
        return o

    def conclave_se_dev(self, length, T_off, n_hits, best_score, h_tmpl, h_start, h_end, aln_scores, uniq_scores,
                        o_tmpl, o_start, o_end, w_scores, fragment_counts=None, read_counts=None, depth=None, stream=None):
        """Stage 3b on device tensors (outputs of align_se_dev); asynchronous on `stream`."""
        dp = lambda t: t.data_ptr() if t is not None else None
        r = Reads(length.numel(), None, None, length.data_ptr(), None, None, 0, 0, 0)
        c = Cands(None, None, T_off.data_ptr(), None, 0)
        h = Hits(n_hits.data_ptr(), best_score.data_ptr(), None, h_tmpl.data_ptr(), None, h_start.data_ptr(), h_end.data_ptr(),
                 aln_scores.data_ptr(), uniq_scores.data_ptr(), None)
        o = Conclave(o_tmpl.data_ptr(), o_start.data_ptr(), o_end.data_ptr(), w_scores.data_ptr(), dp(fragment_counts),
                     dp(read_counts), dp(depth))
        _check(lib().kmahip_conclave_se_dev(self.h, self.ws, C.byref(r), C.byref(c), C.byref(h), C.byref(o), C.c_void_p(stream or 0)))

    def align_trace(self, batch, rc, tmpl, tmpl_ok=None, circular=False):
        """Stage 3c per read (host arrays): traceback alignment of every read against the template ConClave chose.
        -> stats [n, 10] (score, start, end, aln_len, clip_start, clip_end, match, tGaps, qGaps, mapQ; zeros = dropped),
        ops_off [n], n_ops [n], ops (runs (len << 2) | class, classes = X I D)"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        fl = np.ascontiguousarray(rc if n else np.zeros(1, np.int32), np.int32)
        tm = np.ascontiguousarray(tmpl if n else np.zeros(1, np.int32), np.int32)
        ok = None if tmpl_ok is None else np.ascontiguousarray(tmpl_ok, np.uint8)
        stats = np.zeros((max(n, 1), 10), np.int32)
        off = np.zeros(max(n, 1), np.int64)
        nops = np.zeros(max(n, 1), np.int32)
        cap = max(1024, 8 * n)
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        need = C.c_int64()
        for _ in range(3):
            ops = np.zeros(cap, np.uint32)
            o = Traces(_p(stats), _p(off), _p(nops), _p(ops), cap)
            rc = lib().kmahip_align_trace(self.h, self.ws, C.byref(r), _p(fl), _p(tm), None if ok is None else _p(ok), C.byref(p),
                                          C.byref(o), C.byref(need))
            if rc == -6:
                cap = need.value + 16
                continue
            _check(rc)
            return stats[:n], off[:n], nops[:n], ops[:need.value]
        raise KmaHipError("align_trace: output capacity kept overflowing")

    def align_trace_mt1(self, batch, tmpl, one2one=0, circular=False):
        """`-Mt1 tmpl`: every raw read against one template, strand by anker_rc -> (stats, ops_off, n_ops, ops) as align_trace, rc [n]"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        stats = np.zeros((max(n, 1), 10), np.int32)
        off = np.zeros(max(n, 1), np.int64)
        nops = np.zeros(max(n, 1), np.int32)
        rc_out = np.zeros(max(n, 1), np.int32)
        cap = max(1024, int(batch.length.sum()) // 4)
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        need = C.c_int64()
        for _ in range(3):
            ops = np.zeros(cap, np.uint32)
            o = Traces(_p(stats), _p(off), _p(nops), _p(ops), cap)
            rc = lib().kmahip_align_trace_mt1(self.h, self.ws, C.byref(r), int(tmpl), int(one2one), C.byref(p), C.byref(o), _p(rc_out), C.byref(need))
            if rc == -6 and need.value > cap:
                cap = need.value + 16
                continue
            _check(rc)
            return (stats[:n], off[:n], nops[:n], ops[:need.value]), rc_out[:n]
        raise KmaHipError("align_trace_mt1: output capacity kept overflowing")

    def assemble(self, batch, rc, tmpl, traces, max_frag=0, bcd=1, evalue=0.05, consensus=False, frag_rank=None):
        """Stage 3c per template: pile-up of the traced reads + consensus -> dict(cover, aln_len, depth, asm_len [DB_size],
        consensus {template: str} when asked). traces = the tuple align_trace returned. frag_rank: positions of the reads among
        the filed fragments of the whole stream, for a batch gathered from several read shards (kmahip_assemble_opts.frag_rank)."""
        n = batch.n
        stats, off, nops, ops = traces
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        fl = np.ascontiguousarray(rc if n else np.zeros(1, np.int32), np.int32)
        tm = np.ascontiguousarray(tmpl if n else np.zeros(1, np.int32), np.int32)
        st = np.ascontiguousarray(stats if n else np.zeros((1, 10), np.int32), np.int32)
        of = np.ascontiguousarray(off if n else np.zeros(1, np.int64), np.int64)
        no = np.ascontiguousarray(nops if n else np.zeros(1, np.int32), np.int32)
        op = np.ascontiguousarray(ops if len(ops) else np.zeros(1, np.uint32), np.uint32)
        tr = Traces(_p(st), _p(of), _p(no), _p(op), len(op))
        D = int(self.info.DB_size)
        o = dict(cover=np.zeros(D, np.int64), aln_len=np.zeros(D, np.int64), depth=np.zeros(D, np.int64), asm_len=np.zeros(D, np.int64))
        cap = 0
        cbuf = coff = None
        if consensus:
            cap = int(2 * np.fromfile(self.prefix + ".length.b", dtype=np.int32)[1:].astype(np.int64).sum() + 4 * D + (1 << 20))
            cbuf = np.zeros(cap, np.uint8)
            coff = np.full(D, -1, np.int64)
        a = Assembly(_p(o["cover"]), _p(o["aln_len"]), _p(o["depth"]), _p(o["asm_len"]), None if cbuf is None else _p(cbuf),
                     None if coff is None else _p(coff), cap, 0)
        fr = None if frag_rank is None else np.ascontiguousarray(frag_rank if n else np.zeros(1, np.int64), np.int64)
        ao = AssembleOpts(int(max_frag), float(evalue), int(bcd), 0, 0, 0, None if fr is None else _p(fr))
        _check(lib().kmahip_assemble2(self.h, self.ws, C.byref(r), _p(fl), _p(tm), C.byref(tr), C.byref(ao), C.byref(a)))
        if consensus:
            raw = cbuf.tobytes()
            o["consensus"] = {t: raw[coff[t]:raw.index(b"\0", coff[t])].decode() for t in range(D) if coff[t] >= 0}
        return o

    def run_se(self, batch, evalue=0.05, bcd=1, max_frag=0, consensus=True, per_read=True, bc_nano=False, min_frac=1.0, circular=False, conclave=1, count_kmers=False):
        """The whole single-end run in one call (kmahip_run_se) -> dict(rows [ResRow], cover, aln_len, depth, asm_len, consensus,
        tmpl, n_hits, rc, trace_stats, ms). min_frac: proximity matching (-proxi f), as map_se. conclave: `-ConClave n`, for this call."""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        D = int(self.info.DB_size)
        o = dict(cover=np.zeros(D, np.int64), aln_len=np.zeros(D, np.int64), depth=np.zeros(D, np.int64), asm_len=np.zeros(D, np.int64))
        cap = 0
        cbuf = coff = None
        if consensus:
            cap = int(2 * np.fromfile(self.prefix + ".length.b", dtype=np.int32)[1:].astype(np.int64).sum() + 4 * D + (1 << 20))
            cbuf = np.zeros(cap, np.uint8)
            coff = np.full(D, -1, np.int64)
        rows = (ResRow * D)()
        pr = {k: np.zeros(max(1, n) * (10 if k == "trace_stats" else 1), np.int32) for k in ("tmpl", "n_hits", "rc", "trace_stats")} if per_read else {}
        run = Run(C.cast(rows, C.c_void_p), D, 0,
                  Assembly(_p(o["cover"]), _p(o["aln_len"]), _p(o["depth"]), _p(o["asm_len"]), None if cbuf is None else _p(cbuf),
                           None if coff is None else _p(coff), cap, 0),
                  *[(_p(pr[k]) if per_read else None) for k in ("tmpl", "n_hits", "rc", "trace_stats")])
        run.caller = run.sig90 = 1 if bc_nano else 0
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        if min_frac != 1.0:
            p.minFrac = float(min_frac)
        with conclave_version(conclave), self._counting(count_kmers):
            _check(lib().kmahip_run_se(self.h, self.ws, C.byref(r), C.byref(p), float(evalue), int(bcd), int(max_frag), C.byref(run)))
        o["rows"] = [rows[i] for i in range(run.n_rows)]
        if consensus:
            raw = cbuf.tobytes()
            o["consensus"] = {t: raw[coff[t]:raw.index(b"\0", coff[t])].decode() for t in range(D) if coff[t] >= 0}
        for k, v in pr.items():
            o[k] = v[:n * 10].reshape(n, 10) if k == "trace_stats" else v[:n]
        o["ms"] = list(run.ms)
        return o

    def run_mt1(self, batch, tmpl, one2one=0, bc_nano=True, evalue=0.05, bcd=1, consensus=True, circular=False):
        """The `-Mt1 tmpl [-bcNano]` run in one call (kmahip_run_mt1) -> dict(row, cover, aln_len, depth, asm_len, consensus, tmpl, n_hits,
        rc, trace_stats, ms)"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        D = int(self.info.DB_size)
        o = dict(cover=np.zeros(D, np.int64), aln_len=np.zeros(D, np.int64), depth=np.zeros(D, np.int64), asm_len=np.zeros(D, np.int64))
        cap = 0
        cbuf = coff = None
        if consensus:
            cap = int(2 * np.fromfile(self.prefix + ".length.b", dtype=np.int32)[1:].astype(np.int64).sum() + 4 * D + (1 << 20))
            cbuf = np.zeros(cap, np.uint8)
            coff = np.full(D, -1, np.int64)
        rows = (ResRow * 1)()
        pr = {k: np.zeros(max(1, n) * (10 if k == "trace_stats" else 1), np.int32) for k in ("tmpl", "n_hits", "rc", "trace_stats")}
        run = Run(C.cast(rows, C.c_void_p), 1, 0,
                  Assembly(_p(o["cover"]), _p(o["aln_len"]), _p(o["depth"]), _p(o["asm_len"]), None if cbuf is None else _p(cbuf),
                           None if coff is None else _p(coff), cap, 0),
                  *[_p(pr[k]) for k in ("tmpl", "n_hits", "rc", "trace_stats")])
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        ao = AssembleOpts(0, float(evalue), int(bcd), 1, 1 if bc_nano else 0, 1 if bc_nano else 0)
        _check(lib().kmahip_run_mt1(self.h, self.ws, C.byref(r), int(tmpl), int(one2one), C.byref(p), C.byref(ao), C.byref(run)))
        o["row"] = rows[0]
        if consensus:
            raw = cbuf.tobytes()
            o["consensus"] = {t: raw[coff[t]:raw.index(b"\0", coff[t])].decode() for t in range(D) if coff[t] >= 0}
        for k, v in pr.items():
            o[k] = v[:n * 10].reshape(n, 10) if k == "trace_stats" else v[:n]
        o["ms"] = list(run.ms)
        return o

    def frag_write2(self, path, batch, rc, tmpl, n_hits, stats, read_names, order=1, max_frag=0, frag_rank=None):
        """kmahip_frag_write3: order 1 = stream order (`-Mt1`); frag_rank as in assemble"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        fl = np.ascontiguousarray(rc if n else np.zeros(1, np.int32), np.int32)
        tm = np.ascontiguousarray(tmpl if n else np.zeros(1, np.int32), np.int32)
        nh = np.ascontiguousarray(n_hits if n else np.zeros(1, np.int32), np.int32)
        st = np.ascontiguousarray(stats if n else np.zeros((1, 10), np.int32), np.int32)
        blob = b"".join(nm + b"\0" for nm in read_names) + b"\0"
        noff = np.zeros(n + 1, np.int64)
        if n:
            noff[1:] = np.cumsum([len(nm) + 1 for nm in read_names])
        rows = C.c_int64()
        fr = None if frag_rank is None else np.ascontiguousarray(frag_rank if n else np.zeros(1, np.int64), np.int64)
        _check(lib().kmahip_frag_write3(os.fsencode(path), self.h, C.byref(r), _p(fl), _p(tm), _p(nh), _p(st), int(max_frag), int(order),
                                        None if fr is None else _p(fr), blob, _p(noff), C.byref(rows)))
        return rows.value

    def sam_header(self, path, program="kmahip", cmdline=None):
        """kmahip_sam_header: @HD, @PG and the @SQ lines into `path` (created or emptied; "-" = standard output)"""
        _check(lib().kmahip_sam_header(self.h, program.encode(), None if cmdline is None else cmdline.encode(), os.fsencode(path)))

    def sam_write(self, path, batch, rc, tmpl, n_hits, flag, traces, read_names, drops=None, tmpl_ok=None, level=1, order=0, max_frag=0,
                  frag_rank=None):
        """kmahip_sam_write: the SAM rows of a batch (host arrays) appended to `path`, made on the device. traces = (stats [n, 10],
        ops_off, n_ops, ops) as align_trace returns them, drops = (stats [n, 6], ops_off, n_ops) or None.
        -> (rows, [rows of classes 1, 2, 3a, 3b, 3c + 3d])"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        i32 = lambda a: np.ascontiguousarray(a if n else np.zeros(1, np.int32), np.int32)  # noqa: E731
        fl, tm, nh, fg = i32(rc), i32(tmpl), i32(n_hits), i32(flag)
        st = np.ascontiguousarray(traces[0] if n else np.zeros((1, 10), np.int32), np.int32)
        off = np.ascontiguousarray(traces[1] if n else np.zeros(1, np.int64), np.int64)
        nops = i32(traces[2])
        ops = np.ascontiguousarray(traces[3], np.uint32)
        tr = Traces(_p(st), _p(off), _p(nops), _p(ops) if len(ops) else None, len(ops))
        dr = None
        if drops is not None:
            dst = np.ascontiguousarray(drops[0] if n else np.zeros((1, 6), np.int32), np.int32)
            doff = np.ascontiguousarray(drops[1] if n else np.zeros(1, np.int64), np.int64)
            dn = i32(drops[2])
            dr = TraceDrops(_p(dst), _p(doff), _p(dn))
        ok = None if tmpl_ok is None else np.ascontiguousarray(tmpl_ok, np.uint8)
        fr = None if frag_rank is None else np.ascontiguousarray(frag_rank if n else np.zeros(1, np.int64), np.int64)
        blob = b"".join(nm + b"\0" for nm in read_names) + b"\0"
        noff = np.zeros(n + 1, np.int64)
        if n:
            noff[1:] = np.cumsum([len(nm) + 1 for nm in read_names])
        rows = C.c_int64()
        per = (C.c_int64 * 5)()
        _check(lib().kmahip_sam_write(os.fsencode(path), self.h, C.byref(r), _p(fl), _p(tm), _p(nh), _p(fg), C.byref(tr),
                                      None if dr is None else C.byref(dr), None if ok is None else _p(ok), int(max_frag), int(order),
                                      None if fr is None else _p(fr), blob, _p(noff), int(level), C.byref(rows), per))
        return rows.value, list(per)

    def session(self, evalue=0.05, bcd=1, max_frag=0, reads_hint=0, conclave=1, count_kmers=False):
        """a kmahip_session on this database and workspace, for choosing its mode (Session); conclave: `-ConClave n` until it is closed;
        count_kmers: `-ck`"""
        return Session(self, evalue, bcd, max_frag, reads_hint, conclave, count_kmers)

    def set_pe_chain(self, on=True, minlen=16, coverT=0.1, mrs=0.5):
        """Paired runs on this workspace in the reference's default mode (no -1t1): records that lost their mate go to the chain
        finder (kmahip_ws_set_pe_chain); on=False: back to -1t1."""
        _check(lib().kmahip_ws_set_pe_chain(self.ws, C.byref(ChainParams(int(minlen), 0, float(coverT), float(mrs))) if on else None))

    def run_pe(self, batch, names, pair, evalue=0.05, bcd=1, max_frag=0, frag_path=None, circular=False, conclave=1, count_kmers=False):
        """The paired run in one call (kmahip_run_pe) on what Ingest.next returned for two mate files -> dict(rows, cover, aln_len,
        depth, asm_len, consensus, ms). conclave: `-ConClave n`, for this call."""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        blob = b"".join(nm + b"\0" for nm in names) + b"\0"
        blob_buf = C.create_string_buffer(blob, len(blob))
        noff = np.zeros(n + 1, np.int64)
        if n:
            noff[1:] = np.cumsum([len(nm) + 1 for nm in names])
        pr = np.ascontiguousarray(pair, np.uint8)
        rb = ReadBatchC(Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                              int(batch.length.max()) if n else 0), C.cast(blob_buf, C.c_void_p), _p(noff), _p(pr), 0)
        D = int(self.info.DB_size)
        o = dict(cover=np.zeros(D, np.int64), aln_len=np.zeros(D, np.int64), depth=np.zeros(D, np.int64), asm_len=np.zeros(D, np.int64))
        cap = int(2 * np.fromfile(self.prefix + ".length.b", dtype=np.int32)[1:].astype(np.int64).sum() + 4 * D + (1 << 20))
        cbuf = np.zeros(cap, np.uint8)
        coff = np.full(D, -1, np.int64)
        rows = (ResRow * D)()
        run = Run(C.cast(rows, C.c_void_p), D, 0, Assembly(_p(o["cover"]), _p(o["aln_len"]), _p(o["depth"]), _p(o["asm_len"]), _p(cbuf), _p(coff), cap, 0),
                  None, None, None, None)
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        with conclave_version(conclave), self._counting(count_kmers):
            _check(lib().kmahip_run_pe(self.h, self.ws, C.byref(rb), C.byref(p), float(evalue), int(bcd), int(max_frag),
                                       os.fsencode(frag_path) if frag_path else None, C.byref(run)))
        o["rows"] = [rows[i] for i in range(run.n_rows)]
        raw = cbuf.tobytes()
        o["consensus"] = {t: raw[coff[t]:raw.index(b"\0", coff[t])].decode() for t in range(D) if coff[t] >= 0}
        o["ms"] = list(run.ms)
        return o

    def frag_write(self, path, batch, rc, tmpl, n_hits, stats, read_names, max_frag=0):
        """`.frag.gz` of the traced reads (kmahip_frag_write); read_names = list[bytes] (Ingest.next) -> number of rows"""
        n = batch.n
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        fl = np.ascontiguousarray(rc if n else np.zeros(1, np.int32), np.int32)
        tm = np.ascontiguousarray(tmpl if n else np.zeros(1, np.int32), np.int32)
        nh = np.ascontiguousarray(n_hits if n else np.zeros(1, np.int32), np.int32)
        st = np.ascontiguousarray(stats if n else np.zeros((1, 10), np.int32), np.int32)
        blob = b"".join(nm + b"\0" for nm in read_names) + b"\0"
        noff = np.zeros(n + 1, np.int64)
        if n:
            noff[1:] = np.cumsum([len(nm) + 1 for nm in read_names])
        rows = C.c_int64()
        _check(lib().kmahip_frag_write(os.fsencode(path), self.h, C.byref(r), _p(fl), _p(tm), _p(nh), _p(st), int(max_frag), blob,
                                       _p(noff), C.byref(rows)))
        return rows.value

    def assemble_ef(self, tmpl, traces, asm, flag=None):
        """The extended features of the pile-up the last assemble() call on this database left in HBM (kmahip_assemble_ef; host arrays):
        tmpl and traces as given there, asm = what it returned (its depth is read), flag = the frag_raw flag per read or None.
        -> dict(depth_var, snp_sum, insert_sum, deletion_sum, score_sum [u64], max_depth, nuc_high_var, read_count_aln, fragment_count_aln
        [u32], var [f64]), DB_size entries each"""
        n = len(tmpl)
        tm = np.ascontiguousarray(tmpl if n else np.zeros(1, np.int32), np.int32)
        st = np.ascontiguousarray(traces[0] if n else np.zeros((1, 10), np.int32), np.int32)
        fl = None if flag is None else np.ascontiguousarray(flag if n else np.zeros(1, np.int32), np.int32)
        tr = Traces(_p(st), None, None, None, 0)
        D = int(self.info.DB_size)
        depth = np.ascontiguousarray(asm["depth"], np.int64)
        a = Assembly(None, None, _p(depth), None, None, None, 0, 0)
        o = {k: np.zeros(D, np.uint64) for k in ("depth_var", "snp_sum", "insert_sum", "deletion_sum", "score_sum")}
        o.update({k: np.zeros(D, np.uint32) for k in ("max_depth", "nuc_high_var", "read_count_aln", "fragment_count_aln")})
        o["var"] = np.zeros(D, np.float64)
        e = AssemblyEf(*[_p(o[k]) for k in ("depth_var", "snp_sum", "insert_sum", "deletion_sum", "max_depth", "nuc_high_var", "score_sum", "read_count_aln",
                                            "fragment_count_aln", "var")])
        p = Params.from_buffer_copy(self.params)
        _check(lib().kmahip_assemble_ef(self.h, self.ws, n, _p(tm), C.byref(tr), None if fl is None else _p(fl), C.byref(p), C.byref(a), C.byref(e)))
        return o

    def assemble_matrix(self, mask, chunk_bytes=0):
        """The count-matrix rows (`-matrix`) of the pile-up the last assemble() call on this database left in HBM, for the templates with
        mask[t] != 0 (kmahip_assemble_matrix_dev). -> (the rows of all those templates as bytes, templates ascending; bytes per template [i64])"""
        D = int(self.info.DB_size)
        m = np.ascontiguousarray(mask, np.uint8)
        assert len(m) == D
        per = np.zeros(D, np.int64)
        parts = []

        def take(user, text, n):
            parts.append(C.string_at(text, n))
            return 0
        cb = TEXT_SINK(take)
        _check(lib().kmahip_assemble_matrix_dev(self.h, self.ws, _p(m), int(chunk_bytes), _p(per), cb, None))
        return b"".join(parts), per

    def assemble_vcf(self, mask):
        """The records of the rows `-vcf` prints, chosen on the device (kmahip_assemble_vcf_dev) -> (records [VCF_REC], records per template [i64])"""
        D = int(self.info.DB_size)
        m = np.ascontiguousarray(mask, np.uint8)
        assert len(m) == D
        per = np.zeros(D, np.int64)
        n = C.c_int64(0)
        _check(lib().kmahip_assemble_vcf_dev(self.h, self.ws, _p(m), _p(per), None, 0, C.byref(n)))
        recs = np.zeros(max(n.value, 1), VCF_REC)
        if n.value:
            _check(lib().kmahip_assemble_vcf_dev(self.h, self.ws, _p(m), _p(per), _p(recs), n.value, C.byref(n)))
        return recs[:n.value], per

    @staticmethod
    def vcf_header(t_db):
        """The header lines of `<out>.vcf.gz` (kmahip_vcf_header) as bytes"""
        buf = C.create_string_buffer(4096 + len(t_db))
        n = lib().kmahip_vcf_header(os.fsencode(t_db), buf, len(buf))
        return buf.raw[:n]

    @staticmethod
    def vcf_line(name, rec, evalue=0.05, support=0.0, bcd=1, filter=1, cap=None):
        """One row of `<out>.vcf.gz` (kmahip_vcf_line) as bytes, b"" when it does not fit `cap`. rec: a VcfRec, an element of a VCF_REC
        array, or (pos, ref, call, best_score, counts)"""
        if isinstance(rec, tuple):
            pos, ref, call, best, counts = rec
            rec = VcfRec(0, int(pos), ord(ref), ord(call), 0, int(best), (C.c_uint32 * 6)(*[int(x) for x in counts]))
        elif not isinstance(rec, VcfRec):
            rec = VcfRec(int(rec["tmpl"]), int(rec["pos"]), int(rec["ref"]), int(rec["call"]), 0, int(rec["best_score"]), (C.c_uint32 * 6)(*[int(x) for x in rec["counts"]]))
        cap = 4096 + len(name) if cap is None else int(cap)
        buf = C.create_string_buffer(max(cap, 1))
        n = lib().kmahip_vcf_line(name.encode(), C.byref(rec), float(evalue), float(support), int(bcd), int(filter), buf, cap)
        return buf.raw[:n]

    @staticmethod
    def mapstat_header(t_db, fragment_count, cmdline=None):
        """The header lines of `<out>.mapstat` (kmahip_mapstat_header) as bytes"""
        buf = C.create_string_buffer(4096 + len(t_db) + len(cmdline or ""))
        n = lib().kmahip_mapstat_header(os.fsencode(t_db), int(fragment_count), None if cmdline is None else cmdline.encode(), buf, len(buf))
        return buf.raw[:n]

    @staticmethod
    def mapstat_line(name, row, cover, aln_len, depth, ef, ID_t=1.0, Depth_t=0.0):
        """The `.mapstat` row (kmahip_mapstat_line; ef: a MapstatRow), or None where res_line gives None"""
        buf = C.create_string_buffer(4096 + len(name))
        n = lib().kmahip_mapstat_line(name.encode(), C.byref(row), int(cover), int(aln_len), int(depth), ID_t, Depth_t, C.byref(ef), buf, len(buf))
        return buf.raw[:n].decode() if n else None

    @staticmethod
    def res_line(name, row, cover, aln_len, depth, ID_t=1.0, Depth_t=0.0):
        """The `.res` row as the reference prints it, or None when it prints none"""
        buf = C.create_string_buffer(4096 + len(name))
        n = lib().kmahip_res_line(name.encode(), C.byref(row), int(cover), int(aln_len), int(depth), ID_t, Depth_t, buf, len(buf))
        return buf.raw[:n].decode() if n else None

    def res_rows(self, w_scores, evalue=0.05, scoreT=0.5):
        """Leading `.res` columns per template with a score -> list of ResRow (host arithmetic, runkma.c:765-783)"""
        w = np.ascontiguousarray(w_scores, np.uint64)
        cap = int((w[1:] > 0).sum()) + 1
        rows = (ResRow * cap)()
        n = C.c_int64()
        _check(lib().kmahip_res_rows(self.h, _p(w), C.c_double(evalue), C.c_double(scoreT), rows, cap, C.byref(n)))
        return [rows[i] for i in range(n.value)]

    # -- paired end stage 2 (-apm p), host buffers ------------------------------------
    def scan_pe(self, batch, exhaustive=0, t_cap=None, count_kmers=False):
        """batch = mates interleaved (read 2i, 2i+1 = pair i) -> mate, rc, rc_flag, flag [2*pairs], R_off, T. count_kmers (-ck): the
        candidates of a mate score one point per k-mer (get_kmers_for_pair_count); the pairing is the same"""
        n = batch.n
        assert n % 2 == 0
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        mate, rc, rc_flag, flag = (np.zeros(max(n, 1), np.int32) for _ in range(4))
        R_off = np.zeros(n + 1, np.int64)
        cap = t_cap or max(1024, 16 * n)
        p = Params.from_buffer_copy(self.params)
        p.exhaustive = exhaustive
        for _ in range(6):
            T = np.zeros(cap, np.int32)
            out = PeRecs(_p(mate), _p(rc), _p(rc_flag), _p(flag), _p(R_off), _p(T), cap)
            with self._counting(count_kmers):
                rcode = lib().kmahip_scan_pe(self.h, self.ws, C.byref(r), C.byref(p), C.byref(out))
            if rcode == -6:
                cap = max(cap * 2, int(R_off[n]) + 16)
                continue
            _check(rcode)
            return mate[:n], rc[:n], rc_flag[:n], flag[:n], R_off, T[:R_off[n]]
        raise KmaHipError("scan_pe: output capacity kept overflowing")

    def map_pe(self, batch, exhaustive=0, t_cap=None, circular=False, count_kmers=False):
        """Stages 2 + 3a for interleaved mates -> (mate, rc, rc_flag, flag, R_off, T), hits dict (+ "kind" per pair)"""
        n = batch.n
        assert n % 2 == 0
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        r = Reads(n, _p(seq), _p(batch.seq_off), _p(batch.length), _p(Nn), _p(batch.N_off), len(seq), len(batch.N),
                  int(batch.length.max()) if n else 0)
        mate, rc, rc_flag, flag = (np.zeros(max(n, 1), np.int32) for _ in range(4))
        R_off = np.zeros(n + 1, np.int64)
        cap = t_cap or max(1024, 16 * n)
        p = Params.from_buffer_copy(self.params)
        if circular:
            p.ca = 1          # -ca: chainSeeds_circular (chain.c:262, kma.c:722)
        p.exhaustive = exhaustive
        D = int(self.info.DB_size)
        for _ in range(6):
            T = np.zeros(cap, np.int32)
            h = dict(n_hits=np.zeros(max(n, 1), np.int32), best_score=np.zeros(max(n, 1), np.int32),
                     flag=np.zeros(max(n, 1), np.int32), tmpl=np.zeros(cap, np.int32), score=np.zeros(cap, np.int32),
                     start=np.zeros(cap, np.int32), end=np.zeros(cap, np.int32), kind=np.zeros(max(n // 2, 1), np.int32),
                     alignment_scores=np.zeros(D, np.uint64), uniq_alignment_scores=np.zeros(D, np.uint64),
                     rc=np.zeros(max(n, 1), np.int32))
            out = PeRecs(_p(mate), _p(rc), _p(rc_flag), _p(flag), _p(R_off), _p(T), cap)
            hs = Hits(_p(h["n_hits"]), _p(h["best_score"]), _p(h["flag"]), _p(h["tmpl"]), _p(h["score"]), _p(h["start"]),
                      _p(h["end"]), _p(h["alignment_scores"]), _p(h["uniq_alignment_scores"]), _p(h["rc"]))
            with self._counting(count_kmers):
                rcode = lib().kmahip_map_pe(self.h, self.ws, C.byref(r), C.byref(p), C.byref(out), C.byref(hs), _p(h["kind"]))
            if rcode == -6:
                cap = max(cap * 2, int(R_off[n]) + 16)
                continue
            _check(rcode)
            return (mate[:n], rc[:n], rc_flag[:n], flag[:n], R_off, T[:R_off[n]]), h
        raise KmaHipError("map_pe: output capacity kept overflowing")


class SparseInfo(C.Structure):
    _fields_ = [("DB_size", C.c_uint32), ("kmersize", C.c_uint32), ("prefix_len", C.c_uint32), ("values_u16", C.c_uint32),
                ("prefix", C.c_uint64), ("n_kmers", C.c_uint64), ("n_hdr", C.c_uint64), ("n_values", C.c_uint64), ("total_bytes", C.c_uint64)]


class SparseOpts(C.Structure):
    _fields_ = [("ID_t", C.c_double), ("Depth_t", C.c_double), ("evalue", C.c_double), ("ss", C.c_int32), ("pad_", C.c_int32)]


class SparseRow(C.Structure):
    _fields_ = [("tmpl", C.c_int32), ("expected", C.c_int32), ("score", C.c_uint64), ("ulen", C.c_uint32), ("pad_", C.c_uint32),
                ("query_cover", C.c_double), ("cover", C.c_double), ("depth", C.c_double), ("tot_query_cover", C.c_double),
                ("tot_cover", C.c_double), ("tot_depth", C.c_double), ("q_value", C.c_double), ("p_value", C.c_double)]


class SparseDB:
    """Sparse mapping (`kma -Sparse`; kmahip_sparse_*): a sparse index (`kma index -Sparse`) resident in HBM with the k-mer counts of
    the reads given so far. count() adds a batch; rows() / write() rank and name the templates like save_kmers_sparse_batch."""

    def __init__(self, prefix: str, device: int = 0):
        L = lib()
        if not hasattr(L, "kmahip_sparse_open"):
            raise KmaHipError("this libkmahip.so has no sparse mapping (kmahip_sparse_open)")
        L.kmahip_sparse_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.kmahip_sparse_close.argtypes = [C.c_void_p]
        L.kmahip_sparse_close.restype = None
        L.kmahip_sparse_get_info.argtypes = [C.c_void_p, C.POINTER(SparseInfo)]
        L.kmahip_sparse_template.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.kmahip_sparse_count.argtypes = [C.c_void_p, C.POINTER(Reads)]
        L.kmahip_sparse_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.kmahip_sparse_collect.argtypes = [C.c_void_p]
        L.kmahip_sparse_withdraw.argtypes = [C.c_void_p, C.c_int32]
        L.kmahip_sparse_scores.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.kmahip_sparse_default_opts.argtypes = [C.POINTER(SparseOpts)]
        L.kmahip_sparse_default_opts.restype = None
        L.kmahip_sparse_rows.argtypes = [C.c_void_p, C.POINTER(SparseOpts), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.kmahip_sparse_write.argtypes = [C.c_void_p, C.POINTER(SparseOpts), C.c_char_p]
        L.kmahip_sparse_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.kmahip_sparse_get_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.kmahip_sparse_set_noadd.argtypes = [C.c_void_p, C.c_int]
        self.h = C.c_void_p()
        _check(L.kmahip_init(device))
        _check(L.kmahip_sparse_open(os.fsencode(prefix), C.byref(self.h)))
        self.prefix = prefix
        self.info = SparseInfo()
        _check(L.kmahip_sparse_get_info(self.h, C.byref(self.info)))

    def close(self):
        if getattr(self, "h", None):
            lib().kmahip_sparse_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def template(self, t):
        """-> (name bytes, length, unique length) of template t"""
        name, ln, ul = C.c_char_p(), C.c_uint32(), C.c_uint32()
        _check(lib().kmahip_sparse_template(self.h, int(t), C.byref(name), C.byref(ln), C.byref(ul)))
        return name.value, ln.value, ul.value

    def count(self, batch):
        """add the k-mers of a formats.ReadBatch (both strands) to the counts"""
        n = batch.n
        if n == 0:
            return
        seq = np.ascontiguousarray(batch.seq, np.uint64)
        Nn = np.ascontiguousarray(batch.N if len(batch.N) else np.zeros(1, np.int32), np.int32)
        seq_off, length, N_off = (np.ascontiguousarray(a, d) for a, d in ((batch.seq_off, np.int64), (batch.length, np.int32), (batch.N_off, np.int64)))
        r = Reads(n, _p(seq), _p(seq_off), _p(length), _p(Nn), _p(N_off), len(seq), len(batch.N), int(length.max()))
        _check(lib().kmahip_sparse_count(self.h, C.byref(r)))

    def count_dev(self, seq, seq_off, length, N, N_off):
        """count() on CUDA(HIP) torch tensors (u64 words as int64, int64, int32, int32, int64), every read followed by its pad word
        (the layout of formats.ReadBatch); asynchronous on the null stream"""
        n = length.numel()
        if n == 0:
            return
        L = lib()
        L.kmahip_sparse_count_dev.argtypes = [C.c_void_p, C.POINTER(Reads)]
        r = Reads(n, seq.data_ptr(), seq_off.data_ptr(), length.data_ptr(), N.data_ptr(), N_off.data_ptr(), seq.numel(), N.numel(), 0)
        _check(L.kmahip_sparse_count_dev(self.h, C.byref(r)))

    def counts(self):
        """-> (keys u32[n_kmers], counts u32[n_kmers], Ntot): the count of every k-mer of the index, in the order of its ids"""
        n = int(self.info.n_kmers)
        keys, cnt, ntot = np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint32), C.c_uint64()
        _check(lib().kmahip_sparse_counts(self.h, _p(keys), _p(cnt), C.byref(ntot)))
        return keys[:n], cnt[:n], int(ntot.value)

    def collect(self):
        """collect_Kmers: the scores from the counts; the working copies start from them"""
        _check(lib().kmahip_sparse_collect(self.h))

    def withdraw(self, t):
        """withDraw_Kmers on the working copies"""
        _check(lib().kmahip_sparse_withdraw(self.h, int(t)))

    def scores(self, working=False):
        """-> (Scores u32[DB_size], Scores_tot u64[DB_size], (Nhits.n, Nhits.tot)) of the last collect(), or the working copies.
        Collects first when the counts changed since."""
        D = int(self.info.DB_size)
        sc, tot, hits = np.zeros(D, np.uint32), np.zeros(D, np.uint64), np.zeros(2, np.uint64)
        rc = lib().kmahip_sparse_scores(self.h, 1 if working else 0, _p(sc), _p(tot), _p(hits))
        if rc == -1 and not working:
            self.collect()
            rc = lib().kmahip_sparse_scores(self.h, 0, _p(sc), _p(tot), _p(hits))
        _check(rc)
        return sc, tot, (int(hits[0]), int(hits[1]))

    @staticmethod
    def _opts(ss, id_t, depth_t, evalue):
        o = SparseOpts()
        lib().kmahip_sparse_default_opts(C.byref(o))
        o.ss = ord(ss)
        if id_t is not None:
            o.ID_t = float(id_t)
        if depth_t is not None:
            o.Depth_t = float(depth_t)
        if evalue is not None:
            o.evalue = float(evalue)
        return o

    def rows(self, ss="q", id_t=None, depth_t=None, evalue=None):
        """the rows of <out>.spa as tuples (template, score, expected, unique length, query cover, cover, depth, tot query cover,
        tot cover, tot depth, q_value, p_value)"""
        o = self._opts(ss, id_t, depth_t, evalue)
        cap = int(self.info.DB_size)
        buf = (SparseRow * max(1, cap))()
        n = C.c_int64()
        _check(lib().kmahip_sparse_rows(self.h, C.byref(o), buf, cap, C.byref(n)))
        return [(r.tmpl, r.score, r.expected, r.ulen, r.query_cover, r.cover, r.depth, r.tot_query_cover, r.tot_cover, r.tot_depth, r.q_value, r.p_value)
                for r in buf[:n.value]]

    def write(self, path, ss="q", id_t=None, depth_t=None, evalue=None):
        """<out>.spa, byte for byte the reference's"""
        o = self._opts(ss, id_t, depth_t, evalue)
        _check(lib().kmahip_sparse_write(self.h, C.byref(o), os.fsencode(path)))

    def set_timing(self, on=True):
        _check(lib().kmahip_sparse_set_timing(self.h, 1 if on else 0))

    def get_timing(self, kernel):
        """(milliseconds, launches) of kernel 0 count, 1 collect, 2 withdraw since the last call"""
        ms, n = C.c_double(), C.c_int64()
        _check(lib().kmahip_sparse_get_timing(self.h, int(kernel), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_noadd(self, on=True):
        """timing only: the counting kernel keeps its probes and drops its adds (the counts are wrong by design)"""
        _check(lib().kmahip_sparse_set_noadd(self.h, 1 if on else 0))


class TdistInfo(C.Structure):
    _fields_ = [("DB_size", C.c_uint32), ("mlen", C.c_uint32), ("kmersize", C.c_uint32), ("flag", C.c_uint32), ("prefix_len", C.c_uint32),
                ("direct", C.c_uint32), ("value_bytes", C.c_uint32), ("form", C.c_uint32),
                ("n_kmers", C.c_uint64), ("n_lists", C.c_uint64), ("n_values", C.c_uint64), ("name_bytes", C.c_uint64), ("total_bytes", C.c_uint64)]


def _tdist_lib():
    L = lib()
    if not hasattr(L, "kmahip_tdist_open"):
        raise KmaHipError("this libkmahip.so has no template distances (kmahip_tdist_open)")
    L.kmahip_tdist_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.kmahip_tdist_open_lists.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
    L.kmahip_tdist_close.argtypes = [C.c_void_p]
    L.kmahip_tdist_close.restype = None
    L.kmahip_tdist_get_info.argtypes = [C.c_void_p, C.POINTER(TdistInfo)]
    L.kmahip_tdist_name.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p)]
    L.kmahip_tdist_count.argtypes = [C.c_void_p]
    L.kmahip_tdist_get_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.kmahip_tdist_write.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    L.kmahip_tdist_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.kmahip_tdist_get_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.kmahip_test_tdist_cells.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return L


def tdist_cells(method, Ni, Nj, D):
    """kmahip_test_tdist_cells (a test hook): the cells of one distance measure (`kma dist -d method`) for explicit triples, formatted
    on the device -> list of 11-byte strings"""
    a, b, d = (np.ascontiguousarray(x, np.int32) for x in (Ni, Nj, D))
    assert a.shape == b.shape == d.shape and a.ndim == 1
    out = np.zeros(11 * max(1, len(a)), np.uint8)
    _check(_tdist_lib().kmahip_test_tdist_cells(int(method), _p(a), _p(b), _p(d), len(a), _p(out)))
    raw = out.tobytes()
    return [raw[11 * i:11 * i + 11] for i in range(len(a))]


class TemplateDist:
    """Template distances (`kma dist`; kmahip_tdist_*): the value lists of <prefix>.comp.b (any form of index the reference writes)
    resident in HBM. count() counts, for every pair of templates, the k-mers they share; write() formats the PHYLIP matrices."""

    def __init__(self, prefix=None, device: int = 0, _handle=None):
        L = _tdist_lib()
        self.h = C.c_void_p()
        if _handle is not None:
            self.h = _handle
        else:
            _check(L.kmahip_init(device))
            _check(L.kmahip_tdist_open(os.fsencode(prefix), C.byref(self.h)))
        self.prefix = prefix
        self.info = TdistInfo()
        _check(L.kmahip_tdist_get_info(self.h, C.byref(self.info)))
        self.n = int(self.info.DB_size) - 1

    @classmethod
    def from_lists(cls, n_templates, offsets, values, value_bytes=2, device: int = 0):
        """the same object over explicit arrays: offsets[k] = where k-mer k's list stands in values (1 = none), values the lists as
        [length, ids ...] with ids 1 .. n_templates, stored 16- or 32-bit; the templates are named by their ids"""
        L = _tdist_lib()
        off = np.ascontiguousarray(offsets, np.uint32)
        val = np.ascontiguousarray(values, np.uint16 if value_bytes == 2 else np.uint32)
        h = C.c_void_p()
        _check(L.kmahip_init(device))
        _check(L.kmahip_tdist_open_lists(int(n_templates), len(off), _p(off) if len(off) else None, _p(val) if len(val) else None, int(value_bytes), len(val), C.byref(h)))
        return cls(_handle=h)

    def close(self):
        if getattr(self, "h", None):
            lib().kmahip_tdist_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def name(self, t):
        nm = C.c_char_p()
        _check(lib().kmahip_tdist_name(self.h, int(t), C.byref(nm)))
        return nm.value

    def count(self):
        """kmerSimilarity on the device (KMAHIP_TDIST_FORM = rows | pairs) -> the form used"""
        L = lib()
        _check(L.kmahip_tdist_count(self.h))
        _check(L.kmahip_tdist_get_info(self.h, C.byref(self.info)))
        return "pairs" if self.info.form else "rows"

    def counts(self, row_lo=0, row_hi=None):
        """-> (N int32[n], the rows row_lo <= hi < row_hi of the lower triangle, row hi holding hi cells, one after the other)"""
        row_hi = self.n if row_hi is None else int(row_hi)
        row_lo = int(row_lo)
        cells = row_hi * max(0, row_hi - 1) // 2 - row_lo * max(0, row_lo - 1) // 2
        N, D = np.zeros(max(1, self.n), np.int32), np.zeros(max(1, cells), np.int32)
        _check(lib().kmahip_tdist_get_counts(self.h, _p(N), _p(D), row_lo, row_hi))
        return N[:self.n], D[:cells]

    def write(self, path, methods=1, fmt=1):
        """the file of `kma dist -d methods -f fmt`"""
        _check(lib().kmahip_tdist_write(self.h, os.fsencode(path), int(methods), int(fmt)))

    def set_timing(self, on=True):
        _check(lib().kmahip_tdist_set_timing(self.h, 1 if on else 0))

    def get_timing(self, kernel):
        """(milliseconds, launches) of kernel 0 mult, 1 inverted index, 2 rows, 3 pairs, 4 write since the last call"""
        ms, n = C.c_double(), C.c_int64()
        _check(lib().kmahip_tdist_get_timing(self.h, int(kernel), C.byref(ms), C.byref(n)))
        return ms.value, n.value
