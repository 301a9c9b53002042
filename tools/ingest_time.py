#!/usr/bin/env python3
"""Stage 1 on the host against stage 1 on the device, on one seeded FASTQ file, in ONE call (GPU box):

  (a) host reader   kmahip_ingest_open -> last batch delivered, each batch uploaded with kmahip_session_upload
  (b) device reader kmahip_ingest_dev_open -> last batch resident (kmahip_session_upload_dev) and the stream synchronised

alternating, REPS repetitions each after one warm-up of each; medians and spreads, the device reader's own split (file read,
waiting for copies, kernels + scans), input bytes per second against the rate of a plain pinned host-to-device copy measured
in the same call. Then examples/kmahip_map -1t1 on the same file as fresh child processes, with and without -s1dev, alternating:
whole-process wall and the program's own "ingest done after" figure. The device reader's split is the reader's own host clock
(kmahip_ingest_dev_timing): file_read = the preads into pinned memory (copies of earlier pieces run behind them), copy_wait = only what
of the copies was still outstanding after the last pread of a chunk, kernels_scans = the rest of the calls; kernel time proper comes
from the rocprofv3 run of --only-dev. Writes profiles/ingest_dev_time.json (or --out).

usage: python3 tools/ingest_time.py [--reads 10000000] [--pairs 1000000] [--reps 5] [--out profiles/ingest_dev_time.json] [--dir DIR]
       python3 tools/ingest_time.py --only-dev ...      (one warm-up and one run of (b) alone: the run to put under rocprofv3)"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kma_amd import binding, formats, synth  # noqa: E402

MAP = os.path.join(ROOT, "examples", "kmahip_map")


def write_reads(path, seqs, n, L, seed, name):
    """n reads of L bases cut from the genes (1 % substitutions), qualities 'I' with a low-quality tail of 1-11 bases on a third of
    them, names of a fixed width: records of one size, made a block at a time as a byte matrix"""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    genes = [np.asarray(g, np.uint8) for g in seqs if len(g) > L + 10]
    cat = np.concatenate(genes)
    g0 = np.cumsum([0] + [len(g) for g in genes[:-1]])
    room = np.array([len(g) - L for g in genes])
    W = 9                                            # digits of a name
    reclen = 1 + len(name) + W + 1 + L + 3 + L + 1
    with open(path, "wb") as f:
        done = 0
        while done < n:
            m = min(500000, n - done)
            gi = rng.integers(0, len(genes), m)
            a = g0[gi] + (rng.random(m) * room[gi]).astype(np.int64)
            codes = cat[a[:, None] + np.arange(L)[None, :]] & 3
            sub = rng.random((m, L), dtype=np.float32) < 0.01
            codes = np.where(sub, (codes + 1) & 3, codes)
            rec = np.empty((m, reclen), np.uint8)
            rec[:, 0] = ord("@")
            rec[:, 1:1 + len(name)] = np.frombuffer(name, np.uint8)
            ids = np.arange(done, done + m)
            for d in range(W):
                rec[:, 1 + len(name) + d] = ord("0") + (ids // 10 ** (W - 1 - d)) % 10
            o = 1 + len(name) + W
            rec[:, o] = ord("\n")
            rec[:, o + 1:o + 1 + L] = lut[codes]
            rec[:, o + 1 + L:o + 4 + L] = np.frombuffer(b"\n+\n", np.uint8)
            q = rec[:, o + 4 + L:o + 4 + 2 * L]
            q[:] = ord("I")
            tail = np.where(ids % 3 == 0, rng.integers(1, 12, m), 0)
            q[np.arange(L)[None, :] >= (L - tail)[:, None]] = ord("#")
            rec[:, -1] = ord("\n")
            rec.tofile(f)
            done += m


class ShardOpts(C.Structure):                      # kmahip_shard_opts (include/kmahip.h)
    _fields_ = [("evalue", C.c_double), ("bcd", C.c_int32), ("caller", C.c_int32), ("sig90", C.c_int32), ("max_frag", C.c_int64),
                ("ID_t", C.c_double), ("Depth_t", C.c_double), ("support", C.c_double), ("ref_fsa", C.c_int32), ("write_aln", C.c_int32)]


def spread(xs):
    return {"median_s": statistics.median(xs), "min_s": min(xs), "max_s": max(xs), "all_s": xs}


def pinned_copy_rate(gb=1.0):
    hip = C.CDLL("libamdhip64.so")
    n = int(gb * (1 << 30))
    h, d = C.c_void_p(), C.c_void_p()
    assert hip.hipHostMalloc(C.byref(h), C.c_size_t(n), 0) == 0 and hip.hipMalloc(C.byref(d), C.c_size_t(n)) == 0
    C.memset(h, 1, n)
    ts = []
    for _ in range(4):
        t0 = time.perf_counter()
        assert hip.hipMemcpy(d, h, C.c_size_t(n), 1) == 0
        hip.hipDeviceSynchronize()
        ts.append(time.perf_counter() - t0)
    hip.hipFree(d)
    hip.hipHostFree(h)
    return gb * (1 << 30) / min(ts)


def session_for(db, paired):
    L = binding.lib()
    ses = C.c_void_p()
    L.kmahip_session_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    L.kmahip_session_upload.argtypes = [C.c_void_p, C.POINTER(binding.ReadBatchC)]
    L.kmahip_session_upload_dev.argtypes = [C.c_void_p, C.POINTER(binding.ReadBatchC)]
    L.kmahip_session_set_pe.argtypes = [C.c_void_p]
    L.kmahip_session_close.argtypes = [C.c_void_p]
    L.kmahip_session_close.restype = None
    p = binding.default_params()
    opts = ShardOpts()                             # zeroed: only uploads happen here
    binding._check(L.kmahip_session_open(db.h, db.ws, C.byref(p), C.byref(opts), 1000, C.byref(ses)))
    if paired:
        binding._check(L.kmahip_session_set_pe(ses))
    return ses


def one_host(db, p1, p2, batch):
    L = binding.lib()
    ses = session_for(db, p2 is not None)
    t0 = time.perf_counter()
    t = binding.Trim(20, 0, 0, 16, 2**31 - 1)
    h = C.c_void_p()
    binding._check(L.kmahip_ingest_open(os.fsencode(p1), os.fsencode(p2) if p2 else None, C.byref(t), C.byref(h)))
    n = 0
    while True:
        b = binding.ReadBatchC()
        binding._check(L.kmahip_ingest_next(h, batch, C.byref(b)))
        if b.reads.n_reads == 0:
            break
        binding._check(L.kmahip_session_upload(ses, C.byref(b)))
        n += b.reads.n_reads
    dt = time.perf_counter() - t0
    L.kmahip_ingest_close(h)
    L.kmahip_session_close(ses)
    return dt, n


def one_dev(db, p1, p2, batch):
    L = binding.lib()
    ses = session_for(db, p2 is not None)
    t0 = time.perf_counter()
    ing = binding.IngestDev(p1, p2)
    n = 0
    while True:
        b = ing.next_dev(batch)
        if b is None:
            break
        binding._check(L.kmahip_session_upload_dev(ses, C.byref(b)))          # (synchronises before it returns)
        n += b.reads.n_reads
    dt = time.perf_counter() - t0
    split = ing.timing()
    assert ing.handed_back == 0
    ing.close()
    L.kmahip_session_close(ses)
    return dt, n, split


def map_runs(args, reps):
    out = {"host": {"wall": [], "ingest_done": []}, "s1dev": {"wall": [], "ingest_done": []}}
    for r in range(reps + 1):                       # (the first round of each is the warm-up)
        for mode in ("host", "s1dev"):
            t0 = time.perf_counter()
            p = subprocess.run([MAP] + args + (["-s1dev"] if mode == "s1dev" else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            dt = time.perf_counter() - t0
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            m = re.search(rb"ingest done after ([0-9.]+)", p.stderr)
            if r:
                out[mode]["wall"].append(dt)
                out[mode]["ingest_done"].append(float(m.group(1)) if m else None)
    return {k: {"wall": spread(v["wall"]), "ingest_done_s": v["ingest_done"]} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_dev_time.json"))
    ap.add_argument("--dir", default=None)
    ap.add_argument("--no-map", action="store_true")
    ap.add_argument("--only-dev", action="store_true")
    a = ap.parse_args()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    res = {"reads": a.reads, "pairs": a.pairs, "reps": a.reps, "batch": a.batch}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        names, seqs = synth.make_gene_db(n_families=40, variants=5, seed=77)
        prefix = os.path.join(tmp, "db")
        formats.write_index(prefix, names, seqs)
        se = os.path.join(tmp, "reads.fq")
        r1, r2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        t0 = time.perf_counter()
        write_reads(se, seqs, a.reads, 150, 1, b"r")
        if not a.only_dev:
            write_reads(r1, seqs, a.pairs, 150, 2, b"p")
            write_reads(r2, seqs, a.pairs, 150, 3, b"p")
        print(f"# inputs written in {time.perf_counter() - t0:.1f} s", flush=True)
        db = binding.KmaHipDB(prefix, device=0)
        if a.only_dev:
            for _ in range(2):
                print("# device reader alone: %.3f s, %d reads, split %s" % one_dev(db, se, None, a.batch), flush=True)
            db.close()
            return
        res["input_bytes"] = {"se": os.path.getsize(se), "pe": os.path.getsize(r1) + os.path.getsize(r2)}
        res["pinned_h2d_bytes_per_s"] = pinned_copy_rate()
        for label, p1, p2 in (("se", se, None), ("pe", r1, r2)):
            host, dev, splits = [], [], []
            for r in range(a.reps + 1):             # (round 0 warms both up)
                th, nh = one_host(db, p1, p2, a.batch)
                td, nd, sp = one_dev(db, p1, p2, a.batch)
                assert nh == nd, (nh, nd)
                if r:
                    host.append(th)
                    dev.append(td)
                    splits.append(sp)
            nbytes = res["input_bytes"][label]
            res[label] = {"kept_reads": nh, "host_reader": spread(host), "device_reader": spread(dev),
                          "device_split_ms": {"file_read": statistics.median(s[0] for s in splits), "copy_wait": statistics.median(s[1] for s in splits),
                                              "kernels_scans": statistics.median(s[2] for s in splits)},
                          "device_input_bytes_per_s": nbytes / statistics.median(dev)}
            print(f"# {label}: host {statistics.median(host):.3f} s  device {statistics.median(dev):.3f} s  split {res[label]['device_split_ms']}", flush=True)
        db.close()
        if not a.no_map:
            res["kmahip_map_se"] = map_runs(["-i", se, "-t_db", prefix, "-o", os.path.join(tmp, "o"), "-1t1"], a.reps)
            print(f"# kmahip_map: {res['kmahip_map_se']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
