#!/usr/bin/env python3
"""The counting scan (`-ck`) timed on one MI355X: warm-up, five runs, median and range of each figure.

  kernels   the first-tier kernel of stage 2 on the benchmark's input (10 M reads of 150 bases against 5 k genes, resident in HBM),
            scan_count_kernel next to scan_se_kernel, with the prefilter of each launch (HIP events, KmaHipDB.set_timing), and the
            whole stage-2 call by the wall clock
  e2e       file to file: examples/kmahip_map -1t1 -ck against oracle/_ref/kma -1t1 -ck on the same FASTQ and host; the reference
            as one process with 16 threads and as 16 independent -t 1 processes over equal shards, the better of the two

usage (GPU box): python3 tools/ck_time.py [kernels|e2e|both] [reads] [e2e reads]      -> one JSON document on stdout"""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kma_amd import binding, formats, synth  # noqa: E402

RUNS = 5


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "runs": [round(x, 3) for x in xs]}


def kernels(prefix, seqs, n):
    import torch
    from kma_amd import synth_dev
    dev = torch.device("cuda", 0)
    db = binding.KmaHipDB(prefix)
    rd = synth_dev.make_packed_reads(seqs, n, seed=1000, device=dev)
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)  # noqa: E731
    rc_flag, flag, T_off, T = i32(n), i32(n), torch.empty(n + 1, dtype=torch.int64, device=dev), i32(8 * n)
    out = {"reads": n, "unit": "ms"}
    for name, ck in (("plain", 0), ("ck", 1), ("plain_again", 0)):
        db.set_count_kmers(bool(ck))
        scan = lambda: db.scan_se_dev(rd["seq"], rd["seq_off"], rd["length"], rd["N"], rd["N_off"], rc_flag, flag, T_off, T)  # noqa: E731
        scan()
        torch.cuda.synchronize()
        first, pre, wall = [], [], []
        for _ in range(RUNS):
            db.set_timing(True)
            t0 = time.perf_counter()
            scan()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            first.append(db.get_timing(0)[0])
            pre.append(db.get_timing(2)[0])
            db.set_timing(False)
        out[name] = {"first_tier_kernel": summary(first), "prefilter": summary(pre), "stage2_call_wall": summary(wall),
                     "records": int((rc_flag != 0).sum().item()), "handed_on": db.get_scan_overflow()}
    db.set_count_kmers(False)
    db.close()
    return out


def e2e(prefix, seqs, n, tmp):
    import bench
    kma = os.path.join(ROOT, "oracle", "_ref", "kma")
    mapper = os.path.join(ROOT, "examples", "kmahip_map")
    fq = os.path.join(tmp, "ck.fq")
    with open(fq, "wb") as f:
        for a in range(0, n, 2_000_000):
            codes, _, _, _ = synth.make_reads(seqs, min(2_000_000, n - a), seed=1000 + a)
            part = os.path.join(tmp, "part.fq")
            bench.write_fastq_fixed(part, codes)
            with open(part, "rb") as g:
                shutil.copyfileobj(g, f, 1 << 24)
            os.unlink(part)
    rec = os.path.getsize(fq) // n
    out = {"reads": n, "unit": "s"}

    def wall(cmds):
        t0 = time.perf_counter()
        ps = [subprocess.Popen(c, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for c in cmds]
        rcs = [p.wait() for p in ps]
        assert all(r in (0, 2) for r in rcs), rcs          # (the reference ORs errno into its exit status)
        return time.perf_counter() - t0

    got = os.path.join(tmp, "got")
    ours = [mapper, "-i", fq, "-t_db", prefix, "-o", got, "-1t1", "-ck"]
    wall([ours])
    out["kmahip_map"] = summary([wall([ours]) for _ in range(RUNS)])
    shards = []
    per = (n + 15) // 16
    with open(fq, "rb") as f:
        for i in range(16):
            sl = os.path.join(tmp, "shard%02d.fq" % i)
            with open(sl, "wb") as g:
                g.write(f.read(rec * per))
            shards.append(sl)
    one = [kma, "-i", fq, "-t_db", prefix, "-o", os.path.join(tmp, "ref"), "-1t1", "-ck", "-t", "16"]
    many = [[kma, "-i", sl, "-t_db", prefix, "-o", sl + ".out", "-1t1", "-ck", "-t", "1"] for sl in shards]
    out["kma_t16"] = summary([wall([one]) for _ in range(RUNS)])
    out["kma_16_processes"] = summary([wall(many) for _ in range(RUNS)])
    out["same_res"] = open(got + ".res", "rb").read() == open(os.path.join(tmp, "ref.res"), "rb").read()
    best = min(out["kma_t16"]["median"], out["kma_16_processes"]["median"])
    out["speedup_over_the_reference_best"] = round(best / out["kmahip_map"]["median"], 2)
    return out


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    n_e2e = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000_000
    tmp = tempfile.mkdtemp(prefix="ck_time_")
    try:
        names, seqs = synth.make_gene_db(1000, 5, 600, 1500, 0.04, seed=12345)
        prefix = os.path.join(tmp, "db5k")
        formats.write_index(prefix, names, seqs)
        out = {}
        if what in ("kernels", "both"):
            out["kernels"] = kernels(prefix, seqs, n)
        if what in ("e2e", "both"):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
            out["e2e"] = e2e(prefix, seqs, n_e2e, tmp)
        print(json.dumps(out, indent=1))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
