#!/usr/bin/env python3
"""The QC report (-qc) and `kmahip_trim` timed on one MI355X host: a warm-up, five runs, median and range of each figure.
Input: 2 M reads of 150 bases, plain FASTQ, against 5 k genes.

  stage1    the device reader alone over the file (binding.IngestDev, batches of 2^20 records left on the device), without and with an
            accumulator: its kernels + scans + what comes back (timing()[2]), and of that the fetch of the counted sequences' (sp, len)
            and the host's adding and binning (qc_timing()) -- what is left of the difference is the cost of leaving the plain
            trimming path (phred_stat_dev for every read, s1_qc_kernel, one more scan)
  map       file to file: examples/kmahip_map -1t1 -s1dev without and with -qc; with --parent DIR (a tree holding the parent commit's
            examples/kmahip_map and kma_amd/libkmahip.so) the same run without -qc through the parent's program and library
  trim      examples/kmahip_trim -s1dev -qc and its host path against oracle/_ref/kma trim -qc on the same file and host

usage (GPU box): python3 tools/qc_time.py [--parent DIR] [reads]      -> one JSON document on stdout"""
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


def summary(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd), "runs": [round(x, nd) for x in xs]}


def wall(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
    return time.perf_counter() - t0


def stage1(fq):
    out = {"unit": "ms"}
    for name in ("plain", "qc", "plain_again"):
        kern, fetch, binning = [], [], []
        for run in range(RUNS + 1):
            qc = binding.QC() if name == "qc" else None
            with binding.IngestDev(fq, qc=qc) as ing:
                while ing.next_dev(1 << 20) is not None:
                    pass
                k = ing.timing()[2]
                f, b = ing.qc_timing()
            if qc is not None:
                out["sequences_counted"] = int(qc.stats()["count"])
                qc.close()
            if run:          # (the first run is the warm-up)
                kern.append(k); fetch.append(f); binning.append(b)
        out[name] = {"kernels_scans_and_figures": summary(kern)}
        if name == "qc":
            out[name]["fetch_of_sp_len"] = summary(fetch)
            out[name]["host_sum_and_bins"] = summary(binning)
    return out


def main():
    args = sys.argv[1:]
    parent = None
    if args and args[0] == "--parent":
        parent = os.path.abspath(args[1])
        args = args[2:]
    n = int(args[0]) if args else 2_000_000
    import bench
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    kma = os.path.join(ROOT, "oracle", "_ref", "kma")
    mapper, trimmer = os.path.join(ROOT, "examples", "kmahip_map"), os.path.join(ROOT, "examples", "kmahip_trim")
    tmp = tempfile.mkdtemp(prefix="qc_time_")
    try:
        names, seqs = synth.make_gene_db(1000, 5, 600, 1500, 0.04, seed=12345)
        prefix = os.path.join(tmp, "db5k")
        formats.write_index(prefix, names, seqs)
        fq = os.path.join(tmp, "reads.fq")
        codes, _, _, _ = synth.make_reads(seqs, n, seed=1000)
        bench.write_fastq_fixed(fq, codes)
        del codes
        out = {"reads": n, "read_length": 150, "fastq_bytes": os.path.getsize(fq), "runs": RUNS}
        out["stage1"] = stage1(fq)
        o = os.path.join(tmp, "o")
        runs = {"plain": [mapper, "-i", fq, "-t_db", prefix, "-o", o, "-1t1", "-s1dev"],
                "qc": [mapper, "-i", fq, "-t_db", prefix, "-o", o + "q", "-1t1", "-s1dev", "-qc"]}
        if parent:
            runs["parent_plain"] = [os.path.join(parent, "examples", "kmahip_map"), "-i", fq, "-t_db", prefix, "-o", o + "p", "-1t1", "-s1dev"]
        out["map"] = {"unit": "s"}
        for name, cmd in runs.items():
            wall(cmd)
        # (interleaved, so that a drift of the host touches every variant alike)
        times = {name: [] for name in runs}
        for _ in range(RUNS):
            for name, cmd in runs.items():
                times[name].append(wall(cmd))
        for name in runs:
            out["map"][name] = summary(times[name])
        if parent:
            out["map"]["parent_same_res"] = open(o + ".res", "rb").read() == open(o + "p.res", "rb").read()
        out["map"]["qc_same_res"] = open(o + ".res", "rb").read() == open(o + "q.res", "rb").read()
        trims = {"kmahip_trim_s1dev": [trimmer, "-i", fq, "-o", o + "t", "-qc", "-s1dev"],
                 "kmahip_trim_host": [trimmer, "-i", fq, "-o", o + "h", "-qc"],
                 "kma_trim": [kma, "trim", "-i", fq, "-o", o + "r", "-qc"]}
        out["trim"] = {"unit": "s"}
        for name, cmd in trims.items():
            wall(cmd)
            out["trim"][name] = summary([wall(cmd) for _ in range(RUNS)])
        same = all(open(o + "t" + e, "rb").read() == open(o + "r" + e, "rb").read() for e in (".fq", ".json"))
        out["trim"]["same_files"] = same and open(o + "h.fq", "rb").read() == open(o + "r.fq", "rb").read()
        out["trim"]["kma_trim_over_kmahip_trim_s1dev"] = round(out["trim"]["kma_trim"]["median"] / out["trim"]["kmahip_trim_s1dev"]["median"], 2)
        print(json.dumps(out, indent=1))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
