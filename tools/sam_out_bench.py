#!/usr/bin/env python
"""SAM text output of the file path, host formatter against the GPU's: the cfg3 file of tools/bam_bench.py through run_bam to
a `.sam` name at level 1 (samtext::bam_to_line on the host's threads) and at level -2 (gce_raw_format_output: the lines made in HBM, the
host only copies and writes them).
    python tools/sam_out_bench.py [--workload cfg3] [--pairs 4000000] [--lib PARENT/libgencore_amd.so] [--out profiles/sam_out.json]
--lib points the level-1 variant at another build of the library (the parent commit's), so the yardstick is never the code under test.  The
two variants are interleaved, one warm-up and --reps timed runs each, medians; every run is a fresh child process under its own time limit.
The two outputs are compared for equality.  One rocprofv3 --kernel-trace --stats run of the GPU variant, in a process of its own, gives the
time of every k_samfmt_* kernel and the formatter's rate in text bytes per second."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    from gencore_amd import capi
    from gencore_amd.bamio import run_bam
    src, out = os.path.join(args.child, "in.bam"), os.path.join(args.child, "out_lv%d.sam" % args.child_level)
    prm = capi.default_params(umi_prefix="auto", cluster_size_req=int(args.sreq))
    with open(src, "rb") as f:                                    # the input in the page cache
        while f.read(1 << 26):
            pass
    t0 = time.perf_counter()
    r = run_bam(src, out, prm, fasta=None, threads=args.threads, level=args.child_level)
    res = dict(wall_s=time.perf_counter() - t0, write_s=r.write_s, total_s=r.total_s, process_s=r.process_s, drain_s=r.drain_s, n_out=int(r.n_out), out_bytes=os.path.getsize(out))
    lib = capi.load_library()
    if hasattr(lib, "gce_get_sam_format_counters"):
        from gencore_amd.bamio import sam_format_counters
        res["counters"] = sam_format_counters()
    print(json.dumps(res), flush=True)


def run_child(args, tmp, level, prefix=(), lib=None):
    env = dict(os.environ)
    if lib:
        env["GCE_LIB"] = lib
    p = subprocess.run(["timeout", "-k", "10", "600"] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--threads", str(args.threads), "--child-level", str(level),
                                                                      "--sreq", str(args.sreq)], stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("sam_out_bench: a child run failed (exit %d)" % p.returncode)
    return json.loads(lines[-1])


def make_input(args, src):
    import numpy as np
    import torch
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    d = synth.generate(args.workload, n_pairs=args.pairs, device=torch.device("cuda:0" if torch.cuda.is_available() else "cpu"))
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    write_batch_as_bam(src, batch, tl, ["chr%d" % (i + 1) for i in range(len(tl))], threads=args.threads, level=1)
    print("sam_out_bench: %d records written" % batch.n, flush=True)
    return int(d.info["supporting_reads"]), int(batch.n)


def same_file(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="the library of the level-1 (host formatter) variant: the parent commit's build")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-level", type=int, default=1)
    ap.add_argument("--sreq", default="1")
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "sam_out.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_samout_")
    args.sreq, n_reads = make_input(args, os.path.join(tmp, "in.bam"))
    variants = (("host_level_1", 1, args.lib), ("gpu_level_-2", -2, None))
    for _, lv, lib in variants:                                   # warm-up: page cache, code objects
        run_child(args, tmp, lv, lib=lib)
    runs = {v[0]: [] for v in variants}
    for _ in range(args.reps):                                    # interleaved: a drift of the machine falls on both
        for v, lv, lib in variants:
            runs[v].append(run_child(args, tmp, lv, lib=lib))
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    a, b = runs["host_level_1"], runs["gpu_level_-2"]
    identical = same_file(os.path.join(tmp, "out_lv1.sam"), os.path.join(tmp, "out_lv-2.sam"))
    prof = os.path.join(tmp, "prof_samfmt")
    rp = run_child(args, tmp, -2, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "samfmt", "--output-format", "csv", "--"])
    kern = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_samfmt_\w+", r["Name"])              # (the CSV holds the demangled name: "(anonymous namespace)::k_samfmt_size(...)")
            if m:
                k = kern.setdefault(m.group(0), dict(calls=0, seconds=0.0))
                k["calls"] += int(r["Calls"]); k["seconds"] += float(r["TotalDurationNs"]) * 1e-9
    if not kern:
        raise SystemExit("sam_out_bench: no k_samfmt_ row in rocprofv3's *kernel_stats.csv under %s" % prof)
    fmt_s = sum(k["seconds"] for k in kern.values())
    text_bytes = rp["counters"][3]
    stages = ("write_s", "total_s", "wall_s")
    res = dict(workload=args.workload, pairs=int(args.pairs), reads=n_reads, records_out=b[0]["n_out"], out_sam_bytes=b[0]["out_bytes"], outputs_identical=bool(identical), reps=args.reps,
               host_level_1=dict(library=args.lib or "this tree's", **{k: round(med(a, k), 4) for k in stages}, write_s_all=[round(r["write_s"], 4) for r in a], out_bytes=a[0]["out_bytes"]),
               gpu_level_minus_2=dict(**{k: round(med(b, k), 4) for k in stages}, write_s_all=[round(r["write_s"], 4) for r in b], out_bytes=b[0]["out_bytes"], counters=b[0]["counters"]),
               format_kernels=dict(source="rocprofv3 --kernel-trace --stats, a run of the level -2 variant in a process of its own",
                                   kernels={n: dict(calls=k["calls"], seconds=round(k["seconds"], 6)) for n, k in sorted(kern.items())}, seconds=round(fmt_s, 6), text_bytes=text_bytes,
                                   text_gb_per_s=round(text_bytes / fmt_s / 1e9, 2), n_host_records=rp["counters"][1]))
    res["host_write_over_gpu_write"] = round(res["host_level_1"]["write_s"] / res["gpu_level_minus_2"]["write_s"], 3)
    res["host_total_over_gpu_total"] = round(res["host_level_1"]["total_s"] / res["gpu_level_minus_2"]["total_s"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
