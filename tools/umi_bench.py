#!/usr/bin/env python
"""gce_bam_umi_to_mi beside calmd_bam_stream of the same build on the same file: the file tools/calmd_bench.py uses -- the
output of a run on the cfg3 stream, made by that tool's own `make` step -- goes through umi_to_mi with source RX and with source name, and
through calmd_bam_stream, the variants interleaved.
    python tools/umi_bench.py [--workload cfg3] [--pairs 4000000] [--level -2] [--reps 5] [--out profiles/umi_mi.json]
calmd reads the same bytes and does strictly more per record (the CIGAR walk over read and reference), so it is the yardstick to report
against; it is not a gate and there is no pass mark.  What this file can show: its records carry no RX (source RX: every record without a
source, the walk of the optional fields and the whole-record copy) and fastp-style names (...:UMI_ACGT: source name finds a last field that
is not a UMI, the same copy).  The tagged path -- k_umi_tag and a body copy in stretches -- is NOT measured here: no record of this file
takes it.  Stage times are the library's own host clocks around work that ends in a device synchronise (umi_s / calmd_s: the kernels and
their scan); no kernel was traced.  Every run is a fresh child process under its own time limit."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("read_s", "inflate_index_s", "kernels_s", "write_s", "total_s", "wall_s")


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("umi_bench: no GPU; nothing is measured without one")
    from gencore_amd import bamio
    src, out = os.path.join(args.child, "out.bam"), os.path.join(args.child, "umi_bench_out.bam")
    with open(src, "rb") as f:                                    # the input in the page cache
        while f.read(1 << 26):
            pass
    t0 = time.perf_counter()
    if args.mode == "calmd":
        r = bamio.calmd_bam_stream(src, out, os.path.join(args.child, "ref.fa"), threads=args.threads, level=args.level)
    else:
        r = bamio.umi_to_mi(src, out, source=args.mode, threads=args.threads, level=args.level)
    wall = time.perf_counter() - t0
    d = r.as_dict()
    d["kernels_s"] = d.pop("calmd_s" if args.mode == "calmd" else "umi_s")
    print(json.dumps(dict(d, wall_s=wall)), flush=True)


def run_child(args, tmp, mode):
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", mode, "--threads", str(args.threads), "--level", str(args.level)],
                       stdout=subprocess.PIPE, universal_newlines=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("umi_bench: a child run (%s) failed (exit %d)" % (mode, p.returncode))
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--level", type=int, default=-2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--mode", default="RX", help="(child) calmd, or the source of umi_to_mi")
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "umi_mi.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_umi_")
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "tools", "calmd_bench.py"), "--child", tmp, "--mode", "make", "--workload", args.workload,
                        "--pairs", str(args.pairs), "--threads", str(args.threads)], stdout=subprocess.PIPE, universal_newlines=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("umi_bench: making the file failed (exit %d)" % p.returncode)
    made = json.loads(lines[-1])
    variants = dict(umi_rx="RX", umi_name="name", calmd_stream="calmd")
    per = {k: [] for k in variants}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for k, mode in variants.items():
            r = run_child(args, tmp, mode)
            if rep:
                per[k].append(r)
        print("umi_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    res = dict(workload=args.workload, pairs=int(args.pairs), level=args.level, reps=args.reps, **made,
               file="the output of run_bam on the stream, as tools/calmd_bench.py makes it", input_bytes=os.path.getsize(os.path.join(tmp, "out.bam")),
               yardstick="calmd_bam_stream of the same build on the same file, interleaved; not a gate",
               measured="source RX (no record has the tag) and source name (no name ends in a UMI): the walk of the optional fields and the whole-record copy",
               not_measured="the tagged path (k_umi_tag, the body copy in stretches): no record of this file takes it; kernel times by rocprofv3",
               clocks="the library's stage times: host clocks around work that ends in a device synchronise",
               variants={k: dict(stages={x: round(med(rs, x), 4) for x in STAGES}, total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                                 inflated_bytes=int(rs[0]["inflated_bytes"]), out_record_bytes=int(rs[0]["out_record_bytes"]), n_flushes=int(rs[0]["n_flushes"]),
                                 counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_") and c != "n_flushes"}) for k, rs in per.items()})
    for k in ("umi_rx", "umi_name"):
        res["variants"][k]["total_over_calmd"] = round(res["variants"][k]["stages"]["total_s"] / res["variants"]["calmd_stream"]["stages"]["total_s"], 3)
        res["variants"][k]["kernels_over_calmd"] = round(res["variants"][k]["stages"]["kernels_s"] / max(res["variants"]["calmd_stream"]["stages"]["kernels_s"], 1e-9), 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
