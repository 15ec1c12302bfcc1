#!/usr/bin/env python
"""Device-memory footprint and timing of the pass runner (gce_run_bam_passes) on a synthetic sorted BAM:
    python tools/pass_profile.py --workload cfg3 --pairs 4000000 --passes 1,2,4
Prints one JSON line: the single-pass run's peak device bytes against its reads and inflated bytes, then per pass count P the total, key-pass
and per-pass seconds, the peak device bytes and the records held across pass boundaries (budget chosen so that the estimator gives P)."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from gencore_amd import capi  # noqa: E402
from gencore_amd.bamio import run_bam_passes, write_batch_as_bam  # noqa: E402


def inflated_bytes(path):
    """sum of the BGZF members' ISIZE fields"""
    total = 0
    with open(path, "rb") as f:
        data = f.read()
    o = 0
    while o + 18 <= len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bsize = None
        x = 0
        while x + 4 <= xlen:
            si1, si2, sl = data[o + 12 + x], data[o + 13 + x], struct.unpack_from("<H", data, o + 14 + x)[0]
            if si1 == 66 and si2 == 67 and sl == 2:
                bsize = struct.unpack_from("<H", data, o + 16 + x)[0] + 1
            x += 4 + sl
        total += struct.unpack_from("<I", data, o + bsize - 4)[0]
        o += bsize
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--passes", default="")
    ap.add_argument("--threads", type=int, default=0)
    args = ap.parse_args()
    import torch
    from gencore_amd import synth
    d = synth.generate(args.workload, n_pairs=args.pairs, device=torch.device("cuda:0" if torch.cuda.is_available() else "cpu"))
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    tmp = tempfile.mkdtemp(prefix="gce_pass_")
    src, out = os.path.join(tmp, "in.bam"), os.path.join(tmp, "out.bam")
    write_batch_as_bam(src, batch, tl, ["chr%d" % (i + 1) for i in range(len(tl))], threads=args.threads, level=1)
    prm = capi.default_params(umi_prefix="auto", cluster_size_req=d.info["supporting_reads"])
    res = dict(workload=args.workload, pairs=args.pairs, bam_bytes=os.path.getsize(src), inflated_bytes=inflated_bytes(src))
    r, _, pr = run_bam_passes(src, out, prm, 0, threads=args.threads, level=1)           # auto: the single-pass path when it fits
    res["single_pass"] = dict(path_single=pr["single_pass"], reads=int(r.n_reads), total_s=round(r.total_s, 3), peak_device_bytes=pr["peak_device_bytes"],
                              peak_bytes_per_read=round(pr["peak_device_bytes"] / max(r.n_reads, 1), 1),
                              peak_bytes_per_inflated_byte=round(pr["peak_device_bytes"] / max(res["inflated_bytes"], 1), 3))
    if args.passes:
        t0 = time.time()
        _, _, big = run_bam_passes(src, out, prm, 0, threads=args.threads, level=1, device_budget_bytes=1 << 40)
        res["plan"] = dict(total_weight=big["total_weight"], fixed_bytes=big["fixed_bytes"], reserve=big["budget_bytes"] - big["fixed_bytes"] - big["pass_room"])
        res["passes"] = []
        for P in [int(x) for x in args.passes.split(",")]:
            budget = (1 << 40) if P == 1 else big["budget_bytes"] - big["pass_room"] + -(-big["total_weight"] // P) + 1
            t0 = time.time()
            r2, _, p2 = run_bam_passes(src, out, prm, 0, threads=args.threads, level=1, device_budget_bytes=budget)
            res["passes"].append(dict(P=p2["n_passes"], budget=budget, wall_s=round(time.time() - t0, 3), total_s=round(r2.total_s, 3), key_pass_s=round(p2["key_pass_s"], 3),
                                      pass_s=[round(x, 3) for x in p2["pass_s"]], peak_device_bytes=p2["peak_device_bytes"], held_max=p2["held_max"],
                                      reads_per_pass=p2["reads_per_pass"], n_out=int(r2.n_out)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
