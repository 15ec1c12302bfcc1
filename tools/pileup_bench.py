#!/usr/bin/env python
"""gce_bam_pileup with its LDS tile beside the same pass with direct atomics (GCE_PILEUP_DIRECT) and beside gce_bam_index, the streaming
pass over the same file this pass was built on: the cfg3 stream of tools/bam_bench.py as a BAM file, with its panel as the BED.
    python tools/pileup_bench.py [--workload cfg3] [--pairs 4000000] [--reps 3] [--out profiles/pileup.json]
The variants are interleaved; every run is a fresh child process under its own time limit; one warm-up round, then --reps timed rounds,
reported as medians with all values.  The question is which variant has the lower median pileup_s (the scan + k_pile_count, host clocks
around work that ends in a device synchronise): if the two differ by less than the spread of their values the default is direct, the simpler
path.  gce_bam_index's gpu_s (inflate, record index, facts and the index's kernels) stands beside pileup_s + inflate_index_s so that the cost
of the count kernels above read, inflate and index is visible.  One rocprofv3 --kernel-trace --stats run per variant, each in a process of its
own, gives the kernel times.  There is no pass mark.
    python tools/pileup_bench.py --fragments [--out profiles/pileup_fragments.json]
runs gce_bam_pileup_fragments (frag_tile, frag_direct) beside gce_bam_pileup (tile, direct) on the same file in the same
interleaved rounds: both passes' pileup_s with all values and the median, the new pass's share of its total_s, tile against direct, and one
kernel trace per variant.  No time is fixed for the join or the paired walk; the pass is opt-in and no default rides on the outcome.
    python tools/pileup_bench.py --fragments --parent_lib PATH [--out ...]
runs the library built from the parent commit (loaded through GCE_LIB) in the same rounds as tools/errprof_bench.py does: parent_tile,
parent_direct, parent_frag_tile and parent_frag_direct.  Per pair it reports this_minus_parent_s, the spread, `unchanged` (the medians of
pileup_s differ by less than the spread of the values) and counters_identical (the CRC of the counts and the n_* counters but n_deferred)."""
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
FRAG_MODES = ("tile", "frag_tile", "direct", "frag_direct")
PARENT_MODES = tuple("parent_" + m for m in FRAG_MODES)


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pileup_bench: no GPU; nothing is measured without one")
    from gencore_amd import bamio
    src, bed = os.path.join(args.child, "in.bam"), os.path.join(args.child, "panel.bed")
    with open(src, "rb") as f:                                    # the input in the page cache
        while f.read(1 << 26):
            pass
    mode = args.mode[len("parent_"):] if args.mode.startswith("parent_") else args.mode   # (the parent's library is GCE_LIB's doing, run_child)
    t0 = time.perf_counter()
    if mode == "index":
        d = bamio.index_bam(src, os.path.join(args.child, "in.bam.bai"), threads=args.threads)
        d = {k: v for k, v in (d if isinstance(d, dict) else vars(d)).items() if isinstance(v, (int, float))}
    else:
        run = bamio.pileup_fragments_bam if mode.startswith("frag_") else bamio.pileup_bam
        r = run(src, bed, tsv=os.path.join(args.child, "%s.tsv" % args.mode), threads=args.threads, direct=mode.endswith("direct"))
        d = dict(r.as_dict(), counts_sum=int(r.counts.sum()), counts_crc=int(__import__("zlib").crc32(r.counts.tobytes())))
    print(json.dumps(dict(d, wall_s=time.perf_counter() - t0)), flush=True)


def child_make(args):
    """in.bam (the stream) and panel.bed (its panel) under args.child"""
    import numpy as np
    import torch
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    d = synth.generate(args.workload, n_pairs=args.pairs, device=torch.device("cuda:0" if torch.cuda.is_available() else "cpu"))
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(os.path.join(args.child, "in.bam"), batch, tl, names, threads=args.threads, level=1)
    bed = np.asarray(d.info["bed"])[:, :3]
    with open(os.path.join(args.child, "panel.bed"), "w") as f:
        for t, a, z in bed:
            f.write("%s\t%d\t%d\n" % (names[int(t)], int(a), int(z)))
    print(json.dumps(dict(reads=int(batch.n), bed_regions=int(len(bed)))), flush=True)


def run_child(args, tmp, mode, prefix=(), limit=300):
    env = dict(os.environ, GCE_LIB=os.path.abspath(args.parent_lib)) if mode.startswith("parent_") else None
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", mode, "--threads", str(args.threads),
                                                                           "--workload", args.workload, "--pairs", str(args.pairs)], stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("pileup_bench: a child run (%s) failed (exit %d)" % (mode, p.returncode))
    return json.loads(lines[-1])


def kernel_times(args, tmp, mode):
    prof = os.path.join(tmp, "prof_" + mode)
    run_child(args, tmp, mode, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "pileup", "--output-format", "csv", "--"])
    kern = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_pile_\w+|k_frag_\w+|k_reduce_scan", r["Name"])  # (the CSV holds the demangled name)
            if m:
                k = kern.setdefault(m.group(0), dict(calls=0, seconds=0.0))
                k["calls"] += int(r["Calls"]); k["seconds"] += float(r["TotalDurationNs"]) * 1e-9
    if not kern:
        raise SystemExit("pileup_bench: no k_pile_ or k_frag_ row in rocprofv3's *kernel_stats.csv under %s" % prof)
    return {n: dict(calls=k["calls"], seconds=round(k["seconds"], 6)) for n, k in sorted(kern.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", default=None)
    ap.add_argument("--mode", default="tile", choices=("make", "index") + FRAG_MODES + PARENT_MODES)
    ap.add_argument("--fragments", action="store_true", help="gce_bam_pileup_fragments beside gce_bam_pileup; writes profiles/pileup_fragments.json")
    ap.add_argument("--parent_lib", default=None, help="with --fragments: the parent commit's libgencore_amd.so, run in the same rounds through GCE_LIB")
    args = ap.parse_args()
    if args.child is not None:
        return child_make(args) if args.mode == "make" else child(args)
    if args.fragments:
        return main_fragments(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "pileup.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_pileup_")
    made = run_child(args, tmp, "make", limit=600)
    modes = ("tile", "direct", "index")
    per = {m: [] for m in modes}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for m in modes:
            r = run_child(args, tmp, m)
            if rep:
                per[m].append(r)
        print("pileup_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    spread = lambda rs, k: max(r[k] for r in rs) - min(r[k] for r in rs)
    res = dict(workload=args.workload, pairs=int(args.pairs), reps=args.reps, **made, input_bytes=os.path.getsize(os.path.join(tmp, "in.bam")),
               clocks="the library's stage times: host clocks around work that ends in a device synchronise", variants={})
    for m in ("tile", "direct"):
        rs = per[m]
        res["variants"][m] = dict(stages={k: round(med(rs, k), 5) for k in ("read_s", "inflate_index_s", "pileup_s", "write_s", "total_s", "wall_s")},
                                  pileup_s_all=[round(r["pileup_s"], 5) for r in rs], total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                                  counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_")}, counts_sum=rs[0]["counts_sum"], counts_crc=rs[0]["counts_crc"])
    rs = per["index"]
    res["index"] = dict(what="gce_bam_index on the same file, interleaved: the streaming pass this one is built on; not a gate",
                        stages={k: round(med(rs, k), 5) for k in ("read_s", "gpu_s", "write_s", "total_s", "wall_s")}, gpu_s_all=[round(r["gpu_s"], 5) for r in rs],
                        total_s_all=[round(r["total_s"], 4) for r in rs])
    t, d = res["variants"]["tile"], res["variants"]["direct"]
    res["counters_identical"] = t["counts_crc"] == d["counts_crc"] and t["counters"] == d["counters"]
    gap = abs(t["stages"]["pileup_s"] - d["stages"]["pileup_s"])
    noise = max(spread(per["tile"], "pileup_s"), spread(per["direct"], "pileup_s"))
    res["decision"] = dict(rule="the lower median pileup_s; direct, the simpler path, when the medians differ by less than the spread of the three values",
                           median_gap_s=round(gap, 5), spread_s=round(noise, 5),
                           default="direct" if gap < noise or d["stages"]["pileup_s"] <= t["stages"]["pileup_s"] else "tile")
    for m in ("tile", "direct"):
        v = res["variants"][m]
        v["gpu_s_beside_index"] = dict(pileup_s=v["stages"]["pileup_s"], inflate_index_s=v["stages"]["inflate_index_s"], index_gpu_s=res["index"]["stages"]["gpu_s"])
        v["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run of this variant in a process of its own", **kernel_times(args, tmp, m))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main_fragments(args):
    args.out = args.out or os.path.join(ROOT, "profiles", "pileup_fragments.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_fragpile_")
    made = run_child(args, tmp, "make", limit=600)
    modes = FRAG_MODES + (PARENT_MODES if args.parent_lib else ())
    per = {m: [] for m in modes}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for m in modes:
            r = run_child(args, tmp, m)
            if rep:
                per[m].append(r)
        print("pileup_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    res = dict(workload=args.workload, pairs=int(args.pairs), reps=args.reps, **made, input_bytes=os.path.getsize(os.path.join(tmp, "in.bam")),
               clocks="the library's stage times: host clocks around work that ends in a device synchronise",
               what="gce_bam_pileup_fragments (frag_*) beside gce_bam_pileup on the same file, interleaved; no pass mark", variants={})
    for m in modes:
        rs = per[m]
        res["variants"][m] = dict(stages={k: round(med(rs, k), 5) for k in ("read_s", "inflate_index_s", "pileup_s", "write_s", "total_s", "wall_s")},
                                  pileup_s_all=[round(r["pileup_s"], 5) for r in rs], total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                                  pileup_share_of_total=round(med(rs, "pileup_s") / med(rs, "total_s"), 4),
                                  counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_")}, counts_sum=rs[0]["counts_sum"], counts_crc=rs[0]["counts_crc"])
    v = res["variants"]
    res["counters_identical"] = dict(pileup=v["tile"]["counts_crc"] == v["direct"]["counts_crc"], fragments=v["frag_tile"]["counts_crc"] == v["frag_direct"]["counts_crc"] and
                                     {k: c for k, c in v["frag_tile"]["counters"].items() if k != "n_deferred"} == {k: c for k, c in v["frag_direct"]["counters"].items() if k != "n_deferred"})
    res["pileup_s_ratio"] = dict(frag_tile_over_tile=round(v["frag_tile"]["stages"]["pileup_s"] / v["tile"]["stages"]["pileup_s"], 3),
                                 frag_direct_over_direct=round(v["frag_direct"]["stages"]["pileup_s"] / v["direct"]["stages"]["pileup_s"], 3),
                                 frag_tile_over_frag_direct=round(v["frag_tile"]["stages"]["pileup_s"] / v["frag_direct"]["stages"]["pileup_s"], 3))
    if args.parent_lib:
        spread = lambda rs: max(r["pileup_s"] for r in rs) - min(r["pileup_s"] for r in rs)
        same = lambda a, b: v[a]["counts_crc"] == v[b]["counts_crc"] and {k: c for k, c in v[a]["counters"].items() if k != "n_deferred"} == {k: c for k, c in v[b]["counters"].items() if k != "n_deferred"}
        res["against_the_parent"] = {}
        for m in FRAG_MODES:
            gap, noise = v[m]["stages"]["pileup_s"] - v["parent_" + m]["stages"]["pileup_s"], max(spread(per[m]), spread(per["parent_" + m]))
            res["against_the_parent"][m] = dict(rule="pileup_s is unchanged when the medians differ by less than the spread of the values", this_minus_parent_s=round(gap, 5),
                                                spread_s=round(noise, 5), unchanged=abs(gap) <= noise, counters_identical=same(m, "parent_" + m))
    for m in FRAG_MODES:
        v[m]["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run of this variant in a process of its own", **kernel_times(args, tmp, m))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
