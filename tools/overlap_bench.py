#!/usr/bin/env python
"""gce_bam_merge_overlap on the files of a run: the cfg3 stream of tools/bam_bench.py goes through run_bam once; its output file
and its 8.0 M-record input each go through merge_overlap_bam, interleaved with calmd_bam (in-core) of another build of the library on the
same files -- the nearest existing runner that inflates, rewrites and writes a whole file.
    python tools/overlap_bench.py --lib PARENT.so [--workload cfg3] [--pairs 4000000] [--level -2] [--out profiles/merge_overlap.json]
--lib: the parent commit's build, loaded through GCE_LIB (never the code under test as its own yardstick).  Every run is a fresh child process
under its own time limit: one warm-up round and --reps timed rounds, medians.  Then one rocprofv3 --kernel-trace --stats run per file, each in
a process of its own, for k_ovl_check, k_frag_prep, k_frag_join and k_ovl_merge.  Recorded: the stage times, the counters, the kernel times,
and k_ovl_merge's nanoseconds per shared column beside DESIGN.md 4k's k_frag_count figure.  There is no pass mark."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
FRAG_COUNT_4K = dict(seconds=0.0094, shared_columns=27.4e6, source="DESIGN.md 4k, profiles/pileup_fragments.json: k_frag_count, which also counts")
KERNELS = r"k_ovl_check|k_ovl_merge|k_frag_prep|k_frag_join"
COUNTERS = ("n_records", "n_pairs", "n_pairs_no_qual", "n_ambiguous", "n_shared_columns", "n_disagree_columns", "n_columns_skipped", "n_records_changed")


def child_run(args):
    from gencore_amd import bamio
    src, out = os.path.join(args.child, args.file), os.path.join(args.child, "rewritten.bam")
    with open(src, "rb") as f:                                    # the input in the page cache
        while f.read(1 << 26):
            pass
    t0 = time.perf_counter()
    if args.mode == "overlap":
        r = bamio.merge_overlap_bam(src, out, threads=args.threads, level=args.level)
    else:
        r = bamio.calmd_bam(src, out, os.path.join(args.child, "ref.fa"), threads=args.threads, level=args.level)
    wall = time.perf_counter() - t0
    os.remove(out)
    print(json.dumps(dict(r.as_dict(), wall_s=wall)), flush=True)


def run_child(args, tmp, mode, file, prefix=(), lib=None):
    env = dict(os.environ)
    if lib:
        env["GCE_LIB"] = lib
    p = subprocess.run(["timeout", "-k", "10", "600"] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", mode, "--file", file, "--threads", str(args.threads),
                                                                      "--level", str(args.level)], stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("overlap_bench: a child run (%s of %s) failed (exit %d)" % (mode, file, p.returncode))
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--level", type=int, default=-2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", default=None)
    ap.add_argument("--mode", default="overlap", choices=("make", "overlap", "calmd"))
    ap.add_argument("--file", default="out.bam")
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's) for the calmd_bam yardstick")
    args = ap.parse_args()
    if args.child is not None:
        if args.mode == "make":
            import calmd_bench
            return calmd_bench.child_make(args)
        return child_run(args)
    if not (args.lib and os.path.exists(args.lib)):
        raise SystemExit("overlap_bench: --lib, the parent commit's build of the library, is needed for the yardstick")
    args.out = args.out or os.path.join(ROOT, "profiles", "merge_overlap.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_overlap_")
    p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", "make", "--workload", args.workload, "--pairs", str(args.pairs),
                        "--threads", str(args.threads)], stdout=subprocess.PIPE, universal_newlines=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("overlap_bench: making the files failed (exit %d)" % p.returncode)
    made = json.loads(lines[-1])
    files = dict(output="out.bam", input="in.bam")
    variants = {}
    for k, f in files.items():
        variants["merge_overlap_" + k] = dict(mode="overlap", file=f, lib=None)
        variants["parent_calmd_" + k] = dict(mode="calmd", file=f, lib=args.lib)
    per = {k: [] for k in variants}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for k, v in variants.items():
            r = run_child(args, tmp, v["mode"], v["file"], lib=v["lib"])
            if rep:
                per[k].append(r)
        print("overlap_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    res = dict(workload=args.workload, pairs=int(args.pairs), level=args.level, reps=args.reps, **made,
               yardstick="calmd_bam (in-core) of the parent commit's build (GCE_LIB) on the same file, interleaved, every run a fresh process", variants={})
    for k, rs in per.items():
        stages = [s for s in ("read_s", "inflate_index_s", "merge_s", "calmd_s", "write_s", "total_s", "wall_s") if s in rs[0]]
        v = dict(file=variants[k]["file"], file_bytes=os.path.getsize(os.path.join(tmp, variants[k]["file"])), stages={s: round(med(rs, s), 4) for s in stages},
                 total_s_all=[round(r["total_s"], 4) for r in rs], inflated_bytes=int(rs[0]["inflated_bytes"]), peak_device_bytes=int(rs[0]["peak_device_bytes"]))
        if variants[k]["mode"] == "overlap":
            v["counters"] = {c: int(rs[0][c]) for c in COUNTERS}
        res["variants"][k] = v
    for k in files:
        m, c = res["variants"]["merge_overlap_" + k], res["variants"]["parent_calmd_" + k]
        m["total_over_parent_calmd"] = round(m["stages"]["total_s"] / c["stages"]["total_s"], 3)
    for k, f in files.items():                                     # one kernel trace per file, each in a process of its own
        prof = os.path.join(tmp, "prof_" + k)
        run_child(args, tmp, "overlap", f, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "overlap", "--output-format", "csv", "--"])
        kern = {}
        for path in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                m = re.search(KERNELS, r["Name"])
                if m:
                    x = kern.setdefault(m.group(0), dict(calls=0, seconds=0.0))
                    x["calls"] += int(r["Calls"]); x["seconds"] += float(r["TotalDurationNs"]) * 1e-9
        if "k_ovl_merge" not in kern:
            raise SystemExit("overlap_bench: no k_ovl_merge row in rocprofv3's *kernel_stats.csv under %s" % prof)
        v = res["variants"]["merge_overlap_" + k]
        shared = v["counters"]["n_shared_columns"]
        v["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run in a process of its own", kernels={n: dict(calls=x["calls"], seconds=round(x["seconds"], 6)) for n, x in sorted(kern.items())},
                            seconds=round(sum(x["seconds"] for x in kern.values()), 6))
        v["k_ovl_merge_ns_per_shared_column"] = round(kern["k_ovl_merge"]["seconds"] * 1e9 / shared, 4) if shared else None
    res["k_frag_count_4k"] = dict(FRAG_COUNT_4K, ns_per_shared_column=round(FRAG_COUNT_4K["seconds"] * 1e9 / FRAG_COUNT_4K["shared_columns"], 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
