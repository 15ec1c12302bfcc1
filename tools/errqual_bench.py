#!/usr/bin/env python
"""gce_bam_error_profile_quality, its adds meeting in the block's table on chip (the tree's kernel, --name), beside the same pass with direct
atomics (GCE_ERRQUAL_DIRECT), beside other builds of the on-chip kernel (--alt NAME=PATH, loaded through GCE_LIB: an aggregation in front of
the table that is being tried) and beside gce_bam_error_profile on the same file, the yardstick.  Two files: `in`, the cfg3
stream of tools/errprof_bench.py, whose qualities are three numbers (37, 25 and 11 at 80 / 12 / 8 %): the contended case; and `out`, that
stream through the consensus engine at -s 1.
    python tools/errqual_bench.py [--workload cfg3] [--pairs 4000000] [--reps 3] [--name plain] [--alt runs=ab/libgencore_amd_runs.so] [--order plain,runs]
                                  [--out profiles/errqual.json]
The variants are interleaved; every run is a fresh child process under its own time limit and the first failure ends the script; one warm-up
round, then --reps timed rounds, reported as medians with all values.  errprof_s is the scan + the count kernel, host clocks around work that
ends in a device synchronise.  A variant is faster only when the medians differ by more than the spread of the values; the default is the
variant with the lowest errprof_s on `in`, ties going to the simpler kernel (direct, then the on-chip variants in --order).  The counters of
all variants must be identical and, summed over the buckets, equal the yardstick's summed over the cycles.  One rocprofv3 --kernel-trace
--stats run per variant and file, each in a process of its own and without counters, gives the kernel times.  The ratio to
gce_bam_error_profile is reported, not gated.  profiles/errqual.json: --name plain, with the lane-private runs and the wave-aggregated adds
as --alt builds; neither won and neither is in the tree."""
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
FILES = ("in", "out")
NOT_MEASURED = ["real binned qualities", "a BED", "a mask", "min_baseq > 0", "long reads", "windows of 4 GB and more"]


def child(args):
    import zlib
    from gencore_amd import bamio
    variant, which = args.mode.rsplit("_", 1)
    src, fa = os.path.join(args.child, which + ".bam"), os.path.join(args.child, "ref.fa")
    for p in (src, fa):                                           # the inputs in the page cache
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    t0 = time.perf_counter()
    if variant == "cycle":
        r = bamio.error_profile_bam(src, fa, threads=args.threads)
    else:
        r = bamio.error_profile_quality_bam(src, fa, tsv=os.path.join(args.child, "%s.tsv" % args.mode), threads=args.threads, direct=variant == "direct")
    by_class = r.counts.sum(axis=1)[:, :21]
    d = dict(r.as_dict(), counts_sum=int(r.counts.sum()), counts_crc=int(zlib.crc32(r.counts.tobytes())), by_class_crc=int(zlib.crc32(by_class.tobytes())))
    if variant != "cycle":
        d["rows"] = int((r.counts.sum(axis=(0, 2)) != 0).sum())
    print(json.dumps(dict(d, wall_s=time.perf_counter() - t0)), flush=True)


def run_child(args, tmp, mode, prefix=(), limit=None):
    variant = mode.rsplit("_", 1)[0]
    limit = limit or (args.direct_limit if variant == "direct" else args.limit)
    env = dict(os.environ, GCE_LIB=os.path.abspath(args.alts[variant])) if variant in args.alts else None
    script = os.path.join(ROOT, "tools", "errsup_bench.py") if mode == "make" else os.path.abspath(__file__)     # (make: errsup_bench's in.bam, out.bam and ref.fa)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, script, "--child", tmp, "--mode", "onchip_" + mode.rsplit("_", 1)[1] if variant in args.alts else mode,
                                                                           "--threads", str(args.threads), "--workload", args.workload, "--pairs", str(args.pairs)],
                       stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("errqual_bench: a child run (%s) failed (exit %d, limit %d s)" % (mode, p.returncode, limit))
    return json.loads(lines[-1])


def kernel_times(args, tmp, mode):
    prof = os.path.join(tmp, "prof_" + mode)
    run_child(args, tmp, mode, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "errqual", "--output-format", "csv", "--"])
    kern = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_qual_\w+|k_err_\w+|k_reduce_scan", r["Name"])   # (the CSV holds the demangled name)
            if m:
                k = kern.setdefault(m.group(0), dict(calls=0, seconds=0.0))
                k["calls"] += int(r["Calls"]); k["seconds"] += float(r["TotalDurationNs"]) * 1e-9
    if not kern:
        raise SystemExit("errqual_bench: no kernel row in rocprofv3's *kernel_stats.csv under %s" % prof)
    return {n: dict(calls=k["calls"], seconds=round(k["seconds"], 6)) for n, k in sorted(kern.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--direct_limit", type=int, default=900)
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH", help="another build of libgencore_amd.so whose on-chip kernel runs in the same rounds as variant NAME")
    ap.add_argument("--alt_note", action="append", default=[], metavar="NAME=TEXT", help="what the build NAME is, in a sentence; kept in the result")
    ap.add_argument("--name", default="onchip", help="what the tree's on-chip kernel is called in the result")
    ap.add_argument("--order", default=None, help="the on-chip variants from the simplest to the most involved, comma separated; default: the --alt builds, then --name")
    ap.add_argument("--child", default=None)
    ap.add_argument("--mode", default="make")
    args = ap.parse_args()
    args.alts = dict(a.split("=", 1) for a in args.alt)
    if args.child is not None:
        return child(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "errqual.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_errqual_")
    made = run_child(args, tmp, "make", limit=1100)
    onchip = (args.order.split(",") if args.order else list(args.alts) + [args.name])
    assert sorted(onchip) == sorted(list(args.alts) + [args.name]) and not {"direct", "cycle"} & set(onchip)
    variants = tuple(onchip) + ("direct", "cycle")
    modes = ["%s_%s" % (v, f) for f in FILES for v in variants]
    per = {m: [] for m in modes}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for m in modes:
            r = run_child(args, tmp, m)
            if rep:
                per[m].append(r)
        print("errqual_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    spread = lambda rs, k: max(r[k] for r in rs) - min(r[k] for r in rs)
    res = dict(workload=args.workload, pairs=int(args.pairs), reps=args.reps, **made, bytes={f: os.path.getsize(os.path.join(tmp, f + ".bam")) for f in FILES},
               clocks="the library's stage times: host clocks around work that ends in a device synchronise",
               tree_kernel=args.name,
               what="gce_bam_error_profile_quality (--name: the tree's on-chip kernel; direct: GCE_ERRQUAL_DIRECT; the other names: --alt builds of the on-chip kernel) beside "
                    "gce_bam_error_profile (cycle) on the same files, without a BED or a mask, interleaved; in: the cfg3 stream, three quality values; out: the stream through the "
                    "consensus engine at -s 1",
               alt_builds={n: t for n, t in (a.split("=", 1) for a in args.alt_note)}, not_measured=NOT_MEASURED, files={})
    for f in FILES:
        v = {}
        for var in variants:
            rs = per["%s_%s" % (var, f)]
            v[var] = dict(stages={k: round(med(rs, k), 5) for k in ("read_s", "inflate_index_s", "errprof_s", "write_s", "total_s", "wall_s")},
                          errprof_s_all=[round(r["errprof_s"], 5) for r in rs], total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                          counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_")}, sums={c: rs[0][c] for c in ("counts_sum", "counts_crc", "by_class_crc", "rows") if c in rs[0]})
        e = lambda var: v[var]["stages"]["errprof_s"]
        sp = lambda a, b: max(spread(per["%s_%s" % (a, f)], "errprof_s"), spread(per["%s_%s" % (b, f)], "errprof_s"))
        quality = [x for x in variants if x != "cycle"]
        # the winner: from the simplest on, a later variant takes over only when it is faster by more than the spread
        best = "direct"
        steps = []
        for var in onchip:
            gap, noise = e(best) - e(var), sp(best, var)
            steps.append(dict(holder=best, challenger=var, holder_minus_challenger_s=round(gap, 5), spread_s=round(noise, 5), challenger_wins=gap > noise))
            if gap > noise:
                best = var
        dec = dict(rule="from the simplest kernel on (direct, then the on-chip variants in their order) a variant takes over only when its median errprof_s is lower by more than the "
                        "spread of the values",
                   counters_identical=all(v[x]["sums"] == v[quality[0]]["sums"] and v[x]["counters"] == v[quality[0]]["counters"] for x in quality),
                   classes_equal_the_cycle_tables=all(v[x]["sums"]["by_class_crc"] == v["cycle"]["sums"]["by_class_crc"] for x in quality),
                   totals_equal_the_cycle_tables=all(v[x]["counters"] == v["cycle"]["counters"] for x in quality), steps=steps, winner=best,
                   ratio_to_the_cycle_profile={x: round(e(x) / e("cycle"), 3) for x in quality})
        res["files"][f] = dict(variants=v, decision=dec)
    res["default"] = res["files"]["in"]["decision"]["winner"]
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")
    write()                                                       # (the timed rounds stand if a trace below fails: a failure ends the script)
    for f in FILES:
        for var in variants:
            res["files"][f]["variants"][var]["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run of this variant in a process of its own",
                                                               **kernel_times(args, tmp, "%s_%s" % (var, f)))
            write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
