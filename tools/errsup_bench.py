#!/usr/bin/env python
"""gce_bam_error_profile_support, collecting a record's adds on chip (the default), beside the same pass with direct atomics
(GCE_ERRSUP_DIRECT) and beside gce_bam_error_profile on the same file, the yardstick.  Two files: `out`, the cfg3 stream of
tools/errprof_bench.py through the consensus engine at -s 1 (every record carries FR, duplex records RR), and `in`, that stream itself, the
heavy case: no record carries a tag, so every record lands in row (segment, absent, absent), the worst case for adds to one address.
    python tools/errsup_bench.py [--workload cfg3] [--pairs 4000000] [--reps 3] [--direct_limit 900] [--alt_lib PATH] [--out profiles/errsup.json]
The variants are interleaved; every run is a fresh child process under its own time limit and the first failure ends the script; one warm-up
round, then --reps timed rounds, reported as medians with all values.  errprof_s is the scan + the count kernel, host clocks around work that
ends in a device synchronise.  The on-chip variant stays the default only if its median errprof_s beats direct's by more than the spread of
the values on BOTH files.  With --alt_lib, another build of the library (loaded through GCE_LIB) runs its default variant in the same rounds
as alt_onchip: the A/B of a kernel change.  One rocprofv3 --kernel-trace --stats run per variant and file, each in a process of its own,
gives the kernel times.  There is no pass mark."""
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
VARIANTS = ("onchip", "direct", "cycle")
FILES = ("out", "in")


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
        by_class = r.counts.sum(axis=1)[:, :21]
    else:
        r = bamio.error_profile_support_bam(src, fa, tsv=os.path.join(args.child, "%s.tsv" % args.mode), threads=args.threads, direct=variant == "direct")
        by_class = r.counts.sum(axis=(1, 2))[:, :21]
    d = dict(r.as_dict(), counts_sum=int(r.counts.sum()), counts_crc=int(zlib.crc32(r.counts.tobytes())), by_class_crc=int(zlib.crc32(by_class.tobytes())))
    if variant != "cycle":
        d["rows"] = int((r.counts[..., 22] != 0).sum())
    print(json.dumps(dict(d, wall_s=time.perf_counter() - t0)), flush=True)


def child_make(args):
    """errprof_bench's in.bam and ref.fa under args.child, then out.bam: in.bam through the consensus engine at cluster_size_req 1"""
    import errprof_bench
    from gencore_amd.bamio import run_bam
    from gencore_amd.capi import default_params
    args.mask = True                                              # (errprof_bench.child_make prints its line itself without it)
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        errprof_bench.child_make(args)
    finally:
        sys.stdout = stdout
    t0 = time.perf_counter()
    run = run_bam(os.path.join(args.child, "in.bam"), os.path.join(args.child, "out.bam"), default_params(umi_prefix="auto", cluster_size_req=1), fasta=os.path.join(args.child, "ref.fa"),
                  threads=args.threads, level=1)
    print(json.dumps(dict(reads=int(run.n_reads), out_records=int(run.n_out), consensus_s=round(time.perf_counter() - t0, 2))), flush=True)


def run_child(args, tmp, mode, prefix=(), limit=None):
    limit = limit or (args.direct_limit if mode.startswith("direct") else args.limit)
    env = dict(os.environ, GCE_LIB=os.path.abspath(args.alt_lib)) if mode.startswith("alt_") else None
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", mode[4:] if mode.startswith("alt_") else mode,
                                                                           "--threads", str(args.threads), "--workload", args.workload, "--pairs", str(args.pairs)],
                       stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("errsup_bench: a child run (%s) failed (exit %d, limit %d s)" % (mode, p.returncode, limit))
    return json.loads(lines[-1])


def kernel_times(args, tmp, mode):
    prof = os.path.join(tmp, "prof_" + mode)
    run_child(args, tmp, mode, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "errsup", "--output-format", "csv", "--"])
    kern = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_sup_\w+|k_err_\w+|k_reduce_scan", r["Name"])   # (the CSV holds the demangled name)
            if m:
                k = kern.setdefault(m.group(0), dict(calls=0, seconds=0.0))
                k["calls"] += int(r["Calls"]); k["seconds"] += float(r["TotalDurationNs"]) * 1e-9
    if not kern:
        raise SystemExit("errsup_bench: no kernel row in rocprofv3's *kernel_stats.csv under %s" % prof)
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
    ap.add_argument("--alt_lib", default=None, help="another build of libgencore_amd.so whose default variant runs in the same rounds (alt_onchip), through GCE_LIB")
    ap.add_argument("--alt_note", default=None, help="what --alt_lib is, in a sentence; kept in the result")
    ap.add_argument("--child", default=None)
    ap.add_argument("--mode", default="make")
    args = ap.parse_args()
    if args.child is not None:
        return child_make(args) if args.mode == "make" else child(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "errsup.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_errsup_")
    made = run_child(args, tmp, "make", limit=1100)
    variants = VARIANTS + (("alt_onchip",) if args.alt_lib else ())
    modes = ["%s_%s" % (v, f) for f in FILES for v in variants]
    per = {m: [] for m in modes}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for m in modes:
            r = run_child(args, tmp, m)
            if rep:
                per[m].append(r)
        print("errsup_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    spread = lambda rs, k: max(r[k] for r in rs) - min(r[k] for r in rs)
    res = dict(workload=args.workload, pairs=int(args.pairs), reps=args.reps, **made, bytes={f: os.path.getsize(os.path.join(tmp, f + ".bam")) for f in FILES},
               clocks="the library's stage times: host clocks around work that ends in a device synchronise",
               what="gce_bam_error_profile_support (onchip: the default; direct: GCE_ERRSUP_DIRECT) beside gce_bam_error_profile (cycle) on the same files, without a BED or a mask, "
                    "interleaved; out: the stream through the consensus engine at -s 1; in: the stream itself, no tags, every record in row (segment, absent, absent); no pass mark",
               files={})
    if args.alt_lib:
        res["alt_lib"] = args.alt_note or "another build of the library; its default variant is alt_onchip"
    for f in FILES:
        v = {}
        for var in variants:
            rs = per["%s_%s" % (var, f)]
            v[var] = dict(stages={k: round(med(rs, k), 5) for k in ("read_s", "inflate_index_s", "errprof_s", "write_s", "total_s", "wall_s")},
                          errprof_s_all=[round(r["errprof_s"], 5) for r in rs], total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                          counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_")}, sums={c: rs[0][c] for c in ("counts_sum", "counts_crc", "by_class_crc", "rows") if c in rs[0]})
        e = lambda var: v[var]["stages"]["errprof_s"]
        noise = max(spread(per["onchip_" + f], "errprof_s"), spread(per["direct_" + f], "errprof_s"))
        gap = e("direct") - e("onchip")
        dec = dict(rule="the on-chip variant stays the default only if its median errprof_s beats direct's by more than the spread of the values, on both files",
                   counters_identical=v["onchip"]["sums"] == v["direct"]["sums"] and v["onchip"]["counters"] == v["direct"]["counters"],
                   classes_equal_the_cycle_tables=v["onchip"]["sums"]["by_class_crc"] == v["cycle"]["sums"]["by_class_crc"],
                   direct_minus_onchip_s=round(gap, 5), spread_s=round(noise, 5), onchip_wins=gap > noise)
        ynoise = max(spread(per["onchip_" + f], "errprof_s"), spread(per["cycle_" + f], "errprof_s"))
        dec["against_the_cycle_profile"] = dict(onchip_minus_cycle_s=round(e("onchip") - e("cycle"), 5), spread_s=round(ynoise, 5), slower=e("onchip") - e("cycle") > ynoise)
        if args.alt_lib:
            anoise = max(spread(per["onchip_" + f], "errprof_s"), spread(per["alt_onchip_" + f], "errprof_s"))
            dec["against_alt_lib"] = dict(onchip_minus_alt_s=round(e("onchip") - e("alt_onchip"), 5), spread_s=round(anoise, 5),
                                          counters_identical=v["onchip"]["sums"] == v["alt_onchip"]["sums"])
        res["files"][f] = dict(variants=v, decision=dec)
    res["default"] = "onchip" if all(res["files"][f]["decision"]["onchip_wins"] for f in FILES) else "direct"
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")
    write()                                                       # (the timed rounds stand if a trace below fails: a failure ends the script)
    for f in FILES:
        for var in VARIANTS:
            res["files"][f]["variants"][var]["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run of this variant in a process of its own",
                                                               **kernel_times(args, tmp, "%s_%s" % (var, f)))
            write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
