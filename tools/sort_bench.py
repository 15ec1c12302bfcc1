#!/usr/bin/env python
"""Measurement of gce_bam_sort: the cfg3 stream of tools/bam_bench.py as a BAM in aligner order (pairs adjacent, pairs
shuffled) -> sort_bam at level -2 in fresh child processes (one warm-up, three timed, median) -> profiles/sort_bam.json with the stage times
of gce_sort_run, the gather kernel's time from a rocprofv3 --kernel-trace --stats run of its own, and one device-to-device hipMemcpyAsync of
the same bytes in the same process as the yardstick.
    python tools/sort_bench.py [--workload cfg3] [--pairs 4000000] [--threads 0] [--dir DIR] [--out profiles/sort_bam.json]
--passes measures gce_bam_sort_passes on the same file instead: T(P) for P = 1 (in-core), 2 and 4 (sort_bam_passes with min_passes = P, one
warm-up, --reps timed runs each, median) and k_sort_scatter's time from one rocprofv3 --kernel-trace --stats run at --min-passes, beside
the same device-to-device copy -> profiles/sort_bam_passes.json.  An unsorted.bam already in --dir is used as it is.
    python tools/sort_bench.py --passes [--min-passes 2] [--reps 3] [--dir DIR] [--out profiles/sort_bam_passes.json]
--sam measures gce_sam_sort: the same stream as SAM text (bam_to_sam of unsorted.bam -> unsorted.sam), sort_sam against the
composition sam_to_bam (level 1, 16 threads) + sort_bam, both at level -2.  Every run is a fresh child process under its own time limit; the
two variants are interleaved, one warm-up and --reps timed runs each, medians.  One rocprofv3 --kernel-trace --stats run of sort_sam in a
process of its own gives the k_sam_* kernels' times and the parse rate in text bytes per second -> profiles/sort_sam.json.  --lib PATH: the
composition's children load that build of the library (the parent commit's, for the yardstick); sort_sam always runs this tree's.
    python tools/sort_bench.py --sam [--reps 3] [--lib PATH] [--dir DIR] [--out profiles/sort_sam.json]"""
import argparse
import csv
import ctypes as C
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
import numpy as np  # noqa: E402


def d2d_copy_s(nbytes, reps=5):
    """seconds of one hipMemcpyAsync device-to-device of nbytes (the best of reps, after one untimed copy)"""
    hip = C.CDLL("libamdhip64.so")
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)) == 0
    assert hip.hipMemset(a, 1, C.c_size_t(nbytes)) == 0 and hip.hipMemset(b, 2, C.c_size_t(nbytes)) == 0 and hip.hipDeviceSynchronize() == 0
    best = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        assert hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, None) == 0 and hip.hipDeviceSynchronize() == 0      # 3: hipMemcpyDeviceToDevice
        dt = time.perf_counter() - t0
        if rep and (best is None or dt < best):
            best = dt
    hip.hipFree(a); hip.hipFree(b)
    return best


def aligner_order(batch):
    """the batch with its reads in the order an aligner writes: pairs in pseudo-random order, mates adjacent.  No per-record loop: a 64-bit
    hash of every read name (mates share it) by one reduceat over the name bytes, the reads ordered by it (stable: the first mate stays in
    front).  Only the per-read arrays are permuted; the blobs stay where they are (gce_batch's offsets are free-form)."""
    from gencore_amd.batch import ReadBatch
    c = batch.core
    off, lq = batch.qname_off.astype(np.int64), c["l_qname"].astype(np.int64)
    assert np.all(off[1:] == off[:-1] + lq[:-1]), "the names lie back to back in batch order"
    q = batch.qname[off[0]:off[-1] + lq[-1]].astype(np.uint64)
    pw = np.array([pow(1099511628211, k, 1 << 64) for k in range(256)], np.uint64)       # a polynomial hash mod 2^64 (a name is < 256 bytes)
    h = np.add.reduceat((q + np.uint64(1)) * pw[np.arange(len(q)) - np.repeat(off - off[0], lq)], off - off[0])
    perm = np.argsort(h * np.uint64(0x9E3779B97F4A7C15), kind="stable")
    kw = {f: getattr(batch, f) for f in ReadBatch.FIELDS}
    for f in ("core", "qname_off", "cigar_off", "seq_off", "qual_off", "nm", "nm_type", "mi_off"):
        if kw[f] is not None:
            kw[f] = np.ascontiguousarray(kw[f][perm])
    return ReadBatch(**kw)


def child(args):
    from gencore_amd.bamio import sort_bam, sort_bam_passes
    out = os.path.join(args.child, "sorted_%d.bam" % os.getpid())
    if args.child_min_passes < 0:
        r = sort_bam(os.path.join(args.child, "unsorted.bam"), out, device=0, threads=args.threads, level=-2)
    else:
        r = sort_bam_passes(os.path.join(args.child, "unsorted.bam"), out, device=0, threads=args.threads, level=-2, min_passes=args.child_min_passes)
    os.remove(out)
    r["d2d_copy_s"] = d2d_copy_s(r["inflated_bytes"])
    print(json.dumps(r), flush=True)


def child_sam(args):
    """one variant of --sam on unsorted.sam: `sort_sam`, or `compose` = sam_to_bam (level 1, 16 threads) + sort_bam; both write level -2"""
    from gencore_amd.bamio import sam_to_bam, sort_bam, sort_sam
    sam = os.path.join(args.child, "unsorted.sam")
    out = os.path.join(args.child, "sorted_%d.bam" % os.getpid())
    t0 = time.perf_counter()
    if args.child_sam == "sort_sam":
        r = sort_sam(sam, out, device=0, threads=args.threads, level=-2)
        r["wall_s"] = time.perf_counter() - t0
    else:
        mid = os.path.join(args.child, "mid_%d.bam" % os.getpid())
        sam_to_bam(sam, mid, threads=16, level=1)
        t1 = time.perf_counter()
        r = sort_bam(mid, out, device=0, threads=args.threads, level=-2)
        r["wall_s"] = time.perf_counter() - t0
        r["sam_to_bam_s"] = t1 - t0
        r["mid_bam_bytes"] = os.path.getsize(mid)
        os.remove(mid)
    os.remove(out)
    print(json.dumps(r), flush=True)


def run_child(args, tmp, prefix=(), min_passes=-1, sam=None, lib=None):
    env = dict(os.environ)
    if lib:
        env["GCE_LIB"] = lib
    p = subprocess.run(["timeout", "-k", "10", "600"] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--threads", str(args.threads),
                                                                      "--child-min-passes", str(min_passes)] + (["--child-sam", sam] if sam else []),
                       stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("sort_bench: a child run failed (exit %d)" % p.returncode)
    return json.loads(lines[-1])


def make_input(args, src):
    """the workload's stream in aligner order as a BAM file at src; -> the seconds it took to write"""
    import torch
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    d = synth.generate(args.workload, n_pairs=args.pairs, device=torch.device("cuda:0" if torch.cuda.is_available() else "cpu"))
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    unsorted = aligner_order(batch)
    t0 = time.time()
    write_batch_as_bam(src, unsorted, tl, names, text="@HD\tVN:1.6\tSO:unsorted\n", threads=args.threads, level=1)
    make_s = time.time() - t0
    print("sort_bench: %d records written in aligner order (%.1f s)" % (unsorted.n, make_s), flush=True)
    return make_s


def kernel_rows(prof, name):
    rows = []
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if name in r["Name"]]
    if not rows:
        raise SystemExit("sort_bench: no %s row in rocprofv3's *kernel_stats.csv under %s" % (name, prof))
    return rows


def passes_mode(args, tmp, src, make_s):
    run_child(args, tmp, min_passes=1)                           # warm-up: page cache, code objects
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    per_p = {}
    for P in (1, 2, 4):
        rs = [run_child(args, tmp, min_passes=P) for _ in range(args.reps)]
        print("sort_bench: min_passes %d: total_s %s" % (P, [round(r["total_s"], 3) for r in rs]), flush=True)
        r0 = rs[0]
        assert r0["in_core"] == (1 if P == 1 else 0) and (P == 1 or r0["n_passes"] == P), r0
        per_p[P] = dict(n_passes=r0["n_passes"], in_core=r0["in_core"], pass_bytes=r0["pass_bytes"], resident_bytes=r0["resident_bytes"], peak_device_bytes=r0["peak_device_bytes"],
                        total_s=round(med(rs, "total_s"), 4), total_s_all=[round(r["total_s"], 4) for r in rs],
                        stage_s_median={k: round(med(rs, k), 4) for k in ("read_s", "inflate_index_s", "sort_s", "gather_s", "write_s", "key_pass_s", "plan_s")},
                        pass_s=[round(x, 4) for x in r0["pass_s"]], d2d_copy_s=med(rs, "d2d_copy_s"))
    prof = os.path.join(tmp, "prof_passes")
    rp = run_child(args, tmp, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "sort", "--output-format", "csv", "--"], min_passes=args.min_passes)
    row = kernel_rows(prof, "k_sort_scatter")[0]
    nbytes = rp["inflated_bytes"]
    scatter_s = float(row["TotalDurationNs"]) * 1e-9
    copy_s = per_p[1]["d2d_copy_s"]
    res = dict(workload=args.workload, pairs=int(args.pairs), records=rp["n_records"], in_bam_bytes=os.path.getsize(src), inflated_bytes=nbytes, level=-2, reps=args.reps,
               make_input_s=round(make_s, 2), T={str(P): per_p[P]["total_s"] for P in per_p}, runs={str(P): per_p[P] for P in per_p},
               scatter_kernel=dict(source="rocprofv3 --kernel-trace --stats, a run of its own at min_passes %d" % args.min_passes, n_passes=rp["n_passes"], calls=int(row["Calls"]),
                                   seconds=scatter_s, bytes_moved=2 * nbytes, gb_per_s=round(2 * nbytes / scatter_s / 1e9, 1),
                                   note="all launches of all passes together move every record byte once; the launches also walk the records outside their pass's range"),
               d2d_copy=dict(source="one hipMemcpyAsync device-to-device of inflated_bytes in the sorting process, best of 5", seconds=round(copy_s, 6),
                             gb_per_s=round(2 * nbytes / copy_s / 1e9, 1)))
    res["scatter_over_copy"] = round(res["scatter_kernel"]["gb_per_s"] / res["d2d_copy"]["gb_per_s"], 3)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


def sam_mode(args, tmp, src, make_s):
    sam = os.path.join(tmp, "unsorted.sam")
    if not os.path.exists(sam):                                   # host only, in a child of its own
        p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-c", "import sys; sys.path.insert(0, %r); from gencore_amd.bamio import bam_to_sam; bam_to_sam(%r, %r, threads=%d)"
                            % (ROOT, src, sam, args.threads)])
        if p.returncode != 0:
            raise SystemExit("sort_bench: bam_to_sam failed (exit %d)" % p.returncode)
    text_bytes = os.path.getsize(sam)
    variants = (("sort_sam", None), ("compose", args.lib))
    for v, lib in variants:                                       # warm-up: page cache, code objects
        run_child(args, tmp, sam=v, lib=lib)
    runs = {"sort_sam": [], "compose": []}
    for _ in range(args.reps):                                    # interleaved: a drift of the machine falls on both
        for v, lib in variants:
            runs[v].append(run_child(args, tmp, sam=v, lib=lib))
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    for v in runs:
        print("sort_bench: %s: wall_s %s" % (v, [round(r["wall_s"], 3) for r in runs[v]]), flush=True)
    a, b = runs["sort_sam"], runs["compose"]
    assert a[0]["n_records"] == b[0]["n_records"] and a[0]["out_bytes"] == b[0]["out_bytes"], (a[0], b[0])
    stages = ("read_s", "inflate_index_s", "sort_s", "gather_s", "write_s", "total_s", "wall_s")
    prof = os.path.join(tmp, "prof_sam")
    rp = run_child(args, tmp, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "sort", "--output-format", "csv", "--"], sam="sort_sam")
    kern = {}
    for r in kernel_rows(prof, "k_sam_"):
        name = re.search(r"k_sam_\w+", r["Name"]).group(0)         # (the CSV holds the demangled name: "(anonymous namespace)::k_sam_size(...)")
        k = kern.setdefault(name, dict(calls=0, seconds=0.0))
        k["calls"] += int(r["Calls"]); k["seconds"] += float(r["TotalDurationNs"]) * 1e-9
    parse_s = sum(k["seconds"] for k in kern.values())
    res = dict(workload=args.workload, pairs=int(args.pairs), records=a[0]["n_records"], text_bytes=text_bytes, record_bytes=a[0]["inflated_bytes"], out_bam_bytes=a[0]["out_bytes"], level=-2,
               reps=args.reps, make_input_s=round(make_s, 2), n_host_lines=a[0]["n_host_lines"],
               sort_sam=dict(wall_s=round(med(a, "wall_s"), 4), wall_s_all=[round(r["wall_s"], 4) for r in a], peak_device_bytes=a[0]["peak_device_bytes"],
                             stage_s_median={k: round(med(a, k), 4) for k in stages}),
               composition=dict(library=args.lib or "this tree's", sam_to_bam="level 1, 16 threads", wall_s=round(med(b, "wall_s"), 4), wall_s_all=[round(r["wall_s"], 4) for r in b],
                                sam_to_bam_s=round(med(b, "sam_to_bam_s"), 4), mid_bam_bytes=b[0]["mid_bam_bytes"], peak_device_bytes=b[0]["peak_device_bytes"],
                                stage_s_median={k: round(med(b, k), 4) for k in stages}),
               parse_kernels=dict(source="rocprofv3 --kernel-trace --stats, a run of sort_sam in a process of its own", kernels={n: dict(calls=k["calls"], seconds=round(k["seconds"], 6)) for n, k in sorted(kern.items())},
                                  seconds=round(parse_s, 6), text_gb_per_s=round(text_bytes / parse_s / 1e9, 2), n_host_lines=rp["n_host_lines"]))
    res["composition_over_sort_sam"] = round(res["composition"]["wall_s"] / res["sort_sam"]["wall_s"], 3)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--min-passes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sam", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--child-sam", default=None, choices=["sort_sam", "compose"])
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-min-passes", type=int, default=-1)
    args = ap.parse_args()
    if args.child is not None:
        return child_sam(args) if args.child_sam else child(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sort_sam.json" if args.sam else "sort_bam_passes.json" if args.passes else "sort_bam.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_sort_")
    src = os.path.join(tmp, "unsorted.bam")
    make_s = 0.0
    if not os.path.exists(src):
        make_s = make_input(args, src)
    if args.sam:
        return sam_mode(args, tmp, src, make_s)
    if args.passes:
        return passes_mode(args, tmp, src, make_s)
    run_child(args, tmp)                                         # warm-up: page cache, code objects
    runs = [run_child(args, tmp) for _ in range(3)]
    print("sort_bench: total_s of the timed runs: %s" % [round(r["total_s"], 3) for r in runs], flush=True)
    med = lambda k: sorted(r[k] for r in runs)[1]
    r0 = runs[0]
    prof = os.path.join(tmp, "prof")
    run_child(args, tmp, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "sort", "--output-format", "csv", "--"])
    rows = kernel_rows(prof, "k_sort_gather")
    gather_s = float(rows[0]["AverageNs"]) * 1e-9
    nbytes = r0["inflated_bytes"]
    res = dict(workload=args.workload, pairs=int(args.pairs), records=r0["n_records"], n_descents=r0["n_descents"], in_bam_bytes=os.path.getsize(src), inflated_bytes=nbytes,
               out_bam_bytes=r0["out_bytes"], peak_device_bytes=r0["peak_device_bytes"], level=-2, make_input_s=round(make_s, 2),
               stage_s_median={k: round(med(k), 4) for k in ("read_s", "inflate_index_s", "sort_s", "gather_s", "write_s", "total_s")},
               total_s_all=[round(r["total_s"], 4) for r in runs],
               gather_kernel=dict(source="rocprofv3 --kernel-trace --stats, a run of its own", calls=int(rows[0]["Calls"]), seconds=gather_s,
                                  bytes_moved=2 * nbytes, gb_per_s=round(2 * nbytes / gather_s / 1e9, 1)),
               d2d_copy=dict(source="one hipMemcpyAsync device-to-device of inflated_bytes in the sorting process, best of 5", seconds=round(med("d2d_copy_s"), 6),
                             gb_per_s=round(2 * nbytes / med("d2d_copy_s") / 1e9, 1)))
    res["gather_over_copy"] = round(res["gather_kernel"]["gb_per_s"] / res["d2d_copy"]["gb_per_s"], 3)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
