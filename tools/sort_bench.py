#!/usr/bin/env python
"""Measurement of gce_bam_sort: the cfg3 stream of tools/bam_bench.py as a BAM in aligner order (pairs adjacent, pairs
shuffled) -> sort_bam at level -2 in fresh child processes (one warm-up, three timed, median) -> profiles/sort_bam.json with the stage times
of gce_sort_run, the gather kernel's time from a rocprofv3 --kernel-trace --stats run of its own, and one device-to-device hipMemcpyAsync of
the same bytes in the same process as the yardstick.
    python tools/sort_bench.py [--workload cfg3] [--pairs 4000000] [--threads 0] [--dir DIR] [--out profiles/sort_bam.json]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
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
    from gencore_amd.bamio import sort_bam
    out = os.path.join(args.child, "sorted_%d.bam" % os.getpid())
    r = sort_bam(os.path.join(args.child, "unsorted.bam"), out, device=0, threads=args.threads, level=-2)
    os.remove(out)
    r["d2d_copy_s"] = d2d_copy_s(r["inflated_bytes"])
    print(json.dumps(r), flush=True)


def run_child(args, tmp, prefix=()):
    p = subprocess.run(["timeout", "-k", "10", "600"] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--threads", str(args.threads)], stdout=subprocess.PIPE, universal_newlines=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("sort_bench: a child run failed (exit %d)" % p.returncode)
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_bam.json"))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    import torch
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    d = synth.generate(args.workload, n_pairs=args.pairs, device=torch.device("cuda:0" if torch.cuda.is_available() else "cpu"))
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    unsorted = aligner_order(batch)
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_sort_")
    src = os.path.join(tmp, "unsorted.bam")
    t0 = time.time()
    write_batch_as_bam(src, unsorted, tl, names, text="@HD\tVN:1.6\tSO:unsorted\n", threads=args.threads, level=1)
    make_s = time.time() - t0
    print("sort_bench: %d records written in aligner order (%.1f s)" % (unsorted.n, make_s), flush=True)
    del d, batch, unsorted
    run_child(args, tmp)                                         # warm-up: page cache, code objects
    runs = [run_child(args, tmp) for _ in range(3)]
    print("sort_bench: total_s of the timed runs: %s" % [round(r["total_s"], 3) for r in runs], flush=True)
    med = lambda k: sorted(r[k] for r in runs)[1]
    r0 = runs[0]
    prof = os.path.join(tmp, "prof")
    run_child(args, tmp, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "sort", "--output-format", "csv", "--"])
    rows = []
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "k_sort_gather" in r["Name"]]
    if not rows:
        raise SystemExit("sort_bench: no k_sort_gather row in rocprofv3's *kernel_stats.csv under %s" % prof)
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
