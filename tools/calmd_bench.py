#!/usr/bin/env python
"""gce_bam_calmd on the output of a run: the cfg3 file of tools/bam_bench.py goes through run_bam once, and its output file --
consensus records with the MD of one read of their cluster -- through calmd_bam.
    python tools/calmd_bench.py [--workload cfg3] [--pairs 4000000] [--level -2] [--out profiles/calmd.json] [--stream --lib PARENT.so]
--stream: calmd_bam_stream with the auto budget, and with --resident_bytes forcing about 8 flushes on that file, beside calmd_bam of another
build of the library (--lib: the parent commit's, through GCE_LIB; never the code under test as its own yardstick); the variants are
interleaved.  A flush happens in front of a window and that file is less than one window of 64 MB, so the forced-flush variant reads it in
windows of a ninth of the file, and has a yardstick of its own: the parent's calmd_bam with the same windows.
Recorded: the stage times of calmd_bam (one warm-up and --reps timed runs, medians), one rocprofv3 --kernel-trace --stats run in a process
of its own for the k_md_* kernels, and as the yardstick a device-to-device copy of the bytes the kernels read and write (the inflated record
bytes in, the output record bytes out).  Every run is a fresh child process under its own time limit.  There is no pass mark."""
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


def child_calmd(args):
    from gencore_amd import bamio
    src, out = os.path.join(args.child, "out.bam"), os.path.join(args.child, "calmd.bam")
    with open(src, "rb") as f:                                    # the input in the page cache
        while f.read(1 << 26):
            pass
    t0 = time.perf_counter()
    if args.mode == "stream":
        r = bamio.calmd_bam_stream(src, out, os.path.join(args.child, "ref.fa"), threads=args.threads, level=args.level, window_bytes=int(args.window_bytes),
                                   resident_bytes=int(args.resident_bytes))
    else:
        r = bamio.calmd_bam(src, out, os.path.join(args.child, "ref.fa"), threads=args.threads, level=args.level, window_bytes=int(args.window_bytes))
    wall = time.perf_counter() - t0
    import hashlib
    h = hashlib.sha256()
    with open(out, "rb") as f:
        for piece in iter(lambda: f.read(1 << 26), b""):
            h.update(piece)
    print(json.dumps(dict(r.as_dict(), wall_s=wall, sha256=h.hexdigest())), flush=True)


def child_copy(args):
    import torch
    n = int(args.copy_bytes)
    a, b = torch.empty(n, dtype=torch.uint8, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0")
    a.zero_(); b.copy_(a); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    print(json.dumps(dict(bytes=n, seconds=round(sorted(ts)[len(ts) // 2], 7), seconds_all=[round(t, 7) for t in ts])), flush=True)


def run_child(args, tmp, mode, prefix=(), extra=(), lib=None):
    env = dict(os.environ)
    if lib:
        env["GCE_LIB"] = lib
    p = subprocess.run(["timeout", "-k", "10", "600"] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", mode, "--threads", str(args.threads),
                                                                      "--level", str(args.level)] + list(extra), stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("calmd_bench: a child run (%s) failed (exit %d)" % (mode, p.returncode))
    return json.loads(lines[-1])


def child_make(args):
    """in.bam (the stream), ref.fa (its reference) and out.bam (the run's output, level -2) under args.child"""
    import numpy as np
    import torch
    from gencore_amd import capi, synth
    from gencore_amd.bamio import run_bam, write_batch_as_bam
    d = synth.generate(args.workload, n_pairs=args.pairs, device=torch.device("cuda:0" if torch.cuda.is_available() else "cpu"))
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(os.path.join(args.child, "in.bam"), batch, tl, names, threads=args.threads, level=1)
    code = np.frombuffer(b"NATCG" + b"N" * 11, np.uint8)
    with open(os.path.join(args.child, "ref.fa"), "wb") as f:
        for nm, (nib, ln) in zip(names, d.reference_host()):
            if nib is None:
                continue
            both = np.empty(len(nib) * 2, np.uint8)
            both[0::2] = nib & 0xF
            both[1::2] = nib >> 4
            lines = np.concatenate([code[both[:ln]], np.zeros((-ln) % 60, np.uint8)]).reshape(-1, 60)
            body = np.concatenate([lines, np.full((len(lines), 1), 10, np.uint8)], 1).reshape(-1)
            f.write(b">" + nm.encode() + b"\n" + body.tobytes().replace(b"\0", b""))
    prm = capi.default_params(umi_prefix="auto", cluster_size_req=int(d.info["supporting_reads"]))
    r = run_bam(os.path.join(args.child, "in.bam"), os.path.join(args.child, "out.bam"), prm, fasta=os.path.join(args.child, "ref.fa"), threads=args.threads, level=-2)
    print(json.dumps(dict(reads=int(batch.n), records_out=int(r.n_out))), flush=True)


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
    ap.add_argument("--mode", default="calmd", choices=("make", "calmd", "stream", "copy"))
    ap.add_argument("--copy-bytes", default="0")
    ap.add_argument("--stream", action="store_true", help="measure calmd_bam_stream (auto budget; forced flushes) beside --lib's calmd_bam")
    ap.add_argument("--lib", default=None, help="another build of the library (the parent commit's) for the calmd_bam yardstick of --stream")
    ap.add_argument("--window_bytes", default="0", help="(child) compressed bytes per window; 0 = 64 MB")
    ap.add_argument("--resident_bytes", default="0", help="the cap of the forced-flush variant; 0 = an eighth of the output record bytes")
    args = ap.parse_args()
    if args.child is not None:
        return {"make": child_make, "calmd": child_calmd, "stream": child_calmd, "copy": child_copy}[args.mode](args)
    if args.stream and not (args.lib and os.path.exists(args.lib)):
        raise SystemExit("calmd_bench: --stream needs --lib, the parent commit's build of the library, for its yardstick")
    args.out = args.out or os.path.join(ROOT, "profiles", "calmd.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_calmd_")
    made = run_child(args, tmp, "make", extra=["--workload", args.workload, "--pairs", str(args.pairs)])
    stages = ("read_s", "inflate_index_s", "calmd_s", "write_s", "total_s", "wall_s")
    stream = None
    if args.stream:
        first = run_child(args, tmp, "calmd", lib=args.lib)        # warm-up: page cache, code objects (and the output's size, for the cap)
        cap = int(args.resident_bytes) or max(0xff00, int(first["out_record_bytes"]) // 8 // 0xff00 * 0xff00)
        win = ["--window_bytes", str(max(1 << 16, os.path.getsize(os.path.join(tmp, "out.bam")) // 9))]
        variants = dict(parent_in_core=dict(mode="calmd", lib=args.lib, extra=[]), stream_auto=dict(mode="stream", lib=None, extra=[]),
                        parent_in_core_windows=dict(mode="calmd", lib=args.lib, extra=win), stream_flush=dict(mode="stream", lib=None, extra=win + ["--resident_bytes", str(cap)]))
        per = {k: [] for k in variants}
        for rep in range(args.reps + 1):                           # interleaved; the first round is the warm-up
            for k, v in variants.items():
                r = run_child(args, tmp, v["mode"], extra=v["extra"], lib=v["lib"])
                if rep:
                    per[k].append(r)
            print("calmd_bench: round %d done" % rep, flush=True)
        medv = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
        assert len({r["sha256"] for rs in per.values() for r in rs}) == 1, "the variants wrote different files"
        stream = dict(yardstick="calmd_bam of the parent commit's build (GCE_LIB), in-core, the same input (stream_flush: with the same windows)", resident_bytes=cap, window_bytes=int(win[1]), sha256_equal=True,
                      variants={k: dict(stages={x: round(medv(rs, x), 4) for x in stages}, total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                                        **({} if k.startswith("parent") else dict(n_flushes=int(rs[0]["n_flushes"]), resident_cap_bytes=int(rs[0]["resident_cap_bytes"]), flushed_bytes=int(rs[0]["flushed_bytes"])))) for k, rs in per.items()})
        for k, y in (("stream_auto", "parent_in_core"), ("stream_flush", "parent_in_core_windows")):
            stream["variants"][k]["total_over_parent"] = round(stream["variants"][k]["stages"]["total_s"] / stream["variants"][y]["stages"]["total_s"], 3)
        runs = per["stream_auto"]
    else:
        run_child(args, tmp, "calmd")                              # warm-up: page cache, code objects
        runs = [run_child(args, tmp, "calmd") for _ in range(args.reps)]
    med = lambda k: sorted(r[k] for r in runs)[len(runs) // 2]
    prof = os.path.join(tmp, "prof_calmd")
    run_child(args, tmp, "stream" if args.stream else "calmd", prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "calmd", "--output-format", "csv", "--"])
    kern = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_md_\w+", r["Name"])                  # (the CSV holds the demangled name: "(anonymous namespace)::k_md_size(...)")
            if m:
                k = kern.setdefault(m.group(0), dict(calls=0, seconds=0.0))
                k["calls"] += int(r["Calls"]); k["seconds"] += float(r["TotalDurationNs"]) * 1e-9
    if not kern:
        raise SystemExit("calmd_bench: no k_md_ row in rocprofv3's *kernel_stats.csv under %s" % prof)
    moved = int(runs[0]["inflated_bytes"]) + int(runs[0]["out_record_bytes"])
    copy = run_child(args, tmp, "copy", extra=["--copy-bytes", str(moved // 2)])      # a copy of n bytes reads n and writes n
    md_s = sum(k["seconds"] for k in kern.values())
    res = dict(workload=args.workload, pairs=int(args.pairs), level=args.level, reps=args.reps, **made,
               counters={k: int(runs[0][k]) for k in ("n_records", "n_rewritten", "n_unchanged", "n_no_ref", "n_nm_changed", "n_md_changed")},
               inflated_bytes=int(runs[0]["inflated_bytes"]), out_record_bytes=int(runs[0]["out_record_bytes"]), out_bytes=int(runs[0]["out_bytes"]),
               **({} if stream else dict(peak_device_bytes=int(runs[0]["peak_device_bytes"]), stages={k: round(med(k), 4) for k in stages}, total_s_all=[round(r["total_s"], 4) for r in runs])),
               kernels=dict(source="rocprofv3 --kernel-trace --stats, one run in a process of its own", kernels={n: dict(calls=k["calls"], seconds=round(k["seconds"], 6)) for n, k in sorted(kern.items())},
                            seconds=round(md_s, 6), bytes_moved=moved, gb_per_s=round(moved / md_s / 1e9, 2)),
               yardstick=dict(what="device-to-device copy that reads and writes the same number of bytes", **copy, gb_per_s=round(moved / copy["seconds"] / 1e9, 2)))
    res["kernels_over_copy"] = round(md_s / copy["seconds"], 2)
    res["entry"] = "calmd_bam_stream (auto budget)" if args.stream else "calmd_bam"
    if stream:
        res["stream"] = stream
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:                                 # (--stream: the stage times are the variants', under "stream")
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
