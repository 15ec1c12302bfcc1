"""The measurements behind level -3, on the GPU:

  sizes  [--parent-lib L]     deflate bytes of every payload of tests/test_gpu_deflate_dynamic.py at 65 280-byte blocks under fixed codes (codes=0), the
                              smallest of dynamic / fixed / stored (codes=1) and zlib level 1, and the cfg3 output FILE at levels -2, -3 and 1
                              -> profiles/deflate_dynamic_sizes.json; with --parent-lib also: level -2 bytes of one payload under that older build
  e2e    [--parent-lib L]     gce_run_bam file to file (cfg3, --pairs) at levels -3, -2 and 1 with 16 and 4 host threads, three repetitions, every run a
                              fresh process, interleaved; with --parent-lib level -2 under that build as the baseline -> profiles/deflate_dynamic_e2e.json
  kernel                      the two encoders once each on the same 100 MB record stream (run it under rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def device_name():
    import torch
    return torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none"


def make_input(tmp, pairs):
    import torch
    from gencore_amd import capi, synth
    from gencore_amd.bamio import write_batch_as_bam
    d = synth.generate("cfg3", n_pairs=pairs, device=torch.device("cuda:0"))
    tl = np.asarray(d.target_len, np.uint32)
    src = os.path.join(tmp, "in.bam")
    write_batch_as_bam(src, d.to_batch(), tl, ["chr%d" % (i + 1) for i in range(len(tl))], threads=16, level=1)
    return src, int(d.info["supporting_reads"])


def one_run(src, out, sreq, level, threads, warm=1):
    from gencore_amd import capi
    from gencore_amd.bamio import run_bam
    prm = capi.default_params(umi_prefix="auto", cluster_size_req=sreq)
    for _ in range(warm):
        run_bam(src, out, prm, threads=threads, level=level)
    t0 = time.time()
    r = run_bam(src, out, prm, threads=threads, level=level)
    return dict(wall_s=round(time.time() - t0, 4), total_s=round(r.total_s, 4), write_s=round(r.write_s, 4), out_bytes=os.path.getsize(out), n_out=int(r.n_out))


def sizes(args):
    import test_gpu_deflate_dynamic as T
    from gencore_amd.bamio import bgzf_deflate
    raw = lambda blob: sum(len(m[1]) for m in T.members_of(blob))

    def z1(d):
        t = 0
        for at in range(0, len(d), 0xff00):
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            t += len(co.compress(d[at:at + 0xff00]) + co.flush())
        return t
    rows = {"_note": "deflate bytes (BGZF framing excluded) at 65 280-byte blocks, written by tools/deflate_dynamic_profile.py sizes (device: %s): codes0 = fixed codes "
                     "(level -2), codes1 = the smallest of dynamic / fixed / stored per block (level -3), zlib1 = zlib.compressobj(1, DEFLATED, -15) per block; "
                     "cfg3_output_file: whole file sizes of gce_run_bam at levels -2 / -3 / 1 (input_bytes = the inflated file).  The encoder is deterministic: exact values." % device_name()}
    for name, d in T.payloads(np.random.default_rng(11)):
        rows[name] = dict(input_bytes=len(d), codes0_bytes=raw(bgzf_deflate(d, 0xff00, 0)), codes1_bytes=raw(bgzf_deflate(d, 0xff00, 1)), zlib1_bytes=z1(d))
        print(name, rows[name], flush=True)
    if args.parent_lib:
        from test_gpu_deflate import gpu_deflate
        d = T.record_stream()[:1 << 20]
        rc, pb = gpu_deflate(C.CDLL(args.parent_lib), d, 0xff00)
        same = rc == 0 and pb == bgzf_deflate(d, 0xff00, 0)
        rows["_level_minus_2_against_parent_build"] = dict(payload_bytes=len(d), blob_bytes=len(pb), identical=bool(same))
        print("level -2 bytes identical to the parent build:", same, flush=True)
    import gzip
    with tempfile.TemporaryDirectory(prefix="gce_dyn_") as tmp:
        src, sreq = make_input(tmp, args.pairs)
        out = os.path.join(tmp, "out.bam")
        f = {lv: one_run(src, out, sreq, lv, 16, warm=0)["out_bytes"] for lv in (-2, -3, 1)}
        unc = sum(m[3] for m in T.members_of(open(out, "rb").read()))
    rows["cfg3_output_file"] = dict(pairs=args.pairs, input_bytes=unc, codes0_bytes=f[-2], codes1_bytes=f[-3], zlib1_bytes=f[1])
    print("cfg3_output_file", rows["cfg3_output_file"], flush=True)
    json.dump(rows, open(args.out or os.path.join(ROOT, "profiles", "deflate_dynamic_sizes.json"), "w"), indent=1)


def e2e(args):
    tmp = tempfile.mkdtemp(prefix="gce_dyn_")
    try:
        e2e_in(args, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def e2e_in(args, tmp):
    src, sreq = make_input(tmp, args.pairs)
    res = dict(workload="cfg3", pairs=args.pairs, input_file_bytes=os.path.getsize(src), note="every run a fresh process: one warm-up run, then the timed one; "
               "total_s / write_s: gce_run_bam's own clock; 'parent' = level -2 under the build of the parent commit", runs=[])
    variants = [("this", -3), ("this", -2)] + ([("parent", -2)] if args.parent_lib else []) + [("this", 1)]
    for rep in range(3):
        for threads in (16, 4):
            for lib, level in variants:
                env = dict(os.environ)
                if lib == "parent":
                    env["GCE_LIB"] = args.parent_lib
                o = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child", "--src", src, "--sreq", str(sreq), "--level", str(level),
                                    "--threads", str(threads)], env=env, stdout=subprocess.PIPE, universal_newlines=True)
                if o.returncode != 0:
                    print("child failed:", lib, level, threads, o.returncode, flush=True)
                    sys.exit(1)                                                        # nothing more is started on the GPU after a failure
                row = dict(rep=rep, threads=threads, build=lib, level=level, **json.loads(o.stdout.strip().splitlines()[-1]))
                res["runs"].append(row)
                print(row, flush=True)
    med = {}
    for r in res["runs"]:
        med.setdefault("%s_level_%d_threads_%d" % (r["build"], r["level"], r["threads"]), []).append(r["total_s"])
    res["median_total_s"] = {k: sorted(v)[len(v) // 2] for k, v in med.items()}
    print(res["median_total_s"], flush=True)
    res["device"] = device_name()
    if args.kernel_stats:                                                                  # the *_kernel_stats.csv of `rocprofv3 --kernel-trace --stats -- ... kernel`
        import csv
        rows = [r for r in csv.DictReader(open(args.kernel_stats)) if "deflate" in r["Name"]]
        res["encoder_kernels"] = dict(note="rocprofv3 --kernel-trace --stats of `deflate_dynamic_profile.py kernel`: each encoder twice on the same record stream "
                                           "(tests' cfg3 stream x 40, 65 280-byte blocks), a run of its own", input_bytes=args.kernel_bytes,
                                      stats=[{k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r} for r in rows])
        print(res["encoder_kernels"], flush=True)
    json.dump(res, open(args.out or os.path.join(ROOT, "profiles", "deflate_dynamic_e2e.json"), "w"), indent=1)


def child(args):
    out = os.path.join(os.path.dirname(args.src), "out_%d.bam" % os.getpid())
    print(json.dumps(one_run(args.src, out, args.sreq, args.level, args.threads)))
    os.remove(out)


def kernel(args):
    import test_gpu_deflate_dynamic as T
    from gencore_amd.bamio import bgzf_deflate
    d = T.record_stream() * 40
    for codes in (0, 1, 0, 1):
        t0 = time.time()
        b = bgzf_deflate(d, 0xff00, codes)
        print("codes", codes, "in", len(d), "out", len(b), "call_s", round(time.time() - t0, 3), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sizes", "e2e", "kernel", "child"])
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, help="e2e: fold this rocprofv3 kernel_stats.csv of the `kernel` run into the json")
    ap.add_argument("--kernel-bytes", type=int, default=None, help="e2e: the input bytes the `kernel` run printed")
    ap.add_argument("--src"); ap.add_argument("--sreq", type=int); ap.add_argument("--level", type=int); ap.add_argument("--threads", type=int)
    a = ap.parse_args()
    {"sizes": sizes, "e2e": e2e, "kernel": kernel, "child": child}[a.what](a)
