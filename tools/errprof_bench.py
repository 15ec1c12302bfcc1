#!/usr/bin/env python
"""gce_bam_error_profile with its LDS planes beside the same pass with direct atomics (GCE_ERRPROF_DIRECT) and beside gce_bam_index, the
streaming floor over the same file: the cfg3 stream of tools/bam_bench.py as a BAM file, without a BED and with its panel as BED.
    python tools/errprof_bench.py [--workload cfg3] [--pairs 4000000] [--reps 3] [--direct_limit 900] [--out profiles/errprof.json]
The variants are interleaved; every run is a fresh child process under its own time limit (--limit; the direct variant, whose every add is a
global atomic on a few thousand addresses, has --direct_limit, and the file is never truncated for it); one warm-up round, then --reps timed
rounds, reported as medians with all values.  The question is which variant has the lower median errprof_s (the scan + k_err_count, host
clocks around work that ends in a device synchronise): the planes stay the default only if their median beats direct's by more than the
spread of the values.  gce_bam_index's gpu_s (inflate, record index and the index's kernels) stands beside errprof_s + inflate_index_s so
that the cost of the count kernels above read, inflate and index is visible.  One rocprofv3 --kernel-trace --stats run per variant, each in a
process of its own, gives the kernel times.  There is no pass mark.
    python tools/errprof_bench.py --fragments [--parent_lib PATH] [--out profiles/errprof_fragments.json]
runs gce_bam_error_profile_fragments (frag_planes, frag_direct) beside gce_bam_error_profile (planes, direct) on the same file,
without a BED, in the same interleaved way.  With --parent_lib, the library built from the parent commit (loaded through GCE_LIB) runs in the
same rounds: its gce_bam_error_profile (parent_planes) is the comparison partner, its gce_bam_error_profile_fragments (parent_frag_planes)
stands beside this tree's frag_planes, and its gce_bam_pileup_fragments (parent_pileup_fragments) beside this tree's (pileup_fragments),
whose join is gce_matejoin.hpp's: errprof_s and pileup_s are unchanged when the two medians differ by less than the spread of the values.
    python tools/errprof_bench.py --mask [--parent_lib PATH] [--out profiles/errprof_mask.json]
runs gce_bam_error_profile_masked beside gce_bam_error_profile on the same file, without a BED, in the same interleaved way:
planes (the unmasked entry point of this build), parent_planes and parent_mask_vcf (with --parent_lib: the parent commit's library,
through GCE_LIB), mask_vcf (a synthetic VCF of one SNP per 1000 reference bases) and mask_bed (a BED mask of about 10 % of the reference in
1 kb blocks).  It reports errprof_s, fill_s, load_s and peak_device_bytes, whether planes differs from parent_planes by more than the spread
of the values (a run without a mask is to pay nothing), and what the two masks cost over planes; one rocprofv3 --kernel-trace --stats run per masked variant, each in a process of
its own, gives k_mask_fill's own time beside fill_s, the host clock around set_mask."""
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
MODES = ("planes", "direct", "planes_bed", "direct_bed", "index")
FRAG_MODES = ("planes", "frag_planes", "direct", "frag_direct")
PARENT_MODES = ("parent_planes", "parent_frag_planes", "pileup_fragments", "parent_pileup_fragments")
MASK_MODES = ("planes", "mask_vcf", "mask_bed")


def child(args):
    import zlib
    from gencore_amd import bamio
    src, bed, fa = (os.path.join(args.child, n) for n in ("in.bam", "panel.bed", "ref.fa"))
    for p in (src, fa):                                           # the inputs in the page cache
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    mode = args.mode[len("parent_"):] if args.mode.startswith("parent_") else args.mode   # (the parent's library is GCE_LIB's doing, run_child)
    t0 = time.perf_counter()
    if mode == "index":
        d = bamio.index_bam(src, os.path.join(args.child, "in.bam.bai"), threads=args.threads)
        d = {k: v for k, v in (d if isinstance(d, dict) else vars(d)).items() if isinstance(v, (int, float))}
    elif mode.endswith("pileup_fragments"):
        r = bamio.pileup_fragments_bam(src, bed, threads=args.threads)
        d = dict(r.as_dict(), counts_sum=int(r.counts.sum()), counts_crc=int(zlib.crc32(r.counts.tobytes())))
    elif mode.startswith("mask_"):
        r = bamio.error_profile_masked_bam(src, fa, os.path.join(args.child, "mask.vcf" if mode == "mask_vcf" else "mask.bed"), tsv=os.path.join(args.child, "%s.tsv" % args.mode),
                                           threads=args.threads)
        d = dict(r.as_dict(), counts_sum=int(r.counts.sum()), counts_crc=int(zlib.crc32(r.counts.tobytes())), rows_sum_crc=int(zlib.crc32(r.counts.sum(axis=2).tobytes())))
    elif mode.startswith("frag_"):
        r = bamio.error_profile_fragments_bam(src, fa, tsv=os.path.join(args.child, "%s.tsv" % args.mode), overlap_tsv=os.path.join(args.child, "%s.overlap.tsv" % args.mode),
                                              threads=args.threads, direct=mode.endswith("direct"))
        d = dict(r.as_dict(), counts_sum=int(r.counts.sum()), counts_crc=int(zlib.crc32(r.counts.tobytes())), overlap_sum=int(r.overlap.sum()),
                 overlap_crc=int(zlib.crc32(r.overlap.tobytes())))
    else:
        r = bamio.error_profile_bam(src, fa, bed=bed if mode.endswith("_bed") else None, tsv=os.path.join(args.child, "%s.tsv" % args.mode), threads=args.threads,
                                    direct="direct" in mode)
        d = dict(r.as_dict(), counts_sum=int(r.counts.sum()), counts_crc=int(zlib.crc32(r.counts.tobytes())), rows_sum_crc=int(zlib.crc32(r.counts.sum(axis=2).tobytes())))
    print(json.dumps(dict(d, wall_s=time.perf_counter() - t0)), flush=True)


def child_make(args):
    """in.bam (the stream), ref.fa (its reference) and panel.bed (its panel) under args.child"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("errprof_bench: no GPU; nothing is measured without one")
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    d = synth.generate(args.workload, n_pairs=args.pairs, device=torch.device("cuda:0"))
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(os.path.join(args.child, "in.bam"), batch, tl, names, threads=args.threads, level=1)
    code = np.frombuffer(b"NATCG" + b"N" * 11, np.uint8)          # FastaReader's nibbles -> ASCII bases
    ref_bytes = 0
    with open(os.path.join(args.child, "ref.fa"), "wb") as f:
        for nm, (nib, ln) in zip(names, d.reference_host()):
            if nib is None:
                continue
            both = np.empty(len(nib) * 2, np.uint8)
            both[0::2] = nib & 0xF
            both[1::2] = nib >> 4
            lines = np.concatenate([code[both[:ln]], np.zeros((-ln) % 60, np.uint8)]).reshape(-1, 60)
            body = np.concatenate([lines, np.full((len(lines), 1), 10, np.uint8)], 1).reshape(-1)
            f.write(b">" + nm.encode() + b" synthetic\n" + body.tobytes().replace(b"\0", b""))
            ref_bytes += int(ln)
    bed = np.asarray(d.info["bed"])[:, :3]
    with open(os.path.join(args.child, "panel.bed"), "w") as f:
        for t, a, z in bed:
            f.write("%s\t%d\t%d\n" % (names[int(t)], int(a), int(z)))
    if not args.mask:
        print(json.dumps(dict(reads=int(batch.n), bed_regions=int(len(bed)), reference_bases=ref_bytes)), flush=True)
        return
    # ---- the masks of --mask: one SNP per 1000 reference bases as VCF, and about 10 % of the reference in 1 kb blocks as BED
    with open(os.path.join(args.child, "mask.vcf"), "w") as fv, open(os.path.join(args.child, "mask.bed"), "w") as fb:
        fv.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for nm, (nib, ln) in zip(names, d.reference_host()):
            if nib is None:
                continue
            for x in range(500, int(ln), 1000):
                fv.write("%s\t%d\t.\tN\t<X>\n" % (nm, x + 1))
            for x in range(2000, int(ln) - 1000, 10000):
                fb.write("%s\t%d\t%d\n" % (nm, x, x + 1000))
    print(json.dumps(dict(reads=int(batch.n), bed_regions=int(len(bed)), reference_bases=ref_bytes)), flush=True)


def run_child(args, tmp, mode, prefix=(), limit=None):
    limit = limit or (args.direct_limit if "direct" in mode else args.limit)
    env = dict(os.environ, GCE_LIB=os.path.abspath(args.parent_lib)) if mode.startswith("parent_") else None
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tmp, "--mode", mode, "--threads", str(args.threads),
                                                                           "--workload", args.workload, "--pairs", str(args.pairs)] + (["--mask"] if args.mask else []), stdout=subprocess.PIPE, universal_newlines=True, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        raise SystemExit("errprof_bench: a child run (%s) failed (exit %d, limit %d s)" % (mode, p.returncode, limit))
    return json.loads(lines[-1])


def kernel_times(args, tmp, mode):
    prof = os.path.join(tmp, "prof_" + mode)
    run_child(args, tmp, mode, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "errprof", "--output-format", "csv", "--"])
    kern = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_err_\w+|k_fragerr_\w+|k_frag_\w+|k_reduce_scan|k_mask_fill", r["Name"])   # (the CSV holds the demangled name)
            if m:
                k = kern.setdefault(m.group(0), dict(calls=0, seconds=0.0))
                k["calls"] += int(r["Calls"]); k["seconds"] += float(r["TotalDurationNs"]) * 1e-9
    if not kern:
        raise SystemExit("errprof_bench: no k_err_ row in rocprofv3's *kernel_stats.csv under %s" % prof)
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
    ap.add_argument("--child", default=None)
    ap.add_argument("--mode", default="planes", choices=("make",) + MODES + FRAG_MODES[1::2] + PARENT_MODES + MASK_MODES[1:] + ("parent_mask_vcf",))
    ap.add_argument("--mask", action="store_true", help="gce_bam_error_profile_masked beside gce_bam_error_profile; writes profiles/errprof_mask.json")
    ap.add_argument("--fragments", action="store_true", help="gce_bam_error_profile_fragments beside gce_bam_error_profile; writes profiles/errprof_fragments.json")
    ap.add_argument("--parent_lib", default=None, help="with --fragments or --mask: the parent commit's libgencore_amd.so, run in the same rounds through GCE_LIB")
    args = ap.parse_args()
    if args.child is not None:
        return child_make(args) if args.mode == "make" else child(args)
    if args.fragments:
        return main_fragments(args)
    if args.mask:
        return main_mask(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "errprof.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_errprof_")
    made = run_child(args, tmp, "make", limit=900)
    per = {m: [] for m in MODES}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for m in MODES:
            r = run_child(args, tmp, m)
            if rep:
                per[m].append(r)
        print("errprof_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    spread = lambda rs, k: max(r[k] for r in rs) - min(r[k] for r in rs)
    res = dict(workload=args.workload, pairs=int(args.pairs), reps=args.reps, **made, input_bytes=os.path.getsize(os.path.join(tmp, "in.bam")),
               clocks="the library's stage times: host clocks around work that ends in a device synchronise",
               limits=dict(planes_s=args.limit, direct_s=args.direct_limit, direct_file="the whole file, not truncated"), variants={})
    for m in MODES[:4]:
        rs = per[m]
        res["variants"][m] = dict(stages={k: round(med(rs, k), 5) for k in ("read_s", "inflate_index_s", "errprof_s", "write_s", "total_s", "wall_s")},
                                  errprof_s_all=[round(r["errprof_s"], 5) for r in rs], total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                                  counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_")}, counts_sum=rs[0]["counts_sum"], counts_crc=rs[0]["counts_crc"])
    rs = per["index"]
    res["index"] = dict(what="gce_bam_index on the same file, interleaved: the streaming floor; not a gate",
                        stages={k: round(med(rs, k), 5) for k in ("read_s", "gpu_s", "write_s", "total_s", "wall_s")}, gpu_s_all=[round(r["gpu_s"], 5) for r in rs],
                        total_s_all=[round(r["total_s"], 4) for r in rs])
    res["decision"] = {}
    for suffix in ("", "_bed"):
        t, d = res["variants"]["planes" + suffix], res["variants"]["direct" + suffix]
        gap = d["stages"]["errprof_s"] - t["stages"]["errprof_s"]
        noise = max(spread(per["planes" + suffix], "errprof_s"), spread(per["direct" + suffix], "errprof_s"))
        res["decision"]["bed" if suffix else "no_bed"] = dict(
            rule="the planes stay the default only if their median errprof_s beats direct's by more than the spread of the values",
            counters_identical=t["counts_crc"] == d["counts_crc"] and t["counters"] == d["counters"], counts_sum=t["counts_sum"],
            direct_minus_planes_s=round(gap, 5), spread_s=round(noise, 5), default="planes" if gap > noise else "direct")
    for m in MODES[:4]:
        v = res["variants"][m]
        v["gpu_s_beside_index"] = dict(errprof_s=v["stages"]["errprof_s"], inflate_index_s=v["stages"]["inflate_index_s"], index_gpu_s=res["index"]["stages"]["gpu_s"])
    for m in ("planes", "direct"):
        res["variants"][m]["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run of this variant in a process of its own", **kernel_times(args, tmp, m))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def against_parent(per, v, m, identical):
    """errprof_s of mode m beside the parent library's run of it, by the rule of every A/B here"""
    spread = lambda rs: max(r["errprof_s"] for r in rs) - min(r["errprof_s"] for r in rs)
    gap, noise = v[m]["stages"]["errprof_s"] - v["parent_" + m]["stages"]["errprof_s"], max(spread(per[m]), spread(per["parent_" + m]))
    return dict(rule="errprof_s is unchanged when the medians differ by less than the spread of the values", this_minus_parent_s=round(gap, 5), spread_s=round(noise, 5),
                unchanged=abs(gap) <= noise, counters_identical=identical)


def main_fragments(args):
    args.out = args.out or os.path.join(ROOT, "profiles", "errprof_fragments.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_fragerr_")
    made = run_child(args, tmp, "make", limit=900)
    modes = FRAG_MODES + (PARENT_MODES if args.parent_lib else ())
    per = {m: [] for m in modes}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for m in modes:
            r = run_child(args, tmp, m)
            if rep:
                per[m].append(r)
        print("errprof_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    spread = lambda rs, k: max(r[k] for r in rs) - min(r[k] for r in rs)
    res = dict(workload=args.workload, pairs=int(args.pairs), reps=args.reps, **made, input_bytes=os.path.getsize(os.path.join(tmp, "in.bam")),
               clocks="the library's stage times: host clocks around work that ends in a device synchronise",
               what="gce_bam_error_profile_fragments (frag_*) beside gce_bam_error_profile on the same file, without a BED, interleaved; no pass mark", variants={})
    for m in modes:
        rs = per[m]
        key = "pileup_s" if m.endswith("pileup_fragments") else "errprof_s"
        res["variants"][m] = dict(stages={k: round(med(rs, k), 5) for k in ("read_s", "inflate_index_s", key, "write_s", "total_s", "wall_s")},
                                  **{key + "_all": [round(r[key], 5) for r in rs]}, total_s_all=[round(r["total_s"], 4) for r in rs], peak_device_bytes=int(rs[0]["peak_device_bytes"]),
                                  share_of_total=round(med(rs, key) / med(rs, "total_s"), 4), counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_")},
                                  sums={c: rs[0][c] for c in ("counts_sum", "counts_crc", "overlap_sum", "overlap_crc") if c in rs[0]})
    v = res["variants"]
    same = lambda a, b: v[a]["sums"] == v[b]["sums"] and {k: c for k, c in v[a]["counters"].items() if k != "n_deferred"} == {k: c for k, c in v[b]["counters"].items() if k != "n_deferred"}
    res["counters_identical"] = dict(error_profile=same("planes", "direct"), fragments=same("frag_planes", "frag_direct"),
                                     overlap_sum_is_twice_shared=v["frag_planes"]["sums"]["overlap_sum"] == 2 * v["frag_planes"]["counters"]["n_shared_columns"])
    e = lambda m: v[m]["stages"]["errprof_s"]
    res["errprof_s_ratio"] = dict(frag_planes_over_planes=round(e("frag_planes") / e("planes"), 3), frag_direct_over_direct=round(e("frag_direct") / e("direct"), 3),
                                  frag_planes_over_frag_direct=round(e("frag_planes") / e("frag_direct"), 3))
    if args.parent_lib:
        res["errprof_s_ratio"]["frag_planes_over_parent_planes"] = round(e("frag_planes") / e("parent_planes"), 3)
        res["against_the_parent"] = {m: against_parent(per, v, m, same(m, "parent_" + m)) for m in ("planes", "frag_planes")}
        a, b = v["pileup_fragments"], v["parent_pileup_fragments"]
        gap = a["stages"]["pileup_s"] - b["stages"]["pileup_s"]
        noise = max(spread(per["pileup_fragments"], "pileup_s"), spread(per["parent_pileup_fragments"], "pileup_s"))
        res["pileup_fragments_after_the_move"] = dict(rule="pileup_s is unchanged when the medians differ by less than the spread of the values", this_minus_parent_s=round(gap, 5),
                                                      spread_s=round(noise, 5), unchanged=abs(gap) <= noise, counters_identical=same("pileup_fragments", "parent_pileup_fragments"))
    for m in FRAG_MODES:
        v[m]["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run of this variant in a process of its own", **kernel_times(args, tmp, m))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main_mask(args):
    args.out = args.out or os.path.join(ROOT, "profiles", "errprof_mask.json")
    tmp = args.dir or tempfile.mkdtemp(prefix="gce_errmask_")
    made = run_child(args, tmp, "make", limit=900)
    modes = MASK_MODES[:1] + (("parent_planes",) if args.parent_lib else ()) + MASK_MODES[1:2] + (("parent_mask_vcf",) if args.parent_lib else ()) + MASK_MODES[2:]
    per = {m: [] for m in modes}
    for rep in range(args.reps + 1):                               # interleaved; the first round is the warm-up
        for m in modes:
            r = run_child(args, tmp, m)
            if rep:
                per[m].append(r)
        print("errprof_bench: round %d done" % rep, flush=True)
    med = lambda rs, k: sorted(r[k] for r in rs)[len(rs) // 2]
    spread = lambda rs, k: max(r[k] for r in rs) - min(r[k] for r in rs)
    res = dict(workload=args.workload, pairs=int(args.pairs), reps=args.reps, **made, input_bytes=os.path.getsize(os.path.join(tmp, "in.bam")),
               clocks="the library's stage times: host clocks around work that ends in a device synchronise",
               what="gce_bam_error_profile_masked (mask_vcf: one SNP per 1000 reference bases; mask_bed: about 10 % of the reference in 1 kb blocks) beside gce_bam_error_profile "
                    "(planes; parent_planes: the parent commit's library) on the same file, without a BED, interleaved; no pass mark", variants={})
    for m in modes:
        rs = per[m]
        keys = ("read_s", "inflate_index_s", "errprof_s", "write_s", "total_s", "wall_s") + (("load_s", "fill_s") if "mask_" in m else ())
        res["variants"][m] = dict(stages={k: round(med(rs, k), 5) for k in keys}, errprof_s_all=[round(r["errprof_s"], 5) for r in rs], total_s_all=[round(r["total_s"], 4) for r in rs],
                                  peak_device_bytes=int(rs[0]["peak_device_bytes"]), counters={c: int(rs[0][c]) for c in rs[0] if c.startswith("n_")},
                                  sums={c: rs[0][c] for c in ("counts_sum", "counts_crc", "rows_sum_crc") if c in rs[0]})
        if "mask_" in m:
            res["variants"][m].update(fill_s_all=[round(r["fill_s"], 5) for r in rs], load_s_all=[round(r["load_s"], 5) for r in rs])
    v = res["variants"]
    e = lambda m: v[m]["stages"]["errprof_s"]
    res["rows_keep_their_sums"] = all(v[m]["sums"]["rows_sum_crc"] == v["planes"]["sums"]["rows_sum_crc"] for m in MASK_MODES[1:])
    res["cost_over_planes"] = {m: dict(errprof_s=round(e(m) - e("planes"), 5), errprof_s_ratio=round(e(m) / e("planes"), 3), fill_s=v[m]["stages"]["fill_s"], load_s=v[m]["stages"]["load_s"],
                                       peak_device_bytes=v[m]["peak_device_bytes"] - v["planes"]["peak_device_bytes"], spread_s=round(max(spread(per[m], "errprof_s"), spread(per["planes"], "errprof_s")), 5),
                                       masked_share_of_events=round(v[m]["counters"]["n_masked_events"] / max(v["planes"]["sums"]["counts_sum"], 1), 5)) for m in MASK_MODES[1:]}
    if args.parent_lib:
        gap = e("planes") - e("parent_planes")
        noise = max(spread(per["planes"], "errprof_s"), spread(per["parent_planes"], "errprof_s"))
        res["unmasked_against_the_parent"] = dict(rule="a run without a mask pays nothing when the medians differ by less than the spread of the values", this_minus_parent_s=round(gap, 5),
                                                  spread_s=round(noise, 5), unchanged=abs(gap) <= noise,
                                                  counters_identical=v["planes"]["sums"]["counts_crc"] == v["parent_planes"]["sums"]["counts_crc"] and v["planes"]["counters"] == v["parent_planes"]["counters"])
        res["masked_against_the_parent"] = against_parent(per, v, "mask_vcf", v["mask_vcf"]["sums"] == v["parent_mask_vcf"]["sums"] and v["mask_vcf"]["counters"] == v["parent_mask_vcf"]["counters"])
    for m in MASK_MODES[1:]:                                      # where fill_s goes: k_mask_fill's own time beside the host clock around set_mask
        try:
            v[m]["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, one run of this variant in a process of its own", **kernel_times(args, tmp, m))
        except SystemExit as e:                                   # (the timed rounds stand without the trace)
            v[m]["kernels"] = dict(source="no kernel trace: %s" % e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
