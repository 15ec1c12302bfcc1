#!/usr/bin/env python
"""bench.py — consensus read-pairs/s of the HIP engine on BASELINE.json's workload, with the dominant kernel's
HBM roofline, the CPU baseline (oracle port, 1 thread and all host cores) and a parity check of the timed entry
points in the same JSON line.

    python bench.py --gpus 1 --steps 5 --warmup 2                       # default workload: cfg3 (10 M pairs, UMI, depth 8, -s 2)
    python bench.py --gpus N ...                                        # starts its own N ranks (torch.distributed.run, one per GPU, RCCL)
    python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs DIR    # + the last timed step's outputs as DIR/*.npy, to compare two builds
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...   # the driver's form

A "step" = one gce_process() pass of the whole hot path (clustering scan -> pairing/UMI grouping -> scoring ->
template pick + column vote -> duplex/filter/tags -> Stats -> output order + compaction) over one synthetic
coordinate-sorted stream that is already resident in HBM (gce_submit_device).  Every step (warm-up included) gets its
own pristine copy of the mutable seq/qual blobs, so no work is skipped or cached.
Multi-GPU (N > 1): ONE stream of N x pairs-per-GPU pairs is planned by every rank -- by default the workload of the one-GPU line, cfg3, N times as
large (10 M pairs PER GPU, the panel's targets grow with the stream): the per-GPU work is what it is at N = 1, so value(N) / value(1) is a scaling
figure (rounds 1-4 ran cfg4s = BASELINE configs[3] at N > 1, 12.5 M pairs per GPU at depth 16: another workload than the N = 1 line it is divided by;
`--workload cfg4s` still runs it) --, cut into N key ranges of equal read count (gencore_amd/synth.py plan/materialise, cuts fall inside contigs);
each rank materialises and processes only its own range, with the global ticks and the stream's flush events handed
to the engine — no data-path collective, one RCCL all-reduce for the Stats merge.  Weak scaling (per-GPU work fixed).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # first: the engine must share torch's HIP runtime

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s achievable copy rate


def _hip():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def device_batch(capi, t, n_reads, seq, qual, tick=None):
    b = capi.GceBatch()
    b.n_reads = n_reads
    b.core, b.qname_off, b.qname = t["core"].data_ptr(), t["qname_off"].data_ptr(), t["qname"].data_ptr()
    b.cigar_off, b.cigar = t["cigar_off"].data_ptr(), t["cigar"].data_ptr()
    b.seq_off, b.seq, b.qual_off, b.qual = t["seq_off"].data_ptr(), seq.data_ptr(), t["qual_off"].data_ptr(), qual.data_ptr()
    b.nm, b.nm_type = t["nm"].data_ptr(), t["nm_type"].data_ptr()
    b.mi_off, b.mi = None, None
    b.tick = tick.data_ptr() if tick is not None else None
    b.qname_bytes, b.cigar_words = t["qname"].numel(), t["cigar"].numel()
    b.seq_bytes, b.qual_bytes, b.mi_bytes = t["seq"].numel(), t["qual"].numel(), 0
    return b


def padded_clone(x):                                        # device blobs must be readable 16 bytes past their end
    y = torch.zeros(x.numel() + 64, dtype=x.dtype, device=x.device)
    y[:x.numel()].copy_(x)
    return y


def fetch_rows(capi, lib, eng):
    """gce_result_device -> numpy rows (the table of emitted records) + Stats blocks."""
    import numpy as np
    r = capi.GceResult()
    assert lib.gce_result_device(eng, C.byref(r)) == 0
    hip = _hip()
    n = int(r.n_out)

    def dev(ptr, count, dt):
        out = np.empty(count, dt)
        if count:
            assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out
    rows = {k: dev(getattr(r, k), n, dt) for k, dt in (("src", np.uint32), ("kind", np.uint8), ("qname_src", np.uint32), ("nm_new", np.int32),
                                                       ("fr", np.int16), ("rr", np.int16), ("mate", np.uint32), ("seq_off", np.uint64), ("qual_off", np.uint64))}
    rows["seq"], rows["qual"] = dev(r.seq, int(r.seq_bytes), np.uint8), dev(r.qual, int(r.qual_bytes), np.uint8)
    pre, post = capi.GceStats(), capi.GceStats()
    C.memmove(C.byref(pre), C.byref(r.pre), C.sizeof(capi.GceStats))
    C.memmove(C.byref(post), C.byref(r.post), C.sizeof(capi.GceStats))
    return rows, pre, post


DUMP_BYTES = 60 * 10 ** 6  # --dump-outputs: at most this much in all (under 64 MB in either unit)


def dump_outputs(out_dir, capi, lib, eng, core, budget, prefix="", extra=None):
    """What a caller of gce_result_device holds after the last step, as out_dir/<prefix><name>.npy: float64 where values can pass 2**24,
    float32 elsewhere.  Both Stats blocks and the record count always; the records -- row index, table fields, bases (packed bytes, the
    pad nibble of an odd-length read masked) and qualities, padded with -1 -- all of them if they fit in `budget` bytes, else a fixed,
    seeded sample of rows.  core: the batch's core block on the device (int32 [n_reads, 8], l_qseq in column 4)."""
    import numpy as np
    rows, pre, post = fetch_rows(capi, lib, eng)
    n = len(rows["src"])
    out = {"n_records": np.array([n], np.float64), "stats_pre": pre.as_array().astype(np.float64), "stats_post": post.as_array().astype(np.float64)}
    out.update({k: np.asarray(v).astype(np.float64) for k, v in (extra or {}).items()})
    L = int(core[:, 4].max().item()) if core.shape[0] else 0
    SB = (L + 1) // 2
    per_row = 6 * 8 + 4 * 4 + 4 * (SB + L)
    fixed = sum(a.nbytes for a in out.values()) + 256 * (len(out) + 12)          # (+ the .npy headers)
    k = max(0, min(n, (budget - fixed) // per_row))
    idx = np.arange(n, dtype=np.int64) if k == n else np.sort(np.random.default_rng(0).choice(n, k, replace=False))
    out["record_index"] = idx.astype(np.float64)
    for f in ("src", "qname_src", "mate", "seq_off", "qual_off"):
        out[f] = rows[f][idx].astype(np.float64)
    for f in ("kind", "nm_new", "fr", "rr"):
        out[f] = rows[f][idx].astype(np.float32)
    src = torch.from_numpy(rows["src"][idx].astype(np.int64)).to(core.device)
    lq = core[src, 4].cpu().numpy().astype(np.int64)

    def slices(blob, off, width, lens):                     # blob[off[r] + j] for j < lens[r], -1 beyond
        cols = np.arange(width, dtype=np.int64)[None, :]
        have = cols < lens[:, None]
        got = blob[np.where(have, off[:, None] + cols, 0)].astype(np.int32) if blob.size else np.zeros(have.shape, np.int32)
        return np.where(have, got, np.int32(-1)), have
    seq, _ = slices(rows["seq"], rows["seq_off"][idx].astype(np.int64), SB, (lq + 1) // 2)
    odd = np.nonzero(lq % 2 == 1)[0]
    seq[odd, lq[odd] // 2] &= 0xF0
    out["seq"] = seq.astype(np.float32)
    out["qual"] = slices(rows["qual"], rows["qual_off"][idx].astype(np.int64), L, lq)[0].astype(np.float32)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, prefix + name + ".npy"), a)


_CPU_JOBS = None      # set before the fork: the workers of the all-cores CPU baseline inherit the shards copy-on-write


def _cpu_shard_worker(k, barrier, q):
    """One process of the all-cores CPU baseline: the oracle over one contiguous shard of the sample."""
    import numpy as np
    from gencore_amd import capi
    from oracle import oracle_py
    sub, ctx, tl, umi_prefix, s_req, ref_host = _CPU_JOBS[k]
    tl = np.asarray(tl, np.uint32)
    prm = capi.default_params(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix=umi_prefix, cluster_size_req=s_req, **ctx)
    barrier.wait()
    t0 = time.perf_counter()
    res = oracle_py.run(sub, prm, ref_host)
    q.put((k, res.status, time.perf_counter() - t0, res.pre.as_array(), res.post.as_array()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default=None, help="cfg2 | cfg3 | cfg4s | cfg5 (gencore_amd/synth.py); default cfg3 at every N (N > 1: N x as many pairs, cut into N key ranges)")
    ap.add_argument("--pairs", type=int, default=None, help="override the workload's pair count (per GPU)")
    ap.add_argument("--scale", type=float, default=None, help="genome scale of cfg3 (1.0 = hg19 lengths, the default here)")
    ap.add_argument("--bed-targets", type=int, default=None, help="override the number of BED targets of cfg3 (0 = molecules spread uniformly)")
    ap.add_argument("--cpu-sample-pairs", type=int, default=2_000_000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--test-one-gpu", action="store_true", help="testing aid: every rank uses cuda:0 and torch.distributed runs over gloo, so the N > 1 code path (one stream cut into key ranges, ticks + flush events, Stats all-reduce) can be exercised on a 1-GPU box")
    ap.add_argument("--nccl-world1", action="store_true", help="testing aid: with --gpus 1, run the N > 1 code path (key-range plan, global ticks + flush events, the Stats payload all-reduced) "
                    "as a world of ONE rank over the nccl backend, so that the RCCL int64 all-reduce of the payload is loaded and executed on a 1-GPU box")
    ap.add_argument("--coverage-step", type=int, default=10000, help="Options::coverageStep of the depth statistics in the Stats merge (src/options.cpp:36)")
    ap.add_argument("--stats-merge", default="full", choices=["full", "counters"], help="what the ranks all-reduce after every step at N > 1: the whole Stats payload (counters + "
                    "histogram + per-contig depth bins + BED region counts, SURVEY 8e; gce_stats_payload_device) or the two counter blocks alone (rounds 1-4)")
    ap.add_argument("--align", type=int, default=1, help="byte alignment of each read's seq/qual slice in the SoA blobs")
    ap.add_argument("--layout", default="soa", choices=["soa", "record", "record64"], help="where a read's packed bases and qualities lie in HBM (gce_batch offsets are free-form): soa = two blobs "
                    "(bases of all reads, qualities of all reads); record = ONE blob, a read's qualities right behind its bases as in a BAM record (bam1_t: seq, then qual) -- 225 contiguous "
                    "bytes at 150 bp touch 4.5 sectors of 64 bytes where the two slices touch 5.5; record64 = the same with every record on a 64-byte boundary (256-byte stride at 150 bp: 4 sectors)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed -- both Stats blocks and a "
                    "seeded sample of the emitted records (table fields, bases, qualities) -- as DIR/<name>.npy in float32 / float64, at most 64 MB in all")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` by itself: start the N ranks here (one process per GPU under torch.distributed.run, RCCL) and become
        # the launcher -- the line rank 0 prints is this command's output
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.stdout.flush()
        os.execvpe(cmd[0], cmd, env)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(args.gpus, 1):
        raise SystemExit("bench.py: --gpus %d but the launcher started %d ranks (WORLD_SIZE)" % (args.gpus, world))
    if world > 1 and not args.test_one_gpu and torch.cuda.is_available() and torch.cuda.device_count() < world:
        raise SystemExit("bench.py: --gpus %d but only %d HIP devices are visible (use --test-one-gpu to put every rank on cuda:0)" % (world, torch.cuda.device_count()))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.test_one_gpu:
        local_rank = 0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the engine has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or args.nccl_world1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:                                      # --nccl-world1 without a launcher: a rendezvous of one
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        if args.test_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    workload = args.workload or "cfg3"

    import __graft_entry__ as ge
    if rank == 0:
        ge.build()
    if dist:
        dist.barrier()
    import numpy as np
    from gencore_amd import capi, synth
    from gencore_amd.batch import table_from_rows
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from parity_helpers import check_output_order, diff_results          # test infrastructure (the parity_checked leg only)
    from gencore_amd.capi import GceTiming
    lib = capi.load_library()
    dev = torch.device("cuda", local_rank)
    over = {}
    if workload == "cfg3":
        over["scale"] = args.scale if args.scale is not None else 1.0     # hg19-length contigs (3.04 Gb); tests use the 0.1 default
    if args.bed_targets is not None:
        over["bed_targets"] = args.bed_targets
    if workload == "cfg4s":
        over["scale"] = args.scale if args.scale is not None else 0.125 * world   # 100 M pairs over hg19 at 8 GPUs; an eighth of both per GPU

    # ------------------------------------------------------------------ workload (synthetic, generated on the GPU)
    stream_ctx = None
    if dist is None:
        data = synth.generate(workload, n_pairs=args.pairs, seed=0, device=dev, align=args.align, **over)
    else:
        per_gpu = args.pairs if args.pairs is not None else synth.CONFIGS[workload]["n_pairs"]
        data = synth.generate(workload, n_pairs=per_gpu * world, seed=0, device=dev, align=args.align, shard=(rank, world), **over)
        stream_ctx = data.stream_context
    t = data.t
    n_reads, n_pairs = data.n_reads, data.info["n_pairs"]
    tl = np.asarray(data.target_len, np.uint32)
    prm = capi.default_params(device=local_rank, n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix=data.info["umi_prefix"],
                              cluster_size_req=data.info["supporting_reads"])
    eng = C.c_void_p()
    rc = lib.gce_create(C.byref(prm), C.byref(eng))
    if rc:
        raise SystemExit("gce_create failed: %s" % lib.gce_status_message(rc).decode())
    for tid, (nib, ln) in enumerate(data.reference):
        assert lib.gce_set_reference(eng, tid, nib.data_ptr(), ln) == 0
    tick_dev = None
    if stream_ctx is not None:
        tick_dev = stream_ctx["tick"]
        et, ep = stream_ctx["ev_tid"], stream_ctx["ev_pos"]
        assert lib.gce_set_flush_events(eng, len(et), et.ctypes.data, ep.ctypes.data) == 0

    if args.layout != "soa":
        # one blob of records: [packed bases][qualities] per read; both base pointers of the batch are the blob's, the offsets tell the two apart
        SBl, Ll = (data.info["read_len"] + 1) // 2, data.info["read_len"]
        stride = SBl + Ll if args.layout == "record" else (SBl + Ll + 63) // 64 * 64
        sstr, qstr = t["seq"].numel() // n_reads, t["qual"].numel() // n_reads
        rec = torch.zeros(n_reads * stride + 64, dtype=torch.uint8, device=dev)
        rv = rec[:n_reads * stride].view(n_reads, stride)
        rv[:, :SBl] = t["seq"].view(n_reads, sstr)[:, :SBl]
        rv[:, SBl:SBl + Ll] = t["qual"].view(n_reads, qstr)[:, :Ll]
        t["seq_off"] = torch.arange(n_reads, dtype=torch.int64, device=dev) * stride
        t["qual_off"] = t["seq_off"] + SBl
        t["seq"] = t["qual"] = rec[:n_reads * stride]
        del rec, rv
    # one pristine copy of the mutable blobs per step while they fit in HBM (up to 40 % of what is free); beyond that a ring of copies,
    # refilled from the untouched blobs in t with the clock stopped, so that --steps sets the number of timed steps whatever it is
    blobs = ("seq",) if args.layout != "soa" else ("seq", "qual")
    per_copy = sum(t[b].numel() * t[b].element_size() + 64 for b in blobs)
    n_copies = min(args.steps + args.warmup, max(1, int(0.4 * torch.cuda.mem_get_info(dev)[0]) // per_copy))
    if dist:                                                # every rank refills at the same steps: the timed region's barriers must pair up
        nc = torch.tensor([n_copies], dtype=torch.int64, device=dev)
        dist.all_reduce(nc, op=dist.ReduceOp.MIN)
        n_copies = int(nc.item())
    seqs = [padded_clone(t["seq"]) for _ in range(n_copies)]
    quals = seqs if args.layout != "soa" else [padded_clone(t["qual"]) for _ in range(n_copies)]

    def refill():                                           # the ring is used up: every copy pristine again
        for k in range(n_copies):
            seqs[k][:t["seq"].numel()].copy_(t["seq"])
            if quals is not seqs:
                quals[k][:t["qual"].numel()].copy_(t["qual"])
    t["qname"] = padded_clone(t["qname"])

    stats_dev = torch.zeros(2 * capi.GCE_STATS_WORDS, dtype=torch.int64, device=dev)
    # the regions of the depth statistics: the workload's BED panel, or -- a whole-genome stream (configs[3]: "whole-genome BED") -- 200 bp every ~150 kb
    bed = data.info.get("bed")
    if bed is None:
        regs = []
        for tid_, ln_ in enumerate(tl):
            stp = max(int(data.info["genome_bases"]) // 20000, 1000)
            regs += [(tid_, a, a + 200) for a in range(stp // 2, max(int(ln_) - 200, 1), stp)]
        bed = np.asarray(regs, np.int64).reshape(-1, 3)
    r_tid, r_start, r_end = (np.ascontiguousarray(np.asarray(bed)[:, k], np.int32) for k in range(3))
    payload_lay = capi.GcePayloadLayout()

    def stats_payload():
        """gce_stats_payload_device: Stats blocks + depth bins + BED counts of this rank's reads and records as one int64 buffer in HBM -> (pointer, words)"""
        pp = C.c_void_p()
        rc = lib.gce_stats_payload_device(eng, args.coverage_step, len(r_tid), r_tid.ctypes.data, r_start.ctypes.data, r_end.ctypes.data, C.byref(pp), C.byref(payload_lay))
        if rc:
            raise SystemExit("gce_stats_payload_device failed: %s" % lib.gce_last_error(eng).decode())
        return pp, int(payload_lay.total_words)
    hip = _hip()
    timings, last_res = [], {}

    def step(k):
        b = device_batch(capi, t, n_reads, seqs[k % n_copies], quals[k % n_copies], tick_dev)
        rc = lib.gce_submit_device(eng, C.byref(b))
        rc = rc or lib.gce_process(eng)
        if rc:
            raise SystemExit("engine failed: %s" % lib.gce_last_error(eng).decode())
        r = capi.GceResult()
        lib.gce_result_device(eng, C.byref(r))
        if dist:                                            # the final Stats merge: ONE RCCL all-reduce over xGMI, device to device
            nonlocal stats_dev
            if args.stats_merge == "full":                  # counters + histogram + depth bins + BED region counts in one buffer (~5 MB at hg19 / 10 kb)
                sp, words = stats_payload()
                if stats_dev.numel() != words:
                    stats_dev = torch.zeros(words, dtype=torch.int64, device=dev)
            else:                                           # (gce_stats_device: both blocks as they lie in HBM, 2 x 114 int64)
                sp = C.c_void_p()
                assert lib.gce_stats_device(eng, C.byref(sp)) == 0
            assert hip.hipMemcpyAsync(C.c_void_p(stats_dev.data_ptr()), sp, C.c_size_t(stats_dev.numel() * 8), 3, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            dist.all_reduce(stats_dev)
        tm = GceTiming()
        lib.gce_get_timing(eng, C.byref(tm))
        timings.append(tm.as_dict())
        last_res["n_out"], last_res["pre"], last_res["post"] = int(r.n_out), r.pre.as_dict(), r.post.as_dict()

    def sync():
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
            torch.cuda.synchronize()

    for k in range(args.warmup):
        if k and k % n_copies == 0:
            sync()
            refill()
            sync()
        step(k)
    sync()
    elapsed, t0 = 0.0, time.perf_counter()
    for k in range(args.warmup, args.warmup + args.steps):
        if k and k % n_copies == 0:                         # the ring is used up: refilled with the clock stopped
            sync()
            elapsed += time.perf_counter() - t0
            refill()
            sync()
            t0 = time.perf_counter()
        step(k)
    sync()
    elapsed += time.perf_counter() - t0
    el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if dist:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    ms_per_step = elapsed * 1000.0 / args.steps
    if args.dump_outputs:                                   # the last timed step's result, still held by the engine (outside the timed region)
        dump_outputs(args.dump_outputs, capi, lib, eng, t["core"], DUMP_BYTES // world, prefix=("rank%d_" % rank) if world > 1 else "",
                     extra={"stats_merged": stats_dev.cpu().numpy()} if dist else None)
    # what the N > 1 step does that the N = 1 step does not -- the Stats payload (k_depth over the rank's reads and records, two passes) and its all-reduce --
    # timed ALONE behind the timed region (max over ranks), so that value(N) / value(1) can be read like for like: ms_per_step - merge_ms is the engine pass
    merge_ms = None
    if dist and args.stats_merge == "full":
        def merge_only():
            sp, words = stats_payload()
            assert hip.hipMemcpyAsync(C.c_void_p(stats_dev.data_ptr()), sp, C.c_size_t(stats_dev.numel() * 8), 3, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            dist.all_reduce(stats_dev)
        stats_keep = stats_dev.clone()
        merge_only(); sync()
        m0 = time.perf_counter()
        for _ in range(args.steps):
            merge_only()
        sync()
        mt = torch.tensor([time.perf_counter() - m0], dtype=torch.float64, device=dev)
        dist.all_reduce(mt, op=dist.ReduceOp.MAX)
        merge_ms = float(mt.item()) * 1000.0 / args.steps
        stats_dev.copy_(stats_keep)                         # (the line reports the sums of the last timed step: ONE all-reduce of them)
    total_pairs = torch.tensor([n_pairs], dtype=torch.int64, device=dev)
    if dist:
        dist.all_reduce(total_pairs)
    pairs_all = int(total_pairs.item())
    value = pairs_all / (ms_per_step / 1000.0)

    # ------------------------------------------------------------------ roofline of the dominant kernel (HIP events, timed steps only)
    timed = timings[args.warmup:]
    avg = {k: sum(x[k] for x in timed) / len(timed) for k in timed[0]}
    n_groups = max(1.0, avg["n_groups"])
    d = max(1.0, avg["n_pairs"]) / n_groups                 # mean group depth (pairs per UMI group)
    L = data.info["read_len"]
    per_read = (L + 1) // 2 + L + 4                         # seq + qual + one CIGAR word (229 B at 150 bp)
    consensus_bytes = n_pairs * (2 * per_read + (2 * ((L + 1) // 2 + L) + L) / d)    # 458 + 600/d per pair at 150 bp
    cluster_bytes = n_reads * 40.0                          # 32 B key record in + 8 B (slot, rank) out
    kernels = {
        "cluster": dict(ms=avg["cluster_ms"], algorithmic_bytes=cluster_bytes),
        "consensus": dict(ms=avg["score_ms"] + avg["consensus_ms"], algorithmic_bytes=consensus_bytes),
        "cluster_formation": dict(ms=avg["cluster_ms"] + avg["csr_ms"], algorithmic_bytes=cluster_bytes),
        # mate pairing + UMI grouping (A3-A5): every read name (the UMI is part of it) read once, one (left, right) pair record written per pair
        "pairing": dict(ms=avg["pairing_ms"], algorithmic_bytes=float(data.t["qname"].numel() - 64) + 8.0 * n_pairs),
    }
    for v in kernels.values():
        v["achieved_gbs"] = v["algorithmic_bytes"] / (v["ms"] * 1e-3) / 1e9 if v["ms"] > 0 else 0.0
        v["frac"] = v["achieved_gbs"] / HBM_PEAK_GBS
    phase_ms = {k: avg[k] for k in ("cluster_ms", "csr_ms", "describe_ms", "pairing_ms", "score_ms", "consensus_ms", "finish_ms", "output_ms", "total_ms")}
    dom = "consensus" if kernels["consensus"]["ms"] >= kernels["cluster"]["ms"] else "cluster"
    # HBM traffic of the dominant phase from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate runs of this
    # same command: profiles/hbm_traffic.json, tools/hbm_summary.py): bytes per launch, FETCH_SIZE doubled as MI355X_MICROARCH.md
    # prescribes for gfx950.  Quoted only for the workload it was measured on; PMC counters cannot be read inside this process.
    traffic, hj = None, {}
    tj = os.path.join(ROOT, "profiles", "hbm_traffic_%s.json" % workload)       # one file per workload (tools/hbm_summary.py); cfg3's is also profiles/hbm_traffic.json
    if not os.path.exists(tj):
        tj = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from hbm_summary import csrc_sha16                    # sha256 over gencore_amd/csrc: a traffic file is quoted only for the sources it was measured on
    src_hash, traffic_stale = csrc_sha16(), None
    if os.path.exists(tj) and args.pairs is None and world == 1:
        hj = json.load(open(tj))
        if hj.get("workload") == workload and hj.get("csrc_sha16") != src_hash:
            traffic_stale = "profiles/%s (%s) was measured on other sources (csrc_sha16 %s, tree %s): traffic dropped" % (os.path.basename(tj), hj.get("tag", "?"), hj.get("csrc_sha16"), src_hash)
        elif hj.get("workload") == workload:
            kk = hj["kernels"]
            names = {"consensus": hj.get("consensus_kernels", []), "cluster": ["k_cluster"]}     # (consensus_kernels: k_vote + k_score2 + k_consensus_fast/_slow, and the deep kernels where they run)
            traffic = {k: sum(kk[n]["fetch_bytes_x2"] + kk[n]["write_bytes"] for n in v if n in kk) for k, v in names.items()}
    roofline = dict(bound="hbm", kernel={"consensus": ("k_vote_deep + k_deep_prepare + k_score2 (+ k_vote's hand-on, k_consensus_fast): Pair::computeScore + Group::makeConsensus on deep groups" if d > 24 else
                                                       "k_vote (+ k_score2/k_consensus_fast/_slow for handed-on groups): Pair::computeScore + Group::makeConsensus"),
                                         "cluster": "k_cluster (clustering scan)"}[dom],
                    achieved=round(kernels[dom]["achieved_gbs"], 2), peak=HBM_PEAK_GBS, unit="GB/s",
                    frac=round(kernels[dom]["frac"], 5), traffic=(round(traffic[dom]) if traffic and traffic[dom] else None),
                    traffic_source=("static: profiles/hbm_traffic*.json (%s, csrc_sha16 %s = this tree), separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, not a measurement of this run" % (hj.get("tag", "?"), src_hash)) if traffic else traffic_stale,
                    algorithmic_bytes=round(kernels[dom]["algorithmic_bytes"]),
                    clustering_scan=dict(achieved=round(kernels["cluster"]["achieved_gbs"], 2), frac=round(kernels["cluster"]["frac"], 5),
                                         ms=round(kernels["cluster"]["ms"], 4), algorithmic_bytes=round(cluster_bytes),
                                         traffic=(round(traffic["cluster"]) if traffic and traffic["cluster"] else None)),
                    pairing=dict(what="k_pairing_sub<16|32> + fast/deep/generic + group tables: qname bytes once + 8 B per pair",
                                 ms=round(kernels["pairing"]["ms"], 4), algorithmic_bytes=round(kernels["pairing"]["algorithmic_bytes"]), frac=round(kernels["pairing"]["frac"], 5)),
                    cluster_formation=dict(what="everything that forms the clusters (SURVEY 8 A1-A3): k_cluster + tick scan + flush events + leader table + cluster/member lists, against the same 40 B/read; the bucket table is wiped by its users, no memset",
                                           ms=round(kernels["cluster_formation"]["ms"], 4), frac=round(kernels["cluster_formation"]["frac"], 5)),
                    phase_ms={k: round(v, 4) for k, v in phase_ms.items()}, mean_group_depth=round(d, 3), leader_runs=round(avg["n_leaders"]))
    # LDS figures of the per-column vote (north_star: "LDS hit-rate for the per-column vote"): static like `traffic`, from the committed SQ / LDS counter passes
    # (tools/lds_round.sh + lds_summary.py -> profiles/lds_<workload>.json), quoted only for the sources they were measured on
    lj = os.path.join(ROOT, "profiles", "lds_%s.json" % workload)
    if os.path.exists(lj) and args.pairs is None and world == 1:
        ld = json.load(open(lj))
        roofline["lds"] = ld["k_vote"] if ld.get("csrc_sha16") == src_hash else "profiles/%s was measured on other sources (csrc_sha16 %s, tree %s): dropped" % (os.path.basename(lj), ld.get("csrc_sha16"), src_hash)

    # ------------------------------------------------------------------ CPU baseline (oracle port) + parity of the timed entry points
    cpu, parity = None, None
    if rank == 0 and world == 1 and dist is None and not args.no_cpu_baseline:
        from oracle import oracle_py
        sample_pairs = min(args.cpu_sample_pairs, n_pairs)
        sd = synth.generate(workload, n_pairs=sample_pairs, seed=12345, device=dev, **over)
        sb = sd.to_batch()
        stl = np.asarray(sd.target_len, np.uint32)
        sprm = capi.default_params(device=local_rank, n_targets=len(stl), target_len=stl.ctypes.data, umi_prefix=sd.info["umi_prefix"],
                                   cluster_size_req=sd.info["supporting_reads"])
        ref_host = sd.reference_host()
        oracle_py.lib()
        c0 = time.perf_counter()
        res = oracle_py.run(sb, sprm, ref_host)
        cs = time.perf_counter() - c0
        assert res.status == 0
        # the same sample through the entry points timed above (gce_submit_device -> gce_process -> gce_result_device)
        seng = C.c_void_p()
        assert lib.gce_create(C.byref(sprm), C.byref(seng)) == 0
        for tid, (nib, ln) in enumerate(sd.reference):
            assert lib.gce_set_reference(seng, tid, nib.data_ptr(), ln) == 0
        st = sd.t
        s_seq, s_qual = padded_clone(st["seq"]), padded_clone(st["qual"])
        st["qname"] = padded_clone(st["qname"])
        sbd = device_batch(capi, st, sd.n_reads, s_seq, s_qual)
        assert lib.gce_submit_device(seng, C.byref(sbd)) == 0 and lib.gce_process(seng) == 0, lib.gce_last_error(seng)
        rows, pre, post = fetch_rows(capi, lib, seng)
        lib.gce_destroy(seng)
        got = table_from_rows(sb, rows, pre, post)
        diffs = diff_results(sb, got, res) + check_output_order(sb, rows)
        parity = dict(pairs=sd.info["n_pairs"], records=int(len(rows["src"])), ok=not diffs,
                      what="engine via gce_submit_device/gce_result_device vs oracle on the CPU-baseline sample: every emitted record "
                           "(bases, quals, NM, qname source, FR/RR, mate), both Stats blocks, bamComp order")
        if diffs:
            parity["first_diffs"] = diffs[:3]
        # all host cores: N independent processes on contiguous shards of the same sample cut where no cluster spans (the only way
        # the single-threaded reference scales), Stats merged and compared; wall time from a common start to the last result
        from gencore_amd.shard import effective_cpus
        cores = effective_cpus()                            # affinity mask capped by the cgroup CPU quota
        multi = None
        if cores > 1:
            import multiprocessing as mp
            from gencore_amd.shard import contiguous_cuts, shard_contiguous
            global _CPU_JOBS
            nproc = min(cores, 64)
            bounds = contiguous_cuts(sb.core, nproc, sd.target_len)
            _CPU_JOBS = []
            for r in range(nproc):
                if bounds[r] < bounds[r + 1]:
                    sub, _, ctx = shard_contiguous(sb, bounds, r)
                    _CPU_JOBS.append((sub, ctx, sd.target_len, sd.info["umi_prefix"], sd.info["supporting_reads"], ref_host))
            ctxm = mp.get_context("fork")
            barrier, q = ctxm.Barrier(len(_CPU_JOBS) + 1), ctxm.Queue()
            procs = [ctxm.Process(target=_cpu_shard_worker, args=(k, barrier, q)) for k in range(len(_CPU_JOBS))]
            for pr in procs:
                pr.start()
            barrier.wait()
            m0 = time.perf_counter()
            outs = [q.get(timeout=600) for _ in procs]
            ms_ = time.perf_counter() - m0
            for pr in procs:
                pr.join(60)
            ok = all(o[1] == 0 for o in outs) and np.array_equal(sum(o[3] for o in outs), res.pre.as_array()) and np.array_equal(sum(o[4] for o in outs), res.post.as_array())
            multi = dict(value=round(sd.info["n_pairs"] / ms_, 1), processes=len(procs), host_cores=cores, seconds=round(ms_, 2),
                         slowest_process_seconds=round(max(o[2] for o in outs), 2), stats_equal_single=bool(ok))
        oflags = [ln.split("?=", 1)[1].strip() for ln in open(os.path.join(ROOT, "oracle", "Makefile")) if ln.startswith("CFLAGS")]
        cpu = dict(value=round(sd.info["n_pairs"] / cs, 1), unit="read-pairs/s", cores=1, kind="port", port_vs_reference=None,
                   compiler="gcc " + (oflags[0] if oflags else "?") + " (oracle/Makefile; the reference builds -O3, /root/reference/Makefile:20)",
                   why_no_reference="reference gencore links htslib (Makefile:17), absent from this image and not to be stubbed: oracle/_ref holds only util.h's split; the port restates the reference function by function at -O3 and was never calibrated against it",
                   sample="%s generator, %d pairs, oracle/gencore_oracle.c single thread, %.1f s" % (workload, sd.info["n_pairs"], cs),
                   all_cores=multi)

    if rank == 0:
        pre = last_res.get("pre", {})
        out = {
            "metric": "consensus read-pairs/sec (whole node) + clustering HBM GB/s vs roofline",
            "value": round(value, 1), "unit": "read-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": "%s: %d paired %d bp reads per GPU, %s, mean cluster depth %.1f pairs (UMI groups: %.1f), -s %d, %s, genome %.2f Gb%s" % (
                workload, n_pairs, L, ("%d bp UMI" % data.info["umi_len"]) if data.info["umi_len"] else "no UMI", n_pairs / max(1, pre.get("clusters") or 1), d,
                data.info["supporting_reads"], ("one stream cut into %d key ranges" % world) if dist else "one stream",
                data.info["genome_bases"] / 1e9, (", %d BED targets x 200 bp" % data.info["bed_targets"]) if data.info.get("bed_targets") else ""),
                "pairs_per_gpu": n_pairs, "reads_per_gpu": n_reads, "records_out_per_gpu": last_res.get("n_out"),
                "clusters": pre.get("clusters"), "multi_molecule_clusters": pre.get("multi_molecule_clusters"),
                "parallelism": ("key-range shards x%d (cluster key (tid,left), global ticks + flush events), Stats all-reduce" % world) if dist else "single GPU"},
            "roofline": roofline, "cpu_baseline": cpu, "parity_checked": parity,
        }
        if dist:
            out["step_includes"] = ("gce_process + the Stats merge (gce_stats_payload_device: k_depth over this rank's reads and records, then ONE %s all-reduce of the payload); "
                                    "the N = 1 line times gce_process alone -- stats_merge_ms_per_step is the merge timed by itself behind the timed steps (max over ranks)"
                                    % ("gloo" if args.test_one_gpu else "RCCL"))
            out["stats_merge_ms_per_step"] = round(merge_ms, 4) if merge_ms is not None else None
            out["backend"] = "gloo (--test-one-gpu)" if args.test_one_gpu else "nccl (RCCL)"
        # the whole stream's Stats: at N > 1 the blocks every rank holds after the all-reduce (sums over the key-range shards), at N = 1 the
        # engine's own -- the same stream cut into 1 or N ranges must give the same numbers (tests/test_bench_ranks.py)
        names = ("reads", "bases", "reads_unmapped", "bases_unmapped", "base_mismatches", "reads_with_mismatches", "clusters", "multi_molecule_clusters",
                 "molecules", "molecules_se", "molecules_pe", "sscs", "dcs", "uncounted_supporting_reads")
        def depth_digest(v, lay):              # sums and a position-weighted checksum of the four vectors behind the Stats blocks
            nb, nr, o = int(lay.n_bins), int(lay.n_regions), 2 * capi.GCE_STATS_WORDS
            parts = {"pre_depth": v[o:o + nb], "post_depth": v[o + nb:o + 2 * nb], "pre_bed": v[o + 2 * nb:o + 2 * nb + nr], "post_bed": v[o + 2 * nb + nr:o + 2 * nb + 2 * nr]}
            dg = {k: {"sum": int(x.sum()), "checksum": int((x * (np.arange(len(x), dtype=np.int64) % 1000003 + 1)).sum() % (1 << 61))} for k, x in parts.items()}
            dg.update(coverage_step=args.coverage_step, depth_bins=nb, bed_regions=nr, payload_bytes=int(lay.total_words) * 8)
            return dg
        if dist:
            sv = stats_dev.cpu().numpy()
            W = capi.GCE_STATS_WORDS
            out["stats_whole_stream"] = {"pre": dict(zip(names, sv[:14].tolist())), "post": dict(zip(names, sv[W:W + 14].tolist())), "pre_hist_sum": int(sv[14:W].sum()), "post_hist_sum": int(sv[W + 14:2 * W].sum()),
                                         "how": ("one all-reduce(sum) of %d int64 = %.2f MB per rank straight from device memory (gce_stats_payload_device: counters + histogram + depth bins + BED region counts)" % (len(sv), len(sv) * 8 / 1e6))
                                                if args.stats_merge == "full" else "one all-reduce(sum) of 2 x %d int64 straight from device memory (gce_stats_device)" % W}
            if args.stats_merge == "full":
                out["stats_whole_stream"]["depth"] = depth_digest(sv, payload_lay)
        else:
            po = last_res.get("post", {})
            out["stats_whole_stream"] = {"pre": {k: pre.get(k) for k in names}, "post": {k: po.get(k) for k in names}, "pre_hist_sum": int(sum(pre.get("supporting_hist", []))),
                                         "post_hist_sum": int(sum(po.get("supporting_hist", []))), "how": "single engine"}
            sp, words = stats_payload()                # (outside the timed steps: one engine has nothing to merge)
            host = np.zeros(words, np.int64)
            assert lib.gce_stats_payload_read(eng, sp, words, host.ctypes.data) == 0
            out["stats_whole_stream"]["depth"] = depth_digest(host, payload_lay)
        if cpu:
            out["speedup_vs_cpu_port"] = round(value / cpu["value"], 2)
        line = json.dumps(out)
    lib.gce_destroy(eng)
    if dist:
        dist.destroy_process_group()
    if dist:                                                # RCCL writes a version banner through C stdio, which a pipe buffers until exit: out with it now, so that
        try:                                                # the JSON line is the LAST thing on stdout
            C.CDLL(None).fflush(None)
        except Exception:
            pass
    if rank == 0:
        sys.stdout.flush()
        print(line, flush=True)


if __name__ == "__main__":
    main()
