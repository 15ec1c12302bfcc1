"""One engine over many streams, against the oracle after every step.

Every other parity test builds a fresh engine for one stream.  bench.py, the pass runner and the file runners do not: they reuse one engine
step after step, and several optimisations are right only if the step before left the engine in the right state -- the bucket table that
k_scatter wipes instead of a per-step memset (engine.hip `tab_clean`), the upload cache of reference and params, buffers that grow and are
never cleared, and what survives gce_reset (include/gencore_amd.h).  Each test here drives one engine (or two interleaved ones) through a
sequence of streams and requires after EVERY step:
  - the table of the step bit-exact with the oracle's for that stream alone (diff_results, the bamComp order, both Stats blocks);
  - k_vote's group counters and the pairing tiers of a fresh engine on the same stream (per step, not summed over the engine's life);
  - where a step asks for depth, gce_depth_stats and the Stats payload equal to oracle.depth_stats.
The CPU tests at the bottom check the properties the sequences rely on: the colliding streams share every cluster key, the error streams
have the oracle statuses the sequences expect, and the reference changes really change the oracle's output."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import fuzzgen
import pybam
from parity_helpers import check_output_order, diff_results

CODE2BASE = np.frombuffer(b"NATCGNNNNNNNNNNN", np.uint8)       # FastaReader's 4-bit code (A=1, T=2, C=3, G=4, other 0)


# ---------------------------------------------------------------------------------------------------------------------------- streams
def _ascii(nib, n):
    """The upper-case ASCII of a contig in FastaReader's code (low nibble = even position)."""
    nib = np.asarray(nib, np.uint8)
    codes = np.empty(2 * len(nib), np.uint8)
    codes[0::2], codes[1::2] = nib & 0xF, nib >> 4
    return CODE2BASE[codes[:n]].tobytes()


def _records(batch):
    """python records (dicts) of a ReadBatch, for ReadBatch.from_records and pybam.record_bytes"""
    out = []
    for i in range(batch.n):
        c = batch.core[i]
        mi = None
        if batch.mi_off is not None and int(batch.mi_off[i]) != 0xFFFFFFFFFFFFFFFF:
            mi = bytes(batch.mi[int(batch.mi_off[i]):]).split(b"\0")[0].decode()
        out.append(dict(qname=batch.qname_of(i), flag=int(c["flag"]), tid=int(c["tid"]), pos=int(c["pos"]), cigar=batch.cigar_of(i) or "*",
                        mtid=int(c["mtid"]), mpos=int(c["mpos"]), isize=int(c["isize"]), seq=batch.seq_of(i), qual=batch.qual_of(i).tolist(),
                        mapq=int(c["mapq"]), bin=int(c["bin"]), nm=(int(batch.nm[i]) if batch.nm_type[i] else None),
                        nm_type=(chr(batch.nm_type[i]) if batch.nm_type[i] else "C"), mi=mi))
    return out


def _cluster_keys(batch):
    """(tid, left, |isize|) of every read that reaches the cluster map (gencore.cpp:295-312)"""
    from gencore_amd.shard import cluster_left, clustered_mask
    core = batch.core
    cm = clustered_mask(core)
    left = cluster_left(core)
    return {(int(t), int(l), abs(int(s))) for t, l, s in zip(core["tid"][cm], left[cm], core["isize"][cm])}


def colliding_pair(seed=910):
    """Stream A (a fuzz case) and stream B with exactly A's cluster keys: per cluster key of A the first read and the reads of its name, under
    a new name and a new UMI -- so fewer reads, other names, other UMIs.  Both stay far below 1638 reads: the bucket table then has the same
    size (4096 buckets) in both steps, and a bucket of A that nobody wiped is the home bucket of the same key in B."""
    from gencore_amd.batch import ReadBatch
    from gencore_amd.shard import cluster_left, clustered_mask
    a, over, reference, contig_len = fuzzgen.make_case(seed, n_mol=60, umi_mode="prefix", period=10000)
    over.update(skip_low_complexity_cluster_threshold=1000, cluster_size_req=1)
    recs = _records(a)
    cm, left = clustered_mask(a.core), cluster_left(a.core)
    seen, keep_names = set(), {}
    for i in range(a.n):
        if not cm[i]:
            continue
        k = (int(a.core["tid"][i]), int(left[i]), abs(int(a.core["isize"][i])))
        if k not in seen:
            seen.add(k)
            keep_names.setdefault(recs[i]["qname"], len(keep_names))
    b = []
    for i, r in enumerate(recs):
        if r["qname"] in keep_names:
            j = keep_names[r["qname"]]
            umi = "".join("ACGT"[(j >> (2 * q)) & 3] for q in range(5))         # (five bases: A has UMIs of 4, 6 and 8)
            b.append(dict(r, qname="COL:%d:UMI_%s" % (j, umi), mi=None))
    return a, ReadBatch.from_records(b), fuzzgen.make_params(over, contig_len), reference


def _base_rec(**kw):
    r = dict(flag=99, tid=0, cigar="20M", mtid=0, isize=50, seq="ACGTACGTACGTACGTACGT", qual=[37] * 20, nm=0)
    r.update(kw)
    return r


def error_streams(reference):
    """(name, status, batch, staged reference, window) of every fatal path of test_error_codes_match_reference_fatal_paths and
    tests/stress_small.py, on the colliding streams' contigs and parameters (umi_prefix "UMI"): the oracle's status, except for the window
    stream (the oracle stages whole contigs; the engine, given a window that misses the reads, fails with GCE_ERR_REF_WINDOW)."""
    from gencore_amd.batch import ReadBatch
    from oracle import oracle_py
    ref_seq = "ACGTACGTACGTACGTACGT"
    lowq = [37] * 20
    lowq[3] = 2
    bad = ref_seq[:3] + "A" + ref_seq[4:]
    nm_ref = [(oracle_py.pack_reference("G" * 100 + ref_seq + "G" * 200), 320)] + list(reference[1:])
    pair = [_base_rec(qname="a:UMI_AAAA", pos=100, mpos=130), _base_rec(qname="a:UMI_AAAA", flag=147, pos=130, mpos=100, isize=-50)]
    return [
        ("unsorted", -10, [_base_rec(qname="a:UMI_AAAA", pos=500, mpos=530), _base_rec(qname="b:UMI_CCCC", pos=100, mpos=130)], reference, None),
        ("mi_mismatch", -11, [_base_rec(qname="a:UMI_AAAA", pos=100, mpos=130, mi="x:UMI_AAAA"),
                              _base_rec(qname="a:UMI_AAAA", flag=147, pos=130, mpos=100, isize=-50, mi="x:UMI_CCCC")], reference, None),
        ("nm_missing", -12, [_base_rec(qname="a:UMI_AAAA", pos=100, mpos=130, seq=bad, qual=lowq, nm=None),
                             _base_rec(qname="a:UMI_AAAA", flag=147, pos=130, mpos=100, isize=-50, nm=None)], nm_ref, None),
        ("umi_parse", -13, [_base_rec(qname="readUI", pos=100, mpos=130)], reference, None),
        ("ref_window", -15, pair, reference, (1000, 2000)),
    ]


def error_batch(recs):
    from gencore_amd.batch import ReadBatch
    return ReadBatch.from_records(recs)


def reference_variants(reference):
    """Contig 0 with every 5th base of [0, 3000) changed: a second reference of the same length."""
    nib, n = reference[0]
    a = bytearray(_ascii(nib, n))
    for i in range(0, min(n, 3000), 5):
        a[i] = {65: 67, 67: 71, 71: 84, 84: 65}.get(a[i], 65)
    from oracle import oracle_py
    alt = bytes(a)
    return _ascii(nib, n), alt, oracle_py.pack_reference(alt.decode())


def reference_case(seed=920):
    """A fuzz case whose molecules lie on contig 0 (window [0, 3000)), with reference arbitration (isize != 0) on most of them."""
    from gencore_amd.batch import ReadBatch
    batch, over, reference, contig_len = fuzzgen.make_case(seed, n_mol=60, umi_mode="prefix", period=10000)
    recs = [r for r in _records(batch) if r["tid"] == 0 and r["mtid"] == 0 and 0 <= r["pos"] and r["pos"] + 400 < 3000 and 0 <= r["mpos"] < 2600]
    over.update(skip_low_complexity_cluster_threshold=1000, cluster_size_req=1)
    return ReadBatch.from_records(recs), fuzzgen.make_params(over, contig_len), reference, contig_len


# ---------------------------------------------------------------------------------------------------------------------------- the engine side
_DIRTY = []


def _dirty_device_memory():
    """Before the module's first engine: fill and free a quarter GB of device memory (as tests/stress_small.py does), so that a new
    allocation that assumes zeros sees garbage instead."""
    if _DIRTY:
        return
    import torch
    g = torch.empty(1 << 28, dtype=torch.uint8, device="cuda").fill_(0xAB)
    del g
    torch.cuda.empty_cache()
    _DIRTY.append(True)


def _stage(e, reference):
    """Every contig of `reference` staged on engine e; None = removed (gce_set_reference with a null pointer)."""
    for tid, (nib, ln) in enumerate(reference):
        if nib is None:
            assert e.lib.gce_set_reference(e._h, tid, None, 0) == 0
        else:
            e.set_reference(tid, nib, ln)


def _engine(prm):
    from gencore_amd.engine import Engine
    _dirty_device_memory()
    return Engine(prm)


def _signature(e):
    """What a step's counters must equal on a fresh engine: k_vote's group count and the clusters per pairing tier.  (The vote-round and
    hand-on counters depend on which groups share a vote batch, i.e. on the cluster numbering, which follows the claiming leaders of the
    bucket table and may differ between two runs of the same stream: a fresh engine gave 54 handed-on sides where the reused one gave 56,
    with bit-identical tables.)"""
    return dict(groups=e.vote_counters()["groups"], tiers=e.pairing_tiers()[2])


def _fresh(prm, batch, reference, events=None):
    e = _engine(prm)
    try:
        if events is not None:
            e.set_flush_events(*events)
        _stage(e, reference)
        e.add_reads(batch)
        e.finish()
        return e.output(batch), _signature(e)
    finally:
        e.close()


def _want(batch, prm, reference, events=None):
    from oracle import oracle_py
    w = oracle_py.run(batch, prm, reference, events)
    assert w.status == 0, w.message
    return w


def check_step(tag, e, batch, prm, reference, got, events=None, want=None, fresh=True):
    """The step just processed on e: its table vs the oracle, its counters vs a fresh engine's on the same stream."""
    want = want if want is not None else _want(batch, prm, reference, events)
    diffs = diff_results(batch, got, want) + check_output_order(batch, got.rows)
    assert not diffs, "%s:\n%s" % (tag, "\n".join(diffs))
    assert np.array_equal(got.out_index, np.nonzero(got.out_flag)[0]), tag
    if fresh:
        sig = _signature(e)
        f_got, f_sig = _fresh(prm, batch, reference, events)
        assert sig == f_sig, "%s: counters %s, a fresh engine %s" % (tag, sig, f_sig)
        assert not diff_results(batch, f_got, want), tag
    return want


def check_depth(tag, e, batch, prm_tl, want, step, regions):
    """gce_depth_stats and gce_stats_payload_device + gce_stats_payload_read of the step vs oracle.depth_stats."""
    from gencore_amd import capi
    from oracle import oracle_py
    off, pre_d, post_d, pre_b, post_b = oracle_py.depth_stats(batch, want, prm_tl, step, regions)
    got = e.depth_stats(step, regions)
    for name, x, y in zip(("bin_off", "pre_depth", "post_depth", "pre_bed", "post_bed"), got, (off, pre_d, post_d, pre_b, post_b)):
        assert np.array_equal(x, y), "%s: depth_stats %s differs" % (tag, name)
    reg = np.asarray(regions, np.int32).reshape(-1, 3)
    t, a, z = (np.ascontiguousarray(reg[:, k]) for k in range(3))
    pp, lay = C.c_void_p(), capi.GcePayloadLayout()
    e._check(e.lib.gce_stats_payload_device(e._h, step, len(reg), t.ctypes.data, a.ctypes.data, z.ctypes.data, C.byref(pp), C.byref(lay)))
    host = np.zeros(int(lay.total_words), np.int64)
    e._check(e.lib.gce_stats_payload_read(e._h, pp, int(lay.total_words), host.ctypes.data))
    sw, nb, nr = capi.GCE_STATS_WORDS, int(lay.n_bins), int(lay.n_regions)
    expect = np.concatenate([want.pre.as_array(), want.post.as_array(), pre_d, post_d, pre_b, post_b]).astype(np.int64)
    assert int(lay.total_words) == 2 * sw + 2 * nb + 2 * nr and np.array_equal(host, expect), "%s: Stats payload differs" % tag


def run_host(e, batch, reference, events=None, cuts=None):
    """One stream through gce_submit (in the pieces `cuts`), gce_process, gce_drain."""
    from gencore_amd.shard import slice_batch
    if events is not None:
        e.set_flush_events(*events)
    _stage(e, reference)
    cuts = cuts or [0, batch.n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sub = slice_batch(batch, np.arange(lo, hi)) if (lo, hi) != (0, batch.n) else batch
        if batch.tick is not None and sub is not batch:
            sub.tick = np.ascontiguousarray(batch.tick[lo:hi], np.uint64)
        e.add_reads(sub)
    e.finish()
    return e.output(batch)


def _device_struct(batch, keep):
    """A gce_batch of device copies of a host batch (torch tensors kept in `keep`, 64 readable bytes behind every blob)."""
    import torch
    from gencore_amd.capi import GceBatch
    st = GceBatch()
    st.n_reads = batch.n
    for f in batch.FIELDS:
        a = getattr(batch, f)
        if a is None or (a.size == 0 and f in ("mi", "mi_off")):
            setattr(st, f, None)
            continue
        t = torch.from_numpy(np.concatenate([a.view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])).cuda()
        keep.append(t)
        setattr(st, f, t.data_ptr())
    st.qname_bytes, st.cigar_words, st.seq_bytes, st.qual_bytes = batch.qname.size, batch.cigar.size, batch.seq.size, batch.qual.size
    st.mi_bytes = 0 if batch.mi is None else batch.mi.size
    st.tick = None
    if batch.tick is not None:
        t = torch.from_numpy(np.ascontiguousarray(batch.tick, np.uint64).view(np.uint8)).cuda()
        keep.append(t)
        st.tick = t.data_ptr()
    return st


def run_device(e, batch, reference, pieces=1, events=None):
    """gce_submit_device: one zero-copy batch, or `pieces` batches appended into the engine's own copy (each freed when its call returns)."""
    from gencore_amd.shard import slice_batch
    if events is not None:
        e.set_flush_events(*events)
    _stage(e, reference)
    cuts = [batch.n * k // pieces for k in range(pieces + 1)]
    first = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sub = batch if pieces == 1 else slice_batch(batch, np.arange(lo, hi))
        if pieces > 1 and batch.tick is not None:
            sub.tick = np.ascontiguousarray(batch.tick[lo:hi], np.uint64)
        keep = []
        st = _device_struct(sub, keep)
        e._check(e.lib.gce_submit_device(e._h, C.byref(st)))
        if lo == 0:
            first = keep                                 # (the zero-copy batch lives until gce_process; later ones may go at once)
    e.finish()
    out = e.output(batch)
    del first
    return out


def run_reserved(e, batch, reference, reserve_reads, events=None):
    """gce_reserve (for `reserve_reads` reads and the blobs in proportion) + gce_submit_async in three batches."""
    from gencore_amd.shard import slice_batch
    if events is not None:
        e.set_flush_events(*events)
    _stage(e, reference)
    f = reserve_reads / max(batch.n, 1)
    e._check(e.lib.gce_reserve(e._h, int(reserve_reads), int(batch.qname.size * f), int(batch.cigar.size * f), int(batch.seq.size * f), int(batch.qual.size * f)))
    cuts = [0, batch.n // 4, (2 * batch.n) // 3, batch.n]
    keep = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sub = slice_batch(batch, np.arange(lo, hi))
        if batch.tick is not None:
            sub.tick = np.ascontiguousarray(batch.tick[lo:hi], np.uint64)
        keep.append(sub)
        st = sub.as_struct()
        t = C.c_int32(-1)
        e._check(e.lib.gce_submit_async(e._h, C.byref(st), C.byref(t)))
    e.finish()
    return e.output(batch)


def _raw_stream(batch, target_len):
    """The inflated BAM stream of a batch (header + records, pybam's encoder) and where its records begin."""
    text = "@HD\tVN:1.6\tSO:coordinate\n"
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(target_len))
    for k, ln in enumerate(target_len):
        nm = ("chr%d" % k).encode()
        head += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", int(ln))
    return head + b"".join(pybam.record_bytes(r) for r in _records(batch)), len(head)


def _raw_lib(lib):
    lib.gce_raw_begin.argtypes = [C.c_void_p, C.c_size_t]
    lib.gce_raw_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    lib.gce_raw_finish.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_int64)]
    lib.gce_raw_select_shard.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.gce_raw_build_output.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
    lib.gce_raw_read_output_async.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    return lib


def run_raw(e, batch, reference, target_len, shard=None):
    """gce_raw_begin / push (two pieces) / finish [/ gce_raw_select_shard(world, rank)] / gce_process: (drained rows, output record bytes)."""
    lib = _raw_lib(e.lib)
    stream, begin = _raw_stream(batch, target_len)
    _stage(e, reference)
    e._check(lib.gce_raw_begin(e._h, len(stream)))
    data = np.frombuffer(stream, np.uint8).copy()
    tk = C.c_int32()
    for lo, hi in ((0, len(data) // 2 + 7), (len(data) // 2 + 7, len(data))):
        e._check(lib.gce_raw_push(e._h, data[lo:].ctypes.data, hi - lo, C.byref(tk)))
        e._check(lib.gce_submit_wait(e._h, tk.value))
    n = C.c_int64()
    e._check(lib.gce_raw_finish(e._h, begin, len(target_len), C.byref(n)))
    assert n.value == batch.n
    if shard is not None:
        e._check(lib.gce_raw_select_shard(e._h, shard[0], shard[1], 0))
    e.finish()
    rows = e.rows()
    body, n_out = C.c_uint64(), C.c_int64()
    e._check(lib.gce_raw_build_output(e._h, C.byref(body), C.byref(n_out)))
    out = np.zeros(int(body.value), np.uint8)
    if body.value:
        e._check(lib.gce_raw_read_output_async(e._h, 0, out.ctypes.data, int(body.value), C.byref(tk)))
        e._check(lib.gce_submit_wait(e._h, tk.value))
    return rows, out.tobytes()


def _table(batch, rows):
    from gencore_amd.batch import table_from_rows
    r, pre, post = rows
    t = table_from_rows(batch, r, pre, post)
    t.out_index = np.sort(r["src"])
    return t


@functools.lru_cache(maxsize=None)
def _synth(name, n_pairs):
    from gencore_amd import synth
    d = synth.generate(name, n_pairs=n_pairs)
    return d.to_batch(), d.reference_host(), list(d.target_len), d.info


# ---------------------------------------------------------------------------------------------------------------------------- 1. sizes down and up
@pytest.mark.gpu
def test_sizes_down_and_up_on_one_engine(built):
    """cfg3 (30 k pairs), one pair, no read, a fuzz case, a cfg5 deep stream, cfg3 again -- one engine, the reference re-staged where the
    stream's contigs differ.  The table, cluster and vote buffers meet every size relation to the step before; k_vote_deep runs after k_vote."""
    from gencore_amd.batch import ReadBatch
    from gencore_amd.capi import default_params
    b3, ref3, tl3, info3 = _synth("cfg3", 30000)
    b5, ref5, tl5, _ = _synth("cfg5", 3000)
    tl = np.asarray(tl3, np.uint32)
    tl[0] = max(tl3[0], tl5[0])                                  # cfg5's one contig is longer than cfg3's first: one header for both
    prm = default_params(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix=info3["umi_prefix"], cluster_size_req=1)
    prm._keep = tl
    fz, _, fz_ref, _ = fuzzgen.make_case(930, n_mol=50, umi_mode="prefix", period=10000)
    fz_ref = list(fz_ref) + list(ref3[len(fz_ref):])
    ref5 = list(ref5) + list(ref3[1:])
    one = ReadBatch.from_records([_base_rec(qname="p:UMI_ACGT", pos=1000, mpos=1030), _base_rec(qname="p:UMI_ACGT", flag=147, pos=1030, mpos=1000, isize=-50)])
    empty = ReadBatch.from_records([])
    regions = [(0, 100000, 900000), (1, 0, 5000000), (3, 17, 40000)]
    e = _engine(prm)
    try:
        for k, (tag, batch, ref, depth) in enumerate((("cfg3", b3, ref3, 100000), ("one pair", one, ref3, None), ("empty", empty, ref3, 1000),
                                                       ("fuzz", fz, fz_ref, None), ("cfg5", b5, ref5, 50000), ("cfg3 again", b3, ref3, 250000))):
            got = run_host(e, batch, ref)
            want = check_step("step %d (%s)" % (k, tag), e, batch, prm, ref, got, fresh=batch.n > 0)
            if batch.n == 0:
                assert e.vote_counters()["groups"] == 0 and e.pairing_tiers()[2] == dict.fromkeys(e.PAIR_TIERS, 0)
            if depth:
                check_depth(tag, e, batch, tl, want, depth, regions)
            if tag == "cfg5":
                assert e.pairing_tiers()[2]["deep_lds"] > 0
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------- 2. colliding keys
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["A_then_B", "B_then_A"])
def test_colliding_cluster_keys_on_one_engine(built, order):
    """B has exactly A's cluster keys and fewer reads: a bucket that A's step left behind would let B's reads join A's cluster."""
    a, b, prm, ref = colliding_pair()
    seq = [("A", a), ("B", b)] if order == "A_then_B" else [("B", b), ("A", a)]
    e = _engine(prm)
    try:
        for tag, batch in seq + seq:
            check_step("%s %s" % (order, tag), e, batch, prm, ref, run_host(e, batch, ref))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------- 3. after every failure
@pytest.mark.gpu
def test_clean_stream_after_every_failure(built, capfd):
    """Every fatal status of the engine, then the colliding stream B with no gce_reset in between: B's table must be the oracle's.  Then the
    host-side refusals.  A failed gce_process and a second gce_process need no reset (the next submit starts a new stream); a refused
    gce_submit after gce_submit_device, and a tick / no-tick mix inside one stream, leave the batches accepted so far in the engine: the
    caller resets (include/gencore_amd.h, gce_reset)."""
    from gencore_amd.capi import GceError
    from gencore_amd.engine import Engine
    a, b, prm, ref = colliding_pair()
    e = _engine(prm)
    try:
        check_step("B first", e, b, prm, ref, run_host(e, b, ref), fresh=False)
        for name, status, recs, sref, window in error_streams(ref):
            batch = error_batch(recs)
            _stage(e, sref)
            if window is not None:
                nib, n = sref[0]
                e.set_reference_window(0, n, window[0], _ascii(nib, n)[window[0]:window[1]])
            e.add_reads(batch)
            with pytest.raises(GceError) as ei:
                e.finish()
            assert ei.value.status == status, name
            check_step("B after %s" % name, e, b, prm, ref, run_host(e, b, ref), fresh=False)
        # gce_process twice
        got = run_host(e, a, ref)
        with pytest.raises(GceError):
            e.finish()
        check_step("A before the second process", e, a, prm, ref, got, fresh=False)
        check_step("B after a second process", e, b, prm, ref, run_host(e, b, ref), fresh=False)
        # gce_submit after gce_submit_device: refused, and refused again until the caller resets
        keep = []
        e._check(e.lib.gce_submit_device(e._h, C.byref(_device_struct(a, keep))))
        for _ in range(2):
            with pytest.raises(GceError):
                e.add_reads(b)
        e.reset()
        check_step("B after submit / submit_device", e, b, prm, ref, run_host(e, b, ref))
        # ticks in one batch of a stream and not in the next: refused; reset
        from gencore_amd.shard import stream_context
        tick, _, _ = stream_context(a.core, 10000)
        a_t = a.copy()
        a_t.tick = np.ascontiguousarray(tick, np.uint64)
        e.add_reads(a_t)
        with pytest.raises(GceError):
            e.add_reads(b)
        e.reset()
        check_step("B after a tick mix", e, b, prm, ref, run_host(e, b, ref))
        # score constants the engine refuses, on a second engine of the process: the first is untouched
        over_bad = fuzzgen.make_params({}, [1000])
        over_bad.score_high = 252
        e2 = Engine(over_bad)
        try:
            with pytest.raises(GceError) as ei:
                e2.run(error_batch([_base_rec(qname="a:UMI_AAAA", pos=100, mpos=130)]))
            assert ei.value.status == -1
        finally:
            e2.close()
        check_step("B after a refused engine", e, b, prm, ref, run_host(e, b, ref))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------- 4. submit modes in turn
@pytest.mark.gpu
def test_submit_modes_in_turn_on_one_engine(built):
    """host (two batches), device zero copy, device (three batches: the engine's own copy), reserve + async with a reservation below and
    above the stream, the raw BAM path, host again -- MI tags on and off, ticks + flush events on and off.  (Regression: gce_reserve on an
    engine whose last stream was processed was refused as "gce_reserve after a submit"; it now starts a new stream as the submits do.)"""
    from gencore_amd.shard import stream_context
    from gencore_amd.engine import Engine
    mi, over, ref, contig_len = fuzzgen.make_case(940, n_mol=70, umi_mode="mi", period=10000)
    pre, _, _, _ = fuzzgen.make_case(940, n_mol=90, umi_mode="prefix", period=10000)       # (the same seed: the same contigs)
    over.update(umi_prefix="UMI", skip_low_complexity_cluster_threshold=1000)
    prm = fuzzgen.make_params(over, contig_len)

    def ticked(batch):
        t, et, ep = stream_context(batch.core, 10000)
        out = batch.copy()
        out.tick = np.ascontiguousarray(t, np.uint64)
        return out, (et, ep)
    mi_t, mi_ev = ticked(mi)
    pre_t, pre_ev = ticked(pre)
    e = _engine(prm)
    try:
        steps = [
            ("host, 2 batches, MI", mi, None, lambda bt, ev: run_host(e, bt, ref, ev, cuts=[0, bt.n // 2, bt.n])),
            ("device zero copy, ticks", pre_t, pre_ev, lambda bt, ev: run_device(e, bt, ref, 1, ev)),
            ("device 3 batches, MI", mi, None, lambda bt, ev: run_device(e, bt, ref, 3)),
            ("reserve below, ticks, MI", mi_t, mi_ev, lambda bt, ev: run_reserved(e, bt, ref, bt.n // 3, ev)),
            ("reserve above", pre, None, lambda bt, ev: run_reserved(e, bt, ref, 3 * bt.n)),
        ]
        for tag, batch, ev, fn in steps:
            check_step(tag, e, batch, prm, ref, fn(batch, ev), events=ev)
        # the raw path: the table of the oracle, the output records of a fresh engine
        rows, body = run_raw(e, mi, ref, contig_len)
        check_step("raw, MI", e, mi, prm, ref, _table(mi, rows))
        f = Engine(prm)
        try:
            _, f_body = run_raw(f, mi, ref, contig_len)
        finally:
            f.close()
        assert body == f_body and len(body) > 0
        check_step("host again", e, pre, prm, ref, run_host(e, pre, ref))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------- 5. reference changes
@pytest.mark.gpu
def test_reference_changes_between_streams(built):
    """Same contig length with other bases (gce_set_reference, then gce_set_reference_ascii), a window / the whole contig / another window,
    a contig removed (null pointer) and restored: each step's oracle gets the reference as staged at that step."""
    from oracle import oracle_py
    batch, prm, ref, contig_len = reference_case()
    base, alt, alt_nib = reference_variants(ref)
    n = ref[0][1]
    r_base, r_alt, r_none = list(ref), [(alt_nib, n)] + list(ref[1:]), [(None, 0)] + list(ref[1:])
    e = _engine(prm)
    try:
        _stage(e, ref)

        def step(tag, staged):
            e.add_reads(batch)
            e.finish()
            check_step(tag, e, batch, prm, staged, e.output(batch))
        step("base", r_base)
        e.set_reference(0, alt_nib, n)
        step("other bases, nibbles", r_alt)
        e.set_reference_ascii(0, base)
        step("base, ascii", r_base)
        e.set_reference_window(0, n, 0, alt[:3200])
        step("window [0, 3200) of the other bases", r_alt)
        e.set_reference_ascii(0, base)
        step("whole contig", r_base)
        ws = int(batch.core["pos"].min()) & ~1
        e.set_reference_window(0, n, ws, alt[ws:4000])
        step("window [%d, 4000) of the other bases" % ws, r_alt)
        assert e.lib.gce_set_reference(e._h, 0, None, 0) == 0
        step("contig removed", r_none)
        e.set_reference(0, ref[0][0], n)
        step("contig restored", r_base)
        e.set_reference_ascii(0, base + alt)                                     # a longer contig, never processed: its buffer replaces the first ...
        e.set_reference(0, alt_nib, n)                                           # ... and the same length as the step before comes back in it
        step("same length, new buffer", r_alt)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------- 6. bench's step loop
def _device_rows(lib, eng):
    """gce_result_device -> the table of emitted records on the host (hipMemcpy from the engine's device buffers)."""
    from gencore_amd import capi
    from gencore_amd.engine import _ROW_FIELDS
    r = capi.GceResult()
    assert lib.gce_result_device(eng, C.byref(r)) == 0
    hip = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])
            break
    n = int(r.n_out)

    def dev(ptr, count, dt):
        out = np.zeros(count, dt)
        if count:
            assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out
    rows = {k: dev(getattr(r, k), n, dt) for k, dt in _ROW_FIELDS}
    rows["seq"] = dev(r.seq, int(r.seq_bytes), np.uint8)
    rows["qual"] = dev(r.qual, int(r.qual_bytes), np.uint8)
    pre, post = capi.GceStats(), capi.GceStats()
    C.memmove(C.byref(pre), C.byref(r.pre), C.sizeof(capi.GceStats))
    C.memmove(C.byref(post), C.byref(r.post), C.sizeof(capi.GceStats))
    return rows, pre, post


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
@pytest.mark.parametrize("ticks", [False, True])
def test_bench_step_loop_checked_every_step(built, name, ticks):
    """bench.py's timed path on one engine: K = 4 steps of gce_submit_device (fresh seq / qual copies: the stream is mutated in place) ->
    gce_process -> gce_result_device, every step's table vs the oracle.  ticks: per-read ticks + flush events set ONCE before step 1 (bench's
    N > 1 path; the events outlive the implicit reset of every later submit).  The Stats payload every step, with other regions and another
    coverage step each time."""
    import torch
    from gencore_amd import capi, synth
    from gencore_amd.batch import table_from_rows
    from gencore_amd.shard import stream_context
    from oracle import oracle_py
    _dirty_device_memory()
    d = synth.generate(name, n_pairs=3000, device="cuda")
    t = d.t
    host = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    prm = capi.default_params(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix=d.info["umi_prefix"], cluster_size_req=d.info["supporting_reads"])
    events = tick_dev = None
    if ticks:
        tk, et, ep = stream_context(host.core, 10000)
        events = (et, ep)
        host.tick = np.ascontiguousarray(tk, np.uint64)
        tick_dev = torch.from_numpy(host.tick.view(np.int64).copy()).cuda()
    want = oracle_py.run(host, prm, d.reference_host(), events)
    assert want.status == 0
    lib = capi.load_library()
    eng = C.c_void_p()
    assert lib.gce_create(C.byref(prm), C.byref(eng)) == 0
    qname = torch.zeros(t["qname"].numel() + 64, dtype=t["qname"].dtype, device="cuda")
    qname[:t["qname"].numel()].copy_(t["qname"])
    try:
        for tid, (nib, ln) in enumerate(d.reference):
            assert lib.gce_set_reference(eng, tid, nib.data_ptr(), ln) == 0
        if events is not None:
            assert lib.gce_set_flush_events(eng, len(events[0]), events[0].ctypes.data, events[1].ctypes.data) == 0
        sig0 = None
        for k in range(4):
            seq = torch.zeros(t["seq"].numel() + 64, dtype=torch.uint8, device="cuda")
            qual = torch.zeros(t["qual"].numel() + 64, dtype=torch.uint8, device="cuda")
            seq[:t["seq"].numel()].copy_(t["seq"])
            qual[:t["qual"].numel()].copy_(t["qual"])
            b = capi.GceBatch()
            b.n_reads = d.n_reads
            b.core, b.qname_off, b.qname = t["core"].data_ptr(), t["qname_off"].data_ptr(), qname.data_ptr()
            b.cigar_off, b.cigar = t["cigar_off"].data_ptr(), t["cigar"].data_ptr()
            b.seq_off, b.seq, b.qual_off, b.qual = t["seq_off"].data_ptr(), seq.data_ptr(), t["qual_off"].data_ptr(), qual.data_ptr()
            b.nm, b.nm_type, b.mi_off, b.mi = t["nm"].data_ptr(), t["nm_type"].data_ptr(), None, None
            b.tick = tick_dev.data_ptr() if tick_dev is not None else None
            b.qname_bytes, b.cigar_words, b.seq_bytes, b.qual_bytes, b.mi_bytes = t["qname"].numel(), t["cigar"].numel(), t["seq"].numel(), t["qual"].numel(), 0
            assert lib.gce_submit_device(eng, C.byref(b)) == 0
            assert lib.gce_process(eng) == 0, lib.gce_last_error(eng)
            torch.cuda.synchronize()
            rows, pre, post = _device_rows(lib, eng)
            got = table_from_rows(host, rows, pre, post)
            diffs = diff_results(host, got, want) + check_output_order(host, rows)
            assert not diffs, "step %d:\n%s" % (k, "\n".join(diffs))
            v = (C.c_int64 * 4)()
            assert lib.gce_get_vote_counters(eng, v) == 0
            sig = v[3]
            assert sig0 is None or sig == sig0, "step %d: vote counters %s, step 0 %s" % (k, sig, sig0)
            sig0 = sig
            step = (10000, 1000000, 333, 50000)[k]
            regions = [(tid, 1000 * (k + 1), 1000 * (k + 1) + 100000 * (tid + 1)) for tid in range(min(len(tl), 2 + k))]
            off, pre_d, post_d, pre_b, post_b = oracle_py.depth_stats(host, want, tl, step, regions)
            reg = np.asarray(regions, np.int32)
            rt, rs, re_ = (np.ascontiguousarray(reg[:, j]) for j in range(3))
            pp, lay = C.c_void_p(), capi.GcePayloadLayout()
            assert lib.gce_stats_payload_device(eng, step, len(reg), rt.ctypes.data, rs.ctypes.data, re_.ctypes.data, C.byref(pp), C.byref(lay)) == 0
            hb = np.zeros(int(lay.total_words), np.int64)
            assert lib.gce_stats_payload_read(eng, pp, int(lay.total_words), hb.ctypes.data) == 0
            expect = np.concatenate([want.pre.as_array(), want.post.as_array(), pre_d, post_d, pre_b, post_b]).astype(np.int64)
            assert np.array_equal(hb, expect), "step %d: Stats payload differs" % k
    finally:
        lib.gce_destroy(eng)


# ---------------------------------------------------------------------------------------------------------------------------- 7. interleaved engines
@pytest.mark.gpu
def test_interleaved_engines_keep_their_state(built, capfd):
    """E1 with score constants that turn k_vote off, E2 with the defaults: E1, E2, E1, E2 in one process, other streams each time.  Their
    tables, counters and pinned StreamInfo stay apart; E1 says once that k_vote is off."""
    c1, over1, ref1, cl1 = fuzzgen.make_case(950, n_mol=60, umi_mode="prefix", period=10000, scores=(120, 6, 4, 2))
    c2, over2, ref2, cl2 = fuzzgen.make_case(951, n_mol=60, umi_mode="duplex", period=23)
    from gencore_amd.shard import slice_batch
    d1, d2 = slice_batch(c1, np.arange(c1.n // 3, c1.n)), slice_batch(c2, np.arange(0, (2 * c2.n) // 3))
    p1, p2 = fuzzgen.make_params(over1, cl1), fuzzgen.make_params(over2, cl2)
    e1, e2 = _engine(p1), _engine(p2)
    try:
        capfd.readouterr()
        for tag, e, prm, batch, ref in (("E1 a", e1, p1, c1, ref1), ("E2 a", e2, p2, c2, ref2), ("E1 b", e1, p1, d1, ref1), ("E2 b", e2, p2, d2, ref2),
                                        ("E1 a again", e1, p1, c1, ref1)):
            check_step(tag, e, batch, prm, ref, run_host(e, batch, ref))
        err = capfd.readouterr().err
        assert err.count("k_vote off for this engine") == 1 + 3, err          # E1 once, and each of the three fresh engines of E1's steps once
    finally:
        e1.close()
        e2.close()


# ---------------------------------------------------------------------------------------------------------------------------- 8. cuts and shards reused
@pytest.mark.gpu
def test_quit_after_contig_then_an_uncut_stream(built):
    """max_contig = 2: a stream cut at its first read of contig 2, then a stream of contigs 0 and 1 only (nothing cut), then the cut one again.
    The cut inserts fewer buckets than the stream holds."""
    from gencore_amd.shard import slice_batch
    cut, over, ref, contig_len = fuzzgen.make_case(960, n_mol=80, umi_mode="prefix", period=10000)
    assert (cut.core["tid"] == 2).any()
    over.update(max_contig=2)
    prm = fuzzgen.make_params(over, contig_len)
    uncut = slice_batch(cut, np.nonzero((cut.core["tid"] >= 0) & (cut.core["tid"] < 2))[0])
    e = _engine(prm)
    try:
        for tag, batch in (("cut", cut), ("uncut", uncut), ("cut again", cut)):
            check_step(tag, e, batch, prm, ref, run_host(e, batch, ref))
    finally:
        e.close()


@pytest.mark.gpu
def test_raw_shard_selection_then_the_whole_stream(built):
    """gce_raw_select_shard rank 0 of 2, then rank 1, then no selection, on one engine: every step's rows and output records those of a fresh
    engine doing the same, the two shards' records together the whole stream's, the last step the oracle's table."""
    from gencore_amd.engine import Engine
    batch, over, ref, contig_len = fuzzgen.make_case(970, n_mol=120, umi_mode="prefix", period=37)
    prm = fuzzgen.make_params(over, contig_len)
    e = _engine(prm)
    try:
        outs = []
        for shard in ((2, 0), (2, 1), None):
            rows, body = run_raw(e, batch, ref, contig_len, shard)
            f = Engine(prm)
            try:
                f_rows, f_body = run_raw(f, batch, ref, contig_len, shard)
            finally:
                f.close()
            for k in ("src", "kind", "qname_src", "nm_new", "fr", "rr", "mate"):
                assert np.array_equal(rows[0][k], f_rows[0][k]), (shard, k)
            assert bytes(rows[1]) == bytes(f_rows[1]) and bytes(rows[2]) == bytes(f_rows[2]) and body == f_body, shard
            outs.append((rows, body))
        check_step("whole stream", e, batch, prm, ref, _table(batch, outs[2][0]))
        assert len(outs[0][0][0]["src"]) + len(outs[1][0][0]["src"]) == len(outs[2][0][0]["src"]) and len(outs[0][1]) + len(outs[1][1]) == len(outs[2][1])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------------- CPU spec
def test_colliding_streams_share_every_cluster_key(built):
    """The property sequence 2 relies on: B has exactly A's cluster keys, fewer reads, none of A's names, and other UMIs."""
    a, b, prm, ref = colliding_pair()
    assert _cluster_keys(a) == _cluster_keys(b) and len(_cluster_keys(a)) > 20
    assert b.n < a.n and a.n < 1638 and b.n > 0                                      # (one bucket-table size for both: 4096 buckets)
    na = {a.qname_of(i) for i in range(a.n)}
    nb = {b.qname_of(i) for i in range(b.n)}
    assert not (na & nb)
    umi = lambda names: {q[q.find("UMI_") + 4:] for q in names if "UMI_" in q}
    assert not (umi(na) & umi(nb))


def test_error_streams_have_the_expected_oracle_status(built):
    """The statuses sequence 3 expects: the oracle's for every fatal path; 0 for the window stream (whole contigs in the oracle) -- and the
    colliding streams themselves pass."""
    from oracle import oracle_py
    a, b, prm, ref = colliding_pair()
    for name, status, recs, sref, window in error_streams(ref):
        want = oracle_py.run(error_batch(recs), prm, sref)
        assert want.status == (0 if window is not None else status), name
    assert oracle_py.run(a, prm, ref).status == 0 and oracle_py.run(b, prm, ref).status == 0


def test_reference_changes_change_the_output(built):
    """Every reference change of sequence 5 changes at least one emitted base or NM of the oracle's output: the other bases vs the base
    reference, and the contig removed vs present.  The windows cover every read of the stream."""
    from oracle import oracle_py
    batch, prm, ref, contig_len = reference_case()
    assert batch.n > 50
    base, alt, alt_nib = reference_variants(ref)
    n = ref[0][1]
    assert len(alt) == n and alt != base and oracle_py.pack_reference(base.decode()).tobytes() == np.asarray(ref[0][0], np.uint8).tobytes()
    w_base = oracle_py.run(batch, prm, ref)
    w_alt = oracle_py.run(batch, prm, [(alt_nib, n)] + list(ref[1:]))
    w_none = oracle_py.run(batch, prm, [(None, 0)] + list(ref[1:]))
    assert w_base.status == w_alt.status == w_none.status == 0
    for other in (w_alt, w_none):
        assert diff_results(batch, w_base, other), "the reference change does not change the output"
    ends = [int(batch.core["pos"][i]) + sum(int(w) >> 4 for w in batch.cigar[int(batch.cigar_off[i]):int(batch.cigar_off[i]) + int(batch.core["n_cigar"][i])] if int(w) & 15 in (0, 2, 3, 7, 8))
            for i in range(batch.n)]
    assert max(ends) <= 3200
