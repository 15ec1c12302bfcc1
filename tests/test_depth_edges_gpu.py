"""Depth bins and BED region counts (gce_depth.hpp: k_depth; engine.hip: gce_stats_payload_device, k_payload_finish) on the streams of tests/depthcases.py,
engine against oracle.depth_stats on oracle.run's table: bin_off, pre and post bins, pre and post region counts, all exactly equal.  Then the same numbers
through repeated calls on one processed engine, through the Stats payload, and through the file runners (one engine, three shards on device 0).

Measured on the MI355X: the module's 50 tests take 2.6 s in all, oracle runs included; the slowest are interior:len1000_step1 0.18 s (it builds the
1000-base stream), the file runners on three shards 0.12 - 0.14 s and table:window_regions (6100 regions) 0.13 s.

That the cases bite was tried with three edits of k_depth that change amounts and no address: without the interior-bin loop 27 of the 50 tests fail, without
the global atomicAdd behind DepthAgg::add's eight probes 13 (table:512_keys, 513_keys, 30000_keys, window_bins, window_regions and the step-1 streams),
with `continue` for the unsorted path's `break` 5 (bed:one_contig_unsorted, bed:unsorted_break, the repeated calls, the file runners on contig_end:step50).
The `rp >= nb` guard was not edited on a GPU: without it the dropped reads of the contig_end cases would land in the next contig's first bin, in the post
block or, behind the last post bin, in the region counts -- all compared here."""
import ctypes as C

import numpy as np
import pytest

import depthcases as dc

pytestmark = pytest.mark.gpu

NAMES = ("bin_off", "pre_depth", "post_depth", "pre_bed", "post_bed")


def processed_engine(case):
    from gencore_amd.engine import Engine
    e = Engine(case.params())
    try:
        for tid, (nib, ln) in enumerate(case.reference or []):
            if nib is not None:
                e.set_reference(tid, nib, ln)
        e.add_reads(case.batch)
        e.finish()
    except BaseException:
        e.close()
        raise
    return e


def check(tag, got, want):
    """Exact equality of the five arrays; a failure names the array and the first places that differ."""
    for name, x, y in zip(NAMES, got, want):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == np.int64 and len(x) == len(y), (tag, name, x.dtype, len(x), len(y))
        bad = np.nonzero(x != y)[0]
        assert not len(bad), "%s: %s differs in %d places, first at %s: engine %s, oracle %s" % (tag, name, len(bad), bad[:8], x[bad[:8]], y[bad[:8]])


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case(built, oracle, name):
    case = dc.get(name)
    _, want = dc.expect(name)
    e = processed_engine(case)
    try:
        got = e.depth_stats(case.step, case.regions)
    finally:
        e.close()
    check(name, got, want)


def test_repeated_calls_on_one_engine(built, oracle):
    """A coarse step with ten regions, then step 1 with 600 regions (larger dp_* buffers; contigs 0 and 2 sorted, contig 1 as drawn: the unsorted path; a
    sixth of them on contigs the header lacks), then the first again -- and a coarser one still: what a call leaves in the buffers must not show in the next."""
    a = dc.get("bed:interleaved")
    table, want_a = dc.expect(a.name)
    rng = np.random.RandomState(11)
    st = rng.randint(0, 900, 600)
    fine = [(int(t), int(s), int(s) + int(w)) for t, s, w in zip(rng.randint(-1, 5, 600), st, rng.randint(0, 300, 600))]
    fine.sort(key=lambda r: (0, r[1]) if r[0] in (0, 2) else (1, 0))                      # (stable: the other contigs keep the order drawn)
    want_fine = oracle.depth_stats(a.batch, table, a.contig_len, 1, fine)
    want_coarse = oracle.depth_stats(a.batch, table, a.contig_len, 5000, a.regions[:3])
    e = processed_engine(a)
    try:
        first = e.depth_stats(a.step, a.regions)
        second = e.depth_stats(1, fine)
        third = e.depth_stats(a.step, a.regions)
        fourth = e.depth_stats(5000, a.regions[:3])
        fifth = e.depth_stats(a.step, a.regions)
    finally:
        e.close()
    check("first", first, want_a)
    check("fine", second, want_fine)
    check("coarse", fourth, want_coarse)
    for tag, got in (("third", third), ("fifth", fifth)):
        check(tag, got, want_a)
        for x, y in zip(got, first):
            assert np.array_equal(x, y), tag
    assert len(second[1]) > 50 * len(first[1]) and dc.sorted_contigs(fine, 4).tolist() == [True, False, True, False]
    assert int((want_fine[3] > 0).sum()) > 50 and int((want_fine[4] > 0).sum()) > 50 and want_coarse[3].sum() > 0


THREE = ("contig_end:step50", "table:513_keys", "bed:absent_mixed")


@pytest.mark.parametrize("name", THREE)
def test_payload(built, oracle, name):
    """gce_stats_payload_device + gce_stats_payload_read: [pre Stats][post Stats][pre bins][post bins][pre regions][post regions] in one buffer."""
    from gencore_amd import capi
    case = dc.get(name)
    table, (off, pre_d, post_d, pre_b, post_b) = dc.expect(name)
    reg = np.asarray(case.regions, np.int32).reshape(-1, 3)
    t, a, z = (np.ascontiguousarray(reg[:, k]) for k in range(3))
    e = processed_engine(case)
    try:
        pp, lay = C.c_void_p(), capi.GcePayloadLayout()
        e._check(e.lib.gce_stats_payload_device(e._h, case.step, len(reg), t.ctypes.data, a.ctypes.data, z.ctypes.data, C.byref(pp), C.byref(lay)))
        host = np.full(int(lay.total_words), -1, np.int64)
        e._check(e.lib.gce_stats_payload_read(e._h, pp, int(lay.total_words), host.ctypes.data))
        lay_off = np.ctypeslib.as_array(lay.bin_off, shape=(int(lay.n_targets) + 1,)).copy()
    finally:
        e.close()
    sw = capi.GCE_STATS_WORDS
    assert (int(lay.stats_words), int(lay.n_targets), int(lay.n_bins), int(lay.n_regions)) == (2 * sw, len(case.contig_len), len(pre_d), len(reg))
    assert int(lay.total_words) == 2 * sw + 2 * len(pre_d) + 2 * len(reg) and np.array_equal(lay_off, off)
    expect = np.concatenate([table.pre.as_array(), table.post.as_array(), pre_d, post_d, pre_b, post_b]).astype(np.int64)
    assert np.array_equal(host, expect), (name, np.nonzero(host != expect)[0][:8])


def interleave(regions):
    """The regions dealt round over their contigs: the file changes contig on nearly every line, the order inside a contig stays."""
    by = {}
    for r in regions:
        by.setdefault(r[0], []).append(r)
    out = []
    while any(by.values()):
        for t in list(by):
            if by[t]:
                out.append(by[t].pop(0))
    return out


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("name", THREE)
def test_file_runners(built, oracle, tmp_path, name, shards):
    """The stream as a BAM file through gce_run_bam_depth, with a BED file that interleaves contigs (and names some the header lacks): one engine, and three
    engines on device 0 whose payloads are summed.  The sums are the whole stream's."""
    import pybam
    from gencore_amd.bamio import run_bam_depth
    from gencore_amd.capi import default_params
    from test_bamio import records_of
    case = dc.get(name)
    nt = len(case.contig_len)
    regions = interleave(list(case.regions) + [(t, 3, 33) for t in range(nt)] + [(t, 40, 45) for t in range(nt)])      # (two more lines on every contig: every file interleaves)
    table = dc.table_of(name)
    off, pre_d, post_d, pre_b, post_b = oracle.depth_stats(case.batch, table, case.contig_len, case.step, regions)
    src, dst, bed = (str(tmp_path / x) for x in ("in.bam", "out.bam", "panel.bed"))
    pybam.write_bam(src, records_of(case.batch), [("chr%d" % (i + 1), int(l)) for i, l in enumerate(case.contig_len)])
    with open(bed, "w") as f:
        for t, a, z in regions:
            f.write("%s\t%d\t%d\tr\n" % ("chr%d" % (t + 1) if 0 <= t < nt else "absent%d" % t, a, z))
    prm = default_params(umi_prefix="", flush_period=100, skip_low_complexity_cluster_threshold=1 << 20)
    run, got = run_bam_depth(src, dst, prm, [0] * shards, case.step, bed=bed, threads=4)
    assert got["regions"] == [(t if 0 <= t < nt else -1, a, z) for t, a, z in regions]
    assert int((np.diff([r[0] for r in regions]) != 0).sum()) >= nt
    check("%s x%d" % (name, shards), (got["bin_off"], got["pre_depth"], got["post_depth"], got["pre_bed"], got["post_bed"]), (off, pre_d, post_d, pre_b, post_b))
    assert got["pre"] == bytes(table.pre) and got["post"] == bytes(table.post) and got["pre"] == bytes(run.pre) and got["post"] == bytes(run.post)
    assert got["payload_bytes"] == 8 * (2 * 114 + 2 * len(pre_d) + 2 * len(regions))
