"""CPU side of the depth / BED edge tests (tests/depthcases.py): every case builds and its premise holds, and two references agree on it.

(a) oracle.depth_stats: the literal restatement of Stats::statDepth and Bed::statDepth (orc_stat_depth, orc_bed_depth; stats.cpp:56-83, bed.cpp:64-79).
    It is the arbiter for every case, here and in tests/test_depth_edges_gpu.py.
(b) `brute`: an independent count in numpy int64 that knows neither loop.  One per BASE: every counted read with start >= 0 that the drop rule keeps adds
    1 to the bin base // step for each base of [start, end); every well-formed region (start <= end) of a contig whose regions are sorted gets the number
    of bases [start, end) shares with it, summed over the counted reads of its contig; a region of a contig the header lacks gets 0.

(b) is defined on that subset only.  OUTSIDE lists what lies outside it and rests on (a) alone -- and on the hand-worked numbers below:
  * bins of a case that counts a read with pos < 0 (C truncation puts its first bases into bin 0, or drops the read at step 1): no base // step says that;
  * inverted regions (end < start): the reference adds a negative amount;
  * every region of a contig whose regions are not sorted: the early `break` skips regions that share bases with the read.
"""
import numpy as np
import pytest

import depthcases as dc
from gencore_amd.capi import CORE_DTYPE

# case -> what of it (b) does not define: "bins", or the file indices of regions
OUTSIDE = {
    "unclustered:step1": "bins",
    "unclustered:step7": "bins",
    "bed:inverted": (0, 1, 3, 4, 6),
    "bed:one_contig_unsorted": (3, 4, 5, 6),
    "bed:unsorted_break": (0, 1, 2, 3, 4),
}


def brute(core, sel, contig_len, step, regions):
    """(depth, depth defined, bed, bed defined per region) over the reads `sel` (stream indices)."""
    tl = np.asarray(contig_len, np.int64)
    off = dc.bin_offsets(tl, step)
    reg = np.asarray(regions, np.int64).reshape(-1, 3)
    sel = np.asarray(sel, np.int64)
    sel = sel[dc.counted(core, len(tl))[sel]]
    tid = core["tid"][sel].astype(np.int64)
    s = core["pos"][sel].astype(np.int64)
    ln = core["l_qseq"][sel].astype(np.int64)
    e = s + ln
    keep = (s >= 0) & (e // step <= tl[tid] // step)                                   # the bin of `end` is one of the contig's 1 + len / step
    first = np.cumsum(ln[keep]) - ln[keep]
    base = np.repeat(s[keep] - first, ln[keep]) + np.arange(int(ln[keep].sum()))       # every base of every kept read
    depth = np.bincount(np.repeat(off[tid[keep]], ln[keep]) + base // step, minlength=int(off[-1])).astype(np.int64)
    srt = dc.sorted_contigs(reg, len(tl))
    bed, defined = np.zeros(len(reg), np.int64), np.zeros(len(reg), bool)
    for k, (t, a, z) in enumerate(reg.tolist()):
        if not 0 <= t < len(tl):
            defined[k] = True                                                          # dropped by the loader (bed.cpp:165): never counted
        elif srt[t] and a <= z:
            on = tid == t
            bed[k] = np.clip(np.minimum(z, e[on]) - np.maximum(a, s[on]), 0, None).sum()
            defined[k] = True
    return depth, not (s < 0).any(), bed, defined


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case(oracle, name):
    """The premise holds (depthcases asserts it when it builds the case), and (a) == (b) wherever (b) is defined -- which is everywhere but OUTSIDE."""
    c = dc.get(name)
    assert c.premise and all(c.premise.values()), (name, c.premise, c.facts)
    table, (off, pre_d, post_d, pre_b, post_b) = dc.expect(name)
    assert np.array_equal(off, dc.bin_offsets(c.contig_len, c.step)) and len(pre_d) == off[-1] and len(pre_b) == len(c.regions)
    core = c.batch.core
    out = OUTSIDE.get(name, ())
    for tag, sel, want_d, want_b in (("pre", np.nonzero(core["tid"] >= 0)[0], pre_d, pre_b), ("post", np.nonzero(table.out_flag)[0], post_d, post_b)):
        depth, depth_ok, bed, bed_ok = brute(core, sel, c.contig_len, c.step, c.regions)
        if tag == "pre":                                                               # OUTSIDE is exact: nothing rests on the oracle alone without being listed
            assert depth_ok == (out != "bins"), (name, "bins outside the brute-force count's domain")
            assert tuple(np.nonzero(~bed_ok)[0].tolist()) == (() if out == "bins" else tuple(out)), (name, np.nonzero(~bed_ok)[0])
        if depth_ok:
            assert np.array_equal(depth, want_d), (name, tag, np.nonzero(depth != want_d)[0][:10])
        assert np.array_equal(bed[bed_ok], want_b[bed_ok]), (name, tag, np.nonzero(bed_ok & (bed != want_b))[0][:10])
    assert pre_d.sum() > 0 and 0 < post_d.sum() <= pre_d.sum() and len(sel) > 0


def test_catalogue_is_whole():
    assert set(n.split(":")[0] for n in dc.CASES) == set(dc.FAMILIES) and set(OUTSIDE) <= set(dc.CASES)
    for want in (["interior:len%d_step%d" % (L, s) for L in (1000, 5000) for s in (1, 100, 250)] + ["interior:len20_step1", "interior:len20_step7", "interior:one_step",
                 "interior:two_steps"] + ["table:size_%d" % n for n in (1, 255, 256, 2047, 2048, 2049, 4097)] + ["table:512_keys", "table:513_keys"]):
        assert want in dc.CASES, want


def test_slot_function_by_hand():
    """The mirrored slot function on numbers worked out with Python integers (no numpy wrap-around in the way)."""
    for k in (0, 1, 2, 511, 512, 12345, (1 << 31) + 7, (1 << 40) + 3):
        assert int(dc.slot_of([k])[0]) == ((k * 0x9E3779B97F4A7C15) % (1 << 64)) >> 55
    assert dc.most_in_one_window(range(100000)) > dc.DP_PROBES and dc.most_in_one_window([3, 4, 5]) == 1


def _one_read(pos, ln, tid=0):
    core = np.zeros(1, CORE_DTYPE)
    core["tid"], core["pos"], core["l_qseq"] = tid, pos, ln
    return core


def test_bin_shapes_by_hand(oracle):
    """One read of every bin shape at step 7 on a contig of 60 bases = 1 + 60 / 7 = 9 bins (stats.cpp:41-47), through (a), and through (b) where it is defined."""
    L = oracle.lib()
    d = np.zeros(9, np.int64)
    b = np.zeros(9, np.int64)

    def add(pos, ln, in_b=True):
        L.orc_stat_depth(d.ctypes.data, 9, 7, pos, ln)
        if in_b:
            depth, ok, _, _ = brute(_one_read(pos, ln), [0], (60,), 7, [])
            assert ok
            b[:] += depth
        return d.tolist()

    assert add(21, 5) == [0, 0, 0, 5, 0, 0, 0, 0, 0]             # [21, 26): inside bin 3, + len
    assert add(12, 20) == [0, 2, 7, 12, 4, 0, 0, 0, 0]           # [12, 32): 14 - 12 = 2 to bin 1, bins 2 and 3 whole, 32 - 28 = 4 to bin 4
    assert add(14, 7) == [0, 2, 14, 12, 4, 0, 0, 0, 0]           # one step on a multiple: [14, 21) -> 7 to bin 2, 21 - 21 = 0 to bin 3
    assert add(15, 7) == [0, 2, 20, 13, 4, 0, 0, 0, 0]           # one step off it: 6 to bin 2, 1 to bin 3
    assert add(28, 14) == [0, 2, 20, 13, 11, 7, 0, 0, 0]         # two steps on a multiple: 7 to bin 4, bin 5 whole, 0 to bin 6
    assert add(36, 20) == [0, 2, 20, 13, 11, 13, 7, 7, 0]        # [36, 56): 56 / 7 = 8 is the last bin -> kept; 6 to bin 5, bins 6, 7 whole, 0 to bin 8
    assert add(40, 20) == [0, 2, 20, 13, 11, 15, 14, 14, 4]      # [40, 60): 2 to bin 5, bins 6, 7 whole, 60 - 56 = 4 to bin 8
    assert add(43, 20) == [0, 2, 20, 13, 11, 15, 14, 14, 4]      # [43, 63): 63 / 7 = 9 is no bin -> the whole read is dropped (stats.cpp:68-69)
    assert add(55, 1) == [0, 2, 20, 13, 11, 15, 14, 15, 4]       # [55, 56): one base, lp 7 != rp 8: 56 - 55 = 1 to bin 7, 0 to bin 8
    assert b.tolist() == d.tolist()
    # pos = -1 on a contig (stats.cpp:118-119 counts it): -1 / 7 = 0 in C, so bin 0 gets (0 + 1) * 7 - (-1) = 8, bin 1 a whole step, bin 2 19 - 14 = 5
    before = d.copy()
    assert (np.asarray(add(-1, 20, in_b=False)) - before).tolist() == [8, 7, 5, 0, 0, 0, 0, 0, 0]
    assert brute(_one_read(-1, 20), [0], (60,), 7, [])[1] is False
    # ... and at step 1 it is bin -1: dropped
    d1 = np.zeros(61, np.int64)
    L.orc_stat_depth(d1.ctypes.data, 61, 1, -1, 20)
    assert not d1.any()
    L.orc_stat_depth(d1.ctypes.data, 61, 1, 3, 4)                # step 1: one per base, and a 0 to the bin of `end`
    assert d1[:9].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0]


def test_region_shapes_by_hand(oracle):
    """The read [100, 120) over a sorted list of every region shape (bed.cpp:70-78)."""
    L = oracle.lib()
    regs = [(90, 100),      # touches the read's start: end 100 < start 100 is false -> min(100, 120) - max(90, 100) = 0
            (105, 110),     # inside: 5
            (105, 200),     # the same start: 120 - 105 = 15
            (110, 110),     # empty: 0
            (115, 105),     # inverted: min(105, 120) - max(115, 100) = -10
            (118, 90),      # inverted, end 90 < start 100: skipped
            (120, 130),     # touches the read's end: start 120 > end 120 is false -> 120 - 120 = 0
            (121, 300)]     # start 121 > end 120: break
    rs, re_ = np.asarray([r[0] for r in regs], np.int32), np.asarray([r[1] for r in regs], np.int32)
    cnt = np.zeros(len(regs), np.int64)
    L.orc_bed_depth(rs.ctypes.data, re_.ctypes.data, cnt.ctypes.data, len(regs), 100, 20)
    assert cnt.tolist() == [0, 5, 15, 0, -10, 0, 0, 0]
    _, _, bed, ok = brute(_one_read(100, 20), [0], (500,), 7, [(0, a, z) for a, z in regs])
    assert ok.tolist() == [True, True, True, True, False, False, True, True] and bed[ok].tolist() == cnt[ok].tolist()
    L.orc_bed_depth(rs.ctypes.data, re_.ctypes.data, cnt.ctypes.data, len(regs), -1, 20)          # [-1, 19) meets nothing
    assert cnt.tolist() == [0, 5, 15, 0, -10, 0, 0, 0]
