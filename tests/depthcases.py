"""Streams for the edges of the depth and BED statistics (gce_depth.hpp: k_depth; engine.hip: gce_stats_payload_device, k_payload_finish).  CPU only.

A case is a named stream with its contig lengths, a coverage step, a region list in BED FILE ORDER [(tid, start, end)] and a PREMISE: facts about
the input, computed here in plain numpy and asserted when the case is built, that say why the case is in the catalogue (how many bins a read
spans, which reads end in the bin behind their contig's last one, how many distinct keys a block of the pre pass sends to the aggregation table,
which regions share a probe window).  Nothing here asks the engine; `expect` asks the oracle, once per case.

What is counted (stats.cpp:56-83, 101-121, bed.cpp:64-79, gencore.cpp:110, 222): the pre pass counts every input read with tid >= 0 -- secondary,
supplementary and mate-unmapped reads and a read with pos = -1 included -- the post pass every emitted record.  A read adds its l_qseq bases from
`pos` on: to the bins start / step .. end / step of its contig (C division; the read is dropped whole when end / step is not a bin of the contig),
and to every region the literal loop of Bed::statDepth reaches.

The streams come from the existing builders: clustercases (reads of 20 bases: reads, pairs, dense, junk, unmapped_read, build) and lencases (the
"plain" family: 45 pairs of 1000 or 5000 bases).

MIRRORED FROM THE KERNEL (gce_depth.hpp) -- these must move with it: DP_T x DP_RPT = 2048 reads per block of a pass (the pre pass: stream reads
[2048 b, 2048 b + 2048)), DP_SLOTS = 512 slots per table, 8 probes from slot ((key x 0x9E3779B97F4A7C15) >> 55) & 511, a bin's key is its index
in the concatenated bins, a region's key its index among the regions of the header's contigs GROUPED BY CONTIG (file order inside a contig).
Only premises use them: what the engine must give is the oracle's business.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import clustercases as cc
import lencases
from gencore_amd import shard
from gencore_amd.batch import ReadBatch
from gencore_amd.capi import default_params

DP_BLOCK = 256 * 8                          # DP_T * DP_RPT
DP_SLOTS = 512
DP_PROBES = 8
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
RL = cc.READ_LEN


def slot_of(keys):
    """Home slot of DepthAgg::add."""
    with np.errstate(over="ignore"):
        return ((np.asarray(keys, np.int64).astype(np.uint64) * _GOLDEN) >> np.uint64(55)).astype(np.int64) & (DP_SLOTS - 1)


# ------------------------------------------------------------------------------------------------------------ facts about a stream
def bin_offsets(contig_len, step):
    return np.concatenate([[0], np.cumsum(1 + np.asarray(contig_len, np.int64) // step)]).astype(np.int64)


def counted(core, n_targets):
    """Reads the pre pass counts: on a contig of the header."""
    return (core["tid"] >= 0) & (core["tid"] < n_targets)


def spans(core, contig_len, step):
    """Per read (start, end, lp, rp, nb, kept): C division, and the drop rule of stats.cpp:68-69.  nb = 0 for a read that is not counted."""
    tl = np.asarray(contig_len, np.int64)
    ok = counted(core, len(tl))
    start = core["pos"].astype(np.int64)
    end = start + core["l_qseq"].astype(np.int64)
    trunc = lambda a: np.where(a >= 0, a // step, -((-a) // step))
    lp, rp = trunc(start), trunc(end)
    nb = np.where(ok, 1 + tl[np.clip(core["tid"], 0, max(len(tl) - 1, 0))] // step if len(tl) else 0, 0)
    kept = ok & (rp < nb) & (lp >= 0)
    return start, end, lp, rp, nb, kept


def bin_keys(core, contig_len, step, sel):
    """Distinct bin keys the reads `sel` (stream indices) send to the table."""
    start, end, lp, rp, nb, kept = spans(core, contig_len, step)
    off = bin_offsets(contig_len, step)
    out = set()
    for i in np.nonzero(kept[sel])[0] + (sel.start or 0):
        b0 = int(off[core["tid"][i]])
        out.update(range(b0 + int(lp[i]), b0 + int(rp[i]) + 1))
    return out


def grouped(regions, n_targets):
    """(file index of every region of a contig of the header, grouped by contig in file order; first grouped index per contig)."""
    reg = np.asarray(regions, np.int64).reshape(-1, 3)
    present = np.nonzero((reg[:, 0] >= 0) & (reg[:, 0] < n_targets))[0]
    order = present[np.argsort(reg[present, 0], kind="stable")]
    first = np.searchsorted(reg[order, 0], np.arange(n_targets + 1))
    return order, first


def sorted_contigs(regions, n_targets):
    """Per contig: its regions' starts never fall in file order (the engine's sorted path; bed.cpp's `break` then only ends the scan)."""
    reg = np.asarray(regions, np.int64).reshape(-1, 3)
    return np.asarray([bool((np.diff(reg[reg[:, 0] == t, 1]) >= 0).all()) for t in range(n_targets)], bool)


def region_keys(core, contig_len, regions, sel):
    """Distinct region keys (grouped indices) the reads `sel` add to: the literal loop of bed.cpp:70-78."""
    reg = np.asarray(regions, np.int64).reshape(-1, 3)
    order, first = grouped(regions, len(contig_len))
    ok = counted(core, len(contig_len))
    out = set()
    for i in np.nonzero(ok[sel])[0] + (sel.start or 0):
        t, s = int(core["tid"][i]), int(core["pos"][i])
        e = s + int(core["l_qseq"][i])
        for g in range(int(first[t]), int(first[t + 1])):
            ps, pe = int(reg[order[g], 1]), int(reg[order[g], 2])
            if pe < s:
                continue
            if ps > e:
                break
            out.add(g)
    return out


def block(b):
    return slice(b * DP_BLOCK, (b + 1) * DP_BLOCK)


def most_in_one_window(keys):
    """The largest number of keys with one home slot: with more than DP_PROBES of them, one at least finds its eight slots taken whatever the order."""
    k = np.asarray(sorted(keys), np.int64)
    return int(np.bincount(slot_of(k), minlength=DP_SLOTS).max()) if len(k) else 0


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    batch: ReadBatch
    contig_len: tuple
    step: int
    regions: list
    premise: dict = field(default_factory=dict)              # name -> bool, all must hold
    facts: dict = field(default_factory=dict)                # numbers behind the premise, for the reader of a failure
    reference: list = None                                   # lencases streams bring their contigs
    prm: object = None                                       # ... and their parameters
    stream: str = None                                       # cases of one `stream` share a batch (and the oracle's table)

    def params(self):
        if self.prm is not None:
            return self.prm
        tl = np.asarray(self.contig_len, np.uint32)
        p = default_params(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix="", flush_period=100, skip_low_complexity_cluster_threshold=1 << 20)
        p._keep = tl
        return p


CASES = {}


def _register(name, fn):
    assert name not in CASES, name

    @functools.lru_cache(maxsize=None)
    def make():
        c = fn()
        assert c.name == name and c.premise, name
        bad = [k for k, v in c.premise.items() if not v]
        assert not bad, (name, bad, c.facts)                 # the premise is asserted when the case is built
        assert c.batch.n <= 10500, (name, c.batch.n)
        return c
    CASES[name] = make


def get(name):
    return CASES[name]()


def family(prefix):
    return [n for n in CASES if n.startswith(prefix + ":")]


_TABLES = {}


def table_of(name):
    """The oracle's table of a case's stream: one run for all the cases that share the stream."""
    from oracle import oracle_py
    c = get(name)
    if c.stream not in _TABLES:
        t = oracle_py.run(c.batch, c.params(), c.reference)
        assert t.status == 0, (name, t.status, t.message)
        _TABLES[c.stream] = t
    return _TABLES[c.stream]


@functools.lru_cache(maxsize=None)
def expect(name):
    """(table, (bin_off, pre_depth, post_depth, pre_bed, post_bed)) of oracle.depth_stats: computed once, shared, never changed."""
    from oracle import oracle_py
    c = get(name)
    t = table_of(name)
    want = oracle_py.depth_stats(c.batch, t, c.contig_len, c.step, c.regions)
    for a in want:
        a.setflags(write=False)
    return t, want


def single_pairs(cid0, tid, left, gap=10):
    """One pair per entry of `left`: forward read at left, reverse read at left + gap."""
    left = np.asarray(left, np.int64)
    return cc.pairs(cid0 + np.arange(len(left)), 0, tid, left, gap + RL, left + gap)


# ---- Interior bins
@functools.lru_cache(maxsize=None)
def _long_stream(L):
    st = lencases.family_stream("plain", L)
    batch, prm, ref = st.build()
    return batch, prm, ref, tuple(int(x) for x in prm._keep)


def _span_facts(core, contig_len, step):
    start, end, lp, rp, nb, kept = spans(core, contig_len, step)
    d = (rp - lp)[kept]
    right0 = kept & (rp > lp) & (end == rp * step)
    return dict(max_span=int(d.max()) if len(d) else -1, kept=int(kept.sum()), right_amount_0=int(right0.sum()),
                aligned=int((kept & (start % step == 0)).sum()), unaligned=int((kept & (start % step != 0)).sum()))


def _interior_long(L, step):
    batch, prm, ref, tl = _long_stream(L)
    n0 = tl[0]
    regions = [(0, 0, n0), (0, 50, 50 + L), (0, 50 + L // 2, 60 + L // 2), (0, n0 - 30, n0 + 500), (1, 0, 10)]
    f = _span_facts(batch.core, tl, step)
    f["reads"] = batch.n
    prem = dict(interior_bins=f["max_span"] >= 2, span_is_read_length=f["max_span"] in (L // step, L // step + 1), handful_of_groups=batch.n == 90,
                all_kept=f["kept"] == batch.n)
    return Case("interior:len%d_step%d" % (L, step), batch, tl, step, regions, prem, f, reference=ref, prm=prm, stream="long%d" % L)


for _L in (1000, 5000):
    for _s in (1, 100, 250):
        _register("interior:len%d_step%d" % (_L, _s), functools.partial(_interior_long, _L, _s))

SHORT_CONTIGS = (3000, 2000, 2500, 1000)


@functools.lru_cache(maxsize=None)
def _short_stream():
    """Small clusters on contigs 0, 1 and 2 of four (contig 3 holds no read), a position apart; about 3000 reads in two blocks of the pre pass."""
    return cc.build([cc.dense(1600, 0, 100), cc.dense(900, 1000, 40, tid=1), cc.dense(500, 2000, 700, tid=2)])


SHORT_REGIONS = [(0, 90, 200), (0, 150, 150), (0, 300, 480), (1, 0, 45), (1, 60, 61), (2, 700, 900), (3, 10, 500)]


def _interior_short(step):
    b = _short_stream()
    f = _span_facts(b.core, SHORT_CONTIGS, step)
    prem = dict(interior_bins=f["max_span"] >= 2, all_kept=f["kept"] == b.n, two_blocks=-(-b.n // DP_BLOCK) == 2)
    return Case("interior:len20_step%d" % step, b, SHORT_CONTIGS, step, SHORT_REGIONS, prem, f, stream="short")


for _s in (1, 7):
    _register("interior:len20_step%d" % _s, functools.partial(_interior_short, _s))


def _interior_exact(name, step, want_span):
    """Reads of exactly one step (step 20) or two (step 10): on a multiple of the step -- left amount one whole step, right amount 0 -- and off it."""
    k = np.arange(60)
    b = cc.build([cc.pairs(k, 0, 0, 40 * k, 2 * RL, 40 * k + RL),                     # both mates on multiples of 20
                  cc.pairs(100 + k, 0, 0, 3000 + 40 * k + 5, 2 * RL, 3000 + 40 * k + 5 + RL + 2)])
    contigs = (6000,)
    f = _span_facts(b.core, contigs, step)
    prem = dict(read_is_whole_steps=RL == want_span * step, span=f["max_span"] == want_span, aligned_reads=f["aligned"] == 120, unaligned_reads=f["unaligned"] == 120,
                right_amount_0=f["right_amount_0"] == 120, interior=(want_span >= 2) == (f["max_span"] >= 2))
    return Case(name, b, contigs, step, [(0, 0, 20), (0, 20, 40), (0, 3000, 3005)], prem, f, stream="exact")


_register("interior:one_step", functools.partial(_interior_exact, "interior:one_step", 20, 1))
_register("interior:two_steps", functools.partial(_interior_exact, "interior:two_steps", 10, 2))


# ---- Contig end
def end_contigs(step):
    """k x step, 0, less than the step, k x step - 1, k x step + 1, k x step: the first, four middle contigs and the last."""
    return (4 * step, 0, step // 2, 5 * step - 1, 6 * step + 1, 3 * step)


@functools.lru_cache(maxsize=None)
def _end_stream(step):
    """On every contig pairs from position 0 to two bins behind the last one, two bases apart (reads may lie behind the end of their contig: the
    header's length bounds the bins, not the reads)."""
    parts = []
    for t, ln in enumerate(end_contigs(step)):
        nb = 1 + ln // step
        parts.append(single_pairs(1000 * t, t, np.arange(0, (nb + 2) * step, 2)))
    return cc.build(parts)


def _end_case(step):
    contigs = end_contigs(step)
    b = _end_stream(step)
    core = b.core
    start, end, lp, rp, nb, kept = spans(core, contigs, step)
    regions = []
    for t, ln in enumerate(contigs):                                                   # a region across the end of every contig: the dropped reads still count there
        n = 1 + ln // step
        regions += [(t, 0, 10), (t, max(ln - 5, 0), (n + 1) * step)]
    f = dict(reads=b.n)
    prem = dict(lengths=contigs[0] % step == 0 and contigs[1] == 0 and 0 < contigs[2] < step and contigs[3] % step == step - 1 and contigs[4] % step == 1 and contigs[5] % step == 0)
    for t in range(len(contigs)):
        on = core["tid"] == t
        last, behind = on & (rp == nb - 1), on & (rp == nb)
        f["contig%d" % t] = dict(in_last_bin=int(last.sum()), in_bin_behind=int(behind.sum()), adds_0_to_last=int((last & (lp < rp) & (end == rp * step)).sum()))
        rs, re_ = regions[2 * t + 1][1], regions[2 * t + 1][2]
        if RL // step > int(nb[on][0]):                                                # a contig of fewer bins than a read spans: the shortest `end` lies behind them all
            prem["contig%d_every_read_dropped" % t] = not kept[on].any() and bool((on & (end > rs) & (start < re_)).any())
            continue
        prem["contig%d_last_bin_kept" % t] = bool(last.any()) and bool(kept[last].all())
        prem["contig%d_bin_behind_dropped" % t] = bool(behind.any()) and not kept[behind].any()
        prem["contig%d_dropped_reads_meet_a_region" % t] = bool((behind & (end > rs) & (start < re_)).any())
    prem["adds_0_to_a_last_bin"] = any(f["contig%d" % t]["adds_0_to_last"] > 0 for t in range(len(contigs)))
    return Case("contig_end:step%d" % step, b, contigs, step, regions, prem, f, stream="end%d" % step)


for _s in (50, 7):
    _register("contig_end:step%d" % _s, functools.partial(_end_case, _s))


# ---- Not clustered, still counted
@functools.lru_cache(maxsize=None)
def _unclustered_stream():
    """Small clusters between runs of secondary / supplementary / mate-unmapped reads; a read without a contig in mid-stream (what is clustered behind it and
    taken by no later walk is never emitted), a read at pos = -1 of contig 1 (in front of that contig's reads: the stream stays sorted) and two reads
    without a contig at the end."""
    parts = [cc.dense(700, 0, 100), cc.junk(300, 90000000, 150), cc.dense(500, 1000, 600), cc.junk(90, 90001000, 620), cc.dense(600, 2000, 50, tid=1),
             cc.junk(120, 90002000, 60, tid=1)]
    r = cc.sorted_reads(parts)
    first1 = int(np.argmax(r["tid"] == 1))
    n = len(r["pos"])
    return cc.build(parts, inserts=[(400, cc.unmapped_read("tid<0")), (first1 + 1, cc.unmapped_read("pos<0") | dict(tid=1)), (n + 2, cc.unmapped_read("tid<0")),
                                    (n + 3, cc.unmapped_read("tid<0"))])


def _unclustered(step):
    contigs = (1500, 900)
    b = _unclustered_stream()
    core = b.core
    cm = shard.clustered_mask(core)
    pre = counted(core, 2)
    neg = pre & (core["pos"] < 0)
    start, end, lp, rp, nb, kept = spans(core, contigs, step)
    f = dict(reads=b.n, counted_by_pre=int(pre.sum()), clustered=int(cm.sum()), counted_not_clustered=int((pre & ~cm).sum()), no_contig=int((core["tid"] < 0).sum()),
             negative_pos=int(neg.sum()), negative_pos_kept=int((neg & kept).sum()))
    prem = dict(junk_counted=f["counted_not_clustered"] == 300 + 90 + 120 + 1, counted=f["counted_by_pre"] == b.n - 3, no_contig_mid_stream=int(core["tid"][400]) == -1,
                no_contig_at_end=bool((core["tid"][-2:] == -1).all()), negative_pos_on_contig=f["negative_pos"] == 1,
                negative_pos_leads_its_contig=int(core["tid"][np.argmax(neg) - 1]) == 0 and int(core["tid"][np.argmax(neg) + 1]) == 1,
                # C truncation: -1 / step is bin 0 unless the step is 1, where it is bin -1 and the read is dropped
                negative_pos_bin=f["negative_pos_kept"] == (0 if step == 1 else 1), kinds=set((core["flag"][pre & ~cm] & 0x900).tolist()) == {0, 0x100, 0x800})
    regions = [(1, -5, 3), (1, 0, 10), (0, 140, 260), (0, 600, 640), (1, 40, 200)]
    return Case("unclustered:step%d" % step, b, contigs, step, regions, prem, f, stream="unclustered")


for _s in (1, 7):
    _register("unclustered:step%d" % _s, functools.partial(_unclustered, _s))


def _beyond_header():
    """Reads on contigs 2 and 3 of a header that names two: mapped for Stats::addRead, but statDepth and Bed::statDepth return at once (stats.cpp:60-61,
    bed.cpp:65-66) -- there is no bin_off[tid + 1] to look up.  Regions that name those contigs are dropped by the loader."""
    contigs = (700, 400)
    b = cc.build([cc.dense(1500, 0, 100), cc.dense(400, 3000, 20, tid=1), cc.dense(800, 5000, 100, tid=2), cc.dense(800, 6000, 100, tid=3)])
    core = b.core
    pre = counted(core, 2)
    f = dict(reads=b.n, counted_by_pre=int(pre.sum()), beyond=int((core["tid"] >= 2).sum()), blocks=-(-b.n // DP_BLOCK))
    prem = dict(beyond=f["beyond"] == 1600, counted=f["counted_by_pre"] == 1900, block_of_both=bool(pre[block(0)].any()) and not pre[block(0)].all(), block_of_none=not pre[block(1)].any())
    regions = [(2, 100, 300), (0, 90, 300), (3, 0, 1000), (1, 0, 50), (0, 400, 490)]
    return Case("unclustered:tid_beyond_header", b, contigs, 7, regions, prem, f, stream="beyond_header")


_register("unclustered:tid_beyond_header", _beyond_header)


# ---- Table
def _table_facts(b, contigs, step, regions, blk=0):
    bk = bin_keys(b.core, contigs, step, block(blk))
    rk = region_keys(b.core, contigs, regions, block(blk))
    return dict(reads=b.n, blocks=-(-b.n // DP_BLOCK), bin_keys=len(bk), region_keys=len(rk), bins_in_one_window=most_in_one_window(bk),
                regions_in_one_window=most_in_one_window(rk))


def _table_one_key():
    """Block 0 whole: 2048 reads in one bin and one region -- one cluster of 1024 reads and 256 small ones.  Then a partial block elsewhere."""
    contigs = (5000, 5000)
    b = cc.build([cc.pairs(700, np.arange(512), 0, 100, cc.ISZ, 110), cc.dense(1024, 0, 200), cc.dense(300, 5000, 1500, tid=1)])
    regions, step = [(1, 1400, 1600), (0, 0, 1000)], 1000
    f = _table_facts(b, contigs, step, regions)
    prem = dict(block_full=b.n > DP_BLOCK, one_bin=f["bin_keys"] == 1, one_region=f["region_keys"] == 1, region_is_not_first_in_file=regions[0][0] == 1)
    return Case("table:one_key", b, contigs, step, regions, prem, f, stream="one_key")


def _table_keys(n_keys):
    """One block of 2048 reads at step 1: clusters on m consecutive positions send the bins of m + 30 positions, a pile of pairs on the first adds no key."""
    contigs = (50, 2000)
    m = n_keys - cc.ISZ
    pad = (DP_BLOCK - 4 * m) // 2
    b = cc.build([cc.dense(4 * m, 0, 100, tid=1), cc.pairs(70000, np.arange(pad), 1, 100, cc.ISZ, 110)])
    regions, step = [(1, 90, 700)], 1
    f = _table_facts(b, contigs, step, regions)
    prem = dict(one_block=b.n == DP_BLOCK, bin_keys=f["bin_keys"] == n_keys, slots=n_keys - DP_SLOTS in (0, 1), keys_not_from_zero=min(bin_keys(b.core, contigs, step, block(0))) > 51)
    return Case("table:%d_keys" % n_keys, b, contigs, step, regions, prem, f, stream="keys%d" % n_keys)


def _table_many_keys():
    """One block: 1024 pairs 40 bases apart at step 1 -- 31 bins a pair, none shared."""
    contigs = (42000,)
    b = cc.build(cc.dense(DP_BLOCK, 0, 100, npairs=1, step=40))
    regions, step = [(0, 0, 42000), (0, 20000, 20100)], 1
    f = _table_facts(b, contigs, step, regions)
    prem = dict(one_block=b.n == DP_BLOCK, about_30000_keys=f["bin_keys"] == 1024 * 31, far_beyond_the_table=f["bin_keys"] > 50 * DP_SLOTS)
    return Case("table:30000_keys", b, contigs, step, regions, prem, f, stream="many_keys")


def _same_slot(lo, hi, n):
    """n keys of [lo, hi) with one home slot (the slot that the most keys of the range share)."""
    k = np.arange(lo, hi, dtype=np.int64)
    s = slot_of(k)
    best = int(np.bincount(s, minlength=DP_SLOTS).argmax())
    pick = k[s == best][:n]
    assert len(pick) == n
    return pick


def _table_window_bins():
    """Twelve bins of contig 1 whose keys share a home slot, eight reads in each, and nothing else in the block: the table holds at most eight of them."""
    contigs, step = (30000, 1200000), 100
    b0 = 1 + contigs[0] // step
    keys = _same_slot(b0 + 10, b0 + 1 + contigs[1] // step - 10, 12)
    left = (keys - b0) * step + 10                                                     # reads at +10 .. +60 of the bin: inside it
    b = cc.build([cc.pairs(np.arange(12), k, 1, left, cc.ISZ, left + 10) for k in range(4)])
    regions = [(1, int(left[0]), int(left[0]) + 5), (0, 0, 100)]
    f = _table_facts(b, contigs, step, regions)
    prem = dict(one_block=b.n == 96, nearly_empty=f["bin_keys"] == 12, ninth_key_finds_no_slot=f["bins_in_one_window"] >= DP_PROBES + 1, keys_are_what_was_picked=bin_keys(b.core, contigs, step, block(0)) == set(keys.tolist()))
    return Case("table:window_bins", b, contigs, step, regions, prem, f, stream="window_bins")


def _table_window_regions():
    """6000 regions of 20 bases on contig 1, 100 bases apart, behind 100 regions of contig 0 LATER in the file (a region's key is its grouped index: 100 + i);
    eight reads in each of twelve regions whose keys share a home slot."""
    contigs, step = (20000, 600200), 100000
    n_reg = 6000
    keys = _same_slot(100, 100 + n_reg, 12)
    left = (keys - 100) * 100 + 40
    regions = [(1, 100 * i + 40, 100 * i + 60) for i in range(n_reg)] + [(0, 100 * i, 100 * i + 30) for i in range(100)]
    b = cc.build([cc.pairs(np.arange(12), k, 1, left, cc.ISZ, left + 10) for k in range(4)] + [cc.dense(200, 500, 1000)])
    f = _table_facts(b, contigs, step, regions)
    rk = region_keys(b.core, contigs, regions, block(0))
    prem = dict(one_block=b.n == 296, nearly_empty=f["region_keys"] <= 32 and f["bin_keys"] <= 8, ninth_key_finds_no_slot=f["regions_in_one_window"] >= DP_PROBES + 1,
                picked_keys_in_use=set(keys.tolist()) <= rk, key_is_not_file_index=bool((grouped(regions, 2)[0][keys] != keys).all()))
    return Case("table:window_regions", b, contigs, step, regions, prem, f, stream="window_regions")


TABLE_SIZES = (1, 255, 256, 2047, 2048, 2049, 4097)


def _table_size(n):
    contigs = (3000, 50)
    b = cc.build(cc.dense(n + 40, 0, 100), truncate=n)
    regions, step = [(0, 95, 130), (0, 100, 2000), (1, 0, 10)], 7
    f = _table_facts(b, contigs, step, regions, blk=(n - 1) // DP_BLOCK)
    prem = dict(n_reads=b.n == n, blocks=f["blocks"] == -(-n // DP_BLOCK), last_block_holds=(n - 1) % DP_BLOCK + 1 == b.n - (f["blocks"] - 1) * DP_BLOCK, last_block_adds=f["bin_keys"] > 0)
    return Case("table:size_%d" % n, b, contigs, step, regions, prem, f, stream="size%d" % n)


_register("table:one_key", _table_one_key)
_register("table:512_keys", functools.partial(_table_keys, 512))
_register("table:513_keys", functools.partial(_table_keys, 513))
_register("table:30000_keys", _table_many_keys)
_register("table:window_bins", _table_window_bins)
_register("table:window_regions", _table_window_regions)
for _n in TABLE_SIZES:
    _register("table:size_%d" % _n, functools.partial(_table_size, _n))


# ---- BED: region lists over the short stream (reads on contigs 0, 1, 2 of four; contig 3 has none)
def overlaps(core, contig_len, regions):
    """Per region (file order): reads whose [start, end) shares a base with it, by brute force."""
    reg = np.asarray(regions, np.int64).reshape(-1, 3)
    s = core["pos"].astype(np.int64)
    e = s + core["l_qseq"]
    return np.asarray([int(((core["tid"] == t) & (s < z) & (e > a)).sum()) if 0 <= t < len(contig_len) else 0 for t, a, z in reg], np.int64)


def _bed_case(name, regions, premise):
    b = _short_stream()
    f = dict(regions=len(regions), sorted=sorted_contigs(regions, len(SHORT_CONTIGS)).tolist(), reads_on=np.bincount(b.core["tid"], minlength=4).tolist())
    prem = premise(b.core, np.asarray(regions, np.int64).reshape(-1, 3), f)
    return Case("bed:" + name, b, SHORT_CONTIGS, 100, regions, prem, f, stream="short")


def _bed(name, regions, premise):
    _register("bed:" + name, functools.partial(_bed_case, name, regions, premise))


def _all_sorted(f):
    return all(f["sorted"])


_bed("equal_starts", [(0, 120, 130), (0, 120, 400), (0, 120, 121), (0, 120, 120), (0, 300, 310), (0, 300, 305), (1, 50, 90), (1, 50, 60)],
     lambda core, reg, f: dict(sorted=_all_sorted(f), equal_starts=int((np.diff(reg[reg[:, 0] == 0, 1]) == 0).sum()) == 4, every_region_meets_reads=bool((overlaps(core, SHORT_CONTIGS, reg)[[0, 1, 2, 4, 5, 6, 7]] > 0).all())))

_LONG_FRONT = [(0, 100, 2900)] + [(0, 110 + 6 * i, 113 + 6 * i) for i in range(60)] + [(1, 30, 1900), (1, 35, 36), (1, 200, 203), (1, 260, 261)]
_bed("long_in_front", _LONG_FRONT,
     # a read at 400 meets none of the short regions (the last ends at 467): only r_pmax, held up by the first region, keeps the walk going back over all sixty
     lambda core, reg, f: dict(sorted=_all_sorted(f), long_first=reg[0, 2] > reg[1:61, 2].max() + 1000, reads_behind_the_short_ones=int(((core["tid"] == 0) & (core["pos"] > 470)).sum()) > 100,
                               short_ones=int((overlaps(core, SHORT_CONTIGS, reg)[1:61] > 0).sum()) == 60))

_bed("touching", [(0, 0, 100), (0, 529, 540), (1, 0, 40), (1, 294, 300)],
     # reads cover [100, 529) on contig 0 and [40, 294) on contig 1: regions that end where the first read starts or start where the last one ends add 0
     lambda core, reg, f: dict(sorted=_all_sorted(f), first_read=int(core["pos"][core["tid"] == 0].min()) == 100 and int(core["pos"][core["tid"] == 1].min()) == 40,
                               last_end=int((core["pos"] + core["l_qseq"])[core["tid"] == 0].max()) == 529 and int((core["pos"] + core["l_qseq"])[core["tid"] == 1].max()) == 294,
                               share_no_base=int(overlaps(core, SHORT_CONTIGS, reg).sum()) == 0))

_bed("zero_length", [(0, 50, 50), (0, 200, 200), (0, 200, 260), (0, 300, 300), (1, 100, 100), (2, 5000, 5000)],
     lambda core, reg, f: dict(sorted=_all_sorted(f), zero_length=int((reg[:, 1] == reg[:, 2]).sum()) == 5))

_bed("inverted", [(0, 150, 140), (0, 200, 100), (0, 210, 260), (0, 300, 299), (1, 100, 20), (1, 120, 180), (2, 800, 700)],
     lambda core, reg, f: dict(sorted=_all_sorted(f), inverted=int((reg[:, 2] < reg[:, 1]).sum()) == 5, well_formed_beside=int((reg[:, 2] > reg[:, 1]).sum()) == 2))

_bed("interleaved", [(0, 100, 200), (1, 40, 80), (2, 700, 720), (0, 150, 300), (1, 60, 300), (3, 0, 100), (0, 400, 405), (2, 710, 900), (1, 250, 251), (0, 400, 600)],
     lambda core, reg, f: dict(sorted=_all_sorted(f), contig_changes=int((np.diff(reg[:, 0]) != 0).sum()) == 9, grouped_order_is_not_file_order=grouped(reg, 4)[0].tolist() != list(range(10))))

_bed("one_contig_unsorted", [(0, 100, 200), (0, 150, 300), (0, 400, 600), (1, 200, 260), (1, 40, 80), (1, 60, 300), (1, 50, 55), (2, 700, 720)],
     lambda core, reg, f: dict(sorted=f["sorted"] == [True, False, True, True]))

_bed("absent_mixed", [(-1, 0, 5000), (0, 100, 200), (4, 100, 200), (1, 40, 80), (-1, 40, 80), (0, 150, 300), (7, 0, 1), (2, 700, 900), (1 << 20, 0, 100)],
     lambda core, reg, f: dict(sorted=_all_sorted(f), absent=int(((reg[:, 0] < 0) | (reg[:, 0] >= 4)).sum()) == 5, below=bool((reg[:, 0] == -1).any()), beyond=bool((reg[:, 0] >= 4).any()),
                               present=len(grouped(reg, 4)[0]) == 4))

_bed("none", [], lambda core, reg, f: dict(no_region=len(reg) == 0))

_bed("all_absent", [(-1, 100, 200), (4, 100, 200), (-1, 0, 10), (99, 150, 300)],
     lambda core, reg, f: dict(none_present=len(grouped(reg, 4)[0]) == 0, below=bool((reg[:, 0] == -1).any()), beyond=bool((reg[:, 0] >= 4).any())))

_bed("regions_without_reads", [(3, 0, 100), (3, 50, 900), (0, 100, 200), (2, 700, 900)],
     lambda core, reg, f: dict(sorted=_all_sorted(f), contig3_regions_no_reads=f["reads_on"][3] == 0 and int((reg[:, 0] == 3).sum()) == 2,
                               contig1_reads_no_regions=f["reads_on"][1] > 0 and not (reg[:, 0] == 1).any()))


def _break_skips(core, reg, f):
    """Region 1 of contig 0 shares bases with reads, but region 0 starts behind those reads' ends: the loop breaks before it gets there."""
    s = core["pos"].astype(np.int64)[core["tid"] == 0]
    e = s + RL
    meets = (s < reg[1, 2]) & (e > reg[1, 1])
    f["reads_that_meet_the_skipped_region"] = int(meets.sum())
    return dict(unsorted=f["sorted"][0] is False, skipped_region_meets_reads=f["reads_that_meet_the_skipped_region"] > 100, break_in_front=bool((reg[0, 1] > e[meets]).all()),
                later_reads_reach_both=bool(((e >= reg[0, 1]) & (s <= reg[0, 2])).any()))


_bed("unsorted_break", [(0, 450, 520), (0, 100, 430), (0, 440, 460), (1, 100, 150), (1, 40, 90)], _break_skips)

FAMILIES = ("interior", "contig_end", "unclustered", "table", "bed")
