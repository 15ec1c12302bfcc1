"""Streams for the edges of cluster formation (gce_cluster.hpp: k_cluster, k_blk_scan, k_events, k_leaders, k_num_*, k_scatter).  CPU only.

A case is a named stream with its parameter overrides, its contig lengths and a PREMISE: facts about the input that say why the stream is
in the catalogue (which scan block a read falls in, how many clustered reads a block holds, on which reads the periodic flush fires, how
many clusters stay pending behind an unmapped read).  The premise comes from the Python spec in gencore_amd/shard.py (clustered_mask,
cluster_left, cluster_right, stream_context), from plain numpy and from `spec_formation` below, a literal restatement of the reference's
read loop and flush walk (gencore.cpp:233-279, 295-390) over cluster KEYS only.  Nothing here asks the engine.

What the streams are made of: reads of 20 bases, no reference.  A cluster is a key (tid, left, right) with two or more pairs whose UMIs
(in the read name, behind the last ':') differ in their last base only: the periodic flush groups with --umi_diff_threshold 1 and merges
them, the end-of-file flush groups with 0 and does not, so a read that lands in the wrong cluster instance, or a cluster that gets the
wrong instance, changes out_flag / mate / fr of the table.  The bases of a read are a function of its cluster's number: two clusters
merged by mistake vote different bases.

A pair is a forward read at `left` (flag 99, isize +I) and a reverse read at `rpos` >= left (flag 147, mpos = left, isize -I): the
reverse read's position is free (inside 100 000 bases and not behind `right`), which is how a cluster's reads are put into chosen scan
blocks.  The stream is the stable sort of all reads by (tid, pos).
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from gencore_amd import shard
from gencore_amd.batch import ReadBatch
from gencore_amd.capi import CORE_DTYPE, default_params

SB = 1024                                   # SB_READS: reads per scan block of k_cluster
READ_LEN = 20
ISZ = 30                                    # |isize| of the ordinary pairs: the reverse read lies at left + 10
STD_CONTIGS = (1 << 28, 1 << 28)
GCE_ERR_UNSORTED = -10
_FIELDS = ("tid", "pos", "mtid", "mpos", "isize", "flag", "cid", "k")


# ------------------------------------------------------------------------------------------------------------ reads as arrays
def reads(n=None, **kw):
    """Table of reads: int64 arrays of one length, scalars broadcast."""
    n = max([np.size(v) for v in kw.values()]) if n is None else n
    return {f: np.broadcast_to(np.asarray(kw[f], np.int64), (n,)).copy() for f in _FIELDS}


def cat(parts):
    return {f: np.concatenate([p[f] for p in parts]) for f in _FIELDS}


def pairs(cid, k, tid, left, isz, rpos):
    """Both mates of every pair: all forward reads, then all reverse reads."""
    cid, k, tid, left, isz, rpos = np.broadcast_arrays(*(np.asarray(x, np.int64) for x in (cid, k, tid, left, isz, rpos)))
    return cat([reads(tid=tid, pos=left, mtid=tid, mpos=rpos, isize=isz, flag=99, cid=cid, k=k),
                reads(tid=tid, pos=rpos, mtid=tid, mpos=left, isize=-isz, flag=147, cid=cid, k=k)])


def dense(n, cid0, left0, tid=0, npairs=2, isz=ISZ, step=1):
    """n reads of small clusters, one cluster per `step` positions from left0 on: 2 x npairs reads each, the last cluster cut short (its
    reverse reads go first).  Occupies [left0, left0 + clusters x step + isz)."""
    per = 2 * npairs
    nc = -(-n // per)
    j = np.repeat(np.arange(nc), npairs)
    k = np.tile(np.arange(npairs), nc)
    left = left0 + j * step
    r = pairs(cid0 + j, k, tid, left, isz, left + isz - READ_LEN)
    drop = nc * per - n
    if drop:
        fwd_last = np.arange((nc - 1) * npairs, nc * npairs)
        order = np.concatenate([fwd_last, nc * npairs + fwd_last])            # the last cluster's reads: forward, then reverse
        keep = np.ones(2 * nc * npairs, bool)
        keep[order[len(order) - drop:]] = False
        r = {f: v[keep] for f, v in r.items()}
    return r


def junk(n, cid0, pos0, tid=0):
    """n reads that never reach the cluster map (gencore.cpp:269-271, 307-309): secondary, supplementary, mate unmapped far away."""
    i = np.arange(n)
    kind = i % 3
    return reads(tid=tid, pos=pos0 + i // 4, mtid=np.where(kind == 2, -1, tid), mpos=np.where(kind == 2, -1, pos0 + i // 4),
                 isize=0, flag=np.choose(kind, [0x100 | 99, 0x800 | 99, 73]), cid=cid0 + i, k=0)


ODD_KINDS = ("isize0", "mate_far_below", "isize_short", "left_ahead", "cross_contig")


def odd_group(kind, cid, pos, tid=0):
    """Four reads at one position with one cluster key (two names, UMIs one base apart) whose key is not the proper pair's:
    isize0          isize == 0, mate on the same contig        key (pos, pos - 1): right < pos
    mate_far_below  isize < 0, mpos = pos - 600                key (pos - 600, pos - 571): both ends far in front of the read
    isize_short     isize = -10 with mpos = pos - 30           isize inconsistent with mpos: right = pos - 21 < pos
    left_ahead      isize < 0 with mpos = pos + 30             isize inconsistent with mpos: left lies BEHIND the read's own position
    cross_contig    mate on the next contig                    right = -len(tid) x (mtid + 1) + mpos < 0"""
    cid, pos = np.broadcast_arrays(np.atleast_1d(np.asarray(cid, np.int64)), np.atleast_1d(np.asarray(pos, np.int64)))
    c4, p4 = np.repeat(cid, 4), np.repeat(pos, 4)
    k = np.tile([0, 1, 0, 1], len(cid))
    flag = np.tile([99, 99, 147, 147], len(cid))
    mtid, mpos, isz = {"isize0": (tid, p4 + 5, 0), "mate_far_below": (tid, p4 - 600, -ISZ), "isize_short": (tid, p4 - 30, -10),
                       "left_ahead": (tid, p4 + 30, -ISZ), "cross_contig": (tid + 1, np.full(len(p4), 777), 0)}[kind]
    return reads(tid=tid, pos=p4, mtid=mtid, mpos=mpos, isize=isz, flag=flag, cid=c4, k=k)


def unmapped_read(kind):
    """The read that ends the stream's first segment (gencore.cpp:255-262)."""
    tid, pos = {"tid<0": (-1, -1), "pos<0": (0, -1)}[kind]
    return dict(tid=tid, pos=pos, mtid=-1, mpos=-1, isize=0, flag=77, cid=99999999, k=0)


_NIB = np.asarray([1, 2, 4, 8], np.uint8)                                       # A C G T
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def sorted_reads(parts, truncate=None):
    """The parts as one table in stream order: stable sort by (tid, pos) -- equal positions keep the order given --, cut to `truncate` reads."""
    r = cat(parts) if isinstance(parts, (list, tuple)) else parts
    order = np.lexsort((np.arange(len(r["pos"])), r["pos"], r["tid"]))
    if truncate is not None:
        assert truncate <= len(order)
        order = order[:truncate]
    return {f: v[order] for f, v in r.items()}


def build(parts, truncate=None, inserts=(), pokes=()):
    """ReadBatch of the stream: parts sorted by (tid, pos) (stable: equal positions keep the order given), cut to `truncate` reads,
    `inserts` = [(stream index, read dict)] put in and `pokes` = [(index, field, value)] applied behind the sort."""
    r = sorted_reads(parts, truncate)
    for at, rd in sorted(inserts, key=lambda x: x[0]):
        r = {f: np.insert(v, at, rd[f]) for f, v in r.items()}
    for at, f, val in pokes:
        r[f][at] = val
    n = len(r["pos"])
    core = np.zeros(n, CORE_DTYPE)
    for f in ("tid", "pos", "mtid", "mpos", "isize", "flag"):
        core[f] = r[f]
    core["l_qname"], core["mapq"], core["n_cigar"], core["l_qseq"] = 22, 60, 1, READ_LEN
    cid, k = r["cid"], r["k"]
    name = np.zeros((n, 22), np.uint8)                                          # cccccccc kkkk : UUUUUUUU \0
    for d in range(8):
        name[:, 7 - d] = 48 + (cid // 10 ** d) % 10
    for d in range(4):
        name[:, 11 - d] = 48 + (k // 10 ** d) % 10
    name[:, 12] = ord(":")
    for j in range(7):
        name[:, 13 + j] = _ACGT[(cid >> (2 * j)) & 3]
    name[:, 20] = _ACGT[k & 3]                                                   # pairs of one cluster: UMIs one base apart
    h = cid.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)                    # 40 bits of a hash of the cluster number: two clusters differ in bases
    base = ((h[:, None] >> (np.uint64(2) * np.arange(4, 4 + READ_LEN, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)
    nib = _NIB[base]
    seq = (nib[:, 0::2] << 4 | nib[:, 1::2]).astype(np.uint8)
    qual = np.repeat((30 + 5 * (k & 1)).astype(np.uint8)[:, None], READ_LEN, axis=1)
    i64 = np.arange(n, dtype=np.uint64)
    return ReadBatch(core=core, qname_off=i64 * np.uint64(22), qname=np.ascontiguousarray(name).reshape(-1),
                     cigar_off=i64.copy(), cigar=np.full(n, READ_LEN << 4, np.uint32),
                     seq_off=i64 * np.uint64(READ_LEN // 2), seq=np.ascontiguousarray(seq).reshape(-1),
                     qual_off=i64 * np.uint64(READ_LEN), qual=np.ascontiguousarray(qual).reshape(-1),
                     nm=np.zeros(n, np.int32), nm_type=np.full(n, ord("C"), np.uint8), mi_off=None, mi=None)


# ------------------------------------------------------------------------------------------------------------ the spec
def keys_of(core, contig_len):
    """(clustered mask, left, right) per read: gencore.cpp:295-312."""
    return shard.clustered_mask(core), shard.cluster_left(core), shard.cluster_right(core, np.asarray(contig_len, np.int64))


def event_reads(core, period, tick_offset=0):
    """Stream indices of the reads on which the periodic flush fires (gencore.cpp:319-322), unmapped reads or not."""
    cm = shard.clustered_mask(core)
    tick = np.cumsum(cm) + tick_offset
    return np.nonzero(cm & (tick % period == 0))[0]


def spec_formation(core, period, contig_len, tick_offset=0, trailing_flush=0):
    """The reference's read loop over cluster keys alone: every clustered read joins the pending cluster of its key or opens one; on every
    period-th clustered read the flush walk takes the pending keys with tid < T, or tid == T and left < P and right < P (gencore.cpp:333-354:
    the break rules of the three nested loops come to that); the first unmapped read takes everything (finishConsensus, :255-262) and so does
    the end of the stream unless that has happened: what is opened behind the unmapped read and not taken by a later walk stays pending for
    good.  A cluster with left < 0 that finishConsensus meets is written pair by pair without clusterByUMI (gencore.cpp:401-407): n_as_they_are (a
    trailing flush stands for a later slice's periodic walk, which knows no such exception).
    Returns dict(n_taken: clusters handed to clusterByUMI, n_pending: clusters never handed on, n_as_they_are, n_events, first_unmapped (-1: none),
    events_in_front: walks before the first unmapped read, split: keys that had more than one cluster instance)."""
    cm, left, right = keys_of(core, contig_len)
    tid, pos = core["tid"].astype(np.int64), core["pos"].astype(np.int64)
    unm = (tid < 0) | (pos < 0)
    pending, n_taken, n_events, tick, first_unm, ev_front, seen, split, n_raw = set(), 0, 0, int(tick_offset), -1, 0, set(), set(), 0
    for i in np.nonzero(cm | unm)[0].tolist():
        if unm[i]:
            if first_unm < 0:
                first_unm, ev_front = i, n_events
                raw = sum(1 for q in pending if q[1] < 0)
                n_raw += raw; n_taken += len(pending) - raw; pending.clear()
            continue
        key = (int(tid[i]), int(left[i]), int(right[i]))
        if key not in pending:
            pending.add(key)
            if key in seen:
                split.add(key)
            seen.add(key)
        tick += 1
        if tick % period == 0:
            n_events += 1
            T, P = int(tid[i]), int(pos[i])
            took = [q for q in pending if q[0] < T or (q[0] == T and q[1] < P and q[2] < P)]
            n_taken += len(took)
            pending.difference_update(took)
    if first_unm < 0:
        raw = 0 if trailing_flush else sum(1 for q in pending if q[1] < 0)
        n_raw += raw; n_taken += len(pending) - raw; pending.clear()
        ev_front = n_events
    return dict(n_taken=n_taken, n_pending=len(pending), n_as_they_are=n_raw, n_events=n_events, first_unmapped=first_unm, events_in_front=ev_front,
                split=len(split))


def block_counts(core):
    """Clustered reads per scan block."""
    cm = shard.clustered_mask(core)
    nb = -(-len(core) // SB)
    return np.bincount(np.arange(len(core)) // SB, weights=cm, minlength=nb).astype(np.int64)


def event_places(core, period, tick_offset=0):
    """Which of the places k_events has to find hold a flush event: the first / the last clustered read of a scan block, the first
    clustered read behind a block without one, a read of the partial last block."""
    cm = shard.clustered_mask(core)
    ev = event_reads(core, period, tick_offset)
    cnt = block_counts(core)
    base = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rank = np.cumsum(cm)[ev] - base[ev // SB]                                 # `need` of k_events: 1 .. cnt
    first, last = rank == 1, rank == cnt[ev // SB]
    blk = ev // SB
    behind = first & (blk > 0) & (cnt[np.maximum(blk - 1, 0)] == 0)
    partial = (blk == len(cnt) - 1) & (len(core) % SB != 0)
    return dict(first=bool(first.any()), last=bool(last.any()), behind_empty=bool(behind.any()), partial=bool(partial.any()))


def nw_bd_of(n_reads, contig_len):
    """Bits of the (right - left + 1) field of a normal bucket word as gce_process lays it out (engine.hip: T, cb, qb, nw_bd).  This mirrors
    the engine and is used to SELECT inputs only; what the stream must give is the oracle's business."""
    n1 = max(n_reads, 1)
    T = (n1 + n1 // 4 + 2 * 2048 - 1) // 2048 * 2048
    qmax = (sum(contig_len) * 8 + 8) // T + 1
    cb = 1
    while cb < 33 and (1 << cb) <= n_reads + 1024:
        cb += 1
    qb = 1
    while qb < 52 and (1 << qb) <= qmax:
        qb += 1
    return min(62 - cb - qb, 40)


def key_bits_of(contig_len):
    """(key_bt, key_bl) of d_pack_key (engine.hip): bits of the largest tid and of the longest contig.  Mirrors the engine; selects inputs."""
    bt = 1
    while bt < 31 and (1 << bt) < max(len(contig_len), 1):
        bt += 1
    bl = 1
    while bl < 32 and (1 << bl) <= max(list(contig_len) + [1]):
        bl += 1
    return bt, bl


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    batch: ReadBatch
    period: int
    contig_len: tuple = STD_CONTIGS
    over: dict = field(default_factory=dict)                 # further gce_params overrides (tick_offset, trailing_flush)
    premise: dict = field(default_factory=dict)              # name -> bool, all must hold
    facts: dict = field(default_factory=dict)                # numbers the GPU test compares the engine with
    status: int = 0                                          # what the oracle must return
    events: bool = False                                     # run through batch.tick + gce_set_flush_events (key-range shard interface)

    def params(self):
        tl = np.asarray(self.contig_len, np.uint32)
        p = default_params(n_targets=len(tl), target_len=tl.ctypes.data if len(tl) else None, umi_prefix="", flush_period=self.period,
                           skip_low_complexity_cluster_threshold=1 << 20, **self.over)
        p._keep = tl
        return p

    def with_ticks(self):
        """(batch carrying the global ticks, (ev_tid, ev_pos)) from the spec (shard.stream_context)."""
        tick, et, ep = shard.stream_context(self.batch.core, self.period)
        b = self.batch.copy()
        b.tick = tick
        return b, (et, ep)


def _facts(batch, period, contig_len, tick_offset=0, trailing_flush=0):
    return spec_formation(batch.core, period, contig_len, tick_offset, trailing_flush)


def _case(name, batch, period, premise=None, contig_len=STD_CONTIGS, **kw):
    over = kw.get("over", {})
    f = _facts(batch, period, contig_len, over.get("tick_offset", 0), over.get("trailing_flush", 0)) if kw.get("status", 0) == 0 else {}
    return Case(name=name, batch=batch, period=period, contig_len=tuple(contig_len), premise=premise or {}, facts=f, **kw)


CASES = {}


def _register(name, fn):
    assert name not in CASES, name
    CASES[name] = functools.lru_cache(maxsize=None)(fn)


def get(name):
    return CASES[name]()


def family(prefix):
    return [n for n in CASES if n.startswith(prefix + ":")]


# ---- Sizes: N reads of dense small clusters at period 7
SIZES = (1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)


def _size_case(n):
    b = build(dense(n + 40, 0, 100), truncate=n)
    return _case("size:%d" % n, b, 7, dict(n_reads=b.n == n, blocks=-(-b.n // SB) == -(-n // SB), all_clustered=int(block_counts(b.core).sum()) == n))


for _n in SIZES:
    _register("size:%d" % _n, functools.partial(_size_case, _n))


# ---- Block fill
def _distinct_keys_in_block(core, contig_len, blk):
    cm, left, right = keys_of(core, contig_len)
    s = slice(blk * SB, (blk + 1) * SB)
    return len({(int(t), int(l), int(r)) for t, l, r, c in zip(core["tid"][s], left[s], right[s], cm[s]) if c})


def _fill_distinct():
    """Blocks 0 and 1: the forward reads of 1024 clusters; block 2: one reverse read of each = 1024 leaders in one block (LeadRec slots 0..1023,
    s_num 1023); block 3: the other reverse read of each; then a partial block of small clusters."""
    j = np.arange(1024)
    big = cat([pairs(j, 0, 0, 100 + j, 5000, 2000 + j), pairs(j, 1, 0, 100 + j, 5000, 4000 + j)])
    b = build([big, dense(300, 5000, 6000)])
    cnt = block_counts(b.core)
    return _case("fill:1024_keys", b, 100, dict(blocks=len(cnt) == 5, block2_full=cnt[2] == SB, block2_keys=_distinct_keys_in_block(b.core, STD_CONTIGS, 2) == SB,
                                                 block3_keys=_distinct_keys_in_block(b.core, STD_CONTIGS, 3) == SB))


def _one_cluster(shift, name):
    """Block 0: 256 small clusters; then ONE cluster of 1024 reads (512 forward at 1000, 512 reverse at 1010): the whole of block 1, one leader with
    the ranks 0..1023 -- or, behind one secondary read in front of the stream, the last 1023 reads of block 1 and the first of block 2."""
    k = np.arange(512)
    parts = [dense(1024, 0, 100), pairs(700, k, 0, 1000, ISZ, 1010), dense(1200, 1000, 2000)]
    if shift:
        parts.insert(0, junk(shift, 90000000, 50))
    b = build(parts)
    cm, left, right = keys_of(b.core, STD_CONTIGS)
    mine = np.nonzero(cm & (left == 1000))[0]
    return _case(name, b, 100, dict(cluster_reads=len(mine) == 1024, first_read=int(mine[0]) == 1024 + shift, contiguous=int(mine[-1]) - int(mine[0]) == 1023,
                                    in_block1=int((mine // SB == 1).sum()) == 1024 - shift, in_block2=int((mine // SB == 2).sum()) == shift))


def _fill_three_blocks():
    """One cluster of 2300 reads over blocks 0..3 between small clusters: its forward reads in ten runs with other keys of the same `left` between
    them, its reverse reads one per position among the small clusters' reads."""
    k = np.arange(1150)
    L = 617                                                                                       # the first read at 617 is read 2048
    parts = [dense(4 * 1300, 10000, 100)]
    for c in range(10):
        kk = k[c * 115:(c + 1) * 115]
        parts.append(reads(tid=0, pos=L, mtid=0, mpos=L + 11 + kk // 8, isize=2000, flag=99, cid=800, k=kk))
        parts.append(pairs(810 + c, np.arange(2), 0, L, 61 + c, L + 41 + c))                      # same left, another right
    parts.append(reads(tid=0, pos=L + 11 + k // 8, mtid=0, mpos=L, isize=-2000, flag=147, cid=800, k=k))
    b = build(parts)
    cm, left, right = keys_of(b.core, STD_CONTIGS)
    mine = np.nonzero(cm & (left == L) & (right == L + 1999))[0]
    blocks = np.unique(mine // SB)
    inter = int(cm[mine[0]:mine[-1] + 1].sum()) - len(mine)
    return _case("fill:2300_reads_three_blocks", b, 100, dict(cluster_reads=len(mine) == 2300, three_blocks=blocks.tolist() == [2, 3, 4], interleaved=inter >= 500))


def _fill_empty_block():
    """Block 0: clustered reads; block 1: secondary / supplementary / mate-unmapped reads only (n_lead = 0, blk_base[1] == blk_base[2]); blocks 2, 3."""
    b = build([dense(1024, 0, 100), junk(1024, 90000000, 1000), dense(1024 + 600, 1000, 2000)])
    cnt = block_counts(b.core)
    return _case("fill:empty_block", b, 100, dict(block0=cnt[0] == SB, block1_empty=cnt[1] == 0, block2=cnt[2] == SB, partial=cnt[3] == 600))


_register("fill:1024_keys", _fill_distinct)
_register("fill:one_cluster_1024", functools.partial(_one_cluster, 0, "fill:one_cluster_1024"))
_register("fill:one_cluster_1023+1", functools.partial(_one_cluster, 1, "fill:one_cluster_1023+1"))
_register("fill:2300_reads_three_blocks", _fill_three_blocks)
_register("fill:empty_block", _fill_empty_block)


# ---- Events
def events_stream():
    """Five blocks.  0: 1024 clustered reads; 1: none; 2: 1022 clustered reads around two secondary reads; 3: 524 reads that are not clustered, then
    500 that are; 4 (partial, 600 reads): all clustered.  Ticks: block 0 1..1024, block 2 1025..2046, block 3 2047..2546, block 4 2547..3146."""
    return build([dense(1024, 0, 100), junk(1024, 90000000, 1000), dense(500, 1000, 2000), junk(2, 90002000, 2500), dense(522, 2000, 3000),
                  junk(524, 90003000, 4000), dense(500, 3000, 5000), dense(600, 4000, 6000)])


EVENT_PERIODS = {1: ("first", "last", "behind_empty", "partial"), 2: ("last", "partial"), 3: ("first", "last", "partial"),
                 1023: ("last", "partial"), 1024: ("last", "partial"), 1025: ("first", "behind_empty", "partial")}


def _events_case(period, contigs=STD_CONTIGS, name=None):
    b = events_stream()
    cnt = block_counts(b.core)
    pl = event_places(b.core, period)
    tick, et, ep = shard.stream_context(b.core, period)
    ev = event_reads(b.core, period)
    prem = dict(layout=cnt.tolist() == [1024, 0, 1022, 500, 600], n_reads=b.n == 4 * SB + 600,
                spec_events=np.array_equal(b.core["pos"][ev], ep) and np.array_equal(b.core["tid"][ev], et))
    for place in ("first", "last", "behind_empty", "partial"):
        prem["event_on_" + place] = pl[place] == (place in EVENT_PERIODS[period])
    return _case(name or "events:period_%d" % period, b, period, prem, contig_len=contigs)


for _p in EVENT_PERIODS:
    _register("events:period_%d" % _p, functools.partial(_events_case, _p))


def _blocks_case(nblk):
    """nblk scan blocks at period 3 (k_events' 64-ary search: one level up to 65 blocks, two from 66 on; thousands of events = many k_events blocks),
    block 5 without a clustered read, the last block partial."""
    b = build([dense(5 * SB, 0, 100), junk(SB, 90000000, 2000), dense((nblk - 6) * SB - 500, 10000, 3000)])
    cnt = block_counts(b.core)
    ev = event_reads(b.core, 3)
    return _case("eventblocks:%d" % nblk, b, 3, dict(blocks=len(cnt) == nblk, empty_block=cnt[5] == 0, partial=b.n % SB == SB - 500,
                                                     many_event_blocks=len(ev) > 16 * 64, event_in_last_block=int(ev[-1]) // SB == nblk - 1))


for _n in (64, 65, 66, 67, 130):
    _register("eventblocks:%d" % _n, functools.partial(_blocks_case, _n))


def _count_case(name, n, period):
    b = build(dense(n, 0, 100))
    total = int(block_counts(b.core).sum())
    k, rem = divmod(total, period)
    want = {"events:none": (0, total), "events:k_period": (5, 0), "events:k_period-1": (4, period - 1), "events:k_period+1": (5, 1)}[name]
    return _case(name, b, period, dict(clustered=total == n, events=(k, rem) == want, three_blocks=-(-b.n // SB) == 3,
                                       last_read_is_event=(rem == 0) == (name == "events:k_period")))


_register("events:none", functools.partial(_count_case, "events:none", 2500, 2501))
_register("events:k_period", functools.partial(_count_case, "events:k_period", 2500, 500))
_register("events:k_period-1", functools.partial(_count_case, "events:k_period-1", 2499, 500))
_register("events:k_period+1", functools.partial(_count_case, "events:k_period+1", 2501, 500))


# ---- Odd reads
def odd_stream(n, every=16, contig1=True, borders=True):
    """n reads of small clusters on contig 0 with a group of odd reads every `every` positions, the five kinds in turn (and some reads on contig 1)."""
    npos = n // 4
    at = np.arange(1010, 1000 + npos - 40, every)
    parts = [dense(n + 400, 0, 1000)]
    for q, kind in enumerate(ODD_KINDS):
        sel = at[q::len(ODD_KINDS)]
        parts.append(odd_group(kind, 50000000 + 1000000 * q + np.arange(len(sel)), sel))
    b0 = sorted_reads(parts, n)
    for blk in range(1, -(-n // SB) if borders else 0):                        # an isize0 group at the end of every block: the walk that takes it comes in the next
        parts.append(odd_group("isize0", 59000000 + blk, b0["pos"][blk * SB - 6]))
        b0 = sorted_reads(parts, n)                                            # (a group moves the reads behind it: the next border is looked up in the new order)
    return [b0] + ([dense(600, 40000000, 100, tid=1)] if contig1 else [])


def odd_premise(core, period, contig_len):
    """Where the event that decides an odd read's instance lies (the first walk that takes its key: earlier block, the read's block, a later block)."""
    cm, left, right = keys_of(core, contig_len)
    tid, pos = core["tid"].astype(np.int64), core["pos"].astype(np.int64)
    odd = np.nonzero(cm & (right < pos))[0]
    ev = event_reads(core, period)
    eT, eP = tid[ev], pos[ev]
    where = {"earlier": 0, "same": 0, "later": 0, "none": 0}
    for i in odd.tolist():
        takes = (tid[i] < eT) | ((tid[i] == eT) & (left[i] < eP) & (right[i] < eP))
        j = int(np.argmax(takes)) if takes.any() else -1
        if j < 0:
            where["none"] += 1
        else:
            d = int(ev[j]) // SB - i // SB
            where["earlier" if d < 0 else ("same" if d == 0 else "later")] += 1
    kinds = dict(isize0=int((cm & (core["isize"] == 0) & (core["mtid"] == core["tid"])).sum()),
                 mate_far_below=int((cm & (core["isize"] < 0) & (core["mpos"] == pos - 600)).sum()),
                 isize_short=int((cm & (core["isize"] == -10)).sum()), left_ahead=int((cm & (left > pos)).sum()),
                 cross_contig=int((cm & (core["mtid"] != core["tid"])).sum()))
    return len(odd), where, kinds


def _odd_case(period, contigs=STD_CONTIGS, name=None):
    b = build(odd_stream(4 * SB - 600))
    n_odd, where, kinds = odd_premise(b.core, period, contigs)
    prem = dict(four_blocks=-(-b.n // SB) == 4, odd_reads=n_odd >= 100, decided_earlier=where["earlier"] > 0, decided_same=where["same"] > 0,
                decided_later=where["later"] > 0)
    for kd, v in kinds.items():
        prem["has_" + kd] = v >= 8
    c = _case(name or "odd:period_%d" % period, b, period, prem, contig_len=contigs)
    c.premise["keys_split_by_events"] = c.facts["split"] > 0
    return c


_register("odd:period_5", functools.partial(_odd_case, 5))
_register("odd:period_50", functools.partial(_odd_case, 50))


# ---- Keys that do not pack (d_pack_key gives 0: k_cluster makes every such read a leader, k_leaders takes the key from the key record)
def _nopack_beyond_contig():
    """Contig 1 is declared with 512 bases, contig 0 with 2^20: key_bl = 21, and clusters at 3 000 000 on contig 1 have left >> key_bl != 0."""
    contigs = (1 << 20, 512)
    b = build([dense(1500, 0, 100), dense(1500, 5000, 3000000, tid=1)])
    cm, left, right = keys_of(b.core, contigs)
    bt, bl = key_bits_of(contigs)
    return _case("nopack:beyond_contig", b, 50, dict(key_bl=bl == 21, beyond=int((cm & ((left >> bl) != 0)).sum()) == 1500, three_blocks=-(-b.n // SB) == 3), contig_len=contigs)


def _nopack_negative_left():
    """mpos == -1 with isize < 0 on the read's own contig: left = -1 (gencore.cpp:300-304).  The clusters sit at the head of the stream and the period is
    small, so a periodic walk takes them (gencore.cpp:355) like any other cluster; nopack:negative_left_pending holds the other path."""
    neg = []
    for c, (p, isz) in enumerate(((3, -30), (3, -31), (40, -30), (90, -200))):
        neg.append(reads(tid=0, pos=p, mtid=0, mpos=-1, isize=isz, flag=np.asarray([99, 99, 147, 147]), cid=60000000 + c, k=np.asarray([0, 1, 0, 1])))
    b = build(neg + [dense(2500, 0, 100)])
    cm, left, right = keys_of(b.core, STD_CONTIGS)
    ev = event_reads(b.core, 50)
    taken = all(b.core["pos"][ev[-1]] > r for r in right[cm & (left < 0)])
    return _case("nopack:negative_left", b, 50, dict(negative_left=int((cm & (left < 0)).sum()) == 16, taken_by_a_walk=bool(taken), three_blocks=-(-b.n // SB) == 3))


def _nopack_tid_beyond():
    """Reads on contigs 2 and 3 of a header that declares two."""
    b = build([dense(1500, 0, 100), dense(800, 5000, 100, tid=2), dense(800, 6000, 100, tid=3),
               odd_group("cross_contig", 70000000 + np.arange(4), 300 + 10 * np.arange(4), tid=2)])
    return _case("nopack:tid_beyond_header", b, 50, dict(beyond=int((b.core["tid"] >= 2).sum()) == 1616, four_blocks=-(-b.n // SB) == 4))


def _negative_left_pending(name, unmapped_at=None, trailing=0):
    """Clusters with left = -1 whose right end (|isize| = 5000) lies behind every read of the stream: no periodic walk takes them, finishConsensus meets
    them and writes their pairs as they are, without clusterByUMI (gencore.cpp:401-407): two pairs one base apart stay two records each and carry no tag.
    Groups at 500 and 600 (two pairs), at 650 (a pair and a read without its mate) and at 700 (a name with three reads: the third replaces the second as
    the right one, cluster.cpp:260-273), rights one apart at one position.  `unmapped_at`: an unmapped read there ends the first segment -- the group at 700
    comes behind it and is never processed.  `trailing`: the end of the stream counts as a later slice's periodic walk, which knows no such exception."""
    grp = lambda c, p, isz, k, flag: reads(tid=0, pos=p, mtid=0, mpos=-1, isize=isz, flag=np.asarray(flag), cid=61000000 + c, k=np.asarray(k))
    parts = [dense(2500, 0, 100), grp(0, 500, -5000, [0, 1, 0, 1], [99, 99, 147, 147]), grp(1, 500, -5001, [0, 1, 0, 1], [99, 99, 147, 147]),
             grp(2, 600, -5000, [0, 1, 0, 1], [99, 99, 147, 147]), grp(3, 650, -5002, [0, 1, 0], [99, 99, 147]), grp(4, 700, -5003, [0, 0, 0, 1, 1], [99, 147, 147, 99, 147])]
    ins = [(unmapped_at, unmapped_read("tid<0"))] if unmapped_at is not None else []
    b = build(parts, inserts=ins)
    c = _case(name, b, 50, {}, over=dict(trailing_flush=1) if trailing else {})
    cm, left, right = keys_of(b.core, STD_CONTIGS)
    neg = np.nonzero(cm & (left < 0))[0]
    last_p = int(b.core["pos"][event_reads(b.core, 50)[-1]])
    want_raw = 0 if trailing else (4 if unmapped_at is None else 3)                 # keys (-1, 4998) at 500 and 600 are one cluster
    c.premise = dict(negative_left=len(neg) == 20, behind_every_walk=bool((right[neg] > last_p).all()), three_blocks=-(-b.n // SB) == 3,
                     as_they_are=c.facts["n_as_they_are"] == want_raw, pending=(c.facts["n_pending"] > 0) == (unmapped_at is not None),
                     group_behind_unmapped=unmapped_at is None or int((neg > unmapped_at).sum()) == 5)
    return c


def _nopack_behind_contig_end():
    """Clusters that start behind the declared end of their contig: contig 0 has 250 bases and clusters at 100..399, contig 1 has none and clusters at 0..149, contig 2
    clusters at 0..149 inside it.  In genome-linear coordinates (the sum of the contig lengths in front + left) the clusters of contig 0 from 250 on, those of contig
    1 and those of contig 2 lie on the SAME 150 places with the same right - left: an identity made of the linear place and the span alone would count three
    clusters as one."""
    contigs = (250, 0, 1000, 1 << 20)
    b = build([dense(1200, 0, 100), dense(600, 5000, 0, tid=1), dense(600, 6000, 0, tid=2), dense(800, 7000, 100, tid=3)])
    cm, left, right = keys_of(b.core, contigs)
    tid = b.core["tid"].astype(np.int64)
    lin = np.concatenate([[0], np.cumsum(contigs)])[tid] + left
    keys = np.unique(np.stack([tid, left, right - left, lin], axis=1)[cm], axis=0)
    places, cnt = np.unique(keys[:, 2:], axis=0, return_counts=True)
    behind = cm & (left >= np.asarray(contigs, np.int64)[tid])
    return _case("nopack:behind_contig_end", b, 50, dict(behind_the_end=int(behind.sum()) == 600 + 600, three_keys_on_one_place=int((cnt == 3).sum()) == 150,
                                                         four_blocks=-(-b.n // SB) == 4), contig_len=contigs)


_register("nopack:behind_contig_end", _nopack_behind_contig_end)
_register("nopack:negative_left_pending", functools.partial(_negative_left_pending, "nopack:negative_left_pending"))
_register("nopack:negative_left_pending_unmapped", functools.partial(_negative_left_pending, "nopack:negative_left_pending_unmapped", 2300))
_register("nopack:negative_left_pending_trailing", functools.partial(_negative_left_pending, "nopack:negative_left_pending_trailing", None, 1))
_register("nopack:beyond_contig", _nopack_beyond_contig)
_register("nopack:negative_left", _nopack_negative_left)
_register("nopack:tid_beyond_header", _nopack_tid_beyond)
_register("nopack:no_contigs_events", functools.partial(_events_case, 1025, (), "nopack:no_contigs_events"))
_register("nopack:no_contigs_odd", functools.partial(_odd_case, 50, (), "nopack:no_contigs_odd"))


# ---- delta1 overflow
BIG_CONTIGS = (4294967000,) * 24


def _delta1():
    """24 contigs of nearly 2^32 bases make the quotient field of a normal bucket word wide and leave few bits for right - left + 1 (nw_bd).  Pairs that lie
    10 bases apart but carry |isize| = 2^30 (two clusters, rights one apart) do not fit it -- nor d_pack_key's field (kw == 0); |isize| = 2^24 fits
    d_pack_key but not nw_bd (fits == false with a packed key).  Both beside ordinary clusters of the same `left`, on the first and on the last contig.
    nw_bd_of / key_bits_of mirror the engine and only select the inputs; the oracle stays the judge."""
    parts = [dense(1800, 0, 100), dense(1200, 5000, 100, tid=23)]
    c = 80000000
    for tid in (0, 23):
        for isz in (1 << 30, (1 << 30) + 1, 1 << 24, (1 << 24) + 1):
            parts.append(pairs(c, np.arange(2), tid, 300, isz, 310)); c += 1
    b = build(parts)
    nw_bd = nw_bd_of(b.n, BIG_CONTIGS)
    bt, bl = key_bits_of(BIG_CONTIGS)
    cm, left, right = keys_of(b.core, BIG_CONTIGS)
    return _case("delta1:overflow", b, 50, dict(nw_bd_small=1 <= nw_bd <= 24, overflow_2_30=(1 << 30) >= (1 << nw_bd), overflow_2_24=(1 << 24) >= (1 << nw_bd),
                                                packs_2_24=((1 << 24) + 1) >> (62 - bt - bl) == 0, no_pack_2_30=(1 << 30) >> (62 - bt - bl) != 0,
                                                same_left=int((cm & (left == 300)).sum()) == 2 * (16 + 4), a_few_thousand=2000 <= b.n <= 5000), contig_len=BIG_CONTIGS)


_register("delta1:overflow", _delta1)


# ---- Home bucket taken
def _home_taken():
    """Twelve clusters with one (tid, left) and twelve rights: a position has TAB_WAYS = 8 home buckets, so at least two of the twelve share one whatever
    the way hash is, and the second to come goes to an exotic entry.  Four pairs each; the reverse reads are spread over 60 positions across the border of
    blocks 0 and 1, so that runs of one cluster in two blocks meet in the bucket (claim + join).  A second pile at the same left on contig 1."""
    parts = [dense(2 * SB + 300, 0, 100), dense(600, 20000, 100, tid=1)]
    for tid in (0, 1):
        for c in range(12):
            parts.append(pairs(30000 + 100 * tid + c, np.arange(4), tid, 340, 100 + c, 340 + 10 + 5 * c + np.arange(4)))
    b = build(parts)
    cm, left, right = keys_of(b.core, STD_CONTIGS)
    pile = cm & (left == 340) & (right >= 340 + 99) & (b.core["tid"] == 0)
    idx = np.nonzero(pile)[0]
    two = sum(1 for r in np.unique(right[pile]) if len(np.unique(idx[right[idx] == r] // SB)) == 2)
    pile1 = cm & (left == 340) & (right >= 340 + 99) & (b.core["tid"] == 1)
    return _case("home:taken", b, 50, dict(twelve_rights=len(np.unique(right[pile])) == 12, more_than_ways=12 > 8, pile_reads=len(idx) == 96,
                                           pile_in_two_blocks=sorted(np.unique(idx // SB).tolist()) == [0, 1], clusters_in_two_blocks=two >= 4,
                                           second_pile=len(np.unique(right[pile1])) == 12))


_register("home:taken", _home_taken)


# ---- Unmapped in mid-stream
UNMAPPED_OFFSETS = (0, 1, 511, 512, 1023)


def _unmapped_case(kind, off):
    """Four blocks of small clusters with an unmapped read at offset `off` of block 1: the walk ends the first segment there (finishConsensus with the
    end-of-file threshold), what comes behind opens new clusters -- also for keys whose forward reads lie in front -- and those that no later periodic walk
    takes are never processed."""
    at = SB + off
    b = build(dense(4 * SB - 1, 0, 100), inserts=[(at, unmapped_read(kind))])
    c = _case("unmapped:%s@%d" % (kind, off), b, 100, {})
    cm, left, right = keys_of(b.core, STD_CONTIGS)
    ev = event_reads(b.core, 100)
    key = (left << 32) | (right & 0xFFFFFFFF)
    both = np.intersect1d(key[:at][cm[:at]], key[at + 1:][cm[at + 1:]])
    c.premise = dict(first_unmapped=c.facts["first_unmapped"] == at, place=(at // SB, at % SB) == (1, off), four_blocks=b.n == 4 * SB,
                     clustered_behind_in_block=bool(cm[at + 1:2 * SB].any()) == (off < 1023), clustered_in_later_blocks=bool(cm[2 * SB:].all()),
                     keys_on_both_sides=len(both) >= 5, events_in_front=c.facts["events_in_front"] == int((ev < at).sum()) and c.facts["events_in_front"] >= 10,
                     events_behind=int((ev > at).sum()) >= 20, pending_clusters=c.facts["n_pending"] >= 5)
    return c


for _kind in ("tid<0", "pos<0"):
    for _off in UNMAPPED_OFFSETS:
        _register("unmapped:%s@%d" % (_kind, _off), functools.partial(_unmapped_case, _kind, _off))


# ---- Unsorted
def _unsorted_case(at):
    """One order violation: read `at` lies 5 bases in front of read at - 1 (k_cluster's neighbour load pv[] across the u = 0 / 1 border at 512 and across a
    block border)."""
    b0 = build(dense(4 * SB, 0, 100))
    b = build(dense(4 * SB, 0, 100), pokes=[(at, "pos", int(b0.core["pos"][at - 1]) - 5)])
    p = b.core["pos"].astype(np.int64)
    bad = np.nonzero(p[1:] < p[:-1])[0] + 1
    return _case("unsorted:@%d" % at, b, 100, dict(one_violation=bad.tolist() == [at]), status=GCE_ERR_UNSORTED)


for _at in (512, 1024, 3 * SB):
    _register("unsorted:@%d" % _at, functools.partial(_unsorted_case, _at))


# ---- Tick context
def _tick_case(period, off_name, trailing):
    off = {"1": 1, "period-1": period - 1, "period": period, "3e9+5": 3000000005}[off_name]
    b = build(dense(3 * SB - 300, 0, 100))
    name = "tick:period_%d_offset_%s_trailing_%d" % (period, off_name, trailing)
    c = _case(name, b, period, {}, over=dict(tick_offset=off, trailing_flush=trailing))
    total = int(block_counts(b.core).sum())
    c.premise = dict(three_blocks=-(-b.n // SB) == 3, events=c.facts["n_events"] == (off + total) // period - off // period,
                     first_event_moves=int(event_reads(b.core, period, off)[0]) == (period - off % period) - 1)
    return c


for _p in (7, 977):
    for _o in ("1", "period-1", "period", "3e9+5"):
        for _t in (0, 1):
            _register("tick:period_%d_offset_%s_trailing_%d" % (_p, _o, _t), functools.partial(_tick_case, _p, _o, _t))


# ---- Many blocks
MANY_READS = 300 * SB + 517


@functools.lru_cache(maxsize=None)
def _many_stream():
    b = build(odd_stream(MANY_READS, contig1=False, borders=False))
    return b, _facts(b, 977, STD_CONTIGS)


def _many(events):
    """300 full scan blocks and 517 reads: k_blk_scan's waves 0 and 1 (256 blocks each) and a second range that ends off a multiple of four; period 977; a
    group of odd reads every 16 positions.  `events`: the same stream through batch.tick + gce_set_flush_events (ticks and events from shard.stream_context)."""
    b, facts = _many_stream()
    cnt = block_counts(b.core)
    n_odd, where, kinds = odd_premise(b.core, 977, STD_CONTIGS)
    prem = dict(n_reads=b.n == MANY_READS, blocks=len(cnt) == 301, second_wave_range=256 < len(cnt) <= 512 and (len(cnt) - 256) % 4 != 0,
                odd_share=n_odd >= 10000, every_block_clustered=bool((cnt > 0).all()))
    return Case(name="many:blocks_301" + ("_ticks" if events else ""), batch=b, period=977, premise=prem, facts=facts, events=events)


_register("many:blocks_301", functools.partial(_many, False))
_register("many:blocks_301_ticks", functools.partial(_many, True))

FAMILIES = ("size", "fill", "events", "eventblocks", "odd", "nopack", "delta1", "home", "unmapped", "unsorted", "tick", "many")
