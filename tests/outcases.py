"""Streams for the edges of the output table (gce_output.hpp: k_out_reduce, k_out_partials, k_out_meta<UNIFORM>, k_out_rows, k_out_mate, k_out_gather, and
the launch logic around them in engine.hip: capacities, the lq_uniform decision, the capped grids).  CPU only.

A case is a named stream with its parameters and a PREMISE: facts computed from the batch and from the ORACLE's result (out_flag, mate, nm_new) in plain numpy
that say the stream reaches the edge it is named for ("an emitted read among the last n % 8", "the mate sits at place 56 of its block behind flag bytes of both
values").  A premise that fails is an error of the catalogue, never a skip.  Nothing here asks the engine.

What the streams are made of -- four kinds of read whose fate is known before a base is read:
  pass-through    mapped, mtid = -1 (d_classify -> CLS_BYPASS, flag byte 2): emitted as it is at any position, length and NM state; its mpos / isize are free sort keys
  filler          flag 0x100 or 0x800: dropped, flag byte 0, any length
  emitted pair    one pair with a cluster key of its own (no UMI, cluster_size_req 1): two kind-1 records that are each other's mates;
                  two pairs of one cluster: which read becomes the template is the oracle's answer
  filtered pair   under cluster_size_req 2 a lone pair: clustered, never emitted
A stream is laid out in stream order from the start: read i lies at position pos0 + i // per_pos, and a read's role is changed in place, so that a case puts a
read on the index it wants (the last of a partial 8-read group, place 56 of a 64-read block, either side of read 4 194 304).
"""
import functools
import json
import os
from dataclasses import dataclass

import numpy as np

from gencore_amd.batch import ReadBatch
from gencore_amd.capi import CORE_DTYPE, GCE_NONE, default_params

TILE = 4096                                  # OUT_TILE: reads per block of k_out_reduce / k_out_meta
BLK = 64                                     # reads per rank64 entry
PARTIAL_ROUND = 1024                         # tiles per round of k_out_partials
ROWS_CAP = 8192 * 256                        # records per round of k_out_rows / k_out_mate
STD_CONTIGS = (1 << 28, 1 << 28)
PT_FLAG = 73                                 # paired, mate unmapped, first in pair
_FIELDS = ("tid", "pos", "mtid", "mpos", "isize", "flag", "lq", "nm", "cid")
HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------------------ reads as arrays
def stream(n, lq=20, per_pos=3, pos0=100, tid=0):
    """n pass-through reads in stream order, per_pos on a position.  nm: -1 = no NM tag.  cid names the read and seeds its bases."""
    i = np.arange(n, dtype=np.int64)
    full = lambda v: np.broadcast_to(np.asarray(v, np.int64), (n,)).copy()
    return dict(tid=full(tid), pos=pos0 + i // per_pos, mtid=full(-1), mpos=full(-1), isize=full(0), flag=full(PT_FLAG), lq=full(lq), nm=full(0), cid=i.copy())


def cat(parts):
    return {f: np.concatenate([p[f] for p in parts]) for f in _FIELDS}


def fill(R, idx, lq=None):
    """Make the reads fillers: secondary (even index) or supplementary (odd)."""
    idx = np.asarray(idx, np.int64)
    R["flag"][idx] = np.where(idx % 2 == 0, 0x100, 0x800) | PT_FLAG
    if lq is not None:
        R["lq"][idx] = lq
    return R


def pair(R, i, j, extra=0):
    """Reads i (forward, flag 99) and j > i (reverse, flag 147) become pairs: isize = distance + 50 + extra + the pair's number, so that pairs that share
    `left` get cluster keys of their own (every case's premise counts its kind-1 records)."""
    i, j = np.atleast_1d(np.asarray(i, np.int64)), np.atleast_1d(np.asarray(j, np.int64))
    assert (i < j).all() and (R["tid"][i] == R["tid"][j]).all()
    isz = R["pos"][j] - R["pos"][i] + 50 + extra + np.arange(len(i))
    for a, b, fl, sg in ((i, j, 99, 1), (j, i, 147, -1)):
        R["flag"][a], R["mtid"][a], R["mpos"][a], R["isize"][a] = fl, R["tid"][a], R["pos"][b], sg * isz
    R["cid"][j] = R["cid"][i]
    return R


def pair2(R, i1, i2, j1, j2, isz):
    """Two pairs of ONE cluster: forward reads i1, i2 on one position, reverse reads j1, j2 on one position, one isize."""
    assert R["pos"][i1] == R["pos"][i2] and R["pos"][j1] == R["pos"][j2]
    for a, b in ((i1, j1), (i2, j2)):
        for x, y, fl, sg in ((a, b, 99, 1), (b, a, 147, -1)):
            R["flag"][x], R["mtid"][x], R["mpos"][x], R["isize"][x] = fl, R["tid"][x], R["pos"][y], sg * isz
        R["cid"][b] = R["cid"][a]
    return R


_NIB = np.asarray([1, 2, 4, 8], np.uint8)                                       # A C G T


def build(R, name_w=8):
    """ReadBatch of the table (already in stream order).  Names: cid in name_w characters (digits; one letter at name_w 1) and a NUL, no ':' -- no UMI.  Bases: a hash of
    (cid, column); qualities 25 + cid % 16.  A read of L bases has the CIGAR L M, a read of none has no CIGAR."""
    n = len(R["pos"])
    key = R["tid"] * (1 << 32) + R["pos"]
    assert (key[1:] >= key[:-1]).all(), "stream is not sorted"
    core = np.zeros(n, CORE_DTYPE)
    for f in ("tid", "pos", "mtid", "mpos", "isize", "flag"):
        core[f] = R[f]
    lq = R["lq"]
    core["l_qname"], core["mapq"], core["n_cigar"], core["l_qseq"] = name_w + 1, 60, lq > 0, lq
    cid = R["cid"]
    name = np.zeros((n, name_w + 1), np.uint8)
    if name_w == 1:
        name[:, 0] = 65 + cid % 26
    else:
        for d in range(name_w):
            name[:, name_w - 1 - d] = 48 + (cid // 10 ** d) % 10
    sb = (lq + 1) // 2
    seq_off, qual_off, cig_off = np.cumsum(sb) - sb, np.cumsum(lq) - lq, np.cumsum(lq > 0) - (lq > 0)
    rid = np.repeat(np.arange(n), lq)
    col = np.arange(int(lq.sum()), dtype=np.int64) - np.repeat(qual_off, lq)
    h = cid[rid].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + col.astype(np.uint64) * np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(31)
    h *= np.uint64(0x94D049BB133111EB)
    nib = _NIB[((h >> np.uint64(40)) & np.uint64(3)).astype(np.int64)]
    seq = np.zeros(int(sb.sum()), np.uint8)
    at, even = seq_off[rid] + col // 2, col % 2 == 0
    seq[at[even]] = nib[even] << 4
    seq[at[~even]] |= nib[~even]
    qual = (25 + cid % 16).astype(np.uint8)[rid]
    return ReadBatch(core=core, qname_off=np.arange(n, dtype=np.uint64) * np.uint64(name_w + 1), qname=np.ascontiguousarray(name).reshape(-1),
                     cigar_off=cig_off.astype(np.uint64), cigar=(lq[lq > 0] << 4).astype(np.uint32), seq_off=seq_off.astype(np.uint64), seq=seq,
                     qual_off=qual_off.astype(np.uint64), qual=qual, nm=np.maximum(R["nm"], 0).astype(np.int32),
                     nm_type=np.where(R["nm"] >= 0, ord("C"), 0).astype(np.uint8), mi_off=None, mi=None)


def one_blob(batch):
    """The batch with ONE blob that holds a read's qualities right behind its packed bases, three pad bytes between records, records back to front
    (test_record_layout_one_blob_for_bases_and_qualities' layout, vectorised)."""
    lq = batch.core["l_qseq"].astype(np.int64)
    sb = (lq + 1) // 2
    rec_len = sb + lq + 3
    order = np.arange(batch.n)[::-1]
    start = np.zeros(batch.n, np.int64); start[order] = np.cumsum(rec_len[order]) - rec_len[order]
    blob = np.full(int(rec_len.sum()) + 64, 0x5A, np.uint8)
    for lens, off, data, dst in ((sb, batch.seq_off.astype(np.int64), batch.seq, start), (lq, batch.qual_off.astype(np.int64), batch.qual, start + sb)):
        within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
        blob[np.repeat(dst, lens) + within] = data[np.repeat(off, lens) + within]
    rec = batch.copy()
    rec.seq, rec.qual = blob, blob.copy()
    rec.seq_off, rec.qual_off = start.astype(np.uint64), (start + sb).astype(np.uint64)
    return rec


# ------------------------------------------------------------------------------------------------------------ the model table
def _gather(dst, dst_off, src, src_off, lens):
    for a in range(0, len(lens), 200000):
        ln = lens[a:a + 200000]
        tot = int(ln.sum())
        if tot:
            within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
            dst[np.repeat(dst_off[a:a + 200000], ln) + within] = src[np.repeat(src_off[a:a + 200000], ln) + within]


def rows_from_table(batch, t):
    """The engine's table of emitted records (gce_result) rebuilt from a per-read ResultTable: rows in bamComp order (gencore.h:19-47, input index as the
    last key), compact 16-byte aligned blobs laid out in row order (a layout of the model's own: the engine's is its business)."""
    em = np.nonzero(t.out_flag)[0]
    c = batch.core[em]
    order = np.lexsort((em, c["isize"], c["mpos"], c["mtid"], c["pos"], c["tid"]))
    src = em[order].astype(np.uint32)
    row_of = np.full(batch.n, GCE_NONE, np.uint32); row_of[src] = np.arange(len(src), dtype=np.uint32)
    s64 = src.astype(np.int64)
    lq = batch.core["l_qseq"].astype(np.int64)[s64]
    su, qu = ((lq + 1) // 2 + 15) // 16 * 16, (lq + 15) // 16 * 16
    seq_off, qual_off = np.cumsum(su) - su, np.cumsum(qu) - qu
    seq, qual = np.zeros(int(su.sum()), np.uint8), np.zeros(int(qu.sum()), np.uint8)
    _gather(seq, seq_off, t.seq, batch.seq_off.astype(np.int64)[s64], (lq + 1) // 2)
    _gather(qual, qual_off, t.qual, batch.qual_off.astype(np.int64)[s64], lq)
    m = t.mate[s64]
    mate = np.where(m == GCE_NONE, np.uint32(GCE_NONE), row_of[np.where(m == GCE_NONE, 0, m).astype(np.int64)])
    return dict(src=src, kind=t.out_flag[s64], qname_src=t.qname_src[s64], nm_new=t.nm_new[s64], fr=t.fr[s64], rr=t.rr[s64],
                mate=mate.astype(np.uint32), seq_off=seq_off.astype(np.uint64), qual_off=qual_off.astype(np.uint64), seq=seq, qual=qual)


def check_blobs(batch, rows):
    """The header's contract for the blobs of a table (include/gencore_amd.h), not their layout: offsets are multiples of 16, the intervals [off, off + 16 x units)
    of different rows are disjoint and lie inside the blobs, whose sizes are the sums of the rows' units; a record of no bases has no interval and need only keep
    its offsets aligned and inside.  Returns a list of complaints."""
    bad = []
    lq = batch.core["l_qseq"].astype(np.int64)[rows["src"].astype(np.int64)]
    for what, units, off, total in zip(("seq", "qual"), units_of(lq), (rows["seq_off"], rows["qual_off"]), (len(rows["seq"]), len(rows["qual"]))):
        off = off.astype(np.int64)
        if (off % 16 != 0).any():
            bad.append("%s_off is not a multiple of 16 at row %d" % (what, int(np.nonzero(off % 16)[0][0])))
        if total != 16 * int(units.sum()):
            bad.append("%s_bytes is %d, the rows' units come to %d" % (what, total, 16 * int(units.sum())))
        if len(off) and (off.min() < 0 or (off + 16 * units).max() > total):
            bad.append("%s: a row lies outside the blob" % what)
        o = np.argsort(off[units > 0], kind="stable")
        start = off[units > 0][o]
        end = start + 16 * units[units > 0][o]
        if (start[1:] < end[:-1]).any():
            bad.append("%s: the intervals of two rows overlap" % what)
    return bad


def units_of(lq):
    """(16-byte units of the packed bases, of the qualities) of a record of lq bases."""
    lq = np.asarray(lq, np.int64)
    return ((lq + 1) // 2 + 15) // 16, (lq + 15) // 16


def classes(core):
    """0 dropped, 1 clustered, 2 pass-through per read: gencore.cpp:255-271, 295-312."""
    drop = (core["tid"] < 0) | (core["pos"] < 0) | ((core["flag"] & 0x900) != 0)
    d = np.abs(core["mpos"].astype(np.int64) - core["pos"].astype(np.int64))
    cl = ((core["mtid"] == core["tid"]) & (d < 100000)) | (core["mtid"] >= 0)
    return np.where(drop, 0, np.where(cl, 1, 2)).astype(np.uint8)


def uniform_length(core):
    """The one length of every read that is not dropped, or -1: what k_describe's (lq_min, lq_max) tells the host."""
    lq = core["l_qseq"][classes(core) != 0]
    return int(lq[0]) if len(lq) and lq.min() == lq.max() else -1


def deciders(batch, rows):
    """Per neighbouring pair of rows of one (tid, pos) run: which key decides their order -- counts of mtid, mpos, isize, index."""
    c = batch.core[rows["src"].astype(np.int64)]
    same = (c["tid"][1:] == c["tid"][:-1]) & (c["pos"][1:] == c["pos"][:-1])
    out, undecided = {}, same.copy()
    for f in ("mtid", "mpos", "isize"):
        d = undecided & (c[f][1:] != c[f][:-1])
        out[f] = int(d.sum())
        undecided &= ~d
    out["index"] = int(undecided.sum())
    return out


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    batch: ReadBatch
    premise_fn: object                                       # (case, oracle result) -> {fact: bool}
    size_req: int = 1                                        # cluster_size_req (-s)
    contig_len: tuple = STD_CONTIGS
    contigs: tuple = None                                    # ASCII reference per contig (None: no reference)
    group: int = 0                                           # the family's number in the catalogue (1 Sizes .. 8 Large)

    def params(self, **over):
        tl = np.asarray(self.contig_len, np.uint32)
        kw = dict(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix="", flush_period=1 << 30, cluster_size_req=self.size_req,
                  skip_low_complexity_cluster_threshold=1 << 20)
        kw.update(over)
        p = default_params(**kw)
        p._keep = tl
        return p

    def reference(self):
        """[(FastaReader nibbles, bases)] for oracle_py.run / Engine.run, or None."""
        if self.contigs is None:
            return None
        from lencases import pack_reference
        return [(pack_reference(s), len(s)) for s in self.contigs]

    def premise(self, want):
        return self.premise_fn(self, want)

    @property
    def tiles(self):
        return -(-self.batch.n // TILE)


CASES = {}
GROUPS = {1: "size", 2: "tail", 3: "len", 4: "runs", 5: "mates", 6: "stats", 7: "cap", 8: "large"}


def _register(name, fn):
    assert name not in CASES and name.split(":")[0] in ("lq",) + tuple(GROUPS.values()), name
    CASES[name] = functools.lru_cache(maxsize=None)(fn)


def get(name):
    return CASES[name]()


def family(prefix):
    return [n for n in CASES if n.split(":")[0] == prefix]


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """The oracle's table of a case, once per process (the model test and the GPU tests share it; nobody changes it)."""
    from oracle import oracle_py
    c = get(name)
    return oracle_py.run(c.batch, c.params(), c.reference())


def _sprinkle(n, mod=5, at=3):
    i = np.arange(n)
    return i[i % mod == at]


# ---- 1 Sizes: all pass-through, and with fillers so that the last emitted read is not the last read
SIZES = (1, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, 8191, 8193)


def _size_case(n, fillers):
    R = stream(n)
    nf = 0
    if fillers:
        idx = np.union1d(_sprinkle(n), [n - 1])
        fill(R, idx); nf = len(idx)

    def prem(c, w):
        em = w.emitted()
        return dict(n_reads=c.batch.n == n, emitted=len(em) == n - nf, all_pass_through=bool((w.out_flag[em] == 2).all()),
                    last_read=(len(em) > 0 and em[-1] == n - 1) == (not fillers), one_length=uniform_length(c.batch.core) == (20 if n > nf else -1))
    return Case("size:%d%s" % (n, ":fillers" if fillers else ""), build(R), prem, group=1)


for _n in SIZES:
    for _f in (False, True):
        _register("size:%d%s" % (_n, ":fillers" if _f else ""), functools.partial(_size_case, _n, _f))


# ---- 2 Tail: n = 4096 + r; of the last, partial 8-read group only the last one or two reads are emitted
def _tail_case(r, as_pair):
    n = TILE + r
    R = stream(n)
    k = 1 if (as_pair or r % 2 or r < 2) else 2
    fill(R, np.union1d(_sprinkle(TILE, 7, 4), np.arange(TILE, n - k)))
    if as_pair:
        pair(R, 100, n - 1)

    def prem(c, w):
        f = w.out_flag
        d = dict(partial_group=0 < n % 8 == r, emitted_in_last_group=bool(f[n - r:].any()), only_the_last=bool((f[TILE:n - k] == 0).all() and (f[n - k:] != 0).all()),
                 second_tile_holds_only_them=int((f[TILE:] != 0).sum()) == k)
        if as_pair:
            d.update(kind1=f[n - 1] == 1 and f[100] == 1, mate_in_tile0=int(w.mate[n - 1]) == 100 and int(w.mate[100]) == n - 1)
        return d
    return Case("tail:%d%s" % (r, ":pair" if as_pair else ""), build(R), prem, group=2)


for _r in range(1, 8):
    for _p in (False, True):
        _register("tail:%d%s" % (_r, ":pair" if _p else ""), functools.partial(_tail_case, _r, _p))


# ---- 3 Lengths
LENGTHS = (0, 1, 2, 31, 32, 33, 255, 256, 257)
UNITS = {0: (0, 0), 1: (1, 1), 31: (1, 2), 32: (1, 2), 33: (2, 3), 255: (8, 16)}           # the issue's table of out_units_of


def _len_case(L):
    n = 200
    R = stream(n, lq=L)
    fill(R, _sprinkle(n))
    if L > 0:
        pair(R, [10, 32, 150], [20, 97, 151])
        pair2(R, 60, 61, 120, 121, 300)                      # two pairs of one cluster: one template per side, whichever the oracle takes

    def prem(c, w):
        em = w.emitted()
        u = units_of(L)
        return dict(one_length=uniform_length(c.batch.core) == L, units=UNITS.get(L, (int(u[0]), int(u[1]))) == (int(u[0]), int(u[1])),
                    emitted=len(em) >= 150, pairs=int((w.out_flag == 1).sum()) == (8 if L > 0 else 0),
                    one_template_of_two=L == 0 or (int((w.out_flag[[60, 61]] == 1).sum()), int((w.out_flag[[120, 121]] == 1).sum())) == (1, 1),
                    pass_through_only_at_0=L > 0 or bool((w.out_flag[em] == 2).all()))
    return Case("len:%d" % L, build(R), prem, group=3)


for _L in LENGTHS:
    _register("len:%d" % _L, functools.partial(_len_case, _L))


def _free_pairs(R, cand, gap, ok):
    """Of the candidate indices those where reads i and i + gap are both pass-through reads that `ok` admits."""
    cand = cand[(cand + gap < len(R["pos"]))]
    good = (R["flag"][cand] == PT_FLAG) & (R["flag"][cand + gap] == PT_FLAG) & ok(cand) & ok(cand + gap)
    return cand[good]


def _len_mixed():
    """About three tiles that cycle through every length; the last 8-read group is partial."""
    n = 3 * TILE - 7
    i = np.arange(n)
    lens = np.asarray(LENGTHS)
    R = stream(n, lq=lens[i % 9])
    fill(R, _sprinkle(n))
    a = _free_pairs(R, np.arange(20, n - 20, 181), 9, lambda x: R["lq"][x] > 0)
    pair(R, a, a + 9)

    def prem(c, w):
        em = w.emitted()
        cnt = {int(L): int((c.batch.core["l_qseq"][em] == L).sum()) for L in LENGTHS}
        k1 = c.batch.core["l_qseq"][w.out_flag == 1]
        return dict(three_tiles=c.tiles == 3, kind1=int((w.out_flag == 1).sum()) == 2 * len(a) >= 60, not_uniform=uniform_length(c.batch.core) == -1, every_length=min(cnt.values()) >= 500,
                    pairs_of_several_lengths=len(np.unique(k1)) >= 6, partial_last_group=n % 8 == 1 and w.out_flag[n - 1] != 0,
                    empty_record_in_front_of_a_record=bool(((c.batch.core["l_qseq"][em][:-1] == 0) & (c.batch.core["l_qseq"][em][1:] > 0)).any()))
    return Case("len:mixed", build(R), prem, group=3)


_register("len:mixed", _len_mixed)


def _lq_case(which):
    """The lq_uniform decision (engine.hip): k_describe's length range runs over every read that is not dropped."""
    n = TILE + 50
    R = stream(n, lq=32)
    fill(R, _sprinkle(n), lq=100 if which == "dropped" else None)
    if which == "pass_through":
        R["lq"][2222] = 33
    if which == "filtered":
        pair(R, 1000, 1007); R["lq"][[1000, 1007]] = 33
    else:
        pair(R, [50, 4000], [60, 4100])

    def prem(c, w):
        core, em = c.batch.core, w.emitted()
        elq, u = core["l_qseq"][em], uniform_length(core)
        d = dict(two_tiles=c.tiles == 2, emitted=len(em) > 3000)
        if which == "dropped":
            d.update(uniform_path=u == 32, dropped_read_of_another_length=bool((core["l_qseq"][classes(core) == 0] == 100).any()), kind1=int((w.out_flag == 1).sum()) == 4)
        elif which == "pass_through":
            d.update(leaves_the_uniform_path=u == -1, one_emitted_read_of_another_length=int((elq != 32).sum()) == 1 and w.out_flag[2222] == 2)
        else:
            d.update(leaves_the_uniform_path=u == -1, emitted_set_uniform=bool((elq == 32).all()), cluster_filtered=not w.out_flag[[1000, 1007]].any(),
                     clustered=bool((classes(core)[[1000, 1007]] == 1).all()))
        return d
    return Case("lq:" + {"dropped": "dropped_other_length", "pass_through": "pass_through_other_length", "filtered": "filtered_cluster_other_length"}[which],
                build(R), prem, size_req=2 if which == "filtered" else 1, group=3)


for _w, _nm in (("dropped", "dropped_other_length"), ("pass_through", "pass_through_other_length"), ("filtered", "filtered_cluster_other_length")):
    _register("lq:" + _nm, functools.partial(_lq_case, _w))


# ---- 3 / 6: 67 tiles of mixed short reads: the s_so / s_qo lists over many tiles and the 64 post-Stats slots wrapping, per tile another mix of NM
MANY_LENGTHS = (0, 1, 2, 17, 31, 32, 33)
MANY_TILES = 66


def _many_tiles():
    n = MANY_TILES * TILE + 11
    i = np.arange(n)
    tile = i // TILE
    R = stream(n, lq=np.asarray(MANY_LENGTHS)[i % 7])
    u = ((i * 2654435761) >> 7) % 67
    lo = 4 + tile % 23
    R["nm"] = np.where(u < lo, -1, np.where(u < lo + 10 + tile // 23 * 4, 0, 1 + i % 5))
    fill(R, _sprinkle(n, 6, 1))
    a = _free_pairs(R, np.arange(40, n - 100, 997), 70, lambda x: R["lq"][x] > 0)
    pair(R, a, a + 70)

    def prem(c, w):
        core, f = c.batch.core, w.out_flag
        nt = c.tiles
        t = np.arange(c.batch.n) // TILE
        em = f != 0
        present = c.batch.nm_type != 0
        mix = [(int((em & ~present & (t == k)).sum()), int((em & present & (c.batch.nm == 0) & (t == k)).sum()), int((em & present & (c.batch.nm > 0) & (t == k)).sum()))
               for k in range(nt)]
        full = mix[:MANY_TILES]
        return dict(tiles=nt == MANY_TILES + 1 > 64 + 2, kind1=int((f == 1).sum()) == 2 * len(a) >= 300, not_uniform=uniform_length(core) == -1, short_reads=int(core["l_qseq"].max()) <= 33,
                    every_tile_emits=min(sum(m) for m in full) > 3000, slots_wrap_onto_nonzero=all(sum(mix[k]) > 0 and sum(mix[k + 64]) > 0 for k in range(nt - 64)),
                    every_tile_its_own_mix=len(set(mix)) == nt, every_nm_state_in_every_full_tile=min(min(m) for m in full) > 100,
                    pairs_in_most_tiles=len(np.unique(t[f == 1])) >= 60, partial_last_tile=c.batch.n % TILE == 11)
    return Case("stats:67_tiles_mixed", build(R), prem, group=6)


_register("stats:67_tiles_mixed", _many_tiles)


def _nm_patched():
    """The hand-derived vector nm_is_patched_only_when_stored_as_type_C: two clusters of three pairs whose consensus moves the template back to the reference;
    NM is rewritten where it is stored as type 'C' (nm_new >= 0 in the table) and kept where it is stored as 'S'."""
    v = json.load(open(os.path.join(HERE, "golden", "hand_derived", "nm_is_patched_only_when_stored_as_type_C.json")))
    b = ReadBatch.from_records(v["records"])
    contigs = tuple(c["sequence"]["repeat"] * c["sequence"]["times"] for c in v["contigs"])

    def prem(c, w):
        em = w.emitted()
        return dict(four_records=len(em) == 4, one_nm_patched=int((w.nm_new[em] >= 0).sum()) == 1, patched_to_zero=int(w.nm_new[em].max()) == 0,
                    one_kept_with_mismatch=int(((w.nm_new[em] < 0) & (c.batch.nm[em] > 0)).sum()) == 1, templates=bool((w.out_flag[em] == 1).all()))
    return Case("stats:nm_patched", b, prem, contig_len=tuple(len(s) for s in contigs), contigs=contigs, group=6)


_register("stats:nm_patched", _nm_patched)


# ---- 4 Runs of equal (tid, pos)
RUN_MPOS, RUN_ISIZE = (-7, -1, 0, 5), (-3, 0, 4)


def _runs_case(name, n, runs, cross=4, npairs=24):
    """Reads [a, b) of every run lie on ONE position.  In a run, in an order drawn by a seeded generator: pass-through reads whose (mpos, isize) come from
    4 x 3 values (ties in every key, full ties by the hundred), a few fillers, forward reads of emitted pairs whose mates lie behind the run and reverse reads of
    pairs whose mates lie in front of it (mtid = tid), and `cross` clustered reads whose mates lie on the next contig (mtid = tid + 1; the mates close the stream)."""
    rng = np.random.default_rng(len(name) * 1000 + n)
    R = stream(n, per_pos=1)
    in_run = np.zeros(n, bool)
    for a, b in runs:
        R["pos"][a:b] = R["pos"][a]
        in_run[a:b] = True
    free = np.nonzero(~in_run)[0]
    parts, used, ncross = [R], set(), 0
    for a, b in runs:
        m = b - a
        idx = a + rng.permutation(m)
        R["mpos"][a:b] = rng.choice(RUN_MPOS, m)
        R["isize"][a:b] = rng.choice(RUN_ISIZE, m)
        fill(R, idx[:m // 20])
        idx = idx[m // 20:]
        k = min(npairs, m // 10)
        behind = [x for x in free if x >= b and x not in used][:k]
        front = [x for x in free[::-1] if x < a and x not in used][:k]
        used.update(behind); used.update(front)
        if behind:
            pair(R, np.sort(idx[:len(behind)]), behind, extra=1000)
        if front:
            pair(R, front[::-1], np.sort(idx[k:k + len(front)]), extra=2000)
        for x in idx[2 * k:2 * k + cross]:
            R["flag"][x], R["mtid"][x], R["mpos"][x], R["isize"][x] = 97, 1, 777 + ncross, 0
            ncross += 1
    if ncross:
        T = stream(ncross, per_pos=1, pos0=777, tid=1)
        cr = np.nonzero(R["mtid"] == 1)[0]
        T["flag"][:], T["mtid"][:], T["mpos"][:], T["cid"] = 145, 0, R["pos"][cr], R["cid"][cr]
        parts.append(T)
    R = cat(parts)
    first_last = name.endswith("first_last")

    def prem(c, w):
        core, f = c.batch.core, w.out_flag
        rows = rows_from_table(c.batch, w)
        dec = deciders(c.batch, rows)
        em = np.nonzero(f)[0]
        d = dict(every_key_decides=min(dec["mtid"], dec["mpos"], dec["isize"]) >= 1, full_ties=dec["index"] >= 50,
                 order_is_not_input_order=not np.array_equal(rows["src"], em), negative_keys=bool((core["mpos"][em] < -1).any() and (core["isize"][em] < 0).any()))
        for a, b in runs:
            e = em[(em >= a) & (em < b)]
            mt = core["mtid"][e]
            d["run_%d_records" % a] = len(e) >= {"runs:300": 300, "runs:5000": 5000}.get(name, (b - a) * 17 // 20)
            d["run_%d_mtid_kinds" % a] = bool((mt == -1).any() and (mt == 0).any()) and (cross == 0 or bool((mt == 1).any()))
            d["run_%d_kind1" % a] = bool((f[e] == 1).any())
        if first_last:
            d.update(run_at_the_first_position=runs[0][0] == 0 and core["pos"][0] == core["pos"][runs[0][1] - 1],
                     run_at_the_last_position=runs[-1][1] == c.batch.n and core["pos"][-1] == core["pos"][runs[-1][0]])
        for a, b in runs:
            if a // TILE != (b - 1) // TILE:
                edge = (a // TILE + 1) * TILE
                lo, hi = em[em < edge][-1], em[em >= edge][0]
                d["run_%d_spans_a_tile_edge" % a] = a <= lo and hi < b and core["pos"][lo] == core["pos"][hi]
        return d
    return Case(name, build(R), prem, group=4)


_register("runs:300", functools.partial(_runs_case, "runs:300", 1000, ((200, 560),)))
_register("runs:5000", functools.partial(_runs_case, "runs:5000", 8000, ((1500, 7000),)))
_register("runs:4000_4200", functools.partial(_runs_case, "runs:4000_4200", 4500, ((4000, 4201),)))
_register("runs:first_last", functools.partial(_runs_case, "runs:first_last", 600, ((0, 60), (540, 600)), 0))


# ---- 5 Mates
PLACES = (0, 1, 7, 8, 9, 56, 63)
DISTANCES = (1, 63, 64, 65, 4095, 4096, 10000)


def _mates():
    """Emitted pairs placed so that the mate sits at every place of PLACES in its 64-read block, every distance of DISTANCES behind and in front of the record;
    fillers on every fifth read put flag bytes of value 0 between those of value 2; the last block is partial and holds a mate."""
    n = 4 * TILE + 37
    R = stream(n)
    used = set()
    I, J = [], []
    for p in PLACES:
        for d in DISTANCES:
            for behind in (True, False):
                for b in range(n // BLK + 1):
                    blk = (b * 37 + 11 * p + d) % (n // BLK + 1)                 # spread the pairs over the stream
                    i, j = (blk * BLK + p - d, blk * BLK + p) if behind else (blk * BLK + p, blk * BLK + p + d)
                    if 0 <= i and j < n and i not in used and j not in used:
                        used.update((i, j)); I.append(i); J.append(j)
                        break
                else:
                    raise AssertionError((p, d, behind))
    for i, j in ((n - 37 - 100, n - 5), (n - 30, n - 3)):                          # mates in the last, partial block
        assert i not in used and j not in used
        used.update((i, j)); I.append(i); J.append(j)
    fl = _sprinkle(n)
    fill(R, fl[~np.isin(fl, list(used))])
    o = np.argsort(I)
    pair(R, np.asarray(I)[o], np.asarray(J)[o])

    def prem(c, w):
        f = w.out_flag
        k = np.nonzero((f == 1) & (w.mate != GCE_NONE))[0]
        m = w.mate[k].astype(np.int64)
        place, delta = m % BLK, m - k
        c2, c0 = np.concatenate([[0], np.cumsum(f == 2)]), np.concatenate([[0], np.cumsum(f == 0)])
        n2, n0 = c2[m] - c2[m - place], c0[m] - c0[m - place]
        d = dict(pairs=len(k) == 2 * len(I), partial_last_block=c.batch.n % BLK == 37, mate_in_the_last_block=bool((m >= c.batch.n - 37).any()),
                 other_tile=bool((m // TILE != k // TILE).any()), other_block_same_tile=bool(((m // BLK != k // BLK) & (m // TILE == k // TILE)).any()))
        for p in PLACES:
            at = place == p
            d["place_%d" % p] = bool(at.any()) and (p == 0 or bool((n2[at] + n0[at] > 0).any())) and (p < 7 or bool(((n2[at] > 0) & (n0[at] > 0)).any()))
            d["place_%d_both_directions" % p] = bool((delta[at] > 0).any() and (delta[at] < 0).any())
        for dd in DISTANCES:
            d["distance_%d" % dd] = bool((delta == dd).any() and (delta == -dd).any())
        return d
    return Case("mates:places", build(R), prem, group=5)


_register("mates:places", _mates)


# ---- 7 Capacity: every read emitted at the lengths where the 16-byte padding is largest against the payload
def _cap_case(L):
    n = 3 * TILE + 5
    R = stream(n, lq=L)

    def prem(c, w):
        su, qu = units_of(L)
        return dict(every_read_emitted=len(w.emitted()) == n, fifteen_pad_bytes=max(16 * int(su) - (L + 1) // 2, 16 * int(qu) - L) == 15,
                    uniform=uniform_length(c.batch.core) == L, partial_last_group=n % 8 == 5)
    return Case("cap:%d" % L, build(R), prem, group=7)


for _L in (1, 17, 33):
    _register("cap:%d" % _L, functools.partial(_cap_case, _L))


def _cap_one_blob():
    n = 300
    R = stream(n, lq=33)
    fill(R, _sprinkle(n))
    pair(R, [10, 32, 150], [20, 97, 151])
    b = one_blob(build(R))

    def prem(c, w):
        bt = c.batch
        return dict(one_blob=np.array_equal(bt.seq, bt.qual), qualities_behind_bases=bool((bt.qual_off == bt.seq_off + np.uint64(17)).all()),
                    back_to_front=bool((np.diff(bt.seq_off.astype(np.int64)) < 0).all()), kind1=int((w.out_flag == 1).sum()) == 6)
    return Case("cap:one_blob_33", b, prem, group=7)


_register("cap:one_blob_33", _cap_one_blob)


# ---- 8 Large: 1025 tiles + 5 reads of one base
LARGE_N = (PARTIAL_ROUND + 1) * TILE + 5
LARGE_EDGE = PARTIAL_ROUND * TILE                          # read 4 194 304: the first of k_out_partials' second round


def _large():
    """k_out_partials' second round (s_carry) and the second trip of k_out_rows / k_out_mate round their capped grid: pass-through reads and fillers of one base with
    one-letter names, three on a position (1.4 M short runs), and emitted pairs in the last two tiles whose mates straddle read 4 194 304."""
    n = LARGE_N
    R = stream(n, lq=1)
    R["mpos"] = -1 - (np.arange(n) * 7 % 3)                   # the three reads of a position come in another order than they go out
    fill(R, _sprinkle(n, 11, 5))
    k = np.arange(1, 40)
    cand_i, cand_j = LARGE_EDGE - 1 - 53 * k, LARGE_EDGE + 47 * k
    ok = (R["flag"][cand_i] == PT_FLAG) & (R["flag"][cand_j] == PT_FLAG)
    I, J = list(cand_i[ok][::-1]), list(cand_j[ok][::-1])
    I += [LARGE_EDGE - 1, LARGE_EDGE + 1, n - 700]; J += [LARGE_EDGE, n - 1, n - 2]
    o = np.argsort(I)
    pair(R, np.asarray(I)[o], np.asarray(J)[o])

    def prem(c, w):
        f = w.out_flag
        k1 = np.nonzero(f == 1)[0]
        m = w.mate[k1].astype(np.int64)
        n_out = int((f != 0).sum())
        rows_before_edge = int((f[:LARGE_EDGE] != 0).sum())
        return dict(second_round_of_partials=c.batch.n // TILE == PARTIAL_ROUND + 1 and c.tiles == PARTIAL_ROUND + 2, second_round_emits=int((f[LARGE_EDGE:] != 0).sum()) > 3000,
                    rows_grid_goes_round=n_out > ROWS_CAP, pairs=len(k1) == 2 * len(I) >= 48, only_in_the_last_two_tiles=int(k1.min()) >= LARGE_EDGE - TILE,
                    mates_straddle_the_edge=int(((k1 < LARGE_EDGE) != (m < LARGE_EDGE)).sum()) >= 40, mate_in_the_last_group=bool((m >= n - 5).any()),
                    neighbours_across_the_edge=int(w.mate[LARGE_EDGE]) == LARGE_EDGE - 1, partial_last_group=n % 8 == 5,
                    short_runs=int(c.batch.core["pos"][-1]) - int(c.batch.core["pos"][0]) > 1390000, rows_in_front_of_the_edge=rows_before_edge > ROWS_CAP)
    return Case("large:1025_tiles", build(R, name_w=1), prem, group=8)


_register("large:1025_tiles", _large)


def back_to_back_order():
    """The cases of groups 1-7 in an order that goes down and up in size at every step: the largest, the smallest, the second largest, the second smallest, ..."""
    names = sorted((n for n in CASES if not n.startswith("large:")), key=lambda x: (get(x).batch.n, x))
    out = []
    while names:
        out.append(names.pop())
        if names:
            out.append(names.pop(0))
    return out
