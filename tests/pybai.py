"""Pure-Python model of the BAI index gce_bam_index writes (SAMv1 5.2, with the rules of DESIGN.md 4c): written from the specification, not
from the kernels.  build(path) -> the .bai bytes (raises BaiError naming the record for a stream it refuses); parse_bai(bytes) -> its fields;
query(bam, bai, tid, beg, end) -> the mapped records a reader finds through the index.

Rules, in short: B  beg = max(pos, 0), end = beg + the M/D/N/=/X length of the CIGAR (1 if unmapped, no CIGAR or 0), bin = reg2bin(beg, end);
V  stream offset u -> coff << 16 | (u - uoff) of the first non-empty member that ends behind u, the stream's end -> the end of the last non-empty
member << 16; C  a run of consecutive records of one contig with one bin is a chunk (first start, last end); within a bin in file order, a
chunk merges into the one before when that one ends in the block the next begins in; bins ascending, not folded; pseudo-bin 37450 last;
L  mapped records only, every 16 kb window they overlap holds the smallest start, holes before the first filled window take ref_beg, later ones
the window before; O  (tid, pos) non-decreasing, unplaced records last, end <= 2^29."""
import struct
import zlib

from pybam import reg2bin
from recordstreams import bgzf_members

PSEUDO_BIN = 37450


class BaiError(ValueError):
    def __init__(self, record, why):
        self.record, self.why = record, why
        super().__init__("BAM record %d %s" % (record, why))


def inflate(blob):
    """-> (the inflated stream, [(uoff, coff, csize, usize)] of the non-empty members)"""
    u, mem = bytearray(), []
    for coff, csize, isize in bgzf_members(blob):
        xlen = struct.unpack_from("<H", blob, coff + 10)[0]
        data = zlib.decompress(blob[coff + 12 + xlen:coff + csize - 8], -15)
        assert len(data) == isize
        if isize:
            mem.append((len(u), coff, csize, isize))
        u += data
    return bytes(u), mem


def voff_of(mem, n_u):
    starts = [m[0] for m in mem]
    import bisect

    def v(u):
        if u >= n_u:
            return (mem[-1][1] + mem[-1][2]) << 16 if mem else 0
        j = bisect.bisect_right(starts, u) - 1
        return mem[j][1] << 16 | (u - mem[j][0])
    return v


def header_end(u):
    lt = struct.unpack_from("<i", u, 4)[0]
    o = 8 + lt
    n_ref = struct.unpack_from("<i", u, o)[0]; o += 4
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", u, o)[0]; o += 4 + ln + 4
    return o, n_ref


def records(path):
    """-> (n_ref, [dict(tid, pos, beg, end, bin, mapped, flag, start, vbeg, vend)]) in file order"""
    blob = open(path, "rb").read()
    u, mem = inflate(blob)
    v = voff_of(mem, len(u))
    o, n_ref = header_end(u)
    out = []
    while o < len(u):
        bs = struct.unpack_from("<i", u, o)[0]
        tid, pos, lq, _, _, nc, flag = struct.unpack_from("<iiBBHHH", u, o + 4)
        cig = struct.unpack_from("<%dI" % nc, u, o + 36 + lq)
        rlen = sum(w >> 4 for w in cig if (w & 15) in (0, 2, 3, 7, 8))
        if flag & 4 or rlen == 0:
            rlen = 1
        beg = max(pos, 0)
        end = beg + rlen
        out.append(dict(tid=tid, pos=pos, beg=beg, end=end, bin=reg2bin(beg, end), mapped=not flag & 4, flag=flag, start=o, vbeg=v(o), vend=v(o + 4 + bs)))
        o += 4 + bs
    return n_ref, out


def check_order(n_ref, recs):
    prev = None
    for i, r in enumerate(recs):
        if r["tid"] >= 0:
            if prev is not None and (prev["tid"] < 0 or (prev["tid"], prev["pos"]) > (r["tid"], r["pos"])):
                raise BaiError(i, "is out of coordinate order")
            if r["end"] > 1 << 29:
                raise BaiError(i, "ends beyond 2^29")
            if r["tid"] >= n_ref:
                raise BaiError(i, "names a contig the header does not have")
        prev = r


def index_fields(path):
    """-> (n_ref, contigs, n_no_coor); a contig: dict(bins={bin: [[beg, end], ..]}, meta=(ref_beg, ref_end, n_mapped, n_unmapped) or None,
    intervals=[...])"""
    n_ref, recs = records(path)
    check_order(n_ref, recs)
    contigs = [dict(bins={}, meta=None, intervals=[]) for _ in range(n_ref)]
    placed = [r for r in recs if r["tid"] >= 0]
    i = 0
    while i < len(placed):                                     # rule C: runs, then the merge within each bin in file order
        j = i
        while j < len(placed) and placed[j]["tid"] == placed[i]["tid"] and placed[j]["bin"] == placed[i]["bin"]:
            j += 1
        c = contigs[placed[i]["tid"]]["bins"].setdefault(placed[i]["bin"], [])
        beg, end = placed[i]["vbeg"], placed[j - 1]["vend"]
        if c and c[-1][1] >> 16 >= beg >> 16:
            c[-1][1] = max(c[-1][1], end)
        else:
            c.append([beg, end])
        i = j
    for t in range(n_ref):
        rs = [r for r in placed if r["tid"] == t]
        if not rs:
            continue
        nm = sum(1 for r in rs if r["mapped"])
        contigs[t]["meta"] = (rs[0]["vbeg"], rs[-1]["vend"], nm, len(rs) - nm)
        mapped = [r for r in rs if r["mapped"]]
        if not mapped:
            continue
        n_intv = max(((r["end"] - 1) >> 14) + 1 for r in mapped)
        lin = [None] * n_intv
        for r in mapped:                                       # rule L
            for w in range(r["beg"] >> 14, ((r["end"] - 1) >> 14) + 1):
                if lin[w] is None or r["vbeg"] < lin[w]:
                    lin[w] = r["vbeg"]
        last = rs[0]["vbeg"]
        for w in range(n_intv):
            if lin[w] is None:
                lin[w] = last
            last = lin[w]
        contigs[t]["intervals"] = lin
    return n_ref, contigs, len(recs) - len(placed)


def serialise(n_ref, contigs, n_no_coor):
    out = bytearray(b"BAI\1" + struct.pack("<i", n_ref))
    for c in contigs:
        bins = sorted(c["bins"])
        out += struct.pack("<i", len(bins) + (1 if c["meta"] else 0))
        for b in bins:
            out += struct.pack("<Ii", b, len(c["bins"][b]))
            for beg, end in c["bins"][b]:
                out += struct.pack("<QQ", beg, end)
        if c["meta"]:
            out += struct.pack("<Ii", PSEUDO_BIN, 2) + struct.pack("<QQQQ", *c["meta"])
        out += struct.pack("<i", len(c["intervals"]))
        for x in c["intervals"]:
            out += struct.pack("<Q", x)
    out += struct.pack("<Q", n_no_coor)
    return bytes(out)


def build(path):
    return serialise(*index_fields(path))


def parse_bai(data):
    """-> (n_ref, contigs as index_fields gives them, n_no_coor); asserts the layout is whole."""
    assert data[:4] == b"BAI\1"
    o = 4
    n_ref = struct.unpack_from("<i", data, o)[0]; o += 4
    contigs = []
    for _ in range(n_ref):
        c = dict(bins={}, meta=None, intervals=[])
        n_bin = struct.unpack_from("<i", data, o)[0]; o += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, o); o += 8
            ch = [list(struct.unpack_from("<QQ", data, o + 16 * k)) for k in range(n_chunk)]
            o += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2
                c["meta"] = (ch[0][0], ch[0][1], ch[1][0], ch[1][1])
            else:
                c["bins"][b] = ch
        n_intv = struct.unpack_from("<i", data, o)[0]; o += 4
        c["intervals"] = list(struct.unpack_from("<%dQ" % n_intv, data, o)); o += 8 * n_intv
        contigs.append(c)
    n_no_coor = struct.unpack_from("<Q", data, o)[0]; o += 8
    assert o == len(data)
    return n_ref, contigs, n_no_coor


def reg2bins(beg, end):
    """SAMv1 5.3: the bins that may hold a record overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, off in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(off + (beg >> shift), off + (end >> shift) + 1)
    return out


def query(bam, bai, tid, beg, end, recs=None):
    """The mapped records overlapping [beg, end) of contig tid, found the way a reader finds them: the chunks of every bin that may overlap,
    those ending at or before the linear index's bound dropped, the records read from each chunk's start to its end.  -> sorted record
    numbers (file order).  recs: records(bam)[1], when the caller has them."""
    _, contigs, _ = parse_bai(bai if isinstance(bai, (bytes, bytearray)) else open(bai, "rb").read())
    recs = records(bam)[1] if recs is None else recs
    by_v = {r["vbeg"]: i for i, r in enumerate(recs)}
    c = contigs[tid]
    iv = c["intervals"]
    min_off = 0 if not iv else iv[min(beg >> 14, len(iv) - 1)]
    found = set()
    for b in reg2bins(beg, end):
        for cb, ce in c["bins"].get(b, []):
            if ce <= min_off:
                continue
            i = by_v[cb]                                       # a chunk starts on a record
            while i < len(recs) and recs[i]["vbeg"] < ce:
                r = recs[i]
                if r["vbeg"] >= min_off and r["tid"] == tid and r["mapped"] and r["beg"] < end and r["end"] > beg:
                    found.add(i)
                i += 1
    return sorted(found)


def brute_force(bam, tid, beg, end, recs=None):
    recs = records(bam)[1] if recs is None else recs
    return [i for i, r in enumerate(recs) if r["tid"] == tid and r["mapped"] and r["beg"] < end and r["end"] > beg]
