"""Million-record streams for the tests that take the file layer's kernels past one grid (tests/test_file_second_trip_gpu.py,
tests/test_gpu_inflate_launches.py), built in a second or two: a base block of K items (raw BAM records, or SAM lines) made with the
existing case builders is tiled R times with numpy, and every copy is then patched in place at known offsets -- an 8-digit global index
in the read name (fixed width, so that text tiles too), `pos` and `tid` where a test wants them -- so that no two records are equal and a
record that lands in the wrong place, or never lands, shows.  The expectation of a per-record rewriter is the Python model's output on
the base block, tiled and patched the same way; the expectation of the sort is a numpy stable argsort of rule S's key
(tests/test_bigstreams.py ties it to tests/pysort.py on a prefix, and the tiled expectations to the models on two tiles).

The constants below are mirrored from the kernels' launch sites; tests/test_bigstreams.py reads them back from the sources."""
import re
import struct
import zlib

import numpy as np

import pybam

GRID_CAP = 65535                                               # `65535u`: the most blocks a file-layer copy kernel is launched with
BLOCK = 256                                                    # `dim3(256)`
LANES_SHIFT = 4                                                # `>> 4`: 16 lanes per record
WAVE_SHIFT = 6                                                 # `>> 6`: one wave per record (the host's records / lines)
TRIP16 = (GRID_CAP * BLOCK) >> LANES_SHIFT                     # 1 048 560 records in one trip of a 16-lanes-per-record loop
TRIP64 = (GRID_CAP * BLOCK) >> WAVE_SHIFT                      # 262 140 records in one trip of a wave-per-record loop
INFLATE_LAUNCH = 1 << 18                                       # `(size_t)1 << 18`: members per launch of dev_inflate_members
WINDOW = 64 << 20                                              # the compressed bytes of a window at window_bytes=0
MEMBER = 0xff00

# kernel -> (source file, lanes per record); tests/test_bigstreams.py::test_constants_equal_the_sources walks this table
KERNELS = {
    "k_sort_gather": ("gce_sort.hpp", 16), "k_sort_scatter": ("gce_sort.hpp", 16), "k_md_body": ("gce_calmd.hpp", 16), "k_umi_body": ("gce_umi.hpp", 16),
    "k_samfmt_seq": ("gce_samfmt.hpp", 16), "k_sam_emit_seq": ("gce_samdev.hpp", 16), "k_pass_append": ("gce_passes.hpp", 16), "k_rec_build": ("gce_bamdev.hpp", 16),
    "k_merge_copy": ("gce_bamdev.hpp", 16), "k_samfmt_gather": ("gce_samfmt.hpp", 64), "k_samfmt_patch": ("gce_samfmt.hpp", 64), "k_sam_patch": ("gce_samdev.hpp", 64),
}


def launch_of(src, kernel):
    """(rounding, divisor, cap, block) of `hipLaunchKernelGGL(kernel, dim3(min((n + rounding) / divisor, cap)), dim3(block)` in src"""
    m = re.search(r"hipLaunchKernelGGL\(%s, dim3\(\(unsigned\)std::min<uint64_t>\(\(.+? \+ (\d+)\) / (\d+), (\d+)u\)\), dim3\((\d+)\)" % kernel, src)
    assert m, kernel
    return tuple(int(x) for x in m.groups())


def loop_of(src, kernel):
    """records per trip and per block of the kernel's grid-stride loop, from its start and its step:
    `(blockIdx.x * blockDim.x + threadIdx.x) >> a [<< b]` and `(gridDim.x * blockDim.x) >> a [<< b]` -> ((a, b) of the start, (a, b) of the step)"""
    body = src[src.index("void %s(" % kernel):]
    body = body[:body.index("\n}\n")]
    start = re.search(r"\(uint64_t\)blockIdx\.x \* blockDim\.x \+ threadIdx\.x\) >> (\d+)\)?(?: << (\d+))?", body)
    step = re.search(r"\(uint64_t\)gridDim\.x \* blockDim\.x\) >> (\d+)\)?(?: << (\d+))?", body)
    assert start and step, kernel
    return tuple(int(x or 0) for x in start.groups()), tuple(int(x or 0) for x in step.groups())


# ---------------------------------------------------------------- tiling
class Tiled:
    """K items (bytes) back to back, R times: .buf (uint8, writable), .starts (N + 1 offsets), .lens, .kind (the base item of every copy)"""

    def __init__(self, items, reps):
        self.items = [bytes(x) for x in items]
        self.K, self.R = len(self.items), int(reps)
        self.N = self.K * self.R
        self.item_len = np.array([len(x) for x in self.items], np.int64)
        self.buf = np.tile(np.frombuffer(b"".join(self.items), np.uint8), self.R)
        self.lens = np.tile(self.item_len, self.R)
        self.starts = np.zeros(self.N + 1, np.int64)
        np.cumsum(self.lens, out=self.starts[1:])
        self.kind = np.tile(np.arange(self.K), self.R)

    def per_item(self, x):
        """a value per base item (list of K) or one for all -> a value per copy"""
        x = np.asarray(x)
        return np.tile(x, self.R) if x.ndim else np.full(self.N, x)

    def put_digits(self, at, values=None, width=8):
        """`values` (default: the global index), zero-padded to `width` digits, at offset at[k] of every copy of item k (-1: not in this item)"""
        at = self.per_item(at).astype(np.int64)
        sel = np.nonzero(at >= 0)[0]
        where = self.starts[sel] + at[sel]
        v = sel if values is None else np.asarray(values, np.int64)[sel]
        assert v.size == 0 or (v.min() >= 0 and v.max() < 10 ** width)
        for d in range(width):
            self.buf[where + d] = 48 + (v // 10 ** (width - 1 - d)) % 10

    def put_i32(self, off, values, where=None):
        """a little-endian 32-bit value at offset `off` (one, or one per base item) of the copies in `where` (a mask; default all)"""
        sel = np.arange(self.N) if where is None else np.nonzero(where)[0]
        at = self.starts[sel] + self.per_item(off).astype(np.int64)[sel]
        v = np.ascontiguousarray(np.asarray(values, np.int64)[sel].astype("<i4")).view(np.uint8).reshape(-1, 4)
        for b in range(4):
            self.buf[at + b] = v[:, b]

    def get(self, off, dtype):
        """the little-endian field of `dtype` at offset `off` of every copy"""
        n = np.dtype(dtype).itemsize
        at = self.starts[:-1] + off
        raw = np.empty((self.N, n), np.uint8)
        for b in range(n):
            raw[:, b] = self.buf[at + b]
        return raw.view(dtype).reshape(-1)

    def head(self, n):
        """the first n copies, as views of this one's arrays"""
        import copy
        h = copy.copy(self)
        h.N, h.buf, h.lens, h.starts, h.kind = n, self.buf[:self.starts[n]], self.lens[:n], self.starts[:n + 1], self.kind[:n]
        return h


def reps_for(K, trip=TRIP16):
    """the fewest tiles whose second trip holds one whole block: K * R >= trip + K"""
    assert K % 2 == 1 and trip % K != 0, "K is odd and no divisor of the trip, so that tile borders never line up with the trip border"
    return -(-(trip + K) // K)


# ---------------------------------------------------------------- BAM records
ZEROS = b"00000000"


def with_name(rec, name):
    """the raw record (block_size first) under another read name (bytes, without its NUL)"""
    lq = rec[12]
    nm = name + b"\0"
    assert len(nm) <= 255
    body = rec[4:12] + bytes([len(nm)]) + rec[13:36] + nm + rec[36 + lq:]
    return struct.pack("<I", len(body)) + body


def digits_at(recs):
    """per raw record: 36 where its name begins with the eight zeros that take the index, else -1"""
    return [36 if r[12] >= 9 and r[36:44] == ZEROS else -1 for r in recs]


def stamp(t, at=None):
    """the global index into every copy: as digits in the name where the base record made room (`at`, default digits_at), as `mpos`
    (a fixed-width field that no rule here reads) in the records whose name is too short for it, the smallest legal record among them"""
    at = digits_at(t.items) if at is None else at
    t.put_digits(at)
    short = t.per_item(np.asarray(at) < 0)
    if short.any():
        t.put_i32(32, np.arange(t.N), where=short)
    return t


def size_residues(t, first=TRIP16):
    """the record sizes modulo 16 among the copies from index `first` on"""
    return set((t.lens[first:] % 16).tolist())


def write_bam(path, head, body, level=1, block=MEMBER):
    """header bytes and a record stream (bytes or uint8 array) as one BGZF file: members of `block` input bytes at zlib level `level`"""
    stream = np.concatenate([np.frombuffer(head, np.uint8), np.frombuffer(body, np.uint8) if isinstance(body, (bytes, bytearray)) else body])
    mv = memoryview(stream)
    with open(str(path), "wb") as f:
        for o in range(0, len(stream), block):
            f.write(pybam.bgzf_block(mv[o:o + block], level))
        f.write(pybam.EOF_BLOCK)


def first_difference(got, want):
    """None if the two byte strings / uint8 arrays are equal, else a few words on where they part"""
    a = np.frombuffer(got, np.uint8) if isinstance(got, (bytes, bytearray)) else got
    b = np.frombuffer(want, np.uint8) if isinstance(want, (bytes, bytearray)) else want
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    if len(d):
        return "first difference at byte %d of %d (%d bytes differ)" % (d[0], len(b), len(d))
    return None if len(a) == len(b) else "%d bytes, expected %d" % (len(a), len(b))


def record_at(starts, byte):
    """the record that holds stream byte `byte`"""
    return int(np.searchsorted(starts, byte, side="right")) - 1


# ---------------------------------------------------------------- the sort's model in numpy
def sort_keys(t, n_ref):
    """rule S's key of every copy of a Tiled of raw records: t << 33 | (pos + 1) << 1 | reverse, t = n_ref for unplaced records"""
    tid, pos, flag = t.get(4, "<i4"), t.get(8, "<i4"), t.get(18, "<u2")
    assert int(tid.max()) < n_ref
    tt = np.where(tid < 0, n_ref, tid).astype(np.uint64)
    return (tt << np.uint64(33)) | (((pos.astype(np.int64) + 1) & 0xFFFFFFFF).astype(np.uint64) << np.uint64(1)) | ((flag >> 4) & 1).astype(np.uint64)


def descents(keys):
    return int(np.count_nonzero(keys[1:] < keys[:-1]))


def gather(buf, starts, lens, order, chunk=1 << 16):
    """the items in `order`, back to back (uint8 array)"""
    ln = lens[order]
    out = np.empty(int(ln.sum()), np.uint8)
    o = 0
    for a in range(0, len(order), chunk):
        l = ln[a:a + chunk]
        n = int(l.sum())
        dst = np.zeros(len(l), np.int64)
        np.cumsum(l[:-1], out=dst[1:])
        out[o:o + n] = buf[np.repeat(starts[order[a:a + chunk]] - dst, l) + np.arange(n)]
        o += n
    return out


def sorted_stream(t, n_ref):
    """-> (order: input index per output slot, the sorted record stream, keys in input order)"""
    keys = sort_keys(t, n_ref)
    order = np.argsort(keys, kind="stable")
    return order, gather(t.buf, t.starts, t.lens, order), keys


# ---------------------------------------------------------------- a base block for the sort
SORT_TARGETS = [("a", 300000), ("b", 300000), ("c", 300000), ("d", 5000)]


def sort_block(K=2003):
    """K raw records: names of 8 digits and 0..15 more bytes against 0, 1, 3, 6 and 9 bases (every size modulo 16), both strands, an
    unplaced record in every 50; record 0 is the smallest legal record (38 bytes), record K // 2 one of 3000 bases (4.5 KB)"""
    recs = []
    for k in range(K):
        L = (0, 1, 3, 6, 9)[k % 5]
        r = dict(qname="00000000" + "abcdefghijklmno"[:k % 16], flag=16 if k % 3 == 0 else 0, tid=0, pos=0, mapq=60, cigar="%dM" % L if L else "*", mtid=-1, mpos=-1, isize=0,
                 seq="ACGT"[k % 4] * L, qual=[20 + k % 20] * L)
        if k % 50 == 7:
            r.update(tid=-1, pos=-1, flag=4 | (16 if k % 100 == 7 else 0))
        if k == 0:
            r.update(qname="s", cigar="*", seq="", qual=[])
        if k == K // 2:
            r.update(cigar="3000M", seq="ACGTTGCA" * 375, qual=[(7 * q) % 41 for q in range(3000)])
        recs.append(pybam.record_bytes(r))
    return recs


def sort_stream(K=2003, P=7919, M=1021, n_passes=3):
    """the sort tests' input: sort_block tiled past one trip and stamped; pos = (i * P) mod M (M far below N: hundreds of ties per key, so
    stability shows); of the placed records, those of the second trip lie on contig 1 and those of the first on contigs 0 and 2, split so
    that the first cut of a sort in `n_passes` output-range passes falls among the second trip's records.  Unplaced records stay unplaced.
    -> (Tiled, header bytes)"""
    base = sort_block(K)
    t = stamp(Tiled(base, reps_for(K)))
    i = np.arange(t.N)
    placed = t.get(4, "<i4") >= 0
    total = int(t.starts[-1])
    pass_bytes = (-(-total // n_passes) + MEMBER - 1) // MEMBER * MEMBER
    second = placed & (i >= TRIP16)
    cum = np.cumsum(np.where(placed & (i < TRIP16), t.lens, 0))
    t0 = int(np.searchsorted(cum, pass_bytes - int(t.lens[second].sum()) // 2))
    t.put_i32(4, np.where(i >= TRIP16, 1, np.where(i < t0, 0, 2)), where=placed)
    t.put_i32(8, (i * P) % M, where=placed)
    import test_bai_model
    return t, test_bai_model.header(SORT_TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n")


# ---------------------------------------------------------------- the inflater's members
def member_pool(n=61):
    """n distinct small BGZF members, payloads of 0..400 bytes, stored, fixed and dynamic blocks -> (members, payloads, block types)"""
    from inflate_helpers import member
    rng = np.random.default_rng(61)
    text = b"".join(b"read%d\t99\tchr1\t%d\t60\t150M\t=\t%d\t300\n" % (i, 1000 + 7 * i, 1200 + i) for i in range(40))
    members, datas, types = [], [], []
    for k in range(n):
        size = (k * 400) // (n - 1)
        way = k % 6
        if way in (0, 3):
            d = bytes(rng.integers(0, 256, size, dtype=np.uint8))                                  # does not compress: stored at level 0, and what zlib chooses at 6
        elif way in (1, 4):
            d = (text[k:] + text)[:size]
        else:
            d = bytes(np.minimum(rng.geometric(0.35, size), 11).astype(np.uint8) + 64)              # a skewed alphabet: worth a code of its own
        level, strategy = [(0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY)][way]
        m = member(d, level, strategy)
        members.append(m); datas.append(d); types.append((m[18] >> 1) & 3)
    return members, datas, types


# ---------------------------------------------------------------- calmd: the records of calmdcases on a periodic reference
CALMD_PERIOD = 100                                             # two units of calmdcases.CHR1, 25 of "ACGT": a shift by it keeps every NM and MD
CALMD_UNITS = 1000


def calmd_reference():
    """-> (targets, {contig name: bases}, FASTA text): calmdcases' contigs, each repeated to CALMD_PERIOD * CALMD_UNITS bases; the header's
    third contig stays out of the FASTA"""
    import calmdcases as cc
    n = CALMD_PERIOD * CALMD_UNITS
    fasta = {"chr1": (cc.CHR1 * (n // len(cc.CHR1))).encode(), "chr2": ("ACGT" * (n // 4)).encode()}
    text = "".join(">%s\n" % nm + "".join(s[k:k + 80].decode() + "\n" for k in range(0, n, 80)) for nm, s in fasta.items())
    return [("chr1", n), ("chr2", n), ("missing", 1000)], fasta, text


def calmd_block(copies=8):
    """calmdcases' file records below 1 KB (hand vectors, every tag layout: NM / MD that grow, shrink or are absent; the ineligible records,
    which pass through; 16 name lengths against four layouts), each under a name of eight zeros and its own, `copies` times over with a
    letter between the two; one record with an insertion of 3000 bases (4.6 KB, its NM needs an S field); the smallest legal record.  K is odd and no divisor of the trip."""
    import calmdcases as cc
    small = [r for r in cc.file_records() if len(r) < 1000]
    recs = [with_name(r, ZEROS + b"abcdefghijklmnop"[c:c + 1] + r[36:36 + r[12]].split(b"\0")[0]) for c in range(copies) for r in small]
    recs.insert(len(recs) // 2, cc.record(0, 0, "5M3000I5M", "ACGTA" + "T" * 3000 + "CGTCA", aux=cc.nm("C", 7), qname="00000000big"))
    recs.insert(0, cc.record(-1, -1, "", "", flag=4, qname="s"))
    if len(recs) % 2 == 0 or TRIP16 % len(recs) == 0:
        recs.append(recs[1])
    return recs


def shift_positions(t, period=CALMD_PERIOD, units=CALMD_UNITS - 10):
    """pos += period * (a scramble of the global index), in the copies of base records that are placed at pos >= 0 (a record at a negative
    pos has bases in front of the contig: a shift would change what it is compared with)"""
    i = np.arange(t.N)
    pos = t.get(8, "<i4")
    where = (t.get(4, "<i4") >= 0) & (pos >= 0)
    t.put_i32(8, pos.astype(np.int64) + period * ((i * 7919) % units), where=where)
    return t


# ---------------------------------------------------------------- the UMI pass: the records of umicases
def umi_block(copies=11):
    """umicases' records of both sources whose name leaves room for eight digits in front of it, those above 200 bytes left out but for
    big_record(4000) (a 4 KB B array between two dropped MI fields), `copies` times over, and the smallest legal record.  The digits stand
    first in the name: the name rule reads behind the last colon, the tag rule not at all."""
    import umicases as uc
    small = [c[2] for c in uc.all_cases() if len(c[2]) <= 200 and c[2][12] + 9 <= 255]
    recs = [with_name(r, ZEROS + b"abcdefghijklmnop"[c:c + 1] + r[36:36 + r[12] - 1]) for c in range(copies) for r in small]
    recs.insert(len(recs) // 2, with_name(uc.big_record(4000)[0], ZEROS + b"big:ACGT+TTGA"))
    recs.insert(0, uc.rec(qname="s", nm=None, cigar="*", seq="", flag=4, tid=-1, pos=-1, mtid=-1, mpos=-1, isize=0))
    if len(recs) % 2 == 0 or TRIP16 % len(recs) == 0:
        recs.append(recs[1])
    return recs


# ---------------------------------------------------------------- SAM text and its records, both from samcases.case
def sam_block(K=1001):
    """K cases of samcases.case -> (lines with their line feed, records, host flags): names of eight zeros and 0..15 more bytes, 0..22 bases
    (one case of 3000), both strands, unplaced and unmapped records, mates on the same and on another contig, integer, string and array
    fields; two cases in seven carry an f, d or B:f field in the form %g prints it (so that the text is the line of the record and the record
    the parse of the text), which is more than the 27 % that put the host's share of N records above one trip of the wave-per-record kernels"""
    import samcases
    a = pybam.aux_bytes
    floats = [("XF:f:3.14159", b"XFf" + struct.pack("<f", 3.14159), True), ("XD:d:-1e-300", b"XDd" + struct.pack("<d", -1e-300), True),
              ("XB:B:f,0.1,-2.5,1.5e+10", a("XB", "B", ("f", [0.1, -2.5, 1.5e10])), True)]
    lines, recs, host = [], [], []
    for k in range(K):
        n = (k * 7) % 23
        kw = dict(qname="00000000" + "abcdefghijklmno"[:k % 16], n=n, pos=1 + (k * 37) % 900000, flag=16 if k % 3 == 0 else 0, mapq=k % 61)
        aux = [("NM:i:%d" % (k % 200), a("NM", "C", k % 200), False)]
        if k % 5 == 1:
            aux.append(("XZ:Z:tile%d" % (k % 13), a("XZ", "Z", "tile%d" % (k % 13)), False))
        if k % 11 == 2:
            aux.append(("XS:B:s,-300,7", a("XS", "B", ("s", [-300, 7])), False))
        if k % 7 in (0, 3):
            aux.insert(k % 2, floats[(k // 7) % 3])
        if k % 9 == 4:
            kw.update(rname="chr2", rnext="=", pnext=500 + k, tlen=(-1) ** k * 300, flag=kw["flag"] | 1)
        if k % 9 == 5:
            kw.update(rname="chr10", rnext="chrM", pnext=77, flag=kw["flag"] | 1)
        if k % 50 == 7:
            kw.update(rname="*", pos=0, flag=4 | kw["flag"], cigar="*", mapq=0, rnext="*", pnext=0, tlen=0)
        if k % 50 == 8 or n == 0:
            kw.update(seq="*", qual="*", cigar="*", flag=4 | kw["flag"], n=0)
        if k % 50 == 9:
            kw.update(qual="*")
        if k == 0:
            kw, aux = dict(qname="00000000", seq="*", qual="*", cigar="*", flag=4, rname="*", pos=0, mapq=0), []      # the smallest line and record with room for the index
        if k == K // 2:
            kw.update(n=3000)
        line, rec, h = samcases.case(aux=aux, **kw)
        lines.append(line.encode() + b"\n"); recs.append(rec); host.append(h)
    return lines, recs, host
