"""The file layer's copy kernels past one grid.  Every "16 lanes per record" kernel of the file layer is launched with at most 65 535 blocks
of 256 threads and walks its records in a grid-stride loop: one trip holds 1 048 560 records (bigstreams.TRIP16), the wave-per-record
kernels of the SAM paths 262 140 (bigstreams.TRIP64).  A default window of 64 MB of compressed BAM holds more than that, so production
takes the second trip on every window, and no other test here builds a stream that reaches it.  These tests do, with the streams of
tests/bigstreams.py: a base block of K records (K odd, no divisor of the trip; every record size modulo 16, the smallest legal record, one
of several KB, unplaced records, both strands) tiled to N >= 1 048 560 + K records and stamped with its global index, so that the second
trip holds a whole block and a record left uncopied, or copied to the wrong place, shows.  Each test asserts its premise first: N records
above the trip reach the kernel in one launch (for the windowed runners: the file is smaller than the 64 MB piece, so one window holds
them all), and the records behind index 1 048 560 cover all 16 size residues.  The caps are mirrored in bigstreams.py and read back from
the sources by tests/test_bigstreams.py, so these tests move with the kernels.  The three tests of the engine's file writers take
outcases' "large:1025_tiles" instead of a tiled block (its oracle table is computed once for this and for tests/test_output_table_gpu.py):
3.8 M output records of 48, 52 and 56 bytes.

Measured on an MI355X, test body / module fixture, in seconds: test_sort_in_core 0.53 / 0.83, test_sort_in_passes 0.56, test_calmd 0.34 / 0.62,
test_umi_pass 0.38 and 0.36 / 0.34, test_bam_to_sam_in_one_call 0.29 / 0.11, test_sam_to_bam_in_one_call 0.15,
test_run_bam_writes_the_oracles_records 0.99 / 0.97, test_sharded_run_merges_the_single_pass_records 0.50,
test_key_range_passes_append_the_single_pass_records 0.90; the module takes 8.4 s.  The CPU side alone (build the input and the
expectation, inflate a file of the output's size with zlib, compare) takes on a build machine without a GPU: sort 2.1 + 0.8 s,
calmd 1.6 + 1.0 s, UMI 1.0 + 0.8 s, SAM 0.4 + 0.2 s, the engine's case, oracle table and rows 2.2 s; so no test spends more in the runner
than in building and checking its streams, and none was shrunk.  The streams of calmd, the UMI pass and SAM are 90-107 MB inflated, not
the 60-80 MB of the sort's: their case records carry optional fields and average 87-102 bytes.

Out of reach for a test of seconds, and not faked here: k_deflate_pack (16 384 blocks of four members: a second trip needs about 4 GB of
output) and the second round of k_scan_partials (more than 16.7 M scan elements)."""
import os

import numpy as np
import pytest

import bigstreams as bs
import pysort

pytestmark = pytest.mark.gpu


def one_window(path):
    """premise of the windowed runners: the whole file is one piece of window_bytes=0"""
    assert os.path.getsize(str(path)) < bs.WINDOW
    return True


def inflated(path):
    blob = open(str(path), "rb").read()
    assert blob.endswith(pysort.EOF_BLOCK)
    return np.frombuffer(pysort.inflate(blob), np.uint8)


# ---------------------------------------------------------------- a, b: the sort
class SortCase:
    def __init__(self, d):
        self.d = d
        self.t, head = bs.sort_stream()
        self.path = d / "big.bam"
        bs.write_bam(self.path, head, self.t.buf)
        self.n_ref = len(bs.SORT_TARGETS)
        self.head = pysort.header_bytes(pysort.split(head)[0])   # rule H
        self.order, self.stream, self.keys = bs.sorted_stream(self.t, self.n_ref)
        self.want = np.concatenate([np.frombuffer(self.head, np.uint8), self.stream])
        self.n_unplaced = int((self.t.get(4, "<i4") < 0).sum())
        for a in (self.t.buf, self.order, self.stream, self.keys, self.want):
            a.flags.writeable = False

    def premise(self):
        t = self.t
        assert t.N > bs.TRIP16 and one_window(self.path)
        assert bs.size_residues(t) == set(range(16))
        tid, flag = t.get(4, "<i4")[bs.TRIP16:], t.get(18, "<u2")[bs.TRIP16:]
        assert (tid < 0).any() and (tid >= 0).any() and {0, 16} <= set((flag & 16).tolist())     # unplaced records and both strands in the second trip
        assert len(np.unique(self.keys)) < t.N // 100                                            # ties everywhere: the order within a key is the input's

    def check_counters(self, r):
        assert (r["n_records"], r["n_no_coor"], r["n_descents"]) == (self.t.N, self.n_unplaced, bs.descents(self.keys))
        assert r["inflated_bytes"] == int(self.t.starts[-1])


@pytest.fixture(scope="module")
def sortcase(built, tmp_path_factory):
    return SortCase(tmp_path_factory.mktemp("trip_sort"))


def test_sort_in_core(sortcase):
    """k_sort_gather (gce_sort.hpp): sort_bam gathers all N > 1 048 560 records of the file in one launch; the inflated output is rule H's
    header and the records in the order of the numpy model (bigstreams.sorted_stream, tied to pysort on the CPU), the counters are the model's."""
    from gencore_amd.bamio import sort_bam
    c = sortcase
    c.premise()
    out = c.d / "incore.bam"
    r = sort_bam(str(c.path), str(out), device=0, threads=4, level=-2, window_bytes=0)
    got = inflated(out)
    assert bs.first_difference(got, c.want) is None, bs.first_difference(got, c.want)
    c.check_counters(r)
    assert r["out_bytes"] == os.path.getsize(str(out))


def test_sort_in_passes(sortcase):
    """k_sort_scatter (gce_sort.hpp): with window_bytes=0 the one window of each of three output-range passes holds all N > 1 048 560
    records, four to a wave; records of the second trip straddle the first cut, so the clipped copies run there too.  The file equals the
    in-core sort's byte for byte (made here, not taken from the test above) and its inflated stream is the model's."""
    from gencore_amd.bamio import sort_bam, sort_bam_passes
    c = sortcase
    c.premise()
    total = int(c.t.starts[-1])
    pass_bytes = (-(-total // 3) + bs.MEMBER - 1) // bs.MEMBER * bs.MEMBER
    dst = np.zeros(c.t.N + 1, np.int64)
    np.cumsum(c.t.lens[c.order], out=dst[1:])
    cuts = list(range(pass_bytes, total, pass_bytes))
    assert len(cuts) == 2
    straddlers = [int(c.order[bs.record_at(dst, x)]) for x in cuts if dst[np.searchsorted(dst, x)] != x]     # (a cut on a record border cuts no record)
    assert any(i >= bs.TRIP16 for i in straddlers), straddlers   # an input record behind the trip border is written partly by two passes
    ref, out = c.d / "ref.bam", c.d / "passes.bam"
    sort_bam(str(c.path), str(ref), device=0, threads=4, level=-2, window_bytes=0)
    r = sort_bam_passes(str(c.path), str(out), device=0, threads=4, level=-2, window_bytes=0, min_passes=3)
    assert (r["n_passes"], r["pass_bytes"], r["in_core"]) == (3, pass_bytes, 0)
    blob = out.read_bytes()
    assert blob == ref.read_bytes()
    got = inflated(out)
    assert bs.first_difference(got, c.want) is None, bs.first_difference(got, c.want)
    c.check_counters(r)


# ---------------------------------------------------------------- c, d: the per-record rewriters
class RewriteCase:
    """a base block, tiled and patched, as a BAM file; and the model's records for the base block, tiled and patched the same way"""

    def __init__(self, path, head, base, new, patch):
        self.path, self.head = path, head
        R = bs.reps_for(len(base))
        self.t = patch(bs.stamp(bs.Tiled(base, R)))
        bs.write_bam(path, head, self.t.buf)
        w = patch(bs.stamp(bs.Tiled(new, R)))
        self.want_bytes = int(w.starts[-1])
        self.want = np.concatenate([np.frombuffer(head, np.uint8), w.buf])
        self.R = R
        for a in (self.t.buf, self.want):
            a.flags.writeable = False

    def premise(self):
        assert self.t.N > bs.TRIP16 and self.t.N - bs.TRIP16 >= self.t.K and one_window(self.path)
        assert bs.size_residues(self.t) == set(range(16))


@pytest.fixture(scope="module")
def calmdcase(built, tmp_path_factory):
    import pycalmd
    from test_bai_model import header
    d = tmp_path_factory.mktemp("trip_calmd")
    targets, fasta, text = bs.calmd_reference()
    (d / "ref.fa").write_text(text)
    base = bs.calmd_block()
    new, counters = pycalmd.calmd_records(base, [t[0] for t in targets], fasta)
    c = RewriteCase(d / "big.bam", header(targets, text="@HD\tVN:1.6\tSO:unsorted\n"), base, new, bs.shift_positions)
    c.d, c.counters = d, counters
    return c


def test_calmd(calmdcase):
    """k_md_body (gce_calmd.hpp): calmd_bam rewrites the bodies of all N > 1 048 560 records of the one window in one launch.  The reference
    has a period of 100 bases and every copy of a base record lies a multiple of it further on, so the expected file is pycalmd's output
    on the base block, tiled, stamped and shifted (tests/test_bigstreams.py runs the model record by record on two tiles); the block holds
    records whose NM / MD grow, shrink and are absent, and the ineligible ones, which pass through."""
    from gencore_amd.bamio import calmd_bam
    c = calmdcase
    c.premise()
    out = c.d / "out.bam"
    r = calmd_bam(str(c.path), str(out), str(c.d / "ref.fa"), device=0, threads=4, level=-2, window_bytes=0)
    got = inflated(out)
    assert bs.first_difference(got, c.want) is None, bs.first_difference(got, c.want)
    assert {k: getattr(r, k) for k in c.counters} == {k: v * c.R for k, v in c.counters.items()}
    assert r.out_record_bytes == c.want_bytes and r.inflated_bytes == int(c.t.starts[-1])


@pytest.fixture(scope="module")
def umicase(built, tmp_path_factory):
    import umicases as uc
    from test_bai_model import header
    d = tmp_path_factory.mktemp("trip_umi")
    base = bs.umi_block()
    t = bs.stamp(bs.Tiled(base, bs.reps_for(len(base))))
    head = header(uc.TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n")
    bs.write_bam(d / "big.bam", head, t.buf)
    t.buf.flags.writeable = False
    return d, base, t, head


@pytest.mark.parametrize("source", ["RX", "name"])
def test_umi_pass(umicase, source):
    """k_umi_body (gce_umi.hpp): umi_to_mi rewrites the bodies of all N > 1 048 560 records of the one window in one launch (no flush: the
    file is one window), with the UMI taken from RX and from the read name; the index digits stand first in the name, where neither rule
    reads.  The expected file is pyumi's output on the base block, tiled and stamped."""
    import pyumi
    from gencore_amd.bamio import umi_to_mi
    d, base, t, head = umicase
    assert t.N > bs.TRIP16 and t.N - bs.TRIP16 >= t.K and one_window(d / "big.bam") and bs.size_residues(t) == set(range(16))
    new, counters = pyumi.umi_records(base, source)
    w = bs.stamp(bs.Tiled(new, t.R))
    out = d / ("out_%s.bam" % source)
    r = umi_to_mi(str(d / "big.bam"), str(out), source=source, device=0, threads=4, level=-2, window_bytes=0)
    assert r.n_flushes == 0
    got = inflated(out)
    want = np.concatenate([np.frombuffer(head, np.uint8), w.buf])
    assert bs.first_difference(got, want) is None, bs.first_difference(got, want)
    assert {k: getattr(r, k) for k in counters} == {k: v * t.R for k, v in counters.items()}
    assert r.out_record_bytes == int(w.starts[-1]) and r.inflated_bytes == int(t.starts[-1])


# ---------------------------------------------------------------- e, f: SAM text in one call
@pytest.fixture(scope="module")
def samcase(built):
    """(records, text): the SAM block's records and lines, tiled and stamped; both from samcases.case, neither from the code under test"""
    lines, recs, host = bs.sam_block()
    R = bs.reps_for(len(recs))
    tr = bs.stamp(bs.Tiled(recs, R))
    tl = bs.Tiled(lines, R)
    tl.put_digits(0)
    n_host = sum(host) * R
    for a in (tr.buf, tl.buf):
        a.flags.writeable = False
    assert tr.N > bs.TRIP16 and n_host > bs.TRIP64 and bs.size_residues(tr) == set(range(16))
    assert sum(host[k] for k in tr.kind[bs.TRIP16:]) > 0 and n_host - bs.TRIP64 > sum(host)       # host records in the second trip of either grouping
    return tr, tl, n_host


def test_bam_to_sam_in_one_call(samcase):
    """k_samfmt_seq (16 lanes per record, N > 1 048 560 records) and k_samfmt_gather / k_samfmt_patch (a wave per record of the host's,
    more than 262 140 of them: the records with an f, d or B:f field) of gce_samfmt.hpp, in the one launch each that format_sam makes."""
    from gencore_amd.bamio import format_sam, sam_format_counters
    from samfmtcases import NAMES
    tr, tl, n_host = samcase
    before = sam_format_counters()
    r = format_sam(tr.buf, NAMES, out_cap=len(tl.buf))
    after = sam_format_counters()
    assert after[1] - before[1] == n_host > bs.TRIP64 and after[0] - before[0] == tr.N - n_host and after[2] - before[2] == 1
    assert (r["n_records"], r["n_host_records"]) == (tr.N, n_host)
    assert bs.first_difference(r["text"], tl.buf) is None, bs.first_difference(r["text"], tl.buf)


def test_sam_to_bam_in_one_call(samcase):
    """k_sam_emit_seq (16 lanes per line, N > 1 048 560 lines) and k_sam_patch (a wave per line of the host's, more than 262 140) of
    gce_samdev.hpp, in the one launch each that parse_sam makes: the text of the test above back into its records."""
    from gencore_amd.bamio import parse_sam
    from samfmtcases import NAMES
    tr, tl, n_host = samcase
    r = parse_sam(tl.buf, NAMES, out_cap=len(tr.buf))
    assert (r["n_records"], r["n_host_lines"]) == (tr.N, n_host) and n_host > bs.TRIP64
    assert bs.first_difference(r["records"], tr.buf) is None, bs.first_difference(r["records"], tr.buf)


# ---------------------------------------------------------------- g: the engine's file writers
def record_stream(path):
    """the inflated record stream of a BAM file (uint8 array), its header cut off"""
    import struct
    u = inflated(path)
    lt = struct.unpack_from("<i", u, 4)[0]
    o = 8 + lt
    nref = struct.unpack_from("<i", u, o)[0]; o += 4
    for _ in range(nref):
        o += 4 + struct.unpack_from("<i", u, o)[0] + 4
    return u[o:]


class EngineCase:
    """outcases' "large:1025_tiles" (4.2 M reads of one base under one-letter names, 3.8 M of them emitted; the oracle's table of it is shared
    with tests/test_output_table_gpu.py) as a BAM file, and the single-pass run's records, made once"""

    def __init__(self, d):
        import outcases
        from gencore_amd.bamio import run_bam, write_batch_as_bam
        self.d, self.c = d, outcases.get("large:1025_tiles")
        self.want = outcases.oracle_result("large:1025_tiles")
        assert self.want.status == 0
        self.path = d / "in.bam"
        write_batch_as_bam(str(self.path), self.c.batch, np.asarray(self.c.contig_len, np.uint32), threads=4)
        self.n_out = int((self.want.out_flag != 0).sum())
        self.run = run_bam(str(self.path), str(d / "one.bam"), self.c.params(), threads=4, chunk_reads=1 << 23, level=-2)
        self.one = record_stream(d / "one.bam")

    def premise(self):
        assert self.n_out > bs.TRIP16 and self.c.batch.n <= 1 << 23 and one_window(self.path)


@pytest.fixture(scope="module")
def enginecase(built, tmp_path_factory):
    return EngineCase(tmp_path_factory.mktemp("trip_engine"))


def test_run_bam_writes_the_oracles_records(enginecase):
    """k_rec_build (gce_bamdev.hpp): run_bam with all reads in one chunk builds its 3.8 M > 1 048 560 output records in one launch.  Every
    record of the file, in the table's order (outcases.rows_from_table), carries what the oracle's table says, as
    tests/test_bamio.py::test_bam_end_to_end compares it: name, flag, contig, position, mate fields, bases, qualities, NM, FR and RR; the
    records here have one base, a one-letter name and NM:C, so a record is 48 bytes plus 4 per FR / RR field and its fields lie at fixed
    offsets, which the block sizes confirm."""
    import outcases
    e = enginecase
    e.premise()
    b, w = e.c.batch, e.want
    rows = outcases.rows_from_table(b, w)
    src = rows["src"].astype(np.int64)
    assert len(src) == e.n_out == e.run.n_out and e.run.n_reads == b.n
    core = b.core[src]
    assert (core["l_qseq"] == 1).all() and (core["l_qname"] == 2).all() and (b.nm_type[src] == ord("C")).all()
    fr, rr = w.fr[src].astype(np.int64), w.rr[src].astype(np.int64)
    size = 48 + 4 * (fr >= 0) + 4 * (rr >= 0)
    start = np.cumsum(size) - size
    u = e.one
    assert len(u) == int(size.sum())
    field = lambda off, dt: np.stack([u[start + off + k] for k in range(np.dtype(dt).itemsize)], 1).copy().view(dt).reshape(-1)
    assert np.array_equal(field(0, "<u4"), size - 4)                                            # block_size: so every start is a record's
    for name, off, dt in (("tid", 4, "<i4"), ("pos", 8, "<i4"), ("flag", 18, "<u2"), ("mtid", 24, "<i4"), ("mpos", 28, "<i4"), ("isize", 32, "<i4")):
        assert np.array_equal(field(off, dt), core[name].astype(dt)), name
    assert np.array_equal(u[start + 12], np.full(len(src), 2)) and np.array_equal(field(16, "<u2"), np.ones(len(src), "<u2")) and np.array_equal(field(20, "<i4"), np.ones(len(src), "<i4"))
    qs = w.qname_src[src].astype(np.int64)
    assert np.array_equal(u[start + 36], b.qname[b.qname_off[qs].astype(np.int64)]) and not u[start + 37].any()
    assert np.array_equal(field(38, "<u4"), np.full(len(src), 1 << 4, "<u4"))                    # 1M
    assert np.array_equal(u[start + 42], w.seq[b.seq_off[src].astype(np.int64)] & 0xF0)
    assert np.array_equal(u[start + 43], w.qual[b.qual_off[src].astype(np.int64)])
    nm = np.where(w.nm_new[src] >= 0, w.nm_new[src], b.nm[src])
    assert bytes(u[start[0] + 44:start[0] + 47]) == b"NMC" and np.array_equal(field(44, "<u4") & 0xFFFFFF, np.full(len(src), 0x434D4E, "<u4")) and np.array_equal(u[start + 47], nm.astype(np.uint8))
    has_fr, has_rr = np.nonzero(fr >= 0)[0], np.nonzero(rr >= 0)[0]
    assert len(has_fr) > 0
    tag = lambda t: int.from_bytes(t, "little")
    at_fr = start[has_fr] + 48
    assert np.array_equal(u[at_fr] | (u[at_fr + 1].astype(np.int64) << 8), np.full(len(has_fr), tag(b"FR"))) and np.array_equal(u[at_fr + 3], (fr[has_fr] & 0xFF).astype(np.uint8))
    at_rr = start[has_rr] + 48 + 4 * (fr[has_rr] >= 0)
    assert np.array_equal(u[at_rr] | (u[at_rr + 1].astype(np.int64) << 8), np.full(len(has_rr), tag(b"RR"))) and np.array_equal(u[at_rr + 3], (rr[has_rr] & 0xFF).astype(np.uint8))
    assert bytes(e.run.pre) == bytes(w.pre) and bytes(e.run.post) == bytes(w.post)          # (record sizes here are 48, 52 and 56: the case is the engine's own, not a tiled block)


def test_sharded_run_merges_the_single_pass_records(enginecase):
    """k_merge_copy (gce_bamdev.hpp): run_bam_sharded on two engines of one device merges the shards' 3.8 M > 1 048 560 records in one
    launch (and each shard builds more than one trip's worth with k_rec_build); the record stream is the single-pass run's."""
    from gencore_amd.bamio import run_bam_sharded
    e = enginecase
    e.premise()
    assert e.n_out // 2 > bs.TRIP16
    r = run_bam_sharded(str(e.path), str(e.d / "sharded.bam"), e.c.params(), [0, 0], threads=4, level=-2)
    assert r.n_out == e.n_out and r.n_reads == e.c.batch.n
    got = record_stream(e.d / "sharded.bam")
    assert bs.first_difference(got, e.one) is None, bs.first_difference(got, e.one)
    assert bytes(r.pre) == bytes(e.run.pre) and bytes(r.post) == bytes(e.run.post)


def test_key_range_passes_append_the_single_pass_records(enginecase):
    """k_pass_append (gce_passes.hpp): run_bam_passes in two forced passes with window_bytes=0: the one window of each pass holds that pass's
    selected records, more than 1 048 560 of them in either pass; the record stream is the single-pass run's."""
    from gencore_amd.bamio import run_bam_passes
    e = enginecase
    e.premise()
    r, _, pr = run_bam_passes(str(e.path), str(e.d / "passes.bam"), e.c.params(), 0, threads=4, level=-2, min_passes=2, window_bytes=0)
    assert pr["n_passes"] == 2 and not pr["single_pass"] and min(pr["reads_per_pass"]) > bs.TRIP16 and sum(pr["reads_per_pass"]) == e.c.batch.n
    assert r.n_out == e.n_out
    got = record_stream(e.d / "passes.bam")
    assert bs.first_difference(got, e.one) is None, bs.first_difference(got, e.one)
    assert bytes(r.pre) == bytes(e.run.pre) and bytes(r.post) == bytes(e.run.post)
