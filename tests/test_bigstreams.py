"""tests/bigstreams.py without a GPU: its constants equal the kernels' sources, its numpy sort model equals tests/pysort.py byte for byte on a
5 000-record prefix of the stream the GPU test sorts, and its tiled expectations of calmd, the UMI pass and the two SAM directions equal the
Python models run record by record on a two-tile stream."""
import os
import re

import numpy as np

import bigstreams as bs
import pysort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gencore_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_equal_the_sources():
    """every kernel of bigstreams.KERNELS is launched with min(ceil(n / records per block), 65535) blocks of 256 threads, and its loop starts
    and steps by the same grouping: so one trip holds TRIP16 (16 lanes per record) or TRIP64 (a wave per record) records; the inflater's
    launch takes 2^18 members"""
    assert bs.TRIP16 == 1048560 and bs.TRIP64 == 262140
    for kernel, (name, lanes) in bs.KERNELS.items():
        src = source(name)
        rounding, divisor, cap, block = bs.launch_of(src, kernel)
        assert (cap, block) == (bs.GRID_CAP, bs.BLOCK), kernel
        assert divisor == block // lanes and rounding == divisor - 1, kernel
        start, step = bs.loop_of(src, kernel)
        assert start == step, kernel
        per_trip = ((cap * block) >> start[0]) << start[1]
        assert per_trip == (bs.TRIP16 if lanes == 16 else bs.TRIP64), kernel
        if lanes == 16 and start[1] == 0:
            assert start[0] == bs.LANES_SHIFT, kernel
        elif lanes == 16:
            assert start == (bs.WAVE_SHIFT, bs.WAVE_SHIFT - bs.LANES_SHIFT), kernel            # k_sort_scatter: four records per wave
        else:
            assert start == (bs.WAVE_SHIFT, 0), kernel
    m = re.search(r"const size_t LAUNCH = \(size_t\)1 << (\d+);", source("gce_devstream.hpp"))
    assert m and 1 << int(m.group(1)) == bs.INFLATE_LAUNCH
    for name in ("bamio_sort.hpp", "bamio_index.hpp", "bamio_reduce.hpp", "bamio_passes.hpp"):
        m = re.search(r"rd\.piece = window_bytes > 0 \? (?:\(size_t\))?window_bytes : \(\(size_t\)(\d+) << (\d+)\);", source(name))
        assert m and int(m.group(1)) << int(m.group(2)) == bs.WINDOW, name


def test_sort_stream_is_what_the_gpu_test_needs():
    """the shape of the sort tests' input, checked where it is cheap: more than one trip, every size residue, unplaced records and both
    strands behind the trip border, no two records equal"""
    t, head = bs.sort_stream()
    assert t.N >= bs.TRIP16 + t.K and t.K % 2 == 1 and bs.TRIP16 % t.K != 0
    assert bs.size_residues(t) == set(range(16))
    assert int(t.lens.min()) == 38 and int(t.lens.max()) > 4000 and t.lens.mean() <= 66
    tid, flag = t.get(4, "<i4")[bs.TRIP16:], t.get(18, "<u2")[bs.TRIP16:]
    assert (tid < 0).any() and (tid == 1).any() and {0, 16} <= set((flag & 16).tolist())
    names = t.buf[(t.starts[:-1] + 36)[:, None] + np.arange(8)]
    mpos = t.get(32, "<i4")
    short = np.asarray(bs.digits_at(t.items))[t.kind] < 0
    idx = np.where(short, mpos, (names - 48).astype(np.int64) @ (10 ** np.arange(7, -1, -1)))
    assert np.array_equal(idx, np.arange(t.N))


def test_numpy_sort_model_equals_pysort_on_a_prefix(tmp_path):
    t, head = bs.sort_stream()
    n = 5000
    path = tmp_path / "prefix.bam"
    p = t.head(n)
    bs.write_bam(path, head, p.buf)
    want_head, want = pysort.sort_model(path)
    order, stream, keys = bs.sorted_stream(p, len(bs.SORT_TARGETS))
    assert stream.tobytes() == b"".join(want)
    assert bs.descents(keys) == pysort.descents(path) > 1000
    hdr = pysort.split(head)[0]
    assert pysort.header_bytes(hdr) == want_head
    assert len(set(keys.tolist())) < n // 2                      # ties: stability decides


def records_of(t):
    return [t.buf[a:z].tobytes() for a, z in zip(t.starts[:-1], t.starts[1:])]


def block_is_fit(recs):
    K = len(recs)
    sizes = [len(r) for r in recs]
    assert K % 2 == 1 and bs.TRIP16 % K != 0 and set(s % 16 for s in sizes) == set(range(16))
    assert min(sizes) == 38 and 3000 < max(sizes) < 10000


def test_tiled_calmd_expectation_equals_the_model_on_two_tiles():
    """pycalmd on the base block, tiled, stamped and shifted by the reference's period, is pycalmd on every record of the tiled, stamped
    and shifted stream: the shift keeps every NM and MD, the records that grow, shrink and pass through among them"""
    import pycalmd
    targets, fasta, _ = bs.calmd_reference()
    names = [t[0] for t in targets]
    base = bs.calmd_block()
    block_is_fit(base)
    new, c = pycalmd.calmd_records(base, names, fasta)
    assert c["n_unchanged"] >= 8 and c["n_no_ref"] >= 1 and c["n_nm_changed"] > 50 and c["n_md_changed"] > 50
    grow = sum(1 for a, b in zip(base, new) if len(b) > len(a))
    shrink = sum(1 for a, b in zip(base, new) if len(b) < len(a))
    assert grow > 50 and shrink > 50
    t = bs.shift_positions(bs.stamp(bs.Tiled(base, 2)))
    want = bs.shift_positions(bs.stamp(bs.Tiled(new, 2)))
    assert (t.get(8, "<i4")[t.K:] != t.get(8, "<i4")[:t.K]).sum() > t.K // 2        # the second tile lies elsewhere
    got, c2 = pycalmd.calmd_records(records_of(t), names, fasta)
    assert b"".join(got) == want.buf.tobytes()
    assert c2 == {k: (2 * v) for k, v in c.items()}


def test_tiled_umi_expectation_equals_the_model_on_two_tiles():
    import pyumi
    base = bs.umi_block()
    block_is_fit(base)
    for source in ("RX", "name"):
        new, c = pyumi.umi_records(base, source)
        assert min(c["n_tagged"], c["n_no_source"], c["n_not_umi"], c["n_mi_dropped"]) > 10       # every outcome, under either source
        t = bs.stamp(bs.Tiled(base, 2))
        want = bs.stamp(bs.Tiled(new, 2))
        got, c2 = pyumi.umi_records(records_of(t), source)
        assert b"".join(got) == want.buf.tobytes(), source
        assert c2 == {k: (2 * v) for k, v in c.items()}


def test_tiled_sam_text_is_the_line_of_every_tiled_record():
    """the SAM block's lines and records come from samcases.case; the independent line model of samfmtcases agrees on every stamped copy, and
    more than 27 % of the block goes through the host's float formatter"""
    import samfmtcases
    lines, recs, host = bs.sam_block()
    K = len(recs)
    assert K % 2 == 1 and bs.TRIP16 % K != 0 and set(len(r) % 16 for r in recs) == set(range(16)) and max(len(r) for r in recs) > 4000
    assert sum(host) >= 0.27 * K and [samfmtcases.holds_float(r) for r in recs] == host
    assert all(r[36:44] == bs.ZEROS for r in recs) and all(ln[:8] == bs.ZEROS for ln in lines)
    tr = bs.stamp(bs.Tiled(recs, 2))
    tl = bs.Tiled(lines, 2)
    tl.put_digits(0)
    assert b"".join(samfmtcases.line_of(r) for r in records_of(tr)) == tl.buf.tobytes()
