"""gce_bam_merge_overlap on the GPU: the malformed-record check, the join over the whole file (k_frag_prep, k_frag_join) and
k_ovl_merge, through bamio.merge_overlap_bam, against the model (tests/pyovlmerge.py) and the hand-written bytes (tests/ovlcases.py): every
output record and every counter equal, the header untouched, nothing but QUAL bytes changed.  With the full and the weak hash, with windows so
small that pairs straddle them and records are cut by them, at two levels, on its own output, on a stream that takes every kernel past its
first grid trip, the pileup cross-check on the device, and the refusals."""
import os
import re
import zlib

import pytest

import fragcases as fc
import ovlcases as oc
import pileupcases as pc
import pyfragpile
import pyovlmerge
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHES = pytest.mark.parametrize("weak", [False, True], ids=["hash", "weak_hash"])


def inflate(path):
    raw, stream = open(path, "rb").read(), b""
    while raw:
        d = zlib.decompressobj(31)
        stream += d.decompress(raw)
        raw = d.unused_data
    return stream


def merged(tmp_path, records, tag="x", block=0xff00, **kw):
    """records as in.bam through merge_overlap_bam -> (the run, the output's records); the header bytes are the input's"""
    from gencore_amd.bamio import merge_overlap_bam
    src, dst = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.out.bam" % tag)
    if not src.exists():
        pc.write_raw_bam(str(src), records, oc.NAMES, oc.LENS, block)
    if dst.exists():
        dst.unlink()
    run = merge_overlap_bam(src, dst, threads=2, **kw)
    _, _, got = pyfragpile.read_raw_records(str(dst))
    a, b = inflate(str(src)), inflate(str(dst))
    n = len(a) - sum(map(len, records))
    assert len(a) == len(b) and a[:n] == b[:n]
    assert not os.path.exists(str(dst) + ".tmp%d" % os.getpid())
    return run, got


def same(run, got, want, res, records):
    assert got == want, [k for k, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    for k in pyovlmerge.COUNTERS:
        assert getattr(run, k) == res[k], k
    for r, w in zip(records, got):                                                   # nothing but QUAL bytes
        o, n = pyovlmerge.qual_offset(r), pypileup.fields(r)["lseq"]
        assert len(r) == len(w) and r[:o] == w[:o] and r[o + n:] == w[o + n:]
    assert run.inflated_bytes == sum(map(len, records)) and run.n_ref == len(oc.NAMES)


@pytest.mark.gpu
@HASHES
def test_hand_cases(built, tmp_path, weak):
    """every case of ovlcases -- rule Q column by column, the geometry, every op at the overlap's edges, the runs around 16 columns, the
    non-pairs -- and their records as one stream: the bytes written out by hand"""
    for cs in oc.all_cases():
        run, got = merged(tmp_path, cs["records"], tag=cs["label"], weak_hash=weak, min_mapq=cs["min_mapq"], exclude_flags=cs["exclude"])
        want, res = pyovlmerge.merge_overlap(cs["records"], cs["min_mapq"], cs["exclude"])
        same(run, got, want, res, cs["records"])
        assert got == oc.expected_records(cs) and res == cs["counters"], cs["label"]
    recs = oc.combined_stream()
    want, res = pyovlmerge.merge_overlap(recs)
    run, got = merged(tmp_path, recs, tag="combined", weak_hash=weak)
    same(run, got, want, res, recs)
    assert run.n_pairs >= 35 and run.n_ambiguous == 3 and run.n_pairs_no_qual == 2


@pytest.fixture(scope="module")
def fuzz():
    recs = oc.fuzz_pairs(400, 21)
    return recs, pyovlmerge.merge_overlap(recs)


@pytest.mark.gpu
@HASHES
def test_pairs_across_windows(built, fuzz, tmp_path, weak):
    """members of 300 bytes and windows of 2000 compressed bytes: a in one window and b in a later one, records cut between two windows; the
    join runs over the whole file, so the file is the one-window file and the model's"""
    recs, (want, res) = fuzz
    assert res["n_pairs"] == 400 and res["n_shared_columns"] > 4000 and res["n_disagree_columns"] > 300
    one, got = merged(tmp_path, recs, block=300, weak_hash=weak)
    same(one, got, want, res, recs)
    size = os.path.getsize(tmp_path / "x.bam")
    assert size > 20 * 2000 and max(map(len, recs)) < 300 < 2000                      # more than 20 windows, members that cut records
    cut, got = merged(tmp_path, recs, block=300, weak_hash=weak, window_bytes=2000)
    same(cut, got, want, res, recs)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [-2, 6])
def test_levels_and_idempotence(built, fuzz, tmp_path, level):
    """the same records at both levels; the pass over its own output changes no byte"""
    from gencore_amd.bamio import merge_overlap_bam
    recs, (want, res) = fuzz
    run, got = merged(tmp_path, recs, level=level)
    same(run, got, want, res, recs)
    again = merge_overlap_bam(tmp_path / "x.out.bam", tmp_path / "again.bam", level=level, threads=2)
    assert pyfragpile.read_raw_records(str(tmp_path / "again.bam"))[2] == want
    assert again.n_records_changed == 0 and again.n_pairs == res["n_pairs"] and again.n_shared_columns == res["n_shared_columns"] == again.n_columns_skipped


@pytest.mark.gpu
def test_past_the_first_grid_trip(built, tmp_path):
    """20000 pairs of 2 x 30 bases: 40000 entries are more than k_ovl_merge's grid takes in one trip (OV_GRID_BLOCKS blocks of 16 entries) and
    many blocks of the join's kernels (256 entries each)"""
    src = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_ovlmerge.hpp")).read()
    blocks = int(re.search(r"#define OV_GRID_BLOCKS (\d+)u", src).group(1))
    assert "(N + 15) / 16, OV_GRID_BLOCKS" in src and "e += (uint64_t)gridDim.x * 16u" in src
    recs = oc.fuzz_pairs(20000, 9, read_len=(30, 31), indels=False)
    assert len(recs) == 40000 > blocks * 16 > 256
    want, res = pyovlmerge.merge_overlap(recs)
    assert res["n_pairs"] == 20000 and res["n_shared_columns"] > 200000
    run, got = merged(tmp_path, recs)
    same(run, got, want, res, recs)


@pytest.mark.gpu
def test_pileup_of_the_rewritten_file_is_the_fragment_pileup(built, fuzz, tmp_path):
    """the cross-check of the model test on the device: gce_bam_pileup over the rewritten file counts what gce_bam_pileup_fragments counts over
    the original one, in every counter but LOWQ"""
    from gencore_amd.bamio import pileup_bam, pileup_fragments_bam
    recs, _ = fuzz
    merged(tmp_path, recs)
    (tmp_path / "whole.bed").write_text("".join("%s\t0\t%d\n" % t for t in zip(oc.NAMES, oc.LENS)))
    for m in (1, 13, 93):
        plain = pileup_bam(tmp_path / "x.out.bam", tmp_path / "whole.bed", min_baseq=m, threads=2)
        frag = pileup_fragments_bam(tmp_path / "x.bam", tmp_path / "whole.bed", min_baseq=m, threads=2)
        assert frag.n_pairs == 400 and frag.n_ambiguous == 0 and plain.counts.shape == frag.counts.shape == (sum(oc.LENS), 2, 8)
        assert (plain.counts[:, :, :7] == frag.counts[:, :, :7]).all()
        assert int(frag.counts[:, :, :7].sum()) > (10000 if m == 1 else 500)           # (at 93 only agreeing columns whose qualities sum to 93 or more are counted)


OOM = re.compile(r"out of device memory: gce_bam_merge_overlap is in-core and needs the inflated record bytes.*\(-?\d+ bytes live, budget (\d+), (\d+) more for [^)]+\)$")


@pytest.mark.gpu
def test_refusals_leave_no_output(built, fuzz, tmp_path):
    """rule P inside a window and on a window's first record, the malformed record in front of it, a budget below the file's need"""
    from gencore_amd.bamio import merge_overlap_bam
    from gencore_amd.capi import GceError
    bam, out = tmp_path / "in.bam", tmp_path / "out.bam"
    for k, wb in [(37, 0), (fc.ORDER_N - 8, 0), (fc.ORDER_N - 1, 0), (61, 2000), (fc.ORDER_N - 2, 2000)]:
        pc.write_raw_bam(str(bam), fc.order_stream(k), block=300)
        with pytest.raises(GceError) as ei:
            merge_overlap_bam(bam, out, window_bytes=wb)
        assert ei.value.status == -1 and str(ei.value).endswith("BAM record %d (counting from 0) lies in front of its predecessor: gce_bam_merge_overlap needs a coordinate-sorted file" % k), (k, wb)
    recs = fc.order_stream(60)
    pc.write_raw_bam(str(bam), recs[:70] + [pc.malformed()[0][1]] + recs[70:])
    with pytest.raises(GceError) as ei:
        merge_overlap_bam(bam, out)
    assert ei.value.status == -1 and "BAM record 70 (counting from 0): its fields overrun its block_size" in str(ei.value)
    recs, _ = fuzz
    pc.write_raw_bam(str(bam), recs, oc.NAMES, oc.LENS)
    free = merge_overlap_bam(bam, out)
    assert free.peak_device_bytes > sum(map(len, recs))
    out.unlink()
    with pytest.raises(GceError) as ei:
        merge_overlap_bam(bam, out, device_budget_bytes=sum(map(len, recs)) // 2)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and int(m.group(1)) == sum(map(len, recs)) // 2 and int(m.group(2)) > 0, str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam"]
