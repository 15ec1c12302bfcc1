"""The GPU BGZF encoder with dynamic Huffman codes (gce_deflate.hpp, k_bgzf_deflate_dyn; level -3) against zlib, gzip and the GPU inflater as
DECODERS: every kind of data and every block size, also with dynamic codes forced (codes=2) so that the degenerate trees are decoded too; member
for member never larger than the fixed-code encoder (codes=0); dynamic codes really chosen where they pay; and every runner at level -3 against the
same run at level 1 and level -2."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from gencore_amd import capi

pytestmark = pytest.mark.gpu

BLOCKS = [1, 7, 300, 4096, 16384, 65279, 65280]
M_RECORDS = 0.0779                 # test_record_stream_against_zlib_level_1: the measured excess 0.0579 + 0.02


def members_of(blob):
    """the BGZF members of a blob: (BSIZE from the BC subfield, raw deflate bytes, CRC, ISIZE) -- walked by the framing alone"""
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04" and blob[p + 12:p + 16] == b"BC\x02\x00", p
        (bs,) = struct.unpack_from("<H", blob, p + 16)
        bs += 1
        crc, isize = struct.unpack_from("<II", blob, p + bs - 8)
        out.append((bs, blob[p + 18:p + bs - 8], crc, isize))
        p += bs
    assert p == len(blob)
    return out


def gpu_inflate(lib, blob, mem):
    import ctypes as C
    csize = np.array([m[0] for m in mem], np.uint32)
    coff = (np.cumsum(csize, dtype=np.uint64) - csize).astype(np.uint64)
    usize = np.array([m[3] for m in mem], np.uint32)
    out = np.zeros(int(usize.sum()) + 8, np.uint8)
    bad = C.c_int32(-2)
    buf = np.frombuffer(blob, np.uint8)
    rc = lib.gce_bgzf_inflate(0, buf.ctypes.data, len(blob), len(mem), coff.ctypes.data, csize.ctypes.data, usize.ctypes.data, out.ctypes.data, C.byref(bad))
    return rc, bad.value, out[:int(usize.sum())].tobytes()


_STREAM = []


def record_stream():
    """a real record stream: cfg3 written as a BAM file, inflated"""
    if not _STREAM:
        import tempfile
        from gencore_amd import synth
        from gencore_amd.bamio import write_batch_as_bam
        d = synth.generate("cfg3", n_pairs=4000)
        with tempfile.TemporaryDirectory() as t:
            p = os.path.join(t, "s.bam")
            write_batch_as_bam(p, d.to_batch(), np.asarray(d.target_len, np.uint32))
            _STREAM.append(gzip.decompress(open(p, "rb").read()))
    return _STREAM[0]


def payloads(rng):
    """test_gpu_deflate.py's payloads, then the cases of the dynamic coder; (name, bytes)"""
    text = (b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"read%d\t99\tchr1\t%d\t60\t150M\t=\t%d\t300\tACGT\tFFFF\tNM:i:%d\n" % (i, 1000 + i, 1200 + i, i % 3) for i in range(6000)))
    base = [b"A", b"AC", b"ACG", b"ACGT", b"ACGTA", bytes(rng.integers(0, 256, 200000, dtype=np.uint8)),               # incompressible: stored blocks
            text, b"\0" * 300000, b"ab" * 100000, bytes(rng.integers(0, 4, 150000, dtype=np.uint8)),
            bytes(np.repeat(rng.integers(0, 256, 3000, dtype=np.uint8), rng.integers(1, 300, 3000))),                 # runs: distance 1, lengths up to 258 and beyond
            bytes(rng.integers(33, 74, 100000, dtype=np.uint8)),                                                      # quality-like
            (bytes(rng.integers(0, 256, 3000, dtype=np.uint8)) * 60),                                                 # distances of 3000
            (bytes(rng.integers(0, 256, 40000, dtype=np.uint8)) * 3),                                                 # distances beyond 32 768: no match allowed there
            bytes(rng.integers(144, 256, 50000, dtype=np.uint8)) + b"\x90" * 70000]                                   # 9-bit literals
    names = ["A", "AC", "ACG", "ACGT", "ACGTA", "random", "sam_text", "zeros", "ab", "two_bit", "runs", "quality", "dist3000", "dist40000", "nine_bit"]
    more = [("one_byte", b"Q" * 70000),                                                                                # a single repeated byte
            ("two_values", bytes(rng.choice(np.array([7, 200], np.uint8), 65280))),                                   # 65 280 bytes, exactly two distinct values
            ("distance_1", bytes(range(40)) + b"\x55" * 900 + bytes(range(100, 140))),                               # the only match distance is 1: one used distance code
            ("all_256", bytes(range(256))),                                                                           # 256 distinct bytes once each: no match
            ("records", record_stream())]
    return list(zip(names, base)) + more


def cut(name, d, block, k):
    return d[:3000 + k] if block < 300 and len(d) > 3000 else d


@pytest.mark.parametrize("codes", [1, 2])
@pytest.mark.parametrize("block", BLOCKS)
def test_every_member_decodes(built, block, codes):
    """1. validity, under zlib, gzip and the GPU inflater; codes=2 writes dynamic codes wherever they fit, so the trees of tiny and degenerate blocks
    (no match, one literal, one distance code) are decoded as well"""
    from gencore_amd.bamio import bgzf_deflate
    lib = capi.load_library()
    rng = np.random.default_rng(11)
    n_dyn = 0
    for k, (name, d) in enumerate(payloads(rng)):
        d = cut(name, d, block, k)
        blob = bgzf_deflate(d, block, codes)
        mem = members_of(blob)
        assert len(mem) == (len(d) + block - 1) // block
        at = 0
        for bs, raw, crc, isize in mem:
            piece = d[at:at + isize]
            assert isize == min(block, len(d) - at) and bs <= 0x10000, (name, block, at)
            assert zlib.decompress(raw, -15) == piece, (name, block, at)
            assert crc == (zlib.crc32(piece) & 0xFFFFFFFF), (name, block, at)
            n_dyn += (raw[0] >> 1) & 3 == 2
            at += isize
        assert at == len(d) and gzip.decompress(blob) == d, (name, block)
        rc, bad, got = gpu_inflate(lib, blob, mem)
        assert (rc, bad) == (0, -1) and got == d, (name, block, rc, bad)
    assert codes == 1 or n_dyn > 0


@pytest.mark.parametrize("block", BLOCKS)
def test_never_larger_than_fixed_codes_member_for_member(built, block):
    """2. the three candidates are priced exactly and the smallest is written, and codes=0 writes one of them from the same tokens"""
    from gencore_amd.bamio import bgzf_deflate
    rng = np.random.default_rng(11)
    for k, (name, d) in enumerate(payloads(rng)):
        d = cut(name, d, block, k)
        m0, m1 = members_of(bgzf_deflate(d, block, 0)), members_of(bgzf_deflate(d, block, 1))
        assert len(m0) == len(m1)
        for j, (a, b) in enumerate(zip(m0, m1)):
            assert b[0] <= a[0] and b[2:] == a[2:], (name, block, j, a[0], b[0])


def test_codes_0_is_the_fixed_code_entry_point(built):
    from gencore_amd.bamio import bgzf_deflate
    from test_gpu_deflate import gpu_deflate
    d = record_stream()[:300000]
    rc, blob = gpu_deflate(capi.load_library(), d, 0xff00)
    assert rc == 0 and blob == bgzf_deflate(d, 0xff00, 0)


def test_dynamic_codes_are_chosen_where_they_pay(built):
    """3. quality-like bytes and a record stream at 65 280: BTYPE 10 in a member's first block, and a strictly smaller blob"""
    from gencore_amd.bamio import bgzf_deflate
    rng = np.random.default_rng(11)
    for name, d in payloads(rng):
        if name not in ("quality", "records"):
            continue
        b0, b1 = bgzf_deflate(d, 0xff00, 0), bgzf_deflate(d, 0xff00, 1)
        assert any((raw[0] >> 1) & 3 == 2 for _, raw, _, _ in members_of(b1)), name
        assert len(b1) < len(b0), (name, len(b0), len(b1))


def test_record_stream_against_zlib_level_1(built):
    """The record stream at 65 280-byte blocks: deflate bytes at codes=1 <= zlib level 1's x (1 + m).  The encoder is deterministic, so the figures
    are exact: 2 500 489 bytes in, 611 294 at codes=1 against zlib level 1's 577 857 -- measured excess 0.0579 (profiles/deflate_dynamic_sizes.json;
    codes=0: 755 682, excess 0.3077).  m = 0.0779 = the measured 0.0579 + 0.02, the room for a later matcher change that trades a little ratio for
    speed."""
    from gencore_amd.bamio import bgzf_deflate
    d = record_stream()
    z1 = 0
    for at in range(0, len(d), 0xff00):
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += len(co.compress(d[at:at + 0xff00]) + co.flush())
    g = sum(len(raw) for _, raw, _, _ in members_of(bgzf_deflate(d, 0xff00, 1)))
    print("record stream: %d bytes, codes=1 %d, zlib-1 %d, excess %.4f" % (len(d), g, z1, g / z1 - 1))
    assert g <= z1 * (1 + M_RECORDS)


def bam_inputs(tmp_path, workload, n_pairs):
    import pybam
    from gencore_amd import synth
    from gencore_amd.capi import default_params
    from test_bamio import records_of
    d = synth.generate(workload, n_pairs=n_pairs)
    batch = d.to_batch()
    targets = [("chr%d" % (i + 1), int(l)) for i, l in enumerate(np.asarray(d.target_len, np.uint32))]
    src = str(tmp_path / "in.bam")
    pybam.write_bam(src, records_of(batch), targets)
    return src, default_params(umi_prefix="auto", cluster_size_req=d.info["supporting_reads"])


def same_bam(r1, r3, a, c):
    import pybam
    assert (r1.n_reads, r1.n_out) == (r3.n_reads, r3.n_out) and r1.n_out > 0
    assert pybam.read_bam(a) == pybam.read_bam(c)


@pytest.mark.parametrize("workload,n_pairs", [("cfg3", 30000), ("cfg2", 20000), ("cfg5", 3000)])
def test_run_bam_level_minus_3(built, tmp_path, workload, n_pairs):
    """4. gce_run_bam at level -3 writes the header and records of level 1, in a file no larger than level -2's"""
    from gencore_amd.bamio import run_bam
    src, prm = bam_inputs(tmp_path, workload, n_pairs)
    a, b, c = (str(tmp_path / x) for x in ("l1.bam", "m2.bam", "m3.bam"))
    r1 = run_bam(src, a, prm, threads=4, level=1)
    run_bam(src, b, prm, threads=4, level=-2)
    r3 = run_bam(src, c, prm, threads=4, level=-3)
    same_bam(r1, r3, a, c)
    assert os.path.getsize(c) <= os.path.getsize(b)
    if workload == "cfg3":
        assert os.path.getsize(c) < os.path.getsize(b)


def test_run_bam_sharded_level_minus_3(built, tmp_path):
    from gencore_amd.bamio import run_bam_sharded
    src, prm = bam_inputs(tmp_path, "cfg3", 30000)
    a, b, c = (str(tmp_path / x) for x in ("l1.bam", "m2.bam", "m3.bam"))
    r1 = run_bam_sharded(src, a, prm, [0, 0], threads=4, level=1)
    run_bam_sharded(src, b, prm, [0, 0], threads=4, level=-2)
    r3 = run_bam_sharded(src, c, prm, [0, 0], threads=4, level=-3)
    same_bam(r1, r3, a, c)
    assert os.path.getsize(c) <= os.path.getsize(b)


def test_run_bam_passes_level_minus_3(built, tmp_path):
    from test_passes_gpu import inputs, params, passes, same, single
    d, _, _ = inputs(tmp_path)
    prm = params(d)
    r1, d1 = single(tmp_path, prm, "one.bam", level=1)
    passes(tmp_path, prm, "m2.bam", level=-2, min_passes=4)
    r, dp, pr = passes(tmp_path, prm, "m3.bam", level=-3, min_passes=4)
    assert pr["n_passes"] == 4
    same(tmp_path, "one.bam", "m3.bam", r1, r, d1, dp)
    assert os.path.getsize(tmp_path / "m3.bam") <= os.path.getsize(tmp_path / "m2.bam")


def test_cli_level_minus_3_with_index(built, tmp_path):
    """`--level -3 --index`: the GPU index of each output is the model's index of that same file (virtual offsets differ between the two files)"""
    import pybai
    import pybam
    from test_cli_gpu import cli
    from test_passes_gpu import inputs
    inputs(tmp_path, n_pairs=20000)
    base = ["-i", "in.bam", "-r", "ref.fa", "-b", "panel.bed", "--threads", "4", "-s", "2", "--index"]
    for name, level in (("l6", "6"), ("m3", "-3")):
        r = cli(base + ["-o", name + ".bam", "-j", name + ".json", "--level", level], tmp_path)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / (name + ".bam.bai")).read_bytes() == pybai.build(tmp_path / (name + ".bam")), name
    assert pybam.read_bam(str(tmp_path / "l6.bam")) == pybam.read_bam(str(tmp_path / "m3.bam"))
