"""The number a failing BGZF member gets from each caller of the shared GPU inflate driver (dev_inflate_members, gce_devstream.hpp): the
stand-alone entry numbers every member it is given, the engine's batch and the window runners number the non-empty ones, the window runners
from the window's first member.  One small BAM whose members run good, empty, BAD (a wrong CRC), good, good, and a second one with one more
good member in front, so that a window can begin behind the header.

gce_bam_index reads the BAM header with the host's inflater, one window's worth of the file at a time, before the GPU sees anything: a window
that holds the whole file hands the damaged member to the host first, whose message is "inflate / CRC failure" without a member number.
The window runner's "member 1 of a window" is therefore asserted on the second file, whose second window runs good, empty, BAD."""
import ctypes as C
import random
import struct
import zlib

import numpy as np
import pytest

import deflatecraft
import pybam
import recordstreams as R
from inflate_helpers import gpu_inflate, member
from test_bai_model import header

TARGETS = [("a", 100000), ("b", 50000)]


def _stream(n=12):
    rng = random.Random(7)
    recs = [dict(qname="q%03d" % i, flag=0, tid=0, pos=100 * i, mapq=60, cigar="100M", mtid=-1, mpos=-1, isize=0,
                 seq="".join(rng.choice("ACGT") for _ in range(100)), qual=[rng.randrange(2, 41) for _ in range(100)]) for i in range(n)]
    h = header(TARGETS)
    return h, h + b"".join(pybam.record_bytes(r) for r in recs), n


def _members(stream, cuts):
    return [member(stream[a:z], 6) for a, z in zip([0] + cuts, cuts + [len(stream)])]


def _bad_crc(m):
    crc = struct.unpack_from("<I", m, len(m) - 8)[0]
    return m[:-8] + struct.pack("<I", crc ^ 0x00010000) + m[-4:]


def _file_a():
    """good (header + records), empty, x, good, good: x is member 2 of the file, the second non-empty one"""
    h, stream, n = _stream()
    good = _members(stream, [len(h) + 700, len(h) + 1300, len(h) + 1900])
    assert len(good) == 4 and all(150 < len(m) < 700 for m in good)
    return h, n, good[:1] + [deflatecraft.EOF_MEMBER] + good[1:], 2


def _file_b():
    """good (header + records, larger than the next three together), good, empty, x, good: a window of the first member's size leaves the
    header to the host and starts the second window on the second member"""
    h, stream, n = _stream()
    good = _members(stream, [len(h) + 1600, len(h) + 1850, len(h) + 2100])
    assert len(good[0]) >= len(good[1]) + 28 + len(good[2]) and len(good[0]) >= len(good[3])
    return h, n, good[:2] + [deflatecraft.EOF_MEMBER] + good[2:], 3


def _write(path, members):
    path.write_bytes(b"".join(members) + pybam.EOF_BLOCK)
    assert [c for _, c, _ in R.bgzf_members(path.read_bytes())] == [len(m) for m in members] + [28]
    return path


def _spoil(members, k):
    return members[:k] + [_bad_crc(members[k])] + members[k + 1:]


def _usizes(members):
    return [struct.unpack_from("<I", m, len(m) - 4)[0] for m in members]


def _raw_batch(lib, members, first, n_ref):
    """the members through gce_raw_push_bgzf + gce_raw_finish on a fresh engine: (status, records, message)"""
    from gencore_amd.capi import default_params
    from gencore_amd.engine import Engine
    lib.gce_raw_begin.argtypes = [C.c_void_p, C.c_size_t]
    lib.gce_raw_push_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.gce_raw_finish.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_int64)]
    tl = np.asarray([ln for _, ln in TARGETS], np.uint32)
    E = Engine(default_params(n_targets=len(tl), target_len=tl.ctypes.data))
    try:
        blob = np.frombuffer(b"".join(members), np.uint8).copy()
        coff = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64)
        cs = np.array([len(m) for m in members], np.uint32); us = np.array(_usizes(members), np.uint32)
        tk = C.c_int32(); n = C.c_int64()
        assert lib.gce_raw_begin(E._h, int(us.sum())) == 0
        assert lib.gce_raw_push_bgzf(E._h, blob.ctypes.data, len(blob), len(members), coff.ctypes.data, cs.ctypes.data, us.ctypes.data, C.byref(tk)) == 0
        assert lib.gce_submit_wait(E._h, tk.value) == 0
        rc = lib.gce_raw_finish(E._h, first, n_ref, C.byref(n))
        return rc, n.value, lib.gce_last_error(E._h).decode()
    finally:
        E.close()


def _index_error(path, window_bytes):
    from gencore_amd.bamio import index_bam
    from gencore_amd.capi import GceError
    with pytest.raises(GceError) as x:
        index_bam(str(path), str(path) + ".bai", device=0, threads=2, window_bytes=window_bytes)
    print("index_bam(window_bytes=%d): %s" % (window_bytes, x.value))
    return str(x.value)


@pytest.mark.gpu
def test_failing_member_is_numbered_by_each_caller(built, tmp_path):
    from gencore_amd import capi
    from gencore_amd.bamio import index_bam
    lib = capi.load_library()
    h, n_rec, good, k = _file_a()
    bad = _spoil(good, k)
    whole = sum(len(m) for m in good) + 28

    # the stand-alone entry: every member it is given has a number
    rc, first_bad, _ = gpu_inflate(lib, bad, _usizes(bad))
    print("gce_bgzf_inflate:", rc, first_bad)
    assert (rc, first_bad) == (-1, 2)
    # the engine's batch: empty members have none
    rc, _, msg = _raw_batch(lib, bad, len(h), len(TARGETS))
    print("gce_raw_finish:", rc, msg)
    assert rc == -1 and "member 1 of the GPU batch" in msg
    # the index runner, the whole file in one window: the host reads the header from the same window and meets the member first
    pa = _write(tmp_path / "a_bad.bam", bad)
    msg = _index_error(pa, 2 * whole)
    assert "inflate / CRC failure" in msg and "of a window" not in msg
    # ... the damaged member the first one of the second window
    w = len(bad[0]) + 28
    assert w >= max(len(m) for m in bad) and w < len(bad[0]) + 28 + len(bad[2])
    assert "member 0 of a window" in _index_error(pa, w)

    # the second file: the second window is good, empty, BAD, ...
    hb, _, good_b, kb = _file_b()
    bad_b = _spoil(good_b, kb)
    pb = _write(tmp_path / "b_bad.bam", bad_b)
    assert "member 1 of a window" in _index_error(pb, len(bad_b[0]))

    # the CRC restored: every caller takes both files
    for hh, members, name in ((h, good, "a"), (hb, good_b, "b")):
        us = _usizes(members)
        rc, first_bad, out = gpu_inflate(lib, members, us)
        assert (rc, first_bad) == (0, -1) and out == b"".join(zlib.decompress(m, 31) for m in members)
        rc, n, msg = _raw_batch(lib, members, len(hh), len(TARGETS))
        assert (rc, n) == (0, n_rec), msg
        p = _write(tmp_path / (name + "_good.bam"), members)
        for w in (0, len(members[0]) + 28, len(members[0])):
            assert index_bam(str(p), str(p) + ".bai", device=0, threads=2, window_bytes=w)["n_records"] == n_rec
