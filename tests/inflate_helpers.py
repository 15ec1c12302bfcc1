"""What the tests of the GPU BGZF decoder share: a member written by zlib, and one launch of gce_bgzf_inflate over a list of members."""
import ctypes as C
import struct
import zlib

import numpy as np


def member(data, level, strategy=zlib.Z_DEFAULT_STRATEGY, extra=b""):
    """one BGZF member (SAM spec 4.1): gzip header with the BC subfield (and optionally more subfields in front), raw deflate, CRC-32, ISIZE"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = co.compress(data) + co.flush()
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(body) + 8
    assert bsize <= 0x10000
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\0" + struct.pack("<H", bsize - 1) + body + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def gpu_inflate(lib, members, sizes):
    blob = b"".join(members)
    coff = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64) if members else np.zeros(0, np.uint64)
    csize = np.array([len(m) for m in members], np.uint32)
    usize = np.array(sizes, np.uint32)
    out = np.zeros(int(usize.sum()) + 8, np.uint8)
    bad = C.c_int32(-2)
    buf = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
    rc = lib.gce_bgzf_inflate(0, buf.ctypes.data, len(blob), len(members), coff.ctypes.data, csize.ctypes.data, usize.ctypes.data, out.ctypes.data, C.byref(bad))
    return rc, bad.value, out[:int(usize.sum())].tobytes()
