"""The GPU BGZF decoder (gce_inflate.hpp) on the hand-built members of deflatecraft.py: what zlib takes comes out byte for byte, at every
alignment of the member and of its deflate data; what zlib refuses is refused, and the members around it are delivered.  zlib has judged
the catalogue before (test_deflatecraft.py); the host decoder sees the same members in test_bgzf_host.py."""
import zlib

import pytest

import deflatecraft as dc
from gencore_amd import capi
from inflate_helpers import gpu_inflate, member

pytestmark = pytest.mark.gpu

CASES = dc.cases()
VALID = [c for c in CASES if c[3] is not None]
INVALID = [c for c in CASES if c[3] is None]
GOOD = [b"a member zlib wrote " * 40, bytes(range(256)) * 3, b"ACGTTGCA" * 111 + b"N"]


def check_valid(lib, cs):
    rc, bad, got = gpu_inflate(lib, [c[1] for c in cs], [c[2] for c in cs])
    assert rc == 0 and bad == -1, (rc, bad, cs[bad][0] if 0 <= bad < len(cs) else None)
    off = 0
    for name, _, usize, want in cs:
        assert got[off:off + usize] == want, name                                     # the first case that differs
        off += usize
    assert off == len(got)


def test_all_valid_cases_in_one_launch_and_in_reverse(built):
    lib = capi.load_library()
    assert VALID[0][0] == "stored_final" and VALID[-1][0] == "eof_member"              # each is the last member of one of the two launches
    check_valid(lib, VALID)
    check_valid(lib, VALID[::-1])                                                      # other coff and uoff alignments, other lanes


def test_deflate_data_at_every_alignment_of_member_and_data(built):
    """the eight align_x members (deflate data at every offset mod 8 inside the member), each at every offset mod 8 of the member itself: a
    member of fitting size stands in front of each"""
    lib = capi.load_library()
    by_name = {c[0]: c for c in CASES}
    cs, off, seen = [], 0, set()
    for x in range(4, 12):
        c = by_name["align_x%d" % x]
        for a in range(8):
            d = dc.Deflate().fixed(dc.lits(3, a) + [dc.EOB], final=True)
            body = d.body()
            n = next(n for n in range(8) if (off + 18 + 4 + n + len(body) + 8) % 8 == a)
            filler = dc.frame(body, zlib.crc32(bytes(d.out)), len(d.out), extra=dc.subfield(n))
            cs.append(("filler", filler, len(d.out), bytes(d.out)))
            off += len(filler)
            assert off % 8 == a
            seen.add((off % 8, (off + 18 + x) % 8))
            cs.append(c)
            off += len(c[1])
    assert len(seen) == 64
    check_valid(lib, cs)


@pytest.mark.parametrize("name", [c[0] for c in INVALID])
def test_invalid_case_is_refused_between_good_members(built, name):
    lib = capi.load_library()
    _, m, usize, _ = next(c for c in INVALID if c[0] == name)
    rc, bad, got = gpu_inflate(lib, [member(GOOD[0], 6), m, member(GOOD[1], 1)], [len(GOOD[0]), usize, len(GOOD[1])])
    assert rc == -1 and bad == 1, (rc, bad)
    assert got[:len(GOOD[0])] == GOOD[0] and got[len(GOOD[0]) + usize:] == GOOD[1]


def test_mixed_launch_reports_the_first_invalid_case(built):
    lib = capi.load_library()
    members, sizes, wants = [], [], []
    for k, (name, m, usize, want) in enumerate(CASES):
        g = GOOD[k % 3]
        members += [m, member(g, (1, 6, 9)[k % 3])]; sizes += [usize, len(g)]; wants += [want, g]
    first = next(i for i, w in enumerate(wants) if w is None)
    rc, bad, got = gpu_inflate(lib, members, sizes)
    assert rc == -1 and bad == first, (rc, bad, first, CASES[bad // 2][0] if bad >= 0 else None)
    off = 0
    for i, (n, w) in enumerate(zip(sizes, wants)):
        if i % 2:
            assert got[off:off + n] == w, "the zlib-written member behind %s" % CASES[i // 2][0]
        off += n
