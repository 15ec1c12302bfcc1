"""The second launch of dev_inflate_members (gencore_amd/csrc/gce_devstream.hpp): gce_bgzf_inflate over 2^18 + 61 members, one more launch
than any other test makes.  A pool of 61 distinct members (61 is prime: a member decoded at a neighbour's offset, or with a neighbour's
code lengths, shows) of payloads from 0 to 400 bytes, stored, fixed and dynamic blocks, is cycled; the second launch then holds every pool
member, and its dynamic members reuse the code-length scratch of the first launch's.  The premise -- the member count is above
bigstreams.INFLATE_LAUNCH, which tests/test_bigstreams.py reads back from the source -- is asserted in the fixture.

A damaged member must be reported by its index in the caller's directory, not by its index within its launch; with damage in both launches
the first launch's is reported.  Only the returned index is asserted.

Measured on an MI355X: the good case 0.34 s (it compares 52 MB), each damaged case 0.06 s, the fixture 0.06 s; the module takes 1.2 s."""
import numpy as np
import pytest

import bigstreams as bs
from gencore_amd import capi
from inflate_helpers import gpu_inflate

pytestmark = pytest.mark.gpu

N = bs.INFLATE_LAUNCH + 61
LAST = N - 1


@pytest.fixture(scope="module")
def cycled(built):
    pool, datas, types = bs.member_pool(61)
    assert len(set(pool)) == len(set(datas)) == 61 and min(map(len, datas)) == 0 and max(map(len, datas)) == 400
    assert types.count(0) >= 10 and types.count(1) >= 10 and types.count(2) >= 10          # stored, fixed, dynamic
    assert N > bs.INFLATE_LAUNCH and N - bs.INFLATE_LAUNCH >= len(pool)                  # a second launch, with every pool member in it
    members = [pool[k % 61] for k in range(N)]
    sizes = [len(datas[k % 61]) for k in range(N)]
    want = (b"".join(datas) * (N // 61 + 1))[:sum(sizes)]
    return capi.load_library(), members, sizes, want, types


def test_both_launches_deliver_their_members(cycled):
    """k_bgzf_inflate's second launch (members 2^18 .. 2^18 + 60): every payload of both launches is zlib's"""
    lib, members, sizes, want, types = cycled
    assert {types[k % 61] for k in range(bs.INFLATE_LAUNCH, N)} == {0, 1, 2}
    rc, bad, got = gpu_inflate(lib, members, sizes)
    assert rc == 0 and bad == -1, (rc, bad)
    assert bs.first_difference(got, want) is None, bs.first_difference(got, want)


def damaged(members, k):
    m = bytearray(members[k])
    m[-8] ^= 1                                                  # a CRC bit, as tests/test_gpu_inflate.py::test_damaged_members_are_reported flips it
    return bytes(m)


@pytest.mark.parametrize("at,want", [((bs.INFLATE_LAUNCH - 1,), bs.INFLATE_LAUNCH - 1), ((bs.INFLATE_LAUNCH,), bs.INFLATE_LAUNCH), ((bs.INFLATE_LAUNCH + 7,), bs.INFLATE_LAUNCH + 7),
                                     ((LAST,), LAST), ((bs.INFLATE_LAUNCH - 1, bs.INFLATE_LAUNCH + 7), bs.INFLATE_LAUNCH - 1), ((5, bs.INFLATE_LAUNCH + 7), 5)],
                         ids=["last_of_launch_0", "first_of_launch_1", "launch_1_plus_7", "last_member", "both_launches_edge", "both_launches_early"])
def test_a_damaged_member_is_reported_by_its_own_index(cycled, at, want):
    """dev_inflate_members reports `base + got[1]`: the failing member of the second launch by its index among all members"""
    lib, members, sizes, _, _ = cycled
    ms = list(members)
    for k in at:
        ms[k] = damaged(members, k)
    rc, bad, _ = gpu_inflate(lib, ms, sizes)
    assert rc == -1 and bad == want, (rc, bad)
