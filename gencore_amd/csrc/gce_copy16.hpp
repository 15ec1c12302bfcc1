// gce_copy16.hpp — the 16-lane copy of a stretch of bytes that the sort's gather and scatter (gce_sort.hpp) and calmd's body copy
// (gce_calmd.hpp) share.  __host__ __device__: tests/calmd_host_check.hip runs it on the host, lane after lane.
#pragma once
#include <cstdint>

namespace {

typedef uint32_t c16_u32u __attribute__((aligned(1), may_alias));
// the copy of one record (or of a stretch of one) by its 16 lanes: sz bytes from s to d.  The stores are 16 bytes wide and aligned on the
// destination: head = the bytes in front of the first 16-byte boundary (one byte per lane), then whole chunks (each lane reads its 16 source
// bytes unaligned), then the bytes behind the last boundary (one byte per lane).  Every read stays inside [s, s + sz) and every write inside
// [d, d + sz), for any size and any pair of alignments.
__host__ __device__ __forceinline__ void sort_copy16(const uint8_t *s, uint8_t *d, uint32_t sz, uint32_t sub) {
    const uint32_t lead = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u, head = sz < lead ? sz : lead;
    const uint32_t nchunk = (sz - head) >> 4, tail = head + (nchunk << 4);
    if (sub < head) d[sub] = s[sub];
    for (uint32_t c = sub; c < nchunk; c += 16) {
        const uint32_t q = head + (c << 4);
        uint4 v;
        v.x = *(const c16_u32u *)(s + q); v.y = *(const c16_u32u *)(s + q + 4); v.z = *(const c16_u32u *)(s + q + 8); v.w = *(const c16_u32u *)(s + q + 12);
        *reinterpret_cast<uint4 *>(d + q) = v;
    }
    if (tail + sub < sz) d[tail + sub] = s[tail + sub];
}

}  // namespace
