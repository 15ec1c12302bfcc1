// gce_matejoin.hpp — the mate join that survives window boundaries: what gce_bam_pileup_fragments (gce_fragpile.hpp) and
// gce_bam_error_profile_fragments (gce_fragerr.hpp) share.  Rule P (the file is coordinate-sorted) and rule M (which two records
// are the mates of one fragment) are DESIGN.md 4k's.  Per window, behind the pass's scan (k_reduce_scan, gce_reduce.hpp):
//   k_frag_prep    one thread per entry -- the pending records of the arena, then the window's records.  Rule P against the predecessor (for
//                  the window's first record a device word that holds the previous window's last key), the lowest offender by atomicMin; rule
//                  M's candidate test; every candidate goes into an open-addressing table (slot = hash & mask, linear probing, atomicCAS on a
//                  32-bit entry index) under a 64-bit hash of (name bytes, refID, min(pos, next_pos), max(pos, next_pos)).  READ is the pass's
//                  part: how the 4 bytes of meta its scan left say whether the record is eligible and which interval it touches first
//   k_frag_join    one thread per entry: a candidate walks its probe run and compares, byte for byte, with every entry of equal hash: one
//                  partner, none, or ambiguity, whatever the insertion order.  A candidate without partner whose next_pos >= pos and whose
//                  partner may still come (the window's last key is not beyond (refID, next_pos), the file has not ended) is deferred
//   the count      the pass's own kernel, launched by the callback MateJoin::run is given, over the entries and what the join left of them
//   k_frag_carry   the deferred entries, whole and with their file-wide record index, into the other of two arenas, bump-allocated with one
//                  atomic per record; the next window joins against it
// fragpile::candidate, key, same_group and is_pair are __host__ __device__: the passes' host checks run them against the models.
#pragma once
#include <cstdint>
#include "gce_reduce.hpp"

namespace fragpile {

#define FP_HD __host__ __device__ inline

typedef uint32_t __attribute__((aligned(1), may_alias)) fp_u32u;
typedef uint16_t __attribute__((aligned(1), may_alias)) fp_u16u;

// what the join leaves per entry: the partner's entry index (FP_IS_B: this entry is the later of the two in the file), or one of
#define FP_ALONE 0xFFFFFFFFu          // counted by rule W alone
#define FP_DEFER 0xFFFFFFFEu          // not counted yet: carried to the next window
#define FP_SKIP  0xFFFFFFFDu          // touches no site, or is not eligible
#define FP_IS_B  0x80000000u
#define FP_Q_CAP 200u

FP_HD int32_t rd_i32(const uint8_t *p) { return (int32_t) * (const fp_u32u *)p; }

// rule P's key of a record: placed records by (tid, pos), every record with tid < 0 behind them
FP_HD uint64_t order_key(int32_t tid, int32_t pos) { return tid < 0 ? ~0ull : ((uint64_t)(uint32_t)tid << 32) | ((uint32_t)pos ^ 0x80000000u); }
FP_HD uint64_t order_key(const uint8_t *r) { return order_key(rd_i32(r + 4), rd_i32(r + 8)); }

// rule M's candidate test for an eligible record: C as reduce::rule_e left it, first as the scan did
FP_HD bool candidate(const uint8_t *r, const reduce::Core &C, uint32_t first) {
    if (first == RD_NONE) return false;
    const uint32_t fl = C.flag;
    if (!(fl & 0x1u) || (fl & (0x4u | 0x8u | 0x100u | 0x800u)) || !(((fl >> 6) ^ (fl >> 7)) & 1u)) return false;
    const int32_t ntid = rd_i32(r + 24), npos = rd_i32(r + 28);
    if (ntid != C.tid) return false;
    return !(npos >= C.pos && (int64_t)npos >= (int64_t)C.pos + C.rlen);
}

// the join's key: a 64-bit hash of (name bytes, refID, min(pos, next_pos), max(pos, next_pos)); weak: its low 4 bits alone
FP_HD uint64_t key(const uint8_t *r, bool weak) {
    const uint32_t lq = r[12];
    const int32_t pos = rd_i32(r + 8), npos = rd_i32(r + 28);
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t k = 0; k < lq; k++) h = (h ^ r[36 + k]) * 0x100000001b3ull;
    const uint32_t w[3] = {(uint32_t)rd_i32(r + 4), (uint32_t)(pos < npos ? pos : npos), (uint32_t)(pos < npos ? npos : pos)};
    for (int k = 0; k < 3; k++) { h = (h ^ w[k]) * 0x100000001b3ull; h ^= h >> 29; }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
    return weak ? (h & 15u) : h;
}

// two candidates of one group: the same l_read_name and name bytes, refID and unordered {pos, next_pos}
FP_HD bool same_group(const uint8_t *a, const uint8_t *b) {
    const uint32_t lq = a[12];
    if (lq != b[12] || rd_i32(a + 4) != rd_i32(b + 4)) return false;
    const int32_t pa = rd_i32(a + 8), na = rd_i32(a + 28), pb = rd_i32(b + 8), nb = rd_i32(b + 28);
    if ((pa < na ? pa : na) != (pb < nb ? pb : nb) || (pa < na ? na : pa) != (pb < nb ? nb : pb)) return false;
    for (uint32_t k = 0; k < lq; k++) if (a[36 + k] != b[36 + k]) return false;
    return true;
}
// ... that are a pair: one first, one last, each where the other says its mate is
FP_HD bool is_pair(const uint8_t *a, const uint8_t *b) {
    const uint32_t fa = *(const fp_u16u *)(a + 18), fb = *(const fp_u16u *)(b + 18);
    return ((fa ^ fb) & 0x40u) && rd_i32(a + 28) == rd_i32(b + 8) && rd_i32(b + 28) == rd_i32(a + 8);
}

#undef FP_HD

}  // namespace fragpile

#if !defined(GCE_FRAGPILE_HOST_CHECK) && !defined(GCE_FRAGERR_HOST_CHECK)

namespace {

// the join's device words
enum { FM_BAD = 0, FM_NCARRY, FM_CBYTES, FM_BUMP, FM_PAIRS, FM_SHARED, FM_DIFFER, FM_AMBIG, FM_DEFER, FM_KEY0, FM_KEY1, FM_WORDS = 12 };
// a slot of the arena: the file-wide record index (8 bytes), the scan's first interval (4), the slot's bytes (4), the record, padded to 8
#define FP_AHDR 16u
#define FP_EMPTY 0xFFFFFFFFu
#define FP_BUMP_SHIFT 40

// the entries of a window's join: [0, n_pend) the pending records of the arena, [n_pend, n) the window's records
struct FragView {
    const uint8_t *u; const uint64_t *off; const uint8_t *arena; const uint64_t *aoff; uint64_t n_pend, n, gbase;
    __device__ const uint8_t *rec(uint64_t e) const { return e < n_pend ? arena + aoff[e] + FP_AHDR : u + off[e - n_pend]; }
    __device__ uint64_t gidx(uint64_t e) const { return e < n_pend ? *(const uint64_t *)(arena + aoff[e]) : gbase + (e - n_pend); }
};
__device__ __forceinline__ uint32_t fp_slot_bytes(const uint8_t *r) { return (FP_AHDR + 4u + rb32(r) + 7u) & ~7u; }

// READ: read(r, meta[i], first, C) (meta NULL, for a pass without a scan: 0) -> the record is eligible; first: the first interval it can touch, or RD_NONE; C: its core fields, set for
// an eligible record whose first is not RD_NONE
template <class READ> __global__ __launch_bounds__(256) void k_frag_prep(FragView V, READ read, const uint32_t *meta, uint32_t par, uint32_t weak, uint64_t *hkey, uint32_t *first,
                                                                         uint32_t *partner, uint32_t *table, uint32_t mask, unsigned long long *fm) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= V.n) return;
    const uint8_t *r = V.rec(e);
    uint32_t f; bool cand;
    if (e < V.n_pend) { f = *(const uint32_t *)(V.arena + V.aoff[e] + 8); cand = true; }
    else {
        const uint64_t i = e - V.n_pend;
        const uint64_t k = fragpile::order_key(r), prev = i ? fragpile::order_key(V.u + V.off[i - 1]) : (uint64_t)fm[FM_KEY0 + par];
        if (k < prev) atomicMin(fm + FM_BAD, (unsigned long long)(V.gbase + i));
        if (e + 1 == V.n) fm[FM_KEY0 + (par ^ 1u)] = k;
        reduce::Core C;
        cand = read(r, meta ? meta[i] : 0u, f, C) && f != RD_NONE && fragpile::candidate(r, C, f);
    }
    first[e] = f;
    partner[e] = cand ? 0u : f == RD_NONE ? FP_SKIP : FP_ALONE;
    if (!cand) return;
    const uint64_t h = fragpile::key(r, weak != 0);
    hkey[e] = h;
    for (uint32_t slot = (uint32_t)h & mask;; slot = (slot + 1u) & mask)
        if (atomicCAS(table + slot, FP_EMPTY, (uint32_t)e) == FP_EMPTY) break;
}

__global__ __launch_bounds__(256) void k_frag_join(FragView V, const uint64_t *hkey, uint32_t *partner, const uint32_t *table, uint32_t mask, uint32_t par, uint32_t final, unsigned long long *fm) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool cand = e < V.n && partner[e] == 0u;
    bool pair_b = false, ambig = false, defer = false, fresh = false;
    uint32_t cbytes = 0;
    if (cand) {
        const uint8_t *r = V.rec(e);
        const uint64_t h = hkey[e];
        uint32_t cnt = 0, other = 0, res = FP_ALONE;
        for (uint32_t slot = (uint32_t)h & mask;; slot = (slot + 1u) & mask) {
            const uint32_t o = table[slot];
            if (o == FP_EMPTY) break;
            if (o != (uint32_t)e && hkey[o] == h && fragpile::same_group(r, V.rec(o))) { cnt++; other = o; }
        }
        if (cnt >= 2) ambig = true;
        else if (cnt == 1 && fragpile::is_pair(r, V.rec(other))) {
            pair_b = V.gidx(e) > V.gidx(other);
            res = other | (pair_b ? FP_IS_B : 0u);
        } else {
            const int32_t pos = fragpile::rd_i32(r + 8), npos = fragpile::rd_i32(r + 28);
            const bool expired = final || (uint64_t)fm[FM_KEY0 + (par ^ 1u)] > fragpile::order_key(fragpile::rd_i32(r + 4), npos);
            if (npos >= pos && !expired) { res = FP_DEFER; defer = true; fresh = e >= V.n_pend; cbytes = fp_slot_bytes(r); }
        }
        partner[e] = res;
    }
    const unsigned long long bp = __ballot(pair_b), ba = __ballot(ambig), bd = __ballot(defer), bf = __ballot(fresh);
#pragma unroll
    for (int d = 32; d; d >>= 1) cbytes += __shfl_xor(cbytes, d);
    if (lane_id() == 0) {
        if (bp) atomicAdd(fm + FM_PAIRS, (unsigned long long)__popcll(bp));
        if (ba) atomicAdd(fm + FM_AMBIG, (unsigned long long)__popcll(ba));
        if (bf) atomicAdd(fm + FM_DEFER, (unsigned long long)__popcll(bf));
        if (bd) { atomicAdd(fm + FM_NCARRY, (unsigned long long)__popcll(bd)); atomicAdd(fm + FM_CBYTES, (unsigned long long)cbytes); }
    }
}

// the deferred entries into the other arena: one atomic per record takes its slot number (the high bits) and its bytes (the low 40)
__global__ __launch_bounds__(256) void k_frag_carry(FragView V, const uint32_t *first, const uint32_t *partner, uint8_t *arena_out, uint64_t *aoff_out, uint64_t n_out, uint64_t bytes_out,
                                                    unsigned long long *fm) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= V.n || partner[e] != FP_DEFER) return;
    const uint8_t *r = V.rec(e);
    const uint32_t sz = fp_slot_bytes(r), body = 4u + rb32(r);
    const unsigned long long old = atomicAdd(fm + FM_BUMP, (1ull << FP_BUMP_SHIFT) | sz);
    const uint64_t k = old >> FP_BUMP_SHIFT, o = old & ((1ull << FP_BUMP_SHIFT) - 1);
    if (k >= n_out || o + sz > bytes_out) return;                                     // (the join counted exactly these: cannot be)
    aoff_out[k] = o;
    uint8_t *w = arena_out + o;
    *(uint64_t *)w = V.gidx(e); *(uint32_t *)(w + 8) = first[e]; *(uint32_t *)(w + 12) = sz;
    for (uint32_t b = 0; b < body; b++) w[FP_AHDR + b] = r[b];
}

}  // namespace

// The join's buffers and its host half, a member of the pass's device object p (a ReduceSession, whose needs() names them).
struct MateJoin {
    bool weak = false;
    DevBuf fm, hkey, first, partner, table;                                           // the device words; 16 bytes per entry; the join's table
    DevBuf arena[2], aoff[2]; int cur = 0; uint64_t n_pend = 0;                        // the pending records: arena[cur] is joined against, the other is written
    uint32_t par = 0;
    uint64_t table_bytes() const { return hkey.cap + first.cap + partner.cap + table.cap; }
    uint64_t arena_bytes() const { return arena[0].cap + arena[1].cap + aoff[0].cap + aoff[1].cap; }
    void release() { for (DevBuf *x : {&fm, &hkey, &first, &partner, &table, &arena[0], &arena[1], &aoff[0], &aoff[1]}) x->release(); }

    static int oom_own(ReduceSession *p, const char *what, uint64_t add) {
        char m[256];
        snprintf(m, sizeof m, "out of device memory: %s (%lld bytes live, budget %llu, %llu more for %s)", p->needs().c_str(), __atomic_load_n(&g_dev_live, __ATOMIC_RELAXED),
                 (unsigned long long)p->budget, (unsigned long long)add, what);
        return p->fail(GCE_ERR_OOM, m);
    }
    static int grow(ReduceSession *p, DevBuf &b, uint64_t bytes, const char *what) {
        if (bytes <= b.cap && b.p) return GCE_OK;
        const uint64_t add = DevBuf::padded(bytes);
        if (!p->room(add > b.cap ? add - b.cap : 0)) return oom_own(p, what, add);
        const hipError_t e = b.ensure(bytes);
        if (e == hipErrorOutOfMemory) return oom_own(p, what, add);
        return e == hipSuccess ? GCE_OK : p->fail(GCE_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    // the device words, made and set: once, behind the pass's rd_set_sites
    int init(ReduceSession *p) {
        const int rc = grow(p, fm, FM_WORDS * 8, "the pass's device words");
        if (rc != GCE_OK) return rc;
        const unsigned long long init[FM_WORDS] = {~0ull};
        RDCHK(hipMemcpyAsync(fm.p, init, sizeof init, hipMemcpyHostToDevice, p->s)); RDCHK(hipStreamSynchronize(p->s));
        return GCE_OK;
    }
    // One join: the pending records and the window's n_rec records (none: the flush behind the last window).  final: nothing more can come.
    // who: the entry point rule P's refusal names.  count(V, N, first, partner, fm) launches the pass's count kernel on p's stream.
    template <class READ, class COUNT> int run(ReduceSession *p, const char *who, const READ &read, const uint8_t *u, const uint64_t *off, uint64_t n_rec, bool final, COUNT &&count) {
        hipStream_t s = p->s;
        const uint64_t N = n_pend + n_rec;
        if (!N) return GCE_OK;
        if (N >= 0x7FFFFFF0ull) return p->fail(GCE_ERR_INVALID, "2^31 records or more in one window");
        uint64_t cap = 16; while (cap < 2 * N) cap <<= 1;
        int rc;
        if ((rc = grow(p, hkey, N * 8, "the join table")) != GCE_OK || (rc = grow(p, first, N * 4, "the join table")) != GCE_OK || (rc = grow(p, partner, N * 4, "the join table")) != GCE_OK ||
            (rc = grow(p, table, cap * 4, "the join table")) != GCE_OK) return rc;
        unsigned long long *m = fm.as<unsigned long long>();
        RDCHK(hipMemsetAsync(table.p, 0xFF, cap * 4, s));
        RDCHK(hipMemsetAsync(m + FM_NCARRY, 0, 3 * 8, s));
        const FragView V{u, off, arena[cur].as<uint8_t>(), aoff[cur].as<uint64_t>(), n_pend, N, p->n};
        const unsigned nb = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(k_frag_prep<READ>, dim3(nb), dim3(256), 0, s, V, read, (const uint32_t *)p->meta.p, par, weak ? 1u : 0u, hkey.as<uint64_t>(), first.as<uint32_t>(), partner.as<uint32_t>(),
                           table.as<uint32_t>(), (uint32_t)(cap - 1), m);
        RDCHK(hipGetLastError());
        hipLaunchKernelGGL(k_frag_join, dim3(nb), dim3(256), 0, s, V, (const uint64_t *)hkey.p, partner.as<uint32_t>(), (const uint32_t *)table.p, (uint32_t)(cap - 1), par, final ? 1u : 0u, m);
        RDCHK(hipGetLastError());
        unsigned long long h[3] = {~0ull, 0, 0};
        RDCHK(hipMemcpyAsync(h, m, sizeof h, hipMemcpyDeviceToHost, s)); RDCHK(hipStreamSynchronize(s)); RDCHK(hipGetLastError());
        if (h[FM_BAD] != ~0ull) {
            char msg[220]; snprintf(msg, sizeof msg, "BAM record %llu (counting from 0) lies in front of its predecessor: %s needs a coordinate-sorted file", h[FM_BAD], who);
            return p->fail(GCE_ERR_INVALID, msg);
        }
        const uint64_t n_carry = h[FM_NCARRY], cbytes = h[FM_CBYTES];
        if (n_carry) {
            if (cbytes >> FP_BUMP_SHIFT) return p->fail(GCE_ERR_INVALID, "2^40 bytes of deferred records or more");
            if ((rc = grow(p, arena[cur ^ 1], cbytes, "the arena")) != GCE_OK || (rc = grow(p, aoff[cur ^ 1], n_carry * 8, "the arena")) != GCE_OK) return rc;
        }
        if (count(V, N, (const uint32_t *)first.p, (const uint32_t *)partner.p, m)) RDCHK(hipGetLastError());
        if (n_carry) {
            hipLaunchKernelGGL(k_frag_carry, dim3(nb), dim3(256), 0, s, V, (const uint32_t *)first.p, (const uint32_t *)partner.p, arena[cur ^ 1].as<uint8_t>(), aoff[cur ^ 1].as<uint64_t>(), n_carry,
                               cbytes, m);
            RDCHK(hipGetLastError());
        }
        RDCHK(hipStreamSynchronize(s)); RDCHK(hipGetLastError());
        cur ^= 1; n_pend = n_carry;
        if (n_rec) par ^= 1u;
        return GCE_OK;
    }
};

#endif  // the host checks
