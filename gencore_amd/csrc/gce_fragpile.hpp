// gce_fragpile.hpp — gce_bam_pileup's table with every fragment counted once where its mates overlap (gce_bam_pileup_fragments).
//
// The same sites (rule S), record filters (rule E), walk (rule W) and table (rule O) as gce_pileup.hpp, over the same windowed reduce frame
// (gce_reduce.hpp), for a coordinate-sorted file (rule P).  What is new is a mate join that survives window boundaries (rule M) and a count
// kernel that walks two records at once (rule V).  The join -- k_frag_prep, k_frag_join, k_frag_carry, the arenas and their host half -- is
// gce_matejoin.hpp's, shared with gce_fragerr.hpp; this file gives it FragpileRead and k_frag_count.  Per window, behind the scan
// (k_reduce_scan over PileScan):
//   k_frag_prep    one thread per entry -- the pending records of the arena, then the window's records.  Rule P against the predecessor (for
//                  the window's first record a device word that holds the previous window's last key), the lowest offender by atomicMin; rule
//                  M's candidate test; every candidate goes into an open-addressing table (slot = hash & mask, linear probing, atomicCAS on a
//                  32-bit entry index) under a 64-bit hash of (name bytes, refID, min(pos, next_pos), max(pos, next_pos))
//   k_frag_join    one thread per entry: a candidate walks its probe run and compares, byte for byte, with every entry of equal hash: one
//                  partner, none, or ambiguity, whatever the insertion order.  A candidate without partner whose next_pos >= pos and whose
//                  partner may still come (the window's last key is not beyond (refID, next_pos), the file has not ended) is deferred
//   k_frag_count   16 lanes per entry, 16 entries per block, the LDS tile and PileAdd of k_pile_count: pileup::count_record for an entry
//                  without partner, nothing for a deferred one, fragpile::paired_walk for a mate: pileup::walk_record (gce_pileup.hpp)
//                  under the functor ColumnV, which at each of the mate's own columns looks the partner's (class, quality) up from the
//                  partner's CIGAR (fragpile::column) and decides the mate's add by rule V; no order between the mates is needed.  The later mate's walk alone adds to rule V's counters, reduced per wave.  k_frag_count<true>
//                  (GCE_FRAGPILE_DIRECT): global atomics only
//   k_frag_carry   the deferred entries, whole and with their file-wide record index, into the other of two arenas, bump-allocated with one
//                  atomic per record; the next window joins against it
// fragpile::candidate, key, same_group, is_pair, column and paired_walk are __host__ __device__: tests/fragpile_host_check.hip runs them on
// the host against tests/pyfragpile.py, the model of the rules.
#pragma once
#include <cstdint>
#include "gce_pileup.hpp"
#include "gce_matejoin.hpp"

namespace fragpile {

#define FP_HD __host__ __device__ inline

using pileup::Params; using pileup::Sites; using pileup::PU_DEL; using pileup::PU_LOWQ;

// Rule V's lookup: the raw class (A C G T N, DEL for a D column) and the quality (0 for a D column or a record without qualities) of eligible
// record r at reference column x; false: no M / = / X / D op of it covers x
FP_HD bool column(const uint8_t *r, int64_t x, uint32_t &cls, uint32_t &q) {
    const reduce::Head h(r);
    int64_t x0 = h.pos; uint32_t q0 = 0;
    if (x < x0) return false;
    for (uint32_t k = 0; k < h.nc; k++) {
        const uint32_t w = *(const reduce::rd_u32u *)(h.cg + 4 * k), op = w & 15u, len = w >> 4;
        if (op == 0 || op == 7 || op == 8 || op == 2 || op == 3) {
            if (x < x0 + len) {
                if (op == 3) return false;
                if (op == 2) { cls = PU_DEL; q = 0; return true; }
                const uint32_t yi = q0 + (uint32_t)(x - x0);
                cls = reduce::read_class(h.sq, yi);
                q = h.has_q() ? h.ql[yi] : 0u;
                return true;
            }
            x0 += len; if (op != 2 && op != 3) q0 += len;
        } else if (op == 1 || op == 4) q0 += len;
    }
    return false;
}

// Rule V at one column of a mate of a pair whose other mate is o: pileup::walk_record's functor, so that the mate is walked as
// pileup::count_record walks a record alone.  is_b: the mate is the later of the two in the file.  A column that o covers is decided by rule V
// and the mate adds only what it has won; every other column is rule W's.  shared, differ: rule V's counters, added to by the later mate's
// walk alone.
struct ColumnV {
    const uint8_t *o; bool is_b; uint32_t &shared, &differ;
    FP_HD bool operator()(const Params &P, const pileup::Column &c, uint32_t &cls) {
        uint32_t mq;
        c.load(cls, mq);
        uint32_t oc = 0, oq = 0, adj = mq;
        if (column(o, c.x, oc, oq)) {
            const uint32_t qa = is_b ? oq : mq, qb = is_b ? mq : oq;
            bool mine;
            if (cls == oc) { mine = !is_b; adj = qa + qb < FP_Q_CAP ? qa + qb : FP_Q_CAP; }
            else { mine = is_b ? qa < qb : qa >= qb; adj = (4u * mq) / 5u; }
            if (is_b) { shared++; differ += cls != oc; }
            if (!mine) return false;
        }
        if (c.lowq(P, adj)) cls = PU_LOWQ;
        return true;
    }
};
// Rules W and V for a mate r of a pair whose other mate is o, by lane `lane` of the record's `nlanes`; the insertions are rule W's
template <class ADD> FP_HD void paired_walk(const uint8_t *r, const uint8_t *o, bool is_b, const Params &P, const Sites &S, uint32_t first, uint32_t lane, uint32_t nlanes, ADD &add,
                                            uint32_t &shared, uint32_t &differ) {
    ColumnV at{o, is_b, shared, differ};
    pileup::walk_record(r, P, S, first, lane, nlanes, at, add);
}

#undef FP_HD

}  // namespace fragpile

#ifndef GCE_FRAGPILE_HOST_CHECK

namespace {

// what k_reduce_scan over PileScan left in meta: the first interval, or PU_NONE for a record that is skipped or touches none
struct FragpileRead {
    pileup::Params P;
    __device__ bool operator()(const uint8_t *r, uint32_t m, uint32_t &first, reduce::Core &C) const {
        first = m;
        return m != RD_NONE && reduce::rule_e(r, 4ull + rb32(r), P.n_ref, P.min_mapq, P.exclude, C) == reduce::ELIGIBLE;
    }
};

// 16 lanes per entry, 16 entries per block (block b: entries [16 b, 16 b + 16)), the tile and the adds of k_pile_count (PileAdd,
// gce_pileup.hpp); n_counts: 16 x the number of sites
template <bool DIRECT> __global__ __launch_bounds__(256) void k_frag_count(FragView V, pileup::Params P, pileup::Sites S, const uint32_t *first, const uint32_t *partner, uint32_t *counts,
                                                                           uint64_t n_counts, unsigned long long *fm) {
    const uint32_t sub = threadIdx.x & 15u;
    const uint64_t e = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 4);
    uint32_t f = PU_NONE, pc = FP_SKIP;
    if (e < V.n) { pc = partner[e]; if (pc != FP_SKIP && pc != FP_DEFER) f = first[e]; }
    const uint8_t *r = f != PU_NONE ? V.rec(e) : nullptr;
    PileAdd<DIRECT> add;
    if (!add.open(f, S, counts, [&] { return r; })) return;
    uint32_t shared = 0, differ = 0;
    if (f != PU_NONE) {
        if (pc == FP_ALONE) pileup::count_record(r, P, S, f, sub, 16u, add);
        else fragpile::paired_walk(r, V.rec(pc & ~FP_IS_B), (pc & FP_IS_B) != 0, P, S, f, sub, 16u, add, shared, differ);
    }
    add.flush(n_counts);
#pragma unroll
    for (int d = 32; d; d >>= 1) { shared += __shfl_xor(shared, d); differ += __shfl_xor(differ, d); }
    if (lane_id() == 0) {
        if (shared) atomicAdd(fm + FM_SHARED, (unsigned long long)shared);
        if (differ) atomicAdd(fm + FM_DIFFER, (unsigned long long)differ);
    }
}

}  // namespace

struct gce_fragpile : PileSession {
    MateJoin J; int cb_rc = GCE_OK;
    std::string needs() const override {
        return "gce_bam_pileup_fragments needs 64 bytes per site (" + std::to_string(n_sites) + " sites), a join table (" + std::to_string(J.table_bytes()) + " bytes) and an arena (" +
               std::to_string(J.arena_bytes()) + " bytes)";
    }
    int process(const uint8_t *u, const uint64_t *off, uint64_t n_rec, bool final);
};

// One join (MateJoin::run) with k_frag_count between join and carry
int gce_fragpile::process(const uint8_t *u, const uint64_t *off, uint64_t n_rec, bool final) {
    return J.run(this, "gce_bam_pileup_fragments", FragpileRead{P}, u, off, n_rec, final, [&](const FragView &V, uint64_t N, const uint32_t *first, const uint32_t *partner, unsigned long long *m) {
        if (!n_sites) return false;
        dispatch([&](auto D) {
            hipLaunchKernelGGL(k_frag_count<decltype(D)::value>, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, s, V, P, sites(), first, partner, counts.as<uint32_t>(), n_sites * 16, m);
        });
        return true;
    });
}

extern "C" {

int gce_fragpile_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_fragpile **out) {
    if (out) *out = nullptr;
    if (options & ~(uint32_t)(GCE_FRAGPILE_DIRECT | GCE_FRAGPILE_WEAK_HASH)) return GCE_ERR_INVALID;
    const int rc = rd_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options & (uint32_t)GCE_FRAGPILE_DIRECT, (uint32_t)GCE_FRAGPILE_DIRECT, out);
    if (rc == GCE_OK) (*out)->J.weak = (options & GCE_FRAGPILE_WEAK_HASH) != 0;
    return rc;
}
void gce_fragpile_destroy(gce_fragpile *p) {
    if (!p) return;
    (void)hipSetDevice(p->device); (void)hipStreamSynchronize(p->s);
    p->J.release();
    rd_destroy(p, {&p->counts});
}
const char *gce_fragpile_error(gce_fragpile *p) { return p ? p->err.c_str() : ""; }

// rule S's intervals, as gce_pileup_set_sites takes them; the counters and the pass's device words are made and zeroed
int gce_fragpile_set_sites(gce_fragpile *p, int32_t n_ref, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, const uint32_t *site0) {
    int rc = pu_set_sites(p, "gce_fragpile_set_sites", n_ref, n_intervals, tid, start, end, site0);
    if (rc != GCE_OK) return rc;
    p->sites_set = false;
    if ((rc = p->J.init(p)) != GCE_OK) return rc;
    p->sites_set = true;
    return GCE_OK;
}

// the next piece of the file, as gce_pileup_window takes it; *pileup_s: the seconds of the scan, the join and the count, added to.
// GCE_ERR_INVALID names the lowest malformed record, else the first record that lies in front of its predecessor, counting from 0 over the file.
int gce_fragpile_window(gce_fragpile *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, double *pileup_s) {
    if (!p) return GCE_ERR_INVALID;
    p->cb_rc = GCE_OK;
    const int rc = rd_window(p, PileScan{p->P, p->sites()}, p->P.n_ref, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, pileup_s,
                             [&](const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t) { p->cb_rc = p->process(u, off, n_rec, last != 0); return p->cb_rc == GCE_OK; });
    return rc != GCE_OK ? rc : p->cb_rc;
}

// after the last window: what is still pending is counted alone; counters[0..7] as gce_pileup_finish gives them, [8] pairs, [9] shared columns,
// [10] those whose classes differ, [11] ambiguous candidates, [12] records carried across a window boundary
int gce_fragpile_finish(gce_fragpile *p, int64_t counters[13], uint32_t *counts_out) {
    if (!p || !p->sites_set || !counters) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    int rc = p->process(nullptr, nullptr, 0, true);
    if (rc != GCE_OK) return rc;
    if ((rc = pu_finish(p, counters, counts_out)) != GCE_OK) return rc;
    unsigned long long f[FM_WORDS];
    RDCHK(hipMemcpyAsync(f, p->J.fm.p, sizeof f, hipMemcpyDeviceToHost, s)); RDCHK(hipStreamSynchronize(s));
    counters[8] = (int64_t)f[FM_PAIRS]; counters[9] = (int64_t)f[FM_SHARED]; counters[10] = (int64_t)f[FM_DIFFER]; counters[11] = (int64_t)f[FM_AMBIG]; counters[12] = (int64_t)f[FM_DEFER];
    return GCE_OK;
}

}  // extern "C"
#endif  // GCE_FRAGPILE_HOST_CHECK
