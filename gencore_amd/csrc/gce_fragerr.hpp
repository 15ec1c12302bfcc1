// gce_fragerr.hpp — gce_bam_error_profile's table with every fragment counted once where its mates overlap, and a second table of what the two
// mates say about each other there (gce_bam_error_profile_fragments).
//
// Rules E, G, C, B, W and O are gce_errprof.hpp's, rules P and M and the join that carries them across windows gce_matejoin.hpp's.  New here:
// rule V' (at a column that an M / = / X op of both mates covers, one of the two is counted in the primary table, as gce_fragpile.hpp's rule V
// chooses it) and rule X (both mates add to the overlap table there: agreement with the reference, agreement against it, or which of the two
// made a sequencing error at which cycle).  Per window, behind the scan (k_reduce_scan over ErrScan) and the join:
//   k_fragerr_count  k_err_count's shape: 16 lanes per entry, 32 entries per step of a block of 512 threads, a fixed grid whose blocks stride
//                    over the entries.  errprof::count_record for an entry without partner, nothing for a deferred one,
//                    errprof::paired_walk for a mate: gce_errprof.hpp's walk_record under the functor MateColumn, which at every column of
//                    the mate's own asks an errprof::Cursor over the partner's CIGAR; the cursor only moves forward, so a lane reads every
//                    op of the partner once per record, not once per column.  One LDS plane for the
//                    primary table and one for the overlap table; cycles past EP_CYC are 64-bit global atomics.  k_fragerr_count<true>
//                    (GCE_FRAGERR_DIRECT): global atomics only.
// errprof::Cursor and errprof::paired_walk are __host__ __device__: tests/fragerr_host_check.hip runs them on the host against
// tests/pyfragerr.py, the model of the rules.
#pragma once
#include <cstdint>
#include "gce_errprof.hpp"
#include "gce_matejoin.hpp"

namespace errprof {

#define EP_HD __host__ __device__ inline

enum { OVL_AGREE_REF = 16, OVL_AGREE_ALT, OVL_DIFF_OTHER, OVL_UNUSABLE, OVL_LOWQ, OVL_NCLASS };
#define OVL_MASKED EP_MASKED                                                          // rule Y in the overlap table: class 21, with a variant mask alone
static_assert((unsigned)OVL_NCLASS == EP_CLS, "the overlap table has the primary table's row");

// A forward-only cursor over the CIGAR of an eligible record o: op k starts at reference x0 and query q0.  at(x, cls, q): the raw class
// (0..3 = A C G T, 4 = N) and the quality (0 for a record without qualities) of o's base at reference column x; false: no M / = / X op of o
// covers x.  The x of successive calls must not decrease: every op is read once however many columns are asked for.
struct Cursor {
    const uint8_t *cg, *sq, *ql; uint32_t nc, k, q0; int64_t x0; bool has_q;
    EP_HD explicit Cursor(const uint8_t *o) {
        const Head h(o);
        cg = h.cg; sq = h.sq; ql = h.ql; nc = h.nc; has_q = h.has_q();
        k = 0; q0 = 0; x0 = h.pos;
    }
    EP_HD bool at(int64_t x, uint32_t &cls, uint32_t &q) {
        if (x < x0) return false;                                                     // (in front of pos: x0 never passes an x that was asked for)
        for (; k < nc; k++) {
            const uint32_t w = *(const reduce::rd_u32u *)(cg + 4 * k), op = w & 15u, len = w >> 4;
            if (op == 0 || op == 7 || op == 8) {
                if (x < x0 + len) {
                    const uint32_t yi = q0 + (uint32_t)(x - x0);
                    cls = read_class(sq, yi);
                    q = has_q ? ql[yi] : 0u;
                    return true;
                }
                x0 += len; q0 += len;
            } else if (op == 2 || op == 3) {
                if (x < x0 + len) return false;
                x0 += len;
            } else if (op == 1 || op == 4) q0 += len;
        }
        return false;
    }
};

// Rules W, V' and X at one column of a mate r of a pair whose other mate is o: walk_record's functor (gce_errprof.hpp), so that r is walked
// as count_record walks a record alone.  is_b: r is the later of the two in the file.  A column that an M / = / X op of o covers is shared:
// add2(row, cls) takes r's count of rule X, and add(row, cls) r's count of rule V' if r is the one rule V' counts.  Every other column, every
// insertion and every deletion is rule W's.  shared, differ: rule V's counters, added to by the later mate's walk alone.  Under a mask (rule
// Y, the column's `masked`) both mates add OVL_MASKED to the overlap table at a masked shared column and the mate rule V' counts adds MASKED
// to the primary one, so the fragment is still counted once and shared / differ are what they are without a mask.
template <class ADD, class ADD2> struct MateColumn {
    ADD &add; ADD2 &add2; Cursor oc; bool is_b; uint32_t &shared, &differ;
    EP_HD void operator()(const Params &P, const Column &c) {
        uint32_t ob = 0, oq = 0;
        const bool both = oc.at(c.x, ob, oq);                                         // (in front of this mate's loads: its base is not live across the cursor's loop)
        const uint32_t mq = c.q(), rc = c.rc(), bc = c.bc();
        uint32_t adj = mq;
        if (both) {
            // ---- rule X: this mate's count in the overlap table
            uint32_t xc;
            if (c.lowq(P, mq) || (oc.has_q && (int32_t)oq < P.min_baseq)) xc = OVL_LOWQ;
            else if (bc > 3 || ob > 3 || rc > 3) xc = OVL_UNUSABLE;
            else if (bc == ob) xc = bc == rc ? (uint32_t)OVL_AGREE_REF : (uint32_t)OVL_AGREE_ALT;
            else if (ob == rc || bc == rc) xc = base_class(rc, bc, c.rev);
            else xc = OVL_DIFF_OTHER;
            add2(c.row, c.masked ? OVL_MASKED : xc);
            // ---- rule V': which of the two the primary table counts, and at which quality
            const uint32_t qa = is_b ? oq : mq, qb = is_b ? mq : oq;
            bool mine;
            if (bc == ob) { mine = !is_b; adj = qa + qb < FP_Q_CAP ? qa + qb : FP_Q_CAP; }
            else { mine = is_b ? qa < qb : qa >= qb; adj = (4u * mq) / 5u; }
            if (is_b) { shared++; differ += bc != ob; }
            if (!mine) return;
        }
        add(c.row, EP_PRIMARY(c, P, adj, rc, bc));
    }
};
// without a mask (M is not read), and under the bitmap M
template <class ADD, class ADD2> EP_HD void paired_walk(const uint8_t *r, const uint8_t *o, bool is_b, const Params &P, const calmd::Ref &ref, const reduce::Sites &S, uint32_t first,
                                                        uint32_t lane, uint32_t nlanes, ADD &add, ADD2 &add2, uint32_t &shared, uint32_t &differ) {
    MateColumn<ADD, ADD2> at{add, add2, Cursor(o), is_b, shared, differ};
    walk_record<false>(r, P, ref, S, first, lane, nlanes, at, Mask{nullptr});
}
template <class ADD, class ADD2> EP_HD void paired_walk(const uint8_t *r, const uint8_t *o, bool is_b, const Params &P, const calmd::Ref &ref, const reduce::Sites &S, uint32_t first,
                                                        uint32_t lane, uint32_t nlanes, ADD &add, ADD2 &add2, uint32_t &shared, uint32_t &differ, const Mask &M) {
    MateColumn<ADD, ADD2> at{add, add2, Cursor(o), is_b, shared, differ};
    walk_record<true>(r, P, ref, S, first, lane, nlanes, at, M);
}

#undef EP_HD

}  // namespace errprof

// k_fragerr_count's LDS is k_err_count's: two planes of EP_PLANE 32-bit counters, 80 640 bytes, 2 blocks of 8 waves a CU.  Here one plane
// belongs to the primary table and one to the overlap table, so the two entries of a 32-lane LDS lane group share a plane (DESIGN.md 4j
// measured one plane as fast as two).  Row stride EP_CLS 21 for both: the 16 lanes of an entry, on 16 consecutive cycles, fall on 16
// different banks.
// The 32-bit counters cannot wrap within one launch.  Per table, every add reads a byte of the entries no other add to that table reads: in
// the primary table the quality byte of the counted base (at a shared column the one mate that rule V' counts adds, at its own base) or the
// low byte of the CIGAR word of a D; in the overlap table each mate adds once per base of its own, that base's quality byte.  So a launch
// adds fewer than 2^32 times to either table while the window and the pending records together are shorter than 2^32 bytes;
// gce_fragerr::process launches the direct kernel otherwise.
static_assert(2u * EP_PLANE * 4u <= EP_LDS_PER_CU / EP_BLOCKS_PER_CU, "k_fragerr_count's planes must leave the CU its 2 blocks of 8 waves");

#ifndef GCE_FRAGERR_HOST_CHECK

namespace {

// what k_reduce_scan over ErrScan left in meta: the first interval (0 without a BED), or EP_NONE for a record that is skipped or touches none
struct FragerrRead {
    errprof::Params P;
    __device__ bool operator()(const uint8_t *r, uint32_t m, uint32_t &first, reduce::Core &C) const {
        first = m;
        return m != EP_NONE && reduce::rule_e(r, 4ull + rb32(r), P.n_ref, P.min_mapq, P.exclude, C) == reduce::ELIGIBLE;
    }
};

// 16 lanes per entry, 32 entries per step; block b takes the entries [32 (b + k gridDim.x), + 32) of the join, k = 0, 1, ...
// MASK: none, or one errprof::Mask for rule Y (MASKED and OVL_MASKED go to memory, as in k_err_count)
template <bool DIRECT, class... MASK> __global__ __launch_bounds__(EP_THREADS) void k_fragerr_count(FragView V, errprof::Params P, calmd::Ref ref, reduce::Sites S, const uint32_t *first,
                                                                                                    const uint32_t *partner, unsigned long long *counts, unsigned long long *ovl,
                                                                                                    unsigned long long *fm, MASK... mask) {
    __shared__ uint32_t s_tab[DIRECT ? 1 : 2 * EP_PLANE];
    const uint32_t slot = threadIdx.x >> 4, sub = threadIdx.x & 15u;
    if (!DIRECT) {
        for (uint32_t i = threadIdx.x; i < 2 * EP_PLANE; i += EP_THREADS) s_tab[i] = 0u;
        __syncthreads();
    }
    ErrAdd<DIRECT, sizeof...(MASK) != 0> add{s_tab, counts}, add2{s_tab + (DIRECT ? 0u : EP_PLANE), ovl};
    uint32_t shared = 0, differ = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * EP_STEP_RECS + slot; e < V.n; e += (uint64_t)gridDim.x * EP_STEP_RECS) {
        const uint32_t pc = partner[e];
        if (pc == FP_SKIP || pc == FP_DEFER) continue;
        const uint32_t f = first[e];
        if (f == EP_NONE) continue;
        const uint8_t *r = V.rec(e);
        if (pc == FP_ALONE) errprof::count_record(r, P, ref, S, f, sub, 16u, add, mask...);
        else errprof::paired_walk(r, V.rec(pc & ~FP_IS_B), (pc & FP_IS_B) != 0, P, ref, S, f, sub, 16u, add, add2, shared, differ, mask...);
    }
    if (!DIRECT) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 2 * EP_PLANE; i += EP_THREADS) {
            const uint32_t v = s_tab[i];
            if (v) {
                const uint32_t t = i >= EP_PLANE ? 1u : 0u, ii = i - t * EP_PLANE, prow = ii / EP_CLS, cls = ii - prow * EP_CLS, seg = prow / EP_CYC, c0 = prow - seg * EP_CYC;
                atomicAdd((t ? ovl : counts) + (seg * EP_MAX_CYCLE + c0) * EP_ROW + cls, (unsigned long long)v);
            }
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) { shared += __shfl_xor(shared, d); differ += __shfl_xor(differ, d); }
    if (lane_id() == 0) {
        if (shared) atomicAdd(fm + FM_SHARED, (unsigned long long)shared);
        if (differ) atomicAdd(fm + FM_DIFFER, (unsigned long long)differ);
    }
}

}  // namespace

struct gce_fragerr : ErrSession {                                                     // counts: two blocks of EP_COUNTERS totals, the primary table and the overlap table
    MateJoin J; int cb_rc = GCE_OK;
    std::string needs() const override {
        return "gce_bam_error_profile_fragments needs the reference bases (" + std::to_string(ref_bytes) + " bytes) + 1152 KiB of counters, a join table (" + std::to_string(J.table_bytes()) +
               " bytes) and an arena (" + std::to_string(J.arena_bytes()) + " bytes)" + varmask_needs(mask_bytes);
    }
    int process(const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end, bool final);
};

// One join (MateJoin::run) with k_fragerr_count between join and carry.  end: the bytes of the window
int gce_fragerr::process(const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end, bool final) {
    const bool wide = ((end + J.arena[J.cur].cap) >> 32) != 0;                        // (the no-wrap argument of the planes does not hold)
    return J.run(this, "gce_bam_error_profile_fragments", FragerrRead{P}, u, off, n_rec, final, [&](const FragView &V, uint64_t N, const uint32_t *first, const uint32_t *partner, unsigned long long *fm) {
        const unsigned nb = (unsigned)std::min<uint64_t>((N + EP_STEP_RECS - 1) / EP_STEP_RECS, EP_GRID);
        unsigned long long *c = counts.as<unsigned long long>();
        dispatch(direct || wide, [&](auto D, auto... m) {
            hipLaunchKernelGGL((k_fragerr_count<decltype(D)::value, decltype(m)...>), dim3(nb), dim3(EP_THREADS), 0, s, V, P, ref(), sites(), first, partner, c, c + EP_COUNTERS, fm, m...);
        });
        return true;
    });
}

extern "C" {

int gce_fragerr_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_fragerr **out) {
    if (out) *out = nullptr;
    if (options & ~(uint32_t)(GCE_FRAGERR_DIRECT | GCE_FRAGERR_WEAK_HASH)) return GCE_ERR_INVALID;
    const int rc = rd_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options & (uint32_t)GCE_FRAGERR_DIRECT, (uint32_t)GCE_FRAGERR_DIRECT, out);
    if (rc == GCE_OK) (*out)->J.weak = (options & GCE_FRAGERR_WEAK_HASH) != 0;
    return rc;
}
void gce_fragerr_destroy(gce_fragerr *p) {
    if (!p) return;
    (void)hipSetDevice(p->device); (void)hipStreamSynchronize(p->s);
    p->J.release();
    rd_destroy(p, {&p->blob, &p->tab, &p->counts, &p->mask});
}
const char *gce_fragerr_error(gce_fragerr *p) { return p ? p->err.c_str() : ""; }

// the reference, once, first of all, as gce_errprof_set_ref takes it
int gce_fragerr_set_ref(gce_fragerr *p, int32_t n_ref, const char *const *seq, const int64_t *len) { return ep_set_ref(p, n_ref, seq, len); }

// rule B's intervals, once, behind the reference and in front of the first window, as gce_errprof_set_sites takes them.  Both counter blocks
// and the join's device words are made and zeroed.
int gce_fragerr_set_sites(gce_fragerr *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end) {
    int rc = ep_set_sites(p, "gce_fragerr_set_sites", n_intervals, tid, start, end, 2ull * EP_COUNTERS * 8ull);
    if (rc != GCE_OK) return rc;
    p->sites_set = false;
    if ((rc = p->J.init(p)) != GCE_OK) return rc;
    p->sites_set = true;
    return GCE_OK;
}

// rule Y's mask, a chunk of it, as gce_errprof_set_mask takes it: class 21 of the primary table is MASKED, of the overlap table OVL_MASKED
int gce_fragerr_set_mask(gce_fragerr *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end) { return ep_set_mask(p, n, tid, start, end); }

// the next piece of the file, as gce_errprof_window takes it; *errprof_s: the seconds of the scan, the join and the count, added to.
// GCE_ERR_INVALID names the lowest malformed record, else the first record that lies in front of its predecessor, counting from 0 over the file.
int gce_fragerr_window(gce_fragerr *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                       int32_t n_ref, int32_t last, double *errprof_s) {
    if (!p) return GCE_ERR_INVALID;
    p->cb_rc = GCE_OK;
    const int rc = rd_window(p, ErrScan{p->P, p->ref(), p->sites()}, p->P.n_ref, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, errprof_s,
                             [&](const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end) { p->cb_rc = p->process(u, off, n_rec, end, last != 0); return p->cb_rc == GCE_OK; });
    return rc != GCE_OK ? rc : p->cb_rc;
}

// after the last window: what is still pending is counted alone; counters[0..9] as gce_errprof_finish gives them, [10] pairs, [11] shared
// columns, [12] those whose classes differ, [13] ambiguous candidates, [14] records carried across a window boundary; counts_out,
// overlap_out: room for 3 x 1024 x 24 uint64 each
int gce_fragerr_finish(gce_fragerr *p, int64_t counters[15], uint64_t *counts_out, uint64_t *overlap_out) {
    if (!p || !p->sites_set || !counters || !counts_out || !overlap_out) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    int rc = p->process(nullptr, nullptr, 0, 0, true);
    if (rc != GCE_OK) return rc;
    if ((rc = ep_finish(p, ErrScan::NSKIP, counters, {counts_out, overlap_out}, EP_COUNTERS * 8ull)) != GCE_OK) return rc;
    unsigned long long f[FM_WORDS];
    RDCHK(hipMemcpyAsync(f, p->J.fm.p, sizeof f, hipMemcpyDeviceToHost, s)); RDCHK(hipStreamSynchronize(s));
    counters[10] = (int64_t)f[FM_PAIRS]; counters[11] = (int64_t)f[FM_SHARED]; counters[12] = (int64_t)f[FM_DIFFER]; counters[13] = (int64_t)f[FM_AMBIG]; counters[14] = (int64_t)f[FM_DEFER];
    return GCE_OK;
}

}  // extern "C"
#endif  // GCE_FRAGERR_HOST_CHECK
