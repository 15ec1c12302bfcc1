// gce_errqual.hpp — the error profile by reported base quality, counted on the GPU (gce_bam_error_profile_quality).
//
// Of the bases a file reports at quality q, how many differ from the reference: what GATK's recalibration table, Picard
// QualityScoreDistribution beside its artifact metrics or `fgbio ErrorRateByReadPosition` split by quality answer on the host.  The pass is
// gce_bam_error_profile's (gce_errprof.hpp) with another row: rules E, G, W, B and Y unchanged -- errprof::scan_record under
// the existing k_reduce_scan<ErrScan>, errprof::walk_record as the one CIGAR loop -- and the counter
//   counts[((segment * 96 + bucket) * 24) + class]            3 x 96 x 24 64-bit totals, 55 296 bytes
// where the bucket is rule Q's: the QUAL byte of the event's query base, 0..93 as it is, 94 for every other byte, 95 for every event of a
// record without qualities (QUAL[0] == 0xFF).  A column's byte is QUAL[yi]; an inserted base's its own; a deletion's the byte of the query
// base in front of it (the first, when there is none), the base whose cycle 4j charges.  QUAL is stored in reference orientation like SEQ:
// on the reverse strand the cycle is mirrored, the quality index is not.  Class 21 is MASKED as in 4m, 22 and 23 are zero.
//
// The walk hands its functor the cycle row for I and D (at.add(row, cls), row = segment * 1024 + cycle - 1); the query index comes back out
// of it (c0 = row & 1023, yi = rev ? l_seq - 1 - c0 : c0), so errprof::walk_record is untouched and the other passes' kernels compile to
// what they compiled to.
//
// k_qual_count<DIRECT, MASK...>: k_err_count's shape, 16 lanes per record, 32 records per step of a block of 512 threads, a fixed grid whose
// blocks stride over the window's records.  The row is a property of the COLUMN and real files have very few values of it (binned Illumina
// qualities are four numbers), so with most bases matching the reference the 64 adds of a wave instruction fall on about a dozen addresses:
// the worst contention of the family.  The whole table fits a block: EQ_COUNTERS 32-bit counters in LDS at the memory table's own index
// (27 648 bytes, MASKED included: stride 24 costs nothing here, where lanes meet on addresses, not on banks), zeroed once, every add a
// 32-bit LDS atomic, sent once per block with one 64-bit atomic per non-zero counter.  Two aggregations in front of the table were built
// and measured against it on the contended file -- a run of (index, count) in each lane's registers, and the wave's equal keys under
// readfirstlane and ballot as one atomic of the popcount -- and both were slower than the plain table, which is within 7 % of 4j's
// kernel: same-address LDS atomics are not what this kernel waits for (DESIGN.md 4o has the figures; the variants are not in the tree).
// k_qual_count<true> (GCE_ERRQUAL_DIRECT) has no LDS: every add is a 64-bit global atomic.
// errqual::bucket, the column functor and errqual::count_record are __host__ __device__: tests/errqual_host_check.hip runs them on the host
// against tests/pyerrqual.py, the model of the rules.
#pragma once
#include <cstdint>
#include "gce_errprof.hpp"

namespace errqual {

#define EQ_HD __host__ __device__ inline

#define EQ_BUCKETS 96u                                                                // rule Q: 0..93 the byte, 94 the rest, 95 no qualities
#define EQ_TOP 94u
#define EQ_NOQ 95u
#define EQ_ROWS (3u * EQ_BUCKETS)
#define EQ_COUNTERS (EQ_ROWS * EP_ROW)

// rule Q's bucket of a QUAL byte
EQ_HD uint32_t bucket(uint32_t b) { return b <= 93u ? b : EQ_TOP; }

// Rule W under rule Q: the walk's functor.  out(row, cls): counter row * 24 + cls += 1, row = segment * 96 + bucket < EQ_ROWS
template <class ADD> struct ColumnQ {
    ADD &out; const uint8_t *ql; uint32_t lseq; bool has_q, rev;
    EQ_HD uint32_t row_of(uint32_t seg, uint32_t yi) const { return seg * EQ_BUCKETS + (has_q ? bucket(ql[yi]) : EQ_NOQ); }
    // a column of an M / = / X op: its class is 4j's, its row its own quality's (LOWQ too)
    EQ_HD void operator()(const errprof::Params &P, const errprof::Column &c) {
        using namespace errprof;                                                      // (EP_PRIMARY names base_class and the classes)
        out(row_of(c.row >> 10, c.yi), EP_PRIMARY(c, P, c.q(), c.rc(), c.bc()));
    }
    // an inserted base or a deletion, which the walk charges to the cycle row `row`: the query index back out of the cycle
    EQ_HD void add(uint32_t row, uint32_t cls) {
        const uint32_t c0 = row & (EP_MAX_CYCLE - 1u);
        out(row_of(row >> 10, rev ? lseq - 1u - c0 : c0), cls);
    }
};

// Rules W and Q (and Y, with a mask) for a record the scan kept, by lane `lane` of `nlanes`.  add(row, cls): counter row * 24 + cls += 1,
// row < EQ_ROWS, cls < 21 (< 22 with a mask).  Reads stay inside the record: every query index is below l_seq (errprof::walk_record)
template <class ADD, class... MASK> EQ_HD void count_record(const uint8_t *r, const errprof::Params &P, const calmd::Ref &ref, const reduce::Sites &S, uint32_t first, uint32_t lane,
                                                            uint32_t nlanes, ADD &add, const MASK &...mask) {
    const errprof::Head h(r);
    ColumnQ<ADD> at{add, h.ql, (uint32_t)h.lseq, h.has_q(), (h.flag & 16u) != 0};
    if constexpr (sizeof...(MASK) != 0) errprof::walk_record<true>(r, P, ref, S, first, lane, nlanes, at, mask...);
    else errprof::walk_record<false>(r, P, ref, S, first, lane, nlanes, at, errprof::Mask{nullptr});
}

#undef EQ_HD

}  // namespace errqual

#define EQ_THREADS 512u
#define EQ_STEP_RECS 32u
#define EQ_GRID 512u
// The 32-bit counters of the block's table cannot wrap within one launch: every add reads a byte of the window no other add reads (a
// quality byte for a base of M = X I, the low byte of the CIGAR word for a D), so a launch adds fewer than 2^32 times in all while the
// window is shorter than 2^32 bytes; gce_errqual_window launches the direct kernel for a longer one, as gce_errprof_window does.
static_assert(EQ_STEP_RECS * 16u == EQ_THREADS && EQ_COUNTERS * 4u <= (64u << 10) && EP_MASKED < EP_ROW, "k_qual_count's layout: the table fits a block's 64 KB of LDS");

#ifndef GCE_ERRQUAL_HOST_CHECK

namespace {

// an add of k_qual_count<false>: into the block's table, whose index is the memory table's.  The table is the block's: workgroup scope
struct QualAddTab {
    uint32_t *tab;
    __device__ __forceinline__ void operator()(uint32_t row, uint32_t cls) { atomicAdd(tab + row * EP_ROW + cls, 1u); }
};
// ... and of k_qual_count<true>: to memory
struct QualAddDirect {
    unsigned long long *counts;
    __device__ __forceinline__ void operator()(uint32_t row, uint32_t cls) { atomicAdd(counts + row * EP_ROW + cls, 1ull); }
};

// 16 lanes per record, 32 records per step; block b takes the records [32 (b + k gridDim.x), + 32) of the window, k = 0, 1, ...
// MASK: none, or one errprof::Mask for rule Y.  No barrier stands in the record loop: the slots of a block run different numbers of records
template <bool DIRECT, class... MASK> __global__ __launch_bounds__(EQ_THREADS) void k_qual_count(const uint8_t *u, const uint64_t *off, uint64_t n, errprof::Params P, calmd::Ref ref, reduce::Sites S,
                                                                                                 const uint32_t *meta, unsigned long long *counts, MASK... mask) {
    __shared__ uint32_t s_tab[DIRECT ? 1 : EQ_COUNTERS];
    const uint32_t slot = threadIdx.x >> 4, sub = threadIdx.x & 15u;
    if (!DIRECT) {
        for (uint32_t i = threadIdx.x; i < EQ_COUNTERS; i += EQ_THREADS) s_tab[i] = 0u;
        __syncthreads();
    }
    for (uint64_t j = (uint64_t)blockIdx.x * EQ_STEP_RECS + slot; j < n; j += (uint64_t)gridDim.x * EQ_STEP_RECS) {
        const uint32_t first = meta[j];
        if (first == EP_NONE) continue;
        if (DIRECT) {
            QualAddDirect add{counts};
            errqual::count_record(u + off[j], P, ref, S, first, sub, 16u, add, mask...);
        } else {
            QualAddTab add{s_tab};
            errqual::count_record(u + off[j], P, ref, S, first, sub, 16u, add, mask...);
        }
    }
    if (!DIRECT) {                                                                    // (no thread leaves the loop by a return: every one arrives)
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < EQ_COUNTERS; i += EQ_THREADS) {
            const uint32_t v = s_tab[i];
            if (v) atomicAdd(counts + i, (unsigned long long)v);
        }
    }
}

}  // namespace

struct gce_errqual : ErrSession {                                                     // counts: EQ_COUNTERS totals
    std::string needs() const override {
        return "gce_bam_error_profile_quality needs the reference bases (" + std::to_string(ref_bytes) + " bytes) + " + std::to_string(EQ_COUNTERS * 8ull) + " bytes of counters" +
               varmask_needs(mask_bytes);
    }
};

extern "C" {

int gce_errqual_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_errqual **out) {
    return rd_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options, (uint32_t)GCE_ERRQUAL_DIRECT, out);
}
void gce_errqual_destroy(gce_errqual *p) { if (p) rd_destroy(p, {&p->blob, &p->tab, &p->counts, &p->mask}); }
const char *gce_errqual_error(gce_errqual *p) { return p ? p->err.c_str() : ""; }

// the reference, rule Y's mask and rule B's intervals, in gce_errprof's order and with its rules (ep_set_ref, ep_set_mask, ep_set_sites)
int gce_errqual_set_ref(gce_errqual *p, int32_t n_ref, const char *const *seq, const int64_t *len) { return ep_set_ref(p, n_ref, seq, len); }
int gce_errqual_set_mask(gce_errqual *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end) { return ep_set_mask(p, n, tid, start, end); }
int gce_errqual_set_sites(gce_errqual *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end) {
    return ep_set_sites(p, "gce_errqual_set_sites", n_intervals, tid, start, end, EQ_COUNTERS * 8ull);
}

// the next piece of the file, as gce_errprof_window takes it, under gce_errprof's scan; *errprof_s: the seconds of the scan and
// k_qual_count, added to
int gce_errqual_window(gce_errqual *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                       int32_t n_ref, int32_t last, double *errprof_s) {
    if (!p) return GCE_ERR_INVALID;
    const calmd::Ref ref = p->ref();
    const reduce::Sites S = p->sites();
    return rd_window(p, ErrScan{p->P, ref, S}, p->P.n_ref, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, errprof_s, [&](const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end) {
        const unsigned nb = (unsigned)std::min<uint64_t>((n_rec + EQ_STEP_RECS - 1) / EQ_STEP_RECS, EQ_GRID);
        p->dispatch(p->direct || (end >> 32), [&](auto D, auto... m) {
            hipLaunchKernelGGL((k_qual_count<decltype(D)::value, decltype(m)...>), dim3(nb), dim3(EQ_THREADS), 0, p->s, u, off, n_rec, p->P, ref, S, (const uint32_t *)p->meta.p,
                               p->counts.as<unsigned long long>(), m...);
        });
        return true;
    });
}

// after the last window: counters[0] records, [1..8] the skip counters of rule E in its order, [9] eligible; counts_out: room for
// 3 x 96 x 24 uint64
int gce_errqual_finish(gce_errqual *p, int64_t counters[10], uint64_t *counts_out) {
    if (!p || !p->sites_set || !counters || !counts_out) return GCE_ERR_INVALID;
    return ep_finish(p, ErrScan::NSKIP, counters, {counts_out}, EQ_COUNTERS * 8ull);
}

}  // extern "C"
#endif  // GCE_ERRQUAL_HOST_CHECK
