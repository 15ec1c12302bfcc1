// gce_ovlmerge.hpp — rule V's decision written into the records: the QUAL bytes of overlapping mates rewritten so that a plain pileup of the
// file counts every fragment once (gce_bam_merge_overlap).  The file is streamed as the sort streams it (gce_sort_window,
// gce_sort.hpp), which leaves every record resident with its offset.  After the last window (gce_sort_overlap_finish):
//   k_ovl_check    one thread per record: the lowest record whose fields overrun its block_size (atomicMin), rule E's refusal
//   the join       k_frag_prep / k_frag_join of gce_matejoin.hpp over all records at once: no pending arena, nothing deferred, so the result
//                  cannot depend on the windows.  OvlRead is the pass's READ: rule E from the record itself, no scan meta.  Rule P is the
//                  join's own check
//   k_ovl_merge    16 lanes per entry, launched over the LATER mate of every pair, so that a pair has one writer.  The group walks both
//                  CIGARs together with two cursors (ovlmerge::Cursor: op index, reference column, query offset), all 16 lanes alike: the
//                  per-op partner cursor DESIGN.md 4k left open.  Every stretch where both cursors sit inside an M / = / X op is a run of
//                  columns with two query offsets; the lanes take its columns 16 at a time: two nibble reads, two byte reads, at most two
//                  byte stores per column (rule Q), no CIGAR walk of a column's own.  The counters are reduced per wave
// and the resident buffer itself becomes the stream gce_sort_read hands out: no gather, no second copy of the records.
// ovlmerge::Cursor, shared_runs, rule_q and merge_pair are __host__ __device__: tests/overlap_host_check.hip runs them on the host against
// tests/pyovlmerge.py, the model of the rules.
#pragma once
#include <cstdint>
#include "gce_matejoin.hpp"

namespace ovlmerge {

#define OV_HD __host__ __device__ inline
#define OV_Q_MAX 93u

// One cursor over a record's CIGAR: the op that covers reference columns [x, xe), base: it is an M / = / X op whose first query offset is q
// (else a D or N op).  next() goes to the following op of either kind that has a column; live: there was one
struct Cursor {
    const uint8_t *cg; uint32_t nc, k, q; int64_t x, xe; bool base, live;
    OV_HD explicit Cursor(const reduce::Head &h) : cg(h.cg), nc(h.nc), k(0), q(0), x(h.pos), xe(h.pos), base(false), live(true) { next(); }
    OV_HD void next() {
        if (base) q += (uint32_t)(xe - x);
        x = xe; base = false;
        while (k < nc) {
            const uint32_t w = *(const reduce::rd_u32u *)(cg + 4 * k), op = w & 15u, len = w >> 4;
            k++;
            if (op == 0 || op == 7 || op == 8) { if (len) { base = true; xe = x + len; return; } }
            else if (op == 2 || op == 3) { if (len) { xe = x + len; return; } }
            else if (op == 1 || op == 4) q += len;
        }
        live = false;
    }
};

// Both CIGARs walked together: run(x, n, ya, yb) for every maximal stretch of n columns from x that an M / = / X op of both records covers,
// ya and yb the query offsets of its first column.  One step per op of either record
template <class RUN> OV_HD void shared_runs(const reduce::Head &ha, const reduce::Head &hb, RUN &&run) {
    Cursor A(ha), B(hb);
    while (A.live && B.live) {
        const int64_t lo = A.x > B.x ? A.x : B.x, hi = A.xe < B.xe ? A.xe : B.xe;
        if (lo < hi && A.base && B.base) run(lo, (uint32_t)(hi - lo), A.q + (uint32_t)(lo - A.x), B.q + (uint32_t)(lo - B.x));
        const bool step_a = A.xe <= B.xe, step_b = B.xe <= A.xe;
        if (step_a) A.next();
        if (step_b) B.next();
    }
}

// Rule Q at one shared column: a's and b's class and quality in, their new qualities out.  0: the column is left as it is (a quality of 0 or
// above 93), 1: the classes agree, 2: they do not
OV_HD uint32_t rule_q(uint32_t ca, uint32_t qa, uint32_t cb, uint32_t qb, uint32_t &na, uint32_t &nb) {
    na = qa; nb = qb;
    if (qa == 0 || qb == 0 || qa > OV_Q_MAX || qb > OV_Q_MAX) return 0u;
    if (ca == cb) { na = qa + qb < OV_Q_MAX ? qa + qb : OV_Q_MAX; nb = 0; return 1u; }
    if (qa >= qb) { na = (4u * qa) / 5u; nb = 0; } else { nb = (4u * qb) / 5u; na = 0; }
    return 2u;
}

// what a pair added to the counters; changed: bit 0 a byte of a differs afterwards, bit 1 one of b
struct Tally { uint32_t shared, differ, skipped, changed, no_qual; };

// Rule Q over the pair (a: the earlier record in the file; both eligible, r at block_size), by lane `lane` of the pair's `nlanes`: nothing but
// QUAL bytes is written.  no_qual is lane 0's alone
OV_HD void merge_pair(uint8_t *a, uint8_t *b, uint32_t lane, uint32_t nlanes, Tally &t) {
    const reduce::Head ha(a), hb(b);
    if (!ha.has_q() || !hb.has_q()) { if (lane == 0) t.no_qual++; return; }
    uint8_t *qla = a + (ha.ql - a), *qlb = b + (hb.ql - b);
    shared_runs(ha, hb, [&](int64_t, uint32_t n, uint32_t ya, uint32_t yb) {
        for (uint32_t j = lane; j < n; j += nlanes) {
            const uint32_t qa = qla[ya + j], qb = qlb[yb + j];
            uint32_t na, nb;
            const uint32_t kind = rule_q(reduce::read_class(ha.sq, ya + j), qa, reduce::read_class(hb.sq, yb + j), qb, na, nb);
            t.shared++; t.differ += kind == 2u; t.skipped += kind == 0u;
            if (na != qa) { qla[ya + j] = (uint8_t)na; t.changed |= 1u; }
            if (nb != qb) { qlb[yb + j] = (uint8_t)nb; t.changed |= 2u; }
        }
    });
}

#undef OV_HD

}  // namespace ovlmerge

#ifndef GCE_OVLMERGE_HOST_CHECK

namespace {

// the pass's device words
enum { OM_BAD = 0, OM_SHARED, OM_DIFFER, OM_SKIPPED, OM_CHANGED, OM_NO_QUAL, OM_WORDS = 8 };
// k_ovl_merge's grid: 16 entries per block of 256 threads, OV_GRID_BLOCKS blocks at most, the rest by grid stride
#define OV_GRID_BLOCKS 2048u

// rule E's refusal: the lowest record with block_size < 32 or fields that overrun it (the index put every record whole inside [0, end))
__global__ __launch_bounds__(256) void k_ovl_check(const uint8_t *u, const uint64_t *off, uint64_t n, uint64_t end, unsigned long long *om) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = off[i], avail = a < end ? end - a : 0;
    bool bad = avail < 36;
    if (!bad) {
        const uint8_t *r = u + a;
        const uint64_t bs = rb32(r);
        const int32_t lseq = (int32_t)rb32(r + 20);
        bad = bs < 32 || 4 + bs > avail || lseq < 0 || 32ull + r[12] + 4ull * rb16(r + 16) + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > bs;
    }
    if (bad) atomicMin(om + OM_BAD, (unsigned long long)i);
}

// the join's READ without a scan in front of it: rule E from the record; every eligible record "touches" (first = 0)
struct OvlRead {
    int32_t min_mapq; uint32_t exclude;
    __device__ bool operator()(const uint8_t *r, uint32_t, uint32_t &first, reduce::Core &C) const {
        const bool ok = reduce::rule_e(r, 4ull + rb32(r), 0x7FFFFFFF, min_mapq, exclude, C) == reduce::ELIGIBLE;
        first = ok ? 0u : RD_NONE;
        return ok;
    }
};

// 16 lanes per entry; an entry that is the later mate of a pair merges the pair, every other one does nothing
__global__ __launch_bounds__(256) void k_ovl_merge(uint8_t *u, const uint64_t *off, uint64_t n, const uint32_t *partner, unsigned long long *om) {
    const uint32_t sub = threadIdx.x & 15u;
    ovlmerge::Tally t = {0, 0, 0, 0, 0};
    uint32_t changed = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 4); e < n; e += (uint64_t)gridDim.x * 16u) {
        const uint32_t pc = partner[e];
        if (pc >= FP_SKIP || !(pc & FP_IS_B)) continue;
        t.changed = 0;
        ovlmerge::merge_pair(u + off[pc & ~FP_IS_B], u + off[e], sub, 16u, t);
        uint32_t c = t.changed;                                                       // (the pair's 16 lanes: a byte of a, a byte of b)
        c |= __shfl_xor(c, 1); c |= __shfl_xor(c, 2); c |= __shfl_xor(c, 4); c |= __shfl_xor(c, 8);
        if (sub == 0) changed += (c & 1u) + (c >> 1);
    }
    uint32_t v[5] = {t.shared, t.differ, t.skipped, changed, t.no_qual};
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int d = 32; d; d >>= 1) v[k] += __shfl_xor(v[k], d);
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < 5; k++) if (v[k]) atomicAdd(om + OM_SHARED + k, (unsigned long long)v[k]);
    }
}

// the join's session over the sort's resident records: its stream and its budget are the sort's
struct OvlSession : ReduceSession {
    MateJoin J; uint64_t rec_bytes = 0;
    std::string needs() const override {
        return "gce_bam_merge_overlap is in-core and needs the inflated record bytes (" + std::to_string(rec_bytes) + "), 8 bytes per record and a join table (" +
               std::to_string(J.table_bytes()) + " bytes)";
    }
    ~OvlSession() { J.release(); }
};

}  // namespace

extern "C" {

// in front of the first gce_sort_window: the object is gce_bam_merge_overlap's (its out-of-memory message says so)
int gce_sort_overlap_begin(gce_sort *b) {
    if (!b || b->passes || b->calmd || b->cm_stream || b->sam_text || b->n || b->out_n) return GCE_ERR_INVALID;
    b->overlap = true;
    return GCE_OK;
}

// After the last gce_sort_window: the malformed-record test, the join over all records, rule Q in place; the resident buffer becomes the
// stream gce_sort_read hands out.  options: GCE_OVERLAP_WEAK_HASH.  counts: records, pairs, pairs without qualities, ambiguous candidates,
// shared columns, those that disagree, those left as they are, records changed.  *bad_rec: the first record whose tid the header does not
// have (-1: none; nothing is done then).  codes / piece_bytes: as gce_sort_finish takes them.
int gce_sort_overlap_finish(gce_sort *b, int32_t min_mapq, uint32_t exclude_flags, uint32_t options, int32_t codes, uint64_t piece_bytes, int64_t counts[8], int64_t *bad_rec,
                            uint64_t *out_bytes) {
    if (!b || !b->overlap || !counts || !bad_rec || !out_bytes || codes > 1 || (options & ~(uint32_t)GCE_OVERLAP_WEAK_HASH)) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    SCHK(hipStreamSynchronize(s));
    b->w.release();                                                                   // (the last window is done with)
    *out_bytes = 0;
    for (int k = 0; k < 8; k++) counts[k] = 0;
    int64_t sc[3];
    int rc = sort_counts(b, sc, bad_rec);
    counts[0] = (int64_t)b->n;
    if (rc != GCE_OK || b->n == 0 || *bad_rec >= 0) return rc;
    b->key.release(); b->size.release();                                              // (nothing is sorted)
    const uint64_t n = b->n;
    uint8_t *u = b->rec.as<uint8_t>(); const uint64_t *off = (const uint64_t *)b->off.p;
    OvlSession ps; OvlSession *p = &ps;
    p->device = b->device; p->s = s; p->budget = b->budget; p->rec_bytes = b->rec_n; p->J.weak = (options & GCE_OVERLAP_WEAK_HASH) != 0;
    auto failed = [&](int code) { return sfail(b, code, p->err); };
    ScopedBuf omb;
    if (!sort_room(b, 512)) return sort_oom(b, "the pass's counters", 512);
    SCHK(omb.ensure(OM_WORDS * 8));
    unsigned long long *om = omb.as<unsigned long long>();
    const unsigned long long init[OM_WORDS] = {~0ull};
    SCHK(hipMemcpyAsync(om, init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_ovl_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint8_t *)u, off, n, b->rec_n, om);
    SCHK(hipGetLastError());
    unsigned long long h[OM_WORDS];
    SCHK(hipMemcpyAsync(h, om, 8, hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    if (h[OM_BAD] != ~0ull) {
        char m[160]; snprintf(m, sizeof m, "BAM record %llu (counting from 0): its fields overrun its block_size", h[OM_BAD]);
        return sfail(b, GCE_ERR_INVALID, m);
    }
    if ((rc = p->J.init(p)) != GCE_OK) return failed(rc);
    rc = p->J.run(p, "gce_bam_merge_overlap", OvlRead{min_mapq, exclude_flags}, u, off, n, true, [&](const FragView &, uint64_t N, const uint32_t *, const uint32_t *partner, unsigned long long *) {
        hipLaunchKernelGGL(k_ovl_merge, dim3((unsigned)std::min<uint64_t>((N + 15) / 16, OV_GRID_BLOCKS)), dim3(256), 0, s, u, off, N, partner, om);
        return true;
    });
    if (rc != GCE_OK) return failed(rc);
    unsigned long long f[FM_WORDS];
    SCHK(hipMemcpyAsync(f, p->J.fm.p, sizeof f, hipMemcpyDeviceToHost, s)); SCHK(hipMemcpyAsync(h, om, sizeof h, hipMemcpyDeviceToHost, s));
    SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    counts[1] = (int64_t)f[FM_PAIRS]; counts[2] = (int64_t)h[OM_NO_QUAL]; counts[3] = (int64_t)f[FM_AMBIG]; counts[4] = (int64_t)h[OM_SHARED]; counts[5] = (int64_t)h[OM_DIFFER];
    counts[6] = (int64_t)h[OM_SKIPPED]; counts[7] = (int64_t)h[OM_CHANGED];
    p->J.release(); b->off.release();
    // ---- the resident records are the output stream
    SCHK(hipMemsetAsync(u + b->rec_n, 0, 64, s));                                    // (the deflate kernels may look a few bytes ahead; sort_take left 64 bytes of room)
    SCHK(hipStreamSynchronize(s));
    std::swap(b->out, b->rec);
    b->out_n = b->rec_n; *out_bytes = b->rec_n;
    if (codes >= 0 && piece_bytes) return sort_deflate_bufs(b, std::min<uint64_t>(piece_bytes, b->rec_n));
    return GCE_OK;
}

}  // extern "C"
#endif  // GCE_OVLMERGE_HOST_CHECK
