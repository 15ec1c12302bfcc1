// gce_errsup.hpp — residual error by consensus support, counted on the GPU (gce_bam_error_profile_support).
//
// Every consensus record this library writes carries FR:C, the forward-strand reads merged into it, and a duplex record RR:C as well (quirk
// A11).  A run at -s 1 followed by this pass gives the residual error of every (FR, RR) from one file: how many reads a family needs, and
// whether both strands are needed.  The pass is gce_bam_error_profile's (gce_errprof.hpp) with another row: rule E with a
// ninth skip, rules W, B and Y (the walk, the BED, the variant mask) unchanged -- errprof::count_record as it is -- and the counter
//   counts[((segment * 33 + f) * 33 + r) * 24 + class]        3 x 33 x 33 x 24 64-bit totals, 627 264 bytes
// where f and r are rule U's buckets of the forward and the reverse tag: 0 absent, 1..31 the value, 32 anything else.  Class 21 is MASKED as
// in 4m, class 22 RECORDS (one per eligible record the scan keeps), class 23 zero.
//
// Where the tag walk runs.  The scan (k_reduce_scan over SupScan, one thread per record) walks the optional fields once for rule E's ninth
// skip: a record whose walk is refused goes to n_bad_aux and gets EP_NONE.  The count kernel then REPEATS the walk, all 16 lanes of a record
// slot in step on bytes the scan has proven well formed, and every lane ends with (f, r) in registers.  The other choice, a second meta word
// behind an `if constexpr` hook of k_reduce_scan and rd_window, was not taken: it adds a buffer of 4 bytes per window record with its
// write, its read and its entry in the out-of-memory message, and touches the frame the other four passes are built on, to save a walk over
// a few dozen bytes that lie right behind the QUAL bytes the slot reads anyway (the 16 lanes load the same address: one request).  The frame
// is untouched; gce_reduce.hpp compiles to what it compiled to.
//
// k_sup_count<DIRECT, MASK...>: k_err_count's shape, 16 lanes per record, 32 records per step of a block of 512 threads, a fixed grid whose
// blocks stride over the window's records.  The row is the record's, not the column's, so all adds of a record meet in ONE row of 24
// counters.  The default keeps that row in LDS, private to the record slot (32 slots x 24 words = 3 KB a block: LDS does not limit
// occupancy as 4j's 80 KB of planes do): the lanes add with 32-bit LDS atomics, then lane `sub` takes classes sub and sub + 16 back with an
// exchange against 0 and sends at most one atomic per non-zero class, RECORDS among them: a 64-bit global atomic, or, for a row whose buckets
// are both below ES_LOW, an add to the block's table in LDS, which the block sends once at its end (below).  A 32-bit slot counter cannot
// wrap: a record adds once per query base and once per CIGAR op, fewer than 2^17 times.  k_sup_count<true> (GCE_ERRSUP_DIRECT) has no LDS:
// every add is a 64-bit global atomic.
// errsup::support, errsup::scan_record and the walk are __host__ __device__: tests/errsup_host_check.hip runs them on the host against
// tests/pyerrsup.py, the model of the rules.
#pragma once
#include <cstdint>
#include "gce_errprof.hpp"

namespace errsup {

#define ES_HD __host__ __device__ inline

#define ES_BUCKETS 33u                                                                // rule U: 0 absent, 1..31, 32 the rest
#define ES_TOP 32u
#define ES_ROWS (3u * ES_BUCKETS * ES_BUCKETS)
#define ES_COUNTERS (ES_ROWS * EP_ROW)
#define ES_RECORDS 22u                                                                // class 22: the eligible records the scan keeps
enum { ES_SKIP_BAD_AUX = errprof::EP_N_SKIP + 1, ES_N_SKIP = ES_SKIP_BAD_AUX };       // behind 4j's eight

// the two tags, each as the 16-bit little-endian word of its two characters
struct Tags { uint16_t fwd, rev; };
struct Support { uint32_t f, r; bool bad; };

// rule U's bucket of a value read with its type's sign
ES_HD uint32_t bucket(int64_t v) { return v >= 1 && v <= 31 ? (uint32_t)v : ES_TOP; }

// Rule U for one record whose core fields rule E has checked (r at its block_size): the optional fields from the end of QUAL to the end of the
// block, walked with calmd::field_bytes.  f, r: the bucket of the first field with the forward / the reverse tag, 0 when there is none or
// when that first field's type is not one of c C s S i I.  bad: the walk was refused while bytes remained (f and r are then what the walk
// had found).  No byte is read outside r[0, 4 + block_size).
ES_HD Support support(const uint8_t *r, const Tags &T) {
    Support s{0u, 0u, false};
    const uint8_t *c = r + 4;
    const uint32_t bs = *(const reduce::rd_u32u *)r, lq = c[8], nc = *(const reduce::rd_u16u *)(c + 12), lseq = *(const reduce::rd_u32u *)(c + 16);
    const uint8_t *end = c + bs, *p = c + 32 + lq + 4 * nc + (lseq + 1) / 2 + lseq;
    bool seen_f = false, seen_r = false;
    while (p < end) {
        uint64_t fs;
        if (!calmd::field_bytes(p, end, fs)) { s.bad = true; return s; }
        const uint32_t tag = *(const reduce::rd_u16u *)p;
        const bool is_f = !seen_f && tag == T.fwd, is_r = !seen_r && tag == T.rev;
        if (is_f || is_r) {
            const uint8_t type = p[2]; const uint8_t *v = p + 3;
            bool num = true; int64_t val = 0;
            if (type == 'c') val = (int8_t)v[0]; else if (type == 'C') val = v[0];
            else if (type == 's') val = (int16_t) * (const reduce::rd_u16u *)v; else if (type == 'S') val = *(const reduce::rd_u16u *)v;
            else if (type == 'i') val = (int32_t) * (const reduce::rd_u32u *)v; else if (type == 'I') val = *(const reduce::rd_u32u *)v;
            else num = false;
            const uint32_t b = num ? bucket(val) : 0u;
            if (is_f) { seen_f = true; s.f = b; }
            if (is_r) { seen_r = true; s.r = b; }
        }
        p += 3 + fs;
    }
    return s;
}

// One record: 4j's rule E with its eight skips (errprof::scan_record), then the ninth, n_bad_aux.  No byte is read outside
// r[0, min(avail, 4 + block_size)).
ES_HD void scan_record(const uint8_t *r, uint64_t avail, const errprof::Params &P, const Tags &T, const calmd::Ref &ref, const reduce::Sites &S, errprof::Rec &R) {
    errprof::scan_record(r, avail, P, ref, S, R);
    if (R.bad || R.skip) return;
    if (support(r, T).bad) { R.first = EP_NONE; R.skip = ES_SKIP_BAD_AUX; }
}

ES_HD uint32_t segment(const uint8_t *r) {
    const uint32_t flag = *(const reduce::rd_u16u *)(r + 4 + 14);
    return (flag & 0xC0u) == 0x40u ? 1u : (flag & 0xC0u) == 0x80u ? 2u : 0u;
}
// the row of an eligible record, < ES_ROWS
ES_HD uint32_t row_of(const uint8_t *r, const Support &s) { return (segment(r) * ES_BUCKETS + s.f) * ES_BUCKETS + s.r; }

// Rule W (and Y, with a mask) for a record the scan kept, by lane `lane` of `nlanes`: errprof::count_record with its row dropped, since every
// add of the record goes to the record's own row.  add(cls): the record's counter of class cls += 1, cls < 22; lane 0 adds RECORDS.
template <class ADD> struct RowAdd {
    ADD &add;
    ES_HD void operator()(uint32_t, uint32_t cls) { add(cls); }
};
template <class ADD, class... MASK> ES_HD void count_record(const uint8_t *r, const errprof::Params &P, const calmd::Ref &ref, const reduce::Sites &S, uint32_t first, uint32_t lane,
                                                            uint32_t nlanes, ADD &add, const MASK &...mask) {
    RowAdd<ADD> ra{add};
    if (lane == 0) add(ES_RECORDS);
    errprof::count_record(r, P, ref, S, first, lane, nlanes, ra, mask...);
}

#undef ES_HD

}  // namespace errsup

#define ES_THREADS 512u
#define ES_STEP_RECS 32u
#define ES_GRID 512u
// The block's table on top of the per-record reduce: the rows whose two buckets are both below ES_LOW (absent, 1 .. 7: the supports most
// records of a consensus output have, and the one row per segment of a file without tags) have 32-bit counters in LDS, 3 x 8 x 8 x 24 of them,
// 18 KB.  A slot's read-back adds such a row there instead of to memory, and the block sends its non-zero counters once, when it is done: a
// file whose records share a few rows otherwise sends every record's half dozen 64-bit atomics to the same dozen addresses (DESIGN.md 4n has
// the A/B; ES_LOW 0 builds the kernel without the table).  The 32-bit counters cannot wrap within one launch: every add reads a byte of the
// window no other add reads (a quality byte for a base of M = X I, the low byte of the CIGAR word for a D, the low byte of block_size for
// RECORDS), so a launch adds fewer than 2^32 times in all while the window is shorter than 2^32 bytes; gce_errsup_window launches the direct
// kernel for a longer one, as gce_errprof_window does.
#ifndef ES_LOW
#define ES_LOW 8u
#endif
#define ES_LOW_ROWS (3u * ES_LOW * ES_LOW)
static_assert(ES_STEP_RECS * 16u == ES_THREADS && ES_RECORDS < EP_ROW && EP_MASKED < ES_RECORDS, "k_sup_count's layout");
static_assert(ES_LOW <= ES_BUCKETS && (ES_STEP_RECS + ES_LOW_ROWS) * EP_ROW * 4u <= (64u << 10), "the slots' rows and the block's table fit a block's 64 KB of LDS");

#ifndef GCE_ERRSUP_HOST_CHECK

namespace {

// the scan of k_reduce_scan.  misc: [0] the lowest malformed record, [1..9] the skip counters in rule E's order, [10] eligible records
struct SupScan {
    typedef errprof::Rec Rec;
    static constexpr int NSKIP = errsup::ES_N_SKIP; static constexpr bool OPS = false;
    errprof::Params P; errsup::Tags T; calmd::Ref ref; reduce::Sites S;
    __device__ void operator()(const uint8_t *r, uint64_t avail, Rec &R) const { errsup::scan_record(r, avail, P, T, ref, S, R); }
};

// an add of k_sup_count<false>: into the record slot's row in LDS.  Wavefront scope is enough for it: the row is touched by the 16 lanes of
// its slot alone, which are lanes of one wave
struct SupAddSlot {
    uint32_t *row;
    __device__ __forceinline__ void operator()(uint32_t cls) { __hip_atomic_fetch_add(row + cls, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
};
// ... and of k_sup_count<true>: to the record's row in memory
struct SupAddDirect {
    unsigned long long *row;
    __device__ __forceinline__ void operator()(uint32_t cls) { atomicAdd(row + cls, 1ull); }
};

// The 16 lanes of a slot are a quarter of a wave and leave the walk at different times; what orders the read-back behind the slot's adds
// (and the next record's adds behind the read-back) is that they are lanes of ONE wave that take the same branches around the walk (j and
// `first` are the slot's): a wave has one instruction stream, so a lane that is done waits masked off where the walk's loops end, the
// exchange below is one instruction for all 16, issued behind every add of the walk, and the LDS executes the instructions of a wave in the
// order they were issued.  The fence and the (convergent) wave barrier keep the compiler from moving an LDS access across that point or
// making it depend on the lane.  No barrier instruction is needed, and none that spans waves may be used: the slots of a block run
// different numbers of records.
__device__ __forceinline__ void sup_slot_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// 16 lanes per record, 32 records per step; block b takes the records [32 (b + k gridDim.x), + 32) of the window, k = 0, 1, ...
// MASK: none, or one errprof::Mask for rule Y
template <bool DIRECT, class... MASK> __global__ __launch_bounds__(ES_THREADS) void k_sup_count(const uint8_t *u, const uint64_t *off, uint64_t n, errprof::Params P, errsup::Tags T, calmd::Ref ref,
                                                                                                reduce::Sites S, const uint32_t *meta, unsigned long long *counts, MASK... mask) {
    __shared__ uint32_t s_row[DIRECT ? 1 : ES_STEP_RECS * EP_ROW];
    __shared__ uint32_t s_low[DIRECT || !ES_LOW ? 1 : ES_LOW_ROWS * EP_ROW];
    const uint32_t slot = threadIdx.x >> 4, sub = threadIdx.x & 15u;
    uint32_t *mine = s_row + (DIRECT ? 0u : slot * EP_ROW);
    if (!DIRECT) {
        for (uint32_t i = sub; i < EP_ROW; i += 16u) mine[i] = 0u;
        if (ES_LOW) {
            for (uint32_t i = threadIdx.x; i < ES_LOW_ROWS * EP_ROW; i += ES_THREADS) s_low[i] = 0u;
            __syncthreads();
        }
        sup_slot_order();
    }
    for (uint64_t j = (uint64_t)blockIdx.x * ES_STEP_RECS + slot; j < n; j += (uint64_t)gridDim.x * ES_STEP_RECS) {
        const uint32_t first = meta[j];
        if (first == EP_NONE) continue;
        const uint8_t *r = u + off[j];
        const errsup::Support sp = errsup::support(r, T);
        unsigned long long *grow = counts + (uint64_t)errsup::row_of(r, sp) * EP_ROW;
        if (DIRECT) {
            SupAddDirect add{grow};
            errsup::count_record(r, P, ref, S, first, sub, 16u, add, mask...);
        } else {
            SupAddSlot add{mine};
            errsup::count_record(r, P, ref, S, first, sub, 16u, add, mask...);
            sup_slot_order();
            const bool low = ES_LOW && sp.f < ES_LOW && sp.r < ES_LOW;
            uint32_t *lrow = s_low + (low ? ((errsup::segment(r) * ES_LOW + sp.f) * ES_LOW + sp.r) * EP_ROW : 0u);
#pragma unroll
            for (uint32_t cls = sub; cls < EP_ROW; cls += 16u) {
                const uint32_t v = __hip_atomic_exchange(mine + cls, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                if (v) { if (low) atomicAdd(lrow + cls, v); else atomicAdd(grow + cls, (unsigned long long)v); }
            }
            sup_slot_order();
        }
    }
    if (!DIRECT && ES_LOW) {                                                          // (no thread leaves the loop by a return: every one arrives)
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < ES_LOW_ROWS * EP_ROW; i += ES_THREADS) {
            const uint32_t v = s_low[i];
            if (v) {
                constexpr uint32_t L = ES_LOW ? ES_LOW : 1u;
                const uint32_t lr = i / EP_ROW, cls = i - lr * EP_ROW, g = lr / (L * L), fr = lr - g * (L * L), f = fr / L, rv = fr - f * L;
                atomicAdd(counts + (uint64_t)((g * ES_BUCKETS + f) * ES_BUCKETS + rv) * EP_ROW + cls, (unsigned long long)v);
            }
        }
    }
}

}  // namespace

struct gce_errsup : ErrSession {                                                      // counts: ES_COUNTERS totals
    errsup::Tags T{0, 0};
    std::string needs() const override {
        return "gce_bam_error_profile_support needs the reference bases (" + std::to_string(ref_bytes) + " bytes) + " + std::to_string(ES_COUNTERS * 8ull) + " bytes of counters" +
               varmask_needs(mask_bytes);
    }
};

extern "C" {

// tags: four characters, the forward tag and the reverse tag (NULL: "FRRR")
int gce_errsup_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, const char *tags, gce_errsup **out) {
    if (!out) return GCE_ERR_INVALID;
    *out = nullptr;
    if (!tags) tags = "FRRR";
    if (strlen(tags) != 4) return GCE_ERR_INVALID;
    const int rc = rd_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options, (uint32_t)GCE_ERRSUP_DIRECT, out);
    if (rc != GCE_OK) return rc;
    (*out)->T = errsup::Tags{(uint16_t)((uint8_t)tags[0] | (uint8_t)tags[1] << 8), (uint16_t)((uint8_t)tags[2] | (uint8_t)tags[3] << 8)};
    return GCE_OK;
}
void gce_errsup_destroy(gce_errsup *p) { if (p) rd_destroy(p, {&p->blob, &p->tab, &p->counts, &p->mask}); }
const char *gce_errsup_error(gce_errsup *p) { return p ? p->err.c_str() : ""; }

// the reference, rule Y's mask and rule B's intervals, in gce_errprof's order and with its rules (ep_set_ref, ep_set_mask, ep_set_sites)
int gce_errsup_set_ref(gce_errsup *p, int32_t n_ref, const char *const *seq, const int64_t *len) { return ep_set_ref(p, n_ref, seq, len); }
int gce_errsup_set_mask(gce_errsup *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end) { return ep_set_mask(p, n, tid, start, end); }
int gce_errsup_set_sites(gce_errsup *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end) {
    return ep_set_sites(p, "gce_errsup_set_sites", n_intervals, tid, start, end, ES_COUNTERS * 8ull, SupScan::NSKIP + 2);
}

// the next piece of the file, as gce_errprof_window takes it; *errprof_s: the seconds of the scan and k_sup_count, added to
int gce_errsup_window(gce_errsup *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                      int32_t n_ref, int32_t last, double *errprof_s) {
    if (!p) return GCE_ERR_INVALID;
    const calmd::Ref ref = p->ref();
    const reduce::Sites S = p->sites();
    return rd_window(p, SupScan{p->P, p->T, ref, S}, p->P.n_ref, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, errprof_s, [&](const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end) {
        const unsigned nb = (unsigned)std::min<uint64_t>((n_rec + ES_STEP_RECS - 1) / ES_STEP_RECS, ES_GRID);
        p->dispatch(p->direct || (end >> 32), [&](auto D, auto... m) {
            hipLaunchKernelGGL((k_sup_count<decltype(D)::value, decltype(m)...>), dim3(nb), dim3(ES_THREADS), 0, p->s, u, off, n_rec, p->P, p->T, ref, S, (const uint32_t *)p->meta.p,
                               p->counts.as<unsigned long long>(), m...);
        });
        return true;
    });
}

// after the last window: counters[0] records, [1..9] the skip counters of rule E in its order, [10] eligible; counts_out: room for
// 3 x 33 x 33 x 24 uint64
int gce_errsup_finish(gce_errsup *p, int64_t counters[11], uint64_t *counts_out) {
    if (!p || !p->sites_set || !counters || !counts_out) return GCE_ERR_INVALID;
    return ep_finish(p, SupScan::NSKIP, counters, {counts_out}, ES_COUNTERS * 8ull);
}

}  // extern "C"
#endif  // GCE_ERRSUP_HOST_CHECK
