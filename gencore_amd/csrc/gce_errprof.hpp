// gce_errprof.hpp — mismatches by read cycle against the reference, counted on the GPU (gce_bam_error_profile).
//
// Stands in for `fgbio ErrorRateByReadPosition`, Picard's artifact metrics or the mismatches-per-cycle block of `samtools stats` around a
// consensus step.  The file is streamed window by window as gce_bam_pileup streams it (win_inflate_index / win_carry, gce_passes.hpp); the
// reference bases are resident in calmd's layout (calmd::Ref, gce_calmd.hpp); an optional BED restricts the events to the union of its
// regions (reduce::Sites, reduce::seek, gce_reduce.hpp).  The reduction is the opposite corner from pileup's: 3 segments x 1024 cycles x 24
// classes of 64-bit totals (576 KiB) stay on the device, and every base of every read lands on the few thousand of them its cycle can reach.
// Per window:
//   the scan       (k_reduce_scan over ErrScan, gce_reduce.hpp) one thread per record: eligibility (rule E), the first interval the record can
//                  touch; the skip counters by ballot and one atomic per wave, the lowest malformed record (atomicMin), 4 bytes of meta per
//                  record (the first interval, 0 without a BED, or EP_NONE for a record that is skipped or can touch no interval: the count
//                  kernel drops it on one load)
//   k_err_count    16 lanes per record, 32 records per step of a block of 512 threads, a fixed grid whose blocks stride over the window's
//                  records.  Adds of the first EP_CYC cycles meet in LDS: two planes of 32-bit counters per block, a record slot's parity
//                  choosing the plane, so that the two records of a 32-lane LDS lane group, which walk the same cycles at the same time,
//                  never add to one address in one instruction.  Later cycles are 64-bit global atomics.  At the end the sum of the two
//                  planes goes to memory, one 64-bit global atomic per non-zero counter.  k_err_count<true> (GCE_ERRPROF_DIRECT) has no
//                  planes: every add is a 64-bit global atomic.
// With a variant mask (gce_errprof_set_mask; gce_varmask.hpp) an event whose anchor has its bit set goes to class 21, MASKED
// (rule Y): k_err_count<DIRECT, errprof::Mask>, the same walk with one bit test per event.
// errprof::scan_record and errprof::count_record are __host__ __device__: tests/errprof_host_check.hip runs them on the host against
// tests/pyerrprof.py, the model of the rules.  What the pass shares with gce_bam_pileup -- rule E, the interval table, the scan kernel and the
// device object -- is gce_reduce.hpp's.  What it shares with gce_fragerr.hpp (4l), gce_errsup.hpp (4n) and gce_errqual.hpp (4o) is here, once: the CIGAR walk
// (errprof::walk_record, which calls a functor at every column of an M / = / X op; count_record is the walk under rule W's functor), the
// classes of a reference base, a read base and a counted base, the device object's base (ErrSession, with the one choice of a count kernel's
// instantiation), the add of the planes (ErrAdd) and ep_set_ref / ep_set_sites / ep_finish; ep_set_mask is gce_varmask.hpp's.
#pragma once
#include <cstdint>
#include "gce_reduce.hpp"

namespace errprof {

#define EP_HD __host__ __device__ inline

#define EP_NONE RD_NONE
#define EP_MAX_CYCLE 1024u
#define EP_ROW 24u                                                                    // counters per (segment, cycle): 21 classes, MASKED, 2 zeros
#define EP_COUNTERS (3u * EP_MAX_CYCLE * EP_ROW)
enum { EP_READ_N = 16, EP_REF_OTHER, EP_LOWQ, EP_INS, EP_DEL, EP_NCLASS };
#define EP_MASKED 21u                                                                 // rule Y's class, counted with a variant mask alone (gce_varmask.hpp); 22, 23: zero
enum { EP_SKIP_NO_REF = reduce::N_SKIP + 1, EP_SKIP_TOO_LONG, EP_N_SKIP = EP_SKIP_TOO_LONG };            // behind rule E's six (gce_reduce.hpp)

// bed: rule B is on (S holds the intervals); off, S is not read
struct Params { int32_t n_ref, min_mapq, min_baseq; uint32_t exclude, bed; };
// rule Y's bitmap (gce_varmask.hpp): one bit per byte of ref.blob, bit i of byte i / 8, so the bit of (tid, x) is ref.tab[2 tid] + x
struct Mask { const uint8_t *bits; };
// what the scan learns about a record.  bad: reduce::rule_e's BAD; skip: 0, or the one counter of rule E the record goes to; first: the first interval it can touch (0 without a BED; EP_NONE: none, or not eligible)
struct Rec { uint32_t first; uint8_t bad, skip; };

// One record (r at its block_size, `avail` bytes from r to the end of the buffer): rule E, the first interval.  No byte is read outside
// r[0, min(avail, 4 + block_size)).
EP_HD void scan_record(const uint8_t *r, uint64_t avail, const Params &P, const calmd::Ref &ref, const reduce::Sites &S, Rec &R) {
    R.first = EP_NONE; R.bad = 0; R.skip = 0;
    reduce::Core c;
    const int e = reduce::rule_e(r, avail, P.n_ref, P.min_mapq, P.exclude, c);
    if (e != reduce::ELIGIBLE) { if (e == reduce::BAD) R.bad = 1; else R.skip = (uint8_t)e; return; }
    if (ref.tab[2 * c.tid + 1] < 0) { R.skip = EP_SKIP_NO_REF; return; }
    if ((uint32_t)c.l_seq > EP_MAX_CYCLE) { R.skip = EP_SKIP_TOO_LONG; return; }
    if (!P.bed) { R.first = 0; return; }
    // ---- rule B's anchors lie in [pos - 1, pos + rlen] (pos - 1: an insertion behind a zero-length M; pos + rlen: a leading insertion of a
    //      record without reference bases): the first interval that ends behind pos - 1, if it starts at or in front of pos + rlen
    R.first = reduce::first_interval(S, c.tid, c.pos, (int64_t)c.pos + c.rlen + 1);
}

// rule B for one anchor a, which is x or x - 1, with cur = reduce::seek(S, ., tend, x): the intervals in front of cur end at or in front of
// x - 1 and hold neither; cur itself may end at x
EP_HD bool in_sites(const reduce::Sites &S, uint32_t cur, uint32_t tend, int64_t a) {
    if (cur < tend && (int64_t)S.iv[cur].end <= a) cur++;
    return cur < tend && (int64_t)S.iv[cur].start <= a;
}

// rule Y for the anchor a of an event on a contig whose bases start at byte `base` of the blob and whose FASTA has rlen of them: an anchor
// outside [0, rlen) is not masked (there is no bit where there is no reference base)
EP_HD bool mask_at(const Mask &M, int64_t base, int64_t rlen, int64_t a) {
    if (a < 0 || a >= rlen) return false;
    const uint64_t i = (uint64_t)(base + a);
    return (M.bits[i >> 3] >> (i & 7u)) & 1u;
}

using reduce::Head; using reduce::read_class;                                         // the record header and the class of a read base, gce_reduce.hpp's
// the class of a reference base (rb: the contig's bases, rlen of them): 0..3 = A C G T, 4 = anything else, as reduce::read_class has a read's
EP_HD uint32_t ref_class(const uint8_t *rb, int64_t rlen, int64_t col) {
    if (col >= rlen) return 4u;
    const uint8_t b = rb[col] & 0xDFu;
    return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
}
// the class of a reference base rc against a read's base bc in sequencing orientation: 4 r + b for two usable bases, cls < 18
EP_HD uint32_t base_class(uint32_t rc, uint32_t bc, bool rev) {
    return rc > 3 ? (uint32_t)EP_REF_OTHER : bc > 3 ? (uint32_t)EP_READ_N : rev ? 4u * (3u - rc) + (3u - bc) : 4u * rc + bc;
}
// One column of an M / = / X op as the walk hands it to its functor: the reference position x, the query index yi, the counter row (segment *
// 1024 + cycle - 1) and rule Y's bit (false without a mask).  Nothing of the read or the reference is loaded until a functor asks: q() the
// base's quality (0 for a record without qualities), rc() and bc() the classes of the reference base and the read's.
// EP_PRIMARY(c, P, at_q, rc, bc): the class in the primary table of column c's base when it counts at quality at_q.  MASKED stands in front
// of LOWQ (the position's property, not the read's) and both in front of the bases; a macro, so that rc and bc may be the calls c.rc() and
// c.bc(), evaluated for a base that is neither
struct Column {
    const uint8_t *rb, *sq, *ql; int64_t rlen, x; uint32_t yi, row; bool has_q, rev, masked;
    EP_HD uint32_t q() const { return has_q ? ql[yi] : 0u; }
    EP_HD uint32_t rc() const { return ref_class(rb, rlen, x); }
    EP_HD uint32_t bc() const { return read_class(sq, yi); }
    EP_HD bool lowq(const Params &P, uint32_t at_q) const { return has_q && (int32_t)at_q < P.min_baseq; }
};
#define EP_PRIMARY(c, P, at_q, rc, bc) ((c).masked ? EP_MASKED : (c).lowq(P, at_q) ? (uint32_t)EP_LOWQ : base_class(rc, bc, (c).rev))

// The one CIGAR walk of the error profile, for an eligible record whose scan gave `first`, by lane `lane` of the record's `nlanes`: the lanes
// stride over the columns of each M / = / X op and over the bases of each I op, lane 0 takes the deletions.  at(P, column) is what happens at
// one column of an M / = / X op: rule W's ColumnW below, rules X and V' in gce_fragerr.hpp's MateColumn.  at.add(row, cls): counter
// row * 24 + cls += 1 for an insertion or a deletion, row < 3072.  Reads stay inside the record (the scan checked its fields against
// block_size, the CIGAR's query length against l_seq and l_seq against 1024) and inside the contig's [0, length).  MASK: rule Y is on and M
// holds the bitmap (cls is then < 22); off, M is not read and the code is the walk without a mask.
template <bool MASK, class AT> EP_HD void walk_record(const uint8_t *r, const Params &P, const calmd::Ref &ref, const reduce::Sites &S, uint32_t first, uint32_t lane, uint32_t nlanes, AT &at,
                                                      const Mask &M) {
    const Head h(r);
    const bool has_q = h.has_q(), rev = (h.flag & 16u) != 0;
    const uint32_t seg = (h.flag & 0xC0u) == 0x40u ? 1u : (h.flag & 0xC0u) == 0x80u ? 2u : 0u, row0 = seg * EP_MAX_CYCLE;
    const uint32_t tend = P.bed ? S.tfirst[h.tid + 1] : 0u;
    const int64_t rbase = ref.tab[2 * h.tid];
    const uint8_t *rb = ref.blob + rbase; const int64_t rlen = ref.tab[2 * h.tid + 1];
    uint32_t cur = first, q = 0; int64_t x = h.pos; bool seen = false;
#define EP_CYC0(y) (rev ? (uint32_t)h.lseq - 1u - (y) : (y))                           // rule C, less one
    for (uint32_t k = 0; k < h.nc; k++) {
        const uint32_t w = *(const reduce::rd_u32u *)(h.cg + 4 * k), op = w & 15u, len = w >> 4;
        if (op == 0 || op == 7 || op == 8) {
            const int64_t xe = x + len;
            if (P.bed) cur = reduce::seek(S, cur, tend, x);
            for (uint32_t j = cur;; j++) {                                            // the op's columns, or with a BED their part in every interval
                int64_t a = x, z = xe;
                if (P.bed) {
                    if (j >= tend || (int64_t)S.iv[j].start >= xe) break;
                    const reduce::Ivl v = S.iv[j];
                    a = x > v.start ? x : (int64_t)v.start; z = xe < v.end ? xe : (int64_t)v.end;
                }
                for (int64_t col = a + lane; col < z; col += nlanes) {
                    const uint32_t yi = q + (uint32_t)(col - x);
                    at(P, Column{rb, h.sq, h.ql, rlen, col, yi, row0 + EP_CYC0(yi), has_q, rev, MASK && mask_at(M, rbase, rlen, col)});
                }
                if (!P.bed) break;
            }
            x = xe; q += len; seen = true;
        } else if (op == 2) {
            if (P.bed) cur = reduce::seek(S, cur, tend, x);
            if (lane == 0 && (!P.bed || in_sites(S, cur, tend, x))) at.add(row0 + EP_CYC0(q ? q - 1u : 0u), MASK && mask_at(M, rbase, rlen, x) ? EP_MASKED : (uint32_t)EP_DEL);
            x += len; seen = true;
        } else if (op == 3) x += len;
        else if (op == 1) {
            if (P.bed) cur = reduce::seek(S, cur, tend, x);
            if (!P.bed || in_sites(S, cur, tend, seen ? x - 1 : x)) {
                const uint32_t cls = MASK && mask_at(M, rbase, rlen, seen ? x - 1 : x) ? EP_MASKED : (uint32_t)EP_INS;
                for (uint32_t j = lane; j < len; j += nlanes) at.add(row0 + EP_CYC0(q + j), cls);
            }
            q += len;
        } else if (op == 4) q += len;
    }
#undef EP_CYC0
}
// rule W at one column: the base's class, cls < 21 (< 22 with a mask)
template <class ADD> struct ColumnW {
    ADD &add;
    EP_HD void operator()(const Params &P, const Column &c) { add(c.row, EP_PRIMARY(c, P, c.q(), c.rc(), c.bc())); }
};
// rule W alone, and rules W and Y under the bitmap M
template <class ADD> EP_HD void count_record(const uint8_t *r, const Params &P, const calmd::Ref &ref, const reduce::Sites &S, uint32_t first, uint32_t lane, uint32_t nlanes, ADD &add) {
    ColumnW<ADD> at{add};
    walk_record<false>(r, P, ref, S, first, lane, nlanes, at, Mask{nullptr});
}
template <class ADD> EP_HD void count_record(const uint8_t *r, const Params &P, const calmd::Ref &ref, const reduce::Sites &S, uint32_t first, uint32_t lane, uint32_t nlanes, ADD &add,
                                             const Mask &M) {
    ColumnW<ADD> at{add};
    walk_record<true>(r, P, ref, S, first, lane, nlanes, at, M);
}

#undef EP_HD

}  // namespace errprof

// The planes of k_err_count.  A plane holds the first EP_CYC cycles of the 3 segments, EP_CLS counters of 4 bytes per cycle: 21 is the
// number of classes and odd, so the 16 lanes of a record, on 16 consecutive cycles, fall on 16 different banks.  EP_CYC 160 takes every base
// of a 150-cycle run, the common long one; longer reads pay a global atomic per base past it.  A block has EP_PLANES 2 of them, 80 640 bytes:
// a CU of the MI355X has 160 KiB of LDS and holds 32 waves, so 2 blocks of 8 waves fit, 16 waves per CU, half its wave slots.  That is the
// price of the planes; four planes of 160 cycles do not fit one CU, and one plane leaves the two records of a lane group on one address
// (measured afterwards on the cfg3 file: a build with one plane is as fast within the spread).
// The 32-bit counters cannot wrap within one launch: every add reads a byte of the window no other add reads (a quality byte for a base of
// M = X I, the low byte of the CIGAR word for a D), so a launch adds fewer than 2^32 times in all while the window is shorter than 2^32
// bytes; gce_errprof_window launches the direct kernel for a longer one.
// MASKED (class 21, rule Y) has no slot in a plane's row: a 22nd slot makes the stride even, so the 16 lanes of a record fall on 8 banks two
// by two, and 23 slots make two planes 88 320 bytes, more than half a CU's LDS.  A masked event is a 64-bit global atomic, as an add past
// EP_CYC is: under a sample's VCF about one base in a thousand, and the kernels without a mask (k_err_count<DIRECT>, no Mask argument) are
// the instantiations they were, so a run without a mask pays nothing.  A mask that covers a large share of the targets (a BED of repeats)
// pays an atomic per masked base; a per-block plane of 3 x EP_CYC MASKED counters is the next step if DESIGN.md 4m's measurement asks for it.
#define EP_CYC 160u
#define EP_CLS 21u
#define EP_PLANES 2u
#define EP_PLANE (3u * EP_CYC * EP_CLS)
#define EP_THREADS 512u
#define EP_STEP_RECS 32u
#define EP_GRID 512u
#define EP_LDS_PER_CU (160u << 10)
#define EP_BLOCKS_PER_CU 2u
static_assert(EP_PLANES * EP_PLANE * 4u <= EP_LDS_PER_CU / EP_BLOCKS_PER_CU, "k_err_count's planes must leave the CU its 2 blocks of 8 waves");
static_assert(EP_CLS == (unsigned)errprof::EP_NCLASS && (EP_CLS & 1u) && EP_CYC <= EP_MAX_CYCLE && EP_STEP_RECS * 16u == EP_THREADS, "k_err_count's layout");

#ifndef GCE_ERRPROF_HOST_CHECK

// The device object of an error-profile pass: what gce_errprof, gce_fragerr (gce_fragerr.hpp), gce_errsup (gce_errsup.hpp) and gce_errqual
// (gce_errqual.hpp) hold alike.
// needs() stays the pass's own.
struct ErrSession : ReduceSession {
    errprof::Params P{0, 0, 0, 0, 0}; bool direct = false;
    DevBuf blob, tab; uint64_t ref_bytes = 0; bool ref_set = false;                   // calmd::Ref
    DevBuf counts;                                                                    // the pass's 64-bit totals
    DevBuf mask; uint64_t mask_bytes = 0;                                             // rule Y's bitmap (gce_varmask.hpp); 0 bytes: no mask
    calmd::Ref ref() const { return calmd::Ref{blob.as<uint8_t>(), tab.as<int64_t>(), P.n_ref}; }
    // The instantiation of a count kernel k<DIRECT, MASK...> for (direct_now, a mask or none): launch(std::bool_constant<DIRECT>, the
    // errprof::Mask or nothing) names the kernel as k<decltype(D)::value, decltype(m)...> and hands it m... behind its other arguments
    template <class LAUNCH> void dispatch(bool direct_now, LAUNCH &&launch) const {
        const errprof::Mask M{mask.as<uint8_t>()};
        if (mask_bytes) { if (direct_now) launch(std::true_type{}, M); else launch(std::false_type{}, M); }
        else if (direct_now) launch(std::true_type{});
        else launch(std::false_type{});
    }
};
#include "gce_varmask.hpp"

namespace {

// the scan of k_reduce_scan.  misc: [0] the lowest malformed record, [1..8] the skip counters of rule E in its order, [9] eligible records
struct ErrScan {
    typedef errprof::Rec Rec;
    static constexpr int NSKIP = errprof::EP_N_SKIP; static constexpr bool OPS = false;
    errprof::Params P; calmd::Ref ref; reduce::Sites S;
    __device__ void operator()(const uint8_t *r, uint64_t avail, Rec &R) const { errprof::scan_record(r, avail, P, ref, S, R); }
};

// an add of k_err_count and k_fragerr_count: into the plane when the cycle lies in it, else to memory.  MASK: MASKED goes to memory, whatever
// its cycle
template <bool DIRECT, bool MASK> struct ErrAdd {
    uint32_t *plane; unsigned long long *counts;
    __device__ __forceinline__ void operator()(uint32_t row, uint32_t cls) {
        const uint32_t c0 = row & (EP_MAX_CYCLE - 1u);
        if (!DIRECT && c0 < EP_CYC && (!MASK || cls != EP_MASKED)) atomicAdd(plane + ((row >> 10) * EP_CYC + c0) * EP_CLS + cls, 1u);
        else atomicAdd(counts + row * EP_ROW + cls, 1ull);
    }
};
// 16 lanes per record, 32 records per step; block b takes the records [32 (b + k gridDim.x), + 32) of the window, k = 0, 1, ...
// MASK: none, or one errprof::Mask for rule Y
template <bool DIRECT, class... MASK> __global__ __launch_bounds__(EP_THREADS) void k_err_count(const uint8_t *u, const uint64_t *off, uint64_t n, errprof::Params P, calmd::Ref ref, reduce::Sites S,
                                                                                                const uint32_t *meta, unsigned long long *counts, MASK... mask) {
    __shared__ uint32_t s_tab[DIRECT ? 1 : EP_PLANES * EP_PLANE];
    const uint32_t slot = threadIdx.x >> 4, sub = threadIdx.x & 15u;
    if (!DIRECT) {
        for (uint32_t i = threadIdx.x; i < EP_PLANES * EP_PLANE; i += EP_THREADS) s_tab[i] = 0u;
        __syncthreads();
    }
    ErrAdd<DIRECT, sizeof...(MASK) != 0> add{s_tab + (DIRECT ? 0u : (slot & (EP_PLANES - 1u)) * EP_PLANE), counts};
    for (uint64_t j = (uint64_t)blockIdx.x * EP_STEP_RECS + slot; j < n; j += (uint64_t)gridDim.x * EP_STEP_RECS) {
        const uint32_t first = meta[j];
        if (first != EP_NONE) errprof::count_record(u + off[j], P, ref, S, first, sub, 16u, add, mask...);
    }
    if (!DIRECT) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < EP_PLANE; i += EP_THREADS) {
            const uint32_t v = s_tab[i] + s_tab[EP_PLANE + i];
            if (v) {
                const uint32_t prow = i / EP_CLS, cls = i - prow * EP_CLS, seg = prow / EP_CYC, c0 = prow - seg * EP_CYC;
                atomicAdd(counts + (seg * EP_MAX_CYCLE + c0) * EP_ROW + cls, (unsigned long long)v);
            }
        }
    }
}

}  // namespace

struct gce_errprof : ErrSession {
    std::string needs() const override {
        return "gce_bam_error_profile needs the reference bases (" + std::to_string(ref_bytes) + " bytes) + 576 KiB of counters" + varmask_needs(mask_bytes);
    }
};

// The reference and rule B's intervals of an error-profile pass: gce_errprof_set_ref / gce_errprof_set_sites, gce_fragerr.hpp's and
// gce_errsup.hpp's.  counts_bytes: the pass's counters; misc_words: the scan's counters to start from zero, its NSKIP + 2
static int ep_set_ref(ErrSession *p, int32_t n_ref, const char *const *seq, const int64_t *len) {
    if (!p || p->ref_set || n_ref < 0 || (n_ref && (!seq || !len))) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    std::vector<int64_t> tab;
    const uint64_t total = calmd_ref_layout(n_ref, seq, len, tab);
    p->ref_bytes = total; p->P.n_ref = n_ref;
    const uint64_t want = DevBuf::padded(total + 64) + DevBuf::padded(tab.size() * 8);
    if (!p->room(want)) return p->oom("the reference bases", want);
    RDCHK(calmd_ref_upload(p->blob, p->tab, n_ref, seq, len, tab, total, p->s));
    p->ref_set = true;
    return GCE_OK;
}
static int ep_set_sites(ErrSession *p, const char *entry, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, uint64_t counts_bytes, int misc_words = 10) {
    if (!p || !p->ref_set || p->sites_set || (n_intervals > 0 && (!tid || !start || !end))) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    p->P.bed = n_intervals >= 0;
    RdTable t;
    const int rc = rd_intervals(p, entry, p->P.n_ref, std::max<int64_t>(n_intervals, 0), tid, start, end, t);
    if (rc != GCE_OK) return rc;
    return rd_set_sites(p, t, p->counts, counts_bytes, misc_words);
}
// After the last window, behind rd_finish: counters[0] records, [1..nskip] the skip counters in the pass's order, [nskip + 1] eligible; then
// the pass's tables, `bytes` each, one behind the other in p->counts
static int ep_finish(ErrSession *p, int nskip, int64_t *counters, std::initializer_list<uint64_t *> tables, uint64_t bytes) {
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    unsigned long long h[RD_MISC_WORDS];
    const int rc = rd_finish(p, nskip, counters, h, nskip + 2);
    if (rc != GCE_OK) return rc;
    const uint8_t *src = p->counts.as<uint8_t>();
    for (uint64_t *t : tables) { RDCHK(hipMemcpyAsync(t, src, bytes, hipMemcpyDeviceToHost, s)); src += bytes; }
    RDCHK(hipStreamSynchronize(s));
    RDCHK(hipGetLastError());
    return GCE_OK;
}

extern "C" {

int gce_errprof_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_errprof **out) {
    return rd_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options, (uint32_t)GCE_ERRPROF_DIRECT, out);
}
void gce_errprof_destroy(gce_errprof *p) { if (p) rd_destroy(p, {&p->blob, &p->tab, &p->counts, &p->mask}); }
const char *gce_errprof_error(gce_errprof *p) { return p ? p->err.c_str() : ""; }

// the reference, once, first of all: seq[t] / len[t] as gce_sort_calmd_ref takes them, laid out as it lays them out (calmd_ref_layout)
int gce_errprof_set_ref(gce_errprof *p, int32_t n_ref, const char *const *seq, const int64_t *len) { return ep_set_ref(p, n_ref, seq, len); }

// rule B's intervals, once, behind the reference and in front of the first window, as gce_pileup_set_sites takes them; n_intervals < 0: no BED.
// The counters are made and zeroed.
int gce_errprof_set_sites(gce_errprof *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end) {
    return ep_set_sites(p, "gce_errprof_set_sites", n_intervals, tid, start, end, EP_COUNTERS * 8ull);
}

// rule Y's mask, a chunk of it: the bits of [start[j], end[j]) of contig tid[j], clamped to the contig's FASTA length, are set.  Any number
// of times, behind the reference and in front of the first window; chunks may repeat or overlap.  Class 21 is MASKED from the first call on.
int gce_errprof_set_mask(gce_errprof *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end) { return ep_set_mask(p, n, tid, start, end); }

// the next piece of the file, as gce_pileup_window takes it; *errprof_s: the seconds of the scan and k_err_count, added to.  GCE_ERR_INVALID
// names the lowest malformed record, counting from 0 over the file.
int gce_errprof_window(gce_errprof *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                       int32_t n_ref, int32_t last, double *errprof_s) {
    if (!p) return GCE_ERR_INVALID;
    const calmd::Ref ref = p->ref();
    const reduce::Sites S = p->sites();
    return rd_window(p, ErrScan{p->P, ref, S}, p->P.n_ref, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, errprof_s, [&](const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end) {
        const unsigned nb = (unsigned)std::min<uint64_t>((n_rec + EP_STEP_RECS - 1) / EP_STEP_RECS, EP_GRID);
        p->dispatch(p->direct || (end >> 32), [&](auto D, auto... m) {
            hipLaunchKernelGGL((k_err_count<decltype(D)::value, decltype(m)...>), dim3(nb), dim3(EP_THREADS), 0, p->s, u, off, n_rec, p->P, ref, S, (const uint32_t *)p->meta.p,
                               p->counts.as<unsigned long long>(), m...);
        });
        return true;
    });
}

// after the last window: counters[0] records, [1..8] the skip counters of rule E in its order, [9] eligible; counts_out: room for
// 3 x 1024 x 24 uint64
int gce_errprof_finish(gce_errprof *p, int64_t counters[10], uint64_t *counts_out) {
    if (!p || !p->sites_set || !counters || !counts_out) return GCE_ERR_INVALID;
    return ep_finish(p, ErrScan::NSKIP, counters, {counts_out}, EP_COUNTERS * 8ull);
}

}  // extern "C"
#endif  // GCE_ERRPROF_HOST_CHECK
