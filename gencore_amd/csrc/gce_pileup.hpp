// gce_pileup.hpp — bases per strand at BED targets, counted on the GPU (gce_bam_pileup).
//
// Stands in for the `samtools mpileup` / `bam-readcount` a panel's user runs on the input and on the consensus output to see which mismatches
// consensus removed.  The file is streamed window by window as the BAI indexer streams it (win_inflate_index / win_carry, gce_passes.hpp); a
// reduce pass instead of a rewriter: nothing of a window outlives it but what it added to the counters, 16 uint32 per site (2 strands x
// A C G T N DEL INS LOWQ), which stay on the device across windows.  The sites are the union of the BED's regions as merged intervals
// (tid, start, end, site index of start) with a per-tid first-interval table.  Per window:
//   the scan       (k_reduce_scan over PileScan, gce_reduce.hpp) one thread per record: eligibility (rule E), the reference span, the first
//                  interval the record can touch (binary search); the skip counters by ballot and one atomic per wave, the lowest malformed
//                  record (atomicMin), 4 bytes of meta per record (the first interval, or PU_NONE for a record that is skipped or overlaps no
//                  interval: the count kernel drops it on one load)
//   k_pile_count   16 lanes per record, 16 records per block: the lanes stride over the columns of each M / = / X / D op (rule W).  Adds meet
//                  in an LDS tile of PU_TILE sites' counters that starts at the first site the block's first overlapping record can touch;
//                  an add outside the tile is a global atomic; at the end the tile's non-zero counters go to memory, one global atomic each.
//                  Sortedness decides only how many adds the tile catches.  k_pile_count<true> (GCE_PILEUP_DIRECT) has no tile: every add is a
//                  global atomic.
// pileup::scan_record and pileup::count_record are __host__ __device__: tests/pileup_host_check.hip runs them on the host against
// tests/pypileup.py, the model of the rules.  What the pass shares with gce_bam_error_profile -- rule E, the interval table, the scan kernel,
// the device object, the decode of a record's header (reduce::Head) and the class of a 4-bit base (reduce::read_class) -- is
// gce_reduce.hpp's.  What it shares with gce_fragpile.hpp (4k) is here, once: the CIGAR walk (pileup::walk_record, which asks a functor at
// every column of an M / = / X / D op; count_record is the walk under rule W's functor), the LDS tile and its adds (PileAdd), the device
// object's base (PileSession, with the one choice of a count kernel's instantiation) and pu_set_sites / pu_finish.
#pragma once
#include <cstdint>
#include "gce_reduce.hpp"

namespace pileup {

#define PU_HD __host__ __device__ inline

#define PU_NONE RD_NONE
#define PU_MAX_SITES (1u << 28)
enum { PU_A = 0, PU_C, PU_G, PU_T, PU_N, PU_DEL, PU_INS, PU_LOWQ };
static_assert(PU_A == 0 && PU_C == 1 && PU_G == 2 && PU_T == 3 && PU_N == 4, "the classes of a base are reduce::read_class's 0..4");

using reduce::Ivl; using reduce::Sites; using reduce::seek;                           // rule S on the device
struct Params { int32_t n_ref, min_mapq, min_baseq; uint32_t exclude; };
// what the scan learns about a record.  bad: reduce::rule_e's BAD; skip: 0, or the one counter of rule E the record goes to; first: the first
// interval it can touch (PU_NONE: none, or not eligible); nc: n_cigar_op of an eligible record
struct Rec { uint32_t first, nc; uint8_t bad, skip; };

// One record (r at its block_size, `avail` bytes from r to the end of the buffer): rule E, the span, the first overlapping interval.  No byte
// is read outside r[0, min(avail, 4 + block_size)).
PU_HD void scan_record(const uint8_t *r, uint64_t avail, const Params &P, const Sites &S, Rec &R) {
    R.first = PU_NONE; R.nc = 0; R.bad = 0; R.skip = 0;
    reduce::Core c;
    const int e = reduce::rule_e(r, avail, P.n_ref, P.min_mapq, P.exclude, c);
    if (e != reduce::ELIGIBLE) { if (e == reduce::BAD) R.bad = 1; else R.skip = (uint8_t)e; return; }
    R.nc = c.n_cigar_op;
    // ---- the record touches sites of [pos - 1, pos + rlen) at most (pos - 1: an insertion behind a zero-length M): the first interval that ends
    //      behind pos - 1, if it starts in front of pos + rlen
    R.first = reduce::first_interval(S, c.tid, c.pos, (int64_t)c.pos + c.rlen);
}

// One column of an M / = / X / D op as walk_record hands it to its functor: the reference position x, the query index yi (of the op's first
// base at a D column, and not to be used), whether a D op covers it.  Nothing of the read is loaded until a functor asks: load(cls, q) gives
// the raw class (A C G T N, DEL at a D column) and the base's quality (0 at a D column or for a record without qualities), under one test of
// `del`, so that a column costs one branch; lowq(P, at_q): the column counts as LOWQ at quality at_q
struct Column {
    const uint8_t *sq, *ql; int64_t x; uint32_t yi; bool has_q, del;
    PU_HD void load(uint32_t &cls, uint32_t &q) const {
        cls = PU_DEL; q = 0;
        if (!del) { cls = reduce::read_class(sq, yi); if (has_q) q = ql[yi]; }
    }
    PU_HD bool lowq(const Params &P, uint32_t at_q) const { return !del && has_q && (int32_t)at_q < P.min_baseq; }
};

// The one CIGAR walk of the pileup pair, for an eligible record whose scan gave `first`, by lane `lane` of the record's `nlanes`: the lanes
// stride over the columns of each M / = / X / D op, clipped to every interval the op meets, lane 0 takes the insertions.  at(P, column, cls)
// is what happens at one column: the class the record adds there, or false, not mine -- rule W's ColumnW below, rule V's fragpile::ColumnV
// (gce_fragpile.hpp).  add(i): counter i (site * 16 + strand * 8 + class) += 1.  Reads stay inside the record (the scan checked its fields
// against block_size and the CIGAR's query length against l_seq); i < 16 * the number of sites.
template <class AT, class ADD> PU_HD void walk_record(const uint8_t *r, const Params &P, const Sites &S, uint32_t first, uint32_t lane, uint32_t nlanes, AT &at, ADD &add) {
    const reduce::Head h(r);
    const uint32_t sbase = ((h.flag >> 4) & 1u) * 8u, tend = S.tfirst[h.tid + 1];
    const bool has_q = h.has_q();
    uint32_t cur = first, q = 0; int64_t x = h.pos; bool seen = false;
    for (uint32_t k = 0; k < h.nc; k++) {
        const uint32_t w = *(const reduce::rd_u32u *)(h.cg + 4 * k), op = w & 15u, len = w >> 4;
        if (op == 0 || op == 7 || op == 8 || op == 2) {
            cur = seek(S, cur, tend, x);
            const int64_t xe = x + len;
            for (uint32_t j = cur; j < tend && (int64_t)S.iv[j].start < xe; j++) {
                const Ivl v = S.iv[j];
                const int64_t a = x > v.start ? x : (int64_t)v.start, z = xe < v.end ? xe : (int64_t)v.end;
                for (int64_t col = a + lane; col < z; col += nlanes) {
                    uint32_t cls;
                    if (at(P, Column{h.sq, h.ql, col, q + (uint32_t)(col - x), has_q, op == 2}, cls)) add((v.site0 + (uint32_t)(col - v.start)) * 16u + sbase + cls);
                }
            }
            x = xe; if (op != 2) q += len;
            seen = true;
        } else if (op == 3) x += len;
        else if (op == 1) {
            if (seen && x >= 1) {
                cur = seek(S, cur, tend, x);
                if (cur < tend && (int64_t)S.iv[cur].start <= x - 1 && lane == 0) add((S.iv[cur].site0 + (uint32_t)(x - 1 - S.iv[cur].start)) * 16u + sbase + PU_INS);
            }
            q += len;
        } else if (op == 4) q += len;
    }
}
// rule W at one column: the raw class, LOWQ for a base under min_baseq
struct ColumnW {
    PU_HD bool operator()(const Params &P, const Column &c, uint32_t &cls) const {
        uint32_t q;
        c.load(cls, q);
        if (c.lowq(P, q)) cls = PU_LOWQ;
        return true;
    }
};
// rule W for a record alone
template <class ADD> PU_HD void count_record(const uint8_t *r, const Params &P, const Sites &S, uint32_t first, uint32_t lane, uint32_t nlanes, ADD &add) {
    ColumnW at;
    walk_record(r, P, S, first, lane, nlanes, at, add);
}

#undef PU_HD

}  // namespace pileup

#ifndef GCE_PILEUP_HOST_CHECK

namespace {

// The LDS tile of k_pile_count and k_frag_count (PileAdd below): PU_TILE sites x 16 counters x 4 bytes.  A CU of the MI355X has 160 KiB of LDS and holds 32 waves; a block of
// 256 threads is 4 waves, so 8 blocks fill a CU and each may hold 160 KiB / 8 = 20 KiB.  256 sites are 16 KiB (+ 64 bytes of tile starts): a
// block's 16 reads of a sorted panel span a read length and a little.
#define PU_TILE 256u
#define PU_LDS_PER_CU (160u << 10)
#define PU_BLOCKS_PER_CU 8u
static_assert(PU_TILE * 64u + 64u <= PU_LDS_PER_CU / PU_BLOCKS_PER_CU, "k_pile_count's tile must leave the CU its 8 blocks of 4 waves");

// the scan of k_reduce_scan.  misc: [0] the lowest malformed record, [1..6] the skip counters of rule E in its order, [7] eligible records,
// [8] their n_cigar_op summed
struct PileScan {
    typedef pileup::Rec Rec;
    static constexpr int NSKIP = reduce::N_SKIP; static constexpr bool OPS = true;
    pileup::Params P; pileup::Sites S;
    __device__ void operator()(const uint8_t *r, uint64_t avail, Rec &R) const { pileup::scan_record(r, avail, P, S, R); }
    __device__ uint32_t ops(const Rec &R) const { return R.nc; }
};

// The adds of k_pile_count and k_frag_count (gce_fragpile.hpp), 16 lanes per record and 16 records per block of 256: into the block's tile
// when the counter lies in it, else to memory.  The tile starts at the first site the block's first overlapping record can touch.  DIRECT: no
// tile, every add is a global atomic
template <bool DIRECT> struct PileAdd {
    uint32_t *tile, *counts; uint32_t base16;
    __device__ __forceinline__ void operator()(uint32_t idx) {
        const uint32_t d = idx - base16;                                              // (a counter in front of the tile wraps beyond it)
        if (!DIRECT && d < PU_TILE * 16u) atomicAdd(tile + d, 1u);
        else atomicAdd(counts + idx, 1u);
    }
    // The tile zeroed and placed, by the whole block.  rec(): the record of this thread's slot (threadIdx.x >> 4) whose scan gave `first`, asked
    // for by the slot's first lane, and not when first is PU_NONE: the record is skipped or touches no site.  false, for the whole block: no
    // record of it touches a site, and no barrier may follow
    template <class REC> __device__ __forceinline__ bool open(uint32_t first, const pileup::Sites &S, uint32_t *counts_, REC &&rec) {
        __shared__ uint32_t s_tile[DIRECT ? 1 : PU_TILE * 16u];
        __shared__ uint32_t s_base[16];
        tile = s_tile; counts = counts_; base16 = 0;
        if (DIRECT) return true;
        for (uint32_t i = threadIdx.x; i < PU_TILE * 16u; i += 256u) s_tile[i] = 0u;
        if ((threadIdx.x & 15u) == 0) {                                               // the first site this record can touch: that of max(pos - 1, the interval's start)
            uint32_t b = PU_NONE;
            if (first != PU_NONE) {
                const int32_t pos = (int32_t)rb32(rec() + 8);
                const pileup::Ivl v = S.iv[first];
                b = v.site0 + (uint32_t)(max(pos - 1, v.start) - v.start);
            }
            s_base[threadIdx.x >> 4] = b;
        }
        __syncthreads();
        uint32_t base = PU_NONE;
#pragma unroll
        for (int k = 15; k >= 0; k--) if (s_base[k] != PU_NONE) base = s_base[k];       // the block's first overlapping record's
        base16 = base * 16u;
        return base != PU_NONE;
    }
    // the tile's non-zero counters to memory, one global atomic each, by the whole block; n_counts: 16 x the number of sites
    __device__ __forceinline__ void flush(uint64_t n_counts) {
        if (DIRECT) return;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < PU_TILE * 16u; i += 256u) {
            const uint32_t v = tile[i];
            const uint64_t at = (uint64_t)base16 + i;
            if (v && at < n_counts) atomicAdd(counts + at, v);
        }
    }
};
// block b: records [16 b, 16 b + 16) of the window
template <bool DIRECT> __global__ __launch_bounds__(256) void k_pile_count(const uint8_t *u, const uint64_t *off, uint64_t n, pileup::Params P, pileup::Sites S, const uint32_t *meta,
                                                                           uint32_t *counts, uint64_t n_counts) {
    const uint64_t j = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 4);
    const uint32_t first = j < n ? meta[j] : PU_NONE;
    PileAdd<DIRECT> add;
    if (!add.open(first, S, counts, [&] { return u + off[j]; })) return;
    if (first != PU_NONE) pileup::count_record(u + off[j], P, S, first, threadIdx.x & 15u, 16u, add);
    add.flush(n_counts);
}

}  // namespace

// The device object of a pileup pass: what gce_pileup and gce_fragpile (gce_fragpile.hpp) hold alike.  needs() stays the pass's own.
struct PileSession : ReduceSession {
    pileup::Params P{0, 0, 0, 0}; bool direct = false;
    DevBuf counts; uint64_t n_sites = 0;                                              // 64 bytes per site
    // The instantiation of a count kernel k<DIRECT>: launch(std::bool_constant<DIRECT>) names the kernel as k<decltype(D)::value>
    template <class LAUNCH> void dispatch(LAUNCH &&launch) const { if (direct) launch(std::true_type{}); else launch(std::false_type{}); }
};
struct gce_pileup : PileSession {
    std::string needs() const override { return "gce_bam_pileup needs 64 bytes per site (" + std::to_string(n_sites) + " sites: " + std::to_string(n_sites * 64) + " bytes)"; }
};

// gce_pileup_set_sites and gce_fragpile_set_sites: rule S's intervals, once, in front of the first window: interval j = [start[j], end[j]) of
// contig tid[j], in (tid, start) order, disjoint and not abutting, inside the contig; site0[j]: the site index of start[j] (the sum of the
// lengths in front of it).  The counters are made and zeroed.  entry: the entry point that names itself in the refusal
static int pu_set_sites(PileSession *p, const char *entry, int32_t n_ref, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, const uint32_t *site0) {
    if (!p || p->sites_set || n_ref < 0 || n_intervals < 0 || (n_intervals && (!tid || !start || !end || !site0))) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    RdTable t;
    const int rc = rd_intervals(p, entry, n_ref, n_intervals, tid, start, end, t);
    if (rc != GCE_OK) return rc;
    for (int64_t j = 0; j < n_intervals; j++) if (site0[j] != t.iv[(size_t)j].site0) return p->out_of_order(entry);
    if (t.sites > PU_MAX_SITES) return p->fail(GCE_ERR_INVALID, "more than 2^28 sites");
    p->n_sites = t.sites; p->P.n_ref = n_ref;
    return rd_set_sites(p, t, p->counts, t.sites * 64 + 64, 9);
}
// gce_pileup_finish and the first part of gce_fragpile_finish, after the last window: counters[0] records, [1..6] the skip counters of rule E
// in its order, [7] eligible; counts_out (NULL, or room for 16 uint32 per site): the counters.  GCE_ERR_INVALID when the eligible records'
// n_cigar_op sum to 2^32 or more.
static int pu_finish(PileSession *p, int64_t *counters, uint32_t *counts_out) {
    if (!p || !p->sites_set || !counters) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    unsigned long long h[9];
    const int rc = rd_finish(p, PileScan::NSKIP, counters, h, 9);
    if (rc != GCE_OK) return rc;
    if (h[8] >> 32) return p->fail(GCE_ERR_INVALID, "the eligible records hold 2^32 CIGAR operations or more: the 32-bit counters cannot be shown to hold");
    if (counts_out && p->n_sites) { RDCHK(hipMemcpyAsync(counts_out, p->counts.p, p->n_sites * 64, hipMemcpyDeviceToHost, s)); RDCHK(hipStreamSynchronize(s)); }
    RDCHK(hipGetLastError());
    return GCE_OK;
}

extern "C" {

int gce_pileup_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_pileup **out) {
    return rd_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options, (uint32_t)GCE_PILEUP_DIRECT, out);
}
void gce_pileup_destroy(gce_pileup *p) { if (p) rd_destroy(p, {&p->counts}); }
const char *gce_pileup_error(gce_pileup *p) { return p ? p->err.c_str() : ""; }

int gce_pileup_set_sites(gce_pileup *p, int32_t n_ref, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, const uint32_t *site0) {
    return pu_set_sites(p, "gce_pileup_set_sites", n_ref, n_intervals, tid, start, end, site0);
}

// the next piece of the file, as gce_bai_window takes it; *pileup_s: the seconds of the scan and k_pile_count, added to.  GCE_ERR_INVALID
// names the lowest malformed record, counting from 0 over the file.
int gce_pileup_window(gce_pileup *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                      int32_t n_ref, int32_t last, double *pileup_s) {
    if (!p) return GCE_ERR_INVALID;
    const pileup::Sites S = p->sites();
    return rd_window(p, PileScan{p->P, S}, p->P.n_ref, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, pileup_s, [&](const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t) {
        if (!p->n_sites) return false;
        p->dispatch([&](auto D) {
            hipLaunchKernelGGL(k_pile_count<decltype(D)::value>, dim3((unsigned)((n_rec + 15) / 16)), dim3(256), 0, p->s, u, off, n_rec, p->P, S, (const uint32_t *)p->meta.p, p->counts.as<uint32_t>(),
                               p->n_sites * 16);
        });
        return true;
    });
}

int gce_pileup_finish(gce_pileup *p, int64_t counters[8], uint32_t *counts_out) { return pu_finish(p, counters, counts_out); }

}  // extern "C"
#endif  // GCE_PILEUP_HOST_CHECK
