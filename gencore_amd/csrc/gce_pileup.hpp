// gce_pileup.hpp — bases per strand at BED targets, counted on the GPU (gce_bam_pileup).
//
// Stands in for the `samtools mpileup` / `bam-readcount` a panel's user runs on the input and on the consensus output to see which mismatches
// consensus removed.  The file is streamed window by window as the BAI indexer streams it (win_inflate_index / win_carry, gce_passes.hpp); a
// reduce pass instead of a rewriter: nothing of a window outlives it but what it added to the counters, 16 uint32 per site (2 strands x
// A C G T N DEL INS LOWQ), which stay on the device across windows.  The sites are the union of the BED's regions as merged intervals
// (tid, start, end, site index of start) with a per-tid first-interval table.  Per window:
//   k_pile_scan    one thread per record: eligibility (rule E), the reference span, the first interval the record can touch (binary search);
//                  the skip counters by ballot and one atomic per wave, the lowest malformed record (atomicMin), 4 bytes of meta per record
//                  (the first interval, or PU_NONE for a record that is skipped or overlaps no interval: the count kernel drops it on one load)
//   k_pile_count   16 lanes per record, 16 records per block: the lanes stride over the columns of each M / = / X / D op (rule W).  Adds meet
//                  in an LDS tile of PU_TILE sites' counters that starts at the first site the block's first overlapping record can touch;
//                  an add outside the tile is a global atomic; at the end the tile's non-zero counters go to memory, one global atomic each.
//                  Sortedness decides only how many adds the tile catches.  k_pile_count<true> (GCE_PILEUP_DIRECT) has no tile: every add is a
//                  global atomic.
// pileup::scan_record and pileup::count_record are __host__ __device__: tests/pileup_host_check.hip runs them on the host against
// tests/pypileup.py, the model of the rules.
#pragma once
#include <cstdint>

namespace pileup {

#define PU_HD __host__ __device__ inline

typedef uint32_t __attribute__((aligned(1), may_alias)) pu_u32u;
typedef uint16_t __attribute__((aligned(1), may_alias)) pu_u16u;

#define PU_NONE 0xFFFFFFFFu
#define PU_MAX_SITES (1u << 28)
enum { PU_A = 0, PU_C, PU_G, PU_T, PU_N, PU_DEL, PU_INS, PU_LOWQ };
enum { PU_SKIP_UNPLACED = 1, PU_SKIP_FLAGGED, PU_SKIP_LOW_MAPQ, PU_SKIP_NO_CIGAR, PU_SKIP_NO_SEQ, PU_SKIP_BAD_CIGAR };

// rule S on the device: interval j = sites [start, end) of contig tid, the site of `start` has index site0; the intervals of contig t are
// [tfirst[t], tfirst[t + 1]), in ascending order, disjoint and not abutting
struct Ivl { int32_t tid, start, end; uint32_t site0; };
struct Sites { const Ivl *iv; const uint32_t *tfirst; };
struct Params { int32_t n_ref, min_mapq, min_baseq; uint32_t exclude; };
// what the scan learns about a record.  bad: block_size < 32 or beyond the buffer, or fields that overrun block_size; skip: 0, or the one
// counter of rule E the record goes to; first: the first interval it can touch (PU_NONE: none, or not eligible); nc: n_cigar_op of an eligible record
struct Rec { uint32_t first, nc; uint8_t bad, skip; };

// One record (r at its block_size, `avail` bytes from r to the end of the buffer): rule E, the span, the first overlapping interval.  No byte
// is read outside r[0, min(avail, 4 + block_size)).
PU_HD void scan_record(const uint8_t *r, uint64_t avail, const Params &P, const Sites &S, Rec &R) {
    R.first = PU_NONE; R.nc = 0; R.bad = 0; R.skip = 0;
    if (avail < 4) { R.bad = 1; return; }
    const uint64_t bs = *(const pu_u32u *)r;
    if (bs < 32 || 4 + bs > avail) { R.bad = 1; return; }
    const uint8_t *c = r + 4;
    const int32_t tid = (int32_t) * (const pu_u32u *)(c + 0), pos = (int32_t) * (const pu_u32u *)(c + 4), lseq = (int32_t) * (const pu_u32u *)(c + 16);
    const uint32_t lq = c[8], mapq = c[9], nc = *(const pu_u16u *)(c + 12), flag = *(const pu_u16u *)(c + 14);
    if (lseq < 0 || 32ull + lq + 4ull * nc + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > bs) { R.bad = 1; return; }
    // ---- rule E, in its order
    if (tid < 0 || tid >= P.n_ref || pos < 0) { R.skip = PU_SKIP_UNPLACED; return; }
    if (flag & P.exclude) { R.skip = PU_SKIP_FLAGGED; return; }
    if ((int32_t)mapq < P.min_mapq) { R.skip = PU_SKIP_LOW_MAPQ; return; }
    if (nc == 0) { R.skip = PU_SKIP_NO_CIGAR; return; }
    if (lseq == 0) { R.skip = PU_SKIP_NO_SEQ; return; }
    const uint8_t *cg = c + 32 + lq;
    uint64_t qn = 0; int64_t rlen = 0;
    for (uint32_t k = 0; k < nc; k++) {
        const uint32_t w = *(const pu_u32u *)(cg + 4 * k), op = w & 15u;
        if (op > 8) { R.skip = PU_SKIP_BAD_CIGAR; return; }
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qn += w >> 4;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += w >> 4;
    }
    if (qn != (uint64_t)lseq) { R.skip = PU_SKIP_BAD_CIGAR; return; }
    R.nc = nc;
    // ---- the record touches sites of [pos - 1, pos + rlen) at most (pos - 1: an insertion behind a zero-length M): the first interval that ends
    //      behind pos - 1, if it starts in front of pos + rlen
    uint32_t lo = S.tfirst[tid]; const uint32_t tend = S.tfirst[tid + 1]; uint32_t hi = tend;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (S.iv[mid].end < pos) lo = mid + 1; else hi = mid; }
    if (lo < tend && (int64_t)S.iv[lo].start < (int64_t)pos + rlen) R.first = lo;
}

// the first interval of [cur, tend) that ends at or behind x (every interval in front of it holds neither x - 1 nor anything behind it)
PU_HD uint32_t seek(const Sites &S, uint32_t cur, uint32_t tend, int64_t x) {
    if (cur >= tend || (int64_t)S.iv[cur].end >= x) return cur;
    uint32_t lo = cur + 1, hi = tend;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((int64_t)S.iv[mid].end < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// Rule W for an eligible record whose scan gave `first`, by lane `lane` of the record's `nlanes`: the lanes stride over the columns of each
// M / = / X / D op, lane 0 takes the insertions.  add(i): counter i (site * 16 + strand * 8 + class) += 1.  Reads stay inside the record (the
// scan checked its fields against block_size and the CIGAR's query length against l_seq); i < 16 * the number of sites.
template <class ADD> PU_HD void count_record(const uint8_t *r, const Params &P, const Sites &S, uint32_t first, uint32_t lane, uint32_t nlanes, ADD &add) {
    const uint8_t *c = r + 4;
    const int32_t tid = (int32_t) * (const pu_u32u *)(c + 0), pos = (int32_t) * (const pu_u32u *)(c + 4), lseq = (int32_t) * (const pu_u32u *)(c + 16);
    const uint32_t lq = c[8], nc = *(const pu_u16u *)(c + 12), flag = *(const pu_u16u *)(c + 14);
    const uint8_t *cg = c + 32 + lq, *sq = cg + 4 * nc, *ql = sq + ((uint32_t)lseq + 1) / 2;
    const uint32_t sbase = ((flag >> 4) & 1u) * 8u, tend = S.tfirst[tid + 1];
    const bool has_q = ql[0] != 0xFF;
    uint32_t cur = first, q = 0; int64_t x = pos; bool seen = false;
    for (uint32_t k = 0; k < nc; k++) {
        const uint32_t w = *(const pu_u32u *)(cg + 4 * k), op = w & 15u, len = w >> 4;
        if (op == 0 || op == 7 || op == 8 || op == 2) {
            cur = seek(S, cur, tend, x);
            const int64_t xe = x + len;
            for (uint32_t j = cur; j < tend && (int64_t)S.iv[j].start < xe; j++) {
                const Ivl v = S.iv[j];
                const int64_t a = x > v.start ? x : (int64_t)v.start, z = xe < v.end ? xe : (int64_t)v.end;
                for (int64_t col = a + lane; col < z; col += nlanes) {
                    uint32_t cls = PU_DEL;
                    if (op != 2) {
                        const uint32_t yi = q + (uint32_t)(col - x), nib = (sq[yi >> 1] >> ((~yi & 1u) << 2)) & 15u;
                        cls = nib == 1 ? PU_A : nib == 2 ? PU_C : nib == 4 ? PU_G : nib == 8 ? PU_T : PU_N;
                        if (has_q && (int32_t)ql[yi] < P.min_baseq) cls = PU_LOWQ;
                    }
                    add((v.site0 + (uint32_t)(col - v.start)) * 16u + sbase + cls);
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

#undef PU_HD

}  // namespace pileup

#ifndef GCE_PILEUP_HOST_CHECK

namespace {

// The LDS tile of k_pile_count: PU_TILE sites x 16 counters x 4 bytes.  A CU of the MI355X has 160 KiB of LDS and holds 32 waves; a block of
// 256 threads is 4 waves, so 8 blocks fill a CU and each may hold 160 KiB / 8 = 20 KiB.  256 sites are 16 KiB (+ 64 bytes of tile starts): a
// block's 16 reads of a sorted panel span a read length and a little.
#define PU_TILE 256u
#define PU_LDS_PER_CU (160u << 10)
#define PU_BLOCKS_PER_CU 8u
static_assert(PU_TILE * 64u + 64u <= PU_LDS_PER_CU / PU_BLOCKS_PER_CU, "k_pile_count's tile must leave the CU its 8 blocks of 4 waves");

// misc: [0] the lowest malformed record (atomicMin), [1..6] the skip counters of rule E in its order, [7] eligible records, [8] their n_cigar_op summed
__global__ __launch_bounds__(256) void k_pile_scan(const uint8_t *u, const uint64_t *off, uint64_t n, uint64_t end, uint64_t gbase, pileup::Params P, pileup::Sites S, uint32_t *meta,
                                                   unsigned long long *misc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    pileup::Rec R; R.first = PU_NONE; R.nc = 0; R.bad = 0; R.skip = 0;
    const bool live = i < n;
    if (live) {
        const uint64_t a = off[i];
        pileup::scan_record(u + a, a < end ? end - a : 0, P, S, R);
        meta[i] = R.bad ? PU_NONE : R.first;
        if (R.bad) atomicMin(misc, (unsigned long long)(gbase + i));
    }
    const bool elig = live && !R.bad && !R.skip;
    unsigned long long b[7];
#pragma unroll
    for (int k = 1; k <= 6; k++) b[k] = __ballot(R.skip == k);
    b[0] = __ballot(elig);
    uint32_t ops = elig ? R.nc : 0u;
#pragma unroll
    for (int d = 32; d; d >>= 1) ops += __shfl_xor(ops, d);
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 1; k <= 6; k++) if (b[k]) atomicAdd(misc + k, (unsigned long long)__popcll(b[k]));
        if (b[0]) atomicAdd(misc + 7, (unsigned long long)__popcll(b[0]));
        if (ops) atomicAdd(misc + 8, (unsigned long long)ops);
    }
}

// an add of k_pile_count: into the block's tile when the counter lies in it, else to memory
template <bool DIRECT> struct PileAdd {
    uint32_t *tile, *counts; uint32_t base16;
    __device__ __forceinline__ void operator()(uint32_t idx) {
        const uint32_t d = idx - base16;                                              // (a counter in front of the tile wraps beyond it)
        if (!DIRECT && d < PU_TILE * 16u) atomicAdd(tile + d, 1u);
        else atomicAdd(counts + idx, 1u);
    }
};
// 16 lanes per record, 16 records per block (block b: records [16 b, 16 b + 16) of the window); n_counts: 16 x the number of sites
template <bool DIRECT> __global__ __launch_bounds__(256) void k_pile_count(const uint8_t *u, const uint64_t *off, uint64_t n, pileup::Params P, pileup::Sites S, const uint32_t *meta,
                                                                           uint32_t *counts, uint64_t n_counts) {
    __shared__ uint32_t s_tile[DIRECT ? 1 : PU_TILE * 16u];
    __shared__ uint32_t s_base[16];
    const uint32_t g = threadIdx.x >> 4, sub = threadIdx.x & 15u;
    const uint64_t j = (uint64_t)blockIdx.x * 16u + g;
    const uint32_t first = j < n ? meta[j] : PU_NONE;
    uint32_t base = 0;
    if (!DIRECT) {
        for (uint32_t i = threadIdx.x; i < PU_TILE * 16u; i += 256u) s_tile[i] = 0u;
        if (sub == 0) {                                                               // the first site this record can touch: that of max(pos - 1, the interval's start)
            uint32_t b = PU_NONE;
            if (first != PU_NONE) {
                const int32_t pos = (int32_t)rb32(u + off[j] + 8);
                const pileup::Ivl v = S.iv[first];
                b = v.site0 + (uint32_t)(max(pos - 1, v.start) - v.start);
            }
            s_base[g] = b;
        }
        __syncthreads();
        base = PU_NONE;
#pragma unroll
        for (int k = 15; k >= 0; k--) if (s_base[k] != PU_NONE) base = s_base[k];       // the block's first overlapping record's
        if (base == PU_NONE) return;                                                  // (the whole block: no record of it touches a site)
    }
    PileAdd<DIRECT> add{s_tile, counts, base * 16u};
    if (first != PU_NONE) pileup::count_record(u + off[j], P, S, first, sub, 16u, add);
    if (!DIRECT) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < PU_TILE * 16u; i += 256u) {
            const uint32_t v = s_tile[i];
            const uint64_t at = (uint64_t)base * 16u + i;
            if (v && at < n_counts) atomicAdd(counts + at, v);
        }
    }
}

}  // namespace

struct gce_pileup {
    int32_t device = 0;
    hipStream_t s = nullptr;
    std::string err;
    uint64_t budget = 0;                                                              // device bytes the process may hold (0: no limit beyond the device)
    pileup::Params P{0, 0, 0, 0}; bool direct = false;
    WinIdx w; DevBuf tmp, misc, meta;                                                 // the window; the counters of k_pile_scan; 4 bytes per window record
    DevBuf iv, tfirst, counts; uint64_t n_sites = 0, n_iv = 0; bool sites_set = false; // rule S's table; 64 bytes per site
    uint64_t n = 0;                                                                   // records so far
};

static int pile_fail(gce_pileup *p, int code, const std::string &m) { if (p) p->err = m; return code; }
static int pile_oom(gce_pileup *p, const char *what, uint64_t add) {
    char m[256];
    snprintf(m, sizeof m, "out of device memory: gce_bam_pileup needs 64 bytes per site (%llu sites: %llu bytes) + 16 bytes per interval + one window + 4 bytes per window record "
                          "(%lld bytes live, budget %llu, %llu more for %s)", (unsigned long long)p->n_sites, (unsigned long long)p->n_sites * 64ull,
             __atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), (unsigned long long)p->budget, (unsigned long long)add, what);
    return pile_fail(p, GCE_ERR_OOM, m);
}
static bool pile_room(const gce_pileup *p, uint64_t add) {
    return !p->budget || (uint64_t)std::max<long long>(__atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), 0) + add <= p->budget;
}
#define PUCHK(call) do { hipError_t _e = (call); if (_e == hipErrorOutOfMemory) return pile_oom(p, #call, 0); if (_e != hipSuccess) return pile_fail(p, GCE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); } while (0)

extern "C" {

// options: GCE_PILEUP_DIRECT or 0.  The thresholds are the runner's, checked there.
int gce_pileup_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_pileup **out) {
    if (!out) return GCE_ERR_INVALID;
    *out = nullptr;
    if (options & ~(uint32_t)GCE_PILEUP_DIRECT) return GCE_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    gce_pileup *p = new gce_pileup();
    p->device = device; p->budget = (uint64_t)device_budget_bytes;
    p->P.min_mapq = min_mapq; p->P.min_baseq = min_baseq; p->P.exclude = exclude_flags; p->direct = (options & GCE_PILEUP_DIRECT) != 0;
    if (hipStreamCreate(&p->s) != hipSuccess) { delete p; return GCE_ERR_HIP; }
    *out = p;
    return GCE_OK;
}
void gce_pileup_destroy(gce_pileup *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->s);
    p->w.release();
    for (DevBuf *x : {&p->tmp, &p->misc, &p->meta, &p->iv, &p->tfirst, &p->counts}) x->release();
    (void)hipStreamDestroy(p->s);
    delete p;
}
const char *gce_pileup_error(gce_pileup *p) { return p ? p->err.c_str() : ""; }

// rule S's intervals, once, in front of the first window: interval j = [start[j], end[j]) of contig tid[j], in (tid, start) order, disjoint and
// not abutting, inside the contig; site0[j]: the site index of start[j] (the sum of the lengths in front of it).  The counters are made and zeroed.
int gce_pileup_set_sites(gce_pileup *p, int32_t n_ref, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, const uint32_t *site0) {
    if (!p || p->sites_set || n_ref < 0 || n_intervals < 0 || (n_intervals && (!tid || !start || !end || !site0))) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    std::vector<pileup::Ivl> iv((size_t)n_intervals);
    std::vector<uint32_t> tf((size_t)n_ref + 1, 0);
    uint64_t sites = 0;
    for (int64_t j = 0; j < n_intervals; j++) {
        const bool ordered = j == 0 || tid[j - 1] < tid[j] || (tid[j - 1] == tid[j] && end[j - 1] < start[j]);
        if (tid[j] < 0 || tid[j] >= n_ref || start[j] < 0 || end[j] <= start[j] || !ordered || site0[j] != sites) return pile_fail(p, GCE_ERR_INVALID, "gce_pileup_set_sites: intervals out of rule S's order");
        iv[(size_t)j] = {tid[j], start[j], end[j], site0[j]};
        sites += (uint64_t)(end[j] - start[j]);
        if (sites > PU_MAX_SITES) return pile_fail(p, GCE_ERR_INVALID, "more than 2^28 sites");
        tf[(size_t)tid[j] + 1]++;
    }
    for (int32_t t = 0; t < n_ref; t++) tf[(size_t)t + 1] += tf[(size_t)t];
    p->n_sites = sites; p->n_iv = (uint64_t)n_intervals; p->P.n_ref = n_ref;
    const uint64_t need = DevBuf::padded(sites * 64 + 64) + DevBuf::padded(iv.size() * sizeof(pileup::Ivl) + 64) + DevBuf::padded(tf.size() * 4) + DevBuf::padded(128);
    if (!pile_room(p, need)) return pile_oom(p, "the counters and the interval table", need);
    PUCHK(p->counts.ensure(sites * 64 + 64)); PUCHK(p->iv.ensure(iv.size() * sizeof(pileup::Ivl) + 64)); PUCHK(p->tfirst.ensure(tf.size() * 4)); PUCHK(p->misc.ensure(128));
    PUCHK(hipMemsetAsync(p->counts.p, 0, sites * 64 + 64, s));
    if (!iv.empty()) PUCHK(hipMemcpyAsync(p->iv.p, iv.data(), iv.size() * sizeof(pileup::Ivl), hipMemcpyHostToDevice, s));
    PUCHK(hipMemcpyAsync(p->tfirst.p, tf.data(), tf.size() * 4, hipMemcpyHostToDevice, s));
    const unsigned long long init[9] = {~0ull, 0, 0, 0, 0, 0, 0, 0, 0};
    PUCHK(hipMemcpyAsync(p->misc.p, init, sizeof init, hipMemcpyHostToDevice, s));
    PUCHK(hipStreamSynchronize(s));
    p->sites_set = true;
    return GCE_OK;
}

// the next piece of the file, as gce_bai_window takes it; *pileup_s: the seconds of k_pile_scan and k_pile_count, added to.  GCE_ERR_INVALID
// names the lowest malformed record, counting from 0 over the file.
int gce_pileup_window(gce_pileup *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                      int32_t n_ref, int32_t last, double *pileup_s) {
    if (!p || !p->sites_set || n_ref != p->P.n_ref || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize))) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    {
        uint64_t u_all = p->w.carry_n; for (int32_t k = 0; k < n_members; k++) u_all += usize[k];
        const uint64_t add = win_room(p->w, comp_bytes, u_all);
        if (add && !pile_room(p, add)) return pile_oom(p, "a window of the file", add);
    }
    uint64_t total = 0, n_rec = 0, end = 0;
    int rc = win_inflate_index(p->w, p->tmp, s, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, nullptr, &total, &n_rec, &end, p->err);
    if (rc == GCE_ERR_OOM) return pile_oom(p, "a window of the file", 0);
    if (rc != GCE_OK) return rc;
    if (n_rec) {
        const double t0 = mono_s();
        if (n_rec * 4 > p->meta.cap) {
            const uint64_t add = DevBuf::padded(n_rec * 4);
            if (!pile_room(p, add)) return pile_oom(p, "the meta of a window's records", add);
            PUCHK(p->meta.ensure(n_rec * 4));
        }
        const uint8_t *u = (const uint8_t *)p->w.win.p; const uint64_t *off = (const uint64_t *)p->w.idx.off.p;
        const pileup::Sites S{p->iv.as<pileup::Ivl>(), p->tfirst.as<uint32_t>()};
        unsigned long long *misc = p->misc.as<unsigned long long>();
        hipLaunchKernelGGL(k_pile_scan, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, u, off, n_rec, end, p->n, p->P, S, p->meta.as<uint32_t>(), misc);
        PUCHK(hipGetLastError());
        unsigned long long bad = ~0ull;
        PUCHK(hipMemcpyAsync(&bad, misc, 8, hipMemcpyDeviceToHost, s)); PUCHK(hipStreamSynchronize(s)); PUCHK(hipGetLastError());
        if (bad != ~0ull) {
            char m[160]; snprintf(m, sizeof m, "BAM record %llu (counting from 0): its fields overrun its block_size", bad);
            return pile_fail(p, GCE_ERR_INVALID, m);
        }
        if (p->n_sites) {
            const unsigned nb = (unsigned)((n_rec + 15) / 16);
            if (p->direct) hipLaunchKernelGGL(k_pile_count<true>, dim3(nb), dim3(256), 0, s, u, off, n_rec, p->P, S, (const uint32_t *)p->meta.p, p->counts.as<uint32_t>(), p->n_sites * 16);
            else hipLaunchKernelGGL(k_pile_count<false>, dim3(nb), dim3(256), 0, s, u, off, n_rec, p->P, S, (const uint32_t *)p->meta.p, p->counts.as<uint32_t>(), p->n_sites * 16);
            PUCHK(hipGetLastError()); PUCHK(hipStreamSynchronize(s)); PUCHK(hipGetLastError());
        }
        p->n += n_rec;
        if (pileup_s) *pileup_s += mono_s() - t0;
    }
    return win_carry(p->w, s, total, end, p->err);
}

// after the last window: counters[0] records, [1..6] the skip counters of rule E in its order, [7] eligible; counts_out (NULL, or room for
// 16 uint32 per site): the counters.  GCE_ERR_INVALID when the eligible records' n_cigar_op sum to 2^32 or more.
int gce_pileup_finish(gce_pileup *p, int64_t counters[8], uint32_t *counts_out) {
    if (!p || !p->sites_set || !counters) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    PUCHK(hipStreamSynchronize(s));
    p->w.release(); p->meta.release();
    unsigned long long h[9];
    PUCHK(hipMemcpyAsync(h, p->misc.p, sizeof h, hipMemcpyDeviceToHost, s)); PUCHK(hipStreamSynchronize(s));
    counters[0] = (int64_t)p->n;
    for (int k = 1; k <= 7; k++) counters[k] = (int64_t)h[k];
    if (h[8] >> 32) return pile_fail(p, GCE_ERR_INVALID, "the eligible records hold 2^32 CIGAR operations or more: the 32-bit counters cannot be shown to hold");
    if (counts_out && p->n_sites) { PUCHK(hipMemcpyAsync(counts_out, p->counts.p, p->n_sites * 64, hipMemcpyDeviceToHost, s)); PUCHK(hipStreamSynchronize(s)); }
    PUCHK(hipGetLastError());
    return GCE_OK;
}

}  // extern "C"
#undef PUCHK
#endif  // GCE_PILEUP_HOST_CHECK
