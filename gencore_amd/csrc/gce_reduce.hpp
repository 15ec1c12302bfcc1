// gce_reduce.hpp — what a windowed reduce pass is: the part gce_bam_pileup (gce_pileup.hpp) and gce_bam_error_profile
// (gce_errprof.hpp) share, and what a third pass of their kind starts from (gce_errsup.hpp, DESIGN.md 4n, is one).  Such a pass streams the file window by window
// (win_inflate_index / win_carry, gce_passes.hpp) and keeps nothing of a window but what it added to counters that stay on the device: per window
// k_reduce_scan runs one thread per record over the pass's scan functor and leaves 4 bytes of meta per record, then the pass's own count kernels
// walk the records the meta keeps.  reduce::rule_e (the malformed-record test and rule E), rule S's interval table with its searches, the
// decode of a record's header (reduce::Head) and the class of a 4-bit base (reduce::read_class) are __host__ __device__: the passes' host
// checks (tests/pileup_host_check.hip, tests/errprof_host_check.hip) compile that half alone.
// ReduceSession is the device object: the out-of-memory message, the interval upload, the window sequence and the counter read-back, once.
#pragma once
#include <cstdint>

namespace reduce {

#define RD_HD __host__ __device__ inline

typedef uint32_t __attribute__((aligned(1), may_alias)) rd_u32u;
typedef uint16_t __attribute__((aligned(1), may_alias)) rd_u16u;

#define RD_NONE 0xFFFFFFFFu
// what rule_e returns: BAD, ELIGIBLE, or the one counter of rule E the record goes to, in rule E's order; a pass's own skips go on from N_SKIP + 1
enum { BAD = -1, ELIGIBLE = 0, SKIP_UNPLACED, SKIP_FLAGGED, SKIP_LOW_MAPQ, SKIP_NO_CIGAR, SKIP_NO_SEQ, SKIP_BAD_CIGAR, N_SKIP = SKIP_BAD_CIGAR };

// rule S on the device: interval j = sites [start, end) of contig tid, the site of `start` has index site0; the intervals of contig t are
// [tfirst[t], tfirst[t + 1]), in ascending order, disjoint and not abutting
struct Ivl { int32_t tid, start, end; uint32_t site0; };
struct Sites { const Ivl *iv; const uint32_t *tfirst; };
// the core fields of an eligible record; rlen: the reference bases its CIGAR spans
struct Core { int32_t tid, pos, l_seq; uint32_t n_cigar_op, flag; int64_t rlen; };

// One record (r at its block_size, `avail` bytes from r to the end of the buffer).  BAD: block_size < 32 or beyond the buffer, or fields that
// overrun block_size.  No byte is read outside r[0, min(avail, 4 + block_size)).  C is set for an ELIGIBLE record alone.
RD_HD int rule_e(const uint8_t *r, uint64_t avail, int32_t n_ref, int32_t min_mapq, uint32_t exclude, Core &C) {
    if (avail < 4) return BAD;
    const uint64_t bs = *(const rd_u32u *)r;
    if (bs < 32 || 4 + bs > avail) return BAD;
    const uint8_t *c = r + 4;
    const int32_t tid = (int32_t) * (const rd_u32u *)(c + 0), pos = (int32_t) * (const rd_u32u *)(c + 4), lseq = (int32_t) * (const rd_u32u *)(c + 16);
    const uint32_t lq = c[8], mapq = c[9], nc = *(const rd_u16u *)(c + 12), flag = *(const rd_u16u *)(c + 14);
    if (lseq < 0 || 32ull + lq + 4ull * nc + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > bs) return BAD;
    // ---- rule E, in its order
    if (tid < 0 || tid >= n_ref || pos < 0) return SKIP_UNPLACED;
    if (flag & exclude) return SKIP_FLAGGED;
    if ((int32_t)mapq < min_mapq) return SKIP_LOW_MAPQ;
    if (nc == 0) return SKIP_NO_CIGAR;
    if (lseq == 0) return SKIP_NO_SEQ;
    const uint8_t *cg = c + 32 + lq;
    uint64_t qn = 0; int64_t rlen = 0;
    for (uint32_t k = 0; k < nc; k++) {
        const uint32_t w = *(const rd_u32u *)(cg + 4 * k), op = w & 15u;
        if (op > 8) return SKIP_BAD_CIGAR;
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qn += w >> 4;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += w >> 4;
    }
    if (qn != (uint64_t)lseq) return SKIP_BAD_CIGAR;
    C.tid = tid; C.pos = pos; C.l_seq = lseq; C.n_cigar_op = nc; C.flag = flag; C.rlen = rlen;
    return ELIGIBLE;
}

// the first interval of contig tid that ends behind pos - 1, if it starts in front of `limit` (exclusive); RD_NONE: there is none
RD_HD uint32_t first_interval(const Sites &S, int32_t tid, int32_t pos, int64_t limit) {
    uint32_t lo = S.tfirst[tid]; const uint32_t tend = S.tfirst[tid + 1]; uint32_t hi = tend;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (S.iv[mid].end < pos) lo = mid + 1; else hi = mid; }
    return lo < tend && (int64_t)S.iv[lo].start < limit ? lo : RD_NONE;
}

// the first interval of [cur, tend) that ends at or behind x (every interval in front of it holds neither x - 1 nor anything behind it)
RD_HD uint32_t seek(const Sites &S, uint32_t cur, uint32_t tend, int64_t x) {
    if (cur >= tend || (int64_t)S.iv[cur].end >= x) return cur;
    uint32_t lo = cur + 1, hi = tend;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((int64_t)S.iv[mid].end < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// The fields of a record (r at its block_size) that the CIGAR walks read, decoded once: the passes' walks for the record they walk,
// fragpile::column and errprof::Cursor for the partner.  The constructor reads the record's fixed part alone; has_q() reads the first quality
// byte, which lies behind the sequence: a walk asks once and keeps the answer, fragpile::column asks only at a column it has found
struct Head {
    const uint8_t *cg, *sq, *ql; int32_t tid, pos, lseq; uint32_t nc, flag;
    RD_HD explicit Head(const uint8_t *r) {
        const uint8_t *c = r + 4;
        tid = (int32_t) * (const rd_u32u *)(c + 0); pos = (int32_t) * (const rd_u32u *)(c + 4); lseq = (int32_t) * (const rd_u32u *)(c + 16);
        nc = *(const rd_u16u *)(c + 12); flag = *(const rd_u16u *)(c + 14);
        cg = c + 32 + c[8]; sq = cg + 4 * nc; ql = sq + ((uint32_t)lseq + 1) / 2;
    }
    RD_HD bool has_q() const { return ql[0] != 0xFF; }
};
// the class of a read's 4-bit base: 0..3 = A C G T, 4 = anything else
RD_HD uint32_t read_class(const uint8_t *sq, uint32_t yi) {
    const uint32_t nib = (sq[yi >> 1] >> ((~yi & 1u) << 2)) & 15u;
    return nib == 1 ? 0u : nib == 2 ? 1u : nib == 4 ? 2u : nib == 8 ? 3u : 4u;
}

#undef RD_HD

}  // namespace reduce

#if !defined(GCE_PILEUP_HOST_CHECK) && !defined(GCE_ERRPROF_HOST_CHECK)

namespace {

// The scan of a window, one thread per record.  SCAN is the pass's functor: SCAN::Rec is what its scan_record learns about a record (first,
// bad, skip), scan(r, avail, R) runs it, SCAN::NSKIP is the number of its skip counters, SCAN::OPS says whether scan.ops(R) of the eligible
// records is summed as well.  misc: [0] the lowest malformed record (atomicMin), [1..NSKIP] the skip counters in the pass's order,
// [NSKIP + 1] eligible records, [NSKIP + 2] with OPS, that sum.  meta[i]: R.first, RD_NONE for a malformed record.
template <class SCAN> __global__ __launch_bounds__(256) void k_reduce_scan(const uint8_t *u, const uint64_t *off, uint64_t n, uint64_t end, uint64_t gbase, SCAN scan, uint32_t *meta,
                                                                           unsigned long long *misc) {
    constexpr int NSKIP = SCAN::NSKIP;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    typename SCAN::Rec R{}; R.first = RD_NONE;
    const bool live = i < n;
    if (live) {
        const uint64_t a = off[i];
        scan(u + a, a < end ? end - a : 0, R);
        meta[i] = R.bad ? RD_NONE : R.first;
        if (R.bad) atomicMin(misc, (unsigned long long)(gbase + i));
    }
    const bool elig = live && !R.bad && !R.skip;
    unsigned long long b[NSKIP + 1];
#pragma unroll
    for (int k = 1; k <= NSKIP; k++) b[k] = __ballot(R.skip == k);
    b[0] = __ballot(elig);
    uint32_t ops = 0;
    if constexpr (SCAN::OPS) {
        ops = elig ? scan.ops(R) : 0u;
#pragma unroll
        for (int d = 32; d; d >>= 1) ops += __shfl_xor(ops, d);
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 1; k <= NSKIP; k++) if (b[k]) atomicAdd(misc + k, (unsigned long long)__popcll(b[k]));
        if (b[0]) atomicAdd(misc + NSKIP + 1, (unsigned long long)__popcll(b[0]));
        if (SCAN::OPS && ops) atomicAdd(misc + NSKIP + 2, (unsigned long long)ops);
    }
}

}  // namespace

#define RD_MISC_WORDS 16
struct RdTable { std::vector<reduce::Ivl> iv; std::vector<uint32_t> tf; uint64_t sites = 0; };

// The device object of a reduce pass; the pass derives its own from it and adds its parameters, its counters and what else stays resident.
struct ReduceSession {
    int32_t device = 0;
    hipStream_t s = nullptr;
    std::string err;
    uint64_t budget = 0;                                                              // device bytes the process may hold (0: no limit beyond the device)
    WinIdx w; DevBuf tmp, misc, meta;                                                 // the window; the counters of k_reduce_scan; 4 bytes per window record
    DevBuf iv, tfirst; bool sites_set = false;                                        // rule S's table
    uint64_t n = 0;                                                                   // records so far
    virtual std::string needs() const = 0;                                            // "<entry point> needs <what the pass itself holds>", for the out-of-memory message

    int fail(int code, const std::string &m) { err = m; return code; }
    int oom(const char *what, uint64_t add) {
        char m[256];
        snprintf(m, sizeof m, "out of device memory: %s + 16 bytes per interval + one window + 4 bytes per window record (%lld bytes live, budget %llu, %llu more for %s)", needs().c_str(),
                 __atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), (unsigned long long)budget, (unsigned long long)add, what);
        return fail(GCE_ERR_OOM, m);
    }
    bool room(uint64_t add) const { return !budget || (uint64_t)std::max<long long>(__atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), 0) + add <= budget; }
    reduce::Sites sites() const { return reduce::Sites{iv.as<reduce::Ivl>(), tfirst.as<uint32_t>()}; }
    int out_of_order(const char *entry) { return fail(GCE_ERR_INVALID, std::string(entry) + ": intervals out of rule S's order"); }
};
// (p: the session, or the pass's object)
#define RDCHK(call) do { hipError_t _e = (call); if (_e == hipErrorOutOfMemory) return p->oom(#call, 0); if (_e != hipSuccess) return p->fail(GCE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); } while (0)

// options: direct_bit (the pass's count kernel without LDS) or 0.  The thresholds are the runner's, checked there.
template <class T> static int rd_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint32_t direct_bit, T **out) {
    if (!out) return GCE_ERR_INVALID;
    *out = nullptr;
    if (options & ~direct_bit) return GCE_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    T *p = new T();
    p->device = device; p->budget = (uint64_t)device_budget_bytes;
    p->P.min_mapq = min_mapq; p->P.min_baseq = min_baseq; p->P.exclude = exclude_flags; p->direct = (options & direct_bit) != 0;
    if (hipStreamCreate(&p->s) != hipSuccess) { delete p; return GCE_ERR_HIP; }
    *out = p;
    return GCE_OK;
}
// own: the buffers the pass added
template <class T> static void rd_destroy(T *p, std::initializer_list<DevBuf *> own) {
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->s);
    p->w.release();
    for (DevBuf *x : {&p->tmp, &p->misc, &p->meta, &p->iv, &p->tfirst}) x->release();
    for (DevBuf *x : own) x->release();
    (void)hipStreamDestroy(p->s);
    delete p;
}

// rule S's intervals on the host: interval j = [start[j], end[j]) of contig tid[j], in (tid, start) order, disjoint and not abutting, inside
// [0, n_ref); t.iv with the site index of every start (the sum of the lengths in front of it), t.tf the per-tid first-interval table, t.sites
// their sites.  entry: the entry point that names itself in the refusal.
static int rd_intervals(ReduceSession *p, const char *entry, int32_t n_ref, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, RdTable &t) {
    t.iv.resize((size_t)n_intervals); t.tf.assign((size_t)n_ref + 1, 0); t.sites = 0;
    for (int64_t j = 0; j < n_intervals; j++) {
        const bool ordered = j == 0 || tid[j - 1] < tid[j] || (tid[j - 1] == tid[j] && end[j - 1] < start[j]);
        if (tid[j] < 0 || tid[j] >= n_ref || start[j] < 0 || end[j] <= start[j] || !ordered) return p->out_of_order(entry);
        t.iv[(size_t)j] = {tid[j], start[j], end[j], (uint32_t)t.sites};
        t.sites += (uint64_t)(end[j] - start[j]);
        t.tf[(size_t)tid[j] + 1]++;
    }
    for (int32_t k = 0; k < n_ref; k++) t.tf[(size_t)k + 1] += t.tf[(size_t)k];
    return GCE_OK;
}
// ... and on the device, once, in front of the first window: the pass's counters (counts_bytes of them) are made and zeroed, the first
// misc_words of the scan's counters are ~0 and zeros
static int rd_set_sites(ReduceSession *p, const RdTable &t, DevBuf &counts, uint64_t counts_bytes, int misc_words) {
    hipStream_t s = p->s;
    const uint64_t need = DevBuf::padded(counts_bytes) + DevBuf::padded(t.iv.size() * sizeof(reduce::Ivl) + 64) + DevBuf::padded(t.tf.size() * 4) + DevBuf::padded(RD_MISC_WORDS * 8);
    if (!p->room(need)) return p->oom("the counters and the interval table", need);
    RDCHK(counts.ensure(counts_bytes)); RDCHK(p->iv.ensure(t.iv.size() * sizeof(reduce::Ivl) + 64)); RDCHK(p->tfirst.ensure(t.tf.size() * 4)); RDCHK(p->misc.ensure(RD_MISC_WORDS * 8));
    RDCHK(hipMemsetAsync(counts.p, 0, counts_bytes, s));
    if (!t.iv.empty()) RDCHK(hipMemcpyAsync(p->iv.p, t.iv.data(), t.iv.size() * sizeof(reduce::Ivl), hipMemcpyHostToDevice, s));
    RDCHK(hipMemcpyAsync(p->tfirst.p, t.tf.data(), t.tf.size() * 4, hipMemcpyHostToDevice, s));
    const unsigned long long init[RD_MISC_WORDS] = {~0ull};
    RDCHK(hipMemcpyAsync(p->misc.p, init, (size_t)misc_words * 8, hipMemcpyHostToDevice, s));
    RDCHK(hipStreamSynchronize(s));
    p->sites_set = true;
    return GCE_OK;
}

// The next piece of the file, as gce_bai_window takes it: the window inflated and indexed, scanned by k_reduce_scan<SCAN>, then
// count(u, off, n_rec, end) launches the pass's count kernel or kernels on the session's stream (false: it launched none).  *secs: the seconds
// of the scan and the count, added to.  pass_n_ref: the contigs the pass was set up with.  GCE_ERR_INVALID names the lowest malformed record,
// counting from 0 over the file.
template <class SCAN, class COUNT> static int rd_window(ReduceSession *p, const SCAN &scan, int32_t pass_n_ref, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff,
                                                         const uint32_t *csize, const uint32_t *usize, uint64_t skip, int32_t n_ref, int32_t last, double *secs, COUNT &&count) {
    if (!p->sites_set || n_ref != pass_n_ref || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize))) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    {
        uint64_t u_all = p->w.carry_n; for (int32_t k = 0; k < n_members; k++) u_all += usize[k];
        const uint64_t add = win_room(p->w, comp_bytes, u_all);
        if (add && !p->room(add)) return p->oom("a window of the file", add);
    }
    uint64_t total = 0, n_rec = 0, end = 0;
    int rc = win_inflate_index(p->w, p->tmp, s, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, nullptr, &total, &n_rec, &end, p->err);
    if (rc == GCE_ERR_OOM) return p->oom("a window of the file", 0);
    if (rc != GCE_OK) return rc;
    if (n_rec) {
        const double t0 = mono_s();
        if (n_rec * 4 > p->meta.cap) {
            const uint64_t add = DevBuf::padded(n_rec * 4);
            if (!p->room(add)) return p->oom("the meta of a window's records", add);
            RDCHK(p->meta.ensure(n_rec * 4));
        }
        const uint8_t *u = (const uint8_t *)p->w.win.p; const uint64_t *off = (const uint64_t *)p->w.idx.off.p;
        unsigned long long *misc = p->misc.as<unsigned long long>();
        hipLaunchKernelGGL(k_reduce_scan<SCAN>, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, u, off, n_rec, end, p->n, scan, p->meta.as<uint32_t>(), misc);
        RDCHK(hipGetLastError());
        unsigned long long bad = ~0ull;
        RDCHK(hipMemcpyAsync(&bad, misc, 8, hipMemcpyDeviceToHost, s)); RDCHK(hipStreamSynchronize(s)); RDCHK(hipGetLastError());
        if (bad != ~0ull) {
            char m[160]; snprintf(m, sizeof m, "BAM record %llu (counting from 0): its fields overrun its block_size", bad);
            return p->fail(GCE_ERR_INVALID, m);
        }
        if (count(u, off, n_rec, end)) { RDCHK(hipGetLastError()); RDCHK(hipStreamSynchronize(s)); RDCHK(hipGetLastError()); }
        p->n += n_rec;
        if (secs) *secs += mono_s() - t0;
    }
    return win_carry(p->w, s, total, end, p->err);
}

// after the last window: the window and the meta are let go; h: the first misc_words of the scan's counters; counters[0] records,
// [1..nskip] the skip counters in the pass's order, [nskip + 1] eligible
static int rd_finish(ReduceSession *p, int nskip, int64_t *counters, unsigned long long *h, int misc_words) {
    hipStream_t s = p->s;
    RDCHK(hipStreamSynchronize(s));
    p->w.release(); p->meta.release();
    RDCHK(hipMemcpyAsync(h, p->misc.p, (size_t)misc_words * 8, hipMemcpyDeviceToHost, s)); RDCHK(hipStreamSynchronize(s));
    counters[0] = (int64_t)p->n;
    for (int k = 1; k <= nskip + 1; k++) counters[k] = (int64_t)h[k];
    return GCE_OK;
}

#endif  // the host checks
