// gce_bai.hpp — the BAI index of a coordinate-sorted BAM on the GPU (gce_bam_index).  The file is streamed window by window as
// the pass runner streams it (win_inflate_index / win_carry, gce_passes.hpp): the host hands whole BGZF members, the GPU inflates them behind the
// record the last window's end cut and finds the record starts (dev_inflate_members, dev_record_index: gce_devstream.hpp).  Per record one 24-byte fact stays resident (BaiFact: tid, pos, end, bin,
// mapped bit, start virtual offset); nothing else of a window outlives it.  After the last window:
//   k_bai_check     the first record that breaks (tid, pos) order or BAI's range (atomicMin), run heads, contig spans, the mapped bits
//   k_bai_runs      one chunk per run of records with one (tid, bin); hipcub::DeviceRadixSort orders them by (tid, bin), stable: file order
//   k_bai_merge     the chunks of one bin that share a BGZF block merge (heads flagged and compacted)
//   k_bai_nintv / k_bai_lin_min / k_bai_lin_fill + a max-scan: the linear index
//   k_bai_meta      the pseudo-bin of every contig (ref_beg, ref_end, n_mapped, n_unmapped)
// The host copies the compacted arrays back and writes the SAMv1 5.2 layout (gce_bai_serialise).  The rules B/V/C/L/O the bytes follow are
// the issue's and DESIGN.md 4c's; tests/pybai.py models them.
#pragma once

namespace {

struct BaiFact { int32_t tid, pos, end; uint32_t bin_m; uint64_t voff; };     // bin_m: bin | mapped << 16; end saturates at INT32_MAX
static_assert(sizeof(BaiFact) == 24, "BaiFact is 24 bytes");
#define BAI_MAX_END (1ll << 29)

__device__ __forceinline__ uint32_t bai_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// one thread per record of the window (rule B; rule V: the record's start, by binary search over the window's non-empty members, whose
// inflated bytes follow each other from mem_u[0] on; the record the last window's end cut starts at carry_voff)
__global__ __launch_bounds__(256) void k_bai_facts(const uint8_t *u, const uint64_t *off, int64_t n, uint64_t carry_n, uint64_t carry_voff, const uint64_t *mem_u,
                                                   const uint64_t *mem_c, int32_t n_mem, BaiFact *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i];
    uint64_t voff = carry_voff;
    if (o >= carry_n) {
        int32_t lo = 0, hi = n_mem - 1;                                               // the last member that starts at or before o
        while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (mem_u[mid] <= o) lo = mid; else hi = mid - 1; }
        voff = mem_c[lo] << 16 | (o - mem_u[lo]);
    }
    const uint8_t *r = u + o + 4;
    const int32_t tid = (int32_t)rb32(r), pos = (int32_t)rb32(r + 4);
    const uint32_t bs = rb32(u + o), lq = r[8], flag = rb16(r + 14);
    uint32_t nc = rb16(r + 12);
    if (32ull + lq + 4ull * nc > bs) nc = 0;                                          // (the walk checked block_size only: stay inside the record)
    const uint8_t *cig = r + 32 + lq;
    int64_t rlen = 0;
    for (uint32_t k = 0; k < nc; k++) {
        const uint32_t w = rb32(cig + 4 * k), op = w & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += w >> 4;
    }
    if ((flag & 4u) || rlen == 0) rlen = 1;
    const int64_t beg = pos < 0 ? 0 : pos, end = beg + rlen;
    BaiFact f;
    f.tid = tid; f.pos = pos; f.end = (int32_t)min<int64_t>(end, 0x7FFFFFFFll);
    f.bin_m = (end <= BAI_MAX_END ? bai_reg2bin(beg, end) : 0u) | ((flag & 4u) ? 0u : 1u << 16);
    f.voff = voff;
    out[i] = f;
}

// rule O and what the later kernels need: bad = min(4 * record + kind) (kind 0: out of order, 1: ends beyond 2^29, 2: no contig of the header); nocoor = the first record
// with tid < 0; head: a run of one (tid, bin) starts here; cfirst / clast: the records [cfirst, clast) of every contig; mapped: indexed and mapped
__global__ __launch_bounds__(256) void k_bai_check(const BaiFact *f, int64_t n, int32_t n_ref, unsigned long long *bad, unsigned long long *nocoor, uint8_t *head,
                                                   uint32_t *cfirst, uint32_t *clast, uint8_t *mapped) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const BaiFact a = f[i];
    uint8_t h = 0, m = 0;
    if (a.tid < 0) atomicMin(nocoor, (unsigned long long)i);
    else {
        const bool prev = i > 0;
        const BaiFact p = prev ? f[i - 1] : a;
        if (prev && (p.tid < 0 || p.tid > a.tid || (p.tid == a.tid && p.pos > a.pos))) atomicMin(bad, 4ull * (unsigned long long)i);
        else if (a.end > BAI_MAX_END) atomicMin(bad, 4ull * (unsigned long long)i + 1);
        else if (a.tid >= n_ref) atomicMin(bad, 4ull * (unsigned long long)i + 2);
        else {
            h = !prev || p.tid != a.tid || (p.bin_m & 0xFFFFu) != (a.bin_m & 0xFFFFu);
            m = (uint8_t)(a.bin_m >> 16);
            if (!prev || p.tid != a.tid) cfirst[a.tid] = (uint32_t)i;
            if (i + 1 == n || f[i + 1].tid != a.tid) clast[a.tid] = (uint32_t)(i + 1);
        }
    }
    head[i] = h; mapped[i] = m;
}

// run r = records [h[r], h[r + 1]) (the last one ends at the first unplaced record, n_c): its chunk is the first record's start to the last
// record's end, which is the next record's start (rule V's end of the data, eod, behind the last record of the file)
__global__ __launch_bounds__(256) void k_bai_runs(const BaiFact *f, int64_t n, int64_t n_c, uint64_t eod, const uint32_t *h, const unsigned long long *n_runs,
                                                  unsigned long long *key, uint64_t *beg, uint64_t *end, uint32_t *idx) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t R = (int64_t)*n_runs;
    if (r >= R) return;
    const int64_t i0 = h[r], i1 = r + 1 < R ? (int64_t)h[r + 1] : n_c;
    key[r] = (unsigned long long)(uint32_t)f[i0].tid << 16 | (f[i0].bin_m & 0xFFFFu);
    beg[r] = f[i0].voff; end[r] = i1 < n ? f[i1].voff : eod;
    idx[r] = (uint32_t)r;
}

// rule C: the sorted chunk k starts a merged chunk unless the one before it has the same (tid, bin) and ends in the BGZF block k starts in
__global__ __launch_bounds__(256) void k_bai_merge(const unsigned long long *skey, const uint32_t *sr, const uint64_t *beg, const uint64_t *end, int64_t R, uint8_t *head) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= R) return;
    head[k] = k == 0 || skey[k] != skey[k - 1] || (end[sr[k - 1]] >> 16) < (beg[sr[k]] >> 16);
}
// merged chunk m = sorted chunks [mh[m], mh[m + 1]): the first one's start, the largest end
__global__ __launch_bounds__(256) void k_bai_chunks(const unsigned long long *skey, const uint32_t *sr, const uint64_t *beg, const uint64_t *end, int64_t R, const uint32_t *mh,
                                                    const unsigned long long *n_merged, uint64_t *out) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t M = (int64_t)*n_merged;
    if (m >= M) return;
    const int64_t k0 = mh[m], k1 = m + 1 < M ? (int64_t)mh[m + 1] : R;
    uint64_t e = 0;
    for (int64_t k = k0; k < k1; k++) e = max(e, end[sr[k]]);
    out[3 * m] = skey[k0]; out[3 * m + 1] = beg[sr[k0]]; out[3 * m + 2] = e;
}

// rule L: n_intv of every contig (the largest ((end - 1) >> 14) + 1 of its mapped records)
__global__ __launch_bounds__(256) void k_bai_nintv(const BaiFact *f, const uint8_t *mapped, int64_t n, uint32_t *nintv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !mapped[i]) return;
    atomicMax(nintv + f[i].tid, (uint32_t)((f[i].end - 1) >> 14) + 1u);
}
// the smallest start of the mapped records over every 16 kb window each one overlaps
__global__ __launch_bounds__(256) void k_bai_lin_min(const BaiFact *f, const uint8_t *mapped, int64_t n, const uint64_t *loff, unsigned long long *lin) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !mapped[i]) return;
    const BaiFact a = f[i];
    const int32_t beg = a.pos < 0 ? 0 : a.pos;
    unsigned long long *l = lin + loff[a.tid];
    for (int32_t w = beg >> 14; w <= (a.end - 1) >> 14; w++) atomicMin(l + w, (unsigned long long)a.voff);
}
// a window no mapped record overlaps takes its contig's ref_beg.  (The max-scan behind it then gives every later hole the window before it: the
// filled windows of a contig never decrease along it and lie above every earlier contig's, so the scan leaves them as they are.)
__global__ __launch_bounds__(256) void k_bai_lin_fill(const uint64_t *loff, int32_t n_ref, const uint32_t *cfirst, const BaiFact *f, unsigned long long *lin) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= loff[n_ref] || lin[x] != ~0ull) return;
    int32_t lo = 0, hi = n_ref - 1;                                                   // the last contig whose windows start at or before x
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (loff[mid] <= x) lo = mid; else hi = mid - 1; }
    lin[x] = f[cfirst[lo]].voff;
}

// the pseudo-bin of every contig with records: ref_beg, ref_end, n_mapped, n_unmapped (xs: the exclusive sum of the mapped bits)
__global__ __launch_bounds__(256) void k_bai_meta(const BaiFact *f, int64_t n, uint64_t eod, const uint32_t *cfirst, const uint32_t *clast, const uint64_t *xs, int32_t n_ref, uint64_t *meta) {
    const int32_t t = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n_ref) return;
    const uint32_t a = cfirst[t];
    if (a == 0xFFFFFFFFu) { meta[4 * t] = meta[4 * t + 1] = meta[4 * t + 2] = meta[4 * t + 3] = 0; return; }
    const uint32_t b = clast[t];
    const uint64_t nm = xs[b] - xs[a];
    meta[4 * t] = f[a].voff; meta[4 * t + 1] = (int64_t)b < n ? f[b].voff : eod;
    meta[4 * t + 2] = nm; meta[4 * t + 3] = (uint64_t)(b - a) - nm;
}

}  // namespace

struct gce_bai {
    int32_t device = 0;
    hipStream_t s = nullptr;
    std::string err;
    WinIdx w; DevBuf tmp, mem;                                                        // the window; its member table
    DevBuf facts; int64_t n = 0; uint64_t carry_voff = 0;                             // one BaiFact per record so far
    // what gce_bai_finish copies back
    std::vector<uint64_t> chunks, lin, meta; std::vector<uint64_t> loff; int64_t n_no_coor = 0;
};

static int bfail(gce_bai *b, int code, const std::string &m) { if (b) b->err = m; return code; }
#define BCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) return bfail(b, _e == hipErrorOutOfMemory ? GCE_ERR_OOM : GCE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); } while (0)

extern "C" {

int gce_bai_create(int32_t device, gce_bai **out) {
    if (!out) return GCE_ERR_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    gce_bai *b = new gce_bai();
    b->device = device;
    if (hipStreamCreate(&b->s) != hipSuccess) { delete b; return GCE_ERR_HIP; }
    *out = b;
    return GCE_OK;
}
void gce_bai_destroy(gce_bai *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->s);
    b->w.release(); b->tmp.release(); b->mem.release(); b->facts.release();
    (void)hipStreamDestroy(b->s);
    delete b;
}
const char *gce_bai_error(gce_bai *b) { return b ? b->err.c_str() : ""; }

// the next piece of the file, as gce_passes_window takes it; file_base: the file offset of comp[0] (member k lies at file_base + coff[k])
int gce_bai_window(gce_bai *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t file_base,
                   uint64_t skip, int32_t n_ref, int32_t last) {
    if (!b || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize))) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    // the window's non-empty members: where their bytes start in the window (behind the carried ones) and in the file
    std::vector<uint64_t> mt; uint64_t u = b->w.carry_n;
    for (int32_t k = 0; k < n_members; k++) if (usize[k]) { mt.push_back(u); mt.push_back(file_base + coff[k]); u += usize[k]; }
    const int32_t n_mem = (int32_t)(mt.size() / 2);
    const uint64_t carry_n = b->w.carry_n;
    uint64_t total = 0, n_rec = 0, end = 0;
    int rc = win_inflate_index(b->w, b->tmp, s, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, nullptr, &total, &n_rec, &end, b->err);
    if (rc != GCE_OK) return rc;
    if (n_rec) {
        if ((uint64_t)b->n + n_rec >= 0x7FFFFFF0ull) return bfail(b, GCE_ERR_INVALID, "more than 2^31 records in one BAM file");
        const hipError_t g = pass_grow(b->facts, (size_t)(b->n + (int64_t)n_rec) * sizeof(BaiFact), (size_t)b->n * sizeof(BaiFact), s);
        if (g != hipSuccess) {
            char m[160]; snprintf(m, sizeof m, "out of device memory for the index's per-record facts (%llu records, %zu bytes each)", (unsigned long long)(b->n + (int64_t)n_rec), sizeof(BaiFact));
            return bfail(b, g == hipErrorOutOfMemory ? GCE_ERR_OOM : GCE_ERR_HIP, m);
        }
        // (mem: mem_u at [0, n_mem), mem_c at [n_mem, 2 n_mem))
        std::vector<uint64_t> mu((size_t)std::max(n_mem, 1)), mc((size_t)std::max(n_mem, 1));
        for (int32_t k = 0; k < n_mem; k++) { mu[k] = mt[2 * k]; mc[k] = mt[2 * k + 1]; }
        BCHK(b->mem.ensure(mu.size() * 16 + 64));
        BCHK(hipMemcpyAsync(b->mem.p, mu.data(), mu.size() * 8, hipMemcpyHostToDevice, s));
        BCHK(hipMemcpyAsync(b->mem.as<uint64_t>() + mu.size(), mc.data(), mc.size() * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_bai_facts, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, (const uint8_t *)b->w.win.p, (const uint64_t *)b->w.idx.off.p, (int64_t)n_rec, carry_n, b->carry_voff,
                           (const uint64_t *)b->mem.p, (const uint64_t *)b->mem.as<uint64_t>() + mu.size(), n_mem, b->facts.as<BaiFact>() + b->n);
        BCHK(hipGetLastError());
        b->n += (int64_t)n_rec;
    }
    if (end < total && end >= carry_n && n_mem > 0) {                                 // rule V for the record the window's end cuts (one that
        int32_t j = n_mem - 1;                                                        // began in an earlier window keeps its start)
        while (j > 0 && mt[2 * j] > end) j--;
        b->carry_voff = mt[2 * j + 1] << 16 | (end - mt[2 * j]);
    }
    return win_carry(b->w, s, total, end, b->err);
}

// after the last window: the kernels of the index; eod: rule V's offset of the end of the data.  *bad_rec / *bad_kind: the first record that
// breaks rule O (-1: none) and why (0: order, 1: ends beyond 2^29, 2: no contig of the header); the compacted arrays stay in b for gce_bai_serialise.
int gce_bai_finish(gce_bai *b, int32_t n_ref, uint64_t eod, int64_t counts[5], int64_t *bad_rec, int32_t *bad_kind) {
    if (!b || n_ref < 0 || !counts || !bad_rec || !bad_kind) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    BCHK(hipStreamSynchronize(s));
    b->w.release(); b->mem.release();                                                 // (the last window is done with)
    *bad_rec = -1; *bad_kind = 0;
    const int64_t n = b->n;
    const size_t nr1 = (size_t)std::max(n_ref, 1);
    b->chunks.clear(); b->lin.clear(); b->meta.assign((size_t)n_ref * 4, 0); b->loff.assign((size_t)n_ref + 1, 0); b->n_no_coor = 0;
    for (int k = 0; k < 5; k++) counts[k] = 0;
    counts[0] = n;
    if (n == 0) return GCE_OK;
    const unsigned nb = (unsigned)((n + 255) / 256);
    ScopedBuf misc, head, mapped, cfirst, clast, xs, sel;
    BCHK(misc.ensure(64)); BCHK(head.ensure((size_t)n + 64)); BCHK(mapped.ensure((size_t)n + 64)); BCHK(cfirst.ensure(nr1 * 4)); BCHK(clast.ensure(nr1 * 4));
    BCHK(hipMemsetAsync(misc.p, 0xFF, 64, s)); BCHK(hipMemsetAsync(cfirst.p, 0xFF, nr1 * 4, s)); BCHK(hipMemsetAsync(clast.p, 0, nr1 * 4, s));
    unsigned long long *dm = misc.as<unsigned long long>();                           // [0] bad, [1] nocoor, [2] runs, [3] merged chunks
    const BaiFact *f = b->facts.as<BaiFact>();
    hipLaunchKernelGGL(k_bai_check, dim3(nb), dim3(256), 0, s, f, n, n_ref, dm, dm + 1, head.as<uint8_t>(), cfirst.as<uint32_t>(), clast.as<uint32_t>(), mapped.as<uint8_t>());
    unsigned long long h2[2];
    BCHK(hipMemcpyAsync(h2, dm, 16, hipMemcpyDeviceToHost, s)); BCHK(hipStreamSynchronize(s)); BCHK(hipGetLastError());
    if (h2[0] != ~0ull) { *bad_rec = (int64_t)(h2[0] >> 2); *bad_kind = (int32_t)(h2[0] & 3); return GCE_OK; }
    const int64_t n_c = h2[1] == ~0ull ? n : (int64_t)h2[1];                          // the records with tid >= 0 come first
    b->n_no_coor = n - n_c;
    counts[1] = b->n_no_coor;
    // ---- the pseudo-bins
    BCHK(xs.ensure((size_t)n * 8 + 16));
    BCHK(dev_exclusive_sum(mapped.as<uint8_t>(), (uint64_t)n, xs.as<uint64_t>(), b->tmp, s));
    {
        ScopedBuf meta; BCHK(meta.ensure(nr1 * 32));
        if (n_ref) hipLaunchKernelGGL(k_bai_meta, dim3((unsigned)((n_ref + 255) / 256)), dim3(256), 0, s, f, n, eod, (const uint32_t *)cfirst.p, (const uint32_t *)clast.p, (const uint64_t *)xs.p, n_ref, meta.as<uint64_t>());
        if (n_ref) BCHK(hipMemcpyAsync(b->meta.data(), meta.p, (size_t)n_ref * 32, hipMemcpyDeviceToHost, s));
        BCHK(hipStreamSynchronize(s)); BCHK(hipGetLastError());
    }
    xs.release();
    if (n_c == 0) return GCE_OK;
    // ---- the chunks: runs, sorted by (tid, bin), merged
    BCHK(sel.ensure((size_t)n_c * 4 + 64));
    BCHK(dev_select_flagged(head.as<uint8_t>(), (uint64_t)n_c, sel.as<uint32_t>(), dm + 2, b->tmp, s));
    unsigned long long R = 0;
    BCHK(hipMemcpyAsync(&R, dm + 2, 8, hipMemcpyDeviceToHost, s)); BCHK(hipStreamSynchronize(s));
    {
        ScopedBuf key, skey, beg, end, idx, sidx, st, mh, out;
        BCHK(key.ensure(R * 8)); BCHK(skey.ensure(R * 8)); BCHK(beg.ensure(R * 8)); BCHK(end.ensure(R * 8)); BCHK(idx.ensure(R * 4)); BCHK(sidx.ensure(R * 4));
        const unsigned rb = (unsigned)((R + 255) / 256);
        hipLaunchKernelGGL(k_bai_runs, dim3(rb), dim3(256), 0, s, f, n, n_c, eod, (const uint32_t *)sel.p, (const unsigned long long *)(dm + 2), key.as<unsigned long long>(), beg.as<uint64_t>(),
                           end.as<uint64_t>(), idx.as<uint32_t>());
        size_t tb = 0;
        BCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, key.as<unsigned long long>(), skey.as<unsigned long long>(), idx.as<uint32_t>(), sidx.as<uint32_t>(), (int)R, 0, 48, s));
        BCHK(st.ensure(tb + 64));
        BCHK(hipcub::DeviceRadixSort::SortPairs(st.p, tb, key.as<unsigned long long>(), skey.as<unsigned long long>(), idx.as<uint32_t>(), sidx.as<uint32_t>(), (int)R, 0, 48, s));
        st.release(); key.release(); idx.release();
        hipLaunchKernelGGL(k_bai_merge, dim3(rb), dim3(256), 0, s, (const unsigned long long *)skey.p, (const uint32_t *)sidx.p, (const uint64_t *)beg.p, (const uint64_t *)end.p, (int64_t)R, head.as<uint8_t>());
        BCHK(mh.ensure(R * 4 + 64));
        BCHK(dev_select_flagged(head.as<uint8_t>(), R, mh.as<uint32_t>(), dm + 3, b->tmp, s));
        unsigned long long M = 0;
        BCHK(hipMemcpyAsync(&M, dm + 3, 8, hipMemcpyDeviceToHost, s)); BCHK(hipStreamSynchronize(s));
        BCHK(out.ensure(M * 24 + 64));
        hipLaunchKernelGGL(k_bai_chunks, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, (const unsigned long long *)skey.p, (const uint32_t *)sidx.p, (const uint64_t *)beg.p, (const uint64_t *)end.p,
                           (int64_t)R, (const uint32_t *)mh.p, (const unsigned long long *)(dm + 3), out.as<uint64_t>());
        b->chunks.resize(M * 3);
        BCHK(hipMemcpyAsync(b->chunks.data(), out.p, M * 24, hipMemcpyDeviceToHost, s)); BCHK(hipStreamSynchronize(s)); BCHK(hipGetLastError());
        counts[3] = (int64_t)M;
    }
    sel.release();
    // ---- the linear index
    {
        ScopedBuf nintv, loff, lin, lin2, st;
        BCHK(nintv.ensure(nr1 * 4)); BCHK(hipMemsetAsync(nintv.p, 0, nr1 * 4, s));
        hipLaunchKernelGGL(k_bai_nintv, dim3(nb), dim3(256), 0, s, f, (const uint8_t *)mapped.p, n_c, nintv.as<uint32_t>());
        std::vector<uint32_t> ni(nr1, 0);
        BCHK(hipMemcpyAsync(ni.data(), nintv.p, nr1 * 4, hipMemcpyDeviceToHost, s)); BCHK(hipStreamSynchronize(s));
        for (int32_t t = 0; t < n_ref; t++) b->loff[t + 1] = b->loff[t] + ni[t];
        const uint64_t W = b->loff[n_ref];
        if (W) {
            BCHK(loff.ensure(((size_t)n_ref + 1) * 8)); BCHK(lin.ensure(W * 8 + 64));
            BCHK(hipMemcpyAsync(loff.p, b->loff.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, s));
            BCHK(hipMemsetAsync(lin.p, 0xFF, W * 8, s));
            hipLaunchKernelGGL(k_bai_lin_min, dim3(nb), dim3(256), 0, s, f, (const uint8_t *)mapped.p, n_c, (const uint64_t *)loff.p, lin.as<unsigned long long>());
            hipLaunchKernelGGL(k_bai_lin_fill, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, s, (const uint64_t *)loff.p, n_ref, (const uint32_t *)cfirst.p, f, lin.as<unsigned long long>());
            size_t tb = 0;
            BCHK(lin2.ensure(W * 8 + 64));
            BCHK(hipcub::DeviceScan::InclusiveScan(nullptr, tb, lin.as<unsigned long long>(), lin2.as<unsigned long long>(), hipcub::Max(), (int)W, s));
            BCHK(st.ensure(tb + 64));
            BCHK(hipcub::DeviceScan::InclusiveScan(st.p, tb, lin.as<unsigned long long>(), lin2.as<unsigned long long>(), hipcub::Max(), (int)W, s));
            b->lin.resize(W);
            BCHK(hipMemcpyAsync(b->lin.data(), lin2.p, W * 8, hipMemcpyDeviceToHost, s)); BCHK(hipStreamSynchronize(s)); BCHK(hipGetLastError());
        }
        counts[4] = (int64_t)W;
    }
    // distinct (tid, bin) of the merged chunks
    int64_t nbins = 0;
    for (size_t m = 0; m < b->chunks.size() / 3; m++) nbins += m == 0 || b->chunks[3 * m] != b->chunks[3 * (m - 1)];
    counts[2] = nbins;
    return GCE_OK;
}

// SAMv1 5.2: magic, n_ref, per contig its bins in ascending order (the pseudo-bin 37450 last, for a contig with records) and its linear index,
// n_no_coor.  *out: malloc'd (free())
int gce_bai_serialise(gce_bai *b, int32_t n_ref, uint8_t **out, size_t *out_bytes) {
    if (!b || !out || !out_bytes || (int64_t)b->meta.size() != 4 * (int64_t)n_ref) return GCE_ERR_INVALID;
    std::vector<uint8_t> o;
    o.reserve(16 + (size_t)n_ref * 8 + b->chunks.size() * 8 + b->lin.size() * 8 + (size_t)n_ref * 48);
    auto put = [&](const void *p, size_t k) { o.insert(o.end(), (const uint8_t *)p, (const uint8_t *)p + k); };
    auto u32 = [&](uint32_t v) { put(&v, 4); };
    auto u64 = [&](uint64_t v) { put(&v, 8); };
    put("BAI\1", 4); u32((uint32_t)n_ref);
    const size_t M = b->chunks.size() / 3;
    size_t m = 0;
    for (int32_t t = 0; t < n_ref; t++) {
        const size_t m0 = m;
        while (m < M && (b->chunks[3 * m] >> 16) == (uint64_t)t) m++;
        const bool has = b->meta[4 * t + 2] + b->meta[4 * t + 3] > 0;
        uint32_t nbin = has ? 1u : 0u;
        for (size_t q = m0; q < m; q++) nbin += q == m0 || b->chunks[3 * q] != b->chunks[3 * (q - 1)];
        u32(nbin);
        for (size_t q = m0; q < m; ) {
            size_t q1 = q;
            while (q1 < m && b->chunks[3 * q1] == b->chunks[3 * q]) q1++;
            u32((uint32_t)(b->chunks[3 * q] & 0xFFFFu)); u32((uint32_t)(q1 - q));
            for (size_t x = q; x < q1; x++) { u64(b->chunks[3 * x + 1]); u64(b->chunks[3 * x + 2]); }
            q = q1;
        }
        if (has) { u32(37450u); u32(2u); for (int k = 0; k < 4; k++) u64(b->meta[4 * t + k]); }
        const uint64_t a = b->lin.empty() ? 0 : b->loff[t], z = b->lin.empty() ? 0 : b->loff[t + 1];
        u32((uint32_t)(z - a));
        for (uint64_t x = a; x < z; x++) u64(b->lin[x]);
    }
    u64((uint64_t)b->n_no_coor);
    *out = (uint8_t *)malloc(o.size());
    if (!*out) return GCE_ERR_OOM;
    memcpy(*out, o.data(), o.size()); *out_bytes = o.size();
    return GCE_OK;
}

}  // extern "C"
