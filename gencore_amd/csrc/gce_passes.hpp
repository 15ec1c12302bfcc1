// gce_passes.hpp — one file in key-range passes on ONE engine (gce_run_bam_passes): device memory bounded by the largest pass,
// not by the file.  Pass k of P is shard k of a P-way key-range plan (gce_plan_shards mode 2); the file is streamed once for the plan (the
// key pass) and once per pass, window by window, and only what a window contributes stays resident:
//   key pass   per read: the cluster key and a weight (12 bytes, kept until the plan is made); per window: the global tick carried as a scalar,
//              the flush events, the --quit_after_contig cut, the first unmapped read
//   pass k     per window: the records of range k (and, in pass 0, the cut read) appended to the engine's raw stream with their global ticks
//              and places in the whole stream; the smallest (tid, pos) of any read of a later range (the watermark W_k)
// A window arrives as whole BGZF members of the file, is inflated by the GPU behind the record the last window's end cut and indexed by the
// record index of gce_devstream.hpp (dev_record_index, with a soft end: the record the window's end cuts is carried over in HBM to the next window).  The
// per-read decisions reuse the planner's kernels (k_plan_keys, k_plan_range) and the cut of gce_process (k_first_contig_ge): every pass sees
// the same key, tick and event as the whole stream does.
#pragma once

namespace {

// the key record of every record of the window (k_raw_fill's first half, without the per-read blobs)
__global__ __launch_bounds__(256) void k_pass_core(const uint8_t *u, const uint64_t *off, int64_t n, gce_core *core) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *r = u + off[i] + 4;
    union { gce_core c; uint32_t w[8]; uint4 q[2]; } t;
#pragma unroll
    for (int k = 0; k < 8; k++) t.w[k] = rb32(r + 4 * k);
    reinterpret_cast<uint4 *>(core + i)[0] = t.q[0]; reinterpret_cast<uint4 *>(core + i)[1] = t.q[1];
}
// global tick of every read (clustered flag -> carry + inclusive count; the exclusive sum of the flags is in xs[0 .. n]); the weight of the
// read's record; flush events (tick % period == 0 on a clustered read in front of the first unmapped read, gencore.cpp:319-322: k_plan_events)
__global__ __launch_bounds__(256) void k_pass_tick(const uint8_t *u, const uint64_t *off, int64_t n, unsigned long long *cls_tick, const uint64_t *xs, unsigned long long carry,
                                                   unsigned long long period, unsigned int front, uint8_t *ev_flag, uint32_t *weight, int *bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool cm = cls_tick[i] != 0;
    const unsigned long long t = carry + xs[i + 1];
    cls_tick[i] = t;
    if (ev_flag) ev_flag[i] = cm && (unsigned int)i < front && t % period == 0;
    if (bad && cm && (unsigned int)i >= front) *bad = 1;
    if (weight) weight[i] = plan_weight(4ull + rb32(u + off[i]));
}
__global__ __launch_bounds__(256) void k_pass_event_pos(const gce_core *core, const uint32_t *idx, const unsigned long long *n_ev, int32_t *tid, int32_t *pos) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < *n_ev) { tid[j] = core[idx[j]].tid; pos[j] = core[idx[j]].pos; }
}
// (tid, pos) as one signed word in bamComp's order of the two fields
__device__ __forceinline__ long long pass_tidpos(int32_t tid, int32_t pos) { return (long long)(((unsigned long long)(long long)tid << 32) | (unsigned long long)((uint32_t)pos ^ 0x80000000u)) ; }
// pass k: the reads of range k (k_plan_range's rule) and, in pass 0, the cut read at n_eff; the watermark over the reads of later ranges
// that can emit a record: an unmapped read (tid < 0 or pos < 0) is never written (gencore.cpp:254-265), so it does not hold anything back
__global__ __launch_bounds__(256) void k_pass_flag(const gce_core *core, const unsigned long long *key, int64_t n_eff, int64_t n_cut, PlanCuts cuts, int32_t k, uint8_t *flag, long long *wm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cut) return;
    if (i >= n_eff) { flag[i] = k == 0; return; }
    int s = 0;
    for (int q = 0; q < cuts.n; q++) s += cuts.c[q] <= key[i];
    flag[i] = s == k;
    if (s > k && core[i].tid >= 0 && core[i].pos >= 0) { const long long v = pass_tidpos(core[i].tid, core[i].pos); if (v < *(volatile long long *)wm) atomicMin(wm, v); }
}
__global__ __launch_bounds__(256) void k_pass_size(const uint8_t *u, const uint64_t *off, const uint32_t *sel, const unsigned long long *m, uint64_t *size) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < *m) size[j] = 4ull + rb32(u + off[sel[j]]);
}
// 16 lanes per selected record: its bytes behind the raw stream, its global tick (0 for the cut read: gce_process drops it) and place
__global__ __launch_bounds__(256) void k_pass_append(const uint8_t *u, const uint64_t *off, const uint32_t *sel, const unsigned long long *m, const uint64_t *dst, uint8_t *raw,
                                                     const unsigned long long *tick, int64_t n_eff, uint64_t gbase, uint64_t *tick_out, uint32_t *gidx_out) {
    const int sub = threadIdx.x & 15;
    const uint64_t mm = *m;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < mm; j += ((uint64_t)gridDim.x * blockDim.x) >> 4) {
        const uint32_t r = sel[j];
        const uint8_t *s = u + off[r]; uint8_t *d = raw + dst[j]; const uint32_t sz = 4u + rb32(s);
        for (uint32_t q = 4 * sub; q < sz; q += 64) {
            if (q + 4 <= sz) *(rb_u32u *)(d + q) = rb32(s + q);
            else for (uint32_t b = q; b < sz; b++) d[b] = s[b];
        }
        if (sub == 0) { tick_out[j] = (int64_t)r < n_eff ? tick[r] : 0ull; gidx_out[j] = (uint32_t)(gbase + r); }
    }
}
__global__ void k_pass_range_w(const unsigned long long *key, const uint32_t *w, int64_t n, PlanCuts cuts, unsigned long long *sum) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int s = 0;
    for (int q = 0; q < cuts.n; q++) s += cuts.c[q] <= key[i];
    atomicAdd(sum + s, (unsigned long long)w[i]);
}

// a device buffer that keeps its first `used` bytes when it grows: half as much again as is needed (and DevBuf's eighth)
static hipError_t pass_grow(DevBuf &b, size_t need, size_t used, hipStream_t s) { return dev_grow_keep(b, need, used, DevBuf::padded(need + need / 2), s); }

// one window of a BGZF file on the GPU, shared by the pass runner (gce_passes_window), the BAI indexer (gce_bai.hpp) and the sort (gce_sort.hpp):
// whole BGZF members in host memory are copied to HBM and inflated (dev_inflate_members, as gce_raw_push_bgzf) behind the record the last
// window's end cut; the records of [skip, total) are indexed by dev_record_index with a soft end: the record the window's end cuts is left
// for win_carry to move to the front.  win holds the inflated bytes, idx.off the n_rec record starts.
struct WinIdx {
    DevBuf win, zc, zdir, zerr, ctmp; RecIdx idx; uint64_t carry_n = 0;
    void release() { for (DevBuf *b : {&win, &zc, &zdir, &zerr, &ctmp}) b->release(); idx.release(); carry_n = 0; }
    uint64_t held() const { uint64_t a = 0; for (const DevBuf *b : {&win, &zc, &zdir, &zerr, &ctmp, &idx.guess, &idx.leave, &idx.cnt, &idx.base, &idx.bad_of, &idx.misc, &idx.off}) a += b->cap; return a; }
};
// the device bytes the next window takes beyond what w holds: its inflated bytes (u_all of them, the carried ones included) as pass_grow makes
// the buffer (3/2 x 9/8 = 27/16) and its compressed bytes as DevBuf::ensure does (9/8), each only where the buffer has to grow
static uint64_t win_room(const WinIdx &w, uint64_t comp_bytes, uint64_t u_all) {
    uint64_t add = 0;
    if (u_all + 64 > w.win.cap) add += (u_all + 64) * 27 / 16 + 256;
    if (comp_bytes + 64 > w.zc.cap) add += (comp_bytes + 64) * 9 / 8 + 256;
    return add;
}
// -> *total (inflated bytes in w.win, the carried ones included), *n_rec, *end (where the window's last whole record ends).  ctr: the four index
// counters to add to (gce_get_index_counters) or NULL.  last: the final piece of the file (a record cut there is a truncated stream).
static int win_inflate_index(WinIdx &w, DevBuf &tmp, hipStream_t s, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize,
                             const uint32_t *usize, uint64_t skip, int32_t n_ref, int32_t last, int64_t *ctr, uint64_t *total_out, uint64_t *n_rec_out, uint64_t *end_out, std::string &msg) {
    std::vector<InfDir> dir; uint64_t total = w.carry_n;
    for (int32_t k = 0; k < n_members; k++) {
        if (coff[k] > comp_bytes || csize[k] > comp_bytes - coff[k] || usize[k] > 0x10000u) { msg = "BGZF member outside its buffer"; return GCE_ERR_INVALID; }
        if (usize[k] == 0) continue;
        InfDir d; d.coff = coff[k]; d.uoff = total; d.csize = csize[k]; d.usize = usize[k]; dir.push_back(d); total += usize[k];
    }
    if (w.carry_n && skip) return GCE_ERR_INVALID;
    MCHK(pass_grow(w.win, (size_t)total + 64, (size_t)w.carry_n, s));
    if (!dir.empty()) {
        MCHK(w.zc.ensure(comp_bytes + 64)); MCHK(w.zdir.ensure(dir.size() * (sizeof(InfDir) + INF_NSYM) + 64));   // (a window's directory scratch has 64 spare bytes)
        MCHK(hipMemcpyAsync(w.zc.p, comp, comp_bytes, hipMemcpyHostToDevice, s));
        int64_t bad = -1;
        const int rc = dev_inflate_members(w.zc.as<uint8_t>(), comp_bytes, dir.data(), dir.size(), w.win.as<uint8_t>(), w.zdir, w.zerr, s, &bad, msg);
        if (rc != GCE_OK) return rc;
        if (bad >= 0) { char m2[96]; snprintf(m2, sizeof m2, "inflate / CRC failure in BGZF member %u of a window", (uint32_t)bad); msg = m2; return GCE_ERR_INVALID; }
    }
    MCHK(hipMemsetAsync(w.win.as<uint8_t>() + total, 0, 64, s));
    const uint64_t start = std::min<uint64_t>(skip, total);
    uint64_t n_rec = 0, end = start;
    if (total > start) {                                                             // ---- the record index of [start, total), soft end
        int64_t c[4];
        const int rc = dev_record_index<true>(w.idx, tmp, s, w.win.as<uint8_t>(), start, total, n_ref, c, &n_rec, &end, msg);
        if (ctr) for (int k = 0; k < 4; k++) __atomic_add_fetch(&ctr[k], c[k], __ATOMIC_RELAXED);
        if (rc != GCE_OK) return rc;
        MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    }
    if (last && end != total) { msg = "truncated record at the end of the BAM stream"; return GCE_ERR_INVALID; }
    *total_out = total; *n_rec_out = n_rec; *end_out = end;
    return GCE_OK;
}
// the record the window's end cut ([end, total) of w.win) to the front, for the next window
static int win_carry(WinIdx &w, hipStream_t s, uint64_t total, uint64_t end, std::string &msg) {
    w.carry_n = total - end;
    if (w.carry_n) {
        MCHK(w.ctmp.ensure(w.carry_n + 64));
        MCHK(hipMemcpyAsync(w.ctmp.p, w.win.as<uint8_t>() + end, w.carry_n, hipMemcpyDeviceToDevice, s));
        MCHK(hipMemcpyAsync(w.win.p, w.ctmp.p, w.carry_n, hipMemcpyDeviceToDevice, s));
        MCHK(hipStreamSynchronize(s));
    }
    return GCE_OK;
}

}  // namespace

struct gce_passes {
    int32_t device = 0, max_contig = 0; unsigned long long period = 10000;
    hipStream_t s = nullptr;
    std::string err;
    // the window
    DevBuf core, key, tick, xs, flag, sel, size, dst, misc, tmp, ev_tid, ev_pos;
    WinIdx w;                                                                        // GPU inflate + record index of the window
    // the stream so far: records seen, global tick, cut, first unmapped read
    uint64_t gbase = 0; unsigned long long carry = 0; int64_t cut = -1; bool unmapped_seen = false, bad = false;
    // key pass: key + weight of every read in front of the cut; the flush events
    DevBuf key_all, w_all; int64_t n_all = 0;
    std::vector<int32_t> ev_t, ev_p;
    // the plan
    PlanCuts cuts{}; int32_t P = 1; std::vector<unsigned long long> range_w;
    // the current pass
    int32_t k = -1; DevBuf ptick, pgidx; int64_t pm = 0; long long wm = 0;
};

static int pfail(gce_passes *p, int code, const std::string &m) { if (p) p->err = m; return code; }
#define PCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) return pfail(p, _e == hipErrorOutOfMemory ? GCE_ERR_OOM : GCE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); } while (0)

extern "C" {

// live / peak device bytes of the process (every DevBuf and planner buffer); reset_peak: the peak restarts at the live count
int gce_device_bytes(int64_t *live, int64_t *peak, int32_t reset_peak) {
    if (reset_peak) __atomic_store_n(&g_dev_peak, __atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), __ATOMIC_RELAXED);
    if (live) *live = __atomic_load_n(&g_dev_live, __ATOMIC_RELAXED);
    if (peak) *peak = __atomic_load_n(&g_dev_peak, __ATOMIC_RELAXED);
    return GCE_OK;
}

int gce_passes_create(int32_t device, int32_t max_contig, int32_t flush_period, gce_passes **out) {
    if (!out) return GCE_ERR_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    gce_passes *p = new gce_passes();
    for (int64_t &c : g_pass_idx_ctr) __atomic_store_n(&c, (int64_t)0, __ATOMIC_RELAXED);
    p->device = device; p->max_contig = max_contig; p->period = (unsigned long long)(flush_period > 0 ? flush_period : 10000);
    if (hipStreamCreate(&p->s) != hipSuccess) { delete p; return GCE_ERR_HIP; }
    *out = p;
    return GCE_OK;
}
void gce_passes_destroy(gce_passes *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->s);
    p->w.release();
    for (DevBuf *b : {&p->core, &p->key, &p->tick, &p->xs, &p->flag, &p->sel, &p->size, &p->dst, &p->misc, &p->tmp, &p->ev_tid, &p->ev_pos, &p->key_all, &p->w_all, &p->ptick, &p->pgidx}) b->release();
    (void)hipStreamDestroy(p->s);
    delete p;
}
const char *gce_passes_error(gce_passes *p) { return p ? p->err.c_str() : ""; }
int gce_device_mem_info(int32_t device, size_t *free_bytes, size_t *total_bytes) {
    if (!free_bytes || !total_bytes || hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    return hipMemGetInfo(free_bytes, total_bytes) == hipSuccess ? GCE_OK : GCE_ERR_HIP;
}

// the records of the window (n, at p->w.idx.off in p->w.win, on the device): e == NULL: the key pass; otherwise pass p->k, whose records go to e's raw
// stream.  *cut_reached: the --quit_after_contig cut lies in this window (nothing behind it exists: the caller stops reading).
static int pass_records(gce_passes *p, gce_engine *e, int64_t n, int32_t *cut_reached) {
    *cut_reached = 0;
    if (p->cut >= 0) { *cut_reached = 1; return GCE_OK; }
    if (n == 0) return GCE_OK;
    if (p->gbase + (uint64_t)n >= 0x7FFFFFF0ull) return pfail(p, GCE_ERR_INVALID, "more than 2^31 records in one stream");
    hipStream_t s = p->s;
    const size_t n1 = (size_t)n;
    PCHK(p->core.ensure(n1 * sizeof(gce_core) + 64)); PCHK(p->key.ensure(n1 * 8)); PCHK(p->tick.ensure(n1 * 8 + 8));
    PCHK(p->xs.ensure(n1 * 8 + 16)); PCHK(p->flag.ensure(n1 + 64)); PCHK(p->sel.ensure(n1 * 4 + 64)); PCHK(p->misc.ensure(64));
    const uint8_t *u = p->w.win.as<uint8_t>(); const uint64_t *off = p->w.idx.off.as<uint64_t>();
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_pass_core, dim3(nb), dim3(256), 0, s, u, off, n, p->core.as<gce_core>());
    // misc: [0] the first read of contig >= max_contig, [1] the first unmapped read, [2] bad, [4..5] a count (uint64)
    unsigned int init[4] = {NONE32, NONE32, 0u, 0u};
    PCHK(hipMemcpyAsync(p->misc.p, init, sizeof init, hipMemcpyHostToDevice, s));
    if (p->max_contig > 0) hipLaunchKernelGGL(k_first_contig_ge, dim3(nb), dim3(256), 0, s, (const gce_core *)p->core.p, n, p->max_contig, p->misc.as<unsigned int>());
    unsigned int first = NONE32;
    PCHK(hipMemcpyAsync(&first, p->misc.p, 4, hipMemcpyDeviceToHost, s)); PCHK(hipStreamSynchronize(s));
    const int64_t n_eff = first != NONE32 ? (int64_t)first : n;                     // reads in front of the cut
    const int64_t n_cut = first != NONE32 ? n_eff + 1 : n;                          // ... and the cut read
    if (n_eff > 0) {
        const unsigned ne = (unsigned)((n_eff + 255) / 256);
        hipLaunchKernelGGL(k_plan_keys, dim3(ne), dim3(256), 0, s, (const gce_core *)p->core.p, n_eff, p->tick.as<unsigned long long>(), p->key.as<unsigned long long>(), p->misc.as<unsigned int>() + 1);
        PCHK(dev_exclusive_sum(p->tick.as<unsigned long long>(), (uint64_t)n_eff, p->xs.as<uint64_t>(), p->tmp, s));
    }
    if (!e) {                                                                        // ---- key pass
        unsigned int front = NONE32;
        if (n_eff > 0) {
            if (!p->unmapped_seen) { PCHK(hipMemcpyAsync(&front, p->misc.as<unsigned int>() + 1, 4, hipMemcpyDeviceToHost, s)); PCHK(hipStreamSynchronize(s)); } else front = 0;
            PCHK(pass_grow(p->key_all, (size_t)(p->n_all + n_eff) * 8, (size_t)p->n_all * 8, s)); PCHK(pass_grow(p->w_all, (size_t)(p->n_all + n_eff) * 4, (size_t)p->n_all * 4, s));
            const unsigned ne = (unsigned)((n_eff + 255) / 256);
            hipLaunchKernelGGL(k_pass_tick, dim3(ne), dim3(256), 0, s, u, off, n_eff, p->tick.as<unsigned long long>(), (const uint64_t *)p->xs.p, p->carry, p->period, front, p->flag.as<uint8_t>(),
                               p->w_all.as<uint32_t>() + p->n_all, p->misc.as<int>() + 2);
            PCHK(hipMemcpyAsync(p->key_all.as<unsigned long long>() + p->n_all, p->key.p, (size_t)n_eff * 8, hipMemcpyDeviceToDevice, s));
            PCHK(dev_select_flagged(p->flag.as<uint8_t>(), (uint64_t)n_eff, p->sel.as<uint32_t>(), (unsigned long long *)(p->misc.as<unsigned int>() + 4), p->tmp, s));
            PCHK(p->ev_tid.ensure(n1 * 4)); PCHK(p->ev_pos.ensure(n1 * 4));
            hipLaunchKernelGGL(k_pass_event_pos, dim3(ne), dim3(256), 0, s, (const gce_core *)p->core.p, (const uint32_t *)p->sel.p, (const unsigned long long *)(p->misc.as<unsigned int>() + 4), p->ev_tid.as<int32_t>(), p->ev_pos.as<int32_t>());
            struct { unsigned int c0, fu, bad, pad; unsigned long long nev; } h;
            PCHK(hipMemcpyAsync(&h, p->misc.p, sizeof h, hipMemcpyDeviceToHost, s));
            unsigned long long last = 0;
            PCHK(hipMemcpyAsync(&last, p->xs.as<uint64_t>() + n_eff, 8, hipMemcpyDeviceToHost, s)); PCHK(hipStreamSynchronize(s));
            if (h.nev) {
                const size_t a = p->ev_t.size();
                p->ev_t.resize(a + h.nev); p->ev_p.resize(a + h.nev);
                PCHK(hipMemcpyAsync(p->ev_t.data() + a, p->ev_tid.p, h.nev * 4, hipMemcpyDeviceToHost, s)); PCHK(hipMemcpyAsync(p->ev_p.data() + a, p->ev_pos.p, h.nev * 4, hipMemcpyDeviceToHost, s));
            }
            if (h.bad) p->bad = true;
            if (h.fu != NONE32) p->unmapped_seen = true;
            p->carry += last; p->n_all += n_eff;
        }
    } else {                                                                         // ---- pass k
        if (n_eff > 0) {
            const unsigned ne = (unsigned)((n_eff + 255) / 256);
            hipLaunchKernelGGL(k_pass_tick, dim3(ne), dim3(256), 0, s, u, off, n_eff, p->tick.as<unsigned long long>(), (const uint64_t *)p->xs.p, p->carry, p->period, NONE32, (uint8_t *)nullptr, (uint32_t *)nullptr, (int *)nullptr);
        }
        long long *dwm = (long long *)(p->misc.as<unsigned int>() + 6);                     // (behind the count: one copy fetches both)
        PCHK(hipMemcpyAsync(dwm, &p->wm, 8, hipMemcpyHostToDevice, s));
        const int64_t n_look = p->k == 0 ? n_cut : n_eff;                            // (pass 0 also looks at the cut read)
        if (n_look > 0) hipLaunchKernelGGL(k_pass_flag, dim3((unsigned)((n_look + 255) / 256)), dim3(256), 0, s, (const gce_core *)p->core.p, (const unsigned long long *)p->key.p, n_eff, n_look, p->cuts, p->k, p->flag.as<uint8_t>(), dwm);
        unsigned long long *dm = (unsigned long long *)(p->misc.as<unsigned int>() + 4);
        PCHK(dev_select_flagged(p->flag.as<uint8_t>(), (uint64_t)n_look, p->sel.as<uint32_t>(), dm, p->tmp, s));
        struct { unsigned long long m; long long wm; } h;
        PCHK(hipMemcpyAsync(&h, dm, sizeof h, hipMemcpyDeviceToHost, s));
        unsigned long long last = 0;
        if (n_eff > 0) PCHK(hipMemcpyAsync(&last, p->xs.as<uint64_t>() + n_eff, 8, hipMemcpyDeviceToHost, s));
        PCHK(hipStreamSynchronize(s));
        p->wm = h.wm;
        if (h.m) {
            PCHK(p->size.ensure(h.m * 8 + 8)); PCHK(p->dst.ensure(h.m * 8 + 16));
            hipLaunchKernelGGL(k_pass_size, dim3((unsigned)((h.m + 255) / 256)), dim3(256), 0, s, u, off, (const uint32_t *)p->sel.p, (const unsigned long long *)dm, p->size.as<uint64_t>());
            PCHK(dev_exclusive_sum(p->size.as<uint64_t>(), h.m, p->dst.as<uint64_t>(), p->tmp, s));
            uint64_t add = 0;
            PCHK(hipMemcpyAsync(&add, p->dst.as<uint64_t>() + h.m, 8, hipMemcpyDeviceToHost, s)); PCHK(hipStreamSynchronize(s));
            {   // the engine's raw stream grows behind what it holds (the header + the records of earlier windows)
                const hipError_t g = pass_grow(e->raw, e->raw_n + add + 256, e->raw_n, s);
                if (g != hipSuccess) return pfail(p, g == hipErrorOutOfMemory ? GCE_ERR_OOM : GCE_ERR_HIP, "out of device memory (raw stream of a pass)");
            }
            PCHK(pass_grow(p->ptick, (size_t)(p->pm + h.m) * 8 + 64, (size_t)p->pm * 8, s)); PCHK(pass_grow(p->pgidx, (size_t)(p->pm + h.m) * 4 + 64, (size_t)p->pm * 4, s));
            hipLaunchKernelGGL(k_pass_append, dim3((unsigned)std::min<uint64_t>((h.m + 15) / 16, 65535u)), dim3(256), 0, s, u, off, (const uint32_t *)p->sel.p, (const unsigned long long *)dm, (const uint64_t *)p->dst.p,
                               e->raw.as<uint8_t>() + e->raw_n, (const unsigned long long *)p->tick.p, n_eff, p->gbase, p->ptick.as<uint64_t>() + p->pm, p->pgidx.as<uint32_t>() + p->pm);
            PCHK(hipStreamSynchronize(s));
            e->raw_n += add; p->pm += (int64_t)h.m;
        }
        p->carry += last;
    }
    PCHK(hipGetLastError());
    if (first != NONE32) { p->cut = (int64_t)p->gbase + (int64_t)first; *cut_reached = 1; }
    p->gbase += (uint64_t)n;
    return GCE_OK;
}

// the next piece of the file: `n_members` whole BGZF members in host memory (member k at comp + coff[k], csize[k] bytes, ISIZE usize[k]).  They
// are copied to HBM and inflated by the GPU (dev_inflate_members, as gce_raw_push_bgzf) behind the record the last window's end cut; the first
// `skip` inflated bytes (the BAM header) are passed over; the records are indexed from the carried offset (dev_record_index of
// gce_devstream.hpp with a soft end: the record the window's end cuts is carried over to the next window) and
// go to pass_records.  last: the final piece of the file (a record cut there is a truncated stream).
int gce_passes_window(gce_passes *p, gce_engine *e, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize,
                      uint64_t skip, int32_t n_ref, int32_t last, int32_t *cut_reached) {
    if (!p || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize)) || !cut_reached) return GCE_ERR_INVALID;
    *cut_reached = 0;
    if (p->cut >= 0) { *cut_reached = 1; return GCE_OK; }
    (void)hipSetDevice(p->device);
    uint64_t total = 0, n_rec = 0, end = 0;
    int rc = win_inflate_index(p->w, p->tmp, p->s, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, g_pass_idx_ctr, &total, &n_rec, &end, p->err);
    if (rc != GCE_OK) return rc;
    if ((rc = pass_records(p, e, (int64_t)n_rec, cut_reached)) != GCE_OK) return rc;
    if (*cut_reached) { p->w.carry_n = total - end; return GCE_OK; }              // ---- the record the window's end cut, to the front
    return win_carry(p->w, p->s, total, end, p->err);
}

// after the key pass: the plan.  budget == 0: exactly min_passes passes; otherwise P >= min_passes passes whose weight fits what the budget
// leaves beside the device bytes live now without the key pass's state, less `reserve` (*per_pass).  GCE_ERR_OOM, with the bytes or the key
// in the message, when nothing is left or one cluster key outweighs a pass.  The key pass's per-read state is freed.
int gce_passes_plan(gce_passes *p, int32_t min_passes, uint64_t budget, uint64_t reserve, int32_t *P_out, uint64_t *total_w, uint64_t *per_pass, uint64_t *fixed_out) {
    if (!p || min_passes < 1 || min_passes > 64 || !P_out) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    if (p->bad) return pfail(p, GCE_ERR_INVALID, "not processable in passes: a mapped read follows the first unmapped read");
    PCHK(hipStreamSynchronize(p->s));
    const long long fixed = __atomic_load_n(&g_dev_live, __ATOMIC_RELAXED) - (long long)p->key_all.cap - (long long)p->w_all.cap;
    if (fixed_out) *fixed_out = (uint64_t)fixed;
    PlanWeighted pw;
    int rc = plan_weighted_cuts(p->key_all.as<unsigned long long>(), p->w_all.as<uint32_t>(), p->n_all, 1, &pw);
    if (rc != GCE_OK) return pfail(p, rc, "planner");
    int32_t P = min_passes; uint64_t room = 0;
    if (total_w) *total_w = pw.total;
    if (budget > 0) {
        if ((long long)budget <= fixed + (long long)reserve) {
            char m[200]; snprintf(m, sizeof m, "device budget of %llu bytes below the fixed part of a pass: %lld bytes needed", (unsigned long long)budget, fixed + (long long)reserve + 1);
            return pfail(p, GCE_ERR_OOM, m);
        }
        room = budget - (uint64_t)fixed - reserve;
        if (pw.heavy_w > room) {
            char m[200]; snprintf(m, sizeof m, "cluster key (tid %lld, pos %lld) needs %llu device bytes in one pass, %llu are left in the budget",
                                  (long long)(pw.heavy_key >> 32), (long long)(pw.heavy_key & 0xFFFFFFFFull), pw.heavy_w, (unsigned long long)room);
            return pfail(p, GCE_ERR_OOM, m);
        }
        const uint64_t q = (pw.total + room - 1) / room;
        if ((uint64_t)P < q) P = (int32_t)std::min<uint64_t>(q, 65);
    }
    if (per_pass) *per_pass = room;
    *P_out = P;
    if (P > 64) return pfail(p, GCE_ERR_OOM, "the budget needs more than 64 passes");
    if (P > 1 && (rc = plan_weighted_cuts(p->key_all.as<unsigned long long>(), p->w_all.as<uint32_t>(), p->n_all, P, &pw)) != GCE_OK) return pfail(p, rc, "planner");
    p->P = P; p->cuts = pw.cuts; p->cuts.n = P - 1;
    p->range_w.assign((size_t)P, 0ull);
    if (p->n_all > 0) {
        PCHK(p->misc.ensure(64 * 8 + 64)); PCHK(hipMemsetAsync(p->misc.p, 0, 64 * 8, p->s));
        hipLaunchKernelGGL(k_pass_range_w, dim3((unsigned)((p->n_all + 255) / 256)), dim3(256), 0, p->s, (const unsigned long long *)p->key_all.p, (const uint32_t *)p->w_all.p, p->n_all, p->cuts, p->misc.as<unsigned long long>());
        PCHK(hipMemcpyAsync(p->range_w.data(), p->misc.p, (size_t)P * 8, hipMemcpyDeviceToHost, p->s)); PCHK(hipStreamSynchronize(p->s));
    }
    p->key_all.release(); p->w_all.release();
    return GCE_OK;
}
// the weight of pass k; the cuts (P - 1 keys) and flush events of the plan (host copies; valid until gce_passes_destroy)
int gce_passes_info(gce_passes *p, int32_t k, uint64_t *weight, const uint64_t **cuts, int32_t *n_events, const int32_t **ev_tid, const int32_t **ev_pos) {
    if (!p || k < 0 || k >= p->P) return GCE_ERR_INVALID;
    if (weight) *weight = p->range_w[(size_t)k];
    if (cuts) *cuts = (const uint64_t *)p->cuts.c;
    if (n_events) *n_events = (int32_t)p->ev_t.size();
    if (ev_tid) *ev_tid = p->ev_t.data();
    if (ev_pos) *ev_pos = p->ev_p.data();
    return GCE_OK;
}

// pass k starts on `e` (after gce_raw_begin and the push of the BAM header): the stream is read again from its first record
int gce_passes_begin(gce_passes *p, gce_engine *e, int32_t k) {
    if (!p || !e || !e->raw_mode || k < 0 || k >= p->P) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    if (e->up_stream) PCHK(hipStreamSynchronize(e->up_stream));
    p->k = k; p->pm = 0; p->gbase = 0; p->carry = 0; p->cut = -1; p->wm = 0x7FFFFFFFFFFFFFFFll; p->w.carry_n = 0;
    return GCE_OK;
}
// pass k's windows are in: the engine indexes its part of the stream (gce_raw_finish) and gets the reads' global ticks, the flush events of the
// whole stream and -- in pass 0 -- the cut read as its last read (gce_raw_select_shard's rule for shard 0: gce_process finds it; the other
// passes do not look for a cut).  *watermark_tid / _pos: the smallest (tid, pos) of a read of a later pass (INT32_MAX, INT32_MAX: none).
int gce_passes_end(gce_passes *p, gce_engine *e, uint64_t records_begin, int32_t n_ref, int64_t *n_records, int32_t *watermark_tid, int32_t *watermark_pos) {
    if (!p || !e || p->k < 0 || !n_records) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    PCHK(hipStreamSynchronize(p->s));
    int rc = gce_raw_finish(e, records_begin, n_ref, n_records);
    if (rc != GCE_OK) return pfail(p, rc, gce_last_error(e));
    if (*n_records != p->pm) return pfail(p, GCE_ERR_INVALID, "pass: the engine indexed another number of records than were selected");
    if (p->pm > 0) {
        e->dev_batch.tick = p->ptick.as<uint64_t>(); e->have_tick = true;
        e->shard_cut_done = !(p->k == 0 && p->cut >= 0);
        if ((rc = gce_set_flush_events(e, (int32_t)p->ev_t.size(), p->ev_t.data(), p->ev_p.data())) != GCE_OK) return pfail(p, rc, "flush events");
    }
    if (watermark_tid && watermark_pos) {
        if (p->wm == 0x7FFFFFFFFFFFFFFFll) { *watermark_tid = INT32_MAX; *watermark_pos = INT32_MAX; }
        else { *watermark_tid = (int32_t)(p->wm >> 32); *watermark_pos = (int32_t)((uint32_t)p->wm ^ 0x80000000u); }
    }
    return GCE_OK;
}
// after gce_raw_build_output of the pass: per output record its merge key (bamComp's fields, place in the whole stream, size: 32 bytes as
// gce_raw_merge_outputs compares them) and the record bytes, to the host
int gce_passes_output(gce_passes *p, gce_engine *e, void *keys_host, void *body_host) {
    if (!p || !e || !e->processed) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    const uint64_t no = (uint64_t)e->n_out;
    if (!no) return GCE_OK;
    if (!keys_host || !body_host) return GCE_ERR_INVALID;
    hipStream_t s = e->stream;
    PCHK(e->sh_keys.ensure(no * sizeof(MergeKey)));
    hipLaunchKernelGGL(k_merge_keys, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, s, e->dev_batch.core, (const uint32_t *)e->o_src.p, (const uint32_t *)p->pgidx.p, (const uint64_t *)e->rw_rsize.p, no, e->sh_keys.as<MergeKey>());
    PCHK(hipMemcpyAsync(keys_host, e->sh_keys.p, no * sizeof(MergeKey), hipMemcpyDeviceToHost, s));
    if (e->raw_body_bytes) PCHK(hipMemcpyAsync(body_host, e->rw_body.p, e->raw_body_bytes, hipMemcpyDeviceToHost, s));
    PCHK(hipStreamSynchronize(s));
    PCHK(hipGetLastError());
    e->sh_keys.release();
    return GCE_OK;
}
// the engine's buffers between passes: everything gce_raw_begin / gce_process sized for this pass goes (the next pass sizes its own)
int gce_passes_release(gce_passes *p, gce_engine *e) {
    if (!p || !e) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(e->stream);
    e->dev_batch = gce_batch{};
    for (DevBuf *b : {&e->b_core, &e->b_qoff, &e->b_qname, &e->b_coff, &e->b_cigar, &e->b_soff, &e->b_seq, &e->b_loff, &e->b_qual, &e->b_nm, &e->b_nmt, &e->b_mioff, &e->b_mi, &e->b_tick,
                      &e->raw, &e->rw.bad_of, &e->rw.guess, &e->rw.leave, &e->rw.cnt, &e->rw.base, &e->rw.off, &e->rw_ncig, &e->rw_nmpos, &e->rw_rsize, &e->rw_roff, &e->rw_body, &e->o_src, &e->o_qsrc, &e->o_nm, &e->o_fr, &e->o_rr})
        b->release();
    p->ptick.release(); p->pgidx.release();
    return gce_reset(e);
}

}  // extern "C"
