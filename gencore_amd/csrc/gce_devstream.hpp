// gce_devstream.hpp — the device side of the file path in one place: the kernels of the BAM record index and the host drivers that turn the
// kernels of the BGZF codec (gce_inflate.hpp, gce_deflate.hpp) and of the index into steps.  Every file runner goes through them: the engine's
// raw stream (gce_bamdev.hpp), the windows of the pass runner, the BAI indexer and the sort (gce_passes.hpp, gce_bai.hpp, gce_sort.hpp).
//   dev_exclusive_sum / dev_select_flagged   prefix sums and compaction on the engine's scan kernels
//   dev_grow_keep                            a device buffer grows and keeps its first bytes
//   dev_record_index<SOFT>                   the record starts of an inflated BAM stream: segment walks, check, repair rounds, scan, offsets
//   dev_inflate_members                      a directory of BGZF members -> their bytes, the first member that failed
//   dev_deflate_members / dev_deflate_pack   bytes -> BGZF members in slots, their packed size; the members back to back
#pragma once

namespace {

typedef uint32_t rb_u32u __attribute__((aligned(1)));
typedef uint16_t rb_u16u __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t rb32(const uint8_t *p) { return *(const rb_u32u *)p; }
__device__ __forceinline__ uint32_t rb16(const uint8_t *p) { return *(const rb_u16u *)p; }
#define RAW_SEG (16u << 10)

// does a record start at o?  (bamio.cpp's test: sane block_size, contig ids inside the header's, a NUL-terminated name, the fixed fields fit)
__device__ __forceinline__ bool raw_plausible(const uint8_t *u, uint64_t o, uint64_t n, int32_t nref) {
    if (o + 36 > n) return false;
    const uint32_t bs = rb32(u + o);
    if (bs < 32 || bs > (1u << 28) || o + 4 + bs > n) return false;
    const uint8_t *r = u + o + 4;
    const int32_t tid = (int32_t)rb32(r), mtid = (int32_t)rb32(r + 20), ls = (int32_t)rb32(r + 16); const uint32_t lq = r[8], nc = rb16(r + 12);
    if (tid < -1 || tid >= nref || mtid < -1 || mtid >= nref || lq == 0 || ls < 0) return false;
    if (32ull + lq + 4ull * nc + (uint64_t)(ls + 1) / 2 + (uint64_t)ls > bs) return false;
    return r[32 + lq - 1] == 0;
}
// records starting in [o, hi): count, optionally their offsets; returns where the chain leaves the range (~0 = broken chain).  SOFT (a window
// of the pass runner, whose end cuts a record): a record that does not fit in n ends the chain there instead of breaking it
template <bool SOFT = false>
__device__ __forceinline__ uint64_t raw_walk(const uint8_t *u, uint64_t o, uint64_t hi, uint64_t n, uint32_t &cnt, uint64_t *out) {
    while (o < hi && o + 4 <= n) {
        const uint32_t bs = rb32(u + o);
        if (bs < 32) return ~0ull;
        if (o + 4 + bs > n) return SOFT ? o : ~0ull;
        if (out) out[cnt] = o;
        cnt++;
        o += 4ull + bs;
    }
    return o;
}
template <bool SOFT = false>
__global__ __launch_bounds__(256) void k_raw_seg(const uint8_t *u, uint64_t first, uint64_t n, int32_t nref, uint64_t nseg, uint64_t *guess, uint64_t *leave, uint32_t *cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const uint64_t lo = first + s * RAW_SEG, hi = min(n, lo + RAW_SEG);
    uint64_t o = lo;
    if (s > 0) {                                                   // a guessed start: two sane records in a row (the first segment starts on the first record)
        while (o < hi && !(raw_plausible(u, o, n, nref) && (o + 4 + rb32(u + o) + 3 >= n || raw_plausible(u, o + 4 + rb32(u + o), n, nref)))) o++;
        if (o >= hi) { guess[s] = ~0ull; leave[s] = ~0ull; cnt[s] = 0; return; }
    }
    uint32_t c = 0;
    guess[s] = o;
    leave[s] = raw_walk<SOFT>(u, o, hi, n, c, nullptr);
    cnt[s] = c;
}
// every segment's guess must be where the chain of the segment in front of it leaves: flag = number of segments for which it is not
template <bool SOFT = false>
__global__ __launch_bounds__(256) void k_raw_check(const uint64_t *guess, const uint64_t *leave, uint64_t nseg, uint64_t n, unsigned int *bad, uint8_t *bad_of) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const bool b = leave[s] == ~0ull || (s > 0 && guess[s] != leave[s - 1]) || (s == nseg - 1 && (SOFT ? leave[s] > n : leave[s] != n));
    bad_of[s] = b;
    if (b) atomicAdd(bad, 1u);
}
// repair, in parallel.  A guess can be a coincidence: one byte in front of a record of contig 0 the shifted fields pass the test about once
// in 4000 segments (block_size x 256 + the last NM byte, tid x 256 = 0 ...), and the chain walked from there leaves far behind the
// segment, which also puts the NEXT segment off the chain although its own guess is right.  Bytes inside a long record (a B:C array of
// record-shaped bytes) can even carry a false chain of their own across several segments, consistent from segment to segment: a segment
// that is NOT flagged may still be wrong, when it agrees with a wrong predecessor.  Every round re-walks the flagged segments whose
// predecessor is not flagged (nothing that predecessor holds changes in the round) from where the predecessor's chain leaves.  That start
// is only right when every segment in front is right, so a walk from it that breaks proves nothing: the segment is left as it is (still
// flagged) and only k_raw_repair, which walks from the first record, may call the stream damaged.  Progress: the first wrong segment is
// always flagged and its predecessor is right and unflagged, so every round puts at least it on the chain; no flag at all means, by
// induction from segment 0 (whose guess is the first record), that every segment is on the chain.  Rounds <= the longest run of wrong
// segments (records longer than a segment, false chains).
template <bool SOFT = false>
__global__ __launch_bounds__(256) void k_raw_fix(const uint8_t *u, uint64_t first, uint64_t n, uint64_t nseg, uint64_t *guess, uint64_t *leave, uint32_t *cnt, const uint8_t *bad_of) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg || s == 0 || !bad_of[s] || bad_of[s - 1]) return;
    const uint64_t at = leave[s - 1];
    if (at == ~0ull) return;
    const uint64_t hi = min(n, first + s * RAW_SEG + RAW_SEG);
    uint32_t c = 0; uint64_t x = at;
    if (at < hi) { x = raw_walk<SOFT>(u, at, hi, n, c, nullptr); if (x == ~0ull) return; }
    guess[s] = at; leave[s] = x; cnt[s] = c;
}
// the last resort (after several parallel rounds): ONE thread follows the chain from segment to segment
// and re-walks only the segments whose guess does not lie on it
template <bool SOFT = false>
__global__ void k_raw_repair(const uint8_t *u, uint64_t first, uint64_t n, uint64_t nseg, uint64_t *guess, uint64_t *leave, uint32_t *cnt, unsigned int *broken) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t at = first;
    for (uint64_t s = 0; s < nseg; s++) {
        const uint64_t lo = first + s * RAW_SEG, hi = min(n, lo + RAW_SEG);
        if (at >= hi) { guess[s] = at; leave[s] = at; cnt[s] = 0; continue; }       // a record spans the whole segment
        if (guess[s] != at || leave[s] == ~0ull) {
            uint32_t c = 0;
            const uint64_t x = raw_walk<SOFT>(u, at, hi, n, c, nullptr);
            if (x == ~0ull) { *broken = 1u; return; }
            guess[s] = at; leave[s] = x; cnt[s] = c;
        }
        at = leave[s];
    }
    if (SOFT ? at > n : at != n) *broken = 1u;
}
template <bool SOFT = false>
__global__ __launch_bounds__(256) void k_raw_offsets(const uint8_t *u, uint64_t first, uint64_t n, uint64_t nseg, const uint64_t *guess, const uint64_t *base, uint64_t *rec_off) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const uint64_t hi = min(n, first + s * RAW_SEG + RAW_SEG);
    uint32_t c = 0;
    (void)raw_walk<SOFT>(u, guess[s], hi, n, c, rec_off + base[s]);
}

}  // namespace


// ---- prefix sums and compaction of the file layer on the engine's own scan kernels (gce_cluster.hpp: tiles of 2048, one block over the tile
//      totals): exclusive sums out[0 .. n] (out[n] = the total) of n 32- or 64-bit values, three launches; flagged indices, three launches
namespace {
template <class T> __global__ __launch_bounds__(256) void k_xs_reduce(const T *in, uint64_t n, uint64_t *part) {
    __shared__ uint64_t s4[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE; uint64_t v = 0;
    for (int k = 0; k < SCAN_TILE / 256; k++) { const uint64_t i = base + k * 256 + threadIdx.x; v += i < n ? (uint64_t)in[i] : 0ull; }
    v = (uint64_t)wave_sum64((long long)v);
    if (lane_id() == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = s4[0] + s4[1] + s4[2] + s4[3];
}
template <class T> __global__ __launch_bounds__(256) void k_xs_apply(const T *in, uint64_t n, const uint64_t *part, uint64_t *out) {
    __shared__ uint64_t s_w[4]; __shared__ uint64_t s_carry;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = part[blockIdx.x];
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    for (int k = 0; k < SCAN_TILE / 256; k++) {
        const uint64_t i = base + k * 256 + threadIdx.x;
        const uint64_t v = i < n ? (uint64_t)in[i] : 0ull; uint64_t x = v;
        for (int q = 1; q < 64; q <<= 1) { const uint64_t t = (uint64_t)__shfl_up((long long)x, q); if (lane >= q) x += t; }
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        uint64_t woff = 0;
        for (int q = 0; q < wv; q++) woff += s_w[q];
        const uint64_t carry = s_carry, ex = carry + woff + x - v;
        if (i < n) out[i] = ex;
        if (i + 1 == n) out[n] = ex + v;                                              // the total behind the last element
        __syncthreads();
        if (threadIdx.x == 255) s_carry = carry + woff + x;
        __syncthreads();
    }
}
}  // namespace
template <class T> static hipError_t dev_exclusive_sum(const T *in, uint64_t n, uint64_t *out, DevBuf &tmp, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(out, 0, 8, s);
    const unsigned nb = (unsigned)((n + SCAN_TILE - 1) / SCAN_TILE);
    hipError_t e = tmp.ensure((size_t)nb * 8 + 64);
    if (e != hipSuccess) return e;
    uint64_t *part = tmp.as<uint64_t>();
    hipLaunchKernelGGL(k_xs_reduce<T>, dim3(nb), dim3(256), 0, s, in, n, part);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, s, part, (uint64_t)nb, (unsigned long long *)(part + nb), (unsigned long long *)(part + nb + 1));
    hipLaunchKernelGGL(k_xs_apply<T>, dim3(nb), dim3(256), 0, s, in, n, (const uint64_t *)part, out);
    return hipGetLastError();
}
// indices (ascending) of the set flags -> out, their number -> *count (device memory)
static hipError_t dev_select_flagged(const uint8_t *flag, uint64_t n, uint32_t *out, unsigned long long *count, DevBuf &tmp, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(count, 0, 8, s);
    const unsigned nb = (unsigned)((n + SCAN_TILE - 1) / SCAN_TILE);
    hipError_t e = tmp.ensure((size_t)nb * 8 + 64);
    if (e != hipSuccess) return e;
    uint64_t *part = tmp.as<uint64_t>();
    hipLaunchKernelGGL(k_flag_reduce, dim3(nb), dim3(256), 0, s, flag, n, part);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, s, part, (uint64_t)nb, count, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(k_flag_apply, dim3(nb), dim3(256), 0, s, flag, n, (const uint64_t *)part, out);
    return hipGetLastError();
}

// ---- the host drivers.  Each takes plain arguments (buffers, a stream, an error string) and returns a GCE_ status; none knows the objects of
//      its callers.  MCHK: a HIP call that failed names itself in the function's `msg` and ends the function (out of memory apart from the
//      other errors).  It stays defined for gce_passes.hpp, gce_samdev.hpp and gce_samfmt.hpp; engine.hip undefines it behind them.
#define MCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) { msg = std::string(#call) + ": " + hipGetErrorString(_e); return _e == hipErrorOutOfMemory ? GCE_ERR_OOM : GCE_ERR_HIP; } } while (0)

// `b` holds at least `need` bytes afterwards, its first `used` ones kept: a new buffer of exactly new_cap bytes, the prefix copied on s, s
// waited for, the old buffer freed.  The growth rule (new_cap) is the caller's.  *in_alloc: the error returned is the allocation's.
static hipError_t dev_grow_keep(DevBuf &b, size_t need, size_t used, size_t new_cap, hipStream_t s, bool *in_alloc = nullptr) {
    if (need <= b.cap && b.p) return hipSuccess;
    DevBuf nb;
    hipError_t r = nb.take(new_cap);
    if (in_alloc) *in_alloc = r != hipSuccess;
    if (r != hipSuccess) return r;
    if (used && (r = hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, s)) != hipSuccess) { nb.release(); return r; }
    if ((r = hipStreamSynchronize(s)) != hipSuccess) { nb.release(); return r; }
    b.release(); b = nb;
    return hipSuccess;
}

// the buffers of one record index: per segment its guessed start, where its chain leaves, its record count and their scan, the flag of
// k_raw_check; the flag words; the record starts
struct RecIdx {
    DevBuf guess, leave, cnt, base, bad_of, misc, off;
    void release() { for (DevBuf *b : {&guess, &leave, &cnt, &base, &bad_of, &misc, &off}) b->release(); }
};
// The record index of u[first, n): the starts of its records -> x.off[0 .. *n_rec), by the kernels above.  Every segment is walked from a
// guessed start (k_raw_seg) and checked against its predecessor (k_raw_check); up to 64 parallel rounds put the flagged segments on the chain
// (k_raw_fix), then one thread follows it from the first record (k_raw_repair), and the scan of the segments' counts places the offsets
// (k_raw_offsets, queued on s and not waited for).  SOFT: the end may cut a record, *end is where the last whole record ends; otherwise the
// chain must end on n.  ctr: segments, initially flagged, parallel rounds, serial repair -- filled as far as the index came, also when it fails.
template <bool SOFT>
static int dev_record_index(RecIdx &x, DevBuf &tmp, hipStream_t s, const uint8_t *u, uint64_t first, uint64_t n, int32_t n_ref, int64_t ctr[4], uint64_t *n_rec, uint64_t *end, std::string &msg) {
    const uint64_t nseg = (n - first + RAW_SEG - 1) / RAW_SEG;
    const unsigned nbs = (unsigned)((nseg + 255) / 256);
    for (int k = 0; k < 4; k++) ctr[k] = 0;
    MCHK(x.guess.ensure(nseg * 8)); MCHK(x.leave.ensure(nseg * 8)); MCHK(x.cnt.ensure(nseg * 4 + 8)); MCHK(x.base.ensure(nseg * 8 + 8)); MCHK(x.bad_of.ensure(nseg + 8)); MCHK(x.misc.ensure(64));
    uint64_t *guess = x.guess.as<uint64_t>(), *leave = x.leave.as<uint64_t>(); uint32_t *cnt = x.cnt.as<uint32_t>(); unsigned int *misc = x.misc.as<unsigned int>(); uint8_t *bad_of = x.bad_of.as<uint8_t>();
    unsigned int flags[2] = {0, 0};                                                    // misc[0]: segments off the chain, misc[1]: the chain is broken
    const auto check = [&]() -> hipError_t {
        hipError_t r = hipMemcpyAsync(flags, misc, 8, hipMemcpyDeviceToHost, s);
        return r != hipSuccess ? r : hipStreamSynchronize(s);
    };
    MCHK(hipMemsetAsync(misc, 0, 64, s));
    hipLaunchKernelGGL(k_raw_seg<SOFT>, dim3(nbs), dim3(256), 0, s, u, first, n, n_ref, nseg, guess, leave, cnt);
    hipLaunchKernelGGL(k_raw_check<SOFT>, dim3(nbs), dim3(256), 0, s, (const uint64_t *)guess, (const uint64_t *)leave, nseg, n, misc, bad_of);
    MCHK(check());
    ctr[0] = (int64_t)nseg; ctr[1] = flags[0];
    for (int round = 0; flags[0] && round < 64; round++) {                             // parallel repair rounds
        MCHK(hipMemsetAsync(misc, 0, 16, s));
        hipLaunchKernelGGL(k_raw_fix<SOFT>, dim3(nbs), dim3(256), 0, s, u, first, n, nseg, guess, leave, cnt, (const uint8_t *)bad_of);
        hipLaunchKernelGGL(k_raw_check<SOFT>, dim3(nbs), dim3(256), 0, s, (const uint64_t *)guess, (const uint64_t *)leave, nseg, n, misc, bad_of);
        MCHK(check());
        ctr[2]++;
    }
    if (flags[0]) {
        ctr[3] = 1;
        MCHK(hipMemsetAsync(misc, 0, 16, s));
        hipLaunchKernelGGL(k_raw_repair<SOFT>, dim3(1), dim3(64), 0, s, u, first, n, nseg, guess, leave, cnt, misc + 1);
        MCHK(check());
        if (flags[1]) { msg = "truncated or damaged BAM record stream"; return GCE_ERR_INVALID; }
    }
    MCHK(dev_exclusive_sum(cnt, nseg, x.base.as<uint64_t>(), tmp, s));                // exclusive scan of the segments' record counts: the total comes out as base[nseg]
    MCHK(hipMemcpyAsync(n_rec, x.base.as<uint64_t>() + nseg, 8, hipMemcpyDeviceToHost, s));
    if (SOFT) MCHK(hipMemcpyAsync(end, leave + nseg - 1, 8, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    if (SOFT && *end > n) { msg = "truncated or damaged BAM record stream"; return GCE_ERR_INVALID; }
    if (*n_rec >= 0x7FFFFFF0ull) { msg = SOFT ? "truncated or damaged BAM record stream" : "more than 2^31 records in one stream"; return GCE_ERR_INVALID; }
    MCHK(x.off.ensure((size_t)(*n_rec + 1) * 8));
    if (!SOFT || *n_rec) hipLaunchKernelGGL(k_raw_offsets<SOFT>, dim3(nbs), dim3(256), 0, s, u, first, n, nseg, (const uint64_t *)guess, (const uint64_t *)x.base.p, x.off.as<uint64_t>());
    return GCE_OK;
}

// BGZF members -> bytes (k_bgzf_inflate, one lane per member): member k of the caller's directory `dir` (host memory, n entries) lies at
// comp + dir[k].coff and inflates to out + dir[k].uoff; comp and out are device memory, comp_bytes the compressed bytes in use, with 64 more
// behind them that are zeroed here (the bit reader looks up to 32 bytes ahead).  zdir takes the directory and the code lengths of one launch's
// members (320 bytes each), zerr the error word; a launch takes at most 2^18 members, which bounds that scratch.  *first_bad: the first
// member in `dir` that failed a check (its bytes and those of later members are undefined), or -1.
static int dev_inflate_members(uint8_t *comp, size_t comp_bytes, const InfDir *dir, size_t n, uint8_t *out, DevBuf &zdir, DevBuf &zerr, hipStream_t s, int64_t *first_bad, std::string &msg) {
    *first_bad = -1;
    if (!n) return GCE_OK;
    const size_t LAUNCH = (size_t)1 << 18;
    MCHK(zdir.ensure(n * sizeof(InfDir) + std::min(n, LAUNCH) * INF_NSYM)); MCHK(zerr.ensure(16));
    MCHK(hipMemcpyAsync(zdir.p, dir, n * sizeof(InfDir), hipMemcpyHostToDevice, s));
    const unsigned int init[2] = {0u, 0xFFFFFFFFu};                                    // {a member failed, the smallest such member of its launch}
    MCHK(hipMemcpyAsync(zerr.p, init, 8, hipMemcpyHostToDevice, s));
    MCHK(hipMemsetAsync(comp + comp_bytes, 0, 64, s));
    for (size_t base = 0; base < n && *first_bad < 0; base += LAUNCH) {
        const size_t m = std::min(LAUNCH, n - base);
        hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)((m + INF_T - 1) / INF_T)), dim3(INF_T), 0, s, (const uint8_t *)comp, (const InfDir *)zdir.p + base, (uint32_t)m, out, zerr.as<unsigned int>(), zdir.as<uint8_t>() + n * sizeof(InfDir));
        unsigned int got[2] = {0, 0};                                                  // (the member number of a failure is relative to its launch)
        MCHK(hipMemcpyAsync(got, zerr.p, 8, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s));
        if (got[0]) *first_bad = (int64_t)(base + got[1]);
    }
    MCHK(hipGetLastError());
    return GCE_OK;
}

// either encoder of gce_deflate.hpp over `nb` blocks on stream s (codes: see gce_bgzf_deflate_codes)
static void def_launch(int codes, uint32_t nb, hipStream_t s, const uint8_t *in, uint64_t total, uint32_t blk, uint8_t *slots, uint32_t slot, uint32_t *sizes) {
    if (codes == 0) hipLaunchKernelGGL(k_bgzf_deflate, dim3((nb + DEF_T - 1) / DEF_T), dim3(DEF_T), 0, s, in, total, blk, nb, slots, slot, sizes);
    else hipLaunchKernelGGL(k_bgzf_deflate_dyn, dim3((nb + DEF_T - 1) / DEF_T), dim3(DEF_T), 0, s, in, total, blk, nb, slots, slot, sizes, codes);
}
// bytes -> BGZF members, in two steps.  dev_deflate_members: in[0, total) (device memory, readable 64 bytes past its end) in nb blocks of blk
// input bytes, each deflated into its slot of `slot` bytes (slots: nb of them; sizes: nb + 1 words; offs: nb + 1), the sizes scanned;
// *csz = the bytes of the members back to back.  The caller grows or checks its output buffer, then dev_deflate_pack puts them there
// (queued on s and not waited for).
static int dev_deflate_members(int codes, const uint8_t *in, uint64_t total, uint32_t blk, uint32_t nb, uint8_t *slots, uint32_t slot, uint32_t *sizes, uint64_t *offs, DevBuf &tmp, hipStream_t s,
                               uint64_t *csz, std::string &msg) {
    def_launch(codes, nb, s, in, total, blk, slots, slot, sizes);
    MCHK(hipMemsetAsync(sizes + nb, 0, 4, s));
    MCHK(dev_exclusive_sum((const uint32_t *)sizes, (uint64_t)nb, offs, tmp, s));
    MCHK(hipMemcpyAsync(csz, offs + nb, 8, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s));
    return GCE_OK;
}
static void dev_deflate_pack(const uint8_t *slots, uint32_t slot, const uint32_t *sizes, const uint64_t *offs, uint32_t nb, uint8_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_deflate_pack, dim3(std::min<uint32_t>((nb + 3) / 4, 16384u)), dim3(256), 0, s, slots, slot, sizes, offs, nb, out);
}
