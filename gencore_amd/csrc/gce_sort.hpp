// gce_sort.hpp — an unsorted BAM into coordinate order on the GPU (gce_bam_sort).  The file is streamed window by window as the
// BAI indexer streams it (win_inflate_index / win_carry, gce_passes.hpp).  Per window:
//   k_sort_keys     one thread per record: the 64-bit key t << 33 | p << 1 | r of rule S (t: tid, n_ref for an unplaced record; p: pos + 1 as
//                   unsigned; r: the reverse-strand bit), the record's size (4 + block_size) and its offset in the resident stream; the first
//                   record whose tid the header does not have (atomicMin); the unplaced records; the descents (records whose key is below their
//                   predecessor's, the first record of a window against the last one of the window before)
//   one device-to-device copy appends the window's whole records to the resident record buffer
// Resident across windows: the inflated record bytes and 8 + 4 + 8 bytes per record.  After the last window (gce_sort_finish):
//   hipcub::DeviceRadixSort::SortPairs(key, index) over the key bits in use (stable: the input index needs no key bits), the sizes gathered
//   in sorted order, dev_exclusive_sum -> the destination offsets, and
//   k_sort_gather   the record bytes into a second buffer in the new order: 16 lanes per record, 16-byte stores aligned on the DESTINATION
//                   (the bytes in front of the first aligned chunk and behind the last one go as single bytes), source read unaligned
// gce_sort_read hands the sorted stream out in pieces: raw, or as BGZF members of 0xff00 input bytes deflated on the device (dev_deflate_members,
// dev_deflate_pack).  In-core: about 2 x the inflated record bytes + 20 bytes per record + one window; a file beyond that is GCE_ERR_OOM.
//
// A file beyond that is sorted in output-range passes (gce_bam_sort_passes): the key pass streams the file the same way but keeps only key and
// size of every record (gce_sort_key_window); gce_sort_plan sorts and scans as above and inverts the order,
//   k_sort_dest     dest[sidx[j]] = dst[j]: the destination byte offset of every record in INPUT order, the only thing resident afterwards,
// and cuts the sorted stream [0, total) into passes of pass_bytes (a multiple of 0xff00: cuts fall on rule F's member boundaries, not on
// record boundaries).  Pass k streams the file again from its first byte (gce_sort_pass_begin / _window / _end); per window
//   k_sort_scatter  16 lanes per window record: the part of [dest, dest + size) inside the pass's range [lo, hi) goes to the pass buffer with
//                   k_sort_gather's copy (a record that straddles a cut is written partly by each pass it touches); the bytes written are
//                   summed, so that a pass whose records do not tile its range (the input changed) is refused
// and gce_sort_read hands the pass buffer out as it hands out the in-core stream.  tests/pysort.py models the rules.
#pragma once
#include "gce_copy16.hpp"                                                           // sort_copy16: the 16-lane copy k_sort_gather and k_sort_scatter use

namespace {

#define SORT_MAX_RECORDS 0xFFFFFFF0ull

// misc: [0] the first record with tid >= n_ref (atomicMin), [1] unplaced records, [2] descents
__global__ __launch_bounds__(256) void k_sort_keys(const uint8_t *u, const uint64_t *off, int64_t n, uint64_t start, uint64_t res_base, uint64_t gbase, int32_t n_ref,
                                                   unsigned long long *key, uint32_t *size, uint64_t *roff, unsigned long long *misc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    bool unplaced = false, descent = false;
    if (live) {
        const uint64_t o = off[i];
        const uint8_t *r = u + o + 4;
        const int32_t tid = (int32_t)rb32(r), pos = (int32_t)rb32(r + 4);
        const uint32_t flag = rb16(r + 14);
        if (tid >= n_ref) atomicMin(misc, (unsigned long long)(gbase + (uint64_t)i));
        unplaced = tid < 0;
        const unsigned long long t = (unsigned long long)(uint32_t)(tid < 0 || tid >= n_ref ? n_ref : tid);
        const unsigned long long k = t << 33 | (unsigned long long)(uint32_t)(pos + 1) << 1 | ((flag >> 4) & 1u);
        const uint64_t g = gbase + (uint64_t)i;
        key[g] = k; size[g] = 4u + rb32(u + o);
        if (roff) roff[g] = res_base + (o - start);                                  // (NULL in the key pass of the output-range passes: no record bytes stay resident)
        if (g > 0) {                                                                  // (the predecessor of a window's first record: the last key of the window before, resident)
            unsigned long long kp;
            if (i > 0) {
                const uint8_t *q = u + off[i - 1] + 4;
                const int32_t ptid = (int32_t)rb32(q);
                const unsigned long long pt = (unsigned long long)(uint32_t)(ptid < 0 || ptid >= n_ref ? n_ref : ptid);
                kp = pt << 33 | (unsigned long long)(uint32_t)((int32_t)rb32(q + 4) + 1) << 1 | ((rb16(q + 14) >> 4) & 1u);
            } else kp = key[g - 1];
            descent = k < kp;
        }
    }
    const unsigned long long bu = __ballot(unplaced), bd = __ballot(descent);
    if (lane_id() == 0) {
        if (bu) atomicAdd(misc + 1, (unsigned long long)__popcll(bu));
        if (bd) atomicAdd(misc + 2, (unsigned long long)__popcll(bd));
    }
}
__global__ __launch_bounds__(256) void k_sort_iota(uint32_t *idx, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_sort_sizes(const uint32_t *size, const uint32_t *sidx, uint64_t n, uint32_t *ssize) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) ssize[j] = size[sidx[j]];
}
// 16 lanes per record of the sorted order: record j = input record sidx[j], ssize[j] bytes from src + roff[sidx[j]] to out + dst[j] (sort_copy16)
__global__ __launch_bounds__(256) void k_sort_gather(const uint8_t *src, const uint64_t *roff, const uint32_t *sidx, const uint32_t *ssize, const uint64_t *dst, uint64_t n, uint8_t *out) {
    const uint32_t sub = threadIdx.x & 15u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < n; j += ((uint64_t)gridDim.x * blockDim.x) >> 4)
        sort_copy16(src + roff[sidx[j]], out + dst[j], ssize[j], sub);
}
// the inverse of the sorted order: the destination byte offset of every record in input order
__global__ __launch_bounds__(256) void k_sort_dest(const uint32_t *sidx, const uint64_t *dst, uint64_t n, uint64_t *dest) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dest[sidx[j]] = dst[j];
}
// one pass of the output-range passes over one window: 16 lanes per window record (a wave takes four records at a time, so that its trip
// count is uniform).  Record i is global record gbase + i, sz bytes (its own block_size) for [d, d + sz) of the sorted stream, d = dest[gbase + i].
// Outside [lo, hi): nothing to do ((P - 1) / P of the records).  Otherwise the stretch [max(d, lo), min(d + sz, hi)) goes to out at - lo, the
// source advanced by the same clip: reads stay inside the record, writes inside [0, hi - lo).  misc: [0] |= 1 for a record whose
// [d, d + sz) leaves [0, total] (nothing is copied); [1] += the bytes written.
__global__ __launch_bounds__(256) void k_sort_scatter(const uint8_t *u, const uint64_t *off, uint64_t n, const uint64_t *dest, uint64_t gbase, uint64_t lo, uint64_t hi, uint64_t total,
                                                      uint8_t *out, unsigned long long *misc) {
    const uint32_t lane = threadIdx.x & 63u, sub = lane & 15u;
    const uint64_t step = (((uint64_t)gridDim.x * blockDim.x) >> 6) << 2;
    for (uint64_t j0 = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 2; j0 < n; j0 += step) {
        const uint64_t j = j0 + (lane >> 4);
        unsigned long long len = 0; bool bad = false;
        if (j < n) {
            const uint8_t *s = u + off[j];
            const uint64_t sz = 4ull + rb32(s), d = dest[gbase + j];
            if (d > total || sz > total - d) bad = true;
            else {
                const uint64_t a = max(d, lo), z = min(d + sz, hi);
                if (a < z) {
                    sort_copy16(s + (a - d), out + (a - lo), (uint32_t)(z - a), sub);
                    if (sub == 0) len = z - a;
                }
            }
        }
        const unsigned long long bb = __ballot(bad);
        len += __shfl_xor(len, 16); len += __shfl_xor(len, 32);
        if (lane == 0) {
            if (bb) atomicOr(misc, 1ull);
            if (len) atomicAdd(misc + 1, len);
        }
    }
}

}  // namespace

struct gce_sort {
    int32_t device = 0;
    hipStream_t s = nullptr;
    std::string err;
    uint64_t budget = 0;                                                              // device bytes the process may hold (0: no limit beyond the device)
    WinIdx w; DevBuf tmp, misc;                                                       // the window; the counters of k_sort_keys
    DevBuf rec, key, size, off; uint64_t rec_n = 0, n = 0;                            // resident: the records' bytes, key / size / offset of each
    DevBuf out; uint64_t out_n = 0;                                                   // the sorted stream (gce_sort_finish)
    DevBuf zs, zz, zf, zo;                                                            // a piece's deflate slots, sizes, offsets, packed members
    // the output-range passes: no record bytes resident (rec_n counts them); after gce_sort_plan only dest; `out` is the pass buffer
    bool passes = false;
    DevBuf dest, pmisc; uint64_t total = 0, win_need = 0;                             // dest: 8 bytes per record; win_need: the device bytes a window took in the key pass
    uint64_t p_lo = 0, p_hi = 0, p_g = 0; bool p_open = false; double p_scatter_s = 0;
    // SAM text in (gce_sam_sort, gce_samdev.hpp): the window is text, its records are written straight into `rec`
    bool sam_text = false; SamDev sam;
    // calmd (gce_bam_calmd, gce_calmd.hpp): nothing is sorted; every window's records are rewritten straight into `out`, behind the ones before
    bool calmd = false; DevBuf cm_blob, cm_tab, cm_size, cm_meta, cm_dst; uint64_t cm_in = 0;   // the reference and its table; a window's sizes, descriptions, destinations
    // calmd with its output streamed (gce_bam_calmd_stream): `out` holds at most cm_cap bytes beside one window's; whole members leave early
    bool cm_stream = false; int32_t cm_codes = -1, cm_flushes = 0; uint64_t cm_piece = 0, cm_cap = 0, cm_flushed = 0;
    // the UMI pass (gce_bam_umi_to_mi, gce_umi.hpp): calmd mode, streamed, under another record rewriter; um_src: 0 the read name, else the tag's two bytes
    bool umi = false; uint32_t um_src = 0;
    // overlapping mates merged (gce_bam_merge_overlap, gce_ovlmerge.hpp): nothing is sorted; after the last window `rec` is rewritten in place and becomes `out`
    bool overlap = false;
};

static int sfail(gce_sort *b, int code, const std::string &m) { if (b) b->err = m; return code; }
static int sort_oom(gce_sort *b, const char *what, uint64_t add) {
    char m[256];                                                                      // (the footprint first: a long `what` is cut off, not the formula)
    snprintf(m, sizeof m, b->overlap ? "out of device memory: gce_bam_merge_overlap is in-core and needs the inflated record bytes + 20 bytes per record + one window, then a join table of about 24 bytes per record (%lld bytes live, budget %llu, %llu more for %s)" :
                          b->umi ? "out of device memory: gce_bam_umi_to_mi needs one window + 40 bytes per window record + one piece's deflate buffers + at least one window's output (%lld bytes live, budget %llu, %llu more for %s)" :
                          b->cm_stream ? "out of device memory: gce_bam_calmd_stream needs the reference bases + one window + 40 bytes per window record + one piece's deflate buffers + at least one window's output (%lld bytes live, budget %llu, %llu more for %s)" :
                          b->calmd ? "out of device memory: calmd is in-core and needs about the output record bytes + the reference bases + 40 bytes per window record + one window (%lld bytes live, budget %llu, %llu more for %s)" :
                          b->sam_text ? "out of device memory: SAM text is sorted in-core only (else gce_sam_to_bam, then gce_bam_sort_passes): 2 x the record bytes + 20 per record + a window of 2 per text byte + 41 per line (%lld live, budget %llu, %llu more for %s)" :
                          b->passes ? "out of device memory: the sort in output-range passes needs 8 bytes per record + one window + one pass of at least one BGZF member (about 44 bytes per record for its plan) (%lld bytes live, budget %llu, %llu more for %s)"
                                    : "out of device memory: the sort is in-core and needs about 2 x the inflated record bytes + 20 bytes per record + one window (%lld bytes live, budget %llu, %llu more for %s)",
             __atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), (unsigned long long)b->budget, (unsigned long long)add, what);
    return sfail(b, GCE_ERR_OOM, m);
}
#define SCHK(call) do { hipError_t _e = (call); if (_e == hipErrorOutOfMemory) return sort_oom(b, #call, 0); if (_e != hipSuccess) return sfail(b, GCE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); } while (0)
// may `add` more device bytes be taken?  (the live count of gce_device_bytes against the budget, before the allocation)
static bool sort_room(const gce_sort *b, uint64_t add) {
    return !b->budget || (uint64_t)std::max<long long>(__atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), 0) + add <= b->budget;
}
// `buf` holds at least `need` bytes, its first `used` ones kept; a new buffer has exactly max(need, target) bytes (DevBuf::ensure would add an
// eighth, and the resident record buffer is the sort's largest: it is sized once from the caller's estimate, so that it seldom grows)
static int sort_grow(gce_sort *b, DevBuf &buf, size_t need, size_t used, size_t target, const char *what) {
    if (need <= buf.cap && buf.p) return GCE_OK;
    const size_t want = std::max(need, target) + 256;
    if (!sort_room(b, want)) return sort_oom(b, what, want);
    bool in_alloc = false;
    const hipError_t r = dev_grow_keep(buf, need, used, want, b->s, &in_alloc);
    if (r == hipErrorOutOfMemory && in_alloc) return sort_oom(b, what, want);
    return r == hipSuccess ? GCE_OK : sfail(b, GCE_ERR_HIP, std::string(in_alloc ? "hipMalloc: " : "") + hipGetErrorString(r));
}
// the slots of one deflated piece of `piece` input bytes
static uint32_t sort_slot() { return 0xff00u + 0xff00u / 8 + 64; }
// the device bytes of the four buffers gce_sort_read deflates a piece of pn members with, as DevBuf::ensure takes them
static uint64_t sort_deflate_need(uint64_t pn) { return (pn * sort_slot() + 64) * 9 / 4 + pn * 14 + 2048; }
static int sort_deflate_bufs(gce_sort *b, uint64_t piece_bytes) {
    const uint64_t pn = (piece_bytes + 0xff00u - 1) / 0xff00u;
    if (!sort_room(b, sort_deflate_need(pn))) return sort_oom(b, "deflating a piece of the output", sort_deflate_need(pn));
    SCHK(b->zs.ensure((size_t)pn * sort_slot() + 64)); SCHK(b->zo.ensure((size_t)pn * sort_slot() + 64)); SCHK(b->zz.ensure(((size_t)pn + 1) * 4)); SCHK(b->zf.ensure(((size_t)pn + 1) * 8));
    return GCE_OK;
}
// the device bytes a window holds (a window that grows holds its old inflated bytes beside the new ones for a moment: pass_grow)
static uint64_t sort_win_need(const WinIdx &w, const DevBuf &tmp) { return w.win.cap + tmp.cap + w.held(); }
// before win_inflate_index makes the window's own buffers: is there room for them (win_room)?
static int sort_win_check(gce_sort *b, size_t comp_bytes, int32_t n_members, const uint32_t *usize) {
    uint64_t u_all = b->w.carry_n; for (int32_t k = 0; k < n_members; k++) u_all += usize[k];
    const uint64_t add = win_room(b->w, comp_bytes, u_all);
    return add && !sort_room(b, add) ? sort_oom(b, "a window of the file", add) : GCE_OK;
}
// the counters of k_sort_keys, made and set on first use
static int sort_counters_init(gce_sort *b) {
    if (b->misc.p) return GCE_OK;
    if (!sort_room(b, 512)) return sort_oom(b, "the sort's counters", 512);
    SCHK(b->misc.ensure(64));
    const unsigned long long init[3] = {~0ull, 0ull, 0ull};
    SCHK(hipMemcpyAsync(b->misc.p, init, sizeof init, hipMemcpyHostToDevice, b->s)); SCHK(hipStreamSynchronize(b->s));
    return GCE_OK;
}
// room for n_rec more records of add_bytes bytes behind the resident ones (the output-range passes keep neither the bytes nor their offsets).
// A buffer that has to be made or grown is sized from the estimates: the file's record bytes (est_bytes, never below what is known), and its
// records at the bytes per record seen so far, 1/16 added to each.
static int sort_take(gce_sort *b, uint64_t n_rec, uint64_t add_bytes, uint64_t est_bytes) {
    const uint64_t n1 = b->n + n_rec, have = b->rec_n + add_bytes;
    const uint64_t eb = std::max<uint64_t>(est_bytes, have), en = (uint64_t)((double)n1 * ((double)eb / (double)have));
    const size_t tn = (size_t)(en + en / 16 + 64);
    int rc;
    if (!b->passes && (rc = sort_grow(b, b->rec, (size_t)(have + 64), (size_t)b->rec_n, (size_t)(eb + eb / 16 + 64), "the resident record bytes")) != GCE_OK) return rc;
    if ((rc = sort_grow(b, b->key, (size_t)n1 * 8, (size_t)b->n * 8, tn * 8, "the records' keys")) != GCE_OK) return rc;
    if ((rc = sort_grow(b, b->size, (size_t)n1 * 4, (size_t)b->n * 4, tn * 4, "the records' sizes")) != GCE_OK) return rc;
    if (!b->passes && (rc = sort_grow(b, b->off, (size_t)n1 * 8, (size_t)b->n * 8, tn * 8, "the records' offsets")) != GCE_OK) return rc;
    return GCE_OK;
}

extern "C" {

int gce_sort_create(int32_t device, size_t device_budget_bytes, gce_sort **out) {
    if (!out) return GCE_ERR_INVALID;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    gce_sort *b = new gce_sort();
    b->device = device; b->budget = (uint64_t)device_budget_bytes;
    if (hipStreamCreate(&b->s) != hipSuccess) { delete b; return GCE_ERR_HIP; }
    *out = b;
    return GCE_OK;
}
void gce_sort_destroy(gce_sort *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->s);
    b->w.release(); b->sam.release();
    for (DevBuf *x : {&b->tmp, &b->misc, &b->rec, &b->key, &b->size, &b->off, &b->out, &b->zs, &b->zz, &b->zf, &b->zo, &b->dest, &b->pmisc, &b->cm_blob, &b->cm_tab, &b->cm_size, &b->cm_meta, &b->cm_dst}) x->release();
    (void)hipStreamDestroy(b->s);
    delete b;
}
const char *gce_sort_error(gce_sort *b) { return b ? b->err.c_str() : ""; }

// the next piece of the file, as gce_bai_window takes it.  est_bytes: the caller's estimate of the whole file's inflated bytes (the members'
// ISIZE totals so far scaled to the file size): the resident buffers are sized from it when they are first made, or grow.
static int sort_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                       int32_t n_ref, int32_t last, uint64_t est_bytes) {
    if (!b || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize))) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    int rc;
    if ((rc = sort_win_check(b, comp_bytes, n_members, usize)) != GCE_OK || (rc = sort_counters_init(b)) != GCE_OK) return rc;
    uint64_t total = 0, n_rec = 0, end = 0;
    rc = win_inflate_index(b->w, b->tmp, s, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, nullptr, &total, &n_rec, &end, b->err);
    if (rc == GCE_ERR_OOM) return sort_oom(b, "a window of the file", 0);
    if (rc != GCE_OK) return rc;
    if (n_rec) {
        const uint64_t start = std::min<uint64_t>(skip, total), add = end - start, n1 = b->n + n_rec;
        if (n1 >= SORT_MAX_RECORDS) return sfail(b, GCE_ERR_INVALID, "more than 2^32 - 16 records in one BAM file");
        if ((rc = sort_take(b, n_rec, add, est_bytes)) != GCE_OK) return rc;
        hipLaunchKernelGGL(k_sort_keys, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, (const uint8_t *)b->w.win.p, (const uint64_t *)b->w.idx.off.p, (int64_t)n_rec, start, b->rec_n, b->n, n_ref,
                           b->key.as<unsigned long long>(), b->size.as<uint32_t>(), b->off.as<uint64_t>(), b->misc.as<unsigned long long>());
        SCHK(hipGetLastError());
        if (!b->passes) SCHK(hipMemcpyAsync(b->rec.as<uint8_t>() + b->rec_n, b->w.win.as<uint8_t>() + start, add, hipMemcpyDeviceToDevice, s));
        b->rec_n += add; b->n = n1;
    }
    rc = win_carry(b->w, s, total, end, b->err);
    b->win_need = std::max(b->win_need, sort_win_need(b->w, b->tmp));
    return rc;
}
int gce_sort_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                    int32_t n_ref, int32_t last, uint64_t est_bytes) {
    if (b && b->passes) return GCE_ERR_INVALID;
    return sort_window(b, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, est_bytes);
}
// the key pass of the output-range passes: gce_sort_window without the record bytes and their offsets (12 bytes per record stay resident)
int gce_sort_key_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, uint64_t est_bytes) {
    if (!b || b->rec.p || b->dest.p) return GCE_ERR_INVALID;
    b->passes = true;
    return sort_window(b, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, est_bytes);
}

// SAM text in (gce_sam_sort): the contig names once, then window after window of whole alignment lines (host memory, n < 2^32).  The lines
// become BAM records on the device (gce_samdev.hpp), written behind the resident records; their starts are what w.idx.off is to gce_sort_window.
// *bad_line >= 0: the window's first bad line (counting its record lines from 0), *bad_start its first byte in text, the error line_to_bam's
// message for it; nothing of the window is kept.  *n_host_lines: the lines the host re-parsed (floating-point values); it and *parse_s are
// added to.  *resident_bytes: the record bytes held so far.
int gce_sort_sam_contigs(gce_sort *b, int32_t n_ref, const char *const *ref_name) {
    if (!b || n_ref < 0 || (n_ref && !ref_name) || b->passes) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    b->sam_text = true;
    std::vector<std::string> names; for (int32_t k = 0; k < n_ref; k++) names.emplace_back(ref_name[k] ? ref_name[k] : "");
    uint64_t nb = 0; for (const std::string &x : names) nb += x.size() + 8;
    if (!sort_room(b, nb + nb / 4 + 1024)) return sort_oom(b, "the contig names", nb + nb / 4 + 1024);
    const int rc = sam_contigs(b->sam, b->s, names, b->err);
    return rc == GCE_ERR_OOM ? sort_oom(b, "the contig names", 0) : rc;
}
int gce_sort_sam_window(gce_sort *b, const char *text, size_t n, int32_t n_ref, uint64_t est_bytes, int64_t *n_host_lines, int64_t *bad_line, uint64_t *bad_start, double *parse_s,
                        uint64_t *resident_bytes) {
    if (!b || !resident_bytes || !b->sam_text || b->passes || (n && !text) || n >= 0xFFFFFF00ull || !n_host_lines || !bad_line || !bad_start || !parse_s) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    SamDev &d = b->sam;
    *bad_line = -1; *bad_start = 0;
    int rc = sort_counters_init(b);
    if (rc != GCE_OK) return rc;
    const double k0 = d.kernel_s;
    auto grown = [&](uint64_t need) { const uint64_t held = d.held(); return need > held ? need - held : 0; };
    { const uint64_t add = grown(sam_win_need(n, 0)); if (add && !sort_room(b, add)) return sort_oom(b, "a window of SAM text", add); }
    rc = sam_lines(d, b->tmp, s, text, n, b->err);
    if (rc == GCE_ERR_OOM) return sort_oom(b, "a window of SAM text", 0);
    if (rc != GCE_OK) return rc;
    { const uint64_t add = grown(sam_win_need(n, d.nl)); if (add && !sort_room(b, add)) return sort_oom(b, "the lines of a window of SAM text", add); }
    rc = sam_sizes(d, b->tmp, s, b->err);
    if (rc == GCE_ERR_OOM) return sort_oom(b, "the lines of a window of SAM text", 0);
    if (rc != GCE_OK) return rc;
    if (d.n_host) { const uint64_t add = sam_host_need(d); if (add > d.hstage.cap + d.hsoff.cap && !sort_room(b, add)) return sort_oom(b, "the host's records of the lines with floating-point values", add); }
    if (d.bad >= 0) { *bad_line = d.bad; *bad_start = d.bad_start; *parse_s += d.kernel_s - k0; return sfail(b, GCE_ERR_INVALID, sam_line_message(d, text, n, d.bad_start)); }
    const uint64_t n_rec = d.nl, add = d.total;
    if (n_rec) {
        const uint64_t n1 = b->n + n_rec;
        if (n1 >= SORT_MAX_RECORDS) return sfail(b, GCE_ERR_INVALID, "more than 2^32 - 16 records in one SAM file");
        if ((rc = sort_take(b, n_rec, add, est_bytes)) != GCE_OK) return rc;
        uint8_t *dst = b->rec.as<uint8_t>() + b->rec_n;
        if ((rc = sam_emit(d, s, text, dst, b->err)) != GCE_OK) return rc;
        hipLaunchKernelGGL(k_sort_keys, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, (const uint8_t *)dst, (const uint64_t *)d.roff.p, (int64_t)n_rec, (uint64_t)0, b->rec_n, b->n, n_ref,
                           b->key.as<unsigned long long>(), b->size.as<uint32_t>(), b->off.as<uint64_t>(), b->misc.as<unsigned long long>());
        SCHK(hipGetLastError()); SCHK(hipStreamSynchronize(s));
        b->rec_n += add; b->n = n1;
    }
    *n_host_lines += (int64_t)d.n_host; *parse_s += d.kernel_s - k0;
    b->win_need = std::max(b->win_need, d.held());
    *resident_bytes = b->rec_n;
    return GCE_OK;
}

// the order and where it puts every record: sidx[j] = the input record at place j, ssize[j] its size, dst[j] its byte offset in the sorted
// stream (dst[n] = *total).  Keys and sizes are released on the way.
static int sort_order(gce_sort *b, int32_t n_ref, ScopedBuf &sidx, ScopedBuf &ssize, ScopedBuf &dst, uint64_t *total_out) {
    hipStream_t s = b->s;
    const uint64_t n = b->n;
    const unsigned nb = (unsigned)((n + 255) / 256);
    int end_bit = 33; for (uint32_t v = (uint32_t)n_ref; v; v >>= 1) end_bit++;
    {
        ScopedBuf idx, skey, st;
        if (!sort_room(b, n * 18)) return sort_oom(b, "the radix sort of the keys", n * 18);
        SCHK(idx.ensure(n * 4)); SCHK(sidx.ensure(n * 4)); SCHK(skey.ensure(n * 8));
        hipLaunchKernelGGL(k_sort_iota, dim3(nb), dim3(256), 0, s, idx.as<uint32_t>(), n);
        size_t tb = 0;
        SCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, b->key.as<unsigned long long>(), skey.as<unsigned long long>(), idx.as<uint32_t>(), sidx.as<uint32_t>(), n, 0, end_bit, s));
        if (!sort_room(b, tb + tb / 8 + 320)) return sort_oom(b, "the radix sort of the keys", tb);
        SCHK(st.ensure(tb + 64));
        SCHK(hipcub::DeviceRadixSort::SortPairs(st.p, tb, b->key.as<unsigned long long>(), skey.as<unsigned long long>(), idx.as<uint32_t>(), sidx.as<uint32_t>(), n, 0, end_bit, s));
        SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    }
    b->key.release();
    if (!sort_room(b, n * 14)) return sort_oom(b, "the destination offsets", n * 14);
    SCHK(ssize.ensure(n * 4)); SCHK(dst.ensure((n + 1) * 8));
    hipLaunchKernelGGL(k_sort_sizes, dim3(nb), dim3(256), 0, s, (const uint32_t *)b->size.p, (const uint32_t *)sidx.p, n, ssize.as<uint32_t>());
    SCHK(dev_exclusive_sum(ssize.as<uint32_t>(), n, dst.as<uint64_t>(), b->tmp, s));
    uint64_t total = 0;
    SCHK(hipMemcpyAsync(&total, dst.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    if (total != b->rec_n) return sfail(b, GCE_ERR_INVALID, "sort: the records' sizes do not add up to the resident stream");
    b->size.release();
    *total_out = total;
    return GCE_OK;
}
// after the last window, both ways: the counters of k_sort_keys.  *bad_rec >= 0: nothing is sorted
static int sort_counts(gce_sort *b, int64_t counts[3], int64_t *bad_rec) {
    hipStream_t s = b->s;
    *bad_rec = -1;
    counts[0] = (int64_t)b->n; counts[1] = counts[2] = 0;
    if (b->n == 0) return GCE_OK;
    unsigned long long h[3];
    SCHK(hipMemcpyAsync(h, b->misc.p, sizeof h, hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    if (h[0] != ~0ull) { *bad_rec = (int64_t)h[0]; return GCE_OK; }
    counts[1] = (int64_t)h[1]; counts[2] = (int64_t)h[2];
    return GCE_OK;
}

// after the last window: sort, scan, gather.  counts: records, unplaced records, descents; *bad_rec: the first record whose tid the header
// does not have (-1: none; nothing is sorted then); *out_bytes: the sorted stream's bytes; times: seconds of the sort (keys, sizes, scan) and
// of the gather kernel.  codes >= 0: the buffers gce_sort_read deflates pieces of up to piece_bytes with are made here, so that running out
// of device memory is known before the caller opens its output.
int gce_sort_finish(gce_sort *b, int32_t n_ref, int32_t codes, uint64_t piece_bytes, int64_t counts[3], int64_t *bad_rec, uint64_t *out_bytes, double times[2]) {
    if (!b || b->passes || n_ref < 0 || !counts || !bad_rec || !out_bytes || !times || codes > 1) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    SCHK(hipStreamSynchronize(s));
    b->w.release(); b->sam.release();                                                 // (the last window is done with)
    *out_bytes = 0; times[0] = times[1] = 0;
    int rc = sort_counts(b, counts, bad_rec);
    if (rc != GCE_OK || b->n == 0 || *bad_rec >= 0) return rc;
    const uint64_t n = b->n;
    double t0 = mono_s();
    ScopedBuf sidx, ssize, dst;
    uint64_t total = 0;
    if ((rc = sort_order(b, n_ref, sidx, ssize, dst, &total)) != GCE_OK) return rc;
    times[0] = mono_s() - t0;
    if ((rc = sort_grow(b, b->out, (size_t)total + 64, 0, 0, "the sorted record bytes")) != GCE_OK) return rc;
    SCHK(hipMemsetAsync(b->out.as<uint8_t>() + total, 0, 64, s));                    // (the deflate kernels may look a few bytes ahead)
    SCHK(hipStreamSynchronize(s));
    t0 = mono_s();                                                                    // (gather_s: the kernel alone, not the output buffer's hipMalloc)
    hipLaunchKernelGGL(k_sort_gather, dim3((unsigned)std::min<uint64_t>((n + 15) / 16, 65535u)), dim3(256), 0, s, (const uint8_t *)b->rec.p, (const uint64_t *)b->off.p, (const uint32_t *)sidx.p,
                       (const uint32_t *)ssize.p, (const uint64_t *)dst.p, n, b->out.as<uint8_t>());
    SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    times[1] = mono_s() - t0;
    b->rec.release(); b->off.release();
    b->out_n = total; *out_bytes = total;
    if (codes >= 0 && piece_bytes) return sort_deflate_bufs(b, std::min<uint64_t>(piece_bytes, total));
    return GCE_OK;
}

// after the last window of the key pass: sort and scan as gce_sort_finish, then the inverse (k_sort_dest) and the pass cuts.  counts / *bad_rec
// as gce_sort_finish; *total: the sorted stream's bytes.  P = max(min_passes, 1), raised until dest + one window (what a window took in the
// key pass) + the pass buffer + the deflate buffers of its largest piece fit the budget, 64 at most; *pass_bytes = ceil(total / P) rounded up
// to a multiple of 0xff00, *n_passes = ceil(total / pass_bytes).  The pass buffer and the deflate buffers are made here, so that running out
// of device memory is known before the caller opens its output.  *resident: the device bytes held from here on, a window's aside.
int gce_sort_plan(gce_sort *b, int32_t n_ref, int32_t codes, uint64_t piece_bytes, int32_t min_passes, int64_t counts[3], int64_t *bad_rec, uint64_t *total_out, int32_t *n_passes,
                  uint64_t *pass_bytes, uint64_t *resident, double *plan_s) {
    if (!b || !b->passes || b->dest.p || n_ref < 0 || !counts || !bad_rec || !total_out || !n_passes || !pass_bytes || !resident || !plan_s || codes > 1 || min_passes > 64) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    SCHK(hipStreamSynchronize(s));
    b->w.release();                                                                   // (the plan's scratch takes its place; the passes make it again)
    *total_out = 0; *n_passes = 0; *pass_bytes = 0; *resident = 0; *plan_s = 0;
    int rc = sort_counts(b, counts, bad_rec);
    if (rc != GCE_OK || b->n == 0 || *bad_rec >= 0) return rc;
    const uint64_t n = b->n;
    const double t0 = mono_s();
    uint64_t total = 0;
    {
        ScopedBuf sidx, ssize, dst;
        if ((rc = sort_order(b, n_ref, sidx, ssize, dst, &total)) != GCE_OK) return rc;
        if ((rc = sort_grow(b, b->dest, (size_t)n * 8, 0, 0, "the records' destinations")) != GCE_OK) return rc;
        hipLaunchKernelGGL(k_sort_dest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint32_t *)sidx.p, (const uint64_t *)dst.p, n, b->dest.as<uint64_t>());
        SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    }
    if (!b->pmisc.p) { if (!sort_room(b, 512)) return sort_oom(b, "the passes' counters", 512); SCHK(b->pmisc.ensure(64)); }
    b->total = total;
    // ---- the cuts: the smallest P from min_passes on whose pass fits
    const uint64_t M = 0xff00u, slack = 65536;                                       // (slack: dev_exclusive_sum's scratch, allocator rounding)
    const uint64_t live = (uint64_t)std::max<long long>(__atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), 0);
    auto pass_need = [&](uint64_t pb) { return pb + 64 + 256 + (codes >= 0 && piece_bytes ? sort_deflate_need((std::min<uint64_t>(piece_bytes, pb) + M - 1) / M) : 0); };
    uint64_t P = (uint64_t)std::max<int32_t>(min_passes, 1), pb = 0;
    for (;; P++) {
        pb = ((total + P - 1) / P + M - 1) / M * M;
        if (!b->budget || live + b->win_need + slack + pass_need(pb) <= b->budget) break;
        if (P == 64 || pb == M) return sort_oom(b, "a window and one pass of the output", b->win_need + slack + pass_need(pb));
    }
    *total_out = total; *pass_bytes = pb; *n_passes = (int32_t)((total + pb - 1) / pb);
    if ((rc = sort_grow(b, b->out, (size_t)pb + 64, 0, 0, "one pass of the sorted record bytes")) != GCE_OK) return rc;
    if (codes >= 0 && piece_bytes && (rc = sort_deflate_bufs(b, std::min<uint64_t>(piece_bytes, pb))) != GCE_OK) return rc;
    *resident = (uint64_t)std::max<long long>(__atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), 0);
    *plan_s = mono_s() - t0;
    return GCE_OK;
}

// pass k of the output-range passes: bytes [lo, hi) of the sorted stream (lo a multiple of 0xff00) are collected in the pass buffer while the
// file goes by once more, window by window, from its first byte; after gce_sort_pass_end, gce_sort_read hands them out (offsets from lo).
int gce_sort_pass_begin(gce_sort *b, uint64_t lo, uint64_t hi) {
    if (!b || !b->passes || !b->dest.p || b->p_open || lo >= hi || hi > b->total || lo % 0xff00u || hi - lo + 64 > b->out.cap) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    b->p_lo = lo; b->p_hi = hi; b->p_g = 0; b->p_scatter_s = 0; b->out_n = 0; b->p_open = true;
    b->w.carry_n = 0;
    SCHK(hipMemsetAsync(b->pmisc.p, 0, 64, s));
    SCHK(hipMemsetAsync(b->out.as<uint8_t>() + (hi - lo), 0, 64, s));                // (the deflate kernels may look a few bytes ahead)
    return GCE_OK;
}
int gce_sort_pass_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                         int32_t n_ref, int32_t last) {
    if (!b || !b->p_open || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize))) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    int rc = sort_win_check(b, comp_bytes, n_members, usize);
    if (rc != GCE_OK) return rc;
    uint64_t total = 0, n_rec = 0, end = 0;
    rc = win_inflate_index(b->w, b->tmp, s, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, nullptr, &total, &n_rec, &end, b->err);
    if (rc == GCE_ERR_OOM) return sort_oom(b, "a window of the file", 0);
    if (rc != GCE_OK) return rc;
    if (n_rec) {
        if (n_rec > b->n - b->p_g) return sfail(b, GCE_ERR_INVALID, "the input changed while it was being sorted (more records than the key pass saw)");
        const double t0 = mono_s();
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)std::min<uint64_t>((n_rec + 15) / 16, 65535u)), dim3(256), 0, s, (const uint8_t *)b->w.win.p, (const uint64_t *)b->w.idx.off.p, n_rec,
                           (const uint64_t *)b->dest.p, b->p_g, b->p_lo, b->p_hi, b->total, b->out.as<uint8_t>(), b->pmisc.as<unsigned long long>());
        SCHK(hipGetLastError()); SCHK(hipStreamSynchronize(s));
        b->p_scatter_s += mono_s() - t0;
        b->p_g += n_rec;
    }
    return win_carry(b->w, s, total, end, b->err);
}
// *scatter_s: the seconds of the pass's k_sort_scatter launches.  A pass that saw another record count than the key pass, a record outside
// [0, total] or whose records did not write every byte of [lo, hi) once is GCE_ERR_INVALID.
int gce_sort_pass_end(gce_sort *b, double *scatter_s) {
    if (!b || !b->p_open) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    b->p_open = false;
    unsigned long long h[2] = {0, 0};
    SCHK(hipMemcpyAsync(h, b->pmisc.p, sizeof h, hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    if (b->p_g != b->n || h[0] || h[1] != b->p_hi - b->p_lo) return sfail(b, GCE_ERR_INVALID, "the input changed while it was being sorted");
    b->out_n = b->p_hi - b->p_lo;
    if (scatter_s) *scatter_s = b->p_scatter_s;
    return GCE_OK;
}

// bytes [offset, offset + bytes) of the sorted stream to `host`: codes < 0: as they are; 0 / 1: as BGZF members of 0xff00 input bytes each,
// deflated on the device with fixed codes / the smallest of dynamic, fixed and stored per member (offset: a multiple of 0xff00).  *got: the
// bytes written to host (at most host_cap: n + n / 8 + 64 per member is always enough).
int gce_sort_read(gce_sort *b, uint64_t offset, size_t bytes, int32_t codes, void *host, size_t host_cap, size_t *got) {
    if (!b || !got || codes > 1 || offset > b->out_n || bytes > b->out_n - offset || (bytes && !host)) return GCE_ERR_INVALID;
    *got = 0;
    if (!bytes) return GCE_OK;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    const uint8_t *in = b->out.as<uint8_t>() + offset;
    if (codes < 0) {
        if (bytes > host_cap) return GCE_ERR_INVALID;
        SCHK(hipMemcpyAsync(host, in, bytes, hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s));
        *got = bytes;
        return GCE_OK;
    }
    if (offset % 0xff00u) return GCE_ERR_INVALID;
    const uint64_t nb64 = (bytes + 0xff00u - 1) / 0xff00u;
    if (nb64 >= 0x7FFFFFF0ull) return GCE_ERR_INVALID;
    const uint32_t nb = (uint32_t)nb64, slot = sort_slot();
    // (gce_sort_finish made the four buffers for the largest piece: nothing grows here, behind the caller's open output)
    if ((size_t)nb * slot + 64 > b->zs.cap || (size_t)nb * slot + 64 > b->zo.cap || ((size_t)nb + 1) * 4 > b->zz.cap || ((size_t)nb + 1) * 8 > b->zf.cap)
        return sfail(b, GCE_ERR_INVALID, "sort: a piece larger than gce_sort_finish was told");
    uint64_t csz = 0;
    const int rc = dev_deflate_members(codes, in, (uint64_t)bytes, 0xff00u, nb, b->zs.as<uint8_t>(), slot, b->zz.as<uint32_t>(), b->zf.as<uint64_t>(), b->tmp, s, &csz, b->err);
    if (rc == GCE_ERR_OOM) return sort_oom(b, std::string(b->err, 0, b->err.rfind(": ")).c_str(), 0);   // (as SCHK: the call that ran out of memory)
    if (rc != GCE_OK) return rc;
    if (csz > host_cap) return sfail(b, GCE_ERR_INVALID, "sort: a deflated piece is larger than its host buffer");
    if (csz + 64 > b->zo.cap) return sfail(b, GCE_ERR_INVALID, "sort: a deflated piece is larger than its device buffer");
    dev_deflate_pack((const uint8_t *)b->zs.p, slot, (const uint32_t *)b->zz.p, (const uint64_t *)b->zf.p, nb, b->zo.as<uint8_t>(), s);
    SCHK(hipMemcpyAsync(host, b->zo.p, csz, hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    *got = (size_t)csz;
    return GCE_OK;
}

}  // extern "C"
