// gce_calmd.hpp — NM and MD of every record recomputed against the reference on the GPU (gce_bam_calmd).
//
// Stands in for the `samtools calmd` a pipeline runs behind the reference program, whose consensus records keep the MD of one read of their
// cluster and an NM it patches only when stored as type C (src/group.cpp:531-570).  The file is streamed window by window as the sort streams
// it (win_inflate_index / win_carry, gce_passes.hpp) on a gce_sort object in calmd mode: nothing is sorted, the rewritten records of every
// window go straight behind the resident output, and gce_sort_read hands that stream out.  The reference goes up once: one blob of the contigs'
// ASCII bases and per tid (offset, length), length -1 for a contig the FASTA lacks.  Per window:
//   k_md_size   one thread per record: eligibility (rule E), the walk of the CIGAR over read and reference (rule W) for NM and the length of
//               MD, the walk of the optional fields (rule T) for the NM and MD fields to drop, the new size; the counters by ballot and one
//               atomic per wave; the lowest malformed record (atomicMin)
//   dev_exclusive_sum(size) -> the window's destinations behind the resident output
//   k_md_tags   one thread per eligible record: the NM and the MD field at their place in the new record
//   k_md_body   16 lanes per record: block_size rewritten, the core up to the end of QUAL and the kept stretches of optional fields
//               (sort_copy16, gce_copy16.hpp); an ineligible record whole
// k_md_size and k_md_tags are one function, calmd::md_record<EMIT>: the size pass and the emit cannot disagree about a byte.  It and
// calmd::copy_body are __host__ __device__: tests/calmd_host_check.hip runs them on the host against tests/pycalmd.py, the model of the rules.
// A record with more than two NM / MD fields has more than three kept stretches: its kept fields are copied by md_record<true> as it walks
// them, and copy_body leaves them alone.
// The window loop, the streamed output and the finish are written over "a record rewriter" (rewrite_window, rewrite_finish): calmd is one,
// the UMI pass of gce_umi.hpp the other, which also uses field_bytes (rule T's step) and copy_body.
#pragma once
#include <cstdint>
#include "gce_copy16.hpp"

namespace calmd {

#define CM_HD __host__ __device__ inline

typedef uint32_t __attribute__((aligned(1), may_alias)) cm_u32u;
typedef uint16_t __attribute__((aligned(1), may_alias)) cm_u16u;

// the reference on the device: contig tid = blob[tab[2 tid], + tab[2 tid + 1]), length -1 for a contig the FASTA lacks
struct Ref { const uint8_t *blob; const int64_t *tab; int32_t n_ref; };
// what the size pass learns about a record (offsets count from the record's block_size).  size: the new record's bytes, block_size included
// (an ineligible record's own).  core_end: the end of QUAL.  [d0a, d0z), [d1a, d1z): the first two dropped fields (the record's end where there
// is none); many: more than two were dropped.  The largest new block_size is 2^28, the largest the record index accepts.
struct Rec { uint32_t size, core_end, d0a, d0z, d1a, d1z, nm, md_len; uint8_t bad, elig, no_ref, many, nm_changed, md_changed; };
// Rec as k_md_size leaves it for k_md_tags and k_md_body: 28 bytes per record; core: core_end | elig << 31 | many << 30
struct Meta { uint32_t core, d0a, d0z, d1a, d1z, nm, md_len; };
#define CM_MAX_BLOCK (1u << 28)

// rule R: the 16-code of a reference byte (its index in "=ACMGRSVTWYHKDBN", 15 for any other byte) and the letter MD shows for it
CM_HD uint32_t code16(uint8_t b) {
    if (b == '=') return 0;
    const uint32_t k = (uint32_t)b - 'A';
    if (k >= 26) return 15;
    return (uint32_t)((k < 16 ? 0xFFF3FCFFB4FFD2E1ull >> (4 * k) : 0xFFFFFFFAF97F865Full >> (4 * (k - 16))) & 15u);
}
CM_HD uint8_t md_letter(uint8_t b) { return b >= 'A' && b <= 'Z' ? b : (uint8_t)'N'; }

// rule T, one step: the optional field at p (tag, type, value) inside [p, end), p < end.  fs: the bytes of its value (the field takes 3 + fs).
// false: fewer than 3 bytes are left, an unknown type or array subtype, a Z / H value without its NUL, or a value that passes `end`.
CM_HD bool field_bytes(const uint8_t *p, const uint8_t *end, uint64_t &fs) {
    if ((uint64_t)(end - p) < 3) return false;
    const uint8_t type = p[2]; const uint8_t *v = p + 3; const uint64_t left = (uint64_t)(end - v);
    if (type == 'A' || type == 'c' || type == 'C') fs = 1;
    else if (type == 's' || type == 'S') fs = 2;
    else if (type == 'i' || type == 'I' || type == 'f') fs = 4;
    else if (type == 'd') fs = 8;
    else if (type == 'Z' || type == 'H') { uint64_t n = 0; while (n < left && v[n]) n++; fs = n + 1; }               // (no NUL: n + 1 > left)
    else if (type == 'B') {
        if (left < 5) return false;
        const uint8_t sub = v[0]; const uint64_t cnt = *(const cm_u32u *)(v + 1);
        const uint32_t es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
        if (!es) return false;
        fs = 5 + es * cnt;
    }
    else return false;
    return fs <= left;
}

// One record (r at its block_size, `avail` bytes from r to the end of the buffer).  EMIT == false: R is filled.  EMIT == true: R is the size
// pass's; the NM field and the MD field are written at their place in the new record at `out` (and, R.many, the kept fields in front of
// them).  No byte is read outside r[0, min(avail, 4 + block_size)) and the contig's [0, length); no byte is written outside
// out[R.core_end, R.size).
template <bool EMIT> CM_HD void md_record(const uint8_t *r, uint64_t avail, const Ref &ref, uint8_t *out, Rec &R) {
    const uint32_t nm_in = EMIT ? R.nm : 0u; const bool many_in = EMIT && R.many;
    if (!EMIT) { R.size = 0; R.core_end = 0; R.d0a = R.d0z = R.d1a = R.d1z = 0; R.nm = 0; R.md_len = 0; R.bad = 0; R.elig = 0; R.no_ref = 0; R.many = 0; R.nm_changed = 0; R.md_changed = 0; }
    if (avail < 4) { if (!EMIT) R.bad = 1; return; }
    const uint64_t bs = *(const cm_u32u *)r;
    if (bs < 32 || 4 + bs > avail) { if (!EMIT) R.bad = 1; return; }
    const uint32_t old_size = (uint32_t)(4 + bs);
    if (!EMIT) { R.size = old_size; R.d0a = R.d0z = R.d1a = R.d1z = old_size; }
    const uint8_t *c = r + 4, *end = c + bs;
    // ---- rule E
    const int32_t tid = (int32_t) * (const cm_u32u *)(c + 0), pos = (int32_t) * (const cm_u32u *)(c + 4), lseq = (int32_t) * (const cm_u32u *)(c + 16);
    const uint32_t lq = c[8], nc = *(const cm_u16u *)(c + 12), flag = *(const cm_u16u *)(c + 14);
    if (lq < 1 || lseq < 0 || 32ull + lq + 4ull * nc + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > bs) return;     // (the record index accepts no such record)
    const uint8_t *cg = c + 32 + lq, *sq = cg + 4 * nc, *ax = sq + ((uint32_t)lseq + 1) / 2 + (uint32_t)lseq;
    const uint32_t core_end = (uint32_t)(ax - r);
    if ((flag & 4u) || tid < 0 || tid >= ref.n_ref || nc == 0 || lseq <= 0) return;
    {
        uint64_t qn = 0;
        for (uint32_t k = 0; k < nc; k++) {
            const uint32_t w = *(const cm_u32u *)(cg + 4 * k), op = w & 15u;
            if (op > 8) return;
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qn += w >> 4;
        }
        if (qn != (uint64_t)lseq) return;
    }
    const int64_t roff = ref.tab[2 * (int64_t)tid], rlen = ref.tab[2 * (int64_t)tid + 1];
    if (rlen < 0) { if (!EMIT) R.no_ref = 1; return; }
    // ---- rule T: the optional fields tile [ax, end) exactly; every NM and MD is dropped
    uint32_t ndrop = 0, kept = 0; bool has_nm = false, nm_int = false, has_md = false; int64_t nm_old = 0; const uint8_t *md_old = nullptr; uint64_t md_old_len = 0;
    for (const uint8_t *p = ax; p < end;) {
        uint64_t fs;
        if (!field_bytes(p, end, fs)) { if (!EMIT) R.bad = 1; return; }
        const uint8_t type = p[2]; const uint8_t *v = p + 3;
        const bool is_nm = p[0] == 'N' && p[1] == 'M', is_md = p[0] == 'M' && p[1] == 'D';
        if (is_nm || is_md) {
            if (!EMIT) {
                if (is_nm && !has_nm) {
                    has_nm = true; nm_int = true;
                    if (type == 'c') nm_old = (int8_t)v[0]; else if (type == 'C') nm_old = v[0];
                    else if (type == 's') nm_old = (int16_t) * (const cm_u16u *)v; else if (type == 'S') nm_old = *(const cm_u16u *)v;
                    else if (type == 'i') nm_old = (int32_t) * (const cm_u32u *)v; else if (type == 'I') nm_old = *(const cm_u32u *)v;
                    else nm_int = false;
                }
                if (is_md && !has_md) { has_md = true; if (type == 'Z') { md_old = v; md_old_len = fs - 1; } }
                const uint32_t a = (uint32_t)(p - r), z = (uint32_t)(a + 3 + fs);
                if (ndrop == 0) { R.d0a = a; R.d0z = z; } else if (ndrop == 1) { R.d1a = a; R.d1z = z; }
            }
            ndrop++;
        } else {
            if (EMIT && many_in) for (uint64_t k = 0; k < 3 + fs; k++) out[core_end + kept + k] = p[k];
            kept += (uint32_t)(3 + fs);
        }
        p = v + fs;
    }
    // ---- rule W
    const uint32_t o_nm = core_end + kept, w_nm = nm_in <= 255u ? 4u : nm_in <= 65535u ? 5u : 7u;
    uint8_t *md = EMIT ? out + o_nm + w_nm + 3 : nullptr;
    uint64_t m = 0, nm = 0; bool same = md_old != nullptr;
#define CM_P8(x) do { const uint8_t _b = (uint8_t)(x); if (EMIT) md[m] = _b; else if (same && (m >= md_old_len || md_old[m] != _b)) same = false; m++; } while (0)
#define CM_NUM(val) do { uint32_t _v = (val), _nd = 1; for (uint32_t _t = _v; _t >= 10; _t /= 10) _nd++; uint32_t _p = 1; for (uint32_t _k = 1; _k < _nd; _k++) _p *= 10; \
                         for (; _p; _p /= 10) { CM_P8('0' + _v / _p); _v %= _p; } } while (0)
    {
        int64_t x = pos; uint32_t y = 0, u = 0; bool stop = false;
        const uint8_t *rb = ref.blob + roff;
        for (uint32_t k = 0; k < nc && !stop; k++) {
            const uint32_t w = *(const cm_u32u *)(cg + 4 * k), op = w & 15u, len = w >> 4;
            if (op == 0 || op == 7 || op == 8) {
                for (uint32_t j = 0; j < len; j++) {
                    const int64_t xi = x + j;
                    if (xi < 0 || xi >= rlen) { stop = true; break; }
                    const uint32_t yi = y + j, c1 = (sq[yi >> 1] >> ((~yi & 1u) << 2)) & 15u;
                    const uint8_t b = rb[xi];
                    if (c1 == 0 || (c1 == code16(b) && c1 != 15)) u++;
                    else { CM_NUM(u); CM_P8(md_letter(b)); u = 0; nm++; }
                }
                x += len; y += len;
            } else if (op == 2) {
                const uint64_t cnt = x >= 0 && x < rlen ? ((uint64_t)(rlen - x) < len ? (uint64_t)(rlen - x) : len) : 0;
                if (!cnt) { stop = true; break; }                                       // (an ^ that no letter follows is not written)
                CM_NUM(u); CM_P8('^');
                for (uint64_t j = 0; j < cnt; j++) CM_P8(md_letter(rb[x + (int64_t)j]));
                nm += cnt; u = 0; x += len;
                if (cnt < len) stop = true;
            } else if (op == 1) { y += len; nm += len; }
            else if (op == 4) y += len;
            else if (op == 3) x += len;
        }
        CM_NUM(u);
    }
#undef CM_NUM
#undef CM_P8
    if (EMIT) {
        uint8_t *q = out + o_nm;
        q[0] = 'N'; q[1] = 'M';
        if (w_nm == 4) { q[2] = 'C'; q[3] = (uint8_t)nm_in; }
        else if (w_nm == 5) { q[2] = 'S'; q[3] = (uint8_t)nm_in; q[4] = (uint8_t)(nm_in >> 8); }
        else { q[2] = 'I'; q[3] = (uint8_t)nm_in; q[4] = (uint8_t)(nm_in >> 8); q[5] = (uint8_t)(nm_in >> 16); q[6] = (uint8_t)(nm_in >> 24); }
        q += w_nm; q[0] = 'M'; q[1] = 'D'; q[2] = 'Z'; q[3 + m] = 0;
        return;
    }
    const uint64_t new_bs = (uint64_t)(core_end - 4) + kept + (nm <= 255u ? 4u : nm <= 65535u ? 5u : 7u) + 4 + m;
    if (nm > 0xFFFFFFFFull || new_bs > CM_MAX_BLOCK) { R.bad = 1; return; }             // (a record that would outgrow what the record index reads back)
    R.elig = 1; R.core_end = core_end; R.many = ndrop > 2; R.nm = (uint32_t)nm; R.md_len = (uint32_t)m; R.size = (uint32_t)(4 + new_bs);
    R.nm_changed = !(has_nm && nm_int && nm_old == (int64_t)nm);
    R.md_changed = !(same && m == md_old_len);
}

CM_HD Meta pack(const Rec &R) { Meta M = {R.core_end | (uint32_t)R.elig << 31 | (uint32_t)R.many << 30, R.d0a, R.d0z, R.d1a, R.d1z, R.nm, R.md_len}; return M; }
CM_HD void unpack(const Meta &M, uint32_t size, Rec &R) {
    R.size = size; R.core_end = M.core & 0x3FFFFFFFu; R.elig = (uint8_t)(M.core >> 31); R.many = (uint8_t)((M.core >> 30) & 1u); R.d0a = M.d0a; R.d0z = M.d0z; R.d1a = M.d1a; R.d1z = M.d1z;
    R.nm = M.nm; R.md_len = M.md_len; R.bad = 0; R.no_ref = 0; R.nm_changed = 0; R.md_changed = 0;
}

// What md_record<true> does not write of the new record at d, by lane `sub` of the record's 16: block_size, the core up to the end of QUAL
// and the kept stretches of optional fields (R.many: md_record<true> copied those); an ineligible record (s, old_size bytes) whole.
__host__ __device__ __forceinline__ void copy_body(const uint8_t *s, uint32_t old_size, uint8_t *d, const Rec &R, uint32_t sub) {
    if (!R.elig) { sort_copy16(s, d, old_size, sub); return; }
    if (sub < 4) d[sub] = (uint8_t)((R.size - 4u) >> (8 * sub));
    sort_copy16(s + 4, d + 4, R.core_end - 4, sub);
    if (R.many) return;
    uint32_t o = R.core_end;
    sort_copy16(s + R.core_end, d + o, R.d0a - R.core_end, sub); o += R.d0a - R.core_end;
    sort_copy16(s + R.d0z, d + o, R.d1a - R.d0z, sub); o += R.d1a - R.d0z;
    sort_copy16(s + R.d1z, d + o, old_size - R.d1z, sub);
}

#undef CM_HD

}  // namespace calmd

#ifndef GCE_CALMD_HOST_CHECK

namespace {

// misc: [0] the lowest malformed record (atomicMin), [1] rewritten records, [2] records whose contig the FASTA lacks, [3] NM changed, [4] MD changed
__global__ __launch_bounds__(256) void k_md_size(const uint8_t *u, const uint64_t *off, uint64_t n, uint64_t end, uint64_t gbase, calmd::Ref ref, uint32_t *size, calmd::Meta *meta,
                                                 unsigned long long *misc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    calmd::Rec R; R.elig = 0; R.no_ref = 0; R.nm_changed = 0; R.md_changed = 0;
    if (i < n) {
        const uint64_t a = off[i];
        calmd::md_record<false>(u + a, a < end ? end - a : 0, ref, nullptr, R);
        size[i] = R.size; meta[i] = calmd::pack(R);
        if (R.bad) atomicMin(misc, (unsigned long long)(gbase + i));
    }
    const unsigned long long be = __ballot(R.elig), br = __ballot(R.no_ref), bn = __ballot(R.nm_changed), bm = __ballot(R.md_changed);
    if (lane_id() == 0) {
        if (be) atomicAdd(misc + 1, (unsigned long long)__popcll(be));
        if (br) atomicAdd(misc + 2, (unsigned long long)__popcll(br));
        if (bn) atomicAdd(misc + 3, (unsigned long long)__popcll(bn));
        if (bm) atomicAdd(misc + 4, (unsigned long long)__popcll(bm));
    }
}
// one thread per eligible record: its NM and MD fields at out + dst[i]
__global__ __launch_bounds__(256) void k_md_tags(const uint8_t *u, const uint64_t *off, uint64_t n, uint64_t end, calmd::Ref ref, const uint32_t *size, const calmd::Meta *meta, const uint64_t *dst,
                                                 uint8_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    calmd::Rec R; calmd::unpack(meta[i], size[i], R);
    if (!R.elig) return;
    const uint64_t a = off[i];
    calmd::md_record<true>(u + a, end - a, ref, out + dst[i], R);
}
// 16 lanes per record: everything else of the new record (calmd::copy_body)
__global__ __launch_bounds__(256) void k_md_body(const uint8_t *u, const uint64_t *off, uint64_t n, const uint32_t *size, const calmd::Meta *meta, const uint64_t *dst, uint8_t *out) {
    const uint32_t sub = threadIdx.x & 15u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < n; j += ((uint64_t)gridDim.x * blockDim.x) >> 4) {
        const uint8_t *s = u + off[j];
        calmd::Rec R; calmd::unpack(meta[j], size[j], R);
        calmd::copy_body(s, 4u + rb32(s), out + dst[j], R, sub);
    }
}

static int calmd_counters_init(gce_sort *b) {
    if (b->misc.p) return GCE_OK;
    if (!sort_room(b, 512)) return sort_oom(b, "calmd's counters", 512);
    SCHK(b->misc.ensure(64));
    const unsigned long long init[5] = {~0ull, 0ull, 0ull, 0ull, 0ull};
    SCHK(hipMemcpyAsync(b->misc.p, init, sizeof init, hipMemcpyHostToDevice, b->s)); SCHK(hipStreamSynchronize(b->s));
    return GCE_OK;
}

// ---- the output streamed (gce_bam_calmd_stream): the resident output is capped, whole members of 0xff00 bytes leave before the last window
// flush(ctx, n): the caller writes the first n resident bytes (gce_sort_read) and lets them go (gce_sort_calmd_consume)
typedef int (*calmd_flush_fn)(void *ctx, uint64_t n);

// the deflate buffers of the largest piece of the first n resident bytes, before they are first needed (gce_sort_read makes none).  Buffers
// that suffice stay; others are let go before the budget is asked, so that they are not counted beside their successors.  ahead: size them
// for a piece of the cap as well, so that later flushes find them made.
static int calmd_stream_zbufs(gce_sort *b, uint64_t n, bool ahead) {
    if (b->cm_codes < 0 || !b->cm_piece || !n) return GCE_OK;
    const uint64_t need = (std::min<uint64_t>(b->cm_piece, n) + 0xff00u - 1) / 0xff00u;
    if (need * sort_slot() + 64 <= b->zs.cap && need * sort_slot() + 64 <= b->zo.cap && (need + 1) * 4 <= b->zz.cap && (need + 1) * 8 <= b->zf.cap) return GCE_OK;
    for (DevBuf *x : {&b->zs, &b->zz, &b->zf, &b->zo}) x->release();
    return sort_deflate_bufs(b, std::min<uint64_t>(b->cm_piece, ahead ? std::max<uint64_t>(n, b->cm_cap) : n));
}
// room for a window's wtotal output bytes behind the resident ones, `target` the size a new buffer should have: the cap R is derived from the
// budget on first use; when the window would pass it (or the buffer cannot grow within the budget) the whole members resident so far are
// flushed and the tail below 0xff00 bytes moves to the front.  One window's output always fits beside the tail, or GCE_ERR_OOM.
static int calmd_stream_room(gce_sort *b, uint64_t wtotal, uint64_t target, calmd_flush_fn flush, void *ctx) {
    const uint64_t M = 0xff00u, slack = 65536;                                        // (slack: the scans' scratch, allocator rounding)
    hipStream_t s = b->s;
    if (!b->cm_cap) {                                                                 // what the budget leaves now, beside the deflate buffers of one piece
        // (held back: as much again as the window holds, for a later window that inflates to more and has to grow)
        const uint64_t live = (uint64_t)std::max<long long>(__atomic_load_n(&g_dev_live, __ATOMIC_RELAXED), 0) + sort_win_need(b->w, b->tmp) + slack;
        const uint64_t avail = b->budget > live ? b->budget - live : 0;
        uint64_t R = avail;
        if (b->cm_codes >= 0 && b->cm_piece) { const uint64_t dp = sort_deflate_need(b->cm_piece / M); R = avail > dp + b->cm_piece ? avail - dp : avail / 18 * 5; }
        b->cm_cap = b->budget ? std::max<uint64_t>(R / M * M, M) : ~0ull / M * M;
    }
    auto want_of = [&]() { return std::max<uint64_t>(b->out_n + wtotal + 64, std::min<uint64_t>(target, b->cm_cap + 64)) + 256; };
    auto grows = [&]() { return !(b->out_n + wtotal + 64 <= b->out.cap && b->out.p); };
    if (b->out_n >= M && flush && (b->out_n + wtotal > b->cm_cap || (grows() && !sort_room(b, want_of())))) {
        const uint64_t n = b->out_n / M * M;
        int rc;
        if ((rc = calmd_stream_zbufs(b, n, true)) != GCE_OK || (rc = flush(ctx, n)) != GCE_OK) return rc;
        if (b->out_n >= M) return sfail(b, GCE_ERR_INVALID, "calmd: the flushed bytes were not consumed");
    }
    if (!grows()) return GCE_OK;
    const uint64_t want = want_of();
    if (b->out.p && b->out_n < M && !sort_room(b, want)) {
        // the old buffer and the new one do not fit side by side: the tail waits in host memory while the buffer is made anew
        std::vector<uint8_t> tail((size_t)b->out_n);
        if (b->out_n) { SCHK(hipMemcpyAsync(tail.data(), b->out.p, (size_t)b->out_n, hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s)); }
        b->out.release();
        if (!sort_room(b, want)) return sort_oom(b, "one window's output record bytes", want);
        const int rc = sort_grow(b, b->out, (size_t)(b->out_n + wtotal + 64), 0, (size_t)(want - 256), "one window's output record bytes");
        if (rc != GCE_OK) return rc;
        if (b->out_n) { SCHK(hipMemcpyAsync(b->out.p, tail.data(), (size_t)b->out_n, hipMemcpyHostToDevice, s)); SCHK(hipStreamSynchronize(s)); }
        return GCE_OK;
    }
    return sort_grow(b, b->out, (size_t)(b->out_n + wtotal + 64), (size_t)b->out_n, (size_t)(want - 256), "the output record bytes");
}

// calmd::Ref on the host and its way to the device, shared with the error profile (gce_errprof.hpp).  tab: per contig the offset of its bases
// in the blob and their length, -1 for a contig the FASTA lacks (seq[t] NULL or len[t] < 0); -> the blob's bytes
static uint64_t calmd_ref_layout(int32_t n_ref, const char *const *seq, const int64_t *len, std::vector<int64_t> &tab) {
    tab.assign((size_t)n_ref * 2 + 2, 0);
    uint64_t total = 0;
    for (int32_t t = 0; t < n_ref; t++) {
        const bool have = seq[t] && len[t] >= 0;
        tab[2 * (size_t)t] = (int64_t)total; tab[2 * (size_t)t + 1] = have ? len[t] : -1;
        if (have) total += (uint64_t)len[t];
    }
    return total;
}
static hipError_t calmd_ref_upload(DevBuf &blob, DevBuf &dtab, int32_t n_ref, const char *const *seq, const int64_t *len, const std::vector<int64_t> &tab, uint64_t total, hipStream_t s) {
    hipError_t e;
    if ((e = blob.ensure(total + 64)) != hipSuccess || (e = dtab.ensure(tab.size() * 8)) != hipSuccess) return e;
    for (int32_t t = 0; t < n_ref; t++)
        if (tab[2 * (size_t)t + 1] > 0 && (e = hipMemcpyAsync(blob.as<uint8_t>() + tab[2 * (size_t)t], seq[t], (size_t)len[t], hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(dtab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

}  // namespace

extern "C" {

// the reference of a calmd run, once, in front of the first window: seq[t] / len[t] the ASCII bases of the header's contig t as gce_fasta_load
// returns them (NULL / -1: the FASTA has no contig of that name).  Puts the object into calmd mode.
int gce_sort_calmd_ref(gce_sort *b, int32_t n_ref, const char *const *seq, const int64_t *len) {
    if (!b || n_ref < 0 || (n_ref && (!seq || !len)) || b->n || b->passes || b->sam_text || b->cm_tab.p) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    b->calmd = true;
    std::vector<int64_t> tab;
    const uint64_t total = calmd_ref_layout(n_ref, seq, len, tab);
    const uint64_t want = DevBuf::padded(total + 64) + DevBuf::padded(tab.size() * 8);
    if (!sort_room(b, want)) return sort_oom(b, "the reference bases", want);
    SCHK(calmd_ref_upload(b->cm_blob, b->cm_tab, n_ref, seq, len, tab, total, b->s));
    return GCE_OK;
}

}  // extern "C"

// A window of a gce_sort object in calmd mode under a record rewriter RW (calmd's own below, the UMI pass of gce_umi.hpp): the next piece of
// the file, as gce_sort_window takes it; its whole records are rewritten behind the resident output.  RW gives
//   meta_bytes          the bytes per record that its size pass leaves for its emit in cm_meta (cm_size and cm_dst are the window's)
//   size(nb, ...)       launches the size pass: cm_size[i], cm_meta[i], misc[0] the lowest malformed record (atomicMin), misc[1..4] its counters
//   emit(nb, ..., out)  launches what writes the new records at out + cm_dst[i]
//   bad_fmt             the message for the lowest malformed record (one %llu)
// est_bytes: the caller's estimate of the file's inflated bytes; *calmd_s: the seconds of the rewriter's kernels and their scan, added to.
// GCE_ERR_INVALID names the lowest malformed record, counting from 0 over the file.
template <class RW> static int rewrite_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                                              int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s, calmd_flush_fn flush, void *ctx, const RW &rw) {
    if (!b || !b->calmd || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize))) return GCE_ERR_INVALID;
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    int rc;
    if ((rc = sort_win_check(b, comp_bytes, n_members, usize)) != GCE_OK || (rc = calmd_counters_init(b)) != GCE_OK) return rc;
    uint64_t total = 0, n_rec = 0, end = 0;
    rc = win_inflate_index(b->w, b->tmp, s, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, nullptr, &total, &n_rec, &end, b->err);
    if (rc == GCE_ERR_OOM) return sort_oom(b, "a window of the file", 0);
    if (rc != GCE_OK) return rc;
    if (n_rec) {
        if (b->n + n_rec >= SORT_MAX_RECORDS) return sfail(b, GCE_ERR_INVALID, "more than 2^32 - 16 records in one BAM file");
        const double t0 = mono_s();
        {   // 40 bytes per window record: size, description, destination
            uint64_t add = 0;
            if (n_rec * 4 > b->cm_size.cap) add += DevBuf::padded(n_rec * 4);
            if (n_rec * rw.meta_bytes > b->cm_meta.cap) add += DevBuf::padded(n_rec * rw.meta_bytes);
            if ((n_rec + 1) * 8 > b->cm_dst.cap) add += DevBuf::padded((n_rec + 1) * 8);
            if (add && !sort_room(b, add)) return sort_oom(b, "the sizes and destinations of a window's records", add);
            SCHK(b->cm_size.ensure(n_rec * 4)); SCHK(b->cm_meta.ensure(n_rec * rw.meta_bytes)); SCHK(b->cm_dst.ensure((n_rec + 1) * 8));
        }
        const uint8_t *u = (const uint8_t *)b->w.win.p; const uint64_t *off = (const uint64_t *)b->w.idx.off.p;
        const unsigned nb = (unsigned)((n_rec + 255) / 256);
        rw.size(nb, s, u, off, n_rec, end, b->n);
        SCHK(hipGetLastError());
        SCHK(dev_exclusive_sum((const uint32_t *)b->cm_size.p, n_rec, b->cm_dst.as<uint64_t>(), b->tmp, s));
        uint64_t wtotal = 0; unsigned long long bad = ~0ull;
        SCHK(hipMemcpyAsync(&wtotal, b->cm_dst.as<uint64_t>() + n_rec, 8, hipMemcpyDeviceToHost, s)); SCHK(hipMemcpyAsync(&bad, b->misc.p, 8, hipMemcpyDeviceToHost, s));
        SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
        if (bad != ~0ull) {
            char m[256]; snprintf(m, sizeof m, rw.bad_fmt, bad);
            return sfail(b, GCE_ERR_INVALID, m);
        }
        const uint64_t start = std::min<uint64_t>(skip, total), in1 = b->cm_in + (end - start), seen = b->cm_flushed + b->out_n + wtotal;
        const uint64_t eo = (uint64_t)((double)std::max<uint64_t>(est_bytes, in1) * ((double)seen / (double)in1));    // the file's output bytes at the growth seen so far
        double fl = 0;
        if (b->cm_stream) {                                                           // (a flush is the caller's write_s, not calmd_s)
            const double f0 = mono_s();
            if ((rc = calmd_stream_room(b, wtotal, eo + eo / 16 + 64, flush, ctx)) != GCE_OK) return rc;
            fl = mono_s() - f0;
        }
        const uint64_t have = b->out_n + wtotal;
        if ((rc = sort_grow(b, b->out, (size_t)(have + 64), (size_t)b->out_n, (size_t)(eo + eo / 16 + 64), "the output record bytes")) != GCE_OK) return rc;
        uint8_t *out = b->out.as<uint8_t>() + b->out_n;
        rw.emit(nb, s, u, off, n_rec, end, out);
        SCHK(hipGetLastError()); SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
        b->out_n = have; b->n += n_rec; b->cm_in = in1;
        if (calmd_s) *calmd_s += mono_s() - t0 - fl;
    }
    rc = win_carry(b->w, s, total, end, b->err);
    b->win_need = std::max(b->win_need, sort_win_need(b->w, b->tmp));
    return rc;
}

// calmd's own rewriter (rules E, W, T): k_md_size, then k_md_tags and k_md_body
struct CalmdRW {
    gce_sort *b; calmd::Ref ref;
    size_t meta_bytes = sizeof(calmd::Meta);
    const char *bad_fmt = "BAM record %llu (counting from 0): its optional fields do not tile its block_size, or its new MD would take it beyond 2^28 bytes";
    void size(unsigned nb, hipStream_t s, const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end, uint64_t gbase) const {
        hipLaunchKernelGGL(k_md_size, dim3(nb), dim3(256), 0, s, u, off, n_rec, end, gbase, ref, b->cm_size.as<uint32_t>(), b->cm_meta.as<calmd::Meta>(), b->misc.as<unsigned long long>());
    }
    void emit(unsigned nb, hipStream_t s, const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end, uint8_t *out) const {
        hipLaunchKernelGGL(k_md_tags, dim3(nb), dim3(256), 0, s, u, off, n_rec, end, ref, (const uint32_t *)b->cm_size.p, (const calmd::Meta *)b->cm_meta.p, (const uint64_t *)b->cm_dst.p, out);
        hipLaunchKernelGGL(k_md_body, dim3((unsigned)std::min<uint64_t>((n_rec + 15) / 16, 65535u)), dim3(256), 0, s, u, off, n_rec, (const uint32_t *)b->cm_size.p, (const calmd::Meta *)b->cm_meta.p,
                           (const uint64_t *)b->cm_dst.p, out);
    }
};
static int calmd_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s, calmd_flush_fn flush, void *ctx) {
    if (!b || !b->calmd || !b->cm_tab.p) return GCE_ERR_INVALID;
    CalmdRW rw; rw.b = b; rw.ref = {b->cm_blob.as<uint8_t>(), b->cm_tab.as<int64_t>(), n_ref};
    return rewrite_window(b, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, est_bytes, calmd_s, flush, ctx, rw);
}

extern "C" {

int gce_sort_calmd_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                          int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s) {
    if (b && b->cm_stream) return GCE_ERR_INVALID;
    return calmd_window(b, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, est_bytes, calmd_s, nullptr, nullptr);
}

// ---- the output streamed (gce_bam_calmd_stream).  On a new object, before gce_sort_calmd_ref: the object caps its resident output
// at resident_bytes (a multiple of 0xff00; 0: what the budget leaves beside the reference bases + one window + 40 bytes per window record +
// one piece's deflate buffers, found when the first window's records are known).  codes / piece_bytes: as gce_sort_calmd_finish takes them.
int gce_sort_calmd_stream_begin(gce_sort *b, int32_t codes, uint64_t piece_bytes, uint64_t resident_bytes) {
    if (!b || b->calmd || b->cm_stream || b->passes || b->sam_text || b->n || b->out_n || codes > 1 || resident_bytes % 0xff00u || piece_bytes % 0xff00u) return GCE_ERR_INVALID;
    b->cm_stream = true; b->cm_codes = codes; b->cm_piece = piece_bytes; b->cm_cap = resident_bytes;
    return GCE_OK;
}
// gce_sort_calmd_window with the cap: when the window's output would pass it, flush(ctx, n) is called once, before the window's records are
// emitted, with n = floor(resident bytes / 0xff00) * 0xff00 > 0: the caller reads [0, n) with gce_sort_read (the deflate buffers exist) and
// then calls gce_sort_calmd_consume(b, n); what it returns other than GCE_OK ends the window.
int gce_sort_calmd_stream_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                                 int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s, int (*flush)(void *ctx, uint64_t n), void *ctx) {
    if (!b || !b->cm_stream || !flush) return GCE_ERR_INVALID;
    return calmd_window(b, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, est_bytes, calmd_s, flush, ctx);
}
// the first n bytes of the resident output are let go and the tail moves to the front.  n: a multiple of 0xff00 and at least the tail's
// length, so that source and destination do not overlap: one device-to-device copy on the object's stream does it.
int gce_sort_calmd_consume(gce_sort *b, uint64_t n) {
    if (!b || !b->cm_stream || n % 0xff00u || n > b->out_n || (n && b->out_n - n > n)) return GCE_ERR_INVALID;
    if (!n) return GCE_OK;
    (void)hipSetDevice(b->device);
    const uint64_t tail = b->out_n - n;
    if (tail) SCHK(hipMemcpyAsync(b->out.p, b->out.as<uint8_t>() + n, (size_t)tail, hipMemcpyDeviceToDevice, b->s));
    SCHK(hipStreamSynchronize(b->s)); SCHK(hipGetLastError());
    b->out_n = tail; b->cm_flushes++; b->cm_flushed += n;
    return GCE_OK;
}
// what a streamed run did so far: the flushes, the cap (0: no window had records yet and none was given), the bytes flushed
int gce_sort_calmd_stream_stats(gce_sort *b, int32_t *n_flushes, uint64_t *resident_cap_bytes, uint64_t *flushed_bytes) {
    if (!b || !b->cm_stream || !n_flushes || !resident_cap_bytes || !flushed_bytes) return GCE_ERR_INVALID;
    *n_flushes = b->cm_flushes; *resident_cap_bytes = b->cm_cap; *flushed_bytes = b->cm_flushed;
    return GCE_OK;
}

// after the last window: the window, the reference and the descriptions are let go; counts: records, rewritten, unchanged, contig missing,
// NM changed, MD changed; *out_bytes: the output stream's bytes, which gce_sort_read hands out.  codes >= 0: the buffers gce_sort_read
// deflates pieces of up to piece_bytes with are made here, so that running out of device memory is known before the caller opens its output.
// h: the rewriter's misc[0..4] as its size pass left them (zeros for a file without records)
static int rewrite_finish(gce_sort *b, int32_t codes, uint64_t piece_bytes, unsigned long long h[5], uint64_t *in_bytes, uint64_t *out_bytes) {
    (void)hipSetDevice(b->device);
    hipStream_t s = b->s;
    SCHK(hipStreamSynchronize(s));
    b->w.release();
    for (DevBuf *x : {&b->cm_blob, &b->cm_tab, &b->cm_size, &b->cm_meta, &b->cm_dst}) x->release();
    for (int k = 0; k < 5; k++) h[k] = 0;
    *in_bytes = b->cm_in; *out_bytes = b->out_n;
    if (b->n == 0) return GCE_OK;
    SCHK(hipMemcpyAsync(h, b->misc.p, 5 * sizeof h[0], hipMemcpyDeviceToHost, s)); SCHK(hipStreamSynchronize(s)); SCHK(hipGetLastError());
    SCHK(hipMemsetAsync(b->out.as<uint8_t>() + b->out_n, 0, 64, s));                  // (the deflate kernels may look a few bytes ahead)
    SCHK(hipStreamSynchronize(s));
    if (b->cm_stream) return calmd_stream_zbufs(b, b->out_n, false);                  // (the buffers of the flushes are live: not counted twice)
    if (codes >= 0 && piece_bytes) return sort_deflate_bufs(b, std::min<uint64_t>(piece_bytes, b->out_n));
    return GCE_OK;
}
int gce_sort_calmd_finish(gce_sort *b, int32_t codes, uint64_t piece_bytes, int64_t counts[6], uint64_t *in_bytes, uint64_t *out_bytes) {
    if (!b || !b->calmd || !counts || !in_bytes || !out_bytes || codes > 1) return GCE_ERR_INVALID;
    unsigned long long h[5];
    for (int k = 0; k < 6; k++) counts[k] = 0;
    const int rc = rewrite_finish(b, codes, piece_bytes, h, in_bytes, out_bytes);
    if (b->n) { counts[0] = (int64_t)b->n; counts[1] = (int64_t)h[1]; counts[2] = (int64_t)(b->n - h[1]); counts[3] = (int64_t)h[2]; counts[4] = (int64_t)h[3]; counts[5] = (int64_t)h[4]; }
    return rc;
}

}  // extern "C"
#endif  // GCE_CALMD_HOST_CHECK
