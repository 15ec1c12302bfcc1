// gce_umi.hpp — the UMI of every record moved into the MI:Z field the engine reads (gce_bam_umi_to_mi).
//
// The engine finds a read's UMI as the reference does (src/bamutil.cpp:23-112): the last `:`-field of an MI:Z value or of the read name, A C G T
// and at most one `_`.  A file whose UMIs are in an RX:Z tag (fgbio, DRAGEN, `bwa mem -C`: ACGT-TTGA) or in an Illumina name (…:ACGT+TTGA) runs
// with every UMI empty.  This pass in front of the run gives every record with such a UMI an MI:Z field that parser accepts (bamutil.cpp:23-38
// is the contract); nothing of the run changes.  It is a record rewriter on a gce_sort object in calmd mode, streamed (rewrite_window,
// calmd_stream_room, gce_sort_calmd_consume of gce_calmd.hpp): nothing is sorted, the new records of every window go behind the resident
// output, whole members leave when the cap is reached.  Per window:
//   k_umi_size   one thread per record: the source string (rule S), is it a UMI (rule V), the walk of the optional fields (rule T, calmd's
//                field_bytes) for the MI fields to drop, the new size; the counters by ballot and one atomic per wave; the lowest malformed
//                record (atomicMin)
//   dev_exclusive_sum(size) -> the window's destinations behind the resident output
//   k_umi_tag    one thread per tagged record: M I Z : norm(s) NUL at the end of the new record (the `:` is what getUMI looks for)
//   k_umi_body   16 lanes per record: block_size rewritten, the core up to the end of QUAL and the kept stretches of optional fields
//                (calmd::copy_body over sort_copy16); an untouched record whole
// k_umi_size and k_umi_tag are one function, umi::umi_record<EMIT>: the size pass and the emit cannot disagree about a byte.  It and
// umi::copy_body are __host__ __device__: tests/umi_host_check.hip runs them on the host against tests/pyumi.py, the model of the rules.
// A record with more than two MI fields has more than three kept stretches: its kept fields are copied by umi_record<true> as it walks them.
#pragma once
#include <cstdint>
#include "gce_calmd.hpp"

namespace umi {

#define UM_HD __host__ __device__ inline

typedef uint32_t __attribute__((aligned(1), may_alias)) um_u32u;
typedef uint16_t __attribute__((aligned(1), may_alias)) um_u16u;

// what the size pass learns about a record (offsets count from the record's block_size).  size: the new record's bytes, block_size included
// (an untouched record's own).  core_end: the end of QUAL.  [d0a, d0z), [d1a, d1z): the first two dropped MI fields (the record's end where
// there is none); many: more than two were dropped.  [s_off, s_off + s_len): the source string.
struct Rec { uint32_t size, core_end, d0a, d0z, d1a, d1z, s_off, s_len; uint8_t bad, tagged, no_source, not_umi, many, mi_dropped; };
// Rec as k_umi_size leaves it for k_umi_tag and k_umi_body: 28 bytes per record, as calmd's; core: core_end | tagged << 31 | many << 30
struct Meta { uint32_t core, d0a, d0z, d1a, d1z, s_off, s_len; };
static_assert(sizeof(Meta) == sizeof(calmd::Meta), "40 bytes per window record, as calmd");
#define UM_MAX_LEN 250u
// the source of a run: 0 the read name, else the tag's two bytes, the first in the low byte
#define UM_SRC_NAME 0u

UM_HD bool is_sep(uint8_t c) { return c == '-' || c == '+' || c == '_'; }
UM_HD bool is_base(uint8_t c) { const uint8_t u = (uint8_t)(c & 0xDFu); return u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'N'; }
UM_HD uint8_t norm(uint8_t c) { return is_sep(c) ? (uint8_t)'_' : (uint8_t)(c & 0xDFu); }

// One record (r at its block_size, `avail` bytes from r to the end of the buffer).  EMIT == false: R is filled.  EMIT == true (tagged records
// only): R is the size pass's; the MI field is written at the end of the new record at `out` (and, R.many, the kept fields in front of it).
// No byte is read outside r[0, min(avail, 4 + block_size)); no byte is written outside out[R.core_end, R.size).
template <bool EMIT> UM_HD void umi_record(const uint8_t *r, uint64_t avail, uint32_t src, uint8_t *out, Rec &R) {
    const bool many_in = EMIT && R.many;
    if (!EMIT) { R.size = 0; R.core_end = 0; R.d0a = R.d0z = R.d1a = R.d1z = 0; R.s_off = 0; R.s_len = 0; R.bad = 0; R.tagged = 0; R.no_source = 0; R.not_umi = 0; R.many = 0; R.mi_dropped = 0; }
    if (avail < 4) { if (!EMIT) R.bad = 1; return; }
    const uint64_t bs = *(const um_u32u *)r;
    if (bs < 32 || 4 + bs > avail) { if (!EMIT) R.bad = 1; return; }
    const uint32_t old_size = (uint32_t)(4 + bs);
    if (!EMIT) { R.size = old_size; R.d0a = R.d0z = R.d1a = R.d1z = old_size; R.no_source = 1; }
    const uint8_t *c = r + 4, *end = c + bs;
    const int32_t lseq = (int32_t) * (const um_u32u *)(c + 16);
    const uint32_t lq = c[8], nc = *(const um_u16u *)(c + 12);
    if (lq < 1 || lseq < 0 || 32ull + lq + 4ull * nc + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > bs) return;     // (the record index accepts no such record)
    const uint8_t *ax = c + 32 + lq + 4 * nc + ((uint32_t)lseq + 1) / 2 + (uint32_t)lseq;
    const uint32_t core_end = (uint32_t)(ax - r);
    // ---- rule S, the name: up to its first NUL inside l_read_name, behind its last `:`
    uint32_t s_off = EMIT ? R.s_off : 0u, s_len = EMIT ? R.s_len : 0u;
    if (!EMIT && src == UM_SRC_NAME) {
        const uint8_t *nm = c + 32;
        uint32_t n = 0, colon = ~0u;
        while (n < lq && nm[n]) { if (nm[n] == ':') colon = n; n++; }
        if (colon != ~0u) { s_off = 36 + colon + 1; s_len = n - colon - 1; }
    }
    // ---- rule T: the optional fields tile [ax, end) exactly; every MI is dropped.  Rule S, a tag: its first field, if that is a Z
    uint32_t ndrop = 0, kept = 0; bool found = false;
    if (!EMIT || many_in)
        for (const uint8_t *p = ax; p < end;) {
            uint64_t fs;
            if (!calmd::field_bytes(p, end, fs)) { if (!EMIT) R.bad = 1; return; }
            if (p[0] == 'M' && p[1] == 'I') {
                if (!EMIT) {
                    const uint32_t a = (uint32_t)(p - r), z = (uint32_t)(a + 3 + fs);
                    if (ndrop == 0) { R.d0a = a; R.d0z = z; } else if (ndrop == 1) { R.d1a = a; R.d1z = z; }
                }
                ndrop++;
            } else {
                if (!EMIT && src != UM_SRC_NAME && !found && ((uint32_t)p[0] | (uint32_t)p[1] << 8) == src) {
                    found = true;
                    if (p[2] == 'Z') { s_off = (uint32_t)(p + 3 - r); s_len = (uint32_t)(fs - 1); }
                }
                if (EMIT) for (uint64_t k = 0; k < 3 + fs; k++) out[core_end + kept + k] = p[k];
                kept += (uint32_t)(3 + fs);
            }
            p += 3 + fs;
        }
    if (EMIT) {
        uint8_t *q = out + (R.size - (s_len + 5u));
        q[0] = 'M'; q[1] = 'I'; q[2] = 'Z'; q[3] = ':';
        for (uint32_t k = 0; k < s_len; k++) q[4 + k] = norm(r[s_off + k]);
        q[4 + s_len] = 0;
        return;
    }
    if (!s_len) return;                                                                 // no source: copied whole, its own MI fields with it
    R.no_source = 0;
    // ---- rule V
    bool ok = s_len <= UM_MAX_LEN; uint32_t nsep = 0;
    for (uint32_t k = 0; ok && k < s_len; k++) {
        const uint8_t b = r[s_off + k];
        if (is_sep(b)) { nsep++; if (k == 0 || k + 1 == s_len || nsep > 1) ok = false; }
        else if (!is_base(b)) ok = false;
    }
    if (!ok) { R.not_umi = 1; return; }
    const uint64_t new_bs = (uint64_t)(core_end - 4) + kept + s_len + 5;                // (M I Z : s NUL)
    if (new_bs > CM_MAX_BLOCK) { R.bad = 1; return; }                                   // (a record that would outgrow what the record index reads back)
    R.tagged = 1; R.core_end = core_end; R.many = ndrop > 2; R.mi_dropped = ndrop > 0; R.s_off = s_off; R.s_len = s_len; R.size = (uint32_t)(4 + new_bs);
}

UM_HD Meta pack(const Rec &R) { Meta M = {R.core_end | (uint32_t)R.tagged << 31 | (uint32_t)R.many << 30, R.d0a, R.d0z, R.d1a, R.d1z, R.s_off, R.s_len}; return M; }
UM_HD void unpack(const Meta &M, uint32_t size, Rec &R) {
    R.size = size; R.core_end = M.core & 0x3FFFFFFFu; R.tagged = (uint8_t)(M.core >> 31); R.many = (uint8_t)((M.core >> 30) & 1u); R.d0a = M.d0a; R.d0z = M.d0z; R.d1a = M.d1a; R.d1z = M.d1z;
    R.s_off = M.s_off; R.s_len = M.s_len; R.bad = 0; R.no_source = 0; R.not_umi = 0; R.mi_dropped = 0;
}

// What umi_record<true> does not write of the new record at d, by lane `sub` of the record's 16: calmd's body copy, with the MI fields as the
// dropped stretches; an untouched record (s, old_size bytes) whole.
__host__ __device__ __forceinline__ void copy_body(const uint8_t *s, uint32_t old_size, uint8_t *d, const Rec &R, uint32_t sub) {
    calmd::Rec C;
    C.size = R.size; C.core_end = R.core_end; C.d0a = R.d0a; C.d0z = R.d0z; C.d1a = R.d1a; C.d1z = R.d1z; C.elig = R.tagged; C.many = R.many;
    calmd::copy_body(s, old_size, d, C, sub);
}

#undef UM_HD

}  // namespace umi

#ifndef GCE_CALMD_HOST_CHECK

namespace {

// misc: [0] the lowest malformed record (atomicMin), [1] records given an MI, [2] without a source, [3] whose source is not a UMI, [4] that lost an MI field
__global__ __launch_bounds__(256) void k_umi_size(const uint8_t *u, const uint64_t *off, uint64_t n, uint64_t end, uint64_t gbase, uint32_t src, uint32_t *size, umi::Meta *meta,
                                                  unsigned long long *misc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    umi::Rec R; R.tagged = 0; R.no_source = 0; R.not_umi = 0; R.mi_dropped = 0;
    if (i < n) {
        const uint64_t a = off[i];
        umi::umi_record<false>(u + a, a < end ? end - a : 0, src, nullptr, R);
        size[i] = R.size; meta[i] = umi::pack(R);
        if (R.bad) atomicMin(misc, (unsigned long long)(gbase + i));
    }
    const unsigned long long bt = __ballot(R.tagged), bn = __ballot(R.no_source), bv = __ballot(R.not_umi), bd = __ballot(R.mi_dropped);
    if (lane_id() == 0) {
        if (bt) atomicAdd(misc + 1, (unsigned long long)__popcll(bt));
        if (bn) atomicAdd(misc + 2, (unsigned long long)__popcll(bn));
        if (bv) atomicAdd(misc + 3, (unsigned long long)__popcll(bv));
        if (bd) atomicAdd(misc + 4, (unsigned long long)__popcll(bd));
    }
}
// one thread per tagged record: its MI field at the end of the new record at out + dst[i]
__global__ __launch_bounds__(256) void k_umi_tag(const uint8_t *u, const uint64_t *off, uint64_t n, uint64_t end, uint32_t src, const uint32_t *size, const umi::Meta *meta, const uint64_t *dst,
                                                 uint8_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    umi::Rec R; umi::unpack(meta[i], size[i], R);
    if (!R.tagged) return;
    const uint64_t a = off[i];
    umi::umi_record<true>(u + a, end - a, src, out + dst[i], R);
}
// 16 lanes per record: everything else of the new record (umi::copy_body)
__global__ __launch_bounds__(256) void k_umi_body(const uint8_t *u, const uint64_t *off, uint64_t n, const uint32_t *size, const umi::Meta *meta, const uint64_t *dst, uint8_t *out) {
    const uint32_t sub = threadIdx.x & 15u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < n; j += ((uint64_t)gridDim.x * blockDim.x) >> 4) {
        const uint8_t *s = u + off[j];
        umi::Rec R; umi::unpack(meta[j], size[j], R);
        umi::copy_body(s, 4u + rb32(s), out + dst[j], R, sub);
    }
}

// the UMI pass as a record rewriter of rewrite_window (rules S, V, M, T)
struct UmiRW {
    gce_sort *b;
    size_t meta_bytes = sizeof(umi::Meta);
    const char *bad_fmt = "BAM record %llu (counting from 0): its optional fields do not tile its block_size, or its MI field would take it beyond 2^28 bytes";
    void size(unsigned nb, hipStream_t s, const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end, uint64_t gbase) const {
        hipLaunchKernelGGL(k_umi_size, dim3(nb), dim3(256), 0, s, u, off, n_rec, end, gbase, b->um_src, b->cm_size.as<uint32_t>(), b->cm_meta.as<umi::Meta>(), b->misc.as<unsigned long long>());
    }
    void emit(unsigned nb, hipStream_t s, const uint8_t *u, const uint64_t *off, uint64_t n_rec, uint64_t end, uint8_t *out) const {
        hipLaunchKernelGGL(k_umi_tag, dim3(nb), dim3(256), 0, s, u, off, n_rec, end, b->um_src, (const uint32_t *)b->cm_size.p, (const umi::Meta *)b->cm_meta.p, (const uint64_t *)b->cm_dst.p, out);
        hipLaunchKernelGGL(k_umi_body, dim3((unsigned)std::min<uint64_t>((n_rec + 15) / 16, 65535u)), dim3(256), 0, s, u, off, n_rec, (const uint32_t *)b->cm_size.p, (const umi::Meta *)b->cm_meta.p,
                           (const uint64_t *)b->cm_dst.p, out);
    }
};

}  // namespace

extern "C" {

// On a new object: the UMI pass, its output streamed as gce_sort_calmd_stream_begin sets it up (codes, piece_bytes, resident_bytes: as there).
// source: "name", or a two-character tag other than MI.
int gce_sort_umi_begin(gce_sort *b, int32_t codes, uint64_t piece_bytes, uint64_t resident_bytes, const char *source) {
    if (!b || !source || b->umi) return GCE_ERR_INVALID;
    uint32_t src;
    if (strcmp(source, "name") == 0) src = UM_SRC_NAME;
    else {
        const uint8_t a = (uint8_t)source[0], z = a ? (uint8_t)source[1] : 0;
        const bool al = (a >= 'A' && a <= 'Z') || (a >= 'a' && a <= 'z'), zl = (z >= 'A' && z <= 'Z') || (z >= 'a' && z <= 'z') || (z >= '0' && z <= '9');
        if (!al || !zl || source[2] || (a == 'M' && z == 'I')) return GCE_ERR_INVALID;
        src = (uint32_t)a | (uint32_t)z << 8;
    }
    const int rc = gce_sort_calmd_stream_begin(b, codes, piece_bytes, resident_bytes);
    if (rc != GCE_OK) return rc;
    b->calmd = true; b->umi = true; b->um_src = src;
    return GCE_OK;
}
// the next piece of the file, as gce_sort_calmd_stream_window takes it (flush and gce_sort_calmd_consume as there); *umi_s: the seconds of
// the k_umi_* kernels and their scan, added to.  GCE_ERR_INVALID names the lowest malformed record, counting from 0 over the file.
int gce_sort_umi_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, uint64_t est_bytes, double *umi_s, int (*flush)(void *ctx, uint64_t n), void *ctx) {
    if (!b || !b->umi || !b->cm_stream || !flush) return GCE_ERR_INVALID;
    UmiRW rw; rw.b = b;
    return rewrite_window(b, comp, comp_bytes, n_members, coff, csize, usize, skip, n_ref, last, est_bytes, umi_s, flush, ctx, rw);
}
// after the last window, as gce_sort_calmd_finish; counts: records, given an MI, without a source, not a UMI, that lost an MI field
int gce_sort_umi_finish(gce_sort *b, int32_t codes, uint64_t piece_bytes, int64_t counts[5], uint64_t *in_bytes, uint64_t *out_bytes) {
    if (!b || !b->umi || !counts || !in_bytes || !out_bytes || codes > 1) return GCE_ERR_INVALID;
    unsigned long long h[5];
    for (int k = 0; k < 5; k++) counts[k] = 0;
    const int rc = rewrite_finish(b, codes, piece_bytes, h, in_bytes, out_bytes);
    if (b->n) { counts[0] = (int64_t)b->n; for (int k = 1; k < 5; k++) counts[k] = (int64_t)h[k]; }
    return rc;
}

}  // extern "C"
#endif  // GCE_CALMD_HOST_CHECK
