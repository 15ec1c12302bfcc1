// gce_samfmt.hpp — BAM records into SAM text lines on the GPU (gce_sam_format, gce_raw_format_output).
//
// Replaces what the reference gets from htslib's sam_write1 / sam_format1 when its output name ends in "sam" (sam_open(out, "w"),
// src/gencore.cpp:170-173,104), which this tree had on host threads only (samtext::bam_to_line, gce_samtext.hpp: the specification of every
// byte written here and of every record refused).  The inverse of gce_samdev.hpp, in its shape.  The records lie back to back in HBM with
// their starts (the output stream's record offsets, or a walk of the block sizes); the contig names go up once as a blob with offsets in
// header order, so `tid` indexes them.  Per stream:
//   k_samfmt_size     one thread per record: the sanity test, every refusal of bam_to_line, the length of the line (64 bits: a B array may
//                     hold 2^32 - 1 elements), where SEQ starts in the line, whether the record holds a floating-point value; the lowest
//                     refused record (atomicMin)
//   dev_select_flagged -> the records with floating-point values (the host records), in order
//   k_samfmt_hostmeta, k_samfmt_gather, k_samfmt_hostsize   those records only: their bytes to the host in one staged copy, the lengths of
//                     the host's lines into the size array
//   dev_exclusive_sum(size) -> the line starts, the text's size
//   k_samfmt_core     one thread per record: every byte of the line except SEQ and QUAL where they are not `*`
//   k_samfmt_seq      16 lanes per record: nibble -> "=ACMGRSVTWYHKDBN" (the table in LDS) and quality + 33, 16-byte stores aligned on the
//                     DESTINATION, the bytes in front of the first boundary and behind the last whole chunk as single bytes (as sort_copy16)
//   k_samfmt_patch    one wave per host record: the host's line, staged in one buffer, into its place
// k_samfmt_size and k_samfmt_core are one function, samfmt::format_record<EMIT>: the size pass and the emit pass cannot disagree about a
// byte.  It, samfmt::emit_seq and samfmt::walk_records are __host__ __device__: tests/samfmt_host_check.hip runs them on the host against
// bam_to_line, one lane and 16 lanes standing in for the group.
// Floating point: `f`, `d` and `B:f` values are printed with %g, which the device does not have.  The size pass walks such a record to its
// end (its refusals are still the device's) and lists it; the host formats the listed records with bam_to_line on one thread before the
// scan.  No other record reaches the host formatter.
#pragma once
#include <cstdint>

namespace samfmt {

#define SF_HD __host__ __device__ inline

// the contig names in header order: name k = blob[off[k], off[k + 1])
struct Names { const uint8_t *blob; const uint32_t *off; int32_t n; };
// what the size pass learns about a record.  oseq: where SEQ starts in the line (the QUAL field starts lseq + 1 bytes behind it)
struct Rec { uint64_t size; uint32_t bad, host, oseq, lseq; };

typedef uint32_t __attribute__((aligned(1), may_alias)) sf_u32u;
typedef uint16_t __attribute__((aligned(1), may_alias)) sf_u16u;

// The block sizes of records[0, n) followed from the first byte: start[k] = the k-th record's first byte for k < cap, start[nr] = the byte
// behind the last good one (when nr <= cap).  bad: -1, or the index of the record whose block_size is below 32, is cut by the end of the
// buffer or runs past it; the walk stops there.  start may be NULL (count only).
SF_HD void walk_records(const uint8_t *p, uint64_t n, uint64_t *start, uint64_t cap, uint64_t &nr, int64_t &bad) {
    uint64_t o = 0, k = 0; bad = -1;
    while (o < n) {
        if (n - o < 4) { bad = (int64_t)k; break; }
        const uint64_t bs = *(const sf_u32u *)(p + o);
        if (bs < 32 || 4 + bs > n - o) { bad = (int64_t)k; break; }
        if (start && k < cap) start[k] = o;
        k++; o += 4 + bs;
    }
    if (start && k <= cap) start[k] = o;
    nr = k;
}

#define SF_P8(x) do { if (EMIT) out[o] = (uint8_t)(x); o++; } while (0)
// a decimal number: every value a record holds fits 32 bits of magnitude ((int64)INT32_MAX + 1 and -(int64)INT32_MIN are 2^31)
template <bool EMIT> SF_HD void put_num(uint8_t *out, uint64_t &o, bool neg, uint32_t mag) {
    if (neg) SF_P8('-');
    uint32_t nd = 1; for (uint32_t v = mag; v >= 10; v /= 10) nd++;
    if (EMIT) { uint32_t v = mag; for (uint32_t k = nd; k-- > 0;) { out[o + k] = (uint8_t)('0' + v % 10); v /= 10; } }
    o += nd;
}
template <bool EMIT> SF_HD void put_i64(uint8_t *out, uint64_t &o, int64_t x) { put_num<EMIT>(out, o, x < 0, (uint32_t)(x < 0 ? -x : x)); }
template <bool EMIT> SF_HD void put_name(uint8_t *out, uint64_t &o, const Names &nm, int32_t t) {          // `*` for a tid the table does not have
    if (t < 0 || t >= nm.n) { SF_P8('*'); return; }
    const uint32_t a = nm.off[t], z = nm.off[t + 1];
    if (EMIT) for (uint32_t k = a; k < z; k++) out[o + (k - a)] = nm.blob[k];
    o += z - a;
}

// One record (r at its block_size, `avail` bytes from r to the end of the buffer): bam_to_line's refusals (R.bad), the length of its line
// with the line feed (R.size) and -- EMIT -- every byte of the line at `out` except the characters of SEQ and QUAL (emit_seq; a `*` in
// their place is written here).  A floating-point value prints nothing and sets R.host: such a record's line is the host's.  No byte is
// read outside r[0, min(avail, 4 + block_size)).
template <bool EMIT> SF_HD void format_record(const uint8_t *r, uint64_t avail, const Names &nm, uint8_t *out, Rec &R) {
    R.size = 0; R.bad = 1; R.host = 0; R.oseq = 0; R.lseq = 0;
    if (avail < 4) return;
    const uint64_t bs = *(const sf_u32u *)r;
    if (bs < 32 || 4 + bs > avail) return;
    const uint8_t *c = r + 4, *end = c + bs;
    const int32_t tid = (int32_t) * (const sf_u32u *)(c + 0), pos = (int32_t) * (const sf_u32u *)(c + 4), lseq = (int32_t) * (const sf_u32u *)(c + 16), mtid = (int32_t) * (const sf_u32u *)(c + 20),
                  mpos = (int32_t) * (const sf_u32u *)(c + 24), tlen = (int32_t) * (const sf_u32u *)(c + 28);
    const uint32_t lq = c[8], mapq = c[9], nc = *(const sf_u16u *)(c + 12), flag = *(const sf_u16u *)(c + 14);
    if (lq < 1 || lseq < 0 || 32ull + lq + 4ull * nc + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > bs) return;
    const uint8_t *qn = c + 32, *cg = qn + lq, *sq = cg + 4 * nc, *ql = sq + ((uint32_t)lseq + 1) / 2, *ax = ql + lseq;
    uint64_t o = 0;
    {   // QNAME: strnlen -- an embedded NUL cuts it, a missing NUL does not overrun
        uint32_t n = 0; while (n < lq && qn[n]) n++;
        if (EMIT) for (uint32_t k = 0; k < n; k++) out[k] = qn[k];
        o += n;
    }
    SF_P8('\t'); put_num<EMIT>(out, o, false, flag); SF_P8('\t');
    put_name<EMIT>(out, o, nm, tid);
    SF_P8('\t'); put_i64<EMIT>(out, o, (int64_t)pos + 1); SF_P8('\t'); put_num<EMIT>(out, o, false, mapq); SF_P8('\t');
    if (nc == 0) SF_P8('*');
    else for (uint32_t k = 0; k < nc; k++) {
        const uint32_t w = *(const sf_u32u *)(cg + 4 * k), op = w & 15u;
        put_num<EMIT>(out, o, false, w >> 4); SF_P8(op < 9 ? "MIDNSHP=X"[op] : '?');
    }
    SF_P8('\t');
    if (mtid < 0) SF_P8('*'); else if (mtid == tid) SF_P8('='); else put_name<EMIT>(out, o, nm, mtid);
    SF_P8('\t'); put_i64<EMIT>(out, o, (int64_t)mpos + 1); SF_P8('\t'); put_i64<EMIT>(out, o, tlen); SF_P8('\t');
    R.oseq = (uint32_t)o; R.lseq = (uint32_t)lseq;
    if (lseq == 0) { SF_P8('*'); SF_P8('\t'); SF_P8('*'); }
    else { o += (uint32_t)lseq; SF_P8('\t'); if (ql[0] == 0xFF) SF_P8('*'); else o += (uint32_t)lseq; }
    for (const uint8_t *p = ax; (uint64_t)(end - p) >= 3;) {                            // (one or two stray bytes at the end are ignored)
        const uint8_t type = p[2]; const uint8_t *v = p + 3; const uint64_t left = (uint64_t)(end - v);
        SF_P8('\t'); SF_P8(p[0]); SF_P8(p[1]); SF_P8(':');
        if (type == 'A') { if (left < 1) return; SF_P8('A'); SF_P8(':'); SF_P8(v[0]); p = v + 1; }
        else if (type == 'c' || type == 'C') { if (left < 1) return; SF_P8('i'); SF_P8(':'); put_i64<EMIT>(out, o, type == 'c' ? (int64_t)(int8_t)v[0] : (int64_t)v[0]); p = v + 1; }
        else if (type == 's' || type == 'S') { if (left < 2) return; const uint16_t x = *(const sf_u16u *)v; SF_P8('i'); SF_P8(':'); put_i64<EMIT>(out, o, type == 's' ? (int64_t)(int16_t)x : (int64_t)x); p = v + 2; }
        else if (type == 'i' || type == 'I') { if (left < 4) return; const uint32_t x = *(const sf_u32u *)v; SF_P8('i'); SF_P8(':'); put_i64<EMIT>(out, o, type == 'i' ? (int64_t)(int32_t)x : (int64_t)x); p = v + 4; }
        else if (type == 'f') { if (left < 4) return; R.host = 1; p = v + 4; }            // (%g: the host's)
        else if (type == 'd') { if (left < 8) return; R.host = 1; p = v + 8; }
        else if (type == 'Z' || type == 'H') {
            uint64_t n = 0; while (n < left && v[n]) n++;
            if (n == left) return;                                                      // no NUL in front of the record's end
            SF_P8(type); SF_P8(':');
            if (EMIT) for (uint64_t k = 0; k < n; k++) out[o + k] = v[k];
            o += n; p = v + n + 1;
        }
        else if (type == 'B') {
            if (left < 5) return;
            const uint8_t sub = v[0]; const uint64_t cnt = *(const sf_u32u *)(v + 1);
            const uint32_t es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
            if (!es || 5 + es * cnt > left) return;
            SF_P8('B'); SF_P8(':'); SF_P8(sub);
            const uint8_t *q = v + 5;
            if (sub == 'f') R.host = 1;
            else for (uint64_t k = 0; k < cnt; k++, q += es) {
                SF_P8(',');
                int64_t x;
                if (es == 1) x = sub == 'c' ? (int64_t)(int8_t)q[0] : (int64_t)q[0];
                else if (es == 2) { const uint16_t y = *(const sf_u16u *)q; x = sub == 's' ? (int64_t)(int16_t)y : (int64_t)y; }
                else { const uint32_t y = *(const sf_u32u *)q; x = sub == 'i' ? (int64_t)(int32_t)y : (int64_t)y; }
                put_i64<EMIT>(out, o, x);
            }
            p = v + 5 + es * cnt;
        }
        else return;
    }
    SF_P8('\n');
    R.size = o; R.bad = 0;
}
#undef SF_P8

// four qualities at once: x + 33 in every byte, modulo 256, no carry between them
SF_HD uint32_t qual4(uint32_t x) { return ((x & 0x7F7F7F7Fu) + 0x21212121u) ^ (x & 0x80808080u); }
// SEQ and QUAL of one record (lseq > 0) by the `nl` lanes of its group (`lane` of them): sq the packed bases, ql the qualities, w where SEQ
// starts in the line (QUAL starts lseq + 1 bytes behind it and is left alone when its first byte is 0xFF: format_record wrote the `*`),
// codes the 16 characters of the nibbles.  Stores of 16 bytes, aligned on the destination; single bytes in front of the first boundary and
// behind the last whole chunk.  Every read stays inside the two fields and every write inside the two fields of the line.
SF_HD void emit_seq(const uint8_t *sq, const uint8_t *ql, uint8_t *w, uint32_t lseq, uint32_t lane, uint32_t nl, const uint8_t *codes) {
    {   // bases: chunk c takes the nibbles [head + 16 c, + 16), eight or (an odd start) nine bytes
        uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)w & 15u)) & 15u); if (head > lseq) head = lseq;
        const uint32_t nchunk = (lseq - head) >> 4, tail = head + (nchunk << 4);
        for (uint32_t k = lane; k < head; k += nl) w[k] = codes[(sq[k >> 1] >> ((~k & 1u) << 2)) & 15u];
        for (uint32_t c = lane; c < nchunk; c += nl) {
            const uint32_t k0 = head + (c << 4), odd = k0 & 1u; const uint8_t *t = sq + (k0 >> 1);
            const uint32_t lo = *(const sf_u32u *)t, hi = *(const sf_u32u *)(t + 4), ex = odd ? t[8] : 0u;
            uint32_t v[4];
            for (uint32_t j = 0; j < 4; j++) {
                uint32_t x = 0;
                for (uint32_t i = 0; i < 4; i++) {
                    const uint32_t nb = 4 * j + i + odd, by = nb >> 1;                 // nibble nb of the bytes loaded, the high one first
                    const uint32_t b = by < 4 ? (lo >> (8 * by)) & 255u : by < 8 ? (hi >> (8 * (by - 4))) & 255u : ex;
                    x |= (uint32_t)codes[(b >> ((~nb & 1u) << 2)) & 15u] << (8 * i);
                }
                v[j] = x;
            }
            uint32_t *d = reinterpret_cast<uint32_t *>(w + k0);                        // (16-byte aligned)
#if defined(__HIP_DEVICE_COMPILE__)
            *reinterpret_cast<uint4 *>(d) = make_uint4(v[0], v[1], v[2], v[3]);
#else
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
#endif
        }
        for (uint32_t k = tail + lane; k < lseq; k += nl) w[k] = codes[(sq[k >> 1] >> ((~k & 1u) << 2)) & 15u];
    }
    if (ql[0] == 0xFF) return;
    w += lseq + 1;
    {   // qualities
        uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)w & 15u)) & 15u); if (head > lseq) head = lseq;
        const uint32_t nchunk = (lseq - head) >> 4, tail = head + (nchunk << 4);
        for (uint32_t k = lane; k < head; k += nl) w[k] = (uint8_t)(ql[k] + 33);
        for (uint32_t c = lane; c < nchunk; c += nl) {
            const uint32_t b0 = head + (c << 4);
            uint32_t v[4];
            for (int j = 0; j < 4; j++) v[j] = qual4(*(const sf_u32u *)(ql + b0 + 4 * j));
            uint32_t *d = reinterpret_cast<uint32_t *>(w + b0);
#if defined(__HIP_DEVICE_COMPILE__)
            *reinterpret_cast<uint4 *>(d) = make_uint4(v[0], v[1], v[2], v[3]);
#else
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
#endif
        }
        for (uint32_t k = tail + lane; k < lseq; k += nl) w[k] = (uint8_t)(ql[k] + 33);
    }
}

#undef SF_HD

}  // namespace samfmt

#ifndef GCE_SAMFMT_HOST_CHECK
#include <algorithm>
#include "gce_samtext.hpp"

// process-wide counters of the GPU writer (gce_get_sam_format_counters): records formatted on the device, records the host formatted for
// it, formatter runs, text bytes
static int64_t g_samfmt_ctr[4] = {0, 0, 0, 0};

namespace {

// misc[0]: the lowest refused record (atomicMin)
__global__ __launch_bounds__(256) void k_samfmt_size(const uint8_t *rec, uint64_t n, const uint64_t *roff, uint64_t nr, samfmt::Names nm, uint64_t *size, uint8_t *hostf, uint32_t *oseq,
                                                     unsigned long long *misc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nr) return;
    const uint64_t a = roff[i];
    samfmt::Rec R;
    if (a >= n) { R.size = 0; R.bad = 1; R.host = 0; R.oseq = 0; }
    else samfmt::format_record<false>(rec + a, n - a, nm, nullptr, R);
    size[i] = R.bad || R.host ? 0ull : R.size;                                       // (a host record's size comes from the host: k_samfmt_hostsize)
    hostf[i] = (uint8_t)(!R.bad && R.host);
    oseq[i] = R.oseq;
    if (R.bad) atomicMin(misc, (unsigned long long)i);
}
__global__ __launch_bounds__(256) void k_samfmt_core(const uint8_t *rec, uint64_t n, const uint64_t *roff, const uint64_t *loff, const uint8_t *hostf, uint64_t nr, samfmt::Names nm, uint8_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nr || hostf[i]) return;
    const uint64_t a = roff[i];
    samfmt::Rec R;
    samfmt::format_record<true>(rec + a, n - a, nm, out + loff[i], R);
}
__global__ __launch_bounds__(256) void k_samfmt_seq(const uint8_t *rec, const uint64_t *roff, const uint64_t *loff, const uint8_t *hostf, const uint32_t *oseq, uint64_t nr, uint8_t *out) {
    __shared__ uint8_t codes[16];
    if (threadIdx.x < 16) codes[threadIdx.x] = (uint8_t)"=ACMGRSVTWYHKDBN"[threadIdx.x];
    __syncthreads();
    const uint32_t sub = threadIdx.x & 15u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < nr; j += ((uint64_t)gridDim.x * blockDim.x) >> 4) {
        if (hostf[j]) continue;
        const uint8_t *c = rec + roff[j] + 4;                                           // (the size pass accepted every record of the stream)
        const uint32_t lseq = *(const samfmt::sf_u32u *)(c + 16);
        if (!lseq) continue;
        const uint8_t *sq = c + 32 + c[8] + 4u * *(const samfmt::sf_u16u *)(c + 12);
        samfmt::emit_seq(sq, sq + (lseq + 1) / 2, out + loff[j] + oseq[j], lseq, sub, 16u, codes);
    }
}
// the records listed for the host: first byte and size (block_size included) of record hlist[j]
__global__ __launch_bounds__(256) void k_samfmt_hostmeta(const uint32_t *hlist, uint64_t nh, const uint8_t *rec, const uint64_t *roff, uint64_t *meta) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nh) return;
    const uint64_t a = roff[hlist[j]];
    meta[2 * j] = a; meta[2 * j + 1] = 4ull + *(const samfmt::sf_u32u *)(rec + a);
}
// one wave per listed record: its bytes to stage[soff[j], soff[j + 1])
__global__ __launch_bounds__(256) void k_samfmt_gather(const uint8_t *rec, const uint64_t *meta, const uint64_t *soff, uint64_t nh, uint8_t *stage) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; j < nh; j += ((uint64_t)gridDim.x * blockDim.x) >> 6) {
        const uint8_t *sp = rec + meta[2 * j]; uint8_t *d = stage + soff[j];
        const uint64_t sz = soff[j + 1] - soff[j];
        for (uint64_t k = lane; k < sz; k += 64) d[k] = sp[k];
    }
}
// the lengths of the host's lines into the size array
__global__ __launch_bounds__(256) void k_samfmt_hostsize(const uint32_t *hlist, uint64_t nh, const uint64_t *toff, uint64_t *size) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nh) return;
    size[hlist[j]] = toff[j + 1] - toff[j];
}
// the host's lines into their places: one wave per listed record, line j = stage[toff[j], toff[j + 1]) to out + loff[hlist[j]]
__global__ __launch_bounds__(256) void k_samfmt_patch(const uint8_t *stage, const uint64_t *toff, const uint32_t *hlist, const uint64_t *loff, uint64_t nh, uint8_t *out) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; j < nh; j += ((uint64_t)gridDim.x * blockDim.x) >> 6) {
        const uint8_t *sp = stage + toff[j]; uint8_t *d = out + loff[hlist[j]];
        const uint64_t sz = toff[j + 1] - toff[j];
        for (uint64_t k = lane; k < sz; k += 64) d[k] = sp[k];
    }
}
// the record walk of a stream whose starts nobody kept: one thread follows the block sizes.  res[0] = records, res[1] = the bad one or ~0
__global__ void k_samfmt_walk(const uint8_t *rec, uint64_t n, uint64_t *start, uint64_t cap, unsigned long long *res) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t nr = 0; int64_t bad = -1;
    samfmt::walk_records(rec, n, start, cap, nr, bad);
    res[0] = nr; res[1] = bad < 0 ? ~0ull : (unsigned long long)bad;
}

// the device side of one stream and the contig table
struct SamFmt {
    DevBuf size, hostf, oseq, loff, hlist, misc, nblob, noff, hmeta, hsoff, hstage, htoff, htext;
    std::vector<uint8_t> lines; std::vector<uint64_t> toff;                            // the host's lines, back to back, and their starts
    samfmt::Names nm{nullptr, nullptr, 0};
    uint64_t nr = 0, total = 0, n_host = 0; int64_t bad = -1;
    void release() { for (DevBuf *b : {&size, &hostf, &oseq, &loff, &hlist, &misc, &nblob, &noff, &hmeta, &hsoff, &hstage, &htoff, &htext}) b->release(); }
};

static int samfmt_names(SamFmt &d, hipStream_t s, const std::vector<std::string> &names, std::string &msg) {
    std::vector<uint8_t> blob; std::vector<uint32_t> off;
    for (const std::string &x : names) { off.push_back((uint32_t)blob.size()); blob.insert(blob.end(), x.begin(), x.end()); }
    off.push_back((uint32_t)blob.size());
    MCHK(d.nblob.ensure(blob.size() + 16)); MCHK(d.noff.ensure(off.size() * 4));
    if (!blob.empty()) MCHK(hipMemcpyAsync(d.nblob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    MCHK(hipMemcpyAsync(d.noff.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    MCHK(hipStreamSynchronize(s));
    d.nm.blob = d.nblob.as<uint8_t>(); d.nm.off = d.noff.as<uint32_t>(); d.nm.n = (int32_t)names.size();
    return GCE_OK;
}
// sizes, verdicts and line starts of the nr records of rec[0, n) (device memory) that start at roff[0, nr) -> d.total, d.bad, d.n_host; the
// host records' lines -> d.lines
static int samfmt_sizes(SamFmt &d, DevBuf &tmp, hipStream_t s, const uint8_t *rec, uint64_t n, const uint64_t *roff, uint64_t nr, const std::vector<std::string> &names, std::string &msg) {
    d.nr = nr; d.total = 0; d.n_host = 0; d.bad = -1; d.lines.clear(); d.toff.assign(1, 0);
    if (!nr) return GCE_OK;
    if (nr >= 0xFFFFFFF0ull) { msg = "more than 2^32 records in one stream"; return GCE_ERR_INVALID; }
    MCHK(d.size.ensure(nr * 8)); MCHK(d.hostf.ensure(nr + 8)); MCHK(d.oseq.ensure(nr * 4)); MCHK(d.loff.ensure((nr + 1) * 8)); MCHK(d.hlist.ensure(nr * 4 + 8)); MCHK(d.misc.ensure(64));
    const unsigned long long init[2] = {~0ull, 0ull};
    MCHK(hipMemcpyAsync(d.misc.p, init, sizeof init, hipMemcpyHostToDevice, s));
    const unsigned nb = (unsigned)((nr + 255) / 256);
    hipLaunchKernelGGL(k_samfmt_size, dim3(nb), dim3(256), 0, s, rec, n, roff, nr, d.nm, d.size.as<uint64_t>(), d.hostf.as<uint8_t>(), d.oseq.as<uint32_t>(), d.misc.as<unsigned long long>());
    MCHK(dev_select_flagged(d.hostf.as<uint8_t>(), nr, d.hlist.as<uint32_t>(), d.misc.as<unsigned long long>() + 1, tmp, s));
    unsigned long long h[2] = {0, 0};
    MCHK(hipMemcpyAsync(h, d.misc.p, sizeof h, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    if (h[0] != ~0ull) { d.bad = (int64_t)h[0]; return GCE_OK; }
    d.n_host = h[1];
    if (d.n_host) {                                                                   // f / d / B:f values: %g is the host's
        const uint64_t nh = d.n_host;
        MCHK(d.hmeta.ensure(nh * 16)); MCHK(d.hsoff.ensure((nh + 1) * 8)); MCHK(d.htoff.ensure((nh + 1) * 8));
        hipLaunchKernelGGL(k_samfmt_hostmeta, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, (const uint32_t *)d.hlist.p, nh, rec, roff, d.hmeta.as<uint64_t>());
        std::vector<uint64_t> hm((size_t)nh * 2), so((size_t)nh + 1, 0);
        MCHK(hipMemcpyAsync(hm.data(), d.hmeta.p, hm.size() * 8, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
        for (uint64_t j = 0; j < nh; j++) so[j + 1] = so[j] + hm[2 * j + 1];
        MCHK(d.hstage.ensure(so[nh] + 16));
        MCHK(hipMemcpyAsync(d.hsoff.p, so.data(), so.size() * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_samfmt_gather, dim3((unsigned)std::min<uint64_t>((nh + 3) / 4, 65535u)), dim3(256), 0, s, rec, (const uint64_t *)d.hmeta.p, (const uint64_t *)d.hsoff.p, nh, d.hstage.as<uint8_t>());
        std::vector<uint8_t> recs((size_t)so[nh]);
        MCHK(hipMemcpyAsync(recs.data(), d.hstage.p, recs.size(), hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
        std::string text; d.toff.assign((size_t)nh + 1, 0);
        for (uint64_t j = 0; j < nh; j++) {
            if (!samtext::bam_to_line(recs.data() + so[j], names, text)) { msg = "the device and the host disagree about a record"; return GCE_ERR_INVALID; }
            d.toff[j + 1] = text.size();
        }
        d.lines.assign(text.begin(), text.end());
        MCHK(hipMemcpyAsync(d.htoff.p, d.toff.data(), d.toff.size() * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_samfmt_hostsize, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, (const uint32_t *)d.hlist.p, nh, (const uint64_t *)d.htoff.p, d.size.as<uint64_t>());
    }
    MCHK(dev_exclusive_sum(d.size.as<uint64_t>(), nr, d.loff.as<uint64_t>(), tmp, s));
    MCHK(hipMemcpyAsync(&d.total, d.loff.as<uint64_t>() + nr, 8, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    return GCE_OK;
}
// the lines to out[0, d.total) (device memory; line i at loff[i]); the host's lines patched in
static int samfmt_emit(SamFmt &d, hipStream_t s, const uint8_t *rec, uint64_t n, const uint64_t *roff, uint8_t *out, std::string &msg) {
    const uint64_t nr = d.nr;
    if (!nr) return GCE_OK;
    hipLaunchKernelGGL(k_samfmt_core, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, s, rec, n, roff, (const uint64_t *)d.loff.p, (const uint8_t *)d.hostf.p, nr, d.nm, out);
    hipLaunchKernelGGL(k_samfmt_seq, dim3((unsigned)std::min<uint64_t>((nr + 15) / 16, 65535u)), dim3(256), 0, s, rec, roff, (const uint64_t *)d.loff.p, (const uint8_t *)d.hostf.p, (const uint32_t *)d.oseq.p, nr, out);
    if (d.n_host) {
        MCHK(d.htext.ensure(d.lines.size() + 16));
        MCHK(hipMemcpyAsync(d.htext.p, d.lines.data(), d.lines.size(), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_samfmt_patch, dim3((unsigned)std::min<uint64_t>((d.n_host + 3) / 4, 65535u)), dim3(256), 0, s, (const uint8_t *)d.htext.p, (const uint64_t *)d.htoff.p, (const uint32_t *)d.hlist.p,
                           (const uint64_t *)d.loff.p, d.n_host, out);
    }
    MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    __atomic_add_fetch(&g_samfmt_ctr[0], (int64_t)(nr - d.n_host), __ATOMIC_RELAXED); __atomic_add_fetch(&g_samfmt_ctr[1], (int64_t)d.n_host, __ATOMIC_RELAXED);
    __atomic_add_fetch(&g_samfmt_ctr[2], 1, __ATOMIC_RELAXED); __atomic_add_fetch(&g_samfmt_ctr[3], (int64_t)d.total, __ATOMIC_RELAXED);
    return GCE_OK;
}

static bool samfmt_names_ok(int32_t n_ref, const char *const *ref_name, std::vector<std::string> &names) {      // (offsets into the blob and SEQ's place in a line are 32 bits)
    uint64_t sum = 0;
    for (int32_t k = 0; k < n_ref; k++) { names.emplace_back(ref_name[k] ? ref_name[k] : ""); sum += names.back().size(); }
    return sum < (1ull << 30);
}

}  // namespace

extern "C" {

// Whole BAM records (host memory, back to back) through the kernels: their SAM lines, in record order, to out (host memory).  Replaces:
// samtext::bam_to_line over the records of a buffer, which is what sam_write1 does for the reference (src/gencore.cpp:104 behind sam_open(out, "w")).
int gce_sam_format(int32_t device, const void *records, size_t n, int32_t n_ref, const char *const *ref_name, void *out, size_t out_cap, size_t *out_bytes, int64_t *n_records, int64_t *n_host_records,
                   int64_t *bad_record, char err[256]) {
    auto seterr = [&](const std::string &m) { if (err) { strncpy(err, m.c_str(), 255); err[255] = 0; } };
    seterr("");
    if ((n && !records) || n_ref < 0 || (n_ref && !ref_name) || !out_bytes || !n_records || !n_host_records || !bad_record) { seterr("bad argument"); return GCE_ERR_INVALID; }
    *out_bytes = 0; *n_records = 0; *n_host_records = 0; *bad_record = -1;
    std::vector<std::string> names;
    if (!samfmt_names_ok(n_ref, ref_name, names)) { seterr("bad argument"); return GCE_ERR_INVALID; }
    // the record starts: the block sizes followed on the host, where the records are (a record cut by the end of the buffer stops the walk)
    const uint8_t *rp = (const uint8_t *)records;
    uint64_t nr = 0; int64_t wbad = -1;
    samfmt::walk_records(rp, n, nullptr, 0, nr, wbad);
    std::vector<uint64_t> start((size_t)nr + 1);
    samfmt::walk_records(rp, n, start.data(), nr, nr, wbad);
    const uint64_t used = start[(size_t)nr];                                          // the bytes of the records in front of the one the walk refused
    auto bad = [&](int64_t k) { *bad_record = k; seterr("bad record in the output stream"); return GCE_ERR_INVALID; };
    if (!nr) return wbad >= 0 ? bad(wbad) : GCE_OK;
    if (hipSetDevice(device) != hipSuccess) { seterr("no HIP device"); return GCE_ERR_NO_DEVICE; }
    SamFmt d; ScopedBuf tmp, rec, roff, text; std::string msg;
    hipStream_t s = nullptr;
    auto done = [&](int code) { d.release(); seterr(msg); return code; };
    int rc = samfmt_names(d, s, names, msg);
    if (rc != GCE_OK) return done(rc);
    if (rec.ensure(used + 64) != hipSuccess || roff.ensure((nr + 1) * 8) != hipSuccess) { msg = "out of device memory"; return done(GCE_ERR_OOM); }
    if (hipMemcpyAsync(rec.p, rp, used, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(roff.p, start.data(), (nr + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess) { msg = "hipMemcpy of the records failed"; return done(GCE_ERR_HIP); }
    if ((rc = samfmt_sizes(d, tmp, s, rec.as<uint8_t>(), used, roff.as<uint64_t>(), nr, names, msg)) != GCE_OK) return done(rc);
    if (d.bad >= 0 || wbad >= 0) { d.release(); return bad(d.bad >= 0 ? d.bad : wbad); }
    *out_bytes = (size_t)d.total; *n_records = (int64_t)nr; *n_host_records = (int64_t)d.n_host;
    if (d.total > out_cap || (d.total && !out)) { msg = "the output buffer is smaller than the text"; return done(GCE_ERR_OOM); }
    if (text.ensure(d.total + 64) != hipSuccess) { msg = "out of device memory"; return done(GCE_ERR_OOM); }
    if ((rc = samfmt_emit(d, s, rec.as<uint8_t>(), used, roff.as<uint64_t>(), text.as<uint8_t>(), msg)) != GCE_OK) return done(rc);
    if (hipMemcpy(out, text.p, d.total, hipMemcpyDeviceToHost) != hipSuccess) { msg = "hipMemcpy of the text failed"; return done(GCE_ERR_HIP); }
    return done(GCE_OK);
}

// After gce_raw_build_output (or gce_raw_merge_outputs on engs[0]): the resident record stream as SAM text in HBM -- replaces sam_write1's
// text under sam_open(out, "w") (src/gencore.cpp:170-173,104).  The record starts are what the build / merge left in rw_roff, or a walk of
// the block sizes when they are not there.  *text_bytes = the size of the text; gce_raw_read_text_async copies a piece of it out.
int gce_raw_format_output(gce_engine *e, int32_t n_ref, const char *const *ref_name, uint64_t *text_bytes) {
    if (!e || !e->raw_mode || n_ref < 0 || (n_ref && !ref_name) || !text_bytes) return GCE_ERR_INVALID;
    *text_bytes = 0; e->sf_bytes = 0;
    std::vector<std::string> names;
    if (!samfmt_names_ok(n_ref, ref_name, names)) return fail(e, GCE_ERR_INVALID, "gce_raw_format_output: contig names too long");
    const uint64_t total = e->raw_body_bytes;
    if (!total) return GCE_OK;
    (void)hipSetDevice(e->prm.device);
    hipStream_t s = e->stream;
    const uint8_t *rec = e->rw_body.as<uint8_t>();
    uint64_t nr = (uint64_t)std::max<int64_t>(e->raw_body_nrec, 0);
    if (e->raw_body_nrec < 0 || e->rw_roff.cap < (nr + 1) * 8) {                      // nobody kept the starts: follow the block sizes
        const uint64_t cap = total / 36 + 1;
        HIPCHK(e->rw_roff.ensure((cap + 1) * 8)); HIPCHK(e->rw.misc.ensure(64));
        hipLaunchKernelGGL(k_samfmt_walk, dim3(1), dim3(64), 0, s, rec, total, e->rw_roff.as<uint64_t>(), cap, e->rw.misc.as<unsigned long long>());
        unsigned long long res[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(res, e->rw.misc.p, sizeof res, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipGetLastError());
        if (res[1] != ~0ull || res[0] > cap) return fail(e, GCE_ERR_INVALID, "bad record in the output stream");
        nr = res[0]; e->raw_body_nrec = (int64_t)nr;
    }
    SamFmt d; std::string msg;
    auto done = [&](int code) { d.release(); return code == GCE_OK ? GCE_OK : fail(e, code, msg); };
    int rc = samfmt_names(d, s, names, msg);
    if (rc == GCE_OK) rc = samfmt_sizes(d, e->rw_tmp, s, rec, total, e->rw_roff.as<uint64_t>(), nr, names, msg);
    if (rc != GCE_OK) return done(rc);
    if (d.bad >= 0) { msg = "bad record in the output stream"; return done(GCE_ERR_INVALID); }
    if (e->sf_text.ensure(d.total + 64) != hipSuccess) { msg = "out of device memory"; return done(GCE_ERR_OOM); }
    if ((rc = samfmt_emit(d, s, rec, total, e->rw_roff.as<uint64_t>(), e->sf_text.as<uint8_t>(), msg)) != GCE_OK) return done(rc);
    e->sf_bytes = d.total; *text_bytes = d.total;
    return done(GCE_OK);
}
int gce_raw_read_text_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket) {
    if (!e || !e->raw_mode || offset + bytes > e->sf_bytes || (!host && bytes)) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    if (bytes) HIPCHK(hipMemcpyAsync(host, (const char *)e->sf_text.p + offset, bytes, hipMemcpyDeviceToHost, e->up_stream));
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev, e->up_stream));
    e->up_events.push_back(ev);
    if (ticket) *ticket = (int32_t)e->up_events.size() - 1;
    return GCE_OK;
}
int gce_get_sam_format_counters(int64_t out[4]) {
    if (!out) return GCE_ERR_INVALID;
    for (int k = 0; k < 4; k++) out[k] = __atomic_load_n(&g_samfmt_ctr[k], __ATOMIC_RELAXED);
    return GCE_OK;
}

}  // extern "C"
#endif  // GCE_SAMFMT_HOST_CHECK
