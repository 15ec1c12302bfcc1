// gce_samdev.hpp — SAM text lines into BAM records on the GPU (gce_sam_parse, gce_sam_sort).
//
// Replaces what the reference gets from htslib's sam_read1 / sam_parse1 when its input is SAM text (src/gencore.cpp:164,205), which this
// tree had on host threads only (samtext::line_to_bam, gce_samtext.hpp: the specification of every byte written here).  A window of text
// that holds whole alignment lines goes to HBM; the `@` lines stay on the host.  Per window:
//   k_sam_flag      four bytes per thread: the bytes that start a line which is a record (not empty, not a lone '\r')
//   dev_select_flagged -> the line starts, in order
//   k_sam_size      one thread per line: the line's end, its 11 fields, every check of line_to_bam in line_to_bam's order, the record's
//                   size; where SEQ and QUAL lie (16 bytes per line for k_sam_emit_seq); whether the line holds a floating-point value;
//                   the lowest failing line (atomicMin)
//   dev_exclusive_sum(size) -> the record starts (what WinIdx::off is to the sort), the window's record bytes
//   k_sam_emit_core one thread per line: block_size, the core block, the name, the CIGAR words, the optional fields
//   k_sam_hostmeta, k_sam_patch  the lines with floating-point values only: their starts and sizes to the host, the host's records, staged
//                   in one buffer, over the device's
//   k_sam_emit_seq  16 lanes per line: SEQ packed (nt16, two bases per byte) and QUAL - 33, 16-byte stores aligned on the DESTINATION, the
//                   bytes in front of the first boundary and behind the last one as single bytes (as sort_copy16)
// k_sam_size and k_sam_emit_core are one function, samdev::parse_line<EMIT>: the size pass and the emit pass cannot disagree about a byte.
// It and samdev::emit_seq are __host__ __device__: tests/samdev_host_check.hip runs them on the host against line_to_bam, one lane standing
// in for the 16.
// Floating point: `f`, `d` and `B:f` values need a correctly rounded decimal-to-binary conversion (strtof / strtod); the device writes
// zeroes in their place and lists the line, and the host overwrites the record with line_to_bam's (the same size by construction).  No
// other line reaches the host parser, except the first bad one, for its message.
#pragma once
#include <cstdint>

namespace samdev {

#define SD_HD __host__ __device__ inline

enum : uint32_t { SD_OK = 0, SD_FEW_FIELDS, SD_BAD_NUM, SD_BAD_QNAME, SD_CIG_RANGE, SD_CIG_MALFORMED, SD_CIG_UNKNOWN, SD_CIG_MANY, SD_SEQ_CIGAR, SD_SEQ_QUAL,
                  SD_AUX_MALFORMED, SD_AUX_A, SD_AUX_INT, SD_AUX_B, SD_AUX_B_SUB, SD_AUX_B_VALUE, SD_AUX_B_RANGE, SD_AUX_TYPE, SD_N_ERR };
// line_to_bam's message for each verdict (the library itself asks line_to_bam; the host check compares the two)
inline const char *message(uint32_t code) {
    static const char *const m[SD_N_ERR] = {"", "SAM line with fewer than 11 fields", "SAM line with a bad numeric field", "SAM line with a bad QNAME", "CIGAR length out of range", "malformed CIGAR",
        "unknown CIGAR operation", "more than 65535 CIGAR operations", "CIGAR and query sequence are of different length", "SEQ and QUAL of different length", "malformed optional field",
        "malformed A field", "integer field out of range", "malformed B field", "unknown B subtype", "malformed B value", "B value out of its type's range", "unknown optional field type"};
    return code < SD_N_ERR ? m[code] : "";
}

// the contig names sorted as byte strings (off[k] .. off[k + 1] of blob), tid[k] the header's index of the k-th (the first of equal names)
struct Contigs { const uint8_t *blob; const uint32_t *off; const int32_t *tid; int32_t n; };
// what the size pass learns about a line.  seq_off / qual_off: from the line's first byte (qual_off ~0: QUAL is `*`); oseq: where the packed
// bases start in the record
struct Line { uint32_t size, err, host, seq_off, lseq, qual_off, oseq; };

typedef uint32_t __attribute__((aligned(1), may_alias)) sd_u32u;

SD_HD int reg2bin(int64_t beg, int64_t end) {                                        // SAMv1 5.3 (arithmetic shifts: pos -1 gives bin 4680)
    --end;
    if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (int)(beg >> 14);
    if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (int)(beg >> 17);
    if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (int)(beg >> 20);
    if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (int)(beg >> 23);
    if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (int)(beg >> 26);
    return 0;
}
SD_HD uint8_t nt16(uint32_t c) {                                                     // "=ACMGRSVTWYHKDBN", either case; anything else 15
    const char *codes = "=ACMGRSVTWYHKDBN";
    for (uint32_t k = 0; k < 16; k++) if (c == (uint32_t)(uint8_t)codes[k] || (codes[k] >= 'A' && c == (uint32_t)(uint8_t)codes[k] + 32u)) return (uint8_t)k;
    return 15;
}
SD_HD bool parse_int(const uint8_t *a, const uint8_t *e, long long &out) {           // samtext::parse_int: an optional sign, digits, at most 2^40
    if (a >= e) return false;
    bool neg = false; const uint8_t *p = a;
    if (*p == '-' || *p == '+') { neg = *p == '-'; p++; }
    if (p >= e) return false;
    long long v = 0;
    for (; p < e; p++) { const uint32_t d = (uint32_t)*p - '0'; if (d > 9u) return false; v = v * 10 + (long long)d; if (v > (1ll << 40)) return false; }
    out = neg ? -v : v; return true;
}
SD_HD int32_t lookup(const Contigs &c, const uint8_t *a, const uint8_t *z) {         // `*` or a name the header does not have: -1
    const uint32_t len = (uint32_t)(z - a);
    if (len == 1 && *a == '*') return -1;
    int32_t lo = 0, hi = c.n - 1;
    while (lo <= hi) {
        const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
        const uint8_t *m = c.blob + c.off[mid]; const uint32_t ml = c.off[mid + 1] - c.off[mid], mn = len < ml ? len : ml;
        uint32_t k = 0; while (k < mn && a[k] == m[k]) k++;
        const int cmp = k < mn ? (int)a[k] - (int)m[k] : (len < ml ? -1 : len > ml ? 1 : 0);
        if (cmp == 0) return c.tid[mid];
        if (cmp < 0) hi = mid - 1; else lo = mid + 1;
    }
    return -1;
}

// One alignment line [s, e) (no line feed): line_to_bam's checks in line_to_bam's order, the record's size, and -- EMIT -- every byte of the
// record at `out` except the packed bases and the qualities (emit_seq).  A floating-point value is written as zeroes and sets L.host.
template <bool EMIT> SD_HD void parse_line(const uint8_t *s, const uint8_t *e, const Contigs &cg, uint8_t *out, Line &L) {
    L.size = 0; L.err = SD_OK; L.host = 0; L.seq_off = 0; L.lseq = 0; L.qual_off = ~0u; L.oseq = 0;
    if (e > s && e[-1] == '\r') e--;
    const uint8_t *fb[11], *fe[11]; int nf = 0; const uint8_t *aux = s;
    fb[0] = s;
    while (nf < 11) {
        const uint8_t *t = aux; while (t < e && *t != '\t') t++;
        if (t >= e) { fe[nf++] = e; aux = e; break; }
        fe[nf++] = t; aux = t + 1;
        if (nf < 11) fb[nf] = aux;
    }
    if (nf < 11) { L.err = SD_FEW_FIELDS; return; }
    long long flag, pos, mapq, pnext, tlen;
    if (!parse_int(fb[1], fe[1], flag) || !parse_int(fb[3], fe[3], pos) || !parse_int(fb[4], fe[4], mapq) || !parse_int(fb[7], fe[7], pnext) || !parse_int(fb[8], fe[8], tlen)
        || flag < 0 || flag > 0xFFFF || mapq < 0 || mapq > 255 || pos < 0 || pos > 0x7FFFFFFFll || pnext < 0 || pnext > 0x7FFFFFFFll || tlen < -0x7FFFFFFFll || tlen > 0x7FFFFFFFll) { L.err = SD_BAD_NUM; return; }
    const uint32_t lq = (uint32_t)(fe[0] - fb[0]);
    if (lq < 1 || lq > 254) { L.err = SD_BAD_QNAME; return; }
    int32_t tid = lookup(cg, fb[2], fe[2]);
    if (pos == 0 && tid >= 0) tid = -1;
    if (tid < 0) flag |= 4;
    const int32_t mtid = (fe[6] - fb[6] == 1 && *fb[6] == '=') ? tid : lookup(cg, fb[6], fe[6]);      // ('=' copies the tid as it stands after that reset)
    uint32_t o = 36;                                                                 // block_size and the core block: written last
#define SD_P8(x) do { if (EMIT) out[o] = (uint8_t)(x); o++; } while (0)
#define SD_P16(x) do { const uint32_t _v = (uint32_t)(x); SD_P8(_v); SD_P8(_v >> 8); } while (0)
#define SD_P32(x) do { const uint32_t _w = (uint32_t)(x); SD_P8(_w); SD_P8(_w >> 8); SD_P8(_w >> 16); SD_P8(_w >> 24); } while (0)
    if (EMIT) for (uint32_t k = 0; k < lq; k++) out[o + k] = fb[0][k];
    o += lq; SD_P8(0);
    uint32_t n_cigar = 0; int64_t rlen = 0, qlen = 0;
    if (fe[5] - fb[5] == 1 && *fb[5] == '*') flag |= 4;                               // (the flag only: contig and position stay)
    else {
        const uint8_t *p = fb[5], *z = fe[5];
        while (p < z) {
            uint64_t len = 0; const uint8_t *d = p;
            while (p < z && *p >= '0' && *p <= '9') { len = len * 10 + (uint64_t)(*p - '0'); p++; if (len >= (1ull << 28)) { L.err = SD_CIG_RANGE; return; } }
            if (p == d || p >= z) { L.err = SD_CIG_MALFORMED; return; }
            const char *ops = "MIDNSHP=X"; uint32_t op = 9;
            for (uint32_t k = 0; k < 9; k++) if (*p == (uint8_t)ops[k]) op = k;
            if (op == 9) { L.err = SD_CIG_UNKNOWN; return; }                          // (a NUL byte too)
            SD_P32((uint32_t)(len << 4 | op));
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += (int64_t)len;
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += (int64_t)len;
            n_cigar++; p++;
            if (n_cigar > 65535) { L.err = SD_CIG_MANY; return; }
        }
    }
    uint32_t lseq = 0;
    L.oseq = o;
    if (!(fe[9] - fb[9] == 1 && *fb[9] == '*')) {
        lseq = (uint32_t)(fe[9] - fb[9]);
        if (n_cigar > 0 && qlen != (int64_t)lseq) { L.err = SD_SEQ_CIGAR; return; }
    }
    L.lseq = lseq; L.seq_off = (uint32_t)(fb[9] - s);
    if (!(fe[10] - fb[10] == 1 && *fb[10] == '*')) {
        if ((uint32_t)(fe[10] - fb[10]) != lseq) { L.err = SD_SEQ_QUAL; return; }
        L.qual_off = (uint32_t)(fb[10] - s);
    }
    o += (lseq + 1) / 2 + lseq;
    for (const uint8_t *p = aux; p < e;) {
        const uint8_t *z = p; while (z < e && *z != '\t') z++;
        if (z - p < 5 || p[2] != ':' || p[4] != ':') { L.err = SD_AUX_MALFORMED; return; }
        const uint8_t type = p[3]; const uint8_t *v = p + 5;
        SD_P8(p[0]); SD_P8(p[1]);
        if (type == 'A') { if (z - v != 1) { L.err = SD_AUX_A; return; } SD_P8('A'); SD_P8(*v); }
        else if (type == 'i') {
            long long x; if (!parse_int(v, z, x) || x < -(1ll << 31) || x > 0xFFFFFFFFll) { L.err = SD_AUX_INT; return; }
            if (*v == '-') { if (x >= -128) { SD_P8('c'); SD_P8(x); } else if (x >= -32768) { SD_P8('s'); SD_P16(x); } else { SD_P8('i'); SD_P32(x); } }
            else { if (x <= 255) { SD_P8('C'); SD_P8(x); } else if (x <= 65535) { SD_P8('S'); SD_P16(x); } else { SD_P8('I'); SD_P32(x); } }
        }
        else if (type == 'f') { SD_P8('f'); SD_P32(0); L.host = 1; }                  // (the host writes the value: strtof)
        else if (type == 'd') { SD_P8('d'); SD_P32(0); SD_P32(0); L.host = 1; }
        else if (type == 'Z' || type == 'H') {
            SD_P8(type);
            if (EMIT) for (const uint8_t *q = v; q < z; q++) out[o + (uint32_t)(q - v)] = *q;
            o += (uint32_t)(z - v); SD_P8(0);
        }
        else if (type == 'B') {
            if (z - v < 1) { L.err = SD_AUX_B; return; }
            const uint8_t sub = *v;
            if (!(sub == 'c' || sub == 'C' || sub == 's' || sub == 'S' || sub == 'i' || sub == 'I' || sub == 'f')) { L.err = SD_AUX_B_SUB; return; }
            SD_P8('B'); SD_P8(sub);
            uint32_t cnt = 0; for (const uint8_t *q = v + 1; q < z; q++) cnt += *q == ',';
            SD_P32(cnt);
            const uint8_t *q = v + 1;
            while (q < z) {
                q++;                                                                  // the comma
                const uint8_t *n = q; while (n < z && *n != ',') n++;
                if (sub == 'f') { SD_P32(0); L.host = 1; }
                else {
                    long long x; if (!parse_int(q, n, x)) { L.err = SD_AUX_B_VALUE; return; }
                    const long long lo_ = sub == 'c' ? -128 : sub == 's' ? -32768 : sub == 'i' ? -(1ll << 31) : 0, hi_ = sub == 'c' ? 127 : sub == 'C' ? 255 : sub == 's' ? 32767 : sub == 'S' ? 65535 : sub == 'i' ? 0x7FFFFFFFll : 0xFFFFFFFFll;
                    if (x < lo_ || x > hi_) { L.err = SD_AUX_B_RANGE; return; }
                    if (sub == 'c' || sub == 'C') SD_P8(x); else if (sub == 's' || sub == 'S') SD_P16(x); else SD_P32(x);
                }
                q = n;
            }
        }
        else { L.err = SD_AUX_TYPE; return; }
        p = z < e ? z + 1 : e;
    }
    L.size = o;
    if (EMIT) {
        const int64_t p0 = pos - 1;
        int64_t span = (flag & 4) ? 1 : rlen; if (span == 0) span = 1;
        const uint32_t bin = (uint32_t)reg2bin(p0, p0 + span) & 0xFFFFu;
        const uint32_t end = o;
        o = 0; SD_P32(end - 4);
        SD_P32(tid); SD_P32((int32_t)p0); SD_P8(lq + 1); SD_P8(mapq); SD_P16(bin); SD_P16(n_cigar); SD_P16(flag);
        SD_P32(lseq); SD_P32(mtid); SD_P32((int32_t)(pnext - 1)); SD_P32((int32_t)tlen);
    }
#undef SD_P8
#undef SD_P16
#undef SD_P32
}

// byte k of the packed bases / four qualities at once (x - 33 in every byte, no borrow between them)
SD_HD uint8_t seq_byte(const uint8_t *q, uint32_t k, uint32_t lseq, const uint8_t *t16) { return (uint8_t)(t16[q[2 * k]] << 4 | (2 * k + 1 < lseq ? t16[q[2 * k + 1]] : 0)); }
SD_HD uint32_t qual4(uint32_t x) { const uint32_t H = 0x80808080u, y = 0x21212121u; return ((x | H) - y) ^ ((x ^ ~y) & H); }
// SEQ and QUAL of one line by the `nl` lanes of its group (`lane` of them): q / ql the text (ql NULL: QUAL is `*`), w the record's packed
// bases, (lseq + 1) / 2 bytes, the qualities behind them.  Stores of 16 bytes, aligned on the destination; single bytes in front of the first
// boundary and behind the last whole chunk.  Every read stays inside the two fields and every write inside the record.
SD_HD void emit_seq(const uint8_t *q, const uint8_t *ql, uint8_t *w, uint32_t lseq, uint32_t lane, uint32_t nl, const uint8_t *t16) {
    {   // bases: chunk c packs text bytes [2 (head + 16 c), + 32) into 16 bytes
        const uint32_t nb = (lseq + 1) / 2, nfull = lseq / 2;
        uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)w & 15u)) & 15u); if (head > nfull) head = nfull;
        const uint32_t nchunk = (nfull - head) >> 4, tail = head + (nchunk << 4);
        for (uint32_t k = lane; k < head; k += nl) w[k] = seq_byte(q, k, lseq, t16);
        for (uint32_t c = lane; c < nchunk; c += nl) {
            const uint32_t b0 = head + (c << 4); const uint8_t *t = q + 2 * b0;
            uint32_t v[4];
            for (int j = 0; j < 4; j++) {
                const uint32_t lo = *(const sd_u32u *)(t + 8 * j), hi = *(const sd_u32u *)(t + 8 * j + 4);
                v[j] = (uint32_t)(t16[lo & 255u] << 4 | t16[(lo >> 8) & 255u]) | (uint32_t)(t16[(lo >> 16) & 255u] << 4 | t16[lo >> 24]) << 8
                     | (uint32_t)(t16[hi & 255u] << 4 | t16[(hi >> 8) & 255u]) << 16 | (uint32_t)(t16[(hi >> 16) & 255u] << 4 | t16[hi >> 24]) << 24;
            }
            uint32_t *d = reinterpret_cast<uint32_t *>(w + b0);                       // (16-byte aligned)
#if defined(__HIP_DEVICE_COMPILE__)
            *reinterpret_cast<uint4 *>(d) = make_uint4(v[0], v[1], v[2], v[3]);
#else
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
#endif
        }
        for (uint32_t k = tail + lane; k < nb; k += nl) w[k] = seq_byte(q, k, lseq, t16);
        w += nb;
    }
    {   // qualities
        uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)w & 15u)) & 15u); if (head > lseq) head = lseq;
        const uint32_t nchunk = (lseq - head) >> 4, tail = head + (nchunk << 4);
        for (uint32_t k = lane; k < head; k += nl) w[k] = ql ? (uint8_t)(ql[k] - 33) : (uint8_t)0xFF;
        for (uint32_t c = lane; c < nchunk; c += nl) {
            const uint32_t b0 = head + (c << 4);
            uint32_t v[4];
            for (int j = 0; j < 4; j++) v[j] = ql ? qual4(*(const sd_u32u *)(ql + b0 + 4 * j)) : 0xFFFFFFFFu;
            uint32_t *d = reinterpret_cast<uint32_t *>(w + b0);
#if defined(__HIP_DEVICE_COMPILE__)
            *reinterpret_cast<uint4 *>(d) = make_uint4(v[0], v[1], v[2], v[3]);
#else
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
#endif
        }
        for (uint32_t k = tail + lane; k < lseq; k += nl) w[k] = ql ? (uint8_t)(ql[k] - 33) : (uint8_t)0xFF;
    }
}

#undef SD_HD

}  // namespace samdev

#ifndef GCE_SAMDEV_HOST_CHECK
#include <algorithm>
#include <numeric>
#include "gce_samtext.hpp"

namespace {

// flag[i] = 1: byte i starts a line that is a record.  Four bytes per thread; the text is followed by zero bytes up to a multiple of 4.
__global__ __launch_bounds__(256) void k_sam_flag(const uint8_t *t, uint64_t n, uint8_t *flag) {
    const uint64_t i4 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    const uint32_t w = *reinterpret_cast<const uint32_t *>(t + i4);
    uint8_t c[6];
    c[0] = i4 ? t[i4 - 1] : (uint8_t)'\n';
    c[1] = (uint8_t)w; c[2] = (uint8_t)(w >> 8); c[3] = (uint8_t)(w >> 16); c[4] = (uint8_t)(w >> 24);
    c[5] = i4 + 4 < n ? t[i4 + 4] : (uint8_t)'\n';
    uint32_t f = 0;
    for (int k = 0; k < 4; k++) {
        const uint64_t i = i4 + (uint64_t)k;
        if (i >= n) break;
        const uint8_t nx = i + 1 < n ? c[k + 2] : (uint8_t)'\n';
        if (c[k] == '\n' && c[k + 1] != '\n' && !(c[k + 1] == '\r' && nx == '\n')) f |= 1u << (8 * k);
    }
    *reinterpret_cast<uint32_t *>(flag + i4) = f;
}
// misc[0]: the lowest failing line (atomicMin)
__global__ __launch_bounds__(256) void k_sam_size(const uint8_t *t, uint64_t n, const uint32_t *start, uint64_t nl, samdev::Contigs cg, uint32_t *len, uint32_t *size, uint8_t *hostf, uint4 *d4,
                                                  unsigned long long *misc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const uint8_t *s = t + start[i], *e = s, *lim = t + n;
    while (e < lim && *e != '\n') e++;
    samdev::Line L;
    samdev::parse_line<false>(s, e, cg, nullptr, L);
    len[i] = (uint32_t)(e - s);
    size[i] = L.err ? 0u : L.size;
    hostf[i] = (uint8_t)(!L.err && L.host);
    d4[i] = make_uint4(L.seq_off, L.lseq, L.qual_off, L.oseq);
    if (L.err) atomicMin(misc, (unsigned long long)i);
}
__global__ __launch_bounds__(256) void k_sam_emit_core(const uint8_t *t, const uint32_t *start, const uint32_t *len, const uint64_t *roff, uint64_t nl, samdev::Contigs cg, uint8_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl) return;
    const uint8_t *s = t + start[i];
    samdev::Line L;
    samdev::parse_line<true>(s, s + len[i], cg, out + roff[i], L);
}
__global__ __launch_bounds__(256) void k_sam_emit_seq(const uint8_t *t, const uint32_t *start, const uint4 *d4, const uint64_t *roff, uint64_t nl, uint8_t *out) {
    __shared__ uint8_t t16[256];
    t16[threadIdx.x] = samdev::nt16(threadIdx.x);
    __syncthreads();
    const uint32_t sub = threadIdx.x & 15u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < nl; j += ((uint64_t)gridDim.x * blockDim.x) >> 4) {
        const uint4 d = d4[j];
        if (!d.y) continue;
        const uint8_t *s = t + start[j];
        samdev::emit_seq(s + d.x, d.z == ~0u ? nullptr : s + d.z, out + roff[j] + d.w, d.y, sub, 16u, t16);
    }
}

// the lines listed for the host: first byte, record start and size of line hlist[j]
__global__ __launch_bounds__(256) void k_sam_hostmeta(const uint32_t *hlist, uint64_t nh, const uint32_t *start, const uint64_t *roff, const uint32_t *size, uint64_t *meta) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nh) return;
    const uint32_t i = hlist[j];
    meta[3 * j] = start[i]; meta[3 * j + 1] = roff[i]; meta[3 * j + 2] = size[i];
}
// the host's records over the device's: one wave per listed line, record j = stage[soff[j], soff[j + 1]) to out + meta[3 j + 1]
__global__ __launch_bounds__(256) void k_sam_patch(const uint8_t *stage, const uint64_t *soff, const uint64_t *meta, uint64_t nh, uint8_t *out) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; j < nh; j += ((uint64_t)gridDim.x * blockDim.x) >> 6) {
        const uint8_t *sp = stage + soff[j]; uint8_t *d = out + meta[3 * j + 1];
        const uint64_t sz = soff[j + 1] - soff[j];
        for (uint64_t k = lane; k < sz; k += 64) d[k] = sp[k];
    }
}

// the device side of one window and the contig table
struct SamDev {
    DevBuf text, flag, start, len, size, hostf, d4, roff, hlist, misc, cblob, coff, ctid, hmeta, hstage, hsoff;
    std::vector<uint64_t> hm; uint64_t host_bytes = 0;                                // the listed lines (start, record start, size each); their records' bytes
    samdev::Contigs cg{nullptr, nullptr, nullptr, 0};
    samtext::NameMap nmap;
    uint64_t n = 0, nl = 0, total = 0, n_host = 0; int64_t bad = -1; uint64_t bad_start = 0;
    double kernel_s = 0;
    void release() { for (DevBuf *b : {&text, &flag, &start, &len, &size, &hostf, &d4, &roff, &hlist, &misc, &cblob, &coff, &ctid, &hmeta, &hstage, &hsoff}) b->release(); }
    uint64_t held() const { uint64_t a = 0; for (const DevBuf *b : {&text, &flag, &start, &len, &size, &hostf, &d4, &roff, &hlist, &misc, &cblob, &coff, &ctid, &hmeta, &hstage, &hsoff}) a += b->cap; return a; }
};
// the device bytes a window of n text bytes and nl lines takes, as DevBuf::ensure makes them: the text and the flags, 41 bytes per line
// (the staging of the host's records is counted apart: SamDev::host_bytes)
static uint64_t sam_win_need(uint64_t n, uint64_t nl) { return ((n + 128) * 2 + nl * 45 + 4096) * 9 / 8 + 13 * 256; }
// ... and that staging: the records and their 8-byte starts, as DevBuf::ensure makes the two buffers
static uint64_t sam_host_need(const SamDev &d) { return (d.host_bytes + d.n_host * 8 + 64) * 9 / 8 + 512; }

static int sam_contigs(SamDev &d, hipStream_t s, const std::vector<std::string> &names, std::string &msg) {
    d.nmap.build(names);
    std::vector<uint32_t> idx(names.size()); std::iota(idx.begin(), idx.end(), 0u);
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { const int c = names[a].compare(names[b]); return c < 0 || (c == 0 && a < b); });
    std::vector<uint8_t> blob; std::vector<uint32_t> off; std::vector<int32_t> tid;
    for (size_t k = 0; k < idx.size(); k++) {
        if (k && names[idx[k]] == names[idx[k - 1]]) continue;                        // (the first of equal names, as the host's map keeps it)
        off.push_back((uint32_t)blob.size()); tid.push_back((int32_t)idx[k]);
        blob.insert(blob.end(), names[idx[k]].begin(), names[idx[k]].end());
    }
    off.push_back((uint32_t)blob.size());
    MCHK(d.cblob.ensure(blob.size() + 16)); MCHK(d.coff.ensure(off.size() * 4)); MCHK(d.ctid.ensure(tid.size() * 4 + 16));
    if (!blob.empty()) MCHK(hipMemcpyAsync(d.cblob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    MCHK(hipMemcpyAsync(d.coff.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    if (!tid.empty()) MCHK(hipMemcpyAsync(d.ctid.p, tid.data(), tid.size() * 4, hipMemcpyHostToDevice, s));
    MCHK(hipStreamSynchronize(s));
    d.cg.blob = d.cblob.as<uint8_t>(); d.cg.off = d.coff.as<uint32_t>(); d.cg.tid = d.ctid.as<int32_t>(); d.cg.n = (int32_t)tid.size();
    return GCE_OK;
}
// the text (whole alignment lines; n < 2^32) to the device and the lines counted -> d.nl
static int sam_lines(SamDev &d, DevBuf &tmp, hipStream_t s, const char *text, uint64_t n, std::string &msg) {
    d.n = n; d.nl = 0; d.total = 0; d.n_host = 0; d.bad = -1;
    if (!n) return GCE_OK;
    MCHK(d.text.ensure(n + 128)); MCHK(d.flag.ensure(n + 128)); MCHK(d.misc.ensure(64));
    MCHK(hipMemcpyAsync(d.text.p, text, n, hipMemcpyHostToDevice, s));
    MCHK(hipMemsetAsync(d.text.as<uint8_t>() + n, 0, 128, s));
    const unsigned long long init[2] = {~0ull, 0ull};
    MCHK(hipMemcpyAsync(d.misc.p, init, sizeof init, hipMemcpyHostToDevice, s));
    MCHK(hipStreamSynchronize(s));                                                    // (kernel_s: the kernels, not the copy in front of them)
    const double t0 = mono_s();
    hipLaunchKernelGGL(k_sam_flag, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, s, (const uint8_t *)d.text.p, n, d.flag.as<uint8_t>());
    // dev_select_flagged in its three steps, the count read in the middle: the list of line starts is made for the lines there are
    const unsigned nb = (unsigned)((n + SCAN_TILE - 1) / SCAN_TILE);
    MCHK(tmp.ensure((size_t)nb * 8 + 64));
    hipLaunchKernelGGL(k_flag_reduce, dim3(nb), dim3(256), 0, s, (const uint8_t *)d.flag.p, n, tmp.as<uint64_t>());
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, s, tmp.as<uint64_t>(), (uint64_t)nb, d.misc.as<unsigned long long>() + 1, (unsigned long long *)nullptr);
    unsigned long long h[2] = {0, 0};
    MCHK(hipMemcpyAsync(h, d.misc.p, sizeof h, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    d.nl = h[1];
    if (d.nl) {
        MCHK(d.start.ensure((size_t)d.nl * 4));
        hipLaunchKernelGGL(k_flag_apply, dim3(nb), dim3(256), 0, s, (const uint8_t *)d.flag.p, n, (const uint64_t *)tmp.p, d.start.as<uint32_t>());
        MCHK(hipGetLastError());
    }
    d.kernel_s += mono_s() - t0;
    return GCE_OK;
}
// sizes, verdicts and record starts -> d.total, d.bad (with d.bad_start, the line's first byte), d.n_host
static int sam_sizes(SamDev &d, DevBuf &tmp, hipStream_t s, std::string &msg) {
    const uint64_t nl = d.nl;
    if (!nl) return GCE_OK;
    MCHK(d.len.ensure(nl * 4)); MCHK(d.size.ensure(nl * 4)); MCHK(d.hostf.ensure(nl + 8)); MCHK(d.d4.ensure(nl * 16)); MCHK(d.roff.ensure((nl + 1) * 8)); MCHK(d.hlist.ensure(nl * 4 + 8));
    const double t0 = mono_s();
    const unsigned nb = (unsigned)((nl + 255) / 256);
    hipLaunchKernelGGL(k_sam_size, dim3(nb), dim3(256), 0, s, (const uint8_t *)d.text.p, d.n, (const uint32_t *)d.start.p, nl, d.cg, d.len.as<uint32_t>(), d.size.as<uint32_t>(), d.hostf.as<uint8_t>(),
                       d.d4.as<uint4>(), d.misc.as<unsigned long long>());
    MCHK(dev_exclusive_sum(d.size.as<uint32_t>(), nl, d.roff.as<uint64_t>(), tmp, s));
    MCHK(dev_select_flagged(d.hostf.as<uint8_t>(), nl, d.hlist.as<uint32_t>(), d.misc.as<unsigned long long>() + 1, tmp, s));
    unsigned long long h[2] = {0, 0};
    MCHK(hipMemcpyAsync(h, d.misc.p, sizeof h, hipMemcpyDeviceToHost, s));
    MCHK(hipMemcpyAsync(&d.total, d.roff.as<uint64_t>() + nl, 8, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    d.kernel_s += mono_s() - t0;
    d.n_host = h[1]; d.host_bytes = 0; d.hm.clear();
    if (d.n_host && h[0] == ~0ull) {                                                  // what the host patch needs of the listed lines, and of no other
        const double t1 = mono_s();
        MCHK(d.hmeta.ensure((size_t)d.n_host * 24));
        hipLaunchKernelGGL(k_sam_hostmeta, dim3((unsigned)((d.n_host + 255) / 256)), dim3(256), 0, s, (const uint32_t *)d.hlist.p, d.n_host, (const uint32_t *)d.start.p, (const uint64_t *)d.roff.p,
                           (const uint32_t *)d.size.p, d.hmeta.as<uint64_t>());
        d.hm.resize((size_t)d.n_host * 3);
        MCHK(hipMemcpyAsync(d.hm.data(), d.hmeta.p, d.hm.size() * 8, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
        for (uint64_t j = 0; j < d.n_host; j++) d.host_bytes += d.hm[3 * j + 2];
        d.kernel_s += mono_s() - t1;
    }
    if (h[0] != ~0ull) {
        d.bad = (int64_t)h[0];
        uint32_t st = 0;
        MCHK(hipMemcpyAsync(&st, d.start.as<uint32_t>() + h[0], 4, hipMemcpyDeviceToHost, s)); MCHK(hipStreamSynchronize(s));
        d.bad_start = st;
    }
    return GCE_OK;
}
// line_to_bam's message for the line that starts at byte `a` of text[0, n)
static std::string sam_line_message(const SamDev &d, const char *text, uint64_t n, uint64_t a) {
    const char *q = (const char *)memchr(text + a, '\n', (size_t)(n - a)); const uint64_t le = q ? (uint64_t)(q - text) : n;
    std::vector<uint8_t> o; std::string m;
    if (samtext::line_to_bam(text + a, text + le, d.nmap, o, m)) m = "the device and the host disagree about a SAM line";
    return m;
}
// the window's records to out[0, d.total) (device memory; record i at roff[i]); the listed lines re-parsed by the host and overwritten
static int sam_emit(SamDev &d, hipStream_t s, const char *text, uint8_t *out, std::string &msg) {
    const uint64_t nl = d.nl;
    if (!nl) return GCE_OK;
    const double t0 = mono_s();
    hipLaunchKernelGGL(k_sam_emit_core, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, (const uint8_t *)d.text.p, (const uint32_t *)d.start.p, (const uint32_t *)d.len.p, (const uint64_t *)d.roff.p, nl, d.cg, out);
    hipLaunchKernelGGL(k_sam_emit_seq, dim3((unsigned)std::min<uint64_t>((nl + 15) / 16, 65535u)), dim3(256), 0, s, (const uint8_t *)d.text.p, (const uint32_t *)d.start.p, (const uint4 *)d.d4.p,
                       (const uint64_t *)d.roff.p, nl, out);
    MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    if (d.n_host) {                                                                   // f / d / B:f values: strtof and strtod are the host's
        std::vector<uint8_t> stage; std::vector<uint64_t> so((size_t)d.n_host + 1, 0); std::string m;
        stage.reserve((size_t)d.host_bytes);
        for (uint64_t j = 0; j < d.n_host; j++) {
            const uint64_t a = d.hm[3 * j]; const char *q = (const char *)memchr(text + a, '\n', (size_t)(d.n - a)); const uint64_t le = q ? (uint64_t)(q - text) : d.n;
            if (!samtext::line_to_bam(text + a, text + le, d.nmap, stage, m) || stage.size() - so[j] != d.hm[3 * j + 2]) { msg = "the device and the host disagree about a SAM line"; return GCE_ERR_INVALID; }
            so[j + 1] = stage.size();
        }
        MCHK(d.hstage.ensure(stage.size() + 16)); MCHK(d.hsoff.ensure(so.size() * 8));
        MCHK(hipMemcpyAsync(d.hstage.p, stage.data(), stage.size(), hipMemcpyHostToDevice, s));
        MCHK(hipMemcpyAsync(d.hsoff.p, so.data(), so.size() * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_sam_patch, dim3((unsigned)std::min<uint64_t>((d.n_host + 3) / 4, 65535u)), dim3(256), 0, s, (const uint8_t *)d.hstage.p, (const uint64_t *)d.hsoff.p, (const uint64_t *)d.hmeta.p, d.n_host, out);
        MCHK(hipStreamSynchronize(s)); MCHK(hipGetLastError());
    }
    d.kernel_s += mono_s() - t0;
    return GCE_OK;
}

}  // namespace

extern "C" {

// One window of SAM text (alignment lines only; host memory) through the kernels: the BAM records of its lines, back to back, to out (host
// memory).  Replaces: samtext::line_to_bam over the lines of a window, which is what sam_read1 does for the reference (src/gencore.cpp:205).
int gce_sam_parse(int32_t device, const char *text, size_t n, int32_t n_ref, const char *const *ref_name, void *out, size_t out_cap, size_t *out_bytes, int64_t *n_records, int64_t *n_host_lines,
                  int64_t *bad_line, char err[256]) {
    auto seterr = [&](const std::string &m) { if (err) { strncpy(err, m.c_str(), 255); err[255] = 0; } };
    seterr("");
    if ((n && !text) || n_ref < 0 || (n_ref && !ref_name) || !out_bytes || !n_records || !n_host_lines || !bad_line || n >= 0xFFFFFF00ull) { seterr("bad argument"); return GCE_ERR_INVALID; }
    *out_bytes = 0; *n_records = 0; *n_host_lines = 0; *bad_line = -1;
    if (hipSetDevice(device) != hipSuccess) { seterr("no HIP device"); return GCE_ERR_NO_DEVICE; }
    std::vector<std::string> names; for (int32_t k = 0; k < n_ref; k++) names.emplace_back(ref_name[k] ? ref_name[k] : "");
    SamDev d; ScopedBuf tmp, rec; std::string msg;
    hipStream_t s = nullptr;
    auto done = [&](int code) { d.release(); seterr(msg); return code; };
    int rc = sam_contigs(d, s, names, msg);
    if (rc == GCE_OK) rc = sam_lines(d, tmp, s, text, n, msg);
    if (rc == GCE_OK) rc = sam_sizes(d, tmp, s, msg);
    if (rc != GCE_OK) return done(rc);
    if (d.bad >= 0) { *bad_line = d.bad; msg = sam_line_message(d, text, n, d.bad_start); return done(GCE_ERR_INVALID); }
    *out_bytes = (size_t)d.total; *n_records = (int64_t)d.nl; *n_host_lines = (int64_t)d.n_host;
    if (d.total > out_cap || (d.total && !out)) { msg = "the output buffer is smaller than the records"; return done(GCE_ERR_OOM); }
    if (!d.total) return done(GCE_OK);
    if (rec.ensure(d.total + 64) != hipSuccess) { msg = "out of device memory"; return done(GCE_ERR_OOM); }
    if ((rc = sam_emit(d, s, text, rec.as<uint8_t>(), msg)) != GCE_OK) return done(rc);
    if (hipMemcpy(out, rec.p, d.total, hipMemcpyDeviceToHost) != hipSuccess) { msg = "hipMemcpy of the records failed"; return done(GCE_ERR_HIP); }
    return done(GCE_OK);
}

}  // extern "C"
#endif  // GCE_SAMDEV_HOST_CHECK
