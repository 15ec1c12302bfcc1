// gce_bgzf.hpp — the host's BGZF and BAM-header pieces, once (included by bamio.cpp and by tests/bgzf_host_check.cpp; no GPU code, no C-ABI):
// one member's framing (scan_member), the BAM header (parse_bam_header, bam_header_bytes), the member codec (inflate_block: the raw-deflate
// decoder below with zlib as fallback and arbiter, the CRC-32 by carry-less multiplication; deflate_block: zlib or the fixed-Huffman encoder
// below), the EOF member and two small file helpers.  The formats are the published ones (SAMv1 section 4), restated here.
// Everything sits in an unnamed namespace: the header is the private part of ONE translation unit per program.
#pragma once
#include <zlib.h>
#include <unistd.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Block { uint64_t coff; uint32_t csize, usize; uint64_t uoff; };

inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | p[1] << 8); }
inline uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline int32_t rdi32(const uint8_t *p) { int32_t v; memcpy(&v, p, 4); return v; }

// ---- one BGZF member's framing (SAMv1 4.1): gzip magic with FEXTRA, the extra field's subfields walked for "BC" (BSIZE), ISIZE from the trailer
enum class Scan { Member, More, NotBgzf, BadBlock, BadIsize };
struct Member { uint32_t bsize = 0, isize = 0; uint16_t xlen = 0; };          // xlen: set as soon as the magic has passed (gce_bam_open's truncation messages)
inline const char *scan_message(Scan s) {
    return s == Scan::NotBgzf ? "not a BGZF file" : s == Scan::BadBlock ? "bad BGZF block" : s == Scan::BadIsize ? "bad BGZF block (ISIZE above 64 KB)" : "";
}
// The member that starts at buf + off, of a buffer of `have` bytes: Member (m is filled), More (the buffer ends inside it: a streaming
// caller carries the tail over to its next piece, gce_bam_open calls the file truncated) or what is wrong with it.  No byte at or beyond
// buf + have is read.  The checks run in this order, so every damaged file keeps its message.
inline Scan scan_member(const uint8_t *buf, size_t have, size_t off, Member &m) {
    if (off + 18 > have) return Scan::More;
    const uint8_t *p = buf + off;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return Scan::NotBgzf;
    const uint16_t xlen = m.xlen = rd16(p + 10);
    if (off + 12 + (size_t)xlen > have) return Scan::More;
    uint32_t bsize = 0; bool found = false;
    for (uint32_t x = 0; x + 4 <= xlen; ) {
        const uint8_t *sf = p + 12 + x; const uint16_t sl = rd16(sf + 2);
        if (x + 4 + (uint32_t)sl > xlen) break;                                   // a subfield that runs past the extra field
        if (sf[0] == 'B' && sf[1] == 'C' && sl == 2) { bsize = (uint32_t)rd16(sf + 4) + 1; found = true; }
        x += 4 + sl;
    }
    if (!found || bsize < 12u + xlen + 8u) return Scan::BadBlock;
    if (off + bsize > have) return Scan::More;
    m.bsize = bsize; m.isize = rd32(p + bsize - 4);
    if (m.isize > 0x10000u) return Scan::BadIsize;                                // the format's limit (callers size their buffers by the sum of these)
    return Scan::Member;
}

// ---- the BAM header (SAMv1 4.2): magic, l_text, text, n_ref, then (l_name, name, l_ref) per contig, at the front of the n inflated bytes u.
// NotBam: four bytes are there and they are not the magic.  Incomplete: more bytes may complete it (every caller has its own words for a
// stream that ends here).  Complete: h is filled, hdr_end is the first record's offset.  The contig table is read in one of two dialects,
// kept apart as the runners had them:
//   Collect (gce_bam_open, gce_run_bam, gce_run_bam_passes): names and lengths go to *names / *lens; a zero-length name reads as Incomplete.
//   Skip    (gce_bam_index, the sort runners): the table is only stepped over; a zero-length name is accepted, n_ref must be below 2^31.
enum class Contigs { Collect, Skip };
enum class Hdr { NotBam, Incomplete, Complete };
struct BamHeader { uint64_t text_off = 8; uint32_t l_text = 0, n_ref = 0; uint64_t hdr_end = 0; };
inline Hdr parse_bam_header(const uint8_t *u, uint64_t n, Contigs dialect, BamHeader &h, std::vector<std::string> *names = nullptr, std::vector<uint32_t> *lens = nullptr) {
    if (n >= 4 && memcmp(u, "BAM\1", 4) != 0) return Hdr::NotBam;
    if (n < 12) return Hdr::Incomplete;
    uint64_t p = 8; const uint32_t l_text = rd32(u + 4);
    if (p + l_text + 4 > n) return Hdr::Incomplete;
    p += l_text;
    const uint32_t n_ref = rd32(u + p); p += 4;
    if (dialect == Contigs::Skip && n_ref >= 0x7FFFFFFFu) return Hdr::Incomplete;
    if (names) names->clear();
    if (lens) lens->clear();
    for (uint32_t r = 0; r < n_ref; r++) {
        if (p + 4 > n) return Hdr::Incomplete;
        const uint32_t ln = rd32(u + p); p += 4;
        if ((dialect == Contigs::Collect && ln == 0) || p + (uint64_t)ln + 4 > n) return Hdr::Incomplete;
        if (names) names->emplace_back((const char *)u + p, ln ? ln - 1 : 0);
        p += ln;
        if (lens) lens->push_back(rd32(u + p));
        p += 4;
    }
    h.text_off = 8; h.l_text = l_text; h.n_ref = n_ref; h.hdr_end = p;
    return Hdr::Complete;
}
// the bytes parse_bam_header reads: BAM magic, text, contig table
inline std::vector<uint8_t> bam_header_bytes(const std::string &text, const std::vector<std::string> &names, const std::vector<uint32_t> &lens) {
    std::vector<uint8_t> hdr;
    auto put32 = [&](uint32_t x) { const uint8_t *p = (const uint8_t *)&x; hdr.insert(hdr.end(), p, p + 4); };
    hdr.insert(hdr.end(), {'B', 'A', 'M', 1});
    put32((uint32_t)text.size()); hdr.insert(hdr.end(), text.begin(), text.end());
    put32((uint32_t)lens.size());
    for (size_t r = 0; r < lens.size(); r++) { put32((uint32_t)names[r].size() + 1); hdr.insert(hdr.end(), names[r].begin(), names[r].end()); hdr.push_back(0); put32(lens[r]); }
    return hdr;
}

// the empty member that ends a BGZF file
const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// n bytes of the file from offset off into dst; returns the bytes read (fewer than n: the file ended or a read failed)
inline size_t pread_full(int fd, void *dst, size_t n, uint64_t off) {
    size_t o = 0;
    while (o < n) { const ssize_t g = pread(fd, (char *)dst + o, n - o, (off_t)(off + o)); if (g <= 0) break; o += (size_t)g; }
    return o;
}
// does the file start with the gzip magic?  (sam_open takes either format, src/gencore.cpp:164: a file without it is SAM text)
inline bool looks_gzip(int fd, uint64_t fsz) {
    uint8_t m2[2] = {0, 0};
    return fsz >= 2 && pread(fd, m2, 2, 0) == 2 && m2[0] == 0x1f && m2[1] == 0x8b;
}
// does the file start with a BGZF member's magic (scan_member's first check, on the file's first 18 bytes)?
inline bool starts_bgzf(int fd, uint64_t fsz) {
    uint8_t h[18]; Member m;
    return fsz >= 18 && pread_full(fd, h, 18, 0) == 18 && scan_member(h, 18, 0, m) != Scan::NotBgzf;
}

// ---- CRC-32 (gzip polynomial, reflected) by carry-less multiplication: "Fast CRC Computation for Generic Polynomials Using PCLMULQDQ"
// (Gopal et al., Intel 2009) -- fold four 128-bit lanes over 64 input bytes a step, fold the lanes together, reduce 128 -> 64 -> 32
// bits (Barrett).  zlib 1.2.11's table-driven crc32 runs at 1.0 GB/s per thread, which made the checksum 45 % of a BGZF block's
// inflate time (zlib inflates BAM data at ~0.8 GB/s).  Used only when the CPU has PCLMULQDQ and a self-check against zlib passes;
// tails and short buffers stay with zlib.
#if defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("pclmul,sse4.1"))) inline __m128i crc_fold(__m128i acc, __m128i k, __m128i next) {   // acc * x^distance mod P, plus the next 16 bytes
    return _mm_xor_si128(_mm_xor_si128(_mm_clmulepi64_si128(acc, k, 0x00), _mm_clmulepi64_si128(acc, k, 0x11)), next);
}
__attribute__((target("pclmul,sse4.1"))) uint32_t crc32_clmul_state(const uint8_t *buf, size_t len /* >= 64, multiple of 16 */, uint32_t state) {
    // x^(n) mod P constants of the paper for the bit-reflected gzip polynomial: fold distances 4 x 128 (+-32), 128 (+-32), 64, and P / mu
    const __m128i k_fold4 = _mm_set_epi64x(0x01c6e41596ll, 0x0154442bd4ll), k_fold1 = _mm_set_epi64x(0x00ccaa009ell, 0x01751997d0ll);
    const __m128i k_64 = _mm_set_epi64x(0, 0x0163cd6124ll), k_poly = _mm_set_epi64x(0x01f7011641ll, 0x01db710641ll);
    const __m128i *p = reinterpret_cast<const __m128i *>(buf);
    __m128i a0 = _mm_xor_si128(_mm_loadu_si128(p), _mm_cvtsi32_si128((int)state)), a1 = _mm_loadu_si128(p + 1), a2 = _mm_loadu_si128(p + 2), a3 = _mm_loadu_si128(p + 3);
    p += 4; len -= 64;
    for (; len >= 64; p += 4, len -= 64) {
        a0 = crc_fold(a0, k_fold4, _mm_loadu_si128(p)); a1 = crc_fold(a1, k_fold4, _mm_loadu_si128(p + 1));
        a2 = crc_fold(a2, k_fold4, _mm_loadu_si128(p + 2)); a3 = crc_fold(a3, k_fold4, _mm_loadu_si128(p + 3));
    }
    a0 = crc_fold(a0, k_fold1, a1); a0 = crc_fold(a0, k_fold1, a2); a0 = crc_fold(a0, k_fold1, a3);
    for (; len >= 16; p += 1, len -= 16) a0 = crc_fold(a0, k_fold1, _mm_loadu_si128(p));
    // 128 -> 64 bits
    const __m128i low32 = _mm_setr_epi32(~0, 0, ~0, 0);
    __m128i t = _mm_xor_si128(_mm_srli_si128(a0, 8), _mm_clmulepi64_si128(a0, k_fold1, 0x10));
    t = _mm_xor_si128(_mm_srli_si128(t, 4), _mm_clmulepi64_si128(_mm_and_si128(t, low32), k_64, 0x00));
    // Barrett reduction 64 -> 32 bits
    __m128i q = _mm_clmulepi64_si128(_mm_and_si128(t, low32), k_poly, 0x10);
    q = _mm_clmulepi64_si128(_mm_and_si128(q, low32), k_poly, 0x00);
    return (uint32_t)_mm_extract_epi32(_mm_xor_si128(t, q), 1);
}
bool crc32_clmul_usable() {
    static const bool ok = [] {
        if (!__builtin_cpu_supports("pclmul") || !__builtin_cpu_supports("sse4.1")) return false;
        uint8_t tmp[1024 + 16];
        uint32_t x = 0x9E3779B9u;
        for (size_t i = 0; i < sizeof tmp; i++) { x = x * 1664525u + 1013904223u; tmp[i] = (uint8_t)(x >> 24); }
        for (size_t off = 0; off < 3; off++)
            for (size_t n : {(size_t)64, (size_t)80, (size_t)128, (size_t)1008, (size_t)1024}) {
                const uint32_t want = (uint32_t)crc32(crc32(0L, Z_NULL, 0), tmp + off, (uInt)n);
                if ((uint32_t)~crc32_clmul_state(tmp + off, n, 0xFFFFFFFFu) != want) return false;
            }
        return true;
    }();
    return ok;
}
#else
bool crc32_clmul_usable() { return false; }
uint32_t crc32_clmul_state(const uint8_t *, size_t, uint32_t s) { return s; }
#endif
// CRC-32 of a whole buffer (what a gzip member stores)
uint32_t crc32_buf(const uint8_t *buf, size_t n) {
    uint32_t c = (uint32_t)crc32(0L, Z_NULL, 0);
    size_t done = 0;
    if (n >= 64 && crc32_clmul_usable()) { done = n & ~(size_t)15; c = ~crc32_clmul_state(buf, done, 0xFFFFFFFFu); }
    while (done < n) { const size_t m = std::min<size_t>(n - done, 1u << 30); c = (uint32_t)crc32(c, buf + done, (uInt)m); done += m; }
    return c;
}

// ---- raw-deflate decoder for BGZF members (RFC 1951), used in front of zlib: 64-bit bit buffer refilled eight bytes at a time, one
// table look-up per symbol (10-bit primary table + subtables for literals/lengths, 8-bit + subtables for distances), matches copied
// in 8-byte words.  A BGZF member is self-contained (empty window at its start, <= 64 KB out), every output byte is bounds-checked,
// and the caller verifies the member's CRC-32 -- whatever this decoder does not handle (incomplete Huffman codes, damaged streams)
// or gets wrong falls back to zlib's inflate, which stays the arbiter of what a valid stream is.
namespace fastinf {
enum : uint32_t { K_INVALID = 0, K_LIT = 1, K_LEN = 2, K_EOB = 4, K_SUB = 8, K_DIST = 6 };   // (K_LIT and K_SUB are single bits: tested with one AND)
constexpr int LIT_BITS = 10, DIST_BITS = 8, LIT_CAP = (1 << LIT_BITS) + 1024, DIST_CAP = (1 << DIST_BITS) + 512;
// entry: bits 0..7 code bits to consume | 8..11 kind | 12..15 extra bits (K_SUB: subtable bits) | 16..31 value (literal, base, subtable start)
inline uint32_t mk(uint32_t kind, uint32_t bits, uint32_t extra, uint32_t value) { return bits | kind << 8 | extra << 12 | value << 16; }
const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

inline uint32_t sym_entry_litlen(int sym, uint32_t bits) {
    if (sym < 256) return mk(K_LIT, bits, 0, (uint32_t)sym);
    if (sym == 256) return mk(K_EOB, bits, 0, 0);
    if (sym <= 285) return mk(K_LEN, bits, LEN_EXTRA[sym - 257], LEN_BASE[sym - 257]);
    return mk(K_INVALID, bits, 0, 0);
}
inline uint32_t sym_entry_dist(int sym, uint32_t bits) {
    if (sym < 30) return mk(K_DIST, bits, DIST_EXTRA[sym], DIST_BASE[sym]);
    return mk(K_INVALID, bits, 0, 0);
}
inline uint32_t rev_bits(uint32_t code, int len) { uint32_t r = 0; for (int i = 0; i < len; i++) { r = r << 1 | (code & 1); code >>= 1; } return r; }

// canonical Huffman code of `lens` -> look-up table.  Only COMPLETE codes are taken (Kraft sum exactly 1); returns false otherwise.
template <class EntryOf> bool build_table(const uint8_t *lens, int nsym, int primary, uint32_t *table, int cap, EntryOf entry_of) {
    int count[16] = {0};
    for (int s = 0; s < nsym; s++) count[lens[s]]++;
    count[0] = 0;
    uint32_t kraft = 0;
    for (int l = 1; l <= 15; l++) kraft += (uint32_t)count[l] << (15 - l);
    if (kraft != (1u << 15)) return false;
    uint32_t next_code[16]; { uint32_t code = 0; for (int l = 1; l <= 15; l++) { code = (code + (uint32_t)count[l - 1]) << 1; next_code[l] = code; } }
    // reversed code of every coded symbol; the longest code behind every primary prefix
    uint16_t rcode[288]; uint8_t sub_bits[1 << LIT_BITS];
    const int np = 1 << primary;
    memset(sub_bits, 0, (size_t)np);
    for (int s = 0; s < nsym; s++) {
        const int l = lens[s];
        if (!l) continue;
        const uint32_t r = rev_bits(next_code[l]++, l);
        rcode[s] = (uint16_t)r;
        if (l > primary) { uint8_t &b = sub_bits[r & (uint32_t)(np - 1)]; b = (uint8_t)std::max<int>(b, l - primary); }
    }
    int used = np;
    for (int i = 0; i < np; i++) {
        if (!sub_bits[i]) continue;
        if (used + (1 << sub_bits[i]) > cap) return false;
        table[i] = mk(K_SUB, (uint32_t)primary, sub_bits[i], (uint32_t)used);
        used += 1 << sub_bits[i];
    }
    for (int s = 0; s < nsym; s++) {
        const int l = lens[s];
        if (!l) continue;
        const uint32_t r = rcode[s];
        if (l <= primary) { const uint32_t e = entry_of(s, (uint32_t)l); for (uint32_t i = r; i < (uint32_t)np; i += 1u << l) table[i] = e; }
        else {
            const uint32_t pi = r & (uint32_t)(np - 1), sb = sub_bits[pi], start = table[pi] >> 16, e = entry_of(s, (uint32_t)(l - primary));
            for (uint32_t i = r >> primary; i < (1u << sb); i += 1u << (l - primary)) table[start + i] = e;
        }
    }
    return true;
}

struct Tables { uint32_t lit[LIT_CAP], dist[DIST_CAP]; };
const Tables *fixed_tables() {
    static const Tables *t = [] {
        Tables *x = new Tables;
        uint8_t l[288]; for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        uint8_t d[32]; for (int i = 0; i < 32; i++) d[i] = 5;
        build_table(l, 288, LIT_BITS, x->lit, LIT_CAP, sym_entry_litlen); build_table(d, 32, DIST_BITS, x->dist, DIST_CAP, sym_entry_dist);
        return x;
    }();
    return t;
}

// src[0, n): raw deflate; dst[0, want): exactly `want` bytes must come out.  src must be readable up to src + n + 8 (a BGZF member's
// CRC-32 and ISIZE follow its deflate data).  false = not handled (the caller runs zlib).
bool inflate_raw(const uint8_t *src, size_t n, uint8_t *dst, size_t want) {
    const uint8_t *in = src, *const in_end = src + n;
    uint8_t *out = dst, *const out_end = dst + want;
    uint64_t bb = 0; int nb = 0;                                              // bit buffer, valid bits
    const uint8_t *const lim = in_end + 8;                                    // readable up to here (the member's CRC-32 and ISIZE)
    auto refill = [&]() -> bool {                                             // >= 56 valid bits afterwards; bits past the deflate data are whatever follows
        uint64_t w = 0;                                                       // it (or zeros) -- a stream that needs them fails the position check at the end
        if (in + 8 <= lim) memcpy(&w, in, 8);
        else { if (in > lim) return false; for (int i = 0; in + i < lim; i++) w |= (uint64_t)in[i] << (8 * i); }
        bb |= w << nb; in += (63 - nb) >> 3; nb |= 56;
        return true;
    };
    Tables dyn;
    for (bool last = false; !last;) {
        if (!refill()) return false;
        last = bb & 1; const uint32_t type = (uint32_t)(bb >> 1) & 3; bb >>= 3; nb -= 3;
        if (type == 0) {                                                      // stored
            const int drop = nb & 7; bb >>= drop; nb -= drop;
            if (!refill()) return false;
            const uint32_t len = (uint32_t)bb & 0xFFFF, nlen = (uint32_t)(bb >> 16) & 0xFFFF; bb >>= 32; nb -= 32;
            if ((len ^ nlen) != 0xFFFF) return false;
            const uint8_t *p = in - (nb >> 3);                                // first byte not yet consumed (nb is a multiple of 8 here)
            if ((size_t)(in_end - p) < len || p > in_end || (size_t)(out_end - out) < len) return false;
            memcpy(out, p, len); out += len; in = p + len; bb = 0; nb = 0;
            continue;
        }
        const uint32_t *lit, *dist;
        if (type == 1) { const Tables *f = fixed_tables(); lit = f->lit; dist = f->dist; }
        else if (type == 2) {
            const int hlit = (int)(bb & 31) + 257, hdist = (int)(bb >> 5 & 31) + 1, hclen = (int)(bb >> 10 & 15) + 4; bb >>= 14; nb -= 14;
            if (hlit > 286 || hdist > 30) return false;
            static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t cl[19] = {0};
            for (int i = 0; i < hclen; i++) { if (nb < 3 && !refill()) return false; cl[order[i]] = (uint8_t)(bb & 7); bb >>= 3; nb -= 3; }
            uint32_t clt[1 << 7];
            if (!build_table(cl, 19, 7, clt, 1 << 7, [](int s, uint32_t bits) { return mk(K_LIT, bits, 0, (uint32_t)s); })) return false;
            uint8_t lens[288 + 32]; int k = 0;
            memset(lens, 0, sizeof lens);
            while (k < hlit + hdist) {
                if (!refill()) return false;
                const uint32_t e = clt[bb & 127]; const int s = (int)(e >> 16); bb >>= (e & 0xFF); nb -= (int)(e & 0xFF);
                if (s < 16) { lens[k++] = (uint8_t)s; continue; }
                int rep; uint8_t v = 0;
                if (s == 16) { if (k == 0) return false; v = lens[k - 1]; rep = 3 + (int)(bb & 3); bb >>= 2; nb -= 2; }
                else if (s == 17) { rep = 3 + (int)(bb & 7); bb >>= 3; nb -= 3; }
                else { rep = 11 + (int)(bb & 127); bb >>= 7; nb -= 7; }
                if (k + rep > hlit + hdist) return false;
                memset(lens + k, v, (size_t)rep); k += rep;
            }
            if (lens[256] == 0) return false;                                 // no end-of-block code
            uint8_t dl[32]; memset(dl, 0, sizeof dl); memcpy(dl, lens + hlit, (size_t)hdist);
            memset(lens + hlit, 0, (size_t)(288 - hlit));
            if (!build_table(lens, 288, LIT_BITS, dyn.lit, LIT_CAP, sym_entry_litlen)) return false;
            if (!build_table(dl, 32, DIST_BITS, dyn.dist, DIST_CAP, sym_entry_dist)) return false;      // (a lone distance code: zlib's business)
            lit = dyn.lit; dist = dyn.dist;
        } else return false;
        for (;;) {                                                            // symbols of the block
            if (!refill()) return false;                                      // >= 56 bits: a length/distance pair needs at most 15 + 5 + 15 + 13 = 48
            uint32_t e = lit[bb & ((1u << LIT_BITS) - 1)];
            if (e & (K_LIT << 8)) {                                           // literals first: up to four from one refill (<= 10 + 3 x 10 + ... bits of the 56)
                if (out_end - out < 4) { if (out >= out_end) return false; bb >>= (e & 0xFF); nb -= (int)(e & 0xFF); *out++ = (uint8_t)(e >> 16); continue; }
                bb >>= (e & 0xFF); nb -= (int)(e & 0xFF); *out++ = (uint8_t)(e >> 16);
                e = lit[bb & ((1u << LIT_BITS) - 1)];
                if (!(e & (K_LIT << 8))) continue;
                bb >>= (e & 0xFF); nb -= (int)(e & 0xFF); *out++ = (uint8_t)(e >> 16);
                e = lit[bb & ((1u << LIT_BITS) - 1)];
                if (!(e & (K_LIT << 8))) continue;
                bb >>= (e & 0xFF); nb -= (int)(e & 0xFF); *out++ = (uint8_t)(e >> 16);
                e = lit[bb & ((1u << LIT_BITS) - 1)];
                if (!(e & (K_LIT << 8))) continue;
                bb >>= (e & 0xFF); nb -= (int)(e & 0xFF); *out++ = (uint8_t)(e >> 16);
                continue;
            }
            if (e & (K_SUB << 8)) { bb >>= LIT_BITS; nb -= LIT_BITS; e = lit[(e >> 16) + (uint32_t)(bb & ((1u << ((e >> 12) & 15)) - 1))]; }
            bb >>= (e & 0xFF); nb -= (int)(e & 0xFF);
            const uint32_t kind = (e >> 8) & 15;
            if (kind == K_LIT) { if (out >= out_end) return false; *out++ = (uint8_t)(e >> 16); continue; }      // (a literal with a long code)
            if (kind == K_EOB) break;
            if (kind != K_LEN) return false;
            const uint32_t xl = (e >> 12) & 15, length = (e >> 16) + (uint32_t)(bb & ((1u << xl) - 1)); bb >>= xl; nb -= (int)xl;
            uint32_t d = dist[bb & ((1u << DIST_BITS) - 1)];
            if (d & (K_SUB << 8)) { bb >>= DIST_BITS; nb -= DIST_BITS; d = dist[(d >> 16) + (uint32_t)(bb & ((1u << ((d >> 12) & 15)) - 1))]; }
            bb >>= (d & 0xFF); nb -= (int)(d & 0xFF);
            if (((d >> 8) & 15) != K_DIST) return false;
            const uint32_t xd = (d >> 12) & 15, distance = (d >> 16) + (uint32_t)(bb & ((1u << xd) - 1)); bb >>= xd; nb -= (int)xd;
            if (nb < 0) return false;                                         // ran past what the refill provided
            if (distance > (size_t)(out - dst) || length > (size_t)(out_end - out)) return false;
            const uint8_t *from = out - distance;
            if (distance >= 8 && (size_t)(out_end - out) >= length + 8) {     // whole words (may run up to 7 bytes over the match, inside the member)
                uint8_t *o = out; const uint8_t *f = from;
                for (uint32_t c = 0; c < length; c += 8) { uint64_t w; memcpy(&w, f + c, 8); memcpy(o + c, &w, 8); }
            } else if (distance == 1) memset(out, from[0], length);           // a run of one byte (quality strings are full of them)
            else for (uint32_t c = 0; c < length; c++) out[c] = from[c];
            out += length;
        }
        if (nb < 0) return false;
    }
    if ((size_t)(in - src) * 8 - (size_t)nb > n * 8) return false;            // consumed bits past the end of the deflate data
    return out == out_end;
}
}  // namespace fastinf

// one raw-deflate BGZF member -> dst (usize bytes); checks the CRC
bool inflate_block(const uint8_t *src, const Block &b, uint8_t *dst) {
    const uint16_t xlen = rd16(src + 10);
    const uint8_t *cdata = src + 12 + xlen;
    const uint32_t clen = b.csize - 12 - xlen - 8;
    static const bool zlib_only = getenv("GCE_BAM_ZLIB_ONLY") != nullptr;     // (A/B and tests)
    if (!zlib_only && fastinf::inflate_raw(cdata, clen, dst, b.usize) && crc32_buf(dst, b.usize) == rd32(src + b.csize - 8)) return true;
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t *>(cdata); zs.avail_in = clen; zs.next_out = dst; zs.avail_out = b.usize;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    if (rc != Z_STREAM_END || zs.total_out != b.usize) return false;
    return crc32_buf(dst, b.usize) == rd32(src + b.csize - 8);
}

// ---- "level 1" raw-deflate encoder for BGZF members: greedy LZ77 over a 2^13-entry hash of 4-byte strings (the member is its own
// window: positions fit 16 bits), ONE fixed-Huffman block (RFC 1951 3.2.6) -- no code construction, a 64-bit bit accumulator.  Gives
// up (returns 0) when the result would not fit a BGZF member; the caller then takes zlib as before.
namespace fastdef {
struct Codes {
    uint16_t lit[286]; uint8_t lit_bits[286];              // literal / end-of-block codes, bit-reversed for the LSB-first stream
    uint32_t len[259]; uint8_t len_bits[259];              // match length 3..258: code + extra bits in one word
    uint8_t dcode[512];                                    // distance - 1 -> distance code (zlib's two-level index)
};
inline uint32_t rev(uint32_t code, int len) { uint32_t r = 0; for (int i = 0; i < len; i++) { r = r << 1 | (code & 1); code >>= 1; } return r; }
const Codes &codes() {
    static const Codes c = [] {
        Codes x; memset(&x, 0, sizeof x);
        auto fixed = [](int s, uint32_t &code, int &bits) {
            if (s < 144) { code = 0x30 + (uint32_t)s; bits = 8; } else if (s < 256) { code = 0x190 + (uint32_t)(s - 144); bits = 9; }
            else if (s < 280) { code = (uint32_t)(s - 256); bits = 7; } else { code = 0xC0 + (uint32_t)(s - 280); bits = 8; }
        };
        for (int s = 0; s <= 256; s++) { uint32_t code; int bits; fixed(s, code, bits); x.lit[s] = (uint16_t)rev(code, bits); x.lit_bits[s] = (uint8_t)bits; }
        for (int L = 3; L <= 258; L++) {
            int idx = 28; while (fastinf::LEN_BASE[idx] > L) idx--;
            if (L == 258) idx = 28;
            uint32_t code; int bits; fixed(257 + idx, code, bits);
            x.len[L] = rev(code, bits) | (uint32_t)(L - fastinf::LEN_BASE[idx]) << bits; x.len_bits[L] = (uint8_t)(bits + fastinf::LEN_EXTRA[idx]);
        }
        for (int d = 1; d <= 32768; d++) {
            int dc = 29; while (fastinf::DIST_BASE[dc] > d) dc--;
            const int k = d - 1;
            x.dcode[k < 256 ? k : 256 + (k >> 7)] = (uint8_t)dc;           // (all distances that share an index share a code)
        }
        return x;
    }();
    return c;
}
// src[0, n), n <= 65535 -> dst[0, cap); returns the size or 0
size_t deflate_fixed(const uint8_t *src, uint32_t n, uint8_t *dst, size_t cap) {
    const Codes &c = codes();
    uint16_t head[1 << 13];
    memset(head, 0, sizeof head);
    uint8_t *out = dst, *const out_end = dst + cap;
    uint64_t acc = 0; int nacc = 0;
    auto put = [&](uint64_t v, int bits) -> bool {                            // bits <= 31 per call
        acc |= v << nacc; nacc += bits;
        if (nacc >= 32) { if (out + 4 > out_end) return false; const uint32_t w = (uint32_t)acc; memcpy(out, &w, 4); out += 4; acc >>= 32; nacc -= 32; }
        return true;
    };
    if (!put(1 | 1 << 1, 3)) return 0;                                        // BFINAL = 1, BTYPE = 01
    uint32_t i = 0;
    while (i + 4 <= n) {
        uint32_t cur; memcpy(&cur, src + i, 4);
        const uint32_t h = (cur * 2654435761u) >> 19;
        const uint32_t cand = head[h];
        head[h] = (uint16_t)(i + 1);
        uint32_t at;
        if (cand && (memcpy(&at, src + cand - 1, 4), at == cur) && i - (cand - 1) <= 32768u) {
            const uint8_t *a = src + i, *b = src + cand - 1;
            const uint32_t maxlen = std::min<uint32_t>(258u, n - i);
            uint32_t len = 4;
            while (len + 8 <= maxlen) { uint64_t x, y; memcpy(&x, a + len, 8); memcpy(&y, b + len, 8); if (x != y) { len += (uint32_t)__builtin_ctzll(x ^ y) >> 3; goto done; } len += 8; }
            while (len < maxlen && a[len] == b[len]) len++;
        done:
            const uint32_t d = i - (cand - 1), dc = c.dcode[d - 1 < 256 ? d - 1 : 256 + ((d - 1) >> 7)];
            if (!put(c.len[len], c.len_bits[len])) return 0;
            if (!put(rev(dc, 5) | (uint64_t)(d - fastinf::DIST_BASE[dc]) << 5, 5 + fastinf::DIST_EXTRA[dc])) return 0;
            i += len;
        } else {
            if (!put(c.lit[src[i]], c.lit_bits[src[i]])) return 0;
            i++;
        }
    }
    for (; i < n; i++) if (!put(c.lit[src[i]], c.lit_bits[src[i]])) return 0;
    if (!put(c.lit[256], c.lit_bits[256])) return 0;
    while (nacc > 0) { if (out >= out_end) return 0; *out++ = (uint8_t)acc; acc >>= 8; nacc -= 8; }
    return (size_t)(out - dst);
}
}  // namespace fastdef

// one BGZF member from `n` (<= 0xff00) bytes; returns its size
size_t deflate_block(const uint8_t *src, uint32_t n, int level, uint8_t *dst /* >= 0x10000 + 64 */) {
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(dst, head, 16);
    static const bool zlib_only = getenv("GCE_BAM_ZLIB_ONLY") != nullptr;
    if (level < 0 && !zlib_only) {                                            // level -1, "fastest": the fixed-Huffman encoder above
        const size_t clen = fastdef::deflate_fixed(src, n, dst + 18, 0x10000 - 18 - 8);
        if (clen) {
            const size_t total = 18 + clen + 8;
            const uint16_t bsize = (uint16_t)(total - 1);
            memcpy(dst + 16, &bsize, 2);
            const uint32_t crc = crc32_buf(src, n);
            memcpy(dst + 18 + clen, &crc, 4); memcpy(dst + 18 + clen + 4, &n, 4);
            return total;
        }
    }
    if (level < 0) level = 1;
    if (level > 9) level = 9;
    z_stream zs; memset(&zs, 0, sizeof zs);
    deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
    zs.next_in = const_cast<uint8_t *>(src); zs.avail_in = n; zs.next_out = dst + 18; zs.avail_out = 0x10000 - 18 - 8;
    int rc = deflate(&zs, Z_FINISH);
    if (rc != Z_STREAM_END) {                                                 // incompressible: store
        deflateEnd(&zs); memset(&zs, 0, sizeof zs);
        deflateInit2(&zs, 0, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        zs.next_in = const_cast<uint8_t *>(src); zs.avail_in = n; zs.next_out = dst + 18; zs.avail_out = 0x10000 - 18 - 8;
        rc = deflate(&zs, Z_FINISH);
    }
    const size_t clen = zs.total_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) return 0;                                         // (cannot happen for <= 0xff00 bytes stored; the caller reports it)
    const size_t total = 18 + clen + 8;
    const uint16_t bsize = (uint16_t)(total - 1);
    memcpy(dst + 16, &bsize, 2);
    const uint32_t crc = crc32_buf(src, n);
    memcpy(dst + 18 + clen, &crc, 4); memcpy(dst + 18 + clen + 4, &n, 4);
    return total;
}

}  // namespace
