// gce_deflate.hpp — the output record stream compressed into BGZF blocks ON THE GPU (SURVEY.md 8(f)1 "multi-threaded or GPU-assisted"; replaces
// bgzf_write's deflate under sam_write1, src/gencore.cpp:104 via htslib): the mirror of gce_inflate.hpp.  The stream in HBM is cut into blocks of
// <= 65 280 input bytes (as many as keep every CU busy: a block is an independent deflate stream, RFC 1951 inside the gzip framing of SAM spec
// 4.1), ONE LANE PER BLOCK, 32 blocks per workgroup:
//   * greedy LZ77 with one hash-table probe per position (the last place the next four bytes were seen: 2048 entries of 16 bits per lane, one
//     column of a 128 KB table in LDS -- one workgroup per CU), matches extended eight bytes at a time, up to 258 bytes, distances up to 32 768;
//   * FIXED Huffman codes (BTYPE 01): no code construction, literal / length / distance codes from the bit patterns of RFC 1951 3.2.6 computed with
//     v_bfrev and a count-leading-zeros each -- no tables; the bit stream leaves through a 64-bit buffer, four bytes a store;
//   * a block that fixed codes would expand (incompressible bytes: 9 bits per literal) is written STORED (BTYPE 00) instead;
//   * or (k_bgzf_deflate_dyn, level -3) DYNAMIC Huffman codes (BTYPE 10): the same lane runs the same matcher twice -- once to count the symbols,
//     once to emit -- and builds length-limited (12 bits) canonical codes in between, in its hash column; dynamic, fixed and stored are priced
//     exactly from the histogram and the smallest is written, so a block is never larger than under fixed codes;
//   * CRC-32 of the block's input (slicing-by-8, tables in LDS) and ISIZE in the trailer, BSIZE in the BGZF extra field.
// The blocks come out in slots of worst-case size; a prefix sum over their sizes and one gather make the file image the host writes.
// What it is for: the host's deflate is the largest stage of the file path that scales with the host (16 threads: 0.08 s for 230 MB at level 1;
// 4 threads: 0.3 s); this encoder takes a few milliseconds and leaves the host the write() alone.  Ratio: that of a greedy fixed-Huffman encoder
// (the library's host level -1 is the same scheme).
#pragma once

#define DEF_T 32
#define DEF_HBITS 11
// the hash table is sized for gfx950's 160 KB of LDS per CU (one 32-lane workgroup per CU holds 136 KB of it): this library is built for gfx950 only
static_assert((size_t)(1u << DEF_HBITS) * DEF_T * 2 + 8 * 256 * 4 <= 160u * 1024u, "k_bgzf_deflate: hash table + CRC tables must fit gfx950's 160 KB of LDS");
namespace {
typedef uint32_t def_u32u __attribute__((aligned(1)));
typedef uint64_t def_u64u __attribute__((aligned(1)));
typedef uint16_t def_u16u __attribute__((aligned(1)));

// this lane's column of a [rows][DEF_T] table of 16-bit entries in LDS (the hash table, the symbol counters)
struct DefCol {
    uint16_t (*t)[DEF_T]; int lane;
    __host__ __device__ uint16_t &operator[](uint32_t k) const { return t[k][lane]; }
};

// THE matcher of both encoders: the longest match (4..258 bytes, distance <= 32 768) at the one place the hash of the next four bytes was last
// seen, 0 = none; the position is entered into the table either way.  Both kernels cut a block into the same tokens because both call this.
__host__ __device__ inline uint32_t def_match(const uint8_t *src, uint32_t pos, uint32_t n, const DefCol &tab, uint32_t &dist) {
    uint32_t len = 0; dist = 0;
    if (pos + 4 <= n) {
        const uint32_t w4 = *(const def_u32u *)(src + pos);
        const uint32_t h = (w4 * 2654435761u) >> (32 - DEF_HBITS);
        const uint32_t cand = tab[h];
        tab[h] = (uint16_t)(pos + 1);
        if (cand != 0u) {
            const uint32_t c = cand - 1u;
            if (pos - c <= 32768u && *(const def_u32u *)(src + c) == w4) {
                const uint32_t lim = n - pos < 258u ? n - pos : 258u;
                len = 4; dist = pos - c;
                bool open = true;
                while (open && len + 8 <= lim) {
                    const uint64_t x = *(const def_u64u *)(src + c + len) ^ *(const def_u64u *)(src + pos + len);
                    if (x) { len += (uint32_t)(__builtin_ffsll((long long)x) - 1) >> 3; open = false; } else len += 8;
                }
                while (open && len < lim && src[c + len] == src[pos + len]) len++;
            }
        }
    }
    return len;
}
// length symbol (RFC 1951 3.2.5): 3..10 -> 257..264; beyond, 4 codes per number of extra bits; 258 -> 285
__host__ __device__ inline uint32_t def_len_sym(uint32_t len, uint32_t &eb, uint32_t &ev) {
    const uint32_t x = len - 3u;
    eb = 0; ev = 0;
    if (len == 258u) return 285u;
    if (x < 8u) return 257u + x;
    const uint32_t nb = 31u - (uint32_t)__builtin_clz(x);
    eb = nb - 2u; ev = x & ((1u << eb) - 1u);
    return 261u + 4u * eb + ((x >> eb) & 3u);
}
// distance code: 1..4 -> 0..3; beyond, 2 codes per number of extra bits
__host__ __device__ inline uint32_t def_dist_sym(uint32_t dist, uint32_t &deb, uint32_t &dev) {
    const uint32_t d = dist - 1u;
    deb = 0; dev = 0;
    if (d < 4u) return d;
    const uint32_t nb = 31u - (uint32_t)__builtin_clz(d);
    deb = nb - 1u; dev = d & ((1u << deb) - 1u);
    return 2u * nb + ((d >> deb) & 1u);
}
// the fixed code (RFC 1951 3.2.6) of a literal / length symbol, bit-reversed for the LSB-first stream; returns its length
__host__ __device__ inline int def_fixed_code(uint32_t sym, uint32_t &code) {
    if (sym < 144u) { code = __builtin_bitreverse32(0x30u + sym) >> 24; return 8; }
    if (sym < 256u) { code = __builtin_bitreverse32(0x190u + (sym - 144u)) >> 23; return 9; }
    if (sym < 280u) { code = __builtin_bitreverse32(sym - 256u) >> 25; return 7; }
    code = __builtin_bitreverse32(0xC0u + (sym - 280u)) >> 24; return 8;
}
// CRC-32 of the block's input, the 18-byte BGZF header in front of `dbytes` of deflate data at dst + 18, CRC and ISIZE behind: the member's size
// (inf_crc_word is gce_inflate.hpp's, which engine.hip includes first; tests/deflate_host_check.hip, which includes this file alone and never
// calls def_frame, declares a stand-in of the same signature -- keep the two in step)
__device__ inline uint32_t def_frame(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t dbytes, const uint32_t (*s_crc)[256]) {
    uint32_t crc = 0xFFFFFFFFu, k = 0;
    for (; k + 8 <= n; k += 8) crc = inf_crc_word(s_crc, crc, *(const def_u64u *)(src + k));
    for (; k < n; k++) crc = s_crc[0][(crc ^ src[k]) & 0xFF] ^ (crc >> 8);
    crc = ~crc;
    const uint32_t bsize = 18u + dbytes + 8u;
    const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int j = 0; j < 16; j++) dst[j] = hdr[j];
    dst[16] = (uint8_t)(bsize - 1u); dst[17] = (uint8_t)((bsize - 1u) >> 8);
    uint8_t *t = dst + 18 + dbytes;
    *(def_u32u *)t = crc; *(def_u32u *)(t + 4) = n;
    return bsize;
}
// one stored block (BFINAL, BTYPE 00; LEN, NLEN, the bytes): n + 5 bytes
__host__ __device__ inline uint32_t def_stored(const uint8_t *src, uint32_t n, uint8_t *q) {
    q[0] = 1; q[1] = (uint8_t)n; q[2] = (uint8_t)(n >> 8); q[3] = (uint8_t)~n; q[4] = (uint8_t)(~n >> 8);
    uint32_t k = 0;
    for (; k + 8 <= n; k += 8) *(def_u64u *)(q + 5 + k) = *(const def_u64u *)(src + k);
    for (; k < n; k++) q[5 + k] = src[k];
    return n + 5u;
}

__global__ __launch_bounds__(DEF_T) void k_bgzf_deflate(const uint8_t *in, uint64_t total, uint32_t blk, uint32_t n_blocks, uint8_t *slots, uint32_t slot_bytes, uint32_t *sizes) {
    __shared__ uint16_t s_tab[1 << DEF_HBITS][DEF_T];                                 // last position + 1 of a 4-byte hash, one column per lane
    __shared__ uint32_t s_crc[8][256];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += DEF_T) {                                         // CRC-32 (reflected 0xEDB88320), slicing-by-8 tables
        uint32_t c = (uint32_t)k;
        for (int j = 0; j < 8; j++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
        s_crc[0][k] = c;
    }
    __syncthreads();
    for (int k = lane; k < 256; k += DEF_T) { uint32_t c = s_crc[0][k]; for (int t = 1; t < 8; t++) { c = s_crc[0][c & 0xFF] ^ (c >> 8); s_crc[t][k] = c; } }
    for (int k = 0; k < (1 << DEF_HBITS); k++) s_tab[k][lane] = 0;
    __syncthreads();
    const uint32_t bi = blockIdx.x * DEF_T + (uint32_t)lane;
    if (bi >= n_blocks) return;
    const uint8_t *src = in + (uint64_t)bi * blk;
    const uint32_t n = (uint32_t)min((uint64_t)blk, total - (uint64_t)bi * blk);
    uint8_t *dst = slots + (uint64_t)bi * slot_bytes, *o = dst + 18;
    const DefCol tab = {s_tab, lane};
    uint64_t bb = 0; int bc = 0;
    auto put = [&](uint32_t v, int nb) {                                              // nb <= 13 bits, LSB first
        bb |= (uint64_t)v << bc; bc += nb;
        if (bc >= 32) { *(def_u32u *)o = (uint32_t)bb; o += 4; bb >>= 32; bc -= 32; }
    };
    put(3u, 3);                                                                       // BFINAL = 1, BTYPE = 01 (bits 1, then 1 0)
    uint32_t pos = 0;
    while (pos < n) {
        uint32_t dist;
        const uint32_t len = def_match(src, pos, n, tab, dist);
        if (len >= 4) {
            uint32_t eb, ev, deb, dev;
            const uint32_t sym = def_len_sym(len, eb, ev), dc = def_dist_sym(dist, deb, dev);
            if (sym < 280u) put(__brev(sym - 256u) >> 25, 7); else put(__brev(0xC0u + (sym - 280u)) >> 24, 8);
            if (eb) put(ev, (int)eb);
            put(__brev(dc) >> 27, 5);
            if (deb) put(dev, (int)deb);
            pos += len;
        } else {
            const uint32_t lit = src[pos];
            if (lit < 144u) put(__brev(0x30u + lit) >> 24, 8); else put(__brev(0x190u + (lit - 144u)) >> 23, 9);
            pos++;
        }
    }
    put(0u, 7);                                                                       // end of block (symbol 256)
    while (bc > 0) { *o++ = (uint8_t)bb; bb >>= 8; bc -= 8; }
    uint32_t dbytes = (uint32_t)(o - (dst + 18));
    if (dbytes > n + 5u) dbytes = def_stored(src, n, dst + 18);                       // fixed codes expanded it: one stored block
    sizes[bi] = def_frame(src, n, dst, dbytes, s_crc);
}
// block bi of the file image = its slot's first sizes[bi] bytes, at off[bi]: a wave per block
__global__ __launch_bounds__(256) void k_deflate_pack(const uint8_t *slots, uint32_t slot_bytes, const uint32_t *sizes, const uint64_t *off, uint32_t n_blocks, uint8_t *out) {
    const int lane = threadIdx.x & 63;
    for (uint32_t bi = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; bi < n_blocks; bi += (gridDim.x * blockDim.x) >> 6) {
        const uint8_t *s = slots + (uint64_t)bi * slot_bytes; uint8_t *d = out + off[bi]; const uint32_t sz = sizes[bi];
        for (uint32_t j = 8u * (uint32_t)lane; j < sz; j += 512u) {
            if (j + 8 <= sz) *(def_u64u *)(d + j) = *(const def_u64u *)(s + j);
            else for (uint32_t q = j; q < sz; q++) d[q] = s[q];
        }
    }
}

// ---- dynamic Huffman codes (BTYPE 10): structure (a) of DESIGN.md 4b -- still one lane per block, the matcher run TWICE: once to count the 286
// literal / length and 30 distance symbols, once (over a cleared hash column) to emit with the codes built in between.  No token buffer.
// Between the two runs the lane's hash column (2048 entries) is free and is the code builder's workspace; the counters (16 bits: a count cannot
// exceed 65 280) become (bit-reversed code << 4 | length) for the second run, which is why codes are limited to DEF_MAXBITS = 12 bits, not 15:
// 12 + 4 = 16, and RFC 1951 allows any limit up to 15.
#define DEF_NLL 286
#define DEF_ND 30
#define DEF_CROWS 320                                                                  // 286 + 30 counters, rounded up
#define DEF_MAXBITS 12
static_assert((size_t)(1u << DEF_HBITS) * DEF_T * 2 + 8 * 256 * 4 + (size_t)DEF_CROWS * DEF_T * 2 <= 160u * 1024u, "k_bgzf_deflate_dyn: hash table + CRC tables + counters must fit gfx950's 160 KB of LDS");
// the workspace in the hash column: code lengths of the 316 symbols, sort keys / symbols (twice: the radix sort's two sides), its histogram, counts per
// length and first codes, the code length alphabet's counters (then codes) and lengths
enum { DW_LEN = 0, DW_KEY = 320, DW_SYM = 608, DW_KEY2 = 896, DW_SYM2 = 1184, DW_HIST = 1472, DW_NUM = 1728, DW_CLF = 1760, DW_CLL = 1780, DW_END = 1800 };
static_assert(DW_END <= (1 << DEF_HBITS), "the code builder's workspace must fit the hash column");

struct DefBits {                                                                        // the bit stream: LSB first, through a 64-bit buffer, four bytes a store
    uint64_t bb; int bc; uint8_t *o;
    __host__ __device__ void put(uint32_t v, int nb) {                                 // nb <= 32
        bb |= (uint64_t)v << bc; bc += nb;
        if (bc >= 32) { *(def_u32u *)o = (uint32_t)bb; o += 4; bb >>= 32; bc -= 32; }
    }
    __host__ __device__ void flush() { while (bc > 0) { *o++ = (uint8_t)bb; bb >>= 8; bc -= 8; } }
};

// Length-limited code lengths of the `nsym` symbols counted in f[f0 ..): w[l0 + s] = 0 (unused) or 1..maxbits, a COMPLETE code.  Sort the used
// symbols by count (LSD radix sort, 8 bits a pass), Moffat & Katajainen's in-place minimum-redundancy lengths over the sorted counts (every
// intermediate sum <= the block's symbol total <= 65 281: 16 bits hold it), then the counts per length are bent under `maxbits` until the Kraft sum
// is 1 again and the lengths are dealt out, longest to the rarest.  Fewer than two used symbols: two codes of one bit, as zlib's encoder does (one
// distance code needs a bit anyway; every decoder takes a complete code).
__host__ __device__ inline void def_build_lengths(const DefCol &f, uint32_t f0, uint32_t nsym, uint32_t maxbits, const DefCol &w, uint32_t l0) {
    uint32_t m = 0, maxk = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        w[l0 + s] = 0;
        const uint32_t c = f[f0 + s];
        if (c) { w[DW_KEY + m] = (uint16_t)c; w[DW_SYM + m] = (uint16_t)s; m++; if (c > maxk) maxk = c; }
    }
    if (m < 2u) { const uint32_t a = m ? (uint32_t)w[DW_SYM] : 0u; w[l0 + a] = 1; w[l0 + (a ? 0u : 1u)] = 1; return; }
    uint32_t ka = DW_KEY, sa = DW_SYM, kb = DW_KEY2, sb = DW_SYM2;
    for (uint32_t shift = 0; shift < 16u; shift += 8u) {
        if (shift && maxk < 256u) break;
        for (uint32_t k = 0; k < 256u; k++) w[DW_HIST + k] = 0;
        for (uint32_t i = 0; i < m; i++) w[DW_HIST + ((w[ka + i] >> shift) & 255u)]++;
        uint32_t acc = 0;
        for (uint32_t k = 0; k < 256u; k++) { const uint32_t c = w[DW_HIST + k]; w[DW_HIST + k] = (uint16_t)acc; acc += c; }
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t k = w[ka + i], d = (k >> shift) & 255u, p = w[DW_HIST + d];
            w[DW_HIST + d] = (uint16_t)(p + 1u); w[kb + p] = (uint16_t)k; w[sb + p] = w[sa + i];
        }
        uint32_t t = ka; ka = kb; kb = t; t = sa; sa = sb; sb = t;
    }
#define DEF_A(i) w[ka + (uint32_t)(i)]
    const int mi = (int)m;
    DEF_A(0) = (uint16_t)(DEF_A(0) + DEF_A(1));
    int root = 0, leaf = 2, next;
    for (next = 1; next < mi - 1; next++) {
        if (leaf >= mi || DEF_A(root) < DEF_A(leaf)) { DEF_A(next) = DEF_A(root); DEF_A(root) = (uint16_t)next; root++; } else { DEF_A(next) = DEF_A(leaf); leaf++; }
        if (leaf >= mi || (root < next && DEF_A(root) < DEF_A(leaf))) { DEF_A(next) = (uint16_t)(DEF_A(next) + DEF_A(root)); DEF_A(root) = (uint16_t)next; root++; }
        else { DEF_A(next) = (uint16_t)(DEF_A(next) + DEF_A(leaf)); leaf++; }
    }
    DEF_A(mi - 2) = 0;
    for (next = mi - 3; next >= 0; next--) DEF_A(next) = (uint16_t)(DEF_A(DEF_A(next)) + 1u);
    int avbl = 1, used = 0, dpth = 0;
    root = mi - 2; next = mi - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)DEF_A(root) == dpth) { used++; root--; }
        while (avbl > used) { DEF_A(next) = (uint16_t)dpth; next--; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
    for (uint32_t k = 0; k <= maxbits; k++) w[DW_NUM + k] = 0;
    for (uint32_t i = 0; i < m; i++) { uint32_t l = DEF_A(i); if (l > maxbits) l = maxbits; w[DW_NUM + l]++; }
#undef DEF_A
    uint32_t total = 0;
    for (uint32_t k = maxbits; k >= 1u; k--) total += (uint32_t)w[DW_NUM + k] << (maxbits - k);
    while (total > (1u << maxbits)) {                                                   // over-subscribed by the clamp: one code of maxbits fewer, a shorter one a bit longer
        w[DW_NUM + maxbits]--;
        for (uint32_t k = maxbits - 1u; k >= 1u; k--) if (w[DW_NUM + k]) { w[DW_NUM + k]--; w[DW_NUM + k + 1u] += 2; break; }
        total--;
    }
    uint32_t i = 0;
    for (uint32_t k = maxbits; k >= 1u; k--) for (uint32_t c = w[DW_NUM + k]; c > 0u; c--) { w[l0 + w[sa + i]] = (uint16_t)k; i++; }
}
// canonical codes (RFC 1951 3.2.2) of the lengths w[l0 ..): out[o0 + s] = bit-reversed code << 4 | length
__host__ __device__ inline void def_assign_codes(const DefCol &w, uint32_t l0, uint32_t nsym, const DefCol &out, uint32_t o0) {
    for (uint32_t k = 0; k < 32u; k++) w[DW_NUM + k] = 0;
    for (uint32_t s = 0; s < nsym; s++) w[DW_NUM + w[l0 + s]]++;
    w[DW_NUM] = 0;
    uint32_t code = 0;
    for (uint32_t k = 1; k <= 15u; k++) { code = (code + w[DW_NUM + k - 1u]) << 1; w[DW_NUM + 16u + k] = (uint16_t)code; }
    for (uint32_t s = 0; s < nsym; s++) {
        const uint32_t l = w[l0 + s];
        uint32_t e = 0;
        if (l) { const uint32_t c = w[DW_NUM + 16u + l]; w[DW_NUM + 16u + l] = (uint16_t)(c + 1u); e = (__builtin_bitreverse32(c) >> (32u - l)) << 4 | l; }
        out[o0 + s] = (uint16_t)e;
    }
}
// the code length sequence of a dynamic header (the first hlit literal / length lengths, then hdist distance lengths, as ONE sequence: runs cross the
// border) in the symbols of 3.2.7: f(symbol, extra value, extra bits)
template <class F> __host__ __device__ inline void def_rle(const DefCol &w, uint32_t hlit, uint32_t hdist, F f) {
    const uint32_t total = hlit + hdist;
    auto seq = [&](uint32_t i) -> uint32_t { return w[DW_LEN + (i < hlit ? i : DEF_NLL + i - hlit)]; };
    uint32_t i = 0;
    while (i < total) {
        const uint32_t v = seq(i);
        uint32_t run = 1;
        while (i + run < total && seq(i + run) == v) run++;
        i += run;
        if (v == 0u) {
            while (run >= 11u) { const uint32_t r = run < 138u ? run : 138u; f(18u, r - 11u, 7); run -= r; }
            if (run >= 3u) { f(17u, run - 3u, 3); run = 0; }
        } else {
            f(v, 0u, 0); run--;
            while (run >= 3u) { const uint32_t r = run < 6u ? run : 6u; f(16u, r - 3u, 2); run -= r; }
        }
        while (run > 0u) { f(v, 0u, 0); run--; }
    }
}

// One block -> its deflate data at `out`, the smallest of dynamic codes (header included), fixed codes and stored, each PRICED EXACTLY from the
// histogram before a byte is written: never larger than k_bgzf_deflate's (same tokens, and its two candidates are among the three).  tab: a zeroed
// hash column; cnt: DEF_CROWS counters.  codes 2: dynamic codes whenever they fit `cap` bytes (tests: the degenerate trees, which are never the
// smallest).  Returns the bytes written (<= n + 5 for codes 1, <= cap for codes 2).
__host__ __device__ inline uint32_t def_encode_best(const uint8_t *src, uint32_t n, uint8_t *out, uint32_t cap, int codes, const DefCol &tab, const DefCol &cnt) {
    for (uint32_t s = 0; s < DEF_CROWS; s++) cnt[s] = 0;
    for (uint32_t pos = 0; pos < n;) {                                                  // run 1: count
        uint32_t dist, x, y;
        const uint32_t len = def_match(src, pos, n, tab, dist);
        if (len >= 4u) { cnt[def_len_sym(len, x, y)]++; cnt[DEF_NLL + def_dist_sym(dist, x, y)]++; pos += len; }
        else { cnt[src[pos]]++; pos++; }
    }
    cnt[256] = 1;                                                                       // end of block, once
    // extra bits of lengths and distances (the same under either code), the fixed codes' price
    uint32_t xbits = 0, fixed_bits = 3;
    for (uint32_t s = 0; s < DEF_NLL; s++) {
        const uint32_t c = cnt[s];
        fixed_bits += c * (s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
        if (s >= 265u && s < 285u) xbits += c * ((s - 261u) >> 2);
    }
    for (uint32_t d = 0; d < DEF_ND; d++) { const uint32_t c = cnt[DEF_NLL + d]; fixed_bits += 5u * c; if (d >= 4u) xbits += c * ((d >> 1) - 1u); }
    fixed_bits += xbits;
    // the dynamic codes and their price
    const DefCol &w = tab;
    def_build_lengths(cnt, 0, DEF_NLL, DEF_MAXBITS, w, DW_LEN);
    def_build_lengths(cnt, DEF_NLL, DEF_ND, DEF_MAXBITS, w, DW_LEN + DEF_NLL);
    uint32_t hlit = DEF_NLL, hdist = DEF_ND;
    while (hlit > 257u && w[DW_LEN + hlit - 1u] == 0) hlit--;
    while (hdist > 1u && w[DW_LEN + DEF_NLL + hdist - 1u] == 0) hdist--;
    for (uint32_t k = 0; k < 19u; k++) w[DW_CLF + k] = 0;
    uint32_t hdr_x = 0;
    def_rle(w, hlit, hdist, [&](uint32_t s, uint32_t, int xb) { w[DW_CLF + s]++; hdr_x += (uint32_t)xb; });
    def_build_lengths(w, DW_CLF, 19, 7, w, DW_CLL);
    const uint8_t ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hclen = 19;
    while (hclen > 4u && w[DW_CLL + ord[hclen - 1u]] == 0) hclen--;
    uint32_t dyn_bits = 3u + 5u + 5u + 4u + 3u * hclen + hdr_x + xbits;
    for (uint32_t k = 0; k < 19u; k++) dyn_bits += (uint32_t)w[DW_CLF + k] * w[DW_CLL + k];
    for (uint32_t s = 0; s < DEF_NLL + DEF_ND; s++) dyn_bits += (uint32_t)cnt[s] * w[DW_LEN + s];
    const uint32_t dyn_bytes = (dyn_bits + 7u) >> 3, fixed_bytes = (fixed_bits + 7u) >> 3, stored_bytes = n + 5u;
    const bool dyn = codes == 2 ? dyn_bytes <= cap : (dyn_bytes < fixed_bytes && dyn_bytes < stored_bytes);
    if (!dyn && fixed_bytes > stored_bytes) return def_stored(src, n, out);
    DefBits b = {0, 0, out};
    if (dyn) {
        b.put(5u, 3);                                                                   // BFINAL = 1, BTYPE = 10
        b.put(hlit - 257u, 5); b.put(hdist - 1u, 5); b.put(hclen - 4u, 4);
        for (uint32_t k = 0; k < hclen; k++) b.put(w[DW_CLL + ord[k]], 3);
        def_assign_codes(w, DW_CLL, 19, w, DW_CLF);
        def_rle(w, hlit, hdist, [&](uint32_t s, uint32_t xv, int xb) { const uint32_t e = w[DW_CLF + s]; b.put(e >> 4, (int)(e & 15u)); if (xb) b.put(xv, xb); });
        def_assign_codes(w, DW_LEN, DEF_NLL, cnt, 0);
        def_assign_codes(w, DW_LEN + DEF_NLL, DEF_ND, cnt, DEF_NLL);
    } else b.put(3u, 3);                                                                // BFINAL = 1, BTYPE = 01
    for (uint32_t k = 0; k < (1u << DEF_HBITS); k++) tab[k] = 0;
    for (uint32_t pos = 0; pos < n;) {                                                  // run 2: the same tokens, emitted
        uint32_t dist;
        const uint32_t len = def_match(src, pos, n, tab, dist);
        if (len >= 4u) {
            uint32_t eb, ev, deb, dev, code;
            const uint32_t sym = def_len_sym(len, eb, ev), dc = def_dist_sym(dist, deb, dev);
            if (dyn) { const uint32_t e = cnt[sym]; b.put(e >> 4, (int)(e & 15u)); } else { const int l = def_fixed_code(sym, code); b.put(code, l); }
            if (eb) b.put(ev, (int)eb);
            if (dyn) { const uint32_t e = cnt[DEF_NLL + dc]; b.put(e >> 4, (int)(e & 15u)); } else b.put(__builtin_bitreverse32(dc) >> 27, 5);
            if (deb) b.put(dev, (int)deb);
            pos += len;
        } else {
            const uint32_t lit = src[pos];
            uint32_t code;
            if (dyn) { const uint32_t e = cnt[lit]; b.put(e >> 4, (int)(e & 15u)); } else { const int l = def_fixed_code(lit, code); b.put(code, l); }
            pos++;
        }
    }
    if (dyn) { const uint32_t e = cnt[256]; b.put(e >> 4, (int)(e & 15u)); } else b.put(0u, 7);      // end of block
    b.flush();
    return (uint32_t)(b.o - out);
}

// codes 1: the smallest of dynamic / fixed / stored per block; 2: dynamic wherever it fits the slot.  Launch like k_bgzf_deflate.
__global__ __launch_bounds__(DEF_T) void k_bgzf_deflate_dyn(const uint8_t *in, uint64_t total, uint32_t blk, uint32_t n_blocks, uint8_t *slots, uint32_t slot_bytes, uint32_t *sizes, int codes) {
    __shared__ uint16_t s_tab[1 << DEF_HBITS][DEF_T];
    __shared__ uint16_t s_cnt[DEF_CROWS][DEF_T];
    __shared__ uint32_t s_crc[8][256];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += DEF_T) {                                         // CRC-32 (reflected 0xEDB88320), slicing-by-8 tables
        uint32_t c = (uint32_t)k;
        for (int j = 0; j < 8; j++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
        s_crc[0][k] = c;
    }
    __syncthreads();
    for (int k = lane; k < 256; k += DEF_T) { uint32_t c = s_crc[0][k]; for (int t = 1; t < 8; t++) { c = s_crc[0][c & 0xFF] ^ (c >> 8); s_crc[t][k] = c; } }
    for (int k = 0; k < (1 << DEF_HBITS); k++) s_tab[k][lane] = 0;
    __syncthreads();
    const uint32_t bi = blockIdx.x * DEF_T + (uint32_t)lane;
    if (bi >= n_blocks) return;
    const uint8_t *src = in + (uint64_t)bi * blk;
    const uint32_t n = (uint32_t)min((uint64_t)blk, total - (uint64_t)bi * blk);
    uint8_t *dst = slots + (uint64_t)bi * slot_bytes;
    const DefCol tab = {s_tab, lane}, cnt = {s_cnt, lane};
    // forced dynamic codes (codes 2) must fit the slot (8: the bit writer stores four bytes at a time) AND a BGZF member: BSIZE - 1 is 16 bits
    const uint32_t cap = min(slot_bytes, 0x10000u) - 18u - 8u - 8u;
    const uint32_t dbytes = def_encode_best(src, n, dst + 18, cap, codes, tab, cnt);
    sizes[bi] = def_frame(src, n, dst, dbytes, s_crc);
}
}  // namespace
