// def_encode_best of gencore_amd/csrc/gce_deflate.hpp -- the function each lane of k_bgzf_deflate_dyn runs -- compiled for the HOST and checked
// against zlib as the decoder (tests/test_level_minus3.py): every block inflates to its input, under codes 1 it is never larger than the fixed-code
// encoder's block (the body of k_bgzf_deflate, rebuilt here from the same shared functions) and equals it byte for byte when no dynamic codes
// were chosen, and it fits its slot.  No kernel is launched.  Usage: deflate_host_check FILE...  (one line per file; exit 1 on any failure)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <zlib.h>
namespace { __device__ inline uint32_t inf_crc_word(const uint32_t (*)[256], uint32_t, uint64_t) { return 0; } }      // (def_frame's, device only: not called here)
#include "../gencore_amd/csrc/gce_deflate.hpp"

static uint16_t g_tab[1 << DEF_HBITS][DEF_T], g_cnt[DEF_CROWS][DEF_T];
static int fails = 0;

static uint32_t fixed_ref(const uint8_t *src, uint32_t n, uint8_t *out) {
    memset(g_tab, 0, sizeof g_tab);
    const DefCol tab = {g_tab, 3};
    DefBits b = {0, 0, out};
    b.put(3u, 3);
    for (uint32_t pos = 0; pos < n;) {
        uint32_t dist, code;
        const uint32_t len = def_match(src, pos, n, tab, dist);
        if (len >= 4u) {
            uint32_t eb, ev, deb, dev;
            const uint32_t sym = def_len_sym(len, eb, ev), dc = def_dist_sym(dist, deb, dev);
            const int l = def_fixed_code(sym, code);
            b.put(code, l); if (eb) b.put(ev, (int)eb);
            b.put(__builtin_bitreverse32(dc) >> 27, 5); if (deb) b.put(dev, (int)deb);
            pos += len;
        } else { const int l = def_fixed_code(src[pos], code); b.put(code, l); pos++; }
    }
    b.put(0u, 7); b.flush();
    uint32_t d = (uint32_t)(b.o - out);
    if (d > n + 5u) d = def_stored(src, n, out);
    return d;
}

static void one(const char *name, const uint8_t *src, uint32_t n, uint32_t blk, uint64_t *fix, uint64_t *best, uint64_t *ndyn) {
    const uint32_t slot = blk + blk / 8 + 64, cap = std::min(slot, 0x10000u) - 34u;
    std::vector<uint8_t> out(slot + 64), ref(slot + 64), back(n + 8);
    const uint32_t fx = fixed_ref(src, n, ref.data());
    for (int codes = 1; codes <= 2; codes++) {
        memset(g_tab, 0, sizeof g_tab); memset(g_cnt, 0xAB, sizeof g_cnt);
        const DefCol tab = {g_tab, 5}, cnt = {g_cnt, 5};
        const uint32_t d = def_encode_best(src, n, out.data(), cap, codes, tab, cnt);
        if (d + 26u + 4u > slot || d + 26u > 0x10000u) { printf("FAIL %s n=%u codes=%d: %u bytes do not fit\n", name, n, codes, d); fails++; continue; }
        z_stream zs; memset(&zs, 0, sizeof zs); inflateInit2(&zs, -15);
        zs.next_in = out.data(); zs.avail_in = d; zs.next_out = back.data(); zs.avail_out = n + 8;
        const int rc = inflate(&zs, Z_FINISH);
        if (rc != Z_STREAM_END || zs.total_out != n || zs.total_in != d || memcmp(back.data(), src, n)) { printf("FAIL %s n=%u codes=%d: zlib rc=%d %s\n", name, n, codes, rc, zs.msg ? zs.msg : ""); fails++; }
        inflateEnd(&zs);
        if (codes == 1) {
            const int bt = (out[0] >> 1) & 3;
            if (d > fx) { printf("FAIL %s n=%u: %u bytes, fixed codes %u\n", name, n, d, fx); fails++; }
            if (bt != 2 && (d != fx || memcmp(out.data(), ref.data(), d))) { printf("FAIL %s n=%u: BTYPE %d differs from the fixed-code encoder's bytes\n", name, n, bt); fails++; }
            *fix += fx; *best += d; *ndyn += bt == 2;
        }
    }
}

int main(int argc, char **argv) {
    const uint32_t blks[] = {1, 7, 300, 4096, 16384, 65279, 65280};
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { printf("FAIL cannot open %s\n", argv[a]); return 1; }
        std::vector<uint8_t> d(16u << 20); d.resize(fread(d.data(), 1, d.size(), f)); fclose(f);
        for (uint32_t blk : blks) {
            const size_t lim = blk < 300 ? std::min<size_t>(d.size(), 3000) : d.size();
            uint64_t fix = 0, best = 0, ndyn = 0;
            for (size_t at = 0; at < lim; at += blk) one(argv[a], d.data() + at, (uint32_t)std::min<size_t>(blk, lim - at), blk, &fix, &best, &ndyn);
            if (blk == 65280) printf("%s %zu %lu %lu %lu\n", argv[a], lim, (unsigned long)fix, (unsigned long)best, (unsigned long)ndyn);
        }
    }
    return fails != 0;
}
