// samfmt::format_record, samfmt::emit_seq and samfmt::walk_records of gencore_amd/csrc/gce_samfmt.hpp -- what each thread of k_samfmt_size /
// k_samfmt_core and each 16-lane group of k_samfmt_seq runs -- compiled for the HOST and checked against samtext::bam_to_line
// (tests/test_samfmt_model.py): per record the verdict, the line's length and, for a record without floating-point values, every byte of the
// line; a record with such a value must be listed for the host and not refused.  The group is stood in for twice: by one lane, and by 16
// lanes one after another, with the line's first byte at every offset 0..15 modulo 16.  Every record is handed over in a heap block of exactly
// its frame's size, so a host sanitizer sees a read past it.  No kernel is launched.
// Usage: samfmt_host_check NAMES TEXT FRAMES OUT
//   NAMES: one contig per line; TEXT: alignment lines, made records by samtext::line_to_bam; FRAMES: further records, each behind a 32-bit
//   length of the bytes that are there (a frame may be shorter than its block_size says); OUT: the lines of the good records, in order.
//   One output line per record: "<index> ok <length> <host>" or "<index> bad"; exit 1 on any failure.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#define GCE_SAMFMT_HOST_CHECK
#include "../gencore_amd/csrc/gce_samfmt.hpp"
#include "../gencore_amd/csrc/gce_samtext.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

// a record bam_to_line accepted: does an optional field hold an f, d or B:f value
static bool holds_float(const std::vector<uint8_t> &r) {
    uint32_t bs, lseq; uint16_t nc; memcpy(&bs, &r[0], 4); memcpy(&lseq, &r[20], 4); memcpy(&nc, &r[16], 2);
    size_t p = 36 + r[12] + 4u * nc + (lseq + 1) / 2 + lseq; const size_t end = 4 + (size_t)bs;
    while (p + 3 <= end) {
        const uint8_t t = r[p + 2]; p += 3;
        if (t == 'f' || t == 'd') return true;
        if (t == 'A' || t == 'c' || t == 'C') p += 1; else if (t == 's' || t == 'S') p += 2; else if (t == 'i' || t == 'I') p += 4;
        else if (t == 'Z' || t == 'H') { while (r[p]) p++; p++; }
        else { const uint8_t sub = r[p]; uint32_t cnt; memcpy(&cnt, &r[p + 1], 4); if (sub == 'f') return true; p += 5 + (size_t)cnt * ((sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4); }
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    std::vector<std::string> names;
    { std::istringstream f(slurp(argv[1])); std::string l; while (std::getline(f, l)) if (!l.empty()) names.push_back(l); }
    const std::string text = slurp(argv[2]), framed = slurp(argv[3]);
    samtext::NameMap nmap; nmap.build(names);
    std::vector<uint8_t> blob; std::vector<uint32_t> off;
    for (const std::string &x : names) { off.push_back((uint32_t)blob.size()); blob.insert(blob.end(), x.begin(), x.end()); }
    off.push_back((uint32_t)blob.size()); blob.push_back(0);
    const samfmt::Names nm = {blob.data(), off.data(), (int32_t)names.size()};
    const uint8_t *codes = (const uint8_t *)"=ACMGRSVTWYHKDBN";

    std::vector<std::vector<uint8_t>> frames;
    for (size_t x = 0; x < text.size();) {
        const char *q = (const char *)memchr(text.data() + x, '\n', text.size() - x); const size_t le = q ? (size_t)(q - text.data()) : text.size();
        if (le > x) {
            std::vector<uint8_t> rec; std::string msg;
            if (!samtext::line_to_bam(text.data() + x, text.data() + le, nmap, rec, msg)) { printf("FAIL text line at byte %zu: %s\n", x, msg.c_str()); return 1; }
            frames.push_back(rec);
        }
        x = le + 1;
    }
    for (size_t x = 0; x + 4 <= framed.size();) {
        uint32_t fl; memcpy(&fl, framed.data() + x, 4); x += 4;
        if (x + fl > framed.size()) { printf("FAIL frame file\n"); return 1; }
        frames.emplace_back(framed.begin() + (ptrdiff_t)x, framed.begin() + (ptrdiff_t)(x + fl)); x += fl;
    }

    int fails = 0; std::string all_lines; std::vector<uint8_t> chain; std::vector<uint64_t> chain_start;
    for (size_t i = 0; i < frames.size(); i++) {
        const std::vector<uint8_t> &f = frames[i];
        std::unique_ptr<uint8_t[]> heap(new uint8_t[f.size() ? f.size() : 1]);
        if (!f.empty()) memcpy(heap.get(), f.data(), f.size());
        // the host's verdict: bam_to_line takes a record that is whole (its caller's walk checked block_size against the buffer)
        uint32_t bs = 0; if (f.size() >= 4) memcpy(&bs, f.data(), 4);
        std::string want;
        const bool whole = f.size() >= 4 && bs >= 32 && 4ull + bs <= f.size();
        const bool ok = whole && samtext::bam_to_line(f.data(), names, want);
        samfmt::Rec L;
        samfmt::format_record<false>(heap.get(), f.size(), nm, nullptr, L);
        bool good = ok == !L.bad;
        const bool has_float = ok && holds_float(f);
        if (ok && good) good = (L.host != 0) == has_float && (L.host || L.size == want.size());
        if (ok && good && !L.host) {
            for (int groups = 0; groups < 2 && good; groups++) for (uint32_t al = 0; al < 16 && good; al++) {
                std::vector<uint8_t> buf(want.size() + 64, 0xA5);
                uint8_t *o = buf.data() + ((16 - ((uintptr_t)buf.data() & 15)) & 15) + 16 + al;        // the line's first byte at every alignment
                samfmt::Rec E;
                samfmt::format_record<true>(heap.get(), f.size(), nm, o, E);
                const uint32_t nl = groups ? 16u : 1u;
                if (!E.bad && E.lseq) {
                    const uint8_t *c = heap.get() + 4; uint16_t nc; memcpy(&nc, c + 12, 2);
                    const uint8_t *sq = c + 32 + c[8] + 4u * nc;
                    for (uint32_t lane = 0; lane < nl; lane++) samfmt::emit_seq(sq, sq + (E.lseq + 1) / 2, o + E.oseq, E.lseq, lane, nl, codes);
                }
                good = !E.bad && !E.host && E.size == want.size() && E.oseq == L.oseq && E.lseq == L.lseq && o[want.size()] == 0xA5 && o[-1] == 0xA5 && memcmp(o, want.data(), want.size()) == 0;
                for (size_t k = 0; good && k < 16 + al; k++) good = o[-(ptrdiff_t)k - 1] == 0xA5;
                for (size_t k = want.size(); good && o + k < buf.data() + buf.size(); k++) good = o[k] == 0xA5;
            }
        }
        if (!good) { fails++; printf("FAIL record %zu: host %s %zu, device %s %llu host=%u\n", i, ok ? "ok" : "bad", want.size(), L.bad ? "bad" : "ok", (unsigned long long)L.size, L.host); }
        else if (ok) printf("%zu ok %zu %u\n", i, want.size(), L.host);
        else printf("%zu bad\n", i);
        if (ok) { all_lines += want; chain_start.push_back(chain.size()); chain.insert(chain.end(), f.begin(), f.begin() + 4 + bs); }
    }
    {   // the walk over the good records back to back; then with a record of block_size 31, a cut record and two stray bytes behind them
        std::vector<uint64_t> st(chain_start.size() + 1, ~0ull); uint64_t nr = 0; int64_t bad = 0;
        samfmt::walk_records(chain.data(), chain.size(), nullptr, 0, nr, bad);
        bool good = nr == chain_start.size() && bad == -1;
        samfmt::walk_records(chain.data(), chain.size(), st.data(), chain_start.size(), nr, bad);
        good = good && nr == chain_start.size() && bad == -1 && st[nr] == chain.size();
        for (size_t k = 0; good && k < chain_start.size(); k++) good = st[k] == chain_start[k];
        const size_t n0 = chain.size();
        for (int v = 0; v < 3 && good; v++) {
            std::vector<uint8_t> c2 = chain;
            if (v == 0) { const uint32_t b31 = 31; c2.insert(c2.end(), (const uint8_t *)&b31, (const uint8_t *)&b31 + 4); c2.resize(c2.size() + 31, 0); }
            else if (v == 1) { const uint32_t b40 = 40; c2.insert(c2.end(), (const uint8_t *)&b40, (const uint8_t *)&b40 + 4); c2.resize(c2.size() + 39, 0); }
            else c2.resize(c2.size() + 2, 0);
            std::unique_ptr<uint8_t[]> h2(new uint8_t[c2.size()]); memcpy(h2.get(), c2.data(), c2.size());
            std::vector<uint64_t> s2(chain_start.size() + 1, ~0ull);
            samfmt::walk_records(h2.get(), c2.size(), s2.data(), chain_start.size(), nr, bad);
            good = nr == chain_start.size() && bad == (int64_t)chain_start.size() && s2[nr] == n0;
        }
        if (!good) { fails++; printf("FAIL walk_records\n"); }
    }
    { std::ofstream f(argv[4], std::ios::binary); f.write(all_lines.data(), (std::streamsize)all_lines.size()); }
    return fails ? 1 : 0;
}
