// samdev::parse_line and samdev::emit_seq of gencore_amd/csrc/gce_samdev.hpp -- what each thread of k_sam_size / k_sam_emit_core and each
// 16-lane group of k_sam_emit_seq runs -- compiled for the HOST and checked against samtext::line_to_bam (tests/test_sort_sam_model.py): per line
// the verdict (line_to_bam's message), the size and, for a line without floating-point values, every byte of the record; a line with such a
// value must be listed for the host, have line_to_bam's size and line_to_bam's bytes everywhere outside those values (which the device zeroes).  The group is stood in for twice: by one lane, and by 16 lanes one after
// another, at every alignment of the record's first byte.  No kernel is launched.
// Usage: samdev_host_check NAMES TEXT   (NAMES: one contig per line; TEXT: alignment lines; one output line per line; exit 1 on any failure)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>
#define GCE_SAMDEV_HOST_CHECK
#include "../gencore_amd/csrc/gce_samdev.hpp"
#include "../gencore_amd/csrc/gce_samtext.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

// the f / d / B:f values of a record's optional fields (from byte `a` on) zeroed; false: the fields do not parse
static bool zero_floats(std::vector<uint8_t> &r, size_t a) {
    size_t p = a; bool any = false;
    while (p < r.size()) {
        if (p + 3 > r.size()) return false;
        const uint8_t t = r[p + 2]; p += 3;
        size_t n = 0;
        if (t == 'A' || t == 'c' || t == 'C') n = 1; else if (t == 's' || t == 'S') n = 2; else if (t == 'i' || t == 'I') n = 4;
        else if (t == 'f') { n = 4; memset(&r[p], 0, 4); any = true; }
        else if (t == 'd') { n = 8; memset(&r[p], 0, 8); any = true; }
        else if (t == 'Z' || t == 'H') { while (p + n < r.size() && r[p + n]) n++; n++; }
        else if (t == 'B') {
            if (p + 5 > r.size()) return false;
            const uint8_t sub = r[p]; uint32_t cnt; memcpy(&cnt, &r[p + 1], 4);
            const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            p += 5; n = es * (size_t)cnt;
            if (sub == 'f' && p + n <= r.size()) { memset(r.data() + p, 0, n); any = true; }
        } else return false;
        if (p + n > r.size()) return false;
        p += n;
    }
    return any;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::vector<std::string> names;
    { std::istringstream f(slurp(argv[1])); std::string l; while (std::getline(f, l)) if (!l.empty()) names.push_back(l); }
    const std::string text = slurp(argv[2]);
    samtext::NameMap nm; nm.build(names);
    // the device's table: names sorted as byte strings, the first of equal names
    std::vector<uint32_t> idx(names.size()); std::iota(idx.begin(), idx.end(), 0u);
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { const int c = names[a].compare(names[b]); return c < 0 || (c == 0 && a < b); });
    std::vector<uint8_t> blob; std::vector<uint32_t> off; std::vector<int32_t> tid;
    for (size_t k = 0; k < idx.size(); k++) {
        if (k && names[idx[k]] == names[idx[k - 1]]) continue;
        off.push_back((uint32_t)blob.size()); tid.push_back((int32_t)idx[k]); blob.insert(blob.end(), names[idx[k]].begin(), names[idx[k]].end());
    }
    off.push_back((uint32_t)blob.size()); blob.push_back(0);
    const samdev::Contigs cg = {blob.data(), off.data(), tid.data(), (int32_t)tid.size()};
    uint8_t t16[256]; for (int k = 0; k < 256; k++) t16[k] = samdev::nt16((uint32_t)k);
    for (int k = 0; k < 256; k++) if (t16[k] != samtext::nt16_table()[k]) { printf("FAIL nt16 %d\n", k); return 1; }
    int fails = 0; size_t line = 0;
    const uint8_t *d = (const uint8_t *)text.data(); const size_t n = text.size();
    for (size_t x = 0; x < n; line++) {
        const uint8_t *q = (const uint8_t *)memchr(d + x, '\n', n - x); const size_t le = q ? (size_t)(q - d) : n;
        if (le > x && !(le == x + 1 && d[x] == '\r')) {
            std::vector<uint8_t> want; std::string msg;
            const bool ok = samtext::line_to_bam((const char *)d + x, (const char *)d + le, nm, want, msg);
            samdev::Line L;
            samdev::parse_line<false>(d + x, d + le, cg, nullptr, L);
            const char *got_msg = samdev::message(L.err);
            bool good = ok == !L.err && (ok || msg == got_msg) && (!ok || L.size == want.size());
            if (ok && good) {
                for (int groups = 0; groups < 2 && good; groups++) for (uint32_t al = 0; al < 16 && good; al++) {
                    std::vector<uint8_t> buf(want.size() + 64, 0xA5);
                    uint8_t *o = buf.data() + ((16 - ((uintptr_t)buf.data() & 15)) & 15) + al;      // the record's first byte at every alignment
                    samdev::Line E;
                    samdev::parse_line<true>(d + x, d + le, cg, o, E);
                    const uint32_t nl = groups ? 16u : 1u;
                    if (E.lseq) for (uint32_t lane = 0; lane < nl; lane++) samdev::emit_seq(d + x + E.seq_off, E.qual_off == ~0u ? nullptr : d + x + E.qual_off, o + E.oseq, E.lseq, lane, nl, t16);
                    good = E.size == want.size() && E.err == 0 && E.host == L.host && o[want.size()] == 0xA5 && (o == buf.data() || o[-1] == 0xA5);
                    if (good && !E.host) good = memcmp(o, want.data(), want.size()) == 0;
                    if (good && E.host) {                                                          // every byte but the floating-point values, which the device leaves zero
                        std::vector<uint8_t> w0 = want;
                        good = zero_floats(w0, E.oseq + (E.lseq + 1) / 2 + E.lseq) && memcmp(o, w0.data(), w0.size()) == 0;
                    }
                }
            }
            if (!good) { fails++; printf("FAIL line %zu: host %s '%s' %zu, device '%s' %u\n", line, ok ? "ok" : "bad", msg.c_str(), want.size(), got_msg, L.size); }
            else printf("%zu %s %zu %u %s\n", line, ok ? "ok" : "bad", ok ? want.size() : (size_t)0, ok ? L.host : 0u, ok ? "" : got_msg);
        }
        x = le + 1;
    }
    return fails ? 1 : 0;
}
