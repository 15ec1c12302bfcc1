// umi::umi_record<false>, umi::umi_record<true> and umi::copy_body of gencore_amd/csrc/gce_umi.hpp -- what each thread of k_umi_size /
// k_umi_tag and each 16-lane group of k_umi_body runs -- compiled for the HOST (tests/test_umi_model.py builds this with the host's address
// and undefined-behaviour sanitizers and compares what it prints and writes with tests/pyumi.py).  Every record is handed over in a heap
// block of exactly its size, so the sanitizer sees a read past it; the new record is written at every offset 0..15 modulo 16 into a buffer
// of guard bytes, its 16 lanes one after another, in both orders.  No kernel is launched.
// Usage: umi_host_check SOURCE FRAMES OUT
//   SOURCE: a two-character tag, or name; FRAMES: records, each behind a 32-bit length; OUT: the new record of every input record behind a
//   32-bit length (0 for a malformed one).
//   One output line per record: "<index> <bad> <tagged> <no_source> <not_umi> <mi_dropped> <many> <size>"; exit 1 on any failure.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#define GCE_CALMD_HOST_CHECK
#include "../gencore_amd/csrc/gce_umi.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::string source = argv[1], framed = slurp(argv[2]);
    if (source != "name" && source.size() != 2) return 2;
    const uint32_t src = source == "name" ? UM_SRC_NAME : (uint32_t)(uint8_t)source[0] | (uint32_t)(uint8_t)source[1] << 8;
    std::vector<std::vector<uint8_t>> frames;
    for (size_t x = 0; x + 4 <= framed.size();) {
        uint32_t fl; memcpy(&fl, framed.data() + x, 4); x += 4;
        if (x + fl > framed.size()) { printf("FAIL frame file\n"); return 1; }
        frames.emplace_back(framed.begin() + (ptrdiff_t)x, framed.begin() + (ptrdiff_t)(x + fl)); x += fl;
    }
    int fails = 0; std::string outb;
    for (size_t i = 0; i < frames.size(); i++) {
        const std::vector<uint8_t> &f = frames[i];
        std::unique_ptr<uint8_t[]> heap(new uint8_t[f.size() ? f.size() : 1]);
        if (!f.empty()) memcpy(heap.get(), f.data(), f.size());
        umi::Rec L;
        umi::umi_record<false>(heap.get(), f.size(), src, nullptr, L);
        printf("%zu %u %u %u %u %u %u %u\n", i, L.bad, L.tagged, L.no_source, L.not_umi, L.mi_dropped, L.many, L.size);
        std::vector<uint8_t> first;
        if (!L.bad) {
            // what the kernels keep of L between the passes
            umi::Rec K; umi::unpack(umi::pack(L), L.size, K);
            for (int order = 0; order < 2; order++) for (uint32_t al = 0; al < 16; al++) {
                std::vector<uint8_t> buf((size_t)L.size + 96, 0xA5);
                uint8_t *o = buf.data() + ((16 - ((uintptr_t)buf.data() & 15)) & 15) + 16 + al;
                umi::Rec E = K;
                if (E.tagged) umi::umi_record<true>(heap.get(), f.size(), src, o, E);
                for (uint32_t k = 0; k < 16; k++) umi::copy_body(heap.get(), (uint32_t)f.size(), o, K, order ? 15 - k : k);
                bool good = true;
                for (const uint8_t *q = buf.data(); q < o; q++) good = good && *q == 0xA5;
                for (const uint8_t *q = o + L.size; q < buf.data() + buf.size(); q++) good = good && *q == 0xA5;
                if (first.empty()) first.assign(o, o + L.size);
                else good = good && memcmp(first.data(), o, L.size) == 0;
                if (!good) { fails++; printf("FAIL record %zu at alignment %u, lane order %d\n", i, al, order); }
            }
        }
        const uint32_t n = (uint32_t)first.size();
        outb.append((const char *)&n, 4); outb.append((const char *)first.data(), first.size());
    }
    { std::ofstream o(argv[3], std::ios::binary); o.write(outb.data(), (std::streamsize)outb.size()); }
    return fails ? 1 : 0;
}
