// calmd::md_record<false>, calmd::md_record<true> and calmd::copy_body of gencore_amd/csrc/gce_calmd.hpp -- what each thread of k_md_size /
// k_md_tags and each 16-lane group of k_md_body runs -- compiled for the HOST (tests/test_calmd_model.py builds this with the host's address
// and undefined-behaviour sanitizers and compares what it prints and writes with tests/pycalmd.py).  Every record is handed over in a heap
// block of exactly its size and every contig in a block of exactly its length, so the sanitizer sees a read past either; the new record is
// written at every offset 0..15 modulo 16 into a buffer of guard bytes, its 16 lanes one after another, in both orders.  No kernel is launched.
// Usage: calmd_host_check REF FRAMES OUT
//   REF: n_ref (int32), then per tid a 64-bit length (-1: the FASTA lacks the contig) and the bases; FRAMES: records, each behind a 32-bit
//   length; OUT: the new record of every input record behind a 32-bit length (0 for a malformed one).
//   One output line per record: "<index> <bad> <rewritten> <no_ref> <nm> <md_len> <size> <nm_changed> <md_changed>"; exit 1 on any failure.
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
#include "../gencore_amd/csrc/gce_calmd.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::string rf = slurp(argv[1]), framed = slurp(argv[2]);
    // ---- the reference: every contig in a block of its own; the table's offsets count from the lowest block
    int32_t n_ref = 0; memcpy(&n_ref, rf.data(), 4);
    std::vector<std::unique_ptr<uint8_t[]>> contig((size_t)n_ref); std::vector<int64_t> len((size_t)n_ref, -1), tab((size_t)n_ref * 2 + 2, 0);
    {
        size_t x = 4;
        for (int32_t t = 0; t < n_ref; t++) {
            memcpy(&len[(size_t)t], rf.data() + x, 8); x += 8;
            if (len[(size_t)t] < 0) continue;
            contig[(size_t)t].reset(new uint8_t[len[(size_t)t] ? (size_t)len[(size_t)t] : 1]);
            memcpy(contig[(size_t)t].get(), rf.data() + x, (size_t)len[(size_t)t]); x += (size_t)len[(size_t)t];
        }
    }
    const uint8_t *base = nullptr;
    for (int32_t t = 0; t < n_ref; t++) if (contig[(size_t)t] && (!base || contig[(size_t)t].get() < base)) base = contig[(size_t)t].get();
    for (int32_t t = 0; t < n_ref; t++) { tab[2 * (size_t)t] = contig[(size_t)t] ? (int64_t)(contig[(size_t)t].get() - base) : 0; tab[2 * (size_t)t + 1] = len[(size_t)t]; }
    const calmd::Ref ref = {base, tab.data(), n_ref};

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
        calmd::Rec L;
        calmd::md_record<false>(heap.get(), f.size(), ref, nullptr, L);
        printf("%zu %u %u %u %u %u %u %u %u\n", i, L.bad, L.elig, L.no_ref, L.nm, L.md_len, L.size, L.nm_changed, L.md_changed);
        std::vector<uint8_t> first;
        if (!L.bad) {
            // what the kernels keep of L between the passes
            calmd::Rec K; calmd::unpack(calmd::pack(L), L.size, K);
            for (int order = 0; order < 2; order++) for (uint32_t al = 0; al < 16; al++) {
                std::vector<uint8_t> buf((size_t)L.size + 96, 0xA5);
                uint8_t *o = buf.data() + ((16 - ((uintptr_t)buf.data() & 15)) & 15) + 16 + al;
                calmd::Rec E = K;
                if (E.elig) calmd::md_record<true>(heap.get(), f.size(), ref, o, E);
                for (uint32_t k = 0; k < 16; k++) calmd::copy_body(heap.get(), (uint32_t)f.size(), o, K, order ? 15 - k : k);
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
