// pileup::scan_record and pileup::count_record of gencore_amd/csrc/gce_pileup.hpp -- what each thread of the scan kernel and each 16-lane group of
// k_pile_count runs -- compiled for the HOST (tests/test_pileup_model.py builds this with the host's address and undefined-behaviour
// sanitizers and compares what it prints and writes with tests/pypileup.py).  Every record is handed over in a heap block of exactly its
// size, so the sanitizer sees a read past it; the walk runs once with one lane and once with 16 lanes standing in for the group, one after
// another and in both orders, and the three sets of counters must be equal.  An add outside [0, 16 * sites) is a failure.  No kernel is launched.
// Usage: pileup_host_check N_REF MIN_MAPQ MIN_BASEQ EXCLUDE INTERVALS FRAMES OUT
//   INTERVALS: text, one "tid start end site0" per line, in rule S's order; FRAMES: records, each behind a 32-bit length; OUT: the counters,
//   16 uint32 per site.  One output line per record: "<index> <bad> <skip> <first> <n_cigar_op>"; exit 1 on any failure.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#define GCE_PILEUP_HOST_CHECK
#include "../gencore_amd/csrc/gce_pileup.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

struct HostAdd {
    std::vector<uint32_t> *c; int *fails;
    void operator()(uint32_t idx) { if (idx < c->size()) (*c)[idx]++; else { (*fails)++; printf("FAIL add at counter %u of %zu\n", idx, c->size()); } }
};

int main(int argc, char **argv) {
    if (argc != 8) return 2;
    pileup::Params P{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 0)};
    std::vector<pileup::Ivl> iv; std::vector<uint32_t> tf((size_t)P.n_ref + 1, 0);
    uint64_t n_sites = 0;
    {
        std::istringstream in(slurp(argv[5]));
        long long t, a, z, s0;
        while (in >> t >> a >> z >> s0) {
            if (t < 0 || t >= P.n_ref || (uint64_t)s0 != n_sites) { printf("FAIL interval file\n"); return 1; }
            iv.push_back({(int32_t)t, (int32_t)a, (int32_t)z, (uint32_t)s0}); tf[(size_t)t + 1]++; n_sites += (uint64_t)(z - a);
        }
    }
    for (int32_t t = 0; t < P.n_ref; t++) tf[(size_t)t + 1] += tf[(size_t)t];
    // (the table in a heap block of exactly its size, too)
    std::unique_ptr<pileup::Ivl[]> ivh(new pileup::Ivl[iv.size() ? iv.size() : 1]);
    for (size_t k = 0; k < iv.size(); k++) ivh[k] = iv[k];
    const pileup::Sites S{ivh.get(), tf.data()};
    const std::string framed = slurp(argv[6]);
    std::vector<std::vector<uint8_t>> frames;
    for (size_t x = 0; x + 4 <= framed.size();) {
        uint32_t fl; memcpy(&fl, framed.data() + x, 4); x += 4;
        if (x + fl > framed.size()) { printf("FAIL frame file\n"); return 1; }
        frames.emplace_back(framed.begin() + (ptrdiff_t)x, framed.begin() + (ptrdiff_t)(x + fl)); x += fl;
    }
    int fails = 0;
    std::vector<uint32_t> one(n_sites * 16, 0), fwd(n_sites * 16, 0), rev(n_sites * 16, 0);
    for (size_t i = 0; i < frames.size(); i++) {
        const std::vector<uint8_t> &f = frames[i];
        std::unique_ptr<uint8_t[]> heap(new uint8_t[f.size() ? f.size() : 1]);
        if (!f.empty()) memcpy(heap.get(), f.data(), f.size());
        pileup::Rec R;
        pileup::scan_record(heap.get(), f.size(), P, S, R);
        printf("%zu %u %u %lld %u\n", i, R.bad, R.skip, R.first == PU_NONE ? -1ll : (long long)R.first, R.nc);
        if ((R.bad || R.skip) && R.first != PU_NONE) { fails++; printf("FAIL record %zu: skipped, yet it has a first interval\n", i); }
        if (R.first == PU_NONE) continue;                                             // (as k_pile_count drops it)
        HostAdd a1{&one, &fails}, af{&fwd, &fails}, ar{&rev, &fails};
        pileup::count_record(heap.get(), P, S, R.first, 0u, 1u, a1);
        for (uint32_t l = 0; l < 16; l++) pileup::count_record(heap.get(), P, S, R.first, l, 16u, af);
        for (uint32_t l = 16; l-- > 0;) pileup::count_record(heap.get(), P, S, R.first, l, 16u, ar);
    }
    if (one != fwd || one != rev) { fails++; printf("FAIL one lane and 16 lanes disagree\n"); }
    { std::ofstream o(argv[7], std::ios::binary); o.write((const char *)one.data(), (std::streamsize)(one.size() * 4)); }
    return fails ? 1 : 0;
}
