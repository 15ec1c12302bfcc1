// errsup::support, errsup::scan_record and errsup::count_record of gencore_amd/csrc/gce_errsup.hpp -- what one thread of the scan and each
// 16-lane group of k_sup_count run -- compiled for the HOST (tests/test_errsup_model.py builds this with the host's address and
// undefined-behaviour sanitizers and compares what it writes with tests/pyerrsup.py).  Every record, the reference bases, the interval table
// and the bitmap are handed over in heap blocks of exactly their size, so the sanitizer sees a read past them: the tag walk runs up to the
// last byte of a record's block.  The walk runs once with one lane and once with 16 lanes standing in for the group, in both orders, each
// lane repeating the tag walk as the kernel's lanes do, and the three sets of counters must be equal.  An add outside [0, 23) is a failure.
// No kernel is launched.
// Usage: errsup_host_check N_REF MIN_MAPQ MIN_BASEQ EXCLUDE TAGS REF INTERVALS MASK FRAMES OUT
//   TAGS: four characters; REF, INTERVALS, FRAMES as errprof_host_check takes them (INTERVALS "-": no BED); MASK: "-" for none, else text, one
//   "tid start end" per line, rule K's intervals; OUT: 3 x 33 x 33 x 24 uint64.
//   One output line: "# <records> <the nine skips> <eligible>"; exit 1 on any failure.
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
#define GCE_CALMD_HOST_CHECK
#define GCE_PILEUP_HOST_CHECK
#define GCE_ERRPROF_HOST_CHECK
#define GCE_ERRSUP_HOST_CHECK
#include "../gencore_amd/csrc/gce_calmd.hpp"
#include "../gencore_amd/csrc/gce_errsup.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

struct HostAdd {
    uint64_t *row; int *fails;
    void operator()(uint32_t cls) {
        if (cls <= ES_RECORDS) row[cls]++;
        else { (*fails)++; printf("FAIL add at class %u\n", cls); }
    }
};

int main(int argc, char **argv) {
    if (argc != 11 || strlen(argv[5]) != 4) return 2;
    const bool bed = strcmp(argv[7], "-") != 0, masked = strcmp(argv[8], "-") != 0;
    errprof::Params P{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 0), bed ? 1u : 0u};
    const uint8_t *tg = (const uint8_t *)argv[5];
    const errsup::Tags T{(uint16_t)(tg[0] | tg[1] << 8), (uint16_t)(tg[2] | tg[3] << 8)};
    // ---- the reference in calmd::Ref's layout
    std::vector<int64_t> tab((size_t)P.n_ref * 2 + 2, 0); std::string bases;
    {
        std::istringstream in(slurp(argv[6]));
        std::string line;
        for (int32_t t = 0; t < P.n_ref; t++) {
            if (!(in >> line)) { printf("FAIL reference file\n"); return 1; }
            tab[2 * (size_t)t] = (int64_t)bases.size(); tab[2 * (size_t)t + 1] = line == "-" ? -1 : (int64_t)line.size();
            if (line != "-") bases += line;
        }
    }
    std::unique_ptr<uint8_t[]> blob(new uint8_t[bases.size() ? bases.size() : 1]);
    if (!bases.empty()) memcpy(blob.get(), bases.data(), bases.size());
    const calmd::Ref ref{blob.get(), tab.data(), P.n_ref};
    // ---- rule B's table
    std::vector<reduce::Ivl> iv; std::vector<uint32_t> tf((size_t)P.n_ref + 1, 0);
    if (bed) {
        std::istringstream in(slurp(argv[7]));
        long long t, a, z, s0;
        while (in >> t >> a >> z >> s0) {
            if (t < 0 || t >= P.n_ref) { printf("FAIL interval file\n"); return 1; }
            iv.push_back({(int32_t)t, (int32_t)a, (int32_t)z, (uint32_t)s0}); tf[(size_t)t + 1]++;
        }
    }
    for (int32_t t = 0; t < P.n_ref; t++) tf[(size_t)t + 1] += tf[(size_t)t];
    std::unique_ptr<reduce::Ivl[]> ivh(new reduce::Ivl[iv.size() ? iv.size() : 1]);
    for (size_t k = 0; k < iv.size(); k++) ivh[k] = iv[k];
    const reduce::Sites S{bed ? ivh.get() : nullptr, bed ? tf.data() : nullptr};
    // ---- rule Y's bitmap, bit by bit, in a block of exactly the bytes that hold a bit per base
    const size_t mbytes = (bases.size() + 7) / 8;
    std::unique_ptr<uint8_t[]> bits(new uint8_t[mbytes ? mbytes : 1]);
    memset(bits.get(), 0, mbytes ? mbytes : 1);
    if (masked) {
        std::istringstream in(slurp(argv[8]));
        long long t, a, z;
        while (in >> t >> a >> z) {
            if (t < 0 || t >= P.n_ref || a < 0 || z > tab[2 * (size_t)t + 1] || a >= z) { printf("FAIL mask file\n"); return 1; }
            for (long long x = a; x < z; x++) { const uint64_t i = (uint64_t)(tab[2 * (size_t)t] + x); bits[i >> 3] |= (uint8_t)(1u << (i & 7u)); }
        }
    }
    const errprof::Mask M{bits.get()};
    const std::string framed = slurp(argv[9]);
    std::vector<std::unique_ptr<uint8_t[]>> heap; std::vector<size_t> size;
    for (size_t x = 0; x + 4 <= framed.size();) {
        uint32_t fl; memcpy(&fl, framed.data() + x, 4); x += 4;
        if (x + fl > framed.size()) { printf("FAIL frame file\n"); return 1; }
        heap.emplace_back(new uint8_t[fl ? fl : 1]); size.push_back(fl);
        if (fl) memcpy(heap.back().get(), framed.data() + x, fl);
        x += fl;
    }
    const size_t n = heap.size();
    int fails = 0;
    unsigned long long misc[errsup::ES_N_SKIP + 2] = {0};
    std::vector<uint64_t> one(ES_COUNTERS, 0), fwd(ES_COUNTERS, 0), rev(ES_COUNTERS, 0);
    for (size_t i = 0; i < n; i++) {
        const uint8_t *r = heap[i].get();
        errprof::Rec R;
        errsup::scan_record(r, size[i], P, T, ref, S, R);
        misc[0]++;
        if (R.bad) { printf("FAIL record %zu is malformed\n", i); fails++; continue; }
        if (R.skip) { if (R.skip > errsup::ES_N_SKIP || R.first != EP_NONE) { fails++; printf("FAIL skip %u\n", R.skip); } else misc[R.skip]++; continue; }
        misc[errsup::ES_N_SKIP + 1]++;
        if (R.first == EP_NONE) continue;
        for (int pass = 0; pass < 3; pass++) {
            std::vector<uint64_t> &c = pass == 0 ? one : pass == 1 ? fwd : rev;
            const uint32_t nl = pass == 0 ? 1u : 16u;
            for (uint32_t k = 0; k < nl; k++) {
                const uint32_t lane = pass == 2 ? nl - 1 - k : k;
                const errsup::Support s = errsup::support(r, T);                   // (every lane walks the tags itself)
                const uint32_t row = errsup::row_of(r, s);
                if (s.bad || s.f >= ES_BUCKETS || s.r >= ES_BUCKETS || row >= ES_ROWS) { fails++; printf("FAIL support of record %zu\n", i); break; }
                HostAdd add{c.data() + (size_t)row * EP_ROW, &fails};
                if (masked) errsup::count_record(r, P, ref, S, R.first, lane, nl, add, M);
                else errsup::count_record(r, P, ref, S, R.first, lane, nl, add);
            }
        }
    }
    if (one != fwd || one != rev) { fails++; printf("FAIL one lane and 16 lanes disagree\n"); }
    printf("#");
    for (int k = 0; k < errsup::ES_N_SKIP + 2; k++) printf(" %llu", misc[k]);
    printf("\n");
    {
        std::ofstream o(argv[10], std::ios::binary);
        o.write((const char *)one.data(), (std::streamsize)(one.size() * 8));
    }
    return fails ? 1 : 0;
}
