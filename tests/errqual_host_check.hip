// errqual::bucket, the column functor and errqual::count_record of gencore_amd/csrc/gce_errqual.hpp, under errprof::scan_record -- what one
// thread of the scan and each 16-lane group of k_qual_count run -- compiled for the HOST (tests/test_errqual_model.py builds this with the
// host's address and undefined-behaviour sanitizers and compares what it writes with tests/pyerrqual.py).  Every record, the reference
// bases, the interval table and the bitmap are handed over in heap blocks of exactly their size, so the sanitizer sees a read past them: a
// quality index that is mirrored where it should not be, or taken from a cycle of another record, lands outside QUAL.  The walk runs once with
// one lane and once with 16 lanes standing in for the group, in both orders, and the three sets of counters must be equal.  An add outside
// [0, 288) x [0, 22) is a failure.  No kernel is launched.
// Usage: errqual_host_check N_REF MIN_MAPQ MIN_BASEQ EXCLUDE REF INTERVALS MASK FRAMES OUT
//   REF, INTERVALS, FRAMES as errprof_host_check takes them (INTERVALS "-": no BED); MASK: "-" for none, else text, one "tid start end" per
//   line, rule K's intervals; OUT: 3 x 96 x 24 uint64.
//   One output line: "# <records> <the eight skips> <eligible>"; exit 1 on any failure.
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
#define GCE_ERRQUAL_HOST_CHECK
#include "../gencore_amd/csrc/gce_calmd.hpp"
#include "../gencore_amd/csrc/gce_errqual.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

struct HostAdd {
    uint64_t *counts; int *fails; uint32_t top;
    void operator()(uint32_t row, uint32_t cls) {
        if (row < EQ_ROWS && cls <= top) counts[(size_t)row * EP_ROW + cls]++;
        else { (*fails)++; printf("FAIL add at row %u class %u\n", row, cls); }
    }
};

int main(int argc, char **argv) {
    if (argc != 10) return 2;
    const bool bed = strcmp(argv[6], "-") != 0, masked = strcmp(argv[7], "-") != 0;
    errprof::Params P{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 0), bed ? 1u : 0u};
    // ---- the bucket of every byte
    int fails = 0;
    for (uint32_t b = 0; b < 256; b++)
        if (errqual::bucket(b) != (b <= 93 ? b : 94u)) { fails++; printf("FAIL bucket of %u\n", b); }
    // ---- the reference in calmd::Ref's layout
    std::vector<int64_t> tab((size_t)P.n_ref * 2 + 2, 0); std::string bases;
    {
        std::istringstream in(slurp(argv[5]));
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
        std::istringstream in(slurp(argv[6]));
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
        std::istringstream in(slurp(argv[7]));
        long long t, a, z;
        while (in >> t >> a >> z) {
            if (t < 0 || t >= P.n_ref || a < 0 || z > tab[2 * (size_t)t + 1] || a >= z) { printf("FAIL mask file\n"); return 1; }
            for (long long x = a; x < z; x++) { const uint64_t i = (uint64_t)(tab[2 * (size_t)t] + x); bits[i >> 3] |= (uint8_t)(1u << (i & 7u)); }
        }
    }
    const errprof::Mask M{bits.get()};
    const std::string framed = slurp(argv[8]);
    std::vector<std::unique_ptr<uint8_t[]>> heap; std::vector<size_t> size;
    for (size_t x = 0; x + 4 <= framed.size();) {
        uint32_t fl; memcpy(&fl, framed.data() + x, 4); x += 4;
        if (x + fl > framed.size()) { printf("FAIL frame file\n"); return 1; }
        heap.emplace_back(new uint8_t[fl ? fl : 1]); size.push_back(fl);
        if (fl) memcpy(heap.back().get(), framed.data() + x, fl);
        x += fl;
    }
    const size_t n = heap.size();
    unsigned long long misc[errprof::EP_N_SKIP + 2] = {0};
    std::vector<uint64_t> one(EQ_COUNTERS, 0), fwd(EQ_COUNTERS, 0), rev(EQ_COUNTERS, 0);
    for (size_t i = 0; i < n; i++) {
        const uint8_t *r = heap[i].get();
        errprof::Rec R;
        errprof::scan_record(r, size[i], P, ref, S, R);
        misc[0]++;
        if (R.bad) { printf("FAIL record %zu is malformed\n", i); fails++; continue; }
        if (R.skip) { if (R.skip > errprof::EP_N_SKIP || R.first != EP_NONE) { fails++; printf("FAIL skip %u\n", R.skip); } else misc[R.skip]++; continue; }
        misc[errprof::EP_N_SKIP + 1]++;
        if (R.first == EP_NONE) continue;
        for (int pass = 0; pass < 3; pass++) {
            std::vector<uint64_t> &c = pass == 0 ? one : pass == 1 ? fwd : rev;
            const uint32_t nl = pass == 0 ? 1u : 16u;
            for (uint32_t k = 0; k < nl; k++) {
                const uint32_t lane = pass == 2 ? nl - 1 - k : k;
                HostAdd add{c.data(), &fails, masked ? EP_MASKED : (uint32_t)errprof::EP_DEL};
                if (masked) errqual::count_record(r, P, ref, S, R.first, lane, nl, add, M);
                else errqual::count_record(r, P, ref, S, R.first, lane, nl, add);
            }
        }
    }
    if (one != fwd || one != rev) { fails++; printf("FAIL one lane and 16 lanes disagree\n"); }
    printf("#");
    for (int k = 0; k < errprof::EP_N_SKIP + 2; k++) printf(" %llu", misc[k]);
    printf("\n");
    {
        std::ofstream o(argv[9], std::ios::binary);
        o.write((const char *)one.data(), (std::streamsize)(one.size() * 8));
    }
    return fails ? 1 : 0;
}
