// errprof::scan_record and errprof::count_record of gencore_amd/csrc/gce_errprof.hpp -- what each thread of the scan kernel and each 16-lane group of
// k_err_count runs -- compiled for the HOST (tests/test_errprof_model.py builds this with the host's address and undefined-behaviour
// sanitizers and compares what it prints and writes with tests/pyerrprof.py).  Every record, the reference bases and the interval table are
// handed over in heap blocks of exactly their size, so the sanitizer sees a read past them; the walk runs once with one lane and once with
// 16 lanes standing in for the group, one after another and in both orders, and the three sets of counters must be equal.  An add outside
// [0, 3072) x [0, 21) is a failure.  No kernel is launched.
// Usage: errprof_host_check N_REF MIN_MAPQ MIN_BASEQ EXCLUDE REF INTERVALS FRAMES OUT
//   REF: text, one line per contig of the header, its bases or "-" for a contig the FASTA lacks; INTERVALS: "-" for no BED, else text, one
//   "tid start end site0" per line, in rule S's order; FRAMES: records, each behind a 32-bit length; OUT: the counters, 3 x 1024 x 24 uint64.
//   One output line per record: "<index> <bad> <skip> <first>"; exit 1 on any failure.
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
#include "../gencore_amd/csrc/gce_calmd.hpp"
#include "../gencore_amd/csrc/gce_pileup.hpp"
#include "../gencore_amd/csrc/gce_errprof.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

struct HostAdd {
    std::vector<uint64_t> *c; int *fails;
    void operator()(uint32_t row, uint32_t cls) {
        if (row < 3u * EP_MAX_CYCLE && cls < EP_CLS) (*c)[(size_t)row * EP_ROW + cls]++;
        else { (*fails)++; printf("FAIL add at row %u class %u\n", row, cls); }
    }
};

int main(int argc, char **argv) {
    if (argc != 9) return 2;
    const bool bed = strcmp(argv[6], "-") != 0;
    errprof::Params P{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 0), bed ? 1u : 0u};
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
    std::vector<pileup::Ivl> iv; std::vector<uint32_t> tf((size_t)P.n_ref + 1, 0);
    if (bed) {
        std::istringstream in(slurp(argv[6]));
        long long t, a, z, s0;
        while (in >> t >> a >> z >> s0) {
            if (t < 0 || t >= P.n_ref) { printf("FAIL interval file\n"); return 1; }
            iv.push_back({(int32_t)t, (int32_t)a, (int32_t)z, (uint32_t)s0}); tf[(size_t)t + 1]++;
        }
    }
    for (int32_t t = 0; t < P.n_ref; t++) tf[(size_t)t + 1] += tf[(size_t)t];
    std::unique_ptr<pileup::Ivl[]> ivh(new pileup::Ivl[iv.size() ? iv.size() : 1]);
    for (size_t k = 0; k < iv.size(); k++) ivh[k] = iv[k];
    const pileup::Sites S{bed ? ivh.get() : nullptr, bed ? tf.data() : nullptr};
    const std::string framed = slurp(argv[7]);
    std::vector<std::vector<uint8_t>> frames;
    for (size_t x = 0; x + 4 <= framed.size();) {
        uint32_t fl; memcpy(&fl, framed.data() + x, 4); x += 4;
        if (x + fl > framed.size()) { printf("FAIL frame file\n"); return 1; }
        frames.emplace_back(framed.begin() + (ptrdiff_t)x, framed.begin() + (ptrdiff_t)(x + fl)); x += fl;
    }
    int fails = 0;
    std::vector<uint64_t> one(EP_COUNTERS, 0), fwd(EP_COUNTERS, 0), rev(EP_COUNTERS, 0);
    for (size_t i = 0; i < frames.size(); i++) {
        const std::vector<uint8_t> &f = frames[i];
        std::unique_ptr<uint8_t[]> heap(new uint8_t[f.size() ? f.size() : 1]);
        if (!f.empty()) memcpy(heap.get(), f.data(), f.size());
        errprof::Rec R;
        errprof::scan_record(heap.get(), f.size(), P, ref, S, R);
        printf("%zu %u %u %lld\n", i, R.bad, R.skip, R.first == EP_NONE ? -1ll : (long long)R.first);
        if ((R.bad || R.skip) && R.first != EP_NONE) { fails++; printf("FAIL record %zu: skipped, yet it has a first interval\n", i); }
        if (R.first == EP_NONE) continue;                                             // (as k_err_count drops it)
        HostAdd a1{&one, &fails}, af{&fwd, &fails}, ar{&rev, &fails};
        errprof::count_record(heap.get(), P, ref, S, R.first, 0u, 1u, a1);
        for (uint32_t l = 0; l < 16; l++) errprof::count_record(heap.get(), P, ref, S, R.first, l, 16u, af);
        for (uint32_t l = 16; l-- > 0;) errprof::count_record(heap.get(), P, ref, S, R.first, l, 16u, ar);
    }
    if (one != fwd || one != rev) { fails++; printf("FAIL one lane and 16 lanes disagree\n"); }
    { std::ofstream o(argv[8], std::ios::binary); o.write((const char *)one.data(), (std::streamsize)(one.size() * 8)); }
    return fails ? 1 : 0;
}
