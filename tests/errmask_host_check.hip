// errprof::count_record and errprof::paired_walk of gencore_amd/csrc/gce_errprof.hpp / gce_fragerr.hpp under a variant mask (rule Y of DESIGN.md
// 4m) -- what each 16-lane group of k_err_count<., errprof::Mask> and k_fragerr_count<., errprof::Mask> runs -- compiled for the HOST
// (tests/test_errmask_model.py builds this with the host's address and undefined-behaviour sanitizers and compares what it writes with
// tests/pyerrmask.py).  Every record, the reference bases, the interval table and the bitmap are handed over in heap blocks of exactly their
// size -- the bitmap has (reference bytes + 7) / 8 bytes, the fewest that hold a bit per base --, so the sanitizer sees a read past them.
// PAIRS 0: every record is walked alone, as gce_bam_error_profile_masked walks it; 1: the join is done here as fragerr_host_check does it
// and the mates of a pair are walked with paired_walk.  The walks run once with one lane and once with 16 lanes standing in for the group,
// in both orders, and the three sets of counters must be equal.  An add outside [0, 3072) x [0, 22) is a failure.  No kernel is launched.
// Usage: errmask_host_check N_REF MIN_MAPQ MIN_BASEQ EXCLUDE PAIRS REF INTERVALS MASK FRAMES OUT
//   REF, INTERVALS, FRAMES as errprof_host_check takes them; MASK: text, one "tid start end" per line, rule K's intervals (inside the
//   contigs' FASTA lengths); OUT: the primary table, then the overlap table, 3 x 1024 x 24 uint64 each.
//   One output line: "# <pairs> <shared columns> <disagreeing>"; exit 1 on any failure.
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
#define GCE_FRAGPILE_HOST_CHECK
#define GCE_ERRPROF_HOST_CHECK
#define GCE_FRAGERR_HOST_CHECK
#include "../gencore_amd/csrc/gce_calmd.hpp"
#include "../gencore_amd/csrc/gce_pileup.hpp"
#include "../gencore_amd/csrc/gce_fragpile.hpp"
#include "../gencore_amd/csrc/gce_errprof.hpp"
#include "../gencore_amd/csrc/gce_fragerr.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

struct HostAdd {
    std::vector<uint64_t> *c; int *fails;
    void operator()(uint32_t row, uint32_t cls) {
        if (row < 3u * EP_MAX_CYCLE && cls <= EP_MASKED) (*c)[(size_t)row * EP_ROW + cls]++;
        else { (*fails)++; printf("FAIL add at row %u class %u\n", row, cls); }
    }
};

int main(int argc, char **argv) {
    if (argc != 11) return 2;
    const bool pairs_on = atoi(argv[5]) != 0, bed = strcmp(argv[7], "-") != 0;
    errprof::Params P{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 0), bed ? 1u : 0u};
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
    std::vector<pileup::Ivl> iv; std::vector<uint32_t> tf((size_t)P.n_ref + 1, 0);
    if (bed) {
        std::istringstream in(slurp(argv[7]));
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
    // ---- rule Y's bitmap, bit by bit, in a block of exactly the bytes that hold a bit per base
    const size_t mbytes = (bases.size() + 7) / 8;
    std::unique_ptr<uint8_t[]> bits(new uint8_t[mbytes ? mbytes : 1]);
    memset(bits.get(), 0, mbytes ? mbytes : 1);
    {
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
    // ---- the scan and, with PAIRS, the join over the whole file
    std::vector<errprof::Rec> R(n); std::vector<char> cand(n, 0); std::vector<uint64_t> hk(n, 0); std::vector<long long> partner(n, -1);
    for (size_t i = 0; i < n; i++) {
        const uint8_t *r = heap[i].get();
        errprof::scan_record(r, size[i], P, ref, S, R[i]);
        if (R[i].bad || !pairs_on) continue;
        reduce::Core C;
        if (R[i].first != EP_NONE && reduce::rule_e(r, size[i], P.n_ref, P.min_mapq, P.exclude, C) == reduce::ELIGIBLE) cand[i] = fragpile::candidate(r, C, R[i].first);
        if (cand[i]) hk[i] = fragpile::key(r, false);
    }
    unsigned long long pairs = 0;
    for (size_t i = 0; i < n; i++) {
        if (!cand[i]) continue;
        uint32_t cnt = 0; size_t other = 0;
        for (size_t o = 0; o < n; o++) if (o != i && cand[o] && hk[o] == hk[i] && fragpile::same_group(heap[i].get(), heap[o].get())) { cnt++; other = o; }
        if (cnt >= 2) partner[i] = -2;
        else if (cnt == 1 && fragpile::is_pair(heap[i].get(), heap[other].get())) { partner[i] = (long long)other; pairs += i > other; }
    }
    // ---- the walks
    std::vector<uint64_t> one[2], fwd[2], rev[2];
    for (int t = 0; t < 2; t++) { one[t].assign(EP_COUNTERS, 0); fwd[t].assign(EP_COUNTERS, 0); rev[t].assign(EP_COUNTERS, 0); }
    uint32_t sh[3] = {0, 0, 0}, df[3] = {0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        if (R[i].first == EP_NONE) continue;
        const uint8_t *r = heap[i].get();
        HostAdd a1{&one[0], &fails}, af{&fwd[0], &fails}, ar{&rev[0], &fails}, x1{&one[1], &fails}, xf{&fwd[1], &fails}, xr{&rev[1], &fails};
        if (partner[i] < 0) {
            errprof::count_record(r, P, ref, S, R[i].first, 0u, 1u, a1, M);
            for (uint32_t l = 0; l < 16; l++) errprof::count_record(r, P, ref, S, R[i].first, l, 16u, af, M);
            for (uint32_t l = 16; l-- > 0;) errprof::count_record(r, P, ref, S, R[i].first, l, 16u, ar, M);
            continue;
        }
        const uint8_t *o = heap[(size_t)partner[i]].get();
        const bool is_b = (size_t)partner[i] < i;
        errprof::paired_walk(r, o, is_b, P, ref, S, R[i].first, 0u, 1u, a1, x1, sh[0], df[0], M);
        for (uint32_t l = 0; l < 16; l++) errprof::paired_walk(r, o, is_b, P, ref, S, R[i].first, l, 16u, af, xf, sh[1], df[1], M);
        for (uint32_t l = 16; l-- > 0;) errprof::paired_walk(r, o, is_b, P, ref, S, R[i].first, l, 16u, ar, xr, sh[2], df[2], M);
    }
    for (int t = 0; t < 2; t++) if (one[t] != fwd[t] || one[t] != rev[t]) { fails++; printf("FAIL one lane and 16 lanes disagree in table %d\n", t); }
    if (sh[0] != sh[1] || sh[0] != sh[2] || df[0] != df[1] || df[0] != df[2]) { fails++; printf("FAIL one lane and 16 lanes disagree in rule V's counters\n"); }
    unsigned long long xs = 0; for (uint64_t v : one[1]) xs += v;
    if (xs != 2ull * sh[0]) { fails++; printf("FAIL the overlap table sums to %llu, twice the shared columns is %llu\n", xs, 2ull * sh[0]); }
    printf("# %llu %u %u\n", pairs, sh[0], df[0]);
    {
        std::ofstream o(argv[10], std::ios::binary);
        for (int t = 0; t < 2; t++) o.write((const char *)one[t].data(), (std::streamsize)(one[t].size() * 8));
    }
    return fails ? 1 : 0;
}
