// fragpile::candidate, key, same_group, is_pair, column and paired_walk of gencore_amd/csrc/gce_fragpile.hpp -- what each thread of k_frag_prep and
// k_frag_join and each 16-lane group of k_frag_count runs -- compiled for the HOST (tests/test_fragpile_model.py builds this with the host's
// address and undefined-behaviour sanitizers and compares what it prints and writes with tests/pyfragpile.py).  Every record is handed over
// in a heap block of exactly its size, so the sanitizer sees a read past it.  The join is done here as k_frag_join does it, over the whole
// file: a candidate looks at every other candidate of equal key; the walks run once with one lane and once with 16 lanes standing in for
// the group, in both orders, and the three sets of counters must be equal.  An add outside [0, 16 * sites) is a failure.  No kernel is launched.
// Usage: fragpile_host_check N_REF MIN_MAPQ MIN_BASEQ EXCLUDE WEAK INTERVALS FRAMES OUT
//   INTERVALS, FRAMES, OUT as pileup_host_check takes them.  One output line per record: "<index> <bad> <skip> <first> <candidate> <partner>"
//   (partner: the other record's index, -1 none, -2 ambiguous), then "# <pairs> <shared columns> <disagreeing> <ambiguous> <order offender>";
//   exit 1 on any failure.
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
#define GCE_FRAGPILE_HOST_CHECK
#include "../gencore_amd/csrc/gce_fragpile.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

struct HostAdd {
    std::vector<uint32_t> *c; int *fails;
    void operator()(uint32_t idx) { if (idx < c->size()) (*c)[idx]++; else { (*fails)++; printf("FAIL add at counter %u of %zu\n", idx, c->size()); } }
};

int main(int argc, char **argv) {
    if (argc != 9) return 2;
    pileup::Params P{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), (uint32_t)strtoul(argv[4], nullptr, 0)};
    const bool weak = atoi(argv[5]) != 0;
    std::vector<pileup::Ivl> iv; std::vector<uint32_t> tf((size_t)P.n_ref + 1, 0);
    uint64_t n_sites = 0;
    {
        std::istringstream in(slurp(argv[6]));
        long long t, a, z, s0;
        while (in >> t >> a >> z >> s0) {
            if (t < 0 || t >= P.n_ref || (uint64_t)s0 != n_sites) { printf("FAIL interval file\n"); return 1; }
            iv.push_back({(int32_t)t, (int32_t)a, (int32_t)z, (uint32_t)s0}); tf[(size_t)t + 1]++; n_sites += (uint64_t)(z - a);
        }
    }
    for (int32_t t = 0; t < P.n_ref; t++) tf[(size_t)t + 1] += tf[(size_t)t];
    std::unique_ptr<pileup::Ivl[]> ivh(new pileup::Ivl[iv.size() ? iv.size() : 1]);
    for (size_t k = 0; k < iv.size(); k++) ivh[k] = iv[k];
    const pileup::Sites S{ivh.get(), tf.data()};
    const std::string framed = slurp(argv[7]);
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
    // ---- what the scan, k_frag_prep and k_frag_join learn
    std::vector<pileup::Rec> R(n); std::vector<char> cand(n, 0); std::vector<uint64_t> hk(n, 0); std::vector<long long> partner(n, -1);
    long long offender = -1; uint64_t prev = 0;
    for (size_t i = 0; i < n; i++) {
        const uint8_t *r = heap[i].get();
        pileup::scan_record(r, size[i], P, S, R[i]);
        if (R[i].bad) continue;
        const uint64_t k = fragpile::order_key(r);
        if (k < prev && offender < 0) offender = (long long)i;
        prev = k;
        reduce::Core C;
        if (R[i].first != PU_NONE && reduce::rule_e(r, size[i], P.n_ref, P.min_mapq, P.exclude, C) == reduce::ELIGIBLE) cand[i] = fragpile::candidate(r, C, R[i].first);
        if (cand[i]) hk[i] = fragpile::key(r, weak);
    }
    unsigned long long pairs = 0, ambiguous = 0;
    for (size_t i = 0; i < n; i++) {
        if (!cand[i]) continue;
        uint32_t cnt = 0; size_t other = 0;
        for (size_t o = 0; o < n; o++) if (o != i && cand[o] && hk[o] == hk[i] && fragpile::same_group(heap[i].get(), heap[o].get())) { cnt++; other = o; }
        if (cnt >= 2) { partner[i] = -2; ambiguous++; }
        else if (cnt == 1 && fragpile::is_pair(heap[i].get(), heap[other].get())) { partner[i] = (long long)other; pairs += i > other; }
    }
    for (size_t i = 0; i < n; i++)
        printf("%zu %u %u %lld %d %lld\n", i, R[i].bad, R[i].skip, R[i].first == PU_NONE ? -1ll : (long long)R[i].first, (int)cand[i], partner[i]);
    // ---- the walks
    std::vector<uint32_t> one(n_sites * 16, 0), fwd(n_sites * 16, 0), rev(n_sites * 16, 0);
    uint32_t sh[3] = {0, 0, 0}, df[3] = {0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        if (R[i].first == PU_NONE) continue;
        const uint8_t *r = heap[i].get();
        HostAdd a1{&one, &fails}, af{&fwd, &fails}, ar{&rev, &fails};
        if (partner[i] < 0) {
            pileup::count_record(r, P, S, R[i].first, 0u, 1u, a1);
            for (uint32_t l = 0; l < 16; l++) pileup::count_record(r, P, S, R[i].first, l, 16u, af);
            for (uint32_t l = 16; l-- > 0;) pileup::count_record(r, P, S, R[i].first, l, 16u, ar);
        } else {
            const uint8_t *o = heap[(size_t)partner[i]].get();
            const bool is_b = (size_t)partner[i] < i;
            fragpile::paired_walk(r, o, is_b, P, S, R[i].first, 0u, 1u, a1, sh[0], df[0]);
            for (uint32_t l = 0; l < 16; l++) fragpile::paired_walk(r, o, is_b, P, S, R[i].first, l, 16u, af, sh[1], df[1]);
            for (uint32_t l = 16; l-- > 0;) fragpile::paired_walk(r, o, is_b, P, S, R[i].first, l, 16u, ar, sh[2], df[2]);
        }
    }
    if (one != fwd || one != rev || sh[0] != sh[1] || sh[0] != sh[2] || df[0] != df[1] || df[0] != df[2]) { fails++; printf("FAIL one lane and 16 lanes disagree\n"); }
    printf("# %llu %u %u %llu %lld\n", pairs, sh[0], df[0], ambiguous, offender);
    { std::ofstream o(argv[8], std::ios::binary); o.write((const char *)one.data(), (std::streamsize)(one.size() * 4)); }
    return fails ? 1 : 0;
}
