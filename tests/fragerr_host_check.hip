// errprof::Cursor and errprof::paired_walk of gencore_amd/csrc/gce_fragerr.hpp -- what each 16-lane group of k_fragerr_count runs for a mate -- with
// errprof::scan_record / count_record and fragpile::candidate, key, same_group and is_pair, compiled for the HOST (tests/test_fragerr_model.py
// builds this with the host's address and undefined-behaviour sanitizers and compares what it prints and writes with tests/pyfragerr.py).
// Every record, the reference bases and the interval table are handed over in heap blocks of exactly their size, so the sanitizer sees a
// read past them.  The join is done here as k_frag_join does it, over the whole file; the walks run once with one lane and once with 16
// lanes standing in for the group, in both orders, and the three sets of counters must be equal.  For every mate of a pair a cursor over its
// partner is asked for every column from two in front of the partner to two behind it, in ascending order, and its answers must be
// fragpile::column's (a D column of which is no aligned base).  An add outside [0, 3072) x [0, 21) is a failure.  No kernel is launched.
// Usage: fragerr_host_check N_REF MIN_MAPQ MIN_BASEQ EXCLUDE WEAK REF INTERVALS FRAMES OUT
//   REF, INTERVALS, FRAMES as errprof_host_check takes them; OUT: the primary table, then the overlap table, 3 x 1024 x 24 uint64 each.
//   One output line per record: "<index> <bad> <skip> <first> <candidate> <partner>" (partner: the other record's index, -1 none, -2
//   ambiguous), then "# <pairs> <shared columns> <disagreeing> <ambiguous> <order offender> <cursor columns checked> <most ops of a partner>";
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
        if (row < 3u * EP_MAX_CYCLE && cls < EP_CLS) (*c)[(size_t)row * EP_ROW + cls]++;
        else { (*fails)++; printf("FAIL add at row %u class %u\n", row, cls); }
    }
};

int main(int argc, char **argv) {
    if (argc != 10) return 2;
    const bool weak = atoi(argv[5]) != 0, bed = strcmp(argv[7], "-") != 0;
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
    int fails = 0;
    // ---- what the scan, k_frag_prep and k_frag_join learn
    std::vector<errprof::Rec> R(n); std::vector<char> cand(n, 0); std::vector<uint64_t> hk(n, 0); std::vector<long long> partner(n, -1);
    long long offender = -1; uint64_t prev = 0;
    for (size_t i = 0; i < n; i++) {
        const uint8_t *r = heap[i].get();
        errprof::scan_record(r, size[i], P, ref, S, R[i]);
        if (R[i].bad) continue;
        const uint64_t k = fragpile::order_key(r);
        if (k < prev && offender < 0) offender = (long long)i;
        prev = k;
        reduce::Core C;
        if (R[i].first != EP_NONE && reduce::rule_e(r, size[i], P.n_ref, P.min_mapq, P.exclude, C) == reduce::ELIGIBLE) cand[i] = fragpile::candidate(r, C, R[i].first);
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
        printf("%zu %u %u %lld %d %lld\n", i, R[i].bad, R[i].skip, R[i].first == EP_NONE ? -1ll : (long long)R[i].first, (int)cand[i], partner[i]);
    // ---- the walks
    std::vector<uint64_t> one[2], fwd[2], rev[2];
    for (int t = 0; t < 2; t++) { one[t].assign(EP_COUNTERS, 0); fwd[t].assign(EP_COUNTERS, 0); rev[t].assign(EP_COUNTERS, 0); }
    uint32_t sh[3] = {0, 0, 0}, df[3] = {0, 0, 0};
    unsigned long long checked = 0; uint32_t most_ops = 0;
    for (size_t i = 0; i < n; i++) {
        if (R[i].first == EP_NONE) continue;
        const uint8_t *r = heap[i].get();
        HostAdd a1{&one[0], &fails}, af{&fwd[0], &fails}, ar{&rev[0], &fails}, x1{&one[1], &fails}, xf{&fwd[1], &fails}, xr{&rev[1], &fails};
        if (partner[i] < 0) {
            errprof::count_record(r, P, ref, S, R[i].first, 0u, 1u, a1);
            for (uint32_t l = 0; l < 16; l++) errprof::count_record(r, P, ref, S, R[i].first, l, 16u, af);
            for (uint32_t l = 16; l-- > 0;) errprof::count_record(r, P, ref, S, R[i].first, l, 16u, ar);
            continue;
        }
        const uint8_t *o = heap[(size_t)partner[i]].get();
        const bool is_b = (size_t)partner[i] < i;
        errprof::paired_walk(r, o, is_b, P, ref, S, R[i].first, 0u, 1u, a1, x1, sh[0], df[0]);
        for (uint32_t l = 0; l < 16; l++) errprof::paired_walk(r, o, is_b, P, ref, S, R[i].first, l, 16u, af, xf, sh[1], df[1]);
        for (uint32_t l = 16; l-- > 0;) errprof::paired_walk(r, o, is_b, P, ref, S, R[i].first, l, 16u, ar, xr, sh[2], df[2]);
        // ---- the cursor over o against fragpile::column, with a stride of 1 and of 16
        reduce::Core C;
        if (reduce::rule_e(o, size[(size_t)partner[i]], P.n_ref, P.min_mapq, P.exclude, C) != reduce::ELIGIBLE) { fails++; printf("FAIL partner of %zu is not eligible\n", i); continue; }
        if (C.n_cigar_op > most_ops) most_ops = C.n_cigar_op;
        for (int64_t stride : {1, 16})
            for (int64_t lane = 0; lane < stride; lane++) {
                errprof::Cursor cur(o);
                for (int64_t x = (int64_t)C.pos - 2 + lane; x < (int64_t)C.pos + C.rlen + 2; x += stride) {
                    uint32_t c0 = 9, q0 = 999, c1 = 9, q1 = 999;
                    const bool got = cur.at(x, c0, q0);
                    const bool want = fragpile::column(o, x, c1, q1) && c1 != pileup::PU_DEL;
                    checked++;
                    if (got != want || (got && (c0 != c1 || q0 != q1))) { fails++; printf("FAIL cursor over record %lld at %lld: %d %u %u, column says %d %u %u\n", partner[i], (long long)x, (int)got, c0, q0, (int)want, c1, q1); }
                }
            }
    }
    for (int t = 0; t < 2; t++) if (one[t] != fwd[t] || one[t] != rev[t]) { fails++; printf("FAIL one lane and 16 lanes disagree in table %d\n", t); }
    if (sh[0] != sh[1] || sh[0] != sh[2] || df[0] != df[1] || df[0] != df[2]) { fails++; printf("FAIL one lane and 16 lanes disagree in rule V's counters\n"); }
    unsigned long long xs = 0; for (uint64_t v : one[1]) xs += v;
    if (xs != 2ull * sh[0]) { fails++; printf("FAIL the overlap table sums to %llu, twice the shared columns is %llu\n", xs, 2ull * sh[0]); }
    printf("# %llu %u %u %llu %lld %llu %u\n", pairs, sh[0], df[0], ambiguous, offender, checked, most_ops);
    {
        std::ofstream o(argv[9], std::ios::binary);
        for (int t = 0; t < 2; t++) o.write((const char *)one[t].data(), (std::streamsize)(one[t].size() * 8));
    }
    return fails ? 1 : 0;
}
