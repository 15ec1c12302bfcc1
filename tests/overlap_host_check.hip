// ovlmerge::Cursor, shared_runs, rule_q and merge_pair of gencore_amd/csrc/gce_ovlmerge.hpp -- what each 16-lane group of k_ovl_merge runs --
// with the join's fragpile::candidate, key, same_group and is_pair, compiled for the HOST (tests/test_overlap_model.py builds this with the
// host's address and undefined-behaviour sanitizers and compares what it prints and writes with tests/pyovlmerge.py).  Every record is handed
// over in a heap block of exactly its size, so the sanitizer sees a read or a write past it.  The join is done here as k_frag_join does it,
// over the whole file.  Every pair is merged three times on copies of its records: with one lane, with 16 lanes in ascending and in
// descending order standing in for the group; the three results must be equal, and outside the QUAL bytes every record must be what it was.
// The dual-cursor walk is also held against the walk it replaces: at every column of the pair's span, the walk names the column shared
// exactly when fragpile::column finds a base of both records there, with the same classes and qualities.  No kernel is launched.
// Usage: overlap_host_check MIN_MAPQ EXCLUDE WEAK FRAMES OUT
//   FRAMES: the records, each behind its length as 4 bytes; OUT: the records afterwards, framed alike.  One output line per record:
//   "<index> <eligible> <candidate> <partner>" (partner: the other record's index, -1 none, -2 ambiguous), then
//   "# <pairs> <pairs without qualities> <ambiguous> <shared columns> <disagreeing> <skipped> <records changed> <order offender>"; exit 1 on any failure.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#define GCE_PILEUP_HOST_CHECK
#define GCE_FRAGPILE_HOST_CHECK
#define GCE_OVLMERGE_HOST_CHECK
#include "../gencore_amd/csrc/gce_fragpile.hpp"
#include "../gencore_amd/csrc/gce_ovlmerge.hpp"

static std::string slurp(const char *p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

typedef std::unique_ptr<uint8_t[]> Block;
static Block copy_of(const uint8_t *r, size_t n) { Block b(new uint8_t[n ? n : 1]); if (n) memcpy(b.get(), r, n); return b; }

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int32_t min_mapq = atoi(argv[1]); const uint32_t exclude = (uint32_t)strtoul(argv[2], nullptr, 0);
    const bool weak = atoi(argv[3]) != 0;
    const std::string framed = slurp(argv[4]);
    std::vector<Block> heap; std::vector<size_t> size;
    for (size_t x = 0; x + 4 <= framed.size();) {
        uint32_t fl; memcpy(&fl, framed.data() + x, 4); x += 4;
        if (x + fl > framed.size()) { printf("FAIL frame file\n"); return 1; }
        heap.push_back(copy_of((const uint8_t *)framed.data() + x, fl)); size.push_back(fl);
        x += fl;
    }
    const size_t n = heap.size();
    int fails = 0;
    // ---- rule E, rule P, rule M as OvlRead, k_frag_prep and k_frag_join do them
    std::vector<char> elig(n, 0), cand(n, 0); std::vector<uint64_t> hk(n, 0); std::vector<long long> partner(n, -1);
    long long offender = -1; uint64_t prev = 0;
    for (size_t i = 0; i < n; i++) {
        const uint8_t *r = heap[i].get();
        reduce::Core C;
        const int e = reduce::rule_e(r, size[i], 0x7FFFFFFF, min_mapq, exclude, C);
        if (e == reduce::BAD) { printf("FAIL malformed record %zu\n", i); return 1; }
        const uint64_t k = fragpile::order_key(r);
        if (k < prev && offender < 0) offender = (long long)i;
        prev = k;
        elig[i] = e == reduce::ELIGIBLE;
        if (elig[i]) cand[i] = fragpile::candidate(r, C, 0u);
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
    for (size_t i = 0; i < n; i++) printf("%zu %d %d %lld\n", i, (int)elig[i], (int)cand[i], partner[i]);
    // ---- rule Q
    unsigned long long shared = 0, differ = 0, skipped = 0, changed = 0, no_qual = 0;
    std::vector<Block> out;
    for (size_t i = 0; i < n; i++) out.push_back(copy_of(heap[i].get(), size[i]));
    for (size_t ib = 0; offender < 0 && ib < n; ib++) {
        if (partner[ib] < 0 || (size_t)partner[ib] > ib) continue;
        const size_t ia = (size_t)partner[ib];
        const uint8_t *a0 = heap[ia].get(), *b0 = heap[ib].get();
        // the dual cursor against fragpile::column, column by column over the pair's span
        {
            std::map<int64_t, std::pair<uint32_t, uint32_t>> runs;
            const reduce::Head ha(a0), hb(b0);
            ovlmerge::shared_runs(ha, hb, [&](int64_t x, uint32_t len, uint32_t ya, uint32_t yb) {
                for (uint32_t j = 0; j < len; j++) {
                    if (runs.count(x + j)) { fails++; printf("FAIL column %lld twice\n", (long long)(x + j)); }
                    runs[x + j] = {ya + j, yb + j};
                }
            });
            reduce::Core Ca, Cb;
            (void)reduce::rule_e(a0, size[ia], 0x7FFFFFFF, min_mapq, exclude, Ca); (void)reduce::rule_e(b0, size[ib], 0x7FFFFFFF, min_mapq, exclude, Cb);
            const int64_t lo = Ca.pos, hi = (Ca.pos + Ca.rlen > Cb.pos + Cb.rlen ? Ca.pos + Ca.rlen : Cb.pos + Cb.rlen) + 1;
            for (int64_t x = lo - 1; x < hi; x++) {
                uint32_t ca = 0, qa = 0, cb = 0, qb = 0;
                const bool both = fragpile::column(a0, x, ca, qa) && fragpile::column(b0, x, cb, qb) && ca != fragpile::PU_DEL && cb != fragpile::PU_DEL;
                if (both != (runs.count(x) != 0)) { fails++; printf("FAIL pair %zu/%zu column %lld: shared %d by column, %d by the cursors\n", ia, ib, (long long)x, (int)both, (int)!both); continue; }
                if (!both) continue;
                const uint32_t ya = runs[x].first, yb = runs[x].second;
                if (reduce::read_class(ha.sq, ya) != ca || reduce::read_class(hb.sq, yb) != cb || (ha.has_q() && ha.ql[ya] != qa) || (hb.has_q() && hb.ql[yb] != qb)) {
                    fails++; printf("FAIL pair %zu/%zu column %lld: the cursors' query offsets\n", ia, ib, (long long)x);
                }
            }
        }
        Block a1 = copy_of(a0, size[ia]), b1 = copy_of(b0, size[ib]), af = copy_of(a0, size[ia]), bf = copy_of(b0, size[ib]), ar = copy_of(a0, size[ia]), br = copy_of(b0, size[ib]);
        ovlmerge::Tally t1 = {0, 0, 0, 0, 0}, tf = {0, 0, 0, 0, 0}, tr = {0, 0, 0, 0, 0};
        ovlmerge::merge_pair(a1.get(), b1.get(), 0u, 1u, t1);
        for (uint32_t l = 0; l < 16; l++) ovlmerge::merge_pair(af.get(), bf.get(), l, 16u, tf);
        for (uint32_t l = 16; l-- > 0;) ovlmerge::merge_pair(ar.get(), br.get(), l, 16u, tr);
        if (memcmp(a1.get(), af.get(), size[ia]) || memcmp(a1.get(), ar.get(), size[ia]) || memcmp(b1.get(), bf.get(), size[ib]) || memcmp(b1.get(), br.get(), size[ib]) ||
            t1.shared != tf.shared || t1.shared != tr.shared || t1.differ != tf.differ || t1.differ != tr.differ || t1.skipped != tf.skipped || t1.skipped != tr.skipped ||
            t1.changed != tf.changed || t1.changed != tr.changed || t1.no_qual != tf.no_qual || t1.no_qual != tr.no_qual) { fails++; printf("FAIL pair %zu/%zu: one lane and 16 lanes disagree\n", ia, ib); }
        // outside the QUAL bytes nothing may differ
        for (int w = 0; w < 2; w++) {
            const uint8_t *was = w ? b0 : a0, *is = w ? b1.get() : a1.get();
            const reduce::Head h(was);
            const size_t q0 = (size_t)(h.ql - was), q1 = q0 + (size_t)h.lseq;
            for (size_t k = 0; k < size[w ? ib : ia]; k++) if ((k < q0 || k >= q1) && was[k] != is[k]) { fails++; printf("FAIL pair %zu/%zu: byte %zu outside QUAL written\n", ia, ib, k); break; }
            if (((t1.changed >> w) & 1u) != (memcmp(was, is, size[w ? ib : ia]) != 0 ? 1u : 0u)) { fails++; printf("FAIL pair %zu/%zu: changed bit %d\n", ia, ib, w); }
        }
        shared += t1.shared; differ += t1.differ; skipped += t1.skipped; changed += (t1.changed & 1u) + (t1.changed >> 1); no_qual += t1.no_qual;
        out[ia] = std::move(a1); out[ib] = std::move(b1);
    }
    printf("# %llu %llu %llu %llu %llu %llu %llu %lld\n", pairs, no_qual, ambiguous, shared, differ, skipped, changed, offender);
    {
        std::ofstream o(argv[5], std::ios::binary);
        for (size_t i = 0; i < n; i++) { const uint32_t fl = (uint32_t)size[i]; o.write((const char *)&fl, 4); o.write((const char *)out[i].get(), (std::streamsize)fl); }
    }
    return fails ? 1 : 0;
}
