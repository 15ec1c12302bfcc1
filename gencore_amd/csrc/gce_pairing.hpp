// gce_pairing.hpp — mate pairing + UMI grouping per cluster, the tiers that give a cluster a whole wave: qname order and mate pairing
// (cluster.cpp:260-273, pair.cpp:188-216), greedy UMI grouping (cluster.cpp:55-100).
//
//   pairing_generic<PHASE> / k_pairing_slow<PHASE>   any cluster size, any name or UMI length: three launches over cluster-local scratch
//                    in device memory (w.k64), one wave per cluster (phase 1: several)
//   pairing_fast_cluster / k_pairing_fast   one wave per cluster of <= 64 reads, names <= 64 bytes, UMIs <= 24 bytes, everything in
//                    registers: names as big-endian words, hash-filtered name classes verified exactly, lexicographic rank, read -> pair
//                    transposition, UMI grouping.  The 16- and 32-lane tiers of gce_pair2.hpp are this algorithm, several clusters to a wave.
// Stage pair_clusters of engine.hip launches them: k_pairing_fast over every cluster or over pf_list (what the 32-lane tier flagged),
// k_pairing_slow over left_list (what k_pairing_deep, gce_deep.hpp, left over).  d_qname, load_be_words and the unaligned word types
// serve gce_pair2.hpp and gce_deep.hpp as well.
//
// A part of gce_kernels.hpp, which includes it behind Work and the wave helpers.
#pragma once

__device__ __forceinline__ const char *d_qname(const DevBatch &b, uint32_t r) { return b.qname + b.qname_off[r]; }

typedef uint64_t u64_unaligned __attribute__((aligned(1)));
typedef uint32_t u32_unaligned __attribute__((aligned(1)));
__device__ __forceinline__ uint64_t d_bswap64(uint64_t x) { return __builtin_bswap64(x); }
// up to 8*NW bytes of a string as big-endian words, zero padded: integer order == strcmp order
template <int NW>
__device__ __forceinline__ void load_be_words(const char *s, int len, uint64_t (&wd)[NW]) {
#pragma unroll
    for (int k = 0; k < NW; k++) {
        uint64_t v = 0;
        int rem = len - 8 * k;
        if (rem > 0) {
            v = *(const u64_unaligned *)(s + 8 * k);
            if (rem < 8) v &= (1ull << (8 * rem)) - 1ull;
            v = d_bswap64(v);
        }
        wd[k] = v;
    }
}
// generic path: any cluster size / name length, cluster-local global scratch
// Three launches (PHASE 0: name windows, 1: ranks, 2: pairs + UMI grouping + layout): the rank scan is O(n^2 / 64) per cluster and
// a cluster of thousands of reads would otherwise keep one wave busy for milliseconds; phase 1 spreads a cluster's 64-read blocks
// over `ibstep` waves.
template <int PHASE>
__device__ void pairing_generic(const DevBatch &b, const DevParams &p, const Work &w, uint32_t c, int lane, uint32_t ib0 = 0, uint32_t ibstep = 1) {
    const uint32_t start = w.cl_start[c], n = w.cl_n[c];
    uint32_t mode = d_thr_mode(w.cl_ikey[c], w.si, p);
    if (mode >= THR_NEVER) {                      // pending after an early finishConsensus: never processed (gencore.cpp:23); THR_RAW: k_raw_emit's
        if (PHASE == 2 && lane == 0) { w.cl_npairs[c] = 0; w.cl_ngroups[c] = 0; w.cl_hasumi[c] = 0; w.cl_tier[c] = TIER_NEVER; }
        return;
    }
    const int thr = mode == THR_PROPER ? p.proper_thr : p.unproper_thr;
    // ---- (a) order the cluster's reads by (qname, input index): map<string,Pair*> order + arrival order (cluster.cpp:260-273)
    //      Rank = number of reads that sort before mine.  The names of a cluster share a long prefix (instrument, run, flowcell);
    //      16 bytes after the cluster's common prefix, as two big-endian words per read in scratch, decide almost every
    //      comparison in registers; equal windows (mates, near-identical names) fall back to strcmp.
    uint64_t *kw = w.k64 + (size_t)start * 3;
    if (PHASE == 0) {
        const char *n0 = d_qname(b, w.members[start]);
        int cp = 0x7FFFFFFF;
        for (uint32_t i = lane; i < n; i += 64) {
            const char *mq = d_qname(b, w.members[start + i]);
            int l = 0;
            while (n0[l] && n0[l] == mq[l]) l++;
            cp = min(cp, l);
        }
        cp = wave_min(cp);
        for (uint32_t i = lane; i < n; i += 64) {
            const uint32_t my = w.members[start + i];
            const int nl = (int)b.core[my].l_qname - 1;
            uint64_t k2[2];
            load_be_words<2>(d_qname(b, my) + cp, max(nl - cp, 0), k2);
            kw[2 * i] = k2[0]; kw[2 * i + 1] = k2[1];
        }
        return;
    }
    if (PHASE == 1) {
    for (uint32_t base = 64 * ib0; base < n; base += 64 * ibstep) {
        const uint32_t i = base + lane;
        const bool mine = i < n;
        const uint32_t my = mine ? w.members[start + i] : NONE32;
        const char *mq = mine ? d_qname(b, my) : nullptr;
        const uint64_t m0 = mine ? kw[2 * i] : 0ull, m1 = mine ? kw[2 * i + 1] : 0ull;
        uint32_t rk = 0, ntie = 0, t1 = 0, t2 = 0;                           // equal windows (the mate, as a rule) are settled after the scan,
        for (uint32_t jb = 0; jb < n; jb += 64) {                             // every lane on its own: 64 windows per memory round trip, then
            const uint32_t jj = jb + lane;                                    // register broadcasts
            const uint64_t c0 = jj < n ? kw[2 * jj] : 0ull, c1 = jj < n ? kw[2 * jj + 1] : 0ull;
            const int lim = (int)min(64u, n - jb);
            for (int t = 0; t < lim; t++) {
                const uint64_t o0 = rl64(c0, t), o1 = rl64(c1, t);
                const uint32_t j = jb + t;
                rk += (o0 < m0 || (o0 == m0 && o1 < m1));
                if (o0 == m0 && o1 == m1 && j != i) { if (ntie == 0) t1 = j; else if (ntie == 1) t2 = j; ntie++; }
            }
        }
        if (mine) {
            auto before = [&](uint32_t j) { const uint32_t o = w.members[start + j]; const int cmp = d_strcmp(d_qname(b, o), mq); return cmp < 0 || (cmp == 0 && o < my); };
            if (ntie <= 2) { if (ntie >= 1) rk += before(t1); if (ntie == 2) rk += before(t2); }
            else for (uint32_t j = 0; j < n; j++) if (j != i && kw[2 * j] == m0 && kw[2 * j + 1] == m1) rk += before(j);
            w.sorted[start + rk] = my;
        }
    }
    return;
    }
    // ---- (b) pairs: first read of a qname run = mLeft, last of the run (if any other) = mRight (pair.cpp:188-216)
    uint32_t npairs = 0;
    int any_umi = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        uint32_t i = base + lane;
        bool valid = i < n, first = false, last = false;
        uint32_t q = NONE32;
        if (valid) {
            q = w.sorted[start + i];
            const char *mq = d_qname(b, q);
            first = (i == 0) || d_strcmp(d_qname(b, w.sorted[start + i - 1]), mq) != 0;
            last = (i == n - 1) || d_strcmp(d_qname(b, w.sorted[start + i + 1]), mq) != 0;
            if (!first) {       // setRight: `if(!mUMI.empty() && umi!=mUMI) error_exit` (pair.cpp:201-212)
                uint32_t pv = w.sorted[start + i - 1];
                if (d_umi_len(w, pv) != 0 && !d_bytes_equal(d_umi_ptr(b, w, pv), d_umi_len(w, pv), d_umi_ptr(b, w, q), d_umi_len(w, q))) raise_error(w.si, GCE_ERR_UMI_MISMATCH, q);
            }
        }
        unsigned long long fm = __ballot(first);
        uint32_t pidx = npairs + __popcll(fm & ((2ull << lane) - 1ull)) - 1;      // firsts up to and including this lane
        if (valid) {
            if (first) { w.pl[start + pidx] = q; if (last) w.pr[start + pidx] = NONE32; }
            if (last && !first) w.pr[start + pidx] = q;
            if (last) { w.pu[start + pidx] = q; if (d_umi_len(w, q)) any_umi = 1; }
        }
        npairs += __popcll(fm);
    }
    any_umi = __any(any_umi);
    WAVE_SYNC();
    // ---- (c) greedy UMI grouping (cluster.cpp:57-100)
    uint32_t ngroups = 0;
    if (!any_umi) {
        for (uint32_t i = lane; i < npairs; i += 64) w.pg[start + i] = 0;
        ngroups = 1;
    } else {
        uint32_t *pc = w.sorted;                 // reuse: per-pair count of identical UMIs (umiCount)
        // UMIs of <= 24 bytes as three zero-padded words per pair in scratch: equal words <=> equal strings
        bool longu = false;
        for (uint32_t i = lane; i < npairs; i += 64) {
            const uint32_t ui = w.pu[start + i]; const int ul = d_umi_len(w, ui);
            uint64_t u3[3];
            load_be_words<3>(d_umi_ptr(b, w, ui), min(ul, 24), u3);
            kw[3 * i] = u3[0]; kw[3 * i + 1] = u3[1]; kw[3 * i + 2] = u3[2];
            if (ul > 24) longu = true;
        }
        longu = __any(longu);
        WAVE_SYNC();
        for (uint32_t i = lane; i < npairs; i += 64) {
            uint32_t ui = w.pu[start + i];
            const char *up = d_umi_ptr(b, w, ui); int ul = d_umi_len(w, ui);
            uint32_t cnt = 0;
            if (!longu) {
                const uint64_t a0 = kw[3 * i], a1 = kw[3 * i + 1], a2 = kw[3 * i + 2];
                for (uint32_t j = 0; j + 3 < npairs; j += 4) {                    // four independent loads in flight per step
                    const uint64_t x0 = kw[3 * j], x1 = kw[3 * j + 1], x2 = kw[3 * j + 2], y0 = kw[3 * j + 3], y1 = kw[3 * j + 4], y2 = kw[3 * j + 5];
                    const uint64_t z0 = kw[3 * j + 6], z1 = kw[3 * j + 7], z2 = kw[3 * j + 8], v0 = kw[3 * j + 9], v1 = kw[3 * j + 10], v2 = kw[3 * j + 11];
                    cnt += (x0 == a0 && x1 == a1 && x2 == a2) + (y0 == a0 && y1 == a1 && y2 == a2) + (z0 == a0 && z1 == a1 && z2 == a2) + (v0 == a0 && v1 == a1 && v2 == a2);
                }
                for (uint32_t j = npairs & ~3u; j < npairs; j++) cnt += (kw[3 * j] == a0 && kw[3 * j + 1] == a1 && kw[3 * j + 2] == a2);
            } else
            for (uint32_t j = 0; j < npairs; j++) { uint32_t uj = w.pu[start + j]; cnt += d_bytes_equal(up, ul, d_umi_ptr(b, w, uj), d_umi_len(w, uj)); }
            pc[start + i] = cnt;
            w.pg[start + i] = NONE32;
        }
        WAVE_SYNC();
        uint32_t remaining = npairs;
        while (remaining > 0) {
            // top UMI: highest count, lexicographically first on ties (map order + strict `>`, cluster.cpp:68-76)
            uint32_t best = NONE32, bcnt = 0; const char *bu = nullptr; int bl = 0;
            for (uint32_t i = lane; i < npairs; i += 64) {
                if (w.pg[start + i] != NONE32) continue;
                uint32_t ui = w.pu[start + i], cnt = pc[start + i];
                const char *up = d_umi_ptr(b, w, ui); int ul = d_umi_len(w, ui);
                bool better = best == NONE32 || cnt > bcnt || (cnt == bcnt && d_slice_cmp(up, ul, bu, bl) < 0);
                if (better) { best = i; bcnt = cnt; bu = up; bl = ul; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                uint32_t ob = __shfl_xor(best, o), oc = __shfl_xor(bcnt, o);
                if (ob == NONE32) continue;
                uint32_t oui = w.pu[start + ob];
                const char *ou = d_umi_ptr(b, w, oui); int ol = d_umi_len(w, oui);
                bool better;
                if (best == NONE32) better = true;
                else if (oc != bcnt) better = oc > bcnt;
                else { int sc = d_slice_cmp(ou, ol, bu, bl); better = sc < 0 || (sc == 0 && ob < best); }
                if (better) { best = ob; bcnt = oc; bu = ou; bl = ol; }
            }
            uint32_t absorbed = 0;
            for (uint32_t base = 0; base < npairs; base += 64) {
                uint32_t i = base + lane;
                bool take = false;
                if (i < npairs && w.pg[start + i] == NONE32) {
                    uint32_t ui = w.pu[start + i];
                    take = d_umi_diff(d_umi_ptr(b, w, ui), d_umi_len(w, ui), bu, bl) <= thr;
                    if (take) w.pg[start + i] = ngroups;
                }
                absorbed += __popcll(__ballot(take));
            }
            remaining -= absorbed;
            ngroups++;
            WAVE_SYNC();
        }
    }
    WAVE_SYNC();
    // ---- (d) lay the pairs out group by group, qname order kept inside a group (Group::addPair, group.cpp:17-22)
    uint32_t gbase = 0;
    for (uint32_t g = 0; g < ngroups; g++) {
        uint32_t run = 0;
        for (uint32_t base = 0; base < npairs; base += 64) {
            uint32_t i = base + lane;
            bool in = i < npairs && w.pg[start + i] == g;
            unsigned long long m = __ballot(in);
            if (in) { uint32_t d = start + gbase + run + lanes_below(m); w.gpl[d] = w.pl[start + i]; w.gpr[d] = w.pr[start + i]; }
            run += __popcll(m);
        }
        if (lane == 0) { w.grp_begin[start + g] = start + gbase; w.grp_n[start + g] = run; }
        gbase += run;
    }
    if (lane == 0) { const bool cross = d_key(b.core[w.members[start]], p).right < 0; w.cl_npairs[c] = npairs; w.cl_ngroups[c] = ngroups; w.cl_hasumi[c] = (uint8_t)((any_umi ? 1 : 0) | (cross ? 2 : 0)); w.cl_tier[c] = TIER_GENERIC; }
}


template <int PHASE>
__global__ __launch_bounds__(256) void k_pairing_slow(DevBatch b, DevParams p, Work w) {
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t n_slow = w.si->n_slow_pair2;                                      // what k_pairing_deep (gce_deep.hpp) left over
    for (uint32_t idx = blockIdx.x * WAVES_PER_BLOCK + wv; idx < n_slow; idx += gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t c = w.left_list[idx];
        if (c != NONE32) pairing_generic<PHASE>(b, p, w, c, lane, blockIdx.y, gridDim.y);      // (NONE32: taken by the device-memory instantiation of k_pairing_deep)
        WAVE_SYNC();
    }
}

__device__ __forceinline__ int popc_nonzero_bytes(uint64_t x) {
    x |= x >> 4; x |= x >> 2; x |= x >> 1;
    return __popcll(x & 0x0101010101010101ull);
}

// One wave per cluster, <= 64 reads, names <= 64 bytes, UMIs <= 24 bytes: everything in registers.
__device__ void pairing_fast_cluster(const DevBatch &b, const DevParams &p, const Work &w, uint32_t c, int lane) {
    const uint32_t start = w.cl_start[c], n = w.cl_n[c];
    uint32_t mode = d_thr_mode(w.cl_ikey[c], w.si, p);
    if (mode >= THR_NEVER) { if (lane == 0) { w.cl_npairs[c] = 0; w.cl_ngroups[c] = 0; w.cl_hasumi[c] = 0; w.cl_tier[c] = TIER_NEVER; } return; }
    const int thr = mode == THR_PROPER ? p.proper_thr : p.unproper_thr;
    bool defer = n > 64;
    uint32_t my = NONE32; int nl = 0; const char *nm = nullptr; int ul = 0; uint64_t ui_ = 0;
    if (!defer && lane < (int)n) {
        my = w.members[start + lane];
        ui_ = w.uinfo[my];
        nl = (int)((ui_ >> 41) & 0xFFu) - 1;
        nm = d_qname(b, my);
        ul = uinfo_len(ui_);
    }
    if (!defer && __any(nl > 64 || ul > 24)) defer = true;
    if (defer) { if (lane == 0) w.slow_list[atomicAdd(&w.si->n_slow_pair, 1u)] = c; return; }
    const bool act = lane < (int)n;
    uint64_t nw[8];
    load_be_words<8>(nm, act ? nl : 0, nw);
    const int nwords = (wave_max(nl) + 7) >> 3;
    // ---- same-name detection through a 32-bit add-rotate-xor hash of the name words.  It is only a filter: every match is verified
    //      word by word below, and a false match sends the cluster to the generic kernel.  EQ = the other reads of my name (one
    //      ballot per read gives a whole name class at once), LOW = those of them that arrived earlier (smaller input index).
    uint32_t h32 = 0x9E3779B9u;
#pragma unroll
    for (int k = 0; k < 8; k++) if (k < nwords) {
        const uint32_t lo = (uint32_t)nw[k], hi = (uint32_t)(nw[k] >> 32);
        h32 = (__builtin_rotateleft32(h32, 5) ^ lo) + hi;
        h32 = __builtin_rotateleft32(h32, 11) ^ (hi + 0x7F4A7C15u);
    }
    h32 ^= h32 >> 15;
    const unsigned long long ACT = __ballot(act);
    unsigned long long EQ = 0, LOW = 0;
    for (unsigned long long todo = ACT; todo;) {             // one ballot per DISTINCT hash: a whole name class at a time
        const int j = __ffsll((long long)todo) - 1;
        const uint32_t oh = (uint32_t)rl32((int)h32, j);
        const unsigned long long cls = __ballot(h32 == oh) & ACT;
        if (h32 == oh) EQ = cls;
        todo &= ~cls;
    }
    EQ &= ~(1ull << lane);
    {   // exact verification of every hash match (all lanes run the shuffles)
        bool bad = false;
        const int rounds = wave_max(act ? __popcll(EQ) : 0);
        unsigned long long rest = act ? EQ : 0ull;
        for (int r = 0; r < rounds; r++) {
            const bool has = rest != 0;
            const int src = has ? __ffsll((long long)rest) - 1 : lane;
            rest &= rest - 1;
            const uint32_t oj = (uint32_t)__shfl((int)my, src);
            if (has && oj < my) LOW |= 1ull << src;
#pragma unroll
            for (int k = 0; k < 8; k++) if (k < nwords) { const uint64_t o = (uint64_t)__shfl((long long)nw[k], src); if (o != nw[k]) bad = true; }
        }
        if (__any(bad)) { if (lane == 0) w.slow_list[atomicAdd(&w.si->n_slow_pair, 1u)] = c; return; }
    }
    // ---- pairs (cluster.cpp:260-273, pair.cpp:188-216): first read of a name = mLeft, last one = mRight
    const bool first = act && !(EQ & LOW), last = act && !(EQ & ~LOW);
    const unsigned long long FIRST = __ballot(first);
    const uint32_t npairs = __popcll(FIRST);
    // ---- map<string,Pair*> order: compares only against the first read of every OTHER name, and on ONE word: the 8 name bytes behind
    //      the cluster's common prefix decide nearly every comparison (the names share instrument / run / lane / tile); names whose
    //      order words tie take the full compare
    unsigned long long LT = 0;
    {
        int cpb = 64;                                       // bytes my name shares with the cluster's first read
#pragma unroll
        for (int k = 7; k >= 0; k--) if (k < nwords) { const uint64_t x = rl64(nw[k], 0) ^ nw[k]; if (x) cpb = 8 * k + (__clzll((long long)x) >> 3); }
        const int cp = min(wave_min(act ? cpb : 64), 56);
        uint64_t okey;
        {
            const int wi = cp >> 3, sh = 8 * (cp & 7);
            uint64_t a = 0, c2 = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) { if (k == wi) a = nw[k]; if (k == wi + 1) c2 = nw[k]; }
            okey = sh ? ((a << sh) | (c2 >> (64 - sh))) : a;
        }
        unsigned long long TIE = 0;
        for (unsigned long long fm = FIRST; fm; fm &= fm - 1) {
            const int j = __ffsll((long long)fm) - 1;
            const uint64_t o = rl64(okey, j);
            if (o < okey) LT |= 1ull << j;
            if (o == okey && !((EQ >> j) & 1ull) && j != lane) TIE |= 1ull << j;
        }
        for (unsigned long long tm = __ballot(act && TIE != 0) ? FIRST : 0ull; tm; tm &= tm - 1) {      // (rare) ties: whole names, for the lanes that have one with j
            const int j = __ffsll((long long)tm) - 1;
            int cmp = 0;                                    // sign of name_j - name_mine
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (k < nwords) {
                    uint64_t o = rl64(nw[k], j);
                    if (cmp == 0) cmp = o < nw[k] ? -1 : (o > nw[k] ? 1 : 0);
                }
            }
            if (((TIE >> j) & 1ull) && cmp < 0) LT |= 1ull << j;
        }
    }
    const uint32_t pidx = __popcll(LT);                     // distinct names before mine
    // every read's UMI as big-endian words in registers (<= 24 bytes, checked above): no byte loops over global memory below
    uint64_t ruw[3];
    load_be_words<3>(act ? uinfo_ptr(b, ui_) : nullptr, act ? ul : 0, ruw);
    {   // setRight (pair.cpp:201-212): the UMI must equal the pair's current UMI if that is non-empty.  The pair's current
        // read is the predecessor in arrival order = the largest read index among the same-name reads before mine.
        unsigned long long prev = act ? (EQ & LOW) : 0ull;
        const int rounds = wave_max(__popcll(prev));
        int plane = -1; uint32_t pv = 0;
        for (int r = 0; r < rounds; r++) {                  // (all lanes run the shuffles)
            const bool has = prev != 0;
            const int src = has ? __ffsll((long long)prev) - 1 : lane;
            prev &= prev - 1;
            const uint32_t o = (uint32_t)__shfl((int)my, src);
            if (has && (plane < 0 || o > pv)) { pv = o; plane = src; }
        }
        if (rounds > 0) {
            const int src = plane < 0 ? lane : plane;
            const uint64_t q0 = (uint64_t)__shfl((long long)ruw[0], src), q1 = (uint64_t)__shfl((long long)ruw[1], src), q2 = (uint64_t)__shfl((long long)ruw[2], src);
            const int qul = __shfl(ul, src);
            if (plane >= 0 && qul != 0 && !(qul == ul && q0 == ruw[0] && q1 == ruw[1] && q2 == ruw[2])) raise_error(w.si, GCE_ERR_UMI_MISMATCH, my);
        }
    }
    const int any_umi = __any(act && last && ul > 0);
    // ---- lanes now stand for pairs (qname order): every read pushes its fields to the lane of its pair (ds_permute).
    //      Lanes that have nothing to send aim at lane 63, which is a pair lane only when all 64 reads are mate-less
    //      singletons -- and then every lane sends.  Unwritten destination lanes read 0.
    const bool pact = lane < (int)npairs;
    uint32_t L = NONE32, R = NONE32, g_of = 0, ngroups = 1;
    {
        const int to_first = (first ? (int)pidx : 63) << 2, to_right = ((last && !first) ? (int)pidx : 63) << 2;
        L = (uint32_t)__builtin_amdgcn_ds_permute(to_first, first ? (int)(my + 1u) : 0) - 1u;
        R = (uint32_t)__builtin_amdgcn_ds_permute(to_right, (last && !first) ? (int)(my + 1u) : 0) - 1u;
        if (!pact) { L = NONE32; R = NONE32; }
    }
    if (any_umi) {                                           // greedy UMI grouping (cluster.cpp:57-100)
        uint64_t uw[3]; int ulen;
        {
            const int to_last = (last ? (int)pidx : 63) << 2;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(to_last, last ? (int)(uint32_t)ruw[k] : 0);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute(to_last, last ? (int)(uint32_t)(ruw[k] >> 32) : 0);
                uw[k] = pact ? (((uint64_t)hi << 32) | lo) : 0ull;
            }
            ulen = __builtin_amdgcn_ds_permute(to_last, last ? ul : 0);
            if (!pact) ulen = 0;
        }
        int cnt = 0, urank = 0;                              // umiCount[umi], and the rank of my UMI in std::string order
        {   // one round per DISTINCT UMI: its pairs learn their count, the pairs with a larger UMI add it to their rank
            const bool one_word = wave_max(ulen) <= 8;       // every UMI fits the first word (the usual 6-8 bp barcode)
            for (unsigned long long todo = __ballot(pact); todo;) {
                const int q = __ffsll((long long)todo) - 1;
                const uint64_t a0 = rl64(uw[0], q); const int al = rl32(ulen, q);
                bool eq, lt;
                if (one_word) { eq = a0 == uw[0] && al == ulen; lt = a0 != uw[0] ? a0 < uw[0] : al < ulen; }
                else {
                    const uint64_t a1 = rl64(uw[1], q), a2 = rl64(uw[2], q);
                    eq = a0 == uw[0] && a1 == uw[1] && a2 == uw[2] && al == ulen;
                    lt = a0 != uw[0] ? a0 < uw[0] : (a1 != uw[1] ? a1 < uw[1] : (a2 != uw[2] ? a2 < uw[2] : al < ulen));
                }
                const unsigned long long cls = __ballot(pact && eq);
                const int sz = __popcll(cls);
                if (pact && eq) cnt = sz;
                if (pact && lt) urank += sz;
                todo &= ~cls;
            }
        }
        g_of = NONE32; ngroups = 0;
        unsigned long long remaining = __ballot(pact);
        while (remaining) {
            int key = (pact && g_of == NONE32) ? (cnt * 64 + (63 - urank)) : -1;     // highest count, then smallest UMI
            int best = wave_max(key);
            int tl = __ffsll((long long)__ballot(key == best)) - 1;
            uint64_t t0 = rl64(uw[0], tl), t1 = rl64(uw[1], tl), t2 = rl64(uw[2], tl);
            int diff = popc_nonzero_bytes(t0 ^ uw[0]) + popc_nonzero_bytes(t1 ^ uw[1]) + popc_nonzero_bytes(t2 ^ uw[2]);   // Cluster::umiDiff
            bool take = pact && g_of == NONE32 && diff <= thr;
            if (take) g_of = ngroups;
            remaining &= ~__ballot(take);
            ngroups++;
        }
    }
    // ---- lay the pairs out group by group (qname order inside a group)
    uint32_t gbase = 0;
    for (uint32_t g = 0; g < ngroups; g++) {
        unsigned long long m = __ballot(pact && g_of == g);
        if (pact && g_of == g) { uint32_t d = start + gbase + lanes_below(m); w.gpl[d] = L; w.gpr[d] = R; }
        uint32_t run = __popcll(m);
        if (lane == 0) { w.grp_begin[start + g] = start + gbase; w.grp_n[start + g] = run; }
        gbase += run;
    }
    if (lane == 0) { const bool cross = d_key(b.core[w.members[start]], p).right < 0; w.cl_npairs[c] = npairs; w.cl_ngroups[c] = ngroups; w.cl_hasumi[c] = (uint8_t)((any_umi ? 1 : 0) | (cross ? 2 : 0)); w.cl_tier[c] = TIER_FAST; }
}
// one wave per cluster: every cluster (list == nullptr) or the clusters k_pairing_half (gce_pair2.hpp) flagged, compacted into pf_list
__global__ __launch_bounds__(256) void k_pairing_fast(DevBatch b, DevParams p, Work w, uint32_t n_clusters, const uint32_t *list) {
    const int lane = lane_id();
    const uint32_t total = list ? (uint32_t)w.si->n_pf_items : n_clusters, stride = gridDim.x * WAVES_PER_BLOCK;
    for (uint32_t idx = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); idx < total; idx += stride) {
        pairing_fast_cluster(b, p, w, list ? list[idx] : idx, lane);
        WAVE_SYNC();
    }
}
