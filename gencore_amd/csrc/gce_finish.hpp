// gce_finish.hpp — what follows the consensus of a group's sides: Cluster::consensusMerge's tail and Gencore::outputPair's decisions
// (cluster.cpp:116-244, pair.cpp:43-68, stats.cpp:123-139).
//
//   d_duplex_merge_bam, d_emit_pair, d_emit_group   the duplex merge of two groups' results; the OutRec of an emitted record
//   d_group_tail / k_group_tail   a thread per group: deferred NM patch, qname reconciliation, filter / FR tag and the Stats events of
//                    every group that is final there
//   finish_cluster_lanes, finish_cluster, k_finish_screen, k_finish   only when a UMI of the stream holds a '_': duplex merge / filter /
//                    FR, RR tags per cluster
//   k_raw_emit       clusters written as they are
//   k_stats          Stats events of the duplex stage's clusters
//   k_flag_reduce, k_flag_apply   a byte flag per item -> the ascending list of the flagged ones
// Stage consensus of engine.hip launches k_group_tail, k_finish_screen and k_finish behind the consensus kernels, stage output_table
// k_raw_emit and k_stats; the flag compaction is engine.hip's compact_flags (the pairing tiers' lists, the finish screen) and the record
// lists of gce_devstream.hpp and gce_samdev.hpp.
//
// A part of gce_kernels.hpp.
#pragma once

// ===================================================================================================== finish
// Cluster::duplexMergeBam (cluster.cpp:199-244).  The reference loop is
//     for(i=0;i<len;i++){ if(seq1[i/2]==seq2[i/2]){ i++; continue; } compare base i; mismatch -> N / qual 0 in both }
// i.e. a two-phase automaton over the packed bytes: arriving at a byte on its EVEN index it examines both nibbles;
// after a masked high nibble whose low nibbles agree the bytes become equal, the `i++; continue` lands on the ODD index
// of the next byte, and while it stays on odd indices only whole-byte equality and LOW nibbles are examined (a high
// nibble mismatch is then skipped) until an unequal byte re-synchronises it.  The phase each byte is entered in is
// computed exactly from two ballots (EQ = bytes equal, TO = byte sends the walk to the odd phase).
// Only b1 (the surviving pair) is written: b2 is deleted right after the merge (cluster.cpp:151-152).
__device__ inline int d_duplex_merge_bam(const DevBatch &b, uint32_t r1, uint32_t r2, int lane) {
    int l1 = b.core[r1].l_qseq, l2 = b.core[r2].l_qseq;
    int len = min(l1, l2), diff = 0;
    uint8_t *s1 = b.seq + b.seq_off[r1], *q1 = b.qual + b.qual_off[r1];
    const uint8_t *s2 = b.seq + b.seq_off[r2];
    const int nb = (len + 1) >> 1;
    bool phase_odd = false;                                  // phase in which the chunk's first byte is entered (wave-uniform)
    for (int base = 0; base < nb; base += 64) {
        int k = base + lane;
        bool valid = k < nb;
        uint8_t x = valid ? s1[k] : 0, y = valid ? s2[k] : 0;
        int xh = x >> 4, xl = x & 0xF, yh = y >> 4, yl = y & 0xF;
        bool has_lo = (2 * k + 1) < len;
        bool ne = valid && x != y;
        bool mark_hi = ne && d_base_class(xh) != d_base_class(yh);
        bool to_odd = mark_hi && xl == yl && has_lo;          // bytes equal after masking -> the walk continues on odd indices
        unsigned long long EQ = __ballot(!ne), TO = __ballot(to_odd);
        unsigned long long oddin = 0;
        int pos = 0; bool st = phase_odd;
        while (pos < 64) {
            if (!st) {
                unsigned long long m = TO & (~0ull << pos);
                if (!m) { pos = 64; break; }
                pos = __ffsll((long long)m);                 // index + 1: the byte after the one that switched phase
                st = true;
            } else {
                unsigned long long m = ~EQ & (~0ull << pos);
                int nx = m ? __ffsll((long long)m) - 1 : 64; // first unequal byte met in odd phase (it re-synchronises)
                unsigned long long upto = nx >= 63 ? ~0ull : ((2ull << nx) - 1ull);
                oddin |= upto & (~0ull << pos);
                if (nx == 64) pos = 64; else { pos = nx + 1; st = false; }
            }
        }
        phase_odd = st;
        bool in_odd = (oddin >> lane) & 1ull;
        if (ne) {
            if (!in_odd) {
                if (mark_hi) { diff++; xh = 15; q1[2 * k] = 0; }
                if (has_lo && !(mark_hi && xl == yl) && d_base_class(xl) != d_base_class(yl)) { diff++; xl = 15; q1[2 * k + 1] = 0; }
            } else if (has_lo && d_base_class(xl) != d_base_class(yl)) { diff++; xl = 15; q1[2 * k + 1] = 0; }
            s1[k] = (uint8_t)((xh << 4) | xl);
        }
    }
    return wave_sum(diff) + (l1 > l2 ? l1 - l2 : l2 - l1);
}

// Pair::writeSscsDcsTag + Gencore::outputPair of one result pair.  Everything comes as arguments: k_group_tail has it in registers, the duplex stage loads what
// k_group_tail stored for its clusters (d_emit_group).
__device__ inline void d_emit_pair(const Work &w, uint32_t l, uint32_t r, uint32_t merge, uint32_t rmerge, uint32_t qsl, uint32_t qsr, int nml, int nmr, bool duplex) {
    int fr = (int)min(merge, 65535u) & 0xFF;                                        // low byte of an unsigned short (quirk Q8)
    int rr = (int)min(rmerge, 65535u) & 0xFF;
    OutRec o; o.fr = (int16_t)fr; o.rr = duplex ? (int16_t)rr : (int16_t)-1; o.pad = 0;
    if (l != NONE32) { w.out_flag[l] = 1; o.qname_src = qsl; o.mate = r; o.nm_new = (int16_t)nml; w.orec[l] = o; }
    if (r != NONE32) { w.out_flag[r] = 1; o.qname_src = qsr; o.mate = l; o.nm_new = (int16_t)nmr; w.orec[r] = o; }
}
__device__ inline void d_emit_group(const Work &w, uint32_t gi, uint32_t l, uint32_t r, uint32_t merge, uint32_t rmerge, bool duplex) {      // a group of the duplex stage
    const int2 nv = *reinterpret_cast<const int2 *>(w.rp_nm + 2 * (size_t)gi);
    d_emit_pair(w, l, r, merge, rmerge, w.rp_qsl[gi], w.rp_qsr[gi], nv.x, nv.y, duplex);
}

// The tail of Group::consensusMerge (group.cpp:104-132) — mMergeReads, qname reconciliation, the new Pair's UMI — one
// THREAD per group; groups of clusters that cannot form a duplex (no UMI, --no_duplex, a single group, or a stream none of whose UMIs
// holds a '_': duplex_on == 0, StreamInfo::umi_us) are FINAL here: filtered, tagged and emitted (cluster.cpp:169-183; with one group or
// one-token UMIs the duplex loop finds no partner, :157-166), and their Stats events (addMolecule, addSSCS, outputPair's addMolecule(1, PE),
// addCluster before and after: cluster.cpp:102,185-187) are counted from the registers -- nothing of such a group is stored for a later
// kernel.  Groups of the other clusters are left pending for k_finish, with everything it needs in the rp_* arrays; k_stats counts those.
enum { TF_FINAL = 1, TF_PE = 2, TF_OUT = 4, TF_CFIRST = 8, TF_CMULTI = 16, TF_POSTC = 32, TF_POSTM = 64 };
__device__ __forceinline__ uint32_t d_group_tail(const DevBatch &b, const DevParams &p, const Work &w, uint32_t gi, bool duplex_on, uint32_t &supp, uint32_t &cl_pairs) {
    // everything the group index alone addresses is asked for first, then what hangs on the cluster and on the result reads: two round trips in a row, not four
    // (a skipped group's rp_left / rp_right are still NONE32, its rp_nm -1: the clears of the step)
    const uint32_t c = w.gl_cluster[gi], c_prev = gi ? w.gl_cluster[gi - 1] : NONE32;
    const uint32_t begin = w.g_begin[gi], np = w.g_np[gi];
    const uint32_t left = w.rp_left[gi], right = w.rp_right[gi];
    int2 nmv = *reinterpret_cast<const int2 *>(w.rp_nm + 2 * (size_t)gi);
    const uint8_t cflags = w.cl_hasumi[c];
    const uint32_t G = w.cl_ngroups[c];
    // the two templates' name lengths and UMI places: one word each (round 5; core record + UMI pointer + UMI length + MI flag were four sectors per side)
    const uint64_t uL = left != NONE32 ? w.uinfo[left] : 0ull, uR = right != NONE32 ? w.uinfo[right] : 0ull;
    const bool duplex_cluster = duplex_on && (cflags & 1) && !p.disable_duplex && G >= 2;
    uint32_t tf = 0;
    if (!duplex_cluster && c_prev != c) {                 // the cluster's first group: Stats::addCluster before and after, the pairs behind timing.n_pairs
        tf |= TF_CFIRST | (G > 1 ? TF_CMULTI : 0);
        cl_pairs = w.cl_npairs[c];
        if (G > 1 && !p.duplex_only) {                                                // written groups among the siblings: merge == pairs of the group (below), a skipped group has one pair
            uint32_t nr = 0;
            for (uint32_t g = 0; g < G && nr < 2; g++) nr += (int)w.g_np[gi + g] >= p.cluster_size_req;
            tf |= (nr > 0 ? TF_POSTC : 0) | (nr > 1 ? TF_POSTM : 0);
        }
    }
    if (d_group_skipped(p, cflags, G, np)) {
        // no kernel looked at this group (k_group_fill) and its cluster forms no duplex: one supporting read, never written
        supp = 1;
        return tf | TF_FINAL | ((w.gpl[begin] != NONE32 && w.gpr[begin] != NONE32) ? TF_PE : 0);
    }
    {   // the NM patches k_vote deferred (group.cpp:528-573): mismatchInc != 0 reads the template's NM tag -- absent: the reference crashes (quirk Q9);
        // mismatchInc > 5: the template was restored, NM stays; else NM + mismatchInc goes into the tag if it is stored as type 'C' and stays a byte
        if (NM_IS_DEFERRED(nmv.x) || NM_IS_DEFERRED(nmv.y)) {
            auto resolve = [&](int v, uint32_t out) -> int {
                if (!NM_IS_DEFERRED(v)) return v;
                const int minc = v - NM_DEFER, ty = b.nm_type[out], nn = b.nm[out] + minc;
                if (ty == 0) { raise_error(w.si, GCE_ERR_NM_MISSING, out); return -1; }
                return (minc <= 5 && ty == 'C' && nn >= 0 && nn <= 255) ? nn : -1;
            };
            nmv.x = resolve(nmv.x, left); nmv.y = resolve(nmv.y, right);
            if (duplex_cluster) *reinterpret_cast<int2 *>(w.rp_nm + 2 * (size_t)gi) = nmv;
        }
    }
    const bool single = np == 1 && w.gpr[begin] == NONE32;
    uint32_t qsl = left, qsr = right;                                     // BamUtil::copyQName sources (== the record itself if unchanged)
    if (!single) {
        if (cflags & 2) {                                                 // cross-contig cluster: group.cpp:79-99,109-112
            uint32_t ntc = NONE32; int bl = 0;
            for (uint32_t k = 0; k < np; k++) {
                uint32_t l = w.gpl[begin + k];
                int ll = d_lqname_pad(b.core[l]);
                if (ntc == NONE32 || ll < bl || (ll == bl && d_strcmp(d_qname(b, l), d_qname(b, ntc)) < 0)) { ntc = l; bl = ll; }
            }
            if (left != NONE32 && ntc != NONE32 && ntc != left) {
                if (d_lqname_pad(b.core[left]) < d_lqname_pad(b.core[ntc])) raise_error(w.si, GCE_ERR_QNAME_SHORT, left);
                qsl = ntc;
            }
        } else if (left != NONE32 && right != NONE32) {                   // group.cpp:114-123
            if (uinfo_lqname_pad(uL) <= uinfo_lqname_pad(uR)) qsr = left;
            else qsl = right;
        }
    }
    const uint32_t merge = single ? 1 : np;                               // (== np: a single has one pair)
    const char *u = nullptr; int ul = 0;                                  // Pair::setLeft / setRight (pair.cpp:188-216)
    if ((cflags & 1) || b.mi) {
        auto rec_umi = [&](uint64_t vrec, uint32_t src, const char *&uo, int &ulo) {       // d_record_umi on the words already here
            if (uinfo_hm(vrec)) { uo = uinfo_ptr(b, vrec); ulo = uinfo_len(vrec); return; }
            const uint64_t vn = src == left ? uL : (src == right ? uR : w.uinfo[src]);
            if (!uinfo_hm(vn)) { uo = uinfo_ptr(b, vn); ulo = uinfo_len(vn); return; }
            const char *q = d_qname(b, src); int s0, l0;
            d_umi_slice(q, p, s0, l0);
            uo = q + s0; ulo = l0;
        };
        if (left != NONE32) rec_umi(uL, qsl, u, ul);
        if (right != NONE32) {
            const char *u2; int ul2;
            rec_umi(uR, qsr, u2, ul2);
            if (left != NONE32 && ul != 0) {                               // (two word loads per side instead of a byte loop with a data-dependent exit)
                bool same = ul == ul2;
                if (same && u == u2) { }                                    // both records carry the same read's name (the usual case): nothing to fetch
                else if (same && ul <= 24) { uint64_t a[3], c3[3]; load_be_words<3>(u, ul, a); load_be_words<3>(u2, ul2, c3); same = a[0] == c3[0] && a[1] == c3[1] && a[2] == c3[2]; }
                else if (same) same = d_bytes_equal(u, ul, u2, ul2);
                if (!same) raise_error(w.si, GCE_ERR_UMI_MISMATCH, right);
            }
            u = u2; ul = ul2;
        }
    }
    if (duplex_cluster) {                                                 // -> k_finish, k_stats
        w.rp_qsl[gi] = qsl; w.rp_qsr[gi] = qsr;
        w.rp_merge[gi] = merge; w.rp_rmerge[gi] = 0; w.rp_umi[gi] = u; w.rp_umilen[gi] = (uint16_t)ul;
        w.rp_state[gi] = RP_PENDING; w.rp_supp[gi] = -1;
        return tf;
    }
    const bool outp = !p.duplex_only && (int)merge >= p.cluster_size_req;
    if (outp) d_emit_pair(w, left, right, merge, 0u, qsl, qsr, nmv.x, nmv.y, false);
    if (G == 1 && outp) tf |= TF_POSTC;
    supp = merge;
    return tf | TF_FINAL | ((left != NONE32 && right != NONE32) ? TF_PE : 0) | (outp ? TF_OUT : 0);
}
__global__ __launch_bounds__(256) void k_group_tail(DevBatch b, DevParams p, Work w, uint32_t n_groups, int duplex_on) {
    __shared__ unsigned int s_hist[GCE_MAX_SUPPORTING_READS];
    __shared__ unsigned long long s_ts[TS_WORDS];
    if (threadIdx.x < GCE_MAX_SUPPORTING_READS) s_hist[threadIdx.x] = 0;
    if (threadIdx.x < TS_WORDS) s_ts[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t tf = 0, supp = 0, cl_pairs = 0;
    if (gi < n_groups) tf = d_group_tail(b, p, w, gi, duplex_on != 0, supp, cl_pairs);
    // Stats: every counter but the pair count is a predicate of the thread -- a ballot per counter and wave, the histogram through LDS, then one
    // set of atomics per block on one of GCE_TAIL_SLOTS address sets (the host and k_fold_stats add them up)
    const bool fin = tf & TF_FINAL, out = tf & TF_OUT, pe = tf & TF_PE;
    const bool uncounted = fin && supp >= (uint32_t)GCE_MAX_SUPPORTING_READS;
    if (fin && !uncounted) atomicAdd(&s_hist[supp], 1u);
    unsigned int cnt[TS_WORDS];
    cnt[TS_PRE_CLUSTERS] = __popcll(__ballot(tf & TF_CFIRST)); cnt[TS_PRE_MULTI] = __popcll(__ballot(tf & TF_CMULTI));
    cnt[TS_PRE_MOLECULES] = __popcll(__ballot(fin)); cnt[TS_PRE_SE] = __popcll(__ballot(fin && !pe)); cnt[TS_PRE_PE] = __popcll(__ballot(fin && pe));
    cnt[TS_PRE_UNCOUNTED] = __popcll(__ballot(uncounted));
    cnt[TS_NPAIRS] = 0;
    cnt[TS_POST_CLUSTERS] = __popcll(__ballot(tf & TF_POSTC)); cnt[TS_POST_MULTI] = __popcll(__ballot(tf & TF_POSTM));
    cnt[TS_POST_SSCS] = __popcll(__ballot(out)); cnt[TS_POST_SE] = __popcll(__ballot(out && !pe)); cnt[TS_POST_PE] = __popcll(__ballot(out && pe));
    const long long npw = wave_sum64((long long)cl_pairs);
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < TS_WORDS; k++) if (cnt[k]) atomicAdd(&s_ts[k], (unsigned long long)cnt[k]);
        if (npw) atomicAdd(&s_ts[TS_NPAIRS], (unsigned long long)npw);
    }
    __syncthreads();
    if (threadIdx.x < TS_WORDS && s_ts[threadIdx.x]) atomicAdd((unsigned long long *)&w.si->tail_slot[blockIdx.x & (GCE_TAIL_SLOTS - 1)][threadIdx.x], s_ts[threadIdx.x]);
    if (threadIdx.x < GCE_MAX_SUPPORTING_READS && s_hist[threadIdx.x]) atomicAdd((unsigned long long *)&w.si->tail_hist[(blockIdx.x >> 4) & (GCE_TAIL_HSLOTS - 1)][threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
}

// Duplex matching (cluster.cpp:119-168), one wave per cluster that has UMIs and at least two groups.
// Round 5: a cluster of <= 64 groups keeps its groups in the LANES -- state, reads, merge count, and the two '_'-separated tokens of the UMI as zero-padded big-endian
// words (UMI characters are never NUL, so equal words are equal strings: Cluster::isDuplex, cluster.cpp:246-258, is two 64-bit compares) -- and the walk from the
// last group down is a broadcast and a ballot per group.  The walk over memory below (any number of groups, tokens of any length) loads every partner's UMI bytes
// and state again for every group: ~8 dependent round trips per group on a one-wave chain, 305 us at cfg5 for clusters of ~45 groups.
__device__ bool finish_cluster_lanes(const DevBatch &b, const DevParams &p, const Work &w, uint32_t g0, uint32_t G, int lane) {
    const bool in = lane < (int)G;
    const uint32_t gme = g0 + (uint32_t)lane;
    uint32_t l = NONE32, r = NONE32, m = 0; uint64_t t0 = 0, t1 = 0; bool two = false, lng = false;
    if (in) {
        const char *u = w.rp_umi[gme]; const int ul = w.rp_umilen[gme];
        l = w.rp_left[gme]; r = w.rp_right[gme]; m = w.rp_merge[gme];
        int s0, l0, s1, l1;
        two = d_split2(u, ul, s0, l0, s1, l1) == 2;
        if (two) {
            if (l0 > 8 || l1 > 8) lng = true;
            else { uint64_t a[1], c2[1]; load_be_words<1>(u + s0, l0, a); load_be_words<1>(u + s1, l1, c2); t0 = a[0]; t1 = c2[0]; }
        }
    }
    if (__any(lng)) return false;                            // a token beyond eight bytes: the walk over memory
    int st = RP_PENDING;                                     // (k_group_tail left every group of such a cluster pending)
    for (int idx = (int)G - 1; idx >= 0; idx--) {
        if (__shfl(st, idx) == RP_CONSUMED) continue;        // (wave-uniform)
        const uint64_t a0 = (uint64_t)__shfl((long long)t0, idx), a1 = (uint64_t)__shfl((long long)t1, idx);
        const int atwo = __shfl((int)two, idx);
        const bool hit = lane < idx && st == RP_PENDING && two && atwo && a0 == t1 && a1 == t0;
        const unsigned long long hm = __ballot(hit);
        const uint32_t gi = g0 + (uint32_t)idx;
        const uint32_t l1 = (uint32_t)__shfl((int)l, idx), r1 = (uint32_t)__shfl((int)r, idx), m1 = (uint32_t)__shfl((int)m, idx);
        if (hm) {
            const int found = __ffsll((long long)hm) - 1;    // the first partner in group order (cluster.cpp:130-141)
            const uint32_t g2 = g0 + (uint32_t)found;
            const uint32_t l2 = (uint32_t)__shfl((int)l, found), r2 = (uint32_t)__shfl((int)r, found), m2 = (uint32_t)__shfl((int)m, found);
            int diff = 0;
            if (l1 != NONE32 && l2 != NONE32) diff += d_duplex_merge_bam(b, l1, l2, lane);
            if (r1 != NONE32 && r2 != NONE32) diff += d_duplex_merge_bam(b, r1, r2, lane);
            const bool outp = diff <= p.duplex_mismatch_thr && (int)(m1 + m2) >= p.cluster_size_req;
            if (lane == idx) st = outp ? RP_OUT_DCS : RP_DROPPED;
            if (lane == found) st = RP_CONSUMED;
            if (lane == 0) {
                w.rp_supp[gi] = (int)(m1 + m2);
                w.rp_rmerge[gi] = m2;
                w.rp_state[gi] = outp ? RP_OUT_DCS : RP_DROPPED;
                w.rp_state[g2] = RP_CONSUMED;
                if (outp) d_emit_group(w, gi, l1, r1, m1, m2, true);
            }
            WAVE_SYNC();                                     // (the merged bases / qualities of this pair before anybody reads them again)
        } else {
            const bool outp = !p.duplex_only && (int)m1 >= p.cluster_size_req;
            if (lane == idx) st = outp ? RP_OUT_SSCS : RP_DROPPED;
            if (lane == 0) { w.rp_supp[gi] = (int)m1; w.rp_state[gi] = outp ? RP_OUT_SSCS : RP_DROPPED; if (outp) d_emit_group(w, gi, l1, r1, m1, 0u, false); }
        }
    }
    return true;
}
__device__ void finish_cluster(const DevBatch &b, const DevParams &p, const Work &w, uint32_t c, int lane) {
    const uint32_t G = w.cl_ngroups[c];
    const uint32_t g0 = w.cl_gbase[c];
    if (G <= 64u && finish_cluster_lanes(b, p, w, g0, G, lane)) return;
    for (int idx = (int)G - 1; idx >= 0; idx--) {
        uint32_t gi = g0 + idx;
        if (w.rp_state[gi] == RP_CONSUMED) continue;
        const char *u1 = w.rp_umi[gi]; int ul1 = w.rp_umilen[gi];
        uint32_t found = NONE32;
        for (int base = 0; base < idx && found == NONE32; base += 64) {
            int i = base + lane;
            bool hit = i < idx && w.rp_state[g0 + i] == RP_PENDING && d_is_duplex(u1, ul1, w.rp_umi[g0 + i], w.rp_umilen[g0 + i]);
            unsigned long long m = __ballot(hit);
            if (m) found = base + (__ffsll((long long)m) - 1);
        }
        uint32_t l1 = w.rp_left[gi], r1 = w.rp_right[gi], m1 = w.rp_merge[gi];
        if (found != NONE32) {
            uint32_t g2 = g0 + found;
            uint32_t l2 = w.rp_left[g2], r2 = w.rp_right[g2], m2 = w.rp_merge[g2];
            int diff = 0;
            if (l1 != NONE32 && l2 != NONE32) diff += d_duplex_merge_bam(b, l1, l2, lane);
            if (r1 != NONE32 && r2 != NONE32) diff += d_duplex_merge_bam(b, r1, r2, lane);
            bool outp = diff <= p.duplex_mismatch_thr && (int)(m1 + m2) >= p.cluster_size_req;
            if (lane == 0) {
                w.rp_supp[gi] = (int)(m1 + m2);
                w.rp_rmerge[gi] = m2;
                w.rp_state[gi] = outp ? RP_OUT_DCS : RP_DROPPED;
                w.rp_state[g2] = RP_CONSUMED;
                if (outp) d_emit_group(w, gi, l1, r1, m1, m2, true);
            }
        } else {
            bool outp = !p.duplex_only && (int)m1 >= p.cluster_size_req;
            if (lane == 0) { w.rp_supp[gi] = (int)m1; w.rp_state[gi] = outp ? RP_OUT_SSCS : RP_DROPPED; if (outp) d_emit_group(w, gi, l1, r1, m1, 0u, false); }
        }
        WAVE_SYNC();
    }
}
// Few clusters need the duplex stage (UMIs and >= 2 groups): they are flagged, compacted, and then get a wave each -- a deep amplicon
// cluster with a hundred UMI groups keeps its wave busy for a long time, and 64 neighbouring clusters behind one wave (the first
// version) serialised exactly those.
__global__ __launch_bounds__(256) void k_finish_screen(Work w, uint32_t n_clusters, uint8_t *flag) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_clusters) flag[c] = w.cl_ngroups[c] >= 2 && (w.cl_hasumi[c] & 1);
}
__global__ __launch_bounds__(256) void k_finish(DevBatch b, DevParams p, Work w, const uint32_t *list, const unsigned long long *list_n) {
    const int lane = lane_id();
    const uint32_t n = (uint32_t)*list_n;
    for (uint32_t k = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); k < n; k += gridDim.x * WAVES_PER_BLOCK) {
        finish_cluster(b, p, w, list[k], lane);
        WAVE_SYNC();
    }
}

// ===================================================================================================== clusters written as they are
// finishConsensus on a cluster with left < 0 (gencore.cpp:401-407): every Pair of the name map goes to outputPair as Cluster::addRead built it
// (cluster.cpp:260-273: the first read of a name is the left one, every later one replaces the right one -- Pair::setRight checks its UMI,
// pair.cpp:195-216), without clusterByUMI: no group, no consensus, no tag, no Stats but outputPair's addMolecule(1, PE).  Such keys need a
// malformed mate position (mpos == -1 on the read's own contig); one thread per cluster, launched only when k_leaders met one.
__global__ __launch_bounds__(256) void k_raw_emit(DevBatch b, DevParams p, Work w, uint32_t n_clusters) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters || d_thr_mode(w.cl_ikey[c], w.si, p) != THR_RAW) return;
    const uint32_t start = w.cl_start[c], n = w.cl_n[c];
    auto same = [&](const char *x, const char *y) { int k = 0; while (x[k] && x[k] == y[k]) k++; return x[k] == y[k]; };
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t ra = w.members[start + a];
        const char *qa = d_qname(b, ra);
        bool first = true;
        for (uint32_t x = 0; x < n && first; x++) { const uint32_t rx = w.members[start + x]; if (rx < ra && same(qa, d_qname(b, rx))) first = false; }
        if (!first) continue;
        uint32_t right = NONE32, prev = ra; uint64_t pu = w.uinfo[ra];
        for (;;) {                                                                       // the name's later reads in arrival order
            uint32_t nx = NONE32;
            for (uint32_t x = 0; x < n; x++) { const uint32_t rx = w.members[start + x]; if (rx > prev && rx < nx && same(qa, d_qname(b, rx))) nx = rx; }
            if (nx == NONE32) break;
            const uint64_t u = w.uinfo[nx];
            const int ul = uinfo_len(u), pl = uinfo_len(pu);
            bool eq = ul == pl;
            if (eq) { const char *s1 = uinfo_ptr(b, u), *s2 = uinfo_ptr(b, pu); for (int k = 0; k < ul; k++) eq = eq && s1[k] == s2[k]; }
            if (pl != 0 && !eq) raise_error(w.si, GCE_ERR_UMI_MISMATCH, nx); else pu = u;
            right = nx; prev = nx;
        }
        OutRec o; o.nm_new = -1; o.fr = -1; o.rr = -1; o.pad = 0;
        w.out_flag[ra] = 1; o.qname_src = ra; o.mate = right; w.orec[ra] = o;
        if (right != NONE32) { w.out_flag[right] = 1; o.qname_src = right; o.mate = ra; w.orec[right] = o; }
        atomicAdd((unsigned long long *)&w.si->post[8], 1ull); atomicAdd((unsigned long long *)&w.si->post[14 + 1], 1ull);
        atomicAdd((unsigned long long *)&w.si->post[right != NONE32 ? 10 : 9], 1ull);
    }
}

// ===================================================================================================== Stats
// All counters are additive (stats.h:47-65).  Block-local accumulation in LDS, one global atomic per non-zero counter.
// (Stats::addRead of the emitted records: k_out_meta, gce_output.hpp)
// Only the clusters that went through the duplex stage (UMIs and two or more groups; launched when that stage ran): every other group was final in k_group_tail
// and is counted there.  A group's thread looks at its cluster's flags; the cluster's first group counts the cluster.
__global__ __launch_bounds__(256) void k_stats(DevBatch b, Work w, uint32_t n_groups) {
    __shared__ unsigned long long s_pre[GCE_STATS_WORDS], s_post[GCE_STATS_WORDS], s_np;
    for (int k = threadIdx.x; k < GCE_STATS_WORDS; k += blockDim.x) { s_pre[k] = 0; s_post[k] = 0; }
    if (threadIdx.x == 0) s_np = 0;
    __syncthreads();
    const uint64_t tid0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    // indices into gce_stats: 0 reads, 1 bases, 2 reads_unmapped, 3 bases_unmapped, 4 mismatches, 5 reads_with_mismatches,
    // 6 clusters, 7 multi, 8 molecules, 9 se, 10 pe, 11 sscs, 12 dcs, 13 uncounted, 14.. hist.
    // The scalar counters are summed in registers and reduced per wave at the end (64 lanes adding to one LDS word serialise);
    // only the histogram goes through LDS atomics.
    long long pre[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, post[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, np = 0, post_h1 = 0;
    for (uint64_t g = tid0; g < n_groups; g += stride) {
        const uint32_t c = w.gl_cluster[g];
        const uint32_t G = w.cl_ngroups[c];
        if (!(w.cl_hasumi[c] & 1) || G < 2) continue;                                    // final in k_group_tail
        if (g == 0 || w.gl_cluster[g - 1] != c) {
            pre[6] += 1; pre[7] += 1;                                                    // cluster.cpp:102
            np += w.cl_npairs[c];
            uint32_t nr = 0; for (uint32_t k = 0; k < G; k++) { uint8_t st = w.rp_state[g + k]; nr += (st == RP_OUT_SSCS || st == RP_OUT_DCS); }
            if (nr > 0) { post[6] += 1; if (nr > 1) post[7] += 1; }                     // cluster.cpp:185-187
        }
        int supp = w.rp_supp[g];
        if (supp < 0) continue;                                                          // consumed as the reverse strand: no event
        bool pe = w.rp_left[g] != NONE32 && w.rp_right[g] != NONE32;
        pre[8] += 1;                                                                     // Stats::addMolecule, stats.cpp:123-133
        if (supp < GCE_MAX_SUPPORTING_READS) atomicAdd(&s_pre[14 + supp], 1ull); else pre[13] += 1;
        pre[pe ? 10 : 9] += 1;
        uint8_t st = w.rp_state[g];
        if (st == RP_OUT_SSCS || st == RP_OUT_DCS) {
            post[st == RP_OUT_DCS ? 12 : 11] += 1;                                       // addSSCS / addDCS
            post[8] += 1; post_h1 += 1; post[pe ? 10 : 9] += 1;                          // outputPair: addMolecule(1, PE)
        }
    }
    const int lane = lane_id();
#pragma unroll
    for (int k = 0; k < 14; k++) {
        const long long a = wave_sum64(pre[k]), c2 = wave_sum64(post[k]);
        if (lane == 0) { if (a) atomicAdd(&s_pre[k], (unsigned long long)a); if (c2) atomicAdd(&s_post[k], (unsigned long long)c2); }
    }
    { const long long a = wave_sum64(np), c2 = wave_sum64(post_h1); if (lane == 0) { if (a) atomicAdd(&s_np, (unsigned long long)a); if (c2) atomicAdd(&s_post[14 + 1], (unsigned long long)c2); } }
    __syncthreads();
    for (int k = threadIdx.x; k < GCE_STATS_WORDS; k += blockDim.x) {
        if (s_pre[k]) atomicAdd((unsigned long long *)&w.si->pre[k], s_pre[k]);
        if (s_post[k]) atomicAdd((unsigned long long *)&w.si->post[k], s_post[k]);
    }
    if (threadIdx.x == 0 && s_np) atomicAdd(&w.si->n_pairs_total, s_np);
}

// out_index: ascending list of emitted reads (3-phase scan over out_flag != 0)
__global__ __launch_bounds__(256) void k_flag_reduce(const uint8_t *flag, uint64_t n, uint64_t *part) {
    __shared__ uint64_t s[4];
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE, v = 0;
    for (int k = 0; k < SCAN_TILE / 256; k++) { uint64_t i = base + k * 256 + threadIdx.x; v += (i < n && flag[i]) ? 1 : 0; }
    v = (uint64_t)wave_sum64((long long)v);
    if (lane_id() == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (s[0] + s[1] + s[2] + s[3]) << 32;    // keep the total in the high word like the table scan
}
__global__ __launch_bounds__(256) void k_flag_apply(const uint8_t *flag, uint64_t n, const uint64_t *part, uint32_t *out_index) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_carry;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = (uint32_t)(part[blockIdx.x] >> 32);
    __syncthreads();
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    for (int k = 0; k < SCAN_TILE / 256; k++) {
        uint64_t i = base + k * 256 + threadIdx.x;
        bool f = i < n && flag[i];
        unsigned long long m = __ballot(f);
        if (lane == 0) s_w[wv] = __popcll(m);
        __syncthreads();
        uint32_t woff = 0;
        for (int q = 0; q < wv; q++) woff += s_w[q];
        uint32_t carry = s_carry;
        if (f) out_index[carry + woff + lanes_below(m)] = (uint32_t)i;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}
