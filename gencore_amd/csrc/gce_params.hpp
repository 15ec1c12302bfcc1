// gce_params.hpp — the scalar fields of DevParams derived from the caller's parameters: host arithmetic only (no engine, no HIP call), with an
// edge at every power of two.  tests/params_host_check.hip calls it without a GPU.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "gce_kernels.hpp"      // DevParams (gce_device.hpp), TAB_WAYS (gce_cluster.hpp)

// Fills every scalar field of *out for a step of N reads over a bucket table of `tsize` entries; the device pointers (target_len, target_cum, ref_*) and
// n_ref stay the caller's.  GCE_ERR_INVALID: score constants out of range.  *vote_off_why: why k_vote is off for these parameters (vote_ok 0), or null.
static inline int make_dev_params(const gce_params &prm, const std::vector<uint32_t> &target_len, bool have_tick, int64_t N, uint64_t tsize, DevParams *out, const char **vote_off_why) {
    DevParams &p = *out;
    *vote_off_why = nullptr;
    p.proper_thr = prm.proper_umi_diff_threshold; p.unproper_thr = prm.unproper_umi_diff_threshold;
    p.duplex_mismatch_thr = prm.duplex_mismatch_threshold; p.cluster_size_req = prm.cluster_size_req; p.base_score_req = prm.base_score_req;
    p.high_q = prm.high_quality; p.moderate_q = prm.moderate_quality; p.low_q = prm.low_quality;
    p.s_high = prm.score_high; p.s_moderate = prm.score_moderate; p.s_low = prm.score_low; p.s_bad = prm.score_bad;
    p.skip_low_complexity_thr = prm.skip_low_complexity_cluster_threshold; p.duplex_only = prm.duplex_only; p.disable_duplex = prm.disable_duplex;
    p.period = prm.flush_period; p.score_percent_req = prm.score_percent_req;
    {   // scores are qual2score(q) in {s_*}, +4 on overlap match, -3 on overlap mismatch, or 0 (pair.cpp:77-172)
        int mn = std::min(std::min(p.s_high, p.s_moderate), std::min(p.s_low, p.s_bad)), mx = std::max(std::max(p.s_high, p.s_moderate), std::max(p.s_low, p.s_bad));
        p.score_bias = std::max(0, 3 - mn); p.score_max = std::max(0, mx + 4);
        if (p.score_max + p.score_bias > 255) return GCE_ERR_INVALID;
        auto by = [&](int sc) { return (uint32_t)((sc + p.score_bias) & 0xFF); };
        p.q2s_lut = by(p.s_bad) | by(p.s_low) << 8 | by(p.s_moderate) << 16 | by(p.s_high) << 24;
        p.thr_low4 = 0x01010101u * (uint32_t)(p.low_q & 0xFF); p.thr_mod4 = 0x01010101u * (uint32_t)(p.moderate_q & 0xFF); p.thr_high4 = 0x01010101u * (uint32_t)(p.high_q & 0xFF);
        p.q2s_swar_ok = p.low_q >= 0 && p.low_q <= p.moderate_q && p.moderate_q <= p.high_q && p.high_q <= 127;
        // k_vote (gce_vote.hpp): scores in a sane range (the packed tally keys of decide_column_packed), and whether a unanimous column whose
        // top quality reaches `moderate` is bound to reach baseScoreReq too: that voter scores s_moderate or s_high (or >= min + 4 inside a
        // matching mate overlap) and nobody scores below 0
        p.s_min_lb = mn;
        p.vote_ok = mn >= 0 && mx + 4 <= 120 && p.moderate_q >= 0 && p.moderate_q <= 127 && p.base_score_req <= 100 && p.q2s_swar_ok;   // (nested thresholds: k_vote's items index q2s_lut by the number of thresholds passed)
        p.vote_accept_by_qual = std::min(std::min(p.s_moderate, p.s_high), mn + 4) >= std::max(p.base_score_req, 1);
        if (!p.vote_ok)      // every group then goes to k_score2 and the per-side kernels
            *vote_off_why = !p.q2s_swar_ok ? "quality thresholds not nested (low <= moderate <= high <= 127)" : mn < 0 ? "a score constant below 0"
                          : mx + 4 > 120 ? "a score constant above 116" : (p.moderate_q < 0 || p.moderate_q > 127) ? "moderate quality outside 0..127" : "base_score_req above 100";
    }
    memcpy(p.prefix, prm.umi_prefix, 32); p.prefix[31] = 0; p.prefix_len = (int)strlen(p.prefix);
    p.n_targets = (int)target_len.size();
    p.tick_offset = have_tick ? 0 : prm.tick_offset; p.tick_epoch0 = p.tick_offset / p.period; p.tick_rem0 = (int32_t)(p.tick_offset % p.period); p.trailing_flush = have_tick ? 0 : prm.trailing_flush;
    {   // packed cluster key of the bucket table: bits of the largest tid and of the longest contig
        uint32_t mx = 1; for (uint32_t v : target_len) mx = std::max(mx, v);
        int bt = 1; while (bt < 31 && (1ll << bt) < (long long)std::max<size_t>(target_len.size(), 1)) bt++;
        int bl = 1; while (bl < 32 && (1ull << bl) <= (uint64_t)mx) bl++;
        p.key_bt = bt; p.key_bl = bl;
    }
    {   // normal bucket words: OCC | x div T | right - left + 1 | reads (gce_cluster.hpp, k_leaders)
        uint64_t genome = 0; for (uint32_t v : target_len) genome += v;
        const uint64_t qmax = (genome * TAB_WAYS + TAB_WAYS) / tsize + 1;
        int cb = 1; while (cb < 33 && (1ull << cb) <= (uint64_t)N + 1024) cb++;
        int qb = 1; while (qb < 52 && (1ull << qb) <= qmax) qb++;
        p.nw_cb = cb; p.nw_bd = 62 - cb - qb; p.nw_ok = !target_len.empty() && p.nw_bd >= 1;
        if (p.nw_bd > 40) p.nw_bd = 40;
    }
    return GCE_OK;
}
