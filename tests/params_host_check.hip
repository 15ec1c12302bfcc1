// make_dev_params of gencore_amd/csrc/gce_params.hpp -- the scalar fields of DevParams, derived on the host -- called without an engine and without
// a GPU (tests/test_params_host.py), built with the address and undefined-behaviour sanitizers for the host.  No kernel is launched.
// Usage: params_host_check CASE...      CASE = label,key=value,...   over a zeroed gce_params:
//   the integer fields of gce_params by name; prefix=TEXT (umi_prefix, up to 32 bytes and then without a NUL); nt= and len=: that many targets, all
//   of that length; N=, tsize=, have_tick=: the function's other arguments.
// One output line per case: "<label> rc=-1", or "<label> rc=0" and every scalar field.
#include <hip/hip_runtime.h>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "../gencore_amd/csrc/gce_params.hpp"

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        std::unique_ptr<gce_params> prm(new gce_params());          // (on the heap, of exactly its size: a sanitizer sees a read past umi_prefix[32])
        uint64_t nt = 0, len = 0, tsize = 0; int64_t N = 0; bool have_tick = false;
        std::stringstream ss(argv[a]); std::string label, kv;
        std::getline(ss, label, ',');
        while (std::getline(ss, kv, ',')) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad case %s\n", argv[a]); return 2; }
            const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
            const long long i = strtoll(v.c_str(), nullptr, 0);
            struct { const char *name; int32_t *field; } ints[] = {
                {"proper_umi_diff_threshold", &prm->proper_umi_diff_threshold}, {"unproper_umi_diff_threshold", &prm->unproper_umi_diff_threshold},
                {"duplex_mismatch_threshold", &prm->duplex_mismatch_threshold}, {"cluster_size_req", &prm->cluster_size_req}, {"base_score_req", &prm->base_score_req},
                {"high_quality", &prm->high_quality}, {"moderate_quality", &prm->moderate_quality}, {"low_quality", &prm->low_quality},
                {"score_high", &prm->score_high}, {"score_moderate", &prm->score_moderate}, {"score_low", &prm->score_low}, {"score_bad", &prm->score_bad},
                {"skip_low_complexity_cluster_threshold", &prm->skip_low_complexity_cluster_threshold}, {"duplex_only", &prm->duplex_only},
                {"disable_duplex", &prm->disable_duplex}, {"flush_period", &prm->flush_period}, {"trailing_flush", &prm->trailing_flush}};
            bool known = true;
            if (k == "prefix") memcpy(prm->umi_prefix, v.data(), v.size() < 32 ? v.size() : 32);
            else if (k == "tick_offset") prm->tick_offset = i;
            else if (k == "score_percent_req") prm->score_percent_req = strtod(v.c_str(), nullptr);
            else if (k == "nt") nt = strtoull(v.c_str(), nullptr, 0);
            else if (k == "len") len = strtoull(v.c_str(), nullptr, 0);
            else if (k == "tsize") tsize = strtoull(v.c_str(), nullptr, 0);
            else if (k == "N") N = i;
            else if (k == "have_tick") have_tick = i != 0;
            else { known = false; for (auto &f : ints) if (k == f.name) { *f.field = (int32_t)i; known = true; } }
            if (!known) { fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
        }
        const std::vector<uint32_t> target_len((size_t)nt, (uint32_t)len);
        DevParams p{}; const char *why = "unset";
        const int rc = make_dev_params(*prm, target_len, have_tick, N, tsize, &p, &why);
        if (rc != GCE_OK) { printf("%s rc=%d\n", label.c_str(), rc); continue; }
        if (p.target_len || p.target_cum || p.ref_data || p.ref_len || p.ref_win || p.n_ref) { fprintf(stderr, "%s: a field of the caller's was written\n", label.c_str()); return 1; }
        printf("%s rc=0 thr=%d/%d/%d/%d/%d q=%d/%d/%d s=%d/%d/%d/%d misc=%d/%d/%d/%d/%g bias=%d max=%d lut=0x%08X thr4=0x%08X/0x%08X/0x%08X swar=%d min_lb=%d vote_ok=%d accept=%d "
               "prefix=%s/%d n_targets=%d key_bt=%d key_bl=%d nw_cb=%d nw_bd=%d nw_ok=%d tick=%" PRId64 "/%" PRId64 "/%d trailing=%d why=%s\n", label.c_str(),
               p.proper_thr, p.unproper_thr, p.duplex_mismatch_thr, p.cluster_size_req, p.base_score_req, p.high_q, p.moderate_q, p.low_q, p.s_high, p.s_moderate, p.s_low, p.s_bad,
               p.skip_low_complexity_thr, p.duplex_only, p.disable_duplex, p.period, p.score_percent_req, p.score_bias, p.score_max, p.q2s_lut, p.thr_low4, p.thr_mod4, p.thr_high4,
               p.q2s_swar_ok, p.s_min_lb, p.vote_ok, p.vote_accept_by_qual, p.prefix, p.prefix_len, p.n_targets, p.key_bt, p.key_bl, p.nw_cb, p.nw_bd, p.nw_ok,
               p.tick_offset, p.tick_epoch0, p.tick_rem0, p.trailing_flush, why ? why : "-");
    }
    return 0;
}
