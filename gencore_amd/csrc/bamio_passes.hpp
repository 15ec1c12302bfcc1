// bamio_passes.hpp -- one file in key-range passes on one device: gce_run_bam_passes (gce_passes.hpp).  A part of bamio.cpp.
#pragma once
#include "gce_entry.h"
#include "bamio_reader.hpp"
#include "bamio_writer.hpp"

extern "C" {

int gce_run_bam_passes(const char *in_path, const char *out_path, const char *fasta_path, const char *bed_path, int32_t coverage_step, const gce_params *params,
                       int32_t device, int threads, int level, size_t device_budget_bytes, int32_t min_passes, size_t window_bytes,
                       gce_bam_run *out, gce_depth_run *depth, gce_pass_run *run, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !params || !out || !depth || !run || min_passes < 0 || min_passes > 64 || coverage_step <= 0) return GCE_ERR_INVALID;
    memset(out, 0, sizeof *out); memset(run, 0, sizeof *run); memset(depth, 0, sizeof *depth);
    const double t_start = now_s();
    out->rss_start_kb = status_kb("VmRSS:");
    (void)gce_device_bytes(nullptr, nullptr, 1);
    auto peak_now = [&] { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); return pk; };
    const bool auto_budget = device_budget_bytes == 0;
    uint64_t budget = device_budget_bytes;
    if (auto_budget) {
        size_t fr = 0, tot = 0;
        const int r0 = gce_device_mem_info(device, &fr, &tot);
        if (r0 != GCE_OK) { set_err(err, "no device"); return r0; }
        budget = (uint64_t)((double)fr * GCE_PASS_BUDGET_FRACTION);
    }
    run->budget_bytes = (int64_t)budget;
    InputFile in;
    if (const char *verb = in.open(in_path)) { set_err(err, (std::string("cannot ") + verb + " the input BAM").c_str()); return GCE_ERR_INVALID; }
    const uint64_t fsz = in.fsz;
    const bool is_sam = in.is_sam();
    // today's single-pass path (gce_run_bam_depth), unchanged, whenever the auto budget is in force and no passes are forced: at once when even a
    // generous bound fits (measured, DESIGN.md 4b: peak ~6.2 x inflated bytes, inflated ~4.3 - 4.7 x the file; the bound takes 6.5 x 6), otherwise
    // after the key pass when the plan needs one pass.  SAM text is never processed in passes; with the auto budget it always runs as today.
    const bool single_ok = auto_budget && min_passes <= 1;
    const uint64_t est = fsz * 39 + ((uint64_t)2 << 30);
    auto single = [&]() -> int {
        gce_params pr1 = *params; pr1.device = device;
        const int r1 = gce_run_bam_depth(in_path, out_path, fasta_path, bed_path, coverage_step, &pr1, 1, &device, 0, threads, level, out, depth, err);
        run->n_passes = 1; run->single_pass = 1; run->reads_per_pass[0] = out->n_reads; run->peak_device_bytes = peak_now(); run->pass_s[0] = out->total_s;
        return r1;
    };
    if (is_sam) {
        in.close();
        if (min_passes > 1) { set_err(err, "SAM text input is not processed in passes"); return GCE_ERR_INVALID; }
        if (!auto_budget && est > budget) {
            char m[256]; snprintf(m, sizeof m, "SAM text input of %llu bytes needs an estimated %llu device bytes, the budget is %llu: SAM input is not processed in passes (convert it to BAM)",
                                  (unsigned long long)fsz, (unsigned long long)est, (unsigned long long)budget);
            set_err(err, m); return GCE_ERR_OOM;
        }
        return single();
    }
    if (single_ok && est <= budget) { in.close(); return single(); }
    const int T = threads > 0 ? threads : default_threads();
    gce_engine *e = nullptr; gce_fasta *fa = nullptr; gce_passes *p = nullptr;
    auto done = [&](int code, const char *m) { set_err(err, m); if (p) gce_passes_destroy(p); if (e) gce_destroy(e); if (fa) gce_fasta_free(fa); in.close(); if (code != GCE_OK) gce_depth_run_free(depth); return code; };
    // 64 MB of compressed bytes per window by default: the GPU inflate runs one lane per BGZF member and wants thousands of members per launch
    // (8 MB windows, ~400 members each, made a cfg3 4 M pass 2.6 s instead of ~1 s)
    PassReader rd; rd.fd = in.fd; rd.fsz = fsz; rd.T = T; rd.piece = window_bytes > 0 ? window_bytes : ((size_t)64 << 20);
    // ---- the header (the first window(s)) and, for the "auto" UMI prefix, the first record's name (src/gencore.cpp:207-220)
    gce_params prm = *params; prm.device = device;
    std::vector<std::string> names; std::vector<uint32_t> lens; BamHeader bh;
    switch (read_bam_header(rd, Contigs::Collect, umi_auto(prm), bh, &names, &lens)) {
    case HeaderRead::Failed: return done(GCE_ERR_INVALID, rd.msg.c_str());
    case HeaderRead::NotBam: return done(GCE_ERR_INVALID, "not a BAM stream");
    case HeaderRead::Ended: return done(GCE_ERR_INVALID, "truncated header");
    case HeaderRead::Empty: return done(GCE_ERR_INVALID, "empty file");
    case HeaderRead::Complete: break;
    }
    if (lens.empty()) return done(GCE_ERR_INVALID, "this SAM file has no header");
    const uint64_t hdr_end = bh.hdr_end;
    const std::string text((const char *)rd.win.p + bh.text_off, bh.l_text);
    const std::vector<uint8_t> hdr_raw(rd.win.p, rd.win.p + hdr_end);
    // ---- engine and reference
    file_params(prm, (int32_t)lens.size(), lens.data(), first_name_there(rd, hdr_end) ? (const char *)rd.win.p + hdr_end + 36 : nullptr);
    int rc;
    if ((rc = gce_create(&prm, &e)) != GCE_OK) return done(rc, gce_status_message(rc));
    if (fasta_path && *fasta_path) {
        if ((rc = gce_fasta_load(fasta_path, threads, &fa)) != GCE_OK) return done(rc, "cannot read the FASTA file");
        if ((rc = set_reference(e, fa, names.data(), lens.size())) != GCE_OK) return done(rc, gce_last_error(e));
        gce_fasta_free(fa); fa = nullptr;
    }
    if ((rc = gce_passes_create(device, prm.max_contig, prm.flush_period, &p)) != GCE_OK) return done(rc, "pass state");
    // ---- depth statistics (as gce_run_bam_depth)
    if (bed_path && *bed_path) {
        std::vector<const char *> np; for (auto &x : names) np.push_back(x.c_str());
        if ((rc = gce_bed_load(bed_path, (int32_t)np.size(), np.data(), &depth->n_regions, &depth->region_tid, &depth->region_start, &depth->region_end, nullptr)) != GCE_OK) return done(rc, "cannot read the BED file");
    }
    if (!depth_alloc(depth, lens, coverage_step)) return done(GCE_ERR_OOM, "out of host memory");
    // the file from its first byte, piece by piece: its BGZF members go to the GPU (gce_passes_window inflates and indexes them there; the
    // header's bytes are passed over); e == NULL: the key pass
    auto stream = [&](gce_engine *x) -> int {
        rd.reset();
        uint64_t skip = hdr_end;
        for (;;) {
            const int g = rd.members_next();
            if (g < 0) { set_err(err, rd.msg.c_str()); return GCE_ERR_INVALID; }
            if (g == 0) return GCE_OK;
            const uint64_t sk = std::min<uint64_t>(skip, rd.member_arrays());
            int32_t cut = 0;
            const int r2 = gce_passes_window(p, x, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, prm.n_targets,
                                             rd.last_piece() ? 1 : 0, &cut);
            if (r2 != GCE_OK) { set_err(err, gce_passes_error(p)); return r2; }
            skip -= sk;
            if (cut || rd.last_piece()) return GCE_OK;
        }
    };
    out->open_s = now_s() - t_start;
    // ---- key pass
    double t0 = now_s();
    rc = stream(nullptr);
    std::string kmsg;                                                                // (the key pass failed: why)
    if (rc != GCE_OK) {
        kmsg = err ? err : "";
        if (rc == GCE_ERR_OOM) { char mm[200]; snprintf(mm, sizeof mm, "the key pass needs more device memory than the budget of %llu bytes", (unsigned long long)budget); kmsg = mm; }
    } else if ((uint64_t)peak_now() > budget) {
        char m[200]; snprintf(m, sizeof m, "the key pass needs %lld device bytes, the budget is %llu", (long long)peak_now(), (unsigned long long)budget); kmsg = m; rc = GCE_ERR_OOM;
    }
    int32_t P = 1; uint64_t total_w = 0, room = 0, fixed = 0;
    // beside the weights: the engine's working set that does not scale with a pass's reads (measured: a pass of 43 MB of weight on cfg3 peaked
    // 82 MB above the fixed part), hipCUB temporaries, the GPU encoder's 16 MB pieces
    const uint64_t reserve = ((uint64_t)96 << 20) + (level == -2 || level == -3 ? ((uint64_t)64 << 20) : 0);
    if (rc == GCE_OK && (rc = gce_passes_plan(p, std::max(min_passes, 1), budget, reserve, &P, &total_w, &room, &fixed)) != GCE_OK) kmsg = gce_passes_error(p);
    if (rc != GCE_OK && single_ok) {                                                 // nothing written yet: the file goes the way it goes today
        gce_passes_destroy(p); p = nullptr; gce_destroy(e); e = nullptr; in.close();
        gce_depth_run_free(depth);
        return single();
    }
    if (rc != GCE_OK) return done(rc, kmsg.c_str());
    run->n_passes = P; run->key_pass_s = now_s() - t0; run->fixed_bytes = (int64_t)fixed; run->pass_room = (int64_t)room; run->total_weight = (int64_t)total_w;
    if (single_ok && P == 1) {                                                       // the plan fits one pass: today's path (the key pass only measured)
        const double kp = run->key_pass_s;
        gce_passes_destroy(p); p = nullptr; gce_destroy(e); e = nullptr; in.close();
        gce_depth_run_free(depth);
        const int r1 = single();
        run->key_pass_s = kp; run->fixed_bytes = (int64_t)fixed; run->pass_room = (int64_t)room; run->total_weight = (int64_t)total_w;
        return r1;
    }
    // ---- the passes
    PassWriter wr; wr.level = level; wr.T = T; wr.device = device;
    if (!wr.open(out_path, text, names, lens, bam_header_bytes(text, names, lens))) return done(GCE_ERR_INVALID, "cannot open the output file");
    std::vector<PassKey> hk, pk, nk; std::vector<uint8_t> hb, pb, nb2, emit;
    std::vector<int64_t> pay_sum;
    int64_t *acc_pre = (int64_t *)&out->pre, *acc_post = (int64_t *)&out->post;
    for (int32_t k = 0; k < P; k++) {
        const double tp = now_s();
        uint64_t wk = 0;                                                             // the pass's weight: A x its record bytes + B per read -> room for its records
        if ((rc = gce_passes_info(p, k, &wk, nullptr, nullptr, nullptr, nullptr)) != GCE_OK) return done(rc, "pass weight");
        if ((rc = gce_raw_begin(e, (size_t)(wk / GCE_PASS_WEIGHT_A) + hdr_raw.size())) != GCE_OK) return done(rc, gce_last_error(e));
        int32_t tk;
        if ((rc = gce_raw_push(e, hdr_raw.data(), hdr_raw.size(), &tk)) != GCE_OK || (rc = gce_submit_wait(e, tk)) != GCE_OK) return done(rc, gce_last_error(e));
        if ((rc = gce_passes_begin(p, e, k)) != GCE_OK) return done(rc, gce_passes_error(p));
        rc = stream(e);
        if (rc != GCE_OK) { const std::string m = err ? err : ""; return done(rc, m.c_str()); }
        int64_t n_rec = 0; int32_t wt = INT32_MAX, wp = INT32_MAX;
        if ((rc = gce_passes_end(p, e, hdr_end, prm.n_targets, &n_rec, &wt, &wp)) != GCE_OK) return done(rc, gce_passes_error(p));
        run->reads_per_pass[k] = n_rec;
        pk.clear(); pb.clear();
        if (n_rec > 0) {
            gce_result res; uint64_t body = 0; int64_t n_out = 0;
            if ((rc = gce_process(e)) != GCE_OK) return done(rc, gce_last_error(e)[0] ? gce_last_error(e) : gce_status_message(rc));
            gce_timing tm; if (gce_get_timing(e, &tm) == GCE_OK) out->kernel_ms += tm.total_ms;
            if ((rc = gce_result_device(e, &res)) != GCE_OK) return done(rc, gce_last_error(e));
            out->n_reads += res.n_reads; out->n_out += res.n_out;
            for (int w = 0; w < GCE_STATS_WORDS; w++) { acc_pre[w] += ((const int64_t *)&res.pre)[w]; acc_post[w] += ((const int64_t *)&res.post)[w]; }
            if ((rc = gce_raw_build_output(e, &body, &n_out)) != GCE_OK) return done(rc, gce_last_error(e));
            const int64_t *pay = nullptr; gce_payload_layout lay;
            if ((rc = gce_stats_payload_device(e, coverage_step, depth->n_regions, depth->region_tid, depth->region_start, depth->region_end, &pay, &lay)) != GCE_OK) return done(rc, gce_last_error(e));
            std::vector<int64_t> host((size_t)lay.total_words);
            if ((rc = gce_stats_payload_read(e, pay, lay.total_words, host.data())) != GCE_OK) return done(rc, gce_last_error(e));
            if (pay_sum.empty()) pay_sum.assign(host.size(), 0);
            if (pay_sum.size() != host.size()) return done(GCE_ERR_INVALID, "payload layout");
            for (size_t w = 0; w < host.size(); w++) pay_sum[w] += host[w];
            pk.resize((size_t)n_out); pb.resize((size_t)body);
            if ((rc = gce_passes_output(p, e, pk.data(), pb.data())) != GCE_OK) return done(rc, gce_passes_error(p));
        }
        if ((rc = gce_passes_release(p, e)) != GCE_OK) return done(rc, "release");
        // ---- merge: the held records and this pass's (both in bamComp order); below the watermark they are final
        const bool last = k == P - 1;
        auto below = [&](const PassKey &x) { return last || x.tid < wt || (x.tid == wt && x.pos < wp); };
        nk.clear(); nb2.clear(); emit.clear();
        size_t a = 0, b = 0, ao = 0, bo = 0;
        while (a < hk.size() || b < pk.size()) {
            const bool take_a = b >= pk.size() || (a < hk.size() && pass_less(hk[a], pk[b]));
            const PassKey &x = take_a ? hk[a] : pk[b];
            const uint8_t *src = take_a ? hb.data() + ao : pb.data() + bo;
            if (below(x)) emit.insert(emit.end(), src, src + x.size); else { nk.push_back(x); nb2.insert(nb2.end(), src, src + x.size); }
            if (take_a) { ao += x.size; a++; } else { bo += x.size; b++; }
        }
        if (ao != hb.size() || bo != pb.size()) return done(GCE_ERR_INVALID, "merge: record sizes do not add up");
        if (!emit.empty() && !wr.records(emit.data(), emit.size())) return done(GCE_ERR_INVALID, "cannot write the output file");
        hk.swap(nk); hb.swap(nb2);
        run->held_max = std::max<int64_t>(run->held_max, (int64_t)hk.size());
        run->pass_s[k] = now_s() - tp;
    }
    if (!wr.close()) return done(GCE_ERR_INVALID, "cannot write the output file");
    if (!pay_sum.empty()) depth_unpack(depth, pay_sum.data(), 2 * GCE_STATS_WORDS);
    run->peak_device_bytes = peak_now();
    out->total_s = now_s() - t_start;
    out->peak_rss_kb = status_kb("VmHWM:"); out->rss_end_kb = status_kb("VmRSS:");
    return done(GCE_OK, "");
}

}  // extern "C"
