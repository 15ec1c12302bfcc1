// bamio_umi.hpp -- the UMI of every record, from a tag such as RX or from an Illumina read name, into the MI:Z field the run reads:
// gce_bam_umi_to_mi (gce_umi.hpp).  A part of bamio.cpp.
#pragma once
#include "bamio_calmd.hpp"

namespace {

// `name`, or a two-character tag [A-Za-z][A-Za-z0-9] other than MI
int umi_source_check(const char *source, char err[256]) {
    if (strcmp(source, "name") == 0) return GCE_OK;
    const unsigned char a = (unsigned char)source[0], z = a ? (unsigned char)source[1] : 0;
    if (!isalpha(a) || !isalnum(z) || source[2]) { set_err(err, "source should be a two-character tag such as RX, or name"); return GCE_ERR_INVALID; }
    if (a == 'M' && z == 'I') { set_err(err, "source MI is what the run reads without this pass"); return GCE_ERR_INVALID; }
    return GCE_OK;
}

}  // namespace

extern "C" {

// the streamed runner of gce_bam_calmd_stream under the UMI rewriter: no reference, the same windows, cap, flushes and output
int gce_bam_umi_to_mi(const char *in_path, const char *out_path, const char *source, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes,
                      uint64_t resident_bytes, gce_umi_run *out, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !source || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    if (level < -3 || level > 9) { set_err(err, "level should be -3, -2, -1 or 0..9"); return GCE_ERR_INVALID; }
    { const int rc = umi_source_check(source, err); if (rc != GCE_OK) return rc; }
    const double t_start = now_s();
    SortJob j; j.who = "gce_bam_umi_to_mi"; j.keep_header = true;
    auto done = [&](int code) { j.close_all(code); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    uint64_t budget = device_budget_bytes;
    if (!budget) { const int r0 = stream_auto_budget(j, device, &budget); if (r0 != GCE_OK) return done(r0); }
    const uint64_t M = PassWriter::BS;
    j.set_pieces();
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, (size_t)budget, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    if ((rc = gce_sort_umi_begin(j.b, j.codes, j.piece, (resident_bytes + M - 1) / M * M, source)) != GCE_OK) return done(j.fail(rc, "bad argument"));
    // ---- rule F from the first window on: the header's members now, the record stream's as they are flushed
    if ((rc = j.begin_output(0)) != GCE_OK) return done(rc);
    StreamFlush fl = {&j, 0};
    auto flush = stream_flush;
    // ---- the file from its first byte, window by window: the GPU inflates, indexes and rewrites the records behind the resident output
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_umi_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est,
                                   &out->umi_s, flush, &fl); });
    if (rc != GCE_OK) return done(rc);
    out->inflate_index_s -= out->umi_s + fl.s;
    uint64_t cap = 0, flushed = 0; int32_t n_flushes = 0;
    (void)gce_sort_calmd_stream_stats(j.b, &n_flushes, &cap, &flushed);
    out->n_flushes = n_flushes;
    int64_t counts[5] = {0, 0, 0, 0, 0}; uint64_t in_bytes = 0, rest = 0;
    if ((rc = gce_sort_umi_finish(j.b, j.codes, j.piece, counts, &in_bytes, &rest)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    out->n_records = counts[0]; out->n_tagged = counts[1]; out->n_no_source = counts[2]; out->n_not_umi = counts[3]; out->n_mi_dropped = counts[4];
    out->inflated_bytes = (int64_t)in_bytes; out->out_record_bytes = (int64_t)(flushed + rest);
    // ---- the rest with the last short member, the EOF marker, the rename
    const double t0 = now_s();
    if ((rc = j.host_room(rest)) != GCE_OK || (rc = j.write_range(rest)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = fl.s + (now_s() - t0);
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

}  // extern "C"
