// bamio_overlap.hpp -- the QUAL bytes of overlapping mates rewritten so that a pileup of the file counts every fragment once:
// gce_bam_merge_overlap (gce_ovlmerge.hpp), over SortJob as gce_bam_calmd is.  A part of bamio.cpp.
#pragma once
#include "bamio_sort.hpp"

extern "C" {

int gce_bam_merge_overlap(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes, int32_t min_mapq,
                          uint32_t exclude_flags, uint32_t options, gce_overlap_run *out, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    if (level < -3 || level > 9) { set_err(err, "level should be -3, -2, -1 or 0..9"); return GCE_ERR_INVALID; }
    if (min_mapq < 0 || min_mapq > 255) { set_err(err, "min_mapq should be 0..255"); return GCE_ERR_INVALID; }
    if (options & ~(uint32_t)GCE_OVERLAP_WEAK_HASH) { set_err(err, "unknown option bit (GCE_OVERLAP_WEAK_HASH is the only one)"); return GCE_ERR_INVALID; }
    const double t_start = now_s();
    SortJob j; j.who = "gce_bam_merge_overlap"; j.keep_header = true;
    auto done = [&](int code) { j.close_all(code); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    out->n_ref = n_ref;
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, device_budget_bytes, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    if ((rc = gce_sort_overlap_begin(j.b)) != GCE_OK) return done(j.fail(rc, "bad argument"));
    // ---- the file from its first byte, window by window: the GPU inflates and indexes them, the records stay resident with their offsets
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est); });
    if (rc != GCE_OK) return done(rc);
    // ---- rules E, P, M and Q over the whole file
    j.set_pieces();
    int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bad = -1; uint64_t total = 0;
    double t0 = now_s();
    if ((rc = gce_sort_overlap_finish(j.b, min_mapq, exclude_flags, options, j.codes, j.piece, counts, &bad, &total)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    out->merge_s = now_s() - t0;
    if (bad >= 0) {
        char m[256]; snprintf(m, sizeof m, "BAM record %lld (counting from 0) names a contig the header does not have", (long long)bad);
        return done(j.fail(GCE_ERR_INVALID, m));
    }
    out->n_records = counts[0]; out->n_pairs = counts[1]; out->n_pairs_no_qual = counts[2]; out->n_ambiguous = counts[3]; out->n_shared_columns = counts[4];
    out->n_disagree_columns = counts[5]; out->n_columns_skipped = counts[6]; out->n_records_changed = counts[7];
    out->inflated_bytes = (int64_t)total;
    // ---- rule F
    t0 = now_s();
    if ((rc = j.begin_output(total)) != GCE_OK || (rc = j.write_range(total)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

}  // extern "C"
