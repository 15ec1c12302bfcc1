// bamio_calmd.hpp -- NM and MD recomputed against the reference: gce_bam_calmd and gce_bam_calmd_stream (gce_calmd.hpp).  A
// part of bamio.cpp.
#pragma once
#include "bamio_sort.hpp"

namespace {

// what gce_bam_calmd and gce_bam_calmd_stream refuse before a device is touched, beside their NULL arguments
int calmd_check(int level, const char *fasta_path, char err[256]) {
    if (level < -3 || level > 9) { set_err(err, "level should be -3, -2, -1 or 0..9"); return GCE_ERR_INVALID; }
    struct stat sf;
    if (stat(fasta_path, &sf) != 0 || S_ISDIR(sf.st_mode)) { set_err(err, "cannot open the reference FASTA"); return GCE_ERR_INVALID; }
    return GCE_OK;
}
// rule R: the FASTA loaded (*fa: the caller frees it once the bases are on the device) and, per contig of j's header, its bases and their
// length as gce_sort_calmd_ref takes them, matched by name
int calmd_contigs(SortJob &j, const char *fasta_path, gce_fasta **fa, std::vector<const char *> &seq, std::vector<int64_t> &len) {
    const int rc = gce_fasta_load(fasta_path, j.T, fa);
    if (rc != GCE_OK) return j.fail(rc, "cannot read the reference FASTA");
    match_contigs(j.names, *fa, seq, len);
    return GCE_OK;
}

// the streamed runners (gce_bam_calmd_stream, gce_bam_umi_to_mi): the budget when the caller gives none, a fraction of the free device memory
int stream_auto_budget(SortJob &j, int32_t device, uint64_t *budget) {
    size_t fr = 0, tot = 0;
    const int r0 = gce_device_mem_info(device, &fr, &tot);
    if (r0 != GCE_OK) return j.fail(r0, "no HIP device");
    *budget = std::max<uint64_t>((uint64_t)((double)fr * GCE_PASS_BUDGET_FRACTION), 1);
    return GCE_OK;
}
// ... and their flush callback: the first n resident bytes are written as members and let go; s: the seconds flushes took
struct StreamFlush { SortJob *j; double s; };
int stream_flush(void *ctx, uint64_t n) {
    StreamFlush &f = *(StreamFlush *)ctx;
    const double f0 = now_s();
    int r = f.j->host_room(n);
    if (r == GCE_OK) r = f.j->write_range(n);
    if (r == GCE_OK && (r = gce_sort_calmd_consume(f.j->b, n)) != GCE_OK) r = f.j->fail(r, gce_sort_error(f.j->b));
    f.s += now_s() - f0;
    return r;
}

}  // namespace

extern "C" {

int gce_bam_calmd(const char *in_path, const char *out_path, const char *fasta_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes,
                  gce_calmd_run *out, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !fasta_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    { const int rc = calmd_check(level, fasta_path, err); if (rc != GCE_OK) return rc; }
    const double t_start = now_s();
    SortJob j; j.who = "gce_bam_calmd"; j.keep_header = true;
    gce_fasta *fa = nullptr;
    auto done = [&](int code) { j.close_all(code); if (fa) gce_fasta_free(fa); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    out->n_ref = n_ref;
    // ---- rule R: the contigs by the header's names
    double t0 = now_s();
    std::vector<const char *> seq; std::vector<int64_t> len;
    if ((rc = calmd_contigs(j, fasta_path, &fa, seq, len)) != GCE_OK) return done(rc);
    out->read_s += now_s() - t0;
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, device_budget_bytes, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    if ((rc = gce_sort_calmd_ref(j.b, n_ref, seq.data(), len.data())) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    gce_fasta_free(fa); fa = nullptr;
    // ---- the file from its first byte, window by window: the GPU inflates, indexes and rewrites the records behind the resident output
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_calmd_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est,
                                     &out->calmd_s); });
    if (rc != GCE_OK) return done(rc);
    out->inflate_index_s -= out->calmd_s;
    j.set_pieces();
    int64_t counts[6] = {0, 0, 0, 0, 0, 0}; uint64_t in_bytes = 0, total = 0;
    if ((rc = gce_sort_calmd_finish(j.b, j.codes, j.piece, counts, &in_bytes, &total)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    out->n_records = counts[0]; out->n_rewritten = counts[1]; out->n_unchanged = counts[2]; out->n_no_ref = counts[3]; out->n_nm_changed = counts[4]; out->n_md_changed = counts[5];
    out->inflated_bytes = (int64_t)in_bytes; out->out_record_bytes = (int64_t)total;
    // ---- rule F
    t0 = now_s();
    if ((rc = j.begin_output(total)) != GCE_OK || (rc = j.write_range(total)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

// gce_bam_calmd with its output streamed: the temporary output is open from the first window on, and whenever the next window's output would
// take the resident record bytes past the cap R, the whole members of 0xff00 bytes resident so far are written and let go
int gce_bam_calmd_stream(const char *in_path, const char *out_path, const char *fasta_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes,
                         uint64_t resident_bytes, gce_calmd_run *out, gce_calmd_stream_run *run, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !fasta_path || !out || !run) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out); memset(run, 0, sizeof *run);
    { const int rc = calmd_check(level, fasta_path, err); if (rc != GCE_OK) return rc; }
    const double t_start = now_s();
    SortJob j; j.who = "gce_bam_calmd_stream"; j.keep_header = true;
    gce_fasta *fa = nullptr;
    auto done = [&](int code) { j.close_all(code); if (fa) gce_fasta_free(fa); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    out->n_ref = n_ref;
    uint64_t budget = device_budget_bytes;
    if (!budget) { const int r0 = stream_auto_budget(j, device, &budget); if (r0 != GCE_OK) return done(r0); }
    // ---- rule R: the contigs by the header's names
    double t0 = now_s();
    std::vector<const char *> seq; std::vector<int64_t> len;
    if ((rc = calmd_contigs(j, fasta_path, &fa, seq, len)) != GCE_OK) return done(rc);
    out->read_s += now_s() - t0;
    const uint64_t M = PassWriter::BS;
    j.set_pieces();
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, (size_t)budget, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    if ((rc = gce_sort_calmd_stream_begin(j.b, j.codes, j.piece, (resident_bytes + M - 1) / M * M)) != GCE_OK) return done(j.fail(rc, "bad argument"));
    if ((rc = gce_sort_calmd_ref(j.b, n_ref, seq.data(), len.data())) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    gce_fasta_free(fa); fa = nullptr;
    // ---- rule F from the first window on: the header's members now, the record stream's as they are flushed
    if ((rc = j.begin_output(0)) != GCE_OK) return done(rc);
    StreamFlush fl = {&j, 0};
    auto flush = stream_flush;
    // ---- the file from its first byte, window by window: the GPU inflates, indexes and rewrites the records behind the resident output
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_calmd_stream_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est,
                                            &out->calmd_s, flush, &fl); });
    if (rc != GCE_OK) return done(rc);
    out->inflate_index_s -= out->calmd_s + fl.s;
    { uint64_t cap = 0, flushed = 0; (void)gce_sort_calmd_stream_stats(j.b, &run->n_flushes, &cap, &flushed); run->resident_cap_bytes = (int64_t)cap; run->flushed_bytes = (int64_t)flushed; }
    int64_t counts[6] = {0, 0, 0, 0, 0, 0}; uint64_t in_bytes = 0, rest = 0;
    if ((rc = gce_sort_calmd_finish(j.b, j.codes, j.piece, counts, &in_bytes, &rest)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    out->n_records = counts[0]; out->n_rewritten = counts[1]; out->n_unchanged = counts[2]; out->n_no_ref = counts[3]; out->n_nm_changed = counts[4]; out->n_md_changed = counts[5];
    out->inflated_bytes = (int64_t)in_bytes; out->out_record_bytes = (int64_t)((uint64_t)run->flushed_bytes + rest);
    // ---- the rest with the last short member, the EOF marker, the rename
    t0 = now_s();
    if ((rc = j.host_room(rest)) != GCE_OK || (rc = j.write_range(rest)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = fl.s + (now_s() - t0);
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

}  // extern "C"
