// bamio_fragerr.hpp -- gce_bam_error_profile's table with every fragment counted once where its mates overlap, and the overlap table:
// gce_bam_error_profile_fragments (gce_fragerr.hpp).  A part of bamio.cpp: the pass's own part of reduce_run
// (bamio_reduce.hpp), which runs it and writes the primary table; the rows of both tables and the runner's base (ErrPass) are
// bamio_errprof.hpp's.
#pragma once
#include "bamio_errprof.hpp"

extern "C" {

void gce_fragerr_free(gce_fragerr_run *out) {
    if (!out) return;
    free(out->counts); free(out->overlap);
    out->counts = out->overlap = nullptr;
}

}  // extern "C"

namespace {

struct FragerrPass : ErrPass<FragerrPass, gce_fragerr_run, gce_fragerr> {
    static constexpr const char *who = "gce_bam_error_profile_fragments", *options_known = "GCE_FRAGERR_DIRECT and GCE_FRAGERR_WEAK_HASH are the only ones";
    static constexpr uint32_t option = GCE_FRAGERR_DIRECT | GCE_FRAGERR_WEAK_HASH;
    static constexpr auto create = gce_fragerr_create; static constexpr auto window = gce_fragerr_window; static constexpr auto error = gce_fragerr_error;
    static constexpr auto destroy = gce_fragerr_destroy; static constexpr auto free_out = gce_fragerr_free;
    static constexpr auto set_ref = gce_fragerr_set_ref; static constexpr auto set_mask = gce_fragerr_set_mask; static constexpr auto set_sites = gce_fragerr_set_sites;
    std::string ovl_tmp;                                                              // the overlap table's temporary name, empty for no file
    bool alloc(const ReduceInput &) {
        const size_t bytes = (size_t)3 * GCE_ERRPROF_MAX_CYCLE * GCE_ERRPROF_CLASSES * 8;
        out->counts = (uint64_t *)malloc(bytes); out->overlap = (uint64_t *)malloc(bytes);
        return out->counts != nullptr && out->overlap != nullptr;
    }
    int finish() {
        int64_t c[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int rc = gce_fragerr_finish(p, c, out->counts, out->overlap);
        if (rc != GCE_OK) return rc;
        counters(c, 9);
        out->n_pairs = c[10]; out->n_shared_columns = c[11]; out->n_disagree_columns = c[12]; out->n_ambiguous = c[13]; out->n_deferred = c[14];
        if (mk.on) mk.out->n_masked_events = MaskJob::events(out->counts);
        return GCE_OK;
    }
    // rule O for the primary table through the frame; the overlap table to its temporary name, which the entry point renames
    template <class EMIT> bool table(const ReduceInput &, bool, EMIT &&emit) {
        std::string buf;
        errprof_table(out->counts, "bases", "mismatches", tail(), 16, out->n_bases, out->n_mismatches, buf, n_cls());
        if (!emit(buf)) return false;
        if (ovl_tmp.empty()) return true;
        int64_t shared = 0, errors = 0;
        buf.clear();
        errprof_table(out->overlap, "shared", "errors", tail(true), 19, shared, errors, buf, n_cls());
        FILE *fo = fopen(ovl_tmp.c_str(), "wb");
        if (!fo) return false;
        const bool wrote = fwrite(buf.data(), 1, buf.size(), fo) == buf.size();
        return (fclose(fo) == 0) && wrote;
    }
};

}  // namespace

namespace {

// both entry points: mask NULL for the one without a mask
int fragerr_run(const char *bam_path, const char *fasta_path, const char *bed_path, bool masked, const char *mask_path, const char *tsv_path, const char *overlap_tsv_path, int32_t device,
                int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_fragerr_run *out,
                gce_mask_run *mask, char err[256]) {
    FragerrPass ps{{out}, overlap_tsv_path ? std::string(overlap_tsv_path) + ".tmp" + std::to_string((long long)getpid()) : std::string()};
    ps.mk.on = masked; ps.mk.path = mask_path; ps.mk.out = mask;
    int rc = reduce_run(ps, bam_path, bed_path, fasta_path, tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes, device_budget_bytes, err);
    if (!overlap_tsv_path) return rc;
    if (rc == GCE_OK && rename(ps.ovl_tmp.c_str(), overlap_tsv_path) != 0) {
        if (tsv_path) unlink(tsv_path);
        gce_fragerr_free(out);
        set_err(err, "cannot write the overlap table");
        rc = GCE_ERR_INVALID;
    }
    if (rc != GCE_OK) unlink(ps.ovl_tmp.c_str());
    return rc;
}

}  // namespace

extern "C" {

int gce_bam_error_profile_fragments(const char *bam_path, const char *fasta_path, const char *bed_path, const char *tsv_path, const char *overlap_tsv_path, int32_t device, int threads,
                                    int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_fragerr_run *out,
                                    char err[256]) {
    return fragerr_run(bam_path, fasta_path, bed_path, false, nullptr, tsv_path, overlap_tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes,
                       device_budget_bytes, out, nullptr, err);
}

int gce_bam_error_profile_fragments_masked(const char *bam_path, const char *fasta_path, const char *bed_path, const char *mask_path, const char *tsv_path, const char *overlap_tsv_path,
                                           int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes,
                                           size_t device_budget_bytes, gce_fragerr_run *out, gce_mask_run *mask, char err[256]) {
    return fragerr_run(bam_path, fasta_path, bed_path, true, mask_path, tsv_path, overlap_tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes,
                       device_budget_bytes, out, mask, err);
}

}  // extern "C"
