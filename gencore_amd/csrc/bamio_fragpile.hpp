// bamio_fragpile.hpp -- gce_bam_pileup's table with every fragment counted once where its mates overlap: gce_bam_pileup_fragments
// (gce_fragpile.hpp).  A part of bamio.cpp: the pass's own part of reduce_run (bamio_reduce.hpp), which runs it; everything but
// the five join counters is bamio_pileup.hpp's PilePass.
#pragma once
#include "bamio_pileup.hpp"

extern "C" {

void gce_fragpile_free(gce_fragpile_run *out) { pile_free(out); }

}  // extern "C"

namespace {

struct FragpilePass : PilePass<FragpilePass, gce_fragpile_run, gce_fragpile> {
    static constexpr const char *who = "gce_bam_pileup_fragments", *options_known = "GCE_FRAGPILE_DIRECT and GCE_FRAGPILE_WEAK_HASH are the only ones";
    static constexpr uint32_t option = GCE_FRAGPILE_DIRECT | GCE_FRAGPILE_WEAK_HASH;
    static constexpr auto create = gce_fragpile_create; static constexpr auto window = gce_fragpile_window; static constexpr auto error = gce_fragpile_error;
    static constexpr auto destroy = gce_fragpile_destroy; static constexpr auto free_out = gce_fragpile_free; static constexpr auto set_sites = gce_fragpile_set_sites;
    int finish() {
        int64_t c[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int rc = gce_fragpile_finish(p, c, out->counts);
        if (rc != GCE_OK) return rc;
        counters(c);
        out->n_pairs = c[8]; out->n_shared_columns = c[9]; out->n_disagree_columns = c[10]; out->n_ambiguous = c[11]; out->n_deferred = c[12];
        return GCE_OK;
    }
};

}  // namespace

extern "C" {

int gce_bam_pileup_fragments(const char *bam_path, const char *bed_path, const char *fasta_path, const char *tsv_path, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq,
                             uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_fragpile_run *out, char err[256]) {
    FragpilePass ps{{out}};
    return reduce_run(ps, bam_path, bed_path, fasta_path, tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes, device_budget_bytes, err);
}

}  // extern "C"
