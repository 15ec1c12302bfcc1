// bamio_errqual.hpp -- the error profile by reported base quality: gce_bam_error_profile_quality (gce_errqual.hpp).
// A part of bamio.cpp: the pass's own part of reduce_run (bamio_reduce.hpp), which runs it, over bamio_errprof.hpp's ErrPass.
#pragma once
#include "bamio_errprof.hpp"

extern "C" {

void gce_errqual_free(gce_errqual_run *out) {
    if (!out) return;
    free(out->counts);
    out->counts = nullptr;
}

}  // extern "C"

namespace {

constexpr int ERRQUAL_ROWS = 3 * GCE_ERRQUAL_BUCKETS;

struct ErrqualPass : ErrPass<ErrqualPass, gce_errqual_run, gce_errqual> {
    static constexpr const char *who = "gce_bam_error_profile_quality", *options_known = "GCE_ERRQUAL_DIRECT is the only one";
    static constexpr uint32_t option = GCE_ERRQUAL_DIRECT;
    static constexpr auto create = gce_errqual_create; static constexpr auto window = gce_errqual_window; static constexpr auto error = gce_errqual_error;
    static constexpr auto destroy = gce_errqual_destroy; static constexpr auto free_out = gce_errqual_free;
    static constexpr auto set_ref = gce_errqual_set_ref; static constexpr auto set_mask = gce_errqual_set_mask; static constexpr auto set_sites = gce_errqual_set_sites;
    bool alloc(const ReduceInput &) {
        out->counts = (uint64_t *)malloc((size_t)ERRQUAL_ROWS * GCE_ERRPROF_CLASSES * 8);
        return out->counts != nullptr;
    }
    int finish() {
        int64_t c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int rc = gce_errqual_finish(p, c, out->counts);
        if (rc != GCE_OK) return rc;
        counters(c, 9);
        if (mk.on) {
            int64_t masked = 0;
            for (int row = 0; row < ERRQUAL_ROWS; row++) masked += (int64_t)out->counts[(size_t)row * GCE_ERRPROF_CLASSES + 21];
            mk.out->n_masked_events = masked;
        }
        return GCE_OK;
    }
    // rule O: the totals, with or without a file, and one row per (segment, quality) with a counter
    template <class EMIT> bool table(const ReduceInput &, bool, EMIT &&emit) {
        std::string buf = "#segment\tquality\tbases\tmismatches";
        for (const char *r : {"A", "C", "G", "T"}) for (const char *b : {"A", "C", "G", "T"}) { buf += '\t'; buf += r; buf += '>'; buf += b; }
        buf += tail();
        const int n_cls = this->n_cls();
        for (int row = 0; row < ERRQUAL_ROWS; row++) {
            const uint64_t *k = out->counts + (size_t)row * GCE_ERRPROF_CLASSES;
            bool any = false;
            for (int q = 0; q < 22; q++) any = any || k[q];
            if (!any) continue;
            uint64_t bases = 0, mism = 0;
            for (int q = 0; q < 16; q++) { bases += k[q]; if ((q >> 2) != (q & 3)) mism += k[q]; }
            out->n_bases += (int64_t)bases; out->n_mismatches += (int64_t)mism;
            const int b = row % GCE_ERRQUAL_BUCKETS;
            char line[32 * 21], *w = line;
            w = pile_num(w, (uint64_t)(row / GCE_ERRQUAL_BUCKETS)); *w++ = '\t';
            if (b == GCE_ERRQUAL_BUCKETS - 1) *w++ = '.';
            else { w = pile_num(w, (uint64_t)b); if (b == GCE_ERRQUAL_BUCKETS - 2) *w++ = '+'; }
            *w++ = '\t'; w = pile_num(w, bases); *w++ = '\t'; w = pile_num(w, mism);
            for (int q = 0; q < n_cls; q++) { *w++ = '\t'; w = pile_num(w, k[q]); }
            *w++ = '\n';
            buf.append(line, (size_t)(w - line));
        }
        return emit(buf);
    }
};

}  // namespace

extern "C" {

int gce_bam_error_profile_quality(const char *bam_path, const char *fasta_path, const char *bed_path, const char *mask_path, const char *tsv_path, int32_t device, int threads,
                                  int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errqual_run *out,
                                  gce_mask_run *mask, char err[256]) {
    ErrqualPass ps{{out}};
    if (mask_path) { ps.mk.on = true; ps.mk.path = mask_path; ps.mk.out = mask; }
    return reduce_run(ps, bam_path, bed_path, fasta_path, tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes, device_budget_bytes, err);
}

}  // extern "C"
