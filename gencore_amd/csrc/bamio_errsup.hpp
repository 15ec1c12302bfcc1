// bamio_errsup.hpp -- the error profile by consensus support, the FR / RR tags: gce_bam_error_profile_support (gce_errsup.hpp).
// A part of bamio.cpp: the pass's own part of reduce_run (bamio_reduce.hpp), which runs it, over bamio_errprof.hpp's ErrPass.
#pragma once
#include "bamio_errprof.hpp"

extern "C" {

void gce_errsup_free(gce_errsup_run *out) {
    if (!out) return;
    free(out->counts);
    out->counts = nullptr;
}

}  // extern "C"

namespace {

constexpr int ERRSUP_ROWS = 3 * GCE_ERRSUP_BUCKETS * GCE_ERRSUP_BUCKETS;

// a tag as the SAM specification spells one: a letter, then a letter or a digit
inline bool errsup_tag_ok(const char *t) {
    auto alpha = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); };
    return alpha(t[0]) && (alpha(t[1]) || (t[1] >= '0' && t[1] <= '9'));
}

struct ErrsupPass : ErrPass<ErrsupPass, gce_errsup_run, gce_errsup> {
    static constexpr const char *who = "gce_bam_error_profile_support", *options_known = "GCE_ERRSUP_DIRECT is the only one";
    static constexpr uint32_t option = GCE_ERRSUP_DIRECT;
    static constexpr auto window = gce_errsup_window; static constexpr auto error = gce_errsup_error;
    static constexpr auto destroy = gce_errsup_destroy; static constexpr auto free_out = gce_errsup_free;
    static constexpr auto set_ref = gce_errsup_set_ref; static constexpr auto set_mask = gce_errsup_set_mask; static constexpr auto set_sites = gce_errsup_set_sites;
    const char *tags = nullptr;
    int create(int32_t device, size_t budget, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_errsup **o) const {
        return gce_errsup_create(device, budget, min_mapq, min_baseq, exclude_flags, options, tags, o);
    }
    bool alloc(const ReduceInput &) {
        out->counts = (uint64_t *)malloc((size_t)ERRSUP_ROWS * GCE_ERRPROF_CLASSES * 8);
        return out->counts != nullptr;
    }
    int finish() {
        int64_t c[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int rc = gce_errsup_finish(p, c, out->counts);
        if (rc != GCE_OK) return rc;
        counters(c, 10); out->n_bad_aux = c[9];
        int64_t masked = 0;
        for (int row = 0; row < ERRSUP_ROWS; row++) {
            const uint64_t *k = out->counts + (size_t)row * GCE_ERRPROF_CLASSES;
            const int f = row / GCE_ERRSUP_BUCKETS % GCE_ERRSUP_BUCKETS, r = row % GCE_ERRSUP_BUCKETS;
            if (f) out->n_with_forward += (int64_t)k[22];
            if (r) out->n_with_reverse += (int64_t)k[22];
            masked += (int64_t)k[21];
        }
        if (mk.on) mk.out->n_masked_events = masked;
        return GCE_OK;
    }
    // rule O: the totals, with or without a file, and one row per (segment, forward, reverse) with a counter
    template <class EMIT> bool table(const ReduceInput &, bool, EMIT &&emit) {
        std::string buf = "#segment\tforward\treverse\trecords\tbases\tmismatches";
        for (const char *r : {"A", "C", "G", "T"}) for (const char *b : {"A", "C", "G", "T"}) { buf += '\t'; buf += r; buf += '>'; buf += b; }
        buf += tail();
        const int n_cls = this->n_cls();
        auto bucket = [](char *w, int b) {
            if (b == 0) { *w++ = '.'; return w; }
            w = pile_num(w, (uint64_t)b);
            if (b == GCE_ERRSUP_BUCKETS - 1) *w++ = '+';
            return w;
        };
        for (int row = 0; row < ERRSUP_ROWS; row++) {
            const uint64_t *k = out->counts + (size_t)row * GCE_ERRPROF_CLASSES;
            bool any = false;
            for (int q = 0; q < 23; q++) any = any || k[q];
            if (!any) continue;
            uint64_t bases = 0, mism = 0;
            for (int q = 0; q < 16; q++) { bases += k[q]; if ((q >> 2) != (q & 3)) mism += k[q]; }
            out->n_bases += (int64_t)bases; out->n_mismatches += (int64_t)mism;
            char line[32 * 21], *w = line;
            w = pile_num(w, (uint64_t)(row / (GCE_ERRSUP_BUCKETS * GCE_ERRSUP_BUCKETS))); *w++ = '\t';
            w = bucket(w, row / GCE_ERRSUP_BUCKETS % GCE_ERRSUP_BUCKETS); *w++ = '\t'; w = bucket(w, row % GCE_ERRSUP_BUCKETS); *w++ = '\t';
            w = pile_num(w, k[22]); *w++ = '\t'; w = pile_num(w, bases); *w++ = '\t'; w = pile_num(w, mism);
            for (int q = 0; q < n_cls; q++) { *w++ = '\t'; w = pile_num(w, k[q]); }
            *w++ = '\n';
            buf.append(line, (size_t)(w - line));
        }
        return emit(buf);
    }
};

}  // namespace

extern "C" {

int gce_bam_error_profile_support(const char *bam_path, const char *fasta_path, const char *bed_path, const char *mask_path, const char *tsv_path, const char *tags, int32_t device, int threads,
                                  int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errsup_run *out,
                                  gce_mask_run *mask, char err[256]) {
    if (tags && (strlen(tags) != 4 || !errsup_tag_ok(tags) || !errsup_tag_ok(tags + 2))) { set_err(err, "tags should be two two-character tags, four characters"); return GCE_ERR_INVALID; }
    ErrsupPass ps{{out}};
    ps.tags = tags;
    if (mask_path) { ps.mk.on = true; ps.mk.path = mask_path; ps.mk.out = mask; }
    return reduce_run(ps, bam_path, bed_path, fasta_path, tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes, device_budget_bytes, err);
}

}  // extern "C"
