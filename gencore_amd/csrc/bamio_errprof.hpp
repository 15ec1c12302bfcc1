// bamio_errprof.hpp -- mismatches by read cycle against the reference: gce_bam_error_profile (gce_errprof.hpp).  A part of
// bamio.cpp: the pass's own part of reduce_run (bamio_reduce.hpp), which runs it, and ErrPass, what this runner, bamio_fragerr.hpp's and
// bamio_errsup.hpp's do alike.
#pragma once
#include "bamio_reduce.hpp"

extern "C" {

void gce_errprof_free(gce_errprof_run *out) {
    if (!out) return;
    free(out->counts);
    out->counts = nullptr;
}

}  // extern "C"

namespace {

// rule O's table of one block of counters: the header line (its third and fourth column and the five behind the sixteen are the caller's),
// then per segment one row per cycle up to the last with a counter: segment, cycle, the sum of the classes below n_sum, the off-diagonal
// ones of the sixteen, the 21 counters.  total, offdiag: those two sums over the table, added to
// n_cls: 21, or 22 with a variant mask, whose MASKED column the caller's tail names
inline void errprof_table(const uint64_t *counts, const char *col3, const char *col4, const char *tail, int n_sum, int64_t &total, int64_t &offdiag, std::string &buf, int n_cls = 21) {
    buf += "#segment\tcycle\t"; buf += col3; buf += '\t'; buf += col4;
    for (const char *r : {"A", "C", "G", "T"}) for (const char *b : {"A", "C", "G", "T"}) { buf += '\t'; buf += r; buf += '>'; buf += b; }
    buf += tail;
    for (int g = 0; g < 3; g++) {
        const uint64_t *seg = counts + (size_t)g * GCE_ERRPROF_MAX_CYCLE * GCE_ERRPROF_CLASSES;
        int last = 0;                                                                 // the last cycle with a counter
        for (int cy = 1; cy <= GCE_ERRPROF_MAX_CYCLE; cy++) for (int k = 0; k < n_cls; k++) if (seg[(size_t)(cy - 1) * GCE_ERRPROF_CLASSES + k]) last = cy;
        for (int cy = 1; cy <= last; cy++) {
            const uint64_t *k = seg + (size_t)(cy - 1) * GCE_ERRPROF_CLASSES;
            uint64_t bases = 0, mism = 0;
            for (int q = 0; q < n_sum; q++) { bases += k[q]; if (q < 16 && (q >> 2) != (q & 3)) mism += k[q]; }
            total += (int64_t)bases; offdiag += (int64_t)mism;
            char line[27 * 21], *w = line;
            w = pile_num(w, (uint64_t)g); *w++ = '\t'; w = pile_num(w, (uint64_t)cy); *w++ = '\t'; w = pile_num(w, bases); *w++ = '\t'; w = pile_num(w, mism);
            for (int q = 0; q < n_cls; q++) { *w++ = '\t'; w = pile_num(w, k[q]); }
            *w++ = '\n';
            buf.append(line, (size_t)(w - line));
        }
    }
}

// What the error-profile passes do alike around their device objects: ErrprofPass, FragerrPass (bamio_fragerr.hpp), ErrsupPass
// (bamio_errsup.hpp) and ErrqualPass (bamio_errqual.hpp) derive from it and name their set_ref / set_mask / set_sites beside create / window / ... (bamio_reduce.hpp)
template <class PASS, class RUN, class OBJ> struct ErrPass {
    static constexpr bool bed_first = false;
    RUN *out; MaskJob mk{}; OBJ *p = nullptr;
    void zero() { memset(out, 0, sizeof *out); out->n_intervals = -1; }
    void sites(const ReduceInput &in) { out->n_intervals = (int64_t)in.ps.tid.size(); }
    // the reference bases go to the device and the host's copy is let go; then the mask and rule B's intervals
    int set(ReduceInput &in) {
        int rc = PASS::set_ref(p, in.n_ref, in.seq.data(), in.slen.data());
        if (rc != GCE_OK) return rc;
        gce_fasta_free(in.fa); in.fa = nullptr;
        if (mk.on && (rc = mk.fill([&](int64_t n, const int32_t *t, const int32_t *a, const int32_t *z) { return PASS::set_mask(p, n, t, a, z); })) != GCE_OK) return rc;
        return PASS::set_sites(p, in.has_bed ? (int64_t)in.ps.tid.size() : -1, in.ps.tid.data(), in.ps.start.data(), in.ps.end.data());
    }
    double *pass_s() { return &out->errprof_s; }
    // c[0] records, c[1..8] rule E's skips in its order, then the pass's own skips; `eligible`: the index behind them
    void counters(const int64_t *c, int eligible) {
        out->n_records = c[0]; out->n_unplaced = c[1]; out->n_flagged = c[2]; out->n_low_mapq = c[3]; out->n_no_cigar = c[4]; out->n_no_seq = c[5]; out->n_bad_cigar = c[6];
        out->n_no_ref = c[7]; out->n_too_long = c[8]; out->n_eligible = c[eligible];
    }
    // the header's tail behind the sixteen (of the overlap table with `overlap`), and the classes a row has: MASKED with a mask alone
    const char *tail(bool overlap = false) const {
        if (overlap) return mk.on ? "\tAGREE_REF\tAGREE_ALT\tDIFF_OTHER\tUNUSABLE\tLOWQ\tMASKED\n" : "\tAGREE_REF\tAGREE_ALT\tDIFF_OTHER\tUNUSABLE\tLOWQ\n";
        return mk.on ? "\tREAD_N\tREF_OTHER\tLOWQ\tINS\tDEL\tMASKED\n" : "\tREAD_N\tREF_OTHER\tLOWQ\tINS\tDEL\n";
    }
    int n_cls() const { return mk.on ? 22 : 21; }
};

struct ErrprofPass : ErrPass<ErrprofPass, gce_errprof_run, gce_errprof> {
    static constexpr const char *who = "gce_bam_error_profile", *options_known = "GCE_ERRPROF_DIRECT is the only one";
    static constexpr uint32_t option = GCE_ERRPROF_DIRECT;
    static constexpr auto create = gce_errprof_create; static constexpr auto window = gce_errprof_window; static constexpr auto error = gce_errprof_error;
    static constexpr auto destroy = gce_errprof_destroy; static constexpr auto free_out = gce_errprof_free;
    static constexpr auto set_ref = gce_errprof_set_ref; static constexpr auto set_mask = gce_errprof_set_mask; static constexpr auto set_sites = gce_errprof_set_sites;
    bool alloc(const ReduceInput &) {
        out->counts = (uint64_t *)malloc((size_t)3 * GCE_ERRPROF_MAX_CYCLE * GCE_ERRPROF_CLASSES * 8);
        return out->counts != nullptr;
    }
    int finish() {
        int64_t c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int rc = gce_errprof_finish(p, c, out->counts);
        if (rc != GCE_OK) return rc;
        counters(c, 9);
        if (mk.on) mk.out->n_masked_events = MaskJob::events(out->counts);
        return GCE_OK;
    }
    // rule O: the totals, with or without a file, and one row per cycle up to the last with a counter
    template <class EMIT> bool table(const ReduceInput &, bool, EMIT &&emit) {
        std::string buf;
        errprof_table(out->counts, "bases", "mismatches", tail(), 16, out->n_bases, out->n_mismatches, buf, n_cls());
        return emit(buf);
    }
};

}  // namespace

extern "C" {

int gce_bam_error_profile(const char *bam_path, const char *fasta_path, const char *bed_path, const char *tsv_path, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq,
                          uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errprof_run *out, char err[256]) {
    ErrprofPass ps{{out}};
    return reduce_run(ps, bam_path, bed_path, fasta_path, tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes, device_budget_bytes, err);
}

int gce_bam_error_profile_masked(const char *bam_path, const char *fasta_path, const char *bed_path, const char *mask_path, const char *tsv_path, int32_t device, int threads, int32_t min_mapq,
                                 int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errprof_run *out, gce_mask_run *mask,
                                 char err[256]) {
    ErrprofPass ps{{out}};
    ps.mk.on = true; ps.mk.path = mask_path; ps.mk.out = mask;
    return reduce_run(ps, bam_path, bed_path, fasta_path, tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes, device_budget_bytes, err);
}

}  // extern "C"
