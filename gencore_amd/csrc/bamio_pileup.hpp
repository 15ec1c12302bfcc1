// bamio_pileup.hpp -- bases per strand at BED targets: gce_bam_pileup (gce_pileup.hpp).  A part of bamio.cpp: the pass's own part
// of reduce_run (bamio_reduce.hpp), which runs it, and PilePass, what this runner and bamio_fragpile.hpp's do alike: the site arrays, the
// eight shared counters and the table's rows.
#pragma once
#include "bamio_reduce.hpp"

namespace {

// gce_pileup_free and gce_fragpile_free
template <class RUN> void pile_free(RUN *out) {
    if (!out) return;
    free(out->site_tid); free(out->site_pos); free(out->counts);
    out->site_tid = out->site_pos = nullptr; out->counts = nullptr;
}
// the site arrays of a gce_pileup_run or gce_fragpile_run: tid and pos of every site, room for its 16 counters
template <class RUN> bool pile_alloc(const ReduceInput &in, RUN *out) {
    const size_t ns = std::max<size_t>((size_t)in.ps.n_sites, 1);
    out->site_tid = (int32_t *)malloc(ns * 4); out->site_pos = (int32_t *)malloc(ns * 4); out->counts = (uint32_t *)malloc(ns * 64);
    if (!out->site_tid || !out->site_pos || !out->counts) return false;
    const PileSites &ps = in.ps;
    for (size_t j = 0, i = 0; j < ps.tid.size(); j++)
        for (int32_t x = ps.start[j]; x < ps.end[j]; x++, i++) { out->site_tid[i] = ps.tid[j]; out->site_pos[i] = x; }
    return true;
}
// rule O: one row per site from counts (16 per site), handed on in pieces of 1 MB; the ref column from the FASTA's bases, which stay on the host
template <class EMIT> bool pile_table(const ReduceInput &in, const uint32_t *counts, EMIT &&emit) {
    const PileSites &ps = in.ps;
    std::string buf;
    buf = "#contig\tpos\tref\tdepth";
    for (const char *st : {"fwd", "rev"}) for (const char *cl : {"A", "C", "G", "T", "N", "DEL", "INS", "LOWQ"}) { buf += '\t'; buf += st; buf += '_'; buf += cl; }
    buf += '\n';
    size_t i = 0;
    for (size_t j = 0; j < ps.tid.size(); j++) {
        const int32_t t = ps.tid[j];
        const char *nm = in.names[(size_t)t].c_str(); const size_t nl = strlen(nm);
        for (int32_t x = ps.start[j]; x < ps.end[j]; x++, i++) {
            char line[16 + 20 * 20], *w = line;
            const uint32_t *k = counts + 16 * i;
            char b = 'N';
            if (in.seq[(size_t)t] && (int64_t)x < in.slen[(size_t)t]) { b = fa_upper(in.seq[(size_t)t][x]); if (b <= 32 || b >= 127) b = 'N'; }   // (FastaReader keeps a line feed of an empty line as a base)
            *w++ = '\t'; w = pile_num(w, (uint64_t)x + 1); *w++ = '\t'; *w++ = b; *w++ = '\t';
            w = pile_num(w, (uint64_t)k[0] + k[1] + k[2] + k[3] + k[4] + k[8] + k[9] + k[10] + k[11] + k[12]);
            for (int q = 0; q < 16; q++) { *w++ = '\t'; w = pile_num(w, k[q]); }
            *w++ = '\n';
            buf.append(nm, nl); buf.append(line, (size_t)(w - line));
            if (buf.size() >= (1u << 20)) { if (!emit(buf)) return false; buf.clear(); }
        }
    }
    return emit(buf);
}

// What the two pileup passes do alike around their device objects: PileupPass and FragpilePass (bamio_fragpile.hpp) derive from it and
// name their set_sites beside create / window / ... (bamio_reduce.hpp)
template <class PASS, class RUN, class OBJ> struct PilePass {
    static constexpr bool bed_first = true;
    RUN *out; OBJ *p = nullptr;
    void zero() { memset(out, 0, sizeof *out); }
    void sites(const ReduceInput &in) { out->n_sites = (int64_t)in.ps.n_sites; out->n_intervals = (int64_t)in.ps.tid.size(); }
    int set(ReduceInput &in) { return PASS::set_sites(p, in.n_ref, (int64_t)in.ps.tid.size(), in.ps.tid.data(), in.ps.start.data(), in.ps.end.data(), in.ps.site0.data()); }
    double *pass_s() { return &out->pileup_s; }
    bool alloc(const ReduceInput &in) { return pile_alloc(in, out); }
    // c[0] records, c[1..6] rule E's skips in its order, c[7] eligible
    void counters(const int64_t *c) {
        out->n_records = c[0]; out->n_unplaced = c[1]; out->n_flagged = c[2]; out->n_low_mapq = c[3]; out->n_no_cigar = c[4]; out->n_no_seq = c[5]; out->n_bad_cigar = c[6]; out->n_eligible = c[7];
    }
    template <class EMIT> bool table(const ReduceInput &in, bool to_file, EMIT &&emit) { return !to_file || pile_table(in, out->counts, emit); }
};

}  // namespace

extern "C" {

void gce_pileup_free(gce_pileup_run *out) { pile_free(out); }

}  // extern "C"

namespace {

struct PileupPass : PilePass<PileupPass, gce_pileup_run, gce_pileup> {
    static constexpr const char *who = "gce_bam_pileup", *options_known = "GCE_PILEUP_DIRECT is the only one";
    static constexpr uint32_t option = GCE_PILEUP_DIRECT;
    static constexpr auto create = gce_pileup_create; static constexpr auto window = gce_pileup_window; static constexpr auto error = gce_pileup_error;
    static constexpr auto destroy = gce_pileup_destroy; static constexpr auto free_out = gce_pileup_free; static constexpr auto set_sites = gce_pileup_set_sites;
    int finish() {
        int64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int rc = gce_pileup_finish(p, c, out->counts);
        if (rc == GCE_OK) counters(c);
        return rc;
    }
};

}  // namespace

extern "C" {

int gce_bam_pileup(const char *bam_path, const char *bed_path, const char *fasta_path, const char *tsv_path, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq,
                   uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_pileup_run *out, char err[256]) {
    PileupPass ps{{out}};
    return reduce_run(ps, bam_path, bed_path, fasta_path, tsv_path, device, threads, min_mapq, min_baseq, exclude_flags, options, window_bytes, device_budget_bytes, err);
}

}  // extern "C"
