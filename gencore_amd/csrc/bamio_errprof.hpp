// bamio_errprof.hpp -- mismatches by read cycle against the reference: gce_bam_error_profile (gce_errprof.hpp).  A part of
// bamio.cpp, in the shape of gce_bam_pileup: header, FASTA, optional BED, window loop, finish, table.
#pragma once
#include <unordered_map>
#include "gce_entry.h"
#include "bamio_reader.hpp"
#include "bamio_pileup.hpp"

extern "C" {

void gce_errprof_free(gce_errprof_run *out) {
    if (!out) return;
    free(out->counts);
    out->counts = nullptr;
}

int gce_bam_error_profile(const char *bam_path, const char *fasta_path, const char *bed_path, const char *tsv_path, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq,
                          uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errprof_run *out, char err[256]) {
    set_err(err, "");
    if (!bam_path || !fasta_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    out->n_intervals = -1;
    if (min_mapq < 0 || min_mapq > 255) { set_err(err, "min_mapq should be 0..255"); return GCE_ERR_INVALID; }
    if (min_baseq < 0 || min_baseq > 255) { set_err(err, "min_baseq should be 0..255"); return GCE_ERR_INVALID; }
    if (options & ~(uint32_t)GCE_ERRPROF_DIRECT) { set_err(err, "unknown option bit (GCE_ERRPROF_DIRECT is the only one)"); return GCE_ERR_INVALID; }
    { struct stat sf; if (stat(fasta_path, &sf) != 0 || S_ISDIR(sf.st_mode)) { set_err(err, "cannot open the reference FASTA"); return GCE_ERR_INVALID; } }
    if (bed_path) { struct stat sf; if (stat(bed_path, &sf) != 0 || S_ISDIR(sf.st_mode)) { set_err(err, "cannot open the BED file"); return GCE_ERR_INVALID; } }
    const double t_start = now_s();
    InputFile in;
    if (const char *verb = in.open(bam_path)) { set_err(err, (std::string("cannot ") + verb + " the BAM file").c_str()); return GCE_ERR_INVALID; }
    const std::string tmp = tsv_path ? std::string(tsv_path) + ".tmp" + std::to_string((long long)getpid()) : std::string();
    gce_errprof *p = nullptr; FILE *fo = nullptr; gce_fasta *fa = nullptr;
    auto done = [&](int code, const char *m) {
        set_err(err, m);                                                              // (m may be p's: copied before p goes)
        if (p) gce_errprof_destroy(p);
        if (fa) gce_fasta_free(fa);
        if (fo) { fclose(fo); fo = nullptr; }
        if (code != GCE_OK) { if (tsv_path) unlink(tmp.c_str()); gce_errprof_free(out); }
        return code;
    };
    if (in.fsz > 0 && !(in.fsz >= 4 && looks_gzip(in.fd, in.fsz))) return done(GCE_ERR_INVALID, "gce_bam_error_profile reads BAM, not SAM text");
    if (!in.is_bgzf()) return done(GCE_ERR_INVALID, "not a BGZF file");
    const int T = threads > 0 ? threads : default_threads();
    // ---- the header: the host inflates the first members (1 MB pieces) until it is whole
    uint64_t hdr_end = 0; int32_t n_ref = 0;
    std::vector<std::string> names; std::vector<uint32_t> lens;
    {
        PassReader rh; rh.fd = in.fd; rh.fsz = in.fsz; rh.T = T; rh.piece = window_bytes > 0 ? (size_t)std::min<uint64_t>(window_bytes, (uint64_t)1 << 20) : ((size_t)1 << 20);
        BamHeader bh;
        switch (read_bam_header(rh, Contigs::Skip, false, bh, &names, &lens)) {
        case HeaderRead::Failed: return done(GCE_ERR_INVALID, rh.msg.c_str());
        case HeaderRead::NotBam: return done(GCE_ERR_INVALID, "not a BAM stream");
        case HeaderRead::Ended: case HeaderRead::Empty: return done(GCE_ERR_INVALID, "truncated BAM header");
        case HeaderRead::Complete: break;
        }
        hdr_end = bh.hdr_end; n_ref = (int32_t)bh.n_ref;
    }
    // ---- rule B: the BED against the header's names, as gce_bam_pileup's rule S
    PileSites ps;
    if (bed_path) {
        std::vector<const char *> np; for (const std::string &s : names) np.push_back(s.c_str());
        int32_t n_reg = 0, *rt = nullptr, *rs = nullptr, *re = nullptr;
        if (gce_bed_load(bed_path, n_ref, np.data(), &n_reg, &rt, &rs, &re, nullptr) != GCE_OK) return done(GCE_ERR_INVALID, "cannot read the BED file");
        const bool fits = pile_sites(n_reg, rt, rs, re, lens, ps);
        gce_bed_free(n_reg, rt, rs, re, nullptr);
        if (!fits) return done(GCE_ERR_INVALID, "more than 2^28 sites in the BED file");
        out->n_intervals = (int64_t)ps.tid.size();
    }
    // ---- the contigs by the header's names, as calmd matches them
    std::vector<const char *> seq((size_t)n_ref, nullptr); std::vector<int64_t> slen((size_t)n_ref, -1);
    double t0 = now_s();
    {
        if (gce_fasta_load(fasta_path, T, &fa) != GCE_OK) return done(GCE_ERR_INVALID, "cannot read the reference FASTA");
        int32_t nc = 0; const char *const *ids = nullptr; const char *const *seqs = nullptr; const int64_t *flen = nullptr;
        gce_fasta_get(fa, &nc, &ids, &seqs, &flen);
        std::unordered_map<std::string, int32_t> where;
        for (int32_t c = 0; c < nc; c++) where.emplace(ids[c], c);
        for (int32_t t = 0; t < n_ref; t++) {
            auto it = where.find(names[(size_t)t].c_str());                            // (the name up to its first NUL)
            if (it != where.end()) { seq[(size_t)t] = seqs[it->second]; slen[(size_t)t] = flen[it->second]; }
        }
    }
    out->read_s += now_s() - t0;
    (void)gce_device_bytes(nullptr, nullptr, 1);
    int rc = gce_errprof_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options, &p);
    if (rc != GCE_OK) return done(rc, "no HIP device");
    if ((rc = gce_errprof_set_ref(p, n_ref, seq.data(), slen.data())) != GCE_OK) return done(rc, gce_errprof_error(p));
    gce_fasta_free(fa); fa = nullptr;
    if ((rc = gce_errprof_set_sites(p, bed_path ? (int64_t)ps.tid.size() : -1, ps.tid.data(), ps.start.data(), ps.end.data())) != GCE_OK) return done(rc, gce_errprof_error(p));
    // ---- the file from its first byte, window by window: the host reads and finds the members, the GPU inflates, indexes and counts them
    PassReader rd; rd.fd = in.fd; rd.fsz = in.fsz; rd.T = T; rd.piece = window_bytes > 0 ? (size_t)window_bytes : ((size_t)64 << 20);
    double gpu_s = 0;
    std::string wmsg;
    rc = for_each_window(rd, hdr_end, &out->read_s, &gpu_s, wmsg, [&](PassReader &r, uint64_t, uint64_t sk) {
        return gce_errprof_window(p, r.comp.data(), r.used, (int32_t)r.blocks.size(), r.z_coff.data(), r.z_csize.data(), r.z_usize.data(), sk, n_ref, r.last_piece() ? 1 : 0, &out->errprof_s);
    });
    if (rc != GCE_OK) return done(rc, wmsg.empty() ? gce_errprof_error(p) : wmsg.c_str());
    const size_t nk = (size_t)3 * GCE_ERRPROF_MAX_CYCLE * GCE_ERRPROF_CLASSES;
    out->counts = (uint64_t *)malloc(nk * 8);
    if (!out->counts) return done(GCE_ERR_OOM, "out of host memory for the counters");
    t0 = now_s();
    int64_t c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = gce_errprof_finish(p, c, out->counts)) != GCE_OK) return done(rc, gce_errprof_error(p));
    gpu_s += now_s() - t0;
    out->n_records = c[0]; out->n_unplaced = c[1]; out->n_flagged = c[2]; out->n_low_mapq = c[3]; out->n_no_cigar = c[4]; out->n_no_seq = c[5]; out->n_bad_cigar = c[6];
    out->n_no_ref = c[7]; out->n_too_long = c[8]; out->n_eligible = c[9];
    out->inflate_index_s = gpu_s - out->errprof_s;
    // ---- rule O: the totals, and the table, to a temporary name, renamed at the end
    t0 = now_s();
    std::string buf = "#segment\tcycle\tbases\tmismatches";
    for (const char *r : {"A", "C", "G", "T"}) for (const char *b : {"A", "C", "G", "T"}) { buf += '\t'; buf += r; buf += '>'; buf += b; }
    buf += "\tREAD_N\tREF_OTHER\tLOWQ\tINS\tDEL\n";
    for (int g = 0; g < 3; g++) {
        const uint64_t *seg = out->counts + (size_t)g * GCE_ERRPROF_MAX_CYCLE * GCE_ERRPROF_CLASSES;
        int last = 0;                                                                 // the last cycle with a counter
        for (int cy = 1; cy <= GCE_ERRPROF_MAX_CYCLE; cy++) for (int k = 0; k < 21; k++) if (seg[(size_t)(cy - 1) * GCE_ERRPROF_CLASSES + k]) last = cy;
        for (int cy = 1; cy <= last; cy++) {
            const uint64_t *k = seg + (size_t)(cy - 1) * GCE_ERRPROF_CLASSES;
            uint64_t bases = 0, mism = 0;
            for (int q = 0; q < 16; q++) { bases += k[q]; if ((q >> 2) != (q & 3)) mism += k[q]; }
            out->n_bases += (int64_t)bases; out->n_mismatches += (int64_t)mism;
            char line[26 * 21], *w = line;
            w = pile_num(w, (uint64_t)g); *w++ = '\t'; w = pile_num(w, (uint64_t)cy); *w++ = '\t'; w = pile_num(w, bases); *w++ = '\t'; w = pile_num(w, mism);
            for (int q = 0; q < 21; q++) { *w++ = '\t'; w = pile_num(w, k[q]); }
            *w++ = '\n';
            buf.append(line, (size_t)(w - line));
        }
    }
    if (tsv_path) {
        fo = fopen(tmp.c_str(), "wb");
        if (!fo) return done(GCE_ERR_INVALID, "cannot write the table");
        const bool ok = fwrite(buf.data(), 1, buf.size(), fo) == buf.size();
        const bool closed = fclose(fo) == 0; fo = nullptr;
        if (!ok || !closed || rename(tmp.c_str(), tsv_path) != 0) return done(GCE_ERR_INVALID, "cannot write the table");
    }
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK, "");
}

}  // extern "C"
