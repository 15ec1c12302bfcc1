// bamio_pileup.hpp -- bases per strand at BED targets: gce_bam_pileup (gce_pileup.hpp).  A part of bamio.cpp, in the shape of
// gce_bam_index: header, BED, optional FASTA, window loop, finish, table.
#pragma once
#include <unordered_map>
#include "gce_entry.h"
#include "bamio_reader.hpp"

namespace {

// rule S: the regions clamped to their contigs, sorted by (tid, start), merged where they overlap or abut; site0: the site index of every
// interval's start.  false: more than 2^28 sites
struct PileSites { std::vector<int32_t> tid, start, end; std::vector<uint32_t> site0; uint64_t n_sites = 0; };
bool pile_sites(int32_t n_reg, const int32_t *tid, const int32_t *start, const int32_t *end, const std::vector<uint32_t> &lens, PileSites &o) {
    struct R { int32_t tid; int64_t a, z; };
    std::vector<R> v;
    for (int32_t k = 0; k < n_reg; k++) {
        if (tid[k] < 0 || tid[k] >= (int32_t)lens.size()) continue;
        const int64_t a = std::max<int64_t>(start[k], 0), z = std::min<int64_t>(end[k], (int64_t)std::min<uint32_t>(lens[(size_t)tid[k]], 0x7FFFFFFFu));
        if (a < z) v.push_back({tid[k], a, z});
    }
    std::sort(v.begin(), v.end(), [](const R &x, const R &y) { return x.tid != y.tid ? x.tid < y.tid : x.a != y.a ? x.a < y.a : x.z < y.z; });
    for (const R &r : v) {
        if (!o.tid.empty() && o.tid.back() == r.tid && r.a <= o.end.back()) { o.end.back() = (int32_t)std::max<int64_t>(o.end.back(), r.z); continue; }
        o.tid.push_back(r.tid); o.start.push_back((int32_t)r.a); o.end.push_back((int32_t)r.z);
    }
    for (size_t j = 0; j < o.tid.size(); j++) {
        o.site0.push_back((uint32_t)o.n_sites);
        o.n_sites += (uint64_t)(o.end[j] - o.start[j]);
        if (o.n_sites > (1ull << 28)) return false;
    }
    return true;
}

inline char *pile_num(char *w, uint64_t v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) *w++ = t[--n]; return w; }

}  // namespace

extern "C" {

void gce_pileup_free(gce_pileup_run *out) {
    if (!out) return;
    free(out->site_tid); free(out->site_pos); free(out->counts);
    out->site_tid = out->site_pos = nullptr; out->counts = nullptr;
}

int gce_bam_pileup(const char *bam_path, const char *bed_path, const char *fasta_path, const char *tsv_path, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq,
                   uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_pileup_run *out, char err[256]) {
    set_err(err, "");
    if (!bam_path || !bed_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    if (min_mapq < 0 || min_mapq > 255) { set_err(err, "min_mapq should be 0..255"); return GCE_ERR_INVALID; }
    if (min_baseq < 0 || min_baseq > 255) { set_err(err, "min_baseq should be 0..255"); return GCE_ERR_INVALID; }
    if (options & ~(uint32_t)GCE_PILEUP_DIRECT) { set_err(err, "unknown option bit (GCE_PILEUP_DIRECT is the only one)"); return GCE_ERR_INVALID; }
    { struct stat sf; if (stat(bed_path, &sf) != 0 || S_ISDIR(sf.st_mode)) { set_err(err, "cannot open the BED file"); return GCE_ERR_INVALID; } }
    if (fasta_path) { struct stat sf; if (stat(fasta_path, &sf) != 0 || S_ISDIR(sf.st_mode)) { set_err(err, "cannot open the reference FASTA"); return GCE_ERR_INVALID; } }
    const double t_start = now_s();
    InputFile in;
    if (const char *verb = in.open(bam_path)) { set_err(err, (std::string("cannot ") + verb + " the BAM file").c_str()); return GCE_ERR_INVALID; }
    const std::string tmp = tsv_path ? std::string(tsv_path) + ".tmp" + std::to_string((long long)getpid()) : std::string();
    gce_pileup *p = nullptr; FILE *fo = nullptr; gce_fasta *fa = nullptr;
    auto done = [&](int code, const char *m) {
        set_err(err, m);                                                              // (m may be p's: copied before p goes)
        if (p) gce_pileup_destroy(p);
        if (fa) gce_fasta_free(fa);
        if (fo) { fclose(fo); fo = nullptr; }
        if (code != GCE_OK) { if (tsv_path) unlink(tmp.c_str()); gce_pileup_free(out); }
        return code;
    };
    if (in.fsz > 0 && !(in.fsz >= 4 && looks_gzip(in.fd, in.fsz))) return done(GCE_ERR_INVALID, "gce_bam_pileup reads BAM, not SAM text");
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
    // ---- rule S: the BED against the header's names
    PileSites ps;
    {
        std::vector<const char *> np; for (const std::string &s : names) np.push_back(s.c_str());
        int32_t n_reg = 0, *rt = nullptr, *rs = nullptr, *re = nullptr;
        if (gce_bed_load(bed_path, n_ref, np.data(), &n_reg, &rt, &rs, &re, nullptr) != GCE_OK) return done(GCE_ERR_INVALID, "cannot read the BED file");
        const bool fits = pile_sites(n_reg, rt, rs, re, lens, ps);
        gce_bed_free(n_reg, rt, rs, re, nullptr);
        if (!fits) return done(GCE_ERR_INVALID, "more than 2^28 sites in the BED file");
    }
    out->n_sites = (int64_t)ps.n_sites; out->n_intervals = (int64_t)ps.tid.size();
    // ---- rule O's ref column: the contigs by the header's names, as calmd matches them; the bases stay on the host
    std::vector<const char *> seq((size_t)n_ref, nullptr); std::vector<int64_t> slen((size_t)n_ref, -1);
    double t0 = now_s();
    if (fasta_path) {
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
    int rc = gce_pileup_create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options, &p);
    if (rc != GCE_OK) return done(rc, "no HIP device");
    if ((rc = gce_pileup_set_sites(p, n_ref, (int64_t)ps.tid.size(), ps.tid.data(), ps.start.data(), ps.end.data(), ps.site0.data())) != GCE_OK) return done(rc, gce_pileup_error(p));
    // ---- the file from its first byte, window by window: the host reads and finds the members, the GPU inflates, indexes and counts them
    PassReader rd; rd.fd = in.fd; rd.fsz = in.fsz; rd.T = T; rd.piece = window_bytes > 0 ? (size_t)window_bytes : ((size_t)64 << 20);
    double gpu_s = 0;
    std::string wmsg;
    rc = for_each_window(rd, hdr_end, &out->read_s, &gpu_s, wmsg, [&](PassReader &r, uint64_t, uint64_t sk) {
        return gce_pileup_window(p, r.comp.data(), r.used, (int32_t)r.blocks.size(), r.z_coff.data(), r.z_csize.data(), r.z_usize.data(), sk, n_ref, r.last_piece() ? 1 : 0, &out->pileup_s);
    });
    if (rc != GCE_OK) return done(rc, wmsg.empty() ? gce_pileup_error(p) : wmsg.c_str());
    const size_t ns = (size_t)ps.n_sites;
    out->site_tid = (int32_t *)malloc(std::max<size_t>(ns, 1) * 4); out->site_pos = (int32_t *)malloc(std::max<size_t>(ns, 1) * 4); out->counts = (uint32_t *)malloc(std::max<size_t>(ns, 1) * 64);
    if (!out->site_tid || !out->site_pos || !out->counts) return done(GCE_ERR_OOM, "out of host memory for the counters");
    t0 = now_s();
    int64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = gce_pileup_finish(p, c, out->counts)) != GCE_OK) return done(rc, gce_pileup_error(p));
    gpu_s += now_s() - t0;
    out->n_records = c[0]; out->n_unplaced = c[1]; out->n_flagged = c[2]; out->n_low_mapq = c[3]; out->n_no_cigar = c[4]; out->n_no_seq = c[5]; out->n_bad_cigar = c[6]; out->n_eligible = c[7];
    out->inflate_index_s = gpu_s - out->pileup_s;
    for (size_t j = 0, i = 0; j < ps.tid.size(); j++)
        for (int32_t x = ps.start[j]; x < ps.end[j]; x++, i++) { out->site_tid[i] = ps.tid[j]; out->site_pos[i] = x; }
    // ---- rule O: the table, to a temporary name, renamed at the end
    t0 = now_s();
    if (tsv_path) {
        fo = fopen(tmp.c_str(), "wb");
        if (!fo) return done(GCE_ERR_INVALID, "cannot write the table");
        std::string buf;
        buf = "#contig\tpos\tref\tdepth";
        for (const char *st : {"fwd", "rev"}) for (const char *cl : {"A", "C", "G", "T", "N", "DEL", "INS", "LOWQ"}) { buf += '\t'; buf += st; buf += '_'; buf += cl; }
        buf += '\n';
        bool ok = true;
        size_t i = 0;
        for (size_t j = 0; j < ps.tid.size() && ok; j++) {
            const int32_t t = ps.tid[j];
            const char *nm = names[(size_t)t].c_str(); const size_t nl = strlen(nm);
            for (int32_t x = ps.start[j]; x < ps.end[j]; x++, i++) {
                char line[16 + 20 * 20], *w = line;
                const uint32_t *k = out->counts + 16 * i;
                char b = 'N';
                if (seq[(size_t)t] && (int64_t)x < slen[(size_t)t]) { b = fa_upper(seq[(size_t)t][x]); if (b <= 32 || b >= 127) b = 'N'; }   // (FastaReader keeps a line feed of an empty line as a base)
                *w++ = '\t'; w = pile_num(w, (uint64_t)x + 1); *w++ = '\t'; *w++ = b; *w++ = '\t';
                w = pile_num(w, (uint64_t)k[0] + k[1] + k[2] + k[3] + k[4] + k[8] + k[9] + k[10] + k[11] + k[12]);
                for (int q = 0; q < 16; q++) { *w++ = '\t'; w = pile_num(w, k[q]); }
                *w++ = '\n';
                buf.append(nm, nl); buf.append(line, (size_t)(w - line));
                if (buf.size() >= (1u << 20)) { ok = fwrite(buf.data(), 1, buf.size(), fo) == buf.size(); buf.clear(); if (!ok) break; }
            }
        }
        ok = ok && fwrite(buf.data(), 1, buf.size(), fo) == buf.size();
        const bool closed = fclose(fo) == 0; fo = nullptr;
        if (!ok || !closed || rename(tmp.c_str(), tsv_path) != 0) return done(GCE_ERR_INVALID, "cannot write the table");
    }
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK, "");
}

}  // extern "C"
