// gce_report.hpp — the reference's reports and the header of an input file, on the host (included by bamio.cpp; no GPU code).
//
// Replaces what the reference writes after its read loop (src/gencore.cpp:284-292):
//   JsonReporter::report (src/jsonreporter.cpp:11-44), Stats::reportJSON (src/stats.cpp:153-193), Bed::reportJSON (src/bed.cpp:81-100)
//     -> gce_report_json: the same bytes, from the Stats blocks and the depth statistics the GPU computed (gce_run_bam_depth);
//   Stats::print (src/stats.cpp:195-215) -> gce_report_summary;
//   sam_hdr_read's contig table (src/gencore.cpp:180 via htslib) -> gce_bam_read_header: only the BGZF members the header spans are inflated.
// Numbers are printed as a default std::ostream prints them (doubles: "%g", precision 6, glibc's nan / -nan / inf; integers as they are),
// and every rate is computed with the reference's expression so that a 0/0 gives the same NaN; names are written raw, without JSON escaping.
#pragma once
#include <zlib.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/gencore_amd.h"
#include "gce_samtext.hpp"

namespace gce_report {

inline void put_g(std::string &o, double v) { char b[64]; snprintf(b, sizeof b, "%g", v); o += b; }              // ostream << double
inline void put_i(std::string &o, long long v) { o += std::to_string(v); }
inline void put_f(std::string &o, double v) { char b[512]; snprintf(b, sizeof b, "%f", v); o += b; }              // std::to_string(double)

inline long mapped_reads(const gce_stats &s) { return (long)(s.reads - s.reads_unmapped); }                   // stats.cpp:89-91
inline long mapped_bases(const gce_stats &s) { return (long)(s.bases - s.bases_unmapped); }                   // :85-87
inline double mapping_rate(const gce_stats &s) { return mapped_reads(s) / (double)s.reads; }                   // :131-133
inline double dup_rate(const gce_stats &s) { return 1.0 - (s.molecules_se + s.molecules_pe * 2) / (double)mapped_reads(s); }   // :135-137
inline double mismatch_rate(const gce_stats &s) { return (double)s.base_mismatches / mapped_bases(s); }       // :139-141 (:160)

struct Depth {               // one block's depth statistics
    int32_t n_targets; const char *const *target_name; const int64_t *bin_off; const int64_t *bins; int32_t step;
    bool has_bed; int32_t n_regions; const int32_t *tid, *start, *end; const char *const *region_name; const int64_t *count;
};

// BedRegion::getAvgDepth (src/bed.h:29-34)
inline int avg_depth(int32_t start, int32_t end, int64_t count) { return end <= start ? 0 : (int)round(double(count) / (end - start)); }

// Bed::reportJSON (src/bed.cpp:81-100): the regions grouped by contig in header order, in file order inside a contig; regions of a contig
// that is not in the header were never put in the map (bed.cpp:164-165)
inline void bed_json(std::string &o, const Depth &d) {
    o += "\t\t\"coverage_bed\":{\n";
    for (int32_t c = 0; c < d.n_targets; c++) {
        o += "\t\t\t\""; o += d.target_name[c]; o += "\":[\n";
        std::vector<int32_t> sel;
        for (int32_t k = 0; k < d.n_regions; k++) if (d.tid[k] == c) sel.push_back(k);
        for (size_t p = 0; p < sel.size(); p++) {
            const int32_t k = sel[p];
            o += "\t\t\t\t[\""; o += d.region_name ? d.region_name[k] : ""; o += "\",";
            put_i(o, d.start[k]); o += ","; put_i(o, d.end[k]); o += ","; put_i(o, avg_depth(d.start[k], d.end[k], d.count[k])); o += "]";
            if (p != sel.size() - 1) o += ",";
            o += "\n";
        }
        o += "\t\t\t]";
        if (c != d.n_targets - 1) o += ",";
        o += "\n";
    }
    o += "\t\t}\n";
}

// Stats::reportJSON (src/stats.cpp:153-193)
inline void stats_json(std::string &o, const gce_stats &s, const Depth &d) {
    o += "\t\t\"total_reads\": "; put_i(o, s.reads); o += ",\n";
    o += "\t\t\"total_bases\": "; put_i(o, s.bases); o += ",\n";
    o += "\t\t\"mapped_reads\": "; put_i(o, mapped_reads(s)); o += ",\n";
    o += "\t\t\"mapped_bases\": "; put_i(o, mapped_bases(s)); o += ",\n";
    o += "\t\t\"mismatched_bases\": "; put_i(o, s.base_mismatches); o += ",\n";
    o += "\t\t\"reads_with_mismatched_bases\": "; put_i(o, s.reads_with_mismatches); o += ",\n";
    o += "\t\t\"mismatch_rate\": "; put_g(o, mismatch_rate(s)); o += ",\n";
    o += "\t\t\"total_mapping_clusters\": "; put_i(o, s.clusters); o += ",\n";
    o += "\t\t\"multiple_fragments_clusters\": "; put_i(o, s.multi_molecule_clusters); o += ",\n";
    o += "\t\t\"total_fragments\": "; put_i(o, s.molecules); o += ",\n";
    o += "\t\t\"single_end_fragments\": "; put_i(o, s.molecules_se); o += ",\n";
    o += "\t\t\"paired_end_fragments\": "; put_i(o, s.molecules_pe); o += ",\n";
    o += "\t\t\"duplication_level_histogram\": [";
    for (int i = 1; i < GCE_MAX_SUPPORTING_READS - 1; i++) { put_i(o, s.supporting_hist[i]); o += ","; }
    put_i(o, s.supporting_hist[GCE_MAX_SUPPORTING_READS - 1]);
    o += "],\n";
    o += "\t\t\"coverage_sampling\": "; put_i(o, d.step); o += ",\n";
    o += "\t\t\"coverage\":{\n";
    for (int32_t c = 0; c < d.n_targets; c++) {
        o += "\t\t\t\""; o += d.target_name[c]; o += "\":[";
        for (int64_t i = d.bin_off[c]; i < d.bin_off[c + 1]; i++) {
            put_i(o, (long)round((double)d.bins[i] / d.step));
            if (i < d.bin_off[c + 1] - 1) o += ",";
        }
        o += "]";
        if (c != d.n_targets - 1) o += ",";
        o += "\n";
    }
    o += "\t\t}";
    if (d.has_bed) { o += ",\n"; bed_json(o, d); }
    else o += "\n";
}

// Stats::print (src/stats.cpp:195-215)
inline void summary(std::string &o, const gce_stats &s, bool is_post) {
    o += "Total reads: "; put_i(o, s.reads); o += "\n";
    o += "Total bases: "; put_i(o, s.bases); o += "\n";
    o += "Mapped reads: "; put_i(o, mapped_reads(s)); o += " ("; put_f(o, mapped_reads(s) * 100.0 / s.reads); o += "%)\n";
    o += "Mapped bases: "; put_i(o, mapped_bases(s)); o += " ("; put_f(o, mapped_bases(s) * 100.0 / s.bases); o += "%)\n";
    o += "Bases mismatched with reference: "; put_i(o, s.base_mismatches); o += " ("; put_f(o, s.base_mismatches * 100.0 / mapped_bases(s)); o += "%)\n";
    o += "Reads with mismatched bases: "; put_i(o, s.reads_with_mismatches); o += " ("; put_f(o, s.reads_with_mismatches * 100.0 / mapped_reads(s)); o += "%)\n";
    o += "Total mapping clusters: "; put_i(o, s.clusters); o += "\n";
    o += "Mapping clusters with multiple fragments: "; put_i(o, s.multi_molecule_clusters); o += "\n";
    o += "Total fragments: "; put_i(o, s.molecules); o += "\n";
    o += "Fragments with single-end reads: "; put_i(o, s.molecules_se); o += "\n";
    o += "Fragments with paired-end reads: "; put_i(o, s.molecules_pe); o += "\n";
    if (!is_post) {
        o += "Duplication level histogram: \n";
        for (int i = 1; i < GCE_MAX_SUPPORTING_READS && i <= 10; i++) {
            if (s.supporting_hist[i] == 0) break;
            o += "    Fragments with "; put_i(o, i); o += " duplicates: "; put_i(o, s.supporting_hist[i]); o += "\n";
        }
    } else {
        o += "\nSingle Stranded Consensus Sequence (has 'FR' tag): "; put_i(o, s.sscs); o += "\n";
        o += "Duplex Consensus Sequence (has both 'FS' and 'RR' tags): "; put_i(o, s.dcs); o += "\n";
    }
}

// BGZF members from the front of a file, inflated one at a time until `need` bytes of the stream are there (or the file ends)
struct BgzfFront {
    FILE *f; std::vector<uint8_t> out; std::string err; bool eof = false;
    bool more() {
        uint8_t h[18];
        const size_t got = fread(h, 1, 12, f);
        if (got == 0) { eof = true; return false; }
        if (got < 12 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) { err = "not a BGZF member"; return false; }
        const uint16_t xlen = (uint16_t)(h[10] | h[11] << 8);
        std::vector<uint8_t> extra(xlen);
        if (fread(extra.data(), 1, xlen, f) != xlen) { err = "truncated BGZF header"; return false; }
        int bsize = -1;
        for (size_t p = 0; p + 4 <= xlen;) {                        // subfields SI1 SI2 SLEN(2) data; BC carries BSIZE
            const uint16_t slen = (uint16_t)(extra[p + 2] | extra[p + 3] << 8);
            if (extra[p] == 'B' && extra[p + 1] == 'C' && slen == 2 && p + 6 <= xlen) bsize = extra[p + 4] | extra[p + 5] << 8;
            p += 4 + (size_t)slen;
        }
        if (bsize < 0 || bsize + 1 < 12 + xlen + 8) { err = "BGZF member without a valid BSIZE"; return false; }
        std::vector<uint8_t> rest((size_t)(bsize + 1 - 12 - xlen));
        if (fread(rest.data(), 1, rest.size(), f) != rest.size()) { err = "truncated BGZF member"; return false; }
        const size_t cdata = rest.size() - 8;
        const uint32_t isize = (uint32_t)rest[cdata + 4] | (uint32_t)rest[cdata + 5] << 8 | (uint32_t)rest[cdata + 6] << 16 | (uint32_t)rest[cdata + 7] << 24;
        if (isize > 0x10000) { err = "BGZF member larger than 64 KiB"; return false; }
        const size_t at = out.size();
        out.resize(at + isize);
        z_stream z; memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) { err = "zlib"; return false; }
        z.next_in = rest.data(); z.avail_in = (uInt)cdata; z.next_out = out.data() + at; z.avail_out = isize;
        const int zr = inflate(&z, Z_FINISH);
        inflateEnd(&z);
        if (zr != Z_STREAM_END || z.avail_out != 0) { err = "damaged BGZF member"; return false; }
        return true;
    }
    bool need(size_t n) { while (out.size() < n) if (!more()) { if (err.empty()) err = "the file ends inside the BAM header"; return false; } return true; }
};

inline uint32_t rd_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

inline bool read_header(const char *path, std::vector<std::string> &names, std::vector<uint32_t> &lens, std::string &err) {
    FILE *f = fopen(path, "rb");
    if (!f) { err = "cannot open the input file"; return false; }
    uint8_t m[2] = {0, 0};
    const size_t nm = fread(m, 1, 2, f);
    rewind(f);
    bool ok = false;
    if (nm == 2 && m[0] == 0x1f && m[1] == 0x8b) {                 // BAM: magic, l_text, text, n_ref, then (l_name, name, l_ref) per contig
        BgzfFront z{f};
        ok = z.need(8);
        if (ok && memcmp(z.out.data(), "BAM\1", 4) != 0) { ok = false; err = "not a BAM file"; }
        size_t p = 8;
        if (ok) { p += rd_u32(z.out.data() + 4); ok = z.need(p + 4); }
        if (ok) {
            const uint32_t n_ref = rd_u32(z.out.data() + p);
            p += 4;
            for (uint32_t k = 0; ok && k < n_ref; k++) {
                if (!(ok = z.need(p + 4))) break;
                const uint32_t ln = rd_u32(z.out.data() + p);
                if (!(ok = z.need(p + 4 + ln + 4))) break;
                const char *s = (const char *)z.out.data() + p + 4;
                names.emplace_back(s, strnlen(s, ln));
                lens.push_back(rd_u32(z.out.data() + p + 4 + ln));
                p += 8 + (size_t)ln;
            }
        }
        if (!ok && err.empty()) err = z.err;
    } else {                                                       // SAM text: the '@' lines in front of the first alignment
        std::string text; char *line = nullptr; size_t cap = 0; ssize_t n;
        while ((n = getline(&line, &cap, f)) > 0 && line[0] == '@') text.append(line, (size_t)n);
        free(line);
        ok = samtext::parse_header_text(text, names, lens);
        if (!ok) err = "bad @SQ line in the SAM header";
    }
    fclose(f);
    return ok;
}

}  // namespace gce_report

extern "C" {

int gce_report_json(const char *path, const gce_stats *pre, const gce_stats *post, const gce_depth_run *depth, const char *const *target_name,
                    const char *const *region_name, int32_t has_bed, int32_t coverage_step, const char *command, char err[256]) {
    auto fail = [&](const char *m) { if (err) { strncpy(err, m, 255); err[255] = 0; } return GCE_ERR_INVALID; };
    if (err) err[0] = 0;
    if (!path || !pre || !post || !depth || coverage_step <= 0) return fail("invalid argument");
    if (depth->n_targets > 0 && (!target_name || !depth->bin_off || !depth->pre_depth || !depth->post_depth)) return fail("depth statistics without contigs");
    if (has_bed && depth->n_regions > 0 && (!depth->region_tid || !depth->region_start || !depth->region_end || !depth->pre_bed || !depth->post_bed))
        return fail("BED statistics without regions");
    using namespace gce_report;
    const Depth dpre{depth->n_targets, target_name, depth->bin_off, depth->pre_depth, coverage_step, has_bed != 0, depth->n_regions,
                     depth->region_tid, depth->region_start, depth->region_end, region_name, depth->pre_bed};
    Depth dpost = dpre; dpost.bins = depth->post_depth; dpost.count = depth->post_bed;
    std::string o;                                                 // JsonReporter::report (src/jsonreporter.cpp:11-44)
    o += "{\n";
    o += "\t\"summary\": {\n";
    o += "\t\t\"mapping_rate\":"; put_g(o, mapping_rate(*pre)); o += ",\n";
    o += "\t\t\"duplication_rate\":"; put_g(o, dup_rate(*pre)); o += ",\n";
    o += "\t\t\"single_stranded_consensus_sequence\":"; put_i(o, post->sscs); o += ",\n";
    o += "\t\t\"duplex_consensus_sequence\":"; put_i(o, post->dcs); o += "\n";
    o += "\t},\n";
    o += "\t\"before_processing\": {\n"; stats_json(o, *pre, dpre); o += "\n\t},\n";
    o += "\t\"after_processing\": {\n"; stats_json(o, *post, dpost); o += "\n\t},\n";
    o += "\t\"command\": \""; o += command ? command : ""; o += "\"\n";
    o += "}";
    FILE *f = fopen(path, "wb");
    if (!f) return fail("cannot open the JSON report");
    const bool wrote = fwrite(o.data(), 1, o.size(), f) == o.size();
    if (fclose(f) != 0 || !wrote) return fail("cannot write the JSON report");
    return GCE_OK;
}

int gce_report_summary(const gce_stats *stats, int32_t is_post, char *buf, size_t cap, size_t *len) {
    if (!stats) return GCE_ERR_INVALID;
    std::string o;
    gce_report::summary(o, *stats, is_post != 0);
    if (len) *len = o.size();
    if (!buf || cap < o.size() + 1) return GCE_ERR_INVALID;
    memcpy(buf, o.c_str(), o.size() + 1);
    return GCE_OK;
}

int gce_bam_read_header(const char *path, int32_t *n_targets, char ***target_name, uint32_t **target_len, char err[256]) {
    if (err) err[0] = 0;
    if (!path || !n_targets || !target_name || !target_len) return GCE_ERR_INVALID;
    std::vector<std::string> names; std::vector<uint32_t> lens; std::string e;
    if (!gce_report::read_header(path, names, lens, e)) { if (err) { strncpy(err, e.c_str(), 255); err[255] = 0; } return GCE_ERR_INVALID; }
    const size_t n = names.size();
    *n_targets = (int32_t)n;
    *target_name = (char **)malloc(std::max<size_t>(n, 1) * sizeof(char *));
    *target_len = (uint32_t *)malloc(std::max<size_t>(n, 1) * sizeof(uint32_t));
    for (size_t k = 0; k < n; k++) { (*target_name)[k] = strdup(names[k].c_str()); (*target_len)[k] = lens[k]; }
    return GCE_OK;
}

void gce_bam_header_free(int32_t n_targets, char **target_name, uint32_t *target_len) {
    if (target_name) { for (int32_t k = 0; k < n_targets; k++) free(target_name[k]); free(target_name); }
    free(target_len);
}

}  // extern "C"
