// bamio_varmask.hpp -- the variant mask of the error profile, read on the host: gce_mask_load (rule K of DESIGN.md 4m).  A part of bamio.cpp,
// host only like gce_bed_load and gce_fasta_load; reduce_run (bamio_reduce.hpp) calls it for the masked entry points and hands the
// intervals to the pass's set_mask (gce_varmask.hpp).
//
// A `.vcf` / `.vcf.gz` is read as a stream, 1 MiB of inflated text at a time (zlib's gz reader takes plain gzip and BGZF alike and goes on
// over any number of members), through a per-byte state machine that keeps the first five fields of the line it is in and nothing else: a
// line of a multi-sample file may be as long as it likes, and a member boundary may cut it anywhere.  A `.bed` goes through gce_bed_load.
#pragma once
#include <zlib.h>
#include "bamio_common.hpp"

namespace {

// rule K's VCF half: text in, pieces at a time, records out through rec(chrom, pos, ref_len, alt); false: a refusal, its words in why
struct VcfLines {
    int64_t n_lines = 0;
    std::string f[5]; int nf = 0; bool any = false, comment = false, cr = false;     // the line so far: fields 0..4, tabs seen, a byte seen, begins with '#', a CR is held back
    std::string why;
    void put(char c) {
        if (!any) { any = true; comment = c == '#'; }
        if (comment) return;
        if (c == '\t') nf++;
        else if (nf < 5) f[nf] += c;
    }
    template <class REC> bool feed(const char *p, size_t n, REC &&rec) {
        for (size_t k = 0; k < n; k++) {
            const char c = p[k];
            if (c == '\n') { if (!end_line(rec)) return false; continue; }
            if (cr) { cr = false; put('\r'); }                                        // (a CR in front of anything but the line feed is text)
            if (c == '\r') { any = true; cr = true; } else put(c);
        }
        return true;
    }
    template <class REC> bool finish(REC &&rec) { return !any || end_line(rec); }     // the last line may lack its line feed
    template <class REC> bool end_line(REC &&rec) {
        n_lines++;
        const bool record = any && !comment && !(nf == 0 && f[0].empty());
        bool ok = true;
        if (record) {
            uint64_t pos = 0; bool digits = !f[1].empty();
            for (const char d : f[1]) { if (d < '0' || d > '9') { digits = false; break; } if (pos < (1ull << 40)) pos = pos * 10 + (uint64_t)(d - '0'); }
            if (nf < 4) ok = refuse("fewer than five tab-separated fields");
            else if (!digits || pos < 1) ok = refuse("POS is not a decimal integer >= 1");
            else if (f[3].empty()) ok = refuse("REF is empty");
            else rec(f[0], pos, (uint64_t)f[3].size(), f[4]);
        }
        for (std::string &x : f) x.clear();
        nf = 0; any = comment = cr = false;
        return ok;
    }
    bool refuse(const char *what) { why = "variant mask line " + std::to_string((long long)n_lines) + ": " + what; return false; }
};

inline bool ends_with(const std::string &s, const char *e) { const size_t n = strlen(e); return s.size() >= n && s.compare(s.size() - n, n, e) == 0; }
// what a mask file's name says it is: 'v' VCF text, 'z' gzip or BGZF of it, 'b' BED, 0 none of them
inline char mask_kind(const char *path) {
    const std::string s(path);
    return ends_with(s, ".vcf.gz") ? 'z' : ends_with(s, ".vcf") ? 'v' : ends_with(s, ".bed") ? 'b' : 0;
}
#define GCE_MASK_NAME_REFUSAL "the variant mask should be a file whose name ends in .vcf, .vcf.gz or .bed"

}  // namespace

extern "C" {

void gce_mask_free(gce_mask *m) {
    if (!m) return;
    free(m->tid); free(m->start); free(m->end);
    m->tid = m->start = m->end = nullptr;
}

int gce_mask_load(const char *path, int32_t n_ref, const char *const *names, const int64_t *lens, int threads, gce_mask *out, char err[256]) {
    (void)threads;
    set_err(err, "");
    if (out) memset(out, 0, sizeof *out);
    if (!path || !out || n_ref < 0 || (n_ref && (!names || !lens))) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    const char kind = mask_kind(path);
    if (!kind) { set_err(err, GCE_MASK_NAME_REFUSAL); return GCE_ERR_INVALID; }
    struct R { int32_t tid; int64_t a, z; };
    std::vector<R> v;
    auto keep = [&](int32_t t, int64_t a, int64_t z) {                                // clamped to [0, lens[t]); nothing where there is no reference base
        const int64_t len = std::min<int64_t>(lens[t], 0x7FFFFFFF);
        a = std::max<int64_t>(a, 0); z = std::min(z, len);
        if (a < z) v.push_back({t, a, z});
    };
    if (kind == 'b') {
        int32_t n_reg = 0, *rt = nullptr, *rs = nullptr, *re = nullptr;
        if (gce_bed_load(path, n_ref, names, &n_reg, &rt, &rs, &re, nullptr) != GCE_OK) { set_err(err, "cannot read the variant mask"); return GCE_ERR_INVALID; }
        for (int32_t k = 0; k < n_reg; k++) {
            out->n_records++;
            if (rt[k] < 0 || rt[k] >= n_ref) out->n_unknown_contig++; else keep(rt[k], rs[k], re[k]);
        }
        gce_bed_free(n_reg, rt, rs, re, nullptr);
    } else {
        std::unordered_map<std::string, int32_t> by_name;
        for (int32_t t = 0; t < n_ref; t++) if (names[t]) by_name[names[t]] = t;      // (the last of a repeated name, as gce_bed_load)
        VcfLines L;
        auto rec = [&](const std::string &chrom, uint64_t pos, uint64_t ref_len, const std::string &alt) {
            out->n_records++;
            const auto it = by_name.find(chrom);
            if (it == by_name.end()) { out->n_unknown_contig++; return; }
            if (alt == "." || alt == "<NON_REF>" || alt == "<*>") { out->n_no_alt++; return; }
            keep(it->second, (int64_t)pos - 1, (int64_t)(pos - 1 + ref_len));
        };
        std::vector<char> buf((size_t)1 << 20);
        bool ok = true, read_ok = true;
        if (kind == 'z') {
            gzFile g = gzopen(path, "rb");
            if (!g) { set_err(err, "cannot open the variant mask"); return GCE_ERR_INVALID; }
            for (;;) {
                const int got = gzread(g, buf.data(), (unsigned)buf.size());
                if (got < 0) { read_ok = false; break; }
                if (got == 0) break;
                if (!(ok = L.feed(buf.data(), (size_t)got, rec))) break;
            }
            // a member cut short gives the bytes it has and then 0, never a negative count: the error shows in gzerror and gzclose alone
            int zerr = Z_OK;
            (void)gzerror(g, &zerr);
            const int closed = gzclose(g);
            if (ok && ((zerr != Z_OK && zerr != Z_STREAM_END) || closed != Z_OK)) read_ok = false;
        } else {
            FILE *fi = fopen(path, "rb");
            if (!fi) { set_err(err, "cannot open the variant mask"); return GCE_ERR_INVALID; }
            for (;;) {
                const size_t got = fread(buf.data(), 1, buf.size(), fi);
                if (got == 0) { read_ok = !ferror(fi); break; }
                if (!(ok = L.feed(buf.data(), got, rec))) break;
            }
            fclose(fi);
        }
        if (ok && read_ok) ok = L.finish(rec);
        if (!read_ok || !ok) {
            const std::string why = !read_ok ? std::string("cannot inflate the variant mask") : L.why;
            memset(out, 0, sizeof *out);
            set_err(err, why.c_str());
            return GCE_ERR_INVALID;
        }
        out->n_lines = L.n_lines;
    }
    // ---- sorted by (tid, start), merged where they overlap or abut, as rule S merges (without pile_sites' cap on the sites)
    std::sort(v.begin(), v.end(), [](const R &x, const R &y) { return x.tid != y.tid ? x.tid < y.tid : x.a != y.a ? x.a < y.a : x.z < y.z; });
    size_t m = 0;
    for (const R &r : v) {
        if (m && v[m - 1].tid == r.tid && r.a <= v[m - 1].z) { v[m - 1].z = std::max(v[m - 1].z, r.z); continue; }
        v[m++] = r;
    }
    out->tid = (int32_t *)malloc(std::max<size_t>(m, 1) * 4); out->start = (int32_t *)malloc(std::max<size_t>(m, 1) * 4); out->end = (int32_t *)malloc(std::max<size_t>(m, 1) * 4);
    if (!out->tid || !out->start || !out->end) { gce_mask_free(out); memset(out, 0, sizeof *out); set_err(err, "out of host memory for the variant mask"); return GCE_ERR_OOM; }
    for (size_t k = 0; k < m; k++) {
        out->tid[k] = v[k].tid; out->start[k] = (int32_t)v[k].a; out->end[k] = (int32_t)v[k].z;
        out->n_masked_bases += v[k].z - v[k].a;
    }
    out->n_intervals = (int64_t)m;
    return GCE_OK;
}

}  // extern "C"
