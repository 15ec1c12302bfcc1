// bamio_sort.hpp -- an unsorted BAM, or SAM text, into coordinate order: gce_bam_sort, gce_sam_sort and gce_bam_sort_passes (gce_sort.hpp;
// DESIGN.md 4d, 4e), over SortJob, which the calmd runners (bamio_calmd.hpp) use too.  A part of bamio.cpp.
#pragma once
#include <memory>
#include "gce_entry.h"
#include "bamio_reader.hpp"
#include "bamio_writer.hpp"

namespace {

// rule H: the header text (up to its first NUL) with SO:coordinate in its @HD line
std::string sort_header_text(const uint8_t *t, size_t l_text) {
    std::string text((const char *)t, strnlen((const char *)t, l_text));
    if (text.compare(0, 3, "@HD") != 0) return "@HD\tVN:1.6\tSO:coordinate\n" + text;
    size_t eol = text.find('\n'); if (eol == std::string::npos) eol = text.size();
    const size_t so = text.find("\tSO:");
    if (so == std::string::npos || so >= eol) { text.insert(eol, "\tSO:coordinate"); return text; }
    size_t ve = text.find('\t', so + 4); if (ve == std::string::npos || ve > eol) ve = eol;
    text.replace(so + 4, ve - (so + 4), "coordinate");
    return text;
}

// what gce_bam_sort and gce_bam_sort_passes share: the input's checks and header (rule H), the file streamed window by window, the output
// (rule F: the header in members of its own, the record stream in members of 0xff00 bytes, the EOF marker) under a temporary name
struct SortJob {
    InputFile in; std::string tmp, msg; bool tmp_made = false;
    gce_sort *b = nullptr; PassWriter pw; Pinned hb;
    int T = 1, level = 0; int32_t device = 0, codes = -1, n_ref = 0; uint64_t window_bytes = 0, hdr_end = 0, piece = 0;
    std::vector<uint8_t> hdr;
    const char *who = "gce_bam_sort"; bool keep_header = false; std::vector<std::string> names;   // gce_bam_calmd: the header byte for byte, its contig names kept
    int fail(int code, const std::string &m) { msg = m; return code; }
    // everything is let go; a failed call leaves no output
    void close_all(int code) {
        if (b) { gce_sort_destroy(b); b = nullptr; }
        pw.out.drop();
        if (code != GCE_OK && tmp_made) unlink(tmp.c_str());
        in.close();
    }
    // the input opened, the temporary name made, an output that is the input refused.  who: the entry point; what: the input's kind
    int open_paths(const char *in_path, const char *out_path, const char *who, const char *what) {
        if (const char *verb = in.open(in_path)) return fail(GCE_ERR_INVALID, std::string("cannot ") + verb + " the input " + what);
        tmp = std::string(out_path) + ".tmp" + std::to_string((long long)getpid());
        {   // the output may not be the input (by name or by file)
            struct stat so;
            bool same = stat(out_path, &so) == 0 && so.st_dev == in.st.st_dev && so.st_ino == in.st.st_ino;
            char *ri = realpath(in_path, nullptr), *ro = realpath(out_path, nullptr);
            if (ri && ro && strcmp(ri, ro) == 0) same = true;
            free(ri); free(ro);
            if (same) return fail(GCE_ERR_INVALID, std::string("the output path is the input file: ") + who + (keep_header ? " does not rewrite a file in place" : " does not sort in place"));
        }
        return GCE_OK;
    }
    int open_input(const char *in_path, const char *out_path, int threads, int lv, uint64_t wb, int32_t dev) {
        level = lv; window_bytes = wb; device = dev;
        { const int rc = open_paths(in_path, out_path, who, "BAM"); if (rc != GCE_OK) return rc; }
        if (in.fsz > 0 && !(in.fsz >= 4 && looks_gzip(in.fd, in.fsz))) return fail(GCE_ERR_INVALID, std::string(who) + " reads BAM, not SAM text");
        if (!in.is_bgzf()) return fail(GCE_ERR_INVALID, "not a BGZF file");
        T = threads > 0 ? threads : default_threads();
        // ---- the header: the host inflates the first members (1 MB pieces) until it is whole
        PassReader rh; BamHeader bh; const char *why = "";
        if (read_stream_header(rh, in, T, window_bytes, bh, &why, keep_header ? &names : nullptr) != HeaderRead::Complete) return fail(GCE_ERR_INVALID, why);
        const uint8_t *u = rh.win.p;
        hdr_end = bh.hdr_end; n_ref = (int32_t)bh.n_ref;
        if (keep_header) { hdr.assign(u, u + bh.hdr_end); return GCE_OK; }
        const std::string text = sort_header_text(u + bh.text_off, bh.l_text);                // rule H: the text rewritten, the contig table as it is
        const uint32_t lt = (uint32_t)text.size();
        hdr.assign(u, u + 4); hdr.insert(hdr.end(), (const uint8_t *)&lt, (const uint8_t *)&lt + 4);
        hdr.insert(hdr.end(), text.begin(), text.end()); hdr.insert(hdr.end(), u + bh.text_off + bh.l_text, u + bh.hdr_end);
        return GCE_OK;
    }
    // the file from its first byte, window by window: the host reads and finds the members, window(rd, skip, est) hands them to the GPU.
    // est: the whole file's inflated bytes, from the ISIZE totals so far and the file size.  read_s / gpu_s: the two sides' seconds, added to.
    template <class F> int stream(double *read_s, double *gpu_s, F &&window) {
        PassReader rd; rd.fd = in.fd; rd.fsz = in.fsz; rd.T = T; rd.piece = window_bytes > 0 ? (size_t)window_bytes : ((size_t)64 << 20);
        uint64_t comp_seen = 0, infl_seen = 0;
        msg.clear();
        const int rc = for_each_window(rd, hdr_end, read_s, gpu_s, msg, [&](PassReader &r, uint64_t u_all, uint64_t sk) {
            comp_seen += r.used; infl_seen += u_all;
            return window(r, sk, comp_seen ? (uint64_t)((double)infl_seen * ((double)in.fsz / (double)comp_seen)) : 0);
        });
        return rc != GCE_OK && msg.empty() ? fail(rc, gce_sort_error(b)) : rc;
    }
    // The output comes back in pieces that are multiples of 0xff00: 8192 members when the GPU deflates them (one lane per member), 1024 when
    // the host threads do
    void set_pieces() { codes = level == -3 ? 1 : level == -2 ? 0 : -1; piece = PassWriter::BS * (codes >= 0 ? 8192 : 1024); }
    // the pinned buffer one piece of a write_range call of up to `largest` bytes comes back in
    int host_room(uint64_t largest) {
        const size_t pmax = (size_t)std::min<uint64_t>(piece, largest), hcap = codes >= 0 ? pmax + pmax / 8 + 64 * (pmax / PassWriter::BS + 2) : pmax;
        if (largest && !hb.ensure(hcap)) return fail(GCE_ERR_OOM, "out of pinned host memory");
        return GCE_OK;
    }
    // the temporary file with the header's members; largest: the most bytes one write_range call will be asked for
    int begin_output(uint64_t largest) {
        { const int rc = host_room(largest); if (rc != GCE_OK) return rc; }
        pw.level = level; pw.T = T; pw.device = device;
        if (!pw.out.reserve()) return fail(GCE_ERR_OOM, "out of host memory");
        if (!pw.out.open(tmp.c_str(), false)) return fail(GCE_ERR_INVALID, "cannot write the output BAM");
        tmp_made = true;
        if (!pw.out.header_members(hdr, level, codes >= 0, T)) return fail(GCE_ERR_INVALID, "cannot write the output BAM");
        return GCE_OK;
    }
    // the first n bytes gce_sort_read has to give, piece by piece, as members of 0xff00 bytes
    int write_range(uint64_t n) {
        for (uint64_t o = 0; o < n; o += piece) {
            const size_t nb = (size_t)std::min<uint64_t>(piece, n - o); size_t got = 0;
            const int rc = gce_sort_read(b, o, nb, codes, hb.p, hb.cap, &got);
            if (rc != GCE_OK) return fail(rc, gce_sort_error(b));
            if (!(codes >= 0 ? pw.out.write(hb.p, got) : pw.out.members(hb.p, got, level, T))) return fail(GCE_ERR_INVALID, "cannot write the output BAM");
        }
        return GCE_OK;
    }
    int end_output(const char *out_path, int64_t *out_bytes) {
        if (!pw.close()) return fail(GCE_ERR_INVALID, "cannot write the output BAM");
        { struct stat so; *out_bytes = stat(tmp.c_str(), &so) == 0 ? (int64_t)so.st_size : 0; }
        if (rename(tmp.c_str(), out_path) != 0) return fail(GCE_ERR_INVALID, "cannot write the output BAM");
        return GCE_OK;
    }
};

}  // namespace

extern "C" {

int gce_bam_sort(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes, gce_sort_run *out, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    if (level < -3 || level > 9) { set_err(err, "level should be -3, -2, -1 or 0..9"); return GCE_ERR_INVALID; }
    const double t_start = now_s();
    SortJob j;
    auto done = [&](int code) { j.close_all(code); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    out->n_ref = n_ref;
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, device_budget_bytes, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    // ---- the file from its first byte, window by window: the host reads and finds the members, the GPU inflates, indexes and keys them
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est); });
    if (rc != GCE_OK) return done(rc);
    // ---- sort, scan, gather
    j.set_pieces();
    int64_t counts[3] = {0, 0, 0}, bad = -1; uint64_t total = 0; double times[2] = {0, 0};
    if ((rc = gce_sort_finish(j.b, n_ref, j.codes, j.piece, counts, &bad, &total, times)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    if (bad >= 0) {
        char m[256]; snprintf(m, sizeof m, "BAM record %lld (counting from 0) names a contig the header does not have", (long long)bad);
        return done(j.fail(GCE_ERR_INVALID, m));
    }
    out->sort_s = times[0]; out->gather_s = times[1];
    out->n_records = counts[0]; out->n_no_coor = counts[1]; out->n_descents = counts[2]; out->inflated_bytes = (int64_t)total;
    // ---- rule F
    const double t0 = now_s();
    if ((rc = j.begin_output(total)) != GCE_OK || (rc = j.write_range(total)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

// SAM text in any order into the coordinate-sorted BAM, file to file.  Replaces: gce_sam_to_bam (host threads, the whole text
// and the whole record stream in host memory, a BAM written and read again) in front of gce_bam_sort -- what `samtools sort` does with an
// aligner's SAM output in front of the reference.  The text is read in windows cut at their last line feed; the `@` lines make the header as
// gce_sam_to_bam makes it, then rule H; the alignment lines become records on the GPU (gce_sort_sam_window), behind the resident ones; from
// there on it is gce_bam_sort.
int gce_sam_sort(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes, gce_sort_run *out, int64_t *n_host_lines,
                 char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !out || !n_host_lines) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out); *n_host_lines = 0;
    if (level < -3 || level > 9) { set_err(err, "level should be -3, -2, -1 or 0..9"); return GCE_ERR_INVALID; }
    const double t_start = now_s();
    SortJob j;
    auto done = [&](int code) { j.close_all(code); set_err(err, j.msg.c_str()); return code; };
    j.level = level; j.device = device; j.window_bytes = window_bytes; j.T = threads > 0 ? threads : default_threads();
    int rc = j.open_paths(in_path, out_path, "gce_sam_sort", "SAM");
    if (rc != GCE_OK) return done(rc);
    if (looks_gzip(j.in.fd, j.in.fsz)) return done(j.fail(GCE_ERR_INVALID, "gce_sam_sort reads SAM text, not BAM"));
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, device_budget_bytes, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    const uint64_t W = window_bytes ? std::min<uint64_t>(window_bytes, (uint64_t)1 << 30) : ((uint64_t)64 << 20), LONGEST = (uint64_t)256 << 20;
    std::unique_ptr<Pinned> buf(new Pinned());                                       // the window: what the last one left over, then the next piece of the file
    uint64_t have = 0, at = 0, base = 0, text_seen = 0, rec_bytes = 0;                              // base: the file offset of buf[0]
    bool in_header = true; std::string text; std::vector<std::string> names; std::vector<uint32_t> lens; int32_t n_ref = 0;
    // the line that starts at file offset `o`, counting from 1 over the file (an error's path only: the file is read once more up to there)
    auto line_number = [&](uint64_t o) {
        long long ln = 1; std::vector<char> pb((size_t)1 << 20);
        for (uint64_t a = 0; a < o;) { const ssize_t g = pread(j.in.fd, pb.data(), (size_t)std::min<uint64_t>(pb.size(), o - a), (off_t)a); if (g <= 0) break; ln += (long long)std::count(pb.data(), pb.data() + g, '\n'); a += (uint64_t)g; }
        return ln;
    };
    for (bool last = j.in.fsz == 0; ;) {
        double t0 = now_s();
        if (!last) {
            const uint64_t want = std::min<uint64_t>(W, j.in.fsz - at);
            if (have + want + 64 > buf->cap) {
                std::unique_ptr<Pinned> nb(new Pinned());
                if (!nb->ensure((size_t)(have + want + 64))) return done(j.fail(GCE_ERR_OOM, "out of pinned host memory"));
                if (have) memcpy(nb->p, buf->p, (size_t)have);
                buf.swap(nb);
            }
            if (pread_full(j.in.fd, buf->p + have, (size_t)want, at) != (size_t)want) return done(j.fail(GCE_ERR_INVALID, "cannot read the input SAM"));
            have += want; at += want; last = at >= j.in.fsz;
        }
        const char *cur = (const char *)buf->p;
        uint64_t lim = have;
        if (!last) {
            const char *nl = have ? (const char *)memrchr(cur, '\n', (size_t)have) : nullptr;
            lim = nl ? (uint64_t)(nl - cur) + 1 : 0;
            if (!nl && have > LONGEST) return done(j.fail(GCE_ERR_INVALID, "SAM line longer than 256 MB"));
        }
        out->read_s += now_s() - t0;
        uint64_t p = 0;
        if (in_header) {
            while (p < lim && cur[p] == '@') { const char *q = (const char *)memchr(cur + p, '\n', (size_t)(lim - p)); const uint64_t z = q ? (uint64_t)(q - cur) + 1 : lim; text.append(cur + p, (size_t)(z - p)); if (!q) text.push_back('\n'); p = z; }
            if (p < lim || last) {
                in_header = false;
                if (!samtext::parse_header_text(text, names, lens)) return done(j.fail(GCE_ERR_INVALID, "bad @SQ line"));
                n_ref = (int32_t)lens.size(); out->n_ref = n_ref; j.n_ref = n_ref;
                const std::string ht = sort_header_text((const uint8_t *)text.data(), text.size());      // rule H
                j.hdr = bam_header_bytes(ht, names, lens);
                std::vector<const char *> np; for (const std::string &x : names) np.push_back(x.c_str());
                if ((rc = gce_sort_sam_contigs(j.b, n_ref, np.data())) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
            }
        }
        if (!in_header && p < lim) {
            // the whole file's record bytes, from the records the text so far gave (the first window: unknown, the buffers hold just that window)
            const uint64_t est = text_seen ? (uint64_t)((double)rec_bytes * ((double)j.in.fsz / (double)text_seen)) : 0;
            text_seen += lim - p;
            int64_t bad = -1; uint64_t bad_start = 0; double ps = 0;
            rc = gce_sort_sam_window(j.b, cur + p, (size_t)(lim - p), n_ref, est, n_host_lines, &bad, &bad_start, &ps, &rec_bytes);
            out->inflate_index_s += ps;                                              // (the parse kernels and the host patch; the copy of the text, the buffers' growth and k_sort_keys are in total_s only)
            if (rc != GCE_OK) {
                std::string m = gce_sort_error(j.b);
                if (bad >= 0) m += " (line " + std::to_string(line_number(base + p + bad_start)) + ")";
                return done(j.fail(rc, m));
            }
        }
        if (lim) { if (lim < have) memmove(buf->p, buf->p + lim, (size_t)(have - lim)); have -= lim; base += lim; }
        if (last) break;
    }
    buf.reset();
    // ---- sort, scan, gather: gce_bam_sort from here on
    j.set_pieces();
    int64_t counts[3] = {0, 0, 0}, bad = -1; uint64_t total = 0; double times[2] = {0, 0};
    if ((rc = gce_sort_finish(j.b, n_ref, j.codes, j.piece, counts, &bad, &total, times)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    if (bad >= 0) return done(j.fail(GCE_ERR_INVALID, "a record names a contig the header does not have"));
    out->sort_s = times[0]; out->gather_s = times[1];
    out->n_records = counts[0]; out->n_no_coor = counts[1]; out->n_descents = counts[2]; out->inflated_bytes = (int64_t)total;
    const double t0 = now_s();
    if ((rc = j.begin_output(total)) != GCE_OK || (rc = j.write_range(total)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

// gce_bam_sort for a file of any size: in-core when that fits the budget, otherwise in output-range passes: a key pass
// (gce_sort_key_window), the plan (gce_sort_plan), then per pass the file once more (gce_sort_pass_*) and that range of the output written.
int gce_bam_sort_passes(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes, int32_t min_passes,
                        gce_sort_run *out, gce_sort_pass_run *run, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !out || !run || min_passes < 0 || min_passes > 64) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out); memset(run, 0, sizeof *run);
    if (level < -3 || level > 9) { set_err(err, "level should be -3, -2, -1 or 0..9"); return GCE_ERR_INVALID; }
    const double t_start = now_s();
    uint64_t budget = device_budget_bytes;
    if (!budget) {
        size_t fr = 0, tot = 0;
        const int r0 = gce_device_mem_info(device, &fr, &tot);
        if (r0 != GCE_OK) { set_err(err, "no HIP device"); return r0; }
        budget = std::max<uint64_t>((uint64_t)((double)fr * GCE_PASS_BUDGET_FRACTION), 1);
    }
    const uint64_t M = PassWriter::BS;
    // ---- in-core first, unless passes are forced or even the compressed file is beyond half the budget (in-core holds the inflated records twice)
    if (min_passes <= 1) {
        struct stat sf;
        const bool hopeless = stat(in_path, &sf) == 0 && sf.st_size > 0 && (uint64_t)sf.st_size > budget / 2;
        if (!hopeless) {
            const int r1 = gce_bam_sort(in_path, out_path, device, threads, level, window_bytes, (size_t)budget, out, err);
            if (r1 != GCE_ERR_OOM) {
                if (r1 == GCE_OK) {
                    const uint64_t total = (uint64_t)out->inflated_bytes;
                    run->in_core = 1; run->pass_bytes = (int64_t)((total + M - 1) / M * M); run->n_passes = total ? 1 : 0; run->resident_bytes = out->peak_device_bytes;
                    run->pass_s[0] = out->sort_s + out->gather_s + out->write_s;
                }
                return r1;
            }
            set_err(err, ""); memset(out, 0, sizeof *out);                                 // (GCE_ERR_OOM leaves no output)
        }
    }
    SortJob j;
    auto done = [&](int code) { j.close_all(code); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    out->n_ref = n_ref;
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, (size_t)budget, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    // ---- the key pass: key and size of every record
    double t0 = now_s();
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_key_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est); });
    if (rc != GCE_OK) return done(rc);
    run->key_pass_s = now_s() - t0;
    // ---- the plan: the order, every record's destination, the cuts
    j.set_pieces();
    int64_t counts[3] = {0, 0, 0}, bad = -1; uint64_t total = 0, pass_bytes = 0, resident = 0; int32_t P = 0;
    if ((rc = gce_sort_plan(j.b, n_ref, j.codes, j.piece, min_passes, counts, &bad, &total, &P, &pass_bytes, &resident, &run->plan_s)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    if (bad >= 0) {
        char m[256]; snprintf(m, sizeof m, "BAM record %lld (counting from 0) names a contig the header does not have", (long long)bad);
        return done(j.fail(GCE_ERR_INVALID, m));
    }
    out->sort_s = run->plan_s;
    out->n_records = counts[0]; out->n_no_coor = counts[1]; out->n_descents = counts[2]; out->inflated_bytes = (int64_t)total;
    run->n_passes = P; run->pass_bytes = (int64_t)pass_bytes; run->resident_bytes = (int64_t)resident;
    // ---- rule F, one output range per pass: the member layout is the in-core sort's, because pass_bytes is a multiple of 0xff00
    if ((rc = j.begin_output(pass_bytes)) != GCE_OK) return done(rc);
    for (int32_t k = 0; k < P; k++) {
        t0 = now_s();
        const uint64_t lo = (uint64_t)k * pass_bytes, hi = std::min<uint64_t>(lo + pass_bytes, total);
        if ((rc = gce_sort_pass_begin(j.b, lo, hi)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
        rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t) {
            return gce_sort_pass_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0); });
        if (rc != GCE_OK) return done(rc);
        double sc = 0;
        if ((rc = gce_sort_pass_end(j.b, &sc)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
        out->gather_s += sc; out->inflate_index_s -= sc;
        const double tw = now_s();
        if ((rc = j.write_range(hi - lo)) != GCE_OK) return done(rc);
        out->write_s += now_s() - tw;
        run->pass_s[k] = now_s() - t0;
    }
    t0 = now_s();
    if ((rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s += now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

}  // extern "C"
