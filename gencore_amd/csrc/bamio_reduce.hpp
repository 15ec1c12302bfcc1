// bamio_reduce.hpp -- the runner of a windowed reduce pass (gce_reduce.hpp): what gce_bam_pileup (bamio_pileup.hpp) and gce_bam_error_profile
// (bamio_errprof.hpp) do around their device objects, in the shape of gce_bam_index: checks, header, BED, FASTA, window loop, finish, table.  A
// part of bamio.cpp.
#pragma once
#include "gce_entry.h"
#include "bamio_reader.hpp"
#include "bamio_varmask.hpp"

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

// what the frame has learned of the input when it hands over to the pass: the header's contigs, the BED as rule S's intervals (has_bed: one was
// given), the FASTA (fa: NULL without one, or once the pass has let it go) with each contig's bases and length, NULL / -1 for one it lacks
struct ReduceInput {
    int32_t n_ref = 0; std::vector<std::string> names; std::vector<uint32_t> lens;
    bool has_bed = false; PileSites ps;
    gce_fasta *fa = nullptr; std::vector<const char *> seq; std::vector<int64_t> slen;
};

// The variant mask of a run (rule K and rule Y of DESIGN.md 4m), for the passes that take one: a pass with a member `MaskJob mk` has it loaded
// behind the header and the FASTA (on: the entry point is a masked one; path and out are then its arguments) and sets it in its set()
struct MaskJob {
    bool on = false; const char *path = nullptr; gce_mask_run *out = nullptr;
    gce_mask m{};
    // the intervals through the pass's set_mask, at least once, so that an empty mask is a mask; fill_s: the seconds of it
    template <class SET> int fill(SET &&set_mask) {
        const double t0 = now_s();
        const int rc = set_mask(m.n_intervals, m.tid, m.start, m.end);
        out->fill_s += now_s() - t0;
        return rc;
    }
    // class 21 of a block of counters, summed
    static int64_t events(const uint64_t *counts) {
        int64_t n = 0;
        for (size_t r = 0; r < (size_t)3 * GCE_ERRPROF_MAX_CYCLE; r++) n += (int64_t)counts[r * GCE_ERRPROF_CLASSES + 21];
        return n;
    }
};
template <class P> auto mask_job(P &ps, int) -> decltype(&ps.mk) { return &ps.mk; }
template <class P> MaskJob *mask_job(P &, long) { return nullptr; }

// One run of a reduce pass over a BAM file.  PASS is the entry point's own part:
//   who, option, options_known the entry point's name, its option bits, and what the refusal of any other says of them
//   bed_first                  the BED is the required file and checked first, the FASTA optional (else the other way round)
//   out                        its gce_*_run: read_s, inflate_index_s, write_s, total_s and peak_device_bytes are the frame's to fill
//   zero(), sites(in)          out as a call starts; what out says of the BED
//   create, window, error, destroy, free_out   the entry points of its device object p (gce_entry.h) and the free of its gce_*_run; create is called on
//                              the pass, so one whose object takes more than the common arguments (gce_errsup's tags) has a member function
//   set(in), pass_s()          p set up in front of the first window; where out keeps the seconds of the pass's kernels
//   alloc(in), finish()         out's arrays; the counters into out
//   table(in, to_file, emit)   rule O: the table through emit(buf), a piece or all at once; to_file: there is a file to write
//   mk (optional)              a MaskJob: with mk.on the mask file is checked with the other files, loaded behind the FASTA and freed by the frame
template <class PASS> int reduce_run(PASS &ps, const char *bam_path, const char *bed_path, const char *fasta_path, const char *tsv_path, int32_t device, int threads, int32_t min_mapq,
                                     int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, char err[256]) {
    set_err(err, "");
    MaskJob *mj = mask_job(ps, 0);
    if (mj && !mj->on) mj = nullptr;
    if (!bam_path || !(PASS::bed_first ? bed_path : fasta_path) || !ps.out || (mj && (!mj->path || !mj->out))) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    ps.zero();
    if (mj) memset(mj->out, 0, sizeof *mj->out);
    auto *out = ps.out;
    if (min_mapq < 0 || min_mapq > 255) { set_err(err, "min_mapq should be 0..255"); return GCE_ERR_INVALID; }
    if (min_baseq < 0 || min_baseq > 255) { set_err(err, "min_baseq should be 0..255"); return GCE_ERR_INVALID; }
    if (options & ~PASS::option) { set_err(err, (std::string("unknown option bit (") + PASS::options_known + ")").c_str()); return GCE_ERR_INVALID; }
    for (const bool bed : {PASS::bed_first, !PASS::bed_first}) {
        const char *path = bed ? bed_path : fasta_path;
        struct stat sf;
        if (path && (stat(path, &sf) != 0 || S_ISDIR(sf.st_mode))) { set_err(err, bed ? "cannot open the BED file" : "cannot open the reference FASTA"); return GCE_ERR_INVALID; }
    }
    if (mj) {
        struct stat sf;
        if (stat(mj->path, &sf) != 0 || S_ISDIR(sf.st_mode)) { set_err(err, "cannot open the variant mask"); return GCE_ERR_INVALID; }
        if (!mask_kind(mj->path)) { set_err(err, GCE_MASK_NAME_REFUSAL); return GCE_ERR_INVALID; }
    }
    const double t_start = now_s();
    InputFile in;
    if (const char *verb = in.open(bam_path)) { set_err(err, (std::string("cannot ") + verb + " the BAM file").c_str()); return GCE_ERR_INVALID; }
    const std::string tmp = tsv_path ? std::string(tsv_path) + ".tmp" + std::to_string((long long)getpid()) : std::string();
    ReduceInput ri; FILE *fo = nullptr;
    auto done = [&](int code, const char *m) {
        set_err(err, m);                                                              // (m may be the device object's: copied before it goes)
        if (ps.p) PASS::destroy(ps.p);
        if (ri.fa) gce_fasta_free(ri.fa);
        if (mj) gce_mask_free(&mj->m);
        if (fo) { fclose(fo); fo = nullptr; }
        if (code != GCE_OK) { if (tsv_path) unlink(tmp.c_str()); PASS::free_out(out); }
        return code;
    };
    if (in.fsz > 0 && !(in.fsz >= 4 && looks_gzip(in.fd, in.fsz))) return done(GCE_ERR_INVALID, (std::string(PASS::who) + " reads BAM, not SAM text").c_str());
    if (!in.is_bgzf()) return done(GCE_ERR_INVALID, "not a BGZF file");
    const int T = threads > 0 ? threads : default_threads();
    // ---- the header: the host inflates the first members (1 MB pieces) until it is whole
    uint64_t hdr_end = 0;
    {
        PassReader rh; BamHeader bh; const char *why = "";
        if (read_stream_header(rh, in, T, window_bytes, bh, &why, &ri.names, &ri.lens) != HeaderRead::Complete) return done(GCE_ERR_INVALID, why);
        hdr_end = bh.hdr_end; ri.n_ref = (int32_t)bh.n_ref;
    }
    const int32_t n_ref = ri.n_ref;
    // ---- rule S: the BED against the header's names
    if (bed_path) {
        std::vector<const char *> np; for (const std::string &s : ri.names) np.push_back(s.c_str());
        int32_t n_reg = 0, *rt = nullptr, *rs = nullptr, *re = nullptr;
        if (gce_bed_load(bed_path, n_ref, np.data(), &n_reg, &rt, &rs, &re, nullptr) != GCE_OK) return done(GCE_ERR_INVALID, "cannot read the BED file");
        const bool fits = pile_sites(n_reg, rt, rs, re, ri.lens, ri.ps);
        gce_bed_free(n_reg, rt, rs, re, nullptr);
        if (!fits) return done(GCE_ERR_INVALID, "more than 2^28 sites in the BED file");
        ri.has_bed = true;
        ps.sites(ri);
    }
    // ---- the contigs by the header's names, as calmd matches them; the bases stay on the host
    ri.seq.assign((size_t)n_ref, nullptr); ri.slen.assign((size_t)n_ref, -1);
    double t0 = now_s();
    if (fasta_path) {
        if (gce_fasta_load(fasta_path, T, &ri.fa) != GCE_OK) return done(GCE_ERR_INVALID, "cannot read the reference FASTA");
        match_contigs(ri.names, ri.fa, ri.seq, ri.slen);
    }
    out->read_s += now_s() - t0;
    // ---- rule K: the mask against the header's names, clamped to min(header length, FASTA length)
    if (mj) {
        t0 = now_s();
        std::vector<const char *> np; for (const std::string &s : ri.names) np.push_back(s.c_str());
        std::vector<int64_t> ml((size_t)n_ref);
        for (int32_t t = 0; t < n_ref; t++) ml[(size_t)t] = std::min<int64_t>(ri.slen[(size_t)t], (int64_t)ri.lens[(size_t)t]);
        char why[256];
        const int mrc = gce_mask_load(mj->path, n_ref, np.data(), ml.data(), T, &mj->m, why);
        if (mrc != GCE_OK) return done(mrc, why);
        gce_mask_run *mo = mj->out;
        mo->n_lines = mj->m.n_lines; mo->n_records = mj->m.n_records; mo->n_unknown_contig = mj->m.n_unknown_contig; mo->n_no_alt = mj->m.n_no_alt;
        mo->n_intervals = mj->m.n_intervals; mo->n_masked_bases = mj->m.n_masked_bases;
        mo->load_s = now_s() - t0;
    }
    (void)gce_device_bytes(nullptr, nullptr, 1);
    int rc = ps.create(device, device_budget_bytes, min_mapq, min_baseq, exclude_flags, options, &ps.p);
    if (rc != GCE_OK) return done(rc, "no HIP device");
    if ((rc = ps.set(ri)) != GCE_OK) return done(rc, PASS::error(ps.p));
    // ---- the file from its first byte, window by window: the host reads and finds the members, the GPU inflates, indexes and counts them
    PassReader rd; rd.fd = in.fd; rd.fsz = in.fsz; rd.T = T; rd.piece = window_bytes > 0 ? (size_t)window_bytes : ((size_t)64 << 20);
    double gpu_s = 0;
    std::string wmsg;
    rc = for_each_window(rd, hdr_end, &out->read_s, &gpu_s, wmsg, [&](PassReader &r, uint64_t, uint64_t sk) {
        return PASS::window(ps.p, r.comp.data(), r.used, (int32_t)r.blocks.size(), r.z_coff.data(), r.z_csize.data(), r.z_usize.data(), sk, n_ref, r.last_piece() ? 1 : 0, ps.pass_s());
    });
    if (rc != GCE_OK) return done(rc, wmsg.empty() ? PASS::error(ps.p) : wmsg.c_str());
    if (!ps.alloc(ri)) return done(GCE_ERR_OOM, "out of host memory for the counters");
    t0 = now_s();
    if ((rc = ps.finish()) != GCE_OK) return done(rc, PASS::error(ps.p));
    gpu_s += now_s() - t0;
    out->inflate_index_s = gpu_s - *ps.pass_s();
    // ---- rule O: the table, to a temporary name, renamed at the end
    t0 = now_s();
    auto emit = [&](const std::string &buf) {
        if (!tsv_path) return true;
        if (!fo && !(fo = fopen(tmp.c_str(), "wb"))) return false;
        return fwrite(buf.data(), 1, buf.size(), fo) == buf.size();
    };
    bool ok = ps.table(ri, tsv_path != nullptr, emit);
    if (tsv_path) {
        ok = ok && emit(std::string());
        const bool closed = fo && fclose(fo) == 0; fo = nullptr;
        if (!ok || !closed || rename(tmp.c_str(), tsv_path) != 0) return done(GCE_ERR_INVALID, "cannot write the table");
    }
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK, "");
}

}  // namespace
