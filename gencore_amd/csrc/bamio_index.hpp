// bamio_index.hpp -- the BAI index of a coordinate-sorted BAM: gce_bam_index (gce_bai.hpp).  A part of bamio.cpp.
#pragma once
#include "gce_entry.h"
#include "bamio_reader.hpp"

extern "C" {

int gce_bam_index(const char *bam_path, const char *bai_path, int32_t device, int threads, uint64_t window_bytes, gce_bai_run *out, char err[256]) {
    set_err(err, "");
    if (!bam_path || !bai_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    const double t_start = now_s();
    InputFile in;
    if (const char *verb = in.open(bam_path)) { set_err(err, (std::string("cannot ") + verb + " the BAM file").c_str()); return GCE_ERR_INVALID; }
    const int fd = in.fd; const uint64_t fsz = in.fsz;
    const std::string tmp = std::string(bai_path) + ".tmp" + std::to_string((long long)getpid());
    gce_bai *b = nullptr; FILE *fo = nullptr;
    auto done = [&](int code, const char *m) {
        set_err(err, m);
        if (b) gce_bai_destroy(b);
        if (fo) { fclose(fo); fo = nullptr; }
        if (code != GCE_OK) unlink(tmp.c_str());
        return code;
    };
    if (!in.is_bgzf()) return done(GCE_ERR_INVALID, "not a BGZF file");
    const int T = threads > 0 ? threads : default_threads();
    // ---- the header: the host inflates the first members (1 MB pieces) until it is whole
    uint64_t hdr_end = 0; int32_t n_ref = 0;
    {
        PassReader rh; BamHeader bh; const char *why = "";
        if (read_stream_header(rh, in, T, window_bytes, bh, &why) != HeaderRead::Complete) return done(GCE_ERR_INVALID, why);
        hdr_end = bh.hdr_end; n_ref = (int32_t)bh.n_ref;
    }
    out->n_ref = n_ref;
    int rc = gce_bai_create(device, &b);
    if (rc != GCE_OK) return done(rc, "no HIP device");
    // ---- the file from its first byte, window by window: the host reads and finds the members, the GPU inflates and indexes them
    PassReader rd; rd.fd = fd; rd.fsz = fsz; rd.T = T; rd.piece = window_bytes > 0 ? (size_t)window_bytes : ((size_t)64 << 20);
    uint64_t eod = 0;
    double read_s = 0, gpu_s = 0;
    std::string wmsg;
    rc = for_each_window(rd, hdr_end, &read_s, &gpu_s, wmsg, [&](PassReader &r, uint64_t, uint64_t sk) {
        const uint64_t file_base = r.at - r.have;
        for (const Block &k : r.blocks) if (k.usize) eod = (file_base + k.coff + k.csize) << 16;      // rule V: just past the last non-empty member
        return gce_bai_window(b, r.comp.data(), r.used, (int32_t)r.blocks.size(), r.z_coff.data(), r.z_csize.data(), r.z_usize.data(), file_base, sk, n_ref, r.last_piece() ? 1 : 0);
    });
    if (rc != GCE_OK) return done(rc, wmsg.empty() ? gce_bai_error(b) : wmsg.c_str());
    double t0 = now_s();
    int64_t counts[5] = {0, 0, 0, 0, 0}, bad = -1; int32_t kind = 0;
    if ((rc = gce_bai_finish(b, n_ref, eod, counts, &bad, &kind)) != GCE_OK) return done(rc, gce_bai_error(b));
    gpu_s += now_s() - t0;
    if (bad >= 0) {
        static const char *why[3] = {"is out of coordinate order (records must come in (tid, pos) order, unplaced ones last)", "ends beyond 2^29, the range of a BAI index",
                                     "names a contig the header does not have"};
        char m[256]; snprintf(m, sizeof m, "BAM record %lld (counting from 0) %s", (long long)bad, why[kind < 3 ? kind : 0]);
        return done(GCE_ERR_INVALID, m);
    }
    t0 = now_s();
    uint8_t *bytes = nullptr; size_t nbytes = 0;
    if ((rc = gce_bai_serialise(b, n_ref, &bytes, &nbytes)) != GCE_OK) return done(rc, "out of host memory");
    fo = fopen(tmp.c_str(), "wb");
    const bool wrote = fo && fwrite(bytes, 1, nbytes, fo) == nbytes;
    free(bytes);
    if (!wrote) return done(GCE_ERR_INVALID, "cannot write the index file");
    const bool closed = fclose(fo) == 0; fo = nullptr;
    if (!closed || rename(tmp.c_str(), bai_path) != 0) return done(GCE_ERR_INVALID, "cannot write the index file");
    out->write_s = now_s() - t0;
    out->n_records = counts[0]; out->n_no_coor = counts[1]; out->n_bins = counts[2]; out->n_chunks = counts[3]; out->n_intervals = counts[4];
    out->read_s = read_s; out->gpu_s = gpu_s;
    out->total_s = now_s() - t_start;
    return done(GCE_OK, "");
}

}  // extern "C"
