// bamio_run.hpp -- the consensus runners, file to file: gce_run_bam and its sharded and depth forms over the streaming pipeline (BamRun), and the
// whole-file host-codec runners of round 2 (GCE_BAM_HOSTCODEC=1).  A part of bamio.cpp, included behind its whole-file reader and writer
// (gce_bam, bam_chunk_impl, bam_write_rows), which the host-codec runners use.
#pragma once
#include "bamio_common.hpp"
#include "gce_fileout.hpp"

namespace {

// Replaces Gencore::consensus() end to end (src/gencore.cpp:162-293) as a PIPELINE with a bounded host footprint: a reader thread preads the
// file in pieces; the host threads inflate the BGZF blocks of piece k (own decoder + CLMUL CRC) into a pinned window while the DMA engine
// copies window k - 1 into HBM; nothing of the input stays on the host.  Records are indexed, parsed (gce_raw_finish) and -- after
// gce_process -- re-assembled as BAM records (gce_raw_build_output) on the GPU; the output stream comes back in pieces that are deflated by
// all host threads and written in order while the next piece is on its way.  Host memory: two compressed pieces, three inflated windows,
// three output pieces -- independent of the file's size (round 2 held the whole inflated file and every record table on the host).
// gce_run_bam (n_shards == 1) and gce_run_bam_sharded over the same pipeline: with several shards every piece of the file goes to one engine per
// entry of `devices` (the mirrors of the first), each inflates and indexes the stream on its own GPU, plans it there and keeps its share
// (gce_raw_select_shard); the record streams are merged on the first engine's device (gce_raw_merge_outputs) and written as one.
//
// BamRun is one such run: what its stages share, and the stages in the order run() calls them.  A stage returns a status and, when that is
// not GCE_OK, leaves its words in msg; whatever the run holds when it ends, however it ends, the destructor lets go.
struct BamRun {
    const char *const fasta_path; const int threads, level; gce_bam_run *const out; const int32_t n_shards; const int32_t *const devices; const int32_t plan_mode;
    const char *const bed_path; const int32_t coverage_step; gce_depth_run *const depth;
    const double t_start = now_s();
    const int T;
    const size_t PIECE;                                 // compressed bytes per window (tests shrink it through chunk_reads)
    // GCE_BAM_HOST_INFLATE=1: the BGZF members are inflated by the host threads (the path of the first half of round 3); default: they go to
    // HBM compressed and the GPU inflates them (gce_raw_push_bgzf) -- the host inflates only the window(s) that hold the BAM header
    const bool gpu_inflate = getenv("GCE_BAM_HOST_INFLATE") == nullptr;
    const bool tlap = getenv("GCE_RAW_TIMING") != nullptr; double tl0 = 0;
    InputFile in;
    gce_engine *e = nullptr; gce_fasta *fa = nullptr; OutFile of;
    std::vector<gce_engine *> mir;                      // the engines of shards 1 .. n_shards - 1 (they receive every push made to e)
    std::thread reader; ssize_t got_next = 0; bool reader_on = false;      // feed_bam's read-ahead of the next piece (start_read); the destructor joins it
    Pinned comp[2]; int32_t comp_ticket[2] = {-1, -1};
    Pinned win[3]; int32_t win_ticket[3] = {-1, -1, -1};
    Pinned obuf[2];                                     // write_output's pieces
    uint64_t file_off = 0; double t_read = 0, t_inflate = 0, t_wait = 0, t0 = 0;
    std::vector<std::string> names; std::vector<uint32_t> lens; std::string text;       // the contig table and the header text
    uint64_t hdr_end = 0; bool have_header = false;
    gce_params prm;
    int64_t n_rec = 0; uint64_t body = 0; int64_t n_out = 0;
    std::string msg;

    BamRun(const char *fasta_path, const gce_params *params, int threads, int64_t chunk_reads, int level, gce_bam_run *out, int32_t n_shards, const int32_t *devices, int32_t plan_mode,
           const char *bed_path, int32_t coverage_step, gce_depth_run *depth)
        : fasta_path(fasta_path), threads(threads), level(level), out(out), n_shards(n_shards), devices(devices), plan_mode(plan_mode), bed_path(bed_path), coverage_step(coverage_step),
          depth(depth), T(threads > 0 ? threads : default_threads()), PIECE((size_t)(chunk_reads > 0 && chunk_reads < (1 << 16) ? (1 << 20) : (8 << 20))), prm(*params) {}
    BamRun(const BamRun &) = delete; BamRun &operator=(const BamRun &) = delete;
    ~BamRun() {
        if (reader_on) { reader.join(); reader_on = false; }
        for (auto *x : mir) if (x) gce_destroy(x);
        if (e) gce_destroy(e);
        if (fa) gce_fasta_free(fa);
        of.drop();
    }
    int fail(int code, const char *m) { msg = m ? m : ""; return code; }
    void lap(const char *what) { if (tlap) { const double x = now_s(); fprintf(stderr, "gce_run_bam %s %.4f s\n", what, x - tl0); tl0 = x; } }
    // wait for a window's or a piece's copy into HBM, if one is under way
    int wait_ticket(int32_t &ticket) {
        if (ticket < 0) return GCE_OK;
        const double w0 = now_s();
        const int rc = gce_submit_wait(e, ticket);
        if (rc != GCE_OK) return fail(rc, gce_last_error(e));
        t_wait += now_s() - w0; ticket = -1;
        return GCE_OK;
    }
    std::vector<gce_engine *> engines() const { std::vector<gce_engine *> all; all.push_back(e); for (auto *x : mir) all.push_back(x); return all; }

    int open_input(const char *in_path) {
        if (const char *verb = in.open(in_path)) return fail(GCE_ERR_INVALID, (std::string("cannot ") + verb + " the input BAM").c_str());
        tl0 = now_s();
        if (!comp[0].ensure(PIECE + (1 << 17)) || !comp[1].ensure(PIECE + (1 << 17))) return fail(GCE_ERR_OOM, "out of pinned host memory");
        lap("compressed-piece buffers");
        return GCE_OK;
    }
    // the contig table is known (BAM header / SAM header lines): engine, reference, raw stream.  first_qname: the first record's name or NULL
    int setup_engine(const char *first_qname, size_t capacity) {
        have_header = true;
        file_params(prm, (int32_t)lens.size(), lens.data(), first_qname);
        if (getenv("GCE_RAW_TIMING")) fprintf(stderr, "gce_run_bam: RSS before gce_create %ld MB (entry %ld MB)\n", status_kb("VmRSS:") >> 10, (long)(out->rss_start_kb >> 10));
        lap("up to the header");
        int r2;
        if (devices) prm.device = devices[0];
        // One host thread per engine: gce_create, the reference, and the raw stream's buffers (gce_raw_begin: a few GB of hipMalloc per engine, 0.15 s per GB on a
        // fresh process -- the four engines of a sharded run, set up one after the other, were 0.4 - 1.7 s of "input pipeline" on some boxes) side by side; on a
        // multi-GPU node every device allocates for itself.  The FASTA file is read once, in front.
        if (fasta_path && *fasta_path && (r2 = gce_fasta_load(fasta_path, threads, &fa)) != GCE_OK) return fail(r2, "cannot read the FASTA file");
        std::vector<gce_engine *> made((size_t)std::max(n_shards, 1), nullptr);
        std::vector<int> rcs((size_t)made.size(), GCE_OK); std::vector<std::string> msgs(made.size());
        auto setup = [&](int32_t r) {
            gce_params pr = prm; if (devices) pr.device = devices[r];
            gce_engine *x = nullptr; int c2;
            if ((c2 = gce_create(&pr, &x)) != GCE_OK) { rcs[(size_t)r] = c2; msgs[(size_t)r] = gce_status_message(c2); return; }
            made[(size_t)r] = x;
            if (fa && (c2 = set_reference(x, fa, names.data(), lens.size())) != GCE_OK) { rcs[(size_t)r] = c2; msgs[(size_t)r] = gce_last_error(x); return; }
            if ((c2 = gce_raw_begin(x, capacity)) != GCE_OK) { rcs[(size_t)r] = c2; msgs[(size_t)r] = gce_last_error(x); }
        };
        if (made.size() == 1) setup(0);
        else { std::vector<std::thread> th; for (int32_t r = 0; r < n_shards; r++) th.emplace_back(setup, r); for (auto &t : th) t.join(); }
        e = made[0]; for (size_t r = 1; r < made.size(); r++) if (made[r]) mir.push_back(made[r]);       // (owned by the destructor from here on)
        if (fa) { gce_fasta_free(fa); fa = nullptr; }                                    // (packed in HBM: the host copy goes)
        for (size_t r = 0; r < made.size(); r++) if (rcs[r] != GCE_OK) return fail(rcs[r], msgs[r].c_str());
        lap("gce_create + reference + gce_raw_begin (a thread per engine)");
        for (gce_engine *x : mir) if ((r2 = gce_raw_attach_mirror(e, x)) != GCE_OK) return fail(r2, gce_last_error(x));
        return GCE_OK;
    }

    // ---- SAM text input.  sam_open(in, "r") takes either format (src/gencore.cpp:164): a file that does not start with the gzip magic is SAM text.
    // Pieces of the text are cut at line feeds; the '@' lines in front give the header text and the contig table; alignment lines become BAM
    // records on all host threads (gce_samtext.hpp) in a pinned window that goes to HBM like an inflated BAM window, behind BAM header bytes
    // made from the SAM header: from there on the stream is the one a BAM file gives.
    int feed_sam() {
        const uint64_t fsz = in.fsz; int rc;
        Raw<char> tbuf[2]; uint64_t at = 0; bool in_header = true; samtext::NameMap nmap; int wk = 0, kb = 0;
        std::vector<std::vector<uint8_t>> parts; std::vector<std::string> perr;
        const size_t TP = PIECE < ((size_t)8 << 20) ? PIECE : ((size_t)64 << 20);          // text bytes per piece (tests: 1 MB pieces that cut lines)
        ssize_t rd_got = 0;
        auto read_into = [&](char *dst, size_t want, uint64_t off) { const double r0 = now_s(); rd_got = (ssize_t)pread_full(in.fd, dst, want, off); t_read += now_s() - r0; };
        struct ReadAhead { std::thread t; bool on = false; void join() { if (on) { t.join(); on = false; } } ~ReadAhead() { join(); } } rd;      // (a stage that fails waits for its read)
        size_t n = 0;                                                                      // bytes in tbuf[kb]: what the last piece left over + this piece
        {
            const size_t want = (size_t)std::min<uint64_t>(TP, fsz);
            tbuf[0].resize(want + 1); if (!tbuf[0].ok()) return fail(GCE_ERR_OOM, "out of host memory");
            read_into(tbuf[0].data(), want, 0);
            if ((size_t)rd_got != want) return fail(GCE_ERR_INVALID, "cannot read the input SAM");
            at = want; n = want;
        }
        for (;;) {
            char *cur = tbuf[kb].data();
            const bool last = at >= fsz;
            size_t lim = n;
            if (!last) {
                const char *nl = (const char *)memrchr(cur, '\n', n);
                lim = nl ? (size_t)(nl - cur) + 1 : 0;
                if (!nl && n > ((size_t)256 << 20)) return fail(GCE_ERR_INVALID, "SAM line longer than 256 MB");
            } else if (n && cur[n - 1] != '\n') { cur[n] = '\n'; lim = n + 1; }
            // the next piece is read behind what this one leaves over (the line its end cut) while this one is converted
            size_t want2 = 0, left = lim >= n ? 0 : n - lim;
            if (!last) {
                want2 = (size_t)std::min<uint64_t>(TP, fsz - at);
                Raw<char> &nx = tbuf[kb ^ 1];
                nx.resize(left + want2 + 1); if (!nx.ok()) return fail(GCE_ERR_OOM, "out of host memory");
                if (left) memcpy(nx.data(), cur + lim, left);
                char *dst = nx.data() + left; const uint64_t off = at;
                rd.on = true; rd.t = std::thread([&, dst, off, want2] { read_into(dst, want2, off); });
                at += want2;
            }
            size_t p = 0;
            if (in_header) {
                while (p < lim && cur[p] == '@') { const char *q = (const char *)memchr(cur + p, '\n', lim - p); const size_t z2 = (size_t)(q - cur) + 1; text.append(cur + p, z2 - p); p = z2; }
                if (p < lim || last) {
                    in_header = false;
                    if (!samtext::parse_header_text(text, names, lens) || lens.empty()) return fail(GCE_ERR_INVALID, "this SAM file has no header");      // src/gencore.cpp:186-189
                    nmap.build(names);
                    std::string fq;
                    if (p < lim) { const char *q = cur + p; const char *t = (const char *)memchr(q, '\t', lim - p); if (t) fq.assign(q, t); }
                    if ((rc = setup_engine(fq.empty() ? nullptr : fq.c_str(), (size_t)std::max<uint64_t>(fsz + (1u << 20), 1u << 20))) != GCE_OK) return rc;
                    const std::vector<uint8_t> hb = bam_header_bytes(text, names, lens);
                    hdr_end = hb.size();
                    int32_t tk; if ((rc = gce_raw_push(e, hb.data(), hb.size(), &tk)) != GCE_OK || (rc = gce_submit_wait(e, tk)) != GCE_OK) return fail(rc, gce_last_error(e));
                }
            }
            if (!in_header && p < lim) {
                const double i0 = now_s();
                if (const char *m = lines_to_records(cur, p, lim, T, nmap, parts, perr)) return fail(GCE_ERR_INVALID, m);
                size_t tot = 0; std::vector<size_t> po((size_t)T + 1, 0);
                for (int t = 0; t < T; t++) { po[(size_t)t] = tot; tot += parts[(size_t)t].size(); }
                if (tot) {
                    const int ws = wk % 3;
                    if ((rc = wait_ticket(win_ticket[ws])) != GCE_OK) return rc;
                    if (!win[ws].ensure(tot + 64)) return fail(GCE_ERR_OOM, "out of pinned host memory");
                    parallel_for(T, T, [&](int, int64_t a, int64_t b2) { for (int64_t t = a; t < b2; t++) if (!parts[(size_t)t].empty()) memcpy(win[ws].p + po[(size_t)t], parts[(size_t)t].data(), parts[(size_t)t].size()); });
                    if ((rc = gce_raw_push(e, win[ws].p, tot, &win_ticket[ws])) != GCE_OK) return fail(rc, gce_last_error(e));
                    wk++;
                }
                t_inflate += now_s() - i0;                                                 // (lines -> records: reported where a BAM input reports its inflate)
            }
            if (last) break;
            rd.join();
            if ((size_t)rd_got != want2) return fail(GCE_ERR_INVALID, "cannot read the input SAM");
            n = left + want2; kb ^= 1;
        }
        return GCE_OK;
    }

    // ---- BAM input
    // reader: piece k of the file into comp[k & 1] behind the carry-over of piece k - 1 (a BGZF block cut by the piece border)
    void start_read(int slot, size_t keep) {
        const uint64_t at = file_off; const size_t want = (size_t)std::min<uint64_t>(PIECE, in.fsz - at);
        reader_on = true;
        reader = std::thread([this, slot, keep, at, want] {                                 // the piece in up to four parts, read side by side (one pread stream copies ~7 GB/s out of the page cache)
            const double r0 = now_s();
            static const size_t RP = getenv("GCE_READ_PARTS") ? (size_t)atoi(getenv("GCE_READ_PARTS")) : 4;
            const int R = (int)std::max<size_t>(1, std::min<size_t>({RP, (size_t)T, want >> 20}));
            std::vector<size_t> done_(R, 0); std::vector<std::thread> sub;
            auto part = [&](int r) { const size_t a = want * (size_t)r / R, z2 = want * (size_t)(r + 1) / R; done_[r] = pread_full(in.fd, comp[slot].p + keep + a, z2 - a, at + a); };
            for (int r = 1; r < R; r++) sub.emplace_back(part, r);
            part(0);
            for (auto &t : sub) t.join();
            size_t o = 0; for (int r = 0; r < R; r++) { const size_t a = want * (size_t)r / R, z2 = want * (size_t)(r + 1) / R; o += done_[r]; if (done_[r] != z2 - a) break; }      // (bytes in order up to the first short part)
            got_next = (ssize_t)o; t_read += now_s() - r0; });
        file_off += want;
    }
    // the read-ahead's piece behind the carry-over: the bytes now in the other compressed buffer (0: the file is through)
    size_t next_piece(size_t carry) { if (!reader_on) return 0; reader.join(); reader_on = false; return carry + (size_t)got_next; }
    // This loop reads the header itself, not through read_bam_header: the header's window is inflated, and the next piece read, while the
    // one before is on its way to HBM, and the windows inflated up to the header go to the engine as they are.
    int feed_bam() {
        const uint64_t fsz = in.fsz; int rc;
        std::vector<Block> blocks; std::vector<uint64_t> z_coff; std::vector<uint32_t> z_csize, z_usize;
        Raw<uint8_t> head;                              // the inflated start of the stream until the header is complete (usually one window)
        int k = 0;
        size_t have = 0;                                // bytes in comp[k & 1]: carry + piece
        if (fsz) { start_read(0, 0); have = next_piece(0); }
        while (have > 0) {
            const int cs = k & 1, ws = k % 3;
            uint8_t *z = comp[cs].p;
            // ---- BGZF members of this piece
            blocks.clear();
            size_t off = 0; uint64_t uoff = 0;
            for (Member m;;) {
                const Scan sc = scan_member(z, have, off, m);
                if (sc == Scan::More) break;                                                // cut by the piece border: carried over
                if (sc != Scan::Member) return fail(GCE_ERR_INVALID, scan_message(sc));
                blocks.push_back(Block{off, m.bsize, m.isize, uoff}); off += m.bsize; uoff += m.isize;
            }
            const bool last = file_off >= fsz;
            if (last && off != have) return fail(GCE_ERR_INVALID, "truncated BGZF block at the end of the file");
            if (!last && blocks.empty()) return fail(GCE_ERR_INVALID, "BGZF block larger than a window");
            // ---- the next piece is read while this one is inflated
            const size_t carry = have - off;
            if (!last) {
                if ((rc = wait_ticket(comp_ticket[cs ^ 1])) != GCE_OK) return rc;          // (its members are in HBM)
                memcpy(comp[cs ^ 1].p, z + off, carry); start_read(cs ^ 1, carry);
            }
            if (have_header && gpu_inflate) {                                               // this piece's members: to HBM as they are
                z_coff.clear(); z_csize.clear(); z_usize.clear();
                for (const Block &bk : blocks) { z_coff.push_back(bk.coff); z_csize.push_back(bk.csize); z_usize.push_back(bk.usize); }
                if ((rc = gce_raw_push_bgzf(e, z, off, (int32_t)blocks.size(), z_coff.data(), z_csize.data(), z_usize.data(), &comp_ticket[cs])) != GCE_OK) return fail(rc, gce_last_error(e));
                have = next_piece(carry);
                k++;
                continue;
            }
            if ((rc = wait_ticket(win_ticket[ws])) != GCE_OK) return rc;
            if (!win[ws].ensure((size_t)uoff + 64)) return fail(GCE_ERR_OOM, "out of pinned host memory");
            const double i0 = now_s();
            std::atomic<int> bad{0};
            parallel_for(T, (int64_t)blocks.size(), [&](int, int64_t a, int64_t b2) { for (int64_t q = a; q < b2; q++) if (blocks[q].usize && !inflate_block(z + blocks[q].coff, blocks[q], win[ws].p + blocks[q].uoff)) bad = 1; });
            t_inflate += now_s() - i0;
            if (bad) return fail(GCE_ERR_INVALID, "inflate / CRC failure");
            // ---- header (first window(s)), engine, reference
            if (!have_header) {
                const size_t old = head.size();
                Raw<uint8_t> h2; h2.resize(old + (size_t)uoff + 1); if (!h2.ok()) return fail(GCE_ERR_OOM, "out of host memory");
                if (old) memcpy(h2.data(), head.data(), old);
                memcpy(h2.data() + old, win[ws].p, (size_t)uoff); h2.n = old + (size_t)uoff; head = std::move(h2);
                const uint8_t *u = head.data(); const uint64_t n = head.size();
                BamHeader bh;
                const Hdr hs = n >= 12 ? parse_bam_header(u, n, Contigs::Collect, bh, &names, &lens) : Hdr::Incomplete;      // (this runner looks at the magic only once 12 bytes are there)
                if (hs == Hdr::NotBam) return fail(GCE_ERR_INVALID, "not a BAM stream");
                const bool complete = hs == Hdr::Complete;
                if (complete && lens.empty()) return fail(GCE_ERR_INVALID, "this SAM file has no header");      // src/gencore.cpp:186-189 (n_targets == 0), as the SAM-text branch does
                if (complete) { hdr_end = bh.hdr_end; text.assign((const char *)u + bh.text_off, bh.l_text); }
                if (!complete && last) return fail(GCE_ERR_INVALID, "truncated header");
                if (complete) {
                    const char *fq = nullptr;                                                 // src/gencore.cpp:207-220: the first record's name
                    if (hdr_end + 36 < n) { const uint32_t lq = u[hdr_end + 12]; if (hdr_end + 36 + lq <= n) fq = (const char *)u + hdr_end + 36; }
                    if ((rc = setup_engine(fq, (size_t)std::max<uint64_t>(fsz * 5, head.size()))) != GCE_OK) return rc;
                    // what was inflated so far goes up in one piece (normally: this very window)
                    if (old) { int32_t tk; if ((rc = gce_raw_push(e, head.data(), old, &tk)) != GCE_OK || (rc = gce_submit_wait(e, tk)) != GCE_OK) return fail(rc, gce_last_error(e)); }
                    head.release();
                    lap("gce_raw_begin + first push");
                }
            }
            if (have_header && uoff && (rc = gce_raw_push(e, win[ws].p, (size_t)uoff, &win_ticket[ws])) != GCE_OK) return fail(rc, gce_last_error(e));
            have = next_piece(carry);
            k++;
        }
        return GCE_OK;
    }
    // the input is through: the header must have been, the input stages' seconds
    int input_done() {
        if (!have_header) return fail(GCE_ERR_INVALID, in.fsz ? "truncated header" : "empty file");
        lap("rest of the input loop");
        out->read_s = t_read; out->inflate_s = t_inflate; out->submit_s = t_wait;
        out->open_s = now_s() - t_start;
        if (getenv("GCE_RAW_TIMING")) fprintf(stderr, "gce_run_bam: RSS after the input pipeline %ld MB\n", status_kb("VmRSS:") >> 10);
        t0 = now_s();
        return GCE_OK;
    }

    // ---- the depth statistics of the report (Options::coverageStep, Options::bedFile; stats.cpp:56-83, bed.cpp:64-79): every engine adds up its own reads and
    //      records on its GPU right behind its run -- BEFORE the merge adds the other engines' Stats blocks into the first one's -- (gce_stats_payload_device)
    int depth_begin() {
        if (!depth) return GCE_OK;
        int rc;
        memset(depth, 0, sizeof *depth);
        if (coverage_step <= 0) return fail(GCE_ERR_INVALID, "coverage_step must be positive");
        if (bed_path && *bed_path) {
            std::vector<const char *> np; for (auto &x : names) np.push_back(x.c_str());
            if ((rc = gce_bed_load(bed_path, (int32_t)np.size(), np.data(), &depth->n_regions, &depth->region_tid, &depth->region_start, &depth->region_end, nullptr)) != GCE_OK) return fail(rc, "cannot read the BED file");
        }
        if (!depth_alloc(depth, lens, coverage_step)) return fail(GCE_ERR_OOM, "out of host memory");
        return GCE_OK;
    }
    int engine_payload(gce_engine *x) {
        if (!depth) return GCE_OK;
        const int64_t *pay = nullptr; gce_payload_layout lay;
        return gce_stats_payload_device(x, coverage_step, depth->n_regions, depth->region_tid, depth->region_start, depth->region_end, &pay, &lay);
    }
    // the engines' payloads (each computed on its own Stats blocks) summed in device memory, to the host once
    int depth_payload() {
        if (!depth || n_rec <= 0) return GCE_OK;
        int rc;
        std::vector<gce_engine *> all = engines();
        const int64_t *pay = nullptr; gce_payload_layout lay;
        if ((rc = gce_stats_payload_sum(all.data(), (int32_t)all.size(), &pay, &lay)) != GCE_OK) return fail(rc, gce_last_error(e));
        std::vector<int64_t> host((size_t)lay.total_words);
        if ((rc = gce_stats_payload_read(e, pay, lay.total_words, host.data())) != GCE_OK) return fail(rc, gce_last_error(e));
        if (lay.n_bins != depth->n_bins || lay.n_regions != depth->n_regions) return fail(GCE_ERR_INVALID, "payload layout");
        depth_unpack(depth, host.data(), lay.stats_words);
        return GCE_OK;
    }

    int compute_one() {
        int rc;
        if ((rc = gce_raw_finish(e, hdr_end, prm.n_targets, &n_rec)) != GCE_OK) return fail(rc, gce_last_error(e));
        out->index_s = now_s() - t0; t0 = now_s();
        if (n_rec > 0) {
            if ((rc = gce_process(e)) != GCE_OK) return fail(rc, gce_last_error(e)[0] ? gce_last_error(e) : gce_status_message(rc));
            out->process_s = now_s() - t0; t0 = now_s();
            gce_timing tm; if (gce_get_timing(e, &tm) == GCE_OK) out->kernel_ms = tm.total_ms;
            gce_result res;
            if ((rc = gce_result_device(e, &res)) != GCE_OK) return fail(rc, gce_last_error(e));
            out->n_reads = res.n_reads; out->n_out = res.n_out; out->pre = res.pre; out->post = res.post;
            if ((rc = gce_raw_build_output(e, &body, &n_out)) != GCE_OK) return fail(rc, gce_last_error(e));
            if ((rc = engine_payload(e)) != GCE_OK) return fail(rc, gce_last_error(e));
            out->drain_s = now_s() - t0; t0 = now_s();
            if (getenv("GCE_RAW_TIMING")) fprintf(stderr, "gce_run_bam: RSS after process + output records %ld MB\n", status_kb("VmRSS:") >> 10);
        }
        return GCE_OK;
    }
    // several engines: each indexes the stream it received, keeps its shard, runs it and assembles its records -- side by side, one host
    // thread per engine, nothing exchanged; then the streams are merged on the first engine's device
    int compute_shards() {
        int rc;
        std::vector<gce_engine *> all = engines();
        std::vector<int> rcs((size_t)n_shards, GCE_OK); std::vector<std::string> msgs((size_t)n_shards); std::vector<int64_t> nrec((size_t)n_shards, 0); std::vector<double> kms((size_t)n_shards, 0.0), t_idx((size_t)n_shards, 0.0);
        std::vector<std::thread> th;
        for (int32_t r = 0; r < n_shards; r++) th.emplace_back([&, r] {
            gce_engine *x = all[(size_t)r]; int c2; int64_t n0 = 0; uint64_t b2 = 0; int64_t o2 = 0;
            auto failr = [&](int code) { rcs[(size_t)r] = code; const char *m = gce_last_error(x); msgs[(size_t)r] = m && m[0] ? m : gce_status_message(code); };
            const double a0 = now_s();
            if ((c2 = gce_raw_finish(x, hdr_end, prm.n_targets, &n0)) != GCE_OK) return failr(c2);
            if (n0 > 0 && (c2 = gce_raw_select_shard(x, n_shards, r, plan_mode)) != GCE_OK) return failr(c2);
            t_idx[(size_t)r] = now_s() - a0;
            gce_result rs;
            if (n0 > 0 && ((c2 = gce_process(x)) != GCE_OK || (c2 = gce_result_device(x, &rs)) != GCE_OK || (c2 = gce_raw_build_output(x, &b2, &o2)) != GCE_OK || (c2 = engine_payload(x)) != GCE_OK)) return failr(c2);
            gce_timing tm; if (n0 > 0 && gce_get_timing(x, &tm) == GCE_OK) kms[(size_t)r] = tm.total_ms;
            nrec[(size_t)r] = n0;
        });
        for (auto &t : th) t.join();
        for (int32_t r = 0; r < n_shards; r++) if (rcs[(size_t)r] != GCE_OK) return fail(rcs[(size_t)r], msgs[(size_t)r].c_str());
        for (int32_t r = 0; r < n_shards; r++) { out->kernel_ms = std::max(out->kernel_ms, kms[(size_t)r]); out->index_s = std::max(out->index_s, t_idx[(size_t)r]); }
        out->process_s = now_s() - t0 - out->index_s; t0 = now_s();
        n_rec = nrec[0];
        if (n_rec > 0) {
            if ((rc = gce_raw_merge_outputs(all.data(), n_shards, &body, &n_out, &out->pre, &out->post, &out->n_reads)) != GCE_OK) return fail(rc, gce_last_error(e));
            out->n_out = n_out;
        }
        out->drain_s = now_s() - t0; t0 = now_s();
        return GCE_OK;
    }

    // ---- the output file: its header, then a stream in HBM walked in pieces (pump_pieces), each piece handed to what writes it.  A name that ends
    //      in "sam" is written as SAM text (src/gencore.cpp:170-173: sam_open(out, "w")), any other as BGZF members.  Levels -2 / -3: the stream is what
    //      the GPU made of the records -- the lines (gce_samfmt.hpp) or the deflated file image (gce_deflate.hpp: -2 fixed Huffman codes, -3 the smallest
    //      of dynamic codes, fixed codes and stored per block) -- and the host only copies it out and writes it.  Other levels: the stream is the records,
    //      made into lines or, behind the header's bytes, deflated into members of 0xff00 bytes by all host threads.
    int write_output(const char *out_path) {
        int rc;
        const bool gpu_out = level == -2 || level == -3;
        if (!of.open(out_path, OutFile::named_sam(out_path))) return fail(GCE_ERR_INVALID, of.sam ? "cannot open the output SAM" : "cannot open the output BAM");
        const char *const cannot = of.sam ? "cannot write the output SAM" : "cannot write the output BAM";
        const char *why = "output piece";                                                      // what a walk that ends early says: a fetch's words, unless wait or sink put theirs
        const uint64_t SMALL = PIECE < ((size_t)8 << 20) ? ((uint64_t)64 << 10) : ((uint64_t)16 << 20);   // pieces of text and of records for lines (tests: small ones that cut records)
        auto records = [&](uint64_t o, uint8_t *dst, size_t n, int32_t *tk) { return gce_raw_read_output_async(e, o, dst, n, tk); };
        auto wait = [&](int32_t tk) { const int r = gce_submit_wait(e, tk); if (r != GCE_OK) why = gce_last_error(e); return r; };
        auto written = [&](bool ok) -> int { if (ok) return GCE_OK; why = cannot; return GCE_ERR_INVALID; };
        auto write = [&](const uint8_t *p, size_t n) { return written(of.write(p, n)); };
        if (of.sam) {
            if (!of.sam_header(text, names, lens)) return fail(GCE_ERR_INVALID, cannot);
            if (gpu_out) {
                uint64_t tb = 0;
                std::vector<const char *> np; for (auto &x : names) np.push_back(x.c_str());
                if (body && (rc = gce_raw_format_output(e, (int32_t)np.size(), np.data(), &tb)) != GCE_OK) return fail(rc, gce_last_error(e)[0] ? gce_last_error(e) : gce_status_message(rc));
                rc = pump_pieces(nullptr, 0, tb, SMALL, obuf, [&](uint64_t o, uint8_t *dst, size_t n, int32_t *tk) { return gce_raw_read_text_async(e, o, dst, n, tk); }, wait, write);
            } else {
                std::vector<uint8_t> cur; std::vector<uint64_t> ro; std::vector<std::string> lines;
                rc = pump_pieces(nullptr, 0, body, SMALL, obuf, records, wait, [&](const uint8_t *p, size_t n) -> int {
                    cur.insert(cur.end(), p, p + n);                                           // behind the record a piece border cut
                    const size_t o = whole_records(cur.data(), cur.size(), ro);
                    if (o == SIZE_MAX || !records_to_lines(cur.data(), ro, names, T, lines)) { why = "bad record in the output stream"; return GCE_ERR_INVALID; }
                    for (const std::string &L : lines) if (!of.write(L.data(), L.size())) return written(false);
                    cur.erase(cur.begin(), cur.begin() + (ptrdiff_t)o);
                    return GCE_OK;
                });
                if (rc == GCE_OK && !cur.empty()) { rc = GCE_ERR_INVALID; why = "truncated record at the end of the output stream"; }
            }
        } else {
            const std::vector<uint8_t> hdr = bam_header_bytes(text, names, lens);
            if (!of.reserve()) return fail(GCE_ERR_OOM, "out of host memory");
            if (gpu_out) {
                uint64_t cb = 0;
                if (!of.header_members(hdr, level, true, T)) return fail(GCE_ERR_INVALID, cannot);
                if (body && (rc = gce_raw_deflate_output_codes(e, level == -3 ? 1 : 0, &cb)) != GCE_OK) return fail(rc, gce_last_error(e));
                rc = pump_pieces(nullptr, 0, cb, (uint64_t)16 << 20, obuf, [&](uint64_t o, uint8_t *dst, size_t n, int32_t *tk) { return gce_raw_read_deflated_async(e, o, dst, n, tk); }, wait, write);
            } else rc = pump_pieces(hdr.data(), hdr.size(), body, ROUND_BYTES, obuf, records, wait, [&](const uint8_t *p, size_t n) { return written(of.members(p, n, level, T)); });
        }
        if (rc != GCE_OK) return fail(rc, why);
        if (!of.close()) return fail(GCE_ERR_INVALID, cannot);
        out->write_s = now_s() - t0;
        out->total_s = now_s() - t_start;
        out->peak_rss_kb = status_kb("VmHWM:"); out->rss_end_kb = status_kb("VmRSS:");
        return GCE_OK;
    }

    int run(const char *in_path, const char *out_path) {
        int rc;
        if ((rc = open_input(in_path)) != GCE_OK) return rc;
        if ((rc = in.is_sam() ? feed_sam() : feed_bam()) != GCE_OK || (rc = input_done()) != GCE_OK) return rc;
        if ((rc = depth_begin()) != GCE_OK) return rc;
        if ((rc = n_shards > 1 ? compute_shards() : compute_one()) != GCE_OK) return rc;
        if ((rc = depth_payload()) != GCE_OK) return rc;
        return write_output(out_path);
    }
};

int run_bam_impl(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int threads, int64_t chunk_reads, int level, gce_bam_run *out,
                 char err[256], int32_t n_shards, const int32_t *devices, int32_t plan_mode, const char *bed_path = nullptr, int32_t coverage_step = 0, gce_depth_run *depth = nullptr) {
    set_err(err, "");
    if (!in_path || !out_path || !params || !out) return GCE_ERR_INVALID;
    memset(out, 0, sizeof *out);
    out->rss_start_kb = status_kb("VmRSS:");
    BamRun run(fasta_path, params, threads, chunk_reads, level, out, n_shards, devices, plan_mode, bed_path, coverage_step, depth);
    const int rc = run.run(in_path, out_path);
    set_err(err, run.msg.c_str());
    return rc;
}

}  // namespace

extern "C" {

// Gencore::consensus() for a sorted BAM (src/gencore.cpp:162-293) through the C-ABI.
// The whole-file path of round 2 (gce_bam_open: everything inflated and indexed on the host, struct-of-arrays chunks, gce_bam_write): kept as
// gce_run_bam_hostcodec for callers that want the host codec end to end and as the fallback of gce_run_bam.
int gce_run_bam_hostcodec(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int threads,
                int64_t chunk_reads, int level, gce_bam_run *out, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !params || !out) return GCE_ERR_INVALID;
    memset(out, 0, sizeof *out);
    const double t_start = now_s();
    gce_bam *f = nullptr; gce_engine *e = nullptr; gce_fasta *fa = nullptr;
    int rc = gce_bam_open(in_path, threads, &f);
    auto done = [&](int code, const char *m) { set_err(err, m); if (e) gce_destroy(e); if (f) gce_bam_close(f); if (fa) gce_fasta_free(fa); return code; };
    if (rc != GCE_OK) return done(rc, f ? gce_bam_error(f) : "open failed");
    out->open_s = now_s() - t_start;
    gce_bam_info bi; gce_bam_get_info(f, &bi);
    out->read_s = bi.read_s; out->inflate_s = bi.inflate_s; out->index_s = bi.index_s;
    gce_params prm = *params;
    gce_batch one;
    file_params(prm, bi.n_targets, bi.target_len, umi_auto(prm) && bi.n_records > 0 && gce_bam_chunk(f, 0, 1, 0, &one) == GCE_OK ? one.qname : nullptr);
    if ((rc = gce_create(&prm, &e)) != GCE_OK) return done(rc, gce_status_message(rc));
    if (fasta_path && *fasta_path) {
        if ((rc = gce_fasta_load(fasta_path, threads, &fa)) != GCE_OK) return done(rc, "cannot read the FASTA file");
        if ((rc = set_reference(e, fa, bi.target_name, (size_t)bi.n_targets)) != GCE_OK) return done(rc, gce_last_error(e));
    }
    double t0 = now_s();
    if ((rc = gce_reserve(e, bi.n_records, bi.qname_bytes, bi.cigar_words, bi.seq_bytes, bi.qual_bytes)) != GCE_OK) return done(rc, gce_last_error(e));     // (MI tags travel on the streamed path since round 5)
    if (chunk_reads <= 0) chunk_reads = 1 << 21;
    int32_t tickets[2] = {-1, -1};
    int64_t k = 0;
    for (int64_t first = 0; first < bi.n_records; first += chunk_reads, k++) {
        const int sl = (int)(k & 1);
        if (tickets[sl] >= 0 && (rc = gce_submit_wait(e, tickets[sl])) != GCE_OK) return done(rc, gce_last_error(e));   // the slot's previous copy
        gce_batch b;
        if ((rc = gce_bam_chunk(f, first, std::min(chunk_reads, bi.n_records - first), sl, &b)) != GCE_OK) return done(rc, "chunk");
        rc = gce_submit_async(e, &b, &tickets[sl]);
        if (rc != GCE_OK) return done(rc, gce_last_error(e));
    }
    out->submit_s = now_s() - t0; t0 = now_s();
    if (bi.n_records > 0) {
        if ((rc = gce_process(e)) != GCE_OK) return done(rc, gce_last_error(e)[0] ? gce_last_error(e) : gce_status_message(rc));
        out->process_s = now_s() - t0; t0 = now_s();
        gce_timing tm; if (gce_get_timing(e, &tm) == GCE_OK) out->kernel_ms = tm.total_ms;
        gce_result res;
        if ((rc = gce_drain(e, &res)) != GCE_OK) return done(rc, gce_last_error(e));
        out->drain_s = now_s() - t0; t0 = now_s();
        out->n_reads = res.n_reads; out->n_out = res.n_out; out->pre = res.pre; out->post = res.post;
        if ((rc = gce_bam_write(out_path, f, &res, threads, level)) != GCE_OK) return done(rc, "cannot write the output BAM");
    } else {
        gce_result res; memset(&res, 0, sizeof res);
        if ((rc = gce_bam_write(out_path, f, &res, threads, level)) != GCE_OK) return done(rc, "cannot write the output BAM");
    }
    out->write_s = now_s() - t0;
    out->total_s = now_s() - t_start;
    return done(GCE_OK, "");
}

// Gencore::consensus() for one BAM over SEVERAL engines: the stream is cut into n_shards ranges of the cluster key by the
// GPU planner (gce_stream_context + gce_plan_shards on devices[0]); shard r runs on HIP device devices[r] (ordinals may repeat: several
// engines on one GPU, which is how a one-GPU box tests it) with its reads, their global ticks, the flush events of the whole stream and
// -- per-shard staging -- only the reference window its reads can touch; the engines run side by side on host threads.  No data-path
// exchange: the output tables (each in bamComp order) are merged k-way by (tid, pos, mtid, mpos, isize, input index), mate rows are
// re-pointed, the two Stats blocks are SUMMED ON THE HOST (one process owns all engines here; one process per GPU merges them with one
// RCCL all-reduce instead, bench.py).  The result equals gce_run_bam's: same records, same order, same Stats.
int gce_run_bam_sharded_hostcodec(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int32_t n_shards, const int32_t *devices,
                                  int32_t plan_mode, int threads, int level, gce_bam_run *out, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !params || !out || n_shards < 1 || n_shards > 64 || !devices) return GCE_ERR_INVALID;
    memset(out, 0, sizeof *out);
    const double t_start = now_s();
    gce_bam *f = nullptr; gce_fasta *fa = nullptr;
    std::vector<gce_engine *> eng((size_t)n_shards, nullptr);
    int32_t *ev_tid = nullptr, *ev_pos = nullptr;
    int rc = gce_bam_open(in_path, threads, &f);
    auto done = [&](int code, const char *m) { set_err(err, m); for (auto *e : eng) if (e) gce_destroy(e); if (f) gce_bam_close(f); if (fa) gce_fasta_free(fa); gce_free(ev_tid); gce_free(ev_pos); return code; };
    if (rc != GCE_OK) return done(rc, f ? gce_bam_error(f) : "open failed");
    out->open_s = now_s() - t_start;
    gce_bam_info bi; gce_bam_get_info(f, &bi);
    out->read_s = bi.read_s; out->inflate_s = bi.inflate_s; out->index_s = bi.index_s;
    gce_params prm = *params;
    prm.tick_offset = 0; prm.trailing_flush = 0;
    gce_batch one;
    file_params(prm, bi.n_targets, bi.target_len, umi_auto(prm) && bi.n_records > 0 && gce_bam_chunk(f, 0, 1, 0, &one) == GCE_OK ? one.qname : nullptr);
    const int64_t n = bi.n_records;
    const int T = f->threads;
    const uint8_t *u = f->u.data();
    double t0 = now_s();
    // ---- the key records of the whole stream, the plan
    Raw<gce_core> cores; cores.resize((size_t)std::max<int64_t>(n, 1));
    Raw<uint64_t> tick; tick.resize((size_t)std::max<int64_t>(n, 1));
    Raw<int32_t> shard; shard.resize((size_t)std::max<int64_t>(n, 1));
    if (!cores.ok() || !tick.ok() || !shard.ok()) return done(GCE_ERR_OOM, "out of host memory");
    parallel_for(T, n, [&](int, int64_t a, int64_t e) { for (int64_t k = a; k < e; k++) memcpy(&cores[k], u + f->rec[k] + 4, 32); });
    int32_t n_ev = 0;
    const int period = prm.flush_period > 0 ? prm.flush_period : 10000;
    // --quit_after_contig (gencore.cpp:243-246): ONE cut on the whole stream, in front of the plan; the cut read goes to shard 0 behind its own reads (that
    // engine counts it and drops it), the other engines do not look for a cut (see gce_raw_select_shard)
    int64_t n_plan = n, cut = -1;
    if (prm.max_contig > 0) for (int64_t k = 0; k < n; k++) if (cores[k].tid >= prm.max_contig) { cut = k; n_plan = k; break; }
    if (n_plan > 0) {
        if ((rc = gce_stream_context(devices[0], cores.data(), n_plan, period, tick.data(), &n_ev, &ev_tid, &ev_pos)) != GCE_OK)
            return done(rc, rc == GCE_ERR_INVALID ? "not shardable by cluster key: a mapped read follows the first unmapped read" : gce_status_message(rc));
        if ((rc = gce_plan_shards(devices[0], cores.data(), n_plan, n_shards, plan_mode, shard.data())) != GCE_OK) return done(rc, gce_status_message(rc));
    }
    std::vector<std::vector<int64_t>> idx((size_t)n_shards);
    { std::vector<int64_t> cnt((size_t)n_shards, 0); for (int64_t k = 0; k < n_plan; k++) cnt[shard[k]]++; for (int r = 0; r < n_shards; r++) idx[r].reserve((size_t)cnt[r] + 1); for (int64_t k = 0; k < n_plan; k++) idx[shard[k]].push_back(k); }
    if (cut >= 0) { idx[0].push_back(cut); tick[cut] = 0; }
    if (fasta_path && *fasta_path && (rc = gce_fasta_load(fasta_path, threads, &fa)) != GCE_OK) return done(rc, "cannot read the FASTA file");
    int32_t nc = 0; const char *const *ids = nullptr; const char *const *seqs = nullptr; const int64_t *lens = nullptr;
    if (fa) gce_fasta_get(fa, &nc, &ids, &seqs, &lens);
    std::vector<int32_t> fa_of((size_t)bi.n_targets, -1);                        // Reference::getData looks contigs up by BAM target name (reference.cpp:43-53)
    for (int32_t t = 0; t < bi.n_targets; t++) for (int32_t c = 0; c < nc; c++) if (strcmp(ids[c], bi.target_name[t]) == 0) fa_of[t] = c;
    out->submit_s = now_s() - t0; t0 = now_s();
    // ---- the engines, side by side
    std::vector<gce_result> res((size_t)n_shards);
    std::vector<int> rcs((size_t)n_shards, GCE_OK); std::vector<std::string> msgs((size_t)n_shards);
    std::vector<Slot> slots((size_t)n_shards);
    std::vector<Raw<uint64_t>> ticks((size_t)n_shards);
    std::vector<double> kms((size_t)n_shards, 0.0);
    std::vector<std::thread> th;
    const int Tsub = std::max(1, T / n_shards);
    for (int r = 0; r < n_shards; r++) th.emplace_back([&, r] {
        auto failr = [&](int code, const char *m) { rcs[r] = code; msgs[r] = m ? m : ""; };
        const int64_t cnt = (int64_t)idx[r].size();
        memset(&res[r], 0, sizeof res[r]);
        gce_params pr = prm; pr.device = devices[r];
        if (r != 0 || cut < 0) pr.max_contig = 0;                                // (the cut is made above, once)
        int c2;
        if ((c2 = gce_create(&pr, &eng[r])) != GCE_OK) return failr(c2, gce_status_message(c2));
        if (cnt == 0) return;
        gce_batch b;
        {   // (gce_bam's own thread count is shared: the chunker of a shard uses its share of the host threads)
            const int keep = f->threads; (void)keep;
            if ((c2 = bam_chunk_impl(f, 0, idx[r].data(), cnt, slots[r], &b)) != GCE_OK) return failr(c2, "chunk");
        }
        ticks[r].resize((size_t)cnt);
        if (!ticks[r].ok()) return failr(GCE_ERR_OOM, "out of host memory");
        for (int64_t k = 0; k < cnt; k++) ticks[r][k] = tick[idx[r][k]];
        b.tick = ticks[r].data();
        if (fa) {                                                                // per-shard staging: per contig the bases between the shard's first read and its last reference position
            std::vector<int64_t> lo((size_t)bi.n_targets, INT64_MAX), hi((size_t)bi.n_targets, -1);
            for (int64_t k = 0; k < cnt; k++) {
                const gce_core &c = b.core[k];
                if (c.tid < 0 || c.tid >= bi.n_targets || c.pos < 0) continue;
                int64_t rl = 0; const uint32_t *cg = b.cigar + b.cigar_off[k];
                for (uint32_t q = 0; q < c.n_cigar; q++) { const uint32_t op = cg[q] & 0xF; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[q] >> 4; }
                lo[c.tid] = std::min<int64_t>(lo[c.tid], c.pos); hi[c.tid] = std::max<int64_t>(hi[c.tid], (int64_t)c.pos + rl);
            }
            for (int32_t t = 0; t < bi.n_targets; t++) {
                if (fa_of[t] < 0 || hi[t] < 0) continue;
                const int64_t clen = lens[fa_of[t]];
                const int64_t a = std::min<int64_t>(lo[t] & ~(int64_t)1, clen & ~(int64_t)1), z = std::min<int64_t>(hi[t], clen);
                if ((c2 = gce_set_reference_window(eng[r], t, clen, a, seqs[fa_of[t]] + a, std::max<int64_t>(z - a, 0))) != GCE_OK) return failr(c2, gce_last_error(eng[r]));
            }
        }
        if ((c2 = gce_set_flush_events(eng[r], n_ev, ev_tid, ev_pos)) != GCE_OK || (c2 = gce_submit(eng[r], &b)) != GCE_OK) return failr(c2, gce_last_error(eng[r]));
        if ((c2 = gce_process(eng[r])) != GCE_OK) return failr(c2, gce_last_error(eng[r])[0] ? gce_last_error(eng[r]) : gce_status_message(c2));
        gce_timing tm; if (gce_get_timing(eng[r], &tm) == GCE_OK) kms[r] = tm.total_ms;
        if ((c2 = gce_drain(eng[r], &res[r])) != GCE_OK) return failr(c2, gce_last_error(eng[r]));
    });
    for (auto &x : th) x.join();
    (void)Tsub;
    for (int r = 0; r < n_shards; r++) if (rcs[r] != GCE_OK) return done(rcs[r], msgs[r].c_str());
    out->process_s = now_s() - t0; t0 = now_s();
    for (int r = 0; r < n_shards; r++) out->kernel_ms = std::max(out->kernel_ms, kms[r]);
    // ---- merge: k-way by bamComp over the global input index
    int64_t n_out = 0;
    for (int r = 0; r < n_shards; r++) n_out += res[r].n_out;
    std::vector<uint32_t> m_src((size_t)n_out), m_qsrc((size_t)n_out); std::vector<int32_t> m_nm((size_t)n_out); std::vector<int16_t> m_fr((size_t)n_out), m_rr((size_t)n_out);
    std::vector<const uint8_t *> m_seq((size_t)n_out), m_qual((size_t)n_out);
    std::vector<std::vector<uint32_t>> rowmap((size_t)n_shards);
    std::vector<int64_t> head((size_t)n_shards, 0);
    for (int r = 0; r < n_shards; r++) rowmap[r].resize((size_t)res[r].n_out);
    auto gsrc = [&](int r, int64_t k) { return (uint32_t)idx[r][res[r].src[k]]; };
    auto less = [&](int ra, int64_t ka, int rb, int64_t kb) {
        const uint32_t ia = gsrc(ra, ka), ib = gsrc(rb, kb);
        const gce_core &a = cores[ia], &b = cores[ib];
        if (a.tid != b.tid) return a.tid < b.tid;
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.mtid != b.mtid) return a.mtid < b.mtid;
        if (a.mpos != b.mpos) return a.mpos < b.mpos;
        if (a.isize != b.isize) return a.isize < b.isize;
        return ia < ib;
    };
    for (int64_t row = 0; row < n_out; row++) {
        int best = -1;
        for (int r = 0; r < n_shards; r++) if (head[r] < res[r].n_out && (best < 0 || less(r, head[r], best, head[best]))) best = r;
        const int64_t k = head[best]++;
        rowmap[best][k] = (uint32_t)row;
        m_src[row] = gsrc(best, k); m_qsrc[row] = (uint32_t)idx[best][res[best].qname_src[k]];
        m_nm[row] = res[best].nm_new[k]; m_fr[row] = res[best].fr[k]; m_rr[row] = res[best].rr[k];
        m_seq[row] = res[best].seq + res[best].seq_off[k]; m_qual[row] = res[best].qual + res[best].qual_off[k];
    }
    // (the unsigned tid of an unmapped record sorts it last in the engines' tables; bamComp compares the signed field: pass-through
    //  records of unmapped reads do not exist -- unmapped reads are dropped, gencore.cpp:255-266 -- so the two orders agree)
    for (int r = 0; r < n_shards; r++) {
        out->n_reads += res[r].n_reads; out->n_out += res[r].n_out;
        const int64_t *a = (const int64_t *)&res[r].pre, *c = (const int64_t *)&res[r].post;
        int64_t *pa = (int64_t *)&out->pre, *pc = (int64_t *)&out->post;
        for (int q = 0; q < GCE_STATS_WORDS; q++) { pa[q] += a[q]; pc[q] += c[q]; }
    }
    out->drain_s = now_s() - t0; t0 = now_s();
    const OutRows rows{n_out, m_src.data(), m_qsrc.data(), m_nm.data(), m_fr.data(), m_rr.data()};
    if ((rc = bam_write_rows(out_path, f, rows, [&](int64_t k) { return m_seq[k]; }, [&](int64_t k) { return m_qual[k]; }, threads, level)) != GCE_OK) return done(rc, "cannot write the output BAM");
    out->write_s = now_s() - t0;
    out->total_s = now_s() - t_start;
    return done(GCE_OK, "");
}

int gce_run_bam(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int threads,
                int64_t chunk_reads, int level, gce_bam_run *out, char err[256]) {
    if (!in_path || !out_path || !params || !out) return GCE_ERR_INVALID;
    if (getenv("GCE_BAM_HOSTCODEC")) return gce_run_bam_hostcodec(in_path, out_path, fasta_path, params, threads, chunk_reads, level, out, err);
    return run_bam_impl(in_path, out_path, fasta_path, params, threads, chunk_reads, level, out, err, 1, nullptr, 0);
}

void gce_depth_run_free(gce_depth_run *d) {
    if (!d) return;
    free(d->bin_off); free(d->pre_depth); free(d->post_depth); free(d->pre_bed); free(d->post_bed);
    if (d->region_tid || d->region_start || d->region_end) gce_bed_free(d->n_regions, d->region_tid, d->region_start, d->region_end, nullptr);
    memset(d, 0, sizeof *d);
}

// gce_run_bam / gce_run_bam_sharded with the depth statistics of the reference's report: see include/gencore_amd.h.
int gce_run_bam_depth(const char *in_path, const char *out_path, const char *fasta_path, const char *bed_path, int32_t coverage_step, const gce_params *params,
                      int32_t n_shards, const int32_t *devices, int32_t plan_mode, int threads, int level, gce_bam_run *out, gce_depth_run *depth, char err[256]) {
    if (!depth || n_shards < 1 || n_shards > 64 || (n_shards > 1 && !devices)) return GCE_ERR_INVALID;
    gce_params prm;
    if (params && n_shards == 1 && devices) { prm = *params; prm.device = devices[0]; params = &prm; }
    const int rc = run_bam_impl(in_path, out_path, fasta_path, params, threads, 0, level, out, err, n_shards, n_shards > 1 ? devices : nullptr, plan_mode, bed_path, coverage_step, depth);
    if (rc != GCE_OK) gce_depth_run_free(depth);
    return rc;
}

// Gencore::consensus() for one file over SEVERAL engines on the GPU codec (src/gencore.cpp:164-205): see run_bam_impl.  The host
// reads the file once; every engine gets the compressed pieces over its own PCIe link, inflates, indexes and plans on its own GPU and keeps its
// key range; outputs are merged device to device.  GCE_BAM_HOSTCODEC=1: round 2's runner (host inflate and index, host-side cut, host merge).
int gce_run_bam_sharded(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int32_t n_shards, const int32_t *devices,
                        int32_t plan_mode, int threads, int level, gce_bam_run *out, char err[256]) {
    if (!in_path || !out_path || !params || !out || n_shards < 1 || n_shards > 64 || !devices || (plan_mode != 0 && plan_mode != 1)) return GCE_ERR_INVALID;
    if (getenv("GCE_BAM_HOSTCODEC")) return gce_run_bam_sharded_hostcodec(in_path, out_path, fasta_path, params, n_shards, devices, plan_mode, threads, level, out, err);
    return run_bam_impl(in_path, out_path, fasta_path, params, threads, 0, level, out, err, n_shards, devices, plan_mode);
}

}  // extern "C"
