// bamio_reader.hpp -- a BGZF file read piece by piece on the host: PassReader (the members of each piece, inflated on request), read_bam_header
// (the one loop that host-inflates a file's first members until its BAM header is whole), read_stream_header (the same with the streaming
// runners' pieces and words) and for_each_window (the window loop of the index,
// sort and calmd runners).  Needs no device: beside gce_bgzf.hpp and parallel_for, its pinned window comes from gce_host_alloc / gce_host_free,
// which a program without HIP supplies over malloc (tests/reader_host_check.cpp).
#pragma once
#include <atomic>
#include "bamio_common.hpp"
#include "gce_fileout.hpp"

namespace {

// the inflated record stream of a BGZF file, window by window: a piece of compressed bytes is inflated by the host threads behind what the
// last window left over (the record its end cut); the window handed on is its whole records, with their offsets
struct PassReader {
    int fd = -1; uint64_t fsz = 0, at = 0; size_t piece = 8 << 20; int T = 1;
    std::vector<uint8_t> comp; size_t have = 0;
    Pinned win; size_t n = 0;
    std::vector<Block> blocks; std::vector<uint64_t> z_coff; std::vector<uint32_t> z_csize, z_usize;
    std::string msg;
    size_t used = 0;                                 // compressed bytes of the members handed out last
    void reset() { at = 0; have = 0; n = 0; used = 0; }
    // the next piece's whole BGZF members -> blocks (their bytes at comp[0 ..]); 1: members, 0: end of the file, -1: error (msg)
    int members_next() {
        if (used) { memmove(comp.data(), comp.data() + used, have - used); have -= used; used = 0; }
        if (at >= fsz) { if (have) { msg = "truncated BGZF block at the end of the file"; return -1; } return 0; }
        const size_t want = (size_t)std::min<uint64_t>(piece, fsz - at);
        if (comp.size() < have + want) comp.resize(have + want);
        if (pread_full(fd, comp.data() + have, want, at) != want) { msg = "cannot read the input BAM"; return -1; }
        at += want; have += want;
        blocks.clear();
        size_t c = 0; uint64_t uoff = 0;
        for (Member m;;) {
            const Scan sc = scan_member(comp.data(), have, c, m);
            if (sc == Scan::More) break;                                                // cut by the piece's end: it stays for the next piece
            if (sc != Scan::Member) { msg = scan_message(sc); return -1; }
            blocks.push_back(Block{c, m.bsize, m.isize, n + uoff}); c += m.bsize; uoff += m.isize;
        }
        if (blocks.empty() && at < fsz) { msg = "BGZF block larger than a window"; return -1; }
        used = c;
        return 1;
    }
    bool last_piece() const { return at >= fsz; }
    // blocks as the arrays the GPU entry points take (z_coff, z_csize, z_usize); returns the members' inflated bytes
    uint64_t member_arrays() {
        z_coff.clear(); z_csize.clear(); z_usize.clear(); uint64_t u_all = 0;
        for (const Block &b : blocks) { z_coff.push_back(b.coff); z_csize.push_back(b.csize); z_usize.push_back(b.usize); u_all += b.usize; }
        return u_all;
    }
    // (the BAM header) the next piece inflated by the host threads behind win[0, n); 1: bytes added, 0: end of the file, -1: error (msg)
    int inflate_next() {
        const int g = members_next();
        if (g <= 0) return g;
        uint64_t uoff = 0;
        for (Block &b : blocks) { b.uoff = n + uoff; uoff += b.usize; }
        if (n + (size_t)uoff + 64 > win.cap) {                                       // (Pinned::ensure does not keep the bytes: the carry-over moves by hand)
            Pinned nw;
            if (!nw.ensure(n + (size_t)uoff + 64)) { msg = "out of pinned host memory"; return -1; }
            if (n) memcpy(nw.p, win.p, n);
            std::swap(win.p, nw.p); std::swap(win.cap, nw.cap);
        }
        std::atomic<int> bad{0};
        parallel_for(T, (int64_t)blocks.size(), [&](int, int64_t a, int64_t b2) { for (int64_t q = a; q < b2; q++) if (blocks[q].usize && !inflate_block(comp.data() + blocks[q].coff, blocks[q], win.p + blocks[q].uoff)) bad = 1; });
        if (bad) { msg = "inflate / CRC failure"; return -1; }
        n += (size_t)uoff;
        return 1;
    }
};

// is the first record's name, behind a header that ends at hdr_end, within the bytes inflated so far?
inline bool first_name_there(const PassReader &rd, uint64_t hdr_end) { return rd.n >= hdr_end + 36 && rd.n >= hdr_end + 36 + rd.win.p[hdr_end + 12]; }
// How an attempt to read a file's BAM header ended.  Ended: the stream has no more bytes and the header is not whole; Empty: the same for a
// file of no bytes; Failed: the reader's own error, its words in rd.msg.  The runners put their own words to each.
enum class HeaderRead { Complete, NotBam, Ended, Empty, Failed };
// The BAM header of rd's file: pieces are inflated behind one another (rd.win[0, rd.n)) until parse_bam_header, in the given dialect, finds
// the header whole; bh, *names and *lens (either may be NULL) are then the parser's.  first_name: the reading goes on until the name of the
// first record is there too, or the stream ends (the "auto" UMI prefix is read off that name) -- not for a header without contigs, which the
// runner that asks for the name refuses as it stands.
inline HeaderRead read_bam_header(PassReader &rd, Contigs dialect, bool first_name, BamHeader &bh, std::vector<std::string> *names = nullptr, std::vector<uint32_t> *lens = nullptr) {
    for (;;) {
        const int g = rd.inflate_next();
        if (g < 0) return HeaderRead::Failed;
        const Hdr hs = parse_bam_header(rd.win.p, rd.n, dialect, bh, names, lens);
        if (hs == Hdr::NotBam) return HeaderRead::NotBam;
        if (hs == Hdr::Complete) break;
        if (g == 0) return rd.fsz ? HeaderRead::Ended : HeaderRead::Empty;
    }
    while (first_name && bh.n_ref && !first_name_there(rd, bh.hdr_end)) {
        const int g = rd.inflate_next();
        if (g < 0) return HeaderRead::Failed;
        if (g == 0) break;
    }
    return HeaderRead::Complete;
}
// ... for a runner that then streams the file from its first byte: rh reads `in` with T threads in pieces of 1 MB (of a window, where that is
// smaller), the contigs passed over.  *why: the words for what is returned, the reader's own (rh.msg) when it failed.
inline HeaderRead read_stream_header(PassReader &rh, const InputFile &in, int T, uint64_t window_bytes, BamHeader &bh, const char **why, std::vector<std::string> *names = nullptr,
                                     std::vector<uint32_t> *lens = nullptr) {
    rh.fd = in.fd; rh.fsz = in.fsz; rh.T = T; rh.piece = window_bytes > 0 ? (size_t)std::min<uint64_t>(window_bytes, (uint64_t)1 << 20) : ((size_t)1 << 20);
    const HeaderRead h = read_bam_header(rh, Contigs::Skip, false, bh, names, lens);
    switch (h) {
    case HeaderRead::Failed: *why = rh.msg.c_str(); break;
    case HeaderRead::NotBam: *why = "not a BAM stream"; break;
    case HeaderRead::Ended: case HeaderRead::Empty: *why = "truncated BAM header"; break;
    case HeaderRead::Complete: *why = ""; break;
    }
    return h;
}

// A BGZF file from its first byte, window by window, for the index and sort runners: the host reads a piece and finds its members, the
// first hdr_end inflated bytes (the BAM header) are passed over, window(rd, u_all, sk) hands the members to the GPU (u_all: their inflated
// bytes, sk: how many of those belong to the header); then the end-of-file checks.  read_s / gpu_s: the two sides' seconds, added to.
// Returns GCE_OK, GCE_ERR_INVALID with msg set, or what `window` returned with msg left alone (the caller asks its GPU object why).
template <class F> int for_each_window(PassReader &rd, uint64_t hdr_end, double *read_s, double *gpu_s, std::string &msg, F &&window) {
    uint64_t skip = hdr_end;
    for (;;) {
        double t0 = now_s();
        const int g = rd.members_next();
        if (g < 0) { msg = rd.msg; return GCE_ERR_INVALID; }
        if (g == 0) break;
        const uint64_t u_all = rd.member_arrays(), sk = std::min<uint64_t>(skip, u_all);
        *read_s += now_s() - t0; t0 = now_s();
        const int rc = window(rd, u_all, sk);
        *gpu_s += now_s() - t0;
        if (rc != GCE_OK) return rc;
        skip -= sk;
        if (rd.last_piece()) break;
    }
    if (rd.have != rd.used) { msg = "truncated BGZF block at the end of the file"; return GCE_ERR_INVALID; }
    if (skip) { msg = "truncated BAM header"; return GCE_ERR_INVALID; }
    return GCE_OK;
}

}  // namespace
