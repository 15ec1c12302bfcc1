// gce_fileout.hpp — the output side of the file runners, once (included by bamio.cpp and by tests/fileout_host_check.cpp; no GPU code, no
// C-ABI): the piece pump (a byte stream that lives in device memory walked in pieces over two host buffers), the output file (SAM text or
// BGZF members, its header and its checked close) and the two text conversions on all host threads (records -> lines, lines -> records).
// The GPU is known only through the callables handed to pump_pieces.  Like gce_bgzf.hpp, the private part of ONE translation unit per program.
#pragma once
#include <atomic>
#include <cstdio>
#include <thread>
#include "../../include/gencore_amd.h"
#include "gce_bgzf.hpp"
#include "gce_samtext.hpp"

namespace {

template <class F> void parallel_for(int threads, int64_t n, F f) {          // f(thread, begin, end) over contiguous ranges
    threads = (int)std::max<int64_t>(1, std::min<int64_t>(threads, n));
    if (threads == 1) { f(0, (int64_t)0, n); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) th.emplace_back([=] { f(t, n * t / threads, n * (t + 1) / threads); });
    for (auto &x : th) x.join();
}

// What the file-to-file runners write: src[0, n) as BGZF members of 0xff00 bytes, deflated by all host threads 256 members a round (the
// slots of zbuf: 256 * 0x10000 + 64 bytes) and written in order.  false: a member could not be deflated or written.
constexpr uint64_t MEMBER_BYTES = 0xff00, ROUND_BYTES = MEMBER_BYTES * 256;
inline bool write_members(FILE *fo, const uint8_t *src, size_t n, int level, int T, uint8_t *zbuf) {
    for (size_t o = 0; o < n; o += (size_t)ROUND_BYTES) {
        const size_t m = std::min<size_t>((size_t)ROUND_BYTES, n - o);
        const int64_t nb = (int64_t)((m + MEMBER_BYTES - 1) / MEMBER_BYTES);
        uint32_t zs[256] = {0};
        parallel_for(T, nb, [&](int, int64_t x, int64_t y) { for (int64_t q = x; q < y; q++) { const uint64_t a = (uint64_t)q * MEMBER_BYTES; zs[q] = (uint32_t)deflate_block(src + o + a, (uint32_t)std::min<uint64_t>(MEMBER_BYTES, m - a), level, zbuf + (size_t)q * 0x10000); } });
        for (int64_t q = 0; q < nb; q++) if (zs[q] == 0 || fwrite(zbuf + (size_t)q * 0x10000, 1, zs[q], fo) != zs[q]) return false;
    }
    return true;
}

// ---- the piece pump: prefix[0, prefix_n) (host bytes, the BAM header) followed by stream[0, stream_n) (device bytes) goes to `sink` in pieces
// of `piece` bytes.  Per piece k: fetch(offset in the stream, dst, n, &ticket) starts the copy of piece k + 1's stream bytes behind its
// prefix bytes, wait(ticket) ends piece k's, sink(ptr, n) takes piece k.  A piece that lies wholly in the prefix is neither fetched nor
// waited for.  The first status that is not GCE_OK ends the walk and is returned as it is (a buffer that cannot grow: GCE_ERR_OOM).
// Two buffers are enough: the fetch of piece k + 1 goes into the buffer of piece k - 1, whose sink returned before piece k's turn began.
template <class Buf, class Fetch, class Wait, class Sink>
int pump_pieces(const uint8_t *prefix, uint64_t prefix_n, uint64_t stream_n, uint64_t piece, Buf (&buf)[2], Fetch &&fetch, Wait &&wait, Sink &&sink) {
    const uint64_t total = prefix_n + stream_n;
    const int64_t n = (int64_t)((total + piece - 1) / piece);
    int32_t ticket[2] = {-1, -1};
    auto start = [&](int64_t pc) -> int {
        const uint64_t a = (uint64_t)pc * piece, z = std::min<uint64_t>(total, a + piece), hn = a < prefix_n ? std::min<uint64_t>(prefix_n, z) - a : 0;
        Buf &b = buf[pc & 1];
        if (!b.ensure((size_t)(z - a) + 64)) return GCE_ERR_OOM;
        if (hn) memcpy(b.p, prefix + a, (size_t)hn);
        ticket[pc & 1] = -1;
        return a + hn < z ? fetch(a + hn - prefix_n, b.p + hn, (size_t)(z - a - hn), &ticket[pc & 1]) : GCE_OK;
    };
    int rc = n > 0 ? start(0) : GCE_OK;
    for (int64_t pc = 0; pc < n && rc == GCE_OK; pc++) {
        if (pc + 1 < n && (rc = start(pc + 1)) != GCE_OK) break;
        if (ticket[pc & 1] >= 0 && (rc = wait(ticket[pc & 1])) != GCE_OK) break;
        rc = sink((const uint8_t *)buf[pc & 1].p, (size_t)(std::min<uint64_t>(total, (uint64_t)(pc + 1) * piece) - (uint64_t)pc * piece));
    }
    return rc;
}

// ---- the output file of a runner: SAM text for a name that ends in "sam" (src/gencore.cpp:170-173: sam_open(out, "w")), BGZF members otherwise
struct OutFile {
    FILE *fo = nullptr; bool sam = false; uint8_t *zbuf = nullptr;
    OutFile() = default;
    OutFile(const OutFile &) = delete; OutFile &operator=(const OutFile &) = delete;
    ~OutFile() { drop(); free(zbuf); }
    void drop() { if (fo) { fclose(fo); fo = nullptr; } }                         // closed without a word (a failed run)
    static bool named_sam(const char *path) { const size_t n = strlen(path); return n >= 3 && strcmp(path + n - 3, "sam") == 0; }
    bool open(const char *path, bool as_sam) { sam = as_sam; fo = fopen(path, sam ? "w" : "wb"); return fo != nullptr; }
    bool write(const void *p, size_t n) { return fwrite(p, 1, n, fo) == n; }
    // SAM: the header text, with @SQ lines from the contig table if it has none
    bool sam_header(const std::string &text, const std::vector<std::string> &names, const std::vector<uint32_t> &lens) { const std::string ht = samtext::header_text_for_sam(text, names, lens); return write(ht.data(), ht.size()); }
    bool reserve() { if (!zbuf) zbuf = (uint8_t *)malloc((size_t)256 * 0x10000 + 64); return zbuf != nullptr; }      // the slots write_members deflates into
    bool members(const uint8_t *src, size_t n, int level, int T) { return write_members(fo, src, n, level, T, zbuf); }
    // BAM: the header in members of its own -- by the host at level 1 where the GPU deflates the body, at `level` otherwise
    bool header_members(const std::vector<uint8_t> &hdr, int level, bool gpu_body, int T) { return members(hdr.data(), hdr.size(), gpu_body ? 1 : level, T); }
    // BAM: the EOF marker; then the close, checked (a full disk must not pass for a finished file: the reference exits when sam_close fails)
    bool close() { bool ok = sam || write(BGZF_EOF, 28); ok = fclose(fo) == 0 && ok; fo = nullptr; return ok; }
};

// ---- records -> lines.  The offsets of the whole records of p[0, n) -> ro; returns the offset behind the last of them (n unless the end cuts a
// record), SIZE_MAX for a block_size below 32
inline size_t whole_records(const uint8_t *p, size_t n, std::vector<uint64_t> &ro) {
    ro.clear();
    size_t o = 0;
    while (o + 4 <= n) { const uint32_t bs = rd32(p + o); if (bs < 32) return SIZE_MAX; if (o + 4 + (size_t)bs > n) break; ro.push_back(o); o += 4 + (size_t)bs; }
    return o;
}
// the records at buf + ro[..] as SAM lines, the records spread over T threads: thread t's lines in lines[t], to be written in that order.  false: a bad record
inline bool records_to_lines(const uint8_t *buf, const std::vector<uint64_t> &ro, const std::vector<std::string> &names, int T, std::vector<std::string> &lines) {
    lines.resize((size_t)T);
    std::atomic<int> bad{0};
    const size_t nr = ro.size();
    parallel_for(T, T, [&](int, int64_t x, int64_t y) { for (int64_t t = x; t < y; t++) { std::string &L = lines[(size_t)t]; L.clear(); const size_t ra = nr * (size_t)t / (size_t)T, rb = nr * (size_t)(t + 1) / (size_t)T; for (size_t q = ra; q < rb; q++) if (!samtext::bam_to_line(buf + ro[q], names, L)) { bad = 1; return; } } });
    return !bad;
}

// ---- lines -> records: the alignment lines of d[p, lim) (lim: behind a line feed, or the text's end) as BAM records, thread t converting the
// lines that START in its range of the text (cut at line feeds) into parts[t]; an empty line and a lone '\r' are passed over.  Returns
// nullptr, or the message of the lowest-numbered thread that has one.
inline const char *lines_to_records(const char *d, size_t p, size_t lim, int T, const samtext::NameMap &nmap, std::vector<std::vector<uint8_t>> &parts, std::vector<std::string> &perr) {
    parts.resize((size_t)T); perr.resize((size_t)T);
    std::vector<size_t> cut((size_t)T + 1, lim);
    cut[0] = p;
    for (int t = 1; t < T; t++) { size_t c = p + (lim - p) * (size_t)t / (size_t)T; if (c > p) { const char *q = (const char *)memchr(d + c - 1, '\n', lim - (c - 1)); c = q ? (size_t)(q - d) + 1 : lim; } cut[(size_t)t] = std::max(c, cut[(size_t)t - 1]); }
    std::atomic<int> bad{0};
    parallel_for(T, T, [&](int, int64_t a, int64_t b2) {
        for (int64_t t = a; t < b2; t++) {
            std::vector<uint8_t> &o = parts[(size_t)t]; o.clear();
            size_t x = cut[(size_t)t]; const size_t xe = cut[(size_t)t + 1];
            while (x < xe) {
                const char *q = (const char *)memchr(d + x, '\n', lim - x); const size_t le = q ? (size_t)(q - d) : lim;
                if (le > x && !(le == x + 1 && d[x] == '\r') && !samtext::line_to_bam(d + x, d + le, nmap, o, perr[(size_t)t])) { bad = 1; return; }
                x = le + 1;
            }
        }
    });
    if (!bad) return nullptr;
    for (auto &m : perr) if (!m.empty()) return m.c_str();
    return "malformed SAM line";
}

}  // namespace
