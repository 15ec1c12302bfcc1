// bamio.cpp — the file side of the C-ABI (include/gencore_amd.h, "files" section), in two halves.
//
// Host only: the whole-file BAM reader (gce_bam_open / gce_bam_chunk: records -> gce_batch) and writer (gce_bam_write), SAM text <-> BAM
// (gce_samtext.hpp), the FASTA and BED loaders, the reports (gce_report.hpp).  They replace what the reference does through htslib and
// FastaReader around the hot path:
//   sam_open / sam_hdr_read / sam_read1        src/gencore.cpp:164-205      -> gce_bam_open (+ gce_bam_chunk)
//   sam_hdr_write / sam_write1 / sam_close     src/gencore.cpp:187-190,104  -> gce_bam_write (result rows -> records -> BGZF)
//   FastaReader::readAll / readNext / to4bits  src/fastareader.cpp:57-104,139-152,157-168 -> gce_fasta_load
// htslib itself is a pinned dependency that is absent from the reference tree; the formats are the published ones (SAMv1 section 4).
//
// Drivers of the GPU: the file-to-file runners gce_run_bam (+ sharded, depth), gce_run_bam_passes, gce_bam_index, gce_bam_sort,
// gce_bam_sort_passes and gce_sam_sort.  This file launches no kernel itself: the runners read the file, find its BGZF members and hand
// them, window by window, to the engine's entry points in engine.hip (gce_raw_*, gce_passes_*, gce_bai_*, gce_sort_*), which inflate, index,
// process, sort and deflate in HBM; the output comes back in pieces and is written here.
//
// One copy of each shared piece: member framing, the BAM header, the member codec, the EOF member and the file helpers are in
// gce_bgzf.hpp; PassReader (a file's members, piece by piece), for_each_window (the window loop of the index and sort runners) and
// write_members (a piece deflated into 0xff00-byte members on all host threads, written in order) are below.
// Everything that scales with the file is spread over `threads` host threads: inflate per BGZF block, the struct-of-arrays fill
// per record range, record rebuild + deflate per output block.
#include <zlib.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../include/gencore_amd.h"
#include "gce_bgzf.hpp"
#include "gce_samtext.hpp"
#include "gce_fileout.hpp"
#include "gce_report.hpp"

static double now_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

namespace {

// host threads when the caller does not say: the CPUs this process may run on (affinity mask / cgroup quota), at most 64 -- on the
// 256-thread box the measurements were made on, inflate and deflate stop scaling near 64 threads and lose 30 % at 256
int default_threads() {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {                       // cgroup v2: "<quota> <period>" or "max <period>"
        long long q = 0, per = 0;
        if (fscanf(f, "%lld %lld", &q, &per) == 2 && q > 0 && per > 0) n = std::min<long long>(n, std::max<long long>(1, (q + per - 1) / per));
        fclose(f);
    }
    return std::min(n, 64);
}

template <class V> bool read_file(const char *path, V &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize((size_t)std::max(0l, sz));
    const size_t got = sz > 0 ? fread(out.data(), 1, (size_t)sz, f) : 0;
    fclose(f);
    return got == (size_t)std::max(0l, sz);
}

// a growable buffer that is NOT value-initialised (std::vector::resize would write gigabytes of zeros on one thread)
template <class T> struct Raw {
    T *p = nullptr; size_t cap = 0, n = 0;
    Raw() = default;
    Raw(const Raw &) = delete; Raw &operator=(const Raw &) = delete;
    Raw(Raw &&o) noexcept : p(o.p), cap(o.cap), n(o.n) { o.p = nullptr; o.cap = o.n = 0; }
    Raw &operator=(Raw &&o) noexcept { if (this != &o) { free(p); p = o.p; cap = o.cap; n = o.n; o.p = nullptr; o.cap = o.n = 0; } return *this; }
    ~Raw() { free(p); }
    void release() { free(p); p = nullptr; cap = n = 0; }
    void resize(size_t k) {
        if (k > cap) {
            free(p);
            const size_t bytes = std::max<size_t>(k, 1) * sizeof(T);
            if (bytes >= (8u << 20)) {                                           // big buffers: 2 MB pages where the kernel offers them (first touch
                const size_t rounded = (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);    // of 4 KB pages is what the host path mostly waits for)
                p = (T *)aligned_alloc(2u << 20, rounded);
                if (p) madvise(p, rounded, MADV_HUGEPAGE);
            } else p = (T *)malloc(bytes);
            cap = p ? k : 0;
        }
        n = p ? k : 0;
    }
    bool ok() const { return p != nullptr; }                                     // false after a failed allocation (callers return GCE_ERR_OOM)
    T *data() { return p; }
    const T *data() const { return p; }
    size_t size() const { return n; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};

// the whole file into an uninitialised buffer, every thread pulling its own range (one thread copies out of the page cache at ~10 GB/s:
// 60 ms for the 572 MB of the benchmark's file)
bool read_file_parallel(const char *path, Raw<uint8_t> &out, int threads) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 0) { close(fd); return false; }
    const int64_t sz = (int64_t)st.st_size;
    out.resize((size_t)sz);
    if (!out.ok()) { close(fd); return false; }
    std::atomic<int> bad{0};
    const int64_t piece = 8 << 20;
    parallel_for(threads, (sz + piece - 1) / piece, [&](int, int64_t a, int64_t e) {
        for (int64_t k = a; k < e; k++) {
            const int64_t off = k * piece, end = std::min(sz, off + piece);
            if (pread_full(fd, out.data() + off, (size_t)(end - off), (uint64_t)off) != (size_t)(end - off)) { bad = 1; return; }
        }
    });
    close(fd);
    return !bad;
}
struct Slot {                                     // struct-of-arrays buffers of one chunk
    Raw<gce_core> core; Raw<uint64_t> qoff, coff, soff, loff, mioff;
    Raw<char> qname, mi; Raw<uint32_t> cigar; Raw<uint8_t> seq, qual, nmt; Raw<int32_t> nm;
};

// aux walk of one record: NM (type + value as bam_aux2i gives it) and MI:Z
struct AuxInfo { uint8_t nm_type; int32_t nm; const char *mi; };
inline size_t aux_size(uint8_t type, const uint8_t *p, const uint8_t *end) {   // bytes of the value behind the type byte, or SIZE_MAX
    switch (type) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'd': return 8;
    case 'Z': case 'H': { const uint8_t *q = p; while (q < end && *q) q++; return q < end ? (size_t)(q - p) + 1 : SIZE_MAX; }
    case 'B': {
        if (p + 5 > end) return SIZE_MAX;
        const size_t es = aux_size(p[0], nullptr, nullptr);
        return es == SIZE_MAX ? SIZE_MAX : 5 + es * (size_t)rd32(p + 1);
    }
    default: return SIZE_MAX;
    }
}
inline AuxInfo scan_aux(const uint8_t *p, const uint8_t *end) {
    AuxInfo a{0, 0, nullptr};
    while (p + 3 <= end) {
        const uint8_t t0 = p[0], t1 = p[1], type = p[2];
        const uint8_t *v = p + 3;
        const size_t sz = aux_size(type, v, end);
        if (sz == SIZE_MAX || v + sz > end) break;
        if (t0 == 'N' && t1 == 'M' && a.nm_type == 0) {                      // bam_aux_get returns the first match
            a.nm_type = type;
            switch (type) {                                                   // bam_aux2i
            case 'c': a.nm = (int8_t)v[0]; break;   case 'C': a.nm = v[0]; break;
            case 's': a.nm = (int16_t)rd16(v); break; case 'S': a.nm = rd16(v); break;
            case 'i': a.nm = rdi32(v); break;        case 'I': a.nm = (int32_t)rd32(v); break;
            default: a.nm = 0; break;
            }
        } else if (t0 == 'M' && t1 == 'I' && type == 'Z' && !a.mi) a.mi = (const char *)v;
        p = v + sz;
    }
    return a;
}

// body -> BGZF blocks of 0xff00 bytes + the EOF marker block
int write_bgzf(const char *path, const Raw<uint8_t> &body, int T, int level) {
    const uint64_t BS = 0xff00;
    const int64_t nb = (int64_t)((body.size() + BS - 1) / BS);
    Raw<uint8_t> z; z.resize((size_t)nb * 0x10000 + 64);                      // (not a std::vector: its zero fill of these 400 MB, and of the body's, on one
                                                                              //  thread was most of the write stage)
    if (!z.ok()) return GCE_ERR_OOM;
    std::vector<uint32_t> zs((size_t)nb, 0);
    parallel_for(T, nb, [&](int, int64_t a, int64_t e) {
        for (int64_t k = a; k < e; k++) {
            const uint64_t o = (uint64_t)k * BS; const uint32_t len = (uint32_t)std::min<uint64_t>(BS, body.size() - o);
            zs[k] = (uint32_t)deflate_block(body.data() + o, len, level, z.data() + (size_t)k * 0x10000);
        }
    });
    for (int64_t k = 0; k < nb; k++) if (zs[k] == 0) return GCE_ERR_INVALID;       // a block that could not be deflated
    FILE *f = fopen(path, "wb");
    if (!f) return GCE_ERR_INVALID;
    for (int64_t k = 0; k < nb; k++) if (fwrite(z.data() + (size_t)k * 0x10000, 1, zs[k], f) != zs[k]) { fclose(f); return GCE_ERR_INVALID; }
    const bool eof_ok = fwrite(BGZF_EOF, 1, 28, f) == 28;                          // (a full disk must not pass for a finished BAM: the reference exits when sam_write1 / sam_close fail)
    if (fclose(f) != 0 || !eof_ok) return GCE_ERR_INVALID;
    return GCE_OK;
}

// the message of a C-ABI call into its caller's buffer
void set_err(char err[256], const char *m) { if (err) { strncpy(err, m ? m : "", 255); err[255] = 0; } }

}  // namespace

struct gce_bam {
    Raw<uint8_t> u;                               // the inflated stream
    std::string text;
    std::vector<std::string> names; std::vector<const char *> name_ptr; std::vector<uint32_t> lens;
    std::vector<uint64_t> rec;                    // offset of every record's block_size
    uint64_t tot_q = 0, tot_c = 0, tot_s = 0, tot_l = 0, tot_mi = 0;
    int threads = 1;
    Slot slot[2];
    std::string err;
    double t_read = 0, t_inflate = 0, t_index = 0;
};


extern "C" {

int gce_bam_open(const char *path, int threads, gce_bam **out) {
    if (!path || !out) return GCE_ERR_INVALID;
    gce_bam *f = new gce_bam();
    f->threads = threads > 0 ? threads : default_threads();
    *out = f;
    double t0 = now_s();
    Raw<uint8_t> z;
    if (!read_file_parallel(path, z, f->threads)) { f->err = std::string("cannot read ") + path; return GCE_ERR_INVALID; }
    f->t_read = now_s() - t0; t0 = now_s();
    // ---- BGZF members
    std::vector<Block> blocks;
    uint64_t off = 0, uoff = 0;
    while (off + 18 <= z.size()) {
        Member m;
        const Scan sc = scan_member(z.data(), z.size(), (size_t)off, m);
        if (sc != Scan::Member) {                                                       // the whole file is here: a member that needs more bytes is cut by the file's end
            const bool header_cut = off + 12 + (uint64_t)m.xlen + 8 > z.size();         // the extra field (and the trailer) must lie inside the file
            f->err = sc == Scan::NotBgzf ? scan_message(sc) : header_cut ? "truncated BGZF block header" : sc == Scan::More ? "bad BGZF block" : scan_message(sc);
            return GCE_ERR_INVALID;
        }
        blocks.push_back(Block{off, m.bsize, m.isize, uoff});
        off += m.bsize; uoff += m.isize;
    }
    if (off != z.size()) { f->err = "trailing bytes after the last BGZF block"; return GCE_ERR_INVALID; }
    f->u.resize(uoff + 64);
    if (!f->u.ok()) { f->err = "out of host memory for the inflated stream"; return GCE_ERR_OOM; }
    if (getenv("GCE_BAM_PRETOUCH")) {                                              // diagnostic: first-touch cost of the destination alone
        const double tp = now_s();
        parallel_for(f->threads, (int64_t)((uoff + 4095) / 4096), [&](int, int64_t a, int64_t e) { for (int64_t k = a; k < e; k++) f->u.data()[(size_t)k * 4096] = 0; });
        fprintf(stderr, "pretouch %.3f s\n", now_s() - tp);
    }
    std::atomic<int> bad{0};
    parallel_for(f->threads, (int64_t)blocks.size(), [&](int, int64_t a, int64_t e) {
        for (int64_t k = a; k < e; k++) if (blocks[k].usize && !inflate_block(z.data() + blocks[k].coff, blocks[k], f->u.data() + blocks[k].uoff)) bad = 1;
    });
    if (bad) { f->err = "inflate / CRC failure"; return GCE_ERR_INVALID; }
    f->t_inflate = now_s() - t0; t0 = now_s();
    z.release();
    // ---- header (SAMv1 4.2)
    const uint8_t *u = f->u.data(); const uint64_t n = uoff;
    BamHeader bh;
    const Hdr hs = parse_bam_header(u, n, Contigs::Collect, bh, &f->names, &f->lens);
    if (hs == Hdr::NotBam || n < 12) { f->err = "not a BAM stream"; return GCE_ERR_INVALID; }
    if (hs != Hdr::Complete) { f->err = "truncated header"; return GCE_ERR_INVALID; }
    f->text.assign((const char *)u + bh.text_off, bh.l_text);
    uint64_t p = bh.hdr_end;
    const uint32_t n_ref = bh.n_ref;
    for (auto &s : f->names) f->name_ptr.push_back(s.c_str());
    // ---- record index.  The records form a chain (every block_size leads to the next record): one dependent cache miss per record
    //      when walked by one thread.  The stream is cut into segments instead; every segment is walked from a GUESSED record start
    //      (a position where two records in a row look sane), and the pieces are then joined: segment s is accepted from the exact
    //      offset at which the verified chain of segment s - 1 leaves that segment.  A guess that never meets the true chain costs a
    //      sequential re-walk of its segment, never a wrong index.
    {
        const uint64_t first = p;
        const int32_t nref = (int32_t)n_ref;
        auto plausible = [&](uint64_t o) -> bool {                                   // does a record start at o?
            if (o + 36 > n) return false;
            const uint32_t bs = rd32(u + o);
            if (bs < 32 || bs > (1u << 24) || o + 4 + bs > n) return false;
            const uint8_t *r = u + o + 4;
            const int32_t tid = rdi32(r), mtid = rdi32(r + 20); const uint32_t lq = r[8], nc = rd16(r + 12); const int32_t ls = rdi32(r + 16);
            if (tid < -1 || tid >= nref || mtid < -1 || mtid >= nref || lq == 0 || ls < 0) return false;
            if (32ull + lq + 4ull * nc + (uint64_t)(ls + 1) / 2 + (uint64_t)ls > bs) return false;
            return r[32 + lq - 1] == 0;
        };
        const int S = (int)std::max<int64_t>(1, std::min<int64_t>(f->threads, (int64_t)((n - first) >> 22)));       // >= 4 MB per segment
        std::vector<std::vector<uint64_t>> part(S);
        std::vector<uint64_t> seg_lo(S + 1);
        for (int sg = 0; sg <= S; sg++) seg_lo[sg] = first + (n - first) * (uint64_t)sg / (uint64_t)S;
        auto walk = [&](uint64_t o, uint64_t hi, std::vector<uint64_t> &out) -> uint64_t {    // records starting in [o, hi); returns where the chain leaves
            while (o < hi && o + 4 <= n) {
                const uint32_t bs = rd32(u + o);
                if (bs < 32 || o + 4 + bs > n) return UINT64_MAX;                        // broken chain
                out.push_back(o);
                o += 4 + bs;
            }
            return o;
        };
        std::vector<uint64_t> leave(S, 0);
        parallel_for(S, S, [&](int, int64_t a, int64_t e) {
            for (int64_t sg = a; sg < e; sg++) {
                uint64_t o = seg_lo[sg];
                if (sg > 0) {                                                            // guess: first position where two records in a row look sane
                    const uint64_t lim = std::min<uint64_t>(seg_lo[sg + 1], o + (1u << 20));
                    while (o < lim && !(plausible(o) && (o + 4 + rd32(u + o) >= n - 3 || plausible(o + 4 + rd32(u + o))))) o++;
                    if (o >= lim) { leave[sg] = UINT64_MAX; continue; }
                }
                part[sg].reserve((size_t)((seg_lo[sg + 1] - seg_lo[sg]) / 200));
                leave[sg] = walk(o, seg_lo[sg + 1], part[sg]);
            }
        });
        const double t_walk = now_s();
        int rewalks = 0;
        uint64_t at = first;                                                             // where the verified chain enters the next segment
        for (int sg = 0; sg < S; sg++) {
            std::vector<uint64_t> &v = part[sg];
            size_t from = 0; bool ok = leave[sg] != UINT64_MAX;
            if (ok && at < seg_lo[sg + 1]) {                                             // (a record longer than a segment skips it entirely)
                const auto it = std::lower_bound(v.begin(), v.end(), at);
                ok = it != v.end() && *it == at; from = (size_t)(it - v.begin());
            } else if (ok) from = v.size();
            if (!ok) {                                                                   // the guess never met the chain: walk the segment for real
                rewalks++;
                v.clear(); from = 0;
                leave[sg] = at < seg_lo[sg + 1] ? walk(at, seg_lo[sg + 1], v) : at;
                if (leave[sg] == UINT64_MAX) { f->err = "truncated record"; return GCE_ERR_INVALID; }
            }
            f->rec.insert(f->rec.end(), v.begin() + from, v.end());
            if (at < seg_lo[sg + 1]) at = leave[sg];
            std::vector<uint64_t>().swap(v);
        }
        p = at;
        if (getenv("GCE_BAM_VERBOSE")) fprintf(stderr, "index: %d segments, walk %.3f s, join %.3f s, %d re-walked\n", S, t_walk - t0, now_s() - t_walk, rewalks);
    }
    if (p != n) { f->err = "trailing bytes after the last record"; return GCE_ERR_INVALID; }
    const int64_t nr = (int64_t)f->rec.size();
    std::vector<uint64_t> tq(f->threads + 1, 0), tc(f->threads + 1, 0), ts(f->threads + 1, 0), tl(f->threads + 1, 0), tm(f->threads + 1, 0);
    std::atomic<int> badrec{0};
    parallel_for(f->threads, nr, [&](int t, int64_t a, int64_t e) {
        uint64_t q = 0, c = 0, sq = 0, l = 0, m = 0;                              // (thread-local: the shared arrays would bounce between cores)
        for (int64_t k = a; k < e; k++) {
            const uint8_t *r = u + f->rec[k] + 4; const uint32_t bs = rd32(u + f->rec[k]);
            const uint32_t lq = r[8], nc = rd16(r + 12); const int32_t ls = rdi32(r + 16);
            if (lq == 0 || ls < 0 || 32ull + lq + 4ull * nc + (uint64_t)(ls + 1) / 2 + (uint64_t)ls > bs) { badrec = 1; continue; }
            q += lq; c += nc; sq += (uint64_t)(ls + 1) / 2; l += (uint64_t)ls;
            const AuxInfo ai = scan_aux(r + 32 + lq + 4 * nc + (ls + 1) / 2 + ls, r + bs);
            if (ai.mi) m += strlen(ai.mi) + 1;
        }
        tq[t] = q; tc[t] = c; ts[t] = sq; tl[t] = l; tm[t] = m;
    });
    if (badrec) { f->err = "inconsistent record lengths"; return GCE_ERR_INVALID; }
    for (int t = 0; t < f->threads; t++) { f->tot_q += tq[t]; f->tot_c += tc[t]; f->tot_s += ts[t]; f->tot_l += tl[t]; f->tot_mi += tm[t]; }
    f->t_index = now_s() - t0;
    return GCE_OK;
}

void gce_bam_close(gce_bam *f) { delete f; }
const char *gce_bam_error(const gce_bam *f) { return f ? f->err.c_str() : "null"; }

int gce_bam_get_info(const gce_bam *f, gce_bam_info *o) {
    if (!f || !o) return GCE_ERR_INVALID;
    o->n_targets = (int32_t)f->lens.size(); o->target_len = f->lens.data(); o->target_name = f->name_ptr.data();
    o->text = f->text.data(); o->l_text = (int64_t)f->text.size();
    o->n_records = (int64_t)f->rec.size();
    o->qname_bytes = f->tot_q; o->cigar_words = f->tot_c; o->seq_bytes = f->tot_s; o->qual_bytes = f->tot_l; o->mi_bytes = f->tot_mi;
    o->read_s = f->t_read; o->inflate_s = f->t_inflate; o->index_s = f->t_index;
    return GCE_OK;
}

// records [first, first + count) as a gce_batch in one of the two chunk slots (offsets relative to the slot's blobs)
// records first .. first + count - 1, or (sel != nullptr) the records sel[0 .. count - 1] in that order
static int bam_chunk_impl(gce_bam *f, int64_t first, const int64_t *sel, int64_t count, Slot &s, gce_batch *out) {
    const uint8_t *u = f->u.data();
    const int T = f->threads;
    std::vector<uint64_t> tq(T + 1, 0), tc(T + 1, 0), ts(T + 1, 0), tl(T + 1, 0), tm(T + 1, 0);
    parallel_for(T, count, [&](int t, int64_t a, int64_t e) {
        uint64_t q = 0, c = 0, sq = 0, l = 0, m = 0;
        for (int64_t k = a; k < e; k++) {
            const uint8_t *r = u + f->rec[sel ? sel[k] : first + k] + 4; const uint32_t bs = rd32(u + f->rec[sel ? sel[k] : first + k]);
            const uint32_t lq = r[8], nc = rd16(r + 12); const int32_t ls = rdi32(r + 16);
            q += lq; c += nc; sq += (uint64_t)(ls + 1) / 2; l += (uint64_t)ls;
            if (f->tot_mi) { const AuxInfo ai = scan_aux(r + 32 + lq + 4 * nc + (ls + 1) / 2 + ls, r + bs); if (ai.mi) m += strlen(ai.mi) + 1; }
        }
        tq[t + 1] = q; tc[t + 1] = c; ts[t + 1] = sq; tl[t + 1] = l; tm[t + 1] = m;
    });
    for (int t = 0; t < T; t++) { tq[t + 1] += tq[t]; tc[t + 1] += tc[t]; ts[t + 1] += ts[t]; tl[t + 1] += tl[t]; tm[t + 1] += tm[t]; }
    const bool mi = f->tot_mi != 0;
    s.core.resize(count); s.qoff.resize(count); s.coff.resize(count); s.soff.resize(count); s.loff.resize(count); s.nm.resize(count); s.nmt.resize(count);
    s.qname.resize(tq[T] + 64); s.cigar.resize(tc[T] + 16); s.seq.resize(ts[T] + 64); s.qual.resize(tl[T] + 64);
    if (mi) { s.mioff.resize(count); s.mi.resize(tm[T] + 64); }
    if (!s.core.ok() || !s.qoff.ok() || !s.coff.ok() || !s.soff.ok() || !s.loff.ok() || !s.nm.ok() || !s.nmt.ok() || !s.qname.ok() || !s.cigar.ok() || !s.seq.ok() || !s.qual.ok() ||
        (mi && (!s.mioff.ok() || !s.mi.ok()))) { f->err = "out of host memory for a batch"; return GCE_ERR_OOM; }
    const int nthreads_used = (int)std::max<int64_t>(1, std::min<int64_t>(T, count));
    parallel_for(T, count, [&](int t, int64_t a, int64_t e) {
        // parallel_for hands thread t the same range as in the counting pass, so the prefix sums are this range's start offsets
        uint64_t q = tq[t], c = tc[t], sq = ts[t], l = tl[t], m = tm[t];
        for (int64_t k = a; k < e; k++) {
            const uint8_t *r = u + f->rec[sel ? sel[k] : first + k] + 4; const uint32_t bs = rd32(u + f->rec[sel ? sel[k] : first + k]);
            memcpy(&s.core[k], r, 32);                                        // gce_core IS the 32-byte BAM core block
            const uint32_t lq = r[8], nc = rd16(r + 12); const int32_t ls = rdi32(r + 16);
            const uint8_t *pq = r + 32, *pc = pq + lq, *ps = pc + 4 * nc, *pl = ps + (ls + 1) / 2, *pa = pl + ls;
            s.qoff[k] = q; memcpy(s.qname.data() + q, pq, lq); q += lq;
            s.coff[k] = c; memcpy(s.cigar.data() + c, pc, 4 * nc); c += nc;
            s.soff[k] = sq; memcpy(s.seq.data() + sq, ps, (ls + 1) / 2); sq += (uint64_t)(ls + 1) / 2;
            s.loff[k] = l; memcpy(s.qual.data() + l, pl, ls); l += (uint64_t)ls;
            const AuxInfo ai = scan_aux(pa, r + bs);
            s.nmt[k] = ai.nm_type; s.nm[k] = ai.nm;
            if (mi) {
                if (ai.mi) { const size_t n = strlen(ai.mi) + 1; s.mioff[k] = m; memcpy(s.mi.data() + m, ai.mi, n); m += n; }
                else s.mioff[k] = UINT64_MAX;
            }
        }
    });
    (void)nthreads_used;
    memset(out, 0, sizeof *out);
    out->n_reads = count; out->core = s.core.data();
    out->qname_off = s.qoff.data(); out->qname = s.qname.data(); out->cigar_off = s.coff.data(); out->cigar = s.cigar.data();
    out->seq_off = s.soff.data(); out->seq = s.seq.data(); out->qual_off = s.loff.data(); out->qual = s.qual.data();
    out->nm = s.nm.data(); out->nm_type = s.nmt.data();
    if (mi) { out->mi_off = s.mioff.data(); out->mi = s.mi.data(); out->mi_bytes = tm[T]; }
    out->qname_bytes = tq[T]; out->cigar_words = tc[T]; out->seq_bytes = ts[T]; out->qual_bytes = tl[T];
    return GCE_OK;
}

// Gencore::writeBam for every row of the result (src/gencore.cpp:85-111): the input record res->src[k] with the row's bases,
// qualities, name (BamUtil::copyQName, src/bamutil.cpp:338-364), NM byte (src/group.cpp:570) and FR / RR aux (src/pair.cpp:57-67).

int gce_bam_chunk(gce_bam *f, int64_t first, int64_t count, int slot_id, gce_batch *out) {
    if (!f || !out || first < 0 || count < 0 || first + count > (int64_t)f->rec.size() || (slot_id != 0 && slot_id != 1)) return GCE_ERR_INVALID;
    return bam_chunk_impl(f, first, nullptr, count, f->slot[slot_id], out);
}

// the rows of an output table as BAM records: row k = input record src[k] with the name of record qname_src[k], the bases / qualities
// at seqp(k) / qualp(k), NM patched, FR / RR appended (gce_result's meaning; one table, or several engines' tables merged)
struct OutRows { int64_t n; const uint32_t *src, *qname_src; const int32_t *nm_new; const int16_t *fr, *rr; };
extern "C++" {
template <class SP, class QP>
static int bam_write_rows(const char *path, const gce_bam *in, const OutRows rows, SP seqp, QP qualp, int threads, int level) {
    const OutRows *res = &rows;
    const int T = threads > 0 ? threads : in->threads;
    const uint8_t *u = in->u.data();
    const int64_t n = rows.n;
    for (int64_t k = 0; k < n; k++) if (res->src[k] >= in->rec.size() || res->qname_src[k] >= in->rec.size()) return GCE_ERR_INVALID;
    // ---- header bytes
    std::vector<uint8_t> hdr;
    auto put32 = [&](std::vector<uint8_t> &v, uint32_t x) { const uint8_t *p = (const uint8_t *)&x; v.insert(v.end(), p, p + 4); };
    hdr.insert(hdr.end(), {'B', 'A', 'M', 1});
    put32(hdr, (uint32_t)in->text.size()); hdr.insert(hdr.end(), in->text.begin(), in->text.end());
    put32(hdr, (uint32_t)in->lens.size());
    for (size_t r = 0; r < in->lens.size(); r++) {
        put32(hdr, (uint32_t)in->names[r].size() + 1);
        hdr.insert(hdr.end(), in->names[r].begin(), in->names[r].end()); hdr.push_back(0);
        put32(hdr, in->lens[r]);
    }
    // ---- record sizes, then the records
    std::vector<uint64_t> roff((size_t)n + 1, 0);
    parallel_for(T, n, [&](int, int64_t a, int64_t e) {
        for (int64_t k = a; k < e; k++) {
            const uint64_t ro = in->rec[res->src[k]]; const uint32_t bs = rd32(u + ro);
            const uint32_t lq_old = u[ro + 4 + 8], lq_new = u[in->rec[res->qname_src[k]] + 4 + 8];
            roff[k + 1] = 4ull + bs - lq_old + lq_new + (res->fr[k] >= 0 ? 4 : 0) + (res->rr[k] >= 0 ? 4 : 0);
        }
    });
    for (int64_t k = 0; k < n; k++) roff[k + 1] += roff[k];
    Raw<uint8_t> body; body.resize(hdr.size() + roff[n]);
    if (!body.ok()) return GCE_ERR_OOM;
    memcpy(body.data(), hdr.data(), hdr.size());
    uint8_t *rb = body.data() + hdr.size();
    parallel_for(T, n, [&](int, int64_t a, int64_t e) {
        for (int64_t k = a; k < e; k++) {
            const uint8_t *r = u + in->rec[res->src[k]] + 4; const uint32_t bs = rd32(r - 4);
            const uint8_t *nr = u + in->rec[res->qname_src[k]] + 4;
            const uint32_t lq_old = r[8], lq_new = nr[8], nc = rd16(r + 12); const int32_t ls = rdi32(r + 16);
            uint8_t *o = rb + roff[k];
            const uint32_t nbs = (uint32_t)(roff[k + 1] - roff[k] - 4);
            memcpy(o, &nbs, 4); memcpy(o + 4, r, 32);
            o[4 + 8] = (uint8_t)lq_new;
            uint8_t *w = o + 36;
            memcpy(w, nr + 32, lq_new); w += lq_new;
            memcpy(w, r + 32 + lq_old, 4 * nc); w += 4 * nc;
            memcpy(w, seqp(k), (ls + 1) / 2); w += (ls + 1) / 2;
            memcpy(w, qualp(k), ls); w += ls;
            const uint8_t *aux = r + 32 + lq_old + 4 * nc + (ls + 1) / 2 + ls; const size_t al = (size_t)(r + bs - aux);
            memcpy(w, aux, al);
            if (res->nm_new[k] >= 0) {                                       // dataNM[1] = newValNM (type 'C' only, checked by the engine)
                uint8_t *p = w, *end = w + al;
                while (p + 3 <= end) {
                    const size_t sz = aux_size(p[2], p + 3, end);
                    if (sz == SIZE_MAX) break;
                    if (p[0] == 'N' && p[1] == 'M') { p[3] = (uint8_t)res->nm_new[k]; break; }
                    p += 3 + sz;
                }
            }
            w += al;
            if (res->fr[k] >= 0) { w[0] = 'F'; w[1] = 'R'; w[2] = 'C'; w[3] = (uint8_t)res->fr[k]; w += 4; }
            if (res->rr[k] >= 0) { w[0] = 'R'; w[1] = 'R'; w[2] = 'C'; w[3] = (uint8_t)res->rr[k]; w += 4; }
        }
    });
    return write_bgzf(path, body, T, level);
}
}  // extern "C++"

int gce_bam_write(const char *path, const gce_bam *in, const gce_result *res, int threads, int level) {
    if (!path || !in || !res) return GCE_ERR_INVALID;
    const OutRows rows{res->n_out, res->src, res->qname_src, res->nm_new, res->fr, res->rr};
    return bam_write_rows(path, in, rows, [&](int64_t k) { return res->seq + res->seq_off[k]; }, [&](int64_t k) { return res->qual + res->qual_off[k]; }, threads, level);
}

// The inverse of gce_bam_chunk: a gce_batch (host pointers) as a BAM file -- header, one record per read with its NM tag (type and
// value as given) and MI:Z tag.  Used to materialise synthetic streams as files (tools/bam_bench.py, tests).
int gce_bam_from_batch(const char *path, const gce_batch *b, int32_t n_targets, const uint32_t *target_len, const char *const *target_name,
                       const char *text, int threads, int level) {
    if (!path || !b || n_targets < 0) return GCE_ERR_INVALID;
    const int T = threads > 0 ? threads : default_threads();
    std::vector<uint8_t> hdr;
    auto put32 = [&](std::vector<uint8_t> &v, uint32_t x) { const uint8_t *p = (const uint8_t *)&x; v.insert(v.end(), p, p + 4); };
    const std::string tx = text ? text : "";
    hdr.insert(hdr.end(), {'B', 'A', 'M', 1});
    put32(hdr, (uint32_t)tx.size()); hdr.insert(hdr.end(), tx.begin(), tx.end());
    put32(hdr, (uint32_t)n_targets);
    for (int32_t r = 0; r < n_targets; r++) {
        const std::string nm = target_name && target_name[r] ? target_name[r] : ("contig" + std::to_string(r));
        put32(hdr, (uint32_t)nm.size() + 1); hdr.insert(hdr.end(), nm.begin(), nm.end()); hdr.push_back(0);
        put32(hdr, target_len[r]);
    }
    const int64_t n = b->n_reads;
    auto nm_bytes = [](uint8_t t) -> size_t { return t == 0 ? 0 : 3 + ((t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : 4); };
    std::vector<uint64_t> roff((size_t)n + 1, 0);
    parallel_for(T, n, [&](int, int64_t a, int64_t e) {
        for (int64_t k = a; k < e; k++) {
            const gce_core &c = b->core[k];
            size_t mi = 0;
            if (b->mi && b->mi_off && b->mi_off[k] != UINT64_MAX) mi = 3 + strlen(b->mi + b->mi_off[k]) + 1;
            roff[k + 1] = 4ull + 32 + c.l_qname + 4ull * c.n_cigar + (uint64_t)(c.l_qseq + 1) / 2 + (uint64_t)c.l_qseq + nm_bytes(b->nm_type[k]) + mi;
        }
    });
    for (int64_t k = 0; k < n; k++) roff[k + 1] += roff[k];
    Raw<uint8_t> body; body.resize(hdr.size() + roff[n]);
    if (!body.ok()) return GCE_ERR_OOM;
    memcpy(body.data(), hdr.data(), hdr.size());
    uint8_t *rb = body.data() + hdr.size();
    parallel_for(T, n, [&](int, int64_t a, int64_t e) {
        for (int64_t k = a; k < e; k++) {
            const gce_core &c = b->core[k];
            uint8_t *o = rb + roff[k];
            const uint32_t bs = (uint32_t)(roff[k + 1] - roff[k] - 4);
            memcpy(o, &bs, 4); memcpy(o + 4, &c, 32);
            uint8_t *w = o + 36;
            memcpy(w, b->qname + b->qname_off[k], c.l_qname); w += c.l_qname;
            memcpy(w, b->cigar + b->cigar_off[k], 4ull * c.n_cigar); w += 4ull * c.n_cigar;
            memcpy(w, b->seq + b->seq_off[k], (c.l_qseq + 1) / 2); w += (c.l_qseq + 1) / 2;
            memcpy(w, b->qual + b->qual_off[k], c.l_qseq); w += c.l_qseq;
            const uint8_t t = b->nm_type[k];
            if (t) {
                w[0] = 'N'; w[1] = 'M'; w[2] = t;
                const int32_t v = b->nm[k];
                const size_t sz = nm_bytes(t) - 3;
                memcpy(w + 3, &v, sz);                                           // little endian: the low bytes are the value
                w += 3 + sz;
            }
            if (b->mi && b->mi_off && b->mi_off[k] != UINT64_MAX) {
                const char *m = b->mi + b->mi_off[k]; const size_t ml = strlen(m) + 1;
                w[0] = 'M'; w[1] = 'I'; w[2] = 'Z'; memcpy(w + 3, m, ml); w += 3 + ml;
            }
        }
    });
    return write_bgzf(path, body, T, level);
}

// SAM text -> BAM and back on the host alone (no engine, no GPU): what sam_read1 / sam_write1 do when the reference is given SAM text
// (src/gencore.cpp:164-173,205,104 via htslib); gce_run_bam takes and writes SAM text through the same line functions (gce_samtext.hpp).
int gce_sam_to_bam(const char *sam_path, const char *bam_path, int threads, int level, char err[256]) {
    auto fail = [&](const char *m) { set_err(err, m); return GCE_ERR_INVALID; };
    set_err(err, "");
    if (!sam_path || !bam_path) return GCE_ERR_INVALID;
    const int T = threads > 0 ? threads : default_threads();
    std::vector<char> tx;
    if (!read_file(sam_path, tx)) return fail("cannot read the input SAM");
    if (!tx.empty() && tx.back() != '\n') tx.push_back('\n');
    const char *d = tx.data(); const size_t lim = tx.size();
    size_t p = 0; std::string text;
    while (p < lim && d[p] == '@') { const char *q = (const char *)memchr(d + p, '\n', lim - p); const size_t z = (size_t)(q - d) + 1; text.append(d + p, z - p); p = z; }
    std::vector<std::string> names; std::vector<uint32_t> lens;
    if (!samtext::parse_header_text(text, names, lens)) return fail("bad @SQ line");
    samtext::NameMap nmap; nmap.build(names);
    std::vector<std::vector<uint8_t>> parts; std::vector<std::string> perr;
    if (const char *m = lines_to_records(d, p, lim, T, nmap, parts, perr)) return fail(m);
    const std::vector<uint8_t> hdr = bam_header_bytes(text, names, lens);
    size_t tot = hdr.size(); for (auto &v : parts) tot += v.size();
    Raw<uint8_t> body; body.resize(tot);
    if (!body.ok()) return GCE_ERR_OOM;
    memcpy(body.data(), hdr.data(), hdr.size());
    size_t o = hdr.size(); for (auto &v : parts) { if (!v.empty()) memcpy(body.data() + o, v.data(), v.size()); o += v.size(); }
    const int rc = write_bgzf(bam_path, body, T, level);
    if (rc != GCE_OK) fail("cannot write the output BAM");
    return rc;
}

int gce_bam_to_sam(const char *bam_path, const char *sam_path, int threads, char err[256]) {
    auto fail = [&](const char *m) { set_err(err, m); return GCE_ERR_INVALID; };
    set_err(err, "");
    if (!bam_path || !sam_path) return GCE_ERR_INVALID;
    const int T = threads > 0 ? threads : default_threads();
    gce_bam *f = nullptr;
    const int rc = gce_bam_open(bam_path, T, &f);
    if (rc != GCE_OK) { fail(f ? f->err.c_str() : "cannot open the input BAM"); if (f) gce_bam_close(f); return rc; }
    OutFile of;
    if (!of.open(sam_path, true)) { gce_bam_close(f); return fail("cannot open the output SAM"); }
    bool ok = of.sam_header(f->text, f->names, f->lens);
    std::vector<std::string> lines;
    const bool bad = !records_to_lines(f->u.data(), f->rec, f->names, T, lines);
    for (int t = 0; t < T && ok && !bad; t++) ok = of.write(lines[(size_t)t].data(), lines[(size_t)t].size());
    ok = of.close() && ok;
    gce_bam_close(f);
    if (bad) return fail("bad record in the input BAM");
    return ok ? GCE_OK : fail("cannot write the output SAM");
}

// ------------------------------------------------------------------------------------------------------------ FASTA
// FastaReader(file) + readAll (src/fastareader.cpp:7-41,57-104,157-168) with its quirks: the FIRST character of every line is
// taken by get(c) and appended without the validity filter of str_keep_valid_sequence (util.h:194-210) -- an empty line inside a
// contig therefore contributes its '\n' as one base (code 0) and the line after it is taken whole; lower case is folded
// (forceUpperCase = true, fastareader.h:21); the contig ID is the header up to the first blank.  Later contigs of the same name
// replace earlier ones (std::map assignment).  Returns the contigs as upper-cased ASCII, ready for gce_set_reference_ascii.
//
// The walk of FastaReader::readNext is a chain of ITERATIONS: get(c) takes one character -- '>' ends the record, anything else goes
// unfiltered into the header (first iteration of a record) or the sequence --, then getline takes the rest of the line.  Where an
// iteration starts depends on the file only through its line feeds, so the file (read by parallel preads) is cut into one range per
// thread at positions that are PROVABLY iteration starts: a position q with d[q-1] == '\n' and d[q-2] neither '\n' nor '>' (that
// line feed cannot be the first character of an iteration, because the character in front of it neither ended an iteration nor was
// a one-character '>' iteration: it ends one, and q starts the next; q is never the start of a header iteration, which follows a
// '>').  Every thread then walks its iterations exactly as the reference does; the pieces are stitched per contig.  threads == 1 is
// the literal one-pass walk (the test oracle of the parallel one); a file without such cut positions falls back to it.
struct FaPiece { int64_t hdr_a = -1, hdr_b = -1; char *seq = nullptr; size_t n = 0; };     // one (part of a) record seen by one thread: a slice of the thread's arena
struct gce_fasta {
    std::vector<std::string> ids; std::vector<Raw<char>> seqs, arena; Raw<uint8_t> file; std::vector<const char *> idp, seqp; std::vector<int64_t> len;
    double t_map = 0, t_parse = 0, t_stitch = 0;
};

namespace {
inline char fa_upper(char c) { return (c >= 'a' && c <= 'z') ? (char)(c - ('a' - 'A')) : c; }
// walk the iterations of [p, end): `end` is an iteration start (or the file's end).  `in_header`: the first iteration is a header's.
// Sequence characters are appended to pieces.back(); a '>' iteration opens a new piece whose header follows.
void fa_walk(const uint8_t *d, size_t n, size_t p, size_t end, bool in_header, std::vector<FaPiece> &pieces, char *arena) {
    // (an iteration never emits more characters than it consumes: the arena, as long as the range, cannot overflow)
    bool header_next = in_header;
    char *o = arena;
    pieces.back().seq = o;
    while (p < end) {
        const char c = (char)d[p++];
        if (c == '>') { pieces.back().n = (size_t)(o - pieces.back().seq); pieces.emplace_back(); pieces.back().seq = o; header_next = true; continue; }   // `if(c == '>' || eof) break;` -- in a header iteration too: that record has an empty header
        size_t e = p;
        if (e < n) { const void *nl = memchr(d + p, '\n', n - p); e = nl ? (size_t)((const uint8_t *)nl - d) : n; }
        if (header_next) { pieces.back().hdr_a = (int64_t)p - 1; pieces.back().hdr_b = (int64_t)e; header_next = false; }   // header = c + rest of the line
        else {
            *o++ = fa_upper(c);                                                                      // get(c): no validity filter
            for (size_t k = p; k < e; k++) { const char ch = fa_upper((char)d[k]); if ((ch >= 'A' && ch <= 'Z') || ch == '-' || ch == '*') *o++ = ch; }   // str_keep_valid_sequence (util.h:194-210); isalpha after the fold = A-Z
        }
        p = e < n ? e + 1 : n;
    }
    pieces.back().n = (size_t)(o - pieces.back().seq);
}
}  // namespace

int gce_fasta_load(const char *path, int threads, gce_fasta **out) {
    if (!path || !out) return GCE_ERR_INVALID;
    *out = nullptr;
    double t0 = now_s();
    int T = threads > 0 ? threads : default_threads();
    gce_fasta *fa = new gce_fasta();
    *out = fa;
    if (!read_file_parallel(path, fa->file, T)) return GCE_ERR_INVALID;          // parallel preads into one 2 MB-page buffer (page faults of an mmap'ed file
    const size_t n = fa->file.size();                                              //  from eight threads, next to their allocations, serialised on the mm lock: slower than one thread)
    const uint8_t *d = fa->file.data();
    fa->t_map = now_s() - t0; t0 = now_s();
    size_t p0 = 0;
    while (p0 < n && d[p0] != '>') p0++;                                      // seek to the first contig
    if (p0 < n) p0++;
    std::vector<std::vector<FaPiece>> per;
    if (p0 < n) {
        // ---- cut positions
        { const char *mb = getenv("GCE_FASTA_MIN_PARALLEL"); const size_t min_par = mb ? (size_t)atoll(mb) : (size_t)(1 << 20); if ((n - p0) < min_par) T = 1; }   // (tests set it to 0)
        std::vector<size_t> cut{p0};
        for (int t = 1; t < T; t++) {
            size_t q = std::max(p0 + (n - p0) / T * t, cut.back() + 2);
            const size_t lim = std::min(n, q + (size_t)(16 << 20));              // (a cut is found within a line or two; give up on odd files)
            for (; q < lim; q++) if (d[q - 1] == '\n' && d[q - 2] != '\n' && d[q - 2] != '>' && q - 2 >= p0) break;
            if (q >= lim) { cut.assign(1, p0); break; }                          // no provable iteration start: one thread walks it all
            if (q > cut.back()) cut.push_back(q);
        }
        const int nt = (int)cut.size();
        cut.push_back(n);
        per.resize(nt); fa->arena.resize(nt);
        for (int t = 0; t < nt; t++) { fa->arena[t].resize(cut[t + 1] - cut[t] + 64); if (!fa->arena[t].ok()) return GCE_ERR_OOM; }   // (all allocations in front of the threads)
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++) th.emplace_back([&, t] {
            per[t].emplace_back();                                               // thread 0: the first record; others: the record that is open at the cut
            fa_walk(d, n, cut[t], cut[t + 1], t == 0, per[t], fa->arena[t].data());
        });
        for (auto &x : th) x.join();
    }
    fa->t_parse = now_s() - t0; t0 = now_s();
    // ---- stitch: a thread's first piece continues the last piece of the thread in front of it (unless it is thread 0's)
    struct Rec { std::string hdr; std::vector<std::pair<int, int>> parts; size_t total = 0; };
    std::vector<Rec> recs;
    bool any = false;
    for (size_t t = 0; t < per.size(); t++)
        for (size_t k = 0; k < per[t].size(); k++) {
            FaPiece &pc = per[t][k];
            if (!(t > 0 && k == 0)) { recs.emplace_back(); if (pc.hdr_a >= 0) recs.back().hdr.assign((const char *)d + pc.hdr_a, (size_t)(pc.hdr_b - pc.hdr_a)); }
            recs.back().parts.emplace_back((int)t, (int)k); recs.back().total += pc.n; any = true;
        }
    (void)any;
    // readAll (fastareader.cpp:157-168): `while(!eof) readNext()` -- a record that a '>' opened right at the end of the file exists
    // (empty id, empty sequence) exactly when the walk above produced its piece; contigs of the same id: the LAST one stays, at the
    // place of the first (std::map assignment).
    std::unordered_map<std::string, size_t> where;
    std::vector<int64_t> rec_of;                                               // contig -> record that supplies its sequence
    for (size_t r = 0; r < recs.size(); r++) {
        const size_t sp = recs[r].hdr.find(' ');
        const std::string id = recs[r].hdr.substr(0, sp);
        auto it = where.find(id);
        if (it == where.end()) { where.emplace(id, fa->ids.size()); fa->ids.push_back(id); rec_of.push_back((int64_t)r); }
        else rec_of[it->second] = (int64_t)r;
    }
    fa->seqs.resize(fa->ids.size()); fa->seqp.assign(fa->ids.size(), nullptr); fa->len.assign(fa->ids.size(), 0);
    static const char empty_seq[1] = {0};
    {
        std::vector<std::thread> th;                                           // a contig inside one thread's range stays where it is; one that spans ranges is
        for (size_t c = 0; c < fa->ids.size(); c++) {                          // copied together, one thread per part
            Rec &r = recs[(size_t)rec_of[c]];
            fa->len[c] = (int64_t)r.total;
            if (r.total == 0) { fa->seqp[c] = empty_seq; continue; }
            if (r.parts.size() == 1) { fa->seqp[c] = per[r.parts[0].first][r.parts[0].second].seq; continue; }
            fa->seqs[c].resize(r.total + 1);
            if (!fa->seqs[c].ok()) { for (auto &x : th) x.join(); return GCE_ERR_OOM; }
            fa->seqp[c] = fa->seqs[c].p;
            size_t at = 0;
            for (auto &pr : r.parts) { const FaPiece *pc = &per[pr.first][pr.second]; char *dst = fa->seqs[c].p + at; if (pc->n) th.emplace_back([pc, dst] { memcpy(dst, pc->seq, pc->n); }); at += pc->n; }
        }
        for (auto &x : th) x.join();
    }
    fa->file.release();
    for (size_t k = 0; k < fa->ids.size(); k++) fa->idp.push_back(fa->ids[k].c_str());
    fa->t_stitch = now_s() - t0;
    if (getenv("GCE_FASTA_TIMING")) fprintf(stderr, "gce_fasta_load: %zu bytes, %d threads: map %.3f s, parse %.3f s, stitch %.3f s\n", n, (int)per.size(), fa->t_map, fa->t_parse, fa->t_stitch);
    return GCE_OK;
}
int gce_fasta_get(const gce_fasta *fa, int32_t *n, const char *const **ids, const char *const **seqs, const int64_t **lens) {
    if (!fa || !n) return GCE_ERR_INVALID;
    *n = (int32_t)fa->ids.size();
    if (ids) *ids = fa->idp.data();
    if (seqs) *seqs = fa->seqp.data();
    if (lens) *lens = fa->len.data();
    return GCE_OK;
}
void gce_fasta_free(gce_fasta *fa) { delete fa; }

// ------------------------------------------------------------------------------------------------------------ BED
// Bed::loadFromFile (src/bed.cpp:111-168) with util.h's trim / split (util.h:44-85).  An empty (or blank-only) line indexes an
// empty vector in the reference (undefined behaviour); it is skipped here.
int gce_bed_load(const char *path, int32_t n_targets, const char *const *target_name, int32_t *n_regions, int32_t **tid_out, int32_t **start_out,
                 int32_t **end_out, char ***name_out) {
    if (!path || !n_regions || !tid_out || !start_out || !end_out) return GCE_ERR_INVALID;
    std::vector<uint8_t> d;
    if (!read_file(path, d)) return GCE_ERR_INVALID;
    auto trim = [](const std::string &x) -> std::string {                          // spaces only (util.h:44-57)
        const size_t a = x.find_first_not_of(' ');
        if (a == std::string::npos) return "";
        const size_t b = x.find_last_not_of(' ');
        return x.substr(a, b - a + 1);
    };
    std::vector<int32_t> tids, starts, ends; std::vector<std::string> names;
    size_t p = 0; const size_t n = d.size();
    while (p < n) {                                                                // file.getline(line, 4096)
        size_t e = p;
        while (e < n && d[e] != '\n') e++;
        if (e - p > 4095) break;                                                   // the line does not fit the buffer: failbit, the loop ends
        std::string line((const char *)d.data() + p, e - p);
        const size_t nul = line.find('\0');                                        // strlen(line)
        if (nul != std::string::npos) line.resize(nul);
        p = e < n ? e + 1 : n;
        if (line.size() >= 2 && line.back() == '\r') { line.pop_back(); if (line.back() == '\r') line.pop_back(); }      // bed.cpp:126-133
        line = trim(line);
        std::vector<std::string> tok;                                              // split(linestr, "\t") (util.h:59-85)
        if (!line.empty()) {
            size_t b = line.find_first_not_of('\t');
            while (b != std::string::npos) {
                const size_t c = line.find('\t', b);
                if (c != std::string::npos) { tok.push_back(line.substr(b, c - b)); b = c + 1; }
                else { tok.push_back(line.substr(b)); b = c; }
            }
        }
        if (tok.empty()) continue;
        if (tok[0].compare(0, 1, "#") == 0) continue;                              // bed.cpp:139-140
        if (tok.size() < 3) continue;                                              // :142-143
        const std::string chr = trim(tok[0]);
        int tid = -1;
        for (int32_t t = 0; t < n_targets; t++) if (target_name && target_name[t] && chr == target_name[t]) tid = t;   // :154-162 (the last match wins)
        tids.push_back(tid); starts.push_back(atoi(trim(tok[1]).c_str())); ends.push_back(atoi(trim(tok[2]).c_str()));
        names.push_back(tok.size() > 3 ? trim(tok[3]) : "");
    }
    const size_t m = tids.size();
    *n_regions = (int32_t)m;
    *tid_out = (int32_t *)malloc(std::max<size_t>(m, 1) * 4); *start_out = (int32_t *)malloc(std::max<size_t>(m, 1) * 4); *end_out = (int32_t *)malloc(std::max<size_t>(m, 1) * 4);
    memcpy(*tid_out, tids.data(), m * 4); memcpy(*start_out, starts.data(), m * 4); memcpy(*end_out, ends.data(), m * 4);
    if (name_out) {
        *name_out = (char **)malloc(std::max<size_t>(m, 1) * sizeof(char *));
        for (size_t k = 0; k < m; k++) (*name_out)[k] = strdup(names[k].c_str());
    }
    return GCE_OK;
}
void gce_bed_free(int32_t n_regions, int32_t *tid, int32_t *start, int32_t *end, char **name) {
    free(tid); free(start); free(end);
    if (name) { for (int32_t k = 0; k < n_regions; k++) free(name[k]); free(name); }
}

extern "C++" {
namespace {
// ---- what every runner does once the contig table is known
inline bool umi_auto(const gce_params &prm) { return strcmp(prm.umi_prefix, "auto") == 0; }
// the contig table into the engine's parameters; the "auto" UMI prefix from the first record's name, or none without one (src/gencore.cpp:207-220)
void file_params(gce_params &prm, int32_t n_targets, const uint32_t *target_len, const char *first_qname) {
    prm.n_targets = n_targets; prm.target_len = target_len;
    if (!umi_auto(prm)) return;
    memset(prm.umi_prefix, 0, sizeof prm.umi_prefix);
    if (first_qname) gce_detect_umi_prefix(first_qname, prm.umi_prefix);
}
inline bool same_name(const char *a, const char *b) { return strcmp(a, b) == 0; }
inline bool same_name(const std::string &a, const char *b) { return a == b; }
// Reference::getData looks contigs up by BAM target name (reference.cpp:43-53): every contig of names[0, n) that the loaded FASTA has goes to
// the engine; the first status that is not GCE_OK is returned (gce_last_error(e) says why)
template <class Name> int set_reference(gce_engine *e, const gce_fasta *fa, const Name *names, size_t n) {
    int32_t nc = 0; const char *const *ids = nullptr; const char *const *seqs = nullptr; const int64_t *flen = nullptr; int rc;
    gce_fasta_get(fa, &nc, &ids, &seqs, &flen);
    for (size_t t = 0; t < n; t++)
        for (int32_t c = 0; c < nc; c++)
            if (same_name(names[t], ids[c]) && (rc = gce_set_reference_ascii(e, (int32_t)t, seqs[c], flen[c])) != GCE_OK) return rc;
    return GCE_OK;
}
// the depth report's arrays (freed by gce_depth_run_free), n_regions being set: bins of coverage_step per contig, contigs back to back.  false: out of host memory
bool depth_alloc(gce_depth_run *depth, const std::vector<uint32_t> &lens, int32_t coverage_step) {
    const int nt = (int)lens.size();
    depth->n_targets = nt;
    depth->bin_off = (int64_t *)calloc((size_t)nt + 1, 8);
    if (!depth->bin_off) return false;
    for (int t = 0; t < nt; t++) depth->bin_off[t + 1] = depth->bin_off[t] + 1 + (int64_t)lens[(size_t)t] / coverage_step;
    const int64_t nb = depth->bin_off[nt];
    depth->n_bins = nb;
    depth->pre_depth = (int64_t *)calloc((size_t)std::max<int64_t>(nb, 1), 8); depth->post_depth = (int64_t *)calloc((size_t)std::max<int64_t>(nb, 1), 8);
    depth->pre_bed = (int64_t *)calloc((size_t)std::max(depth->n_regions, 1), 8); depth->post_bed = (int64_t *)calloc((size_t)std::max(depth->n_regions, 1), 8);
    depth->payload_bytes = (2 * (int64_t)GCE_STATS_WORDS + 2 * nb + 2 * (int64_t)depth->n_regions) * 8;
    return depth->pre_depth && depth->post_depth && depth->pre_bed && depth->post_bed;
}
// the payload's words (gce_payload_layout: two Stats blocks in stats_words words, then the depth and BED blocks) into those arrays
void depth_unpack(gce_depth_run *depth, const int64_t *words, int64_t stats_words) {
    const int64_t nb = depth->n_bins; const int32_t nreg = depth->n_regions;
    memcpy(&depth->pre, words, sizeof(gce_stats)); memcpy(&depth->post, words + GCE_STATS_WORDS, sizeof(gce_stats));
    const int64_t *d0 = words + stats_words;
    memcpy(depth->pre_depth, d0, (size_t)nb * 8); memcpy(depth->post_depth, d0 + nb, (size_t)nb * 8);
    memcpy(depth->pre_bed, d0 + 2 * nb, (size_t)nreg * 8); memcpy(depth->post_bed, d0 + 2 * nb + nreg, (size_t)nreg * 8);
}
}  // namespace
}  // extern "C++"

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



// ---- the streaming, GPU-assisted file path
int gce_raw_begin(gce_engine *e, size_t capacity_hint);
int gce_raw_push(gce_engine *e, const void *host, size_t bytes, int32_t *ticket);
int gce_raw_finish(gce_engine *e, uint64_t records_begin, int32_t n_ref, int64_t *n_records);
int gce_raw_build_output(gce_engine *e, uint64_t *body_bytes, int64_t *n_out);
int gce_raw_read_output_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket);
int gce_host_alloc(size_t bytes, void **out);
int gce_raw_deflate_output(gce_engine *e, uint64_t *comp_bytes);
int gce_raw_deflate_output_codes(gce_engine *e, int32_t codes, uint64_t *comp_bytes);
int gce_raw_read_deflated_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket);
int gce_raw_attach_mirror(gce_engine *e, gce_engine *mirror);
int gce_raw_select_shard(gce_engine *e, int32_t world, int32_t rank, int32_t plan_mode);
int gce_stats_payload_device(gce_engine *e, int32_t coverage_step, int32_t n_regions, const int32_t *region_tid, const int32_t *region_start, const int32_t *region_end, const int64_t **payload, gce_payload_layout *layout);
int gce_stats_payload_sum(gce_engine **engs, int32_t n_engs, const int64_t **payload, gce_payload_layout *layout);
int gce_stats_payload_read(gce_engine *e, const int64_t *payload, int64_t n_words, int64_t *host);
int gce_raw_merge_outputs(gce_engine **engs, int32_t n_engs, uint64_t *body_bytes, int64_t *n_out_total, gce_stats *pre, gce_stats *post, int64_t *n_reads_total);
void gce_host_free(void *p);
}  // extern "C" (declarations)
extern "C++" {
namespace {
struct Pinned {                                   // a pinned host buffer that grows
    uint8_t *p = nullptr; size_t cap = 0;
    ~Pinned() { gce_host_free(p); }
    bool ensure(size_t n) { if (n <= cap) return true; gce_host_free(p); p = nullptr; cap = 0; void *q = nullptr; if (gce_host_alloc(n + (n >> 3) + 4096, &q) != GCE_OK) return false; p = (uint8_t *)q; cap = n + (n >> 3) + 4096; return true; }
};
long status_kb(const char *key) { FILE *f = fopen("/proc/self/status", "r"); if (!f) return 0; char line[256]; long v = 0; const size_t kl = strlen(key); while (fgets(line, sizeof line, f)) if (strncmp(line, key, kl) == 0) { v = atol(line + kl); break; } fclose(f); return v; }
}  // namespace
}  // extern "C++"
extern "C" {

// Replaces Gencore::consensus() end to end (src/gencore.cpp:162-293) as a PIPELINE with a bounded host footprint: a reader thread preads the
// file in pieces; the host threads inflate the BGZF blocks of piece k (own decoder + CLMUL CRC) into a pinned window while the DMA engine
// copies window k - 1 into HBM; nothing of the input stays on the host.  Records are indexed, parsed (gce_raw_finish) and -- after
// gce_process -- re-assembled as BAM records (gce_raw_build_output) on the GPU; the output stream comes back in pieces that are deflated by
// all host threads and written in order while the next piece is on its way.  Host memory: two compressed pieces, three inflated windows,
// three output pieces -- independent of the file's size (round 2 held the whole inflated file and every record table on the host).
// gce_run_bam (n_shards == 1) and gce_run_bam_sharded over the same pipeline: with several shards every piece of the file goes to one engine per
// entry of `devices` (the mirrors of the first), each inflates and indexes the stream on its own GPU, plans it there and keeps its share
// (gce_raw_select_shard); the record streams are merged on the first engine's device (gce_raw_merge_outputs) and written as one.
static int run_bam_impl(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int threads,
                        int64_t chunk_reads, int level, gce_bam_run *out, char err[256], int32_t n_shards, const int32_t *devices, int32_t plan_mode,
                        const char *bed_path = nullptr, int32_t coverage_step = 0, gce_depth_run *depth = nullptr) {
    set_err(err, "");
    if (!in_path || !out_path || !params || !out) return GCE_ERR_INVALID;
    memset(out, 0, sizeof *out);
    out->rss_start_kb = status_kb("VmRSS:");
    const double t_start = now_s();
    const int T = threads > 0 ? threads : default_threads();
    const int fd = open(in_path, O_RDONLY);
    if (fd < 0) { set_err(err, "cannot open the input BAM"); return GCE_ERR_INVALID; }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 0) { close(fd); set_err(err, "cannot stat the input BAM"); return GCE_ERR_INVALID; }
    const uint64_t fsz = (uint64_t)st.st_size;
    gce_engine *e = nullptr; gce_fasta *fa = nullptr; OutFile of;
    std::vector<gce_engine *> mir;                      // the engines of shards 1 .. n_shards - 1 (they receive every push made to e)
    std::thread reader; ssize_t got_next = 0; bool reader_on = false;      // the BAM branch's read-ahead of the next piece (start_read); done joins it
    auto done = [&](int code, const char *m) { if (reader_on) { reader.join(); reader_on = false; } set_err(err, m); for (auto *x : mir) if (x) gce_destroy(x); if (e) gce_destroy(e); if (fa) gce_fasta_free(fa); of.drop(); close(fd); return code; };
    const size_t PIECE = (size_t)(chunk_reads > 0 && chunk_reads < (1 << 16) ? (1 << 20) : (8 << 20));       // compressed bytes per window (tests shrink it through chunk_reads)
    // GCE_BAM_HOST_INFLATE=1: the BGZF members are inflated by the host threads (the path of the first half of round 3); default: they go to
    // HBM compressed and the GPU inflates them (gce_raw_push_bgzf) -- the host inflates only the window(s) that hold the BAM header
    const bool gpu_inflate = getenv("GCE_BAM_HOST_INFLATE") == nullptr;
    const bool tlap = getenv("GCE_RAW_TIMING") != nullptr; double tl0 = now_s();
    auto lap = [&](const char *what) { if (tlap) { const double x = now_s(); fprintf(stderr, "gce_run_bam %s %.4f s\n", what, x - tl0); tl0 = x; } };
    Pinned comp[2]; int32_t comp_ticket[2] = {-1, -1};
    if (!comp[0].ensure(PIECE + (1 << 17)) || !comp[1].ensure(PIECE + (1 << 17))) return done(GCE_ERR_OOM, "out of pinned host memory");
    std::vector<uint64_t> z_coff; std::vector<uint32_t> z_csize, z_usize;
    lap("compressed-piece buffers");
    Pinned win[3]; int32_t win_ticket[3] = {-1, -1, -1};
    // reader: piece k of the file into comp[k & 1] behind the carry-over of piece k - 1 (a BGZF block cut by the piece border)
    uint64_t file_off = 0; size_t carry = 0; double t_read = 0, t_inflate = 0, t_wait = 0;
    std::vector<Block> blocks;
    std::vector<std::string> names; std::vector<uint32_t> lens; std::string text;
    uint64_t hdr_end = 0; bool have_header = false;
    gce_params prm = *params;
    Raw<uint8_t> head;                                  // the inflated start of the stream until the header is complete (usually one window)
    auto start_read = [&](int slot, size_t keep) {
        const uint64_t at = file_off; const size_t want = (size_t)std::min<uint64_t>(PIECE, fsz - at);
        reader_on = true;
        reader = std::thread([&, slot, keep, at, want] {                                    // the piece in up to four parts, read side by side (one pread stream copies ~7 GB/s out of the page cache)
            const double r0 = now_s();
            static const size_t RP = getenv("GCE_READ_PARTS") ? (size_t)atoi(getenv("GCE_READ_PARTS")) : 4;
            const int R = (int)std::max<size_t>(1, std::min<size_t>({RP, (size_t)T, want >> 20}));
            std::vector<size_t> done_(R, 0); std::vector<std::thread> sub;
            auto part = [&](int r) { const size_t a = want * (size_t)r / R, z2 = want * (size_t)(r + 1) / R; done_[r] = pread_full(fd, comp[slot].p + keep + a, z2 - a, at + a); };
            for (int r = 1; r < R; r++) sub.emplace_back(part, r);
            part(0);
            for (auto &t : sub) t.join();
            size_t o = 0; for (int r = 0; r < R; r++) { const size_t a = want * (size_t)r / R, z2 = want * (size_t)(r + 1) / R; o += done_[r]; if (done_[r] != z2 - a) break; }      // (bytes in order up to the first short part)
            got_next = (ssize_t)o; t_read += now_s() - r0; });
        file_off += want;
    };
    int rc = GCE_OK;
    std::string emsg;
    // the contig table is known (BAM header / SAM header lines): engine, reference, raw stream.  first_qname: the first record's name or NULL
    auto setup_engine = [&](const char *first_qname, size_t capacity) -> int {
        have_header = true;
        file_params(prm, (int32_t)lens.size(), lens.data(), first_qname);
        if (getenv("GCE_RAW_TIMING")) fprintf(stderr, "gce_run_bam: RSS before gce_create %ld MB (entry %ld MB)\n", status_kb("VmRSS:") >> 10, (long)(out->rss_start_kb >> 10));
        lap("up to the header");
        int r2;
        if (devices) prm.device = devices[0];
        // One host thread per engine: gce_create, the reference, and the raw stream's buffers (gce_raw_begin: a few GB of hipMalloc per engine, 0.15 s per GB on a
        // fresh process -- the four engines of a sharded run, set up one after the other, were 0.4 - 1.7 s of "input pipeline" on some boxes) side by side; on a
        // multi-GPU node every device allocates for itself.  The FASTA file is read once, in front.
        if (fasta_path && *fasta_path && (r2 = gce_fasta_load(fasta_path, threads, &fa)) != GCE_OK) { emsg = "cannot read the FASTA file"; return r2; }
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
        e = made[0]; for (size_t r = 1; r < made.size(); r++) if (made[r]) mir.push_back(made[r]);       // (owned by `done` from here on)
        if (fa) { gce_fasta_free(fa); fa = nullptr; }                                    // (packed in HBM: the host copy goes)
        for (size_t r = 0; r < made.size(); r++) if (rcs[r] != GCE_OK) { emsg = msgs[r]; return rcs[r]; }
        lap("gce_create + reference + gce_raw_begin (a thread per engine)");
        for (gce_engine *x : mir) if ((r2 = gce_raw_attach_mirror(e, x)) != GCE_OK) { emsg = gce_last_error(x); return r2; }
        return GCE_OK;
    };
    uint64_t pushed = 0;
    // sam_open(in, "r") takes either format (src/gencore.cpp:164): a file that does not start with the gzip magic is SAM text
    const bool is_sam = fsz > 0 && !looks_gzip(fd, fsz);
    if (is_sam) {
        // Pieces of the text are cut at line feeds; the '@' lines in front give the header text and the contig table; alignment lines become BAM
        // records on all host threads (gce_samtext.hpp) in a pinned window that goes to HBM like an inflated BAM window, behind BAM header bytes
        // made from the SAM header: from there on the stream is the one a BAM file gives.
        Raw<char> tbuf[2]; uint64_t at = 0; bool in_header = true; samtext::NameMap nmap; int wk = 0, kb = 0;
        std::vector<std::vector<uint8_t>> parts; std::vector<std::string> perr;
        const size_t TP = PIECE < ((size_t)8 << 20) ? PIECE : ((size_t)64 << 20);          // text bytes per piece (tests: 1 MB pieces that cut lines)
        std::thread rd; bool rd_on = false; ssize_t rd_got = 0;
        auto read_into = [&](char *dst, size_t want, uint64_t off) { const double r0 = now_s(); rd_got = (ssize_t)pread_full(fd, dst, want, off); t_read += now_s() - r0; };
        auto bail = [&](int code, const char *m) { if (rd_on) { rd.join(); rd_on = false; } return done(code, m); };
        size_t n = 0;                                                                      // bytes in tbuf[kb]: what the last piece left over + this piece
        {
            const size_t want = (size_t)std::min<uint64_t>(TP, fsz);
            tbuf[0].resize(want + 1); if (!tbuf[0].ok()) return done(GCE_ERR_OOM, "out of host memory");
            read_into(tbuf[0].data(), want, 0);
            if ((size_t)rd_got != want) return done(GCE_ERR_INVALID, "cannot read the input SAM");
            at = want; n = want;
        }
        for (;;) {
            char *cur = tbuf[kb].data();
            const bool last = at >= fsz;
            size_t lim = n;
            if (!last) {
                const char *nl = (const char *)memrchr(cur, '\n', n);
                lim = nl ? (size_t)(nl - cur) + 1 : 0;
                if (!nl && n > ((size_t)256 << 20)) return done(GCE_ERR_INVALID, "SAM line longer than 256 MB");
            } else if (n && cur[n - 1] != '\n') { cur[n] = '\n'; lim = n + 1; }
            // the next piece is read behind what this one leaves over (the line its end cut) while this one is converted
            size_t want2 = 0, left = lim >= n ? 0 : n - lim;
            if (!last) {
                want2 = (size_t)std::min<uint64_t>(TP, fsz - at);
                Raw<char> &nx = tbuf[kb ^ 1];
                nx.resize(left + want2 + 1); if (!nx.ok()) return done(GCE_ERR_OOM, "out of host memory");
                if (left) memcpy(nx.data(), cur + lim, left);
                char *dst = nx.data() + left; const uint64_t off = at;
                rd_on = true; rd = std::thread([&, dst, off, want2] { read_into(dst, want2, off); });
                at += want2;
            }
            size_t p = 0;
            if (in_header) {
                while (p < lim && cur[p] == '@') { const char *q = (const char *)memchr(cur + p, '\n', lim - p); const size_t z2 = (size_t)(q - cur) + 1; text.append(cur + p, z2 - p); p = z2; }
                if (p < lim || last) {
                    in_header = false;
                    if (!samtext::parse_header_text(text, names, lens) || lens.empty()) return bail(GCE_ERR_INVALID, "this SAM file has no header");      // src/gencore.cpp:186-189
                    nmap.build(names);
                    std::string fq;
                    if (p < lim) { const char *q = cur + p; const char *t = (const char *)memchr(q, '\t', lim - p); if (t) fq.assign(q, t); }
                    if ((rc = setup_engine(fq.empty() ? nullptr : fq.c_str(), (size_t)std::max<uint64_t>(fsz + (1u << 20), 1u << 20))) != GCE_OK) return bail(rc, emsg.c_str());
                    const std::vector<uint8_t> hb = bam_header_bytes(text, names, lens);
                    hdr_end = hb.size();
                    int32_t tk; if ((rc = gce_raw_push(e, hb.data(), hb.size(), &tk)) != GCE_OK || (rc = gce_submit_wait(e, tk)) != GCE_OK) return bail(rc, gce_last_error(e));
                    pushed += hb.size();
                }
            }
            if (!in_header && p < lim) {
                const double i0 = now_s();
                if (const char *m = lines_to_records(cur, p, lim, T, nmap, parts, perr)) return bail(GCE_ERR_INVALID, m);
                size_t tot = 0; std::vector<size_t> po((size_t)T + 1, 0);
                for (int t = 0; t < T; t++) { po[(size_t)t] = tot; tot += parts[(size_t)t].size(); }
                if (tot) {
                    const int ws = wk % 3;
                    if (win_ticket[ws] >= 0) { const double w0 = now_s(); if ((rc = gce_submit_wait(e, win_ticket[ws])) != GCE_OK) return bail(rc, gce_last_error(e)); t_wait += now_s() - w0; win_ticket[ws] = -1; }
                    if (!win[ws].ensure(tot + 64)) return bail(GCE_ERR_OOM, "out of pinned host memory");
                    parallel_for(T, T, [&](int, int64_t a, int64_t b2) { for (int64_t t = a; t < b2; t++) if (!parts[(size_t)t].empty()) memcpy(win[ws].p + po[(size_t)t], parts[(size_t)t].data(), parts[(size_t)t].size()); });
                    if ((rc = gce_raw_push(e, win[ws].p, tot, &win_ticket[ws])) != GCE_OK) return bail(rc, gce_last_error(e));
                    pushed += tot; wk++;
                }
                t_inflate += now_s() - i0;                                                 // (lines -> records: reported where a BAM input reports its inflate)
            }
            if (last) break;
            rd.join(); rd_on = false;
            if ((size_t)rd_got != want2) return done(GCE_ERR_INVALID, "cannot read the input SAM");
            n = left + want2; kb ^= 1;
        }
    } else {
    int k = 0;
    size_t have = 0;                                    // bytes in comp[k & 1]: carry + piece
    if (fsz) { start_read(0, 0); reader.join(); reader_on = false; have = (size_t)got_next; }
    while (have > 0) {
        const int cs = k & 1, ws = k % 3;
        uint8_t *z = comp[cs].p;
        // ---- BGZF members of this piece
        blocks.clear();
        size_t off = 0; uint64_t uoff = 0;
        for (Member m;;) {
            const Scan sc = scan_member(z, have, off, m);
            if (sc == Scan::More) break;                                                // cut by the piece border: carried over
            if (sc != Scan::Member) return done(GCE_ERR_INVALID, scan_message(sc));
            blocks.push_back(Block{off, m.bsize, m.isize, uoff}); off += m.bsize; uoff += m.isize;
        }
        const bool last = file_off >= fsz;
        if (last && off != have) return done(GCE_ERR_INVALID, "truncated BGZF block at the end of the file");
        if (!last && blocks.empty()) return done(GCE_ERR_INVALID, "BGZF block larger than a window");
        // ---- the next piece is read while this one is inflated
        carry = have - off;
        if (!last) {
            if (comp_ticket[cs ^ 1] >= 0) { const double w0 = now_s(); if ((rc = gce_submit_wait(e, comp_ticket[cs ^ 1])) != GCE_OK) return done(rc, gce_last_error(e)); t_wait += now_s() - w0; comp_ticket[cs ^ 1] = -1; }   // (its members are in HBM)
            memcpy(comp[cs ^ 1].p, z + off, carry); start_read(cs ^ 1, carry);
        }
        if (have_header && gpu_inflate) {                                               // this piece's members: to HBM as they are
            z_coff.clear(); z_csize.clear(); z_usize.clear();
            for (const Block &bk : blocks) { z_coff.push_back(bk.coff); z_csize.push_back(bk.csize); z_usize.push_back(bk.usize); }
            if ((rc = gce_raw_push_bgzf(e, z, off, (int32_t)blocks.size(), z_coff.data(), z_csize.data(), z_usize.data(), &comp_ticket[cs])) != GCE_OK) return done(rc, gce_last_error(e));
            pushed += uoff;
            if (reader_on) { reader.join(); reader_on = false; have = carry + (size_t)got_next; } else have = 0;
            k++;
            continue;
        }
        if (win_ticket[ws] >= 0) { const double w0 = now_s(); if ((rc = gce_submit_wait(e, win_ticket[ws])) != GCE_OK) return done(rc, gce_last_error(e)); t_wait += now_s() - w0; win_ticket[ws] = -1; }
        if (!win[ws].ensure((size_t)uoff + 64)) return done(GCE_ERR_OOM, "out of pinned host memory");
        const double i0 = now_s();
        std::atomic<int> bad{0};
        parallel_for(T, (int64_t)blocks.size(), [&](int, int64_t a, int64_t b2) { for (int64_t q = a; q < b2; q++) if (blocks[q].usize && !inflate_block(z + blocks[q].coff, blocks[q], win[ws].p + blocks[q].uoff)) bad = 1; });
        t_inflate += now_s() - i0;
        if (bad) return done(GCE_ERR_INVALID, "inflate / CRC failure");
        // ---- header (first window(s)), engine, reference
        if (!have_header) {
            const size_t old = head.size();
            Raw<uint8_t> h2; h2.resize(old + (size_t)uoff + 1); if (!h2.ok()) return done(GCE_ERR_OOM, "out of host memory");
            if (old) memcpy(h2.data(), head.data(), old);
            memcpy(h2.data() + old, win[ws].p, (size_t)uoff); h2.n = old + (size_t)uoff; head = std::move(h2);
            const uint8_t *u = head.data(); const uint64_t n = head.size();
            BamHeader bh;
            const Hdr hs = n >= 12 ? parse_bam_header(u, n, Contigs::Collect, bh, &names, &lens) : Hdr::Incomplete;      // (this runner looks at the magic only once 12 bytes are there)
            if (hs == Hdr::NotBam) return done(GCE_ERR_INVALID, "not a BAM stream");
            const bool complete = hs == Hdr::Complete;
            if (complete && lens.empty()) return done(GCE_ERR_INVALID, "this SAM file has no header");      // src/gencore.cpp:186-189 (n_targets == 0), as the SAM-text branch does
            if (complete) { hdr_end = bh.hdr_end; text.assign((const char *)u + bh.text_off, bh.l_text); }
            if (!complete && last) return done(GCE_ERR_INVALID, "truncated header");
            if (complete) {
                const char *fq = nullptr;                                                 // src/gencore.cpp:207-220: the first record's name
                if (hdr_end + 36 < n) { const uint32_t lq = u[hdr_end + 12]; if (hdr_end + 36 + lq <= n) fq = (const char *)u + hdr_end + 36; }
                if ((rc = setup_engine(fq, (size_t)std::max<uint64_t>(fsz * 5, head.size()))) != GCE_OK) return done(rc, emsg.c_str());
                // what was inflated so far goes up in one piece (normally: this very window)
                if (old) { int32_t tk; if ((rc = gce_raw_push(e, head.data(), old, &tk)) != GCE_OK || (rc = gce_submit_wait(e, tk)) != GCE_OK) return done(rc, gce_last_error(e)); pushed += old; }
                head.release();
                lap("gce_raw_begin + first push");
            }
        }
        if (have_header && uoff) {
            if ((rc = gce_raw_push(e, win[ws].p, (size_t)uoff, &win_ticket[ws])) != GCE_OK) return done(rc, gce_last_error(e));
            pushed += uoff;
        }
        if (reader_on) { reader.join(); reader_on = false; have = carry + (size_t)got_next; } else have = 0;
        k++;
    }
    }   // (BAM input)
    if (!have_header) return done(GCE_ERR_INVALID, fsz ? "truncated header" : "empty file");
    lap("rest of the input loop");
    out->read_s = t_read; out->inflate_s = t_inflate; out->submit_s = t_wait;
    out->open_s = now_s() - t_start;
    if (getenv("GCE_RAW_TIMING")) fprintf(stderr, "gce_run_bam: RSS after the input pipeline %ld MB\n", status_kb("VmRSS:") >> 10);
    double t0 = now_s();
    int64_t n_rec = 0;
    uint64_t body = 0; int64_t n_out = 0;
    // ---- the depth statistics of the report (Options::coverageStep, Options::bedFile; stats.cpp:56-83, bed.cpp:64-79): every engine adds up its own reads and
    //      records on its GPU right behind its run -- BEFORE the merge adds the other engines' Stats blocks into the first one's -- (gce_stats_payload_device)
    if (depth) {
        memset(depth, 0, sizeof *depth);
        if (coverage_step <= 0) return done(GCE_ERR_INVALID, "coverage_step must be positive");
        if (bed_path && *bed_path) {
            std::vector<const char *> np; for (auto &x : names) np.push_back(x.c_str());
            if ((rc = gce_bed_load(bed_path, (int32_t)np.size(), np.data(), &depth->n_regions, &depth->region_tid, &depth->region_start, &depth->region_end, nullptr)) != GCE_OK) return done(rc, "cannot read the BED file");
        }
        if (!depth_alloc(depth, lens, coverage_step)) return done(GCE_ERR_OOM, "out of host memory");
    }
    auto engine_payload = [&](gce_engine *x) -> int {
        if (!depth) return GCE_OK;
        const int64_t *pay = nullptr; gce_payload_layout lay;
        return gce_stats_payload_device(x, coverage_step, depth->n_regions, depth->region_tid, depth->region_start, depth->region_end, &pay, &lay);
    };
    if (n_shards > 1) {
        // ---- several engines: each indexes the stream it received, keeps its shard, runs it and assembles its records -- side by side, one host
        //      thread per engine, nothing exchanged; then the streams are merged on the first engine's device
        std::vector<gce_engine *> all; all.push_back(e); for (auto *x : mir) all.push_back(x);
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
        for (int32_t r = 0; r < n_shards; r++) if (rcs[(size_t)r] != GCE_OK) return done(rcs[(size_t)r], msgs[(size_t)r].c_str());
        for (int32_t r = 0; r < n_shards; r++) { out->kernel_ms = std::max(out->kernel_ms, kms[(size_t)r]); out->index_s = std::max(out->index_s, t_idx[(size_t)r]); }
        out->process_s = now_s() - t0 - out->index_s; t0 = now_s();
        n_rec = nrec[0];
        if (n_rec > 0) {
            if ((rc = gce_raw_merge_outputs(all.data(), n_shards, &body, &n_out, &out->pre, &out->post, &out->n_reads)) != GCE_OK) return done(rc, gce_last_error(e));
            out->n_out = n_out;
        }
        out->drain_s = now_s() - t0; t0 = now_s();
    } else {
    if ((rc = gce_raw_finish(e, hdr_end, prm.n_targets, &n_rec)) != GCE_OK) return done(rc, gce_last_error(e));
    out->index_s = now_s() - t0; t0 = now_s();
    if (n_rec > 0) {
        if ((rc = gce_process(e)) != GCE_OK) return done(rc, gce_last_error(e)[0] ? gce_last_error(e) : gce_status_message(rc));
        out->process_s = now_s() - t0; t0 = now_s();
        gce_timing tm; if (gce_get_timing(e, &tm) == GCE_OK) out->kernel_ms = tm.total_ms;
        gce_result res;
        if ((rc = gce_result_device(e, &res)) != GCE_OK) return done(rc, gce_last_error(e));
        out->n_reads = res.n_reads; out->n_out = res.n_out; out->pre = res.pre; out->post = res.post;
        if ((rc = gce_raw_build_output(e, &body, &n_out)) != GCE_OK) return done(rc, gce_last_error(e));
        if ((rc = engine_payload(e)) != GCE_OK) return done(rc, gce_last_error(e));
        out->drain_s = now_s() - t0; t0 = now_s();
        if (getenv("GCE_RAW_TIMING")) fprintf(stderr, "gce_run_bam: RSS after process + output records %ld MB\n", status_kb("VmRSS:") >> 10);
    }
    }   // (one engine)
    // ---- the depth statistics of the report: the engines' payloads (computed above, each on its own Stats blocks) summed in device memory, to the host once
    if (depth && n_rec > 0) {
        std::vector<gce_engine *> all; all.push_back(e); for (auto *x : mir) all.push_back(x);
        const int64_t *pay = nullptr; gce_payload_layout lay;
        if ((rc = gce_stats_payload_sum(all.data(), (int32_t)all.size(), &pay, &lay)) != GCE_OK) return done(rc, gce_last_error(e));
        std::vector<int64_t> host((size_t)lay.total_words);
        if ((rc = gce_stats_payload_read(e, pay, lay.total_words, host.data())) != GCE_OK) return done(rc, gce_last_error(e));
        if (lay.n_bins != depth->n_bins || lay.n_regions != depth->n_regions) return done(GCE_ERR_INVALID, "payload layout");
        depth_unpack(depth, host.data(), lay.stats_words);
    }
    // ---- the output file: its header, then a stream in HBM walked in pieces (pump_pieces), each piece handed to what writes it.  A name that ends
    //      in "sam" is written as SAM text (src/gencore.cpp:170-173: sam_open(out, "w")), any other as BGZF members.  Levels -2 / -3: the stream is what
    //      the GPU made of the records -- the lines (gce_samfmt.hpp) or the deflated file image (gce_deflate.hpp: -2 fixed Huffman codes, -3 the smallest
    //      of dynamic codes, fixed codes and stored per block) -- and the host only copies it out and writes it.  Other levels: the stream is the records,
    //      made into lines or, behind the header's bytes, deflated into members of 0xff00 bytes by all host threads.
    const bool gpu_out = level == -2 || level == -3;
    if (!of.open(out_path, OutFile::named_sam(out_path))) return done(GCE_ERR_INVALID, of.sam ? "cannot open the output SAM" : "cannot open the output BAM");
    const char *const cannot = of.sam ? "cannot write the output SAM" : "cannot write the output BAM";
    const char *why = "output piece";                                                      // what a walk that ends early says: a fetch's words, unless wait or sink put theirs
    Pinned obuf[2];
    const uint64_t SMALL = PIECE < ((size_t)8 << 20) ? ((uint64_t)64 << 10) : ((uint64_t)16 << 20);   // pieces of text and of records for lines (tests: small ones that cut records)
    auto records = [&](uint64_t o, uint8_t *dst, size_t n, int32_t *tk) { return gce_raw_read_output_async(e, o, dst, n, tk); };
    auto wait = [&](int32_t tk) { const int r = gce_submit_wait(e, tk); if (r != GCE_OK) why = gce_last_error(e); return r; };
    auto written = [&](bool ok) -> int { if (ok) return GCE_OK; why = cannot; return GCE_ERR_INVALID; };
    auto write = [&](const uint8_t *p, size_t n) { return written(of.write(p, n)); };
    if (of.sam) {
        if (!of.sam_header(text, names, lens)) return done(GCE_ERR_INVALID, cannot);
        if (gpu_out) {
            uint64_t tb = 0;
            std::vector<const char *> np; for (auto &x : names) np.push_back(x.c_str());
            if (body && (rc = gce_raw_format_output(e, (int32_t)np.size(), np.data(), &tb)) != GCE_OK) return done(rc, gce_last_error(e)[0] ? gce_last_error(e) : gce_status_message(rc));
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
        if (!of.reserve()) return done(GCE_ERR_OOM, "out of host memory");
        if (gpu_out) {
            uint64_t cb = 0;
            if (!of.header_members(hdr, level, true, T)) return done(GCE_ERR_INVALID, cannot);
            if (body && (rc = gce_raw_deflate_output_codes(e, level == -3 ? 1 : 0, &cb)) != GCE_OK) return done(rc, gce_last_error(e));
            rc = pump_pieces(nullptr, 0, cb, (uint64_t)16 << 20, obuf, [&](uint64_t o, uint8_t *dst, size_t n, int32_t *tk) { return gce_raw_read_deflated_async(e, o, dst, n, tk); }, wait, write);
        } else rc = pump_pieces(hdr.data(), hdr.size(), body, ROUND_BYTES, obuf, records, wait, [&](const uint8_t *p, size_t n) { return written(of.members(p, n, level, T)); });
    }
    if (rc != GCE_OK) return done(rc, why);
    if (!of.close()) return done(GCE_ERR_INVALID, cannot);
    out->write_s = now_s() - t0;
    out->total_s = now_s() - t_start;
    out->peak_rss_kb = status_kb("VmHWM:"); out->rss_end_kb = status_kb("VmRSS:");
    (void)pushed;
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


// ---- one file in key-range passes on one device (gce_passes.hpp)
struct gce_passes;
int gce_passes_create(int32_t device, int32_t max_contig, int32_t flush_period, gce_passes **out);
void gce_passes_destroy(gce_passes *p);
const char *gce_passes_error(gce_passes *p);
int gce_device_mem_info(int32_t device, size_t *free_bytes, size_t *total_bytes);
int gce_passes_window(gce_passes *p, gce_engine *e, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize,
                      uint64_t skip, int32_t n_ref, int32_t last, int32_t *cut_reached);
int gce_passes_plan(gce_passes *p, int32_t min_passes, uint64_t budget, uint64_t reserve, int32_t *P_out, uint64_t *total_w, uint64_t *per_pass, uint64_t *fixed_out);
int gce_passes_info(gce_passes *p, int32_t k, uint64_t *weight, const uint64_t **cuts, int32_t *n_events, const int32_t **ev_tid, const int32_t **ev_pos);
int gce_passes_begin(gce_passes *p, gce_engine *e, int32_t k);
int gce_passes_end(gce_passes *p, gce_engine *e, uint64_t records_begin, int32_t n_ref, int64_t *n_records, int32_t *watermark_tid, int32_t *watermark_pos);
int gce_passes_output(gce_passes *p, gce_engine *e, void *keys_host, void *body_host);
int gce_passes_release(gce_passes *p, gce_engine *e);
}  // extern "C" (declarations)
extern "C++" {
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
// what the merge compares per output record (the 32-byte MergeKey of gce_raw_merge_outputs)
struct PassKey { int32_t tid, pos, mtid, mpos, isize; uint32_t gidx, size, pad; };
static_assert(sizeof(PassKey) == 32, "PassKey mirrors MergeKey");
inline bool pass_less(const PassKey &a, const PassKey &b) {
    if (a.tid != b.tid) return a.tid < b.tid;
    if (a.pos != b.pos) return a.pos < b.pos;
    if (a.mtid != b.mtid) return a.mtid < b.mtid;
    if (a.mpos != b.mpos) return a.mpos < b.mpos;
    if (a.isize != b.isize) return a.isize < b.isize;
    return a.gidx < b.gidx;
}
// the output of the pass runner (and, for its members and its close, of the sort runners): the record stream arrives in pieces of whole
// records, in order; it is written a round of members at a time -- by the host threads, or at levels -2 and -3 by the GPU encoder as
// gce_raw_deflate_output_codes -- or, to a SAM file, piece by piece as lines (by gce_sam_format at levels -2 and -3)
struct PassWriter {
    OutFile out; int level = -1, T = 1; int32_t device = 0; const std::vector<std::string> *names = nullptr;
    std::vector<uint8_t> buf, gz; std::vector<uint64_t> ro; std::vector<std::string> lines;
    static constexpr uint64_t BS = MEMBER_BYTES, CH = ROUND_BYTES;
    bool gpu() const { return level == -2 || level == -3; }
    bool flush(size_t n) {                               // the first n bytes of buf
        if (!n) return true;
        if (out.sam && gpu()) {                          // the lines by the GPU (gce_samfmt.hpp), as the BAM levels below take the GPU's deflate
            std::vector<const char *> np; for (auto &x : *names) np.push_back(x.c_str());
            size_t tb = 0; int64_t nr = 0, nh = 0, bad = -1;
            int rc = gce_sam_format(device, buf.data(), n, (int32_t)np.size(), np.data(), gz.data(), gz.size(), &tb, &nr, &nh, &bad, nullptr);
            if (rc == GCE_ERR_OOM && tb > gz.size()) { gz.resize(tb); rc = gce_sam_format(device, buf.data(), n, (int32_t)np.size(), np.data(), gz.data(), gz.size(), &tb, &nr, &nh, &bad, nullptr); }
            if (rc != GCE_OK || !out.write(gz.data(), tb)) return false;
        } else if (out.sam) {
            if (whole_records(buf.data(), n, ro) != n || !records_to_lines(buf.data(), ro, *names, T, lines)) return false;
            for (const std::string &L : lines) if (!out.write(L.data(), L.size())) return false;
        } else if (gpu()) {
            size_t zb = 0;
            if (gz.size() < n + n / 8 + 64 * (n / BS + 1) + 64) gz.resize(n + n / 8 + 64 * (n / BS + 1) + 64);
            if (gce_bgzf_deflate_codes(device, buf.data(), n, (uint32_t)BS, level == -3 ? 1 : 0, gz.data(), gz.size(), &zb) != GCE_OK || !out.write(gz.data(), zb)) return false;
        } else if (!out.members(buf.data(), n, level, T)) return false;
        buf.erase(buf.begin(), buf.begin() + (ptrdiff_t)n);
        return true;
    }
    // the header: a SAM file's text; at levels -2 / -3 members of its own; at host levels it goes in front of the records, into their members
    bool open(const char *path, const std::string &text, const std::vector<std::string> &nm, const std::vector<uint32_t> &lens, const std::vector<uint8_t> &hdr) {
        names = &nm;
        if (!out.open(path, OutFile::named_sam(path))) return false;
        if (out.sam) return out.sam_header(text, nm, lens);
        if (!out.reserve()) return false;
        if (gpu()) return out.header_members(hdr, level, true, T);
        buf.assign(hdr.begin(), hdr.end());
        return true;
    }
    bool records(const uint8_t *p, size_t n) {           // whole records
        buf.insert(buf.end(), p, p + n);
        if (out.sam) return flush(buf.size());
        while (buf.size() >= CH) if (!flush((size_t)CH)) return false;
        return true;
    }
    bool close() { const bool good = flush(buf.size()); return out.close() && good; }
};
}  // namespace
}  // extern "C++"
extern "C" {

int gce_run_bam_passes(const char *in_path, const char *out_path, const char *fasta_path, const char *bed_path, int32_t coverage_step, const gce_params *params,
                       int32_t device, int threads, int level, size_t device_budget_bytes, int32_t min_passes, size_t window_bytes,
                       gce_bam_run *out, gce_depth_run *depth, gce_pass_run *run, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !params || !out || !depth || !run || min_passes < 0 || min_passes > 64 || coverage_step <= 0) return GCE_ERR_INVALID;
    memset(out, 0, sizeof *out); memset(run, 0, sizeof *run); memset(depth, 0, sizeof *depth);
    const double t_start = now_s();
    out->rss_start_kb = status_kb("VmRSS:");
    (void)gce_device_bytes(nullptr, nullptr, 1);
    auto peak_now = [&] { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); return pk; };
    const bool auto_budget = device_budget_bytes == 0;
    uint64_t budget = device_budget_bytes;
    if (auto_budget) {
        size_t fr = 0, tot = 0;
        const int r0 = gce_device_mem_info(device, &fr, &tot);
        if (r0 != GCE_OK) { set_err(err, "no device"); return r0; }
        budget = (uint64_t)((double)fr * GCE_PASS_BUDGET_FRACTION);
    }
    run->budget_bytes = (int64_t)budget;
    struct stat st;
    const int fd = open(in_path, O_RDONLY);
    if (fd < 0) { set_err(err, "cannot open the input BAM"); return GCE_ERR_INVALID; }
    if (fstat(fd, &st) != 0 || st.st_size < 0) { close(fd); set_err(err, "cannot stat the input BAM"); return GCE_ERR_INVALID; }
    const uint64_t fsz = (uint64_t)st.st_size;
    const bool is_sam = fsz > 0 && !looks_gzip(fd, fsz);
    // today's single-pass path (gce_run_bam_depth), unchanged, whenever the auto budget is in force and no passes are forced: at once when even a
    // generous bound fits (measured, DESIGN.md 4b: peak ~6.2 x inflated bytes, inflated ~4.3 - 4.7 x the file; the bound takes 6.5 x 6), otherwise
    // after the key pass when the plan needs one pass.  SAM text is never processed in passes; with the auto budget it always runs as today.
    const bool single_ok = auto_budget && min_passes <= 1;
    const uint64_t est = fsz * 39 + ((uint64_t)2 << 30);
    auto single = [&]() -> int {
        gce_params pr1 = *params; pr1.device = device;
        const int r1 = gce_run_bam_depth(in_path, out_path, fasta_path, bed_path, coverage_step, &pr1, 1, &device, 0, threads, level, out, depth, err);
        run->n_passes = 1; run->single_pass = 1; run->reads_per_pass[0] = out->n_reads; run->peak_device_bytes = peak_now(); run->pass_s[0] = out->total_s;
        return r1;
    };
    if (is_sam) {
        close(fd);
        if (min_passes > 1) { set_err(err, "SAM text input is not processed in passes"); return GCE_ERR_INVALID; }
        if (!auto_budget && est > budget) {
            char m[256]; snprintf(m, sizeof m, "SAM text input of %llu bytes needs an estimated %llu device bytes, the budget is %llu: SAM input is not processed in passes (convert it to BAM)",
                                  (unsigned long long)fsz, (unsigned long long)est, (unsigned long long)budget);
            set_err(err, m); return GCE_ERR_OOM;
        }
        return single();
    }
    if (single_ok && est <= budget) { close(fd); return single(); }
    const int T = threads > 0 ? threads : default_threads();
    gce_engine *e = nullptr; gce_fasta *fa = nullptr; gce_passes *p = nullptr;
    auto done = [&](int code, const char *m) { set_err(err, m); if (p) gce_passes_destroy(p); if (e) gce_destroy(e); if (fa) gce_fasta_free(fa); close(fd); if (code != GCE_OK) gce_depth_run_free(depth); return code; };
    // 64 MB of compressed bytes per window by default: the GPU inflate runs one lane per BGZF member and wants thousands of members per launch
    // (8 MB windows, ~400 members each, made a cfg3 4 M pass 2.6 s instead of ~1 s)
    PassReader rd; rd.fd = fd; rd.fsz = fsz; rd.T = T; rd.piece = window_bytes > 0 ? window_bytes : ((size_t)64 << 20);
    // ---- the header (the first window(s))
    std::vector<std::string> names; std::vector<uint32_t> lens; std::string text; uint64_t hdr_end = 0;
    for (;;) {
        const int g = rd.inflate_next();
        if (g < 0) return done(GCE_ERR_INVALID, rd.msg.c_str());
        BamHeader bh;
        const Hdr hs = parse_bam_header(rd.win.p, rd.n, Contigs::Collect, bh, &names, &lens);
        if (hs == Hdr::NotBam) return done(GCE_ERR_INVALID, "not a BAM stream");
        if (hs == Hdr::Complete && lens.empty()) return done(GCE_ERR_INVALID, "this SAM file has no header");
        if (hs == Hdr::Complete) { hdr_end = bh.hdr_end; text.assign((const char *)rd.win.p + bh.text_off, bh.l_text); break; }
        if (g == 0) return done(GCE_ERR_INVALID, fsz ? "truncated header" : "empty file");
    }
    const std::vector<uint8_t> hdr_raw(rd.win.p, rd.win.p + hdr_end);
    // ---- engine and reference (src/gencore.cpp:207-220: "auto" UMI prefix from the first record's name)
    gce_params prm = *params; prm.device = device;
    auto name_there = [&] { return rd.n >= hdr_end + 36 && rd.n >= hdr_end + 36 + rd.win.p[hdr_end + 12]; };
    if (umi_auto(prm)) while (!name_there()) { const int g = rd.inflate_next(); if (g < 0) return done(GCE_ERR_INVALID, rd.msg.c_str()); if (g == 0) break; }
    file_params(prm, (int32_t)lens.size(), lens.data(), name_there() ? (const char *)rd.win.p + hdr_end + 36 : nullptr);
    int rc;
    if ((rc = gce_create(&prm, &e)) != GCE_OK) return done(rc, gce_status_message(rc));
    if (fasta_path && *fasta_path) {
        if ((rc = gce_fasta_load(fasta_path, threads, &fa)) != GCE_OK) return done(rc, "cannot read the FASTA file");
        if ((rc = set_reference(e, fa, names.data(), lens.size())) != GCE_OK) return done(rc, gce_last_error(e));
        gce_fasta_free(fa); fa = nullptr;
    }
    if ((rc = gce_passes_create(device, prm.max_contig, prm.flush_period, &p)) != GCE_OK) return done(rc, "pass state");
    // ---- depth statistics (as gce_run_bam_depth)
    if (bed_path && *bed_path) {
        std::vector<const char *> np; for (auto &x : names) np.push_back(x.c_str());
        if ((rc = gce_bed_load(bed_path, (int32_t)np.size(), np.data(), &depth->n_regions, &depth->region_tid, &depth->region_start, &depth->region_end, nullptr)) != GCE_OK) return done(rc, "cannot read the BED file");
    }
    if (!depth_alloc(depth, lens, coverage_step)) return done(GCE_ERR_OOM, "out of host memory");
    // the file from its first byte, piece by piece: its BGZF members go to the GPU (gce_passes_window inflates and indexes them there; the
    // header's bytes are passed over); e == NULL: the key pass
    auto stream = [&](gce_engine *x) -> int {
        rd.reset();
        uint64_t skip = hdr_end;
        for (;;) {
            const int g = rd.members_next();
            if (g < 0) { set_err(err, rd.msg.c_str()); return GCE_ERR_INVALID; }
            if (g == 0) return GCE_OK;
            const uint64_t sk = std::min<uint64_t>(skip, rd.member_arrays());
            int32_t cut = 0;
            const int r2 = gce_passes_window(p, x, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, prm.n_targets,
                                             rd.last_piece() ? 1 : 0, &cut);
            if (r2 != GCE_OK) { set_err(err, gce_passes_error(p)); return r2; }
            skip -= sk;
            if (cut || rd.last_piece()) return GCE_OK;
        }
    };
    out->open_s = now_s() - t_start;
    // ---- key pass
    double t0 = now_s();
    rc = stream(nullptr);
    std::string kmsg;                                                                // (the key pass failed: why)
    if (rc != GCE_OK) {
        kmsg = err ? err : "";
        if (rc == GCE_ERR_OOM) { char mm[200]; snprintf(mm, sizeof mm, "the key pass needs more device memory than the budget of %llu bytes", (unsigned long long)budget); kmsg = mm; }
    } else if ((uint64_t)peak_now() > budget) {
        char m[200]; snprintf(m, sizeof m, "the key pass needs %lld device bytes, the budget is %llu", (long long)peak_now(), (unsigned long long)budget); kmsg = m; rc = GCE_ERR_OOM;
    }
    int32_t P = 1; uint64_t total_w = 0, room = 0, fixed = 0;
    // beside the weights: the engine's working set that does not scale with a pass's reads (measured: a pass of 43 MB of weight on cfg3 peaked
    // 82 MB above the fixed part), hipCUB temporaries, the GPU encoder's 16 MB pieces
    const uint64_t reserve = ((uint64_t)96 << 20) + (level == -2 || level == -3 ? ((uint64_t)64 << 20) : 0);
    if (rc == GCE_OK && (rc = gce_passes_plan(p, std::max(min_passes, 1), budget, reserve, &P, &total_w, &room, &fixed)) != GCE_OK) kmsg = gce_passes_error(p);
    if (rc != GCE_OK && single_ok) {                                                 // nothing written yet: the file goes the way it goes today
        gce_passes_destroy(p); p = nullptr; gce_destroy(e); e = nullptr; close(fd);
        gce_depth_run_free(depth);
        return single();
    }
    if (rc != GCE_OK) return done(rc, kmsg.c_str());
    run->n_passes = P; run->key_pass_s = now_s() - t0; run->fixed_bytes = (int64_t)fixed; run->pass_room = (int64_t)room; run->total_weight = (int64_t)total_w;
    if (single_ok && P == 1) {                                                       // the plan fits one pass: today's path (the key pass only measured)
        const double kp = run->key_pass_s;
        gce_passes_destroy(p); p = nullptr; gce_destroy(e); e = nullptr; close(fd);
        gce_depth_run_free(depth);
        const int r1 = single();
        run->key_pass_s = kp; run->fixed_bytes = (int64_t)fixed; run->pass_room = (int64_t)room; run->total_weight = (int64_t)total_w;
        return r1;
    }
    // ---- the passes
    PassWriter wr; wr.level = level; wr.T = T; wr.device = device;
    if (!wr.open(out_path, text, names, lens, bam_header_bytes(text, names, lens))) return done(GCE_ERR_INVALID, "cannot open the output file");
    std::vector<PassKey> hk, pk, nk; std::vector<uint8_t> hb, pb, nb2, emit;
    std::vector<int64_t> pay_sum;
    int64_t *acc_pre = (int64_t *)&out->pre, *acc_post = (int64_t *)&out->post;
    for (int32_t k = 0; k < P; k++) {
        const double tp = now_s();
        uint64_t wk = 0;                                                             // the pass's weight: A x its record bytes + B per read -> room for its records
        if ((rc = gce_passes_info(p, k, &wk, nullptr, nullptr, nullptr, nullptr)) != GCE_OK) return done(rc, "pass weight");
        if ((rc = gce_raw_begin(e, (size_t)(wk / GCE_PASS_WEIGHT_A) + hdr_raw.size())) != GCE_OK) return done(rc, gce_last_error(e));
        int32_t tk;
        if ((rc = gce_raw_push(e, hdr_raw.data(), hdr_raw.size(), &tk)) != GCE_OK || (rc = gce_submit_wait(e, tk)) != GCE_OK) return done(rc, gce_last_error(e));
        if ((rc = gce_passes_begin(p, e, k)) != GCE_OK) return done(rc, gce_passes_error(p));
        rc = stream(e);
        if (rc != GCE_OK) { const std::string m = err ? err : ""; return done(rc, m.c_str()); }
        int64_t n_rec = 0; int32_t wt = INT32_MAX, wp = INT32_MAX;
        if ((rc = gce_passes_end(p, e, hdr_end, prm.n_targets, &n_rec, &wt, &wp)) != GCE_OK) return done(rc, gce_passes_error(p));
        run->reads_per_pass[k] = n_rec;
        pk.clear(); pb.clear();
        if (n_rec > 0) {
            gce_result res; uint64_t body = 0; int64_t n_out = 0;
            if ((rc = gce_process(e)) != GCE_OK) return done(rc, gce_last_error(e)[0] ? gce_last_error(e) : gce_status_message(rc));
            gce_timing tm; if (gce_get_timing(e, &tm) == GCE_OK) out->kernel_ms += tm.total_ms;
            if ((rc = gce_result_device(e, &res)) != GCE_OK) return done(rc, gce_last_error(e));
            out->n_reads += res.n_reads; out->n_out += res.n_out;
            for (int w = 0; w < GCE_STATS_WORDS; w++) { acc_pre[w] += ((const int64_t *)&res.pre)[w]; acc_post[w] += ((const int64_t *)&res.post)[w]; }
            if ((rc = gce_raw_build_output(e, &body, &n_out)) != GCE_OK) return done(rc, gce_last_error(e));
            const int64_t *pay = nullptr; gce_payload_layout lay;
            if ((rc = gce_stats_payload_device(e, coverage_step, depth->n_regions, depth->region_tid, depth->region_start, depth->region_end, &pay, &lay)) != GCE_OK) return done(rc, gce_last_error(e));
            std::vector<int64_t> host((size_t)lay.total_words);
            if ((rc = gce_stats_payload_read(e, pay, lay.total_words, host.data())) != GCE_OK) return done(rc, gce_last_error(e));
            if (pay_sum.empty()) pay_sum.assign(host.size(), 0);
            if (pay_sum.size() != host.size()) return done(GCE_ERR_INVALID, "payload layout");
            for (size_t w = 0; w < host.size(); w++) pay_sum[w] += host[w];
            pk.resize((size_t)n_out); pb.resize((size_t)body);
            if ((rc = gce_passes_output(p, e, pk.data(), pb.data())) != GCE_OK) return done(rc, gce_passes_error(p));
        }
        if ((rc = gce_passes_release(p, e)) != GCE_OK) return done(rc, "release");
        // ---- merge: the held records and this pass's (both in bamComp order); below the watermark they are final
        const bool last = k == P - 1;
        auto below = [&](const PassKey &x) { return last || x.tid < wt || (x.tid == wt && x.pos < wp); };
        nk.clear(); nb2.clear(); emit.clear();
        size_t a = 0, b = 0, ao = 0, bo = 0;
        while (a < hk.size() || b < pk.size()) {
            const bool take_a = b >= pk.size() || (a < hk.size() && pass_less(hk[a], pk[b]));
            const PassKey &x = take_a ? hk[a] : pk[b];
            const uint8_t *src = take_a ? hb.data() + ao : pb.data() + bo;
            if (below(x)) emit.insert(emit.end(), src, src + x.size); else { nk.push_back(x); nb2.insert(nb2.end(), src, src + x.size); }
            if (take_a) { ao += x.size; a++; } else { bo += x.size; b++; }
        }
        if (ao != hb.size() || bo != pb.size()) return done(GCE_ERR_INVALID, "merge: record sizes do not add up");
        if (!emit.empty() && !wr.records(emit.data(), emit.size())) return done(GCE_ERR_INVALID, "cannot write the output file");
        hk.swap(nk); hb.swap(nb2);
        run->held_max = std::max<int64_t>(run->held_max, (int64_t)hk.size());
        run->pass_s[k] = now_s() - tp;
    }
    if (!wr.close()) return done(GCE_ERR_INVALID, "cannot write the output file");
    if (!pay_sum.empty()) depth_unpack(depth, pay_sum.data(), 2 * GCE_STATS_WORDS);
    run->peak_device_bytes = peak_now();
    out->total_s = now_s() - t_start;
    out->peak_rss_kb = status_kb("VmHWM:"); out->rss_end_kb = status_kb("VmRSS:");
    return done(GCE_OK, "");
}

}  // extern "C"


// ---- the BAI index of a coordinate-sorted BAM (gce_bai.hpp)
extern "C" {
struct gce_bai;
int gce_bai_create(int32_t device, gce_bai **out);
void gce_bai_destroy(gce_bai *b);
const char *gce_bai_error(gce_bai *b);
int gce_bai_window(gce_bai *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t file_base,
                   uint64_t skip, int32_t n_ref, int32_t last);
int gce_bai_finish(gce_bai *b, int32_t n_ref, uint64_t eod, int64_t counts[5], int64_t *bad_rec, int32_t *bad_kind);
int gce_bai_serialise(gce_bai *b, int32_t n_ref, uint8_t **out, size_t *out_bytes);

int gce_bam_index(const char *bam_path, const char *bai_path, int32_t device, int threads, uint64_t window_bytes, gce_bai_run *out, char err[256]) {
    set_err(err, "");
    if (!bam_path || !bai_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    const double t_start = now_s();
    const int fd = open(bam_path, O_RDONLY);
    if (fd < 0) { set_err(err, "cannot open the BAM file"); return GCE_ERR_INVALID; }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 0) { close(fd); set_err(err, "cannot stat the BAM file"); return GCE_ERR_INVALID; }
    const uint64_t fsz = (uint64_t)st.st_size;
    const std::string tmp = std::string(bai_path) + ".tmp" + std::to_string((long long)getpid());
    gce_bai *b = nullptr; FILE *fo = nullptr;
    auto done = [&](int code, const char *m) {
        set_err(err, m);
        if (b) gce_bai_destroy(b);
        if (fo) { fclose(fo); fo = nullptr; }
        if (code != GCE_OK) unlink(tmp.c_str());
        close(fd);
        return code;
    };
    if (!starts_bgzf(fd, fsz)) return done(GCE_ERR_INVALID, "not a BGZF file");
    const int T = threads > 0 ? threads : default_threads();
    // ---- the header: the host inflates the first members (1 MB pieces) until it is whole
    uint64_t hdr_end = 0; int32_t n_ref = 0;
    {
        PassReader rh; rh.fd = fd; rh.fsz = fsz; rh.T = T; rh.piece = window_bytes > 0 ? (size_t)std::min<uint64_t>(window_bytes, (uint64_t)1 << 20) : ((size_t)1 << 20);
        for (;;) {
            const int g = rh.inflate_next();
            if (g < 0) return done(GCE_ERR_INVALID, rh.msg.c_str());
            BamHeader bh;
            const Hdr hs = parse_bam_header(rh.win.p, rh.n, Contigs::Skip, bh);
            if (hs == Hdr::NotBam) return done(GCE_ERR_INVALID, "not a BAM stream");
            if (hs == Hdr::Complete) { hdr_end = bh.hdr_end; n_ref = (int32_t)bh.n_ref; break; }
            if (g == 0) return done(GCE_ERR_INVALID, "truncated BAM header");
        }
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


// ---- an unsorted BAM into coordinate order (gce_sort.hpp)
extern "C" {
struct gce_sort;
int gce_sort_create(int32_t device, size_t device_budget_bytes, gce_sort **out);
void gce_sort_destroy(gce_sort *b);
const char *gce_sort_error(gce_sort *b);
int gce_sort_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                    int32_t n_ref, int32_t last, uint64_t est_bytes);
int gce_sort_finish(gce_sort *b, int32_t n_ref, int32_t codes, uint64_t piece_bytes, int64_t counts[3], int64_t *bad_rec, uint64_t *out_bytes, double times[2]);
int gce_sort_read(gce_sort *b, uint64_t offset, size_t bytes, int32_t codes, void *host, size_t host_cap, size_t *got);
int gce_sort_key_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, uint64_t est_bytes);
int gce_sort_plan(gce_sort *b, int32_t n_ref, int32_t codes, uint64_t piece_bytes, int32_t min_passes, int64_t counts[3], int64_t *bad_rec, uint64_t *total_out, int32_t *n_passes,
                  uint64_t *pass_bytes, uint64_t *resident, double *plan_s);
int gce_sort_pass_begin(gce_sort *b, uint64_t lo, uint64_t hi);
int gce_sort_pass_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                         int32_t n_ref, int32_t last);
int gce_sort_pass_end(gce_sort *b, double *scatter_s);
int gce_sort_sam_contigs(gce_sort *b, int32_t n_ref, const char *const *ref_name);
int gce_sort_sam_window(gce_sort *b, const char *text, size_t n, int32_t n_ref, uint64_t est_bytes, int64_t *n_host_lines, int64_t *bad_line, uint64_t *bad_start, double *parse_s,
                        uint64_t *resident_bytes);
}  // extern "C" (declarations)
extern "C++" {
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
    int fd = -1; uint64_t fsz = 0; struct stat st{}; std::string tmp, msg; bool tmp_made = false;
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
        if (fd >= 0) { ::close(fd); fd = -1; }
    }
    // the input opened, the temporary name made, an output that is the input refused.  who: the entry point; what: the input's kind
    int open_paths(const char *in_path, const char *out_path, const char *who, const char *what) {
        fd = open(in_path, O_RDONLY);
        if (fd < 0) return fail(GCE_ERR_INVALID, std::string("cannot open the input ") + what);
        if (fstat(fd, &st) != 0 || st.st_size < 0) return fail(GCE_ERR_INVALID, std::string("cannot stat the input ") + what);
        fsz = (uint64_t)st.st_size;
        tmp = std::string(out_path) + ".tmp" + std::to_string((long long)getpid());
        {   // the output may not be the input (by name or by file)
            struct stat so;
            bool same = stat(out_path, &so) == 0 && so.st_dev == st.st_dev && so.st_ino == st.st_ino;
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
        if (fsz > 0 && !(fsz >= 4 && looks_gzip(fd, fsz))) return fail(GCE_ERR_INVALID, std::string(who) + " reads BAM, not SAM text");
        if (!starts_bgzf(fd, fsz)) return fail(GCE_ERR_INVALID, "not a BGZF file");
        T = threads > 0 ? threads : default_threads();
        // ---- the header: the host inflates the first members (1 MB pieces) until it is whole
        PassReader rh; rh.fd = fd; rh.fsz = fsz; rh.T = T; rh.piece = window_bytes > 0 ? (size_t)std::min<uint64_t>(window_bytes, (uint64_t)1 << 20) : ((size_t)1 << 20);
        for (;;) {
            const int g = rh.inflate_next();
            if (g < 0) return fail(GCE_ERR_INVALID, rh.msg);
            const uint8_t *u = rh.win.p;
            BamHeader bh;
            const Hdr hs = parse_bam_header(u, rh.n, Contigs::Skip, bh, keep_header ? &names : nullptr);
            if (hs == Hdr::NotBam) return fail(GCE_ERR_INVALID, "not a BAM stream");
            if (hs == Hdr::Complete) {                                               // rule H: the text rewritten, the contig table as it is
                hdr_end = bh.hdr_end; n_ref = (int32_t)bh.n_ref;
                if (keep_header) { hdr.assign(u, u + bh.hdr_end); return GCE_OK; }
                const std::string text = sort_header_text(u + bh.text_off, bh.l_text);
                const uint32_t lt = (uint32_t)text.size();
                hdr.assign(u, u + 4); hdr.insert(hdr.end(), (const uint8_t *)&lt, (const uint8_t *)&lt + 4);
                hdr.insert(hdr.end(), text.begin(), text.end()); hdr.insert(hdr.end(), u + bh.text_off + bh.l_text, u + bh.hdr_end);
                return GCE_OK;
            }
            if (g == 0) return fail(GCE_ERR_INVALID, "truncated BAM header");
        }
    }
    // the file from its first byte, window by window: the host reads and finds the members, window(rd, skip, est) hands them to the GPU.
    // est: the whole file's inflated bytes, from the ISIZE totals so far and the file size.  read_s / gpu_s: the two sides' seconds, added to.
    template <class F> int stream(double *read_s, double *gpu_s, F &&window) {
        PassReader rd; rd.fd = fd; rd.fsz = fsz; rd.T = T; rd.piece = window_bytes > 0 ? (size_t)window_bytes : ((size_t)64 << 20);
        uint64_t comp_seen = 0, infl_seen = 0;
        msg.clear();
        const int rc = for_each_window(rd, hdr_end, read_s, gpu_s, msg, [&](PassReader &r, uint64_t u_all, uint64_t sk) {
            comp_seen += r.used; infl_seen += u_all;
            return window(r, sk, comp_seen ? (uint64_t)((double)infl_seen * ((double)fsz / (double)comp_seen)) : 0);
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
}  // extern "C++"
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
    if (looks_gzip(j.fd, j.fsz)) return done(j.fail(GCE_ERR_INVALID, "gce_sam_sort reads SAM text, not BAM"));
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, device_budget_bytes, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    const uint64_t W = window_bytes ? std::min<uint64_t>(window_bytes, (uint64_t)1 << 30) : ((uint64_t)64 << 20), LONGEST = (uint64_t)256 << 20;
    std::unique_ptr<Pinned> buf(new Pinned());                                       // the window: what the last one left over, then the next piece of the file
    uint64_t have = 0, at = 0, base = 0, text_seen = 0, rec_bytes = 0;                              // base: the file offset of buf[0]
    bool in_header = true; std::string text; std::vector<std::string> names; std::vector<uint32_t> lens; int32_t n_ref = 0;
    // the line that starts at file offset `o`, counting from 1 over the file (an error's path only: the file is read once more up to there)
    auto line_number = [&](uint64_t o) {
        long long ln = 1; std::vector<char> pb((size_t)1 << 20);
        for (uint64_t a = 0; a < o;) { const ssize_t g = pread(j.fd, pb.data(), (size_t)std::min<uint64_t>(pb.size(), o - a), (off_t)a); if (g <= 0) break; ln += (long long)std::count(pb.data(), pb.data() + g, '\n'); a += (uint64_t)g; }
        return ln;
    };
    for (bool last = j.fsz == 0; ;) {
        double t0 = now_s();
        if (!last) {
            const uint64_t want = std::min<uint64_t>(W, j.fsz - at);
            if (have + want + 64 > buf->cap) {
                std::unique_ptr<Pinned> nb(new Pinned());
                if (!nb->ensure((size_t)(have + want + 64))) return done(j.fail(GCE_ERR_OOM, "out of pinned host memory"));
                if (have) memcpy(nb->p, buf->p, (size_t)have);
                buf.swap(nb);
            }
            if (pread_full(j.fd, buf->p + have, (size_t)want, at) != (size_t)want) return done(j.fail(GCE_ERR_INVALID, "cannot read the input SAM"));
            have += want; at += want; last = at >= j.fsz;
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
            const uint64_t est = text_seen ? (uint64_t)((double)rec_bytes * ((double)j.fsz / (double)text_seen)) : 0;
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

// ---- NM and MD recomputed against the reference (gce_calmd.hpp)
int gce_sort_calmd_ref(gce_sort *b, int32_t n_ref, const char *const *seq, const int64_t *len);
int gce_sort_calmd_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                          int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s);
int gce_sort_calmd_finish(gce_sort *b, int32_t codes, uint64_t piece_bytes, int64_t counts[6], uint64_t *in_bytes, uint64_t *out_bytes);

}  // extern "C"
extern "C++" {
namespace {
// what gce_bam_calmd and gce_bam_calmd_stream refuse before a device is touched, beside their NULL arguments
int calmd_check(int level, const char *fasta_path, char err[256]) {
    if (level < -3 || level > 9) { set_err(err, "level should be -3, -2, -1 or 0..9"); return GCE_ERR_INVALID; }
    struct stat sf;
    if (stat(fasta_path, &sf) != 0 || S_ISDIR(sf.st_mode)) { set_err(err, "cannot open the reference FASTA"); return GCE_ERR_INVALID; }
    return GCE_OK;
}
// rule R: the FASTA loaded (*fa: the caller frees it once the bases are on the device) and, per contig of j's header, its bases and their
// length as gce_sort_calmd_ref takes them, matched by name
int calmd_contigs(SortJob &j, const char *fasta_path, gce_fasta **fa, std::vector<const char *> &seq, std::vector<int64_t> &len) {
    const int rc = gce_fasta_load(fasta_path, j.T, fa);
    if (rc != GCE_OK) return j.fail(rc, "cannot read the reference FASTA");
    seq.assign((size_t)j.n_ref, nullptr); len.assign((size_t)j.n_ref, -1);
    int32_t nc = 0; const char *const *ids = nullptr; const char *const *seqs = nullptr; const int64_t *flen = nullptr;
    gce_fasta_get(*fa, &nc, &ids, &seqs, &flen);
    std::unordered_map<std::string, int32_t> where;
    for (int32_t c = 0; c < nc; c++) where.emplace(ids[c], c);
    for (int32_t t = 0; t < j.n_ref; t++) {
        auto it = where.find(j.names[(size_t)t].c_str());                              // (the name up to its first NUL)
        if (it != where.end()) { seq[(size_t)t] = seqs[it->second]; len[(size_t)t] = flen[it->second]; }
    }
    return GCE_OK;
}
}  // namespace
}  // extern "C++"
extern "C" {

int gce_bam_calmd(const char *in_path, const char *out_path, const char *fasta_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes,
                  gce_calmd_run *out, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !fasta_path || !out) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out);
    { const int rc = calmd_check(level, fasta_path, err); if (rc != GCE_OK) return rc; }
    const double t_start = now_s();
    SortJob j; j.who = "gce_bam_calmd"; j.keep_header = true;
    gce_fasta *fa = nullptr;
    auto done = [&](int code) { j.close_all(code); if (fa) gce_fasta_free(fa); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    out->n_ref = n_ref;
    // ---- rule R: the contigs by the header's names
    double t0 = now_s();
    std::vector<const char *> seq; std::vector<int64_t> len;
    if ((rc = calmd_contigs(j, fasta_path, &fa, seq, len)) != GCE_OK) return done(rc);
    out->read_s += now_s() - t0;
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, device_budget_bytes, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    if ((rc = gce_sort_calmd_ref(j.b, n_ref, seq.data(), len.data())) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    gce_fasta_free(fa); fa = nullptr;
    // ---- the file from its first byte, window by window: the GPU inflates, indexes and rewrites the records behind the resident output
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_calmd_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est,
                                     &out->calmd_s); });
    if (rc != GCE_OK) return done(rc);
    out->inflate_index_s -= out->calmd_s;
    j.set_pieces();
    int64_t counts[6] = {0, 0, 0, 0, 0, 0}; uint64_t in_bytes = 0, total = 0;
    if ((rc = gce_sort_calmd_finish(j.b, j.codes, j.piece, counts, &in_bytes, &total)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    out->n_records = counts[0]; out->n_rewritten = counts[1]; out->n_unchanged = counts[2]; out->n_no_ref = counts[3]; out->n_nm_changed = counts[4]; out->n_md_changed = counts[5];
    out->inflated_bytes = (int64_t)in_bytes; out->out_record_bytes = (int64_t)total;
    // ---- rule F
    t0 = now_s();
    if ((rc = j.begin_output(total)) != GCE_OK || (rc = j.write_range(total)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = now_s() - t0;
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

// gce_bam_calmd with its output streamed: the temporary output is open from the first window on, and whenever the next window's output would
// take the resident record bytes past the cap R, the whole members of 0xff00 bytes resident so far are written and let go
int gce_sort_calmd_stream_begin(gce_sort *b, int32_t codes, uint64_t piece_bytes, uint64_t resident_bytes);
int gce_sort_calmd_stream_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                                 int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s, int (*flush)(void *ctx, uint64_t n), void *ctx);
int gce_sort_calmd_consume(gce_sort *b, uint64_t n);
int gce_sort_calmd_stream_stats(gce_sort *b, int32_t *n_flushes, uint64_t *resident_cap_bytes, uint64_t *flushed_bytes);

int gce_bam_calmd_stream(const char *in_path, const char *out_path, const char *fasta_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes,
                         uint64_t resident_bytes, gce_calmd_run *out, gce_calmd_stream_run *run, char err[256]) {
    set_err(err, "");
    if (!in_path || !out_path || !fasta_path || !out || !run) { set_err(err, "bad argument"); return GCE_ERR_INVALID; }
    memset(out, 0, sizeof *out); memset(run, 0, sizeof *run);
    { const int rc = calmd_check(level, fasta_path, err); if (rc != GCE_OK) return rc; }
    const double t_start = now_s();
    SortJob j; j.who = "gce_bam_calmd_stream"; j.keep_header = true;
    gce_fasta *fa = nullptr;
    auto done = [&](int code) { j.close_all(code); if (fa) gce_fasta_free(fa); set_err(err, j.msg.c_str()); return code; };
    int rc = j.open_input(in_path, out_path, threads, level, window_bytes, device);
    if (rc != GCE_OK) return done(rc);
    const int32_t n_ref = j.n_ref;
    out->n_ref = n_ref;
    uint64_t budget = device_budget_bytes;
    if (!budget) {
        size_t fr = 0, tot = 0;
        const int r0 = gce_device_mem_info(device, &fr, &tot);
        if (r0 != GCE_OK) return done(j.fail(r0, "no HIP device"));
        budget = std::max<uint64_t>((uint64_t)((double)fr * GCE_PASS_BUDGET_FRACTION), 1);
    }
    // ---- rule R: the contigs by the header's names
    double t0 = now_s();
    std::vector<const char *> seq; std::vector<int64_t> len;
    if ((rc = calmd_contigs(j, fasta_path, &fa, seq, len)) != GCE_OK) return done(rc);
    out->read_s += now_s() - t0;
    const uint64_t M = PassWriter::BS;
    j.set_pieces();
    (void)gce_device_bytes(nullptr, nullptr, 1);
    if ((rc = gce_sort_create(device, (size_t)budget, &j.b)) != GCE_OK) return done(j.fail(rc, "no HIP device"));
    if ((rc = gce_sort_calmd_stream_begin(j.b, j.codes, j.piece, (resident_bytes + M - 1) / M * M)) != GCE_OK) return done(j.fail(rc, "bad argument"));
    if ((rc = gce_sort_calmd_ref(j.b, n_ref, seq.data(), len.data())) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    gce_fasta_free(fa); fa = nullptr;
    // ---- rule F from the first window on: the header's members now, the record stream's as they are flushed
    if ((rc = j.begin_output(0)) != GCE_OK) return done(rc);
    struct Flush { SortJob *j; double s; } fl = {&j, 0};
    auto flush = [](void *ctx, uint64_t n) {
        Flush &f = *(Flush *)ctx;
        const double f0 = now_s();
        int r = f.j->host_room(n);
        if (r == GCE_OK) r = f.j->write_range(n);
        if (r == GCE_OK && (r = gce_sort_calmd_consume(f.j->b, n)) != GCE_OK) r = f.j->fail(r, gce_sort_error(f.j->b));
        f.s += now_s() - f0;
        return r;
    };
    // ---- the file from its first byte, window by window: the GPU inflates, indexes and rewrites the records behind the resident output
    rc = j.stream(&out->read_s, &out->inflate_index_s, [&](PassReader &rd, uint64_t sk, uint64_t est) {
        return gce_sort_calmd_stream_window(j.b, rd.comp.data(), rd.used, (int32_t)rd.blocks.size(), rd.z_coff.data(), rd.z_csize.data(), rd.z_usize.data(), sk, n_ref, rd.last_piece() ? 1 : 0, est,
                                            &out->calmd_s, flush, &fl); });
    if (rc != GCE_OK) return done(rc);
    out->inflate_index_s -= out->calmd_s + fl.s;
    { uint64_t cap = 0, flushed = 0; (void)gce_sort_calmd_stream_stats(j.b, &run->n_flushes, &cap, &flushed); run->resident_cap_bytes = (int64_t)cap; run->flushed_bytes = (int64_t)flushed; }
    int64_t counts[6] = {0, 0, 0, 0, 0, 0}; uint64_t in_bytes = 0, rest = 0;
    if ((rc = gce_sort_calmd_finish(j.b, j.codes, j.piece, counts, &in_bytes, &rest)) != GCE_OK) return done(j.fail(rc, gce_sort_error(j.b)));
    out->n_records = counts[0]; out->n_rewritten = counts[1]; out->n_unchanged = counts[2]; out->n_no_ref = counts[3]; out->n_nm_changed = counts[4]; out->n_md_changed = counts[5];
    out->inflated_bytes = (int64_t)in_bytes; out->out_record_bytes = (int64_t)((uint64_t)run->flushed_bytes + rest);
    // ---- the rest with the last short member, the EOF marker, the rename
    t0 = now_s();
    if ((rc = j.host_room(rest)) != GCE_OK || (rc = j.write_range(rest)) != GCE_OK || (rc = j.end_output(out_path, &out->out_bytes)) != GCE_OK) return done(rc);
    out->write_s = fl.s + (now_s() - t0);
    { int64_t pk = 0; (void)gce_device_bytes(nullptr, &pk, 0); out->peak_device_bytes = pk; }
    out->total_s = now_s() - t_start;
    return done(GCE_OK);
}

}  // extern "C"
