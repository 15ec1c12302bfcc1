// bamio.cpp — the file side of the C-ABI (include/gencore_amd.h, "files" section): this file's host-only formats and, in the parts it includes,
// the runners that drive the GPU.
//
// Host only, here: the whole-file BAM reader (gce_bam_open / gce_bam_chunk: records -> gce_batch) and writer (gce_bam_write), SAM text <-> BAM
// (gce_samtext.hpp), the FASTA and BED loaders, the reports (gce_report.hpp).  They replace what the reference does through htslib and
// FastaReader around the hot path:
//   sam_open / sam_hdr_read / sam_read1        src/gencore.cpp:164-205      -> gce_bam_open (+ gce_bam_chunk)
//   sam_hdr_write / sam_write1 / sam_close     src/gencore.cpp:187-190,104  -> gce_bam_write (result rows -> records -> BGZF)
//   FastaReader::readAll / readNext / to4bits  src/fastareader.cpp:57-104,139-152,157-168 -> gce_fasta_load
// htslib itself is a pinned dependency that is absent from the reference tree; the formats are the published ones (SAMv1 section 4).
//
// Drivers of the GPU, one runner family per part, included at the end in this order:
//   bamio_run.hpp     gce_run_bam (+ sharded, depth) and the host-codec runners
//   bamio_passes.hpp  gce_run_bam_passes
//   bamio_index.hpp   gce_bam_index
//   bamio_sort.hpp    gce_bam_sort, gce_bam_sort_passes, gce_sam_sort
//   bamio_calmd.hpp   gce_bam_calmd, gce_bam_calmd_stream
//   bamio_overlap.hpp gce_bam_merge_overlap
//   bamio_umi.hpp     gce_bam_umi_to_mi
//   bamio_varmask.hpp gce_mask_load, the variant mask of the error profile (host only)
//   bamio_reduce.hpp  reduce_run, the runner of the reduce passes
//   bamio_pileup.hpp  gce_bam_pileup
//   bamio_fragpile.hpp gce_bam_pileup_fragments
//   bamio_errprof.hpp gce_bam_error_profile
//   bamio_fragerr.hpp gce_bam_error_profile_fragments
//   bamio_errsup.hpp  gce_bam_error_profile_support
//   bamio_errqual.hpp gce_bam_error_profile_quality
// No part launches a kernel itself: the runners read the file, find its BGZF members and hand them, window by window, to the engine's entry
// points in engine.hip (gce_raw_* of the public header; gce_passes_*, gce_bai_*, gce_sort_*, gce_pileup_*, gce_fragpile_*, gce_errprof_*, gce_fragerr_* of gce_entry.h, the one place they are declared),
// which inflate, index, process, sort and deflate in HBM; the output comes back in pieces and is written on the host.
//
// One copy of each shared piece: member framing, the BAM header, the member codec, the EOF member and the file helpers are in gce_bgzf.hpp;
// the output file in gce_fileout.hpp; the clock, the input file, pinned buffers and the engine set-up in bamio_common.hpp; PassReader (a
// file's members, piece by piece), read_bam_header, read_stream_header and for_each_window (the window loop of the index, sort and reduce
// runners) in bamio_reader.hpp; the FASTA's contigs matched by name (match_contigs) in bamio_common.hpp; the runner of the pileup and the error
// profile (reduce_run) in bamio_reduce.hpp;
// PassWriter (a record stream in rounds of 0xff00-byte members deflated on all host threads, or by the GPU) in bamio_writer.hpp.  Each part
// is an anonymous-namespace helper section, then one extern "C" block of entry points.
// Everything that scales with the file is spread over `threads` host threads: inflate per BGZF block, the struct-of-arrays fill
// per record range, record rebuild + deflate per output block.
#include <zlib.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../include/gencore_amd.h"
#include "gce_bgzf.hpp"
#include "gce_samtext.hpp"
#include "gce_fileout.hpp"
#include "gce_report.hpp"
#include "bamio_common.hpp"

namespace {

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

// records [first, first + count) as a gce_batch in one of the two chunk slots (offsets relative to the slot's blobs)
// records first .. first + count - 1, or (sel != nullptr) the records sel[0 .. count - 1] in that order
int bam_chunk_impl(gce_bam *f, int64_t first, const int64_t *sel, int64_t count, Slot &s, gce_batch *out) {
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
// the rows of an output table as BAM records: row k = input record src[k] with the name of record qname_src[k], the bases / qualities
// at seqp(k) / qualp(k), NM patched, FR / RR appended (gce_result's meaning; one table, or several engines' tables merged)
struct OutRows { int64_t n; const uint32_t *src, *qname_src; const int32_t *nm_new; const int16_t *fr, *rr; };
template <class SP, class QP>
int bam_write_rows(const char *path, const gce_bam *in, const OutRows rows, SP seqp, QP qualp, int threads, int level) {
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

int gce_bam_chunk(gce_bam *f, int64_t first, int64_t count, int slot_id, gce_batch *out) {
    if (!f || !out || first < 0 || count < 0 || first + count > (int64_t)f->rec.size() || (slot_id != 0 && slot_id != 1)) return GCE_ERR_INVALID;
    return bam_chunk_impl(f, first, nullptr, count, f->slot[slot_id], out);
}

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

// ------------------------------------------------------------------------------------------------------------ FASTA (gce_fasta: above)
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

}  // extern "C"

// ---- the file-to-file runners, one family per part
#include "bamio_run.hpp"
#include "bamio_passes.hpp"
#include "bamio_index.hpp"
#include "bamio_sort.hpp"
#include "bamio_calmd.hpp"
#include "bamio_overlap.hpp"
#include "bamio_umi.hpp"
#include "bamio_varmask.hpp"
#include "bamio_pileup.hpp"
#include "bamio_fragpile.hpp"
#include "bamio_errprof.hpp"
#include "bamio_fragerr.hpp"
#include "bamio_errsup.hpp"
#include "bamio_errqual.hpp"
