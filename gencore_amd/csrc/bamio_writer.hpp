// bamio_writer.hpp -- the output side the pass runner and the sort runners share: PassKey / pass_less (the order the pass runner merges in)
// and PassWriter (a record stream written a round of BGZF members at a time, or as SAM lines).
#pragma once
#include "bamio_common.hpp"
#include "gce_fileout.hpp"

namespace {

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
