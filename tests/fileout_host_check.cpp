// The host-only output pieces of gencore_amd/csrc/gce_fileout.hpp -- the piece pump, the output file, records -> lines and lines -> records --
// in a program of their own, built with the address and undefined-behaviour sanitizers (tests/test_fileout_host.py).  The pump runs over a
// fake device: fetch only notes the request, the bytes arrive when its ticket is waited for; the buffers are heap blocks of exactly the size
// the pump asked for.
// Usage: fileout_host_check DIR   (DIR/manifest: one case per line; one output line per case; exit 1 when a pump case breaks a rule)
//   pump PIECE TOTAL PREFIX          "... ok fetches=N waits=N sinks=n,n,..."; the rules are checked here, the counts by the test's model
//   fail WHO J PIECE TOTAL PREFIX    the callable WHO (fetch, wait, sink) fails with -77 at its piece J: "... status=S later=N" (callables run afterwards)
//   r2l NAME T                       DIR/NAME (records; DIR/names: the contigs) -> "lines=<CRC-32>:<bytes>" or "lines=bad", then whole_records' end
//   l2r NAME T nl|cut                DIR/NAME (text; nl: a line feed added where the text lacks its last one; cut: up to the last line feed)
//                                    -> "ok:<CRC-32>:<bytes>:left=<bytes behind lim>" or "err:<message>"
//   outfile                          open in a missing directory, the BAM close, the SAM close, the name test
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../gencore_amd/csrc/gce_fileout.hpp"

static std::string slurp(const std::string &p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }
static uint8_t stream_byte(uint64_t i) { return (uint8_t)(i * 131 + 7); }
static uint8_t prefix_byte(uint64_t i) { return (uint8_t)((i * 17 + 3) ^ 0xA5); }

struct Exact {                                        // a buffer of exactly the bytes asked for
    uint8_t *p = nullptr; size_t cap = 0;
    ~Exact() { free(p); }
    bool ensure(size_t n) { if (n <= cap) return true; free(p); p = (uint8_t *)malloc(n); cap = p ? n : 0; return p != nullptr; }
};

struct Fake {
    Exact buf[2]; bool unseen[2] = {false, false};    // unseen[b]: buf[b] was fetched into and the sink has not been given it yet
    struct Req { uint64_t off; uint8_t *dst; size_t n; bool done; };
    std::vector<Req> reqs; std::string got; std::vector<size_t> sinks;
    int fetches = 0, waits = 0, calls = 0, fail_at = -1, later = 0; std::string fail_who; bool failed = false, broke = false;
    int which(const uint8_t *p) const { for (int b = 0; b < 2; b++) if (buf[b].p && p >= buf[b].p && p < buf[b].p + buf[b].cap) return b; return -1; }
    int step(const char *who, int k) { if (failed) later++; if (!failed && fail_who == who && fail_at == k) { failed = true; return -77; } return GCE_OK; }
    int run(uint64_t piece, uint64_t total, uint64_t prefix_n) {
        std::vector<uint8_t> prefix((size_t)prefix_n);
        for (uint64_t i = 0; i < prefix_n; i++) prefix[(size_t)i] = prefix_byte(i);
        int sink_k = 0;
        return pump_pieces(prefix.data(), prefix_n, total, piece, buf,
            [&](uint64_t off, uint8_t *dst, size_t n, int32_t *tk) -> int {
                const int r = step("fetch", fetches); if (r) return r;
                const int b = which(dst);
                if (b < 0 || unseen[b] || off + n > total || n == 0) broke = true; else unseen[b] = true;
                reqs.push_back(Req{off, dst, n, false}); *tk = (int32_t)reqs.size() - 1; fetches++;
                return GCE_OK;
            },
            [&](int32_t tk) -> int {
                const int r = step("wait", waits); if (r) return r;
                if (tk < 0 || (size_t)tk >= reqs.size() || reqs[(size_t)tk].done) { broke = true; return GCE_OK; }
                Req &q = reqs[(size_t)tk]; q.done = true; waits++;
                for (size_t i = 0; i < q.n; i++) q.dst[i] = stream_byte(q.off + i);      // the copy "completes" here
                return GCE_OK;
            },
            [&](const uint8_t *p, size_t n) -> int {
                const int r = step("sink", sink_k); if (r) return r;
                sink_k++;
                const int b = which(p);
                if (b < 0 || p != buf[b].p || n > piece || n == 0) broke = true; else unseen[b] = false;
                got.append((const char *)p, n); sinks.push_back(n);
                return GCE_OK;
            });
    }
};

static bool pump_case(uint64_t piece, uint64_t total, uint64_t prefix_n) {
    Fake f;
    const int rc = f.run(piece, total, prefix_n);
    bool ok = rc == GCE_OK && !f.broke && f.got.size() == prefix_n + total;
    for (uint64_t i = 0; ok && i < prefix_n + total; i++) ok = (uint8_t)f.got[(size_t)i] == (i < prefix_n ? prefix_byte(i) : stream_byte(i - prefix_n));
    for (auto &q : f.reqs) ok = ok && q.done;                                      // every ticket issued was waited for
    printf("pump %llu %llu %llu %s fetches=%d waits=%d sinks=", (unsigned long long)piece, (unsigned long long)total, (unsigned long long)prefix_n, ok ? "ok" : "FAIL", f.fetches, f.waits);
    for (size_t k = 0; k < f.sinks.size(); k++) printf("%s%zu", k ? "," : "", f.sinks[k]);
    printf("\n");
    return ok;
}

static bool fail_case(const std::string &who, int j, uint64_t piece, uint64_t total, uint64_t prefix_n) {
    Fake f; f.fail_who = who; f.fail_at = j;
    const int rc = f.run(piece, total, prefix_n);
    printf("fail %s %d %llu %llu %llu status=%d later=%d\n", who.c_str(), j, (unsigned long long)piece, (unsigned long long)total, (unsigned long long)prefix_n, rc, f.later);
    return !f.broke;
}

static void r2l_case(const std::string &dir, const std::string &name, int T) {
    const std::string d = slurp(dir + "/" + name);
    std::vector<std::string> names; { std::istringstream nf(slurp(dir + "/names")); std::string x; while (nf >> x) names.push_back(x); }
    uint8_t *buf = (uint8_t *)malloc(d.size() ? d.size() : 1); memcpy(buf, d.data(), d.size());
    std::vector<uint64_t> ro, ro2;
    for (size_t o = 0; o + 4 <= d.size() && o + 4 + (size_t)rd32(buf + o) <= d.size(); o += 4 + (size_t)rd32(buf + o)) ro.push_back(o);      // every whole record, a short one too: records_to_lines judges it
    std::vector<std::string> lines;
    printf("r2l %s %d ", name.c_str(), T);
    if (records_to_lines(buf, ro, names, T, lines)) {
        std::string all; for (auto &L : lines) all += L;
        printf("lines=%08lx:%zu", (unsigned long)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)all.data(), (uInt)all.size()), all.size());
        if (lines.size() != (size_t)T) printf(" FAIL");
    } else printf("lines=bad");
    const size_t end = whole_records(buf, d.size(), ro2);
    if (end == SIZE_MAX) printf(" whole=bad\n"); else printf(" whole=%zu:%zu\n", end, ro2.size());
    free(buf);
}

static void l2r_case(const std::string &dir, const std::string &name, int T, const std::string &mode) {
    std::string d = slurp(dir + "/" + name);
    std::vector<std::string> names; { std::istringstream nf(slurp(dir + "/names")); std::string x; while (nf >> x) names.push_back(x); }
    samtext::NameMap nmap; nmap.build(names);
    size_t lim = d.size();
    if (mode == "nl") { if (!d.empty() && d.back() != '\n') d.push_back('\n'); lim = d.size(); }
    else { const size_t nl = d.rfind('\n'); lim = nl == std::string::npos ? 0 : nl + 1; }
    char *text = (char *)malloc(d.size() ? d.size() : 1); memcpy(text, d.data(), d.size());      // (exactly the text: a read behind it is reported)
    std::vector<std::vector<uint8_t>> parts; std::vector<std::string> perr;
    const char *m = lines_to_records(text, 0, lim, T, nmap, parts, perr);
    printf("l2r %s %d %s ", name.c_str(), T, mode.c_str());
    if (m) printf("err:%s\n", m);
    else {
        std::string all; for (auto &v : parts) all.append((const char *)v.data(), v.size());
        printf("ok:%08lx:%zu:left=%zu%s\n", (unsigned long)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)all.data(), (uInt)all.size()), all.size(), d.size() - lim, parts.size() == (size_t)T ? "" : " FAIL");
    }
    free(text);
}

static bool outfile_case(const std::string &dir) {
    bool ok = true;
    { OutFile f; ok = ok && !f.open((dir + "/no_such_directory/out.bam").c_str(), false) && f.fo == nullptr; }
    {
        OutFile f; const std::string p = dir + "/o.bam";
        ok = ok && f.open(p.c_str(), OutFile::named_sam(p.c_str())) && !f.sam && f.write("xyz", 3) && f.close() && f.fo == nullptr;
        ok = ok && slurp(p) == "xyz" + std::string((const char *)BGZF_EOF, 28);
    }
    {
        OutFile f; const std::string p = dir + "/o.sam";
        const std::vector<std::string> nm = {"chrA", "b"}; const std::vector<uint32_t> ln = {7, 9};
        ok = ok && f.open(p.c_str(), OutFile::named_sam(p.c_str())) && f.sam && f.sam_header("@HD\tVN:1.6\n", nm, ln) && f.write("r\n", 2) && f.close();
        ok = ok && slurp(p) == "@HD\tVN:1.6\n@SQ\tSN:chrA\tLN:7\n@SQ\tSN:b\tLN:9\nr\n";
    }
    {   // the header's members: one member of the header's bytes, by the host
        OutFile f; const std::string p = dir + "/h.bam"; const std::vector<uint8_t> hdr = {'B', 'A', 'M', 1, 0, 0, 0, 0, 0, 0, 0, 0};
        ok = ok && f.open(p.c_str(), false) && f.reserve() && f.header_members(hdr, 6, true, 2) && f.close();
        const std::string z = slurp(p); Member m;
        ok = ok && scan_member((const uint8_t *)z.data(), z.size(), 0, m) == Scan::Member && m.isize == hdr.size() && z.size() == m.bsize + 28;
    }
    ok = ok && OutFile::named_sam("a.sam") && OutFile::named_sam("sam") && !OutFile::named_sam("am") && !OutFile::named_sam("x.bam") && !OutFile::named_sam("x.SAM") && !OutFile::named_sam("x.sam.tmp12");
    printf("outfile %s\n", ok ? "ok" : "FAIL");
    return ok;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: fileout_host_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::istringstream man(slurp(dir + "/manifest"));
    std::string kind; bool ok = true;
    while (man >> kind) {
        if (kind == "pump") { unsigned long long a, b, c; man >> a >> b >> c; ok = pump_case(a, b, c) && ok; }
        else if (kind == "fail") { std::string who; int j; unsigned long long a, b, c; man >> who >> j >> a >> b >> c; ok = fail_case(who, j, a, b, c) && ok; }
        else if (kind == "r2l") { std::string name; int T; man >> name >> T; r2l_case(dir, name, T); }
        else if (kind == "l2r") { std::string name, mode; int T; man >> name >> T >> mode; l2r_case(dir, name, T, mode); }
        else if (kind == "outfile") ok = outfile_case(dir) && ok;
        else { fprintf(stderr, "unknown case kind %s\n", kind.c_str()); return 2; }
    }
    return ok ? 0 : 1;
}
