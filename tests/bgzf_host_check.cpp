// The host-only BGZF / BAM-header pieces of gencore_amd/csrc/gce_bgzf.hpp -- the member scanner, the header parser in its two dialects and the
// member codec -- in a program of their own, built with the address and undefined-behaviour sanitizers (tests/test_bgzf_host.py).  Every
// buffer handed to the scanner and the parser is a heap block of exactly the bytes it may read, so a read at or beyond `have` is reported.
// Usage: bgzf_host_check DIR   (DIR/manifest: one case per line; one output line per case and dialect; exit 1 on any failure)
//   scan NAME          DIR/NAME at every prefix length: "L,members,end" per prefix; end: "more" or the scanner's message
//   hdr NAME           DIR/NAME at every prefix length, once per dialect: "L=notbam", "L=incomplete" or
//                      "L=complete:text_off:l_text:n_ref:hdr_end[:name/length ...]" (the names only where the dialect collects them)
//   codec NAME LEVEL   DIR/NAME through deflate_block, scan_member and inflate_block; the member is appended to DIR/NAME.LEVEL.gz
//   inflate NAME USIZE DIR/NAME, one member in a heap block of exactly its bytes, through inflate_block into a heap block of exactly USIZE
//                      bytes: "ok:<CRC-32 of the output, hex>" or "refused" (inflate_raw's word copies stay below out_end by their own condition);
//                      then the table decoder alone, fastinf::inflate_raw, on blocks of the same kind: "raw:ok:<CRC-32>" or "raw:refused"
//                      (inflate_block hides it: whatever it refuses or gets wrong goes to zlib)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../gencore_amd/csrc/gce_bgzf.hpp"

static std::string slurp(const std::string &p) { std::ifstream f(p, std::ios::binary); std::stringstream s; s << f.rdbuf(); return s.str(); }

// the first n bytes of d in a heap block of exactly n bytes
struct Exact {
    uint8_t *p;
    Exact(const std::string &d, size_t n) : p((uint8_t *)malloc(n ? n : 1)) { if (n) memcpy(p, d.data(), n); }
    ~Exact() { free(p); }
};

static void scan_case(const std::string &name, const std::string &d) {
    printf("scan %s", name.c_str());
    for (size_t L = 0; L <= d.size(); L++) {
        Exact b(d, L);
        size_t off = 0, members = 0; Member m; Scan s;
        while ((s = scan_member(b.p, L, off, m)) == Scan::Member) { off += m.bsize; members++; }
        printf("%c%zu,%zu,%s", L ? ';' : ' ', L, members, s == Scan::More ? "more" : scan_message(s));
    }
    printf("\n");
}

static void hdr_case(const std::string &name, const std::string &d, Contigs dialect) {
    printf("hdr %s %s", name.c_str(), dialect == Contigs::Collect ? "collect" : "skip");
    for (size_t L = 0; L <= d.size(); L++) {
        Exact b(d, L);
        BamHeader h; std::vector<std::string> names; std::vector<uint32_t> lens;
        const bool collect = dialect == Contigs::Collect;
        const Hdr r = parse_bam_header(b.p, L, dialect, h, collect ? &names : nullptr, collect ? &lens : nullptr);
        printf("%c%zu=", L ? ';' : ' ', L);
        if (r == Hdr::NotBam) printf("notbam");
        else if (r == Hdr::Incomplete) printf("incomplete");
        else {
            printf("complete:%llu:%u:%u:%llu", (unsigned long long)h.text_off, h.l_text, h.n_ref, (unsigned long long)h.hdr_end);
            for (size_t k = 0; k < names.size(); k++) printf(":%s/%u", names[k].c_str(), lens[k]);
        }
    }
    printf("\n");
}

static bool codec_case(const std::string &dir, const std::string &name, int level) {
    const std::string d = slurp(dir + "/" + name);
    Exact src(d, d.size());
    std::vector<uint8_t> z(0x10000 + 64);
    const size_t zs = deflate_block(src.p, (uint32_t)d.size(), level, z.data());
    bool ok = zs != 0;
    Member m;
    if (ok) { Exact zb(std::string((const char *)z.data(), zs), zs); ok = scan_member(zb.p, zs, 0, m) == Scan::Member && m.bsize == zs && m.isize == d.size(); }
    if (ok) {
        Exact zb(std::string((const char *)z.data(), zs), zs);
        std::vector<uint8_t> u(d.size() + 64);                                         // (inflate_raw copies matches in 8-byte words: the callers' buffers have this room)
        Block b; b.coff = 0; b.csize = (uint32_t)zs; b.usize = m.isize; b.uoff = 0;
        ok = inflate_block(zb.p, b, u.data()) && memcmp(u.data(), d.data(), d.size()) == 0;
    }
    if (ok) { std::ofstream f(dir + "/" + name + "." + std::to_string(level) + ".gz", std::ios::binary); f.write((const char *)z.data(), (std::streamsize)zs); }
    printf("codec %s %d %s\n", name.c_str(), level, ok ? "ok" : "FAIL");
    return ok;
}

static void inflate_case(const std::string &dir, const std::string &name, uint32_t usize) {
    const std::string d = slurp(dir + "/" + name);
    Exact src(d, d.size());
    uint8_t *dst = (uint8_t *)malloc(usize ? usize : 1);
    Block b; b.coff = 0; b.csize = (uint32_t)d.size(); b.usize = usize; b.uoff = 0;
    if (inflate_block(src.p, b, dst)) printf("inflate %s ok:%08lx", name.c_str(), (unsigned long)crc32(crc32(0L, Z_NULL, 0), dst, usize));
    else printf("inflate %s refused", name.c_str());
    free(dst);
    dst = (uint8_t *)malloc(usize ? usize : 1);
    const uint32_t xlen = rd16(src.p + 10);
    if (fastinf::inflate_raw(src.p + 12 + xlen, d.size() - 12 - xlen - 8, dst, usize)) printf(" raw:ok:%08lx\n", (unsigned long)crc32(crc32(0L, Z_NULL, 0), dst, usize));
    else printf(" raw:refused\n");
    free(dst);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: bgzf_host_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::istringstream man(slurp(dir + "/manifest"));
    std::string kind, name; bool ok = true;
    while (man >> kind >> name) {
        if (kind == "scan") scan_case(name, slurp(dir + "/" + name));
        else if (kind == "hdr") { const std::string d = slurp(dir + "/" + name); hdr_case(name, d, Contigs::Collect); hdr_case(name, d, Contigs::Skip); }
        else if (kind == "inflate") { uint32_t usize = 0; man >> usize; inflate_case(dir, name, usize); }
        else if (kind == "codec") { int level = 0; man >> level; ok = codec_case(dir, name, level) && ok; }
        else { fprintf(stderr, "unknown case kind %s\n", kind.c_str()); return 2; }
    }
    // the shared small pieces: the EOF member is a whole, empty member; bam_header_bytes parses back to what went in
    Member m;
    if (scan_member(BGZF_EOF, sizeof BGZF_EOF, 0, m) != Scan::Member || m.bsize != 28 || m.isize != 0) { printf("eof FAIL\n"); ok = false; } else printf("eof ok\n");
    const std::vector<std::string> nm = {"chrA", "b"}; const std::vector<uint32_t> ln = {7, 9};
    const std::vector<uint8_t> hb = bam_header_bytes("@HD\n", nm, ln);
    BamHeader h; std::vector<std::string> n2; std::vector<uint32_t> l2;
    if (parse_bam_header(hb.data(), hb.size(), Contigs::Collect, h, &n2, &l2) != Hdr::Complete || n2 != nm || l2 != ln || h.hdr_end != hb.size() || h.l_text != 4) { printf("header_bytes FAIL\n"); ok = false; }
    else printf("header_bytes ok\n");
    return ok ? 0 : 1;
}
