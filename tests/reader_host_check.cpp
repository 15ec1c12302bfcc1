// The host's file reader (gencore_amd/csrc/bamio_reader.hpp: PassReader::members_next and read_bam_header, the one loop that inflates a
// file's first members until its BAM header is whole) in a program of its own, without HIP: the reader's pinned window comes from malloc
// through the two functions below.  Built with the address and undefined-behaviour sanitizers (tests/test_reader_host.py).
// Usage: reader_host_check DIR   -- writes its case files into DIR, prints one line per case, exit 2 if a file could not be made.
//   header NAME DIALECT[+name] piece=P -> OUTCOME [hdr_end n_ref inflated-bytes [contigs] [first name or -]]   (Failed: the reader's words)
//   members NAME piece=P -> the whole members every members_next call hands out, then "end" or the reader's words
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../gencore_amd/csrc/bamio_reader.hpp"

extern "C" int gce_host_alloc(size_t bytes, void **out) { *out = malloc(bytes ? bytes : 1); return *out ? GCE_OK : GCE_ERR_OOM; }
extern "C" void gce_host_free(void *p) { free(p); }

typedef std::vector<uint8_t> Bytes;

static Bytes member(const Bytes &d, size_t a, size_t b) {                              // d[a, b) as one BGZF member of stored bytes: its size depends on b - a alone
    std::vector<uint8_t> z(0x10000 + 64);
    const size_t zs = deflate_block(d.data() + a, (uint32_t)(b - a), 0, z.data());
    if (!zs) { fprintf(stderr, "deflate_block failed\n"); exit(2); }
    return Bytes(z.begin(), z.begin() + (ptrdiff_t)zs);
}
static void add(Bytes &f, const Bytes &m) { f.insert(f.end(), m.begin(), m.end()); }
static const Bytes EOF_MEMBER(BGZF_EOF, BGZF_EOF + 28);

static std::string put(const std::string &dir, const char *name, const Bytes &f) {
    const std::string p = dir + "/" + name;
    FILE *o = fopen(p.c_str(), "wb");
    if (!o || (!f.empty() && fwrite(f.data(), 1, f.size(), o) != f.size()) || fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", p.c_str()); exit(2); }
    return p;
}

struct Opened { InputFile in; PassReader rd; };
static void open_case(Opened &o, const std::string &path, size_t piece) {
    if (o.in.open(path.c_str())) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    o.rd.fd = o.in.fd; o.rd.fsz = o.in.fsz; o.rd.T = 2; if (piece) o.rd.piece = piece;
}

static void header_case(const std::string &path, const char *name, Contigs dialect, bool first_name, size_t piece) {
    Opened o; open_case(o, path, piece);
    BamHeader bh; std::vector<std::string> names; std::vector<uint32_t> lens;
    const bool collect = dialect == Contigs::Collect;
    const HeaderRead r = read_bam_header(o.rd, dialect, first_name, bh, collect ? &names : nullptr, collect ? &lens : nullptr);
    printf("header %s %s%s piece=%zu -> ", name, collect ? "collect" : "skip", first_name ? "+name" : "", piece);
    switch (r) {
    case HeaderRead::NotBam: printf("notbam\n"); return;
    case HeaderRead::Ended: printf("ended\n"); return;
    case HeaderRead::Empty: printf("empty\n"); return;
    case HeaderRead::Failed: printf("failed: %s\n", o.rd.msg.c_str()); return;
    case HeaderRead::Complete: break;
    }
    printf("complete %llu %u %zu", (unsigned long long)bh.hdr_end, bh.n_ref, o.rd.n);
    for (size_t k = 0; k < names.size(); k++) printf(" %s/%u", names[k].c_str(), lens[k]);
    printf(" %s\n", first_name_there(o.rd, bh.hdr_end) ? (const char *)o.rd.win.p + bh.hdr_end + 36 : "-");
}

static void members_case(const std::string &path, const char *name, size_t piece) {
    Opened o; open_case(o, path, piece);
    printf("members %s piece=%zu ->", name, piece);
    for (;;) {
        const int g = o.rd.members_next();
        if (g < 0) { printf(" %s\n", o.rd.msg.c_str()); return; }
        if (g == 0) { printf(" end\n"); return; }
        printf(" %zu", o.rd.blocks.size());
    }
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: reader_host_check DIR\n"); return 2; }
    const std::string dir = argv[1];
    // a header of 65 bytes: five times 13
    const Bytes hdr = bam_header_bytes("@HD\tVN:1.6\tSO:coordinate\n", {"chr11", "chr22"}, {200000, 50000});
    if (hdr.size() != 65) { fprintf(stderr, "the header has %zu bytes\n", hdr.size()); return 2; }
    // one record: block_size, the 32 fixed bytes (l_read_name at byte 8), the name "read_one", nothing else
    Bytes rec(4 + 32 + 9, 0);
    { const uint32_t bs = 32 + 9; memcpy(rec.data(), &bs, 4); rec[4 + 8] = 9; memcpy(rec.data() + 36, "read_one", 9); }

    Bytes one; add(one, member(hdr, 0, hdr.size())); add(one, EOF_MEMBER);
    const std::string p_one = put(dir, "one_member", one);

    Bytes five; size_t M = 0;
    for (size_t k = 0; k < 5; k++) { const Bytes m = member(hdr, 13 * k, 13 * (k + 1)); if (k && m.size() != M) { fprintf(stderr, "members of unequal size\n"); return 2; } M = m.size(); add(five, m); }
    add(five, EOF_MEMBER);
    const std::string p_five = put(dir, "five_members", five);

    // the header, then the record cut two bytes into its name: a piece of the first member's size ends there
    Bytes hr = hdr; hr.insert(hr.end(), rec.begin(), rec.end());
    const Bytes first = member(hr, 0, hdr.size() + 38);
    Bytes cut = first; add(cut, member(hr, hdr.size() + 38, hr.size())); add(cut, EOF_MEMBER);
    const std::string p_cut = put(dir, "name_cut", cut);

    Bytes ends; add(ends, member(hdr, 0, hdr.size() - 6)); add(ends, EOF_MEMBER);
    const std::string p_ends = put(dir, "ends_in_header", ends);
    const std::string p_zero = put(dir, "zero_bytes", Bytes());
    Bytes bax = hdr; bax[2] = 'X';
    Bytes magic; add(magic, member(bax, 0, bax.size())); add(magic, EOF_MEMBER);
    const std::string p_magic = put(dir, "wrong_magic", magic);

    printf("sizes member=%zu file=%zu first=%zu\n", M, five.size(), first.size());
    for (Contigs d : {Contigs::Collect, Contigs::Skip}) {
        header_case(p_one, "one_member", d, false, 0);
        header_case(p_five, "five_members", d, false, M);
        header_case(p_five, "five_members", d, false, 2 * M - 1);
        header_case(p_five, "five_members", d, false, 0);
        header_case(p_cut, "name_cut", d, true, first.size());
        header_case(p_cut, "name_cut", d, false, first.size());
        header_case(p_ends, "ends_in_header", d, false, 0);
        header_case(p_zero, "zero_bytes", d, false, 0);
        header_case(p_magic, "wrong_magic", d, false, 0);
        header_case(p_five, "five_members", d, false, M - 1);                           // a member larger than the piece
    }
    members_case(p_five, "five_members", M);
    members_case(p_five, "five_members", 2 * M - 1);
    members_case(p_five, "five_members", 0);
    members_case(p_five, "five_members", M - 1);
    members_case(p_zero, "zero_bytes", 0);
    { Bytes t(five.begin(), five.end() - 10); members_case(put(dir, "cut_in_eof", t), "cut_in_eof", 0); }
    return 0;
}
