"""The host's shared BGZF / BAM-header pieces (gencore_amd/csrc/gce_bgzf.hpp) without a GPU: the member scanner, the header parser in its
two dialects and the member codec, in a program of their own (tests/bgzf_host_check.cpp) built with the address and undefined-behaviour
sanitizers, against the models below.  The models restate the order of checks every file runner applied before the pieces were shared,
so each damaged file keeps its message; the case files come from the pure-Python writers (pybam, recordstreams)."""
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import deflatecraft
import pybam
import recordstreams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------ members
def member(data, front=b"", sub=None, bsize=None, isize=None):
    """a BGZF member; front: extra subfields in front of BC; sub: the bytes that stand where the BC subfield should; bsize: the BSIZE field's
    value; isize: the ISIZE field's value"""
    comp = zlib.compress(data, 6)[2:-4]
    total = 12 + len(front) + 6 + len(comp) + 8
    bc = sub if sub is not None else b"BC\x02\x00" + struct.pack("<H", total - 1 if bsize is None else bsize)
    assert len(bc) == 6
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(front) + 6) + front + bc + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) if isize is None else isize))


ORDINARY = pybam.bgzf_block(b"an ordinary member " * 3)
FRONT = member(b"a subfield in front of BC", front=b"XY\x03\x00abc")
GOOD = ORDINARY + FRONT + pybam.bgzf_block(b"") + pybam.EOF_BLOCK

NOT_BGZF, BAD, BAD_ISIZE = "not a BGZF file", "bad BGZF block", "bad BGZF block (ISIZE above 64 KB)"
# the damaged member stands second: (file, the message of the whole file)
DAMAGED = {
    "magic": (ORDINARY + b"\x1e" + FRONT[1:] + pybam.EOF_BLOCK, NOT_BGZF),
    "flag": (ORDINARY + FRONT[:3] + b"\x00" + FRONT[4:] + pybam.EOF_BLOCK, NOT_BGZF),
    "no_bc": (ORDINARY + member(b"no BC subfield", sub=b"XY\x02\x00\x30\x00") + pybam.EOF_BLOCK, BAD),
    "subfield_past_xlen": (ORDINARY + member(b"a subfield that runs past XLEN", sub=b"BC\x04\x00\x30\x00") + pybam.EOF_BLOCK, BAD),
    "small_bsize": (ORDINARY + member(b"BSIZE below header plus trailer", bsize=20) + pybam.EOF_BLOCK, BAD),
    "isize": (ORDINARY + member(b"ISIZE above 64 KB", isize=0x10001) + pybam.EOF_BLOCK, BAD_ISIZE),
}


def scan_model(buf, off):
    """one member at buf[off:]: (bsize, isize), "more" or the message -- the streaming runners' order of checks"""
    have = len(buf)
    if off + 18 > have:
        return "more"
    if buf[off] != 0x1f or buf[off + 1] != 0x8b or buf[off + 2] != 8 or not buf[off + 3] & 4:
        return NOT_BGZF
    xlen = struct.unpack_from("<H", buf, off + 10)[0]
    if off + 12 + xlen > have:
        return "more"
    bsize, x = None, 0
    while x + 4 <= xlen:
        s = off + 12 + x
        sl = struct.unpack_from("<H", buf, s + 2)[0]
        if x + 4 + sl > xlen:
            break
        if buf[s:s + 2] == b"BC" and sl == 2:
            bsize = struct.unpack_from("<H", buf, s + 4)[0] + 1
        x += 4 + sl
    if bsize is None or bsize < 12 + xlen + 8:
        return BAD
    if off + bsize > have:
        return "more"
    isize = struct.unpack_from("<I", buf, off + bsize - 4)[0]
    return BAD_ISIZE if isize > 0x10000 else (bsize, isize)


def scan_line(name, blob):
    out = []
    for L in range(len(blob) + 1):
        off = n = 0
        while isinstance(r := scan_model(blob[:L], off), tuple):
            off += r[0]; n += 1
        out.append("%d,%d,%s" % (L, n, r))
    return "scan %s %s" % (name, ";".join(out))


def test_scanner_model_on_the_good_file():
    """every prefix yields the members wholly inside it (recordstreams' walker), then "more", never an error"""
    mem = recordstreams.bgzf_members(GOOD)
    assert [(c, u) for _, c, u in mem] == [(len(ORDINARY), 57), (len(FRONT), 25), (28, 0), (28, 0)] and sum(c for _, c, _ in mem) == len(GOOD)
    toks = scan_line("good", GOOD).split(" ", 2)[2].split(";")
    assert len(toks) == len(GOOD) + 1
    for L, t in enumerate(toks):
        assert t == "%d,%d,more" % (L, sum(1 for o, c, _ in mem if o + c <= L))


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_scanner_model_on_damaged_files(name):
    blob, msg = DAMAGED[name]
    toks = scan_line(name, blob).split(" ", 2)[2].split(";")
    assert toks[-1] == "%d,1,%s" % (len(blob), msg)
    assert all(t.endswith(",more") for t in toks[:len(ORDINARY) + 18])            # (nothing is judged before 18 bytes of the member are there)


# ------------------------------------------------------------------------------------------------------------------------ headers
def header(targets, text="@HD\tVN:1.6\n", magic=b"BAM\1", l_text=None, n_ref=None):
    out = magic + struct.pack("<I", len(text) if l_text is None else l_text) + text.encode() + struct.pack("<I", len(targets) if n_ref is None else n_ref)
    for nm, ln in targets:
        out += struct.pack("<I", len(nm) + 1 if nm is not None else 0) + (nm.encode() + b"\0" if nm is not None else b"") + struct.pack("<I", ln)
    return out


T3 = [("chr1", 1000), ("c", 7), ("a_longer_name", 123456789)]
TAIL = b"\x07\x00\x00\x00rec"                                                      # (bytes behind the header: hdr_end does not move)
HEADERS = {
    "contigs0": header([]) + TAIL,
    "contigs1": header(T3[:1]) + TAIL,
    "contigs3": header(T3) + TAIL,
    "magic": header(T3[:1], magic=b"BAM\2") + TAIL,
    "zero_name": header([("chr1", 1000), (None, 55), ("z", 9)]) + TAIL,
    "huge_n_ref": header([], n_ref=0x7FFFFFFF),
    "huge_n_ref_with_a_contig": header(T3[:1], n_ref=0x7FFFFFFF) + TAIL,
    "l_text_beyond": header(T3[:1], l_text=1000) + TAIL,
}


def hdr_model(u, collect):
    """"notbam", "incomplete" or (text_off, l_text, n_ref, hdr_end, [(name, length)]); collect: names kept, a zero-length name incomplete;
    otherwise the table is stepped over, a zero-length name accepted and n_ref bounded below 2^31"""
    n = len(u)
    if n >= 4 and u[:4] != b"BAM\1":
        return "notbam"
    if n < 12:
        return "incomplete"
    l_text = struct.unpack_from("<I", u, 4)[0]
    p = 8
    if p + l_text + 4 > n:
        return "incomplete"
    p += l_text
    n_ref = struct.unpack_from("<I", u, p)[0]; p += 4
    if not collect and n_ref >= 0x7FFFFFFF:
        return "incomplete"
    tg = []
    for _ in range(n_ref):
        if p + 4 > n:
            return "incomplete"
        ln = struct.unpack_from("<I", u, p)[0]; p += 4
        if (collect and ln == 0) or p + ln + 4 > n:
            return "incomplete"
        tg.append((u[p:p + ln - 1].decode() if ln else "", struct.unpack_from("<I", u, p + ln)[0]))
        p += ln + 4
    return (8, l_text, n_ref, p, tg)


def hdr_line(name, blob, collect):
    out = []
    for L in range(len(blob) + 1):
        r = hdr_model(blob[:L], collect)
        if isinstance(r, tuple):
            r = "complete:%d:%d:%d:%d" % r[:4] + ("".join(":%s/%d" % t for t in r[4]) if collect else "")
        out.append("%d=%s" % (L, r))
    return "hdr %s %s %s" % (name, "collect" if collect else "skip", ";".join(out))


def last(line):
    return line.rsplit(";", 1)[1].split("=", 1)[1]


def test_header_model():
    for k, name in ((0, "contigs0"), (1, "contigs1"), (3, "contigs3")):
        blob = HEADERS[name]; end = len(blob) - len(TAIL)
        for collect in (True, False):
            toks = hdr_line(name, blob, collect).split(" ", 3)[3].split(";")
            assert all(t == "%d=incomplete" % L for L, t in enumerate(toks[:end]))
            want = "complete:8:11:%d:%d" % (k, end) + ("".join(":%s/%d" % t for t in T3[:k]) if collect else "")
            assert all(t == "%d=%s" % (end + i, want) for i, t in enumerate(toks[end:]))
    for collect in (True, False):
        toks = hdr_line("magic", HEADERS["magic"], collect).split(" ", 3)[3].split(";")
        assert toks[:4] == ["%d=incomplete" % L for L in range(4)] and all(t.endswith("=notbam") for t in toks[4:])
        assert last(hdr_line("l_text_beyond", HEADERS["l_text_beyond"], collect)) == "incomplete"
        assert last(hdr_line("huge_n_ref", HEADERS["huge_n_ref"], collect)) == "incomplete"
        assert last(hdr_line("huge_n_ref_with_a_contig", HEADERS["huge_n_ref_with_a_contig"], collect)) == "incomplete"
    # the two dialects part on a zero-length name: never complete where the names are collected, stepped over where they are not
    z = HEADERS["zero_name"]
    assert last(hdr_line("zero_name", z, True)) == "incomplete"
    assert last(hdr_line("zero_name", z, False)) == "complete:8:11:3:%d" % (len(z) - len(TAIL))


# ------------------------------------------------------------------------------------------------------------------------ codec
def codec_data(n):
    """n compressible bytes: a short alphabet with runs (a member of 0x10000 such bytes fits its 64 KB)"""
    out, x = bytearray(), 12345
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out += bytes([65 + (x >> 16) % 7]) * (1 + (x >> 8) % 9)
    return bytes(out[:n])


CODEC_SIZES = (0, 1, 0xff00, 0x10000)
CODEC_LEVELS = (-1, 1, 6)


# the valid members whose code sets are incomplete: the table decoder takes complete sets alone and hands these to zlib by design
ZLIBS_BUSINESS = ("single_dist_len1", "no_dist_literal_only", "only_eob_len1", "hclen5")          # (hclen5: no distance code either)


# ------------------------------------------------------------------------------------------------------------------------ the program
def test_host_check_under_sanitizers(tmp_path):
    """bgzf_host_check.cpp (scan_member, parse_bam_header, deflate_block / inflate_block of gce_bgzf.hpp; every input in a heap block of its
    exact size) built with -fsanitize=address,undefined: its lines are the models' lines, the members it deflates are gzip's.  The
    hand-built members of deflatecraft go through inflate_block twice, once with the table decoder in front of zlib and once with zlib
    alone (GCE_BAM_ZLIB_ONLY): the valid ones come out with the catalogue's bytes, the others are refused, both times.  The table decoder
    is also called on its own: it delivers every valid member's bytes itself, but for the four whose code sets are incomplete, and
    refuses every invalid one."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        cxx = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path / "bgzf_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "bgzf_host_check.cpp"), "-o", exe, "-lz"])
    d = tmp_path / "cases"
    d.mkdir()
    man, want = [], []
    for name, blob in [("good", GOOD)] + [(k, v[0]) for k, v in sorted(DAMAGED.items())]:
        (d / name).write_bytes(blob); man.append("scan " + name); want.append(scan_line(name, blob))
    for name, blob in sorted(HEADERS.items()):
        (d / ("h_" + name)).write_bytes(blob); man.append("hdr h_" + name)
        want += [hdr_line("h_" + name, blob, True), hdr_line("h_" + name, blob, False)]
    for n in CODEC_SIZES:
        (d / ("d%d" % n)).write_bytes(codec_data(n))
        for lv in CODEC_LEVELS:
            man.append("codec d%d %d" % (n, lv)); want.append("codec d%d %d ok" % (n, lv))
    for name, m, usize, expected in deflatecraft.cases():
        (d / ("c_" + name)).write_bytes(m); man.append("inflate c_%s %d" % (name, usize))
        verdict = "refused" if expected is None else "ok:%08x" % (zlib.crc32(expected) & 0xFFFFFFFF)
        want.append("inflate c_%s %s raw:%s" % (name, verdict, "refused" if name in ZLIBS_BUSINESS else verdict))
    want += ["eof ok", "header_bytes ok"]
    (d / "manifest").write_text("\n".join(man) + "\n")
    for zlib_only in (False, True):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        env.pop("GCE_BAM_ZLIB_ONLY", None)
        if zlib_only:
            env["GCE_BAM_ZLIB_ONLY"] = "1"
        r = subprocess.run(["timeout", "-k", "10", "300", exe, str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
        assert r.returncode == 0, (zlib_only, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        got = r.stdout.splitlines()
        assert len(got) == len(want), zlib_only
        for g, w in zip(got, want):
            assert g == w, (zlib_only, g[:300], w[:300])
    for n in CODEC_SIZES:
        for lv in CODEC_LEVELS:
            z = (d / ("d%d.%d.gz" % (n, lv))).read_bytes()
            assert gzip.decompress(z) == codec_data(n) and recordstreams.bgzf_members(z) == [(0, len(z), n)]
