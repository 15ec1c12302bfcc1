"""The output side of the file runners (gencore_amd/csrc/gce_fileout.hpp) without a GPU: the piece pump over a fake device, the output-file
object and the two text conversions, in a program of their own (tests/fileout_host_check.cpp) built with the address and undefined-behaviour
sanitizers.  Its lines are compared with the models below: the pump's fetches, waits and sink sizes follow from the piece arithmetic alone;
the lines of a record come from pybam.sam_line, the records of a line from samcases' expectations."""
import os
import shutil
import struct
import subprocess
import zlib

import pybam
import samcases
import samfmtcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = (8, 4096)
THREADS_R2L = (1, 3, 8, 100)
THREADS_L2R = (1, 3, 8)


def totals(p):
    return (0, 1, p - 1, p, p + 1, 3 * p, 3 * p + 1)


def prefixes(p):
    return (0, 1, p - 1, p, p + 1, 2 * p + 3)


def pump_line(piece, total, prefix):
    """the walk of prefix + total bytes in pieces: a fetch (and its wait) per piece that holds stream bytes, a sink per piece"""
    whole = prefix + total
    sizes = [min(whole, a + piece) - a for a in range(0, whole, piece)]
    fetched = sum(1 for a in range(0, whole, piece) if min(whole, a + piece) > prefix)
    return "pump %d %d %d ok fetches=%d waits=%d sinks=%s" % (piece, total, prefix, fetched, fetched, ",".join(map(str, sizes)))


def test_pump_model():
    assert pump_line(8, 0, 0) == "pump 8 0 0 ok fetches=0 waits=0 sinks="
    assert pump_line(8, 0, 19) == "pump 8 0 19 ok fetches=0 waits=0 sinks=8,8,3"                 # a prefix alone: nothing is fetched
    assert pump_line(8, 1, 16) == "pump 8 1 16 ok fetches=1 waits=1 sinks=8,8,1"                 # the prefix ends at a piece border
    assert pump_line(8, 25, 19) == "pump 8 25 19 ok fetches=4 waits=4 sinks=8,8,8,8,8,4"         # the prefix spans two pieces and ends inside the third


def pybam_records():
    """a few dozen records pybam can express, with their lines"""
    rs = []
    for k in range(37):
        n = (1, 2, 15, 16, 17, 31, 32, 33, 151)[k % 9]
        rs.append(dict(qname="p%d" % k, flag=99 if k & 1 else 147, tid=k % 4, pos=1000 * k, mapq=k, cigar="%dM" % n, mtid=(k + (k % 3 == 0)) % 4, mpos=1000 * k + 50, isize=(-1) ** k * 200,
                       seq=samcases.bases(n, "ACGTN"), qual=samcases.quals(n), nm=k, mi="UMI%d" % k, aux_pre=[("XS", "s", -300 - k), ("XA", "A", b"!")],
                       aux_post=[("XI", "I", 4000000000 + k), ("BC", "B", ("S", [k, 65535, 0]))]))
    rs.append(dict(qname="unmapped", flag=4, tid=-1, pos=-1, cigar="*", mtid=-1, mpos=-1, isize=0, seq="", qual=[]))
    rs.append(dict(qname="noqual", flag=0, tid=0, pos=5, cigar="3M", mtid=-1, mpos=-1, isize=0, seq="ACG", qual=[0xFF] * 3))
    recs = [pybam.record_bytes(r) for r in rs]
    lines = [pybam.sam_line(r, samfmtcases.TARGETS).encode("latin-1") + b"\n" for r in rs]
    return recs, lines


def crc(b):
    return "%08x:%d" % (zlib.crc32(b) & 0xFFFFFFFF, len(b))


def test_host_check_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        cxx = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path / "fileout_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fileout_host_check.cpp"), "-o", exe, "-lz", "-lpthread"])
    d = tmp_path / "cases"
    d.mkdir()
    man, want = [], []
    # ---- the pump
    for p in PIECES:
        for t in totals(p):
            for h in prefixes(p):
                man.append("pump %d %d %d" % (p, t, h)); want.append(pump_line(p, t, h))
        last = 3                                                                   # 3 * p + 1 bytes: pieces 0 .. 3
        for who in ("fetch", "wait", "sink"):
            for j in (0, 1, last):
                man.append("fail %s %d %d %d 0" % (who, j, p, 3 * p + 1)); want.append("fail %s %d %d %d 0 status=-77 later=0" % (who, j, p, 3 * p + 1))
    # ---- records -> lines
    (d / "names").write_text("\n".join(nm for nm, _ in samfmtcases.TARGETS) + "\n")
    recs, lines = pybam_records()
    assert len(recs) >= 36
    short = struct.pack("<I", 31) + bytes(31)                                      # block_size below 32, the records behind it in step
    (d / "recs").write_bytes(b"".join(recs))
    (d / "none").write_bytes(b"")
    (d / "short").write_bytes(b"".join(recs[:5]) + short + b"".join(recs[5:]))
    (d / "cut").write_bytes(b"".join(recs)[:-7])
    for T in THREADS_R2L:
        assert T != 100 or T > len(recs)
        man.append("r2l recs %d" % T); want.append("r2l recs %d lines=%s whole=%d:%d" % (T, crc(b"".join(lines)), len(b"".join(recs)), len(recs)))
        man.append("r2l none %d" % T); want.append("r2l none %d lines=%s whole=0:0" % (T, crc(b"")))
        man.append("r2l short %d" % T); want.append("r2l short %d lines=bad whole=bad" % T)
    man.append("r2l cut 1")                                                        # (the walk of whole_records stops in front of the record the end cuts)
    want.append("r2l cut 1 lines=%s whole=%d:%d" % (crc(b"".join(lines[:-1])), len(b"".join(recs[:-1])), len(recs) - 1))
    # ---- lines -> records
    cases = samcases.field_edge_cases()
    body = b"".join(c[1] for c in cases)
    bad = samcases.malformed_cases()
    texts = {
        "good": (samcases.text_of(cases), body),
        "crlf": (samcases.text_of(cases, newline="\r\n"), body),
        "blank": (samcases.text_of(cases[:7]) + b"\n\r\n" + samcases.text_of(cases[7:]) + b"\n", body),      # an empty line, a lone \r, an empty last line
        "nothing": (b"", b""),
    }
    for name, (text, recs_of) in sorted(texts.items()):
        (d / name).write_bytes(text)
        for T in THREADS_L2R:
            for mode in ("nl", "cut"):
                man.append("l2r %s %d %s" % (name, T, mode)); want.append("l2r %s %d %s ok:%s:left=0" % (name, T, mode, crc(recs_of)))
    (d / "open_end").write_bytes(samcases.text_of(cases, last_newline=False))      # the last line without its line feed
    for T in THREADS_L2R:
        man.append("l2r open_end %d nl" % T); want.append("l2r open_end %d nl ok:%s:left=0" % (T, crc(body)))
        man.append("l2r open_end %d cut" % T)                                       # (a piece that is not the last: the open line is left for the next)
        want.append("l2r open_end %d cut ok:%s:left=%d" % (T, crc(b"".join(c[1] for c in cases[:-1])), len(cases[-1][0].encode())))
    assert bad[1][0] != bad[8][0]
    (d / "bad_middle").write_bytes(samcases.text_of(cases[:9]) + bad[8][1].encode() + b"\n" + samcases.text_of(cases[9:20]) + bad[1][1].encode() + b"\n" + samcases.text_of(cases[20:]))
    for T in THREADS_L2R:
        man.append("l2r bad_middle %d nl" % T); want.append("l2r bad_middle %d nl err:%s" % (T, bad[8][0]))
    man.append("outfile"); want.append("outfile ok")
    (d / "manifest").write_text("\n".join(man) + "\n")
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    got = r.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w, (g[:300], w[:300])
    assert r.returncode == 0 and len(got) == len(want), (r.returncode, len(got), len(want), r.stderr[-4000:])
