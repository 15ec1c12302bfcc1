"""BAM records for the GPU line writer (gce_samfmt.hpp): hand-built records that no parser produces, records every writer must refuse, and
an independent model of the line a record prints (SAMv1 1.4-1.5 and the rules of samtext::bam_to_line, worked out here and not by the code
under test).  Shared by test_samfmt_model.py (host check, no GPU) and test_samfmt_gpu.py."""
import struct

import pybam
import samcases

TARGETS = samcases.TARGETS
NAMES = [t[0] for t in TARGETS]
CODES = "=ACMGRSVTWYHKDBN"
INT32_MAX = 2147483647


def rec(qname=b"r\0", flag=0, tid=0, pos=99, mapq=60, cigar=None, mtid=-1, mpos=-1, tlen=0, lseq=10, seq=None, qual=None, aux=b"", bin_=4680, l_read_name=None,
        l_seq=None, n_cigar=None, block_size=None):
    """one record from raw parts.  cigar: list of 32-bit words (default lseq M, none for lseq 0); seq: packed bytes; qual: bytes; the three
    overrides put a value into the core block that the bytes behind it do not keep"""
    cigar = ([lseq << 4] if lseq else []) if cigar is None else cigar
    seq = samcases.pack(samcases.bases(lseq)) if seq is None else seq
    qual = bytes((k * 5) % 42 for k in range(lseq)) if qual is None else qual
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(qname) if l_read_name is None else l_read_name, mapq, bin_, len(cigar) if n_cigar is None else n_cigar, flag,
                       lseq if l_seq is None else l_seq, mtid, mpos, tlen)
    body = core + qname + b"".join(struct.pack("<I", w) for w in cigar) + seq + qual + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def fmt_g(x):
    return "%g" % x


def line_of(r, names=NAMES):
    """the SAM line (bytes, line feed included) of one whole record, or None where the writer refuses it"""
    return analyse(r, names)[0]


def holds_float(r):
    """a good record: does the host have to print it (an f, d or B:f value)?"""
    return analyse(r)[1]


def analyse(r, names=NAMES):
    host = [False]
    return _line(r, names, host), host[0]


def _line(r, names, host):
    if len(r) < 4:
        return None
    bs, = struct.unpack_from("<I", r)
    if bs < 32 or 4 + bs > len(r):
        return None
    tid, pos, lq, mapq, _bin, nc, flag, lseq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", r, 4)
    if lq < 1 or lseq < 0 or 32 + lq + 4 * nc + (lseq + 1) // 2 + lseq > bs:
        return None
    end = 4 + bs
    p = 36
    qn = r[p:p + lq].split(b"\0")[0]
    p += lq
    cig = struct.unpack_from("<%dI" % nc, r, p)
    p += 4 * nc
    sq = r[p:p + (lseq + 1) // 2]
    p += (lseq + 1) // 2
    ql = r[p:p + lseq]
    p += lseq

    def name(t):
        return names[t].encode() if 0 <= t < len(names) else b"*"
    f = [qn, b"%d" % flag, name(tid), b"%d" % (pos + 1), b"%d" % mapq, b"".join(b"%d%c" % (w >> 4, ord("MIDNSHP=X???????"[w & 15])) for w in cig) or b"*",
         b"*" if mtid < 0 else b"=" if mtid == tid else name(mtid), b"%d" % (mpos + 1), b"%d" % tlen,
         bytes(ord(CODES[(sq[k >> 1] >> (0 if k & 1 else 4)) & 15]) for k in range(lseq)) or b"*",
         b"*" if lseq == 0 or ql[0] == 0xFF else bytes((q + 33) & 255 for q in ql)]
    ints = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
    while p + 3 <= end:
        tag, t = r[p:p + 2], chr(r[p + 2])
        p += 3
        if t == "A":
            if p + 1 > end:
                return None
            f.append(tag + b":A:" + r[p:p + 1])
            p += 1
        elif t in ints or t in "fd":
            fm = ints.get(t) or {"f": "<f", "d": "<d"}[t]
            n = struct.calcsize(fm)
            if p + n > end:
                return None
            v, = struct.unpack_from(fm, r, p)
            host[0] = host[0] or t in "fd"
            f.append(tag + (b":i:%d" % v if t in ints else (":%s:%s" % (t, fmt_g(v))).encode()))
            p += n
        elif t in "ZH":
            z = r.find(b"\0", p, end)
            if z < 0:
                return None
            f.append(tag + b":" + t.encode() + b":" + r[p:z])
            p = z + 1
        elif t == "B":
            if p + 5 > end:
                return None
            sub = chr(r[p])
            cnt, = struct.unpack_from("<I", r, p + 1)
            fm = ints.get(sub) or ({"f": "<f"}.get(sub))
            if fm is None or p + 5 + struct.calcsize(fm) * cnt > end:
                return None
            vals = struct.unpack_from("<%d%s" % (cnt, fm[1]), r, p + 5)
            host[0] = host[0] or sub == "f"
            f.append(tag + b":B:" + sub.encode() + b"".join(b"," + (fmt_g(v).encode() if sub == "f" else b"%d" % v) for v in vals))
            p += 5 + struct.calcsize(fm) * cnt
        else:
            return None
    return b"\t".join(f) + b"\n"


def hand_built():
    """good records that no parser produces: (label, record bytes)"""
    a = pybam.aux_bytes
    n_ref = len(NAMES)
    c = []
    c.append(("tid and mtid beyond the table, equal", rec(tid=n_ref + 3, mtid=n_ref + 3, mpos=5)))
    c.append(("tid and mtid beyond the table, unequal", rec(tid=n_ref, mtid=n_ref + 1, mpos=5)))
    c.append(("tid in the table, mtid beyond it", rec(tid=1, mtid=n_ref, mpos=5)))
    c.append(("tid beyond the table, mtid in it", rec(tid=n_ref + 7, mtid=2, mpos=5)))
    c.append(("mtid == tid == -1", rec(tid=-1, mtid=-1, pos=-1, flag=4)))
    c.append(("mtid -2", rec(tid=-2, mtid=-2)))
    c.append(("pos and mpos INT32_MAX", rec(pos=INT32_MAX, mtid=0, mpos=INT32_MAX, tlen=-2147483648)))
    c.append(("pos -1", rec(pos=-1, mpos=-1, tlen=INT32_MAX)))
    c.append(("pos INT32_MIN", rec(pos=-2147483648, mpos=-2147483648)))
    c.append(("cigar ops 9 and 15", rec(cigar=[(3 << 4) | 9, (7 << 4) | 15, (0xFFFFFFF << 4) | 8, 0])))
    c.append(("n_cigar 0", rec(cigar=[])))
    for n in (0, 1, 2, 15, 16, 17, 31, 32, 33, 255):
        c.append(("l_seq %d" % n, rec(qname=b"s%d\0" % n, lseq=n, seq=bytes((k * 37 + 11) & 255 for k in range((n + 1) // 2)))))
    c.append(("qual starts 0xFF", rec(lseq=37, qual=b"\xff" + bytes(range(36)))))
    c.append(("qual all 0xFF", rec(lseq=33, qual=b"\xff" * 33)))
    c.append(("qual bytes 223..255 not in front", rec(lseq=34, qual=b"\x00" + bytes(range(223, 256)))))
    c.append(("qual bytes 94..222", rec(lseq=129, qual=bytes(range(94, 223)))))
    c.append(("qname with an embedded NUL", rec(qname=b"ab\0cd\0")))
    c.append(("qname that starts with NUL", rec(qname=b"\0abc")))
    c.append(("qname without any NUL", rec(qname=b"nonul")))
    c.append(("qname of 255 bytes without NUL", rec(qname=b"Q" * 255)))
    ext = [("c", -128), ("c", 127), ("C", 0), ("C", 255), ("s", -32768), ("s", 32767), ("S", 0), ("S", 65535), ("i", -2147483648), ("i", INT32_MAX), ("I", 0), ("I", 4294967295)]
    c.append(("every integer type at both extremes", rec(aux=b"".join(a("X%s" % chr(65 + k), t, v) for k, (t, v) in enumerate(ext)))))
    bx = {"c": [-128, 127], "C": [0, 255], "s": [-32768, 32767], "S": [0, 65535], "i": [-2147483648, INT32_MAX], "I": [0, 4294967295]}
    for sub, (lo, hi) in bx.items():
        for cnt in (0, 1, 17):
            c.append(("B:%s of %d" % (sub, cnt), rec(aux=a("B" + sub, "B", (sub, [(lo, hi, 7)[k % 3] for k in range(cnt)])) + a("NM", "C", 3))))
    for cnt in (0, 1, 17):
        c.append(("B:f of %d" % cnt, rec(aux=a("Bf", "B", ("f", [(0.1, -2.5e10, 7.0)[k % 3] for k in range(cnt)])) + a("XZ", "Z", "behind"))))
    c.append(("f and d", rec(aux=b"XFf" + struct.pack("<f", 3.14159) + b"XDd" + struct.pack("<d", -1e-300) + a("NM", "C", 0))))
    c.append(("f of special values", rec(aux=b"".join(b"F%df" % k + struct.pack("<f", v) for k, v in enumerate((0.0, -0.0, 1e38, 1e-45, 100000.0, 1000000.0, 0.0001, 0.00001))))))
    c.append(("A with a tab byte", rec(aux=b"XAA\t" + a("NM", "C", 1))))
    c.append(("A with a NUL and a line feed", rec(aux=b"XAA\0XBA\n")))
    c.append(("Z with bytes above 127 and a tab", rec(aux=b"XZZa\tb\x80\xff\0" + b"XHH\0")))
    c.append(("one stray byte behind the last tag", rec(aux=a("NM", "C", 1) + b"X")))
    c.append(("two stray bytes behind the last tag", rec(aux=a("NM", "C", 1) + b"XY")))
    c.append(("two stray bytes and no tag", rec(aux=b"\0\0")))
    c.append(("a tag of bytes that are no letters", rec(aux=b"\t\nC\x07")))
    return c


def bad_records():
    """records every writer must refuse: (label, the bytes that are there).  Each is made from known-good bytes with one thing wrong."""
    a = pybam.aux_bytes
    good = rec()
    c = []
    c.append(("block_size 31", struct.pack("<I", 31) + good[4:4 + 31]))
    c.append(("l_read_name 0", rec(l_read_name=0)))
    c.append(("l_seq < 0", rec(l_seq=-1)))
    c.append(("l_seq overruns block_size", rec(l_seq=4000)))
    c.append(("l_seq INT32_MAX", rec(l_seq=INT32_MAX)))
    c.append(("n_cigar overruns block_size", rec(n_cigar=65535)))
    c.append(("l_read_name overruns block_size", rec(qname=b"r\0", lseq=0, cigar=[], seq=b"", qual=b"", l_read_name=255)))
    c.append(("block_size cuts the qualities", rec(block_size=len(good) - 4 - 1)))
    c.append(("Z without NUL", rec(aux=b"XZZabc")))
    c.append(("H without NUL behind a good tag", rec(aux=a("NM", "C", 1) + b"XHH1A")))
    c.append(("type Q", rec(aux=b"XQQ\1")))
    c.append(("type NUL", rec(aux=b"XQ\0\1")))
    c.append(("B:q", rec(aux=b"XBBq" + struct.pack("<I", 1) + b"\0" * 8)))
    c.append(("B:d", rec(aux=b"XBBd" + struct.pack("<I", 1) + b"\0" * 8)))
    c.append(("B whose count overruns", rec(aux=b"XBBs" + struct.pack("<I", 3) + b"\0" * 5)))
    c.append(("B with a count of 2^32 - 1", rec(aux=b"XBBC" + struct.pack("<I", 0xFFFFFFFF) + b"\0" * 9)))
    c.append(("B:f whose count overruns", rec(aux=b"XBBf" + struct.pack("<I", 2) + b"\0" * 7)))
    c.append(("B cut inside its count", rec(aux=b"XBBc\1\0\0")))
    c.append(("a 4-byte value cut at 3", rec(aux=b"XIi\1\2\3")))
    c.append(("an f cut at 3", rec(aux=b"XFf\1\2\3")))
    c.append(("a d cut at 7", rec(aux=a("NM", "C", 1) + b"XDd" + b"\0" * 7)))
    c.append(("an s cut at 1", rec(aux=b"XSs\1")))
    c.append(("an A without its byte", rec(aux=b"XAA")))
    c.append(("a float in front of a bad tag", rec(aux=b"XFf" + struct.pack("<f", 1.5) + b"XQQ\1")))
    return c


def cut_records():
    """frames shorter than their block_size says (the end of the buffer cuts the record): bad for a walk and for the size pass"""
    good = rec(aux=pybam.aux_bytes("XZ", "Z", "tail"))
    return [("the buffer ends inside block_size", good[:3]), ("the buffer ends behind block_size", good[:4]), ("the buffer ends inside the core", good[:20]),
            ("the buffer ends one byte early", good[:-1])]


def frames(records):
    return b"".join(struct.pack("<I", len(r)) + r for r in records)
