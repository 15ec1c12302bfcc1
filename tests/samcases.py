"""SAM text cases for the GPU line parser (gce_samdev.hpp): field edges with the bytes pybam's independent model gives them, and one malformed
line per message of samtext::line_to_bam.  Shared by test_sort_sam_model.py (host check, no GPU) and test_samdev_gpu.py."""
import struct

import pybam

TARGETS = [("chr1", 1000000), ("chr2", 500000), ("chrM", 16569), ("chr10", 300000)]
NT16 = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN")}
NT16.update({c.lower(): k for c, k in list(NT16.items()) if c != "="})


def pack(seq):
    out = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        out[i // 2] |= NT16.get(ch, 15) << (4 if i % 2 == 0 else 0)
    return bytes(out)


def bases(n, alphabet="ACGT"):
    return "".join(alphabet[(i * 7 + i // 3) % len(alphabet)] for i in range(n))


def quals(n):
    return "".join(chr(33 + (i * 5) % 42) for i in range(n))


def case(qname="r", flag=0, rname="chr1", pos=100, mapq=60, cigar=None, rnext="*", pnext=0, tlen=0, seq=None, qual=None, aux=(), n=10):
    """-> (line, expected record bytes, needs the host).  aux: (text, bytes, float?) per optional field; the expectation follows SAMv1 and
    the two htslib conventions of gce_samtext.hpp, worked out here and not by the code under test."""
    seq = bases(n) if seq is None else seq
    ls = 0 if seq == "*" else len(seq)
    qual = (quals(ls) if ls else "*") if qual is None else qual
    cigar = ("%dM" % ls if ls else "*") if cigar is None else cigar
    names = [t[0] for t in TARGETS]
    tid = names.index(rname) if rname in names else -1
    if pos == 0:
        tid = -1
    if tid < 0:
        flag_out = flag | 4
    else:
        flag_out = flag
    mtid = tid if rnext == "=" else (names.index(rnext) if rnext in names else -1)
    if cigar == "*":
        flag_out |= 4
    words = pybam.parse_cigar(cigar)
    span = 1 if flag_out & 4 else (pybam.cigar_ref_len(words) or 1)
    bin_ = pybam.reg2bin(pos - 1, pos - 1 + span)
    nm = qname.encode() + b"\0"
    q = b"\xff" * ls if qual == "*" else bytes(ord(c) - 33 for c in qual)
    body = struct.pack("<iiBBHHHiiii", tid, pos - 1, len(nm), mapq, bin_, len(words), flag_out, ls, mtid, pnext - 1, tlen)
    body += nm + b"".join(struct.pack("<I", w) for w in words) + (pack(seq) if ls else b"") + q + b"".join(a[1] for a in aux)
    line = "\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual] + [a[0] for a in aux])
    return line, struct.pack("<i", len(body)) + body, any(a[2] for a in aux)


def itag(tag, text, typ, val):
    return ("%s:i:%s" % (tag, text), pybam.aux_bytes(tag, typ, val), False)


INT_TAGS = [("-2147483648", "i", -2147483648), ("-32769", "i", -32769), ("-32768", "s", -32768), ("-129", "s", -129), ("-128", "c", -128), ("-1", "c", -1),
            ("-0", "c", 0), ("0", "C", 0), ("+5", "C", 5), ("255", "C", 255), ("256", "S", 256), ("65535", "S", 65535), ("65536", "I", 65536), ("4294967295", "I", 4294967295)]


def field_edge_cases():
    c = []
    c.append(case(qname="q"))
    c.append(case(qname="Q" * 254))
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 151, 5000):
        c.append(case(qname="len%d" % n, n=n, pos=1000 + n))
    c.append(case(qname="noseq", seq="*", qual="*", cigar="*"))
    c.append(case(qname="noqual", n=37, qual="*"))
    c.append(case(qname="iupac", seq="acgtnACGTNMRSVWYHKDB=mrsvwyhkdb.x@", n=0, cigar="34M"))
    c.append(case(qname="nocigar", n=20, cigar="*", flag=0))
    c.append(case(qname="everyop", seq=bases(1 + 2 + 5 + 8 + 9), cigar="5S1M2I3D4N6H7P8=9X", pos=5000))
    c.append(case(qname="oneop", n=1, cigar="1M"))
    c.append(case(qname="ops300", seq=bases(300), cigar="1M1I" * 150, pos=777))
    c.append(case(qname="pos0", pos=0, rnext="=", pnext=5, flag=1))
    c.append(case(qname="unknown", rname="chrUn", rnext="=", flag=16))
    c.append(case(qname="other", rname="chr2", rnext="chr10", pnext=99, tlen=-2147483647, flag=65535, mapq=255))
    c.append(case(qname="prefix", rname="chr1", rnext="chr", pnext=2147483647, tlen=2147483647, pos=2147483647))
    c.append(case(qname="star", rname="*", pos=0, rnext="*"))
    c.append(case(qname="ints", aux=[itag("X%s" % chr(65 + k), t, ty, v) for k, (t, ty, v) in enumerate(INT_TAGS)]))
    c.append(case(qname="others", aux=[("XA:A:!", pybam.aux_bytes("XA", "A", b"!"), False), ("XZ:Z:", pybam.aux_bytes("XZ", "Z", ""), False),
                                       ("YZ:Z:a b:c", pybam.aux_bytes("YZ", "Z", "a b:c"), False), ("XH:H:1AE3", pybam.aux_bytes("XH", "H", "1AE3"), False)]))
    bvals = {"c": [-128, 127, -0], "C": [0, 255], "s": [-32768, 32767], "S": [65535, 0, 1], "i": [-2147483648, 2147483647], "I": [4294967295, 0]}
    c.append(case(qname="barrays", aux=[("B%s:B:%s" % (s, s) + "".join(",%d" % v for v in vs), pybam.aux_bytes("B" + s, "B", (s, vs)), False) for s, vs in bvals.items()]
                  + [("BE:B:c", pybam.aux_bytes("BE", "B", ("c", [])), False), ("BP:B:C,+7", pybam.aux_bytes("BP", "B", ("C", [7])), False)]))
    c.append(case(qname="float_f", aux=[("XF:f:3.14159", b"XFf" + struct.pack("<f", 3.14159), True), ("NM:i:2", pybam.aux_bytes("NM", "C", 2), False)]))
    c.append(case(qname="float_d", aux=[("XD:d:-1e-300", b"XDd" + struct.pack("<d", -1e-300), True)]))
    c.append(case(qname="float_b", n=33, aux=[("XB:B:f,0.1,-2.5e10,7", pybam.aux_bytes("XB", "B", ("f", [0.1, -2.5e10, 7.0])), True), ("XZ:Z:behind", pybam.aux_bytes("XZ", "Z", "behind"), False)]))
    c.append(case(qname="fields11"))
    return c


def n_float_lines(cases):
    return sum(1 for k in cases if k[2])


def text_of(cases, newline="\n", last_newline=True):
    t = newline.join(k[0] for k in cases)
    return (t + newline if last_newline else t).encode()


GOOD = "g\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tFFFF"


def malformed_cases():
    """(message of samtext::line_to_bam, a line that earns it and no earlier one), one per message"""
    def ln(**kw):
        f = GOOD.split("\t")
        for k, v in kw.items():
            f[int(k[1:])] = v
        return "\t".join(f)
    return [
        ("SAM line with fewer than 11 fields", "\t".join(GOOD.split("\t")[:10])),
        ("SAM line with a bad numeric field", ln(f3="12x")),
        ("SAM line with a bad QNAME", ln(f0="N" * 255)),
        ("CIGAR length out of range", ln(f5="268435456M")),
        ("malformed CIGAR", ln(f5="4")),
        ("unknown CIGAR operation", ln(f5="4Q")),
        ("more than 65535 CIGAR operations", ln(f5="1M" * 65536, f9="*", f10="*")),
        ("CIGAR and query sequence are of different length", ln(f5="5M")),
        ("SEQ and QUAL of different length", ln(f10="FFF")),
        ("malformed optional field", GOOD + "\tNM:i"),
        ("malformed A field", GOOD + "\tXA:A:ab"),
        ("integer field out of range", GOOD + "\tNM:i:4294967296"),
        ("malformed B field", GOOD + "\tXB:B:"),
        ("unknown B subtype", GOOD + "\tXB:B:d,1"),
        ("malformed B value", GOOD + "\tXB:B:c,1,,2"),
        ("B value out of its type's range", GOOD + "\tXB:B:c,128"),
        ("unknown optional field type", GOOD + "\tXQ:q:1"),
    ]


def more_bad_lines():
    """further lines every check must refuse (no message pinned to them here: the host check compares the two parsers on each)"""
    return [GOOD.replace("\t60\t", "\t256\t"), GOOD.replace("g\t0", "g\t65536"), GOOD.replace("g\t0", "g\t-1"), GOOD.replace("\t100\t", "\t2147483648\t"),
            "\t" + GOOD.split("\t", 1)[1], GOOD.replace("\t100\t", "\t\t"), GOOD.replace("\t100\t", "\t+\t"), GOOD.replace("4M", "4M\0"), GOOD.replace("4M", "M"),
            GOOD + "\tNM:i:-2147483649", GOOD + "\tNM:i:", GOOD + "\tNM:i:1099511627777", GOOD + "\tXB:B:c1,2", GOOD + "\tXB:B:S,-1", GOOD + "\tXB:B:\0,1", GOOD + "\t\tNM:i:1",
            GOOD + "\tXA:A:", GOOD + "\tN:i:1"]


def more_good_lines():
    """lines both parsers must accept with the same bytes although no writer prints them (no independent model: host check only)"""
    return [GOOD + "\t", GOOD.replace("\t100\t", "\t+100\t"), GOOD + "\tXB:B:cX1,2", GOOD + "\tXB:B:i,-5", GOOD + "\tNM:i:7\t", GOOD.replace("4M", "2M2X").replace("\t0\t0\t", "\t0\t-5\t"),
            GOOD.replace("\t*\t0", "\tchr1\t0"), GOOD.replace("chr1", "chr1 "), GOOD.replace("ACGT\tFFFF", "ACGT\t!~!~"), GOOD + "\tXZ:Z:\x80\xff"]
