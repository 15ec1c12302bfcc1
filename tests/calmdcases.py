"""The records gce_bam_calmd is tested on (tests/test_calmd_model.py, tests/calmd_host_check.hip, tests/test_calmd_gpu.py): a small reference,
vectors whose NM and MD were worked out by hand from it, optional-field layouts with their new bytes spelled out, malformed areas, every cause
of rule E, and records of every size modulo 16.  Nothing here is made with tests/pycalmd.py."""
import struct

CODES = "=ACMGRSVTWYHKDBN"

#        0         10        20        30        40
CHR1 = "ACGTACGTCA" "GGATCCATTG" "ACCAGTNRAC" "TTGACGTAGC" "GGACTGGCAT"
CHR2 = "ACGT" * 75
# the FASTA as a file: a description behind the name, a lower-case line, IUPAC letters (N, R in chr1), a contig the header lacks
FASTA_TEXT = (">chr1 hand vectors\n" + CHR1[:20] + "\n" + CHR1[20:40].lower() + "\n" + CHR1[40:] + "\n"
              ">extra not in the header\nACGTNNACGT\n"
              ">chr2\n" + CHR2[:60].lower() + "\n" + "".join(CHR2[k:k + 60] + "\n" for k in range(60, 300, 60)))
CONTIGS = {"chr1": CHR1.encode(), "extra": b"ACGTNNACGT", "chr2": CHR2.encode()}     # what the loader returns for FASTA_TEXT
TARGETS = [("chr1", len(CHR1)), ("chr2", len(CHR2)), ("missing", 1000)]              # the header: `missing` is not in the FASTA
NAMES = [t[0] for t in TARGETS]

OPS = "MIDNSHP=X"


def cigar_words(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | OPS.index(ch))
            n = ""
    return out


def pack(seq):
    nib = [CODES.index(c) for c in seq] + [0]
    return bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(seq), 2))


def record(tid, pos, cigar, seq, aux=b"", flag=0, qname="r", words=None, qual=None):
    """a raw record, block_size first; words: the CIGAR as numbers where the text cannot say it"""
    name = qname.encode() + b"\0"
    cw = cigar_words(cigar) if words is None else words
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(name), 60, 4680, len(cw), flag, len(seq), -1, -1, 0)
    body = core + name + b"".join(struct.pack("<I", w) for w in cw) + pack(seq) + bytes(qual if qual is not None else [30 + k % 10 for k in range(len(seq))]) + aux
    return struct.pack("<I", len(body)) + body


def hand_vectors():
    """(label, record, NM, MD), NM and MD derived by hand from CHR1"""
    v = [
        ("perfect match", 0, "10M", "ACGTACGTCA", 0, "10"),
        ("mismatch at the first base", 0, "10M", "CCGTACGTCA", 1, "0A9"),
        ("mismatch at the last base", 0, "10M", "ACGTACGTCC", 1, "9A0"),
        ("deletion", 0, "4M2D4M", "ACGTGTCA", 2, "4^AC4"),
        ("insertion", 0, "4M2I4M", "ACGTTTACGT", 2, "8"),
        ("soft clips at both ends", 2, "2S6M2S", "NNGTCCGTNN", 1, "2A3"),
        ("N between two M runs", 0, "3M5N3M", "ACGCAG", 0, "6"),
        ("N between two M runs, mismatch behind it", 0, "3M5N3M", "ACGCAT", 1, "5G0"),
        ("= bases in the read always match", 0, "4M", "=C=T", 0, "4"),
        ("read N against reference N is a mismatch, read R against reference R matches", 24, "4M", "GTNR", 1, "2N1"),
        ("read A against reference R", 24, "4M", "GTNA", 2, "2N0R0"),
        ("mismatch directly after a deletion", 40, "2M2D4M", "GGAGGC", 3, "2^AC0T3"),
        ("over the contig's end inside M", 46, "8M", "GCATAAAA", 0, "4"),
        ("over the contig's end inside M, a mismatch in front of it", 46, "8M", "GCTTAAAA", 1, "2A1"),
        ("over the contig's end inside D", 44, "4M4D2M", "TGGCAA", 2, "4^AT0"),
        ("a D wholly behind the contig's end", 46, "4M2D2M", "GCATAA", 0, "4"),
        ("negative pos", -1, "4M", "ACGT", 0, "0"),
        ("negative pos, a D first", -3, "2D4M", "ACGT", 0, "0"),
        ("= and X operations", 0, "2=1X2=", "ACTTA", 1, "2G2"),
        ("hard clips and padding", 0, "2H2M1P2M2H", "ACGT", 0, "4"),
        ("lower-case line of the FASTA (folded by the loader)", 20, "6M", "ACCTGT", 1, "3A2"),
    ]
    return [(label, record(0, pos, cg, seq, qname="h%d" % k), nm, md) for k, (label, pos, cg, seq, nm, md) in enumerate(v)]


BASE = dict(tid=0, pos=0, cigar="10M", seq="CCGTACGTCA")                              # NM 1, MD 0A9
NEW_NM_MD = b"NMC\x01" + b"MDZ0A9\0"
XA = b"XAZhello\0"
XB = b"XBi" + struct.pack("<i", -7)
XC = b"XCBi" + struct.pack("<Iiii", 3, 1, -2, 3)
XD = b"XDA!"
XF = b"XFf" + struct.pack("<f", 1.5)
XG = b"XGd" + struct.pack("<d", 2.5)
XH = b"XHH1AE3\0"
XS = b"XSBs" + struct.pack("<Ihh", 2, -1, 300)


def nm(typ, val):
    return b"NM" + typ.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ], val)


def md(text):
    return b"MDZ" + text.encode() + b"\0"


def tag_cases():
    """(label, record, the new record's optional fields, nm_changed, md_changed) on a record of NM 1 and MD 0A9"""
    c = [
        ("no optional field at all", b"", b"", 1, 1),
        ("no NM or MD", XA + XB, XA + XB, 1, 1),
        ("only NM", nm("C", 1), b"", 0, 1),
        ("only MD", md("0A9"), b"", 1, 0),
        ("only MD, another string", md("10"), b"", 1, 1),
        ("MD that is a prefix of the new one", md("0A"), b"", 1, 1),
        ("MD that the new one is a prefix of", md("0A90"), b"", 1, 1),
        ("NM as i, same value", nm("i", 1) + md("0A9"), b"", 0, 0),
        ("NM as i, another value", nm("i", 7) + md("0A9"), b"", 1, 0),
        ("NM as c, negative", nm("c", -1), b"", 1, 1),
        ("NM as C, another value", nm("C", 2), b"", 1, 1),
        ("NM as S and I", nm("S", 1) + XA, XA, 0, 1),
        ("NM as a Z field", b"NMZ1\0" + XA, XA, 1, 1),
        ("MD as an integer", b"MDC\x09" + XA, XA, 1, 1),
        ("NM first, MD last", nm("C", 1) + XA + XB + md("0A9"), XA + XB, 0, 0),
        ("NM and MD in the middle", XA + nm("C", 1) + XB + md("0A9") + XC, XA + XB + XC, 0, 0),
        ("MD first, NM last", md("0A9") + XA + XB + nm("C", 1), XA + XB, 0, 0),
        ("NM and MD side by side in the middle", XA + md("0A9") + nm("C", 1) + XB, XA + XB, 0, 0),
        ("NM twice", nm("C", 1) + XA + nm("C", 5), XA, 0, 1),
        ("NM twice, the first one wrong", nm("C", 5) + XA + nm("C", 1), XA, 1, 1),
        ("NM twice and MD twice", XD + nm("C", 1) + XA + md("0A9") + XB + nm("i", 3) + XC + md("7") + XF, XD + XA + XB + XC + XF, 0, 0),
        ("three dropped fields side by side", nm("C", 1) + nm("C", 1) + md("0A9") + XA, XA, 0, 0),
        ("behind a B:i array", XC + nm("C", 1) + md("0A9"), XC, 0, 0),
        ("behind a Z field", XA + md("0A9") + nm("C", 1), XA, 0, 0),
        ("every type", XD + XB + XF + XG + XH + XS + XC + XA + nm("s", 1), XD + XB + XF + XG + XH + XS + XC + XA, 0, 1),
        ("every type but d", XD + XB + XF + XH + XS + XC + XA + nm("s", 1), XD + XB + XF + XH + XS + XC + XA, 0, 1),
        ("an empty B array and an empty Z field", b"XEBC" + struct.pack("<I", 0) + b"XZZ\0" + md("0A9"), b"XEBC" + struct.pack("<I", 0) + b"XZZ\0", 1, 0),
    ]
    out = []
    for k, (label, aux, kept, nmc, mdc) in enumerate(c):
        r = record(aux=aux, qname="t%d" % k, **BASE)
        body = r[4:len(r) - len(aux)] + kept + NEW_NM_MD
        out.append((label, r, struct.pack("<I", len(body)) + body, nmc, mdc))
    return out


def long_cases():
    """(label, record, NM, MD, the type of the new NM field): NM of 256 and of 65 536 from long I runs (the second record is larger than a
    BGZF member), an MD of more than 255 bytes (every base of CHR2[0:130] mismatches: the read holds the next letter)"""
    nxt = {"A": "C", "C": "G", "G": "T", "T": "A"}
    allmis = "".join(nxt[b] for b in CHR2[:130])
    return [
        ("NM 255 stays C", record(0, 0, "5M255I5M", "ACGTA" + "T" * 255 + "CGTCA", aux=nm("C", 255), qname="l0"), 255, "10", "C"),
        ("NM 256 needs S", record(0, 0, "5M256I5M", "ACGTA" + "T" * 256 + "CGTCA", aux=XA, qname="l1"), 256, "10", "S"),
        ("NM 65535 stays S", record(0, 0, "5M65535I5M", "ACGTA" + "G" * 65535 + "CGTCA", qname="l2"), 65535, "10", "S"),
        ("NM 65536 needs I", record(0, 0, "5M65536I5M", "ACGTA" + "G" * 65536 + "CGTCA", aux=md("10") + XB, qname="l3"), 65536, "10", "I"),
        ("MD of 261 bytes", record(1, 0, "130M", allmis, aux=nm("C", 130), qname="l4"), 130, "".join("0" + b for b in CHR2[:130]) + "0", "C"),
    ]


def malformed():
    """(label, record): eligible records whose optional fields do not tile block_size"""
    return [
        ("a Z field without NUL", record(aux=XB + b"XAZhello", qname="m0", **BASE)),
        ("a B count past the end", record(aux=b"XCBi" + struct.pack("<Iii", 3, 1, 2) + b"\0\0\0", qname="m1", **BASE)),
        ("one stray byte", record(aux=XA + b"X", qname="m2", **BASE)),
        ("two stray bytes", record(aux=XA + b"XY", qname="m3", **BASE)),
        ("an unknown type", record(aux=b"XQq\0" + XA, qname="m4", **BASE)),
        ("an unknown B subtype", record(aux=b"XQBd" + struct.pack("<I", 0), qname="m5", **BASE)),
        ("an i field cut by the end", record(aux=nm("C", 1) + b"XBi\1\0", qname="m6", **BASE)),
        ("a B header cut by the end", record(aux=b"XCBi\1\0", qname="m7", **BASE)),
    ]


def ineligible():
    """(label, record, may stand in a BAM file, counts as n_no_ref): one record per cause of rule E, each with a stale NM and MD that stay;
    nobody walks the optional fields of such a record, so a malformed area is no error there (that record stands in no file: the tests read
    every file back with pybam)"""
    stale = nm("C", 9) + md("stale")
    return [
        ("unmapped (flag & 4)", record(0, 0, "10M", "CCGTACGTCA", aux=stale, flag=4, qname="e0"), True, False),
        ("tid -1", record(-1, 0, "10M", "CCGTACGTCA", aux=stale, qname="e1"), True, False),
        ("tid == n_ref", record(len(TARGETS), 0, "10M", "CCGTACGTCA", aux=stale, qname="e2"), False, False),
        ("no CIGAR", record(0, 0, "", "CCGTACGTCA", aux=stale, qname="e3"), True, False),
        ("no bases", record(0, 0, "5H", "", aux=stale, qname="e4"), True, False),
        ("a CIGAR code above 8", record(0, 0, "", "CCGTACGTCA", aux=stale, qname="e5", words=[10 << 4, 1 << 4 | 9]), True, False),
        ("the CIGAR consumes fewer bases than l_seq", record(0, 0, "9M", "CCGTACGTCA", aux=stale, qname="e6"), True, False),
        ("the CIGAR consumes more bases than l_seq", record(0, 0, "4M2I5M", "CCGTACGTCA", aux=stale, qname="e7"), True, False),
        ("the FASTA lacks the contig", record(2, 0, "10M", "CCGTACGTCA", aux=stale, qname="e8"), True, True),
        ("unmapped, its optional fields malformed", record(0, 0, "10M", "CCGTACGTCA", aux=stale + b"X", flag=4, qname="e9"), False, False),
    ]


def alignment_cases():
    """(record, the new record): 16 name lengths against four layouts of the optional fields, so that record sizes and the starts of the
    kept stretches cover every residue modulo 16"""
    layouts = [(b"", b""), (XA + nm("C", 3) + XB, XA + XB), (nm("i", 1) + XC + XD + md("0A9") + XH, XC + XD + XH), (XD + md("1") + XA + nm("C", 1) + XD + XS, XD + XA + XD + XS)]
    out = []
    for nl in range(1, 17):
        for k, (aux, kept) in enumerate(layouts):
            r = record(aux=aux, qname="abcdefghijklmnop"[:nl], **dict(BASE, pos=0))
            body = r[4:len(r) - len(aux)] + kept + NEW_NM_MD
            out.append((r, struct.pack("<I", len(body)) + body))
    return out


def file_records():
    """every record above that may stand in a BAM file, malformed ones apart, in one order (the big records in the middle); the tests read
    the files back with pybam, which knows no `d` field: that record stays with the model and the host check"""
    recs = [r for _, r, _, _ in hand_vectors()] + [r for label, r, _, _, _ in tag_cases() if label != "every type"] + [r for _, r, _, _, _ in long_cases()]
    recs += [r for _, r, in_file, _ in ineligible() if in_file] + [r for r, _ in alignment_cases()]
    return recs


def frames(recs):
    """records behind a 32-bit length each, as tests/calmd_host_check.hip reads them"""
    return b"".join(struct.pack("<I", len(r)) + r for r in recs)


def ref_frames(fasta):
    """the header's contigs for tests/calmd_host_check.hip: n_ref, then per tid a 64-bit length (-1: the FASTA lacks it) and the bases"""
    out = struct.pack("<i", len(NAMES))
    for n in NAMES:
        s = fasta.get(n)
        out += struct.pack("<q", -1) if s is None else struct.pack("<q", len(s)) + s
    return out
