"""Hand-written records for gce_bam_error_profile_support: every case names its premise and lists, written out by hand, every
counter that is not zero and every skip counter.  The model (tests/pyerrsup.py), the per-record functions on the host
(tests/errsup_host_check.hip) and the kernels, on chip and with direct atomics (tests/test_errsup_gpu.py), are all held against these numbers.

A case: errprofcases' dict plus mask = None or [(contig name, start, end)], tags, and expect = [(segment, forward bucket, reverse bucket, class
name, count)].  The header and the FASTA are errprofcases':   c0:  0 ACGTACGTAC  10 acgtNRYKMn  20 GGGGGCCCCC  30 TTTTTAAAAA   c1: ACGT x 12, AC
Unless a case says otherwise its records are 2M over c0:0 showing AC: one A>A, one C>C and one RECORDS each."""
import struct

import errprofcases as ec
from errprofcases import FASTA, LENS, NAMES, rec  # noqa: F401

FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f", "A": "<c"}


def num(tag, typ, v):
    return tag.encode() + typ.encode() + struct.pack(FMT[typ], v)


def text(tag, s, typ="Z"):
    return tag.encode() + typ.encode() + s.encode() + b"\0"


def array(tag, sub, vals):
    return tag.encode() + b"B" + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(FMT[sub], v) for v in vals)


def ac(aux=b"", flag=0, **kw):
    return rec(0, 0, "2M", "AC", flag=flag, aux=aux, **kw)


def row(g, f, r, n=1, **more):
    """n records of the usual kind in row (g, f, r)"""
    out = [(g, f, r, "RECORDS", n), (g, f, r, "A>A", n), (g, f, r, "C>C", n)]
    return out + [(g, f, r, cl, v) for cl, v in more.items()]


def case(label, premise, records, expect, skips=None, bed=None, mask=None, tags=("FR", "RR"), **kw):
    c = ec.case(label, premise, records, expect, skips=skips, bed=bed, **kw)
    c["skips"].setdefault("n_bad_aux", 0)
    c["mask"], c["tags"] = mask, tags
    return c


def all_cases():
    c = []
    # ---- rule U: types, values, presence
    c.append(case("each_integer_type", "FR = 3 as c, C, s, S, i and I: six records in row forward 3, reverse absent", [ac(num("FR", t, 3)) for t in "cCsSiI"], row(0, 3, 0, 6)))
    c.append(case("values", "FR -1 (c), 0 (C), 32 (C), 255 (C), 65535 (S), -1 (s), -1 (i) and 4000000000 (I) all fall in the top bucket; 1 and 31 are their own",
                  [ac(num("FR", "c", -1)), ac(num("FR", "C", 0)), ac(num("FR", "C", 32)), ac(num("FR", "C", 255)), ac(num("FR", "S", 65535)), ac(num("FR", "s", -1)), ac(num("FR", "i", -1)),
                   ac(num("FR", "I", 4000000000)), ac(num("FR", "C", 1)), ac(num("FR", "C", 31))], row(0, 32, 0, 8) + row(0, 1, 0) + row(0, 31, 0)))
    c.append(case("zero_is_the_top_bucket", "FR:C:0 with RR:S:300: the low byte of 256 reads, and a count past 31", [ac(num("FR", "C", 0) + num("RR", "S", 300))], row(0, 32, 32)))
    c.append(case("presence", "FR alone, RR alone, both, neither", [ac(num("FR", "C", 2)), ac(num("RR", "C", 4)), ac(num("FR", "C", 2) + num("RR", "C", 4)), ac()],
                  row(0, 2, 0) + row(0, 0, 4) + row(0, 2, 4) + row(0, 0, 0)))
    c.append(case("other_types_are_absent", "FR:Z:3, FR:A:3 and FR:f:3 are absent; so is RR:B:C,3", [ac(text("FR", "3")), ac(num("FR", "A", b"3")), ac(num("FR", "f", 3.0)), ac(array("RR", "C", [3]))],
                  row(0, 0, 0, 4)))
    c.append(case("first_field_wins", "FR:C:2 then FR:C:5: 2.  FR:Z:x then FR:C:5: the first is of the wrong type, absent.  RR likewise behind them",
                  [ac(num("FR", "C", 2) + num("FR", "C", 5) + num("RR", "C", 1) + num("RR", "C", 9)), ac(text("FR", "x") + num("FR", "C", 5) + text("RR", "y", "H") + num("RR", "i", 7))],
                  row(0, 2, 1) + row(0, 0, 0)))
    c.append(case("between_z_h_and_b", "the tags in front of, between and behind MD:Z, XH:H and XB:B fields of every element size",
                  [ac(num("FR", "C", 2) + text("MD", "10A5") + text("XH", "1AE3", "H") + num("RR", "C", 3) + array("XB", "S", [1, 2, 3])),
                   ac(text("MD", "") + array("XB", "c", []) + num("FR", "s", 4) + array("XC", "i", [-5, 7]) + num("RR", "I", 5) + text("XH", "", "H")),
                   ac(array("XB", "f", [1.5]) + text("XH", "00", "H") + text("RG", "grp") + num("NM", "C", 0) + num("XD", "f", 2.0) + num("FR", "i", 6) + num("RR", "S", 7))],
                  row(0, 2, 3) + row(0, 4, 5) + row(0, 6, 7)))
    c.append(case("no_optional_fields", "an empty optional area: both absent", [ac()], row(0, 0, 0)))
    c.append(case("custom_tags", "tags aD,bD: fgbio's duplex depths; the FR of the same record is not read", [ac(num("FR", "C", 9) + num("aD", "C", 4) + num("bD", "s", 2))], row(0, 4, 2),
                  tags=("aD", "bD")))
    c.append(case("tags_are_case_sensitive", "fr:C:2 and Fr:C:2 are not FR", [ac(num("fr", "C", 2) + num("Fr", "C", 2) + num("RR", "C", 2))], row(0, 0, 2)))
    # ---- the row: segment, strand
    c.append(case("segments_and_strands", "0x40 is segment 1, 0x90 segment 2 on the reverse strand (AC over AC complemented: T>T and G>G), 0xC0 segment 0",
                  [ac(num("FR", "C", 2) + num("RR", "C", 1), flag=0x40), ac(num("FR", "C", 2) + num("RR", "C", 1), flag=0x90), ac(num("FR", "C", 2) + num("RR", "C", 1), flag=0xC0)],
                  row(1, 2, 1) + [(2, 2, 1, "RECORDS", 1), (2, 2, 1, "T>T", 1), (2, 2, 1, "G>G", 1)] + row(0, 2, 1)))
    c.append(case("every_class_in_one_row", "1M1I1M1D2M at c0:12 showing GAAAC with qualities 30 30 5 30 30 under min_baseq 10: G>G, INS, LOWQ, DEL at 14, A over R and C over Y are REF_OTHER; "
                  "N over c0:1's C in another record is READ_N, T over it C>T",
                  [rec(0, 12, "1M1I1M1D2M", "GAAAC", [30, 30, 5, 30, 30], aux=num("FR", "C", 3)), rec(0, 1, "1M", "N", aux=num("FR", "C", 3)), rec(0, 1, "1M", "T", aux=num("FR", "C", 3))],
                  [(0, 3, 0, "RECORDS", 3), (0, 3, 0, "G>G", 1), (0, 3, 0, "INS", 1), (0, 3, 0, "LOWQ", 1), (0, 3, 0, "DEL", 1), (0, 3, 0, "REF_OTHER", 2), (0, 3, 0, "READ_N", 1),
                   (0, 3, 0, "C>T", 1)], min_baseq=10))
    # ---- rule E's ninth skip
    c.append(case("bad_aux", "a Z without its NUL, an unknown type, a B with an unknown subtype, an i with two bytes left, two trailing bytes: five records in n_bad_aux, none "
                  "counted, although FR was read in front of the fault; a whole record beside them is counted",
                  [ac(num("FR", "C", 2) + b"MDZ10A"), ac(num("FR", "C", 2) + b"XQQ\1"), ac(num("FR", "C", 2) + b"XBBx" + struct.pack("<I", 0)), ac(num("FR", "C", 2) + b"XIi\1\2"),
                   ac(num("FR", "C", 2) + b"XY"), ac(num("FR", "C", 2))], row(0, 2, 0), dict(n_bad_aux=5)))
    c.append(case("bad_aux_more", "a B whose count passes the block, a B with fewer than five bytes, an H without its NUL, one trailing byte, a d with four bytes",
                  [ac(array("XB", "S", [1, 2])[:-1]), ac(b"XBBc\1\0"), ac(b"XHH1A"), ac(num("RR", "C", 1) + b"X"), ac(b"XDd\0\0\0\0"), ac(b"XDd" + bytes(8) + num("RR", "C", 1))], row(0, 0, 1),
                  dict(n_bad_aux=5)))
    c.append(case("bad_aux_comes_last", "a flagged record, one on the contig without reference and one of 1025 bases, each with a broken optional area, go to the earlier counter",
                  [ac(b"XY", flag=0x400), rec(2, 0, "2M", "AC", aux=b"XY"), rec(1, 0, "1025M", aux=b"XY"), ac(b"XY", mapq=3)], [],
                  dict(n_flagged=1, n_no_ref=1, n_too_long=1, n_low_mapq=1), min_mapq=10))
    # ---- rule B and RECORDS; rule Y
    c.append(case("bed_and_records", "the targets are c0:2 and 3.  4M at 0 adds its two target columns; 2M at 4 touches the widened span alone: RECORDS and nothing else, a row of the "
                  "table all the same; 2M at 20 is eligible and not kept; 2M at 5 is not kept either",
                  [rec(0, 0, "4M", "ACGT", aux=num("FR", "C", 3)), rec(0, 4, "2M", "AC", aux=num("FR", "C", 5)), rec(0, 20, "2M", "GG", aux=num("FR", "C", 7)),
                   rec(0, 5, "2M", "CG", aux=num("FR", "C", 8))],
                  [(0, 3, 0, "RECORDS", 1), (0, 3, 0, "G>G", 1), (0, 3, 0, "T>T", 1), (0, 5, 0, "RECORDS", 1)], bed=[("c0", 2, 4)]))
    c.append(case("masked", "c0:1 is masked: the C of every record goes to MASKED in the record's own row",
                  [ac(num("FR", "C", 2) + num("RR", "C", 2)), ac(num("FR", "C", 1)), ac(num("FR", "C", 1))],
                  [(0, 2, 2, "RECORDS", 1), (0, 2, 2, "A>A", 1), (0, 2, 2, "MASKED", 1), (0, 1, 0, "RECORDS", 2), (0, 1, 0, "A>A", 2), (0, 1, 0, "MASKED", 2)], mask=[("c0", 1, 2)]))
    return c


def expected(cs):
    """the case's expect list as {(segment, forward, reverse, class name): count}"""
    out = {}
    for g, f, r, cl, n in cs["expect"]:
        out[g, f, r, cl] = out.get((g, f, r, cl), 0) + n
    return out


def mask_of(cs, names=NAMES):
    return None if cs["mask"] is None else [(names.index(nm), a, z) for nm, a, z in cs["mask"]]


def add_aux(r, aux):
    """the record r with the optional fields aux appended: block_size grows by their bytes"""
    return struct.pack("<I", struct.unpack_from("<I", r, 0)[0] + len(aux)) + r[4:] + aux


def random_aux(rng):
    """optional fields as a consensus writer leaves them, and stranger ones: FR in most records, RR in about a third, now and then twice, of a
    type that is not an integer's, past 31 or 0, between NM, MD, RG and B fields"""
    parts = [num("NM", "C", int(rng.randint(0, 5)))] * int(rng.randint(0, 2)) + [text("MD", "%d" % rng.randint(1, 200))] * int(rng.randint(0, 2))
    if rng.rand() < 0.85:
        parts.append(num("FR", "CcSsIi"[int(rng.randint(0, 6))], int(rng.choice([1, 1, 2, 2, 3, 4, 5, 9, 31, 32, 0, 100]))))
    if rng.rand() < 0.1:
        parts.append(text("FR", "7"))
    if rng.rand() < 0.35:
        parts.append(num("RR", "CS"[int(rng.randint(0, 2))], int(rng.choice([1, 1, 2, 3, 6, 31, 40]))))
    if rng.rand() < 0.1:
        parts.append(num("RR", "C", 9))
    if rng.rand() < 0.2:
        parts.append(array("XB", "cSif"[int(rng.randint(0, 4))], [1] * int(rng.randint(0, 4))))
    order = rng.permutation(len(parts))
    return b"".join(parts[i] for i in order)


def with_tags(records, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    return [add_aux(r, random_aux(rng)) for r in records]


def random_records(seed, n=120):
    """reads over c1 and the FASTA's part of c0 with M, I, D, N and S ops on both strands and in all segments, every anchor inside [0, header
    length), with random_aux's optional fields"""
    import numpy as np
    rng = np.random.RandomState(seed)
    recs = []
    for k in range(n):
        tid = int(rng.randint(0, 2))
        ops = [(4, 2)] * int(rng.randint(0, 2)) + [(int(rng.choice([0, 1, 2])), int(rng.randint(1, 4))) for _ in range(int(rng.randint(0, 2)))]
        for _ in range(int(rng.randint(1, 4))):
            ops += [(0, int(rng.randint(1, 7))), (int(rng.choice([1, 2, 3])), int(rng.randint(1, 4)))]
        ops.append((0, int(rng.randint(1, 5))))
        span = sum(ln for op, ln in ops if op in (0, 2, 3))
        pos = int(rng.randint(1, (45 if tid else 42) - min(span, 40)))
        nq = sum(ln for op, ln in ops if op in (0, 1, 4))
        recs.append(rec(tid, pos, ops, "".join("ACGTN"[i] for i in rng.randint(0, 5, nq)), rng.randint(0, 41, nq).tolist(), flag=int(rng.choice([0, 16, 0x40, 0x90, 0x400])),
                        mapq=int(rng.randint(0, 61)), aux=random_aux(rng)))
    return recs


def raw_records(path):
    """a BAM file -> (contig names, contig lengths, the records as bytes, block_size first), read with Python's gzip"""
    import gzip
    with gzip.open(str(path), "rb") as f:
        data = f.read()
    assert data[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, p)
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, p)
        names.append(data[p + 4:p + 4 + l_name - 1].decode())
        lens.append(struct.unpack_from("<I", data, p + 4 + l_name)[0])
        p += 8 + l_name
    recs = []
    while p < len(data):
        (bs,) = struct.unpack_from("<I", data, p)
        recs.append(data[p:p + 4 + bs])
        p += 4 + bs
    return names, lens, recs


def duplex_stream(n_mol=40, seed=13):
    """a small duplex stream as tests/pybam.py's record dicts, every record eligible: molecules of 1 to 5 pairs of 20M reads on c0 = ACGT x
    500, two-token UMIs behind the prefix UMI, A_B on the forward strand of the molecule (flags 99 / 147) and B_A on the other (163 / 83),
    a base changed now and then -> (records in coordinate order, the reference's bases)"""
    import random
    rng = random.Random(seed)
    ref = "ACGT" * 500
    recs = []
    for m in range(n_mol):
        left = 100 + 41 * m
        right = left + 60 + rng.randrange(20)
        ua, ub = ("".join(rng.choice("ACGT") for _ in range(4)) for _ in range(2))
        for dpl in range(1 + rng.randrange(5)):
            strand = rng.randrange(2)
            name = "m%02d_%d:UMI_%s" % (m, dpl, ua + "_" + ub if strand == 0 else ub + "_" + ua)
            isz = right + 20 - left
            seqs = []
            for a in (left, right):
                s = list(ref[a:a + 20])
                if rng.random() < 0.3:
                    k = rng.randrange(20)
                    s[k] = "ACGT"[("ACGT".index(s[k]) + 1) % 4]
                seqs.append("".join(s))
            nm = [sum(x != y for x, y in zip(s, ref[a:a + 20])) for s, a in zip(seqs, (left, right))]
            f1, f2 = (99, 147) if strand == 0 else (163, 83)
            recs.append(dict(qname=name, flag=f1, tid=0, pos=left, cigar="20M", mtid=0, mpos=right, isize=isz, seq=seqs[0], qual=[rng.choice([37, 25]) for _ in range(20)], nm=nm[0]))
            recs.append(dict(qname=name, flag=f2, tid=0, pos=right, cigar="20M", mtid=0, mpos=left, isize=-isz, seq=seqs[1], qual=[rng.choice([37, 25]) for _ in range(20)], nm=nm[1]))
    recs.sort(key=lambda r: r["pos"])
    return recs, ref
