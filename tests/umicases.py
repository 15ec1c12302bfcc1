"""The records gce_bam_umi_to_mi is tested on (tests/test_umi_model.py, tests/umi_host_check.hip, tests/test_umi_gpu.py): every case names its
source, the record and the record the pass must make of it, both spelled out field by field and built with pybam.record_bytes (which places
aux_pre, NM, MI, aux_post in that order).  Nothing here is made with tests/pyumi.py."""
import functools
import struct

import pybam

TARGETS = [("chr1", 2000), ("chr2", 500)]
XA = ("XA", "Z", "hello")
XI = ("XI", "i", -7)
XB = ("XB", "B", ("s", [1, -2, 300]))
XH = ("XH", "H", "1AE3")


def rec(qname="r", aux_pre=(), nm=1, mi=None, aux_post=(), flag=99, tid=0, pos=100, cigar="10M", seq="ACGTACGTAC", mtid=0, mpos=300, isize=210):
    return pybam.record_bytes(dict(qname=qname, flag=flag, tid=tid, pos=pos, cigar=cigar, mtid=mtid, mpos=mpos, isize=isize, seq=seq, qual=[30 + k % 10 for k in range(len(seq))],
                                   nm=nm, mi=mi, aux_pre=list(aux_pre), aux_post=list(aux_post)))


def RX(v, typ="Z"):
    return ("RX", typ, v)


def MI(v):
    return ("MI", "Z", v)


def cases():
    """(label, source, record, expected record, kind, mi_dropped); kind: tagged / no_source / not_umi.  An untouched record is expected as it is."""
    out = []

    def tagged(label, source, r, want, dropped=False):
        out.append((label, source, r, want, "tagged", dropped))

    def same(label, source, r, kind):
        out.append((label, source, r, r, kind, False))

    # ---- where RX stands among the fields
    tagged("RX first", "RX", rec(aux_pre=[RX("ACGT"), XA, XI]), rec(aux_pre=[RX("ACGT"), XA, XI], mi=":ACGT"))
    tagged("RX in the middle", "RX", rec(aux_pre=[XA, RX("ACGT"), XI]), rec(aux_pre=[XA, RX("ACGT"), XI], mi=":ACGT"))
    tagged("RX last", "RX", rec(aux_post=[XA, RX("ACGT")]), rec(aux_post=[XA, RX("ACGT"), MI(":ACGT")]))
    tagged("RX the only field", "RX", rec(nm=None, aux_pre=[RX("TTGACA")]), rec(nm=None, aux_pre=[RX("TTGACA")], mi=":TTGACA"))
    tagged("a B array in front of RX", "RX", rec(aux_pre=[XB, RX("ACGT")]), rec(aux_pre=[XB, RX("ACGT")], mi=":ACGT"))
    tagged("an H field and a B array around RX", "RX", rec(aux_pre=[XH, RX("GG-CC")], aux_post=[XB]), rec(aux_pre=[XH, RX("GG-CC")], aux_post=[XB, MI(":GG_CC")]))
    # ---- RX that is no source
    same("RX of type A", "RX", rec(aux_pre=[RX(b"C", "A")]), "no_source")
    same("RX of type H", "RX", rec(aux_pre=[RX("ACCA", "H")]), "no_source")
    same("RX of type B", "RX", rec(aux_pre=[RX(("C", [65, 67]), "B")]), "no_source")
    same("RX of type i", "RX", rec(aux_pre=[RX(7, "i")]), "no_source")
    same("no RX", "RX", rec(aux_pre=[XA]), "no_source")
    same("no RX, its own MI stays", "RX", rec(aux_pre=[XA], mi="ACG_TTT"), "no_source")
    same("an empty RX", "RX", rec(aux_pre=[RX("")]), "no_source")
    same("an empty RX, its own MI stays", "RX", rec(aux_pre=[RX("")], mi=":AAA"), "no_source")
    same("no optional fields at all", "RX", rec(nm=None), "no_source")
    same("Rx and rX are other tags", "RX", rec(aux_pre=[("Rx", "Z", "ACGT"), ("rX", "Z", "ACGT")]), "no_source")
    tagged("two RX fields: the first wins", "RX", rec(aux_pre=[RX("AAAA"), RX("CCCC")]), rec(aux_pre=[RX("AAAA"), RX("CCCC")], mi=":AAAA"))
    same("two RX fields: the first, of type A, wins", "RX", rec(aux_pre=[RX(b"G", "A"), RX("CCCC")]), "no_source")
    same("two RX fields: the first, empty, wins", "RX", rec(aux_pre=[RX(""), RX("CCCC")]), "no_source")
    tagged("another tag as source", "BC", rec(aux_pre=[RX("AAAA"), ("BC", "Z", "ccgg")]), rec(aux_pre=[RX("AAAA"), ("BC", "Z", "ccgg")], mi=":CCGG"))
    tagged("a tag with a digit", "U2", rec(aux_pre=[("U2", "Z", "ACG")]), rec(aux_pre=[("U2", "Z", "ACG")], mi=":ACG"))
    # ---- rule V and norm
    tagged("lower case", "RX", rec(aux_pre=[RX("acgtn")]), rec(aux_pre=[RX("acgtn")], mi=":ACGTN"))
    tagged("mixed case", "RX", rec(aux_pre=[RX("AcGt-tTgA")]), rec(aux_pre=[RX("AcGt-tTgA")], mi=":ACGT_TTGA"))
    tagged("N is passed on", "RX", rec(aux_pre=[RX("ACNT")]), rec(aux_pre=[RX("ACNT")], mi=":ACNT"))
    tagged("separator -", "RX", rec(aux_pre=[RX("ACGT-TTGA")]), rec(aux_pre=[RX("ACGT-TTGA")], mi=":ACGT_TTGA"))
    tagged("separator +", "RX", rec(aux_pre=[RX("ACGT+TTGA")]), rec(aux_pre=[RX("ACGT+TTGA")], mi=":ACGT_TTGA"))
    tagged("separator _", "RX", rec(aux_pre=[RX("ACGT_TTGA")]), rec(aux_pre=[RX("ACGT_TTGA")], mi=":ACGT_TTGA"))
    tagged("one base either side", "RX", rec(aux_pre=[RX("A-C")]), rec(aux_pre=[RX("A-C")], mi=":A_C"))
    tagged("a single base", "RX", rec(aux_pre=[RX("G")]), rec(aux_pre=[RX("G")], mi=":G"))
    same("a separator first", "RX", rec(aux_pre=[RX("-ACGT")]), "not_umi")
    same("a separator last", "RX", rec(aux_pre=[RX("ACGT+")]), "not_umi")
    same("a separator alone", "RX", rec(aux_pre=[RX("_")]), "not_umi")
    same("two separators", "RX", rec(aux_pre=[RX("AC-GT-TT")]), "not_umi")
    same("two separators of two kinds", "RX", rec(aux_pre=[RX("AC-GT+TT")]), "not_umi")
    same("another letter", "RX", rec(aux_pre=[RX("ACGU")]), "not_umi")
    same("a digit", "RX", rec(aux_pre=[RX("ACG7")]), "not_umi")
    same("a colon", "RX", rec(aux_pre=[RX("AC:GT")]), "not_umi")
    same("a blank", "RX", rec(aux_pre=[RX("ACGT ")]), "not_umi")
    same("bytes next to the letters in ASCII", "RX", rec(aux_pre=[RX("@B`[{")]), "not_umi")
    same("not a UMI, its own MI stays", "RX", rec(aux_pre=[RX("ACGX")], mi=":ACG"), "not_umi")
    tagged("250 bytes", "RX", rec(aux_pre=[RX("ACGTA" * 50)]), rec(aux_pre=[RX("ACGTA" * 50)], mi=":" + "ACGTA" * 50))
    tagged("250 bytes with a separator", "RX", rec(aux_pre=[RX("a" * 124 + "+" + "c" * 125)]), rec(aux_pre=[RX("a" * 124 + "+" + "c" * 125)], mi=":" + "A" * 124 + "_" + "C" * 125))
    same("251 bytes", "RX", rec(aux_pre=[RX("ACGTA" * 50 + "C")]), "not_umi")
    same("1000 bytes", "RX", rec(aux_pre=[RX("ACGT" * 250)]), "not_umi")
    # ---- MI fields the record has
    tagged("one MI:Z behind RX", "RX", rec(aux_pre=[RX("AC-GT")], mi="old:TTTT"), rec(aux_pre=[RX("AC-GT")], mi=":AC_GT"), True)
    tagged("one MI:Z in front of RX", "RX", rec(aux_pre=[MI("zzz"), RX("AC-GT"), XA]), rec(aux_pre=[RX("AC-GT"), XA], mi=":AC_GT"), True)
    tagged("one MI:i", "RX", rec(aux_pre=[("MI", "i", 123456), RX("ACGT")]), rec(aux_pre=[RX("ACGT")], mi=":ACGT"), True)
    tagged("MI:Z first and MI:C last", "RX", rec(aux_pre=[MI("q"), RX("ACGT")], aux_post=[XI, ("MI", "C", 9)]), rec(aux_pre=[RX("ACGT")], aux_post=[XI, MI(":ACGT")]), True)
    tagged("MI:B between kept fields", "RX", rec(aux_pre=[XA, ("MI", "B", ("i", [5, 6])), RX("ACGT")], aux_post=[XH]), rec(aux_pre=[XA, RX("ACGT")], aux_post=[XH, MI(":ACGT")]), True)
    tagged("three MI fields (the many path)", "RX", rec(aux_pre=[MI("a"), XA, ("MI", "i", 4), RX("ACGT-AAAA"), ("MI", "A", b"x"), XI], aux_post=[XB]),
           rec(aux_pre=[XA, RX("ACGT-AAAA")], nm=None, aux_post=[XI, ("NM", "C", 1), XB, MI(":ACGT_AAAA")]), True)
    tagged("four MI fields, adjacent and last", "RX", rec(aux_pre=[RX("TT"), MI("a"), MI("b")], mi="c", aux_post=[MI("d")]), rec(aux_pre=[RX("TT")], mi=":TT"), True)
    tagged("only MI fields beside RX", "RX", rec(nm=None, aux_pre=[MI("a"), RX("CC")], aux_post=[MI("b")]), rec(nm=None, aux_pre=[RX("CC")], mi=":CC"), True)
    tagged("the MI already there in the form written", "RX", rec(aux_pre=[RX("AC-GT")], mi=":AC_GT"), rec(aux_pre=[RX("AC-GT")], mi=":AC_GT"), True)
    # ---- records of other shapes
    tagged("an unmapped record", "RX", rec(flag=77, tid=-1, pos=-1, cigar="*", mtid=-1, mpos=-1, isize=0, nm=None, aux_pre=[RX("ACGT-TTGA")]),
           rec(flag=77, tid=-1, pos=-1, cigar="*", mtid=-1, mpos=-1, isize=0, nm=None, aux_pre=[RX("ACGT-TTGA")], mi=":ACGT_TTGA"))
    tagged("l_seq = 0", "RX", rec(seq="", cigar="*", aux_pre=[RX("ACGT")]), rec(seq="", cigar="*", aux_pre=[RX("ACGT")], mi=":ACGT"))
    tagged("l_seq odd", "RX", rec(seq="ACGTACG", cigar="7M", aux_pre=[RX("ACGT")]), rec(seq="ACGTACG", cigar="7M", aux_pre=[RX("ACGT")], mi=":ACGT"))
    tagged("a long CIGAR", "RX", rec(seq="ACGTACGTAC", cigar="1S2M1I2M1D2M2S", aux_pre=[RX("ACGT")]), rec(seq="ACGTACGTAC", cigar="1S2M1I2M1D2M2S", aux_pre=[RX("ACGT")], mi=":ACGT"))
    # ---- the read name as the source
    ill = "M01:23:000-AB:1:1101:15589:1332"
    tagged("an Illumina name", "name", rec(qname=ill + ":ACGT+TTGA"), rec(qname=ill + ":ACGT+TTGA", mi=":ACGT_TTGA"))
    tagged("an Illumina name, one index", "name", rec(qname=ill + ":acgtac"), rec(qname=ill + ":acgtac", mi=":ACGTAC"))
    tagged("a name with RX beside it", "name", rec(qname="q:GG+TT", aux_pre=[RX("AAAA")]), rec(qname="q:GG+TT", aux_pre=[RX("AAAA")], mi=":GG_TT"))
    tagged("a name, its MI replaced", "name", rec(qname="q:GG+TT", mi="q:CCCC"), rec(qname="q:GG+TT", mi=":GG_TT"), True)
    tagged("a name that is only a colon and a UMI", "name", rec(qname=":ACGT"), rec(qname=":ACGT", mi=":ACGT"))
    same("a name with no colon", "name", rec(qname="ACGT+TTGA"), "no_source")
    same("a name with a trailing colon", "name", rec(qname=ill + ":"), "no_source")
    same("a name that is a colon", "name", rec(qname=":"), "no_source")
    same("a name whose last field is a number", "name", rec(qname=ill), "not_umi")
    same("a name with fastp's prefix", "name", rec(qname="q:UMI_ACGT"), "not_umi")
    same("a name with two separators", "name", rec(qname="q:AC+GT+TT"), "not_umi")
    n254 = "x" * 244 + ":ACGT+TTGA"
    assert len(n254) == 254
    tagged("a name of 254 bytes", "name", rec(qname=n254), rec(qname=n254, mi=":ACGT_TTGA"))
    tagged("a name of 254 bytes, 250 of them the UMI", "name", rec(qname="ab::" + "T" * 250), rec(qname="ab::" + "T" * 250, mi=":" + "T" * 250))
    same("a name whose last field has 251 bytes", "name", rec(qname="ab:" + "T" * 251), "not_umi")
    tagged("a NUL inside l_read_name: the name is q:ACGT, what follows is not looked at", "name", rec(qname="q:ACGT\0:TT!T"), rec(qname="q:ACGT\0:TT!T", mi=":ACGT"))
    same("a NUL first in the name", "name", rec(qname="\0:ACGT"), "no_source")
    return out


def alignment_cases():
    """names of 1..16 bytes in front of RX: records, and new records, of every size modulo 16"""
    out = []
    for k in range(1, 17):
        q = "n" * k
        out.append(("name of %d bytes" % k, "RX", rec(qname=q, aux_pre=[RX("ACG-TT"), XA], mi="x"), rec(qname=q, aux_pre=[RX("ACG-TT"), XA], mi=":ACG_TT"), "tagged", True))
    return out


def all_cases():
    return cases() + alignment_cases()


def with_aux(r, aux):
    """the raw record r with the bytes `aux` behind its last field, block_size following"""
    body = r[4:] + aux
    return struct.pack("<I", len(body)) + body


def malformed():
    """(label, record): the optional fields do not tile block_size"""
    good = rec(aux_pre=[RX("ACGT"), XA])
    return [
        ("fields that stop one byte short of block_size", with_aux(good, b"X")),
        ("fields that stop two bytes short of block_size", with_aux(good, b"XY")),
        ("a Z value without a NUL", with_aux(good, b"XZZabc")),
        ("the source's own Z value without a NUL", with_aux(rec(aux_pre=[XA]), b"RXZACGT")),
        ("an unknown type byte", with_aux(good, b"XQ?x")),
        ("a B array of an unknown subtype", with_aux(good, b"XBBd" + struct.pack("<I", 1) + b"\0" * 8)),
        ("a B array whose count passes block_size", with_aux(good, b"XBBi" + struct.pack("<I", 3) + b"\0" * 8)),
        ("a B header cut", with_aux(good, b"XBBi\1\0")),
        ("an integer cut", with_aux(good, b"XIi\1\0")),
        ("malformed without a source all the same", with_aux(rec(aux_pre=[XA]), b"X")),
        ("malformed behind a value that is not a UMI", with_aux(rec(aux_pre=[RX("ACGU")]), b"XQ?x")),
    ]


@functools.lru_cache(maxsize=None)
def big_record(n_bytes=70000, umi="ACGTAC-TTGACA"):
    """a record with a B:C field of n_bytes values (that do not compress), a dropped MI of 3000 bytes in front of it and one behind it, RX
    last; and what it becomes"""
    import random
    rng = random.Random(5)
    arr = ("XL", "B", ("C", [rng.randrange(256) for _ in range(n_bytes)]))
    old = MI("m" * 3000)
    r = rec(qname="big", aux_pre=[XA, old, arr, MI("behind"), RX(umi)])
    want = rec(qname="big", aux_pre=[XA, arr, RX(umi)], nm=None, aux_post=[("NM", "C", 1), MI(":" + umi.replace("-", "_"))])
    return r, want


def frames(recs):
    return b"".join(struct.pack("<I", len(r)) + r for r in recs)


def file_records():
    """every case record and the alignment family: the file of the GPU tests (about 9 KB; they repeat it)"""
    return [c[2] for c in all_cases()]


# ---------------------------------------------------------------- an end-to-end stream
def norm(u):
    return u.upper().replace("-", "_").replace("+", "_")


def stream(style, seed=11):
    """About 30 molecules of 1-4 pairs, 20M reads on a 2 kb reference, duplex UMIs such as ACGTAC-TTGACA; molecules come two to a position
    pair with UMIs far apart, some reads one mismatch off their molecule's UMI, some molecules with a duplex partner (B-A on the other
    strand).  style "RX": the UMI in RX:Z; "name": as ...:ACGTAC+TTGACA behind the name; None: nowhere.
    -> (reference, targets, records A as the file has them, records B: the same with mi = ":" + norm(UMI) and no other change)"""
    import random
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(2000))
    half = lambda: "".join(rng.choice("ACGT") for _ in range(6))
    a, b = [], []
    for m in range(30):
        left = 100 + 55 * (m // 2)                                # two molecules to a position pair
        right = left + 200 + (m // 2) % 7
        u1, u2 = half(), half()
        sides = [(99, 147, u1, u2)] + ([(83, 163, u2, u1)] if m % 3 == 0 else [])
        for fl, fr, x, y in sides:
            for dpl in range(1 + rng.randrange(4)):
                xs = x if rng.random() < 0.8 else x[:5] + rng.choice("ACGT")
                if rng.random() < 0.1:
                    xs = xs.lower()
                umi = xs + "-" + y
                name = "m%02d_%d_%d" % (m, fl, dpl)
                extra = {}
                if style == "RX":
                    extra = dict(aux_pre=[("RX", "Z", umi)])
                elif style == "name":
                    name = "M01:7:FC:1:1101:%d:%d:%s" % (m, 10 * fl + dpl, umi.replace("-", "+"))
                isz = right + 20 - left
                mates = ((99, left, right, isz), (147, right, left, -isz)) if fl == 99 else ((83, right, left, -isz), (163, left, right, isz))
                for flag, pos, mpos, isize in mates:
                    r = dict(qname=name, flag=flag, tid=0, pos=pos, cigar="20M", mtid=0, mpos=mpos, isize=isize, seq=ref[pos:pos + 20],
                             qual=[rng.choice([37, 25, 11]) for _ in range(20)], nm=0, **extra)
                    a.append(r)
                    b.append(dict(r, mi=":" + norm(umi)) if style else dict(r))
    order = sorted(range(len(a)), key=lambda k: a[k]["pos"])
    return ref, [("c0", len(ref))], [a[k] for k in order], [b[k] for k in order]
