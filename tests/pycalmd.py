"""Pure-Python model of gce_bam_calmd (struct only, on the raw records tests/pysort.py cuts a file into), written from the
rules and not from gencore_amd/csrc/gce_calmd.hpp:
  E  a record is rewritten when flag & 4 == 0, 0 <= tid < n_ref, n_cigar_op > 0, l_seq > 0, every CIGAR code <= 8, the query bases the CIGAR
     consumes (M I S = X) equal l_seq and the FASTA has a contig of the header's name for tid; every other record is copied byte for byte
     (a record whose fixed fields overrun its block_size -- no file reader lets one through -- is copied too)
  R  reference bases are the loader's ASCII bytes; 16-code = index in "=ACMGRSVTWYHKDBN", else 15; MD letter = the byte if A..Z else N
  W  the walk of the CIGAR: see walk()
  T  the optional fields must tile the area behind QUAL (only rewritten records are walked); every NM and MD is dropped, the others are kept
     verbatim and in order, then NM (C / S / I, the smallest unsigned type) and MD:Z are appended; block_size follows
  C  counters: n_nm_changed -- no NM, or the FIRST NM is no integer or has another value; n_md_changed -- no MD, or the FIRST MD is no Z
     field or has another string
A record whose new block_size would pass 2^28 (the largest the record index reads back) is refused like a malformed one."""
import struct

import pysort

CODES = "=ACMGRSVTWYHKDBN"
MAX_BLOCK = 1 << 28
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class CalmdError(ValueError):
    """.record: the lowest malformed record, counting from 0"""

    def __init__(self, record):
        self.record = record
        super().__init__("record %d: optional fields do not tile block_size" % record)


class Malformed(ValueError):
    pass


def fields(area):
    """the optional fields of `area` as (tag, type, whole field bytes, value bytes); Malformed unless they tile it exactly"""
    out, p = [], 0
    while p < len(area):
        if len(area) - p < 3:
            raise Malformed("stray bytes")
        tag, typ = area[p:p + 2], chr(area[p + 2])
        v = p + 3
        if typ in FIXED:
            n = FIXED[typ]
        elif typ in "ZH":
            z = area.find(b"\0", v)
            if z < 0:
                raise Malformed("no NUL")
            n = z + 1 - v
        elif typ == "B":
            if len(area) - v < 5:
                raise Malformed("B header cut")
            es = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(chr(area[v]))
            if es is None:
                raise Malformed("B subtype")
            n = 5 + es * struct.unpack_from("<I", area, v + 1)[0]
        else:
            raise Malformed("type")
        if v + n > len(area):
            raise Malformed("field cut")
        out.append((tag, typ, area[p:v + n], area[v:v + n]))
        p = v + n
    return out


def code16(b):
    i = CODES.find(chr(b))
    return i if i >= 0 else 15


def letter(b):
    return chr(b) if 65 <= b <= 90 else "N"


def walk(pos, cigar, nib, contig):
    """rule W.  cigar: [(code, length)]; nib(i): the read's nibble i; contig: bytes.  -> (nm, md)"""
    x, y, u, nm, md = pos, 0, 0, 0, []
    inside = lambda q: 0 <= q < len(contig)
    for op, ln in cigar:
        if op in (0, 7, 8):
            stop = False
            for j in range(ln):
                if not inside(x + j):
                    stop = True
                    break
                c1, c2 = nib(y + j), code16(contig[x + j])
                if c1 == 0 or (c1 == c2 and c1 != 15):
                    u += 1
                else:
                    md.append("%d%s" % (u, letter(contig[x + j])))
                    u = 0
                    nm += 1
            if stop:
                break
            x += ln
            y += ln
        elif op == 2:
            k = 0
            while k < ln and inside(x + k):
                k += 1
            if k == 0:                                          # an ^ that no letter follows is not written
                break
            md.append("%d^%s" % (u, "".join(letter(contig[x + j]) for j in range(k))))
            nm += k
            u = 0
            x += ln
            if k < ln:
                break
        elif op == 1:
            y += ln
            nm += ln
        elif op == 4:
            y += ln
        elif op == 3:
            x += ln
    md.append("%d" % u)
    return nm, "".join(md)


def nm_field(nm):
    if nm <= 255:
        return b"NMC" + struct.pack("<B", nm)
    if nm <= 65535:
        return b"NMS" + struct.pack("<H", nm)
    return b"NMI" + struct.pack("<I", nm)


def rewrite(rec, n_ref, contig_of):
    """one raw record (block_size first) -> (new record, info); info: dict(rewritten, no_ref, nm_changed, md_changed, nm, md).
    contig_of(tid) -> bytes or None.  Malformed for rule T's refusal."""
    same = (rec, dict(rewritten=False, no_ref=False, nm_changed=False, md_changed=False, nm=None, md=None))
    bs = struct.unpack_from("<I", rec, 0)[0]
    assert len(rec) == 4 + bs and bs >= 32
    tid, pos, lq, _mapq, _bin, nc, flag, lseq = struct.unpack_from("<iiBBHHHi", rec, 4)
    if lq < 1 or lseq < 0 or 32 + lq + 4 * nc + (lseq + 1) // 2 + lseq > bs:
        return same
    if flag & 4 or not 0 <= tid < n_ref or nc == 0 or lseq <= 0:
        return same
    cg = 36 + lq
    words = struct.unpack_from("<%dI" % nc, rec, cg)
    cigar = [(w & 15, w >> 4) for w in words]
    if any(op > 8 for op, _ in cigar) or sum(ln for op, ln in cigar if op in (0, 1, 4, 7, 8)) != lseq:
        return same
    contig = contig_of(tid)
    if contig is None:
        return rec, dict(same[1], no_ref=True)
    sq = cg + 4 * nc
    ax = sq + (lseq + 1) // 2 + lseq
    fl = fields(rec[ax:])
    nm, md = walk(pos, cigar, lambda i: (rec[sq + (i >> 1)] >> (0 if i & 1 else 4)) & 15, contig)
    kept = b"".join(f[2] for f in fl if f[0] not in (b"NM", b"MD"))
    new = rec[4:ax] + kept + nm_field(nm) + b"MDZ" + md.encode() + b"\0"
    if len(new) > MAX_BLOCK or nm > 0xFFFFFFFF:
        raise Malformed("the record would outgrow 2^28 bytes")
    old_nm = [f for f in fl if f[0] == b"NM"]
    old_md = [f for f in fl if f[0] == b"MD"]
    nm_changed = not (old_nm and old_nm[0][1] in INT_FMT and struct.unpack(INT_FMT[old_nm[0][1]], old_nm[0][3])[0] == nm)
    md_changed = not (old_md and old_md[0][1] == "Z" and old_md[0][3] == md.encode() + b"\0")
    return struct.pack("<I", len(new)) + new, dict(rewritten=True, no_ref=False, nm_changed=nm_changed, md_changed=md_changed, nm=nm, md=md)


def contig_names(hdr):
    """the names of the header's contig table (pysort.split's hdr), each up to its first NUL"""
    t, p, names = hdr["contigs"], 4, []
    for _ in range(hdr["n_ref"]):
        (ln,) = struct.unpack_from("<i", t, p)
        names.append(t[p + 4:p + 4 + ln].split(b"\0", 1)[0].decode("latin-1"))
        p += 4 + ln + 4
    return names


def calmd_records(recs, names, fasta):
    """raw records -> (new raw records, the six counters); fasta: {name: bytes} as load_fasta returns it.  CalmdError names the lowest
    malformed record."""
    contig_of = lambda t: fasta.get(names[t])
    out, c = [], dict(n_records=len(recs), n_rewritten=0, n_unchanged=0, n_no_ref=0, n_nm_changed=0, n_md_changed=0)
    for k, r in enumerate(recs):
        try:
            new, info = rewrite(r, len(names), contig_of)
        except Malformed:
            raise CalmdError(k)
        out.append(new)
        c["n_rewritten"] += info["rewritten"]
        c["n_unchanged"] += not info["rewritten"]
        c["n_no_ref"] += info["no_ref"]
        c["n_nm_changed"] += info["nm_changed"]
        c["n_md_changed"] += info["md_changed"]
    return out, c


def calmd_model(path, fasta):
    """a BAM file -> (its header's bytes, unchanged; the new raw records; the counters)"""
    u = pysort.inflate(open(str(path), "rb").read())
    hdr, recs = pysort.split(u)
    head = u[:len(u) - sum(len(r) for r in recs)]
    out, c = calmd_records(recs, contig_names(hdr), fasta)
    return head, out, c
