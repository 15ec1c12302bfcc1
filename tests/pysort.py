"""Pure-Python model of gce_bam_sort (zlib and struct only, its own reader): the inflated stream of a BAM file cut into raw
records, rule S's order with Python's stable sort, rule H's header.  The GPU tests compare bytes with it."""
import struct
import zlib


class SortError(ValueError):
    pass


EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def inflate(blob):
    """the members of a BGZF file, one after another, each with plain zlib (CRC and ISIZE checked)"""
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04", "not a BGZF member at %d" % p
        (xlen,) = struct.unpack_from("<H", blob, p + 10)
        x, bsize = p + 12, None
        while x < p + 12 + xlen:
            si, sl = blob[x:x + 2], struct.unpack_from("<H", blob, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", blob, x + 4)[0] + 1
            x += 4 + sl
        assert bsize is not None and p + bsize <= len(blob)
        data = zlib.decompress(blob[p + 12 + xlen:p + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", blob, p + bsize - 8)
        assert zlib.crc32(data) & 0xFFFFFFFF == crc and len(data) == isize
        out.append(data)
        p += bsize
    return b"".join(out)


def split(u):
    """inflated stream -> (header fields, raw records); header fields: dict(text=bytes as stored, l_text, n_ref, contigs=the contig table's bytes)"""
    assert u[:4] == b"BAM\1"
    (lt,) = struct.unpack_from("<i", u, 4)
    p = 8 + lt
    (n_ref,) = struct.unpack_from("<i", u, p)
    q = p + 4
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", u, q)
        q += 4 + ln + 4
    hdr = dict(text=u[8:8 + lt], l_text=lt, n_ref=n_ref, contigs=u[p:q])
    recs = []
    while q < len(u):
        (bs,) = struct.unpack_from("<i", u, q)
        assert bs >= 32 and q + 4 + bs <= len(u)
        recs.append(u[q:q + 4 + bs])
        q += 4 + bs
    return hdr, recs


def records(path):
    return split(inflate(open(str(path), "rb").read()))


def key(n_ref, k, r):
    """rule S without the input index (the sort is stable)"""
    tid, pos = struct.unpack_from("<ii", r, 4)
    (flag,) = struct.unpack_from("<H", r, 18)
    if tid >= n_ref:
        raise SortError("record %d names a contig the header does not have" % k)
    return (n_ref if tid < 0 else tid, (pos + 1) & 0xFFFFFFFF, (flag >> 4) & 1)


def header_text(text):
    """rule H on the stored text (bytes)"""
    t = text.split(b"\0", 1)[0]
    if not t.startswith(b"@HD"):
        return b"@HD\tVN:1.6\tSO:coordinate\n" + t
    eol = t.find(b"\n")
    if eol < 0:
        eol = len(t)
    line, rest = t[:eol], t[eol:]
    f = line.split(b"\t")
    if any(x.startswith(b"SO:") for x in f[1:]):
        done = False
        for i in range(1, len(f)):
            if f[i].startswith(b"SO:") and not done:
                f[i], done = b"SO:coordinate", True
        line = b"\t".join(f)
    else:
        line += b"\tSO:coordinate"
    return line + rest


def header_bytes(hdr):
    t = header_text(hdr["text"])
    return b"BAM\1" + struct.pack("<i", len(t)) + t + hdr["contigs"]


def sort_model(path):
    """-> (new header bytes, raw records in rule S's order)"""
    hdr, recs = records(path)
    keys = [key(hdr["n_ref"], k, r) for k, r in enumerate(recs)]
    order = sorted(range(len(recs)), key=lambda k: keys[k])
    return header_bytes(hdr), [recs[k] for k in order]


def descents(path):
    hdr, recs = records(path)
    keys = [key(hdr["n_ref"], k, r) for k, r in enumerate(recs)]
    return sum(1 for a, b in zip(keys, keys[1:]) if b < a)


def n_unplaced(recs):
    return sum(1 for r in recs if struct.unpack_from("<i", r, 4)[0] < 0)


def write(path, header, recs, block=0xff00, level=1):
    """header bytes and raw records as a BAM file: the header in members of its own, then the record stream (rule F)"""
    import pybam
    body = b"".join(recs)
    with open(str(path), "wb") as f:
        for o in range(0, len(header), block):
            f.write(pybam.bgzf_block(header[o:o + block], level))
        for o in range(0, len(body), block):
            f.write(pybam.bgzf_block(body[o:o + block], level))
        f.write(EOF_BLOCK)
