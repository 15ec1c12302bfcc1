"""Pure-Python model of gce_bam_umi_to_mi (struct only, on the raw records tests/pysort.py cuts a file into), written from the
rules and not from gencore_amd/csrc/gce_umi.hpp.  `source` is a two-character tag or "name".  Per record:
  S  the source string s.  A tag: the value of the FIRST optional field with that tag, if its type is Z.  "name": the bytes of the read name up
     to its first NUL inside l_read_name, behind its last `:`.  No such field, no `:`, another type or an empty s: the record has no source.
  V  s is a UMI when every byte is one of ACGTNacgtn or a separator (- + _), there is at most one separator, it is neither the first nor the
     last byte, and len(s) <= 250.  (A separator at either end leaves one half empty; the reference's parser would also skip a leading `_`,
     src/bamutil.cpp:95-96, so the value would not arrive as written.)
  M  a record with a source that is a UMI: every optional field tagged MI, of any type, is dropped, the others are kept verbatim and in order,
     and MI Z ":" norm(s) NUL is appended; norm: letters upper case, - and + to _.  block_size follows; nothing else changes.  N is passed on.
     Every other record is copied byte for byte, its own MI fields with it.
  T  the optional fields of EVERY record must tile the area behind QUAL (calmd's walk, tests/pycalmd.fields); a record whose fields do not,
     or whose new block_size would pass 2^28, is malformed and ends the run, which names the lowest such record.  (A record whose fixed fields
     overrun its block_size -- no file reader lets one through -- has no such area: it is copied, without a source.)
Counters: n_tagged (rule M applied), n_no_source, n_not_umi (the three add up to n_records), n_mi_dropped (tagged records that had an MI)."""
import struct

import pycalmd
import pysort

MAX_BLOCK = 1 << 28
MAX_LEN = 250
SEPARATORS = b"-+_"
BASES = b"ACGTNacgtn"


class UmiError(ValueError):
    """.record: the lowest malformed record, counting from 0"""

    def __init__(self, record):
        self.record = record
        super().__init__("record %d: optional fields do not tile block_size" % record)


Malformed = pycalmd.Malformed


def is_umi(s):
    seps = [k for k, b in enumerate(s) if b in SEPARATORS]
    return (len(s) <= MAX_LEN and all(b in BASES or b in SEPARATORS for b in s) and len(seps) <= 1
            and not (seps and seps[0] in (0, len(s) - 1)))


def norm(s):
    return bytes(ord("_") if b in SEPARATORS else b & 0xDF for b in s)


def rewrite(rec, source):
    """one raw record (block_size first) -> (new record, info); info: dict(tagged, no_source, not_umi, mi_dropped, umi).  Malformed for rule T."""
    info = dict(tagged=False, no_source=True, not_umi=False, mi_dropped=False, umi=None)
    bs = struct.unpack_from("<I", rec, 0)[0]
    assert len(rec) == 4 + bs and bs >= 32
    lq, nc, lseq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    if lq < 1 or lseq < 0 or 32 + lq + 4 * nc + (lseq + 1) // 2 + lseq > bs:
        return rec, info
    ax = 36 + lq + 4 * nc + (lseq + 1) // 2 + lseq
    fl = pycalmd.fields(rec[ax:])                                # rule T, for every record
    s = b""
    if source == "name":
        name = rec[36:36 + lq].split(b"\0", 1)[0]
        if b":" in name:
            s = name.rsplit(b":", 1)[1]
    else:
        first = [f for f in fl if f[0] == source.encode()][:1]
        if first and first[0][1] == "Z":
            s = first[0][3][:-1]
    if not s:
        return rec, info
    info["no_source"] = False
    if not is_umi(s):
        return rec, dict(info, not_umi=True)
    kept = b"".join(f[2] for f in fl if f[0] != b"MI")
    new = rec[4:ax] + kept + b"MIZ:" + norm(s) + b"\0"
    if len(new) > MAX_BLOCK:
        raise Malformed("the record would outgrow 2^28 bytes")
    return struct.pack("<I", len(new)) + new, dict(info, tagged=True, mi_dropped=any(f[0] == b"MI" for f in fl), umi=norm(s))


def umi_records(recs, source):
    """raw records -> (new raw records, the counters); UmiError names the lowest malformed record"""
    out, c = [], dict(n_records=len(recs), n_tagged=0, n_no_source=0, n_not_umi=0, n_mi_dropped=0)
    for k, r in enumerate(recs):
        try:
            new, info = rewrite(r, source)
        except Malformed:
            raise UmiError(k)
        out.append(new)
        for key in ("tagged", "no_source", "not_umi", "mi_dropped"):
            c["n_" + key] += info[key]
    return out, c


def umi_model(path, source):
    """a BAM file -> (its header's bytes, unchanged; the new raw records; the counters)"""
    u = pysort.inflate(open(str(path), "rb").read())
    _, recs = pysort.split(u)
    head = u[:len(u) - sum(len(r) for r in recs)]
    out, c = umi_records(recs, source)
    return head, out, c
