"""The model of gce_bam_error_profile_support's rules: eligible records (rule E with its ninth skip, n_bad_aux), support (rule U:
the buckets of the forward and the reverse tag), the walk, the BED and the mask (rules W, B, Y: pyerrprof's and pyerrmask's, imported and left
alone) and the table (rule O), in plain Python over whole BAM records (bytes, block_size first).  The kernels of gencore_amd/csrc/gce_errsup.hpp
reproduce its integers exactly; tests/supcases.py holds records whose rows are written out by hand."""
import struct

import pyerrmask
import pyerrprof
import pypileup

BUCKETS = 33
TOP = 32
ROW = pyerrprof.ROW
MASKED, RECORDS = 21, 22
CLASSES = pyerrprof.CLASSES + ["MASKED", "RECORDS"]
SKIPS = pyerrprof.SKIPS + ["n_bad_aux"]
HEADER = "#segment\tforward\treverse\trecords\tbases\tmismatches\t" + "\t".join(pyerrprof.CLASSES) + "\n"
HEADER_MASKED = HEADER[:-1] + "\tMASKED\n"
INT_TYPES = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
ELEMENT = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def aux_start(r):
    """the offset of the first optional field of a record whose core fields fit its block_size"""
    lq, _, _, nc, _, lseq = struct.unpack_from("<BBHHHi", r, 12)
    return 36 + lq + 4 * nc + (lseq + 1) // 2 + lseq


def aux_fields(r):
    """rule T's walk from the end of QUAL to the end of the block -> ([(tag, type, offset of the value)], bad); bad: the walk was refused while
    bytes remained -- fewer than three, an unknown type or B subtype, a Z / H without its NUL, a value that passes the block's end"""
    end = 4 + struct.unpack_from("<I", r, 0)[0]
    p, out = aux_start(r), []
    while p < end:
        if end - p < 3:
            return out, True
        tag, typ, v = r[p:p + 2], chr(r[p + 2]), p + 3
        if typ in SIZES:
            n = SIZES[typ]
        elif typ in "ZH":
            z = r.find(b"\0", v, end)
            if z < 0:
                return out, True
            n = z + 1 - v
        elif typ == "B":
            if end - v < 5 or chr(r[v]) not in ELEMENT:
                return out, True
            n = 5 + ELEMENT[chr(r[v])] * struct.unpack_from("<I", r, v + 1)[0]
        else:
            return out, True
        if n > end - v:
            return out, True
        out.append((tag, typ, v))
        p = v + n
    return out, False


def bucket(v):
    return v if 1 <= v <= 31 else TOP


def support(r, tags=("FR", "RR")):
    """rule U -> (f, r, bad): per tag the bucket of the FIRST field that carries it, 0 when there is none or its type is not one of c C s S i I"""
    fields, bad = aux_fields(r)
    out = []
    for t in tags:
        b = 0
        for tag, typ, v in fields:
            if tag == t.encode("latin-1"):
                if typ in INT_TYPES:
                    b = bucket(struct.unpack_from(INT_TYPES[typ], r, v)[0])
                break
        out.append(b)
    return out[0], out[1], bad


def kept(f, iv):
    """what the scan keeps of an eligible record: all without a BED; with one those whose reference span, widened by one position at both
    ends, touches an interval (iv: pypileup.intervals' (tid, start, end, site0))"""
    if iv is None:
        return True
    rlen = sum(ln for op, ln in f["cigar"] if op in (0, 2, 3, 7, 8))
    return any(t == f["tid"] and z >= f["pos"] and a <= f["pos"] + rlen for t, a, z, _ in iv)


def profile(records, refs, lens, mask=None, regions=None, min_mapq=0, min_baseq=0, exclude=0x704, tags=("FR", "RR")):
    """records: whole BAM records (bytes); refs, lens, regions, the thresholds: pyerrprof.profile's; mask: None, or rule K's intervals as
    pyerrmask.profile takes them -> dict(counts ([3][33][33][24]), n_records, n_eligible, the nine skip counters, n_with_forward,
    n_with_reverse, n_bases, n_mismatches, n_masked_events, n_intervals); ErrprofError names the lowest malformed record"""
    iv, target, n_intervals = None, None, -1
    if regions is not None:
        iv, _ = pypileup.intervals(regions, lens)
        n_intervals = len(iv)
        target = pyerrmask.tester([(t, a, z) for t, a, z, _ in iv])
    inside = pyerrmask.tester(mask) if mask is not None else None
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(pyerrprof.fields(r))
        except pyerrprof.Malformed as e:
            raise pyerrprof.ErrprofError("BAM record %d (counting from 0): %s" % (k, e), k)
    counts = [[[[0] * ROW for _ in range(BUCKETS)] for _ in range(BUCKETS)] for _ in range(3)]
    res = dict(n_records=len(records), n_eligible=0, n_intervals=n_intervals)
    res.update({k: 0 for k in SKIPS})
    for f, r in zip(parsed, records):
        sk = pyerrprof.skip_of(f, refs, min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        sf, sr, bad = support(r, tags)
        if bad:
            res["n_bad_aux"] += 1
            continue
        res["n_eligible"] += 1
        if not kept(f, iv):
            continue
        row = counts[pyerrprof.segment(f["flag"])][sf][sr]
        row[RECORDS] += 1
        for x, g, cy, c in pyerrprof.walk(f, refs[f["tid"]], min_baseq):
            if target is None or target(f["tid"], x):
                row[MASKED if inside is not None and pyerrmask.masked_at(inside, refs, f["tid"], x) else c] += 1
    res["counts"] = counts
    rows = [(sf, sr, row) for seg in counts for sf, fr in enumerate(seg) for sr, row in enumerate(fr)]
    res["n_bases"] = sum(sum(row[:16]) for _, _, row in rows)
    res["n_mismatches"] = sum(row[4 * a + b] for _, _, row in rows for a in range(4) for b in range(4) if a != b)
    res["n_masked_events"] = sum(row[MASKED] for _, _, row in rows)
    res["n_with_forward"] = sum(row[RECORDS] for sf, _, row in rows if sf)
    res["n_with_reverse"] = sum(row[RECORDS] for _, sr, row in rows if sr)
    return res


def nonzero(res):
    """{(segment, forward, reverse, class name): count} of the counters that are not zero"""
    return {(g, sf, sr, CLASSES[c]): v for g, seg in enumerate(res["counts"]) for sf, fr in enumerate(seg) for sr, row in enumerate(fr) for c, v in enumerate(row[:23]) if v}


def by_class(res):
    """the table summed over (forward, reverse): [segment][class 0..21]"""
    return [[sum(row[c] for fr in seg for row in fr) for c in range(22)] for seg in res["counts"]]


def label(b):
    return "." if b == 0 else "32+" if b == TOP else str(b)


def table(res, masked=False):
    """rule O: the table's bytes; masked: the run had a mask, so the trailing MASKED column"""
    out = [HEADER_MASKED if masked else HEADER]
    for g, seg in enumerate(res["counts"]):
        for sf, fr in enumerate(seg):
            for sr, k in enumerate(fr):
                if any(k[:23]):
                    mism = sum(k[4 * a + b] for a in range(4) for b in range(4) if a != b)
                    out.append("%d\t%s\t%s\t%d\t%d\t%d\t%s\n" % (g, label(sf), label(sr), k[RECORDS], sum(k[:16]), mism, "\t".join(str(v) for v in k[:22 if masked else 21])))
    return "".join(out).encode()
