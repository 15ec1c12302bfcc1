"""The model of gce_bam_error_profile_quality's rules: eligible records, segment, the walk, the BED and the mask (rules E, G, W, B,
Y: pyerrprof's and pyerrmask's, imported and left alone), the quality bucket of an event (rule Q) and the table (rule O), in plain Python over
whole BAM records (bytes, block_size first).  The kernels of gencore_amd/csrc/gce_errqual.hpp reproduce its integers exactly;
tests/qualcases.py holds records whose rows are written out by hand.

Rule Q is stated on the query index, not on the cycle: query_indices walks the CIGAR itself, in pyerrprof.walk's order, and QUAL is read at
that index in the stored orientation -- the kernel gets the same index back out of the cycle row the walk hands it."""
import pyerrmask
import pyerrprof
import pypileup

BUCKETS = 96
TOP, NOQ = 94, 95
ROW = pyerrprof.ROW
MASKED = 21
CLASSES = pyerrprof.CLASSES + ["MASKED"]
SKIPS = pyerrprof.SKIPS
HEADER = "#segment\tquality\tbases\tmismatches\t" + "\t".join(pyerrprof.CLASSES) + "\n"
HEADER_MASKED = HEADER[:-1] + "\tMASKED\n"


def bucket(b):
    """rule Q's bucket of a QUAL byte"""
    return b if b <= 93 else TOP


def query_indices(f):
    """the query index whose QUAL byte an event is charged to, one per event of pyerrprof.walk and in its order: a column's own, an inserted
    base's own, a deletion's the base in front of it (the first, when there is none)"""
    q = 0
    for op, ln in f["cigar"]:
        if op in (0, 7, 8):
            for k in range(ln):
                yield q + k
            q += ln
        elif op == 2:
            yield max(q - 1, 0)
        elif op == 1:
            for k in range(ln):
                yield q + k
            q += ln
        elif op == 4:
            q += ln


def events(f, ref, min_baseq):
    """(anchor, segment, bucket, class) of every event of an eligible record"""
    has_q = f["qual"][0] != 0xFF
    ev = list(pyerrprof.walk(f, ref, min_baseq))
    ys = list(query_indices(f))
    assert len(ev) == len(ys)
    for (x, g, _, c), y in zip(ev, ys):
        yield x, g, (bucket(f["qual"][y]) if has_q else NOQ), c


def profile(records, refs, lens, mask=None, regions=None, min_mapq=0, min_baseq=0, exclude=0x704):
    """records: whole BAM records (bytes); refs, lens, regions, the thresholds: pyerrprof.profile's; mask: None, or rule K's intervals as
    pyerrmask.profile takes them -> dict(counts ([3][96][24]), n_records, n_eligible, the eight skip counters, n_bases, n_mismatches,
    n_masked_events, n_intervals); ErrprofError names the lowest malformed record"""
    target, n_intervals = None, -1
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
    counts = [[[0] * ROW for _ in range(BUCKETS)] for _ in range(3)]
    res = dict(n_records=len(records), n_eligible=0, n_intervals=n_intervals)
    res.update({k: 0 for k in SKIPS})
    for f in parsed:
        sk = pyerrprof.skip_of(f, refs, min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        res["n_eligible"] += 1
        for x, g, b, c in events(f, refs[f["tid"]], min_baseq):
            if target is None or target(f["tid"], x):
                counts[g][b][MASKED if inside is not None and pyerrmask.masked_at(inside, refs, f["tid"], x) else c] += 1
    res["counts"] = counts
    return pyerrmask.totals(res)


def nonzero(res):
    """{(segment, bucket, class name): count} of the counters that are not zero"""
    return {(g, b, CLASSES[c]): v for g, seg in enumerate(res["counts"]) for b, row in enumerate(seg) for c, v in enumerate(row[:22]) if v}


def by_class(res):
    """the table summed over the buckets: [segment][class 0..21]"""
    return [[sum(row[c] for row in seg) for c in range(22)] for seg in res["counts"]]


def label(b):
    return "." if b == NOQ else "94+" if b == TOP else str(b)


def table(res, masked=False):
    """rule O: the table's bytes; masked: the run had a mask, so the trailing MASKED column"""
    out = [HEADER_MASKED if masked else HEADER]
    for g, seg in enumerate(res["counts"]):
        for b, k in enumerate(seg):
            if any(k[:22]):
                mism = sum(k[4 * a + c] for a in range(4) for c in range(4) if a != c)
                out.append("%d\t%s\t%d\t%d\t%s\n" % (g, label(b), sum(k[:16]), mism, "\t".join(str(v) for v in k[:22 if masked else 21])))
    return "".join(out).encode()
