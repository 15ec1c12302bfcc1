"""The model of gce_bam_error_profile's rules: eligible records (rule E), segment (G), cycle (C), the walk (W), the BED (B) and the
table (O), in plain Python over whole BAM records (bytes, block_size first).  The kernels of gencore_amd/csrc/gce_errprof.hpp reproduce its
integers exactly; tests/errprofcases.py holds records whose counters are written out by hand.  Record fields, pileup's six skips and rule S's
intervals are tests/pypileup.py's."""
import bisect

import pypileup
from pypileup import Malformed, fields, fields_of_pybam, read_bed, read_fasta  # noqa: F401

MAX_CYCLE = 1024
ROW = 24
CLASSES = ["%s>%s" % (r, b) for r in "ACGT" for b in "ACGT"] + ["READ_N", "REF_OTHER", "LOWQ", "INS", "DEL"]
READ_N, REF_OTHER, LOWQ, INS, DEL = 16, 17, 18, 19, 20
SKIPS = pypileup.SKIPS + ["n_no_ref", "n_too_long"]
HEADER = "#segment\tcycle\tbases\tmismatches\t" + "\t".join(CLASSES) + "\n"


class ErrprofError(Exception):
    def __init__(self, msg, record=None):
        super().__init__(msg)
        self.record = record


def skip_of(f, refs, min_mapq, exclude):
    """rule E: None for an eligible record, else the one counter it goes to.  refs: per tid the contig's bases (bytes or str), None where the
    FASTA lacks it"""
    sk = pypileup.skip_of(f, len(refs), min_mapq, exclude)
    if sk:
        return sk
    if refs[f["tid"]] is None:
        return "n_no_ref"
    if f["lseq"] > MAX_CYCLE:
        return "n_too_long"
    return None


def segment(flag):
    return 1 if flag & 0xC0 == 0x40 else 2 if flag & 0xC0 == 0x80 else 0


def walk(f, ref, min_baseq):
    """rule W: every event of an eligible record as (anchor position, segment, cycle, class), whether or not the anchor is a target"""
    if isinstance(ref, str):
        ref = ref.encode()
    x, q, rev, g, n = f["pos"], 0, bool(f["flag"] & 16), segment(f["flag"]), f["lseq"]
    cyc = (lambda y: n - y) if rev else (lambda y: y + 1)
    has_q = f["qual"][0] != 0xFF
    seen = False
    for op, ln in f["cigar"]:
        if op in (0, 7, 8):
            for k in range(ln):
                y = q + k
                nib = (f["seq"][y >> 1] >> (0 if y & 1 else 4)) & 15
                r = "ACGT".find(chr(ref[x + k]).upper()) if x + k < len(ref) else -1
                b = {1: 0, 2: 1, 4: 2, 8: 3}.get(nib, -1)
                if has_q and f["qual"][y] < min_baseq:
                    c = LOWQ
                elif r < 0:
                    c = REF_OTHER
                elif b < 0:
                    c = READ_N
                else:
                    c = 4 * (3 - r) + (3 - b) if rev else 4 * r + b
                yield x + k, g, cyc(y), c
            x += ln
            q += ln
            seen = True
        elif op == 2:
            yield x, g, cyc(max(q - 1, 0)), DEL
            x += ln
            seen = True
        elif op == 3:
            x += ln
        elif op == 1:
            for k in range(ln):
                yield (x - 1 if seen else x), g, cyc(q + k), INS
            q += ln
        elif op == 4:
            q += ln


def profile(records, refs, lens, regions=None, min_mapq=0, min_baseq=0, exclude=0x704):
    """records: whole BAM records (bytes), or dicts of tests/pybam.py's read_bam; refs: per tid the FASTA's bases or None; lens: the header's
    contig lengths (rule B clamps to them); regions: None, or [(tid, start, end)] as gce_bed_load gives them
    -> dict(counts ([3][1024][24]), n_records, n_eligible, the eight skip counters, n_bases, n_mismatches, n_intervals); ErrprofError names
    the lowest malformed record"""
    target = None
    n_intervals = -1
    if regions is not None:
        iv, _ = pypileup.intervals(regions, lens)
        n_intervals = len(iv)
        ends = [(it, z) for it, a, z, _ in iv]                   # (disjoint and in order: the first interval that ends behind x holds it or none does)

        def target(t, x):
            j = bisect.bisect_right(ends, (t, x))
            return j < len(iv) and iv[j][0] == t and iv[j][1] <= x
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(fields_of_pybam(r) if isinstance(r, dict) else fields(r))
        except Malformed as e:
            raise ErrprofError("BAM record %d (counting from 0): %s" % (k, e), k)
    counts = [[[0] * ROW for _ in range(MAX_CYCLE)] for _ in range(3)]
    res = dict(n_records=len(records), n_eligible=0, n_intervals=n_intervals)
    res.update({k: 0 for k in SKIPS})
    for f in parsed:
        sk = skip_of(f, refs, min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        res["n_eligible"] += 1
        for x, g, cy, c in walk(f, refs[f["tid"]], min_baseq):
            if target is None or target(f["tid"], x):
                counts[g][cy - 1][c] += 1
    res["counts"] = counts
    res["n_bases"] = sum(sum(row[:16]) for seg in counts for row in seg)
    res["n_mismatches"] = sum(row[4 * r + b] for seg in counts for row in seg for r in range(4) for b in range(4) if r != b)
    return res


def refs_of(fasta, names):
    """{contig name: bases} -> the per-tid list profile takes"""
    return [fasta.get(nm) for nm in names]


def nonzero(res):
    """{(segment, cycle, class name): count} of the counters that are not zero"""
    return {(g, cy + 1, CLASSES[c]): v for g, seg in enumerate(res["counts"]) for cy, row in enumerate(seg) for c, v in enumerate(row[:21]) if v}


def table(res):
    """rule O: the table's bytes"""
    out = [HEADER]
    for g, seg in enumerate(res["counts"]):
        last = max([cy + 1 for cy, row in enumerate(seg) if any(row)] or [0])
        for cy in range(1, last + 1):
            k = seg[cy - 1]
            mism = sum(k[4 * r + b] for r in range(4) for b in range(4) if r != b)
            out.append("%d\t%d\t%d\t%d\t%s\n" % (g, cy, sum(k[:16]), mism, "\t".join(str(v) for v in k[:21])))
    return "".join(out).encode()
