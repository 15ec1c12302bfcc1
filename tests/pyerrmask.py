"""The model of the error profile's variant mask: rule K (the mask file -> merged intervals and counters) and rule Y (an event
whose anchor is masked goes to class 21, MASKED) for gce_bam_error_profile_masked and gce_bam_error_profile_fragments_masked, in plain Python.
Rule Y for the plain pass re-classes pyerrprof.walk's events, which carry their anchor; for the fragment pass it is restated on pyfragerr's
helpers.  Both files are imported and left alone.  gce_mask_load, the kernels of gencore_amd/csrc/gce_errprof.hpp / gce_fragerr.hpp and the
fill kernel of gce_varmask.hpp reproduce these integers exactly; tests/maskcases.py holds texts and records written out by hand."""
import bisect
import gzip

import pyerrprof
import pyfragerr
import pyfragpile
import pypileup
from pyerrprof import DEL, INS, LOWQ, READ_N, REF_OTHER, ErrprofError

MASKED = 21
CLASSES = pyerrprof.CLASSES + ["MASKED"]
OVL_CLASSES = pyfragerr.OVL_CLASSES + ["MASKED"]
HEADER = pyerrprof.HEADER[:-1] + "\tMASKED\n"
OVL_HEADER = pyfragerr.OVL_HEADER[:-1] + "\tMASKED\n"
COUNTERS = ["n_lines", "n_records", "n_unknown_contig", "n_no_alt", "n_intervals", "n_masked_bases"]
NAME_REFUSAL = "the variant mask should be a file whose name ends in .vcf, .vcf.gz or .bed"


class MaskError(Exception):
    def __init__(self, line, what):
        super().__init__("variant mask line %d: %s" % (line, what))
        self.line = line


def clamp_lens(lens, refs):
    """per contig min(header length, FASTA length); -1 for a contig the FASTA lacks"""
    return [-1 if r is None else min(ln, len(r)) for ln, r in zip(lens, refs)]


def merge(raw, clamp):
    """intervals [(tid, start, end)] clamped to [0, clamp[tid]), sorted, merged where they overlap or abut"""
    v = sorted((t, max(a, 0), min(z, clamp[t])) for t, a, z in raw if max(a, 0) < min(z, clamp[t]))
    out = []
    for t, a, z in v:
        if out and out[-1][0] == t and a <= out[-1][2]:
            out[-1] = (t, out[-1][1], max(out[-1][2], z))
        else:
            out.append((t, a, z))
    return out


def result(raw, clamp, **counters):
    iv = merge(raw, clamp)
    res = dict(n_lines=0, n_records=0, n_unknown_contig=0, n_no_alt=0)
    res.update(counters, intervals=iv, n_intervals=len(iv), n_masked_bases=sum(z - a for _, a, z in iv))
    return res


def parse_vcf(text, names, clamp):
    """rule K: VCF text (bytes) -> dict(COUNTERS, intervals); MaskError names the first malformed line, counting from 1"""
    by_name = {nm: t for t, nm in enumerate(names)}                  # (the last of a repeated name)
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    raw, n_records, n_unknown, n_no_alt = [], 0, 0, 0
    for n, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line == b"" or line.startswith(b"#"):
            continue
        f = line.split(b"\t")
        if len(f) < 5:
            raise MaskError(n, "fewer than five tab-separated fields")
        if not f[1] or any(c not in b"0123456789" for c in f[1]) or int(f[1]) < 1:
            raise MaskError(n, "POS is not a decimal integer >= 1")
        if f[3] == b"":
            raise MaskError(n, "REF is empty")
        n_records += 1
        t = by_name.get(f[0].decode("latin-1"))
        if t is None:
            n_unknown += 1
        elif f[4] in (b".", b"<NON_REF>", b"<*>"):
            n_no_alt += 1
        else:
            raw.append((t, int(f[1]) - 1, int(f[1]) - 1 + len(f[3])))
    return result(raw, clamp, n_lines=len(lines), n_records=n_records, n_unknown_contig=n_unknown, n_no_alt=n_no_alt)


def load(path, names, clamp):
    """rule K for a file, by the ending of its name"""
    path = str(path)
    if path.endswith(".vcf.gz"):
        with gzip.open(path, "rb") as f:
            return parse_vcf(f.read(), names, clamp)
    if path.endswith(".vcf"):
        with open(path, "rb") as f:
            return parse_vcf(f.read(), names, clamp)
    if path.endswith(".bed"):
        regions = pyerrprof.read_bed(path, names)
        return result([r for r in regions if r[0] >= 0], clamp, n_records=len(regions), n_unknown_contig=sum(1 for r in regions if r[0] < 0))
    raise ValueError(NAME_REFUSAL)


def complement(iv, lens):
    """the positions of [0, lens[t]) of every contig that no interval of iv holds, as regions"""
    out = []
    for t, ln in enumerate(lens):
        x = 0
        for _, a, z in [i for i in iv if i[0] == t]:
            if x < a:
                out.append((t, x, a))
            x = z
        if x < ln:
            out.append((t, x, ln))
    return out


def tester(iv):
    """(tid, x) -> x lies in an interval of iv (disjoint, in order)"""
    ends = [(t, z) for t, a, z in iv]

    def inside(t, x):
        j = bisect.bisect_right(ends, (t, x))
        return j < len(iv) and iv[j][0] == t and iv[j][1] <= x
    return inside


def masked_at(inside, refs, t, x):
    """rule Y's test of an anchor: outside [0, FASTA length) nothing is masked"""
    return 0 <= x < len(refs[t]) and inside(t, x)


def totals(res):
    counts = res["counts"]
    res["n_bases"] = sum(sum(row[:16]) for seg in counts for row in seg)
    res["n_mismatches"] = sum(row[4 * r + b] for seg in counts for row in seg for r in range(4) for b in range(4) if r != b)
    res["n_masked_events"] = sum(row[MASKED] for seg in counts for row in seg)
    return res


def profile(records, refs, lens, mask, regions=None, min_mapq=0, min_baseq=0, exclude=0x704):
    """pyerrprof.profile under rule Y.  mask: rule K's intervals -> pyerrprof.profile's dict, with class 21 counted and n_masked_events"""
    target = None
    n_intervals = -1
    if regions is not None:
        iv, _ = pypileup.intervals(regions, lens)
        n_intervals = len(iv)
        target = tester([(t, a, z) for t, a, z, _ in iv])
    inside = tester(mask)
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(pyerrprof.fields(r))
        except pyerrprof.Malformed as e:
            raise ErrprofError("BAM record %d (counting from 0): %s" % (k, e), k)
    counts = [[[0] * pyerrprof.ROW for _ in range(pyerrprof.MAX_CYCLE)] for _ in range(3)]
    res = dict(n_records=len(records), n_eligible=0, n_intervals=n_intervals)
    res.update({k: 0 for k in pyerrprof.SKIPS})
    for f in parsed:
        sk = pyerrprof.skip_of(f, refs, min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        res["n_eligible"] += 1
        for x, g, cy, c in pyerrprof.walk(f, refs[f["tid"]], min_baseq):
            if target is None or target(f["tid"], x):                # rule B first: an event off the targets is not counted at all
                counts[g][cy - 1][MASKED if masked_at(inside, refs, f["tid"], x) else c] += 1
    res["counts"] = counts
    return totals(res)


def profile_fragments(records, refs, lens, mask, regions=None, min_mapq=0, min_baseq=0, exclude=0x704):
    """pyfragerr.profile_fragments under rule Y: at a shared masked column the mate rule V' counts adds MASKED to counts, both add class 21 to
    overlap; the pairs, the shared and the disagreeing columns are what they are without a mask"""
    iv, target, n_intervals = None, (lambda t, x: True), -1
    if regions is not None:
        iv, _ = pypileup.intervals(regions, lens)
        n_intervals = len(iv)
        target = tester([(t, a, z) for t, a, z, _ in iv])
    inside = tester(mask)
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(pypileup.fields(r))
        except pypileup.Malformed as e:
            raise ErrprofError("BAM record %d (counting from 0): %s" % (k, e), k)
    for k in range(1, len(parsed)):
        if pyfragpile.order_key(parsed[k]["tid"], parsed[k]["pos"]) < pyfragpile.order_key(parsed[k - 1]["tid"], parsed[k - 1]["pos"]):
            raise ErrprofError("BAM record %d (counting from 0) lies in front of its predecessor: %s needs a coordinate-sorted file" % (k, pyfragerr.WHO), k)
    counts = [[[0] * pyerrprof.ROW for _ in range(pyerrprof.MAX_CYCLE)] for _ in range(3)]
    ovl = [[[0] * pyerrprof.ROW for _ in range(pyerrprof.MAX_CYCLE)] for _ in range(3)]
    res = dict(n_records=len(records), n_eligible=0, n_intervals=n_intervals)
    res.update({k: 0 for k in pyerrprof.SKIPS + pyfragerr.FRAG_COUNTERS})
    groups, eligible = {}, []
    for k, (f, r) in enumerate(zip(parsed, records)):
        sk = pyerrprof.skip_of(f, refs, min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        res["n_eligible"] += 1
        eligible.append(k)
        if pyfragerr.is_candidate(f, r, iv):
            _, npos, name = pyfragpile.mate_fields(r)
            groups.setdefault((name, f["tid"], min(f["pos"], npos), max(f["pos"], npos)), []).append(k)
    partner = {}
    for g in groups.values():
        if len(g) > 2:
            res["n_ambiguous"] += len(g)
        elif len(g) == 2:
            a, b = g
            fa, fb = parsed[a]["flag"], parsed[b]["flag"]
            if bool(fa & 0x40) != bool(fb & 0x40) and pyfragpile.mate_fields(records[a])[1] == parsed[b]["pos"] and pyfragpile.mate_fields(records[b])[1] == parsed[a]["pos"]:
                partner[a], partner[b] = b, a
                res["n_pairs"] += 1
    for k in eligible:
        f = parsed[k]
        ref = refs[f["tid"]]
        ref = ref.encode() if isinstance(ref, str) else ref
        o = parsed[partner[k]] if k in partner else None
        who = int(o is not None and partner[k] < k)
        rev, has_q = bool(f["flag"] & 16), f["qual"][0] != 0xFF
        for x, g, cy, c in pyerrprof.walk(f, ref, min_baseq):
            if not target(f["tid"], x):
                continue
            mk = masked_at(inside, refs, f["tid"], x)
            there = pyfragerr.base_at(o, x) if o is not None and c not in (INS, DEL) else None
            if there is None:
                counts[g][cy - 1][MASKED if mk else c] += 1
                continue
            (bm, qm), (bo, qo) = pyfragerr.base_at(f, x), there
            r = pyfragerr.ref_class(ref, x)
            ovl[g][cy - 1][MASKED if mk else pyfragerr.rule_x(bm, qm, has_q, bo, qo, o["qual"][0] != 0xFF, r, rev, min_baseq)] += 1
            (ca, qa), (cb, qb) = ((bm, qm), (bo, qo)) if who == 0 else ((bo, qo), (bm, qm))
            w, q, differ = pyfragpile.rule_v(ca, qa, cb, qb)
            if who == 1:
                res["n_shared_columns"] += 1
                res["n_disagree_columns"] += int(differ)
            if w != who:
                continue
            if mk:
                c = MASKED
            elif has_q and q < min_baseq:
                c = LOWQ
            elif r < 0:
                c = REF_OTHER
            elif bm > 3:
                c = READ_N
            else:
                c = 4 * (3 - r) + (3 - bm) if rev else 4 * r + bm
            counts[g][cy - 1][c] += 1
    res["counts"], res["overlap"] = counts, ovl
    return totals(res)


def nonzero(res, key="counts", names=CLASSES):
    """{(segment, cycle, class name): count} of the counters of classes 0..21 that are not zero"""
    return {(g, cy + 1, names[c]): v for g, seg in enumerate(res[key]) for cy, row in enumerate(seg) for c, v in enumerate(row[:22]) if v}


def nonzero_overlap(res):
    return nonzero(res, "overlap", OVL_CLASSES)


def _table(block, header, n_sum):
    out = [header]
    for g, seg in enumerate(block):
        last = max([cy + 1 for cy, row in enumerate(seg) if any(row)] or [0])
        for cy in range(1, last + 1):
            k = seg[cy - 1]
            mism = sum(k[4 * r + b] for r in range(4) for b in range(4) if r != b)
            out.append("%d\t%d\t%d\t%d\t%s\n" % (g, cy, sum(k[:n_sum]), mism, "\t".join(str(v) for v in k[:22])))
    return "".join(out).encode()


def table(res):
    """rule O with a mask: the primary table's bytes, MASKED as its last column"""
    return _table(res["counts"], HEADER, 16)


def overlap_table(res):
    return _table(res["overlap"], OVL_HEADER, 19)
