"""The model of gce_bam_error_profile_fragments' rules: the shared columns (rule V') and the overlap table (rule X), over
pyerrprof's rules E, G, C, W, B and O and pyfragpile's rules P and M, which it imports and leaves alone.  Plain Python over whole BAM records
(bytes, block_size first), the whole file at once: the result does not know of windows, and the partner's base at a column comes from a
fresh walk of its CIGAR for every column, so nothing here resembles the kernels' cursor.  The kernels of gencore_amd/csrc/gce_fragerr.hpp
reproduce its integers exactly; tests/fragerrcases.py holds records whose counters are written out by hand."""
import bisect

import pyerrprof
import pyfragpile
import pypileup
from pyerrprof import DEL, INS, LOWQ, READ_N, REF_OTHER, ErrprofError

OVL_CLASSES = pyerrprof.CLASSES[:16] + ["AGREE_REF", "AGREE_ALT", "DIFF_OTHER", "UNUSABLE", "LOWQ"]
AGREE_REF, AGREE_ALT, DIFF_OTHER, UNUSABLE, OVL_LOWQ = 16, 17, 18, 19, 20
OVL_HEADER = "#segment\tcycle\tshared\terrors\t" + "\t".join(OVL_CLASSES) + "\n"
FRAG_COUNTERS = pyfragpile.FRAG_COUNTERS
WHO = "gce_bam_error_profile_fragments"


def base_at(f, x):
    """the base class (0..3 = A C G T, 4 = N) and the quality (0 for a record without qualities) of record f at reference position x, or
    None when no M / = / X op of it covers x: one walk of the CIGAR from its first op"""
    x0, q0 = f["pos"], 0
    for op, n in f["cigar"]:
        if op in (0, 7, 8):
            if x0 <= x < x0 + n:
                y = q0 + (x - x0)
                nib = (f["seq"][y >> 1] >> (0 if y & 1 else 4)) & 15
                return {1: 0, 2: 1, 4: 2, 8: 3}.get(nib, 4), (f["qual"][y] if f["qual"][0] != 0xFF else 0)
            x0 += n
            q0 += n
        elif op in (2, 3):
            if x0 <= x < x0 + n:
                return None
            x0 += n
        elif op in (1, 4):
            q0 += n
    return None


def touches(f, iv):
    """errprof::scan_record's `first` is not none: an interval of the record's contig ends at or behind pos and starts at or in front of
    pos + rlen; no BED: every eligible record"""
    if iv is None:
        return True
    return any(t == f["tid"] and z >= f["pos"] and a <= f["pos"] + pyfragpile.rlen_of(f) for t, a, z, _ in iv)


def is_candidate(f, r, iv):
    """rule M for an eligible record, with this pass's reading of `can touch a site`"""
    ntid, npos, _ = pyfragpile.mate_fields(r)
    fl = f["flag"]
    if not touches(f, iv):
        return False
    if not fl & 0x1 or fl & (0x4 | 0x8 | 0x100 | 0x800) or bool(fl & 0x40) == bool(fl & 0x80):
        return False
    if ntid != f["tid"]:
        return False
    return not (npos >= f["pos"] and npos >= f["pos"] + pyfragpile.rlen_of(f))


def ref_class(ref, x):
    return "ACGT".find(chr(ref[x]).upper()) if x < len(ref) else -1


def rule_x(bm, qm, m_has_q, bo, qo, o_has_q, r, rev, min_baseq):
    """the overlap table's class of mate m at a shared column: the first condition that applies"""
    if (m_has_q and qm < min_baseq) or (o_has_q and qo < min_baseq):
        return OVL_LOWQ
    if bm > 3 or bo > 3 or r < 0:
        return UNUSABLE
    if bm == bo:
        return AGREE_REF if bm == r else AGREE_ALT
    if bo == r or bm == r:
        return 4 * (3 - r) + (3 - bm) if rev else 4 * r + bm
    return DIFF_OTHER


def profile_fragments(records, refs, lens, regions=None, min_mapq=0, min_baseq=0, exclude=0x704):
    """records: whole BAM records (bytes) in file order -> pyerrprof.profile's dict plus overlap ([3][1024][24]), n_pairs, n_shared_columns,
    n_disagree_columns and n_ambiguous; ErrprofError names the lowest malformed record, else the first record that lies in front of its
    predecessor"""
    iv, target, n_intervals = None, (lambda t, x: True), -1
    if regions is not None:
        iv, _ = pypileup.intervals(regions, lens)
        n_intervals = len(iv)
        ends = [(it, z) for it, a, z, _ in iv]

        def target(t, x):
            j = bisect.bisect_right(ends, (t, x))
            return j < len(iv) and iv[j][0] == t and iv[j][1] <= x
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(pypileup.fields(r))
        except pypileup.Malformed as e:
            raise ErrprofError("BAM record %d (counting from 0): %s" % (k, e), k)
    for k in range(1, len(parsed)):
        if pyfragpile.order_key(parsed[k]["tid"], parsed[k]["pos"]) < pyfragpile.order_key(parsed[k - 1]["tid"], parsed[k - 1]["pos"]):
            raise ErrprofError("BAM record %d (counting from 0) lies in front of its predecessor: %s needs a coordinate-sorted file" % (k, WHO), k)
    counts = [[[0] * pyerrprof.ROW for _ in range(pyerrprof.MAX_CYCLE)] for _ in range(3)]
    ovl = [[[0] * pyerrprof.ROW for _ in range(pyerrprof.MAX_CYCLE)] for _ in range(3)]
    res = dict(n_records=len(records), n_eligible=0, n_intervals=n_intervals)
    res.update({k: 0 for k in pyerrprof.SKIPS + FRAG_COUNTERS})
    groups, eligible = {}, []
    for k, (f, r) in enumerate(zip(parsed, records)):
        sk = pyerrprof.skip_of(f, refs, min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        res["n_eligible"] += 1
        eligible.append(k)
        if is_candidate(f, r, iv):
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
        who = int(o is not None and partner[k] < k)                  # 0: this record is a, the earlier in the file; 1: it is b
        rev, has_q = bool(f["flag"] & 16), f["qual"][0] != 0xFF
        for x, g, cy, c in pyerrprof.walk(f, ref, min_baseq):
            if not target(f["tid"], x):
                continue
            there = base_at(o, x) if o is not None and c not in (INS, DEL) else None
            if there is None:
                counts[g][cy - 1][c] += 1                            # rule W: no partner, an insertion, a deletion, or a column the partner does not cover
                continue
            (bm, qm), (bo, qo) = base_at(f, x), there
            r = ref_class(ref, x)
            ovl[g][cy - 1][rule_x(bm, qm, has_q, bo, qo, o["qual"][0] != 0xFF, r, rev, min_baseq)] += 1
            (ca, qa), (cb, qb) = ((bm, qm), (bo, qo)) if who == 0 else ((bo, qo), (bm, qm))
            w, q, differ = pyfragpile.rule_v(ca, qa, cb, qb)
            if who == 1:
                res["n_shared_columns"] += 1
                res["n_disagree_columns"] += int(differ)
            if w != who:
                continue
            if has_q and q < min_baseq:
                c = LOWQ
            elif r < 0:
                c = REF_OTHER
            elif bm > 3:
                c = READ_N
            else:
                c = 4 * (3 - r) + (3 - bm) if rev else 4 * r + bm
            counts[g][cy - 1][c] += 1
    res["counts"], res["overlap"] = counts, ovl
    res["n_bases"] = sum(sum(row[:16]) for seg in counts for row in seg)
    res["n_mismatches"] = sum(row[4 * r + b] for seg in counts for row in seg for r in range(4) for b in range(4) if r != b)
    return res


def nonzero_overlap(res):
    """{(segment, cycle, class name): count} of the overlap table's counters that are not zero"""
    return {(g, cy + 1, OVL_CLASSES[c]): v for g, seg in enumerate(res["overlap"]) for cy, row in enumerate(seg) for c, v in enumerate(row[:21]) if v}


def overlap_sum(res):
    return sum(sum(row) for seg in res["overlap"] for row in seg)


def overlap_table(res):
    """rule O for the overlap table: its bytes"""
    out = [OVL_HEADER]
    for g, seg in enumerate(res["overlap"]):
        last = max([cy + 1 for cy, row in enumerate(seg) if any(row)] or [0])
        for cy in range(1, last + 1):
            k = seg[cy - 1]
            err = sum(k[4 * r + b] for r in range(4) for b in range(4) if r != b)
            out.append("%d\t%d\t%d\t%d\t%s\n" % (g, cy, sum(k[:19]), err, "\t".join(str(v) for v in k[:21])))
    return "".join(out).encode()
