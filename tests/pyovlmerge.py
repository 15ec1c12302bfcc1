"""The model of gce_bam_merge_overlap's rules: the premise (rule P), eligibility (rule E), mates (rule M) and the rewrite of the
QUAL bytes (rule Q), over pyfragpile and pypileup, which it imports and leaves alone.  Plain Python over whole BAM records (bytes, block_size
first), the whole file at once.  The kernels of gencore_amd/csrc/gce_ovlmerge.hpp reproduce its bytes and counters exactly; tests/ovlcases.py
holds records whose new QUAL bytes are written out by hand."""
import pyfragpile
import pypileup
from pypileup import PileupError

COUNTERS = ["n_records", "n_pairs", "n_pairs_no_qual", "n_ambiguous", "n_shared_columns", "n_disagree_columns", "n_columns_skipped", "n_records_changed"]
Q_MAX = 93
WHO = "gce_bam_merge_overlap"


def qual_offset(r):
    """the first QUAL byte of a whole record"""
    f = pypileup.fields(r)
    return 36 + r[12] + 4 * len(f["cigar"]) + (f["lseq"] + 1) // 2


def base_columns(f):
    """{x: query offset} over the M / = / X columns of a record"""
    x, q, out = f["pos"], 0, {}
    for op, n in f["cigar"]:
        if op in (0, 7, 8):
            for k in range(n):
                out[x + k] = q + k
            x += n
            q += n
        elif op in (2, 3):
            x += n
        elif op in (1, 4):
            q += n
    return out


def rule_q(ca, qa, cb, qb):
    """-> (qa', qb', kind): kind 0 the column is left as it is, 1 the classes agree, 2 they do not"""
    if qa == 0 or qb == 0 or qa > Q_MAX or qb > Q_MAX:
        return qa, qb, 0
    if ca == cb:
        return min(qa + qb, Q_MAX), 0, 1
    if qa >= qb:
        return (4 * qa) // 5, 0, 2
    return 0, (4 * qb) // 5, 2


def find_pairs(records, min_mapq=0, exclude=0x704):
    """rules E and M over the whole file -> (parsed fields, [(a, b)] with a < b, the number of ambiguous candidates); PileupError names the
    lowest malformed record, else the first record that lies in front of its predecessor"""
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(pypileup.fields(r))
        except pypileup.Malformed:
            raise PileupError("BAM record %d (counting from 0): its fields overrun its block_size" % k, k)
    for k in range(1, len(parsed)):
        if pyfragpile.order_key(parsed[k]["tid"], parsed[k]["pos"]) < pyfragpile.order_key(parsed[k - 1]["tid"], parsed[k - 1]["pos"]):
            raise PileupError("BAM record %d (counting from 0) lies in front of its predecessor: %s needs a coordinate-sorted file" % (k, WHO), k)
    groups = {}
    for k, (f, r) in enumerate(zip(parsed, records)):
        if pypileup.skip_of(f, 1 << 31, min_mapq, exclude):
            continue
        if pyfragpile.is_candidate(f, r, [(f["tid"], -1, 1 << 40, 0)]):                  # (no site test: one interval that every record touches)
            _, npos, name = pyfragpile.mate_fields(r)
            groups.setdefault((name, f["tid"], min(f["pos"], npos), max(f["pos"], npos)), []).append(k)
    pairs, ambiguous = [], 0
    for g in groups.values():
        if len(g) > 2:
            ambiguous += len(g)
        elif len(g) == 2:
            a, b = g
            fa, fb = parsed[a]["flag"], parsed[b]["flag"]
            if bool(fa & 0x40) != bool(fb & 0x40) and pyfragpile.mate_fields(records[a])[1] == parsed[b]["pos"] and pyfragpile.mate_fields(records[b])[1] == parsed[a]["pos"]:
                pairs.append((a, b))
    return parsed, sorted(pairs), ambiguous


def merge_overlap(records, min_mapq=0, exclude=0x704):
    """records: whole BAM records (bytes) in file order -> (the rewritten records, the counters)"""
    parsed, pairs, ambiguous = find_pairs(records, min_mapq, exclude)
    out = [bytearray(r) for r in records]
    res = {k: 0 for k in COUNTERS}
    res.update(n_records=len(records), n_pairs=len(pairs), n_ambiguous=ambiguous)
    for a, b in pairs:
        fa, fb = parsed[a], parsed[b]
        if fa["qual"][0] == 0xFF or fb["qual"][0] == 0xFF:
            res["n_pairs_no_qual"] += 1
            continue
        ya, yb = base_columns(fa), base_columns(fb)
        ca, cb = pyfragpile.columns(fa), pyfragpile.columns(fb)
        oa, ob = qual_offset(records[a]), qual_offset(records[b])
        for x in sorted(set(ya) & set(yb)):
            qa, qb = out[a][oa + ya[x]], out[b][ob + yb[x]]
            assert (ca[x][1], cb[x][1]) == (qa, qb)
            na, nb, kind = rule_q(ca[x][0], qa, cb[x][0], qb)
            res["n_shared_columns"] += 1
            res["n_disagree_columns"] += kind == 2
            res["n_columns_skipped"] += kind == 0
            out[a][oa + ya[x]], out[b][ob + yb[x]] = na, nb
    out = [bytes(r) for r in out]
    res["n_records_changed"] = sum(1 for r, w in zip(records, out) if r != w)
    return out, res
