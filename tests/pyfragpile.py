"""The model of gce_bam_pileup_fragments' rules: the premise (rule P), mates (rule M) and the shared columns (rule V), over
pypileup's rules S, E, W and O, which it imports and leaves alone.  Plain Python over whole BAM records (bytes, block_size first), the whole
file at once: the result does not know of windows.  The kernels of gencore_amd/csrc/gce_fragpile.hpp reproduce its integers exactly;
tests/fragcases.py holds records whose counters are written out by hand."""
import struct

import pypileup
from pypileup import PileupError

FRAG_COUNTERS = ["n_pairs", "n_shared_columns", "n_disagree_columns", "n_ambiguous"]
DEL = 5
Q_CAP = 200


def mate_fields(r):
    """next_refID, next_pos and the name's bytes (with its NUL: l_read_name of them) of a whole record"""
    lq = r[12]
    ntid, npos = struct.unpack_from("<ii", r, 24)
    return ntid, npos, bytes(r[36:36 + lq])


def order_key(tid, pos):
    """rule P: placed records by (tid, pos), every record with tid < 0 behind them"""
    return (1, 0, 0) if tid < 0 else (0, tid, pos)


def rlen_of(f):
    return sum(n for op, n in f["cigar"] if op in (0, 2, 3, 7, 8))


def touches(f, iv):
    """the scan's `first` is not none: an interval of the record's contig ends at or behind pos and starts in front of pos + rlen"""
    for t, a, z, _ in iv:
        if t == f["tid"] and z >= f["pos"] and a < f["pos"] + rlen_of(f):
            return True
    return False


def is_candidate(f, r, iv):
    """rule M for an eligible record"""
    ntid, npos, _ = mate_fields(r)
    fl = f["flag"]
    if not touches(f, iv):
        return False
    if not fl & 0x1 or fl & (0x4 | 0x8 | 0x100 | 0x800) or bool(fl & 0x40) == bool(fl & 0x80):
        return False
    if ntid != f["tid"]:
        return False
    return not (npos >= f["pos"] and npos >= f["pos"] + rlen_of(f))


def columns(f):
    """{x: (raw class, quality)} over the M / = / X / D columns of a record: the class without the LOWQ test, quality 0 for a D column or a
    record without qualities"""
    x, q, out = f["pos"], 0, {}
    has_q = f["qual"][0] != 0xFF
    for op, n in f["cigar"]:
        if op in (0, 7, 8):
            for k in range(n):
                y = q + k
                nib = (f["seq"][y >> 1] >> (0 if y & 1 else 4)) & 15
                out[x + k] = ({1: 0, 2: 1, 4: 2, 8: 3}.get(nib, 4), f["qual"][y] if has_q else 0)
            x += n
            q += n
        elif op == 2:
            for k in range(n):
                out[x + k] = (DEL, 0)
            x += n
        elif op == 3:
            x += n
        elif op in (1, 4):
            q += n
    return out


def rule_v(ca, qa, cb, qb):
    """-> (0 for a or 1 for b, the winner's adjusted quality, whether the classes differ)"""
    if ca == cb:
        return 0, min(qa + qb, Q_CAP), False
    if qa >= qb:
        return 0, (4 * qa) // 5, True
    return 1, (4 * qb) // 5, True


def paired_adds(fa, fb, min_baseq):
    """every add of the pair (a: the earlier in the file) as (pos, strand, class) whether or not pos is a site, and the shared columns as
    [(pos, differ)]"""
    cols = [columns(fa), columns(fb)]
    shared = sorted(set(cols[0]) & set(cols[1]))
    adds, decided = [], []
    for who, f in enumerate((fa, fb)):
        for x, s, c in pypileup.walk(f, min_baseq):
            if c == 6 or x not in cols[1 - who]:
                adds.append((x, s, c))                          # rule W: an insertion, or a column the other mate does not cover
    for x in shared:
        (ca, qa), (cb, qb) = cols[0][x], cols[1][x]
        w, q, differ = rule_v(ca, qa, cb, qb)
        f = (fa, fb)[w]
        c = (ca, cb)[w]
        if c != DEL and f["qual"][0] != 0xFF and q < min_baseq:
            c = 7
        adds.append((x, (f["flag"] >> 4) & 1, c))
        decided.append((x, differ))
    return adds, decided


def pileup_fragments(records, regions, lens, min_mapq=0, min_baseq=0, exclude=0x704):
    """records: whole BAM records (bytes) in file order -> pypileup.pileup's dict plus n_pairs, n_shared_columns, n_disagree_columns and
    n_ambiguous; PileupError names the lowest malformed record, else the first record that lies in front of its predecessor"""
    iv, n_sites = pypileup.intervals(regions, lens)
    index, tid, pos = {}, [], []
    for t, a, z, s0 in iv:
        for x in range(a, z):
            index[t, x] = s0 + (x - a)
            tid.append(t)
            pos.append(x)
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(pypileup.fields(r))
        except pypileup.Malformed as e:
            raise PileupError("BAM record %d (counting from 0): %s" % (k, e), k)
    for k in range(1, len(parsed)):
        if order_key(parsed[k]["tid"], parsed[k]["pos"]) < order_key(parsed[k - 1]["tid"], parsed[k - 1]["pos"]):
            raise PileupError("BAM record %d (counting from 0) lies in front of its predecessor: gce_bam_pileup_fragments needs a coordinate-sorted file" % k, k)
    counts = [[0] * 16 for _ in range(n_sites)]
    res = dict(n_records=len(records), n_eligible=0, n_sites=n_sites, n_intervals=len(iv))
    res.update({k: 0 for k in pypileup.SKIPS + FRAG_COUNTERS})
    groups, eligible = {}, []
    for k, (f, r) in enumerate(zip(parsed, records)):
        sk = pypileup.skip_of(f, len(lens), min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        res["n_eligible"] += 1
        eligible.append(k)
        if is_candidate(f, r, iv):
            _, npos, name = mate_fields(r)
            groups.setdefault((name, f["tid"], min(f["pos"], npos), max(f["pos"], npos)), []).append(k)
    partner = {}
    for g in groups.values():
        if len(g) > 2:
            res["n_ambiguous"] += len(g)
        elif len(g) == 2:
            a, b = g
            fa, fb = parsed[a]["flag"], parsed[b]["flag"]
            if bool(fa & 0x40) != bool(fb & 0x40) and mate_fields(records[a])[1] == parsed[b]["pos"] and mate_fields(records[b])[1] == parsed[a]["pos"]:
                partner[a], partner[b] = b, a

    def add(t, x, s, c):
        i = index.get((t, x))
        if i is not None:
            counts[i][s * 8 + c] += 1
    for k in eligible:
        f = parsed[k]
        if k not in partner:
            for x, s, c in pypileup.walk(f, min_baseq):
                add(f["tid"], x, s, c)
        elif partner[k] > k:
            adds, decided = paired_adds(f, parsed[partner[k]], min_baseq)
            for x, s, c in adds:
                add(f["tid"], x, s, c)
            res["n_pairs"] += 1
            for x, differ in decided:
                if (f["tid"], x) in index:
                    res["n_shared_columns"] += 1
                    res["n_disagree_columns"] += int(differ)
    res.update(tid=tid, pos=pos, counts=counts)
    return res


def read_raw_records(path):
    """a BAM file as (contig names, lengths, whole records as bytes, block_size first)"""
    import zlib
    raw, stream = open(path, "rb").read(), b""
    while raw:
        d = zlib.decompressobj(31)
        stream += d.decompress(raw)
        raw = d.unused_data
    assert stream[:4] == b"BAM\1"
    (lt,) = struct.unpack_from("<i", stream, 4)
    p = 8 + lt
    (n_ref,) = struct.unpack_from("<i", stream, p)
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", stream, p)
        names.append(stream[p + 4:p + 4 + ln - 1].decode())
        lens.append(struct.unpack_from("<I", stream, p + 4 + ln)[0])
        p += 8 + ln
    recs = []
    while p < len(stream):
        (bs,) = struct.unpack_from("<I", stream, p)
        recs.append(stream[p:p + 4 + bs])
        p += 4 + bs
    return names, lens, recs
