"""The model of gce_bam_pileup's rules: sites (rule S), eligible records (rule E), the walk (rule W) and the table (rule O),
in plain Python over whole BAM records (bytes, block_size first).  The kernels of gencore_amd/csrc/gce_pileup.hpp reproduce its integers
exactly; tests/pileupcases.py holds records whose counters are written out by hand."""
import struct

CLASSES = ["A", "C", "G", "T", "N", "DEL", "INS", "LOWQ"]
SKIPS = ["n_unplaced", "n_flagged", "n_low_mapq", "n_no_cigar", "n_no_seq", "n_bad_cigar"]
MAX_SITES = 1 << 28
HEADER = "#contig\tpos\tref\tdepth\t" + "\t".join("%s_%s" % (s, c) for s in ("fwd", "rev") for c in CLASSES) + "\n"


class Malformed(Exception):
    """block_size < 32, or fields that overrun block_size"""


class PileupError(Exception):
    def __init__(self, msg, record=None):
        super().__init__(msg)
        self.record = record


def intervals(regions, lens):
    """rule S: regions = [(tid, start, end)] as gce_bed_load gives them -> [(tid, start, end, site0)] and the number of sites"""
    v = []
    for tid, a, z in regions:
        if tid < 0 or tid >= len(lens):
            continue
        a, z = max(a, 0), min(z, lens[tid])
        if a < z:
            v.append((tid, a, z))
    v.sort()
    out = []
    for tid, a, z in v:
        if out and out[-1][0] == tid and a <= out[-1][2]:
            out[-1][2] = max(out[-1][2], z)
        else:
            out.append([tid, a, z])
    n, res = 0, []
    for tid, a, z in out:
        res.append((tid, a, z, n))
        n += z - a
    if n > MAX_SITES:
        raise PileupError("more than 2^28 sites")
    return res, n


def fields(r):
    (bs,) = struct.unpack_from("<I", r, 0)
    if bs < 32 or 4 + bs > len(r):
        raise Malformed("block_size")
    tid, pos, lq, mapq, _bin, nc, flag, lseq = struct.unpack_from("<iiBBHHHi", r, 4)
    if lseq < 0 or 32 + lq + 4 * nc + (lseq + 1) // 2 + lseq > bs:
        raise Malformed("fields overrun block_size")
    p = 36 + lq
    cig = struct.unpack_from("<%dI" % nc, r, p)
    p += 4 * nc
    seq = r[p:p + (lseq + 1) // 2]
    qual = r[p + (lseq + 1) // 2:p + (lseq + 1) // 2 + lseq]
    return dict(tid=tid, pos=pos, mapq=mapq, flag=flag, lseq=lseq, cigar=[(w & 15, w >> 4) for w in cig], seq=seq, qual=qual)


def fields_of_pybam(g):
    """the same dict from a record as tests/pybam.py's read_bam returns it"""
    code = "=ACMGRSVTWYHKDBN"
    nib = [code.index(c) for c in g["seq"]] + [0]
    return dict(tid=g["tid"], pos=g["pos"], mapq=g["mapq"], flag=g["flag"], lseq=len(g["seq"]), cigar=[(w & 15, w >> 4) for w in g["cigar"]],
                seq=bytes(nib[2 * k] << 4 | nib[2 * k + 1] for k in range((len(g["seq"]) + 1) // 2)), qual=bytes(g["qual"]))


def skip_of(f, n_ref, min_mapq, exclude):
    """rule E: None for an eligible record, else the one counter it goes to"""
    if not (0 <= f["tid"] < n_ref) or f["pos"] < 0:
        return "n_unplaced"
    if f["flag"] & exclude:
        return "n_flagged"
    if f["mapq"] < min_mapq:
        return "n_low_mapq"
    if not f["cigar"]:
        return "n_no_cigar"
    if f["lseq"] == 0:
        return "n_no_seq"
    if any(op > 8 for op, _ in f["cigar"]) or sum(n for op, n in f["cigar"] if op in (0, 1, 4, 7, 8)) != f["lseq"]:
        return "n_bad_cigar"
    return None


def walk(f, min_baseq):
    """rule W: every add of an eligible record as (pos, strand, class), whether or not pos is a site"""
    x, q, s = f["pos"], 0, (f["flag"] >> 4) & 1
    has_q = f["qual"][0] != 0xFF
    seen = False
    for op, n in f["cigar"]:
        if op in (0, 7, 8):
            for k in range(n):
                y = q + k
                nib = (f["seq"][y >> 1] >> (0 if y & 1 else 4)) & 15
                c = {1: 0, 2: 1, 4: 2, 8: 3}.get(nib, 4)
                if has_q and f["qual"][y] < min_baseq:
                    c = 7
                yield x + k, s, c
            x += n
            q += n
            seen = True
        elif op == 2:
            for k in range(n):
                yield x + k, s, 5
            x += n
            seen = True
        elif op == 3:
            x += n
        elif op == 1:
            if seen:
                yield x - 1, s, 6
            q += n
        elif op == 4:
            q += n


def pileup(records, regions, lens, min_mapq=0, min_baseq=0, exclude=0x704):
    """records: whole BAM records (bytes), or dicts of tests/pybam.py's read_bam
    -> dict(tid, pos, counts ([n_sites][16]), n_records, n_eligible, the six skip counters, n_sites, n_intervals); PileupError names the
    lowest malformed record"""
    iv, n_sites = intervals(regions, lens)
    index, tid, pos = {}, [], []
    for t, a, z, s0 in iv:
        for x in range(a, z):
            index[t, x] = s0 + (x - a)
            tid.append(t)
            pos.append(x)
    parsed = []
    for k, r in enumerate(records):
        try:
            parsed.append(fields_of_pybam(r) if isinstance(r, dict) else fields(r))
        except Malformed as e:
            raise PileupError("BAM record %d (counting from 0): %s" % (k, e), k)
    counts = [[0] * 16 for _ in range(n_sites)]
    res = dict(n_records=len(records), n_eligible=0, n_sites=n_sites, n_intervals=len(iv))
    res.update({k: 0 for k in SKIPS})
    ops = 0
    for f in parsed:
        sk = skip_of(f, len(lens), min_mapq, exclude)
        if sk:
            res[sk] += 1
            continue
        res["n_eligible"] += 1
        ops += len(f["cigar"])
        for x, s, c in walk(f, min_baseq):
            i = index.get((f["tid"], x))
            if i is not None:
                counts[i][s * 8 + c] += 1
    if ops >= 1 << 32:
        raise PileupError("2^32 CIGAR operations or more")
    res.update(tid=tid, pos=pos, counts=counts)
    return res


def read_fasta(path):
    """contigs by the header up to its first blank, upper case (clean files only: the loader's quirks are not modelled)"""
    out, name = {}, None
    for line in open(path).read().split("\n"):
        if line.startswith(">"):
            name = line[1:].split(" ")[0]
            out[name] = []
        elif name is not None:
            out[name].append(line.strip().upper())
    return {k: "".join(v) for k, v in out.items()}


def read_bed(path, names):
    """(tid, start, end) per line of three or more tab-separated fields, `#` lines skipped; tid -1 for a contig the header lacks"""
    out = []
    for line in open(path).read().split("\n"):
        tok = [t for t in line.strip(" \r").split("\t")]
        if len(tok) < 3 or tok[0].startswith("#"):
            continue
        out.append((names.index(tok[0]) if tok[0] in names else -1, int(tok[1]), int(tok[2])))
    return out


def table(res, names, fasta=None):
    """rule O: the table's bytes; fasta: {contig name: bases} or None"""
    out = [HEADER]
    for i in range(res["n_sites"]):
        t, x, k = res["tid"][i], res["pos"][i], res["counts"][i]
        seq = (fasta or {}).get(names[t])
        ref = seq[x].upper() if seq is not None and x < len(seq) else "N"
        out.append("%s\t%d\t%s\t%d\t%s\n" % (names[t], x + 1, ref, sum(k[0:5]) + sum(k[8:13]), "\t".join(str(v) for v in k)))
    return "".join(out).encode()
