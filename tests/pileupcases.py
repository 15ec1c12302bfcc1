"""Hand-written records for gce_bam_pileup: every case names its premise and lists, written out by hand, every counter that is
not zero and every skip counter.  The model (tests/pypileup.py), the per-record functions on the host (tests/pileup_host_check.hip) and the
kernels, with the LDS tile and with direct atomics (tests/test_pileup_gpu.py), are all held against these numbers.

A case: dict(label, premise, bed = [(contig name, start, end)], records = [bytes], min_mapq, min_baseq, exclude, expect = [(tid, pos, strand,
class, count)], skips = {counter: n}, n_sites, n_intervals).  The header is always NAMES / LENS."""
import re
import struct

NAMES = ["c0", "c1"]
LENS = [100, 50]
CODE = "=ACMGRSVTWYHKDBN"            # the nibble of a letter: = is 0, M is 3, N is 15
OPS = "MIDNSHP=X"


def rec(tid, pos, cigar, seq=None, qual=None, flag=0, mapq=60, name="r", lseq=None, aux=b""):
    """a BAM record (block_size first).  cigar: text, or a list of (op code, length) for codes the text cannot say; seq: letters of CODE
    (default: A for every query base of the CIGAR); qual: a list, "*" for 0xFF bytes, default 30s; lseq: l_seq when it is not len(seq)"""
    ops = [(OPS.index(o), int(n)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", cigar)] if isinstance(cigar, str) else list(cigar)
    if seq is None:
        seq = "A" * sum(n for op, n in ops if op in (0, 1, 4, 7, 8))
    n = len(seq)
    if qual is None:
        qual = [30] * n
    elif qual == "*":
        qual = [0xFF] * n
    nib = [CODE.index(c) for c in seq] + [0]
    packed = bytes(nib[2 * k] << 4 | nib[2 * k + 1] for k in range((n + 1) // 2))
    nm = name.encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, 4680, len(ops), flag, n if lseq is None else lseq, -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", ln << 4 | op) for op, ln in ops) + packed + bytes(qual) + aux
    return struct.pack("<I", len(body)) + body


def case(label, premise, bed, records, expect, skips=None, n_sites=None, n_intervals=None, min_mapq=0, min_baseq=0, exclude=0x704):
    sk = dict(n_unplaced=0, n_flagged=0, n_low_mapq=0, n_no_cigar=0, n_no_seq=0, n_bad_cigar=0)
    sk.update(skips or {})
    return dict(label=label, premise=premise, bed=bed, records=records, expect=expect, skips=sk, n_sites=n_sites, n_intervals=n_intervals, min_mapq=min_mapq,
                min_baseq=min_baseq, exclude=exclude)


T = [("c0", 10, 12)]                 # two sites: c0:10 and c0:11


def all_cases():
    c = []
    # ---- every op at an interval's edges
    c.append(case("m_begins_one_before", "an M that begins one base in front of the interval adds from its second column on",
                  [("c0", 10, 20)], [rec(0, 9, "4M", "ACGT")], [(0, 10, "+", "C", 1), (0, 11, "+", "G", 1), (0, 12, "+", "T", 1)], n_sites=10, n_intervals=1))
    c.append(case("m_ends_on_last_site", "an M whose last column is the interval's last site", [("c0", 10, 20)], [rec(0, 17, "3M", "ACG")],
                  [(0, 17, "+", "A", 1), (0, 18, "+", "C", 1), (0, 19, "+", "G", 1)], n_sites=10, n_intervals=1))
    c.append(case("d_across_end", "a D over c0:18..21 adds DEL at 18 and 19 only; the M behind it lies outside", [("c0", 10, 20)], [rec(0, 17, "1M4D1M", "AC")],
                  [(0, 17, "+", "A", 1), (0, 18, "+", "DEL", 1), (0, 19, "+", "DEL", 1)], n_sites=10))
    c.append(case("n_over_interval", "an N over the whole interval [10, 12) adds nothing there; the M behind it lands on the next interval",
                  [("c0", 10, 12), ("c0", 13, 14)], [rec(0, 9, "1M3N1M", "AC")], [(0, 13, "+", "C", 1)], n_sites=3, n_intervals=2))
    c.append(case("i_behind_last_site", "an I whose x - 1 is the interval's last site adds INS there", T, [rec(0, 10, "2M1I1M", "ACGT")],
                  [(0, 10, "+", "A", 1), (0, 11, "+", "C", 1), (0, 11, "+", "INS", 1)], n_sites=2))
    c.append(case("i_in_front_of_interval", "an I whose x - 1 = 9 lies one base in front of the interval adds nothing; the M behind it reads bases 3 and 4",
                  T, [rec(0, 8, "2M1I2M", "ACGTA")], [(0, 10, "+", "T", 1), (0, 11, "+", "A", 1)]))
    c.append(case("leading_i", "a leading I adds nothing although x - 1 = 10 is a site", T, [rec(0, 11, "1I1M", "AC")], [(0, 11, "+", "C", 1)]))
    c.append(case("s_then_i", "S then I: still no M, =, X or D in front of the I", T, [rec(0, 11, "1S1I1M", "ACG")], [(0, 11, "+", "G", 1)]))
    c.append(case("two_adjacent_i", "two adjacent I ops add two", T, [rec(0, 10, "1M1I1I1M", "ACGT")], [(0, 10, "+", "A", 1), (0, 10, "+", "INS", 2), (0, 11, "+", "T", 1)]))
    c.append(case("h_and_p", "H and P move nothing", T, [rec(0, 10, "2H1M1P1M2H", "AC")], [(0, 10, "+", "A", 1), (0, 11, "+", "C", 1)]))
    c.append(case("eq_and_x", "= and X walk as M does", T, [rec(0, 10, "1=1X", "AC")], [(0, 10, "+", "A", 1), (0, 11, "+", "C", 1)]))
    c.append(case("i_behind_d", "a D counts as an earlier op: the I behind it adds INS at the deleted site", T, [rec(0, 9, "1M1D1I1M", "ACG")],
                  [(0, 10, "+", "DEL", 1), (0, 10, "+", "INS", 1), (0, 11, "+", "G", 1)]))
    c.append(case("i_behind_zero_length_m", "a 0M is an earlier op: the I behind it adds INS at pos - 1", T, [rec(0, 11, "0M1I1M", "AC")],
                  [(0, 10, "+", "INS", 1), (0, 11, "+", "C", 1)]))
    # ---- regions
    c.append(case("two_intervals_and_gap", "one read over two intervals and the gap between them", [("c0", 10, 12), ("c0", 14, 16)], [rec(0, 9, "8M", "ACGTACGT")],
                  [(0, 10, "+", "C", 1), (0, 11, "+", "G", 1), (0, 14, "+", "C", 1), (0, 15, "+", "G", 1)], n_sites=4, n_intervals=2))
    c.append(case("merged_regions", "overlapping, abutting and duplicate regions are one interval of 7 sites", [("c0", 10, 13), ("c0", 12, 15), ("c0", 15, 17), ("c0", 10, 13)],
                  [rec(0, 10, "7M")], [(0, 10 + k, "+", "A", 1) for k in range(7)], n_sites=7, n_intervals=1))
    c.append(case("unknown_contig", "a region on a contig the header lacks gives no site", [("zz", 0, 50), ("c0", 10, 11)], [rec(0, 10, "1M", "G")], [(0, 10, "+", "G", 1)],
                  n_sites=1, n_intervals=1))
    c.append(case("beyond_contig_end", "c1 has 50 bases: [45, 60) is clamped to five sites, [60, 70) gives none; the read runs past the end", [("c1", 45, 60), ("c1", 60, 70)],
                  [rec(1, 48, "5M", "ACGTA")], [(1, 48, "+", "A", 1), (1, 49, "+", "C", 1)], n_sites=5, n_intervals=1))
    c.append(case("negative_start", "a negative start is clamped to 0", [("c0", -5, 2)], [rec(0, 0, "3M", "ACG")], [(0, 0, "+", "A", 1), (0, 1, "+", "C", 1)], n_sites=2, n_intervals=1))
    c.append(case("empty_bed", "no region at all: an eligible record, no site", [], [rec(0, 10, "2M")], [], n_sites=0, n_intervals=0))
    c.append(case("inverted_region", "start >= end contributes nothing", [("c0", 20, 20), ("c0", 30, 25), ("c0", 10, 11)], [rec(0, 10, "1M", "T")], [(0, 10, "+", "T", 1)],
                  n_sites=1, n_intervals=1))
    # ---- bases and strands
    c.append(case("nibbles_0_3_15", "nibbles 0 (=), 3 (M) and 15 (N) all count as N", [("c0", 10, 13)], [rec(0, 10, "3M", "=MN")],
                  [(0, 10, "+", "N", 1), (0, 11, "+", "N", 1), (0, 12, "+", "N", 1)]))
    c.append(case("odd_first_query_offset", "an odd soft clip in front: the first counted base is the low nibble of byte 0", T, [rec(0, 10, "1S2M", "ACG")],
                  [(0, 10, "+", "C", 1), (0, 11, "+", "G", 1)]))
    c.append(case("even_first_query_offset", "an even soft clip in front: the first counted base is the high nibble of byte 1", T, [rec(0, 10, "2S2M", "AACG")],
                  [(0, 10, "+", "C", 1), (0, 11, "+", "G", 1)]))
    c.append(case("no_qualities", "QUAL[0] == 0xFF: no quality test although min_baseq is 20", T, [rec(0, 10, "2M", "AC", "*")], [(0, 10, "+", "A", 1), (0, 11, "+", "C", 1)],
                  min_baseq=20))
    c.append(case("quality_edges", "quality 19 under min_baseq 20 goes to LOWQ, quality 20 is counted", T, [rec(0, 10, "2M", "AC", [19, 20])],
                  [(0, 10, "+", "LOWQ", 1), (0, 11, "+", "C", 1)], min_baseq=20))
    c.append(case("d_has_no_quality_test", "low qualities around a D: the M columns go to LOWQ, the DEL is counted", [("c0", 10, 13)], [rec(0, 10, "1M1D1M", "AC", [3, 3])],
                  [(0, 10, "+", "LOWQ", 1), (0, 11, "+", "DEL", 1), (0, 12, "+", "LOWQ", 1)], min_baseq=20))
    c.append(case("both_strands", "flag 0x10 selects the reverse strand's counters", T, [rec(0, 10, "2M", "AC"), rec(0, 10, "2M", "AG", flag=16), rec(0, 11, "1M1I1M", "TTT", flag=16)],
                  [(0, 10, "+", "A", 1), (0, 11, "+", "C", 1), (0, 10, "-", "A", 1), (0, 11, "-", "G", 1), (0, 11, "-", "T", 1), (0, 11, "-", "INS", 1)]))
    # ---- skips: the exact counter, and no add
    flagged = [rec(0, 10, "2M", flag=f) for f in (0x4, 0x100, 0x200, 0x400)]
    c.append(case("each_bit_of_0x704", "each bit of 0x704 skips; 0x800, outside it, does not", T, flagged + [rec(0, 10, "2M", "CC", flag=0x800)],
                  [(0, 10, "+", "C", 1), (0, 11, "+", "C", 1)], dict(n_flagged=4)))
    c.append(case("mapq_edges", "mapq 9 under min_mapq 10 skips, mapq 10 is counted", T, [rec(0, 10, "2M", "GG", mapq=9), rec(0, 10, "2M", "TT", mapq=10)],
                  [(0, 10, "+", "T", 1), (0, 11, "+", "T", 1)], dict(n_low_mapq=1), min_mapq=10))
    c.append(case("no_cigar", "n_cigar_op 0", T, [rec(0, 10, [], "AC")], [], dict(n_no_cigar=1)))
    c.append(case("no_seq", "l_seq 0 with a CIGAR", T, [rec(0, 10, "2D", "")], [], dict(n_no_seq=1)))
    c.append(case("op_code_9", "an op code 9", T, [rec(0, 10, [(0, 1), (9, 1), (0, 1)], "AC")], [], dict(n_bad_cigar=1)))
    c.append(case("query_length_off_by_one", "the CIGAR's query length is 3 and 1, l_seq is 2", T, [rec(0, 10, "3M", "AC"), rec(0, 10, "1M", "AC")], [], dict(n_bad_cigar=2)))
    c.append(case("unplaced", "tid -1, tid == n_ref, pos -1", T, [rec(-1, 10, "2M"), rec(2, 10, "2M"), rec(0, -1, "2M")], [], dict(n_unplaced=3)))
    c.append(case("skip_order", "the first failing test decides: unplaced before flagged before low mapq before no CIGAR before no bases before a bad CIGAR", T,
                  [rec(-1, 10, [], "", flag=0x400, mapq=0), rec(0, 10, [], "", flag=0x400, mapq=0), rec(0, 10, [], "", mapq=0), rec(0, 10, [], ""), rec(0, 10, [(9, 1)], "")],
                  [], dict(n_unplaced=1, n_flagged=1, n_low_mapq=1, n_no_cigar=1, n_no_seq=1), min_mapq=1))
    c.append(case("other_exclude_flags", "exclude_flags is the caller's: under 0x10 the reverse strand is skipped and 0x400 is counted", T,
                  [rec(0, 10, "2M", "AC", flag=16), rec(0, 10, "2M", "GT", flag=0x400)], [(0, 10, "+", "G", 1), (0, 11, "+", "T", 1)], dict(n_flagged=1), exclude=0x10))
    return c


def malformed():
    """records the scan refuses: fields that overrun block_size"""
    good = rec(0, 10, "2M", "AC")
    over = bytearray(good)
    struct.pack_into("<i", over, 4 + 16, 40)                 # l_seq 40: bases and qualities no longer fit block_size
    neg = bytearray(good)
    struct.pack_into("<i", neg, 4 + 16, -1)
    cig = bytearray(good)
    struct.pack_into("<H", cig, 4 + 12, 60)                  # n_cigar_op 60
    return [("l_seq_overruns", bytes(over)), ("l_seq_negative", bytes(neg)), ("n_cigar_overruns", bytes(cig))]


def expected_counts(cs, sites):
    """the case's expect list as [n_sites][16], sites = [(tid, pos)] in order"""
    import pypileup
    out = [[0] * 16 for _ in sites]
    for tid, pos, strand, cls, n in cs["expect"]:
        out[sites.index((tid, pos))][(8 if strand == "-" else 0) + pypileup.CLASSES.index(cls)] += n
    return out


def regions_of(cs):
    return [(NAMES.index(nm) if nm in NAMES else -1, a, z) for nm, a, z in cs["bed"]]


def bed_text(cs):
    return "".join("%s\t%d\t%d\n" % r for r in cs["bed"])


def write_raw_bam(path, records, names=NAMES, lens=LENS, block=0xff00):
    """whole records (bytes) behind a header of names / lens, in BGZF members of `block` inflated bytes"""
    import pybam
    text = "@HD\tVN:1.6\tSO:unsorted\n"
    stream = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(names))
    for nm, ln in zip(names, lens):
        stream += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<I", ln)
    stream += b"".join(records)
    with open(path, "wb") as f:
        for o in range(0, len(stream), block):
            f.write(pybam.bgzf_block(stream[o:o + block]))
        f.write(pybam.EOF_BLOCK)


def frames(records):
    return b"".join(struct.pack("<I", len(r)) + r for r in records)
