"""Hand-written records for gce_bam_error_profile: every case names its premise and lists, written out by hand, every counter
that is not zero and every skip counter.  The model (tests/pyerrprof.py), the per-record functions on the host (tests/errprof_host_check.hip)
and the kernels, with the LDS planes and with direct atomics (tests/test_errprof_gpu.py), are all held against these numbers.

A case: dict(label, premise, bed = None or [(contig name, start, end)], records = [bytes], min_mapq, min_baseq, exclude, expect = [(segment,
cycle, class name, count)], skips = {counter: n}).  The header is always NAMES / LENS and the FASTA is always FASTA: c0 has 40 of its header's
100 bases, c2 is missing.

c0:  0 ACGTACGTAC  10 acgtNRYKMn  20 GGGGGCCCCC  30 TTTTTAAAAA        c1: ACGT x 12, AC"""
from pileupcases import frames, malformed, rec, write_raw_bam  # noqa: F401

NAMES = ["c0", "c1", "c2"]
LENS = [100, 50, 30]
FASTA = {"c0": "ACGTACGTAC" + "acgtNRYKMn" + "GGGGGCCCCC" + "TTTTTAAAAA", "c1": "ACGT" * 12 + "AC"}


def case(label, premise, records, expect, skips=None, bed=None, min_mapq=0, min_baseq=0, exclude=0x704):
    sk = dict(n_unplaced=0, n_flagged=0, n_low_mapq=0, n_no_cigar=0, n_no_seq=0, n_bad_cigar=0, n_no_ref=0, n_too_long=0)
    sk.update(skips or {})
    return dict(label=label, premise=premise, bed=bed, records=records, expect=expect, skips=sk, min_mapq=min_mapq, min_baseq=min_baseq, exclude=exclude)


# one record with every op: 1H 1S 2M 1I 1M 2D 1M 3N 1M 1P 1S 1H at c0:20, query T|GA|T|G|C|T|A (clip, 2M, I, M, M, M, clip).  The columns:
# y1 G on G (20), y2 A on G (21), y3 inserted, y4 G on G (22), the D at 23 behind y4, y5 C on C (25), y6 T on C (29)
EVERY_OP = "1H1S2M1I1M2D1M3N1M1P1S1H"
EVERY_OP_FWD = [(2, "G>G"), (3, "G>A"), (4, "INS"), (5, "G>G"), (5, "DEL"), (6, "C>C"), (7, "C>T")]
# ... on the reverse strand the cycle of y is 8 - y and both bases are complemented
EVERY_OP_REV = [(7, "C>C"), (6, "C>T"), (5, "INS"), (4, "C>C"), (4, "DEL"), (3, "G>G"), (2, "G>A")]


def all_cases():
    c = []
    # ---- strands, segments, ops, cycles
    c.append(case("forward_columns", "a forward read: cycle y + 1, reference base against read base", [rec(0, 0, "4M", "ACCT")],
                  [(0, 1, "A>A", 1), (0, 2, "C>C", 1), (0, 3, "G>C", 1), (0, 4, "T>T", 1)]))
    c.append(case("reverse_complement", "a reverse read showing C over reference A is T>G at cycle l_seq - 0; the matches behind it are G>G, C>C, A>A at cycles 3, 2, 1",
                  [rec(0, 0, "4M", "CCGT", flag=16)], [(0, 4, "T>G", 1), (0, 3, "G>G", 1), (0, 2, "C>C", 1), (0, 1, "A>A", 1)]))
    c.append(case("g_to_t_apart_from_c_to_a", "G>T on the forward strand and the same columns on the reverse strand (C>A) stay apart",
                  [rec(0, 2, "1M", "T"), rec(0, 2, "1M", "T", flag=16)], [(0, 1, "G>T", 1), (0, 1, "C>A", 1)]))
    c.append(case("segments", "0x40 alone is segment 1, 0x80 alone segment 2, both or neither segment 0",
                  [rec(0, 0, "1M", "A", flag=f) for f in (0x40, 0x80, 0xC0, 0)], [(1, 1, "A>A", 1), (2, 1, "A>A", 1), (0, 1, "A>A", 2)]))
    c.append(case("every_op_strand_segment", "every op, with soft and hard clips at both ends, on both strands in all three segments",
                  [rec(0, 20, EVERY_OP, "TGATGCTA", flag=f) for f in (0, 0x10, 0x40, 0x50, 0x80, 0x90)],
                  [(g, cy, cl, 1) for g in (0, 1, 2) for cy, cl in EVERY_OP_FWD + EVERY_OP_REV]))
    c.append(case("soft_clips_forward", "3S2M1S forward: the aligned bases are cycles 4 and 5", [rec(0, 0, "3S2M1S", "TTTACT")], [(0, 4, "A>A", 1), (0, 5, "C>C", 1)]))
    c.append(case("soft_clips_reverse", "3S2M1S reverse, l_seq 6: the aligned bases y = 3, 4 are cycles 3 and 2", [rec(0, 0, "3S2M1S", "TTTACT", flag=16)],
                  [(0, 3, "T>T", 1), (0, 2, "G>G", 1)]))
    c.append(case("hard_clips_not_counted", "5H in front moves no cycle", [rec(0, 0, "5H2M", "AC")], [(0, 1, "A>A", 1), (0, 2, "C>C", 1)]))
    c.append(case("eq_and_x", "= and X walk as M does", [rec(0, 0, "1=1X", "AG")], [(0, 1, "A>A", 1), (0, 2, "C>G", 1)]))
    # ---- reference bytes
    c.append(case("reference_bytes", "c0:10..19 is acgt N R Y K M n: lower case folds, everything else is REF_OTHER whatever the read shows",
                  [rec(0, 10, "10M", "ACGTAAAAAA")], [(0, 1, "A>A", 1), (0, 2, "C>C", 1), (0, 3, "G>G", 1), (0, 4, "T>T", 1)] + [(0, cy, "REF_OTHER", 1) for cy in range(5, 11)]))
    c.append(case("fasta_end", "the FASTA's c0 has 40 bases under a header of 100: c0:39 is its last base, c0:40 and 41 are REF_OTHER", [rec(0, 38, "4M", "AAAA")],
                  [(0, 1, "A>A", 1), (0, 2, "A>A", 1), (0, 3, "REF_OTHER", 1), (0, 4, "REF_OTHER", 1)]))
    c.append(case("contig_missing", "c2 is not in the FASTA", [rec(2, 0, "2M", "AC"), rec(0, 0, "1M", "A")], [(0, 1, "A>A", 1)], dict(n_no_ref=1)))
    # ---- read nibbles
    c.append(case("read_nibbles", "nibbles 0 (=), 15 (N) and 3 (M) are READ_N; A over T is T>A", [rec(0, 0, "4M", "=NMA")],
                  [(0, 1, "READ_N", 1), (0, 2, "READ_N", 1), (0, 3, "READ_N", 1), (0, 4, "T>A", 1)]))
    c.append(case("ref_other_before_read_n", "N over N: the reference is tested first", [rec(0, 14, "1M", "N")], [(0, 1, "REF_OTHER", 1)]))
    # ---- qualities
    c.append(case("lowq_before_ref_other", "quality 5 under min_baseq 10, N over N: the quality is tested first", [rec(0, 14, "1M", "N", [5])], [(0, 1, "LOWQ", 1)], min_baseq=10))
    c.append(case("no_qualities", "QUAL[0] == 0xFF: no quality test although min_baseq is 20", [rec(0, 0, "2M", "AC", "*")], [(0, 1, "A>A", 1), (0, 2, "C>C", 1)], min_baseq=20))
    c.append(case("quality_edges", "quality 19 under min_baseq 20 goes to LOWQ, quality 20 is counted", [rec(0, 0, "2M", "AC", [19, 20])],
                  [(0, 1, "LOWQ", 1), (0, 2, "C>C", 1)], min_baseq=20))
    c.append(case("ins_and_del_have_no_quality_test", "qualities 3 under min_baseq 20: the M columns go to LOWQ, INS and DEL are counted",
                  [rec(0, 0, "1M1I1D1M", "AAC", [3, 3, 3])], [(0, 1, "LOWQ", 1), (0, 2, "INS", 1), (0, 2, "DEL", 1), (0, 3, "LOWQ", 1)], min_baseq=20))
    # ---- insertions and deletions at the edges of a record
    c.append(case("leading_insertion", "1I1M: INS at cycle 1, the M is cycle 2", [rec(0, 0, "1I1M", "GA")], [(0, 1, "INS", 1), (0, 2, "A>A", 1)]))
    c.append(case("long_insertion", "every inserted base adds INS at its own cycle", [rec(0, 0, "1M3I1M", "AGGGC")],
                  [(0, 1, "A>A", 1), (0, 2, "INS", 1), (0, 3, "INS", 1), (0, 4, "INS", 1), (0, 5, "C>C", 1)]))
    c.append(case("insertion_behind_zero_length_m", "0M1I1M at c0:1", [rec(0, 1, "0M1I1M", "GC")], [(0, 1, "INS", 1), (0, 2, "C>C", 1)]))
    c.append(case("d_first", "a D as first op: DEL at the cycle of query index 0", [rec(0, 0, "1D1M", "C")], [(0, 1, "DEL", 1), (0, 1, "C>C", 1)]))
    c.append(case("d_first_reverse", "1D2M reverse, l_seq 2: DEL at the cycle of query index 0, which is 2", [rec(0, 0, "1D2M", "CG", flag=16)],
                  [(0, 2, "DEL", 1), (0, 2, "G>G", 1), (0, 1, "C>C", 1)]))
    c.append(case("d_n_d", "1M1D2N1D1M: two DEL at the cycle of query index 0, one per op whatever its length", [rec(0, 0, "1M1D2N1D1M", "AA")],
                  [(0, 1, "A>A", 1), (0, 1, "DEL", 2), (0, 2, "C>A", 1)]))
    c.append(case("long_d_counts_once", "a 5D adds one DEL", [rec(0, 0, "1M5D1M", "AG")], [(0, 1, "A>A", 1), (0, 1, "DEL", 1), (0, 2, "G>G", 1)]))
    # ---- l_seq at the limit
    c.append(case("l_seq_1024", "l_seq 1024 is eligible: the last two bases are cycles 1023 and 1024 forward, 2 and 1 reverse",
                  [rec(1, 0, "1022S2M", "A" * 1022 + "AC"), rec(1, 0, "1022S2M", "A" * 1022 + "AC", flag=16), rec(1, 0, "2M1022S", "AC" + "A" * 1022, flag=16)],
                  [(0, 1023, "A>A", 1), (0, 1024, "C>C", 1), (0, 2, "T>T", 1), (0, 1, "G>G", 1), (0, 1024, "T>T", 1), (0, 1023, "G>G", 1)]))
    c.append(case("l_seq_1025", "l_seq 1025 is too long", [rec(1, 0, "1023S2M", "A" * 1023 + "AC")], [], dict(n_too_long=1)))
    # ---- skips: the exact counter, and no add
    c.append(case("each_bit_of_0x704", "each bit of 0x704 skips; 0x800, outside it, does not", [rec(0, 0, "1M", "A", flag=f) for f in (0x4, 0x100, 0x200, 0x400, 0x800)],
                  [(0, 1, "A>A", 1)], dict(n_flagged=4)))
    c.append(case("mapq_edges", "mapq 9 under min_mapq 10 skips, mapq 10 is counted", [rec(0, 0, "1M", "A", mapq=9), rec(0, 1, "1M", "C", mapq=10)], [(0, 1, "C>C", 1)],
                  dict(n_low_mapq=1), min_mapq=10))
    c.append(case("pileup_skips", "tid -1, pos -1, n_cigar_op 0, l_seq 0, an op code 9, a query length off by one",
                  [rec(-1, 0, "1M"), rec(0, -1, "1M"), rec(0, 0, [], "A"), rec(0, 0, "2D", ""), rec(0, 0, [(0, 1), (9, 1)], "A"), rec(0, 0, "3M", "AC")], [],
                  dict(n_unplaced=2, n_no_cigar=1, n_no_seq=1, n_bad_cigar=2)))
    c.append(case("skip_order", "the first failing test decides, and every record here fails the next test too: unplaced, flagged, low mapq, no CIGAR, no bases, bad CIGAR, "
                  "no reference, too long",
                  [rec(-1, 10, [], "", flag=0x400, mapq=0), rec(0, 10, [], "", flag=0x400, mapq=0), rec(0, 10, [], "", mapq=0), rec(0, 10, [], ""), rec(0, 10, [(9, 1)], ""),
                   rec(2, 0, [(9, 1)], "A"), rec(2, 0, "1025M"), rec(0, 0, "1025M")], [],
                  dict(n_unplaced=1, n_flagged=1, n_low_mapq=1, n_no_cigar=1, n_no_seq=1, n_bad_cigar=1, n_no_ref=1, n_too_long=1), min_mapq=1))
    # ---- rule B: the targets are c0:2 and c0:3
    T = [("c0", 2, 4)]
    c.append(case("bed_columns", "columns at c0:1..4: the first site, the last site, not the one in front nor the one past the end", [rec(0, 1, "4M", "CGTA")],
                  [(0, 2, "G>G", 1), (0, 3, "T>T", 1)], bed=T))
    c.append(case("bed_insertions", "an inserted base is anchored one in front of it: anchors 1, 2, 3 and 4 count as out, in, in, out",
                  [rec(0, 1, "1M1I1M", "CAG"), rec(0, 2, "1M1I1M", "GAT"), rec(0, 3, "1M1I1M", "TAA"), rec(0, 4, "1M1I1M", "AAC")],
                  [(0, 3, "G>G", 1), (0, 1, "G>G", 1), (0, 2, "INS", 2), (0, 3, "T>T", 1), (0, 1, "T>T", 1)], bed=T))
    c.append(case("bed_leading_insertions", "a leading inserted base is anchored at x itself: at 1 out, at 2 and 3 in, at 4 out although 3 is a site",
                  [rec(0, 1, "1I1M", "AC"), rec(0, 2, "1I1M", "AG"), rec(0, 3, "1S1I1M", "AAT"), rec(0, 4, "1I1M", "AA")],
                  [(0, 1, "INS", 1), (0, 2, "G>G", 1), (0, 2, "INS", 1), (0, 3, "T>T", 1)], bed=T))
    c.append(case("bed_deletions", "a deletion is anchored at its first position: 1 (out, although it runs over both sites), 2, 3 (in), 4 (out)",
                  [rec(0, 0, "1M3D1M", "AA"), rec(0, 1, "1M2D1M", "CA"), rec(0, 2, "1M1D1M", "GA"), rec(0, 3, "1M2D1M", "TC")],
                  [(0, 1, "DEL", 2), (0, 1, "G>G", 1), (0, 1, "T>T", 1)], bed=T))
    c.append(case("bed_two_intervals", "one read over two intervals and the gap between them; an N over the first", [rec(0, 0, "8M", "ACGTACGT"), rec(0, 1, "1M3N2M", "CCG")],
                  [(0, 3, "G>G", 1), (0, 4, "T>T", 1), (0, 7, "G>G", 1), (0, 3, "G>G", 1)], bed=[("c0", 2, 4), ("c0", 6, 7)]))
    c.append(case("bed_empty", "a BED without a region: an eligible record, no counter", [rec(0, 0, "2M", "AC")], [], bed=[]))
    c.append(case("bed_unknown_contig", "a BED whose only region lies on a contig the header lacks", [rec(0, 0, "2M", "AC")], [], bed=[("zz", 0, 50)]))
    c.append(case("bed_clamped", "[45, 60) of c1 is clamped to the header's 50 bases; the FASTA has them all", [rec(1, 44, "4M", "ACGT")],
                  [(0, 2, "C>C", 1), (0, 3, "G>G", 1), (0, 4, "T>T", 1)], bed=[("c1", 45, 60)]))
    return c


def expected(cs):
    """the case's expect list as {(segment, cycle, class name): count}"""
    out = {}
    for g, cy, cl, n in cs["expect"]:
        out[g, cy, cl] = out.get((g, cy, cl), 0) + n
    return out


def regions_of(cs, names=NAMES):
    return None if cs["bed"] is None else [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in cs["bed"]]


def refs():
    return [FASTA.get(nm) for nm in NAMES]


def fasta_text(fasta=FASTA):
    return "".join(">%s\n%s\n" % kv for kv in fasta.items())
