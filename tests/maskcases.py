"""Hand-written inputs for the error profile's variant mask.  vcf_cases(): VCF texts with their intervals and counters written out
(rule K); refusals(): texts that are refused, with the line that is named; record_cases() and pair_cases(): records under a mask with every
counter that is not zero written out (rule Y), in errprofcases' and fragerrcases' shape plus mask = [(contig name, start, end)], the mask's
intervals as a file gives them, in front of rule K's clamp.  The model (tests/pyerrmask.py), gce_mask_load, the per-record functions on the
host (tests/errmask_host_check.hip) and the kernels (tests/test_errmask_gpu.py, tests/test_fragerrmask_gpu.py) are all held against these.

The header and the FASTA are errprofcases': c0 has 40 of its header's 100 bases, c1 all 50, c2 (30) is missing; the mask is clamped to 40, 50
and nothing.   c0:  0 ACGTACGTAC  10 acgtNRYKMn  20 GGGGGCCCCC  30 TTTTTAAAAA        c1: ACGT x 12, AC"""
import errprofcases as ec
import fragerrcases as fx
from errprofcases import FASTA, LENS, NAMES, rec  # noqa: F401

CLAMP = [40, 50, -1]


def vcf(*rows):
    """rows of (CHROM, POS, REF, ALT) as VCF lines with a header"""
    return ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n" + "".join("%s\t%s\t.\t%s\t%s\n" % r for r in rows)).encode()


def vcase(label, premise, text, intervals, n_lines, n_records, n_unknown_contig=0, n_no_alt=0):
    return dict(label=label, premise=premise, text=text, intervals=intervals,
                counters=dict(n_lines=n_lines, n_records=n_records, n_unknown_contig=n_unknown_contig, n_no_alt=n_no_alt, n_intervals=len(intervals),
                              n_masked_bases=sum(z - a for _, a, z in intervals)))


def vcf_cases():
    c = []
    c.append(vcase("snp", "POS 5 is the 0-based position 4", vcf(("c0", 5, "A", "G")), [(0, 4, 5)], 3, 1))
    c.append(vcase("insertion", "an insertion masks its anchor base alone", vcf(("c0", 5, "A", "AGG")), [(0, 4, 5)], 3, 1))
    c.append(vcase("deletion", "a deletion with a three-base REF masks its anchor and the two deleted bases", vcf(("c0", 5, "ACG", "A")), [(0, 4, 7)], 3, 1))
    c.append(vcase("multi_allelic", "two ALT alleles, one record, one base", vcf(("c1", 10, "C", "A,T")), [(1, 9, 10)], 3, 1))
    c.append(vcase("no_alt", "ALT `.`, `<NON_REF>` and `<*>` alone are a gVCF's reference blocks; `A,<*>` is a variant", vcf(("c0", 1, "A", "."), ("c0", 2, "C", "<NON_REF>"),
                   ("c0", 3, "G", "<*>"), ("c0", 4, "T", "A,<*>")), [(0, 3, 4)], 6, 4, n_no_alt=3))
    c.append(vcase("unknown_contig", "a CHROM the header lacks, `.` as its ALT or not: n_unknown_contig", vcf(("zz", 1, "A", "C"), ("C0", 1, "A", "C"), ("zz", 1, "A", ".")), [], 5, 3,
                   n_unknown_contig=3))
    c.append(vcase("clamped_at_the_contig_end", "POS 50 is c1's last base; its REF of four runs past it", vcf(("c1", 50, "CACG", "C")), [(1, 49, 50)], 3, 1))
    c.append(vcase("fasta_shorter_than_header", "c0 has 40 bases in the FASTA under a header of 100: [38, 42) keeps 38 and 39, POS 41 keeps nothing",
                   vcf(("c0", 39, "AAAA", "A"), ("c0", 41, "N", "A"), ("c0", 100, "N", "A")), [(0, 38, 40)], 5, 3))
    c.append(vcase("contig_without_reference", "c2 is not in the FASTA: its records are records, its intervals are dropped", vcf(("c2", 1, "A", "C"), ("c2", 30, "A", "C")), [], 4, 2))
    c.append(vcase("abut_and_overlap", "[4, 6) and [6, 7) abut, [19, 23) and [21, 25) overlap, one inside another; not in order",
                   vcf(("c1", 22, "ACGT", "A"), ("c1", 7, "G", "T"), ("c1", 20, "ACGT", "A"), ("c1", 5, "AC", "A"), ("c1", 21, "C", "T"), ("c0", 9, "A", "C")),
                   [(0, 8, 9), (1, 4, 7), (1, 19, 25)], 8, 6))
    c.append(vcase("crlf_and_no_final_line_feed", "CR LF line ends, an empty line, and a last line without its line feed",
                   b"##fileformat=VCFv4.2\r\n\r\nc0\t1\t.\tA\tC\r\n\nc0\t3\trs7\tG\tT,A\tq\tPASS", [(0, 0, 1), (0, 2, 3)], 5, 2))
    c.append(vcase("long_line", "100 000 characters of genotypes behind the fifth field, and a short record behind the long one",
                   b"c1\t2\t.\tC\tT\t" + b"\t".join([b"0/1:35,12:47"] * 7700)[:100000] + b"\nc1\t4\t.\tT\tC\n", [(1, 1, 2), (1, 3, 4)], 2, 2))
    c.append(vcase("only_a_header", "no record: an empty mask", vcf(), [], 2, 0))
    c.append(vcase("empty_file", "no byte: an empty mask", b"", [], 0, 0))
    return c


def refusals():
    """(label, text, the line that is named, the words behind it)"""
    return [("four_fields", vcf(("c0", 1, "A", "C")) + b"c0\t2\t.\tC\n", 4, "fewer than five tab-separated fields"),
            ("pos_zero", vcf(("c0", 0, "A", "C")), 3, "POS is not a decimal integer >= 1"),
            ("pos_12x", b"\n" + vcf(("c0", 1, "A", "C"), ("c0", "12x", "A", "C")), 5, "POS is not a decimal integer >= 1"),
            ("pos_empty", vcf(("c0", "", "A", "C")), 3, "POS is not a decimal integer >= 1"),
            ("pos_negative", vcf(("c0", "-3", "A", "C")), 3, "POS is not a decimal integer >= 1"),
            ("ref_empty", vcf(("zz", 7, "", "C")), 3, "REF is empty"),
            ("no_tab_at_all", b"c0 1 . A C", 1, "fewer than five tab-separated fields")]


def mask_vcf(mask):
    """a case's mask as VCF text: one record per interval, REF as long as the interval"""
    return vcf(*[(nm, a + 1, "N" * (z - a), "<DEL>") for nm, a, z in mask])


def mask_of(cs, names=NAMES):
    """a case's mask as the intervals in front of rule K's clamp"""
    return [(names.index(nm), a, z) for nm, a, z in cs["mask"] if nm in names]


def rcase(label, premise, mask, records, expect, **kw):
    c = ec.case(label, premise, records, expect, **kw)
    c["mask"] = mask
    return c


def record_cases():
    c = []
    c.append(rcase("masked_snp_each_strand_and_segment", "T over the masked G at c0:2, forward and reverse in segments 0, 1 and 2: MASKED at cycle 3, on the reverse strand at 4 - 2",
                   [("c0", 2, 3)], [rec(0, 0, "4M", "ACTT", flag=f) for f in (0, 0x10, 0x40, 0x90)],
                   [(0, 1, "A>A", 1), (0, 2, "C>C", 1), (0, 3, "MASKED", 1), (0, 4, "T>T", 1), (0, 4, "T>T", 1), (0, 3, "G>G", 1), (0, 2, "MASKED", 1), (0, 1, "A>A", 1),
                    (1, 1, "A>A", 1), (1, 2, "C>C", 1), (1, 3, "MASKED", 1), (1, 4, "T>T", 1), (2, 4, "T>T", 1), (2, 3, "G>G", 1), (2, 2, "MASKED", 1), (2, 1, "A>A", 1)]))
    c.append(rcase("masked_in_front_of_lowq", "qualities 5 under min_baseq 10: c0:0 is LOWQ, the masked c0:1 is MASKED, a property of the position", [("c0", 1, 2)],
                   [rec(0, 0, "2M", "AC", [5, 5])], [(0, 1, "LOWQ", 1), (0, 2, "MASKED", 1)], min_baseq=10))
    c.append(rcase("insertion_by_the_position_in_front", "c0:1 is masked.  2M1I1M: the column at 1 and the inserted base behind it are MASKED.  1M1I1M: the inserted base is "
                   "anchored at 0 and counts, the column behind it at 1 is MASKED", [("c0", 1, 2)], [rec(0, 0, "2M1I1M", "ACAG"), rec(0, 0, "1M1I1M", "AAC")],
                   [(0, 1, "A>A", 2), (0, 2, "MASKED", 1), (0, 3, "MASKED", 2), (0, 4, "G>G", 1), (0, 2, "INS", 1)]))
    c.append(rcase("leading_insertion_by_its_own_position", "c0:2 is masked.  1I1M at 2: no M came earlier, the inserted base is anchored at 2 itself.  1I1M at 3: anchored at 3, "
                   "counted, although 2 is masked", [("c0", 2, 3)], [rec(0, 2, "1I1M", "AG"), rec(0, 3, "1I1M", "AT")],
                   [(0, 1, "MASKED", 1), (0, 2, "MASKED", 1), (0, 1, "INS", 1), (0, 2, "T>T", 1)]))
    c.append(rcase("deletion_by_its_first_position", "c0:2 is masked.  1M2D1M at 1 deletes 2 and 3: MASKED.  1M2D1M at 0 deletes 1 and 2: its first position is not masked, DEL",
                   [("c0", 2, 3)], [rec(0, 0, "1M2D1M", "AT"), rec(0, 1, "1M2D1M", "CA")],
                   [(0, 1, "C>C", 1), (0, 1, "MASKED", 1), (0, 2, "A>A", 1), (0, 1, "A>A", 1), (0, 1, "DEL", 1), (0, 2, "T>T", 1)]))
    c.append(rcase("masked_off_the_targets_is_not_counted", "the targets are c0:2 and 3, the mask holds c0:1 and 3: 1 is not counted at all, 3 is MASKED", [("c0", 1, 2), ("c0", 3, 4)],
                   [rec(0, 0, "4M", "ACGT")], [(0, 3, "G>G", 1), (0, 4, "MASKED", 1)], bed=[("c0", 2, 4)]))
    c.append(rcase("no_bit_beyond_the_fasta", "the mask's [38, 45) of c0 is clamped to the FASTA's 40 bases: 38 and 39 are MASKED, 40 and 41 stay REF_OTHER", [("c0", 38, 45)],
                   [rec(0, 38, "4M", "AAAA")], [(0, 1, "MASKED", 1), (0, 2, "MASKED", 1), (0, 3, "REF_OTHER", 1), (0, 4, "REF_OTHER", 1)]))
    c.append(rcase("last_base_of_a_contig", "c0:39 is masked, the FASTA's last base of c0; c1:0 is the next byte of the reference and stays clear", [("c0", 39, 40)],
                   [rec(0, 39, "1M", "A"), rec(1, 0, "1M", "A")], [(0, 1, "MASKED", 1), (0, 1, "A>A", 1)]))
    c.append(rcase("first_base_of_a_contig", "c1:0 is masked; c0:39, the byte in front of it, stays clear", [("c1", 0, 1)], [rec(0, 39, "1M", "A"), rec(1, 0, "1M", "A")],
                   [(0, 1, "A>A", 1), (0, 1, "MASKED", 1)]))
    return c


def pcase(label, premise, mask, records, expect, xexpect, pairs, shared, differ, **kw):
    c = fx.case(label, premise, records, expect, xexpect, pairs, shared, differ, **kw)
    c["mask"] = mask
    return c


def pair_cases():
    """fragerrcases' usual pair: a (first, forward) 6M over c0:20..25, b (last, reverse) 6M over 23..28; 23, 24 and 25 are shared"""
    c = []
    c.append(pcase("shared_masked_column", "c0:25 is masked and both mates read its C: a, which rule V' counts, adds MASKED once; both add OVL_MASKED; three shared columns as ever",
                   [("c0", 25, 26)], [fx.pa(), fx.pb()], fx.P2 + [(1, 6, "MASKED", 1)], fx.X2 + [(1, 6, "MASKED", 1), (2, 4, "MASKED", 1)], 1, 3, 0))
    c.append(pcase("shared_masked_column_b_counted", "a's T of 29 against b's C of 30 at the masked c0:25: b is the one counted and adds MASKED at its cycle 4; the column still "
                   "disagrees", [("c0", 25, 26)], [fx.pa("GGGGGT", [30] * 5 + [29]), fx.pb()], fx.P2 + [(2, 4, "MASKED", 1)], fx.X2 + [(1, 6, "MASKED", 1), (2, 4, "MASKED", 1)],
                   1, 3, 1))
    c.append(pcase("masked_columns_of_one_mate", "c0:20 (a alone, cycle 1) and c0:28 (b alone, cycle 1) are masked: rule W's columns, the overlap table is the unmasked one",
                   [("c0", 20, 21), ("c0", 28, 29)], [fx.pa(), fx.pb()],
                   [(1, 1, "MASKED", 1), (1, 2, "G>G", 1), (1, 3, "G>G", 1), (1, 4, "G>G", 1), (1, 5, "G>G", 1), (1, 6, "C>C", 1), (2, 3, "G>G", 1), (2, 2, "G>G", 1), (2, 1, "MASKED", 1)],
                   fx.X2 + [(1, 6, "AGREE_REF", 1), (2, 4, "AGREE_REF", 1)], 1, 3, 0))
    return c
