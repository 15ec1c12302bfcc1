"""Hand-written records for gce_bam_error_profile_fragments: every case names its premise and lists, written out by hand, every
counter of the primary table and of the overlap table that is not zero, every skip counter, and n_pairs, n_shared_columns,
n_disagree_columns and n_ambiguous.  The model (tests/pyfragerr.py), the per-record functions on the host (tests/fragerr_host_check.hip) and
the kernels, with the LDS planes and with direct atomics, with the full and the weak hash (tests/test_fragerr_gpu.py), are all held against
these numbers.

The header, the FASTA and the case dict are errprofcases' (c0: 20 GGGGG 25 CCCCC; 10 acgtNRYKMn; 40 bases under a header of 100), plus
xexpect = [(segment, cycle, overlap class name, count)], pairs, shared, differ and ambiguous.  The usual shape: mate a (first, forward) at
c0:20 with 6M over 20..25, cycles 1..6 of segment 1; mate b (last, reverse) at c0:23 with 6M over 23..28, cycle 6 - y of segment 2.  Columns
23, 24 and 25 are shared: a's cycles 4, 5, 6 and b's cycles 6, 5, 4.  The reference there is G, G, C; a reverse mate that reads the
reference's G adds C>C, one that reads its C adds G>G.  Most cases leave 23 and 24 in agreement with the reference and put their subject
on column 25."""
import errprofcases as ec
from errprofcases import FASTA, LENS, NAMES, rec  # noqa: F401
from fragcases import mated

A_FWD, B_REV = 0x41, 0x91


def pa(seq="GGGGGC", qual=None, flag=A_FWD, pos=20, cigar="6M", next_pos=23, name="p", tid=0, **kw):
    return mated(rec(tid, pos, cigar, seq, qual, flag=flag, name=name, **kw), next_pos)


def pb(seq="GGCCCC", qual=None, flag=B_REV, pos=23, cigar="6M", next_pos=20, name="p", tid=0, **kw):
    return pa(seq, qual, flag, pos, cigar, next_pos, name, tid, **kw)


def case(label, premise, records, expect, xexpect, pairs, shared, differ, ambiguous=0, **kw):
    c = ec.case(label, premise, records, expect, **kw)
    c.update(xexpect=xexpect, pairs=pairs, shared=shared, differ=differ, ambiguous=ambiguous)
    return c


A_ALONE = [(1, 1, "G>G", 1), (1, 2, "G>G", 1), (1, 3, "G>G", 1)]                 # a's columns 20, 21, 22
B_ALONE = [(2, 3, "G>G", 1), (2, 2, "G>G", 1), (2, 1, "G>G", 1)]                 # b's columns 26, 27, 28: C on C, complemented
# columns 23 and 24 where both mates read the reference's G: a is counted, both add AGREE_REF
P2 = A_ALONE + [(1, 4, "G>G", 1), (1, 5, "G>G", 1)] + B_ALONE
X2 = [(1, 4, "AGREE_REF", 1), (1, 5, "AGREE_REF", 1), (2, 6, "AGREE_REF", 1), (2, 5, "AGREE_REF", 1)]
# a record of the usual shape counted alone
A_WHOLE = A_ALONE + [(1, 4, "G>G", 1), (1, 5, "G>G", 1), (1, 6, "C>C", 1)]
B_WHOLE = [(2, 6, "C>C", 1), (2, 5, "C>C", 1), (2, 4, "G>G", 1)] + B_ALONE


def all_cases():
    c = []
    # ---- column 25 (reference C): a's cycle 6, b's cycle 4
    c.append(case("agree_ref", "both mates read C: a is counted once, both add AGREE_REF", [pa(), pb()], P2 + [(1, 6, "C>C", 1)],
                  X2 + [(1, 6, "AGREE_REF", 1), (2, 4, "AGREE_REF", 1)], 1, 3, 0))
    c.append(case("agree_alt", "both mates read T over C: one C>T in the primary table, a's; AGREE_ALT from both", [pa("GGGGGT"), pb("GGTCCC")], P2 + [(1, 6, "C>T", 1)],
                  X2 + [(1, 6, "AGREE_ALT", 1), (2, 4, "AGREE_ALT", 1)], 1, 3, 0))
    c.append(case("differ_a_wins_by_quality", "a's T of 31 against b's C of 30: a is counted; a's sequencing error C>T at its cycle 6, b read it right: the diagonal, complemented",
                  [pa("GGGGGT", [30] * 5 + [31]), pb()], P2 + [(1, 6, "C>T", 1)], X2 + [(1, 6, "C>T", 1), (2, 4, "G>G", 1)], 1, 3, 1))
    c.append(case("differ_b_wins", "a's T of 29 against b's C of 30: b is counted, at its own segment, cycle and orientation; the overlap table is as before",
                  [pa("GGGGGT", [30] * 5 + [29]), pb()], P2 + [(2, 4, "G>G", 1)], X2 + [(1, 6, "C>T", 1), (2, 4, "G>G", 1)], 1, 3, 1))
    c.append(case("differ_tie_a_wins", "a's T of 30 against b's C of 30: a wins the tie", [pa("GGGGGT"), pb()], P2 + [(1, 6, "C>T", 1)],
                  X2 + [(1, 6, "C>T", 1), (2, 4, "G>G", 1)], 1, 3, 1))
    c.append(case("reverse_mate_error", "b, on the reverse strand, reads T over C at its y = 2: its sequencing error is G>A at cycle 6 - 2; a wins the tie and read it right",
                  [pa(), pb("GGTCCC")], P2 + [(1, 6, "C>C", 1)], X2 + [(1, 6, "C>C", 1), (2, 4, "G>A", 1)], 1, 3, 1))
    c.append(case("diff_other", "a reads T, b reads A, the reference has C: a wins the tie; neither matches", [pa("GGGGGT"), pb("GGACCC")], P2 + [(1, 6, "C>T", 1)],
                  X2 + [(1, 6, "DIFF_OTHER", 1), (2, 4, "DIFF_OTHER", 1)], 1, 3, 1))
    c.append(case("n_in_one_mate", "a reads N against b's C: the classes differ, a wins the tie and adds READ_N; the column is unusable for both", [pa("GGGGGN"), pb()],
                  P2 + [(1, 6, "READ_N", 1)], X2 + [(1, 6, "UNUSABLE", 1), (2, 4, "UNUSABLE", 1)], 1, 3, 1))
    # ---- the reference
    c.append(case("reference_bytes", "a at 10 over a c g t N R, b at 13 over t N R Y K M: lower case folds (13 agrees with the reference), N and R are REF_OTHER and unusable",
                  [pa("ACGTAA", pos=10, next_pos=13), pb("TAAAAA", pos=13, next_pos=10)],
                  [(1, 1, "A>A", 1), (1, 2, "C>C", 1), (1, 3, "G>G", 1), (1, 4, "T>T", 1), (1, 5, "REF_OTHER", 1), (1, 6, "REF_OTHER", 1)] + [(2, cy, "REF_OTHER", 1) for cy in (3, 2, 1)],
                  [(1, 4, "AGREE_REF", 1), (2, 6, "AGREE_REF", 1), (1, 5, "UNUSABLE", 1), (2, 5, "UNUSABLE", 1), (1, 6, "UNUSABLE", 1), (2, 4, "UNUSABLE", 1)], 1, 3, 0))
    c.append(case("fasta_end", "a at 35, b at 38: the FASTA's c0 ends at 39, the shared column 40 is REF_OTHER for a and unusable for both; 41..43 are b's alone",
                  [pa("AAAAAA", pos=35, next_pos=38), pb("AAAAAA", pos=38, next_pos=35)],
                  [(1, cy, "A>A", 1) for cy in (1, 2, 3, 4, 5)] + [(1, 6, "REF_OTHER", 1)] + [(2, cy, "REF_OTHER", 1) for cy in (3, 2, 1)],
                  [(1, 4, "AGREE_REF", 1), (1, 5, "AGREE_REF", 1), (2, 6, "AGREE_REF", 1), (2, 5, "AGREE_REF", 1), (1, 6, "UNUSABLE", 1), (2, 4, "UNUSABLE", 1)], 1, 3, 0))
    # ---- qualities
    c.append(case("sum_passes_raw_fails", "agreeing qualities 10 and 12 under min_baseq 20: the primary table counts a with 22, the overlap table says LOWQ",
                  [pa(qual=[30] * 5 + [10]), pb(qual=[30, 30, 12, 30, 30, 30])], P2 + [(1, 6, "C>C", 1)], X2 + [(1, 6, "LOWQ", 1), (2, 4, "LOWQ", 1)], 1, 3, 0, min_baseq=20))
    c.append(case("scaled_below_min_baseq", "a's T of 25 wins against b's C of 21 and is counted as (4 x 25) / 5 = 20 under min_baseq 21: LOWQ in the primary table; both raw "
                  "qualities pass, so the overlap table keeps the error", [pa("GGGGGT", [30] * 5 + [25]), pb(qual=[30, 30, 21, 30, 30, 30])], P2 + [(1, 6, "LOWQ", 1)],
                  X2 + [(1, 6, "C>T", 1), (2, 4, "G>G", 1)], 1, 3, 1, min_baseq=21))
    c.append(case("no_qualities_agree", "a has no qualities (0xFF): it is counted and never as LOWQ although 0 + 5 is below min_baseq 20; b's raw 5 makes the column LOWQ in the "
                  "overlap table", [pa(qual="*"), pb(qual=[30, 30, 5, 30, 30, 30])], P2 + [(1, 6, "C>C", 1)], X2 + [(1, 6, "LOWQ", 1), (2, 4, "LOWQ", 1)], 1, 3, 0, min_baseq=20))
    c.append(case("no_qualities_differ", "a has no qualities (0) and reads T against b's C of 25: b wins with (4 x 25) / 5 = 20, which passes min_baseq 20",
                  [pa("GGGGGT", "*"), pb(qual=[30, 30, 25, 30, 30, 30])], P2 + [(2, 4, "G>G", 1)], X2 + [(1, 6, "C>T", 1), (2, 4, "G>G", 1)], 1, 3, 1, min_baseq=20))
    # ---- the partner's CIGAR
    c.append(case("partner_d", "a = 5M1D: column 25 is its D, not shared: a adds DEL at cycle 5, b its own C (rule W)", [pa("GGGGG", cigar="5M1D"), pb()],
                  P2 + [(1, 5, "DEL", 1), (2, 4, "G>G", 1)], X2, 1, 2, 0))
    c.append(case("partner_n_skip", "a = 5M1N1M skips 25, which b counts alone, and shares 26 with its sixth base", [pa("GGGGGC", cigar="5M1N1M"), pb()],
                  A_ALONE + [(1, 4, "G>G", 1), (1, 5, "G>G", 1), (1, 6, "C>C", 1), (2, 4, "G>G", 1), (2, 2, "G>G", 1), (2, 1, "G>G", 1)],
                  X2 + [(1, 6, "AGREE_REF", 1), (2, 3, "AGREE_REF", 1)], 1, 3, 0))
    c.append(case("insertions_in_both", "a = 4M1I2M and b = 1M1I5M, l_seq 7: every I is rule W's, one INS per mate at its own cycle; 23, 24, 25 are shared at a's cycles 4, 6, 7 "
                  "and b's 7, 5, 4", [pa("GGGGTGC", cigar="4M1I2M"), pb("GAGCCCC", cigar="1M1I5M")],
                  A_ALONE + [(1, 4, "G>G", 1), (1, 5, "INS", 1), (1, 6, "G>G", 1), (1, 7, "C>C", 1), (2, 6, "INS", 1)] + B_ALONE,
                  [(1, 4, "AGREE_REF", 1), (1, 6, "AGREE_REF", 1), (1, 7, "AGREE_REF", 1), (2, 7, "AGREE_REF", 1), (2, 5, "AGREE_REF", 1), (2, 4, "AGREE_REF", 1)], 1, 3, 0))
    c.append(case("soft_clips", "a = 2S6M and b = 6M2S, l_seq 8: a's columns are cycles 3..8, b's 8 - y", [pa("TTGGGGGC", cigar="2S6M"), pb("GGCCCCTT", cigar="6M2S")],
                  [(1, 3, "G>G", 1), (1, 4, "G>G", 1), (1, 5, "G>G", 1), (1, 6, "G>G", 1), (1, 7, "G>G", 1), (1, 8, "C>C", 1), (2, 5, "G>G", 1), (2, 4, "G>G", 1), (2, 3, "G>G", 1)],
                  [(1, 6, "AGREE_REF", 1), (1, 7, "AGREE_REF", 1), (1, 8, "AGREE_REF", 1), (2, 8, "AGREE_REF", 1), (2, 7, "AGREE_REF", 1), (2, 6, "AGREE_REF", 1)], 1, 3, 0))
    # ---- rule B
    c.append(case("bed_cuts_overlap", "the targets are 23 and 25: two shared columns, nothing else", [pa(), pb()], [(1, 4, "G>G", 1), (1, 6, "C>C", 1)],
                  [(1, 4, "AGREE_REF", 1), (1, 6, "AGREE_REF", 1), (2, 6, "AGREE_REF", 1), (2, 4, "AGREE_REF", 1)], 1, 2, 0, bed=[("c0", 23, 24), ("c0", 25, 26)]))
    c.append(case("bed_empty", "a BED without a region: two eligible records, no candidate, no counter", [pa(), pb()], [], [], 0, 0, 0, bed=[]))
    # ---- non-pairs: each record is counted as gce_bam_error_profile counts it
    c.append(case("partner_too_long", "b has 1025 bases: not eligible, a waits for it and is counted alone", [pa(), pb("T" * 1019 + "GGCCCC", cigar="1019S6M")], A_WHOLE, [], 0, 0, 0,
                  skips=dict(n_too_long=1)))
    c.append(case("contig_missing", "a pair on c2, which the FASTA lacks: neither is eligible", [pa(tid=2, pos=3, next_pos=5), pb(tid=2, pos=5, next_pos=3)], [], [], 0, 0, 0,
                  skips=dict(n_no_ref=2)))
    c.append(case("three_candidates", "a, b and a second b of one name: none pairs, n_ambiguous 3; the second b's T over C is G>A", [pa(), pb(), pb("GGTCCC")],
                  A_WHOLE + B_WHOLE + [(2, 6, "C>C", 1), (2, 5, "C>C", 1), (2, 4, "G>A", 1)] + B_ALONE, [], 0, 0, 0, ambiguous=3))
    c.append(case("supplementary_beside_pair", "a supplementary record (0x800) of the pair's name at 21 is counted alone, in segment 1, beside the pair",
                  [pa(), pa("GG", flag=0x841, pos=21, cigar="2M"), pb()], P2 + [(1, 6, "C>C", 1), (1, 1, "G>G", 1), (1, 2, "G>G", 1)],
                  X2 + [(1, 6, "AGREE_REF", 1), (2, 4, "AGREE_REF", 1)], 1, 3, 0))
    return c


def expected(cs, key="expect"):
    """the case's expect (or xexpect) list as {(segment, cycle, class name): count}"""
    out = {}
    for g, cy, cl, n in cs[key]:
        out[g, cy, cl] = out.get((g, cy, cl), 0) + n
    return out


def counters_of(cs):
    return dict(n_pairs=cs["pairs"], n_shared_columns=cs["shared"], n_disagree_columns=cs["differ"], n_ambiguous=cs["ambiguous"])


def long_cigar_pair():
    """a partner whose CIGAR has 40 ops (M, I, D, N, S, =, X, P and H among them) under a 60M mate on c1: the cursor's answer at every column
    must be fragpile::column's"""
    ops = "2S3M1I2M1D1=1X2N3M1I1M1P2M2D1M1I2=1N1X1M1I1M1D2M1N1M1I1M1D1M1I1=2M1N1M1I1M1D2M1S"
    import re
    parts = re.findall(r"(\d+)([MIDNSHP=X])", ops)
    assert len(parts) == 40
    nq = sum(int(n) for n, o in parts if o in "MIS=X")
    seq = ("ACGT" * 20)[:nq]
    b = mated(rec(1, 4, ops, seq, [(7 * k) % 41 for k in range(nq)], flag=0x91, name="lc"), 0)
    a = mated(rec(1, 0, "50M", ("ACGT" * 13)[:50], flag=0x41, name="lc"), 4)
    return [a, b]
