"""Hand-written records for gce_bam_pileup_fragments: every case names its premise and lists, written out by hand, every counter
that is not zero, every skip counter, and n_pairs, n_shared_columns, n_disagree_columns and n_ambiguous.  The model (tests/pyfragpile.py), the
per-record functions on the host (tests/fragpile_host_check.hip) and the kernels, with the LDS tile and with direct atomics, with the full
and the weak hash (tests/test_fragpile_gpu.py), are all held against these numbers.

A case is a pileupcases case (the records in coordinate order) plus pairs, shared, differ and ambiguous.  The usual shape: mate a at c0:8 with
3M over 8..10, mate b at c0:10 with 3M over 10..12, the sites c0:10 and c0:11 -- column 10 is shared, column 11 is b's alone."""
import struct

import numpy as np

import pileupcases as pc
from pileupcases import rec

NAMES, LENS = pc.NAMES, pc.LENS
T = pc.T                             # two sites: c0:10 and c0:11
A_FWD, B_REV = 0x41, 0x91            # first of the pair, forward; last of the pair, reverse


def mated(r, next_pos, next_tid=None, tlen=0):
    """a record with next_refID (default: its own refID), next_pos and tlen patched in at bytes 24..36 of the framed record"""
    b = bytearray(r)
    (tid,) = struct.unpack_from("<i", b, 4)
    struct.pack_into("<iii", b, 24, tid if next_tid is None else next_tid, next_pos, tlen)
    return bytes(b)


def ma(seq="AAC", qual=None, flag=A_FWD, pos=8, cigar="3M", next_pos=10, name="p", **kw):
    return mated(rec(0, pos, cigar, seq, qual, flag=flag, name=name, **{k: v for k, v in kw.items() if k != "next_tid"}), next_pos, kw.get("next_tid"))


def mb(seq="CGG", qual=None, flag=B_REV, pos=10, cigar="3M", next_pos=8, name="p", **kw):
    return ma(seq, qual, flag, pos, cigar, next_pos, name, **kw)


def case(label, premise, bed, records, expect, pairs, shared, differ, ambiguous=0, **kw):
    c = pc.case(label, premise, bed, records, expect, **kw)
    c.update(pairs=pairs, shared=shared, differ=differ, ambiguous=ambiguous)
    return c


NP = [(0, 10, "+", "C", 1), (0, 10, "-", "C", 1), (0, 11, "-", "G", 1)]          # a and b of the usual shape, each counted alone


def all_cases():
    c = []
    # ---- rule V, one shared column (c0:10); c0:11 is b's alone
    c.append(case("v_agree", "both mates show C at 10: a is counted, b adds nothing there", T, [ma(), mb()], [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 0))
    c.append(case("v_differ_qa_gt", "C of quality 31 against T of 30: a wins", T, [ma(qual=[30, 30, 31]), mb("TGG")], [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 1))
    c.append(case("v_differ_qa_eq", "C of quality 30 against T of 30: a wins a tie", T, [ma(), mb("TGG")], [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 1))
    c.append(case("v_differ_qa_lt", "C of quality 29 against T of 30: b wins, on its own strand", T, [ma(qual=[30, 30, 29]), mb("TGG")], [(0, 10, "-", "T", 1), (0, 11, "-", "G", 1)], 1, 1, 1))
    c.append(case("v_scaled_crosses", "a wins with quality 25, counted as (4 x 25) / 5 = 20 under min_baseq 21: LOWQ although 25 alone would pass", T,
                  [ma(qual=[30, 30, 25]), mb("TGG", [10, 30, 30])], [(0, 10, "+", "LOWQ", 1), (0, 11, "-", "G", 1)], 1, 1, 1, min_baseq=21))
    c.append(case("v_sum_crosses", "agreeing qualities 10 and 12 sum to 22 under min_baseq 20: counted although either alone would be LOWQ", T,
                  [ma(qual=[30, 30, 10]), mb(qual=[12, 30, 30])], [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 0, min_baseq=20))
    c.append(case("v_sum_cap", "agreeing qualities 150 and 150 are capped at 200 under min_baseq 201: LOWQ", T,
                  [ma(qual=[250, 250, 150]), mb(qual=[150, 250, 250])], [(0, 10, "+", "LOWQ", 1), (0, 11, "-", "G", 1)], 1, 1, 0, min_baseq=201))
    c.append(case("v_a_without_qualities_agree", "a has no qualities: it is counted, and never as LOWQ, although 0 + 5 is below min_baseq 20", T,
                  [ma(qual="*"), mb(qual=[5, 30, 30])], [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 0, min_baseq=20))
    c.append(case("v_a_without_qualities_differ", "a has no qualities (0) against T of 5: b wins with (4 x 5) / 5 = 4, LOWQ under min_baseq 20", T,
                  [ma(qual="*"), mb("TGG", [5, 30, 30])], [(0, 10, "-", "LOWQ", 1), (0, 11, "-", "G", 1)], 1, 1, 1, min_baseq=20))
    c.append(case("v_d_against_base", "a's D (quality 0) against C of 30: b wins", T, [ma("AA", cigar="2M1D"), mb()], [(0, 10, "-", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 1))
    c.append(case("v_d_against_base_q0", "a's D (quality 0) against C of 0: a wins the tie and adds DEL, which has no quality test", T,
                  [ma("AA", cigar="2M1D"), mb(qual=[0, 30, 30])], [(0, 10, "+", "DEL", 1), (0, 11, "-", "G", 1)], 1, 1, 1, min_baseq=20))
    c.append(case("v_d_against_d", "D against D: one DEL, a's", T, [ma("AA", cigar="2M1D"), mb("GG", cigar="1D2M")], [(0, 10, "+", "DEL", 1), (0, 11, "-", "G", 1)], 1, 1, 0))
    c.append(case("v_n_against_base", "a's base N of 30 against C of 30: the classes differ, a wins the tie", T, [ma("AAN"), mb()], [(0, 10, "+", "N", 1), (0, 11, "-", "G", 1)], 1, 1, 1))
    c.append(case("v_n_skip_shifts_query", "a = 1M3N2M from 5: column 10 is its third base, G, which agrees with b's G", T,
                  [ma("ACG", pos=5, cigar="1M3N2M"), mb("GTT", next_pos=5)], [(0, 10, "+", "G", 1), (0, 11, "-", "T", 1)], 1, 1, 0))
    c.append(case("v_n_skip_over_sites", "a = 1M3N1M from 8 skips 9..11: both sites are b's alone (rule W); the shared column 12 is no site", T,
                  [ma("AC", cigar="1M3N1M"), mb()], [(0, 10, "-", "C", 1), (0, 11, "-", "G", 1)], 1, 0, 0))
    c.append(case("v_soft_clip_shifts_query", "b = 2S3M: column 10 is its third base, C", T, [ma(), mb("AACGG", cigar="2S3M")], [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 0))
    c.append(case("v_insertion_in_both", "a = 3M1I1M from 8 and b = 1M1I2M from 10 agree at 10 and 11 and both insert behind 10: INS is rule W's, one per mate", T,
                  [ma("AACTG", cigar="3M1I1M"), mb("CTGG", cigar="1M1I2M")], [(0, 10, "+", "C", 1), (0, 11, "+", "G", 1), (0, 10, "+", "INS", 1), (0, 10, "-", "INS", 1)], 1, 2, 0))
    c.append(case("v_strands_swapped", "a on the reverse strand, b forward: b wins with 30 against 10 and adds on the forward strand", T,
                  [ma(qual=[30, 30, 10], flag=0x51), mb("TGG", flag=0x81)], [(0, 10, "+", "T", 1), (0, 11, "+", "G", 1)], 1, 1, 1))
    # ---- overlap geometry
    c.append(case("g_b_at_a_end_minus_1", "b.pos == a.end - 1, a the last of the pair and b the first", T, [ma(flag=0x81), mb(flag=0x51)], [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1)], 1, 1, 0))
    c.append(case("g_b_at_a_end", "b.pos == a.end: a's next_pos is not inside its span, no pair", [("c0", 9, 12)], [ma(pos=7), mb(next_pos=7)],
                  [(0, 9, "+", "C", 1), (0, 10, "-", "C", 1), (0, 11, "-", "G", 1)], 0, 0, 0))
    c.append(case("g_b_inside_a", "b = 2M at 10 inside a = 6M at 8: both sites shared, both agree", T, [ma("AACGTT", cigar="6M"), mb("CG", cigar="2M")],
                  [(0, 10, "+", "C", 1), (0, 11, "+", "G", 1)], 1, 2, 0))
    c.append(case("g_same_pos", "both at 10: the first in the file is a; C agrees, G against T of equal quality goes to a", T,
                  [ma("CG", pos=10, cigar="2M", next_pos=10), mb("CT", cigar="2M", next_pos=10)], [(0, 10, "+", "C", 1), (0, 11, "+", "G", 1)], 1, 2, 1))
    c.append(case("g_same_pos_swapped", "the same two records in the other file order: now the reverse one is a", T,
                  [mb("CT", cigar="2M", next_pos=10), ma("CG", pos=10, cigar="2M", next_pos=10)], [(0, 10, "-", "C", 1), (0, 11, "-", "T", 1)], 1, 2, 1))
    c.append(case("g_shared_on_first_site", "the shared column is the interval's first site", [("c0", 10, 13)], [ma(), mb()],
                  [(0, 10, "+", "C", 1), (0, 11, "-", "G", 1), (0, 12, "-", "G", 1)], 1, 1, 0))
    c.append(case("g_shared_on_last_site", "the shared column is the interval's last site", [("c0", 8, 11)], [ma(), mb()],
                  [(0, 8, "+", "A", 1), (0, 9, "+", "A", 1), (0, 10, "+", "C", 1)], 1, 1, 0))
    c.append(case("g_overlap_outside_sites", "a pair whose one shared column, 10, lies between two intervals: nothing for rule V to decide", [("c0", 8, 10), ("c0", 11, 13)], [ma(), mb()],
                  [(0, 8, "+", "A", 1), (0, 9, "+", "A", 1), (0, 11, "-", "G", 1), (0, 12, "-", "G", 1)], 1, 0, 0))
    # ---- non-pairs: each record is counted as gce_bam_pileup counts it
    for label, flag, ex in (("no_0x1", 0x40, 0x704), ("0x4", 0x45, 0), ("0x8", 0x49, 0x704), ("0x100", 0x141, 0), ("0x800", 0x841, 0x704), ("0x40_and_0x80", 0xC1, 0x704), ("neither_0x40_nor_0x80", 0x1, 0x704)):
        c.append(case("np_flag_" + label, "a's flag is 0x%x: no candidate" % flag, T, [ma(flag=flag), mb()], NP, 0, 0, 0, exclude=ex))
    c.append(case("np_next_refid", "a's next_refID is c1", T, [ma(next_tid=1), mb()], NP, 0, 0, 0))
    c.append(case("np_a_next_pos", "a's next_pos is 9, b lies at 10", T, [ma(next_pos=9), mb()], NP, 0, 0, 0))
    c.append(case("np_b_next_pos", "b's next_pos is 7, a lies at 8", T, [ma(), mb(next_pos=7)], NP, 0, 0, 0))
    c.append(case("np_both_first", "both records have 0x40: one group of two, no pair, nothing ambiguous", T, [ma(), mb(flag=0x51)], NP, 0, 0, 0))
    c.append(case("np_name_last_byte", "frag1 and frag2", T, [ma(name="frag1"), mb(name="frag2")], NP, 0, 0, 0))
    c.append(case("np_name_prefix", "frag and frag1: equal up to the shorter name's end", T, [ma(name="frag"), mb(name="frag1")], NP, 0, 0, 0))
    c.append(case("np_supplementary_beside_pair", "a supplementary record (0x800) of the pair's name at 9 is counted alone beside the pair", T,
                  [ma(), ma("TT", flag=0x841, pos=9, cigar="2M"), mb()], [(0, 10, "+", "C", 1), (0, 10, "+", "T", 1), (0, 11, "-", "G", 1)], 1, 1, 0))
    c.append(case("np_partner_below_min_mapq", "b's mapq 5 is below min_mapq 10: a waits for it, then is counted alone", T, [ma(), mb(mapq=5)], [(0, 10, "+", "C", 1)], 0, 0, 0,
                  skips=dict(n_low_mapq=1), min_mapq=10))
    c.append(case("np_three_candidates", "a, b and a second b of one name: none pairs, n_ambiguous 3", T, [ma(), mb(), mb("TGG")],
                  [(0, 10, "+", "C", 1), (0, 10, "-", "C", 1), (0, 10, "-", "T", 1), (0, 11, "-", "G", 2)], 0, 0, 0, ambiguous=3))
    return c


def counters_of(cs):
    return dict(n_pairs=cs["pairs"], n_shared_columns=cs["shared"], n_disagree_columns=cs["differ"], n_ambiguous=cs["ambiguous"])


ORDER_N = 120


def order_stream(k=None):
    """rule P: ORDER_N records of 100 or more incompressible bytes at c0:k/2 (so a window of 2000 compressed bytes holds fewer than 30),
    a few on c1 and two unplaced at the end; with k, record k is moved one base in front of its predecessor (or, behind the unplaced ones,
    placed).  Some index of any 40 consecutive ones is the first record of a window."""
    rng = np.random.RandomState(5)
    out = []
    for i in range(ORDER_N):
        tid, pos = (0, 10 + i // 2) if i < ORDER_N - 8 else (1, i - (ORDER_N - 8)) if i < ORDER_N - 2 else (-1, -1)
        if k == i:
            tid, pos = (0, 10 + (i - 1) // 2 - 1) if i < ORDER_N - 8 else (0, 0)
        seq = "".join("ACGT"[j] for j in rng.randint(0, 4, 80))
        out.append(rec(tid, pos, "80M", seq, rng.randint(0, 42, 80).tolist(), name="o%03d" % i))
    return out
