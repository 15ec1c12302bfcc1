"""Hand-written records for gce_bam_merge_overlap: every case names its premise and lists, written out by hand, the QUAL bytes of
every record after the pass and every counter.  The model (tests/pyovlmerge.py), the dual-cursor walk on the host
(tests/overlap_host_check.hip) and the kernels (tests/test_overlap_gpu.py) are all held against these bytes.

A case: dict(label, premise, records = [bytes] in coordinate order, quals = [the record's QUAL bytes afterwards, or None: unchanged], counters,
min_mapq, exclude).  The usual shape is fragcases': mate a at c0:8 with 3M over 8..10 ("AAC"), mate b at c0:10 with 3M over 10..12 ("CGG"),
every quality 30: column 10 is the one shared column, a's third base against b's first."""
import numpy as np

import fragcases as fc
import pileupcases as pc
import pypileup
from fragcases import ma, mb

NAMES, LENS = ["c0", "c1"], [1000, 500]


def case(label, premise, records, quals, pairs=1, shared=0, differ=0, skipped=0, changed=0, no_qual=0, ambiguous=0, min_mapq=0, exclude=0x704):
    assert len(quals) == len(records)
    return dict(label=label, premise=premise, records=records, quals=quals, min_mapq=min_mapq, exclude=exclude,
                counters=dict(n_records=len(records), n_pairs=pairs, n_pairs_no_qual=no_qual, n_ambiguous=ambiguous, n_shared_columns=shared, n_disagree_columns=differ,
                              n_columns_skipped=skipped, n_records_changed=changed))


def expected_records(cs):
    """the case's records with the hand-written QUAL bytes put in"""
    out = []
    for r, q in zip(cs["records"], cs["quals"]):
        if q is not None:
            f = pypileup.fields(r)
            o = 36 + r[12] + 4 * len(f["cigar"]) + (f["lseq"] + 1) // 2
            assert len(q) == f["lseq"]
            r = r[:o] + bytes(q) + r[o + len(q):]
        out.append(r)
    return out


def run_case(L):
    """a = (2 + L)M from 8, b = (L + 1)M from 10: one both-M run of L columns, column j of it a's base 2 + j against b's base j; the qualities
    differ from column to column (never 0), b's base differs from a's where j % 5 == 3"""
    sa = "AA" + "".join("ACGT"[j % 4] for j in range(L))
    sb = "".join("ACGT"[(j + (j % 5 == 3)) % 4] for j in range(L)) + "T"
    qa = [5 + j % 11 for j in range(L)]
    qb = [3 + j % 13 for j in range(L)]
    na = [qa[j] + qb[j] if j % 5 != 3 else (4 * qa[j]) // 5 if qa[j] >= qb[j] else 0 for j in range(L)]
    nb = [0 if j % 5 != 3 or qa[j] >= qb[j] else (4 * qb[j]) // 5 for j in range(L)]
    return case("run_%d" % L, "one both-M run of %d columns: %s the 16 lanes' trip" % (L, "below" if L < 16 else "exactly" if L == 16 else "beyond"),
                [ma(sa, [30, 30] + qa, cigar="%dM" % (L + 2)), mb(sb, qb + [30], cigar="%dM" % (L + 1))], [[30, 30] + na, nb + [30]], shared=L, differ=len([j for j in range(L) if j % 5 == 3]),
                changed=2)


def all_cases():
    c = []
    # ---- rule Q at one shared column (an overlap of exactly one column)
    c.append(case("q_agree", "both mates show C at 10: a carries 30 + 30, b carries 0", [ma(), mb()], [[30, 30, 60], [0, 30, 30]], shared=1, changed=2))
    c.append(case("q_differ_qa_gt", "C of 31 against T of 30: a keeps (4 x 31) / 5 = 24", [ma(qual=[30, 30, 31]), mb("TGG")], [[30, 30, 24], [0, 30, 30]], shared=1, differ=1, changed=2))
    c.append(case("q_differ_qa_eq", "C of 30 against T of 30: a wins the tie and keeps 24", [ma(), mb("TGG")], [[30, 30, 24], [0, 30, 30]], shared=1, differ=1, changed=2))
    c.append(case("q_differ_qa_lt", "C of 29 against T of 30: b keeps 24, a gets 0", [ma(qual=[30, 30, 29]), mb("TGG")], [[30, 30, 0], [24, 30, 30]], shared=1, differ=1, changed=2))
    c.append(case("q_sum_cap", "60 + 60 is capped at 93", [ma(qual=[30, 30, 60]), mb(qual=[60, 30, 30])], [[30, 30, 93], [0, 30, 30]], shared=1, changed=2))
    c.append(case("q_sum_at_cap", "46 + 47 = 93 is not capped", [ma(qual=[30, 30, 46]), mb(qual=[47, 30, 30])], [[30, 30, 93], [0, 30, 30]], shared=1, changed=2))
    c.append(case("q_scale_of_1", "C of 1 against T of 1: (4 x 1) / 5 = 0, both bytes end as 0", [ma(qual=[30, 30, 1]), mb("TGG", [1, 30, 30])], [[30, 30, 0], [0, 30, 30]], shared=1, differ=1, changed=2))
    c.append(case("q_zero_in_a", "a's quality is 0: the column is left as it is (what a second run of the pass meets)", [ma(qual=[30, 30, 0]), mb()], [None, None], shared=1, skipped=1))
    c.append(case("q_zero_in_b", "b's quality is 0 and the classes differ: left as it is", [ma(), mb("TGG", [0, 30, 30])], [None, None], shared=1, skipped=1))
    c.append(case("q_94_in_a", "a's quality is 94: left as it is, the byte never enters a sum", [ma(qual=[30, 30, 94]), mb()], [None, None], shared=1, skipped=1))
    c.append(case("q_94_in_b", "b's quality is 94", [ma(), mb(qual=[94, 30, 30])], [None, None], shared=1, skipped=1))
    c.append(case("q_93_in_both", "93 is still a quality: 93 + 93 is capped at 93", [ma(qual=[30, 30, 93]), mb(qual=[93, 30, 30])], [None, [0, 30, 30]], shared=1, changed=1))
    c.append(case("q_a_without_qualities", "a has no qualities: the pair is left alone", [ma(qual="*"), mb()], [None, None], no_qual=1))
    c.append(case("q_b_without_qualities", "b has no qualities", [ma(), mb(qual="*")], [None, None], no_qual=1))
    c.append(case("q_n_against_base", "a's N of 30 against C of 30: the classes differ, a wins the tie", [ma("AAN"), mb()], [[30, 30, 24], [0, 30, 30]], shared=1, differ=1, changed=2))
    c.append(case("q_n_against_n", "N against N: one class, the qualities are summed", [ma("AAN"), mb("NGG")], [[30, 30, 60], [0, 30, 30]], shared=1, changed=2))
    c.append(case("q_other_codes_are_n", "a's M (amino) against b's R (purine): both are class N", [ma("AAM"), mb("RGG")], [[30, 30, 60], [0, 30, 30]], shared=1, changed=2))
    # ---- the overlap's geometry
    c.append(case("g_b_inside_a", "b = 2M at 10 inside a = 6M at 8: two shared columns, both agree", [ma("AACGTT", cigar="6M"), mb("CG", cigar="2M")], [[30, 30, 60, 60, 30, 30], [0, 0]], shared=2, changed=2))
    c.append(case("g_same_end", "a = 4M from 8 and b = 2M from 10 end on the same column", [ma("AACG", cigar="4M"), mb("CG", cigar="2M")], [[30, 30, 60, 60], [0, 0]], shared=2, changed=2))
    c.append(case("g_same_pos", "both at 10: the first in the file is a; C agrees, G against T of equal quality goes to a",
                  [ma("CG", pos=10, cigar="2M", next_pos=10), mb("CT", cigar="2M", next_pos=10)], [[60, 24], [0, 0]], shared=2, differ=1, changed=2))
    c.append(case("g_same_pos_swapped", "the same two records in the other file order: now the reverse one is a",
                  [mb("CT", cigar="2M", next_pos=10), ma("CG", pos=10, cigar="2M", next_pos=10)], [[60, 24], [0, 0]], shared=2, differ=1, changed=2))
    c.append(case("g_b_at_a_end_minus_1", "a the last of the pair and reverse, b the first and forward: flags do not decide who is a", [ma(flag=0x91), mb(flag=0x41)], [[30, 30, 60], [0, 30, 30]],
                  shared=1, changed=2))
    c.append(case("g_odd_offsets", "a = 4M from 9, b = 4M from 10: a's bases 1, 2, 3 against b's 0, 1, 2 -- both nibbles of a byte in both mates",
                  [ma("ACGT", [11, 12, 13, 14], pos=9, cigar="4M"), mb("CGTA", [21, 22, 23, 24], cigar="4M", next_pos=9)], [[11, 33, 35, 37], [0, 0, 0, 24]], shared=3, changed=2))
    # ---- the other ops, inside and at the edges of the overlap
    c.append(case("o_i_in_a", "a = 3M1I1M: the inserted base keeps its quality, column 11 is a's base 4", [ma("AACTG", cigar="3M1I1M"), mb()], [[30, 30, 60, 30, 60], [0, 0, 30]], shared=2, changed=2))
    c.append(case("o_i_in_a_at_b_start", "a = 2M1I2M: the insertion lies right in front of b's first column; 10 and 11 are a's bases 3 and 4", [ma("AATCG", cigar="2M1I2M"), mb()],
                  [[30, 30, 30, 60, 60], [0, 0, 30]], shared=2, changed=2))
    c.append(case("o_i_at_b_start", "b = 1I2M: its first base is inserted and untouched; 10 and 11 are its bases 1 and 2", [ma("AACG", cigar="4M"), mb("TCG", cigar="1I2M")],
                  [[30, 30, 60, 60], [30, 0, 0]], shared=2, changed=2))
    c.append(case("o_b_starts_in_a_deletion", "a = 2M2D2M deletes 10 and 11, where b = 4M starts: those two are not touched; 12 agrees, 13 is G against T",
                  [ma("AAGG", cigar="2M2D2M"), mb("CGGT", cigar="4M")], [[30, 30, 60, 24], [30, 30, 0, 0]], shared=2, differ=1, changed=2))
    c.append(case("o_d_in_b", "b = 1M1D1M deletes 11: a's base there keeps its quality", [ma("AACTG", cigar="5M"), mb("CG", cigar="1M1D1M")], [[30, 30, 60, 30, 60], [0, 0]], shared=2, changed=2))
    c.append(case("o_n_in_b", "b = 1M2N2M skips 11 and 12: column 13 is a's base 5 against b's base 1", [ma("AACGTG", cigar="6M"), mb("CGT", cigar="1M2N2M")],
                  [[30, 30, 60, 30, 30, 60], [0, 0, 30]], shared=2, changed=2))
    c.append(case("o_n_in_a_over_b", "a = 1M3N1M skips 9..11: the one shared column is 12, a's base 1 against b's base 2", [ma("AG", cigar="1M3N1M"), mb()], [[30, 60], [30, 30, 0]], shared=1, changed=2))
    c.append(case("o_soft_clips", "a = 3M2S and b = 2S3M: the clips shift b's query by two and are not touched", [ma("AACTT", cigar="3M2S"), mb("AACGG", cigar="2S3M")],
                  [[30, 30, 60, 30, 30], [30, 30, 0, 30, 30]], shared=1, changed=2))
    c.append(case("o_hard_clips", "H moves nothing", [ma(cigar="2H3M"), mb(cigar="3M2H")], [[30, 30, 60], [0, 30, 30]], shared=1, changed=2))
    c.append(case("o_eq_and_x", "= and X are M", [ma(cigar="2=1X"), mb(cigar="1X2=")], [[30, 30, 60], [0, 30, 30]], shared=1, changed=2))
    c.append(case("o_d_against_d", "both delete column 10: nothing is shared there; 11 is", [ma("AAG", cigar="2M1D1M"), mb("G", pos=10, cigar="1D1M")], [[30, 30, 60], [0]], shared=1, changed=2))
    c.append(case("o_zero_length_ops", "0M and 0D in front of the shared column move nothing", [ma(cigar="2M0D0M1M"), mb(cigar="0M3M")], [[30, 30, 60], [0, 30, 30]], shared=1, changed=2))
    # ---- runs at the 16 lanes' trip, long reads, long CIGARs
    for L in (15, 16, 17, 33):
        c.append(run_case(L))
    c.append(case("r_300_bases", "two reads of 300 bases 100 apart: 200 shared columns, all agree", [ma("A" * 300, cigar="300M", next_pos=108), mb("A" * 300, pos=108, cigar="300M")],
                  [[30] * 100 + [60] * 200, [0] * 200 + [30] * 100], shared=200, changed=2))
    c.append(case("r_19_ops", "a = (2M1I) x 9 + 2M, 19 ops over 8..27, against b = 18M from 10: a's columns 8 + 2i and 9 + 2i are its bases 3i and 3i + 1",
                  [ma("A" * 29, cigar="2M1I" * 9 + "2M"), mb("A" * 18, cigar="18M")], [[30, 30, 30] + [60, 60, 30] * 8 + [60, 60], [0] * 18], shared=18, changed=2))
    # ---- no pair: nothing is touched
    c.append(case("np_three_candidates", "a, b and a second b of one name: none pairs, n_ambiguous 3", [ma(), mb(), mb("TGG")], [None, None, None], pairs=0, ambiguous=3))
    c.append(case("np_supplementary_beside_pair", "a supplementary record (0x800) of the pair's name is no candidate; the pair is merged around it",
                  [ma(), ma("TT", flag=0x841, pos=9, cigar="2M"), mb()], [[30, 30, 60], None, [0, 30, 30]], shared=1, changed=2))
    c.append(case("np_duplicate_mate", "b is a duplicate (0x400): excluded by 0x704, a stays alone", [ma(), mb(flag=0x491)], [None, None], pairs=0))
    c.append(case("np_duplicate_mate_included", "the same two records with exclude_flags 0x304: a pair", [ma(), mb(flag=0x491)], [[30, 30, 60], [0, 30, 30]], shared=1, changed=2, exclude=0x304))
    c.append(case("np_other_contig", "b lies on c1 and each names the other's contig", [ma(next_tid=1), fc.mated(pc.rec(1, 10, "3M", "CGG", flag=fc.B_REV, name="p"), 8, next_tid=0)], [None, None], pairs=0))
    c.append(case("np_next_pos_at_end", "a's next_pos is its own end: no candidate", [ma(pos=7), mb(next_pos=7)], [None, None], pairs=0))
    c.append(case("np_next_pos_beyond_end", "a's next_pos lies behind its end", [ma(pos=5), mb(next_pos=5)], [None, None], pairs=0))
    c.append(case("np_partner_missing", "a's mate is not in the file; a single read covers the same columns", [ma(), pc.rec(0, 10, "3M", "CGG", name="single")], [None, None], pairs=0))
    c.append(case("np_partner_below_min_mapq", "b's mapq 5 is below min_mapq 10", [ma(), mb(mapq=5)], [None, None], pairs=0, min_mapq=10))
    c.append(case("np_both_first", "both records have 0x40: a group of two that is no pair", [ma(), mb(flag=0x51)], [None, None], pairs=0))
    c.append(case("np_unpaired_flag", "a lacks 0x1", [ma(flag=0x40), mb()], [None, None], pairs=0))
    return c


def renamed(r, suffix):
    """the record under its name + suffix"""
    b = bytearray(r)
    new = bytes(b[36:36 + b[12] - 1]) + suffix + b"\0"
    b = b[:36] + new + bytes(b[36 + b[12]:])
    b[12] = len(new)
    b[0:4] = (len(b) - 4).to_bytes(4, "little")
    return bytes(b)


def combined_stream(exclude=0x704, min_mapq=0):
    """the records of every case with these thresholds as one sorted stream under distinct names"""
    recs = []
    for k, cs in enumerate(c for c in all_cases() if c["min_mapq"] == min_mapq and c["exclude"] == exclude):
        recs += [renamed(r, b"_%02d" % k) for r in cs["records"]]
    order = sorted(range(len(recs)), key=lambda i: (pypileup.fields(recs[i])["tid"], pypileup.fields(recs[i])["pos"], i))
    return [recs[i] for i in order]


def fuzz_pairs(n, seed, read_len=(20, 60), indels=True):
    """n fragments on c0 as overlapping pairs with mismatches, qualities in 1..60 and, with indels, an insertion or a soft clip in some reads
    (never a D or N op: the premise of the pileup cross-check), sorted; names are unique"""
    rng = np.random.RandomState(seed)
    ref = rng.randint(0, 4, LENS[0])
    recs = []
    for i in range(n):
        la, lb = int(rng.randint(*read_len)), int(rng.randint(*read_len))
        s = int(rng.randint(0, LENS[0] - 2 * read_len[1] - 4))
        sb = s + int(rng.randint(0, la))                                             # b starts inside a
        out = []
        for first, at, ln in ((True, s, la), (False, sb, lb)):
            b = ref[at:at + ln].copy()
            hit = rng.rand(ln) < 0.1
            b[hit] = rng.randint(0, 4, int(hit.sum()))
            seq = "".join("ACGT"[j] for j in b)
            cigar = "%dM" % ln
            kind = int(rng.randint(0, 4)) if indels and ln > 8 else 0
            if kind == 1:                                                            # an insertion of two bases somewhere inside
                k = int(rng.randint(2, ln - 2))
                seq, cigar = seq[:k] + "GT" + seq[k:], "%dM2I%dM" % (k, ln - k)
            elif kind == 2:                                                          # soft clips at both ends
                seq, cigar = "TT" + seq + "C", "2S%dM1S" % ln
            out.append((at, seq, cigar, first))
        (pa, qa_seq, ca, _), (pb, qb_seq, cb, _) = out
        for (at, seq, cigar, first), other in ((out[0], pb), (out[1], pa)):
            recs.append((at, len(recs), fc.mated(pc.rec(0, at, cigar, seq, rng.randint(1, 61, len(seq)).tolist(), flag=0x61 if first else 0x91, name="z%06d" % i), other)))
    recs.sort(key=lambda t: t[:2])
    return [r for _, _, r in recs]
