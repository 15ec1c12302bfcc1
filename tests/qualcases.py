"""Hand-written records for gce_bam_error_profile_quality: every case names its premise and lists, written out by hand, every
counter that is not zero.  The model (tests/pyerrqual.py), the per-record functions on the host (tests/errqual_host_check.hip) and the
kernels, on chip and with direct atomics (tests/test_errqual_gpu.py), are all held against these numbers.

A case: errprofcases' dict plus mask = None or [(contig name, start, end)], and expect = [(segment, quality bucket, class name, count)].  The
header and the FASTA are errprofcases':   c0:  0 ACGTACGTAC  10 acgtNRYKMn  20 GGGGGCCCCC  30 TTTTTAAAAA   c1: ACGT x 12, AC
On the reverse strand both bases are complemented (A>A becomes T>T); the quality index is the stored one."""
import errprofcases as ec
from errprofcases import FASTA, LENS, NAMES, rec  # noqa: F401


def case(label, premise, records, expect, mask=None, **kw):
    c = ec.case(label, premise, records, expect, **kw)
    c["mask"] = mask
    return c


def all_cases():
    c = []
    # ---- rule Q: the bucket of a byte, the record without qualities
    c.append(case("byte_edges", "6M over c0:0 with the bytes 0, 1, 93, 94, 254 and 0xFF: 0, 1 and 93 are their own rows, 94, 254 and a 0xFF behind position 0 are row 94",
                  [rec(0, 0, "6M", "ACGTAC", [0, 1, 93, 94, 254, 255])],
                  [(0, 0, "A>A", 1), (0, 1, "C>C", 1), (0, 93, "G>G", 1), (0, 94, "T>T", 1), (0, 94, "A>A", 1), (0, 94, "C>C", 1)]))
    c.append(case("no_qualities", "QUAL[0] is 0xFF: every event is in row 95 whatever the later bytes say, and none is LOWQ under min_baseq 40",
                  [rec(0, 0, "4M", "ACGT", "*"), rec(0, 0, "2M", "AC", [255, 30]), rec(0, 0, "1M1I1D1M", "AAG", [255, 3, 3])],
                  [(0, 95, "A>A", 3), (0, 95, "C>C", 2), (0, 95, "G>G", 2), (0, 95, "T>T", 1), (0, 95, "INS", 1), (0, 95, "DEL", 1)], min_baseq=40))
    c.append(case("reverse_strand_index", "4M of ACGT on the reverse strand with the qualities 10 20 30 40: the A at the stored index 0 is T>T at 10, not at 40 where its cycle's "
                  "mirror lies", [rec(0, 0, "4M", "ACGT", [10, 20, 30, 40], flag=16)], [(0, 10, "T>T", 1), (0, 20, "G>G", 1), (0, 30, "C>C", 1), (0, 40, "A>A", 1)]))
    # ---- I and D
    c.append(case("insertion_own_qualities", "1M2I1M with the qualities 30 11 12 31 on both strands: the inserted bases count at 11 and at 12",
                  [rec(0, 0, "1M2I1M", "ATTC", [30, 11, 12, 31]), rec(0, 0, "1M2I1M", "ATTC", [30, 11, 12, 31], flag=16)],
                  [(0, 30, "A>A", 1), (0, 31, "C>C", 1), (0, 11, "INS", 2), (0, 12, "INS", 2), (0, 30, "T>T", 1), (0, 31, "G>G", 1)]))
    c.append(case("deletion_behind_m", "2M1D1M with the qualities 20 21 22 on both strands: the deletion counts at 21, the quality of the base in front of it",
                  [rec(0, 0, "2M1D1M", "ACT", [20, 21, 22]), rec(0, 0, "2M1D1M", "ACT", [20, 21, 22], flag=16)],
                  [(0, 20, "A>A", 1), (0, 21, "C>C", 1), (0, 22, "T>T", 1), (0, 21, "DEL", 2), (0, 20, "T>T", 1), (0, 21, "G>G", 1), (0, 22, "A>A", 1)]))
    c.append(case("deletion_first", "1D2M: no query base stands in front of the deletion, it counts at the first base's quality, 17, on both strands",
                  [rec(0, 0, "1D2M", "CG", [17, 18]), rec(0, 0, "1D2M", "CG", [17, 18], flag=16)],
                  [(0, 17, "DEL", 2), (0, 17, "C>C", 1), (0, 18, "G>G", 1), (0, 17, "G>G", 1), (0, 18, "C>C", 1)]))
    c.append(case("deletion_behind_soft_clip", "2S1D2M with the qualities 5 6 17 18: the base in front of the deletion is the clipped one of quality 6",
                  [rec(0, 0, "2S1D2M", "TTCG", [5, 6, 17, 18])], [(0, 6, "DEL", 1), (0, 17, "C>C", 1), (0, 18, "G>G", 1)]))
    # ---- the thresholds, the mask, the BED, the segments
    c.append(case("min_baseq_splits_rows", "min_baseq 20 over the qualities 10 19 20 30: LOWQ once in row 10 and once in row 19, the bases of 20 and 30 in theirs",
                  [rec(0, 0, "4M", "ACGT", [10, 19, 20, 30])], [(0, 10, "LOWQ", 1), (0, 19, "LOWQ", 1), (0, 20, "G>G", 1), (0, 30, "T>T", 1)], min_baseq=20))
    c.append(case("masked_column_and_insertion", "c0:1 is masked: the column over it is MASKED in row 31 and the inserted base anchored there MASKED in its own row 32",
                  [rec(0, 0, "2M1I1M", "ACTG", [30, 31, 32, 33])], [(0, 30, "A>A", 1), (0, 31, "MASKED", 1), (0, 32, "MASKED", 1), (0, 33, "G>G", 1)], mask=[("c0", 1, 2)]))
    c.append(case("bed_edges", "the targets are c0:2 and 3.  6M adds its columns at 2 and 3; an insertion anchored at 2 counts, one anchored at 1 does not; a deletion at 3 counts, "
                  "one at 4 does not",
                  [rec(0, 0, "6M", "ACGTAC", [10, 11, 12, 13, 14, 15]), rec(0, 0, "3M1I1M", "ACGAT", [10, 11, 12, 13, 14]), rec(0, 0, "2M1I1M", "ACAG", [20, 21, 22, 23]),
                   rec(0, 0, "4M1D1M", "ACGTC", [40, 41, 42, 43, 44]), rec(0, 0, "3M1D1M", "ACGA", [50, 51, 52, 53])],
                  [(0, 12, "G>G", 2), (0, 13, "T>T", 1), (0, 13, "INS", 1), (0, 14, "T>T", 1), (0, 23, "G>G", 1), (0, 42, "G>G", 1), (0, 43, "T>T", 1), (0, 52, "DEL", 1),
                   (0, 52, "G>G", 1)], bed=[("c0", 2, 4)]))
    c.append(case("segments", "flags 0x40, 0x80, 0xC0 and 0: segments 1, 2, 0 and 0", [rec(0, 0, "1M", "A", [37], flag=f) for f in (0x40, 0x80, 0xC0, 0)],
                  [(1, 37, "A>A", 1), (2, 37, "A>A", 1), (0, 37, "A>A", 2)]))
    return c


def expected(cs):
    """the case's expect list as {(segment, bucket, class name): count}"""
    out = {}
    for g, b, cl, n in cs["expect"]:
        out[g, b, cl] = out.get((g, b, cl), 0) + n
    return out


def mask_of(cs, names=NAMES):
    return None if cs["mask"] is None else [(names.index(nm), a, z) for nm, a, z in cs["mask"]]


def random_records(seed, n=160):
    """reads over c1 and the FASTA's part of c0 with M, I, D, N and S ops on both strands and in all segments, every anchor inside [0, header
    length): binned qualities in most records, any byte in some, none in a few"""
    import numpy as np
    rng = np.random.RandomState(seed)
    recs = []
    for k in range(n):
        tid = int(rng.randint(0, 2))
        ops = [(4, 2)] * int(rng.randint(0, 2)) + [(int(rng.choice([0, 1, 2])), int(rng.randint(1, 4))) for _ in range(int(rng.randint(0, 2)))]
        for _ in range(int(rng.randint(1, 4))):
            ops += [(0, int(rng.randint(1, 7))), (int(rng.choice([1, 2, 3])), int(rng.randint(1, 4)))]
        ops.append((0, int(rng.randint(1, 5))))
        span = sum(ln for op, ln in ops if op in (0, 2, 3))
        pos = int(rng.randint(1, (45 if tid else 42) - min(span, 40)))
        nq = sum(ln for op, ln in ops if op in (0, 1, 4))
        kind = rng.rand()
        qual = "*" if kind < 0.08 else rng.randint(0, 256, nq).tolist() if kind < 0.25 else rng.choice([2, 11, 25, 37], nq, p=[.05, .1, .15, .7]).tolist()
        recs.append(rec(tid, pos, ops, "".join("ACGTN"[i] for i in rng.randint(0, 5, nq)), qual, flag=int(rng.choice([0, 16, 0x40, 0x90, 0x400])), mapq=int(rng.randint(0, 61))))
    return recs
