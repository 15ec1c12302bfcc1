#!/usr/bin/env python
"""Writes tied_quality_thresholds_score_by_the_swar_count.json.  A WRITING AID, not an oracle: the `expected` block and the derivation were
worked out by hand from the cited reference lines; no oracle or engine run is involved."""
import json, os
HERE = os.path.dirname(os.path.abspath(__file__))

UNIT = "ACGTTGCAAGCTTCGA"                  # the contig: UNIT x 100 (1600 bases)
REF = (UNIT * 100)[1000:1016]              # the left reads' 16 positions: AGCTTCGAACGTTGCA
RREF = (UNIT * 100)[1200:1216]
ALT = {"A": "C", "C": "G", "G": "T", "T": "A"}
R, X = "R", "X"
# column -> (bases of a, b, c, d as R = reference / X = ALT[reference], their qualities)
COLS = {0: ("RRRR", (26, 26, 26, 26)), 1: ("RRXR", (24, 24, 25, 24)), 2: ("XXRR", (26, 26, 25, 24)), 3: ("XXXX", (24, 24, 24, 24)),
        4: ("XXXX", (25, 24, 24, 24)), 5: ("RRRR", (24, 24, 24, 24)), 6: ("XXXR", (24, 24, 24, 26)), 7: ("RRXR", (25, 24, 25, 24))}
assert REF == "AGCTTCGAACGTTGCA"


def read(k):
    seq, qual = [], []
    for i in range(16):
        b, q = COLS.get(i, ("RRRR", (26, 26, 26, 26)))
        seq.append(REF[i] if b[k] == R else ALT[REF[i]]); qual.append(q[k])
    return "".join(seq), qual


def rec(qname, flag, pos, mpos, isize, seq, qual, nm):
    return dict(qname=qname, flag=flag, tid=0, pos=pos, cigar="16M", mtid=0, mpos=mpos, isize=isize, seq=seq, qual=qual, nm=nm)


records = []
for k, name in enumerate("abcd"):
    s, q = read(k)
    records.append(rec(name, 99, 1000, 1200, 216, s, q, sum(1 for x, y in zip(s, REF) if x != y)))
for name in "abcd":
    records.append(rec(name, 147, 1200, 1000, -216, RREF, [37] * 16, 0))

out_seq = "".join(ALT[REF[i]] if i in (1, 4) else REF[i] for i in range(16))
out_qual = [26, 25, 25, 0, 25, 24, 26, 25] + [26] * 8
v = dict(
    name="tied_quality_thresholds_score_by_the_swar_count",
    cites=["src/options.cpp:72-100", "src/pair.cpp:77-86", "src/pair.cpp:88-131", "src/group.cpp:196-261", "src/group.cpp:381-501", "src/group.cpp:503-573"],
    derivation=(
        "--high_qual 25 --moderate_qual 25 --low_qual 25 (equal thresholds are allowed: options.cpp:72-100) and baseScoreReq 8, default scores 8/6/4/2.  "
        "qual2score (pair.cpp:77-86) then gives 8 to every quality >= 25 and 2 to every quality < 25: of the qualities 24, 25, 26 used here, 25 and 26 score 8 and 24 "
        "scores 2 (a count of thresholds passed that reads `>` for `>=` scores 25 as 2).  One cluster (0, 1000, 1215), four pairs a, b, c, d, no UMI: left reads 16M at "
        "1000, right reads 16M at 1200, isize 216.  The mates do not overlap: posDis = 200, cmpLen = min(16 - 200, 16) < 0, so every base scores qual2score of its own "
        "quality (pair.cpp:108-131).  Reads identical in CIGAR and length: the first in qname order, a, is the template of both sides; all four vote (group.cpp:196-261).  "
        "The contig is ACGTTGCAAGCTTCGA x 100: positions 1000..1015 read AGCTTCGAACGTTGCA.  Below R is the reference base of the column, X = the next base of ACGT "
        "after it (A->C, C->G, G->T, T->A); qualities of a, b, c, d in that order.  "
        "Column 0: R R R R, 26 26 26 26: secNum 0, 32 >= 8, topQual 26 >= 25: accepted, R q26.  "
        "Column 1: R R X R, 24 24 25 24: R scores 2+2+2 = 6, X scores 8: top X (8), second R with secNum 3 > 1 and 8 < 0.8 x 14 = 11.2: needToCheckRef (group.cpp:460-464).  "
        "No read with R reaches highQuality 25 and topQual 25 is not < moderate 25: X stays, with topQual 25.  a's base R becomes X: diff, out base == reference: mismatchInc +1.  "
        "(Were 25 scored as 2: top R (6), second X with secNum 1 and quals 25 <= low 25, topNum 3; but 6 < 8 and topQual 24 <= 25 check the reference: topQual 24 < 25 gives "
        "R with quality 24.)  "
        "Column 2: X X R R, 26 26 25 24: X 16, R 8 + 2 = 10: top X, second R with secNum 2 and 16 < 0.8 x 26 = 20.8: needToCheckRef; read c shows R with quality 25 >= high 25: "
        "topBase = R, topQual = the largest quality of an R read = 25 (group.cpp:470-501).  a's X becomes R: mismatchInc -1.  (With 25 scored as 2: 16 < 0.8 x 20 is false, 16 >= 8, "
        "topQual 26 > 25: X q26 would stay.)  "
        "Column 3: X X X X, 24 24 24 24: secNum 0, topScore 8 == baseScoreReq 8 but topQual 24 < 25: not accepted; reference R, no read shows it: refBaseQual 0; topQual 24 < 25: "
        "topBase = R with quality 0.  a's X becomes R: mismatchInc -1.  "
        "Column 4: X X X X, 25 24 24 24: secNum 0, 8 + 2 + 2 + 2 = 14 >= 8, topQual 25 >= 25: accepted (`continue` before any base is written): X q25 stays in a.  "
        "Column 5: R R R R, 24 x 4: 8 >= 8 but topQual 24 < 25: reference R, refBaseQual 24, topQual < 25: R with quality 24.  "
        "Column 6: X X X R, 24 24 24 26: X 6, R 8: top R, second X with secNum 3 and 8 < 0.8 x 14: needToCheckRef; d shows R at 26 >= 25: R, quality 26.  a's X becomes R: "
        "mismatchInc -1.  "
        "Column 7: R R X R, 25 24 25 24: R 8 + 2 + 2 = 12, X 8: top R, second X with secNum 1, quals 25 <= low 25, topNum 3 >= 2; then topQual 25 <= low 25: needToCheckRef; "
        "a shows R at 25: R, refBaseQual 25.  "
        "Columns 8..15: R x 4 at 26: accepted.  "
        "Left consensus: a's bases with columns 1 and 4 off the reference, qualities 26 25 25 0 25 24 26 25 and 26 x 8.  mismatchInc = +1 - 1 - 1 - 1 = -2, a's NM 4 (columns "
        "2, 3, 4, 6) is 'C': 2 (group.cpp:528-573).  Right side: four identical reads at quality 37 matching the reference: accepted everywhere, template a, NM 0.  "
        "Both records leave with a's name and FR = 4."),
    params=dict(high_quality=25, moderate_quality=25, low_quality=25, base_score_req=8),
    contigs=[dict(name="c0", length=1600, sequence=dict(repeat=UNIT, times=100))],
    records=records,
    expected_status=0,
    expected=[dict(qname="a", flag=99, tid=0, pos=1000, cigar="16M", seq=out_seq, qual=out_qual, nm=2, fr=4, rr=-1),
              dict(qname="a", flag=147, tid=0, pos=1200, cigar="16M", seq=RREF, qual=[37] * 16, nm=0, fr=4, rr=-1)],
)
with open(os.path.join(HERE, v["name"] + ".json"), "w") as f:
    json.dump(v, f, indent=1)
    f.write("\n")
