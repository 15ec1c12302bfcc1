"""gce_bam_pileup_fragments on the GPU: the order check and the join (k_frag_prep, k_frag_join), k_frag_count with the LDS tile and
with direct atomics, with the full and the weak hash where the join is the subject, and the carry across windows, against the model
(tests/pyfragpile.py) and the hand-written counters (tests/fragcases.py): every integer equal.  The cases are the smallest at which the
kernels can go wrong: rule V column by column, the overlap's geometry, every way not to be a pair, a pair across a 16-record block, mates on a tile's edge, 300
pairs at one locus, mates in different windows and every way a waiting record expires, rule P inside a window and on a window's first
record, the budget, one generated paired stream, the table's bytes and the command line."""
import os
import re

import numpy as np
import pytest

import fragcases as fc
import pileupcases as pc
import pyfragpile
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"#define PU_TILE (\d+)u", open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_pileup.hpp")).read()).group(1))
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["tile", "direct"])
HASHES = pytest.mark.parametrize("weak", [False, True], ids=["hash", "weak_hash"])
BIG = (["c0", "c1"], [20000, 3000])


def same(run, res, deferred=None):
    """a run against the model's dict: the sites, every counter, every skip, rule M's and rule V's counters"""
    assert run.n_sites == res["n_sites"] and run.n_intervals == res["n_intervals"]
    assert run.tid.tolist() == res["tid"] and run.pos.tolist() == res["pos"]
    assert run.counts.dtype == np.uint32 and run.counts.shape == (res["n_sites"], 2, 8)
    for k in ["n_records", "n_eligible"] + pypileup.SKIPS + pyfragpile.FRAG_COUNTERS:
        assert getattr(run, k) == res[k], k
    got = run.counts.reshape(-1, 16).tolist()
    assert got == res["counts"], [(i, g, w) for i, (g, w) in enumerate(zip(got, res["counts"])) if g != w][:5]
    if deferred is not None:
        assert run.n_deferred == deferred


def run_files(tmp_path, records, bed, names, lens, direct, weak=False, tag="x", block=0xff00, **kw):
    """records (bytes) and bed = [(contig name, start, end)] as files, through pileup_fragments_bam -> (the run, the model's result)"""
    from gencore_amd.bamio import pileup_fragments_bam
    bam, bedf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.bed" % tag)
    if not bam.exists():
        pc.write_raw_bam(str(bam), records, names, lens, block)
        bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    run = pileup_fragments_bam(bam, bedf, direct=direct, weak_hash=weak, threads=2, **kw)
    regions = [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    res = pyfragpile.pileup_fragments(records, regions, lens, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704))
    return run, res


@pytest.mark.gpu
@VARIANTS
@HASHES
def test_hand_cases(built, tmp_path, direct, weak):
    """every case of fragcases: rule V, the geometry, the non-pairs -- the counters written out by hand"""
    for cs in fc.all_cases():
        run, res = run_files(tmp_path, cs["records"], cs["bed"], pc.NAMES, pc.LENS, direct, weak, tag=cs["label"], min_mapq=cs["min_mapq"], min_baseq=cs["min_baseq"],
                             exclude_flags=cs["exclude"])
        same(run, res, deferred=0)
        assert run.counts.reshape(-1, 16).tolist() == pc.expected_counts(cs, list(zip(res["tid"], res["pos"]))), cs["label"]
        assert {k: getattr(run, k) for k in pypileup.SKIPS} == cs["skips"], cs["label"]
        assert {k: getattr(run, k) for k in pyfragpile.FRAG_COUNTERS} == fc.counters_of(cs), cs["label"]


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("n", [15, 16, 17])
def test_pair_at_a_block_edge(built, tmp_path, direct, n):
    """n - 2 single reads, then a pair as the last two records: with 17 records a is the last entry of one 16-entry block and b the first of
    the next; with 15 and 16 the pair ends a partial and a whole block"""
    recs = [pc.rec(0, 5 + k // 5, "6M", "ACGTAC"[k % 3:] + "ACGTAC"[:k % 3], flag=16 * (k & 1), name="s%02d" % k) for k in range(n - 2)] + [fc.ma(qual=[30, 30, 20]), fc.mb("TGG")]
    run, res = run_files(tmp_path, recs, fc.T, pc.NAMES, pc.LENS, direct)
    same(run, res, deferred=0)
    assert (run.n_pairs, run.n_shared_columns, run.n_disagree_columns) == (1, 1, 1)


@pytest.mark.gpu
@VARIANTS
@HASHES
def test_300_pairs_at_one_locus(built, tmp_path, direct, weak):
    """300 pairs whose names differ in one digit, every a at c0:8 and every b at c0:10: one probe run under the weak hash, 600 entries on two
    sites of one tile"""
    rng = np.random.RandomState(3)
    a = [fc.ma("AA" + "ACGT"[rng.randint(4)], [30, 30, int(rng.randint(0, 41))], name="frag%03d" % k) for k in range(300)]
    b = [fc.mb("ACGT"[rng.randint(4)] + "GG", [int(rng.randint(0, 41)), 30, 30], name="frag%03d" % k) for k in range(300)]
    run, res = run_files(tmp_path, a + b[::-1], fc.T, pc.NAMES, pc.LENS, direct, weak, min_baseq=13)
    assert res["n_pairs"] == 300 == res["n_shared_columns"] and 150 < res["n_disagree_columns"] < 300 and res["n_ambiguous"] == 0
    same(run, res, deferred=0)


def tile_edge_records():
    """one sorted block of 6 entries on one interval [0, 3 TILE) of c0 of BIG.  The first record lies at pos 100, so the block's tile holds
    the sites [99, 99 + TILE).  Pair `edge` shares the four columns e - 2 .. e + 1 around the tile's end e = 99 + TILE: they agree at e - 2
    and e (a is counted, inside and behind the tile), differ at e - 1 (b is of higher quality: the later mate adds to the tile's last site)
    and at e + 1 (a is: the earlier mate adds behind the tile).  Pair `far` shares two columns behind an N skip of 2 TILE, one agreeing and
    one not.  A single read ends exactly on the tile's last site."""
    e = 99 + TILE
    return [pc.rec(0, 100, "3M", "ACG", name="first"),
            fc.ma("ACGT", pos=101, cigar="1M%dN3M" % (2 * TILE), next_pos=103 + 2 * TILE, name="far"),
            fc.ma("ACGTAC", [30] * 6, pos=e - 4, cigar="6M", next_pos=e - 2, name="edge"),
            pc.rec(0, e - 3, "3M", "CCC", name="single"),
            fc.mb("GAAGTT", [40, 40, 30, 20, 30, 30], pos=e - 2, cigar="6M", next_pos=e - 4, name="edge"),
            fc.mb("GAT", pos=103 + 2 * TILE, cigar="3M", next_pos=101, name="far")]


@pytest.mark.gpu
@VARIANTS
def test_paired_mates_at_the_tile_edges(built, tmp_path, direct):
    """rule V's adds on the last site of a block's tile, on the first site behind it and far behind it over an N skip, by either mate: the
    model's counters, and the tile and the direct kernel agree"""
    e = 99 + TILE
    bed = [("c0", 0, 3 * TILE)]
    recs = tile_edge_records()
    assert len(recs) <= 16
    run, res = run_files(tmp_path, recs, bed, *BIG, direct)
    assert (res["n_pairs"], res["n_shared_columns"], res["n_disagree_columns"]) == (2, 6, 3)
    same(run, res, deferred=0)
    assert run.n_shared_columns == res["n_shared_columns"] and run.n_disagree_columns == res["n_disagree_columns"]
    c = run.counts.reshape(-1, 16)
    assert c[e - 1].sum() > 0 and c[e].sum() > 0 and c[103 + 2 * TILE].sum() > 0
    assert c[e - 1].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]      # the single read's C; b's A, reverse, over a's T
    assert c[e].tolist() == [1] + [0] * 15 and c[e + 1].tolist() == [0, 1] + [0] * 14   # a's A where they agree; a's C over b's G
    other, _ = run_files(tmp_path, recs, bed, *BIG, not direct)
    assert (other.counts == run.counts).all() and other.n_shared_columns == run.n_shared_columns and other.n_disagree_columns == run.n_disagree_columns


def window_stream(tail):
    """a sorted stream on BIG: overlapping pairs 20 bases apart; every 25th a is 40M2000N40M with its b 2040 bases on, so it waits through many
    windows; every 30th b is missing, so its a expires when the records pass its next_pos; a lonely a is the last record of c0 (the contig
    changes) and of c1 (the file ends, or `tail` unplaced records follow)"""
    rng = np.random.RandomState(7)
    bases = lambda n: "".join("ACGT"[j] for j in rng.randint(0, 4, n))
    recs = []
    for i in range(190):
        tid, s = (0, 100 + 20 * i) if i < 170 else (1, 100 + 20 * (i - 170))
        L = int(rng.randint(90, 141))
        frag = bases(L)
        q = lambda: rng.randint(2, 41, 80).tolist()
        mut = lambda t: "".join(c if rng.rand() > 0.05 else "ACGT"[rng.randint(4)] for c in t)
        nm = "w%04d" % i
        if i % 25 == 3:
            recs.append((tid, s, fc.mated(pc.rec(tid, s, "40M2000N40M", mut(frag[:80]), q(), flag=0x61, name=nm), s + 2040)))
            recs.append((tid, s + 2040, fc.mated(pc.rec(tid, s + 2040, "80M", mut(frag[:80]), q(), flag=0x91, name=nm), s)))
            continue
        recs.append((tid, s, fc.mated(pc.rec(tid, s, "80M", mut(frag[:80]), q(), flag=0x61, name=nm), s + L - 80)))
        if i % 30 != 7:
            recs.append((tid, s + L - 80, fc.mated(pc.rec(tid, s + L - 80, "80M", mut(frag[L - 80:]), q(), flag=0x91, name=nm), s)))
    recs.append((0, 15000, fc.mated(pc.rec(0, 15000, "80M", bases(80), flag=0x61, name="endc0"), 15050)))
    recs.append((1, 2500, fc.mated(pc.rec(1, 2500, "80M", bases(80), flag=0x61, name="endc1"), 2550)))
    recs.sort(key=lambda t: t[:2])
    return [r for _, _, r in recs] + [pc.rec(-1, -1, "80M", bases(80), name="u%d" % k) for k in range(tail)]


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("tail", [0, 3], ids=["ends_placed", "ends_unplaced"])
def test_mates_in_different_windows(built, tmp_path, direct, tail):
    """members of 300 bytes and windows of 2000: a in one window and b in the next, a waiting through many windows, b cut between windows, and
    a expiring by position, by contig, by an unplaced record and by the end of the file; the result equals the one-window result and the model's"""
    recs = window_stream(tail)
    bed = [("c0", 50, 9000), ("c0", 14990, 15100), ("c1", 0, 3000)]
    one, res = run_files(tmp_path, recs, bed, *BIG, direct, block=300, min_baseq=13)
    assert res["n_pairs"] > 150 and res["n_shared_columns"] > 5000 and res["n_disagree_columns"] > 100 and res["n_unplaced"] == tail
    same(one, res, deferred=0)
    cut, _ = run_files(tmp_path, recs, bed, *BIG, direct, block=300, min_baseq=13, window_bytes=2000)
    same(cut, res)
    assert (cut.counts == one.counts).all() and cut.n_deferred > 20
    weak, _ = run_files(tmp_path, recs, bed, *BIG, direct, weak=True, block=300, min_baseq=13, window_bytes=2000)
    same(weak, res, deferred=cut.n_deferred)


@pytest.mark.gpu
@VARIANTS
def test_rule_p(built, tmp_path, direct):
    """a record in front of its predecessor is named by its index, inside a window and as the first record of a window: of 40 consecutive
    offenders at least one opens a window of 2000 compressed bytes (fragcases.order_stream); the malformed-record refusal comes first; no
    table and no temporary file is left"""
    from gencore_amd.bamio import pileup_fragments_bam
    from gencore_amd.capi import GceError
    (tmp_path / "t.bed").write_text("c0\t0\t100\n")
    bam = tmp_path / "in.bam"
    for k, wb in [(37, 0), (fc.ORDER_N - 8, 0), (fc.ORDER_N - 1, 0)] + [(k, 2000) for k in range(40, 80)] + [(fc.ORDER_N - 2, 2000)]:
        pc.write_raw_bam(str(bam), fc.order_stream(k), block=300)
        with pytest.raises(GceError) as ei:
            pileup_fragments_bam(bam, tmp_path / "t.bed", tsv=tmp_path / "out.tsv", direct=direct, window_bytes=wb)
        assert ei.value.status == -1 and str(ei.value).endswith("BAM record %d (counting from 0) lies in front of its predecessor: gce_bam_pileup_fragments needs a coordinate-sorted file" % k), (k, wb)
    recs = fc.order_stream(60)
    pc.write_raw_bam(str(bam), recs[:70] + [pc.malformed()[0][1]] + recs[70:])
    with pytest.raises(GceError) as ei:
        pileup_fragments_bam(bam, tmp_path / "t.bed", tsv=tmp_path / "out.tsv", direct=direct)
    assert ei.value.status == -1 and "BAM record 70 (counting from 0): its fields overrun its block_size" in str(ei.value)
    pc.write_raw_bam(str(bam), fc.order_stream(), block=300)
    run = pileup_fragments_bam(bam, tmp_path / "t.bed", direct=direct, window_bytes=2000)
    assert run.n_records == fc.ORDER_N and run.n_unplaced == 2
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "t.bed"]


@pytest.mark.gpu
@VARIANTS
def test_no_candidates_is_pileup_bam(built, tmp_path, direct):
    """a sorted file without a paired flag: every counter is gce_bam_pileup's, through windows too"""
    from gencore_amd.bamio import pileup_bam
    rng = np.random.RandomState(11)
    recs = []
    for k in range(400):
        n = int(rng.randint(20, 120))
        recs.append(pc.rec(int(k >= 300), 6 * (k % 300) + int(rng.randint(0, 6)), "%dM" % n, "".join("ACGTN"[i] for i in rng.randint(0, 5, n)), rng.randint(0, 41, n).tolist(),
                           flag=16 * int(rng.randint(0, 2)), name="read%04d" % k))
    bed = [("c0", 50, 400), ("c0", 1000, 1300), ("c1", 0, 3000)]
    run, res = run_files(tmp_path, recs, bed, *BIG, direct, block=300, min_baseq=13, window_bytes=2000)
    same(run, res, deferred=0)
    ref = pileup_bam(tmp_path / "x.bam", tmp_path / "x.bed", direct=direct, min_baseq=13, window_bytes=2000)
    assert (ref.counts == run.counts).all() and ref.counts.sum() > 2000 and run.n_pairs == run.n_shared_columns == run.n_ambiguous == 0
    for k in ["n_records", "n_eligible"] + pypileup.SKIPS:
        assert getattr(ref, k) == getattr(run, k)


def paired_stream(n_frag, seed):
    """n_frag fragments of 60..250 bases on c0 of BIG as pairs of reads of 100 (a fragment below 100: two reads of its length), with
    mismatches and varied qualities, sorted"""
    rng = np.random.RandomState(seed)
    ref = rng.randint(0, 4, 20000)
    recs = []
    for i in range(n_frag):
        L = int(rng.randint(60, 251))
        s = int(rng.randint(0, 19000))
        n = min(100, L)
        for first, at in ((True, s), (False, s + L - n)):
            b = ref[at:at + n].copy()
            hit = rng.rand(n) < 0.02
            b[hit] = rng.randint(0, 4, int(hit.sum()))
            seq = "".join("ACGT"[j] for j in b)
            recs.append((at, not first, fc.mated(pc.rec(0, at, "%dM" % n, seq, rng.randint(2, 42, n).tolist(), flag=0x61 if first else 0x91, name="f%05d" % i), s + L - n if first else s)))
    recs.sort(key=lambda t: t[:2])
    return [r for _, _, r in recs]


@pytest.fixture(scope="module")
def generated():
    recs = paired_stream(3000, 17)
    bed = [("c0", 1000, 1400), ("c0", 5000, 5600), ("c0", 7000, 9000), ("c0", 12000, 12300), ("c0", 18990, 19300)]
    regions = [(0, a, z) for _, a, z in bed]
    return recs, bed, pyfragpile.pileup_fragments(recs, regions, BIG[1], 0, 20), pypileup.pileup(recs, regions, BIG[1], 0, 20)


@pytest.mark.gpu
@VARIANTS
def test_generated_paired_stream_and_table(built, generated, tmp_path, direct):
    """3000 generated fragments against the model, and the table's bytes; gce_bam_pileup on the same file still counts twice"""
    from gencore_amd.bamio import pileup_bam, pileup_fragments_bam
    recs, bed, res, twice = generated
    assert res["n_pairs"] > 300 and res["n_shared_columns"] > 10000 and res["n_disagree_columns"] > 300 and res["n_eligible"] == 6000
    pc.write_raw_bam(str(tmp_path / "in.bam"), recs, *BIG, block=4000)
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    run = pileup_fragments_bam(tmp_path / "in.bam", tmp_path / "t.bed", tsv=tmp_path / "frag.tsv", min_baseq=20, direct=direct, threads=2)
    same(run, res, deferred=0)
    assert (tmp_path / "frag.tsv").read_bytes() == pypileup.table(res, BIG[0])
    small = pileup_fragments_bam(tmp_path / "in.bam", tmp_path / "t.bed", min_baseq=20, direct=direct, threads=2, window_bytes=1 << 14)
    same(small, res)
    assert small.n_deferred > 0
    old = pileup_bam(tmp_path / "in.bam", tmp_path / "t.bed", min_baseq=20, direct=direct, threads=2)
    assert old.counts.reshape(-1, 16).tolist() == twice["counts"] and int(old.counts.sum()) - int(run.counts.sum()) == res["n_shared_columns"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["frag.tsv", "in.bam", "t.bed"]


OOM = re.compile(r"out of device memory: gce_bam_pileup_fragments needs 64 bytes per site \((\d+) sites\), a join table \((\d+) bytes\) and an arena \((\d+) bytes\) "
                 r"\(\d+ bytes live, budget (\d+), (\d+) more for the arena\)")


@pytest.mark.gpu
@VARIANTS
def test_budget_too_small_for_the_arena(built, tmp_path, direct):
    """200 waiting records of 4.6 kB: a budget that holds everything but the second arena is GCE_ERR_OOM with the footprint in its message"""
    from gencore_amd.bamio import pileup_fragments_bam
    from gencore_amd.capi import GceError
    rng = np.random.RandomState(2)
    big = "".join("ACGT"[j] for j in rng.randint(0, 4, 3000))
    recs = [fc.mated(pc.rec(0, 100 + k, "3000M", big, rng.randint(0, 41, 3000).tolist(), flag=0x61, name="big%03d" % k), 2900) for k in range(200)]
    recs += [pc.rec(0, 400 + 5 * k, "50M", big[:50], name="fill%03d" % k) for k in range(300)]
    bam, bed = tmp_path / "in.bam", tmp_path / "t.bed"
    pc.write_raw_bam(str(bam), recs, *BIG, block=300)
    bed.write_text("c0\t0\t4000\n")
    free = pileup_fragments_bam(bam, bed, direct=direct, window_bytes=2000)
    assert free.n_deferred == 200 and free.n_pairs == 0 and free.peak_device_bytes > 2 * 200 * 4500
    with pytest.raises(GceError) as ei:
        pileup_fragments_bam(bam, bed, tsv=tmp_path / "out.tsv", direct=direct, window_bytes=2000, device_budget_bytes=free.peak_device_bytes - 800000)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and str(ei.value).endswith(m.group(0)), str(ei.value)
    assert int(m.group(1)) == 4000 and int(m.group(3)) > 0 and int(m.group(4)) == free.peak_device_bytes - 800000 and int(m.group(5)) > 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "t.bed"]


@pytest.fixture(scope="module")
def consensus_input(tmp_path_factory):
    """the generated stream of test_pileup_gpu.py's command-line test at a fifth of its size: 600 pairs as in.bam / ref.fa / panel.bed"""
    from test_cli_gpu import write_inputs
    from test_depth_bed import depth_case
    d = tmp_path_factory.mktemp("fragpilestream")
    data, batch, _, panel = depth_case("cfg3", 600)
    regions = [(t, a - 150 + 20 * k, a - 150 + 20 * k + 12) for t, a, _ in panel[:2] for k in range(18)]
    write_inputs(d, data, batch, regions)
    return d


@pytest.mark.gpu
def test_command_line(built, consensus_input, tmp_path):
    """--pileup_in and --pileup with --pileup_fragments: both tables equal the model's over the input and over the output file, the second
    STDERR line gives rule V's counters, and at every site the depth is at most that of the twice-counting table"""
    from test_cli_gpu import cli
    d = consensus_input
    r = cli(["-i", str(d / "in.bam"), "-o", "out.bam", "-r", str(d / "ref.fa"), "-b", str(d / "panel.bed"), "-j", "r.json", "--threads", "4", "--pileup_in", "before.tsv",
             "--pileup", "after.tsv", "--pileup_min_baseq", "20", "--pileup_fragments"], tmp_path)
    assert r.returncode == 0, r.stderr
    fasta = pypileup.read_fasta(str(d / "ref.fa"))
    pairs = 0
    for label, bam, tsv in (("pileup_in", d / "in.bam", "before.tsv"), ("pileup", tmp_path / "out.bam", "after.tsv")):
        names, lens, recs = pyfragpile.read_raw_records(str(bam))
        bed = pypileup.read_bed(str(d / "panel.bed"), names)
        res, twice = pyfragpile.pileup_fragments(recs, bed, lens, 0, 20), pypileup.pileup(recs, bed, lens, 0, 20)
        assert (tmp_path / tsv).read_bytes() == pypileup.table(res, names, fasta), label
        assert ("%s: %d records, %d eligible, %d sites\n" % (label, res["n_records"], res["n_eligible"], res["n_sites"])) in r.stderr
        assert ("%s: %d pairs, %d shared columns, %d disagreeing\n" % (label, res["n_pairs"], res["n_shared_columns"], res["n_disagree_columns"])) in r.stderr
        depth = lambda x: [sum(k[0:5]) + sum(k[8:13]) for k in x["counts"]]
        assert len(depth(res)) == res["n_sites"] > 100 and all(a <= b for a, b in zip(depth(res), depth(twice))) and sum(depth(res)) > 0
        pairs += res["n_pairs"]
    assert pairs > 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["after.tsv", "before.tsv", "out.bam", "r.json"]
