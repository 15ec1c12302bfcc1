"""gce_bam_error_profile_fragments on the GPU: the shared join (gce_matejoin.hpp) under a second pass and k_fragerr_count, with the
LDS planes and with direct atomics, with the full and the weak hash where the join is the subject, against the model (tests/pyfragerr.py) and
the hand-written counters (tests/fragerrcases.py): every integer of both tables equal, and the overlap table's sum twice the shared columns
on every run.  The cases are the smallest at which the kernel can go wrong: rules V' and X column by column, a pair across a 32-entry block
step and a 16-entry boundary, 300 pairs at one locus, overlaps that cross the planes' last cycle, l_seq at its limit, mates in different
windows, rule P inside a window and at a window cut, the budget, one generated paired stream with both tables' bytes, and the command
line."""
import os
import re

import numpy as np
import pytest

import errprofcases as ec
import fragcases as fc
import fragerrcases as fx
import pileupcases as pc
import pyerrprof
import pyfragerr
import pyfragpile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["planes", "direct"])
HASHES = pytest.mark.parametrize("weak", [False, True], ids=["hash", "weak_hash"])
BIG = (["c0", "c1"], [20000, 3000])
COUNTERS = ["n_records", "n_eligible", "n_bases", "n_mismatches", "n_intervals"] + pyerrprof.SKIPS + pyfragerr.FRAG_COUNTERS


def big_fasta(seed=23):
    rng = np.random.RandomState(seed)
    return {nm: "".join("ACGTacgtNR"[j] for j in rng.choice(10, ln, p=[.22, .22, .22, .22, .02, .02, .02, .02, .02, .02])) for nm, ln in zip(*BIG)}


def same(run, res, deferred=None):
    """a run against the model's dict: both tables, every counter, every skip, rule M's and rule V's counters, and the overlap table's sum"""
    for k in COUNTERS:
        assert getattr(run, k) == res[k], k
    for name, got, want in (("counts", run.counts, res["counts"]), ("overlap", run.overlap, res["overlap"])):
        assert got.dtype == np.uint64 and got.shape == (3, pyerrprof.MAX_CYCLE, pyerrprof.ROW)
        want = np.array(want, np.uint64)
        assert (got == want).all(), (name, [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in np.argwhere(got != want)[:5]])
    assert int(run.overlap.sum()) == 2 * run.n_shared_columns and not run.overlap[:, :, 21:].any()
    if deferred is not None:
        assert run.n_deferred == deferred


def run_files(tmp_path, records, fasta, bed, names, lens, direct, weak=False, tag="x", block=0xff00, **kw):
    """records (bytes), fasta = {name: bases} and bed = None or [(contig name, start, end)] as files, through error_profile_fragments_bam
    -> (the run, the model's result)"""
    from gencore_amd.bamio import error_profile_fragments_bam
    bam, fa, bedf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.fa" % tag), tmp_path / ("%s.bed" % tag)
    if not bam.exists():
        pc.write_raw_bam(str(bam), records, names, lens, block)
        fa.write_text(ec.fasta_text(fasta))
        if bed is not None:
            bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    run = error_profile_fragments_bam(bam, fa, bed=None if bed is None else bedf, direct=direct, weak_hash=weak, threads=2, **kw)
    regions = None if bed is None else [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    res = pyfragerr.profile_fragments(records, [fasta.get(nm) for nm in names], lens, regions, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704))
    return run, res


@pytest.mark.gpu
@VARIANTS
@HASHES
def test_hand_cases(built, tmp_path, direct, weak):
    """every case of fragerrcases: both tables and the counters written out by hand"""
    for cs in fx.all_cases():
        run, res = run_files(tmp_path, cs["records"], ec.FASTA, cs["bed"], ec.NAMES, ec.LENS, direct, weak, tag=cs["label"], min_mapq=cs["min_mapq"], min_baseq=cs["min_baseq"],
                             exclude_flags=cs["exclude"])
        same(run, res, deferred=0)
        assert pyerrprof.nonzero(dict(counts=run.counts.tolist())) == fx.expected(cs), cs["label"]
        assert pyfragerr.nonzero_overlap(dict(overlap=run.overlap.tolist())) == fx.expected(cs, "xexpect"), cs["label"]
        assert {k: getattr(run, k) for k in pyerrprof.SKIPS} == cs["skips"], cs["label"]
        assert {k: getattr(run, k) for k in pyfragerr.FRAG_COUNTERS} == fx.counters_of(cs), cs["label"]


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("n", [16, 17, 32, 33])
def test_pair_at_a_step_edge(built, tmp_path, direct, n):
    """n - 2 single reads, then a pair as the last two records: with 33 records a is record slot 31 of one block and b slot 0 of the next
    (entries 31 / 32); with 17, entries 15 / 16; with 16 and 32 the pair ends a half and a whole step"""
    singles = [ec.rec(0, 2 + k // 4, "6M", "ACGTAC"[k % 3:] + "ACGTAC"[:k % 3], flag=16 * (k & 1), name="s%02d" % k) for k in range(n - 2)]
    run, res = run_files(tmp_path, singles + [fx.pa("GGGGGT", [30] * 5 + [31]), fx.pb()], ec.FASTA, None, ec.NAMES, ec.LENS, direct)
    same(run, res, deferred=0)
    assert (run.n_pairs, run.n_shared_columns, run.n_disagree_columns) == (1, 3, 1) and run.overlap[1, 5, 4 * 1 + 3] == 1 and run.overlap[2, 3, 4 * 2 + 2] == 1


@pytest.mark.gpu
@VARIANTS
def test_300_pairs_at_one_locus_weak_hash(built, tmp_path, direct):
    """300 pairs whose names differ in one digit, every a at c0:20 and every b at c0:23, under the weak hash: one probe run, and 600 entries
    that add to the same few counters of both tables"""
    rng = np.random.RandomState(3)
    a = [fx.pa("GGGGG" + "ACGT"[rng.randint(4)], [30] * 5 + [int(rng.randint(0, 41))], name="frag%03d" % k) for k in range(300)]
    b = [fx.pb("GG" + "ACGT"[rng.randint(4)] + "CCC", [30, 30, int(rng.randint(0, 41)), 30, 30, 30], name="frag%03d" % k) for k in range(300)]
    run, res = run_files(tmp_path, a + b[::-1], ec.FASTA, None, ec.NAMES, ec.LENS, direct, weak=True, min_baseq=13)
    assert res["n_pairs"] == 300 and res["n_shared_columns"] == 900 and 150 < res["n_disagree_columns"] < 300 and res["n_ambiguous"] == 0
    same(run, res, deferred=0)


def long_pair(la, lb, shift, seed, name):
    """a of la bases at c0:100 (forward, first) and b of lb bases at c0:100 + shift (reverse, last), both copies of the reference with a few
    other bases"""
    rng = np.random.RandomState(seed)
    ref = big_fasta()["c0"].upper()
    out = []
    for first, at, n in ((True, 100, la), (False, 100 + shift, lb)):
        seq = "".join(c if c in "ACGT" and rng.rand() > 0.05 else "ACGT"[rng.randint(4)] for c in ref[at:at + n])
        out.append(fc.mated(ec.rec(0, at, "%dM" % n, seq, rng.randint(2, 41, n).tolist(), flag=0x41 if first else 0x91, name=name), 100 + shift if first else 100))
    return out


@pytest.mark.gpu
@VARIANTS
def test_overlap_crosses_the_planes_last_cycle(built, tmp_path, direct):
    """reads of 161 and 200 cycles that overlap in 150 columns: a's cycles 12..161 and b's 200..51 meet cycle 160, where the adds of both
    tables pass from the planes to global atomics"""
    run, res = run_files(tmp_path, long_pair(161, 200, 11, 5, "long"), big_fasta(), None, *BIG, direct, min_baseq=10)
    assert res["n_pairs"] == 1 and res["n_shared_columns"] == 150 and res["n_disagree_columns"] > 3
    ovl = np.array(res["overlap"])
    assert ovl[1, 158:161].sum() == 3 and ovl[2, 150:200].sum() == 50 and ovl[2, 50:160].sum() == 110
    same(run, res, deferred=0)


@pytest.mark.gpu
@VARIANTS
def test_l_seq_at_the_limit(built, tmp_path, direct):
    """a 1024-base read paired with a 1024-base one shares 1000 columns up to cycle 1024; paired with a 1025-base one, its partner is too
    long and it is counted alone"""
    run, res = run_files(tmp_path, long_pair(1024, 1024, 24, 6, "edge"), big_fasta(), None, *BIG, direct, tag="ok")
    assert res["n_pairs"] == 1 and res["n_shared_columns"] == 1000 and np.array(res["overlap"])[1, 1023].sum() == 1
    same(run, res, deferred=0)
    run, res = run_files(tmp_path, long_pair(1024, 1025, 24, 6, "edge"), big_fasta(), None, *BIG, direct, tag="long")
    assert res["n_pairs"] == 0 and res["n_too_long"] == 1 and res["n_eligible"] == 1 and np.array(res["counts"])[1, 1023].sum() == 1
    same(run, res, deferred=0)


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("tail", [0, 3], ids=["ends_placed", "ends_unplaced"])
def test_mates_in_different_windows(built, tmp_path, direct, tail):
    """members of 300 bytes and windows of 2000 (test_fragpile_gpu.py's stream): a in one window and b in the next, a waiting through many
    windows, and a expiring by position, by contig, by an unplaced record and by the end of the file; both tables equal the one-window
    result and the model's, with a BED and without"""
    from test_fragpile_gpu import window_stream
    recs = window_stream(tail)
    for tag, bed in (("nobed", None), ("bed", [("c0", 50, 9000), ("c0", 14990, 15100), ("c1", 0, 3000)])):
        one, res = run_files(tmp_path, recs, big_fasta(), bed, *BIG, direct, tag=tag, block=300, min_baseq=13)
        assert res["n_pairs"] > 150 and res["n_shared_columns"] > 5000 and res["n_disagree_columns"] > 100 and res["n_unplaced"] == tail
        same(one, res, deferred=0)
        cut, _ = run_files(tmp_path, recs, big_fasta(), bed, *BIG, direct, tag=tag, block=300, min_baseq=13, window_bytes=2000)
        same(cut, res)
        assert (cut.counts == one.counts).all() and (cut.overlap == one.overlap).all() and cut.n_deferred > 20
    weak, _ = run_files(tmp_path, recs, big_fasta(), bed, *BIG, direct, weak=True, tag=tag, block=300, min_baseq=13, window_bytes=2000)
    same(weak, res, deferred=cut.n_deferred)


@pytest.mark.gpu
@VARIANTS
def test_rule_p(built, tmp_path, direct):
    """a record in front of its predecessor is named by its index, inside a window and as the first record of a window: of 40 consecutive
    offenders at least one opens a window of 2000 compressed bytes (fragcases.order_stream); the malformed-record refusal comes first; no
    table and no temporary file is left"""
    from gencore_amd.bamio import error_profile_fragments_bam
    from gencore_amd.capi import GceError
    (tmp_path / "ref.fa").write_text(">c0\n" + "ACGT" * 25 + "\n>c1\n" + "ACGT" * 12 + "\n")
    bam = tmp_path / "in.bam"
    out = dict(tsv=tmp_path / "out.tsv", overlap_tsv=tmp_path / "ovl.tsv")
    for k, wb in [(37, 0), (fc.ORDER_N - 8, 0), (fc.ORDER_N - 1, 0)] + [(k, 2000) for k in range(40, 80)] + [(fc.ORDER_N - 2, 2000)]:
        pc.write_raw_bam(str(bam), fc.order_stream(k), block=300)
        with pytest.raises(GceError) as ei:
            error_profile_fragments_bam(bam, tmp_path / "ref.fa", direct=direct, window_bytes=wb, **out)
        assert ei.value.status == -1 and str(ei.value).endswith("BAM record %d (counting from 0) lies in front of its predecessor: gce_bam_error_profile_fragments needs a "
                                                                "coordinate-sorted file" % k), (k, wb)
    recs = fc.order_stream(60)
    pc.write_raw_bam(str(bam), recs[:70] + [pc.malformed()[0][1]] + recs[70:])
    with pytest.raises(GceError) as ei:
        error_profile_fragments_bam(bam, tmp_path / "ref.fa", direct=direct, **out)
    assert ei.value.status == -1 and "BAM record 70 (counting from 0): its fields overrun its block_size" in str(ei.value)
    pc.write_raw_bam(str(bam), fc.order_stream(), block=300)
    run = error_profile_fragments_bam(bam, tmp_path / "ref.fa", direct=direct, window_bytes=2000)
    assert run.n_records == fc.ORDER_N and run.n_unplaced == 2 and run.n_eligible == fc.ORDER_N - 2
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]


@pytest.mark.gpu
@VARIANTS
def test_no_candidates_is_error_profile_bam(built, tmp_path, direct):
    """a sorted file without a paired flag: the primary table and every counter are gce_bam_error_profile's, through windows too; the
    overlap table is empty"""
    from gencore_amd.bamio import error_profile_bam
    rng = np.random.RandomState(11)
    recs = []
    for k in range(400):
        n = int(rng.randint(20, 200))
        recs.append(ec.rec(int(k >= 300), 6 * (k % 300) + int(rng.randint(0, 6)), "%dM" % n, "".join("ACGTN"[i] for i in rng.randint(0, 5, n)), rng.randint(0, 41, n).tolist(),
                           flag=int(rng.choice([0, 16, 0x40, 0x90])), name="read%04d" % k))
    bed = [("c0", 50, 400), ("c0", 1000, 1300), ("c1", 0, 3000)]
    run, res = run_files(tmp_path, recs, big_fasta(), bed, *BIG, direct, block=300, min_baseq=13, window_bytes=2000)
    same(run, res, deferred=0)
    ref = error_profile_bam(tmp_path / "x.bam", tmp_path / "x.fa", bed=tmp_path / "x.bed", direct=direct, min_baseq=13, window_bytes=2000)
    assert (ref.counts == run.counts).all() and ref.counts.sum() > 2000 and run.n_pairs == run.n_shared_columns == run.n_ambiguous == 0 and not run.overlap.any()
    for k in ["n_records", "n_eligible", "n_bases", "n_mismatches", "n_intervals"] + pyerrprof.SKIPS:
        assert getattr(ref, k) == getattr(run, k), k


OOM = re.compile(r"out of device memory: gce_bam_error_profile_fragments needs the reference bases \((\d+) bytes\) \+ 1152 KiB of counters, a join table \((\d+) bytes\) and an arena "
                 r"\((\d+) bytes\) \(\d+ bytes live, budget (\d+), (\d+) more for the arena\)")


@pytest.mark.gpu
@VARIANTS
def test_budget_too_small_for_the_arena(built, tmp_path, direct):
    """300 waiting records of 1.6 kB: a budget that holds everything but the second arena is GCE_ERR_OOM with the footprint in its message"""
    from gencore_amd.bamio import error_profile_fragments_bam
    from gencore_amd.capi import GceError
    rng = np.random.RandomState(2)
    big = "".join("ACGT"[j] for j in rng.randint(0, 4, 1000))
    recs = [fc.mated(ec.rec(0, 100 + k, "1000M", big, rng.randint(0, 41, 1000).tolist(), flag=0x61, name="big%03d" % k), 1050) for k in range(300)]
    recs += [ec.rec(0, 400 + 2 * k, "50M", big[:50], name="fill%03d" % k) for k in range(300)]
    bam, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    pc.write_raw_bam(str(bam), recs, *BIG, block=300)
    fa.write_text(ec.fasta_text(big_fasta()))
    free = error_profile_fragments_bam(bam, fa, direct=direct, window_bytes=2000)
    assert free.n_deferred == 300 and free.n_pairs == 0 and free.n_eligible == 600 and free.peak_device_bytes > 2 * 300 * 1500
    with pytest.raises(GceError) as ei:
        error_profile_fragments_bam(bam, fa, tsv=tmp_path / "out.tsv", overlap_tsv=tmp_path / "ovl.tsv", direct=direct, window_bytes=2000,
                                    device_budget_bytes=free.peak_device_bytes - 400000)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and str(ei.value).endswith(m.group(0)), str(ei.value)
    assert int(m.group(1)) == 23000 and int(m.group(3)) > 0 and int(m.group(4)) == free.peak_device_bytes - 400000 and int(m.group(5)) > 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]


@pytest.fixture(scope="module")
def generated():
    """2000 generated fragments (test_fragpile_gpu.py's generator) and the model's result without a BED and with one, computed once"""
    from test_fragpile_gpu import paired_stream
    recs = paired_stream(2000, 17)
    bed = [("c0", 1000, 1400), ("c0", 5000, 5600), ("c0", 7000, 9000), ("c0", 12000, 12300), ("c0", 18990, 19300)]
    fasta = big_fasta()
    refs = [fasta[nm] for nm in BIG[0]]
    return recs, fasta, bed, {False: pyfragerr.profile_fragments(recs, refs, BIG[1], None, 0, 20), True: pyfragerr.profile_fragments(recs, refs, BIG[1], [(0, a, z) for _, a, z in bed], 0, 20)}


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("with_bed", [False, True], ids=["nobed", "bed"])
def test_generated_paired_stream_and_tables(built, generated, tmp_path, direct, with_bed):
    """2000 generated fragments against the model, both tables' bytes, and the same through small windows; gce_bam_error_profile on the same
    file counts the shared columns twice"""
    from gencore_amd.bamio import error_profile_bam, error_profile_fragments_bam
    recs, fasta, bed, results = generated
    res = results[with_bed]
    assert res["n_pairs"] > (200 if with_bed else 1200) and res["n_shared_columns"] > (5000 if with_bed else 40000) and res["n_disagree_columns"] > 300 and res["n_eligible"] == 4000
    pc.write_raw_bam(str(tmp_path / "in.bam"), recs, *BIG, block=4000)
    (tmp_path / "ref.fa").write_text(ec.fasta_text(fasta))
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    kw = dict(bed=tmp_path / "t.bed" if with_bed else None, min_baseq=20, direct=direct, threads=2)
    run = error_profile_fragments_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tsv=tmp_path / "p.tsv", overlap_tsv=tmp_path / "o.tsv", **kw)
    same(run, res, deferred=0)
    assert (tmp_path / "p.tsv").read_bytes() == pyerrprof.table(res) and (tmp_path / "o.tsv").read_bytes() == pyfragerr.overlap_table(res)
    small = error_profile_fragments_bam(tmp_path / "in.bam", tmp_path / "ref.fa", window_bytes=1 << 14, **kw)
    same(small, res)
    assert small.n_deferred > 0
    old = error_profile_bam(tmp_path / "in.bam", tmp_path / "ref.fa", **kw)
    assert int(old.counts[:, :, :19].sum()) - int(run.counts[:, :, :19].sum()) == res["n_shared_columns"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "o.tsv", "p.tsv", "ref.fa", "t.bed"]


@pytest.fixture(scope="module")
def consensus_input(tmp_path_factory):
    """the generated stream of test_errprof_gpu.py's command-line test at three fifths of its size: 600 pairs as in.bam / ref.fa / panel.bed"""
    from test_cli_gpu import write_inputs
    from test_depth_bed import depth_case
    d = tmp_path_factory.mktemp("fragerrstream")
    data, batch, _, panel = depth_case("cfg3", 600)
    regions = [(t, a - 150 + 20 * k, a - 150 + 20 * k + 12) for t, a, _ in panel[:2] for k in range(18)]
    write_inputs(d, data, batch, regions)
    return d


@pytest.mark.gpu
def test_command_line(built, consensus_input, tmp_path):
    """--error_profile_in and --error_profile with --error_profile_fragments: both tables and both overlap tables equal the model's over the
    input and over the output file, the second STDERR line gives rule V's counters; the flag alone is a usage error"""
    from test_cli_gpu import cli
    d = consensus_input
    r = cli(["-i", str(d / "in.bam"), "-o", "out.bam", "-r", str(d / "ref.fa"), "-j", "r.json", "--threads", "4", "--error_profile_in", "before.tsv", "--error_profile", "after.tsv",
             "--error_profile_min_baseq", "20", "--error_profile_fragments"], tmp_path)
    assert r.returncode == 0, r.stderr
    fasta = pyerrprof.read_fasta(str(d / "ref.fa"))
    pairs = 0
    for label, bam, tsv in (("error_profile_in", d / "in.bam", "before.tsv"), ("error_profile", tmp_path / "out.bam", "after.tsv")):
        names, lens, recs = pyfragpile.read_raw_records(str(bam))
        res = pyfragerr.profile_fragments(recs, pyerrprof.refs_of(fasta, names), lens, None, 0, 20)
        assert (tmp_path / tsv).read_bytes() == pyerrprof.table(res), label
        assert (tmp_path / (tsv + ".overlap.tsv")).read_bytes() == pyfragerr.overlap_table(res), label
        assert pyfragerr.overlap_sum(res) == 2 * res["n_shared_columns"]
        assert ("%s: %d records, %d eligible, %d bases, %d mismatches\n%s: %d pairs, %d shared columns, %d disagreeing\n"
                % (label, res["n_records"], res["n_eligible"], res["n_bases"], res["n_mismatches"], label, res["n_pairs"], res["n_shared_columns"], res["n_disagree_columns"])) in r.stderr
        pairs += res["n_pairs"]
    assert pairs > 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["after.tsv", "after.tsv.overlap.tsv", "before.tsv", "before.tsv.overlap.tsv", "out.bam", "r.json"]
    r = cli(["-i", str(d / "in.bam"), "-o", "out2.bam", "-r", str(d / "ref.fa"), "--error_profile_fragments"], tmp_path)
    assert r.returncode == 255 and "ERROR: --error_profile_fragments needs --error_profile or --error_profile_in" in r.stderr
