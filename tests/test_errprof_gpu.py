"""gce_bam_error_profile on the GPU: the scan (k_reduce_scan) and k_err_count, with the LDS planes and with direct atomics (direct=True), against
the model (tests/pyerrprof.py) and the hand-written counters (tests/errprofcases.py): every integer equal, so the two variants equal each
other.  The cases are the smallest at which the kernels can go wrong: every hand case, the cycles at the planes' last index and past it, the
32-record steps and the grid's stride, 300 identical reads, file order, records cut between windows, the scan's counter slots, the budget, malformed records, the
table's text and the command line."""
import os
import re

import numpy as np
import pytest

import errprofcases as ec
import pybam
import pyerrprof

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_errprof.hpp")).read()
CYC, STEP, GRID = (int(re.search(r"#define %s (\d+)u" % n, SRC).group(1)) for n in ("EP_CYC", "EP_STEP_RECS", "EP_GRID"))
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["planes", "direct"])
BIG_NAMES, BIG_LENS = ["c0", "c1"], [20000, 3000]
BIG_FASTA = {nm: "".join("ACGT"[i] for i in np.random.RandomState(21 + k).randint(0, 4, ln)) for k, (nm, ln) in enumerate(zip(BIG_NAMES, BIG_LENS))}


def same(run, res):
    """an ErrorProfileRun against the model's dict: every counter, every skip, the totals"""
    assert run.counts.dtype == np.uint64 and run.counts.shape == (3, pyerrprof.MAX_CYCLE, pyerrprof.ROW)
    assert run.counts.tolist() == res["counts"]
    for k in ["n_records", "n_eligible", "n_bases", "n_mismatches", "n_intervals"] + pyerrprof.SKIPS:
        assert getattr(run, k) == res[k], k


def run_files(tmp_path, records, names, lens, fasta, direct, bed=None, tag="x", block=0xff00, **kw):
    """records (bytes), fasta = {name: bases} and bed = None or [(contig name, start, end)] as files, through error_profile_bam
    -> (the run, the model's result)"""
    from gencore_amd.bamio import error_profile_bam
    bam, fa, bedf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.fa" % tag), tmp_path / ("%s.bed" % tag)
    if not bam.exists():
        ec.write_raw_bam(str(bam), records, names, lens, block)
        fa.write_text(ec.fasta_text(fasta))
    if bed is not None:
        bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    run = error_profile_bam(bam, fa, bed=None if bed is None else bedf, direct=direct, threads=2, **kw)
    regions = None if bed is None else [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    res = pyerrprof.profile(records, [fasta.get(nm) for nm in names], lens, regions, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704))
    return run, res


@pytest.mark.gpu
@VARIANTS
def test_hand_cases(built, tmp_path, direct):
    """every case of errprofcases: strands, segments, ops, cycles, reference bytes, nibbles, qualities, skips, l_seq 1024 and 1025, the BED's
    anchors -- the counters written out by hand"""
    for cs in ec.all_cases():
        run, res = run_files(tmp_path, cs["records"], ec.NAMES, ec.LENS, ec.FASTA, direct, bed=cs["bed"], tag=cs["label"], min_mapq=cs["min_mapq"], min_baseq=cs["min_baseq"],
                             exclude_flags=cs["exclude"])
        same(run, res)
        assert pyerrprof.nonzero(dict(counts=run.counts.tolist())) == ec.expected(cs), cs["label"]
        assert {k: getattr(run, k) for k in pyerrprof.SKIPS} == cs["skips"], cs["label"]
        assert run.n_eligible == len(cs["records"]) - sum(cs["skips"].values())
        assert run.peak_device_bytes > 0 and run.total_s > 0


def read_at(k, n, flag, pos=100):
    """read k of n aligned bases copied from c0 with every seventh base changed"""
    ref = BIG_FASTA["c0"][pos + k:pos + k + n]
    return ec.rec(0, pos + k, "%dM" % n, "".join("ACGT"[("ACGT".index(b) + 1) % 4] if i % 7 == 3 else b for i, b in enumerate(ref)), flag=flag)


@pytest.mark.gpu
@VARIANTS
def test_plane_edges_and_file_order(built, tmp_path, direct):
    """reads of EP_CYC - 1, EP_CYC, EP_CYC + 1 and EP_CYC + 40 bases on both strands in all three segments: cycle EP_CYC is the last the planes
    hold, EP_CYC + 1 the first that goes to memory, and segment 2's cycle EP_CYC is a plane's last counter row.  The same records in reverse
    file order (other slots, other planes) give the same counters"""
    recs = [read_at(3 * k + j, n, flag) for k, n in enumerate((CYC - 1, CYC, CYC + 1, CYC + 40)) for j, flag in enumerate((0, 0x10, 0x40, 0x50, 0x80, 0x90))]
    recs += [ec.rec(0, 500, "%dS1M1I1D1M" % (CYC - 2), "A" * (CYC - 2) + "CGT", flag=f) for f in (0x80, 0x90)]     # M at EP_CYC - 1, I and D at EP_CYC, M at EP_CYC + 1
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="fwd")
    same(run, res)
    c = run.counts[:, :, :16].sum(axis=2)
    for g in range(3):
        assert c[g, CYC - 1] == 6 and c[g, CYC] == 4 + (g == 2) and c[g, CYC + 39] == 2 and c[g, CYC + 40] == 0
    assert run.counts[2, CYC - 1, pyerrprof.INS] == 1 and run.counts[2, CYC - 1, pyerrprof.DEL] == 1 and run.n_mismatches > 100
    back, res2 = run_files(tmp_path, recs[::-1], BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="rev")
    same(back, res2)
    assert (back.counts == run.counts).all()


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("n", [STEP - 1, STEP, STEP + 1, 300, GRID * STEP + 1])
def test_whole_and_partial_steps(built, tmp_path, direct, n):
    """one record short of, exactly and one past a block's 32-record step; 300 identical reads, every add on the same counters, and then the
    flush; one record more than a whole grid's steps, which block 0 takes in its second step"""
    if n == 300:
        recs = [read_at(0, 20, 0x50)] * 300
    elif n > 1000:
        recs = [read_at(k % 1000, 3, 0x40 if k & 1 else 0x90, pos=7) for k in range(n)]
    else:
        recs = [ec.rec(0, 10 + 3 * k, "2M1D2M", "ACGT", flag=16 * (k % 3 == 0)) for k in range(n)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct)
    same(run, res)
    assert run.n_eligible == n
    if n == 300:
        assert run.counts[1, :20, :16].sum(axis=1).tolist() == [300] * 20 and run.counts.sum() == 6000 and (run.counts[1, :20] == 300).sum() == 20
    elif n > 1000:
        assert run.counts[:, :3, :16].sum() == 3 * n
    else:
        assert run.counts[0, :, pyerrprof.DEL].sum() == n


def window_records():
    rng = np.random.RandomState(11)
    recs = []
    for k in range(400):
        n = int(rng.randint(20, 200))
        ops = [(4, int(rng.randint(1, 5)))] * int(rng.randint(0, 2)) + [(0, n), (int(rng.choice([1, 2, 3])), int(rng.randint(1, 6))), (0, int(rng.randint(1, 30)))]
        nq = sum(ln for op, ln in ops if op in (0, 1, 4))
        seq = "".join("ACGTN"[i] for i in rng.choice(5, nq, p=[.24, .24, .24, .24, .04]))
        recs.append(ec.rec(int(k >= 300), int(rng.randint(0, 2500)), ops, seq, rng.randint(0, 41, nq).tolist(), flag=int(rng.choice([0, 16, 0x40, 0x50, 0x80, 0x90, 0x400])),
                           mapq=int(rng.randint(0, 61)), name="read%04d" % k))
    recs.insert(150, ec.rec(0, 100, "1000M", "".join("ACGT"[i] for i in rng.randint(0, 4, 1000)), rng.randint(0, 41, 1000).tolist()))    # 1.5 kB: larger than a window
    return recs


@pytest.mark.gpu
@VARIANTS
def test_records_cut_between_windows(built, tmp_path, direct):
    """members of 300 bytes and windows of 1000: most records are cut between windows and one record is larger than a window; the result
    equals the one-window result and the model's, with and without a BED"""
    recs = window_records()
    bed = [("c0", 50, 400), ("c0", 1000, 1300), ("c0", 5000, 6500), ("c1", 0, 3000)]
    for tag, b in (("nobed", None), ("bed", bed)):
        one, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, bed=b, tag=tag, block=300, min_baseq=13, min_mapq=5)
        same(one, res)
        cut, _ = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, bed=b, tag=tag, block=300, min_baseq=13, min_mapq=5, window_bytes=1000)
        same(cut, res)
        assert (cut.counts == one.counts).all() and one.counts[:, :, pyerrprof.LOWQ].sum() > 0 and one.n_bases >= 2000 and one.n_flagged > 0 and one.n_low_mapq > 0
    assert res["n_intervals"] == 4


@pytest.mark.gpu
@VARIANTS
def test_scan_counter_slots(built, tmp_path, direct):
    """65 records, one wave of the scan and one record: a record for each of rule E's eight skips (the skip_order case's, under min_mapq 1) among
    eligible ones, so every counter slot of the scan is added to by a wave's ballot and the tail wave runs; in one window, and in windows of half
    the file, where the slots are added to twice.  Every n_* counter equals the model's"""
    skips = [c for c in ec.all_cases() if c["label"] == "skip_order"][0]["records"]
    assert len(skips) == 8
    good = [ec.rec(0, k % 9, "3M", "ACG", flag=(0, 0x10, 0x40, 0x90)[k & 3]) for k in range(57)]
    recs = [r for k in range(8) for r in good[7 * k:7 * k + 7] + [skips[k]]] + good[56:]
    assert len(recs) == 65
    one, res = run_files(tmp_path, recs, ec.NAMES, ec.LENS, ec.FASTA, direct, block=300, min_mapq=1)
    assert [res[k] for k in pyerrprof.SKIPS] == [1] * 8 and res["n_eligible"] == 57 and res["n_records"] == 65
    same(one, res)
    size = os.path.getsize(str(tmp_path / "x.bam"))
    assert size // 2 >= 400                                                                # (a member of 300 inflated bytes takes some 330 at the most: half the file holds whole ones)
    two, _ = run_files(tmp_path, recs, ec.NAMES, ec.LENS, ec.FASTA, direct, block=300, min_mapq=1, window_bytes=size // 2)
    same(two, res)


OOM = re.compile(r"out of device memory: gce_bam_error_profile needs the reference bases \((\d+) bytes\) \+ 576 KiB of counters \+ 16 bytes per interval \+ one window \+ 4 bytes per "
                 r"window record \(\d+ bytes live, budget (\d+), (\d+) more for the reference bases\)")


@pytest.mark.gpu
@VARIANTS
def test_budget(built, tmp_path, direct):
    """a budget that cannot hold the reference is GCE_ERR_OOM naming the reference bases, with the footprint in its message; no file is left"""
    from gencore_amd.bamio import error_profile_bam
    from gencore_amd.capi import GceError
    bam, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    ec.write_raw_bam(str(bam), [ec.rec(0, 10, "2M")], ["c0"], [3 << 20])
    fa.write_text(">c0\n" + "ACGT" * (3 << 18) + "\n")
    with pytest.raises(GceError) as ei:
        error_profile_bam(bam, fa, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=1 << 20)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and str(ei.value).endswith(m.group(0)), str(ei.value)
    assert [int(x) for x in m.groups()[:2]] == [3 << 20, 1 << 20] and int(m.group(3)) > 3 << 20
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]
    run = error_profile_bam(bam, fa, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=64 << 20)
    assert run.n_eligible == 1 and run.n_bases == 2 and 3 << 20 < run.peak_device_bytes <= 64 << 20


@pytest.mark.gpu
@VARIANTS
def test_malformed_records(built, tmp_path, direct):
    """malformed records at k and k + j: the lowest is named; no table, no temporary file"""
    from gencore_amd.bamio import error_profile_bam
    from gencore_amd.capi import GceError
    good = [ec.rec(0, k, "3M", "ACG") for k in range(40)]
    (tmp_path / "ref.fa").write_text(ec.fasta_text())
    for k, (label, bad) in enumerate(ec.malformed()):
        at = 17 + 8 * k
        recs = good[:at] + [bad] + good[at:at + 5] + [ec.malformed()[0][1]] + good[at + 5:]
        with pytest.raises(pyerrprof.ErrprofError) as mi:
            pyerrprof.profile(recs, ec.refs(), ec.LENS)
        assert mi.value.record == at
        bam = tmp_path / ("%s.bam" % label)
        ec.write_raw_bam(str(bam), recs, ec.NAMES, ec.LENS)
        with pytest.raises(GceError) as ei:
            error_profile_bam(bam, tmp_path / "ref.fa", tsv=tmp_path / "out.tsv", direct=direct)
        assert ei.value.status == -1 and ("BAM record %d (counting from 0)" % at) in str(ei.value), label
        bam.unlink()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ref.fa"]


@pytest.mark.gpu
@VARIANTS
def test_table_text(built, tmp_path, direct):
    """the table's bytes against the model's text: three segments with different last cycles, then a BED that leaves one segment empty"""
    from gencore_amd.bamio import error_profile_bam
    recs = [read_at(k, 30 + 5 * (k % 4), (0, 0x10, 0x40, 0x90)[k % 4]) for k in range(40)] + [ec.rec(0, 900, "3M1I2M1D4M", "ACGTACGTAC", flag=0x80)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="t", tsv=tmp_path / "all.tsv")
    same(run, res)
    text = (tmp_path / "all.tsv").read_bytes()
    assert text == pyerrprof.table(res) and len(text.split(b"\n")) == 1 + 35 + 40 + 45 + 1
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, bed=[("c0", 895, 910)], tag="t", tsv=tmp_path / "bed.tsv")
    same(run, res)
    text = (tmp_path / "bed.tsv").read_bytes()
    assert text == pyerrprof.table(res) and {l.split(b"\t")[0] for l in text.split(b"\n")[1:-1]} == {b"2"}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["all.tsv", "bed.tsv", "t.bam", "t.bed", "t.fa"]


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """one generated stream of 1000 pairs from the suite's generators as in.bam / ref.fa / panel.bed with a BED of a few dozen targets"""
    from test_cli_gpu import write_inputs
    from test_depth_bed import depth_case
    d = tmp_path_factory.mktemp("errprofstream")
    data, batch, _, panel = depth_case("cfg3", 1000)
    regions = [(t, a - 150 + 20 * k, a - 150 + 20 * k + 12) for t, a, _ in panel[:2] for k in range(18)]
    targets = write_inputs(d, data, batch, regions)
    names, lens = [t[0] for t in targets], [t[1] for t in targets]
    fasta = pyerrprof.read_fasta(str(d / "ref.fa"))
    return d, names, lens, pyerrprof.read_bed(str(d / "panel.bed"), names), pyerrprof.refs_of(fasta, names)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bed", [False, True], ids=["nobed", "bed"])
def test_command_line_before_and_after(built, stream, tmp_path, with_bed):
    """one run with --error_profile_in and --error_profile, with and without -b: both tables equal the model's over the input and over the
    written output, and the stderr lines carry the model's totals"""
    from test_cli_gpu import cli
    d, names, lens, bed, refs = stream
    r = cli(["-i", str(d / "in.bam"), "-o", "out.bam", "-r", str(d / "ref.fa"), "-j", "r.json", "--threads", "4", "--error_profile_in", "before.tsv", "--error_profile", "after.tsv",
             "--error_profile_min_baseq", "20"] + (["-b", str(d / "panel.bed")] if with_bed else []), tmp_path)
    assert r.returncode == 0, r.stderr
    for label, bam, tsv in (("error_profile_in", d / "in.bam", "before.tsv"), ("error_profile", tmp_path / "out.bam", "after.tsv")):
        res = pyerrprof.profile(pybam.read_bam(str(bam))[2], refs, lens, bed if with_bed else None, 0, 20)
        assert (tmp_path / tsv).read_bytes() == pyerrprof.table(res), label
        assert ("%s: %d records, %d eligible, %d bases, %d mismatches\n" % (label, res["n_records"], res["n_eligible"], res["n_bases"], res["n_mismatches"])) in r.stderr
        assert res["n_eligible"] > 200 and res["n_bases"] > (0 if with_bed else 20000)       # (1000 pairs in clusters of 8: 250 consensus records or more, of about 150 bases)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["after.tsv", "before.tsv", "out.bam", "r.json"]
