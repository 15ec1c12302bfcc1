"""gce_bam_pileup on the GPU: the scan (k_reduce_scan) and k_pile_count, with the LDS tile and with direct atomics (direct=True), against the
model (tests/pypileup.py) and the hand-written counters (tests/pileupcases.py): every integer equal, so the two variants equal each other.
The cases are the smallest at which the kernels can go wrong: every op at an interval's edges, the regions' clamping and merging, the
nibbles and qualities, every skip, the tile's edges and the 16-record blocks, records cut between windows, the scan's counter slots, the budget, malformed records,
one generated stream, the table's text and the command line."""
import os
import re

import numpy as np
import pytest

import pileupcases as pc
import pybam
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"#define PU_TILE (\d+)u", open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_pileup.hpp")).read()).group(1))
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["tile", "direct"])
BIG = (["c0", "c1"], [20000, 3000])


def same(run, res):
    """a PileupRun against the model's dict: the sites, every counter, every skip"""
    assert run.n_sites == res["n_sites"] and run.n_intervals == res["n_intervals"]
    assert run.tid.tolist() == res["tid"] and run.pos.tolist() == res["pos"]
    assert run.counts.dtype == np.uint32 and run.counts.shape == (res["n_sites"], 2, 8)
    assert run.counts.reshape(-1, 16).tolist() == res["counts"]
    for k in ["n_records", "n_eligible"] + pypileup.SKIPS:
        assert getattr(run, k) == res[k], k


def run_files(tmp_path, records, bed, names, lens, direct, tag="x", block=0xff00, **kw):
    """records (bytes) and bed = [(contig name, start, end)] as files, through pileup_bam -> (the run, the model's result)"""
    from gencore_amd.bamio import pileup_bam
    bam, bedf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.bed" % tag)
    if not bam.exists():
        pc.write_raw_bam(str(bam), records, names, lens, block)
        bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    run = pileup_bam(bam, bedf, direct=direct, threads=2, **kw)
    regions = [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    res = pypileup.pileup(records, regions, lens, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704))
    return run, res


@pytest.mark.gpu
@VARIANTS
def test_hand_cases(built, tmp_path, direct):
    """every case of pileupcases: ops at interval edges, regions, bases and strands, skips -- the counters written out by hand"""
    for cs in pc.all_cases():
        run, res = run_files(tmp_path, cs["records"], cs["bed"], pc.NAMES, pc.LENS, direct, tag=cs["label"], min_mapq=cs["min_mapq"], min_baseq=cs["min_baseq"],
                             exclude_flags=cs["exclude"])
        same(run, res)
        assert run.counts.reshape(-1, 16).tolist() == pc.expected_counts(cs, list(zip(res["tid"], res["pos"]))), cs["label"]
        assert {k: getattr(run, k) for k in pypileup.SKIPS} == cs["skips"], cs["label"]
        assert run.n_eligible == len(cs["records"]) - sum(cs["skips"].values())
        assert run.peak_device_bytes > 0 and run.total_s > 0


def tile_records():
    """one block of 16 records on one interval [0, 3 TILE) of c0: the first record's tile starts at site 99 (pos - 1) and ends in front of site
    99 + TILE; records end on the tile's last site, straddle its end, start on the first site behind it, jump far beyond it over an N and
    lie in front of it"""
    e = 99 + TILE
    r = [pc.rec(0, 100, "3M", "ACG"), pc.rec(0, e - 3, "3M", "CCC"), pc.rec(0, e - 1, "2M", "GT", flag=16), pc.rec(0, e, "2M", "TT"), pc.rec(0, 101, "1M%dN2M" % (2 * TILE), "ACG"),
         pc.rec(0, e - 2, "1M1I1M1D1M", "ACGT"), pc.rec(0, e - 1, "1M1I1M", "GGG"), pc.rec(0, 120, "2M3D2M", "ACGT", flag=16)]
    r += [pc.rec(0, 100 + 7 * k, "5M", "ACGTA", flag=16 * (k & 1)) for k in range(7)] + [pc.rec(0, 40, "4M", "TTTT")]
    assert len(r) == 16
    return r


@pytest.mark.gpu
@VARIANTS
def test_tile_edges_and_file_order(built, tmp_path, direct):
    """sites at index TILE - 1 and TILE of a block's tile, an N skip far outside it, a record in front of it; the same records in reverse file
    order (another tile start) give the same counters"""
    bed = [("c0", 0, 3 * TILE)]
    recs = tile_records()
    run, res = run_files(tmp_path, recs, bed, *BIG, direct, tag="fwd")
    same(run, res)
    c = run.counts.reshape(-1, 16)
    assert c[99 + TILE - 1].sum() > 0 and c[99 + TILE].sum() > 0 and c[101 + 1 + 2 * TILE].sum() > 0 and c[40].sum() > 0
    back, res2 = run_files(tmp_path, recs[::-1], bed, *BIG, direct, tag="rev")
    same(back, res2)
    assert (back.counts == run.counts).all()


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("n", [31, 32, 33, 300])
def test_whole_and_partial_blocks(built, tmp_path, direct, n):
    """16 k - 1, 16 k and 16 k + 1 records (k = 2): one short of, exactly and one past whole 16-record blocks; 300 identical reads on one site"""
    if n == 300:
        recs, bed = [pc.rec(0, 500, "1M", "G")] * 300, [("c0", 500, 501)]
    else:
        recs, bed = [pc.rec(0, 10 + 3 * k, "2M1D2M", "ACGT", flag=16 * (k % 3 == 0)) for k in range(n)], [("c0", 5, 60), ("c0", 70, 200)]
    run, res = run_files(tmp_path, recs, bed, *BIG, direct)
    same(run, res)
    if n == 300:
        assert run.counts.reshape(-1).tolist() == [0, 0, 300] + [0] * 13
    else:
        assert run.n_eligible == n and run.counts[res["pos"].index(10 + 3 * (n - 1))].sum() > 0           # (the last record was counted)


def window_records():
    rng = np.random.RandomState(11)
    recs = []
    for k in range(400):
        n = int(rng.randint(20, 120))
        seq = "".join("ACGTN"[i] for i in rng.randint(0, 5, n))
        recs.append(pc.rec(int(k >= 300), int(rng.randint(0, 2500)), "%dM" % n, seq, rng.randint(0, 41, n).tolist(), flag=16 * int(rng.randint(0, 2)), name="read%04d" % k))
    big = 6000                                                  # a record of 9 kB: larger than a window of 2000 bytes
    recs.insert(150, pc.rec(0, 100, "%dM" % big, "".join("ACGT"[i] for i in rng.randint(0, 4, big)), rng.randint(0, 41, big).tolist()))
    return recs


@pytest.mark.gpu
@VARIANTS
def test_records_cut_between_windows(built, tmp_path, direct):
    """members of 300 bytes and windows of 2000: most records are cut between windows and one record is larger than many windows; the result
    equals the one-window result and the model's"""
    recs = window_records()
    bed = [("c0", 50, 400), ("c0", 1000, 1300), ("c0", 5000, 6500), ("c1", 0, 3000)]
    one, res = run_files(tmp_path, recs, bed, *BIG, direct, block=300, min_baseq=13)
    same(one, res)
    cut, _ = run_files(tmp_path, recs, bed, *BIG, direct, block=300, min_baseq=13, window_bytes=2000)
    same(cut, res)
    assert (cut.counts == one.counts).all() and one.counts[:, :, 7].sum() > 0 and one.counts.sum() >= 2000     # (c1's 100 reads of 20 bases or more lie on sites whole)


@pytest.mark.gpu
@VARIANTS
def test_scan_counter_slots(built, tmp_path, direct):
    """65 records, one wave of the scan and one record: a record for each of rule E's six skips (the skip_order case's, under min_mapq 1) among
    eligible ones, so every counter slot of the scan is added to by a wave's ballot and the tail wave runs; in one window, and in windows of half
    the file, where the slots are added to twice.  Every n_* counter equals the model's"""
    skips = [c for c in pc.all_cases() if c["label"] == "skip_order"][0]["records"] + [pc.rec(0, 10, [(9, 1)], "A")]
    assert len(skips) == 6
    good = [pc.rec(0, 5 + k % 9, "3M", "ACG", flag=16 * (k & 1)) for k in range(59)]
    recs = [r for k in range(6) for r in good[9 * k:9 * k + 9] + [skips[k]]] + good[54:]
    assert len(recs) == 65
    bed = [("c0", 8, 14)]
    one, res = run_files(tmp_path, recs, bed, pc.NAMES, pc.LENS, direct, block=300, min_mapq=1)
    assert [res[k] for k in pypileup.SKIPS] == [1] * 6 and res["n_eligible"] == 59 and res["n_records"] == 65
    same(one, res)
    size = os.path.getsize(str(tmp_path / "x.bam"))
    assert size // 2 >= 400                                                                # (a member of 300 inflated bytes takes some 330 at the most: half the file holds whole ones)
    two, _ = run_files(tmp_path, recs, bed, pc.NAMES, pc.LENS, direct, block=300, min_mapq=1, window_bytes=size // 2)
    same(two, res)


OOM = re.compile(r"out of device memory: gce_bam_pileup needs 64 bytes per site \((\d+) sites: (\d+) bytes\) \+ 16 bytes per interval \+ one window \+ 4 bytes per window record "
                 r"\(\d+ bytes live, budget (\d+), (\d+) more for the counters and the interval table\)")


@pytest.mark.gpu
@VARIANTS
def test_budget_and_site_limit(built, tmp_path, direct):
    """a budget that cannot hold the counters is GCE_ERR_OOM with the footprint in its message; more than 2^28 sites is GCE_ERR_INVALID;
    neither leaves a file"""
    from gencore_amd.bamio import pileup_bam
    from gencore_amd.capi import GceError
    bam, bed = tmp_path / "in.bam", tmp_path / "t.bed"
    pc.write_raw_bam(str(bam), [pc.rec(0, 10, "2M")], ["c0"], [1 << 30])
    bed.write_text("c0\t0\t%d\n" % (1 << 20))
    with pytest.raises(GceError) as ei:
        pileup_bam(bam, bed, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=1 << 20)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and str(ei.value).endswith(m.group(0)), str(ei.value)
    assert [int(x) for x in m.groups()[:3]] == [1 << 20, 64 << 20, 1 << 20] and int(m.group(4)) > 64 << 20
    bed.write_text("c0\t0\t%d\n" % ((1 << 28) + 1))
    with pytest.raises(GceError) as ei:
        pileup_bam(bam, bed, tsv=tmp_path / "out.tsv", direct=direct)
    assert ei.value.status == -1 and "more than 2^28 sites" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "t.bed"]


@pytest.mark.gpu
@VARIANTS
def test_malformed_records(built, tmp_path, direct):
    """the lowest record whose fields overrun its block_size is named; no table, no temporary file"""
    from gencore_amd.bamio import pileup_bam
    from gencore_amd.capi import GceError
    good = [pc.rec(0, 10 + k, "3M", "ACG") for k in range(40)]
    (tmp_path / "t.bed").write_text("c0\t0\t90\n")
    for k, (label, bad) in enumerate(pc.malformed()):
        at = 17 + 8 * k
        recs = good[:at] + [bad] + good[at:] + [pc.malformed()[0][1]]
        with pytest.raises(pypileup.PileupError) as mi:
            pypileup.pileup(recs, [(0, 0, 90)], pc.LENS)
        assert mi.value.record == at
        bam = tmp_path / ("%s.bam" % label)
        pc.write_raw_bam(str(bam), recs)
        with pytest.raises(GceError) as ei:
            pileup_bam(bam, tmp_path / "t.bed", tsv=tmp_path / "out.tsv", direct=direct)
        assert ei.value.status == -1 and ("BAM record %d (counting from 0)" % at) in str(ei.value), label
        bam.unlink()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["t.bed"]


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """one generated stream of 3000 pairs from the suite's generators as in.bam / ref.fa / panel.bed, a BED of a few dozen targets, and the
    model's result over the file as tests/pybam.py reads it -- computed once"""
    from test_cli_gpu import write_inputs
    from test_depth_bed import depth_case
    d = tmp_path_factory.mktemp("pileupstream")
    data, batch, _, panel = depth_case("cfg3", 3000)
    regions = [(t, a - 150 + 20 * k, a - 150 + 20 * k + 12) for t, a, _ in panel[:2] for k in range(18)]       # 36 targets of 12 sites over the reads
    targets = write_inputs(d, data, batch, regions)
    names, lens = [t[0] for t in targets], [t[1] for t in targets]
    _, _, recs = pybam.read_bam(str(d / "in.bam"))
    bed = pypileup.read_bed(str(d / "panel.bed"), names)
    assert len(bed) == 37 and len(recs) >= 6000                # (the 37th: a region on a contig the header lacks)
    res = pypileup.pileup(recs, bed, lens, 0, 20)
    return d, names, lens, bed, res, pypileup.read_fasta(str(d / "ref.fa"))


@pytest.mark.gpu
@VARIANTS
def test_generated_stream_and_table(built, stream, tmp_path, direct):
    """the generated stream against the model; the table's text against the model's, byte for byte, with and without a FASTA"""
    from gencore_amd.bamio import pileup_bam
    d, names, lens, bed, res, fasta = stream
    assert res["n_eligible"] > 5000 and res["n_sites"] == 36 * 12 and res["n_intervals"] == 36 and sum(map(sum, res["counts"])) > 10000
    run = pileup_bam(d / "in.bam", d / "panel.bed", fasta=d / "ref.fa", tsv=tmp_path / "with.tsv", min_baseq=20, direct=direct, threads=2)
    same(run, res)
    assert (tmp_path / "with.tsv").read_bytes() == pypileup.table(res, names, fasta)
    bare = pileup_bam(d / "in.bam", d / "panel.bed", tsv=tmp_path / "bare.tsv", min_baseq=20, direct=direct, threads=2)
    same(bare, res)
    text = (tmp_path / "bare.tsv").read_bytes()
    assert text == pypileup.table(res, names) and {l.split(b"\t")[2] for l in text.split(b"\n")[1:-1]} == {b"N"}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bare.tsv", "with.tsv"]


@pytest.mark.gpu
def test_command_line_before_and_after(built, stream, tmp_path):
    """one run with --pileup_in and --pileup: both tables equal the model's over the input and over the output file, and at every site the
    output's depth is at most the input's"""
    from test_cli_gpu import cli
    d, names, lens, bed, before, fasta = stream
    r = cli(["-i", str(d / "in.bam"), "-o", "out.bam", "-r", str(d / "ref.fa"), "-b", str(d / "panel.bed"), "-j", "r.json", "--threads", "4", "--pileup_in", "before.tsv",
             "--pileup", "after.tsv", "--pileup_min_baseq", "20"], tmp_path)
    assert r.returncode == 0, r.stderr
    depth = {}
    for label, bam, tsv in (("pileup_in", d / "in.bam", "before.tsv"), ("pileup", tmp_path / "out.bam", "after.tsv")):
        res = before if label == "pileup_in" else pypileup.pileup(pybam.read_bam(str(bam))[2], bed, lens, 0, 20)
        assert (tmp_path / tsv).read_bytes() == pypileup.table(res, names, fasta), label
        assert ("%s: %d records, %d eligible, %d sites\n" % (label, res["n_records"], res["n_eligible"], res["n_sites"])) in r.stderr
        depth[label] = [sum(k[0:5]) + sum(k[8:13]) for k in res["counts"]]
    assert len(depth["pileup"]) == len(depth["pileup_in"]) == 36 * 12 and sum(depth["pileup"]) > 0
    assert all(a <= b for a, b in zip(depth["pileup"], depth["pileup_in"]))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["after.tsv", "before.tsv", "out.bam", "r.json"]
