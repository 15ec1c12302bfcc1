"""--merge_overlap on the command line: the output is the model (tests/pyovlmerge.py) applied to the output of the same command
without the flag, alone and behind --calmd with --index; the line on STDERR; the --pileup table, written in front of it, is what it is
without the flag; the usage errors."""
import pytest

import pyfragpile
import pyovlmerge


@pytest.fixture(scope="module")
def consensus_input(tmp_path_factory):
    """the generated stream of test_fragpile_gpu.py's command-line test: 600 pairs as in.bam / ref.fa / panel.bed"""
    from test_cli_gpu import write_inputs
    from test_depth_bed import depth_case
    d = tmp_path_factory.mktemp("overlapstream")
    data, batch, _, panel = depth_case("cfg3", 600)
    regions = [(t, a - 150 + 20 * k, a - 150 + 20 * k + 12) for t, a, _ in panel[:2] for k in range(18)]
    write_inputs(d, data, batch, regions)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--calmd", "--index"]], ids=["alone", "calmd_index"])
def test_merge_overlap_flag(built, consensus_input, tmp_path, extra):
    from gencore_amd.bamio import index_bam
    from test_cli_gpu import cli
    d = consensus_input
    base = ["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-b", str(d / "panel.bed"), "--threads", "4", "--level", "-2"] + extra
    r0 = cli(base + ["-o", "plain.bam", "-j", "plain.json", "--pileup", "plain.tsv"], tmp_path)
    r1 = cli(base + ["-o", "merged.bam", "-j", "merged.json", "--pileup", "merged.tsv", "--merge_overlap"], tmp_path)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    names, lens, recs = pyfragpile.read_raw_records(str(tmp_path / "plain.bam"))
    want, res = pyovlmerge.merge_overlap(recs)
    assert res["n_pairs"] > 50 and res["n_shared_columns"] > 1000 and res["n_records_changed"] > 100
    got = pyfragpile.read_raw_records(str(tmp_path / "merged.bam"))
    assert got[:2] == (names, lens) and got[2] == want
    assert ("merge_overlap: %d pairs, %d shared columns, %d disagreeing, %d records changed\n" % (res["n_pairs"], res["n_shared_columns"], res["n_disagree_columns"], res["n_records_changed"])) in r1.stderr
    assert "merge_overlap:" not in r0.stderr
    assert (tmp_path / "plain.tsv").read_bytes() == (tmp_path / "merged.tsv").read_bytes() and (tmp_path / "plain.json").exists()
    files = ["merged.bam", "merged.json", "merged.tsv", "plain.bam", "plain.json", "plain.tsv"]
    if extra:
        index_bam(tmp_path / "merged.bam", tmp_path / "check.bai", threads=2)
        assert (tmp_path / "merged.bam.bai").read_bytes() == (tmp_path / "check.bai").read_bytes() and (tmp_path / "check.bai").stat().st_size > 100
        files += ["check.bai", "merged.bam.bai", "plain.bam.bai"]
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(files)


@pytest.mark.gpu
def test_usage_errors(built, consensus_input, tmp_path):
    from test_cli_gpu import cli
    d = consensus_input
    for out, words in (("-", "--merge_overlap needs an output file, not STDOUT"), ("out.sam", "--merge_overlap needs BAM output, not SAM text")):
        r = cli(["-i", str(d / "in.bam"), "-o", out, "-r", str(d / "ref.fa"), "--merge_overlap"], tmp_path)
        assert r.returncode == 255 and ("ERROR: " + words) in r.stderr and r.stdout == ""
    assert list(tmp_path.iterdir()) == []
