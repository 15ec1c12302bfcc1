"""The command line and the reports (gencore_amd/cli.py, gencore_amd/csrc/gce_report.hpp), without a GPU.

Report writer: gce_report_json on hand-built Stats, depth bins and regions against golden files derived by reading the reference's
writers (src/jsonreporter.cpp:11-44, src/stats.cpp:153-193, src/bed.cpp:81-100).  Summary: gce_report_summary against Stats::print
(src/stats.cpp:195-215) worked by hand.  Header reader: gce_bam_read_header against files tests/pybam.py writes.  Validation:
`python -m gencore_amd` in a subprocess, one case per rule of src/main.cpp:96-98 and Options::validate (src/options.cpp:42-111)."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import pytest

import pybam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "report")


def stats(**kw):
    from gencore_amd.capi import GceStats
    s = GceStats()
    hist = kw.pop("hist", {})
    for k, v in kw.items():
        setattr(s, k, v)
    for i, v in hist.items():
        s.supporting_hist[i] = v
    return s


# Stats of the first golden file.  pre: mapping_rate 990/1000 = 0.99; duplication_rate 1 - (20 + 2 * 480) / 990 = 0.0101010.. -> "0.010101";
# mismatch_rate 333 / 148500 = 0.00224242..; post mismatch_rate 7 / 147000 = 4.76190e-05 -> "4.7619e-05" (%g drops the trailing 0).
PRE = dict(reads=1000, bases=150000, reads_unmapped=10, bases_unmapped=1500, base_mismatches=333, reads_with_mismatches=200, clusters=400,
           multi_molecule_clusters=12, molecules=500, molecules_se=20, molecules_pe=480, hist={1: 300, 2: 150, 3: 40, 10: 4, 99: 6})
POST = dict(reads=980, bases=147000, base_mismatches=7, reads_with_mismatches=5, clusters=400, multi_molecule_clusters=12, molecules=490,
            molecules_se=10, molecules_pe=480, sscs=300, dcs=180, hist={1: 490})


def test_report_json_with_bed(built, tmp_path):
    """Two contigs (chrB has no region), step 100.  Bins print round(depth / 100) half away from zero: pre chrA 150 -> 2 (.5 up), 50 -> 1,
    chrB 249 -> 2, 1000 -> 10; post chrA 49 -> 0, 250 -> 3.  Regions: r1 [10,110) count 250 -> 2.5 -> 3 (post 149 -> 1); a contig not in the
    header (tid -1) is left out; "empty" (end == start) and "neg" (end < start) are 0 whatever their count; "" [0,3) 4 -> 1 (post 5 -> 2)."""
    from gencore_amd.report import write_json
    depth = dict(bin_off=[0, 3, 5], pre_depth=[150, 50, 0, 249, 1000], post_depth=[100, 49, 250, 0, 1],
                 regions=[(0, 10, 110), (-1, 5, 50), (0, 200, 200), (0, 300, 250), (0, 0, 3)],
                 pre_bed=[250, 0, 77, 0, 4], post_bed=[149, 0, 5, 0, 5], pre=stats(**PRE), post=stats(**POST))
    out = tmp_path / "r.json"
    write_json(out, depth, ["chrA", "chrB"], 100, "gencore -i in.bam -o out.bam -r ref.fa -b panel.bed -j r.json ",
               region_names=["r1", "offhdr", "empty", "neg", ""], has_bed=True)
    want = open(os.path.join(GOLDEN, "bed_two_contigs.json"), "rb").read()
    assert out.read_bytes() == want
    rep = json.loads(want)
    assert list(rep) == ["summary", "before_processing", "after_processing", "command"]
    assert rep["before_processing"]["duplication_level_histogram"][-1] == 6 and len(rep["before_processing"]["duplication_level_histogram"]) == 99


def test_report_json_without_mapped_reads_or_bed(built, tmp_path):
    """No mapped read: mapping_rate 0 / 4.0 = 0, duplication_rate 1 - 0 / 0.0 and both mismatch rates 0 / 0.0 are the NaN of x86 (sign set),
    which glibc prints "-nan".  No BED file: no coverage_bed key, the coverage block ends the Stats block."""
    from gencore_amd.report import write_json
    depth = dict(bin_off=[0, 1, 3], pre_depth=[0, 0, 0], post_depth=[0, 0, 0], pre=stats(reads=4, bases=400, reads_unmapped=4, bases_unmapped=400),
                 post=stats())
    out = tmp_path / "u.json"
    write_json(out, depth, ["chrM", "c1"], 10000, "gencore -i u.bam -r ref.fa ")
    assert out.read_bytes() == open(os.path.join(GOLDEN, "no_mapped_reads.json"), "rb").read()
    assert b"coverage_bed" not in out.read_bytes()


def test_report_json_rejects_bad_arguments(built, tmp_path):
    from gencore_amd.capi import GceError
    from gencore_amd.report import write_json
    depth = dict(bin_off=[0, 1], pre_depth=[0], post_depth=[0], pre=stats(), post=stats())
    with pytest.raises(GceError):
        write_json(tmp_path / "x.json", depth, ["c"], 0, "")
    with pytest.raises(GceError):
        write_json(tmp_path / "no_such_dir" / "x.json", depth, ["c"], 10, "")


SUMMARY_PRE = """\
Total reads: 1000
Total bases: 150000
Mapped reads: 990 (99.000000%)
Mapped bases: 148500 (99.000000%)
Bases mismatched with reference: 333 (0.224242%)
Reads with mismatched bases: 200 (20.202020%)
Total mapping clusters: 400
Mapping clusters with multiple fragments: 12
Total fragments: 500
Fragments with single-end reads: 20
Fragments with paired-end reads: 480
Duplication level histogram:
    Fragments with 1 duplicates: 300
    Fragments with 2 duplicates: 150
    Fragments with 3 duplicates: 40
""".replace("histogram:\n", "histogram: \n")        # stats.cpp:208 prints a blank behind the colon

SUMMARY_POST = """\
Total reads: 980
Total bases: 147000
Mapped reads: 980 (100.000000%)
Mapped bases: 147000 (100.000000%)
Bases mismatched with reference: 7 (0.004762%)
Reads with mismatched bases: 5 (0.510204%)
Total mapping clusters: 400
Mapping clusters with multiple fragments: 12
Total fragments: 490
Fragments with single-end reads: 10
Fragments with paired-end reads: 480

Single Stranded Consensus Sequence (has 'FR' tag): 300
Duplex Consensus Sequence (has both 'FS' and 'RR' tags): 180
"""


def test_summary_text(built):
    """Stats::print: percentages by std::to_string (%f); the pre block lists the histogram up to the first empty entry (entry 4 here, so
    entry 10 is never reached); the post block has no histogram but the SSCS / DCS lines after an empty line."""
    from gencore_amd.report import summary
    assert summary(stats(**PRE), False) == SUMMARY_PRE
    assert summary(stats(**POST), True) == SUMMARY_POST


def test_summary_buffer_too_small(built):
    from gencore_amd import capi
    lib = capi.load_library()
    st, n = stats(**PRE), C.c_size_t()
    buf = C.create_string_buffer(10)
    assert lib.gce_report_summary(C.byref(st), 0, buf, 10, C.byref(n)) != 0 and n.value == len(SUMMARY_PRE)


def _pairs(n, n_targets=1):
    recs = []
    for m in range(n):
        left = 50 + 3 * m
        isz = 140
        q = [30 + (m + k) % 9 for k in range(20)]
        seq = "ACGTTGCA" * 2 + "ACGT"
        recs.append(dict(qname="p%06d" % m, flag=99, tid=m % n_targets, pos=left, cigar="20M", mtid=m % n_targets, mpos=left + 120, isize=isz, seq=seq, qual=q, nm=0))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs


def test_read_header_bam_and_sam(built, tmp_path):
    from gencore_amd.report import read_header
    targets = [("chr1", 248956422), ("chrM", 16569), ("HLA-A*01:01:01:01", 3503)]
    pybam.write_bam(str(tmp_path / "a.bam"), _pairs(50), targets)
    assert read_header(tmp_path / "a.bam") == ([t[0] for t in targets], [t[1] for t in targets])
    pybam.write_sam(str(tmp_path / "a.sam"), _pairs(50), targets)
    assert read_header(tmp_path / "a.sam") == ([t[0] for t in targets], [t[1] for t in targets])
    pybam.write_sam(str(tmp_path / "crlf.sam"), _pairs(5), targets, newline="\r\n")
    assert read_header(tmp_path / "crlf.sam")[0] == [t[0] for t in targets]
    pybam.write_sam(str(tmp_path / "none.sam"), [], [], sq_lines=False)
    assert read_header(tmp_path / "none.sam") == ([], [])


def test_read_header_spanning_many_members(built, tmp_path):
    """A header of 3000 contigs (~100 KB) cut into 700-byte BGZF members, plus a long text part."""
    from gencore_amd.report import read_header
    targets = [("contig_%05d_%s" % (k, "x" * (k % 17)), 1000 + 7 * k) for k in range(3000)]
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@CO\tcomment %d\n" % k for k in range(500))
    p = str(tmp_path / "big.bam")
    pybam.write_bam(p, _pairs(20, 3000), targets, text=text, block=700)
    assert read_header(p) == ([t[0] for t in targets], [t[1] for t in targets])


def _member_ends(data):
    ends, o = [], 0
    while o < len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bsize = struct.unpack_from("<H", data, o + 12 + xlen - 2)[0]        # the BC subfield is the only one pybam writes
        o += bsize + 1
        ends.append(o)
    return ends


def test_read_header_inflates_only_the_header(built, tmp_path):
    """A small header in front of a large body (thousands of records): every member after the first is overwritten with garbage, so a
    reader that inflated more than the header's members would fail."""
    from gencore_amd.report import read_header
    p = tmp_path / "body.bam"
    pybam.write_bam(str(p), _pairs(20000), [("chr1", 100000)], block=0x4000)
    data = bytearray(p.read_bytes())
    ends = _member_ends(bytes(data))
    assert len(ends) > 20
    data[ends[0]:] = b"\xa5" * (len(data) - ends[0])
    p.write_bytes(bytes(data))
    assert read_header(p) == (["chr1"], [100000])


def test_read_header_errors(built, tmp_path):
    from gencore_amd.capi import GceError
    from gencore_amd.report import read_header
    with pytest.raises(GceError):
        read_header(tmp_path / "missing.bam")
    p = tmp_path / "t.bam"
    pybam.write_bam(str(p), [], [("chr1", 100)] * 400, block=200)
    data = p.read_bytes()
    p.write_bytes(data[:_member_ends(data)[2]])                              # the file ends inside the contig table
    with pytest.raises(GceError):
        read_header(p)


# ------------------------------------------------------------------------------------------------------------------ the command line
def cli(args, cwd, timeout=60):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "gencore_amd"] + list(args), cwd=str(cwd), env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


# (extra arguments, the message), in the order of Options::validate.  Every rule has a rejected value just past its bound here, and the
# value on the bound in ACCEPTED below.
REJECTED = [
    (["-a", "1.01"], "ERROR: ratio_threshold cannot be greater than 1.0"),
    (["-a", "0.49"], "ERROR: ratio_threshold cannot be less than 0.5"),
    (["-s", "11"], "ERROR: supporting_reads cannot be greater than 10"),
    (["-s", "0"], "ERROR: supporting_reads cannot be less than 1"),
    (["-c", "11"], "ERROR: score_threshold cannot be greater than 10"),
    (["-c", "0"], "ERROR: score_threshold cannot be less than 1"),
    (["--high_qual", "41"], "ERROR: high_qual cannot be greater than 40"),
    (["--high_qual", "19"], "ERROR: high_qual cannot be less than 20"),
    (["--moderate_qual", "36", "--high_qual", "40"], "ERROR: moderate_qual cannot be greater than 35"),
    (["--moderate_qual", "14"], "ERROR: moderate_qual cannot be less than 15"),
    (["--low_qual", "31", "--moderate_qual", "35", "--high_qual", "40"], "ERROR: low_qual cannot be greater than 30"),
    (["--low_qual", "7"], "ERROR: low_qual cannot be less than 8"),
    (["-d", "11"], "ERROR: umi_diff_threshold cannot be greater than 10"),
    (["-d", "-1"], "ERROR: umi_diff_threshold cannot be negative"),
    (["--low_qual", "21"], "ERROR: low_qual cannot be greater than moderate_qual"),
    (["--moderate_qual", "31"], "ERROR: moderate_qual cannot be greater than high_qual"),
    (["-D", "11"], "ERROR: duplex_diff_threshold cannot be greater than 10, suggest 2."),
    (["-D", "-1"], "ERROR: duplex_diff_threshold cannot be less than 0, suggest 2."),
    (["-x", "--no_duplex"], "ERROR: You cannot enable both duplex_only and no_duplex"),
    (["--coverage_sampling", "0"], "ERROR: coverage_sampling should be greater than 0"),
    (["--coverage_sampling", "-5"], "ERROR: coverage_sampling should be greater than 0"),
    (["-a", "2", "-s", "20", "-D", "99"], "ERROR: ratio_threshold cannot be greater than 1.0"),         # the first broken rule is reported
    (["-D", "99", "-x", "--no_duplex"], "ERROR: You cannot enable both duplex_only and no_duplex"),     # main.cpp checks this before validate()
]

ACCEPTED = [["-a", "1.0"], ["-a", "0.5"], ["-s", "10"], ["-s", "1"], ["-c", "10"], ["-c", "1"], ["--high_qual", "40"], ["--high_qual", "20"],
            ["--moderate_qual", "35", "--high_qual", "40"], ["--moderate_qual", "15"], ["--low_qual", "30", "--moderate_qual", "30", "--high_qual", "30"],
            ["--low_qual", "8"], ["-d", "10"], ["-d", "0"], ["--low_qual", "20"], ["--moderate_qual", "30"], ["-D", "10"], ["-D", "0"], ["-x"], ["--no_duplex"]]


@pytest.fixture
def workdir(tmp_path):
    (tmp_path / "in.bam").write_bytes(b"")
    return tmp_path


@pytest.mark.parametrize("case", range(len(REJECTED)))
def test_cli_rejects(workdir, case):
    extra, msg = REJECTED[case]
    r = cli(["-i", "in.bam", "-r", "ref.fa"] + extra, workdir)
    assert r.returncode != 0 and r.returncode != 124
    assert r.stderr == msg + "\n" and r.stdout == ""
    assert not (workdir / "gencore.json").exists()


@pytest.mark.parametrize("case", range(len(ACCEPTED)))
def test_cli_accepts_the_bound(workdir, case):
    """The value on the bound passes its rule: the run goes on to the next check, here the coverage step this command adds last."""
    r = cli(["-i", "in.bam", "-r", "ref.fa", "--coverage_sampling", "0"] + ACCEPTED[case], workdir)
    assert r.returncode != 0 and r.stderr == "ERROR: coverage_sampling should be greater than 0\n"


def test_cli_files(workdir):
    r = cli(["-r", "ref.fa"], workdir)                                        # -i defaults to "-", which check_file_valid does not find
    assert r.returncode != 0 and r.stderr == "ERROR: file '-' doesn't exist, quit now\n"
    r = cli(["-i", "missing.bam", "-r", "ref.fa"], workdir)
    assert r.returncode != 0 and r.stderr == "ERROR: file 'missing.bam' doesn't exist, quit now\n"
    os.mkdir(str(workdir / "adir"))
    r = cli(["-i", "adir", "-r", "ref.fa"], workdir)
    assert r.returncode != 0 and r.stderr == "ERROR: 'adir' is a folder, not a file, quit now\n"
    r = cli(["-i", "in.bam", "-r", "hg38.fa.gz"], workdir)
    assert r.returncode != 0 and r.stderr == "reference fasta file should not be compressed.\nplease unzip hg38.fa.gz and try again.\n"
    r = cli(["-i", "in.bam", "-r", "ref.fa", "-b", "missing.bed"], workdir)
    assert r.returncode != 0 and r.stderr == "ERROR: file 'missing.bed' doesn't exist, quit now\n"
    r = cli(["-i", "in.bam"], workdir)                                        # --ref is required (main.cpp:33)
    assert r.returncode != 0 and "--ref" in r.stderr


def test_cli_help(workdir):
    r = cli(["--help"], workdir)
    assert r.returncode == 0
    for flag in ("--in", "--out", "--ref", "--bed", "--duplex_only", "--no_duplex", "--umi_prefix", "--supporting_reads", "--ratio_threshold",
                 "--score_threshold", "--umi_diff_threshold", "--duplex_diff_threshold", "--high_qual", "--moderate_qual", "--low_qual",
                 "--coverage_sampling", "--json", "--html", "--debug", "--quit_after_contig", "--devices", "--threads", "--level"):
        assert flag in r.stdout, flag
    assert "Known difference" in r.stdout


def test_cli_maps_flags_to_params():
    from gencore_amd import cli as m
    o = m.build_parser().parse_args(["-r", "x", "-a", "0.6", "-d", "3", "-D", "4", "-c", "5", "--quit_after_contig", "2", "-u", "UMI_", "-s", "3",
                                     "--high_qual", "35", "--moderate_qual", "25", "--low_qual", "10", "--no_duplex"])
    p = m.params_of(o)
    assert (p.score_percent_req, p.proper_umi_diff_threshold, p.duplex_mismatch_threshold, p.base_score_req, p.max_contig) == (0.6, 3, 4, 5, 2)
    assert (p.umi_prefix, p.cluster_size_req, p.high_quality, p.moderate_quality, p.low_quality) == (b"UMI_", 3, 35, 25, 10)
    assert (p.disable_duplex, p.duplex_only) == (1, 0)
    d = m.build_parser().parse_args(["-r", "x"])
    assert (d.input, d.output, d.umi_prefix, d.json, d.coverage_sampling, d.supporting_reads) == ("-", "-", "auto", "gencore.json", 10000, 1)
    assert m.params_of(d).umi_prefix == b"auto"
