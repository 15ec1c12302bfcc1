"""gce_bam_pileup without a GPU: the model of the rules (tests/pypileup.py) against records whose counters are written out by
hand (tests/pileupcases.py), the symbol, its prototype and its argument checks, the flags of the command line, and the per-record functions
of the kernels (gce_pileup.hpp) compiled for the host under the address and undefined-behaviour sanitizers and compared with the model."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import pileupcases as pc
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_model(cs, records=None):
    return pypileup.pileup(cs["records"] if records is None else records, pc.regions_of(cs), pc.LENS, cs["min_mapq"], cs["min_baseq"], cs["exclude"])


def test_model_against_hand_cases():
    labels = [c["label"] for c in pc.all_cases()]
    assert len(set(labels)) == len(labels) and len(labels) >= 30
    for cs in pc.all_cases():
        res = run_model(cs)
        sites = list(zip(res["tid"], res["pos"]))
        assert sites == sorted(sites) and len(sites) == res["n_sites"], cs["label"]
        assert res["counts"] == pc.expected_counts(cs, sites), cs["label"]
        assert {k: res[k] for k in pypileup.SKIPS} == cs["skips"], cs["label"]
        assert res["n_records"] == len(cs["records"]) == res["n_eligible"] + sum(cs["skips"].values()), cs["label"]
        if cs["n_sites"] is not None:
            assert res["n_sites"] == cs["n_sites"], cs["label"]
        if cs["n_intervals"] is not None:
            assert res["n_intervals"] == cs["n_intervals"], cs["label"]
    # a skipped record adds nothing: every skip case's counters are those of its eligible records alone
    for cs in pc.all_cases():
        if sum(cs["skips"].values()):
            f = [pypileup.fields(r) for r in cs["records"]]
            kept = [r for r, x in zip(cs["records"], f) if pypileup.skip_of(x, len(pc.LENS), cs["min_mapq"], cs["exclude"]) is None]
            assert run_model(cs, kept)["counts"] == run_model(cs)["counts"], cs["label"]


def test_model_refusals_and_table():
    cs = pc.all_cases()[0]
    for label, bad in pc.malformed():
        with pytest.raises(pypileup.Malformed):
            pypileup.fields(bad)
        with pytest.raises(pypileup.PileupError) as ei:
            run_model(cs, cs["records"] * 3 + [bad] + cs["records"] + [pc.malformed()[0][1]])
        assert ei.value.record == 3, label
    with pytest.raises(pypileup.PileupError):
        pypileup.intervals([(0, 0, (1 << 28) + 1)], [1 << 30])
    assert pypileup.intervals([(0, 0, 1 << 28)], [1 << 30])[1] == 1 << 28
    res = run_model(cs)
    text = pypileup.table(res, pc.NAMES, {"c0": "acgtacgtacgtACGT"}).decode().split("\n")
    assert text[0].startswith("#contig\tpos\tref\tdepth\tfwd_A\t") and text[0].endswith("\trev_LOWQ") and len(text[0].split("\t")) == 20
    assert text[1] == "c0\t11\tG\t1\t0\t1" + "\t0" * 14 and text[6].split("\t")[:4] == ["c0", "16", "T", "0"] and text[7].split("\t")[2] == "N"
    assert pypileup.table(run_model([c for c in pc.all_cases() if c["label"] == "empty_bed"][0]), pc.NAMES) == pypileup.HEADER.encode()


def test_symbol_prototype_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_pileup(const char *bam_path, const char *bed_path, const char *fasta_path /* NULL: ref = N */, const char *tsv_path /* NULL: no file */, "
            "int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, "
            "gce_pileup_run *out, char err[256]);") in head
    assert "void gce_pileup_free(gce_pileup_run *out);" in head and "#define GCE_PILEUP_DIRECT 1u" in head
    doc = head[head.index("Bases per strand at the sites of a BED file"):head.index("} gce_pileup_run;")]
    assert "addition under ABI v3" in doc and "Replaces: nothing in the reference's source" in doc
    lib = capi.load_library()
    for n in ("gce_bam_pileup", "gce_pileup_free"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n)
    for n in ("gce_pileup_create", "gce_pileup_set_sites", "gce_pileup_window", "gce_pileup_finish", "gce_pileup_error", "gce_pileup_destroy"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS
    assert lib.gce_bam_pileup.argtypes == [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_size_t,
                                           C.POINTER(capi.GcePileupRun), C.c_char_p]
    assert [n for n, _ in capi.GcePileupRun._fields_] == ["n_records", "n_eligible", "n_unplaced", "n_flagged", "n_low_mapq", "n_no_cigar", "n_no_seq", "n_bad_cigar", "n_sites",
                                                          "n_intervals", "peak_device_bytes", "read_s", "inflate_index_s", "pileup_s", "write_s", "total_s", "site_tid", "site_pos", "counts"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %u\\n",sizeof(gce_pileup_run),GCE_PILEUP_DIRECT);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GcePileupRun), capi.GCE_PILEUP_DIRECT]
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the argument checks come before any device is touched
    run, err = capi.GcePileupRun(), (C.c_char * 256)()
    bam, bed, fa, tsv = (str(tmp_path / n).encode() for n in ("in.bam", "t.bed", "ref.fa", "out.tsv"))
    call = lambda b=bam, d=bed, f=None, mq=0, bq=0, opt=0, r=C.byref(run): lib.gce_bam_pileup(b, d, f, tsv, 0, 1, mq, bq, 0x704, opt, 0, 0, r, err)
    assert call(b=None) == -1 and call(d=None) == -1 and call(r=None) == -1
    for v in (-1, 256):
        assert call(mq=v) == -1 and b"min_mapq should be 0..255" in err.value
        assert call(bq=v) == -1 and b"min_baseq should be 0..255" in err.value
    for opt in (2, 3, 1 << 31):
        assert call(opt=opt) == -1 and b"unknown option bit" in err.value
    assert call() == -1 and b"cannot open the BED file" in err.value
    (tmp_path / "t.bed").write_text("c0\t1\t2\n")
    assert call(f=fa) == -1 and b"cannot open the reference FASTA" in err.value
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    for opt in (0, 1):
        assert call(f=fa, opt=opt) == -1 and b"cannot open the BAM file" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert call(f=fa) == -1 and err.value == b"gce_bam_pileup reads BAM, not SAM text"
    with pytest.raises(capi.GceError) as ei:
        bamio.pileup_bam(tmp_path / "in.bam", tmp_path / "t.bed", tsv=tmp_path / "out.tsv", direct=True)
    assert ei.value.status == -1 and "gce_bam_pileup reads BAM, not SAM text" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa", "t.bed"]
    lib.gce_pileup_free(None)
    lib.gce_pileup_free(C.byref(run))
    sig = inspect.signature(bamio.pileup_bam)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("fasta", None), ("tsv", None), ("device", 0), ("threads", 0), ("min_mapq", 0), ("min_baseq", 0),
                                                                          ("exclude_flags", 0x704), ("direct", False), ("window_bytes", 0), ("device_budget_bytes", 0)]


def test_tile_constant_is_checked_against_the_lds():
    src = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_pileup.hpp")).read()
    tile = int(re.search(r"#define PU_TILE (\d+)u", src).group(1))
    assert tile * 64 + 64 <= (160 << 10) // 8 and "static_assert(PU_TILE * 64u + 64u <= PU_LDS_PER_CU / PU_BLOCKS_PER_CU" in src
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_pileup_create", "gce_pileup_set_sites", "gce_pileup_window", "gce_pileup_finish", "gce_pileup_error", "gce_pileup_destroy"):
        assert re.search(r"\b%s\(" % n, entry), n


def test_help_names_the_flags():
    from gencore_amd.cli import EPILOG, build_parser
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--pileup FILE \[gencore_amd\]", h) and re.search(r"--pileup_in FILE \[gencore_amd\]", h)
    assert re.search(r"--pileup_min_mapq PILEUP_MIN_MAPQ \[gencore_amd\]", h) and re.search(r"--pileup_min_baseq PILEUP_MIN_BASEQ \[gencore_amd\]", h)
    assert "--pileup FILE and --pileup_in FILE" in EPILOG and "0x704" in EPILOG and "counted twice" in EPILOG and "no BAQ" in EPILOG
    o = build_parser().parse_args(["-r", "x"])
    assert (o.pileup, o.pileup_in, o.pileup_min_mapq, o.pileup_min_baseq) == (None, None, 0, 0)


@pytest.mark.parametrize("argv, words", [
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--pileup", "{dir}/a.tsv"], "--pileup needs the targets of -b"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--pileup_in", "{dir}/b.tsv"], "--pileup_in needs the targets of -b"),
    (["-i", "{bam}", "-r", "{fa}", "-b", "{bed}", "--pileup", "{dir}/a.tsv"], "--pileup needs an output file, not STDOUT"),
    (["-i", "{bam}", "-o", "{dir}/out.sam", "-r", "{fa}", "-b", "{bed}", "--pileup", "{dir}/a.tsv"], "--pileup needs BAM output, not SAM text"),
    (["-o", "{dir}/out.bam", "-r", "{fa}", "-b", "{bed}", "--pileup_in", "{dir}/b.tsv"], "--pileup_in needs an input file, not STDIN"),
    (["-i", "{sam}", "-o", "{dir}/out.bam", "-r", "{fa}", "-b", "{bed}", "--pileup_in", "{dir}/b.tsv"], "--pileup_in needs BAM input, not SAM text"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "-b", "{bed}", "--pileup", "{dir}/a.tsv", "--pileup_min_mapq", "256"], "pileup_min_mapq should be 0..255"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "-b", "{bed}", "--pileup_in", "{dir}/b.tsv", "--pileup_min_baseq", "-1"], "pileup_min_baseq should be 0..255"),
])
def test_flag_validation_errors(tmp_path, capsys, argv, words):
    from gencore_amd.cli import main
    bam, sam, fa, bed = tmp_path / "in.bam", tmp_path / "in.sam", tmp_path / "ref.fa", tmp_path / "t.bed"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    sam.write_text("@HD\tVN:1.6\n")
    fa.write_text(">c0\nACGT\n")
    bed.write_text("c0\t1\t2\n")
    sub = dict(bam=str(bam), sam=str(sam), fa=str(fa), bed=str(bed), dir=str(tmp_path))
    assert main([a.format(**sub) for a in argv]) == 255
    assert ("ERROR: " + words) in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "in.sam", "ref.fa", "t.bed"]


def test_sam_text_under_sort_sam_passes_validation(tmp_path):
    """--pileup_in reads the sorted temporary BAM under --sort_sam: SAM text input is no usage error there"""
    from gencore_amd.cli import build_parser, validate
    sam, fa, bed = tmp_path / "in.sam", tmp_path / "ref.fa", tmp_path / "t.bed"
    sam.write_text("@HD\tVN:1.6\n")
    fa.write_text(">c0\nACGT\n")
    bed.write_text("c0\t1\t2\n")
    o = build_parser().parse_args(["-i", str(sam), "-o", str(tmp_path / "out.bam"), "-r", str(fa), "-b", str(bed), "--sort_sam", "--pileup_in", str(tmp_path / "b.tsv")])
    assert validate(o) == [0]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """pileup_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("pileuphost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "pileup_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "pileup_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, regions, lens, min_mapq, min_baseq, exclude):
    iv, n_sites = pypileup.intervals(regions, lens)
    (d / "intervals").write_text("".join("%d %d %d %d\n" % x for x in iv))
    (d / "frames").write_bytes(pc.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(len(lens)), str(min_mapq), str(min_baseq), str(exclude), str(d / "intervals"), str(d / "frames"), str(d / "out")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    rows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    return rows, np.frombuffer((d / "out").read_bytes(), np.uint32).reshape(n_sites, 16).tolist()


def test_record_functions_on_the_host(host_check):
    """pileup::scan_record and pileup::count_record on the host, under -fsanitize=address,undefined, with one lane and with 16 lanes: the
    skip of every record and every counter equal the model's and the hand-written numbers, over all of pileupcases"""
    d, exe = host_check
    order = [None] + ["n_unplaced", "n_flagged", "n_low_mapq", "n_no_cigar", "n_no_seq", "n_bad_cigar"]
    for cs in pc.all_cases():
        rows, counts = host_run(d, exe, cs["records"], pc.regions_of(cs), pc.LENS, cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        res = run_model(cs)
        assert counts == res["counts"] == pc.expected_counts(cs, list(zip(res["tid"], res["pos"]))), cs["label"]
        assert len(rows) == len(cs["records"])
        for k, r in enumerate(cs["records"]):
            assert rows[k][1] == 0 and order[rows[k][2]] == pypileup.skip_of(pypileup.fields(r), len(pc.LENS), cs["min_mapq"], cs["exclude"]), (cs["label"], k)
    # the malformed records: refused, nothing read beyond their block, nothing added
    cs = pc.all_cases()[0]
    recs = [b for _, b in pc.malformed()] + [b"\x05\0\0\0abcde", b"\x40\0\0\0" + bytes(40), b"\x01\0"]
    rows, counts = host_run(d, exe, recs, pc.regions_of(cs), pc.LENS, 0, 0, 0x704)
    assert [r[1:4] for r in rows] == [[1, 0, -1]] * len(recs) and not any(any(c) for c in counts)


def test_one_long_stream_on_the_host(host_check):
    """every hand case's records on one set of intervals that cuts through them, and long ops over many intervals: 16 lanes against the model"""
    d, exe = host_check
    recs = [r for cs in pc.all_cases() for r in cs["records"]]
    recs += [pc.rec(0, 0, "40M20D5I30M", "ACGT" * 18 + "ACG", flag=16), pc.rec(0, 3, "17M60N17M", "ACGTN" * 6 + "ACGT", [k % 41 for k in range(34)]), pc.rec(1, 0, "50M", "GATTACA" * 7 + "G")]
    regions = [(0, a, a + w) for a, w in ((0, 1), (2, 3), (9, 2), (12, 1), (14, 5), (30, 17), (48, 1), (60, 25), (99, 5))] + [(1, 0, 50), (1, 10, 20)]
    for mq, bq in ((0, 0), (10, 20)):
        rows, counts = host_run(d, exe, recs, regions, pc.LENS, mq, bq, 0x704)
        res = pypileup.pileup(recs, regions, pc.LENS, mq, bq, 0x704)
        assert counts == res["counts"] and sum(map(sum, counts)) >= 50              # (the 50M read on c1's 50 sites alone adds 50)
        assert sum(1 for r in rows if r[2] == 0) == res["n_eligible"]
