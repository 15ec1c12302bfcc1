"""gce_bam_error_profile without a GPU: the model of the rules (tests/pyerrprof.py) against records whose counters are written out
by hand (tests/errprofcases.py) and against tests/pycalmd.py's NM as an arbiter of its own, the symbol, its prototype and its argument checks,
the flags of the command line, and the per-record functions of the kernels (gce_errprof.hpp) compiled for the host under the address and
undefined-behaviour sanitizers and compared with the model, and its scan beside gce_bam_pileup's: one rule E."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import errprofcases as ec
import pileupcases as pc
import pycalmd
import pyerrprof
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_model(cs, records=None):
    return pyerrprof.profile(cs["records"] if records is None else records, ec.refs(), ec.LENS, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])


def test_model_against_hand_cases():
    labels = [c["label"] for c in ec.all_cases()]
    assert len(set(labels)) == len(labels) and len(labels) >= 35
    for cs in ec.all_cases():
        res = run_model(cs)
        assert pyerrprof.nonzero(res) == ec.expected(cs), cs["label"]
        assert {k: res[k] for k in pyerrprof.SKIPS} == cs["skips"], cs["label"]
        assert res["n_records"] == len(cs["records"]) == res["n_eligible"] + sum(cs["skips"].values()), cs["label"]
        assert all(row[21:] == [0, 0, 0] for seg in res["counts"] for row in seg), cs["label"]
        assert res["n_intervals"] == (-1 if cs["bed"] is None else len(pypileup.intervals(ec.regions_of(cs), ec.LENS)[0])), cs["label"]
        want = ec.expected(cs)
        assert res["n_bases"] == sum(v for (g, cy, cl), v in want.items() if ">" in cl), cs["label"]
        assert res["n_mismatches"] == sum(v for (g, cy, cl), v in want.items() if ">" in cl and cl[0] != cl[2]), cs["label"]
    # a skipped record adds nothing: every skip case's counters are those of its eligible records alone
    for cs in ec.all_cases():
        if sum(cs["skips"].values()):
            kept = [r for r in cs["records"] if pyerrprof.skip_of(pyerrprof.fields(r), ec.refs(), cs["min_mapq"], cs["exclude"]) is None]
            assert run_model(cs, kept)["counts"] == run_model(cs)["counts"], cs["label"]


def test_model_refusals_and_table():
    cs = ec.all_cases()[0]
    for label, bad in ec.malformed():
        with pytest.raises(pyerrprof.ErrprofError) as ei:
            run_model(cs, cs["records"] * 3 + [bad] + cs["records"] + [ec.malformed()[0][1]])
        assert ei.value.record == 3, label
    # rule O, from a model result: the header, one row per cycle up to the last with a counter, no row for a segment without one
    two = [c for c in ec.all_cases() if c["label"] == "g_to_t_apart_from_c_to_a"][0]
    res = run_model(two, two["records"] + [ec.rec(0, 0, "1S1I1M", "AAA", flag=0x80)])
    text = pyerrprof.table(res).decode().split("\n")
    assert text[0] == "#segment\tcycle\tbases\tmismatches\tA>A\tA>C\tA>G\tA>T\tC>A\tC>C\tC>G\tC>T\tG>A\tG>C\tG>G\tG>T\tT>A\tT>C\tT>G\tT>T\tREAD_N\tREF_OTHER\tLOWQ\tINS\tDEL"
    assert len(text[0].split("\t")) == 25 and text[-1] == "" and len(text) == 6
    assert text[1] == "0\t1\t2\t2" + "\t0" * 4 + "\t1" + "\t0" * 6 + "\t1" + "\t0" * 9                   # C>A is column 4, G>T column 11 of the 21
    assert text[2] == "2\t1" + "\t0" * 23                                                             # (cycle 1 of segment 2: the soft clip)
    assert text[3] == "2\t2\t0\t0" + "\t0" * 19 + "\t1\t0" and text[4] == "2\t3\t1\t0\t1" + "\t0" * 20
    assert pyerrprof.table(run_model([c for c in ec.all_cases() if c["label"] == "bed_empty"][0])) == pyerrprof.HEADER.encode()


def balance_records(seed, n):
    """reads of A C G T over c1 (A C G T only) with M, =, X, I, D, N and S ops, every column inside the contig"""
    rng = np.random.RandomState(seed)
    recs = []
    for k in range(n):
        ops, x, pos = [], 0, int(rng.randint(0, 10))
        if rng.randint(0, 3) == 0:
            ops.append((4, int(rng.randint(1, 4))))
        for _ in range(int(rng.randint(1, 5))):
            ops.append((int(rng.choice([0, 7, 8])), int(rng.randint(1, 6))))
            ops.append((int(rng.choice([1, 2, 3, 1, 2])), int(rng.randint(1, 4))))
        ops.append((0, int(rng.randint(1, 5))))
        if rng.randint(0, 3) == 0:
            ops.append((4, int(rng.randint(1, 4))))
        assert pos + sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8)) <= 50
        nq = sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
        recs.append(ec.rec(1, pos, ops, "".join("ACGT"[i] for i in rng.randint(0, 4, nq)), flag=int(rng.choice([0, 16, 0x40, 0x90]))))
    return recs


def test_table_balances_against_calmd_nm():
    """an arbiter that shares nothing with the model: over A C G T reads on an A C G T reference, without a BED and with min_baseq 0, the
    off-diagonal counts + INS + the D lengths summed from the CIGARs equal the sum of tests/pycalmd.py's NM over the same records"""
    contig = ec.FASTA["c1"].encode()
    for seed in (3, 4):
        recs = balance_records(seed, 60)
        nm = d_len = 0
        for r in recs:
            f = pyerrprof.fields(r)
            nm += pycalmd.walk(f["pos"], f["cigar"], lambda i, s=f["seq"]: (s[i >> 1] >> (0 if i & 1 else 4)) & 15, contig)[0]
            d_len += sum(ln for op, ln in f["cigar"] if op == 2)
        res = pyerrprof.profile(recs, ec.refs(), ec.LENS)
        ins = sum(row[pyerrprof.INS] for seg in res["counts"] for row in seg)
        other = sum(row[k] for seg in res["counts"] for row in seg for k in (pyerrprof.READ_N, pyerrprof.REF_OTHER, pyerrprof.LOWQ))
        assert res["n_eligible"] == 60 and other == 0 and res["n_mismatches"] > 50 and ins > 20 and d_len > 20
        assert res["n_mismatches"] + ins + d_len == nm, seed


def test_symbol_prototype_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_error_profile(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *tsv_path /* NULL: no file */, "
            "int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, "
            "gce_errprof_run *out, char err[256]);") in head
    assert "void gce_errprof_free(gce_errprof_run *out);" in head and "#define GCE_ERRPROF_DIRECT 1u" in head and "#define GCE_ERRPROF_MAX_CYCLE 1024" in head
    doc = head[head.index("Mismatches by read cycle against the reference"):head.index("} gce_errprof_run;")]
    assert "addition under ABI v3" in doc and "Replaces: nothing in the reference's source" in doc
    lib = capi.load_library()
    assert lib.gce_abi_version() == 3
    for n in ("gce_bam_error_profile", "gce_errprof_free"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n)
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_errprof_create", "gce_errprof_set_ref", "gce_errprof_set_sites", "gce_errprof_window", "gce_errprof_finish", "gce_errprof_error", "gce_errprof_destroy"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % n, entry), n
    assert lib.gce_bam_error_profile.argtypes == [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                  C.c_size_t, C.POINTER(capi.GceErrprofRun), C.c_char_p]
    assert [n for n, _ in capi.GceErrprofRun._fields_] == ["n_records", "n_eligible", "n_unplaced", "n_flagged", "n_low_mapq", "n_no_cigar", "n_no_seq", "n_bad_cigar", "n_no_ref",
                                                           "n_too_long", "n_bases", "n_mismatches", "n_intervals", "peak_device_bytes", "read_s", "inflate_index_s", "errprof_s",
                                                           "write_s", "total_s", "counts"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %u %d %d\\n",sizeof(gce_errprof_run),GCE_ERRPROF_DIRECT,GCE_ERRPROF_MAX_CYCLE,'
                     'GCE_ERRPROF_CLASSES);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GceErrprofRun), capi.GCE_ERRPROF_DIRECT, capi.GCE_ERRPROF_MAX_CYCLE,
                                                                                          capi.GCE_ERRPROF_CLASSES]
    assert (capi.GCE_ERRPROF_MAX_CYCLE, capi.GCE_ERRPROF_CLASSES) == (pyerrprof.MAX_CYCLE, pyerrprof.ROW)
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the argument checks come before any device is touched
    run, err = capi.GceErrprofRun(), (C.c_char * 256)()
    bam, bed, fa, tsv = (str(tmp_path / n).encode() for n in ("in.bam", "t.bed", "ref.fa", "out.tsv"))
    call = lambda b=bam, f=fa, d=None, mq=0, bq=0, opt=0, r=C.byref(run): lib.gce_bam_error_profile(b, f, d, tsv, 0, 1, mq, bq, 0x704, opt, 0, 0, r, err)
    assert call(b=None) == -1 and call(f=None) == -1 and call(r=None) == -1
    for v in (-1, 256):
        assert call(mq=v) == -1 and b"min_mapq should be 0..255" in err.value
        assert call(bq=v) == -1 and b"min_baseq should be 0..255" in err.value
    for opt in (2, 3, 1 << 31):
        assert call(opt=opt) == -1 and b"unknown option bit" in err.value
    assert call() == -1 and b"cannot open the reference FASTA" in err.value
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    assert call(d=bed) == -1 and b"cannot open the BED file" in err.value
    (tmp_path / "t.bed").write_text("c0\t1\t2\n")
    for opt in (0, 1):
        assert call(d=bed, opt=opt) == -1 and b"cannot open the BAM file" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert call() == -1 and err.value == b"gce_bam_error_profile reads BAM, not SAM text"
    with pytest.raises(capi.GceError) as ei:
        bamio.error_profile_bam(tmp_path / "in.bam", tmp_path / "ref.fa", bed=tmp_path / "t.bed", tsv=tmp_path / "out.tsv", direct=True)
    assert ei.value.status == -1 and "gce_bam_error_profile reads BAM, not SAM text" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa", "t.bed"]
    lib.gce_errprof_free(None)
    lib.gce_errprof_free(C.byref(run))
    sig = inspect.signature(bamio.error_profile_bam)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("bed", None), ("tsv", None), ("device", 0), ("threads", 0), ("min_mapq", 0), ("min_baseq", 0),
                                                                          ("exclude_flags", 0x704), ("direct", False), ("window_bytes", 0), ("device_budget_bytes", 0)]


def test_plane_constants_are_checked_against_the_lds():
    src = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_errprof.hpp")).read()
    cyc, cls, planes = (int(re.search(r"#define %s (\d+)u" % n, src).group(1)) for n in ("EP_CYC", "EP_CLS", "EP_PLANES"))
    assert planes * 3 * cyc * cls * 4 <= (160 << 10) // 2 and cls == 21 and cls % 2 == 1 and 1 <= cyc <= 1024
    assert "static_assert(EP_PLANES * EP_PLANE * 4u <= EP_LDS_PER_CU / EP_BLOCKS_PER_CU" in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4j" in design and "EP_CYC" in design and "cannot wrap" in design


def test_help_names_the_flags():
    from gencore_amd.cli import EPILOG, build_parser
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--error_profile FILE \[gencore_amd\]", h) and re.search(r"--error_profile_in FILE \[gencore_amd\]", h)
    assert re.search(r"--error_profile_min_mapq ERROR_PROFILE_MIN_MAPQ \[gencore_amd\]", h) and re.search(r"--error_profile_min_baseq ERROR_PROFILE_MIN_BASEQ \[gencore_amd\]", h)
    assert h.count("Restricted to the -b targets when -b is given") == 2
    assert "--error_profile FILE and --error_profile_in FILE" in EPILOG and "0x704" in EPILOG and "Hard clips" in EPILOG and "read group" in EPILOG
    o = build_parser().parse_args(["-r", "x"])
    assert (o.error_profile, o.error_profile_in, o.error_profile_min_mapq, o.error_profile_min_baseq) == (None, None, 0, 0)


@pytest.mark.parametrize("argv, words", [
    (["-i", "{bam}", "-r", "{fa}", "--error_profile", "{dir}/a.tsv"], "--error_profile needs an output file, not STDOUT"),
    (["-i", "{bam}", "-o", "{dir}/out.sam", "-r", "{fa}", "--error_profile", "{dir}/a.tsv"], "--error_profile needs BAM output, not SAM text"),
    (["-o", "{dir}/out.bam", "-r", "{fa}", "--error_profile_in", "{dir}/b.tsv"], "--error_profile_in needs an input file, not STDIN"),
    (["-i", "{sam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--error_profile_in", "{dir}/b.tsv"], "--error_profile_in needs BAM input, not SAM text"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--error_profile", "{dir}/a.tsv", "--error_profile_min_mapq", "256"], "error_profile_min_mapq should be 0..255"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "-b", "{bed}", "--error_profile_in", "{dir}/b.tsv", "--error_profile_min_baseq", "-1"],
     "error_profile_min_baseq should be 0..255"),
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


def test_validation_without_bed_and_under_sort_sam(tmp_path):
    """neither flag needs -b; --error_profile_in reads the sorted temporary BAM under --sort_sam, so SAM text input is no usage error there"""
    from gencore_amd.cli import build_parser, validate
    sam, bam, fa = tmp_path / "in.sam", tmp_path / "in.bam", tmp_path / "ref.fa"
    sam.write_text("@HD\tVN:1.6\n")
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    o = build_parser().parse_args(["-i", str(sam), "-o", str(tmp_path / "out.bam"), "-r", str(fa), "--sort_sam", "--error_profile_in", str(tmp_path / "b.tsv")])
    assert validate(o) == [0]
    o = build_parser().parse_args(["-i", str(bam), "-o", str(tmp_path / "out.bam"), "-r", str(fa), "--error_profile_in", str(tmp_path / "b.tsv"), "--error_profile",
                                   str(tmp_path / "a.tsv"), "--devices", "2,0"])
    assert validate(o) == [2, 0]


def test_flag_ordering(monkeypatch, tmp_path, capsys):
    """--error_profile_in runs behind --sort, --calmd_in, --umi_from and --pileup_in and in front of the run, on the file they made;
    --error_profile behind --calmd and --pileup and in front of --index; both on the first device, within --device_memory, with -b as BED"""
    from gencore_amd import bamio, cli, report
    calls = []

    class R:
        def __getattr__(self, k):
            return 0

    def note(name, ret=None):
        def f(*a, **kw):
            calls.append((name, a, kw))
            return ret if ret is not None else R()
        return f
    for n in ("sort_bam_passes", "calmd_bam_stream", "umi_to_mi", "pileup_bam", "error_profile_bam", "index_bam"):
        monkeypatch.setattr(bamio, n, note(n))
    monkeypatch.setattr(bamio, "load_bed", note("load_bed", []))
    depth = {"pre": None, "post": None}
    monkeypatch.setattr(bamio, "run_bam_passes", note("run", (None, depth, None)))
    monkeypatch.setattr(report, "read_header", lambda p: (["c0"], [4]))
    monkeypatch.setattr(report, "summary", lambda *a: "")
    monkeypatch.setattr(report, "write_json", note("json"))
    monkeypatch.setattr(os, "replace", lambda a, b: None)
    bam, fa, bed = tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "t.bed"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    bed.write_text("c0\t1\t2\n")
    out = tmp_path / "out.bam"
    rc = cli.main(["-i", str(bam), "-o", str(out), "-r", str(fa), "-b", str(bed), "-j", str(tmp_path / "r.json"), "--sort", "--calmd_in", "--umi_from", "RX", "--pileup_in",
                   str(tmp_path / "pi.tsv"), "--error_profile_in", str(tmp_path / "ei.tsv"), "--calmd", "--pileup", str(tmp_path / "p.tsv"), "--error_profile", str(tmp_path / "e.tsv"),
                   "--index", "--devices", "3", "--device_memory", "1", "--error_profile_min_mapq", "7", "--error_profile_min_baseq", "9"])
    errtext = capsys.readouterr().err
    assert rc == 0, errtext
    assert [c[0] for c in calls] == ["sort_bam_passes", "calmd_bam_stream", "umi_to_mi", "pileup_bam", "error_profile_bam", "load_bed", "run", "json", "calmd_bam_stream", "pileup_bam",
                                     "error_profile_bam", "index_bam"]
    first, second = [c for c in calls if c[0] == "error_profile_bam"]
    umi_tmp = calls[2][1][1]
    assert first[1] == (umi_tmp, str(fa)) and os.path.basename(umi_tmp).startswith("gencore_umi_") and second[1] == (str(out), str(fa))
    for c, tsv in ((first, "ei.tsv"), (second, "e.tsv")):
        assert c[2] == dict(bed=str(bed), tsv=str(tmp_path / tsv), device=3, threads=0, min_mapq=7, min_baseq=9, exclude_flags=0x704, device_budget_bytes=1 << 30)
    assert "error_profile_in: 0 records, 0 eligible, 0 bases, 0 mismatches\n" in errtext and "error_profile: 0 records, 0 eligible, 0 bases, 0 mismatches\n" in errtext


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """errprof_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("errprofhost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "errprof_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "errprof_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, refs, lens, regions, min_mapq, min_baseq, exclude):
    (d / "ref").write_text("".join("%s\n" % ("-" if r is None else r) for r in refs))
    (d / "intervals").write_text("".join("%d %d %d %d\n" % x for x in pypileup.intervals(regions, lens)[0]) if regions is not None else "")
    (d / "frames").write_bytes(ec.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(len(lens)), str(min_mapq), str(min_baseq), str(exclude), str(d / "ref"), "-" if regions is None else str(d / "intervals"),
                        str(d / "frames"), str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    rows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    return rows, np.frombuffer((d / "out").read_bytes(), np.uint64).reshape(3, pyerrprof.MAX_CYCLE, pyerrprof.ROW).tolist()


def test_record_functions_on_the_host(host_check):
    """errprof::scan_record and errprof::count_record on the host, under -fsanitize=address,undefined, with one lane and with 16 lanes: the
    skip of every record and every counter equal the model's and the hand-written numbers, over all of errprofcases"""
    d, exe = host_check
    order = [None] + pyerrprof.SKIPS
    for cs in ec.all_cases():
        rows, counts = host_run(d, exe, cs["records"], ec.refs(), ec.LENS, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        res = run_model(cs)
        assert counts == res["counts"], cs["label"]
        assert pyerrprof.nonzero(dict(counts=counts)) == ec.expected(cs), cs["label"]
        assert len(rows) == len(cs["records"])
        for k, r in enumerate(cs["records"]):
            assert rows[k][1] == 0 and order[rows[k][2]] == pyerrprof.skip_of(pyerrprof.fields(r), ec.refs(), cs["min_mapq"], cs["exclude"]), (cs["label"], k)
    # the malformed records: refused, nothing read beyond their block, nothing added
    recs = [b for _, b in ec.malformed()] + [b"\x05\0\0\0abcde", b"\x40\0\0\0" + bytes(40), b"\x01\0"]
    rows, counts = host_run(d, exe, recs, ec.refs(), ec.LENS, None, 0, 0, 0x704)
    assert [r[1:4] for r in rows] == [[1, 0, -1]] * len(recs) and not any(any(row) for seg in counts for row in seg)


def test_one_long_stream_on_the_host(host_check):
    """every hand case's records in one stream, the generated reads of the balance test and long ops over many intervals: 16 lanes against the
    model, without a BED and with one that cuts through the records"""
    d, exe = host_check
    recs = [r for cs in ec.all_cases() for r in cs["records"]] + balance_records(5, 40)
    recs += [ec.rec(0, 0, "40M20D5I30M", "ACGT" * 18 + "ACG", flag=0x50), ec.rec(0, 3, "17M60N17M", "ACGTN" * 6 + "ACGT", [k % 41 for k in range(34)], flag=0x80),
             ec.rec(1, 0, "50M", "GATTACA" * 7 + "G"), ec.rec(1, 10, "300S30M694S", "ACGT" * 256, flag=16)]
    regions = [(0, a, a + w) for a, w in ((0, 1), (2, 3), (9, 2), (12, 1), (14, 5), (30, 17), (48, 1), (60, 25), (99, 5))] + [(1, 0, 50), (1, 10, 20)]
    for reg in (None, regions):
        for mq, bq in ((0, 0), (10, 20)):
            rows, counts = host_run(d, exe, recs, ec.refs(), ec.LENS, reg, mq, bq, 0x704)
            res = pyerrprof.profile(recs, ec.refs(), ec.LENS, reg, mq, bq, 0x704)
            assert counts == res["counts"] and res["n_bases"] >= 100
            assert sum(1 for r in rows if r[2] == 0) == res["n_eligible"]


@pytest.fixture(scope="module")
def pileup_host_check(tmp_path_factory):
    """pileup_host_check, as tests/test_pileup_model.py builds it"""
    d = tmp_path_factory.mktemp("pileuphost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "pileup_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "pileup_host_check.hip"), "-o", exe])
    return d, exe


def test_both_scans_apply_one_rule_e(host_check, pileup_host_check):
    """pileup::scan_record and errprof::scan_record on the same records with the same thresholds: the same bad flag and the same skip code 1..6
    for every record.  The records are every one of pileupcases' and errprofcases' cases and both malformed() lists, of at most 1024 bases, on
    a reference that has every contig, so that the error profile's own skips (7 and 8) stay out of it.  Both go through reduce::rule_e
    (gce_reduce.hpp): this holds by construction, and pins that it stays so."""
    d, exe = host_check
    pd, pexe = pileup_host_check
    recs = [r for cs in pc.all_cases() + ec.all_cases() for r in cs["records"]] + [b for _, b in pc.malformed() + ec.malformed()]
    recs = [r for r in recs if len(r) < 24 or int.from_bytes(r[20:24], "little", signed=True) <= pyerrprof.MAX_CYCLE]
    refs = [ec.FASTA.get(nm, "ACGT" * 8) for nm in ec.NAMES]
    assert all(refs) and len(recs) > 100
    seen = set()
    for mq, excl in ((0, 0x704), (10, 0x704), (1, 0x10)):
        rows, _ = host_run(d, exe, recs, refs, ec.LENS, None, mq, 0, excl)
        (pd / "intervals").write_text("".join("%d %d %d %d\n" % x for x in pypileup.intervals([(0, 10, 12)], ec.LENS)[0]))
        (pd / "frames").write_bytes(pc.frames(recs))
        r = subprocess.run(["timeout", "-k", "10", "300", pexe, str(len(ec.LENS)), str(mq), "0", str(excl), str(pd / "intervals"), str(pd / "frames"), str(pd / "out")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
        prows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(rows) == len(prows) == len(recs)
        for k in range(len(recs)):
            assert rows[k][1:3] == prows[k][1:3] and 0 <= rows[k][2] <= 6 and rows[k][1] in (0, 1), (mq, excl, k, rows[k], prows[k])
        seen |= {(r[1], r[2]) for r in rows}
    assert seen == {(1, 0)} | {(0, k) for k in range(7)}                              # malformed, eligible and each of rule E's six skips occur
