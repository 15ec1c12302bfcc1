"""The error profile by reported base quality without a GPU: the model (tests/pyerrqual.py) against the records written out by
hand (tests/qualcases.py); the bucket of every byte; the model's invariant against pyerrprof and pyerrmask; the table's text; the bucket, the
column functor and the count walk of the kernels compiled for the host under the address and undefined-behaviour sanitizers, every record in a
heap block of its exact size; the symbols, prototypes, struct size and argument checks of the entry points; the command line's help and
refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import errprofcases as ec
import maskcases as mc
import pyerrmask
import pyerrprof
import pyerrqual
import pypileup
import qualcases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = ec.refs()


def model_mask(cs):
    return None if cs["mask"] is None else pyerrmask.merge(qc.mask_of(cs), mc.CLAMP)


def run_model(cs):
    return pyerrqual.profile(cs["records"], REFS, ec.LENS, model_mask(cs), ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])


def test_model_against_hand_cases():
    labels = [c["label"] for c in qc.all_cases()]
    assert len(set(labels)) == len(labels) >= 11
    for cs in qc.all_cases():
        res = run_model(cs)
        assert pyerrqual.nonzero(res) == qc.expected(cs), cs["label"]
        assert {k: res[k] for k in pyerrqual.SKIPS} == cs["skips"], cs["label"]
        assert res["n_eligible"] == res["n_records"] == len(cs["records"])
        assert all(row[22] == 0 and row[23] == 0 for seg in res["counts"] for row in seg)
        assert res["n_bases"] == sum(n for (g, b, cl), n in qc.expected(cs).items() if ">" in cl)
    assert np.array(res["counts"]).shape == (3, 96, 24) and 3 * 96 * 24 * 8 == 55296


def test_bucket_of_every_byte():
    assert [pyerrqual.bucket(b) for b in range(256)] == list(range(94)) + [94] * 162
    assert [pyerrqual.label(b) for b in (0, 37, 93, 94, 95)] == ["0", "37", "93", "94+", "."]
    assert (pyerrqual.BUCKETS, pyerrqual.TOP, pyerrqual.NOQ) == (96, 94, 95)


def streams():
    """errprofcases' and maskcases' records (those under the default thresholds), the hand cases of this pass, and random records with binned
    qualities, any byte and none"""
    hand = [r for cs in ec.all_cases() + mc.record_cases() if cs["min_mapq"] == 0 and cs["label"] not in ("l_seq_1024", "l_seq_1025") for r in cs["records"]]
    return hand + [r for cs in qc.all_cases() for r in cs["records"]] + qc.random_records(11, 200)


def test_model_invariant():
    """summed over the buckets the quality table is the cycle table summed over cycles, per segment and class, without and with a BED, without
    and with a mask; every counter in front of the tables is equal"""
    recs = streams()
    mask = pyerrmask.merge([(t, x, x + 1) for t, ln in enumerate(mc.CLAMP) for x in range(max(ln, 0)) if x % 7 == 2], mc.CLAMP)
    for regions in (None, [(0, 3, 20), (1, 10, 30)]):
        for m in (None, mask):
            got = pyerrqual.profile(recs, REFS, ec.LENS, m, regions, 5, 13)
            want = pyerrprof.profile(recs, REFS, ec.LENS, regions, 5, 13) if m is None else pyerrmask.profile(recs, REFS, ec.LENS, m, regions, 5, 13)
            assert pyerrqual.by_class(got) == [[sum(row[c] for row in seg) for c in range(22)] for seg in want["counts"]]
            assert all(got[k] == want[k] for k in ["n_records", "n_eligible", "n_bases", "n_mismatches", "n_intervals"] + pyerrprof.SKIPS)
            rows = {b for g, b, cl in pyerrqual.nonzero(got)}
            assert got["n_eligible"] > 100 and {2, 11, 25, 37, 94, 95} <= rows and len(rows) > 40
            assert sum(row[pyerrprof.LOWQ] for seg in got["counts"] for row in seg[13:95]) == 0 and sum(row[pyerrprof.LOWQ] for seg in got["counts"] for row in seg[:13]) > 0
            assert sum(row[pyerrprof.LOWQ] for seg in got["counts"] for row in seg[95:]) == 0
        assert got["n_masked_events"] == want["n_masked_events"] > 0


def test_table_text():
    cs = [c for c in qc.all_cases() if c["label"] == "byte_edges"][0]
    z = lambda n: "\t0" * n
    want = (pyerrqual.HEADER + "0\t0\t1\t0\t1" + z(20) + "\n" + "0\t1\t1\t0" + z(5) + "\t1" + z(15) + "\n" + "0\t93\t1\t0" + z(10) + "\t1" + z(10) + "\n"
            + "0\t94+\t3\t0\t1" + z(4) + "\t1" + z(9) + "\t1" + z(5) + "\n")
    assert pyerrqual.table(run_model(cs)) == want.encode()
    cs = [c for c in qc.all_cases() if c["label"] == "no_qualities"][0]
    assert pyerrqual.table(run_model(cs)).split(b"\n")[1].startswith(b"0\t.\t8\t0\t3\t")
    cs = [c for c in qc.all_cases() if c["label"] == "masked_column_and_insertion"][0]
    lines = pyerrqual.table(run_model(cs), True).split(b"\n")
    assert lines[0].endswith(b"\tDEL\tMASKED") and lines[2] == ("0\t31\t0\t0" + z(21) + "\t1").encode() and len(lines) == 6
    assert pyerrqual.HEADER.startswith("#segment\tquality\tbases\tmismatches\tA>A\t") and pyerrqual.HEADER.endswith("\tT>T\tREAD_N\tREF_OTHER\tLOWQ\tINS\tDEL\n")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """errqual_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("errqualhost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "errqual_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "errqual_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, refs, lens, regions, mask, min_mapq=0, min_baseq=0, exclude=0x704):
    (d / "ref").write_text("".join("%s\n" % ("-" if r is None else r) for r in refs))
    (d / "intervals").write_text("".join("%d %d %d %d\n" % x for x in pypileup.intervals(regions, lens)[0]) if regions is not None else "")
    (d / "mask").write_text("".join("%d %d %d\n" % x for x in mask or []))
    (d / "frames").write_bytes(ec.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(len(lens)), str(min_mapq), str(min_baseq), str(exclude), str(d / "ref"), "-" if regions is None else str(d / "intervals"),
                        "-" if mask is None else str(d / "mask"), str(d / "frames"), str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    counts = np.frombuffer((d / "out").read_bytes(), np.uint64).reshape(3, 96, 24).tolist()
    return [int(x) for x in r.stdout.splitlines()[-1].split()[1:]], counts


def same_as_model(head, counts, res):
    assert counts == res["counts"]
    assert head == [res["n_records"]] + [res[k] for k in pyerrqual.SKIPS] + [res["n_eligible"]]


def test_record_functions_on_the_host(host_check):
    """errqual::bucket over all bytes and errqual::count_record on the host, under -fsanitize=address,undefined, with one lane and with 16,
    every record in a heap block of its exact size: every counter equals the model's and the hand-written numbers"""
    d, exe = host_check
    for cs in qc.all_cases():
        head, counts = host_run(d, exe, cs["records"], REFS, ec.LENS, ec.regions_of(cs), model_mask(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        same_as_model(head, counts, run_model(cs))
        assert pyerrqual.nonzero(dict(counts=counts)) == qc.expected(cs), cs["label"]


def test_streams_on_the_host(host_check):
    """the random streams, without and with a BED and a mask: 1 and 16 lanes against the model"""
    d, exe = host_check
    recs = streams()
    mask = pyerrmask.merge([(t, x, x + 1) for t, ln in enumerate(mc.CLAMP) for x in range(max(ln, 0)) if x % 5 == 1], mc.CLAMP)
    for regions, m in ((None, None), ([(0, 3, 30), (1, 10, 30)], None), (None, mask), ([(0, 3, 30), (1, 10, 30)], mask)):
        head, counts = host_run(d, exe, recs, REFS, ec.LENS, regions, m, 5, 13)
        same_as_model(head, counts, pyerrqual.profile(recs, REFS, ec.LENS, m, regions, 5, 13))


def test_symbols_prototypes_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_error_profile_quality(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *mask_path /* NULL: no mask */, "
            "const char *tsv_path /* NULL: no file */, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, "
            "uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errqual_run *out, gce_mask_run *mask /* NULL without mask_path */, char err[256]);") in head
    assert "void gce_errqual_free(gce_errqual_run *out);" in head and "#define GCE_ERRQUAL_BUCKETS 96" in head and "#define GCE_ERRQUAL_DIRECT 1u" in head
    assert "GATK" in head and "QualityScoreDistribution" in head
    lib = capi.load_library()
    for n in ("gce_bam_error_profile_quality", "gce_errqual_free"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n)
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_errqual_create", "gce_errqual_set_ref", "gce_errqual_set_mask", "gce_errqual_set_sites", "gce_errqual_window", "gce_errqual_finish", "gce_errqual_destroy", "gce_errqual_error"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS and len(re.findall(r"\b%s\(" % n, entry)) == 1, n
    assert "bamio_errqual.hpp" in open(os.path.join(ROOT, "gencore_amd", "csrc", "bamio.cpp")).read()
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %d\\n",sizeof(gce_errqual_run),offsetof(gce_errqual_run,n_bases),'
                     'offsetof(gce_errqual_run,counts),GCE_ERRQUAL_BUCKETS);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GceErrqualRun), capi.GceErrqualRun.n_bases.offset, capi.GceErrqualRun.counts.offset,
                                                                                          capi.GCE_ERRQUAL_BUCKETS]
    names = [n for n, _ in capi.GceErrqualRun._fields_]
    assert names[:10] == ["n_records", "n_eligible"] + pyerrqual.SKIPS and names[10:14] == ["n_bases", "n_mismatches", "n_intervals", "peak_device_bytes"]
    assert names[14:] == ["read_s", "inflate_index_s", "errprof_s", "write_s", "total_s", "counts"]
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the session's argument checks that come before any device is touched
    vp = C.c_void_p
    lib.gce_errqual_create.argtypes = [C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    p = vp()
    assert lib.gce_errqual_create(0, 0, 0, 0, 0x704, 0, None) == -1
    assert lib.gce_errqual_create(0, 0, 0, 0, 0x704, 2, C.byref(p)) == -1 and not p.value
    for f, args in ((lib.gce_errqual_set_ref, (None, 0, None, None)), (lib.gce_errqual_set_mask, (None, C.c_int64(0), None, None, None)), (lib.gce_errqual_set_sites, (None, C.c_int64(-1), None, None, None)),
                    (lib.gce_errqual_finish, (None, None, None)), (lib.gce_errqual_window, (None, None, 0, 0, None, None, None, C.c_uint64(0), 0, 1, None))):
        assert f(*args) == -1
    lib.gce_errqual_error.restype = C.c_char_p
    assert lib.gce_errqual_error(None) == b"" and lib.gce_errqual_destroy(None) is not None
    # the runner's
    run, mrun, err = capi.GceErrqualRun(), capi.GceMaskRun(), (C.c_char * 256)()
    bam, fa, vcf, tsv = (str(tmp_path / n).encode() for n in ("in.bam", "ref.fa", "m.vcf", "out.tsv"))
    call = lambda b=bam, f=fa, m=None, mr=None, opt=0, out=C.byref(run), mapq=0, baseq=0: lib.gce_bam_error_profile_quality(b, f, None, m, tsv, 0, 1, mapq, baseq, 0x704, opt, 0, 0, out, mr, err)
    assert call(b=None) == -1 and err.value == b"bad argument" and call(f=None) == -1 and call(out=None) == -1 and call(m=vcf) == -1 and err.value == b"bad argument"
    assert call(opt=2) == -1 and b"unknown option bit (GCE_ERRQUAL_DIRECT is the only one)" in err.value
    assert call(mapq=256) == -1 and err.value == b"min_mapq should be 0..255" and call(baseq=-1) == -1 and err.value == b"min_baseq should be 0..255"
    assert call() == -1 and b"cannot open the reference FASTA" in err.value
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    assert call(m=vcf, mr=C.byref(mrun)) == -1 and err.value == b"cannot open the variant mask"
    assert call(m=fa, mr=C.byref(mrun)) == -1 and err.value == pyerrmask.NAME_REFUSAL.encode()
    assert call() == -1 and b"cannot open the BAM file" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert call() == -1 and err.value == b"gce_bam_error_profile_quality reads BAM, not SAM text"
    with pytest.raises(capi.GceError) as ei:
        bamio.error_profile_quality_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tsv=tmp_path / "out.tsv", direct=True)
    assert ei.value.status == -1 and "reads BAM, not SAM text" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]


def test_help_and_flag_validation(tmp_path, capsys):
    from gencore_amd.cli import EPILOG, build_parser, main
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--error_profile_quality FILE \[gencore_amd\]", h) and re.search(r"--error_profile_quality_in FILE \[gencore_amd\]", h)
    assert "the qualities the consensus step wrote" in h and "the sequencer's qualities" in h and h.count("--error_profile_fragments does not apply to it") == 2
    assert "--error_profile_quality FILE and --error_profile_quality_in FILE" in EPILOG and "94+" in EPILOG and "--error_profile_fragments does not apply to them" in EPILOG
    o = build_parser().parse_args(["-r", "x"])
    assert o.error_profile_quality is None and o.error_profile_quality_in is None
    bam, sam, fa, vcf = tmp_path / "in.bam", tmp_path / "in.sam", tmp_path / "ref.fa", tmp_path / "m.vcf"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    sam.write_text("@HD\tVN:1.6\n")
    fa.write_text(">c0\nACGT\n")
    vcf.write_bytes(mc.vcf(("c0", 1, "A", "C")))
    base = ["-i", str(bam), "-r", str(fa)]
    q, qin = ["--error_profile_quality", str(tmp_path / "q.tsv")], ["--error_profile_quality_in", str(tmp_path / "qi.tsv")]
    for argv, words in ((base + ["-o", "-"] + q, "--error_profile_quality needs an output file, not STDOUT"),
                        (base + ["-o", str(tmp_path / "out.sam")] + q, "--error_profile_quality needs BAM output, not SAM text"),
                        (["-r", str(fa), "-o", str(tmp_path / "out.bam")] + qin, "--error_profile_quality_in needs an input file, not STDIN"),
                        (["-i", str(sam), "-r", str(fa), "-o", str(tmp_path / "out.bam")] + qin, "--error_profile_quality_in needs BAM input, not SAM text"),
                        (base + ["-o", str(tmp_path / "out.bam"), "--error_profile_mask", str(tmp_path / "none.vcf")] + q, "none.vcf' doesn't exist"),
                        (base + ["-o", str(tmp_path / "out.bam"), "--error_profile_mask", str(fa)] + qin, "--error_profile_mask needs a .vcf, .vcf.gz or .bed file"),
                        (base + ["-o", str(tmp_path / "out.bam"), "--error_profile_min_baseq", "256"] + q, "error_profile_min_baseq should be 0..255"),
                        (base + ["-o", str(tmp_path / "out.bam"), "--error_profile_fragments"] + q, "--error_profile_fragments needs --error_profile or --error_profile_in")):
        assert main(argv) == 255
        assert words in capsys.readouterr().err
    # a missing -r is argparse's refusal as for every table
    with pytest.raises(SystemExit):
        main(["-i", str(bam), "-o", str(tmp_path / "out.bam")] + q)
    assert "-r" in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "in.sam", "m.vcf", "ref.fa"]
