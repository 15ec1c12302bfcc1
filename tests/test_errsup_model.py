"""The error profile by consensus support without a GPU: the model (tests/pyerrsup.py) against the records written out by hand
(tests/supcases.py); the model's invariant against pyerrprof and pyerrmask; the tag walk, the scan and the count walk of the kernels compiled
for the host under the address and undefined-behaviour sanitizers, every record in a heap block of its exact size; the symbols, prototypes,
struct size and argument checks of the entry points; the command line's help and refusals."""
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
import pyerrsup
import pypileup
import supcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = ec.refs()


def model_mask(cs):
    return None if cs["mask"] is None else pyerrmask.merge(sc.mask_of(cs), mc.CLAMP)


def run_model(cs):
    return pyerrsup.profile(cs["records"], REFS, ec.LENS, model_mask(cs), ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"], cs["tags"])


def test_model_against_hand_cases():
    labels = [c["label"] for c in sc.all_cases()]
    assert len(set(labels)) == len(labels) >= 17
    for cs in sc.all_cases():
        res = run_model(cs)
        assert pyerrsup.nonzero(res) == sc.expected(cs), cs["label"]
        assert {k: res[k] for k in pyerrsup.SKIPS} == cs["skips"], cs["label"]
        assert res["n_eligible"] == len(cs["records"]) - sum(cs["skips"].values()) and res["n_records"] == len(cs["records"])
        assert all(row[23] == 0 for seg in res["counts"] for fr in seg for row in fr)
        exp = sc.expected(cs)
        assert res["n_with_forward"] == sum(n for (g, f, r, cl), n in exp.items() if cl == "RECORDS" and f)
        assert res["n_with_reverse"] == sum(n for (g, f, r, cl), n in exp.items() if cl == "RECORDS" and r)
        assert res["n_bases"] == sum(n for (g, f, r, cl), n in exp.items() if ">" in cl)
    assert np.array(res["counts"]).shape == (3, 33, 33, 24) and 3 * 33 * 33 * 24 * 8 == 627264


def test_support_buckets_and_refused_walks():
    """rule U on single records: every integer type's sign, the edges of the buckets, and each refusal of the walk"""
    for typ, v, want in (("c", -1, 32), ("c", 127, 32), ("C", 255, 32), ("s", -32768, 32), ("S", 65535, 32), ("i", -1, 32), ("I", 2 ** 32 - 1, 32), ("C", 0, 32), ("C", 1, 1), ("i", 31, 31),
                         ("S", 32, 32), ("I", 33, 32)):
        assert pyerrsup.support(sc.ac(sc.num("FR", typ, v) + sc.num("RR", typ, v))) == (want, want, False), (typ, v)
    assert pyerrsup.support(sc.ac()) == (0, 0, False)
    assert pyerrsup.support(sc.ac(sc.num("RR", "C", 3) + b"XY")) == (0, 3, True)
    assert pyerrsup.support(sc.ac(sc.num("FR", "C", 3)), ("RR", "FR")) == (0, 3, False)
    assert [pyerrsup.label(b) for b in (0, 1, 31, 32)] == [".", "1", "31", "32+"]


def streams():
    """errprofcases' and maskcases' records (those under the default thresholds) with random tags behind them, and random records"""
    hand = [r for cs in ec.all_cases() + mc.record_cases() if cs["min_mapq"] == 0 and cs["label"] not in ("l_seq_1024", "l_seq_1025") for r in cs["records"]]
    return sc.with_tags(hand, 3) + sc.random_records(11, 160)


def test_model_invariant():
    """summed over (forward, reverse) the support table is the cycle table summed over cycles, per segment and class, without and with a
    BED, without and with a mask; the first nine counters are equal and no record has a broken optional area"""
    recs = streams()
    mask = pyerrmask.merge([(t, x, x + 1) for t, ln in enumerate(mc.CLAMP) for x in range(max(ln, 0)) if x % 7 == 2], mc.CLAMP)
    for regions in (None, [(0, 3, 20), (1, 10, 30)]):
        for m in (None, mask):
            got = pyerrsup.profile(recs, REFS, ec.LENS, m, regions, 5, 13)
            want = pyerrprof.profile(recs, REFS, ec.LENS, regions, 5, 13) if m is None else pyerrmask.profile(recs, REFS, ec.LENS, m, regions, 5, 13)
            assert pyerrsup.by_class(got) == [[sum(row[c] for row in seg) for c in range(22)] for seg in want["counts"]]
            assert all(got[k] == want[k] for k in ["n_records", "n_eligible", "n_bases", "n_mismatches"] + pyerrprof.SKIPS) and got["n_bad_aux"] == 0
            assert got["n_eligible"] > 100 and 0 < got["n_with_reverse"] < got["n_with_forward"] < got["n_eligible"]
            assert len({(f, r) for g, f, r, cl in pyerrsup.nonzero(got)}) > 15
            if regions is None:
                assert sum(row[22] for seg in got["counts"] for fr in seg for row in fr) == got["n_eligible"]
        assert got["n_masked_events"] == want["n_masked_events"] > 0


def test_table_text():
    cs = [c for c in sc.all_cases() if c["label"] == "bed_and_records"][0]
    zeros = "\t0" * 21
    assert pyerrsup.table(run_model(cs)) == (pyerrsup.HEADER + "0\t3\t.\t1\t2\t0" + "\t0" * 10 + "\t1" + "\t0" * 4 + "\t1" + "\t0" * 5 + "\n" + "0\t5\t.\t1\t0\t0" + zeros + "\n").encode()
    cs = [c for c in sc.all_cases() if c["label"] == "zero_is_the_top_bucket"][0]
    assert pyerrsup.table(run_model(cs), True).split(b"\n")[1].startswith(b"0\t32+\t32+\t1\t2\t0\t1\t") and pyerrsup.HEADER_MASKED.endswith("\tDEL\tMASKED\n")
    assert pyerrsup.HEADER.startswith("#segment\tforward\treverse\trecords\tbases\tmismatches\tA>A\t") and pyerrsup.HEADER.endswith("\tT>T\tREAD_N\tREF_OTHER\tLOWQ\tINS\tDEL\n")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """errsup_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("errsuphost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "errsup_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "errsup_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, refs, lens, regions, mask, tags=("FR", "RR"), min_mapq=0, min_baseq=0, exclude=0x704):
    (d / "ref").write_text("".join("%s\n" % ("-" if r is None else r) for r in refs))
    (d / "intervals").write_text("".join("%d %d %d %d\n" % x for x in pypileup.intervals(regions, lens)[0]) if regions is not None else "")
    (d / "mask").write_text("".join("%d %d %d\n" % x for x in mask or []))
    (d / "frames").write_bytes(ec.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(len(lens)), str(min_mapq), str(min_baseq), str(exclude), tags[0] + tags[1], str(d / "ref"),
                        "-" if regions is None else str(d / "intervals"), "-" if mask is None else str(d / "mask"), str(d / "frames"), str(d / "out")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    counts = np.frombuffer((d / "out").read_bytes(), np.uint64).reshape(3, 33, 33, 24).tolist()
    return [int(x) for x in r.stdout.splitlines()[-1].split()[1:]], counts


def same_as_model(head, counts, res):
    assert counts == res["counts"]
    assert head == [res["n_records"]] + [res[k] for k in pyerrsup.SKIPS] + [res["n_eligible"]]


def test_record_functions_on_the_host(host_check):
    """errsup::support, scan_record and count_record on the host, under -fsanitize=address,undefined, with one lane and with 16, every record
    in a heap block of its exact size: every counter equals the model's and the hand-written numbers"""
    d, exe = host_check
    for cs in sc.all_cases():
        head, counts = host_run(d, exe, cs["records"], REFS, ec.LENS, ec.regions_of(cs), model_mask(cs), cs["tags"], cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        same_as_model(head, counts, run_model(cs))
        assert pyerrsup.nonzero(dict(counts=counts)) == sc.expected(cs), cs["label"]


def test_streams_on_the_host(host_check):
    """the random streams, without and with a BED and a mask, and with the tags swapped: 16 lanes against the model"""
    d, exe = host_check
    recs = streams()
    mask = pyerrmask.merge([(t, x, x + 1) for t, ln in enumerate(mc.CLAMP) for x in range(max(ln, 0)) if x % 5 == 1], mc.CLAMP)
    for regions, m, tags in ((None, None, ("FR", "RR")), ([(0, 3, 30), (1, 10, 30)], None, ("FR", "RR")), (None, mask, ("RR", "FR")), ([(0, 3, 30), (1, 10, 30)], mask, ("FR", "RR"))):
        head, counts = host_run(d, exe, recs, REFS, ec.LENS, regions, m, tags, 5, 13)
        same_as_model(head, counts, pyerrsup.profile(recs, REFS, ec.LENS, m, regions, 5, 13, tags=tags))
    broken = [r for cs in sc.all_cases() if cs["label"].startswith("bad_aux") for r in cs["records"]]
    head, counts = host_run(d, exe, broken + recs[:20], REFS, ec.LENS, None, None)
    same_as_model(head, counts, pyerrsup.profile(broken + recs[:20], REFS, ec.LENS))
    assert head[9] == 11


def test_symbols_prototypes_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_error_profile_support(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *mask_path /* NULL: no mask */, "
            "const char *tsv_path /* NULL: no file */, const char *tags /* NULL: \"FRRR\" */, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, "
            "uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errsup_run *out, gce_mask_run *mask /* NULL without mask_path */, char err[256]);") in head
    assert "void gce_errsup_free(gce_errsup_run *out);" in head and "#define GCE_ERRSUP_BUCKETS 33" in head and "#define GCE_ERRSUP_DIRECT 1u" in head
    lib = capi.load_library()
    for n in ("gce_bam_error_profile_support", "gce_errsup_free"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n)
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_errsup_create", "gce_errsup_set_ref", "gce_errsup_set_mask", "gce_errsup_set_sites", "gce_errsup_window", "gce_errsup_finish", "gce_errsup_destroy", "gce_errsup_error"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS and len(re.findall(r"\b%s\(" % n, entry)) == 1, n
    assert "bamio_errsup.hpp" in open(os.path.join(ROOT, "gencore_amd", "csrc", "bamio.cpp")).read()
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %d\\n",sizeof(gce_errsup_run),offsetof(gce_errsup_run,n_bad_aux),'
                     'offsetof(gce_errsup_run,counts),GCE_ERRSUP_BUCKETS);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GceErrsupRun), capi.GceErrsupRun.n_bad_aux.offset, capi.GceErrsupRun.counts.offset,
                                                                                          capi.GCE_ERRSUP_BUCKETS]
    names = [n for n, _ in capi.GceErrsupRun._fields_]
    assert names[:11] == ["n_records", "n_eligible"] + pyerrsup.SKIPS and names[11:13] == ["n_with_forward", "n_with_reverse"] and names[-1] == "counts"
    assert [n for n in names if n not in ("n_bad_aux", "n_with_forward", "n_with_reverse")] == [n for n, _ in capi.GceErrprofRun._fields_]
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the session's argument checks that come before any device is touched
    vp = C.c_void_p
    lib.gce_errsup_create.argtypes = [C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(vp)]
    p = vp()
    assert lib.gce_errsup_create(0, 0, 0, 0, 0x704, 0, b"FRRR", None) == -1
    assert lib.gce_errsup_create(0, 0, 0, 0, 0x704, 2, b"FRRR", C.byref(p)) == -1 and not p.value
    assert lib.gce_errsup_create(0, 0, 0, 0, 0x704, 0, b"FRR", C.byref(p)) == -1 and lib.gce_errsup_create(0, 0, 0, 0, 0x704, 0, b"FRRRR", C.byref(p)) == -1 and not p.value
    for f, args in ((lib.gce_errsup_set_ref, (None, 0, None, None)), (lib.gce_errsup_set_mask, (None, C.c_int64(0), None, None, None)), (lib.gce_errsup_set_sites, (None, C.c_int64(-1), None, None, None)),
                    (lib.gce_errsup_finish, (None, None, None))):
        assert f(*args) == -1
    lib.gce_errsup_error.restype = C.c_char_p
    assert lib.gce_errsup_error(None) == b"" and lib.gce_errsup_destroy(None) is not None
    # the runner's
    run, mrun, err = capi.GceErrsupRun(), capi.GceMaskRun(), (C.c_char * 256)()
    bam, fa, vcf, tsv = (str(tmp_path / n).encode() for n in ("in.bam", "ref.fa", "m.vcf", "out.tsv"))
    call = lambda b=bam, f=fa, m=None, mr=None, opt=0, tags=None, out=C.byref(run): lib.gce_bam_error_profile_support(b, f, None, m, tsv, tags, 0, 1, 0, 0, 0x704, opt, 0, 0, out, mr, err)
    assert call(b=None) == -1 and err.value == b"bad argument" and call(f=None) == -1 and call(out=None) == -1 and call(m=vcf) == -1 and err.value == b"bad argument"
    assert call(opt=2) == -1 and b"unknown option bit (GCE_ERRSUP_DIRECT is the only one)" in err.value
    for t in (b"", b"FR", b"FRR", b"FR,RR", b"F!RR", b"FR1R"):
        assert call(tags=t) == -1 and err.value == b"tags should be two two-character tags, four characters", t
    assert call() == -1 and b"cannot open the reference FASTA" in err.value
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    assert call(m=vcf, mr=C.byref(mrun)) == -1 and err.value == b"cannot open the variant mask"
    assert call(m=fa, mr=C.byref(mrun)) == -1 and err.value == pyerrmask.NAME_REFUSAL.encode()
    assert call(tags=b"aDbD") == -1 and b"cannot open the BAM file" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert call() == -1 and err.value == b"gce_bam_error_profile_support reads BAM, not SAM text"
    with pytest.raises(capi.GceError) as ei:
        bamio.error_profile_support_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tsv=tmp_path / "out.tsv", direct=True)
    assert ei.value.status == -1 and "reads BAM, not SAM text" in str(ei.value)
    for tags in ("FRRR", ("FR",), ("FR", "R"), ("FR", "RR", "XX"), (b"FR", b"RR")):
        with pytest.raises(ValueError):
            bamio.error_profile_support_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tags=tags)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]


def test_help_and_flag_validation(tmp_path, capsys):
    from gencore_amd.cli import EPILOG, build_parser, main
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--error_profile_support FILE \[gencore_amd\]", h) and re.search(r"--error_profile_support_tags A,B \[gencore_amd\]", h)
    assert "for choosing -s and --duplex_only from one run at -s 1" in h and "aD,bD" in h and "Default FR,RR." in h
    assert "--error_profile_support FILE" in EPILOG and "from ONE run at -s 1" in EPILOG and "32+" in EPILOG
    o = build_parser().parse_args(["-r", "x"])
    assert o.error_profile_support is None and o.error_profile_support_tags == "FR,RR"
    bam, fa, vcf = tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "m.vcf"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    vcf.write_bytes(mc.vcf(("c0", 1, "A", "C")))
    base = ["-i", str(bam), "-r", str(fa)]
    sup = ["--error_profile_support", str(tmp_path / "s.tsv")]
    for argv, words in ((base + ["-o", "-"] + sup, "--error_profile_support needs an output file, not STDOUT"),
                        (base + ["-o", str(tmp_path / "out.sam")] + sup, "--error_profile_support needs BAM output, not SAM text"),
                        (base + ["-o", str(tmp_path / "out.bam"), "--error_profile_support_tags", "aD,bD"], "--error_profile_support_tags needs --error_profile_support"),
                        (base + ["-o", str(tmp_path / "out.bam"), "--error_profile_mask", str(tmp_path / "none.vcf")] + sup, "none.vcf' doesn't exist")):
        assert main(argv) == 255
        assert words in capsys.readouterr().err
    for tags in ("FR", "FRRR", "FR,R", "FR,RR,XX", "F!,RR", "1R,RR", "FR;RR", ""):
        assert main(base + ["-o", str(tmp_path / "out.bam"), "--error_profile_support_tags", tags] + sup) == 255
        assert "--error_profile_support_tags needs two two-character tags, as in FR,RR" in capsys.readouterr().err
    # the mask is accepted with the support table alone, and a missing -r is argparse's refusal as for every table
    with pytest.raises(SystemExit):
        main(["-i", str(bam), "-o", str(tmp_path / "out.bam")] + sup)
    assert "-r" in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "m.vcf", "ref.fa"]
