"""gce_bam_umi_to_mi without a GPU: the symbol, its prototype and its argument checks, the flag of the command line, the model
of the rules (tests/pyumi.py) against records whose new bytes are written out by hand (tests/umicases.py), the per-record functions of the
kernels (gce_umi.hpp) compiled for the host under the address and undefined-behaviour sanitizers and compared with the model record by
record, and the premise of the end-to-end test: without its UMIs the stream gives the oracle fewer records."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pyumi
import umicases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_prototype_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert "typedef struct gce_umi_run { int64_t n_records, n_tagged, n_no_source, n_not_umi, n_mi_dropped;" in head
    assert re.search(r"int64_t n_flushes, inflated_bytes, out_record_bytes, out_bytes, peak_device_bytes;[^}]*double read_s, inflate_index_s, umi_s, write_s, total_s;[^}]*} gce_umi_run;", head)
    assert ("int gce_bam_umi_to_mi(const char *in_path, const char *out_path, const char *source, int32_t device, int threads, int level, uint64_t window_bytes, "
            "size_t device_budget_bytes, uint64_t resident_bytes, gce_umi_run *out, char err[256]);") in head
    assert "bamutil.cpp:23-38" in head[head.index("gce_bam_calmd_stream("):head.index("} gce_umi_run;")]
    lib = capi.load_library()
    assert "gce_bam_umi_to_mi" in capi.EXPORTED_SYMBOLS and hasattr(lib, "gce_bam_umi_to_mi")
    assert lib.gce_bam_umi_to_mi.argtypes == [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int, C.c_int, C.c_uint64, C.c_size_t, C.c_uint64, C.POINTER(capi.GceUmiRun), C.c_char_p]
    assert [n for n, _ in capi.GceUmiRun._fields_] == ["n_records", "n_tagged", "n_no_source", "n_not_umi", "n_mi_dropped", "n_flushes", "inflated_bytes", "out_record_bytes", "out_bytes",
                                                       "peak_device_bytes", "read_s", "inflate_index_s", "umi_s", "write_s", "total_s"]
    assert C.sizeof(capi.GceUmiRun) == 10 * 8 + 5 * 8
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "gencore_amd.h"\nint main(){printf("%zu\\n",sizeof(gce_umi_run));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert int(subprocess.check_output([str(tmp_path / "probe")])) == C.sizeof(capi.GceUmiRun)
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the argument checks come before any device is touched
    run, err = capi.GceUmiRun(), (C.c_char * 256)()
    a, b = str(tmp_path / "in.bam").encode(), str(tmp_path / "out.bam").encode()
    call = lambda i, o, s, lv=-2, r=C.byref(run): lib.gce_bam_umi_to_mi(i, o, s, 0, 1, lv, 0, 0, 0, r, err)
    assert call(None, b, b"RX") == -1 and call(a, None, b"RX") == -1 and call(a, b, None) == -1 and call(a, b, b"RX", r=None) == -1
    for level in (-4, 10):
        assert call(a, b, b"RX", level) == -1 and b"level" in err.value
    for bad in (b"", b"R", b"RXX", b"1X", b"R-", b"R ", b"_X", b"Name", b"NAME", b"names", b"\xc3\xa9"):
        assert call(a, b, bad) == -1 and b"two-character tag such as RX, or name" in err.value, bad
    assert call(a, b, b"MI") == -1 and b"MI is what the run reads" in err.value
    for good in (b"RX", b"name", b"r2", b"Mi", b"mI", b"BC"):                # accepted: the next check, the input, is what fails
        assert call(a, b, good) == -1 and b"cannot open the input BAM" in err.value, good
    with pytest.raises(capi.GceError) as ei:
        bamio.umi_to_mi(tmp_path / "in.bam", tmp_path / "out.bam")
    assert ei.value.status == -1 and "cannot open the input BAM" in str(ei.value)
    with pytest.raises(capi.GceError) as ei:
        bamio.umi_to_mi(tmp_path / "in.bam", tmp_path / "out.bam", source="MI")
    assert ei.value.status == -1 and "MI is what the run reads" in str(ei.value)
    sam = tmp_path / "in.sam"
    sam.write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tRX:Z:ACGT\n")
    for source in ("RX", "name"):
        with pytest.raises(capi.GceError) as ei:
            bamio.umi_to_mi(sam, tmp_path / "out.bam", source=source)
        assert ei.value.status == -1 and "gce_bam_umi_to_mi reads BAM, not SAM text" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.sam"]
    import inspect
    sig = inspect.signature(bamio.umi_to_mi)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("source", "RX"), ("device", 0), ("threads", 0), ("level", -2), ("window_bytes", 0), ("device_budget_bytes", 0),
                                                                          ("resident_bytes", 0)]


def test_help_names_the_flag():
    from gencore_amd.cli import EPILOG, build_parser
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--umi_from TAG\|name \[gencore_amd\]", h)
    assert "--umi_from RX" in EPILOG and "--umi_from name" in EPILOG and "MI:Z" in EPILOG


@pytest.mark.parametrize("argv, words", [
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "R"], "--umi_from should be a two-character tag such as RX, or name, got 'R'"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "NAME"], "--umi_from should be a two-character tag such as RX, or name, got 'NAME'"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "9X"], "--umi_from should be a two-character tag such as RX, or name, got '9X'"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "MI"], "--umi_from MI is what the run reads without the flag"),
    (["-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "RX"], "--umi_from needs an input file, not STDIN"),
    (["-i", "{sam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "RX"], "--umi_from needs BAM input, not SAM text"),
    (["-i", "{sam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "name"], "--umi_from needs BAM input, not SAM text"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "RX", "-u", "UMI"], "--umi_from cannot be combined with --umi_prefix"),
    (["-i", "{bam}", "-o", "{dir}/out.bam", "-r", "{fa}", "--umi_from", "name", "--umi_prefix", ""], "--umi_from cannot be combined with --umi_prefix"),
])
def test_flag_validation_errors(tmp_path, capsys, argv, words):
    from gencore_amd.cli import main
    bam, sam, fa = tmp_path / "in.bam", tmp_path / "in.sam", tmp_path / "ref.fa"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    sam.write_text("@HD\tVN:1.6\n")
    fa.write_text(">c0\nACGT\n")
    sub = dict(bam=str(bam), sam=str(sam), fa=str(fa), dir=str(tmp_path))
    assert main([a.format(**sub) for a in argv]) == 255
    assert ("ERROR: " + words) in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "in.sam", "ref.fa"]


def test_the_run_reads_an_empty_prefix_under_the_flag():
    from gencore_amd.cli import build_parser, params_of
    p = build_parser()
    assert params_of(p.parse_args(["-r", "x", "--umi_from", "RX"])).umi_prefix == b""
    assert params_of(p.parse_args(["-r", "x"])).umi_prefix == b"auto"


def test_model_against_hand_cases():
    labels = [c[0] for c in uc.all_cases()]
    assert len(set(labels)) == len(labels)
    for label, source, r, want, kind, dropped in uc.all_cases():
        new, info = pyumi.rewrite(r, source)
        assert new == want, label
        assert [k for k in ("tagged", "no_source", "not_umi") if info[k]] == [kind] and info["mi_dropped"] == dropped, label
        assert struct.unpack_from("<I", new)[0] == len(new) - 4 and new[4:36] == r[4:36], label       # (the fixed fields, bin included, are left alone)
        if kind == "tagged":
            assert new.endswith(b"MIZ:" + info["umi"] + b"\0") and re.fullmatch(rb"[ACGTN]+(_[ACGTN]+)?", info["umi"]), label
            assert [f[0] for f in pyumi.pycalmd.fields(new[len(new) - len(info["umi"]) - 5:])] == [b"MI"]
            again, info2 = pyumi.rewrite(new, source)               # idempotence: the MI written is dropped and written again
            assert again == new and info2["tagged"] and info2["mi_dropped"], label
        else:
            assert new == r, label
    big, want = uc.big_record()
    assert len(big) > 70000 and pyumi.rewrite(big, "RX")[0] == want and pyumi.rewrite(big, "name")[0] == big
    assert {len(c[2]) % 16 for c in uc.all_cases()} == set(range(16)) and {len(c[3]) % 16 for c in uc.all_cases()} == set(range(16))
    kinds = {(c[1] == "name", c[4]) for c in uc.all_cases()}
    assert kinds == {(n, k) for n in (False, True) for k in ("tagged", "no_source", "not_umi")}


def test_model_refusals_and_counters():
    good = [c[2] for c in uc.all_cases()]
    for label, r in uc.malformed():
        for source in ("RX", "name", "XA"):
            with pytest.raises(pyumi.Malformed):
                pyumi.rewrite(r, source)
            with pytest.raises(pyumi.UmiError) as ei:
                pyumi.umi_records(good[:7] + [r] + good[7:] + [uc.malformed()[0][1]], source)
            assert ei.value.record == 7, label
    for source in ("RX", "name"):
        out, c = pyumi.umi_records(good, source)
        mine = [x for x in uc.all_cases() if x[1] == source]
        assert c["n_records"] == len(good) == c["n_tagged"] + c["n_no_source"] + c["n_not_umi"]
        assert c["n_tagged"] >= sum(1 for x in mine if x[4] == "tagged") and c["n_not_umi"] >= sum(1 for x in mine if x[4] == "not_umi")
        assert 0 < c["n_mi_dropped"] < c["n_tagged"]
    _, c = pyumi.umi_records([x[2] for x in uc.all_cases() if x[1] == "RX"], "RX")
    rx = [x for x in uc.all_cases() if x[1] == "RX"]
    assert c == dict(n_records=len(rx), n_tagged=sum(x[4] == "tagged" for x in rx), n_no_source=sum(x[4] == "no_source" for x in rx), n_not_umi=sum(x[4] == "not_umi" for x in rx),
                     n_mi_dropped=sum(x[5] for x in rx))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """umi_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("umihost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "umi_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "umi_host_check.hip"), "-o", exe])
    return d, exe


@pytest.mark.parametrize("source", ["RX", "name", "BC"])
def test_record_functions_on_the_host(host_check, source):
    """umi::umi_record<false> / <true> and umi::copy_body on the host, under -fsanitize=address,undefined: the size, the counters' bits and
    every byte of every new record equal the model's, over all of umicases (the malformed records and the 70 KB record included), whatever
    the source the case was written for"""
    d, exe = host_check
    recs = uc.file_records() + [uc.big_record()[0]] + [r for _, r in uc.malformed()]
    (d / "frames").write_bytes(uc.frames(recs))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, source, str(d / "frames"), str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    rows = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    assert len(rows) == len(recs)
    got, p = [], 0
    blob = (d / "out").read_bytes()
    while p < len(blob):
        (n,) = struct.unpack_from("<I", blob, p)
        got.append(blob[p + 4:p + 4 + n])
        p += 4 + n
    assert len(got) == len(recs)
    n_bad = n_many = 0
    for k, rec in enumerate(recs):
        _, bad, tagged, no_source, not_umi, dropped, many, size = rows[k]
        try:
            new, info = pyumi.rewrite(rec, source)
        except pyumi.Malformed:
            assert bad == 1 and got[k] == b"", k
            n_bad += 1
            continue
        assert bad == 0 and got[k] == new and size == len(new), k
        assert (tagged, no_source, not_umi, dropped) == (int(info["tagged"]), int(info["no_source"]), int(info["not_umi"]), int(info["mi_dropped"])), k
        n_many += many
    assert n_bad == len(uc.malformed())
    assert n_many >= 2 or source != "RX"                            # (the path on which umi_record<true> copies the kept fields)


def test_without_its_umis_the_stream_gives_fewer_records(built, oracle):
    """the premise of the end-to-end tests (tests/test_umi_gpu.py): on their stream the oracle emits fewer records when the UMIs are not seen,
    so an output equal to the oracle's run WITH them shows that the pass's MI fields reached the engine"""
    from gencore_amd.batch import ReadBatch
    from gencore_amd.capi import default_params
    n = {}
    for style in ("RX", "name", None):
        ref, targets, a, b = uc.stream(style)
        assert all("mi" not in r for r in a) and (style is None or all(r["mi"].startswith(":") for r in b))
        tl = np.asarray([len(ref)], np.uint32)
        for label, recs in (("with", b), ("without", a)):
            want = oracle.run(ReadBatch.from_records(recs), default_params(n_targets=1, target_len=tl.ctypes.data, flush_period=40, umi_prefix=""),
                              [(oracle.pack_reference(ref), len(ref))])
            assert want.status == 0
            n[style, label] = len(want.emitted())
    print(n)
    assert n["RX", "with"] == n["name", "with"] > n["RX", "without"] == n["name", "without"] == n[None, "without"] == n[None, "with"] > 0
