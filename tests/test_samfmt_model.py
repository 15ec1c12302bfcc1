"""gce_sam_format / gce_raw_format_output without a GPU: the symbols and prototypes, the command line's help, and the per-record functions of
the kernels (gce_samfmt.hpp) compiled for the host and compared with samtext::bam_to_line record by record."""
import ctypes as C
import os
import re
import subprocess

import samcases
import samfmtcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_prototypes(built):
    from gencore_amd import capi
    head = open(os.path.join(ROOT, "include", "gencore_amd.h")).read()
    flat = re.sub(r"\s+", " ", head)
    assert ("int gce_sam_format(int32_t device, const void *records, size_t n, int32_t n_ref, const char *const *ref_name, void *out, size_t out_cap, "
            "size_t *out_bytes, int64_t *n_records, int64_t *n_host_records, int64_t *bad_record, char err[256]);") in flat
    assert "int gce_raw_format_output(gce_engine *e, int32_t n_ref, const char *const *ref_name, uint64_t *text_bytes);" in flat
    assert "int gce_raw_read_text_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket);" in flat
    assert "int gce_get_sam_format_counters(int64_t out[4]);" in flat
    lib = capi.load_library()
    for name in ("gce_sam_format", "gce_raw_format_output", "gce_raw_read_text_async", "gce_get_sam_format_counters"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.gce_sam_format.argtypes == [C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p]
    assert lib.gce_raw_format_output.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)]
    assert lib.gce_raw_read_text_async.argtypes == [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    assert lib.gce_get_sam_format_counters.argtypes == [C.POINTER(C.c_int64)]
    # arguments are checked before any device is touched
    err = (C.c_char * 256)()
    assert lib.gce_sam_format(0, None, 5, 0, None, None, 0, None, None, None, None, err) == -1
    tb = C.c_uint64(7)
    assert lib.gce_raw_format_output(None, 0, None, C.byref(tb)) == -1
    assert lib.gce_raw_read_text_async(None, 0, None, 0, None) == -1
    assert lib.gce_get_sam_format_counters(None) == -1
    from gencore_amd import bamio
    assert callable(bamio.format_sam) and len(bamio.sam_format_counters()) == 4


def test_a_walk_refusal_needs_no_device(built):
    """a stream whose FIRST record the walk refuses (block_size 31, or cut by the end of the buffer) is answered on the host"""
    from gencore_amd.bamio import format_sam
    from gencore_amd.capi import GceError
    import pytest
    for _, r in samfmtcases.bad_records()[:1] + samfmtcases.cut_records():
        with pytest.raises(GceError) as ei:
            format_sam(r, samfmtcases.NAMES)
        assert ei.value.status == -1 and ei.value.bad_record == 0 and str(ei.value).endswith(": bad record in the output stream")


def test_help_names_the_gpu_writer():
    from gencore_amd.cli import build_parser
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert "With an output name that ends in sam, -2 and -3 make the GPU write the SAM text" in h


def test_the_model_agrees_with_pybam():
    """samfmtcases.line_of (the independent model of a record's line) against pybam.sam_line on the field-edge cases both can express"""
    for line, recb, _ in samcases.field_edge_cases():
        got = samfmtcases.line_of(recb)
        assert got is not None and got.endswith(b"\n")
        f, g = line.split("\t"), got[:-1].decode("latin-1").split("\t")
        assert g[0] == f[0] and g[9].upper().replace(".", "N") == g[9] and len(g) == len(f)
    for label, r in samfmtcases.hand_built():
        assert samfmtcases.line_of(r) is not None, label
    for label, r in samfmtcases.bad_records() + samfmtcases.cut_records():
        assert samfmtcases.line_of(r) is None, label


def test_record_functions_on_the_host(tmp_path):
    """samfmt::format_record (size, verdict, bytes), samfmt::emit_seq (one lane and 16 lanes standing in for the group, every alignment of the
    line) and samfmt::walk_records against samtext::bam_to_line, tests/samfmt_host_check.hip; the lines also equal the independent model's."""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path / "samfmt_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "samfmt_host_check.hip"), "-o", exe])
    cases = samcases.field_edge_cases()
    more = samcases.more_good_lines()
    hand, bad, cut = samfmtcases.hand_built(), samfmtcases.bad_records(), samfmtcases.cut_records()
    (tmp_path / "names").write_text("".join(n + "\n" for n in samfmtcases.NAMES))
    (tmp_path / "text").write_bytes(samcases.text_of(cases) + b"".join(l.encode("latin-1") + b"\n" for l in more))
    (tmp_path / "frames").write_bytes(samfmtcases.frames([r for _, r in hand + bad + cut]))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(tmp_path / "names"), str(tmp_path / "text"), str(tmp_path / "frames"), str(tmp_path / "out")],
                       stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-3000:]
    rows = [l.split(" ") for l in r.stdout.splitlines()]
    n_text = len(cases) + len(more)
    assert len(rows) == n_text + len(hand) + len(bad) + len(cut)
    for k, c in enumerate(cases):
        assert rows[k][1] == "ok" and int(rows[k][3]) == int(c[2]), (k, rows[k])
        assert int(rows[k][2]) == len(samfmtcases.line_of(c[1]))
    assert all(x[1] == "ok" and x[3] == "0" for x in rows[len(cases):n_text])
    want = [samfmtcases.line_of(c[1]) for c in cases]
    for k, (label, rb) in enumerate(hand):
        line, host = samfmtcases.analyse(rb)
        assert rows[n_text + k][1:] == ["ok", str(len(line)), str(int(host))], (label, rows[n_text + k])
        want.append(line)
    assert all(x[1] == "bad" for x in rows[n_text + len(hand):]), rows[n_text + len(hand):]
    got = (tmp_path / "out").read_bytes()
    lines = got.split(b"\n")
    # the lines of the text cases and of the hand-built records are the model's; those of more_good_lines have no model and lie between them
    assert got.startswith(b"".join(want[:len(cases)])) and got.endswith(b"".join(want[len(cases):]))
    assert len(lines) >= n_text + len(hand)


def test_sam_out_bench_has_its_variants():
    """tools/sam_out_bench.py: the --lib switch of the yardstick and the kernel-name match of its rocprofv3 run"""
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sam_out_bench.py"), "--help"], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and "--lib" in r.stdout and "--reps" in r.stdout
    assert re.search(r"k_samfmt_\w+", "(anonymous namespace)::k_samfmt_seq(unsigned char const*, unsigned long const*)").group(0) == "k_samfmt_seq"
