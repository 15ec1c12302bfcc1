"""gce_bam_calmd_stream without a GPU: the symbol, its prototype, its two structs as the header gives them, the Python entry,
the help text, and the refusals that are made before a device is touched, in gce_bam_calmd's words."""
import ctypes as C
import os
import re

import pytest

import calmdcases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOOTPRINT = "the reference bases + one window + 40 bytes per window record + one piece's deflate buffers + at least one window's output"


def test_symbol_prototype_and_structs(built):
    import inspect
    from gencore_amd import bamio, capi
    text = open(os.path.join(ROOT, "include", "gencore_amd.h")).read()
    head = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    assert "typedef struct gce_calmd_stream_run { int32_t n_flushes, pad; int64_t resident_cap_bytes; int64_t flushed_bytes; } gce_calmd_stream_run;" in head
    assert ("int gce_bam_calmd_stream(const char *in_path, const char *out_path, const char *fasta_path, int32_t device, int threads, int level, uint64_t window_bytes, "
            "size_t device_budget_bytes, uint64_t resident_bytes, gce_calmd_run *out, gce_calmd_stream_run *run, char err[256]);") in head
    assert FOOTPRINT in re.sub(r"[\s*]+", " ", text)               # the header comment states the footprint in the message's words
    lib = capi.load_library()
    assert "gce_bam_calmd_stream" in capi.EXPORTED_SYMBOLS and hasattr(lib, "gce_bam_calmd_stream")
    assert lib.gce_bam_calmd_stream.argtypes == [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int, C.c_int, C.c_uint64, C.c_size_t, C.c_uint64, C.POINTER(capi.GceCalmdRun),
                                                 C.POINTER(capi.GceCalmdStreamRun), C.c_char_p]
    assert capi.GceCalmdStreamRun._fields_ == [("n_flushes", C.c_int32), ("pad", C.c_int32), ("resident_cap_bytes", C.c_int64), ("flushed_bytes", C.c_int64)]
    assert C.sizeof(capi.GceCalmdStreamRun) == 2 * 4 + 2 * 8 and C.sizeof(capi.GceCalmdRun) == 10 * 8 + 8 + 5 * 8
    sig = inspect.signature(bamio.calmd_bam_stream)
    assert list(sig.parameters) == ["in_path", "out_path", "fasta", "device", "threads", "level", "window_bytes", "device_budget_bytes", "resident_bytes"]
    assert [p.default for p in sig.parameters.values()][3:] == [0, 0, 6, 0, 0, 0]
    r = bamio.CalmdRun(capi.GceCalmdRun(), capi.GceCalmdStreamRun(n_flushes=3, resident_cap_bytes=0xff00, flushed_bytes=3 * 0xff00))
    assert (r.n_flushes, r.resident_cap_bytes, r.flushed_bytes, r.n_records) == (3, 0xff00, 3 * 0xff00, 0) and "pad" not in r.as_dict()


def test_refusals_before_a_device(built, tmp_path):
    from gencore_amd import bamio, capi
    lib = capi.load_library()
    fa = tmp_path / "ref.fa"
    fa.write_text(cc.FASTA_TEXT)
    run, srun, err = capi.GceCalmdRun(), capi.GceCalmdStreamRun(), (C.c_char * 256)()
    a, b, f = b"in.bam", str(tmp_path / "out.bam").encode(), str(fa).encode()
    for args in ((None, b, f), (a, None, f), (a, b, None)):
        assert lib.gce_bam_calmd_stream(*args, 0, 1, 6, 0, 0, 0, C.byref(run), C.byref(srun), err) == -1 and err.value == b"bad argument"
    assert lib.gce_bam_calmd_stream(a, b, f, 0, 1, 6, 0, 0, 0, None, C.byref(srun), err) == -1
    assert lib.gce_bam_calmd_stream(a, b, f, 0, 1, 6, 0, 0, 0, C.byref(run), None, err) == -1
    for level in (10, -4):
        assert lib.gce_bam_calmd_stream(a, b, f, 0, 1, level, 0, 0, 0, C.byref(run), C.byref(srun), err) == -1 and err.value == b"level should be -3, -2, -1 or 0..9"
    assert lib.gce_bam_calmd_stream(a, b, str(tmp_path / "none.fa").encode(), 0, 1, 6, 0, 0, 0, C.byref(run), C.byref(srun), err) == -1
    assert err.value == b"cannot open the reference FASTA"
    # the same words as gce_bam_calmd's
    for args, words in (((a, b, f, 0, 1, 10), b"level should be -3, -2, -1 or 0..9"), ((a, b, str(tmp_path / "none.fa").encode(), 0, 1, 6), b"cannot open the reference FASTA"),
                        ((None, b, f, 0, 1, 6), b"bad argument")):
        assert lib.gce_bam_calmd(*args, 0, 0, C.byref(run), err) == -1 and err.value == words
    # the input is looked at before a device too
    with pytest.raises(capi.GceError) as ei:
        bamio.calmd_bam_stream(tmp_path / "in.bam", tmp_path / "out.bam", fa)
    assert ei.value.status == -1 and "cannot open the input BAM" in str(ei.value)
    sam = tmp_path / "in.sam"
    sam.write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    with pytest.raises(capi.GceError) as ei:
        bamio.calmd_bam_stream(sam, tmp_path / "out.bam", fa, resident_bytes=0xff00)
    assert ei.value.status == -1 and "gce_bam_calmd_stream reads BAM, not SAM text" in str(ei.value)
    (tmp_path / "not.bam").write_bytes(b"\x1f\x8b\x08\x00" + bytes(60))
    with pytest.raises(capi.GceError) as ei:
        bamio.calmd_bam_stream(tmp_path / "not.bam", tmp_path / "out.bam", fa)
    assert ei.value.status == -1 and "not a BGZF file" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.sam", "not.bam", "ref.fa"]


def test_help_says_calmd_keeps_to_the_budget():
    from gencore_amd.cli import build_parser
    h = re.sub(r"\s+", " ", build_parser().format_help())
    flags = dict(re.findall(r" (--[a-z_]+)(?: [A-Z_]+)? \[gencore_amd\] (.*?)(?= --[a-z_]+(?: [A-Z_]+)? \[gencore_amd\]|$)", h))
    assert "budget" in flags["--calmd"] and "--device_memory" in flags["--calmd"]
    assert "budget" in flags["--calmd_in"] and "--device_memory" in flags["--calmd_in"]
    assert "--calmd" in flags["--device_memory"] and "--calmd_in" in flags["--device_memory"]
    assert "The report is not changed by it" in flags["--calmd"]
