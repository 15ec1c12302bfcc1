"""gce_sam_parse / gce_sam_sort / --sort_sam without a GPU: the command line's validation, the symbols and prototypes, and the per-line
functions of the kernels (gce_samdev.hpp) compiled for the host and compared with samtext::line_to_bam line by line."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import samcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, GCE_LIB="/nonexistent/libgencore_amd.so")      # (a library that cannot load: validation must come first)
    return subprocess.run([sys.executable, "-m", "gencore_amd"] + args, cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture()
def files(tmp_path):
    (tmp_path / "ref.fa").write_text(">chr1\nACGT\n")
    (tmp_path / "in.sam").write_text("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:4\n" + samcases.GOOD + "\n")
    (tmp_path / "in.bam").write_bytes(b"\x1f\x8b\x08\x04" + b"\0" * 24)
    return tmp_path


def test_validation_messages(files):
    r = cli(["-i", "in.bam", "-r", "ref.fa", "-o", "o.bam", "--sort", "--sort_sam"], files)
    assert r.returncode == 255 and "--sort and --sort_sam cannot be combined" in r.stderr
    r = cli(["-r", "ref.fa", "-o", "o.bam", "--sort_sam"], files)
    assert r.returncode == 255 and "--sort_sam needs an input file, not STDIN" in r.stderr
    r = cli(["-i", "in.bam", "-r", "ref.fa", "-o", "o.bam", "--sort_sam"], files)
    assert r.returncode == 255 and "--sort_sam needs SAM text input, not BAM" in r.stderr
    assert not (files / "o.bam").exists()


def test_sort_still_refuses_sam_text(files):
    r = cli(["-i", "in.sam", "-r", "ref.fa", "-o", "o.bam", "--sort"], files)
    assert r.returncode == 255 and "--sort needs BAM input, not SAM text" in r.stderr
    r = cli(["-i", "in.sam", "-r", "ref.fa", "-o", "o.bam", "--sort", "--sort_sam"], files)
    assert r.returncode == 255 and "--sort needs BAM input, not SAM text" in r.stderr


def test_help_names_the_flag():
    from gencore_amd.cli import EPILOG, build_parser
    assert "--sort_sam" in EPILOG and "--sort_sam" in build_parser().format_help()


def test_symbols_and_prototypes(built):
    from gencore_amd import capi
    from gencore_amd.capi import GceSortRun
    head = open(os.path.join(ROOT, "include", "gencore_amd.h")).read()
    flat = re.sub(r"\s+", " ", head)
    assert ("int gce_sam_parse(int32_t device, const char *text, size_t n, int32_t n_ref, const char *const *ref_name, void *out, size_t out_cap, "
            "size_t *out_bytes, int64_t *n_records, int64_t *n_host_lines, int64_t *bad_line, char err[256]);") in flat
    assert ("int gce_sam_sort(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes, "
            "size_t device_budget_bytes, gce_sort_run *out, int64_t *n_host_lines, char err[256]);") in flat
    lib = capi.load_library()
    assert "gce_sam_parse" in capi.EXPORTED_SYMBOLS and "gce_sam_sort" in capi.EXPORTED_SYMBOLS
    assert lib.gce_sam_parse.argtypes == [C.c_int32, C.c_char_p, C.c_size_t, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p]
    assert lib.gce_sam_sort.argtypes == [C.c_char_p, C.c_char_p, C.c_int32, C.c_int, C.c_int, C.c_uint64, C.c_size_t, C.POINTER(GceSortRun), C.POINTER(C.c_int64), C.c_char_p]
    # arguments are checked before any device is touched
    err = (C.c_char * 256)()
    assert lib.gce_sam_sort(None, b"x", 0, 1, -2, 0, 0, None, None, err) == -1
    assert lib.gce_sam_parse(0, None, 5, 0, None, None, 0, None, None, None, None, err) == -1
    from gencore_amd import bamio
    assert callable(bamio.sort_sam) and callable(bamio.parse_sam)


def test_the_cases_against_the_host_parser(built, tmp_path):
    """the field-edge cases are what pybam's model says (samcases.case) AND what the host's sam_to_bam writes: the two references agree"""
    import pybam
    from gencore_amd.bamio import sam_to_bam
    cases = samcases.field_edge_cases()
    with open(tmp_path / "c.sam", "wb") as f:
        f.write(b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in samcases.TARGETS) + samcases.text_of(cases))
    sam_to_bam(tmp_path / "c.sam", tmp_path / "c.bam", threads=2, level=1)
    import gzip
    u = gzip.decompress(open(tmp_path / "c.bam", "rb").read())
    want = b"".join(k[1] for k in cases)
    assert u.endswith(want) and len(want) > 0
    assert samcases.n_float_lines(cases) == 3


def test_line_functions_on_the_host(tmp_path):
    """samdev::parse_line (size, verdict, bytes) and samdev::emit_seq (one lane and 16 lanes standing in for the group, every alignment of the
    record) against samtext::line_to_bam, tests/samdev_host_check.hip: the field edges, CRLF, every message, and lines no writer prints."""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path / "samdev_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "samdev_host_check.hip"), "-o", exe])
    cases = samcases.field_edge_cases()
    bad = samcases.malformed_cases()
    lines = [k[0].encode() for k in cases] + [k[0].encode() + b"\r" for k in cases[:6]] + [l.encode("latin-1") for _, l in bad] \
        + [l.encode("latin-1") for l in samcases.more_bad_lines()] + [l.encode("latin-1") for l in samcases.more_good_lines()]
    (tmp_path / "names").write_text("".join(n + "\n" for n, _ in samcases.TARGETS) + "chr1\n")        # (a name twice: the first one counts)
    (tmp_path / "text").write_bytes(b"\n".join(lines) + b"\n\r\n\n" + samcases.GOOD.encode())           # (empty lines, a lone CR, no last line feed)
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(tmp_path / "names"), str(tmp_path / "text")], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-3000:]
    rows = [l.split(" ", 4) for l in r.stdout.splitlines()]
    assert len(rows) == len(lines) + 1
    n0 = len(cases) + 6
    for k, c in enumerate(cases):
        assert rows[k][1] == "ok" and int(rows[k][2]) == len(c[1]) and int(rows[k][3]) == int(c[2]), (k, rows[k])
    for k, (msg, _) in enumerate(bad):
        assert rows[n0 + k][1] == "bad" and rows[n0 + k][4] == msg, rows[n0 + k]
    n1 = n0 + len(bad)
    assert all(r_[1] == "bad" for r_ in rows[n1:n1 + len(samcases.more_bad_lines())])
    assert all(r_[1] == "ok" for r_ in rows[n1 + len(samcases.more_bad_lines()):])


def test_sort_bench_has_the_sam_mode():
    """tools/sort_bench.py --sam: the mode, its two child variants and the kernel-name match of its rocprofv3 run"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sort_bench", os.path.join(ROOT, "tools", "sort_bench.py"))
    sb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sb)
    assert callable(sb.sam_mode) and callable(sb.child_sam)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sort_bench.py"), "--help"], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and "--sam" in r.stdout and "--lib" in r.stdout
    assert re.search(r"k_sam_\w+", "(anonymous namespace)::k_sam_emit_seq(unsigned char const*, unsigned int const*)").group(0) == "k_sam_emit_seq"
