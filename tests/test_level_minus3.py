"""Level -3 (the GPU encoder with dynamic Huffman codes, gce_deflate.hpp) as far as it goes without a device: the command line takes the level, the
C-ABI declares, lists and exports the two entry points that carry the choice of coder, and they refuse bad arguments before any GPU call."""
import ctypes as C

import numpy as np
import pytest

from test_capi_symbols import declared_functions
from test_cli import cli

NEW = ("gce_bgzf_deflate_codes", "gce_raw_deflate_output_codes")


@pytest.fixture
def workdir(tmp_path):
    (tmp_path / "in.bam").write_bytes(b"")
    return tmp_path


def test_cli_accepts_level_minus_3(workdir):
    """the level passes its rule: the run goes on to the next check, the device memory budget"""
    for level in ("-3", "-2", "9"):
        r = cli(["-i", "in.bam", "-r", "ref.fa", "--level", level, "--device_memory", "none"], workdir)
        assert r.returncode != 0 and r.stderr == "ERROR: device_memory should be a positive number of GB or auto, got 'none'\n", level


@pytest.mark.parametrize("level", ["-4", "10"])
def test_cli_rejects_levels_outside(workdir, level):
    r = cli(["-i", "in.bam", "-r", "ref.fa", "--level", level], workdir)
    assert r.returncode != 0 and r.returncode != 124
    assert r.stderr == "ERROR: level should be -3, -2, -1 or 0..9\n" and r.stdout == ""


def test_cli_help_names_the_level(workdir):
    r = cli(["--help"], workdir)
    assert r.returncode == 0 and "-3 (" in r.stdout and "dynamic Huffman" in " ".join(r.stdout.split())


def test_symbols_declared_listed_exported(built):
    from gencore_amd import capi
    lib = capi.load_library()
    names = declared_functions()
    for n in NEW:
        assert n in names and n in capi.EXPORTED_SYMBOLS and hasattr(lib, n), n


def test_bad_arguments_are_refused_without_a_device(built):
    """GCE_ERR_INVALID (-1), never GCE_ERR_NO_DEVICE (-2): the checks come before the first HIP call"""
    from gencore_amd import capi
    lib = capi.load_library()
    data = np.zeros(64, np.uint8)
    out = np.zeros(256, np.uint8)
    got = C.c_size_t(7)
    f = lib.gce_bgzf_deflate_codes
    assert f(0, None, 64, 0xff00, 1, out.ctypes.data, 256, C.byref(got)) == -1              # no input
    assert f(0, data.ctypes.data, 64, 0xff00, 1, None, 256, C.byref(got)) == -1             # no output
    assert f(0, data.ctypes.data, 64, 0xff00, 1, out.ctypes.data, 256, None) == -1          # nowhere to put the size
    assert f(0, data.ctypes.data, 64, 0xff01, 1, out.ctypes.data, 256, C.byref(got)) == -1  # a block BGZF cannot hold
    assert f(0, data.ctypes.data, 64, 0, 1, out.ctypes.data, 256, C.byref(got)) == -1
    assert f(0, data.ctypes.data, 64, 0xff00, 3, out.ctypes.data, 256, C.byref(got)) == -1  # no such coder
    assert f(0, data.ctypes.data, 64, 0xff00, -1, out.ctypes.data, 256, C.byref(got)) == -1
    assert got.value == 7
    cb = C.c_uint64(0)
    assert lib.gce_raw_deflate_output_codes(None, 1, C.byref(cb)) == -1


def test_python_wrapper_refuses_a_bad_block(built):
    from gencore_amd.bamio import bgzf_deflate
    from gencore_amd.capi import GceError
    with pytest.raises(GceError) as e:
        bgzf_deflate(b"abc", block=0xff01)
    assert e.value.status == -1


def test_encoder_on_the_host_against_zlib(tmp_path):
    """def_encode_best (what each lane of k_bgzf_deflate_dyn runs) compiled for the host, tests/deflate_host_check.hip: every block of every payload
    kind at every block size inflates under zlib, fits its slot, and under codes=1 is never larger than the fixed-code encoder's block; skewed counts
    (Fibonacci) reach the 12-bit length limit; dynamic codes are chosen for quality-like bytes."""
    import os
    import subprocess
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path / "deflate_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "deflate_host_check.hip"), "-o", exe, "-lz"])
    rng = np.random.default_rng(3)
    fib, a, b = [], 1, 1
    for s in range(22):
        fib += [s * 11] * a
        a, b = b, a + b
    fib = rng.permutation(np.array(fib[:65280], np.uint8))
    text = b"".join(b"read%d\t99\tchr1\t%d\t60\t150M\t=\t%d\t300\tACGT\tFFFF\tNM:i:%d\n" % (i, 1000 + i, 1200 + i, i % 3) for i in range(3000))
    data = {"one_byte": b"Q" * 70000, "two_values": bytes(rng.choice(np.array([7, 200], np.uint8), 65280)), "all_256": bytes(range(256)),
            "distance_1": bytes(range(40)) + b"\x55" * 900 + bytes(range(100, 140)), "random": bytes(rng.integers(0, 256, 140000, dtype=np.uint8)),
            "quality": bytes(rng.integers(33, 74, 100000, dtype=np.uint8)), "text": text, "fibonacci": bytes(fib), "A": b"A", "ACGTA": b"ACGTA",
            "runs": bytes(np.repeat(rng.integers(0, 256, 2000, dtype=np.uint8), rng.integers(1, 300, 2000))),
            "far": bytes(rng.integers(0, 256, 40000, dtype=np.uint8)) * 3}
    paths = []
    for name, d in data.items():
        (tmp_path / name).write_bytes(d)
        paths.append(str(tmp_path / name))
    r = subprocess.run(["timeout", "-k", "10", "300", exe] + paths, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-2000:]
    rows = {os.path.basename(l.split()[0]): [int(x) for x in l.split()[1:]] for l in r.stdout.splitlines()}
    assert set(rows) == set(data)
    n, fixed, best, n_dyn = rows["quality"]
    assert n_dyn > 0 and best < fixed
    assert rows["fibonacci"][3] > 0 and rows["random"][3] == 0 and rows["random"][2] == rows["random"][1]
