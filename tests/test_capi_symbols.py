"""The C-ABI library loads and exports every symbol include/gencore_amd.h declares; struct layouts agree between
the header (compiled with gcc) and the ctypes mirror.  No compute call is made (works without a GPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    txt = open(os.path.join(ROOT, "include", "gencore_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gce_[a-z_0-9]+)\s*\(", txt)))


def test_header_symbols_exported(built):
    from gencore_amd import capi
    lib = capi.load_library()
    names = declared_functions()
    assert set(names) == set(capi.EXPORTED_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.gce_abi_version() == capi.GCE_ABI_VERSION


def entry_functions():
    txt = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    txt = re.sub(r"//[^\n]*", "", txt)
    return sorted(set(re.findall(r"\b(gce_[a-z_0-9]+)\s*\(", txt)))


def test_internal_entry_points_declared_once(built):
    """gce_entry.h declares the device entry points the file side calls beside the public header's: every one is exported, none is also in
    the public header, and the file side (csrc/*.cpp and its bamio_*.hpp parts) holds no gce_ prototype of its own -- no file-scope
    declaration of a gce_ function that ends in `;` -- so the definitions in engine.hip and the calls see one prototype each."""
    import glob
    from gencore_amd import capi
    lib = capi.load_library()
    names = entry_functions()
    assert len(names) > 30 and "gce_sort_read" in names and "gce_passes_window" in names and "gce_bai_finish" in names and "gce_device_mem_info" in names
    for n in names:
        assert hasattr(lib, n), n
    assert not set(names) & set(declared_functions())
    csrc = os.path.join(ROOT, "gencore_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "bamio_*.hpp")))
    assert [os.path.basename(f) for f in files if f.endswith(".cpp")] == ["bamio.cpp"] and len(files) >= 9
    # a prototype: from the start of a line a return type, the name, a parameter list without braces or semicolons, then `;` -- a call
    # starts indented or behind `=`, `(` or `return`, and a definition's parameter list is followed by `{`
    proto = re.compile(r"^(?:extern\s+\"C\"\s+)?(?:static\s+|inline\s+)*(?:const\s+)?[A-Za-z_][A-Za-z_0-9]*[\s\*]+(gce_[a-z_0-9]+)\s*\([^;{}]*\)\s*;", re.M)
    assert proto.search("int gce_sort_read(gce_sort *b, uint64_t offset,\n                  size_t bytes);").group(1) == "gce_sort_read"
    assert proto.search("const char *gce_bai_error(gce_bai *b);") and proto.search("void gce_host_free(void *p);")
    assert not proto.search("int gce_x(int a) { return a; }\n    if (gce_y(1)) return gce_z(2);\nint r = gce_w(3);")
    for f in files:
        txt = re.sub(r"//[^\n]*", "", open(f).read())
        assert not proto.findall(txt), (os.path.basename(f), proto.findall(txt))


def test_index_counters_symbol(built):
    """gce_get_index_counters (ABI v3) is exported, refuses a NULL output and, with no engine, reads the pass runner's window totals (no GPU
    call: this runs without a device)."""
    from gencore_amd import capi
    from gencore_amd.engine import index_counters
    lib = capi.load_library()
    assert "gce_get_index_counters" in capi.EXPORTED_SYMBOLS and hasattr(lib, "gce_get_index_counters")
    assert lib.gce_get_index_counters(None, None) == -1
    c = index_counters()
    assert sorted(c) == ["flagged", "rounds", "segments", "serial"] and all(v >= 0 for v in c.values())
    assert c["flagged"] <= c["segments"] and c["serial"] <= c["rounds"]


def test_consensus_counters_symbol(built):
    """gce_get_consensus_counters (added under ABI v3) is exported and refuses a NULL engine or output (no GPU call: this runs without a device)."""
    from gencore_amd import capi
    from gencore_amd.engine import Engine
    lib = capi.load_library()
    assert "gce_get_consensus_counters" in capi.EXPORTED_SYMBOLS and hasattr(lib, "gce_get_consensus_counters")
    assert lib.gce_get_consensus_counters(None, None) == -1
    v = (C.c_int64 * 5)()
    assert lib.gce_get_consensus_counters(None, v) == -1
    assert len(Engine.CONSENSUS_KERNELS) == 5


def test_pairing_tier_ids_match_header():
    """gce_get_pairing_tiers' tier ids (GCE_PAIR_TIER_*) are the names Engine.pairing_tiers() reports, in order."""
    from gencore_amd.engine import Engine
    txt = open(os.path.join(ROOT, "include", "gencore_amd.h")).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"GCE_PAIR_TIER_([A-Z0-9_]+)\s*=\s*(\d+)", txt)}
    assert ids == {name: k for k, name in enumerate(Engine.PAIR_TIERS)}
    assert int(re.search(r"GCE_PAIR_TIERS\s*=\s*(\d+)", txt).group(1)) == len(Engine.PAIR_TIERS)


def test_struct_layouts_match_header(built, tmp_path):
    from gencore_amd import capi
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",sizeof(gce_core),sizeof(gce_params),'
                   'sizeof(gce_batch),sizeof(gce_stats),sizeof(gce_result),sizeof(gce_timing),sizeof(gce_depth),sizeof(gce_bam_info),'
                   'sizeof(gce_bam_run),sizeof(gce_payload_layout),sizeof(gce_depth_run));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [capi.CORE_DTYPE.itemsize, C.sizeof(capi.GceParams), C.sizeof(capi.GceBatch), C.sizeof(capi.GceStats),
                     C.sizeof(capi.GceResult), C.sizeof(capi.GceTiming), C.sizeof(capi.GceDepth), C.sizeof(capi.GceBamInfo),
                     C.sizeof(capi.GceBamRun), C.sizeof(capi.GcePayloadLayout), C.sizeof(capi.GceDepthRun)]


def test_defaults_match_reference_options(built):
    from gencore_amd import capi
    lib = capi.load_library()
    p = capi.GceParams()
    lib.gce_params_default(C.byref(p))
    q = capi.default_params()
    for name, _ in capi.GceParams._fields_:
        if name in ("target_len", "umi_prefix"):
            continue
        assert getattr(p, name) == getattr(q, name), name
    # src/options.cpp:4-40
    assert (p.proper_umi_diff_threshold, p.unproper_umi_diff_threshold, p.duplex_mismatch_threshold) == (1, 0, 2)
    assert (p.high_quality, p.moderate_quality, p.low_quality) == (30, 20, 15)
    assert (p.score_high, p.score_moderate, p.score_low, p.score_bad, p.base_score_req) == (8, 6, 4, 2, 6)
    assert p.score_percent_req == 0.8 and p.skip_low_complexity_cluster_threshold == 1000 and p.flush_period == 10000


def test_umi_prefix_autodetect(built):
    from gencore_amd import capi
    lib = capi.load_library()
    for name, want in ((b"A:1:UMI_ACGT", b"UMI"), (b"A:1:umi_ACGT", b"umi"), (b"A:1:ACGT", b"")):   # src/gencore.cpp:207-216
        buf = (C.c_char * 32)()
        lib.gce_detect_umi_prefix(name, buf)
        assert buf.value == want


def test_no_device_is_a_loud_error_not_a_fallback(built):
    """Without a GPU gce_create must refuse (GCE_ERR_NO_DEVICE): the product has no CPU path."""
    import torch
    if torch.cuda.is_available():
        return
    from gencore_amd import capi
    lib = capi.load_library()
    h = C.c_void_p()
    p = capi.default_params()
    assert lib.gce_create(C.byref(p), C.byref(h)) == -2


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "gencore_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "oracle_py" not in txt and "gencore_oracle" not in txt and "libgencore_oracle" not in txt, f
