"""The reference's reports (gencore_amd/csrc/gce_report.hpp) as thin ctypes wrappers: write_json (gce_report_json: JsonReporter::report),
summary (gce_report_summary: Stats::print) and read_header (gce_bam_read_header: the contig table of a BAM or SAM file).  No GPU is touched."""
import ctypes as C

import numpy as np

from . import capi
from .capi import GceDepthRun, GceError, GceStats


def _stats(s):
    return s if isinstance(s, GceStats) else GceStats.from_buffer_copy(bytes(s))


def read_header(path):
    """(contig names, contig lengths) of a BAM or SAM file, in header order."""
    lib = capi.load_library()
    n = C.c_int32()
    names, lens = C.POINTER(C.c_char_p)(), C.POINTER(C.c_uint32)()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_read_header(str(path).encode(), C.byref(n), C.byref(names), C.byref(lens), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    out = ([names[k].decode() for k in range(n.value)], [int(lens[k]) for k in range(n.value)])
    lib.gce_bam_header_free(n, names, lens)
    return out


def summary(stats, post):
    """Stats::print of one block as text (pre block: post=False)."""
    lib = capi.load_library()
    st = _stats(stats)
    need = C.c_size_t()
    lib.gce_report_summary(C.byref(st), int(post), None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value + 1)
    rc = lib.gce_report_summary(C.byref(st), int(post), buf, len(buf), C.byref(need))
    if rc != 0:
        raise GceError(rc, "gce_report_summary")
    return buf.value.decode()


def write_json(path, depth, target_names, coverage_step, command, region_names=None, has_bed=False):
    """gce_report_json.  depth: the dict bamio.run_bam_depth returns (bin_off, pre_depth, post_depth, regions, pre_bed, post_bed, pre, post),
    or one built by hand with the same keys; region_names: one per entry of depth["regions"]."""
    lib = capi.load_library()
    keep = []

    def ptr(a, dt, ct):
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ct))
    regions = list(depth.get("regions", []))
    dr = GceDepthRun()
    dr.n_targets = len(target_names)
    dr.bin_off = ptr(depth["bin_off"], np.int64, C.c_int64)
    dr.n_bins = int(dr.bin_off[dr.n_targets]) if dr.n_targets else 0
    dr.pre_depth, dr.post_depth = ptr(depth["pre_depth"], np.int64, C.c_int64), ptr(depth["post_depth"], np.int64, C.c_int64)
    dr.n_regions = len(regions)
    reg = np.asarray(regions, np.int32).reshape(-1, 3)
    dr.region_tid, dr.region_start, dr.region_end = (ptr(reg[:, k], np.int32, C.c_int32) for k in range(3))
    dr.pre_bed, dr.post_bed = ptr(depth.get("pre_bed", []), np.int64, C.c_int64), ptr(depth.get("post_bed", []), np.int64, C.c_int64)
    pre, post = _stats(depth["pre"]), _stats(depth["post"])
    tn = (C.c_char_p * max(len(target_names), 1))(*[n.encode() for n in target_names])
    rn = None
    if region_names is not None:
        rn = (C.c_char_p * max(len(region_names), 1))(*[n.encode() for n in region_names])
    err = (C.c_char * 256)()
    rc = lib.gce_report_json(str(path).encode(), C.byref(pre), C.byref(post), C.byref(dr), tn, rn, int(bool(has_bed)), int(coverage_step),
                             command.encode(), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
