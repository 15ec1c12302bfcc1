"""The GPU record index (gce_bamdev.hpp k_raw_seg / k_raw_check / k_raw_fix / k_raw_repair, the host loops of gce_raw_finish and of the pass
runner's gce_passes_window) on streams built to take each of its paths (tests/recordstreams.py): a shifted false guess, records spanning
1 .. 65 segments, runs of record-shaped bytes inside long B:C arrays whose false chains resync or break, record starts and stream ends at
segment boundaries, a header of odd length.  CPU: every case takes its path in the spec, and the host reader returns exactly the records
written.  GPU: the raw push paths, the file runner and the pass runner index every case as the host does, give the host batch's results,
and their counters (gce_get_index_counters) equal the spec's prediction; damaged streams stay refused."""
import ctypes as C

import numpy as np
import pytest

import recordstreams as R

CASES = sorted(R.CASES)

# the path of every case in the spec: flagged (the first check), rounds, serial repair, a fix walked from a wrong predecessor, such a walk broke
PATHS = {
    "shifted_guess": ([2, 3], 1, False, False, False),
    "span_1": ([1, 2], 1, False, False, False),
    "span_2": ([1, 2, 3], 2, False, False, False),
    "span_63": (list(range(1, 65)), 63, False, False, False),
    "span_64": (list(range(1, 66)), 64, False, False, False),
    "span_65": (list(range(1, 67)), 64, True, False, False),
    "fake_resync": ([1], 3, False, False, False),
    "fake_breaks": ([1, 3, 4], 3, False, True, True),
    "fake_breaks_in_2": ([1, 2, 3, 4, 5], 4, False, False, False),
    "fake_breaks_in_3": ([1, 3, 4, 5], 4, False, True, True),
    "fake_breaks_in_4": ([1, 4, 5], 5, False, True, True),
    "two_long": ([1, 2, 3], 5, False, False, False),
    "start_at_boundary_m1": ([], 0, False, False, False),
    "start_at_boundary_0": ([], 0, False, False, False),
    "start_at_boundary_p1": ([], 0, False, False, False),
    "end_at_boundary_0": ([], 0, False, False, False),
    "end_at_boundary_p1": ([3], 1, False, False, False),
    "odd_header": ([1], 3, False, False, False),
}

_BUILT = {}


def built_case(name):
    if name not in _BUILT:
        _BUILT[name] = R.CASES[name]()
    return _BUILT[name]


def spec(name, soft=False):
    b = built_case(name)
    return R.classify(b.stream(), b.first, len(b.targets), soft)


# ------------------------------------------------------------------------------------------------------------------------------- CPU
def test_every_path_is_named():
    assert sorted(PATHS) == CASES


@pytest.mark.parametrize("name", CASES)
def test_case_takes_its_path(name):
    b = built_case(name)
    res = spec(name)
    flagged, rounds, serial, wrong, broke = PATHS[name]
    assert (res["flagged"], res["rounds"], res["serial"], res["wrong_predecessor"], res["fix_broke"]) == (flagged, rounds, serial, wrong, broke)
    assert res["error"] is None and res["offsets"] == b.record_offsets()
    assert res["segments"] == (len(b.stream()) - b.first + R.SEG - 1) // R.SEG


def test_case_geometry():
    """the builder put the bytes where the cases say"""
    b = built_case("shifted_guess")
    lo = b.first + 2 * R.SEG
    assert lo + 1 in b.record_offsets() and spec("shifted_guess")["guesses"][2] == lo          # the guess one byte in front of a record
    for d in (-1, 0, 1):
        b = built_case("start_at_boundary_%s" % {-1: "m1", 0: "0", 1: "p1"}[d])
        assert b.first + 3 * R.SEG + d in b.record_offsets()
    for d in (0, 1):
        b = built_case("end_at_boundary_%s" % {0: "0", 1: "p1"}[d])
        assert len(b.stream()) == b.first + 3 * R.SEG + d
    assert built_case("odd_header").first % 4 != 0
    for m in (1, 2, 63, 64, 65):                       # m segments without a record start
        b = built_case("span_%d" % m)
        starts = set((o - b.first) // R.SEG for o in b.record_offsets())
        assert sum(1 for s in range(spec("span_%d" % m)["segments"]) if s not in starts) == m
    for name in ("fake_breaks", "fake_breaks_in_2", "fake_breaks_in_3", "fake_breaks_in_4", "two_long", "fake_resync"):
        assert R.fake_record() in built_case(name).stream()


@pytest.mark.parametrize("name", sorted(R.DAMAGED))
def test_damaged_stream_is_refused_by_the_spec(name):
    b, u = R.DAMAGED[name]()
    res = R.classify(u, b.first, len(b.targets), False)
    assert res["serial"] and res["error"] == "truncated or damaged BAM record stream"


def test_spec_soft_end_and_windows():
    """SOFT: a window that ends inside a long record leaves the chain at that record; the pass runner's windows, carried record by carried
    record, give every record start of the file once"""
    b = built_case("span_2")
    u = b.stream()
    cut = b.first + R.SEG + 100                        # inside the long record
    res = R.classify(u[:cut], b.first, len(b.targets), True)
    long_at = max(o for o in b.record_offsets() if o < cut)
    assert res["error"] is None and res["end"] == long_at and res["offsets"] == [o for o in b.record_offsets() if o < long_at]
    hard = R.classify(u[:cut], b.first, len(b.targets), False)
    assert hard["error"] is not None
    for name in ("span_2", "fake_breaks", "two_long", "end_at_boundary_p1"):
        b = built_case(name)
        blob = _bam_bytes(b.stream())
        tot, starts, err, cuts = R.pass_windows(blob, R.min_window(blob), b.first, len(b.targets))
        assert err is None and starts == b.record_offsets() and cuts > 0, name
        assert tot["segments"] >= spec(name)["segments"]


def _bam_bytes(u, block=R.BLOCK):
    return b"".join(R.pybam.bgzf_block(u[k:k + block], 1) for k in range(0, len(u), block)) + R.pybam.EOF_BLOCK


def _host_records(path, threads):
    from gencore_amd.bamio import BamFile
    f = BamFile(path, threads=threads)
    try:
        return f.batch()
    finally:
        f.close()


@pytest.mark.parametrize("name", CASES + sorted(R.DAMAGED))
def test_host_reader_returns_the_records_written(built, tmp_path, name):
    """BamFile (the host index of bamio.cpp) reads every case's file back record for record, at 1, 3 and 8 threads; damaged streams fail"""
    from gencore_amd.capi import GceError
    path = tmp_path / "in.bam"
    if name in R.DAMAGED:
        b, u = R.DAMAGED[name]()
        path.write_bytes(_bam_bytes(u))
        for t in (1, 3, 8):
            with pytest.raises(GceError):
                _host_records(path, t)
        return
    b = built_case(name)
    b.write_bam(path)
    reads = [r.d for _, r in b.reads]
    for t in (1, 3, 8):
        batch = _host_records(path, t)
        assert batch.n == len(reads)
        for f in ("tid", "pos", "flag", "mtid", "mpos", "isize", "mapq"):
            assert batch.core[f].tolist() == [r[f] for r in reads], (f, t)
        assert batch.core["l_qseq"].tolist() == [len(r["seq"]) for r in reads]
        assert [batch.qname_of(i) for i in range(batch.n)] == [r["qname"] for r in reads]
        assert all(batch.seq_of(i) == r["seq"] and batch.qual_of(i).tolist() == r["qual"] and batch.cigar_of(i) == r["cigar"] for i, r in enumerate(reads))
        assert batch.nm_type.tolist() == [ord(r["nm_type"]) if r["nm"] is not None else 0 for r in reads]
        assert np.where(batch.nm_type != 0, batch.nm, 0).tolist() == [r["nm"] if r["nm"] is not None else 0 for r in reads]
        mi = [bytes(batch.mi[int(o):]).split(b"\0")[0].decode() if int(o) != R.NONE else None for o in batch.mi_off]
        assert mi == [r.get("mi") for r in reads]


# ------------------------------------------------------------------------------------------------------------------------------- GPU
def _params(b):
    from gencore_amd.capi import default_params
    tl = np.asarray([ln for _, ln in b.targets], np.uint32)
    p = default_params(n_targets=len(tl), target_len=tl.ctypes.data)
    p._keep = tl
    return p


def _raw_index(lib, E, b, stream, path, gpu_inflate):
    """the stream through gce_raw_begin / gce_raw_push (three host pieces, cut inside records) or gce_raw_push_bgzf (the file's members)
    and gce_raw_finish: (status, n_records)"""
    lib.gce_raw_begin.argtypes = [C.c_void_p, C.c_size_t]
    lib.gce_raw_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    lib.gce_raw_push_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.gce_raw_finish.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_int64)]
    eng = E._h
    assert lib.gce_raw_begin(eng, len(stream)) == 0
    tk = C.c_int32()
    if gpu_inflate:
        blob = path.read_bytes()
        mem = R.bgzf_members(blob)
        piece = np.frombuffer(blob, np.uint8).copy()
        coff = np.array([m[0] for m in mem], np.uint64); cs = np.array([m[1] for m in mem], np.uint32); us = np.array([m[2] for m in mem], np.uint32)
        assert lib.gce_raw_push_bgzf(eng, piece.ctypes.data, len(piece), len(mem), coff.ctypes.data, cs.ctypes.data, us.ctypes.data, C.byref(tk)) == 0
        assert lib.gce_submit_wait(eng, tk.value) == 0
    else:
        data = np.frombuffer(stream, np.uint8).copy()
        cuts = [0, len(data) // 3 + 17, 2 * len(data) // 3 + 5, len(data)]
        for a, z in zip(cuts, cuts[1:]):
            assert lib.gce_raw_push(eng, data[a:].ctypes.data, z - a, C.byref(tk)) == 0
            assert lib.gce_submit_wait(eng, tk.value) == 0
    n = C.c_int64()
    rc = lib.gce_raw_finish(eng, b.first, len(b.targets), C.byref(n))
    return rc, n.value


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_raw_paths_index_every_case(built, tmp_path, name):
    """gce_raw_push and gce_raw_push_bgzf + gce_raw_finish: the host's record count, the spec's counters, and after gce_process the rows of
    run_stream on the host-read batch"""
    from gencore_amd import capi
    from gencore_amd.batch import table_from_rows
    from gencore_amd.engine import Engine, run_stream
    from parity_helpers import diff_results
    b = built_case(name)
    path = tmp_path / "in.bam"
    b.write_bam(path)
    stream = b.stream()
    batch = _host_records(path, 2)
    assert batch.n == len(b.reads)
    params = _params(b)
    want = run_stream(batch, params)
    lib = capi.load_library()
    expect = R.counters(spec(name))
    for gpu_inflate in (False, True):
        E = Engine(params)
        try:
            rc, n = _raw_index(lib, E, b, stream, path, gpu_inflate)
            assert rc == 0, (gpu_inflate, lib.gce_last_error(E._h))
            assert n == batch.n
            assert E.index_counters() == expect, gpu_inflate
            assert lib.gce_process(E._h) == 0, lib.gce_last_error(E._h)
            rows, pre, post = E.rows()
            for k in ("src", "kind", "qname_src", "nm_new", "fr", "rr", "mate"):
                assert np.array_equal(rows[k], want.rows[k]), (k, gpu_inflate)
            d = diff_results(batch, table_from_rows(batch, rows, pre, post), want)
            assert not d, d[:3]
        finally:
            E.close()


def _inflated(path):
    import gzip
    with open(path, "rb") as f:
        return gzip.decompress(f.read())


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_file_and_pass_runners_on_every_case(built, tmp_path, monkeypatch, name):
    """gce_run_bam gives gce_run_bam_hostcodec's bytes; gce_run_bam_passes with windows that end inside the long records gives the
    single-pass bytes and Stats at P = 1, 2, 3, and its window counters are the spec's over the same windows, once per read of the file"""
    from gencore_amd.bamio import run_bam, run_bam_depth, run_bam_passes
    from gencore_amd.engine import index_counters
    b = built_case(name)
    src = tmp_path / "in.bam"
    b.write_bam(src)
    r1 = run_bam(src, tmp_path / "gpu.bam", _params(b), threads=2)
    monkeypatch.setenv("GCE_BAM_HOSTCODEC", "1")
    r2 = run_bam(src, tmp_path / "host.bam", _params(b), threads=2)
    monkeypatch.delenv("GCE_BAM_HOSTCODEC")
    assert r1.n_reads == r2.n_reads == len(b.reads) and r1.n_out == r2.n_out
    assert bytes(r1.pre) == bytes(r2.pre) and bytes(r1.post) == bytes(r2.post)
    assert _inflated(tmp_path / "gpu.bam") == _inflated(tmp_path / "host.bam")

    one, dp1 = run_bam_depth(src, tmp_path / "one.bam", _params(b), [0], 1000, threads=2)
    window = R.min_window(src.read_bytes())                  # (one or a few BGZF members per window: window ends cut records)
    win, starts, err, cuts = R.pass_windows(src.read_bytes(), window, b.first, len(b.targets))
    assert err is None and starts == b.record_offsets() and cuts > 0
    for P in (1, 2, 3):
        kw = dict(device_budget_bytes=1 << 40) if P == 1 else dict(min_passes=P)
        r, dp, pr = run_bam_passes(src, tmp_path / ("p%d.bam" % P), _params(b), 0, 1000, threads=2, window_bytes=window, **kw)
        assert pr["n_passes"] == P and not pr["single_pass"]
        assert _inflated(tmp_path / ("p%d.bam" % P)) == _inflated(tmp_path / "one.bam"), P
        assert r.n_out == one.n_out and r.n_reads == one.n_reads and bytes(r.pre) == bytes(one.pre) and bytes(r.post) == bytes(one.post)
        assert dp["pre"] == dp1["pre"] and dp["post"] == dp1["post"]
        assert index_counters() == {k: v * (P + 1) for k, v in win.items()}, (P, win)       # the key pass and P passes read the file


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.DAMAGED))
def test_gpu_damaged_streams_are_refused(built, tmp_path, name):
    """a long record cut by the end of the stream, and a block_size below 32 behind a fake-laden record: gce_raw_finish refuses them with
    GCE_ERR_INVALID after the serial repair (the counters say so), and so do the file runner and the pass runner"""
    from gencore_amd import capi
    from gencore_amd.bamio import run_bam, run_bam_passes
    from gencore_amd.capi import GceError
    from gencore_amd.engine import Engine
    b, u = R.DAMAGED[name]()
    src = tmp_path / "in.bam"
    src.write_bytes(_bam_bytes(u))
    res = R.classify(u, b.first, len(b.targets), False)
    lib = capi.load_library()
    E = Engine(_params(b))
    try:
        for gpu_inflate in (False, True):
            rc, _ = _raw_index(lib, E, b, u, src, gpu_inflate)
            assert rc == -1, gpu_inflate
            assert b"damaged" in lib.gce_last_error(E._h)
            assert E.index_counters() == R.counters(res)
    finally:
        E.close()
    with pytest.raises(GceError) as ei:
        run_bam(src, tmp_path / "x.bam", _params(b), threads=2)
    assert ei.value.status == -1
    with pytest.raises(GceError) as ei:
        run_bam_passes(src, tmp_path / "y.bam", _params(b), 0, 1000, threads=2, window_bytes=R.min_window(src.read_bytes()), min_passes=2)
    assert ei.value.status == -1
