"""gce_bam_sort_passes on the GPU (gencore_amd/csrc/gce_sort.hpp): sorted in output-range passes, a file gives the bytes
gce_bam_sort gives in-core, and its inflated stream is the pure-Python model's (tests/pysort.py), whatever the number of passes, the window
and the level; a record that straddles a cut is written partly by each pass it touches, one that covers a whole pass included; under a
device budget of half the in-core peak the passes stay below it; the refusals are gce_bam_sort's and leave nothing behind.

The window sizes follow tests/test_sort_gpu.py: a window holds whole BGZF members, so the small window is 2000 compressed bytes for
members of 300 input bytes and 70 000 for members of 0xff00."""
import random

import pytest

import pybam
import pysort
from test_bai_model import header, rec
from test_sort_gpu import FORMULA, leftovers, stream1, write_members
from test_sort_model import TARGETS, shuffled_records

M = 0xff00
FORMULA_PASSES = "8 bytes per record + one window + one pass of at least one BGZF member"


def cuts_of(total, min_passes):
    """(pass_bytes, n_passes) of gce_bam_sort_passes without a budget in the way"""
    P = max(min_passes, 1)
    pb = (-(-total // P) + M - 1) // M * M
    return pb, (-(-total // pb) if pb else 0)


def in_core(path, out, window_bytes=0, level=-2, budget=0):
    from gencore_amd.bamio import sort_bam
    return sort_bam(str(path), str(out), device=0, threads=4, level=level, window_bytes=window_bytes, device_budget_bytes=budget)


def passes(path, out, window_bytes=0, level=-2, budget=0, min_passes=0):
    from gencore_amd.bamio import sort_bam_passes
    return sort_bam_passes(str(path), str(out), device=0, threads=4, level=level, window_bytes=window_bytes, device_budget_bytes=budget, min_passes=min_passes)


class Model:
    """the model's sort of one file and the in-core sort's output per level, computed once"""

    def __init__(self, path):
        self.path, self.before = path, path.read_bytes()
        self.hdr, self.recs = pysort.sort_model(path)
        self.desc = pysort.descents(path)
        self.total = sum(len(r) for r in self.recs)
        self.ref = {}

    def in_core_bytes(self, level):
        if level not in self.ref:
            out = self.path.parent / (self.path.name + ".incore%d.bam" % level)
            in_core(self.path, out, level=level)
            self.ref[level] = out.read_bytes()
            out.unlink()
        return self.ref[level]

    def straddled(self, pass_bytes):
        """every cut lies inside a record (not between two)"""
        ends, p = set(), 0
        for r in self.recs:
            p += len(r)
            ends.add(p)
        return all(c not in ends for c in range(pass_bytes, self.total, pass_bytes))

    def check(self, min_passes, windows=(0,), levels=(-2,), straddle=True):
        pb, n_passes = cuts_of(self.total, min_passes)
        assert n_passes >= 2 or min_passes < 2 or self.total <= M
        if straddle and n_passes >= 2:
            assert self.straddled(pb)
        out = self.path.parent / (self.path.name + ".passes.bam")
        for w in windows:
            for lv in levels:
                if out.exists():
                    out.unlink()
                r = passes(self.path, out, w, lv, min_passes=min_passes)
                what = "min_passes=%d window_bytes=%d level=%d" % (min_passes, w, lv)
                blob = out.read_bytes()
                assert blob == self.in_core_bytes(lv), what
                u = pysort.inflate(blob)
                assert u == self.hdr + b"".join(self.recs), what
                assert (r["n_passes"], r["pass_bytes"]) == (n_passes, pb), what
                assert r["in_core"] == (1 if min_passes <= 1 else 0) and len(r["pass_s"]) == n_passes, what
                assert (r["n_records"], r["n_no_coor"], r["n_descents"]) == (len(self.recs), pysort.n_unplaced(self.recs), self.desc), what
                assert r["inflated_bytes"] == self.total and r["out_bytes"] == len(blob), what
                assert self.path.read_bytes() == self.before
                assert leftovers(self.path.parent) == []
        return out


@pytest.fixture(scope="module")
def streams(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("sortpasses")
    ms = {}
    for block in (300, 0xff00):
        path = d / ("r%d.bam" % block)
        pybam.write_bam(str(path), stream1(block), TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=block, level=1)
        ms[block] = Model(path)
        assert ms[block].total > 2 * M and ms[block].desc > 100
    return ms


@pytest.mark.gpu
@pytest.mark.parametrize("min_passes", [1, 2, 3, 5])
@pytest.mark.parametrize("block", [300, 0xff00])
def test_equal_to_the_in_core_sort_and_the_model(streams, block, min_passes):
    m = streams[block]
    if min_passes >= 2:
        assert cuts_of(m.total, min_passes)[1] >= 2
    m.check(min_passes, windows=(0, 2000) if block < 0xff00 else (0, 70000), levels=(-2, 1))


@pytest.mark.gpu
def test_other_levels(streams):
    streams[300].check(3, windows=(2000,), levels=(-3, -1))


@pytest.mark.gpu
def test_a_record_that_covers_a_whole_pass(built, tmp_path):
    """tests/test_sort_gpu.py::test_record_sizes' family (every record size mod 16 from 38 bytes up, reverse-sorted) with its read of 70 000
    bases between enough small records that the sorted stream has three members and the big record begins in member 0 and ends in member 2:
    with three passes of one member each, pass 1 is a stretch from the record's interior, passes 0 and 2 take its clipped head and tail."""
    rng = random.Random(16)
    recs, k = [], 0
    for L in (0, 1, 10, 33, 150):
        for nl in range(1, 17):
            r = rec(k, 0, 100 + 7 * k, "%dM" % L if L else "*", flag=16 if k % 3 == 0 else 0, L=L)
            r["qname"] = "".join(rng.choice("abcdefgh") for _ in range(nl))
            recs.append(r)
            k += 1
    big = rec(k, 0, 100 + 7 * 40 + 3, "70000M", L=70000)
    big["seq"] = "".join(rng.choice("ACGT") for _ in range(70000))
    big["qual"] = [rng.randrange(41) for _ in range(70000)]
    recs.append(big)
    recs += [rec(1000 + i, 0, i % 100, "50M", flag=16 * (i % 2), L=50) for i in range(300)]             # in front of the family in rule S's order
    recs += [rec(2000 + i, 1, 5 * i, "50M", L=50) for i in range(100)]                                   # behind it
    sizes = [len(pybam.record_bytes(r)) for r in recs]
    assert min(sizes) == 38 and max(sizes) >= 100000 and {s % 16 for s in sizes} == set(range(16))
    recs.sort(key=lambda r: (-r["tid"], -r["pos"]))
    path = tmp_path / "big.bam"
    pybam.write_bam(str(path), recs, TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=16000, level=1)
    m = Model(path)
    assert m.desc > len(recs) // 2
    at = 0
    for r in m.recs:
        if len(r) >= 100000:
            break
        at += len(r)
    assert 2 * M < m.total <= 3 * M and at < M and at + len(r) > 2 * M
    assert cuts_of(m.total, 3) == (M, 3)
    m.check(3, windows=(0, 20000))


@pytest.mark.gpu
def test_order_edges_and_members(built, tmp_path):
    rng = random.Random(3)
    cases = {
        "sorted": [rec(i, i // 200, 10 * (i % 200), "20M", flag=16 * (i % 2)) for i in range(600)] + [rec(600 + k, -1, -1, "*", flag=4) for k in range(5)],
        "stable": [rec(i, 1, 777, "30M", flag=16, L=30) for i in range(1000)],
        "reversed": [rec(i, 3 - i // 200, 4000 - 5 * (i % 200), "20M") for i in range(800)],
        "header_only": [],
        "one": [rec(0, 2, 12345, "100M", L=100)],
        "unplaced": [rec(k, -1, rng.choice([-1, 5, 99]), "*", flag=4 | (16 if k % 2 else 0)) for k in range(300)],
    }
    for name, recs in cases.items():
        path = tmp_path / (name + ".bam")
        pybam.write_bam(str(path), recs, TARGETS, block=500 if name != "header_only" else 0xff00, level=1)
        m = Model(path)
        out = m.check(2, windows=(0, 3000), straddle=False)          # (below two members the formula gives one pass, none for header_only: check compares)
        got = pysort.records(out)[1]
        if name in ("sorted", "stable"):
            assert m.desc == 0 and got == pysort.records(path)[1]
        if name == "reversed":
            assert got == pysort.records(path)[1][::-1]
        if name == "header_only":
            assert cuts_of(m.total, 2) == (0, 0) and got == [] and out.read_bytes().endswith(pybam.EOF_BLOCK)
    recs = [rec(0, 2, 40000, "5M"), rec(1, -1, -1, "*", flag=4), rec(2, 0, 16384, "10M"), rec(3, 0, 10, "60M", flag=16), rec(4, 2, 7, "30M"), rec(5, 0, 10, "50M"),
            rec(6, -1, -1, "*", flag=4), rec(7, 0, 16390, "*", flag=4)]
    h = header(TARGETS, text="@SQ\tSN:a\tLN:300000\n")
    body = [pybam.record_bytes(r) for r in recs]
    stream = h + b"".join(body)
    cuts = [len(h)]
    for b in body[:-1]:
        cuts.append(cuts[-1] + len(b))
    for k, (cs, empty) in enumerate([(cuts, ()), (cuts, (1, 3, 4, 8)), (cuts[1:], (2,)), (cuts[:1] + cuts[2:5], (0, 1))]):
        path = tmp_path / ("m%d.bam" % k)
        write_members(str(path), stream, cs, empty)
        m = Model(path)
        assert cuts_of(m.total, 2) == (M, 1)
        m.check(2, windows=(0, 200), straddle=False)


@pytest.mark.gpu
def test_budget(built, tmp_path, streams):
    """The in-core peak P0 of an unbudgeted run is the reference point: under P0 // 2 the in-core sort refuses, the passes succeed below the
    budget with the same bytes.  The floor of the passes here (the destinations, one window of 20 000 compressed bytes, the scan's scratch):
    DESIGN.md 4d."""
    from gencore_amd.capi import GceError
    path, ref, out = tmp_path / "b.bam", tmp_path / "ref.bam", tmp_path / "out.bam"
    pybam.write_bam(str(path), shuffled_records(random.Random(44), TARGETS, 20000), TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=16000, level=1)
    before = path.read_bytes()
    p0 = in_core(path, ref, 20000, 1)["peak_device_bytes"]
    want = ref.read_bytes()
    budget = p0 // 2
    with pytest.raises(GceError) as ei:
        in_core(path, out, 20000, 1, budget=budget)
    assert ei.value.status == -4 and FORMULA in str(ei.value) and not out.exists() and leftovers(tmp_path) == []
    r = passes(path, out, 20000, 1, budget=budget)
    print("in-core peak %d, budget %d, passes: n_passes %d pass_bytes %d resident %d peak %d" % (p0, budget, r["n_passes"], r["pass_bytes"], r["resident_bytes"], r["peak_device_bytes"]))
    assert r["in_core"] == 0 and r["n_passes"] >= 2
    assert r["peak_device_bytes"] <= budget
    assert out.read_bytes() == want and path.read_bytes() == before and leftovers(tmp_path) == []
    out.unlink()
    with pytest.raises(GceError) as ei:
        passes(path, out, 20000, 1, budget=1 << 16)
    assert ei.value.status == -4 and FORMULA_PASSES in str(ei.value) and FORMULA not in str(ei.value), str(ei.value)
    assert not out.exists() and leftovers(tmp_path) == []
    m = streams[300]
    r = passes(m.path, out, 0, -2)
    assert r["in_core"] == 1 and out.read_bytes() == m.in_core_bytes(-2)


@pytest.mark.gpu
def test_refusals(built, tmp_path):
    import gzip
    import struct
    from gencore_amd.capi import GceError
    good = tmp_path / "good.bam"
    pybam.write_bam(str(good), stream1(300), TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=300, level=1)
    blob = good.read_bytes()
    bounds, p = [], 0
    while p < len(blob):
        bounds.append(p)
        p += struct.unpack_from("<H", blob, p + 16)[0] + 1
    bad_tid = [rec(i, i % 2, 1000 - i, "10M") for i in range(40)]
    bad_tid[7]["tid"] = 2
    bad_tid[30]["tid"] = 9
    pybam.write_bam(str(tmp_path / "tid.bam"), bad_tid, TARGETS[:2], block=400, level=1)
    (tmp_path / "cut.bam").write_bytes(blob[:bounds[len(bounds) // 2] + 9])
    (tmp_path / "gz.bam").write_bytes(gzip.compress(b"BAM\1" + bytes(100)))
    (tmp_path / "text.sam").write_text("@HD\tVN:1.6\n@SQ\tSN:a\tLN:300000\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    cases = [("tid.bam", -1, "record 7 "), ("cut.bam", -1, "truncated"), ("gz.bam", -1, "not a BGZF file"), ("text.sam", -1, "gce_bam_sort reads BAM, not SAM text")]
    for name, status, words in cases:
        src = tmp_path / name
        before = src.read_bytes()
        for w in (0, 1500):
            with pytest.raises(GceError) as ei:
                passes(src, tmp_path / "out.bam", w, min_passes=2)
            assert ei.value.status == status and words in str(ei.value), str(ei.value)
            assert not (tmp_path / "out.bam").exists() and leftovers(tmp_path) == []
        assert src.read_bytes() == before
    for same in (str(good), str(tmp_path) + "/./good.bam", str(tmp_path) + "/../" + tmp_path.name + "/good.bam"):
        with pytest.raises(GceError) as ei:
            passes(good, same, min_passes=2)
        assert ei.value.status == -1 and "input" in str(ei.value)
        assert good.read_bytes() == blob and leftovers(tmp_path) == []
    link = tmp_path / "link.bam"
    link.symlink_to(good)
    with pytest.raises(GceError):
        passes(good, link, min_passes=2)
    assert good.read_bytes() == blob and leftovers(tmp_path) == []
    out = tmp_path / "out.bam"
    passes(good, out, min_passes=2)                                # and the file every refusal left alone still sorts
    h, rs = pysort.sort_model(good)
    assert pysort.inflate(out.read_bytes()) == h + b"".join(rs)
