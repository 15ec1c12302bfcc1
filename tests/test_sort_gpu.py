"""gce_bam_sort on the GPU (gencore_amd/csrc/gce_sort.hpp): the inflated bytes of its output equal the pure-Python model's
(tests/pysort.py: rule H's header, then the input's records, unchanged, in rule S's order) on shuffled streams, on records of every size
residue mod 16 from the smallest legal record to one larger than a BGZF member and a window, on the order's edges, on odd member layouts and
at every kind of compression level; its refusals name their reason and leave no output and no temporary file."""
import gzip
import random
import struct

import pytest

import pybai
import pybam
import pysort
from test_bai_model import header, rec
from test_sort_model import HEADER_CASES, TARGETS, shuffled_records

FORMULA = "2 x the inflated record bytes + 20 bytes per record + one window"


def sort(path, out, window_bytes=0, level=-2, budget=0):
    from gencore_amd.bamio import sort_bam
    return sort_bam(str(path), str(out), device=0, threads=4, level=level, window_bytes=window_bytes, device_budget_bytes=budget)


def leftovers(d):
    return sorted(p.name for p in d.iterdir() if ".tmp" in p.name)


def check(path, windows=(0,), levels=(-2,)):
    before = path.read_bytes()
    want_hdr, want = pysort.sort_model(path)
    desc = pysort.descents(path)
    out = path.parent / (path.name + ".sorted.bam")
    for w in windows:
        for lv in levels:
            if out.exists():
                out.unlink()
            r = sort(path, out, w, lv)
            blob = out.read_bytes()
            assert blob.endswith(pybam.EOF_BLOCK)
            u = pysort.inflate(blob)                              # plain zlib, member by member
            assert u[:len(want_hdr)] == want_hdr, "window_bytes=%d level=%d" % (w, lv)
            hdr, got = pysort.split(u)
            assert pysort.header_bytes(hdr) == want_hdr and hdr["text"] == pysort.header_text(hdr["text"])
            assert len(got) == len(want)
            assert got == want, "window_bytes=%d level=%d: first difference at record %d" % (w, lv, next(k for k, (a, b) in enumerate(zip(got, want)) if a != b))
            assert (r["n_records"], r["n_no_coor"], r["n_descents"]) == (len(want), pysort.n_unplaced(want), desc)
            assert r["inflated_bytes"] == sum(len(x) for x in want) and r["out_bytes"] == len(blob)
            assert path.read_bytes() == before
            assert leftovers(path.parent) == []
    return out


def stream1(block):
    rng = random.Random(block)
    return shuffled_records(rng, TARGETS, 3000)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [0xff00, 300, 777])
def test_random_streams(built, tmp_path, block):
    path = tmp_path / "r.bam"
    pybam.write_bam(str(path), stream1(block), TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=block, level=1)
    assert pysort.descents(path) > 100
    check(path, windows=(0, 2000, 20000) if block < 0xff00 else (0, 70000))


@pytest.mark.gpu
def test_record_sizes(built, tmp_path):
    """16 consecutive name lengths against fixed sequence lengths: every record size mod 16, from the smallest legal record (38 bytes: a
    1-character name, no CIGAR, no bases) up; one read of 70 000 random bases (> 100 000 bytes: larger than a BGZF member and than the
    20 000-byte window: it spans seven members and several windows).  Reverse-sorted, so every record moves and source and destination alignments are unrelated."""
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
    sizes = [len(pybam.record_bytes(r)) for r in recs]
    assert min(sizes) == 38 and max(sizes) >= 100000 and {s % 16 for s in sizes} == set(range(16))
    recs.sort(key=lambda r: -r["pos"])
    path = tmp_path / "sizes.bam"
    # (members of 16 000 input bytes: a window holds whole members, so each must fit in the 20 000 compressed bytes; the big read spans seven)
    pybam.write_bam(str(path), recs, TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=16000, level=1)
    assert pysort.descents(path) == len(recs) - 1
    check(path, windows=(0, 20000))


@pytest.mark.gpu
def test_order_edges(built, tmp_path):
    rng = random.Random(3)
    srt = [rec(i, i // 200, 10 * (i % 200), "20M", flag=16 * (i % 2)) for i in range(600)] + [rec(600 + k, -1, -1, "*", flag=4) for k in range(5)]
    same = [rec(i, 1, 777, "30M", flag=16, L=30) for i in range(1000)]
    cases = {
        "sorted": srt,
        "stable": same,
        "reversed": [rec(i, 3 - i // 200, 4000 - 5 * (i % 200), "20M") for i in range(800)],
        "header_only": [],
        "one": [rec(0, 2, 12345, "100M", L=100)],
        "unplaced": [rec(k, -1, rng.choice([-1, 5, 99]), "*", flag=4 | (16 if k % 2 else 0)) for k in range(300)],
    }
    for name, recs in cases.items():
        path = tmp_path / (name + ".bam")
        pybam.write_bam(str(path), recs, TARGETS, block=500 if name != "header_only" else 0xff00, level=1)
        out = check(path, windows=(0, 3000))
        got = pysort.records(out)[1]
        if name in ("sorted", "stable"):                          # n_descents == 0 (check compared it with the model's), records in input order
            assert pysort.descents(path) == 0 and got == pysort.records(path)[1]
        if name == "reversed":
            assert pysort.descents(path) == len(recs) - 1 and got == pysort.records(path)[1][::-1]


@pytest.mark.gpu
def test_rule_h(built, tmp_path):
    """the header rewrite of the library against the model's on every header case of tests/test_sort_model.py (@HD with and without SO, no
    @HD, NUL padding, an empty text, an @HD line without a newline, SO: on a later line only)"""
    for k, (text, want) in enumerate(HEADER_CASES):
        path = tmp_path / ("h%d.bam" % k)
        pybam.write_bam(str(path), [rec(1, 1, 5, "10M"), rec(0, 0, 5, "10M")], TARGETS[:2], text=text, block=200, level=1)
        out = check(path, windows=(0, 150))
        assert pysort.records(out)[0]["text"] == want.encode()


def write_members(path, stream, cuts, empty_at=()):
    """stream cut at `cuts` into BGZF members; an empty member in front of member k for k in empty_at"""
    with open(path, "wb") as f:
        for k, (a, z) in enumerate(zip([0] + list(cuts), list(cuts) + [len(stream)])):
            if k in empty_at:
                f.write(pybam.bgzf_block(b""))
            f.write(pybam.bgzf_block(stream[a:z]))
        f.write(pybam.EOF_BLOCK)


@pytest.mark.gpu
def test_members(built, tmp_path):
    """every record its own member, empty members in between, and the header and the first record sharing a member"""
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
        check(path, windows=(0, 200))


@pytest.mark.gpu
def test_levels(built, tmp_path):
    from gencore_amd.bamio import index_bam
    path = tmp_path / "r.bam"
    pybam.write_bam(str(path), stream1(777), TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=777, level=1)
    sizes = {}
    for lv in (-3, -2, -1, 1, 6):
        out = check(path, windows=(0,), levels=(lv,))
        sizes[lv] = out.stat().st_size
        if lv == -2:
            index_bam(str(out), str(out) + ".bai", device=0, threads=4)
            assert (tmp_path / (out.name + ".bai")).read_bytes() == pybai.build(out)
    assert sizes[-3] <= sizes[-2]


@pytest.mark.gpu
def test_refusals(built, tmp_path):
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
    with pytest.raises(pysort.SortError):
        pysort.sort_model(tmp_path / "tid.bam")
    cases = [("tid.bam", -1, "record 7 ", 0), ("cut.bam", -1, "truncated", 0), ("gz.bam", -1, "not a BGZF file", 0), ("text.sam", -1, "gce_bam_sort reads BAM, not SAM text", 0),
             ("good.bam", -4, FORMULA, 1 << 16)]
    for name, status, words, budget in cases:
        src = tmp_path / name
        before = src.read_bytes()
        for w in (0, 1500):
            with pytest.raises(GceError) as ei:
                sort(src, tmp_path / "out.bam", w, budget=budget)
            assert ei.value.status == status and words in str(ei.value), str(ei.value)
            assert not (tmp_path / "out.bam").exists() and leftovers(tmp_path) == []
        assert src.read_bytes() == before
    for same in (str(good), str(tmp_path) + "/./good.bam", str(tmp_path) + "/../" + tmp_path.name + "/good.bam"):
        with pytest.raises(GceError) as ei:
            sort(good, same)
        assert ei.value.status == -1 and "input" in str(ei.value)
        assert good.read_bytes() == blob and leftovers(tmp_path) == []
    link = tmp_path / "link.bam"
    link.symlink_to(good)
    with pytest.raises(GceError):
        sort(good, link)
    assert good.read_bytes() == blob and leftovers(tmp_path) == []
    check(good)                                                   # and the file every refusal left alone still sorts
