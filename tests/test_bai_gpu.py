"""gce_bam_index on the GPU (gencore_amd/csrc/gce_bai.hpp): the .bai it writes equals the bytes of the pure-Python model (tests/pybai.py) on
streams built to hit the rules' edges, at the default window and at windows small enough that records straddle them; its refusals name the
record and leave no index; and `python -m gencore_amd ... --index` indexes the output of every runner path (single pass, sharded, passes) so
that region queries through the index find what brute force finds."""
import random
import struct

import pytest

import pybai
import pybam
from test_bai_model import header, random_records, rec


def index(path, window_bytes=0):
    from gencore_amd.bamio import index_bam
    return index_bam(str(path), str(path) + ".bai", device=0, threads=4, window_bytes=window_bytes)


def check(path, windows=(0,)):
    want = pybai.build(path)
    n_ref, contigs, n_no_coor = pybai.parse_bai(want)
    for w in windows:
        r = index(path, w)
        got = open(str(path) + ".bai", "rb").read()
        assert got == want, "window_bytes=%d" % w
        assert r["n_no_coor"] == n_no_coor and r["n_ref"] == n_ref
        assert r["n_bins"] == sum(len(c["bins"]) for c in contigs)
        assert r["n_chunks"] == sum(len(x) for c in contigs for x in c["bins"].values())
        assert r["n_intervals"] == sum(len(c["intervals"]) for c in contigs)
    return want


def write_members(path, stream, cuts, empty_at=()):
    """stream cut at `cuts` into BGZF members; an empty member in front of member k for k in empty_at"""
    with open(path, "wb") as f:
        for k, (a, z) in enumerate(zip([0] + list(cuts), list(cuts) + [len(stream)])):
            if k in empty_at:
                f.write(pybam.bgzf_block(b""))
            f.write(pybam.bgzf_block(stream[a:z]))
        f.write(pybam.EOF_BLOCK)


TARGETS = [("a", 300000), ("b", 2000), ("c", 200000), ("d", 5000), ("e", 1 << 29)]


@pytest.mark.gpu
@pytest.mark.parametrize("block", [0xff00, 300, 777])
def test_random_streams(built, tmp_path, block):
    rng = random.Random(block)
    path = tmp_path / "r.bam"
    pybam.write_bam(str(path), random_records(rng, TARGETS[:4], 3000), TARGETS[:4], block=block, level=1)
    check(path, windows=(0, 2000, 20000) if block < 0xff00 else (0, 70000))


@pytest.mark.gpu
def test_member_boundaries_and_empty_members(built, tmp_path):
    """every record its own member (records start and end exactly on boundaries), empty members in between, and the same stream with the
    header and the first record sharing a member"""
    recs = [rec(0, 0, 10, "50M"), rec(1, 0, 10, "60M"), rec(2, 0, 16384, "10M"), rec(3, 0, 16390, "*", flag=4), rec(4, 2, 7, "30M"), rec(5, 2, 40000, "5M"),
            rec(6, -1, -1, "*", flag=4), rec(7, -1, -1, "*", flag=4)]
    h = header(TARGETS[:4])
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
def test_edges(built, tmp_path):
    """empty contigs between used ones, placed unmapped records, a tid -1 tail, a long-N CIGAR over many 16 kb windows, a record that ends at
    2^29, one record, a header-only file"""
    cases = {
        "edges": [rec(0, 0, 5, "*", flag=4), rec(1, 0, 100, "20M"), rec(2, 0, 150, "20M600000N20M"), rec(3, 0, 200, "10M", flag=4), rec(4, 0, 70000, "10M"),
                  rec(5, 3, 1, "10M"), rec(6, 4, (1 << 29) - 10, "10M"), rec(7, -1, -1, "*", flag=4), rec(8, -1, 100, "*", flag=4)],
        "one": [rec(0, 2, 12345, "100M")],
        "one_unplaced": [rec(0, -1, -1, "*", flag=4)],
        "header_only": [],
    }
    targets = [("a", 1 << 20), ("b", 100), ("c", 20000), ("d", 5000), ("e", 1 << 29)]
    for name, recs in cases.items():
        for block in (0xff00, 150):
            path = tmp_path / ("%s_%d.bam" % (name, block))
            pybam.write_bam(str(path), recs, targets, block=block, level=1)
            check(path, windows=(0, 1000) if block < 0xff00 else (0,))


@pytest.mark.gpu
def test_errors_name_the_record(built, tmp_path):
    from gencore_amd.capi import GceError
    targets = [("a", 1 << 29), ("b", 10000)]
    good = [rec(i, 0, 100 * i, "10M") for i in range(200)] + [rec(200, 1, 5, "10M")]
    cases = [
        ("pos", good[:50] + [rec(50, 0, 10, "10M")] + good[51:], "record 50 "),
        ("tid", good[:1] + [rec(1, 1, 5, "10M"), rec(2, 0, 300, "10M")], "record 2 "),
        ("after_unplaced", good[:10] + [rec(10, -1, -1, "*", flag=4), rec(11, 1, 5, "10M")], "record 11 "),
        ("range", good[:3] + [rec(3, 0, (1 << 29) - 5, "10M")], "record 3 "),
    ]
    for name, recs, words in cases:
        path = tmp_path / (name + ".bam")
        pybam.write_bam(str(path), recs, targets, block=400, level=1)
        with pytest.raises(pybai.BaiError):
            pybai.build(path)
        before = path.read_bytes()
        for w in (0, 1500):
            with pytest.raises(GceError) as ei:
                index(path, w)
            assert ei.value.status == -1 and words in str(ei.value), str(ei.value)
            assert not (tmp_path / (name + ".bam.bai")).exists()
        assert path.read_bytes() == before
        assert [p.name for p in tmp_path.iterdir() if ".bai" in p.name] == []
    path = tmp_path / "trunc.bam"
    pybam.write_bam(str(path), good, targets, block=400, level=1)
    blob = path.read_bytes()
    for cut in (len(blob) // 2, len(blob) - 10, 30):
        tp = tmp_path / ("t%d.bam" % cut)
        tp.write_bytes(blob[:cut])
        with pytest.raises(GceError) as ei:
            index(tp)
        assert ei.value.status == -1 and "truncated" in str(ei.value), str(ei.value)
        assert not (tmp_path / ("t%d.bam.bai" % cut)).exists()
    nb = tmp_path / "plain.bam"
    nb.write_bytes(b"BAM\1" + bytes(100))
    with pytest.raises(GceError) as ei:
        index(nb)
    assert "not a BGZF file" in str(ei.value)
    assert not (tmp_path / "plain.bam.bai").exists()


def queries(bam, bai, targets, rng, n=25):
    recs = pybai.records(bam)[1]
    for _ in range(n):
        t = rng.randrange(len(targets))
        a = rng.randrange(0, targets[t][1])
        z = a + rng.choice([1, 300, 20000, 1000000])
        assert pybai.query(bam, bai, t, a, z, recs) == pybai.brute_force(bam, t, a, z, recs)


@pytest.mark.gpu
def test_cli_index_every_runner(built, tmp_path):
    from test_cli_gpu import cli
    from test_passes_gpu import inputs, params, passes
    d, _, targets = inputs(tmp_path, n_pairs=20000)
    base = ["-i", "in.bam", "-r", "ref.fa", "-b", "panel.bed", "--threads", "4", "-s", "2"]
    _, _, big = passes(tmp_path, params(d), "big.bam", device_budget_bytes=64 << 30)
    gb = (big["budget_bytes"] - big["pass_room"] + big["total_weight"] * 0.3) / (1 << 30)
    runs = {"l6": ["--level", "6"], "gpu": ["--level", "-2"], "sharded": ["--devices", "0,0"], "passes": ["--device_memory", "%.6f" % gb]}
    rng = random.Random(7)
    plain = cli(base + ["-o", "plain.bam", "-j", "plain.json"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    assert not (tmp_path / "plain.bam.bai").exists()
    for name, extra in runs.items():
        out = "%s.bam" % name
        r = cli(base + ["-o", out, "-j", name + ".json", "--index"] + extra, tmp_path)
        assert r.returncode == 0, r.stderr
        bam, bai = tmp_path / out, tmp_path / (out + ".bai")
        assert bai.read_bytes() == pybai.build(bam), name
        queries(bam, bai.read_bytes(), targets, rng)
        summ = lambda s: s.split("\ngencore ")[0]
        assert summ(r.stderr) == summ(plain.stderr)
    assert (tmp_path / "l6.bam").read_bytes() == (tmp_path / "plain.bam").read_bytes()
