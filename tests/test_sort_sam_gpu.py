"""gce_sam_sort on the GPU: SAM text in any order into the coordinate-sorted BAM.  The defining property: the file it writes is, byte for byte,
the file gce_sam_to_bam + gce_bam_sort write -- for every level, and for windows that cut lines or are smaller than one."""
import json
import random

import pytest

import pysort
import samcases
from test_cli_sort_gpu import cli, inputs  # noqa: F401 (the fixture)
from test_samdev_gpu import realistic  # noqa: F401 (the fixture)
from test_sort_gpu import leftovers

UNPLACED = "u%d\t77\t*\t0\t0\t*\t*\t0\t0\tACGTACGTAC\tFFFFFFFFFF\tRG:Z:x"


def sort_sam(path, out, window_bytes=0, level=-2, budget=0):
    from gencore_amd.bamio import sort_sam as f
    return f(str(path), str(out), device=0, threads=4, level=level, window_bytes=window_bytes, device_budget_bytes=budget)


def composition(path, out, level=-2):
    from gencore_amd.bamio import sam_to_bam, sort_bam
    t = out.parent / (out.name + ".t.bam")
    sam_to_bam(path, t, threads=4, level=1)
    r = sort_bam(str(t), str(out), device=0, threads=4, level=level)
    return t, r


@pytest.fixture(scope="module")
def shuffled(realistic):  # noqa: F811
    """the 5000-record stream shuffled, unplaced reads and a POS 0 read (pos -1) on a known contig mixed in"""
    d, head, body, names = realistic
    lines = list(body) + [(UNPLACED % i).encode() for i in range(40)] + [b"p0\t0\tchr1\t0\t9\t4M\t=\t0\t0\tACGT\tFFFF"]
    random.Random(5).shuffle(lines)
    path = d / "shuffled.sam"
    path.write_bytes(head.replace(b"SO:coordinate", b"SO:unsorted") + b"".join(l + b"\n" for l in lines))
    return path, len(lines)


@pytest.mark.gpu
def test_defining_property(shuffled, tmp_path):
    path, n = shuffled
    before = path.read_bytes()
    for level in (1, -2, -3):
        ref = tmp_path / ("ref%d.bam" % level)
        t, rr = composition(path, ref, level)
        want = ref.read_bytes()
        for w in (0, 4096, 300):
            out = tmp_path / "out.bam"
            r = sort_sam(path, out, w, level)
            assert out.read_bytes() == want, "level %d window_bytes %d" % (level, w)
            assert r["n_host_lines"] == 0 and r["n_records"] == n == rr["n_records"]
            assert [r[k] for k in ("n_no_coor", "n_descents", "inflated_bytes", "out_bytes", "n_ref")] == [rr[k] for k in ("n_no_coor", "n_descents", "inflated_bytes", "out_bytes", "n_ref")]
            assert leftovers(tmp_path) == [] and path.read_bytes() == before
            out.unlink()
        if level == -2:                                            # and the model of the rules, on the inflated stream
            h, recs = pysort.sort_model(t)
            assert pysort.inflate(want) == h + b"".join(recs) and pysort.descents(t) > n // 8


HEADERS = ["@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:500000\n@PG\tID:x\n", "@HD\tVN:1.5\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:500000\n",
           "@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:500000\n", "@HD\tVN:1.6\tSO:queryname\n@CO\tno contigs\n", ""]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(HEADERS) + 1))
def test_header_cases(built, tmp_path, k):
    rng = random.Random(k)
    lines = [samcases.GOOD.replace("g\t", "g%d\t" % i).replace("chr1", rng.choice(["chr1", "chr2"])).replace("\t100\t", "\t%d\t" % rng.randrange(1, 400000)) for i in range(300)]
    text = HEADERS[k] if k < len(HEADERS) else HEADERS[0]
    body = "" if k == len(HEADERS) else "".join(l + "\n" for l in lines)      # the last case: no alignment lines
    path, ref, out = tmp_path / "h.sam", tmp_path / "ref.bam", tmp_path / "out.bam"
    path.write_text(text + body)
    _, rr = composition(path, ref)
    for w in (0, 50):
        r = sort_sam(path, out, w)
        assert out.read_bytes() == ref.read_bytes(), "header case %d window_bytes %d" % (k, w)
        assert r["n_records"] == rr["n_records"] and r["n_no_coor"] == rr["n_no_coor"]
        out.unlink()
    if "@SQ" not in text and body:
        assert rr["n_no_coor"] == 300                              # no contig table: every read is unplaced, as the composition gives
    hdr = pysort.split(pysort.inflate(ref.read_bytes()))[0]
    assert b"SO:coordinate" in hdr["text"]


@pytest.mark.gpu
def test_failures(shuffled, tmp_path):
    from gencore_amd.bamio import sam_to_bam
    from gencore_amd.capi import GceError
    path, n = shuffled
    out = tmp_path / "out.bam"
    raw = path.read_bytes().split(b"\n")
    n_head = sum(1 for l in raw if l.startswith(b"@"))
    msg, line = samcases.malformed_cases()[7]
    bad = tmp_path / "bad.sam"
    bad.write_bytes(b"\n".join(raw[:n_head + 2000]) + b"\n\n" + line.encode() + b"\n" + samcases.malformed_cases()[2][1].encode() + b"\n" + b"\n".join(raw[n_head + 2000:]))
    with pytest.raises(GceError) as eh:
        sam_to_bam(bad, tmp_path / "t.bam", threads=1, level=1)
    for w in (0, 5000):
        with pytest.raises(GceError) as ei:
            sort_sam(bad, out, w)
        assert ei.value.status == -1 and str(ei.value) == str(eh.value) + " (line %d)" % (n_head + 2000 + 2), str(ei.value)
        assert not out.exists() and leftovers(tmp_path) == []
    sorted_bam = tmp_path / "ref.bam"
    composition(path, sorted_bam)
    with pytest.raises(GceError) as ei:
        sort_sam(sorted_bam, out)
    assert ei.value.status == -1 and "gce_sam_sort reads SAM text, not BAM" in str(ei.value) and not out.exists()
    before = path.read_bytes()
    for same in (str(path), str(path.parent) + "/./" + path.name):
        with pytest.raises(GceError) as ei:
            sort_sam(path, same)
        assert ei.value.status == -1 and "input" in str(ei.value) and path.read_bytes() == before
    assert leftovers(path.parent) == []
    p0 = sort_sam(path, out, 4096)["peak_device_bytes"]
    out.unlink()
    print("in-core peak of sort_sam %d, budget %d" % (p0, p0 // 2))
    with pytest.raises(GceError) as ei:
        sort_sam(path, out, 4096, budget=p0 // 2)
    assert ei.value.status == -4 and "gce_bam_sort_passes" in str(ei.value) and "gce_sam_to_bam" in str(ei.value), str(ei.value)
    assert not out.exists() and leftovers(tmp_path) == []
    assert sort_sam(path, out, 4096, budget=p0 + (1 << 20))["n_records"] == n


@pytest.mark.gpu
def test_command_line(inputs):  # noqa: F811
    """-i U.sam --sort_sam gives the records and the report that the model's sorted BAM of the same reads (MS.bam) gives without the flag"""
    from gencore_amd.bamio import bam_to_sam
    d = inputs
    from gencore_amd.bamio import sam_to_bam
    bam_to_sam(d / "U.bam", d / "U.sam", threads=4)
    sam_to_bam(d / "U.sam", d / "T.bam", threads=4, level=1)       # the same reads as BAM (text gives every record its bin), sorted by the model
    mh, mrecs = pysort.sort_model(d / "T.bam")
    pysort.write(d / "MS.bam", mh, mrecs)
    base = ["-r", "ref.fa", "-s", "2", "--threads", "4"]
    a = cli(["-i", "U.sam", "--sort_sam", "-o", "sa.bam", "-j", "sa.json"] + base, d)
    assert a.returncode == 0, a.stderr
    b = cli(["-i", "MS.bam", "-o", "sb.bam", "-j", "sb.json"] + base, d)
    assert b.returncode == 0, b.stderr
    ra, rb = pysort.records(d / "sa.bam")[1], pysort.records(d / "sb.bam")[1]
    assert len(ra) > 0 and ra == rb
    ja, jb = json.loads((d / "sa.json").read_text()), json.loads((d / "sb.json").read_text())
    assert "--sort_sam" in ja.pop("command") and "--sort" not in jb.pop("command")
    assert ja == jb
    assert [p.name for p in d.iterdir() if ".tmp" in p.name or p.name.startswith("gencore_sort_")] == []
