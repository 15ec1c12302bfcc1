"""gce_sam_parse on the GPU: SAM text lines into BAM records (gce_samdev.hpp).  The field edges are compared byte for byte with pybam's
independent model (samcases.case) and with the host's sam_to_bam; every malformed line gives the host's message and its index; a realistic
stream never touches the host parser."""
import numpy as np
import pytest

import pysort
import samcases

NAMES = [t[0] for t in samcases.TARGETS]
HEADER = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in samcases.TARGETS)


def parse(text, names=NAMES, **kw):
    from gencore_amd.bamio import parse_sam
    return parse_sam(text, names, **kw)


def host_records(tmp_path, text, header=HEADER):
    from gencore_amd.bamio import sam_to_bam
    (tmp_path / "h.sam").write_bytes(header + text)
    sam_to_bam(tmp_path / "h.sam", tmp_path / "h.bam", threads=3, level=1)
    return b"".join(pysort.records(tmp_path / "h.bam")[1])


@pytest.mark.gpu
def test_field_edges(built, tmp_path):
    cases = samcases.field_edge_cases()
    want = b"".join(k[1] for k in cases)
    text = samcases.text_of(cases)
    assert host_records(tmp_path, text) == want                    # the two references agree
    r = parse(text)
    assert r["n_records"] == len(cases) and r["n_host_lines"] == samcases.n_float_lines(cases) == 3
    if r["records"] != want:
        o = 0
        for k, c in enumerate(cases):
            assert r["records"][o:o + len(c[1])] == c[1], "case %d (%s)" % (k, c[0][:40])
            o += len(c[1])
    assert r["records"] == want
    # one line at a time as well: every record at offset 0, a window of one line
    for c in cases[:12]:
        assert parse(c[0].encode() + b"\n")["records"] == c[1]


@pytest.mark.gpu
def test_line_ends_and_empty_lines(built, tmp_path):
    cases = samcases.field_edge_cases()
    want = b"".join(k[1] for k in cases)
    r = parse(samcases.text_of(cases, newline="\r\n"))
    assert r["records"] == want and r["n_records"] == len(cases)
    lines = [k[0].encode() for k in cases]
    text = b"\n\n" + lines[0] + b"\n\r\n" + b"\n".join(lines[1:5]) + b"\n\n\n\r\n" + b"\n".join(lines[5:])       # no last line feed
    r = parse(text)
    assert r["records"] == want and r["n_records"] == len(cases)
    assert host_records(tmp_path, text) == want
    assert parse(lines[3] + b"\r")["records"] == cases[3][1]      # a last line that ends in a lone CR
    for empty in (b"", b"\n", b"\r\n\n"):
        assert parse(empty) == dict(records=b"", n_records=0, n_host_lines=0)


@pytest.mark.gpu
def test_output_buffer_too_small(built):
    from gencore_amd.capi import GceError
    c = samcases.field_edge_cases()[:4]
    want = b"".join(k[1] for k in c)
    with pytest.raises(GceError) as ei:
        parse(samcases.text_of(c), out_cap=len(want) - 1)
    assert ei.value.status == -4 and ei.value.needed == len(want) and ei.value.bad_line == -1
    assert parse(samcases.text_of(c), out_cap=len(want))["records"] == want


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(samcases.malformed_cases())))
def test_malformed_line(built, tmp_path, k):
    from gencore_amd.bamio import sam_to_bam
    from gencore_amd.capi import GceError
    msg, line = samcases.malformed_cases()[k]
    other = samcases.malformed_cases()[(k + 5) % len(samcases.malformed_cases())]
    good = [samcases.GOOD.replace("g\t", "g%d\t" % i).replace("\t100\t", "\t%d\t" % (100 + i)) for i in range(100)]
    text = ("\n".join(good) + "\n\n" + line + "\n" + other[1] + "\n" + good[0] + "\n").encode()
    with pytest.raises(GceError) as ei:
        parse(text)
    assert ei.value.status == -1 and ei.value.bad_line == 100, str(ei.value)
    assert str(ei.value).endswith(": " + msg) and (other[0] == msg or other[0] not in str(ei.value))
    (tmp_path / "m.sam").write_bytes(HEADER + text)
    with pytest.raises(GceError) as eh:
        sam_to_bam(tmp_path / "m.sam", tmp_path / "m.bam", threads=1, level=1)
    assert str(eh.value) == str(ei.value)                          # the message is the host's


@pytest.fixture(scope="module")
def realistic(built, tmp_path_factory):
    """5000 records from synth (cfg3 pairs with UMIs) as SAM text: (directory, header bytes, alignment lines, contig names)"""
    from gencore_amd import synth
    from gencore_amd.bamio import bam_to_sam, write_batch_as_bam
    d = tmp_path_factory.mktemp("samdev")
    s = synth.generate("cfg3", n_pairs=2500, scale=0.002)
    tl = np.asarray(s.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(str(d / "s.bam"), s.to_batch(), tl, names, threads=4)
    bam_to_sam(d / "s.bam", d / "s.sam", threads=4)
    raw = (d / "s.sam").read_bytes()
    lines = raw.split(b"\n")
    head = [l for l in lines if l.startswith(b"@")]
    body = [l for l in lines if l and not l.startswith(b"@")][:5000]      # (synth adds a few reads beyond the pairs asked for)
    (d / "s.sam").write_bytes(b"".join(l + b"\n" for l in head + body))
    return d, b"".join(l + b"\n" for l in head), body, names


@pytest.mark.gpu
def test_realistic_stream(realistic):
    d, head, body, names = realistic
    from gencore_amd.bamio import sam_to_bam
    assert len(body) == 5000
    sam_to_bam(d / "s.sam", d / "h.bam", threads=4, level=1)
    want = b"".join(pysort.records(d / "h.bam")[1])
    assert len(want) > 5000 * 300
    r = parse(b"".join(l + b"\n" for l in body), names)
    assert r["n_records"] == 5000 and r["records"] == want
    assert r["n_host_lines"] == 0                                  # no floating-point tags: the host parser stays out of the ordinary path
