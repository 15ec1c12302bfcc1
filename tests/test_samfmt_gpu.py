"""gce_sam_format on the GPU: BAM records into SAM lines (gce_samfmt.hpp), and the file runners that write a `.sam` output with it at levels
-2 / -3.  The field edges and the hand-built records are compared byte for byte with the host's bam_to_sam, with the independent model of
samfmtcases.line_of and, where pybam can express the record, with pybam.sam_line; every refused record gives its index and leaves the output
alone; a realistic stream never touches the host formatter; every runner writes the file the host formatter writes."""
import ctypes as C
import struct

import numpy as np
import pytest

import pybam
import samcases
import samfmtcases

NAMES = samfmtcases.NAMES
MSG = "bad record in the output stream"


def fmt(records, names=NAMES, **kw):
    from gencore_amd.bamio import format_sam
    return format_sam(records, names, **kw)


def raw_bam(path, recs, targets, text="@HD\tVN:1.6\n"):
    s = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(targets))
    for nm, ln in targets:
        s += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    s += b"".join(recs)
    with open(path, "wb") as f:
        for o in range(0, len(s), 0xff00):
            f.write(pybam.bgzf_block(s[o:o + 0xff00], 1))
        f.write(pybam.EOF_BLOCK)


def sam_body(path):
    """the alignment lines of a SAM file (a line may hold a line feed of its own: the header is what is cut off)"""
    got = open(path, "rb").read()
    o = 0
    while got[o:o + 1] == b"@":
        o = got.index(b"\n", o) + 1
    return got[o:]


def host_lines(tmp_path, recs, targets=samfmtcases.TARGETS):
    from gencore_amd.bamio import bam_to_sam
    raw_bam(tmp_path / "h.bam", recs, targets)
    bam_to_sam(tmp_path / "h.bam", tmp_path / "h.sam", threads=3)
    return sam_body(tmp_path / "h.sam")


def good_records():
    return [c[1] for c in samcases.field_edge_cases()] + [r for _, r in samfmtcases.hand_built()]


@pytest.mark.gpu
def test_field_edges(built, tmp_path):
    recs = good_records()
    want = host_lines(tmp_path, recs)
    model = [samfmtcases.line_of(r) for r in recs]
    assert want == b"".join(model)                                 # the two references agree
    r = fmt(b"".join(recs))
    n_host = sum(1 for x in recs if samfmtcases.holds_float(x))
    assert r["n_records"] == len(recs) and r["n_host_records"] == n_host and n_host >= 8
    if r["text"] != want:
        o = 0
        for k, m in enumerate(model):
            assert r["text"][o:o + len(m)] == m, "record %d" % k
            o += len(m)
    assert r["text"] == want
    # one record at a time as well: a window of one record, every line at offset 0 (the host records among them)
    for x, m in zip(recs, model):
        assert fmt(x) == dict(text=m, n_records=1, n_host_records=int(samfmtcases.holds_float(x)))


@pytest.mark.gpu
def test_records_pybam_can_express(built):
    """dicts through pybam.record_bytes: the line is pybam.sam_line's"""
    targets = samfmtcases.TARGETS
    rs = []
    for k, n in enumerate((1, 2, 15, 16, 17, 31, 32, 33, 151)):
        rs.append(dict(qname="p%d" % k, flag=99 if k & 1 else 147, tid=k % 4, pos=1000 * k, mapq=k, cigar="%dM" % n, mtid=(k + (k % 3 == 0)) % 4, mpos=1000 * k + 50, isize=(-1) ** k * 200,
                       seq=samcases.bases(n, "ACGTN"), qual=samcases.quals(n), nm=k, mi="UMI%d" % k, aux_pre=[("XS", "s", -300 - k), ("XA", "A", b"!")],
                       aux_post=[("XI", "I", 4000000000 + k), ("BC", "B", ("S", [k, 65535, 0]))]))
    rs.append(dict(qname="unmapped", flag=4, tid=-1, pos=-1, cigar="*", mtid=-1, mpos=-1, isize=0, seq="", qual=[]))
    rs.append(dict(qname="noqual", flag=0, tid=0, pos=5, cigar="3M", mtid=-1, mpos=-1, isize=0, seq="ACG", qual=[0xFF] * 3))
    recs = [pybam.record_bytes(r) for r in rs]
    want = b"".join(pybam.sam_line(r, targets).encode("latin-1") + b"\n" for r in rs)
    got = fmt(b"".join(recs))
    assert got["text"] == want and got["n_host_records"] == 0
    assert want == b"".join(samfmtcases.line_of(x) for x in recs)


@pytest.mark.gpu
def test_every_alignment_of_the_line_starts(built):
    """QNAME lengths 1..17, twice over with SEQ lengths that move QUAL as well: every line start and both fields walk through every alignment"""
    recs = [samfmtcases.rec(qname=b"N" * k + b"\0", lseq=30 + (k * 7 + j) % 41, pos=k, aux=pybam.aux_bytes("NM", "C", k)) for j in range(3) for k in range(1, 18)]
    want = [samfmtcases.line_of(r) for r in recs]
    starts = np.cumsum([0] + [len(w) for w in want[:-1]])
    assert len(set(int(s) % 16 for s in starts)) == 16
    assert fmt(b"".join(recs)) == dict(text=b"".join(want), n_records=len(recs), n_host_records=0)


@pytest.mark.gpu
def test_empty_input(built):
    assert fmt(b"") == dict(text=b"", n_records=0, n_host_records=0)
    assert fmt(b"", []) == dict(text=b"", n_records=0, n_host_records=0)


def raw_call(buf, cap, names=NAMES):
    """gce_sam_format on a buffer of `cap` bytes pre-filled with a sentinel -> (status, bad_record, message, the buffer afterwards)"""
    from gencore_amd import capi
    lib = capi.load_library()
    rec = np.frombuffer(bytes(buf), np.uint8)
    nm = (C.c_char_p * len(names))(*[n.encode() for n in names])
    out = np.full(cap, 0x5A, np.uint8)
    ob, nr, nh, bad = C.c_size_t(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    err = (C.c_char * 256)()
    rc = lib.gce_sam_format(0, rec.ctypes.data, len(rec), len(names), nm, out.ctypes.data, cap, C.byref(ob), C.byref(nr), C.byref(nh), C.byref(bad), err)
    return rc, int(bad.value), err.value.decode(), out


BAD = samfmtcases.bad_records()


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(BAD)), ids=[b[0].replace(" ", "_") for b in BAD])
def test_bad_record(built, k):
    """the bad record at index 100, behind 100 good ones (host records among them) and in front of another bad one"""
    from gencore_amd.capi import GceError
    good = [samfmtcases.rec(qname=b"g%d\0" % i, pos=100 + i, aux=pybam.aux_bytes("XF", "f", 0.5) if i % 10 == 3 else pybam.aux_bytes("NM", "C", i)) for i in range(100)]
    other = BAD[(k + 5) % len(BAD)][1]
    buf = b"".join(good) + BAD[k][1] + other + good[0]
    assert samfmtcases.line_of(BAD[k][1]) is None
    rc, bad, msg, out = raw_call(buf, len(buf) * 8)
    assert (rc, bad, msg) == (-1, 100, MSG)
    assert bool((out == 0x5A).all())                               # nothing is written
    with pytest.raises(GceError) as ei:
        fmt(buf)
    assert ei.value.status == -1 and ei.value.bad_record == 100 and str(ei.value).endswith(": " + MSG)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(samfmtcases.cut_records())))
def test_record_cut_by_the_end_of_the_buffer(built, k):
    good = [samfmtcases.rec(qname=b"g%d\0" % i, pos=100 + i) for i in range(100)]
    buf = b"".join(good) + samfmtcases.cut_records()[k][1]
    rc, bad, msg, out = raw_call(buf, len(buf) * 8)
    assert (rc, bad, msg) == (-1, 100, MSG) and bool((out == 0x5A).all())


@pytest.mark.gpu
def test_an_earlier_bad_record_wins_over_the_walk(built):
    """the walk stops at a block_size of 31 at index 100; the size pass finds the refusal at index 40 in front of it"""
    good = [samfmtcases.rec(qname=b"g%d\0" % i, pos=100 + i) for i in range(100)]
    good[40] = samfmtcases.rec(aux=b"XQQ\1")
    rc, bad, msg, _ = raw_call(b"".join(good) + BAD[0][1], 1 << 16)
    assert (rc, bad, msg) == (-1, 40, MSG)


@pytest.mark.gpu
def test_output_buffer_too_small(built):
    from gencore_amd.capi import GceError
    recs = good_records()[:6] + [samfmtcases.rec(aux=pybam.aux_bytes("XF", "f", 0.25))]
    want = b"".join(samfmtcases.line_of(r) for r in recs)
    with pytest.raises(GceError) as ei:
        fmt(b"".join(recs), out_cap=len(want) - 1)
    assert ei.value.status == -4 and ei.value.needed == len(want) and ei.value.bad_record == -1
    assert fmt(b"".join(recs), out_cap=len(want))["text"] == want


@pytest.fixture(scope="module")
def realistic(built, tmp_path_factory):
    """a sorted paired BAM from synth (cfg3 pairs with UMIs) with its reference: (directory, bam, fasta, contig names, parameters)"""
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    from gencore_amd.capi import default_params
    from test_cabi_driver import ascii_of
    d = tmp_path_factory.mktemp("samfmt")
    s = synth.generate("cfg3", n_pairs=2500, scale=0.002)
    tl = np.asarray(s.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(str(d / "in.bam"), s.to_batch(), tl, names, threads=4)
    with open(d / "ref.fa", "wb") as f:
        for nm, bases in zip(names, ascii_of(s.reference_host())):
            if bases is not None:
                f.write(b">" + nm.encode() + b"\n" + bases + b"\n")
    prm = default_params(umi_prefix="auto", cluster_size_req=s.info["supporting_reads"])
    return d, d / "in.bam", d / "ref.fa", names, prm


@pytest.mark.gpu
def test_realistic_stream(realistic):
    import pysort
    from gencore_amd.bamio import bam_to_sam
    d, bam, _, names, _ = realistic
    recs = pysort.records(bam)[1][:5000]
    assert len(recs) == 5000
    bam_to_sam(bam, d / "in.sam", threads=4)
    want = b"".join(sam_body(d / "in.sam").split(b"\n")[k] + b"\n" for k in range(5000))
    assert len(want) > 5000 * 300
    r = fmt(b"".join(recs), names)
    assert r["n_records"] == 5000 and r["text"] == want
    assert r["n_host_records"] == 0                                # no floating-point tags: the host formatter stays out of the ordinary path


def counters():
    from gencore_amd.bamio import sam_format_counters
    return sam_format_counters()


def check_runner(run, d, what):
    """run(out_path, level) -> n_out: level 1 (the host formatter) and level -2 (the GPU's) write the same file; the counters tell who did"""
    c0 = counters()
    n1 = run(d / ("%s_host.sam" % what), 1)
    c1 = counters()
    n2 = run(d / ("%s_gpu.sam" % what), -2)
    c2 = counters()
    host, gpu = (d / ("%s_host.sam" % what)).read_bytes(), (d / ("%s_gpu.sam" % what)).read_bytes()
    assert n1 == n2 and n1 > 100
    assert c1 == c0, what                                          # level 1: the GPU writer did not run
    assert c2[0] - c1[0] == n2 and c2[1] == c1[1] and c2[2] > c1[2], (what, c1, c2)
    assert host == gpu and gpu.count(b"\n") > n2, what
    assert c2[3] - c1[3] == len(sam_body(d / ("%s_gpu.sam" % what)))
    return gpu


@pytest.mark.gpu
def test_run_bam_writes_the_hosts_file(realistic):
    from gencore_amd.bamio import run_bam
    d, bam, fa, _, prm = realistic
    whole = check_runner(lambda out, lv: run_bam(bam, out, prm, fasta=fa, threads=4, level=lv).n_out, d, "one")
    small = check_runner(lambda out, lv: run_bam(bam, out, prm, fasta=fa, threads=4, level=lv, chunk_reads=4096).n_out, d, "small")      # (the small-piece path)
    assert whole == small
    c0 = counters()
    run_bam(bam, d / "three.sam", prm, fasta=fa, threads=4, level=-3)
    assert (d / "three.sam").read_bytes() == whole and counters()[2] == c0[2] + 1


@pytest.mark.gpu
def test_pass_runner_writes_the_hosts_file(realistic):
    from gencore_amd.bamio import run_bam_passes
    d, bam, fa, _, prm = realistic

    def run(out, lv):
        r, _, p = run_bam_passes(bam, out, prm, fasta=fa, threads=4, level=lv, min_passes=3)
        assert p["n_passes"] >= 3 and not p["single_pass"]
        return r.n_out
    check_runner(run, d, "passes")


@pytest.mark.gpu
def test_sharded_runner_writes_the_hosts_file(realistic):
    from gencore_amd.bamio import run_bam_sharded
    d, bam, fa, _, prm = realistic
    check_runner(lambda out, lv: run_bam_sharded(bam, out, prm, [0, 0], fasta=fa, threads=4, level=lv).n_out, d, "sharded")
