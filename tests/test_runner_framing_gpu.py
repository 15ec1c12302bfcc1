"""What each file-to-file runner says about a file whose BGZF framing or BAM header is damaged (the parts of gencore_amd/csrc/bamio.cpp: the
member scanner and header parser of gce_bgzf.hpp and the reader of bamio_reader.hpp under gce_run_bam (bamio_run.hpp), gce_run_bam_passes
(bamio_passes.hpp), gce_bam_index (bamio_index.hpp), gce_bam_sort and gce_bam_sort_passes (bamio_sort.hpp), gce_bam_calmd and
gce_bam_calmd_stream (bamio_calmd.hpp)).
Every damage here is one the host's framing check rejects before a damaged member reaches a kernel: where members do go to the GPU (a file
cut inside its EOF member) they are whole and well-formed.  The table holds status and message of every (runner, damage) pair, read off
each runner's own copy of the framing code as it stood before that code was shared; the messages are compared whole.  The two calmd
columns were recorded by running them against the library as it stood before bamio.cpp was split into its parts."""
import struct

import numpy as np
import pytest

import pybam

TARGETS = [("chr1", 200_000), ("chr2", 50_000)]
TEXT = "@HD\tVN:1.6\tSO:coordinate\n"
INVALID = -1

NOT_BGZF = "not a BGZF file"
BAD = "bad BGZF block"
BAD_ISIZE = "bad BGZF block (ISIZE above 64 KB)"
CUT = "truncated BGZF block at the end of the file"
WINDOW = "BGZF block larger than a window"
NOT_BAM = "not a BAM stream"

RUNNERS = ("run_bam", "run_bam_passes", "bam_index", "sort_bam", "sort_bam_passes")
# (status, message); one row per damage, one column per runner in the order of RUNNERS.  None: the runner takes no window_bytes.
OK = (0, "")
TABLE = {
    # the file ends inside its last member (the EOF marker): the pass runner stops at the last piece without looking at what is left over
    "cut_in_last_member": [(INVALID, CUT), OK, (INVALID, CUT), (INVALID, CUT), (INVALID, CUT)],
    "cut_in_header_member": [(INVALID, CUT)] * 5,
    "magic_of_second_member": [(INVALID, NOT_BGZF)] * 5,
    "bc_missing": [(INVALID, BAD)] * 5,
    "isize_above_64k": [(INVALID, BAD_ISIZE)] * 5,
    "not_bam": [(INVALID, NOT_BAM)] * 5,
    # whole members, but the stream ends inside the BAM header: the two dialects' words
    "stream_ends_in_header": [(INVALID, "truncated header"), (INVALID, "truncated header"), (INVALID, "truncated BAM header"), (INVALID, "truncated BAM header"),
                              (INVALID, "truncated BAM header")],
    "window_below_a_member": [None, (INVALID, WINDOW), (INVALID, WINDOW), (INVALID, WINDOW), (INVALID, WINDOW)],
}
# the same rows for the two calmd runners, which open their input as the sort runners do
CALMD_RUNNERS = ("calmd", "calmd_stream")
CALMD_TABLE = {
    "cut_in_last_member": [(INVALID, CUT)] * 2,
    "cut_in_header_member": [(INVALID, CUT)] * 2,
    "magic_of_second_member": [(INVALID, NOT_BGZF)] * 2,
    "bc_missing": [(INVALID, BAD)] * 2,
    "isize_above_64k": [(INVALID, BAD_ISIZE)] * 2,
    "not_bam": [(INVALID, NOT_BAM)] * 2,
    "stream_ends_in_header": [(INVALID, "truncated BAM header")] * 2,
    "window_below_a_member": [(INVALID, WINDOW)] * 2,
}
assert sorted(CALMD_TABLE) == sorted(TABLE)
ALL_RUNNERS = RUNNERS + CALMD_RUNNERS


def expected(runner, damage):
    return TABLE[damage][RUNNERS.index(runner)] if runner in RUNNERS else CALMD_TABLE[damage][CALMD_RUNNERS.index(runner)]


@pytest.fixture(scope="module")
def parts(tmp_path_factory):
    """the members of a small sorted BAM: the header in a member of its own, a dozen records in two members, the EOF marker; a FASTA of the
    two contigs for the calmd runners"""
    from gencore_amd import synth
    from test_bamio import records_of
    d = synth.generate("cfg1s", n_pairs=7)
    recs = [pybam.record_bytes(r) for r in records_of(d.to_batch())]
    assert len(recs) == 12
    hdr = b"BAM\1" + struct.pack("<i", len(TEXT)) + TEXT.encode() + struct.pack("<i", len(TARGETS))
    for nm, ln in TARGETS:
        hdr += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    fasta = tmp_path_factory.mktemp("framing") / "ref.fa"
    rng = np.random.default_rng(7)
    with open(fasta, "w") as f:
        for nm, ln in TARGETS:
            f.write(">%s\n" % nm)
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)].tobytes().decode()
            f.write("\n".join(seq[k:k + 60] for k in range(0, ln, 60)) + "\n")
    return dict(d=d, hdr=hdr, fasta=str(fasta), members=[pybam.bgzf_block(hdr), pybam.bgzf_block(b"".join(recs[:6])), pybam.bgzf_block(b"".join(recs[6:])), pybam.EOF_BLOCK])


def damaged(parts, damage):
    """-> (the file's bytes, window_bytes)"""
    m = list(parts["members"])
    whole = b"".join(m)
    if damage == "cut_in_last_member":
        return whole[:-10], 0
    if damage == "cut_in_header_member":
        return whole[:30], 0
    if damage == "magic_of_second_member":
        m[1] = b"\x1e" + m[1][1:]
    elif damage == "bc_missing":
        m[1] = m[1][:12] + b"XY" + m[1][14:]
    elif damage == "isize_above_64k":
        m[1] = m[1][:-4] + struct.pack("<I", 0x10001)
    elif damage == "not_bam":
        m[0] = pybam.bgzf_block(b"BAX\1" + parts["hdr"][4:])
    elif damage == "stream_ends_in_header":
        m = [pybam.bgzf_block(parts["hdr"][:len(parts["hdr"]) - 6]), pybam.EOF_BLOCK]
    elif damage == "window_below_a_member":
        assert min(len(x) for x in m[:3]) > 40
        return whole, 40
    return b"".join(m), 0


def call(runner, parts, src, out, window):
    from gencore_amd import bamio
    from gencore_amd.capi import default_params
    tl = np.asarray([l for _, l in TARGETS], np.uint32)
    prm = default_params(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix=parts["d"].info["umi_prefix"])
    prm._keep = tl
    if runner == "run_bam":
        return bamio.run_bam(src, out, prm, threads=2, level=1)
    if runner == "run_bam_passes":
        return bamio.run_bam_passes(src, out, prm, threads=2, level=1, min_passes=2, window_bytes=window)
    if runner == "bam_index":
        return bamio.index_bam(src, out, threads=2, window_bytes=window)
    if runner == "sort_bam":
        return bamio.sort_bam(src, out, threads=2, level=1, window_bytes=window)
    if runner == "sort_bam_passes":
        return bamio.sort_bam_passes(src, out, threads=2, level=1, window_bytes=window, min_passes=2)
    if runner == "calmd":
        return bamio.calmd_bam(src, out, parts["fasta"], threads=2, level=1, window_bytes=window)
    assert runner == "calmd_stream"
    return bamio.calmd_bam_stream(src, out, parts["fasta"], threads=2, level=1, window_bytes=window)


def test_the_damages_are_what_they_say(parts):
    """the good file is a BAM pybam reads; each damaged file differs from it where its name says"""
    import gzip
    whole = b"".join(parts["members"])
    u = gzip.decompress(whole)
    assert u.startswith(parts["hdr"]) and len(parts["members"][0]) > 40
    for damage in TABLE:
        blob, window = damaged(parts, damage)
        assert (blob != whole) != (damage == "window_below_a_member") and (window > 0) == (damage == "window_below_a_member")
    assert gzip.decompress(damaged(parts, "not_bam")[0])[:4] == b"BAX\1"


@pytest.mark.gpu
@pytest.mark.parametrize("runner,damage", [(r, d) for d in sorted(TABLE) for r in ALL_RUNNERS if expected(r, d) is not None])
def test_runner_message(built, parts, tmp_path, runner, damage):
    from gencore_amd.capi import GceError
    want = expected(runner, damage)
    blob, window = damaged(parts, damage)
    src, out = str(tmp_path / "in.bam"), str(tmp_path / ("out.bai" if runner == "bam_index" else "out.bam"))
    with open(src, "wb") as f:
        f.write(blob)
    try:
        call(runner, parts, src, out, window)
        got = OK
    except GceError as e:
        got = (e.status, str(e).split(": ", 1)[1])
    print("%s / %s: %r" % (runner, damage, got))
    assert got == want
