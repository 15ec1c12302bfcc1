"""gce_bam_calmd_stream on the GPU (gencore_amd/csrc/gce_calmd.hpp): with the cap on resident output forced down to one BGZF
member its file equals gce_bam_calmd's byte for byte at every level and window size, and the model's records and counters; the cut at exact
multiples of 0xff00, one byte either side of one member, inside the 98 KB record, on a file without records and on a window whose output
alone exceeds the cap; a budget at which gce_bam_calmd runs out of device memory; a malformed record found after flushes were written; the
command line under --device_memory.  Every command line runs as its own process under `timeout`, one after another.

A flush happens in front of a window, when at least one whole member is resident, so a run flushes at most once per window after its first.
The 300-byte-member file of every case record is about 40 KB: one window at window_bytes=0 (nothing can leave early: its output is that
window's and the buffer grows to hold it), three at 20000 (measured: 1 flush of one member), dozens at 2000 (measured: 2 flushes, 3 members).
So n_flushes >= 2 is asserted at window_bytes 2000, exactly that one flush at 20000 and n_flushes == 0 at 0, at every level: a run that never
flushed fails wherever it could have flushed."""
import json
import os

import numpy as np
import pytest

import calmdcases as cc
import pybai
import pycalmd
import pysort
from test_calmd_gpu import COUNTERS, calmd, cli, head_of, leftovers, ref, rule_f, write  # noqa: F401  (ref: a fixture)

M = 0xff00
FOOTPRINT = "the reference bases + one window + 40 bytes per window record + one piece's deflate buffers + at least one window's output"


def calmd_stream(path, out, fa, window_bytes=0, level=-2, budget=0, resident=0):
    from gencore_amd.bamio import calmd_bam_stream
    return calmd_bam_stream(str(path), str(out), str(fa), device=0, threads=4, level=level, window_bytes=window_bytes, device_budget_bytes=budget, resident_bytes=resident)


def model_sizes(recs, fasta):
    new, counters = pycalmd.calmd_records(recs, cc.NAMES, fasta)
    return [len(r) for r in new], counters


def pad_record(n):
    """an ineligible record (unmapped: copied whole) of exactly n bytes, block_size included"""
    base = cc.record(0, 0, "10M", "CCGTACGTCA", aux=b"XAZ\0", flag=4, qname="pad")
    assert n >= len(base)
    r = cc.record(0, 0, "10M", "CCGTACGTCA", aux=b"XAZ" + b"x" * (n - len(base)) + b"\0", flag=4, qname="pad")
    assert len(r) == n
    return r


def small_records():
    return [r for _, r, _, _ in cc.hand_vectors()] + [r for r, _ in cc.alignment_cases()]


def both(d, name, recs, fa, window_bytes, level=-2, resident=M, block=300):
    """name.bam through calmd_bam and calmd_bam_stream: the two files are equal; -> (the streamed run, the in-core run, the file's bytes)"""
    path = d / (name + ".bam")
    write(path, recs, block=block)
    before = path.read_bytes()
    core, out = d / (name + ".core.bam"), d / (name + ".stream.bam")
    rc = calmd(path, core, fa, window_bytes, level)
    rs = calmd_stream(path, out, fa, window_bytes, level, resident=resident)
    blob = out.read_bytes()
    print("%s: window_bytes=%d level=%d out_record_bytes=%d n_flushes=%d flushed_bytes=%d cap=%d" % (name, window_bytes, level, rs.out_record_bytes, rs.n_flushes, rs.flushed_bytes, rs.resident_cap_bytes))
    assert blob == core.read_bytes()
    assert {k: getattr(rs, k) for k in COUNTERS} == {k: getattr(rc, k) for k in COUNTERS}
    assert (rs.out_record_bytes, rs.inflated_bytes, rs.out_bytes, rs.n_ref) == (rc.out_record_bytes, rc.inflated_bytes, len(blob), rc.n_ref)
    assert rs.flushed_bytes % M == 0 and rs.flushed_bytes <= rs.out_record_bytes and (rs.n_flushes == 0) == (rs.flushed_bytes == 0)
    assert path.read_bytes() == before and leftovers(d) == []
    return rs, rc, blob


@pytest.mark.gpu
def test_equal_files(ref):
    """levels 1, -1, -2 and -3 against window_bytes 0, 2000 and 20000 on the 300-byte-member file of every case record, the cap one member"""
    d, fa, fasta = ref
    path = d / "swin.bam"
    write(path, cc.file_records(), block=300)
    head, want, counters = pycalmd.calmd_model(path, fasta)
    total = sum(len(x) for x in want)
    assert total > 2 * M
    for lv in (1, -1, -2, -3):
        core = d / "swin.core.bam"
        calmd(path, core, fa, 0, lv)
        want_blob = core.read_bytes()
        for w in (0, 2000, 20000):
            out = d / "swin.stream.bam"
            r = calmd_stream(path, out, fa, w, lv, resident=M)
            blob = out.read_bytes()
            print("level=%d window_bytes=%d out_record_bytes=%d n_flushes=%d flushed_bytes=%d" % (lv, w, r.out_record_bytes, r.n_flushes, r.flushed_bytes))
            assert blob == want_blob, "window_bytes=%d level=%d" % (w, lv)
            assert {k: getattr(r, k) for k in COUNTERS} == counters
            assert r.out_record_bytes == total and r.out_bytes == len(blob) and r.resident_cap_bytes == M
            assert r.flushed_bytes % M == 0 and 0 <= total - r.flushed_bytes
            if w == 2000:
                assert r.n_flushes >= 2 and r.flushed_bytes >= 2 * M, "window_bytes=%d level=%d: %d flushes" % (w, lv, r.n_flushes)
            elif w == 20000:
                assert (r.n_flushes, r.flushed_bytes) == (1, M), "window_bytes=%d level=%d: %d flushes" % (w, lv, r.n_flushes)
            else:
                assert r.n_flushes == 0 and r.flushed_bytes == 0                  # (one window: nothing is resident in front of it)
            out.unlink()
        u = pysort.inflate(want_blob)
        assert u[:len(head)] == head and pysort.split(u)[1] == want
        rule_f(want_blob, head, total)
    assert leftovers(d) == []


@pytest.mark.gpu
def test_cut_at_member_multiples(ref):
    """an output of exactly 3 x 0xff00 bytes (no empty last member), of 0xff00 - 1 and of 0xff00 + 1 bytes"""
    d, fa, fasta = ref
    base = small_records()
    sizes, _ = model_sizes(base, fasta)
    one = sum(sizes)
    for name, target in (("exact3", 3 * M), ("below1", M - 1), ("above1", M + 1)):
        reps = max(1, (target - 2000) // one)
        recs = base * reps
        half = len(recs) // 2
        recs = recs[:half] + [pad_record(target - reps * one)] + recs[half:]
        assert sum(model_sizes(recs, fasta)[0]) == target
        for lv in (-2, 1):
            rs, _, blob = both(d, name, recs, fa, 2000, lv)
            assert rs.out_record_bytes == target
            rule_f(blob, head_of(d / (name + ".bam")), target)                   # (its last member is not empty)
            if target == 3 * M:
                assert rs.n_flushes >= 2 and 2 * M <= rs.flushed_bytes < target  # (the last window's records are never flushed early: a whole last member is left)
            if target < M:
                assert rs.n_flushes == 0


@pytest.mark.gpu
def test_cut_inside_the_large_record(ref):
    """the 98 KB record behind just under one member of small records, more records behind it: the first flush cuts inside it, and what
    stays resident begins in its middle"""
    d, fa, fasta = ref
    base = small_records()
    big = [r for label, r, _, _, _ in cc.long_cases() if label == "NM 65536 needs I"][0]
    sizes, _ = model_sizes(base, fasta)
    reps = (M - 1500) // sum(sizes)
    front = base * reps
    a = sum(model_sizes(front, fasta)[0])
    z = a + model_sizes([big], fasta)[0][0]
    assert a < M and z > 2 * M + 4 and z - 2 * M < M                              # the first flush takes 2 members: its cut is inside [a, z)
    recs = front + [big] + base * 40
    rs, _, _ = both(d, "bigcut", recs, fa, 2000)
    assert rs.n_flushes >= 2
    rs1, _, _ = both(d, "bigcut_tail", front + [big] + base, fa, 2000)            # less than a member behind it: exactly that flush
    assert (rs1.n_flushes, rs1.flushed_bytes) == (1, 2 * M)


@pytest.mark.gpu
def test_no_records_and_one_window_beyond_the_cap(ref):
    d, fa, fasta = ref
    for lv in (-2, 6):
        rs, _, blob = both(d, "sempty", [], fa, 0, lv, block=M)
        assert (rs.n_records, rs.n_flushes, rs.out_record_bytes) == (0, 0, 0)
        rule_f(blob, head_of(d / "sempty.bam"), 0)
    # one window whose output alone exceeds the cap: the buffer grows to hold it, nothing is flushed
    for lv in (-3, 1):
        rs, _, _ = both(d, "onewin", cc.file_records(), fa, 0, lv, block=M)
        assert rs.n_flushes == 0 and rs.out_record_bytes > 2 * M and rs.resident_cap_bytes == M
    rs, _, _ = both(d, "roundup", cc.file_records(), fa, 2000, resident=1)       # the cap is rounded up to a member
    assert rs.resident_cap_bytes == M and rs.n_flushes >= 2


@pytest.mark.gpu
def test_budget(ref):
    """record bytes that dominate the reference and one window: half of what the in-core pass took (at its level) is not enough for it, and is for the
    streamed one, which stays within it and writes the same bytes; a budget below the reference bases says what is needed"""
    from gencore_amd.capi import GceError
    d, fa, fasta = ref
    recs = cc.file_records()
    big = sorted(recs, key=len)[-2:]
    recs = big + [r for r in recs if len(r) < 0x10000]                            # (the windows that hold the large records come first: later ones are smaller)
    path = d / "budget.bam"
    write(path, recs * 60)
    before = path.read_bytes()
    for lv in (1, -2):                                                            # (-2: the in-core pass holds the deflate buffers of the whole output as well)
        r0 = calmd(path, d / "budget.core.bam", fa, 20000, lv)
        budget = r0.peak_device_bytes // 2
        print("in-core: level=%d out_record_bytes=%d peak_device_bytes=%d" % (lv, r0.out_record_bytes, r0.peak_device_bytes))
        assert r0.out_record_bytes > budget or lv != 1                            # (the record bytes dominate: alone they pass the budget)
        with pytest.raises(GceError) as ei:                                       # the premise
            calmd(path, d / "out.bam", fa, 20000, lv, budget=budget)
        assert ei.value.status == -4 and not (d / "out.bam").exists()
        r = calmd_stream(path, d / "budget.stream.bam", fa, 20000, lv, budget=budget)
        print("streamed: level=%d budget=%d peak_device_bytes=%d n_flushes=%d cap=%d" % (lv, budget, r.peak_device_bytes, r.n_flushes, r.resident_cap_bytes))
        assert 0 < r.peak_device_bytes <= budget and r.n_flushes >= 1 and r.resident_cap_bytes % M == 0 and 0 < r.resident_cap_bytes < budget
        assert (d / "budget.stream.bam").read_bytes() == (d / "budget.core.bam").read_bytes()
    # the rest after the last flush: at level -2 the deflate buffers the flushes used also serve the last piece, whatever is left resident.
    # Shorter files at that budget leave other amounts behind their last flush: one of them more than half the cap.
    rests = []
    for reps in (56, 52, 48, 44, 40):
        write(d / "rest.bam", recs * reps)
        calmd(d / "rest.bam", d / "rest.core.bam", fa, 20000, -2)
        r = calmd_stream(d / "rest.bam", d / "rest.stream.bam", fa, 20000, -2, budget=budget)
        rests.append((r.out_record_bytes - r.flushed_bytes) / float(r.resident_cap_bytes))
        print("streamed: %d repeats, budget=%d peak_device_bytes=%d n_flushes=%d cap=%d rest=%d" % (reps, budget, r.peak_device_bytes, r.n_flushes, r.resident_cap_bytes, r.out_record_bytes - r.flushed_bytes))
        assert r.n_flushes >= 1 and 0 < r.peak_device_bytes <= budget
        assert (d / "rest.stream.bam").read_bytes() == (d / "rest.core.bam").read_bytes()
    assert max(rests) > 0.5, rests
    with pytest.raises(GceError) as ei:
        calmd_stream(path, d / "out.bam", fa, 20000, 1, budget=100)               # (the reference bases and their table take more)
    assert ei.value.status == -4 and FOOTPRINT in str(ei.value), str(ei.value)
    assert not (d / "out.bam").exists() and leftovers(d) == [] and path.read_bytes() == before


@pytest.mark.gpu
def test_failure_after_a_flush(ref):
    """a record whose optional fields do not tile its block_size, behind records of which some were already written: the call names it and
    leaves nothing, a file that was at out_path stays"""
    from gencore_amd.capi import GceError
    d, fa, fasta = ref
    good = cc.file_records() + small_records() * 10
    bad = cc.malformed()[2][1]
    write(d / "front.bam", good, block=300)
    r = calmd_stream(d / "front.bam", d / "front.out.bam", fa, 2000, resident=M)
    assert r.n_flushes >= 2                                                       # so flushes came before the record below
    path = d / "late.bam"
    write(path, good + [bad] + small_records(), block=300)
    before = path.read_bytes()
    out = d / "late.out.bam"
    for lv, old in ((-2, None), (1, b"what was here")):
        if old is not None:
            out.write_bytes(old)
        with pytest.raises(GceError) as ei:
            calmd_stream(path, out, fa, 2000, lv, resident=M)
        assert ei.value.status == -1 and ("record %d " % len(good)) in str(ei.value), str(ei.value)
        assert (out.read_bytes() == old) if old is not None else not out.exists()
        assert leftovers(d) == [] and path.read_bytes() == before


# ---------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def windows3(built, tmp_path_factory):
    """synth.bam: 400 000 cfg3 pairs in stored members, 244 MB: four windows of the 64 MB the command line reads with.  The run itself needs
    0.61 GB of device memory beside a pass's reads whatever the file (one such window and the engine), so the in-core pass has to need
    clearly more than that for a budget to lie between them: about 3.6 x the record bytes at level -2, the output and its deflate buffers.
    With ref.fa."""
    import torch
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    from test_calmd_gpu import write_fasta
    d = tmp_path_factory.mktemp("calmdmem")
    s = synth.generate("cfg3", n_pairs=400000, scale=0.002, device=torch.device("cuda:0"))
    tl = np.asarray(s.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(str(d / "synth.bam"), s.to_batch(), tl, names, threads=4, level=0)
    write_fasta(d / "ref.fa", names, s.reference_host())
    assert os.path.getsize(str(d / "synth.bam")) > 3 * (64 << 20)
    return d


@pytest.mark.gpu
def test_cli_device_memory(windows3):
    """--calmd_in --calmd under a --device_memory at which the in-core pass runs out of device memory on the same input (0.8 of its peak:
    above what the run needs and above the streamed pass's reference + window + one window's output and deflate buffers, below the in-core
    pass's whole output and deflate buffers): the output inflates to the bytes of the run without the budget, the reports are equal, --index accepts the result"""
    from gencore_amd.capi import GceError
    d = windows3
    r0 = calmd(d / "synth.bam", d / "probe.bam", d / "ref.fa", level=-2)
    x = r0.peak_device_bytes * 8 // 10
    print("in-core calmd of the input: peak_device_bytes=%d, --device_memory %d bytes" % (r0.peak_device_bytes, x))
    with pytest.raises(GceError) as ei:                                           # the premise: what the command line did before
        calmd(d / "synth.bam", d / "probe2.bam", d / "ref.fa", level=-2, budget=x)
    assert ei.value.status == -4 and not (d / "probe2.bam").exists()
    (d / "probe.bam").unlink()
    base = ["-i", "synth.bam", "-r", "ref.fa", "-s", "2", "--threads", "4", "--calmd_in", "--calmd", "--level", "-2"]
    a = cli(base + ["-o", "m0.bam", "-j", "m0.json"], d, timeout=120)
    assert a.returncode == 0, a.stderr
    b = cli(base + ["-o", "m1.bam", "-j", "m1.json", "--device_memory", repr(x / float(1 << 30)), "--index"], d, timeout=120)
    assert b.returncode == 0, b.stderr
    assert pysort.inflate((d / "m1.bam").read_bytes()) == pysort.inflate((d / "m0.bam").read_bytes()) and len(pysort.records(d / "m1.bam")[1]) > 0
    ja, jb = json.loads((d / "m0.json").read_text()), json.loads((d / "m1.json").read_text())
    assert "--device_memory" not in ja.pop("command") and "--device_memory" in jb.pop("command")
    assert ja == jb
    assert (d / "m1.bam.bai").read_bytes() == pybai.build(d / "m1.bam")
    assert [p.name for p in d.iterdir() if p.name.startswith("gencore_calmd_") or ".tmp" in p.name or ".calmd" in p.name] == []
