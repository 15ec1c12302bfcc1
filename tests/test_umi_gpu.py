"""gce_bam_umi_to_mi on the GPU (gencore_amd/csrc/gce_umi.hpp): the inflated bytes of its output and its counters equal the
pure-Python model's (tests/pyumi.py) on every record of tests/umicases.py across windows, levels, the cap on resident output and both kinds
of source; a record larger than a window and a member, cut inside; files without records or without a source; malformed records before and
after flushes; a file with RX against the same file with the MI the pass must write, byte for byte; the pass and the run against the
oracle's run on the records that carry those MI; `--umi_from` of the command line.  Every command line runs as its own process under
`timeout`, one after another."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pybam
import pysort
import pyumi
import umicases as uc
from test_bai_model import header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 0xff00
COUNTERS = ("n_records", "n_tagged", "n_no_source", "n_not_umi", "n_mi_dropped")
REPEATS = 16                                                    # the 9 KB of case records, repeated: more than two members of output


def umi(path, out, source="RX", window_bytes=0, level=-2, budget=0, resident=0):
    from gencore_amd.bamio import umi_to_mi
    return umi_to_mi(str(path), str(out), source=source, device=0, threads=4, level=level, window_bytes=window_bytes, device_budget_bytes=budget, resident_bytes=resident)


def leftovers(d):
    return sorted(p.name for p in d.iterdir() if ".tmp" in p.name)


def write(path, recs, block=300, text="@HD\tVN:1.6\tSO:unsorted\n"):
    pysort.write(path, header(uc.TARGETS, text=text), recs, block=block)


def check(path, source, out, r):
    """the run r of path into out against the model"""
    head, want, counters = pyumi.umi_model(path, source)
    blob = out.read_bytes()
    u = pysort.inflate(blob)                                    # plain zlib, member by member
    assert blob.endswith(pysort.EOF_BLOCK) and u[:len(head)] == head
    got = pysort.split(u)[1]
    assert len(got) == len(want)
    assert got == want, "first difference at record %d" % next(k for k, (a, b) in enumerate(zip(got, want)) if a != b)
    assert {k: getattr(r, k) for k in COUNTERS} == counters
    assert r.out_record_bytes == sum(len(x) for x in want) and r.out_bytes == len(blob) and r.inflated_bytes == len(pysort.inflate(path.read_bytes())) - len(head)
    assert leftovers(path.parent) == []
    return counters


@pytest.fixture(scope="module")
def casefile(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("umi")
    path = d / "cases.bam"
    write(path, uc.file_records() * REPEATS)
    return d, path


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["RX", "name"])
@pytest.mark.parametrize("level", [1, -2, -3])
def test_all_cases_across_windows_levels_and_caps(casefile, source, level):
    """every case record in one file of 300-byte members: records, header and counters are the model's at every window size, with the cap
    on resident output forced down to one member (flushes happen at 2000: a flush needs a member resident in front of a window) and without"""
    d, path = casefile
    before = path.read_bytes()
    out = d / "cases.out.bam"
    for w in (0, 2000, 20000):
        for resident in (M, 0):
            r = umi(path, out, source, w, level, resident=resident)
            print("source=%s level=%d window_bytes=%d resident=%d: out_record_bytes=%d n_flushes=%d" % (source, level, w, resident, r.out_record_bytes, r.n_flushes))
            c = check(path, source, out, r)
            assert c["n_tagged"] > 0 and c["n_no_source"] > 0 and c["n_not_umi"] > 0 and c["n_mi_dropped"] > 0
            assert r.out_record_bytes > 2 * M
            if resident == M and w == 2000:
                assert r.n_flushes >= 1
            if resident == 0 or w == 0:
                assert r.n_flushes == 0                         # (no cap within the device's budget; or one window: nothing is resident in front of it)
            out.unlink()
    assert path.read_bytes() == before


@pytest.mark.gpu
def test_a_record_larger_than_a_window(casefile):
    """a 70 KB B field with a 3000-byte MI in front of it and another behind it, in members of 300 bytes and windows of 2000: the record spans
    hundreds of members and dozens of windows, cuts of both fall inside its dropped MI, and with just under one member of records in front
    of it the first flush cuts the output inside it"""
    d, _ = casefile
    big, want = uc.big_record()
    small = uc.file_records()
    sizes = [len(x) for x in pyumi.umi_records(small, "RX")[0]]
    front, a = [], 0
    while a + sizes[len(front) % len(small)] <= M - 1000:           # just under one member of output
        a += sizes[len(front) % len(small)]
        front.append(small[len(front) % len(small)])
    assert a < M < a + len(want) < 2 * M + a and len(big) > 70000
    path, out = d / "big.bam", d / "big.out.bam"
    write(path, front + [big] + small * 4)
    for source in ("RX", "name"):
        for w, resident in ((2000, M), (0, 0), (2000, 0)):
            r = umi(path, out, source, w, resident=resident)
            check(path, source, out, r)
            assert (r.n_flushes >= 1) == (resident == M)
    got = pysort.records(out)[1]
    assert got[len(front)] == big                               # (name mode: `big` has no colon)
    r = umi(path, out, "RX", 2000, resident=M)
    assert pysort.records(out)[1][len(front)] == want and r.n_mi_dropped > 1


@pytest.mark.gpu
def test_nothing_to_do(casefile):
    """a header-only file and a file whose records are all without a source: the output's inflated stream is the input's"""
    d, _ = casefile
    none = [c[2] for c in uc.all_cases() if c[1] == "RX" and c[4] == "no_source"]
    assert len(none) >= 10 and any(b"MIZ" in r for r in none)
    for name, recs in (("empty", []), ("nosource", none * 40)):
        path, out = d / (name + ".bam"), d / (name + ".out.bam")
        write(path, recs)
        for lv, w, resident in ((-2, 0, 0), (1, 2000, M), (-3, 2000, M)):
            r = umi(path, out, "RX", w, lv, resident=resident)
            assert pysort.inflate(out.read_bytes()) == pysort.inflate(path.read_bytes())
            assert (r.n_records, r.n_tagged, r.n_no_source, r.n_not_umi, r.n_mi_dropped) == (len(recs), 0, len(recs), 0, 0)
            assert r.out_record_bytes == r.inflated_bytes == sum(len(x) for x in recs) and leftovers(d) == []
            out.unlink()


@pytest.mark.gpu
def test_malformed_records(casefile):
    """each malformed case in the middle of a file: GCE_ERR_INVALID names its index and nothing is left, in one window and across windows; the
    same behind records of which some were already flushed, where a file that was at out_path stays"""
    from gencore_amd.capi import GceError
    d, _ = casefile
    good = uc.file_records()
    out = d / "bad.out.bam"
    for k, (label, bad) in enumerate(uc.malformed()):
        recs = good[:5 + k] + [bad] + good[5 + k:] + [uc.malformed()[0][1]]
        path = d / ("bad%d.bam" % k)
        write(path, recs, block=200)
        for source, w in (("RX", 0), ("name", 400)) if k % 2 else (("name", 0), ("RX", 400)):
            with pytest.raises(pyumi.UmiError) as mi:
                pyumi.umi_model(path, source)
            assert mi.value.record == 5 + k
            with pytest.raises(GceError) as ei:
                umi(path, out, source, w)
            assert ei.value.status == -1 and ("record %d " % (5 + k)) in str(ei.value), (label, str(ei.value))
            assert not out.exists() and leftovers(d) == []
    front = good * REPEATS
    write(d / "front.bam", front)
    assert umi(d / "front.bam", d / "front.out.bam", "RX", 2000, resident=M).n_flushes >= 1     # so flushes come before the record below
    for k, old in ((0, None), (2, b"what was here"), (4, None)):
        path = d / ("late%d.bam" % k)
        write(path, front + [uc.malformed()[k][1]] + good)
        before = path.read_bytes()
        if old is not None:
            out.write_bytes(old)
        with pytest.raises(GceError) as ei:
            umi(path, out, "RX", 2000, 1 if k else -2, resident=M)
        assert ei.value.status == -1 and ("record %d " % len(front)) in str(ei.value), str(ei.value)
        assert (out.read_bytes() == old) if old is not None else not out.exists()
        assert leftovers(d) == [] and path.read_bytes() == before
        if out.exists():
            out.unlink()
    for same in (str(d / "front.bam"), str(d) + "/./front.bam"):                                # the output may not be the input
        with pytest.raises(GceError) as ei:
            umi(d / "front.bam", same)
        assert ei.value.status == -1 and "input" in str(ei.value) and leftovers(d) == []


@pytest.mark.gpu
def test_budget_forces_flushes(casefile):
    """record bytes that dominate one window: within half the device memory an unbounded run took, the cap that the budget leaves makes the
    pass flush, it stays within the budget and writes the same records"""
    d, _ = casefile
    big = uc.big_record()[0]
    path = d / "budget.bam"
    write(path, ([big] + uc.file_records()) * 50, block=M)
    for lv in (1, -2):
        r0 = umi(path, d / "budget.free.bam", "RX", 200000, lv)
        assert r0.n_flushes == 0 and r0.peak_device_bytes > r0.out_record_bytes
        if lv == 1:
            check(path, "RX", d / "budget.free.bam", r0)
        budget = r0.peak_device_bytes // 2
        r = umi(path, d / "budget.out.bam", "RX", 200000, lv, budget=budget)
        print("level=%d: unbounded peak_device_bytes=%d; budget=%d peak_device_bytes=%d n_flushes=%d" % (lv, r0.peak_device_bytes, budget, r.peak_device_bytes, r.n_flushes))
        assert 0 < r.peak_device_bytes <= budget and r.n_flushes >= 1
        assert (d / "budget.out.bam").read_bytes() == (d / "budget.free.bam").read_bytes()
        assert {k: getattr(r, k) for k in COUNTERS} == {k: getattr(r0, k) for k in COUNTERS} and leftovers(d) == []


# ---------------------------------------------------------------- against the file that carries the MI, against the oracle, the command line
@pytest.fixture(scope="module")
def streams(built, tmp_path_factory):
    """per style: A.bam (the UMIs in RX, or in the names), B.bam (the same records with the MI the pass must write) and ref.fa"""
    d = tmp_path_factory.mktemp("umie2e")
    out = {}
    for style in ("RX", "name"):
        ref, targets, a, b = uc.stream(style)
        pybam.write_bam(str(d / ("A_%s.bam" % style)), a, targets, block=700)
        pybam.write_bam(str(d / ("B_%s.bam" % style)), b, targets, block=700)
        (d / "ref.fa").write_text(">c0\n" + ref + "\n")
        out[style] = (ref, a, b)
    return d, out


@pytest.mark.gpu
@pytest.mark.parametrize("style", ["RX", "name"])
def test_equal_to_the_file_with_mi_by_construction(streams, style):
    """file A has aux_pre=[RX], NM and no MI (or the UMI in its names); file B is the same records with mi=":"+norm(u), which pybam places
    behind NM, where the pass appends it: the pass's records on A are B's, byte for byte"""
    d, s = streams
    a, b = d / ("A_%s.bam" % style), d / ("B_%s.bam" % style)
    for w, resident in ((0, 0), (1500, M)):
        r = umi(a, d / "A.mi.bam", style, w, resident=resident)
        got, want = pysort.records(d / "A.mi.bam"), pysort.records(b)
        assert got[1] == want[1] and len(got[1]) == r.n_tagged == r.n_records > 200 and r.n_mi_dropped == 0
        assert pysort.inflate((d / "A.mi.bam").read_bytes()) == pysort.inflate(b.read_bytes())
    r = umi(b, d / "B.mi.bam", style)                              # and B is a fixed point
    assert pysort.records(d / "B.mi.bam")[1] == pysort.records(b)[1] and r.n_mi_dropped == r.n_tagged == r.n_records


@pytest.mark.gpu
@pytest.mark.parametrize("style", ["RX", "name"])
def test_end_to_end_against_the_oracle(streams, oracle, style):
    """umi_to_mi, then run_bam with an empty umi_prefix: the records and both Stats blocks are the oracle's on the batch built with the mi
    values of file B (tests/test_umi_model.py shows that the oracle emits fewer records when it does not see them)"""
    from gencore_amd.bamio import run_bam
    from gencore_amd.batch import ReadBatch
    from gencore_amd.capi import default_params
    d, s = streams
    ref, a, b = s[style]
    batch = ReadBatch.from_records(b)
    tl = np.asarray([len(ref)], np.uint32)
    want = oracle.run(batch, default_params(n_targets=1, target_len=tl.ctypes.data, flush_period=40, umi_prefix=""), [(oracle.pack_reference(ref), len(ref))])
    assert want.status == 0
    mi, out = d / ("A_%s.mi.bam" % style), d / ("A_%s.out.bam" % style)
    r = umi(d / ("A_%s.bam" % style), mi, style)
    assert r.n_tagged == batch.n
    run = run_bam(str(mi), str(out), default_params(flush_period=40, umi_prefix=""), fasta=str(d / "ref.fa"), threads=2, chunk_reads=50)
    assert run.n_reads == batch.n and run.n_out == len(want.emitted()) and 0 < run.n_out < batch.n
    assert bytes(run.pre) == bytes(want.pre) and bytes(run.post) == bytes(want.post)
    _, _, got = pybam.read_bam(str(out))
    key = lambda r: (r["tid"], r["pos"], r["qname"], r["flag"], r["seq"])
    exp = sorted(({**r, "qname": r["qname"].rstrip("\0")} for r in want.records(batch)), key=key)
    assert len(got) == len(exp)
    for g, e in zip(sorted(got, key=key), exp):
        assert (g["qname"], g["flag"], g["pos"], g["seq"], g["qual"]) == (e["qname"], e["flag"], e["pos"], e["seq"], e["qual"])
        assert g["aux"].get("FR", (None, -1))[1] == e["fr"] and g["aux"]["MI"][0] == "Z" and g["aux"]["MI"][1].startswith(":")
    # the premise, on the GPU: without the pass the run sees no UMI and emits fewer records
    bare = run_bam(str(d / ("A_%s.bam" % style)), str(d / "bare.bam"), default_params(flush_period=40, umi_prefix=""), fasta=str(d / "ref.fa"), threads=2, chunk_reads=50)
    assert 0 < bare.n_out < run.n_out


def cli(args, cwd, timeout=120):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "gencore_amd"] + list(args), cwd=str(cwd), env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.mark.gpu
def test_cli_umi_from(streams):
    """-i A.bam --umi_from RX against the same command on B without the flag: equal records, equal reports but for `command`, the umi: line
    on stderr, no temporary file left; the same under a --device_memory (this file is one window of the 64 MB the command line reads with,
    and a flush needs a second one: test_cli_device_memory_forces_a_flush is where the command line's budget makes the pass flush)"""
    d, s = streams
    n = len(s["RX"][1])
    base = ["-r", "ref.fa", "--threads", "2"]
    b = cli(["-i", "B_RX.bam", "-o", "b.bam", "-j", "b.json"] + base, d)
    assert b.returncode == 0, b.stderr
    want = pysort.records(d / "b.bam")[1]
    jb = json.loads((d / "b.json").read_text())
    assert "--umi_from" not in jb.pop("command") and 0 < len(want) < n
    for name, src, more in (("a", "RX", []), ("m", "RX", ["--device_memory", "1.5"]), ("n", "name", [])):
        a = cli(["-i", "A_%s.bam" % src, "--umi_from", src, "-o", name + ".bam", "-j", name + ".json"] + base + more, d)
        assert a.returncode == 0, a.stderr
        assert "umi: %d records, MI written in %d, no source in 0, not a UMI in 0\n" % (n, n) in a.stderr
        ja = json.loads((d / (name + ".json")).read_text())
        assert "--umi_from " + src in ja.pop("command")
        got = pysort.records(d / (name + ".bam"))[1]
        if src == "RX":
            assert got == want and ja == jb
        else:                                                   # (other names, the same molecules)
            assert len(got) == len(want)
        assert [p.name for p in d.iterdir() if p.name.startswith("gencore_umi_") or ".tmp" in p.name] == []


@pytest.fixture(scope="module")
def windows3(built, tmp_path_factory):
    """synth.bam: 400 000 cfg3 pairs in stored members, 244 MB: four windows of the 64 MB the command line reads with (the file of
    tests/test_calmd_stream_gpu.py's budget test); with ref.fa.  Its records have no RX and fastp names: the pass copies every one."""
    import torch
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    from test_calmd_gpu import write_fasta
    d = tmp_path_factory.mktemp("umimem")
    s = synth.generate("cfg3", n_pairs=400000, scale=0.002, device=torch.device("cuda:0"))
    tl = np.asarray(s.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(str(d / "synth.bam"), s.to_batch(), tl, names, threads=4, level=0)
    write_fasta(d / "ref.fa", names, s.reference_host())
    assert os.path.getsize(str(d / "synth.bam")) > 3 * (64 << 20)
    return d


@pytest.mark.gpu
def test_cli_device_memory_forces_a_flush(windows3):
    """--umi_from under a --device_memory of 0.95 of what the pass took without one, on a file of four windows (the run itself needs 0.61 GB
    beside a pass's reads, and the pass holds back a second window's room and its deflate buffers, so it flushes well above 0.8 of its
    peak): at that budget the pass flushes (shown on the library call the command line makes) and the command's output and report are those
    of the run without a budget"""
    d = windows3
    r0 = umi(d / "synth.bam", d / "p0.bam", "RX")
    x = r0.peak_device_bytes * 95 // 100
    r1 = umi(d / "synth.bam", d / "p1.bam", "RX", budget=x)
    print("unbounded: peak_device_bytes=%d n_flushes=%d; budget %d: peak_device_bytes=%d n_flushes=%d" % (r0.peak_device_bytes, r0.n_flushes, x, r1.peak_device_bytes, r1.n_flushes))
    assert r0.n_flushes == 0 and r1.n_flushes >= 1 and 0 < r1.peak_device_bytes <= x
    assert (d / "p1.bam").read_bytes() == (d / "p0.bam").read_bytes() and r1.n_no_source == r1.n_records == r0.n_records > 0
    (d / "p0.bam").unlink(), (d / "p1.bam").unlink()
    base = ["-i", "synth.bam", "-r", "ref.fa", "-s", "2", "--threads", "4", "--level", "-2", "--umi_from", "RX"]
    a = cli(base + ["-o", "m0.bam", "-j", "m0.json"], d)
    assert a.returncode == 0, a.stderr
    b = cli(base + ["-o", "m1.bam", "-j", "m1.json", "--device_memory", repr(x / float(1 << 30))], d)
    assert b.returncode == 0, b.stderr
    line = "umi: %d records, MI written in 0, no source in %d, not a UMI in 0\n" % (r0.n_records, r0.n_records)
    assert line in a.stderr and line in b.stderr
    assert pysort.inflate((d / "m1.bam").read_bytes()) == pysort.inflate((d / "m0.bam").read_bytes()) and len(pysort.records(d / "m1.bam")[1]) > 0
    ja, jb = json.loads((d / "m0.json").read_text()), json.loads((d / "m1.json").read_text())
    assert "--device_memory" not in ja.pop("command") and "--device_memory" in jb.pop("command")
    assert ja == jb
    assert [p.name for p in d.iterdir() if p.name.startswith("gencore_umi_") or ".tmp" in p.name] == []
