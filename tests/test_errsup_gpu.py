"""gce_bam_error_profile_support on the GPU: the scan (k_reduce_scan over the tag walk) and k_sup_count, collecting a record's adds
on chip and with direct atomics (direct=True), against the model (tests/pyerrsup.py) and the hand-written rows (tests/supcases.py): every
integer equal, so the two variants equal each other.  The cases are the smallest at which the kernels can go wrong: every hand case with the
table's bytes, the 32-record steps and the grid's stride, l_seq around the 16 lanes of a slot and at 1024, 1024 adds to one counter, a record
of inserted bases alone, records cut between windows, neighbouring slots with different rows and a block of equal ones, the cycle table of
gce_bam_error_profile_masked as a second reference, a duplex run end to end, the command line, the session's call order and the budget."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import errprofcases as ec
import maskcases as mc
import pyerrmask
import pyerrprof
import pyerrsup
import supcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_errsup.hpp")).read()
STEP, GRID, LOW = (int(re.search(r"#define %s (\d+)u" % n, SRC).group(1)) for n in ("ES_STEP_RECS", "ES_GRID", "ES_LOW"))
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["onchip", "direct"])
BIG_NAMES, BIG_LENS = ["c0", "c1"], [20000, 3000]
BIG_FASTA = {"c0": "".join("ACGT"[i] for i in np.random.RandomState(61).randint(0, 4, 20000)), "c1": "A" * 3000}
SKIP_FIELDS = ["n_records", "n_eligible"] + pyerrsup.SKIPS


def same(run, res):
    """an ErrorProfileSupportRun against the model's dict: every counter of classes 0..23, every skip, the totals"""
    assert run.counts.dtype == np.uint64 and run.counts.shape == (3, 33, 33, 24)
    want = np.array(res["counts"], np.uint64)
    assert (run.counts == want).all(), [(tuple(i), int(run.counts[tuple(i)]), int(want[tuple(i)])) for i in np.argwhere(run.counts != want)[:8]]
    for k in SKIP_FIELDS + ["n_with_forward", "n_with_reverse", "n_bases", "n_mismatches", "n_intervals"]:
        assert getattr(run, k) == res[k], k
    if hasattr(run, "n_masked_events"):
        assert run.n_masked_events == res["n_masked_events"]


def run_files(tmp_path, records, names, lens, fasta, direct, bed=None, mask=None, tag="x", block=0xff00, tags=("FR", "RR"), **kw):
    """records (bytes), fasta = {name: bases}, bed = None or [(contig name, start, end)] and mask = None or VCF text as files, through
    error_profile_support_bam -> (the run, the model's result)"""
    from gencore_amd.bamio import error_profile_support_bam
    bam, fa, bedf, mf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.fa" % tag), tmp_path / ("%s.bed" % tag), tmp_path / ("%s.vcf" % tag)
    if not bam.exists():
        ec.write_raw_bam(str(bam), records, names, lens, block)
        fa.write_text(ec.fasta_text(fasta))
    if bed is not None:
        bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    if mask is not None:
        mf.write_bytes(mask)
    run = error_profile_support_bam(bam, fa, mask=None if mask is None else mf, bed=None if bed is None else bedf, direct=direct, threads=2, tags=tags, **kw)
    refs = [fasta.get(nm) for nm in names]
    regions = None if bed is None else [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    ivs = None if mask is None else pyerrmask.load(mf, names, pyerrmask.clamp_lens(lens, refs))["intervals"]
    res = pyerrsup.profile(records, refs, lens, ivs, regions, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704), tags)
    return run, res


@pytest.mark.gpu
@VARIANTS
def test_hand_cases(built, tmp_path, direct):
    """every case of supcases through the file: the rows written out by hand, the model's counters, and the table's text byte for byte"""
    for cs in sc.all_cases():
        tsv = tmp_path / (cs["label"] + ".tsv")
        run, res = run_files(tmp_path, cs["records"], ec.NAMES, ec.LENS, ec.FASTA, direct, bed=cs["bed"], mask=None if cs["mask"] is None else mc.mask_vcf(cs["mask"]), tag=cs["label"],
                             tags=cs["tags"], tsv=tsv, min_mapq=cs["min_mapq"], min_baseq=cs["min_baseq"], exclude_flags=cs["exclude"])
        same(run, res)
        assert pyerrsup.nonzero(dict(counts=run.counts.tolist())) == sc.expected(cs), cs["label"]
        assert {k: getattr(run, k) for k in pyerrsup.SKIPS} == cs["skips"], cs["label"]
        assert run.n_eligible == len(cs["records"]) - sum(cs["skips"].values()) and not run.counts[..., 23].any()
        assert tsv.read_bytes() == pyerrsup.table(res, cs["mask"] is not None), cs["label"]
        assert run.peak_device_bytes > 0 and run.total_s > 0
    assert not [p.name for p in tmp_path.iterdir() if ".tmp" in p.name]


def fr(f, r=None):
    return sc.num("FR", "C", f) + (b"" if r is None else sc.num("RR", "C", r))


def read_at(k, n, flag, aux, pos=100):
    """read k of n aligned bases copied from c0 with every seventh base changed"""
    ref = BIG_FASTA["c0"][pos + k:pos + k + n]
    return ec.rec(0, pos + k, "%dM" % n, "".join("ACGT"[("ACGT".index(b) + 1) % 4] if i % 7 == 3 else b for i, b in enumerate(ref)), flag=flag, aux=aux)


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("n", [1, STEP - 1, STEP, STEP + 1, GRID * STEP + 1])
def test_whole_and_partial_steps(built, tmp_path, direct, n):
    """windows of 1, 31, 32 and 33 records: one slot, one short of a step, a whole step, one past it; and one record more than a whole grid's
    steps, which block 0 takes in its second step"""
    if n > 1000:
        recs = [read_at(k % 1000, 3, 0x40 if k & 1 else 0x90, fr(1 + k % 3, None if k % 5 else 2), pos=7) for k in range(n)]
    else:
        recs = [ec.rec(0, 10 + 3 * k, "2M1D2M", "ACGT", flag=16 * (k % 3 == 0), aux=fr(1 + k % 4, None if k % 2 else 1 + k % 3)) for k in range(n)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct)
    same(run, res)
    assert run.n_eligible == n and run.counts[..., 22].sum() == n and run.counts[..., :16].sum() == (3 if n > 1000 else 4) * n


@pytest.mark.gpu
@VARIANTS
def test_lengths_and_one_counter(built, tmp_path, direct):
    """l_seq 1, 15, 16, 17 and 1024 on both strands: fewer columns than a slot has lanes, one per lane, one more, and 64 per lane.  c1 is all A:
    a 1024M read of A is 1024 adds to ONE counter of its row, which whatever packing the kernel uses has to survive, and a second such read
    makes it 2048; 1024 columns below min_baseq are 1024 LOWQ.  A record of inserted bases alone has no column and no reference base"""
    recs = [read_at(7 * j, n, flag, fr(1 + j, j or None)) for j, n in enumerate((1, 15, 16, 17, 1024)) for flag in (0, 0x10)]
    recs += [ec.rec(1, 5, "1024M", "A" * 1024, aux=fr(7, 7), flag=0x40)] * 2 + [ec.rec(1, 9, "1024M", "A" * 1024, [3] * 1024, aux=fr(8), flag=0x80)]
    recs += [ec.rec(1, 50, "5I", "ACGTA", aux=fr(9, 9)), ec.rec(1, 50, "3S1024I", lseq=None, seq="A" * 1027, aux=fr(9, 9))]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, min_baseq=10)
    same(run, res)
    assert run.counts[1, 7, 7, 0] == 2048 and run.counts[1, 7, 7, 22] == 2 and run.counts[1, 7, 7].sum() == 2050
    assert run.counts[2, 8, 0, pyerrprof.LOWQ] == 1024 and run.counts[0, 9, 9, pyerrprof.INS] == 5 and run.counts[0, 9, 9].sum() == 6 and run.n_too_long == 1
    assert [int(run.counts[0, 1 + j, j, :16].sum()) for j in range(5)] == [2, 30, 32, 34, 2048]


@pytest.mark.gpu
@VARIANTS
def test_slots_of_a_wave_and_of_a_block(built, tmp_path, direct):
    """four neighbouring slots of one wave carry four different (f, r), over a whole block and a second step; then all 32 slots of a block
    carry the same (f, r), so every flush of the block meets on one row"""
    rows = [(1, None), (2, 1), (32, 32), (None, 5)]
    aux = [(b"" if f is None else sc.num("FR", "C", f)) + (b"" if r is None else sc.num("RR", "S", r)) for f, r in rows]
    recs = [read_at(k, 20 + k % 9, (0, 0x50, 0x80)[k % 3], aux[k % 4]) for k in range(2 * STEP + 4)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="four")
    same(run, res)
    assert sorted({(f, r) for g, f, r, cl in pyerrsup.nonzero(res)}) == [(0, 5), (1, 0), (2, 1), (32, 32)]
    assert [int(run.counts[:, f, r, 22].sum()) for f, r in ((1, 0), (2, 1), (32, 32), (0, 5))] == [17] * 4
    recs = [read_at(k, 40, 0x40, fr(3, 2)) for k in range(STEP)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="one")
    same(run, res)
    assert run.counts[1, 3, 2, 22] == STEP and run.counts[1, 3, 2, :16].sum() == 40 * STEP and run.counts.sum() == 41 * STEP


@pytest.mark.gpu
@VARIANTS
def test_block_table_edges(built, tmp_path, direct):
    """rows at the edge of the block's table in LDS: both buckets ES_LOW - 1 (the table's last row of a segment), either one or both ES_LOW
    (memory), absent with ES_LOW - 1 and with ES_LOW, mixed within one step so that table rows and memory rows leave neighbouring slots, over
    several blocks and a second step of block 0, in all three segments; then one row of the table alone from every slot of many blocks"""
    assert 2 <= LOW <= 31
    rows = [(LOW - 1, LOW - 1), (LOW, LOW - 1), (LOW - 1, LOW), (LOW, LOW), (None, None), (LOW - 1, None), (None, LOW), (1, 1), (32, 1), (None, LOW - 1)]
    aux = [(b"" if f is None else sc.num("FR", "C", f)) + (b"" if r is None else sc.num("RR", "C", r)) for f, r in rows]
    recs = [read_at(k % 3000, 10 + k % 23, (0x40, 0x90, 0)[k % 3], aux[k % len(aux)]) for k in range(GRID * STEP + 3 * STEP)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="edges")
    same(run, res)
    assert {(f, r) for g, f, r, cl in pyerrsup.nonzero(res)} == {(f or 0, r or 0) for f, r in rows} and run.counts[..., 22].sum() == len(recs)
    assert all(run.counts[g, LOW - 1, LOW - 1, 22] > 0 and run.counts[g, LOW, LOW, 22] > 0 for g in range(3))
    recs = [read_at(k % 50, 30, 0x80, fr(LOW - 1, LOW - 1)) for k in range(40 * STEP)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="last")
    same(run, res)
    assert run.counts[2, LOW - 1, LOW - 1, 22] == 40 * STEP and run.counts.sum() == 31 * 40 * STEP


def window_records():
    """test_errprof_gpu.window_records' shape with a seed of its own and supcases' optional fields"""
    rng = np.random.RandomState(37)
    recs = []
    for k in range(400):
        n = int(rng.randint(20, 200))
        ops = [(4, int(rng.randint(1, 5)))] * int(rng.randint(0, 2)) + [(0, n), (int(rng.choice([1, 2, 3])), int(rng.randint(1, 6))), (0, int(rng.randint(1, 30)))]
        nq = sum(ln for op, ln in ops if op in (0, 1, 4))
        seq = "".join("ACGTN"[i] for i in rng.choice(5, nq, p=[.24, .24, .24, .24, .04]))
        recs.append(ec.rec(int(k >= 300), int(rng.randint(0, 2500)), ops, seq, rng.randint(0, 41, nq).tolist(), flag=int(rng.choice([0, 16, 0x40, 0x50, 0x80, 0x90, 0x400])),
                           mapq=int(rng.randint(0, 61)), name="read%04d" % k, aux=sc.random_aux(rng)))
    recs.insert(150, ec.rec(0, 100, "1000M", "".join("ACGT"[i] for i in rng.randint(0, 4, 1000)), rng.randint(0, 41, 1000).tolist(), aux=fr(2, 2)))     # larger than a window
    return recs


@pytest.fixture(scope="module")
def random_case():
    """the random records and a mask of every eleventh position as VCF text, once"""
    text = mc.vcf(*[(nm, x + 1, "N", "<DEL>") for nm, ln in zip(BIG_NAMES, BIG_LENS) for x in range(3, ln, 11)])
    return window_records(), text


@pytest.mark.gpu
@VARIANTS
def test_windows_and_the_cycle_table(built, tmp_path, random_case, direct):
    """random records under a BED and a mask, members of 300 bytes: one window against windows of 1000 bytes, more than three, where most records
    straddle two and one is larger than a window; and summed over (forward, reverse) the table is gce_bam_error_profile_masked's summed over
    cycles on the same files, with its first nine counters and no record in n_bad_aux"""
    from gencore_amd.bamio import error_profile_masked_bam
    recs, text = random_case
    bed = [("c0", 50, 400), ("c0", 1000, 1300), ("c0", 5000, 6500), ("c1", 0, 3000)]
    for tag, b in (("nobed", None), ("bed", bed)):
        one, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, bed=b, mask=text, tag=tag, block=300, min_baseq=13, min_mapq=5)
        same(one, res)
        assert os.path.getsize(str(tmp_path / (tag + ".bam"))) > 3 * 1000
        cut, _ = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, bed=b, mask=text, tag=tag, block=300, min_baseq=13, min_mapq=5, window_bytes=1000)
        same(cut, res)
        assert (cut.counts == one.counts).all()
        cyc = error_profile_masked_bam(tmp_path / (tag + ".bam"), tmp_path / (tag + ".fa"), tmp_path / (tag + ".vcf"), bed=None if b is None else tmp_path / (tag + ".bed"), direct=direct,
                                       min_baseq=13, min_mapq=5)
        assert (one.counts[..., :22].sum(axis=(1, 2)) == cyc.counts[..., :22].sum(axis=1)).all()
        assert [getattr(one, k) for k in SKIP_FIELDS[:10]] == [getattr(cyc, k) for k in SKIP_FIELDS[:10]] and one.n_bad_aux == 0
        assert (one.n_bases, one.n_mismatches, one.n_masked_events) == (cyc.n_bases, cyc.n_mismatches, cyc.n_masked_events) and one.n_masked_events > 50
        assert len({(f, r) for g, f, r, cl in pyerrsup.nonzero(res)}) > 15 and 0 < one.n_with_reverse < one.n_with_forward < one.n_eligible
        if b is None:
            assert one.counts[..., 22].sum() == one.n_eligible
        else:
            assert 0 < one.counts[..., 22].sum() < one.n_eligible


@pytest.fixture(scope="module")
def duplex(tmp_path_factory):
    """supcases' duplex stream as in.bam / ref.fa, and the oracle's result at cluster_size_req 1"""
    import pybam
    from gencore_amd.batch import ReadBatch
    from gencore_amd.capi import default_params
    from oracle import oracle_py
    d = tmp_path_factory.mktemp("errsupduplex")
    recs, ref = sc.duplex_stream()
    batch = ReadBatch.from_records(recs)
    tl = np.asarray([len(ref)], np.uint32)
    want = oracle_py.run(batch, default_params(n_targets=1, target_len=tl.ctypes.data, umi_prefix="UMI", cluster_size_req=1), [(oracle_py.pack_reference(ref), len(ref))])
    assert want.status == 0
    pybam.write_bam(str(d / "in.bam"), recs, [("c0", len(ref))])
    (d / "ref.fa").write_text(">c0\n" + ref + "\n")
    rows = Counter((e["fr"], max(e["rr"], 0)) for e in want.records(batch))
    assert all(1 <= f <= 31 and r <= 31 for f, r in rows) and sum(n for (f, r), n in rows.items() if r) > 20 and sum(n for (f, r), n in rows.items() if not r) > 5
    return d, rows, ref


@pytest.mark.gpu
@VARIANTS
def test_end_to_end_duplex(built, duplex, tmp_path, direct):
    """a duplex stream through run_bam at cluster_size_req 1, then the profile of its output: per (forward, reverse) the records column is the
    number of output records the oracle gives those FR / RR values (no RR: absent), and n_with_reverse is the number of duplex records"""
    from gencore_amd.bamio import error_profile_support_bam, run_bam
    from gencore_amd.capi import default_params
    d, rows, ref = duplex
    out = tmp_path / "out.bam"
    run = run_bam(str(d / "in.bam"), str(out), default_params(umi_prefix="UMI", cluster_size_req=1), fasta=str(d / "ref.fa"), threads=2)
    assert run.n_out == sum(rows.values())
    sup = error_profile_support_bam(out, d / "ref.fa", direct=direct, tsv=tmp_path / "s.tsv")
    got = {(f, r): int(sup.counts[:, f, r, 22].sum()) for f in range(33) for r in range(33) if sup.counts[:, f, r, 22].sum()}
    assert got == dict(rows)
    assert sup.n_with_reverse == sum(n for (f, r), n in rows.items() if r) and sup.n_with_forward == sup.n_eligible == sup.n_records == run.n_out and sup.n_bad_aux == 0
    names, lens, recs = sc.raw_records(out)
    res = pyerrsup.profile(recs, [ref], lens)
    same(sup, res)
    assert (tmp_path / "s.tsv").read_bytes() == pyerrsup.table(res)
    assert sup.counts[..., :21].sum() == 20 * run.n_out and sup.n_bases > 19 * run.n_out                        # every record is 20M: a column each, nearly all of them a base


@pytest.mark.gpu
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
def test_command_line(built, duplex, tmp_path, with_mask):
    """--error_profile_support through python -m gencore_amd at -s 1, without and with --error_profile_mask: the table is the model's over the
    written output and the stderr line carries its totals and the tags' names.  (The command line has no switch for the direct variant.)"""
    from test_cli_gpu import cli
    d, rows, ref = duplex
    (tmp_path / "m.vcf").write_bytes(mc.vcf(*[("c0", x + 1, "N", "<DEL>") for x in range(2, len(ref), 9)]))
    r = cli(["-i", str(d / "in.bam"), "-o", "out.bam", "-r", str(d / "ref.fa"), "-j", "r.json", "-u", "UMI", "-s", "1", "--threads", "2", "--error_profile_support", "s.tsv"]
            + (["--error_profile_mask", "m.vcf"] if with_mask else []), tmp_path)
    assert r.returncode == 0, r.stderr
    names, lens, recs = sc.raw_records(tmp_path / "out.bam")
    mask = pyerrmask.load(tmp_path / "m.vcf", names, lens)["intervals"] if with_mask else None
    res = pyerrsup.profile(recs, [ref], lens, mask)
    assert (tmp_path / "s.tsv").read_bytes() == pyerrsup.table(res, with_mask)
    line = "error_profile_support: %d records, %d eligible, %d bases, %d mismatches, %d with FR, %d with RR\n" % (
        res["n_records"], res["n_eligible"], res["n_bases"], res["n_mismatches"], res["n_with_forward"], res["n_with_reverse"])
    assert line in r.stderr and res["n_with_reverse"] == sum(n for (f, x), n in rows.items() if x) and res["n_records"] == sum(rows.values())
    assert ("events masked\n" in r.stderr) == with_mask and (res["n_masked_events"] > 100) == with_mask
    assert sorted(p.name for p in tmp_path.iterdir()) == ["m.vcf", "out.bam", "r.json", "s.tsv"]


@pytest.mark.gpu
def test_session_call_order(built):
    """the device object refuses calls out of order: the mask and the intervals in front of the reference, the reference twice, a window or
    the finish in front of the intervals, the intervals twice"""
    from gencore_amd import capi
    lib = capi.load_library()
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    lib.gce_errsup_create.argtypes = [C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_char_p, C.POINTER(vp)]
    lib.gce_errsup_destroy.argtypes, lib.gce_errsup_destroy.restype = [vp], None
    lib.gce_errsup_set_ref.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
    lib.gce_errsup_set_mask.argtypes = [vp, C.c_int64, i32p, i32p, i32p]
    lib.gce_errsup_set_sites.argtypes = [vp, C.c_int64, i32p, i32p, i32p]
    lib.gce_errsup_window.argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, vp, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    lib.gce_errsup_finish.argtypes = [vp, C.POINTER(C.c_int64), vp]
    p = vp()
    assert lib.gce_errsup_create(0, 0, 0, 0, 0x704, 1, None, C.byref(p)) == 0 and p.value
    try:
        out, counters, secs = np.zeros((3, 33, 33, 24), np.uint64), (C.c_int64 * 11)(), C.c_double(0)
        assert lib.gce_errsup_set_mask(p, 0, None, None, None) == -1 and lib.gce_errsup_set_sites(p, -1, None, None, None) == -1
        assert lib.gce_errsup_window(p, None, 0, 0, None, None, None, 0, 1, 1, C.byref(secs)) == -1 and lib.gce_errsup_finish(p, counters, out.ctypes.data) == -1
        seq = (C.c_char_p * 1)(b"ACGT")
        assert lib.gce_errsup_set_ref(p, 1, seq, (C.c_int64 * 1)(4)) == 0 and lib.gce_errsup_set_ref(p, 1, seq, (C.c_int64 * 1)(4)) == -1
        assert lib.gce_errsup_window(p, None, 0, 0, None, None, None, 0, 1, 1, C.byref(secs)) == -1
        assert lib.gce_errsup_set_mask(p, 0, None, None, None) == 0 and lib.gce_errsup_set_sites(p, -1, None, None, None) == 0 and lib.gce_errsup_set_sites(p, -1, None, None, None) == -1
        assert lib.gce_errsup_window(p, None, 0, 0, None, None, None, 0, 2, 1, C.byref(secs)) == -1            # (another number of contigs)
        assert lib.gce_errsup_finish(p, None, out.ctypes.data) == -1 and lib.gce_errsup_finish(p, counters, out.ctypes.data) == 0
        assert list(counters) == [0] * 11 and not out.any()
    finally:
        lib.gce_errsup_destroy(p)


OOM = re.compile(r"out of device memory: gce_bam_error_profile_support needs the reference bases \((\d+) bytes\) \+ 627264 bytes of counters \+ 16 bytes per interval \+ one window \+ "
                 r"4 bytes per window record \(\d+ bytes live, budget (\d+), (\d+) more for the reference bases\)")


@pytest.mark.gpu
@VARIANTS
def test_budget(built, tmp_path, direct):
    """a budget below the reference bases is GCE_ERR_OOM that names this pass, its counters and the reference bases that did not fit; no table
    and no temporary file is left"""
    from gencore_amd.bamio import error_profile_support_bam
    from gencore_amd.capi import GceError
    bam, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    ec.write_raw_bam(str(bam), [ec.rec(0, 10, "2M", aux=fr(2, 1))], ["c0"], [3 << 20])
    fa.write_text(">c0\n" + "ACGT" * (3 << 18) + "\n")
    with pytest.raises(GceError) as ei:
        error_profile_support_bam(bam, fa, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=1 << 20)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and str(ei.value).endswith(m.group(0)), str(ei.value)
    assert [int(x) for x in m.groups()[:2]] == [3 << 20, 1 << 20] and int(m.group(3)) > 3 << 20
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]
    run = error_profile_support_bam(bam, fa, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=64 << 20)
    assert run.n_eligible == 1 and run.n_bases == 2 and run.counts[0, 2, 1, 22] == 1 and 3 << 20 < run.peak_device_bytes <= 64 << 20
