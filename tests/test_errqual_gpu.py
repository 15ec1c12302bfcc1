"""gce_bam_error_profile_quality on the GPU: gce_bam_error_profile's scan and k_qual_count, with the block's table on chip
and with direct atomics (direct=True), against the model (tests/pyerrqual.py) and the hand-written rows (tests/qualcases.py):
every integer equal, so the two variants equal each other.  The cases are the smallest at which the kernels can go wrong: every hand case
with the table's bytes, the 32-record steps and the grid's stride, one key for a whole wave, 1024 adds to one counter, a key per lane, 64 keys in
a wave, a key that changes at every step of a lane, l_seq around the 16 lanes of a slot, a short and a long record side by side, records cut
between windows, the cycle table of gce_bam_error_profile_masked as a second reference, the command line, the session's call order and the
budget."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import errprofcases as ec
import maskcases as mc
import pyerrmask
import pyerrprof
import pyerrqual
import qualcases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_errqual.hpp")).read()
STEP, GRID = (int(re.search(r"#define %s (\d+)u" % n, SRC).group(1)) for n in ("EQ_STEP_RECS", "EQ_GRID"))
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["onchip", "direct"])
BIG_NAMES, BIG_LENS = ["c0", "c1"], [20000, 3000]
BIG_FASTA = {"c0": "".join("ACGT"[i] for i in np.random.RandomState(67).randint(0, 4, 20000)), "c1": "A" * 3000}
SKIP_FIELDS = ["n_records", "n_eligible"] + pyerrqual.SKIPS
AA = 0                                                                                # the class A>A


def same(run, res):
    """an ErrorProfileQualityRun against the model's dict: every counter of classes 0..23, every skip, the totals"""
    assert run.counts.dtype == np.uint64 and run.counts.shape == (3, 96, 24)
    want = np.array(res["counts"], np.uint64)
    assert (run.counts == want).all(), [(tuple(i), int(run.counts[tuple(i)]), int(want[tuple(i)])) for i in np.argwhere(run.counts != want)[:8]]
    for k in SKIP_FIELDS + ["n_bases", "n_mismatches", "n_intervals"]:
        assert getattr(run, k) == res[k], k
    if hasattr(run, "n_masked_events"):
        assert run.n_masked_events == res["n_masked_events"]


def run_files(tmp_path, records, names, lens, fasta, direct, bed=None, mask=None, tag="x", block=0xff00, **kw):
    """records (bytes), fasta = {name: bases}, bed = None or [(contig name, start, end)] and mask = None or VCF text as files, through
    error_profile_quality_bam -> (the run, the model's result)"""
    from gencore_amd.bamio import error_profile_quality_bam
    bam, fa, bedf, mf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.fa" % tag), tmp_path / ("%s.bed" % tag), tmp_path / ("%s.vcf" % tag)
    if not bam.exists():
        ec.write_raw_bam(str(bam), records, names, lens, block)
        fa.write_text(ec.fasta_text(fasta))
    if bed is not None:
        bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    if mask is not None:
        mf.write_bytes(mask)
    run = error_profile_quality_bam(bam, fa, mask=None if mask is None else mf, bed=None if bed is None else bedf, direct=direct, threads=2, **kw)
    refs = [fasta.get(nm) for nm in names]
    regions = None if bed is None else [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    ivs = None if mask is None else pyerrmask.load(mf, names, pyerrmask.clamp_lens(lens, refs))["intervals"]
    res = pyerrqual.profile(records, refs, lens, ivs, regions, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704))
    return run, res


@pytest.mark.gpu
@VARIANTS
def test_hand_cases(built, tmp_path, direct):
    """every case of qualcases through the file: the rows written out by hand, the model's counters, and the table's text byte for byte"""
    for cs in qc.all_cases():
        tsv = tmp_path / (cs["label"] + ".tsv")
        run, res = run_files(tmp_path, cs["records"], ec.NAMES, ec.LENS, ec.FASTA, direct, bed=cs["bed"], mask=None if cs["mask"] is None else mc.mask_vcf(cs["mask"]), tag=cs["label"],
                             tsv=tsv, min_mapq=cs["min_mapq"], min_baseq=cs["min_baseq"], exclude_flags=cs["exclude"])
        same(run, res)
        assert pyerrqual.nonzero(dict(counts=run.counts.tolist())) == qc.expected(cs), cs["label"]
        assert {k: getattr(run, k) for k in pyerrqual.SKIPS} == cs["skips"], cs["label"]
        assert run.n_eligible == len(cs["records"]) and not run.counts[..., 22:].any()
        assert tsv.read_bytes() == pyerrqual.table(res, cs["mask"] is not None), cs["label"]
        assert run.peak_device_bytes > 0 and run.total_s > 0
    assert not [p.name for p in tmp_path.iterdir() if ".tmp" in p.name]


def read_at(k, n, flag, qual, pos=100, tid=0):
    """read k of n aligned bases copied from the contig with every seventh base changed; qual: a list, or one value for all"""
    ref = BIG_FASTA[BIG_NAMES[tid]][pos + k:pos + k + n]
    seq = "".join("ACGT"[("ACGT".index(b) + 1) % 4] if i % 7 == 3 else b for i, b in enumerate(ref))
    return ec.rec(tid, pos + k, "%dM" % n, seq, qual if isinstance(qual, list) else [qual] * n, flag=flag)


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("n", [1, STEP - 1, STEP, STEP + 1, GRID * STEP + 1])
def test_whole_and_partial_steps(built, tmp_path, direct, n):
    """windows of 1, 31, 32 and 33 records: a wave with one live slot, one short of a step, a whole step, one past it; and one record more
    than a whole grid's steps, which block 0 takes in its second trip"""
    if n > 1000:
        recs = [read_at(k % 1000, 3, 0x40 if k & 1 else 0x90, [37, 25, 11][k % 3], pos=7) for k in range(n)]
    else:
        recs = [ec.rec(0, 10 + 3 * k, "2M1D2M", "ACGT", [37, 25, 11, 2][k % 4:] + [37, 25, 11, 2][:k % 4], flag=16 * (k % 3 == 0)) for k in range(n)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct)
    same(run, res)
    assert run.n_eligible == n and run.counts[..., :16].sum() == (3 if n > 1000 else 4) * n and run.counts.sum() == (3 if n > 1000 else 5) * n


@pytest.mark.gpu
@VARIANTS
def test_one_key_for_a_wave_and_one_run(built, tmp_path, direct):
    """c1 is all A.  Four neighbouring records of 20 A, all of quality 37: every add of the wave has one key, A>A in row 37.  Then a read of
    1024 A of one quality: one counter takes 1024 adds, 64 per lane, which whatever merges adds in front of the table has to carry to the record's end; two such
    reads make 2048, and
    1024 columns below min_baseq are 1024 LOWQ in their own row"""
    recs = [ec.rec(1, 5 + k, "20M", "A" * 20, [37] * 20) for k in range(4)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="wave")
    same(run, res)
    assert run.counts[0, 37, AA] == 80 and run.counts.sum() == 80
    recs = [ec.rec(1, 5, "1024M", "A" * 1024, [37] * 1024, flag=0x40)] * 2 + [ec.rec(1, 9, "1024M", "A" * 1024, [3] * 1024, flag=0x80)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="run", min_baseq=10)
    same(run, res)
    assert run.counts[1, 37, AA] == 2048 and run.counts[2, 3, pyerrprof.LOWQ] == 1024 and run.counts.sum() == 3072


@pytest.mark.gpu
@VARIANTS
def test_keys_per_lane_wave_and_step(built, tmp_path, direct):
    """every lane its own key: 16 consecutive qualities that all differ; 64 distinct keys in one wave: four neighbouring records of 16 bases
    over 64 qualities; a key that changes at every step of a lane: 64 bases whose qualities alternate between columns 16 apart"""
    recs = [ec.rec(1, 5, "16M", "A" * 16, list(range(20, 36)))]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="lane")
    same(run, res)
    assert (run.counts[0, 20:36, AA] == 1).all() and run.counts.sum() == 16
    recs = [ec.rec(1, 5 + k, "16M", "A" * 16, list(range(16 * k, 16 * k + 16))) for k in range(4)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="wave64")
    same(run, res)
    assert (run.counts[0, :64, AA] == 1).all() and run.counts.sum() == 64
    recs = [ec.rec(1, 5 + k, "64M", "A" * 64, [30 if (i // 16) & 1 else 20 for i in range(64)], flag=16 * (k & 1)) for k in range(3)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="alternate")
    same(run, res)
    assert run.counts[0, 20, AA] == 64 and run.counts[0, 30, AA] == 64 and run.counts[0, 20, 15] == 32 and run.counts[0, 30, 15] == 32 and run.counts.sum() == 192


@pytest.mark.gpu
@VARIANTS
def test_lengths(built, tmp_path, direct):
    """l_seq 1, 15, 16 and 17 on both strands: fewer columns than a slot has lanes, one per lane, one more; then lengths 1 and 1024 in
    neighbouring slots of one wave, the short record's lanes done while the long one's run on; a record of inserted bases alone has no column"""
    recs = [read_at(7 * j, n, flag, [37, 25, 11][j % 3]) for j, n in enumerate((1, 15, 16, 17)) for flag in (0, 0x10)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="short")
    same(run, res)
    assert [int(run.counts[0, q, :16].sum()) for q in (37, 25, 11)] == [2 + 34, 30, 32]
    recs = [read_at(0, 1, 0, 37), read_at(3, 1024, 0, 25), read_at(9, 1, 0x10, 37), read_at(11, 1024, 0x10, [11, 37] * 512), ec.rec(1, 50, "5I", "ACGTA", [7] * 5)]
    run, res = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, tag="mixed")
    same(run, res)
    assert run.counts[0, 37, :16].sum() == 2 + 512 and run.counts[0, 25, :16].sum() == 1024 and run.counts[0, 11, :16].sum() == 512 and run.counts[0, 7, pyerrprof.INS] == 5


def window_records():
    """test_errprof_gpu.window_records' shape with a seed of its own and qualcases' qualities: binned in most records, any byte in some,
    none in a few"""
    rng = np.random.RandomState(41)
    recs = []
    for k in range(400):
        n = int(rng.randint(20, 200))
        ops = [(4, int(rng.randint(1, 5)))] * int(rng.randint(0, 2)) + [(0, n), (int(rng.choice([1, 2, 3])), int(rng.randint(1, 6))), (0, int(rng.randint(1, 30)))]
        nq = sum(ln for op, ln in ops if op in (0, 1, 4))
        seq = "".join("ACGTN"[i] for i in rng.choice(5, nq, p=[.24, .24, .24, .24, .04]))
        kind = rng.rand()
        qual = "*" if kind < 0.05 else rng.randint(0, 256, nq).tolist() if kind < 0.2 else rng.choice([2, 11, 25, 37], nq, p=[.05, .1, .15, .7]).tolist()
        recs.append(ec.rec(int(k >= 300), int(rng.randint(0, 2500)), ops, seq, qual, flag=int(rng.choice([0, 16, 0x40, 0x50, 0x80, 0x90, 0x400])), mapq=int(rng.randint(0, 61)),
                           name="read%04d" % k))
    recs.insert(150, ec.rec(0, 100, "1000M", "".join("ACGT"[i] for i in rng.randint(0, 4, 1000)), rng.choice([11, 25, 37], 1000).tolist()))     # larger than a window
    return recs


@pytest.fixture(scope="module")
def random_case():
    """the random records and a mask of every eleventh position as VCF text, once"""
    text = mc.vcf(*[(nm, x + 1, "N", "<DEL>") for nm, ln in zip(BIG_NAMES, BIG_LENS) for x in range(3, ln, 11)])
    return window_records(), text


@pytest.mark.gpu
@VARIANTS
def test_windows_and_the_cycle_table(built, tmp_path, random_case, direct):
    """random records under a BED, a mask, min_baseq 13 and min_mapq 5, members of 300 bytes: one window against windows of 1000 bytes, more
    than three, where most records straddle two and one is larger than a window; and summed over the buckets the table is
    gce_bam_error_profile_masked's summed over cycles on the same files, per segment and class, with its counters, and without the mask
    gce_bam_error_profile's"""
    from gencore_amd.bamio import error_profile_bam, error_profile_masked_bam
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
        assert (one.counts[..., :22].sum(axis=1) == cyc.counts[..., :22].sum(axis=1)).all()
        assert [getattr(one, k) for k in SKIP_FIELDS] == [getattr(cyc, k) for k in SKIP_FIELDS]
        assert (one.n_bases, one.n_mismatches, one.n_masked_events, one.n_intervals) == (cyc.n_bases, cyc.n_mismatches, cyc.n_masked_events, cyc.n_intervals) and one.n_masked_events > 50
        bare, res0 = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, direct, bed=b, tag=tag, block=300, min_baseq=13, min_mapq=5, window_bytes=1000)     # ... and without the mask
        same(bare, res0)
        cyc0 = error_profile_bam(tmp_path / (tag + ".bam"), tmp_path / (tag + ".fa"), bed=None if b is None else tmp_path / (tag + ".bed"), direct=direct, min_baseq=13, min_mapq=5)
        assert (bare.counts.sum(axis=1) == cyc0.counts.sum(axis=1)).all() and not bare.counts[..., 21:].any()
        assert [getattr(bare, k) for k in SKIP_FIELDS + ["n_bases", "n_mismatches"]] == [getattr(cyc0, k) for k in SKIP_FIELDS + ["n_bases", "n_mismatches"]]
        rows = {q for g, q, cl in pyerrqual.nonzero(res)}
        assert {2, 11, 25, 37, 94, 95} <= rows and len(rows) > 60 and one.counts[:, :13, pyerrprof.LOWQ].sum() > 0 and one.counts[:, 13:, pyerrprof.LOWQ].sum() == 0


@pytest.fixture(scope="module")
def duplex(tmp_path_factory):
    """supcases' duplex stream as in.bam / ref.fa"""
    import pybam
    import supcases as sc
    d = tmp_path_factory.mktemp("errqualduplex")
    recs, ref = sc.duplex_stream()
    pybam.write_bam(str(d / "in.bam"), recs, [("c0", len(ref))])
    (d / "ref.fa").write_text(">c0\n" + ref + "\n")
    return d, ref


@pytest.mark.gpu
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
def test_command_line(built, duplex, tmp_path, with_mask):
    """--error_profile_quality_in and --error_profile_quality through python -m gencore_amd at -s 1, without and with --error_profile_mask:
    the one table is the model's over the input, the other the model's over the written output, and each has its line on STDERR.  (The command
    line has no switch for the direct variant.)"""
    import supcases as sc
    from test_cli_gpu import cli
    d, ref = duplex
    (tmp_path / "m.vcf").write_bytes(mc.vcf(*[("c0", x + 1, "N", "<DEL>") for x in range(2, len(ref), 9)]))
    r = cli(["-i", str(d / "in.bam"), "-o", "out.bam", "-r", str(d / "ref.fa"), "-j", "r.json", "-u", "UMI", "-s", "1", "--threads", "2", "--error_profile_quality", "q.tsv",
             "--error_profile_quality_in", "qi.tsv"] + (["--error_profile_mask", "m.vcf"] if with_mask else []), tmp_path)
    assert r.returncode == 0, r.stderr
    for label, bam, tsv in (("error_profile_quality_in", d / "in.bam", "qi.tsv"), ("error_profile_quality", tmp_path / "out.bam", "q.tsv")):
        names, lens, recs = sc.raw_records(bam)
        mask = pyerrmask.load(tmp_path / "m.vcf", names, lens)["intervals"] if with_mask else None
        res = pyerrqual.profile(recs, [ref], lens, mask)
        assert (tmp_path / tsv).read_bytes() == pyerrqual.table(res, with_mask), label
        line = "%s: %d records, %d eligible, %d bases, %d mismatches, %d qualities\n" % (label, res["n_records"], res["n_eligible"], res["n_bases"], res["n_mismatches"],
                                                                                         len({q for g, q, cl in pyerrqual.nonzero(res)}))
        # (every record is 20M over A C G T: 20 bases each, of which the mask takes every ninth position)
        assert line in r.stderr and res["n_bases"] > (17 if with_mask else 19) * res["n_records"] > 0, (line, r.stderr)
        assert (("%s: mask " % label) in r.stderr) == with_mask and (res["n_masked_events"] > 100) == with_mask
        if label == "error_profile_quality_in":
            assert {q for g, q, cl in pyerrqual.nonzero(res)} == {25, 37}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["m.vcf", "out.bam", "q.tsv", "qi.tsv", "r.json"]


@pytest.mark.gpu
def test_session_call_order(built):
    """the device object refuses calls out of order: the mask and the intervals in front of the reference, the reference twice, a window or
    the finish in front of the intervals, the intervals twice"""
    from gencore_amd import capi
    lib = capi.load_library()
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    lib.gce_errqual_create.argtypes = [C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    lib.gce_errqual_destroy.argtypes, lib.gce_errqual_destroy.restype = [vp], None
    lib.gce_errqual_set_ref.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
    lib.gce_errqual_set_mask.argtypes = [vp, C.c_int64, i32p, i32p, i32p]
    lib.gce_errqual_set_sites.argtypes = [vp, C.c_int64, i32p, i32p, i32p]
    lib.gce_errqual_window.argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, vp, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    lib.gce_errqual_finish.argtypes = [vp, C.POINTER(C.c_int64), vp]
    p = vp()
    assert lib.gce_errqual_create(0, 0, 0, 0, 0x704, 1, C.byref(p)) == 0 and p.value
    try:
        out, counters, secs = np.zeros((3, 96, 24), np.uint64), (C.c_int64 * 10)(), C.c_double(0)
        assert lib.gce_errqual_set_mask(p, 0, None, None, None) == -1 and lib.gce_errqual_set_sites(p, -1, None, None, None) == -1
        assert lib.gce_errqual_window(p, None, 0, 0, None, None, None, 0, 1, 1, C.byref(secs)) == -1 and lib.gce_errqual_finish(p, counters, out.ctypes.data) == -1
        seq = (C.c_char_p * 1)(b"ACGT")
        assert lib.gce_errqual_set_ref(p, 1, seq, (C.c_int64 * 1)(4)) == 0 and lib.gce_errqual_set_ref(p, 1, seq, (C.c_int64 * 1)(4)) == -1
        assert lib.gce_errqual_window(p, None, 0, 0, None, None, None, 0, 1, 1, C.byref(secs)) == -1
        assert lib.gce_errqual_set_mask(p, 0, None, None, None) == 0 and lib.gce_errqual_set_sites(p, -1, None, None, None) == 0 and lib.gce_errqual_set_sites(p, -1, None, None, None) == -1
        assert lib.gce_errqual_window(p, None, 0, 0, None, None, None, 0, 2, 1, C.byref(secs)) == -1            # (another number of contigs)
        assert lib.gce_errqual_finish(p, None, out.ctypes.data) == -1 and lib.gce_errqual_finish(p, counters, out.ctypes.data) == 0
        assert list(counters) == [0] * 10 and not out.any()
    finally:
        lib.gce_errqual_destroy(p)


OOM = re.compile(r"out of device memory: gce_bam_error_profile_quality needs the reference bases \((\d+) bytes\) \+ 55296 bytes of counters \+ 16 bytes per interval \+ one window \+ "
                 r"4 bytes per window record \(\d+ bytes live, budget (\d+), (\d+) more for the reference bases\)")


@pytest.mark.gpu
@VARIANTS
def test_budget(built, tmp_path, direct):
    """a budget below the reference bases is GCE_ERR_OOM from the library's own check, which names this pass, its counters and the reference
    bases that did not fit; no table and no temporary file is left"""
    from gencore_amd.bamio import error_profile_quality_bam
    from gencore_amd.capi import GceError
    bam, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    ec.write_raw_bam(str(bam), [ec.rec(0, 10, "2M", "GT", [37, 25])], ["c0"], [3 << 20])
    fa.write_text(">c0\n" + "ACGT" * (3 << 18) + "\n")
    with pytest.raises(GceError) as ei:
        error_profile_quality_bam(bam, fa, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=1 << 20)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and str(ei.value).endswith(m.group(0)), str(ei.value)
    assert [int(x) for x in m.groups()[:2]] == [3 << 20, 1 << 20] and int(m.group(3)) > 3 << 20
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]
    run = error_profile_quality_bam(bam, fa, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=64 << 20)
    assert run.n_eligible == 1 and run.n_bases == 2 and run.counts[0, 37, 10] == 1 and run.counts[0, 25, 15] == 1 and 3 << 20 < run.peak_device_bytes <= 64 << 20
