"""gce_bam_error_profile_masked on the GPU: the fill kernel of gce_varmask.hpp and k_err_count under a mask, with the LDS planes
and with direct atomics, against the model (tests/pyerrmask.py) and the hand-written counters (tests/maskcases.py): every integer equal.
The cases are the smallest at which the kernels can go wrong: every hand case, the fill kernel at bit, word, block and contig edges through
the device entry points themselves, masked events at the planes' last cycle and past it, the invariants against the unmasked entry point on
random records, records cut between windows, an empty mask, the budget and the table's text."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import errprofcases as ec
import maskcases as mc
import pyerrmask
import pyerrprof
from inflate_helpers import member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_errprof.hpp")).read()
VSRC = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_varmask.hpp")).read()
CYC = int(re.search(r"#define EP_CYC (\d+)u", SRC).group(1))
BLOCK_IVS = int(re.search(r"#define VM_THREADS (\d+)u", VSRC).group(1))
assert "#define VM_BLOCK_IVS VM_THREADS" in VSRC
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["planes", "direct"])
BIG_NAMES, BIG_LENS = ["c0", "c1"], [20000, 3000]
BIG_FASTA = {nm: "".join("ACGT"[i] for i in np.random.RandomState(41 + k).randint(0, 4, ln)) for k, (nm, ln) in enumerate(zip(BIG_NAMES, BIG_LENS))}


def same(run, res, mask=None):
    """an ErrorProfileRun against the model's dict: every counter of classes 0..23, every skip, the totals; mask: rule K's result"""
    assert run.counts.dtype == np.uint64 and run.counts.shape == (3, pyerrprof.MAX_CYCLE, pyerrprof.ROW)
    want = np.array(res["counts"], np.uint64)
    assert (run.counts == want).all(), [(tuple(i), int(run.counts[tuple(i)]), int(want[tuple(i)])) for i in np.argwhere(run.counts != want)[:5]]
    for k in ["n_records", "n_eligible", "n_bases", "n_mismatches", "n_intervals", "n_masked_events"] + pyerrprof.SKIPS:
        assert getattr(run, k) == res[k], k
    if mask is not None:
        for k in ("n_lines", "n_unknown_contig", "n_no_alt", "n_masked_bases"):
            assert getattr(run, k) == mask[k], k
        assert run.n_mask_intervals == mask["n_intervals"] and run.n_mask_records == mask["n_records"] and run.load_s >= 0 and run.fill_s > 0


def run_files(tmp_path, records, names, lens, fasta, mask_text, direct, bed=None, tag="x", block=0xff00, mask_name="m.vcf", **kw):
    """records, fasta = {name: bases}, bed = None or [(contig name, start, end)] and the mask's text as files, through error_profile_masked_bam
    -> (the run, the model's result, rule K's result)"""
    from gencore_amd.bamio import error_profile_masked_bam
    bam, fa, bedf, mf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.fa" % tag), tmp_path / ("%s.bed" % tag), tmp_path / ("%s.%s" % (tag, mask_name))
    if not bam.exists():
        ec.write_raw_bam(str(bam), records, names, lens, block)
        fa.write_text(ec.fasta_text(fasta))
    if bed is not None:
        bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    mf.write_bytes(mask_text)
    run = error_profile_masked_bam(bam, fa, mf, bed=None if bed is None else bedf, direct=direct, threads=2, **kw)
    refs = [fasta.get(nm) for nm in names]
    mask = pyerrmask.load(mf, names, pyerrmask.clamp_lens(lens, refs))
    regions = None if bed is None else [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    res = pyerrmask.profile(records, refs, lens, mask["intervals"], regions, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704))
    return run, res, mask


@pytest.mark.gpu
@VARIANTS
def test_hand_cases(built, tmp_path, direct):
    """every record case of maskcases, and the records of its pair cases walked alone: the counters written out by hand and the model's"""
    for cs in mc.record_cases():
        run, res, mask = run_files(tmp_path, cs["records"], ec.NAMES, ec.LENS, ec.FASTA, mc.mask_vcf(cs["mask"]), direct, bed=cs["bed"], tag=cs["label"], min_mapq=cs["min_mapq"],
                                   min_baseq=cs["min_baseq"], exclude_flags=cs["exclude"])
        same(run, res, mask)
        assert pyerrmask.nonzero(dict(counts=run.counts.tolist())) == ec.expected(cs), cs["label"]
        assert run.n_masked_events == sum(n for g, cy, cl, n in cs["expect"] if cl == "MASKED") > 0 and not run.counts[:, :, 22:].any()
    for cs in mc.pair_cases():
        run, res, mask = run_files(tmp_path, cs["records"], ec.NAMES, ec.LENS, ec.FASTA, mc.mask_vcf(cs["mask"]), direct, tag=cs["label"])
        same(run, res, mask)
        assert run.n_masked_events > 0


# ---- the fill kernel through gce_errprof_set_mask itself: two packed contigs whose boundary falls inside a 32-bit word
EDGE_NAMES, EDGE_LENS = ["c0", "c1"], [4040, 3000]
EDGE_FASTA = {nm: "".join("ACGT"[i] for i in np.random.RandomState(51 + k).randint(0, 4, ln)) for k, (nm, ln) in enumerate(zip(EDGE_NAMES, EDGE_LENS))}
L0, L1 = EDGE_LENS
EDGE_CHUNKS = {
    "bit_0_31_32": [[(0, 0, 1), (0, 31, 32), (0, 32, 33)]],
    "bits_31_to_33": [[(0, 127, 130)]],
    "seventy_words_ragged": [[(0, 205, 205 + 2300)]],
    "seventy_words_across_the_boundary_word": [[(1, 7, 7 + 2400)]],
    "last_base_of_c0": [[(0, L0 - 1, L0)]],
    "first_base_of_c1": [[(1, 0, 1)]],
    "clamped_at_the_contig_end": [[(0, L0 - 3, L0 + 50), (1, L1 - 2, 0x7FFFFFFF), (1, -5, 2)]],
    "given_twice_and_in_two_chunks": [[(0, 10, 11), (0, 60, 200), (0, 10, 11), (1, 31, 33)], [(0, 60, 200), (1, 31, 33), (0, 150, 2600)]],
    "one_interval": [[(1, 1500, 1501)]],
    "one_more_than_a_block": [[(k & 1, 3 + 11 * k, 4 + 11 * k + (k % 5 == 0) * 40) for k in range(BLOCK_IVS + 1)]],
    "unknown_contigs_set_nothing": [[(-1, 0, 10), (2, 0, 10), (0, 5, 5), (0, 9, 3), (1, 77, 78)]],
    "empty_chunk": [[]],
}


def edge_stream():
    """forward 40M reads that copy the reference, one at every 40th position of both contigs: every reference position is covered exactly once,
    so a wrong bit anywhere changes exactly one counter"""
    recs = [ec.rec(t, x, "40M", EDGE_FASTA[nm][x:x + 40]) for t, nm in enumerate(EDGE_NAMES) for x in range(0, EDGE_LENS[t], 40)]
    text = "@HD\tVN:1.6\n"
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 2)
    for nm, ln in zip(EDGE_NAMES, EDGE_LENS):
        head += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<I", ln)
    return recs, head


def session_counts(chunks, direct):
    """one gce_errprof session driven through the device entry points: the reference, every chunk through gce_errprof_set_mask, no BED, the
    edge stream in one window -> counts [3][1024][24]"""
    from gencore_amd import capi
    lib = capi.load_library()
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    lib.gce_errprof_create.argtypes = [C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    lib.gce_errprof_destroy.argtypes, lib.gce_errprof_destroy.restype = [vp], None
    lib.gce_errprof_error.argtypes, lib.gce_errprof_error.restype = [vp], C.c_char_p
    lib.gce_errprof_set_ref.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
    lib.gce_errprof_set_mask.argtypes = [vp, C.c_int64, i32p, i32p, i32p]
    lib.gce_errprof_set_sites.argtypes = [vp, C.c_int64, i32p, i32p, i32p]
    lib.gce_errprof_window.argtypes = [vp, vp, C.c_size_t, C.c_int32, vp, vp, vp, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    lib.gce_errprof_finish.argtypes = [vp, C.POINTER(C.c_int64), vp]
    recs, head = edge_stream()
    stream = head + b"".join(recs)
    pieces = [stream[o:o + 0xff00] for o in range(0, len(stream), 0xff00)]
    members = [member(p, 6) for p in pieces]
    blob = np.frombuffer(b"".join(members), np.uint8)
    coff = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64)
    csize, usize = np.array([len(m) for m in members], np.uint32), np.array([len(p) for p in pieces], np.uint32)
    p = vp()
    assert lib.gce_errprof_create(0, 0, 0, 0, 0x704, 1 if direct else 0, C.byref(p)) == 0
    try:
        ok = lambda rc: (rc == 0) or pytest.fail("rc %d: %s" % (rc, lib.gce_errprof_error(p).decode()))
        assert lib.gce_errprof_set_mask(p, 0, None, None, None) == -1                # (in front of the reference: refused)
        seq = (C.c_char_p * 2)(*[EDGE_FASTA[nm].encode() for nm in EDGE_NAMES])
        ok(lib.gce_errprof_set_ref(p, 2, seq, (C.c_int64 * 2)(*EDGE_LENS)))
        for ch in chunks:
            arr = [(C.c_int32 * max(len(ch), 1))(*[iv[k] for iv in ch]) for k in range(3)]
            ok(lib.gce_errprof_set_mask(p, len(ch), *arr))
        ok(lib.gce_errprof_set_sites(p, -1, None, None, None))
        secs = C.c_double(0)
        ok(lib.gce_errprof_window(p, blob.ctypes.data, len(blob), len(members), coff.ctypes.data, csize.ctypes.data, usize.ctypes.data, len(head), 2, 1, C.byref(secs)))
        assert lib.gce_errprof_set_mask(p, 0, None, None, None) == -1                # (behind the first window: refused)
        counters = (C.c_int64 * 10)()
        out = np.zeros((3, pyerrprof.MAX_CYCLE, pyerrprof.ROW), np.uint64)
        ok(lib.gce_errprof_finish(p, counters, out.ctypes.data))
        assert counters[0] == counters[9] == len(recs)
        return out
    finally:
        lib.gce_errprof_destroy(p)


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("label", sorted(EDGE_CHUNKS))
def test_fill_kernel_edges(built, direct, label):
    """single bits at bit 0, 31 and 32 of a word, bits 31..33, more than 70 whole words with ragged ends (on c1 they start in the word that the
    two contigs share), the last base of c0 and the first of c1 each alone, intervals the kernel has to clamp, the same intervals twice and in
    two chunks, one interval, one more than a block's, intervals that set nothing: every counter equals the model's under the union"""
    assert L0 % 32 != 0 and L0 % 40 == 0 and L1 % 40 == 0                          # c1's first base is bit L0 (the sum of the lengths in front): inside word L0 // 32
    chunks = EDGE_CHUNKS[label]
    recs, _ = edge_stream()
    refs = [EDGE_FASTA[nm] for nm in EDGE_NAMES]
    mask = pyerrmask.merge([iv for ch in chunks for iv in ch if 0 <= iv[0] < 2], EDGE_LENS)
    want = pyerrmask.profile(recs, refs, EDGE_LENS, mask)
    got = session_counts(chunks, direct)
    wc = np.array(want["counts"], np.uint64)
    assert (got == wc).all(), [(tuple(i), int(got[tuple(i)]), int(wc[tuple(i)])) for i in np.argwhere(got != wc)[:8]]
    n_bits = sum(z - a for _, a, z in mask)
    assert int(got[:, :, 21].sum()) == n_bits == want["n_masked_events"] and int(got.sum()) == L0 + L1
    if label == "last_base_of_c0":
        assert got[0, 39, 21] == 1 and n_bits == 1 and got[0, 0, 21] == 0            # cycle 40 of c0's last read; cycle 1 of c1's first stays clear
    if label == "first_base_of_c1":
        assert got[0, 0, 21] == 1 and n_bits == 1 and got[0, 39, 21] == 0
    if label == "seventy_words_ragged":
        assert (205 + 2300) // 32 - (205 + 31) // 32 >= 70 and 205 % 32 and (205 + 2300) % 32
    if label == "one_more_than_a_block":
        assert len(chunks[0]) == BLOCK_IVS + 1 and BLOCK_IVS // 2 < len(mask) <= BLOCK_IVS
    if label in ("unknown_contigs_set_nothing", "empty_chunk"):
        assert n_bits == (1 if label[0] == "u" else 0)


@pytest.mark.gpu
@VARIANTS
def test_fill_edges_through_the_file(built, tmp_path, direct):
    """the same edges as a VCF through gce_mask_load and the runner: records in an order of their own, REFs that run past a contig"""
    recs, _ = edge_stream()
    rows = [("c0", 1, "N", "A"), ("c0", 32, "NN", "A"), ("c0", 128, "NNN", "A"), ("c0", 206, "N" * 2300, "<DEL>"), ("c1", 8, "N" * 2400, "<DEL>"), ("c0", L0, "NNNN", "N"), ("c1", 1, "N", "T"),
            ("c1", L1 - 1, "N" * 60, "N"), ("c0", 3000, "N", "."), ("zz", 5, "N", "A")]
    run, res, mask = run_files(tmp_path, recs, EDGE_NAMES, EDGE_LENS, EDGE_FASTA, mc.vcf(*rows[::-1]), direct)
    same(run, res, mask)
    assert mask["intervals"] == [(0, 0, 1), (0, 31, 33), (0, 127, 130), (0, 205, 2505), (0, L0 - 1, L0), (1, 0, 1), (1, 7, 2407), (1, L1 - 2, L1)]
    assert (mask["n_no_alt"], mask["n_unknown_contig"], mask["n_records"]) == (1, 1, 10) and run.n_masked_events == mask["n_masked_bases"] == 4710


def read_at(k, n, flag, pos=100):
    """read k of n aligned bases copied from c0 with every seventh base changed"""
    ref = BIG_FASTA["c0"][pos + k:pos + k + n]
    return ec.rec(0, pos + k, "%dM" % n, "".join("ACGT"[("ACGT".index(b) + 1) % 4] if i % 7 == 3 else b for i, b in enumerate(ref)), flag=flag)


@pytest.mark.gpu
@VARIANTS
def test_plane_edges(built, tmp_path, direct):
    """masked columns at cycle EP_CYC, the planes' last, and at EP_CYC + 1, the first in memory, on both strands, and a masked insertion and
    deletion at EP_CYC: MASKED never goes through a plane, its neighbours do"""
    n = CYC + 1
    recs = [read_at(0, n, 0x40), read_at(0, n, 0x50)]                               # forward: the column of cycle c is 99 + c; reverse: the column of cycle c is 100 + n - c
    recs += [ec.rec(0, 500, "%dS1M1I1D1M" % (CYC - 2), "A" * (CYC - 2) + "CGT", flag=f) for f in (0x80, 0x90)]      # forward: M at EP_CYC - 1, I and D at EP_CYC, M at EP_CYC + 1
    rows = [("c0", x + 1, "N", "A") for x in (100, 101, 99 + CYC, 100 + CYC, 500, 501)]
    run, res, mask = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, mc.vcf(*rows), direct)
    same(run, res, mask)
    assert run.counts[1, CYC - 1, 21] == 2 and run.counts[1, CYC, 21] == 2 and run.counts[1, 0, 21] == 2 and run.counts[1, 1, 21] == 2        # both strands at EP_CYC and EP_CYC + 1
    assert run.counts[2, CYC - 2, 21] == 1 and run.counts[2, CYC - 1, 21] == 2 and run.counts[2, CYC, 21] == 0                                # forward: the M, then the I and the D
    assert run.n_masked_events == 14 and not run.counts[:, :, pyerrprof.INS].any() and not run.counts[:, :, pyerrprof.DEL].any()
    assert run.counts[1, CYC - 2, :16].sum() == 2


def window_records():
    """test_errprof_gpu.window_records' shape with a seed of its own"""
    rng = np.random.RandomState(29)
    recs = []
    for k in range(400):
        n = int(rng.randint(20, 200))
        ops = [(4, int(rng.randint(1, 5)))] * int(rng.randint(0, 2)) + [(0, n), (int(rng.choice([1, 2, 3])), int(rng.randint(1, 6))), (0, int(rng.randint(1, 30)))]
        nq = sum(ln for op, ln in ops if op in (0, 1, 4))
        seq = "".join("ACGTN"[i] for i in rng.choice(5, nq, p=[.24, .24, .24, .24, .04]))
        recs.append(ec.rec(int(k >= 300), int(rng.randint(0, 2500)), ops, seq, rng.randint(0, 41, nq).tolist(), flag=int(rng.choice([0, 16, 0x40, 0x50, 0x80, 0x90, 0x400])),
                           mapq=int(rng.randint(0, 61)), name="read%04d" % k))
    recs.insert(150, ec.rec(0, 100, "1000M", "".join("ACGT"[i] for i in rng.randint(0, 4, 1000)), rng.randint(0, 41, 1000).tolist()))
    return recs


@pytest.fixture(scope="module")
def random_case():
    """the random records, a mask of about 5 % of the positions as VCF text and its complement as BED rows, once"""
    rng = np.random.RandomState(31)
    sites = [(nm, x) for nm, ln in zip(BIG_NAMES, BIG_LENS) for x in range(ln) if rng.rand() < 0.05]
    text = mc.vcf(*[(nm, x + 1, BIG_FASTA[nm][x], "ACGT"[("ACGT".index(BIG_FASTA[nm][x]) + 1) % 4]) for nm, x in sites])
    merged = pyerrmask.merge([(BIG_NAMES.index(nm), x, x + 1) for nm, x in sites], BIG_LENS)
    comp = [(BIG_NAMES[t], a, z) for t, a, z in pyerrmask.complement(merged, BIG_LENS)]
    assert 900 < len(sites) < 1400 and sum(z - a for _, a, z in comp) + len(sites) == sum(BIG_LENS)
    return window_records(), text, comp


@pytest.mark.gpu
@VARIANTS
def test_invariants_against_the_unmasked_entry_point(built, tmp_path, random_case, direct):
    """random records under a random mask of 5 % of the positions, with and without a BED: per (segment, cycle) classes 0..21 sum to the
    unmasked entry point's 0..20 on the same files; without a BED classes 0..20 are the unmasked entry point's under the mask's complement as
    its BED; members of 300 bytes in windows of 1000 give the one-window result"""
    from gencore_amd.bamio import error_profile_bam
    recs, text, comp = random_case
    bed = [("c0", 50, 400), ("c0", 1000, 1300), ("c0", 5000, 6500), ("c1", 0, 3000)]
    for tag, b in (("nobed", None), ("bed", bed)):
        one, res, mask = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, text, direct, bed=b, tag=tag, block=300, min_baseq=13, min_mapq=5)
        same(one, res, mask)
        plain = error_profile_bam(tmp_path / (tag + ".bam"), tmp_path / (tag + ".fa"), bed=None if b is None else tmp_path / (tag + ".bed"), direct=direct, min_baseq=13, min_mapq=5)
        assert (one.counts[:, :, :22].sum(axis=2) == plain.counts[:, :, :21].sum(axis=2)).all() and not plain.counts[:, :, 21:].any()
        assert 50 < one.n_masked_events < one.n_bases and one.n_mismatches < plain.n_mismatches and one.n_records == plain.n_records
        cut, _, _ = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, text, direct, bed=b, tag=tag, block=300, min_baseq=13, min_mapq=5, window_bytes=1000)
        same(cut, res, mask)
        assert (cut.counts == one.counts).all()
        if b is None:
            (tmp_path / "comp.bed").write_text("".join("%s\t%d\t%d\n" % r for r in comp))
            other = error_profile_bam(tmp_path / "nobed.bam", tmp_path / "nobed.fa", bed=tmp_path / "comp.bed", direct=direct, min_baseq=13, min_mapq=5)
            assert (one.counts[:, :, :21] == other.counts[:, :, :21]).all() and other.n_bases == one.n_bases and other.n_mismatches == one.n_mismatches


@pytest.mark.gpu
@VARIANTS
def test_empty_mask_bed_mask_and_table_text(built, tmp_path, direct):
    """a mask without a record is a valid run: MASKED is zero everywhere, classes 0..20 are the unmasked run's and the table has the extra
    zero column; a .bed mask and a .vcf.gz mask of the same positions give one result; the table's bytes equal the model's"""
    from gencore_amd.bamio import error_profile_bam
    recs = [read_at(k, 30 + 5 * (k % 4), (0, 0x10, 0x40, 0x90)[k % 4]) for k in range(40)] + [ec.rec(0, 900, "3M1I2M1D4M", "ACGTACGTAC", flag=0x80)]
    run, res, mask = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, mc.vcf(), direct, tag="t", tsv=tmp_path / "empty.tsv")
    same(run, res, mask)
    plain = error_profile_bam(tmp_path / "t.bam", tmp_path / "t.fa", direct=direct, tsv=tmp_path / "plain.tsv")
    assert (run.counts == plain.counts).all() and run.n_masked_events == run.n_mask_intervals == run.n_masked_bases == 0 and run.n_lines == 2
    lines, plines = (tmp_path / "empty.tsv").read_bytes().split(b"\n"), (tmp_path / "plain.tsv").read_bytes().split(b"\n")
    assert lines[0] == plines[0] + b"\tMASKED" and lines[1:-1] == [l + b"\t0" for l in plines[1:-1]] and len(lines) == 1 + 35 + 40 + 45 + 1
    assert (tmp_path / "empty.tsv").read_bytes() == pyerrmask.table(res) and (tmp_path / "plain.tsv").read_bytes() == pyerrprof.table(dict(counts=plain.counts.tolist()))
    import gzip
    ivs = [("c0", 110, 125), ("c0", 131, 132), ("c0", 900, 904), ("c0", 19990, 20100)]
    vz, res_v, mask_v = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, gzip.compress(mc.mask_vcf(ivs)), direct, tag="t", mask_name="m.vcf.gz", tsv=tmp_path / "vcf.tsv")
    same(vz, res_v, mask_v)
    bd, res_b, mask_b = run_files(tmp_path, recs, BIG_NAMES, BIG_LENS, BIG_FASTA, "".join("%s\t%d\t%d\n" % r for r in ivs).encode(), direct, tag="t", mask_name="m.bed", tsv=tmp_path / "bed.tsv")
    same(bd, res_b, mask_b)
    assert (vz.counts == bd.counts).all() and mask_v["intervals"] == mask_b["intervals"] == [(0, 110, 125), (0, 131, 132), (0, 900, 904), (0, 19990, 20000)] and mask_b["n_lines"] == 0
    assert (tmp_path / "vcf.tsv").read_bytes() == (tmp_path / "bed.tsv").read_bytes() == pyerrmask.table(res_v) and vz.n_masked_events > 100
    assert b"\tMASKED\n" in (tmp_path / "vcf.tsv").read_bytes()[:400]


OOM = re.compile(r"out of device memory: gce_bam_error_profile needs the reference bases \((\d+) bytes\) \+ 576 KiB of counters \+ the mask \+ 16 bytes per interval "
                 r"\+ one window \+ 4 bytes per window record \(\d+ bytes live, budget (\d+), (\d+) more for the variant mask\)")


@pytest.mark.gpu
@VARIANTS
def test_budget(built, tmp_path, direct):
    """a budget that holds the reference (3 MiB and an eighth, as the buffers are padded) but not the bitmap of an eighth of it: GCE_ERR_OOM
    that names the variant mask, with the footprint in its message; no table and no temporary file is left; a malformed mask line likewise"""
    from gencore_amd.bamio import error_profile_masked_bam
    from gencore_amd.capi import GceError
    bam, fa, vcf = tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "m.vcf"
    ec.write_raw_bam(str(bam), [ec.rec(0, 10, "2M")], ["c0"], [3 << 20])
    fa.write_text(">c0\n" + "ACGT" * (3 << 18) + "\n")
    vcf.write_bytes(mc.vcf(("c0", 11, "A", "C")))
    with pytest.raises(GceError) as ei:
        error_profile_masked_bam(bam, fa, vcf, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=3700000)
    m = OOM.search(str(ei.value))
    assert ei.value.status == -4 and m and str(ei.value).endswith(m.group(0)), str(ei.value)
    assert [int(x) for x in m.groups()] == [3 << 20, 3700000, ((3 << 20) // 8 + 64) * 9 // 8 + 256] and len(str(ei.value).split(": ", 1)[1]) <= 255
    vcf.write_bytes(mc.vcf(("c0", 11, "A", "C")) + b"c0\t12\n")
    with pytest.raises(GceError) as ei:
        error_profile_masked_bam(bam, fa, vcf, tsv=tmp_path / "out.tsv", direct=direct)
    assert ei.value.status == -1 and str(ei.value).endswith("variant mask line 4: fewer than five tab-separated fields")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "m.vcf", "ref.fa"]
    vcf.write_bytes(mc.vcf(("c0", 11, "A", "C")))
    run = error_profile_masked_bam(bam, fa, vcf, tsv=tmp_path / "out.tsv", direct=direct, device_budget_bytes=64 << 20)
    assert run.n_eligible == 1 and run.n_bases == 1 and run.n_masked_events == 1 and 3 << 20 < run.peak_device_bytes <= 64 << 20
