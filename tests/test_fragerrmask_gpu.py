"""gce_bam_error_profile_fragments_masked on the GPU: k_fragerr_count under a mask, with the LDS planes and with direct atomics,
against the model (tests/pyerrmask.py) and the hand-written counters (tests/maskcases.py): every integer of both tables equal, the overlap
table's sum twice the shared columns on every run.  Every hand case, shared masked columns at the planes' last cycle and past it, the
invariants against the unmasked entry point on a generated paired stream in one window and in many, an empty mask, both tables' bytes, and
the command line with all four tables."""
import gzip
import os
import re

import numpy as np
import pytest

import errprofcases as ec
import fragcases as fc
import fragerrcases as fx
import maskcases as mc
import pileupcases as pc
import pyerrmask
import pyerrprof
import pyfragerr
import pyfragpile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYC = int(re.search(r"#define EP_CYC (\d+)u", open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_errprof.hpp")).read()).group(1))
VARIANTS = pytest.mark.parametrize("direct", [False, True], ids=["planes", "direct"])
BIG = (["c0", "c1"], [20000, 3000])
COUNTERS = ["n_records", "n_eligible", "n_bases", "n_mismatches", "n_intervals", "n_masked_events"] + pyerrprof.SKIPS + pyfragerr.FRAG_COUNTERS


def big_fasta(seed=37):
    rng = np.random.RandomState(seed)
    return {nm: "".join("ACGTacgtNR"[j] for j in rng.choice(10, ln, p=[.22, .22, .22, .22, .02, .02, .02, .02, .02, .02])) for nm, ln in zip(*BIG)}


def same(run, res, mask=None, deferred=None):
    """a run against the model's dict: both tables, every counter, and the overlap table's sum; mask: rule K's result"""
    for k in COUNTERS:
        assert getattr(run, k) == res[k], k
    for name, got, want in (("counts", run.counts, res["counts"]), ("overlap", run.overlap, res["overlap"])):
        assert got.dtype == np.uint64 and got.shape == (3, pyerrprof.MAX_CYCLE, pyerrprof.ROW)
        want = np.array(want, np.uint64)
        assert (got == want).all(), (name, [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in np.argwhere(got != want)[:5]])
    assert int(run.overlap.sum()) == 2 * run.n_shared_columns and not run.overlap[:, :, 22:].any() and not run.counts[:, :, 22:].any()
    if mask is not None:
        for k in ("n_lines", "n_unknown_contig", "n_no_alt", "n_masked_bases"):
            assert getattr(run, k) == mask[k], k
        assert run.n_mask_intervals == mask["n_intervals"] and run.n_mask_records == mask["n_records"] and run.fill_s > 0
    if deferred is not None:
        assert run.n_deferred == deferred


def run_files(tmp_path, records, fasta, mask_text, bed, names, lens, direct, tag="x", block=0xff00, mask_name="m.vcf", **kw):
    """records, fasta, bed and the mask's text as files, through error_profile_fragments_masked_bam -> (the run, the model's result, rule K's)"""
    from gencore_amd.bamio import error_profile_fragments_masked_bam
    bam, fa, bedf, mf = tmp_path / ("%s.bam" % tag), tmp_path / ("%s.fa" % tag), tmp_path / ("%s.bed" % tag), tmp_path / ("%s.%s" % (tag, mask_name))
    if not bam.exists():
        pc.write_raw_bam(str(bam), records, names, lens, block)
        fa.write_text(ec.fasta_text(fasta))
    if bed is not None:
        bedf.write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    mf.write_bytes(mask_text)
    run = error_profile_fragments_masked_bam(bam, fa, mf, bed=None if bed is None else bedf, direct=direct, threads=2, **kw)
    refs = [fasta.get(nm) for nm in names]
    mask = pyerrmask.load(mf, names, pyerrmask.clamp_lens(lens, refs))
    regions = None if bed is None else [(names.index(nm) if nm in names else -1, a, z) for nm, a, z in bed]
    res = pyerrmask.profile_fragments(records, refs, lens, mask["intervals"], regions, kw.get("min_mapq", 0), kw.get("min_baseq", 0), kw.get("exclude_flags", 0x704))
    return run, res, mask


@pytest.mark.gpu
@VARIANTS
def test_hand_cases(built, tmp_path, direct):
    """every case of maskcases through the fragment pass: the pairs with a shared masked column (primary MASKED 1, OVL_MASKED 2, the shared
    columns unchanged) and the records without a partner, counted as the plain pass counts them"""
    for cs in mc.pair_cases():
        run, res, mask = run_files(tmp_path, cs["records"], ec.FASTA, mc.mask_vcf(cs["mask"]), cs["bed"], ec.NAMES, ec.LENS, direct, tag=cs["label"], min_mapq=cs["min_mapq"],
                                   min_baseq=cs["min_baseq"], exclude_flags=cs["exclude"])
        same(run, res, mask, deferred=0)
        assert pyerrmask.nonzero(dict(counts=run.counts.tolist())) == fx.expected(cs), cs["label"]
        assert pyerrmask.nonzero_overlap(dict(overlap=run.overlap.tolist())) == fx.expected(cs, "xexpect"), cs["label"]
        assert {k: getattr(run, k) for k in pyfragerr.FRAG_COUNTERS} == fx.counters_of(cs), cs["label"]
    cs = mc.pair_cases()[0]
    run, _, _ = run_files(tmp_path, cs["records"], ec.FASTA, mc.mask_vcf(cs["mask"]), None, ec.NAMES, ec.LENS, direct, tag=cs["label"])
    assert run.counts[:, :, 21].sum() == 1 and run.overlap[:, :, 21].sum() == 2 and run.n_shared_columns == 3
    for cs in mc.record_cases():
        run, res, mask = run_files(tmp_path, cs["records"], ec.FASTA, mc.mask_vcf(cs["mask"]), cs["bed"], ec.NAMES, ec.LENS, direct, tag=cs["label"], min_mapq=cs["min_mapq"],
                                   min_baseq=cs["min_baseq"], exclude_flags=cs["exclude"])
        same(run, res, mask, deferred=0)
        assert pyerrmask.nonzero(dict(counts=run.counts.tolist())) == ec.expected(cs) and not run.overlap.any() and run.n_pairs == 0, cs["label"]


def long_pair(la, lb, shift, seed, name, fasta):
    """a of la bases at c0:100 (forward, first) and b of lb bases at c0:100 + shift (reverse, last), both copies of the reference with a few
    other bases"""
    rng = np.random.RandomState(seed)
    ref = fasta["c0"].upper()
    out = []
    for first, at, n in ((True, 100, la), (False, 100 + shift, lb)):
        seq = "".join(c if c in "ACGT" and rng.rand() > 0.05 else "ACGT"[rng.randint(4)] for c in ref[at:at + n])
        out.append(fc.mated(ec.rec(0, at, "%dM" % n, seq, rng.randint(2, 41, n).tolist(), flag=0x41 if first else 0x91, name=name), 100 + shift if first else 100))
    return out


@pytest.mark.gpu
@VARIANTS
def test_shared_masked_columns_at_the_planes_edge(built, tmp_path, direct):
    """a of EP_CYC + 1 bases and b of 200 that overlap it: the shared columns of a's cycles EP_CYC (the planes' last) and EP_CYC + 1 (memory) are
    masked, and b's cycles EP_CYC and EP_CYC + 1 as well: MASKED and OVL_MASKED beside neighbours that go through the planes"""
    fasta = big_fasta()
    recs = long_pair(CYC + 1, 200, 11, 5, "long", fasta)
    a_cols = [99 + CYC, 100 + CYC]                                                  # a, forward at 100: the column of cycle c is 99 + c
    b_cols = [111 + 200 - CYC, 111 + 200 - CYC - 1]                                 # b, reverse at 111 with 200 bases: the column of cycle c is 111 + 200 - c
    run, res, mask = run_files(tmp_path, recs, fasta, mc.vcf(*[("c0", x + 1, "N", "A") for x in a_cols + b_cols]), None, *BIG, direct, min_baseq=10)
    same(run, res, mask, deferred=0)
    assert res["n_pairs"] == 1 and res["n_shared_columns"] == CYC + 1 - 11 and mask["n_masked_bases"] == 4
    assert run.overlap[1, CYC - 1, 21] == 1 and run.overlap[1, CYC, 21] == 1 and run.overlap[2, CYC - 1, 21] == 1 and run.overlap[2, CYC, 21] == 1
    assert run.overlap[:, :, 21].sum() == 2 * 4 and run.counts[:, :, 21].sum() == 4 and run.overlap[1, CYC - 2, :21].sum() == 1


@pytest.fixture(scope="module")
def generated():
    """1200 generated fragments (test_fragpile_gpu.py's generator), a mask of about 5 % of the positions as VCF text, and the model's results
    without a BED and with one, computed once"""
    from test_fragpile_gpu import paired_stream
    recs = paired_stream(1200, 19)
    bed = [("c0", 1000, 1400), ("c0", 5000, 5600), ("c0", 7000, 9000), ("c0", 12000, 12300), ("c0", 18990, 19300)]
    fasta = big_fasta()
    refs = [fasta[nm] for nm in BIG[0]]
    rng = np.random.RandomState(43)
    text = mc.vcf(*[(nm, x + 1, "N", "A") for nm, ln in zip(*BIG) for x in range(ln) if rng.rand() < 0.05])
    mask = pyerrmask.parse_vcf(text, BIG[0], BIG[1])
    res = {False: pyerrmask.profile_fragments(recs, refs, BIG[1], mask["intervals"], None, 0, 20),
           True: pyerrmask.profile_fragments(recs, refs, BIG[1], mask["intervals"], [(0, a, z) for _, a, z in bed], 0, 20)}
    return recs, fasta, bed, text, mask, res


@pytest.mark.gpu
@VARIANTS
@pytest.mark.parametrize("with_bed", [False, True], ids=["nobed", "bed"])
def test_invariants_and_tables(built, generated, tmp_path, direct, with_bed):
    """generated fragments under a random mask against the model, both tables' bytes, the same through small windows, and against the unmasked
    entry point on the same files: per (segment, cycle) classes 0..21 of either table sum to its 0..20, the pairs, the shared and the
    disagreeing columns are its own, and the mismatches are fewer"""
    from gencore_amd.bamio import error_profile_fragments_bam, error_profile_fragments_masked_bam
    recs, fasta, bed, text, mask, results = generated
    res = results[with_bed]
    assert res["n_pairs"] > (100 if with_bed else 700) and res["n_masked_events"] > 200 and int(np.array(res["overlap"])[:, :, 21].sum()) > 100
    pc.write_raw_bam(str(tmp_path / "in.bam"), recs, *BIG, block=4000)
    (tmp_path / "ref.fa").write_text(ec.fasta_text(fasta))
    (tmp_path / "t.bed").write_text("".join("%s\t%d\t%d\n" % r for r in bed))
    (tmp_path / "m.vcf.gz").write_bytes(gzip.compress(text))
    kw = dict(bed=tmp_path / "t.bed" if with_bed else None, min_baseq=20, direct=direct, threads=2)
    run = error_profile_fragments_masked_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "m.vcf.gz", tsv=tmp_path / "p.tsv", overlap_tsv=tmp_path / "o.tsv", **kw)
    same(run, res, mask, deferred=0)
    assert (tmp_path / "p.tsv").read_bytes() == pyerrmask.table(res) and (tmp_path / "o.tsv").read_bytes() == pyerrmask.overlap_table(res)
    small = error_profile_fragments_masked_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "m.vcf.gz", window_bytes=1 << 14, **kw)
    same(small, res, mask)
    assert small.n_deferred > 0
    plain = error_profile_fragments_bam(tmp_path / "in.bam", tmp_path / "ref.fa", **kw)
    for got, old in ((run.counts, plain.counts), (run.overlap, plain.overlap)):
        assert (got[:, :, :22].sum(axis=2) == old[:, :, :21].sum(axis=2)).all() and not old[:, :, 21:].any()
    for k in pyfragerr.FRAG_COUNTERS + ["n_records", "n_eligible", "n_intervals"]:
        assert getattr(run, k) == getattr(plain, k), k
    assert run.n_mismatches < plain.n_mismatches and run.n_bases < plain.n_bases
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "m.vcf.gz", "o.tsv", "p.tsv", "ref.fa", "t.bed"]


@pytest.mark.gpu
@VARIANTS
def test_empty_mask(built, tmp_path, direct):
    """a mask without a record: both tables are the unmasked run's with a trailing column of zeros"""
    from gencore_amd.bamio import error_profile_fragments_bam
    fasta = big_fasta()
    recs = long_pair(60, 70, 20, 9, "p", fasta)
    run, res, mask = run_files(tmp_path, recs, fasta, b"", None, *BIG, direct, tsv=tmp_path / "p.tsv", overlap_tsv=tmp_path / "o.tsv")
    same(run, res, mask, deferred=0)
    plain = error_profile_fragments_bam(tmp_path / "x.bam", tmp_path / "x.fa", direct=direct, tsv=tmp_path / "pp.tsv", overlap_tsv=tmp_path / "po.tsv")
    assert (run.counts == plain.counts).all() and (run.overlap == plain.overlap).all() and run.n_masked_events == 0 and run.n_lines == 0 and run.n_shared_columns == 40
    for a, b in (("p.tsv", "pp.tsv"), ("o.tsv", "po.tsv")):
        la, lb = (tmp_path / a).read_bytes().split(b"\n"), (tmp_path / b).read_bytes().split(b"\n")
        assert la[0] == lb[0] + b"\tMASKED" and la[1:-1] == [l + b"\t0" for l in lb[1:-1]] and len(la) > 100


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """the suite's generated stream of 1000 pairs (test_errprof_gpu.py's) as in.bam / ref.fa"""
    from test_cli_gpu import write_inputs
    from test_depth_bed import depth_case
    d = tmp_path_factory.mktemp("errmaskstream")
    data, batch, _, panel = depth_case("cfg3", 1000)
    regions = [(t, a - 150 + 20 * k, a - 150 + 20 * k + 12) for t, a, _ in panel[:2] for k in range(18)]
    write_inputs(d, data, batch, regions)
    return d


def mismatch_sites(recs, refs):
    """the (tid, position) of every M / = / X column at which an eligible record of the stream shows another base than the reference"""
    sites = set()
    for r in recs:
        f = pyerrprof.fields(r)
        if pyerrprof.skip_of(f, refs, 0, 0x704):
            continue
        for x, g, cy, c in pyerrprof.walk(f, refs[f["tid"]], 0):
            if c < 16 and (c >> 2) != (c & 3):
                sites.add((f["tid"], x))
    return sites


@pytest.mark.gpu
def test_command_line(built, stream, tmp_path):
    """one run with --error_profile_in, --error_profile, --error_profile_fragments and --error_profile_mask x.vcf.gz, the mask made of the
    positions at which a read of the input differs from the reference and of some at which none does: all four tables equal the model's,
    the STDERR lines carry the model's numbers, and the mismatches are fewer than in the unmasked run of the same files (in the input's
    table strictly; the output's has few to lose)"""
    from test_cli_gpu import cli
    d = stream
    fasta = pyerrprof.read_fasta(str(d / "ref.fa"))
    names, lens, recs = pyfragpile.read_raw_records(str(d / "in.bam"))
    refs = pyerrprof.refs_of(fasta, names)
    sites = sorted(mismatch_sites(recs, refs))
    assert len(sites) > 50
    chosen = sites + [(t, x + 1) for t, x in sites[1::20] if (t, x + 1) not in sites and x + 1 < len(refs[t])]
    rows = [(names[t], x + 1, chr(refs[t][x]) if isinstance(refs[t], bytes) else refs[t][x], "<X>") for t, x in sorted(set(chosen))]
    (tmp_path / "x.vcf.gz").write_bytes(gzip.compress(mc.vcf(*rows)))
    common = ["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "--threads", "4", "--error_profile_min_baseq", "20", "--error_profile_fragments"]
    r = cli(common + ["-o", "out.bam", "-j", "r.json", "--error_profile_in", "before.tsv", "--error_profile", "after.tsv", "--error_profile_mask", "x.vcf.gz"], tmp_path)
    assert r.returncode == 0, r.stderr
    mask = pyerrmask.load(tmp_path / "x.vcf.gz", names, pyerrmask.clamp_lens(lens, refs))
    assert mask["n_records"] == len(rows) and mask["n_masked_bases"] == len(rows)
    totals = {}
    for label, bam, tsv in (("error_profile_in", d / "in.bam", "before.tsv"), ("error_profile", tmp_path / "out.bam", "after.tsv")):
        names2, lens2, recs2 = pyfragpile.read_raw_records(str(bam))
        res = pyerrmask.profile_fragments(recs2, pyerrprof.refs_of(fasta, names2), lens2, mask["intervals"], None, 0, 20)
        assert (tmp_path / tsv).read_bytes() == pyerrmask.table(res), label
        assert (tmp_path / (tsv + ".overlap.tsv")).read_bytes() == pyerrmask.overlap_table(res), label
        assert ("%s: %d records, %d eligible, %d bases, %d mismatches\n%s: %d pairs, %d shared columns, %d disagreeing\n%s: mask %d intervals, %d bases, %d events masked\n"
                % (label, res["n_records"], res["n_eligible"], res["n_bases"], res["n_mismatches"], label, res["n_pairs"], res["n_shared_columns"], res["n_disagree_columns"],
                   label, mask["n_intervals"], mask["n_masked_bases"], res["n_masked_events"])) in r.stderr
        assert res["n_masked_events"] > 0
        totals[label] = res["n_mismatches"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["after.tsv", "after.tsv.overlap.tsv", "before.tsv", "before.tsv.overlap.tsv", "out.bam", "r.json", "x.vcf.gz"]
    plain = cli(common + ["-o", "out2.bam", "--error_profile_in", "before2.tsv", "--error_profile", "after2.tsv"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    for label in totals:
        unmasked = int(re.search(r"^%s: \d+ records, \d+ eligible, \d+ bases, (\d+) mismatches$" % label, plain.stderr, re.M).group(1))
        assert totals[label] < unmasked or (label == "error_profile" and totals[label] == unmasked), label
    assert ": mask " not in plain.stderr and b"MASKED" not in (tmp_path / "before2.tsv").read_bytes()
