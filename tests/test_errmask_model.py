"""The error profile's variant mask without a GPU: the model (tests/pyerrmask.py) against the texts and records written out by
hand (tests/maskcases.py); gce_mask_load (host only) against the model on every text, as .vcf, as one gzip member and as BGZF with members of
300 bytes, a .bed mask and the refusals; the complement identity on the model; the symbols, prototypes, struct sizes and argument checks of the
masked entry points; the command line's help and validation; and the masked per-record functions of the kernels compiled for the host under
the address and undefined-behaviour sanitizers, with the bitmap in a heap block of its exact size."""
import ctypes as C
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import errprofcases as ec
import fragerrcases as fx
import maskcases as mc
import pybam
import pyerrmask
import pyerrprof
import pyfragerr
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = ec.refs()


def model_mask(cs):
    return pyerrmask.merge(mc.mask_of(cs), mc.CLAMP)


def run_model(cs, fragments=False):
    f = pyerrmask.profile_fragments if fragments else pyerrmask.profile
    return f(cs["records"], REFS, ec.LENS, model_mask(cs), ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])


def test_clamp_is_min_of_header_and_fasta():
    assert pyerrmask.clamp_lens(ec.LENS, REFS) == mc.CLAMP == [40, 50, -1]


def test_rule_k_model_against_hand_texts():
    labels = [c["label"] for c in mc.vcf_cases()]
    assert len(set(labels)) == len(labels) >= 14
    for cs in mc.vcf_cases():
        res = pyerrmask.parse_vcf(cs["text"], ec.NAMES, mc.CLAMP)
        assert res["intervals"] == cs["intervals"], cs["label"]
        assert {k: res[k] for k in pyerrmask.COUNTERS} == cs["counters"], cs["label"]
    assert len([c for c in mc.vcf_cases() if c["label"] == "long_line"][0]["text"].split(b"\n")[0]) > 100000
    for label, text, line, words in mc.refusals():
        with pytest.raises(pyerrmask.MaskError) as ei:
            pyerrmask.parse_vcf(text, ec.NAMES, mc.CLAMP)
        assert ei.value.line == line and str(ei.value) == "variant mask line %d: %s" % (line, words), label


def test_rule_y_model_against_hand_records():
    labels = [c["label"] for c in mc.record_cases() + mc.pair_cases()]
    assert len(set(labels)) == len(labels) >= 12
    for cs in mc.record_cases():
        for fragments in (False, True):                                 # records without a partner: the fragment pass counts them as the plain pass does
            res = run_model(cs, fragments)
            assert pyerrmask.nonzero(res) == ec.expected(cs), (cs["label"], fragments)
            assert {k: res[k] for k in pyerrprof.SKIPS} == cs["skips"] and res["n_eligible"] == len(cs["records"])
            assert all(row[22:] == [0, 0] for seg in res["counts"] for row in seg)
            assert res["n_masked_events"] == sum(n for g, cy, cl, n in cs["expect"] if cl == "MASKED") > 0
            assert res["n_bases"] == sum(n for g, cy, cl, n in cs["expect"] if ">" in cl)
        assert not pyerrmask.nonzero_overlap(res) and res["n_pairs"] == 0
    for cs in mc.pair_cases():
        res = run_model(cs, True)
        assert pyerrmask.nonzero(res) == fx.expected(cs), cs["label"]
        assert pyerrmask.nonzero_overlap(res) == fx.expected(cs, "xexpect"), cs["label"]
        assert {k: res[k] for k in pyfragerr.FRAG_COUNTERS} == fx.counters_of(cs), cs["label"]
        assert pyfragerr.overlap_sum(res) == 2 * res["n_shared_columns"]
        # the same pair without the mask: the pairs, the shared and the disagreeing columns do not move, and every row keeps its sum
        plain = pyfragerr.profile_fragments(cs["records"], REFS, ec.LENS, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        assert {k: plain[k] for k in pyfragerr.FRAG_COUNTERS} == fx.counters_of(cs)
        for key in ("counts", "overlap"):
            assert [[sum(row[:22]) for row in seg] for seg in res[key]] == [[sum(row[:21]) for row in seg] for seg in plain[key]], (cs["label"], key)


def random_records(seed, n=120):
    """reads over c1 and the FASTA's part of c0 with M, I, D, N and S ops, every anchor inside [0, header length)"""
    rng = np.random.RandomState(seed)
    recs = []
    for k in range(n):
        tid = int(rng.randint(0, 2))
        ops = [(4, 2)] * int(rng.randint(0, 2)) + [(int(rng.choice([0, 1, 2])), int(rng.randint(1, 4))) for _ in range(int(rng.randint(0, 2)))]
        for _ in range(int(rng.randint(1, 4))):
            ops += [(0, int(rng.randint(1, 7))), (int(rng.choice([1, 2, 3])), int(rng.randint(1, 4)))]
        ops.append((0, int(rng.randint(1, 5))))
        span = sum(ln for op, ln in ops if op in (0, 2, 3))
        pos = int(rng.randint(1, (45 if tid else 42) - min(span, 40)))
        nq = sum(ln for op, ln in ops if op in (0, 1, 4))
        recs.append(ec.rec(tid, pos, ops, "".join("ACGTN"[i] for i in rng.randint(0, 5, nq)), rng.randint(0, 41, nq).tolist(), flag=int(rng.choice([0, 16, 0x40, 0x90]))))
    return recs


def random_mask(seed, lens, share):
    rng = np.random.RandomState(seed)
    return pyerrmask.merge([(t, x, x + 1) for t, ln in enumerate(lens) for x in range(max(ln, 0)) if rng.rand() < share], lens)


def test_model_invariants():
    """per (segment, cycle) classes 0..21 masked sum to 0..20 unmasked; without a BED classes 0..20 under mask M are the unmasked model's under
    the complement of M as its BED"""
    recs = random_records(7)
    for share in (0.05, 0.5, 1.0):
        mask = random_mask(3, mc.CLAMP, share)
        for regions in (None, [(0, 3, 20), (1, 10, 30)]):
            got = pyerrmask.profile(recs, REFS, ec.LENS, mask, regions, 5, 13)
            plain = pyerrprof.profile(recs, REFS, ec.LENS, regions, 5, 13)
            assert [[sum(row[:22]) for row in seg] for seg in got["counts"]] == [[sum(row[:21]) for row in seg] for seg in plain["counts"]]
            assert got["n_masked_events"] > 0 and got["n_eligible"] == plain["n_eligible"] > 50
        comp = pyerrprof.profile(recs, REFS, ec.LENS, pyerrmask.complement(mask, ec.LENS), 5, 13)
        got = pyerrmask.profile(recs, REFS, ec.LENS, mask, None, 5, 13)
        assert [[row[:21] for row in seg] for seg in got["counts"]] == [[row[:21] for row in seg] for seg in comp["counts"]], share
    assert pyerrmask.complement([(0, 0, 2), (0, 5, 100), (2, 3, 4)], ec.LENS) == [(0, 2, 5), (1, 0, 50), (2, 0, 3), (2, 4, 30)]


def bgzf(data, block):
    return b"".join(pybam.bgzf_block(data[o:o + block]) for o in range(0, len(data), block)) + pybam.EOF_BLOCK


def test_mask_load_against_the_model(built, tmp_path):
    """gce_mask_load on every hand text: as .vcf, as one gzip member, as two gzip members cut inside a line and as BGZF with members of 300
    bytes, so that lines are cut between members; every counter and interval equal the model's and the hand-written ones"""
    from gencore_amd import bamio
    for cs in mc.vcf_cases():
        text = cs["text"]
        forms = {"a.vcf": text, "b.vcf.gz": gzip.compress(text), "c.vcf.gz": gzip.compress(text[:len(text) // 2]) + gzip.compress(text[len(text) // 2:]), "d.vcf.gz": bgzf(text, 300)}
        want = pyerrmask.parse_vcf(text, ec.NAMES, mc.CLAMP)
        for name, data in forms.items():
            (tmp_path / name).write_bytes(data)
            got = bamio.load_mask(tmp_path / name, ec.NAMES, mc.CLAMP, threads=2)
            assert got == {k: want[k] for k in pyerrmask.COUNTERS + ["intervals"]}, (cs["label"], name)
            assert got["intervals"] == cs["intervals"] and {k: got[k] for k in pyerrmask.COUNTERS} == cs["counters"], (cs["label"], name)
            assert pyerrmask.load(tmp_path / name, ec.NAMES, mc.CLAMP) == want
    assert len(bgzf(mc.vcf_cases()[9]["text"], 300)) > 3 * 28                       # (several members)


def test_mask_load_bed_and_refusals(built, tmp_path):
    from gencore_amd import bamio, capi
    bed = tmp_path / "m.bed"
    bed.write_text("#a comment\nc1\t45\t60\nzz\t0\t5\nc0\t38\t45\nc0\t-3\t2\nc2\t0\t9\nc1\t44\t45\n")
    want = pyerrmask.load(bed, ec.NAMES, mc.CLAMP)
    assert want["intervals"] == [(0, 0, 2), (0, 38, 40), (1, 44, 50)] and (want["n_lines"], want["n_records"], want["n_unknown_contig"], want["n_no_alt"]) == (0, 6, 1, 0)
    assert want["n_masked_bases"] == 10
    assert bamio.load_mask(bed, ec.NAMES, mc.CLAMP) == {k: want[k] for k in pyerrmask.COUNTERS + ["intervals"]}
    for label, text, line, words in mc.refusals():
        for name, data in (("r.vcf", text), ("r.vcf.gz", bgzf(text, 7))):
            (tmp_path / name).write_bytes(data)
            with pytest.raises(capi.GceError) as ei:
                bamio.load_mask(tmp_path / name, ec.NAMES, mc.CLAMP)
            assert ei.value.status == -1 and str(ei.value).endswith(": variant mask line %d: %s" % (line, words)), (label, name, str(ei.value))
    for name in ("m.txt", "m.vcf.bgz", "m.bcf", "vcf"):
        (tmp_path / name).write_bytes(mc.vcf(("c0", 1, "A", "C")))
        with pytest.raises(capi.GceError) as ei:
            bamio.load_mask(tmp_path / name, ec.NAMES, mc.CLAMP)
        assert ei.value.status == -1 and pyerrmask.NAME_REFUSAL in str(ei.value) and all(e in str(ei.value) for e in (".vcf,", ".vcf.gz", ".bed"))
    with pytest.raises(capi.GceError) as ei:
        bamio.load_mask(tmp_path / "missing.vcf", ec.NAMES, mc.CLAMP)
    assert "cannot open the variant mask" in str(ei.value)


def test_truncated_gzip_is_refused(built, tmp_path):
    """a .vcf.gz cut short is no mask: zlib hands out the bytes it has and then an end of file, so every cut below leaves text whose last line
    still has its five fields (the cut falls in the genotypes behind them) and only the stream's own error tells.  Cut in the middle, by the
    last 20 bytes, inside the 8-byte trailer, in the second of two members and inside a BGZF member: `cannot inflate the variant mask`"""
    from gencore_amd import bamio, capi
    rng = np.random.RandomState(17)
    tail = lambda: "\t".join("%d/%d:%d,%d:%d" % tuple(rng.randint(0, 99, 5)) for _ in range(400))            # about 5 kB behind ALT, and hard to deflate
    text = mc.vcf() + "".join("c1\t%d\t.\tA\tC\tq\tPASS\t.\tGT:AD:DP\t%s\n" % (k + 1, tail()) for k in range(40)).encode()
    whole = gzip.compress(text)
    (tmp_path / "whole.vcf.gz").write_bytes(whole)
    assert bamio.load_mask(tmp_path / "whole.vcf.gz", ec.NAMES, mc.CLAMP)["n_records"] == 40
    two = gzip.compress(text[:len(text) // 2]) + gzip.compress(text[len(text) // 2:])
    cuts = {"middle": whole[:len(whole) // 2], "last_20_bytes": whole[:-20], "trailer": whole[:-4], "second_member": two[:-len(two) // 4], "bgzf_member": bgzf(text, 30000)[:-5000]}
    for label, data in cuts.items():
        (tmp_path / "t.vcf.gz").write_bytes(data)
        # what zlib still inflates ends inside a line's genotypes: it would parse as a complete, shorter mask
        part = zlib.decompressobj(31).decompress(data) if label != "second_member" else text[:len(text) // 2] + b"c1\t1\t.\tA\tC\tq"
        if label != "bgzf_member":
            assert pyerrmask.parse_vcf(part, ec.NAMES, mc.CLAMP)["n_records"] >= 1, label
        with pytest.raises(capi.GceError) as ei:
            bamio.load_mask(tmp_path / "t.vcf.gz", ec.NAMES, mc.CLAMP)
        assert ei.value.status == -1 and str(ei.value).endswith(": cannot inflate the variant mask"), (label, str(ei.value))


def test_symbols_prototypes_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_error_profile_masked(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *mask_path, "
            "const char *tsv_path /* NULL: no file */, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, "
            "uint64_t window_bytes, size_t device_budget_bytes, gce_errprof_run *out, gce_mask_run *mask, char err[256]);") in head
    assert "int gce_bam_error_profile_fragments_masked(" in head and "gce_fragerr_run *out, gce_mask_run *mask, char err[256]);" in head
    assert "int gce_mask_load(const char *path, int32_t n_ref, const char *const *names, const int64_t *lens, int threads, gce_mask *out, char err[256]);" in head
    assert "void gce_mask_free(gce_mask *m);" in head and "a symbolic SV allele" in head
    assert "without a variant mask" not in head
    lib = capi.load_library()
    for n in ("gce_mask_load", "gce_mask_free", "gce_bam_error_profile_masked", "gce_bam_error_profile_fragments_masked"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n)
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_errprof_set_mask", "gce_fragerr_set_mask"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS and len(re.findall(r"\b%s\(" % n, entry)) == 1, n
    assert "bamio_varmask.hpp" in open(os.path.join(ROOT, "gencore_amd", "csrc", "bamio.cpp")).read()
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(gce_mask_run),sizeof(gce_mask),sizeof(gce_errprof_run),'
                     'sizeof(gce_fragerr_run));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GceMaskRun), C.sizeof(capi.GceMask), C.sizeof(capi.GceErrprofRun),
                                                                                          C.sizeof(capi.GceFragerrRun)]
    assert C.sizeof(capi.GceMaskRun) == 72 and [n for n, _ in capi.GceMaskRun._fields_] == pyerrmask.COUNTERS + ["n_masked_events", "load_s", "fill_s"]
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the argument checks come before any device is touched
    run, frun, mrun, err = capi.GceErrprofRun(), capi.GceFragerrRun(), capi.GceMaskRun(), (C.c_char * 256)()
    bam, fa, vcf, tsv = (str(tmp_path / n).encode() for n in ("in.bam", "ref.fa", "m.vcf", "out.tsv"))
    plain = lambda f=fa, m=vcf, mr=C.byref(mrun), opt=0: lib.gce_bam_error_profile_masked(bam, f, None, m, tsv, 0, 1, 0, 0, 0x704, opt, 0, 0, C.byref(run), mr, err)
    frags = lambda f=fa, m=vcf, mr=C.byref(mrun), opt=0: lib.gce_bam_error_profile_fragments_masked(bam, f, None, m, tsv, None, 0, 1, 0, 0, 0x704, opt, 0, 0, C.byref(frun), mr, err)
    for call in (plain, frags):
        assert call(m=None) == -1 and err.value == b"bad argument" and call(mr=None) == -1 and call(f=None) == -1
        assert call(opt=4) == -1 and b"unknown option bit" in err.value
        assert call() == -1 and b"cannot open the reference FASTA" in err.value
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    for call in (plain, frags):
        assert call() == -1 and err.value == b"cannot open the variant mask"
        assert call(m=str(tmp_path).encode()) == -1 and err.value == b"cannot open the variant mask"
        assert call(m=fa) == -1 and err.value == pyerrmask.NAME_REFUSAL.encode()
    (tmp_path / "m.vcf").write_bytes(mc.vcf(("c0", 1, "A", "C")))
    for call in (plain, frags):
        assert call() == -1 and b"cannot open the BAM file" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert plain() == -1 and err.value == b"gce_bam_error_profile reads BAM, not SAM text"
    with pytest.raises(capi.GceError) as ei:
        bamio.error_profile_masked_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "m.vcf", tsv=tmp_path / "out.tsv", direct=True)
    assert ei.value.status == -1 and "reads BAM, not SAM text" in str(ei.value)
    with pytest.raises(capi.GceError):
        bamio.error_profile_fragments_masked_bam(tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "m.vcf", tsv=tmp_path / "out.tsv", overlap_tsv=tmp_path / "o.tsv")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "m.vcf", "ref.fa"]


def test_help_and_flag_validation(tmp_path, capsys):
    from gencore_amd.cli import EPILOG, build_parser, main
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--error_profile_mask FILE \[gencore_amd\]", h) and "--error_profile_mask FILE" in EPILOG and "MASKED" in EPILOG
    assert build_parser().parse_args(["-r", "x"]).error_profile_mask is None
    bam, fa, vcf = tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "m.vcf"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    vcf.write_bytes(mc.vcf(("c0", 1, "A", "C")))
    (tmp_path / "m.txt").write_text("c0\t1\t2\n")
    base = ["-i", str(bam), "-o", str(tmp_path / "out.bam"), "-r", str(fa)]
    for argv, words in ((base + ["--error_profile_mask", str(vcf)], "--error_profile_mask needs --error_profile or --error_profile_in"),
                        (base + ["--error_profile_mask", str(vcf), "--error_profile_fragments"], "--error_profile_fragments needs --error_profile or --error_profile_in"),
                        (base + ["--error_profile", str(tmp_path / "a.tsv"), "--error_profile_mask", str(tmp_path / "none.vcf")], "none.vcf' doesn't exist"),
                        (base + ["--error_profile_in", str(tmp_path / "b.tsv"), "--error_profile_mask", str(tmp_path / "m.txt")], "--error_profile_mask needs a .vcf, .vcf.gz or .bed file")):
        assert main(argv) == 255
        assert words in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "m.txt", "m.vcf", "ref.fa"]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """errmask_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("errmaskhost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "errmask_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "errmask_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, refs, lens, regions, mask, pairs, min_mapq=0, min_baseq=0, exclude=0x704):
    (d / "ref").write_text("".join("%s\n" % ("-" if r is None else r) for r in refs))
    (d / "intervals").write_text("".join("%d %d %d %d\n" % x for x in pypileup.intervals(regions, lens)[0]) if regions is not None else "")
    (d / "mask").write_text("".join("%d %d %d\n" % x for x in mask))
    (d / "frames").write_bytes(ec.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(len(lens)), str(min_mapq), str(min_baseq), str(exclude), str(int(pairs)), str(d / "ref"),
                        "-" if regions is None else str(d / "intervals"), str(d / "mask"), str(d / "frames"), str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    tables = np.frombuffer((d / "out").read_bytes(), np.uint64).reshape(2, 3, pyerrprof.MAX_CYCLE, pyerrprof.ROW).tolist()
    return [int(x) for x in r.stdout.splitlines()[-1].split()[1:]], tables[0], tables[1]


def test_masked_record_functions_on_the_host(host_check):
    """the masked errprof::count_record and errprof::paired_walk on the host, under -fsanitize=address,undefined, with one lane and with 16
    and the bitmap in a heap block of its exact size: every counter equals the model's and the hand-written numbers"""
    d, exe = host_check
    for cs in mc.record_cases():
        for pairs in (False, True):
            _, counts, ovl = host_run(d, exe, cs["records"], REFS, ec.LENS, ec.regions_of(cs), model_mask(cs), pairs, cs["min_mapq"], cs["min_baseq"], cs["exclude"])
            assert counts == run_model(cs)["counts"] and not any(any(row) for seg in ovl for row in seg), cs["label"]
            assert pyerrmask.nonzero(dict(counts=counts)) == ec.expected(cs), cs["label"]
    for cs in mc.pair_cases():
        head, counts, ovl = host_run(d, exe, cs["records"], REFS, ec.LENS, ec.regions_of(cs), model_mask(cs), True, cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        res = run_model(cs, True)
        assert counts == res["counts"] and ovl == res["overlap"], cs["label"]
        assert head == [cs["pairs"], cs["shared"], cs["differ"]], cs["label"]
        assert pyerrmask.nonzero(dict(counts=counts)) == fx.expected(cs) and pyerrmask.nonzero_overlap(dict(overlap=ovl)) == fx.expected(cs, "xexpect"), cs["label"]


def test_masked_streams_on_the_host(host_check):
    """random records and every hand case's pairs in one stream under masks of 5 %, a half and all of the reference -- the last bit of the
    bitmap's last byte among them --, without a BED and with one: 16 lanes against the model"""
    d, exe = host_check
    recs = random_records(9)
    pairs = [r for cs in fx.all_cases() if cs["bed"] is None and cs["min_mapq"] == 0 for r in cs["records"]]
    assert sum(mc.CLAMP[:2]) % 8 != 0                                               # (the last byte of the bitmap is not whole)
    for share in (0.05, 0.5, 1.0):
        mask = random_mask(5, mc.CLAMP, share)
        for regions in (None, [(0, 3, 30), (1, 10, 30)]):
            _, counts, _ = host_run(d, exe, recs, REFS, ec.LENS, regions, mask, False, 5, 13)
            assert counts == pyerrmask.profile(recs, REFS, ec.LENS, mask, regions, 5, 13)["counts"]
    for cs in fx.all_cases():
        mask = random_mask(len(cs["label"]), mc.CLAMP, 0.3)
        head, counts, ovl = host_run(d, exe, cs["records"], REFS, ec.LENS, ec.regions_of(cs), mask, True, cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        res = pyerrmask.profile_fragments(cs["records"], REFS, ec.LENS, mask, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        assert counts == res["counts"] and ovl == res["overlap"], cs["label"]
        assert head == [res["n_pairs"], res["n_shared_columns"], res["n_disagree_columns"]] == [cs["pairs"], cs["shared"], cs["differ"]], cs["label"]
    assert pairs
