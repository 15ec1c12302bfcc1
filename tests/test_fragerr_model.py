"""gce_bam_error_profile_fragments without a GPU: the model of rules V' and X (tests/pyfragerr.py) against records whose counters
are written out by hand (tests/fragerrcases.py), the symbols, the prototype and its argument checks, the flag of the command line, and the
per-record functions of the kernel (gce_fragerr.hpp) compiled for the host under the address and undefined-behaviour sanitizers and
compared with the model."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import errprofcases as ec
import fragerrcases as fx
import pileupcases as pc
import pyerrprof
import pyfragerr
import pyfragpile
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_model(cs, records=None):
    return pyfragerr.profile_fragments(cs["records"] if records is None else records, ec.refs(), ec.LENS, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])


def sorted_records(recs):
    return sorted(recs, key=lambda r: pyfragpile.order_key(pypileup.fields(r)["tid"], pypileup.fields(r)["pos"]))


def renamed(r, suffix):
    """the record under its name + suffix"""
    b = bytearray(r)
    new = bytes(b[36:36 + b[12] - 1]) + suffix + b"\0"
    b = b[:36] + new + b[36 + b[12]:]
    b[12] = len(new)
    b[0:4] = (len(b) - 4).to_bytes(4, "little")
    return bytes(b)


def one_stream():
    """the records of every case that runs under the default thresholds and without a BED, each case under names of its own, sorted"""
    recs = []
    for k, cs in enumerate(c for c in fx.all_cases() if c["min_mapq"] == 0 and c["exclude"] == 0x704 and c["bed"] is None):
        recs += [renamed(r, b"_%02d" % k) for r in cs["records"]]
    return sorted_records(recs + fx.long_cigar_pair())


def test_model_against_hand_cases():
    cases = fx.all_cases()
    labels = [c["label"] for c in cases]
    assert len(set(labels)) == len(labels) and len(labels) >= 24
    for cs in cases:
        assert cs["records"] == sorted_records(cs["records"]), cs["label"]          # (the cases themselves obey rule P)
        assert all(6 <= pypileup.fields(r)["lseq"] <= 12 or cs["label"] in ("partner_too_long", "supplementary_beside_pair", "partner_d") for r in cs["records"]), cs["label"]
        res = run_model(cs)
        assert pyerrprof.nonzero(res) == fx.expected(cs), cs["label"]
        assert pyfragerr.nonzero_overlap(res) == fx.expected(cs, "xexpect"), cs["label"]
        assert {k: res[k] for k in pyerrprof.SKIPS} == cs["skips"], cs["label"]
        assert {k: res[k] for k in pyfragerr.FRAG_COUNTERS} == fx.counters_of(cs), cs["label"]
        assert res["n_records"] == len(cs["records"]) == res["n_eligible"] + sum(cs["skips"].values()), cs["label"]
        assert pyfragerr.overlap_sum(res) == 2 * res["n_shared_columns"], cs["label"]
        assert all(not any(row[21:]) for seg in res["overlap"] for row in seg)
        # counting mates twice can only count more M columns, and more exactly by the shared columns
        twice = pyerrprof.profile(cs["records"], ec.refs(), ec.LENS, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        cols = lambda x: sum(sum(row[:19]) for seg in x["counts"] for row in seg)
        assert cols(twice) - cols(res) == cs["shared"], cs["label"]


def test_model_on_a_stream_and_tables():
    recs = one_stream()
    for bq, regions in ((0, None), (20, None), (0, [(0, 22, 25), (0, 36, 41), (1, 10, 30)])):
        res = pyfragerr.profile_fragments(recs, ec.refs(), ec.LENS, regions, 0, bq)
        assert res["n_pairs"] >= 15 and res["n_shared_columns"] >= 20 and res["n_disagree_columns"] >= 4 and res["n_ambiguous"] == 3
        assert pyfragerr.overlap_sum(res) == 2 * res["n_shared_columns"]
    res = pyfragerr.profile_fragments(recs, ec.refs(), ec.LENS)
    text = pyfragerr.overlap_table(res).decode().splitlines()
    assert text[0] == "#segment\tcycle\tshared\terrors\t" + "\t".join(pyerrprof.CLASSES[:16]) + "\tAGREE_REF\tAGREE_ALT\tDIFF_OTHER\tUNUSABLE\tLOWQ"
    rows = [[int(v) for v in l.split("\t")] for l in text[1:]]
    assert all(len(r) == 25 and r[2] == sum(r[4:23]) and r[3] == sum(r[4 + 4 * a + b] for a in range(4) for b in range(4) if a != b) for r in rows)
    assert sum(r[2] + r[23] + r[24] for r in rows) == 2 * res["n_shared_columns"] and sum(r[3] for r in rows) > 0
    empty = run_model([c for c in fx.all_cases() if c["label"] == "bed_empty"][0])
    assert pyfragerr.overlap_table(empty) == pyfragerr.OVL_HEADER.encode() and pyerrprof.table(empty) == pyerrprof.HEADER.encode()


def test_model_without_candidates_is_pyerrprof():
    """every errprofcases case (no record of them has 0x1) as a sorted stream, and this file's cases with 0x1 taken off every flag: the
    primary table and the counters are pyerrprof's, the overlap table is empty"""
    unpaired = lambda r: r[:18] + (int.from_bytes(r[18:20], "little") & ~1).to_bytes(2, "little") + r[20:]
    streams = [(cs, sorted_records(cs["records"])) for cs in ec.all_cases()]
    streams += [(cs, [unpaired(r) for r in cs["records"]]) for cs in fx.all_cases()]
    for cs, recs in streams:
        a = pyfragerr.profile_fragments(recs, ec.refs(), ec.LENS, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        b = pyerrprof.profile(recs, ec.refs(), ec.LENS, ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        assert all(a[k] == b[k] for k in b) and not any(a[k] for k in pyfragerr.FRAG_COUNTERS) and pyfragerr.overlap_sum(a) == 0, cs["label"]


def test_model_rule_p():
    import fragcases as fc
    refs, lens = [None, None], pc.LENS
    assert pyfragerr.profile_fragments(fc.order_stream(), refs, lens)["n_records"] == fc.ORDER_N
    for k in (1, 37, fc.ORDER_N - 8, fc.ORDER_N - 3, fc.ORDER_N - 1):
        with pytest.raises(pyfragerr.ErrprofError) as ei:
            pyfragerr.profile_fragments(fc.order_stream(k), refs, lens)
        assert ei.value.record == k and str(ei.value) == ("BAM record %d (counting from 0) lies in front of its predecessor: gce_bam_error_profile_fragments needs a "
                                                            "coordinate-sorted file" % k)
    recs = fc.order_stream(5)
    with pytest.raises(pyfragerr.ErrprofError) as ei:
        pyfragerr.profile_fragments(recs[:50] + [pc.malformed()[0][1]] + recs[50:], refs, lens)
    assert ei.value.record == 50 and "lies in front" not in str(ei.value)


def test_symbol_prototype_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_error_profile_fragments(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *tsv_path /* NULL: no file */, "
            "const char *overlap_tsv_path /* NULL: no file */, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, "
            "uint64_t window_bytes, size_t device_budget_bytes, gce_fragerr_run *out, char err[256]);") in head
    assert "void gce_fragerr_free(gce_fragerr_run *out);" in head and "#define GCE_FRAGERR_DIRECT 1u" in head and "#define GCE_FRAGERR_WEAK_HASH 2u" in head
    doc = head[head.index("gce_bam_error_profile's table with every fragment counted once"):head.index("} gce_fragerr_run;")]
    assert "addition under ABI v3" in doc and "Replaces: nothing in the reference's source" in doc
    for word in ("Rule P", "Rule M", "Rule V'", "Rule X", "lies in front of its predecessor", "OVL_AGREE_ALT", "(4 q) / 5", "min(qa + qb, 200)", "2 n_shared_columns"):
        assert word in doc, word
    lib = capi.load_library()
    for n in ("gce_bam_error_profile_fragments", "gce_fragerr_free"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n)
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_fragerr_create", "gce_fragerr_set_ref", "gce_fragerr_set_sites", "gce_fragerr_window", "gce_fragerr_finish", "gce_fragerr_error", "gce_fragerr_destroy"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % n, entry), n
    assert lib.gce_bam_error_profile_fragments.argtypes == [C.c_char_p] * 5 + lib.gce_bam_error_profile.argtypes[4:12] + [C.POINTER(capi.GceFragerrRun), C.c_char_p]
    assert [n for n, _ in capi.GceFragerrRun._fields_] == [n for n, _ in capi.GceErrprofRun._fields_[:-1]] + ["n_pairs", "n_shared_columns", "n_disagree_columns", "n_ambiguous",
                                                                                                            "n_deferred", "counts", "overlap"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %zu %u %u %zu\\n",sizeof(gce_fragerr_run),'
                     'offsetof(gce_fragerr_run,n_pairs),offsetof(gce_fragerr_run,counts),offsetof(gce_fragerr_run,overlap),GCE_FRAGERR_DIRECT,GCE_FRAGERR_WEAK_HASH,'
                     'sizeof(gce_errprof_run));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GceFragerrRun), capi.GceFragerrRun.n_pairs.offset, capi.GceFragerrRun.counts.offset,
                                                                                           capi.GceFragerrRun.overlap.offset, capi.GCE_FRAGERR_DIRECT, capi.GCE_FRAGERR_WEAK_HASH,
                                                                                           C.sizeof(capi.GceErrprofRun)]
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the argument checks come before any device is touched
    run, err = capi.GceFragerrRun(), (C.c_char * 256)()
    bam, bed, fa, tsv, otsv = (str(tmp_path / n).encode() for n in ("in.bam", "t.bed", "ref.fa", "out.tsv", "ovl.tsv"))
    call = lambda b=bam, f=fa, d=None, mq=0, bq=0, opt=0, r=C.byref(run): lib.gce_bam_error_profile_fragments(b, f, d, tsv, otsv, 0, 1, mq, bq, 0x704, opt, 0, 0, r, err)
    assert call(b=None) == -1 and call(f=None) == -1 and call(r=None) == -1
    for v in (-1, 256):
        assert call(mq=v) == -1 and b"min_mapq should be 0..255" in err.value
        assert call(bq=v) == -1 and b"min_baseq should be 0..255" in err.value
    for opt in (4, 7, 1 << 31):
        assert call(opt=opt) == -1 and b"unknown option bit" in err.value and b"GCE_FRAGERR_WEAK_HASH" in err.value
    assert call() == -1 and b"cannot open the reference FASTA" in err.value
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    assert call(d=bed) == -1 and b"cannot open the BED file" in err.value
    (tmp_path / "t.bed").write_text("c0\t1\t2\n")
    for opt in (0, 1, 2, 3):
        assert call(d=bed, opt=opt) == -1 and b"cannot open the BAM file" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert call() == -1 and err.value == b"gce_bam_error_profile_fragments reads BAM, not SAM text"
    with pytest.raises(capi.GceError) as ei:
        bamio.error_profile_fragments_bam(tmp_path / "in.bam", tmp_path / "ref.fa", bed=tmp_path / "t.bed", tsv=tmp_path / "out.tsv", overlap_tsv=tmp_path / "ovl.tsv", direct=True,
                                          weak_hash=True)
    assert ei.value.status == -1 and "gce_bam_error_profile_fragments reads BAM, not SAM text" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa", "t.bed"]
    lib.gce_fragerr_free(None)
    lib.gce_fragerr_free(C.byref(run))
    sig = inspect.signature(bamio.error_profile_fragments_bam)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("bed", None), ("tsv", None), ("overlap_tsv", None), ("device", 0), ("threads", 0), ("min_mapq", 0),
                                                                          ("min_baseq", 0), ("exclude_flags", 0x704), ("direct", False), ("weak_hash", False), ("window_bytes", 0),
                                                                          ("device_budget_bytes", 0)]
    assert bamio.OVERLAP_CLASSES == tuple(pyfragerr.OVL_CLASSES)


def test_one_join_and_the_planes_are_checked():
    """the join's kernels are defined in gce_matejoin.hpp alone, both passes include it, and the count kernel's LDS is asserted against the CU"""
    csrc = os.path.join(ROOT, "gencore_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in ("gce_matejoin.hpp", "gce_fragpile.hpp", "gce_fragerr.hpp")}
    for k in ("void k_frag_prep(", "void k_frag_join(", "void k_frag_carry(", "struct FragView {", "FM_KEY0"):
        assert k in src["gce_matejoin.hpp"] and k not in src["gce_fragpile.hpp"] and k not in src["gce_fragerr.hpp"], k
    for n in ("gce_fragpile.hpp", "gce_fragerr.hpp"):
        assert '#include "gce_matejoin.hpp"' in src[n] and "J.run(this" in src[n]
    assert "static_assert(2u * EP_PLANE * 4u <= EP_LDS_PER_CU / EP_BLOCKS_PER_CU" in src["gce_fragerr.hpp"] and "cannot wrap" in src["gce_fragerr.hpp"]
    assert "asm" not in src["gce_fragerr.hpp"] and "asm" not in src["gce_matejoin.hpp"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4l." in design and "k_fragerr_count" in design and "gce_matejoin.hpp" in design


def test_help_and_usage_errors(tmp_path, capsys):
    from gencore_amd.cli import EPILOG, build_parser, main
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--error_profile_fragments \[gencore_amd\]", h)
    assert "--error_profile_fragments" in EPILOG and "FILE.overlap.tsv" in EPILOG and "AGREE_ALT" in EPILOG
    assert build_parser().parse_args(["-r", "x"]).error_profile_fragments is False
    bam, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    assert main(["-i", str(bam), "-o", str(tmp_path / "out.bam"), "-r", str(fa), "--error_profile_fragments"]) == 255
    assert "ERROR: --error_profile_fragments needs --error_profile or --error_profile_in" in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]


def test_flag_routes_both_tables(monkeypatch, tmp_path, capsys):
    """with the flag both --error_profile_in and --error_profile go through error_profile_fragments_bam with FILE.overlap.tsv beside each, and
    the second STDERR line follows the first; without it error_profile_bam is called as before"""
    from gencore_amd import bamio, cli, report
    calls = []

    class R:
        def __getattr__(self, k):
            return 0

    def note(name, ret=None):
        def f(*a, **kw):
            calls.append((name, a, kw))
            return ret if ret is not None else R()
        return f
    for n in ("error_profile_bam", "error_profile_fragments_bam", "index_bam"):
        monkeypatch.setattr(bamio, n, note(n))
    monkeypatch.setattr(bamio, "load_bed", note("load_bed", []))
    monkeypatch.setattr(bamio, "run_bam_passes", note("run", (None, {"pre": None, "post": None}, None)))
    monkeypatch.setattr(report, "read_header", lambda p: (["c0"], [4]))
    monkeypatch.setattr(report, "summary", lambda *a: "")
    monkeypatch.setattr(report, "write_json", note("json"))
    monkeypatch.setattr(os, "replace", lambda a, b: None)
    bam, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    out = tmp_path / "out.bam"
    argv = ["-i", str(bam), "-o", str(out), "-r", str(fa), "-j", str(tmp_path / "r.json"), "--error_profile_in", str(tmp_path / "ei.tsv"), "--error_profile", str(tmp_path / "e.tsv"),
            "--error_profile_min_baseq", "9"]
    assert cli.main(argv + ["--error_profile_fragments"]) == 0
    errtext = capsys.readouterr().err
    got = [c for c in calls if c[0].startswith("error_profile")]
    assert [c[0] for c in got] == ["error_profile_fragments_bam"] * 2 and [c[1] for c in got] == [(str(bam), str(fa)), (str(out), str(fa))]
    for c, tsv in zip(got, ("ei.tsv", "e.tsv")):
        assert c[2] == dict(bed=None, tsv=str(tmp_path / tsv), overlap_tsv=str(tmp_path / tsv) + ".overlap.tsv", device=0, threads=0, min_mapq=0, min_baseq=9, exclude_flags=0x704,
                            device_budget_bytes=0)
    for label in ("error_profile_in", "error_profile"):
        assert ("%s: 0 records, 0 eligible, 0 bases, 0 mismatches\n%s: 0 pairs, 0 shared columns, 0 disagreeing\n" % (label, label)) in errtext
    del calls[:]
    assert cli.main(argv) == 0
    assert [c[0] for c in calls if c[0].startswith("error_profile")] == ["error_profile_bam"] * 2 and "pairs" not in capsys.readouterr().err


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """fragerr_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("fragerrhost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "fragerr_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fragerr_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, regions, min_mapq, min_baseq, exclude, weak):
    (d / "ref").write_text("".join("%s\n" % (s if s is not None else "-") for s in ec.refs()))
    bedarg = "-"
    if regions is not None:
        iv, _ = pypileup.intervals(regions, ec.LENS)
        (d / "intervals").write_text("".join("%d %d %d %d\n" % x for x in iv))
        bedarg = str(d / "intervals")
    (d / "frames").write_bytes(ec.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(len(ec.LENS)), str(min_mapq), str(min_baseq), str(exclude), str(int(weak)), str(d / "ref"), bedarg, str(d / "frames"),
                        str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    rows = [[int(x) for x in l.split()] for l in lines if not l.startswith("#")]
    tail = [int(x) for x in [l for l in lines if l.startswith("#")][0].split()[1:]]
    both = np.frombuffer((d / "out").read_bytes(), np.uint64).reshape(2, 3, pyerrprof.MAX_CYCLE, pyerrprof.ROW)
    return rows, tail, both[0].tolist(), both[1].tolist()


@pytest.mark.parametrize("weak", [False, True], ids=["hash", "weak_hash"])
def test_record_functions_on_the_host(host_check, weak):
    """errprof::Cursor and paired_walk (with scan_record, count_record and the join's four functions) on the host, under
    -fsanitize=address,undefined, with one lane and with 16: both tables equal the model's and the hand-written numbers over all of
    fragerrcases, then over all cases' records as one stream with a 40-op partner in it, with and without a BED; at every column the cursor
    says what fragpile::column says"""
    d, exe = host_check
    for cs in fx.all_cases():
        rows, tail, counts, ovl = host_run(d, exe, cs["records"], ec.regions_of(cs), cs["min_mapq"], cs["min_baseq"], cs["exclude"], weak)
        res = run_model(cs)
        assert counts == res["counts"] and ovl == res["overlap"], cs["label"]
        assert pyerrprof.nonzero(dict(counts=counts)) == fx.expected(cs) and pyfragerr.nonzero_overlap(dict(overlap=ovl)) == fx.expected(cs, "xexpect"), cs["label"]
        assert tail[:5] == [cs["pairs"], cs["shared"], cs["differ"], cs["ambiguous"], -1], cs["label"]
        assert len(rows) == len(cs["records"]) and sum(1 for r in rows if r[5] >= 0) == 2 * cs["pairs"]
        assert sum(map(sum, (row for seg in ovl for row in seg))) == 2 * cs["shared"]
    recs = one_stream()
    for bq, regions in ((0, None), (20, None), (0, [(0, 22, 25), (0, 36, 41), (1, 10, 30)])):
        res = pyfragerr.profile_fragments(recs, ec.refs(), ec.LENS, regions, 0, bq)
        rows, tail, counts, ovl = host_run(d, exe, recs, regions, 0, bq, 0x704, weak)
        assert counts == res["counts"] and ovl == res["overlap"] and tail[:5] == [res[k] for k in pyfragerr.FRAG_COUNTERS] + [-1]
        assert tail[5] > 500 and tail[6] == 40                                      # (cursor columns checked; the 40-op partner was among them)
    import fragcases as fc
    rows, tail, _, _ = host_run(d, exe, fc.order_stream(37), None, 0, 0, 0x704, weak)
    assert tail[4] == 37
