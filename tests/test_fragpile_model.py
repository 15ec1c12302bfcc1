"""gce_bam_pileup_fragments without a GPU: the model of rules P, M and V (tests/pyfragpile.py) against records whose counters are
written out by hand (tests/fragcases.py), the symbol, its prototype and its argument checks, the flag of the command line, and the
per-record functions of the kernels (gce_fragpile.hpp) compiled for the host under the address and undefined-behaviour sanitizers and
compared with the model."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fragcases as fc
import pileupcases as pc
import pyfragpile
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_model(cs, records=None):
    return pyfragpile.pileup_fragments(cs["records"] if records is None else records, pc.regions_of(cs), pc.LENS, cs["min_mapq"], cs["min_baseq"], cs["exclude"])


def test_model_against_hand_cases():
    cases = fc.all_cases()
    labels = [c["label"] for c in cases]
    assert len(set(labels)) == len(labels) and len(labels) >= 40
    for cs in cases:
        keys = [pyfragpile.order_key(f["tid"], f["pos"]) for f in map(pypileup.fields, cs["records"])]
        assert keys == sorted(keys), cs["label"]                     # (the cases themselves obey rule P)
        res = run_model(cs)
        assert res["counts"] == pc.expected_counts(cs, list(zip(res["tid"], res["pos"]))), cs["label"]
        assert {k: res[k] for k in pypileup.SKIPS} == cs["skips"], cs["label"]
        assert {k: res[k] for k in pyfragpile.FRAG_COUNTERS} == fc.counters_of(cs), cs["label"]
        assert res["n_records"] == len(cs["records"]) == res["n_eligible"] + sum(cs["skips"].values()), cs["label"]
    # where mates are counted twice the depth can only be larger, and it is larger exactly by the columns rule V decided on a base
    for cs in cases:
        twice, once = pypileup.pileup(cs["records"], pc.regions_of(cs), pc.LENS, cs["min_mapq"], cs["min_baseq"], cs["exclude"]), run_model(cs)
        assert sum(map(sum, twice["counts"])) - sum(map(sum, once["counts"])) == cs["shared"], cs["label"]


def test_model_without_pairs_is_pypileup():
    """every pileupcases case (no record of them has 0x1), and their records as one sorted stream: the model's counters are pypileup's"""
    for cs in pc.all_cases():
        recs = sorted(cs["records"], key=lambda r: pyfragpile.order_key(pypileup.fields(r)["tid"], pypileup.fields(r)["pos"]))
        a = pyfragpile.pileup_fragments(recs, pc.regions_of(cs), pc.LENS, cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        b = pypileup.pileup(recs, pc.regions_of(cs), pc.LENS, cs["min_mapq"], cs["min_baseq"], cs["exclude"])
        assert all(a[k] == b[k] for k in b) and not any(a[k] for k in pyfragpile.FRAG_COUNTERS), cs["label"]


def test_model_rule_p():
    regions = [(0, 0, 100)]
    assert pyfragpile.pileup_fragments(fc.order_stream(), regions, pc.LENS)["n_records"] == fc.ORDER_N
    for k in (1, 37, fc.ORDER_N - 8, fc.ORDER_N - 3, fc.ORDER_N - 1):
        with pytest.raises(pypileup.PileupError) as ei:
            pyfragpile.pileup_fragments(fc.order_stream(k), regions, pc.LENS)
        assert ei.value.record == k and ("BAM record %d (counting from 0) lies in front of its predecessor" % k) in str(ei.value)
    # the malformed-record refusal comes first
    recs = fc.order_stream(5)
    with pytest.raises(pypileup.PileupError) as ei:
        pyfragpile.pileup_fragments(recs[:50] + [pc.malformed()[0][1]] + recs[50:], regions, pc.LENS)
    assert ei.value.record == 50 and "lies in front" not in str(ei.value)


def test_symbol_prototype_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_pileup_fragments(const char *bam_path, const char *bed_path, const char *fasta_path /* NULL: ref = N */, const char *tsv_path /* NULL: no file */, "
            "int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, "
            "gce_fragpile_run *out, char err[256]);") in head
    assert "void gce_fragpile_free(gce_fragpile_run *out);" in head and "#define GCE_FRAGPILE_DIRECT 1u" in head and "#define GCE_FRAGPILE_WEAK_HASH 2u" in head
    doc = head[head.index("gce_bam_pileup's table with every fragment counted once"):head.index("} gce_fragpile_run;")]
    assert "addition under ABI v3" in doc and "Replaces: nothing in the reference's source" in doc
    for word in ("Rule P", "Rule M", "Rule V", "lies in front of its predecessor", "n_ambiguous", "(4 q) / 5", "min(qa + qb, 200)"):
        assert word in doc, word
    lib = capi.load_library()
    for n in ("gce_bam_pileup_fragments", "gce_fragpile_free"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n)
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_fragpile_create", "gce_fragpile_set_sites", "gce_fragpile_window", "gce_fragpile_finish", "gce_fragpile_error", "gce_fragpile_destroy"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % n, entry), n
    assert lib.gce_bam_pileup_fragments.argtypes == lib.gce_bam_pileup.argtypes[:12] + [C.POINTER(capi.GceFragpileRun), C.c_char_p]
    assert [n for n, _ in capi.GceFragpileRun._fields_] == [n for n, _ in capi.GcePileupRun._fields_] + ["n_pairs", "n_shared_columns", "n_disagree_columns", "n_ambiguous", "n_deferred"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %u %u %zu\\n",sizeof(gce_fragpile_run),offsetof(gce_fragpile_run,n_pairs),'
                     'GCE_FRAGPILE_DIRECT,GCE_FRAGPILE_WEAK_HASH,sizeof(gce_pileup_run));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GceFragpileRun), capi.GceFragpileRun.n_pairs.offset, capi.GCE_FRAGPILE_DIRECT,
                                                                                           capi.GCE_FRAGPILE_WEAK_HASH, C.sizeof(capi.GcePileupRun)]
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the argument checks come before any device is touched
    run, err = capi.GceFragpileRun(), (C.c_char * 256)()
    bam, bed, fa, tsv = (str(tmp_path / n).encode() for n in ("in.bam", "t.bed", "ref.fa", "out.tsv"))
    call = lambda b=bam, d=bed, f=None, mq=0, bq=0, opt=0, r=C.byref(run): lib.gce_bam_pileup_fragments(b, d, f, tsv, 0, 1, mq, bq, 0x704, opt, 0, 0, r, err)
    assert call(b=None) == -1 and call(d=None) == -1 and call(r=None) == -1
    for v in (-1, 256):
        assert call(mq=v) == -1 and b"min_mapq should be 0..255" in err.value
        assert call(bq=v) == -1 and b"min_baseq should be 0..255" in err.value
    for opt in (4, 7, 1 << 31):
        assert call(opt=opt) == -1 and b"unknown option bit" in err.value and b"GCE_FRAGPILE_WEAK_HASH" in err.value
    assert call() == -1 and b"cannot open the BED file" in err.value
    (tmp_path / "t.bed").write_text("c0\t1\t2\n")
    assert call(f=fa) == -1 and b"cannot open the reference FASTA" in err.value
    (tmp_path / "ref.fa").write_text(">c0\nACGT\n")
    for opt in (0, 1, 2, 3):
        assert call(f=fa, opt=opt) == -1 and b"cannot open the BAM file" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert call(f=fa) == -1 and err.value == b"gce_bam_pileup_fragments reads BAM, not SAM text"
    with pytest.raises(capi.GceError) as ei:
        bamio.pileup_fragments_bam(tmp_path / "in.bam", tmp_path / "t.bed", tsv=tmp_path / "out.tsv", direct=True, weak_hash=True)
    assert ei.value.status == -1 and "gce_bam_pileup_fragments reads BAM, not SAM text" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa", "t.bed"]
    lib.gce_fragpile_free(None)
    lib.gce_fragpile_free(C.byref(run))
    sig = inspect.signature(bamio.pileup_fragments_bam)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("fasta", None), ("tsv", None), ("device", 0), ("threads", 0), ("min_mapq", 0), ("min_baseq", 0),
                                                                          ("exclude_flags", 0x704), ("direct", False), ("weak_hash", False), ("window_bytes", 0),
                                                                          ("device_budget_bytes", 0)]


def test_tile_is_checked_and_pileup_untouched():
    # k_frag_count's tile is k_pile_count's, PileAdd: its size is checked where it is declared, and gce_fragpile.hpp declares none of its own
    src = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_fragpile.hpp")).read()
    pile = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_pileup.hpp")).read()
    assert "static_assert(PU_TILE * 64u + 64u <= PU_LDS_PER_CU / PU_BLOCKS_PER_CU" in pile and pile.count("__shared__ uint32_t s_tile[DIRECT ? 1 : PU_TILE * 16u]") == 1
    assert "PileAdd<DIRECT> add;" in src and "add.open(" in src and "add.flush(" in src and "__shared__" not in src and "_TILE" not in src
    head = open(os.path.join(ROOT, "include", "gencore_amd.h")).read()
    assert "Overlapping mates are counted twice, there is no BAQ and no split by read group." in re.sub(r"\s*\n \* ", " ", head)


def test_help_and_usage_errors(tmp_path, capsys):
    from gencore_amd.cli import EPILOG, build_parser, main
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--pileup_fragments \[gencore_amd\]", h)
    assert "--pileup_fragments" in EPILOG and "counted twice" in EPILOG and "no BAQ" in EPILOG and "0x704" in EPILOG
    assert build_parser().parse_args(["-r", "x"]).pileup_fragments is False
    bam, fa, bed = tmp_path / "in.bam", tmp_path / "ref.fa", tmp_path / "t.bed"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    bed.write_text("c0\t1\t2\n")
    base = ["-i", str(bam), "-o", str(tmp_path / "out.bam"), "-r", str(fa)]
    for argv, words in ((base + ["-b", str(bed), "--pileup_fragments"], "--pileup_fragments needs --pileup or --pileup_in"),
                        (base + ["--pileup_fragments", "--pileup", str(tmp_path / "a.tsv")], "--pileup needs the targets of -b")):
        assert main(argv) == 255
        assert ("ERROR: " + words) in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa", "t.bed"]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """fragpile_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("fragpilehost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "fragpile_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "fragpile_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, regions, lens, min_mapq, min_baseq, exclude, weak):
    iv, n_sites = pypileup.intervals(regions, lens)
    (d / "intervals").write_text("".join("%d %d %d %d\n" % x for x in iv))
    (d / "frames").write_bytes(pc.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(len(lens)), str(min_mapq), str(min_baseq), str(exclude), str(int(weak)), str(d / "intervals"), str(d / "frames"),
                        str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    rows = [[int(x) for x in l.split()] for l in lines if not l.startswith("#")]
    tail = [int(x) for x in [l for l in lines if l.startswith("#")][0].split()[1:]]
    return rows, tail, np.frombuffer((d / "out").read_bytes(), np.uint32).reshape(n_sites, 16).tolist()


@pytest.mark.parametrize("weak", [False, True], ids=["hash", "weak_hash"])
def test_record_functions_on_the_host(host_check, weak):
    """fragpile::candidate, key, same_group, is_pair, column and paired_walk on the host, under -fsanitize=address,undefined, with one lane and
    with 16 lanes: every counter equals the model's and the hand-written numbers, over all of fragcases; then all cases' records as one
    stream under distinct names, where the weak hash puts them into 16 keys"""
    d, exe = host_check
    for cs in fc.all_cases():
        rows, tail, counts = host_run(d, exe, cs["records"], pc.regions_of(cs), pc.LENS, cs["min_mapq"], cs["min_baseq"], cs["exclude"], weak)
        res = run_model(cs)
        assert counts == res["counts"] == pc.expected_counts(cs, list(zip(res["tid"], res["pos"]))), cs["label"]
        assert tail == [cs["pairs"], cs["shared"], cs["differ"], cs["ambiguous"], -1], cs["label"]
        assert len(rows) == len(cs["records"]) and sum(1 for r in rows if r[5] >= 0) == 2 * cs["pairs"]
    regions = [(0, 9, 13)]
    recs = []
    for k, cs in enumerate(c for c in fc.all_cases() if c["min_mapq"] == 0 and c["exclude"] == 0x704):
        for r in cs["records"]:
            nm = pypileup.fields(r) and bytes(r[36:36 + r[12] - 1])
            b = bytearray(r)
            tail = bytes(b[36 + b[12]:])
            new = nm + b"_%02d" % k + b"\0"
            b = b[:36] + new + tail
            b[12] = len(new)
            b[0:4] = (len(b) - 4).to_bytes(4, "little")
            recs.append(bytes(b))
    recs.sort(key=lambda r: pyfragpile.order_key(pypileup.fields(r)["tid"], pypileup.fields(r)["pos"]))
    for bq in (0, 20):
        res = pyfragpile.pileup_fragments(recs, regions, pc.LENS, 0, bq)
        rows, tail, counts = host_run(d, exe, recs, regions, pc.LENS, 0, bq, 0x704, weak)
        assert counts == res["counts"] and tail == [res[k] for k in pyfragpile.FRAG_COUNTERS] + [-1]
        assert res["n_pairs"] >= 20 and res["n_shared_columns"] >= 20 and res["n_disagree_columns"] >= 5 and res["n_ambiguous"] == 3
    # rule P's key
    rows, tail, _ = host_run(d, exe, fc.order_stream(37), regions, pc.LENS, 0, 0, 0x704, weak)
    assert tail[4] == 37
    rows, tail, _ = host_run(d, exe, fc.order_stream(fc.ORDER_N - 1), regions, pc.LENS, 0, 0, 0x704, weak)
    assert tail[4] == fc.ORDER_N - 1
