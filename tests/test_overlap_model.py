"""gce_bam_merge_overlap without a GPU: the model of rules P, E, M and Q (tests/pyovlmerge.py) against records whose new QUAL
bytes are written out by hand (tests/ovlcases.py), its idempotence, the cross-check that justifies rule Q (a plain pileup of the rewritten
records is the fragment pileup of the original ones), the symbol and its argument checks, the flag of the command line, and the dual-cursor
walk of the kernel (gce_ovlmerge.hpp) compiled for the host under the address and undefined-behaviour sanitizers and compared with the model."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import pytest

import fragcases as fc
import ovlcases as oc
import pileupcases as pc
import pyfragpile
import pyovlmerge
import pypileup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHOLE = [(0, 0, oc.LENS[0]), (1, 0, oc.LENS[1])]                     # a BED that covers the contigs whole


def run_model(cs, records=None):
    return pyovlmerge.merge_overlap(cs["records"] if records is None else records, cs["min_mapq"], cs["exclude"])


def test_premises_of_the_cases():
    cases = oc.all_cases()
    labels = [c["label"] for c in cases]
    assert len(set(labels)) == len(labels) and len(labels) >= 50
    for cs in cases:
        f = [pypileup.fields(r) for r in cs["records"]]
        keys = [pyfragpile.order_key(x["tid"], x["pos"]) for x in f]
        assert keys == sorted(keys), cs["label"]                                    # (the cases themselves obey rule P)
        assert all(x["tid"] < len(oc.LENS) and x["pos"] + pyfragpile.rlen_of(x) <= oc.LENS[x["tid"]] for x in f), cs["label"]
        for r, q in zip(cs["records"], cs["quals"]):
            assert q is None or (len(q) == pypileup.fields(r)["lseq"] and bytes(q) != pypileup.fields(r)["qual"]), cs["label"]
        assert cs["counters"]["n_records_changed"] == sum(q is not None for q in cs["quals"]), cs["label"]
    by = {c["label"]: c for c in cases}
    ops = lambda r: len(pypileup.fields(r)["cigar"])
    assert ops(by["r_19_ops"]["records"][0]) > 16 and pypileup.fields(by["r_300_bases"]["records"][0])["lseq"] == 300
    assert [by["run_%d" % L]["counters"]["n_shared_columns"] for L in (15, 16, 17, 33)] == [15, 16, 17, 33]
    assert by["g_b_inside_a"]["counters"]["n_shared_columns"] == 2 and by["q_agree"]["counters"]["n_shared_columns"] == 1


def test_model_against_hand_cases_and_idempotence():
    for cs in oc.all_cases():
        out, res = run_model(cs)
        assert out == oc.expected_records(cs), cs["label"]
        assert res == cs["counters"], (cs["label"], res)
        again, res2 = run_model(cs, out)
        assert again == out and res2["n_records_changed"] == 0, cs["label"]
        assert res2["n_columns_skipped"] == res2["n_shared_columns"] == res["n_shared_columns"], cs["label"]      # (every column the pass decided holds a 0 now)
    recs = oc.combined_stream()
    out, res = pyovlmerge.merge_overlap(recs)
    assert res["n_pairs"] >= 35 and res["n_ambiguous"] == 3 and res["n_pairs_no_qual"] == 2 and res["n_disagree_columns"] >= 15 and res["n_columns_skipped"] == 4
    assert pyovlmerge.merge_overlap(out)[0] == out


def test_model_writes_qual_bytes_only():
    recs = oc.fuzz_pairs(200, 3)
    out, res = pyovlmerge.merge_overlap(recs)
    assert res["n_pairs"] == 200 and res["n_shared_columns"] > 2000 and res["n_disagree_columns"] > 100 and res["n_records_changed"] > 350
    for r, w in zip(recs, out):
        o, n = pyovlmerge.qual_offset(r), pypileup.fields(r)["lseq"]
        assert len(r) == len(w) and r[:o] == w[:o] and r[o + n:] == w[o + n:]


def assert_pileup_premises(records, min_mapq, exclude):
    """what the cross-check rests on: no ambiguous name, shared-column qualities in 1..93, no D op of one mate on a column the other covers"""
    parsed, pairs, ambiguous = pyovlmerge.find_pairs(records, min_mapq, exclude)
    if ambiguous:
        return False
    for a, b in pairs:
        ca, cb = pyfragpile.columns(parsed[a]), pyfragpile.columns(parsed[b])
        if parsed[a]["qual"][0] == 0xFF or parsed[b]["qual"][0] == 0xFF:
            return False
        for x in set(ca) & set(cb):
            if ca[x][0] == pyfragpile.DEL or cb[x][0] == pyfragpile.DEL or not (1 <= ca[x][1] <= 93 and 1 <= cb[x][1] <= 93):
                return False
    return True


def no_lowq(res):
    """every per-strand counter but LOWQ (class 7)"""
    return [[v for k, v in enumerate(site) if k % 8 != 7] for site in res["counts"]]


def cross_check(records, min_mapq=0, exclude=0x704):
    out, _ = pyovlmerge.merge_overlap(records, min_mapq, exclude)
    for m in (1, 13, 93):
        plain = pypileup.pileup(out, WHOLE, oc.LENS, min_mapq, m, exclude)
        frag = pyfragpile.pileup_fragments(records, WHOLE, oc.LENS, min_mapq, m, exclude)
        assert no_lowq(plain) == no_lowq(frag), m
        for k in ["n_records", "n_eligible"] + pypileup.SKIPS:
            assert plain[k] == frag[k]


def test_pileup_of_the_rewritten_file_is_the_fragment_pileup():
    """why rule Q is what it is: where its premises hold, pypileup over the rewritten records counts what pyfragpile counts over the original
    ones, at every min_baseq from 1 on, in every counter but LOWQ"""
    met = 0
    for cs in oc.all_cases():
        if assert_pileup_premises(cs["records"], cs["min_mapq"], cs["exclude"]):
            cross_check(cs["records"], cs["min_mapq"], cs["exclude"])
            met += 1
    assert met >= 35
    for seed in (1, 2):
        recs = oc.fuzz_pairs(150, seed)
        assert assert_pileup_premises(recs, 0, 0x704) and len(pyovlmerge.find_pairs(recs)[1]) == 150
        cross_check(recs)


def test_model_rule_p_and_malformed():
    assert pyovlmerge.merge_overlap(fc.order_stream())[1]["n_records"] == fc.ORDER_N
    for k in (1, 37, fc.ORDER_N - 8, fc.ORDER_N - 3, fc.ORDER_N - 1):
        with pytest.raises(pypileup.PileupError) as ei:
            pyovlmerge.merge_overlap(fc.order_stream(k))
        assert ei.value.record == k and str(ei.value) == "BAM record %d (counting from 0) lies in front of its predecessor: gce_bam_merge_overlap needs a coordinate-sorted file" % k
    recs = fc.order_stream(5)
    with pytest.raises(pypileup.PileupError) as ei:
        pyovlmerge.merge_overlap(recs[:50] + [pc.malformed()[0][1]] + recs[50:])
    assert ei.value.record == 50 and "lies in front" not in str(ei.value)


def test_symbol_prototype_and_argument_checks(built, tmp_path):
    from gencore_amd import bamio, capi
    head = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "gencore_amd.h")).read())
    assert ("int gce_bam_merge_overlap(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes, size_t device_budget_bytes, "
            "int32_t min_mapq, uint32_t exclude_flags, uint32_t options, gce_overlap_run *out, char err[256]);") in head
    assert "#define GCE_OVERLAP_WEAK_HASH 1u" in head
    doc = head[head.index("Overlapping mates resolved in the file"):head.index("} gce_overlap_run;")]
    for word in ("addition under ABI v3", "Replaces: nothing in the reference's source", "Rule P", "Rule E", "Rule M", "Rule Q", "min(qa + qb, 93)", "(4 qa) / 5", "n_columns_skipped", "idempotent"):
        assert word in doc, word
    lib = capi.load_library()
    assert "gce_bam_merge_overlap" in capi.EXPORTED_SYMBOLS and hasattr(lib, "gce_bam_merge_overlap")
    entry = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_entry.h")).read()
    for n in ("gce_sort_overlap_begin", "gce_sort_overlap_finish"):
        assert hasattr(lib, n) and n not in capi.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % n, entry), n
    assert [n for n, _ in capi.GceOverlapRun._fields_] == ["n_records", "n_pairs", "n_pairs_no_qual", "n_ambiguous", "n_shared_columns", "n_disagree_columns", "n_columns_skipped",
                                                           "n_records_changed", "inflated_bytes", "out_bytes", "peak_device_bytes", "n_ref", "pad", "read_s", "inflate_index_s", "merge_s",
                                                           "write_s", "total_s"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %u\\n",sizeof(gce_overlap_run),offsetof(gce_overlap_run,n_ref),'
                     'offsetof(gce_overlap_run,merge_s),GCE_OVERLAP_WEAK_HASH);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [C.sizeof(capi.GceOverlapRun), capi.GceOverlapRun.n_ref.offset, capi.GceOverlapRun.merge_s.offset,
                                                                                           capi.GCE_OVERLAP_WEAK_HASH]
    for p in (probe, tmp_path / "probe"):
        p.unlink()
    # the argument checks come before any device is touched
    run, err = capi.GceOverlapRun(), (C.c_char * 256)()
    bam, outp = (str(tmp_path / n).encode() for n in ("in.bam", "out.bam"))
    call = lambda b=bam, o=outp, lv=-2, mq=0, opt=0, r=C.byref(run): lib.gce_bam_merge_overlap(b, o, 0, 1, lv, 0, 0, mq, 0x704, opt, r, err)
    assert call(b=None) == -1 and call(o=None) == -1 and call(r=None) == -1
    for v in (-4, 10):
        assert call(lv=v) == -1 and b"level should be -3, -2, -1 or 0..9" in err.value
    for v in (-1, 256):
        assert call(mq=v) == -1 and b"min_mapq should be 0..255" in err.value
    for opt in (2, 3, 1 << 31):
        assert call(opt=opt) == -1 and b"unknown option bit" in err.value and b"GCE_OVERLAP_WEAK_HASH" in err.value
    assert call() == -1 and b"cannot open the input BAM" in err.value
    (tmp_path / "in.bam").write_text("@HD\tVN:1.6\nr0\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    assert call() == -1 and err.value == b"gce_bam_merge_overlap reads BAM, not SAM text"
    assert call(o=bam) == -1 and b"the output path is the input file: gce_bam_merge_overlap does not rewrite a file in place" in err.value
    with pytest.raises(capi.GceError) as ei:
        bamio.merge_overlap_bam(tmp_path / "in.bam", tmp_path / "out.bam", weak_hash=True)
    assert ei.value.status == -1 and "gce_bam_merge_overlap reads BAM, not SAM text" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam"]
    sig = inspect.signature(bamio.merge_overlap_bam)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [("device", 0), ("threads", 0), ("level", -2), ("min_mapq", 0), ("exclude_flags", 0x704), ("weak_hash", False),
                                                                          ("window_bytes", 0), ("device_budget_bytes", 0)]


def test_kernel_has_no_column_walk():
    """k_ovl_merge's columns come from the two cursors: gce_ovlmerge.hpp never calls the per-column walk it replaces, and the walk and rule Q
    are host-and-device functions outside the device-only part"""
    src = open(os.path.join(ROOT, "gencore_amd", "csrc", "gce_ovlmerge.hpp")).read()
    host, dev = src.split("#ifndef GCE_OVLMERGE_HOST_CHECK")
    assert "fragpile::column" not in re.sub(r"//[^\n]*", "", src) and "asm" not in re.sub(r"//[^\n]*", "", src)
    for fn in ("struct Cursor", "void shared_runs(", "uint32_t rule_q(", "void merge_pair("):
        assert fn in host and fn not in dev, fn
    assert "k_ovl_merge" in dev and "ovlmerge::merge_pair(" in dev and "__global__" not in host


def test_help_and_usage_errors(tmp_path, capsys):
    from gencore_amd.cli import EPILOG, build_parser, main
    h = re.sub(r"\s+", " ", build_parser().format_help())
    assert re.search(r"--merge_overlap \[gencore_amd\]", h)
    assert "--merge_overlap" in EPILOG and "min(qa + qb, 93)" in EPILOG and "soft clipping" in EPILOG
    assert build_parser().parse_args(["-r", "x"]).merge_overlap is False
    bam, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    bam.write_bytes(b"\x1f\x8b\x08\x04")
    fa.write_text(">c0\nACGT\n")
    for out, words in (("-", "--merge_overlap needs an output file, not STDOUT"), (str(tmp_path / "out.sam"), "--merge_overlap needs BAM output, not SAM text")):
        assert main(["-i", str(bam), "-o", out, "-r", str(fa), "--merge_overlap"]) == 255
        assert ("ERROR: " + words) in capsys.readouterr().err
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """overlap_host_check, built once: a stand-alone program, nothing of it is loaded into Python"""
    d = tmp_path_factory.mktemp("overlaphost")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(d / "overlap_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "overlap_host_check.hip"), "-o", exe])
    return d, exe


def host_run(d, exe, records, min_mapq, exclude, weak):
    (d / "frames").write_bytes(pc.frames(records))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, str(min_mapq), str(exclude), str(int(weak)), str(d / "frames"), str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    rows = [[int(x) for x in l.split()] for l in lines if not l.startswith("#")]
    tail = [int(x) for x in [l for l in lines if l.startswith("#")][0].split()[1:]]
    raw, out, p = (d / "out").read_bytes(), [], 0
    while p < len(raw):
        (n,) = struct.unpack_from("<I", raw, p)
        out.append(raw[p + 4:p + 4 + n])
        p += 4 + n
    return rows, tail, out


def tail_of(res):
    return [res[k] for k in ("n_pairs", "n_pairs_no_qual", "n_ambiguous", "n_shared_columns", "n_disagree_columns", "n_columns_skipped", "n_records_changed")]


@pytest.mark.parametrize("weak", [False, True], ids=["hash", "weak_hash"])
def test_walk_and_rule_q_on_the_host(host_check, weak):
    """the dual-cursor walk, rule Q and the join's functions on the host, under -fsanitize=address,undefined, with one lane and with 16 lanes:
    every byte and every counter equals the model's and the hand-written ones, over all of ovlcases, over their records as one stream (where
    the weak hash puts them into 16 keys) and over the fuzz pairs; inside the program the cursors are held against fragpile::column"""
    d, exe = host_check
    for cs in oc.all_cases():
        rows, tail, out = host_run(d, exe, cs["records"], cs["min_mapq"], cs["exclude"], weak)
        want, res = run_model(cs)
        assert out == want == oc.expected_records(cs), cs["label"]
        assert tail == tail_of(res) + [-1] == tail_of(cs["counters"]) + [-1], cs["label"]
        assert len(rows) == len(cs["records"]) and sum(1 for r in rows if r[3] >= 0) == 2 * cs["counters"]["n_pairs"]
    for recs in (oc.combined_stream(), oc.fuzz_pairs(300, 5), oc.fuzz_pairs(100, 6, read_len=(100, 301))):
        want, res = pyovlmerge.merge_overlap(recs)
        rows, tail, out = host_run(d, exe, recs, 0, 0x704, weak)
        assert out == want and tail == tail_of(res) + [-1]
        again = host_run(d, exe, out, 0, 0x704, weak)
        assert again[2] == out and again[1][6] == 0
    rows, tail, _ = host_run(d, exe, fc.order_stream(37), 0, 0x704, weak)
    assert tail[7] == 37
