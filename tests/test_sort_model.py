"""The sort model of tests/pysort.py (no GPU): its output on shuffled streams is in an order pybai accepts, is a permutation of the input's
records and keeps input order among equal keys; rule H's header cases; gce_sort_run's layout; the command line's --sort checks; the
input order tools/sort_bench.py makes."""
import ctypes as C
import os
import random
import struct
import subprocess
import sys

import pytest

import pybai
import pybam
import pysort
from test_bai_model import header, random_records, rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = [("a", 300000), ("b", 2000), ("c", 200000), ("d", 5000)]


def shuffled_records(rng, targets, n):
    """random_records' stream made hard for a sort: about a third of the records share (tid, pos) with another one, on both strands; some
    placed records have pos -1; unplaced records; everything shuffled"""
    recs = random_records(rng, targets, n, unplaced=n // 50)
    placed = [r for r in recs if r["tid"] >= 0]
    for r in rng.sample(placed, len(placed) // 3):
        o = rng.choice(placed)
        r["tid"], r["pos"] = o["tid"], o["pos"]
        if rng.random() < 0.5:
            r["flag"] |= 16
    for r in rng.sample(placed, 12):
        r["pos"] = -1
        if rng.random() < 0.5:
            r["flag"] |= 16
    rng.shuffle(recs)
    return recs


def skey(n_ref, r):
    return pysort.key(n_ref, 0, r)


@pytest.mark.parametrize("seed,block", [(1, 0xff00), (2, 700)])
def test_model_output(tmp_path, seed, block):
    rng = random.Random(seed)
    src, dst = tmp_path / "u.bam", tmp_path / "s.bam"
    pybam.write_bam(str(src), shuffled_records(rng, TARGETS, 800), TARGETS, text="@HD\tVN:1.6\tSO:unsorted\n", block=block, level=1)
    assert pysort.descents(src) > 0
    with pytest.raises(pybai.BaiError):
        pybai.build(src)
    hdr, recs = pysort.sort_model(src)
    pysort.write(dst, hdr, recs, block=block)
    pybai.build(dst)                                            # refuses a file that is out of (tid, pos) order
    assert pysort.descents(dst) == 0
    _, before = pysort.records(src)
    h2, after = pysort.records(dst)
    assert sorted(before) == sorted(after) and after == recs
    assert h2["text"] == b"@HD\tVN:1.6\tSO:coordinate\n"
    # input order among equal (t, p, r): the names r<i> are unique, so a record's bytes give its place in the input
    place = {r: k for k, r in enumerate(before)}
    assert len(place) == len(before)
    for a, b in zip(after, after[1:]):
        ka, kb = skey(4, a), skey(4, b)
        assert ka < kb or (ka == kb and place[a] < place[b])
    # the forward strand in front of the reverse strand at one position, pos -1 first on its contig, the unplaced records last
    n_un = pysort.n_unplaced(after)
    assert n_un > 0 and all(struct.unpack_from("<i", r, 4)[0] < 0 for r in after[-n_un:])
    assert any(skey(4, a)[:2] == skey(4, b)[:2] and skey(4, a)[2] < skey(4, b)[2] for a, b in zip(after, after[1:]))
    assert any(skey(4, r)[1] == 0 for r in after[:-n_un])


def test_model_refuses_a_contig_the_header_lacks(tmp_path):
    p = tmp_path / "bad.bam"
    pybam.write_bam(str(p), [rec(0, 0, 5, "10M"), rec(1, 1, 5, "10M"), rec(2, 2, 5, "10M")], TARGETS[:2], level=1)
    with pytest.raises(pysort.SortError) as ei:
        pysort.sort_model(p)
    assert "record 2 " in str(ei.value)


HEADER_CASES = [
    ("@HD\tVN:1.5\tSO:unsorted\tGO:query\n@SQ\tSN:a\tLN:300000\n@CO\tSO:unsorted\n", "@HD\tVN:1.5\tSO:coordinate\tGO:query\n@SQ\tSN:a\tLN:300000\n@CO\tSO:unsorted\n"),
    ("@HD\tVN:1.6\n@PG\tID:x\tSO:queryname\n", "@HD\tVN:1.6\tSO:coordinate\n@PG\tID:x\tSO:queryname\n"),
    ("@SQ\tSN:a\tLN:300000\n", "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:300000\n"),
    ("@HD\tVN:1.6\tSO:queryname\n\0\0\0\0\0", "@HD\tVN:1.6\tSO:coordinate\n"),
    ("", "@HD\tVN:1.6\tSO:coordinate\n"),
    ("@HD\tVN:1.6", "@HD\tVN:1.6\tSO:coordinate"),
]


@pytest.mark.parametrize("case", range(len(HEADER_CASES)))
def test_rule_h(tmp_path, case):
    text, want = HEADER_CASES[case]
    assert pysort.header_text(text.encode()) == want.encode()
    p = tmp_path / "h.bam"
    pybam.write_bam(str(p), [rec(0, 0, 5, "10M")], TARGETS[:2], text=text, level=1)
    hb, recs = pysort.sort_model(p)
    assert hb == header(TARGETS[:2], text=want) and len(recs) == 1


def test_sort_run_layout_matches_header(built, tmp_path):
    from gencore_amd import capi
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(gce_sort_run),'
                   'offsetof(gce_sort_run,n_ref),offsetof(gce_sort_run,read_s),offsetof(gce_sort_run,total_s));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = capi.GceSortRun
    assert sizes == [C.sizeof(S), S.n_ref.offset, S.read_s.offset, S.total_s.offset]
    assert "gce_bam_sort" in capi.EXPORTED_SYMBOLS and hasattr(capi.load_library(), "gce_bam_sort")


def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "gencore_amd"] + args, cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


def test_cli_sort_flag(tmp_path):
    from gencore_amd.cli import build_parser
    assert build_parser().parse_args(["-r", "x.fa"]).sort is False
    assert build_parser().parse_args(["-r", "x.fa", "--sort"]).sort is True
    h = run_cli(["--help"], tmp_path)
    assert h.returncode == 0 and "--sort" in h.stdout and "[gencore_amd] the input BAM is not coordinate-sorted" in " ".join(h.stdout.split())
    (tmp_path / "ref.fa").write_text(">a\nACGT\n")
    (tmp_path / "in.sam").write_text("@HD\tVN:1.6\n")
    r = run_cli(["-r", "ref.fa", "--sort", "-o", "o.bam"], tmp_path)
    assert r.returncode == 255 and r.stderr == "ERROR: --sort needs an input file, not STDIN\n"
    r = run_cli(["-i", "in.sam", "-r", "ref.fa", "--sort", "-o", "o.bam"], tmp_path)
    assert r.returncode == 255 and r.stderr == "ERROR: --sort needs BAM input, not SAM text\n"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.sam", "ref.fa"]


def test_sort_bench_aligner_order(built, tmp_path):
    """tools/sort_bench.py's input: the permuted batch (per-read arrays only, blobs in place) written by gce_bam_from_batch holds the sorted
    stream's records, mates adjacent, out of coordinate order"""
    import importlib.util
    import numpy as np
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    spec = importlib.util.spec_from_file_location("sort_bench", os.path.join(ROOT, "tools", "sort_bench.py"))
    sb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sb)
    d = synth.generate("cfg3", n_pairs=1500, scale=0.002)
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    write_batch_as_bam(str(tmp_path / "s.bam"), batch, tl, threads=2)
    write_batch_as_bam(str(tmp_path / "u.bam"), sb.aligner_order(batch), tl, text="@HD\tVN:1.6\tSO:unsorted\n", threads=2)
    s, u = pysort.records(tmp_path / "s.bam")[1], pysort.records(tmp_path / "u.bam")[1]
    assert sorted(s) == sorted(u) and pysort.descents(tmp_path / "u.bam") > len(u) // 8
    names = [r[36:36 + r[12] - 1] for r in u]
    assert sum(a == b for a, b in zip(names, names[1:])) == len(set(names)) == len(u) // 2
    assert pysort.sort_model(tmp_path / "u.bam")[1] != u
