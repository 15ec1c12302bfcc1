"""The BAI model of tests/pybai.py (no GPU): its bytes for a hand-derived case, region queries through its index against brute force on random
sorted streams, and the command line's --index checks."""
import random
import struct

import pytest

import pybai
import pybam


def rec(i, tid, pos, cigar, flag=0, L=10):
    return dict(qname="r%d" % i, flag=flag, tid=tid, pos=pos, mapq=60, cigar=cigar, mtid=-1, mpos=-1, isize=0, seq="A" * L, qual=[30] * L)


def header(targets, text="@HD\tVN:1.6\tSO:coordinate\n"):
    h = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(targets))
    for nm, ln in targets:
        h += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    return h


def test_model_hand_derived(tmp_path):
    """Three contigs (the middle one empty); on contig 0 a run of bin 4681, a long record of bin 585, bin 4681 again in the same BGZF block
    (the two chunks of 4681 merge); a placed unmapped record on contig 2 that straddles the two blocks; an unplaced record last."""
    targets = [("c0", 100000), ("c1", 5000), ("c2", 5000)]
    recs = [rec(0, 0, 100, "10M"), rec(1, 0, 150, "10000M2I10000M"), rec(2, 0, 200, "5M3D5M"), rec(3, 2, 5, "*", flag=4), rec(4, -1, -1, "*", flag=4)]
    h = header(targets)
    L = [len(pybam.record_bytes(r)) for r in recs]
    stream = h + b"".join(pybam.record_bytes(r) for r in recs)
    block = len(h) + L[0] + L[1] + L[2] + 5                    # record 3 starts in member 0 and ends in member 1
    m0, m1 = pybam.bgzf_block(stream[:block]), pybam.bgzf_block(stream[block:])
    path = tmp_path / "hand.bam"
    path.write_bytes(m0 + m1 + pybam.EOF_BLOCK)
    c0, c1 = len(m0), len(m1)
    s = [len(h)]
    for x in L:
        s.append(s[-1] + x)                                    # s[k]: where record k starts in the stream; s[5] its end
    v = [s[0], s[1], s[2], s[3], (c0 << 16) | (s[4] - block)]  # rule V (records 0-3 start in member 0, record 4 in member 1)
    eod = (c0 + c1) << 16
    # bins: 100+10 -> 4681; 150+20000 spans windows 0 and 1 -> 585; 200+10 -> 4681; the unmapped record: [5, 6) -> 4681
    want = b"BAI\1" + struct.pack("<i", 3)
    want += struct.pack("<i", 3)                               # contig 0: bins 585, 4681 and the pseudo-bin
    want += struct.pack("<Ii", 585, 1) + struct.pack("<QQ", v[1], v[2])
    want += struct.pack("<Ii", 4681, 1) + struct.pack("<QQ", v[0], v[3])    # [v0, v1] and [v2, v3] share member 0: merged
    want += struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", v[0], v[3], 3, 0)
    want += struct.pack("<i", 2) + struct.pack("<QQ", v[0], v[1])           # window 1 overlaps record 1 only
    want += struct.pack("<ii", 0, 0)                           # contig 1: nothing
    want += struct.pack("<i", 2)                               # contig 2: bin 4681 and the pseudo-bin, no mapped record: no intervals
    want += struct.pack("<Ii", 4681, 1) + struct.pack("<QQ", v[3], v[4])
    want += struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", v[3], v[4], 0, 1)
    want += struct.pack("<i", 0)
    want += struct.pack("<Q", 1)
    got = pybai.build(path)
    assert got == want
    n_ref, contigs, n_no_coor = pybai.parse_bai(got)
    assert n_ref == 3 and n_no_coor == 1 and contigs[0]["meta"] == (v[0], v[3], 3, 0)
    assert eod > v[4]


def random_records(rng, targets, n, unplaced=3):
    out = []
    for i in range(n):
        tid = rng.randrange(len(targets))
        pos = rng.randrange(0, targets[tid][1] - 200)
        if rng.random() < 0.05:
            cig, flag = "*", 4
        elif rng.random() < 0.05:
            cig, flag = "20M%dN20M" % rng.randrange(1000, 60000), 0
        else:
            cig, flag = "%dM" % rng.randrange(20, 150), 0
        out.append((tid, pos, cig, flag))
    out.sort(key=lambda x: (x[0], x[1]))
    recs = [rec(i, t, p, c, f) for i, (t, p, c, f) in enumerate(out)]
    recs += [rec(n + k, -1, -1, "*", 4) for k in range(unplaced)]
    return recs


@pytest.mark.parametrize("seed,block", [(1, 0xff00), (2, 700), (3, 3000)])
def test_model_query_equals_brute_force(tmp_path, seed, block):
    rng = random.Random(seed)
    targets = [("a", 300000), ("b", 2000), ("c", 200000)]
    path = tmp_path / "r.bam"
    pybam.write_bam(str(path), random_records(rng, targets, 600), targets, block=block, level=1)
    bai = pybai.build(path)
    for _ in range(60):
        t = rng.randrange(len(targets))
        a = rng.randrange(0, targets[t][1])
        z = a + rng.choice([1, 50, 5000, 40000])
        assert pybai.query(path, bai, t, a, z) == pybai.brute_force(path, t, a, z)


def test_model_refuses_unsorted(tmp_path):
    targets = [("a", 10000)]
    path = tmp_path / "u.bam"
    pybam.write_bam(str(path), [rec(0, 0, 50, "10M"), rec(1, 0, 40, "10M")], targets)
    with pytest.raises(pybai.BaiError) as ei:
        pybai.build(path)
    assert ei.value.record == 1


def run_cli(argv, capsys):
    from gencore_amd import cli
    rc = cli.main(argv)
    return rc, capsys.readouterr().err


@pytest.mark.parametrize("out,msg", [("-", "ERROR: --index needs an output file, not STDOUT"), ("x.sam", "ERROR: --index needs BAM output, not SAM text")])
def test_cli_index_rejections(tmp_path, capsys, monkeypatch, out, msg):
    (tmp_path / "in.bam").write_bytes(b"x")
    (tmp_path / "ref.fa").write_text(">c\nA\n")
    monkeypatch.chdir(tmp_path)
    rc, err = run_cli(["-i", "in.bam", "-r", "ref.fa", "-o", out, "--index"], capsys)
    assert rc == 255 and err.strip() == msg
    assert not (tmp_path / "gencore.json").exists()


def test_cli_help_names_index(capsys):
    from gencore_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["--help"])
    assert "--index" in capsys.readouterr().out


def test_bai_run_layout_and_symbol(built, tmp_path):
    """gce_bai_run of include/gencore_amd.h (compiled with gcc) and its ctypes mirror agree; gce_bam_index is exported (no GPU call)."""
    import ctypes as C
    import os
    import subprocess
    from gencore_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(gce_bai_run),'
                   'offsetof(gce_bai_run,n_ref),offsetof(gce_bai_run,total_s));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.GceBaiRun), capi.GceBaiRun.n_ref.offset, capi.GceBaiRun.total_s.offset]
    assert "gce_bam_index" in capi.EXPORTED_SYMBOLS and hasattr(capi.load_library(), "gce_bam_index")
