"""`python -m gencore_amd --sort` end to end on the GPU: an input shuffled pair-wise (mates adjacent, as an aligner writes them) run with
--sort gives the records, the report and the index that the model's sorted file (tests/pysort.py) gives without --sort; the shuffled input
without --sort still ends with the reference's message; the sharded runner reads the sorted temporary file too.
Every command line runs as its own process under `timeout`, one after another."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pybai
import pysort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSORTED = "ERROR: the input is unsorted. Please sort the input first."


def cli(args, cwd, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "gencore_amd"] + list(args), cwd=str(cwd), env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


def name_of(r):
    return r[36:36 + r[12] - 1]


@pytest.fixture(scope="module")
def inputs(built, tmp_path_factory):
    """sorted.bam: 4000 cfg3 pairs with UMIs on contigs scaled to 0.2 % (a 6 MB FASTA), coordinate-sorted (gce_bam_from_batch); ref.fa; U.bam: its records shuffled pair-wise with a
    fixed seed; M.bam: the model's sort of U"""
    from gencore_amd import synth
    from gencore_amd.bamio import write_batch_as_bam
    d = tmp_path_factory.mktemp("clisort")
    s = synth.generate("cfg3", n_pairs=4000, scale=0.002)
    tl = np.asarray(s.target_len, np.uint32)
    names = ["chr%d" % (i + 1) for i in range(len(tl))]
    write_batch_as_bam(str(d / "sorted.bam"), s.to_batch(), tl, names, threads=4)
    code = np.frombuffer(b"NATCG" + b"N" * 11, np.uint8)      # FastaReader's nibbles -> ASCII bases
    with open(str(d / "ref.fa"), "wb") as f:
        for nm, (nib, ln) in zip(names, s.reference_host()):
            if nib is None:
                continue
            both = np.empty(len(nib) * 2, np.uint8)
            both[0::2] = nib & 0xF
            both[1::2] = nib >> 4
            lines = np.concatenate([code[both[:ln]], np.zeros((-ln) % 60, np.uint8)]).reshape(-1, 60)       # 60 bases a line
            body = np.concatenate([lines, np.full((len(lines), 1), 10, np.uint8)], 1).reshape(-1)
            f.write(b">" + nm.encode() + b" synthetic\n" + body.tobytes().replace(b"\0", b""))
    hdr, recs = pysort.records(d / "sorted.bam")
    groups = {}
    for r in recs:
        groups.setdefault(name_of(r), []).append(r)
    order = list(groups)
    random.Random(11).shuffle(order)
    head = b"BAM\1" + len(hdr["text"]).to_bytes(4, "little") + hdr["text"] + hdr["contigs"]
    pysort.write(d / "U.bam", head, [r for k in order for r in groups[k]])
    mh, mrecs = pysort.sort_model(d / "U.bam")
    pysort.write(d / "M.bam", mh, mrecs)
    assert len(recs) >= 8000 and sorted(mrecs) == sorted(recs)
    return d


@pytest.mark.gpu
def test_sort_flag_against_the_model(inputs):
    d = inputs
    assert pysort.descents(d / "U.bam") > 0 and pysort.descents(d / "M.bam") == 0
    base = ["-r", "ref.fa", "-s", "2", "--threads", "4"]
    a = cli(["-i", "U.bam", "--sort", "-o", "a.bam", "-j", "a.json", "--index"] + base, d)
    assert a.returncode == 0, a.stderr
    b = cli(["-i", "M.bam", "-o", "b.bam", "-j", "b.json", "--index"] + base, d)
    assert b.returncode == 0, b.stderr
    ra, rb = pysort.records(d / "a.bam")[1], pysort.records(d / "b.bam")[1]
    assert len(ra) > 0 and ra == rb
    ja, jb = json.loads((d / "a.json").read_text()), json.loads((d / "b.json").read_text())
    assert "--sort" in ja.pop("command") and "--sort" not in jb.pop("command")
    assert ja == jb
    assert (d / "a.bam.bai").read_bytes() == pybai.build(d / "a.bam")
    assert sorted(p.name for p in d.iterdir() if p.name.endswith(".bam")) == ["M.bam", "U.bam", "a.bam", "b.bam", "sorted.bam"]
    assert [p.name for p in d.iterdir() if ".tmp" in p.name] == []
    # the sharded runner reads the sorted temporary file as well
    c = cli(["-i", "U.bam", "--sort", "--devices", "0,0", "-o", "c.bam", "-j", "c.json"] + base, d)
    assert c.returncode == 0, c.stderr
    assert pysort.records(d / "c.bam")[1] == ra
    assert sorted(p.name for p in d.iterdir() if p.name.endswith(".bam")) == ["M.bam", "U.bam", "a.bam", "b.bam", "c.bam", "sorted.bam"]


@pytest.mark.gpu
def test_unsorted_input_without_the_flag_is_still_refused(inputs):
    d = inputs
    assert pysort.descents(d / "U.bam") > 0
    r = cli(["-i", "U.bam", "-o", "n.bam", "-j", "n.json", "-r", "ref.fa", "-s", "2", "--threads", "4"], d)
    assert r.returncode == 255 and UNSORTED in r.stderr, r.stderr
