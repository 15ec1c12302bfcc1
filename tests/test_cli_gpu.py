"""`python -m gencore_amd` end to end on the GPU: a BAM + FASTA (+ BED) on disk -> the command line -> output records equal to the oracle's,
a JSON report equal to one built here from the oracle's Stats and depth statistics with the reference's rules restated in Python
(src/jsonreporter.cpp:11-44, src/stats.cpp:131-193, src/bed.cpp:81-100, src/bed.h:29-34), and the summaries of Stats::print on stderr.
Every command line runs as its own process under `timeout`, one after another."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pybam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli(args, cwd, text=True, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "gencore_amd"] + list(args), cwd=str(cwd), env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=text)


def half_away(x):
    """C's round(): halves away from zero (Python's round() would round them to even)"""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def g6(x):
    """what json.loads makes of a double printed by a default ostream ("%g")"""
    return float("%g" % x)


def expected_block(st, names, off, depth, step, regions, counts, has_bed):
    mr, mb = st["reads"] - st["reads_unmapped"], st["bases"] - st["bases_unmapped"]
    b = {"total_reads": st["reads"], "total_bases": st["bases"], "mapped_reads": mr, "mapped_bases": mb, "mismatched_bases": st["base_mismatches"],
         "reads_with_mismatched_bases": st["reads_with_mismatches"], "mismatch_rate": g6(st["base_mismatches"] / mb),
         "total_mapping_clusters": st["clusters"], "multiple_fragments_clusters": st["multi_molecule_clusters"], "total_fragments": st["molecules"],
         "single_end_fragments": st["molecules_se"], "paired_end_fragments": st["molecules_pe"],
         "duplication_level_histogram": st["supporting_hist"][1:100], "coverage_sampling": step,
         "coverage": {nm: [half_away(int(depth[i]) / step) for i in range(off[c], off[c + 1])] for c, nm in enumerate(names)}}
    if has_bed:
        b["coverage_bed"] = {nm: [[rn, s, e, 0 if e <= s else half_away(int(n) / (e - s))] for (t, s, e, rn), n in zip(regions, counts) if t == c]
                             for c, nm in enumerate(names)}
    return b


def expected_summary(st, post):
    mr, mb = st["reads"] - st["reads_unmapped"], st["bases"] - st["bases_unmapped"]
    t = "Total reads: %d\nTotal bases: %d\n" % (st["reads"], st["bases"])
    t += "Mapped reads: %d (%f%%)\nMapped bases: %d (%f%%)\n" % (mr, mr * 100.0 / st["reads"], mb, mb * 100.0 / st["bases"])
    t += "Bases mismatched with reference: %d (%f%%)\n" % (st["base_mismatches"], st["base_mismatches"] * 100.0 / mb)
    t += "Reads with mismatched bases: %d (%f%%)\n" % (st["reads_with_mismatches"], st["reads_with_mismatches"] * 100.0 / mr)
    t += "Total mapping clusters: %d\nMapping clusters with multiple fragments: %d\n" % (st["clusters"], st["multi_molecule_clusters"])
    t += "Total fragments: %d\nFragments with single-end reads: %d\nFragments with paired-end reads: %d\n" % (
        st["molecules"], st["molecules_se"], st["molecules_pe"])
    if post:
        t += "\nSingle Stranded Consensus Sequence (has 'FR' tag): %d\nDuplex Consensus Sequence (has both 'FS' and 'RR' tags): %d\n" % (st["sscs"], st["dcs"])
    else:
        t += "Duplication level histogram: \n"
        for i in range(1, 11):
            if st["supporting_hist"][i] == 0:
                break
            t += "    Fragments with %d duplicates: %d\n" % (i, st["supporting_hist"][i])
    return t


def write_inputs(tmp_path, d, batch, regions):
    """in.bam, ref.fa and panel.bed as test_bamio.py / test_depth_bed.py write them; the BED names its regions r0, r1, .. and ends with a
    region on a contig the header does not have."""
    from test_bamio import records_of
    from test_cabi_driver import ascii_of
    tl = np.asarray(d.target_len, np.uint32)
    targets = [("chr%d" % (i + 1), int(l)) for i, l in enumerate(tl)]
    src, fa, bed = (str(tmp_path / x) for x in ("in.bam", "ref.fa", "panel.bed"))
    pybam.write_bam(src, records_of(batch), targets)
    with open(fa, "wb") as f:
        for (nm, _), bases in zip(targets, ascii_of(d.reference_host())):
            if bases is None:
                continue
            f.write(b">" + nm.encode() + b" synthetic\n")
            for o in range(0, len(bases), 60):
                f.write(bases[o:o + 60] + b"\n")
    with open(bed, "w") as f:
        f.write("# panel\n")
        for k, (t, a, z) in enumerate(regions):
            f.write("chr%d\t%d\t%d\tr%d\n" % (t + 1, a, z, k))
        f.write("chrNotInHeader\t5\t50\tx\n")
    return targets


def check_records(out_bam, targets, want, batch):
    _, tg, got = pybam.read_bam(out_bam)
    assert tg == targets
    assert len(got) == len(want.emitted())
    key = lambda r: (r["tid"], r["pos"], r["qname"], r["flag"], r["seq"])
    exp = sorted(({**r, "qname": r["qname"].rstrip("\0")} for r in want.records(batch)), key=key)
    assert [(g["tid"], g["pos"]) for g in got] == sorted((g["tid"], g["pos"]) for g in got)
    for g, e in zip(sorted(got, key=key), exp):
        assert (g["qname"], g["flag"], g["tid"], g["pos"], g["seq"], g["qual"]) == (e["qname"], e["flag"], e["tid"], e["pos"], e["seq"], e["qual"])
        assert g["aux"].get("FR", (None, -1))[1] == e["fr"] and g["aux"].get("RR", (None, -1))[1] == e["rr"]
        assert e["nm"] is None or g["aux"]["NM"][1] == e["nm"]


CASES = [
    # workload, pairs, BED, output name, extra flags, (supporting reads, ratio, score, high_qual) of the oracle run (None: the workload's)
    ("cfg3", 30000, True, "out.bam", ["-s", "2"], (2, 0.8, 6, 30)),
    ("cfg5", 3000, True, "out.bam", ["--coverage_sampling", "250"], (None, 0.8, 6, 30)),
    ("cfg2", 20000, False, "out.sam", ["-a", "0.6", "-c", "4", "--high_qual", "35"], (None, 0.6, 4, 35)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
def test_cli_end_to_end(built, oracle, tmp_path, case):
    from gencore_amd.bamio import sam_to_bam
    from gencore_amd.capi import default_params
    from test_depth_bed import depth_case
    workload, n_pairs, with_bed, out_name, extra, (sup, ratio, score, hq) = CASES[case]
    d, batch, _, regions = depth_case(workload, n_pairs)
    sup = d.info["supporting_reads"] if sup is None else sup
    if "-s" not in extra:
        extra = extra + ["-s", str(sup)]
    step = int(extra[extra.index("--coverage_sampling") + 1]) if "--coverage_sampling" in extra else 10000
    tl = np.asarray(d.target_len, np.uint32)
    prm = default_params(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix=d.info["umi_prefix"], cluster_size_req=sup,
                         score_percent_req=ratio, base_score_req=score, high_quality=hq)
    want = oracle.run(batch, prm, d.reference_host())
    assert want.status == 0
    off, pre_d, post_d, pre_b, post_b = oracle.depth_stats(batch, want, d.target_len, step, regions)
    targets = write_inputs(tmp_path, d, batch, regions)
    args = ["-i", "in.bam", "-o", out_name, "-r", "ref.fa", "-j", "r.json", "--threads", "4"] + (["-b", "panel.bed"] if with_bed else []) + extra
    r = cli(args, tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ""
    # records
    out = str(tmp_path / out_name)
    if out_name.endswith("sam"):
        assert open(out).read(1) == "@"
        sam_to_bam(out, str(tmp_path / "back.bam"), threads=2)
        out = str(tmp_path / "back.bam")
    check_records(out, targets, want, batch)
    # the JSON report
    pre, post = want.pre.as_dict(), want.post.as_dict()
    names = [t[0] for t in targets]
    named = [(t, a, z, "r%d" % k) for k, (t, a, z) in enumerate(regions)]
    command = "".join(a + " " for a in ["gencore"] + args)
    exp = {"summary": {"mapping_rate": g6((pre["reads"] - pre["reads_unmapped"]) / pre["reads"]),
                       "duplication_rate": g6(1.0 - (pre["molecules_se"] + 2 * pre["molecules_pe"]) / (pre["reads"] - pre["reads_unmapped"])),
                       "single_stranded_consensus_sequence": post["sscs"], "duplex_consensus_sequence": post["dcs"]},
           "before_processing": expected_block(pre, names, off, pre_d, step, named, pre_b, with_bed),
           "after_processing": expected_block(post, names, off, post_d, step, named, post_b, with_bed),
           "command": command}
    text = (tmp_path / "r.json").read_text()
    rep = json.loads(text)
    assert rep == exp
    assert list(rep) == list(exp) and list(rep["before_processing"]) == list(exp["before_processing"])
    assert text.startswith("{\n\t\"summary\": {\n\t\t\"mapping_rate\":") and text.endswith("\t\"command\": \"%s\"\n}" % command)
    # stderr: the two summaries, then the command line and the time
    want_err = ("----Before gencore processing:\n" + expected_summary(pre, False) + "\n----After gencore processing:\n" + expected_summary(post, True) +
                "\n" + command + "\n")
    assert want_err in r.stderr
    assert r.stderr.rstrip("\n").split("\n")[-1].startswith("gencore_amd v")


@pytest.mark.gpu
def test_cli_sharded_and_piped_output(built, tmp_path):
    """--devices 0,0,0 (three engines on one GPU, the sharded runner) writes the JSON report --devices 0 writes; `-o -` into a pipe gives the
    bytes `-o file.bam` gives (the runner never seeks on its output)."""
    from test_depth_bed import depth_case
    d, batch, _, regions = depth_case("cfg3", 8000)
    write_inputs(tmp_path, d, batch, regions)
    base = ["-i", "in.bam", "-r", "ref.fa", "-b", "panel.bed", "--threads", "4", "-s", str(d.info["supporting_reads"])]
    r1 = cli(base + ["-o", "one.bam", "-j", "one.json", "--devices", "0"], tmp_path)
    assert r1.returncode == 0, r1.stderr
    r3 = cli(base + ["-o", "three.bam", "-j", "three.json", "--devices", "0,0,0"], tmp_path)
    assert r3.returncode == 0, r3.stderr
    strip = lambda p: (tmp_path / p).read_text().rsplit("\t\"command\": ", 1)[0]
    assert strip("one.json") == strip("three.json") and "coverage_bed" in strip("one.json")
    rp = cli(base + ["-o", "-", "-j", "pipe.json"], tmp_path, text=False)
    assert rp.returncode == 0, rp.stderr.decode(errors="replace")
    assert len(rp.stdout) > 28 and rp.stdout == (tmp_path / "one.bam").read_bytes()
    assert not (tmp_path / "-").exists()
