"""The host's file reader (gencore_amd/csrc/bamio_reader.hpp) without a GPU: PassReader::members_next and read_bam_header -- the loop that
inflates a file's first members until its BAM header is whole, once written in gce_run_bam_passes, in gce_bam_index and in the sort
runners' SortJob::open_input -- in a program of their own (tests/reader_host_check.cpp, over malloc instead of pinned memory) built with
the address and undefined-behaviour sanitizers.  The expected lines are what those three loops did with each file: all three went on while
the parser said "incomplete", stopped at "not BAM", and at the stream's end said "truncated header" / "truncated BAM header", the pass
runner "empty file" for a file of no bytes; only the pass runner went on reading for the first record's name."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HDR_END = 4 + 4 + len("@HD\tVN:1.6\tSO:coordinate\n") + 4 + 2 * (4 + 6 + 4)            # magic, l_text, text, n_ref, two contigs with names of 5 + NUL
RECORD = 4 + 32 + 9                                                                    # block_size, the fixed fields, "read_one" + NUL
CONTIGS = " chr11/200000 chr22/50000"
WINDOW = "BGZF block larger than a window"


def expected(member, first):
    """the program's lines; member: the size of each of the five header members, first: of name_cut's first member"""
    out = []
    for dialect, contigs in (("collect", CONTIGS), ("skip", "")):
        whole = "complete %d 2 %d%s -" % (HDR_END, HDR_END, contigs)
        out += [
            "header one_member %s piece=0 -> %s" % (dialect, whole),
            # the header over five members: five pieces of one member; pieces that end one byte short of a second member (1, 2 and 2 members);
            # everything in the default piece
            "header five_members %s piece=%d -> %s" % (dialect, member, whole),
            "header five_members %s piece=%d -> %s" % (dialect, 2 * member - 1, whole),
            "header five_members %s piece=0 -> %s" % (dialect, whole),
            # the piece ends two bytes into the first record's name: a caller that wants the name gets the next piece too, another does not
            "header name_cut %s+name piece=%d -> complete %d 2 %d%s read_one" % (dialect, first, HDR_END, HDR_END + RECORD, contigs),
            "header name_cut %s piece=%d -> complete %d 2 %d%s -" % (dialect, first, HDR_END, HDR_END + 38, contigs),
            "header ends_in_header %s piece=0 -> ended" % dialect,
            "header zero_bytes %s piece=0 -> empty" % dialect,
            "header wrong_magic %s piece=0 -> notbam" % dialect,
            "header five_members %s piece=%d -> failed: %s" % (dialect, member - 1, WINDOW),
        ]
    out += [
        "members five_members piece=%d -> 1 1 1 1 1 1 end" % member,                   # (the sixth: the EOF member)
        "members five_members piece=%d -> 1 2 3 end" % (2 * member - 1),
        "members five_members piece=0 -> 6 end",
        "members five_members piece=%d -> %s" % (member - 1, WINDOW),
        "members zero_bytes piece=0 -> end",
        "members cut_in_eof piece=0 -> 5 truncated BGZF block at the end of the file",
    ]
    return out


def test_reader_host_check_under_sanitizers(tmp_path):
    assert HDR_END == 65
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        cxx = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path / "reader_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "reader_host_check.cpp"), "-o", exe, "-lz", "-lpthread"])
    d = tmp_path / "cases"
    d.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = r.stdout.splitlines()
    sizes = dict(kv.split("=") for kv in got[0].split()[1:])
    member, first = int(sizes["member"]), int(sizes["first"])
    assert got[0].startswith("sizes ") and int(sizes["file"]) == 5 * member + 28 and member > 31
    want = expected(member, first)
    assert len(got) - 1 == len(want)
    for g, w in zip(got[1:], want):
        assert g == w
