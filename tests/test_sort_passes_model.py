"""gce_bam_sort_passes without a GPU: gce_sort_pass_run's layout against the header, the exported symbol, the arithmetic of the
pass cuts, and the command line handing --device_memory to the sort."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 0xff00


def test_sort_pass_run_layout_matches_header(built, tmp_path):
    from gencore_amd import capi
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gencore_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",sizeof(gce_sort_pass_run),'
                   'offsetof(gce_sort_pass_run,n_passes),offsetof(gce_sort_pass_run,in_core),offsetof(gce_sort_pass_run,pass_bytes),offsetof(gce_sort_pass_run,resident_bytes),'
                   'offsetof(gce_sort_pass_run,key_pass_s),offsetof(gce_sort_pass_run,plan_s),offsetof(gce_sort_pass_run,pass_s));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = capi.GceSortPassRun
    assert sizes == [C.sizeof(S), S.n_passes.offset, S.in_core.offset, S.pass_bytes.offset, S.resident_bytes.offset, S.key_pass_s.offset, S.plan_s.offset, S.pass_s.offset]
    assert S.pass_s.size == 64 * 8 and S.pass_s.offset + S.pass_s.size == C.sizeof(S)
    assert "gce_bam_sort_passes" in capi.EXPORTED_SYMBOLS and hasattr(capi.load_library(), "gce_bam_sort_passes")


def cuts_of(total, P):
    """pass_bytes = ceil(total / P) rounded up to a multiple of 0xff00, n_passes = ceil(total / pass_bytes)"""
    pb = (-(-total // P) + M - 1) // M * M
    return pb, (-(-total // pb) if pb else 0)


def test_pass_cut_arithmetic():
    assert [cuts_of(0, P) for P in (1, 2, 64)] == [(0, 0)] * 3
    assert [cuts_of(1, P) for P in (1, 2, 64)] == [(M, 1)] * 3
    assert [cuts_of(M, P) for P in (1, 2, 64)] == [(M, 1)] * 3
    assert cuts_of(M + 1, 1) == (2 * M, 1) and cuts_of(M + 1, 2) == (M, 2) and cuts_of(M + 1, 64) == (M, 2)
    assert cuts_of(3 * M, 2) == (2 * M, 2) and cuts_of(3 * M, 3) == (M, 3) and cuts_of(64 * M + 5, 64) == (2 * M, 33)
    for total in (0, 1, M - 1, M, M + 1, 2 * M, 7 * M + 3, 64 * M, 64 * M + 1, 1000 * M + 17, (1 << 40) + 12345):
        for P in range(1, 65):
            pb, n = cuts_of(total, P)
            assert pb % M == 0 and n <= P
            if total == 0:
                assert (pb, n) == (0, 0)
                continue
            # the passes tile [0, total): all but the last are whole, the last is not empty; the cuts are member boundaries of rule F
            assert (n - 1) * pb < total <= n * pb and pb * P >= total
            assert pb - M < -(-total // P) <= pb
            assert all((k * pb) % M == 0 for k in range(n))
            # no fewer passes than asked for, unless the stream has fewer members than that
            assert n == P or -(-total // M) < P or n == -(-total // pb)
            if -(-total // M) % P == 0 and total % M == 0:
                assert n == P


def test_cli_hands_device_memory_to_the_sort(tmp_path, monkeypatch):
    from gencore_amd import bamio, cli
    from gencore_amd.capi import GceError
    (tmp_path / "ref.fa").write_text(">a\nACGT\n")
    (tmp_path / "in.bam").write_bytes(b"\x1f\x8b" + bytes(30))
    seen = []

    def recorder(bam, out, **kw):
        seen.append((bam, kw))
        raise GceError(-1, "recorded")

    monkeypatch.setattr(bamio, "sort_bam_passes", recorder)
    monkeypatch.chdir(tmp_path)
    for value, want in (("2", 2 << 30), ("auto", 0), (None, 0)):
        args = ["-i", "in.bam", "-r", "ref.fa", "-o", "o.bam", "--sort", "--devices", "3", "--threads", "5"] + (["--device_memory", value] if value else [])
        assert cli.main(args) == 255
        bam, kw = seen.pop()
        assert bam == "in.bam" and kw == dict(device=3, threads=5, level=-2, device_budget_bytes=want)
    assert seen == [] and sorted(p.name for p in tmp_path.iterdir()) == ["in.bam", "ref.fa"]
