"""make_dev_params (gencore_amd/csrc/gce_params.hpp) without a GPU: the derived constants of DevParams -- score bias and table, the packed
thresholds, whether k_vote may run and why not, the key widths of the clustering scan, the split of the bucket words -- at the edges of
their arithmetic, in a program of its own (tests/params_host_check.hip) built with the address and undefined-behaviour sanitizers.
Every case starts from gce_params_default (asked of the library), one target of 1000 bases, no reads and the bucket table of an empty
step (4096 entries).  The expected values are derived by hand in the comments; none is computed here."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOT_NESTED = "quality thresholds not nested (low <= moderate <= high <= 127)"
BELOW_0 = "a score constant below 0"
ABOVE_116 = "a score constant above 116"
REQ_ABOVE_100 = "base_score_req above 100"

# What the defaults give.  Scores (8, 6, 4, 2): the smallest is 2, so bias = max(0, 3 - 2) = 1 (a score byte holds score + bias, and an overlap
# mismatch takes 3 off); max = 8 + 4 = 12 (an overlap match adds 4); lut = (bad, low, moderate, high) + bias, low byte first = 03 05 07 09.
# Thresholds 15 / 20 / 30 = 0x0F / 0x14 / 0x1E in every byte, nested and <= 127.  accept: min(6, 8, 2 + 4) = 6 >= base_score_req 6.
# key_bt: one target needs no bit, the floor is 1.  key_bl: 2^9 <= 1000 < 2^10.  nw_cb: 2^10 <= 0 + 1024 < 2^11.
# qmax = (1000 * 8 + 8) / 4096 + 1 = 1 + 1 = 2, two bits; nw_bd = 62 - 11 - 2 = 49, capped at 40.
DERIVED = dict(bias=1, max=12, lut=0x09070503, low4=0x0F0F0F0F, mod4=0x14141414, high4=0x1E1E1E1E, swar=1, min_lb=2, vote_ok=1, accept=1, prefix="", prefix_len=0,
               n_targets=1, key_bt=1, key_bl=10, nw_cb=11, nw_bd=40, nw_ok=1, tick_offset=0, tick_epoch0=0, tick_rem0=0, trailing=0, why="-")
ARGS = dict(nt=1, len=1000, N=0, tsize=4096, have_tick=0)
T32 = 0xFFFFFFFF

# (label, what the case sets, what that changes among the derived values -- None: the call is refused)
CASES = [
    ("defaults", {}, {}),
    # key_bt: the smallest b >= 1 with 2^b >= targets.  The genome grows with the targets, 1000 bases each: qmax = (8000 t + 8) / 4096 + 1 = 4, 6, 8, 10 for
    # t = 2..5 (3, 3, 4, 4 bits) and 8200008 / 4096 + 1 = 2002 for t = 1025 (11 bits: 62 - 11 - 11 = 40); no targets: qmax 1, one bit, and nw_ok 0
    ("targets_0", dict(nt=0), dict(n_targets=0, key_bt=1, key_bl=1, nw_ok=0)),
    ("targets_1", dict(nt=1), dict(key_bt=1)),
    ("targets_2", dict(nt=2), dict(n_targets=2, key_bt=1)),
    ("targets_3", dict(nt=3), dict(n_targets=3, key_bt=2)),
    ("targets_4", dict(nt=4), dict(n_targets=4, key_bt=2)),
    ("targets_5", dict(nt=5), dict(n_targets=5, key_bt=3)),
    ("targets_1025", dict(nt=1025), dict(n_targets=1025, key_bt=11, nw_bd=40)),
    # key_bl: the smallest b >= 1 with 2^b > longest contig, at most 32.  qmax = (8 L + 8) / 4096 + 1: 1 for L = 1; 129 for L = 65535 and 65536 (8 bits:
    # 62 - 11 - 8 = 43, capped); 2^23 + 1 for L = 2^32 - 1 (8 L + 8 = 2^35 exactly; 24 bits: 62 - 11 - 24 = 27)
    ("longest_1", dict(len=1), dict(key_bl=1)),
    ("longest_65535", dict(len=65535), dict(key_bl=16)),
    ("longest_65536", dict(len=65536), dict(key_bl=17)),
    ("longest_2^32-1", dict(len=T32), dict(key_bl=32, nw_bd=27)),
    # nw_cb: the smallest b >= 1 with 2^b > N + 1024, at most 33; two bits of qmax as in the defaults: nw_bd = 60 - nw_cb, capped at 40
    ("reads_1023", dict(N=1023), dict(nw_cb=11)),
    ("reads_1024", dict(N=1024), dict(nw_cb=12)),
    ("reads_2^32-1025", dict(N=2 ** 32 - 1025), dict(nw_cb=32, nw_bd=28)),
    ("reads_2^32-1024", dict(N=2 ** 32 - 1024), dict(nw_cb=33, nw_bd=27)),
    # nw_ok 0 for nw_bd < 1: a table of ONE bucket and t contigs of 2^32 - 1 bases.  qmax = 8 t (2^32 - 1) + 8 + 1: for t = 32768 that is 2^50 - 2^18 + 9 < 2^50,
    # 50 bits, nw_bd = 62 - 11 - 50 = 1; for t = 32769 it is 2^50 + 2^35 - 2^18 + 1 >= 2^50, 51 bits, nw_bd = 0.  key_bt: 2^15 = 32768 < 32769 <= 2^16.
    ("bucket_bits_1", dict(nt=32768, len=T32, tsize=1), dict(n_targets=32768, key_bt=15, key_bl=32, nw_bd=1, nw_ok=1)),
    ("bucket_bits_0", dict(nt=32769, len=T32, tsize=1), dict(n_targets=32769, key_bt=16, key_bl=32, nw_bd=0, nw_ok=0)),
    # k_vote off, and why.  25 = 0x19.  Neither the score table nor `accept` looks at the thresholds.
    ("not_nested", dict(low_quality=25, moderate_quality=20), dict(low4=0x19191919, swar=0, vote_ok=0, why=NOT_NESTED)),
    # score_bad -1: bias = 3 + 1 = 4, lut = (-1, 4, 6, 8) + 4 = 03 08 0A 0C; accept: min(6, 8, -1 + 4) = 3 < 6
    ("score_bad_-1", dict(score_bad=-1), dict(bias=4, lut=0x0C0A0803, min_lb=-1, vote_ok=0, accept=0, why=BELOW_0)),
    # score_high 117: max = 121 > 120; lut's top byte 118 = 0x76; accept: min(6, 117, 2 + 4) = 6
    ("score_high_117", dict(score_high=117), dict(max=121, lut=0x76070503, vote_ok=0, why=ABOVE_116)),
    ("base_score_req_101", dict(base_score_req=101), dict(vote_ok=0, accept=0, why=REQ_ABOVE_100)),
    # moderate 128 = 0x80 is beyond `high` 30, and beside a `high` of 200 = 0xC8 that one is beyond 127: "not nested" either way
    ("moderate_128", dict(moderate_quality=128), dict(mod4=0x80808080, swar=0, vote_ok=0, why=NOT_NESTED)),
    ("moderate_128_high_200", dict(moderate_quality=128, high_quality=200), dict(mod4=0x80808080, high4=0xC8C8C8C8, swar=0, vote_ok=0, why=NOT_NESTED)),
    # two reasons: the thresholds are named first
    ("not_nested_and_bad_-1", dict(low_quality=25, moderate_quality=20, score_bad=-1),
     dict(low4=0x19191919, swar=0, bias=4, lut=0x0C0A0803, min_lb=-1, vote_ok=0, accept=0, why=NOT_NESTED)),
    # accept: min(6, 8, 2 + 4) = 6 < 7; k_vote stays on
    ("base_score_req_7", dict(base_score_req=7), dict(accept=0)),
    # the score byte: max + bias = 250 + 4 + 1 = 255 fits (top byte of lut 251 = 0xFB), 251 + 4 + 1 = 256 does not
    ("score_high_250", dict(score_high=250), dict(max=254, lut=0xFB070503, vote_ok=0, why=ABOVE_116)),
    ("score_high_251", dict(score_high=251), None),
    # the score byte at its limit with every score inside the reference's `char`: high 123 + 4 = 127, bad -125 - 3 = -128, bias = 3 + 125 = 128,
    # max + bias = 255; lut = (-125, 4, 6, 123) + 128 = 03 84 86 FB; accept: min(6, 123, -125 + 4) < 6
    ("score_byte_255", dict(score_high=123, score_bad=-125), dict(bias=128, max=127, lut=0xFB868403, min_lb=-125, vote_ok=0, accept=0, why=BELOW_0)),
    # ticks: 25000 = 2 x 10000 + 5000; a batch that brings its own ticks starts at 0 and has no trailing flush
    ("tick_25000", dict(tick_offset=25000, trailing_flush=1), dict(tick_offset=25000, tick_epoch0=2, tick_rem0=5000, trailing=1)),
    ("own_ticks", dict(tick_offset=25000, trailing_flush=1, have_tick=1), {}),
    # the UMI prefix: copied, cut to 31 bytes where it fills the field
    ("prefix_UMI", dict(prefix="UMI"), dict(prefix="UMI", prefix_len=3)),
    ("prefix_32_bytes", dict(prefix="abcdefghijklmnopqrstuvwxyz012345"), dict(prefix="abcdefghijklmnopqrstuvwxyz01234", prefix_len=31)),
]

ECHOED = ("proper_umi_diff_threshold", "unproper_umi_diff_threshold", "duplex_mismatch_threshold", "cluster_size_req", "base_score_req", "high_quality", "moderate_quality",
          "low_quality", "score_high", "score_moderate", "score_low", "score_bad", "skip_low_complexity_cluster_threshold", "duplex_only", "disable_duplex", "flush_period")


def test_make_dev_params_under_sanitizers(built, tmp_path):
    from gencore_amd import capi
    prm = capi.GceParams()
    capi.load_library().gce_params_default(C.byref(prm))
    base = {n: int(getattr(prm, n)) for n in ECHOED + ("trailing_flush", "tick_offset")}
    assert [base[n] for n in ECHOED] == [1, 0, 2, 1, 6, 30, 20, 15, 8, 6, 4, 2, 1000, 0, 0, 10000] and prm.score_percent_req == 0.8
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    exe = str(tmp_path / "params_host_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "params_host_check.hip"), "-o", exe])
    argv, want = [], []
    for label, sets, changes in CASES:
        given = dict(base, score_percent_req=0.8, **ARGS)
        given.update(sets)
        argv.append(",".join([label] + ["%s=%s" % kv for kv in given.items()]))
        if changes is None:
            want.append("%s rc=-1" % label)
            continue
        d = dict(DERIVED, **changes)
        want.append(("%s rc=0 thr=%d/%d/%d/%d/%d q=%d/%d/%d s=%d/%d/%d/%d misc=%d/%d/%d/%d/0.8 " % ((label,) + tuple(given[n] for n in ECHOED)))
                    + "bias=%(bias)d max=%(max)d lut=0x%(lut)08X thr4=0x%(low4)08X/0x%(mod4)08X/0x%(high4)08X swar=%(swar)d min_lb=%(min_lb)d vote_ok=%(vote_ok)d accept=%(accept)d "
                      "prefix=%(prefix)s/%(prefix_len)d n_targets=%(n_targets)d key_bt=%(key_bt)d key_bl=%(key_bl)d nw_cb=%(nw_cb)d nw_bd=%(nw_bd)d nw_ok=%(nw_ok)d "
                      "tick=%(tick_offset)d/%(tick_epoch0)d/%(tick_rem0)d trailing=%(trailing)d why=%(why)s" % d)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run(["timeout", "-k", "10", "120", exe] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
