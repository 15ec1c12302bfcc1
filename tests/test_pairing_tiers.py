"""Every mate-pairing tier at its routing edges, engine against oracle (bit-exact) AND the tier that paired each cluster
(gce_get_pairing_tiers) against the routing spec of tests/paircases.py, in both dispatch orders of engine.hip: size classes with direct
hand-on (N > 10 C) and the flag-and-compact chain (N <= 10 C, forced by padding with one-pair clusters)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import paircases as pc
from parity_helpers import check_output_order, diff_results

pytestmark = pytest.mark.gpu


def run_stream_checked(clusters, mode, seed=0):
    """One engine run over `clusters` (padded into `mode`), bit-exact against the oracle, every cluster's tier as expected_tier says.
    Returns the tier counts."""
    from gencore_amd.engine import Engine
    from oracle import oracle_py
    st = pc.Stream(seed=seed)
    for cl in clusters:
        st.add(cl)
    if mode == "chain":
        st.pad_singletons(max(0, -(-st.n_reads // 8) - len(st.clusters)))
    assert st.mode() == mode
    batch, prm, ref, owner = st.build()
    want = oracle_py.run(batch, prm, ref)
    assert want.status == 0, want.message
    e = Engine(prm)
    try:
        got = e.run(batch, ref)
        tier, read, counts = e.pairing_tiers()
    finally:
        e.close()
    diffs = diff_results(batch, got, want) + check_output_order(batch, got.rows)
    assert not diffs, "\n".join(diffs)
    assert len(tier) == len(st.clusters) and counts["never"] == 0
    assert np.all(read < batch.n)
    seen = owner[read.astype(np.int64)]
    assert sorted(seen.tolist()) == list(range(len(st.clusters)))          # one engine cluster per stream cluster
    bad = []
    for c in range(len(tier)):
        cl = st.clusters[seen[c]]
        want_t = pc.expected_tier(cl, mode)
        if pc.TIERS[tier[c]] != want_t:
            bad.append("%s (%d reads): tier %s, expected %s" % (cl.label, cl.n, pc.TIERS[tier[c]], want_t))
    assert not bad, "\n".join(bad)
    return counts


MODES = ("classes", "chain")


@pytest.mark.parametrize("mode", MODES)
def test_core_edges(built, mode):
    """Size edges 1..4098, names of 63/64/65/254 bytes and UMIs of 16/17/24/25 bytes in every tier, a 65-byte name in the first /
    middle / last lane, the register tiers' name-order branches, the deep kernel's 16-byte window (names ending at cp+15/16/17 with
    longer names behind them, the short name's reads first or last), runs of 32 / 33 reads behind one window."""
    counts = run_stream_checked(pc.core_clusters(), mode)
    for t in pc.TIERS[1:]:
        assert counts[t] > 0, (t, counts)


@pytest.mark.parametrize("mode", MODES)
def test_false_hash_matches(built, mode):
    """Two different names with one h32 in clusters of <= 16, 17..32 and 33..64 reads: the exact check catches it, the generic kernels pair."""
    counts = run_stream_checked(pc.collision_clusters(), mode)
    assert counts["generic"] == 12


def test_deep_device_limit(built):
    """65 534 reads (PD_BIGMAX - 2) are the device-memory deep kernel's; 65 535 go to the generic kernels.  Size classes only: the
    oracle needs ~40 s for the stream (the 32 767-pair group), and the limit is one comparison the dispatch order does not touch."""
    cls = [pc.sized_cluster(pc.PD_BIGMAX - 2, b"big", label="65534"), pc.sized_cluster(pc.PD_BIGMAX - 1, b"gen", label="65535")]
    counts = run_stream_checked(cls, "classes")
    assert counts["deep_device"] >= 1 and counts["generic"] >= 1


def umi_mismatch_cluster(n, tag):
    """n reads, one name with a third read whose MI:Z UMI differs from its mates' (setRight: pair.cpp:201-212)."""
    cl = pc.filled_cluster(n - 1, tag, [tag + b":bad"], 0, shuffle=False)
    cl.fwd.append(tag + b":bad")
    cl.mi = {tag + b":bad": [b"u:ACGTACGT", b"u:ACGTACGT", b"u:TTTTCCCC"]}
    return cl


@pytest.mark.parametrize("n,tier", [(9, "sub16"), (25, "sub32"), (49, "fast"), (201, "deep_lds"), (4201, "deep_device")])
def test_set_right_umi_mismatch(built, n, tier):
    """A third read with another UMI in each tier: the engine returns the oracle's fatal status."""
    from gencore_amd.capi import GceError
    from gencore_amd.engine import run_stream
    from oracle import oracle_py
    cl = umi_mismatch_cluster(n, b"um%d" % n)
    assert pc.expected_tier(cl) == tier
    st = pc.Stream()
    st.add(cl)
    batch, prm, ref, _ = st.build()
    want = oracle_py.run(batch, prm, ref)
    assert want.status != 0
    with pytest.raises(GceError) as ei:
        run_stream(batch, prm, ref)
    assert ei.value.status == want.status


def test_set_right_umi_mismatch_generic(built):
    """... and in the generic kernels (a 65-byte name sends the cluster there)."""
    from gencore_amd.capi import GceError
    from gencore_amd.engine import run_stream
    from oracle import oracle_py
    cl = umi_mismatch_cluster(9, b"ug")
    long_ = b"ug:" + b"z" * 62
    cl.fwd = [long_ if x == b"ug:f0" else x for x in cl.fwd]
    cl.rev = [long_ if x == b"ug:f0" else x for x in cl.rev]
    assert pc.expected_tier(cl) == "generic"
    st = pc.Stream()
    st.add(cl)
    batch, prm, ref, _ = st.build()
    want = oracle_py.run(batch, prm, ref)
    assert want.status != 0
    with pytest.raises(GceError) as ei:
        run_stream(batch, prm, ref)
    assert ei.value.status == want.status


def test_tiers_without_the_aux_stream(built):
    """GCE_NO_AUX_STREAM (read once per process) runs the size-class tiers on one stream: a fresh child process, same checks."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import paircases as pc, test_pairing_tiers as t\n"
            "t.run_stream_checked(pc.core_clusters() + pc.collision_clusters(), 'classes')\n"
            "print('child ok')\n") % (root, os.path.join(root, "tests"))
    env = dict(os.environ, GCE_NO_AUX_STREAM="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
