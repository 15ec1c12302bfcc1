"""The finish stage: no duplex pass on a stream none of whose UMIs holds a '_' (k_describe, StreamInfo::umi_us), and the Stats events of the groups
that are final in k_group_tail counted there (k_stats only counts the clusters of the duplex stage).

The CPU tests hold the stream builders (tests/finishcases.py) against the oracle: every stream runs clean and sets the trap it is meant to set.  The GPU
tests compare the engine with the oracle: the table, its order and both Stats blocks, bit for bit.
"""
import numpy as np
import pytest

import finishcases as fc
from parity_helpers import check_output_order, diff_results

_ORACLE = {}


def oracle(key, make):
    """(batch, prm, ref, oracle result) of a stream: built and run once, shared, never changed."""
    if key not in _ORACLE:
        from oracle import oracle_py
        batch, prm, ref = make()
        want = oracle_py.run(batch, prm, ref)
        assert want.status == 0, want.message
        _ORACLE[key] = (batch, prm, ref, want)
    return _ORACLE[key]


SETTINGS = {"s1": dict(cluster_size_req=1), "s2": dict(cluster_size_req=2), "duplex_only": dict(cluster_size_req=1, duplex_only=1)}


def s_stream(setting, extra):
    return oracle(("S", setting, extra), lambda: fc.build(fc.stream_s(extra), **SETTINGS[setting]))


def seen_stream(case):
    cl, prefix = fc.DUPLEX_SEEN[case]
    return oracle(("seen", case), lambda: fc.build(cl, umi_prefix=prefix, cluster_size_req=2))


def no_duplex_stream(case):
    return oracle(("nodup", case), lambda: fc.build(fc.NO_DUPLEX[case], cluster_size_req=1))


def edge_stream(shift, rot):
    return oracle(("edge", shift, rot), lambda: fc.build(fc.edges(shift, rot), cluster_size_req=2, disable_duplex=1))


def hist_stream():
    from gencore_amd.capi import GCE_MAX_SUPPORTING_READS
    return oracle("hist", lambda: fc.build(fc.hist_end(GCE_MAX_SUPPORTING_READS), cluster_size_req=2))


def mixed_stream():
    return oracle("mixed", lambda: fc.build(fc.mixed(), cluster_size_req=2))


def empty_stream(which):
    def make():
        prm, ref = fc.bare_params(cluster_size_req=1)
        return (fc.no_clustered_read() if which == "no_clustered_read" else fc.clusters_without_group()), prm, ref
    return oracle(("empty", which), make)


# ------------------------------------------------------------------------------------------------------------ CPU: the builders
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_stream_s_has_every_shape_and_no_duplex(setting):
    batch, prm, ref, want = s_stream(setting, False)
    cl = fc.stream_s()
    assert sorted({len(c.groups) for c in cl}) == [1, 2, 3] and sorted({g[1] for c in cl for g in c.groups}) == [1, 2, 3]
    assert any(g[2] for c in cl for g in c.groups)
    pre, post = want.pre.as_dict(), want.post.as_dict()
    assert want.n_groups == sum(len(c.groups) for c in cl) == pre["molecules"] and pre["clusters"] == len(cl) and post["dcs"] == 0
    assert pre["multi_molecule_clusters"] == sum(1 for c in cl if len(c.groups) > 1)
    if setting == "duplex_only":
        assert len(want.emitted()) == 0
    else:
        req = SETTINGS[setting]["cluster_size_req"]
        assert post["sscs"] == sum(1 for c in cl for g in c.groups if g[1] >= req)
    batch2, _, _, want2 = s_stream(setting, True)
    assert batch2.n == batch.n + 2 and want2.pre.as_dict()["clusters"] == len(cl) + 1 and want2.post.as_dict()["dcs"] == 0
    assert np.array_equal(batch2.core[:batch.n], batch.core)                                 # S' is S with two reads behind it


@pytest.mark.parametrize("case", sorted(fc.DUPLEX_SEEN))
def test_duplex_streams_give_one_dcs(case):
    batch, prm, ref, want = seen_stream(case)
    post = want.post.as_dict()
    assert post["dcs"] == 1 and post["sscs"] == 0 and len(want.emitted()) == 2 and want.n_groups == 2
    if case == "name_of_70":
        assert set(batch.core["l_qname"].tolist()) == {71}
    if case == "2x17_byte_walk":
        assert int(batch.core["l_qname"][0]) - 1 - 36 > 0                                     # the ':' lies in front of the name's last 32 bytes
    if case == "mi_only":
        assert batch.mi is not None and b":" not in bytes(batch.qname)


@pytest.mark.parametrize("case", sorted(fc.NO_DUPLEX))
def test_underscores_that_form_no_duplex(case):
    batch, prm, ref, want = no_duplex_stream(case)
    post = want.post.as_dict()
    assert post["dcs"] == 0 and post["sscs"] == want.n_groups == (2 if case == "leading_underscore" else 1)


def test_edge_streams_count_what_the_patterns_say():
    for rot in range(3):
        batch, prm, ref, want = edge_stream(0, rot)
        pre, post = want.pre.as_dict(), want.post.as_dict()
        written = [sum(1 for n in fc.EDGE_PATTERNS[(k + rot) % 3] if n >= 2) for k in range(fc.EDGE_CLUSTERS)]
        assert want.n_groups == 3 * fc.EDGE_CLUSTERS > 257 and pre["multi_molecule_clusters"] == fc.EDGE_CLUSTERS
        assert post["sscs"] == sum(written) and post["clusters"] == sum(1 for x in written if x) and post["multi_molecule_clusters"] == sum(1 for x in written if x > 1)
    assert sorted(sum(1 for n in fc.EDGE_PATTERNS[(21 + rot) % 3] if n >= 2) for rot in range(3)) == [0, 1, 2]


def test_histogram_end_stream():
    from gencore_amd.capi import GCE_MAX_SUPPORTING_READS as M
    batch, prm, ref, want = hist_stream()
    pre = want.pre.as_dict()
    assert pre["uncounted_supporting_reads"] == 1 and pre["supporting_hist"][M - 1] == 1 and pre["molecules"] == 2


def test_mixed_stream_has_both_kinds():
    batch, prm, ref, want = mixed_stream()
    pre, post = want.pre.as_dict(), want.post.as_dict()
    assert post["dcs"] >= 3 and post["sscs"] >= 4 and pre["clusters"] == len(fc.mixed())
    assert pre["molecules"] < want.n_groups                                                  # merged strands count once


@pytest.mark.parametrize("which", ("no_clustered_read", "clusters_without_group"))
def test_empty_streams(which):
    batch, prm, ref, want = empty_stream(which)
    pre = want.pre.as_dict()
    assert want.n_groups == 0 and pre["clusters"] == 0 and pre["molecules"] == 0 and pre["reads"] == batch.n
    assert len(want.emitted()) == batch.n


# ------------------------------------------------------------------------------------------------------------ GPU
def run_engine(stream, engine=None):
    from gencore_amd.engine import Engine
    batch, prm, ref, want = stream
    e = engine or Engine(prm)
    try:
        got = e.run(batch, ref)
    finally:
        if engine is None:
            e.close()
    diffs = diff_results(batch, got, want) + check_output_order(batch, got.rows)
    assert not diffs, "\n".join(diffs)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_both_paths_on_one_stream(setting):
    """S forms no duplex and has no '_' in a UMI: no duplex stage.  S' has one in a far-away single-pair cluster: the duplex stage and k_stats run.
    Both equal the oracle, and the records of S are the same in both."""
    s, s2 = s_stream(setting, False), s_stream(setting, True)
    got, got2 = run_engine(s), run_engine(s2)
    n = s[0].n
    for f in ("out_flag", "qname_src", "nm_new", "fr", "rr", "mate"):
        assert np.array_equal(getattr(got, f)[:n], getattr(got2, f)[:n]), f
    nq, ns = len(s[0].qual), len(s[0].seq)
    assert np.array_equal(got.qual[:nq], got2.qual[:nq]) and np.array_equal(got.seq[:ns], got2.seq[:ns])


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(fc.DUPLEX_SEEN))
def test_a_real_duplex_survives_wherever_the_underscore_is_seen(case):
    got = run_engine(seen_stream(case))
    assert got.post.as_dict()["dcs"] == 1 and len(got.emitted()) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(fc.NO_DUPLEX))
def test_underscores_that_must_not_set_off_a_duplex(case):
    got = run_engine(no_duplex_stream(case))
    assert got.post.as_dict()["dcs"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("rot", range(3))
@pytest.mark.parametrize("shift", range(3))
def test_fold_at_wave_and_block_edges(shift, rot):
    run_engine(edge_stream(shift, rot))


@pytest.mark.gpu
def test_histogram_end():
    from gencore_amd.capi import GCE_MAX_SUPPORTING_READS as M
    got = run_engine(hist_stream())
    pre = got.pre.as_dict()
    assert pre["uncounted_supporting_reads"] == 1 and pre["supporting_hist"][M - 1] == 1


@pytest.mark.gpu
def test_mixed_stream_adds_both_accumulators():
    run_engine(mixed_stream())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("no_clustered_read", "clusters_without_group"))
def test_empty_cases(which):
    run_engine(empty_stream(which))


@pytest.mark.gpu
def test_engine_reuse_starts_every_step_without_the_fact():
    """S, a duplex stream, S again through one engine: the second S must not inherit the duplex stream's '_' (nor the duplex stream S's lack of one)."""
    from gencore_amd.engine import Engine
    s = oracle("reuse_s", lambda: fc.build(fc.stream_s(), n_ref=1200, cluster_size_req=2))
    d = oracle("reuse_d", lambda: fc.build(fc.mixed(), n_ref=1200, cluster_size_req=2))
    e = Engine(s[1])
    try:
        a = run_engine(s, e)
        run_engine(d, e)
        c = run_engine(s, e)
        run_engine(d, e)
    finally:
        e.close()
    assert np.array_equal(a.pre.as_array(), c.pre.as_array()) and np.array_equal(a.post.as_array(), c.post.as_array())
