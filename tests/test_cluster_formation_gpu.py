"""Cluster formation (gce_cluster.hpp) on the streams of tests/clustercases.py, engine against oracle: status, every record of the table
(diff_results), the output order, and the cluster counts.

The two cluster counts differ by definition: the oracle counts the clusters it hands to clusterByUMI (orc_result.n_clusters), the engine numbers every
cluster INSTANCE it forms (gce_get_pairing_tiers' n_clusters), those behind an unmapped read that no walk ever takes included -- they get tier NEVER, and so
do the clusters with left < 0 that finishConsensus writes pair by pair without clusterByUMI (gencore.cpp:401-407): no pairing tier works on either.
test_cluster_counts_mean_the_same_on_fuzz_streams holds `engine - NEVER == oracle` on the fuzz streams; per case the engine's count is held to the key-only
restatement of the read loop (clustercases.spec_formation: distinct (key, instance)) as well, and its NEVER count to the spec's pending clusters.

Measured on the MI355X: the module's 75 tests take 4.2 s in all, oracle runs included; the slowest are many:blocks_301 (307 717 reads) 0.54 s, its twin through
batch.tick 0.37 s, eventblocks:130 0.34 s and the 33 streams back to back on one engine 0.27 s; every other case is below 0.2 s."""
import pytest

import clustercases as cc
from parity_helpers import check_output_order, diff_results

pytestmark = pytest.mark.gpu


def oracle_of(case, prm=None):
    from oracle import oracle_py
    prm = prm or case.params()
    if case.events:
        b, ev = case.with_ticks()
        return oracle_py.run(b, prm, None, events=ev)
    return oracle_py.run(case.batch, prm)


def check_stream(tag, e, case, want, facts):
    """One stream on engine `e` (fresh or used): status, table, order, cluster counts."""
    from gencore_amd.capi import GceError
    batch = case.batch
    if case.events:
        batch, ev = case.with_ticks()
        e.set_flush_events(*ev)
    if want.status != 0:
        with pytest.raises(GceError) as ei:
            e.run(batch)
        assert ei.value.status == want.status, (tag, ei.value.status, want.status)
        e.reset()
        return
    got = e.run(batch)
    tier, read, counts = e.pairing_tiers()
    diffs = diff_results(batch, got, want) + check_output_order(batch, got.rows)
    assert not diffs, tag + ":\n" + "\n".join(diffs)
    assert len(tier) - counts["never"] == want.n_clusters, (tag, len(tier), counts, want.n_clusters)
    assert len(tier) == facts["n_taken"] + facts["n_pending"] + facts["n_as_they_are"], (tag, len(tier), facts)
    assert counts["never"] == facts["n_pending"] + facts["n_as_they_are"], (tag, counts, facts)          # (no pairing tier works on either kind)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case(built, name):
    """Per case one fresh engine."""
    from gencore_amd.engine import Engine
    case = cc.get(name)
    prm = case.params()
    want = oracle_of(case, prm)
    assert want.status == case.status, (want.status, want.message)
    e = Engine(prm)
    try:
        check_stream(name, e, case, want, case.facts)
    finally:
        e.close()


def test_cluster_counts_mean_the_same_on_fuzz_streams(built):
    """gce_get_pairing_tiers' n_clusters minus its NEVER clusters is the oracle's n_clusters (fuzz streams hold unmapped tails, exotic keys, small periods)."""
    import fuzzgen
    from gencore_amd.engine import Engine
    from oracle import oracle_py
    checked = 0
    for seed, kw in ((0, {}), (103, dict(umi_mode="colon", period=3)), (605, dict(n_mol=50, exotic=True)), (31, dict(n_mol=50))):
        batch, over, ref, contig_len = fuzzgen.make_case(seed, **kw)
        prm = fuzzgen.make_params(over, contig_len)
        want = oracle_py.run(batch, prm, ref)
        if want.status != 0:
            continue
        e = Engine(prm)
        try:
            e.run(batch, ref)
            tier, read, counts = e.pairing_tiers()
        finally:
            e.close()
        assert len(tier) - counts["never"] == want.n_clusters, (seed, len(tier), counts, want.n_clusters)
        f = cc.spec_formation(batch.core, prm.flush_period, contig_len)
        assert (len(tier), counts["never"]) == (f["n_taken"] + f["n_pending"] + f["n_as_they_are"], f["n_pending"] + f["n_as_they_are"]), (seed, len(tier), counts, f)
        checked += 1
    assert checked >= 3


BACK_TO_BACK = (["size:%d" % n for n in cc.SIZES] + cc.family("fill") + ["unmapped:tid<0@511", "unmapped:pos<0@1023", "unsorted:@1024", "unmapped:tid<0@0"]
                + ["home:taken", "nopack:negative_left_pending", "odd:period_5", "nopack:negative_left_pending_unmapped"] + ["size:%d" % n for n in reversed(cc.SIZES)])


def test_streams_back_to_back_on_one_engine(built):
    """The Sizes cases in growing order, the Block fill, Unmapped (with an unsorted stream, which ends its step early, between them), Home bucket, Odd
    and negative-left families, and the Sizes cases again in shrinking order on ONE engine at period 7: the bucket table is wiped by its users (k_scatter), so a formation that
    leaves a bucket behind shows in the next stream."""
    import dataclasses
    from gencore_amd.engine import Engine
    from oracle import oracle_py
    period = 7
    proto = dataclasses.replace(cc.get("size:1"), period=period)
    prm = proto.params()
    e = Engine(prm)
    try:
        for k, name in enumerate(BACK_TO_BACK):
            case = cc.get(name)
            assert tuple(case.contig_len) == cc.STD_CONTIGS and not case.over and not case.events
            want = oracle_py.run(case.batch, prm)
            assert want.status == case.status
            facts = cc.spec_formation(case.batch.core, period, cc.STD_CONTIGS) if case.status == 0 else {}
            check_stream("step %d (%s)" % (k, name), e, case, want, facts)
    finally:
        e.close()
