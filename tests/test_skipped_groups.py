"""Groups the engine does not evaluate because nothing could write them (d_group_skipped, gce_groups.hpp; gce_get_skipped_groups).

The CPU tests hold the stream builders (tests/skipcases.py) against the oracle: every stream runs clean and the trap it sets is really there.  The GPU tests
run every stream through one engine and compare the table, its order and both Stats blocks bit for bit with the oracle, and the skipped count and the
per-kernel side counters with what the rule says.
"""
import pytest

import skipcases as sc
from parity_helpers import check_output_order, diff_results

_ORACLE = {}


def oracle(case):
    """(batch, prm, ref, facts, oracle result) of a case: built and run once, shared, never changed."""
    if case not in _ORACLE:
        from oracle import oracle_py
        batch, prm, ref, facts = sc.build(case)
        _ORACLE[case] = (batch, prm, ref, facts, oracle_py.run(batch, prm, ref))
    return _ORACLE[case]


# ------------------------------------------------------------------------------------------------------------ CPU: the builders
@pytest.mark.parametrize("case", sc.CASES)
def test_stream_runs_clean_in_the_oracle(case):
    batch, prm, ref, facts, want = oracle(case)
    assert want.status == 0, want.message
    assert want.n_groups == facts["groups"]
    pre = want.pre.as_dict()
    assert pre["clusters"] == facts["clusters"] and pre["molecules"] <= facts["groups"]


def test_builder_is_deterministic():
    a, b = sc.build("b")[0], sc.build("b")[0]
    for f in a.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), f


def test_case_a_emits_nothing_and_counts_its_molecules():
    batch, prm, ref, facts, want = oracle("a")
    pre, post = want.pre.as_dict(), want.post.as_dict()
    assert len(want.emitted()) == 0 and post["molecules"] == 0
    assert pre["molecules"] == 40 and pre["supporting_hist"][1] == 40
    assert pre["molecules_se"] == facts["mateless"] and pre["molecules_pe"] == 40 - facts["mateless"]


def test_case_b_writes_the_live_groups_only():
    batch, prm, ref, facts, want = oracle("b")
    assert want.post.as_dict()["sscs"] == facts["live"] and facts["live"] > 16
    assert want.pre.as_dict()["supporting_hist"][1] == facts["skipped"]
    assert [n for k, n in facts["live_runs"] if k == "skip"] == [1, 15, 16, 17, 40]


@pytest.mark.parametrize("case", ("c_pair", "c_third", "c_alone"))
def test_case_c_duplex(case):
    batch, prm, ref, facts, want = oracle(case)
    post = want.post.as_dict()
    assert post["dcs"] == facts["dcs"] and post["sscs"] == 0
    assert len(want.emitted()) == 2 * facts["dcs"]
    if facts["dcs"]:
        assert want.pre.as_dict()["supporting_hist"][2] == 1               # m1 + m2 = 2: the merged molecule


def test_case_e_low_complexity_singletons_are_se():
    batch, prm, ref, facts, want = oracle("e")
    pre = want.pre.as_dict()
    assert pre["molecules_se"] == facts["low"] and pre["molecules_pe"] == facts["groups"] - facts["low"]


def test_case_d_f_g_emit_what_the_settings_allow():
    assert len(oracle("d")[4].emitted()) == 0
    assert oracle("f")[4].post.as_dict()["sscs"] == 2                      # the two groups of three pairs
    assert oracle("g")[4].post.as_dict()["sscs"] == oracle("g")[3]["groups"]


# ------------------------------------------------------------------------------------------------------------ GPU
def run_engine(case):
    from gencore_amd.engine import Engine
    batch, prm, ref, facts, want = oracle(case)
    assert want.status == 0, want.message
    e = Engine(prm)
    try:
        got = e.run(batch, ref)
        vc, cc, skipped, batches = e.vote_counters(), e.consensus_counters(), e.skipped_groups(), e.vote_batches()
    finally:
        e.close()
    diffs = diff_results(batch, got, want) + check_output_order(batch, got.rows)
    print(case, "groups", vc["groups"], "skipped", skipped, "batches", batches, "sides per kernel", cc)
    assert not diffs, "\n".join(diffs)
    assert vc["groups"] == want.n_groups == facts["groups"]
    assert skipped == facts["skipped"], (skipped, facts)
    assert sum(cc.values()) == 2 * (vc["groups"] - skipped), (cc, vc, skipped)       # every side of a live group is finished by exactly one kernel
    assert cc["vote"] == 2 * (vc["groups"] - skipped) - vc["handed_on_sides"]
    return got, want, facts, vc, cc, skipped, batches


@pytest.mark.gpu
@pytest.mark.parametrize("case", sc.CASES)
def test_engine_matches_oracle(case):
    got, want, facts, vc, cc, skipped, batches = run_engine(case)
    if case == "a":
        assert len(got.emitted()) == 0
        assert got.pre.as_dict() == want.pre.as_dict() and got.post.as_dict() == want.post.as_dict()
        assert got.pre.as_dict()["supporting_hist"][1] == 40
    if case == "b":      # 69 live groups of weight 6 = 414 of 96 to a batch: five batches, each over the group ids of a skipped run
        assert vc["groups"] - skipped == facts["live"]
        assert batches == facts["live"] * 6 // 96 + 1 and batches >= 2, batches
    if case == "c_pair":
        assert got.post.as_dict()["dcs"] == 1 and len(got.emitted()) == 2
    if case == "e":
        assert got.pre.as_dict() == want.pre.as_dict()
    if case == "g":
        assert skipped == 0 and sum(cc.values()) == 2 * vc["groups"]
