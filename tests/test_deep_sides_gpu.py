"""The deep tier of consensus -- side_prepare's class path, k_deep_prepare, k_vote_deep, k_score2 -- on the catalogue of tests/deepcases.py: engine against
oracle, exact equality (diff_results, check_output_order), the exact tuple of Engine.consensus_counters() per case, and the status of the error cases.  Then the
combined stream (every default-parameter case in one stream, flushed every 500 reads), and every such case back to back on ONE engine, largest, smallest,
second largest, ...: prep_next, deep_next, n_deep and the scratch arrays of one step meet the next.  An engine's parameters are fixed when it is created, so the
threshold cases run back to back on an engine per threshold value (64, 65, 69, 70); the two score-constant cases meet no other case.
Measured on the MI355X: the module's 146 tests take 9.2 s -- the combined stream 1.4 s, the largest back-to-back test 1.2 s, every single case below 0.5 s."""
import numpy as np
import pytest

import deepcases as dc
from parity_helpers import check_output_order, diff_results

NAMES = list(dc.CASES)


def counters_tuple(e):
    cc = e.consensus_counters()
    return tuple(cc[k] for k in dc.KERNELS)


def stage_reference(e, ref, n_targets):
    for tid in range(n_targets):
        nib, ln = ref[tid] if tid < len(ref) else (None, 0)
        if nib is None:
            assert e.lib.gce_set_reference(e._h, tid, None, 0) == 0
        else:
            e.set_reference(tid, nib, ln)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_alone(built, name):
    from gencore_amd.capi import GceError
    from gencore_amd.engine import Engine
    from oracle import oracle_py
    c = dc.CASES[name]
    b = dc.Built(c)
    c.premise(b)
    want = oracle_py.run(b.batch, b.prm, b.ref)
    assert want.status == c.error, want.message
    e = Engine(b.prm)
    try:
        if c.error:
            with pytest.raises(GceError) as ei:
                e.run(b.batch, b.ref)
            assert ei.value.status == c.error
            return
        got = e.run(b.batch, b.ref)
        cc = counters_tuple(e)
    finally:
        e.close()
    diffs = diff_results(b.batch, got, want) + check_output_order(b.batch, got.rows)
    assert not diffs, "\n".join(diffs)
    assert cc == c.routing, (cc, c.routing)


@pytest.mark.gpu
def test_combined_stream(built):
    from gencore_amd.engine import Engine
    from oracle import oracle_py
    st = dc.combined_stream()
    batch, prm, ref = st.build()
    want = oracle_py.run(batch, prm, ref)
    assert want.status == 0, want.message
    e = Engine(prm)
    try:
        got = e.run(batch, ref)
        cc = counters_tuple(e)
    finally:
        e.close()
    diffs = diff_results(batch, got, want) + check_output_order(batch, got.rows)
    assert not diffs, "\n".join(diffs)
    assert cc == dc.combined_routing(), (cc, dc.combined_routing())


def back_to_back_groups():
    """skip_low_complexity_cluster_threshold -> the error-free cases with that value and otherwise default parameters."""
    out = {}
    for c in dc.CASES.values():
        st = c.make()
        if not c.error and not st.prm:
            out.setdefault(st.skip, []).append(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("skip", sorted(back_to_back_groups()))
def test_back_to_back_on_one_engine(built, skip):
    """One engine with the parameters the cases of one threshold value share (five targets of the longest contig's length: the cluster key of a read with its
    mate on its own contig does not look at them), reset between the streams, each stream's contigs staged and the others removed."""
    from gencore_amd.capi import default_params
    from gencore_amd.engine import Engine
    from oracle import oracle_py
    builts = [dc.Built(c) for c in back_to_back_groups()[skip]]
    assert len(builts) >= 6
    builts.sort(key=lambda b: b.batch.n)
    order = []
    while builts:                                                           # largest, smallest, second largest, ...
        order.append(builts.pop())
        if builts:
            order.append(builts.pop(0))
    nt = max(len(b.ref) for b in order)
    tl = np.full(nt, max(ln for b in order for _, ln in b.ref), np.uint32)
    prm = default_params(n_targets=nt, target_len=tl.ctypes.data, umi_prefix="", flush_period=1 << 30, skip_low_complexity_cluster_threshold=skip)
    e = Engine(prm)
    bad = []
    try:
        for b in order:
            want = oracle_py.run(b.batch, prm, b.ref)
            assert want.status == 0, want.message
            e.reset()
            stage_reference(e, b.ref, nt)
            e.add_reads(b.batch)
            e.finish()
            got = e.output(b.batch)
            diffs = diff_results(b.batch, got, want) + check_output_order(b.batch, got.rows)
            cc = counters_tuple(e)
            if diffs or cc != b.case.routing:
                bad.append("%s: counters %s, expected %s\n%s" % (b.case.name, cc, b.case.routing, "\n".join(diffs[:5])))
    finally:
        e.close()
    assert not bad, "\n".join(bad)
