"""The output table (gce_output.hpp and its launch logic in engine.hip) on the streams of tests/outcases.py, engine against oracle.  Per case: every record of
the table (diff_results), the output order, the raw rows of Engine.rows() -- src, kind, qname_src, nm_new, fr, rr, mate -- equal to the model table
(outcases.rows_from_table of the oracle's result) element by element, and the header's contract for the blobs (outcases.check_blobs: aligned, disjoint, inside,
totals = the sums of the units; the layout itself is the engine's business).  Then the cases of groups 1-7 back to back on one engine, in an order that goes down
and up in size at every step: rank64, part3 and the flag bytes beyond n are left over from the step before.

Measured on the MI355X: the module's 64 tests take 5.3 s in all, oracle runs included.  The large case (4 198 405 reads, 3 816 733 records) takes 2.1 s: 0.31 s for
the engine (create, submit, step, drain, per-read table), of which the GPU step is 4.4 ms and its output kernels 0.7 ms, and 1.35 s for the checks; the 62 streams
back to back 0.9 s, the 67-tile stream 0.33 s, every other case below 0.1 s.  The large case prints its times (pytest -s); nothing is asserted on them."""
import time

import numpy as np
import pytest

import outcases as oc
from parity_helpers import check_output_order, diff_results

pytestmark = pytest.mark.gpu

RAW_FIELDS = ("src", "kind", "qname_src", "nm_new", "fr", "rr", "mate")


def check_table(tag, batch, got, want):
    """The engine's ResultTable `got` (with its raw rows) against the oracle's `want`."""
    diffs = diff_results(batch, got, want) + check_output_order(batch, got.rows)
    assert not diffs, tag + ":\n" + "\n".join(diffs)
    model = oc.rows_from_table(batch, want)
    for f in RAW_FIELDS:
        g, m = got.rows[f], model[f]
        assert g.shape == m.shape and g.dtype == m.dtype, (tag, f, g.shape, m.shape, g.dtype, m.dtype)
        bad = np.nonzero(g != m)[0]
        assert not len(bad), "%s: rows[%s] differs from the model table at %d rows, first %s: %s vs %s" % (tag, f, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), m[bad[:5]].tolist())
    bad = oc.check_blobs(batch, got.rows)
    assert not bad, tag + ":\n" + "\n".join(bad)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_case(built, name):
    """Per case one fresh engine."""
    from gencore_amd.engine import Engine
    case = oc.get(name)
    want = oc.oracle_result(name)
    assert want.status == 0, (want.status, want.message)
    prem = case.premise(want)
    assert prem and all(prem.values()), [k for k, v in prem.items() if not v]
    large = case.batch.n > 1000000
    t0 = time.perf_counter()
    e = Engine(case.params())
    try:
        got = e.run(case.batch, case.reference())
        t1 = time.perf_counter()
        step_ms = e.timing()["total_ms"] if large else 0.0
        out_ms = e.timing()["output_ms"] if large else 0.0
    finally:
        e.close()
    check_table(name, case.batch, got, want)
    if large:
        print("\n%s: %d reads, %d records: engine (create, submit, step, drain, per-read table) %.2f s of which GPU step %.1f ms (output kernels %.1f ms); "
              "checks %.2f s" % (name, case.batch.n, len(got.rows["src"]), t1 - t0, step_ms, out_ms, time.perf_counter() - t1))


def test_streams_back_to_back_on_one_engine(built):
    """Groups 1-7 on ONE engine with the catalogue's standard parameters (cluster_size_req 1, no reference: the oracle runs every stream with the engine's own
    parameters, so the lone pair of lq:filtered_cluster_other_length is emitted here and stats:nm_patched patches nothing).  The order
    (outcases.back_to_back_order) goes from the largest stream to the smallest and back at every step and changes between the uniform and the non-uniform
    k_out_meta a dozen times: what a step leaves in rank64, part3 and the flag bytes beyond its n meets a shorter, a longer, another kind of stream."""
    from gencore_amd.engine import Engine
    from oracle import oracle_py
    prm = oc.get("size:1").params()
    e = Engine(prm)
    try:
        for k, name in enumerate(oc.back_to_back_order()):
            case = oc.get(name)
            want = oc.oracle_result(name) if (case.size_req == 1 and case.contigs is None) else oracle_py.run(case.batch, prm)
            assert want.status == 0
            got = e.run(case.batch)
            check_table("step %d (%s)" % (k, name), case.batch, got, want)
    finally:
        e.close()
