"""The catalogue of tests/deepcases.py on the CPU: every premise holds, every planted decision is decisive in the oracle (a case and its neighbour differ),
side_spec agrees with what the oracle emits (template read, SE / PE, the bytes at the witness columns), the routing a case states is the one side_spec and the
kernels' scope rules give, and the catalogue is frozen by digests.  The whole module builds each case once (about 35 s, most of it side_spec and the premises over
the 1025-pair groups)."""
import hashlib

import numpy as np
import pytest

import deepcases as dc

NAMES = list(dc.CASES)
FAMILY_SIZES = {"V": 39, "C": 42, "T": 34, "A": 6, "X": 10, "O": 9}
# sha256 over core, cigar, seq, qual, nm, nm_type of every case's batch, in catalogue order, and over the combined stream: a change of any case shows here
DIGEST_ALL = "282f4f1f4f39f8afea55e3e96ff4c7905b9bd0874771b492a7081b6a5c79a0f3"
DIGEST_COMBINED = "155297bc287f3389a2b286efed7de0ad0275dec47d00f9c5a9693e6254b4964a"


# cases whose output qualities or NM depend on which reference bases happen to repeat (two right ends two bases apart; right reads of many lengths on one end)
BASES_DECIDE_QUALITIES = ("C.right_end", "O.windows.np70")


def batch_digest(h, batch):
    for f in ("core", "cigar", "seq", "qual", "nm", "nm_type"):
        h.update(getattr(batch, f).tobytes())


@pytest.fixture(scope="module")
def built_cases(oracle):
    """name -> (Built, the oracle's result): built and run once for the whole module; the results are not modified."""
    out = {}
    for name, c in dc.CASES.items():
        b = dc.Built(c)
        out[name] = (b, oracle.run(b.batch, b.prm, b.ref))
    return out


def test_the_catalogue_holds_every_family():
    fam = {}
    for c in dc.CASES.values():
        fam[c.family] = fam.get(c.family, 0) + 1
    assert fam == FAMILY_SIZES, fam
    for c in dc.CASES.values():
        assert c.neighbour is None or c.neighbour in dc.CASES, c.name
        assert len(c.routing) == 5 and all(v >= 0 for v in c.routing)


@pytest.mark.parametrize("name", NAMES)
def test_premise_oracle_and_routing(built_cases, name):
    """The premise holds (a failure is an error of the catalogue); the oracle's status is the case's; the witness columns, the template read and SE / PE are
    what the case states; no group is larger than the catalogue allows; the stated counter tuple is the model's."""
    c = dc.CASES[name]
    b, want = built_cases[name]
    c.premise(b)
    assert want.status == c.error, (want.status, want.message)
    assert max(len(g.left) for g in b.st.groups) <= 1100
    if c.witness:
        c.witness(b, want)
    assert b.model_routing() == c.routing and sum(c.routing) == 2 * len(b.st.groups)
    if c.error:
        return
    for gi, g in enumerate(b.st.groups):                                  # side_spec against the oracle's observable outcome
        for side in (0, 1):
            sp = b.spec(gi, side)
            emitted = [k for k, r in enumerate(b.st.reads_of(gi, side)) if r is not None and want.out_flag[r] != 0]
            if len(g.left) > 64:
                assert emitted == ([] if sp["template"] is None else [sp["template"]]), (gi, side, emitted, sp["template"], sp["reason"])
            else:
                assert len(emitted) == 1


@pytest.mark.parametrize("name", [n for n in NAMES if dc.CASES[n].neighbour])
def test_the_planted_decision_is_decisive(built_cases, name):
    a, o = built_cases[name][1], built_cases[dc.CASES[name].neighbour][1]
    same = a.status == o.status and all(np.array_equal(getattr(a, f), getattr(o, f)) for f in ("seq", "qual", "out_flag", "nm_new"))
    assert not same, (name, dc.CASES[name].neighbour)


def test_the_catalogue_is_frozen(built_cases):
    h = hashlib.sha256()
    for name in NAMES:
        batch_digest(h, built_cases[name][0].batch)
    assert h.hexdigest() == DIGEST_ALL
    again = dc.Built(dc.CASES["O.windows.np70"])                          # (and deterministic)
    assert again.batch.seq.tobytes() == built_cases["O.windows.np70"][0].batch.seq.tobytes()


def test_the_combined_stream(oracle, built_cases):
    """Every case with default parameters and no error in one stream, flushed every 500 reads: the oracle accepts it, and every read of every group comes out as
    it does in the case alone -- emitted or not, and but for the cases named above NM and qualities (the bases are cut from another random contig; the routing of the combined stream is the sum of
    the cases')."""
    st = dc.combined_stream()
    batch, prm, ref = st.build()
    h = hashlib.sha256()
    batch_digest(h, batch)
    assert h.hexdigest() == DIGEST_COMBINED
    want = oracle.run(batch, prm, ref)
    assert want.status == 0, want.message
    assert want.n_groups == len(st.groups) == sum(len(c.make().items) for c in dc.CASES.values() if c.combine and not c.error)
    assert prm.flush_period == 500 and batch.n > 20 * 500
    assert sum(dc.combined_routing()) == 2 * len(st.groups)

    gi, differ = 0, set()
    for c in dc.CASES.values():
        if not (c.combine and not c.error):
            continue
        one, alone = built_cases[c.name]
        for lg, g in enumerate(one.st.groups):
            for (g1, side, k), r1 in one.st.where.items():
                if g1 != lg:
                    continue
                r2 = st.where[(gi, side, k)]
                assert want.out_flag[r2] == alone.out_flag[r1], (c.name, lg, side, k)
                n = int(batch.core["l_qseq"][r2])
                q1, q2 = int(one.batch.qual_off[r1]), int(batch.qual_off[r2])
                if want.nm_new[r2] != alone.nm_new[r1] or want.qual[q2:q2 + n].tobytes() != alone.qual[q1:q1 + n].tobytes():
                    differ.add(c.name)
            gi += 1
    assert gi == len(st.groups)
    assert differ <= set(BASES_DECIDE_QUALITIES), sorted(differ)
