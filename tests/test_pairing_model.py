"""CPU side of the mate-pairing tier tests: the h32 collision pairs, the cluster stream builder and its routing spec, and the oracle on the
deep kernel's window case (tests/paircases.py).  No GPU."""
import collections

import numpy as np

import paircases as pc


def test_collision_pairs_collide_and_differ():
    pairs = pc.collision_pairs()
    assert len(pairs) == 4 and len({x for p in pairs for x in p}) == 8
    for a, b in pairs:
        assert a != b and len(a) == len(b)
        nw0 = (len(a) + 7) // 8
        for nw in range(nw0, 9):                      # any wave-wide word count that covers the names
            assert pc.h32(pc.name_words(a), nw) == pc.h32(pc.name_words(b), nw)
        assert pc.hash_false_match([a, b, a, b])


def test_h32_vectorised_matches_scalar():
    rng = np.random.default_rng(5)
    names = [bytes(rng.integers(33, 127, int(rng.integers(1, 65))).astype(np.uint8)) for _ in range(200)]
    raw = np.asarray([pc.name_words(x) for x in names], np.uint64)
    for nw in (1, 3, 8):
        sub = [x for x in names if len(x) <= 8 * nw]
        got = pc.h32_np(np.asarray([pc.name_words(x) for x in sub], np.uint64).reshape(len(sub), 8), nw)
        assert got.tolist() == [pc.h32(pc.name_words(x), nw) for x in sub]
    assert raw.shape == (200, 8)
    # the constants of gce_pair2.hpp: one known value
    assert pc.h32(pc.name_words(b"SIM:1:2:3"), 2) == pc.h32(pc.name_words(b"SIM:1:2:3"), 2) != pc.h32(pc.name_words(b"SIM:1:2:4"), 2)


def test_expected_tier_routing_table():
    for n, tier in pc.TIER_OF_SIZE.items():
        assert pc.expected_tier(pc.sized_cluster(n, b"t")) == tier, n
    assert pc.expected_tier(pc.sized_cluster(pc.PD_BIGMAX - 2, b"t")) == "deep_device"
    assert pc.expected_tier(pc.sized_cluster(pc.PD_BIGMAX - 1, b"t")) == "generic"
    for n in (16, 32, 64):
        assert pc.expected_tier(pc.sized_cluster(n, b"t", name_len=64)) != "generic"
        assert pc.expected_tier(pc.sized_cluster(n, b"t", name_len=65)) == "generic"
    assert pc.expected_tier(pc.sized_cluster(100, b"t", name_len=254)) == "deep_lds"
    # a run of 33 reads with different names behind one window goes to the generic kernels, 32 stay
    for run, tier in ((32, "deep_lds"), (34, "generic")):
        sp = pc.window_names(b"r", 16, longer=run // 2)[1:]
        assert pc.expected_tier(pc.filled_cluster(100, b"r", sp, 0)) == tier
    # 32 reads of ONE name behind a window: no rest, no hand-on
    assert pc.expected_tier(pc.Cluster(fwd=[b"r:one"] * 40 + [b"r:x%d" % i for i in range(40)])) == "deep_lds"


def test_builder_clusters_have_their_sizes_and_keys():
    st = pc.Stream(seed=3)
    cls = pc.core_clusters() + pc.collision_clusters()
    for cl in cls:
        st.add(cl)
    st.pad_singletons(50)
    contig = st.contig()
    recs = st.records(contig)
    assert [r["pos"] for r in recs] == sorted(r["pos"] for r in recs)
    keys = collections.defaultdict(list)
    for i, r in enumerate(recs):
        left = r["mpos"] if r["isize"] < 0 else r["pos"]
        keys[(r["tid"], left, abs(r["isize"]))].append(i)
        assert r["seq"] == contig[r["pos"]:r["pos"] + pc.READ_LEN]
    assert len(keys) == len(st.clusters)
    by_cl = collections.defaultdict(list)
    for i, r in enumerate(recs):
        by_cl[r["_cl"]].append(i)
    for ci, cl in enumerate(st.clusters):
        idx = by_cl[ci]
        left = {recs[i]["mpos"] if recs[i]["isize"] < 0 else recs[i]["pos"] for i in idx}
        assert left == {cl.left} and len(idx) == cl.n and idx[0] == cl.first
        assert [recs[i]["qname"].encode() for i in idx] == cl.reads()          # arrival order as given
    sizes = collections.Counter(cl.n for cl in cls)
    for n in pc.REGISTER_SIZES + pc.DEEP_SIZES:
        assert sizes[n] >= 1
    assert st.mode() == "classes"
    st.pad_singletons(20000, tag=b"more")
    assert st.mode() == "chain"


def test_window_names_tie_on_the_deep_window():
    names = pc.window_names(b"dw", 16, longer=2) + [b"dw:f%d" % i for i in range(40)]
    cp, wr = pc._deep_windows(names)
    assert cp == 3
    assert wr[0][0] == wr[1][0] == wr[2][0] and wr[0][1] == 0 and wr[1][1] == 1
    names = pc.window_names(b"dw", 15, longer=1) + [b"dw:f"]
    _, wr = pc._deep_windows(names)
    assert wr[0][0] != wr[1][0]


def _oracle_pairs(cl):
    """Run the oracle over one cluster whose names carry far-apart MI:Z UMIs: every pair is a group of its own, so the molecules it
    reports are its pairs (paired-end: both mates found; single-end: one read)."""
    from oracle import oracle_py
    rng = np.random.default_rng(11)
    names = sorted(set(cl.reads()))
    cl.mi = {nm: b"u:" + bytes(rng.choice(list(b"ACGT"), 12).astype(np.uint8)) for nm in names}
    st = pc.Stream()
    st.add(cl)
    batch, prm, ref, _ = st.build()
    prm.proper_umi_diff_threshold = 0
    res = oracle_py.run(batch, prm, ref)
    assert res.status == 0, res.message
    return res.post.molecules, res.post.molecules_pe


def test_oracle_pairs_the_deep_window_case(oracle):
    """A name that ends exactly at the window's end and a longer one that starts with it, the short name's first read first: two pairs."""
    for end in (15, 16, 17):
        for short_first in (True, False):
            sp = pc.window_names(b"dw", end, longer=1)
            cl = pc.filled_cluster(136, b"dw", sp, 0, shuffle=False)
            if not short_first:
                cl.fwd = [x for x in cl.fwd if x != sp[0]] + [sp[0]]
                cl.rev = [x for x in cl.rev if x != sp[0]] + [sp[0]]
            assert pc.expected_tier(cl) == "deep_lds"
            assert _oracle_pairs(cl) == (68, 68)
