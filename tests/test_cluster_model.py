"""CPU side of the cluster-formation tests (tests/clustercases.py): every case builds, its premise -- the facts about the INPUT that put it into the
catalogue -- holds, the oracle returns the status the case names and hands as many clusters to clusterByUMI as the key-only restatement of the read
loop (clustercases.spec_formation) says, and the catalogue is frozen by a digest of every batch.  No GPU.

The oracle's own time over the whole catalogue is printed by test_oracle_on_the_catalogue (pytest -s): 73 streams, 1.22 M reads, about 2.8 s on one core of
the CPU host the suite runs on (slowest: many:blocks_301_ticks 0.51 s, eventblocks:130 0.50 s, many:blocks_301 0.42 s)."""
import hashlib
import time

import numpy as np
import pytest

import clustercases as cc
from gencore_amd import shard
from gencore_amd.batch import ReadBatch


def batch_digest(case):
    h = hashlib.sha256()
    for f in ReadBatch.FIELDS:
        a = getattr(case.batch, f)
        h.update(f.encode()); h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    h.update(repr((case.period, tuple(case.contig_len), sorted(case.over.items()), case.status, case.events)).encode())
    return h.hexdigest()[:16]


FROZEN = {
    "size:1": "51a9df1aefe371e7",
    "size:511": "4fef3191132be653",
    "size:512": "7496c0b2242ff426",
    "size:513": "e52eeed4090a3185",
    "size:1023": "a539109e8823e515",
    "size:1024": "b11f32010c7b114b",
    "size:1025": "5f32bbf321c7225a",
    "size:2047": "42c376614ede4afe",
    "size:2048": "5ebb2210982634d0",
    "size:2049": "593a061fb228c9c4",
    "fill:1024_keys": "d02f5e4287947bfe",
    "fill:one_cluster_1024": "20d4d0184650ee59",
    "fill:one_cluster_1023+1": "50e060349e1b5f73",
    "fill:2300_reads_three_blocks": "639815c0110017ce",
    "fill:empty_block": "f7416a0c218a7dde",
    "events:period_1": "b8619db9b5fc7ec5",
    "events:period_2": "0578db53816efdee",
    "events:period_3": "1e31e34440d72c38",
    "events:period_1023": "b833a14f923a94f4",
    "events:period_1024": "af67aada14dc0287",
    "events:period_1025": "72bf93eda5ad1152",
    "eventblocks:64": "e72b15e00070cf31",
    "eventblocks:65": "6ee0c85964aa9535",
    "eventblocks:66": "687351e8c1665f88",
    "eventblocks:67": "6d9276ad59115f02",
    "eventblocks:130": "d3b31faf50613120",
    "events:none": "1e6b7097d386369d",
    "events:k_period": "71bcd43b01f71cfc",
    "events:k_period-1": "befeb9ff1b50f61a",
    "events:k_period+1": "a7de4eff478a63c6",
    "odd:period_5": "73ef218287239a4b",
    "odd:period_50": "bbf3e7abbe1ddbd6",
    "nopack:negative_left_pending": "606ff6c4f4866d0b",
    "nopack:negative_left_pending_unmapped": "e42f66312d62412f",
    "nopack:negative_left_pending_trailing": "7f4eb403e0183612",
    "nopack:beyond_contig": "a5845338f49bb3df",
    "nopack:negative_left": "13bc98b76f417a3e",
    "nopack:tid_beyond_header": "0afdcab22d2412e2",
    "nopack:behind_contig_end": "1c66cc1562eeb5db",
    "nopack:no_contigs_events": "cca66e707424cdc9",
    "nopack:no_contigs_odd": "2d3cb586ef69267a",
    "delta1:overflow": "e5c4b48358f80bfe",
    "home:taken": "a8142a597e1a281c",
    "unmapped:tid<0@0": "4e382287d6d7e772",
    "unmapped:tid<0@1": "e04fced2695ca691",
    "unmapped:tid<0@511": "7cb1754974eb7e38",
    "unmapped:tid<0@512": "c666034ee5c7321a",
    "unmapped:tid<0@1023": "c81dcacd0a5b66d4",
    "unmapped:pos<0@0": "ac11ed8e9311c1e2",
    "unmapped:pos<0@1": "0da8cdcde8ea79ed",
    "unmapped:pos<0@511": "cb4d29c443ff70b9",
    "unmapped:pos<0@512": "4584a324c79a2155",
    "unmapped:pos<0@1023": "392630f1b5b15895",
    "unsorted:@512": "55a4e7201d915fe0",
    "unsorted:@1024": "7689aa9bde06a4b8",
    "unsorted:@3072": "8bece4339006be6e",
    "tick:period_7_offset_1_trailing_0": "aed1d65c99e3aafc",
    "tick:period_7_offset_1_trailing_1": "c0e4367165e564c0",
    "tick:period_7_offset_period-1_trailing_0": "9404f86dabb1d650",
    "tick:period_7_offset_period-1_trailing_1": "aa8fd75ac54f256f",
    "tick:period_7_offset_period_trailing_0": "5363032fc742836f",
    "tick:period_7_offset_period_trailing_1": "52dffc5c69cdc4c6",
    "tick:period_7_offset_3e9+5_trailing_0": "8a2b93bf79a672de",
    "tick:period_7_offset_3e9+5_trailing_1": "79afadc20097ab44",
    "tick:period_977_offset_1_trailing_0": "df969c4098dfbe2d",
    "tick:period_977_offset_1_trailing_1": "f97fd4d8d5ac8861",
    "tick:period_977_offset_period-1_trailing_0": "05ba80201c58c908",
    "tick:period_977_offset_period-1_trailing_1": "6115e2624666120e",
    "tick:period_977_offset_period_trailing_0": "fe1ba9338115adfd",
    "tick:period_977_offset_period_trailing_1": "d142128a212f3632",
    "tick:period_977_offset_3e9+5_trailing_0": "b78927b3f6e154c1",
    "tick:period_977_offset_3e9+5_trailing_1": "86e475df9ff409b4",
    "many:blocks_301": "a2aad91aab41c419",
    "many:blocks_301_ticks": "68d3e3a70a0169bf",
}


def test_catalogue_holds_every_family():
    assert set(FROZEN) == set(cc.CASES)
    for fam in cc.FAMILIES:
        assert cc.family(fam), fam
    assert [n for n in cc.CASES if n.split(":")[0] not in cc.FAMILIES] == []
    assert len(cc.family("size")) == 10 and len(cc.family("unmapped")) == 10 and len(cc.family("tick")) == 16 and len(cc.family("unsorted")) == 3


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_case_builds_and_its_premise_holds(name):
    case = cc.get(name)
    assert case.batch.n > 0 and case.premise
    bad = [k for k, v in case.premise.items() if not v]
    assert not bad, "%s: premise does not hold: %s" % (name, bad)
    assert (case.batch.core["l_qseq"] == cc.READ_LEN).all()
    assert batch_digest(case) == FROZEN[name], "%s drifted: %s" % (name, batch_digest(case))


RULE_CASES = ("size:2049", "fill:1024_keys", "fill:one_cluster_1024", "fill:2300_reads_three_blocks", "events:period_1025", "eventblocks:66", "odd:period_50",
              "nopack:negative_left", "nopack:negative_left_pending", "nopack:beyond_contig", "nopack:tid_beyond_header", "delta1:overflow", "home:taken",
              "unmapped:pos<0@511", "tick:period_7_offset_1_trailing_0", "many:blocks_301")


@pytest.mark.parametrize("name", RULE_CASES)
def test_every_cluster_that_matters_has_two_pairs_one_base_apart(name):
    """The catalogue's rule, on at least one case of every family that forms clusters: every key with four or more reads holds two names whose UMIs
    differ in the last base only (what makes the flush's threshold visible in the table), a name has at most three reads, and two clusters that are
    neighbours in key order carry different bases (a wrong merge changes the consensus)."""
    case = cc.get(name)
    b = case.batch
    cm, left, right = cc.keys_of(b.core, case.contig_len)
    idx = np.nonzero(cm)[0]
    nm = b.qname.reshape(b.n, 22)[idx]
    assert (nm[:, 12] == ord(":")).all() and (nm[:, 21] == 0).all()
    keys = np.stack([b.core["tid"][idx].astype(np.int64), left[idx], right[idx]], axis=1)
    uk, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    # the reads of a key with one UMI stem (7 bases) are one group of pairs put there together (an odd group may share its key with an ordinary cluster)
    gk, ginv, gcnt = np.unique(np.concatenate([inv[:, None], nm[:, 13:20].astype(np.int64)], axis=1), axis=0, return_inverse=True, return_counts=True)
    ginv = ginv.reshape(-1)
    big = gcnt >= 4
    assert big.sum() >= min(100, len(uk) // 2)
    last = np.unique(np.stack([ginv, nm[:, 20].astype(np.int64)], axis=1), axis=0)
    n_last = np.bincount(last[:, 0], minlength=len(gk))
    assert (n_last[big] >= 2).all(), "four or more reads with one UMI: blind to the threshold"
    names = np.unique(np.concatenate([inv[:, None], nm[:, :21].astype(np.int64)], axis=1), axis=0, return_counts=True)[1]
    assert names.max() <= 3
    # bases: one sequence per group, and the groups that are neighbours in key order differ
    seq = b.seq.reshape(b.n, cc.READ_LEN // 2)[idx]
    gs = np.unique(np.concatenate([ginv[:, None], seq.astype(np.int64)], axis=1), axis=0)
    assert len(gs) == len(gk), "a group holds two base sequences"
    assert (gs[1:, 1:] != gs[:-1, 1:]).any(axis=1).all(), "two neighbouring clusters carry the same bases"

def test_spec_formation_on_hand_made_streams():
    """The key-only restatement against streams whose answer is plain: no event -> one cluster per key; period 1 on one key -> every read opens a
    cluster only if the walk took the one before, and a walk on the key's own reads never takes it (left < pos fails)."""
    b = cc.build(cc.dense(40, 0, 100))
    f = cc.spec_formation(b.core, 1000, cc.STD_CONTIGS)
    assert (f["n_taken"], f["n_pending"], f["n_events"], f["split"]) == (10, 0, 0, 0)
    one = cc.build(cc.pairs(0, np.arange(2), 0, 100, 30, 110))
    f = cc.spec_formation(one.core, 1, cc.STD_CONTIGS)
    assert (f["n_taken"], f["n_events"], f["split"]) == (1, 4, 0)
    # a key whose both ends lie far in front of its reads: the walk between its two groups of reads takes it, the second group opens it again
    grp = lambda pos: cc.reads(tid=0, pos=pos, mtid=0, mpos=400, isize=-30, flag=np.asarray([99, 99, 147, 147]), cid=1, k=np.asarray([0, 1, 0, 1]))
    g = cc.build([grp(1000), cc.dense(8, 5, 1005), grp(1020)])
    f = cc.spec_formation(g.core, 6, cc.STD_CONTIGS)
    assert (f["n_taken"], f["n_events"], f["split"]) == (4, 2, 1)
    # an unmapped read in the middle: what is opened behind it and never walked over stays pending
    u = cc.build(cc.dense(40, 0, 100), inserts=[(20, cc.unmapped_read("tid<0"))])
    f = cc.spec_formation(u.core, 1000, cc.STD_CONTIGS)
    assert f["first_unmapped"] == 20 and f["n_taken"] + f["n_pending"] > 10 and f["n_pending"] >= 5


def test_event_places_agree_with_stream_context():
    b = cc.events_stream()
    for period in cc.EVENT_PERIODS:
        tick, et, ep = shard.stream_context(b.core, period)
        ev = cc.event_reads(b.core, period)
        assert np.array_equal(b.core["pos"][ev], ep) and len(ev) == len(et)
    got = {p: tuple(k for k in ("first", "last", "behind_empty", "partial") if cc.event_places(b.core, p)[k]) for p in cc.EVENT_PERIODS}
    assert got == cc.EVENT_PERIODS
    for place in ("first", "last", "behind_empty", "partial"):                      # every place is hit at one of the large periods too
        assert any(place in cc.EVENT_PERIODS[p] for p in (1023, 1024, 1025))


def run_oracle(oracle, case):
    prm = case.params()
    if case.events:
        b, ev = case.with_ticks()
        return oracle.run(b, prm, None, events=ev)
    return oracle.run(case.batch, prm)


def test_oracle_on_the_catalogue(oracle):
    """The status every case names, as many clusters as the spec says, and the oracle's time over the whole catalogue."""
    total, reads, slow = 0.0, 0, []
    for name in cc.CASES:
        case = cc.get(name)
        t0 = time.perf_counter()
        want = run_oracle(oracle, case)
        dt = time.perf_counter() - t0
        total += dt; reads += case.batch.n
        slow.append((dt, name))
        assert want.status == case.status, (name, want.status, want.message)
        if case.status == 0:
            assert want.n_clusters == case.facts["n_taken"], (name, want.n_clusters, case.facts)
            assert len(want.emitted()) > 0
    slow.sort(reverse=True)
    print("\noracle over the cluster catalogue: %d streams, %d reads, %.2f s; slowest: %s" % (
        len(cc.CASES), reads, total, ", ".join("%s %.2f s" % (n, t) for t, n in slow[:4])))


def test_tick_interface_gives_the_same_table(oracle):
    """The many-blocks stream through batch.tick + the event list (ticks and events from shard.stream_context, the spec) is the same table as the plain run."""
    a, b = run_oracle(oracle, cc.get("many:blocks_301")), run_oracle(oracle, cc.get("many:blocks_301_ticks"))
    for f in ("out_flag", "mate", "fr", "rr", "qname_src"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_thresholds_show_in_the_table(oracle):
    """The catalogue's point: the same stream with the periodic threshold at 0 emits more records (the pairs one base apart stay apart)."""
    case = cc.get("size:2049")
    prm = case.params()
    one = oracle.run(case.batch, prm)
    prm.proper_umi_diff_threshold = 0
    zero = oracle.run(case.batch, prm)
    assert len(zero.emitted()) > len(one.emitted()) + 500


def test_left_below_zero_pairs_are_written_as_they_are(oracle):
    """gencore.cpp:401-407: a cluster with left < 0 that finishConsensus meets goes to outputPair pair by pair, without clusterByUMI -- every name's first
    and last read written, no tag, the two pairs one base apart not merged -- at the end of the file and in front of an unmapped read; behind the unmapped
    read it is never processed, and under a trailing flush (a later slice's periodic walk, :355) it is clustered like any other."""
    for name, emitted, tagged in (("nopack:negative_left_pending", 4 + 4 + 4 + 3 + 4, False), ("nopack:negative_left_pending_unmapped", 4 + 4 + 4 + 3, False),
                                  ("nopack:negative_left_pending_trailing", None, True)):
        case = cc.get(name)
        b = case.batch
        want = run_oracle(oracle, case)
        assert want.status == 0
        cm, left, right = cc.keys_of(b.core, case.contig_len)
        neg = np.nonzero(cm & (left < 0))[0]
        out = neg[want.out_flag[neg] != 0]
        if tagged:
            assert (want.fr[out] >= 1).all() and len(out) < 19            # merged by the periodic threshold 1
            continue
        assert len(out) == emitted and (want.fr[out] == -1).all() and (want.rr[out] == -1).all() and (want.nm_new[out] == -1).all()
        assert np.array_equal(want.qname_src[out], out)
        third = [i for i in neg if b.qname_of(int(i)).startswith("610000040000")]   # the name with three reads: first and last written, mates of each other
        first_unm = case.facts["first_unmapped"]
        if first_unm < 0:
            assert want.out_flag[third].tolist() == [1, 0, 1] and int(want.mate[third[0]]) == int(third[2]) and int(want.mate[third[2]]) == int(third[0])
        else:
            assert (want.out_flag[neg[neg > first_unm]] == 0).all()
