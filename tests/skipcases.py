"""Hand-built streams around the groups the engine does not evaluate (d_group_skipped, gce_groups.hpp) -- CPU only, no engine.

A one-pair group that no setting of the run can write (--supporting_reads > 1 or --duplex_only, no duplex partner possible) is left out of k_vote's
batches; its Stats entry is written from the pair slot.  Every stream here is a few dozen to a few hundred reads of 30 bases: clusters lie one behind
the other on one contig, a cluster is a list of groups (UMI or none, pairs, which pairs lack their mate), every read is cut from the contig, and pair 0
of a group of several pairs carries one planted minor base so that its consensus has something to vote on.

build(case) -> (ReadBatch, params, reference, facts): facts["skipped"] is the number of groups the rule names, facts["groups"] the number of groups,
facts["live_runs"] (case b) the layout, and what else the case's trap needs.
"""
import numpy as np

L = 30                 # read length
GAP = 10               # between the mates
STEP = 2 * L + GAP + 7  # from one cluster's left end to the next one's

CASES = ("a", "b", "c_pair", "c_third", "c_alone", "d", "e", "f", "g")


def _alt(ch):
    return "ACGT"[("ACGT".index(ch) + 1) % 4]


class Cluster:
    """groups: [(umi or None, pairs, mateless)] -- mateless: indices of the group's pairs whose right read is absent from the stream;
    low: the cluster's reads are homopolymers (Group::consensusMergeBam's low-complexity test, group.cpp:142-175); strand2: group indices
    whose pairs are the other strand (flags 163 / 83)."""

    def __init__(self, groups, low=False, strand2=()):
        self.groups, self.low, self.strand2 = groups, low, tuple(strand2)


def single(mateless=False, umi=None, low=False):
    return Cluster([(umi, 1, (0,) if mateless else ())], low=low)


def plain(pairs):
    return Cluster([(None, pairs, ())])


def _layout(case):
    """(clusters, parameter overrides, facts)"""
    if case == "a":      # 40 singleton clusters, every third one mate-less
        cl = [single(mateless=(k % 3 == 1)) for k in range(40)]
        return cl, dict(cluster_size_req=2), dict(skipped=40, mateless=sum(1 for k in range(40) if k % 3 == 1))
    if case == "b":      # runs of one-pair groups between two-pair groups (weight VB_MINW = 6 each: 16 to a batch of VB_W = 96)
        runs = [("live", 16), ("skip", 1), ("live", 16), ("skip", 15), ("live", 8), ("skip", 16), ("live", 8), ("skip", 17), ("live", 16), ("skip", 40),
                ("live", 5)]
        cl = []
        for kind, n in runs:
            cl += [plain(2) if kind == "live" else single(mateless=(len(cl) % 4 == 0)) for _ in range(n)]
        return cl, dict(cluster_size_req=2), dict(skipped=sum(n for k, n in runs if k == "skip"), live=sum(n for k, n in runs if k == "live"), live_runs=runs)
    if case == "c_pair":   # the two strands of one molecule, one pair each: a DCS of 1 + 1 = 2 supporting reads
        return [Cluster([("AAAA_CCCC", 1, ()), ("CCCC_AAAA", 1, ())], strand2=(1,))], dict(cluster_size_req=2), dict(skipped=0, dcs=1)
    if case == "c_third":  # ... plus a one-pair group whose UMI has one token: it finds no partner, but its cluster forms duplexes -- the full path, an equal result
        return ([Cluster([("AAAA_CCCC", 1, ()), ("CCCC_AAAA", 1, ()), ("GGGGTGGGG", 1, ())], strand2=(1,))], dict(cluster_size_req=2),
                dict(skipped=0, dcs=1))
    if case == "c_alone":  # a UMI cluster with a single one-pair group: no duplex without a second group
        return [single(umi="AAAA_CCCC"), single(umi="GGGGTGGGG", mateless=True)], dict(cluster_size_req=2), dict(skipped=2, dcs=0)
    if case == "d":      # --duplex_only without UMIs: nothing can be written, groups of three pairs still take the full path
        cl = [single(), plain(3), single(mateless=True), plain(3), single()]
        return cl, dict(duplex_only=1), dict(skipped=3)
    if case == "e":      # threshold 0: consensusMergeBam may return NULL for ONE pair (both sides here: the molecule counts as SE) -- nothing is skipped
        cl = [single(), single(low=True), plain(2), single(low=True), single(), single(low=True)]
        return cl, dict(cluster_size_req=2, skip_low_complexity_cluster_threshold=0), dict(skipped=0, low=3)
    if case == "f":      # -s 3: groups of two pairs cannot be written either, but their PE flag needs the template choice
        cl = [single(), plain(2), plain(3), single(mateless=True), plain(2), plain(3)]
        return cl, dict(cluster_size_req=3), dict(skipped=2)
    if case == "g":      # -s 1: everything can be written
        cl = [single(), plain(2), single(mateless=True), plain(3), single(umi="AAAA_CCCC")]
        return cl, dict(cluster_size_req=1), dict(skipped=0)
    raise ValueError(case)


def build(case, seed=5):
    from gencore_amd.batch import ReadBatch
    from gencore_amd.capi import default_params
    from lencases import pack_reference
    clusters, over, facts = _layout(case)
    rng = np.random.default_rng(seed)
    n_ref = 50 + STEP * len(clusters) + 50
    contig = bytearray(bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_ref)]))
    recs, ngroups = [], 0
    for ci, cl in enumerate(clusters):
        p0, p1 = 50 + STEP * ci, 50 + STEP * ci + L + GAP
        if cl.low:                                   # a homopolymer stretch of the contig: fewer than half of a read's neighbours differ
            contig[p0:p1 + L] = b"A" * (p1 + L - p0)
        for gi, (umi, pairs, mateless) in enumerate(cl.groups):
            ngroups += 1
            f_left, f_right = (163, 83) if gi in cl.strand2 else (99, 147)
            for k in range(pairs):
                name = "c%03dg%dp%d" % (ci, gi, k) + (":" + umi if umi else "")
                ls, rs = contig[p0:p0 + L].decode(), contig[p1:p1 + L].decode()
                nml = nmr = 0
                if pairs > 1 and k == 0:             # the template's minor base: the other voters flip it
                    ls = ls[:7] + _alt(ls[7]) + ls[8:]; nml = 1
                    rs = rs[:L - 3] + _alt(rs[L - 3]) + rs[L - 2:]; nmr = 1
                isz = p1 + L - p0
                recs.append(dict(qname=name, flag=f_left, tid=0, pos=p0, cigar="%dM" % L, mtid=0, mpos=p1, isize=isz, seq=ls, qual=[37] * L, nm=nml))
                if k not in mateless:
                    recs.append(dict(qname=name, flag=f_right, tid=0, pos=p1, cigar="%dM" % L, mtid=0, mpos=p0, isize=-isz, seq=rs, qual=[37] * L, nm=nmr))
    order = sorted(range(len(recs)), key=lambda i: (recs[i]["pos"], i))
    batch = ReadBatch.from_records([recs[i] for i in order])
    tl = np.asarray([n_ref], np.uint32)
    prm = default_params(n_targets=1, target_len=tl.ctypes.data, umi_prefix="", flush_period=1 << 30, **over)
    prm._keep = tl
    ref = [(pack_reference(contig.decode()), n_ref)]
    facts = dict(facts, groups=ngroups, clusters=len(clusters))
    return batch, prm, ref, facts
