"""Hand-built streams around the finish stage: the duplex pass that runs only when some UMI of the stream holds a '_' (k_describe's StreamInfo::umi_us),
and the Stats events k_group_tail counts for the groups that are final there -- CPU only, no engine.

The streams are built the way tests/skipcases.py builds them: clusters lie one behind the other on one contig, a cluster is a list of groups (UMI or
none, pairs, which pairs lack their mate), reads are 30 bases cut from the contig, and pair 0 of a group of several pairs carries one planted minor base.
What is new here: how the UMI gets into the record (`name` / `mi` of a Cluster), and streams whose group indices are placed on purpose.

build(clusters, **overrides) -> (ReadBatch, params, reference)
"""
import numpy as np

from skipcases import GAP, L, STEP, _alt

U3 = ("AAAAAAAA", "CCCCCCCC", "GGGGGGGG")          # three UMIs without '_', far apart: three groups


class Cluster:
    """groups: [(umi or None, pairs, mateless)]; strand2: group indices on the other strand (flags 163 / 83).
    name(stem, umi) -> read name (default: stem + ':' + umi); mi(umi) -> the MI:Z tag's text or None."""

    def __init__(self, groups, strand2=(), name=None, mi=None, gap=0):
        self.groups, self.strand2, self.name, self.mi, self.gap = groups, tuple(strand2), name, mi, gap


def default_name(stem, umi):
    return stem + (":" + umi if umi else "")


def build(clusters, umi_prefix="", seed=11, n_ref=None, **over):
    from gencore_amd.batch import ReadBatch
    from gencore_amd.capi import default_params
    from lencases import pack_reference
    rng = np.random.default_rng(seed)
    starts, at = [], 50
    for cl in clusters:
        at += cl.gap
        starts.append(at)
        at += STEP
    assert n_ref is None or n_ref >= at + 50
    n_ref = n_ref or at + 50                                  # (n_ref: two streams for one engine share the contig's length)
    contig = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_ref)])
    recs = []
    for ci, cl in enumerate(clusters):
        p0, p1 = starts[ci], starts[ci] + L + GAP
        for gi, (umi, pairs, mateless) in enumerate(cl.groups):
            f_left, f_right = (163, 83) if gi in cl.strand2 else (99, 147)
            for k in range(pairs):
                name = (cl.name or default_name)("c%03dg%dp%d" % (ci, gi, k), umi)
                mi = cl.mi(umi) if cl.mi else None
                ls, rs = contig[p0:p0 + L].decode(), contig[p1:p1 + L].decode()
                nml = nmr = 0
                if pairs > 1 and k == 0:
                    ls = ls[:7] + _alt(ls[7]) + ls[8:]; nml = 1
                    rs = rs[:L - 3] + _alt(rs[L - 3]) + rs[L - 2:]; nmr = 1
                isz = p1 + L - p0
                recs.append(dict(qname=name, flag=f_left, tid=0, pos=p0, cigar="%dM" % L, mtid=0, mpos=p1, isize=isz, seq=ls, qual=[37] * L, nm=nml, mi=mi))
                if k not in mateless:
                    recs.append(dict(qname=name, flag=f_right, tid=0, pos=p1, cigar="%dM" % L, mtid=0, mpos=p0, isize=-isz, seq=rs, qual=[37] * L, nm=nmr, mi=mi))
    order = sorted(range(len(recs)), key=lambda i: (recs[i]["pos"], i))
    batch = ReadBatch.from_records([recs[i] for i in order])
    tl = np.asarray([n_ref], np.uint32)
    prm = default_params(n_targets=1, target_len=tl.ctypes.data, umi_prefix=umi_prefix, flush_period=1 << 30, **over)
    prm._keep = tl
    return batch, prm, [(pack_reference(contig.decode()), n_ref)]


# ------------------------------------------------------------------------------------------------------------ 1. both paths on one stream
def stream_s(extra_duplex_umi=False):
    """Clusters of 1, 2 and 3 groups, groups of 1, 2 and 3 pairs, mate-less pairs; name UMIs without '_'.  With extra_duplex_umi one far-away
    single-pair cluster `AAAA_CCCC` follows: the only '_' of the stream, and no duplex anywhere."""
    a, c, g = U3
    cl = [Cluster([(a, 1, ())]), Cluster([(a, 1, (0,))]), Cluster([(c, 2, ())]), Cluster([(g, 3, (1,))]),
          Cluster([(a, 1, ()), (c, 1, ())]), Cluster([(a, 2, ()), (c, 1, (0,))]), Cluster([(a, 3, ()), (g, 2, (0, 1))], strand2=(1,)),
          Cluster([(a, 1, ()), (c, 2, ()), (g, 3, ())]), Cluster([(a, 1, (0,)), (c, 1, ()), (g, 1, ())], strand2=(2,)), Cluster([(a, 2, ()), (c, 2, ()), (g, 2, (1,))]),
          Cluster([(None, 2, ())]), Cluster([(None, 1, ())])]
    if extra_duplex_umi:
        cl.append(Cluster([("AAAA_CCCC", 1, ())], gap=5000))
    return cl


# ------------------------------------------------------------------------------------------------------------ 2. / 3. where the '_' is seen
X, Y = "AAAA", "CCCC"
X17, Y17 = "ACGTACGTACGTACGTA", "CATGCATGCATGCATGC"


def duplex_pair(x=X, y=Y, **kw):
    """one cluster, two one-pair groups x_y / y_x on opposite strands"""
    return [Cluster([(x + "_" + y, 1, ()), (y + "_" + x, 1, ())], strand2=(1,), **kw)]


def _name70(stem, umi):
    tail = ":" + umi
    return stem + "x" * (70 - len(stem) - len(tail)) + tail


DUPLEX_SEEN = {          # case -> (clusters, umi_prefix)
    "prefix": (duplex_pair(name=lambda stem, umi: stem + ":UMI_" + umi), "UMI"),
    "colon": (duplex_pair(), ""),
    "2x17_byte_walk": (duplex_pair(X17, Y17), ""),
    "name_of_70": (duplex_pair(name=_name70), ""),
    "mi_only": (duplex_pair(name=lambda stem, umi: stem, mi=lambda umi: "x:" + umi), ""),
}
NO_DUPLEX = {            # one leading '_' is skipped (one-token UMIs: no duplex); two '_' are no UMI at all
    "leading_underscore": [Cluster([("_" + X + Y, 1, ()), ("_" + Y + X, 1, ())], strand2=(1,))],
    "two_underscores": [Cluster([(X + "__" + Y, 1, ()), (Y + "__" + X, 1, ())], strand2=(1,))],
}


# ------------------------------------------------------------------------------------------------------------ 4. block and wave edges of the fold
EDGE_PATTERNS = ((1, 1, 1), (1, 2, 1), (2, 1, 2))       # pairs of a cluster's three groups: 0, 1 and 2 of them written at -s 2
EDGE_CLUSTERS = 88


def edges(shift, rot):
    """`shift` single-group clusters, then 88 UMI clusters of three groups: cluster k holds the group indices shift + 3k .. shift + 3k + 2 (a thread per
    group, 64 to a wave, 256 to a block).  shift 0: clusters 21 and 85 hold 63..65 and 255..257; shift 1: they START at 64 and 256 (the look at the
    group in front crosses the edge); shift 2: clusters 20 and 84 hold 62..64 and 254..256.  Cluster k takes EDGE_PATTERNS[(k + rot) % 3]: over the three
    rotations every edge cluster has 0, 1 and 2 written groups."""
    cl = [Cluster([("TTTTTTTT", 2, ())]) for _ in range(shift)]
    for k in range(EDGE_CLUSTERS):
        cl.append(Cluster([(u, n, ()) for u, n in zip(U3, EDGE_PATTERNS[(k + rot) % 3])]))
    return cl


# ------------------------------------------------------------------------------------------------------------ 5. the histogram's end
def hist_end(max_supporting_reads):
    return [Cluster([("AAAAAAAA", max_supporting_reads, ())]), Cluster([("CCCCCCCC", max_supporting_reads - 1, ())])]


# ------------------------------------------------------------------------------------------------------------ 6. mixed stream
def mixed():
    return [Cluster([(None, 2, ())]), Cluster([(None, 1, ())]),                                                  # plain, skipped at -s 2
            Cluster([("AAAA_CCCC", 1, ()), ("CCCC_AAAA", 1, ())], strand2=(1,)),                                  # matched
            Cluster([(None, 3, (1,))]),
            Cluster([("AAAA_CCCC", 2, ()), ("GGGG_TTTT", 1, ())], strand2=(1,)),                                  # unmatched
            Cluster([("GGGGTGGGG", 1, ())]),                                                                      # a UMI, one group: final at once
            Cluster([("AAAA_CCCC", 1, ()), ("CCCC_AAAA", 2, ()), ("GGGGTGGGG", 1, ())], strand2=(1,)),            # matched + a third one-token group
            Cluster([(None, 1, (0,))]), Cluster([("ACGTACGT", 2, ()), ("TGCATGCA", 3, ())]),                     # one-token UMIs in a stream that forms duplexes
            Cluster([("AAAA_CCCC", 2, ()), ("CCCC_AAAA", 2, ()), ("AAAA_GGGG", 2, ()), ("GGGG_AAAA", 1, (0,))], strand2=(1, 3))]


# ------------------------------------------------------------------------------------------------------------ 7. empty cases
def no_clustered_read():
    """every read has an unmapped mate: written as it is, no cluster"""
    from gencore_amd.batch import ReadBatch
    recs = [dict(qname="b%d" % k, flag=73, tid=0, pos=100 + 40 * k, cigar="30M", mtid=-1, mpos=-1, isize=0, seq="ACGT" * 7 + "AC", qual=[30] * L, nm=0) for k in range(5)]
    return ReadBatch.from_records(recs)


def clusters_without_group():
    """mate position -1 and isize < 0 on the read's own contig: clusters with left = -1 (gencore.cpp:300-304), which the end of the stream writes pair by
    pair without clusterByUMI (gencore.cpp:401-407): no group"""
    from gencore_amd.batch import ReadBatch
    recs = [dict(qname="r%d" % (k // 2), flag=(99, 147)[k % 2], tid=0, pos=100 + 200 * (k // 2), cigar="30M", mtid=0, mpos=-1, isize=-30, seq="ACGT" * 7 + "AC", qual=[30] * L, nm=0)
            for k in range(6)]
    return ReadBatch.from_records(recs)


def bare_params(n_ref=2000, **over):
    from gencore_amd.capi import default_params
    from lencases import pack_reference
    tl = np.asarray([n_ref], np.uint32)
    prm = default_params(n_targets=1, target_len=tl.ctypes.data, umi_prefix="", flush_period=1 << 30, **over)
    prm._keep = tl
    return prm, [(pack_reference("ACGT" * (n_ref // 4)), n_ref)]
