"""Streams of hand-built clusters for the mate-pairing tiers (CPU only).

Mate pairing and UMI grouping run in six GPU tiers; a cluster goes to one of them by its read count, its name and UMI lengths and
what its names look like.  This module builds streams whose clusters sit on the routing edges, with every name, UMI and arrival order
chosen by the caller, and states the routing as a spec (`expected_tier`) the GPU tests hold the engine's per-cluster tier ids to.

Every cluster is N reads that share one key (tid, left, |isize|) (d_key, gce_device.hpp): forward reads (flag 99) at `left`, reverse
reads (flag 147) at left + INSERT - READ_LEN, both with isize +-INSERT.  The forward reads of a cluster arrive first, in the order given,
then its reverse reads.  Reads with the same name in a cluster are one pair (first read = left, last read = right; pair.cpp:188-216);
a name with one read is a lost mate, a name with three is a third read.  UMIs ride in the name behind its last ':' (umi_prefix "")
or in an MI:Z tag.
"""
from dataclasses import dataclass, field

import numpy as np

READ_LEN = 30
INSERT = 80
STEP = 3                                   # positions between the `left`s of two clusters

TIERS = ("never", "sub16", "sub32", "fast", "deep_lds", "deep_device", "generic")      # GCE_PAIR_TIER_* (include/gencore_amd.h)
PD_MAX = 4096                              # k_pairing_deep in LDS: 65..PD_MAX reads (gce_deep.hpp)
PD_BIGMAX = 65536                          # ... in device memory: up to PD_BIGMAX - 2 reads
RUN_MAX = 32                               # reads with different names behind one 16-byte window the deep kernel sorts itself


# ------------------------------------------------------------------------------------------------------------ the name hash
def name_words(name, nwords=8):
    """A name as big-endian 64-bit words, zero-padded (what the register tiers load: gce_pair2.hpp:114-123)."""
    b = bytes(name) + bytes(8 * nwords - len(name))
    return [int.from_bytes(b[8 * k:8 * k + 8], "big") for k in range(nwords)]


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF


def h32(words, nwords):
    """The add-rotate-xor filter of k_pairing_sub / k_pairing_fast (gce_pair2.hpp:127-134) over the first `nwords` words.
    nwords is the wave-wide maximum there (over 4 clusters in <16>, 2 in <32>).  A zero word maps the state through a bijection, so
    whether two names hash alike does not depend on nwords once it covers both names."""
    h = 0x9E3779B9
    for k in range(nwords):
        lo, hi = words[k] & 0xFFFFFFFF, words[k] >> 32
        h = ((_rotl(h, 5) ^ lo) + hi) & 0xFFFFFFFF
        h = _rotl(h, 11) ^ ((hi + 0x7F4A7C15) & 0xFFFFFFFF)
    return h ^ (h >> 15)


def h32_np(words, nwords):
    """h32 over many names at once: words uint64 [n, >= nwords]."""
    h = np.full(words.shape[0], 0x9E3779B9, np.uint64)
    m = np.uint64(0xFFFFFFFF)
    rot = lambda x, r: ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & m
    for k in range(nwords):
        lo, hi = words[:, k] & m, words[:, k] >> np.uint64(32)
        h = ((rot(h, 5) ^ lo) + hi) & m
        h = rot(h, 11) ^ ((hi + np.uint64(0x7F4A7C15)) & m)
    return (h ^ (h >> np.uint64(15))).astype(np.uint32)


def collision_pairs(prefix=b"hc:", count=4, n=1 << 18, seed=1):
    """Distinct names of one length whose h32 is equal: a birthday search over `n` names prefix + 10 pseudo-random letters (deterministic:
    a fixed seed.  Names that count up hash without a collision -- the filter is close to linear in a few varying bytes)."""
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz234567", np.uint8)
    pick = letters[np.random.default_rng(seed).integers(0, 32, (n, 10))]
    names = sorted({prefix + bytes(row) for row in pick})
    n = len(names)
    L = len(names[0])
    nw = (L + 7) // 8
    raw = np.frombuffer(b"".join(x + bytes(8 * nw - L) for x in names), ">u8").reshape(n, nw).astype(np.uint64)
    h = h32_np(raw, nw)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    dup = np.nonzero(hs[1:] == hs[:-1])[0]
    out = [(names[order[i]], names[order[i + 1]]) for i in dup[:count]]
    assert len(out) == count, "too few h32 collisions among %d names" % n
    return out


# ------------------------------------------------------------------------------------------------------------ clusters
@dataclass
class Cluster:
    """fwd / rev: names (bytes) of the forward / reverse reads in arrival order.  mi: name -> MI:Z value (bytes) for every read of that
    name (or per read: a list as long as that name's reads, forward reads first)."""
    fwd: list
    rev: list = field(default_factory=list)
    mi: dict = field(default_factory=dict)
    label: str = ""
    tier: str = None                       # what the test means to reach (checked against expected_tier when the stream is built)
    left: int = -1
    first: int = -1                        # stream index of its first read

    @property
    def n(self):
        return len(self.fwd) + len(self.rev)

    def reads(self):
        return list(self.fwd) + list(self.rev)

    def umis(self):
        """UMI of every read in arrival order (BamUtil::getUMI with umi_prefix "": MI:Z if present, else the name; the slice behind the
        last ':' if it is all [ACGT_] with at most one '_')."""
        seen, out = {}, []
        for nm in self.reads():
            k = seen.get(nm, 0); seen[nm] = k + 1
            v = self.mi.get(nm)
            if isinstance(v, list):
                v = v[k]
            out.append(umi_slice(v if v is not None else nm))
        return out


def umi_slice(s):
    s = bytes(s)
    i = s.rfind(b":")
    if i < 0 or i >= len(s) - 1:
        return b""
    u = s[i + 1:]
    if len(u) > 1 and u[:1] == b"_":
        u = u[1:]
    if any(ch not in b"ACGT_" for ch in u) or u.count(b"_") > 1:
        return b""
    return u


def pairs_cluster(names, lost=(), third=(), **kw):
    """Both mates of every name (forward reads in the order of `names`, reverse reads likewise); `lost`: names whose reverse read is
    missing; `third`: names with one more forward read (behind all other forward reads)."""
    fwd = list(names) + list(third)
    rev = [x for x in names if x not in set(lost)]
    return Cluster(fwd=fwd, rev=rev, **kw)


def sized_cluster(n, tag, name_len=None, **kw):
    """n reads: n // 2 pairs, and a lost mate when n is odd.  Names tag + serial, padded with 'x' to name_len."""
    names = []
    for i in range((n + 1) // 2):
        nm = b"%s:%d" % (tag, i)
        if name_len is not None:
            assert len(nm) <= name_len, (nm, name_len)
            nm += b"x" * (name_len - len(nm))
        names.append(nm)
    return pairs_cluster(names, lost=names[-1:] if n % 2 else (), **kw)


# ------------------------------------------------------------------------------------------------------------ the routing spec
def _deep_windows(names):
    """cp, and per read (window, rest) as k_pairing_deep computes them: the common prefix of every name with the first read's, the 16
    name bytes behind it (zero-padded) and how many bytes follow the window."""
    n0 = names[0]

    def common(a, b):
        k = 0
        while k < min(len(a), len(b)) and a[k] == b[k]:
            k += 1
        return k
    cp = min(common(n0, nm) for nm in names)
    out = []
    for nm in names:
        w = nm[cp:cp + 16]
        out.append((w + bytes(16 - len(w)), max(len(nm) - cp - 16, 0)))
    return cp, out


def deep_run_too_long(names):
    """k_pairing_deep's hand-on for name order (gce_deep.hpp, after the bitonic sort): a run of more than RUN_MAX reads with equal windows
    in which some read's name goes on behind the window."""
    _, wr = _deep_windows(names)
    runs = {}
    for w, rest in wr:
        r = runs.setdefault(w, [0, 0]); r[0] += 1; r[1] |= rest
    return any(cnt > RUN_MAX and rest for cnt, rest in runs.values())


def hash_false_match(names):
    nw = (max(len(x) for x in names) + 7) // 8
    by = {}
    for x in set(names):
        by.setdefault(h32(name_words(x), nw), set()).add(x)
    return any(len(v) > 1 for v in by.values())


def expected_tier(cl, mode=None):
    """The tier that pairs a cluster (engine.hip's pairing dispatch; include/gencore_amd.h GCE_PAIR_TIER_*).  mode ("classes": size classes
    with direct hand-on to left_list, N > 10 C; "chain": flag-and-compact) does not change the tier: every hand-on of either order ends
    where the other's does -- it is an argument so that the spec says so.  Clusters are never THR_NEVER here (the whole stream is flushed)."""
    assert mode in (None, "classes", "chain")
    names = cl.reads()
    n = len(names)
    nl = max(len(x) for x in names)
    ul = max(len(u) for u in cl.umis())
    if n <= 64:                                                          # k_pairing_sub<16>, <32>, k_pairing_fast
        if nl > 64 or ul > 24 or hash_false_match(names):
            return "generic"
        return "sub16" if n <= 16 else ("sub32" if n <= 32 else "fast")
    if n > PD_BIGMAX - 2 or ul > 16 or deep_run_too_long(names):          # k_pairing_deep, both instantiations
        return "generic"
    return "deep_lds" if n <= PD_MAX else "deep_device"


# ------------------------------------------------------------------------------------------------------------ the stream
class Stream:
    """Clusters laid out on one contig, each at its own `left`; `records()` gives them coordinate-sorted for ReadBatch.from_records."""

    def __init__(self, seed=0):
        self.clusters = []
        self.rng = np.random.default_rng(seed)

    def add(self, cl):
        cl.left = 50 + STEP * len(self.clusters)
        self.clusters.append(cl)
        if cl.tier is not None:
            assert expected_tier(cl) == cl.tier, (cl.label, expected_tier(cl), cl.tier)
        return cl

    def pad_singletons(self, count, tag=b"pad"):
        """`count` clusters of one pair each (they lower the mean cluster size: N <= 10 C chooses the flag-and-compact order)."""
        for i in range(count):
            self.add(sized_cluster(2, b"%s:%d" % (tag, i), label="pad"))

    @property
    def n_reads(self):
        return sum(c.n for c in self.clusters)

    def mode(self):
        return "classes" if self.n_reads > 10 * len(self.clusters) else "chain"

    def contig(self):
        ln = 50 + STEP * len(self.clusters) + INSERT + 100
        return "".join(self.rng.choice(list("ACGT"), ln))

    def records(self, contig):
        recs = []
        for ci, cl in enumerate(self.clusters):
            lp, rp = cl.left, cl.left + INSERT - READ_LEN
            seen = {}
            for side, nms, pos, mpos, flag, isz in (("F", cl.fwd, lp, rp, 99, INSERT), ("R", cl.rev, rp, lp, 147, -INSERT)):
                for nm in nms:
                    k = seen.get(nm, 0); seen[nm] = k + 1
                    mi = cl.mi.get(nm)
                    if isinstance(mi, list):
                        mi = mi[k]
                    r = dict(qname=nm.decode(), flag=flag, tid=0, pos=pos, cigar="%dM" % READ_LEN, mtid=0, mpos=mpos, isize=isz,
                             seq=contig[pos:pos + READ_LEN], qual=[30] * READ_LEN, nm=0, _cl=ci)
                    if mi is not None:
                        r["mi"] = mi.decode()
                    recs.append(r)
        recs.sort(key=lambda r: r["pos"])                               # (stable: arrival order inside a cluster stays as given)
        for i, r in enumerate(recs):
            cl = self.clusters[r["_cl"]]
            if cl.first < 0:
                cl.first = i
        return recs

    def build(self):
        """(ReadBatch, params, reference, cluster of every stream read)."""
        from gencore_amd.batch import ReadBatch
        from gencore_amd.capi import default_params
        from oracle import oracle_py
        contig = self.contig()
        recs = self.records(contig)
        owner = np.asarray([r.pop("_cl") for r in recs], np.int64)
        batch = ReadBatch.from_records(recs)
        tl = np.asarray([len(contig)], np.uint32)
        prm = default_params(n_targets=1, target_len=tl.ctypes.data, umi_prefix="", flush_period=1 << 30,
                             skip_low_complexity_cluster_threshold=1 << 20)
        prm._keep = tl
        return batch, prm, [(oracle_py.pack_reference(contig), len(contig))], owner


# ------------------------------------------------------------------------------------------------------------ the edge catalogue
def filled_cluster(n, tag, special, seed, shuffle=True, **kw):
    """n reads: both mates of every name in `special`, then pairs of filler names tag:f<i> (a lost mate when n is odd), forward and
    reverse reads each in a seeded shuffle."""
    names = list(special)
    i = 0
    while 2 * len(names) < n:
        names.append(b"%s:f%d" % (tag, i)); i += 1
    assert 2 * len(names) - n in (0, 1), (n, len(special))
    lost = names[-1:] if n % 2 else ()
    fwd, rev = list(names), [x for x in names if x not in set(lost)]
    if shuffle:
        rng = np.random.default_rng(seed)
        fwd = [fwd[k] for k in rng.permutation(len(fwd))]
        rev = [rev[k] for k in rng.permutation(len(rev))]
    return Cluster(fwd=fwd, rev=rev, **kw)


REGISTER_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)
DEEP_SIZES = (65, 66, 4095, 4096, 4097, 4098)
TIER_OF_SIZE = {1: "sub16", 2: "sub16", 15: "sub16", 16: "sub16", 17: "sub32", 31: "sub32", 32: "sub32", 33: "fast", 63: "fast", 64: "fast",
                65: "deep_lds", 66: "deep_lds", 4095: "deep_lds", 4096: "deep_lds", 4097: "deep_device", 4098: "deep_device"}
REGISTER_EDGE = (16, 17, 64)               # one size per register tier for the name / UMI edges
DEEP_EDGE = (70, 4100)


def order_names(tag, kind):
    """Names that take the unusual branches of the register tiers' name order (gce_pair2.hpp:173-221, gce_pairing.hpp:295-329)."""
    t = tag
    if kind == "prefix":                   # names that are prefixes of others
        return [t + b":ab", t + b":abc", t + b":abcd", t + b":ab7", t + b":a", t + b":abc0"]
    if kind == "tie":                      # equal 8-byte order words behind the common prefix: the full compare decides
        return [t + b":QRSTUVWXa", t + b":QRSTUVWXb", t + b":QRSTUVWX", t + b":QRSTUVWXab", t + b":QRSTUVWW", t + b":QRSTUVWXYZ0"]
    if kind == "cp56":                     # common prefix of 56 bytes or more: the order word stops at byte 56 (min(cp, 56))
        p = t + b":" + b"L" * (58 - len(t))
        return [p + b"b", p + b"ab", p + b"a", p + b"aa", p + b"c"]
    if kind == "byte63":                   # 64-byte names that differ only in their last byte
        p = t + b":" + b"M" * (62 - len(t))
        return [p + b"b", p + b"a", p + b"z", p + b"B"]
    if kind == "high":                     # bytes >= 0x80: strcmp orders them as unsigned
        return [t + b":" + x.encode() for x in ("e", "é", "z", "ÿ", "Āx", "E")]
    raise ValueError(kind)


def window_names(tag, end, longer=1):
    """For the deep kernel's 16-byte window behind the common prefix cp = len(tag) + 1: a name that ends at cp + end and `longer` names
    that start with it (the long ones share its window when end == 16)."""
    p = tag + b":"
    a = p + b"W" * end
    return [a] + [a + b"%d" % k for k in range(7, 7 + longer)]


def core_clusters(seed=0):
    """Every edge of the routing table and of the name order, one cluster each (labels say which)."""
    cls = []
    add = lambda cl: cls.append(cl)
    for n in REGISTER_SIZES + DEEP_SIZES:
        add(filled_cluster(n, b"sz%d" % n, [], seed + n, label="size %d" % n, tier=TIER_OF_SIZE[n]))
    for n in REGISTER_EDGE + DEEP_EDGE:
        home = TIER_OF_SIZE.get(n, "deep_lds" if n <= PD_MAX else "deep_device")
        deep = n > 64
        for ln in (63, 64, 65, 254):       # one pair with a name of ln bytes
            nm = b"nl%d.%d:" % (n, ln); nm += b"q" * (ln - len(nm))
            add(filled_cluster(n, b"nl%d.%d" % (n, ln), [nm], seed + ln, label="name %d B in %d" % (ln, n),
                               tier=home if (deep or ln <= 64) else "generic"))
        for ul in (16, 17, 24, 25):        # one pair with a UMI of ul bytes, in the name and in MI:Z
            umi = (b"ACGT" * 7)[:ul]
            nm = b"ul%d.%d:xx:" % (n, ul) + umi
            limit = 16 if deep else 24
            add(filled_cluster(n, b"ul%d.%d" % (n, ul), [nm], seed + ul, label="name UMI %d B in %d" % (ul, n),
                               tier=home if ul <= limit else "generic"))
            nm2 = b"mi%d.%d:xx" % (n, ul)
            add(filled_cluster(n, b"mi%d.%d" % (n, ul), [nm2], seed + ul + 1, mi={nm2: b"u:" + umi}, label="MI UMI %d B in %d" % (ul, n),
                               tier=home if ul <= limit else "generic"))
        if not deep:
            for where in ("first", "middle", "last"):      # one 65-byte name among short ones, in the first / a middle / the last lane
                long_ = b"lw%d%s:" % (n, where.encode()); long_ += b"r" * (65 - len(long_))
                cl = filled_cluster(n, b"lw%d%s" % (n, where.encode()), [], seed, shuffle=False)
                k = {"first": 0, "middle": len(cl.fwd) // 2, "last": len(cl.fwd) - 1}[where]
                old = cl.fwd[k]
                cl.fwd[k] = long_
                cl.rev = [long_ if x == old else x for x in cl.rev]
                cl.label, cl.tier = "65 B name in the %s lane of %d" % (where, n), "generic"
                add(cl)
            for kind in ("prefix", "tie", "cp56", "byte63", "high"):
                tag = b"o%s%d" % (kind.encode()[:2], n)
                add(filled_cluster(n, tag, order_names(tag, kind), seed + n, label="name order %s in %d" % (kind, n), tier=TIER_OF_SIZE[n]))
                # the same names as the whole cluster (the common prefix is then theirs)
                sp = order_names(tag + b"w", kind)
                if 2 * len(sp) <= n:
                    add(filled_cluster(2 * len(sp), tag + b"w", sp, seed + n, label="only %s names" % kind, tier=expected_tier(
                        filled_cluster(2 * len(sp), tag + b"w", sp, seed + n))))
    for n in DEEP_EDGE:
        home = "deep_lds" if n <= PD_MAX else "deep_device"
        for end in (15, 16, 17):
            for short_first in (True, False):
                tag = b"dw%d.%d%s" % (n, end, b"f" if short_first else b"l")
                sp = window_names(tag, end, longer=2)
                cl = filled_cluster(n, tag, sp, seed + end, shuffle=False)
                if not short_first:                        # the longer names' reads arrive first, the short name's last
                    cl.fwd = [x for x in cl.fwd if x != sp[0]] + [sp[0]]
                    cl.rev = [x for x in cl.rev if x != sp[0]] + [sp[0]]
                cl.label, cl.tier = "name ends at cp+%d, short name %s, in %d" % (end, "first" if short_first else "last", n), home
                add(cl)
        for run in (32, 33):               # `run` reads with different names behind one window
            tag = b"dr%d.%d" % (n, run)
            sp = window_names(tag, 16, longer=(run + 1) // 2)[1:]
            cl = filled_cluster(n, tag, sp, seed + run, shuffle=False)
            if run % 2:                    # an odd run: one name of the run loses its mate; a lost mate of a filler name keeps the read count
                cl.rev.remove(sp[-1])
                cl.fwd.append(b"%s:odd" % tag)
            cl.label, cl.tier = "run of %d reads behind one window in %d" % (run, n), home if run <= RUN_MAX else "generic"
            add(cl)
        tag = b"ds%d" % n                   # the first read has the shortest name
        cl = filled_cluster(n, tag, [tag + b":", tag + b":" + b"s" * 40], seed, shuffle=False, label="shortest name first in %d" % n, tier=home)
        add(cl)
    for cl in cls:
        assert cl.tier is None or expected_tier(cl) == cl.tier, (cl.label, expected_tier(cl), cl.tier)
    return cls


def collision_clusters(seed=0):
    """Clusters of <= 16, 17..32 and 33..64 reads with two different names that hash alike under h32 (the false-match hand-on), and
    the same sizes without them.  Every name of these clusters is 13 bytes long (two words)."""
    cls = []
    pairs = collision_pairs()
    for n in (4, 16, 17, 32, 33, 64):
        for k, (a, b) in enumerate(pairs[:2]):
            names = [a, b]
            i = 0
            while 2 * len(names) < n:
                names.append(b"hc:f%03d%05d" % (n, i)); i += 1
            cl = filled_cluster(n, b"unused", names, seed + n + k, label="h32 collision %d in %d" % (k, n), tier="generic")
            cls.append(cl)
        names = [b"hc:g%03d%05d" % (n, i) for i in range((n + 1) // 2)]
        cls.append(filled_cluster(n, b"unused", names, seed + n, label="no collision in %d" % n, tier=TIER_OF_SIZE.get(n, "sub16")))
    return cls
