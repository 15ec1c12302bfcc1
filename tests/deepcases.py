"""Named streams for the deep tier of consensus (group sides of more than 64 pairs): side_prepare's class path, k_deep_prepare, k_vote_deep and
k_score2 at their class, voter, window and threshold edges (CPU only; built on lencases.Stream).

A CASE is a named stream of a few groups with
  premise   facts that say the stream reaches its edge, computed from side_spec (below) and plain numpy over the built batch; a premise that fails
            is an error of the catalogue (an AssertionError), never a skip
  routing   the exact tuple of Engine.consensus_counters(): sides finished by (k_vote, k_consensus_fast, k_deep_prepare, k_vote_deep, k_consensus_slow)
  witness   what the oracle's output must show where the case plants its decision (a base, a quality, NM, SE / PE)
  neighbour the name of the case one vote / one parameter step / one plant away: the oracle's outputs of the two differ (the decision is decisive)

side_spec is a plain-Python restatement of the choices of Group::consensusMergeBam (the reference's group.cpp:136-348, bamutil.cpp:204-255 through
oracle_py.is_part_of); it is not a transcription of the kernel and knows nothing of classes, lanes or chunks.

Families: V tallies of k_vote_deep, C classes of side_prepare, T the three thresholds, A alignment, O mate overlap, X back-outs / restore / errors.
Reads are 40 bases, mates apart and the reference present unless a family says otherwise; no case has more than about 1100 pairs."""
from dataclasses import dataclass

import numpy as np

import lencases as lc

DV_CHUNK, DV_COLS, SC2_MAXU = 256, 512, 1280                # gce_deep.hpp, gce_consensus.hpp
GCE_ERR_NM_MISSING = -12
KERNELS = ("vote", "fast", "deep_prepare", "vote_deep", "slow")
NIB = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
OFF = 1 << 20                                                # skip_low_complexity_cluster_threshold: never


# ------------------------------------------------------------------------------------------------------------ the model
def cigar_words(batch, r):
    o = int(batch.cigar_off[r])
    return [int(x) for x in batch.cigar[o:o + int(batch.core["n_cigar"][r])]]


def right_ref_pos(batch, r):
    """BamUtil::getRightRefPos: pos + the reference bases the CIGAR consumes (M, D, N, =, X)."""
    return int(batch.core["pos"][r]) + sum(w >> 4 for w in cigar_words(batch, r) if (w & 15) in (0, 2, 3, 7, 8))


def side_spec(batch, params, reads, is_left):
    """Group::consensusMergeBam's choices for one side.  reads: the side's read index per pair in qname order (None: the pair has no such read).
    Returns a dict: left_mode, n_cigars (distinct CIGAR strings), n_classes (distinct (n_cigar, right end on a right side, words)), max_ops,
    diff_neighbor (of the first present read), contained (as the early break leaves it), template (index into `reads`, or None) and reason,
    voters (indices into `reads`, the template first), len_diff (per voter) and length (columns of the consensus)."""
    from oracle import oracle_py
    n, thr = len(reads), int(params.skip_low_complexity_cluster_threshold)
    memo = {}

    def part_of(a, b, lm):                                     # (reads of one CIGAR are interchangeable: one call per pair of CIGARs)
        key = (tuple(a), tuple(b), lm)
        if key not in memo:
            memo[key] = oracle_py.is_part_of(a, b, lm)
        return memo[key]
    cg = {k: cigar_words(batch, r) for k, r in enumerate(reads) if r is not None}
    rr = {k: right_ref_pos(batch, reads[k]) for k in cg}
    present = sorted(cg)
    out = dict(left_mode=is_left, n_cigars=len({tuple(v) for v in cg.values()}), max_ops=max([len(v) for v in cg.values()] or [0]),
               n_classes=len({(tuple(cg[k]), 0 if is_left else rr[k]) for k in cg}), diff_neighbor=None, contained=[0] * n, template=None,
               reason=None, voters=[], len_diff=[], length=0)
    if present:
        s = batch.seq_of(reads[present[0]])
        out["diff_neighbor"] = sum(1 for i in range(len(s) - 1) if s[i] != s[i + 1])
        if n > thr and out["n_cigars"] > n * 0.1 and out["diff_neighbor"] < len(s) * 0.5:      # group.cpp:142-175
            out["reason"] = "low complexity"
            return out
    if not is_left:                                                                          # group.cpp:177-194
        left_aligned, last = True, -1
        for k in present:
            p = int(batch.core["pos"][reads[k]])
            if last >= 0 and p != last:
                left_aligned = False
                break
            last = p
        out["left_mode"] = left_aligned
    lm = out["left_mode"]
    for i in range(n):                                                                       # group.cpp:196-233
        if i not in cg:
            continue
        c = 1
        for j in present:
            if j == i or (not is_left and rr[i] != rr[j]):
                continue
            c += part_of(cg[i], cg[j], lm)
        out["contained"][i] = c
        if n > thr and c >= n // 2:
            break
    best, bn = -1, -1                                                                        # group.cpp:235-261
    lq = lambda k: int(batch.core["l_qseq"][reads[k]]) if reads[k] is not None else 0
    for i, c in enumerate(out["contained"]):
        if c > bn:
            bn, best = c, i
        elif c == bn and best >= 0 and lq(i) < lq(best):
            best = i
    if bn < n * 0.4 and n != 1:
        out["reason"] = "no majority"
        return out
    if reads[best] is None:
        out["reason"] = "template absent"
        return out
    out["template"] = best
    t = reads[best]
    voters = [best] + [j for j in present if j != best and part_of(cg[best], cg[j], lm)]   # group.cpp:287-313
    ld = []
    for j in voters:                                                                         # group.cpp:339-348
        d = lq(j) - lq(best)
        if d != 0 and batch.core["pos"][reads[j]] == batch.core["pos"][t] and part_of(cg[best], cg[j], True):
            d = 0
        ld.append(d)
    out["voters"], out["len_diff"] = voters, ld
    out["length"] = lq(best) if cg[best] else min(lq(j) for j in voters)
    return out


# ------------------------------------------------------------------------------------------------------------ stream and case
class DeepStream(lc.Stream):
    """lencases.Stream with its own parameters (skip_low_complexity_cluster_threshold and any other field of gce_params) and, per group, hooks
    that edit the built batch: group.post = [f(batch, where, group index)] (the NM type of a read)."""

    def __init__(self, seed=0, flush_period=1 << 30, skip=OFF, **prm):
        super().__init__(seed=seed, flush_period=flush_period)
        self.skip, self.prm = skip, prm

    def build(self, drop=None):
        batch, prm, ref = super().build(drop)
        prm.skip_low_complexity_cluster_threshold = self.skip
        for k, v in self.prm.items():
            setattr(prm, k, v)
        for gi, g in enumerate(self.groups):
            assert None not in g.left                          # (Cluster::addRead: a lone read of a name IS its pair's left read; only right reads can be absent)
            for f in getattr(g, "post", ()):
                f(batch, self.where, gi)
        return batch, prm, ref

    def reads_of(self, gi, side):
        g = self.groups[gi]
        return [self.where.get((gi, side, k)) for k in range(len(g.left))]


@dataclass
class Case:
    name: str
    family: str
    make: object                   # () -> DeepStream (items added)
    premise: object                # (Built) -> None; asserts
    routing: tuple
    witness: object = None         # (Built, oracle result) -> None; asserts
    neighbour: str = None
    error: int = 0
    combine: bool = True           # part of the combined stream (default parameters, no error)


class Built:
    def __init__(self, case):
        self.case, self.st = case, case.make()
        self.batch, self.prm, self.ref = self.st.build()
        self._spec = {}

    def spec(self, gi=0, side=0):
        if (gi, side) not in self._spec:
            self._spec[(gi, side)] = side_spec(self.batch, self.prm, self.st.reads_of(gi, side), side == 0)
        return self._spec[(gi, side)]

    def read(self, gi, side, k):
        return self.st.where[(gi, side, k)]

    def template_read(self, gi=0, side=0):
        t = self.spec(gi, side)["template"]
        return None if t is None else self.read(gi, side, t)

    def model_routing(self):
        """The counter tuple side_spec and the kernels' scope rules give: k_vote up to 64 pairs (every such group here is clean), beyond that
        k_deep_prepare without a template, k_consensus_slow for an exotic voter or more than DV_COLS columns, k_vote_deep otherwise."""
        cnt = dict.fromkeys(KERNELS, 0)
        odd = lambda rd: any(set(self.batch.seq_of(r)) - set("ACGTN") or (self.batch.qual_of(r) >= 128).any() for r in rd)
        for gi, g in enumerate(self.st.groups):
            sides = [[r for r in self.st.reads_of(gi, side) if r is not None] for side in (0, 1)]
            for side in (0, 1):
                sp = self.spec(gi, side)
                if len(g.left) <= 64:                           # an exotic read: k_vote hands the whole group on, k_consensus_fast leaves the exotic side
                    cnt[("slow" if odd(sides[side]) else "fast") if odd(sides[0] + sides[1]) else "vote"] += 1
                elif sp["template"] is None:
                    cnt["deep_prepare"] += 1
                else:
                    exotic = odd([self.read(gi, side, k) for k in sp["voters"]])
                    cnt["slow" if exotic or sp["length"] > DV_COLS else "vote_deep"] += 1
        return tuple(cnt[k] for k in KERNELS)


CASES = {}


def case(name, family, make, premise, routing, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, family, make, premise, tuple(routing), **kw)


def out_nib(b, want, r, col):
    return (int(want.seq[int(b.batch.seq_off[r]) + col // 2]) >> (4 if col % 2 == 0 else 0)) & 15


def out_qual(b, want, r, col):
    return int(want.qual[int(b.batch.qual_off[r]) + col])


def names(n):
    return ["p%04d" % k for k in range(n)]                   # (the reference's pair order is the order of the names)


def dcut(ref, off, ops, rng):
    """A read over `ref` from `off`: M copies, D / N skip, I / S draw bases, H holds none."""
    seq, p = [], off
    for n, op in ops:
        if op == "M":
            seq += list(ref[p:p + n]); p += n
        elif op in "DN":
            p += n
        elif op in "IS":
            seq += ["ACGT"[int(x)] for x in rng.integers(0, 4, n)]
    return seq


def ops_read(ref, off, ops, rng, q=37):
    seq = dcut(ref, off, ops, rng)
    return lc.Read(off, lc.cigar_str(ops), seq, [q] * len(seq))


def plain_group(label, n, L=40, gap=10, **kw):
    """n pairs of L-base reads, all `LM`, mates `gap` apart: builder(fill) -> lencases builder; fill(g, ref, rng) plants the case."""
    def make(fill):
        def build(ref, rng, drop_at):
            g = lc.new_group(label, 2 * L + gap, 2 * L + gap, drop_at, **kw)
            g.left = [lc.plain_read(ref, 0, L) for _ in range(n)]
            g.right = [lc.plain_read(ref, L + gap, L) for _ in range(n)]
            g.names = names(n)
            fill(g, ref, rng)
            return g
        return build
    return make


def set_base(r, col, ch, ref_ch):
    if r.seq[col] == ref_ch and ch != ref_ch:
        r.nm += 1
    elif r.seq[col] != ref_ch and ch == ref_ch:
        r.nm -= 1
    r.seq[col] = ch


def one_stream(builders, seed=1, **kw):
    def make():
        return DeepStream(seed=seed, **kw).add(builders if isinstance(builders, list) else [builders], ("deep", 0))
    return make


def only_quality(b, r, col, reads, q=40):
    """Premise: read r is the only one of `reads` with quality q in column col, and every other shows 37 there."""
    col_q = [int(b.batch.qual[int(b.batch.qual_off[x]) + col]) for x in reads]
    assert col_q[reads.index(r)] == q and sorted(col_q)[-2] == 37 and col_q.count(q) == 1, (col, col_q[:8])


# ============================================================================================================ family V: tallies of k_vote_deep
V_NP = (65, 66, 128, 129, 255, 256, 257, 320, 513, 1025)
V_VOTERS = (0, 1, 3, 4, 15, 16, 17, 31, 32, 63, 64, 255, 256, 257, -1)      # sub, unroll, trip, wave and chunk edges of q = qr + 16 u + sub; -1: nv - 1


def topq_plan(n, L, key_cols, side):
    """(voter, column) pairs of one side: every voter index of V_VOTERS below n on a column of its own, the key columns rotating over the voters with n and the side."""
    voters = sorted({(n - 1 if v < 0 else v) for v in V_VOTERS if v < n})
    extra = [c for c in (1, 14, 18, 31, 32, 33, 3, 4, 7, 8, 2, 5, 6, 9, 10) if c < L and c not in key_cols]
    cols = (list(key_cols) + extra)[:len(voters)]
    rot = (n + 5 * side) % len(voters)
    return [(v, cols[(i + rot) % len(voters)]) for i, v in enumerate(voters)]


def add_topq(n, L, key_cols):
    name = "V.topq.np%d%s" % (n, "" if L == 40 else ".L%d" % L)

    def fill(g, ref, rng):
        for side, reads in ((0, g.left), (1, g.right)):
            for v, c in topq_plan(n, L, key_cols, side):
                reads[v].qual[c] = 40

    def premise(b):
        for side in (0, 1):
            sp = b.spec(0, side)
            assert sp["template"] == 0 and sp["voters"] == list(range(n)) and sp["left_mode"] and sp["n_classes"] == 1 and set(sp["len_diff"]) == {0}
            rd = [b.read(0, side, k) for k in sp["voters"]]
            plan = topq_plan(n, L, key_cols, side)
            assert {v for v, _ in plan} >= {0, 1, n - 1} and len({c for _, c in plan}) == len(plan)
            assert n < 258 or {255, 256, 257} <= {v for v, _ in plan}
            for v, c in plan:
                only_quality(b, rd[v], c, rd)
        used = {c for s in (0, 1) for _, c in topq_plan(n, L, key_cols, s)}
        assert set(key_cols) <= used

    def witness(b, want):
        for side in (0, 1):
            t = b.template_read(0, side)
            cols = {c for _, c in topq_plan(n, L, key_cols, side)}
            assert want.out_flag[t] != 0
            got = [out_qual(b, want, t, c) for c in range(L)]
            assert got == [40 if c in cols else 37 for c in range(L)], (side, got)

    case(name, "V", one_stream(plain_group(name, n, L)(fill), seed=n), premise, (0, 0, 0, 2, 0), witness=witness)


for _n in V_NP:
    add_topq(_n, 40, (0, 15, 16, 17, 39))
add_topq(257, 272, (255, 256, 271, 0, 15, 16, 17))           # the `cb` loop: a second block of 256 columns


def share_sets(n, nd, polarity, where):
    """The nd voters that hold the MINORITY base.  polarity tmaj: the template (voter 0) is in the majority, tmin: in the minority.
    where: first (the first chunk), last (the last, partial chunk), spread (one per 16-voter lane group as far as they go)."""
    if where == "first":
        d = list(range(1, nd + 1))
    elif where == "last":
        d = list(range(n - nd, n))
    else:
        d = [1 + (i * (n - 1)) // nd for i in range(nd)]
    if polarity == "tmin":
        d = [0] + d[:-1]
    assert len(set(d)) == nd and (0 in d) == (polarity == "tmin")
    return d


def add_share(n, nd, polarity, where, keeps, neighbour=None, col=5, prm=None, tag="share", major="alt", mirror=False):
    """n voters, nd of them with the reference's base in column `col` at quality 37, the others with another base (major: alt, or N): the majority's
    score share is (n - nd) / n against scorePercentReq 0.8.  keeps: the majority's base comes out; else the reference's does."""
    name = "V.%s.np%d.%d-%d.%s.%s" % (tag, n, n - nd, nd, polarity, where)
    prm = prm or {}

    def fill(g, ref, rng):
        d = set(share_sets(n, nd, polarity, where))
        for k, r in enumerate(g.left):
            if k not in d:
                set_base(r, col, "N" if major == "N" else lc.alt(ref[col]), ref[col])
        if mirror:                                           # mates in full overlap, base for base: every score is score_high + 4
            for l, r in zip(g.left, g.right):
                r.seq, r.nm = list(l.seq), l.nm

    def premise(b):
        sp = b.spec(0, 0)
        assert sp["template"] == 0 and len(sp["voters"]) == n and sp["n_classes"] == 1
        if mirror:
            l, r = b.read(0, 0, 7), b.read(0, 1, 7)
            assert b.batch.core["pos"][l] == b.batch.core["pos"][r] and b.batch.seq_of(l) == b.batch.seq_of(r)
            assert b.prm.score_high + 4 == 127 and min(b.prm.score_bad, b.prm.score_low, b.prm.score_moderate) - 3 == -128    # biased: 0 .. 255
        rd = [b.read(0, 0, k) for k in sp["voters"]]
        colb = [b.batch.seq_of(r)[col] for r in rd]
        refb = b.batch.seq_of(b.read(0, 1, 0))               # (any base the right side shows is the reference's: nothing is planted there)
        minority = [k for k, ch in enumerate(colb) if ch != colb[0]] if polarity == "tmaj" else [k for k, ch in enumerate(colb) if ch == colb[0]]
        assert len(minority) == nd and len(set(colb)) == 2 and refb is not None
        assert (0 in minority) == (polarity == "tmin")
        if where == "first":
            assert max(minority) < DV_CHUNK
        elif where == "last":
            assert min(m for m in minority if m) >= n - nd and (n - 1 in minority or polarity == "tmin")
        else:
            assert len({k // 16 for k in minority}) >= min(nd, n // 16)
        frac = float(prm.get("score_percent_req", 0.8))
        assert ((n - nd) >= frac * n) == keeps, (n, nd)     # equal scores: the share of the votes is the share of the score

    def witness(b, want):
        t = b.template_read(0, 0)
        tb = b.batch.seq_of(t)[col]
        rd = [b.read(0, 0, k) for k in range(n)]
        bases = {b.batch.seq_of(r)[col] for r in rd}
        major_b = ("N" if major == "N" else None) or [x for x in bases if sum(b.batch.seq_of(r)[col] == x for r in rd) == n - nd][0]
        minor_b = (bases - {major_b}).pop()
        assert out_nib(b, want, t, col) == NIB[major_b if keeps else minor_b], (name, tb)

    case(name, "V", one_stream(plain_group(name, n, gap=-40 if mirror else 10)(fill), seed=n + nd, **prm), premise, (0, 0, 0, 2, 0), witness=witness, neighbour=neighbour,
         combine=not prm)
    return name


for _pol in ("tmaj", "tmin"):
    for _wh in ("first", "last", "spread"):
        _b = add_share(320, 65, _pol, _wh, keeps=False)
        add_share(320, 64, _pol, _wh, keeps=True, neighbour=_b)
    add_share(320, 63, _pol, "spread", keeps=True)
    _b = add_share(1025, 206, _pol, "spread", keeps=False)
    add_share(1025, 205, _pol, "spread", keeps=True, neighbour=_b)


# no voter of a whole chunk has the template's base: voters 256 .. 511 dissent (C4[g] == 0 for that chunk)

def add_chunk_zero(nd, keeps, neighbour=None):
    n, col = 1025, 5
    name = "V.chunk0.np1025.%d" % nd

    def fill(g, ref, rng):
        for k, r in enumerate(g.left):
            if not (DV_CHUNK <= k < DV_CHUNK + nd):
                set_base(r, col, lc.alt(ref[col]), ref[col])

    def premise(b):
        sp = b.spec(0, 0)
        assert sp["template"] == 0 and len(sp["voters"]) == n
        rd = [b.read(0, 0, k) for k in sp["voters"]]
        same = [b.batch.seq_of(r)[col] == b.batch.seq_of(rd[0])[col] for r in rd]
        assert [k for k, s in enumerate(same) if not s] == list(range(DV_CHUNK, DV_CHUNK + nd))
        assert (nd == DV_CHUNK) == (not any(same[DV_CHUNK:2 * DV_CHUNK])) and ((n - nd) >= 0.8 * n) == keeps

    def witness(b, want):
        t = b.template_read(0, 0)
        changed = out_nib(b, want, t, col) != NIB[b.batch.seq_of(t)[col]]
        assert changed == (not keeps) and want.nm_new[t] == (-1 if keeps else 0)

    case(name, "V", one_stream(plain_group(name, n)(fill), seed=nd), premise, (0, 0, 0, 2, 0), witness=witness, neighbour=neighbour)
    return name


add_chunk_zero(256, keeps=False, neighbour=add_chunk_zero(205, keeps=True))


def add_tie(kind):
    """300 voters, 150 : 150 between two bases neither of which is the reference's: the reference cannot arbitrate and the top base comes out.  qsum-lo / qsum-hi: qualities 31 / 30 on the earlier / later bin (equal scores, the larger
    quality sum wins); q6: equal qualities, the later bin wins (quirk Q6); q6-one: one voter of the earlier bin at 38 -- the earlier bin wins."""
    n, col = 300, 5
    name = "V.tie.%s" % kind

    def two(ref_ch):
        return sorted((x for x in "ACGT" if x != ref_ch), key=lambda x: NIB[x])[:2]      # (earlier bin, later bin)

    def fill(g, ref, rng):
        lo, hi = two(ref[col])
        for k, r in enumerate(g.left):
            first = k % 2 == 0
            set_base(r, col, lo if first else hi, ref[col])
            r.qual[col] = {"qsum-lo": 31 if first else 30, "qsum-hi": 30 if first else 31, "q6": 37, "q6-one": 37}[kind]
        if kind == "q6-one":
            g.left[2].qual[col] = 38

    def premise(b):
        sp = b.spec(0, 0)
        rd = [b.read(0, 0, k) for k in sp["voters"]]
        assert len(rd) == n
        cb = [b.batch.seq_of(r)[col] for r in rd]
        cq = np.asarray([int(b.batch.qual[int(b.batch.qual_off[r]) + col]) for r in rd])
        lo, hi = sorted(set(cb), key=lambda x: NIB[x])
        assert cb.count(lo) == cb.count(hi) == 150 and (cq >= 30).all()                   # one score class: the score sums are equal
        ql, qh = cq[[x == lo for x in cb]].sum(), cq[[x == hi for x in cb]].sum()
        assert {"qsum-lo": ql > qh, "qsum-hi": ql < qh, "q6": ql == qh, "q6-one": ql == qh + 1}[kind]

    def witness(b, want):
        t = b.template_read(0, 0)
        rd = [b.read(0, 0, k) for k in range(n)]
        lo, hi = sorted({b.batch.seq_of(r)[col] for r in rd}, key=lambda x: NIB[x])
        assert out_nib(b, want, t, col) == NIB[lo if kind in ("qsum-lo", "q6-one") else hi]

    case(name, "V", one_stream(plain_group(name, n)(fill), seed=300), premise, (0, 0, 0, 2, 0), witness=witness,
         neighbour={"qsum-lo": "V.tie.qsum-hi", "q6": "V.tie.q6-one"}.get(kind))


for _k in ("qsum-hi", "qsum-lo", "q6-one", "q6"):
    add_tie(_k)
# an N majority (bin 4): 240 : 60 of 300 keeps the N, 239 : 61 gives the reference's base
add_share(300, 60, "tmaj", "spread", keeps=True, major="N", tag="Nmajor", neighbour=add_share(300, 61, "tmaj", "spread", keeps=False, major="N", tag="Nmajor"))
# score constants at the limit make_dev_params accepts (the reference's scores are `char`): score_max = 123 + 4 = 127, score_bias = 3 - (-125) = 128, a biased
# score byte of 255 in every column of 513 voters whose mates overlap them base for base: 16 x 255 in a 16-bit lane, 513 x 255 in the 24-bit field
SCORE255 = dict(score_high=123, score_moderate=100, score_low=50, score_bad=-125)
add_share(513, 102, "tmaj", "spread", keeps=True, prm=SCORE255, tag="score255", mirror=True,
          neighbour=add_share(513, 103, "tmaj", "spread", keeps=False, prm=SCORE255, tag="score255", mirror=True))


# ============================================================================================================ family C: classes of side_prepare
C_L = 100


def class_group(label, left, right, L=C_L, gap=20, shift=70, posts=()):
    """A group from per-pair specs: left[k] / right[k] = None (no such read) or (ops, offset): left reads at offset 0, right reads at L + gap + shift +
    offset (shift: room for right reads that start further left)."""
    n = len(left)
    assert len(right) == n

    def build(ref, rng, drop_at):
        span = 2 * L + gap + shift + 80
        g = lc.new_group(label, span, span, drop_at)
        g.left = [None if s is None else ops_read(ref, s[1], s[0], np.random.default_rng(k)) for k, s in enumerate(left)]
        g.right = [None if s is None else ops_read(ref, L + gap + shift + s[1], s[0], np.random.default_rng(1000 + k)) for k, s in enumerate(right)]
        g.names = names(n)
        g.post = list(posts)
        return g
    return build


def M(n):
    return [(n, "M")]


def tail_clip(k, L=C_L):
    return [(L - k, "M"), (k, "S")] if k else M(L)


def head_clip(k, L=C_L):
    return [(k, "S"), (L - k, "M")] if k else M(L)


def plant_q(build, marks):
    """marks: [(side, pair, column, quality)] set on the built group."""
    def wrapped(ref, rng, drop_at):
        g = build(ref, rng, drop_at)
        for side, k, c, q in marks:
            (g.left, g.right)[side][k].qual[c] = q
        return g
    return wrapped


def add_classes(nc, place, n=257, five=None):
    """nc classes on both sides: nc - 1 single reads with soft-clip tails (left side) / heads (right side, one right end) of 1 .. nc - 1 bases, placed at the
    head or the tail of the side (tail: the last class -- the one that overflows the 64 lanes at nc = 65 -- is opened by the side's last read; head: by the majority,
    the read behind the singles), every other read `100M`.  five: index of one read with a 5-op CIGAR (the pairwise path).  The majority is the only class
    with more than one read, its first read the template; a quality 40 in its LAST read shows, a 41 in a single read must not."""
    name = "C.classes.%d.%s%s" % (nc, place, "" if five is None else ".five%d" % five)
    ns = nc - 1 - (five is not None)
    idx = list(range(ns)) if place == "head" else list(range(n - ns, n))
    if five is not None:
        idx = [i + 1 for i in idx] if (place == "head" and five == 0) else ([i - 1 for i in idx] if (place == "tail" and five == n - 1) else idx)
    left = [(M(C_L), 0)] * n
    right = [(M(C_L), 0)] * n
    for j, i in enumerate(idx):
        left[i] = (tail_clip(j + 1), 0)
        right[i] = (head_clip(j + 1), j + 1)
    if five is not None:
        left[five] = ([(5, "S"), (40, "M"), (2, "D"), (50, "M"), (5, "S")], 0)
        right[five] = ([(5, "S"), (40, "M"), (2, "D"), (50, "M"), (5, "S")], 3)      # right end: 3 + 92 != 100
    single = set(idx) | ({five} if five is not None else set())
    major = [k for k in range(n) if k not in single]
    marks = [(s, major[-1], 16, 40) for s in (0, 1)] + [(s, idx[0], 17, 41) for s in (0, 1)] if idx else [(s, major[-1], 16, 40) for s in (0, 1)]

    def premise(b):
        for side in (0, 1):
            sp = b.spec(0, side)
            assert sp["n_classes"] == nc and sp["max_ops"] == (5 if five is not None else (2 if nc > 1 else 1)), (sp["n_classes"], nc)
            assert sp["left_mode"] == (side == 0 or nc == 1)
            assert sp["template"] == major[0] and sp["voters"] == major and sp["contained"][major[0]] == len(major) >= 0.4 * n
            assert all(sp["contained"][k] == 1 for k in single) and set(sp["len_diff"]) == {0}
            if nc >= 63 and place == "tail" and five is None:                # the last class is opened by the side's last read
                assert idx[-1] == n - 1 and cigar_words(b.batch, b.read(0, side, n - 1)) not in [cigar_words(b.batch, b.read(0, side, k)) for k in range(n - 1)]

    def witness(b, want):
        for side in (0, 1):
            t = b.template_read(0, side)
            assert want.out_flag[t] != 0 and out_qual(b, want, t, 16) == 40 and out_qual(b, want, t, 17) == 37

    case(name, "C", one_stream(plant_q(class_group(name, left, right), marks), seed=nc), premise, (0, 0, 0, 2, 0), witness=witness)


for _nc in (1, 2, 63, 64, 65):
    for _pl in (("head",) if _nc <= 2 else ("head", "tail")):
        add_classes(_nc, _pl)
add_classes(3, "head", five=0)
add_classes(3, "tail", five=256)


def add_join():
    """Two classes open inside one 64-read batch (reads 10 and 20) and read 30 of the same batch joins the second; reads 70 and 200 join them from later batches."""
    name, n = "C.join", 257
    left = [(M(C_L), 0)] * n
    right = [(M(C_L), 0)] * n
    for i, k in ((10, 1), (20, 2), (30, 2), (70, 1), (200, 2)):
        left[i], right[i] = (tail_clip(k), 0), (head_clip(k), k)

    def premise(b):
        for side in (0, 1):
            sp = b.spec(0, side)
            assert sp["n_classes"] == 3 and [sp["contained"][k] for k in (10, 20, 30, 70, 200)] == [2, 3, 3, 2, 3] and sp["template"] == 0
            assert len(sp["voters"]) == n - 5

    case(name, "C", one_stream(class_group(name, left, right), seed=3), premise, (0, 0, 0, 2, 0))


add_join()


def add_four_ops():
    """4-op CIGARs on both sides.  The right side is right-aligned by one `100M` read at another position (w3 = cg[0]): 57 reads `6S45M2D50M` take the 200
    `5S45M2D50M` as a part only if the FIRST CIGAR word is compared last; they are one base longer and start at the same position, so lenDiff is 1 (odd: the nibble
    shift).  The left side mirrors it with `50M2D45M6S` / `50M2D45M5S` (left mode: lenDiff 0)."""
    name, n = "C.four_ops", 257
    a_l, b_l = [(50, "M"), (2, "D"), (45, "M"), (5, "S")], [(50, "M"), (2, "D"), (45, "M"), (6, "S")]
    a_r, b_r = [(5, "S"), (45, "M"), (2, "D"), (50, "M")], [(6, "S"), (45, "M"), (2, "D"), (50, "M")]
    second = set(sorted(set(range(3, n, 4)) - {255})[:57])
    left = [((b_l if k in second else a_l), 0) for k in range(n)]
    right = [((b_r if k in second else a_r), 0) for k in range(n)]
    right[255] = (M(C_L), 3)
    wk = max(second)
    marks = [(0, wk, 16, 40), (1, wk, 17, 40)]                  # (right side: lenDiff 1, the voter's column 17 is the template's 16)

    def premise(b):
        for side in (0, 1):
            sp = b.spec(0, side)
            nv = n - side
            assert sp["max_ops"] == 4 and sp["n_classes"] == 2 + side and sp["left_mode"] == (side == 0)
            assert sp["template"] == 0 and len(sp["voters"]) == nv and sp["contained"][0] == nv and sp["contained"][wk] == 57
            assert set(sp["len_diff"]) == ({0} if side == 0 else {0, 1}) and sp["len_diff"][sp["voters"].index(wk)] == side

    def witness(b, want):
        for side in (0, 1):
            t = b.template_read(0, side)
            assert out_qual(b, want, t, 16) == 40 and out_qual(b, want, t, 15) == 37 and out_qual(b, want, t, 17) == 37

    case(name, "C", one_stream(plant_q(class_group(name, left, right), marks), seed=4), premise, (0, 0, 0, 2, 0), witness=witness)


add_four_ops()

PART_SHAPES = {   # name: (template-candidate ops, whole ops, is part) -- left side, from the left end
    "last_op": (M(95), M(100), True),
    "middle_op": ([(40, "M"), (2, "D"), (55, "M")], [(45, "M"), (2, "D"), (55, "M")], False),
    "H2": ([(60, "M"), (5, "H")], [(70, "M"), (5, "H")], True),
    "S2": ([(60, "M"), (5, "S")], [(70, "M"), (5, "S")], False),
    "H3": ([(5, "S"), (55, "M"), (5, "H")], [(5, "S"), (65, "M"), (5, "H")], True),
    "S3": ([(5, "S"), (55, "M"), (5, "S")], [(5, "S"), (65, "M"), (5, "S")], False),
    "H4": ([(30, "M"), (2, "D"), (25, "M"), (5, "H")], [(30, "M"), (2, "D"), (35, "M"), (5, "H")], True),
    "S4": ([(30, "M"), (2, "D"), (25, "M"), (5, "S")], [(30, "M"), (2, "D"), (35, "M"), (5, "S")], False),
}


def add_part(shape, side):
    """70 pairs, one side 40 `whole` reads (even pairs first) and 30 `part` reads.  part IS part of whole: a part read is contained by all 70 and is the
    template, every read votes; it is NOT: the first whole read is the template of its 40.  The right side holds the mirrored CIGARs at one right end (the words
    are compared from the other end, and the `H` rule looks at another word of the array); its whole reads start further left, so lenDiff is their extra length."""
    name, n = "C.part.%s.%s" % (shape, "LR"[side]), 70
    part, whole, is_part = PART_SHAPES[shape]
    qlen = lambda ops: sum(k for k, op in ops if op in "MIS")
    rlen = lambda ops: sum(k for k, op in ops if op in "MDN")
    ld = qlen(whole) - qlen(part)
    pidx = list(range(1, 60, 2))
    plain = [(M(C_L), 0)] * n
    if side == 0:
        spec = [((part if k in pidx else whole), 0) for k in range(n)]
    else:
        part, whole = part[::-1], whole[::-1]
        spec = [((part, rlen(whole) - rlen(part)) if k in pidx else (whole, 0)) for k in range(n)]
    left, right = (spec, plain) if side == 0 else (plain, spec)
    wcol = 10 + (ld if side == 1 and is_part else 0)            # column 10 of the template, in a whole read
    marks = [(side, 0, wcol + (ld if side == 1 and not is_part else 0), 40)]

    def premise(b):
        from oracle import oracle_py
        sp = b.spec(0, side)
        pw, ww = cigar_words(b.batch, b.read(0, side, 1)), cigar_words(b.batch, b.read(0, side, 0))
        assert oracle_py.is_part_of(pw, ww, side == 0) == is_part and not oracle_py.is_part_of(ww, pw, side == 0)
        assert sp["left_mode"] == (side == 0) and sp["n_classes"] == 2
        assert sp["template"] == (1 if is_part else 0) and len(sp["voters"]) == (70 if is_part else 40)
        assert sp["contained"][1] == (70 if is_part else 30) and sp["contained"][0] == 40
        assert set(sp["len_diff"]) == ({0, ld} if side == 1 and is_part else {0})

    def witness(b, want):
        t = b.template_read(0, side)
        col = 10 if is_part or side == 0 else 10 + ld
        assert want.out_flag[t] != 0 and out_qual(b, want, t, col) == 40 and [out_qual(b, want, t, c) for c in range(30)].count(40) == 1
        assert int(b.batch.core["l_qseq"][t]) == qlen(part if is_part else whole)

    case(name, "C", one_stream(plant_q(class_group(name, left, right), marks), seed=5), premise, (0, 0, 0, 2, 0), witness=witness)


for _s in PART_SHAPES:
    add_part(_s, 0)
    add_part(_s, 1)
def add_right_end():
    """A right side of 70 `40M` reads at two right ends (40 at p with quality 37, 30 at p + 2 with quality 38): containedBy counts them apart, the voter list
    takes both, column by column (lenDiff 0).  Where the two ends show one base the 38 comes out, elsewhere the reference arbitrates for the template's base at 37."""
    name, n = "C.right_end", 70
    left = [(M(40), 0)] * n
    right = [(M(40), 2 if k % 7 in (1, 3, 5) else 0) for k in range(n)]
    marks = [(1, k, c, 38) for k in range(n) if k % 7 in (1, 3, 5) for c in range(40)]

    def premise(b):
        sp = b.spec(0, 1)
        assert sp["n_cigars"] == 1 and sp["n_classes"] == 2 and not sp["left_mode"]
        assert sp["contained"][0] == 40 and sp["contained"][1] == 30 and sp["template"] == 0
        assert len(sp["voters"]) == 70 > sp["contained"][0] and set(sp["len_diff"]) == {0}
        a, c = b.batch.seq_of(b.read(0, 1, 0)), b.batch.seq_of(b.read(0, 1, 1))
        b.same_cols = [x == y for x, y in zip(a, c)]
        assert 5 <= sum(b.same_cols) <= 35

    def witness(b, want):
        t = b.template_read(0, 1)
        assert [out_qual(b, want, t, c) for c in range(40)] == [38 if s_ else 37 for s_ in b.same_cols]

    case(name, "C", one_stream(plant_q(class_group(name, left, right, L=40), marks), seed=6), premise, (0, 0, 0, 2, 0), witness=witness)


add_right_end()


def add_right_end_batches():
    """130 right reads of one CIGAR: 20 at right end A, then 44 at right end B (the first 64-read batch opens both classes), then 66 more at B.  B counts 110 and
    its first read (index 20) is the template; a class match that forgot the right end would count the 66 late reads to A (86 against 44)."""
    name, n = "C.right_end.batches", 130
    left = [(M(40), 0)] * n
    right = [(M(40), 0 if k < 20 else 2) for k in range(n)]

    def premise(b):
        sp = b.spec(0, 1)
        assert sp["n_cigars"] == 1 and sp["n_classes"] == 2 and not sp["left_mode"]
        assert sp["contained"][0] == 20 and sp["contained"][20] == 110 == sp["contained"][129] and sp["template"] == 20 and len(sp["voters"]) == n

    def witness(b, want):
        assert want.out_flag[b.read(0, 1, 20)] != 0 and want.out_flag[b.read(0, 1, 0)] == 0

    case(name, "C", one_stream(class_group(name, left, right, L=40), seed=21), premise, (0, 0, 0, 2, 0), witness=witness)


add_right_end_batches()


def add_absent():
    """One-read pairs: the right read is missing at indices 0, 63, 64 and np - 1 (firstRead is not index 0; a lone read of a name is its pair's LEFT read,
    Cluster::addRead, so only right reads can be absent)."""
    name, n = "C.absent", 257
    left = [(M(C_L), 0)] * n
    right = [None if k in (0, 63, 64, n - 1) else (M(C_L), 0) for k in range(n)]
    marks = [(1, n - 2, 16, 40)]

    def premise(b):
        r = b.spec(0, 1)
        assert r["template"] == 1 and [r["contained"][k] for k in (0, 63, 64, n - 1)] == [0] * 4 and len(r["voters"]) == n - 4 == r["contained"][1]
        assert b.st.reads_of(0, 1)[0] is None

    def witness(b, want):
        assert out_qual(b, want, b.template_read(0, 1), 16) == 40

    case(name, "C", one_stream(plant_q(class_group(name, left, right), marks), seed=7), premise, (0, 0, 0, 2, 0), witness=witness)


add_absent()


def add_tiebreak(short_at, n=300):
    """Equal containedBy everywhere: 300 reads of `100M` but for three `95M` reads at `short_at` -- every read is contained by all (a 95M read by every read, a
    100M read by the 297 of its kind).  The 95M reads have the most, and the FIRST of them is the template; with short_at None every count is equal and read 0
    is the template (first in qname order)."""
    name = "C.tiebreak.%s" % ("none" if short_at is None else "-".join(map(str, short_at)))
    sa = short_at or ()
    left = [((M(95) if k in sa else M(C_L)), 0) for k in range(n)]
    right = [(M(C_L), 0)] * n

    def premise(b):
        sp = b.spec(0, 0)
        if sa:
            assert all(sp["contained"][k] == n for k in sa) and sp["contained"][0 if 0 not in sa else 1] == n - 3
            assert sp["template"] == sa[0]
        else:
            assert set(sp["contained"]) == {n} and sp["template"] == 0
        assert len(sp["voters"]) == n

    def witness(b, want):
        t = b.template_read(0, 0)
        assert want.out_flag[t] != 0 and all(want.out_flag[b.read(0, 0, k)] == 0 for k in range(n) if b.read(0, 0, k) != t)

    case(name, "C", one_stream(class_group(name, left, right), seed=8), premise, (0, 0, 0, 2, 0), witness=witness)


for _sa in (None, (0, 63, 64), (63, 64, 255), (64, 255, 256), (255, 256, 257), (256, 257, 299), (257, 298, 299)):
    add_tiebreak(_sa)


def add_tiebreak_shorter(first_short, side=0):
    """Two classes of 150 reads that do not contain one another, `60M5S` (65 bases) and `50M9S` (59 bases), interleaved: equal containedBy (150) at different
    lengths -- the shorter read wins wherever it stands; first_short: the 59-base class holds index 0 (else the 65-base class does).  Right side: `5S60M` /
    `9S50M` at one right end."""
    name, n = "C.tiebreak.shorter.%s%s" % ("first" if first_short else "second", ".R" if side else ""), 300
    a, c = [(60, "M"), (5, "S")], [(50, "M"), (9, "S")]
    plain = [(M(C_L), 0)] * n
    if side == 0:
        spec = [((c if (k % 2 == 0) == first_short else a), 0) for k in range(n)]
    else:
        spec = [((c[::-1], 10) if (k % 2 == 0) == first_short else (a[::-1], 0)) for k in range(n)]
    left, right = (spec, plain) if side == 0 else (plain, spec)

    def premise(b):
        sp = b.spec(0, side)
        assert set(sp["contained"]) == {150} and sp["template"] == (0 if first_short else 1) and len(sp["voters"]) == 150
        assert int(b.batch.core["l_qseq"][b.template_read(0, side)]) == 59 and sp["left_mode"] == (side == 0)

    case(name, "C", one_stream(class_group(name, left, right), seed=9), premise, (0, 0, 0, 2, 0))


add_tiebreak_shorter(True)
add_tiebreak_shorter(False)
add_tiebreak_shorter(True, 1)
add_tiebreak_shorter(False, 1)


# ============================================================================================================ family T: the three thresholds
FIVE40 = [(3, "S"), (15, "M"), (1, "D"), (19, "M"), (3, "S")]


def add_majority(n, nmaj, thr_on, pairwise, neighbour=None):
    """n pairs; the left side holds nmaj reads `100M` and single reads with soft-clip tails: best containedBy = nmaj against 0.4 n."""
    name = "T.majority.np%d.%d.%s.%s" % (n, nmaj, "on" if thr_on else "off", "pairwise" if pairwise else "classes")
    left = [(M(C_L), 0) if k < nmaj else (tail_clip(k - nmaj + 1), 0) for k in range(n)]
    if pairwise:
        left[n - 1] = ([(5, "S"), (40, "M"), (2, "D"), (50, "M"), (5, "S")], 0)
    right = [(M(C_L), 0)] * n
    has = nmaj >= 0.4 * n

    def premise(b):
        sp = b.spec(0, 0)
        assert max(sp["contained"]) == nmaj and (sp["template"] is not None) == has and sp["max_ops"] == (5 if pairwise else 2)
        assert sp["reason"] == (None if has else "no majority") and (n > b.prm.skip_low_complexity_cluster_threshold) == thr_on
        assert sp["diff_neighbor"] >= 50 and max(sp["contained"]) < n // 2           # neither the low-complexity skip nor the early break is in play

    def witness(b, want):
        em = [want.out_flag[r] != 0 for r in b.st.reads_of(0, 0)]
        assert sum(em) == (1 if has else 0)                                         # no template: the molecule is written from its right read alone
        assert sum(want.out_flag[r] != 0 for r in b.st.reads_of(0, 1)) == 1

    case(name, "T", one_stream(class_group(name, left, right), seed=n, skip=n - 1 if thr_on else n), premise,
         (0, 0, 0, 2, 0) if has else (0, 0, 1, 1, 0), witness=witness, neighbour=neighbour, combine=False)
    return name


for _on in (True, False):
    for _pw in (False, True):
        add_majority(65, 26, _on, _pw, neighbour=add_majority(65, 25, _on, _pw))
        add_majority(70, 28, _on, _pw, neighbour=add_majority(70, 27, _on, _pw))


def add_early_break(thr_on, pairwise, neighbour=None):
    """65 pairs: 32 reads `100M` (read 0 first) and 33 reads `90M` (pairwise: 32, and one 5-op read).  Read 0 is contained by exactly 32 = 65 / 2: with the
    threshold on the walk stops there (`>=`) and read 0 is the template; off, a `90M` read (contained by all) is."""
    name, n = "T.early_break.%s.%s" % ("on" if thr_on else "off", "pairwise" if pairwise else "classes"), 65
    left = [((M(C_L) if k % 2 == 0 and k < 64 else M(90)), 0) for k in range(n)]
    if pairwise:
        left[n - 1] = ([(5, "S"), (40, "M"), (2, "D"), (50, "M"), (5, "S")], 0)
    right = [(M(C_L), 0)] * n
    nw = 32

    def premise(b):
        sp = b.spec(0, 0)
        assert sp["n_cigars"] == 2 + pairwise and sp["n_cigars"] <= 0.1 * n
        if thr_on:
            assert sp["contained"][0] == nw == n // 2 and set(sp["contained"][1:]) == {0} and sp["template"] == 0 and len(sp["voters"]) == nw
        else:
            assert sp["contained"][1] == n - pairwise > sp["contained"][0] == nw and sp["template"] == 1 and len(sp["voters"]) == n - pairwise

    def witness(b, want):
        assert want.out_flag[b.template_read(0, 0)] != 0

    case(name, "T", one_stream(class_group(name, left, right), seed=65, skip=n - 1 if thr_on else n), premise, (0, 0, 0, 2, 0), witness=witness,
         neighbour=neighbour, combine=False)
    return name


for _pw in (False, True):
    add_early_break(True, _pw, neighbour=add_early_break(False, _pw))


def low_seq(dn):
    """40 bases with exactly dn differing neighbours (dn <= 39)."""
    s = ["A"]
    for i in range(39):
        s.append(lc.alt(s[-1]) if i < dn else s[-1])
    return s


def add_lowc(ncig, dn, side, neighbour=None, two_ends=False, pairwise=False, thr_on=True):
    """70 pairs of 40-base reads: ncig distinct CIGAR strings on `side` against 0.1 * 70 = 7 (strict), the side's first read (a class of its own) with dn
    differing neighbours against 0.5 * 40 = 20; the threshold on (69) or off (70).  two_ends (right side): one more class that repeats a CIGAR at another right
    end.  pairwise: one of the distinct CIGARs has five ops -- side_prepare counts the strings and the neighbours in its pairwise code."""
    name, n = "T.lowc.%s.cig%d.dn%d%s%s%s" % ("LR"[side], ncig, dn, ".two_ends" if two_ends else "", ".pairwise" if pairwise else "", "" if thr_on else ".off"), 70
    mk = (lambda k: (tail_clip(k, 40), 0)) if side == 0 else (lambda k: (head_clip(k, 40), k))
    ns = ncig - 1 - pairwise
    spec = [mk(k + 1) if k < ns else (M(40), 0) for k in range(n)]
    if pairwise:
        spec[ns] = (FIVE40, 0 if side == 0 else 5)             # (right side: 5 + 35 reference bases, the common right end)
    if two_ends:
        spec[n - 1] = (M(40), 2)
    other = [(M(40), 0)] * n
    left, right = (spec, other) if side == 0 else (other, spec)

    def build(ref, rng, drop_at):
        g = class_group(name, left, right, L=40)(ref, rng, drop_at)
        r = (g.left, g.right)[side][0]
        r.seq = low_seq(dn)
        r.nm = 30
        return g
    skipped = thr_on and ncig > 7 and dn < 20

    def premise(b):
        sp = b.spec(0, side)
        assert (n > b.prm.skip_low_complexity_cluster_threshold) == thr_on
        assert sp["n_cigars"] == ncig and sp["diff_neighbor"] == dn and sp["n_classes"] == ncig + two_ends and sp["max_ops"] == (5 if pairwise else 2)
        assert (sp["reason"] == "low complexity") == skipped and (sp["template"] is None) == skipped
        if not skipped:
            assert sp["template"] == ncig - 1 and sp["contained"][ncig - 1] == n - (ncig - 1) - two_ends

    def witness(b, want):
        assert sum(want.out_flag[r] != 0 for r in b.st.reads_of(0, side)) == (0 if skipped else 1)

    case(name, "T", one_stream(build, seed=70, skip=69 if thr_on else 70), premise, (0, 0, 1, 1, 0) if skipped else (0, 0, 0, 2, 0), witness=witness,
         neighbour=neighbour, combine=False)
    return name


for _pw in (False, True):
    _sk = add_lowc(8, 19, 0, pairwise=_pw)
    add_lowc(7, 19, 0, neighbour=_sk, pairwise=_pw)
    add_lowc(8, 20, 0, neighbour=_sk, pairwise=_pw)
    add_lowc(8, 19, 0, neighbour=_sk, pairwise=_pw, thr_on=False)
    _sk = add_lowc(8, 19, 1, pairwise=_pw)
    add_lowc(7, 19, 1, neighbour=_sk, two_ends=True, pairwise=_pw)
    add_lowc(8, 19, 1, neighbour=_sk, pairwise=_pw, thr_on=False)


# ============================================================================================================ family A: alignment
def add_left_mode(kind):
    """A right side of 70: `40M` reads at p, and (last / first) one `38M` read at p + 2 with the same right end.  Any two positions make the side right-aligned:
    the 38M read is the template (part of every 40M read from the right end) and every other voter has lenDiff 2."""
    name, n = "A.left_mode.%s" % kind, 70
    odd = {"equal": None, "last": n - 1, "first": 0}[kind]
    left = [(M(40), 0)] * n
    right = [((M(38), 2) if k == odd else (M(40), 0)) for k in range(n)]
    wk = 35
    marks = [(1, wk, 2, 40), (1, wk, 1, 41)] if odd is not None else [(1, wk, 2, 40)]

    def premise(b):
        sp = b.spec(0, 1)
        assert sp["left_mode"] == (odd is None) and sp["template"] == (0 if odd is None else odd) and len(sp["voters"]) == n
        assert sp["len_diff"] == ([0] * n if odd is None else [0] + [2] * (n - 1))

    def witness(b, want):
        t = b.template_read(0, 1)
        assert out_qual(b, want, t, 2 if odd is None else 0) == 40 and 41 not in [out_qual(b, want, t, c) for c in range(38)]

    case(name, "A", one_stream(plant_q(class_group(name, left, right, L=40), marks), seed=11), premise, (0, 0, 0, 2, 0), witness=witness)


for _k in ("equal", "last", "first"):
    add_left_mode(_k)

LONGER = (1, 2, 15, 16, 17, 31, 33)


def add_longer():
    """Seven groups of 70: 35 right reads of 40 bases and 35 longer by d, right ends equal.  The witness voter (the last, longer) shows 40 in the first and the last
    column it shares with the template (its columns d and 39 + d), 41 one column in front of the first and 42 one behind it."""
    name, n = "A.longer", 70
    builders = []
    for d in LONGER:
        left = [(M(40), 0)] * n
        right = [((M(40 + d), -d) if k % 2 else (M(40), 0)) for k in range(n)]
        marks = [(1, n - 1, d, 40), (1, n - 1, 39 + d, 40), (1, n - 1, d - 1, 41), (1, n - 1, d + 1, 42)]
        builders.append(plant_q(class_group("%s.%d" % (name, d), left, right, L=40), marks))

    def premise(b):
        for gi, d in enumerate(LONGER):
            sp = b.spec(gi, 1)
            assert not sp["left_mode"] and sp["template"] == 0 and len(sp["voters"]) == n and sp["len_diff"] == [0 if k % 2 == 0 else d for k in range(n)]
        assert {d % 2 for d in LONGER} == {0, 1}

    def witness(b, want):
        for gi, d in enumerate(LONGER):
            t = b.template_read(gi, 1)
            assert [out_qual(b, want, t, c) for c in range(40)] == [40, 42] + [37] * 37 + [40], d

    case(name, "A", one_stream(builders, seed=12), premise, (0, 0, 0, 14, 0), witness=witness)


add_longer()


def add_contig_end():
    """70 pairs whose right template ends on its contig's last base, one short of it, one past it, and on a contig the reference lacks: every right read shows one
    base that is not the reference's in its last two columns at quality 19 (unanimous, the reference arbitrates where getData gives it: only one short of the end)."""
    name, n, L = "A.contig_end", 70, 40
    shapes = (("last", 0, True), ("short", -1, True), ("past", 1, True), ("noref", 0, False))
    builders = []
    for nm_, delta, has_ref in shapes:
        def build(ref, rng, drop_at, nm_=nm_, delta=delta, has_ref=has_ref):
            g = lc.new_group("%s.%s" % (name, nm_), 2 * L + 10 - delta, 2 * L + 10, drop_at)
            g.own_contig, g.has_ref = True, has_ref
            body = ref + "ACGT"[L % 4] * max(delta, 0)
            g.left = [lc.plain_read(body, 0, L) for _ in range(n)]
            g.right = [lc.plain_read(body, L + 10, L) for _ in range(n)]
            g.names = names(n)
            for c in (L - 2, L - 1):
                for r in g.right:
                    r.seq[c] = lc.alt(r.seq[c], 2); r.qual[c] = lc.MODERATE_Q - 1; r.nm += 1
            return g
        builders.append(build)

    def premise(b):
        for gi, (nm_, delta, has_ref) in enumerate(shapes):
            g = b.st.groups[gi]
            t = b.template_read(gi, 1)
            clen = b.ref[g.tid][1] if has_ref else None
            end = int(b.batch.core["pos"][t]) + L
            assert b.spec(gi, 1)["template"] == 0 and (b.ref[g.tid][0] is not None) == has_ref
            if has_ref:
                assert end - clen == delta

    def witness(b, want):
        for gi, (nm_, delta, has_ref) in enumerate(shapes):
            t = b.template_read(gi, 1)
            flipped = [out_nib(b, want, t, c) != NIB[b.batch.seq_of(t)[c]] for c in (L - 2, L - 1)]
            assert flipped == [nm_ == "short"] * 2, (nm_, flipped)

    case(name, "A", one_stream(builders, seed=13), premise, (0, 0, 0, 8, 0), witness=witness)


add_contig_end()

SHORTER = (1, 15, 16, 17)


def add_shorter(exotic=False):
    """Negative lenDiff: a right side of 70 whose template has NO CIGAR (n_cigar 0, flag | 4).  isPartOf holds for a part without CIGAR whatever the whole is,
    and its right end is its position: placed on the common right end of the other 69 reads it is contained by all of them and is the template.  The other reads
    are 13 `40M` and 14 each of 39, 25, 24 and 23 bases: lenDiff 0, -1, -15, -16, -17; the consensus has min = 23 columns, and column i of the template meets
    column i + lenDiff of a voter -- none for i < -lenDiff (the reference reads in front of the voter there; oracle and engine skip the vote).  In k_vote_deep the
    lane of columns 0 .. 15 starts at rp0 = -1 / -15 (the bytewise path) or -16 / -17 (wholly in front of the voter), the lane of columns 16 .. 22 at 15 / 1 / 0 / -1.
    One voter of every length shows the only quality 40 of its FIRST column (the template's column 1, 15, 16, 17), and the 39- and the 23-base one 41 in
    their second.  exotic: an IUPAC nibble in the first column of a 39-base voter, met by the bytewise path alone: k_consensus_slow finishes the side."""
    name, n, L = "A.shorter%s" % (".exotic" if exotic else ""), 70, 40
    lens = [40] * 13 + [L - d for d in SHORTER for _ in range(14)]
    order = [lens[(k * 11) % 69] for k in range(69)]           # the lengths interleaved (11 and 69 are coprime)
    tpl = 35                                                     # the pair whose right read is the template
    left = [(M(L), 0)] * n
    right, it = [], iter(order)
    for k in range(n):
        if k == tpl:
            right.append((M(L), L))                              # at the others' right end; its CIGAR is taken away below
        else:
            x = next(it)
            right.append((M(x), L - x))
    wit = {d: max(k for k in range(n) if k != tpl and right[k][0][0][0] == L - d) for d in SHORTER}

    def build(ref, rng, drop_at):
        g = class_group(name, left, right, L=L)(ref, rng, drop_at)
        full = next(r for k, r in enumerate(g.right) if k != tpl and len(r.seq) == L)
        g.right[tpl].seq = list(full.seq)                        # the template shows what the 40M reads show: every column agrees
        for d, k in wit.items():
            g.right[k].qual[0] = 40
            if d in (1, 17):
                g.right[k].qual[1] = 41
        if exotic:
            k = min(k for k in range(n) if k != tpl and len(g.right[k].seq) == L - 1)
            g.right[k].seq[0] = "M"; g.right[k].nm += 1

        def post(batch, where, gi):
            r = where[(gi, 1, tpl)]
            batch.core["n_cigar"][r] = 0
            batch.core["flag"][r] |= 4
        g.post = [post]
        return g

    def premise(b):
        sp = b.spec(0, 1)
        t = b.read(0, 1, tpl)
        assert b.batch.core["n_cigar"][t] == 0 and b.batch.core["flag"][t] & 4 and cigar_words(b.batch, t) == []
        assert not sp["left_mode"] and sp["template"] == tpl and sp["contained"][tpl] == n and len(sp["voters"]) == n and sp["length"] == L - 17
        ld = dict(zip(sp["voters"], sp["len_diff"]))
        assert sorted(set(sp["len_diff"])) == [-17, -16, -15, -1, 0] and all(ld[k] == -d for d, k in wit.items())
        assert [sp["len_diff"].count(-d) for d in SHORTER] == [14] * 4
        rd = [b.read(0, 1, k) for k in sp["voters"]]
        for d, k in wit.items():                                 # the only 40 among the voters that reach the template's column d
            col = [int(b.batch.qual[int(b.batch.qual_off[r]) + d + ld[v]]) for v, r in zip(sp["voters"], rd) if 0 <= d + ld[v]]
            assert col.count(40) == 1 and sorted(col)[-2] == 37, (d, col)
        if exotic:
            assert sum(1 for r in rd if set(b.batch.seq_of(r)) - set("ACGTN")) == 1

    def witness(b, want):
        t = b.read(0, 1, tpl)
        got = [out_qual(b, want, t, c) for c in range(L - 17)]
        exp = [37] * (L - 17)
        for d in SHORTER:
            exp[d] = 40
        exp[2] = exp[18] = 41
        assert want.out_flag[t] != 0 and got == exp, got

    case(name, "A" if not exotic else "X", one_stream(build, seed=31), premise, (0, 0, 0, 1, 1) if exotic else (0, 0, 0, 2, 0), witness=None if exotic else witness)


add_shorter()
add_shorter(exotic=True)


# ============================================================================================================ family O: mate overlap
def windows():
    """Overlap windows [s, e) of a 40-base left read: starts and ends at columns 3, 4, 5, 15, 16, 17, lengths 1 .. 40, odd and even starts."""
    edges = (3, 4, 5, 15, 16, 17)
    w = [(s, e) for s in edges for e in edges + (40,) if e > s]
    w += [(40 - k, 40) for k in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 40)]
    w += [(0, k) for k in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17)]
    return w


def add_windows(n):
    """n pairs; pair k's right read covers columns [s, e) of its left read (windows()[k mod], the template's the first).  In EVERY column the voters are split
    between the two bases that are not the reference's so that the two score sums (12 inside a voter's window, 8 outside) are equal or 4 apart: one voter's
    window taken one column too wide or too narrow moves a sum by 4 and changes the base that comes out (equal sums: the later bin)."""
    name, L = "O.windows.np%d" % n, 40
    W = windows()

    def build(ref, rng, drop_at):
        g = lc.new_group(name, L, 40, drop_at)              # every right read ends inside the left read's span: isize = 40
        g.names = names(n)
        cover = np.zeros((n, L), bool)
        for k in range(n):
            s, e = W[k % len(W)]
            cover[k, s:e] = True
        base = np.zeros((n, L), int)
        for c in range(L):                                   # a0 covering and b0 non-covering voters on the earlier bin: the split with the smallest |difference|
            ca, cb = np.nonzero(cover[:, c])[0], np.nonzero(~cover[:, c])[0]
            a, bb = len(ca), len(cb)
            _, a0, b0 = min((abs(12 * (2 * x - a) + 8 * (2 * y - bb)), x, y) for x in range(a // 2 - 2, a // 2 + 3) for y in range(bb // 2 - 3, bb // 2 + 4)
                            if 0 <= x <= a and 0 <= y <= bb)
            for grp, k0 in ((ca, a0), (cb, b0)):
                order = list(grp[0::2]) + list(grp[1::2])    # (interleaved, so that the earlier bin's voters spread over waves and chunks)
                base[order[k0:], c] = 1
        g.left, g.right = [], []
        for k in range(n):
            s, e = W[k % len(W)]
            seq = [sorted((x for x in "ACGT" if x != ref[c]), key=lambda x: NIB[x])[base[k, c]] for c in range(L)]
            g.left.append(lc.Read(0, "40M", seq, [37] * L, nm=L))
            g.right.append(lc.Read(s, "%dM" % (e - s), seq[s:e], [37] * (e - s), nm=e - s))
        return g

    def premise(b):
        sp = b.spec(0, 0)
        assert sp["template"] == 0 and len(sp["voters"]) == n
        score = np.full((n, L), 8)
        bases = np.zeros((n, L), int)
        seen = set()
        for k in range(n):
            l, r = b.read(0, 0, k), b.read(0, 1, k)
            s = int(b.batch.core["pos"][r]) - int(b.batch.core["pos"][l])
            e = s + int(b.batch.core["l_qseq"][r])
            assert b.batch.seq_of(l)[s:e] == b.batch.seq_of(r)
            score[k, s:e] = 12
            seen.add((s, e))
            bases[k] = [NIB[x] for x in b.batch.seq_of(l)]
        assert seen == set(windows()) and {e - s for s, e in seen} >= {1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 40}
        for c in range(L):
            lo, hi = sorted(set(bases[:, c]))
            d = score[bases[:, c] == lo, c].sum() - score[bases[:, c] == hi, c].sum()
            assert abs(d) <= 4, (c, d)
        b.expect_cols = []
        for c in range(L):                                   # the larger score sum; equal: the larger quality sum (37 a vote); equal again: the later bin
            lo, hi = sorted(set(bases[:, c]))
            key = lambda x: (score[bases[:, c] == x, c].sum(), (bases[:, c] == x).sum(), x)
            b.expect_cols.append(max((lo, hi), key=key))
        ties = sum(1 for c in range(L) if len({score[bases[:, c] == x, c].sum() for x in set(bases[:, c])}) == 1)
        assert 5 <= ties <= L - 5                            # both kinds of column: equal sums, and sums 4 apart

    def witness(b, want):
        t = b.template_read(0, 0)
        assert [out_nib(b, want, t, c) for c in range(L)] == b.expect_cols

    case(name, "O", one_stream(build, seed=n), premise, (0, 0, 0, 2, 0), witness=witness)


add_windows(70)
add_windows(300)


def add_mate_mismatch(mismatch, neighbour=None):
    """70 pairs that overlap in columns [24, 40) of the left read; in the first and the last overlap column 56 voters show base X and 14 the reference's, all at
    score 12 (672 = 0.8 * 840: X stays).  mismatch: voter 8's mate shows the reference's base there at quality 10 -- its own quality is rewritten to 27 and its
    score to 6 - 3 (663 < 0.8 * 831): the reference's base comes out."""
    name, n, L, dis = "O.mate_mismatch.%s" % ("yes" if mismatch else "no"), 70, 40, 24
    cols = (dis, L - 1)

    def build(ref, rng, drop_at):
        g = lc.new_group(name, dis + L, dis + L, drop_at)
        g.names = names(n)
        g.left = [lc.plain_read(ref, 0, L) for _ in range(n)]
        g.right = [lc.plain_read(ref, dis, L) for _ in range(n)]
        for k in range(n):
            if k % 5 != 4:                                   # 56 of 70
                for c in cols:
                    x = lc.alt(ref[c])
                    set_base(g.left[k], c, x, ref[c])
                    if not (mismatch and k == 8):
                        set_base(g.right[k], c - dis, x, ref[c])
                    else:
                        g.right[k].qual[c - dis] = 10
        return g

    def premise(b):
        sp = b.spec(0, 0)
        assert sp["template"] == 0 and len(sp["voters"]) == n
        for c in cols:
            lb = [b.batch.seq_of(b.read(0, 0, k))[c] for k in range(n)]
            rb = [b.batch.seq_of(b.read(0, 1, k))[c - dis] for k in range(n)]
            assert lb.count(lb[0]) == 56 and [k for k in range(n) if lb[k] != rb[k]] == ([8] if mismatch else [])

    def witness(b, want):
        t = b.template_read(0, 0)
        for c in cols:
            assert (out_nib(b, want, t, c) == NIB[b.batch.seq_of(t)[c]]) == (not mismatch)
        if mismatch:                                         # the in-place rewrite of the voter that is not written
            v = b.read(0, 0, 8)
            assert [out_qual(b, want, v, c) for c in cols] == [27, 27]

    case(name, "O", one_stream(build, seed=14), premise, (0, 0, 0, 2, 0), witness=witness, neighbour=neighbour)
    return name


add_mate_mismatch(True, neighbour=add_mate_mismatch(False))


def add_lost_mates(nlost, neighbour=None):
    """70 pairs, mates apart; column 5: 56 voters show base X (score 8), 14 the reference's.  nlost of the 56 have no mate: GCE_PATCH_CONST, score_moderate = 6
    for every base.  X stays while 8 (56 - nlost) + 6 nlost >= 0.8 x the total: with no mate lost (448 = 0.8 x 560), not with one (446 < 0.8 x 558)."""
    name, n, col = "O.lost_mates.%d" % nlost, 70, 5

    def fill(g, ref, rng):
        lost = 0
        for k in range(n):
            if k % 5 != 4:
                set_base(g.left[k], col, lc.alt(ref[col]), ref[col])
                if k > 0 and lost < nlost:
                    g.right[k] = None
                    lost += 1

    keeps = (8 * (56 - nlost) + 6 * nlost) >= 0.8 * (8 * (56 - nlost) + 6 * nlost + 8 * 14)

    def premise(b):
        sp = b.spec(0, 0)
        assert sp["template"] == 0 and len(sp["voters"]) == n and b.st.reads_of(0, 1).count(None) == nlost
        lb = [b.batch.seq_of(b.read(0, 0, k))[col] for k in range(n)]
        assert lb.count(lb[0]) == 56 and all(lb[k] == lb[0] for k in range(n) if b.st.reads_of(0, 1)[k] is None)

    def witness(b, want):
        t = b.template_read(0, 0)
        assert (out_nib(b, want, t, col) == NIB[b.batch.seq_of(t)[col]]) == keeps

    case(name, "O", one_stream(plain_group(name, n)(fill), seed=15), premise, (0, 0, 0, 2, 0), witness=witness, neighbour=neighbour)
    return name, keeps


# 8 * 56 = 448 = 0.8 * 560 with no mate lost: X stays; one lost mate: 446 < 0.8 * 558
add_lost_mates(1, neighbour=add_lost_mates(0)[0])
add_lost_mates(5)


def add_maxu(ov):
    """70 pairs of 168-base reads that overlap in `ov` columns: 21 units of 8 bases each, 64 x 21 = 1344 > SC2_MAXU in the first wave of k_score2 whichever 64
    pairs it holds -- two rounds, one pair astride the cut.  Every left read shows quality 40 in three overlap columns of its own (units 0, 10 and the last) where
    its mate disagrees at quality 10: computeScore rewrites the 40 to 30 in place, and the column's top quality comes out as 37 -- a unit that is not scored
    leaves a 40."""
    name, n, L = "O.maxu.ov%d" % ov, 70, 168
    dis = L - ov

    def cols_of(k):
        return sorted({dis + 8 * u + (k % 8 if 8 * u + k % 8 < ov else ov - 1 - 8 * u) for u in (0, 10, (ov - 1) // 8)})

    def build(ref, rng, drop_at):
        g = lc.new_group(name, dis + L, dis + L, drop_at)
        g.names = names(n)
        g.left = [lc.plain_read(ref, 0, L) for _ in range(n)]
        g.right = [lc.plain_read(ref, dis, L) for _ in range(n)]
        for k in range(n):
            for c in cols_of(k):
                g.left[k].qual[c] = 40
                set_base(g.right[k], c - dis, lc.alt(ref[c]), ref[c])
                g.right[k].qual[c - dis] = 10
        return g

    def premise(b):
        assert (ov + 7) // 8 == 21 and 64 * 21 > SC2_MAXU and (ov % 8 == 0) == (ov == 168)
        for k in range(n):
            l, r = b.read(0, 0, k), b.read(0, 1, k)
            assert int(b.batch.core["pos"][r]) - int(b.batch.core["pos"][l]) == dis
            q = b.batch.qual_of(l)
            assert [c for c in range(L) if q[c] == 40] == cols_of(k) and min(cols_of(k)) >= dis
        assert {(c - dis) // 8 for k in range(n) for c in cols_of(k)} == {0, 10, 20}

    def witness(b, want):
        t = b.template_read(0, 0)
        assert set(out_qual(b, want, t, c) for c in range(L)) == {37}
        for k in range(1, n):
            assert [out_qual(b, want, b.read(0, 0, k), c) for c in cols_of(k)] == [30] * len(cols_of(k))

    case(name, "O", one_stream(build, seed=16), premise, (0, 0, 0, 2, 0), witness=witness)


add_maxu(168)
add_maxu(163)


# ============================================================================================================ family X: back-outs, restore, errors
def add_exotic():
    """Six groups of 70: an IUPAC nibble in the template, in a voter at columns 3 / 4 / 15 / 16, and a quality of 200 in a voter: k_vote_deep backs the left side
    out with nothing written and k_consensus_slow finishes it; the right sides stay."""
    name, n = "X.exotic", 70
    shapes = (("tmpl", 0, 7, "M"), ("v3", 33, 3, "R"), ("v4", 34, 4, "M"), ("v15", 35, 15, "K"), ("v16", 69, 16, "M"), ("q200", 36, 16, None))
    builders = []
    for tag, k, c, ch in shapes:
        def fill(g, ref, rng, k=k, c=c, ch=ch):
            if ch:
                g.left[k].seq[c] = ch; g.left[k].nm += 1
            else:
                g.left[k].qual[c] = 200
        builders.append(plain_group("%s.%s" % (name, tag), n)(fill))

    def premise(b):
        for gi, (tag, k, c, ch) in enumerate(shapes):
            r = b.read(gi, 0, k)
            assert (b.batch.seq_of(r)[c] == ch) if ch else (b.batch.qual_of(r)[c] == 200)
            assert b.spec(gi, 0)["template"] == 0 and k in b.spec(gi, 0)["voters"]

    case(name, "X", one_stream(builders, seed=17), premise, (0, 0, 0, 6, 6))


add_exotic()


def add_masked_byte():
    """A deep group of 38-base reads (a voter ends inside a 4-column group) in front of a two-pair group whose first read opens with quality 200: the byte behind the
    LAST right read of the deep group in the quality blob is that 200.  The deep side stays in k_vote_deep (the `vm` mask)."""
    name, n, L = "X.masked_byte", 70, 38

    def fill2(g, ref, rng):
        g.left[0].qual[0] = 200

    def premise(b):
        last = b.read(0, 1, n - 1)
        nxt = b.read(1, 0, 0)
        assert nxt == last + 1 and int(b.batch.qual_off[nxt]) == int(b.batch.qual_off[last]) + L and L % 4 == 2
        assert b.batch.qual[int(b.batch.qual_off[last]) + L] == 200 and b.spec(0, 1)["voters"][-1] == n - 1

    case(name, "X", one_stream([plain_group(name, n, L)(lambda g, ref, rng: None), plain_group(name + ".two", 2, L)(fill2)], seed=18), premise,
         (0, 1, 0, 2, 1))              # the two-pair group: k_vote hands it on, k_consensus_fast takes its right side and leaves the left to k_consensus_slow


add_masked_byte()


def add_minc(tag, ncols, nm=0, nm_type="C", patched=None, error=0, neighbour=None):
    """70 pairs; in ncols columns the template shows the reference's base and the 69 other voters another: the columns flip, mismatchInc = ncols."""
    name, n = "X.minc.%s" % tag, 70
    cols = (2, 9, 16, 23, 30, 37)[:ncols]

    def fill(g, ref, rng):
        for r in g.left[1:]:
            for c in cols:
                set_base(r, c, lc.alt(ref[c]), ref[c])
        g.left[0].nm = nm

        def post(batch, where, gi):
            batch.nm_type[where[(gi, 0, 0)]] = ord(nm_type) if nm_type else 0
        g.post = [post]

    def premise(b):
        t = b.template_read(0, 0)
        assert b.spec(0, 0)["template"] == 0 and b.batch.nm[t] == nm and b.batch.nm_type[t] == (ord(nm_type) if nm_type else 0)
        ts = b.batch.seq_of(t)
        assert [c for c in range(40) if b.batch.seq_of(b.read(0, 0, 1))[c] != ts[c]] == list(cols)

    def witness(b, want):
        t = b.template_read(0, 0)
        if error:
            assert want.status == error
            return
        flipped = [c for c in range(40) if out_nib(b, want, t, c) != NIB[b.batch.seq_of(t)[c]]]
        assert flipped == ([] if ncols > 5 else list(cols)) and want.nm_new[t] == (patched if patched is not None else -1)

    case(name, "X", one_stream(plain_group(name, n)(fill), seed=19), premise, (0, 0, 0, 2, 0), witness=witness, error=error, neighbour=neighbour,
         combine=not error)
    return name


add_minc("six", 6, neighbour=add_minc("five", 5, patched=5))
add_minc("nmS", 5, nm_type="S")
add_minc("nmi", 5, nm_type="i")
add_minc("nm251", 5, nm=251, neighbour=add_minc("nm250", 5, nm=250, patched=255))
add_minc("missing", 5, nm_type=None, error=GCE_ERR_NM_MISSING)


# ------------------------------------------------------------------------------------------------------------ the combined stream
def combined_stream(flush_period=500):
    """Every case with default parameters and no error in ONE stream (the threshold cases and the score-constant case need parameters of their own), flushed
    every 500 reads: sides of all sizes meet in one k_deep_prepare / k_vote_deep launch."""
    st = DeepStream(seed=99, flush_period=flush_period)
    for c in CASES.values():
        if c.combine and not c.error:
            one = c.make()
            for b, tag in one.items:
                st.items.append((b, (c.name, 0)))
    return st


def combined_routing():
    tot = [0] * 5
    for c in CASES.values():
        if c.combine and not c.error:
            tot = [a + b for a, b in zip(tot, c.routing)]
    return tuple(tot)
