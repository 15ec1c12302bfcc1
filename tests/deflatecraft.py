"""A deflate writer for tests (RFC 1951 inside the BGZF framing of SAM spec 4.1): the caller chooses every field of every block, so that
the streams zlib never writes -- 15-bit codes, 48-bit symbols, a lone distance code, repeats that run from the literal lengths into the
distance lengths, stored blocks at every bit phase -- and the damaged ones exist as named members.  Written from the RFC alone: nothing
here is shared with the decoders it feeds (gce_inflate.hpp, gce_bgzf.hpp); zlib judges the catalogue (test_deflatecraft.py).

    cases()    -> [(name, member bytes, usize to declare, expected bytes or None)]
    records()  -> {name: the builder's notes: what was written at which bit and at which output position}
"""
import struct
import zlib

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CLEXT = {16: 2, 17: 3, 18: 7}
EOB = 256
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FIXED_LIT = {s: (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s in range(288)}
FIXED_DIST = {s: 5 for s in range(32)}


class BitWriter:
    """bits go into each byte from its least significant end; a Huffman code goes in with its most significant bit first"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code_len):
        code, n = code_len
        for k in range(n - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: length} -> {symbol: (code, length)} by the algorithm of RFC 1951 3.2.2.  The set is taken as it is: an incomplete one leaves
    codes unused, an over-subscribed one wraps (the code is cut to its length) -- both are the caller's business."""
    count = [0] * 17
    for ln in lengths.values():
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s in sorted(lengths):
        ln = lengths[s]
        if ln:
            out[s] = (nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def flat_lengths(symbols):
    """a complete code over >= 2 symbols with lengths as equal as they can be"""
    syms = sorted(set(symbols))
    k = len(syms)
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    return {s: (m - 1 if i < short else m) for i, s in enumerate(syms)}


def kraft(lengths):
    """sum of 2^-length in units of 2^-15: 32768 for a complete set"""
    return sum(1 << (15 - ln) for ln in lengths.values() if ln)


def match(length, dist, alt258=False):
    """(length symbol, extra, distance symbol, extra) of a match; alt258: length 258 spelt as symbol 284 with extra 31"""
    if length == 258 and alt258:
        ls, lx = 284, 31
    elif length == 258:
        ls, lx = 285, 0
    else:
        i = max(k for k in range(28) if LBASE[k] <= length)
        ls, lx = 257 + i, length - LBASE[i]
        assert lx < (1 << LEXT[i])
    d = max(k for k in range(30) if DBASE[k] <= dist)
    assert dist - DBASE[d] < (1 << DEXT[d])
    return (ls, lx, d, dist - DBASE[d])


def rle(seq):
    """a sequence of code lengths -> code-length symbols [(symbol, extra)], greedily with 16, 17 and 18"""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138); out.append((18, r - 11)); run -= r
            if run >= 3:
                out.append((17, run - 3)); run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                r = min(run, 6); out.append((16, r - 3)); run -= r
            out += [(v, 0)] * run
        i = j
    return out


def _two(symbols):
    """the set, with 0 and then 1 joining it while it has fewer than two members (a complete code needs two)"""
    u = set(symbols)
    for s in (0, 1):
        if len(u) < 2:
            u.add(s)
    return u


def plain(seq):
    return [(v, 0) for v in seq]


class Deflate:
    """one raw-deflate stream, block by block.  `out` is what the tokens written so far mean; it stops growing at the first token that means
    nothing (a distance beyond the start, a symbol that is no symbol): `broken`.  `notes` says where things went:
    ("block", type, bit position, output position), ("match", bit position, bits of the whole token, output position, length, distance,
    bits of its two codes), ("bad", output position, the bytes the token would have added had it meant something)."""

    def __init__(self):
        self.w, self.out, self.notes, self.broken = BitWriter(), bytearray(), [], False

    def _break(self, need):
        if not self.broken:
            self.notes.append(("bad", len(self.out), need))
        self.broken = True

    def header(self, final, btype):
        self.notes.append(("block", btype, self.w.bitpos, len(self.out)))
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, ln=None, nlen=None, body=None):
        """ln, nlen: the LEN and NLEN fields when they are not to be the truth; body: the bytes that follow them when not `data`"""
        self.header(final, 0)
        self.w.align()
        ln = len(data) if ln is None else ln
        self.w.bits(ln, 16)
        self.w.bits(ln ^ 0xFFFF if nlen is None else nlen, 16)
        self.w.raw(data if body is None else body)
        if not self.broken:
            self.out += data
        return self

    def tokens(self, toks, lit, dist):
        w = self.w
        for t in toks:
            if isinstance(t, int):                                                   # a literal, end-of-block, or a length symbol left bare (286, 287)
                w.code(lit[t])
                if t < 256 and not self.broken:
                    self.out.append(t)
                elif t > 256:
                    self._break(3)
                continue
            ls, lx, ds, dx = t
            at = w.bitpos
            w.code(lit[ls])
            w.bits(lx, LEXT[ls - 257])
            if ds is not None:                                                       # (None: the set has no distance code to write)
                w.code(dist[ds])
                w.bits(dx, DEXT[ds] if ds < 30 else 0)
            length = LBASE[ls - 257] + lx
            distance = DBASE[ds] + dx if ds is not None and ds < 30 else None
            self.notes.append(("match", at, w.bitpos - at, len(self.out), length, distance, lit[ls][1], dist[ds][1] if ds is not None else 0))
            if distance is None or distance > len(self.out):
                self._break(length)
            if not self.broken:
                for _ in range(length):
                    self.out.append(self.out[-distance])

    def fixed(self, toks, final=False):
        self.header(final, 1)
        self.tokens(toks, canonical(FIXED_LIT), canonical(FIXED_DIST))
        return self

    def dynamic(self, toks, lit_lens=None, dist_lens=None, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, cl_syms=None):
        """lit_lens, dist_lens: {symbol: length}; default: a complete set over what the tokens use (two distance codes at least).
        hlit, hdist, hclen: the counts the header declares; default: the smallest that hold the sets.
        cl_syms: the code-length symbols [(symbol, extra)] that spell the hlit + hdist lengths; default: rle() of them.
        cl_lens: the code-length code's own lengths, or a function of the default ones; default: complete over what cl_syms uses."""
        used_l = {t if isinstance(t, int) else t[0] for t in toks} | {EOB}
        used_d = {t[2] for t in toks if not isinstance(t, int) and t[2] is not None}
        if lit_lens is None:
            lit_lens = flat_lengths(_two(used_l))
        if dist_lens is None:
            dist_lens = flat_lengths(_two(used_d))
        hlit = max([257] + [s + 1 for s, ln in lit_lens.items() if ln]) if hlit is None else hlit
        hdist = max([1] + [s + 1 for s, ln in dist_lens.items() if ln]) if hdist is None else hdist
        seq = [lit_lens.get(s, 0) for s in range(hlit)] + [dist_lens.get(s, 0) for s in range(hdist)]
        if cl_syms is None:
            cl_syms = rle(seq)
        used_c = {s for s, _ in cl_syms}
        default_cl = flat_lengths(_two(used_c))
        if cl_lens is None:
            cl_lens = default_cl
        elif callable(cl_lens):
            cl_lens = cl_lens(dict(default_cl))
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CLORD) if cl_lens.get(s, 0)])
        self.header(final, 2)
        w = self.w
        w.bits(hlit - 257, 5); w.bits(hdist - 1, 5); w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens.get(CLORD[i], 0), 3)
        cl = canonical({s: ln for s, ln in cl_lens.items() if CLORD.index(s) < hclen})
        for s, x in cl_syms:
            w.code(cl[s])
            if s >= 16:
                w.bits(x, CLEXT[s])
        self.notes.append(("dynamic", hlit, hdist, hclen, dict(lit_lens), dict(dist_lens), dict(cl_lens), list(cl_syms)))
        self.tokens(toks, canonical(lit_lens), canonical(dist_lens))
        return self

    def body(self):
        return self.w.done()


def subfield(n):
    """an extra subfield of 4 + n bytes to stand in front of BC"""
    return b"XY" + struct.pack("<H", n) + bytes(range(1, n + 1))


def frame(body, crc, isize, extra=b"", tail=b""):
    """one BGZF member around raw deflate data: the gzip header with the BC subfield (extra: subfields in front of it), the data (tail: bytes
    between it and the trailer), CRC-32 and ISIZE as given"""
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(body) + len(tail) + 8
    assert bsize <= 0x10000, bsize
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\0" + struct.pack("<H", bsize - 1) + body + tail + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def deflate_data(member):
    """the raw deflate data of a member (with whatever lies between it and the trailer)"""
    xlen = struct.unpack_from("<H", member, 10)[0]
    return member[12 + xlen:len(member) - 8]


# ---------------------------------------------------------------------------------------------------------------------- the catalogue
def lits(n, seed=1):
    """n literals that do not repeat with any short period"""
    out, x = [], 12345 + seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append((x >> 16) & 0xFF)
    return out


def grow(to, seed=1):
    """fixed-block tokens that bring an empty output to `to` bytes (to >= 64): literals, then matches of 258 at distance 64, then literals"""
    assert to >= 64
    toks, pos = lits(64, seed), 64
    while pos + 258 <= to:
        toks.append(match(258, 64)); pos += 258
    return toks + lits(to - pos, seed + 1)


A, B_, C_ = 0x61, 0x62, 0x63
PHASES = range(8)
MATCH_DISTS = (1, 2, 3, 7, 8, 9, 15, 16)
MATCH_LENS = (3, 4, 7, 8, 9, 16, 17, 257, 258)
# both sets of the long-code cases: lengths 1 .. 14 once and 15 twice (Kraft sum exactly 1)
LONG_LIT = dict([(A + i, i + 1) for i in range(13)] + [(EOB, 14), (284, 15), (285, 15)])
LONG_DIST = dict([(i, i + 1) for i in range(14)] + [(28, 15), (29, 15)])


class Case:
    def __init__(self, name, member, usize, expected, notes):
        self.name, self.member, self.usize, self.expected, self.notes = name, member, usize, expected, notes


def _build():
    out = []

    def add(name, d, valid=True, usize=None, crc_of=None, extra=b"", tail=b"", notes=()):
        """valid: the catalogue expects d.out; otherwise None.  The trailer declares usize and the CRC of crc_of; default: of d.out, i.e.
        of what a lenient decoder would deliver.  Where a token means nothing, the trailer has room for everything in front of it and for
        the bytes it would have added: only the check on the token itself can refuse the member, never the declared size."""
        model = bytes(d.out)
        assert not (valid and d.broken), name
        if d.broken and usize is None:
            need = [n for n in d.notes if n[0] == "bad"][0][2]
            usize, crc_of = len(model) + need, model + bytes(need)
        usize = len(model) if usize is None else usize
        crc_of = model if crc_of is None else crc_of
        body = d.body()
        m = frame(body, zlib.crc32(crc_of), usize, extra, tail)
        out.append(Case(name, m, usize, model if valid else None, list(d.notes) + [("start", 18 + len(extra))] + list(notes)))

    # (first in the catalogue, and so last in the reversed launch) a stored block as the last block of the last member
    add("stored_final", Deflate().fixed(lits(5) + [EOB]).stored(bytes(lits(11, 3)), final=True))

    # ---- bit buffer
    for ph in PHASES:                                                                # a 48-bit token (15 + 5 + 15 + 13) at every bit phase, all extra bits set, behind 32 768 bytes
        for j in range(8):
            d = Deflate().fixed(grow(32768, ph) + [EOB])
            d.dynamic([A] * j + [(284, 31, 29, 8191), EOB], LONG_LIT, LONG_DIST, final=True)
            tok = [n for n in d.notes if n[0] == "match" and n[2] == 48]
            if tok[-1][1] % 8 == ph:
                break
        else:
            raise AssertionError("no phase %d" % ph)
        add("bits48_p%d" % ph, d)
    toks = [A + i for i in range(13)] + [match(258, 1, alt258=True), match(258, 2)]
    toks += [(257 + 27, 7, ds, (1 << DEXT[ds]) - 1) for ds in list(range(14)) + [28, 29]]
    add("huff_1to14_15x2", Deflate().fixed(grow(32768, 9) + [EOB]).dynamic(toks + [EOB], LONG_LIT, LONG_DIST, final=True))
    add("fixed_9bit_literals", Deflate().fixed(list(range(144, 256)) + list(range(255, 143, -1)) + [EOB], final=True))

    # ---- start alignment: the deflate data at every byte alignment of the member
    for n in range(8):
        add("align_x%d" % (4 + n), Deflate().dynamic(lits(9, n) + [match(5, 3), EOB], final=True), extra=subfield(n))

    # ---- stored blocks
    for n in range(10):
        add("stored_len%d" % n, Deflate().stored(bytes(lits(n, 20 + n))).fixed(lits(3, n) + [match(4, 2 if n == 0 else 3), EOB], final=True))
    for ph in PHASES:                                                                # 10 bits per empty fixed block, 19 per fixed block with one 9-bit literal
        a, b = min(((a, b) for a in range(8) for b in range(8) if a + b and (10 * a + 19 * b) % 8 == ph), key=sum)
        d = Deflate()
        for _ in range(a):
            d.fixed([EOB])
        for k in range(b):
            d.fixed([200 + k, EOB])
        d.stored(bytes(lits(13, ph)), final=False).fixed([match(6, 13), EOB], final=True)
        assert [n for n in d.notes if n[0] == "block" and n[1] == 0][0][2] % 8 == ph
        add("stored_phase%d" % ph, d)
    add("stored_max", Deflate().stored(bytes(lits(65505, 5)), final=True))

    # ---- matches at every pos mod 8
    for ph in PHASES:
        for dist in MATCH_DISTS:
            toks, pos = lits(16 + ph, 31 * ph + dist), 16 + ph
            for ln in MATCH_LENS:
                toks.append(match(ln, dist)); pos += ln
                pad = (ph - pos) % 8
                toks += lits(pad, pos); pos += pad
            add("match_p%d_d%d" % (ph, dist), Deflate().fixed(toks + [EOB], final=True))
        add("match_dist_eq_pos_p%d" % ph, Deflate().fixed(lits(24 + ph, ph) + [match(17, 24 + ph), 7, EOB], final=True))
        add("match_ends_at_usize_p%d" % ph, Deflate().fixed(lits(8 + ph, 40 + ph) + [match(11 + ph, 8), EOB], final=True))
        add("match_d32768_p%d" % ph, Deflate().fixed(grow(32768 + ph, 50 + ph) + [match(19, 32768), 9, match(258, 32768), EOB], final=True))
        add("len258_sym285_p%d" % ph, Deflate().fixed(lits(8 + ph, 60 + ph) + [match(258, 5), 1, match(258, 8 + ph), EOB], final=True))
        add("len258_sym284x31_p%d" % ph, Deflate().fixed(lits(8 + ph, 70 + ph) + [match(258, 5, True), 1, match(258, 8 + ph, True), EOB], final=True))

    # ---- dynamic headers
    # HCLEN 4 sends lengths for 16, 17, 18 and 0 alone: every code length such a header can spell is 0, so no end-of-block code can exist.
    # The smallest HCLEN of a valid block is 5 (length 8: 256 literal / length symbols of 8 bits, no distance code).
    l8 = {s: 8 for s in range(1, 257)}
    add("hclen5", Deflate().dynamic([1, 2, 255, EOB], l8, {}, final=True, hclen=5, cl_lens={0: 1, 8: 1}, cl_syms=plain([0] + [8] * 256 + [0])))
    add("hclen19", Deflate().dynamic([A, A + 12, EOB], LONG_LIT, LONG_DIST, final=True, hclen=19))
    seven = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 7}
    lit7 = dict([(A + i, i + 1) for i in range(6)] + [(EOB, 7), (257, 7)])            # lengths 1 .. 6, 7, 7
    add("cl_7bit", Deflate().dynamic([A, A + 5, match(3, 1), EOB], lit7, {0: 1, 1: 1}, final=True, cl_lens=seven,
                                    cl_syms=plain([lit7.get(s, 0) for s in range(258)] + [1, 1])))
    add("hlit286_hdist30", Deflate().fixed(grow(24577, 4) + [EOB]).dynamic([A, (285, 0, 29, 0), EOB], final=True))
    # literal lengths ..., [256] = 2, [257] = 2 | distance lengths 2 2 2 2: a 16 that starts on the last literal length and runs into the distances
    lit4 = {A: 2, B_: 2, EOB: 2, 257: 2}
    head = rle([lit4.get(s, 0) for s in range(257)])
    add("rep16_lit_into_dist", Deflate().dynamic([A, B_, match(3, 2), EOB], lit4, {0: 2, 1: 2, 2: 2, 3: 2}, final=True, cl_syms=head + [(16, 0), (2, 0), (2, 0)]))
    add("rep_ends_on_last", Deflate().dynamic([A, B_, match(3, 2), EOB], lit4, {0: 2, 1: 2, 2: 2, 3: 2}, final=True, cl_syms=head + [(2, 0), (2, 0), (16, 0)]))
    # 97 zeros as 18 x 87 + 17 x 10; 'a', 'b'; 157 zeros as 18 x 138 + 18 x 19; 256
    add("rep17_10_rep18_138", Deflate().dynamic([A, B_, A, EOB], {A: 2, B_: 2, EOB: 1}, {0: 1, 1: 1}, final=True,
                                               cl_syms=[(18, 76), (17, 7), (2, 0), (2, 0), (18, 127), (18, 8), (1, 0), (1, 0), (1, 0)]))
    three = {A: 1, EOB: 2, 257: 2}
    add("single_dist_len1", Deflate().dynamic([A, match(3, 1), EOB], three, {0: 1}, final=True))
    add("no_dist_literal_only", Deflate().dynamic([A, B_, EOB], {A: 2, B_: 2, EOB: 1}, {}, final=True))
    add("only_eob_len1", Deflate().dynamic([EOB], {EOB: 1}, {}, final=True))

    # ---- shape
    add("usize0_stored", Deflate().stored(b"", final=True))
    add("usize0_fixed", Deflate().fixed([EOB], final=True))
    add("usize0_dynamic", Deflate().dynamic([EOB], final=True))
    d = Deflate().stored(bytes(lits(7))).fixed(lits(5, 2) + [match(4, 9), EOB]).dynamic(lits(6, 3) + [match(9, 20), EOB]).stored(b"")
    d.fixed([EOB]).dynamic([A, B_, match(30, 2), EOB]).fixed([match(40, 33), EOB]).stored(bytes(lits(3, 4)), final=True)
    assert sorted(n[1] for n in d.notes if n[0] == "block") == [0, 0, 0, 1, 1, 1, 2, 2]
    add("eight_blocks", d)
    add("trailing_bytes", Deflate().fixed(lits(10, 8) + [EOB], final=True), tail=b"\x00\xff\x55")

    # ---- refused: incomplete and over-subscribed sets.  The trailer agrees with what a decoder that took the set would deliver.
    add("single_dist_len2", Deflate().dynamic([A, match(3, 1), EOB], three, {0: 2}, final=True), valid=False)
    add("only_eob_len2", Deflate().dynamic([EOB], {EOB: 2}, {}, final=True), valid=False)
    add("two_dist_len2", Deflate().dynamic([A, match(3, 1), EOB], three, {0: 2, 1: 2}, final=True), valid=False)
    add("incomplete_lit", Deflate().dynamic([A, B_, EOB], {A: 2, B_: 2, EOB: 2}, {}, final=True), valid=False)
    add("oversub_lit", Deflate().dynamic([A, B_, EOB], {A: 1, B_: 1, EOB: 1}, {}, final=True), valid=False)
    add("oversub_dist", Deflate().dynamic([A, match(3, 1), EOB], three, {0: 1, 1: 1, 2: 1}, final=True), valid=False)
    add("oversub_cl", Deflate().dynamic([A, B_, EOB], {A: 2, B_: 2, EOB: 1}, {0: 1, 1: 1}, final=True, cl_lens=lambda c: {s: 1 for s in c}), valid=False)
    add("incomplete_cl", Deflate().dynamic([A, B_, EOB], {A: 2, B_: 2, EOB: 1}, {0: 1, 1: 1}, final=True, cl_lens=lambda c: {s: ln + (s == max(c)) for s, ln in c.items()}), valid=False)
    # ---- refused: dynamic header errors
    add("hclen4", Deflate().dynamic([], {EOB: 1}, {}, final=True, hclen=4, cl_lens={0: 1, 18: 1}, cl_syms=[(18, 127), (18, 109)]), valid=False)
    eight = {s: 3 for s in (0, 1, 2, A, B_, EOB, 257, 258)}
    add("rep16_first", Deflate().dynamic([A, B_, EOB], eight, {0: 1, 1: 1}, final=True, cl_syms=[(16, 0)] + rle([eight.get(s, 0) for s in range(3, 259)] + [1, 1])), valid=False)
    add("rep_past_last", Deflate().dynamic([A, B_, match(3, 2), EOB], lit4, {0: 2, 1: 2, 2: 2, 3: 2}, final=True, cl_syms=head + [(2, 0), (2, 0), (16, 1)]), valid=False)
    for n in (287, 288):
        add("hlit%d" % n, Deflate().dynamic([A, EOB], {A: 1, EOB: 1}, {0: 1, 1: 1}, final=True, hlit=n), valid=False)
    for n in (31, 32):
        add("hdist%d" % n, Deflate().dynamic([A, EOB], {A: 1, EOB: 1}, {0: 1, 1: 1}, final=True, hdist=n), valid=False)
    d = Deflate()
    d.header(True, 2)
    d.w.bits(0, 5); d.w.bits(1, 5); d.w.bits(14, 4)                                   # HLIT 257, HDIST 2, HCLEN 18: lengths for 0 and 1 (one bit each)
    for i in range(18):
        d.w.bits(1 if CLORD[i] in (0, 1) else 0, 3)
    cl = canonical({0: 1, 1: 1})
    for v in [0] * A + [1, 1] + [0] * (257 - A - 2) + [1, 1]:                         # 'a' and 'b' coded, 256 not
        d.w.code(cl[v])
    d.w.code((0, 1)); d.w.code((1, 1)); d.out += bytes([A, B_])
    add("no_eob_code", d, valid=False)
    add("match_without_dist_codes", Deflate().dynamic([A, (257, 0, None, 0), EOB], three, {}, final=True), valid=False)
    # ---- refused: symbols of the fixed codes that are no symbols
    for s in (286, 287):
        add("fixed_sym%d" % s, Deflate().fixed([A, s, EOB], final=True), valid=False)
    for s in (30, 31):
        add("fixed_dist%d" % s, Deflate().fixed([A, (257, 0, s, 0), EOB], final=True), valid=False)
    # ---- refused: bounds.  Where the output is declared a byte shorter than the stream's, the CRC is that of the shorter output.
    add("dist_pos_plus1", Deflate().fixed(lits(5) + [match(3, 6), EOB], final=True), valid=False)
    add("dist1_at_pos0", Deflate().fixed([match(3, 1), EOB], final=True), valid=False)
    d = Deflate().fixed(lits(8) + [match(8, 8), EOB], final=True)
    add("match_past_usize", d, valid=False, usize=15, crc_of=bytes(d.out[:15]))
    d = Deflate().fixed(lits(9) + [EOB], final=True)
    add("literal_past_usize", d, valid=False, usize=8, crc_of=bytes(d.out[:8]))
    d = Deflate().stored(bytes(lits(9)), final=True)
    add("stored_past_usize", d, valid=False, usize=8, crc_of=bytes(d.out[:8]))
    # LEN 10 over 9 bytes of data: the tenth would be the CRC's first byte; the data is chosen so that a CRC exists that agrees with it
    for seed in range(64):
        data = bytes(lits(9, 100 + seed))
        fix = [b for b in range(256) if zlib.crc32(data + bytes([b])) & 0xFF == b]
        if fix:
            break
    d = Deflate().stored(data + bytes(fix[:1]), final=True, body=data)
    add("stored_past_data", d, valid=False)
    add("stored_nlen_mismatch", Deflate().stored(bytes(lits(9)), final=True, nlen=9 ^ 0xFFFE), valid=False)
    d = Deflate(); d.header(True, 3); d.w.bits(0, 13)
    add("btype3", d, valid=False)
    # 3 header bits, five 9-bit and seven 8-bit literals: the block ends on a byte boundary, so no padding reads as the 7-bit end-of-block.
    # The literals are chosen so that the CRC's first seven bits do: only the end of the data stands between a decoder and acceptance.
    for seed in range(4096):
        toks = [200 + (seed >> 8), 201, 202, 203, 204] + [v & 127 for v in lits(7, seed)]
        if zlib.crc32(bytes(toks)) & 0x7F == 0:
            break
    d = Deflate().fixed(toks, final=True)
    assert d.w.n == 0 and zlib.crc32(bytes(d.out)) & 0x7F == 0
    add("no_eob_before_crc", d, valid=False)
    add("no_bfinal", Deflate().fixed(lits(12, 7) + [EOB], final=False), valid=False)
    d = Deflate().fixed(lits(12, 8) + [EOB], final=True)
    add("output_short", d, valid=False, usize=13, crc_of=bytes(d.out) + b"\0")
    # a dynamic header cut off inside its code-length symbols, the trailer directly behind: a decoder that read on would take the trailer
    # and the next member for lengths
    d = Deflate().dynamic([A, EOB], LONG_LIT, LONG_DIST, final=True, cl_syms=plain([LONG_LIT.get(s, 0) for s in range(286)] + [LONG_DIST.get(s, 0) for s in range(30)]))
    cut = Deflate(); cut.w.raw(d.body()[:40]); cut.notes = [n for n in d.notes if n[0] in ("block", "dynamic")] + [("cut", 40)]
    add("header_past_data", cut, valid=False)

    # (last in the catalogue) the EOF member
    out.append(Case("eof_member", EOF_MEMBER, 0, b"", [("start", 18)]))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CASES = None


def _all():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def cases():
    return [(c.name, c.member, c.usize, c.expected) for c in _all()]


def records():
    return {c.name: c.notes for c in _all()}
