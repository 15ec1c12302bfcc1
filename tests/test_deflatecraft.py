"""The catalogue of hand-built deflate members (deflatecraft.py) before any decoder of ours sees it: zlib is the arbiter of every case, the
names the decoders' tests rely on are all there, and what the names promise -- 15-bit codes, a 48-bit token at every bit phase, every
alignment -- is read from the builder's own notes, not from a decoder."""
import zlib

import pytest

import deflatecraft as dc

CASES = dc.cases()
BY_NAME = {c[0]: c for c in CASES}
NOTES = dc.records()

P8 = range(8)
VALID = (["stored_final", "huff_1to14_15x2", "fixed_9bit_literals", "stored_max", "hclen5", "hclen19", "cl_7bit", "hlit286_hdist30", "rep16_lit_into_dist",
          "rep_ends_on_last", "rep17_10_rep18_138", "single_dist_len1", "no_dist_literal_only", "only_eob_len1", "usize0_stored", "usize0_fixed", "usize0_dynamic",
          "eight_blocks", "trailing_bytes", "eof_member"] +
         ["bits48_p%d" % p for p in P8] + ["align_x%d" % x for x in range(4, 12)] + ["stored_len%d" % n for n in range(10)] + ["stored_phase%d" % p for p in P8] +
         ["match_p%d_d%d" % (p, d) for p in P8 for d in dc.MATCH_DISTS] +
         ["%s_p%d" % (k, p) for k in ("match_dist_eq_pos", "match_ends_at_usize", "match_d32768", "len258_sym285", "len258_sym284x31") for p in P8])
INVALID = ["single_dist_len2", "only_eob_len2", "two_dist_len2", "incomplete_lit", "oversub_lit", "oversub_dist", "oversub_cl", "incomplete_cl",
           "hclen4",                                                                    # (HCLEN 4 can spell no length but 0: see deflatecraft)
           "rep16_first", "rep_past_last", "hlit287", "hlit288", "hdist31", "hdist32", "no_eob_code", "match_without_dist_codes",
           "fixed_sym286", "fixed_sym287", "fixed_dist30", "fixed_dist31",
           "dist_pos_plus1", "dist1_at_pos0", "match_past_usize", "literal_past_usize", "stored_past_usize", "stored_past_data",
           "stored_nlen_mismatch", "btype3", "no_eob_before_crc", "no_bfinal", "output_short", "header_past_data"]


def test_catalogue_names_and_size():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names)) and len(names) < 2000
    assert not set(VALID) - set(names), sorted(set(VALID) - set(names))
    assert not set(INVALID) - set(names), sorted(set(INVALID) - set(names))
    for n in VALID:
        assert BY_NAME[n][3] is not None, n
    for n in INVALID:
        assert BY_NAME[n][3] is None, n
    assert names[0] == "stored_final" and names[-1] == "eof_member"                     # the ends of a launch in catalogue order and in reverse
    for name, m, usize, want in CASES:                                                 # the framing: BSIZE, ISIZE, and the output's CRC where there is one
        assert len(m) <= 0x10000 and usize <= 0x10000 and int.from_bytes(m[-4:], "little") == usize, name
        if want is not None:
            assert len(want) == usize and zlib.crc32(want) == int.from_bytes(m[-8:-4], "little"), name


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_zlib_is_the_arbiter(name):
    """expected bytes: zlib delivers exactly them and ends.  None: zlib raises, does not reach the stream's end (what inflate with Z_FINISH
    refuses), or delivers what the trailer's ISIZE / CRC-32 do not describe"""
    _, m, usize, want = BY_NAME[name]
    o = zlib.decompressobj(-15)
    try:
        got = o.decompress(dc.deflate_data(m))
    except zlib.error:
        assert want is None, name
        return
    if want is not None:
        assert got == want and o.eof
        assert bool(o.unused_data) == (name == "trailing_bytes")
    else:
        assert not o.eof or len(got) != usize or zlib.crc32(got) != int.from_bytes(m[-8:-4], "little")
    if name in ("match_past_usize", "literal_past_usize", "stored_past_usize", "output_short"):
        assert o.eof and len(got) != usize                                            # a sound stream: only the declared size refuses it


BAD_TOKEN = ("match_without_dist_codes", "fixed_sym286", "fixed_sym287", "fixed_dist30", "fixed_dist31", "dist_pos_plus1", "dist1_at_pos0")


@pytest.mark.parametrize("name", BAD_TOKEN)
def test_only_the_bad_token_can_refuse_its_member(name):
    """the declared size holds everything in front of the token that means nothing and the bytes it would add, and the CRC agrees with what
    stands in front of it: neither the size guard nor an earlier token refuses the member"""
    _, m, usize, want = BY_NAME[name]
    (_, pos, need), = [n for n in NOTES[name] if n[0] == "bad"]
    assert want is None and pos < usize and pos + need <= usize
    ms = [x for x in NOTES[name] if x[0] == "match"]
    if ms:
        assert ms[-1][3] == pos and pos + ms[-1][4] <= usize                           # the match fits; its distance or its code is what is wrong
    if name == "dist_pos_plus1":
        assert ms[-1][5] == pos + 1
    if name == "dist1_at_pos0":
        assert (ms[-1][5], pos) == (1, 0)
    o = zlib.decompressobj(-15)
    with pytest.raises(zlib.error):
        o.decompress(dc.deflate_data(m))


def test_header_past_data_is_cut_inside_its_code_length_symbols():
    (hlit, hdist, hclen, lit, dist, cl, syms), = [n[1:] for n in NOTES["header_past_data"] if n[0] == "dynamic"]
    (_, cut), = [n for n in NOTES["header_past_data"] if n[0] == "cut"]
    shortest, longest = min(v for v in cl.values() if v), max(cl.values())
    assert len(dc.deflate_data(BY_NAME["header_past_data"][1])) == cut
    assert 3 + 14 + 3 * hclen + longest * 8 < 8 * cut < 3 + 14 + 3 * hclen + shortest * len(syms)      # behind the first symbols, in front of the last


def _matches(name):
    return [n for n in NOTES[name] if n[0] == "match"]


def _dyn(name):
    return [n for n in NOTES[name] if n[0] == "dynamic"]


def test_long_codes_and_the_48_bit_token():
    lens15 = sorted(list(range(1, 15)) + [15, 15])
    assert dc.kraft(dc.LONG_LIT) == dc.kraft(dc.LONG_DIST) == 1 << 15
    assert sorted(dc.LONG_LIT.values()) == sorted(dc.LONG_DIST.values()) == lens15
    assert dc.LONG_LIT[284] == 15 and dc.LONG_DIST[29] == 15
    phases = set()
    for p in P8:
        (hlit, hdist, hclen, lit, dist, cl, syms), = [n[1:] for n in _dyn("bits48_p%d" % p)]
        assert lit == dc.LONG_LIT and dist == dc.LONG_DIST
        tok, = [m for m in _matches("bits48_p%d" % p) if m[3] >= 32768]                # (the matches in front of it only grow the output)
        _, at, nbits, pos, length, distance, lbits, dbits = tok
        assert (nbits, lbits, dbits, length, distance) == (48, 15, 15, 258, 32768) and pos >= 32768 and at % 8 == p
        phases.add(at % 8)
    assert phases == set(P8)
    # every symbol of both sets is used once at least
    (hlit, hdist, hclen, lit, dist, cl, syms), = [n[1:] for n in _dyn("huff_1to14_15x2")]
    assert lit == dc.LONG_LIT and dist == dc.LONG_DIST and hclen == 19
    ms = [m for m in _matches("huff_1to14_15x2") if m[3] >= 32768]
    assert {m[6] for m in ms} == {15} and {m[7] for m in ms} == set(range(1, 16))
    assert set(BY_NAME["huff_1to14_15x2"][3][32768:32768 + 13]) == {dc.A + i for i in range(13)}             # the literals of 1 .. 13 bits
    assert len(BY_NAME["fixed_9bit_literals"][3]) == 224 and min(BY_NAME["fixed_9bit_literals"][3]) == 144


def test_alignments_and_stored_phases():
    assert sorted(n[1] % 8 for x in range(4, 12) for n in NOTES["align_x%d" % x] if n[0] == "start") == list(P8)
    for p in P8:
        blocks = [n for n in NOTES["stored_phase%d" % p] if n[0] == "block"]
        st, = [b for b in blocks if b[1] == 0]
        assert st[2] % 8 == p and blocks.index(st) > 0 and all(b[1] == 1 for b in blocks if b is not st)
    for n in range(10):
        b0, b1 = [b for b in NOTES["stored_len%d" % n] if b[0] == "block"]
        assert (b0[1], b1[1]) == (0, 1) and b1[3] == n and b1[2] == 8 * (5 + n)        # the fixed block starts on the byte behind LEN bytes of data
    assert [b[1] for b in NOTES["stored_final"] if b[0] == "block"][-1] == 0
    assert BY_NAME["stored_max"][2] == 65505 and len(BY_NAME["stored_max"][1]) == 0x10000


def test_matches_cover_every_position_distance_and_length():
    seen = set()
    for p in P8:
        for d in dc.MATCH_DISTS:
            seen |= {(m[3] % 8, m[5], m[4]) for m in _matches("match_p%d_d%d" % (p, d))}
    assert seen >= {(p, d, ln) for p in P8 for d in dc.MATCH_DISTS for ln in dc.MATCH_LENS}
    for p in P8:
        m = _matches("match_dist_eq_pos_p%d" % p)[0]
        assert m[3] % 8 == p and m[5] == m[3]
        m = _matches("match_ends_at_usize_p%d" % p)[-1]
        assert m[3] % 8 == p and m[3] + m[4] == BY_NAME["match_ends_at_usize_p%d" % p][2]
        ms = _matches("match_d32768_p%d" % p)
        assert ms[-2][3] == 32768 + p and ms[-2][5] == ms[-1][5] == 32768
        for k, nbits in (("len258_sym285", 8), ("len258_sym284x31", 8 + 5)):        # fixed codes: 285 is 8 bits, 284 is 8 bits and 5 extra
            m = _matches("%s_p%d" % (k, p))[0]
            assert m[3] % 8 == p and m[4] == 258 and m[2] - 5 - dc.DEXT[dc.match(1 + 2, m[5])[2]] == nbits


def test_dynamic_headers_say_what_their_names_say():
    h = {k: _dyn(k)[-1] for k in ("hclen4", "hclen5", "hclen19", "cl_7bit", "hlit286_hdist30", "rep16_lit_into_dist", "rep_ends_on_last", "rep17_10_rep18_138",
                                  "single_dist_len1", "single_dist_len2", "no_dist_literal_only", "only_eob_len1", "only_eob_len2", "two_dist_len2", "rep_past_last", "rep16_first")}
    assert h["hclen4"][3] == 4 and h["hclen5"][3] == 5 and h["hclen19"][3] == 19 and h["hclen19"][6].get(15, 0) > 0
    assert max(h["cl_7bit"][6].values()) == 7 and dc.kraft(h["cl_7bit"][6]) == 1 << 15
    assert h["hlit286_hdist30"][1:3] == (286, 30) and _matches("hlit286_hdist30")[-1][5] == 24577 and _matches("hlit286_hdist30")[-1][4] == 258

    def spans(name):
        """(code-length symbol, first index, one past the last index) of every symbol of the header"""
        out, i = [], 0
        for s, x in h[name][7]:
            n = 1 if s < 16 else (3 + x if s < 18 else 11 + x)
            out.append((s, i, i + n)); i += n
        return out, h[name][1], h[name][1] + h[name][2]

    sp, hlit, total = spans("rep16_lit_into_dist")
    assert any(s == 16 and a < hlit < b for s, a, b in sp) and sp[-1][2] == total
    sp, hlit, total = spans("rep_ends_on_last")
    assert sp[-1][0] == 16 and sp[-1][2] == total
    sp, hlit, total = spans("rep_past_last")
    assert sp[-1][0] == 16 and sp[-1][2] == total + 1
    sp, hlit, total = spans("rep17_10_rep18_138")
    assert (17, 10) in {(s, b - a) for s, a, b in sp} and (18, 138) in {(s, b - a) for s, a, b in sp} and sp[-1][2] == total
    assert spans("rep16_first")[0][0][0] == 16
    nz = lambda d: {s: ln for s, ln in d.items() if ln}
    assert nz(h["single_dist_len1"][5]) == {0: 1} and nz(h["single_dist_len2"][5]) == {0: 2} and nz(h["two_dist_len2"][5]) == {0: 2, 1: 2}
    assert nz(h["no_dist_literal_only"][5]) == {} and not _matches("no_dist_literal_only")
    assert nz(h["only_eob_len1"][4]) == {256: 1} and nz(h["only_eob_len2"][4]) == {256: 2}
    # what a decoder that took the two lone codes of two bits would deliver is what their trailers describe
    assert BY_NAME["single_dist_len2"][2] == 4 and int.from_bytes(BY_NAME["single_dist_len2"][1][-8:-4], "little") == zlib.crc32(b"aaaa")
    assert BY_NAME["only_eob_len2"][2] == 0 and int.from_bytes(BY_NAME["only_eob_len2"][1][-8:-4], "little") == 0
    assert len([n for n in NOTES["eight_blocks"] if n[0] == "block"]) == 8
