"""BGZF/BAM reader and writer + FASTA loader (gencore_amd/csrc/bamio.cpp) against an independent pure-Python
implementation of the formats (tests/pybam.py) and hand-derived FASTA cases; GPU: a BAM file end to end through gce_run_bam."""
import numpy as np
import pytest

import fuzzgen
import pybam
from gencore_amd.batch import ReadBatch
from gencore_amd.capi import default_params


def records_of(batch):
    """python records (dicts) of a ReadBatch, for pybam.write_bam"""
    out = []
    for i in range(batch.n):
        c = batch.core[i]
        d = dict(qname=batch.qname_of(i), flag=int(c["flag"]), tid=int(c["tid"]), pos=int(c["pos"]), cigar=batch.cigar_of(i), mtid=int(c["mtid"]),
                 mpos=int(c["mpos"]), isize=int(c["isize"]), seq=batch.seq_of(i), qual=batch.qual_of(i).tolist(), mapq=int(c["mapq"]), bin=int(c["bin"]),
                 nm=(int(batch.nm[i]) if batch.nm_type[i] else None), nm_type=(chr(batch.nm_type[i]) if batch.nm_type[i] else "C"))
        if i % 3 == 0:
            d["aux_pre"] = [("AS", "i", 77 + i), ("XZ", "Z", "before")]
        if i % 5 == 0:
            d["aux_post"] = [("RG", "Z", "grp%d" % (i % 4)), ("XS", "s", -3)]
        out.append(d)
    return out


def same_batch(a, b):
    assert a.n == b.n
    for f in ("tid", "pos", "l_qname", "mapq", "bin", "n_cigar", "flag", "l_qseq", "mtid", "mpos", "isize"):
        assert np.array_equal(a.core[f], b.core[f]), f
    for i in range(a.n):
        assert a.qname_of(i) == b.qname_of(i) and a.cigar_of(i) == b.cigar_of(i) and a.seq_of(i) == b.seq_of(i) and a.qual_of(i).tolist() == b.qual_of(i).tolist()
    assert np.array_equal(a.nm_type, b.nm_type) and np.array_equal(np.where(a.nm_type != 0, a.nm, 0), np.where(b.nm_type != 0, b.nm, 0))


@pytest.mark.parametrize("seed,block", [(5, 0xff00), (9, 700), (31, 65280)])
def test_reader_against_python_writer(built, tmp_path, seed, block):
    """pybam writes the file (odd BGZF block sizes cut records across blocks), the C++ reader must hand back the same batch."""
    from gencore_amd.bamio import BamFile
    batch, over, reference, contig_len = fuzzgen.make_case(seed, n_mol=40)
    recs = records_of(batch)
    targets = [("ctg%d" % i, int(l)) for i, l in enumerate(contig_len)]
    path = str(tmp_path / "in.bam")
    pybam.write_bam(path, recs, targets, block=block)
    f = BamFile(path, threads=3)
    assert f.target_name == [t[0] for t in targets] and f.target_len == [t[1] for t in targets] and f.n_records == batch.n
    same_batch(f.batch(), batch)
    half = batch.n // 2                                         # chunks are relative to their own blobs
    a, b2 = f.batch(0, half), f.batch(half, batch.n - half)
    assert a.n == half and b2.qname_of(0) == batch.qname_of(half) and int(b2.seq_off[0]) == 0
    info = f.info
    assert info.seq_bytes == batch.seq.size and info.qual_bytes == batch.qual.size and info.cigar_words == batch.cigar.size
    f.close()


def test_reader_parallel_index_on_a_large_file(built, tmp_path):
    """> 4 MB per host thread: the record index is built from speculative per-segment walks joined against the verified chain
    (bamio.cpp); the batch must equal the one the file was written from, whatever the thread count."""
    from gencore_amd import synth
    from gencore_amd.bamio import BamFile, write_batch_as_bam
    d = synth.generate("cfg3", n_pairs=60000)
    batch = d.to_batch()
    path = str(tmp_path / "big.bam")
    write_batch_as_bam(path, batch, np.asarray(d.target_len, np.uint32), threads=4)
    for th in (1, 5, 8):
        f = BamFile(path, threads=th)
        b = f.batch()
        assert b.n == batch.n and np.array_equal(b.core, batch.core)
        for name in ("qname_off", "seq_off", "qual_off", "cigar_off", "nm", "nm_type"):
            assert np.array_equal(getattr(b, name), getattr(batch, name)), name
        assert np.array_equal(b.seq, batch.seq[:b.seq.size]) and np.array_equal(b.qual, batch.qual[:b.qual.size])
        assert np.array_equal(b.qname, batch.qname[:b.qname.size]) and np.array_equal(b.cigar, batch.cigar[:b.cigar.size])
        f.close()


def test_reader_mi_tag_and_nm_types(built, tmp_path):
    from gencore_amd.bamio import BamFile
    recs = []
    for k, (typ, val) in enumerate([("C", 7), ("c", -2), ("S", 300), ("s", -300), ("i", -70000), ("I", 70000)]):
        recs.append(dict(qname="r%d" % k, flag=99, tid=0, pos=10 + k, cigar="4M", mtid=0, mpos=100, isize=94, seq="ACGT", qual=[30] * 4, nm=val, nm_type=typ,
                         mi=("AAC_GGT" if k % 2 else None), aux_pre=[("XB", "C", 1)]))
    recs.append(dict(qname="nonm", flag=99, tid=0, pos=30, cigar="4M", mtid=0, mpos=100, isize=74, seq="ACGT", qual=[30] * 4, nm=None))
    path = str(tmp_path / "mi.bam")
    pybam.write_bam(path, recs, [("c", 1000)])
    f = BamFile(path)
    b = f.batch()
    assert b.nm.tolist()[:6] == [7, -2, 300, -300, -70000, 70000] and [chr(x) for x in b.nm_type[:6]] == list("CcSsiI") and b.nm_type[6] == 0
    mi = [None if int(o) == 0xFFFFFFFFFFFFFFFF else bytes(b.mi[int(o):]).split(b"\0")[0].decode() for o in b.mi_off]
    assert mi == [None, "AAC_GGT", None, "AAC_GGT", None, "AAC_GGT", None]
    f.close()


def test_bad_files_are_rejected(built, tmp_path):
    from gencore_amd.bamio import BamFile
    from gencore_amd.capi import GceError
    p = tmp_path / "x.bam"
    p.write_bytes(b"not a bam at all, not even gzip")
    with pytest.raises(GceError):
        BamFile(str(p))
    good = tmp_path / "g.bam"
    pybam.write_bam(str(good), [dict(qname="a", flag=4, tid=-1, pos=-1, cigar="*", mtid=-1, mpos=-1, isize=0, seq="ACGT", qual=[1] * 4, nm=None)], [("c", 10)])
    raw = bytearray(good.read_bytes())
    raw[30] ^= 0xFF                                             # corrupt the deflate stream / CRC
    bad = tmp_path / "b.bam"
    bad.write_bytes(bytes(raw))
    with pytest.raises(GceError):
        BamFile(str(bad))
    # the file cut inside its first member: within the extra field or the room of the trailer behind it, and further in
    whole = good.read_bytes()
    for cut, msg in ((18, "truncated BGZF block header"), (25, "truncated BGZF block header"), (26, "bad BGZF block"), (60, "bad BGZF block"),
                     (17, "trailing bytes after the last BGZF block")):
        bad.write_bytes(whole[:cut])
        with pytest.raises(GceError) as e:
            BamFile(str(bad))
        assert str(e.value).endswith(": " + msg), (cut, str(e.value))


@pytest.mark.parametrize("level,strategy", [(0, "default"), (1, "default"), (9, "default"), (6, "fixed"), (6, "huffman"), (6, "rle"), (1, "filtered")])
def test_reader_on_every_deflate_block_type(built, tmp_path, level, strategy):
    """bamio.cpp decodes BGZF members with its own raw-deflate decoder in front of zlib: stored, fixed-Huffman and dynamic blocks,
    literal-only and run-length streams, short and long codes -- the batch must be the one a zlib-only pass gives, and the records
    the ones that were written."""
    import os
    import subprocess
    import sys
    import zlib
    strat = dict(default=zlib.Z_DEFAULT_STRATEGY, fixed=zlib.Z_FIXED, huffman=zlib.Z_HUFFMAN_ONLY, rle=zlib.Z_RLE, filtered=zlib.Z_FILTERED)[strategy]
    batch, _, _, contig_len = fuzzgen.make_case(900 + level, n_mol=120)
    recs = records_of(batch)
    path = str(tmp_path / "t.bam")
    pybam.write_bam(path, recs, [("c%d" % i, int(l)) for i, l in enumerate(contig_len)], block=0xff00 if level else 0x8000, level=level, strategy=strat)
    from gencore_amd.bamio import BamFile
    f = BamFile(path, threads=3)
    got = f.batch()
    same_batch(got, batch)
    f.close()
    # the same file through zlib alone (the switch is read once per process: a child)
    code = ("import sys; sys.path[:0] = [%r, %r]\nfrom gencore_amd.bamio import BamFile\nimport numpy as np\n"
            "f = BamFile(%r, threads=2); b = f.batch(); print(b.n, int(b.seq.astype(np.uint64).sum()), int(b.qual.astype(np.uint64).sum()))" % (
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)), path))
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, GCE_BAM_ZLIB_ONLY="1")).split()
    assert [int(x) for x in out[-3:]] == [got.n, int(got.seq.astype(np.uint64).sum()), int(got.qual.astype(np.uint64).sum())]


def test_checksum_of_large_blocks_is_verified(built, tmp_path):
    """BGZF members of 64 KB go through the carry-less-multiply CRC-32 (bamio.cpp): a file written by the pure-Python writer must
    open, and one flipped bit -- in a stored CRC, or in the payload of a stored (uncompressed) member -- must be rejected."""
    import struct
    import zlib
    from gencore_amd.bamio import BamFile
    from gencore_amd.capi import GceError
    rng = np.random.default_rng(5)
    recs = [dict(qname="r%05d" % i, flag=4, tid=-1, pos=-1, cigar="*", mtid=-1, mpos=-1, isize=0,
                 seq="".join(rng.choice(list("ACGT"), 150)), qual=[int(q) for q in rng.integers(2, 41, 150)], nm=None) for i in range(3000)]
    good = tmp_path / "g.bam"
    pybam.write_bam(str(good), recs, [("c", 1000)])
    f = BamFile(str(good), threads=2); assert f.info.n_records == len(recs); f.close()
    raw = bytearray(good.read_bytes())
    bsize = struct.unpack_from("<H", raw, 16)[0] + 1              # first member (> 64 bytes of payload)
    assert struct.unpack_from("<I", raw, bsize - 4)[0] > 4096
    flipped = bytearray(raw); flipped[bsize - 8] ^= 0x01          # its stored CRC
    bad = tmp_path / "b.bam"; bad.write_bytes(bytes(flipped))
    with pytest.raises(GceError):
        BamFile(str(bad))
    # a member holding one stored deflate block: a payload bit flips without upsetting the deflate stream itself
    payload = bytes(rng.integers(0, 256, 5000, dtype=np.uint8))
    co = zlib.compressobj(0, zlib.DEFLATED, -15); cd = co.compress(payload) + co.flush()
    member = bytearray(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(cd) + 8 - 1) + cd + struct.pack("<II", zlib.crc32(payload), len(payload)))
    member[18 + 5 + 2000] ^= 0x10                                 # inside the stored bytes (5-byte stored-block header)
    bad2 = tmp_path / "b2.bam"; bad2.write_bytes(bytes(member) + bytes(raw))
    with pytest.raises(GceError):
        BamFile(str(bad2))


@pytest.mark.parametrize("seed,level", [(4, 6), (22, 1), (23, -1), (4, 0)])
def test_writer_against_python_reader(built, oracle, tmp_path, seed, level):
    """gce_bam_write fed with the ORACLE's result table (as gce_result rows): the file, parsed by pybam, holds exactly the records
    the oracle emits -- name copies, NM patches, FR / RR appended behind the untouched aux fields."""
    import ctypes as C
    from gencore_amd import capi
    from gencore_amd.bamio import BamFile
    from test_host_logic import rows_from_table
    batch, over, reference, contig_len = fuzzgen.make_case(seed, n_mol=60, umi_mode="duplex")
    for k in list(over):
        if k not in ("umi_prefix", "flush_period", "cluster_size_req"):
            over.pop(k)
    want = oracle.run(batch, fuzzgen.make_params(over, contig_len), reference)
    assert want.status == 0
    recs = records_of(batch)
    targets = [("ctg%d" % i, int(l)) for i, l in enumerate(contig_len)]
    src = str(tmp_path / "in.bam")
    pybam.write_bam(src, recs, targets, text="@HD\tVN:1.6\n@CO\tkeep me\n")
    f = BamFile(src, threads=2)
    rows = rows_from_table(batch, want)
    r = capi.GceResult()
    keep = {k: np.ascontiguousarray(v) for k, v in rows.items()}
    keep["fr"] = keep["fr"].astype(np.int16); keep["rr"] = keep["rr"].astype(np.int16); keep["nm_new"] = keep["nm_new"].astype(np.int32)
    keep["kind"] = keep["kind"].astype(np.uint8); keep["qname_src"] = keep["qname_src"].astype(np.uint32)
    r.n_reads, r.n_out = batch.n, len(rows["src"])
    for name in ("src", "kind", "qname_src", "nm_new", "fr", "rr", "mate", "seq_off", "qual_off", "seq", "qual"):
        setattr(r, name, keep[name].ctypes.data)
    r.seq_bytes, r.qual_bytes = keep["seq"].size, keep["qual"].size
    out = str(tmp_path / "out.bam")
    assert f.lib.gce_bam_write(out.encode(), f._h, C.byref(r), 3, level) == 0      # (-1: the library's own fixed-Huffman encoder)
    text, tg, got = pybam.read_bam(out)
    assert text == "@HD\tVN:1.6\n@CO\tkeep me\n" and tg == targets
    exp = {x["src"]: x for x in want.records(batch)}
    assert len(got) == len(rows["src"])
    for k, g in enumerate(got):
        i = int(rows["src"][k]); e = exp[i]; o = recs[i]
        assert (g["qname"], g["flag"], g["tid"], g["pos"], g["mtid"], g["mpos"], g["isize"], g["seq"], g["qual"]) == \
               (e["qname"].rstrip("\0"), e["flag"], e["tid"], e["pos"], e["mtid"], e["mpos"], e["isize"], e["seq"], e["qual"]), (k, g, e)
        assert g["mapq"] == o["mapq"] and g["bin"] == o["bin"] and pybam.parse_cigar(o["cigar"]) == g["cigar"]
        if e["nm"] is not None:
            assert g["aux"]["NM"][1] == e["nm"] and g["aux"]["NM"][0] == o["nm_type"]
        assert ("FR" in g["aux"]) == (e["fr"] >= 0) and ("RR" in g["aux"]) == (e["rr"] >= 0)
        if e["fr"] >= 0:
            assert g["aux"]["FR"] == ("C", e["fr"])
        if e["rr"] >= 0:
            assert g["aux"]["RR"] == ("C", e["rr"]) and g["aux_order"][-2:] == ["FR", "RR"]
        for tag, typ, val in o.get("aux_pre", []) + o.get("aux_post", []):      # everything else untouched, in place
            assert g["aux"][tag] == (typ, val)
    f.close()


# ------------------------------------------------------------------------------------------------------------------ FASTA
FASTA_CASES = [
    # (file text, expected {id: bases}) -- worked out by hand from src/fastareader.cpp:7-41,57-104 and util.h:194-210
    (">c1 first contig\nACGT\nacgt\n>c2\nGG\n", {"c1": "ACGTACGT", "c2": "GG"}),
    # an empty line: get(c) takes the '\n' itself as a base, the next line is then consumed whole by getline
    (">c1\nACGT\n\nTTTT\n", {"c1": "ACGT\nTTTT"}),
    # the first character of a line escapes str_keep_valid_sequence (digits / blanks survive there and only there)
    (">c1\n1ACGT\nAC GT9\n", {"c1": "1ACGTACGT"}),
    # no trailing newline; junk before the first '>' is skipped; '-' and '*' are kept
    ("junk\n>c1\nAC-G*\nTT", {"c1": "AC-G*TT"}),
    # CRLF: '\r' is dropped from sequence lines but stays in an ID without a blank
    (">c1 x\r\nACGT\r\n>c2\r\nGG\r\n", {"c1": "ACGT", "c2\r": "GG"}),
    # a later contig of the same name replaces the earlier one; an empty contig is a contig
    (">c1\nAAAA\n>c1\nCC\n>e\n>z\nG\n", {"c1": "CC", "e": "", "z": "G"}),
]


@pytest.mark.parametrize("case", range(len(FASTA_CASES)))
def test_fasta_loader_quirks(built, tmp_path, case):
    from gencore_amd.bamio import load_fasta
    text, want = FASTA_CASES[case]
    p = tmp_path / "ref.fa"
    p.write_bytes(text.encode())
    got = {k: v.decode() for k, v in load_fasta(str(p)).items()}
    assert got == want


def _fasta_walk_py(data):
    """FastaReader(file) + readAll restated literally in Python (src/fastareader.cpp:7-41,57-104,157-168; util.h:194-210): the
    independent check of the loader's one-pass walk and, through it, of the parallel one."""
    n, p = len(data), 0
    while p < n and data[p:p + 1] != b">":
        p += 1
    if p < n:
        p += 1
    eof = p >= n
    ids, seqs = [], {}
    while not eof:
        header, seq, found = bytearray(), bytearray(), False
        while True:
            if p >= n:
                eof = True
                break
            c = data[p]; p += 1
            if c == ord(">"):
                break
            if found:
                seq.append(c - 32 if 97 <= c <= 122 else c)
            else:
                header.append(c)
            if p >= n:
                line, eof = b"", True
            else:
                e = data.find(b"\n", p)
                if e < 0:
                    line, p, eof = data[p:], n, True
                else:
                    line, p = data[p:e], e + 1
            if not found:
                header += line; found = True
            else:
                for ch in line:
                    ch = ch - 32 if 97 <= ch <= 122 else ch
                    if 65 <= ch <= 90 or ch in (45, 42):
                        seq.append(ch)
            if eof:
                break
        hid = bytes(header).split(b" ", 1)[0]
        if hid not in seqs:
            ids.append(hid)
        seqs[hid] = bytes(seq)
    return [(i, seqs[i]) for i in ids]


def _load_fasta_raw(path, threads):
    import ctypes as C
    from gencore_amd import capi
    lib = capi.load_library()
    h = C.c_void_p()
    assert lib.gce_fasta_load(str(path).encode(), threads, C.byref(h)) == 0
    n = C.c_int32()
    ids, seqs, lens = C.POINTER(C.c_char_p)(), C.POINTER(C.c_void_p)(), C.POINTER(C.c_int64)()
    lib.gce_fasta_get(h, C.byref(n), C.byref(ids), C.byref(seqs), C.byref(lens))
    out = [(ids[i], C.string_at(seqs[i], lens[i])) for i in range(n.value)]
    lib.gce_fasta_free(h)
    return out


@pytest.mark.parametrize("seed", range(40))
def test_fasta_parallel_equals_the_literal_walk(built, tmp_path, monkeypatch, seed):
    """Random FASTA-like text with everything the walk is sensitive to (runs of line feeds, '>' at line starts / inside lines / doubled /
    at the very end, CRLF, lower case, digits, missing final newline): the Python restatement, the one-thread walk and the file cut
    into 2..9 ranges must agree byte for byte."""
    rng = np.random.default_rng(1000 + seed)
    monkeypatch.setenv("GCE_FASTA_MIN_PARALLEL", "0")
    parts = [rng.choice([b"", b"junk\n", b"\n"])]
    for _ in range(int(rng.integers(1, 12))):
        hdr = rng.choice([b">c%d" % rng.integers(0, 6), b">c%d some words" % rng.integers(0, 6), b">", b">>x", b">c\r", b"> lead"])
        parts.append(hdr + b"\n")
        for _ in range(int(rng.integers(0, 40))):
            kind = rng.integers(0, 20)
            if kind == 0:
                parts.append(b"\n" * int(rng.integers(1, 5)))
            elif kind == 1:
                parts.append(b"ac>gt\n")
            elif kind == 2:
                parts.append(b"12 AC-*gtn\r\n")
            else:
                ln = int(rng.integers(1, 70))
                parts.append(bytes(rng.choice(list(b"ACGTNacgtn"), ln).astype(np.uint8)) + b"\n")
    data = b"".join(parts)
    if seed % 3 == 0:
        data = data.rstrip(b"\n")
    if seed % 7 == 0:
        data += b">"
    p = tmp_path / "f.fa"
    p.write_bytes(data)
    want = _fasta_walk_py(data)
    assert _load_fasta_raw(p, 1) == want
    for t in (2, 3, 5, 9):
        assert _load_fasta_raw(p, t) == want


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.gpu
@pytest.mark.parametrize("workload,n_pairs,chunk", [("cfg3", 30000, 7000), ("cfg2", 20000, 1 << 21), ("cfg5", 3000, 1000)])
def test_bam_end_to_end(built, oracle, tmp_path, workload, n_pairs, chunk):
    """A sorted BAM + FASTA on disk -> gce_run_bam (reader, chunked gce_submit_async, engine, writer) -> a BAM whose records,
    parsed independently, are the oracle's; Stats blocks equal."""
    from gencore_amd import synth
    from gencore_amd.bamio import run_bam
    from test_cabi_driver import ascii_of
    d = synth.generate(workload, n_pairs=n_pairs)
    batch = d.to_batch()
    tl = np.asarray(d.target_len, np.uint32)
    prm = default_params(n_targets=len(tl), target_len=tl.ctypes.data, umi_prefix=d.info["umi_prefix"], cluster_size_req=d.info["supporting_reads"])
    ref = d.reference_host()
    want = oracle.run(batch, prm, ref)
    assert want.status == 0
    targets = [("chr%d" % (i + 1), int(l)) for i, l in enumerate(tl)]
    src, out, fa = str(tmp_path / "in.bam"), str(tmp_path / "out.bam"), str(tmp_path / "ref.fa")
    pybam.write_bam(src, records_of(batch), targets)
    with open(fa, "wb") as f:
        for (nm, _), bases in zip(targets, ascii_of(ref)):
            if bases is None:
                continue
            f.write(b">" + nm.encode() + b" synthetic\n")
            for o in range(0, len(bases), 60):
                f.write(bases[o:o + 60] + b"\n")
    prm2 = default_params(umi_prefix="auto", cluster_size_req=d.info["supporting_reads"])
    run = run_bam(src, out, prm2, fasta=fa, threads=4, chunk_reads=chunk)
    assert run.n_reads == batch.n and run.n_out == len(want.emitted())
    assert bytes(run.pre) == bytes(want.pre) and bytes(run.post) == bytes(want.post)
    _, tg, got = pybam.read_bam(out)
    assert tg == targets
    key = lambda r: (r["tid"], r["pos"], r["qname"], r["flag"], r["seq"])
    exp = sorted(({**r, "qname": r["qname"].rstrip("\0")} for r in want.records(batch)), key=key)
    got_sorted = sorted(got, key=key)
    assert [(g["tid"], g["pos"]) for g in got] == sorted((g["tid"], g["pos"]) for g in got)      # the file is coordinate sorted
    for g, e in zip(got_sorted, exp):
        assert (g["qname"], g["flag"], g["tid"], g["pos"], g["seq"], g["qual"]) == (e["qname"], e["flag"], e["tid"], e["pos"], e["seq"], e["qual"])
        assert g["aux"].get("FR", (None, -1))[1] == e["fr"] and g["aux"].get("RR", (None, -1))[1] == e["rr"]
        assert e["nm"] is None or g["aux"]["NM"][1] == e["nm"]


@pytest.mark.gpu
def test_bam_end_to_end_with_mi_tags(built, oracle, tmp_path):
    """MI:Z tags carry the UMIs (src/bamutil.cpp:23-38): the reader hands them on, gce_run_bam takes the staged (not the reserved) submit
    path for such files, and the output still equals the oracle's."""
    from gencore_amd.bamio import run_bam
    import random
    rng = random.Random(11)
    ref = "ACGT" * 500
    recs = []
    for m in range(30):
        left = 100 + 37 * m
        right = left + 200 + rng.randrange(30)
        umi = "".join(rng.choice("ACGT") for _ in range(6))
        for dpl in range(1 + rng.randrange(4)):
            name = "m%02d_%d" % (m, dpl)
            u = umi if rng.random() < 0.8 else umi[:5] + rng.choice("ACGT")
            isz = right + 20 - left
            ls, rs = ref[left:left + 20], ref[right:right + 20]
            recs.append(dict(qname=name, flag=99, tid=0, pos=left, cigar="20M", mtid=0, mpos=right, isize=isz, seq=ls, qual=[rng.choice([37, 25, 11]) for _ in range(20)], nm=0, mi=u))
            recs.append(dict(qname=name, flag=147, tid=0, pos=right, cigar="20M", mtid=0, mpos=left, isize=-isz, seq=rs, qual=[rng.choice([37, 25, 11]) for _ in range(20)], nm=0, mi=u))
    recs.sort(key=lambda r: r["pos"])
    batch = ReadBatch.from_records(recs)
    tl = np.asarray([len(ref)], np.uint32)
    prm = default_params(n_targets=1, target_len=tl.ctypes.data, flush_period=40)
    want = oracle.run(batch, prm, [(oracle.pack_reference(ref), len(ref))])
    assert want.status == 0
    src, out, fa = str(tmp_path / "in.bam"), str(tmp_path / "out.bam"), str(tmp_path / "ref.fa")
    pybam.write_bam(src, recs, [("c0", len(ref))])
    open(fa, "w").write(">c0\n" + ref + "\n")
    run = run_bam(src, out, default_params(flush_period=40), fasta=fa, threads=2, chunk_reads=50)
    assert run.n_reads == batch.n and run.n_out == len(want.emitted())
    assert bytes(run.pre) == bytes(want.pre) and bytes(run.post) == bytes(want.post)
    _, _, got = pybam.read_bam(out)
    key = lambda r: (r["tid"], r["pos"], r["qname"], r["flag"], r["seq"])
    exp = sorted(({**r, "qname": r["qname"].rstrip("\0")} for r in want.records(batch)), key=key)
    for g, e in zip(sorted(got, key=key), exp):
        assert (g["qname"], g["flag"], g["pos"], g["seq"], g["qual"]) == (e["qname"], e["flag"], e["pos"], e["seq"], e["qual"])
        assert g["aux"].get("FR", (None, -1))[1] == e["fr"] and g["aux"]["MI"][0] == "Z"


def _small_pairs(n=12, L=20, ref_len=2000):
    import random
    rng = random.Random(3)
    ref = "".join(rng.choice("ACGT") for _ in range(ref_len))
    recs = []
    for m in range(n):
        left = 50 + 31 * m
        right = left + 120
        isz = right + L - left
        q = [rng.choice([37, 25, 11]) for _ in range(L)]
        recs.append(dict(qname="p%02d" % m, flag=99, tid=0, pos=left, cigar="%dM" % L, mtid=0, mpos=right, isize=isz, seq=ref[left:left + L], qual=q, nm=0))
        recs.append(dict(qname="p%02d" % m, flag=147, tid=0, pos=right, cigar="%dM" % L, mtid=0, mpos=left, isize=-isz, seq=ref[right:right + L], qual=q, nm=0))
    recs.sort(key=lambda r: r["pos"])
    return ref, recs


@pytest.mark.gpu
@pytest.mark.parametrize("damage", ["l_read_name_0", "l_seq_negative", "n_cigar_65535", "tid_out_of_range", "mtid_out_of_range", "l_seq_past_block"])
def test_damaged_record_fields_fail_the_gpu_codec(built, tmp_path, damage):
    """A record whose fields do not fit its block_size (CRCs fine: written that way) must fail gce_run_bam's GPU path with
    GCE_ERR_INVALID and the record's index, as gce_bam_open's "inconsistent record lengths" does on the host -- not read out of range."""
    import struct
    import zlib
    from gencore_amd.bamio import run_bam
    from gencore_amd.capi import GceError
    ref, recs = _small_pairs()
    blobs = [bytearray(pybam.record_bytes(r)) for r in recs]
    k = 5
    b = blobs[k]                                               # [block_size][tid pos l_read_name mapq bin n_cigar flag l_seq mtid mpos isize]...
    if damage == "l_read_name_0":
        b[4 + 8] = 0
    elif damage == "l_seq_negative":
        struct.pack_into("<i", b, 4 + 16, -7)
    elif damage == "n_cigar_65535":
        struct.pack_into("<H", b, 4 + 12, 65535)
    elif damage == "tid_out_of_range":
        struct.pack_into("<i", b, 4 + 0, 3)
    elif damage == "mtid_out_of_range":
        struct.pack_into("<i", b, 4 + 20, 9)
    elif damage == "l_seq_past_block":
        struct.pack_into("<i", b, 4 + 16, 4000)
    text = "@HD\tVN:1.6\tSO:coordinate\n"
    stream = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 3) + b"c0\0" + struct.pack("<i", len(ref))
    stream += b"".join(bytes(x) for x in blobs)
    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(pybam.bgzf_block(stream) + pybam.EOF_BLOCK)
    with pytest.raises(GceError) as ei:
        run_bam(str(src), str(out), default_params(), threads=2)
    assert ei.value.status == -1 and "inconsistent record lengths (record %d)" % k in str(ei.value), str(ei.value)
    # and the same stream undamaged runs
    good = tmp_path / "good.bam"
    pybam.write_bam(str(good), recs, [("c0", len(ref))])
    run = run_bam(str(good), str(out), default_params(), threads=2)
    assert run.n_reads == len(recs)


@pytest.mark.gpu
def test_bam_without_contigs_is_refused(built, tmp_path):
    """src/gencore.cpp:186-189: n_targets == 0 -> "this SAM file has no header"; the BAM branch of gce_run_bam as the SAM-text one."""
    from gencore_amd.bamio import run_bam
    from gencore_amd.capi import GceError
    src = tmp_path / "in.bam"
    pybam.write_bam(str(src), [dict(qname="a", flag=4, tid=-1, pos=-1, cigar="*", mtid=-1, mpos=-1, isize=0, seq="ACGT", qual=[1] * 4, nm=None)], [])
    with pytest.raises(GceError) as ei:
        run_bam(str(src), str(tmp_path / "out.bam"), default_params(), threads=2)
    assert "no header" in str(ei.value)


@pytest.mark.gpu
@pytest.mark.parametrize("hostcodec", [False, True])
def test_sharded_run_with_a_read_over_the_contig_end(built, tmp_path, monkeypatch, hostcodec):
    """A read that overhangs the end of its FASTA contig (the FASTA contig is shorter than @SQ LN): gce_run_bam skips the reference lookup
    (Reference::getData returns NULL, reference.cpp:40,60); the sharded runner's per-shard windows must not fail it either."""
    from gencore_amd.bamio import run_bam, run_bam_sharded
    ref, recs = _small_pairs(n=14, L=20, ref_len=700)
    # the FASTA holds 20 bases less than the header says: the last pair's right read [504+..] stays inside, so push one pair to the very end
    last_left, last_right = 400, 670
    isz = last_right + 20 - last_left
    q = [37] * 20
    recs.append(dict(qname="zz", flag=99, tid=0, pos=last_left, cigar="20M", mtid=0, mpos=last_right, isize=isz, seq=ref[last_left:last_left + 20], qual=q, nm=0))
    recs.append(dict(qname="zz", flag=147, tid=0, pos=last_right, cigar="20M", mtid=0, mpos=last_left, isize=-isz, seq=ref[last_right:last_right + 20], qual=q, nm=0))
    recs.sort(key=lambda r: r["pos"])
    src, fa = tmp_path / "in.bam", tmp_path / "ref.fa"
    pybam.write_bam(str(src), recs, [("c0", len(ref))])
    fa.write_text(">c0\n" + ref[:680] + "\n")                  # pos 670 + 20 = 690 > 680: overhang
    one, two = tmp_path / "one.bam", tmp_path / "two.bam"
    prm = default_params(flush_period=7)
    r1 = run_bam(str(src), str(one), prm, fasta=str(fa), threads=2)
    if hostcodec:                                             # (round 2's runner stages per-shard reference windows: the path ADVICE r3 found failing)
        monkeypatch.setenv("GCE_BAM_HOSTCODEC", "1")
    r2 = run_bam_sharded(str(src), str(two), default_params(flush_period=7), [0, 0, 0], fasta=str(fa), threads=2)
    monkeypatch.delenv("GCE_BAM_HOSTCODEC", raising=False)
    assert r1.n_out == r2.n_out and bytes(r1.pre) == bytes(r2.pre) and bytes(r1.post) == bytes(r2.post)
    a, b = pybam.read_bam(str(one))[2], pybam.read_bam(str(two))[2]
    assert [(x["qname"], x["flag"], x["pos"], x["seq"], x["qual"], x["aux"]) for x in a] == [(x["qname"], x["flag"], x["pos"], x["seq"], x["qual"], x["aux"]) for x in b]
