"""Host-side file formats around the hot path, thin ctypes wrappers over gencore_amd/csrc/bamio.cpp (the
host-only formats) and the runners in its parts, csrc/bamio_run.hpp, bamio_passes.hpp, bamio_index.hpp, bamio_sort.hpp, bamio_calmd.hpp, bamio_overlap.hpp, bamio_umi.hpp, bamio_pileup.hpp, bamio_fragpile.hpp, bamio_errprof.hpp, bamio_fragerr.hpp, bamio_errsup.hpp and bamio_errqual.hpp (the last six over bamio_reduce.hpp) and bamio_varmask.hpp (load_mask, host only):
BamFile (gce_bam_open / gce_bam_chunk: a sorted BAM -> ReadBatch), write_bam (gce_bam_write), load_fasta (gce_fasta_load) and
run_bam (gce_run_bam: BAM in -> engine -> BAM out, with the wall time of every stage).  No htslib."""
import ctypes as C

import numpy as np

from . import capi
from .batch import ReadBatch
from .capi import CORE_DTYPE, GceBamInfo, GceBamRun, GceBatch, GceError


class BamFile:
    def __init__(self, path, threads=0):
        self.lib = capi.load_library()
        self._h = C.c_void_p()
        rc = self.lib.gce_bam_open(str(path).encode(), threads, C.byref(self._h))
        if rc != 0:
            msg = self.lib.gce_bam_error(self._h).decode() if self._h else ""
            self.close()
            raise GceError(rc, msg)
        self.info = GceBamInfo()
        self.lib.gce_bam_get_info(self._h, C.byref(self.info))
        n = self.info.n_targets
        self.target_len = [int(self.info.target_len[i]) for i in range(n)]
        self.target_name = [self.info.target_name[i].decode() for i in range(n)]
        self.text = C.string_at(self.info.text, self.info.l_text).decode() if self.info.l_text else ""
        self.n_records = int(self.info.n_records)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gce_bam_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def chunk_struct(self, first, count, slot=0):
        b = GceBatch()
        rc = self.lib.gce_bam_chunk(self._h, first, count, slot, C.byref(b))
        if rc != 0:
            raise GceError(rc, "gce_bam_chunk")
        return b

    def batch(self, first=0, count=None):
        """Records [first, first+count) as a ReadBatch (copies out of the reader's buffers)."""
        count = self.n_records - first if count is None else count
        b = self.chunk_struct(first, count)

        def arr(ptr, dt, n):
            if n == 0 or not ptr:
                return np.zeros(0, dt)
            return np.frombuffer(C.string_at(ptr, n * np.dtype(dt).itemsize), dt).copy()
        n = count
        mi = bool(b.mi)
        return ReadBatch(core=arr(b.core, CORE_DTYPE, n), qname_off=arr(b.qname_off, np.uint64, n), qname=arr(b.qname, np.uint8, b.qname_bytes),
                         cigar_off=arr(b.cigar_off, np.uint64, n), cigar=arr(b.cigar, np.uint32, b.cigar_words),
                         seq_off=arr(b.seq_off, np.uint64, n), seq=arr(b.seq, np.uint8, b.seq_bytes),
                         qual_off=arr(b.qual_off, np.uint64, n), qual=arr(b.qual, np.uint8, b.qual_bytes),
                         nm=arr(b.nm, np.int32, n), nm_type=arr(b.nm_type, np.uint8, n),
                         mi_off=arr(b.mi_off, np.uint64, n) if mi else None, mi=arr(b.mi, np.uint8, b.mi_bytes) if mi else None)


def load_fasta(path, threads=0):
    """{contig id: ASCII bases (bytes)} in file order, with FastaReader's quirks (src/fastareader.cpp:57-104).
    threads: 0 = all host cores (the file is cut at provable line starts), 1 = the literal one-pass walk."""
    lib = capi.load_library()
    h = C.c_void_p()
    rc = lib.gce_fasta_load(str(path).encode(), int(threads), C.byref(h))
    if rc != 0:
        raise GceError(rc, "gce_fasta_load")
    n = C.c_int32()
    ids, seqs, lens = C.POINTER(C.c_char_p)(), C.POINTER(C.c_void_p)(), C.POINTER(C.c_int64)()
    lib.gce_fasta_get(h, C.byref(n), C.byref(ids), C.byref(seqs), C.byref(lens))
    out = {}
    for i in range(n.value):
        out[ids[i].decode()] = C.string_at(seqs[i], lens[i])
    lib.gce_fasta_free(h)
    return out


def run_bam(in_path, out_path, params, fasta=None, threads=0, chunk_reads=1 << 21, level=6):
    """gce_run_bam: returns the GceBamRun record (stage times, Stats blocks).  level: 0..9 = zlib on the host's threads, -1 = the host's fixed-Huffman encoder, -2 = the GPU deflates the record stream with fixed codes,
    -3 = the GPU deflates it with, per block, the smallest of dynamic codes, fixed codes and stored (never larger than -2)."""
    lib = capi.load_library()
    run = GceBamRun()
    err = (C.c_char * 256)()
    rc = lib.gce_run_bam(str(in_path).encode(), str(out_path).encode(), str(fasta).encode() if fasta else None, C.byref(params), threads,
                         chunk_reads, level, C.byref(run), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return run


def run_bam_sharded(in_path, out_path, params, devices, fasta=None, plan_mode=0, threads=0, level=6):
    """gce_run_bam_sharded: one engine per entry of `devices` (HIP ordinals, may repeat), planned on the GPU, tables merged.  level as run_bam
    (-2 / -3: the merged output is deflated by the GPU)."""
    lib = capi.load_library()
    run = GceBamRun()
    err = (C.c_char * 256)()
    dv = (C.c_int32 * len(devices))(*devices)
    rc = lib.gce_run_bam_sharded(str(in_path).encode(), str(out_path).encode(), str(fasta).encode() if fasta else None, C.byref(params), len(devices), dv,
                                 plan_mode, threads, level, C.byref(run), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return run


def run_bam_depth(in_path, out_path, params, devices, coverage_step, bed=None, fasta=None, plan_mode=0, threads=0, level=6):
    """gce_run_bam_depth: gce_run_bam (one device) / gce_run_bam_sharded (several) with the depth statistics of the reference's report
    (Options::coverageStep, Options::bedFile; level as run_bam, -3 included): returns (run, dict(bin_off, pre_depth, post_depth, regions, pre_bed, post_bed, pre, post, payload_bytes))."""
    from .capi import GceDepthRun
    lib = capi.load_library()
    run, dr = GceBamRun(), GceDepthRun()
    err = (C.c_char * 256)()
    dv = (C.c_int32 * len(devices))(*devices)
    rc = lib.gce_run_bam_depth(str(in_path).encode(), str(out_path).encode(), str(fasta).encode() if fasta else None, str(bed).encode() if bed else None, int(coverage_step),
                               C.byref(params), len(devices), dv, plan_mode, threads, level, C.byref(run), C.byref(dr), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].copy()
    nb, nr = int(dr.n_bins), int(dr.n_regions)
    out = dict(bin_off=arr(dr.bin_off, dr.n_targets + 1), pre_depth=arr(dr.pre_depth, nb), post_depth=arr(dr.post_depth, nb),
               regions=[(dr.region_tid[k], dr.region_start[k], dr.region_end[k]) for k in range(nr)], pre_bed=arr(dr.pre_bed, nr), post_bed=arr(dr.post_bed, nr),
               pre=bytes(dr.pre), post=bytes(dr.post), payload_bytes=int(dr.payload_bytes))
    lib.gce_depth_run_free(C.byref(dr))
    return run, out


def run_bam_passes(in_path, out_path, params, device=0, coverage_step=1000000, bed=None, fasta=None, threads=0, level=6, device_budget_bytes=0, min_passes=0, window_bytes=0):
    """gce_run_bam_passes: run_bam_depth on one device in key-range passes, device memory bounded by the largest pass (device_budget_bytes:
    0 = auto; min_passes forces at least that many; window_bytes: compressed bytes per window, 0 = 64 MB; level as run_bam, -2 / -3: each output piece is
    deflated by the GPU).  Returns (run, depth dict as
    run_bam_depth, pass dict(n_passes, single_pass, reads_per_pass, held_max, peak_device_bytes, budget_bytes, fixed_bytes, pass_room, total_weight,
    key_pass_s, pass_s)))."""
    from .capi import GceDepthRun, GcePassRun
    lib = capi.load_library()
    run, dr, pr = GceBamRun(), GceDepthRun(), GcePassRun()
    err = (C.c_char * 256)()
    rc = lib.gce_run_bam_passes(str(in_path).encode(), str(out_path).encode(), str(fasta).encode() if fasta else None, str(bed).encode() if bed else None, int(coverage_step),
                                C.byref(params), int(device), threads, level, int(device_budget_bytes), int(min_passes), int(window_bytes), C.byref(run), C.byref(dr), C.byref(pr), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].copy()
    nb, nr = int(dr.n_bins), int(dr.n_regions)
    out = dict(bin_off=arr(dr.bin_off, dr.n_targets + 1), pre_depth=arr(dr.pre_depth, nb), post_depth=arr(dr.post_depth, nb),
               regions=[(dr.region_tid[k], dr.region_start[k], dr.region_end[k]) for k in range(nr)], pre_bed=arr(dr.pre_bed, nr), post_bed=arr(dr.post_bed, nr),
               pre=bytes(dr.pre), post=bytes(dr.post), payload_bytes=int(dr.payload_bytes))
    lib.gce_depth_run_free(C.byref(dr))
    P = int(pr.n_passes)
    passes = dict(n_passes=P, single_pass=bool(pr.single_pass), reads_per_pass=[int(pr.reads_per_pass[k]) for k in range(P)], held_max=int(pr.held_max),
                  peak_device_bytes=int(pr.peak_device_bytes), budget_bytes=int(pr.budget_bytes), fixed_bytes=int(pr.fixed_bytes), pass_room=int(pr.pass_room), total_weight=int(pr.total_weight), key_pass_s=float(pr.key_pass_s), pass_s=[float(pr.pass_s[k]) for k in range(P)])
    return run, out, passes


def index_bam(bam, bai=None, device=0, threads=0, window_bytes=0):
    """gce_bam_index: the BAI index of a coordinate-sorted BAM file, built on the GPU, written to `bai` (default: bam + ".bai").  window_bytes:
    compressed bytes per window, 0 = 64 MB.  Returns dict(n_records, n_no_coor, n_bins, n_chunks, n_intervals, n_ref, read_s, gpu_s, write_s,
    total_s); raises GceError (and leaves no index) on failure."""
    from .capi import GceBaiRun
    lib = capi.load_library()
    bai = str(bam) + ".bai" if bai is None else str(bai)
    r = GceBaiRun()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_index(str(bam).encode(), bai.encode(), int(device), int(threads), int(window_bytes), C.byref(r), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return {n: (float if t is C.c_double else int)(getattr(r, n)) for n, t in GceBaiRun._fields_ if n != "pad"}


def sort_bam(bam, out, device=0, threads=0, level=-2, window_bytes=0, device_budget_bytes=0):
    """gce_bam_sort: an unsorted BAM file into coordinate order on the GPU (what `samtools sort` does in front of the reference), written to
    `out`.  level as run_bam; window_bytes: compressed bytes per window, 0 = 64 MB; device_budget_bytes: 0 = no limit beyond the device (the
    sort is in-core; sort_bam_passes takes a file beyond that).  Returns dict(n_records, n_no_coor, n_descents, inflated_bytes, out_bytes, peak_device_bytes, n_ref, read_s,
    inflate_index_s, sort_s, gather_s, write_s, total_s); raises GceError (and leaves no output) on failure."""
    from .capi import GceSortRun
    lib = capi.load_library()
    r = GceSortRun()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_sort(str(bam).encode(), str(out).encode(), int(device), int(threads), int(level), int(window_bytes), int(device_budget_bytes), C.byref(r), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return {n: (float if t is C.c_double else int)(getattr(r, n)) for n, t in GceSortRun._fields_ if n != "pad"}


class CalmdRun:
    """gce_calmd_run as an object: one attribute per field (counters and bytes as int, times as float); calmd_bam_stream adds the fields of
    gce_calmd_stream_run (n_flushes, resident_cap_bytes, flushed_bytes)."""

    def __init__(self, r, stream=None):
        for s in (r,) if stream is None else (r, stream):
            for n, t in type(s)._fields_:
                if n != "pad":
                    setattr(self, n, (float if t is C.c_double else int)(getattr(s, n)))

    def as_dict(self):
        return dict(vars(self))


def calmd_bam(in_path, out_path, fasta, device=0, threads=0, level=6, window_bytes=0, device_budget_bytes=0):
    """gce_bam_calmd: NM and MD of every record of a BAM file recomputed against `fasta` on the GPU (what `samtools calmd` does behind the
    reference, whose consensus records keep one read's MD), written to `out_path`; records the rules leave alone (unmapped, no CIGAR, a contig
    the FASTA lacks, ...) and the header are copied byte for byte, in the input's order.  level as run_bam; window_bytes: compressed bytes per
    window, 0 = 64 MB; device_budget_bytes: 0 = no limit beyond the device (the pass is in-core).  Returns a CalmdRun (n_records, n_rewritten,
    n_unchanged, n_no_ref, n_nm_changed, n_md_changed, inflated_bytes, out_record_bytes, out_bytes, peak_device_bytes, n_ref, read_s,
    inflate_index_s, calmd_s, write_s, total_s); raises GceError with the library's message (and leaves no output) on failure."""
    from .capi import GceCalmdRun
    lib = capi.load_library()
    r = GceCalmdRun()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_calmd(str(in_path).encode(), str(out_path).encode(), str(fasta).encode(), int(device), int(threads), int(level), int(window_bytes), int(device_budget_bytes),
                           C.byref(r), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return CalmdRun(r)


def calmd_bam_stream(in_path, out_path, fasta, device=0, threads=0, level=6, window_bytes=0, device_budget_bytes=0, resident_bytes=0):
    """gce_bam_calmd_stream: calmd_bam's file, byte for byte, for an input of any size: the rewritten records leave the device in whole BGZF
    members as soon as the next window's output would take the resident ones past the cap, so the device holds the reference bases + one
    window + 40 bytes per window record + one piece's deflate buffers + at least one window's output.  device_budget_bytes: 0 = auto (a
    fraction of the free device memory, as sort_bam_passes); resident_bytes: 0 = the cap is what the budget leaves, otherwise the cap,
    rounded up to a multiple of 0xff00 (forces flushes on a small file).  Returns calmd_bam's CalmdRun with n_flushes, resident_cap_bytes
    and flushed_bytes added; raises GceError with the library's message (and leaves no output) on failure."""
    from .capi import GceCalmdRun, GceCalmdStreamRun
    lib = capi.load_library()
    r, sr = GceCalmdRun(), GceCalmdStreamRun()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_calmd_stream(str(in_path).encode(), str(out_path).encode(), str(fasta).encode(), int(device), int(threads), int(level), int(window_bytes),
                                  int(device_budget_bytes), int(resident_bytes), C.byref(r), C.byref(sr), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return CalmdRun(r, sr)


def merge_overlap_bam(in_path, out_path, device=0, threads=0, level=-2, min_mapq=0, exclude_flags=0x704, weak_hash=False, window_bytes=0, device_budget_bytes=0):
    """gce_bam_merge_overlap: the QUAL bytes of overlapping mates of a coordinate-sorted BAM rewritten on the GPU so that a plain pileup of
    `out_path` counts every fragment once: where the mates agree the earlier one carries min(qa + qb, 93) and the later one 0,
    where they disagree the better base keeps (4 q) / 5 and the other gets 0.  Nothing but QUAL bytes changes; the header and the record order
    stay.  level as run_bam; weak_hash: the join keeps 4 bits of its hash (a test's switch); window_bytes: compressed bytes per window,
    0 = 64 MB; device_budget_bytes: 0 = no limit beyond the device (the pass is in-core).  Returns a CalmdRun-like object (n_records, n_pairs,
    n_pairs_no_qual, n_ambiguous, n_shared_columns, n_disagree_columns, n_columns_skipped, n_records_changed, inflated_bytes, out_bytes,
    peak_device_bytes, n_ref, read_s, inflate_index_s, merge_s, write_s, total_s); raises GceError with the library's message (and leaves no
    output) on failure."""
    from .capi import GCE_OVERLAP_WEAK_HASH, GceOverlapRun
    lib = capi.load_library()
    r = GceOverlapRun()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_merge_overlap(str(in_path).encode(), str(out_path).encode(), int(device), int(threads), int(level), int(window_bytes), int(device_budget_bytes), int(min_mapq),
                                   int(exclude_flags), GCE_OVERLAP_WEAK_HASH if weak_hash else 0, C.byref(r), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return CalmdRun(r)


class UmiRun:
    """gce_umi_run as an object: one attribute per field (counters and bytes as int, times as float)."""

    def __init__(self, r):
        for n, t in type(r)._fields_:
            setattr(self, n, (float if t is C.c_double else int)(getattr(r, n)))

    def as_dict(self):
        return dict(vars(self))


def umi_to_mi(in_path, out_path, source="RX", device=0, threads=0, level=-2, window_bytes=0, device_budget_bytes=0, resident_bytes=0):
    """gce_bam_umi_to_mi: the UMI of every record of a BAM file, from the Z field tagged `source` (RX: fgbio, DRAGEN, `bwa mem -C`) or from the
    last `:`-field of the read name (source="name": bcl-convert's ...:ACGT+TTGA), into an MI:Z field in the form the run reads
    (src/bamutil.cpp:23-38): upper case, `-` and `+` as `_`, behind a `:`; MI fields the record had are dropped, everything else is kept.  A
    record without such a field, or whose string is not a UMI (a byte other than ACGTNacgtn-+_, more than one separator, one at either end,
    more than 250 bytes), is copied whole.  Streamed as calmd_bam_stream within device_budget_bytes (0 = auto); resident_bytes forces the
    cap on resident output.  Returns a UmiRun (n_records, n_tagged, n_no_source, n_not_umi, n_mi_dropped, n_flushes, inflated_bytes,
    out_record_bytes, out_bytes, peak_device_bytes, read_s, inflate_index_s, umi_s, write_s, total_s); raises GceError with the library's
    message (and leaves no output) on failure."""
    from .capi import GceUmiRun
    lib = capi.load_library()
    r = GceUmiRun()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_umi_to_mi(str(in_path).encode(), str(out_path).encode(), str(source).encode(), int(device), int(threads), int(level), int(window_bytes),
                               int(device_budget_bytes), int(resident_bytes), C.byref(r), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    return UmiRun(r)


class PileupRun:
    """gce_pileup_run or gce_fragpile_run as an object: the counters and bytes as int, the times as float, and the numpy arrays tid, pos ([n_sites], 0-based) and
    counts ([n_sites, 2 strands, 8 classes]: A C G T N DEL INS LOWQ)."""
    CLASSES = ("A", "C", "G", "T", "N", "DEL", "INS", "LOWQ")

    def __init__(self, r):
        _copy_run_fields(self, r)
        ns = self.n_sites
        self.tid = np.ctypeslib.as_array(r.site_tid, (ns,)).copy() if ns else np.zeros(0, np.int32)
        self.pos = np.ctypeslib.as_array(r.site_pos, (ns,)).copy() if ns else np.zeros(0, np.int32)
        self.counts = (np.ctypeslib.as_array(r.counts, (ns * 16,)).copy() if ns else np.zeros(0, np.uint32)).reshape(ns, 2, 8)

    def as_dict(self):
        return {k: v for k, v in vars(self).items() if k not in ("tid", "pos", "counts")}


def pileup_bam(path, bed, fasta=None, tsv=None, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704, direct=False, window_bytes=0, device_budget_bytes=0):
    """gce_bam_pileup: bases per strand at the sites of `bed` (the union of its regions, clamped to the contigs of the BAM's header), counted on
    the GPU over every record with mapq >= min_mapq and no bit of exclude_flags, in any record order: per site and strand A C G T N DEL INS and
    LOWQ (a base whose quality is below min_baseq).  tsv: the table's path (contig, 1-based pos, ref, depth, 16 counters; ref from `fasta`, N
    without it), or None for no file.  direct=True makes every add a global atomic instead of meeting in the kernel's LDS tile: the same
    counters.  Returns a PileupRun (n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar, n_sites,
    n_intervals, peak_device_bytes, read_s, inflate_index_s, pileup_s, write_s, total_s, tid, pos, counts); raises GceError with the library's
    message (and leaves no table) on failure."""
    from .capi import GCE_PILEUP_DIRECT, GcePileupRun
    return _reduce_call("gce_bam_pileup", GcePileupRun, PileupRun, "gce_pileup_free", (str(path), str(bed), fasta, tsv), GCE_PILEUP_DIRECT if direct else 0, device, threads, min_mapq, min_baseq,
                        exclude_flags, window_bytes, device_budget_bytes)


def pileup_fragments_bam(path, bed, fasta=None, tsv=None, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704, direct=False, weak_hash=False, window_bytes=0,
                         device_budget_bytes=0):
    """gce_bam_pileup_fragments: pileup_bam's table over a coordinate-sorted BAM with every fragment counted once where its mates overlap (as
    `samtools mpileup` resolves the overlap, in outline): at a site that both mates of a pair cover, one of them is counted -- the earlier in
    the file where they agree (its quality the sum, at most 200), the one of higher quality where they differ (its quality times 4 / 5).  A
    record without a partner is counted as pileup_bam counts it.  weak_hash=True keeps 4 bits of the join's hash: the same counters, for
    tests.  Returns a PileupRun with pileup_bam's fields plus n_pairs, n_shared_columns, n_disagree_columns, n_ambiguous and n_deferred (the
    records carried across a window boundary: the one counter that depends on window_bytes); raises GceError with the library's message (and
    leaves no table) on failure, a record that lies in front of its predecessor among them."""
    from .capi import GCE_FRAGPILE_DIRECT, GCE_FRAGPILE_WEAK_HASH, GceFragpileRun
    return _reduce_call("gce_bam_pileup_fragments", GceFragpileRun, PileupRun, "gce_fragpile_free", (str(path), str(bed), fasta, tsv),
                        (GCE_FRAGPILE_DIRECT if direct else 0) | (GCE_FRAGPILE_WEAK_HASH if weak_hash else 0), device, threads, min_mapq, min_baseq, exclude_flags, window_bytes,
                        device_budget_bytes)


def _copy_run_fields(obj, r, mask=None):
    """The scalar fields of a gce_*_run onto obj, the counters and bytes as int, the times as float; with `mask`, gce_mask_run's fields too:
    n_records and n_intervals are the BAM's and the BED's, so the mask's are n_mask_records and n_mask_intervals."""
    for n, t in type(r)._fields_:
        if n not in ("site_tid", "site_pos", "counts", "overlap"):
            setattr(obj, n, (float if t is C.c_double else int)(getattr(r, n)))
    if mask is not None:
        for n, t in type(mask)._fields_:
            setattr(obj, {"n_intervals": "n_mask_intervals", "n_records": "n_mask_records"}.get(n, n), (float if t is C.c_double else int)(getattr(mask, n)))


def _reduce_call(entry, run_type, wrap, free, paths, options, device, threads, min_mapq, min_baseq, exclude_flags, window_bytes, device_budget_bytes, masked=False):
    """One pileup or error-profile entry point of the library: `paths` are its leading arguments (None for an optional path that is absent),
    behind them the common ones, its gce_*_run, with `masked` a gce_mask_run, and err.  Returns wrap(run[, mask run]); the run's arrays
    are freed with `free` either way."""
    from .capi import GceMaskRun
    lib = capi.load_library()
    r, m = run_type(), GceMaskRun() if masked else None
    err = (C.c_char * 256)()
    rc = getattr(lib, entry)(*[None if x is None else str(x).encode() for x in paths], int(device), int(threads), int(min_mapq), int(min_baseq), int(exclude_flags), int(options), int(window_bytes), int(device_budget_bytes),
                             C.byref(r), *([C.byref(m)] if masked else []), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    try:
        return wrap(r, m) if masked else wrap(r)
    finally:
        getattr(lib, free)(C.byref(r))


class ErrorProfileRun:
    """gce_errprof_run as an object: the counters and bytes as int, the times as float, and the numpy array counts ([3 segments, 1024 cycles,
    24 classes], uint64: classes 0..15 are 4 r + b over A C G T in sequencing orientation, then READ_N REF_OTHER LOWQ INS DEL and three zeros)."""
    CLASSES = tuple("%s>%s" % (r, b) for r in "ACGT" for b in "ACGT") + ("READ_N", "REF_OTHER", "LOWQ", "INS", "DEL")

    def __init__(self, r, mask=None):
        from .capi import GCE_ERRPROF_CLASSES, GCE_ERRPROF_MAX_CYCLE
        _copy_run_fields(self, r, mask)
        table = lambda p: np.ctypeslib.as_array(p, (3 * GCE_ERRPROF_MAX_CYCLE * GCE_ERRPROF_CLASSES,)).copy().reshape(3, GCE_ERRPROF_MAX_CYCLE, GCE_ERRPROF_CLASSES)
        self.counts = table(r.counts)
        if hasattr(r, "overlap"):
            self.overlap = table(r.overlap)

    def as_dict(self):
        return {k: v for k, v in vars(self).items() if k not in ("counts", "overlap")}


def error_profile_bam(path, fasta, bed=None, tsv=None, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704, direct=False, window_bytes=0, device_budget_bytes=0):
    """gce_bam_error_profile: per segment of the pair (0: neither or both of 0x40 / 0x80, 1: first, 2: last) and sequencing cycle, the 4 x 4
    table of reference base against read base in read orientation, and the read-N, unusable-reference, low-quality, inserted-base and deletion
    counts, counted on the GPU over every record with mapq >= min_mapq and no bit of exclude_flags, in any record order, against the contigs of
    `fasta` matched by name.  bed: restrict the events to the union of its regions.  tsv: the table's path (segment, cycle, bases, mismatches,
    the 21 counters; integers, no rates), or None for no file.  direct=True makes every add a 64-bit global atomic instead of meeting in the
    kernel's LDS planes: the same counters.  Returns an ErrorProfileRun (n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar,
    n_no_seq, n_bad_cigar, n_no_ref, n_too_long, n_bases, n_mismatches, n_intervals (-1 without a BED), peak_device_bytes, read_s,
    inflate_index_s, errprof_s, write_s, total_s, counts); raises GceError with the library's message (and leaves no table) on failure."""
    from .capi import GCE_ERRPROF_DIRECT, GceErrprofRun
    return _reduce_call("gce_bam_error_profile", GceErrprofRun, ErrorProfileRun, "gce_errprof_free", (str(path), str(fasta), bed, tsv), GCE_ERRPROF_DIRECT if direct else 0, device, threads,
                        min_mapq, min_baseq, exclude_flags, window_bytes, device_budget_bytes)


def error_profile_masked_bam(path, fasta, mask, bed=None, tsv=None, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704, direct=False, window_bytes=0, device_budget_bytes=0):
    """gce_bam_error_profile_masked: error_profile_bam with the known variant sites of `mask` (a .vcf, .vcf.gz or .bed, read as load_mask reads
    it) taken out of every class: an event whose anchor -- a column's own position, the position in front of an inserted base, a deletion's
    first position -- is masked goes to class 21, MASKED, at its segment and cycle, and the table gets a trailing MASKED column.  n_bases and
    n_mismatches are then the sequencer's and the polymerase's, not the sample's genotype.  Returns an ErrorProfileRun with error_profile_bam's
    fields plus gce_mask_run's: n_lines, n_mask_records, n_unknown_contig, n_no_alt, n_mask_intervals, n_masked_bases, n_masked_events, load_s and
    fill_s."""
    from .capi import GCE_ERRPROF_DIRECT, GceErrprofRun
    return _reduce_call("gce_bam_error_profile_masked", GceErrprofRun, ErrorProfileRun, "gce_errprof_free", (str(path), str(fasta), bed, str(mask), tsv), GCE_ERRPROF_DIRECT if direct else 0, device,
                        threads, min_mapq, min_baseq, exclude_flags, window_bytes, device_budget_bytes, masked=True)


OVERLAP_CLASSES = ErrorProfileRun.CLASSES[:16] + ("AGREE_REF", "AGREE_ALT", "DIFF_OTHER", "UNUSABLE", "LOWQ")


def error_profile_fragments_bam(path, fasta, bed=None, tsv=None, overlap_tsv=None, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704, direct=False, weak_hash=False,
                                window_bytes=0, device_budget_bytes=0):
    """gce_bam_error_profile_fragments: error_profile_bam's table over a coordinate-sorted BAM with every fragment counted once where its mates
    overlap -- at a reference position that an M / = / X op of both mates of a pair covers, one of them is counted, chosen as
    pileup_fragments_bam chooses it -- and a second table, `overlap` (classes OVERLAP_CLASSES), to which both mates add there, each at its
    own segment and cycle: AGREE_REF, AGREE_ALT (both read the same base and it is not the reference's: older than the sequencer, or a
    variant), r>b with r != b (this mate's sequencing error: the partner reads the reference base), r>r (this mate read it right, the partner
    did not), DIFF_OTHER, UNUSABLE (an N, or no usable reference base) and LOWQ (a raw quality below min_baseq).  overlap.sum() is twice
    n_shared_columns.  tsv, overlap_tsv: the tables' paths, or None.  direct, weak_hash as pileup_fragments_bam takes them.  Returns an
    ErrorProfileRun with error_profile_bam's fields plus n_pairs, n_shared_columns, n_disagree_columns, n_ambiguous, n_deferred and overlap
    ([3, 1024, 24], uint64); raises GceError with the library's message (and leaves no table) on failure, a record that lies in front of its
    predecessor among them."""
    from .capi import GCE_FRAGERR_DIRECT, GCE_FRAGERR_WEAK_HASH, GceFragerrRun
    return _reduce_call("gce_bam_error_profile_fragments", GceFragerrRun, ErrorProfileRun, "gce_fragerr_free", (str(path), str(fasta), bed, tsv, overlap_tsv),
                        (GCE_FRAGERR_DIRECT if direct else 0) | (GCE_FRAGERR_WEAK_HASH if weak_hash else 0), device, threads, min_mapq, min_baseq, exclude_flags, window_bytes,
                        device_budget_bytes)


def error_profile_fragments_masked_bam(path, fasta, mask, bed=None, tsv=None, overlap_tsv=None, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704, direct=False,
                                       weak_hash=False, window_bytes=0, device_budget_bytes=0):
    """gce_bam_error_profile_fragments_masked: error_profile_fragments_bam under error_profile_masked_bam's mask.  At a shared masked column the
    one mate that is counted adds MASKED to counts and both add class 21, OVL_MASKED, to overlap; overlap.sum() is still twice
    n_shared_columns.  Both tables get the trailing MASKED column.  Returns error_profile_fragments_bam's ErrorProfileRun with
    error_profile_masked_bam's mask fields."""
    from .capi import GCE_FRAGERR_DIRECT, GCE_FRAGERR_WEAK_HASH, GceFragerrRun
    return _reduce_call("gce_bam_error_profile_fragments_masked", GceFragerrRun, ErrorProfileRun, "gce_fragerr_free", (str(path), str(fasta), bed, str(mask), tsv, overlap_tsv),
                        (GCE_FRAGERR_DIRECT if direct else 0) | (GCE_FRAGERR_WEAK_HASH if weak_hash else 0), device, threads, min_mapq, min_baseq, exclude_flags, window_bytes,
                        device_budget_bytes, masked=True)


class ErrorProfileSupportRun:
    """gce_errsup_run as an object: the counters and bytes as int, the times as float, and the numpy array counts ([3 segments, 33 forward
    buckets, 33 reverse buckets, 24 classes], uint64: bucket 0 is an absent tag, 1..31 the value, 32 every other value; classes 0..20 are
    ErrorProfileRun.CLASSES, 21 MASKED, 22 RECORDS, 23 zero).  With a mask, gce_mask_run's fields as ErrorProfileRun names them."""
    CLASSES = ErrorProfileRun.CLASSES + ("MASKED", "RECORDS")

    def __init__(self, r, mask=None):
        from .capi import GCE_ERRPROF_CLASSES, GCE_ERRSUP_BUCKETS
        _copy_run_fields(self, r, mask)
        shape = (3, GCE_ERRSUP_BUCKETS, GCE_ERRSUP_BUCKETS, GCE_ERRPROF_CLASSES)
        self.counts = np.ctypeslib.as_array(r.counts, (int(np.prod(shape)),)).copy().reshape(shape)

    def as_dict(self):
        return {k: v for k, v in vars(self).items() if k != "counts"}


def error_profile_support_bam(path, fasta, mask=None, bed=None, tsv=None, tags=("FR", "RR"), direct=False, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704,
                              window_bytes=0, device_budget_bytes=0):
    """gce_bam_error_profile_support: error_profile_bam's classes, walk, BED and (with `mask`, as error_profile_masked_bam takes it) variant
    mask, tabulated not by cycle but by the support of each consensus record: f, the value of its first `tags[0]` field (FR, the forward-strand
    reads merged into it), and r, that of its first `tags[1]` field (RR, written on duplex records alone), each as a bucket: 0 absent (or not
    of an integer type), 1..31 the value, 32 every other value.  A run at -s 1 profiled this way shows the residual error of FR = 1 (no
    consensus), 2, 3, ... and of duplex against single-strand records from one file: the choice of -s and of duplex-only.  Any BAM is taken;
    tags=("aD", "bD") reads fgbio's duplex depths.  A record whose optional fields cannot be walked is counted in n_bad_aux and left out.
    tsv: the table's path (segment, forward, reverse, records, bases, mismatches, the 21 counters, MASKED with a mask; one row per (segment,
    forward, reverse) with a counter), or None.  direct=True makes every add a 64-bit global atomic instead of collecting a record's adds on
    chip: the same counters.  Returns an ErrorProfileSupportRun (error_profile_bam's totals plus n_bad_aux, n_with_forward, n_with_reverse and
    counts [3, 33, 33, 24]); raises GceError with the library's message (and leaves no table) on failure."""
    from .capi import GCE_ERRSUP_DIRECT, GceErrsupRun, GceMaskRun
    lib = capi.load_library()
    r, m = GceErrsupRun(), GceMaskRun()
    err = (C.c_char * 256)()
    enc = lambda x: None if x is None else str(x).encode()
    if isinstance(tags, (str, bytes)) or len(tags) != 2 or any(not isinstance(t, str) or len(t.encode("latin-1", "replace")) != 2 for t in tags):
        raise ValueError("tags should be two two-character tags")
    rc = lib.gce_bam_error_profile_support(str(path).encode(), str(fasta).encode(), enc(bed), enc(mask), enc(tsv), (tags[0] + tags[1]).encode("latin-1", "replace"), int(device), int(threads),
                                           int(min_mapq), int(min_baseq), int(exclude_flags), GCE_ERRSUP_DIRECT if direct else 0, int(window_bytes), int(device_budget_bytes), C.byref(r),
                                           None if mask is None else C.byref(m), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    try:
        return ErrorProfileSupportRun(r, None if mask is None else m)
    finally:
        lib.gce_errsup_free(C.byref(r))


class ErrorProfileQualityRun:
    """gce_errqual_run as an object: the counters and bytes as int, the times as float, and the numpy array counts ([3 segments, 96 quality
    buckets, 24 classes], uint64: bucket 0..93 is the QUAL byte, 94 every other byte, 95 a record without qualities; classes 0..20 are
    ErrorProfileRun.CLASSES, 21 MASKED, 22 and 23 zero).  With a mask, gce_mask_run's fields as ErrorProfileRun names them."""
    CLASSES = ErrorProfileRun.CLASSES + ("MASKED",)

    def __init__(self, r, mask=None):
        from .capi import GCE_ERRPROF_CLASSES, GCE_ERRQUAL_BUCKETS
        _copy_run_fields(self, r, mask)
        shape = (3, GCE_ERRQUAL_BUCKETS, GCE_ERRPROF_CLASSES)
        self.counts = np.ctypeslib.as_array(r.counts, (int(np.prod(shape)),)).copy().reshape(shape)

    def as_dict(self):
        return {k: v for k, v in vars(self).items() if k != "counts"}


def error_profile_quality_bam(path, fasta, mask=None, bed=None, tsv=None, direct=False, device=0, threads=0, min_mapq=0, min_baseq=0, exclude_flags=0x704, window_bytes=0,
                              device_budget_bytes=0):
    """gce_bam_error_profile_quality: error_profile_bam's classes, walk, BED and (with `mask`, as error_profile_masked_bam takes it) variant
    mask, tabulated not by cycle but by the base quality the file reports: of the bases at quality q, how many differ from the reference.
    Over the input it holds the sequencer's qualities against an error rate, over the consensus output the qualities the consensus step
    wrote.  The bucket of an event is the QUAL byte of its query base (an inserted base's own, a deletion's the base in front of it):
    0..93 as it is, 94 every other byte, 95 for a record without qualities.  Summed over the buckets the table is error_profile_bam's summed
    over the cycles.  tsv: the table's path (segment, quality (the number, `94+` or `.`), bases, mismatches, the 21 counters, MASKED with a
    mask; one row per (segment, quality) with a counter), or None.  direct=True makes every add a 64-bit global atomic instead of meeting
    in the kernel's table on chip: the same counters.  Returns an ErrorProfileQualityRun (error_profile_bam's totals and counts [3, 96,
    24]); raises GceError with the library's message (and leaves no table) on failure."""
    from .capi import GCE_ERRQUAL_DIRECT, GceErrqualRun, GceMaskRun
    lib = capi.load_library()
    r, m = GceErrqualRun(), GceMaskRun()
    err = (C.c_char * 256)()
    enc = lambda x: None if x is None else str(x).encode()
    rc = lib.gce_bam_error_profile_quality(str(path).encode(), str(fasta).encode(), enc(bed), enc(mask), enc(tsv), int(device), int(threads), int(min_mapq), int(min_baseq),
                                           int(exclude_flags), GCE_ERRQUAL_DIRECT if direct else 0, int(window_bytes), int(device_budget_bytes), C.byref(r),
                                           None if mask is None else C.byref(m), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    try:
        return ErrorProfileQualityRun(r, None if mask is None else m)
    finally:
        lib.gce_errqual_free(C.byref(r))


def load_mask(path, names, lens, threads=0):
    """gce_mask_load: the variant mask `path` (.vcf, .vcf.gz as gzip or BGZF, or .bed) against the contig names, clamped to lens (per contig
    min(header length, FASTA length); <= 0: no reference bases, its intervals are dropped), sorted and merged.  No device is touched.
    -> dict(n_lines, n_records, n_unknown_contig, n_no_alt, n_intervals, n_masked_bases, intervals=[(tid, start, end)]); raises GceError with
    `variant mask line N: ...` for a malformed line."""
    from .capi import GceMask
    lib = capi.load_library()
    m = GceMask()
    err = (C.c_char * 256)()
    n = len(names)
    cn = (C.c_char_p * max(n, 1))(*[x.encode() if isinstance(x, str) else x for x in names])
    cl = (C.c_int64 * max(n, 1))(*[int(x) for x in lens])
    rc = lib.gce_mask_load(str(path).encode(), n, cn, cl, int(threads), C.byref(m), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    try:
        d = {k: int(getattr(m, k)) for k, _ in GceMask._fields_[:6]}
        d["intervals"] = [(int(m.tid[k]), int(m.start[k]), int(m.end[k])) for k in range(d["n_intervals"])]
        return d
    finally:
        lib.gce_mask_free(C.byref(m))


def sort_sam(sam, out, device=0, threads=0, level=-2, window_bytes=0, device_budget_bytes=0):
    """gce_sam_sort: SAM text in any order into the coordinate-sorted BAM on the GPU, the file sam_to_bam + sort_bam write, without the BAM in
    between: the GPU turns the alignment lines into records (parse_sam) and sorts them.  window_bytes: text bytes per window, 0 = 64 MB, a value above 1 GB
    is taken as 1 GB (line starts are 32-bit offsets into the window), and a window grows to hold one line; in-core only (sam_to_bam, then sort_bam_passes, take a file beyond device_budget_bytes).  Returns sort_bam's dict plus n_host_lines (the
    lines with floating-point values, which the host re-parsed); raises GceError (and leaves no output) on failure."""
    from .capi import GceSortRun
    lib = capi.load_library()
    r = GceSortRun()
    nh = C.c_int64(0)
    err = (C.c_char * 256)()
    rc = lib.gce_sam_sort(str(sam).encode(), str(out).encode(), int(device), int(threads), int(level), int(window_bytes), int(device_budget_bytes), C.byref(r), C.byref(nh), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    d = {n: (float if t is C.c_double else int)(getattr(r, n)) for n, t in GceSortRun._fields_ if n != "pad"}
    d["n_host_lines"] = int(nh.value)
    return d


def parse_sam(text, ref_names, device=0, out_cap=None):
    """gce_sam_parse: the alignment lines of `text` (bytes, no `@` lines) as BAM records, made on the GPU.  Returns dict(records (bytes),
    n_records, n_host_lines); raises GceError -- .bad_line is the first malformed line, counting from 0 over the lines that are records, and
    .needed the bytes a too small out_cap should have been."""
    lib = capi.load_library()
    text = bytes(text)
    names = (C.c_char_p * max(len(ref_names), 1))(*[n.encode() if isinstance(n, str) else n for n in ref_names])
    cap = len(text) * 2 + 64 * (text.count(b"\n") + 2) if out_cap is None else int(out_cap)
    out = np.empty(max(cap, 1), np.uint8)
    ob, nr, nh, bad = C.c_size_t(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    err = (C.c_char * 256)()
    rc = lib.gce_sam_parse(int(device), text, len(text), len(ref_names), names, out.ctypes.data, cap, C.byref(ob), C.byref(nr), C.byref(nh), C.byref(bad), err)
    if rc != 0:
        e = GceError(rc, err.value.decode(errors="replace"))
        e.bad_line, e.needed = int(bad.value), int(ob.value)
        raise e
    return dict(records=out[:ob.value].tobytes(), n_records=int(nr.value), n_host_lines=int(nh.value))


def format_sam(records, ref_names, device=0, out_cap=None):
    """gce_sam_format: whole BAM records (bytes, block_size first, back to back) as SAM alignment lines, made on the GPU.  Returns dict(text
    (bytes), n_records, n_host_records); raises GceError -- .bad_record is the first record the writer refuses, counting from 0, and .needed
    the bytes a too small out_cap should have been."""
    lib = capi.load_library()
    rec = np.frombuffer(bytes(records), np.uint8)
    names = (C.c_char_p * max(len(ref_names), 1))(*[n.encode() if isinstance(n, str) else n for n in ref_names])
    ob, nr, nh, bad = C.c_size_t(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    err = (C.c_char * 256)()
    if out_cap is None:                                        # the size first: a line may be many times its record (a B array of small values)
        rc = lib.gce_sam_format(int(device), rec.ctypes.data if len(rec) else None, len(rec), len(ref_names), names, None, 0, C.byref(ob), C.byref(nr), C.byref(nh), C.byref(bad), err)
        cap = int(ob.value)
    else:
        rc, cap = -4, int(out_cap)
    out = np.empty(max(cap, 1), np.uint8)
    if rc == -4:
        rc = lib.gce_sam_format(int(device), rec.ctypes.data if len(rec) else None, len(rec), len(ref_names), names, out.ctypes.data, cap, C.byref(ob), C.byref(nr), C.byref(nh), C.byref(bad), err)
    if rc != 0:
        e = GceError(rc, err.value.decode(errors="replace"))
        e.bad_record, e.needed = int(bad.value), int(ob.value)
        raise e
    return dict(text=out[:ob.value].tobytes(), n_records=int(nr.value), n_host_records=int(nh.value))


def sam_format_counters():
    """gce_get_sam_format_counters: [records formatted on the device, records the host formatted for it, formatter runs, text bytes] of this
    process."""
    lib = capi.load_library()
    out = (C.c_int64 * 4)()
    lib.gce_get_sam_format_counters(out)
    return [int(x) for x in out]


def sort_bam_passes(bam, out, device=0, threads=0, level=-2, window_bytes=0, device_budget_bytes=0, min_passes=0):
    """gce_bam_sort_passes: sort_bam for a file of any size: in-core when that fits device_budget_bytes (0 = auto, a fraction of the free device
    memory) and min_passes <= 1, otherwise in output-range passes over the file (at least min_passes of them); the output's bytes are
    sort_bam's.  Returns sort_bam's dict plus n_passes, in_core, pass_bytes, resident_bytes, key_pass_s, plan_s and pass_s (a list of n_passes
    entries); raises GceError (and leaves no output) on failure."""
    from .capi import GceSortPassRun, GceSortRun
    lib = capi.load_library()
    r, pr = GceSortRun(), GceSortPassRun()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_sort_passes(str(bam).encode(), str(out).encode(), int(device), int(threads), int(level), int(window_bytes), int(device_budget_bytes), int(min_passes),
                                 C.byref(r), C.byref(pr), err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))
    d = {n: (float if t is C.c_double else int)(getattr(r, n)) for n, t in GceSortRun._fields_ if n != "pad"}
    P = int(pr.n_passes)
    d.update(n_passes=P, in_core=int(pr.in_core), pass_bytes=int(pr.pass_bytes), resident_bytes=int(pr.resident_bytes), key_pass_s=float(pr.key_pass_s), plan_s=float(pr.plan_s),
             pass_s=[float(pr.pass_s[k]) for k in range(P)])
    return d


def bgzf_deflate(data, block=0xff00, codes=1, device=0):
    """gce_bgzf_deflate_codes: `data` (bytes-like) as BGZF members of `block` input bytes each (1..65 280), deflated on the GPU.  codes: 0 = fixed
    Huffman codes (level -2), 1 = per block the smallest of dynamic codes, fixed codes and stored (level -3), 2 = dynamic codes wherever they fit
    (tests).  Returns the members back to back as bytes; raises GceError."""
    lib = capi.load_library()
    buf = np.frombuffer(bytes(data), np.uint8)
    n = len(buf)
    cap = n + n // 8 + 64 * (n // max(int(block), 1) + 2)
    out = np.empty(max(cap, 1), np.uint8)
    got = C.c_size_t(0)
    rc = lib.gce_bgzf_deflate_codes(int(device), buf.ctypes.data if n else None, n, int(block), int(codes), out.ctypes.data, cap, C.byref(got))
    if rc != 0:
        raise GceError(rc, "gce_bgzf_deflate_codes")
    return out[:got.value].tobytes()


def device_bytes(reset_peak=False):
    """gce_device_bytes: (live, peak) device bytes of the engine allocations of this process."""
    lib = capi.load_library()
    live, peak = C.c_int64(), C.c_int64()
    lib.gce_device_bytes(C.byref(live), C.byref(peak), 1 if reset_peak else 0)
    return int(live.value), int(peak.value)


def write_batch_as_bam(path, batch, target_len, target_name=None, text="@HD\tVN:1.6\tSO:coordinate\n", threads=0, level=1):
    """gce_bam_from_batch: a ReadBatch as a BAM file (synthetic inputs for the end-to-end runs)."""
    lib = capi.load_library()
    st = batch.as_struct()
    tl = np.ascontiguousarray(target_len, np.uint32)
    names = None
    if target_name is not None:
        names = (C.c_char_p * len(tl))(*[n.encode() for n in target_name])
    rc = lib.gce_bam_from_batch(str(path).encode(), C.byref(st), len(tl), tl.ctypes.data, names, text.encode(), threads, level)
    if rc != 0:
        raise GceError(rc, "gce_bam_from_batch")


def sam_to_bam(sam_path, bam_path, threads=0, level=6):
    """gce_sam_to_bam: SAM text -> BAM on the host (what sam_read1 does with text under the reference, src/gencore.cpp:164,205)."""
    lib = capi.load_library()
    err = (C.c_char * 256)()
    rc = lib.gce_sam_to_bam(str(sam_path).encode(), str(bam_path).encode(), threads, level, err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))


def bam_to_sam(bam_path, sam_path, threads=0):
    """gce_bam_to_sam: BAM -> SAM text on the host (what sam_write1 prints for an output name that ends in "sam", src/gencore.cpp:170-173)."""
    lib = capi.load_library()
    err = (C.c_char * 256)()
    rc = lib.gce_bam_to_sam(str(bam_path).encode(), str(sam_path).encode(), threads, err)
    if rc != 0:
        raise GceError(rc, err.value.decode(errors="replace"))


def load_bed(path, target_names):
    """Bed::loadFromFile (src/bed.cpp:111-168): list of (tid, start, end, name) in file order; tid -1 = contig not in the header."""
    lib = capi.load_library()
    names = (C.c_char_p * max(len(target_names), 1))(*[n.encode() for n in target_names])
    n = C.c_int32()
    tid, st, en, nm = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_char_p)()
    rc = lib.gce_bed_load(str(path).encode(), len(target_names), names, C.byref(n), C.byref(tid), C.byref(st), C.byref(en), C.byref(nm))
    if rc != 0:
        raise GceError(rc, "gce_bed_load")
    out = [(tid[k], st[k], en[k], nm[k].decode()) for k in range(n.value)]
    lib.gce_bed_free(n, tid, st, en, nm)
    return out
