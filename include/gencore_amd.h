/*
 * gencore_amd.h — C-ABI of the MI355X consensus-read engine (libgencore_amd.so).
 *
 * This is the drop-in boundary for ONE path of OpenGene/gencore v0.17.2: everything between
 * Gencore::addToCluster(b) (call src/gencore.cpp:272, definition :469) and the output set that
 * Gencore::outputPair(p) (src/gencore.cpp:145) feeds, i.e. Cluster -> Group -> Pair -> consensus -> output order.
 * The reference has no FFI; the seam it offers is the C++ call pair
 *     Cluster::addRead(bam1_t*)                                   src/cluster.h:23,  src/cluster.cpp:260
 *     vector<Pair*> Cluster::clusterByUMI(thr, pre, post, cross)  src/cluster.h:26,  src/cluster.cpp:55
 * driven by Gencore::addToProperCluster (src/gencore.cpp:295-390) and Gencore::finishConsensus
 * (src/gencore.cpp:392-434).  Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain C, POD structs, pointers + sizes; no C++/torch types.
 *   - every function returns 0 (GCE_OK) or a negative gce_status; it NEVER calls exit().  The host adapter
 *     maps the codes back to the reference's messages + exit(-1)  (src/util.h:250 error_exit).
 *   - one engine per GPU per host thread; no global state inside the library.
 *   - the engine keeps the whole submitted stream resident in HBM (288 GB per MI355X) and processes it in
 *     one pass at gce_process(): the reference's 10,000-read flush cadence (src/gencore.cpp:319-322) is
 *     reproduced exactly as a per-cluster attribute, not as a host-side loop.
 */
#ifndef GENCORE_AMD_H
#define GENCORE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCE_ABI_VERSION 3              /* (struct layouts and the meaning of every v3 entry point are unchanged; gce_sam_to_bam / gce_bam_to_sam and SAM text in gce_run_bam, the report writers and gce_bam_read_header were ADDED under v3) */
#define GCE_NONE 0xFFFFFFFFu           /* "no record" marker in uint32 index arrays */
#define GCE_MAX_SUPPORTING_READS 100   /* src/stats.h:15 MAX_SUPPORTING_READS */

typedef struct gce_engine gce_engine;   /* opaque */

typedef enum gce_status {
    GCE_OK = 0,
    GCE_ERR_INVALID = -1,          /* bad argument / bad call order */
    GCE_ERR_NO_DEVICE = -2,        /* no HIP device: the product path has NO CPU fallback */
    GCE_ERR_HIP = -3,              /* HIP runtime failure, see gce_last_error() */
    GCE_ERR_OOM = -4,
    /* fatal conditions of the reference path, reported instead of exit(-1).  When a stream has several, the one on the
     * EARLIEST read is reported (the reference stops at the first in stream order). */
    GCE_ERR_UNSORTED = -10,        /* src/gencore.cpp:233-241 "the input is unsorted" */
    GCE_ERR_UMI_MISMATCH = -11,    /* src/pair.cpp:201-212 "The UMI of a read pair should be identical" */
    GCE_ERR_NM_MISSING = -12,      /* src/group.cpp:532-535: NM dereferenced although absent (segfault in the reference); never for a group that is not evaluated (gce_batch) */
    GCE_ERR_UMI_PARSE = -13,       /* src/bamutil.cpp:47-62: substr(start) with start > length throws in the reference */
    GCE_ERR_QNAME_SHORT = -14,     /* src/bamutil.cpp:343-346 "copyQName ERROR: desitination qname is shorter" */
    GCE_ERR_REF_WINDOW = -15       /* a clustered read lies outside the reference window staged for its contig (gce_set_reference_window) */
} gce_status;

/* One read's fixed-size fields.  Byte-for-byte the BAM alignment core block (SAMv1 section 4.2), i.e. what
 * htslib's bam1_core_t is decoded from; 32 bytes, the "packed key record" of the clustering scan. */
typedef struct gce_core {
    int32_t  tid;       /* bam1_core_t.tid   (refID)                                    */
    int32_t  pos;       /* bam1_core_t.pos   0-based leftmost                           */
    uint8_t  l_qname;   /* strlen(qname)+1 as stored in BAM; the engine applies htslib's in-memory
                           padding to a multiple of 4 (l_extranul) wherever the reference compares
                           name lengths (src/group.cpp:94,117; src/bamutil.cpp:341-346)            */
    uint8_t  mapq;
    uint16_t bin;
    uint16_t n_cigar;
    uint16_t flag;
    int32_t  l_qseq;
    int32_t  mtid;
    int32_t  mpos;
    int32_t  isize;
} gce_core;

/* Mirror of the Options fields the path reads (src/options.h:37-60, defaults src/options.cpp:4-40). */
typedef struct gce_params {
    int32_t abi_version;                    /* GCE_ABI_VERSION */
    int32_t device;                         /* HIP device ordinal */
    int32_t proper_umi_diff_threshold;      /* -d  properReadsUmiDiffThreshold      = 1   */
    int32_t unproper_umi_diff_threshold;    /*     unproperReadsUmiDiffThreshold    = 0   */
    int32_t duplex_mismatch_threshold;      /* -D  duplexMismatchThreshold          = 2   */
    int32_t cluster_size_req;               /* -s  clusterSizeReq                   = 1   */
    int32_t base_score_req;                 /* -c  baseScoreReq                     = 6   */
    int32_t high_quality;                   /* --high_qual                          = 30  */
    int32_t moderate_quality;               /* --moderate_qual                      = 20  */
    int32_t low_quality;                    /* --low_qual                           = 15  */
    int32_t score_high;                     /* scoreOfNotOverlappedHighQual         = 8   */
    int32_t score_moderate;                 /* scoreOfNotOverlappedModerateQual     = 6   */
    int32_t score_low;                      /* scoreOfNotOverlappedLowQual          = 4   */
    int32_t score_bad;                      /* scoreOfNotOverlappedBadQual          = 2   */
    int32_t skip_low_complexity_cluster_threshold;  /*                              = 1000 */
    int32_t duplex_only;                    /* -x */
    int32_t disable_duplex;                 /* --no_duplex */
    int32_t flush_period;                   /* the literal 10000 of src/gencore.cpp:321 */
    double  score_percent_req;              /* -a  scorePercentReq                  = 0.8 */
    char    umi_prefix[32];                 /* -u, already resolved ("auto" -> gce_detect_umi_prefix) */
    /* contig lengths of the BAM header: needed by the cross-contig key, src/gencore.cpp:311 */
    int32_t n_targets;
    const uint32_t *target_len;             /* [n_targets], copied by gce_create */
    /* Stream context for contig-granular shards (multi-GPU): this engine sees a contiguous slice of the globally
     * sorted stream.  tick_offset = number of clustered reads before the slice (the reference's static `tick`,
     * src/gencore.cpp:319); trailing_flush != 0 if a flush event occurs after the slice, so clusters still pending
     * at the end of the slice get -d instead of the end-of-file threshold (quirk Q1).  Shards cut INSIDE a contig by
     * cluster key use gce_batch.tick + gce_set_flush_events instead. */
    int64_t tick_offset;
    int32_t trailing_flush;
    /* --quit_after_contig (Options::maxContig, src/options.cpp:10, src/gencore.cpp:243-246): > 0: the read loop ends at the first read whose
     * tid >= max_contig -- that read is still counted by the pre-Stats (addRead comes first, :222) and sorted-checked (:233-241), then it and
     * everything behind it are ignored; what is pending is finished as at the end of the file.  0: off.  (The field was `reserved`, always 0,
     * up to ABI 3: additive.) */
    int32_t max_contig;
} gce_params;

/* A batch of reads in INPUT ORDER (coordinate-sorted), struct-of-arrays.  Offsets are start offsets, lengths
 * come from gce_core (l_qname, n_cigar, l_qseq).  seq is BAM 4-bit packed (high nibble = even base,
 * src/bamutil.cpp:133-147,167-189), qual is raw Phred.  seq/qual are MUTATED IN PLACE where the reference
 * mutates its bam1_t records (src/group.cpp:503-525,555-556, src/cluster.cpp:227-232; the quality rewrite of
 * src/pair.cpp:158-159 persists only in emitted records, see gce_result).  A group that no setting of the run can write -- one pair
 * under --supporting_reads > 1 or --duplex_only in a cluster that forms no duplex (gce_get_skipped_groups) -- is not evaluated: its
 * reads keep their input bytes, and it raises none of the consensus errors (GCE_ERR_NM_MISSING, GCE_ERR_QNAME_SHORT).
 * Device buffers (gce_submit_device): `core` must be 16-byte aligned and every blob readable 16 bytes past its end
 * (vector loads of the last read); gce_submit pads its own copies.  Reads longer than 65535 bases are rejected. */
typedef struct gce_batch {
    int64_t         n_reads;
    const gce_core *core;        /* [n] */
    const uint64_t *qname_off;   /* [n] byte offset into qname; names are NUL-terminated */
    const char     *qname;
    const uint64_t *cigar_off;   /* [n] offset in 32-bit words into cigar */
    const uint32_t *cigar;       /* BAM encoding len<<4|op */
    const uint64_t *seq_off;     /* [n] byte offset into seq */
    uint8_t        *seq;
    const uint64_t *qual_off;    /* [n] byte offset into qual */
    uint8_t        *qual;
    const int32_t  *nm;          /* [n] value of the NM aux tag (bam_aux2i), ignored when nm_type==0 */
    const uint8_t  *nm_type;     /* [n] BAM aux type byte of NM ('C','c','S','s','I','i'), 0 = tag absent */
    const uint64_t *mi_off;      /* optional: [n] offset of the MI:Z string, UINT64_MAX = read has no MI tag */
    const char     *mi;          /* optional: NUL-terminated MI:Z strings (src/bamutil.cpp:23-38); NULL if unused */
    size_t qname_bytes, cigar_words, seq_bytes, qual_bytes, mi_bytes;   /* total sizes of the blobs */
    /* optional (key-range shards, see gce_set_flush_events): [n] the value the reference's `tick` has right after this
     * read was added (src/gencore.cpp:319-320), counted over the WHOLE stream; ignored for reads that never reach the
     * cluster map.  NULL: the engine counts ticks itself from gce_params.tick_offset. */
    const uint64_t *tick;
} gce_batch;

/* Additive QC counters touched on the path (src/stats.h:47-65; call sites src/gencore.cpp:110,146,222 and
 * src/cluster.cpp:102,136,142,158,162,173,177,185).  All int64, all additive => one RCCL all-reduce(sum). */
typedef struct gce_stats {
    int64_t reads;                     /* mRead                */
    int64_t bases;                     /* mBase                */
    int64_t reads_unmapped;            /* mReadUnmapped        */
    int64_t bases_unmapped;            /* mBaseUnmapped        */
    int64_t base_mismatches;           /* mBaseMismatches      */
    int64_t reads_with_mismatches;     /* mReadWithMismatches  */
    int64_t clusters;                  /* mCluster             */
    int64_t multi_molecule_clusters;   /* mMultiMoleculeCluster*/
    int64_t molecules;                 /* mMolecule            */
    int64_t molecules_se;              /* mMoleculeSE          */
    int64_t molecules_pe;              /* mMoleculePE          */
    int64_t sscs;                      /* mSSCSNum             */
    int64_t dcs;                       /* mDCSNum              */
    int64_t uncounted_supporting_reads;/* uncountedSupportingReads */
    int64_t supporting_hist[GCE_MAX_SUPPORTING_READS];  /* mSupportingHistgram */
} gce_stats;
#define GCE_STATS_WORDS (14 + GCE_MAX_SUPPORTING_READS)

/* The output of the path: one row per EMITTED record, struct-of-arrays, in the order of the reference's output set
 * (bamComp, src/gencore.h:19-47): ascending (tid, pos, mtid, mpos, isize); where the reference breaks ties by heap
 * address (quirk Q3) the engine uses the input index, so the order is deterministic.
 * Row k means: "input read src[k], with seq/qual replaced by the bytes at seq_off[k]/qual_off[k] of the compact blobs
 * below, its qname replaced by the qname of input read qname_src[k] (BamUtil::copyQName, src/bamutil.cpp:338), NM
 * patched to nm_new[k] if >= 0 (src/group.cpp:570), FR/RR aux bytes appended if >= 0 (src/pair.cpp:57-67)".
 * Host pointers (gce_drain) or device pointers (gce_result_device), owned by the engine until the next
 * gce_process / gce_reset / gce_destroy. */
typedef struct gce_result {
    int64_t         n_reads;     /* reads of the processed stream */
    int64_t         n_out;       /* emitted records */
    const uint32_t *src;         /* [n_out] input read index of the record (the consensus template, or a pass-through read) */
    const uint8_t  *kind;        /* [n_out] 1 = emitted by outputPair (src/gencore.cpp:145);
                                            2 = mate-unmapped pass-through (src/gencore.cpp:307-309) */
    const uint32_t *qname_src;   /* [n_out] == src[k] if the name is unchanged */
    const int32_t  *nm_new;      /* [n_out] -1 = NM untouched, else the byte written at src/group.cpp:570 */
    const int16_t  *fr;          /* [n_out] -1 = no tag, else the FR:C byte (src/pair.cpp:57-61, low byte, quirk Q8) */
    const int16_t  *rr;          /* [n_out] -1 = no tag, else the RR:C byte (src/pair.cpp:62-67) */
    const uint32_t *mate;        /* [n_out] ROW of the other record of the same output Pair, or GCE_NONE */
    const uint64_t *seq_off;     /* [n_out] byte offset of the record's packed bases in `seq` (16-byte aligned) */
    const uint64_t *qual_off;    /* [n_out] byte offset of its qualities in `qual` (16-byte aligned) */
    const uint8_t  *seq;         /* compact blobs: emitted records only */
    const uint8_t  *qual;
    size_t          seq_bytes, qual_bytes;
    gce_stats       pre;         /* mPreStats  deltas */
    gce_stats       post;        /* mPostStats deltas: reads/bases/mismatches are Stats::addRead (src/stats.cpp:101-121)
                                    over ALL emitted records (what writeBam accumulates once every record is written,
                                    src/gencore.cpp:110) — see INTEGRATION.md for the report-before-drain quirk */
} gce_result;

/* Kernel timing of the last gce_process(), HIP events on the engine's stream. */
typedef struct gce_timing {
    double total_ms;             /* first kernel start -> last kernel end */
    double describe_ms;          /* per-read descriptors, UMI slices, pre-Stats (consumed by pairing and the vote; not cluster formation) */
    double cluster_ms;           /* clustering scan (class, key, block-level leaders), the roofline kernel  */
    double csr_ms;               /* rest of cluster formation: tick scan, flush events, leader table, cluster list + member lists */
    double pairing_ms;           /* mate pairing + UMI grouping per cluster */
    double score_ms;             /* Pair::computeScore launches of the fallback path (0 when every group takes the fused vote) */
    double consensus_ms;         /* template pick + column vote (fused kernel + fallbacks) */
    double finish_ms;            /* duplex merge, filter, tags, stats */
    double output_ms;            /* output order + compaction of the emitted records */
    int64_t n_clusters, n_groups, n_pairs;
    int64_t n_leaders;           /* (cluster, scan block) runs the clustering scan handed to the bucket table (0 when ticks come with the batch) */
} gce_timing;

/* Fill *p with the reference defaults (src/options.cpp:4-40). */
void gce_params_default(gce_params *p);

/* "auto" UMI prefix detection on the first read's qname, src/gencore.cpp:207-220.  Writes "", "umi" or "UMI". */
void gce_detect_umi_prefix(const char *first_qname, char out_prefix[32]);

/* Replaces: Gencore::Gencore(Options*) + Cluster(Options*) construction, src/gencore.cpp:7-19. */
int gce_create(const gce_params *params, gce_engine **out);
void gce_destroy(gce_engine *e);

/* Replaces: Reference::instance(opt)->getData(tid, ...) (src/reference.cpp:33-70) as the source of the staged
 * reference.  `nibbles` is one contig in FastaReader's own 4-bit code (A=1,T=2,C=3,G=4, other=0, LOW nibble =
 * even position; src/fastareader.cpp:106-128,139-152), n_bases its length.  Contigs never set behave like
 * "contig not found in the reference" (getData returns NULL).  Host or device pointer. */
int gce_set_reference(gce_engine *e, int32_t tid, const uint8_t *nibbles, int64_t n_bases);
/* Same from upper-cased ASCII bases (one contig of FastaReader::mAllContigs, src/fastareader.h): packed on the GPU
 * (FastaReader::to4bits, src/fastareader.cpp:139-152). */
int gce_set_reference_ascii(gce_engine *e, int32_t tid, const char *bases, int64_t n_bases);
/* Per-shard staging: only the bases [win_start, win_start + n_bases) of a contig of `contig_len` bases, e.g. what the
 * reads of one key-range shard can touch -- an engine for 1/8 of hg19 then holds 1/8 of the reference.  win_start must be even.
 * Reference::getData's end-of-contig rule (src/reference.cpp:40,60) keeps using contig_len.  gce_process fails with
 * GCE_ERR_REF_WINDOW if a clustered read whose isize != 0 does not lie inside the window of its contig. */
int gce_set_reference_window(gce_engine *e, int32_t tid, int64_t contig_len, int64_t win_start, const char *bases, int64_t n_bases);
/* Convenience: pack an upper-cased ASCII contig into that code on the host (src/fastareader.cpp:139). */
void gce_pack_reference(const char *bases, int64_t n_bases, uint8_t *nibbles_out);

/* Key-range shards (multi-GPU cuts inside a contig): the flush events of the WHOLE stream before its first
 * unmapped read — event j is the read on which `tick` reaches (j+1)*flush_period (src/gencore.cpp:319-322) and carries
 * that read's (tid, pos), which bound the flush walk (src/gencore.cpp:333-354).  Used together with gce_batch.tick;
 * host arrays, copied.  n_events = 0 with tick given means "no flush ever fires".  Unmapped reads must follow every
 * mapped read of the stream in this mode. */
int gce_set_flush_events(gce_engine *e, int32_t n_events, const int32_t *ev_tid, const int32_t *ev_pos);
/*   The events stay set across gce_reset and the implicit reset of the next submit (set once for many steps of the same stream); a call
 *   replaces them, and a stream without gce_batch.tick ignores them. */

/* Replaces: the per-read loop body Gencore::addToCluster(b) (src/gencore.cpp:272,469-476) for a whole batch.
 * Host buffers are copied to HBM; the caller keeps ownership.  May be called repeatedly; batches are
 * concatenated in call order (they must continue the same sorted stream). */
int gce_submit(gce_engine *e, const gce_batch *batch);
/* Same, but every pointer in *batch is a DEVICE pointer that stays valid until the next gce_submit_device / gce_reset /
 * gce_destroy; seq/qual are mutated in place in the caller's HBM buffers (zero-copy path used by bench.py and by a
 * GPU BAM decoder).  ONE batch per gce_process is zero copy.  Further calls before gce_process append to the stream (round 5): the engine then keeps its
 * own copy -- the first batch and every further one are copied device to device when the second call is made; a batch may be freed as soon as the call that
 * appended it returns, and the in-place mutations hit the engine's copy (results come back through the compact blobs of gce_result either way). */
int gce_submit_device(gce_engine *e, const gce_batch *batch);

/* Replaces: every clusterByUMI call of the stream (src/gencore.cpp:355 periodic, :409 end of file), the
 * outputPair bookkeeping (src/gencore.cpp:145-160) and the ordering of the output set (src/gencore.h:19-47).
 * Runs the whole HIP pipeline over everything submitted since the last process.  A second call without a new
 * submit is an error (the stream was mutated in place). */
int gce_process(gce_engine *e);

/* Replaces: draining csPairs into Gencore::outputPair (src/gencore.cpp:356-360,410-414).  Copies the result
 * table (emitted records only) to host memory owned by the engine. */
int gce_drain(gce_engine *e, gce_result *out);
/* Device-side view of the same table (device pointers). */
int gce_result_device(gce_engine *e, gce_result *out);

/* Streamed submission for a stream whose totals are known up front (a BAM file indexed by gce_bam_open): gce_reserve sizes the
 * HBM copy once, then every gce_submit / gce_submit_async copies its batch straight into place on a separate HIP stream -- the
 * copy of batch k overlaps the caller's preparation of batch k+1 (src/gencore.cpp:205-274 interleaves sam_read1 and
 * addToCluster the same way).  With gce_submit_async the caller's buffers must stay untouched until gce_submit_wait(ticket)
 * or gce_process returns.  MI tags (gce_batch.mi / mi_off) and per-read ticks (gce_batch.tick; every batch of a stream or none) travel on this path too
 * (round 5); a batch that exceeds the reservation makes the buffers grow instead of failing. */
/* The reservation outlives gce_reset and every later stream of the engine: each new stream is copied into the reserved buffers (grown
 * when it is larger), through the same gce_submit / gce_submit_async path. */
int gce_reserve(gce_engine *e, int64_t n_reads, size_t qname_bytes, size_t cigar_words, size_t seq_bytes, size_t qual_bytes);
int gce_submit_async(gce_engine *e, const gce_batch *batch, int32_t *ticket);
int gce_submit_wait(gce_engine *e, int32_t ticket);

/* Replaces: Stats::statDepth + Bed::statDepth over the stream (src/stats.cpp:57-84, src/bed.cpp:66-81), i.e. the per-base part of
 * mPreStats->addRead (src/gencore.cpp:222, mapped reads only: src/stats.cpp:118-120) and of mPostStats->addRead in writeBam
 * (src/gencore.cpp:110), computed on the GPU from the batch that is resident after gce_process.  coverage_step = Options::coverageStep
 * (src/options.cpp:36).  Regions: the BED file's (tid, start, end) in FILE order (gce_bed_load); a region whose tid is outside the header
 * is ignored, as Bed::loadFromFile drops it (src/bed.cpp:151-166).  Results (host arrays owned by the engine until the next call):
 * depth bins per contig, 1 + target_len / step each (src/stats.cpp:41-47), and base counts per region (BedRegion::mCount). */
typedef struct gce_depth {
    int32_t        n_targets;
    const int64_t *bin_off;       /* [n_targets + 1] first bin of every contig */
    const int64_t *pre_depth;     /* [bin_off[n_targets]]  mPreStats->mGenomeDepth */
    const int64_t *post_depth;    /*                       mPostStats->mGenomeDepth */
    int32_t        n_regions;
    const int64_t *pre_bed;       /* [n_regions] in the order the regions were given */
    const int64_t *post_bed;
} gce_depth;
int gce_depth_stats(gce_engine *e, int32_t coverage_step, int32_t n_regions, const int32_t *region_tid, const int32_t *region_start,
                    const int32_t *region_end, gce_depth *out);

/* Everything the final Stats merge of a multi-GPU run adds up, as ONE int64 buffer in DEVICE memory (counters + histogram + per-contig depth
 * bins + BED region counts; the buffers the reference makes at src/gencore.cpp:181-184 and fills at src/stats.cpp:39-46,56-83, src/bed.cpp:64-79):
 *     [pre Stats: GCE_STATS_WORDS][post Stats: GCE_STATS_WORDS][pre depth: n_bins][post depth: n_bins][pre BED counts: n_regions][post BED counts: n_regions]
 * Every word is additive over key-range shards of one stream: N ranks merge it with one all-reduce(sum) over RCCL (bench.py), N engines of one process with one
 * add per engine (gce_run_bam_depth).  Depth bins as in gce_depth (1 + target_len / coverage_step per contig, contigs back to back; bin_off: host array of
 * n_targets + 1 entries owned by the engine); BED counts in the order the regions were given (a region whose contig is not in the header counts 0).
 * Valid until the next gce_process / gce_depth_stats / gce_stats_payload_device of this engine.  (Addition under ABI v3, round 5.)
 * The payload is COMPLETE when the call returns (the engine's stream is waited for): it may be read from any stream, e.g. by an RCCL all-reduce. */
typedef struct gce_payload_layout {
    int32_t stats_words;          /* 2 * GCE_STATS_WORDS */
    int32_t n_targets;
    int64_t n_bins;               /* depth bins of one block (pre or post) */
    int32_t n_regions;
    int64_t total_words;          /* stats_words + 2 * n_bins + 2 * n_regions */
    const int64_t *bin_off;       /* [n_targets + 1] */
} gce_payload_layout;
int gce_stats_payload_device(gce_engine *e, int32_t coverage_step, int32_t n_regions, const int32_t *region_tid, const int32_t *region_start,
                             const int32_t *region_end, const int64_t **payload, gce_payload_layout *layout);

int gce_get_timing(gce_engine *e, gce_timing *out);
/* k_vote's counters of the last gce_process (ADDED under v3): out[0] vote rounds behind a batch's first (a batch whose contested columns do not
 * fit one round's tallies), out[1] of those the rounds that start at a side index that is not a multiple of 4, out[2] group sides k_vote handed on
 * to the per-side kernels, out[3] groups of the stream.  For tests and diagnostics. */
int gce_get_vote_counters(gce_engine *e, int64_t out[4]);
/* Group sides finished per consensus kernel in the last gce_process (ADDED under v3; for tests and diagnostics): out[0] k_vote (both sides of
 * every group it did not hand on), out[1] k_consensus_fast, out[2] k_deep_prepare (deep sides without a template), out[3] k_vote_deep,
 * out[4] k_consensus_slow.  out[0] counts only sides k_vote really finished: after a gce_process without a device error the five add up to
 * 2 x (groups - skipped groups). */
int gce_get_consensus_counters(gce_engine *e, int64_t out[5]);
/* Groups of the last gce_process that were not evaluated because their result could not be written (ADDED under v3; for tests and diagnostics):
 * one-pair groups under --supporting_reads > 1 or --duplex_only, with --skip_low_complexity_cluster_threshold >= 1, whose cluster forms no
 * duplex (no UMI, --no_duplex, or a single group).  Their Stats entries are those of the reference; no consensus kernel sees them.
 * out[0]: their number, 0 with -s 1 and no --duplex_only.  out[1]: the batches k_vote formed over the other groups (a batch holds at most 16). */
int gce_get_skipped_groups(gce_engine *e, int64_t out[2]);
/* The GPU record index's counters (ADDED under v3; for tests and diagnostics): out[0] 16 KB segments, out[1] of those flagged by the first
 * check (a guessed record start off the chain), out[2] parallel repair rounds, out[3] serial repairs (0 or 1 per index).  e: its last
 * gce_raw_finish; e == NULL: summed over every window of the last pass runner of the process (gce_run_bam_passes, key pass and passes). */
int gce_get_index_counters(gce_engine *e, int64_t out[4]);
/* Which mate-pairing tier paired every cluster of the last gce_process (ADDED under v3; for tests and diagnostics).  n_clusters: the cluster
 * count; counts[k]: clusters of tier k; for the first min(cap, n_clusters) clusters, tier[c] and read[c] = one read of the cluster (the left read
 * of its first pair slot; 0xFFFFFFFF for GCE_PAIR_TIER_NEVER), as a stream index.  Any output pointer may be NULL. */
enum { GCE_PAIR_TIER_NEVER = 0,          /* the cluster is never processed (pending behind an early finishConsensus) */
       GCE_PAIR_TIER_SUB16 = 1,          /* k_pairing_sub<16>: <= 16 reads, 16 lanes per cluster */
       GCE_PAIR_TIER_SUB32 = 2,          /* k_pairing_sub<32>: 17..32 reads */
       GCE_PAIR_TIER_FAST = 3,           /* k_pairing_fast: 33..64 reads, one wave */
       GCE_PAIR_TIER_DEEP_LDS = 4,       /* k_pairing_deep, arrays in LDS: 65..4096 reads */
       GCE_PAIR_TIER_DEEP_DEVICE = 5,    /* k_pairing_deep, arrays in device memory: 4097..65534 reads */
       GCE_PAIR_TIER_GENERIC = 6,        /* the generic kernels: whatever the others hand on */
       GCE_PAIR_TIERS = 7 };
int gce_get_pairing_tiers(gce_engine *e, int64_t cap, uint8_t *tier, uint32_t *read, int64_t *n_clusters, int64_t counts[GCE_PAIR_TIERS]);
/* The two Stats blocks of the last gce_process in DEVICE memory: 2 x GCE_STATS_WORDS int64, pre then post -- for the final Stats merge
 * of a multi-GPU run (one RCCL all-reduce(sum); all fields are additive, src/stats.h:47-65) without a bounce through the host. */
int gce_stats_device(gce_engine *e, const int64_t **pre_then_post);

/* ------------------------------------------------------------------------------------------------------------------------
 * Multi-GPU planning, on a GPU from the 32-byte key records of the WHOLE sorted stream (host or device pointers).
 * Clusters shard by cluster key (tid, left), not by read position: a right mate follows its mate (src/gencore.cpp:301-303).
 * ------------------------------------------------------------------------------------------------------------------------ */
/* tick_out[i] = the reference's `tick` right after read i was added (src/gencore.cpp:319-320; unchanged by reads that never reach the
 * cluster map) -> gce_batch.tick of a shard; the flush events (src/gencore.cpp:321-322) as malloc'ed host arrays (gce_free) ->
 * gce_set_flush_events.  GCE_ERR_INVALID if a clustered read follows the first unmapped read (not shardable by key). */
int gce_stream_context(int32_t device, const gce_core *core, int64_t n_reads, int32_t flush_period, uint64_t *tick_out,
                       int32_t *n_events, int32_t **ev_tid, int32_t **ev_pos);
/* shard_out[i] in [0, world): mode 0 = contiguous key ranges of equal read count (configs[3]: the cuts fall inside contigs),
 * mode 1 = whole clusters dealt longest-processing-time first with weight reads^2 (configs[4]: ultra-deep hotspots);
 * mode 2 = contiguous key ranges balanced by the pass runner's weight, GCE_PASS_WEIGHT_A x the record's fixed fields + GCE_PASS_WEIGHT_B
 * (addition under ABI v3; gce_run_bam_passes plans the same way with the records' full sizes).  world <= 64. */
int gce_plan_shards(int32_t device, const gce_core *core, int64_t n_reads, int32_t world, int32_t mode, int32_t *shard_out);
void gce_free(void *p);
/* Drop all submitted reads/results but keep params, reference and allocations (for repeated bench steps).
 * Survives a reset: the params (gce_create), every staged contig and window, the flush events of gce_set_flush_events (used only by a stream
 * whose batches carry gce_batch.tick; bench's N > 1 path and the pass runner set them once and rely on this), a gce_reserve reservation, the
 * device buffers (they grow, never shrink), the bucket table (all-zero again after every step that ran the clustering) and the once-per-engine
 * "k_vote off" note.  Dropped: the submitted batches, the result table, ticks / MI tags / the raw stream and any gce_raw_select_shard choice.
 * The first gce_reserve / gce_submit / gce_submit_device / gce_submit_async / gce_raw_begin after a gce_process (successful or failed) resets implicitly,
 * so a new stream needs no call.  gce_reset IS needed after a refused submit that left the batches accepted before it in the engine -- a
 * gce_submit after gce_submit_device, a batch with gce_batch.tick behind one without (or the reverse) -- or to drop a stream never processed. */
int gce_reset(gce_engine *e);

const char *gce_last_error(const gce_engine *e);   /* human-readable detail of the last failure */
const char *gce_status_message(int status);        /* the reference's message for a status code */
int gce_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------------------
 * Files: the callers and data formats on either side of the path.  Host code over zlib
 * (gencore_amd/csrc/bamio.cpp); htslib is not used.
 * ------------------------------------------------------------------------------------------------------------------------ */
typedef struct gce_bam gce_bam;       /* a BAM file held in memory: inflated stream + record index */
typedef struct gce_fasta gce_fasta;

typedef struct gce_bam_info {
    int32_t             n_targets;    /* bam_hdr_t.n_targets / target_len / target_name (src/gencore.cpp:171,311) */
    const uint32_t     *target_len;
    const char *const  *target_name;
    const char         *text;         /* SAM header text, l_text bytes */
    int64_t             l_text;
    int64_t             n_records;
    uint64_t            qname_bytes, cigar_words, seq_bytes, qual_bytes, mi_bytes;   /* blob totals over all records (gce_reserve) */
    double              read_s, inflate_s, index_s;                                  /* wall time of gce_bam_open's stages */
} gce_bam_info;

/* Replaces: sam_open + sam_hdr_read + the sam_read1 loop (src/gencore.cpp:164-205): reads the file, inflates its BGZF blocks on
 * `threads` host threads (0 = all), parses the header and indexes the records. */
int gce_bam_open(const char *path, int threads, gce_bam **out);
void gce_bam_close(gce_bam *f);
const char *gce_bam_error(const gce_bam *f);
int gce_bam_get_info(const gce_bam *f, gce_bam_info *out);
/* Records [first, first+count) as a gce_batch (host pointers into one of two internal buffer sets, slot = 0 / 1, valid until that
 * slot is filled again): the 32-byte core block verbatim, name / CIGAR / bases / qualities blobs, NM (type + value, bam_aux2i)
 * and MI:Z (src/bamutil.cpp:23-38) from the aux area. */
int gce_bam_chunk(gce_bam *f, int64_t first, int64_t count, int slot, gce_batch *out);
/* Replaces: sam_hdr_write + Gencore::writeBam / sam_write1 for every output record (src/gencore.cpp:85-111,187-190): row k of
 * `res` (HOST pointers: gce_drain) becomes input record src[k] with the row's bases / qualities, the name of record qname_src[k]
 * (BamUtil::copyQName, src/bamutil.cpp:338-364), the NM byte (src/group.cpp:570) and FR / RR appended as aux type 'C'
 * (src/pair.cpp:57-67); BGZF blocks of 0xff00 bytes deflated at `level` on `threads` threads, EOF marker block at the end.
 * level 0..9 = zlib's levels (htslib writes at 6); level -1 = the library's own greedy fixed-Huffman encoder: about 3.5 x the speed of
 * level 1, output about a third larger. */
int gce_bam_write(const char *path, const gce_bam *in, const gce_result *res, int threads, int level);

/* The inverse of gce_bam_chunk: a gce_batch (host pointers) as a BAM file, one record per read with its NM and MI tags.  Not a
 * reference call site: it materialises synthetic streams as files for the end-to-end measurement (tools/bam_bench.py) and tests. */
int gce_bam_from_batch(const char *path, const gce_batch *batch, int32_t n_targets, const uint32_t *target_len,
                       const char *const *target_name, const char *text, int threads, int level);

/* Replaces: the SAM TEXT side of htslib under the reference -- sam_open(in, "r") takes BAM or SAM, sam_read1 parses text lines; an output
 * name that ends in "sam" is opened with sam_open(out, "w") and sam_write1 prints text (src/gencore.cpp:164-173,180,187,205,104).
 * gce_run_bam does the same: an input that does not start with the gzip magic is read as SAM text (header lines, then one alignment per
 * line, converted to BAM records on the host threads and pushed to the GPU like an inflated BAM window), an output name that ends in
 * "sam" is written as text -- at level -2 / -3 by the GPU (gce_raw_format_output below: the lines are made in HBM from the output record
 * stream, the host copies and writes them), at every other level by samtext::bam_to_line on the host's threads; the file's bytes are the
 * same either way.  The two functions below are the conversion alone, on the host (no engine, no GPU).  Conventions of htslib
 * that the path can see are kept: an integer tag is stored in the smallest type that holds it ('C' for NM 0..255: src/group.cpp:569
 * patches NM only as 'C'), bin = reg2bin(pos, pos + reference length), QUAL '*' = 0xFF bytes, an unknown RNAME = -1. */
int gce_sam_to_bam(const char *sam_path, const char *bam_path, int threads, int level, char err[256]);
int gce_bam_to_sam(const char *bam_path, const char *sam_path, int threads, char err[256]);

/* Replaces: Reference::Reference -> FastaReader(file) + readAll (src/reference.cpp:13-24, src/fastareader.cpp:7-41,57-104,157-168),
 * including its quirks (first character of every line unfiltered, lower case folded, ID = header up to the first blank, a later
 * contig of the same name wins).  Contigs come back as ASCII for gce_set_reference_ascii. */
int gce_fasta_load(const char *path, int threads, gce_fasta **out);   /* threads <= 0: all host cores; 1: the literal one-pass walk */
int gce_fasta_get(const gce_fasta *fa, int32_t *n_contigs, const char *const **ids, const char *const **bases, const int64_t **lengths);
void gce_fasta_free(gce_fasta *fa);

/* Replaces: Bed::loadFromFile (src/bed.cpp:111-168): tab-separated chr / start / end / [name], '#' comment lines skipped, contig names
 * resolved against the BAM header (regions of unknown contigs get tid -1), reading stops at the first line of >= 4095 characters
 * (ifstream::getline into a 4096-byte buffer).  Arrays are malloc'ed; free them with gce_bed_free. */
int gce_bed_load(const char *path, int32_t n_targets, const char *const *target_name, int32_t *n_regions, int32_t **tid, int32_t **start,
                 int32_t **end, char ***name);
void gce_bed_free(int32_t n_regions, int32_t *tid, int32_t *start, int32_t *end, char **name);

/* The variant mask of the error profile, read on the host (addition under ABI v3; gencore_amd/csrc/bamio_varmask.hpp, DESIGN.md 4m rule K).
 * Replaces: nothing in the reference's source -- it is the `--variants` of `fgbio ErrorRateByReadPosition` and the DB_SNP of Picard's
 * metrics.  path ends in `.vcf` or `.vcf.gz` (plain gzip or BGZF, any number of members; inflated and parsed as a stream, so no line is too
 * long) or in `.bed` (read with gce_bed_load, unchanged); any other name is refused.  VCF: lines end in LF or CR LF, the last may lack it;
 * empty lines and lines that begin with `#` are no records; every other line needs five tab-separated fields CHROM POS ID REF ALT with POS a
 * decimal integer >= 1 and REF not empty, else GCE_ERR_INVALID with "variant mask line N: ..." (N from 1 over all lines).  A record (n_records)
 * gives the 0-based interval [POS - 1, POS - 1 + strlen(REF)) of the contig names[t] == CHROM: the SNP base, an insertion's anchor base, a
 * deletion's anchor and its deleted bases.  Not used: a record of an unknown CHROM (n_unknown_contig), else one whose ALT is `.`, `<NON_REF>`
 * or `<*>` alone (n_no_alt: the reference blocks of a gVCF).  FILTER, INFO (END= too) and the genotypes are not read: a symbolic SV allele
 * masks its one REF base.  BED: every region is a record, one of an unknown contig n_unknown_contig.  The intervals are clamped to
 * [0, lens[t]) -- the caller gives min(header length, FASTA length), <= 0 for a contig without reference bases, whose intervals are dropped
 * --, sorted by (tid, start) and merged where they overlap or abut (n_intervals of them, n_masked_bases positions; no cap on either).
 * threads is accepted for symmetry with gce_fasta_load; inflate and parse are one pass on one thread.  No device is touched.  The arrays are
 * malloc'ed: gce_mask_free.  A failed call leaves *out zeroed. */
typedef struct gce_mask {
    int64_t n_lines, n_records, n_unknown_contig, n_no_alt, n_intervals, n_masked_bases;   /* n_lines: 0 for a BED */
    int32_t *tid, *start, *end;     /* n_intervals each */
} gce_mask;
int gce_mask_load(const char *path, int32_t n_ref, const char *const *names, const int64_t *lens, int threads, gce_mask *out, char err[256]);
void gce_mask_free(gce_mask *m);

typedef struct gce_bam_run {
    int64_t n_reads, n_out;
    double  open_s;          /* gce_bam_open: read + inflate + index */
    double  read_s, inflate_s, index_s;
    double  submit_s;        /* struct-of-arrays fill of every chunk + gce_submit_async (copies overlap the next fill) */
    double  process_s;       /* gce_process wall time (waits for the last copy) */
    double  kernel_ms;       /* gce_timing.total_ms */
    double  drain_s, write_s, total_s;
    gce_stats pre, post;
    int64_t peak_rss_kb;     /* VmHWM of the process when the run ended (the streaming path holds windows, not the file) */
    int64_t rss_start_kb, rss_end_kb;   /* VmRSS when gce_run_bam was entered / left: the path's own footprint is the difference to the peak */
} gce_bam_run;
/* Replaces: Gencore::consensus() end to end for a coordinate-sorted BAM (src/gencore.cpp:162-293) as a pipeline with a bounded host
 * footprint: the file is read and inflated window by window (pinned buffers, copied to HBM while the next window is inflated), records
 * are indexed, parsed and -- after gce_process -- re-assembled as BAM records on the GPU (gce_raw_*), the output stream is deflated by all
 * host threads piece by piece.  chunk_reads < 65536 shrinks the windows to 1 MB of compressed bytes (tests).
 * params->n_targets / target_len are taken from the BAM header; params->umi_prefix "auto" is resolved on the first read
 * (src/gencore.cpp:207-220).  fasta_path may be NULL. */
int gce_run_bam(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int threads,
                int64_t chunk_reads, int level, gce_bam_run *out, char err[256]);
/* The whole-file host-codec path of ABI v2 (gce_bam_open: everything inflated and indexed on the host, struct-of-arrays chunks, gce_bam_write);
 * also what GCE_BAM_HOSTCODEC=1 makes gce_run_bam do. */
int gce_run_bam_hostcodec(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int threads,
                          int64_t chunk_reads, int level, gce_bam_run *out, char err[256]);

/* The GPU side of the BAM codec (gencore_amd/csrc/gce_bamdev.hpp), the pieces gce_run_bam is made of.  Replaces sam_read1's record
 * parsing and sam_write1's record assembly (src/gencore.cpp:205-274,83-111 via htslib) for a whole file at once; the host only inflates
 * and deflates BGZF blocks.
 *   gce_raw_begin / gce_raw_push: the INFLATED BAM stream (header included), in order, window by window; asynchronous (gce_submit_wait on
 *     the ticket before the host buffer is reused; pinned buffers -- gce_host_alloc -- make the copies true DMA).
 *   gce_raw_finish: records indexed and parsed in HBM (records_begin = end of the BAM header, n_ref = its contig count); the engine is then
 *     in the state gce_submit_device leaves it in.  Names, bases and qualities are NOT copied: the batch's blobs are the raw stream.
 *   gce_raw_build_output (after gce_process): the emitted records as a stream of BAM records in HBM, table order; gce_raw_read_output_async
 *     copies a piece of it to the host (ticket -> gce_submit_wait). */
int gce_raw_begin(gce_engine *e, size_t capacity_hint);
int gce_raw_push(gce_engine *e, const void *host, size_t bytes, int32_t *ticket);
/* BGZF members as they lie in the file: copied to HBM COMPRESSED and inflated by the GPU (one lane per member, CRC-32 and ISIZE checked) when
 * gce_raw_finish is called -- replaces bgzf_read's inflate under sam_read1 (src/gencore.cpp:205-274 via htslib); member k lies at comp + coff[k],
 * csize[k] bytes (its BSIZE + 1), usize[k] = its ISIZE.  Their bytes follow what was pushed before.  A damaged member makes gce_raw_finish
 * fail with GCE_ERR_INVALID. */
int gce_raw_push_bgzf(gce_engine *e, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, int32_t *ticket);
/* The same decoder on the caller's buffers (tests, tools): out receives the members' bytes back to back; first_bad = -1 or the first damaged member. */
int gce_bgzf_inflate(int32_t device, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, void *out, int32_t *first_bad);
int gce_raw_finish(gce_engine *e, uint64_t records_begin, int32_t n_ref, int64_t *n_records);
int gce_raw_build_output(gce_engine *e, uint64_t *body_bytes, int64_t *n_out);
int gce_raw_read_output_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket);
/* The output record stream (gce_raw_build_output / gce_raw_merge_outputs) compressed into BGZF blocks BY THE GPU -- replaces bgzf_write's deflate
 * under sam_write1 (src/gencore.cpp:104 via htslib): greedy LZ77 + the fixed Huffman codes of RFC 1951, one lane per block, CRC-32 and ISIZE
 * per block (gencore_amd/csrc/gce_deflate.hpp).  *comp_bytes = size of the records' file image; gce_raw_read_deflated_async copies a piece of
 * it out (ticket -> gce_submit_wait).  The caller writes the BAM header's blocks in front and the 28-byte EOF marker behind: what gce_run_bam
 * does for `level == -2` (level -1 = the same scheme on the host's threads; 0..9 = zlib).  gce_bgzf_deflate: the same encoder on the caller's
 * buffer (tests, tools; mirror of gce_bgzf_inflate).  (Additions under ABI v3.) */
int gce_raw_deflate_output(gce_engine *e, uint64_t *comp_bytes);
int gce_raw_read_deflated_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket);
int gce_bgzf_deflate(int32_t device, const void *in, size_t n, uint32_t block_bytes, void *out, size_t out_cap, size_t *out_bytes);
/* The same two with the choice of entropy coder -- replaces the Huffman stage of bgzf_write's deflate under sam_write1 (src/gencore.cpp:104 via
 * htslib).  codes 0: fixed codes (the two functions above are this case).  codes 1: the same tokens, and per block the SMALLEST of dynamic Huffman
 * codes (length-limited to 12 bits, header included), fixed codes and a stored block, each priced exactly from the block's symbol histogram before
 * a byte is written: never larger than codes 0, block for block (k_bgzf_deflate_dyn; what gce_run_bam does for `level == -3`).  codes 2: dynamic
 * codes wherever they fit the block's slot and a BGZF member (gce_bgzf_deflate_codes only: tests of the degenerate trees; the engine call refuses it).
 * out_cap as for gce_bgzf_deflate.  (Additions under ABI v3.) */
int gce_raw_deflate_output_codes(gce_engine *e, int32_t codes, uint64_t *comp_bytes);
int gce_bgzf_deflate_codes(int32_t device, const void *in, size_t n, uint32_t block_bytes, int32_t codes, void *out, size_t out_cap, size_t *out_bytes);
int gce_host_alloc(size_t bytes, void **out);
void gce_host_free(void *p);

/* Replaces: Gencore::consensus() (src/gencore.cpp:162-293) for one file over SEVERAL engines, one per entry of `devices` (HIP ordinals; they
 * may repeat), ON THE GPU CODEC: the host reads the file once (BAM or SAM text, as gce_run_bam); every engine receives the compressed pieces
 * (its own PCIe link), inflates and indexes the stream on its own GPU, plans it there (gce_stream_context + gce_plan_shards, plan_mode as
 * there: the same plan on every device, nothing exchanged) and keeps its range of the cluster key with the reads' global ticks and the
 * stream's flush events (gce_raw_select_shard); the engines run side by side; their record streams -- each in bamComp order -- are merged
 * device to device on devices[0] (gce_raw_merge_outputs: order from 32 bytes per record on the host, bytes moved by the GPU), the Stats blocks
 * summed in device memory; one writer.  Same records, same order, same Stats as gce_run_bam.  Needs every mapped read in front of the first
 * unmapped one (a coordinate-sorted file).  params->device / tick_offset / trailing_flush are ignored.  An output name that ends in "sam" is
 * written as text.  GCE_BAM_HOSTCODEC=1 (or gce_run_bam_sharded_hostcodec): round 2's runner -- host inflate / index / cut, per-shard
 * reference windows, host merge; BAM in and out only. */
int gce_run_bam_sharded(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int32_t n_shards,
                        const int32_t *devices, int32_t plan_mode, int threads, int level, gce_bam_run *out, char err[256]);
int gce_run_bam_sharded_hostcodec(const char *in_path, const char *out_path, const char *fasta_path, const gce_params *params, int32_t n_shards,
                                  const int32_t *devices, int32_t plan_mode, int threads, int level, gce_bam_run *out, char err[256]);
/* The pieces of the sharded runner (additions under ABI v3; gencore_amd/csrc/gce_bamdev.hpp).
 *   gce_raw_attach_mirror: from now on every gce_raw_push / gce_raw_push_bgzf to `e` goes to `mirror` as well (same bytes, same tickets);
 *   gce_raw_select_shard (after gce_raw_finish, before gce_process): the engine keeps shard `rank` of `world` of the stream it holds (the
 *     reference's read loop src/gencore.cpp:205-274 restricted to one range of the cluster key, with the tick and the flush walk of the
 *     whole stream, :319-354);
 *   gce_raw_merge_outputs (after every engine's gce_raw_build_output): one record stream in bamComp order (src/gencore.h:19-47 over the
 *     whole file) in engs[0]'s output buffer -- read it with gce_raw_read_output_async(engs[0], ...) --, both Stats blocks summed. */
int gce_raw_attach_mirror(gce_engine *e, gce_engine *mirror);
int gce_raw_select_shard(gce_engine *e, int32_t world, int32_t rank, int32_t plan_mode);
int gce_raw_merge_outputs(gce_engine **engs, int32_t n_engs, uint64_t *body_bytes, int64_t *n_out_total, gce_stats *pre, gce_stats *post, int64_t *n_reads_total);
/*   gce_stats_payload_sum (after every engine's gce_stats_payload_device with the same step and regions): the payloads of engs[1..] added into
 *     engs[0]'s in device memory (device-to-device copies, no host bounce, no collective): the merged depth / BED vectors of one file over several engines. */
int gce_stats_payload_sum(gce_engine **engs, int32_t n_engs, const int64_t **payload, gce_payload_layout *layout);
/* The payload (an engine's own, or the sum on engs[0]) copied to the host: n_words int64. */
int gce_stats_payload_read(gce_engine *e, const int64_t *payload, int64_t n_words, int64_t *host);

/* gce_run_bam / gce_run_bam_sharded WITH the depth statistics of the reference's report (Options::coverageStep, Options::bedFile; src/stats.cpp:56-83,
 * src/bed.cpp:64-79,111-168): n_shards == 1 runs one engine on devices[0] (devices NULL: params->device), n_shards > 1 the sharded runner on the GPU
 * codec.  After the consensus run every engine computes its Stats payload on its GPU (gce_stats_payload_device: the reads it holds are resident),
 * the payloads are summed in device memory (gce_stats_payload_sum) and come back here once.  bed_path may be NULL (no regions).  The arrays of
 * `depth` are malloc'ed: gce_depth_run_free.  depth->pre / post are the Stats blocks AS THEY WERE SUMMED IN THE PAYLOAD (equal to out->pre / out->post). */
typedef struct gce_depth_run {
    int32_t  n_targets;
    int64_t  n_bins;
    int64_t *bin_off;             /* [n_targets + 1] */
    int64_t *pre_depth, *post_depth;      /* [n_bins] */
    int32_t  n_regions;
    int32_t *region_tid, *region_start, *region_end;   /* the BED file's regions in file order (gce_bed_load) */
    int64_t *pre_bed, *post_bed;          /* [n_regions] */
    gce_stats pre, post;
    int64_t  payload_bytes;       /* size of the one buffer a multi-GPU run merges */
} gce_depth_run;
int gce_run_bam_depth(const char *in_path, const char *out_path, const char *fasta_path, const char *bed_path, int32_t coverage_step, const gce_params *params,
                      int32_t n_shards, const int32_t *devices, int32_t plan_mode, int threads, int level, gce_bam_run *out, gce_depth_run *depth, char err[256]);
void gce_depth_run_free(gce_depth_run *depth);

/* gce_run_bam_depth on ONE device for a file of any size (addition under ABI v3; gencore_amd/csrc/gce_passes.hpp): the stream is
 * processed in P key-range passes so that device memory is bounded by the largest pass, not by the file.  A key pass streams the file once and
 * keeps 12 bytes per read (cluster key and weight); the plan cuts the cluster keys into P contiguous ranges balanced by weight (gce_plan_shards
 * mode 2); pass k streams the file again and keeps only the records of range k, with their global ticks and the flush events of the whole
 * stream; its output records below the smallest (tid, pos) of any later pass's read are written, the rest are held for the next pass's merge
 * (bamComp order with the input index as the last key, as gce_raw_merge_outputs).  Records, order, Stats, depth and BED counts equal
 * gce_run_bam_depth's.
 *   device_budget_bytes: 0 = auto, GCE_PASS_BUDGET_FRACTION of the device's free memory (hipMemGetInfo) when the call starts;
 *   min_passes: at least this many passes (tests force P with it); with auto and min_passes <= 1 a file whose estimate fits in one pass runs
 *     gce_run_bam_depth's single-pass path unchanged;
 *   window_bytes: compressed bytes per window, 0 = 64 MB (the GPU inflate wants thousands of BGZF members per launch).
 * GCE_ERR_OOM (before any output record is written) when the budget cannot hold the fixed part of a pass or the key pass's state, or one
 * cluster key outweighs a pass.  With the auto budget and min_passes <= 1 the single-pass path runs whenever the plan needs one pass (or the
 * key pass / plan cannot be made): behaviour changes only for files that do not fit.  SAM text input is not processed in passes: with the
 * auto budget it runs the single-pass path; GCE_ERR_OOM when an explicit budget is below its estimate, GCE_ERR_INVALID when min_passes > 1.
 * run->peak_device_bytes: the most device bytes the process's engine allocations held at once during the call (gce_device_bytes). */
#define GCE_PASS_BUDGET_FRACTION 0.85
/* The estimator: a read stands for GCE_PASS_WEIGHT_A x its record bytes + GCE_PASS_WEIGHT_B device bytes in a pass. */
#define GCE_PASS_WEIGHT_A 6u
#define GCE_PASS_WEIGHT_B 1024u
typedef struct gce_pass_run {
    int32_t  n_passes;
    int32_t  single_pass;           /* 1: the single-pass path ran (auto, the estimate fits) */
    int64_t  reads_per_pass[64];    /* records given to each pass's engine */
    int64_t  held_max;              /* the most output records held across a pass boundary */
    int64_t  peak_device_bytes;
    int64_t  budget_bytes;          /* the budget the plan used */
    int64_t  fixed_bytes;           /* device bytes live beside a pass's own: engine, reference, window buffers */
    int64_t  pass_room;             /* weight one pass may hold: budget - fixed part - reserve (0: passes forced without a budget) */
    int64_t  total_weight;          /* the estimator's weight of the stream (GCE_PASS_WEIGHT_A x record bytes + GCE_PASS_WEIGHT_B per read) */
    double   key_pass_s;
    double   pass_s[64];
} gce_pass_run;
int gce_run_bam_passes(const char *in_path, const char *out_path, const char *fasta_path, const char *bed_path, int32_t coverage_step, const gce_params *params,
                       int32_t device, int threads, int level, size_t device_budget_bytes, int32_t min_passes, size_t window_bytes,
                       gce_bam_run *out, gce_depth_run *depth, gce_pass_run *run, char err[256]);
/* The BAI index (SAMv1 5.2) of a coordinate-sorted BAM file, built on ONE device (addition under ABI v3; gencore_amd/csrc/gce_bai.hpp,
 * DESIGN.md 4c).  The file is streamed in windows of window_bytes compressed bytes (0 = 64 MB) as gce_run_bam_passes streams it: the GPU inflates
 * every window and finds its records; 24 bytes per record stay in device memory (GCE_ERR_OOM with a message when they do not fit).  The bins,
 * chunks, linear index and per-contig counts follow DESIGN.md 4c (bins not folded into their parents, written in ascending order).  The index is
 * written to a temporary name beside bai_path and renamed at the end: a failed call leaves no index and never touches the BAM.  GCE_ERR_INVALID
 * with a message when the input is not BGZF or is truncated, or when a record is out of (tid, pos) order or ends beyond 2^29 (the message names
 * the record, counting from 0).  threads: host threads for inflating the header (0 = all cores). */
typedef struct gce_bai_run {
    int64_t n_records;              /* records read */
    int64_t n_no_coor;              /* records with tid < 0 */
    int64_t n_bins, n_chunks, n_intervals;   /* written to the .bai, pseudo-bins excluded */
    int32_t n_ref, pad;
    double  read_s, gpu_s, write_s, total_s;
} gce_bai_run;
int gce_bam_index(const char *bam_path, const char *bai_path, int32_t device, int threads, uint64_t window_bytes, gce_bai_run *out, char err[256]);
/* An unsorted BAM file into coordinate order on ONE device (addition under ABI v3; gencore_amd/csrc/gce_sort.hpp).
 * Replaces: nothing in the reference's source -- it stands in for the `samtools sort` the reference's README asks for in front of gencore (every
 * runner here stops with GCE_ERR_UNSORTED otherwise).  The file is streamed in windows of window_bytes compressed bytes (0 = 64 MB) as
 * gce_bam_index streams it; the GPU inflates every window, finds its records and keys them; records are ordered by (tid with the unplaced ones
 * last, pos + 1, reverse-strand bit, input index), their bytes are moved unchanged, and the header's @HD line gets SO:coordinate (DESIGN.md 4d,
 * rules S / R / H / F).  level: as gce_run_bam, -3..9 (-2 / -3: the GPU deflates the record stream; the members hold 0xff00 input bytes each).
 * The sort is in-core: about 2 x the inflated record bytes + 20 bytes per record + one window of device memory; device_budget_bytes (0 = no
 * limit beyond the device) bounds the process's live device bytes (gce_device_bytes) and is checked before every growth of a buffer that scales with the file or
 * the window: GCE_ERR_OOM with a
 * message that states the footprint, before any output exists.  The output is written to a temporary name beside out_path and renamed at the end: a
 * failed call leaves neither an output nor a temporary file and never touches the input; an out_path that resolves to the input is refused.
 * GCE_ERR_INVALID with a message for SAM text ("gce_bam_sort reads BAM, not SAM text"), a file that is not BGZF or is truncated, and a record
 * whose tid the header does not have (the message names the record, counting from 0). */
typedef struct gce_sort_run {
    int64_t n_records, n_no_coor, n_descents;   /* n_descents == 0: the input was already in rule S's order */
    int64_t inflated_bytes, out_bytes, peak_device_bytes;   /* record bytes sorted; size of the file written; gce_device_bytes' peak during the call */
    int32_t n_ref, pad;
    double  read_s, inflate_index_s, sort_s, gather_s, write_s, total_s;
} gce_sort_run;
int gce_bam_sort(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes,
                 size_t device_budget_bytes, gce_sort_run *out, char err[256]);
/* gce_bam_sort for a file beyond its in-core limit, on ONE device (addition under ABI v3; gencore_amd/csrc/gce_sort.hpp): the same
 * output, byte for byte.  device_budget_bytes: 0 = auto, GCE_PASS_BUDGET_FRACTION of the device's free memory when the call starts, as in
 * gce_run_bam_passes.  With min_passes <= 1, gce_bam_sort is tried with that budget first, unless even the compressed file is beyond half of it
 * (run->in_core = 1 when it wrote the output).  On its GCE_ERR_OOM, or with min_passes >= 2, the file is sorted in output-range passes: a key
 * pass streams it and keeps key and size of every record (12 bytes per record + one window); the plan sorts the keys, scans the sizes and keeps
 * the destination byte offset of every record in input order (8 bytes per record resident from then on; about 44 bytes per record at its
 * peak); the sorted stream [0, total) is cut into P ranges of pass_bytes, P = max(min_passes, what the budget needs), at most 64,
 * pass_bytes = ceil(total / P) rounded up to a multiple of 0xff00, n_passes = ceil(total / pass_bytes); every pass streams the file again
 * from its first byte, the GPU moves the bytes that fall into the pass's range (a record that straddles a cut partly in each pass) and that
 * range is written as gce_bam_sort writes it.  No sorted runs are spilled to host memory or disk and nothing is merged on the host; host
 * buffers do not grow with the file.  GCE_ERR_OOM, with a message that states this footprint, before any output exists when the budget cannot
 * hold the plan, or the destinations + one window + a pass of one BGZF member with its deflate buffers.  GCE_ERR_INVALID ("the input changed
 * while it was being sorted") when a pass sees other records than the key pass saw.  Temporary file, rename and the other refusals:
 * gce_bam_sort's, in its words.  *out as gce_bam_sort fills it: sort_s is the plan, gather_s the sum of the passes' k_sort_scatter launches,
 * read_s / inflate_index_s / write_s sums over the key pass and every pass, peak_device_bytes the peak of the path that wrote the output. */
typedef struct gce_sort_pass_run {
    int32_t n_passes, in_core;                  /* in_core: gce_bam_sort wrote the output (then n_passes is 1, or 0 for a file without records) */
    int64_t pass_bytes, resident_bytes;         /* resident_bytes: device bytes held while the passes run, a window's aside (in_core: the peak) */
    double  key_pass_s, plan_s, pass_s[64];     /* pass_s[k]: pass k, its range written (in_core: [0] = sort + gather + write) */
} gce_sort_pass_run;
int gce_bam_sort_passes(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes,
                        size_t device_budget_bytes, int32_t min_passes, gce_sort_run *out, gce_sort_pass_run *run, char err[256]);
/* NM and MD of every record recomputed against the reference on ONE device, file to file (addition under ABI v3; gencore_amd/csrc/gce_calmd.hpp,
 * DESIGN.md 4g).  Replaces: nothing in the reference's source -- it stands in for the `samtools calmd` a pipeline runs behind the reference,
 * whose consensus records carry the MD:Z of one read of their cluster and an NM it patches only when stored as type C (src/group.cpp:531-570),
 * and in front of it for an input without NM (every runner here stops with GCE_ERR_NM_MISSING otherwise, src/group.cpp:532-535).  The file is
 * streamed in windows of window_bytes compressed bytes (0 = 64 MB) as gce_bam_sort streams it; the GPU inflates every window, finds its
 * records, walks each eligible record's CIGAR over its bases and the contig (rules E / R / W), drops every NM and MD field and appends
 * NM (type C, S or I, the smallest that holds it) and MD:Z (rule T); every other byte of the record, every ineligible record (unmapped, no
 * CIGAR, no bases, a contig the FASTA lacks: n_no_ref, ...) and the header stay as they are, in the input's order.  fasta_path: as
 * gce_run_bam reads it (gce_fasta_load); contigs are matched to the header by name.  level and the file's layout (rule F): gce_bam_sort's.
 * In-core: about the output record bytes + the reference bases + 40 bytes per window record + one window of device memory;
 * device_budget_bytes (0 = no limit beyond the device) is checked before every growth: GCE_ERR_OOM with a message that states this
 * footprint, before any output exists.  Temporary file, rename and an out_path that resolves to the input: as gce_bam_sort.
 * GCE_ERR_INVALID with a message for a NULL path, a level outside -3..9 and a fasta_path that does not exist (all before a device is
 * touched), for SAM text ("gce_bam_calmd reads BAM, not SAM text"), a file that is not BGZF or is truncated, and a record whose optional
 * fields do not tile its block_size (the message names the lowest such record, counting from 0; no output is written). */
typedef struct gce_calmd_run {
    int64_t n_records, n_rewritten, n_unchanged, n_no_ref, n_nm_changed, n_md_changed;   /* n_unchanged = n_records - n_rewritten; n_no_ref of those: the FASTA lacks the contig */
    int64_t inflated_bytes, out_record_bytes, out_bytes, peak_device_bytes;   /* record bytes read / written; size of the file written; gce_device_bytes' peak during the call */
    int32_t n_ref, pad;
    double  read_s, inflate_index_s, calmd_s, write_s, total_s;   /* read_s holds the FASTA's load; calmd_s: the k_md_* kernels and their scan */
} gce_calmd_run;
int gce_bam_calmd(const char *in_path, const char *out_path, const char *fasta_path, int32_t device, int threads, int level,
                  uint64_t window_bytes, size_t device_budget_bytes, gce_calmd_run *out, char err[256]);
/* gce_bam_calmd for a file whose rewritten records do not fit the device: the same file, byte for byte, at every level, with the output
 * streamed (addition under ABI v3; gencore_amd/csrc/gce_calmd.hpp).  calmd never reorders records, so the file is still read
 * once; the temporary output is open before the first window, and whenever a window's output (known after k_md_size and its scan) would take
 * the resident output record bytes past the cap R, the whole members resident so far -- floor(resident / 0xff00) * 0xff00 bytes -- are deflated
 * and written as gce_bam_calmd writes its pieces, and the tail below 0xff00 bytes (which may begin inside a record) moves to the front of the
 * buffer before the window's records are emitted behind it.  Rule F cuts the record stream into members of 0xff00 input bytes and every member
 * is deflated on its own (host zlib, the host's fixed codes, one GPU lane per member at -2 and -3), so the file does not depend on where the
 * stream was cut.  After the last window the rest is written with the last short member, then the EOF marker and the rename.
 * device_budget_bytes: 0 = auto, GCE_PASS_BUDGET_FRACTION of the device's free memory when the call starts, as in gce_bam_sort_passes; it is
 * checked before every growth and out->peak_device_bytes never exceeds an explicit budget.  resident_bytes: 0 = R is what the budget leaves
 * beside the reference bases and their table, one window (and as much again held back for a larger window to come), 40 bytes per window
 * record and the deflate buffers of one piece, found when the first window with records is known; otherwise R is resident_bytes rounded up
 * to a multiple of 0xff00 (how a test forces flushes on a small file).  One window's output always fits beside the tail: the buffer grows
 * to tail + that window's output when the budget allows.  Device memory: the reference bases + one window + 40 bytes per window record +
 * one piece's deflate buffers + at least one window's output; the reference bases stay whole (3.1 GB at hg19).  GCE_ERR_OOM, with a
 * message that states this footprint, when the budget cannot hold it.  A failed call leaves neither an output nor a temporary file and never
 * touches the input, at any point: also for a malformed record found after several flushes were written.  The refusals, the counters in
 * *out and rule C: gce_bam_calmd's, in its words, with gce_bam_calmd_stream where the entry point is named ("gce_bam_calmd_stream reads BAM,
 * not SAM text").  out->write_s holds the flushes; out->inflate_index_s and out->calmd_s do not. */
typedef struct gce_calmd_stream_run {
    int32_t n_flushes, pad;          /* times resident output was written before the final one; 0: nothing left the device before the last window */
    int64_t resident_cap_bytes;      /* the cap R on resident output record bytes that the call worked with (0: auto and no window had records) */
    int64_t flushed_bytes;           /* record bytes written by those n_flushes flushes: a multiple of 0xff00 */
} gce_calmd_stream_run;
int gce_bam_calmd_stream(const char *in_path, const char *out_path, const char *fasta_path, int32_t device, int threads, int level,
                         uint64_t window_bytes, size_t device_budget_bytes, uint64_t resident_bytes,
                         gce_calmd_run *out, gce_calmd_stream_run *run, char err[256]);
/* Overlapping mates resolved in the file on ONE device, file to file (addition under ABI v3; gencore_amd/csrc/gce_ovlmerge.hpp).
 * Replaces: nothing in the reference's source -- it stands in for the tool a pipeline runs behind the reference so that a pileup of the
 * output counts every fragment once (`fgbio ClipBam --clip-overlapping-reads`, `bamUtil clipOverlap`, mpileup's own overlap tweak), and
 * writes gce_bam_pileup_fragments' rule V into the records.  Nothing but QUAL bytes changes: record sizes, positions, CIGARs, NM / MD, the
 * record order and the header (copied byte for byte) stay.  Rule P: the file is coordinate-sorted; the first record in front of its
 * predecessor is GCE_ERR_INVALID ("BAM record %d (counting from 0) lies in front of its predecessor: gce_bam_merge_overlap needs a
 * coordinate-sorted file").  Rule E: a record takes part when gce_bam_pileup's rule E keeps it under min_mapq (0..255) and exclude_flags; a
 * record whose fields overrun its block_size refuses the run, in gce_bam_pileup's words, before rule P is looked at.  Rule M:
 * gce_bam_pileup_fragments' mates without the site test, joined over the whole file at once (the result does not depend on window_bytes);
 * every member of a group of more than two adds to n_ambiguous and is left alone.  Rule Q, for a pair whose earlier record in the file is a:
 * a pair with a record without qualities is left alone (n_pairs_no_qual); at every reference column that an M / = / X op of both mates
 * covers (n_shared_columns), with qualities qa, qb and base classes A C G T N: a column where qa or qb is 0 or above 93 is left as it is
 * (n_columns_skipped; the pass is idempotent); equal classes: qa' = min(qa + qb, 93), qb' = 0; different classes (n_disagree_columns):
 * qa >= qb: qa' = (4 qa) / 5, qb' = 0, else qb' = (4 qb) / 5, qa' = 0.  D and N columns, clips and inserted bases are not touched.
 * n_records_changed: records of which at least one byte differs.  options: GCE_OVERLAP_WEAK_HASH keeps 4 bits of the join's hash (a test's
 * switch: the same file, long probe runs).  level and the file's layout (rule F): gce_bam_calmd's.  In-core: the inflated record bytes + 20
 * bytes per record + one window, then a join table of about 24 bytes per record in place of 12 of the 20; device_budget_bytes (0 = no limit
 * beyond the device) is checked before every growth: GCE_ERR_OOM with a message that states this footprint.  A failed call leaves neither an
 * output nor a temporary file.  The other refusals: gce_bam_calmd's, with this entry point's name. */
#define GCE_OVERLAP_WEAK_HASH 1u
typedef struct gce_overlap_run {
    int64_t n_records, n_pairs, n_pairs_no_qual, n_ambiguous, n_shared_columns, n_disagree_columns, n_columns_skipped, n_records_changed;
    int64_t inflated_bytes, out_bytes, peak_device_bytes;   /* record bytes read (and written); size of the file written; gce_device_bytes' peak during the call */
    int32_t n_ref, pad;
    double  read_s, inflate_index_s, merge_s, write_s, total_s;   /* merge_s: the check, the join and k_ovl_merge behind the last window */
} gce_overlap_run;
int gce_bam_merge_overlap(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes,
                          size_t device_budget_bytes, int32_t min_mapq, uint32_t exclude_flags, uint32_t options, gce_overlap_run *out,
                          char err[256]);
/* The UMI of every record moved into an MI:Z field on ONE device, file to file (addition under ABI v3; gencore_amd/csrc/gce_umi.hpp,
 * DESIGN.md 4h).  Replaces: nothing in the reference's source -- it feeds BamUtil::getUMI's MI:Z path (src/bamutil.cpp:23-38), which every
 * runner here follows: a UMI is the last `:`-field of an MI:Z value or of the read name, of A C G T with at most one `_`.  A file whose UMIs are in
 * an RX:Z tag (fgbio, DRAGEN, `bwa mem -C`: ACGT-TTGA) or in an Illumina name (...:ACGT+TTGA) runs with every UMI empty otherwise.  source: a
 * two-character tag, or "name".  Per record: the source string s is the value of the first optional field with that tag if its type is Z, or
 * what is behind the last `:` of the read name; a record without one (no field, no `:`, another type, s empty) is copied whole (n_no_source),
 * and so is one whose s is not a UMI (n_not_umi): a byte other than ACGTNacgtn - + _, more than one of - + _, one of them first or last, or more
 * than 250 bytes.  Every other record (n_tagged) loses its MI fields of any type (n_mi_dropped counts the records that had one) and gets
 * MI:Z:":" + s, upper case and with - and + as _, behind its last kept field; block_size follows and nothing else changes.  An N is passed on:
 * the run reads such a UMI as "", as the reference does.  The header is kept and the records stay in order.  The output is streamed as
 * gce_bam_calmd_stream streams it, within device_budget_bytes (0: auto); resident_bytes forces the cap (0: what the budget leaves); level,
 * window_bytes, the temporary file, the rename and an out_path that resolves to the input: as there.
 * GCE_ERR_INVALID with a message, before a device is touched, for a NULL argument, a level outside -3..9, a source that is neither "name" nor
 * [A-Za-z][A-Za-z0-9], source "MI" (the run reads that tag without this pass), an input that cannot be opened and SAM text; later for a
 * record whose optional fields do not tile its block_size or whose new block_size would pass 2^28 (the message names the lowest such record,
 * counting from 0).  A failed call leaves neither an output nor a temporary file. */
typedef struct gce_umi_run {
    int64_t n_records, n_tagged, n_no_source, n_not_umi, n_mi_dropped;   /* n_tagged + n_no_source + n_not_umi = n_records; n_mi_dropped of the tagged */
    int64_t n_flushes, inflated_bytes, out_record_bytes, out_bytes, peak_device_bytes;   /* n_flushes: as gce_calmd_stream_run's */
    double  read_s, inflate_index_s, umi_s, write_s, total_s;   /* umi_s: the k_umi_* kernels and their scan; write_s holds the flushes */
} gce_umi_run;
int gce_bam_umi_to_mi(const char *in_path, const char *out_path, const char *source, int32_t device, int threads, int level,
                      uint64_t window_bytes, size_t device_budget_bytes, uint64_t resident_bytes, gce_umi_run *out, char err[256]);
/* Bases per strand at the sites of a BED file, counted on ONE device (addition under ABI v3; gencore_amd/csrc/gce_pileup.hpp).
 * Replaces: nothing in the reference's source -- it stands in for the `samtools mpileup` / `bam-readcount` a panel's user runs on the input
 * and on the consensus output to see which mismatches consensus removed; the reference's own report carries depth per bin and per region only
 * (src/stats.cpp:57-84, src/bed.cpp:66-81).  Sites: the union of the BED's regions (gce_bed_load against the BAM header), each clamped to its
 * contig, merged into intervals, in (tid, pos) order; a region on an unknown contig gives none; more than 2^28 sites is GCE_ERR_INVALID.  The
 * file is streamed in windows of window_bytes compressed bytes (0 = 64 MB) as gce_bam_index streams it, in any record order.  A record is
 * counted when 0 <= tid < n_ref and pos >= 0 (else n_unplaced), no bit of exclude_flags is set (n_flagged), mapq >= min_mapq (n_low_mapq),
 * n_cigar_op > 0 (n_no_cigar), l_seq > 0 (n_no_seq), every CIGAR op is 0..8 and the CIGAR's query length is l_seq (n_bad_cigar): the first test
 * that fails decides the counter.  Per site and strand (flag 0x10) eight uint32 counters: A C G T N DEL INS LOWQ.  An M / = / X column adds
 * to its base's class (nibbles 1 2 4 8; every other nibble is N), or to LOWQ when the record has qualities and the base's is below min_baseq;
 * a D column adds to DEL; an I op that follows an M / = / X / D op adds one to INS of the site in front of it; N skips; S, H, P add nothing.
 * Overlapping mates are counted twice, there is no BAQ and no split by read group.  tsv_path (NULL: no file): a tab-separated table, a header
 * line that begins with `#`, then one line per site: contig, 1-based pos, ref, depth (A + C + G + T + N of both strands), the forward
 * strand's eight counters, the reverse strand's; ref is the upper-case byte of fasta_path's contig of that name, N where it has none or
 * fasta_path is NULL (the reference never goes to the device).  The table is written to a temporary name beside tsv_path and renamed.
 * options: GCE_PILEUP_DIRECT makes every add a global atomic (no LDS tile): the same counters, the A/B partner of the default.  Device memory:
 * 64 bytes per site, the interval table, one window and 4 bytes per window record, within device_budget_bytes (0: no limit), else GCE_ERR_OOM
 * with that footprint.  GCE_ERR_INVALID with a message, before a device is touched, for a NULL bam_path, bed_path or out, min_mapq or min_baseq
 * outside 0..255, an unknown option bit, a BED or FASTA that does not exist and SAM text; later for a record whose fields overrun its
 * block_size (the message names the lowest such record, counting from 0) and for a file whose eligible records hold 2^32 CIGAR operations or
 * more.  A failed call leaves neither a table nor a temporary file.  site_tid, site_pos (0-based) and counts (16 per site) are malloc'ed:
 * gce_pileup_free. */
#define GCE_PILEUP_DIRECT 1u
typedef struct gce_pileup_run {
    int64_t n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar;   /* n_eligible + the six skips = n_records */
    int64_t n_sites, n_intervals, peak_device_bytes;
    double  read_s, inflate_index_s, pileup_s, write_s, total_s;   /* pileup_s: k_pile_scan and k_pile_count; write_s: the table */
    int32_t *site_tid, *site_pos;   /* [n_sites] */
    uint32_t *counts;               /* [n_sites][2 strands][8 classes] */
} gce_pileup_run;
int gce_bam_pileup(const char *bam_path, const char *bed_path, const char *fasta_path /* NULL: ref = N */, const char *tsv_path /* NULL: no file */,
                   int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options,
                   uint64_t window_bytes, size_t device_budget_bytes, gce_pileup_run *out, char err[256]);
void gce_pileup_free(gce_pileup_run *out);
/* gce_bam_pileup's table with every fragment counted once where its mates overlap, on ONE device (addition under ABI v3;
 * gencore_amd/csrc/gce_fragpile.hpp).  Replaces: nothing in the reference's source -- it is the overlap handling of the
 * `samtools mpileup` / `bam-readcount` that gce_bam_pileup stands in for, in outline.  The arguments, sites, record tests, walk, table and
 * gce_pileup_run's counters are gce_bam_pileup's; a record without a partner is counted exactly as gce_bam_pileup counts it.  Rule P: the
 * file is coordinate-sorted -- placed records (tid >= 0) in non-decreasing (tid, pos), every record with tid < 0 behind them; the first
 * record that breaks this ends the run with GCE_ERR_INVALID ("BAM record N (counting from 0) lies in front of its predecessor: ..."),
 * whether or not a site is near, across windows too; within a window the malformed-record refusal comes first.  Rule M: a counted record
 * that can touch a site is a candidate when its flag has 0x1, none of 0x4 0x8 0x100 0x800 and exactly one of 0x40 / 0x80, next_refID ==
 * refID, and next_pos < pos + its reference span when next_pos >= pos.  Two candidates are a pair when their names are byte-equal
 * (with l_read_name), their refIDs equal, one has 0x40 and the other 0x80, and each lies at the other's next_pos; a, the earlier in the
 * file.  More than two candidates of one name, refID and unordered {pos, next_pos}: none pairs, each adds to n_ambiguous (defined for
 * groups inside one window).  A candidate with next_pos >= pos and no partner yet waits (carried across windows on the device, n_deferred)
 * until a placed record beyond (refID, next_pos), a record with tid < 0 or the end of the file shows that none can come; then it is
 * counted alone.  The result does not depend on window_bytes.  Rule V, for a pair, at every site column that an M / = / X / D op of both
 * mates covers (n_shared_columns): each mate has a raw class (A C G T N, DEL for a D column) and a quality (its QUAL byte; 0 for a D column
 * or without qualities).  Same class: a is counted, with quality min(qa + qb, 200) for the LOWQ test, b adds nothing.  Different classes
 * (n_disagree_columns): the winner is a when qa >= qb, else b, counted with quality (4 q) / 5; the loser adds nothing.  The winner adds,
 * on its own strand, to DEL for a DEL, else to LOWQ when it has qualities and the adjusted quality is below min_baseq, else to its class.
 * Columns one mate alone covers, and every I op of both mates, are counted as gce_bam_pileup counts them.  No BAQ, no split by read group.
 * options: GCE_FRAGPILE_DIRECT as GCE_PILEUP_DIRECT; GCE_FRAGPILE_WEAK_HASH keeps 4 bits of the join's 64-bit hash: the same counters, a
 * test's handle on long probe runs.  Device memory: gce_bam_pileup's, 16 bytes per window record, a join table of 4 bytes per slot (at
 * least twice the records) and two arenas of deferred records, within device_budget_bytes, else GCE_ERR_OOM with that footprint.  The
 * refusals are gce_bam_pileup's, and rule P's.  site_tid, site_pos and counts are malloc'ed: gce_fragpile_free. */
#define GCE_FRAGPILE_DIRECT 1u
#define GCE_FRAGPILE_WEAK_HASH 2u
typedef struct gce_fragpile_run {
    int64_t n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar;   /* n_eligible + the six skips = n_records */
    int64_t n_sites, n_intervals, peak_device_bytes;
    double  read_s, inflate_index_s, pileup_s, write_s, total_s;   /* pileup_s: the scan, the join, k_frag_count and the carry; write_s: the table */
    int32_t *site_tid, *site_pos;   /* [n_sites] */
    uint32_t *counts;               /* [n_sites][2 strands][8 classes] */
    int64_t n_pairs, n_shared_columns, n_disagree_columns, n_ambiguous, n_deferred;   /* n_deferred alone depends on window_bytes */
} gce_fragpile_run;
int gce_bam_pileup_fragments(const char *bam_path, const char *bed_path, const char *fasta_path /* NULL: ref = N */, const char *tsv_path /* NULL: no file */,
                             int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options,
                             uint64_t window_bytes, size_t device_budget_bytes, gce_fragpile_run *out, char err[256]);
void gce_fragpile_free(gce_fragpile_run *out);
/* Mismatches by read cycle against the reference, counted on ONE device (addition under ABI v3; gencore_amd/csrc/gce_errprof.hpp).
 * Replaces: nothing in the reference's source -- it stands in for the `fgbio ErrorRateByReadPosition`, Picard artifact metrics or `samtools
 * stats` mismatches-per-cycle a user runs on the input and on the consensus output to see how far the error rate fell; the reference's own
 * report carries one mismatch total from NM (src/stats.cpp:103-108).  One streaming pass over bam_path in any record order.  Eligible records:
 * gce_bam_pileup's tests in its order (n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar), then n_no_ref (fasta_path lacks
 * the contig, matched by name as gce_bam_calmd matches it) and n_too_long (l_seq > GCE_ERRPROF_MAX_CYCLE).  Segment: 1 for flag 0x40 without
 * 0x80, 2 for 0x80 without 0x40, else 0.  Cycle of query index y: y + 1, on the reverse strand l_seq - y (hard clips are not counted).
 * counts[(segment * 1024 + cycle - 1) * 24 + class]; classes 0..15: 4 r + b, reference base r against read base b over A C G T in sequencing
 * orientation (both complemented on the reverse strand); 16 READ_N, 17 REF_OTHER, 18 LOWQ, 19 INS, 20 DEL, 21..23 zero (21 is MASKED under gce_bam_error_profile_masked).  An M / = / X column:
 * LOWQ when QUAL[0] != 0xFF and its quality < min_baseq, else REF_OTHER when it lies at or beyond the contig's FASTA length or the upper-cased
 * reference byte is not A C G T, else READ_N when the read nibble is not 1, 2, 4 or 8, else 4 r + b.  Every inserted base adds INS at its own
 * cycle; a D adds one DEL at the cycle of the query base in front of it (the first, when there is none).  bed_path (NULL: none) restricts the
 * events to the union of its regions (clamped, merged and matched against the header as gce_bam_pileup does): a column by its own position, an
 * inserted base by the position in front of it (its own when no M = X D came earlier), a deletion by its first position.  tsv_path (NULL: no
 * file): a header line that begins with `#`, then per segment with a counter one line per cycle from 1 to the last with a counter: segment,
 * cycle, bases (classes 0..15), mismatches (the off-diagonal ones), the sixteen A>A .. T>T, READ_N REF_OTHER LOWQ INS DEL; written to a
 * temporary name and renamed.  options: GCE_ERRPROF_DIRECT makes every add a 64-bit global atomic (no LDS planes): the same counters, the A/B
 * partner of the default.  Device memory: the reference bases, 576 KiB of counters, the interval table, one window and 4 bytes per window
 * record, within device_budget_bytes (0: no limit), else GCE_ERR_OOM with that footprint.  GCE_ERR_INVALID with a message, before a device is
 * touched, for a NULL bam_path, fasta_path or out, min_mapq or min_baseq outside 0..255, an unknown option bit, a FASTA or BED that does not
 * exist and SAM text; later for a record whose fields overrun its block_size (the message names the lowest such record, counting from 0).  A
 * failed call leaves neither a table nor a temporary file.  counts (3 x 1024 x 24) is malloc'ed: gce_errprof_free. */
#define GCE_ERRPROF_DIRECT 1u
#define GCE_ERRPROF_MAX_CYCLE 1024
#define GCE_ERRPROF_CLASSES 24
typedef struct gce_errprof_run {
    int64_t n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar, n_no_ref, n_too_long;   /* n_eligible + the eight skips = n_records */
    int64_t n_bases, n_mismatches, n_intervals /* -1: no BED */, peak_device_bytes;
    double  read_s, inflate_index_s, errprof_s, write_s, total_s;   /* errprof_s: k_err_scan and k_err_count; write_s: the table */
    uint64_t *counts;               /* [3 segments][1024 cycles][24 classes] */
} gce_errprof_run;
int gce_bam_error_profile(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *tsv_path /* NULL: no file */,
                          int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options,
                          uint64_t window_bytes, size_t device_budget_bytes, gce_errprof_run *out, char err[256]);
void gce_errprof_free(gce_errprof_run *out);
/* gce_bam_error_profile's table with every fragment counted once where its mates overlap, and a second table of what the two mates say of
 * each other there, on ONE device (addition under ABI v3; gencore_amd/csrc/gce_fragerr.hpp).
 * Replaces: nothing in the reference's source -- it stands in for the `fgbio ErrorRateByReadPosition` / Picard artifact metrics that
 * gce_bam_error_profile stands in for, which count overlapping mates twice and cannot tell a sequencing error from an older one at a site
 * no variant mask names (gce_bam_error_profile_fragments_masked takes one).  The arguments, eligible records, segment, cycle, classes, BED and primary table are gce_bam_error_profile's; a record
 * without a partner is counted exactly as gce_bam_error_profile counts it.  Rule P (the file is coordinate-sorted;
 * "BAM record N (counting from 0) lies in front of its predecessor: ...") and Rule M (candidates, pairs, n_ambiguous, waiting across
 * windows, n_deferred) are gce_bam_pileup_fragments', with
 * "can touch a site" read as: every eligible record without a BED, with one a record whose reference span touches a region.  Rule V': for a
 * pair (a, the earlier in the file), a shared column (n_shared_columns) is a reference position that an M / = / X op of both mates covers
 * and, with a BED, lies in its regions; a D or N of either mate there: not shared.  Each mate has a base class over A C G T N and a quality
 * (its QUAL byte; 0 without qualities).  In counts: same class, a is counted at its own segment and cycle with quality min(qa + qb, 200)
 * for the LOWQ test, b adds nothing; different classes (n_disagree_columns), the winner is a when qa >= qb, else b, counted with quality
 * (4 q) / 5, the loser adds nothing; the winner's class is then LOWQ (when it has qualities), REF_OTHER, READ_N or 4 r + b as in
 * gce_bam_error_profile.  Insertions and deletions of both mates and all other columns are counted as gce_bam_error_profile counts them.
 * Rule X: overlap[(segment * 1024 + cycle - 1) * 24 + class], where BOTH mates add one at every shared column, each at its own segment and
 * cycle, the first class that applies (m this mate, o the other, r the reference base): 20 OVL_LOWQ when a mate with qualities has a raw
 * quality < min_baseq; 19 OVL_UNUSABLE when either base is N or r is REF_OTHER; 16 OVL_AGREE_REF when bm == bo == r; 17 OVL_AGREE_ALT when
 * bm == bo != r (older than the sequencer, or a variant); bm != bo: 4 r + bm when bo == r (m's sequencing error) or bm == r (the diagonal: m
 * read it right, o did not), both complemented on m's reverse strand; 18 OVL_DIFF_OTHER when neither is r; 21..23 zero.  The sum of overlap
 * is 2 n_shared_columns.  tsv_path as gce_bam_error_profile's; overlap_tsv_path (NULL: no file): a header line that begins with `#`, then
 * per segment one line per cycle up to the last with a counter: segment, cycle, shared (classes 0..18), errors (the off-diagonal ones), the
 * sixteen A>A .. T>T, AGREE_REF AGREE_ALT DIFF_OTHER UNUSABLE LOWQ; each written to a temporary name and renamed.  The result does not
 * depend on window_bytes (n_deferred alone does).  options: GCE_FRAGERR_DIRECT as GCE_ERRPROF_DIRECT; GCE_FRAGERR_WEAK_HASH as
 * GCE_FRAGPILE_WEAK_HASH.  Device memory: gce_bam_error_profile's with 1152 KiB of counters, 16 bytes per window record, a join table of 4
 * bytes per slot and two arenas of deferred records, within device_budget_bytes, else GCE_ERR_OOM with that footprint.  The refusals are
 * gce_bam_error_profile's, and rule P's.  No BAQ, no split by read group.  counts and overlap (3 x 1024 x 24 each) are malloc'ed:
 * gce_fragerr_free. */
#define GCE_FRAGERR_DIRECT 1u
#define GCE_FRAGERR_WEAK_HASH 2u
typedef struct gce_fragerr_run {
    int64_t n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar, n_no_ref, n_too_long;   /* n_eligible + the eight skips = n_records */
    int64_t n_bases, n_mismatches, n_intervals /* -1: no BED */, peak_device_bytes;
    double  read_s, inflate_index_s, errprof_s, write_s, total_s;   /* errprof_s: the scan, the join, k_fragerr_count and the carry; write_s: the tables */
    int64_t n_pairs, n_shared_columns, n_disagree_columns, n_ambiguous, n_deferred;   /* n_deferred alone depends on window_bytes */
    uint64_t *counts, *overlap;     /* [3 segments][1024 cycles][24 classes] each */
} gce_fragerr_run;
int gce_bam_error_profile_fragments(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *tsv_path /* NULL: no file */,
                                    const char *overlap_tsv_path /* NULL: no file */, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags,
                                    uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_fragerr_run *out, char err[256]);
void gce_fragerr_free(gce_fragerr_run *out);
/* gce_bam_error_profile and gce_bam_error_profile_fragments with known variant sites masked (addition under ABI v3;
 * gencore_amd/csrc/gce_varmask.hpp).  Replaces: nothing in the reference's source -- `fgbio ErrorRateByReadPosition --variants`,
 * Picard's DB_SNP.  mask_path is read with gce_mask_load against the header's names, clamped to min(header length, FASTA length), behind the
 * header and the FASTA; a NULL or missing mask_path or a NULL mask is refused before a device is touched, like the FASTA, a name with
 * another ending and a malformed line (gce_mask_load's message) before a window is read.  On the device the mask is one bit per reference
 * base (ref bytes / 8 more device memory, inside device_budget_bytes; GCE_ERR_OOM names `the variant mask`).  Rule Y: class 21 of every
 * (segment, cycle) row is MASKED, in the overlap table OVL_MASKED.  An event whose anchor is masked goes there, at the segment and cycle it
 * would have had, instead of to any other class: an M / = / X column by its own position (tested in front of LOWQ), every inserted base by
 * the position in front of it (its own when no M = X D came earlier), a deletion by its first position; an anchor outside [0, FASTA length)
 * is not masked; with a BED its test comes first, so an event off the targets is still not counted.  At a shared masked column of a pair the
 * one mate rule V' counts adds MASKED to counts, both add OVL_MASKED to overlap; n_shared_columns, n_disagree_columns and the sum of overlap
 * stay what they are.  So per (segment, cycle) the sum of classes 0..21 equals the sum of 0..20 without a mask, and n_bases, n_mismatches,
 * shared and errors (classes 0..15 and 0..18) lose the masked sites.  The tables get one more trailing column, MASKED, in the header line
 * and every row.  Everything else is the unmasked entry point's, whose counters, tables and structs do not change.  *mask: what
 * gce_mask_load counted, n_masked_events (the sum of class 21 of counts), load_s (the file read and parsed on the host) and fill_s (a host clock around the set_mask calls: the bitmap's allocation and zeroing, the
 * staging copies, k_mask_fill and a synchronise per 65 536 intervals). */
typedef struct gce_mask_run {
    int64_t n_lines, n_records, n_unknown_contig, n_no_alt, n_intervals, n_masked_bases, n_masked_events;
    double  load_s, fill_s;
} gce_mask_run;
int gce_bam_error_profile_masked(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *mask_path, const char *tsv_path /* NULL: no file */,
                                 int32_t device, int threads, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options,
                                 uint64_t window_bytes, size_t device_budget_bytes, gce_errprof_run *out, gce_mask_run *mask, char err[256]);
int gce_bam_error_profile_fragments_masked(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *mask_path,
                                           const char *tsv_path /* NULL: no file */, const char *overlap_tsv_path /* NULL: no file */, int32_t device, int threads, int32_t min_mapq,
                                           int32_t min_baseq, uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_fragerr_run *out,
                                           gce_mask_run *mask, char err[256]);
/* The error profile by consensus support: residual error against the reference per (segment, forward reads, reverse reads), counted on ONE
 * device (addition under ABI v3; gencore_amd/csrc/gce_errsup.hpp).  Replaces: nothing in the reference's source -- it reads
 * back the FR:C and RR:C fields the reference writes on every consensus record (Pair::writeSscsDcsTagBam), which a user otherwise tabulates
 * with a host script to choose -s and duplex-only: one run at -s 1, then this table.  One streaming pass over bam_path in any record order.
 * Eligible records: gce_bam_error_profile's eight tests in its order, then n_bad_aux: the optional fields, from the end of QUAL to the end of
 * the block, do not tile it (fewer than three bytes left, an unknown type or B subtype, a Z / H without its NUL, a value that passes the
 * block's end); such a record is skipped, not refused.  Support: f from the first optional field whose tag is tags[0..1], r from the first
 * whose tag is tags[2..3] (tags NULL: "FRRR"; "aDbD" reads fgbio's duplex depths).  A field of type c C s S i I has the value v its type's
 * sign gives; the bucket is v for 1 <= v <= 31 and 32 for every other v (0 among them: the reference writes the low byte of the count, so 0
 * stands for a multiple of 256 reads); no such field, or a first field of that tag with another type: bucket 0, absent.
 * counts[((segment * 33 + f) * 33 + r) * 24 + class]: classes 0..20 and the walk, the BED and the mask exactly as gce_bam_error_profile and
 * gce_bam_error_profile_masked have them, 21 MASKED (zero without mask_path), 22 RECORDS (one per eligible record; with a BED one per eligible
 * record whose reference span, widened by one position at both ends, touches a region), 23 zero.  mask_path (NULL: no mask; else *mask is
 * filled as gce_bam_error_profile_masked fills it and must not be NULL).  tsv_path (NULL: no file): a header line that begins with `#`, then
 * one line per (segment, forward, reverse) with a counter that is not zero, in ascending order: segment, forward, reverse (`.` absent, 1..31,
 * `32+`), records, bases (classes 0..15), mismatches (the off-diagonal ones), the sixteen A>A .. T>T, READ_N REF_OTHER LOWQ INS DEL, and
 * MASKED with a mask; integers, no rates; written to a temporary name and renamed.  n_with_forward / n_with_reverse: RECORDS summed over
 * f != 0 / r != 0.  options: GCE_ERRSUP_DIRECT makes every add a 64-bit global atomic instead of collecting a record's adds on chip: the same
 * counters, the A/B partner of the default.  Device memory: the reference bases, 627 264 bytes of counters, the mask's bit per base, the
 * interval table, one window and 4 bytes per window record, within device_budget_bytes (0: no limit), else GCE_ERR_OOM with that footprint.
 * The refusals are gce_bam_error_profile's, and tags that are not four characters.  Not here: the once-per-fragment rule of
 * gce_bam_error_profile_fragments, a cycle dimension, read groups, SAM text, several devices.  counts is malloc'ed: gce_errsup_free. */
#define GCE_ERRSUP_DIRECT 1u
#define GCE_ERRSUP_BUCKETS 33
typedef struct gce_errsup_run {
    int64_t n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar, n_no_ref, n_too_long, n_bad_aux;   /* n_eligible + the nine skips = n_records */
    int64_t n_with_forward, n_with_reverse;
    int64_t n_bases, n_mismatches, n_intervals /* -1: no BED */, peak_device_bytes;
    double  read_s, inflate_index_s, errprof_s, write_s, total_s;   /* errprof_s: the scan and k_sup_count; write_s: the table */
    uint64_t *counts;               /* [3 segments][33 forward][33 reverse][24 classes] */
} gce_errsup_run;
int gce_bam_error_profile_support(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *mask_path /* NULL: no mask */,
                                  const char *tsv_path /* NULL: no file */, const char *tags /* NULL: "FRRR" */, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq,
                                  uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errsup_run *out,
                                  gce_mask_run *mask /* NULL without mask_path */, char err[256]);
void gce_errsup_free(gce_errsup_run *out);
/* The error profile by reported base quality: of the bases a file reports at quality q, how many differ from the reference, per (segment,
 * quality), counted on ONE device (addition under ABI v3; gencore_amd/csrc/gce_errqual.hpp).  Replaces: nothing in the
 * reference's source -- it stands in for GATK BaseRecalibrator's table by reported quality, Picard QualityScoreDistribution read beside its
 * artifact metrics, or `fgbio ErrorRateByReadPosition` split by quality, which a user runs on the input and on the consensus output: the
 * consensus step writes qualities of its own, from the voters' scores and the reference's thresholds, and a caller that weights evidence by
 * QUAL trusts them.  One streaming pass over bam_path in any record order.  Eligible records, segment, classes 0..20, the walk, the BED and
 * the mask are exactly gce_bam_error_profile's and gce_bam_error_profile_masked's; the cycle is replaced by the quality bucket of the event:
 * an M / = / X column's own QUAL byte (a column below min_baseq adds LOWQ in its own quality's row), an inserted base's own byte, a
 * deletion's byte of the query base in front of it (the first, when there is none); QUAL is read in the stored, reference orientation.
 * The bucket of a byte b is b for b <= 93 and 94 for every other byte; every event of a record without qualities (QUAL[0] == 0xFF) has
 * bucket 95.  counts[((segment * 96 + bucket) * 24) + class]: 21 MASKED (zero without mask_path), 22 and 23 zero.  For every (segment,
 * class) the sum over the buckets equals gce_bam_error_profile's sum over the cycles on the same file and arguments.  mask_path (NULL: no
 * mask; else *mask is filled as gce_bam_error_profile_masked fills it and must not be NULL).  tsv_path (NULL: no file): a header line that
 * begins with `#`, then one line per (segment, quality) with a counter that is not zero, in ascending order: segment, quality (the number,
 * `94+`, or `.` for bucket 95), bases (classes 0..15), mismatches (the off-diagonal ones), the sixteen A>A .. T>T, READ_N REF_OTHER LOWQ INS
 * DEL, and MASKED with a mask; integers, no rates; written to a temporary name and renamed.  options: GCE_ERRQUAL_DIRECT makes every add a
 * 64-bit global atomic instead of meeting in the block's table on chip: the same counters, the A/B partner of the default.  Device memory:
 * the reference bases, 55 296 bytes of counters, the mask's bit per base, the interval table, one window and 4 bytes per window record,
 * within device_budget_bytes (0: no limit), else GCE_ERR_OOM with that footprint.  The refusals are gce_bam_error_profile's.  Not here: the
 * once-per-fragment rule of gce_bam_error_profile_fragments, a cycle or support dimension beside quality, the overlap table by quality, read
 * groups, SAM text, several devices.  counts is malloc'ed: gce_errqual_free. */
#define GCE_ERRQUAL_DIRECT 1u
#define GCE_ERRQUAL_BUCKETS 96
typedef struct gce_errqual_run {
    int64_t n_records, n_eligible, n_unplaced, n_flagged, n_low_mapq, n_no_cigar, n_no_seq, n_bad_cigar, n_no_ref, n_too_long;   /* n_eligible + the eight skips = n_records */
    int64_t n_bases, n_mismatches, n_intervals /* -1: no BED */, peak_device_bytes;
    double  read_s, inflate_index_s, errprof_s, write_s, total_s;   /* errprof_s: the scan and k_qual_count; write_s: the table */
    uint64_t *counts;               /* [3 segments][96 quality buckets][24 classes] */
} gce_errqual_run;
int gce_bam_error_profile_quality(const char *bam_path, const char *fasta_path, const char *bed_path /* NULL: no BED */, const char *mask_path /* NULL: no mask */,
                                  const char *tsv_path /* NULL: no file */, int32_t device, int threads, int32_t min_mapq, int32_t min_baseq,
                                  uint32_t exclude_flags, uint32_t options, uint64_t window_bytes, size_t device_budget_bytes, gce_errqual_run *out,
                                  gce_mask_run *mask /* NULL without mask_path */, char err[256]);
void gce_errqual_free(gce_errqual_run *out);
/* One window of SAM text through the GPU's line parser (addition under ABI v3; gencore_amd/csrc/gce_samdev.hpp).
 * Replaces: htslib's sam_read1 / sam_parse1 under the reference when its input is SAM text (src/gencore.cpp:164,205), which this library had
 * on host threads only (gce_sam_to_bam, gce_run_bam's SAM input).  text[0, n): alignment lines only (no `@` lines), whole lines, n < 2^32 - 256;
 * a last line may lack its line feed, a '\r' in front of a line feed is dropped, empty lines and lines of one '\r' are no records.
 * ref_name[0, n_ref): the contigs in the header's order.  out receives the BAM records (block_size first) of the lines, in line order and back
 * to back: the bytes gce_sam_to_bam writes for them.  *n_records: the lines that became records; *n_host_lines: those of them that hold an `f`,
 * `d` or `B:f` value, which the host re-parsed for strtof / strtod's rounding -- no other line is parsed on the host.  GCE_ERR_INVALID with the
 * host parser's message for a malformed line: *bad_line is the first one, counting from 0 over the lines that are records (-1 otherwise) and
 * nothing is written.  GCE_ERR_OOM when out_cap is too small: *out_bytes is the size needed. */
int gce_sam_parse(int32_t device, const char *text, size_t n, int32_t n_ref, const char *const *ref_name, void *out, size_t out_cap,
                  size_t *out_bytes, int64_t *n_records, int64_t *n_host_lines, int64_t *bad_line, char err[256]);
/* SAM text in any order into the coordinate-sorted BAM on ONE device, file to file (addition under ABI v3).
 * Replaces: gce_sam_to_bam followed by gce_bam_sort -- the `samtools sort` of an aligner's SAM output that the reference's README asks for --
 * and writes the same file, byte for byte, for every level, without the intermediate BAM: the text is read in windows of window_bytes (0 = 64 MB;
 * a window grows to hold one line, "SAM line longer than 256 MB" beyond that; values above 1 GB are taken as 1 GB) cut at their last line feed,
 * the `@` lines give the header as gce_sam_to_bam makes it (then rule H), the GPU turns the alignment lines into records behind the resident ones
 * (gce_sam_parse's kernels) and sorts as gce_bam_sort does (rules S / R / F, temporary file and rename, budget checks).  Host buffers do not
 * grow with the file.  In-core only: GCE_ERR_OOM before any output, with a message that states the footprint and names the way out
 * (gce_sam_to_bam, then gce_bam_sort_passes).  A malformed line: the host parser's message followed by " (line N)", N counting from 1 over the
 * file, header lines included.  A file that starts with the gzip magic: "gce_sam_sort reads SAM text, not BAM".  A failed call leaves neither an
 * output nor a temporary file.  *out as gce_bam_sort fills it; inflate_index_s: the parse kernels and the host's patch of the lines counted in
 * *n_host_lines (gce_sam_parse) -- not the copy of the text to the device, the growth of the resident buffers or the keys, which total_s holds. */
int gce_sam_sort(const char *in_path, const char *out_path, int32_t device, int threads, int level, uint64_t window_bytes,
                 size_t device_budget_bytes, gce_sort_run *out, int64_t *n_host_lines, char err[256]);
/* Whole BAM records through the GPU's line writer (addition under ABI v3; gencore_amd/csrc/gce_samfmt.hpp): the mirror of
 * gce_sam_parse.  Replaces: htslib's sam_write1 / sam_format1 under the reference when its output name ends in "sam" (sam_open(out, "w"),
 * src/gencore.cpp:170-173,104), which this library had on host threads only (gce_bam_to_sam, gce_run_bam's SAM output).  records[0, n): whole
 * BAM records, each with block_size first, back to back, in host memory.  ref_name[0, n_ref): the contigs in the header's order.  out receives
 * their lines (line feed included) in record order: the bytes gce_bam_to_sam writes for them.  *n_records: the records; *n_host_records: those
 * of them that hold an `f`, `d` or `B:f` value, which the host printed for %g -- no other record is formatted on the host.  GCE_ERR_INVALID
 * with the message "bad record in the output stream" for a record the host writer refuses (a block_size below 32, a record that runs past n,
 * fields that overrun block_size, an optional field that is cut or of an unknown type): *bad_record is the first one, counting from 0 (-1
 * otherwise) and nothing is written.  GCE_ERR_OOM when out_cap is too small: *out_bytes is the size needed.  Arguments are checked before
 * any device is touched. */
int gce_sam_format(int32_t device, const void *records, size_t n, int32_t n_ref, const char *const *ref_name, void *out, size_t out_cap,
                   size_t *out_bytes, int64_t *n_records, int64_t *n_host_records, int64_t *bad_record, char err[256]);
/* The output record stream (gce_raw_build_output, or gce_raw_merge_outputs on engs[0]) as SAM text made BY THE GPU, in HBM (addition under ABI
 * v3) -- replaces sam_write1's text under sam_open(out, "w") (src/gencore.cpp:170-173,104 via htslib): gce_sam_format's kernels over the
 * resident stream, the record starts taken from what the build / merge left behind, or from a walk of the block sizes when they are not
 * there.  *text_bytes = the size of the alignment lines; gce_raw_read_text_async copies a piece of them out (ticket -> gce_submit_wait).
 * The caller writes the header text in front: what gce_run_bam does for an output name that ends in "sam" at `level == -2` or `-3`. */
int gce_raw_format_output(gce_engine *e, int32_t n_ref, const char *const *ref_name, uint64_t *text_bytes);
int gce_raw_read_text_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket);
/* The GPU line writer's counters (addition under ABI v3; for tests and diagnostics, as gce_get_index_counters), process-wide since the process
 * started -- they tell sam_write1's text made by the GPU from the host's (src/gencore.cpp:104): out[0] records formatted on the device,
 * out[1] records the host formatted for it, out[2] formatter runs (one per gce_sam_format / gce_raw_format_output call that had records),
 * out[3] text bytes produced. */
int gce_get_sam_format_counters(int64_t out[4]);
/* Live and peak device bytes of the engine allocations of the whole PROCESS (every engine, every thread); reset_peak != 0 restarts the peak at
 * the live count.  gce_run_bam_passes resets it on entry: its run->peak_device_bytes covers other engines working in the same process as well. */
int gce_device_bytes(int64_t *live, int64_t *peak, int32_t reset_peak);

/* The reference's reports, on the host (gencore_amd/csrc/gce_report.hpp; additions under ABI v3).
 * Replaces: JsonReporter::report (src/jsonreporter.cpp:11-44) with Stats::reportJSON (src/stats.cpp:153-193) and Bed::reportJSON
 * (src/bed.cpp:81-100), called by Gencore::report (src/gencore.cpp:39-44,292): the same bytes from the two Stats blocks and a gce_depth_run
 * (gce_run_bam_depth).  target_name: depth->n_targets contig names (gce_bam_read_header); region_name: depth->n_regions names in the order of
 * depth->region_* (gce_bed_load), NULL = empty names; has_bed: a BED file was given (Options::hasBedFile) -- the "coverage_bed" block is
 * written, regions with tid -1 left out; command: the command line as the reference joins it (src/main.cpp:101-104). */
int gce_report_json(const char *path, const gce_stats *pre, const gce_stats *post, const gce_depth_run *depth, const char *const *target_name,
                    const char *const *region_name, int32_t has_bed, int32_t coverage_step, const char *command, char err[256]);
/* Replaces: Stats::print (src/stats.cpp:195-215) for one block (is_post: Gencore's mPostStats) -- the text into buf (NUL-terminated);
 * *len = its length without the NUL.  GCE_ERR_INVALID (with *len set) if cap < *len + 1. */
int gce_report_summary(const gce_stats *stats, int32_t is_post, char *buf, size_t cap, size_t *len);
/* Replaces: sam_hdr_read's contig table (src/gencore.cpp:180 via htslib) for a BAM or SAM file: contig names and lengths in header order.
 * BAM: only the BGZF members the header spans are inflated; SAM text: the @SQ lines of the '@' lines in front of the first alignment.
 * Arrays are malloc'ed; free them with gce_bam_header_free. */
int gce_bam_read_header(const char *path, int32_t *n_targets, char ***target_name, uint32_t **target_len, char err[256]);
void gce_bam_header_free(int32_t n_targets, char **target_name, uint32_t *target_len);

#ifdef __cplusplus
}
#endif
#endif /* GENCORE_AMD_H */
