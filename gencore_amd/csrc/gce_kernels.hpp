// gce_kernels.hpp — HIP kernels of the MI355X consensus engine (gfx950, wave64): what they share (Work, OutRec, the uinfo word, the wave
// helpers) and, included at the end in the order of the pipeline, the stages that have no header of their own elsewhere.
//
// Pipeline (one gce_process call, everything resident in HBM; engine.hip launches them in this order, in the stages of its Step:
// form_clusters, describe, pair_clusters, consensus, output_table):
//   k_cluster        THE CLUSTERING SCAN (gce_cluster.hpp): class, key (tid,left,right), block-level leaders -> (leader, rank) per read
//   k_blk_scan, k_events   ticks of the scan blocks; the reads on which the reference's periodic flush fires (gencore.cpp:319-322)
//   k_leaders        one lane per leader: instance from the flush events, bucket table -> cluster of every leader run
//   k_num_* k_scatter  cluster list (one claiming leader per cluster) + CSR fill: members[] per cluster
//   k_describe       per read: the 32-byte ReadDesc, UMI slice (and whether any holds a '_'), pre-Stats
//   k_pairing_sub<16|32> (gce_pair2.hpp), k_pairing_fast, k_pairing_deep (gce_deep.hpp), k_pairing_slow (gce_pairing.hpp)
//                    per cluster: qname order, mate pairing (cluster.cpp:260-273), greedy UMI grouping (cluster.cpp:55-100)
//   k_group_fill (gce_groups.hpp), k_vote_batches (gce_vote.hpp)   compact (cluster, group) list, batches of groups
//   k_vote (gce_vote.hpp)   per batch of groups: Pair::computeScore (pair.cpp:88-172) + template pick (group.cpp:136-318) + column
//                    vote (group.cpp:320-579), both sides; groups outside its scope go on through
//   k_score2, k_consensus_fast (gce_consensus.hpp), k_deep_prepare + k_vote_deep (gce_deep.hpp), k_consensus_slow (gce_consensus.hpp)
//   k_group_tail (gce_finish.hpp, as are the next two lines)   qname reconciliation; filter / FR tag and the Stats events (stats.cpp:123-139) of every group that is final there: all of them
//                    unless some UMI of the stream holds a '_' (k_describe: StreamInfo::umi_us), else those of clusters that cannot form a duplex
//   k_finish_screen, k_finish   only when a UMI holds a '_': duplex merge / filter / FR,RR tags (cluster.cpp:116-188, pair.cpp:43-68)
//   k_stats          only then: Stats events of the duplex stage's clusters
//   k_out_* (gce_output.hpp)   emitted records in bamComp order as one compact table, Stats::addRead of the emitted records
//   k_depth (gce_depth.hpp)   depth / BED statistics on request
#pragma once
#include "gce_device.hpp"

#define CHUNK 256            // reads per prescan/cluster block
#define WAVES_PER_BLOCK 4

// what Gencore::outputPair hands on for one emitted record (written once, where the record is emitted)
struct __attribute__((aligned(16))) OutRec { uint32_t qname_src, mate; int16_t nm_new, fr, rr; uint16_t pad; };
static_assert(sizeof(OutRec) == 16, "OutRec must stay 16 bytes");

struct Work {
    // per read
    uint64_t *uinfo;                     // per clustered read: where its UMI lies, its length, its name's length -- ONE word (uinfo_pack, below)
    ReadDescP *rdesc;
    uint32_t *spatch;                    // per read: overlap score patch (start | len << 16), GCE_PATCH_CONST, or 0
    uint32_t *slot;                      // per clustered read: leader of its scan block | rank in the leader's run << 16 (gce_cluster.hpp)
    int8_t *score;                       // parallel to qual
    // outputs per read: out_flag for every read (0 = not emitted, 1 = outputPair, 2 = pass-through); orec only where out_flag == 1
    uint8_t *out_flag; OutRec *orec;
    uint32_t *nmx;                       // per read: NM value << 1 | NM present (k_describe)
    uint32_t *out_index;                 // emitted reads, ascending
    // scan blocks (gce_cluster.hpp): leaders of every block, what k_leaders made of them, where their runs start in members[]
    struct LeadRec *lrec; struct LeadOut *lout;
    struct BlkHdr *bhdr; uint32_t *blk_base; int64_t n_sblk;   // per scan block: leaders + clustered reads; clustered reads in front of the block
    // events
    int32_t *ev_tid, *ev_pos; uint32_t *ev_read; int max_events;
    // hash table
    struct TabEntry *tab; uint32_t *toff; uint64_t tsize; double tinv;   // tsize buckets (any size, not a power of two); toff is written sparsely
    // clusters
    uint32_t *cl_ikey, *cl_start, *cl_n, *cl_npairs, *cl_ngroups, *cl_gbase, *cl_nresult; uint8_t *cl_hasumi;
    uint8_t *cl_tier;                    // which pairing tier paired the cluster (TIER_*, gce_device.hpp): one byte store next to cl_npairs, read by gce_get_pairing_tiers only
    // cluster-local arrays (indexed by cl_start + k)
    uint32_t *members, *sorted, *pl, *pr, *pu, *pg, *gpl, *gpr, *grp_begin, *grp_n;
    uint64_t *k64;                       // generic pairing scratch: 3 words per read (name window / UMI words)
    // groups (compact)
    uint32_t *gl_cluster, *g_begin, *g_np;   // per compact group: owning cluster, first pair slot, pair count
    uint64_t *gw; uint4 *vlive; uint32_t *vb_start;   // k_vote batching: per group its weight | live << 32 (0: d_group_skipped); the LIVE groups as {group, first pair slot, pairs,
                                         // weight prefix}, one 16-byte load in k_vote's P0; first live-list entry of every batch
    uint32_t *slow_list;                 // (group*2 + side) entries deferred to the generic consensus kernel
    uint8_t *pf_flag; uint32_t *pf_list;      // clusters the half-wave pairing kernel hands to the full-wave one (same scheme)
    uint8_t *pq_flag; uint32_t *pq_list;      // ... and the quarter-wave kernel to the half-wave one
    uint32_t *left_list;                 // clusters left for k_pairing_deep<device memory> / the generic pairing kernels (count: si->n_slow_pair2).  A list of its own since round 5:
                                         // it is appended to while the half-wave kernel still reads pq_list (the pairing tiers run side by side on two streams)
    uint8_t *p16_flag; uint32_t *p16_list;    // clusters of <= 16 reads, compacted: the quarter-wave kernel runs on full waves (k_pair_classes)
    void *deep_list;                       // DeepRec[] (gce_deep.hpp)
    uint8_t *gen_flag; uint32_t *gen_list;   // (group*2 + side) entries k_vote hands to the per-side kernels: appended to gen_list by the group's lane (one 64-bit atomic per group
                                          // for this list and k_score2's: si->hand_on); gen_flag: 1 = handed on, 2 = finished by k_vote_deep
    uint32_t *score_list;                 // pair slots of the groups whose sides were handed on (k_score2 scores only those; count: low half of si->hand_on)
    uint32_t *rp_left, *rp_right, *rp_merge, *rp_rmerge; const char **rp_umi; uint16_t *rp_umilen; uint8_t *rp_state; int32_t *rp_supp;
    int32_t *rp_nm;                       // [2 x groups] NM byte patched into the side's template (group.cpp:570), -1 = untouched
    uint32_t *rp_qsl, *rp_qsr;            // per group: copyQName source of the left / right result record
    // generic scan scratch
    uint64_t *scan_part;
    StreamInfo *si;
};

// The UMI of a clustered read (BamUtil::getUMI, bamutil.cpp:23-112: a slice of its name, or its MI:Z tag) and the length of its name in ONE 64-bit word per read:
//   bits 0..39 offset of the UMI in the blob it lies in | bit 40: that blob is the MI blob (else the names) | bits 41..48 core.l_qname | bits 49..63 UMI length
// Rounds 1-4 kept a pointer, a 16-bit length and a byte in three arrays: three scattered 64-byte sectors per read wherever a read's UMI was looked at (the
// pairing kernels, k_group_tail) and one more (the core record) for the name's length.  UMIs beyond 32767 bytes are refused by k_describe.
#define UINFO_MAXLEN 32767
__device__ __forceinline__ uint64_t uinfo_pack(uint64_t off, bool from_mi, int l_qname, int len) {
    return (off & 0xFFFFFFFFFFull) | ((uint64_t)(from_mi ? 1 : 0) << 40) | ((uint64_t)(l_qname & 0xFF) << 41) | ((uint64_t)(len & 0x7FFF) << 49);
}
__device__ __forceinline__ const char *uinfo_ptr(const DevBatch &b, uint64_t v) { return (((v >> 40) & 1ull) ? b.mi : b.qname) + (v & 0xFFFFFFFFFFull); }
__device__ __forceinline__ int uinfo_len(uint64_t v) { return (int)(v >> 49); }
__device__ __forceinline__ bool uinfo_hm(uint64_t v) { return ((v >> 40) & 1ull) != 0; }
__device__ __forceinline__ int uinfo_lqname_pad(uint64_t v) { return ((int)((v >> 41) & 0xFFu) + 3) & ~3; }            // (= d_lqname_pad of the read's core record)
__device__ __forceinline__ const char *d_umi_ptr(const DevBatch &b, const Work &w, uint64_t i) { return uinfo_ptr(b, w.uinfo[i]); }
__device__ __forceinline__ int d_umi_len(const Work &w, uint64_t i) { return uinfo_len(w.uinfo[i]); }
__device__ __forceinline__ bool d_umi_hm(const Work &w, uint64_t i) { return uinfo_hm(w.uinfo[i]); }
__device__ __forceinline__ int d_lqname(const Work &w, uint64_t i) { return (int)((w.uinfo[i] >> 41) & 0xFFu); }            // core.l_qname of a clustered read

enum : uint8_t { RP_PENDING = 0, RP_OUT_SSCS = 1, RP_OUT_DCS = 2, RP_DROPPED = 3, RP_CONSUMED = 4 };
// rp_nm: >= 0 the new NM byte, -1 untouched, NM_DEFER + mismatchInc (k_vote): the delta of a template whose NM tag has not been looked at yet
#define NM_DEFER (-0x40000000)
#define NM_IS_DEFERRED(v) ((v) < -0x20000000)

#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

__device__ __forceinline__ int rl32(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint64_t rl64(uint64_t v, int l) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ long long wave_sum64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

#include "gce_cluster.hpp"
#include "gce_pairing.hpp"
#include "gce_groups.hpp"
#include "gce_consensus.hpp"
#include "gce_finish.hpp"
