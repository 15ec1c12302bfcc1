// gce_groups.hpp — the compact group list behind pairing: which groups are evaluated at all (d_group_skipped), their list and weights
// (k_group_fill: what k_vote_batches, gce_vote.hpp, scans into batches), and the apply pass of the scan of cl_ngroups -> cl_gbase
// (k_u32_apply; its reduce and partials passes are the table scan's, gce_cluster.hpp).
//
// Stage pair_clusters of engine.hip launches both behind the pairing tiers; k_group_tail (gce_finish.hpp) asks d_group_skipped again.
//
// A part of gce_kernels.hpp.
#pragma once

// A group whose result no setting of this run can write is not evaluated: ONE pair (mMergeReads = 1) under --supporting_reads > 1 or --duplex_only is deleted
// unwritten (cluster.cpp:157-181) unless a duplex partner adds its reads -- and its Stats entry is known before a base is read: supporting reads 1, PE iff the
// pair has both reads (group.cpp:73-77 for a mate-less pair; with one pair and --skip_low_complexity_cluster_threshold >= 1 consensusMergeBam returns that pair's
// read, group.cpp:196-285; with a threshold of 0 it may return NULL, group.cpp:142-175, and the group keeps the full path).  It cannot find a partner when its
// cluster forms no duplex at all: no UMI, --no_duplex, a single group (k_group_tail's rule).  A one-pair group of a cluster that does form duplexes keeps the
// full path even where its own UMI could not match (looking at the UMI here cost what it saved), and so do groups of 2 .. cluster_size_req - 1
// pairs: their PE flag needs the template choice.  k_group_fill leaves a skipped group out of k_vote's live list and k_group_tail takes its two
// reads from the pair slot: both ask THIS function.
__device__ __forceinline__ bool d_group_skipped(const DevParams &p, uint8_t cflags, uint32_t cl_groups, uint32_t np) {
    if (np != 1u || p.skip_low_complexity_thr < 1 || !(p.duplex_only || p.cluster_size_req > 1)) return false;
    return !(cflags & 1) || p.disable_duplex || cl_groups < 2u;
}

// the compact group list (one thread per cluster) and what k_vote_batches scans: weight | 1 << 32 of every live group, 0 for a skipped one
__global__ void k_group_fill(DevParams p, Work w, uint32_t n_clusters, uint32_t deep_weight, uint32_t min_weight) {
    uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters) return;
    uint32_t g0 = w.cl_gbase[c], ng = w.cl_ngroups[c];
    const uint32_t cs = w.cl_start[c];
    const uint8_t cflags = ng ? w.cl_hasumi[c] : (uint8_t)0;
    for (uint32_t g = 0; g < ng; g++) {
        const uint32_t np = w.grp_n[cs + g], begin = w.grp_begin[cs + g];
        w.gl_cluster[g0 + g] = c; w.g_begin[g0 + g] = begin; w.g_np[g0 + g] = np;
        // k_vote batches (gce_vote.hpp): a group weighs its pairs (at least VB_MINW: <= 16 groups per batch); a deep group is handed on by a batch of its own
        // (only a group of more than 32 pairs: P0's slot-flag loop is serial in its pairs.  A group that is "deep" by a small --skip_low_complexity
        //  threshold alone is handed on from a shared batch: with a batch of its own for every 2-pair group the batch count left the bound vb_start is sized by)
        const uint64_t wt = np > 32u ? (uint64_t)deep_weight : (uint64_t)(np < min_weight ? min_weight : np);
        w.gw[g0 + g] = d_group_skipped(p, cflags, ng, np) ? 0ull : (wt | (1ull << 32));
    }
}
// scan of cl_ngroups -> cl_gbase : same 3-phase scheme on the plain counts
__global__ __launch_bounds__(256) void k_u32_apply(const uint32_t *in, uint32_t *out, uint64_t n, const uint64_t *part) {
    __shared__ uint64_t s_w[4];
    __shared__ uint64_t s_carry;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = part[blockIdx.x];
    __syncthreads();
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    for (int k = 0; k < SCAN_TILE / 256; k++) {
        uint64_t h = base + k * 256 + threadIdx.x;
        uint64_t v = tab_elem(in, h, n), x = v;
        for (int o = 1; o < 64; o <<= 1) { uint64_t t = (uint64_t)__shfl_up((long long)x, o); if (lane >= o) x += t; }
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        uint64_t woff = 0;
        for (int q = 0; q < wv; q++) woff += s_w[q];
        uint64_t carry = s_carry;
        if (h < n) out[h] = (uint32_t)(carry + woff + x - v);
        __syncthreads();
        if (threadIdx.x == 255) s_carry = carry + woff + x;
        __syncthreads();
    }
}
