// gce_varmask.hpp — the variant mask of the error profile on the device (gce_errprof_set_mask, gce_fragerr_set_mask, gce_errsup_set_mask).
//
// After consensus the residual error rate is 1e-5 to 1e-6 per base and a germline SNP comes once in a thousand bases, so without a mask the
// off-diagonal counters of gce_bam_error_profile are the sample's genotype.  The mask is one bit per byte of calmd::Ref's blob: the bit of
// (tid, x) is ref.tab[2 tid] + x, bit i in bit i % 8 of byte i / 8 (bit i % 32 of the little-endian 32-bit word i / 32, which is how the fill
// kernel writes it and errprof::mask_at, byte by byte, reads it).  Contigs are packed without padding (calmd_ref_layout), so the last base of
// one contig and the first of the next can share a word.  ref_bytes / 8 bytes rounded up to whole words, plus 64 of slack, within the
// session's budget; nothing on the host is proportional to the genome.  The host side (bamio_varmask.hpp's gce_mask_load, rule K) gives
// sorted, merged intervals; the entry points take them in any order and any number of times, since OR is idempotent.
//   k_mask_fill   256 threads per block, one interval per thread, VM_BLOCK_IVS intervals per block.  Most intervals are one base (a SNP): one
//                 atomicOr.  An interval inside one word: one atomicOr; a longer one: an atomicOr for each ragged end and plain stores of
//                 0xFFFFFFFF for the whole words between, by the thread itself up to VM_OWN_WORDS of them, else by all the block's lanes once
//                 every thread has done its own (a BED of repeats has intervals of megabytes).  A whole word is stored only where every bit of
//                 it is to be set, so a store that meets another interval's atomicOr on the same word leaves all ones in either order.
//                 The whole words of one interval are stored by the one block that holds it, so an interval of many megabases is filled by
//                 256 lanes, not by the device: correct, and slow for a BED of few, very long regions (a megabase is 32 768 words, 128
//                 stores a lane).  Cutting such an interval into pieces on the host, one per block, is the way to spread it; not done.
#pragma once
#include <cstdint>

#define VM_THREADS 256u
#define VM_BLOCK_IVS VM_THREADS                                                       // intervals per block of k_mask_fill: one per thread
#define VM_OWN_WORDS 8u                                                               // whole words a thread stores itself
#define VM_CHUNK (1u << 16)                                                           // intervals per launch: 768 KiB of staging
static_assert(VM_BLOCK_IVS == VM_THREADS && VM_CHUNK % VM_BLOCK_IVS == 0, "k_mask_fill's layout");

// the bitmap's bytes for a blob of ref_bytes bases
static inline uint64_t varmask_bytes(uint64_t ref_bytes) { return (ref_bytes + 31) / 32 * 4 + 64; }
// what needs() adds for it: short, since the message has to fit the 255 characters of the entry points' err together with "N more for the variant mask", which gives its bytes
static inline std::string varmask_needs(uint64_t mask_bytes) { return mask_bytes ? " + the mask" : std::string(); }

namespace {

// tab: calmd::Ref's (offset, length) pairs; bits: the bitmap, n_bits of it (the blob's bytes).  An interval of a contig the FASTA lacks, or
// outside [0, n_ref), sets nothing; every other one is clamped to [0, the contig's FASTA length), so no bit at or behind n_bits is written.
__global__ __launch_bounds__(VM_THREADS) void k_mask_fill(const int32_t *tid, const int32_t *start, const int32_t *end, uint32_t n, const int64_t *tab, int32_t n_ref, uint32_t *bits,
                                                          uint64_t n_bits) {
    __shared__ uint32_t s_n;
    __shared__ uint64_t s_a[VM_BLOCK_IVS], s_z[VM_BLOCK_IVS];                         // the whole words [a, z) left to the block
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint32_t j = blockIdx.x * VM_BLOCK_IVS + threadIdx.x;
    if (j < n) {
        const int32_t t = tid[j];
        if (t >= 0 && t < n_ref) {
            const int64_t base = tab[2 * t], len = tab[2 * t + 1];
            const int64_t a = start[j] > 0 ? (int64_t)start[j] : 0, z = (int64_t)end[j] < len ? (int64_t)end[j] : len;
            if (a < z && (uint64_t)(base + z) <= n_bits) {
                const uint64_t b0 = (uint64_t)(base + a), b1 = (uint64_t)(base + z) - 1, w0 = b0 >> 5, w1 = b1 >> 5;      // bits [b0, b1]
                const uint32_t head = ~0u << (b0 & 31u), tail = ~0u >> (31u - (uint32_t)(b1 & 31u));
                if (w0 == w1) atomicOr(bits + w0, head & tail);
                else {
                    atomicOr(bits + w0, head); atomicOr(bits + w1, tail);
                    if (w1 - w0 - 1 <= VM_OWN_WORDS) for (uint64_t w = w0 + 1; w < w1; w++) bits[w] = ~0u;
                    else { const uint32_t k = atomicAdd(&s_n, 1u); s_a[k] = w0 + 1; s_z[k] = w1; }
                }
            }
        }
    }
    __syncthreads();
    const uint32_t m = s_n;
    for (uint32_t k = 0; k < m; k++) for (uint64_t w = s_a[k] + threadIdx.x; w < s_z[k]; w += VM_THREADS) bits[w] = ~0u;
}

}  // namespace

// gce_errprof_set_mask / gce_fragerr_set_mask / gce_errsup_set_mask over the passes' ErrSession (gce_errprof.hpp, which includes this file
// behind it): the first call makes and zeroes the bitmap, every call ORs its intervals in, VM_CHUNK of them per launch
static int ep_set_mask(ErrSession *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end) {
    if (!p || !p->ref_set || p->n || n < 0 || (n > 0 && (!tid || !start || !end))) return GCE_ERR_INVALID;
    (void)hipSetDevice(p->device);
    hipStream_t s = p->s;
    if (!p->mask_bytes) {
        const uint64_t bytes = varmask_bytes(p->ref_bytes), want = DevBuf::padded(bytes);
        p->mask_bytes = bytes;                                                        // (needs() states it in the message)
        int rc = GCE_OK;
        if (!p->room(want)) rc = p->oom("the variant mask", want);
        else {
            const hipError_t e = p->mask.ensure(bytes);
            if (e == hipErrorOutOfMemory) rc = p->oom("the variant mask", want);
            else if (e != hipSuccess) rc = p->fail(GCE_ERR_HIP, std::string("the variant mask: ") + hipGetErrorString(e));
        }
        if (rc != GCE_OK) { p->mask_bytes = 0; return rc; }
        RDCHK(hipMemsetAsync(p->mask.p, 0, bytes, s));
    }
    if (n > 0) {
        const uint64_t cap = (uint64_t)std::min<int64_t>(n, VM_CHUNK), want = DevBuf::padded(cap * 12);
        if (!p->room(want)) return p->oom("the variant mask", want);
        ScopedBuf stage;
        RDCHK(stage.ensure(cap * 12));
        int32_t *dt = stage.as<int32_t>(), *da = dt + cap, *dz = da + cap;
        for (int64_t k = 0; k < n; k += (int64_t)cap) {
            const uint32_t m = (uint32_t)std::min<int64_t>(n - k, (int64_t)cap);
            RDCHK(hipMemcpyAsync(dt, tid + k, (size_t)m * 4, hipMemcpyHostToDevice, s)); RDCHK(hipMemcpyAsync(da, start + k, (size_t)m * 4, hipMemcpyHostToDevice, s));
            RDCHK(hipMemcpyAsync(dz, end + k, (size_t)m * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_mask_fill, dim3((m + VM_BLOCK_IVS - 1) / VM_BLOCK_IVS), dim3(VM_THREADS), 0, s, dt, da, dz, m, p->tab.as<int64_t>(), p->P.n_ref, p->mask.as<uint32_t>(),
                               p->ref_bytes);
            RDCHK(hipGetLastError()); RDCHK(hipStreamSynchronize(s));
        }
    }
    RDCHK(hipStreamSynchronize(s));
    return GCE_OK;
}
