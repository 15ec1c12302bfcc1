// gce_bamdev.hpp — the GPU side of the BAM codec ("multi-threaded or GPU-assisted"): the host only inflates and deflates
// BGZF blocks; everything that touches RECORDS happens in HBM.
//   gce_raw_begin / gce_raw_push     the inflated BAM stream arrives window by window (host pinned buffer -> HBM, asynchronously, while the host
//                                    inflates the next window); the host keeps nothing of it
//   gce_raw_finish                   record index on the GPU (the chain of block_size fields, walked by one lane per 16 KB segment from a
//                                    guessed record start and joined where the guesses meet the chain -- the scheme of the host index in
//                                    bamio.cpp --), then the gce_batch of the stream WITHOUT copying names, bases or qualities: the blobs of
//                                    the struct-of-arrays ARE the raw stream (offsets point into it); only the 32-byte key records, the CIGAR
//                                    words (alignment) and NM / MI (aux walk) are extracted.  Replaces sam_read1's record parsing
//                                    (src/gencore.cpp:205-274 via htslib) for the whole file at once.
//   gce_raw_build_output             after gce_process: the emitted records as BAM records, assembled in HBM from the raw stream (the template's
//                                    record, mutated in place by the vote, with the name of its copyQName source, NM patched, FR / RR
//                                    appended: src/gencore.cpp:83-111 writeBam, src/pair.cpp:43-68) -- the host gets a byte stream that only
//                                    needs BGZF blocks around it
//   gce_raw_read_output[_async]      that stream, piece by piece, into host (pinned) memory
#pragma once

namespace {

// bytes of an aux value behind its type byte, or ~0 (bamio.cpp aux_size)
__device__ __forceinline__ uint64_t raw_aux_size(uint8_t type, const uint8_t *p, const uint8_t *end) {
    switch (type) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'd': return 8;
    case 'Z': case 'H': { const uint8_t *q = p; while (q < end && *q) q++; return q < end ? (uint64_t)(q - p) + 1 : ~0ull; }
    case 'B': {
        if (p + 5 > end) return ~0ull;
        const uint8_t t = p[0];
        const uint64_t es = (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : ~0ull;
        return es == ~0ull ? ~0ull : 5 + es * (uint64_t)rb32(p + 1);
    }
    default: return ~0ull;
    }
}
struct RawSoA {
    gce_core *core; uint64_t *qoff, *soff, *loff, *mioff; uint32_t *ncig, *nm_pos; int32_t *nm; uint8_t *nmt; unsigned int *have_mi;
    unsigned int *bad_rec; int32_t n_ref;      // first record whose fields do not fit its block_size (atomicMin; NONE32 = none)
};
// one thread per record: the 32-byte key record, the offsets of name / bases / qualities INSIDE the raw stream, NM (first match, value as
// bam_aux2i gives it) and MI:Z from the aux area (bamio.cpp scan_aux), the place of NM's value byte for the writer
__global__ __launch_bounds__(256) void k_raw_fill(const uint8_t *u, const uint64_t *rec_off, uint64_t n_rec, RawSoA o) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const uint64_t ro = rec_off[i];
    const uint8_t *r = u + ro + 4; const uint32_t bs = rb32(u + ro);
    union { gce_core c; uint32_t w[8]; uint4 q[2]; } t;
#pragma unroll
    for (int k = 0; k < 8; k++) t.w[k] = rb32(r + 4 * k);
    reinterpret_cast<uint4 *>(o.core + i)[0] = t.q[0]; reinterpret_cast<uint4 *>(o.core + i)[1] = t.q[1];
    const uint32_t lq = t.c.l_qname, nc = t.c.n_cigar; const int32_t ls = t.c.l_qseq;
    // The chain of block_size fields says where records start, not that their fields fit: the test gce_bam_open applies on the host
    // (bamio.cpp, "inconsistent record lengths") -- a name, l_seq >= 0, name + CIGAR + bases + qualities inside block_size, contig ids
    // inside the header's.  A record that fails it gets empty fields here (nothing downstream follows its lengths) and fails the stream.
    if (lq == 0 || ls < 0 || 32ull + lq + 4ull * nc + (uint64_t)(ls + 1) / 2 + (uint64_t)ls > bs || t.c.tid < -1 || t.c.tid >= o.n_ref || t.c.mtid < -1 || t.c.mtid >= o.n_ref) {
        atomicMin(o.bad_rec, (unsigned int)i);
        o.qoff[i] = ro + 4; o.soff[i] = ro + 4; o.loff[i] = ro + 4; o.ncig[i] = 0; o.nm[i] = 0; o.nmt[i] = 0; o.nm_pos[i] = 0; o.mioff[i] = ~0ull;
        return;
    }
    const uint64_t q0 = ro + 36, c0 = q0 + lq, s0 = c0 + 4ull * nc, l0 = s0 + (uint64_t)(ls + 1) / 2, a0 = l0 + (uint64_t)ls;
    o.qoff[i] = q0; o.soff[i] = s0; o.loff[i] = l0; o.ncig[i] = nc;
    uint8_t nmt = 0; int32_t nm = 0; uint32_t nm_pos = 0; uint64_t mi = ~0ull;
    const uint8_t *p = u + a0, *end = r + bs;
    while (p + 3 <= end) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2]; const uint8_t *v = p + 3;
        const uint64_t sz = raw_aux_size(ty, v, end);
        if (sz == ~0ull || v + sz > end) break;
        if (t0 == 'N' && t1 == 'M' && nmt == 0) {
            nmt = ty; nm_pos = (uint32_t)(v - (u + ro));
            switch (ty) {
            case 'c': nm = (int8_t)v[0]; break;            case 'C': nm = v[0]; break;
            case 's': nm = (int16_t)rb16(v); break;        case 'S': nm = (int32_t)rb16(v); break;
            case 'i': nm = (int32_t)rb32(v); break;        case 'I': nm = (int32_t)rb32(v); break;
            default: nm = 0; break;
            }
        } else if (t0 == 'M' && t1 == 'I' && ty == 'Z' && mi == ~0ull) mi = (uint64_t)(v - u);
        p = v + sz;
    }
    o.nm[i] = nm; o.nmt[i] = nmt; o.nm_pos[i] = nm_pos; o.mioff[i] = mi;
    if (mi != ~0ull && *(volatile unsigned int *)o.have_mi == 0u) atomicOr(o.have_mi, 1u);
}
__global__ __launch_bounds__(256) void k_raw_cigar(const uint8_t *u, const uint64_t *rec_off, uint64_t n_rec, const uint64_t *coff, uint32_t *cigar) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const uint8_t *r = u + rec_off[i] + 4;
    const uint32_t lq = r[8], nc = (uint32_t)(coff[i + 1] - coff[i]);           // (the count k_raw_fill accepted, not the record's own field)
    const uint8_t *c = r + 32 + lq;
    uint32_t *dst = cigar + coff[i];
    for (uint32_t k = 0; k < nc; k++) dst[k] = rb32(c + 4 * k);
}

// ---- output records
struct RawOut { const uint32_t *src, *qname_src; const int32_t *nm_new; const int16_t *fr, *rr; };
__global__ __launch_bounds__(256) void k_rec_size(const uint8_t *u, const uint64_t *rec_off, RawOut r, uint64_t n_out, uint64_t *size) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    const uint64_t so = rec_off[r.src[k]], qo = rec_off[r.qname_src[k]];
    const uint32_t bs = rb32(u + so), lq_old = u[so + 12], lq_new = u[qo + 12];
    size[k] = 4ull + bs - lq_old + lq_new + (r.fr[k] >= 0 ? 4 : 0) + (r.rr[k] >= 0 ? 4 : 0);
}
// 16 lanes per record: [block_size][core, l_qname of the name's source][that name][everything behind the name of the template's own record:
// CIGAR, bases and qualities as the vote left them, aux][FR][RR]; NM's value byte patched (type 'C' only, checked by the vote)
__global__ __launch_bounds__(256) void k_rec_build(const uint8_t *u, const uint64_t *rec_off, const uint32_t *nm_pos, RawOut r, uint64_t n_out, const uint64_t *roff, uint8_t *body) {
    const int sub = threadIdx.x & 15;
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; k < n_out; k += ((uint64_t)gridDim.x * blockDim.x) >> 4) {
        const uint32_t src = r.src[k];
        const uint64_t so = rec_off[src], qo = rec_off[r.qname_src[k]];
        const uint32_t bs = rb32(u + so), lq_old = u[so + 12], lq_new = u[qo + 12];
        const int fr = r.fr[k], rr = r.rr[k];
        const uint32_t tail = bs - 32 - lq_old;                                    // CIGAR .. aux
        const uint32_t nbs = 32 + lq_new + tail + (fr >= 0 ? 4 : 0) + (rr >= 0 ? 4 : 0);
        uint8_t *d = body + roff[k];
        if (sub < 9) {                                                             // block_size + the eight words of the core
            uint32_t w = sub == 0 ? nbs : rb32(u + so + 4 * sub);
            if (sub == 3) w = (w & ~0xFFu) | lq_new;                               // l_read_name is the low byte of the third core word
            *(rb_u32u *)(d + 4 * sub) = w;
        }
        for (uint32_t j = sub; j < lq_new; j += 16) d[36 + j] = u[qo + 36 + j];
        const uint8_t *ts = u + so + 36 + lq_old; uint8_t *td = d + 36 + lq_new;
        for (uint32_t j = 4 * sub; j < tail; j += 64) {                            // four bytes per lane and trip
            if (j + 4 <= tail) *(rb_u32u *)(td + j) = rb32(ts + j);
            else for (uint32_t q = j; q < tail; q++) td[q] = ts[q];
        }
        if (sub == 15) {
            uint8_t *e2 = td + tail;
            if (fr >= 0) { e2[0] = 'F'; e2[1] = 'R'; e2[2] = 'C'; e2[3] = (uint8_t)fr; e2 += 4; }
            if (rr >= 0) { e2[0] = 'R'; e2[1] = 'R'; e2[2] = 'C'; e2[3] = (uint8_t)rr; }
        }
    }
}
// (after k_rec_build: one more pass so that the NM patch cannot race with the copy of the same byte by another lane)
__global__ __launch_bounds__(256) void k_rec_nm(const uint8_t *u, const uint64_t *rec_off, const uint32_t *nm_pos, RawOut r, uint64_t n_out, const uint64_t *roff, uint8_t *body) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_out || r.nm_new[k] < 0) return;
    const uint32_t src = r.src[k], np = nm_pos[src];
    if (!np) return;
    const uint64_t so = rec_off[src], qo = rec_off[r.qname_src[k]];
    const uint32_t lq_old = u[so + 12], lq_new = u[qo + 12];
    body[roff[k] + np - lq_old + lq_new] = (uint8_t)r.nm_new[k];                   // dataNM[1] = newValNM (group.cpp:570)
}

// ---- the sharded file runner: one engine per shard, every engine holds the whole stream and takes its share of it
struct ShardSrc { const gce_core *core; const uint64_t *qoff, *coff, *soff, *loff, *mioff, *tick, *roff; const int32_t *nm; const uint8_t *nmt; const uint32_t *nmpos; };
struct ShardDst { gce_core *core; uint64_t *qoff, *coff, *soff, *loff, *mioff, *tick, *roff; int32_t *nm; uint8_t *nmt; uint32_t *nmpos; };
__global__ __launch_bounds__(256) void k_shard_flag(const int32_t *shard, int64_t n, int32_t rank, uint8_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = shard[i] == rank;
}
// thread per selected read: its key record and the per-read words of the batch, gathered (names, CIGAR words, bases and qualities stay where they are)
__global__ __launch_bounds__(256) void k_shard_gather(const uint32_t *sel, int64_t m, ShardSrc a, ShardDst d) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t k = sel[j];
    const uint4 *src = reinterpret_cast<const uint4 *>(a.core + k); uint4 *dst = reinterpret_cast<uint4 *>(d.core + j);
    dst[0] = src[0]; dst[1] = src[1];
    d.qoff[j] = a.qoff[k]; d.coff[j] = a.coff[k]; d.soff[j] = a.soff[k]; d.loff[j] = a.loff[k]; d.nm[j] = a.nm[k]; d.nmt[j] = a.nmt[k];
    if (a.mioff) d.mioff[j] = a.mioff[k];
    d.tick[j] = a.tick[k]; d.roff[j] = a.roff[k]; d.nmpos[j] = a.nmpos[k];
}
// what the merge of the shards' output tables compares: bamComp's fields (gencore.h:19-47) + the read's place in the WHOLE stream (quirk Q3) + the record's bytes
struct __attribute__((aligned(16))) MergeKey { int32_t tid, pos, mtid, mpos, isize; uint32_t gidx; uint32_t size, pad; };
__global__ __launch_bounds__(256) void k_merge_keys(const gce_core *core, const uint32_t *src, const uint32_t *sel, const uint64_t *rsize, uint64_t n_out, MergeKey *out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    const uint32_t r = src[k]; const gce_core c = core[r];
    MergeKey m; m.tid = c.tid; m.pos = c.pos; m.mtid = c.mtid; m.mpos = c.mpos; m.isize = c.isize; m.gidx = sel ? sel[r] : r; m.size = (uint32_t)rsize[k]; m.pad = 0;
    out[k] = m;
}
// 16 lanes per record: record k of the merged stream = bytes [from[k], from[k] + size[k]) of the staged shard streams
__global__ __launch_bounds__(256) void k_merge_copy(const uint8_t *stage, const uint64_t *from, const uint64_t *to, const uint32_t *size, uint64_t n, uint8_t *body) {
    const int sub = threadIdx.x & 15;
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; k < n; k += ((uint64_t)gridDim.x * blockDim.x) >> 4) {
        const uint8_t *s = stage + from[k]; uint8_t *d = body + to[k]; const uint32_t sz = size[k];
        for (uint32_t j = 4 * sub; j < sz; j += 64) {
            if (j + 4 <= sz) *(rb_u32u *)(d + j) = rb32(s + j);
            else for (uint32_t q = j; q < sz; q++) d[q] = s[q];
        }
    }
}
__global__ void k_add_i64(long long *acc, const long long *x, int n) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) acc[i] += x[i]; }

}  // namespace


extern "C" {

int gce_raw_begin(gce_engine *e, size_t capacity_hint) {
    if (!e) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    if (e->processed || e->host_mode || e->device_mode) gce_reset(e);
    if (!e->up_stream) HIPCHK(hipStreamCreate(&e->up_stream));
    HIPCHK(e->raw.ensure(capacity_hint + 256));
    {   // the per-record arrays, sized for the most records the stream can hold (a record with bases is > 96 bytes): allocated NOW, beside
        // the host's first inflate, instead of in gce_raw_finish on the critical path (hipMalloc of gigabytes takes tens of milliseconds)
        const size_t n1 = capacity_hint / 96 + 1024, nseg = capacity_hint / RAW_SEG + 16;
        HIPCHK(e->rw.guess.ensure(nseg * 8)); HIPCHK(e->rw.leave.ensure(nseg * 8)); HIPCHK(e->rw.cnt.ensure(nseg * 4 + 8)); HIPCHK(e->rw.base.ensure(nseg * 8 + 8)); HIPCHK(e->rw.misc.ensure(64));
        HIPCHK(e->rw.off.ensure((n1 + 1) * 8));
        HIPCHK(e->b_core.ensure(n1 * sizeof(gce_core) + 64)); HIPCHK(e->b_qoff.ensure(n1 * 8 + 64)); HIPCHK(e->b_coff.ensure((n1 + 1) * 8 + 64)); HIPCHK(e->b_soff.ensure(n1 * 8 + 64)); HIPCHK(e->b_loff.ensure(n1 * 8 + 64));
        HIPCHK(e->b_nm.ensure(n1 * 4 + 64)); HIPCHK(e->b_nmt.ensure(n1 + 64)); HIPCHK(e->b_mioff.ensure(n1 * 8 + 64)); HIPCHK(e->rw_ncig.ensure(n1 * 4 + 64)); HIPCHK(e->rw_nmpos.ensure(n1 * 4 + 64));
        HIPCHK(e->b_cigar.ensure(n1 * 8 + 64));
    }
    e->raw_n = 0; e->raw_mode = true; e->raw_records = 0; e->z_n = 0; e->z_members.clear();
    return GCE_OK;
}

// bytes of the inflated stream, in order.  Asynchronous: `host` (pinned memory makes it a real DMA) must stay untouched until gce_raw_wait(ticket).
int gce_raw_push(gce_engine *e, const void *host, size_t bytes, int32_t *ticket) {
    if (!e || !e->raw_mode || (!host && bytes)) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    // grow: the copies so far are in flight on the same stream, the move queues behind them (members waiting for the GPU inflate have places,
    // not bytes yet: they may lie past the old buffer)
    HIPCHK(dev_grow_keep(e->raw, e->raw_n + bytes + 256, std::min(e->raw_n, e->raw.cap), DevBuf::padded((e->raw_n + bytes) * 2 + 256), e->up_stream));
    if (bytes) HIPCHK(hipMemcpyAsync((char *)e->raw.p + e->raw_n, host, bytes, hipMemcpyHostToDevice, e->up_stream));
    e->raw_n += bytes;
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev, e->up_stream));
    e->up_events.push_back(ev);
    if (ticket) *ticket = (int32_t)e->up_events.size() - 1;
    for (gce_engine *m : e->mirrors) { const int rm = gce_raw_push(m, host, bytes, nullptr); if (rm != GCE_OK) return fail(e, rm, gce_last_error(m)); }
    return GCE_OK;
}

// BGZF members as they lie in the file (`comp`: host memory, comp_bytes; member k at coff[k], csize[k] bytes, ISIZE usize[k]) -> they are
// copied to HBM compressed and inflated BY THE GPU (gce_inflate.hpp), in one launch, when gce_raw_finish is called; their bytes follow what
// has been pushed so far.  Members with usize 0 (the EOF marker) may be passed or left out.  Asynchronous like gce_raw_push.
int gce_raw_push_bgzf(gce_engine *e, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, int32_t *ticket) {
    if (!e || !e->raw_mode || n_members < 0 || (n_members && (!comp || !coff || !csize || !usize))) return GCE_ERR_INVALID;
    for (int32_t k = 0; k < n_members; k++)                                             // every member is looked at before anything is queued or counted
        if (coff[k] > comp_bytes || csize[k] > comp_bytes - coff[k] || usize[k] > 0x10000u) return fail(e, GCE_ERR_INVALID, "BGZF member outside its buffer");
    (void)hipSetDevice(e->prm.device);
    // (gce_raw_begin sized the raw stream for ~5 x the file: a quarter of it holds the file, no second growth)
    HIPCHK(dev_grow_keep(e->z_comp, e->z_n + comp_bytes + 64, e->z_n, DevBuf::padded(std::max<size_t>((e->z_n + comp_bytes) * 2, e->raw.cap / 4) + 64), e->up_stream));
    if (comp_bytes) HIPCHK(hipMemcpyAsync((char *)e->z_comp.p + e->z_n, comp, comp_bytes, hipMemcpyHostToDevice, e->up_stream));
    for (int32_t k = 0; k < n_members; k++) {
        if (usize[k] == 0) continue;
        InfDir d; d.coff = e->z_n + coff[k]; d.uoff = e->raw_n; d.csize = csize[k]; d.usize = usize[k];
        e->z_members.push_back(d); e->raw_n += usize[k];
    }
    e->z_n += comp_bytes;
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev, e->up_stream));
    e->up_events.push_back(ev);
    if (ticket) *ticket = (int32_t)e->up_events.size() - 1;
    for (gce_engine *m : e->mirrors) { const int rm = gce_raw_push_bgzf(m, comp, comp_bytes, n_members, coff, csize, usize, nullptr); if (rm != GCE_OK) return fail(e, rm, gce_last_error(m)); }
    return GCE_OK;
}

// the launch behind gce_raw_push_bgzf: every member waiting, one lane each
static int raw_inflate_pending(gce_engine *e) {
    if (e->z_members.empty()) return GCE_OK;
    hipStream_t s = e->stream;
    // (everything so far is kept: host windows may lie between the members' places)
    HIPCHK(dev_grow_keep(e->raw, e->raw_n + 256, std::min(e->raw_n, e->raw.cap), DevBuf::padded(e->raw_n + 256), s));
    int64_t bad = -1; std::string msg;
    const int rc = dev_inflate_members(e->z_comp.as<uint8_t>(), e->z_n, e->z_members.data(), e->z_members.size(), e->raw.as<uint8_t>(), e->z_dir, e->z_err, s, &bad, msg);
    if (rc != GCE_OK) return fail(e, rc, msg);
    e->z_comp.release();                                                           // (the compressed copy of the file: not needed while the stream is processed)
    e->z_members.clear(); e->z_n = 0;
    if (bad >= 0) { char m[96]; snprintf(m, sizeof m, "inflate / CRC failure in BGZF member %u of the GPU batch", (uint32_t)bad); return fail(e, GCE_ERR_INVALID, m); }
    return GCE_OK;
}

// BGZF members -> bytes, nothing else (tests, tools): the decoder of gce_raw_push_bgzf on buffers of the caller.  first_bad: -1 or the first
// member that failed a check (its bytes and those of later failures are undefined).
int gce_bgzf_inflate(int32_t device, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, void *out, int32_t *first_bad) {
    if (n_members < 0 || (n_members && (!comp || !coff || !csize || !usize || !out))) return GCE_ERR_INVALID;
    if (first_bad) *first_bad = -1;
    if (hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    std::vector<InfDir> dir; uint64_t total = 0;
    for (int32_t k = 0; k < n_members; k++) {
        if (coff[k] > comp_bytes || csize[k] > comp_bytes - coff[k] || usize[k] > 0x10000u) return GCE_ERR_INVALID;
        InfDir d; d.coff = coff[k]; d.uoff = total; d.csize = csize[k]; d.usize = usize[k]; dir.push_back(d); total += usize[k];
    }
    if (dir.empty()) return GCE_OK;
    ScopedBuf zc, zd, ze, zo;
    if (zc.ensure(comp_bytes + 64) != hipSuccess || zo.ensure(total + 64) != hipSuccess) return GCE_ERR_OOM;
    if (hipMemcpy(zc.p, comp, comp_bytes, hipMemcpyHostToDevice) != hipSuccess) return GCE_ERR_HIP;
    int64_t bad = -1; std::string msg;
    const int rc = dev_inflate_members(zc.as<uint8_t>(), comp_bytes, dir.data(), dir.size(), zo.as<uint8_t>(), zd, ze, 0, &bad, msg);
    if (rc != GCE_OK) return rc;
    if (total && hipMemcpy(out, zo.p, total, hipMemcpyDeviceToHost) != hipSuccess) return GCE_ERR_HIP;
    if (bad >= 0) { if (first_bad) *first_bad = (int32_t)bad; return GCE_ERR_INVALID; }
    return GCE_OK;
}

// The encoder of gce_raw_deflate_output on the caller's buffer (tests, tools): `n` bytes -> BGZF blocks of `block_bytes` input bytes each (<= 65 280),
// back to back in out[0 .. *out_bytes); out_cap >= n + n / 8 + 64 x blocks is always enough.  Mirror of gce_bgzf_inflate.  codes: 0 = fixed Huffman
// codes (k_bgzf_deflate), 1 = per block the smallest of dynamic codes, fixed codes and stored (k_bgzf_deflate_dyn), 2 = dynamic codes wherever they
// fit the block's slot (tests of the degenerate trees).
int gce_bgzf_deflate_codes(int32_t device, const void *in, size_t n, uint32_t block_bytes, int32_t codes, void *out, size_t out_cap, size_t *out_bytes) {
    if ((n && !in) || !out_bytes || block_bytes < 1 || block_bytes > 0xff00u || (n && !out) || codes < 0 || codes > 2) return GCE_ERR_INVALID;
    *out_bytes = 0;
    if (hipSetDevice(device) != hipSuccess) return GCE_ERR_NO_DEVICE;
    if (!n) return GCE_OK;
    const uint64_t nb64 = (n + block_bytes - 1) / block_bytes;
    if (nb64 >= 0x7FFFFFF0ull) return GCE_ERR_INVALID;
    const uint32_t nb = (uint32_t)nb64, slot = block_bytes + block_bytes / 8 + 64;
    ScopedBuf zi, zs, zz, zo, zf, zt;
    if (zi.ensure(n + 64) != hipSuccess || zs.ensure((size_t)nb * slot + 64) != hipSuccess || zz.ensure(((size_t)nb + 1) * 4) != hipSuccess || zf.ensure(((size_t)nb + 1) * 8) != hipSuccess) return GCE_ERR_OOM;
    if (hipMemcpy(zi.p, in, n, hipMemcpyHostToDevice) != hipSuccess || hipMemset((char *)zi.p + n, 0, 64) != hipSuccess) return GCE_ERR_HIP;
    uint64_t csz = 0; std::string msg;
    const int rc = dev_deflate_members(codes, (const uint8_t *)zi.p, (uint64_t)n, block_bytes, nb, zs.as<uint8_t>(), slot, zz.as<uint32_t>(), zf.as<uint64_t>(), zt, 0, &csz, msg);
    if (rc != GCE_OK) return rc;
    if (csz > out_cap) return GCE_ERR_INVALID;
    if (zo.ensure(csz + 64) != hipSuccess) return GCE_ERR_OOM;
    dev_deflate_pack((const uint8_t *)zs.p, slot, (const uint32_t *)zz.p, (const uint64_t *)zf.p, nb, zo.as<uint8_t>(), 0);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess || hipMemcpy(out, zo.p, csz, hipMemcpyDeviceToHost) != hipSuccess) return GCE_ERR_HIP;
    *out_bytes = (size_t)csz;
    return GCE_OK;
}
int gce_bgzf_deflate(int32_t device, const void *in, size_t n, uint32_t block_bytes, void *out, size_t out_cap, size_t *out_bytes) {
    return gce_bgzf_deflate_codes(device, in, n, block_bytes, 0, out, out_cap, out_bytes);
}

// The whole stream is in HBM: index the records behind `records_begin` (the end of the BAM header), build the batch.  Afterwards the engine is
// in the state gce_submit_device leaves it in: gce_process, then gce_drain / gce_result_device or gce_raw_build_output.
int gce_raw_finish(gce_engine *e, uint64_t records_begin, int32_t n_ref, int64_t *n_records) {
    if (!e || !e->raw_mode || records_begin > e->raw_n) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    const bool tprint = getenv("GCE_RAW_TIMING") != nullptr; const auto tnow = [] { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }; double tq = tnow();
    auto lap = [&](const char *what) { if (tprint) { (void)hipStreamSynchronize(e->stream); const double x = tnow(); fprintf(stderr, "gce_raw_finish %s %.4f s\n", what, x - tq); tq = x; } };
    HIPCHK(hipStreamSynchronize(e->up_stream));
    lap("wait for the last copies");
    for (auto ev : e->up_events) (void)hipEventDestroy(ev);
    e->up_events.clear();
    { const int zr = raw_inflate_pending(e); if (zr != GCE_OK) return zr; }
    lap("BGZF members inflated by the GPU");
    hipStream_t s = e->stream;
    const uint8_t *u = e->raw.as<uint8_t>();
    const uint64_t total = e->raw_n;
    HIPCHK(hipMemsetAsync((char *)e->raw.p + total, 0, 64, s));                    // the blobs are readable 16 bytes past their end
    uint64_t n_rec = 0;
    for (int64_t &c : e->idx_ctr) c = 0;
    if (total > records_begin) {
        std::string msg; uint64_t end = 0;
        const int rc = dev_record_index<false>(e->rw, e->rw_tmp, s, u, records_begin, total, n_ref, e->idx_ctr, &n_rec, &end, msg);
        if (tprint) fprintf(stderr, "gce_raw_finish: %lld of %lld segments off the chain\n", (long long)e->idx_ctr[1], (long long)e->idx_ctr[0]);
        if (rc != GCE_OK) return fail(e, rc, msg);
        lap("record index");
    }
    const size_t n1 = (size_t)(n_rec ? n_rec : 1);
    HIPCHK(e->b_core.ensure(n1 * sizeof(gce_core) + 64)); HIPCHK(e->b_qoff.ensure(n1 * 8 + 64)); HIPCHK(e->b_coff.ensure(n1 * 8 + 64)); HIPCHK(e->b_soff.ensure(n1 * 8 + 64)); HIPCHK(e->b_loff.ensure(n1 * 8 + 64));
    HIPCHK(e->b_nm.ensure(n1 * 4 + 64)); HIPCHK(e->b_nmt.ensure(n1 + 64)); HIPCHK(e->b_mioff.ensure(n1 * 8 + 64)); HIPCHK(e->rw_ncig.ensure(n1 * 4 + 64)); HIPCHK(e->rw_nmpos.ensure(n1 * 4 + 64));
    lap("offsets + allocations");
    uint64_t cig_words = 0;
    unsigned int have_mi = 0;
    if (n_rec) {
        RawSoA o{e->b_core.as<gce_core>(), e->b_qoff.as<uint64_t>(), e->b_soff.as<uint64_t>(), e->b_loff.as<uint64_t>(), e->b_mioff.as<uint64_t>(), e->rw_ncig.as<uint32_t>(), e->rw_nmpos.as<uint32_t>(),
                 e->b_nm.as<int32_t>(), e->b_nmt.as<uint8_t>(), e->rw.misc.as<unsigned int>() + 2, e->rw.misc.as<unsigned int>() + 4, n_ref};
        HIPCHK(hipMemsetAsync(e->rw.misc.as<unsigned int>() + 4, 0xFF, 4, s));
        const unsigned nbr = (unsigned)((n_rec + 255) / 256);
        hipLaunchKernelGGL(k_raw_fill, dim3(nbr), dim3(256), 0, s, u, (const uint64_t *)e->rw.off.p, n_rec, o);
        HIPCHK(e->b_coff.ensure((n1 + 1) * 8 + 64));
        HIPCHK(dev_exclusive_sum(e->rw_ncig.as<uint32_t>(), n_rec, e->b_coff.as<uint64_t>(), e->rw_tmp, s));
        HIPCHK(hipMemcpyAsync(&cig_words, e->b_coff.as<uint64_t>() + n_rec, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&have_mi, e->rw.misc.as<unsigned int>() + 2, 4, hipMemcpyDeviceToHost, s));
        unsigned int bad_rec = NONE32;
        HIPCHK(hipMemcpyAsync(&bad_rec, e->rw.misc.as<unsigned int>() + 4, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (bad_rec != NONE32) { char m[96]; snprintf(m, sizeof m, "inconsistent record lengths (record %u)", bad_rec); return fail(e, GCE_ERR_INVALID, m); }
        HIPCHK(e->b_cigar.ensure((size_t)cig_words * 4 + 64));
        hipLaunchKernelGGL(k_raw_cigar, dim3(nbr), dim3(256), 0, s, u, (const uint64_t *)e->rw.off.p, n_rec, (const uint64_t *)e->b_coff.p, e->b_cigar.as<uint32_t>());
    } else HIPCHK(e->b_cigar.ensure(64));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    lap("fill + cigar");
    gce_batch &d = e->dev_batch; memset(&d, 0, sizeof d);
    d.n_reads = (int64_t)n_rec; d.core = e->b_core.as<gce_core>();
    d.qname_off = e->b_qoff.as<uint64_t>(); d.qname = e->raw.as<char>(); d.cigar_off = e->b_coff.as<uint64_t>(); d.cigar = e->b_cigar.as<uint32_t>();
    d.seq_off = e->b_soff.as<uint64_t>(); d.seq = e->raw.as<uint8_t>(); d.qual_off = e->b_loff.as<uint64_t>(); d.qual = e->raw.as<uint8_t>();
    d.nm = e->b_nm.as<int32_t>(); d.nm_type = e->b_nmt.as<uint8_t>();
    if (have_mi) { d.mi_off = e->b_mioff.as<uint64_t>(); d.mi = e->raw.as<char>(); d.mi_bytes = total; }
    d.qname_bytes = total; d.cigar_words = cig_words; d.seq_bytes = total; d.qual_bytes = total;
    e->device_mode = true; e->have_tick = false; e->raw_records = (int64_t)n_rec;
    if (n_records) *n_records = (int64_t)n_rec;
    return GCE_OK;
}

// after gce_process: the emitted records as a stream of BAM records in HBM, in the order of the output table
int gce_raw_build_output(gce_engine *e, uint64_t *body_bytes, int64_t *n_out) {
    if (!e || !e->raw_mode || !e->processed || e->dev_error || !body_bytes) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    hipStream_t s = e->stream;
    const uint64_t no = (uint64_t)e->n_out;
    *body_bytes = 0; if (n_out) *n_out = e->n_out;
    e->raw_body_nrec = -1;
    if (!no) return GCE_OK;
    HIPCHK(e->rw_rsize.ensure((no + 1) * 8)); HIPCHK(e->rw_roff.ensure((no + 1) * 8));
    const uint8_t *u = e->raw.as<uint8_t>();
    RawOut r{e->o_src.as<uint32_t>(), e->o_qsrc.as<uint32_t>(), e->o_nm.as<int32_t>(), e->o_fr.as<int16_t>(), e->o_rr.as<int16_t>()};
    const unsigned nb = (unsigned)((no + 255) / 256);
    hipLaunchKernelGGL(k_rec_size, dim3(nb), dim3(256), 0, s, u, (const uint64_t *)e->rw.off.p, r, no, e->rw_rsize.as<uint64_t>());
    HIPCHK(dev_exclusive_sum(e->rw_rsize.as<uint64_t>(), no, e->rw_roff.as<uint64_t>(), e->rw_tmp, s));
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, e->rw_roff.as<uint64_t>() + no, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    HIPCHK(e->rw_body.ensure(total + 64));
    hipLaunchKernelGGL(k_rec_build, dim3((unsigned)std::min<uint64_t>((no + 15) / 16, 65535u)), dim3(256), 0, s, u, (const uint64_t *)e->rw.off.p, (const uint32_t *)e->rw_nmpos.p, r, no, (const uint64_t *)e->rw_roff.p, e->rw_body.as<uint8_t>());
    hipLaunchKernelGGL(k_rec_nm, dim3(nb), dim3(256), 0, s, u, (const uint64_t *)e->rw.off.p, (const uint32_t *)e->rw_nmpos.p, r, no, (const uint64_t *)e->rw_roff.p, e->rw_body.as<uint8_t>());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    e->raw_body_bytes = total; e->raw_body_nrec = (int64_t)no;                       // (rw_roff: the record starts, for gce_raw_format_output)
    *body_bytes = total;
    return GCE_OK;
}

int gce_raw_read_output_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket) {
    if (!e || !e->raw_mode || offset + bytes > e->raw_body_bytes || (!host && bytes)) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    if (bytes) HIPCHK(hipMemcpyAsync(host, (const char *)e->rw_body.p + offset, bytes, hipMemcpyDeviceToHost, e->up_stream));
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev, e->up_stream));
    e->up_events.push_back(ev);
    if (ticket) *ticket = (int32_t)e->up_events.size() - 1;
    return GCE_OK;
}


// ---- several engines over ONE file (gce_run_bam_sharded): the mirrors of an engine receive every gce_raw_push / gce_raw_push_bgzf made to it
int gce_raw_attach_mirror(gce_engine *e, gce_engine *mirror) {
    if (!e || !mirror || e == mirror || !e->raw_mode || !mirror->raw_mode || e->raw_n != mirror->raw_n) return GCE_ERR_INVALID;
    // gce_submit_wait waits on the SAME ticket number of every mirror: the two engines must have handed out the same tickets so far, and neither
    // may hold BGZF members the other never saw (an attach behind an earlier push made the wait land on the wrong event)
    if (e->up_events.size() != mirror->up_events.size() || !e->z_members.empty() || !mirror->z_members.empty()) return fail(e, GCE_ERR_INVALID, "gce_raw_attach_mirror: attach before the first push to either engine");
    e->mirrors.push_back(mirror);
    return GCE_OK;
}
// After gce_raw_finish: this engine keeps shard `rank` of `world` of the stream it holds -- the planner runs on its own device over the key
// records in HBM (gce_stream_context: every read's global tick, the flush events of the whole stream; gce_plan_shards: key ranges or clusters
// dealt by weight), the reads of the shard are gathered (key records and per-read words; names, CIGARs, bases and qualities stay in the raw
// stream), the engine gets their ticks and the events.  Every engine of a sharded run computes the same plan from the same stream: nothing is
// exchanged.  Replaces the host-side cut of round 2's runner (gencore.cpp:164-205 over several GPUs).
int gce_raw_select_shard(gce_engine *e, int32_t world, int32_t rank, int32_t plan_mode) {
    if (!e || !e->raw_mode || !e->device_mode || e->processed || world < 1 || rank < 0 || rank >= world) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    int64_t n = e->raw_records;
    hipStream_t s = e->stream;
    e->shard_n = 0;
    if (n == 0) { e->have_tick = false; return GCE_OK; }
    const int64_t n_all = n;
    // --quit_after_contig (gencore.cpp:243-246) ends the loop ONCE, on the first read of the whole stream with tid >= maxContig: that read is
    // counted by the pre-Stats and nothing behind it exists.  The cut is made here, on the whole stream, in front of the plan: shard 0 receives
    // the cut read behind its own reads and counts it (its gce_process finds the cut there), the other engines do not look for a cut at all --
    // every shard cutting its own part counted one extra read per shard that held a read of the later contigs.
    int64_t cut = -1;
    e->shard_cut_done = false;
    if (e->prm.max_contig > 0) {
        unsigned int first = NONE32;
        HIPCHK(hipMemcpyAsync(e->rw.misc.p, &first, 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_first_contig_ge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const gce_core *)e->b_core.as<gce_core>(), n, e->prm.max_contig, (unsigned int *)e->rw.misc.p);
        HIPCHK(hipMemcpyAsync(&first, e->rw.misc.p, 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
        if (first != NONE32) { cut = (int64_t)first; n = cut; }
        e->shard_cut_done = rank != 0 || cut < 0;
    }
    HIPCHK(e->sh_tickall.ensure((size_t)n_all * 8)); HIPCHK(e->sh_shard.ensure((size_t)n_all * 4)); HIPCHK(e->sh_flag.ensure((size_t)n_all + 64)); HIPCHK(e->sh_sel.ensure((size_t)n_all * 4 + 64));
    int rc;
    if (n > 0) {
        int32_t n_ev = 0, *ev_tid = nullptr, *ev_pos = nullptr;
        const int period = e->prm.flush_period > 0 ? e->prm.flush_period : 10000;
        rc = gce_stream_context(e->prm.device, e->b_core.as<gce_core>(), n, period, e->sh_tickall.as<uint64_t>(), &n_ev, &ev_tid, &ev_pos);
        if (rc != GCE_OK) return fail(e, rc, rc == GCE_ERR_INVALID ? "not shardable by cluster key: a mapped read follows the first unmapped read" : gce_status_message(rc));
        rc = gce_set_flush_events(e, n_ev, ev_tid, ev_pos);
        gce_free(ev_tid); gce_free(ev_pos);
        if (rc != GCE_OK) return rc;
        if ((rc = gce_plan_shards(e->prm.device, e->b_core.as<gce_core>(), n, world, plan_mode, e->sh_shard.as<int32_t>())) != GCE_OK) return fail(e, rc, gce_status_message(rc));
        const unsigned nb = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(k_shard_flag, dim3(nb), dim3(256), 0, s, (const int32_t *)e->sh_shard.p, n, rank, e->sh_flag.as<uint8_t>());
    } else if ((rc = gce_set_flush_events(e, 0, nullptr, nullptr)) != GCE_OK) return rc;
    if (cut >= 0) {                                                                  // the cut read: shard 0's last read (its tick is never looked at: gce_process drops it)
        HIPCHK(hipMemsetAsync(e->sh_flag.as<uint8_t>() + cut, rank == 0 ? 1 : 0, 1, s));
        HIPCHK(hipMemsetAsync(e->sh_tickall.as<uint64_t>() + cut, 0, 8, s));
    }
    HIPCHK(dev_select_flagged(e->sh_flag.as<uint8_t>(), (uint64_t)(n + (cut >= 0 ? 1 : 0)), e->sh_sel.as<uint32_t>(), (unsigned long long *)e->rw.misc.p, e->rw_tmp, s));
    int64_t m = 0;
    HIPCHK(hipMemcpyAsync(&m, e->rw.misc.p, 8, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    const size_t m1 = (size_t)(m > 0 ? m : 1);
    HIPCHK(e->sh_core.ensure(m1 * sizeof(gce_core) + 64)); HIPCHK(e->sh_qoff.ensure(m1 * 8 + 64)); HIPCHK(e->sh_coff.ensure(m1 * 8 + 64)); HIPCHK(e->sh_soff.ensure(m1 * 8 + 64)); HIPCHK(e->sh_loff.ensure(m1 * 8 + 64));
    HIPCHK(e->sh_nm.ensure(m1 * 4 + 64)); HIPCHK(e->sh_nmt.ensure(m1 + 64)); HIPCHK(e->sh_mioff.ensure(m1 * 8 + 64)); HIPCHK(e->sh_tick.ensure(m1 * 8 + 64)); HIPCHK(e->sh_roff.ensure(m1 * 8 + 64)); HIPCHK(e->sh_nmpos.ensure(m1 * 4 + 64));
    gce_batch &d = e->dev_batch;
    if (m > 0) {
        ShardSrc a{d.core, d.qname_off, d.cigar_off, d.seq_off, d.qual_off, d.mi_off, (const uint64_t *)e->sh_tickall.p, (const uint64_t *)e->rw.off.p, d.nm, d.nm_type, (const uint32_t *)e->rw_nmpos.p};
        ShardDst o{e->sh_core.as<gce_core>(), e->sh_qoff.as<uint64_t>(), e->sh_coff.as<uint64_t>(), e->sh_soff.as<uint64_t>(), e->sh_loff.as<uint64_t>(), e->sh_mioff.as<uint64_t>(), e->sh_tick.as<uint64_t>(),
                   e->sh_roff.as<uint64_t>(), e->sh_nm.as<int32_t>(), e->sh_nmt.as<uint8_t>(), e->sh_nmpos.as<uint32_t>()};
        hipLaunchKernelGGL(k_shard_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, (const uint32_t *)e->sh_sel.p, m, a, o);
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    d.n_reads = m; d.core = e->sh_core.as<gce_core>(); d.qname_off = e->sh_qoff.as<uint64_t>(); d.cigar_off = e->sh_coff.as<uint64_t>(); d.seq_off = e->sh_soff.as<uint64_t>(); d.qual_off = e->sh_loff.as<uint64_t>();
    d.nm = e->sh_nm.as<int32_t>(); d.nm_type = e->sh_nmt.as<uint8_t>(); if (d.mi_off) d.mi_off = e->sh_mioff.as<uint64_t>();
    d.tick = e->sh_tick.as<uint64_t>();
    std::swap(e->rw.off, e->sh_roff); std::swap(e->rw_nmpos, e->sh_nmpos);          // gce_raw_build_output looks records up by the batch's (now: the shard's) read index
    e->have_tick = true; e->raw_records = m; e->shard_n = m;
    e->sh_tickall.release(); e->sh_shard.release(); e->sh_flag.release();
    return GCE_OK;
}
// The Stats payloads of several engines (gce_stats_payload_device, same step and regions on every one) added into engs[0]'s, device to device.
int gce_stats_payload_sum(gce_engine **engs, int32_t n_engs, const int64_t **payload, gce_payload_layout *layout) {
    if (!engs || n_engs < 1 || !payload || !layout || !engs[0]) return GCE_ERR_INVALID;
    gce_engine *e = engs[0];
    const int nt = (int)e->target_len.size();
    if (e->h_binoff.size() != (size_t)nt + 1 || !e->dp_depth.p) return fail(e, GCE_ERR_INVALID, "gce_stats_payload_sum before gce_stats_payload_device");
    const int64_t nbins = e->h_binoff[nt];
    // (the number of regions is what is left of the buffer behind the Stats blocks and the bins: every engine was given the same list)
    for (int r = 1; r < n_engs; r++) if (!engs[r] || engs[r]->h_binoff != e->h_binoff || !engs[r]->dp_depth.p || engs[r]->payload_words != e->payload_words) return fail(e, GCE_ERR_INVALID, "gce_stats_payload_sum: the engines' payloads differ in shape");
    const int64_t words = e->payload_words;
    (void)hipSetDevice(e->prm.device);
    hipStream_t s = e->stream;
    if (n_engs > 1) {
        DevBuf tmp; HIPCHK(tmp.ensure((size_t)words * 8 + 64));
        for (int r = 1; r < n_engs; r++) {
            gce_engine *x = engs[r];
            (void)hipSetDevice(x->prm.device); HIPCHK(hipStreamSynchronize(x->stream)); (void)hipSetDevice(e->prm.device);      // x's payload kernels are through
            const hipError_t ce = x->prm.device == e->prm.device ? hipMemcpyAsync(tmp.p, x->dp_depth.p, (size_t)words * 8, hipMemcpyDeviceToDevice, s)
                                                                  : hipMemcpyPeerAsync(tmp.p, e->prm.device, x->dp_depth.p, x->prm.device, (size_t)words * 8, s);
            if (ce != hipSuccess) return fail(e, GCE_ERR_HIP, "payload sum: device-to-device copy");
            hipLaunchKernelGGL(k_add_i64, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, e->dp_depth.as<long long>(), (const long long *)tmp.p, (int)words);
        }
        HIPCHK(hipStreamSynchronize(s));
        tmp.release();
    }
    layout->stats_words = 2 * GCE_STATS_WORDS; layout->n_targets = nt; layout->n_bins = nbins; layout->n_regions = (int32_t)((words - 2 * GCE_STATS_WORDS - 2 * nbins) / 2); layout->total_words = words;
    layout->bin_off = e->h_binoff.data();
    *payload = e->dp_depth.as<int64_t>();
    return GCE_OK;
}
// After every engine's gce_raw_build_output: the shards' record streams (each in bamComp order) merged into ONE stream in bamComp order over the
// whole file -- (tid, pos, mtid, mpos, isize, place in the input stream), gencore.h:19-47 -- in engs[0]'s output buffer, so that the writer
// streams it like a single engine's; the Stats blocks summed device to device into engs[0]'s (no host bounce of the blocks, no collective).
// The order is worked out on the host from 32 bytes per emitted record (runs of one shard are found by bisection: key ranges overlap only at
// their borders), the bytes are moved by the GPU.
int gce_raw_merge_outputs(gce_engine **engs, int32_t n_engs, uint64_t *body_bytes, int64_t *n_out_total, gce_stats *pre, gce_stats *post, int64_t *n_reads_total) {
    if (!engs || n_engs < 1 || !body_bytes) return GCE_ERR_INVALID;
    gce_engine *e = engs[0];
    for (int r = 0; r < n_engs; r++) if (!engs[r] || !engs[r]->raw_mode || !engs[r]->processed || engs[r]->dev_error) return GCE_ERR_INVALID;
    e->raw_body_nrec = -1;
    std::vector<std::vector<MergeKey>> keys((size_t)n_engs);
    std::vector<uint64_t> base((size_t)n_engs + 1, 0);                              // where shard r's stream lies in the staging buffer
    int64_t total_out = 0, total_reads = 0;
    for (int r = 0; r < n_engs; r++) {
        gce_engine *x = engs[r];
        (void)hipSetDevice(x->prm.device);
        const uint64_t no = (uint64_t)x->n_out;
        base[r + 1] = base[r] + x->raw_body_bytes; total_out += x->n_out; total_reads += x->n;
        keys[r].resize((size_t)no);
        if (!no) continue;
        if (x->sh_keys.ensure(no * sizeof(MergeKey)) != hipSuccess) return fail(e, GCE_ERR_OOM, "out of device memory");
        hipLaunchKernelGGL(k_merge_keys, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, x->stream, x->dev_batch.core, (const uint32_t *)x->o_src.p, x->shard_n >= 0 ? (const uint32_t *)x->sh_sel.p : (const uint32_t *)nullptr,
                           (const uint64_t *)x->rw_rsize.p, no, x->sh_keys.as<MergeKey>());
        if (hipMemcpyAsync(keys[r].data(), x->sh_keys.p, no * sizeof(MergeKey), hipMemcpyDeviceToHost, x->stream) != hipSuccess || hipStreamSynchronize(x->stream) != hipSuccess) return fail(e, GCE_ERR_HIP, "merge keys");
    }
    const uint64_t total = base[n_engs];
    // ---- the order: smallest head first, then as many records of that shard as stay in front of every other head
    std::vector<uint64_t> from((size_t)std::max<int64_t>(total_out, 1)), to((size_t)std::max<int64_t>(total_out, 1)); std::vector<uint32_t> size((size_t)std::max<int64_t>(total_out, 1));
    auto less = [](const MergeKey &a, const MergeKey &b) {
        if (a.tid != b.tid) return a.tid < b.tid;
        if (a.pos != b.pos) return a.pos < b.pos;
        if (a.mtid != b.mtid) return a.mtid < b.mtid;
        if (a.mpos != b.mpos) return a.mpos < b.mpos;
        if (a.isize != b.isize) return a.isize < b.isize;
        return a.gidx < b.gidx;
    };
    {
        std::vector<size_t> head((size_t)n_engs, 0); std::vector<uint64_t> soff((size_t)n_engs, 0);
        int64_t row = 0; uint64_t at = 0;
        while (row < total_out) {
            int best = -1, second = -1;
            for (int r = 0; r < n_engs; r++) if (head[r] < keys[r].size()) {
                if (best < 0 || less(keys[r][head[r]], keys[best][head[best]])) { second = best; best = r; }
                else if (second < 0 || less(keys[r][head[r]], keys[second][head[second]])) second = r;
            }
            size_t stop = keys[best].size();
            if (second >= 0) {                                                      // the first record of `best` that is not in front of `second`'s head (the shard's table is sorted)
                const MergeKey &lim = keys[second][head[second]];
                size_t a = head[best] + 1, z = keys[best].size();
                while (a < z) { const size_t mid = (a + z) >> 1; if (less(keys[best][mid], lim)) a = mid + 1; else z = mid; }
                stop = a;
            }
            for (size_t k = head[best]; k < stop; k++, row++) { const uint32_t sz = keys[best][k].size; from[row] = base[best] + soff[best]; to[row] = at; size[row] = sz; soff[best] += sz; at += sz; }
            head[best] = stop;
        }
        if (at != total) return fail(e, GCE_ERR_INVALID, "merge: record sizes do not add up");
    }
    // ---- the bytes: every shard's stream staged on engs[0]'s device, one gather into the merged stream
    (void)hipSetDevice(e->prm.device);
    hipStream_t s = e->stream;
    if (e->sh_stage.ensure(total + 64) != hipSuccess) return fail(e, GCE_ERR_OOM, "out of device memory");
    for (int r = 0; r < n_engs; r++) {
        gce_engine *x = engs[r];
        if (!x->raw_body_bytes) continue;
        const hipError_t ce = x->prm.device == e->prm.device ? hipMemcpyAsync((char *)e->sh_stage.p + base[r], x->rw_body.p, x->raw_body_bytes, hipMemcpyDeviceToDevice, s)
                                                              : hipMemcpyPeerAsync((char *)e->sh_stage.p + base[r], e->prm.device, x->rw_body.p, x->prm.device, x->raw_body_bytes, s);
        if (ce != hipSuccess) return fail(e, GCE_ERR_HIP, "merge: device-to-device copy");
    }
    HIPCHK(hipStreamSynchronize(s));                                                 // (engs[0]'s own stream was the source of one of the copies: it may be overwritten from here on)
    if (total_out > 0) {
        DevBuf d_from, d_to, d_size;
        HIPCHK(d_from.ensure((size_t)total_out * 8)); HIPCHK(d_to.ensure((size_t)total_out * 8)); HIPCHK(d_size.ensure((size_t)total_out * 4));
        HIPCHK(hipMemcpyAsync(d_from.p, from.data(), (size_t)total_out * 8, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(d_to.p, to.data(), (size_t)total_out * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_size.p, size.data(), (size_t)total_out * 4, hipMemcpyHostToDevice, s));
        HIPCHK(e->rw_body.ensure(total + 64));
        hipLaunchKernelGGL(k_merge_copy, dim3((unsigned)std::min<uint64_t>(((uint64_t)total_out + 15) / 16, 65535u)), dim3(256), 0, s, (const uint8_t *)e->sh_stage.p, (const uint64_t *)d_from.p, (const uint64_t *)d_to.p,
                           (const uint32_t *)d_size.p, (uint64_t)total_out, e->rw_body.as<uint8_t>());
        // the merged stream's record starts stay behind for gce_raw_format_output (engs[0]'s own were read into the keys above)
        HIPCHK(e->rw_roff.ensure(((size_t)total_out + 1) * 8));
        HIPCHK(hipMemcpyAsync(e->rw_roff.p, d_to.p, (size_t)total_out * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(e->rw_roff.as<uint64_t>() + total_out, &total, 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        e->raw_body_nrec = total_out;
        d_from.release(); d_to.release(); d_size.release();
    }
    e->sh_stage.release();
    e->raw_body_bytes = total;
    // ---- Stats: the shards' blocks added into engs[0]'s, device to device
    const int W2 = 2 * GCE_STATS_WORDS;
    if (n_engs > 1) {
        DevBuf tmp; HIPCHK(tmp.ensure((size_t)W2 * 8));
        long long *acc = (long long *)e->si.as<StreamInfo>()->pre;
        for (int r = 1; r < n_engs; r++) {
            gce_engine *x = engs[r];
            const void *src = (const void *)x->si.as<StreamInfo>()->pre;
            const hipError_t ce = x->prm.device == e->prm.device ? hipMemcpyAsync(tmp.p, src, (size_t)W2 * 8, hipMemcpyDeviceToDevice, s) : hipMemcpyPeerAsync(tmp.p, e->prm.device, src, x->prm.device, (size_t)W2 * 8, s);
            if (ce != hipSuccess) return fail(e, GCE_ERR_HIP, "merge: Stats copy");
            hipLaunchKernelGGL(k_add_i64, dim3((W2 + 255) / 256), dim3(256), 0, s, acc, (const long long *)tmp.p, W2);
        }
        HIPCHK(hipStreamSynchronize(s));
        tmp.release();
    }
    static_assert(offsetof(StreamInfo, post) == offsetof(StreamInfo, pre) + GCE_STATS_WORDS * 8, "pre and post lie back to back");
    long long both[2 * GCE_STATS_WORDS];
    HIPCHK(hipMemcpy(both, e->si.as<StreamInfo>()->pre, sizeof both, hipMemcpyDeviceToHost));
    if (pre) memcpy(pre, both, GCE_STATS_WORDS * 8);
    if (post) memcpy(post, both + GCE_STATS_WORDS, GCE_STATS_WORDS * 8);
    *body_bytes = total;
    if (n_out_total) *n_out_total = total_out;
    if (n_reads_total) *n_reads_total = total_reads;
    return GCE_OK;
}


// After gce_raw_build_output (or gce_raw_merge_outputs): the record stream compressed into BGZF blocks by the GPU (gce_deflate.hpp: greedy LZ77,
// fixed Huffman codes, one lane per block) -- replaces bgzf_write's deflate under sam_write1 (src/gencore.cpp:104).  *comp_bytes = size of the
// file image of the records (BGZF blocks back to back; the caller writes the BAM header's blocks in front and the EOF marker behind);
// gce_raw_read_deflated_async copies a piece of it to the host.  codes: 0 = fixed codes, 1 = the smallest of dynamic / fixed / stored per block
// (2, the forcing switch of gce_bgzf_deflate_codes for tests, is refused here).
int gce_raw_deflate_output_codes(gce_engine *e, int32_t codes, uint64_t *comp_bytes) {
    if (!e || !e->raw_mode || !comp_bytes || codes < 0 || codes > 1) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    hipStream_t s = e->stream;
    const uint64_t total = e->raw_body_bytes;
    *comp_bytes = 0; e->zo_bytes = 0;
    if (!total) return GCE_OK;
    // input bytes per block: enough blocks for every CU's 32 lanes (one workgroup per CU: the hash tables fill its LDS), never more than BGZF's 65 280
    uint64_t blk = (total + 8191) / 8192; blk = (blk + 255) & ~(uint64_t)255;
    if (blk < 4096) blk = 4096; if (blk > 0xff00) blk = 0xff00;
    const uint64_t nb64 = (total + blk - 1) / blk;
    if (nb64 >= 0x7FFFFFF0ull) return fail(e, GCE_ERR_INVALID, "output stream too large for one deflate pass");
    const uint32_t nb = (uint32_t)nb64, slot = (uint32_t)(blk + blk / 8 + 64);
    HIPCHK(e->zo_slots.ensure((size_t)nb * slot + 64)); HIPCHK(e->zo_sizes.ensure(((size_t)nb + 1) * 4)); HIPCHK(e->zo_off.ensure(((size_t)nb + 1) * 8));
    uint64_t csz = 0; std::string msg;
    const int rc = dev_deflate_members(codes, (const uint8_t *)e->rw_body.p, total, (uint32_t)blk, nb, e->zo_slots.as<uint8_t>(), slot, e->zo_sizes.as<uint32_t>(), e->zo_off.as<uint64_t>(), e->rw_tmp, s, &csz, msg);
    if (rc != GCE_OK) return fail(e, rc, msg);
    HIPCHK(e->zo_out.ensure(csz + 64));
    dev_deflate_pack((const uint8_t *)e->zo_slots.p, slot, (const uint32_t *)e->zo_sizes.p, (const uint64_t *)e->zo_off.p, nb, e->zo_out.as<uint8_t>(), s);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    e->zo_slots.release();
    e->zo_bytes = csz; *comp_bytes = csz;
    return GCE_OK;
}
int gce_raw_deflate_output(gce_engine *e, uint64_t *comp_bytes) { return gce_raw_deflate_output_codes(e, 0, comp_bytes); }
int gce_raw_read_deflated_async(gce_engine *e, uint64_t offset, void *host, size_t bytes, int32_t *ticket) {
    if (!e || !e->raw_mode || offset + bytes > e->zo_bytes || (!host && bytes)) return GCE_ERR_INVALID;
    (void)hipSetDevice(e->prm.device);
    if (bytes) HIPCHK(hipMemcpyAsync(host, (const char *)e->zo_out.p + offset, bytes, hipMemcpyDeviceToHost, e->up_stream));
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev, e->up_stream));
    e->up_events.push_back(ev);
    if (ticket) *ticket = (int32_t)e->up_events.size() - 1;
    return GCE_OK;
}

// pinned host memory for the windows of the file path (the DMA engines copy from / to it without a staging copy)
int gce_host_alloc(size_t bytes, void **out) { if (!out) return GCE_ERR_INVALID; return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable) == hipSuccess ? GCE_OK : GCE_ERR_OOM; }      // (portable: the sharded runner's devices all copy from the same windows)
void gce_host_free(void *p) { if (p) (void)hipHostFree(p); }

}  // extern "C"
