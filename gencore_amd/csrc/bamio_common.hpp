// bamio_common.hpp -- what every file runner of bamio.cpp's parts does around its own work: the clock, the host thread count, a call's message,
// the input file, pinned host buffers, and what follows once the contig table is known (the engine's parameters, the reference, the depth
// report's arrays).  Host only; every function is inline or a template, so a program that uses a part of it links that part's needs alone.
#pragma once
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <sched.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../include/gencore_amd.h"
#include "gce_bgzf.hpp"

namespace {

inline double now_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

// host threads when the caller does not say: the CPUs this process may run on (affinity mask / cgroup quota), at most 64 -- on the
// 256-thread box the measurements were made on, inflate and deflate stop scaling near 64 threads and lose 30 % at 256
inline int default_threads() {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min(n, std::max(1, CPU_COUNT(&set)));
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {                       // cgroup v2: "<quota> <period>" or "max <period>"
        long long q = 0, per = 0;
        if (fscanf(f, "%lld %lld", &q, &per) == 2 && q > 0 && per > 0) n = std::min<long long>(n, std::max<long long>(1, (q + per - 1) / per));
        fclose(f);
    }
    return std::min(n, 64);
}

// the message of a C-ABI call into its caller's buffer
inline void set_err(char err[256], const char *m) { if (err) { strncpy(err, m ? m : "", 255); err[255] = 0; } }

inline long status_kb(const char *key) { FILE *f = fopen("/proc/self/status", "r"); if (!f) return 0; char line[256]; long v = 0; const size_t kl = strlen(key); while (fgets(line, sizeof line, f)) if (strncmp(line, key, kl) == 0) { v = atol(line + kl); break; } fclose(f); return v; }

// the input file of a runner: opened and measured, closed when the runner is through with it
struct InputFile {
    int fd = -1; uint64_t fsz = 0; struct stat st{};
    InputFile() = default;
    InputFile(const InputFile &) = delete; InputFile &operator=(const InputFile &) = delete;
    ~InputFile() { close(); }
    // nullptr, or what could not be done ("open", "stat"): the runner says it in its own words
    const char *open(const char *path) {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return "open";
        if (fstat(fd, &st) != 0 || st.st_size < 0) { close(); return "stat"; }
        fsz = (uint64_t)st.st_size;
        return nullptr;
    }
    void close() { if (fd >= 0) { ::close(fd); fd = -1; } }
    // sam_open(in, "r") takes either format (src/gencore.cpp:164): a file that does not start with the gzip magic is SAM text
    bool is_sam() const { return fsz > 0 && !looks_gzip(fd, fsz); }
    bool is_bgzf() const { return starts_bgzf(fd, fsz); }
};

struct Pinned {                                   // a pinned host buffer that grows
    uint8_t *p = nullptr; size_t cap = 0;
    ~Pinned() { gce_host_free(p); }
    bool ensure(size_t n) { if (n <= cap) return true; gce_host_free(p); p = nullptr; cap = 0; void *q = nullptr; if (gce_host_alloc(n + (n >> 3) + 4096, &q) != GCE_OK) return false; p = (uint8_t *)q; cap = n + (n >> 3) + 4096; return true; }
};

// ---- what every runner does once the contig table is known
inline bool umi_auto(const gce_params &prm) { return strcmp(prm.umi_prefix, "auto") == 0; }
// the contig table into the engine's parameters; the "auto" UMI prefix from the first record's name, or none without one (src/gencore.cpp:207-220)
inline void file_params(gce_params &prm, int32_t n_targets, const uint32_t *target_len, const char *first_qname) {
    prm.n_targets = n_targets; prm.target_len = target_len;
    if (!umi_auto(prm)) return;
    memset(prm.umi_prefix, 0, sizeof prm.umi_prefix);
    if (first_qname) gce_detect_umi_prefix(first_qname, prm.umi_prefix);
}
inline bool same_name(const char *a, const char *b) { return strcmp(a, b) == 0; }
inline bool same_name(const std::string &a, const char *b) { return a == b; }
// Reference::getData looks contigs up by BAM target name (reference.cpp:43-53): every contig of names[0, n) that the loaded FASTA has goes to
// the engine; the first status that is not GCE_OK is returned (gce_last_error(e) says why)
template <class Name> int set_reference(gce_engine *e, const gce_fasta *fa, const Name *names, size_t n) {
    int32_t nc = 0; const char *const *ids = nullptr; const char *const *seqs = nullptr; const int64_t *flen = nullptr; int rc;
    gce_fasta_get(fa, &nc, &ids, &seqs, &flen);
    for (size_t t = 0; t < n; t++)
        for (int32_t c = 0; c < nc; c++)
            if (same_name(names[t], ids[c]) && (rc = gce_set_reference_ascii(e, (int32_t)t, seqs[c], flen[c])) != GCE_OK) return rc;
    return GCE_OK;
}
// the contigs of names[] the loaded FASTA has, matched by name (a name counts up to its first NUL): seq[t] / len[t] are contig t's bases and
// their length as gce_sort_calmd_ref takes them, NULL / -1 for a contig the FASTA lacks
inline void match_contigs(const std::vector<std::string> &names, const gce_fasta *fa, std::vector<const char *> &seq, std::vector<int64_t> &len) {
    seq.assign(names.size(), nullptr); len.assign(names.size(), -1);
    int32_t nc = 0; const char *const *ids = nullptr; const char *const *seqs = nullptr; const int64_t *flen = nullptr;
    gce_fasta_get(fa, &nc, &ids, &seqs, &flen);
    std::unordered_map<std::string, int32_t> where;
    for (int32_t c = 0; c < nc; c++) where.emplace(ids[c], c);
    for (size_t t = 0; t < names.size(); t++) {
        auto it = where.find(names[t].c_str());
        if (it != where.end()) { seq[t] = seqs[it->second]; len[t] = flen[it->second]; }
    }
}
// the depth report's arrays (freed by gce_depth_run_free), n_regions being set: bins of coverage_step per contig, contigs back to back.  false: out of host memory
inline bool depth_alloc(gce_depth_run *depth, const std::vector<uint32_t> &lens, int32_t coverage_step) {
    const int nt = (int)lens.size();
    depth->n_targets = nt;
    depth->bin_off = (int64_t *)calloc((size_t)nt + 1, 8);
    if (!depth->bin_off) return false;
    for (int t = 0; t < nt; t++) depth->bin_off[t + 1] = depth->bin_off[t] + 1 + (int64_t)lens[(size_t)t] / coverage_step;
    const int64_t nb = depth->bin_off[nt];
    depth->n_bins = nb;
    depth->pre_depth = (int64_t *)calloc((size_t)std::max<int64_t>(nb, 1), 8); depth->post_depth = (int64_t *)calloc((size_t)std::max<int64_t>(nb, 1), 8);
    depth->pre_bed = (int64_t *)calloc((size_t)std::max(depth->n_regions, 1), 8); depth->post_bed = (int64_t *)calloc((size_t)std::max(depth->n_regions, 1), 8);
    depth->payload_bytes = (2 * (int64_t)GCE_STATS_WORDS + 2 * nb + 2 * (int64_t)depth->n_regions) * 8;
    return depth->pre_depth && depth->post_depth && depth->pre_bed && depth->post_bed;
}
// the payload's words (gce_payload_layout: two Stats blocks in stats_words words, then the depth and BED blocks) into those arrays
inline void depth_unpack(gce_depth_run *depth, const int64_t *words, int64_t stats_words) {
    const int64_t nb = depth->n_bins; const int32_t nreg = depth->n_regions;
    memcpy(&depth->pre, words, sizeof(gce_stats)); memcpy(&depth->post, words + GCE_STATS_WORDS, sizeof(gce_stats));
    const int64_t *d0 = words + stats_words;
    memcpy(depth->pre_depth, d0, (size_t)nb * 8); memcpy(depth->post_depth, d0 + nb, (size_t)nb * 8);
    memcpy(depth->pre_bed, d0 + 2 * nb, (size_t)nreg * 8); memcpy(depth->post_bed, d0 + 2 * nb + nreg, (size_t)nreg * 8);
}

}  // namespace
