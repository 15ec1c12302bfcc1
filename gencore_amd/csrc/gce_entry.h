// gce_entry.h — the device entry points the file side (bamio.cpp and its bamio_*.hpp parts) calls that include/gencore_amd.h does not
// declare: the pass, index, sort, calmd, UMI, pileup, fragment-pileup, error-profile and fragment-error-profile objects of gce_passes.hpp, gce_bai.hpp, gce_sort.hpp, gce_calmd.hpp, gce_umi.hpp, gce_pileup.hpp, gce_fragpile.hpp, gce_errprof.hpp and gce_fragerr.hpp, and the support-profile and quality-profile objects of gce_errsup.hpp and gce_errqual.hpp (the last six over gce_reduce.hpp), and the overlap merge of gce_ovlmerge.hpp over the sort object.  They are exported, but
// internal: their signatures may change with the library.  engine.hip includes this file in front of the headers that define them and the
// file side includes it to call them, so a definition and a call that drift apart are a build error (conflicting types), not a link that
// succeeds and breaks at run time.  Every gce_ prototype lives here or in the public header, nowhere else.
#ifndef GCE_ENTRY_H
#define GCE_ENTRY_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/gencore_amd.h"

extern "C" {

struct gce_passes;
struct gce_bai;
struct gce_sort;
struct gce_pileup;
struct gce_fragpile;
struct gce_errprof;
struct gce_fragerr;
struct gce_errsup;
struct gce_errqual;

int gce_device_mem_info(int32_t device, size_t *free_bytes, size_t *total_bytes);

// ---- one file in key-range passes on one device (gce_passes.hpp)
int gce_passes_create(int32_t device, int32_t max_contig, int32_t flush_period, gce_passes **out);
void gce_passes_destroy(gce_passes *p);
const char *gce_passes_error(gce_passes *p);
int gce_passes_window(gce_passes *p, gce_engine *e, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize,
                      uint64_t skip, int32_t n_ref, int32_t last, int32_t *cut_reached);
int gce_passes_plan(gce_passes *p, int32_t min_passes, uint64_t budget, uint64_t reserve, int32_t *P_out, uint64_t *total_w, uint64_t *per_pass, uint64_t *fixed_out);
int gce_passes_info(gce_passes *p, int32_t k, uint64_t *weight, const uint64_t **cuts, int32_t *n_events, const int32_t **ev_tid, const int32_t **ev_pos);
int gce_passes_begin(gce_passes *p, gce_engine *e, int32_t k);
int gce_passes_end(gce_passes *p, gce_engine *e, uint64_t records_begin, int32_t n_ref, int64_t *n_records, int32_t *watermark_tid, int32_t *watermark_pos);
int gce_passes_output(gce_passes *p, gce_engine *e, void *keys_host, void *body_host);
int gce_passes_release(gce_passes *p, gce_engine *e);

// ---- the BAI index of a coordinate-sorted BAM (gce_bai.hpp)
int gce_bai_create(int32_t device, gce_bai **out);
void gce_bai_destroy(gce_bai *b);
const char *gce_bai_error(gce_bai *b);
int gce_bai_window(gce_bai *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t file_base,
                   uint64_t skip, int32_t n_ref, int32_t last);
int gce_bai_finish(gce_bai *b, int32_t n_ref, uint64_t eod, int64_t counts[5], int64_t *bad_rec, int32_t *bad_kind);
int gce_bai_serialise(gce_bai *b, int32_t n_ref, uint8_t **out, size_t *out_bytes);

// ---- an unsorted BAM, or SAM text, into coordinate order (gce_sort.hpp)
int gce_sort_create(int32_t device, size_t device_budget_bytes, gce_sort **out);
void gce_sort_destroy(gce_sort *b);
const char *gce_sort_error(gce_sort *b);
int gce_sort_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                    int32_t n_ref, int32_t last, uint64_t est_bytes);
int gce_sort_finish(gce_sort *b, int32_t n_ref, int32_t codes, uint64_t piece_bytes, int64_t counts[3], int64_t *bad_rec, uint64_t *out_bytes, double times[2]);
int gce_sort_read(gce_sort *b, uint64_t offset, size_t bytes, int32_t codes, void *host, size_t host_cap, size_t *got);
int gce_sort_key_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, uint64_t est_bytes);
int gce_sort_plan(gce_sort *b, int32_t n_ref, int32_t codes, uint64_t piece_bytes, int32_t min_passes, int64_t counts[3], int64_t *bad_rec, uint64_t *total_out, int32_t *n_passes,
                  uint64_t *pass_bytes, uint64_t *resident, double *plan_s);
int gce_sort_pass_begin(gce_sort *b, uint64_t lo, uint64_t hi);
int gce_sort_pass_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                         int32_t n_ref, int32_t last);
int gce_sort_pass_end(gce_sort *b, double *scatter_s);
int gce_sort_sam_contigs(gce_sort *b, int32_t n_ref, const char *const *ref_name);
int gce_sort_sam_window(gce_sort *b, const char *text, size_t n, int32_t n_ref, uint64_t est_bytes, int64_t *n_host_lines, int64_t *bad_line, uint64_t *bad_start, double *parse_s,
                        uint64_t *resident_bytes);

// ---- NM and MD recomputed against the reference, in core and with the output streamed (gce_calmd.hpp)
int gce_sort_calmd_ref(gce_sort *b, int32_t n_ref, const char *const *seq, const int64_t *len);
int gce_sort_calmd_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                          int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s);
int gce_sort_calmd_finish(gce_sort *b, int32_t codes, uint64_t piece_bytes, int64_t counts[6], uint64_t *in_bytes, uint64_t *out_bytes);
int gce_sort_calmd_stream_begin(gce_sort *b, int32_t codes, uint64_t piece_bytes, uint64_t resident_bytes);
int gce_sort_calmd_stream_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                                 int32_t n_ref, int32_t last, uint64_t est_bytes, double *calmd_s, int (*flush)(void *ctx, uint64_t n), void *ctx);
int gce_sort_calmd_consume(gce_sort *b, uint64_t n);
int gce_sort_calmd_stream_stats(gce_sort *b, int32_t *n_flushes, uint64_t *resident_cap_bytes, uint64_t *flushed_bytes);

// ---- the UMI of every record into an MI:Z field, on calmd's streamed output (gce_umi.hpp)
int gce_sort_umi_begin(gce_sort *b, int32_t codes, uint64_t piece_bytes, uint64_t resident_bytes, const char *source);
int gce_sort_umi_window(gce_sort *b, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, uint64_t est_bytes, double *umi_s, int (*flush)(void *ctx, uint64_t n), void *ctx);
int gce_sort_umi_finish(gce_sort *b, int32_t codes, uint64_t piece_bytes, int64_t counts[5], uint64_t *in_bytes, uint64_t *out_bytes);

// ---- bases per strand at BED targets (gce_pileup.hpp)
int gce_pileup_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_pileup **out);
void gce_pileup_destroy(gce_pileup *p);
const char *gce_pileup_error(gce_pileup *p);
int gce_pileup_set_sites(gce_pileup *p, int32_t n_ref, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, const uint32_t *site0);
int gce_pileup_window(gce_pileup *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                      int32_t n_ref, int32_t last, double *pileup_s);
int gce_pileup_finish(gce_pileup *p, int64_t counters[8], uint32_t *counts_out);

// ---- the same table with every fragment counted once where its mates overlap (gce_fragpile.hpp)
int gce_fragpile_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_fragpile **out);
void gce_fragpile_destroy(gce_fragpile *p);
const char *gce_fragpile_error(gce_fragpile *p);
int gce_fragpile_set_sites(gce_fragpile *p, int32_t n_ref, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end, const uint32_t *site0);
int gce_fragpile_window(gce_fragpile *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                        int32_t n_ref, int32_t last, double *pileup_s);
int gce_fragpile_finish(gce_fragpile *p, int64_t counters[13], uint32_t *counts_out);

// ---- mismatches by read cycle against the reference (gce_errprof.hpp)
int gce_errprof_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_errprof **out);
void gce_errprof_destroy(gce_errprof *p);
const char *gce_errprof_error(gce_errprof *p);
int gce_errprof_set_ref(gce_errprof *p, int32_t n_ref, const char *const *seq, const int64_t *len);
int gce_errprof_set_sites(gce_errprof *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end);
int gce_errprof_set_mask(gce_errprof *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end);   /* gce_varmask.hpp; DESIGN.md 4m */
int gce_errprof_window(gce_errprof *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                       int32_t n_ref, int32_t last, double *errprof_s);
int gce_errprof_finish(gce_errprof *p, int64_t counters[10], uint64_t *counts_out);

// ---- the same table with every fragment counted once where its mates overlap, and the overlap table (gce_fragerr.hpp)
int gce_fragerr_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_fragerr **out);
void gce_fragerr_destroy(gce_fragerr *p);
const char *gce_fragerr_error(gce_fragerr *p);
int gce_fragerr_set_ref(gce_fragerr *p, int32_t n_ref, const char *const *seq, const int64_t *len);
int gce_fragerr_set_sites(gce_fragerr *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end);
int gce_fragerr_set_mask(gce_fragerr *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end);
int gce_fragerr_window(gce_fragerr *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                       int32_t n_ref, int32_t last, double *errprof_s);
int gce_fragerr_finish(gce_fragerr *p, int64_t counters[15], uint64_t *counts_out, uint64_t *overlap_out);

// ---- the error profile by consensus support, the FR / RR tags (gce_errsup.hpp)
int gce_errsup_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, const char *tags, gce_errsup **out);
void gce_errsup_destroy(gce_errsup *p);
const char *gce_errsup_error(gce_errsup *p);
int gce_errsup_set_ref(gce_errsup *p, int32_t n_ref, const char *const *seq, const int64_t *len);
int gce_errsup_set_mask(gce_errsup *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end);
int gce_errsup_set_sites(gce_errsup *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end);
int gce_errsup_window(gce_errsup *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                      int32_t n_ref, int32_t last, double *errprof_s);
int gce_errsup_finish(gce_errsup *p, int64_t counters[11], uint64_t *counts_out);

// ---- the error profile by reported base quality (gce_errqual.hpp)
int gce_errqual_create(int32_t device, size_t device_budget_bytes, int32_t min_mapq, int32_t min_baseq, uint32_t exclude_flags, uint32_t options, gce_errqual **out);
void gce_errqual_destroy(gce_errqual *p);
const char *gce_errqual_error(gce_errqual *p);
int gce_errqual_set_ref(gce_errqual *p, int32_t n_ref, const char *const *seq, const int64_t *len);
int gce_errqual_set_mask(gce_errqual *p, int64_t n, const int32_t *tid, const int32_t *start, const int32_t *end);
int gce_errqual_set_sites(gce_errqual *p, int64_t n_intervals, const int32_t *tid, const int32_t *start, const int32_t *end);
int gce_errqual_window(gce_errqual *p, const void *comp, size_t comp_bytes, int32_t n_members, const uint64_t *coff, const uint32_t *csize, const uint32_t *usize, uint64_t skip,
                       int32_t n_ref, int32_t last, double *errprof_s);
int gce_errqual_finish(gce_errqual *p, int64_t counters[10], uint64_t *counts_out);

// ---- the QUAL bytes of overlapping mates rewritten in the resident records of gce_sort_window (gce_ovlmerge.hpp)
int gce_sort_overlap_begin(gce_sort *b);
int gce_sort_overlap_finish(gce_sort *b, int32_t min_mapq, uint32_t exclude_flags, uint32_t options, int32_t codes, uint64_t piece_bytes, int64_t counts[8], int64_t *bad_rec,
                            uint64_t *out_bytes);

}  // extern "C"
#endif
