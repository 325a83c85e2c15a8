/*
 * cont2_amd_filter.h -- ingest that drops points by a per-record label, ring or intensity word: an extension of cont2_amd.h's C-ABI.
 *
 * Nearly every LiDAR place-recognition front end throws points away before it builds the bird's-eye view: the moving-object
 * classes of a semantic segmentation (SemanticKITTI's .label word: class in the low 16 bits, 252-259 the moving ones), a driver's
 * "invalid / noise" tag byte, a subset of rings, an intensity band.  The word lies inside the record the driver delivers, and
 * cc_point_layout_t already lets the rasteriser step over it.  The calls below read it where it lies, so the caller no longer
 * compacts the cloud (mask, gather, a second copy) before it ingests it.
 *
 * A call names ONE filter word inside every record and a rule that says which records are kept.  The result is, byte for byte,
 *   - what cc_ingest_points returns for the same records with the x of every DROPPED record replaced by a quiet NaN,
 *   - and therefore what it returns for the kept records alone, in their original order, whenever more than 10 are kept.
 * So: among equal heights in a cell the first KEPT record in file order wins; the blind zone, the border, max / min height, n_pix
 * and the continuous positions see kept points only; a dropped record that would have owned a cell hands it to the next-best kept
 * one; the limits on a scan (more than 10 points, fewer than 2^21) count RECORDS, not kept points; a scan whose records are all
 * dropped yields the descriptor the all-NaN cloud yields.  The optional per-scan matrix h_tf works as in cc_ingest_points; the
 * filter looks at the record, not at the moved point.  Everything else -- layouts, chunks of max_batch_scans, the debug outputs,
 * cc_profile_enable, stream ordering, the ingest lock, CC_ECAPACITY from the host call -- is cc_ingest_points'.
 *
 * Class rule (type CC_FILTER_U8 / _U16 / _U32; the word is little-endian, at a multiple of its size inside the record):
 *     class = (word >> shift) & mask
 *     kept iff  class < n_classes ? bit (class & 31) of keep_bits[class >> 5] : keep_other
 *   1 <= n_classes <= CC_FILTER_CLASSES_MAX; keep_bits holds (n_classes + 31) / 32 host words, copied before the call returns; one
 *   table per call, for all its scans.  SemanticKITTI: {offset 12, CC_FILTER_U32, shift 0, mask 0xFFFF, n_classes 260, keep_other 1}
 *   with bits 252 .. 259 clear -- the instance id in the high 16 bits never reaches the table.
 * Range rule (type CC_FILTER_F32):
 *     kept iff  lo <= v && v <= hi
 *   A NaN v fails both compares and is dropped; lo or hi may be infinite (-inf, +inf keeps every non-NaN value); -0.0 equals 0.0.
 *
 * Every call refuses with CC_EINVAL, naming the cause in cc_last_error, before anything is queued or read, and the context is
 * usable afterwards: a layout cc_ingest_points refuses; a NULL filter; an unknown type; an offset that is negative, not a multiple
 * of the word's size, or with offset + size > stride_bytes; a word that overlaps the 12 bytes of x, y, z; a shift that is negative
 * or not below the word's bit width; n_classes outside 1 .. CC_FILTER_CLASSES_MAX; a NULL keep_bits with an integer type; a NaN lo
 * or hi.  The fields of the other rule are not read.
 *
 * A filter together with segments or per-point motion is cont2_amd_rig.h's (cc_ingest_rig: one rule, a word offset per segment).
 * Out of scope: a filter together with range images; a table per scan; 64-bit or f64 words; more than one word per call; filtering
 * on the MOVED coordinates (the border and blind-zone tests already do that).
 *
 * What the kernels cost next to cc_ingest_points': DESIGN.md 3.0.
 */
#ifndef CONT2_AMD_FILTER_H
#define CONT2_AMD_FILTER_H

#include "cont2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CC_FILTER_CLASSES_MAX 4096
enum { CC_FILTER_U8 = 0, CC_FILTER_U16 = 1, CC_FILTER_U32 = 2, CC_FILTER_F32 = 3 };
typedef struct {
  int32_t offset;            /* byte offset of the word inside a record, a multiple of the word's size */
  int32_t type;              /* CC_FILTER_* */
  int32_t shift;             /* integer types: class = (word >> shift) & mask */
  uint32_t mask;
  int32_t n_classes;         /* integer types: bits in keep_bits */
  int32_t keep_other;        /* integer types: a class >= n_classes is kept (non-zero) or dropped (0) */
  float lo, hi;              /* CC_FILTER_F32: kept iff lo <= v && v <= hi */
  const uint32_t *keep_bits; /* host; integer types only */
} cc_point_filter_t;         /* 40 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_point_filter_t) == 40 && offsetof(cc_point_filter_t, lo) == 24 && offsetof(cc_point_filter_t, keep_bits) == 32,
              "cc_point_filter_t: 40 bytes, lo at 24, keep_bits at 32");
#else
_Static_assert(sizeof(cc_point_filter_t) == 40 && offsetof(cc_point_filter_t, lo) == 24 && offsetof(cc_point_filter_t, keep_bits) == 32,
               "cc_point_filter_t: 40 bytes, lo at 24, keep_bits at 32");
#endif

/* cc_ingest_points with a filter: device records, read in place */
int cc_ingest_points_filtered(cc_ctx *ctx, const void *d_points, const cc_point_layout_t *layout, const cc_point_filter_t *filter,
                              const int64_t *h_offsets, int n_scans, const float *h_tf, cc_scan_desc_t *d_out,
                              const cc_ingest_debug_t *dbg, void *stream);
/* cc_ingest_points_host with a filter: host records (one H2D copy, results copied back; h_bev may be NULL) */
int cc_ingest_points_filtered_host(cc_ctx *ctx, const void *h_points, const cc_point_layout_t *layout, const cc_point_filter_t *filter,
                                   const int64_t *h_offsets, int n_scans, const float *h_tf, cc_scan_desc_t *h_out, float *h_bev);
/* cc_scan_ingest_points with a filter: the per-scan handle of the online loop (what the class mirror uses) */
int cc_scan_ingest_points_filtered(cc_ctx *ctx, const void *h_points, const cc_point_layout_t *layout, const cc_point_filter_t *filter,
                                   int64_t n_points, const float *h_tf, int want_bev, cc_scan **out);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_FILTER_H */
