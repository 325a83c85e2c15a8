/*
 * cont2_amd_rig.h -- a rig's sensors de-skewed, filtered and joined in ONE sweep: an extension of cont2_amd.h's C-ABI.
 *
 * cc_ingest_segments joins several buffers into one scan, cc_ingest_points_motion de-skews a sweep by its per-point time words and
 * cc_ingest_points_filtered drops records by a word of their own -- each alone.  A deployed front end does all three to every key
 * frame: a vehicle with two or three LiDARs de-skews each sweep by ITS time words, drops the segmentation's moving classes or the
 * driver's noise tag, moves every sensor by its extrinsics and builds one bird's-eye view.  The calls below take all the steps at
 * once, while the rasteriser loads the records where they lie.  No reference counterpart.
 *
 * A scan is an ordered list of 1 .. CC_RIG_SEG_MAX segments, as in cc_ingest_segments.  A segment carries
 *   - points, n_points, layout: cc_point_segment_t's fields, with its rules ({0, 0} stands for {16, 0}; n_points may be 0);
 *   - a MODE:
 *       CC_RIG_NONE    the identity on the bits;
 *       CC_RIG_TF      tf[12]: the operation cc_ingest_points documents for h_tf;
 *       CC_RIG_MOTION  time_offset, time_type (CC_TIME_F32 / CC_TIME_U32), t_begin (CC_TIME_U32: the u32's bits), scale, knot0,
 *                      n_knots: the record is moved by knot  knot0 + b  of ITS SCAN's knot pool, b computed by steps 1 - 2 of
 *                      cc_ingest_points_motion with K replaced by the segment's n_knots -- so the bin is clamped to the segment's
 *                      slice [knot0, knot0 + n_knots) of the pool, not to the pool;
 *   - a FILTER OFFSET: the byte offset of that segment's filter word inside its records, or -1: the segment is not filtered.
 * A call brings
 *   - one KNOT POOL per scan, h_knots [n_scans][n_pool][12] f32, 1 <= n_pool <= CC_MOTION_KNOTS_MAX, the same n_pool for every scan
 *     of the call: two sensors with 32 knots each, or four sweeps with 16 each, share the 64.  h_knots may be NULL (n_pool is not
 *     read then) only if no segment is in motion mode;
 *   - one FILTER RULE for all its segments: a cc_point_filter_t (cont2_amd_filter.h) whose `offset` field is not read -- sensors
 *     differ in where the word sits, not in what the classes mean.  It may be NULL only if every segment's filter offset is -1.
 *
 * The scan's result -- descriptor, bev, pix_rc, labels, every byte -- is what cc_ingest_batch returns for
 *     Q = M_0(segment 0) ++ M_1(segment 1) ++ ...
 * where M_s moves each record by its segment's mode and then replaces x by a quiet NaN if the rule drops the record.  So: the
 * filter looks at the record, not at the moved point; among equal heights in a cell the first KEPT record of Q wins, whichever
 * segment it is in; the limits on a scan (more than 10 points, fewer than 2^21) count RECORDS; a scan that keeps nothing is a valid
 * empty scan.  Everything else -- chunks of max_batch_scans, the debug outputs, cc_profile_enable, stream ordering, the ingest lock,
 * CC_ECAPACITY from the host call -- is cc_ingest_segments'.
 *
 * Every call refuses with CC_EINVAL, naming the entry point and the cause in cc_last_error, before anything is queued or read, and
 * the context is usable afterwards: everything cc_ingest_segments, cc_ingest_points_motion and cc_ingest_points_filtered refuse,
 * per segment (the time and filter rules against the segment's own layout: a word that overlaps x, y, z, a word the record has
 * no room for); an unknown mode; a slice outside the pool; a motion segment without a pool; a filtered segment without a rule;
 * a filter offset below -1; more than CC_RIG_SEG_MAX segments in a scan.
 *
 * Out of scope: a rule per segment or per scan; more than one filter word; interpolation between knots; range images or typed
 * coordinate streams as segments; 64-bit times.
 *
 * What the kernels cost next to the single-step calls': DESIGN.md 3.0.
 */
#ifndef CONT2_AMD_RIG_H
#define CONT2_AMD_RIG_H

#include "cont2_amd.h"
#include "cont2_amd_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fewer than CC_SEG_MAX: the scan's table shares the rasteriser's spare LDS with the knot pool and the class table. */
#define CC_RIG_SEG_MAX 16
enum { CC_RIG_NONE = 0, CC_RIG_TF = 1, CC_RIG_MOTION = 2 };
typedef struct {
  const void *points;       /* first record of the segment (device or host pointer, see the call) */
  int64_t n_points;
  cc_point_layout_t layout; /* {0, 0} stands for {16, 0} */
  int32_t mode;             /* CC_RIG_* */
  int32_t filter_offset;    /* byte offset of the filter word inside a record, a multiple of the word's size; -1: not filtered */
  float tf[12];             /* CC_RIG_TF: row-major 3 x 4 */
  int32_t time_offset;      /* CC_RIG_MOTION: byte offset of the time word inside a record */
  int32_t time_type;        /*   CC_TIME_F32 / CC_TIME_U32 */
  float t_begin, scale;     /*   (CC_TIME_U32: t_begin holds the u32's bits) */
  int32_t knot0, n_knots;   /*   the segment's slice of its scan's pool */
} cc_rig_segment_t;         /* 104 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_rig_segment_t) == 104 && offsetof(cc_rig_segment_t, tf) == 32 && offsetof(cc_rig_segment_t, time_offset) == 80,
              "cc_rig_segment_t: 104 bytes, tf at 32, time_offset at 80");
#else
_Static_assert(sizeof(cc_rig_segment_t) == 104 && offsetof(cc_rig_segment_t, tf) == 32 && offsetof(cc_rig_segment_t, time_offset) == 80,
               "cc_rig_segment_t: 104 bytes, tf at 32, time_offset at 80");
#endif

/* scan i = the segments h_segs[h_scan_segs[i] .. h_scan_segs[i + 1]); `points` are DEVICE pointers, read in place.  h_segs,
 * h_scan_segs, h_knots and the filter's table are copied before the call returns.  Queues work on `stream` like cc_ingest_segments. */
int cc_ingest_rig(cc_ctx *ctx, const cc_rig_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, const float *h_knots, int n_pool,
                  const cc_point_filter_t *filter, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream);
/* The same from HOST records (whole records, one staging pass; results copied back; h_bev may be NULL). */
int cc_ingest_rig_host(cc_ctx *ctx, const cc_rig_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, const float *h_knots, int n_pool,
                       const cc_point_filter_t *filter, cc_scan_desc_t *h_out, float *h_bev);
/* ONE scan made of n_segs host segments: the per-scan handle of the online loop (what the class mirror uses).  h_knots: [n_pool][12]. */
int cc_scan_ingest_rig(cc_ctx *ctx, const cc_rig_segment_t *h_segs, int n_segs, const float *h_knots, int n_pool, const cc_point_filter_t *filter,
                       int want_bev, cc_scan **out);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_RIG_H */
