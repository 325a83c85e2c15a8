/*
 * cont2_amd_coords.h -- ingest of f64, scaled-i32 and split-stream coordinates, read in place: an extension of cont2_amd.h's C-ABI.
 *
 * cc_ingest_points reads three consecutive f32 per record.  Three kinds of caller have something else: f64 clouds (numpy, Open3D, PCD
 * files with double fields, everything in a georeferenced frame such as UTM), survey and prior maps in scaled integers (the LAS
 * convention: int32 X, Y, Z with a scale and an offset), and coordinates held as separate streams (three column arrays of a dataframe,
 * a strided view of a wider array, x, y, z that are not neighbours inside the record).  All of them ran a pass of their own first:
 * cast, subtract an origin, pack, write a second copy of the cloud.  For georeferenced data that pass is also easy to get wrong: an f32
 * has 0.5 m of resolution at a UTM northing of 5.4e6 m, so the origin must be subtracted in f64 BEFORE the narrowing.  The calls below
 * read the coordinates where they lie and do exactly that per point while they rasterise.
 *
 * Specification.  Offsets are in points.  Coordinate k in {x, y, z} of point j of scan i is the element at
 *     stream_k + (h_offsets[i] + j) * stride_bytes
 * and it becomes an f32 by exactly these steps:
 *   1. X = (double)v for CC_COORD_F32 and CC_COORD_F64.  For CC_COORD_I32, X = (double)v * scale[k]: one f64 product, rounded once.
 *   2. D = X - origin[i][k]: one f64 subtraction, rounded once.  With h_origin NULL the origin is 0.0.
 *   3. p = (float)D: IEEE round to nearest even.  Overflow gives +-inf.  The library keeps f32 subnormals.
 * No fused multiply-add is used anywhere in these steps.
 *
 * Result.  Every byte of the descriptors, bev, pix_rc and labels equals what cc_ingest_points returns for the packed {12, 0} records
 * (p_x, p_y, p_z), with the same offsets and the same h_tf.  So: the tie rule still counts a point's index; NaN and out-of-range points
 * are rejected as always; the matrix sees p; the limits on a scan (more than 10 points, fewer than 2^21) count points.  A CC_COORD_F32
 * source with consecutive x, y, z and no origin gives the bytes of cc_ingest_points with that {stride, offset} layout.  Everything
 * else -- chunks of max_batch_scans, the debug outputs, cc_profile_enable, stream ordering, the ingest lock, CC_ECAPACITY from the host
 * call -- is cc_ingest_points'.  h_origin ([n_scans][3] doubles) and h_tf are copied before the call returns.
 *
 * Every call refuses with CC_EINVAL, naming the cause in cc_last_error, before anything is queued or read, and the context is usable
 * afterwards: a NULL src or a NULL stream pointer; an unknown type; a stride_bytes that is not a multiple of the element size
 * (4 / 8 / 4), below it, or above CC_POINT_STRIDE_MAX; a stream pointer not aligned to the element size; a non-finite scale[k] with
 * CC_COORD_I32; a non-finite origin component; whatever cc_ingest_points refuses about offsets and scan sizes.
 *
 * The host forms (cc_ingest_coords_host, cc_scan_ingest_coords) copy exactly the bytes the streams span.  If the highest stream pointer
 * plus one element lies within stride_bytes of the lowest, the streams are one record array: one copy, from the lowest pointer, of
 * (points - 1) * stride_bytes + (highest - lowest) + element bytes.  Otherwise three copies of (points - 1) * stride_bytes + element
 * bytes each.
 *
 * Out of scope: typed coordinates in segments, with per-point motion, with a filter, or in range images; f16, i16 or u16 and 64-bit
 * integers; a type or a stride per axis; an unaligned element (LAS point formats whose record length is not a multiple of 4); a scale
 * per scan.
 *
 * What the kernels cost next to cc_ingest_points': DESIGN.md 3.0.
 */
#ifndef CONT2_AMD_COORDS_H
#define CONT2_AMD_COORDS_H

#include "cont2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CC_COORD_F32 = 0, CC_COORD_F64 = 1, CC_COORD_I32 = 2 };
typedef struct {
  const void *x, *y, *z; /* the first point's x, y and z: three streams, which may lie inside one record array or in three arrays */
  int32_t type;          /* CC_COORD_*: one element type for all three */
  int32_t stride_bytes;  /* between consecutive points, the same for all three streams */
  double scale[3];       /* CC_COORD_I32 only; not read otherwise */
} cc_coord_src_t;        /* 56 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_coord_src_t) == 56 && offsetof(cc_coord_src_t, type) == 24 && offsetof(cc_coord_src_t, stride_bytes) == 28 &&
                  offsetof(cc_coord_src_t, scale) == 32,
              "cc_coord_src_t: 56 bytes, type at 24, stride_bytes at 28, scale at 32");
#else
_Static_assert(sizeof(cc_coord_src_t) == 56 && offsetof(cc_coord_src_t, type) == 24 && offsetof(cc_coord_src_t, stride_bytes) == 28 &&
                   offsetof(cc_coord_src_t, scale) == 32,
               "cc_coord_src_t: 56 bytes, type at 24, stride_bytes at 28, scale at 32");
#endif

/* cc_ingest_points for typed coordinate streams: device streams, read in place */
int cc_ingest_coords(cc_ctx *ctx, const cc_coord_src_t *src, const int64_t *h_offsets, int n_scans, const double *h_origin,
                     const float *h_tf, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream);
/* cc_ingest_points_host for them: host streams (one copy or three, results copied back; h_bev may be NULL) */
int cc_ingest_coords_host(cc_ctx *ctx, const cc_coord_src_t *src, const int64_t *h_offsets, int n_scans, const double *h_origin,
                          const float *h_tf, cc_scan_desc_t *h_out, float *h_bev);
/* cc_scan_ingest_points for them: the per-scan handle of the online loop (what the class mirror uses); origin: 3 doubles or NULL */
int cc_scan_ingest_coords(cc_ctx *ctx, const cc_coord_src_t *src, int64_t n_points, const double *origin, const float *h_tf,
                          int want_bev, cc_scan **out);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_COORDS_H */
