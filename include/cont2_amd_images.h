/*
 * cont2_amd_images.h -- descriptors from caller-made max-height images: an extension of cont2_amd.h's C-ABI.
 *
 * Every ingest call of cont2_amd.h takes points and rasterises them into the n_row x n_col max-height image the contour kernel
 * reads.  A caller that already holds that image -- an elevation-mapping stack on the same GPU, a back end that keeps a fused local
 * height map per key frame, a radar or depth-camera front end, a map server that stored the 90 KB image of a key frame instead of
 * its cloud, the reference's own ContourManager (bev_pixfs_ / resumeImage / getBevImage, contour_mng.h:558-586) -- hands it over
 * here.  No point is read and nothing is rasterised: one small kernel lists the image's active cells, and everything behind that
 * list is what it is for points.
 *
 * Per scan the caller gives
 *   height     : n_row * n_col f32, row-major, cell = row * n_col + col: cc_ingest_debug_t.d_bev's layout.  The values are IMAGE
 *                heights -- what the reference's bev_ holds, z + lidar_height_; lidar_height is NOT applied.
 *   pos_rc     : optional, n_row * n_col pairs of f32 (row_f, col_f): d_pix_rc's layout, pointToContRowCol's frame.  NULL stands
 *                for the cell centres ((float)row, (float)col) -- what pointToContRowCol gives for the middle of a cell.
 *   min_height : optional, ONE f32 per scan in host memory, copied before the call returns (as h_tf is).  It becomes min_bin_val:
 *                the rasteriser's value is the minimum over all accepted points, which an image cannot tell.  NULL stands for the
 *                minimum over the occupied cells.  Copied as given, not checked.
 *
 * Rules -- chosen so that the contour kernel only ever sees inputs the rasteriser itself could have produced:
 *   - a cell is OCCUPIED iff row >= 1 and h > -1000 (VAL_ABS_INF_).  NaN is empty.  Row 0 is empty whatever it holds: makeBEV
 *     never fills it (rc.first > 0, contour_mng.h:515).  +inf is taken as given.
 *   - a position component that is NaN or outside [row - 0.5, row + 0.5] (the column likewise) is replaced by the cell centre's
 *     component, per component.  The rasteriser's own positions always lie inside that closed interval, so the clamp never fires
 *     on them; without it a wild position would reach the key phase's window arithmetic.  Positions of empty cells are never read.
 *   - max_bin_val is the maximum over the occupied cells (the rasteriser's value: a cell's height is the maximum of its points),
 *     n_pix their number.  A scan without an occupied cell gets what cc_ingest_batch writes for a cloud whose points are all
 *     rejected: max_bin_val = -1000, min_bin_val = +1000 (or min_height, when given), and zero contours.  It is a valid scan.
 *   - no blind-zone test, no "more than 10 points" rule, no transform: the image is the caller's.
 *   - behind the list everything is as for points: the three bodies of the contour kernel, the CC_DESC_* flags and CC_ECAPACITY
 *     from the host calls; the debug outputs (d_bev: the image as the library read it -- empties written as -1000, row 0
 *     cleared; d_pix_rc: -1 everywhere but the occupied cells, which hold their positions after the clamp; d_labels as before);
 *     cc_profile_enable, whose first slot times the listing kernel; stream ordering; chunks of max_batch_scans; the ingest lock.
 *
 * The defining property: for any cloud X, let cc_ingest_batch(X) with debug outputs give (desc, bev, pix_rc); then
 * cc_ingest_images(bev, pix_rc, min_height = desc.min_bin_val) returns desc byte for byte, and the same label images.
 *
 * Every call refuses with CC_EINVAL, naming the cause in cc_last_error, before anything is queued: a NULL ctx, height or out;
 * n_scans < 0; a misaligned device base.  n_scans == 0 is CC_OK.
 */
#ifndef CONT2_AMD_IMAGES_H
#define CONT2_AMD_IMAGES_H

#include "cont2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device images; d_height 16-byte aligned, d_pos_rc 8-byte aligned or NULL (CC_EINVAL otherwise, nothing queued) */
int cc_ingest_images(cc_ctx *ctx, const float *d_height, const float *d_pos_rc, int n_scans, const float *h_min_height,
                     cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream);
/* host images (cc_ingest_host_bev's shape: one H2D copy, results copied back; h_bev may be NULL; no alignment asked) */
int cc_ingest_images_host(cc_ctx *ctx, const float *h_height, const float *h_pos_rc, int n_scans, const float *h_min_height,
                          cc_scan_desc_t *h_out, float *h_bev);
/* the per-scan handle of the online loop (what the class mirror uses); h_min_height: one value or NULL */
int cc_scan_ingest_image(cc_ctx *ctx, const float *h_height, const float *h_pos_rc, const float *h_min_height, int want_bev,
                         cc_scan **out);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_IMAGES_H */
