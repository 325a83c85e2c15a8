/*
 * cont2_amd.h -- C-ABI of the MI355X-native contour-context hot path.
 *
 * This is the drop-in boundary of the build.  The reference has no
 * FFI layer: its interface is the C++ class API of the `cont2contops` library.  Every entry
 * point below names the reference function(s) it replaces (file:line under the reference
 * tree), and `contour-context_amd/hostcpp/` re-creates the reference classes on top of it.
 *
 * All functions return 0 on success, a negative CC_E* code otherwise; they never abort.
 * Pointers named d_* are device (HBM) pointers, h_* host pointers.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  No torch types cross this boundary.
 *
 * Layout structs (cc_contour_t, cc_bci_t, cc_scan_desc_t ...) are plain-old-data shared by the
 * device kernels, the host mirror and -- for comparison only -- the CPU oracle under oracle/.
 */
#ifndef CONT2_AMD_H
#define CONT2_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- compile-time shape ---- */
#define CC_NLEV 6          /* lv_grads_.size(); both shipped configs use 6 (yaml :30-31)        */
#define CC_KEY_DIM 10      /* RET_KEY_DIM, contour_mng.h:89                                     */
#define CC_NPIV 6          /* piv_firsts_ upper bound (anchors per level), contour_mng.h:107    */
#define CC_NDIST 10        /* dist_firsts_ upper bound, contour_mng.h:108                       */
#define CC_BCI_LAYERS 4    /* NUM_BIN_KEY_LAYER: DIST_BIN_LAYERS = {1,2,3,4}, contour_mng.h:113 */
#define CC_BITS_PER_LAYER 64 /* contour_mng.h:112                                               */
#define CC_BCI_MAXPTS 40   /* 4 layers x 10 neighbours                                          */
#define CC_MAXC 320        /* stored contours per level per scan (sorted, largest first)        */
#define CC_MAX_CELLS 22500 /* n_row_*n_col_ upper bound (150x150), LDS-resident BEV             */
#define CC_NQLEV 3         /* q_levels_.size() upper bound ([1,2,3], yaml :11)                  */
#define CC_KNN_MAX 64      /* nnk_ of the common kernels and d_knn stride up to it (shipped 50) */
#define CC_KNN_MAX_LARGE 256 /* nnk_ upper bound: 64 < nnk_ <= 256 runs the large-k instances  */
#define CC_GMM_LEVELS 4    /* GMMOptConfig::levels_ = {1,2,3,4}, correlation.h:18               */

/* Status codes.  Every entry point returns one; cc_last_error() (thread-local text) explains a non-zero one.
 * CC_EINVAL / CC_ECAPACITY leave the handle's state unchanged: it stays usable.  CC_EHIP means a HIP runtime
 * call failed part-way: destroy the handle (cc_db_destroy / cc_destroy release everything that was allocated).
 * Threading follows the reference (none): a cc_ctx and the cc_db objects created from it are to be
 * driven by one host thread at a time; different contexts (one per GPU / process) are independent. */
enum {
  CC_OK = 0,
  CC_EINVAL = -1,   /* bad argument / unsupported configuration            */
  CC_EHIP = -2,     /* a HIP runtime call failed (see cc_last_error)       */
  CC_ENOMEM = -3,
  CC_ECAPACITY = -4 /* a fixed capacity (DB size, batch size) was exceeded */
};

/* ------------------------------------------------------------------------- configs ------ */
/* ContourManagerConfig (contour_mng.h:92-110) + ContourViewStatConfig (contour.h:32-37). */
typedef struct {
  float lv_grads[CC_NLEV];
  float reso_row, reso_col;
  int32_t n_row, n_col;
  float lidar_height;
  float blind_sq;
  int32_t min_cont_key_cnt;
  int32_t min_cont_cell_cnt;
  int32_t piv_firsts;
  int32_t dist_firsts;
  float roi_radius;
  /* ContourViewStatConfig */
  int32_t min_cell_cov;
  float point_sigma;
  float com_bias_thres;
} cc_manager_cfg_t;

/* ContourSimThresConfig (contour.h:40-45). */
typedef struct {
  float ta_cell_cnt, tp_cell_cnt, tp_eigval, ta_h_bar, ta_rcom, tp_rcom;
} cc_sim_cfg_t;

/* CandidateScoreEnsemble (contour_db.h:244-250) = the three score unions
 * (contour_mng.h:121-219) flattened. */
typedef struct {
  int32_t i_ovlp_sum, i_ovlp_max_one, i_in_ang_rng; /* ScoreConstellSim */
  int32_t i_indiv_sim, i_orie_sim;                  /* ScorePairwiseSim */
  float correlation, area_perc, neg_est_dist;       /* ScorePostProc    */
} cc_score_t;

/* ContourDBConfig (contour_db.h:658-669) + TreeBucketConfig (:54-57). */
typedef struct {
  int32_t nnk;
  int32_t max_fine_opt;
  int32_t n_q_levels;
  int32_t q_levels[CC_NQLEV];
  cc_sim_cfg_t cont_sim;
  double max_elapse, min_elapse;
} cc_db_cfg_t;

void cc_default_manager_cfg(cc_manager_cfg_t *cfg); /* shipped KITTI values, yaml :27-47 */
void cc_default_db_cfg(cc_db_cfg_t *cfg);           /* yaml :6-23                        */
void cc_default_thresholds(cc_score_t *lb, cc_score_t *ub); /* yaml :69-87              */

/* ------------------------------------------------------------------ per-scan records ---- */
/* ContourView (contour.h:97-119).  eig_vecs is column-major like Eigen: [v00 v10 v01 v11],
 * column 1 (v01,v11) belongs to the larger eigenvalue. pos_cov likewise column-major. */
typedef struct {
  int16_t level;
  int16_t poi[2];
  int16_t cell_cnt;
  float pos_mean[2];
  float pos_cov[4];
  float eig_vals[2];
  float eig_vecs[4];
  float eccen;
  float vol3_mean;
  float com[2];
  uint8_t ecc_feat;
  uint8_t com_feat;
  uint8_t pad_[2];
} cc_contour_t; /* 76 bytes */

/* BCI::RelativePoint (contour_mng.h:245-258). */
typedef struct {
  int8_t level;
  int8_t seq;
  int16_t bit_pos;
  float r;
  float theta;
} cc_relpt_t; /* 12 bytes */

/* BCI (contour_mng.h:243-281).  dist_bin word w bit b  <=>  std::bitset bit 64*w+b.
 * n_segs = nei_idx_segs_.size() (0 when nei_pts_ is empty, else #distinct bit_pos + 1). */
typedef struct {
  uint64_t dist_bin[CC_BCI_LAYERS];
  int8_t piv_seq;
  int8_t level;
  uint8_t n_pts;
  uint8_t n_segs;
  uint16_t segs[CC_BCI_MAXPTS + 2];
  cc_relpt_t pts[CC_BCI_MAXPTS];
} cc_bci_t; /* 32 + 4 + 84 + 480 = 600 bytes */

/* Everything ContourManager keeps after makeContoursRecurs() + clearImage()
 * (contour_mng.h:426-436): sorted contour tables, per-level totals, 36 keys, 36 BCIs.
 * cont_perc_[l][j] is not stored: it is cell_cnt * 1.0f / layer_cell_cnt[l]
 * (contour_mng.h:607) and is recomputed bit-identically where needed. */
/* Descriptor flags.  The reference has no capacities; this build STORES at most CC_MAXC contours per level (only the
 * first piv_firsts_/dist_firsts_ and the largest ~95 % of the area are ever read downstream) and handles any number:
 * a scan with more than CC_MAXC components on a level is redone by an exact slow path (cc_k_contours_big: up to 3 840
 * per level, more than a 150 x 150 image can hold) behind the same call.
 *   CC_DESC_TRUNCATED          : a level has more than CC_MAXC contours, the CC_MAXC largest are stored in std::sort's
 *                                order; everything in the descriptor is exact (the oracle sets the same bit)
 *   CC_DESC_INEXACT_COMPONENTS : not produced any more (rounds 1-4: more than CC_MAXC components on a level); it stands
 *                                in a descriptor only between the fast launch and the slow one of the same call
 *   CC_DESC_INEXACT_KEYS       : a retrieval-key RoI held more cells than the kernel's list (roi_radius_ > 10 on a
 *                                densely built image): the keys are NOT exact
 * cc_ingest_host returns CC_ECAPACITY for CC_DESC_INEXACT_*; callers of cc_ingest_batch (device output) check `flags`
 * themselves.  KITTI/MulRan-like scans have tens to ~150 contours per level. */
#define CC_DESC_TRUNCATED 1
#define CC_DESC_INEXACT_COMPONENTS 2
#define CC_DESC_INEXACT_KEYS 4
typedef struct {
  int32_t n_cont[CC_NLEV];         /* cont_views_[l].size() (true count)                  */
  int32_t n_stored[CC_NLEV];       /* min(n_cont, CC_MAXC)                                */
  int32_t layer_cell_cnt[CC_NLEV]; /* layer_cell_cnt_                                     */
  float max_bin_val, min_bin_val;  /* contour_mng.h:436,524-525                           */
  int32_t n_pix;                   /* bev_pixfs_.size()                                   */
  int32_t flags;                   /* CC_DESC_* bits below; 0 = exact                     */
  float keys[CC_NLEV][CC_NPIV][CC_KEY_DIM];
  cc_bci_t bcis[CC_NLEV][CC_NPIV];
  cc_contour_t cont[CC_NLEV][CC_MAXC];
} cc_scan_desc_t;

/* The part of a scan's descriptor that the query path reads of a DATABASE scan (and of the query scan itself):
 * retrieval keys, the first dist_firsts_ contours and the BCIs of levels 1..4 (DIST_BIN_LAYERS = q_levels_' range =
 * GMMOptConfig::levels_, contour_mng.h:113, correlation.h:18).  18 KB instead of 169 KB: this is what the DB keeps
 * resident per scan (next to the correlation inputs, cc_gmm_feat), and -- together with them -- the wire format of the
 * multi-GPU exchange (cc_pack_scans / cc_db_add_packed).  hot.X[l] = desc.X[l + 1]. */
#define CC_HOT_LEVELS 4
typedef struct {
  int32_t n_cont[CC_HOT_LEVELS];
  int32_t layer_cell_cnt[CC_HOT_LEVELS];
  int32_t flags;
  int32_t pad_[3];
  float keys[CC_HOT_LEVELS][CC_NPIV][CC_KEY_DIM];
  cc_contour_t cont[CC_HOT_LEVELS][CC_NDIST]; /* rows >= n_stored are zero */
  cc_bci_t bcis[CC_HOT_LEVELS][CC_NPIV];
} cc_hot_desc_t; /* 48 + 960 + 3040 + 14400 = 18448 bytes */

/* Optional parity/debug outputs of ingest (device pointers, any may be NULL):
 *   bev     [n_scans][n_row*n_col] f32  : bev_ image (contour_mng.h:432), -1000 = empty
 *   pix_rc  [n_scans][n_row*n_col][2] f32: continuous (row_f,col_f) of the arg-max point of
 *                                          each occupied cell (Pixelf, contour_mng.h:392-411)
 *   labels  [n_scans][CC_NLEV][n_row*n_col] i16: canonical label image L_l(r,c) = seq of the
 *                                          owning contour after the size sort, -1 = none
 *                                          (SURVEY.md 8(a) "integer contour labels bit-exact")
 * Asking for bev or pix_rc makes the rasteriser write its dense arrays for the call's scans; without them it hands the
 * contour kernel the list of active cells only (and writes the dense arrays just for scans whose active cells overflow
 * that list). */
typedef struct {
  float *d_bev;
  float *d_pix_rc;
  int16_t *d_labels;
} cc_ingest_debug_t;

/* --------------------------------------------------------------------- query records ---- */
/* One KNN hit: IndexOfKey (contour_db.h:59-65) + squared distance. */
typedef struct {
  int32_t gidx; /* index of the scan in the DB (all_bevs_ position)  */
  int16_t level;
  int16_t seq;
  float dist_sq;
} cc_knn_hit_t;

/* Result of one query scan = what queryRangedKNN returns (contour_db.h:698-811) plus the
 * integer gate scores the parity contract compares. */
typedef struct {
  int32_t n_res;        /* 0 or 1 (CHECK(ptr_cands.size() < 2), batch_bin_test.cpp:187)      */
  int32_t cand_gidx;    /* DB index of the matched scan, -1 if none                          */
  double correlation;   /* cand_corr[0]                                                      */
  double tf[3];         /* T_delta = (x, y, theta) in BEV pixel units / radians              */
  int32_t cand_aft_check1, cand_aft_check2, cand_aft_check3; /* contour_db.h:357-359         */
  int32_t n_cand_pose;  /* candidates_.size() before tidyUpCandidates                        */
  int32_t n_cand_tidy;  /* candidates_.size() after tidyUpCandidates                         */
  int32_t n_knn_hits;   /* total KNN results over all query keys                             */
  int32_t flags;        /* CC_QF_* bits; 0 = exact.  Non-zero: an internal capacity was hit while this query was
                           scored (the reference has none), the result may differ from the reference's; the call
                           that collects the query returns CC_ECAPACITY (all results are still delivered)        */
  int32_t pad_;
} cc_query_result_t;
#define CC_QF_CHECK_CAP 1 /* a constellation check had more than 256 potential neighbour pairs (contour_mng.h:311-336)
                             or a rotation window of more than 63 pairs (:344-366): pairs were dropped              */
#define CC_QF_GMM_CAP 2   /* a scan of a correlation problem needs more ellipses of a level than the record holds (CC_MAXC; correlation.h:55-78) */
#define CC_QF_DESC_CAP 4  /* the correlation needed a contour beyond the CC_MAXC stored per level                     */
#define CC_QF_QUERY_INEXACT 8 /* the query scan's own descriptor is flagged CC_DESC_INEXACT_* (it exceeded a capacity of the
                                 contour kernel at ingest)                                                             */

/* ------------------------------------------------------------------------ context ------- */
typedef struct cc_ctx cc_ctx; /* opaque: device id, configs, scratch, streams */
typedef struct cc_db cc_db;   /* opaque: device-resident scan descriptors + key matrices +
                                 the host-side LayerDB bookkeeping                           */

const char *cc_last_error(void);
int cc_version(void);

/* Optional: start the device runtime, load the code object and put n_streams (0..32) streams into the per-device pool that
 * contexts and databases take theirs from.  Measured on MI355X / ROCm 7.2: first HIP call ~54 ms, code object 5-20 ms, a
 * stream 3.4-16 ms (a per-scan driver's context + database use 4-7).  A host that calls this when it starts (the class
 * mirror's ContourDB and evaluator constructors do) keeps those one-off costs out of its first scan.  Not calling it
 * changes nothing but when they are paid. */
int cc_runtime_init(int device, int n_streams);

/* Replaces ContourManager::ContourManager (contour_mng.h:478-498): validates the config
 * (n_row,n_col even, <= 150x150, 6 increasing levels) and allocates per-device scratch. */
int cc_create(int device, const cc_manager_cfg_t *cfg, int max_batch_scans, cc_ctx **out);
int cc_destroy(cc_ctx *ctx);

/* Per-kernel timing with HIP events recorded on the launch stream (bench.py roofline figures).
 * enable: subsequent cc_ingest_batch calls bracket K1 (rasterise) and K2 (contours) with events.
 * read  : synchronises, returns accumulated milliseconds {K1, K2} and the number of launches of
 *         each since the last read, then resets the accumulators. */
int cc_profile_enable(cc_ctx *ctx, int on);
int cc_profile_read(cc_ctx *ctx, double ms_out[2], int *n_launches);

/* ------------------------------------------------------------------------- ingest ------- */
/* Replaces, for a batch of scans, readKITTIPointCloudBin's point stream
 * (tools/pointcloud_util.h:9-47) -> ContourManager::makeBEV (contour_mng.h:505-556) ->
 * makeContoursRecurs (contour_mng.h:588-960, src/cont2/contour_mng.cpp:274-353).
 *   d_xyzi     : [total_points][4] f32 KITTI layout (x,y,z,intensity), device memory
 *   h_offsets  : [n_scans+1] point offsets of each scan into d_xyzi (host memory)
 *   d_out      : [n_scans] cc_scan_desc_t, device memory
 * Scans with <= 10 points violate CHECK_GT(size,10) (contour_mng.h:507) -> CC_EINVAL.
 * d_xyzi should be 16-byte aligned: the float4 kernels load 16-byte records.  A base that is only 4-byte aligned is taken
 * by the record-loader kernels of cc_ingest_points instead (same results, 12-byte loads). */
int cc_ingest_batch(cc_ctx *ctx, const float *d_xyzi, const int64_t *h_offsets, int n_scans,
                    cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream);

/* Same, from a host buffer (one H2D copy, then the device path); result copied back to
 * h_out.  This is what the ContourManager host mirror calls for a single scan. */
int cc_ingest_host(cc_ctx *ctx, const float *h_xyzi, const int64_t *h_offsets, int n_scans,
                   cc_scan_desc_t *h_out);
/* Same, and the max-height images too: h_bev [n_scans][n_row*n_col] f32 (bev_, contour_mng.h:432; -1000 = empty cell) --
 * what ContourManager::getBevImage / getContourImage / saveContourImage / saveMatchedPairImg read
 * (contour_mng.h:573-586, 1039-1049, 1286-1311; the SAVE_MID_FILE artefacts of the drivers).  h_bev may be NULL. */
int cc_ingest_host_bev(cc_ctx *ctx, const float *h_xyzi, const int64_t *h_offsets, int n_scans,
                       cc_scan_desc_t *h_out, float *h_bev);

/* ---- points in the caller's own record shape, with an optional per-scan transform ----
 * The rasteriser reads the records where they lie (no repack pass) and, if asked to, moves every point by a per-scan 3 x 4
 * matrix while it does (sensor extrinsics, roll / pitch compensation: no transformed copy of the cloud).  Everything behind
 * the rasteriser is unchanged.
 *   layout : where the three consecutive f32 (x, y, z) of a point sit.  {16, 0} = KITTI records / PCL PointXYZ,
 *            {12, 0} = packed xyz, {32, 0} = PCL PointXYZI (what each costs is measured in DESIGN.md 3.0),
 *            {48, 8} = some driver's PointCloud2 record, ...  NULL means {16, 0}.
 *            stride_bytes and xyz_offset are multiples of 4, xyz_offset + 12 <= stride_bytes <= CC_POINT_STRIDE_MAX, and the base
 *            pointer is 4-byte aligned (CC_EINVAL otherwise, nothing is queued).  CC_POINT_STRIDE_MAX is 256: PointCloud2
 *            records of the common drivers are 16 to 48 bytes, padded PCL types up to 64, and 2^21 points of 256 bytes keep a
 *            point's byte offset inside its scan below 2^32.  Records that are not 4-byte aligned (22-byte Velodyne
 *            packets), f64 or integer coordinates and structure-of-arrays inputs are not supported.
 *   h_offsets : [n_scans+1], in POINTS: scan i starts h_offsets[i] * stride_bytes bytes behind d_points (with 12-byte records
 *            a scan starts 4-byte aligned, not 16).  The limits on a scan (more than 10 points, fewer than 2^21) count points.
 *   h_tf   : [n_scans][12] f32 host memory, row-major 3 x 4 (m00 m01 m02 m03 | m10 .. | m20 ..), or NULL for none.  Copied
 *            before the call returns.  x' = ((m00*x + m01*y) + m02*z) + m03 in f32, every product and every sum rounded
 *            once, rows 1 and 2 likewise; the matrix is applied as given (not checked to be orthonormal).  Cell, blind-zone
 *            test, height, max / min height and the continuous position of a cell's point all see (x', y', z') only.
 * With layout NULL or {16, 0}, h_tf NULL and a 16-byte aligned d_points the call IS cc_ingest_batch (same kernels).  Like
 * cc_ingest_batch the call only queues work on `stream`; cc_profile_enable brackets its kernels the same way. */
#define CC_POINT_STRIDE_MAX 256
typedef struct {
  int32_t stride_bytes; /* distance between consecutive points */
  int32_t xyz_offset;   /* byte offset of x inside a record; y and z follow */
} cc_point_layout_t;
int cc_ingest_points(cc_ctx *ctx, const void *d_points, const cc_point_layout_t *layout, const int64_t *h_offsets, int n_scans,
                     const float *h_tf, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream);
/* The same from host records (cc_ingest_host_bev's shape: one H2D copy of the records as they are, results copied back;
 * h_bev may be NULL).  The host calls (this one and cc_scan_ingest_points*) copy stride_bytes * points bytes: the buffer must
 * hold WHOLE records up to the end of the last one, also where x, y, z end before the record does.  The host pointer need not
 * be aligned. */
int cc_ingest_points_host(cc_ctx *ctx, const void *h_points, const cc_point_layout_t *layout, const int64_t *h_offsets, int n_scans,
                          const float *h_tf, cc_scan_desc_t *h_out, float *h_bev);

/* ---- a scan from several point SEGMENTS, each with its own record shape and its own transform ----
 * A multi-LiDAR rig (every sensor its own driver, buffer, record shape and extrinsics) or a local submap (the last few sweeps, each
 * with its odometry pose) into ONE max-height image / ONE descriptor, without a pass that transforms and concatenates the
 * clouds first: the rasteriser sweeps the segments where they lie, one after the other.  No reference counterpart.
 * A scan is an ordered list of 1 .. CC_SEG_MAX segments; a segment is n_points records at `points` of layout
 * {stride_bytes, xyz_offset} with an optional row-major 3 x 4 f32 matrix.  The scan's result -- descriptor, bev, pix_rc, labels,
 * every byte -- is the one cc_ingest_batch gives for the cloud
 *     Q = T_0(segment 0) ++ T_1(segment 1) ++ ... ++ T_{S-1}(segment S-1)
 * (++: concatenation in the order given; T_s: the operation cc_ingest_points documents for h_tf, or the identity on the bits for
 * a segment without a matrix).  In particular: among points of equal height in one cell the FIRST point of Q owns the cell,
 * whichever segment it is in -- a segment listed earlier wins over one listed later; max / min height, n_pix, the blind zone
 * and the map's border see the moved points only.
 * Checked before anything is queued or read (CC_EINVAL, the context stays as it was): 1 .. CC_SEG_MAX segments per scan;
 * n_points >= 0 (0: a sensor that dropped a frame; `points` may be NULL then); the scan's TOTAL point count is what the limits
 * on a scan count (more than 10, fewer than 2^21: a point's index within Q has 21 bits); every segment's layout passes
 * cc_ingest_points' rules; every non-empty segment's pointer is non-NULL and 4-byte aligned (the host calls too).
 * What the kernels cost next to cc_ingest_points': DESIGN.md 3.0. */
#define CC_SEG_MAX 32
typedef struct {
  const void *points;       /* first record of the segment (device or host pointer, see the call) */
  int64_t n_points;
  cc_point_layout_t layout; /* {0, 0} stands for {16, 0}, like a NULL layout of cc_ingest_points */
  int32_t has_tf, pad_;
  float tf[12];             /* row-major 3 x 4, read when has_tf != 0 */
} cc_point_segment_t;       /* 80 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_point_segment_t) == 80 && offsetof(cc_point_segment_t, tf) == 32, "cc_point_segment_t: 80 bytes, tf at 32");
#else
_Static_assert(sizeof(cc_point_segment_t) == 80 && offsetof(cc_point_segment_t, tf) == 32, "cc_point_segment_t: 80 bytes, tf at 32");
#endif
/* scan i = the segments h_segs[h_scan_segs[i] .. h_scan_segs[i + 1]); `points` are DEVICE pointers, read in place; the segments
 * of one call may lie in different allocations.  h_segs and h_scan_segs are copied before the call returns.  Queues work on
 * `stream` like cc_ingest_points (calls with more scans than the context's max_batch_scans go in chunks; cc_profile_enable
 * brackets the kernels the same way). */
int cc_ingest_segments(cc_ctx *ctx, const cc_point_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, cc_scan_desc_t *d_out,
                       const cc_ingest_debug_t *dbg, void *stream);
/* The same from HOST records: the segments' records are copied to the device as they are (whole records, one staging pass),
 * results copied back; h_bev may be NULL. */
int cc_ingest_segments_host(cc_ctx *ctx, const cc_point_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, cc_scan_desc_t *h_out,
                            float *h_bev);

/* ---- a sweep de-skewed by per-point time while it is rasterised ----
 * A spinning LiDAR's sweep is recorded over ~0.1 s while the vehicle moves: at 15 m/s and 0.5 rad/s a point at 60 m lands 1.5 - 3 m
 * (several 1 m cells) from where a rigid scan would put it.  Every driver delivers a per-point time (Velodyne `time`: f32 in the
 * PointCloud2 record; Ouster `t`: u32 ns) and the odometry has the poses: these calls move every point by the pose of ITS time bin
 * while the rasteriser loads it -- no pass that gathers a pose per point and writes a second copy of the cloud.  No reference
 * counterpart.  Per scan i the call brings K "knot" matrices (the same K for every scan of the call, 1 <= K <=
 * CC_MOTION_KNOTS_MAX; each row-major 3 x 4 f32 like h_tf) and two numbers t_begin_i, scale_i (bins per time unit, f32).  A point
 * whose time word -- the 4 bytes at time_offset inside its record -- is w:
 *   1. CC_TIME_F32: u = (t - t_begin_i) * scale_i, one f32 subtraction and one f32 multiplication, each rounded once.
 *      CC_TIME_U32: u = (float)(uint32)(w - tb_i) * scale_i; tb_i is the u32 whose BITS are passed in the t_begin slot, the
 *      subtraction wraps modulo 2^32, the conversion rounds to nearest even.
 *   2. b = trunc(min(max(u, 0), K - 1)); NaN counts as 0 (the value is clamped before it is converted).
 *   3. the point is moved by knot b of its scan: the operation cc_ingest_points documents for h_tf, in its order.
 * The scan's result -- descriptor, bev, pix_rc, labels, every byte -- is what cc_ingest_batch gives for the moved points in their
 * original order: among equal heights in one cell the first point in file order wins, whatever its time; the blind zone, the
 * border, max / min height and the continuous position see the moved point only.  The matrices are piecewise constant on purpose
 * (K = 32 on a 0.1 s sweep: 3 ms bins, under 10 cm at 30 m/s); a call with K = 1 gives the bytes of cc_ingest_points with that
 * matrix as h_tf (by its own kernels).
 * Checked before anything is queued or read (CC_EINVAL, the context stays as it was): the layout passes cc_ingest_points'
 * rules; time_offset is a multiple of 4 with time_offset + 4 <= stride_bytes; the time word does not overlap the 12 bytes of
 * x, y, z; time_type is CC_TIME_F32 or CC_TIME_U32; 1 <= n_knots <= CC_MOTION_KNOTS_MAX; motion, h_time and h_knots are
 * non-NULL; every scale is finite.  h_time and h_knots are copied before the call returns.
 * A time per segment of a scan made of segments is cont2_amd_rig.h's (cc_ingest_rig: every segment its own time word and its own
 * slice of the scan's knots).  Out of scope: f64 or 64-bit integer time stamps; interpolation between knots; a batch form of the
 * per-scan call; 12-byte records, which have no room for a time.
 * What the kernels cost next to cc_ingest_points': DESIGN.md 3.0. */
#define CC_MOTION_KNOTS_MAX 64
enum { CC_TIME_F32 = 0, CC_TIME_U32 = 1 };
typedef struct {
  int32_t time_offset; /* byte offset of the time word inside a record */
  int32_t time_type;   /* CC_TIME_F32 / CC_TIME_U32 */
  int32_t n_knots;     /* K */
  int32_t pad_;
} cc_point_motion_t;   /* 16 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_point_motion_t) == 16, "cc_point_motion_t: 16 bytes");
#else
_Static_assert(sizeof(cc_point_motion_t) == 16, "cc_point_motion_t: 16 bytes");
#endif
/*   h_time  : [n_scans][2] f32: t_begin (CC_TIME_U32: the u32's bits), scale
 *   h_knots : [n_scans][K][12] f32
 * Everything else as cc_ingest_points (device records read in place, work queued on `stream`, chunks of max_batch_scans). */
int cc_ingest_points_motion(cc_ctx *ctx, const void *d_points, const cc_point_layout_t *layout, const cc_point_motion_t *motion,
                            const int64_t *h_offsets, int n_scans, const float *h_time, const float *h_knots, cc_scan_desc_t *d_out,
                            const cc_ingest_debug_t *dbg, void *stream);
/* The same from host records (cc_ingest_points_host's shape; h_bev may be NULL). */
int cc_ingest_points_motion_host(cc_ctx *ctx, const void *h_points, const cc_point_layout_t *layout, const cc_point_motion_t *motion,
                                 const int64_t *h_offsets, int n_scans, const float *h_time, const float *h_knots, cc_scan_desc_t *h_out,
                                 float *h_bev);
/* Knots from the poses at the sweep's begin and end (host only, f64; row-major 3 x 4 [R | p], sensor to world):
 *   T(s) = [R_b Exp(s Log(R_b^T R_e)) | (1 - s) p_b + s p_e],   knot k = T(ref)^-1 T((k + 0.5) / K), rounded to f32.
 * ref in [0, 1] is the instant the scan is referred to (1: the sweep's end).  Composing an extrinsic matrix is the caller's
 * multiplication. */
void cc_motion_knots(const double pose_begin[12], const double pose_end[12], double ref, int K, float *knots /*[K][12]*/);

/* ---- a sensor's RANGE IMAGE rasterised in place, de-skewed per column ----
 * A spinning LiDAR does not measure x, y, z: it measures one range word per (beam, firing) -- 2 or 4 bytes per pixel of an H x W
 * image -- and its calibration is a few hundred angles.  These calls take the range words as the driver has them and make the
 * points while the rasteriser loads them: no pass that expands the image into a 16-byte-per-point cloud, and none that de-skews
 * it -- in a range image a pixel's time is its column, so the knot of a pixel is a per-column table entry.  No reference counterpart.
 * A pixel is (row, col) = (beam, firing); pixel j of a scan is (j / W, j % W) in CC_RANGE_ROW_MAJOR order (Ouster LidarScan fields)
 * and (j % H, j / H) in CC_RANGE_COL_MAJOR order (firing after firing: Velodyne / Hesai packets).  The model is fixed per sensor:
 *   row_tab[row]     = cos(alt), sin(alt), cos(az_off), sin(az_off) of the beam        (ca, sa, co, so)
 *   col_cos_sin[col] = cos, sin of the encoder azimuth of the firing                   (ce, se)
 *   col_knot[col]    = the knot that moves the firing's points, in [0, K - 1]
 * THE ARITHMETIC, all f32, every product and every sum rounded once, in exactly this association (w: the pixel's word):
 *   r  = (float)w * range_scale      u16 / u32: the conversion is exact or rounds to nearest even; f32: the word itself * range_scale
 *   d  = r - origin_n
 *   h  = d * ca
 *   dx = (ce * co) - (se * so)       dy = (se * co) + (ce * so)
 *   x  = (h * dx) + (origin_n * ce)  y  = (h * dy) + (origin_n * se)      z = (d * sa) + origin_z
 * With K >= 1 knots per scan (x, y, z) is then moved by knot col_knot[col] of ITS scan: the operation cc_ingest_points documents
 * for h_tf, in its order.  K = 1 is a per-scan extrinsic or pose, K = 32 de-skews a sweep (cc_motion_knots makes the matrices);
 * K = 0: the points stay in the sensor frame.  A pixel with NO RETURN -- an integer word of 0; an f32 word that is not > 0: zero,
 * negative or NaN -- is rejected as a NaN point is: it owns nothing and counts nowhere.
 * The scan's result -- descriptor, bev, pix_rc, labels, every byte -- is what cc_ingest_batch gives for these points in pixel
 * storage order j: among equal heights in one cell the pixel with the smaller j wins; the blind zone, the border, max / min
 * height and the continuous position see the final point only.
 * Checked before anything is queued or read (CC_EINVAL, the context stays as it was): 1 <= n_rows <= CC_RANGE_ROWS_MAX, 1 <= n_cols
 * <= CC_RANGE_COLS_MAX, 10 < n_rows * n_cols < 2^21; a known word_type and order; finite range_scale, origin_n, origin_z; 0 <=
 * n_knots <= CC_MOTION_KNOTS_MAX; every col_knot in [0, K - 1] (K = 0: all 0); non-NULL row_tab and col_cos_sin (col_knot may be
 * NULL: all 0); h_knots NULL exactly when K = 0; the base pointer of the range words aligned to the word size; the sensor used
 * with the context it was created on.
 * Out of scope: dual returns; a time word per pixel; destaggered images (the staggered image with az_off per beam is what the model
 * describes); interpolation between knots; range images as segments; intensity channels.  What the kernels cost: DESIGN.md 3.0. */
#define CC_RANGE_ROWS_MAX 128
#define CC_RANGE_COLS_MAX 4096
enum { CC_RANGE_U16 = 0, CC_RANGE_U32 = 1, CC_RANGE_F32 = 2 };
enum { CC_RANGE_ROW_MAJOR = 0 /* j = row * W + col: Ouster LidarScan fields, the synth's order */,
       CC_RANGE_COL_MAJOR = 1 /* j = col * H + row: firing after firing, Velodyne / Hesai packets */ };
typedef struct {
  int32_t n_rows, n_cols, word_type, order;
  float   range_scale;        /* metres per unit of the word (0.001 for Ouster mm, 0.002 Velodyne, 0.004 Hesai, 1 for f32 metres) */
  float   origin_n, origin_z; /* beam origin: distance from the rotation axis, height above the sensor frame's origin (0, 0: Velodyne) */
  int32_t n_knots;            /* K, 0 .. CC_MOTION_KNOTS_MAX; 0: points stay in the sensor frame */
  const float   *row_tab;     /* host [H][4]: cos(alt), sin(alt), cos(az_off), sin(az_off) of the beam */
  const float   *col_cos_sin; /* host [W][2]: cos, sin of the encoder azimuth of the firing */
  const int32_t *col_knot;    /* host [W]: knot index of the firing, each in [0, K-1]; NULL: all 0 */
} cc_range_model_t;           /* 56 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_range_model_t) == 56 && offsetof(cc_range_model_t, range_scale) == 16 && offsetof(cc_range_model_t, n_knots) == 28 &&
                  offsetof(cc_range_model_t, row_tab) == 32 && offsetof(cc_range_model_t, col_knot) == 48,
              "cc_range_model_t: 56 bytes, range_scale at 16, n_knots at 28, row_tab at 32, col_knot at 48");
#else
_Static_assert(sizeof(cc_range_model_t) == 56 && offsetof(cc_range_model_t, range_scale) == 16 && offsetof(cc_range_model_t, n_knots) == 28 &&
                   offsetof(cc_range_model_t, row_tab) == 32 && offsetof(cc_range_model_t, col_knot) == 48,
               "cc_range_model_t: 56 bytes, range_scale at 16, n_knots at 28, row_tab at 32, col_knot at 48");
#endif
typedef struct cc_range_sensor cc_range_sensor;
/* Checks the model and copies its tables to the device once (the device layout is the library's own; the host tables may go when
 * the call returns).  A sensor belongs to the context it was created on and must be destroyed before it. */
int cc_range_sensor_create(cc_ctx *ctx, const cc_range_model_t *model, cc_range_sensor **out);
int cc_range_sensor_destroy(cc_range_sensor *sensor);
/*   d_ranges : scan i is the H * W words at d_ranges + i * H * W * wordsize, device memory, read in place
 *   h_knots  : [n_scans][K][12] f32 host memory (copied before the call returns); NULL iff K == 0
 * Everything else as cc_ingest_points (work queued on `stream`, chunks of max_batch_scans, cc_profile_enable brackets the kernels). */
int cc_ingest_ranges(cc_ctx *ctx, const cc_range_sensor *sensor, const void *d_ranges, int n_scans, const float *h_knots, cc_scan_desc_t *d_out,
                     const cc_ingest_debug_t *dbg, void *stream);
/* The same from host range words (cc_ingest_host_bev's shape: one H2D copy, results copied back; h_bev may be NULL; the host
 * pointer is held to the same alignment). */
int cc_ingest_ranges_host(cc_ctx *ctx, const cc_range_sensor *sensor, const void *h_ranges, int n_scans, const float *h_knots, cc_scan_desc_t *h_out,
                          float *h_bev);

/* ---- the per-scan loop (test/batch_bin_test.cpp:131-237 at sensor rate) ----
 * A cc_scan is ONE scan's descriptor kept on the device between ContourManager::makeContoursRecurs (contour_mng.h:588),
 * ContourDB::queryRangedKNN (contour_db.h:698) and ContourDB::addScan (:814): the class mirror's ContourManager holds one.
 * Nothing is allocated per scan: the context owns pinned staging buffers for the points, a device point buffer and a pool
 * of descriptor slots; the calls only queue work, the host copy of the descriptor (and of the max-height image, if asked
 * for) is fetched when a getter needs it.  Streams: cc_scan_ingest queues on the next of the context's two ingest CHANNELS
 * (own stream, device point buffer and one-scan scratch: consecutive scans' ingests overlap) and records the scan's `ready`
 * event behind its last kernel; cc_scan_desc / cc_scan_offload / cc_db_query_scan / cc_db_add_scan work on
 * the loop stream, which waits for `ready` first.  So scan i + 1 (and i + 2) can be ingested while scan i is queried and
 * added -- also from OTHER host threads: cc_ingest_batch / cc_stage_points* / cc_scan_ingest of one context serialise on
 * the context's ingest lock (the staging slots, the device point buffer and the K1/K2 scratch are shared), next to one
 * thread in the other cc_scan_* / cc_db_* calls (the slot pool is locked, cc_last_error is per thread).  The class
 * mirror's evaluator does exactly that (hostcpp/eval/evaluator.h: a helper thread reads the next files and ingests them).
 *   cc_stage_points  : pinned buffer for n_points x (x,y,z,i) f32 (write the points there to save a host copy), NULL on
 *                      failure.  The buffer belongs to the CALLING THREAD until that thread passes it to cc_scan_ingest
 *                      (or gives it up: cc_stage_points_cancel, or stages the same slot again); another thread that asks for
 *                      the same slot meanwhile waits.  cc_stage_points uses a slot of its own; cc_stage_points_slot names
 *                      slot 0 .. 2 * CC_SCAN_BATCH_MAX - 1 (each allocated when first asked for) -- so that the next scan's file can be read into one while the other's
 *                      scan is on its way to the device (a read-ahead thread alternates them, the driver thread's
 *                      cc_stage_points never collides with it); a slot is handed out again once ITS last copy has passed
 *                      (readKITTIPointCloudBin of scan i+1 next to queryRangedKNN of scan i, tools/pointcloud_util.h:9-47,
 *                      evaluator.h:285-302).  Asking for more points than the buffers hold re-allocates ALL slots (after
 *                      the ingest stream has drained; CC_EINVAL while another thread holds one)
 *   cc_stage_points_cancel : give a staged buffer back without ingesting it (short file, read error)
 *   cc_scan_ingest   : makeBEV + makeContoursRecurs for the points at h_xyzi (may be a staging pointer); want_bev != 0
 *                      keeps the max-height image for cc_scan_bev.  Returns at once (work is queued on the ingest stream).
 *   cc_scan_desc     : host copy of the descriptor (first call: one D2H copy + sync); CC_ECAPACITY if the scan exceeded a
 *                      capacity of the contour kernel (flags CC_DESC_INEXACT_*), the copy is delivered all the same
 *   cc_scan_offload  : move the descriptor to the host and give the device slot back; cc_scan_desc keeps working.  (The
 *                      mirror keeps the descriptors of the last CC_SCANS_ON_DEVICE = 8 192 added scans on the device --
 *                      169 KB each -- and offloads the oldest beyond that: a copy + sync per scan the loop does not need)
 *   cc_scan_release  : free the handle (waits for the scan's ingest and for queued readers of its slot) */
#define CC_SCAN_BATCH_MAX 16 /* scans per cc_scan_ingest_batch / cc_db_add_scan_batch / cc_db_query_scan_batch_submit */
typedef struct cc_scan cc_scan;
float *cc_stage_points(cc_ctx *ctx, int64_t n_points);
float *cc_stage_points_slot(cc_ctx *ctx, int64_t n_points, int slot);
int cc_stage_points_cancel(cc_ctx *ctx, const float *staged);
int cc_scan_ingest(cc_ctx *ctx, const float *h_xyzi, int64_t n_points, int want_bev, cc_scan **out);
/* cc_scan_ingest (want_bev = 0) for 1..CC_SCAN_BATCH_MAX scans at once: h_xyzi[i] must be staging buffers (cc_stage_points_slot,
 * distinct slots) in the calling thread's hands; ONE K1 / K2 launch chain for the batch (a chain takes ~0.2 ms of launch
 * latencies whatever it holds), out[i] are ordinary scan handles.  All or nothing: on an error no handle is returned.
 * cc_scan_ready: 1 once the scan's ingest has finished on the device, 0 while it is in flight (never blocks). */
int cc_scan_ingest_batch(cc_ctx *ctx, const float *const *h_xyzi, const int64_t *n_points, int n, cc_scan **out);
/* The two calls above for records of another shape and / or with a transform (layout, h_tf: as for cc_ingest_points; one
 * layout per call, h_tf = 12 floats per scan or NULL).  The records go to the device as they are: no repack on the host.
 * Staging: a buffer handed out by cc_stage_points* for n_points holds 16 * n_points BYTES, whatever is written there; a
 * caller with records of stride_bytes stages (n * stride_bytes + 15) / 16 "points" for a scan of n and may write
 * n * stride_bytes bytes (CC_EINVAL when a scan's bytes exceed what was staged). */
int cc_scan_ingest_points(cc_ctx *ctx, const void *h_points, const cc_point_layout_t *layout, int64_t n_points, const float *h_tf,
                          int want_bev, cc_scan **out);
int cc_scan_ingest_points_batch(cc_ctx *ctx, const void *const *h_points, const cc_point_layout_t *layout, const int64_t *n_points, int n,
                                const float *h_tf, cc_scan **out);
/* cc_scan_ingest_points for ONE scan made of n_segs host segments (cc_point_segment_t above; the records go through the context's
 * own staging buffer): an ordinary scan handle comes out. */
int cc_scan_ingest_segments(cc_ctx *ctx, const cc_point_segment_t *h_segs, int n_segs, int want_bev, cc_scan **out);
/* cc_scan_ingest_points for ONE scan de-skewed by per-point time (cc_ingest_points_motion above; h_time: 2 values, h_knots:
 * [K][12]): an ordinary scan handle comes out. */
int cc_scan_ingest_points_motion(cc_ctx *ctx, const void *h_points, const cc_point_layout_t *layout, const cc_point_motion_t *motion,
                                 int64_t n_points, const float *h_time, const float *h_knots, int want_bev, cc_scan **out);
/* cc_scan_ingest for ONE scan given as a range image (cc_ingest_ranges above; h_ranges: H * W host words, through the context's own
 * staging buffer; h_knots: [K][12] or NULL iff K == 0): an ordinary scan handle comes out. */
int cc_scan_ingest_ranges(cc_ctx *ctx, const cc_range_sensor *sensor, const void *h_ranges, const float *h_knots, int want_bev, cc_scan **out);
int cc_scan_ready(const cc_scan *scan);
int cc_scan_desc(cc_scan *scan, const cc_scan_desc_t **h_desc);
int cc_scan_bev(cc_scan *scan, const float **h_bev);
int cc_scan_offload(cc_scan *scan);
int cc_scan_on_device(const cc_scan *scan); /* 1: the descriptor still sits in a device slot, 0: offloaded (or NULL) */
int cc_scan_release(cc_scan *scan);

/* ---------------------------------------------------------------------- database -------- */
/* Replaces ContourDB::ContourDB (contour_db.h:680-684).  1 <= cfg->nnk <= CC_KNN_MAX_LARGE: a database with
 * nnk > CC_KNN_MAX runs the large-k instances of the query kernels, in chunks of 256 queries. */
int cc_db_create(cc_ctx *ctx, const cc_db_cfg_t *cfg, int capacity_scans, cc_db **out);
int cc_db_destroy(cc_db *db);
int cc_db_size(const cc_db *db);
/* The last dimension of d_knn (cc_db_query_batch / cc_db_query_submit): CC_KNN_MAX when nnk <= CC_KNN_MAX, else
 * CC_KNN_MAX_LARGE.  0 for NULL. */
int cc_db_knn_stride(const cc_db *db);

/* Replaces ContourDB::addScan + ContourDB::pushAndBalance (contour_db.h:814-843) and
 * LayerDB::rebuild (src/cont2/contour_db.cpp:63-317) for n consecutive scans:
 * for i in [0,n): addScan(desc[i], h_ts[i]); pushAndBalance(h_seed[i], h_ts[i]).
 * The descriptors are appended to the device-resident DB; the bucket bookkeeping (which key
 * is searchable from which epoch on, bucket ranges per epoch) runs on the host.
 * Epoch e = state after e scans have been added and balanced.
 * An append does NOT wait for query chunks in flight (cc_db_query_submit): they were submitted against an earlier epoch
 * and keep reading the state they were submitted with (the sorted key view is double-buffered and a buffer is rewritten
 * only after its readers have finished -- a device-side wait; everything else is append-only).  So the online loop
 * ingest -> add -> submit(query at its own epoch) streams batch after batch without draining the GPU.  The call returns
 * once the host bookkeeping is done and its device work (key upload, sorted-view merge) is QUEUED on `stream`: queries
 * submitted afterwards wait for it on the device, whatever stream they come from; d_desc may be overwritten by work
 * queued on `stream` after the call. */
int cc_db_add_scans(cc_db *db, const cc_scan_desc_t *d_desc, int n, const double *h_ts,
                    const int32_t *h_seed, void *stream);

/* Optional first half of cc_db_add_scans for callers that stream batch after batch (the online loop of bench.py
 * --workload seq): queues, on `stream` and without waiting, what an append needs from the device before the host
 * bookkeeping can run -- the batch's compact records packed into the rows they will occupy, the retrieval keys
 * (key dimension 0 decides the bucket, contour_db.h:184-192) extracted and copied to pinned host memory.  Issued right
 * behind the batch's ingest, the copy travels while the previous batch is being queried; cc_db_add_scans on the same
 * (d_desc, n) then finds the keys on the host instead of waiting for a round trip.  The database is not changed.
 * At most two batches (<= 4096 scans each) may be prepared ahead; they must be added in the order they were prepared and
 * before anything else is added (CC_EINVAL otherwise); if the add of a prepared batch fails (CC_ECAPACITY: a scan flagged
 * inexact), a batch prepared behind it is dropped with it.  d_desc must not be overwritten before the add. */
int cc_db_add_scans_prepare(cc_db *db, const cc_scan_desc_t *d_desc, int n, void *stream);

/* Replaces ContourDB::queryRangedKNN (contour_db.h:698-811) for a batch of query scans.
 * Query i is answered against DB epoch h_epoch[i] (use cc_db_size() for "now"); in the
 * reference loop scan i queries epoch i (batch_bin_test.cpp:179 runs before :234-237).
 *   d_qdesc : [nq] query descriptors (device)
 *   h_res   : [nq] results (host)
 *   d_knn   : optional [nq][CC_NQLEV][CC_NPIV][stride] hits, stride = cc_db_knn_stride(db) (CC_KNN_MAX when
 *             nnk <= CC_KNN_MAX), + d_knn_cnt [nq][3][6] i32
 *             (parity/debug; NULL to skip)
 *   thres_lb: the bars of the four gates and of the post-checks (CandidateScoreEnsemble sim_lb, contour_db.h:374-596)
 *   thres_ub: validated like CandidateManager's ctor does (lb.strictSmaller(ub), contour_db.h:365-367: CC_EINVAL otherwise).
 *             By default the bars stay constant during a query, the reference's shipped DYNAMIC_THRES=0 build
 *             (CMakeLists.txt:19-20), and thres_ub is not used further.  After cc_db_set_dynamic_thres(db, 1) the query
 *             replays the DYNAMIC_THRES=1 build instead: every check that passes raises the five check bars to
 *             min(max(bar, i_orie_sim), ub) (contour_db.h:439-457), every candidate that survives the post-checks raises
 *             the three post bars to min(max(bar, value), ub) (contour_db.h:566-574), in the reference's iteration order. */
int cc_db_query_batch(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch,
                      const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                      cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt,
                      void *stream);

/* The same call split in two, for callers that stream batch after batch (offline evaluation of whole sequences,
 * tools/batch_eval.py, bench.py): cc_db_query_submit queues the batch's launch chains and returns; a chunk's results
 * reach h_res when its lane is needed again (a later submit) or at cc_db_query_wait, so the tail of one batch's chains
 * runs next to the head of the next batch's.  h_res must stay valid until cc_db_query_wait returned; d_qdesc may be
 * overwritten by work queued on `stream` after the call.  An error of an earlier batch's chunk (capacity flags) is
 * reported by the call that collects it.  cc_db_query_batch == submit + wait; cc_db_check_hints, cc_db_set_lanes and
 * cc_db_destroy collect the chunks in flight first; the appends do not need to (see cc_db_add_scans). */
int cc_db_query_submit(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch,
                       const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                       cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt,
                       void *stream);
int cc_db_query_wait(cc_db *db);

/* Host-descriptor variants (one H2D copy each) used by the C++ class mirror, where a ContourManager owns a
 * host copy of its descriptor: ContourDB::addScan + pushAndBalance for one scan, and queryRangedKNN for one
 * query against the current DB state. */
int cc_db_add_scan_host(cc_db *db, const cc_scan_desc_t *h_desc, double ts, int32_t seed);
int cc_db_query_host(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                     cc_query_result_t *h_res);

/* The same two calls for a scan that is still on the device (cc_scan_ingest): no descriptor copy in either direction.
 * cc_db_query_scan answers against the current DB state; cc_db_add_scan = addScan + pushAndBalance. */
int cc_db_query_scan(cc_db *db, cc_scan *scan, const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res);
int cc_db_add_scan(cc_db *db, cc_scan *scan, double ts, int32_t seed);
/* cc_db_query_scan without the wait, at an explicit epoch (0 .. cc_db_size): *h_res is filled by the next cc_db_query_wait.
 * A per-scan driver that knows its next scans (the evaluator mirror does: test/batch_bin_test.cpp:131-237 walks a list) appends
 * them and queues scan k's query at epoch k while the driver is still busy with scan i < k; the answers are the ones the
 * strictly sequential loop gets (a query at epoch k sees the database as it was after k scans). */
int cc_db_query_scan_submit(cc_db *db, cc_scan *scan, int32_t epoch, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                            cc_query_result_t *h_res);
/* cc_db_query_wait for the chunks that write into [h_res, h_res + n) only: the caller's own answer, while later submissions
 * stay in flight. */
int cc_db_query_collect(cc_db *db, const cc_query_result_t *h_res, int n);
/* cc_db_add_scans_prepare (the asynchronous first half of an append) for a scan handle; cc_db_add_scan on the same scan
 * later only commits. */
int cc_db_add_scan_prepare(cc_db *db, cc_scan *scan);

/* cc_db_add_scan and cc_db_query_scan_submit for 1..CC_SCAN_BATCH_MAX scan handles at a time: scans[i] is appended with
 * (h_ts[i], h_seed[i]) in the order given; scans[i] is queried at h_epoch[i] (0 .. cc_db_size), its answer goes to h_res[i]
 * (cc_db_query_collect / cc_db_query_wait).  The answers are those of the same calls made one by one; what changes is the
 * number of launches: one chain per batch.  A per-scan driver that knows its next B scans appends them in one call and then
 * queues each one's query at its own position (scan k at epoch k sees the database as it was after k scans): the class
 * mirror's read-ahead does (hostcpp/cont2/contour_db.h). */
int cc_db_add_scan_batch(cc_db *db, cc_scan *const *scans, int n, const double *h_ts, const int32_t *h_seed);
int cc_db_query_scan_batch_submit(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                  const cc_score_t *thres_ub, cc_query_result_t *h_res);

/* The two batched calls with host descriptor buffers (one H2D copy each): for drivers that keep descriptors on the host,
 * e.g. an offline replay of a whole sequence (all scans added, then scan i queried against epoch i). */
int cc_db_add_scans_host(cc_db *db, const cc_scan_desc_t *h_desc, int n, const double *h_ts, const int32_t *h_seed);
int cc_db_query_batch_host(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch,
                           const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res);

/* CandidateManager driven by explicit anchor hints instead of the KNN search (the single-pair flow of
 * test/kitti_read_bin_test.cpp:226-291): for one query scan, CandidateManager::checkCandWithHint (contour_db.h:374-488)
 * for every hint IN THE GIVEN ORDER, then tidyUpCandidates (:494-596) and fineOptimize (:604-648).  Candidate scans are
 * scans of `db` (any scan added so far, searchable or not).  Hint levels must be within 1..4 (DIST_BIN_LAYERS), at most
 * CC_HINT_MAX hints.  h_scores (optional, [n_hints]) receives what checkCandWithHint returns per hint. */
#define CC_HINT_MAX (CC_NQLEV * CC_NPIV * CC_KNN_MAX)
typedef struct {
  int32_t cand_gidx; /* candidate scan = cm_cand (DB index)                    */
  int8_t level;      /* ConstellationPair{level, seq_src, seq_tgt}, contour_mng.h:221-240 */
  int8_t seq_src;    /* anchor contour of the candidate scan                   */
  int8_t seq_tgt;    /* anchor contour of the query scan                       */
  int8_t pad;
} cc_hint_t;
typedef struct {
  int32_t i_ovlp_sum, i_ovlp_max_one, i_in_ang_rng; /* ScoreConstellSim  */
  int32_t i_indiv_sim, i_orie_sim;                  /* ScorePairwiseSim  */
  int32_t passed;                                   /* 1: a proposal was added for this hint */
} cc_hint_score_t;
int cc_db_check_hints(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints,
                      const cc_score_t *thres_lb, const cc_score_t *thres_ub, int max_fine_opt,
                      cc_query_result_t *h_res, cc_hint_score_t *h_scores, void *stream);
int cc_db_check_hints_host(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints,
                           const cc_score_t *thres_lb, const cc_score_t *thres_ub, int max_fine_opt,
                           cc_query_result_t *h_res, cc_hint_score_t *h_scores);

/* Verification of candidates the CALLER proposes (odometry or GPS proximity, another descriptor, another robot's map, a
 * re-check of accepted loops): the batched, streamed form of the hint flow.  Item i is the query scan d_qdesc[h_qidx[i]]
 * (h_qidx NULL: d_qdesc[i], and then n == n_desc) against the database scans h_cands[i][0 .. m_i), 0 <= m_i <=
 * CC_VERIFY_CANDS_MAX, the list ended by -1; candidates are DB indices below cc_db_size, searchable or not.  Several items
 * may name the same descriptor: one item per (query, candidate) pair gives one verdict per pair instead of the best of a list
 * (cc_db_verify_submit_ranked lists every refined candidate of ONE item instead: the query's pack and prep work is done once).
 *
 * The hint list of an item is generated on the device, in the demo's order (test/kitti_read_bin_test.cpp:226-291 with the
 * candidate as the outermost index): for candidate k in list order, for level 1..4 where set in level_mask, for seq_src
 * 0..CC_NPIV-1 (the candidate's anchor), for seq_tgt 0..CC_NPIV-1 (the query's anchor) -- unless either retrieval key sums
 * to zero (the f32 sum in index order: the anchor does not exist, contour_db.h:726) or the keys' squared f32 distance
 * (accumulated in index order, every product and sum rounded once) exceeds max_key_dist_sq.
 *
 * h_res[i] is, byte for byte, what cc_db_check_hints returns for that query, that hint list, the same thresholds and
 * max_fine_opt: n_knn_hits = the number of hints generated, cand_gidx = a DB index, n_res = 0 for an empty list.  d_hints /
 * d_n_hints (device, optional) receive the generated lists: [n][CC_HINT_MAX] and [n].
 *
 * Refused with CC_EINVAL before anything is queued (the handle and the chunks in flight stay untouched): NULL arguments,
 * n < 0, h_qidx[i] outside [0, n_desc), a candidate outside [0, cc_db_size), a candidate listed twice in one item, an entry
 * other than -1 after the first -1, max_fine_opt < 1, level_mask outside 0..15, a NaN or negative max_key_dist_sq, thresholds
 * that fail lb.strictSmaller(ub).
 *
 * Streaming: the batch is cut into chunks over the lanes exactly like cc_db_query_submit (at most 1024 items per chunk, 256
 * on a database with nnk > CC_KNN_MAX); cc_db_query_wait / cc_db_query_collect collect verify chunks too; chunks wait for the
 * last append on the device; the caller's stream continues once the descriptors are read; CC_QF_* flags / CC_ECAPACITY as for
 * queries; cc_db_set_dynamic_thres applies; with cc_db_profile_enable the hint generation's time lands in ms_out[0]. */
#define CC_VERIFY_CANDS_MAX 8 /* 8 candidates x 4 levels x 6 x 6 anchor pairs = CC_HINT_MAX check slots */
typedef struct {
  int32_t level_mask;    /* bit (level-1) for hint levels 1..4; 0 stands for 0xF                                    */
  int32_t max_fine_opt;  /* >= 1, as cc_db_check_hints                                                              */
  float max_key_dist_sq; /* anchor pairs whose keys are farther apart are not checked (the demo uses 1000.0f);
                            INFINITY = no bound                                                                    */
  int32_t pad_;
} cc_verify_cfg_t;
int cc_db_verify_submit(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                        const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                        cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints, void *stream);
/* submit + cc_db_query_wait */
int cc_db_verify_batch(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                       const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                       cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints, void *stream);
/* ... with host descriptors: one H2D copy of them, like cc_db_query_batch_host */
int cc_db_verify_batch_host(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                            const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                            cc_query_result_t *h_res);

/* ---- the ranked list of a query's refined candidates ----
 * Every entry point above answers with the best candidate: fineOptimize's `ret_size = 1` (contour_db.h:604-648).  The _ranked
 * forms return what fineOptimize would with ret_size = min(max_ret, pre_sel_size): the first entries of candidates_ after its
 * second std::sort -- the (at most max_fine_opt) candidates that were refined, by refined correlation, best first; ties in the
 * order that sort leaves them in.  Entry 0 is the candidate h_res reports, bit for bit; h_res itself is what the plain call
 * returns.  Candidates that were not refined are not listed.  Other passes through the same place show up as further entries:
 * several loop edges per key frame for a back end that weighs or switches hypotheses, one verdict per proposed candidate from
 * ONE verify item.
 *
 * h_n[i] = min(max_ret, max_fine_opt, n_cand_tidy), 0 where n_res is 0; h_cands[i][0 .. h_n[i]) are the entries, the rest of
 * the row is zeroed.  A chunk's rows arrive with its h_res rows (cc_db_query_wait / cc_db_query_collect, or the synchronous
 * call's return), so both buffers must stay valid until then.  Everything else -- chunking, streaming, epochs, thresholds,
 * dynamic thresholds, flags and CC_ECAPACITY -- is the plain call's.  Refused with CC_EINVAL before anything is queued: rank
 * NULL, h_cands or h_n NULL, max_ret outside 1..CC_RANK_MAX (and whatever the plain call refuses). */
#define CC_RANK_MAX 16
typedef struct {
  int32_t cand_gidx;   /* DB index, as cc_query_result_t.cand_gidx of the same entry point                             */
  int32_t flags;       /* the CC_QF_GMM_CAP / CC_QF_DESC_CAP bits of THIS candidate's correlation problem             */
  double correlation;  /* refined                                                                                     */
  double tf[3];        /* (x, y, theta), as cc_query_result_t.tf                                                      */
} cc_ranked_cand_t; /* 40 bytes */
typedef struct {
  cc_ranked_cand_t *h_cands; /* [n][max_ret], host; rows beyond h_n[i] are zeroed */
  int32_t *h_n;              /* [n]                                               */
  int32_t max_ret;           /* 1..CC_RANK_MAX                                    */
  int32_t pad_;
} cc_rank_out_t;
int cc_db_query_submit_ranked(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *thres_lb,
                              const cc_score_t *thres_ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt,
                              void *stream, const cc_rank_out_t *rank);
/* synchronous, host descriptors */
int cc_db_query_batch_host_ranked(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                  const cc_score_t *thres_ub, cc_query_result_t *h_res, const cc_rank_out_t *rank);
/* scan handles (n = 1: the per-scan loop's query) */
int cc_db_query_scan_batch_submit_ranked(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                         const cc_score_t *thres_ub, cc_query_result_t *h_res, const cc_rank_out_t *rank);
/* one item of <= CC_VERIFY_CANDS_MAX candidates -> one entry per candidate that survives (cand_gidx names it) */
int cc_db_verify_submit_ranked(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                               const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                               cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints, void *stream, const cc_rank_out_t *rank);
/* synchronous; n = 1 */
int cc_db_check_hints_ranked(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *thres_lb,
                             const cc_score_t *thres_ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores,
                             void *stream, const cc_rank_out_t *rank);
/* the verify and hint flows with host descriptors (one H2D copy, then the calls above; both synchronous): what a caller without
 * device memory of its own uses -- the class mirror (hostcpp/cont2/contour_db.h) */
int cc_db_verify_batch_host_ranked(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                                   const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                                   cc_query_result_t *h_res, const cc_rank_out_t *rank);
int cc_db_check_hints_host_ranked(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints,
                                  const cc_score_t *thres_lb, const cc_score_t *thres_ub, int max_fine_opt, cc_query_result_t *h_res,
                                  cc_hint_score_t *h_scores, const cc_rank_out_t *rank);

/* ---- pose curvature and refinement detail per ranked candidate ----
 * A ranked entry is a scan, a correlation and a pose; a pose-graph edge also needs to know in which directions that pose is
 * pinned down (a revisit along a straight corridor scores high and is free to slide along it).  The _ranked_detail forms
 * return, next to every ranked entry, the curvature of the objective the refinement minimised, at the pose it stopped at,
 * and what the device knows about the refinement itself.  h_detail is [n][rank->max_ret] on the host, row i / entry k
 * belonging to h_cands[i][k]; its rows arrive with the h_cands rows and the entries beyond h_n[i] are zeroed, exactly as
 * there.  h_res and the ranked lists are the bytes the _ranked call returns.  Everything else is the _ranked call's;
 * h_detail NULL is CC_EINVAL, refused before anything is queued, together with whatever the _ranked call refuses.
 *
 * hess is a CURVATURE, not a calibrated covariance: the second derivative of f(p) = -correlation(p), p = (x, y, theta) in
 * BEV pixels / radians, positive definite at a proper optimum.  A back end scales it (for instance by a variance fitted on
 * its own data) before using it as an information matrix.  The sum runs over the ellipse pairs selected at tf_init -- the
 * set the refinement optimised over; where a capacity cut that list (flags), over the pairs the refinement summed. */
typedef struct {
  double hess[6];    /* xx, xy, xt, yy, yt, tt of f at the entry's tf: (d2 cost / dp2) / sqrt(auto_corr_src * auto_corr_tgt) */
  double grad[3];    /* gradient of f at tf (what the refinement left over)                                                */
  double tf_init[3]; /* T_init the refinement started from (anch_props_[0].T_delta_ after tidyUpCandidates)                */
  double corr_init;  /* the correlation at tf_init                                                                         */
  int32_t iterations, termination; /* of the L-BFGS run: ceres::Solver::Summary's iteration count and termination type     */
  int32_t n_pairs;   /* selected (src, tgt) ellipse pairs                                                                  */
  int32_t flags;     /* == cc_ranked_cand_t.flags of the entry                                                             */
} cc_ranked_detail_t; /* 120 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_ranked_detail_t) == 120, "cc_ranked_detail_t is 120 bytes");
#else
_Static_assert(sizeof(cc_ranked_detail_t) == 120, "cc_ranked_detail_t is 120 bytes");
#endif
int cc_db_query_submit_ranked_detail(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                     const cc_score_t *thres_ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt,
                                     void *stream, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);
int cc_db_query_batch_host_ranked_detail(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch,
                                         const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res,
                                         const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);
int cc_db_query_scan_batch_submit_ranked_detail(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                                const cc_score_t *thres_ub, cc_query_result_t *h_res, const cc_rank_out_t *rank,
                                                cc_ranked_detail_t *h_detail);
int cc_db_verify_submit_ranked_detail(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands,
                                      int n, const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                                      cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints, void *stream,
                                      const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);
int cc_db_verify_batch_host_ranked_detail(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands,
                                          int n, const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                                          cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);
int cc_db_check_hints_ranked_detail(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints,
                                    const cc_score_t *thres_lb, const cc_score_t *thres_ub, int max_fine_opt, cc_query_result_t *h_res,
                                    cc_hint_score_t *h_scores, void *stream, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);
int cc_db_check_hints_host_ranked_detail(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints,
                                         const cc_score_t *thres_lb, const cc_score_t *thres_ub, int max_fine_opt, cc_query_result_t *h_res,
                                         cc_hint_score_t *h_scores, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);

/* ---- caller-given relative poses: score, probe and refine (ConstellCorrelation's public interface, correlation.h:175-238) ----
 * Every entry point above takes the start pose of a correlation problem from a constellation that passed the four gates.  These
 * take it from the caller: item i = (q, gidx, tf) is the query scan d_qdesc[q] (tgt) against the database scan gidx (src, any
 * index below cc_db_size, searchable or not) at T_init = tf = (x, y, theta), BEV pixels / radians as cc_query_result_t.tf.
 * Several items may name the same descriptor or the same database scan.  Nothing is gated, merged or sorted: item i in, row i
 * out.  Per item:
 *   corr_init    initProblem(src, tgt, T_init): the ellipse pairs are selected at T_init (correlation.h:85-96) and summed there
 *   n_pairs      the selected pairs; flags carries the problem's CC_QF_GMM_CAP / CC_QF_DESC_CAP bits, as a ranked entry does
 *   correlation, tf, iterations, termination
 *                calcCorrelation() from T_init (theta reported as atan2(sin, cos)) and the CC_PF_REFINED bit, when cfg->refine
 *                is 1, n_pairs > 0 and !((float)corr_init < cfg->min_corr) -- the test of contour_db.h:552-556 with the bar
 *                given by the caller (-INFINITY: every item that has pairs).  Otherwise correlation is corr_init bit for bit,
 *                tf is T_init with the angle wrapped, iterations and termination are 0 and the bit is clear.
 *   try_corr     h_try_corr[i][t] = tryProblem(h_try[i][t]) for cfg->n_try poses per item: -cost(T_try) / sqrt(ac_src ac_tgt)
 *                over THE PAIR SET OF T_init (the refinement does not change that set; a T_try far from T_init "will cause
 *                problems", as the reference warns: the caller's business).  A problem without pairs gives 0.
 *   curvature    h_curv[i] (optional): Hessian and gradient of f = -correlation at the returned tf (at T_init for an item that
 *                was not refined): function, order and normalisation of cc_ranked_detail_t.hess / grad.  Zeros without pairs.
 * No threshold other than min_corr plays a role; cc_db_set_dynamic_thres does not apply.
 *
 * Refused with CC_EINVAL before anything is queued or collected (the handle and the chunks in flight stay untouched): NULL db,
 * d_qdesc, h_items, cfg or h_res; n < 0 (n == 0 is CC_OK); q outside [0, n_desc); gidx outside [0, cc_db_size); a non-finite
 * component of a tf or a try pose; refine other than 0 / 1; a NaN min_corr; n_try outside 0..CC_POSE_TRY_MAX; n_try > 0 with
 * h_try or h_try_corr NULL.
 *
 * Streaming: as cc_db_verify_submit -- chunks over the lanes (at most 1024 items each, 256 on a database with nnk > CC_KNN_MAX),
 * which wait for the last append on the device; the caller's stream continues once the descriptors are read; cc_db_query_wait
 * collects pose chunks too, and every output buffer must stay valid until then.  cc_db_query_collect is keyed by
 * cc_query_result_t ranges and does NOT see pose chunks.  CC_ECAPACITY as for queries (a flagged row, a pool that overflowed:
 * all rows are still delivered).  With cc_db_profile_enable the problem-building kernel lands in ms_out[0], slots 1 and 2 stay
 * zero, the correlation kernels (with the evaluation of the try poses and the curvature) in ms_out[3], the output kernel in
 * ms_out[4]. */
#define CC_POSE_TRY_MAX 8
#define CC_PF_REFINED 0x100 /* cc_pose_result_t.flags: the item was refined (beside the CC_QF_GMM_CAP / CC_QF_DESC_CAP bits) */
typedef struct {
  int32_t q, gidx; /* descriptor index (tgt), database scan (src) */
  double tf[3];    /* T_init = (x, y, theta)                      */
} cc_pose_item_t; /* 32 bytes */
typedef struct {
  int32_t refine; /* 1: run calcCorrelation() on the items that pass min_corr, 0: initProblem / tryProblem only */
  float min_corr; /* items with (float)corr_init below it are not refined; -INFINITY: no bar                   */
  int32_t n_try;  /* try poses per item, 0..CC_POSE_TRY_MAX (one count per call)                                */
  int32_t pad_;
} cc_pose_cfg_t;
typedef struct {
  double corr_init, correlation, tf[3];
  int32_t n_pairs, iterations, termination, flags;
  int32_t pad_[2];
} cc_pose_result_t; /* 64 bytes */
typedef struct {
  double hess[6], grad[3]; /* as cc_ranked_detail_t.hess / grad */
} cc_pose_curv_t; /* 72 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_pose_item_t) == 32 && sizeof(cc_pose_result_t) == 64 && sizeof(cc_pose_curv_t) == 72, "pose records");
#else
_Static_assert(sizeof(cc_pose_item_t) == 32 && sizeof(cc_pose_result_t) == 64 && sizeof(cc_pose_curv_t) == 72, "pose records");
#endif
/* h_try: [n][n_try][3] or NULL; h_try_corr: [n][n_try] or NULL; h_curv: [n] or NULL (curvature not wanted) */
int cc_db_pose_submit(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const cc_pose_item_t *h_items, int n,
                      const cc_pose_cfg_t *cfg, const double *h_try, cc_pose_result_t *h_res, double *h_try_corr,
                      cc_pose_curv_t *h_curv, void *stream);
/* submit + cc_db_query_wait */
int cc_db_pose_batch(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const cc_pose_item_t *h_items, int n,
                     const cc_pose_cfg_t *cfg, const double *h_try, cc_pose_result_t *h_res, double *h_try_corr,
                     cc_pose_curv_t *h_curv, void *stream);
/* ... with host descriptors: one H2D copy of them, like cc_db_verify_batch_host */
int cc_db_pose_batch_host(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const cc_pose_item_t *h_items, int n,
                          const cc_pose_cfg_t *cfg, const double *h_try, cc_pose_result_t *h_res, double *h_try_corr,
                          cc_pose_curv_t *h_curv);

/* ---- packed records and stored scans as the query of the three flows ----
 * The scoring chain reads a query scan only through the two compact records cc_pack_scans makes of its descriptor (below: "the
 * compact per-scan records") -- the records the database keeps per scan and the ranks exchange.  The _packed forms take the
 * query from such records instead of from 169 KB descriptors: rows of a caller's arrays (a second session's map, records
 * gathered from another rank) or the database's own rows (a re-check among scans of the map, the replay of a finished drive).
 * The chunk's prep stage is then one copy kernel (csrc/k_prep_packed.h) in the place of the two that build the records.
 *
 * Source: d_hot / d_feat are device arrays of n_rec records each (cc_packed_sizes), both bases 16-byte aligned; both NULL
 * names the database's own records, and n_rec is then cc_db_size at the call (a scan that is only prepared is not part of it).
 *
 * Each form carries the most general argument list of its flow: rank NULL is the plain call, rank with h_detail NULL the
 * _ranked call, both given the _ranked_detail call.  h_rec / h_qidx name the record of query / item i (NULL: record i);
 * cc_pose_item_t.q names a record.  The answers are, byte for byte, those of the descriptor form on the descriptors the records
 * were packed from: results, ranked lists, detail rows, generated hint lists, d_knn / d_knn_cnt, CC_QF_* flags and CC_ECAPACITY;
 * chunking, lanes, epochs, dynamic thresholds, large-k databases and collection (cc_db_query_wait / cc_db_query_collect) are
 * the descriptor form's.  Nothing is excluded on the caller's behalf: stored scan g queried at epoch g is the online loop's
 * query of scan g, at a later epoch the answer may be g itself; an item may name one stored scan as query and as candidate.
 * The caller's stream continues once the records are read.
 *
 * Refused with CC_EINVAL before anything is queued or collected: src NULL, exactly one of d_hot / d_feat NULL, n_rec < 1 with
 * caller arrays, a base that is not 16-byte aligned, a record index outside [0, n_rec), h_detail without rank, and whatever the
 * descriptor form of the call refuses. */
typedef struct {
  const void *d_hot;  /* [n_rec] hot records, device; NULL together with d_feat: the database's own records    */
  const void *d_feat; /* [n_rec] correlation inputs, device                                                    */
  int32_t n_rec;      /* records in the arrays; ignored for the database's own (then cc_db_size at the call)   */
  int32_t pad_;
} cc_packed_src_t;
int cc_db_query_submit_packed(cc_db *db, const cc_packed_src_t *src, const int32_t *h_rec, int nq, const int32_t *h_epoch,
                              const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn,
                              int32_t *d_knn_cnt, void *stream, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);
int cc_db_verify_submit_packed(cc_db *db, const cc_packed_src_t *src, const int32_t *h_qidx, const int32_t *h_cands, int n,
                               const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                               cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints, void *stream,
                               const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail);
int cc_db_pose_submit_packed(cc_db *db, const cc_packed_src_t *src, const cc_pose_item_t *h_items, int n, const cc_pose_cfg_t *cfg,
                             const double *h_try, cc_pose_result_t *h_res, double *h_try_corr, cc_pose_curv_t *h_curv, void *stream);

/* ---- masked queries: the retrieval restricted to a caller-given set of database scans ----
 * A query sees the database through its epoch, a prefix of the adding order.  A mask adds a set: the other session's scans but
 * not one's own last seconds, the scans near a position prior, everything but a retired key frame.  A masked query behaves
 * exactly as if the keys of every scan outside its set were not in the buckets' trees (in the reference's terms:
 * TreeBucket::data_tree_ and gkidx_tree_ filtered to the allowed scans, bucket_ranges_ left alone, then queryRangedKNN):
 * the search keeps the nnk nearest ALLOWED keys per anchor, which filtering an unmasked answer cannot give.  Epoch and mask
 * are ANDed; bucket ranges, thresholds and everything after the retrieval are unchanged.
 *
 * A mask is a table of bit rows: bit g & 31 of word g >> 5 of a row set = scan g may answer.  Query i names row h_row[i]
 * (many queries may share a row); -1 = no restriction.
 *
 * cc_db_query_submit_masked is the one masked form of cc_db_query_submit[_packed][_ranked[_detail]]: exactly one of d_qdesc
 * and src is given; src, h_rec, rank and h_detail mean what they mean in cc_db_query_submit_packed.  mask NULL is that call,
 * byte for byte and launch for launch.  A chunk in which some query names a row runs the one-wave-per-search retrieval
 * (the tiled search has no masked instance); a chunk in which none does runs the unmasked launches.
 * LIFETIME: `bits` is read by the lanes after the submit returns; it must stay unchanged until cc_db_query_wait or
 * cc_db_query_collect has delivered the chunk.  h_row is read before the submit returns.
 * Refused with CC_EINVAL (cc_last_error names the cause) before anything is queued: n_rows < 1 or row_words < 1; an h_row[i]
 * outside [-1, n_rows); 32 * row_words smaller than the largest epoch of a query that names a row; a database in
 * cc_db_set_dynamic_thres mode (no masked form of the replay exists); and whatever the unmasked call refuses.
 * cc_db_query_batch_host_masked: host descriptors and a host table, both staged by the call; synchronous.
 *
 * cc_mask_gates makes the rows of a position prior on the device: bit g of row r is set iff, in f32 as written,
 * dx = x_g - x_r, dy = y_g - y_r, dx * dx + dy * dy <= rad_r * rad_r, and rad_r >= 0.  A NaN anywhere or a negative radius sets
 * no bit; bits n_scans .. 32 * row_words - 1 are written as 0.  32 * row_words < n_scans is refused with CC_EINVAL.  The launch
 * is queued on `stream`. */
typedef struct cc_scan_mask {
  const uint32_t *bits; /* [n_rows][row_words]; device memory for the _submit form, host memory for the _host form */
  int32_t n_rows, row_words;
  const int32_t *h_row; /* [nq] host: the row of query i, or -1: every scan may answer */
} cc_scan_mask_t;
int cc_db_query_submit_masked(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_packed_src_t *src, const int32_t *h_rec, int nq,
                              const int32_t *h_epoch, const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res,
                              cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream, const cc_rank_out_t *rank,
                              cc_ranked_detail_t *h_detail, const cc_scan_mask_t *mask);
int cc_db_query_batch_host_masked(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch,
                                  const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res,
                                  const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail, const cc_scan_mask_t *mask);
int cc_mask_gates(cc_ctx *ctx, const float *d_xy /*[n_scans][2]*/, int n_scans, const float *d_gate /*[n_rows][3]: x, y, radius*/,
                  int n_rows, uint32_t *d_bits /*[n_rows][row_words]*/, int row_words, void *stream);
/* Parity / debug: the query chunks submitted on this handle so far, by the retrieval they ran: out[0] one wave per search,
 * out[1] the tiled search, out[2] the masked walk. */
int cc_db_debug_knn_chunks(const cc_db *db, int64_t out[3]);

/* Parity / debug: the constellations of the LAST cc_db_check_hints[_host] call that passed all four gates, in hint
 * order: the pose getTFFromConstell returned for each (contour_mng.h:1246-1277, before any proposal merging) and the
 * constellation it was computed from, so that a test can redo the rigid fit independently (e.g. with an SVD). */
typedef struct {
  int32_t hint;          /* index into the call's hint array                                   */
  int32_t n_pairs;       /* contours pairs in the constellation                                */
  double tf[3];          /* T_pass = (x, y, theta), BEV pixel units / radians                  */
  uint64_t pairs[7];     /* the pairs as a set: bit (level-1)*100 + seq_src*10 + seq_tgt       */
} cc_pass_dbg_t;
int cc_db_debug_passes(cc_db *db, cc_pass_dbg_t *h_out, int cap, int *n_out);

/* ---- the compact per-scan records (multi-GPU exchange) ----
 * cc_pack_scans turns full descriptors into the two records the database keeps per scan: the hot record
 * (cc_hot_desc_t, 18 KB) and the correlation inputs (opaque, 41 KB; cc_packed_sizes gives both sizes).  A rank packs
 * the scans it ingested, the ranks all-gather the two arrays over RCCL (59 KB per scan instead of the 169 KB
 * descriptor), and every rank appends the gathered scans to its replica with cc_db_add_packed -- the same effect as
 * cc_db_add_scans on the full descriptors (which is pack + add_packed).  d_hot_out / d_feat_out: device arrays of n
 * records each. */
void cc_packed_sizes(size_t *hot_bytes, size_t *feat_bytes);
int cc_pack_scans(cc_ctx *ctx, const cc_scan_desc_t *d_desc, int n, void *d_hot_out, void *d_feat_out, void *stream);
int cc_db_add_packed(cc_db *db, const void *d_hot, const void *d_feat, int n, const double *h_ts, const int32_t *h_seed,
                     void *stream);
/* Device pointers of the DB's own record arrays ([cc_db_size()] records each). */
const void *cc_db_hot_ptr(const cc_db *db);
const void *cc_db_feat_ptr(const cc_db *db);

/* Same for the query kernels: accumulated ms {K3 knn, K4 check, K4b merge, K5 gmm, K6 final} summed over the chunk
 * launches (chunks in flight together overlap in time), and the number of QUERIES the sums cover (*n_launches).
 * on = 0: off; 1: every chunk carries the six stage events; n > 1: every n-th chunk does (the events cost throughput:
 * ~7 % on the bench when every chunk is timed; the sums are normalised by the queries they cover either way). */
int cc_db_profile_enable(cc_db *db, int on);
int cc_db_profile_read(cc_db *db, double ms_out[5], int *n_launches);

/* cc_db_query_batch cuts a batch into one chunk per lane (<= 1024 queries each; a streamed cc_db_query_submit of 1024
 * queries or more goes out in chunks of 1024, batch after batch on alternating lanes) and keeps up to two chunks in
 * flight on internal streams
 * (the f64-bound correlation of one chunk overlaps the latency-bound retrieval/checks of the next).  n = 1 runs the
 * chunks one after the other (per-kernel timing, debugging); default 2.  No reference counterpart. */
int cc_db_set_lanes(cc_db *db, int n);
/* The reference's DYNAMIC_THRES=1 build (see cc_db_query_batch, thres_ub): on = 1 raises the bars from check to check and from
 * candidate to candidate, on = 0 (the default) keeps them constant.  The mode applies to every query entry point (batch,
 * submit, host, scan, scan batch, hints) called after this; chunks already submitted keep the mode they were submitted
 * with.  on other than 0 / 1 or a NULL db: CC_EINVAL.  The first switch to 1 allocates ~19 MB per query lane. */
int cc_db_set_dynamic_thres(cc_db *db, int on);

/* Host-side introspection of the K0 bookkeeping for parity tests:
 * tree sizes per (layer, bucket) and bucket ranges at the current epoch. */
int cc_db_bucket_state(const cc_db *db, int32_t *tree_sizes /*[3][6]*/, float *ranges /*[3][7]*/);

/* ---- the multi-GPU exchange, owned by the library ----
 * One process per GPU.  The path has ONE collective: the all-gather of the compact per-scan records (cc_pack_scans ->
 * cc_db_add_packed on every rank; 59 KB per scan) over RCCL / xGMI -- ncclAllGather, no all-reduce anywhere.  The reference
 * has no counterpart (it is a single-process CPU library); these calls are what a C++ multi-GPU driver binds
 * (hostcpp/examples/batch_replay_mgpu.cpp) and what bench.py --comm-owner c reaches through ctypes.  RCCL is loaded with
 * dlopen at the first call: a single-GPU process never touches it.
 *   cc_comm_unique_id        : rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the others by any means
 *   cc_comm_create           : ncclCommInitRank on `device` (collective over the world)
 *   cc_comm_create_from_env  : the two above for a launcher that sets RANK / WORLD_SIZE / LOCAL_RANK / MASTER_PORT
 *                              (torch.distributed.run, batch_replay_mgpu's forker) on ONE node: the id travels through a
 *                              file under /dev/shm named after MASTER_PORT
 *   cc_comm_allgather_packed : d_send = this rank's bytes_per_rank bytes, d_recv = world x bytes_per_rank, rank-major;
 *                              queued on `stream` (hipStream_t)
 * UNMEASURED on hardware with more than one rank: the build boxes have one GPU (world = 1 runs there: tests/test_gpu_comm.py). */
typedef struct cc_comm cc_comm;
int cc_comm_unique_id(void *id128);
int cc_comm_create(int device, int rank, int world, const void *id128, cc_comm **out);
int cc_comm_create_from_env(cc_comm **out, int *rank_out, int *world_out);
int cc_comm_rank(const cc_comm *comm);
int cc_comm_world(const cc_comm *comm);
int cc_comm_allgather_packed(cc_comm *comm, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
int cc_comm_destroy(cc_comm *comm);

/* ------------------------------------------------------------ pose helpers (host) ------- */
/* ConstellCorrelation::getEstSensTF (correlation.h:287-296): BEV-frame T_delta -> sensor
 * frame. in/out = (x, y, theta). */
void cc_est_sens_tf(const double tf_bev[3], int n_row, int n_col, double tf_sens[3]);
/* cc_ranked_detail_t.hess (xx, xy, xt, yy, yt, tt; BEV frame, at the pose tf_bev) for the parameters cc_est_sens_tf returns:
 * J^-T H J^-1 with J = d tf_sens / d tf_bev (identity on the translation, theta column = dR/dtheta * (n_row/2 - 0.5, n_col/2 - 0.5)).
 * The first-order change of variables: exact where the gradient vanishes, so use it where cc_ranked_detail_t.grad ~ 0. */
void cc_est_sens_info(const double hess_bev[6], const double tf_bev[3], int n_row, int n_col, double hess_sens[6]);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_H */
