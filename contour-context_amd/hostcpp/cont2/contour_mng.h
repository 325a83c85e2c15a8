// Host mirror of the reference's include/cont2/contour.h + contour_mng.h public surface, on top of the C-ABI
// (include/cont2_amd.h).  Same names, argument meaning and error behaviour (CHECK -> abort) as used by
// test/batch_bin_test.cpp and include/eval/evaluator.h; the work itself runs in the HIP kernels.
#pragma once
#include <fstream>
#include <iostream>
#include <array>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/cont2_amd.h"
#include "../../../include/cont2_amd_images.h"
#include "../../../include/cont2_amd_filter.h"
#include "../../../include/cont2_amd_coords.h"
#include "../../../include/cont2_amd_rig.h"
#include "../compat/compat.h"

typedef float KeyFloatType;
const int RET_KEY_DIM = CC_KEY_DIM;

// contour_mng.h:39-90
template <size_t sz>
struct ArrayAsKey {
  enum { SizeAtCompileTime = sz };
  KeyFloatType array[sz]{};
  KeyFloatType *data() { return array; }
  KeyFloatType &operator()(size_t i) { return array[i]; }
  const KeyFloatType &operator()(size_t i) const { return array[i]; }
  KeyFloatType &operator[](size_t i) { return array[i]; }
  const KeyFloatType &operator[](size_t i) const { return array[i]; }
  size_t size() const { return sz; }
  KeyFloatType sum() const {
    KeyFloatType ret(0);
    for (const auto &dat : array) ret += dat;
    return ret;
  }
};
using RetrievalKey = ArrayAsKey<RET_KEY_DIM>;

// contour.h:40-45
struct ContourSimThresConfig {
  float ta_cell_cnt = 6, tp_cell_cnt = 0.2;
  float tp_eigval = 0.2;
  float ta_h_bar = 0.3;
  float ta_rcom = 0.4, tp_rcom = 0.25;
};

// contour_mng.h:92-110
struct ContourManagerConfig {
  std::vector<float> lv_grads_;
  float reso_row_ = 1.0f, reso_col_ = 1.0f;
  int n_row_ = 150, n_col_ = 150;
  float lidar_height_ = 2.0f;
  float blind_sq_ = 9.0f;
  int min_cont_key_cnt_ = 9;
  int min_cont_cell_cnt_ = 3;
  int piv_firsts_ = 6;
  int dist_firsts_ = 10;
  float roi_radius_ = 10.0f;
};

// contour_mng.h:121-219 (the three score unions; same member names)
union ScoreConstellSim {
  enum { SizeAtCompileTime = 3 };
  int data[SizeAtCompileTime]{};
  struct {
    int i_ovlp_sum, i_ovlp_max_one, i_in_ang_rng;
  };
  const int &overall() const { return i_in_ang_rng; }  // the value the stage is judged by
  int cnt() const { return i_in_ang_rng; }
  void print() const { printf("%d, %d, %d;", i_ovlp_sum, i_ovlp_max_one, i_in_ang_rng); }
  bool strictSmaller(const ScoreConstellSim &b) const {
    for (int i = 0; i < SizeAtCompileTime; i++)
      if (!(data[i] < b.data[i])) return false;
    return true;
  }
};
union ScorePairwiseSim {
  enum { SizeAtCompileTime = 2 };
  int data[SizeAtCompileTime]{};
  struct {
    int i_indiv_sim, i_orie_sim;
  };
  const int &overall() const { return i_orie_sim; }
  int cnt() const { return i_orie_sim; }
  void print() const { printf("%d, %d;", i_indiv_sim, i_orie_sim); }
  bool strictSmaller(const ScorePairwiseSim &b) const {
    for (int i = 0; i < SizeAtCompileTime; i++)
      if (!(data[i] < b.data[i])) return false;
    return true;
  }
};
union ScorePostProc {
  enum { SizeAtCompileTime = 3 };
  float data[SizeAtCompileTime]{};
  struct {
    float correlation, area_perc, neg_est_dist;
  };
  const float &overall() const { return correlation; }
  void print() const { printf("%6f, %6f%%, %6fm;", correlation, 100 * area_perc, neg_est_dist); }
  bool strictSmaller(const ScorePostProc &b) const {
    for (int i = 0; i < SizeAtCompileTime; i++)
      if (!(data[i] < b.data[i])) return false;
    return true;
  }
};

// contour_mng.h:221-240: one matched contour pair (the "hint" of CandidateManager::checkCandWithHint when it is an anchor)
struct ConstellationPair {
  int8_t level, seq_src, seq_tgt;
  ConstellationPair(int8_t l, int8_t s, int8_t t) : level(l), seq_src(s), seq_tgt(t) {}
  bool operator<(const ConstellationPair &a) const {
    if (level != a.level) return level < a.level;
    if (seq_src != a.seq_src) return seq_src < a.seq_src;
    return seq_tgt < a.seq_tgt;
  }
  bool operator==(const ConstellationPair &a) const { return level == a.level && seq_src == a.seq_src && seq_tgt == a.seq_tgt; }
};

// contour.h:97-119, read-only view over one cc_contour_t
struct ContourView {
  int16_t level_, poi_[2], cell_cnt_;
  float pos_mean_[2], pos_cov_[4], eig_vals_[2], eig_vecs_[4], eccen_, vol3_mean_, com_[2];
  bool ecc_feat_, com_feat_;
};

namespace cc_host {
inline cc_manager_cfg_t to_c(const ContourManagerConfig &c) {
  cc_manager_cfg_t m;
  cc_default_manager_cfg(&m);
  CC_CHECK(c.lv_grads_.size() == CC_NLEV);  // this build handles the shipped 6-level configs
  for (int i = 0; i < CC_NLEV; i++) m.lv_grads[i] = c.lv_grads_[i];
  m.reso_row = c.reso_row_;
  m.reso_col = c.reso_col_;
  m.n_row = c.n_row_;
  m.n_col = c.n_col_;
  m.lidar_height = c.lidar_height_;
  m.blind_sq = c.blind_sq_;
  m.min_cont_key_cnt = c.min_cont_key_cnt_;
  m.min_cont_cell_cnt = c.min_cont_cell_cnt_;
  m.piv_firsts = c.piv_firsts_;
  m.dist_firsts = c.dist_firsts_;
  m.roi_radius = c.roi_radius_;
  return m;
}
// one device context per process and config (the reference has no such object: created lazily).  The device is HIP
// device 0 unless the environment names another one (CC_DEVICE=<n>: one process per GPU in a multi-GPU deployment).
inline int device_id() {
  const char *e = getenv("CC_DEVICE");
  return e ? atoi(e) : 0;
}
// once per process: the device runtime, the code object and the streams a per-scan driver's context and database will use
// (cc_runtime_init) -- called by the constructors of ContourDB and of the evaluator mirror, i.e. before a driver's loop
inline void runtime_warm() {
  static std::once_flag once;
  std::call_once(once, [] {
    if (getenv("CC_NO_RUNTIME_INIT")) return;
    (void)cc_runtime_init(device_id(), 8);  // no device (the evaluator's bookkeeping alone needs none): whoever uses one reports it
  });
}
inline cc_ctx *context(const cc_manager_cfg_t &m) {
  static std::map<std::string, cc_ctx *> pool;
  static std::mutex pool_mu;  // drivers with several worker threads build ContourManagers of one configuration concurrently
  std::lock_guard<std::mutex> lk(pool_mu);
  std::string key((const char *)&m, sizeof(m));
  auto it = pool.find(key);
  if (it != pool.end()) return it->second;
  cc_ctx *c = nullptr;
  if (cc_create(device_id(), &m, 8, &c) != CC_OK) {
    fprintf(stderr, "cont2_amd: %s\n", cc_last_error());
    abort();
  }
  pool[key] = c;
  return c;
}
// What a driver's scan source knows about the scans AFTER the one the driver holds: their device handles (ingested ahead of
// time) and time stamps, in the order the driver will ask for them.  The evaluator mirror publishes its read-ahead here;
// ContourDB reads it to append those scans and queue their queries early (contour_db.h: "read-ahead of the database").
// A source that changes its mind (a jump in the scan list) calls invalidate(): every database that has worked ahead drops
// that work first (the scans it refers to are about to be released).
struct ScanLookahead {
  struct Entry {
    cc_scan *scan;
    double ts;
    const void *source;  // who published it (an evaluator): a database follows ONE source, the one its last scan came from
  };
  std::mutex mu;
  std::deque<Entry> upcoming;                        // under mu; the entries of one source are in that source's order
  std::map<int, std::function<void(const void *)>> on_invalidate;  // registered by the databases (driver thread only); argument: the source
  int next_token = 0;
  int subscribe(std::function<void(const void *)> f) {
    on_invalidate[next_token] = std::move(f);
    return next_token++;
  }
  void unsubscribe(int token) {
    on_invalidate.erase(token);
    on_release.erase(token);
  }
  // A scan handle is about to be released (its ContourManager dies): a database whose queued work refers to the handle drops
  // that work -- the address may be handed out again for a later scan, and a queued answer must never be matched by address
  // against a different scan (driver thread only, like invalidate()).
  std::map<int, std::function<void(cc_scan *)>> on_release;
  void subscribeRelease(int token, std::function<void(cc_scan *)> f) { on_release[token] = std::move(f); }
  void released(cc_scan *scan) {
    if (!scan) return;
    for (auto &f : on_release) f.second(scan);
    popFront(scan);
  }
  void push(cc_scan *scan, double ts, const void *source) {
    std::lock_guard<std::mutex> lk(mu);
    upcoming.push_back({scan, ts, source});
  }
  void popFront(cc_scan *scan) {  // the driver has taken the scan (the oldest one of its source)
    std::lock_guard<std::mutex> lk(mu);
    for (auto it = upcoming.begin(); it != upcoming.end(); ++it)
      if (it->scan == scan) {
        upcoming.erase(it);
        return;
      }
  }
  std::vector<Entry> snapshot(const void *source) {
    std::lock_guard<std::mutex> lk(mu);
    std::vector<Entry> v;
    for (const Entry &e : upcoming)
      if (e.source == source) v.push_back(e);
    return v;
  }
  void invalidate(const void *source) {  // driver thread: `source` is about to release what it has published
    for (auto &f : on_invalidate) f.second(source);
    std::lock_guard<std::mutex> lk(mu);
    for (auto it = upcoming.begin(); it != upcoming.end();) it = it->source == source ? upcoming.erase(it) : it + 1;
  }
};
inline ScanLookahead &lookahead() {
  static ScanLookahead h;
  return h;
}
}  // namespace cc_host

// contour_mng.h:414-1314 (public surface used by the drivers)
class ContourManager {
  static constexpr float VAL_ABS_INF_ = 1e3f;  // contour_mng.h:418: the "no point" height is -VAL_ABS_INF_
  const ContourManagerConfig cfg_;
  cc_manager_cfg_t ccfg_;
  int int_id_;
  std::string str_id_;
  // The scan on the device (cc_scan, include/cont2_amd.h): makeBEV writes the points straight into the context's pinned
  // staging buffer and queues rasterisation + contours + keys + BCIs; the descriptor stays on the device for
  // ContourDB::queryRangedKNN / addScan, its host copy (what the getters below read) is fetched on first use.
  cc_scan *scan_ = nullptr;
  bool want_images_ = false;
  const void *source_ = nullptr;  // mirror-only: the scan source that handed the scan out (ContourDB's read-ahead follows it)

 public:
  const void *scanSource() const { return source_; }
  void setScanSource(const void *src) { source_ = src; }
  explicit ContourManager(const ContourManagerConfig &config, int int_id) : cfg_(config), int_id_(int_id) {
    CC_CHECK(cfg_.n_col_ % 2 == 0);
    CC_CHECK(cfg_.n_row_ % 2 == 0);
    ccfg_ = cc_host::to_c(cfg_);
  }

  ~ContourManager() {
    cc_host::lookahead().released(scan_);  // (nobody may keep matching queued work against this address)
    cc_scan_release(scan_);
  }
  ContourManager(const ContourManager &) = delete;
  ContourManager &operator=(const ContourManager &) = delete;

  // Whether a scan's max-height image is brought back from the device (90 KB extra per scan).  On when the reference
  // would write its SAVE_MID_FILE artefacts (CMakeLists.txt:17), or switched on by the caller before makeBEV().
  static bool &keepImages() {
#if defined(SAVE_MID_FILE) && SAVE_MID_FILE
    static bool keep = true;
#else
    static bool keep = false;
#endif
    return keep;
  }

  // contour_mng.h:505: x,y,z of every point (KITTI layout, intensity unused) -> the device; the kernels are queued here
  // already (nothing of them is observable before makeContoursRecurs() in the reference either)
  template <typename PointType>
  void makeBEV(typename pcl::PointCloud<PointType>::ConstPtr &ptr_gapc, std::string str_id = "") {
    CC_CHECK(ptr_gapc);
    CC_CHECK(ptr_gapc->size() > 10);
    CC_CHECK(!scan_);
    cc_ctx *ctx = cc_host::context(ccfg_);
    const size_t n = ptr_gapc->size();
    float *dst = cc_stage_points(ctx, (int64_t)n);
    if (!dst) die();
    for (size_t i = 0; i < n; i++) {
      dst[4 * i] = ptr_gapc->points[i].x;
      dst[4 * i + 1] = ptr_gapc->points[i].y;
      dst[4 * i + 2] = ptr_gapc->points[i].z;
      dst[4 * i + 3] = 0.f;
    }
    want_images_ = keepImages();
    if (cc_scan_ingest(ctx, dst, (int64_t)n, want_images_ ? 1 : 0, &scan_) != CC_OK) die();
    str_id_ = !str_id.empty() ? std::move(str_id) : std::to_string(ptr_gapc->header.stamp);
  }

  // Mirror-only: makeBEV for a cloud that is not in the frame the BEV is built in (a tilted or offset sensor, a base-frame
  // extrinsic, a roll / pitch compensated scan).  T_bev_sensor: row-major 3 x 4 [R | t], applied on the device while the
  // rasteriser loads the points, x' = ((m00 x + m01 y) + m02 z) + m03 in f32 (cc_scan_ingest_points, include/cont2_amd.h): no
  // transformed copy of the cloud, and no repack either -- the cloud's own records go to the device as they are (x, y, z must
  // be three consecutive floats of PointType).
  template <typename PointType>
  void makeBEV(typename pcl::PointCloud<PointType>::ConstPtr &ptr_gapc, const float (&T_bev_sensor)[12], std::string str_id = "") {
    CC_CHECK(ptr_gapc);
    CC_CHECK(ptr_gapc->size() > 10);
    CC_CHECK(!scan_);
    static_assert(sizeof(PointType) % 4 == 0 && sizeof(PointType) <= CC_POINT_STRIDE_MAX, "makeBEV: a record the rasteriser's loaders do not take");
    const PointType &p0 = ptr_gapc->points[0];
    const char *base = reinterpret_cast<const char *>(&p0);
    CC_CHECK(reinterpret_cast<const char *>(&p0.y) == reinterpret_cast<const char *>(&p0.x) + 4);
    CC_CHECK(reinterpret_cast<const char *>(&p0.z) == reinterpret_cast<const char *>(&p0.x) + 8);
    cc_point_layout_t lay;
    lay.stride_bytes = (int32_t)sizeof(PointType);
    lay.xyz_offset = (int32_t)(reinterpret_cast<const char *>(&p0.x) - base);
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_points(ctx, base, &lay, (int64_t)ptr_gapc->size(), T_bev_sensor, want_images_ ? 1 : 0, &scan_) != CC_OK) die();
    str_id_ = !str_id.empty() ? std::move(str_id) : std::to_string(ptr_gapc->header.stamp);
  }

  // Mirror-only: ONE BEV from several clouds, each in a frame of its own -- the sensors of a multi-LiDAR rig with their extrinsics,
  // or the last few sweeps with their odometry poses (a local submap).  The scan is the clouds' points one after the other in the
  // order given, each moved by its own T_bev_sensor as in the overload above (nullptr: the cloud is in the BEV's frame already);
  // among points of equal height in a cell the first one in that order owns the cell.  The clouds' own records go to the device as
  // they are and are rasterised where they land (cc_scan_ingest_segments, include/cont2_amd.h): no transformed or concatenated
  // copy.  A cloud may be empty (a sensor that dropped a frame); together they must hold more than 10 points.
  template <typename PointType>
  struct BevSegment {
    typename pcl::PointCloud<PointType>::ConstPtr cloud;
    const float (*T_bev_sensor)[12] = nullptr;
  };
  template <typename PointType>
  void makeBEV(const std::vector<BevSegment<PointType>> &segments, std::string str_id = "") {
    CC_CHECK(!segments.empty() && segments.size() <= (size_t)CC_SEG_MAX);
    CC_CHECK(!scan_);
    static_assert(sizeof(PointType) % 4 == 0 && sizeof(PointType) <= CC_POINT_STRIDE_MAX, "makeBEV: a record the rasteriser's loaders do not take");
    std::vector<cc_point_segment_t> segs(segments.size());
    size_t total = 0;
    for (size_t i = 0; i < segments.size(); i++) {
      const auto &cloud = segments[i].cloud;
      CC_CHECK(cloud);
      cc_point_segment_t &g = segs[i];
      memset(&g, 0, sizeof(g));
      g.n_points = (int64_t)cloud->size();
      g.layout.stride_bytes = (int32_t)sizeof(PointType);
      if (cloud->size() > 0) {
        const PointType &p0 = cloud->points[0];
        const char *base = reinterpret_cast<const char *>(&p0);
        CC_CHECK(reinterpret_cast<const char *>(&p0.y) == reinterpret_cast<const char *>(&p0.x) + 4);
        CC_CHECK(reinterpret_cast<const char *>(&p0.z) == reinterpret_cast<const char *>(&p0.x) + 8);
        g.points = base;
        g.layout.xyz_offset = (int32_t)(reinterpret_cast<const char *>(&p0.x) - base);
      }
      if (segments[i].T_bev_sensor) {
        g.has_tf = 1;
        memcpy(g.tf, *segments[i].T_bev_sensor, sizeof(g.tf));
      }
      total += cloud->size();
    }
    CC_CHECK(total > 10);
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_segments(ctx, segs.data(), (int)segs.size(), want_images_ ? 1 : 0, &scan_) != CC_OK) die();
    str_id_ = !str_id.empty() ? std::move(str_id) : std::to_string(segments[0].cloud->header.stamp);
  }

  // Mirror-only: makeBEV for a sweep that is de-skewed while it is rasterised.  Every record of PointType carries a 4-byte time word
  // (CC_TIME_F32: Velodyne's `time`; CC_TIME_U32: Ouster's `t` in ns) at byte time_offset, and the point is moved by the knot matrix
  // of its time bin, b = trunc(clamp((t - t_begin) * scale, 0, K - 1)) -- knots.size() = K <= CC_MOTION_KNOTS_MAX row-major 3 x 4
  // matrices, e.g. from cc_motion_knots with the odometry's poses at the sweep's begin and end (cc_scan_ingest_points_motion,
  // include/cont2_amd.h).  For CC_TIME_U32 t_begin_or_bits holds the BITS of the u32 begin.  The cloud's own records go to the device
  // as they are: no pass that gathers a pose per point and writes a second copy.
  struct BevMotion {
    size_t time_offset = 0;
    int time_type = CC_TIME_F32;
    float t_begin_or_bits = 0.f;
    float scale = 0.f;
    std::vector<std::array<float, 12>> knots;
  };
  template <typename PointType>
  void makeBEV(typename pcl::PointCloud<PointType>::ConstPtr &ptr_gapc, const BevMotion &motion, std::string str_id = "") {
    CC_CHECK(ptr_gapc);
    CC_CHECK(ptr_gapc->size() > 10);
    CC_CHECK(!scan_);
    CC_CHECK(!motion.knots.empty() && motion.knots.size() <= (size_t)CC_MOTION_KNOTS_MAX);
    static_assert(sizeof(PointType) % 4 == 0 && sizeof(PointType) <= CC_POINT_STRIDE_MAX, "makeBEV: a record the rasteriser's loaders do not take");
    static_assert(sizeof(std::array<float, 12>) == 12 * sizeof(float), "makeBEV: the knots are passed as [K][12] floats");
    const PointType &p0 = ptr_gapc->points[0];
    const char *base = reinterpret_cast<const char *>(&p0);
    CC_CHECK(reinterpret_cast<const char *>(&p0.y) == reinterpret_cast<const char *>(&p0.x) + 4);
    CC_CHECK(reinterpret_cast<const char *>(&p0.z) == reinterpret_cast<const char *>(&p0.x) + 8);
    cc_point_layout_t lay;
    lay.stride_bytes = (int32_t)sizeof(PointType);
    lay.xyz_offset = (int32_t)(reinterpret_cast<const char *>(&p0.x) - base);
    cc_point_motion_t mo;
    mo.time_offset = (int32_t)motion.time_offset;
    mo.time_type = (int32_t)motion.time_type;
    mo.n_knots = (int32_t)motion.knots.size();
    mo.pad_ = 0;
    const float h_time[2] = {motion.t_begin_or_bits, motion.scale};
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_points_motion(ctx, base, &lay, &mo, (int64_t)ptr_gapc->size(), h_time, motion.knots[0].data(), want_images_ ? 1 : 0, &scan_) != CC_OK)
      die();
    str_id_ = !str_id.empty() ? std::move(str_id) : std::to_string(ptr_gapc->header.stamp);
  }

  // Mirror-only: makeBEV that DROPS points by a word of their own record while they are rasterised -- the moving-object classes of a
  // semantic segmentation (SemanticKITTI: class = label & 0xFFFF, 252 .. 259 are moving), a driver's noise tag, a subset of rings, an
  // intensity band (cc_scan_ingest_points_filtered, include/cont2_amd_filter.h).  `filter` is the C-ABI's struct as it is: offset and
  // type of the word inside PointType, then the class rule (shift, mask, n_classes, keep_other, keep_bits: bit c set = class c is
  // kept) or the f32 band (lo, hi).  The BEV is that of the kept points alone, in their order; the cloud's own records go to the
  // device as they are: no mask, gather and second copy.  T_bev_sensor: as in the overload above, or nullptr; the filter looks at the
  // record, not at the moved point.  The cloud must hold more than 10 records, however many are kept.
  struct BevFilter {
    cc_point_filter_t filter{};
    const float (*T_bev_sensor)[12] = nullptr;
  };
  template <typename PointType>
  void makeBEV(typename pcl::PointCloud<PointType>::ConstPtr &ptr_gapc, const BevFilter &flt, std::string str_id = "") {
    CC_CHECK(ptr_gapc);
    CC_CHECK(ptr_gapc->size() > 10);
    CC_CHECK(!scan_);
    static_assert(sizeof(PointType) % 4 == 0 && sizeof(PointType) <= CC_POINT_STRIDE_MAX, "makeBEV: a record the rasteriser's loaders do not take");
    const PointType &p0 = ptr_gapc->points[0];
    const char *base = reinterpret_cast<const char *>(&p0);
    CC_CHECK(reinterpret_cast<const char *>(&p0.y) == reinterpret_cast<const char *>(&p0.x) + 4);
    CC_CHECK(reinterpret_cast<const char *>(&p0.z) == reinterpret_cast<const char *>(&p0.x) + 8);
    cc_point_layout_t lay;
    lay.stride_bytes = (int32_t)sizeof(PointType);
    lay.xyz_offset = (int32_t)(reinterpret_cast<const char *>(&p0.x) - base);
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_points_filtered(ctx, base, &lay, &flt.filter, (int64_t)ptr_gapc->size(), flt.T_bev_sensor ? *flt.T_bev_sensor : nullptr,
                                       want_images_ ? 1 : 0, &scan_) != CC_OK)
      die();
    str_id_ = !str_id.empty() ? std::move(str_id) : std::to_string(ptr_gapc->header.stamp);
  }

  // Mirror-only: ONE BEV from a rig's clouds with ALL the steps of the three overloads above at once (cc_scan_ingest_rig,
  // include/cont2_amd_rig.h): every cloud is moved by its own T_bev_sensor, or -- motion -- de-skewed by ITS time words with its own slice
  // [knot0, knot0 + n_knots) of `knots` (bin = trunc(clamp((t - t_begin) * scale, 0, n_knots - 1)), the point moved by knot knot0 + bin;
  // fold the sensor's extrinsics into its knots), or left as it is; and a record is dropped when the rule of `flt` says so of the word at
  // the cloud's own filter_offset (-1: the cloud is not filtered).  ONE rule for all clouds: flt->filter's offset and flt->T_bev_sensor
  // are not read; flt may be nullptr when no cloud is filtered, `knots` empty when none is in motion mode.  The scan is the kept records
  // of the clouds one after the other in the order given; at most CC_RIG_SEG_MAX clouds, together more than 10 records.
  template <typename PointType>
  struct BevRigSegment {
    typename pcl::PointCloud<PointType>::ConstPtr cloud;
    const float (*T_bev_sensor)[12] = nullptr;
    bool motion = false;  // (not together with T_bev_sensor)
    size_t time_offset = 0;
    int time_type = CC_TIME_F32;
    float t_begin_or_bits = 0.f;
    float scale = 0.f;
    int knot0 = 0, n_knots = 0;
    int filter_offset = -1;
  };
  template <typename PointType>
  void makeBEV(const std::vector<BevRigSegment<PointType>> &segments, const std::vector<std::array<float, 12>> &knots, const BevFilter *flt,
               std::string str_id = "") {
    CC_CHECK(!segments.empty() && segments.size() <= (size_t)CC_RIG_SEG_MAX);
    CC_CHECK(knots.size() <= (size_t)CC_MOTION_KNOTS_MAX);
    CC_CHECK(!scan_);
    static_assert(sizeof(PointType) % 4 == 0 && sizeof(PointType) <= CC_POINT_STRIDE_MAX, "makeBEV: a record the rasteriser's loaders do not take");
    static_assert(sizeof(std::array<float, 12>) == 12 * sizeof(float), "makeBEV: the knots are passed as [K][12] floats");
    std::vector<cc_rig_segment_t> segs(segments.size());
    size_t total = 0;
    for (size_t i = 0; i < segments.size(); i++) {
      const BevRigSegment<PointType> &s = segments[i];
      CC_CHECK(s.cloud);
      CC_CHECK(!(s.motion && s.T_bev_sensor));
      cc_rig_segment_t &g = segs[i];
      memset(&g, 0, sizeof(g));
      g.n_points = (int64_t)s.cloud->size();
      g.layout.stride_bytes = (int32_t)sizeof(PointType);
      if (s.cloud->size() > 0) {
        const PointType &p0 = s.cloud->points[0];
        const char *base = reinterpret_cast<const char *>(&p0);
        CC_CHECK(reinterpret_cast<const char *>(&p0.y) == reinterpret_cast<const char *>(&p0.x) + 4);
        CC_CHECK(reinterpret_cast<const char *>(&p0.z) == reinterpret_cast<const char *>(&p0.x) + 8);
        g.points = base;
        g.layout.xyz_offset = (int32_t)(reinterpret_cast<const char *>(&p0.x) - base);
      }
      g.mode = s.motion ? CC_RIG_MOTION : s.T_bev_sensor ? CC_RIG_TF : CC_RIG_NONE;
      if (s.T_bev_sensor) memcpy(g.tf, *s.T_bev_sensor, sizeof(g.tf));
      g.time_offset = (int32_t)s.time_offset;
      g.time_type = (int32_t)s.time_type;
      g.t_begin = s.t_begin_or_bits;
      g.scale = s.scale;
      g.knot0 = (int32_t)s.knot0;
      g.n_knots = (int32_t)s.n_knots;
      g.filter_offset = (int32_t)s.filter_offset;
      total += s.cloud->size();
    }
    CC_CHECK(total > 10);
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_rig(ctx, segs.data(), (int)segs.size(), knots.empty() ? nullptr : knots[0].data(), (int)knots.size(), flt ? &flt->filter : nullptr,
                           want_images_ ? 1 : 0, &scan_) != CC_OK)
      die();
    str_id_ = !str_id.empty() ? std::move(str_id) : std::to_string(segments[0].cloud->header.stamp);
  }

  // Mirror-only: makeBEV from coordinates of another TYPE or SHAPE than a pcl cloud's three consecutive floats (cc_scan_ingest_coords,
  // include/cont2_amd_coords.h): f64 clouds (Eigen / numpy / Open3D arrays, PCD files with double fields, everything in a georeferenced
  // frame), scaled int32 X, Y, Z (the LAS convention), and x, y, z held as three columns or apart inside a record.  x, y, z point at
  // the first point's elements, `type` is CC_COORD_F32 / _F64 / _I32 for all three, stride_bytes lies between consecutive points;
  // scale: CC_COORD_I32 only.  Every coordinate becomes p = (float)((double)v [* scale] - origin), each step rounded once: the origin
  // (3 doubles, e.g. the UTM position of the local frame; nullptr: none) is subtracted in f64 BEFORE the narrowing, which a cast in the
  // caller's code gets wrong by up to 0.5 m at a UTM northing.  The BEV is that of the f32 points p, moved by T_bev_sensor if given.
  // The coordinates go to the device as they are: no cast, subtraction, packing and second copy on the host.  n > 10.
  struct BevCoords {
    const void *x = nullptr, *y = nullptr, *z = nullptr;
    int32_t type = CC_COORD_F64;
    int32_t stride_bytes = 24;
    double scale[3] = {1.0, 1.0, 1.0};
    const double *origin = nullptr;
    int64_t n = 0;
  };
  void makeBEV(const BevCoords &crd, const float (*T_bev_sensor)[12] = nullptr, std::string str_id = "") {
    CC_CHECK(crd.n > 10);
    CC_CHECK(!scan_);
    cc_coord_src_t src;
    src.x = crd.x;
    src.y = crd.y;
    src.z = crd.z;
    src.type = crd.type;
    src.stride_bytes = crd.stride_bytes;
    for (int k = 0; k < 3; k++) src.scale[k] = crd.scale[k];
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_coords(ctx, &src, crd.n, crd.origin, T_bev_sensor ? *T_bev_sensor : nullptr, want_images_ ? 1 : 0, &scan_) != CC_OK) die();
    str_id_ = std::move(str_id);
  }

  // Mirror-only: makeBEV for a scan that is still the sensor's RANGE IMAGE -- H x W range words (u16 / u32 / f32) as the driver has them,
  // no x, y, z.  The sensor's model (beam altitudes and azimuth offsets, the firings' encoder azimuths, the knot of every firing) is
  // made once with rangeSensor() and shared by every scan; the points are computed while the rasteriser loads the words, and with
  // knots.size() = K >= 1 row-major 3 x 4 matrices (K as the sensor was made with; e.g. from cc_motion_knots) every pixel is moved by
  // the knot of ITS COLUMN: the sweep is de-skewed without a time word (cc_scan_ingest_ranges, include/cont2_amd.h, has the
  // arithmetic).  A word of 0 (f32: a word that is not > 0) is a pixel without a return.
  struct RangeImage {
    const cc_range_sensor *sensor = nullptr;
    const void *words = nullptr;  // n_rows * n_cols words of the sensor's type, in its storage order, aligned to their size
    std::vector<std::array<float, 12>> knots;  // empty for a sensor without knots
  };
  // the sensor for scans of this configuration (cc_range_sensor_create on its context); given back with releaseRangeSensor().  The
  // mirror remembers the K a sensor was made with: the C call sees only whether knots are there, not how many.
  static cc_range_sensor *rangeSensor(const ContourManagerConfig &config, const cc_range_model_t &model) {
    cc_range_sensor *s = nullptr;
    if (cc_range_sensor_create(contextOf(config), &model, &s) != CC_OK) die();
    std::lock_guard<std::mutex> lk(rangeSensorMutex());
    rangeSensorKnots()[s] = (int)model.n_knots;
    return s;
  }
  static void releaseRangeSensor(cc_range_sensor *sensor) {
    {
      std::lock_guard<std::mutex> lk(rangeSensorMutex());
      rangeSensorKnots().erase(sensor);
    }
    cc_range_sensor_destroy(sensor);
  }
  void makeBEV(const RangeImage &image, std::string str_id = "") {
    CC_CHECK(image.sensor && image.words);
    CC_CHECK(!scan_);
    {
      std::lock_guard<std::mutex> lk(rangeSensorMutex());
      const auto it = rangeSensorKnots().find(image.sensor);
      CC_CHECK(it != rangeSensorKnots().end());               // a sensor made by rangeSensor()
      CC_CHECK(image.knots.size() == (size_t)it->second);     // exactly the K matrices it was made with
    }
    static_assert(sizeof(std::array<float, 12>) == 12 * sizeof(float), "makeBEV: the knots are passed as [K][12] floats");
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_ranges(ctx, image.sensor, image.words, image.knots.empty() ? nullptr : image.knots[0].data(), want_images_ ? 1 : 0, &scan_) != CC_OK)
      die();
    str_id_ = std::move(str_id);
  }

  // Mirror-only: makeBEV for a scan that already IS a max-height image (cc_scan_ingest_image, include/cont2_amd_images.h, has the
  // rules): n_row_ * n_col_ image heights (z + lidar_height_, what getBevImage() returns), row-major, and optionally the continuous
  // (row_f, col_f) of every occupied cell's point -- the reference's bev_pixfs_, from which resumeImage() rebuilds bev_; without them
  // the cell centres.  min_height (has_min) becomes the descriptor's min_bin_val: an image cannot tell the lowest accepted point.  getBevImage()
  // of a manager made from a cloud, fed back with its pillar positions and its minimum, gives that manager's contours again.
  struct HeightImage {
    const float *height;
    const float *pos_rc = nullptr;
    bool has_min = false;
    float min_height = 0;
  };
  void makeBEV(const HeightImage &image, std::string str_id = "") {
    CC_CHECK(image.height);
    CC_CHECK(!scan_);
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest_image(ctx, image.height, image.pos_rc, image.has_min ? &image.min_height : nullptr, want_images_ ? 1 : 0, &scan_) != CC_OK) die();
    str_id_ = std::move(str_id);
  }

 private:
  static std::mutex &rangeSensorMutex() {
    static std::mutex mu;
    return mu;
  }
  static std::map<const cc_range_sensor *, int> &rangeSensorKnots() {
    static std::map<const cc_range_sensor *, int> m;
    return m;
  }

 public:
  // Mirror-only: the evaluator's .bin reader (tools/pointcloud_util.h:9-47: at most 1 000 000 floats, x y z i records,
  // intensity dropped) without the intermediate cloud.  A KITTI record IS a staging record (the kernels never read the
  // fourth float), so the file is read straight into the context's pinned buffer.  Returns the number of points.
  size_t makeBEVFromKittiBin(FILE *f, std::string str_id) {
    CC_CHECK(f);
    CC_CHECK(!scan_);
    cc_ctx *ctx = cc_host::context(ccfg_);
    const size_t cap = 1000000 / 4;
    float *dst = cc_stage_points(ctx, (int64_t)cap);
    if (!dst) die();
    const size_t n = fread(dst, 4 * sizeof(float), cap, f);
    CC_CHECK(n > 10);
    want_images_ = keepImages();
    if (cc_scan_ingest(ctx, dst, (int64_t)n, want_images_ ? 1 : 0, &scan_) != CC_OK) die();
    str_id_ = std::move(str_id);
    return n;
  }

  // Mirror-only: n KITTI records already sitting in one of the context's staging buffers (cc_stage_points_slot), e.g. read
  // there ahead of time by the evaluator's prefetch thread.
  void makeBEVFromStaged(const float *staged, size_t n, std::string str_id) {
    CC_CHECK(staged);
    CC_CHECK(n > 10);
    CC_CHECK(!scan_);
    cc_ctx *ctx = cc_host::context(ccfg_);
    want_images_ = keepImages();
    if (cc_scan_ingest(ctx, staged, (int64_t)n, want_images_ ? 1 : 0, &scan_) != CC_OK) die();
    str_id_ = std::move(str_id);
  }
  // Mirror-only: a scan that was ingested ahead of time (cc_scan_ingest on the evaluator's helper thread, with
  // want_bev = keepImages() at that moment); the handle is owned from here on.
  void adoptIngested(cc_scan *scan, bool with_images, std::string str_id) {
    CC_CHECK(scan);
    CC_CHECK(!scan_);
    scan_ = scan;
    want_images_ = with_images;
    str_id_ = std::move(str_id);
  }
  // the context the scans of this configuration are ingested on (one per ContourManagerConfig)
  static cc_ctx *contextOf(const ContourManagerConfig &config) { return cc_host::context(cc_host::to_c(config)); }

  // contour_mng.h:588: the work was queued by makeBEV; results are waited for where they are read
  void makeContoursRecurs() { CC_CHECK(scan_); }
  void clearImage() {}  // the dense image is never kept here (see bev_cells_)
  // contour_mng.h:562-571 rebuilds bev_ from the pillar list after clearImage(); here getBevImage() reads the copy that came
  // back from the device with the scan (keepImages() at makeBEV time), which clearImage() does not drop: nothing to rebuild
  void resumeImage() {}

  // contour_mng.h:573-586: the dense max-height image, -VAL_ABS_INF_ where no point fell
  cc_host::Image<float> getBevImage() const {
    cc_host::Image<float> img(cfg_.n_row_, cfg_.n_col_, -VAL_ABS_INF_);
    if (want_images_) {
      const float *bev = nullptr;
      if (cc_scan_bev(scan_, &bev) != CC_OK) die();
      std::memcpy(img.data.data(), bev, sizeof(float) * img.data.size());
    }
    return img;
  }
  // contour_mng.h:1041-1049: cv::threshold(bev, lv_grads_[level], THRESH_TOZERO) then cv::normalize(0, 255, NORM_MINMAX,
  // CV_8U).  Restated from OpenCV's documented semantics (OpenCV is absent here): TOZERO keeps src where src > thresh;
  // MINMAX maps [min, max] of that image to [0, 255] with scale = 255 / (max - min) (0 when max - min <= DBL_EPSILON),
  // shift = -min * scale, evaluated per pixel in f32 and rounded half-to-even with saturation (convertTo to CV_8U).
  cc_host::Image<unsigned char> getContourImage(int level) const {
    CC_CHECK(level >= 0 && level < (int)cfg_.lv_grads_.size());
    cc_host::Image<float> m = getBevImage();
    const float thr = cfg_.lv_grads_[level];
    double mn = 0, mx = 0;
    bool first = true;
    for (float &v : m.data) {
      v = v > thr ? v : 0.f;
      if (first || v < mn) mn = v;
      if (first || v > mx) mx = v;
      first = false;
    }
    const double scale = 255.0 * ((mx - mn) > 2.220446049250313e-16 ? 1.0 / (mx - mn) : 0.0), shift = 0.0 - mn * scale;
    const float a = (float)scale, b = (float)shift;
    cc_host::Image<unsigned char> out(m.rows, m.cols, 0);
    for (size_t i = 0; i < m.data.size(); i++) {
      const long r = lrintf(m.data[i] * a + b);
      out.data[i] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
    return out;
  }
  // contour_mng.cpp (saveContourImage): cv::imwrite(fpath, getContourImage(level))
  void saveContourImage(const std::string &fpath, int level) const {
    if (!cc_host::write_png_gray8(fpath, getContourImage(level))) std::cerr << "Error opening " << fpath << std::endl;
  }
  // contour_mng.h:1286-1311: the level images of two scans, cm1's on the top row and cm2's below, one column per level,
  // separated by one white pixel
  static void saveMatchedPairImg(const std::string &fpath, const ContourManager &cm1, const ContourManager &cm2) {
    const ContourManagerConfig config = cm2.getConfig();
    const int n_lev = (int)config.lv_grads_.size();
    cc_host::Image<unsigned char> output(config.n_row_ * 2 + 1, (config.n_col_ + 1) * n_lev, 255);
    for (int i = 0; i < n_lev; i++) {
      cm1.getContourImage(i).copyTo(output, i * config.n_col_ + i, 0);
      cm2.getContourImage(i).copyTo(output, i * config.n_col_ + i, config.n_row_ + 1);
    }
    if (!cc_host::write_png_gray8(fpath, output)) std::cerr << "Error opening " << fpath << std::endl;
  }

  static void die() {
    fprintf(stderr, "cont2_amd: %s\n", cc_last_error());
    abort();
  }
  // the host copy of everything the reference's ContourManager keeps after makeContoursRecurs() + clearImage()
  const cc_scan_desc_t &desc() const {
    CC_CHECK(scan_);
    const cc_scan_desc_t *d = nullptr;
    if (cc_scan_desc(scan_, &d) != CC_OK) die();  // includes CC_ECAPACITY: the reference has no capacities to exceed
    return *d;
  }
  cc_scan *scanHandle() const { return scan_; }
  const cc_manager_cfg_t &ccfg() const { return ccfg_; }
  std::vector<RetrievalKey> getLevRetrievalKey(int level) const {
    std::vector<RetrievalKey> r(cfg_.piv_firsts_);
    for (int s = 0; s < cfg_.piv_firsts_; s++) std::memcpy(r[s].array, desc().keys[level][s], sizeof(float) * RET_KEY_DIM);
    return r;
  }
  RetrievalKey getRetrievalKey(int level, int seq) const { return getLevRetrievalKey(level)[seq]; }
  // contour_mng.h:1066 (there: a const reference to the stored vector; here the views are rebuilt from the descriptor)
  std::vector<std::shared_ptr<ContourView>> getLevContours(int level) const {
    const cc_scan_desc_t &d = desc();
    std::vector<std::shared_ptr<ContourView>> v(d.n_stored[level]);
    for (int j = 0; j < d.n_stored[level]; j++) {
      const cc_contour_t &c = d.cont[level][j];
      v[j] = std::make_shared<ContourView>();
      ContourView &o = *v[j];
      o.level_ = c.level;
      o.poi_[0] = c.poi[0];
      o.poi_[1] = c.poi[1];
      o.cell_cnt_ = c.cell_cnt;
      std::memcpy(o.pos_mean_, c.pos_mean, 8);
      std::memcpy(o.pos_cov_, c.pos_cov, 16);
      std::memcpy(o.eig_vals_, c.eig_vals, 8);
      std::memcpy(o.eig_vecs_, c.eig_vecs, 16);
      o.eccen_ = c.eccen;
      o.vol3_mean_ = c.vol3_mean;
      std::memcpy(o.com_, c.com, 8);
      o.ecc_feat_ = c.ecc_feat;
      o.com_feat_ = c.com_feat;
    }
    return v;
  }
  int getLevTotalPix(int level) const { return desc().layer_cell_cnt[level]; }
  const cc_bci_t &getBCI(int level, int seq) const { return desc().bcis[level][seq]; }
  // contour_mng.h:1079: the level's BCIs, one per anchor key that exists (valid key <=> a non-zero retrieval key)
  std::vector<cc_bci_t> getLevBCI(int level) const {
    std::vector<cc_bci_t> v;
    const cc_scan_desc_t &d = desc();
    for (int s = 0; s < CC_NPIV; s++) {
      float sum = 0.f;
      for (int k = 0; k < CC_KEY_DIM; k++) sum += d.keys[level][s][k];
      if (sum != 0.f) v.push_back(d.bcis[level][s]);
    }
    return v;
  }
  float getAreaPerc(const int8_t &lev, const int8_t &seq) const {
    return desc().cont[lev][seq].cell_cnt * 1.0f / desc().layer_cell_cnt[lev];
  }
  // contour_mng.cpp:7-47 (saveContours) / contour_mng.h:915-918: the 20-column text dump scripts/plot_contours.py reads --
  // level, cell_cnt, pos_mean(2), pos_cov(4, column-major), eig_vals(2), eig_vecs(4), eccen, vol3_mean, com(2), ecc_feat,
  // com_feat; one row per stored contour, levels in order, between "DATA_START" and "DATA_END"
  void saveContours(const std::string &fpath) const {
    std::fstream out(fpath, std::ios::out);
    if (!out.good()) {
      std::cerr << "Error opening " << fpath << std::endl;
      return;
    }
    printf("Writing results to file \"%s\" ...", fpath.c_str());
    const cc_scan_desc_t &d = desc();
    out << "\nDATA_START\n";
    for (int l = 0; l < CC_NLEV; l++) {
      for (int j = 0; j < d.n_stored[l]; j++) {
        const cc_contour_t &c = d.cont[l][j];
        out << c.level << '\t' << c.cell_cnt << '\t' << c.pos_mean[0] << '\t' << c.pos_mean[1] << '\t';
        for (int i = 0; i < 4; i++) out << c.pos_cov[i] << '\t';
        out << c.eig_vals[0] << '\t' << c.eig_vals[1] << '\t';
        for (int i = 0; i < 4; i++) out << c.eig_vecs[i] << '\t';
        out << c.eccen << '\t' << c.vol3_mean << '\t' << c.com[0] << '\t' << c.com[1] << '\t' << int(c.ecc_feat) << '\t'
            << int(c.com_feat) << '\t' << '\n';
      }
    }
    out << "DATA_END\n";
    out.close();
    printf("Writing results finished.\n");
  }
  std::string getStrID() const { return str_id_; }
  int getIntID() const { return int_id_; }
  const ContourManagerConfig &getConfig() const { return cfg_; }
};
