// Test program (CPU harness or GPU): the class mirror's makeBEV from a rig's clouds (hostcpp/cont2/contour_mng.h: BevRigSegment, a
// knot pool, one BevFilter) gives the descriptor of the single-cloud makeBEV on the cloud Q built on the host -- every record moved by
// its cloud's matrix or by the knot of its time bin within the cloud's slice of the pool, with the library's stated f32 operation
// order (build with -ffp-contract=off), and the records the class rule drops left out.  The file's points (x, y, z, label bits) are
// dealt to three clouds of 32-byte records in three stretches: the first de-skewed on the slice [0, 4) and filtered, the second moved
// by a matrix and filtered, the third de-skewed on [4, 8) with u32 times and not filtered; an empty cloud sits behind the first.
// usage: make_bev_rig_check <file.bin>     prints "ok <records> <kept> <contours>" or the first difference
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cont2/contour_mng.h"

static const char *desc_diff(const cc_scan_desc_t &x, const cc_scan_desc_t &y) {  // everything a descriptor defines
  if (memcmp(&x, &y, offsetof(cc_scan_desc_t, bcis)) != 0) return "counts / keys";
  for (int l = 0; l < CC_NLEV; l++) {
    for (int s = 0; s < CC_NPIV; s++) {
      const cc_bci_t &p = x.bcis[l][s], &q = y.bcis[l][s];
      if (memcmp(p.dist_bin, q.dist_bin, sizeof(p.dist_bin)) != 0 || p.piv_seq != q.piv_seq || p.level != q.level || p.n_pts != q.n_pts ||
          p.n_segs != q.n_segs)
        return "bci header";
      if (memcmp(p.segs, q.segs, sizeof(uint16_t) * p.n_segs) != 0) return "bci segments";
      if (memcmp(p.pts, q.pts, sizeof(cc_relpt_t) * p.n_pts) != 0) return "bci points";
    }
    if (memcmp(x.cont[l], y.cont[l], sizeof(cc_contour_t) * (size_t)x.n_stored[l]) != 0) return "contours";
  }
  return nullptr;
}

struct RigPoint {  // what a driver's record may look like: 32 bytes
  float x, y, z;
  union {
    float t;      // seconds
    uint32_t ns;  // or nanoseconds
  };
  uint32_t label;
  float other[3];
};
static_assert(sizeof(RigPoint) == 32, "RigPoint: 32 bytes");
typedef pcl::PointCloud<RigPoint> RigCloud;
typedef pcl::PointCloud<pcl::PointXYZ> Cloud;

static pcl::PointXYZ moved(const RigPoint &p, const float *M) {
  pcl::PointXYZ m;
  m.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];
  m.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
  m.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
  m.pad_ = 0.f;
  return m;
}
static int bin_of(float u, int n_knots) {
  u = u > 0.f ? u : 0.f;
  const float kmax = (float)(n_knots - 1);
  u = u < kmax ? u : kmax;
  return (int)u;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<RigPoint> all;
  float rec[4];
  while (fread(rec, sizeof(float), 4, f) == 4) {
    RigPoint p;
    memset(&p, 0xA5, sizeof(p));  // (whatever the other bytes hold: the rasteriser must not read them)
    p.x = rec[0];
    p.y = rec[1];
    p.z = rec[2];
    memcpy(&p.label, &rec[3], 4);
    all.push_back(p);
  }
  fclose(f);
  // a pool of 8: two slices of 4, every knot a yaw of a few degrees and a shift that grows with the knot
  std::vector<std::array<float, 12>> knots(8);
  for (int k = 0; k < 8; k++) {
    const float c = cosf(0.02f * (float)(k + 1)), s = sinf(0.02f * (float)(k + 1));
    knots[k] = {c, -s, 0.f, 0.75f * (float)k, s, c, 0.f, -0.5f * (float)k, 0.f, 0.f, 1.f, 0.0625f * (float)(k % 4)};
  }
  static const float T[12] = {0.96592583f, -0.25881905f, 0.f, 2.5f, 0.25881905f, 0.96592583f, 0.f, -1.25f, 0.f, 0.f, 1.f, 0.125f};  // 15 degrees of yaw and a shift
  const size_t n = all.size(), cut[4] = {0, n / 3 + 1, 2 * n / 3 + 5, n};
  const float t_begin = 3.0f, scale = 4.0f / 0.1f;           // cloud 0: f32 seconds, a sweep of 0.1 s from 3.0 on, a little past both ends
  const uint32_t ns_begin = 4286000000u;                     // cloud 2: u32 ns, wrapping past 2^32 inside the sweep
  const float ns_scale = 4.0f / 1.0e8f;
  std::shared_ptr<RigCloud> part[3], none = std::make_shared<RigCloud>();
  std::shared_ptr<Cloud> q = std::make_shared<Cloud>(), plain = std::make_shared<Cloud>();
  size_t dropped = 0;
  for (int s = 0; s < 3; s++) {
    part[s] = std::make_shared<RigCloud>();
    const size_t m = cut[s + 1] - cut[s];
    for (size_t i = cut[s]; i < cut[s + 1]; i++) {
      RigPoint p = all[i];
      const float frac = (float)(i - cut[s]) / (float)m;
      pcl::PointXYZ out;
      if (s == 0) {
        p.t = 2.995f + 0.11f * frac;
        out = moved(p, knots[0 + bin_of((p.t - t_begin) * scale, 4)].data());
      } else if (s == 1) {
        out = moved(p, T);
      } else {
        p.ns = ns_begin + (uint32_t)(1.04e8f * frac);
        out = moved(p, knots[4 + bin_of((float)(uint32_t)(p.ns - ns_begin) * ns_scale, 4)].data());
      }
      part[s]->points.push_back(p);
      const uint32_t cls = p.label & 0xFFFFu;
      pcl::PointXYZ raw;
      raw.x = p.x, raw.y = p.y, raw.z = p.z, raw.pad_ = 0.f;
      plain->points.push_back(raw);
      if (s < 2 && cls >= 252 && cls < 260) {
        dropped++;
        continue;
      }
      q->points.push_back(out);
    }
  }
  if (dropped == 0) {
    printf("the rule drops nothing: the check shows less than it should\n");
    return 1;
  }
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  uint32_t bits[(260 + 31) / 32];
  for (uint32_t &b : bits) b = 0xFFFFFFFFu;
  for (int c = 252; c < 260; c++) bits[c >> 5] &= ~(1u << (c & 31));
  ContourManager::BevFilter flt;
  flt.filter.offset = -12345;  // (not read)
  flt.filter.type = CC_FILTER_U32;
  flt.filter.shift = 0;
  flt.filter.mask = 0xFFFFu;
  flt.filter.n_classes = 260;
  flt.filter.keep_other = 1;
  flt.filter.keep_bits = bits;
  std::vector<ContourManager::BevRigSegment<RigPoint>> segs(4);
  segs[0].cloud = part[0];
  segs[0].motion = true;
  segs[0].time_offset = offsetof(RigPoint, t);
  segs[0].time_type = CC_TIME_F32;
  segs[0].t_begin_or_bits = t_begin;
  segs[0].scale = scale;
  segs[0].knot0 = 0;
  segs[0].n_knots = 4;
  segs[0].filter_offset = (int)offsetof(RigPoint, label);
  segs[1].cloud = none;  // a sensor that dropped its frame
  segs[2].cloud = part[1];
  segs[2].T_bev_sensor = &T;
  segs[2].filter_offset = (int)offsetof(RigPoint, label);
  segs[3].cloud = part[2];
  segs[3].motion = true;
  segs[3].time_offset = offsetof(RigPoint, ns);
  segs[3].time_type = CC_TIME_U32;
  memcpy(&segs[3].t_begin_or_bits, &ns_begin, 4);
  segs[3].scale = ns_scale;
  segs[3].knot0 = 4;
  segs[3].n_knots = 4;
  ContourManager a(config, 0), b(config, 1), c(config, 2);
  Cloud::ConstPtr cq = q, cplain = plain;
  a.makeBEV<RigPoint>(segs, knots, &flt, "rig");
  b.makeBEV<pcl::PointXYZ>(cq, "host");
  c.makeBEV<pcl::PointXYZ>(cplain, "as recorded");
  a.makeContoursRecurs();
  b.makeContoursRecurs();
  c.makeContoursRecurs();
  const cc_scan_desc_t *da = nullptr, *db = nullptr, *dc = nullptr;
  if (cc_scan_desc(a.scanHandle(), &da) != CC_OK || cc_scan_desc(b.scanHandle(), &db) != CC_OK || cc_scan_desc(c.scanHandle(), &dc) != CC_OK) {
    fprintf(stderr, "%s\n", cc_last_error());
    return 4;
  }
  if (const char *why = desc_diff(*da, *db)) {
    printf("differ: %s\n", why);
    return 1;
  }
  if (!desc_diff(*da, *dc)) {
    printf("the steps changed nothing: the check shows nothing\n");
    return 1;
  }
  int nc = 0;
  for (int l = 0; l < CC_NLEV; l++) nc += da->n_cont[l];
  printf("ok %zu %zu %d\n", n, q->points.size(), nc);
  return 0;
}
