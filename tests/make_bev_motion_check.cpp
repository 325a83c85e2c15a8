// Test program (CPU harness or GPU): the class mirror's makeBEV with a BevMotion (hostcpp/cont2/contour_mng.h) gives the descriptor of
// its single-cloud makeBEV on the cloud moved on the host: every point by the knot of its time bin, b = trunc(min(max((t - t_begin) *
// scale, 0), K - 1)) with NaN as 0, in the library's stated f32 operation order (x' = ((m00 x + m01 y) + m02 z) + m03, every product
// and sum rounded once: build with -ffp-contract=off).  The file holds x y z t records; the time rides in the record's fourth float.
// usage: make_bev_motion_check <file.bin> <t_begin> <scale> <K> <12 K values of the knots>    prints "ok <points> <contours>" or the first difference
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

typedef pcl::PointCloud<pcl::PointXYZ> Cloud;

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const float t_begin = (float)atof(argv[2]), scale = (float)atof(argv[3]);
  const int K = atoi(argv[4]);
  if (K < 1 || argc != 5 + 12 * K) return 2;
  ContourManager::BevMotion motion;
  motion.time_offset = offsetof(pcl::PointXYZ, pad_);
  motion.time_type = CC_TIME_F32;
  motion.t_begin_or_bits = t_begin;
  motion.scale = scale;
  motion.knots.resize((size_t)K);
  for (int i = 0; i < 12 * K; i++) motion.knots[(size_t)(i / 12)][(size_t)(i % 12)] = (float)atof(argv[5 + i]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::shared_ptr<Cloud> raw = std::make_shared<Cloud>(), moved = std::make_shared<Cloud>();
  float rec[4];
  int bins_seen = 0;
  std::vector<int> seen((size_t)K, 0);
  while (fread(rec, sizeof(float), 4, f) == 4) {
    pcl::PointXYZ p;
    p.x = rec[0];
    p.y = rec[1];
    p.z = rec[2];
    p.pad_ = rec[3];  // the time
    raw->points.push_back(p);
    float u = (p.pad_ - t_begin) * scale;
    u = u > 0.f ? u : 0.f;
    u = u < (float)(K - 1) ? u : (float)(K - 1);
    const int b = (int)u;
    if (!seen[(size_t)b]++) bins_seen++;
    const float *M = motion.knots[(size_t)b].data();
    pcl::PointXYZ m;
    m.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];
    m.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
    m.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
    m.pad_ = 0.f;
    moved->points.push_back(m);
  }
  fclose(f);
  if (bins_seen != K) {
    printf("only %d of %d bins are used: the check shows less than it should\n", bins_seen, K);
    return 1;
  }
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourManager a(config, 0), b(config, 1), c(config, 2);
  Cloud::ConstPtr craw = raw, cmoved = moved;
  a.makeBEV<pcl::PointXYZ>(craw, motion, "motion");
  b.makeBEV<pcl::PointXYZ>(cmoved, "host");
  c.makeBEV<pcl::PointXYZ>(craw, "uncompensated");
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
    printf("the knots changed nothing: the check shows nothing\n");
    return 1;
  }
  int nc = 0;
  for (int l = 0; l < CC_NLEV; l++) nc += da->n_cont[l];
  printf("ok %zu %d\n", raw->points.size(), nc);
  return 0;
}
