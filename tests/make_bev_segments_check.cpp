// Test program (CPU harness or GPU): the class mirror's makeBEV from several clouds, each with its own transform
// (hostcpp/cont2/contour_mng.h), gives the descriptor of the single-cloud makeBEV on Q = T_0(cloud 0) ++ T_1(cloud 1) ++ cloud 2, built
// on the host with the library's stated f32 operation order (x' = ((m00 x + m01 y) + m02 z) + m03, every product and sum rounded
// once: build with -ffp-contract=off).  The file's points are dealt to the clouds in three stretches; the third cloud has no matrix,
// and an empty cloud sits between the first two.
// usage: make_bev_segments_check <file.bin> <12 values of T_0> <12 values of T_1>     prints "ok <points> <contours>" or the first difference
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
  if (argc != 26) return 2;
  float T[2][12];
  for (int i = 0; i < 24; i++) T[i / 12][i % 12] = (float)atof(argv[2 + i]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<pcl::PointXYZ> all;
  float rec[4];
  while (fread(rec, sizeof(float), 4, f) == 4) {
    pcl::PointXYZ p;
    p.x = rec[0];
    p.y = rec[1];
    p.z = rec[2];
    p.pad_ = rec[3];  // (whatever the file holds there: the rasteriser must not read it)
    all.push_back(p);
  }
  fclose(f);
  const size_t n = all.size(), cut[4] = {0, n / 3 + 1, 2 * n / 3 + 5, n};
  std::shared_ptr<Cloud> part[3], q = std::make_shared<Cloud>(), plain = std::make_shared<Cloud>(), none = std::make_shared<Cloud>();
  for (int s = 0; s < 3; s++) {
    part[s] = std::make_shared<Cloud>();
    for (size_t i = cut[s]; i < cut[s + 1]; i++) {
      const pcl::PointXYZ &p = all[i];
      part[s]->points.push_back(p);
      pcl::PointXYZ m = p;
      if (s < 2) {
        const float *M = T[s];
        m.x = ((M[0] * p.x + M[1] * p.y) + M[2] * p.z) + M[3];
        m.y = ((M[4] * p.x + M[5] * p.y) + M[6] * p.z) + M[7];
        m.z = ((M[8] * p.x + M[9] * p.y) + M[10] * p.z) + M[11];
      }
      m.pad_ = 0.f;
      q->points.push_back(m);
      plain->points.push_back(p);
    }
  }
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourManager a(config, 0), b(config, 1), c(config, 2);
  std::vector<ContourManager::BevSegment<pcl::PointXYZ>> segs(4);
  segs[0].cloud = part[0];
  segs[0].T_bev_sensor = &T[0];
  segs[1].cloud = none;  // a sensor that dropped its frame
  segs[2].cloud = part[1];
  segs[2].T_bev_sensor = &T[1];
  segs[3].cloud = part[2];
  Cloud::ConstPtr cq = q, cplain = plain;
  a.makeBEV<pcl::PointXYZ>(segs, "segments");
  b.makeBEV<pcl::PointXYZ>(cq, "host");
  c.makeBEV<pcl::PointXYZ>(cplain, "untransformed");
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
    printf("the transforms changed nothing: the check shows nothing\n");
    return 1;
  }
  int nc = 0;
  for (int l = 0; l < CC_NLEV; l++) nc += da->n_cont[l];
  printf("ok %zu %d\n", n, nc);
  return 0;
}
