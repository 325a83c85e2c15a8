// Test program (CPU harness or GPU): the class mirror's makeBEV with a sensor transform (hostcpp/cont2/contour_mng.h) gives the
// descriptor of makeBEV on the cloud transformed on the host with the library's stated f32 operation order
// (x' = ((m00 x + m01 y) + m02 z) + m03, every product and sum rounded once: build with -ffp-contract=off).
// usage: make_bev_tf_check <file.bin> <12 matrix values, row-major 3 x 4>      prints "ok <points> <contours>" or the first difference
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

int main(int argc, char **argv) {
  if (argc != 14) return 2;
  float T[12];
  for (int i = 0; i < 12; i++) T[i] = (float)atof(argv[2 + i]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  auto raw = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
  float rec[4];
  while (fread(rec, sizeof(float), 4, f) == 4) {
    pcl::PointXYZ p;
    p.x = rec[0];
    p.y = rec[1];
    p.z = rec[2];
    p.pad_ = rec[3];  // (whatever the file holds there: the rasteriser must not read it)
    raw->points.push_back(p);
  }
  fclose(f);
  auto moved = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
  for (const auto &p : raw->points) {
    pcl::PointXYZ q;
    q.x = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
    q.y = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
    q.z = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
    q.pad_ = 0.f;
    moved->points.push_back(q);
  }
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourManager a(config, 0), b(config, 1), c(config, 2);
  pcl::PointCloud<pcl::PointXYZ>::ConstPtr craw = raw, cmoved = moved;
  a.makeBEV<pcl::PointXYZ>(craw, T, "fused");
  b.makeBEV<pcl::PointXYZ>(cmoved, "host");
  c.makeBEV<pcl::PointXYZ>(craw, "untransformed");
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
    printf("the transform changed nothing: the check shows nothing\n");
    return 1;
  }
  int nc = 0;
  for (int l = 0; l < CC_NLEV; l++) nc += da->n_cont[l];
  printf("ok %zu %d\n", raw->size(), nc);
  return 0;
}
