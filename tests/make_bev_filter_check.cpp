// Test program (CPU harness or GPU): the class mirror's makeBEV with a BevFilter (hostcpp/cont2/contour_mng.h) gives the descriptor of
// its plain makeBEV on the cloud compacted on the host -- the kept points alone, in their order -- with and without T_bev_sensor (then
// against the overload that takes the matrix, on the compacted cloud).  The file holds x y z w records; the fourth word is a
// SemanticKITTI label: class in the low 16 bits (252 .. 259 are dropped), an instance id in the high 16 (ignored).  A second pass uses
// the range rule on the same word read as an f32.
// usage: make_bev_filter_check <file.bin> <lo> <hi>    prints "ok <points> <kept by class> <kept by range> <contours>" or the first difference
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

// 0: equal and the filter mattered; 1: a difference (printed)
static int compare(const ContourManagerConfig &config, Cloud::ConstPtr raw, Cloud::ConstPtr kept, const ContourManager::BevFilter &flt, const char *tag, int *n_cont) {
  ContourManager a(config, 0), b(config, 1), c(config, 2);
  a.makeBEV<pcl::PointXYZ>(raw, flt, "filtered");
  if (flt.T_bev_sensor) {
    b.makeBEV<pcl::PointXYZ>(kept, *flt.T_bev_sensor, "compacted");
    c.makeBEV<pcl::PointXYZ>(raw, *flt.T_bev_sensor, "unfiltered");
  } else {
    b.makeBEV<pcl::PointXYZ>(kept, "compacted");
    c.makeBEV<pcl::PointXYZ>(raw, "unfiltered");
  }
  a.makeContoursRecurs();
  b.makeContoursRecurs();
  c.makeContoursRecurs();
  const cc_scan_desc_t *da = nullptr, *db = nullptr, *dc = nullptr;
  if (cc_scan_desc(a.scanHandle(), &da) != CC_OK || cc_scan_desc(b.scanHandle(), &db) != CC_OK || cc_scan_desc(c.scanHandle(), &dc) != CC_OK) {
    fprintf(stderr, "%s\n", cc_last_error());
    return 1;
  }
  if (const char *why = desc_diff(*da, *db)) {
    printf("%s: differ: %s\n", tag, why);
    return 1;
  }
  if (!desc_diff(*da, *dc)) {
    printf("%s: the filter changed nothing: the check shows nothing\n", tag);
    return 1;
  }
  *n_cont = 0;
  for (int l = 0; l < CC_NLEV; l++) *n_cont += da->n_cont[l];
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const float lo = (float)atof(argv[2]), hi = (float)atof(argv[3]);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::shared_ptr<Cloud> raw = std::make_shared<Cloud>(), by_class = std::make_shared<Cloud>(), by_range = std::make_shared<Cloud>();
  float rec[4];
  while (fread(rec, sizeof(float), 4, f) == 4) {
    pcl::PointXYZ p;
    p.x = rec[0];
    p.y = rec[1];
    p.z = rec[2];
    p.pad_ = rec[3];  // the label's bits
    raw->points.push_back(p);
    uint32_t w;
    memcpy(&w, &rec[3], 4);
    const uint32_t cls = w & 0xFFFFu;
    pcl::PointXYZ q = p;
    q.pad_ = 0.f;
    if (!(cls >= 252 && cls < 260)) by_class->points.push_back(q);
    if (lo <= rec[3] && rec[3] <= hi) by_range->points.push_back(q);
  }
  fclose(f);
  if (by_class->points.size() == raw->points.size() || by_range->points.size() == raw->points.size()) {
    printf("a rule drops nothing: the check shows less than it should\n");
    return 1;
  }
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  uint32_t bits[(260 + 31) / 32];
  for (uint32_t &b : bits) b = 0xFFFFFFFFu;
  for (int c = 252; c < 260; c++) bits[c >> 5] &= ~(1u << (c & 31));
  ContourManager::BevFilter cls;
  cls.filter.offset = (int32_t)offsetof(pcl::PointXYZ, pad_);
  cls.filter.type = CC_FILTER_U32;
  cls.filter.shift = 0;
  cls.filter.mask = 0xFFFFu;
  cls.filter.n_classes = 260;
  cls.filter.keep_other = 1;
  cls.filter.keep_bits = bits;
  ContourManager::BevFilter band;
  band.filter.offset = (int32_t)offsetof(pcl::PointXYZ, pad_);
  band.filter.type = CC_FILTER_F32;
  band.filter.lo = lo;
  band.filter.hi = hi;
  static const float T[12] = {0.96592583f, -0.25881905f, 0.f, 2.5f, 0.25881905f, 0.96592583f, 0.f, -1.25f, 0.f, 0.f, 1.f, 0.125f};  // 15 degrees of yaw and a shift
  ContourManager::BevFilter cls_tf = cls;
  cls_tf.T_bev_sensor = &T;
  Cloud::ConstPtr craw = raw, ccls = by_class, crng = by_range;
  int nc = 0, nc2 = 0, nc3 = 0;
  if (compare(config, craw, ccls, cls, "class rule", &nc) || compare(config, craw, crng, band, "range rule", &nc2) ||
      compare(config, craw, ccls, cls_tf, "class rule with T_bev_sensor", &nc3))
    return 1;
  printf("ok %zu %zu %zu %d\n", raw->points.size(), by_class->points.size(), by_range->points.size(), nc);
  return 0;
}
