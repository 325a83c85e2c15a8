// Test program (CPU harness or GPU): the class mirror's makeBEV with a RangeImage (hostcpp/cont2/contour_mng.h) gives the descriptor of
// its single-cloud makeBEV on the cloud computed on the host by the header's formula -- f32, every product and sum rounded once, in
// its association (build with -ffp-contract=off) -- with every pixel moved by the knot of its column and a pixel without a return as
// a NaN point.  The file holds H * W u16 range words, row-major, in units of 2 mm; the sensor's angles are made here.
// usage: make_bev_range_check <file.bin> <H> <W> <K> <12 K values of the knots>    prints "ok <pixels> <contours>" or the first difference
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

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
  const int H = atoi(argv[2]), W = atoi(argv[3]), K = atoi(argv[4]);
  if (H < 1 || W < 1 || K < 1 || argc != 5 + 12 * K) return 2;
  std::vector<std::array<float, 12>> knots((size_t)K);
  for (int i = 0; i < 12 * K; i++) knots[(size_t)(i / 12)][(size_t)(i % 12)] = (float)atof(argv[5 + i]);
  std::vector<uint16_t> words((size_t)H * W);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  const size_t got = fread(words.data(), sizeof(uint16_t), words.size(), f);
  fclose(f);
  if (got != words.size()) return 3;
  // the sensor: beams from +2 to -24.8 degrees with a staggered azimuth offset, firings around the turn, the knot rising with the firing
  const double PI = 3.14159265358979323846;
  std::vector<float> row_tab((size_t)H * 4), col_cs((size_t)W * 2);
  std::vector<int32_t> col_knot((size_t)W);
  for (int r = 0; r < H; r++) {
    const double alt = (2.0 - 26.8 * r / (H > 1 ? H - 1 : 1)) * PI / 180.0, off = (-0.9 + 0.6 * (r % 4)) * PI / 180.0;
    row_tab[4 * r] = (float)cos(alt);
    row_tab[4 * r + 1] = (float)sin(alt);
    row_tab[4 * r + 2] = (float)cos(off);
    row_tab[4 * r + 3] = (float)sin(off);
  }
  for (int c = 0; c < W; c++) {
    col_cs[2 * c] = (float)cos(2 * PI * c / W);
    col_cs[2 * c + 1] = (float)sin(2 * PI * c / W);
    col_knot[c] = (int32_t)((long long)c * K / W);
  }
  cc_range_model_t model;
  memset(&model, 0, sizeof(model));
  model.n_rows = H;
  model.n_cols = W;
  model.word_type = CC_RANGE_U16;
  model.order = CC_RANGE_ROW_MAJOR;
  model.range_scale = 0.002f;
  model.origin_n = 0.03f;
  model.origin_z = 0.04f;
  model.n_knots = K;
  model.row_tab = row_tab.data();
  model.col_cos_sin = col_cs.data();
  model.col_knot = col_knot.data();
  cc_range_model_t plain_model = model;  // the same sensor without knots: the uncompensated image
  plain_model.n_knots = 0;
  plain_model.col_knot = nullptr;

  // the header's formula on the host
  std::shared_ptr<Cloud> moved = std::make_shared<Cloud>();
  const float on = model.origin_n, oz = model.origin_z, scale = model.range_scale;
  size_t none = 0;
  for (int r = 0; r < H; r++)
    for (int c = 0; c < W; c++) {
      const uint16_t w = words[(size_t)r * W + c];
      const float ca = row_tab[4 * r], sa = row_tab[4 * r + 1], co = row_tab[4 * r + 2], so = row_tab[4 * r + 3], ce = col_cs[2 * c], se = col_cs[2 * c + 1];
      const float rg = (float)w * scale;
      const float d = rg - on;
      const float h = d * ca;
      const float dx = (ce * co) - (se * so), dy = (se * co) + (ce * so);
      const float x = (h * dx) + (on * ce), y = (h * dy) + (on * se), z = (d * sa) + oz;
      const float *M = knots[(size_t)col_knot[c]].data();
      pcl::PointXYZ m;
      m.x = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
      m.y = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
      m.z = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
      m.pad_ = 0.f;
      if (w == 0) {
        m.x = std::numeric_limits<float>::quiet_NaN();
        none++;
      }
      moved->points.push_back(m);
    }
  if (none * 20 < words.size()) {
    printf("fewer than 5 %% of the pixels have no return: the check shows less than it should\n");
    return 1;
  }
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  cc_range_sensor *sensor = ContourManager::rangeSensor(config, model), *plain = ContourManager::rangeSensor(config, plain_model);
  ContourManager a(config, 0), b(config, 1), c(config, 2);
  ContourManager::RangeImage img, raw;
  img.sensor = sensor;
  img.words = words.data();
  img.knots = knots;
  raw.sensor = plain;
  raw.words = words.data();
  Cloud::ConstPtr cmoved = moved;
  a.makeBEV(img, "range image");
  b.makeBEV<pcl::PointXYZ>(cmoved, "host");
  c.makeBEV(raw, "uncompensated");
  a.makeContoursRecurs();
  b.makeContoursRecurs();
  c.makeContoursRecurs();
  const cc_scan_desc_t *da = nullptr, *db = nullptr, *dc = nullptr;
  if (cc_scan_desc(a.scanHandle(), &da) != CC_OK || cc_scan_desc(b.scanHandle(), &db) != CC_OK || cc_scan_desc(c.scanHandle(), &dc) != CC_OK) {
    fprintf(stderr, "%s\n", cc_last_error());
    return 4;
  }
  int rc = 0;
  if (const char *why = desc_diff(*da, *db)) {
    printf("differ: %s\n", why);
    rc = 1;
  } else if (!desc_diff(*da, *dc)) {
    printf("the knots changed nothing: the check shows nothing\n");
    rc = 1;
  } else {
    int nc = 0;
    for (int l = 0; l < CC_NLEV; l++) nc += da->n_cont[l];
    printf("ok %zu %d\n", words.size(), nc);
  }
  ContourManager::releaseRangeSensor(sensor);
  ContourManager::releaseRangeSensor(plain);
  return rc;
}
