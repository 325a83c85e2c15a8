// Test program (CPU harness or GPU): the class mirror's makeBEV with a HeightImage (hostcpp/cont2/contour_mng.h).  A ContourManager made
// from a cloud, and a second one made from the first's getBevImage(), the pillar positions the reference keeps in bev_pixfs_ (computed
// here on the host from the cloud: pointToContRowCol of the first point at each cell's maximum, f32, build with -ffp-contract=off) and the
// first's minimum height, carry the same descriptor -- the reference's resumeImage idea carried through to a descriptor.  A third one,
// made from the image alone, has the same contour counts but other positions: the check shows something.
// usage: make_bev_image_check <file.bin of x y z i f32 records>    prints "ok <occupied cells> <contours>" or the first difference
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

typedef pcl::PointCloud<pcl::PointXYZ> Cloud;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::shared_ptr<Cloud> cloud = std::make_shared<Cloud>();
  float rec[4];
  while (fread(rec, sizeof(float), 4, f) == 4) {
    pcl::PointXYZ p;
    p.x = rec[0];
    p.y = rec[1];
    p.z = rec[2];
    p.pad_ = 0.f;
    cloud->points.push_back(p);
  }
  fclose(f);
  if (cloud->points.size() <= 10) return 3;

  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourManager::keepImages() = true;
  ContourManager a(config, 0), b(config, 1), c(config, 2);
  Cloud::ConstPtr ccloud = cloud;
  a.makeBEV<pcl::PointXYZ>(ccloud, "cloud");
  a.makeContoursRecurs();
  const cc_host::Image<float> img = a.getBevImage();
  const int n_row = config.n_row_, n_col = config.n_col_;

  // bev_pixfs_ (contour_mng.h:505-556): per occupied cell the continuous position of the first point that reaches the cell's maximum
  std::vector<float> pos((size_t)n_row * n_col * 2, -1.f);
  std::vector<char> have((size_t)n_row * n_col, 0);
  const float x_max = (float)(n_row / 2) * config.reso_row_, y_max = (float)(n_col / 2) * config.reso_col_, pad = 1e-2f;
  size_t occupied = 0, found = 0;
  for (size_t i = 0; i < img.data.size(); i++) occupied += img.data[i] > -1000.f ? 1 : 0;
  for (const pcl::PointXYZ &p : cloud->points) {
    if (!(p.x >= -x_max + pad && p.x <= x_max - pad && p.y >= -y_max + pad && p.y <= y_max - pad) || (p.y * p.y + p.x * p.x) < config.blind_sq_) continue;
    const int row = (int)floorf(p.x / config.reso_row_) + n_row / 2, col = (int)floorf(p.y / config.reso_col_) + n_col / 2;
    if (row <= 0 || row >= n_row || col < 0 || col >= n_col) continue;
    const size_t cell = (size_t)row * n_col + col;
    const float h = config.lidar_height_ + p.z;
    if (have[cell] || h != img.data[cell]) continue;
    have[cell] = 1;
    pos[2 * cell] = p.x / config.reso_row_ + (float)(n_row / 2) - 0.5f;
    pos[2 * cell + 1] = p.y / config.reso_col_ + (float)(n_col / 2) - 0.5f;
    found++;
  }
  if (found != occupied || occupied < 100) {
    printf("pillars found for %zu of %zu occupied cells\n", found, occupied);
    return 1;
  }
  const cc_scan_desc_t *da = nullptr, *db = nullptr, *dc = nullptr;
  if (cc_scan_desc(a.scanHandle(), &da) != CC_OK) {
    fprintf(stderr, "%s\n", cc_last_error());
    return 4;
  }
  ContourManager::HeightImage resumed, bare;
  resumed.height = img.data.data();
  resumed.pos_rc = pos.data();
  resumed.has_min = true;
  resumed.min_height = da->min_bin_val;
  bare.height = img.data.data();
  b.makeBEV(resumed, "resumed");
  c.makeBEV(bare, "image alone");
  b.makeContoursRecurs();
  c.makeContoursRecurs();
  if (cc_scan_desc(b.scanHandle(), &db) != CC_OK || cc_scan_desc(c.scanHandle(), &dc) != CC_OK) {
    fprintf(stderr, "%s\n", cc_last_error());
    return 4;
  }
  int rc = 0;
  const cc_host::Image<float> img_b = b.getBevImage();
  if (const char *why = desc_diff(*da, *db)) {
    printf("differ: %s\n", why);
    rc = 1;
  } else if (memcmp(img_b.data.data(), img.data.data(), sizeof(float) * img.data.size()) != 0) {
    printf("differ: the resumed manager's image\n");
    rc = 1;
  } else if (memcmp(da->n_cont, dc->n_cont, sizeof(da->n_cont)) != 0 || da->n_pix != dc->n_pix || da->max_bin_val != dc->max_bin_val) {
    printf("differ: the image alone gives other contour counts\n");
    rc = 1;
  } else if (!desc_diff(*da, *dc)) {
    printf("the positions changed nothing: the check shows nothing\n");
    rc = 1;
  } else {
    int nc = 0;
    for (int l = 0; l < CC_NLEV; l++) nc += da->n_cont[l];
    printf("ok %zu %d\n", occupied, nc);
  }
  return rc;
}
