// Test program (CPU harness or GPU): the class mirror's makeBEV with a BevCoords (hostcpp/cont2/contour_mng.h) gives the descriptor of its
// plain makeBEV on the cloud converted on the host by the header's three steps -- p = (float)((double)v [* scale] - origin), each rounded
// once (this file is compiled with -ffp-contract=off).  The file holds georeferenced f64 x y z; they are ingested
//   - as one f64 record array and as three f64 column arrays, each of EXACTLY the spanned size and in front of an inaccessible page, so
//     that a host form reading one element too many faults here,
//   - as f64 records of 32 bytes with x, y, z at 0, 16, 8,
//   - as scaled i32 records (the LAS convention) with an origin that folds the file offset,
//   - with and without T_bev_sensor,
// and the cloud cast to f32 BEFORE the subtraction must give another descriptor, or the check shows nothing.
// usage: make_bev_coords_check <file.bin> <origin x> <origin y> <origin z>    prints "ok <points> <contours>" or the first difference
#include <sys/mman.h>
#include <unistd.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

// `bytes` of memory that end where an inaccessible page begins
static char *guarded(size_t bytes) {
  const size_t page = (size_t)sysconf(_SC_PAGESIZE), total = (bytes + page - 1) / page * page + page;
  char *m = (char *)mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (m == MAP_FAILED || mprotect(m + total - page, page, PROT_NONE) != 0) {
    perror("guarded");
    exit(4);
  }
  return m + total - page - bytes;
}

typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
static const float T[12] = {0.96592583f, -0.25881905f, 0.f, 2.5f, 0.25881905f, 0.96592583f, 0.f, -1.25f, 0.f, 0.f, 1.f, 0.125f};  // 15 degrees of yaw and a shift

// 0: the mirror's descriptor of `crd` equals the plain makeBEV's of `ref`; 1: a difference (printed)
static int compare(const ContourManagerConfig &config, const ContourManager::BevCoords &crd, Cloud::ConstPtr ref, bool with_tf, const char *tag, int *n_cont) {
  ContourManager a(config, 0), b(config, 1);
  if (with_tf) {
    a.makeBEV(crd, &T, "coords");
    b.makeBEV<pcl::PointXYZ>(ref, T, "converted");
  } else {
    a.makeBEV(crd, nullptr, "coords");
    b.makeBEV<pcl::PointXYZ>(ref, "converted");
  }
  a.makeContoursRecurs();
  b.makeContoursRecurs();
  const cc_scan_desc_t *da = nullptr, *db = nullptr;
  if (cc_scan_desc(a.scanHandle(), &da) != CC_OK || cc_scan_desc(b.scanHandle(), &db) != CC_OK) {
    fprintf(stderr, "%s\n", cc_last_error());
    return 1;
  }
  if (const char *why = desc_diff(*da, *db)) {
    printf("%s: differ: %s\n", tag, why);
    return 1;
  }
  *n_cont = 0;
  for (int l = 0; l < CC_NLEV; l++) *n_cont += da->n_cont[l];
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const double O[3] = {atof(argv[2]), atof(argv[3]), atof(argv[4])};
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> W;
  double rec[3];
  while (fread(rec, sizeof(double), 3, f) == 3) W.insert(W.end(), rec, rec + 3);
  fclose(f);
  const size_t n = W.size() / 3;
  std::shared_ptr<Cloud> conv = std::make_shared<Cloud>(), naive = std::make_shared<Cloud>(), las = std::make_shared<Cloud>();
  // the LAS form: X = v * 0.001 + file offset; the call's origin folds the file offset in
  const double scale[3] = {0.001, 0.001, 0.001}, file_off[3] = {448000.0, 5412000.0, 0.0}, las_origin[3] = {O[0] - file_off[0], O[1] - file_off[1], O[2] - file_off[2]};
  std::vector<int32_t> V(3 * n);
  for (size_t i = 0; i < n; i++) {
    pcl::PointXYZ p, q, r;
    float *pc[3] = {&p.x, &p.y, &p.z}, *qc[3] = {&q.x, &q.y, &q.z}, *rc[3] = {&r.x, &r.y, &r.z};
    for (int k = 0; k < 3; k++) {
      const double X = W[3 * i + k];
      const double D = X - O[k];
      *pc[k] = (float)D;
      *qc[k] = (float)X - (float)O[k];
      V[3 * i + k] = (int32_t)llround((X - file_off[k]) / scale[k]);
      const double P = (double)V[3 * i + k] * scale[k];
      const double E = P - las_origin[k];
      *rc[k] = (float)E;
    }
    conv->points.push_back(p);
    naive->points.push_back(q);
    las->points.push_back(r);
  }
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  Cloud::ConstPtr cconv = conv, cnaive = naive, clas = las;
  int nc = 0, nc2 = 0;

  // one record array of exactly (n - 1) * 24 + 24 bytes
  char *one = guarded(n * 24);
  memcpy(one, W.data(), n * 24);
  ContourManager::BevCoords rec24;
  rec24.x = one;
  rec24.y = one + 8;
  rec24.z = one + 16;
  rec24.type = CC_COORD_F64;
  rec24.stride_bytes = 24;
  rec24.origin = O;
  rec24.n = (int64_t)n;
  if (compare(config, rec24, cconv, false, "f64 records", &nc) || compare(config, rec24, cconv, true, "f64 records with T_bev_sensor", &nc2)) return 1;

  // the check must be able to fail: the cloud narrowed BEFORE the subtraction is another scan
  {
    ContourManager a(config, 0), b(config, 1);
    a.makeBEV<pcl::PointXYZ>(cconv, "converted");
    b.makeBEV<pcl::PointXYZ>(cnaive, "naive");
    a.makeContoursRecurs();
    b.makeContoursRecurs();
    const cc_scan_desc_t *da = nullptr, *db = nullptr;
    if (cc_scan_desc(a.scanHandle(), &da) != CC_OK || cc_scan_desc(b.scanHandle(), &db) != CC_OK) return 1;
    if (!desc_diff(*da, *db)) {
      printf("the naive cast changed nothing: the check shows nothing\n");
      return 1;
    }
  }

  // three column arrays of exactly (n - 1) * 8 + 8 bytes each
  double *col[3];
  for (int k = 0; k < 3; k++) {
    col[k] = (double *)guarded(n * 8);
    for (size_t i = 0; i < n; i++) col[k][i] = W[3 * i + k];
  }
  ContourManager::BevCoords cols = rec24;
  cols.x = col[0];
  cols.y = col[1];
  cols.z = col[2];
  cols.stride_bytes = 8;
  if (compare(config, cols, cconv, false, "f64 columns", &nc2)) return 1;

  // records of 32 bytes with x, y, z at 0, 16, 8: the spanned bytes are (n - 1) * 32 + 24
  char *r32 = guarded((n - 1) * 32 + 24);
  memset(r32, 0xFF, (n - 1) * 32 + 24);
  for (size_t i = 0; i < n; i++) {
    memcpy(r32 + i * 32, &W[3 * i], 8);
    memcpy(r32 + i * 32 + 16, &W[3 * i + 1], 8);
    memcpy(r32 + i * 32 + 8, &W[3 * i + 2], 8);
  }
  ContourManager::BevCoords rec32 = rec24;
  rec32.x = r32;
  rec32.y = r32 + 16;
  rec32.z = r32 + 8;
  rec32.stride_bytes = 32;
  if (compare(config, rec32, cconv, false, "f64 records of 32 bytes", &nc2)) return 1;

  // scaled i32 records of 12 bytes
  char *li = guarded(n * 12);
  memcpy(li, V.data(), n * 12);
  ContourManager::BevCoords lasc;
  lasc.x = li;
  lasc.y = li + 4;
  lasc.z = li + 8;
  lasc.type = CC_COORD_I32;
  lasc.stride_bytes = 12;
  for (int k = 0; k < 3; k++) lasc.scale[k] = scale[k];
  lasc.origin = las_origin;
  lasc.n = (int64_t)n;
  if (compare(config, lasc, clas, false, "scaled i32 records", &nc2) || compare(config, lasc, clas, true, "scaled i32 records with T_bev_sensor", &nc2)) return 1;

  printf("ok %zu %d\n", n, nc);
  return 0;
}
