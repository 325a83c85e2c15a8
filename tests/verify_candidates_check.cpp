// Test program (CPU harness or GPU): the class mirror's ContourDB::verifyCandidates (hostcpp/cont2/contour_db.h, mirror-only: one
// device pass whose hint list is generated on the device) must return what the mirror's own CandidateManager returns for the demo
// loop over the same candidates (hostcpp/examples/pair_demo.cpp with the candidate as the outermost index) + tidyUpCandidates +
// fineOptimize -- the same candidate, the same correlation and pose, bit for bit.
// usage: verify_candidates_check <cand_0.bin> ... <cand_k.bin> <query.bin>    (k + 1 <= CC_VERIFY_CANDS_MAX candidate scans)
// prints "ok <n_res> <index of the candidate> <correlation> <hints>" or the first difference
#include <cmath>
#include <cstring>

#include "cont2/contour_db.h"

SequentialTimeProfiler stp;

static std::shared_ptr<ContourManager> load(const ContourManagerConfig &cfg, const char *path, int id) {
  auto cloud = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(3);
  }
  float rec[4];
  while (fread(rec, sizeof(float), 4, f) == 4) cloud->push_back(pcl::PointXYZ{rec[0], rec[1], rec[2], 0.f});
  fclose(f);
  std::shared_ptr<ContourManager> cm(new ContourManager(cfg, id));
  pcl::PointCloud<pcl::PointXYZ>::ConstPtr cc = cloud;
  cm->makeBEV<pcl::PointXYZ>(cc, std::to_string(id));
  cm->makeContoursRecurs();
  cm->clearImage();
  return cm;
}

int main(int argc, char **argv) {
  if (argc < 3 || argc - 2 > CC_VERIFY_CANDS_MAX) return 2;
  ContourManagerConfig config;
  config.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  const int n_cand = argc - 2;
  std::vector<std::shared_ptr<ContourManager>> scans;
  for (int i = 0; i < n_cand; i++) scans.push_back(load(config, argv[1 + i], i));
  auto cm_new = load(config, argv[argc - 1], n_cand);

  CandidateScoreEnsemble lb, ub;  // the shipped thresholds
  lb.sim_constell.i_ovlp_sum = lb.sim_constell.i_ovlp_max_one = lb.sim_constell.i_in_ang_rng = 3;
  lb.sim_pair.i_indiv_sim = 3;
  lb.sim_pair.i_orie_sim = 4;
  lb.sim_post.correlation = 0.3f;
  lb.sim_post.area_perc = 0.03f;
  lb.sim_post.neg_est_dist = -5.01f;
  ub.sim_constell.i_ovlp_sum = ub.sim_constell.i_ovlp_max_one = ub.sim_constell.i_in_ang_rng = 6;
  ub.sim_pair.i_indiv_sim = ub.sim_pair.i_orie_sim = 6;
  ub.sim_post.correlation = 0.75f;
  ub.sim_post.area_perc = 0.15f;
  ub.sim_post.neg_est_dist = -5.0f;

  ContourDBConfig db_config;
  db_config.q_levels_ = {1, 2, 3};
  db_config.max_fine_opt_ = 5;
  ContourDB db(db_config, 64);
  for (int i = 0; i < n_cand; i++) {
    db.addScan(scans[i], (double)i);
    db.pushAndBalance(i, (double)i);
  }
  // candidates in an order of the caller's own: last added first
  std::vector<int> idx;
  for (int i = n_cand - 1; i >= 0; i--) idx.push_back(i);

  std::vector<std::shared_ptr<const ContourManager>> v_cand, m_cand;
  std::vector<double> v_corr, m_corr;
  std::vector<Eigen::Isometry2d> v_T, m_T;
  const int nv = db.verifyCandidates(cm_new, idx, lb, ub, v_cand, v_corr, v_T);

  CandidateManager cand_mng(cm_new, lb, ub);
  int n_hints = 0;
  for (const int c : idx)
    for (int ll = 1; ll <= CC_BCI_LAYERS; ll++) {
      const auto keys1 = scans[c]->getLevRetrievalKey(ll), keys2 = cm_new->getLevRetrievalKey(ll);
      for (int i1 = 0; i1 < (int)keys1.size(); i1++)
        for (int i2 = 0; i2 < (int)keys2.size(); i2++) {
          if (keys1[i1].sum() == 0 || keys2[i2].sum() == 0) continue;
          KeyFloatType d2 = 0;
          for (int k = 0; k < RET_KEY_DIM; k++) d2 += (keys1[i1][k] - keys2[i2][k]) * (keys1[i1][k] - keys2[i2][k]);
          if (d2 > 1000.0f) continue;
          cand_mng.checkCandWithHint(scans[c], ConstellationPair(ll, i1, i2), db_config.cont_sim_cfg_);
          n_hints++;
        }
    }
  cand_mng.tidyUpCandidates();
  const int nm = cand_mng.fineOptimize(db_config.max_fine_opt_, m_cand, m_corr, m_T);

  if (nv != nm || v_cand.size() != m_cand.size() || v_corr.size() != m_corr.size() || v_T.size() != m_T.size()) {
    printf("differ: %d results against %d\n", nv, nm);
    return 1;
  }
  int which = -1;
  if (nv > 0) {
    if (v_cand[0].get() != m_cand[0].get()) {
      printf("differ: another candidate\n");
      return 1;
    }
    bool same_T = true;
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 3; j++) {
        const double a = v_T[0](i, j), b = m_T[0](i, j);
        same_T = same_T && memcmp(&a, &b, sizeof(double)) == 0;
      }
    if (memcmp(&v_corr[0], &m_corr[0], sizeof(double)) != 0 || !same_T) {
      printf("differ: correlation %.17g against %.17g, or the pose\n", v_corr[0], m_corr[0]);
      return 1;
    }
    for (int i = 0; i < n_cand; i++)
      if (scans[i].get() == v_cand[0].get()) which = i;
  }
  // an empty candidate list gives no result
  std::vector<int> none;
  if (db.verifyCandidates(cm_new, none, lb, ub, v_cand, v_corr, v_T) != 0 || !v_cand.empty()) {
    printf("differ: a result without candidates\n");
    return 1;
  }
  printf("ok %d %d %.9g %d\n", nv, which, nv > 0 ? m_corr[0] : 0.0, n_hints);
  return 0;
}
