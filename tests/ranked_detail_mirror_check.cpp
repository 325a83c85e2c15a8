// TEST PROGRAM (tests/test_hostcpp_ranked_detail.py): the reference driver's loop on the class mirror with
// ContourDB::setWantDetail(true) and setMaxReturn(argv[3]) -- per scan the candidates queryRangedKNN hands out and the bytes of
// lastDetails(); for three scans also verifyCandidates' and CandidateManager::fineOptimize's over the same four candidates.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "cont2/contour_db.h"
#include "eval/evaluator.h"

SequentialTimeProfiler stp;

static void show(const char *label, int id, const std::vector<std::shared_ptr<const ContourManager>> &c, const std::vector<cc_ranked_detail_t> &d) {
  printf("%s %d %d %d", label, id, (int)c.size(), (int)d.size());
  for (size_t k = 0; k < c.size(); k++) printf(" %d", c[k]->getIntID());
  for (size_t k = 0; k < d.size(); k++) {
    printf(" ");
    const unsigned char *b = (const unsigned char *)&d[k];
    for (size_t i = 0; i < sizeof(cc_ranked_detail_t); i++) printf("%02x", b[i]);
  }
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const int max_ret = atoi(argv[3]);
  ContourManagerConfig cfg;
  cfg.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourDBConfig dcfg;
  dcfg.q_levels_ = {1, 2, 3};
  dcfg.tb_cfg_.max_elapse_ = 2.5;
  dcfg.tb_cfg_.min_elapse_ = 1.5;
  ContourDB db(dcfg);
  db.setMaxReturn(max_ret);
  db.setWantDetail(true);
  ContLCDEvaluator ev(argv[1], argv[2], 0.5);
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
  std::vector<std::shared_ptr<const ContourManager>> cands;
  std::vector<double> corr;
  std::vector<Eigen::Isometry2d> tfs;
  std::vector<std::shared_ptr<ContourManager>> added;
  int seq = 0;
  while (ev.loadNewScan()) {
    const auto info = ev.getCurrScanInfo();
    auto cm = ev.getCurrContourManager(cfg);
    db.queryRangedKNN(cm, lb, ub, cands, corr, tfs);
    show("q", cm->getIntID(), cands, db.lastDetails());
    if (seq >= 38 && seq <= 40) {
      const std::vector<int> idx = {0, 1, 2, 3};
      const int nv = db.verifyCandidates(cm, idx, lb, ub, cands, corr, tfs, max_ret);
      if (nv != (int)cands.size()) return 3;
      show("v", cm->getIntID(), cands, db.lastDetails());
      CandidateManager m(cm, lb, ub);
      m.setWantDetail(true);
      for (const int c : idx)
        for (int ll = 1; ll <= CC_BCI_LAYERS; ll++) {
          const auto keys1 = added[c]->getLevRetrievalKey(ll), keys2 = cm->getLevRetrievalKey(ll);
          for (int i1 = 0; i1 < (int)keys1.size(); i1++)
            for (int i2 = 0; i2 < (int)keys2.size(); i2++) {
              if (keys1[i1].sum() == 0 || keys2[i2].sum() == 0) continue;
              KeyFloatType d2 = 0;
              for (int k = 0; k < RET_KEY_DIM; k++) d2 += (keys1[i1][k] - keys2[i2][k]) * (keys1[i1][k] - keys2[i2][k]);
              if (d2 > 1000.0f) continue;
              m.checkCandWithHint(added[c], ConstellationPair(ll, i1, i2), dcfg.cont_sim_cfg_);
            }
        }
      m.tidyUpCandidates();
      const int nf = m.fineOptimize(dcfg.max_fine_opt_, cands, corr, tfs, max_ret);
      if (nf != (int)cands.size()) return 4;
      show("f", cm->getIntID(), cands, m.lastDetails());
    }
    db.addScan(cm, info.ts);
    db.pushAndBalance(seq++, info.ts);
    added.push_back(cm);
  }
  printf("done %d\n", seq);
  return 0;
}
