// Test program (CPU harness or GPU): the class mirror's ranked answers (hostcpp/cont2/contour_db.h: ContourDB::setMaxReturn,
// the verifyCandidates overload, CandidateManager::fineOptimize's max_ret) in the reference driver's loop
// (test/batch_bin_test.cpp:131-237) over a scan list, with or without the database's read-ahead (CC_DB_READ_AHEAD).
// usage: ranked_mirror_check <poses.txt> <scans.txt> <max_ret>     (max_ret 0: setMaxReturn is never called -- the default)
// prints per query   "q <id> <n> { <cand id> <correlation> <x> <y> <theta> } x n"
// for scans 38..40   "v <id> <n> {...}"  verifyCandidates({0, 1, 2, 3}, max_ret)  and  "f <id> <n> {...}"  the same candidates
//                    through CandidateManager's demo loop + fineOptimize(max_fine_opt, ..., max_ret)
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "eval/evaluator.h"

SequentialTimeProfiler stp;

static void show(const char *label, int id, const std::vector<std::shared_ptr<const ContourManager>> &c, const std::vector<double> &corr,
                 const std::vector<Eigen::Isometry2d> &T) {
  printf("%s %d %d", label, id, (int)c.size());
  for (size_t k = 0; k < c.size(); k++)
    printf(" %d %.17g %.17g %.17g %.17g", c[k]->getIntID(), corr[k], T[k](0, 2), T[k](1, 2), std::atan2(T[k](1, 0), T[k](0, 0)));
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
  if (max_ret > 0) db.setMaxReturn(max_ret);
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
    show("q", cm->getIntID(), cands, corr, tfs);
    if (seq >= 38 && seq <= 40) {
      const std::vector<int> idx = {0, 1, 2, 3};
      const int mr = max_ret > 0 ? max_ret : 1;
      const int nv = max_ret > 0 ? db.verifyCandidates(cm, idx, lb, ub, cands, corr, tfs, mr) : db.verifyCandidates(cm, idx, lb, ub, cands, corr, tfs);
      if (nv != (int)cands.size()) return 3;
      show("v", cm->getIntID(), cands, corr, tfs);
      CandidateManager m(cm, lb, ub);
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
      const int nf = max_ret > 0 ? m.fineOptimize(dcfg.max_fine_opt_, cands, corr, tfs, mr) : m.fineOptimize(dcfg.max_fine_opt_, cands, corr, tfs);
      if (nf != (int)cands.size()) return 4;
      show("f", cm->getIntID(), cands, corr, tfs);
    }
    db.addScan(cm, info.ts);
    db.pushAndBalance(seq++, info.ts);
    added.push_back(cm);
  }
  printf("done %d\n", seq);
  return 0;
}
