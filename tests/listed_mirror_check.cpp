// TEST PROGRAM (tests/test_hostcpp_listed.py): the reference driver's loop on the class mirror; at scans 37 and 57 the query is
// asked before the scan is added: queryRangedKNN ("u"), ContourDB::queryAmong with every scan of the database ("a"), queryAmong
// with a restricted list ("m": at 37 every scan but queryRangedKNN's answer, at 57 the scans from 32 on), ContourDB::queryAllowed
// with the same list ("w"), and both again with four entries, detail rows and match rows ("r" among, "s" allowed).
// Every number is printed as a hex float.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cont2/contour_db.h"
#include "eval/evaluator.h"

SequentialTimeProfiler stp;

static void show(int seq, const char *kind, const std::vector<std::shared_ptr<const ContourManager>> &cands, const std::vector<double> &corr,
                 const std::vector<Eigen::Isometry2d> &tfs) {
  printf("m %d %s %d", seq, kind, (int)cands.size());
  for (size_t k = 0; k < cands.size(); k++)
    printf(" %d %a %a %a %a", cands[k]->getIntID(), corr[k], tfs[k](0, 2), tfs[k](1, 2), std::atan2(tfs[k](1, 0), tfs[k](0, 0)));
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  ContourManagerConfig cfg;
  cfg.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourDBConfig dcfg;
  dcfg.q_levels_ = {1, 2, 3};
  dcfg.tb_cfg_.max_elapse_ = 2.5;
  dcfg.tb_cfg_.min_elapse_ = 1.5;
  ContourDB db(dcfg);
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
  int seq = 0;
  while (ev.loadNewScan()) {
    const auto info = ev.getCurrScanInfo();
    auto cm = ev.getCurrContourManager(cfg);
    db.queryRangedKNN(cm, lb, ub, cands, corr, tfs);
    if (seq == 37 || seq == 57) {
      show(seq, "u", cands, corr, tfs);
      const int best = cands.empty() ? -1 : cands[0]->getIntID();
      std::vector<int> all, some;
      for (int g = 0; g < seq; g++) {
        all.push_back(g);
        if (seq == 37 ? g != best : g >= 32) some.push_back(g);
      }
      db.queryAmong(cm, all, lb, ub, cands, corr, tfs);
      show(seq, "a", cands, corr, tfs);
      db.queryAmong(cm, some, lb, ub, cands, corr, tfs);
      show(seq, "m", cands, corr, tfs);
      db.queryAllowed(cm, some, lb, ub, cands, corr, tfs);
      show(seq, "w", cands, corr, tfs);
      db.setMaxReturn(4);  // the ranked list with its detail and match rows: no entry names a scan outside the list
      db.setWantDetail(true);
      db.setWantMatches(2.0);
      db.queryAmong(cm, some, lb, ub, cands, corr, tfs);
      show(seq, "r", cands, corr, tfs);
      if (db.lastDetails().size() != cands.size() || db.lastMatches().size() != cands.size()) return 3;
      const auto det = db.lastDetails();
      const auto mat = db.lastMatches();
      db.queryAllowed(cm, some, lb, ub, cands, corr, tfs);
      show(seq, "s", cands, corr, tfs);
      if (db.lastDetails().size() != det.size() || db.lastMatches().size() != mat.size()) return 4;
      for (size_t k = 0; k < det.size(); k++)
        if (memcmp(&det[k], &db.lastDetails()[k], sizeof(det[k])) != 0 || memcmp(&mat[k], &db.lastMatches()[k], sizeof(mat[k])) != 0) return 5;
      db.setMaxReturn(1);
      db.setWantDetail(false);
      db.setWantMatches(-1.0);
    }
    db.addScan(cm, info.ts);
    db.pushAndBalance(seq++, info.ts);
  }
  printf("done %d\n", seq);
  return 0;
}
