// TEST PROGRAM (tests/test_hostcpp_pose.py): the reference driver's loop on the class mirror; for three scans the candidates
// queryRangedKNN hands out (setMaxReturn(5), setWantDetail(true)) are scored again through ContourDB::scorePoses from their
// detail rows' tf_init -- refined without a bar with two try poses each (T_init and the pose the query returned; the first
// query of a call carries none), and unrefined with the shipped bar.  Every number is printed as a hex float: the test replays
// the same items through the C-ABI and compares bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "cont2/contour_db.h"
#include "eval/evaluator.h"

SequentialTimeProfiler stp;

static void show(int seq, int mode, const std::vector<ContourDB::PoseQuery> &qs, const std::vector<double> &th_in, const std::vector<std::vector<double>> &th_try,
                 const std::vector<ContourDB::PoseScore> &rs) {
  for (size_t k = 0; k < qs.size(); k++) {
    const auto &q = qs[k];
    const auto &r = rs[k];
    printf("p %d %d %d %d %a %a %a %d", seq, mode, (int)k, q.cand, q.T_init(0, 2), q.T_init(1, 2), th_in[k], (int)q.T_try.size());
    for (size_t t = 0; t < q.T_try.size(); t++) printf(" %a %a %a", q.T_try[t](0, 2), q.T_try[t](1, 2), th_try[k][t]);
    printf(" %a %a %a %a %a %d %d %d %d", r.corr_init, r.correlation, r.T_best(0, 2), r.T_best(1, 2), std::atan2(r.T_best(1, 0), r.T_best(0, 0)),
           r.n_pairs, r.iterations, r.termination, r.flags);
    if (r.try_corr.size() != q.T_try.size()) exit(5);
    for (const double v : r.try_corr) printf(" %a", v);
    for (int j = 0; j < 6; j++) printf(" %a", r.hess[j]);
    for (int j = 0; j < 3; j++) printf(" %a", r.grad[j]);
    printf("\n");
  }
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
  db.setMaxReturn(5);
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
  int seq = 0, n_scored = 0;
  while (ev.loadNewScan()) {
    const auto info = ev.getCurrScanInfo();
    auto cm = ev.getCurrContourManager(cfg);
    db.queryRangedKNN(cm, lb, ub, cands, corr, tfs);
    if (seq >= 38 && seq <= 40 && !cands.empty()) {
      const std::vector<cc_ranked_detail_t> det = db.lastDetails();
      if (det.size() != cands.size()) return 3;
      std::vector<ContourDB::PoseQuery> qs(cands.size());
      std::vector<double> th_in(cands.size());
      std::vector<std::vector<double>> th_try(cands.size());
      for (size_t k = 0; k < cands.size(); k++) {
        qs[k].cand = cands[k]->getIntID();
        qs[k].T_init.rotate(det[k].tf_init[2]);
        qs[k].T_init.pretranslate(det[k].tf_init[0], det[k].tf_init[1]);
        th_in[k] = std::atan2(qs[k].T_init(1, 0), qs[k].T_init(0, 0));  // the angle scorePoses hands to the library
        if (k > 0) {
          qs[k].T_try = {qs[k].T_init, tfs[k]};
          th_try[k] = {th_in[k], std::atan2(tfs[k](1, 0), tfs[k](0, 0))};
        }
      }
      show(seq, 1, qs, th_in, th_try, db.scorePoses(cm, qs, true, -INFINITY));
      show(seq, 0, qs, th_in, th_try, db.scorePoses(cm, qs, false));
      n_scored += (int)qs.size();
    }
    db.addScan(cm, info.ts);
    db.pushAndBalance(seq++, info.ts);
  }
  printf("done %d %d\n", seq, n_scored);
  return 0;
}
