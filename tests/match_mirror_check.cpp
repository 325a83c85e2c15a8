// TEST PROGRAM (tests/test_hostcpp_matches.py): the reference driver's loop on the class mirror with
// ContourDB::setWantMatches(argv[4]) and setMaxReturn(argv[3]) -- per scan the candidates queryRangedKNN hands out and the bytes of
// lastMatches(); for three scans also verifyCandidates' over four candidates, and once the pair list cc_match_pairs expands.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "cont2/contour_db.h"
#include "eval/evaluator.h"

SequentialTimeProfiler stp;

static void show(const char *label, int id, const std::vector<std::shared_ptr<const ContourManager>> &c, const std::vector<cc_ranked_match_t> &d) {
  printf("%s %d %d %d", label, id, (int)c.size(), (int)d.size());
  for (size_t k = 0; k < c.size(); k++) printf(" %d", c[k]->getIntID());
  for (size_t k = 0; k < d.size(); k++) {
    printf(" ");
    const unsigned char *b = (const unsigned char *)&d[k];
    for (size_t i = 0; i < sizeof(cc_ranked_match_t); i++) printf("%02x", b[i]);
  }
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const int max_ret = atoi(argv[3]);
  ContourManagerConfig cfg;
  cfg.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourDBConfig dcfg;
  dcfg.q_levels_ = {1, 2, 3};
  dcfg.tb_cfg_.max_elapse_ = 2.5;
  dcfg.tb_cfg_.min_elapse_ = 1.5;
  ContourDB db(dcfg);
  db.setMaxReturn(max_ret);
  db.setWantMatches(atof(argv[4]));
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
  bool listed = false;
  while (ev.loadNewScan()) {
    const auto info = ev.getCurrScanInfo();
    auto cm = ev.getCurrContourManager(cfg);
    db.queryRangedKNN(cm, lb, ub, cands, corr, tfs);
    show("q", cm->getIntID(), cands, db.lastMatches());
    if (!listed && !db.lastMatches().empty()) {  // the winning candidate's pair list, once
      cc_match_pair_t pr[400];
      const int np = cc_match_pairs(&db.lastMatches()[0], pr, 400);
      printf("p %d %d", cm->getIntID(), np);
      for (int i = 0; i < np; i++) printf(" %d:%d:%d", pr[i].level, pr[i].seq_src, pr[i].seq_tgt);
      printf("\n");
      listed = true;
    }
    if (seq >= 38 && seq <= 40) {
      const std::vector<int> idx = {0, 1, 2, 3};
      const int nv = db.verifyCandidates(cm, idx, lb, ub, cands, corr, tfs, max_ret);
      if (nv != (int)cands.size()) return 3;
      show("v", cm->getIntID(), cands, db.lastMatches());
    }
    if (seq == 40) {  // switched off: nothing is collected, the answer is the one queryRangedKNN gave before
      db.setWantMatches(-1.0);
      db.queryRangedKNN(cm, lb, ub, cands, corr, tfs);
      if (!db.lastMatches().empty()) return 5;
      show("o", cm->getIntID(), cands, db.lastMatches());
      db.setWantMatches(atof(argv[4]));
    }
    db.addScan(cm, info.ts);
    db.pushAndBalance(seq++, info.ts);
  }
  printf("done %d\n", seq);
  return 0;
}
