// TEST PROGRAM (tests/test_emu_packed_query.py, tests/test_gpu_packed_query.py): the reference driver's loop on the class mirror,
// feeding two databases -- one with the shipped settings, one with setMaxReturn(4) and setWantDetail(true).  What queryRangedKNN
// answered for scan i during the drive is kept; after the drive ContourDB::queryStored(i, i) must hand out the same candidates,
// correlations and poses (and detail rows), bit for bit, from the records the database keeps.  For the first closed scans
// verifyStored / scorePosesStored are compared with verifyCandidates / scorePoses on the scan's ContourManager the same way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cont2/contour_db.h"
#include "eval/evaluator.h"

SequentialTimeProfiler stp;

struct Answer {
  std::vector<int> id;
  std::vector<double> corr;
  std::vector<Eigen::Isometry2d> tf;
  std::vector<cc_ranked_detail_t> det;
};

static Answer keep(const std::vector<std::shared_ptr<const ContourManager>> &c, const std::vector<double> &corr, const std::vector<Eigen::Isometry2d> &tf,
                   const std::vector<cc_ranked_detail_t> &det) {
  Answer a;
  for (const auto &p : c) a.id.push_back(p->getIntID());
  a.corr = corr;
  a.tf = tf;
  a.det = det;
  return a;
}
static bool same(const Eigen::Isometry2d &a, const Eigen::Isometry2d &b) {
  for (int r = 0; r < 2; r++)  // (the mirror's Isometry2d keeps the two upper rows)
    for (int c = 0; c < 3; c++) {
      const double x = a(r, c), y = b(r, c);
      if (memcmp(&x, &y, sizeof(double)) != 0) return false;
    }
  return true;
}
static bool same(const Answer &a, const Answer &b) {
  if (a.id != b.id || a.corr.size() != b.corr.size() || a.tf.size() != b.tf.size() || a.det.size() != b.det.size()) return false;
  for (size_t k = 0; k < a.corr.size(); k++)
    if (memcmp(&a.corr[k], &b.corr[k], sizeof(double)) != 0) return false;
  for (size_t k = 0; k < a.tf.size(); k++)
    if (!same(a.tf[k], b.tf[k])) return false;
  for (size_t k = 0; k < a.det.size(); k++)
    if (memcmp(&a.det[k], &b.det[k], sizeof(cc_ranked_detail_t)) != 0) return false;
  return true;
}
static bool same(const std::vector<ContourDB::PoseScore> &a, const std::vector<ContourDB::PoseScore> &b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); k++) {
    const auto &x = a[k], &y = b[k];
    if (memcmp(&x.corr_init, &y.corr_init, 8) || memcmp(&x.correlation, &y.correlation, 8) || !same(x.T_best, y.T_best) ||
        x.n_pairs != y.n_pairs || x.iterations != y.iterations || x.termination != y.termination || x.flags != y.flags || x.try_corr != y.try_corr ||
        memcmp(x.hess, y.hess, sizeof(x.hess)) || memcmp(x.grad, y.grad, sizeof(x.grad)))
      return false;
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  ContourManagerConfig cfg;
  cfg.lv_grads_ = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  ContourDBConfig dcfg;
  dcfg.q_levels_ = {1, 2, 3};
  dcfg.tb_cfg_.max_elapse_ = 2.5;
  dcfg.tb_cfg_.min_elapse_ = 1.5;
  ContourDB db(dcfg), dbr(dcfg);
  dbr.setMaxReturn(4);
  dbr.setWantDetail(true);
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
  std::vector<std::shared_ptr<const ContourManager>> scans;
  std::vector<Answer> plain, ranked;
  int seq = 0;
  while (ev.loadNewScan()) {
    const auto info = ev.getCurrScanInfo();
    auto cm = ev.getCurrContourManager(cfg);
    db.queryRangedKNN(cm, lb, ub, cands, corr, tfs);
    plain.push_back(keep(cands, corr, tfs, {}));
    dbr.queryRangedKNN(cm, lb, ub, cands, corr, tfs);
    ranked.push_back(keep(cands, corr, tfs, dbr.lastDetails()));
    scans.push_back(cm);
    db.addScan(cm, info.ts);
    db.pushAndBalance(seq, info.ts);
    dbr.addScan(cm, info.ts);
    dbr.pushAndBalance(seq++, info.ts);
  }
  int closed = 0, lists = 0, bad_q = 0, bad_r = 0, bad_v = 0, bad_p = 0, n_v = 0, n_p = 0;
  for (int i = 0; i < seq; i++) {
    db.queryStored(i, i, lb, ub, cands, corr, tfs);
    bad_q += !same(plain[i], keep(cands, corr, tfs, {}));
    closed += !plain[i].id.empty();
    dbr.queryStored(i, i, lb, ub, cands, corr, tfs);
    bad_r += !same(ranked[i], keep(cands, corr, tfs, dbr.lastDetails()));
    lists += ranked[i].id.size() >= 2;
  }
  for (int i = 0; i < seq && n_v < 4; i++) {
    if (plain[i].id.empty()) continue;
    const int c = plain[i].id[0];
    std::vector<int> cl = {i, c};   // the scan itself is among its candidates
    if (c + 1 < seq && c + 1 != i) cl.push_back(c + 1);
    for (ContourDB *d : {&db, &dbr}) {
      const int mr = d == &db ? 1 : 3;
      const int n1 = d->verifyCandidates(scans[i], cl, lb, ub, cands, corr, tfs, mr);
      const Answer a = keep(cands, corr, tfs, d->lastDetails());
      const int n2 = d->verifyStored(i, cl, lb, ub, cands, corr, tfs, mr);
      bad_v += n1 != n2 || !same(a, keep(cands, corr, tfs, d->lastDetails()));
    }
    n_v++;
    std::vector<ContourDB::PoseQuery> qs(2);
    qs[0].cand = c;
    qs[0].T_init = plain[i].tf[0];
    qs[0].T_try = {plain[i].tf[0]};
    qs[1].cand = i;   // the scan against itself at the identity
    const auto p1 = db.scorePoses(scans[i], qs, true, -INFINITY);
    bad_p += !same(p1, db.scorePosesStored(i, qs, true, -INFINITY));
    n_p += p1[0].n_pairs > 0 && p1[1].n_pairs > 0;
  }
  printf("done %d closed %d lists %d verified %d posed %d bad %d %d %d %d\n", seq, closed, lists, n_v, n_p, bad_q, bad_r, bad_v, bad_p);
  return 0;
}
