// TEST INFRASTRUCTURE: the CPU oracle of the reference's DYNAMIC_THRES=1 build (CMakeLists.txt:19-20), on top of the
// oracle restatement (oracle/cont2_oracle.cpp, included unchanged).  Built by the tests with the oracle's flags:
//   g++ -O3 -std=c++17 -fPIC -ffp-contract=off -shared -I<repo>/oracle -I<repo>/include dyn_thres_oracle.cpp
// The check stage calls the oracle's own CandidateManager::checkCandWithHint and raises sim_var_ after every call that
// passed (contour_db.h:439-457); the gates read sim_var_, so the partial scores under a raised bar come for free.
// tidyUpCandidates (with its post-bar block, contour_db.h:566-574) and the queryRangedKNN loop around both are restated
// from oracle/orc_db.h.  dyn = 0 gives the static oracle's answers.
#include "../oracle/cont2_oracle.cpp"

namespace {

template <typename T>
void dyn_bar(T &var, T v, T ub) {  // alignLB, then alignUB (tools/algos.h:125-148)
  var = var < v ? v : var;
  var = var > ub ? ub : var;
}

struct DynCandidateManager : CandidateManager {
  bool dyn;
  DynCandidateManager(std::shared_ptr<const ContourManager> cm_q, const CandidateScoreEnsemble &lb, const CandidateScoreEnsemble &ub, bool dyn_)
      : CandidateManager(std::move(cm_q), lb, ub), dyn(dyn_) {}

  // contour_db.h:374-488 with DYNAMIC_THRES = 1
  CandidateScoreEnsemble check(const std::shared_ptr<const ContourManager> &cm_cand, const ConstellationPair &anchor_pair,
                               const ContourSimThresConfig &cont_sim) {
    const int before = cand_aft_check3;
    CandidateScoreEnsemble s = checkCandWithHint(cm_cand, anchor_pair, cont_sim);
    if (dyn && cand_aft_check3 > before) {  // contour_db.h:439-457: cnt_curr_valid = ret_pairwise_sim.cnt() = i_orie_sim
      const int cnt = s.sim_pair.i_orie_sim;
      dyn_bar(sim_var_.sim_constell.i_ovlp_sum, cnt, sim_ub_.sim_constell.i_ovlp_sum);
      dyn_bar(sim_var_.sim_constell.i_ovlp_max_one, cnt, sim_ub_.sim_constell.i_ovlp_max_one);
      dyn_bar(sim_var_.sim_constell.i_in_ang_rng, cnt, sim_ub_.sim_constell.i_in_ang_rng);
      dyn_bar(sim_var_.sim_pair.i_indiv_sim, cnt, sim_ub_.sim_pair.i_indiv_sim);
      dyn_bar(sim_var_.sim_pair.i_orie_sim, cnt, sim_ub_.sim_pair.i_orie_sim);
    }
    return s;
  }

  // orc_db.h tidyUpCandidates + the post-bar block of contour_db.h:566-574
  void tidy() {
    GMMOptConfig gmm_config;
    n_cand_pose = (int)candidates_.size();
    for (auto &candidate : candidates_) {
      int idx_sel = 0;
      for (size_t i = 0; i < candidate.anch_props_.size(); i++) {
        std::vector<float> lev_perc(cm_tgt_->getConfig().lv_grads_.size(), 0);
        for (const auto &pr : candidate.anch_props_[i].constell_) lev_perc[pr.first.level] += pr.second;
        float perc = 0;
        for (int j = 0; j < NUM_BIN_KEY_LAYER; j++) perc += LAYER_AREA_WEIGHTS[j] * lev_perc[DIST_BIN_LAYERS[j]];
        candidate.anch_props_[i].area_perc_ = perc;
        if (candidate.anch_props_[i].vote_cnt_ > candidate.anch_props_[idx_sel].vote_cnt_) idx_sel = i;
      }
      std::swap(candidate.anch_props_[0], candidate.anch_props_[idx_sel]);
      if (candidate.anch_props_[0].area_perc_ < sim_var_.sim_post.area_perc) continue;
      double neg_est_trans_norm2d =
          -ConstellCorrelation::getEstSensTF(candidate.anch_props_[0].T_delta_, cm_tgt_->getConfig()).translation().norm();
      if (neg_est_trans_norm2d < sim_var_.sim_post.neg_est_dist) continue;
      std::unique_ptr<ConstellCorrelation> corr_est(new ConstellCorrelation(gmm_config));
      auto corr_score_init = (float)corr_est->initProblem(*(candidate.cm_cand_), *cm_tgt_, candidate.anch_props_[0].T_delta_);
      if (corr_score_init < sim_var_.sim_post.correlation) continue;
      if (dyn) {
        dyn_bar(sim_var_.sim_post.correlation, corr_score_init, sim_ub_.sim_post.correlation);
        dyn_bar(sim_var_.sim_post.area_perc, candidate.anch_props_[0].area_perc_, sim_ub_.sim_post.area_perc);
        dyn_bar(sim_var_.sim_post.neg_est_dist, (float)neg_est_trans_norm2d, sim_ub_.sim_post.neg_est_dist);
      }
      candidate.corr_est_ = std::move(corr_est);
    }
    int p1 = 0, p2 = candidates_.size() - 1;
    while (p1 <= p2) {
      if (!candidates_[p1].corr_est_ && candidates_[p2].corr_est_) {
        std::swap(candidates_[p1], candidates_[p2]);
        p1++;
        p2--;
      } else {
        if (candidates_[p1].corr_est_) p1++;
        if (!candidates_[p2].corr_est_) p2--;
      }
    }
    candidates_.erase(candidates_.begin() + p2 + 1, candidates_.end());
  }
};

void fill_result(const DynCandidateManager &mng, int n_res, int cand_idx, const std::vector<double> &corr, const std::vector<Iso2d> &tfs,
                 cc_query_result_t *res) {
  res->cand_aft_check1 = mng.cand_aft_check1;
  res->cand_aft_check2 = mng.cand_aft_check2;
  res->cand_aft_check3 = mng.cand_aft_check3;
  res->n_cand_pose = mng.n_cand_pose;
  res->n_cand_tidy = (int)mng.candidates_.size();
  res->n_res = n_res;
  res->cand_gidx = n_res ? cand_idx : -1;
  if (n_res) {
    res->correlation = corr[0];
    res->tf[0] = tfs[0](0, 2);
    res->tf[1] = tfs[0](1, 2);
    res->tf[2] = std::atan2(tfs[0](1, 0), tfs[0](0, 0));
  }
}

}  // namespace

extern "C" {

// orc_db_query with the queryRangedKNN loop of orc_db.h restated around DynCandidateManager (no kNN / timer outputs)
void orcdyn_db_query(void *d, void *scan, const cc_score_t *lb, const cc_score_t *ub, int dyn, cc_query_result_t *res) {
  const ContourDB &db = *((DbH *)d)->db;
  const std::shared_ptr<const ContourManager> q_ptr = ((ScanH *)scan)->cm;
  DynCandidateManager cand_mng(q_ptr, toScore(lb), toScore(ub), dyn != 0);
  int n_hits = 0;
  for (size_t ll = 0; ll < db.cfg_.q_levels_.size(); ll++) {
    const std::vector<BCI> &q_bcis = q_ptr->getLevBCI(db.cfg_.q_levels_[ll]);
    std::vector<RetrievalKey> q_keys = q_ptr->getLevRetrievalKey(db.cfg_.q_levels_[ll]);
    for (size_t seq = 0; seq < q_bcis.size(); seq++) {
      if (q_keys[seq].sum() == 0) continue;
      std::vector<std::pair<IndexOfKey, KeyFloatType>> tmp_res;
      KeyFloatType key_bounds[3][2];
      key_bounds[0][0] = q_keys[seq][0] * 0.8;
      key_bounds[0][1] = q_keys[seq][0] / 0.8;
      key_bounds[1][0] = q_keys[seq][1] * 0.8;
      key_bounds[1][1] = q_keys[seq][1] / 0.8;
      key_bounds[2][0] = q_keys[seq][2] * 0.8 * 0.75;
      key_bounds[2][1] = q_keys[seq][2] / (0.8 * 0.75);
      KeyFloatType dist_ub = 1e6;
      dist_ub = std::max((q_keys[seq][0] - key_bounds[0][0]) * (q_keys[seq][0] - key_bounds[0][0]),
                         (q_keys[seq][0] - key_bounds[0][1]) * (q_keys[seq][0] - key_bounds[0][1])) +
                std::max((q_keys[seq][1] - key_bounds[1][0]) * (q_keys[seq][1] - key_bounds[1][0]),
                         (q_keys[seq][1] - key_bounds[1][1]) * (q_keys[seq][1] - key_bounds[1][1])) +
                std::max((q_keys[seq][2] - key_bounds[2][0]) * (q_keys[seq][2] - key_bounds[2][0]),
                         (q_keys[seq][2] - key_bounds[2][1]) * (q_keys[seq][2] - key_bounds[2][1]));
      db.layer_db_[ll].layerKNNSearch(q_keys[seq], db.cfg_.nnk_, dist_ub, tmp_res);
      n_hits += (int)tmp_res.size();
      for (const auto &sear_res : tmp_res)
        cand_mng.check(db.all_bevs_[sear_res.first.gidx], ConstellationPair(db.cfg_.q_levels_[ll], sear_res.first.seq, seq), db.cfg_.cont_sim_cfg_);
    }
  }
  cand_mng.tidy();
  std::vector<std::shared_ptr<const ContourManager>> rc;
  std::vector<double> corr;
  std::vector<Iso2d> tfs;
  const int n_res = cand_mng.fineOptimize(db.cfg_.max_fine_opt_, rc, corr, tfs);
  std::memset(res, 0, sizeof(*res));
  int idx = -1;
  if (n_res)
    for (size_t i = 0; i < db.all_bevs_.size(); i++)
      if (db.all_bevs_[i].get() == rc[0].get()) {
        idx = (int)i;
        break;
      }
  fill_result(cand_mng, n_res, idx, corr, tfs, res);
  res->n_knn_hits = n_hits;
}

// orc_check_hints with the dynamic bars: scores[i] = {ovlp_sum, max_one, in_ang_rng, indiv_sim, orie_sim, passed}
void orcdyn_check_hints(void *tgt, void **cands, int n_cands, const int32_t *hints /*[n][4]*/, int n_hints, const cc_sim_cfg_t *sim,
                        const cc_score_t *lb, const cc_score_t *ub, int max_fine_opt, int dyn, cc_query_result_t *res,
                        int32_t *scores /*[n][6]*/) {
  ContourSimThresConfig cs;
  cs.ta_cell_cnt = sim->ta_cell_cnt;
  cs.tp_cell_cnt = sim->tp_cell_cnt;
  cs.tp_eigval = sim->tp_eigval;
  cs.ta_h_bar = sim->ta_h_bar;
  cs.ta_rcom = sim->ta_rcom;
  cs.tp_rcom = sim->tp_rcom;
  DynCandidateManager mng(((ScanH *)tgt)->cm, toScore(lb), toScore(ub), dyn != 0);
  for (int i = 0; i < n_hints; i++) {
    const int32_t *h = hints + 4 * i;
    const int before = mng.cand_aft_check3;
    CandidateScoreEnsemble s = mng.check(((ScanH *)cands[h[0]])->cm, ConstellationPair(h[1], h[2], h[3]), cs);
    if (scores) {
      int32_t *o = scores + 6 * i;
      o[0] = s.sim_constell.i_ovlp_sum;
      o[1] = s.sim_constell.i_ovlp_max_one;
      o[2] = s.sim_constell.i_in_ang_rng;
      o[3] = s.sim_pair.i_indiv_sim;
      o[4] = s.sim_pair.i_orie_sim;
      o[5] = mng.cand_aft_check3 > before ? 1 : 0;
    }
  }
  mng.tidy();
  std::vector<std::shared_ptr<const ContourManager>> rc;
  std::vector<double> corr;
  std::vector<Iso2d> tfs;
  const int n_res = mng.fineOptimize(max_fine_opt, rc, corr, tfs);
  std::memset(res, 0, sizeof(*res));
  int idx = -1;
  if (n_res)
    for (int i = 0; i < n_cands; i++)
      if (((ScanH *)cands[i])->cm.get() == rc[0].get()) {
        idx = i;
        break;
      }
  fill_result(mng, n_res, idx, corr, tfs, res);
  res->n_knn_hits = n_hints;
}

}  // extern "C"
