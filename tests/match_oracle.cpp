// TEST INFRASTRUCTURE: the oracle of the matched contour pairs behind a candidate (include/cont2_amd_matches.h).  The hint flow of
// orc_check_hints_cands with one more export: the constellation of the proposal tidyUpCandidates selects.  The oracle
// restatement (oracle/cont2_oracle.cpp) is included unchanged; built by tests/match_oracle.py with the oracle's flags:
//   g++ -O3 -std=c++17 -fPIC -ffp-contract=off -shared -I<repo>/oracle -I<repo>/include match_oracle.cpp
#include "../oracle/cont2_oracle.cpp"

extern "C" {
// checkCandWithHint for every hint in the given order (hints[i] = {index into cands[], level, seq_src, seq_tgt}), then per
// candidate in candidates_ order (first appearance):
//   ci[k][0] index into cands[], [1] anch_props_.size(), [2] idx_sel of tidyUpCandidates (first proposal with the most votes),
//   [3] 1 if the candidate survives tidyUpCandidates, [4] vote_cnt_ of the selected proposal, [5] its constell_.size();
//   cf[k][0] area_perc_ of the selected proposal by tidyUpCandidates' expression, evaluated here before tidyUpCandidates runs;
//   cf[k][1] for a survivor the figure tidyUpCandidates itself left in anch_props_[0].area_perc_ after its swap, else 0;
//   keys[k][j] = {level, seq_src, seq_tgt} of the selected proposal's constell_ in the map's order, j < min(ci[k][5], key_cap).
// Returns the number of candidates (at most cap are written).
int orcx_check_hints_matches(void *tgt, void **cands, int n_cands, const int32_t *hints /*[n][4]*/, int n_hints, const cc_sim_cfg_t *sim,
                             const cc_score_t *lb, const cc_score_t *ub, int cap, int key_cap, int32_t *ci /*[cap][6]*/, float *cf /*[cap][2]*/,
                             int8_t *keys /*[cap][key_cap][3]*/) {
  ContourSimThresConfig cs;
  cs.ta_cell_cnt = sim->ta_cell_cnt;
  cs.tp_cell_cnt = sim->tp_cell_cnt;
  cs.tp_eigval = sim->tp_eigval;
  cs.ta_h_bar = sim->ta_h_bar;
  cs.ta_rcom = sim->ta_rcom;
  cs.tp_rcom = sim->tp_rcom;
  auto tcm = ((ScanH *)tgt)->cm;
  CandidateManager mng(tcm, toScore(lb), toScore(ub));
  for (int i = 0; i < n_hints; i++) {
    const int32_t *h = hints + 4 * i;
    mng.checkCandWithHint(((ScanH *)cands[h[0]])->cm, ConstellationPair(h[1], h[2], h[3]), cs);
  }
  const int n = (int)mng.candidates_.size();
  std::vector<const ContourManager *> who(n);
  for (int k = 0; k < n; k++) {
    const auto &c = mng.candidates_[k];
    who[k] = c.cm_cand_.get();
    if (k >= cap) continue;
    int32_t *oi = ci + 6 * k;
    for (int j = 0; j < 6; j++) oi[j] = 0;
    cf[2 * k] = cf[2 * k + 1] = 0;
    oi[0] = -1;
    for (int j = 0; j < n_cands; j++)
      if (((ScanH *)cands[j])->cm.get() == who[k]) oi[0] = j;
    oi[1] = (int)c.anch_props_.size();
    int idx_sel = 0;
    std::vector<float> area(c.anch_props_.size(), 0.f);
    for (size_t p = 0; p < c.anch_props_.size(); p++) {
      const auto &pr = c.anch_props_[p];
      std::vector<float> lev_perc(tcm->getConfig().lv_grads_.size(), 0);
      for (const auto &e : pr.constell_) lev_perc[e.first.level] += e.second;
      float perc = 0;
      for (int j = 0; j < NUM_BIN_KEY_LAYER; j++) perc += LAYER_AREA_WEIGHTS[j] * lev_perc[DIST_BIN_LAYERS[j]];
      area[p] = perc;
      if (pr.vote_cnt_ > c.anch_props_[idx_sel].vote_cnt_) idx_sel = (int)p;
    }
    const auto &sel = c.anch_props_[idx_sel];
    oi[2] = idx_sel;
    oi[4] = sel.vote_cnt_;
    oi[5] = (int)sel.constell_.size();
    cf[2 * k] = area[idx_sel];
    int j = 0;
    for (const auto &e : sel.constell_) {
      if (j >= key_cap) break;
      int8_t *o = keys + ((size_t)k * key_cap + j) * 3;
      o[0] = (int8_t)e.first.level;
      o[1] = (int8_t)e.first.seq_src;
      o[2] = (int8_t)e.first.seq_tgt;
      j++;
    }
  }
  mng.tidyUpCandidates();
  for (const auto &c : mng.candidates_)
    for (int k = 0; k < n && k < cap; k++)
      if (who[k] == c.cm_cand_.get()) {
        ci[6 * k + 3] = 1;
        cf[2 * k + 1] = c.anch_props_[0].area_perc_;
      }
  return n;
}
}
