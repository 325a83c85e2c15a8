// TEST INFRASTRUCTURE: the oracle's whole kNN lists (QueryDebug::knn, every hit up to nnk), for large-k databases whose
// hits go beyond the CC_KNN_MAX entries orc_db_query copies out.  The oracle restatement (oracle/cont2_oracle.cpp) is
// included unchanged; built by the tests with the oracle's flags:
//   g++ -O3 -std=c++17 -fPIC -ffp-contract=off -shared -I<repo>/oracle -I<repo>/include knn_full_oracle.cpp
#include "../oracle/cont2_oracle.cpp"

extern "C" {
// knn: [3][6][stride] hits in the reference's order, knn_cnt: [3][6] (untruncated); returns the query's n_res
int orcknn_db_query(void *d, void *scan, const cc_score_t *lb, const cc_score_t *ub, int stride, cc_knn_hit_t *knn, int32_t *knn_cnt) {
  ContourDB &db = *((DbH *)d)->db;
  std::vector<std::shared_ptr<const ContourManager>> cands;
  std::vector<double> corr;
  std::vector<Iso2d> tfs;
  ContourDB::QueryDebug dbg;
  db.queryRangedKNN(((ScanH *)scan)->cm, toScore(lb), toScore(ub), cands, corr, tfs, &dbg);
  const int piv = ((ScanH *)scan)->cm->getConfig().piv_firsts_;
  for (size_t k = 0; k < dbg.knn.size(); k++) {
    const int ll = (int)k / piv, seq = (int)k % piv;
    knn_cnt[ll * CC_NPIV + seq] = (int)dbg.knn[k].size();
    for (size_t j = 0; j < dbg.knn[k].size() && (int)j < stride; j++) {
      cc_knn_hit_t &h = knn[(size_t)(ll * CC_NPIV + seq) * stride + j];
      h.gidx = (int32_t)dbg.knn[k][j].first.gidx;
      h.level = (int16_t)dbg.knn[k][j].first.level;
      h.seq = (int16_t)dbg.knn[k][j].first.seq;
      h.dist_sq = dbg.knn[k][j].second;
    }
  }
  return (int)cands.size();
}
}
