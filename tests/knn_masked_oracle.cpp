// TEST INFRASTRUCTURE: the oracle of a masked query.  A masked query behaves as if the keys of every scan outside its set were
// not in the buckets' trees: here every bucket's data_tree_ / gkidx_tree_ is filtered to the allowed scans (bucket_ranges_ and
// the buffers are left alone), the trees are rebuilt where they were built, the oracle's own query runs, and everything is put
// back.  The oracle restatement (oracle/cont2_oracle.cpp) is included unchanged; built by tests/masked_oracle.py with the
// oracle's flags:
//   g++ -O3 -std=c++17 -fPIC -ffp-contract=off -shared -I<repo>/oracle -I<repo>/include knn_masked_oracle.cpp
#include "../oracle/cont2_oracle.cpp"

extern "C" {
// row: [row_words] words, bit g & 31 of word g >> 5 set = scan g may answer (a scan at or beyond 32 * row_words may not), or
// NULL: no restriction.  res: as orc_db_query's.  knn: [3][6][stride] whole hit lists in the reference's order (up to stride
// entries each), knn_cnt: [3][6] (untruncated); both may be NULL.
void orcm_db_query(void *d, void *scan, const cc_score_t *lb, const cc_score_t *ub, const uint32_t *row, int row_words,
                   cc_query_result_t *res, int stride, cc_knn_hit_t *knn, int32_t *knn_cnt) {
  ContourDB &db = *((DbH *)d)->db;
  struct Saved {
    std::vector<RetrievalKey> data;
    std::vector<IndexOfKey> gk;
    std::shared_ptr<void> kd;
  };
  std::vector<Saved> saved;
  if (row)
    for (auto &layer : db.layer_db_)
      for (auto &b : layer.buckets_) {
        saved.push_back(Saved{b.data_tree_, b.gkidx_tree_, b.kd_});
        std::vector<RetrievalKey> data;
        std::vector<IndexOfKey> gk;
        for (size_t p = 0; p < b.data_tree_.size(); p++) {
          const size_t g = (size_t)b.gkidx_tree_[p].gidx;
          if (g < (size_t)32 * (size_t)row_words && ((row[g >> 5] >> (g & 31)) & 1u)) {
            data.push_back(b.data_tree_[p]);
            gk.push_back(b.gkidx_tree_[p]);
          }
        }
        b.data_tree_.swap(data);
        b.gkidx_tree_.swap(gk);
        b.kd_.reset();
        if (b.tree_built) b.rebuildTree();
      }
  orc_db_query(d, scan, lb, ub, res, nullptr, nullptr);
  if (knn || knn_cnt) {
    std::vector<std::shared_ptr<const ContourManager>> cands;
    std::vector<double> corr;
    std::vector<Iso2d> tfs;
    ContourDB::QueryDebug dbg;
    db.queryRangedKNN(((ScanH *)scan)->cm, toScore(lb), toScore(ub), cands, corr, tfs, &dbg);
    const int piv = ((ScanH *)scan)->cm->getConfig().piv_firsts_;
    for (size_t k = 0; k < dbg.knn.size(); k++) {
      const int ll = (int)k / piv, seq = (int)k % piv;
      if (knn_cnt) knn_cnt[ll * CC_NPIV + seq] = (int)dbg.knn[k].size();
      if (knn)
        for (size_t j = 0; j < dbg.knn[k].size() && (int)j < stride; j++) {
          cc_knn_hit_t &h = knn[(size_t)(ll * CC_NPIV + seq) * stride + j];
          h.gidx = (int32_t)dbg.knn[k][j].first.gidx;
          h.level = (int16_t)dbg.knn[k][j].first.level;
          h.seq = (int16_t)dbg.knn[k][j].first.seq;
          h.dist_sq = dbg.knn[k][j].second;
        }
    }
  }
  if (row) {
    size_t i = 0;
    for (auto &layer : db.layer_db_)
      for (auto &b : layer.buckets_) {
        b.data_tree_.swap(saved[i].data);
        b.gkidx_tree_.swap(saved[i].gk);
        b.kd_ = saved[i].kd;
        i++;
      }
  }
}
}
