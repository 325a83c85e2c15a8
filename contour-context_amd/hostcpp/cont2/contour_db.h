// Host mirror of include/cont2/contour_db.h (ContourDB, configs, CandidateScoreEnsemble) and of the two
// ConstellCorrelation statics the drivers call (include/cont2/correlation.h:241-296), on top of the C-ABI.
#pragma once
#include <algorithm>
#include <deque>
#include <memory>

#include "../tools/bm_util.h"
#include "contour_mng.h"
#include "../../../include/cont2_amd_matches.h"
#include "../../../include/cont2_amd_lists.h"

// The reference's DYNAMIC_THRES=1 build (CMakeLists.txt:19-20; contour_db.h:439-466, 566-574) raises the lower bars of a
// query's checks from candidate to candidate inside CandidateManager.  Built with that macro, every database of this mirror
// runs in the library's dynamic mode (cc_db_set_dynamic_thres): the device evaluates a query's checks side by side under the
// initial bars and then replays them in order under the rising ones.
#if defined(DYNAMIC_THRES) && DYNAMIC_THRES
#define CC_MIRROR_DYNAMIC_THRES 1
#else
#define CC_MIRROR_DYNAMIC_THRES 0
#endif

// As in the reference (contour_db.h:23): the library records its stage timers ("KNN search", "Constell", "L2 opt") into a
// profiler object that the EXECUTABLE defines.
extern SequentialTimeProfiler stp;

// contour_db.h:54-57
struct TreeBucketConfig {
  double max_elapse_ = 25.0;
  double min_elapse_ = 15.0;
};
// contour_db.h:244-250
struct CandidateScoreEnsemble {
  ScoreConstellSim sim_constell;
  ScorePairwiseSim sim_pair;
  ScorePostProc sim_post;
};
// contour_db.h:658-669
struct ContourDBConfig {
  int nnk_ = 50;
  int max_fine_opt_ = 10;
  std::vector<int> q_levels_;
  ContourSimThresConfig cont_sim_cfg_;
  TreeBucketConfig tb_cfg_;
};

class ContourDB {
  const ContourDBConfig cfg_;
  mutable cc_db *db_ = nullptr;  // created lazily by the first call that sees a ContourManager (queryRangedKNN is const)
  int capacity_;
  std::vector<std::shared_ptr<const ContourManager>> all_bevs_;
  std::vector<double> all_ts_;   // addScan's time stamp and pushAndBalance's seed of every added scan: what a rebuild needs
  std::vector<int> all_seed_;

  // ---- read-ahead of the database (mirror-only; the reference's loop is strictly sequential) ----
  // The driver's loop is  query(i) -> add(i) -> query(i+1) -> ...  and every call waits for a chain of ~20 small kernels.
  // When the scan source has published the scans that come next (cc_host::lookahead(): the evaluator mirror's read-ahead)
  // the database works ahead on the device: it appends scan k and queues scan k+1's query at epoch k+1 -- exactly the
  // state the sequential loop queries it in -- for up to SPEC_DEPTH scans, several chains in flight.  The driver's later
  // calls are then VALIDATED against that work instead of launching it: queryRangedKNN(k) hands out the queued answer if it
  // is the same scan with the same thresholds, addScan / pushAndBalance(k) is a no-op if it is the same scan, time stamp
  // and seed.  Any other call sequence stays correct: a different query is answered at the official epoch (an epoch hides
  // the scans appended after it), a different add REBUILDS the device database from the scans the driver really added.
  struct Spec {
    cc_scan *scan = nullptr;
    double ts = 0;
    int seed = 0;
    cc_score_t lb, ub;
    std::shared_ptr<std::vector<cc_query_result_t>> block;  // the answers of the batch the scan was queued with (epoch = position of the scan)
    int idx = 0;                                             // ... this scan's among them; filled by cc_db_query_collect / _wait
    bool collected = false;
    int max_ret = 1;                                         // setMaxReturn when the scan was queued; > 1: the batch's ranked lists
    std::shared_ptr<std::vector<cc_ranked_cand_t>> rblock;  // [batch][max_ret]
    std::shared_ptr<std::vector<int32_t>> nblock;           // [batch]
    bool detail = false;                                    // setWantDetail when the scan was queued: the batch's detail rows
    std::shared_ptr<std::vector<cc_ranked_detail_t>> dblock; // [batch][max_ret], travels with rblock
    double matches = -1.0;                                  // setWantMatches when the scan was queued (< 0: off): the batch's match rows
    std::shared_ptr<std::vector<cc_ranked_match_t>> mblock; // [batch][max_ret], travels with rblock
    cc_query_result_t *result() const { return block->data() + idx; }
  };
  bool want_detail_ = false;  // setWantDetail: the answers go through the ranked calls' _detail forms (also with max_ret_ == 1)
  mutable std::vector<cc_ranked_detail_t> last_details_;  // lastDetails()
  double want_matches_ = -1.0;  // setWantMatches: inlier_px, or < 0: off.  On: the answers go through the *_matched forms (also with max_ret_ == 1)
  mutable std::vector<cc_ranked_match_t> last_matches_;  // lastMatches()
  bool wantMatches() const { return want_matches_ >= 0.0; }
  bool rankedPath() const { return max_ret_ > 1 || want_detail_ || wantMatches(); }
  int max_ret_ = 1;  // setMaxReturn: entries queryRangedKNN / verifyCandidates hand out (fineOptimize's ret_size, contour_db.h:630)
  static constexpr int SPEC_LOW = 2;  // fewer answers than this queued ahead of the driver: a step goes out with whatever has been published
  mutable std::deque<Spec> spec_;   // scans appended ahead of the driver, oldest first (spec_[j] sits at DB index n_official + j)
  mutable bool have_thres_ = false;
  mutable cc_score_t last_lb_, last_ub_;
  mutable long n_spec_hit_ = 0, n_spec_miss_ = 0, n_rebuild_ = 0;
  mutable double t_ra_[2] = {0, 0};  // host seconds in the two calls of a read-ahead step (CC_EVAL_TIMERS prints them)
  mutable long n_ra_ = 0, n_ra_scans_ = 0;
  mutable int ra_pause_ = 0, ra_backoff_ = 16;  // driver steps the read-ahead still sits out after a rebuild | the next pause (see rebuild())
  mutable const void *source_ = nullptr;  // the scan source of the driver's last scan (ContourManager::scanSource): the one sequence this database predicts
  mutable bool need_rebuild_ = false;  // the device database holds scans the driver has not added (and will not): rebuilt at the next call
  int hub_token_ = -1;
  static int specDepth() {
    static const int d = [] {
      // Scans worked ahead (CC_DB_READ_AHEAD=n, 0: off).  Round 5, first version (one scan per step, one chain of launches per
      // scan): the answers were there when the driver asked and the loop got SLOWER (2 500 -> 1 950 scans/s: every step needed
      // the newest published scan, whose single-scan ingest became the wait).  Batched (a step appends and queries
      // specBatch() scans with ONE chain each; the evaluator ingests its files eight at a time, cc_scan_ingest_batch):
      // 3 080 -> 8 200-8 900 scans/s on MI355X (profiles/r5/dropin_batched_read_ahead.txt).  On by default: 32 scans deep.
      const char *e = getenv("CC_DB_READ_AHEAD");
      return e ? std::max(0, atoi(e)) : 32;
    }();
    return d;
  }
  // scans per read-ahead step: as many of the published scans as have ARRIVED, at most specBatch() (CC_DB_READ_AHEAD_BATCH, default
  // CC_SCAN_BATCH_MAX) and -- unless the queue is about to run dry -- at least specMin() (half of that, at most 8): the step follows
  // the source's own batches (the evaluator publishes eight or sixteen scans at a time)
  static int specBatch() {
    static const int b = [] {
      const char *e = getenv("CC_DB_READ_AHEAD_BATCH");
      const int v = e ? atoi(e) : CC_SCAN_BATCH_MAX;
      return std::max(1, std::min({v, CC_SCAN_BATCH_MAX, std::max(1, specDepth())}));
    }();
    return b;
  }
  static int specMin() { return std::max(1, std::min(8, specBatch() / 2 + specBatch() % 2)); }
  static bool same(const cc_score_t &a, const cc_score_t &b) { return memcmp(&a, &b, sizeof(cc_score_t)) == 0; }
  static void die_cc() {
    fprintf(stderr, "cont2_amd: %s\n", cc_last_error());
    abort();
  }
  void collectSpec() const {  // every queued answer is on the host afterwards
    bool pending = false;
    for (auto &sp : spec_) pending = pending || !sp.collected;
    if (!pending) return;
    if (cc_db_query_wait(db_) != CC_OK) die_cc();
    for (auto &sp : spec_) sp.collected = true;
  }
  // the device database back to the scans the driver has added (all_bevs_): after the driver left the predicted sequence
  // A rebuild costs one append per scan the driver has added so far (batched, sixteen handles per call): a driver that keeps
  // leaving the predicted sequence (every fifth scan never added, two databases fed alternately) would pay that again and
  // again.  So every rebuild PAUSES the read-ahead for ra_backoff_ of the driver's steps and doubles that number: a driver that
  // deviates at a steady rate meets O(log n) rebuilds, one that deviated once is back to full speed sixteen scans later.
  void rebuild() const {
    n_rebuild_++;
    need_rebuild_ = false;
    ra_pause_ = ra_backoff_;
    ra_backoff_ = std::min(ra_backoff_ * 2, 1 << 24);
    if (db_) {
      cc_db_query_wait(db_);
      cc_db_destroy(db_);
      db_ = nullptr;
    }
    spec_.clear();
    if (all_bevs_.empty()) return;
    ensure(*all_bevs_[0]);
    for (size_t i = 0; i < all_bevs_.size();) {
      cc_scan *hs[CC_SCAN_BATCH_MAX];
      int n = 0;
      while (i + n < all_bevs_.size() && n < CC_SCAN_BATCH_MAX) {
        cc_scan *h = all_bevs_[i + n]->scanHandle();
        if (!h || !cc_scan_on_device(h)) break;
        hs[n++] = h;
      }
      int rc;
      if (n > 0) {
        rc = cc_db_add_scan_batch(db_, hs, n, &all_ts_[i], &all_seed_[i]);
        i += (size_t)n;
      } else {  // a scan whose descriptor was moved to the host goes by that copy
        rc = cc_db_add_scan_host(db_, &all_bevs_[i]->desc(), all_ts_[i], all_seed_[i]);
        i++;
      }
      if (rc != CC_OK) die_cc();
    }
  }
  void dropReadAhead() {  // the scan source is about to release the scans spec_ refers to: nothing of them may stay in flight
    if (spec_.empty()) return;
    if (db_ && cc_db_query_wait(db_) != CC_OK) die_cc();
    spec_.clear();
    need_rebuild_ = true;  // their records are still in the device database: rebuilt when (if) the database is used again
  }
  // append + queue for the scans the source has published, behind what is there already: up to specBatch() scans per step
  // (ONE append and ONE chain of query launches for all of them: the loop is bound by the number of launches, host and
  // device side, not by their work).  A step waits until a whole batch has been published unless the queued work is
  // about to run out.
  void readAhead() const {
    if (specDepth() <= 0 || !have_thres_ || !db_) return;
    if (ra_pause_ > 0) {  // called once per pushAndBalance: the driver's steps
      ra_pause_--;
      return;
    }
    if (!source_) return;  // the last scan came from a source that publishes nothing
    const auto up = cc_host::lookahead().snapshot(source_);
    // the published scans that are not in spec_ yet must continue it: spec_ = a prefix of (scan in the driver's hands?, upcoming...)
    size_t pos = 0;
    if (!spec_.empty()) {  // what follows spec_.back() among the published scans is new
      bool found = false;
      for (size_t j = 0; j < up.size(); j++)
        if (up[j].scan == spec_.back().scan) {
          pos = j + 1;
          found = true;
        }
      if (!found) return;
    }
    int seed_next = (all_seed_.empty() ? 0 : all_seed_.back() + 1) + (int)spec_.size();  // the driver counts its scans (batch_bin_test.cpp:237)
    for (;;) {
      const int room = specDepth() - (int)spec_.size();
      int n = (int)std::min<size_t>(up.size() - pos, (size_t)std::max(0, std::min(room, specBatch())));
      const int epoch0 = cc_db_size(db_);
      n = std::min(n, capacity_ - 1 - epoch0);
      for (int j = 0; j < n; j++)
        if (!cc_scan_on_device(up[pos + j].scan)) n = j;
      if (n <= 0) return;
      if ((int)spec_.size() > SPEC_LOW) {  // the queue is not about to run dry: only scans that have ARRIVED, and enough of them
        if (n < specMin()) return;         // (a published scan may still be on its way through K1 / K2: the append would wait for it)
        int n_ready = 0;
        while (n_ready < n && cc_scan_ready(up[pos + n_ready].scan)) n_ready++;
        n = n_ready;
        if (n < specMin()) return;
      }
      cc_scan *scans[CC_SCAN_BATCH_MAX];
      double ts[CC_SCAN_BATCH_MAX];
      int32_t seed[CC_SCAN_BATCH_MAX], epoch[CC_SCAN_BATCH_MAX];
      auto block = std::make_shared<std::vector<cc_query_result_t>>((size_t)n);
      for (int j = 0; j < n; j++) {
        scans[j] = up[pos + j].scan;
        ts[j] = up[pos + j].ts;
        seed[j] = seed_next++;
        epoch[j] = epoch0 + j;  // scan j's query sees the database as it is after the scans before it (an epoch hides the later ones)
      }
      TicToc t0;
      if (cc_db_add_scan_batch(db_, scans, n, ts, seed) != CC_OK) die_cc();
      t_ra_[0] += t0.toc();
      TicToc t1;
      std::shared_ptr<std::vector<cc_ranked_cand_t>> rblock;
      std::shared_ptr<std::vector<int32_t>> nblock;
      std::shared_ptr<std::vector<cc_ranked_detail_t>> dblock;
      std::shared_ptr<std::vector<cc_ranked_match_t>> mblock;
      if (rankedPath()) {  // the answers carry their ranked lists (and, if wanted, the detail and the match rows)
        rblock = std::make_shared<std::vector<cc_ranked_cand_t>>((size_t)n * max_ret_);
        nblock = std::make_shared<std::vector<int32_t>>((size_t)n);
        const cc_rank_out_t ro = {rblock->data(), nblock->data(), max_ret_, 0};
        if (wantMatches()) {
          if (want_detail_) dblock = std::make_shared<std::vector<cc_ranked_detail_t>>((size_t)n * max_ret_);
          mblock = std::make_shared<std::vector<cc_ranked_match_t>>((size_t)n * max_ret_);
          const cc_match_out_t mo = {mblock->data(), want_matches_};
          if (cc_db_query_scan_batch_submit_matched(db_, scans, n, epoch, &last_lb_, &last_ub_, block->data(), &ro, want_detail_ ? dblock->data() : nullptr, &mo) != CC_OK)
            die_cc();
        } else if (want_detail_) {
          dblock = std::make_shared<std::vector<cc_ranked_detail_t>>((size_t)n * max_ret_);
          if (cc_db_query_scan_batch_submit_ranked_detail(db_, scans, n, epoch, &last_lb_, &last_ub_, block->data(), &ro, dblock->data()) != CC_OK)
            die_cc();
        } else if (cc_db_query_scan_batch_submit_ranked(db_, scans, n, epoch, &last_lb_, &last_ub_, block->data(), &ro) != CC_OK) {
          die_cc();
        }
      } else if (cc_db_query_scan_batch_submit(db_, scans, n, epoch, &last_lb_, &last_ub_, block->data()) != CC_OK) {
        die_cc();
      }
      t_ra_[1] += t1.toc();
      n_ra_++;
      n_ra_scans_ += n;
      for (int j = 0; j < n; j++) {
        Spec sp;
        sp.scan = scans[j];
        sp.ts = ts[j];
        sp.seed = seed[j];
        sp.lb = last_lb_;
        sp.ub = last_ub_;
        sp.block = block;
        sp.idx = j;
        sp.max_ret = max_ret_;
        sp.rblock = rblock;
        sp.nblock = nblock;
        sp.detail = want_detail_;
        sp.dblock = dblock;
        sp.matches = want_matches_;
        sp.mblock = mblock;
        spec_.push_back(std::move(sp));
      }
      pos += (size_t)n;
    }
  }
  // the answer of spec_[i] on the host (its whole batch's chain is waited for; batches queued behind it stay in flight)
  void collectOne(size_t i) const {
    Spec &sp = spec_[i];
    if (sp.collected) return;
    if (cc_db_query_collect(db_, sp.result(), 1) != CC_OK) die_cc();
    for (auto &o : spec_)
      if (o.block == sp.block) o.collected = true;
  }

  static cc_score_t to_c(const CandidateScoreEnsemble &e) {
    cc_score_t s;
    s.i_ovlp_sum = e.sim_constell.i_ovlp_sum;
    s.i_ovlp_max_one = e.sim_constell.i_ovlp_max_one;
    s.i_in_ang_rng = e.sim_constell.i_in_ang_rng;
    s.i_indiv_sim = e.sim_pair.i_indiv_sim;
    s.i_orie_sim = e.sim_pair.i_orie_sim;
    s.correlation = e.sim_post.correlation;
    s.area_perc = e.sim_post.area_perc;
    s.neg_est_dist = e.sim_post.neg_est_dist;
    return s;
  }
  void ensure(const ContourManager &cm) const {
    if (db_) return;
    cc_db_cfg_t d;
    cc_default_db_cfg(&d);
    d.nnk = cfg_.nnk_;
    d.max_fine_opt = cfg_.max_fine_opt_;
    d.n_q_levels = (int)cfg_.q_levels_.size();
    for (int i = 0; i < d.n_q_levels && i < CC_NQLEV; i++) d.q_levels[i] = cfg_.q_levels_[i];
    d.cont_sim.ta_cell_cnt = cfg_.cont_sim_cfg_.ta_cell_cnt;
    d.cont_sim.tp_cell_cnt = cfg_.cont_sim_cfg_.tp_cell_cnt;
    d.cont_sim.tp_eigval = cfg_.cont_sim_cfg_.tp_eigval;
    d.cont_sim.ta_h_bar = cfg_.cont_sim_cfg_.ta_h_bar;
    d.cont_sim.ta_rcom = cfg_.cont_sim_cfg_.ta_rcom;
    d.cont_sim.tp_rcom = cfg_.cont_sim_cfg_.tp_rcom;
    d.max_elapse = cfg_.tb_cfg_.max_elapse_;
    d.min_elapse = cfg_.tb_cfg_.min_elapse_;
    if (cc_db_create(cc_host::context(cm.ccfg()), &d, capacity_, &db_) != CC_OK) {
      fprintf(stderr, "cont2_amd: %s\n", cc_last_error());
      abort();
    }
    // per-stage DEVICE times of every query under the reference's stage names (six events per query: they cost a few
    // per cent, so only on request); the wall time of the call is recorded either way
    if (getenv("CC_STP_DEVICE_TIMERS")) cc_db_profile_enable(db_, 1);
    if (CC_MIRROR_DYNAMIC_THRES && cc_db_set_dynamic_thres(db_, 1) != CC_OK) {
      fprintf(stderr, "cont2_amd: %s\n", cc_last_error());
      abort();
    }
    if (specDepth() > 0) cc_db_set_lanes(db_, 4);  // one chain per queued query
  }

 public:
  explicit ContourDB(const ContourDBConfig &config, int capacity_scans = 65536) : cfg_(config), capacity_(capacity_scans) {
    CC_CHECK(!cfg_.q_levels_.empty());
    cc_host::runtime_warm();
    if (specDepth() > 0) hub_token_ = cc_host::lookahead().subscribe([this](const void *src) {
      if (src == source_) dropReadAhead();  // (another source's scans are not among the ones this database has worked ahead on)
    });
    if (hub_token_ >= 0) cc_host::lookahead().subscribeRelease(hub_token_, [this](cc_scan *h) {
      for (const Spec &sp : spec_)
        if (sp.scan == h) {  // a scan this database has worked ahead on dies before the driver added it: its handle's address may come back
          dropReadAhead();
          break;
        }
    });
  }
  ContourDB(const ContourDB &) = delete;
  ContourDB &operator=(const ContourDB &) = delete;
  ~ContourDB() {
    if (hub_token_ >= 0) cc_host::lookahead().unsubscribe(hub_token_);
    if (getenv("CC_EVAL_TIMERS"))
    {
      if (n_ra_ > 0)
        fprintf(stderr, "[ContourDB read-ahead, mean host us per step over %ld steps of %.1f scans] append %.1f  query submit %.1f\n", n_ra_,
                (double)n_ra_scans_ / n_ra_, 1e6 * t_ra_[0] / n_ra_, 1e6 * t_ra_[1] / n_ra_);
      fprintf(stderr, "[ContourDB read-ahead] answers handed out from queued queries %ld, launched on the spot %ld, rebuilds %ld\n", n_spec_hit_, n_spec_miss_, n_rebuild_);
    }
    cc_db_destroy(db_);
  }

  // Mirror-only: how many candidates a query hands out -- what fineOptimize would return with ret_size = n instead of its
  // hard-wired 1 (contour_db.h:630): the refined candidates by refined correlation, best first.  1 (the default) is the reference.
  void setMaxReturn(int n) {
    CC_CHECK(n >= 1 && n <= CC_RANK_MAX);
    max_ret_ = n;  // (answers queued with another setting are not handed out: queryRangedKNN asks again, at the official epoch)
  }
  int maxReturn() const { return max_ret_; }
  // Mirror-only: collect, next to every candidate queryRangedKNN / verifyCandidates hands out, its cc_ranked_detail_t (curvature of
  // -correlation at the pose, the refinement's start, initial correlation, iterations, termination, pair count): lastDetails()
  // after the call, one row per returned candidate, in their order.  Off (the default): the calls the mirror always made.
  void setWantDetail(bool on) { want_detail_ = on; }  // (answers queued with another setting are asked again, as for setMaxReturn)
  bool wantDetail() const { return want_detail_; }
  const std::vector<cc_ranked_detail_t> &lastDetails() const { return last_details_; }
  // Mirror-only: collect, next to every candidate queryRangedKNN / queryStored / queryAllowed / verifyCandidates / verifyStored hands
  // out, its cc_ranked_match_t (include/cont2_amd_matches.h): the matched contour pairs the pose was built from -- what the reference
  // keeps in CandidateManager (anch_props_[0].constell_) and its drivers draw -- the proposal's votes and area, and the pairs'
  // residuals at the returned pose with the number within inlier_px pixels.  lastMatches() after the call, one row per returned
  // candidate, in their order; cc_match_pairs() lists a row's pairs.  A negative value (the default) switches it off: the calls the
  // mirror always made.  (Answers queued with another setting are asked again, as for setMaxReturn.)
  void setWantMatches(double inlier_px) { want_matches_ = inlier_px >= 0.0 ? inlier_px : -1.0; }
  const std::vector<cc_ranked_match_t> &lastMatches() const { return last_matches_; }

  // contour_db.h:698-703
  void queryRangedKNN(const std::shared_ptr<const ContourManager> &q_ptr, const CandidateScoreEnsemble &thres_lb,
                      const CandidateScoreEnsemble &thres_ub, std::vector<std::shared_ptr<const ContourManager>> &cand_ptrs,
                      std::vector<double> &cand_corr, std::vector<Eigen::Isometry2d> &cand_tf) const {
    cand_ptrs.clear();
    cand_corr.clear();
    cand_tf.clear();
    ensure(*q_ptr);
    const cc_score_t lb = to_c(thres_lb), ub = to_c(thres_ub);
    cc_query_result_t r;
    cc_ranked_cand_t rl[CC_RANK_MAX];  // the ranked list (rankedPath())
    cc_ranked_detail_t dl[CC_RANK_MAX];  // ... and its detail rows (want_detail_)
    cc_ranked_match_t ml[CC_RANK_MAX];   // ... and its match rows (wantMatches())
    int32_t rn = 0;
    const cc_rank_out_t ro = {rl, &rn, max_ret_, 0};
    const cc_match_out_t mo = {ml, want_matches_};
    const bool rk = rankedPath(), wm = wantMatches();
    last_details_.clear();
    last_matches_.clear();
    TicToc wall;
    if (need_rebuild_) rebuild();
    last_lb_ = lb;
    last_ub_ = ub;
    have_thres_ = true;
    cc_scan *qh = q_ptr->scanHandle();
    if (!spec_.empty() && qh && spec_.front().scan == qh && same(spec_.front().lb, lb) && same(spec_.front().ub, ub) &&
        spec_.front().max_ret == max_ret_ && spec_.front().detail == want_detail_ && spec_.front().matches == want_matches_) {
      // the answer was queued when the scan was published (at the epoch the database is officially in now); only ITS chain is
      // waited for, the queries queued behind it stay in flight
      collectOne(0);
      const Spec &sp = spec_.front();
      r = *sp.result();
      if (rk) {
        rn = (*sp.nblock)[sp.idx];
        std::copy(sp.rblock->begin() + (size_t)sp.idx * max_ret_, sp.rblock->begin() + (size_t)(sp.idx + 1) * max_ret_, rl);
        if (want_detail_) std::copy(sp.dblock->begin() + (size_t)sp.idx * max_ret_, sp.dblock->begin() + (size_t)(sp.idx + 1) * max_ret_, dl);
        if (wm) std::copy(sp.mblock->begin() + (size_t)sp.idx * max_ret_, sp.mblock->begin() + (size_t)(sp.idx + 1) * max_ret_, ml);
      }
      n_spec_hit_++;
    } else {
      n_spec_miss_++;
      const int32_t epoch = (int32_t)all_bevs_.size();  // the scans appended ahead of the driver are hidden by the epoch
      int rc;
      if (qh && cc_scan_on_device(qh)) {
        rc = wm           ? cc_db_query_scan_batch_submit_matched(db_, &qh, 1, &epoch, &lb, &ub, &r, &ro, want_detail_ ? dl : nullptr, &mo)
             : want_detail_ ? cc_db_query_scan_batch_submit_ranked_detail(db_, &qh, 1, &epoch, &lb, &ub, &r, &ro, dl)
             : rk         ? cc_db_query_scan_batch_submit_ranked(db_, &qh, 1, &epoch, &lb, &ub, &r, &ro)
                          : cc_db_query_scan_submit(db_, qh, epoch, &lb, &ub, &r);
        const int r2 = cc_db_query_wait(db_);
        for (auto &sp : spec_) sp.collected = true;
        if (rc == CC_OK) rc = r2;
      } else {  // a scan that was offloaded goes by its host copy
        collectSpec();
        rc = wm           ? cc_db_query_batch_host_matched(db_, &q_ptr->desc(), 1, &epoch, &lb, &ub, &r, &ro, want_detail_ ? dl : nullptr, nullptr, &mo)
             : want_detail_ ? cc_db_query_batch_host_ranked_detail(db_, &q_ptr->desc(), 1, &epoch, &lb, &ub, &r, &ro, dl)
             : rk         ? cc_db_query_batch_host_ranked(db_, &q_ptr->desc(), 1, &epoch, &lb, &ub, &r, &ro)
                          : cc_db_query_batch_host(db_, &q_ptr->desc(), 1, &epoch, &lb, &ub, &r);
      }
      if (rc != CC_OK) die_cc();  // CHECK(sim_lb.strictSmaller(sim_ub)) etc.; also CC_ECAPACITY (the reference has no capacities)
    }
    stp.addSample("queryRangedKNN (wall)", wall.toc());
    {  // the reference's stage names (contour_db.h:755,772,787), with the device times of this query's kernels:
       // retrieval | checks + proposal merge | correlation + selection
      double ms[5];
      int nq = 0;
      if (getenv("CC_STP_DEVICE_TIMERS") && cc_db_profile_read(db_, ms, &nq) == CC_OK && nq > 0) {
        stp.addSample("KNN search", ms[0] * 1e-3);
        stp.addSample("Constell", (ms[1] + ms[2]) * 1e-3);
        stp.addSample("L2 opt", (ms[3] + ms[4]) * 1e-3);
      }
    }
    handOut(rk, r, rl, rn, dl, ml, cand_ptrs, cand_corr, cand_tf);
  }
  // an answer as the reference's result vectors hold it: the ranked list (with its detail and match rows), or the one candidate of
  // the plain call.  Returns the number of entries.
  int handOut(bool ranked, const cc_query_result_t &r, const cc_ranked_cand_t *rl, int rn, const cc_ranked_detail_t *dl, const cc_ranked_match_t *ml,
              std::vector<std::shared_ptr<const ContourManager>> &res_cand, std::vector<double> &res_corr,
              std::vector<Eigen::Isometry2d> &res_T) const {
    if (ranked) {
      for (int k = 0; k < rn; k++) pushRanked(all_bevs_, rl[k], res_cand, res_corr, res_T);
      if (want_detail_) last_details_.assign(dl, dl + rn);
      if (wantMatches()) last_matches_.assign(ml, ml + rn);
      return rn;
    }
    if (r.n_res > 0) {
      res_cand.push_back(all_bevs_[r.cand_gidx]);
      res_corr.push_back(r.correlation);
      Eigen::Isometry2d T;
      T.rotate(r.tf[2]);
      T.pretranslate(r.tf[0], r.tf[1]);
      res_T.push_back(T);
    }
    return r.n_res;
  }
  // Mirror-only: queryRangedKNN for a scan this database holds, by its index in adding order, against the database as it was
  // after `epoch` scans (epoch == idx: what queryRangedKNN answered when the driver queried that scan; a later epoch may return
  // the scan itself) -- from the records the database keeps (cc_db_query_submit_packed): no descriptor is needed, the scan's
  // ContourManager may have been offloaded.  Honours setMaxReturn / setWantDetail as queryRangedKNN does.
  void queryStored(int idx, int epoch, const CandidateScoreEnsemble &thres_lb, const CandidateScoreEnsemble &thres_ub,
                   std::vector<std::shared_ptr<const ContourManager>> &cand_ptrs, std::vector<double> &cand_corr,
                   std::vector<Eigen::Isometry2d> &cand_tf) const {
    cand_ptrs.clear();
    cand_corr.clear();
    cand_tf.clear();
    CC_CHECK(db_ && idx >= 0 && idx < (int)all_bevs_.size());  // (scans appended ahead of the driver are not the caller's yet)
    CC_CHECK(epoch >= 0 && epoch <= (int)all_bevs_.size());
    if (need_rebuild_) rebuild();
    const cc_score_t lb = to_c(thres_lb), ub = to_c(thres_ub);
    cc_query_result_t r;
    cc_ranked_cand_t rl[CC_RANK_MAX];
    cc_ranked_detail_t dl[CC_RANK_MAX];
    int32_t rn = 0;
    const cc_rank_out_t ro = {rl, &rn, max_ret_, 0};
    const bool rk = rankedPath();
    last_details_.clear();
    last_matches_.clear();
    cc_ranked_match_t ml[CC_RANK_MAX];
    const cc_match_out_t mo = {ml, want_matches_};
    const cc_packed_src_t own = {nullptr, nullptr, 0, 0};
    const int32_t rec = idx, ep = epoch;
    int rc = wantMatches() ? cc_db_query_submit_matched(db_, nullptr, &own, &rec, 1, &ep, &lb, &ub, &r, nullptr, nullptr, nullptr, &ro, want_detail_ ? dl : nullptr, nullptr, &mo)
                           : cc_db_query_submit_packed(db_, &own, &rec, 1, &ep, &lb, &ub, &r, nullptr, nullptr, nullptr, rk ? &ro : nullptr, want_detail_ ? dl : nullptr);
    const int r2 = cc_db_query_wait(db_);
    for (auto &sp : spec_) sp.collected = true;  // the wait collected every chain in flight
    if (rc == CC_OK) rc = r2;
    if (rc != CC_OK) die_cc();
    handOut(rk, r, rl, rn, dl, ml, cand_ptrs, cand_corr, cand_tf);
  }
  // Mirror-only: queryRangedKNN among the scans the caller allows -- scans of this database by their index in adding order
  // (another session's part of the map, the scans near a position prior, everything but a retired key frame) -- as if the other
  // scans' keys were not in the trees (cc_db_query_batch_host_masked): the search keeps the nnk_ nearest ALLOWED keys per anchor.
  // Synchronous, at the official epoch, like verifyCandidates; honours setMaxReturn / setWantDetail; the read-ahead queue is
  // neither consumed nor extended.
  void queryAllowed(const std::shared_ptr<const ContourManager> &q_ptr, const std::vector<int> &allowed_indices,
                    const CandidateScoreEnsemble &thres_lb, const CandidateScoreEnsemble &thres_ub,
                    std::vector<std::shared_ptr<const ContourManager>> &cand_ptrs, std::vector<double> &cand_corr,
                    std::vector<Eigen::Isometry2d> &cand_tf) const {
    cand_ptrs.clear();
    cand_corr.clear();
    cand_tf.clear();
    const int n_db = (int)all_bevs_.size();
    for (const int c : allowed_indices) CC_CHECK(c >= 0 && c < n_db);  // (scans appended ahead of the driver are not the caller's yet)
    ensure(*q_ptr);
    if (need_rebuild_) rebuild();
    const cc_score_t lb = to_c(thres_lb), ub = to_c(thres_ub);
    std::vector<uint32_t> row((size_t)(n_db + 31) / 32 + 1, 0u);
    for (const int c : allowed_indices) row[(size_t)c >> 5] |= 1u << (c & 31);
    const int32_t epoch = n_db, r0 = 0;
    const cc_scan_mask_t mask = {row.data(), 1, (int32_t)row.size(), &r0};
    cc_query_result_t r;
    cc_ranked_cand_t rl[CC_RANK_MAX];
    cc_ranked_detail_t dl[CC_RANK_MAX];
    int32_t rn = 0;
    const cc_rank_out_t ro = {rl, &rn, max_ret_, 0};
    const bool rk = rankedPath();
    last_details_.clear();
    last_matches_.clear();
    cc_ranked_match_t ml[CC_RANK_MAX];
    const cc_match_out_t mo = {ml, want_matches_};
    const int rc = wantMatches() ? cc_db_query_batch_host_matched(db_, &q_ptr->desc(), 1, &epoch, &lb, &ub, &r, &ro, want_detail_ ? dl : nullptr, &mask, &mo)
                                 : cc_db_query_batch_host_masked(db_, &q_ptr->desc(), 1, &epoch, &lb, &ub, &r, rk ? &ro : nullptr, want_detail_ ? dl : nullptr, &mask);
    for (auto &sp : spec_) sp.collected = true;  // the synchronous call (its wait) collected every chain in flight
    if (rc != CC_OK) die_cc();
    handOut(rk, r, rl, rn, dl, ml, cand_ptrs, cand_corr, cand_tf);
  }
  // Mirror-only: queryAllowed for callers whose set is a short index list (the result of a radius search over the poses): the same
  // answers, from the retrieval that enumerates the listed scans' keys instead of walking the layer under a bit row
  // (cc_db_query_batch_host_listed, include/cont2_amd_lists.h).  allowed_indices: strictly increasing, at most CC_LIST_SCANS_MAX.
  // Synchronous, at the official epoch; honours setMaxReturn / setWantDetail / setWantMatches like queryAllowed.
  void queryAmong(const std::shared_ptr<const ContourManager> &q_ptr, const std::vector<int> &allowed_indices,
                  const CandidateScoreEnsemble &thres_lb, const CandidateScoreEnsemble &thres_ub,
                  std::vector<std::shared_ptr<const ContourManager>> &cand_ptrs, std::vector<double> &cand_corr,
                  std::vector<Eigen::Isometry2d> &cand_tf) const {
    cand_ptrs.clear();
    cand_corr.clear();
    cand_tf.clear();
    const int n_db = (int)all_bevs_.size();
    for (const int c : allowed_indices) CC_CHECK(c >= 0 && c < n_db);  // (scans appended ahead of the driver are not the caller's yet)
    ensure(*q_ptr);
    if (need_rebuild_) rebuild();
    const cc_score_t lb = to_c(thres_lb), ub = to_c(thres_ub);
    const std::vector<int32_t> idx(allowed_indices.begin(), allowed_indices.end());
    const int32_t off[2] = {0, (int32_t)idx.size()};
    const int32_t epoch = n_db, r0 = 0;
    const cc_scan_lists_t lists = {idx.data(), off, 1, &r0};
    cc_query_result_t r;
    cc_ranked_cand_t rl[CC_RANK_MAX];
    cc_ranked_detail_t dl[CC_RANK_MAX];
    int32_t rn = 0;
    const cc_rank_out_t ro = {rl, &rn, max_ret_, 0};
    const bool rk = rankedPath();
    last_details_.clear();
    last_matches_.clear();
    cc_ranked_match_t ml[CC_RANK_MAX];
    const cc_match_out_t mo = {ml, want_matches_};
    const int rc = cc_db_query_batch_host_listed(db_, &q_ptr->desc(), 1, &epoch, &lb, &ub, &r, rk ? &ro : nullptr, want_detail_ ? dl : nullptr, &lists,
                                                 wantMatches() ? &mo : nullptr);
    for (auto &sp : spec_) sp.collected = true;  // the synchronous call (its wait) collected every chain in flight
    if (rc != CC_OK) die_cc();
    handOut(rk, r, rl, rn, dl, ml, cand_ptrs, cand_corr, cand_tf);
  }
  // one entry of a ranked list as the reference's result vectors hold it
  template <class Scans>
  static void pushRanked(const Scans &scans, const cc_ranked_cand_t &e, std::vector<std::shared_ptr<const ContourManager>> &res_cand,
                         std::vector<double> &res_corr, std::vector<Eigen::Isometry2d> &res_T) {
    res_cand.push_back(scans[e.cand_gidx]);
    res_corr.push_back(e.correlation);
    Eigen::Isometry2d T;
    T.rotate(e.tf[2]);
    T.pretranslate(e.tf[0], e.tf[1]);
    res_T.push_back(T);
  }
  // Mirror-only (no reference counterpart): score candidates the CALLER proposes -- scans of this database by their index in
  // adding order (odometry or GPS proximity, another descriptor, a re-check of accepted loops) -- instead of the ones the key
  // search retrieves.  At most CC_VERIFY_CANDS_MAX distinct indices.  Returns what the reference demo's loop over the
  // candidates' anchor pairs (test/kitti_read_bin_test.cpp:226-291: checkCandWithHint for every pair of existing anchors
  // whose keys are at most 1000 apart, candidate by candidate) + tidyUpCandidates + fineOptimize(max_fine_opt_) return: one
  // device pass (cc_db_verify_batch_host) whose hint list is generated on the device.
  int verifyCandidates(const std::shared_ptr<const ContourManager> &q_ptr, const std::vector<int> &cand_indices,
                       const CandidateScoreEnsemble &thres_lb, const CandidateScoreEnsemble &thres_ub,
                       std::vector<std::shared_ptr<const ContourManager>> &res_cand, std::vector<double> &res_corr,
                       std::vector<Eigen::Isometry2d> &res_T) const {
    return verifyCandidates(q_ptr, cand_indices, thres_lb, thres_ub, res_cand, res_corr, res_T, 1);
  }
  // verifyCandidates for a scan this database holds, by its index in adding order, from the records the database keeps
  // (cc_db_verify_submit_packed); idx may be among its own candidates.
  int verifyStored(int idx, const std::vector<int> &cand_indices, const CandidateScoreEnsemble &thres_lb, const CandidateScoreEnsemble &thres_ub,
                   std::vector<std::shared_ptr<const ContourManager>> &res_cand, std::vector<double> &res_corr,
                   std::vector<Eigen::Isometry2d> &res_T, int max_ret = 1) const {
    CC_CHECK(db_ && idx >= 0 && idx < (int)all_bevs_.size());
    return verifyFrom(nullptr, idx, cand_indices, thres_lb, thres_ub, res_cand, res_corr, res_T, max_ret);
  }
  // ... and the ranked list of them: up to max_ret (1..CC_RANK_MAX) of the candidates that survive, best first -- one verdict
  // per proposed candidate from one device pass.  Returns the number of entries.
  int verifyCandidates(const std::shared_ptr<const ContourManager> &q_ptr, const std::vector<int> &cand_indices,
                       const CandidateScoreEnsemble &thres_lb, const CandidateScoreEnsemble &thres_ub,
                       std::vector<std::shared_ptr<const ContourManager>> &res_cand, std::vector<double> &res_corr,
                       std::vector<Eigen::Isometry2d> &res_T, int max_ret) const {
    return verifyFrom(q_ptr.get(), 0, cand_indices, thres_lb, thres_ub, res_cand, res_corr, res_T, max_ret);
  }
  // q: the query scan by its host descriptor, or nullptr: the stored scan `idx`
  int verifyFrom(const ContourManager *q, int idx, const std::vector<int> &cand_indices, const CandidateScoreEnsemble &thres_lb,
                 const CandidateScoreEnsemble &thres_ub, std::vector<std::shared_ptr<const ContourManager>> &res_cand,
                 std::vector<double> &res_corr, std::vector<Eigen::Isometry2d> &res_T, int max_ret) const {
    CC_CHECK(max_ret >= 1 && max_ret <= CC_RANK_MAX);
    res_cand.clear();
    res_corr.clear();
    res_T.clear();
    CC_CHECK((int)cand_indices.size() <= CC_VERIFY_CANDS_MAX);
    for (const int c : cand_indices) CC_CHECK(c >= 0 && c < (int)all_bevs_.size());  // (scans appended ahead of the driver are not the caller's yet)
    if (cand_indices.empty()) return 0;
    if (q) ensure(*q);
    if (need_rebuild_) rebuild();
    const cc_score_t lb = to_c(thres_lb), ub = to_c(thres_ub);
    int32_t cands[CC_VERIFY_CANDS_MAX];
    for (int k = 0; k < CC_VERIFY_CANDS_MAX; k++) cands[k] = k < (int)cand_indices.size() ? cand_indices[k] : -1;
    cc_verify_cfg_t vc;
    vc.level_mask = 0;
    vc.max_fine_opt = cfg_.max_fine_opt_;
    vc.max_key_dist_sq = 1000.0f;
    vc.pad_ = 0;
    cc_query_result_t r;
    cc_ranked_cand_t rl[CC_RANK_MAX];
    int32_t rn = 0;
    cc_ranked_detail_t dl[CC_RANK_MAX];
    const cc_rank_out_t ro = {rl, &rn, max_ret, 0};
    last_details_.clear();
    last_matches_.clear();
    cc_ranked_match_t ml[CC_RANK_MAX];
    const cc_match_out_t mo = {ml, want_matches_};
    const bool wm = wantMatches(), rk = max_ret > 1 || want_detail_ || wm;
    int rc;
    if (q) {
      rc = wm           ? cc_db_verify_batch_host_matched(db_, &q->desc(), 1, nullptr, cands, 1, &vc, &lb, &ub, &r, &ro, want_detail_ ? dl : nullptr, &mo)
           : want_detail_ ? cc_db_verify_batch_host_ranked_detail(db_, &q->desc(), 1, nullptr, cands, 1, &vc, &lb, &ub, &r, &ro, dl)
           : max_ret > 1 ? cc_db_verify_batch_host_ranked(db_, &q->desc(), 1, nullptr, cands, 1, &vc, &lb, &ub, &r, &ro)
                         : cc_db_verify_batch_host(db_, &q->desc(), 1, nullptr, cands, 1, &vc, &lb, &ub, &r);
    } else {
      const cc_packed_src_t own = {nullptr, nullptr, 0, 0};
      const int32_t rec = idx;
      rc = wm ? cc_db_verify_submit_matched(db_, nullptr, 0, &own, &rec, cands, 1, &vc, &lb, &ub, &r, nullptr, nullptr, nullptr, &ro, want_detail_ ? dl : nullptr, &mo)
              : cc_db_verify_submit_packed(db_, &own, &rec, cands, 1, &vc, &lb, &ub, &r, nullptr, nullptr, nullptr, rk ? &ro : nullptr, want_detail_ ? dl : nullptr);
      const int r2 = cc_db_query_wait(db_);
      if (rc == CC_OK) rc = r2;
    }
    for (auto &sp : spec_) sp.collected = true;  // the synchronous call (the wait) collected every chain in flight
    if (rc != CC_OK) die_cc();
    return handOut(rk, r, rl, rn, dl, ml, res_cand, res_corr, res_T);
  }
  // Mirror-only as a database call: ConstellCorrelation's public interface (correlation.h:175-238) on scans of this database,
  // in one device pass (cc_db_pose_batch_host).  Per query: the candidate by its index in adding order (as verifyCandidates
  // takes it), the relative pose the caller believes in, and further poses to probe over the pair set of T_init.
  //   corr_init = initProblem(cand, cm_tgt, T_init);  try_corr[t] = tryProblem(T_try[t]);  correlation, T_best = calcCorrelation()
  // on the queries with pairs whose corr_init is not below min_corr (refine; else corr_init and T_init, flags without CC_PF_REFINED);
  // hess / grad: the curvature of -correlation at T_best (cc_pose_curv_t).  Every query carries as many T_try as the longest
  // list of the call needs the device to evaluate (at most CC_POSE_TRY_MAX); shorter lists are padded with T_init.
  struct PoseQuery {
    int cand = 0;
    Eigen::Isometry2d T_init = Eigen::Isometry2d::Identity();
    std::vector<Eigen::Isometry2d> T_try;
  };
  struct PoseScore {
    double corr_init = 0, correlation = 0;
    Eigen::Isometry2d T_best = Eigen::Isometry2d::Identity();
    int n_pairs = 0, iterations = 0, termination = 0, flags = 0;
    std::vector<double> try_corr;
    double hess[6] = {0, 0, 0, 0, 0, 0}, grad[3] = {0, 0, 0};
  };
  std::vector<PoseScore> scorePoses(const std::shared_ptr<const ContourManager> &cm_tgt, const std::vector<PoseQuery> &queries,
                                    bool refine = true, float min_corr = 0.3f) const {
    return scorePosesFrom(cm_tgt.get(), 0, queries, refine, min_corr);
  }
  // scorePoses for a scan this database holds (tgt), by its index in adding order, from the records the database keeps
  // (cc_db_pose_submit_packed); a query's candidate may be that scan itself.
  std::vector<PoseScore> scorePosesStored(int idx, const std::vector<PoseQuery> &queries, bool refine = true, float min_corr = 0.3f) const {
    CC_CHECK(db_ && idx >= 0 && idx < (int)all_bevs_.size());
    return scorePosesFrom(nullptr, idx, queries, refine, min_corr);
  }
  // tgt: the query scan by its host descriptor, or nullptr: the stored scan `idx`
  std::vector<PoseScore> scorePosesFrom(const ContourManager *tgt, int idx, const std::vector<PoseQuery> &queries, bool refine, float min_corr) const {
    std::vector<PoseScore> out(queries.size());
    if (queries.empty()) return out;
    size_t nt = 0;
    for (const auto &pq : queries) {
      CC_CHECK(pq.cand >= 0 && pq.cand < (int)all_bevs_.size());  // (scans appended ahead of the driver are not the caller's yet)
      CC_CHECK(pq.T_try.size() <= (size_t)CC_POSE_TRY_MAX);
      nt = std::max(nt, pq.T_try.size());
    }
    if (tgt) ensure(*tgt);
    if (need_rebuild_) rebuild();
    const auto tf_of = [](const Eigen::Isometry2d &T, double *o) {
      o[0] = T(0, 2);
      o[1] = T(1, 2);
      o[2] = std::atan2(T(1, 0), T(0, 0));
    };
    const int n = (int)queries.size();
    std::vector<cc_pose_item_t> items(n);
    std::vector<double> tries((size_t)n * nt * 3), tc((size_t)n * nt);
    for (int i = 0; i < n; i++) {
      items[i].q = tgt ? 0 : idx;
      items[i].gidx = queries[i].cand;
      tf_of(queries[i].T_init, items[i].tf);
      for (size_t t = 0; t < nt; t++) tf_of(t < queries[i].T_try.size() ? queries[i].T_try[t] : queries[i].T_init, &tries[((size_t)i * nt + t) * 3]);
    }
    cc_pose_cfg_t pc;
    pc.refine = refine ? 1 : 0;
    pc.min_corr = min_corr;
    pc.n_try = (int)nt;
    pc.pad_ = 0;
    std::vector<cc_pose_result_t> res(n);
    std::vector<cc_pose_curv_t> cv(n);
    int rc;
    if (tgt) {
      rc = cc_db_pose_batch_host(db_, &tgt->desc(), 1, items.data(), n, &pc, nt ? tries.data() : nullptr, res.data(), nt ? tc.data() : nullptr, cv.data());
    } else {
      const cc_packed_src_t own = {nullptr, nullptr, 0, 0};
      rc = cc_db_pose_submit_packed(db_, &own, items.data(), n, &pc, nt ? tries.data() : nullptr, res.data(), nt ? tc.data() : nullptr, cv.data(), nullptr);
      const int r2 = cc_db_query_wait(db_);
      if (rc == CC_OK) rc = r2;
    }
    for (auto &sp : spec_) sp.collected = true;  // the synchronous call (the wait) collected every chain in flight
    if (rc != CC_OK) die_cc();
    for (int i = 0; i < n; i++) {
      PoseScore &o = out[i];
      o.corr_init = res[i].corr_init;
      o.correlation = res[i].correlation;
      o.T_best.rotate(res[i].tf[2]);
      o.T_best.pretranslate(res[i].tf[0], res[i].tf[1]);
      o.n_pairs = res[i].n_pairs;
      o.iterations = res[i].iterations;
      o.termination = res[i].termination;
      o.flags = res[i].flags;
      o.try_corr.assign(tc.begin() + (size_t)i * nt, tc.begin() + (size_t)i * nt + queries[i].T_try.size());
      std::copy(cv[i].hess, cv[i].hess + 6, o.hess);
      std::copy(cv[i].grad, cv[i].grad + 3, o.grad);
    }
    return out;
  }
  // contour_db.h:814 and :827
  void addScan(const std::shared_ptr<ContourManager> &added, double curr_timestamp) {
    ensure(*added);
    pending_ = added;
    pending_ts_ = curr_timestamp;
  }
  void pushAndBalance(int seed, double curr_timestamp) {
    // the C-ABI couples addScan + pushAndBalance (they are always called back to back, batch_bin_test.cpp:234-237)
    CC_CHECK(pending_);
    (void)curr_timestamp;
    if (need_rebuild_) rebuild();
    cc_scan *h = pending_->scanHandle();
    if (!spec_.empty() && h && spec_.front().scan == h && spec_.front().ts == pending_ts_ && spec_.front().seed == seed) {
      // appended ahead of time, with exactly these arguments.  (Its own query has been handed out, or is no longer wanted:
      // its answer buffer must outlive the chain that writes it.)
      collectOne(0);
      spec_.pop_front();
    } else {
      if (!spec_.empty()) rebuild();  // the driver left the predicted sequence: back to the scans it really added
      ensure(*pending_);
      const int rc = h && cc_scan_on_device(h) ? cc_db_add_scan(db_, h, pending_ts_, seed) : cc_db_add_scan_host(db_, &pending_->desc(), pending_ts_, seed);
      if (rc != CC_OK) die_cc();
    }
    all_ts_.push_back(pending_ts_);
    all_seed_.push_back(seed);
    // The DB keeps its own compact records of the scan.  The full descriptor (169 KB) stays in its device slot for now: its
    // host copy is fetched when a getter first asks for it, and moving every scan to the host right here cost the loop a
    // 169 KB copy + a stream synchronisation per scan.  Only the most recent residentScans() descriptors stay (1.4 GB at
    // the default 8 192 -- a KITTI sequence fits); beyond that the oldest one moves to the host and its slot is reused.
    if (h) on_device_.push_back(pending_);
    while (on_device_.size() > residentScans()) {
      cc_scan *old = on_device_.front()->scanHandle();
      if (old && cc_scan_offload(old) != CC_OK) {
        fprintf(stderr, "cont2_amd: %s\n", cc_last_error());
        abort();
      }
      on_device_.pop_front();
    }
    all_bevs_.push_back(pending_);
    source_ = pending_->scanSource();
    pending_.reset();
    readAhead();
  }
  // how many added scans keep their full descriptor on the device (env CC_SCANS_ON_DEVICE; 0: none, as before round 4)
  static size_t residentScans() {
    static const size_t n = [] {
      const char *e = getenv("CC_SCANS_ON_DEVICE");
      return e ? (size_t)std::max(0L, atol(e)) : (size_t)8192;
    }();
    return n;
  }

 private:
  std::shared_ptr<ContourManager> pending_;
  double pending_ts_ = 0;
  std::deque<std::shared_ptr<ContourManager>> on_device_;  // added scans whose descriptor still sits in a device slot, oldest first
};

// contour_db.h:264-656, the hint-driven use of CandidateManager (the single-pair flow of test/kitti_read_bin_test.cpp:226-291):
//   CandidateManager m(cm_query, lb, ub);  m.checkCandWithHint(cm_cand, {level, seq_src, seq_tgt}, cont_sim); ...
//   m.tidyUpCandidates();  m.fineOptimize(max_fine_opt, cands, corr, tfs);
// All three stages run on the device (cc_db_check_hints): checkCandWithHint evaluates its hint at once for the returned
// scores and records it; fineOptimize replays the recorded hints in call order through checks, proposal merge, tidy-up
// and refinement.  Candidate scans live in a process-wide device store (one per cont_sim setting).  Hint levels: 1..4.
class CandidateManager {
  // Candidate scans live in a device store shared by the managers of one (grid, cont_sim) setting.  It is a cache: when it
  // is full it is emptied and refilled with what the manager at hand needs, so no number of distinct candidates exhausts it.
  struct Store {
    cc_db *db = nullptr;
    cc_db_cfg_t cfg;
    cc_ctx *ctx = nullptr;
    int cap = 1024;
    std::map<const ContourManager *, int> pos;
    std::vector<std::shared_ptr<const ContourManager>> keep;  // position -> scan (kept alive while it is in the store)
    void reset() {
      cc_db_destroy(db);
      db = nullptr;
      pos.clear();
      keep.clear();
      if (cc_db_create(ctx, &cfg, cap, &db) != CC_OK) die();
      if (CC_MIRROR_DYNAMIC_THRES && cc_db_set_dynamic_thres(db, 1) != CC_OK) die();
    }
    bool has(const ContourManager *p) const { return pos.count(p) != 0; }
    int add(const std::shared_ptr<const ContourManager> &cm) {
      const int g = cc_db_size(db);
      if (cc_db_add_scan_host(db, &cm->desc(), (double)g, g) != CC_OK) die();
      pos[cm.get()] = g;
      keep.push_back(cm);
      return g;
    }
  };
  static Store &store(const ContourManager &cm, const ContourSimThresConfig &cs) {
    static std::map<std::string, Store> pool;
    std::string key((const char *)&cm.ccfg(), sizeof(cc_manager_cfg_t));
    key.append((const char *)&cs, sizeof(cs));
    Store &st = pool[key];
    if (!st.db) {
      cc_default_db_cfg(&st.cfg);
      st.cfg.cont_sim.ta_cell_cnt = cs.ta_cell_cnt;
      st.cfg.cont_sim.tp_cell_cnt = cs.tp_cell_cnt;
      st.cfg.cont_sim.tp_eigval = cs.tp_eigval;
      st.cfg.cont_sim.ta_h_bar = cs.ta_h_bar;
      st.cfg.cont_sim.ta_rcom = cs.ta_rcom;
      st.cfg.cont_sim.tp_rcom = cs.tp_rcom;
      st.ctx = cc_host::context(cm.ccfg());
      if (const char *e = getenv("CC_CAND_STORE_CAP")) st.cap = atoi(e) > 0 ? atoi(e) : st.cap;
      if (cc_db_create(st.ctx, &st.cfg, st.cap, &st.db) != CC_OK) die();
      if (CC_MIRROR_DYNAMIC_THRES && cc_db_set_dynamic_thres(st.db, 1) != CC_OK) die();
    }
    return st;
  }
  // every candidate of THIS manager present in the store (positions may change when the store is recycled)
  void ensureMine() {
    Store &st = *st_;
    bool all = true;
    for (const auto &c : my_cands_) all = all && st.has(c.get());
    if (all) return;
    int missing = 0;
    for (const auto &c : my_cands_) missing += st.has(c.get()) ? 0 : 1;
    CC_CHECK((int)my_cands_.size() <= st.cap);  // one manager's candidates must fit (the reference has no bound; raise CC_CAND_STORE_CAP)
    if (cc_db_size(st.db) + missing > st.cap) st.reset();
    for (const auto &c : my_cands_)
      if (!st.has(c.get())) st.add(c);
  }
  static void die() {
    fprintf(stderr, "cont2_amd: %s\n", cc_last_error());
    abort();
  }
  static cc_score_t to_c(const CandidateScoreEnsemble &e) {
    cc_score_t s;
    s.i_ovlp_sum = e.sim_constell.i_ovlp_sum;
    s.i_ovlp_max_one = e.sim_constell.i_ovlp_max_one;
    s.i_in_ang_rng = e.sim_constell.i_in_ang_rng;
    s.i_indiv_sim = e.sim_pair.i_indiv_sim;
    s.i_orie_sim = e.sim_pair.i_orie_sim;
    s.correlation = e.sim_post.correlation;
    s.area_perc = e.sim_post.area_perc;
    s.neg_est_dist = e.sim_post.neg_est_dist;
    return s;
  }

  std::shared_ptr<const ContourManager> cm_tgt_;
  const CandidateScoreEnsemble sim_lb_, sim_ub_;  // the device always gets the initial bars (raised ones may reach ub)
  CandidateScoreEnsemble sim_var_;                 // the bars as they stand after the hints so far (DYNAMIC_THRES=1)
  Store *st_ = nullptr;
  std::vector<cc_hint_t> hints_;                                // cand_gidx = index into my_cands_ until the call is made
  bool want_detail_ = false;                      // setWantDetail
  std::vector<cc_ranked_detail_t> last_details_;  // lastDetails()
  double want_matches_ = -1.0;                    // setWantMatches (< 0: off)
  std::vector<cc_ranked_match_t> last_matches_;   // lastMatches()
  std::vector<std::shared_ptr<const ContourManager>> my_cands_;  // this manager's candidate scans, first-appearance order
  std::map<int, int> id2local_;                                 // the reference keys candidates_ by getIntID() (contour_db.h:468-476)
  int flow_valve = 0;

 public:
  int cand_aft_check1 = 0, cand_aft_check2 = 0, cand_aft_check3 = 0;

  CandidateManager(std::shared_ptr<const ContourManager> cm_q, const CandidateScoreEnsemble sim_lb, const CandidateScoreEnsemble sim_ub)
      : cm_tgt_(std::move(cm_q)), sim_lb_(sim_lb), sim_ub_(sim_ub), sim_var_(sim_lb) {
    CC_CHECK(sim_lb.sim_constell.strictSmaller(sim_ub.sim_constell));
    CC_CHECK(sim_lb.sim_pair.strictSmaller(sim_ub.sim_pair));
    CC_CHECK(sim_lb.sim_post.strictSmaller(sim_ub.sim_post));
  }

  // contour_db.h:374-488
  CandidateScoreEnsemble checkCandWithHint(const std::shared_ptr<const ContourManager> &cm_cand, const ConstellationPair &anchor_pair,
                                           const ContourSimThresConfig &cont_sim = ContourSimThresConfig()) {
    CC_CHECK(flow_valve == 0);
    Store &st = store(*cm_tgt_, cont_sim);
    CC_CHECK(st_ == nullptr || st_ == &st);  // one cont_sim setting per manager
    st_ = &st;
    auto it = id2local_.find(cm_cand->getIntID());
    if (it == id2local_.end()) {
      it = id2local_.insert({cm_cand->getIntID(), (int)my_cands_.size()}).first;
      my_cands_.push_back(cm_cand);
    }
    ensureMine();
    cc_hint_t h;
    h.cand_gidx = st.pos[my_cands_[it->second].get()];
    h.level = anchor_pair.level;
    h.seq_src = anchor_pair.seq_src;
    h.seq_tgt = anchor_pair.seq_tgt;
    h.pad = 0;
    const cc_score_t lb = to_c(sim_lb_), ub = to_c(sim_ub_);
    cc_query_result_t r;
    cc_hint_score_t sc;
    if (cc_db_check_hints_host(st.db, &cm_tgt_->desc(), &h, 1, &lb, &ub, 1, &r, &sc) != CC_OK) die();
    h.cand_gidx = it->second;  // recorded by the manager's own numbering
    hints_.push_back(h);
    cand_aft_check1 += r.cand_aft_check1;
#if CC_MIRROR_DYNAMIC_THRES
    {  // the full scores under the initial bars decide the hint under the current ones (the gates are monotone in the
       // bars, contour_mng.h:307, 361-363, 1168, 1203); what the gates return under a raised bar is partial
      const CandidateScoreEnsemble &B = sim_var_;
      const bool pc = sc.i_ovlp_sum >= B.sim_constell.i_ovlp_sum && sc.i_ovlp_max_one >= B.sim_constell.i_ovlp_max_one;
      const bool st2 = r.cand_aft_check2 > 0 && pc && sc.i_in_ang_rng >= B.sim_constell.i_in_ang_rng;
      const bool st3 = st2 && r.cand_aft_check3 > 0 && sc.i_indiv_sim >= B.sim_pair.i_indiv_sim && sc.i_orie_sim >= B.sim_pair.i_orie_sim;
      if (!pc) sc.i_in_ang_rng = 0;
      if (!(pc && sc.i_in_ang_rng >= B.sim_constell.i_in_ang_rng)) sc.i_indiv_sim = sc.i_orie_sim = 0;
      else if (sc.i_indiv_sim < B.sim_pair.i_indiv_sim) sc.i_orie_sim = 0;
      cand_aft_check2 += st2 ? 1 : 0;
      cand_aft_check3 += st3 ? 1 : 0;
      if (st3) {  // contour_db.h:439-457
        const int cnt = sc.i_orie_sim;
        auto raise = [cnt](int &var, int ub) {
          var = var < cnt ? cnt : var;
          var = var > ub ? ub : var;
        };
        raise(sim_var_.sim_constell.i_ovlp_sum, sim_ub_.sim_constell.i_ovlp_sum);
        raise(sim_var_.sim_constell.i_ovlp_max_one, sim_ub_.sim_constell.i_ovlp_max_one);
        raise(sim_var_.sim_constell.i_in_ang_rng, sim_ub_.sim_constell.i_in_ang_rng);
        raise(sim_var_.sim_pair.i_indiv_sim, sim_ub_.sim_pair.i_indiv_sim);
        raise(sim_var_.sim_pair.i_orie_sim, sim_ub_.sim_pair.i_orie_sim);
      }
    }
#else
    cand_aft_check2 += r.cand_aft_check2;
    cand_aft_check3 += r.cand_aft_check3;
#endif
    CandidateScoreEnsemble ret;
    ret.sim_constell.i_ovlp_sum = sc.i_ovlp_sum;
    ret.sim_constell.i_ovlp_max_one = sc.i_ovlp_max_one;
    ret.sim_constell.i_in_ang_rng = sc.i_in_ang_rng;
    ret.sim_pair.i_indiv_sim = sc.i_indiv_sim;
    ret.sim_pair.i_orie_sim = sc.i_orie_sim;
    return ret;
  }

  // contour_db.h:494-596.  The work happens in fineOptimize (one device pass over the recorded hints).
  void tidyUpCandidates() {
    CC_CHECK(flow_valve < 1);
    flow_valve++;
  }

  // Mirror-only: fineOptimize collects the detail rows of the candidates it returns (ContourDB::setWantDetail's counterpart for the
  // hint flow); lastDetails() after fineOptimize, one row per returned candidate.  Off (the default): the calls made before.
  void setWantDetail(bool on) { want_detail_ = on; }
  const std::vector<cc_ranked_detail_t> &lastDetails() const { return last_details_; }
  // Mirror-only: ... and their match rows (ContourDB::setWantMatches' counterpart: the constellation this manager merged for each
  // returned candidate -- anch_props_[0].constell_ -- with its residuals at the refined pose); negative: off, the default.
  void setWantMatches(double inlier_px) { want_matches_ = inlier_px >= 0.0 ? inlier_px : -1.0; }
  const std::vector<cc_ranked_match_t> &lastMatches() const { return last_matches_; }

  // contour_db.h:604-648: returns the number of results (0 or 1; with max_ret > 1 -- mirror-only, the reference's ret_size is
  // hard-wired to 1 -- up to min(max_ret, max_fine_opt) refined candidates, best first)
  int fineOptimize(int max_fine_opt, std::vector<std::shared_ptr<const ContourManager>> &res_cand, std::vector<double> &res_corr,
                   std::vector<Eigen::Isometry2d> &res_T, int max_ret = 1) {
    CC_CHECK(max_ret >= 1 && max_ret <= CC_RANK_MAX);
    CC_CHECK(flow_valve == 1);
    flow_valve++;
    res_cand.clear();
    res_corr.clear();
    res_T.clear();
    if (hints_.empty() || !st_) return 0;
    const cc_score_t lb = to_c(sim_lb_), ub = to_c(sim_ub_);  // (dynamic mode: the device replays the rising bars itself)
    cc_query_result_t r;
    ensureMine();
    std::vector<cc_hint_t> hs(hints_);
    for (auto &h : hs) h.cand_gidx = st_->pos[my_cands_[h.cand_gidx].get()];
    last_details_.clear();
    last_matches_.clear();
    const bool wm = want_matches_ >= 0.0;
    if (max_ret > 1 || want_detail_ || wm) {
      cc_ranked_cand_t rl[CC_RANK_MAX];
      cc_ranked_detail_t dl[CC_RANK_MAX];
      cc_ranked_match_t ml[CC_RANK_MAX];
      int32_t rn = 0;
      const cc_rank_out_t ro = {rl, &rn, max_ret, 0};
      const cc_match_out_t mo = {ml, want_matches_};
      const int rc = wm ? cc_db_check_hints_host_matched(st_->db, &cm_tgt_->desc(), hs.data(), (int)hs.size(), &lb, &ub, max_fine_opt, &r, nullptr, &ro,
                                                         want_detail_ ? dl : nullptr, &mo)
                     : want_detail_ ? cc_db_check_hints_host_ranked_detail(st_->db, &cm_tgt_->desc(), hs.data(), (int)hs.size(), &lb, &ub, max_fine_opt,
                                                                         &r, nullptr, &ro, dl)
                                  : cc_db_check_hints_host_ranked(st_->db, &cm_tgt_->desc(), hs.data(), (int)hs.size(), &lb, &ub, max_fine_opt, &r,
                                                                  nullptr, &ro);
      if (rc != CC_OK) die();
      for (int k = 0; k < rn; k++) ContourDB::pushRanked(st_->keep, rl[k], res_cand, res_corr, res_T);
      if (want_detail_) last_details_.assign(dl, dl + rn);
      if (wm) last_matches_.assign(ml, ml + rn);
      return rn;
    }
    if (cc_db_check_hints_host(st_->db, &cm_tgt_->desc(), hs.data(), (int)hs.size(), &lb, &ub, max_fine_opt, &r, nullptr) != CC_OK)
      die();
    if (r.n_res > 0) {
      res_cand.push_back(st_->keep[r.cand_gidx]);
      res_corr.push_back(r.correlation);
      Eigen::Isometry2d T;
      T.rotate(r.tf[2]);
      T.pretranslate(r.tf[0], r.tf[1]);
      res_T.push_back(T);
    }
    return r.n_res;
  }
};

// correlation.h:287-296
struct ConstellCorrelation {
  static Eigen::Isometry2d getEstSensTF(const Eigen::Isometry2d &T_delta, const ContourManagerConfig &bev_config) {
    CC_CHECK(bev_config.reso_row_ == bev_config.reso_col_);
    const double in[3] = {T_delta(0, 2), T_delta(1, 2), std::atan2(T_delta(1, 0), T_delta(0, 0))};
    double out[3];
    cc_est_sens_tf(in, bev_config.n_row_, bev_config.n_col_, out);
    Eigen::Isometry2d T;
    T.rotate(out[2]);
    T.pretranslate(out[0], out[1]);
    return T;
  }

  // correlation.h:241-280: error of the estimated sensor-to-sensor transform (metres, radians) against the 3-D ground
  // truth projected to 2-D (xy offset; yaw after rotating the relative z axis back onto z).  Returns T_gt^-1 * T_est.
  static Eigen::Isometry2d evalMetricEst(const Eigen::Isometry2d &T_delta, const Eigen::Isometry3d &gt_src_3d,
                                         const Eigen::Isometry3d &gt_tgt_3d, const ContourManagerConfig &bev_config) {
    CC_CHECK(bev_config.reso_row_ == bev_config.reso_col_);
    Eigen::Isometry2d T_est = getEstSensTF(T_delta, bev_config);
    T_est.m[0][2] *= bev_config.reso_row_;
    T_est.m[1][2] *= bev_config.reso_row_;
    const Eigen::Isometry3d rel = gt_tgt_3d.inverse() * gt_src_3d;  // src sensor in the tgt sensor frame
    // axis-angle that takes the relative z axis back to (0,0,1): axis = z0 x z1 normalised, angle = -acos(z0 . z1)
    const double z1[3] = {rel.R[0][2], rel.R[1][2], rel.R[2][2]};
    double ax[3] = {-z1[1], z1[0], 0.0};
    const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1]);
    if (an > 0) {
      ax[0] /= an;
      ax[1] /= an;
    }
    const double ang = -std::acos(z1[2]);
    const double c = std::cos(ang), s = std::sin(ang), C = 1 - c;
    const double D[3][3] = {{c + ax[0] * ax[0] * C, ax[0] * ax[1] * C - ax[2] * s, ax[0] * ax[2] * C + ax[1] * s},
                            {ax[1] * ax[0] * C + ax[2] * s, c + ax[1] * ax[1] * C, ax[1] * ax[2] * C - ax[0] * s},
                            {ax[2] * ax[0] * C - ax[1] * s, ax[2] * ax[1] * C + ax[0] * s, c + ax[2] * ax[2] * C}};
    double Rr[2][2];  // top-left 2x2 of D * rel.R
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 2; j++) Rr[i][j] = D[i][0] * rel.R[0][j] + D[i][1] * rel.R[1][j] + D[i][2] * rel.R[2][j];
    Eigen::Isometry2d T_gt;
    T_gt.rotate(std::atan2(Rr[1][0], Rr[0][0]));
    T_gt.pretranslate(rel.t[0], rel.t[1]);
    return T_gt.inverse() * T_est;
  }
};
