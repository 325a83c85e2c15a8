// cc_db_* entry points: device-resident database + batched query (included by cont2_amd.hip inside
// extern "C").  Host side of ContourDB (contour_db.h:264-845): what stays on the host is the LayerDB bucket
// bookkeeping per added scan (cc_hostdb.h: buffers, rebalancing, the epoch at which a key becomes searchable) and
// the launch sequencing; a query batch is a chain of launches (k_knn.h, k_check.h, k_merge.h, k_gmm.h) per chunk and
// one small result copy.
//
// What the DB keeps per scan in HBM: the 18 KB hot record (cc_hot_desc_t: keys, top contours and BCIs of levels 1..4)
// and the 41 KB correlation inputs (cc_gmm_feat) -- 59 KB instead of the 169 KB full descriptor, so a 5 000-scan DB
// takes 297 MB (a little more than the 256 MB Infinity Cache; what a check touches is the 18 KB hot record: 92 MB) and a
// 50 000-scan DB 2.97 GB.  The same two records are the wire
// format of the multi-GPU exchange (cc_pack_scans -> all-gather -> cc_db_add_packed).

namespace {

// Transfers of a few hundred bytes are not worth a copy command in a launch chain (a blit kernel + its dispatch gap, ~10 us
// each on the per-scan loop): up to this many scans / queries the kernels read and write pinned host memory directly.
#define CC_ZC_MAX 64
#define CC_LIST_ZC_ENT 256  // ... and up to this many staged entries of a listed chunk (4 KB) the list retrieval reads where they lie
#define CC_NVIEW 4     // buffers of a layer's sorted view: an append writes the next one, which the chunks submitted CC_NVIEW - 1 appends ago
                       // were the last to read -- with two (rounds 2-4) every append waited for the queries queued just before the previous one
#define CC_NSTAGE 4    // pinned staging buffers of the small appends (the per-scan loop): an append does not wait for the one before it
// compact per-scan record pulled to the host (cc_k_extract)
struct ScanLite {
  float keys[CC_NQLEV][CC_NPIV][CC_KEY_DIM];
  int n_cont[CC_HOT_LEVELS];
  int flags;  // CC_DESC_* of the scan's descriptor
};

}  // namespace

#define CC_N_HEADS 24  // a query lane's list heads (cc_qlane::d_heads): one allocation, so that one kernel (cc_k_pack_hot) clears all
enum cc_head_slot {    // what the chain's kernels count in them (cc_qlane::head)
  CC_HD_NPROB = 0,     // correlation problems of the chunk
  CC_HD_NSEL16 = 1,    // ... of which the 16-lane refinement instance takes this many
  CC_HD_NSEL64 = 2,    // ... and the 64-lane instance this many
  CC_HD_POOL = 3,      // head of the pair pool (d_pool)
  CC_HD_CNT = 4,       // [4] list heads of the checks (CC_CNT_*)
  CC_HD_NMID = 8,      // length of the in-between refinement list
  CC_HD_CODES = 9,     // head of the pair-code pool (d_codes)
  CC_HD_CLS = 12,      // [CC_GMM_NCLS] the long refinement problems by length class
};
static_assert(CC_HD_CLS + CC_GMM_NCLS <= CC_N_HEADS, "the class counts are the last slots of a lane's list heads");
enum cc_sel_list {  // the sub-lists of cc_qlane::d_sel, prob_cap entries each (cc_qlane::sel)
  CC_SEL_16 = 0,    // problems of the 16-lane refinement instance
  CC_SEL_64 = 1,    // (unused: the long problems are listed by class)
  CC_SEL_MID = 2,   // the in-between list, shared by both instances
  CC_SEL_CLS = 3,   // [CC_GMM_NCLS] problems of the 64-lane instance by length class
};
// full descriptor -> hot record.  grid = n scans, block = 256
__global__ void __launch_bounds__(256)
cc_k_pack_hot(const cc_scan_desc_t *__restrict__ desc, int n, cc_hot_desc_t *__restrict__ hot,
              int *__restrict__ z_heads /*[CC_N_HEADS] or nullptr*/, int *__restrict__ z_pass_cnt /*[n][4] or nullptr*/,
              const cc_query_meta *__restrict__ meta_src /*small query chunks: the epoch records in pinned host memory, or nullptr*/,
              cc_query_meta *__restrict__ meta_dst, const int *__restrict__ sel /*[n] record i comes from desc[sel[i]] (verify chunks), or nullptr: from desc[i]*/) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const cc_scan_desc_t *d = desc + (sel ? sel[i] : i);
  cc_hot_desc_t *o = hot + i;
  const int tid = threadIdx.x, nt = blockDim.x;
  // small query chunks: the query's epoch record comes over with this kernel instead of a copy command in front of the chain
  if (meta_src && tid >= 64 && tid < 64 + (int)(sizeof(cc_query_meta) / 4)) ((int *)(meta_dst + i))[tid - 64] = ((const int *)(meta_src + i))[tid - 64];
  // query chunks: the chunk's list heads and per-query counters are cleared here instead of by three memsets in front
  if (z_pass_cnt && tid < 4) z_pass_cnt[i * 4 + tid] = 0;
  if (z_heads && i == 0 && tid < CC_N_HEADS) z_heads[tid] = 0;
  if (tid < CC_HOT_LEVELS) {
    o->n_cont[tid] = d->n_cont[tid + 1];
    o->layer_cell_cnt[tid] = d->layer_cell_cnt[tid + 1];
  }
  if (tid == 0) {
    o->flags = d->flags;
    o->pad_[0] = o->pad_[1] = o->pad_[2] = 0;
  }
  for (int t = tid; t < CC_HOT_LEVELS * CC_NPIV * CC_KEY_DIM; t += nt)
    (&o->keys[0][0][0])[t] = (&d->keys[1][0][0])[t];
  const int CW = (int)(sizeof(cc_contour_t) / 4);
  for (int t = tid; t < CC_HOT_LEVELS * CC_NDIST * CW; t += nt) {
    const int l = t / (CC_NDIST * CW), r = (t - l * CC_NDIST * CW) / CW, w = t - (l * CC_NDIST + r) * CW;
    ((unsigned *)&o->cont[l][r])[w] = r < d->n_stored[l + 1] ? ((const unsigned *)&d->cont[l + 1][r])[w] : 0u;
  }
  const int BW = (int)(sizeof(cc_bci_t) / 4);
  for (int t = tid; t < CC_HOT_LEVELS * CC_NPIV * BW; t += nt) ((unsigned *)&o->bcis[0][0])[t] = ((const unsigned *)&d->bcis[1][0])[t];
}

__global__ void cc_k_extract(const cc_hot_desc_t *__restrict__ hot, int n, int n_q_levels, int q0, int q1, int q2,
                             ScanLite *__restrict__ out) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const cc_hot_desc_t *d = hot + i;
  ScanLite *o = out + i;
  const int ql[3] = {q0, q1, q2};
  for (int t = threadIdx.x; t < CC_NQLEV * CC_NPIV * CC_KEY_DIM; t += blockDim.x) {
    const int ll = t / (CC_NPIV * CC_KEY_DIM), r = t % (CC_NPIV * CC_KEY_DIM);
    o->keys[ll][r / CC_KEY_DIM][r % CC_KEY_DIM] = (ll < n_q_levels) ? d->keys[ql[ll] - 1][r / CC_KEY_DIM][r % CC_KEY_DIM] : 0.f;
  }
  for (int t = threadIdx.x; t < CC_HOT_LEVELS; t += blockDim.x) o->n_cont[t] = d->n_cont[t];
  if (threadIdx.x == 0) o->flags = d->flags;
}

struct cc_qlane {  // scratch of one in-flight chunk of <= QB queries
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  hipEvent_t pev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // boundaries of K3 | K4 | merge | K5 | final
  hipEvent_t prep = nullptr;          // the chunk's query descriptors have been read (recorded after the prep kernels)
  hipEvent_t fin = nullptr;           // the chunk's chain has finished (device-side guard of the sorted-view buffers)
  int view[CC_NQLEV] = {0, 0, 0};     // which buffer of each layer's sorted view the chunk in flight reads
  bool busy = false, profiled = false;
  int b0 = 0, nb = 0;  // the chunk in flight
  cc_query_result_t *h_dst = nullptr;  // where the chunk's results go when it is collected
  cc_query_meta *d_qmeta = nullptr;
  cc_hot_desc_t *d_qhot = nullptr;    // [QB] hot records of the chunk's query scans
  cc_gmm_feat *d_qfeat = nullptr;     // [QB] their correlation inputs
  cc_knn_hit_t *d_hits = nullptr;
  int *d_hit_cnt = nullptr;
  int *d_knn_order = nullptr;         // [CC_NQLEV][CC_KNN_ORDER_CAP] + [CC_NQLEV]: searches by key[0] (shared-walk / tiled K3)
  cc_chk_item *d_items = nullptr;     // [QB * CC_CHK_STRIDE] checks that passed stage A
  int *d_redo = nullptr;              // [QB * CC_CHK_STRIDE] indices of the checks left to the large B1 instance
  cc_cstl_item *d_cstl = nullptr;     // [QB * CC_CHK_STRIDE] constellation record of check i (n_in = 0: did not pass the window test)
  int *d_cstl_idx = nullptr;          // [QB * CC_CHK_STRIDE] dense list of the records that did
  int *d_heads = nullptr;             // [CC_N_HEADS] the chunk's list heads, by cc_head_slot
  int *head(int slot) const { return d_heads + slot; }
  int *d_cnt = nullptr;               // [4] list heads (CC_CNT_*) = head(CC_HD_CNT)
  cc_pass_rec *d_pass = nullptr;      // [QB][CC_CHK_STRIDE] dense, index = candidate iteration order
  unsigned char *d_pass_ok = nullptr; // [QB][CC_CHK_STRIDE]
  cc_cand_post *d_cpost = nullptr;    // [QB][CC_MAXCAND] dynamic thresholds only (cc_db_set_dynamic_thres): post-bar inputs per problem
  unsigned char *d_tidy = nullptr;    // [QB][CC_MAXCAND] ... and the candidates that survive the post bars
  int *d_pass_cnt = nullptr;
  cc_cand_out *d_cands = nullptr;     // [QB][CC_MAXCAND]
  cc_qstate *d_qstate = nullptr;
  int *d_nprob = nullptr;             // = head(CC_HD_NPROB); its first four slots (problems | 16-lane | 64-lane | pool head) go back to h_nprob
  cc_query_result_t *d_results = nullptr;
  cc_gmm_problem *d_prob = nullptr;   // [QB][CC_MAXCAND] problem of candidate k of query q
  int *d_prob_list = nullptr;         // [QB * CC_MAXCAND] dense list of the problems that exist
  cc_gmm_result *d_gres = nullptr;
  int *d_sel = nullptr;               // [3 + CC_GMM_NCLS][prob_cap] GMM problems that get the L-BFGS refinement, by cc_sel_list
  int *sel(int list) const { return d_sel + (size_t)list * prob_cap; }
  char *d_pool = nullptr;             // [pool_cap] records of CC_GRAW_BYTES: pair lists of the refined problems (what does not stay in LDS)
  int *d_pool_off = nullptr;          // [prob_cap] where a selected problem's records go in d_pool (cc_k_select)
  unsigned *d_codes = nullptr;        // [code_cap] pair-code segments of every correlation problem of the chunk (cc_k_gmm_init -> cc_k_gmm_refine)
  int prob_cap = 0, pool_cap = 0, code_cap = 0;
  // pinned host staging (asynchronous copies)
  cc_query_meta *h_meta = nullptr;
  cc_query_result_t *h_results = nullptr;
  int *h_nprob = nullptr;             // [4]
  // verify chunks (cc_db_verify_submit), allocated with the first one: per item the descriptor it reads and its candidates
  int *d_vin = nullptr;               // [QB] descriptor index | [QB][CC_VERIFY_CANDS_MAX] candidate lists
  int *h_vin = nullptr;               // the same, pinned: filled by the submit, one copy per chunk
  // masked chunks (cc_db_query_submit_masked), allocated with the first one: the row of the mask each query names, or -1
  int *d_mrow = nullptr;              // [QB]
  int *h_mrow = nullptr;              // the same, pinned
  // listed chunks (cc_db_query_submit_listed, include/cont2_amd_lists.h), allocated with the first one: per query its staged
  // entries (first, count) or (-1, 0), and the entries -- as many as the largest listed chunk the lane has seen
  cc_list_row *d_lrow = nullptr;      // [QB]
  cc_list_row *h_lrow = nullptr;      // the same, pinned
  cc_list_ent *d_lent = nullptr;      // [lent_cap]
  cc_list_ent *h_lent = nullptr;      // the same, pinned
  size_t lent_cap = 0;
  // ranked chunks (the *_ranked entry points), allocated with the first one: cc_k_final_r's lists, [nb][max_ret]
  cc_ranked_cand_t *d_rank = nullptr; // [QB * CC_RANK_MAX]
  cc_ranked_cand_t *h_rank = nullptr; // the same, pinned: copied out beside h_results (small chunks: written by the kernel)
  cc_rank_out_t rank_dst = {nullptr, nullptr, 0, 0};  // where the chunk's lists go when it is collected (h_cands NULL: not a ranked chunk)
  int rank_mfo = 0;                   // the chunk's max_fine_opt (the counts are min(max_ret, max_fine_opt, n_cand_tidy))
  // detail chunks (the *_ranked_detail entry points), allocated with the first one
  cc_gmm_hess *d_hess = nullptr;            // [prob_cap] cc_k_gmm_hess's record per refined problem
  cc_ranked_detail_t *d_detail = nullptr;   // [QB * CC_RANK_MAX] cc_k_final_rd's rows, beside d_rank
  cc_ranked_detail_t *h_detail = nullptr;   // the same, pinned (small chunks: written by the kernel)
  cc_ranked_detail_t *detail_dst = nullptr; // where the chunk's detail rows go when it is collected (nullptr: not a detail chunk)
  // matched chunks (the *_matched entry points, include/cont2_amd_matches.h), allocated with the first one
  cc_match_rec *d_mrec = nullptr;           // [QB][CC_MAXCAND] cc_k_merge_m's selected proposal per problem, at the problem's place
  cc_ranked_match_t *d_match = nullptr;     // [QB * CC_RANK_MAX] cc_k_match_emit's rows, beside d_rank
  cc_ranked_match_t *h_match = nullptr;     // the same, pinned (small chunks: written by the kernel)
  cc_ranked_match_t *match_dst = nullptr;   // where the chunk's match rows go when it is collected (nullptr: not a matched chunk)
  // pose chunks (cc_db_pose_submit), allocated with the first one.  In: item table | try poses | descriptor selector, filled by
  // the submit, one copy per chunk.  Out: result rows | try results | curvature rows, one copy back (small chunks: written by the kernels)
  char *d_pin = nullptr, *h_pin = nullptr;
  char *d_pout = nullptr, *h_pout = nullptr;
  bool pose = false;                        // the chunk in flight is a pose chunk: its rows are cc_pose_result_t, delivered below
  cc_pose_result_t *pose_res = nullptr;     // where the chunk's rows go when it is collected: row b0 + i of each array
  double *pose_try = nullptr;               // [n][pose_ntry] or nullptr
  cc_pose_curv_t *pose_curv = nullptr;      // [n] or nullptr
  int pose_ntry = 0;
};

struct cc_db {
  cc_ctx *ctx = nullptr;
  int device = 0;         // the context's device (kept here: the context may be destroyed first)
  int n_row = 0, n_col = 0;
  bool sync_call = false;  // cc_db_query_submit is running for cc_db_query_batch (chunking rule)
  bool poisoned = false;  // a HIP call failed after host and device state had started to diverge: every later call fails
  cc_db_cfg_t cfg;
  int cap = 0, n_scans = 0, cap_k = 0;
  cc_hot_desc_t *d_hot = nullptr;  // [cap]
  cc_gmm_feat *d_feat = nullptr;   // [cap]  per-scan correlation inputs of the DB scans
  float *d_keys[CC_NQLEV] = {nullptr, nullptr, nullptr};
  int *d_kgidx[CC_NQLEV] = {nullptr, nullptr, nullptr};
  unsigned char *d_kseq[CC_NQLEV] = {nullptr, nullptr, nullptr};
  int *d_kactive[CC_NQLEV] = {nullptr, nullptr, nullptr};
  // view of the keys sorted by their first dimension (double-buffered: a merge writes the other buffer)
  float *d_skeys[CC_NQLEV][CC_NVIEW] = {};
  int *d_sid[CC_NQLEV][CC_NVIEW] = {};
  int *d_sact[CC_NQLEV][CC_NVIEW] = {};
  int scur[CC_NQLEV] = {0, 0, 0};
  int *d_newpos[CC_NQLEV] = {nullptr, nullptr, nullptr};
  float *d_newsorted0[CC_NQLEV] = {nullptr, nullptr, nullptr};
  // staging of an append: per new key (scan << 3 | anchor), then the tails of the activation arrays (pinned; one upload)
  int *h_add = nullptr, *d_add = nullptr;
  int *h_add_small[CC_NSTAGE] = {};             // CC_ZC_MAX * 64 ints each: the staging of an append small enough for the zero-copy kernel
  hipEvent_t add_small_ev[CC_NSTAGE] = {};      // recorded behind the append that read the buffer
  bool add_small_busy[CC_NSTAGE] = {};
  int add_small_next = 0;
  size_t add_cap = 0;  // ints
  int n_keys[CC_NQLEV] = {0, 0, 0};
  cchost::LayerBook book[CC_NQLEV];
  std::vector<ScanLite> lite;                        // host mirror, one per DB scan
  std::vector<std::array<float, CC_NQLEV * 7>> ranges_hist;  // per epoch
  std::vector<std::array<int, CC_NQLEV>> nkeys_hist;         // per epoch
  // per epoch: -1 when every bucket of every layer indexes its whole range (cc_hostdb.h, Bucket::idx_lo / idx_hi: the steady
  // state), else the position of the epoch's record in idx_store: per layer a full flag and the six indexed intervals
  std::vector<int> idx_slot;
  struct IdxRec {
    int full[CC_NQLEV];
    float iv[CC_NQLEV][12];
  };
  std::vector<IdxRec> idx_store;
  // query scratch: two lanes, each with its own stream, so that consecutive QB-query chunks of a batch overlap
  // (the f64-ALU-bound correlation of one chunk runs next to the latency-bound retrieval/checks of the next)
  static const int QB = 1024;  // queries per chunk (one launch chain): every chain pays ~20 launches and ~20 kernel tails,
                               // a quarter of a 512-query chain's time (measured: 256 / 384 / 512 queries per chunk
                               // 354 / 396 / 440 k scans/s)
  int kmax = CC_KNN_MAX;  // hits per search of the query kernels: CC_KNN_MAX, or CC_KNN_MAX_LARGE when nnk > CC_KNN_MAX (the _l instances)
  int qb_max = QB;        // queries per chunk: QB * CC_KNN_MAX / kmax, so that a lane's per-slot buffers keep their byte size
  static const int KQB = 1024;  // ... of which the tiled K3 takes this many at a time (round 3: 512 -- two launches per chunk, each as long as
                                // its widest group; one launch lets the second half's groups fill in behind the first half's stragglers)
  static_assert(KQB * CC_NPIV <= CC_KNN_ORDER_CAP, "cc_k_knn_order sorts a sub-chunk's searches of one layer in LDS");
  static const int NLANE = 4;  // lanes that exist; n_lanes of them are used (a process gets 4 hardware queues by default:
                               // with the caller's streams, more than 2 lanes only pay off with GPU_MAX_HW_QUEUES raised)
  cc_qlane lane[NLANE];
  int n_lanes = 2;      // lanes in use (cc_db_set_lanes)
  int dyn_thres = 0;    // cc_db_set_dynamic_thres: the chains submitted from now on replay the reference's DYNAMIC_THRES=1 bars
  int next_lane = 0;    // lane of the next query chunk
  struct {  // launch geometry of the list-driven kernels (workgroups); env CC_B1_GRID / CC_B2_GRID / CC_GMM_GRID, read once
    int b1 = 256 * 16, b2 = 256 * 16, gmm = 256 * 16;
    int gmm64 = 256 * 32;  // CC_GMM_GRID64: workgroups (= waves = problems at a time) of the 64-lane refinement instance: with one
                           // problem per workgroup and thousands of long problems per dense-world chunk a small grid makes every
                           // workgroup chain two or three of them and the launch end on its unluckiest chain (2 048 / 8 192 /
                           // 32 768 workgroups: K5 0.98 / 0.90 / 0.90 ms on the dense world, 0.55 / 0.52 / 0.53 at the headline)
    int chunk = QB;   // CC_CHUNK: queries per chunk launch chain (<= QB)
    int knn_mode = 1;   // CC_KNN_MODE: 0 = one wave per search (cc_k_knn), 2 = tiled with the matrix-core prefilter (cc_k_knn_tile),
                        // 1 = by size: tiled once a layer holds CC_KNN_TILE_MIN_KEYS keys (k_knn.h: +2 % at a 5 000-scan DB on contour-rich
                        // scans, +53 % at 50 000 scans)
    int a_class[3] = {8, 14, 22};    // CC_A_CLASSES: overlap counts separating the size classes of the check list (stage A -> B1)
    int b2_class[3] = {6, 10, 16};   // CC_B2_CLASSES: constellation lengths separating the size classes of stage B2's list
  } tune;
  ScanLite *d_lite = nullptr;
  ScanLite *h_lite_zc = nullptr;  // [CC_ZC_MAX] pinned, device-visible: cc_k_extract writes a small append's records straight to the host
  unsigned short *d_perm_tab = nullptr;  // what std::sort does to n equal keys, for every n <= the candidate capacity (cc_tidy_order)
  // cc_db_add_scans_prepare: batches whose records are packed and whose keys are on their way to the host, in order
  struct Prepared {
    const cc_scan_desc_t *d_desc = nullptr;
    int n = 0, row0 = 0;
    hipEvent_t ev = nullptr;
    ScanLite *d_lite = nullptr, *h_lite = nullptr;  // [PREP_MAX], h_lite pinned
  };
  static const int PREP_SLOTS = 2, PREP_MAX = 4096;
  Prepared prep[PREP_SLOTS];
  int prep_head = 0, prep_cnt = 0, n_prepared = 0;
  // the device part of the last append: recorded on the caller's stream instead of waited for.  The lanes wait for it on
  // the device before a chunk starts; the host waits only before it reuses the pinned staging buffer (the next append).
  hipEvent_t add_done = nullptr;
  hipStream_t add_stream = nullptr;  // the stream the last append was queued on (valid while add_done exists)
  bool add_pending = false;
  cc_scan_desc_t *d_stage = nullptr;  // staging for the host-descriptor entry points
  int stage_cap = 0;
  uint32_t *d_mask_stage = nullptr;   // staging for the table of cc_db_query_batch_host_masked, in words
  size_t mask_stage_cap = 0;
  long long knn_chunks[3] = {0, 0, 0};  // query chunks by retrieval so far: walk | tiled | masked walk (cc_db_debug_knn_chunks)
  long long knn_chunks_listed[2] = {0, 0};  // ... that ran the list retrieval alone | behind the unrestricted one (cc_db_debug_knn_chunks_listed)
  cc_scan_desc_t *d_hstage[2] = {nullptr, nullptr};  // [CC_SCAN_BATCH_MAX] each: the descriptors of a batch of scan handles, gathered (append | query)
  int *d_hint_scores = nullptr;     // [CC_CHK_STRIDE][CC_NSCORE] per-check gate scores (cc_db_check_hints)
  bool prof = false;
  int prof_every = 1, prof_tick = 0;  // every prof_every-th chunk carries the stage events
  double ms_acc[5] = {0, 0, 0, 0, 0};
  double launch_w = 0;  // profiled queries
  // tuning aid (CC_ADD_TIMERS=1): host seconds of the appends, by part, printed at cc_db_destroy
  bool add_timers = false;
  double add_s[3] = {0, 0, 0};  // waiting for the new scans' keys | bookkeeping | uploads + merge launches + final wait
  long add_calls = 0, add_scans_n = 0;
};

static void db_free(cc_db *db) {
  hipFree(db->d_hot);
  hipFree(db->d_feat);
  for (int l = 0; l < CC_NQLEV; l++) {
    hipFree(db->d_keys[l]);
    hipFree(db->d_kgidx[l]);
    hipFree(db->d_kseq[l]);
    hipFree(db->d_kactive[l]);
    for (int b = 0; b < CC_NVIEW; b++) {
      hipFree(db->d_skeys[l][b]);
      hipFree(db->d_sid[l][b]);
      hipFree(db->d_sact[l][b]);
    }
  }
  for (int l = 0; l < CC_NQLEV; l++) {
    hipFree(db->d_newpos[l]);
    hipFree(db->d_newsorted0[l]);
  }
  hipFree(db->d_add);
  if (db->h_add) hipHostFree(db->h_add);
  for (int i = 0; i < CC_NSTAGE; i++) {
    if (db->h_add_small[i]) hipHostFree(db->h_add_small[i]);
    if (db->add_small_ev[i]) hipEventDestroy(db->add_small_ev[i]);
  }
  for (auto &ln : db->lane) {
    hipFree(ln.d_qmeta);
    hipFree(ln.d_qhot);
    hipFree(ln.d_qfeat);
    hipFree(ln.d_hits);
    hipFree(ln.d_hit_cnt);
    hipFree(ln.d_knn_order);
    hipFree(ln.d_items);
    hipFree(ln.d_redo);
    hipFree(ln.d_cstl);
    hipFree(ln.d_cstl_idx);
    hipFree(ln.d_heads);
    hipFree(ln.d_pass);
    hipFree(ln.d_pass_cnt);
    hipFree(ln.d_pass_ok);
    hipFree(ln.d_cpost);
    hipFree(ln.d_tidy);
    hipFree(ln.d_cands);
    hipFree(ln.d_qstate);
    hipFree(ln.d_results);
    hipFree(ln.d_prob);
    hipFree(ln.d_prob_list);
    hipFree(ln.d_gres);
    hipFree(ln.d_sel);
    hipFree(ln.d_pool);
    hipFree(ln.d_codes);
    hipFree(ln.d_pool_off);
    hipHostFree(ln.h_meta);
    hipHostFree(ln.h_results);
    hipHostFree(ln.h_nprob);
    hipFree(ln.d_vin);
    if (ln.h_vin) hipHostFree(ln.h_vin);
    hipFree(ln.d_mrow);
    if (ln.h_mrow) hipHostFree(ln.h_mrow);
    hipFree(ln.d_lrow);
    if (ln.h_lrow) hipHostFree(ln.h_lrow);
    hipFree(ln.d_lent);
    if (ln.h_lent) hipHostFree(ln.h_lent);
    hipFree(ln.d_rank);
    if (ln.h_rank) hipHostFree(ln.h_rank);
    hipFree(ln.d_pin);
    if (ln.h_pin) hipHostFree(ln.h_pin);
    hipFree(ln.d_pout);
    if (ln.h_pout) hipHostFree(ln.h_pout);
    hipFree(ln.d_hess);
    hipFree(ln.d_detail);
    if (ln.h_detail) hipHostFree(ln.h_detail);
    hipFree(ln.d_mrec);
    hipFree(ln.d_match);
    if (ln.h_match) hipHostFree(ln.h_match);
    if (ln.done) hipEventDestroy(ln.done);
    if (ln.prep) hipEventDestroy(ln.prep);
    if (ln.fin) hipEventDestroy(ln.fin);
    for (auto &e : ln.pev)
      if (e) hipEventDestroy(e);
    if (ln.stream) stream_give(db->device, ln.stream);
  }
  hipFree(db->d_lite);
  if (db->h_lite_zc) hipHostFree(db->h_lite_zc);
  hipFree(db->d_perm_tab);
  if (db->add_done) hipEventDestroy(db->add_done);
  for (auto &pp : db->prep) {
    if (pp.ev) hipEventDestroy(pp.ev);
    hipFree(pp.d_lite);
    if (pp.h_lite) hipHostFree(pp.h_lite);
  }
  hipFree(db->d_stage);
  hipFree(db->d_mask_stage);
  hipFree(db->d_hstage[0]);
  hipFree(db->d_hstage[1]);
  hipFree(db->d_hint_scores);
}

// Everything a query lane owns (stream, events, ~0.85 GB of device scratch at QB = 1024: the pair pool alone is QB * 8192
// pairs * 80 B = 640 MiB), allocated when the lane comes into use: at cc_db_create for the default two lanes, in
// cc_db_set_lanes for more.  A handle that uses one lane (the class mirror's per-setting stores) pays for one.
// The per-slot buffers are sized QB * CC_CHK_STRIDE (hits: QB * NS * CC_KNN_MAX): a large-k database (nnk > CC_KNN_MAX) runs
// chunks of qb_max = QB * CC_KNN_MAX / CC_KNN_MAX_LARGE = 256 queries with four times the slots each, in the same bytes.
static int lane_env_int(const char *name, int lo, int hi, int dflt) {
  const char *e = getenv(name);
  if (!e) return dflt;
  const int v = atoi(e);
  return v >= lo && v <= hi ? v : dflt;
}
// One buffer of the sets a lane gets on demand (below): allocated when it is not there yet.  A failed pointer stays null, so the
// next call tries again.  `who`: the set's function, for the message.
static int lane_buf(void **p, size_t bytes, bool pinned, const char *who) {
  if (*p) return CC_OK;
  const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
  if (e == hipSuccess) return CC_OK;
  *p = nullptr;
  return set_err(CC_EHIP, (std::string(who) + (pinned ? ": hipHostMalloc" : ": hipMalloc")).c_str(), e);
}
#define LANE_BUF(ptr, bytes, pinned)                                         \
  {                                                                          \
    const int brc_ = lane_buf((void **)&(ptr), bytes, pinned, __func__);     \
    if (brc_ != CC_OK) return brc_;                                          \
  }
// the dynamic-threshold buffers of a lane (19 MB at QB = 1 024): allocated once the mode is first switched on
// (d_tidy last: where it exists, both do; a failed call leaves the lane without it, and the next call tries again)
static int lane_alloc_dyn(cc_qlane &ln) {
  const size_t n = (size_t)cc_db::QB * CC_MAXCAND;
  LANE_BUF(ln.d_cpost, sizeof(cc_cand_post) * n, false);
  LANE_BUF(ln.d_tidy, n, false);
  return CC_OK;
}
// the item table of a lane's verify chunks (36 KB), allocated with the lane's first one
static int lane_alloc_verify(cc_qlane &ln) {
  const size_t bytes = sizeof(int) * (size_t)cc_db::QB * (1 + CC_VERIFY_CANDS_MAX);
  LANE_BUF(ln.h_vin, bytes, true);
  LANE_BUF(ln.d_vin, bytes, false);
  return CC_OK;
}
// the row table of a lane's masked chunks (4 KB), allocated with the lane's first one
static int lane_alloc_mask(cc_qlane &ln) {
  const size_t bytes = sizeof(int) * (size_t)cc_db::QB;
  LANE_BUF(ln.h_mrow, bytes, true);
  LANE_BUF(ln.d_mrow, bytes, false);
  return CC_OK;
}
// the tables of a lane's listed chunks: the row table (8 KB) with the lane's first one; the entries grow to the largest chunk
// the lane has seen (`need` entries for the chunk at hand; 16 MB for a full chunk of full lists).  The lane is idle here
// (submit_chunks has collected its previous chunk), so the old buffers may go.
static int lane_alloc_lists(cc_qlane &ln, size_t need) {
  LANE_BUF(ln.h_lrow, sizeof(cc_list_row) * (size_t)cc_db::QB, true);
  LANE_BUF(ln.d_lrow, sizeof(cc_list_row) * (size_t)cc_db::QB, false);
  if (need <= ln.lent_cap) return CC_OK;
  // to the next power of two (at least 4 096 entries, 64 KB): chunks that slowly get larger do not pay a hipFree -- a
  // device-wide synchronisation -- and a pinned allocation per step
  size_t cap = 4096;
  while (cap < need) cap <<= 1;
  need = cap;
  hipFree(ln.d_lent);
  if (ln.h_lent) hipHostFree(ln.h_lent);
  ln.d_lent = nullptr;
  ln.h_lent = nullptr;
  ln.lent_cap = 0;
  LANE_BUF(ln.h_lent, sizeof(cc_list_ent) * need, true);
  LANE_BUF(ln.d_lent, sizeof(cc_list_ent) * need, false);
  ln.lent_cap = need;
  return CC_OK;
}
// the tables of a lane's pose chunks (2 x 228 KB in, 2 x 200 KB out), allocated with the lane's first one
#define CC_POSE_IN_BYTES(nb, n_try) ((size_t)(nb) * (sizeof(cc_pose_item_t) + (size_t)(n_try) * 3 * sizeof(double) + sizeof(int)))
#define CC_POSE_OUT_BYTES(nb, n_try, curv) ((size_t)(nb) * (sizeof(cc_pose_result_t) + (size_t)(n_try) * sizeof(double) + ((curv) ? sizeof(cc_pose_curv_t) : 0)))
static int lane_alloc_pose(cc_qlane &ln) {
  const size_t bin = CC_POSE_IN_BYTES(cc_db::QB, CC_POSE_TRY_MAX), bout = CC_POSE_OUT_BYTES(cc_db::QB, CC_POSE_TRY_MAX, true);
  LANE_BUF(ln.h_pin, bin, true);
  LANE_BUF(ln.h_pout, bout, true);
  LANE_BUF(ln.d_pin, bin, false);
  LANE_BUF(ln.d_pout, bout, false);
  return CC_OK;
}
// the list buffers of a lane's ranked chunks (2 x 640 KB), allocated with the lane's first one
static int lane_alloc_rank(cc_qlane &ln) {
  const size_t bytes = sizeof(cc_ranked_cand_t) * (size_t)cc_db::QB * CC_RANK_MAX;
  LANE_BUF(ln.h_rank, bytes, true);
  LANE_BUF(ln.d_rank, bytes, false);
  return CC_OK;
}
// the buffers of a lane's detail chunks (2 x 1.9 MB and the Hessian records, 72 B per problem slot), allocated with the lane's
// first one (after lane_alloc: prob_cap is known)
static int lane_alloc_detail(cc_qlane &ln) {
  if (ln.d_detail && ln.d_hess) return CC_OK;
  if (ln.prob_cap <= 0) return set_err(CC_EHIP, "lane_alloc_detail: the lane has no problem buffers");
  const size_t bytes = sizeof(cc_ranked_detail_t) * (size_t)cc_db::QB * CC_RANK_MAX;
  LANE_BUF(ln.h_detail, bytes, true);
  LANE_BUF(ln.d_hess, sizeof(cc_gmm_hess) * (size_t)ln.prob_cap, false);
  LANE_BUF(ln.d_detail, bytes, false);
  return CC_OK;
}
// the buffers of a lane's matched chunks, allocated with the lane's first one: the selected proposals at the problem's place
// (QB * CC_MAXCAND records of 72 B: 85 MB, a tenth of what the lane holds anyway) and the rows (2 x 1.5 MB)
static int lane_alloc_match(cc_qlane &ln) {
  const size_t bytes = sizeof(cc_ranked_match_t) * (size_t)cc_db::QB * CC_RANK_MAX;
  LANE_BUF(ln.h_match, bytes, true);
  LANE_BUF(ln.d_match, bytes, false);
  LANE_BUF(ln.d_mrec, sizeof(cc_match_rec) * (size_t)cc_db::QB * CC_MAXCAND, false);
  return CC_OK;
}
#undef LANE_BUF
// The refusals of the *_matched entry points (match given), worded with the entry point's name; db may be NULL (the call's own
// argument check names that).
static int want_match(const char *fn, const cc_db *db, const cc_rank_out_t *rank, const cc_match_out_t *match) {
  if (!rank) return set_err(CC_EINVAL, (std::string(fn) + ": match comes with rank (the rows belong to the entries of the ranked list)").c_str());
  if (!match->h_match) return set_err(CC_EINVAL, (std::string(fn) + ": h_match must be given").c_str());
  if (!(match->inlier_px >= 0.0) || std::isinf(match->inlier_px))
    return set_err(CC_EINVAL, (std::string(fn) + ": inlier_px must be finite and >= 0").c_str());
  if (db && db->dyn_thres)
    return set_err(CC_EINVAL, (std::string(fn) + ": matches are not supported in dynamic-threshold mode (cc_db_set_dynamic_thres): no test oracle "
                                                 "for merged constellations under rising bars exists").c_str());
  return CC_OK;
}
// The refusals of the *_ranked / *_ranked_detail entry points, worded with the entry point's name (`fn`).  need_detail: the
// call is a *_ranked_detail one.
static int want_ranked(const char *fn, const cc_rank_out_t *rank, const cc_ranked_detail_t *detail, bool need_detail) {
  if (!rank || !rank->h_cands || !rank->h_n || rank->max_ret < 1 || rank->max_ret > CC_RANK_MAX)
    return set_err(CC_EINVAL, (std::string(fn) + ": rank, its h_cands and h_n must be given and max_ret lie within 1..CC_RANK_MAX").c_str());
  if (need_detail && !detail) return set_err(CC_EINVAL, (std::string(fn) + ": h_detail must be given").c_str());
  return CC_OK;
}
// a collected chunk's lists: rows [b0, b0 + nb) of the caller's arrays
static void rank_deliver(const cc_qlane &ln, const cc_rank_out_t &dst, int b0, int nb, int max_fine_opt) {
  const int mr = dst.max_ret;
  memcpy(dst.h_cands + (size_t)b0 * mr, ln.h_rank, sizeof(cc_ranked_cand_t) * (size_t)nb * mr);
  for (int i = 0; i < nb; i++) {
    const cc_query_result_t &r = ln.h_results[i];
    const int pre = max_fine_opt < r.n_cand_tidy ? max_fine_opt : r.n_cand_tidy;
    dst.h_n[b0 + i] = r.n_res > 0 ? (mr < pre ? mr : pre) : 0;
  }
}
static int lane_alloc(cc_db *db, cc_qlane &ln) {
  if (ln.d_qmeta) return db->dyn_thres ? lane_alloc_dyn(ln) : CC_OK;  // (an earlier call may have failed on the dynamic buffers)
  const int QB = cc_db::QB, NS = CC_NQLEV * CC_NPIV;
#define LN_CHK(x)                                                           \
  do {                                                                      \
    hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) return set_err(CC_EHIP, #x, e_);                  \
  } while (0)
  // A lane's stream is created when the lane comes into use (cc_db_set_lanes): a process has few hardware queues
  // (4 by default) and HIP hands them to streams in creation order, so streams of lanes nobody uses would push the
  // caller's own streams (e.g. the one it ingests on) onto a queue shared with a busy lane -- measured: 7 % on the bench.
  if (!ln.stream) LN_CHK(stream_take(db->device, &ln.stream));
  LN_CHK(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
  LN_CHK(hipEventCreateWithFlags(&ln.prep, hipEventDisableTiming));
  LN_CHK(hipEventCreateWithFlags(&ln.fin, hipEventDisableTiming));
  LN_CHK(hipMalloc(&ln.d_qmeta, sizeof(cc_query_meta) * QB));
  LN_CHK(hipMalloc(&ln.d_qhot, sizeof(cc_hot_desc_t) * (size_t)QB));
  LN_CHK(hipMalloc(&ln.d_qfeat, sizeof(cc_gmm_feat) * (size_t)QB));
  LN_CHK(hipMalloc(&ln.d_hits, sizeof(cc_knn_hit_t) * (size_t)QB * NS * CC_KNN_MAX));
  LN_CHK(hipMalloc(&ln.d_hit_cnt, sizeof(int) * QB * NS));
  LN_CHK(hipMalloc(&ln.d_knn_order, sizeof(int) * CC_KNN_ORD_INTS));
  LN_CHK(hipMalloc(&ln.d_items, sizeof(cc_chk_item) * (size_t)QB * CC_CHK_STRIDE));
  LN_CHK(hipMalloc(&ln.d_redo, sizeof(int) * (size_t)QB * CC_CHK_STRIDE));
  LN_CHK(hipMalloc(&ln.d_cstl, sizeof(cc_cstl_item) * (size_t)QB * CC_CHK_STRIDE));
  LN_CHK(hipMalloc(&ln.d_cstl_idx, sizeof(int) * (size_t)QB * CC_CHK_STRIDE));
  LN_CHK(hipMalloc(&ln.d_heads, sizeof(int) * CC_N_HEADS));  // the chunk's list heads, cleared together by the prep kernel
  ln.d_nprob = ln.head(CC_HD_NPROB);
  ln.d_cnt = ln.head(CC_HD_CNT);
  LN_CHK(hipMalloc(&ln.d_pass, sizeof(cc_pass_rec) * (size_t)QB * CC_CHK_STRIDE));
  LN_CHK(hipMalloc(&ln.d_pass_ok, (size_t)QB * CC_CHK_STRIDE));
  LN_CHK(hipMalloc(&ln.d_pass_cnt, sizeof(int) * QB * 4));
  LN_CHK(hipMalloc(&ln.d_cands, sizeof(cc_cand_out) * (size_t)QB * CC_MAXCAND));
  LN_CHK(hipMalloc(&ln.d_qstate, sizeof(cc_qstate) * QB));
  LN_CHK(hipMalloc(&ln.d_results, sizeof(cc_query_result_t) * QB));
  ln.prob_cap = QB * CC_MAXCAND;
  LN_CHK(hipMalloc(&ln.d_prob, sizeof(cc_gmm_problem) * (size_t)ln.prob_cap));
  LN_CHK(hipMalloc(&ln.d_prob_list, sizeof(int) * (size_t)ln.prob_cap));
  LN_CHK(hipMalloc(&ln.d_gres, sizeof(cc_gmm_result) * (size_t)ln.prob_cap));
  LN_CHK(hipMalloc(&ln.d_sel, sizeof(int) * (3 + CC_GMM_NCLS) * (size_t)ln.prob_cap));  // the lists of cc_sel_list
  // pair lists of the refined correlation problems come from one pool per lane (80 B per pair: 640 MiB at 8192 pairs per
  // query of a full chunk; measured use: ~600 per query on the dense world, ~1 700 on the KITTI-shaped one).  Overflow is reported (CC_ECAPACITY), never
  // truncated.  CC_GMM_POOL_PAIRS overrides the size in pairs (a test forces the overflow with it).
  ln.pool_cap = lane_env_int("CC_GMM_POOL_PAIRS", 16, 1 << 30, QB * 8192);
  LN_CHK(hipMalloc(&ln.d_pool, (size_t)CC_GRAW_BYTES * (size_t)ln.pool_cap));
  // EVERY problem's codes (not only the refined ones'), 4 B per pair + 8 B per segment of <= 256
  // half of it: first blocks of 258 entries, one per problem of the chunk (~30 000 problems on a sparse scene, ~160 000 with a
  // 50 000-scan DB; 124 000 fit the default), the other half: the blocks taken from the head
  ln.code_cap = lane_env_int("CC_GMM_POOL_CODES", 1024, 1 << 30, 64 << 20);
  LN_CHK(hipMalloc(&ln.d_pool_off, sizeof(int) * (size_t)ln.prob_cap));
  LN_CHK(hipMalloc(&ln.d_codes, sizeof(unsigned) * (size_t)ln.code_cap));
  LN_CHK(hipHostMalloc((void **)&ln.h_meta, sizeof(cc_query_meta) * QB, hipHostMallocDefault));
  LN_CHK(hipHostMalloc((void **)&ln.h_results, sizeof(cc_query_result_t) * QB, hipHostMallocDefault));
  LN_CHK(hipHostMalloc((void **)&ln.h_nprob, sizeof(int) * 4, hipHostMallocDefault));
  if (db->prof)
    for (auto &e : ln.pev)
      if (!e) LN_CHK(hipEventCreate(&e));
#undef LN_CHK
  return db->dyn_thres ? lane_alloc_dyn(ln) : CC_OK;
}

int cc_db_create(cc_ctx *ctx, const cc_db_cfg_t *cfg, int capacity_scans, cc_db **out) {
  if (!ctx || !cfg || !out || capacity_scans < 1) return set_err(CC_EINVAL, "cc_db_create: bad argument");
  if (cfg->n_q_levels < 1 || cfg->n_q_levels > CC_NQLEV || cfg->nnk < 1 || cfg->nnk > CC_KNN_MAX_LARGE)
    return set_err(CC_EINVAL, "cc_db_create: unsupported ContourDBConfig (q_levels_ <= 3, 1 <= nnk_ <= CC_KNN_MAX_LARGE = 256)");
  for (int i = 0; i < cfg->n_q_levels; i++)
    if (cfg->q_levels[i] < 1 || cfg->q_levels[i] > CC_HOT_LEVELS) return set_err(CC_EINVAL, "cc_db_create: q_levels_ must be within 1..4");
  if (cfg->max_fine_opt < 1) return set_err(CC_EINVAL, "cc_db_create: max_fine_opt_ must be positive");
  // a key id fits 28 bits: the staged entries of a listed query pack (first key id << 3 | key count) into 32 (k_knn_list.h)
  if ((long long)capacity_scans * CC_NPIV > (1ll << 28)) return set_err(CC_EINVAL, "cc_db_create: capacity_scans * CC_NPIV keys per layer exceed 2^28 key ids");
  HIPCHK(hipSetDevice(ctx->device));
  cc_db *db = new cc_db();
  db->ctx = ctx;
  db->device = ctx->device;
  db->n_row = ctx->mcfg.n_row;
  db->n_col = ctx->mcfg.n_col;
#define DB_CHK(call)                        \
  do {                                      \
    hipError_t e_ = (call);                 \
    if (e_ != hipSuccess) {                 \
      cc_db_destroy(db);                    \
      return set_err(CC_EHIP, #call, e_);   \
    }                                       \
  } while (0)
  db->cfg = *cfg;
  db->kmax = cfg->nnk > CC_KNN_MAX ? CC_KNN_MAX_LARGE : CC_KNN_MAX;
  db->qb_max = cc_db::QB * CC_KNN_MAX / db->kmax;
  db->cap = capacity_scans;
  db->cap_k = capacity_scans * CC_NPIV;
  DB_CHK(hipMalloc(&db->d_hot, sizeof(cc_hot_desc_t) * (size_t)db->cap));
  DB_CHK(hipMalloc(&db->d_feat, sizeof(cc_gmm_feat) * (size_t)db->cap));
  for (int l = 0; l < cfg->n_q_levels; l++) {
    DB_CHK(hipMalloc(&db->d_keys[l], sizeof(float) * CC_KEY_DIM * (size_t)db->cap_k));
    DB_CHK(hipMalloc(&db->d_kgidx[l], sizeof(int) * (size_t)db->cap_k));
    DB_CHK(hipMalloc(&db->d_kseq[l], (size_t)db->cap_k));
    DB_CHK(hipMalloc(&db->d_kactive[l], sizeof(int) * (size_t)db->cap_k));
    for (int b = 0; b < CC_NVIEW; b++) {
      DB_CHK(hipMalloc(&db->d_skeys[l][b], sizeof(float) * (CC_KEY_DIM + 1) * (size_t)db->cap_k));
      DB_CHK(hipMalloc(&db->d_sid[l][b], sizeof(int) * (size_t)db->cap_k));
      DB_CHK(hipMalloc(&db->d_sact[l][b], sizeof(int) * (size_t)db->cap_k));
    }
    db->book[l].init(cfg->max_elapse, cfg->min_elapse);
  }
  for (int l = 0; l < cfg->n_q_levels; l++) {
    DB_CHK(hipMalloc(&db->d_newpos[l], sizeof(int) * (size_t)db->cap_k));
    DB_CHK(hipMalloc(&db->d_newsorted0[l], sizeof(float) * (size_t)db->cap_k));
  }
  db->add_cap = (size_t)db->cap_k * 2 * CC_NQLEV;
  DB_CHK(hipMalloc(&db->d_add, sizeof(int) * (size_t)db->cap_k * CC_NQLEV));
  {
    // fineOptimize sorts candidates whose correlation_ is still 0 (contour_db.h:604-610): with a comparator that never
    // says "less", std::sort is a permutation that depends on the length alone.  One row per length, made by std::sort
    // itself (the libstdc++ the reference is built with; csrc/cc_sort.h replays the same algorithm where keys matter).
    // (the large-k table, up to 4 608 candidates, is 21 MB; its rows for n <= CC_MAXCAND are the common table, which the
    // hint flow's 64-stride kernels read)
    const int mc = CC_CHK_STRIDE_K(db->kmax);
    std::vector<unsigned short> tab((size_t)mc * (mc + 1) / 2);
    for (int n = 1; n <= mc; n++) {
      unsigned short *row = tab.data() + (size_t)n * (n - 1) / 2;
      for (int i = 0; i < n; i++) row[i] = (unsigned short)i;
      std::sort(row, row + n, [](unsigned short, unsigned short) { return false; });
    }
    DB_CHK(hipMalloc(&db->d_perm_tab, sizeof(unsigned short) * tab.size()));
    DB_CHK(hipMemcpy(db->d_perm_tab, tab.data(), sizeof(unsigned short) * tab.size(), hipMemcpyHostToDevice));
  }
  DB_CHK(hipHostMalloc((void **)&db->h_add, sizeof(int) * db->add_cap, hipHostMallocDefault));
  for (int i = 0; i < CC_NSTAGE; i++) {
    DB_CHK(hipHostMalloc((void **)&db->h_add_small[i], sizeof(int) * (size_t)CC_ZC_MAX * 64, hipHostMallocDefault));
    DB_CHK(hipEventCreateWithFlags(&db->add_small_ev[i], hipEventDisableTiming));
  }
  db->tune.b1 = lane_env_int("CC_B1_GRID", 1, 1 << 20, db->tune.b1);
  db->tune.b2 = lane_env_int("CC_B2_GRID", 1, 1 << 20, db->tune.b2);
  db->tune.gmm = lane_env_int("CC_GMM_GRID", 1, 1 << 20, db->tune.gmm);
  db->tune.gmm64 = lane_env_int("CC_GMM_GRID64", 1, 1 << 20, getenv("CC_GMM_GRID") ? (db->tune.gmm + 1) / 2 : db->tune.gmm64);
  db->tune.knn_mode = lane_env_int("CC_KNN_MODE", 0, 2, db->tune.knn_mode);
  db->add_timers = getenv("CC_ADD_TIMERS") != nullptr;
  db->tune.chunk = lane_env_int("CC_CHUNK", 64, cc_db::QB, db->tune.chunk);
  db->tune.chunk = db->tune.chunk < db->qb_max ? db->tune.chunk : db->qb_max;
  auto env_triple = [](const char *name, int (&v)[3]) {
    const char *e = getenv(name);
    int a, b, c;
    if (e && sscanf(e, "%d:%d:%d", &a, &b, &c) == 3 && a <= b && b <= c) {
      v[0] = a;
      v[1] = b;
      v[2] = c;
    }
  };
  env_triple("CC_A_CLASSES", db->tune.a_class);
  env_triple("CC_B2_CLASSES", db->tune.b2_class);
  for (int i = 0; i < db->n_lanes; i++) {
    const int lrc = lane_alloc(db, db->lane[i]);
    if (lrc != CC_OK) {
      cc_db_destroy(db);
      return lrc;
    }
  }
  DB_CHK(hipMalloc(&db->d_lite, sizeof(ScanLite) * (size_t)4096));
  DB_CHK(hipFuncSetAttribute((const void *)cc_k_knn_order, hipFuncAttributeMaxDynamicSharedMemorySize, CC_KNN_ORDER_LDS));
  DB_CHK(hipHostMalloc((void **)&db->h_lite_zc, sizeof(ScanLite) * CC_ZC_MAX, hipHostMallocDefault));
#undef DB_CHK
  std::array<float, CC_NQLEV * 7> r0;
  std::array<int, CC_NQLEV> k0;
  for (int l = 0; l < CC_NQLEV; l++) {
    k0[l] = 0;
    for (int b = 0; b < 7; b++) r0[l * 7 + b] = (l < cfg->n_q_levels) ? db->book[l].ranges[b] : 0.f;
  }
  db->ranges_hist.push_back(r0);
  db->nkeys_hist.push_back(k0);
  db->idx_slot.push_back(-1);  // nothing is in a tree yet: nothing to hide
  *out = db;
  return CC_OK;
}

int cc_db_destroy(cc_db *db) {
  if (!db) return CC_OK;
  hipSetDevice(db->device);
  if (db->add_timers && db->add_calls)
    fprintf(stderr, "[cc_db appends: %ld calls, %ld scans; host us per scan] wait for keys %.2f  bookkeeping %.2f  upload + merge + wait %.2f\n",
            db->add_calls, db->add_scans_n, db->add_s[0] * 1e6 / db->add_scans_n, db->add_s[1] * 1e6 / db->add_scans_n,
            db->add_s[2] * 1e6 / db->add_scans_n);
  for (auto &ln : db->lane)
    if (ln.busy && ln.stream) hipStreamSynchronize(ln.stream);
  if (db->add_done) hipEventSynchronize(db->add_done);  // the last append (whichever staging buffer it read) has passed
  for (int i = 0; i < db->prep_cnt; i++)  // copies of prepared batches still travelling to the pinned buffers freed below
    hipEventSynchronize(db->prep[(db->prep_head + i) % cc_db::PREP_SLOTS].ev);
  db_free(db);
  delete db;
  return CC_OK;
}

int cc_db_profile_enable(cc_db *db, int on) {
  if (!db) return set_err(CC_EINVAL, "cc_db_profile_enable: bad argument");
  HIPCHK(hipSetDevice(db->device));
  if (on)
    for (auto &ln : db->lane)
      if (ln.d_qmeta)  // lanes that come into use later get theirs in lane_alloc
        for (auto &e : ln.pev)
          if (!e) HIPCHK(hipEventCreate(&e));
  db->prof = on != 0;
  db->prof_every = on > 1 ? on : 1;
  db->prof_tick = 0;
  return CC_OK;
}
int cc_db_profile_read(cc_db *db, double ms_out[5], int *n_launches) {
  if (!db || !ms_out) return set_err(CC_EINVAL, "cc_db_profile_read: bad argument");
  for (int i = 0; i < 5; i++) {
    ms_out[i] = db->ms_acc[i];
    db->ms_acc[i] = 0;
  }
  if (n_launches) *n_launches = (int)(db->launch_w + 0.5);  // number of queries the sums cover
  db->launch_w = 0;
  return CC_OK;
}

int cc_db_set_lanes(cc_db *db, int n) {
  if (!db || n < 1 || n > cc_db::NLANE) return set_err(CC_EINVAL, "cc_db_set_lanes: 1 .. 4 lanes");
  {
    const int rc = cc_db_query_wait(db);
    if (rc != CC_OK) return rc;
  }
  HIPCHK(hipSetDevice(db->device));
  for (int i = 0; i < n; i++) {
    const int rc = lane_alloc(db, db->lane[i]);  // stream, events and scratch of a lane that was not in use so far
    if (rc != CC_OK) return rc;
  }
  db->n_lanes = n;
  db->next_lane = 0;
  return CC_OK;
}

int cc_db_size(const cc_db *db) { return db ? db->n_scans : 0; }
int cc_db_knn_stride(const cc_db *db) { return db ? db->kmax : 0; }

void cc_packed_sizes(size_t *hot_bytes, size_t *feat_bytes) {
  if (hot_bytes) *hot_bytes = sizeof(cc_hot_desc_t);
  if (feat_bytes) *feat_bytes = sizeof(cc_gmm_feat);
}
const void *cc_db_hot_ptr(const cc_db *db) { return db ? db->d_hot : nullptr; }
const void *cc_db_feat_ptr(const cc_db *db) { return db ? db->d_feat : nullptr; }

int cc_db_bucket_state(const cc_db *db, int32_t *tree_sizes, float *ranges) {
  if (!db || !tree_sizes || !ranges) return set_err(CC_EINVAL, "cc_db_bucket_state: bad argument");
  for (int l = 0; l < CC_NQLEV; l++) {
    for (int b = 0; b < 6; b++) tree_sizes[l * 6 + b] = (l < db->cfg.n_q_levels) ? (int32_t)db->book[l].b[b].tree.size() : 0;
    for (int b = 0; b < 7; b++) ranges[l * 7 + b] = (l < db->cfg.n_q_levels) ? db->book[l].ranges[b] : 0.f;
  }
  return CC_OK;
}

// calls that change or reuse what chunks in flight read collect them first
#define DB_DRAIN(db)                            \
  {                                             \
    const int drc_ = cc_db_query_wait(db);      \
    if (drc_ != CC_OK) return drc_;             \
  }
#define DB_POISON_CHK(db, what) \
  if ((db)->poisoned) return set_err(CC_EHIP, what ": the database handle is in a failed state (an earlier HIP error); destroy it")

// DYNAMIC_THRES=1 of the reference (contour_db.h:439-466, 566-574): recorded per chunk when it is submitted, so chunks in
// flight keep the mode they were launched with
int cc_db_set_dynamic_thres(cc_db *db, int on) {
  if (!db || (on != 0 && on != 1)) return set_err(CC_EINVAL, "cc_db_set_dynamic_thres: db must be valid and on 0 or 1");
  DB_POISON_CHK(db, "cc_db_set_dynamic_thres");
  if (on) {
    HIPCHK(hipSetDevice(db->device));
    for (auto &ln : db->lane)
      if (ln.d_qmeta) {
        const int rc = lane_alloc_dyn(ln);
        if (rc != CC_OK) return rc;
      }
  }
  db->dyn_thres = on;
  return CC_OK;
}

// the buckets' indexed intervals at the current epoch, filed with the epoch's other history
static void push_idx_state(cc_db *db) {
  bool all = true;
  for (int l = 0; l < db->cfg.n_q_levels; l++) all = all && db->book[l].fullyIndexed();
  if (all) {
    db->idx_slot.push_back(-1);
    return;
  }
  cc_db::IdxRec r;
  for (int l = 0; l < CC_NQLEV; l++) {
    r.full[l] = (l >= db->cfg.n_q_levels || db->book[l].fullyIndexed()) ? 1 : 0;
    for (int b = 0; b < 6; b++) {
      r.iv[l][2 * b] = l < db->cfg.n_q_levels ? db->book[l].b[b].idx_lo : 0.f;
      r.iv[l][2 * b + 1] = l < db->cfg.n_q_levels ? db->book[l].b[b].idx_hi : 0.f;
    }
  }
  db->idx_slot.push_back((int)db->idx_store.size());
  db->idx_store.push_back(r);
}

// full descriptors -> the two per-scan records the DB keeps (and ships)
int cc_pack_scans(cc_ctx *ctx, const cc_scan_desc_t *d_desc, int n, void *d_hot_out, void *d_feat_out, void *stream_) {
  if (!ctx || !d_desc || n < 0 || !d_hot_out || !d_feat_out) return set_err(CC_EINVAL, "cc_pack_scans: bad argument");
  if (n == 0) return CC_OK;
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(cc_k_pack_hot, dim3(n), dim3(256), 0, stream, d_desc, n, (cc_hot_desc_t *)d_hot_out, (int *)nullptr, (int *)nullptr,
                     (const cc_query_meta *)nullptr, (cc_query_meta *)nullptr, (const int *)nullptr);
  hipLaunchKernelGGL(cc_k_gmm_prep, dim3(n), dim3(CC_GMM_PREP_BLOCK), 0, stream, d_desc, n, (cc_gmm_feat *)d_feat_out, (const int *)nullptr);
  HIPCHK(hipGetLastError());
  return CC_OK;
}

static int fetch_lite(cc_db *db, const cc_hot_desc_t *d_hot, int n, ScanLite *h_out, hipStream_t stream) {
  if (n <= CC_ZC_MAX) {  // a handful of scans (the per-scan loop brings one): the kernel writes into pinned host memory, no copy command
    hipLaunchKernelGGL(cc_k_extract, dim3(n), dim3(64), 0, stream, d_hot, n, db->cfg.n_q_levels, db->cfg.q_levels[0], db->cfg.q_levels[1],
                       db->cfg.q_levels[2], db->h_lite_zc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    memcpy(h_out, db->h_lite_zc, sizeof(ScanLite) * (size_t)n);
    return CC_OK;
  }
  for (int b0 = 0; b0 < n; b0 += 4096) {
    const int nb = n - b0 < 4096 ? n - b0 : 4096;
    hipLaunchKernelGGL(cc_k_extract, dim3(nb), dim3(64), 0, stream, d_hot + b0, nb, db->cfg.n_q_levels, db->cfg.q_levels[0],
                       db->cfg.q_levels[1], db->cfg.q_levels[2], db->d_lite);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out + b0, db->d_lite, sizeof(ScanLite) * nb, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  return CC_OK;
}

// Failure behaviour: everything that can fail before the host bookkeeping is touched (copies, the per-scan extraction)
// runs first and leaves the handle unchanged on error; the bookkeeping itself cannot fail; a HIP error after it marks
// the handle as failed (host and device views would disagree), and every later call on it returns CC_EHIP.
//
// Device side of an append: ONE upload (the new keys' (scan, anchor) entries + the changed tails of the activation
// arrays, staged in pinned memory), the keys themselves are taken from the hot records already in the DB's array, then
// per layer the merge into the other buffer of the sorted view.  Query chunks still in flight keep reading the buffer
// they were submitted with: a buffer is only rewritten after the chunks that read it have finished (a device-side wait on
// their completion events, the host does not drain the lanes), everything else an append touches is append-only, and an
// activation epoch only ever changes from "never" to an epoch later than any query in flight.
static int add_settle(cc_db *db) {  // the previous append's uploads have left the pinned staging buffer
  if (db->add_pending) {
    db->add_pending = false;
    HIPCHK(hipEventSynchronize(db->add_done));
  }
  return CC_OK;
}

static int add_scans_device_part(cc_db *db, const int *old_n, const std::vector<int> *ent, const int *act_lo, hipStream_t stream) {
  const int nql = db->cfg.n_q_levels;
  // Consecutive appends queued on DIFFERENT streams (the class mirror mixes its loop stream with the null stream of the
  // host-side appends): this append reads the sorted view the previous one's merge writes, so it waits for it on the
  // device.  On the same stream the order is the stream's own and nothing is queued.
  if (db->add_done && db->add_stream != stream) HIPCHK(hipStreamWaitEvent(stream, db->add_done, 0));
  cc_kappend_params AP;
  size_t used = 0;
  size_t need = 0;  // the staging buffer holds the new entries plus the changed activation tails: checked BEFORE anything is copied into it
  for (int l = 0; l < nql; l++) need += ent[l].size() + (act_lo[l] < db->n_keys[l] ? (size_t)(db->n_keys[l] - act_lo[l]) : 0);
  if (need > db->add_cap) return set_err(CC_ECAPACITY, "cc_db_add_scans: staging buffer too small");  // cannot happen (2 * cap_k per layer)
  // A small append (the per-scan loop brings one scan) is staged in the next buffer of a ring and waits for the append that
  // used THAT buffer, CC_NSTAGE appends ago; a large one uses the big buffer and waits for the append before it.
  const bool small_stage = need <= (size_t)CC_ZC_MAX * 64;
  int *h_stage = db->h_add;
  int stage_slot = -1;
  if (small_stage) {
    stage_slot = db->add_small_next;
    db->add_small_next = (stage_slot + 1) % CC_NSTAGE;
    if (db->add_small_busy[stage_slot]) {
      HIPCHK(hipEventSynchronize(db->add_small_ev[stage_slot]));
      db->add_small_busy[stage_slot] = false;
    }
    h_stage = db->h_add_small[stage_slot];
  } else {
    const int src_ = add_settle(db);
    if (src_ != CC_OK) return src_;
  }
  AP.cap_k = db->cap_k;
  for (int l = 0; l < CC_NQLEV; l++) {
    AP.keys[l] = db->d_keys[l];
    AP.kgidx[l] = db->d_kgidx[l];
    AP.kseq[l] = db->d_kseq[l];
    AP.n_old[l] = l < nql ? old_n[l] : 0;
    AP.q_levels[l] = l < nql ? db->cfg.q_levels[l] : 1;
    AP.first[l] = (int)used;
    if (l < nql && !ent[l].empty()) {
      memcpy(h_stage + used, ent[l].data(), sizeof(int) * ent[l].size());
      used += ent[l].size();
    }
  }
  AP.first[CC_NQLEV] = (int)used;
  const size_t n_ent = used;
  size_t act_off[CC_NQLEV] = {0, 0, 0};
  for (int l = 0; l < nql; l++) {
    act_off[l] = used;
    if (act_lo[l] < db->n_keys[l]) {
      const size_t cnt = (size_t)(db->n_keys[l] - act_lo[l]);
      memcpy(h_stage + used, db->book[l].active_from.data() + act_lo[l], sizeof(int) * cnt);
      used += cnt;
    }
  }
  // a small append (the per-scan loop brings one scan): cc_k_keys_append reads the staging buffer where it lies (pinned host
  // memory) and files the activation tails as well -- no copy command in the chain
  const bool zc = used <= (size_t)CC_ZC_MAX * 64;
  size_t act_total = 0;
  for (int l = 0; l < CC_NQLEV; l++) {
    AP.act_first[l] = (int)act_total;
    AP.act_dst[l] = nullptr;
    AP.act_src[l] = 0;
    if (zc && l < nql && act_lo[l] < db->n_keys[l]) {
      AP.act_dst[l] = db->d_kactive[l] + act_lo[l];
      AP.act_src[l] = (int)act_off[l];
      act_total += (size_t)(db->n_keys[l] - act_lo[l]);
    }
  }
  AP.act_first[CC_NQLEV] = (int)act_total;
  if (n_ent > 0 || act_total > 0) {
    if (!zc) HIPCHK(hipMemcpyAsync(db->d_add, h_stage, sizeof(int) * n_ent, hipMemcpyHostToDevice, stream));
    const size_t nthr = n_ent > act_total ? n_ent : act_total;
    hipLaunchKernelGGL(cc_k_keys_append, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, stream, AP, (const cc_hot_desc_t *)db->d_hot,
                       zc ? (const int *)h_stage : (const int *)db->d_add);
  }
  cc_ksort_params SP;
  SP.cap_k = db->cap_k;
  SP.n_layers = nql;
  int longest = 0;
  bool any_new = false, any_bulk = false;
  for (int l = 0; l < CC_NQLEV; l++) {
    const bool on = l < nql;
    const int nn = on ? db->n_keys[l] - old_n[l] : 0;
    // activation epochs: only the ids from the lowest one that changed (new keys included) are uploaded -- keys become
    // searchable roughly in insertion order, so this is a short tail of the array, not all of it
    if (!zc && on && act_lo[l] < db->n_keys[l])
      HIPCHK(hipMemcpyAsync(db->d_kactive[l] + act_lo[l], h_stage + act_off[l], sizeof(int) * (size_t)(db->n_keys[l] - act_lo[l]),
                            hipMemcpyHostToDevice, stream));
    const int cur = db->scur[l], nxt = nn > 0 ? (cur + 1) % CC_NVIEW : cur;
    if (nn > 0)
      for (auto &ln : db->lane)  // chunks in flight that still read the buffer about to be rewritten
        if (ln.busy && ln.view[l] == nxt) HIPCHK(hipStreamWaitEvent(stream, ln.fin, 0));
    SP.keys[l] = db->d_keys[l];
    SP.s_old[l] = db->d_skeys[l][cur];
    SP.sid_old[l] = db->d_sid[l][cur];
    SP.s_new[l] = db->d_skeys[l][nxt];
    SP.sid_new[l] = db->d_sid[l][nxt];
    SP.newpos[l] = db->d_newpos[l];
    SP.newsorted0[l] = db->d_newsorted0[l];
    SP.act[l] = db->d_kactive[l];
    SP.sact_new[l] = db->d_sact[l][nxt];
    SP.n_old[l] = on ? old_n[l] : 0;
    SP.m[l] = nn;
    if (on && db->n_keys[l] > longest) longest = db->n_keys[l];
    any_new = any_new || nn > 0;
    any_bulk = any_bulk || nn > CC_KSORT_LDS;
  }
  SP.blocks_per_layer = (longest + 255) / 256;
  // merge the new keys into the layers' sorted views (into the other buffer), activation epochs in sorted order
  if (any_bulk)
    for (int l = 0; l < nql; l++)
      if (SP.m[l] > CC_KSORT_LDS)
        hipLaunchKernelGGL(cc_k_ksort_new, dim3((SP.m[l] + 255) / 256), dim3(256), 0, stream, (const float *)db->d_keys[l], db->cap_k, old_n[l],
                           SP.m[l], (const float *)SP.s_old[l], db->d_newpos[l], db->d_newsorted0[l]);
  if (any_new) hipLaunchKernelGGL(cc_k_ksort_new_lds, dim3(nql), dim3(1024), 0, stream, SP);
  if (longest > 0) {
    if (any_new) hipLaunchKernelGGL(cc_k_ksort_merge, dim3(nql * SP.blocks_per_layer), dim3(256), 0, stream, SP);
    hipLaunchKernelGGL(cc_k_ksort_act, dim3(nql * SP.blocks_per_layer), dim3(256), 0, stream, SP);
  }
  HIPCHK(hipGetLastError());
  for (int l = 0; l < nql; l++)
    if (SP.m[l] > 0) db->scur[l] = (db->scur[l] + 1) % CC_NVIEW;
  // not waited for: the chunks submitted from now on wait for this event on the device, the host before it touches the
  // pinned staging buffer again (add_settle)
  if (!db->add_done) HIPCHK(hipEventCreateWithFlags(&db->add_done, hipEventDisableTiming));
  HIPCHK(hipEventRecord(db->add_done, stream));
  db->add_stream = stream;
  if (stage_slot >= 0) {
    HIPCHK(hipEventRecord(db->add_small_ev[stage_slot], stream));
    db->add_small_busy[stage_slot] = true;
  } else {
    db->add_pending = true;
  }
  return CC_OK;
}

// rows [n_scans, n_scans + n) of d_hot / d_feat have been filled on `stream`: bookkeeping + key upload + commit
static int add_scans_commit(cc_db *db, int n, const double *h_ts, const int32_t *h_seed, hipStream_t stream,
                            const ScanLite *lite_ready = nullptr /*the scans' keys, already on the host (prepared batch)*/) {
  std::vector<ScanLite> lite_new((size_t)n);
  const auto tm0 = std::chrono::steady_clock::now();
  int rc = CC_OK;
  if (lite_ready)
    std::copy(lite_ready, lite_ready + n, lite_new.begin());
  else
    rc = fetch_lite(db, db->d_hot + db->n_scans, n, lite_new.data(), stream);
  if (rc != CC_OK) return rc;
  const auto tm1 = std::chrono::steady_clock::now();
  for (int i = 0; i < n; i++)
    if (lite_new[i].flags & (CC_DESC_INEXACT_COMPONENTS | CC_DESC_INEXACT_KEYS))
      return set_err(CC_ECAPACITY, "cc_db_add_scans: a scan's descriptor is flagged inexact (CC_DESC_INEXACT_*: it exceeded a capacity of the "
                                   "contour kernel); nothing was added");
  // ---- host bookkeeping (cannot fail)
  const size_t base = db->lite.size();
  db->lite.insert(db->lite.end(), lite_new.begin(), lite_new.end());
  const int nql = db->cfg.n_q_levels;
  int old_n[CC_NQLEV], act_lo[CC_NQLEV];
  std::vector<int> ent[CC_NQLEV];  // per new key: scan index << 3 | anchor
  for (int l = 0; l < nql; l++) act_lo[l] = old_n[l] = db->n_keys[l];
  for (int i = 0; i < n; i++) {
    const ScanLite &sl = db->lite[base + i];
    const int gidx = db->n_scans + i;
    // ContourDB::addScan (contour_db.h:814-824)
    for (int l = 0; l < nql; l++) {
      for (int seq = 0; seq < CC_NPIV; seq++) {
        const float *k = sl.keys[l][seq];
        float sum = 0.f;
        for (int d = 0; d < CC_KEY_DIM; d++) sum += k[d];
        if (sum != 0) {
          const int id = db->n_keys[l]++;
          cchost::LayerBook &bk = db->book[l];
          bk.key0.push_back(k[0]);
          bk.active_from.push_back(INT_MAX);
          bk.pushBuffer(id, k[0], h_ts[i]);
          ent[l].push_back((gidx << 3) | seq);
        }
      }
    }
    // ContourDB::pushAndBalance (contour_db.h:827-843)
    const int idx_t1 = cchost::balance_index(h_seed[i]);
    const int epoch_after = gidx + 1;
    std::array<float, CC_NQLEV * 7> rr;
    std::array<int, CC_NQLEV> kk;
    for (int l = 0; l < CC_NQLEV; l++) {
      kk[l] = 0;
      for (int b = 0; b < 7; b++) rr[l * 7 + b] = 0.f;
    }
    for (int l = 0; l < nql; l++) {
      cchost::LayerBook &bk = db->book[l];
      bk.newly_active.clear();
      bk.rebuild(idx_t1, h_ts[i]);
      for (int id : bk.newly_active) {
        bk.active_from[id] = epoch_after;
        if (id < act_lo[l]) act_lo[l] = id;
      }
      for (int b = 0; b < 7; b++) rr[l * 7 + b] = bk.ranges[b];
      kk[l] = db->n_keys[l];
    }
    db->ranges_hist.push_back(rr);
    db->nkeys_hist.push_back(kk);
    push_idx_state(db);
  }
  // ---- uploads and the sorted-view merge
  const auto tm2 = std::chrono::steady_clock::now();
  rc = add_scans_device_part(db, old_n, ent, act_lo, stream);
  if (db->add_timers) {
    const auto tm3 = std::chrono::steady_clock::now();
    db->add_s[0] += std::chrono::duration<double>(tm1 - tm0).count();
    db->add_s[1] += std::chrono::duration<double>(tm2 - tm1).count();
    db->add_s[2] += std::chrono::duration<double>(tm3 - tm2).count();
    db->add_calls++;
    db->add_scans_n += n;
  }
  if (rc != CC_OK) {
    db->poisoned = true;
    return rc;
  }
  db->n_scans += n;
  return CC_OK;
}

int cc_db_add_scans(cc_db *db, const cc_scan_desc_t *d_desc, int n, const double *h_ts, const int32_t *h_seed, void *stream_) {
  if (!db || !d_desc || n < 0 || !h_ts || !h_seed) return set_err(CC_EINVAL, "cc_db_add_scans: bad argument");
  DB_POISON_CHK(db, "cc_db_add_scans");
  if (db->n_scans + n > db->cap) return set_err(CC_ECAPACITY, "cc_db_add_scans: database capacity exceeded");
  if (n == 0) return CC_OK;
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(db->device));
  if (db->prep_cnt > 0) {  // a prepared batch: its records are packed (or being packed) and its keys are on their way
    cc_db::Prepared &pp = db->prep[db->prep_head];
    if (pp.d_desc != d_desc || pp.n != n || pp.row0 != db->n_scans)
      return set_err(CC_EINVAL, "cc_db_add_scans: batches prepared with cc_db_add_scans_prepare must be added first, in the order they were prepared");
    HIPCHK(hipStreamWaitEvent(stream, pp.ev, 0));  // the append's kernels on `stream` read the packed rows
    HIPCHK(hipEventSynchronize(pp.ev));            // the keys have arrived
    db->prep_head = (db->prep_head + 1) % cc_db::PREP_SLOTS;
    db->prep_cnt--;
    db->n_prepared -= n;
    const int rc_p = add_scans_commit(db, n, h_ts, h_seed, stream, pp.h_lite);
    if (rc_p != CC_OK && db->prep_cnt > 0) {
      // nothing was added, so a batch prepared behind this one sits in rows that are no longer the next ones: it is
      // dropped with it (its copy is waited for: the slot will be reused) and has to be prepared again
      cc_db::Prepared &nx = db->prep[db->prep_head];
      hipEventSynchronize(nx.ev);
      db->prep_cnt = 0;
      db->n_prepared = 0;
    }
    return rc_p;
  }
  // rows >= n_scans of d_hot / d_feat are scratch until n_scans moves
  int rc = cc_pack_scans(db->ctx, d_desc, n, db->d_hot + db->n_scans, db->d_feat + db->n_scans, stream_);
  if (rc != CC_OK) return rc;
  return add_scans_commit(db, n, h_ts, h_seed, stream);
}

// The first half of cc_db_add_scans, asynchronously: pack the batch's records into the rows they will occupy, extract the
// keys the host bookkeeping needs and start their copy to the host -- all queued on `stream`, nothing is waited for and
// the database does not change.  cc_db_add_scans on the same (d_desc, n) later only waits for the copy.
int cc_db_add_scans_prepare(cc_db *db, const cc_scan_desc_t *d_desc, int n, void *stream_) {
  if (!db || !d_desc || n < 1 || n > cc_db::PREP_MAX) return set_err(CC_EINVAL, "cc_db_add_scans_prepare: bad argument (1..4096 scans)");
  DB_POISON_CHK(db, "cc_db_add_scans_prepare");
  if (db->prep_cnt >= cc_db::PREP_SLOTS) return set_err(CC_EINVAL, "cc_db_add_scans_prepare: two prepared batches are already waiting to be added");
  if (db->n_scans + db->n_prepared + n > db->cap) return set_err(CC_ECAPACITY, "cc_db_add_scans_prepare: database capacity exceeded");
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(db->device));
  cc_db::Prepared &pp = db->prep[(db->prep_head + db->prep_cnt) % cc_db::PREP_SLOTS];
  if (!pp.ev) {
    HIPCHK(hipEventCreateWithFlags(&pp.ev, hipEventDisableTiming));
    HIPCHK(hipMalloc(&pp.d_lite, sizeof(ScanLite) * cc_db::PREP_MAX));
    HIPCHK(hipHostMalloc((void **)&pp.h_lite, sizeof(ScanLite) * cc_db::PREP_MAX, hipHostMallocDefault));
  }
  const int row0 = db->n_scans + db->n_prepared;
  int rc = cc_pack_scans(db->ctx, d_desc, n, db->d_hot + row0, db->d_feat + row0, stream_);
  if (rc != CC_OK) return rc;
  hipLaunchKernelGGL(cc_k_extract, dim3(n), dim3(64), 0, stream, (const cc_hot_desc_t *)(db->d_hot + row0), n, db->cfg.n_q_levels,
                     db->cfg.q_levels[0], db->cfg.q_levels[1], db->cfg.q_levels[2], pp.d_lite);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(pp.h_lite, pp.d_lite, sizeof(ScanLite) * (size_t)n, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipEventRecord(pp.ev, stream));
  pp.d_desc = d_desc;
  pp.n = n;
  pp.row0 = row0;
  db->prep_cnt++;
  db->n_prepared += n;
  return CC_OK;
}

// Scans that arrive already packed (cc_pack_scans on this or another GPU, e.g. the far side of an all-gather).
int cc_db_add_packed(cc_db *db, const void *d_hot, const void *d_feat, int n, const double *h_ts, const int32_t *h_seed, void *stream_) {
  if (!db || !d_hot || !d_feat || n < 0 || !h_ts || !h_seed) return set_err(CC_EINVAL, "cc_db_add_packed: bad argument");
  DB_POISON_CHK(db, "cc_db_add_packed");
  if (db->prep_cnt > 0) return set_err(CC_EINVAL, "cc_db_add_packed: batches prepared with cc_db_add_scans_prepare are waiting to be added");
  if (db->n_scans + n > db->cap) return set_err(CC_ECAPACITY, "cc_db_add_packed: database capacity exceeded");
  if (n == 0) return CC_OK;
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(db->device));
  HIPCHK(hipMemcpyAsync(db->d_hot + db->n_scans, d_hot, sizeof(cc_hot_desc_t) * (size_t)n, hipMemcpyDeviceToDevice, stream));
  HIPCHK(hipMemcpyAsync(db->d_feat + db->n_scans, d_feat, sizeof(cc_gmm_feat) * (size_t)n, hipMemcpyDeviceToDevice, stream));
  return add_scans_commit(db, n, h_ts, h_seed, stream);
}

// CandidateManager ctor CHECKs (contour_db.h:365-367)
static bool thres_strict_smaller(const cc_score_t *lb, const cc_score_t *ub) {
  return lb->i_ovlp_sum < ub->i_ovlp_sum && lb->i_ovlp_max_one < ub->i_ovlp_max_one && lb->i_in_ang_rng < ub->i_in_ang_rng &&
         lb->i_indiv_sim < ub->i_indiv_sim && lb->i_orie_sim < ub->i_orie_sim && lb->correlation < ub->correlation &&
         lb->area_perc < ub->area_perc && lb->neg_est_dist < ub->neg_est_dist;
}

// hot records and correlation inputs of a chunk's query scans + the per-chunk list heads
// d_sel: verify chunks -- query record i of the chunk is built from d_q[d_sel[i]] (else from d_q[i])
static int launch_query_prep(cc_db *db, cc_qlane &ln, const cc_scan_desc_t *d_q, int nb, bool meta_from_host = false, const int *d_sel = nullptr) {
  (void)db;
  hipStream_t ls = ln.stream;
  hipLaunchKernelGGL(cc_k_pack_hot, dim3(nb), dim3(256), 0, ls, d_q, nb, ln.d_qhot, ln.d_heads, ln.d_pass_cnt,
                     meta_from_host ? (const cc_query_meta *)ln.h_meta : (const cc_query_meta *)nullptr, ln.d_qmeta, d_sel);
  hipLaunchKernelGGL(cc_k_gmm_prep, dim3(nb), dim3(CC_GMM_PREP_BLOCK), 0, ls, d_q, nb, ln.d_qfeat, d_sel);
  HIPCHK(hipGetLastError());
  return CC_OK;
}

// The same for a chunk whose query scans exist as packed records (k_prep_packed.h): record i of the chunk is a copy of record
// d_sel[i] of the source; the heads, the pass counters and a small chunk's epoch records as above.
struct cc_rec_src {  // a cc_packed_src_t, resolved (packed_resolve)
  const cc_hot_desc_t *hot;
  const cc_gmm_feat *feat;
  int n_rec;
};
static int launch_prep_packed(cc_qlane &ln, const cc_rec_src &rs, const int *d_sel, int nb, bool meta_from_host) {
  hipLaunchKernelGGL(cc_k_prep_packed, dim3(nb * CC_PREPP_SPLIT), dim3(CC_PREPP_BLOCK), 0, ln.stream, rs.hot, rs.feat, d_sel, nb, ln.d_qhot, ln.d_qfeat,
                     ln.d_heads, CC_N_HEADS, ln.d_pass_cnt, meta_from_host ? (const cc_query_meta *)ln.h_meta : (const cc_query_meta *)nullptr, ln.d_qmeta);
  HIPCHK(hipGetLastError());
  return CC_OK;
}
// The refusals every *_submit_packed form shares, worded with the entry point's name, and the source it reads.
static int packed_resolve(const char *fn, const cc_db *db, const cc_packed_src_t *src, cc_rec_src *out) {
  if (!db) return set_err(CC_EINVAL, (std::string(fn) + ": bad argument").c_str());
  if (!src) return set_err(CC_EINVAL, (std::string(fn) + ": src must be given").c_str());
  if ((src->d_hot == nullptr) != (src->d_feat == nullptr)) return set_err(CC_EINVAL, (std::string(fn) + ": d_hot and d_feat are given together, or both NULL (the database's own records)").c_str());
  if (!src->d_hot) {  // the database's committed rows
    *out = cc_rec_src{db->d_hot, db->d_feat, db->n_scans};
    return CC_OK;
  }
  if (src->n_rec < 1) return set_err(CC_EINVAL, (std::string(fn) + ": n_rec must be positive").c_str());
  if (((uintptr_t)src->d_hot | (uintptr_t)src->d_feat) & 15) return set_err(CC_EINVAL, (std::string(fn) + ": the record arrays must be 16-byte aligned").c_str());
  *out = cc_rec_src{(const cc_hot_desc_t *)src->d_hot, (const cc_gmm_feat *)src->d_feat, src->n_rec};
  return CC_OK;
}
// rank NULL: the plain call; h_detail NULL: the ranked one; both: the ranked-detail one
static int packed_modes(const char *fn, const cc_rank_out_t *rank, const cc_ranked_detail_t *h_detail) {
  if (!rank && h_detail) return set_err(CC_EINVAL, (std::string(fn) + ": h_detail comes with rank").c_str());
  return rank ? want_ranked(fn, rank, h_detail, false) : CC_OK;
}

static cc_check_params make_check_params(const cc_db *db, const cc_score_t *lb) {
  cc_check_params CP;
  CP.sim = db->cfg.cont_sim;
  CP.lb = *lb;
  for (int i = 0; i < 3; i++) {
    CP.size_class[i] = db->tune.a_class[i];
    CP.cstl_class[i] = db->tune.b2_class[i];
  }
  return CP;
}

// initial correlation of every problem on the lane's list (cc_k_merge / cc_k_pose_problems filled it)
static void launch_gmm_init(cc_db *db, cc_qlane &ln) {
  hipLaunchKernelGGL(cc_k_gmm_init, dim3(db->tune.gmm), dim3(64), 0, ln.stream, (const cc_gmm_problem *)ln.d_prob, (const int *)ln.d_prob_list,
                     (const int *)ln.d_nprob, (const cc_gmm_feat *)ln.d_qfeat, (const cc_gmm_feat *)db->d_feat, ln.d_gres,
                     cc_gmm_code_pool{ln.d_codes, ln.code_cap, ln.head(CC_HD_CODES), ln.head(CC_HD_POOL), ln.pool_cap});
}
// L-BFGS on the problems cc_k_select / cc_k_pose_select listed: the 16-lane instance takes its own list and the in-between list
// from the front, the 64-lane instance its class lists and the in-between list from the back.  corr_bar: the selection's bar.
static void launch_refine(cc_db *db, cc_qlane &ln, float corr_bar) {
  hipStream_t ls = ln.stream;
  const int *n16 = ln.head(CC_HD_NSEL16), *n64 = ln.head(CC_HD_NSEL64), *n_mid = ln.head(CC_HD_NMID), *mid = ln.sel(CC_SEL_MID);
  hipLaunchKernelGGL(cc_k_gmm_refine<16>, dim3(db->tune.gmm), dim3(64), 0, ls, (const cc_gmm_problem *)ln.d_prob, n16, (const int *)ln.sel(CC_SEL_16), n_mid, mid, n64,
                     (const cc_gmm_feat *)ln.d_qfeat, (const cc_gmm_feat *)db->d_feat, corr_bar, ln.d_pool, ln.pool_cap, (const int *)ln.d_pool_off, ln.d_gres,
                     (const unsigned *)ln.d_codes, (const int *)nullptr, (const int *)nullptr, 0);
  hipLaunchKernelGGL(cc_k_gmm_refine<64>, dim3(db->tune.gmm64), dim3(64), 0, ls, (const cc_gmm_problem *)ln.d_prob, n64, (const int *)ln.sel(CC_SEL_64), n_mid, mid, n16,
                     (const cc_gmm_feat *)ln.d_qfeat, (const cc_gmm_feat *)db->d_feat, corr_bar, ln.d_pool, ln.pool_cap, (const int *)ln.d_pool_off, ln.d_gres,
                     (const unsigned *)ln.d_codes, (const int *)ln.sel(CC_SEL_CLS), (const int *)ln.head(CC_HD_CLS), ln.prob_cap);
}

// The launches of one chunk after the retrieval: checks (K4), proposal merge (K4b), correlation (K5), selection (K6).
// ev: profiling events [2..5] or nullptr; d_scores: per-check gate scores (hint flow) or nullptr.
// km: hits per search in ln.d_hits (db->kmax for queries; CC_KNN_MAX for the hint flow): picks the kernel instances.
static int launch_scoring_chain(cc_db *db, cc_qlane &ln, int nb, const cc_check_params &CP, const cc_score_t *lb, const cc_score_t *ub,
                                int max_fine_opt, hipEvent_t *ev, int *d_scores, bool zc /*results and counters straight into the lane's pinned host buffers*/,
                                int km, int max_ret = 0 /*> 0: a ranked chunk (cc_k_final_r writes the lists to the lane's rank buffer)*/,
                                bool detail = false /*with max_ret > 0: cc_k_gmm_hess behind the refinement, cc_k_final_rd writes the detail rows as well*/,
                                const cc_match_out_t *match = nullptr /*with max_ret > 0: the matched merge instance, cc_k_match_emit behind cc_k_final_r*/) {
  hipStream_t ls = ln.stream;
  const bool lg = km != CC_KNN_MAX;
  // dynamic thresholds (the mode at submission): the stages leave their scores in the pass records, cc_k_check_dyn replays the
  // checks in order, cc_k_select<true> / cc_k_final<true> the post bars
  const bool dyn = db->dyn_thres != 0;
  if (dyn && !ln.d_tidy) return set_err(CC_EHIP, "launch_scoring_chain: the lane has no dynamic-threshold buffers");
  if (match && (dyn || max_ret <= 0 || !ln.d_mrec)) return set_err(CC_EHIP, "launch_scoring_chain: a matched chain is a ranked one on static thresholds with the lane's match buffers");
  cc_pass_rec *const dpass = dyn ? ln.d_pass : nullptr;
  unsigned char *const dok = dyn ? ln.d_pass_ok : nullptr;
  const cc_hot_desc_t *qh = ln.d_qhot, *dh = db->d_hot;
  const size_t n_slots = (size_t)nb * CC_CHK_STRIDE_K(km);
  hipLaunchKernelGGL(lg ? cc_k_check_a_l : cc_k_check_a, dim3((unsigned)((n_slots + CC_CHKA_BLOCK - 1) / CC_CHKA_BLOCK)), dim3(CC_CHKA_BLOCK), 0, ls, CP, qh, dh, nb, (const cc_knn_hit_t *)ln.d_hits,
                     (const int *)ln.d_hit_cnt, ln.d_items, ln.d_cnt, ln.d_pass_ok, ln.d_pass_cnt, d_scores, dpass);
  hipLaunchKernelGGL((lg ? cc_k_check_b1_l<CC_PP_SMALL, false> : cc_k_check_b1<CC_PP_SMALL, false>), dim3(db->tune.b1), dim3(64), 0, ls, CP, qh, dh, (const cc_chk_item *)ln.d_items,
                     ln.d_redo, ln.d_cnt, ln.d_cstl, ln.d_pass_cnt, d_scores, dpass, dok);
  hipLaunchKernelGGL((lg ? cc_k_check_b1_l<CC_PP_MAX, true> : cc_k_check_b1<CC_PP_MAX, true>), dim3((db->tune.b1 + 3) / 4), dim3(64), 0, ls, CP, qh, dh, (const cc_chk_item *)ln.d_items, ln.d_redo,
                     ln.d_cnt, ln.d_cstl, ln.d_pass_cnt, d_scores, dpass, dok);
  hipLaunchKernelGGL(cc_k_compact_cstl, dim3((unsigned)((n_slots + CC_CHKA_BLOCK - 1) / CC_CHKA_BLOCK)), dim3(CC_CHKA_BLOCK), 0, ls, CP, (const cc_cstl_item *)ln.d_cstl, ln.d_cnt,
                     ln.d_cstl_idx);
  hipLaunchKernelGGL(lg ? cc_k_check_b2_l : cc_k_check_b2, dim3(db->tune.b2), dim3(64), 0, ls, CP, qh, dh, (const cc_cstl_item *)ln.d_cstl,
                     (const int *)ln.d_cstl_idx, (const int *)ln.d_cnt, ln.d_pass, ln.d_pass_ok, ln.d_pass_cnt, d_scores, dyn ? 1 : 0);
  hipLaunchKernelGGL(lg ? cc_k_check_c_l : cc_k_check_c, dim3((db->tune.b2 + 3) / 4), dim3(256), 0, ls, (const cc_cstl_item *)ln.d_cstl,
                     (const int *)ln.d_cstl_idx, (const int *)ln.d_cnt, ln.d_pass, (const unsigned char *)ln.d_pass_ok);
  if (dyn)
    hipLaunchKernelGGL(lg ? cc_k_check_dyn_l : cc_k_check_dyn, dim3(nb), dim3(64), 0, ls, nb, *lb, *ub, (const cc_pass_rec *)ln.d_pass, ln.d_pass_ok, ln.d_pass_cnt,
                       d_scores);
  if (ev) HIPCHK(hipEventRecord(ev[2], ls));
  if (match)  // the matched instance replaces the plain one; a chain without `match` launches what it always launched
    hipLaunchKernelGGL(lg ? cc_k_merge_lm : cc_k_merge_m, dim3(nb), dim3(CC_MERGE_BLOCK), 0, ls, nb, *lb, db->n_row, db->n_col, qh, dh, (const cc_pass_rec *)ln.d_pass,
                       (const unsigned char *)ln.d_pass_ok, (const int *)ln.d_pass_cnt, ln.d_cands, ln.d_qstate, ln.d_prob, ln.d_prob_list,
                       ln.d_nprob, ln.d_mrec);
  else
    hipLaunchKernelGGL(lg ? cc_k_merge_l : cc_k_merge, dim3(nb), dim3(CC_MERGE_BLOCK), 0, ls, nb, *lb, db->n_row, db->n_col, qh, dh, (const cc_pass_rec *)ln.d_pass,
                       (const unsigned char *)ln.d_pass_ok, (const int *)ln.d_pass_cnt, ln.d_cands, ln.d_qstate, ln.d_prob, ln.d_prob_list,
                       ln.d_nprob, dyn ? ln.d_cpost : (cc_cand_post *)nullptr);
  if (ev) HIPCHK(hipEventRecord(ev[3], ls));
  // initial correlation of every candidate; the candidates fineOptimize would refine; L-BFGS on those only
  launch_gmm_init(db, ln);
  hipLaunchKernelGGL(lg ? (dyn ? cc_k_select_l<true> : cc_k_select_l<false>) : (dyn ? cc_k_select<true> : cc_k_select<false>), dim3(nb), dim3(64), 0, ls, nb, lb->correlation, max_fine_opt,
                     (const cc_cand_out *)ln.d_cands, (const cc_qstate *)ln.d_qstate, (const cc_gmm_result *)ln.d_gres, ln.d_sel, ln.prob_cap,
                     ln.head(CC_HD_NSEL16), ln.head(CC_HD_NMID), (const unsigned short *)db->d_perm_tab, ln.sel(CC_SEL_CLS), ln.head(CC_HD_CLS),
                     ln.head(CC_HD_POOL), ln.d_pool_off, (const cc_cand_post *)ln.d_cpost, ln.d_tidy, *lb, *ub);
  launch_refine(db, ln, lb->correlation);
  if (detail)  // the curvature at the refined poses, over the three lists cc_k_select filled (only in chains that asked for it)
    hipLaunchKernelGGL(cc_k_gmm_hess, dim3(db->tune.gmm64), dim3(64), 0, ls, (const cc_gmm_problem *)ln.d_prob, (const int *)ln.head(CC_HD_NSEL16), (const int *)ln.sel(CC_SEL_16),
                       (const int *)ln.head(CC_HD_NMID), (const int *)ln.sel(CC_SEL_MID), (const int *)ln.head(CC_HD_NSEL64),
                       (const int *)ln.sel(CC_SEL_CLS), (const int *)ln.head(CC_HD_CLS), ln.prob_cap, (const cc_gmm_feat *)ln.d_qfeat,
                       (const cc_gmm_feat *)db->d_feat, (const cc_gmm_result *)ln.d_gres, (const unsigned *)ln.d_codes, ln.d_hess);
  if (ev) HIPCHK(hipEventRecord(ev[4], ls));
  if (max_ret > 0 && detail) {
    hipLaunchKernelGGL(lg ? (dyn ? cc_k_final_rdl<true> : cc_k_final_rdl<false>) : (dyn ? cc_k_final_rd<true> : cc_k_final_rd<false>), dim3(nb), dim3(64), 0, ls, nb, lb->correlation, max_fine_opt,
                       (const cc_cand_out *)ln.d_cands, (const cc_qstate *)ln.d_qstate, (const cc_gmm_result *)ln.d_gres, (const int *)ln.d_pass_cnt,
                       (const int *)ln.d_hit_cnt, qh, zc ? ln.h_results : ln.d_results, (const unsigned short *)db->d_perm_tab, (const int *)ln.d_nprob,
                       zc ? ln.h_nprob : (int *)nullptr, (const unsigned char *)ln.d_tidy, zc ? ln.h_rank : ln.d_rank, max_ret, (const cc_gmm_hess *)ln.d_hess,
                       (const cc_gmm_problem *)ln.d_prob, zc ? ln.h_detail : ln.d_detail);
  } else if (max_ret > 0) {  // the ranked instance replaces the plain one; a chain without `rank` launches what it always launched
    hipLaunchKernelGGL(lg ? (dyn ? cc_k_final_rl<true> : cc_k_final_rl<false>) : (dyn ? cc_k_final_r<true> : cc_k_final_r<false>), dim3(nb), dim3(64), 0, ls, nb, lb->correlation, max_fine_opt,
                       (const cc_cand_out *)ln.d_cands, (const cc_qstate *)ln.d_qstate, (const cc_gmm_result *)ln.d_gres, (const int *)ln.d_pass_cnt,
                       (const int *)ln.d_hit_cnt, qh, zc ? ln.h_results : ln.d_results, (const unsigned short *)db->d_perm_tab, (const int *)ln.d_nprob,
                       zc ? ln.h_nprob : (int *)nullptr, (const unsigned char *)ln.d_tidy, zc ? ln.h_rank : ln.d_rank, max_ret);
  } else {
    hipLaunchKernelGGL(lg ? (dyn ? cc_k_final_l<true> : cc_k_final_l<false>) : (dyn ? cc_k_final<true> : cc_k_final<false>), dim3(nb), dim3(64), 0, ls, nb, lb->correlation, max_fine_opt,
                       (const cc_cand_out *)ln.d_cands, (const cc_qstate *)ln.d_qstate, (const cc_gmm_result *)ln.d_gres, (const int *)ln.d_pass_cnt,
                       (const int *)ln.d_hit_cnt, qh, zc ? ln.h_results : ln.d_results, (const unsigned short *)db->d_perm_tab, (const int *)ln.d_nprob,
                       zc ? ln.h_nprob : (int *)nullptr, (const unsigned char *)ln.d_tidy);
  }
  if (match)  // the rows of the list cc_k_final_r* just wrote (small chunks: read from and written to the pinned buffers)
    hipLaunchKernelGGL(lg ? cc_k_match_emit_l : cc_k_match_emit, dim3(nb), dim3(64), 0, ls, nb, max_ret, max_fine_opt, match->inlier_px,
                       (const cc_query_result_t *)(zc ? ln.h_results : ln.d_results), (const cc_ranked_cand_t *)(zc ? ln.h_rank : ln.d_rank),
                       (const cc_cand_out *)ln.d_cands, (const cc_qstate *)ln.d_qstate, (const cc_match_rec *)ln.d_mrec, qh, dh,
                       zc ? ln.h_match : ln.d_match);
  if (ev) HIPCHK(hipEventRecord(ev[5], ls));
  HIPCHK(hipGetLastError());
  return CC_OK;
}

// capacity checks on what a finished chunk brought back: the pools of the correlation (every kind of chunk) ...
static int pool_status(const cc_qlane &ln) {
  if (ln.h_nprob[CC_HD_POOL] > ln.pool_cap) return set_err(CC_ECAPACITY, "the pair pool (or the pair-code pool) of the correlation refinement overflowed");
  return CC_OK;
}
// ... and the flags of a query or verify chunk's results
static int chunk_status(const cc_qlane &ln, int nb) {
  const int prc = pool_status(ln);
  if (prc != CC_OK) return prc;
  for (int i = 0; i < nb; i++)
    if (ln.h_results[i].flags)
      return set_err(CC_ECAPACITY, "a query met an internal capacity of the scoring kernels (cc_query_result_t.flags, CC_QF_*): "
                                   "its result may differ from the reference's");
  return CC_OK;
}
// a profiled chunk's stage times (knn | check | merge | gmm | final), those of `stages` (bit k: pev[k] .. pev[k + 1])
static void add_stage_times(cc_db *db, const cc_qlane &ln, unsigned stages) {
  for (int k = 0; k < 5; k++) {
    float t = 0.f;
    if (stages >> k & 1) hipEventElapsedTime(&t, ln.pev[k], ln.pev[k + 1]);
    db->ms_acc[k] += t;
  }
  db->launch_w += (double)ln.nb;  // profiled queries
}

// a finished pose chunk: its rows to rows [b0, b0 + nb) of the caller's arrays, its stage times, its capacity flags
static int pose_finish(cc_db *db, cc_qlane &ln) {
  ln.pose = false;
  const int nb = ln.nb, nt = ln.pose_ntry;
  const cc_pose_result_t *rows = (const cc_pose_result_t *)ln.h_pout;
  const double *tr = (const double *)(rows + nb);
  memcpy(ln.pose_res + ln.b0, rows, sizeof(cc_pose_result_t) * (size_t)nb);
  if (nt > 0) memcpy(ln.pose_try + (size_t)ln.b0 * nt, tr, sizeof(double) * (size_t)nb * nt);
  if (ln.pose_curv) memcpy(ln.pose_curv + ln.b0, tr + (size_t)nb * nt, sizeof(cc_pose_curv_t) * (size_t)nb);
  if (ln.profiled) add_stage_times(db, ln, 1u << 0 | 1u << 3 | 1u << 4);  // problems | - | - | correlation (with the try poses and the curvature) | rows
  const int prc = pool_status(ln);
  if (prc != CC_OK) return prc;
  for (int i = 0; i < nb; i++)
    if (rows[i].flags & ~CC_PF_REFINED)
      return set_err(CC_ECAPACITY, "a pose item met an internal capacity of the correlation (cc_pose_result_t.flags, CC_QF_*): "
                                   "its result may differ from the reference's");
  return CC_OK;
}

// collect a lane's chunk: wait for its chain, copy its results to where its submitter wanted them, check its capacity flags
static int lane_finish(cc_db *db, cc_qlane &ln) {
  if (!ln.busy) return CC_OK;
  ln.busy = false;
  HIPCHK(hipStreamSynchronize(ln.stream));
  if (ln.pose) return pose_finish(db, ln);
  memcpy(ln.h_dst + ln.b0, ln.h_results, sizeof(cc_query_result_t) * ln.nb);
  if (ln.rank_dst.h_cands) rank_deliver(ln, ln.rank_dst, ln.b0, ln.nb, ln.rank_mfo);
  if (ln.detail_dst)
    memcpy(ln.detail_dst + (size_t)ln.b0 * ln.rank_dst.max_ret, ln.h_detail, sizeof(cc_ranked_detail_t) * (size_t)ln.nb * ln.rank_dst.max_ret);
  if (ln.match_dst)
    memcpy(ln.match_dst + (size_t)ln.b0 * ln.rank_dst.max_ret, ln.h_match, sizeof(cc_ranked_match_t) * (size_t)ln.nb * ln.rank_dst.max_ret);
  if (ln.profiled) add_stage_times(db, ln, 0x1Fu);
  return chunk_status(ln, ln.nb);
}

static void lane_abort(cc_db *db, cc_qlane &ln) {
  if (ln.stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ln.stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {  // a caller's capture that reached the lane through the event waits
      hipGraph_t g = nullptr;
      if (hipStreamEndCapture(ln.stream, &g) == hipSuccess && g) hipGraphDestroy(g);
      (void)hipGetLastError();
    }
  }
  if (ln.stream) hipStreamSynchronize(ln.stream);
  ln.busy = false;
  ln.pose = false;
  db->poisoned = true;
}

// Collects every chunk still in flight (cc_db_query_submit).  Returns the first error any of them raised.
int cc_db_query_wait(cc_db *db) {
  if (!db) return set_err(CC_EINVAL, "cc_db_query_wait: bad argument");
  HIPCHK(hipSetDevice(db->device));
  int rc = CC_OK;
  for (auto &ln : db->lane) {
    const int r2 = lane_finish(db, ln);
    if (rc == CC_OK) rc = r2;
  }
  return rc;
}

// Collects only the chunks that write into [h_res, h_res + n): the caller waits for ITS answer, later submissions stay in
// flight (cc_db_query_wait would wait for the newest chain as well).  Nothing in flight there: CC_OK at once.
int cc_db_query_collect(cc_db *db, const cc_query_result_t *h_res, int n) {
  if (!db || !h_res || n < 1) return set_err(CC_EINVAL, "cc_db_query_collect: bad argument");
  HIPCHK(hipSetDevice(db->device));
  int rc = CC_OK;
  for (auto &ln : db->lane) {
    if (!ln.busy || ln.pose) continue;  // (a pose chunk has no cc_query_result_t rows: cc_db_query_wait collects it)
    const cc_query_result_t *lo = ln.h_dst + ln.b0, *hi = lo + ln.nb;
    if (hi <= h_res || lo >= h_res + n) continue;
    const int r2 = lane_finish(db, ln);
    if (rc == CC_OK) rc = r2;
  }
  return rc;
}

// A synchronous call = the submit + the wait -- also after an error: nothing may stay in flight behind a synchronous call.
static int run_sync(cc_db *db, const std::function<int()> &submit) {
  if (db) db->sync_call = true;
  const int rc = submit();
  if (db) db->sync_call = false;
  const int r2 = db ? cc_db_query_wait(db) : CC_OK;
  return rc != CC_OK ? rc : r2;
}

// ---- the chunk driver of the query, verify and pose submits ----
struct cc_chunk {  // one chunk, as the driver hands it to the steps of a plan
  cc_qlane &ln;
  int b0, nb;      // items [b0, b0 + nb) of the call
  // a chunk of a few queries (the per-scan loop brings one): the searches read the epoch records from the lane's pinned
  // host buffer (cc_k_pack_hot brings them over) and cc_k_final writes the results there -- three copy commands less in a
  // chain of ~15 short kernels
  bool zc;
  hipEvent_t *ev;  // the lane's stage events [0..5] when the chunk is profiled, or nullptr
};
struct cc_prep_src {  // what the prep stage makes a chunk's query records from
  const cc_scan_desc_t *d_q;  // descriptors: launch_query_prep builds the records (nullptr with `rec`)
  bool meta_from_host;
  const int *d_sel;
  const cc_rec_src *rec = nullptr;  // packed records (the *_submit_packed forms): launch_prep_packed copies record d_sel[i]
};
// What a submit does of its own, in the order the driver calls it.  The steps from `upload` on return a CC_* code with the
// message set (HIPCHK for their HIP calls).
struct cc_chunk_plan {
  std::function<int(cc_qlane &, int, int)> alloc;                // the lane's on-demand buffers the chunk (items [b0, b0 + nb)) needs
  std::function<void(const cc_chunk &)> stage;                   // fill the lane's pinned staging from the caller's arrays
  std::function<int(const cc_chunk &, cc_prep_src &)> upload;    // the copies in front of the prep kernels, and what those read
  std::function<int(const cc_chunk &)> head;                     // what stands in the place of the retrieval (stage ev[0] .. ev[1])
  std::function<int(const cc_chunk &)> body;                     // the rest of the chain
  std::function<int(const cc_chunk &)> copy_back;                // chunks above CC_ZC_MAX: the results to the lane's pinned buffers
  std::function<void(const cc_chunk &)> note;                    // where lane_finish delivers the chunk
};

// One chunk's chain, queued on its lane's stream.  Whatever fails in here -- a HIP call (HIPCHK) or a step of the plan
// (LANE_CHK: its own CC_* code and message) -- fails with part of the chain queued: submit_chunks drains the lane.
static int queue_chunk(cc_db *db, hipStream_t stream, const cc_chunk_plan &plan, const cc_chunk &c) {
#define LANE_CHK(step)               \
  do {                               \
    const int rc_ = (step);          \
    if (rc_ != CC_OK) return rc_;    \
  } while (0)
  cc_qlane &ln = c.ln;
  hipStream_t ls = ln.stream;
  hipEvent_t *ev = c.ev;
  cc_prep_src src{nullptr, false, nullptr};
  LANE_CHK(plan.upload(c, src));
  if (src.rec) LANE_CHK(launch_prep_packed(ln, *src.rec, src.d_sel, c.nb, src.meta_from_host));
  else LANE_CHK(launch_query_prep(db, ln, src.d_q, c.nb, src.meta_from_host, src.d_sel));
  // the caller's stream goes on once the descriptors (the records) have been read
  HIPCHK(hipEventRecord(ln.prep, ls));
  HIPCHK(hipStreamWaitEvent(stream, ln.prep, 0));
  if (ev) HIPCHK(hipEventRecord(ev[0], ls));
  LANE_CHK(plan.head(c));
  if (ev) HIPCHK(hipEventRecord(ev[1], ls));
  LANE_CHK(plan.body(c));
  if (!c.zc) LANE_CHK(plan.copy_back(c));
  HIPCHK(hipEventRecord(ln.fin, ls));
#undef LANE_CHK
  return CC_OK;
}

// The batch is cut into chunks of <= QB items; chunk c runs as one chain of launches on the next lane's stream, so
// n_lanes chunks are in flight at a time -- of this batch or of the one submitted before it: a lane's previous chunk is
// collected only when the lane is needed again, so the tail of one batch's chains overlaps the head of the next one's.
// The lanes start after everything queued on the caller's stream so far; the caller's stream continues once the
// query descriptors have been read (d_qdesc may then be overwritten).
static int submit_chunks(cc_db *db, int n, hipStream_t stream, const cc_chunk_plan &plan) {
  hipEvent_t e_start = db->lane[0].done;
  HIPCHK(hipEventRecord(e_start, stream));
  for (int i = 0; i < db->n_lanes; i++) {
    HIPCHK(hipStreamWaitEvent(db->lane[i].stream, e_start, 0));
    if (db->add_done) HIPCHK(hipStreamWaitEvent(db->lane[i].stream, db->add_done, 0));  // an append queued on another stream
  }
  // chunk size: a batch is cut so that every lane gets a chunk -- except a streamed submit of QB queries or more, which
  // goes out in chunks of QB: the next batch takes the next lane, and a chain of 1 024 queries is cheaper than two of 512
  // (+2 % on the bench).  Smaller streamed batches stay cut per lane: whole, they would sit one per lane, several
  // batches deep, and an append in between has to wait for the chunks that still read the view buffer it rewrites
  // (measured on the online loop with 512-scan sub-batches and four lanes: 188 k against 265 k scans/s).
  // (a large-k database's lanes take qb_max = 256 items)
  int qb = (((n + db->n_lanes - 1) / db->n_lanes) + 63) / 64 * 64;
  if (!db->sync_call && n >= db->qb_max) qb = db->qb_max;
  qb = qb > db->tune.chunk ? db->tune.chunk : qb;  // (tune.chunk <= qb_max)
  for (int b0 = 0; b0 < n; b0 += qb) {
    const int nb = n - b0 < qb ? n - b0 : qb;
    cc_qlane &ln = db->lane[db->next_lane];
    db->next_lane = (db->next_lane + 1) % db->n_lanes;
    int rc = lane_finish(db, ln);
    if (rc == CC_OK) rc = plan.alloc(ln, b0, nb);  // before anything of the chunk is queued (a lane whose earlier allocation failed tries again)
    if (rc != CC_OK) return rc;
    cc_chunk c{ln, b0, nb, nb <= CC_ZC_MAX, nullptr};
    plan.stage(c);
    ln.profiled = db->prof && (db->prof_tick++ % db->prof_every) == 0;
    c.ev = ln.profiled ? ln.pev : nullptr;
    rc = queue_chunk(db, stream, plan, c);
    if (rc != CC_OK) {
      // the lane is drained (its pinned staging buffers must not be reused under copies still in flight) and the handle is
      // marked failed, as the appends do
      lane_abort(db, ln);
      return rc;
    }
    for (int l = 0; l < CC_NQLEV; l++) ln.view[l] = db->scur[l];  // (a verify or pose chunk reads no sorted view: nothing for an append to wait for beyond this)
    ln.busy = true;
    ln.b0 = b0;
    ln.nb = nb;
    plan.note(c);
  }
  return CC_OK;
}

// query and verify chunks: the lane's on-demand buffers of the chain's modes ...
static int lane_alloc_modes(cc_db *db, cc_qlane &ln, const cc_rank_out_t *rank, const cc_ranked_detail_t *detail, const cc_match_out_t *match = nullptr) {
  int rc = db->dyn_thres ? lane_alloc_dyn(ln) : CC_OK;
  if (rc == CC_OK && rank) rc = lane_alloc_rank(ln);
  if (rc == CC_OK && detail) rc = lane_alloc_detail(ln);
  if (rc == CC_OK && match) rc = lane_alloc_match(ln);
  return rc;
}
// ... what launch_scoring_chain left on the device, to the lane's pinned buffers ...
static int results_copy_back(const cc_chunk &c, const cc_rank_out_t *rank, const cc_ranked_detail_t *detail, const cc_match_out_t *match = nullptr) {
  cc_qlane &ln = c.ln;
  hipStream_t ls = ln.stream;
  const int nb = c.nb;
  HIPCHK(hipMemcpyAsync(ln.h_results, ln.d_results, sizeof(cc_query_result_t) * nb, hipMemcpyDeviceToHost, ls));
  HIPCHK(hipMemcpyAsync(ln.h_nprob, ln.d_nprob, sizeof(int) * 4, hipMemcpyDeviceToHost, ls));
  if (rank) HIPCHK(hipMemcpyAsync(ln.h_rank, ln.d_rank, sizeof(cc_ranked_cand_t) * (size_t)nb * rank->max_ret, hipMemcpyDeviceToHost, ls));
  if (detail) HIPCHK(hipMemcpyAsync(ln.h_detail, ln.d_detail, sizeof(cc_ranked_detail_t) * (size_t)nb * rank->max_ret, hipMemcpyDeviceToHost, ls));
  if (match) HIPCHK(hipMemcpyAsync(ln.h_match, ln.d_match, sizeof(cc_ranked_match_t) * (size_t)nb * rank->max_ret, hipMemcpyDeviceToHost, ls));
  return CC_OK;
}
// ... and where lane_finish delivers them
static void results_note(cc_qlane &ln, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *detail, int max_fine_opt,
                         const cc_match_out_t *match = nullptr) {
  ln.h_dst = h_res;
  ln.match_dst = match ? match->h_match : nullptr;
  ln.rank_dst = rank ? *rank : cc_rank_out_t{nullptr, nullptr, 0, 0};
  ln.detail_dst = detail;
  ln.rank_mfo = max_fine_opt;
}

// The refusals of a masked query (cc_db_query_submit_masked / cc_db_query_batch_host_masked), before anything is queued.
static int mask_validate(const cc_db *db, const cc_scan_mask_t *mask, int nq, const int32_t *h_epoch) {
  if (!mask->bits || (!mask->h_row && nq > 0)) return set_err(CC_EINVAL, "cc_db_query_submit_masked: the mask's bits and h_row must be given");
  if (mask->n_rows < 1 || mask->row_words < 1) return set_err(CC_EINVAL, "cc_db_query_submit_masked: the mask needs n_rows >= 1 and row_words >= 1");
  if (db->dyn_thres)
    return set_err(CC_EINVAL, "cc_db_query_submit_masked: masked queries are not supported in dynamic-threshold mode (cc_db_set_dynamic_thres)");
  int max_epoch = 0;
  for (int i = 0; i < nq; i++) {
    const int r = mask->h_row[i];
    if (r < -1 || r >= mask->n_rows) return set_err(CC_EINVAL, "cc_db_query_submit_masked: h_row names a row outside [-1, n_rows)");
    if (r >= 0 && h_epoch[i] > max_epoch) max_epoch = h_epoch[i];
  }
  if ((long long)32 * mask->row_words < (long long)max_epoch)
    return set_err(CC_EINVAL, "cc_db_query_submit_masked: 32 * row_words is smaller than the largest epoch of a query that names a row");
  return CC_OK;
}

// The refusals of a listed query (cc_db_query_submit_listed / cc_db_query_batch_host_listed, include/cont2_amd_lists.h), before
// anything is queued.  Everything is host memory, so everything is checked.
// fn: the entry point's name, for the messages.
static int lists_validate(const char *fn, const cc_db *db, const cc_scan_lists_t *lists, int nq) {
  auto bad = [&](const char *what) { return set_err(CC_EINVAL, (std::string(fn) + ": " + what).c_str()); };
  if (!lists->h_off || (!lists->h_row && nq > 0)) return bad("the lists' h_off and h_row must be given");
  if (lists->n_lists < 1) return bad("the lists need n_lists >= 1");
  if (db->dyn_thres)
    return bad("listed queries are not supported in dynamic-threshold mode (cc_db_set_dynamic_thres)");
  if (lists->h_off[0] != 0) return bad("h_off must start at 0");
  for (int r = 0; r < lists->n_lists; r++) {
    const int lo = lists->h_off[r], hi = lists->h_off[r + 1];
    if (hi < lo) return bad("h_off must be non-decreasing");
    if (hi - lo > CC_LIST_SCANS_MAX)
      return bad("a list is longer than CC_LIST_SCANS_MAX = 1024 scans (use the mask form, cc_db_query_submit_masked, for larger sets)");
    if (hi > lo && !lists->h_idx) return bad("h_idx must be given");
  }
  for (int r = 0; r < lists->n_lists; r++) {  // (the offsets are in order: nothing beyond h_idx[h_off[n_lists]) is read)
    const int lo = lists->h_off[r], hi = lists->h_off[r + 1];
    for (int j = lo; j < hi; j++) {
      const int g = lists->h_idx[j];
      if (g < 0 || g >= db->n_scans) return bad("a list names a scan outside [0, cc_db_size)");
      if (j > lo && g <= lists->h_idx[j - 1]) return bad("a list must be strictly increasing");
    }
  }
  for (int i = 0; i < nq; i++)
    if (lists->h_row[i] < -1 || lists->h_row[i] >= lists->n_lists)
      return bad("h_row names a list outside [-1, n_lists)");
  return CC_OK;
}

// rank: where the chunks' ranked lists go (the *_ranked entry points, validated there), or nullptr: the plain call
static int query_submit_impl(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                             const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream_,
                             const cc_rank_out_t *rank,
    cc_ranked_detail_t *detail /*with rank: where the chunks' detail rows go, or nullptr*/,
                             const cc_rec_src *rec = nullptr /*the queries are packed records (then d_qdesc is nullptr) ...*/,
                             const int32_t *h_rec = nullptr /*... query i is record h_rec[i] of them, or nullptr: record i*/,
                             const cc_scan_mask_t *mask = nullptr /*the scans that may answer (bits: device), or nullptr: all of them*/,
                             const cc_match_out_t *match = nullptr /*with rank: where the chunks' match rows go (validated by the entry point), or nullptr*/,
                             const cc_scan_lists_t *lists = nullptr /*per query a list of the scans that may answer (host; never with mask), or nullptr*/,
                             bool lists_checked = false /*the entry point has run lists_validate under its own name*/) {
  if (!db || (!d_qdesc && !rec) || nq < 0 || !h_epoch || !lb || !ub || !h_res) return set_err(CC_EINVAL, "cc_db_query_batch: bad argument");
  DB_POISON_CHK(db, "cc_db_query_batch");
  if (mask) {
    const int vrc = mask_validate(db, mask, nq, h_epoch);
    if (vrc != CC_OK) return vrc;
  }
  if (!thres_strict_smaller(lb, ub)) return set_err(CC_EINVAL, "cc_db_query_batch: thresholds must satisfy lb.strictSmaller(ub)");
  HIPCHK(hipSetDevice(db->device));
  const int NS = CC_NQLEV * CC_NPIV;
  const int nql = db->cfg.n_q_levels;
  cc_knn_params KP;
  for (int l = 0; l < CC_NQLEV; l++) {
    KP.skeys[l] = db->d_skeys[l][db->scur[l]];
    KP.sid[l] = db->d_sid[l][db->scur[l]];
    KP.sact[l] = db->d_sact[l][db->scur[l]];
    KP.n_sorted[l] = db->n_keys[l];
    KP.kgidx[l] = db->d_kgidx[l];
    KP.kseq[l] = db->d_kseq[l];
    KP.q_levels[l] = db->cfg.q_levels[l];
  }
  KP.cap_k = db->cap_k;
  KP.nnk = db->cfg.nnk;
  KP.n_q_levels = nql;
  const cc_check_params CP = make_check_params(db, lb);
  for (int i = 0; i < nq; i++)
    if (h_epoch[i] < 0 || h_epoch[i] > db->n_scans) return set_err(CC_EINVAL, "cc_db_query_batch: epoch out of range");
  if (rec)
    for (int i = 0; i < nq; i++) {
      const int r = h_rec ? h_rec[i] : i;
      if (r < 0 || r >= rec->n_rec) return set_err(CC_EINVAL, "cc_db_query_submit_packed: record index outside the source");
    }
  if (lists && !lists_checked) {  // (after what the call without lists refuses)
    const int vrc = lists_validate("cc_db_query_submit_listed", db, lists, nq);
    if (vrc != CC_OK) return vrc;
  }
  bool chunk_vis = false;  // some query of the chunk sees a bucket whose kd-tree does not index its whole range
  bool chunk_masked = false;  // some query of the chunk names a row of the mask
  // listed calls: 0 no query of the chunk names a list, 1 some do (the list retrieval runs behind the unrestricted one), 2 all do
  int chunk_listed = 0;
  size_t chunk_lent = 0;      // the chunk's staged entries
  bool lent_zc = false;       // ... are read from the pinned buffer where they lie (a small chunk with a few of them)
  // the distinct lists of a chunk, in the order its queries first name them: each is staged once
  std::vector<int> list_at(lists ? (size_t)lists->n_lists : 0, -1);  // where list r starts among the chunk's entries, or -1
  std::vector<int> list_used;
  int lists_b0 = -1, lists_nb = 0;  // the chunk the two describe (plan.alloc fills them, plan.stage finds them)
  size_t lists_n = 0;
  auto chunk_lists = [&](int b0, int nb) -> size_t {  // fills the two for items [b0, b0 + nb) -> the entries they take
    if (b0 == lists_b0 && nb == lists_nb) return lists_n;
    for (int r : list_used) list_at[r] = -1;
    list_used.clear();
    size_t n = 0;
    for (int i = 0; i < nb; i++) {
      const int r = lists->h_row[b0 + i];
      if (r < 0 || list_at[r] >= 0) continue;
      list_at[r] = (int)n;  // (<= QB * CC_LIST_SCANS_MAX = 2^20)
      list_used.push_back(r);
      n += (size_t)(lists->h_off[r + 1] - lists->h_off[r]);
    }
    lists_b0 = b0;
    lists_nb = nb;
    lists_n = n;
    return n;
  };
  cc_chunk_plan plan;
  plan.alloc = [&](cc_qlane &ln, int b0, int nb) -> int {
    int rc = rec ? lane_alloc_verify(ln) : CC_OK;  // (the record selector of a packed chunk goes where a verify chunk's does)
    if (rc == CC_OK && mask) rc = lane_alloc_mask(ln);
    if (rc == CC_OK && lists) rc = lane_alloc_lists(ln, chunk_lists(b0, nb));
    return rc != CC_OK ? rc : lane_alloc_modes(db, ln, rank, detail, match);
  };
  plan.stage = [&](const cc_chunk &c) {  // the queries' epoch records
    cc_query_meta *h_meta = c.ln.h_meta;
    chunk_vis = false;
    chunk_masked = false;
    chunk_listed = 0;
    if (lists) {  // per query where its list lies among the chunk's entries; per listed scan its key ids of the three layers
      chunk_lent = chunk_lists(c.b0, c.nb);
      int n_named = 0;
      for (int i = 0; i < c.nb; i++) {
        const int r = lists->h_row[c.b0 + i];
        c.ln.h_lrow[i] = r < 0 ? make_int2(-1, 0) : make_int2(list_at[r], lists->h_off[r + 1] - lists->h_off[r]);
        n_named += r >= 0;
      }
      for (int r : list_used) {
        cc_list_ent *e = c.ln.h_lent + list_at[r];
        for (int j = lists->h_off[r]; j < lists->h_off[r + 1]; j++, e++) {
          const int g = lists->h_idx[j];
          e->g = g;
          for (int l = 0; l < CC_NQLEV; l++)  // scan g's keys of layer l: ids [nkeys_hist[g][l], nkeys_hist[g + 1][l]), in anchor order
            e->w[l] = (db->nkeys_hist[g][l] << 3) | (db->nkeys_hist[g + 1][l] - db->nkeys_hist[g][l]);
        }
      }
      chunk_listed = n_named == 0 ? 0 : n_named == c.nb ? 2 : 1;
    }
    if (mask)
      for (int i = 0; i < c.nb; i++) {
        const int r = mask->h_row[c.b0 + i];
        c.ln.h_mrow[i] = r;
        chunk_masked = chunk_masked || r >= 0;
      }
    if (rec)
      for (int i = 0; i < c.nb; i++) c.ln.h_vin[i] = h_rec ? h_rec[c.b0 + i] : c.b0 + i;
    for (int i = 0; i < c.nb; i++) {
      const int e = h_epoch[c.b0 + i];
      chunk_vis = chunk_vis || db->idx_slot[e] >= 0;
      h_meta[i].epoch = e;
      for (int l = 0; l < CC_NQLEV; l++) {
        h_meta[i].n_keys[l] = db->nkeys_hist[e][l];
        for (int b = 0; b < 7; b++) h_meta[i].ranges[l][b] = db->ranges_hist[e][l * 7 + b];
      }
      const int is_ = db->idx_slot[e];
      for (int l = 0; l < CC_NQLEV; l++) {
        h_meta[i].idx_full[l] = is_ < 0 ? 1 : db->idx_store[is_].full[l];
        for (int b = 0; b < 12; b++) h_meta[i].idx[l][b] = is_ < 0 ? 0.f : db->idx_store[is_].iv[l][b];
      }
    }
  };
  plan.upload = [&](const cc_chunk &c, cc_prep_src &src) -> int {  // (small chunks: cc_k_pack_hot fills d_qmeta from the pinned buffer)
    cc_qlane &ln = c.ln;
    if (!c.zc) HIPCHK(hipMemcpyAsync(ln.d_qmeta, ln.h_meta, sizeof(cc_query_meta) * c.nb, hipMemcpyHostToDevice, ln.stream));
    // (small chunks: the masked walk reads its rows from the pinned buffer, as cc_k_prep_packed reads the selector below)
    if (chunk_masked && !c.zc) HIPCHK(hipMemcpyAsync(ln.d_mrow, ln.h_mrow, sizeof(int) * c.nb, hipMemcpyHostToDevice, ln.stream));
    if (chunk_listed) {  // (small chunks: the list retrieval reads its rows from the pinned buffer as well, and a few entries with them)
      if (!c.zc) HIPCHK(hipMemcpyAsync(ln.d_lrow, ln.h_lrow, sizeof(cc_list_row) * c.nb, hipMemcpyHostToDevice, ln.stream));
      lent_zc = c.zc && chunk_lent <= CC_LIST_ZC_ENT;
      if (!lent_zc && chunk_lent > 0) HIPCHK(hipMemcpyAsync(ln.d_lent, ln.h_lent, sizeof(cc_list_ent) * chunk_lent, hipMemcpyHostToDevice, ln.stream));
    }
    if (rec) {  // (small chunks: cc_k_prep_packed reads the selector from the pinned buffer too)
      if (!c.zc) HIPCHK(hipMemcpyAsync(ln.d_vin, ln.h_vin, sizeof(int) * c.nb, hipMemcpyHostToDevice, ln.stream));
      src = cc_prep_src{nullptr, c.zc, c.zc ? ln.h_vin : ln.d_vin, rec};
      return CC_OK;
    }
    src = cc_prep_src{d_qdesc + c.b0, c.zc, nullptr};
    return CC_OK;
  };
  plan.head = [&](const cc_chunk &c) -> int {  // the retrieval
    cc_qlane &ln = c.ln;
    hipStream_t ls = ln.stream;
    const int nb = c.nb;
    const cc_query_meta *qmeta_dev = ln.d_qmeta;
    // The list retrieval (k_knn_list.h): alone when every query of the chunk names a list, else behind the chunk's unrestricted
    // retrieval, whose hit tables it overwrites for the queries that do.  It reads the layers by key id (d_keys, d_kactive,
    // d_kgidx, d_kseq), not the sorted view: everything there is append-only but the tails of d_kactive, where a later append
    // only ever replaces "never" by an epoch later than any query in flight; the lanes' wait for add_done (submit_chunks) orders
    // these reads behind the append that covers the chunk's largest epoch, as it orders the view's.
    auto launch_list = [&]() -> int {
      db->knn_chunks_listed[chunk_listed == 2 ? 0 : 1]++;
      cc_knn_list_params LP;
      for (int l = 0; l < CC_NQLEV; l++) {
        LP.keys[l] = db->d_keys[l];
        LP.act[l] = db->d_kactive[l];
      }
      const cc_list_row *qlist = c.zc ? ln.h_lrow : ln.d_lrow;
      const cc_list_ent *ent = lent_zc ? ln.h_lent : ln.d_lent;
      if (db->kmax != CC_KNN_MAX)
        hipLaunchKernelGGL(chunk_vis ? cc_k_knn_list_l<true> : cc_k_knn_list_l<false>, dim3(nb * NS), dim3(64), 0, ls, KP, LP,
                           (const cc_hot_desc_t *)ln.d_qhot, qmeta_dev, ln.d_hits, ln.d_hit_cnt, qlist, ent);
      else
        hipLaunchKernelGGL(chunk_vis ? cc_k_knn_list<true> : cc_k_knn_list<false>, dim3(nb * NS), dim3(64), 0, ls, KP, LP,
                           (const cc_hot_desc_t *)ln.d_qhot, qmeta_dev, ln.d_hits, ln.d_hit_cnt, qlist, ent);
      return CC_OK;
    };
    if (chunk_listed == 2) return launch_list();
    int max_keys = 0;
    for (int l = 0; l < nql; l++) max_keys = db->n_keys[l] > max_keys ? db->n_keys[l] : max_keys;
    // (a large-k database always walks: the tiled search has no large-k instance)
    const bool tiled = db->kmax == CC_KNN_MAX && (db->tune.knn_mode == 2 || (db->tune.knn_mode == 1 && max_keys >= CC_KNN_TILE_MIN_KEYS));
    db->knn_chunks[chunk_masked ? 2 : tiled ? 1 : 0]++;
    if (chunk_masked) {  // a masked chunk always walks: the tiled search has no masked instance
      const int *qrow = c.zc ? ln.h_mrow : ln.d_mrow;
      if (db->kmax != CC_KNN_MAX)
        hipLaunchKernelGGL(chunk_vis ? cc_k_knn_lm<true> : cc_k_knn_lm<false>, dim3(nb * NS), dim3(64), 0, ls, KP, (const cc_hot_desc_t *)ln.d_qhot,
                           qmeta_dev, ln.d_hits, ln.d_hit_cnt, (const unsigned *)mask->bits, (int)mask->row_words, qrow);
      else
        hipLaunchKernelGGL(chunk_vis ? cc_k_knn_m<true> : cc_k_knn_m<false>, dim3(nb * NS), dim3(64), 0, ls, KP, (const cc_hot_desc_t *)ln.d_qhot,
                           qmeta_dev, ln.d_hits, ln.d_hit_cnt, (const unsigned *)mask->bits, (int)mask->row_words, qrow);
    } else if (tiled) {
      int *ord = ln.d_knn_order;
      for (int s0 = 0; s0 < nb; s0 += cc_db::KQB) {  // the search order of a sub-chunk is built in LDS (cc_k_knn_order)
        const int ns = nb - s0 < cc_db::KQB ? nb - s0 : cc_db::KQB;
        const cc_hot_desc_t *qh = ln.d_qhot + s0;
        const cc_query_meta *qm = qmeta_dev + s0;
        cc_knn_hit_t *hs = ln.d_hits + (size_t)s0 * NS * CC_KNN_MAX;
        int *hc = ln.d_hit_cnt + (size_t)s0 * NS;
        hipLaunchKernelGGL(cc_k_knn_order, dim3(nql), dim3(1024), CC_KNN_ORDER_LDS, ls, KP, qh, ns, ord, hc);
        hipLaunchKernelGGL(cc_k_knn_tile, dim3(nql * ns * CC_NPIV), dim3(64 * CC_KNN_TW), 0, ls, KP, qh, qm, ns, (const int *)ord, hs, hc);
      }
    } else if (db->kmax != CC_KNN_MAX) {
      hipLaunchKernelGGL(chunk_vis ? cc_k_knn_l<true> : cc_k_knn_l<false>, dim3(nb * NS), dim3(64), 0, ls, KP, (const cc_hot_desc_t *)ln.d_qhot,
                         qmeta_dev, ln.d_hits, ln.d_hit_cnt);
    } else {
      hipLaunchKernelGGL(chunk_vis ? cc_k_knn<true> : cc_k_knn<false>, dim3(nb * NS), dim3(64), 0, ls, KP, (const cc_hot_desc_t *)ln.d_qhot, qmeta_dev,
                         ln.d_hits, ln.d_hit_cnt);
    }
    return chunk_listed ? launch_list() : CC_OK;
  };
  plan.body = [&](const cc_chunk &c) -> int {
    cc_qlane &ln = c.ln;
    hipStream_t ls = ln.stream;
    const int nb = c.nb, b0 = c.b0;
    const int rc = launch_scoring_chain(db, ln, nb, CP, lb, ub, db->cfg.max_fine_opt, c.ev, nullptr, c.zc, db->kmax, rank ? rank->max_ret : 0, detail != nullptr, match);
    if (rc != CC_OK) return rc;
    if (d_knn) HIPCHK(hipMemcpyAsync(d_knn + (size_t)b0 * NS * db->kmax, ln.d_hits, sizeof(cc_knn_hit_t) * (size_t)nb * NS * db->kmax, hipMemcpyDeviceToDevice, ls));
    if (d_knn_cnt) HIPCHK(hipMemcpyAsync(d_knn_cnt + (size_t)b0 * NS, ln.d_hit_cnt, sizeof(int) * nb * NS, hipMemcpyDeviceToDevice, ls));
    return CC_OK;
  };
  plan.copy_back = [&](const cc_chunk &c) -> int { return results_copy_back(c, rank, detail, match); };
  plan.note = [&](const cc_chunk &c) { results_note(c.ln, h_res, rank, detail, db->cfg.max_fine_opt, match); };
  return submit_chunks(db, nq, (hipStream_t)stream_, plan);
}

int cc_db_query_submit(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                       const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream_) {
  return query_submit_impl(db, d_qdesc, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, nullptr, nullptr);
}
int cc_db_query_submit_ranked(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                              const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream_,
                              const cc_rank_out_t *rank) {
  const int vrc = want_ranked(__func__, rank, nullptr, false);
  if (vrc != CC_OK) return vrc;
  return query_submit_impl(db, d_qdesc, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, nullptr);
}
int cc_db_query_submit_ranked_detail(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                     const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream_, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  const int vrc = want_ranked(__func__, rank, h_detail, true);
  if (vrc != CC_OK) return vrc;
  return query_submit_impl(db, d_qdesc, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail);
}

int cc_db_query_batch(cc_db *db, const cc_scan_desc_t *d_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                      const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream_) {
  return run_sync(db, [&] { return cc_db_query_submit(db, d_qdesc, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_); });
}

static int stage_reserve(cc_db *db, int n) {
  if (n <= db->stage_cap) return CC_OK;
  hipFree(db->d_stage);
  db->d_stage = nullptr;
  db->stage_cap = 0;
  HIPCHK(hipMalloc(&db->d_stage, sizeof(cc_scan_desc_t) * (size_t)n));
  db->stage_cap = n;
  return CC_OK;
}

// Host-buffer variants of the two batched calls: one H2D copy of the descriptors, then the device path.
int cc_db_add_scans_host(cc_db *db, const cc_scan_desc_t *h_desc, int n, const double *h_ts, const int32_t *h_seed) {
  if (!db || !h_desc || n < 0 || !h_ts || !h_seed) return set_err(CC_EINVAL, "cc_db_add_scans_host: bad argument");
  if (n == 0) return CC_OK;
  HIPCHK(hipSetDevice(db->device));
  int rc = stage_reserve(db, n);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpy(db->d_stage, h_desc, sizeof(cc_scan_desc_t) * (size_t)n, hipMemcpyHostToDevice));
  return cc_db_add_scans(db, db->d_stage, n, h_ts, h_seed, nullptr);
}

// rank: as for query_submit_impl.  The ranked form refuses what the chain would refuse before the descriptors are staged.
static int query_batch_host_impl(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                 const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank,
    cc_ranked_detail_t *detail /*with rank: where the chunks' detail rows go, or nullptr*/) {
  if (!db || !h_qdesc || nq < 0 || !h_epoch || !h_res) return set_err(CC_EINVAL, "cc_db_query_batch_host: bad argument");
  if (rank) {
    if (!lb || !ub) return set_err(CC_EINVAL, "cc_db_query_batch_host_ranked: bad argument");
    if (!thres_strict_smaller(lb, ub)) return set_err(CC_EINVAL, "cc_db_query_batch_host_ranked: thresholds must satisfy lb.strictSmaller(ub)");
    for (int i = 0; i < nq; i++)
      if (h_epoch[i] < 0 || h_epoch[i] > db->n_scans) return set_err(CC_EINVAL, "cc_db_query_batch_host_ranked: epoch out of range");
  }
  if (nq == 0) return CC_OK;
  HIPCHK(hipSetDevice(db->device));
  int rc = stage_reserve(db, nq);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpy(db->d_stage, h_qdesc, sizeof(cc_scan_desc_t) * (size_t)nq, hipMemcpyHostToDevice));
  if (!rank) return cc_db_query_batch(db, db->d_stage, nq, h_epoch, lb, ub, h_res, nullptr, nullptr, nullptr);
  // cc_db_query_batch's body with the lists
  return run_sync(db, [&] { return query_submit_impl(db, db->d_stage, nq, h_epoch, lb, ub, h_res, nullptr, nullptr, nullptr, rank, detail); });
}
int cc_db_query_batch_host(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                           const cc_score_t *ub, cc_query_result_t *h_res) {
  return query_batch_host_impl(db, h_qdesc, nq, h_epoch, lb, ub, h_res, nullptr, nullptr);
}
int cc_db_query_batch_host_ranked(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                  const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank) {
  const int vrc = want_ranked(__func__, rank, nullptr, false);
  if (vrc != CC_OK) return vrc;
  return query_batch_host_impl(db, h_qdesc, nq, h_epoch, lb, ub, h_res, rank, nullptr);
}
int cc_db_query_batch_host_ranked_detail(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                         const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  const int vrc = want_ranked(__func__, rank, h_detail, true);
  if (vrc != CC_OK) return vrc;
  return query_batch_host_impl(db, h_qdesc, nq, h_epoch, lb, ub, h_res, rank, h_detail);
}

// The per-scan loop on a scan that is still on the device (cc_scan_ingest): the launches follow the scan's ingest on the
// context's loop stream, no descriptor travels.
int cc_db_query_scan(cc_db *db, cc_scan *scan, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res) {
  if (!db || !scan || !h_res) return set_err(CC_EINVAL, "cc_db_query_scan: bad argument");
  if (!scan->d_desc) return set_err(CC_EINVAL, "cc_db_query_scan: the scan was offloaded (use cc_db_query_host with its host copy)");
  if (scan->ctx != db->ctx) return set_err(CC_EINVAL, "cc_db_query_scan: scan and database belong to different contexts");
  const int32_t epoch = db->n_scans;
  const int rcw = scan_wait_ready(scan, false);  // the loop stream behind the scan's ingest
  if (rcw != CC_OK) return rcw;
  return cc_db_query_batch(db, scan->d_desc, 1, &epoch, lb, ub, h_res, nullptr, nullptr, scan->ctx->s_loop);
}

// The asynchronous half of cc_db_query_scan at an explicit epoch: the query is queued (cc_db_query_submit), *h_res is
// filled by the next cc_db_query_wait.  What lets a per-scan driver keep several scans' queries in flight (the class
// mirror's read-ahead, hostcpp/cont2/contour_db.h): scan k at epoch k while the scans before it are being appended.
int cc_db_query_scan_submit(cc_db *db, cc_scan *scan, int32_t epoch, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res) {
  if (!db || !scan || !h_res) return set_err(CC_EINVAL, "cc_db_query_scan_submit: bad argument");
  if (!scan->d_desc) return set_err(CC_EINVAL, "cc_db_query_scan_submit: the scan was offloaded (use cc_db_query_batch_host with its host copy)");
  if (scan->ctx != db->ctx) return set_err(CC_EINVAL, "cc_db_query_scan_submit: scan and database belong to different contexts");
  const int rcw = scan_wait_ready(scan, false);  // the loop stream behind the scan's ingest
  if (rcw != CC_OK) return rcw;
  return cc_db_query_submit(db, scan->d_desc, 1, &epoch, lb, ub, h_res, nullptr, nullptr, scan->ctx->s_loop);
}

// cc_db_add_scans_prepare for a scan handle: the scan's compact records and the keys the host bookkeeping needs are on
// their way while the caller does something else (e.g. queues the scan's own query); cc_db_add_scan then only commits.
int cc_db_add_scan_prepare(cc_db *db, cc_scan *scan) {
  if (!db || !scan) return set_err(CC_EINVAL, "cc_db_add_scan_prepare: bad argument");
  if (!scan->d_desc) return set_err(CC_EINVAL, "cc_db_add_scan_prepare: the scan was offloaded");
  if (scan->ctx != db->ctx) return set_err(CC_EINVAL, "cc_db_add_scan_prepare: scan and database belong to different contexts");
  const int rcw = scan_wait_ready(scan, false);
  if (rcw != CC_OK) return rcw;
  return cc_db_add_scans_prepare(db, scan->d_desc, 1, scan->ctx->s_loop);
}

int cc_db_add_scan(cc_db *db, cc_scan *scan, double ts, int32_t seed) {
  if (!db || !scan) return set_err(CC_EINVAL, "cc_db_add_scan: bad argument");
  if (!scan->d_desc) return set_err(CC_EINVAL, "cc_db_add_scan: the scan was offloaded (use cc_db_add_scan_host with its host copy)");
  if (scan->ctx != db->ctx) return set_err(CC_EINVAL, "cc_db_add_scan: scan and database belong to different contexts");
  const int rcw = scan_wait_ready(scan, false);
  if (rcw != CC_OK) return rcw;
  return cc_db_add_scans(db, scan->d_desc, 1, &ts, &seed, scan->ctx->s_loop);
}

// ---- batches of scan handles: the per-scan loop's scans, a few at a time ----
// A driver that knows its next scans (the class mirror's read-ahead) appends and queries them B at a time: one chain of
// launches per B scans instead of one per scan -- the loop is bound by the number of launches, not by their work.  The
// handles' descriptors sit in separate slots of the context's pool; one small kernel gathers them into a contiguous
// staging array and the batched entry points take it from there.
struct cc_desc_tab {
  const cc_scan_desc_t *p[CC_SCAN_BATCH_MAX];
};
static_assert(sizeof(cc_scan_desc_t) % 8 == 0 && alignof(cc_scan_desc_t) % 8 == 0, "cc_k_gather_desc copies 8 bytes per lane");
#define CC_GATHER_BLOCKS 16  // workgroups per descriptor
__global__ void __launch_bounds__(256)
cc_k_gather_desc(cc_desc_tab tab, int n, cc_scan_desc_t *__restrict__ dst) {
  const int s = (int)blockIdx.x / CC_GATHER_BLOCKS, part = (int)blockIdx.x % CC_GATHER_BLOCKS;
  if (s >= n) return;
  const unsigned long long *__restrict__ src = (const unsigned long long *)tab.p[s];
  unsigned long long *__restrict__ out = (unsigned long long *)(dst + s);
  const int nv = (int)(sizeof(cc_scan_desc_t) / 8);
  for (int i = part * 256 + (int)threadIdx.x; i < nv; i += CC_GATHER_BLOCKS * 256) out[i] = src[i];
}

static int gather_handles(cc_db *db, cc_scan *const *scans, int n, int which, const char *what, const cc_scan_desc_t **out) {
  cc_desc_tab tab;
  for (int i = 0; i < n; i++) {
    if (!scans[i]) return set_err(CC_EINVAL, what);
    if (!scans[i]->d_desc) return set_err(CC_EINVAL, "cc_db_*_scan_batch: a scan of the batch was offloaded");
    if (scans[i]->ctx != db->ctx) return set_err(CC_EINVAL, "cc_db_*_scan_batch: scan and database belong to different contexts");
    tab.p[i] = scans[i]->d_desc;
  }
  for (int i = n; i < CC_SCAN_BATCH_MAX; i++) tab.p[i] = nullptr;
  HIPCHK(hipSetDevice(db->device));
  if (!db->d_hstage[which]) HIPCHK(hipMalloc(&db->d_hstage[which], sizeof(cc_scan_desc_t) * CC_SCAN_BATCH_MAX));
  for (int i = 0; i < n; i++) {
    const int rcw = scan_wait_ready(scans[i], false);  // the loop stream behind every scan's ingest
    if (rcw != CC_OK) return rcw;
  }
  hipLaunchKernelGGL(cc_k_gather_desc, dim3(n * CC_GATHER_BLOCKS), dim3(256), 0, db->ctx->s_loop, tab, n, db->d_hstage[which]);
  HIPCHK(hipGetLastError());
  *out = db->d_hstage[which];
  return CC_OK;
}

int cc_db_add_scan_batch(cc_db *db, cc_scan *const *scans, int n, const double *h_ts, const int32_t *h_seed) {
  if (!db || !scans || n < 1 || n > CC_SCAN_BATCH_MAX || !h_ts || !h_seed)
    return set_err(CC_EINVAL, "cc_db_add_scan_batch: bad argument (1..CC_SCAN_BATCH_MAX scans)");
  DB_POISON_CHK(db, "cc_db_add_scan_batch");
  if (db->prep_cnt > 0) return set_err(CC_EINVAL, "cc_db_add_scan_batch: batches prepared with cc_db_add_scans_prepare are waiting to be added");
  if (db->n_scans + n > db->cap) return set_err(CC_ECAPACITY, "cc_db_add_scan_batch: database capacity exceeded");
  const cc_scan_desc_t *d = nullptr;
  const int rc = gather_handles(db, scans, n, 0, "cc_db_add_scan_batch: null scan handle", &d);
  if (rc != CC_OK) return rc;
  return cc_db_add_scans(db, d, n, h_ts, h_seed, db->ctx->s_loop);
}

static int query_scan_batch_submit_impl(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *lb,
                                        const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank,
    cc_ranked_detail_t *detail /*with rank: where the chunks' detail rows go, or nullptr*/,
                                        const cc_match_out_t *match = nullptr) {
  if (!db || !scans || n < 1 || n > CC_SCAN_BATCH_MAX || !h_epoch || !lb || !ub || !h_res)
    return set_err(CC_EINVAL, "cc_db_query_scan_batch_submit: bad argument (1..CC_SCAN_BATCH_MAX scans)");
  DB_POISON_CHK(db, "cc_db_query_scan_batch_submit");
  for (int i = 0; i < n; i++)
    if (h_epoch[i] < 0 || h_epoch[i] > db->n_scans) return set_err(CC_EINVAL, "cc_db_query_scan_batch_submit: epoch out of range");
  const cc_scan_desc_t *d = nullptr;
  const int rc = gather_handles(db, scans, n, 1, "cc_db_query_scan_batch_submit: null scan handle", &d);
  if (rc != CC_OK) return rc;
  return query_submit_impl(db, d, n, h_epoch, lb, ub, h_res, nullptr, nullptr, db->ctx->s_loop, rank, detail, nullptr, nullptr, nullptr, match);
}
int cc_db_query_scan_batch_submit(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *lb,
                                  const cc_score_t *ub, cc_query_result_t *h_res) {
  return query_scan_batch_submit_impl(db, scans, n, h_epoch, lb, ub, h_res, nullptr, nullptr);
}
int cc_db_query_scan_batch_submit_ranked(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *lb,
                                         const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank) {
  const int vrc = want_ranked(__func__, rank, nullptr, false);
  if (vrc != CC_OK) return vrc;
  if (lb && ub && !thres_strict_smaller(lb, ub))  // (before the handles are gathered: a refused call queues nothing)
    return set_err(CC_EINVAL, "cc_db_query_scan_batch_submit_ranked: thresholds must satisfy lb.strictSmaller(ub)");
  return query_scan_batch_submit_impl(db, scans, n, h_epoch, lb, ub, h_res, rank, nullptr);
}
int cc_db_query_scan_batch_submit_ranked_detail(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *lb,
                                                const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  const int vrc = want_ranked(__func__, rank, h_detail, true);
  if (vrc != CC_OK) return vrc;
  if (lb && ub && !thres_strict_smaller(lb, ub))  // (before the handles are gathered: a refused call queues nothing)
    return set_err(CC_EINVAL, "cc_db_query_scan_batch_submit_ranked_detail: thresholds must satisfy lb.strictSmaller(ub)");
  return query_scan_batch_submit_impl(db, scans, n, h_epoch, lb, ub, h_res, rank, h_detail);
}

int cc_db_add_scan_host(cc_db *db, const cc_scan_desc_t *h_desc, double ts, int32_t seed) {
  return cc_db_add_scans_host(db, h_desc, 1, &ts, &seed);
}

int cc_db_query_host(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res) {
  if (!db || !h_qdesc || !h_res) return set_err(CC_EINVAL, "cc_db_query_host: bad argument");
  const int32_t epoch = db->n_scans;
  return cc_db_query_batch_host(db, h_qdesc, 1, &epoch, lb, ub, h_res);
}

// CandidateManager with explicit hints (single-pair flow, kitti_read_bin_test.cpp:226-291): the scoring chain of one
// query whose check table is the caller's hint list, in the caller's order, instead of the KNN result.
static int check_hints_impl(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                            const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores, void *stream_,
                            const cc_rank_out_t *rank,
    cc_ranked_detail_t *detail /*with rank: where the chunks' detail rows go, or nullptr*/,
                            const cc_match_out_t *match = nullptr /*with rank: where the match rows go (validated by the entry point), or nullptr*/) {
  if (!db || !d_qdesc || n_hints < 0 || (n_hints > 0 && !h_hints) || !lb || !ub || !h_res || max_fine_opt < 1)
    return set_err(CC_EINVAL, "cc_db_check_hints: bad argument");
  DB_POISON_CHK(db, "cc_db_check_hints");
  DB_DRAIN(db);
  if (n_hints > CC_HINT_MAX) return set_err(CC_ECAPACITY, "cc_db_check_hints: more than CC_HINT_MAX hints");
  if (!thres_strict_smaller(lb, ub)) return set_err(CC_EINVAL, "cc_db_check_hints: thresholds must satisfy lb.strictSmaller(ub)");
  const int NS = CC_NQLEV * CC_NPIV;
  std::vector<cc_knn_hit_t> hits((size_t)NS * CC_KNN_MAX);
  memset(hits.data(), 0, sizeof(cc_knn_hit_t) * hits.size());
  int hit_cnt[CC_NQLEV * CC_NPIV];
  for (int i = 0; i < n_hints; i++) {
    const cc_hint_t &h = h_hints[i];
    if (h.cand_gidx < 0 || h.cand_gidx >= db->n_scans) return set_err(CC_EINVAL, "cc_db_check_hints: candidate scan not in the DB");
    if (h.level < 1 || h.level > CC_BCI_LAYERS) return set_err(CC_EINVAL, "cc_db_check_hints: hint level must be within 1..4");
    if (h.seq_src < 0 || h.seq_src >= CC_NPIV || h.seq_tgt < 0 || h.seq_tgt >= CC_NPIV ||
        h.seq_src >= db->lite[h.cand_gidx].n_cont[h.level - 1])
      return set_err(CC_EINVAL, "cc_db_check_hints: hint names an anchor that does not exist");
    hits[i].gidx = h.cand_gidx;
    hits[i].level = CC_HIT_PACK_LEVEL(h.level, h.seq_tgt);
    hits[i].seq = h.seq_src;
  }
  for (int s = 0; s < NS; s++) {
    const int left = n_hints - s * CC_KNN_MAX;
    hit_cnt[s] = left < 0 ? 0 : (left > CC_KNN_MAX ? CC_KNN_MAX : left);
  }
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(db->device));
  if (!db->d_hint_scores) HIPCHK(hipMalloc(&db->d_hint_scores, sizeof(int) * (size_t)CC_CHK_STRIDE * CC_NSCORE));
  cc_qlane &ln = db->lane[0];
  {
    const int arc = lane_alloc_modes(db, ln, rank, detail, match);
    if (arc != CC_OK) return arc;
  }
  HIPCHK(hipEventRecord(ln.done, stream));  // start after what the caller queued
  HIPCHK(hipStreamWaitEvent(ln.stream, ln.done, 0));
  if (db->add_done) HIPCHK(hipStreamWaitEvent(ln.stream, db->add_done, 0));  // ... and after the last append, whatever stream it used
  HIPCHK(hipMemcpyAsync(ln.d_hits, hits.data(), sizeof(cc_knn_hit_t) * hits.size(), hipMemcpyHostToDevice, ln.stream));
  HIPCHK(hipMemcpyAsync(ln.d_hit_cnt, hit_cnt, sizeof(hit_cnt), hipMemcpyHostToDevice, ln.stream));
  const cc_check_params CP = make_check_params(db, lb);
  int rc = launch_query_prep(db, ln, d_qdesc, 1);
  if (rc != CC_OK) return rc;
  {  // a hint must name contours that exist on BOTH sides (the reference would CHECK-fail on the missing view): the query
     // scan is device-resident, so its contour counts are fetched (this flow is not the hot one)
    ScanLite ql;
    rc = fetch_lite(db, ln.d_qhot, 1, &ql, ln.stream);
    if (rc != CC_OK) return rc;
    for (int i = 0; i < n_hints; i++)
      if (h_hints[i].seq_tgt >= ql.n_cont[h_hints[i].level - 1])
        return set_err(CC_EINVAL, "cc_db_check_hints: hint names a contour of the query scan that does not exist");
  }
  rc = launch_scoring_chain(db, ln, 1, CP, lb, ub, max_fine_opt, nullptr, db->d_hint_scores, false, CC_KNN_MAX, rank ? rank->max_ret : 0, detail != nullptr, match);  // any database: 64-stride
  if (rc != CC_OK) return rc;
  std::vector<int> sc((size_t)CC_CHK_STRIDE * CC_NSCORE);
  std::vector<unsigned char> ok(CC_CHK_STRIDE);
  rc = results_copy_back(cc_chunk{ln, 0, 1, false, nullptr}, rank, detail, match);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpyAsync(sc.data(), db->d_hint_scores, sizeof(int) * sc.size(), hipMemcpyDeviceToHost, ln.stream));
  HIPCHK(hipMemcpyAsync(ok.data(), ln.d_pass_ok, ok.size(), hipMemcpyDeviceToHost, ln.stream));
  HIPCHK(hipStreamSynchronize(ln.stream));
  rc = chunk_status(ln, 1);  // CC_ECAPACITY: the result and the scores are delivered all the same (flags says what was hit)
  *h_res = ln.h_results[0];
  if (rank) rank_deliver(ln, *rank, 0, 1, max_fine_opt);
  if (detail) memcpy(detail, ln.h_detail, sizeof(cc_ranked_detail_t) * (size_t)rank->max_ret);
  if (match) memcpy(match->h_match, ln.h_match, sizeof(cc_ranked_match_t) * (size_t)rank->max_ret);
  if (h_scores)
    for (int i = 0; i < n_hints; i++) {
      const int *p = &sc[(size_t)i * CC_NSCORE];
      h_scores[i].i_ovlp_sum = p[0];
      h_scores[i].i_ovlp_max_one = p[1];
      h_scores[i].i_in_ang_rng = p[2];
      h_scores[i].i_indiv_sim = p[3];
      h_scores[i].i_orie_sim = p[4];
      h_scores[i].passed = ok[i] == 1;
    }
  return rc;
}

int cc_db_check_hints(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                      const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores, void *stream_) {
  return check_hints_impl(db, d_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, stream_, nullptr, nullptr);
}
int cc_db_check_hints_ranked(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                             const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores, void *stream_,
                             const cc_rank_out_t *rank) {
  const int vrc = want_ranked(__func__, rank, nullptr, false);
  if (vrc != CC_OK) return vrc;
  return check_hints_impl(db, d_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, stream_, rank, nullptr);
}
int cc_db_check_hints_ranked_detail(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                                    const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores, void *stream_, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  const int vrc = want_ranked(__func__, rank, h_detail, true);
  if (vrc != CC_OK) return vrc;
  return check_hints_impl(db, d_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, stream_, rank, h_detail);
}

int cc_db_debug_passes(cc_db *db, cc_pass_dbg_t *h_out, int cap, int *n_out) {
  if (!db || !h_out || cap < 0 || !n_out) return set_err(CC_EINVAL, "cc_db_debug_passes: bad argument");
  HIPCHK(hipSetDevice(db->device));
  DB_DRAIN(db);  // lane 0 may carry a submitted chunk
  cc_qlane &ln = db->lane[0];  // the hint flow runs on lane 0, query 0
  std::vector<unsigned char> ok(CC_CHK_STRIDE);
  std::vector<cc_pass_rec> rec(CC_CHK_STRIDE);
  HIPCHK(hipMemcpy(ok.data(), ln.d_pass_ok, ok.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rec.data(), ln.d_pass, sizeof(cc_pass_rec) * rec.size(), hipMemcpyDeviceToHost));
  int n = 0;
  for (int t = 0; t < CC_CHK_STRIDE && n < cap; t++) {
    if (ok[t] != 1) continue;
    cc_pass_dbg_t o;
    o.hint = t;
    o.n_pairs = rec[t].n_pairs;
    for (int k = 0; k < 3; k++) o.tf[k] = rec[t].tf[k];
    for (int k = 0; k < 7; k++) o.pairs[k] = rec[t].bits[k];
    h_out[n++] = o;
  }
  *n_out = n;
  return CC_OK;
}

// include/cont2_amd_cands.h: query 0 of lane 0 is the hint flow's; cc_k_merge left the candidates in first-appearance order in
// d_cands, their number in d_qstate, and the correlation problem of a candidate that went on at d_prob[gmm_idx]
int cc_db_debug_cands(cc_db *db, cc_cand_dbg_t *h_out, int cap, int *n_out) {
  if (!db || !h_out || cap < 0 || !n_out) return set_err(CC_EINVAL, "cc_db_debug_cands: bad argument");
  HIPCHK(hipSetDevice(db->device));
  DB_DRAIN(db);
  cc_qlane &ln = db->lane[0];
  cc_qstate st;
  HIPCHK(hipMemcpy(&st, ln.d_qstate, sizeof(st), hipMemcpyDeviceToHost));
  int n = st.n_cand < 0 ? 0 : (st.n_cand > CC_MAXCAND ? CC_MAXCAND : st.n_cand);
  if (n > cap) n = cap;
  std::vector<cc_cand_out> cd(n > 0 ? n : 1);
  if (n > 0) HIPCHK(hipMemcpy(cd.data(), ln.d_cands, sizeof(cc_cand_out) * (size_t)n, hipMemcpyDeviceToHost));
  for (int k = 0; k < n; k++) {
    cc_cand_dbg_t o;
    o.cand_gidx = cd[k].gidx;
    o.n_props = cd[k].nprops;
    o.refined = cd[k].gmm_idx >= 0 ? 1 : 0;
    o.pad_ = 0;
    o.tf_init[0] = o.tf_init[1] = o.tf_init[2] = 0.0;
    if (cd[k].gmm_idx >= 0 && cd[k].gmm_idx < ln.prob_cap) {
      cc_gmm_problem pb;
      HIPCHK(hipMemcpy(&pb, ln.d_prob + cd[k].gmm_idx, sizeof(pb), hipMemcpyDeviceToHost));
      for (int j = 0; j < 3; j++) o.tf_init[j] = pb.tf[j];
    }
    h_out[k] = o;
  }
  *n_out = n;
  return CC_OK;
}

// include/cont2_amd_keyview.h: the buffer of the layer's sorted view that the next chunk would read (scur), after the chunks in
// flight and the last append's merge have finished; read-only
int cc_db_debug_key_view(cc_db *db, int layer, int cap, float *keys, int32_t *sid, int32_t *sact, int32_t *n) {
  if (!db || !keys || !sid || !sact || !n || cap < 0 || layer < 0 || layer >= db->cfg.n_q_levels)
    return set_err(CC_EINVAL, "cc_db_debug_key_view: bad argument");
  HIPCHK(hipSetDevice(db->device));
  DB_DRAIN(db);
  if (db->add_done) HIPCHK(hipEventSynchronize(db->add_done));
  const int nk = db->n_keys[layer], cur = db->scur[layer];
  *n = nk;
  if (nk > cap) return set_err(CC_ECAPACITY, "cc_db_debug_key_view: the layer holds more keys than cap");
  if (nk == 0) return CC_OK;
  for (int d = 0; d <= CC_KEY_DIM; d++)
    HIPCHK(hipMemcpy(keys + (size_t)d * (size_t)cap, db->d_skeys[layer][cur] + (size_t)d * (size_t)db->cap_k, sizeof(float) * (size_t)nk, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sid, db->d_sid[layer][cur], sizeof(int) * (size_t)nk, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sact, db->d_sact[layer][cur], sizeof(int) * (size_t)nk, hipMemcpyDeviceToHost));
  return CC_OK;
}

static int check_hints_host_impl(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                                 const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores,
                                 const cc_rank_out_t *rank,
    cc_ranked_detail_t *detail /*with rank: where the chunks' detail rows go, or nullptr*/,
                                 const cc_match_out_t *match = nullptr) {
  if (!db || !h_qdesc) return set_err(CC_EINVAL, "cc_db_check_hints_host: bad argument");
  HIPCHK(hipSetDevice(db->device));
  int rc = stage_reserve(db, 1);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpy(db->d_stage, h_qdesc, sizeof(cc_scan_desc_t), hipMemcpyHostToDevice));
  return check_hints_impl(db, db->d_stage, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, nullptr, rank, detail, match);
}
int cc_db_check_hints_host(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                           const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores) {
  return check_hints_host_impl(db, h_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, nullptr, nullptr);
}
int cc_db_check_hints_host_ranked(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                                  const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores,
                                  const cc_rank_out_t *rank) {
  const int vrc = want_ranked(__func__, rank, nullptr, false);
  if (vrc != CC_OK) return vrc;
  return check_hints_host_impl(db, h_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, rank, nullptr);
}
int cc_db_check_hints_host_ranked_detail(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                                         const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  const int vrc = want_ranked(__func__, rank, h_detail, true);
  if (vrc != CC_OK) return vrc;
  return check_hints_host_impl(db, h_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, rank, h_detail);
}

// ---- verification of caller-proposed candidates (k_verify.h) ----
// The batched form of the hint flow: item i is query descriptor h_qidx[i] against <= CC_VERIFY_CANDS_MAX database scans.  The
// check table of a chunk is written by cc_k_hints_expand in the place of the KNN search; everything after it is the query
// path's chain, chunked over the lanes and collected like cc_db_query_submit's chunks.
static int verify_validate(const cc_db *db, const void *d_qdesc /*the descriptors, or the hot records of a packed source*/, int n_desc,
                           const int32_t *h_qidx, const int32_t *h_cands, int n, const cc_verify_cfg_t *cfg, const cc_score_t *lb,
                           const cc_score_t *ub, const cc_query_result_t *h_res, bool packed = false) {
  if (!db || !d_qdesc || n_desc < 0 || n < 0 || (n > 0 && !h_cands) || !cfg || !lb || !ub || !h_res)
    return set_err(CC_EINVAL, "cc_db_verify: bad argument");
  if (!h_qidx && packed && n > n_desc) return set_err(CC_EINVAL, "cc_db_verify: without h_qidx item i reads record i, so n must not exceed the source");
  if (!h_qidx && !packed && n != n_desc) return set_err(CC_EINVAL, "cc_db_verify: without h_qidx item i reads descriptor i, so n must equal n_desc");
  if (cfg->max_fine_opt < 1) return set_err(CC_EINVAL, "cc_db_verify: max_fine_opt must be positive");
  if (cfg->level_mask < 0 || cfg->level_mask > 15) return set_err(CC_EINVAL, "cc_db_verify: level_mask must be within 0..15 (bit level-1 of levels 1..4)");
  if (!(cfg->max_key_dist_sq >= 0.f)) return set_err(CC_EINVAL, "cc_db_verify: max_key_dist_sq must be >= 0 (INFINITY: no bound)");
  if (!thres_strict_smaller(lb, ub)) return set_err(CC_EINVAL, "cc_db_verify: thresholds must satisfy lb.strictSmaller(ub)");
  for (int i = 0; i < n; i++) {
    if (h_qidx && (h_qidx[i] < 0 || h_qidx[i] >= n_desc)) return set_err(CC_EINVAL, "cc_db_verify: query descriptor index out of range");
    const int32_t *c = h_cands + (size_t)i * CC_VERIFY_CANDS_MAX;
    bool ended = false;
    for (int k = 0; k < CC_VERIFY_CANDS_MAX; k++) {
      if (c[k] == -1) {
        ended = true;
        continue;
      }
      if (ended) return set_err(CC_EINVAL, "cc_db_verify: a candidate list continues after its first -1");
      if (c[k] < 0 || c[k] >= db->n_scans) return set_err(CC_EINVAL, "cc_db_verify: candidate scan not in the DB");
      for (int j = 0; j < k; j++)
        if (c[j] == c[k]) return set_err(CC_EINVAL, "cc_db_verify: a candidate is listed twice in one item");
    }
  }
  return CC_OK;
}

static int verify_submit_impl(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                              const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                              cc_hint_t *d_hints, int32_t *d_n_hints, void *stream_, const cc_rank_out_t *rank,
    cc_ranked_detail_t *detail /*with rank: where the chunks' detail rows go, or nullptr*/,
                              const cc_rec_src *rec = nullptr /*the queries are packed records: d_qdesc is nullptr, n_desc their number*/,
                              const cc_match_out_t *match = nullptr /*with rank: where the chunks' match rows go (validated by the entry point), or nullptr*/) {
  {  // everything that can be refused is refused before anything is queued or collected
    const int vrc = verify_validate(db, rec ? (const void *)rec->hot : (const void *)d_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, rec != nullptr);
    if (vrc != CC_OK) return vrc;
  }
  DB_POISON_CHK(db, "cc_db_verify_submit");
  HIPCHK(hipSetDevice(db->device));
  const cc_check_params CP = make_check_params(db, lb);
  cc_verify_params VP;
  VP.level_mask = cfg->level_mask ? cfg->level_mask : 0xF;
  VP.max_key_dist_sq = cfg->max_key_dist_sq;
  // the chain is the 64-stride one on any database, as in the hint flow
  cc_chunk_plan plan;
  plan.alloc = [&](cc_qlane &ln, int, int) -> int {
    const int rc = lane_alloc_verify(ln);
    return rc != CC_OK ? rc : lane_alloc_modes(db, ln, rank, detail, match);
  };
  plan.stage = [&](const cc_chunk &c) {  // the chunk's table, packed: [nb] | [nb][CC_VERIFY_CANDS_MAX]
    int *h_sel = c.ln.h_vin, *h_cl = c.ln.h_vin + c.nb;
    for (int i = 0; i < c.nb; i++) h_sel[i] = h_qidx ? h_qidx[c.b0 + i] : c.b0 + i;
    memcpy(h_cl, h_cands + (size_t)c.b0 * CC_VERIFY_CANDS_MAX, sizeof(int) * (size_t)c.nb * CC_VERIFY_CANDS_MAX);
  };
  plan.upload = [&](const cc_chunk &c, cc_prep_src &src) -> int {
    cc_qlane &ln = c.ln;
    HIPCHK(hipMemcpyAsync(ln.d_vin, ln.h_vin, sizeof(int) * (size_t)c.nb * (1 + CC_VERIFY_CANDS_MAX), hipMemcpyHostToDevice, ln.stream));
    src = cc_prep_src{d_qdesc, false, ln.d_vin, rec};
    return CC_OK;
  };
  plan.head = [&](const cc_chunk &c) -> int {  // the check table from the candidate lists
    cc_qlane &ln = c.ln;
    const int nb = c.nb, b0 = c.b0;
    hipLaunchKernelGGL(cc_k_hints_expand, dim3(nb), dim3(64), 0, ln.stream, VP, (const cc_hot_desc_t *)ln.d_qhot, (const cc_hot_desc_t *)db->d_hot,
                       (const int *)(ln.d_vin + nb), nb, ln.d_hits, ln.d_hit_cnt, d_hints ? d_hints + (size_t)b0 * CC_HINT_MAX : (cc_hint_t *)nullptr,
                       d_n_hints ? d_n_hints + b0 : (int32_t *)nullptr);
    return CC_OK;
  };
  plan.body = [&](const cc_chunk &c) -> int {
    return launch_scoring_chain(db, c.ln, c.nb, CP, lb, ub, cfg->max_fine_opt, c.ev, nullptr, c.zc, CC_KNN_MAX, rank ? rank->max_ret : 0, detail != nullptr, match);
  };
  plan.copy_back = [&](const cc_chunk &c) -> int { return results_copy_back(c, rank, detail, match); };
  plan.note = [&](const cc_chunk &c) { results_note(c.ln, h_res, rank, detail, cfg->max_fine_opt, match); };
  return submit_chunks(db, n, (hipStream_t)stream_, plan);
}
int cc_db_verify_submit(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                        const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                        cc_hint_t *d_hints, int32_t *d_n_hints, void *stream_) {
  return verify_submit_impl(db, d_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, d_hints, d_n_hints, stream_, nullptr, nullptr);
}
int cc_db_verify_submit_ranked(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                               const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                               cc_hint_t *d_hints, int32_t *d_n_hints, void *stream_, const cc_rank_out_t *rank) {
  const int vrc = want_ranked(__func__, rank, nullptr, false);
  if (vrc != CC_OK) return vrc;
  return verify_submit_impl(db, d_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, d_hints, d_n_hints, stream_, rank, nullptr);
}
int cc_db_verify_submit_ranked_detail(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                                      const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                                      cc_hint_t *d_hints, int32_t *d_n_hints, void *stream_, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  const int vrc = want_ranked(__func__, rank, h_detail, true);
  if (vrc != CC_OK) return vrc;
  return verify_submit_impl(db, d_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, d_hints, d_n_hints, stream_, rank, h_detail);
}

int cc_db_verify_batch(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                       const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                       cc_hint_t *d_hints, int32_t *d_n_hints, void *stream_) {
  {  // a refused call leaves the chunks in flight where they are
    const int vrc = verify_validate(db, d_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res);
    if (vrc != CC_OK) return vrc;
  }
  return run_sync(db, [&] { return cc_db_verify_submit(db, d_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, d_hints, d_n_hints, stream_); });
}

static int verify_batch_host_impl(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                                  const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                                  const cc_rank_out_t *rank,
    cc_ranked_detail_t *detail /*with rank: where the chunks' detail rows go, or nullptr*/,
                                  const cc_match_out_t *match = nullptr) {
  {
    const int vrc = verify_validate(db, h_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res);
    if (vrc != CC_OK) return vrc;
  }
  if (n == 0) return CC_OK;
  HIPCHK(hipSetDevice(db->device));
  int rc = stage_reserve(db, n_desc);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpy(db->d_stage, h_qdesc, sizeof(cc_scan_desc_t) * (size_t)n_desc, hipMemcpyHostToDevice));
  if (!rank) return cc_db_verify_batch(db, db->d_stage, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, nullptr, nullptr, nullptr);
  return run_sync(db, [&] { return verify_submit_impl(db, db->d_stage, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, nullptr, nullptr, nullptr, rank, detail, nullptr, match); });
}
int cc_db_verify_batch_host(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                            const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res) {
  return verify_batch_host_impl(db, h_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, nullptr, nullptr);
}
int cc_db_verify_batch_host_ranked(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                                   const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                                   const cc_rank_out_t *rank) {
  const int vrc = want_ranked(__func__, rank, nullptr, false);
  if (vrc != CC_OK) return vrc;
  return verify_batch_host_impl(db, h_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, rank, nullptr);
}
int cc_db_verify_batch_host_ranked_detail(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                                          const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  const int vrc = want_ranked(__func__, rank, h_detail, true);
  if (vrc != CC_OK) return vrc;
  return verify_batch_host_impl(db, h_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, rank, h_detail);
}

// ---- caller-given relative poses (k_pose.h) ----
// Item i is correlation problem i of its chunk and reads query record i, which launch_query_prep builds from descriptor q_i (the
// verify flow's selector).  The chain is prep | cc_k_pose_problems | cc_k_gmm_init | cc_k_pose_select | cc_k_gmm_refine x 2 |
// cc_k_pose_eval | cc_k_pose_final: no retrieval, no checks, no merge, no cc_k_select / cc_k_final.
static int pose_validate(const cc_db *db, const void *qdesc /*the descriptors, or the hot records of a packed source*/, int n_desc, const cc_pose_item_t *h_items, int n, const cc_pose_cfg_t *cfg,
                         const double *h_try, const cc_pose_result_t *h_res, const double *h_try_corr) {
  if (!db || !qdesc || !h_items || !cfg || !h_res || n < 0) return set_err(CC_EINVAL, "cc_db_pose: bad argument");
  if (cfg->refine != 0 && cfg->refine != 1) return set_err(CC_EINVAL, "cc_db_pose: refine must be 0 or 1");
  if (cfg->min_corr != cfg->min_corr) return set_err(CC_EINVAL, "cc_db_pose: min_corr is NaN (-INFINITY: no bar)");
  if (cfg->n_try < 0 || cfg->n_try > CC_POSE_TRY_MAX) return set_err(CC_EINVAL, "cc_db_pose: n_try must be within 0..CC_POSE_TRY_MAX");
  if (cfg->n_try > 0 && (!h_try || !h_try_corr)) return set_err(CC_EINVAL, "cc_db_pose: n_try > 0 needs h_try and h_try_corr");
  for (int i = 0; i < n; i++) {
    if (h_items[i].q < 0 || h_items[i].q >= n_desc) return set_err(CC_EINVAL, "cc_db_pose: query descriptor index out of range");
    if (h_items[i].gidx < 0 || h_items[i].gidx >= db->n_scans) return set_err(CC_EINVAL, "cc_db_pose: database scan not in the DB");
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(h_items[i].tf[k])) return set_err(CC_EINVAL, "cc_db_pose: a start pose has a non-finite component");
  }
  for (size_t k = 0; k < (size_t)n * cfg->n_try * 3; k++)
    if (!std::isfinite(h_try[k])) return set_err(CC_EINVAL, "cc_db_pose: a try pose has a non-finite component");
  return CC_OK;
}

// rec: the queries are packed records (then d_qdesc is nullptr and n_desc their number), or nullptr
static int pose_submit_impl(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const cc_pose_item_t *h_items, int n, const cc_pose_cfg_t *cfg,
                            const double *h_try, cc_pose_result_t *h_res, double *h_try_corr, cc_pose_curv_t *h_curv, void *stream_, const cc_rec_src *rec) {
  {  // everything that can be refused is refused before anything is queued or collected
    const int vrc = pose_validate(db, rec ? (const void *)rec->hot : (const void *)d_qdesc, n_desc, h_items, n, cfg, h_try, h_res, h_try_corr);
    if (vrc != CC_OK) return vrc;
  }
  DB_POISON_CHK(db, "cc_db_pose_submit");
  if (n == 0) return CC_OK;
  HIPCHK(hipSetDevice(db->device));
  const int nt = cfg->n_try;
  const bool refine = cfg->refine != 0, curv = h_curv != nullptr;
  // a chunk's tables in the lane's buffers, packed.  In: items [nb] | try poses [nb][nt][3] | selector [nb]; out: rows [nb] | try
  // results [nb][nt] | curvature rows [nb] (small chunks: the kernels write them straight into the lane's pinned buffer)
  struct tables {
    cc_pose_item_t *it;
    double *tp;
    int *sel;
    cc_pose_result_t *res;
    double *tr;
    cc_pose_curv_t *cv;
  };
  auto tables_at = [nt](char *in, char *out, int nb) {
    cc_pose_item_t *it = (cc_pose_item_t *)in;
    double *tp = (double *)(it + nb);
    cc_pose_result_t *res = (cc_pose_result_t *)out;
    double *tr = (double *)(res + nb);
    return tables{it, tp, (int *)(tp + (size_t)nb * nt * 3), res, tr, (cc_pose_curv_t *)(tr + (size_t)nb * nt)};
  };
  cc_chunk_plan plan;
  plan.alloc = [&](cc_qlane &ln, int, int) -> int { return lane_alloc_pose(ln); };
  plan.stage = [&](const cc_chunk &c) {
    const tables h = tables_at(c.ln.h_pin, c.ln.h_pout, c.nb);
    memcpy(h.it, h_items + c.b0, sizeof(cc_pose_item_t) * (size_t)c.nb);
    if (nt > 0) memcpy(h.tp, h_try + (size_t)c.b0 * nt * 3, sizeof(double) * (size_t)c.nb * nt * 3);
    for (int i = 0; i < c.nb; i++) h.sel[i] = h_items[c.b0 + i].q;
  };
  plan.upload = [&](const cc_chunk &c, cc_prep_src &src) -> int {
    cc_qlane &ln = c.ln;
    HIPCHK(hipMemcpyAsync(ln.d_pin, ln.h_pin, CC_POSE_IN_BYTES(c.nb, nt), hipMemcpyHostToDevice, ln.stream));
    src = cc_prep_src{d_qdesc, false, tables_at(ln.d_pin, ln.d_pout, c.nb).sel, rec};
    return CC_OK;
  };
  plan.head = [&](const cc_chunk &c) -> int {  // item i is problem i
    cc_qlane &ln = c.ln;
    hipLaunchKernelGGL(cc_k_pose_problems, dim3((c.nb + 255) / 256), dim3(256), 0, ln.stream, (const cc_pose_item_t *)tables_at(ln.d_pin, ln.d_pout, c.nb).it, c.nb,
                       ln.d_prob, ln.d_prob_list, ln.d_nprob);
    return CC_OK;
  };
  plan.body = [&](const cc_chunk &c) -> int {
    cc_qlane &ln = c.ln;
    hipStream_t ls = ln.stream;
    hipEvent_t *ev = c.ev;
    const int nb = c.nb;
    const tables d = tables_at(ln.d_pin, c.zc ? ln.h_pout : ln.d_pout, nb);
    if (ev) {  // (no checks, no merge: the stages in between are empty)
      HIPCHK(hipEventRecord(ev[2], ls));
      HIPCHK(hipEventRecord(ev[3], ls));
    }
    launch_gmm_init(db, ln);
    if (refine) {  // (else the list counters stay zero: nothing reads them)
      hipLaunchKernelGGL(cc_k_pose_select, dim3((nb + 63) / 64), dim3(64), 0, ls, nb, cfg->min_corr, (const cc_gmm_result *)ln.d_gres, ln.d_sel, ln.prob_cap,
                         ln.head(CC_HD_NSEL16), ln.head(CC_HD_NMID), ln.sel(CC_SEL_CLS), ln.head(CC_HD_CLS), ln.head(CC_HD_POOL), ln.d_pool_off);
      launch_refine(db, ln, cfg->min_corr);
    }
    if (nt > 0 || curv) {
      const int grid = nb < db->tune.gmm64 ? nb : db->tune.gmm64;
      hipLaunchKernelGGL(cc_k_pose_eval, dim3(grid), dim3(64), 0, ls, (const cc_gmm_problem *)ln.d_prob, (const int *)ln.d_prob_list, (const int *)ln.d_nprob,
                         (const cc_gmm_feat *)ln.d_qfeat, (const cc_gmm_feat *)db->d_feat, (const cc_gmm_result *)ln.d_gres, (const unsigned *)ln.d_codes, nt,
                         (const double *)d.tp, d.tr, curv ? d.cv : (cc_pose_curv_t *)nullptr);
    }
    if (ev) HIPCHK(hipEventRecord(ev[4], ls));
    hipLaunchKernelGGL(cc_k_pose_final, dim3((nb + 255) / 256), dim3(256), 0, ls, (const cc_pose_item_t *)d.it, nb, (const cc_gmm_result *)ln.d_gres, d.res, (const int *)ln.d_nprob,
                       c.zc ? ln.h_nprob : (int *)nullptr);
    if (ev) HIPCHK(hipEventRecord(ev[5], ls));
    HIPCHK(hipGetLastError());
    return CC_OK;
  };
  plan.copy_back = [&](const cc_chunk &c) -> int {
    cc_qlane &ln = c.ln;
    HIPCHK(hipMemcpyAsync(ln.h_pout, ln.d_pout, CC_POSE_OUT_BYTES(c.nb, nt, curv), hipMemcpyDeviceToHost, ln.stream));
    HIPCHK(hipMemcpyAsync(ln.h_nprob, ln.d_nprob, sizeof(int) * 4, hipMemcpyDeviceToHost, ln.stream));
    return CC_OK;
  };
  plan.note = [&](const cc_chunk &c) {
    cc_qlane &ln = c.ln;
    ln.pose = true;
    ln.pose_res = h_res;
    ln.pose_try = nt > 0 ? h_try_corr : nullptr;
    ln.pose_curv = h_curv;
    ln.pose_ntry = nt;
  };
  return submit_chunks(db, n, (hipStream_t)stream_, plan);
}
int cc_db_pose_submit(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const cc_pose_item_t *h_items, int n, const cc_pose_cfg_t *cfg,
                      const double *h_try, cc_pose_result_t *h_res, double *h_try_corr, cc_pose_curv_t *h_curv, void *stream_) {
  return pose_submit_impl(db, d_qdesc, n_desc, h_items, n, cfg, h_try, h_res, h_try_corr, h_curv, stream_, nullptr);
}

int cc_db_pose_batch(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const cc_pose_item_t *h_items, int n, const cc_pose_cfg_t *cfg,
                     const double *h_try, cc_pose_result_t *h_res, double *h_try_corr, cc_pose_curv_t *h_curv, void *stream_) {
  {  // a refused call leaves the chunks in flight where they are
    const int vrc = pose_validate(db, d_qdesc, n_desc, h_items, n, cfg, h_try, h_res, h_try_corr);
    if (vrc != CC_OK) return vrc;
  }
  return run_sync(db, [&] { return cc_db_pose_submit(db, d_qdesc, n_desc, h_items, n, cfg, h_try, h_res, h_try_corr, h_curv, stream_); });
}

int cc_db_pose_batch_host(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const cc_pose_item_t *h_items, int n, const cc_pose_cfg_t *cfg,
                          const double *h_try, cc_pose_result_t *h_res, double *h_try_corr, cc_pose_curv_t *h_curv) {
  {
    const int vrc = pose_validate(db, h_qdesc, n_desc, h_items, n, cfg, h_try, h_res, h_try_corr);
    if (vrc != CC_OK) return vrc;
  }
  if (n == 0) return CC_OK;
  HIPCHK(hipSetDevice(db->device));
  const int rc = stage_reserve(db, n_desc);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpy(db->d_stage, h_qdesc, sizeof(cc_scan_desc_t) * (size_t)n_desc, hipMemcpyHostToDevice));
  return cc_db_pose_batch(db, db->d_stage, n_desc, h_items, n, cfg, h_try, h_res, h_try_corr, h_curv, nullptr);
}

// ---- packed records and stored scans as the query of the three flows (k_prep_packed.h) ----
// The submits above with a record source in the place of the descriptors: the chunk driver launches cc_k_prep_packed where it
// launches cc_k_pack_hot + cc_k_gmm_prep for them; every plan.head / plan.body is the descriptor form's.
int cc_db_query_submit_packed(cc_db *db, const cc_packed_src_t *src, const int32_t *h_rec, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                              const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream_,
                              const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  cc_rec_src rs;
  int vrc = packed_resolve(__func__, db, src, &rs);
  if (vrc == CC_OK) vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  return query_submit_impl(db, nullptr, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, &rs, h_rec);
}
int cc_db_verify_submit_packed(cc_db *db, const cc_packed_src_t *src, const int32_t *h_qidx, const int32_t *h_cands, int n, const cc_verify_cfg_t *cfg,
                               const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints,
                               void *stream_, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail) {
  cc_rec_src rs;
  int vrc = packed_resolve(__func__, db, src, &rs);
  if (vrc == CC_OK) vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  return verify_submit_impl(db, nullptr, rs.n_rec, h_qidx, h_cands, n, cfg, lb, ub, h_res, d_hints, d_n_hints, stream_, rank, h_detail, &rs);
}
int cc_db_pose_submit_packed(cc_db *db, const cc_packed_src_t *src, const cc_pose_item_t *h_items, int n, const cc_pose_cfg_t *cfg, const double *h_try,
                             cc_pose_result_t *h_res, double *h_try_corr, cc_pose_curv_t *h_curv, void *stream_) {
  cc_rec_src rs;
  const int vrc = packed_resolve(__func__, db, src, &rs);
  if (vrc != CC_OK) return vrc;
  return pose_submit_impl(db, nullptr, rs.n_rec, h_items, n, cfg, h_try, h_res, h_try_corr, h_curv, stream_, &rs);
}

// ---- masked queries: the retrieval restricted to a caller-given set of scans (k_knn.h: the walk's MASK instances) ----
// The one masked form of cc_db_query_submit[_packed][_ranked[_detail]]: descriptors or a record source, rank / h_detail as in
// the packed form.  mask NULL is the unmasked call of the same arguments.
int cc_db_query_submit_masked(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_packed_src_t *src, const int32_t *h_rec, int nq,
                              const int32_t *h_epoch, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn,
                              int32_t *d_knn_cnt, void *stream_, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                              const cc_scan_mask_t *mask) {
  if ((d_qdesc != nullptr) == (src != nullptr)) return set_err(CC_EINVAL, "cc_db_query_submit_masked: exactly one of d_qdesc and src must be given");
  int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  if (!src) return query_submit_impl(db, d_qdesc, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, nullptr, nullptr, mask);
  cc_rec_src rs;
  vrc = packed_resolve(__func__, db, src, &rs);
  if (vrc != CC_OK) return vrc;
  return query_submit_impl(db, nullptr, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, &rs, h_rec, mask);
}

// ... with host descriptors and a host table: both are staged on the device (the table in a buffer of the handle's that grows
// on demand; the call is synchronous, so the next one finds it free), then the submit above and the wait.
// (fn: the entry point's name for the refusals of its modes; the messages of the body name the masked host form, whose body it is)
static int query_batch_host_masked_impl(const char *fn, cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                        const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                                        const cc_scan_mask_t *mask, const cc_match_out_t *match) {
  if (!db || !h_qdesc || nq < 0 || !h_epoch || !lb || !ub || !h_res) return set_err(CC_EINVAL, "cc_db_query_batch_host_masked: bad argument");
  DB_POISON_CHK(db, "cc_db_query_batch_host_masked");
  int rc = packed_modes(fn, rank, h_detail);
  if (rc != CC_OK) return rc;
  if (!thres_strict_smaller(lb, ub)) return set_err(CC_EINVAL, "cc_db_query_batch_host_masked: thresholds must satisfy lb.strictSmaller(ub)");
  for (int i = 0; i < nq; i++)
    if (h_epoch[i] < 0 || h_epoch[i] > db->n_scans) return set_err(CC_EINVAL, "cc_db_query_batch_host_masked: epoch out of range");
  if (mask) {  // (before anything is staged: a refused call copies nothing)
    rc = mask_validate(db, mask, nq, h_epoch);
    if (rc != CC_OK) return rc;
  }
  if (nq == 0) return CC_OK;
  HIPCHK(hipSetDevice(db->device));
  rc = stage_reserve(db, nq);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpy(db->d_stage, h_qdesc, sizeof(cc_scan_desc_t) * (size_t)nq, hipMemcpyHostToDevice));
  cc_scan_mask_t dm;
  if (mask) {
    const size_t words = (size_t)mask->n_rows * (size_t)mask->row_words;
    if (words > db->mask_stage_cap) {
      hipFree(db->d_mask_stage);
      db->d_mask_stage = nullptr;
      db->mask_stage_cap = 0;
      HIPCHK(hipMalloc(&db->d_mask_stage, sizeof(uint32_t) * words));
      db->mask_stage_cap = words;
    }
    HIPCHK(hipMemcpy(db->d_mask_stage, mask->bits, sizeof(uint32_t) * words, hipMemcpyHostToDevice));
    dm = *mask;
    dm.bits = db->d_mask_stage;
  }
  return run_sync(db, [&] { return query_submit_impl(db, db->d_stage, nq, h_epoch, lb, ub, h_res, nullptr, nullptr, nullptr, rank, h_detail, nullptr, nullptr, mask ? &dm : nullptr, match); });
}
int cc_db_query_batch_host_masked(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                  const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                                  const cc_scan_mask_t *mask) {
  return query_batch_host_masked_impl(__func__, db, h_qdesc, nq, h_epoch, lb, ub, h_res, rank, h_detail, mask, nullptr);
}

// ---- the matched contour pairs behind each ranked entry (include/cont2_amd_matches.h; k_merge.h: the _m instances, k_match.h) ----
// One entry point per flow with the flow's most general argument list, then `match`; match NULL is the existing call of the same
// arguments.  The refusals of `match` come first (want_match), then the underlying call's.
#define CC_WANT_MATCH()                                        \
  if (match) {                                                 \
    const int mrc_ = want_match(__func__, db, rank, match);    \
    if (mrc_ != CC_OK) return mrc_;                            \
  }
int cc_db_query_submit_matched(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_packed_src_t *src, const int32_t *h_rec, int nq,
                               const int32_t *h_epoch, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn,
                               int32_t *d_knn_cnt, void *stream_, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                               const cc_scan_mask_t *mask, const cc_match_out_t *match) {
  if (!match) return cc_db_query_submit_masked(db, d_qdesc, src, h_rec, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, mask);
  CC_WANT_MATCH();
  if ((d_qdesc != nullptr) == (src != nullptr)) return set_err(CC_EINVAL, "cc_db_query_submit_matched: exactly one of d_qdesc and src must be given");
  int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  if (!src) return query_submit_impl(db, d_qdesc, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, nullptr, nullptr, mask, match);
  cc_rec_src rs;
  vrc = packed_resolve(__func__, db, src, &rs);
  if (vrc != CC_OK) return vrc;
  return query_submit_impl(db, nullptr, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, &rs, h_rec, mask, match);
}
int cc_db_query_batch_host_matched(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                   const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                                   const cc_scan_mask_t *mask, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  return query_batch_host_masked_impl(__func__, db, h_qdesc, nq, h_epoch, lb, ub, h_res, rank, h_detail, mask, match);
}
int cc_db_query_scan_batch_submit_matched(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *lb,
                                          const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank,
                                          cc_ranked_detail_t *h_detail, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  const int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  if (lb && ub && !thres_strict_smaller(lb, ub))  // (before the handles are gathered: a refused call queues nothing)
    return set_err(CC_EINVAL, "cc_db_query_scan_batch_submit_matched: thresholds must satisfy lb.strictSmaller(ub)");
  return query_scan_batch_submit_impl(db, scans, n, h_epoch, lb, ub, h_res, rank, h_detail, match);
}
int cc_db_verify_submit_matched(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const cc_packed_src_t *src, const int32_t *h_qidx,
                                const int32_t *h_cands, int n, const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub,
                                cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints, void *stream_, const cc_rank_out_t *rank,
                                cc_ranked_detail_t *h_detail, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  if ((d_qdesc != nullptr) == (src != nullptr)) return set_err(CC_EINVAL, "cc_db_verify_submit_matched: exactly one of d_qdesc and src must be given");
  int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  if (!src) return verify_submit_impl(db, d_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, d_hints, d_n_hints, stream_, rank, h_detail, nullptr, match);
  cc_rec_src rs;
  vrc = packed_resolve(__func__, db, src, &rs);
  if (vrc != CC_OK) return vrc;
  return verify_submit_impl(db, nullptr, rs.n_rec, h_qidx, h_cands, n, cfg, lb, ub, h_res, d_hints, d_n_hints, stream_, rank, h_detail, &rs, match);
}
int cc_db_verify_batch_host_matched(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands, int n,
                                    const cc_verify_cfg_t *cfg, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res,
                                    const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  const int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  return verify_batch_host_impl(db, h_qdesc, n_desc, h_qidx, h_cands, n, cfg, lb, ub, h_res, rank, h_detail, match);
}
int cc_db_check_hints_matched(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                              const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores, void *stream_,
                              const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  const int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  return check_hints_impl(db, d_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, stream_, rank, h_detail, match);
}
int cc_db_check_hints_host_matched(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *lb,
                                   const cc_score_t *ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores,
                                   const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  const int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  return check_hints_host_impl(db, h_qdesc, h_hints, n_hints, lb, ub, max_fine_opt, h_res, h_scores, rank, h_detail, match);
}

// ---- listed queries: the retrieval among per-query lists of scans (include/cont2_amd_lists.h; k_knn_list.h) ----
// The most general query submit with `lists` in the mask's place.  lists NULL is the call without it, launch for launch.
int cc_db_query_submit_listed(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_packed_src_t *src, const int32_t *h_rec, int nq,
                              const int32_t *h_epoch, const cc_score_t *lb, const cc_score_t *ub, cc_query_result_t *h_res, cc_knn_hit_t *d_knn,
                              int32_t *d_knn_cnt, void *stream_, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                              const cc_scan_lists_t *lists, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  if ((d_qdesc != nullptr) == (src != nullptr)) return set_err(CC_EINVAL, "cc_db_query_submit_listed: exactly one of d_qdesc and src must be given");
  int vrc = packed_modes(__func__, rank, h_detail);
  if (vrc != CC_OK) return vrc;
  if (!src) return query_submit_impl(db, d_qdesc, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, nullptr, nullptr, nullptr, match, lists);
  cc_rec_src rs;
  vrc = packed_resolve(__func__, db, src, &rs);
  if (vrc != CC_OK) return vrc;
  return query_submit_impl(db, nullptr, nq, h_epoch, lb, ub, h_res, d_knn, d_knn_cnt, stream_, rank, h_detail, &rs, h_rec, nullptr, match, lists);
}
// ... with host descriptors: staged on the device, then the submit above and the wait (the lists are host memory either way)
int cc_db_query_batch_host_listed(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *lb,
                                  const cc_score_t *ub, cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                                  const cc_scan_lists_t *lists, const cc_match_out_t *match) {
  CC_WANT_MATCH();
  if (!db || !h_qdesc || nq < 0 || !h_epoch || !lb || !ub || !h_res) return set_err(CC_EINVAL, "cc_db_query_batch_host_listed: bad argument");
  DB_POISON_CHK(db, "cc_db_query_batch_host_listed");
  int rc = packed_modes(__func__, rank, h_detail);
  if (rc != CC_OK) return rc;
  if (!thres_strict_smaller(lb, ub)) return set_err(CC_EINVAL, "cc_db_query_batch_host_listed: thresholds must satisfy lb.strictSmaller(ub)");
  for (int i = 0; i < nq; i++)
    if (h_epoch[i] < 0 || h_epoch[i] > db->n_scans) return set_err(CC_EINVAL, "cc_db_query_batch_host_listed: epoch out of range");
  if (lists) {  // (before anything is staged: a refused call copies nothing)
    rc = lists_validate(__func__, db, lists, nq);
    if (rc != CC_OK) return rc;
  }
  if (nq == 0) return CC_OK;
  HIPCHK(hipSetDevice(db->device));
  rc = stage_reserve(db, nq);
  if (rc != CC_OK) return rc;
  HIPCHK(hipMemcpy(db->d_stage, h_qdesc, sizeof(cc_scan_desc_t) * (size_t)nq, hipMemcpyHostToDevice));
  return run_sync(db, [&] { return query_submit_impl(db, db->d_stage, nq, h_epoch, lb, ub, h_res, nullptr, nullptr, nullptr, rank, h_detail, nullptr, nullptr, nullptr, match, lists, true); });
}
int cc_db_debug_knn_chunks_listed(const cc_db *db, int64_t out[2]) {
  if (!db || !out) return set_err(CC_EINVAL, "cc_db_debug_knn_chunks_listed: bad argument");
  for (int i = 0; i < 2; i++) out[i] = db->knn_chunks_listed[i];
  return CC_OK;
}
#undef CC_WANT_MATCH
// host only: the pairs of a row in key order
int cc_match_pairs(const cc_ranked_match_t *m, cc_match_pair_t *out, int cap) {
  if (!m) return -1;
  int n = 0;
  for (int w = 0; w < 7; w++)
    for (uint64_t b = m->pairs[w]; b; b &= b - 1) {
      const int bit = w * 64 + __builtin_ctzll(b);
      if (out && n < cap) out[n] = cc_match_pair_t{(int8_t)(bit / 100 + 1), (int8_t)((bit % 100) / 10), (int8_t)(bit % 10), 0};
      n++;
    }
  return n;
}

// Parity / debug: which retrieval the query chunks submitted so far ran
int cc_db_debug_knn_chunks(const cc_db *db, int64_t out[3]) {
  if (!db || !out) return set_err(CC_EINVAL, "cc_db_debug_knn_chunks: bad argument");
  for (int i = 0; i < 3; i++) out[i] = db->knn_chunks[i];
  return CC_OK;
}

// Rows of a position prior (k_mask.h): bit g of row r = scan g lies within gate r's circle.  Queued on `stream`.
int cc_mask_gates(cc_ctx *ctx, const float *d_xy, int n_scans, const float *d_gate, int n_rows, uint32_t *d_bits, int row_words, void *stream_) {
  if (!ctx || n_scans < 0 || (n_scans > 0 && !d_xy) || !d_gate || n_rows < 1 || !d_bits || row_words < 1)
    return set_err(CC_EINVAL, "cc_mask_gates: bad argument (n_rows >= 1, row_words >= 1)");
  if ((long long)32 * row_words < (long long)n_scans) return set_err(CC_EINVAL, "cc_mask_gates: 32 * row_words is smaller than n_scans");
  HIPCHK(hipSetDevice(ctx->device));
  const long long blocks = (long long)n_rows * ((row_words + 1) / 2);
  if (blocks > INT_MAX) return set_err(CC_EINVAL, "cc_mask_gates: the table is too large for one launch");
  hipLaunchKernelGGL(cc_k_mask_gates, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream_, d_xy, n_scans, d_gate, (unsigned *)d_bits, row_words);
  HIPCHK(hipGetLastError());
  return CC_OK;
}
