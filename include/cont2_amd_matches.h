/*
 * cont2_amd_matches.h -- the matched contour pairs behind each ranked loop candidate: an extension of cont2_amd.h's C-ABI.
 *
 * A ranked entry (cc_ranked_cand_t) is a scan, a correlation and a pose; cc_ranked_detail_t adds the curvature at that pose.
 * The evidence the pose was built from is the constellation of the proposal tidyUpCandidates selects: anch_props_[0].constell_
 * after its std::swap (contour_db.h:267-338, 503-528), the ConstellationPair{level, seq_src, seq_tgt} set the reference keeps in
 * its CandidateManager and its drivers draw.  The *_matched entry points hand it out per ranked entry, together with how well
 * those pairs still agree with the pose the entry returns.
 *
 * Each flow has ONE matched entry point, carrying the flow's most general argument list (the precedent of the _packed and _masked
 * forms) followed by `match`:
 *   match NULL    the existing call of the same arguments, byte for byte and launch for launch.
 *   match given   h_res, the ranked lists, the detail rows, the hit lists and the flags are the bytes the call returns without
 *                 it.  Row i / entry k of h_match belongs to rank->h_cands[i][k]; the rows of a chunk arrive with its h_cands rows
 *                 (cc_db_query_wait / cc_db_query_collect, or the synchronous call's return), so the buffer must stay valid until
 *                 then.  Entries at or beyond rank->h_n[i] are zeroed (by the kernel that writes the rows).  Chunking, lanes,
 *                 epochs, masks, stored and packed queries and large-k databases are the ranked call's.
 * Refused with CC_EINVAL before anything is queued (the handle stays usable): match without rank; h_match NULL; inlier_px negative,
 * NaN or infinite; a database in cc_db_set_dynamic_thres mode (under rising bars which checks pass depends on the order of ALL
 * of a query's checks, and no test oracle for merged constellations under those bars exists: the precedent of the masked form);
 * and whatever the underlying call refuses.  The pose flow (cc_db_pose_*) has no constellation and no matched form.
 */
#ifndef CONT2_AMD_MATCHES_H
#define CONT2_AMD_MATCHES_H
#include "cont2_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t pairs[7];  /* constell_ of the selected proposal as a set: bit (level-1)*100 + seq_src*10 + seq_tgt
                         (cc_pass_dbg_t.pairs' code; ascending bit order == ConstellationPair::operator<)          */
  int32_t n_pairs;    /* constell_.size()                                                                         */
  int32_t vote_cnt;   /* anch_props_[0].vote_cnt_ (counts every merged check's pairs, not unique ones)            */
  int32_t n_props;    /* anch_props_.size(), 1..4                                                                 */
  float area_perc;    /* anch_props_[0].area_perc_                                                                */
  double res_rms;     /* over the pairs, at the ENTRY'S tf: r_i = T * p_src_i - p_tgt_i, T = [c -s x; s c y],     */
  double res_max;     /*   p_src = pos_mean of the database scan's contour (level, seq_src), p_tgt = the query's  */
                      /*   (level, seq_tgt), both as double; rms = sqrt(sum |r_i|^2 / n_pairs), max = max |r_i|   */
  int32_t n_inlier;   /* pairs with sqrt(rx*rx + ry*ry) <= inlier_px                                              */
  int32_t flags;      /* == cc_ranked_cand_t.flags of the entry                                                   */
} cc_ranked_match_t;  /* 96 bytes */
#ifdef __cplusplus
static_assert(sizeof(cc_ranked_match_t) == 96, "cc_ranked_match_t is 96 bytes");
#else
_Static_assert(sizeof(cc_ranked_match_t) == 96, "cc_ranked_match_t is 96 bytes");
#endif

typedef struct {
  cc_ranked_match_t *h_match; /* [n][rank->max_ret], host; row i / entry k belongs to rank->h_cands[i][k]; entries >= h_n[i] zeroed */
  double inlier_px;           /* >= 0, finite */
} cc_match_out_t;

/* The direction of T is the one getTFFromConstell fits (contour_mng.h:1246-1277): source = the database scan, target = the query. */

typedef struct {
  int8_t level, seq_src, seq_tgt, pad;
} cc_match_pair_t;
/* Host only: the pairs of a row in key order (ascending bit), at most `cap` of them to `out` (which may be NULL with cap 0).
 * Returns the number of set bits (== n_pairs of a row the library wrote); -1 for a NULL row. */
int cc_match_pairs(const cc_ranked_match_t *m, cc_match_pair_t *out, int cap);

/* cc_db_query_submit_masked's arguments, then match */
int cc_db_query_submit_matched(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_packed_src_t *src, const int32_t *h_rec, int nq,
                               const int32_t *h_epoch, const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res,
                               cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream, const cc_rank_out_t *rank,
                               cc_ranked_detail_t *h_detail, const cc_scan_mask_t *mask, const cc_match_out_t *match);
/* descriptors (d_qdesc, n_desc) or a record source (src, then n_desc is not read): exactly one of them */
int cc_db_verify_submit_matched(cc_db *db, const cc_scan_desc_t *d_qdesc, int n_desc, const cc_packed_src_t *src, const int32_t *h_qidx,
                                const int32_t *h_cands, int n, const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb,
                                const cc_score_t *thres_ub, cc_query_result_t *h_res, cc_hint_t *d_hints, int32_t *d_n_hints, void *stream,
                                const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail, const cc_match_out_t *match);
/* synchronous; n = 1 */
int cc_db_check_hints_matched(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_hint_t *h_hints, int n_hints, const cc_score_t *thres_lb,
                              const cc_score_t *thres_ub, int max_fine_opt, cc_query_result_t *h_res, cc_hint_score_t *h_scores,
                              void *stream, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail, const cc_match_out_t *match);
/* scan handles (the class mirror's read-ahead) */
int cc_db_query_scan_batch_submit_matched(cc_db *db, cc_scan *const *scans, int n, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                          const cc_score_t *thres_ub, cc_query_result_t *h_res, const cc_rank_out_t *rank,
                                          cc_ranked_detail_t *h_detail, const cc_match_out_t *match);
/* the synchronous host forms */
int cc_db_query_batch_host_matched(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                   const cc_score_t *thres_ub, cc_query_result_t *h_res, const cc_rank_out_t *rank,
                                   cc_ranked_detail_t *h_detail, const cc_scan_mask_t *mask, const cc_match_out_t *match);
int cc_db_verify_batch_host_matched(cc_db *db, const cc_scan_desc_t *h_qdesc, int n_desc, const int32_t *h_qidx, const int32_t *h_cands,
                                    int n, const cc_verify_cfg_t *cfg, const cc_score_t *thres_lb, const cc_score_t *thres_ub,
                                    cc_query_result_t *h_res, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                                    const cc_match_out_t *match);
int cc_db_check_hints_host_matched(cc_db *db, const cc_scan_desc_t *h_qdesc, const cc_hint_t *h_hints, int n_hints,
                                   const cc_score_t *thres_lb, const cc_score_t *thres_ub, int max_fine_opt, cc_query_result_t *h_res,
                                   cc_hint_score_t *h_scores, const cc_rank_out_t *rank, cc_ranked_detail_t *h_detail,
                                   const cc_match_out_t *match);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_MATCHES_H */
