/*
 * cont2_amd_lists.h -- queries among per-query LISTS of database scans: an extension of cont2_amd.h's C-ABI.
 *
 * A mask (cc_scan_mask_t, cont2_amd.h: "masked queries") names the scans that may answer a query as a bit row of the whole
 * database, in device memory, and its retrieval walks the layer and tests every key's scan.  A back end that gates by position
 * already HAS index lists -- the result of a radius search over its poses -- and they are short.  The listed form takes them
 * as they are, from host memory, and its retrieval (csrc/k_knn_list.h) enumerates the keys of the listed scans only: its cost
 * follows the list, not the map (measured: DESIGN.md 3.13 -- a tenth of the mask form's retrieval time at 71 scans per list on a
 * 5 000-scan map, equal to it near 960 scans per list).
 *
 * Semantics: a query that names list r behaves exactly like the query of the mask form whose row has the bits of list r set
 * (cont2_amd.h: the reference's trees filtered to the allowed scans, bucket ranges left alone) -- result records, ranked lists,
 * detail rows, match rows, hit tables and counts are that call's, to the bit.  Epoch and list are ANDed: an entry at or above
 * the query's epoch is legal and never answers.  An empty list answers nothing.  h_row[i] = -1: every scan may answer.
 *
 * Memory: everything a cc_scan_lists_t points to is HOST memory and is read before the submit returns; there is no lifetime
 * rule.  The library stages per chunk what its kernel needs (16 bytes per listed scan; a list shared by several queries of a
 * chunk is staged once) in buffers that are allocated with a handle's first listed call and grow to the largest chunk seen.
 *
 * Which retrieval a chunk runs:
 *   every query of the chunk names a list   the list retrieval alone;
 *   none does                               exactly what the chunk launches without `lists`;
 *   some do                                 first the unrestricted retrieval of the whole chunk (one wave per search, tiled or
 *                                           large-k, as the database would choose), then the list retrieval, which overwrites the
 *                                           hit tables of the queries that name a list and leaves the others alone.  Such a chunk
 *                                           COSTS BOTH retrievals and is correct; callers that care group their queries.
 * lists NULL is the call without it, byte for byte and launch for launch.
 *
 * Refused with CC_EINVAL (cc_last_error names the cause) before anything is queued, the handle stays usable:
 * n_lists < 1, or h_off not non-decreasing from 0; an h_row[i] outside [-1, n_lists); a list that is not strictly increasing;
 * an entry outside [0, cc_db_size); a list longer than CC_LIST_SCANS_MAX (use the mask form for larger sets); a database in
 * cc_db_set_dynamic_thres mode (as for masks: no test oracle exists); not exactly one of d_qdesc and src; and whatever the
 * call without `lists` refuses.
 */
#ifndef CONT2_AMD_LISTS_H
#define CONT2_AMD_LISTS_H
#include "cont2_amd.h"
#include "cont2_amd_matches.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CC_LIST_SCANS_MAX 1024 /* scans per list: a capacity (a full chunk of full lists stages 16 MB per lane), not a measurement */

typedef struct cc_scan_lists {
  const int32_t *h_idx;  /* host: the lists, one after another                                   */
  const int32_t *h_off;  /* host [n_lists + 1]: list r is h_idx[h_off[r] .. h_off[r + 1])         */
  int32_t n_lists;
  const int32_t *h_row;  /* host [nq]: the list of query i, or -1: every scan may answer          */
} cc_scan_lists_t;

/* The most general query submit: the mask form's argument list with `lists` in the place of the mask, then `match`
 * (cont2_amd_matches.h; NULL: no match rows).  Exactly one of d_qdesc and src is given; src, h_rec, rank and h_detail mean what
 * they mean in cc_db_query_submit_packed. */
int cc_db_query_submit_listed(cc_db *db, const cc_scan_desc_t *d_qdesc, const cc_packed_src_t *src, const int32_t *h_rec, int nq,
                              const int32_t *h_epoch, const cc_score_t *thres_lb, const cc_score_t *thres_ub, cc_query_result_t *h_res,
                              cc_knn_hit_t *d_knn, int32_t *d_knn_cnt, void *stream, const cc_rank_out_t *rank,
                              cc_ranked_detail_t *h_detail, const cc_scan_lists_t *lists, const cc_match_out_t *match);
/* host descriptors, staged by the call; synchronous */
int cc_db_query_batch_host_listed(cc_db *db, const cc_scan_desc_t *h_qdesc, int nq, const int32_t *h_epoch, const cc_score_t *thres_lb,
                                  const cc_score_t *thres_ub, cc_query_result_t *h_res, const cc_rank_out_t *rank,
                                  cc_ranked_detail_t *h_detail, const cc_scan_lists_t *lists, const cc_match_out_t *match);
/* Parity / debug: the query chunks submitted on this handle so far that ran ONLY the list retrieval (out[0]) and that ran both
 * (out[1]).  cc_db_debug_knn_chunks keeps its meaning: a chunk of out[0] counts in none of its three, a chunk of out[1] in the
 * one of the unrestricted retrieval it ran first. */
int cc_db_debug_knn_chunks_listed(const cc_db *db, int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_LISTS_H */
