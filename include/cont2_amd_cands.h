/*
 * cont2_amd_cands.h -- the candidates of the last hint call as the merge left them: an extension of cont2_amd.h's C-ABI.
 *
 * One read-only call, the companion of cc_db_debug_passes.  It waits for the work queued so far and copies records the kernels
 * keep anyway; it changes nothing a kernel reads.  Tests use it to see the merged proposal of EVERY candidate of a
 * cc_db_check_hints call, not only of the CC_RANK_MAX ranked ones.
 */
#ifndef CONT2_AMD_CANDS_H
#define CONT2_AMD_CANDS_H
#include "cont2_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t cand_gidx; /* the candidate's database scan                                                                    */
  int32_t n_props;   /* its proposals after the last check was merged (1..4: a fifth is dropped)                         */
  int32_t refined;   /* 1: the candidate passed the area and distance bars and went on to the correlation, else 0        */
  int32_t pad_;
  double tf_init[3]; /* refined = 1: (x, y, theta) of the selected proposal, the correlation's T_init -- what
                        cc_ranked_detail_t.tf_init reports for a ranked entry; zeros otherwise                            */
} cc_cand_dbg_t; /* 40 bytes */

/* The candidates of the last cc_db_check_hints* call on `db`, in first-appearance order (the reference's candidates_ before
 * tidyUpCandidates): at most `cap` records to h_out, their number to *n_out.  Read from the call's own device records after
 * waiting for the queued work; defined only while no other scoring call has run on the database since.  CC_EINVAL: a NULL
 * argument or cap < 0. */
int cc_db_debug_cands(cc_db *db, cc_cand_dbg_t *h_out, int cap, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_CANDS_H */
