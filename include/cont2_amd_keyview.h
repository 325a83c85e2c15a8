/*
 * cont2_amd_keyview.h -- a layer's sorted key view as the last append left it: an extension of cont2_amd.h's C-ABI.
 *
 * One read-only call, the companion of cc_db_debug_cands.  It waits for the work queued so far, the pending append included,
 * and copies the buffer of the view the next query chunk would read; it changes nothing a kernel reads.  Tests use it to hold
 * the view's order, its key bits, its activation epochs and its |key|^2 row after every append.
 */
#ifndef CONT2_AMD_KEYVIEW_H
#define CONT2_AMD_KEYVIEW_H
#include "cont2_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The sorted view of query layer `layer` (0 .. n_q_levels - 1) of `db`: *n = the layer's keys; when *n <= cap, keys[d * cap + i]
 * (d = 0 .. CC_KEY_DIM - 1) is entry d of the i-th key in the view's order, keys[CC_KEY_DIM * cap + i] the view's |key|^2 of it,
 * sid[i] its key id (its place in the layer's insertion order) and sact[i] the first epoch at which it sits in a tree.  When
 * *n > cap nothing else is written and the call returns CC_ECAPACITY.  All arrays are host memory: keys (CC_KEY_DIM + 1) * cap
 * floats, sid and sact cap ints.  CC_EINVAL: a NULL argument, cap < 0 or a layer the database does not query. */
int cc_db_debug_key_view(cc_db *db, int layer, int cap, float *keys, int32_t *sid, int32_t *sact, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_KEYVIEW_H */
