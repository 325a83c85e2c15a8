/*
 * cont2_amd_paths.h -- which body of the contour kernel took a context's scans: an extension of cont2_amd.h's C-ABI.
 *
 * One read-only call.  It waits for the ingest work queued so far and copies counters the kernels keep anyway; it changes nothing
 * a kernel reads.  Tests use it to hold a scene to the body it was built for; an integrator can use it to see how often its scans
 * leave the fast path.
 */
#ifndef CONT2_AMD_PATHS_H
#define CONT2_AMD_PATHS_H
#include "cont2_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Which body of the contour kernel took the context's scans (read-only; counted since cc_create, never reset).  Every scan starts in
 * the list kernel; one that does not fit it is handed to the original body (cc_k_contours_mid), and what that cannot number to the
 * slow exact one (cc_k_contours_big).  out[0]: scans ever handed to the mid body; out[1..4]: those by reason -- the configuration
 * (min_cont_cell_cnt > 3), more entries or slots than the list holds, more than CC_MAXC components on a level, member lists that
 * outgrow their block through padding --; out[5]: scans ever handed on to the big body.  Summed over the context's scratch sets (the
 * batched calls' and the per-scan loop's channels).  The call waits for the ingest work queued so far, then copies the counters: it
 * changes nothing a kernel reads.  The difference of two readings counts the calls between them. */
int cc_ingest_path_counts(cc_ctx *ctx, int32_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* CONT2_AMD_PATHS_H */
