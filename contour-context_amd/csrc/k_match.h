// K6b -- the matched contour pairs behind each ranked entry (include/cont2_amd_matches.h): cc_k_match_emit, behind cc_k_final_r*
// in the tail of a chunk that asked for matches.
#pragma once
#include "../../include/cont2_amd_matches.h"
#include "cc_dev.h"
#include "cc_group.h"
#include "k_merge.h"

// ------------------------------------------------------------------------------------------------
// One wave per query.  cc_k_final_r* left the query's list in rank[q][max_ret] and its counters in res[q]; the matched merge
// instance left the selected proposal of every correlation problem in mrec[problem].  For entry k of the list:
//   * the entry's candidate is the one of the query's candidates whose scan is the entry's (a scan is a candidate once) and that
//     has a problem: the lanes look through cands[0 .. n_cand), lane k keeps entry k's problem;
//   * bit b of the proposal's 400-bit set belongs to lane b & 63 in round b >> 6: the lane decodes (level, seq_src, seq_tgt),
//     gathers the two pos_mean from the hot records (both hold cont[level-1][seq] for every seq < CC_NDIST) and evaluates
//     r = T p_src - p_tgt in f64 at the entry's returned tf;
//   * sum |r|^2, max |r| and the two counts are reduced over the wave (cc_group.h), lane 0 writes the 96-byte row.
// Rows at or beyond the list's length are zeroed here.  No atomics, no LDS, no scratch: every array index is a constant
// after unrolling.
// grid = nq, block = 64.  KM: hits per search of the chain (the stride of cands_all).
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(cc_ranked_match_t) == 96 && sizeof(cc_ranked_match_t) % 8 == 0, "cc_k_match_emit zeroes a row as twelve 8-byte words");
static_assert(CC_RANK_MAX <= 64, "lane k keeps entry k's problem");
static_assert(CC_HOT_LEVELS * 100 <= 7 * 64, "a proposal's set is seven words");

template <int KM>
__device__ __forceinline__ void cc_match_emit_body(int nq, int max_ret, int max_fine_opt, double inlier_px, const cc_query_result_t *res,
                                                   const cc_ranked_cand_t *rank /*[nq][max_ret]*/, const cc_cand_out *cands_all,
                                                   const cc_qstate *qstate, const cc_match_rec *mrec, const cc_hot_desc_t *qhot,
                                                   const cc_hot_desc_t *dbhot, cc_ranked_match_t *out /*[nq][max_ret]*/) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= nq) return;
  // the list's length, as rank_deliver computes h_n from the same record
  int ret = 0;
  {
    const int n_res = res[q].n_res, n_tidy = res[q].n_cand_tidy;
    const int pre = max_fine_opt < n_tidy ? max_fine_opt : n_tidy;
    if (n_res > 0) ret = max_ret < pre ? max_ret : pre;
  }
  ret = cc_uniform_i(ret);
  const int nc = cc_uniform_i(qstate[q].n_cand);
  const cc_ranked_cand_t *row = rank + (size_t)q * max_ret;
  cc_ranked_match_t *orow = out + (size_t)q * max_ret;
  // the rows behind the list
  {
    unsigned long long *z = (unsigned long long *)(orow + ret);
    const int nz = (max_ret - ret) * (int)(sizeof(cc_ranked_match_t) / 8);
    for (int i = lane; i < nz; i += 64) z[i] = 0ull;
  }
  // lane k: entry k's scan, and (after the loop) its problem
  const int my_g = lane < ret ? row[lane].cand_gidx : -1;
  int my_gi = -1;
  const cc_cand_out *cands = cands_all + (size_t)q * CC_CHK_STRIDE_K(KM);
  for (int k0 = 0; k0 < nc; k0 += 64) {
    const int k = k0 + lane;
    int cg = -1, gm = -1;
    if (k < nc) {
      cg = cands[k].gidx;
      gm = cands[k].gmm_idx;
    }
    for (int e = 0; e < ret; e++) {
      const int ge = __shfl(my_g, e);
      const unsigned long long m = __ballot(gm >= 0 && cg == ge);
      const int src = m ? __ffsll(m) - 1 : 0;
      const int v = __shfl(gm, src);
      if (m && lane == e) my_gi = v;
    }
  }
  for (int e = 0; e < ret; e++) {
    const int gi = cc_uniform_i(__shfl(my_gi, e));
    const cc_ranked_cand_t en = row[e];
    unsigned long long bits[7] = {0, 0, 0, 0, 0, 0, 0};
    int vote_cnt = 0, nprops = 0;
    float area = 0.f;
    if (gi >= 0) {
      const cc_match_rec *mr = mrec + gi;
#pragma unroll
      for (int w = 0; w < 7; w++) bits[w] = mr->bits[w];
      vote_cnt = mr->vote_cnt;
      nprops = mr->nprops;
      area = mr->area_perc;
    }
    double sn, cs;
    sincos(en.tf[2], &sn, &cs);
    const double tx = en.tf[0], ty = en.tf[1];
    const cc_hot_desc_t *sd = dbhot + en.cand_gidx, *td = qhot + q;
    double sum = 0.0, mx = 0.0;
    int cnt = 0;  // pairs | inliers << 16 (each <= 400)
#pragma unroll
    for (int w = 0; w < 7; w++) {
      const int b = w * 64 + lane;
      if (b < CC_HOT_LEVELS * 100 && ((bits[w] >> lane) & 1ull)) {  // (the merge sets no bit at or beyond 400: the records' bounds do not depend on it)
        const int l = b / 100, s_ = (b % 100) / 10, t_ = b % 10;
        const double sx = (double)sd->cont[l][s_].pos_mean[0], sy = (double)sd->cont[l][s_].pos_mean[1];
        const double px = (double)td->cont[l][t_].pos_mean[0], py = (double)td->cont[l][t_].pos_mean[1];
        const double rx = (cs * sx - sn * sy + tx) - px, ry = (sn * sx + cs * sy + ty) - py;
        const double d = sqrt(rx * rx + ry * ry);
        sum += rx * rx + ry * ry;
        mx = fmax(mx, d);
        cnt += 1 + (d <= inlier_px ? 1 << 16 : 0);
      }
    }
    sum = cc_wave_sum_d(sum);
    mx = cc_wave_max_d(mx);
    cnt = cc_wave_scan_total(cc_wave_scan_incl(cnt));
    if (lane == 0) {
      cc_ranked_match_t o;
#pragma unroll
      for (int w = 0; w < 7; w++) o.pairs[w] = bits[w];
      const int np = cnt & 0xFFFF;
      o.n_pairs = np;
      o.vote_cnt = vote_cnt;
      o.n_props = nprops;
      o.area_perc = area;
      o.res_rms = np > 0 ? sqrt(sum / (double)np) : 0.0;
      o.res_max = mx;
      o.n_inlier = cnt >> 16;
      o.flags = en.flags;
      orow[e] = o;
    }
  }
}

__global__ void __launch_bounds__(64)
cc_k_match_emit(int nq, int max_ret, int max_fine_opt, double inlier_px, const cc_query_result_t *__restrict__ res,
                const cc_ranked_cand_t *__restrict__ rank, const cc_cand_out *__restrict__ cands_all, const cc_qstate *__restrict__ qstate,
                const cc_match_rec *__restrict__ mrec, const cc_hot_desc_t *__restrict__ qhot, const cc_hot_desc_t *__restrict__ dbhot,
                cc_ranked_match_t *__restrict__ out) {
  cc_match_emit_body<CC_KNN_MAX>(nq, max_ret, max_fine_opt, inlier_px, res, rank, cands_all, qstate, mrec, qhot, dbhot, out);
}
// the large-k instance: CC_CHK_STRIDE_K(CC_KNN_MAX_LARGE) candidate slots per query
__global__ void __launch_bounds__(64)
cc_k_match_emit_l(int nq, int max_ret, int max_fine_opt, double inlier_px, const cc_query_result_t *__restrict__ res,
                  const cc_ranked_cand_t *__restrict__ rank, const cc_cand_out *__restrict__ cands_all, const cc_qstate *__restrict__ qstate,
                  const cc_match_rec *__restrict__ mrec, const cc_hot_desc_t *__restrict__ qhot, const cc_hot_desc_t *__restrict__ dbhot,
                  cc_ranked_match_t *__restrict__ out) {
  cc_match_emit_body<CC_KNN_MAX_LARGE>(nq, max_ret, max_fine_opt, inlier_px, res, rank, cands_all, qstate, mrec, qhot, dbhot, out);
}
