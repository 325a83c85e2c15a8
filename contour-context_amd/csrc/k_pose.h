// K5p -- caller-given relative poses (cc_db_pose_*): ConstellCorrelation's public interface (correlation.h:175-238) in batch.
// Item i of a chunk = (query descriptor, database scan, T_init) is correlation problem i of the chunk, with query record i:
//
//   cc_k_pose_problems  the problem table cc_k_merge writes in a query chain, straight from the items: slot i, listed at i
//   (cc_k_gmm_init)     initProblem: pair selection at T_init, the initial correlation, the problem's pair-code list
//   cc_k_pose_select    the problems calcCorrelation() runs on -- refine asked for, pairs > 0, !((float)corr_init < min_corr) --
//                       filed where cc_k_select files a query chain's: the three lists by pair count, the long ones by length
//                       class, each problem's share of the pair pool.  No tidyUp replay, no permutation, no max_fine_opt.
//   (cc_k_gmm_refine)   both instances, as they are
//   cc_k_pose_eval      tryProblem at the chunk's n_try poses per item over the pair set of T_init (cost only), and -- where
//                       asked for -- the curvature at the returned pose (cc_gmm_hess_one, k_gmm_hess.h); every problem of the
//                       chunk, refined or not
//   cc_k_pose_final     the 64-byte row per item
//
// cc_k_pose_eval builds a pair once (cc_gmm_make_pair: the pose-independent half) and evaluates the term at every try pose:
// what a further pose costs is the ~60 f64 instructions of cc_gmm_term's value, not a second walk of the code list and a
// second gather of the ellipses.  The per-try (x, y, cos, sin, cos 2t, sin 2t) are the same for all lanes: they sit in LDS and
// are read with broadcast reads, so eight poses do not take 96 registers per lane.
#pragma once
#include "k_gmm.h"
#include "k_gmm_hess.h"

static_assert(sizeof(cc_pose_item_t) == 32 && sizeof(cc_pose_result_t) == 64 && sizeof(cc_pose_curv_t) == 72, "cont2_amd.h");
static_assert(sizeof(cc_pose_curv_t) == sizeof(cc_gmm_hess), "nine doubles: (hess | grad) here, (grad | hess) there");

// grid = ceil(n / 256), block = 256: one lane per item
__global__ void __launch_bounds__(256)
cc_k_pose_problems(const cc_pose_item_t *__restrict__ items, int n, cc_gmm_problem *__restrict__ probs, int *__restrict__ prob_list,
                   int *__restrict__ n_prob) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i == 0) *n_prob = n;
  if (i >= n) return;
  const cc_pose_item_t it = items[i];
  cc_gmm_problem pb;
  pb.q = i;  // the chunk's query record i was built from descriptor it.q (launch_query_prep's selector)
  pb.gidx = it.gidx;
  pb.tf[0] = it.tf[0];
  pb.tf[1] = it.tf[1];
  pb.tf[2] = it.tf[2];
  probs[i] = pb;
  prob_list[i] = i;
}

// grid = ceil(n / 64), block = 64: one lane per problem slot, one atomic per list (and per length class that occurs) per
// workgroup -- the filing of cc_select_body with "the first max_fine_opt survivors of the query" replaced by "the slots of
// this wave that are to be refined"
__global__ void __launch_bounds__(64)
cc_k_pose_select(int n, float corr_lb, const cc_gmm_result *__restrict__ gres, int *__restrict__ sel_list /*[3][sel_stride]*/, int sel_stride,
                 int *__restrict__ n_sel /*[2]*/, int *__restrict__ n_sel_wide, int *__restrict__ cls_list /*[CC_GMM_NCLS][sel_stride]*/,
                 int *__restrict__ cls_cnt /*[CC_GMM_NCLS]*/, int *__restrict__ pool_head, int *__restrict__ pool_off /*[problem slot]*/) {
  const int lane = threadIdx.x, g = (int)blockIdx.x * 64 + lane;
  int np = 0;
  if (g < n) {
    const cc_gmm_result *r = &gres[g];
    np = r->n_pairs;
    if ((float)r->corr_init < corr_lb) np = 0;
  }
  const bool take = np > 0;
  const bool big = take && np > CC_GMM_MID_MAX_PAIRS, wide = take && np > CC_GMM_G16_MAX_PAIRS && np <= CC_GMM_MID_MAX_PAIRS,
             small = take && !big && !wide;
  const unsigned long long mbig = __ballot(big), mw = __ballot(wide), msm = __ballot(small);
  if (!(mbig | mw | msm)) return;  // (uniform)
  const unsigned long long lt = (1ull << lane) - 1ull;
  // the part of a problem's records that does not stay in LDS, an even count (an in-between problem: the smaller share,
  // whichever instance takes it)
  const int nl = big ? CC_GMM_NL : CC_GMM_NL / (64 / CC_G);
  const int need = take && np > nl ? ((np - nl + 1) & ~1) : 0;
  int incl = need;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  const int need_tot = __shfl(incl, 63);
  int off = 0;
  {  // the four requests at once, from four lanes
    int *const dst = lane == 0 ? &n_sel[0] : (lane == 1 ? &n_sel[1] : (lane == 2 ? n_sel_wide : pool_head));
    const int amt = lane == 0 ? __popcll(msm) : (lane == 1 ? __popcll(mbig) : (lane == 2 ? __popcll(mw) : need_tot));
    if (lane < 4 && amt) off = atomicAdd(dst, amt);
  }
  const int o_small = __shfl(off, 0), o_wide = __shfl(off, 2), o_pool = __shfl(off, 3);
  if (take) pool_off[g] = o_pool + incl - need;
  if (wide) sel_list[2 * (size_t)sel_stride + o_wide + __popcll(mw & lt)] = g;
  if (small) sel_list[o_small + __popcll(msm & lt)] = g;
  if (mbig) {  // (uniform) one atomic per class that occurs
    const int c = big ? cc_gmm_len_class(np) : -1;
    for (unsigned long long left = mbig; left;) {
      const int c0 = __shfl(c, __ffsll(left) - 1);
      const unsigned long long mc = __ballot(c == c0);
      int base = 0;
      if (lane == __ffsll(mc) - 1) base = atomicAdd(&cls_cnt[c0], __popcll(mc));
      base = __shfl(base, __ffsll(mc) - 1);
      if (c == c0) cls_list[(size_t)c0 * sel_stride + base + __popcll(mc & lt)] = g;
      left &= ~mc;
    }
  }
}

// The cost at n_try poses over one problem's code list: the walk of cc_gmm_hess_one (block header a block ahead, codes a
// sub-batch ahead, the 2 U ellipses of a sub-batch requested together), each pair built once.  tp[t] = (x, y, cos, sin,
// cos 2t, sin 2t) of try t, in LDS.  n_try is uniform over the launch: the unrolled loop's accumulators are registers.
#define CC_POSE_TP 6
template <int G>
__device__ __forceinline__ void cc_pose_try_one(const unsigned *__restrict__ codes, int blk, const cc_gmm_feat *__restrict__ fsrc,
                                                const cc_gmm_feat *__restrict__ ftgt, int sl, int n_try, const double (*tp)[CC_POSE_TP],
                                                const double *exp_tab, double (&sum)[CC_POSE_TRY_MAX]) {
  double acc[CC_POSE_TRY_MAX];
#pragma unroll
  for (int t = 0; t < CC_POSE_TRY_MAX; t++) acc[t] = 0.0;
  int done = 0, n = 0, nxt = -1;
  if (blk >= 0) {
    n = (int)codes[blk];
    nxt = (int)codes[blk + 1];
  }
  while (blk >= 0) {
    int n2 = 0, nxt2 = -1;
    if (nxt >= 0) {
      n2 = (int)codes[nxt];
      nxt2 = (int)codes[nxt + 1];
    }
    const unsigned *cb = codes + blk + 2;
    int e0 = sl - done % G;
    e0 = e0 < 0 ? e0 + G : e0;
    constexpr int U = 2;
    unsigned cc_[U];
#pragma unroll
    for (int u = 0; u < U; u++) cc_[u] = e0 + u * G < n ? cb[e0 + u * G] : 0u;
    for (; e0 < n; e0 += U * G) {
      cc_ell es[U], et[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        es[u] = cc_ell{};
        et[u] = cc_ell{};
        if (e0 + u * G < n) {
          es[u] = cc_gmm_ell_of(fsrc, (int)cc_[u] >> 18, ((int)cc_[u] >> 9) & 511);
          et[u] = cc_gmm_ell_of(ftgt, (int)cc_[u] >> 18, (int)cc_[u] & 511);
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int en = e0 + (U + u) * G;
        cc_[u] = en < n ? cb[en] : 0u;
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (e0 + u * G < n) {
          const cc_gpair P = cc_gmm_make_pair(es[u], et[u]);
#pragma unroll
          for (int t = 0; t < CC_POSE_TRY_MAX; t++)
            if (t < n_try) acc[t] += cc_gmm_term(P, tp[t][0], tp[t][1], tp[t][2], tp[t][3], tp[t][4], tp[t][5], exp_tab).v;
        }
      }
    }
    done += n;
    blk = nxt;
    n = n2;
    nxt = nxt2;
  }
#pragma unroll
  for (int t = 0; t < CC_POSE_TRY_MAX; t++) sum[t] = t < n_try ? cc_gsum<G>(acc[t]) : 0.0;
}

// grid = any (grid-stride over the chunk's problem list: every item), block = 64: one wave per problem.  No atomics.
__global__ void __launch_bounds__(64)
cc_k_pose_eval(const cc_gmm_problem *__restrict__ probs, const int *__restrict__ prob_list, const int *__restrict__ n_prob_p,
               const cc_gmm_feat *__restrict__ qfeat, const cc_gmm_feat *__restrict__ db_feat, const cc_gmm_result *__restrict__ results,
               const unsigned *__restrict__ codes, int n_try, const double *__restrict__ tries /*[slot][n_try][3]*/,
               double *__restrict__ try_out /*[slot][n_try]*/, cc_pose_curv_t *__restrict__ curv_out /*[slot], or nullptr: not wanted*/) {
  __shared__ double exp_tab[64];
  __shared__ double s_tp[CC_POSE_TRY_MAX][CC_POSE_TP];
  exp_tab[threadIdx.x] = __longlong_as_double((long long)cc_exp2_tab64[threadIdx.x]);
  cc_wave_sync();
  const int sl = threadIdx.x;
  const int n_prob = *n_prob_p;
  for (int k = blockIdx.x; k < n_prob; k += gridDim.x) {
    const int pidx = cc_uniform_i(prob_list[k]);
    const cc_gmm_result *R = &results[pidx];
    const cc_gmm_problem *pb = &probs[pidx];
    const cc_gmm_feat *fsrc = db_feat + pb->gidx;
    const cc_gmm_feat *ftgt = qfeat + pb->q;
    const int seg = cc_uniform_i(R->code_seg);
    const bool walk = seg >= 0 && cc_uniform_i(R->n_pairs) > 0;
    if (n_try > 0) {
      double v = 0.0;  // a problem without pairs: 0
      if (walk) {
        cc_wave_sync();  // the previous problem's poses are no longer read
        if (sl < n_try) {
          const double *t = tries + ((size_t)pidx * n_try + sl) * 3;
          double c, s;
          sincos(t[2], &s, &c);
          s_tp[sl][0] = t[0];
          s_tp[sl][1] = t[1];
          s_tp[sl][2] = c;
          s_tp[sl][3] = s;
          s_tp[sl][4] = c * c - s * s;
          s_tp[sl][5] = 2.0 * s * c;
        }
        cc_wave_sync();
        double sum[CC_POSE_TRY_MAX];
        cc_pose_try_one<64>(codes, seg, fsrc, ftgt, sl, n_try, s_tp, exp_tab, sum);
        double cost = sum[0];
#pragma unroll
        for (int t = 1; t < CC_POSE_TRY_MAX; t++) cost = sl == t ? sum[t] : cost;
        v = -cost / sqrt(fsrc->ac * ftgt->ac);
      }
      if (sl < n_try) try_out[(size_t)pidx * n_try + sl] = v;
    }
    if (curv_out) {
      double v = 0.0;
      if (walk) {
        const double x[3] = {R->tf_opt[0], R->tf_opt[1], R->tf_opt[2]};
        double sum[10];
        cc_gmm_hess_one<64>(codes, seg, fsrc, ftgt, sl, x, exp_tab, sum);
        // lanes 0..5: hess (sum[4..9]), lanes 6..8: grad (sum[1..3]) of f = -correlation = cost / sqrt(ac_src ac_tgt)
        v = sum[4];
#pragma unroll
        for (int j = 1; j < 6; j++) v = sl == j ? sum[4 + j] : v;
#pragma unroll
        for (int j = 0; j < 3; j++) v = sl == 6 + j ? sum[1 + j] : v;
        v *= 1.0 / sqrt(fsrc->ac * ftgt->ac);
      }
      if (sl < 9) ((double *)&curv_out[pidx])[sl] = v;
    }
  }
}

// grid = ceil(n / 256), block = 256: one lane per item
__global__ void __launch_bounds__(256)
cc_k_pose_final(const cc_pose_item_t *__restrict__ items, int n, const cc_gmm_result *__restrict__ gres, cc_pose_result_t *__restrict__ out,
                const int *__restrict__ nprob /*[4] the chunk's counters*/, int *__restrict__ nprob_out /*[4] pinned (small chunks), or nullptr*/) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (nprob_out && i < 4) nprob_out[i] = nprob[i];
  if (i >= n) return;
  const cc_gmm_result g = gres[i];
  cc_pose_result_t r;
  r.corr_init = g.corr_init;
  r.n_pairs = g.n_pairs;
  r.flags = ((g.flags & 1) ? CC_QF_GMM_CAP : 0) | ((g.flags & 4) ? CC_QF_DESC_CAP : 0);
  r.pad_[0] = r.pad_[1] = 0;
  double th;
  if (g.optimized) {
    r.correlation = g.corr_opt;
    r.tf[0] = g.tf_opt[0];
    r.tf[1] = g.tf_opt[1];
    th = g.tf_opt[2];
    r.iterations = g.iterations;
    r.termination = g.termination;
    r.flags |= CC_PF_REFINED;
  } else {
    r.correlation = g.corr_init;
    r.tf[0] = items[i].tf[0];
    r.tf[1] = items[i].tf[1];
    th = items[i].tf[2];
    r.iterations = 0;
    r.termination = 0;
  }
  r.tf[2] = atan2(sin(th), cos(th));  // T_best_ = Identity.rotate(theta).pretranslate(x, y), reported as atan2(T10, T00)
  out[i] = r;
}
