// K5h -- curvature of the GMM-L2 objective at the refined pose (the *_ranked_detail entry points).
//
//   cc_k_gmm_hess    the problems cc_k_select listed for refinement, after cc_k_gmm_refine: cost, gradient and the six second
//                    derivatives of  cost(p) = sum over the problem's selected pairs of term(p)  at p = tf_opt, divided by
//                    sqrt(ac_src * ac_tgt) (f = -correlation: the terms are negative): a 9-double record (cc_gmm_hess) per problem,
//                    which the detail instances of cc_k_final hand out per ranked entry.
//
// It runs only in chains that asked for detail and leaves cc_k_gmm_refine alone (256 VGPR and scratch: six more accumulators
// there are not free).  The refinement's pair records are gone by now (LDS) or about to be reused (pair pool), so the sweep
// reads what is still there: the problem's pair-code list in the chunk's code pool and the two scans' ellipse tables, the
// walk and the gather of cc_gmm_eval_first without its stores.
//
// One wave per problem, also for the short lists.  A problem costs one sweep -- no serial line-search code that four problems
// could share on a 16-lane group, which is what the 16-lane refinement instance is for -- so what a short list costs here is
// the latency of its few dependent loads (list header, codes, ellipses), the same for 16 lanes as for 64, and a chunk's few
// thousand selected problems fill the chip's wave slots either way.  The long lists (~1 000 pairs) need the 64 lanes.
#pragma once
#include "k_gmm.h"

// One term, its gradient and its Hessian (xx, xy, xt, yy, yt, tt), in the notation of cc_gmm_term.  With v the term and
// L = grad Q - 1/2 grad ln det (so that grad v = v L):  hess v = v (L L^T + hess Q - 1/2 hess ln det).
//   det depends on theta only:  det' = ddet,  det'' = 4 (2p (n00 - n11) - 8 q^2 + 2 q nx - 8 p^2)      (p' = -2q, q' = 2p)
//   Q = -E / (2 det),  E = m0^2 n11 + m1^2 n00 - m0 m1 nx,  mu' = (g0, g1),  g0' = -g1,  g1' = g0
//   E_x = 2 m0 n11 - m1 nx,  E_y = 2 m1 n00 - m0 nx,  E_xx = 2 n11,  E_yy = 2 n00,  E_xy = -nx
//   Q_xx = -n11 / det,  Q_yy = -n00 / det,  Q_xy = nx / (2 det)
//   Q_t  = -E_t / (2 det) - Q det'/det,   Q_xt = -(E_xt - E_x det'/det) / (2 det)   (y alike)
//   Q_tt = -E_tt / (2 det) - 2 Q_t det'/det - Q det''/det,   (ln det)_tt = det''/det - (det'/det)^2
struct cc_gterm2 {
  double v, gx, gy, gt, hxx, hxy, hxt, hyy, hyt, htt;
};
__device__ __forceinline__ cc_gterm2 cc_gmm_term2(const cc_gpair &P, double px, double py, double c, double s, double c2, double s2,
                                                  const double *exp_tab) {
  const double p = fma(P.sd, c2, -(P.sb * s2)), q = fma(P.sd, s2, P.sb * c2);
  const double p2 = p + p, q2 = q + q;
  const double n00 = P.a00 + p2, n11 = P.a11 - p2;
  const double nx = fma(4.0, q, P.as);
  const double nd = n00 - n11;
  const double det = fma(n00, n11, -fma(q2, q2 + P.as, P.ap));
  const double ddet = 4.0 * fma(q, nd, -(p * nx));
  const double d2det = 8.0 * fma(p, nd, fma(q, nx, -(4.0 * fma(q, q, p * p))));
  const double smx = (double)P.smx, smy = (double)P.smy;
  const double g0 = -fma(s, smx, c * smy), g1 = fma(c, smx, -(s * smy));  // d mu / d theta
  const double m0 = g1 + (px - (double)P.tmx), m1 = (py - (double)P.tmy) - g0;
  const double m00 = m0 * m0, m11 = m1 * m1, m01 = m0 * m1;
  const double E = fma(m00, n11, fma(m11, n00, -(m01 * nx)));
  const double gm = fma(g0, m1, m0 * g1);            // (m0 m1)'
  const double mg = fma(m0, g0, -(m1 * g1));         // (m00 - m11)' / 2
  const double dE = fma(2.0, fma(m0 * g0, n11, m1 * g1 * n00), fma(4.0 * q, m00 - m11, -fma(gm, nx, 8.0 * p * m01)));
  const double r = cc_rsqrt(det);
  const double idet = r * r;
  const double hi = -0.5 * idet;
  const double Q = hi * E;
  const double v = -(P.w * r) * cc_exp_nonpos(Q, exp_tab);
  const double Ex = fma(2.0 * m0, n11, -(m1 * nx)), Ey = fma(2.0 * m1, n00, -(m0 * nx));
  const double Lx = hi * Ex, Ly = hi * Ey;
  const double D1 = ddet * idet, D2 = d2det * idet;
  const double Lt = idet * fma(-0.5, dE, -(ddet * (Q + 0.5)));  // Q_t - D1 / 2, as cc_gmm_term has it
  const double Qt = fma(0.5, D1, Lt);
  const double Ext = fma(2.0 * g0, n11, fma(8.0 * q, m0, -fma(g1, nx, 8.0 * p * m1)));
  const double Eyt = fma(2.0 * g1, n00, -fma(8.0 * q, m1, fma(g0, nx, 8.0 * p * m0)));
  const double Qxt = hi * fma(-Ex, D1, Ext), Qyt = hi * fma(-Ey, D1, Eyt);
  // E_tt, term by term of E_t:
  //   (2 m0 g0 n11)' = 2 (g0^2 - m0 g1) n11 + 8 q m0 g0        (2 m1 g1 n00)' = 2 (g1^2 + m1 g0) n00 - 8 q m1 g1
  //   (4 q (m00 - m11))' = 8 p (m00 - m11) + 8 q mg            (-gm nx)' = -(2 g0 g1 + mg) nx - 8 p gm
  //   (-8 p m01)' = 16 q m01 - 8 p gm
  const double Ett = fma(2.0 * fma(g0, g0, -(m0 * g1)), n11, 2.0 * fma(g1, g1, m1 * g0) * n00) +
                     fma(8.0 * p, (m00 - m11) - (gm + gm), 8.0 * q * (mg + mg + m01 + m01)) - fma(2.0 * g0, g1, mg) * nx;
  const double Qtt = fma(hi, Ett, -fma(2.0 * Qt, D1, Q * D2));
  cc_gterm2 o;
  o.v = v;
  o.gx = v * Lx;
  o.gy = v * Ly;
  o.gt = v * Lt;
  o.hxx = v * fma(Lx, Lx, -(n11 * idet));
  o.hxy = v * fma(Lx, Ly, 0.5 * nx * idet);
  o.hxt = v * fma(Lx, Lt, Qxt);
  o.hyy = v * fma(Ly, Ly, -(n00 * idet));
  o.hyt = v * fma(Ly, Lt, Qyt);
  o.htt = v * (fma(Lt, Lt, Qtt) - 0.5 * fma(-D1, D1, D2));
  return o;
}

// The sweep over one problem's code list (the walk of cc_gmm_eval_first): block header a block ahead, codes a sub-batch ahead,
// the 2 U ellipses of a sub-batch requested together.  G lanes; the ten sums in every lane.
template <int G>
__device__ __forceinline__ void cc_gmm_hess_one(const unsigned *__restrict__ codes, int blk, const cc_gmm_feat *__restrict__ fsrc,
                                                const cc_gmm_feat *__restrict__ ftgt, int sl, const double p[3], const double *exp_tab,
                                                double (&sum)[10]) {
  double c, s;
  sincos(p[2], &s, &c);
  const double c2 = c * c - s * s, s2 = 2.0 * s * c;
  double a = 0.0, ax = 0.0, ay = 0.0, at = 0.0, hxx = 0.0, hxy = 0.0, hxt = 0.0, hyy = 0.0, hyt = 0.0, htt = 0.0;
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
          const cc_gterm2 t = cc_gmm_term2(P, p[0], p[1], c, s, c2, s2, exp_tab);
          a += t.v;
          ax += t.gx;
          ay += t.gy;
          at += t.gt;
          hxx += t.hxx;
          hxy += t.hxy;
          hxt += t.hxt;
          hyy += t.hyy;
          hyt += t.hyt;
          htt += t.htt;
        }
      }
    }
    done += n;
    blk = nxt;
    n = n2;
    nxt = nxt2;
  }
  sum[0] = cc_gsum<G>(a);
  sum[1] = cc_gsum<G>(ax);
  sum[2] = cc_gsum<G>(ay);
  sum[3] = cc_gsum<G>(at);
  sum[4] = cc_gsum<G>(hxx);
  sum[5] = cc_gsum<G>(hxy);
  sum[6] = cc_gsum<G>(hxt);
  sum[7] = cc_gsum<G>(hyy);
  sum[8] = cc_gsum<G>(hyt);
  sum[9] = cc_gsum<G>(htt);
}

// grid = any (grid-stride over the three device-side lists of cc_k_select: the long problems by length class, longest first,
// then the in-between ones, then the short ones), block = 64: one wave per problem.
__global__ void __launch_bounds__(64)
cc_k_gmm_hess(const cc_gmm_problem *__restrict__ probs, const int *__restrict__ n_small_p, const int *__restrict__ small_list,
              const int *__restrict__ n_mid_p, const int *__restrict__ mid_list, const int *__restrict__ n_big_p,
              const int *__restrict__ cls_list, const int *__restrict__ cls_cnt, int sel_stride, const cc_gmm_feat *__restrict__ qfeat,
              const cc_gmm_feat *__restrict__ db_feat, const cc_gmm_result *__restrict__ results, const unsigned *__restrict__ codes,
              cc_gmm_hess *__restrict__ out /*[problem slot]*/) {
  __shared__ double exp_tab[64];
  exp_tab[threadIdx.x] = __longlong_as_double((long long)cc_exp2_tab64[threadIdx.x]);
  cc_wave_sync();
  const int sl = threadIdx.x;
  const int n_big = *n_big_p, n_mid = *n_mid_p, n_small = *n_small_p;
  const int n_all = n_big + n_mid + n_small;
  for (int k = blockIdx.x; k < n_all; k += gridDim.x) {
    int pidx;
    if (k >= n_big + n_mid) {
      pidx = small_list[k - n_big - n_mid];
    } else if (k >= n_big) {
      pidx = mid_list[k - n_big];
    } else {  // the k-th problem in class order, as cc_k_gmm_refine<64> finds it
      int c = 0, kk = k;
#pragma unroll
      for (int j = 0; j < CC_GMM_NCLS - 1; j++) {
        const int cj = cls_cnt[j];
        if (c == j && kk >= cj) {
          kk -= cj;
          c = j + 1;
        }
      }
      pidx = cls_list[(size_t)c * sel_stride + kk];
    }
    pidx = cc_uniform_i(pidx);
    const cc_gmm_result *R = &results[pidx];
    const cc_gmm_problem *pb = &probs[pidx];
    const cc_gmm_feat *fsrc = db_feat + pb->gidx;
    const cc_gmm_feat *ftgt = qfeat + pb->q;
    const double x[3] = {R->tf_opt[0], R->tf_opt[1], R->tf_opt[2]};
    double sum[10];
    cc_gmm_hess_one<64>(codes, cc_uniform_i(R->code_seg), fsrc, ftgt, sl, x, exp_tab, sum);
    if (sl < 9) {  // lanes 0..8 write one double each: (grad | hess) of f = -correlation = cost / sqrt(ac_src ac_tgt)
      const double inv = 1.0 / sqrt(fsrc->ac * ftgt->ac);
      double v = sum[1];
#pragma unroll
      for (int j = 2; j < 10; j++) v = sl == j - 1 ? sum[j] : v;
      ((double *)&out[pidx])[sl] = v * inv;
    }
  }
}
