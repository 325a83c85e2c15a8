// Candidate verification (cc_db_verify_*): the check table of a chunk written on the device from (query, candidate list)
// items instead of by the KNN search.  For every item the kernel below walks the reference demo's hint loop
// (test/kitti_read_bin_test.cpp:226-291, the candidate as the outermost index):
//   for candidate k in list order, for level 1..4 where set in the mask, for seq_src 0..5 (the candidate's anchor), for
//   seq_tgt 0..5 (the query's anchor): a check, unless either retrieval key sums to zero (contour_db.h:726: the anchor does
//   not exist) or the keys' squared distance exceeds the caller's bound
// and writes the surviving tuples densely, in that order, into the item's rows of the lane's hit table -- the layout
// cc_db_check_hints fills on the host (the query's anchor rides in the high byte of `level`), which the scoring chain
// (k_check.h ...) takes from there.
//
// Arithmetic: the f32 key sum and the f32 squared distance are accumulated in index order, every product and sum rounded once
// (the library is built with -ffp-contract=off), like the exact distances of the search.
//
// Bound: an item reads its query's 960 B of keys and 960 B per candidate (<= 9 x 960 B = 8.6 KB, as 16-byte loads of 60
// lanes each, all issued before the first is waited for) and writes <= 1 152 hits of 12 B; 18 steps of 64 tuples, each ~60
// LDS reads and a ballot.  With one wave per item and 1 024 items the launch is a few microseconds of latency, not of work.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cont2_amd.h"
#include "cc_group.h"
#include "k_check.h"

#define CC_VERIFY_KEYS (CC_HOT_LEVELS * CC_NPIV * CC_KEY_DIM)                // 240 floats of keys per hot record
#define CC_VERIFY_TUPLES (CC_HOT_LEVELS * CC_NPIV * CC_NPIV)                 // 144 (level, seq_src, seq_tgt) per candidate
static_assert(CC_VERIFY_CANDS_MAX * CC_VERIFY_TUPLES == CC_HINT_MAX, "every tuple of a full candidate list has a check slot");
static_assert(CC_VERIFY_KEYS % 4 == 0 && CC_VERIFY_KEYS / 4 <= 64, "one 16-byte load per lane brings a record's keys");
static_assert(offsetof(cc_hot_desc_t, keys) % 16 == 0 && sizeof(cc_hot_desc_t) % 16 == 0, "16-byte loads of the keys");
static_assert(CC_HINT_MAX == CC_CHK_STRIDE && CC_NQLEV * CC_NPIV <= 64, "one item's rows of the hit table; its counts by one wave");

struct cc_verify_params {
  int level_mask;         // bit (level - 1), 1..15
  float max_key_dist_sq;  // +inf: no bound
};

// grid = items of the chunk, block = 64 (one wave per item)
__global__ void __launch_bounds__(64)
cc_k_hints_expand(cc_verify_params P, const cc_hot_desc_t *__restrict__ qhot /*[n] the chunk's query records, item order*/,
                  const cc_hot_desc_t *__restrict__ db_hot, const int *__restrict__ cands /*[n][CC_VERIFY_CANDS_MAX], -1 ends a list*/,
                  int n, cc_knn_hit_t *__restrict__ hits /*[n][CC_CHK_STRIDE]*/, int *__restrict__ hit_cnt /*[n][CC_NQLEV * CC_NPIV]*/,
                  cc_hint_t *__restrict__ hints_out /*[n][CC_HINT_MAX] or nullptr*/, int *__restrict__ n_hints_out /*[n] or nullptr*/) {
  __shared__ __attribute__((aligned(16))) float s_q[CC_VERIFY_KEYS];
  __shared__ __attribute__((aligned(16))) float s_c[CC_VERIFY_CANDS_MAX][CC_VERIFY_KEYS];
  __shared__ int s_cand[CC_VERIFY_CANDS_MAX];
  const int item = blockIdx.x, lane = threadIdx.x;
  if (item >= n) return;
  if (lane < CC_VERIFY_CANDS_MAX) s_cand[lane] = cands[(size_t)item * CC_VERIFY_CANDS_MAX + lane];
  cc_wave_sync();
  int m = 0;  // candidates of the item (the list ends at the first -1: validated on the host)
  while (m < CC_VERIFY_CANDS_MAX && s_cand[m] >= 0) m++;
  m = cc_uniform_i(m);
  // the keys: the query's and every candidate's, one float4 per lane and record, all loads in flight together
  constexpr int NV = CC_VERIFY_KEYS / 4;
  if (lane < NV) {
    // straight-line code: a slot beyond the list loads the list's first candidate once more (a cache hit nobody reads), so that
    // the eight loads stay in registers and in flight together whatever the list's length
    ((float4 *)s_q)[lane] = ((const float4 *)&qhot[item].keys[0][0][0])[lane];
    if (m > 0) {
      float4 v[CC_VERIFY_CANDS_MAX];
#pragma unroll
      for (int k = 0; k < CC_VERIFY_CANDS_MAX; k++) v[k] = ((const float4 *)&db_hot[s_cand[k < m ? k : 0]].keys[0][0][0])[lane];
#pragma unroll
      for (int k = 0; k < CC_VERIFY_CANDS_MAX; k++) ((float4 *)s_c[k])[lane] = v[k];
    }
  }
  cc_wave_sync();
  cc_knn_hit_t *out = hits + (size_t)item * CC_CHK_STRIDE;
  cc_hint_t *hout = hints_out ? hints_out + (size_t)item * CC_HINT_MAX : nullptr;
  const int n_tup = m * CC_VERIFY_TUPLES;
  int base = 0;
  for (int t0 = 0; t0 < n_tup; t0 += 64) {
    const int t = t0 + lane;
    const bool valid = t < n_tup;
    const int tc = valid ? t : 0;
    const int k = tc / CC_VERIFY_TUPLES, r = tc - k * CC_VERIFY_TUPLES;
    const int li = r / (CC_NPIV * CC_NPIV), r2 = r - li * (CC_NPIV * CC_NPIV);
    const int a = r2 / CC_NPIV, b = r2 - a * CC_NPIV;  // seq_src (candidate), seq_tgt (query)
    const float *kc = &s_c[k][(li * CC_NPIV + a) * CC_KEY_DIM];
    const float *kq = &s_q[(li * CC_NPIV + b) * CC_KEY_DIM];
    float sum_c = 0.f, sum_q = 0.f, d2 = 0.f;
#pragma unroll
    for (int i = 0; i < CC_KEY_DIM; i++) {
      const float x = kc[i], y = kq[i], df = x - y;
      sum_c += x;
      sum_q += y;
      d2 += df * df;
    }
    const bool emit = valid && ((P.level_mask >> li) & 1) && (sum_c != 0.f) && (sum_q != 0.f) && !(d2 > P.max_key_dist_sq);
    const unsigned long long mk = __ballot(emit);
    if (emit) {
      const int pos = base + cc_mbcnt(mk);
      cc_knn_hit_t h;
      h.gidx = s_cand[k];
      h.level = CC_HIT_PACK_LEVEL(li + 1, b);
      h.seq = (int16_t)a;
      h.dist_sq = 0.f;
      out[pos] = h;
      if (hout) {
        cc_hint_t g;
        g.cand_gidx = h.gidx;
        g.level = (int8_t)(li + 1);
        g.seq_src = (int8_t)a;
        g.seq_tgt = (int8_t)b;
        g.pad = 0;
        hout[pos] = g;
      }
    }
    base += __popcll(mk);
  }
  if (lane < CC_NQLEV * CC_NPIV) {
    const int left = base - lane * CC_KNN_MAX;
    hit_cnt[item * (CC_NQLEV * CC_NPIV) + lane] = left < 0 ? 0 : (left > CC_KNN_MAX ? CC_KNN_MAX : left);
  }
  if (n_hints_out && lane == 0) n_hints_out[item] = base;
}
