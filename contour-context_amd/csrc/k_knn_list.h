// K3, list form -- the k-nearest-key search of a query that names a LIST of database scans (include/cont2_amd_lists.h): the
// keys of the listed scans are enumerated by key id, nothing else of the layer is touched.
#pragma once
#include "cc_group.h"
#include "k_knn.h"

// ------------------------------------------------------------------------------------------------
// A layer keeps its keys in insertion order beside the sorted view (keys SoA [CC_KEY_DIM][cap_k], kgidx, kseq and the
// activation epochs, all by key id), and cc_db_add_scans appends a scan's non-zero keys in ascending anchor order: the key
// ids of scan g in layer l are [nkeys_hist[g][l], nkeys_hist[g + 1][l]).  The host stages that range per listed scan
// (cc_list_ent), so the search of a query whose list has n scans reads at most n * CC_NPIV keys, whatever the layer holds.
//
// The walk's result does not depend on the visiting order (k_knn.h: "only the survivors' order (distance, then key id)
// matters"): it is the nnk smallest by (distance bits, key id) among the keys that pass the walk's tests.  Here the same
// tests run per enumerated key, the candidates go through the same LDS buffer and the same reductions, so the hit table is
// the masked walk's to the bit.
//
// One wave per (query, layer, anchor), the walk's grid.  64 staged scans per step, one per lane; the lanes then take their
// scan's keys of the layer in turns (<= CC_NPIV turns; the loop ends when no lane has a key left, a wave-uniform test).  A
// lane's loads of one turn depend on its staged entry alone, not on the turn before: the turns of a step are independent, and
// the next step's entries are requested before the current step's keys are scored.  (The flattened (scan, anchor) mapping
// would keep every lane busy on sparse layers, but needs a prefix sum over the step's key counts and a search per lane for
// its scan before the first key load can be issued -- one more dependent round trip per step, for lanes that idle at most
// five turns here.)
// ------------------------------------------------------------------------------------------------

// one listed scan, staged by the host: g = the scan, w[ll] = first key id << 3 | number of keys of query layer ll
struct cc_list_ent {
  int g;
  int w[CC_NQLEV];
};
static_assert(sizeof(cc_list_ent) == 16 && CC_NQLEV == 3 && CC_NPIV <= 7, "cc_list_ent: 16 bytes, the key count in 3 bits");
// per query of the chunk: x = its first staged entry (-1: the query names no list), y = the number of entries
typedef int2 cc_list_row;

struct cc_knn_list_params {
  const float *keys[CC_NQLEV];  // insertion order, SoA [CC_KEY_DIM][cap_k]
  const int *act[CC_NQLEV];     // by key id: first epoch at which the key sits in a tree
};

// Pending entries of the LDS buffer: a reduction leaves nnk, the next one runs as soon as 2 nnk are pending (nnk the first
// time), and it is tested after EVERY key turn, which files at most 64 (one per lane): at most 2 nnk - 1 + 64.
static_assert(2 * CC_KNN_MAX - 1 + 64 <= CC_KNN_CAP, "cc_k_knn_list: pending candidates must fit the LDS buffer");
static_assert(2 * CC_KNN_MAX_LARGE - 1 + 64 <= CC_KNN_CAP_LARGE, "cc_k_knn_list_l: pending candidates must fit the LDS buffer");

// grid = nq * CC_NQLEV * CC_NPIV, block = 64, hits / hit_cnt as cc_knn_walk's.  A search whose query names no list returns
// at once and leaves its outputs alone (a mixed chunk: the unrestricted retrieval has written them, in stream order).
template <bool VIS, int KM>
__device__ __forceinline__ void cc_knn_list(cc_knn_params P, cc_knn_list_params LP, const cc_hot_desc_t *qhot, const cc_query_meta *qmeta,
                                            cc_knn_hit_t *hits, int *hit_cnt, const cc_list_row *qlist, const cc_list_ent *ent) {
  static_assert(KM == CC_KNN_MAX || KM == CC_KNN_MAX_LARGE, "cc_knn_list: the two instances");
  __shared__ unsigned long long buf[KM == CC_KNN_MAX ? CC_KNN_CAP : CC_KNN_CAP_LARGE];
  const int lane = threadIdx.x;
  const int slot = blockIdx.x % (CC_NQLEV * CC_NPIV);
  const int q = blockIdx.x / (CC_NQLEV * CC_NPIV);
  const int ll = slot / CC_NPIV, seq = slot - ll * CC_NPIV;
  const cc_list_row row = qlist[q];
  const int e_first = cc_uniform_i(row.x), n_ent = cc_uniform_i(row.y);
  if (e_first < 0) return;
  cc_knn_hit_t *out = hits + (size_t)blockIdx.x * KM;
  if (ll >= P.n_q_levels) {
    if (lane == 0) hit_cnt[blockIdx.x] = 0;
    return;
  }
  const int level = P.q_levels[ll];
  const float *qk = &qhot[q].keys[level - 1][seq][0];
  float k[CC_KEY_DIM];
  float sum = 0.f;
#pragma unroll
  for (int d = 0; d < CC_KEY_DIM; d++) {
    k[d] = qk[d];
    sum += k[d];
  }
  if (!(sum != 0.f) || P.n_sorted[ll] <= 0) {  // cc_knn_walk's early exit
    if (lane == 0) hit_cnt[blockIdx.x] = 0;
    return;
  }
  const cc_query_meta *qm = qmeta + q;
  // dist_ub: cc_knn_walk's lines (k_knn.h, "dist_ub (contour_db.h:733-749)"), repeated here so that the walk's code stays as it is
  const float b00 = (float)((double)k[0] * 0.8), b01 = (float)((double)k[0] / 0.8);
  const float b10 = (float)((double)k[1] * 0.8), b11 = (float)((double)k[1] / 0.8);
  const float b20 = (float)((double)k[2] * 0.8 * 0.75), b21 = (float)((double)k[2] / (0.8 * 0.75));
  const float t0a = (k[0] - b00) * (k[0] - b00), t0b = (k[0] - b01) * (k[0] - b01);
  const float t1a = (k[1] - b10) * (k[1] - b10), t1b = (k[1] - b11) * (k[1] - b11);
  const float t2a = (k[2] - b20) * (k[2] - b20), t2b = (k[2] - b21) * (k[2] - b21);
  float ub = (t0a < t0b ? t0b : t0a) + (t1a < t1b ? t1b : t1a) + (t2a < t2b ? t2b : t2a);
  // (selected, not indexed: indexed by the runtime layer the six pointers are copied to a private array first, which the
  // compiler then places in LDS or in scratch)
  const float *K = ll == 0 ? LP.keys[0] : ll == 1 ? LP.keys[1] : LP.keys[2];
  const int *act = ll == 0 ? LP.act[0] : ll == 1 ? LP.act[1] : LP.act[2];
  const unsigned cap = (unsigned)P.cap_k;
  const int epoch = qm->epoch;
  const int nnk = P.nnk;
  const bool idx_full = VIS ? qm->idx_full[ll] != 0 : true;  // wave-uniform

  // ---- the visible buckets as a predicate on key[0].  The walk visits the sorted index ranges [L0, E1) u [S2, E2) with
  // L0 = lb(rg[0]), E1 = lb(rg[mid + 1]), S2 = lb(rg[2 mid + 1]) (rg[6] when 2 mid + 1 > 6), E2 = lb(rg[6]) and
  // lb(t) = the number of keys with key[0] < t.  In a layer sorted by key[0], index i >= lb(a) iff key[0] of i >= a, and
  // i < lb(b) iff key[0] of i < b (no key is NaN: pushBuffer drops them), so a key is in the ranges iff
  // rg[0] <= key[0] < rg[mid + 1] or rg[2 mid + 1] <= key[0] < rg[6].  mid: the walk's search, 0 when no bucket holds k[0].
  float v_l0, v_e1, v_s2, v_e2;
  {
    float rg[7];
#pragma unroll
    for (int i = 0; i < 7; i++) rg[i] = qm->ranges[ll][i];
    int mid = 0;
    {
      bool found = false;
#pragma unroll
      for (int i = 0; i < 6; i++)
        if (!found && rg[i] <= k[0] && rg[i + 1] > k[0]) {
          mid = i;
          found = true;
        }
    }
    v_l0 = rg[0];
    v_e1 = rg[6];
    v_s2 = rg[6];
    v_e2 = rg[6];
#pragma unroll
    for (int i = 1; i < 7; i++) {
      if (i == mid + 1) v_e1 = rg[i];
      if (i == 2 * mid + 1) v_s2 = rg[i];
    }
  }

  int cnt = 0;
  bool tightened = false;
  int w_next = 0;  // this lane's entry of the next step (first key id << 3 | keys of the layer); 0: none
  if (lane < n_ent) w_next = ent[e_first + lane].w[ll];
  for (int s0 = 0; s0 < n_ent; s0 += 64) {
    const int w = w_next;
    w_next = 0;
    if (s0 + 64 + lane < n_ent) w_next = ent[e_first + s0 + 64 + lane].w[ll];
    const int id0 = (int)((unsigned)w >> 3), nk = w & 7;
    for (int t = 0; t < CC_NPIV; t++) {
      const bool on = t < nk;
      if (__ballot(on) == 0ull) break;  // no lane has a key left in this step
      const unsigned id = on ? (unsigned)(id0 + t) : 0u;
      const int a = act[id];
      float c[CC_KEY_DIM];
#pragma unroll
      for (int d = 0; d < CC_KEY_DIM; d++) c[d] = K[(size_t)d * cap + id];
      // L2_Adaptor::evalMetric accumulation order (nanoflann.hpp:427-461), as in cc_knn_walk
      float r = 0.f;
      float d0 = k[0] - c[0], d1 = k[1] - c[1], d2 = k[2] - c[2], d3 = k[3] - c[3];
      r += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      d0 = k[4] - c[4];
      d1 = k[5] - c[5];
      d2 = k[6] - c[6];
      d3 = k[7] - c[7];
      r += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      d0 = k[8] - c[8];
      r += d0 * d0;
      d0 = k[9] - c[9];
      r += d0 * d0;
      const bool visible = (v_l0 <= c[0] && c[0] < v_e1) || (v_s2 <= c[0] && c[0] < v_e2);
      // the walk's rule for the radius: strictly inside dist_ub before nnk candidates are known, afterwards keys AT the
      // nnk-th best distance still compete, on the key id
      bool pass = on && visible && a <= epoch && (tightened ? (r <= ub) : (r < ub));
      if (VIS && !idx_full && pass) pass = cc_knn_key_indexed(qm, ll, c[0]);
      const unsigned long long m = __ballot(pass);
      if (pass) buf[cnt + cc_mbcnt(m)] = ((unsigned long long)__float_as_uint(r) << 32) | id;
      cnt += __popcll(m);
      if (cnt >= 2 * nnk || (!tightened && cnt >= nnk)) {  // keep the best nnk (by distance, then key id); the radius follows
        if constexpr (KM == CC_KNN_MAX) {
          unsigned long long first;
          ub = cnt <= 128 ? cc_knn_reduce<2>(buf, cnt, nnk, lane, first) : cc_knn_reduce<4>(buf, cnt, nnk, lane, first);
        } else {
          cc_knn_by_width(cnt, [&](auto r_) {
            unsigned long long v[decltype(r_)::value];
            ub = cc_knn_reduce_l(buf, cnt, nnk, lane, v);
          });
        }
        cnt = nnk;
        tightened = true;
        cc_wave_sync();
      }
    }
  }
  // the hits, written as cc_knn_walk writes them
  const int mm = cnt < nnk ? cnt : nnk;
  if constexpr (KM != CC_KNN_MAX) {
    cc_knn_by_width(cnt, [&](auto r_) {
      constexpr int R = decltype(r_)::value;
      unsigned long long v[R];
      cc_knn_reduce_l(buf, cnt, nnk, lane, v);
#pragma unroll
      for (int a = 0; a < (R < KM / 64 ? R : KM / 64); a++) {
        if (a * 64 + lane < mm) {
          const unsigned id = (unsigned)(v[a] & 0xFFFFFFFFu);
          cc_knn_hit_t h;
          h.gidx = P.kgidx[ll][id];
          h.level = (int16_t)level;
          h.seq = (int16_t)P.kseq[ll][id];
          h.dist_sq = __uint_as_float((unsigned)(v[a] >> 32));
          out[a * 64 + lane] = h;
        }
      }
    });
  } else {
    unsigned long long first;
    if (cnt <= 128)
      cc_knn_reduce<2>(buf, cnt, nnk, lane, first);
    else
      cc_knn_reduce<4>(buf, cnt, nnk, lane, first);
    if (lane < mm) {
      const unsigned id = (unsigned)(first & 0xFFFFFFFFu);
      cc_knn_hit_t h;
      h.gidx = P.kgidx[ll][id];
      h.level = (int16_t)level;
      h.seq = (int16_t)P.kseq[ll][id];
      h.dist_sq = __uint_as_float((unsigned)(first >> 32));
      out[lane] = h;
    }
  }
  if (lane == 0) hit_cnt[blockIdx.x] = mm;
}

template <bool VIS>
__global__ void __launch_bounds__(64)
cc_k_knn_list(cc_knn_params P, cc_knn_list_params LP, const cc_hot_desc_t *__restrict__ qhot, const cc_query_meta *__restrict__ qmeta,
              cc_knn_hit_t *hits, int *hit_cnt, const cc_list_row *__restrict__ qlist, const cc_list_ent *__restrict__ ent) {
  cc_knn_list<VIS, CC_KNN_MAX>(P, LP, qhot, qmeta, hits, hit_cnt, qlist, ent);
}

// the large-k instance (64 < nnk <= CC_KNN_MAX_LARGE): hits [.][CC_KNN_MAX_LARGE]
template <bool VIS>
__global__ void __launch_bounds__(64)
cc_k_knn_list_l(cc_knn_params P, cc_knn_list_params LP, const cc_hot_desc_t *__restrict__ qhot, const cc_query_meta *__restrict__ qmeta,
                cc_knn_hit_t *hits, int *hit_cnt, const cc_list_row *__restrict__ qlist, const cc_list_ent *__restrict__ ent) {
  cc_knn_list<VIS, CC_KNN_MAX_LARGE>(P, LP, qhot, qmeta, hits, hit_cnt, qlist, ent);
}
