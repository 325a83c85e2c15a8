// K1 -- BEV rasterisation.  Replaces ContourManager::makeBEV (contour_mng.h:505-556) for a batch
// of scans: one workgroup per scan, the 150x150 max-height grid lives in LDS.
//
//   sweep : stream the scan's points ONCE (KITTI (x,y,z,i) records, or the caller's own records through a point loader, below;
//           an optional per-scan 3 x 4 transform is applied as they arrive), a register-held chunk at a time:
//           LDS atomicMax of the order-preserving height key per cell               (90 KB LDS), then, among the
//           chunk's points whose height equals the cell maximum, keep the smallest point index -- the reference
//           updates a cell only on `bev < height` (strict), so the FIRST point in file order wins ties
//           (contour_mng.h:517).  Indices are 21-bit fields, three per 64-bit LDS word, erased with an atomicOr when
//           the cell's maximum rises and min-updated with a CAS loop                 (60 KB LDS)
//   out   : dense bev image + continuous (row_f,col_f) of the winning point per occupied cell
//           (pointToContRowCol, contour_mng.h:468-472), max/min accepted height, #occupied cells.
//
// Roofline: HBM.  Algorithmic bytes = 16 B x points = what the sweep reads of KITTI records.  Other layouts:
// DESIGN.md 3.0 has the measured rows (the byte ratio of a layout is not its speed).
#pragma once
#include "cc_dev.h"
#include "cc_group.h"

#define CC_K1_IDX_BITS 21
#define CC_K1_IDX_MASK 0x1FFFFFull
#ifndef CC_K1_U_DEFAULT
#define CC_K1_U_DEFAULT 4  // points per lane and chunk (8 measured equal: the sweep is bound by instruction issue, not by loads in flight)
#endif

// The first-index fields: CC_K1_IDX_BITS bits per cell, three cells per 64-bit LDS word; word w holds the cells w, w + n_w3,
// w + 2 n_w3 (round 6: w held 3 w .. 3 w + 2 -- neighbouring cells are what neighbouring lanes bring, and their CAS
// attempts on one word failed each other).
__device__ __forceinline__ void cc_k1_field(int cell, int n_w3, int &w, int &sh) {
  const int f = (cell >= n_w3 ? 1 : 0) + (cell >= 2 * n_w3 ? 1 : 0);
  w = cell - f * n_w3;
  sh = f * CC_K1_IDX_BITS;
}

struct cc_k1_scan_out {
  float max_bin_val, min_bin_val;
  int n_pix;
  int pad;
};

__device__ __forceinline__ float cc_wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) {
    float t = __shfl_xor(v, o);
    v = v < t ? t : v;
  }
  return v;
}
__device__ __forceinline__ float cc_wave_min(float v) {
  for (int o = 32; o > 0; o >>= 1) {
    float t = __shfl_xor(v, o);
    v = v > t ? t : v;
  }
  return v;
}
__device__ __forceinline__ int cc_wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Partial results of one point range of a scan (CC_K1_SPLIT ranges per scan when a call brings only a few scans: the
// per-scan loop of the class mirror brings one, and one workgroup sweeping 120 000 points alone lasts ~100 us):
// per cell the height key and the scan-relative index of the first point that reaches it, plus the range's max / min keys.
#define CC_K1_SPLIT 8
#define CC_K1_SPLIT_MAX_SCANS 8   // calls with up to this many scans take the split path
struct cc_k1_part {
  unsigned *key;   // [n_scans * CC_K1_SPLIT][n_cell]
  int *idx;        // same
  unsigned *red;   // [n_scans * CC_K1_SPLIT][2]: max key, min key
};

// The scan's ACTIVE cells (above the lowest level) as a raster-ordered list -- what K2's list kernel (k_contours_list.h) starts
// from: K1 has every cell's height in LDS when it writes the dense image, so it lists the active ones on the way out
// instead of K2 re-reading 90 KB of image to find the ~2 500 cells it wants (round 6).  Per scan: header (entries, (cell,
// level) slots), and for the first CC_LIST_CAP entries (row << 8 | col), level count, height, continuous position.
#define CC_LIST_CAP 3072
#define CC_K1_NCHUNK ((CC_MAX_CELLS + 63) / 64)
struct cc_k1_list_out {
  int4 *hdr;            // [n_scans]: x = entries (all of them, also beyond the capacity), y = slots = sum of the level counts, z = the dense image / positions were written
  uint16_t *rc;         // [n_scans][CC_LIST_CAP]
  unsigned char *lev;   // same
  float *h;             // same
  float2 *pix;          // same
};
#define CC_K1_EB 8  // cells per thread whose records cc_k1_emit has in flight together
#define CC_K1_LB 4  // list entries per thread whose records it has in flight together
#define CC_K1_EMIT_TAB_BYTES (CC_K1_NCHUNK * 2 * 3 + 16)  // u16 entries per chunk | u16 entries before the chunk | u16 slots per chunk | totals
#define CC_K1_EMIT_LDS_BYTES (CC_K1_EMIT_TAB_BYTES + CC_LIST_CAP * 2)  // ... | u16 cell of every list entry

// ---- point loaders: where a scan's points lie and how they become (x, y, z) ----
// The kernels read points in three places -- the sweep's prefetched chunk and the two owner re-reads of the output pass -- and all
// three go through one of these.  load(j) only ISSUES the read of point j (the sweep keeps the next chunk's records in flight
// while it resolves this one in LDS); xyz() turns a record that has arrived into the coordinates everything downstream sees, and
// owner_xy(j) is both for the owner of a cell: the same loads and the same operations, so the output pass gets the bits the sweep saw.
//   cc_ld_kitti       : float4 (x, y, z, intensity) records, 16-byte aligned, no transform -- what cc_ingest_batch takes
//   cc_ld_rec<STRIDE> : three consecutive f32 at the start of records STRIDE bytes apart (0: the stride is a run-time value), base
//                       and stride multiples of 4: one 12-byte load per point.  An optional per-scan rigid transform (row-major
//                       3 x 4, workgroup-uniform, held in scalar registers) is applied as x' = ((m00 x + m01 y) + m02 z) + m03,
//                       every product and sum rounded once (the library is built with -ffp-contract=off).
struct cc_xyz {
  float x, y, z;
};
struct cc_ld_kitti {
  typedef float4 rec;
  const float4 *__restrict__ P;
  __device__ __forceinline__ void advance(long long n) { P += n; }
  __device__ __forceinline__ rec load(int j) const { return P[j]; }
  __device__ __forceinline__ static rec zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void xyz(const rec &q, float &x, float &y, float &z) const {
    x = q.x;
    y = q.y;
    z = q.z;
  }
  __device__ __forceinline__ float2 owner_xy(int j) const { return *(const float2 *)(P + j); }
};
template <int STRIDE>
struct cc_ld_rec {
  typedef cc_xyz rec;
  const char *__restrict__ B;  // x of the first point
  unsigned stride;             // bytes; a scan has fewer than 2^21 points and a record at most CC_POINT_STRIDE_MAX = 2^8 bytes: j * stride < 2^29
  bool has_tf;                 // a RUN-TIME, workgroup-uniform switch (not a template one): every instance carries the branch and m[]
  float m[12];
  // tf: [n_scans][12] or nullptr.  The twelve values are the same for the whole workgroup: handed to the compiler as scalars.
  __device__ __forceinline__ cc_ld_rec(const char *base, int stride_bytes, const float *__restrict__ tf, int scan)
      : B(base), stride(STRIDE ? (unsigned)STRIDE : (unsigned)stride_bytes), has_tf(tf != nullptr) {
#pragma unroll
    for (int i = 0; i < 12; i++) m[i] = has_tf ? __int_as_float(cc_uniform_i(__float_as_int(tf[(size_t)scan * 12 + i]))) : 0.f;
  }
  __device__ __forceinline__ void advance(long long n) { B += n * (long long)stride; }
  __device__ __forceinline__ rec load(int j) const {
    cc_xyz q;
    cc_load3f(B + (unsigned)j * stride, q.x, q.y, q.z);
    return q;
  }
  __device__ __forceinline__ static rec zero() { return cc_xyz{0.f, 0.f, 0.f}; }
  __device__ __forceinline__ void xyz(const rec &q, float &x, float &y, float &z) const {
    x = q.x;
    y = q.y;
    z = q.z;
    if (has_tf) {  // workgroup-uniform
      const float tx = ((m[0] * q.x + m[1] * q.y) + m[2] * q.z) + m[3];
      const float ty = ((m[4] * q.x + m[5] * q.y) + m[6] * q.z) + m[7];
      const float tz = ((m[8] * q.x + m[9] * q.y) + m[10] * q.z) + m[11];
      x = tx;
      y = ty;
      z = tz;
    }
  }
  __device__ __forceinline__ float2 owner_xy(int j) const {
    float x, y, z;
    xyz(load(j), x, y, z);
    return make_float2(x, y);
  }
};

// The output pass shared by the one-sweep kernel and the merge kernel.  keyfn(c) / idxfn(c): the cell's height key and the
// scan-relative index of the point that owns it (asked for occupied cells only).  Two sweeps over the cells, a wave
// on 64 consecutive cells at a time: (1) active cells per chunk (one ballot), prefix by wave 0; (2) the
// dense image, the continuous position of every occupied cell, and the list entries at their raster-order positions.
// Returns this thread's count of occupied cells.  tab: CC_K1_EMIT_LDS_BYTES of LDS.
template <typename KeyFn, typename IdxFn, typename LD>
__device__ __forceinline__ int cc_k1_emit(const cc_dev_cfg &cfg, KeyFn keyfn, IdxFn idxfn, const LD &P, float *__restrict__ bev,
                                          float2 *__restrict__ pix, const cc_k1_list_out &L, int scan, char *tab, int n_pts, int want_dense, unsigned *kmax_out /*LDS: the largest cell key is max-ed into it (nullptr: not wanted)*/) {
  const int n_cell = cfg.n_cell, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  uint16_t *ccnt = (uint16_t *)tab, *cbase = ccnt + CC_K1_NCHUNK;
  int *tot = (int *)(tab + CC_K1_NCHUNK * 6);
  const int n_chunk = (n_cell + 63) >> 6;
  // (1) active cells per 64-cell chunk: one compare and one ballot per cell (a wave is on 64 consecutive cells)
  unsigned kmx = KEY_EMPTY;
  for (int c0 = 0; c0 < n_cell; c0 += nt) {  // block-uniform trip count: the ballots see whole waves
    const int c = c0 + tid;
    const unsigned k = c < n_cell ? keyfn(c) : KEY_EMPTY;
    kmx = k > kmx ? k : kmx;
    const float h = cc_funkey(k);
    const unsigned long long m0 = __ballot(h > cfg.lv_grads[0]);
    if (lane == 0 && c < n_cell) ccnt[c >> 6] = (uint16_t)__popcll(m0);
  }
  if (kmax_out) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned a = (unsigned)__shfl_xor((int)kmx, o);
      kmx = a > kmx ? a : kmx;
    }
    if (lane == 0) atomicMax(kmax_out, kmx);
  }
  if (tid == 0) tot[1] = 0;
  __syncthreads();
  if (tid < 64) {  // prefix over the chunks, one wave
    int n_act = 0;
    for (int q = 0; q < n_chunk; q += 64) {
      const int b = q + lane;
      const int v1 = b < n_chunk ? (int)ccnt[b] : 0;
      const int i1 = cc_wave_scan_incl(v1);
      if (b < n_chunk) cbase[b] = (uint16_t)(n_act + i1 - v1);
      n_act += cc_wave_scan_total(i1);
    }
    if (lane == 0) tot[0] = n_act;
  }
  __syncthreads();
  // The dense image and the dense position array are written when somebody reads them: the caller asked for them
  // (want_dense: debug outputs, cc_scan_bev, a configuration K2's list kernel does not take) or the list cannot hold the
  // scan's active cells.  Otherwise the list is all K2 needs -- 270 KB per scan that nobody read were a quarter of this
  // kernel's time (round 6) -- and cc_k_contours_mid rebuilds the two arrays from the list for a scan the list kernel hands
  // on (hdr.z says which it is).
  const bool dense = want_dense != 0 || tot[0] > CC_LIST_CAP;
  uint16_t *l_rc = L.rc + (size_t)scan * CC_LIST_CAP;
  unsigned char *l_lev = L.lev + (size_t)scan * CC_LIST_CAP;
  float *l_h = L.h + (size_t)scan * CC_LIST_CAP;
  float2 *l_pix = L.pix + (size_t)scan * CC_LIST_CAP;
  int npix = 0, nslot = 0;
  if (!dense) {
    // (2') the usual case -- only the list is wanted: the active cells' indices go to LDS in raster order (one more sweep over
    // the keys), then every thread takes list entries i, i + nt, ...: all lanes busy, the owners' records requested together,
    // the entries stored side by side (round 6: the dense sweep below kept 22 cells per thread for ~2.4 of them)
    uint16_t *acell = (uint16_t *)(tab + CC_K1_EMIT_TAB_BYTES);  // [CC_LIST_CAP]
    for (int c0 = 0; c0 < n_cell; c0 += nt) {  // block-uniform trip count
      const int c = c0 + tid;
      const unsigned k = c < n_cell ? keyfn(c) : KEY_EMPTY;
      const bool act = cc_funkey(k) > cfg.lv_grads[0];  // cv::threshold BINARY is strict `>` (contour_mng.cpp:283)
      const unsigned long long m0 = __ballot(act);
      npix += k != KEY_EMPTY ? 1 : 0;
      if (act) acell[(int)cbase[c >> 6] + cc_mbcnt(m0)] = (uint16_t)c;  // < CC_LIST_CAP: the list holds the scan
    }
    __syncthreads();
    const int n_act = tot[0];
    for (int i0 = 0; i0 < n_act; i0 += nt * CC_K1_LB) {
      int cc[CC_K1_LB];
      unsigned key[CC_K1_LB];
      float2 xy[CC_K1_LB];
#pragma unroll
      for (int e = 0; e < CC_K1_LB; e++) {
        const int i = i0 + e * nt + tid;
        cc[e] = i < n_act ? (int)acell[i] : -1;
        key[e] = cc[e] >= 0 ? keyfn(cc[e]) : KEY_EMPTY;
      }
#pragma unroll
      for (int e = 0; e < CC_K1_LB; e++) xy[e] = P.owner_xy(cc[e] >= 0 ? idxfn(cc[e]) : 0);  // (an active cell has an owner: n_pts > 0)
#pragma unroll
      for (int e = 0; e < CC_K1_LB; e++) {
        const int i = i0 + e * nt + tid, c = cc[e];
        if (c >= 0) {
          const float h = cc_funkey(key[e]);
          float2 rcf;  // pointToContRowCol, as below
          rcf.x = (cfg.reso_pow2 ? xy[e].x * cfg.inv_row : xy[e].x / cfg.reso_row) + (float)cfg.half_row - 0.5f;
          rcf.y = (cfg.reso_pow2 ? xy[e].y * cfg.inv_col : xy[e].y / cfg.reso_col) + (float)cfg.half_col - 0.5f;
          int lv = 1;
          for (int l = 1; l < CC_NLEV; l++) lv += (h > cfg.lv_grads[l]) ? 1 : 0;
          nslot += lv;
          const int r = c / cfg.n_col;
          l_rc[i] = (uint16_t)((r << 8) | (c - r * cfg.n_col));
          l_lev[i] = (unsigned char)lv;
          l_h[i] = h;
          l_pix[i] = rcf;
        }
      }
    }
  } else {
  // (2) the dense image, the continuous position of every occupied cell, the list entries at their raster-order positions.
  // CC_K1_EB cells per thread at a time: their keys and owners first, the owners' records requested TOGETHER, then the
  // outputs -- one cell at a time every thread waited for its record 22 times in a row, a quarter of the kernel (round 6,
  // measured with clock probes).  A cell without an owner asks for the scan's first record and drops it.
  for (int c0 = 0; c0 < n_cell; c0 += nt * CC_K1_EB) {  // block-uniform trip counts: the ballots see whole waves
    unsigned key[CC_K1_EB];
    float2 xy[CC_K1_EB];
#pragma unroll
    for (int e = 0; e < CC_K1_EB; e++) {
      const int c = c0 + e * nt + tid;
      key[e] = c < n_cell ? keyfn(c) : KEY_EMPTY;
    }
#pragma unroll
    for (int e = 0; e < CC_K1_EB; e++) {
      const int c = c0 + e * nt + tid;
      const bool need = dense ? key[e] != KEY_EMPTY : cc_funkey(key[e]) > cfg.lv_grads[0];
      const int own = need ? idxfn(c) : 0;
      xy[e] = n_pts > 0 ? P.owner_xy(own) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int e = 0; e < CC_K1_EB; e++) {
      const int cb = c0 + e * nt;  // block-uniform
      if (cb >= n_cell) break;
      const int c = cb + tid;
      const float h = cc_funkey(key[e]);
      const bool act = h > cfg.lv_grads[0];  // cv::threshold BINARY is strict `>` (contour_mng.cpp:283)
      const unsigned long long m0 = __ballot(act);
      if (c < n_cell) {
        if (dense) bev[c] = h;
        if (key[e] != KEY_EMPTY) {
          // pointToContRowCol: x / reso + n_row/2 - 0.5f, left to right in f32 (a power-of-two resolution: the product with
          // its reciprocal is the same correctly rounded value)
          float2 rcf;
          rcf.x = (cfg.reso_pow2 ? xy[e].x * cfg.inv_row : xy[e].x / cfg.reso_row) + (float)cfg.half_row - 0.5f;
          rcf.y = (cfg.reso_pow2 ? xy[e].y * cfg.inv_col : xy[e].y / cfg.reso_col) + (float)cfg.half_col - 0.5f;
          if (dense) pix[c] = rcf;
          npix++;
          if (act) {
            int lv = 1;
            for (int l = 1; l < CC_NLEV; l++) lv += (h > cfg.lv_grads[l]) ? 1 : 0;
            nslot += lv;
            const int i = (int)cbase[c >> 6] + cc_mbcnt(m0);
            if (i < CC_LIST_CAP) {
              const int r = c / cfg.n_col;
              l_rc[i] = (uint16_t)((r << 8) | (c - r * cfg.n_col));
              l_lev[i] = (unsigned char)lv;
              l_h[i] = h;
              l_pix[i] = rcf;
            }
          }
        }
      }
    }
  }
  }
  nslot = cc_wave_sum(nslot);
  if (lane == 0 && nslot) atomicAdd(&tot[1], nslot);
  __syncthreads();
  if (tid == 0) L.hdr[scan] = make_int4(tot[0], tot[1], dense ? 1 : 0, 0);
  return npix;
}

// grid = n_scans (PART: n_scans * CC_K1_SPLIT), block = multiple of 64.  dynamic LDS: n_cell*4 + ((n_cell+2)/3)*8 + 16 + CC_K1_EMIT_LDS_BYTES bytes.
// The body of the sweep kernels.  P: the loader of the call's points, positioned at the first point of the call's first scan.
template <int CC_K1_U, bool CC_K1_POW2, bool PART, typename LD>
__device__ __forceinline__ void cc_k1_sweep(char *smem, const cc_dev_cfg &cfg, LD P, const long long *__restrict__ offsets,
                                            float *__restrict__ bev_out, float2 *__restrict__ pix_out, cc_k1_scan_out *__restrict__ scan_out,
                                            const cc_k1_part &part, const cc_k1_list_out &list_out, int want_dense) {
  const int n_cell = cfg.n_cell;
  unsigned *hmax = (unsigned *)smem;
  const int n_w3 = (n_cell + 2) / 3;
  unsigned long long *idx3 = (unsigned long long *)(smem + (((size_t)n_cell * 4 + 15) & ~(size_t)15));
  unsigned *red = (unsigned *)(idx3 + n_w3);  // [0]=max key [1]=min key [2]=n_pix
  char *emit_tab = (char *)(red + 4);          // CC_K1_EMIT_LDS_BYTES: the output pass' chunk tables
  unsigned *idle = (unsigned *)(emit_tab + CC_K1_EMIT_TAB_BYTES);  // [blockDim]: where a lane with nothing to send aims its atomicMax (the sweep's; the output pass has its cell list there)
  static_assert(CC_LIST_CAP * 2 >= 4 * 1024 && CC_K1_EMIT_TAB_BYTES % 4 == 0, "cc_k_rasterize: the idle words fit the list's cells");

  const int tid = threadIdx.x, nt = blockDim.x;
  const int unit = (int)blockIdx.x;  // a scan (PART: a range of one)
  const int scan = PART ? unit / CC_K1_SPLIT : unit;
  long long p0 = offsets[scan];
  int n_pts = (int)(offsets[scan + 1] - p0);
  int idx_base = 0;  // scan-relative index of this workgroup's first point
  if (PART) {
    const int per = (n_pts + CC_K1_SPLIT - 1) / CC_K1_SPLIT, pi = unit % CC_K1_SPLIT;
    idx_base = pi * per < n_pts ? pi * per : n_pts;
    n_pts = n_pts - idx_base < per ? n_pts - idx_base : per;
    p0 += idx_base;
  }
  P.advance(p0);

  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  for (int i = tid; i < n_cell; i += nt) hmax[i] = KEY_EMPTY;
  for (int i = tid; i < n_w3; i += nt) idx3[i] = ~0ull;
  idle[tid] = 0u;
  if (tid == 0) {
    red[0] = cc_fkey(CC_BEV_EMPTY);   // max_bin_val_ starts at -VAL_ABS_INF_ (contour_mng.h:436)
    red[1] = cc_fkey(-CC_BEV_EMPTY);  // min_bin_val_ starts at +VAL_ABS_INF_
    red[2] = 0;
  }
  __syncthreads();

  // ---- one sweep over the stream, in chunks of CC_K1_U * blockDim points held in registers ----
  // step A (all lanes): atomicMax of the chunk's heights; a point that RAISES a cell's maximum erases the cell's
  //                     index field (the index recorded so far belongs to a lower height)
  // step B (after a barrier): the chunk's points that equal the cell maximum min-reduce their index into the field.
  // A cell whose maximum dates from an earlier chunk keeps that (smaller) index: later equal heights never replace
  // it, which is the strict `bev < height` update of contour_mng.h:517.  The barrier after step B keeps the next
  // chunk's erasures behind this chunk's index updates.
  // min accepted height as a key (the map keeps the order); the max accepted height is the largest cell maximum: taken from
  // the grid on the way out
  unsigned kmin = cc_fkey(-CC_BEV_EMPTY);
  const int chunk = CC_K1_U * nt;
  // The records are loaded UNCONDITIONALLY from an index clamped to the scan's last point and a lane past the end drops
  // its point when it uses it: a load under a branch is waited for where the branch ends (round 6: the prefetch below was
  // no prefetch for two of the four loads).
  const int last = n_pts > 0 ? n_pts - 1 : 0;
  typename LD::rec q[CC_K1_U];
#pragma unroll
  for (int u = 0; u < CC_K1_U; u++) q[u] = LD::zero();
  if (n_pts > 0) {
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) {
      const int j = tid + u * nt;
      q[u] = P.load(j < last ? j : last);
    }
  }
  for (int base = 0; base < n_pts; base += chunk) {
    int cell[CC_K1_U];
    unsigned key[CC_K1_U];
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) {
      float px, py, pz;
      P.xyz(q[u], px, py, pz);
      const int c = cc_point_cell<CC_K1_POW2>(cfg, px, py);
      const float h = cfg.lidar_height + pz;
      key[u] = cc_fkey(h);
      // a NaN height never updates a cell or the max/min in the reference (`bev < NaN`, `max < NaN`, `min > NaN` are
      // all false, contour_mng.h:517-524): such a point is dropped here
      cell[u] = ((h == h) & (tid + u * nt < n_pts - base)) ? c : -1;
      const unsigned kb = cell[u] >= 0 ? key[u] : 0xFFFFFFFFu;
      kmin = kb < kmin ? kb : kmin;
    }
    // the next chunk's records travel while this chunk is resolved in LDS
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) {
      const int j = base + chunk + tid + u * nt;
      q[u] = P.load(j < last ? j : last);
    }
    // Consecutive records are neighbouring azimuth steps of one laser: close to the sensor dozens of them fall into
    // the same cell, and same-address LDS atomics of a wave are served one after the other.  So the lanes of a 16-lane
    // row first combine their heights per run of equal cells (segmented max over DPP row shifts), and only the last
    // lane of a run goes to the LDS, with the run's maximum.  Which lanes continue their left neighbour's run is ONE wave
    // mask; the masks of the wider steps ("the 2, 4, 8 lanes to my left are in my run") and the senders' come from it with
    // scalar shifts (round 6: a compare of shifted cells per step before) -- a step is a DPP max and a select.
    unsigned kr[CC_K1_U], was[CC_K1_U];
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) {
      const int c1 = cell[u] + 1;  // 0 = rejected point (and what a row shift reads beyond the row's end: a run ends at its row's end)
      unsigned k = cell[u] >= 0 ? key[u] : 0u;  // (rejected lanes form runs of their own, of zeros)
      const unsigned long long m1 = __ballot(cc_row_shr<1>(c1) == c1);
      const unsigned long long m2 = m1 & (m1 << 1), m4 = m2 & (m2 << 2), m8 = m4 & (m4 << 4);
      {
        const unsigned ok = (unsigned)cc_row_shr<1>((int)k);
        k = cc_mask_lane(m1) ? (ok > k ? ok : k) : k;
      }
      {
        const unsigned ok = (unsigned)cc_row_shr<2>((int)k);
        k = cc_mask_lane(m2) ? (ok > k ? ok : k) : k;
      }
      {
        const unsigned ok = (unsigned)cc_row_shr<4>((int)k);
        k = cc_mask_lane(m4) ? (ok > k ? ok : k) : k;
      }
      {
        const unsigned ok = (unsigned)cc_row_shr<8>((int)k);
        k = cc_mask_lane(m8) ? (ok > k ? ok : k) : k;
      }
      const unsigned long long last_of_run = ~(m1 >> 1) | 0x8000800080008000ull;
      kr[u] = cc_mask_lane(last_of_run) ? k : 0u;  // 0: this lane sends nothing (no height maps to key 0; a rejected lane holds 0)
    }
    // the chunk's atomics leave together (round 6: one after the other, each waited for, they were four LDS round trips)
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) was[u] = atomicMax(kr[u] ? &hmax[cell[u]] : &idle[tid], kr[u]);
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++)
      if (was[u] < kr[u]) {
        int w, sh;
        cc_k1_field(cell[u], n_w3, w, sh);
        atomicOr(&idx3[w], CC_K1_IDX_MASK << sh);
      }
      __syncthreads();
      // step B: which of this lane's points hold their cell's maximum (four reads in flight), then ONE loop in which a lane
    // works off its winners one CAS attempt per turn -- a retry and the next winner's first attempt share a turn
    unsigned pend = 0u;
    {
      unsigned hm[CC_K1_U];
#pragma unroll
      for (int u = 0; u < CC_K1_U; u++) hm[u] = hmax[cell[u] >= 0 ? cell[u] : 0];
#pragma unroll
      for (int u = 0; u < CC_K1_U; u++) pend |= (cell[u] >= 0 && key[u] == hm[u] && key[u] != KEY_EMPTY) ? (1u << u) : 0u;
    }
    {
      bool busy = false;
      int w = 0, sh = 0;
      unsigned long long j = 0ull, old = 0ull;
      while (pend || busy) {
        if (!busy) {
          const int u = __ffs(pend) - 1;
          pend &= pend - 1u;
          int c = cell[0];
#pragma unroll
          for (int v = 1; v < CC_K1_U; v++) c = u == v ? cell[v] : c;
          cc_k1_field(c, n_w3, w, sh);
          j = (unsigned long long)(idx_base + base + tid + u * nt);
          old = idx3[w];
          busy = true;
        }
        const unsigned long long cur = (old >> sh) & CC_K1_IDX_MASK;
        if (j >= cur) {
          busy = false;
        } else {
          const unsigned long long nw = (old & ~(CC_K1_IDX_MASK << sh)) | (j << sh);
          const unsigned long long got = atomicCAS(&idx3[w], old, nw);
          busy = got != old;
          old = got;
        }
      }
    }
      __syncthreads();
    }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned b2 = (unsigned)__shfl_xor((int)kmin, o);
    kmin = b2 < kmin ? b2 : kmin;
  }
  if ((tid & 63) == 0) atomicMin(&red[1], kmin);
  __syncthreads();

  if (PART) {  // this range's grid to the scratch; cc_k_rasterize_merge combines the ranges
    unsigned *pk = part.key + (size_t)unit * n_cell;
    int *pj = part.idx + (size_t)unit * n_cell;
    unsigned kmx = KEY_EMPTY;
    for (int c = tid; c < n_cell; c += nt) {
      const unsigned k = hmax[c];
      kmx = k > kmx ? k : kmx;
      pk[c] = k;
      int w, sh;
      cc_k1_field(c, n_w3, w, sh);
      pj[c] = k != KEY_EMPTY ? (int)((idx3[w] >> sh) & CC_K1_IDX_MASK) : -1;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned a = (unsigned)__shfl_xor((int)kmx, o);
      kmx = a > kmx ? a : kmx;
    }
    if ((tid & 63) == 0) atomicMax(&red[0], kmx);
    __syncthreads();
    if (tid == 0) {
      part.red[(size_t)unit * 2] = red[0];
      part.red[(size_t)unit * 2 + 1] = red[1];
    }
    return;
  }
  // ---- outputs ----
  float *bev = bev_out + (size_t)scan * n_cell;
  float2 *pix = pix_out + (size_t)scan * n_cell;
  int npix = cc_k1_emit(
      cfg,
      [&](int c) { return hmax[c]; },
      [&](int c) {
        int w, sh;
        cc_k1_field(c, n_w3, w, sh);
        return (int)((idx3[w] >> sh) & CC_K1_IDX_MASK);
      },
      P, bev, pix, list_out, scan, emit_tab, n_pts, want_dense, &red[0]);
  npix = cc_wave_sum(npix);
  if ((tid & 63) == 0) atomicAdd(&red[2], (unsigned)npix);
  __syncthreads();
  if (tid == 0) {
    cc_k1_scan_out o;
    o.max_bin_val = cc_funkey(red[0]);
    o.min_bin_val = cc_funkey(red[1]);
    o.n_pix = (int)red[2];
    o.pad = 0;
    scan_out[scan] = o;
  }
}

// The ranges of a scan combined: a cell's height is the largest of the ranges' keys and its point the one of the FIRST
// range that reaches it -- ranges are in file order and each holds the first of its own points, so this is the first point
// of the scan at that height: the reference's strict `bev < height` update (contour_mng.h:517) as in the one-sweep kernel.
// grid = n_scans, block = multiple of 64
template <typename LD>
__device__ __forceinline__ void cc_k1_merge(const cc_dev_cfg &cfg, LD P, const long long *__restrict__ offsets, const cc_k1_part &part,
                                            float *__restrict__ bev_out, float2 *__restrict__ pix_out, cc_k1_scan_out *__restrict__ scan_out,
                                            const cc_k1_list_out &list_out, int want_dense) {
  __shared__ unsigned red[3];
  __shared__ __attribute__((aligned(16))) char emit_tab[CC_K1_EMIT_LDS_BYTES];
  const int scan = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, n_cell = cfg.n_cell;
  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  P.advance(offsets[scan]);
  if (tid == 0) {
    unsigned mx = cc_fkey(CC_BEV_EMPTY), mn = cc_fkey(-CC_BEV_EMPTY);
    for (int p = 0; p < CC_K1_SPLIT; p++) {
      const unsigned a = part.red[((size_t)scan * CC_K1_SPLIT + p) * 2], b = part.red[((size_t)scan * CC_K1_SPLIT + p) * 2 + 1];
      mx = a > mx ? a : mx;
      mn = b < mn ? b : mn;
    }
    red[0] = mx;
    red[1] = mn;
    red[2] = 0;
  }
  __syncthreads();
  float *bev = bev_out + (size_t)scan * n_cell;
  float2 *pix = pix_out + (size_t)scan * n_cell;
  int npix = cc_k1_emit(
      cfg,
      [&](int c) {  // the largest of the ranges' keys
        unsigned best = KEY_EMPTY;
#pragma unroll
        for (int p = 0; p < CC_K1_SPLIT; p++) {
          const unsigned k = part.key[((size_t)scan * CC_K1_SPLIT + p) * n_cell + c];
          best = (k != KEY_EMPTY && (best == KEY_EMPTY || k > best)) ? k : best;
        }
        return best;
      },
      [&](int c) {  // ... and among equals the FIRST range's point (ranges are in file order)
        unsigned best = KEY_EMPTY;
        int bp = 0;
#pragma unroll
        for (int p = 0; p < CC_K1_SPLIT; p++) {
          const unsigned k = part.key[((size_t)scan * CC_K1_SPLIT + p) * n_cell + c];
          if (k != KEY_EMPTY && (best == KEY_EMPTY || k > best)) {
            best = k;
            bp = p;
          }
        }
        return part.idx[((size_t)scan * CC_K1_SPLIT + bp) * n_cell + c];
      },
      P, bev, pix, list_out, scan, emit_tab, (int)(offsets[scan + 1] - offsets[scan]), want_dense, nullptr);
  npix = cc_wave_sum(npix);
  if ((tid & 63) == 0) atomicAdd(&red[2], (unsigned)npix);
  __syncthreads();
  if (tid == 0) {
    cc_k1_scan_out o;
    o.max_bin_val = cc_funkey(red[0]);
    o.min_bin_val = cc_funkey(red[1]);
    o.n_pix = (int)red[2];
    o.pad = 0;
    scan_out[scan] = o;
  }
}
// ---- a scan made of several SEGMENTS (cc_ingest_segments): records in up to CC_SEG_MAX places, each with its own stride and its own
// optional transform; the scan is their points one after the other, and a point's index -- what the 21-bit fields hold, what step B
// min-reduces and what "the first range wins" in the merge kernel is about -- is its index in THAT sequence.  So the tie rule holds
// across segments with the logic above: the sweep only has to hand cc_k1_resolve the right j0.
struct cc_k1_seg {
  const char *base;  // x of the segment's first point
  unsigned stride;   // bytes between records
  int first;         // index within the scan of the segment's first point
  int n;             // points (0: the segment is skipped)
  int has_tf;
  float m[12];       // row-major 3 x 4, read when has_tf != 0
};
struct cc_k1_segs {
  const cc_k1_seg *seg;  // the call's segments, scan after scan
  const int *scan_seg;   // [n_scans + 1]: scan i is made of the segments scan_seg[i] .. scan_seg[i + 1] - 1
};
#define CC_K1_SEG_LDS_BYTES (CC_SEG_MAX * (int)sizeof(cc_k1_seg))  // a scan's table in LDS, behind cc_k1_sweep's layout: 2 304 of the 5 504 bytes K1 leaves of a CU's LDS at 150 x 150

// The scan's table to LDS (a barrier has to follow); returns the number of its segments.
__device__ __forceinline__ int cc_k1_seg_table(cc_k1_seg *T, const cc_k1_segs &segs, int scan) {
  const int s0 = segs.scan_seg[scan], n_seg = segs.scan_seg[scan + 1] - s0;
  const unsigned *__restrict__ src = (const unsigned *)(segs.seg + s0);
  unsigned *dst = (unsigned *)T;
  for (int i = threadIdx.x; i < n_seg * (int)(sizeof(cc_k1_seg) / 4); i += blockDim.x) dst[i] = src[i];
  return n_seg;
}

// The pieces of cc_k1_sweep's chunk loop as functions, for cc_k1_sweep_seg below, which runs them once per piece of a scan.  (cc_k1_sweep
// keeps its own text: built from these functions its instances came out with another register allocation and schedule, and the
// existing kernels are not to move -- a change to one of the two has to be made in the other.)
// The cells and height keys of the chunk's points that have arrived in q[]: lane tid (of nt) holds the points tid + u * nt of the
// chunk, of which the first n_left exist.  kmin: the smallest key of an accepted point.
template <int CC_K1_U, bool CC_K1_POW2, typename LD>
__device__ __forceinline__ void cc_k1_cells(const cc_dev_cfg &cfg, const LD &P, const typename LD::rec (&q)[CC_K1_U], int n_left, int (&cell)[CC_K1_U],
                                            unsigned (&key)[CC_K1_U], unsigned &kmin, const int tid, const int nt) {
#pragma unroll
  for (int u = 0; u < CC_K1_U; u++) {
    float px, py, pz;
    P.xyz(q[u], px, py, pz);
    const int c = cc_point_cell<CC_K1_POW2>(cfg, px, py);
    const float h = cfg.lidar_height + pz;
    key[u] = cc_fkey(h);
    // a NaN height never updates a cell or the max/min in the reference (`bev < NaN`, `max < NaN`, `min > NaN` are
    // all false, contour_mng.h:517-524): such a point is dropped here
    cell[u] = ((h == h) & (tid + u * nt < n_left)) ? c : -1;
    const unsigned kb = cell[u] >= 0 ? key[u] : 0xFFFFFFFFu;
    kmin = kb < kmin ? kb : kmin;
  }
}

// Steps A and B (cc_k1_sweep) for one chunk; j0: the scan-relative index of the chunk's first point.  Two barriers.
template <int CC_K1_U>
__device__ __forceinline__ void cc_k1_resolve(unsigned *hmax, unsigned long long *idx3, unsigned *idle, int n_w3, const int (&cell)[CC_K1_U],
                                              const unsigned (&key)[CC_K1_U], int j0, const int tid, const int nt) {
  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  // Consecutive records are neighbouring azimuth steps of one laser: close to the sensor dozens of them fall into
  // the same cell, and same-address LDS atomics of a wave are served one after the other.  So the lanes of a 16-lane
  // row first combine their heights per run of equal cells (segmented max over DPP row shifts), and only the last
  // lane of a run goes to the LDS, with the run's maximum.  Which lanes continue their left neighbour's run is ONE wave
  // mask; the masks of the wider steps ("the 2, 4, 8 lanes to my left are in my run") and the senders' come from it with
  // scalar shifts (round 6: a compare of shifted cells per step before) -- a step is a DPP max and a select.
  unsigned kr[CC_K1_U], was[CC_K1_U];
#pragma unroll
  for (int u = 0; u < CC_K1_U; u++) {
    const int c1 = cell[u] + 1;  // 0 = rejected point (and what a row shift reads beyond the row's end: a run ends at its row's end)
    unsigned k = cell[u] >= 0 ? key[u] : 0u;  // (rejected lanes form runs of their own, of zeros)
    const unsigned long long m1 = __ballot(cc_row_shr<1>(c1) == c1);
    const unsigned long long m2 = m1 & (m1 << 1), m4 = m2 & (m2 << 2), m8 = m4 & (m4 << 4);
    {
      const unsigned ok = (unsigned)cc_row_shr<1>((int)k);
      k = cc_mask_lane(m1) ? (ok > k ? ok : k) : k;
    }
    {
      const unsigned ok = (unsigned)cc_row_shr<2>((int)k);
      k = cc_mask_lane(m2) ? (ok > k ? ok : k) : k;
    }
    {
      const unsigned ok = (unsigned)cc_row_shr<4>((int)k);
      k = cc_mask_lane(m4) ? (ok > k ? ok : k) : k;
    }
    {
      const unsigned ok = (unsigned)cc_row_shr<8>((int)k);
      k = cc_mask_lane(m8) ? (ok > k ? ok : k) : k;
    }
    const unsigned long long last_of_run = ~(m1 >> 1) | 0x8000800080008000ull;
    kr[u] = cc_mask_lane(last_of_run) ? k : 0u;  // 0: this lane sends nothing (no height maps to key 0; a rejected lane holds 0)
  }
  // the chunk's atomics leave together (round 6: one after the other, each waited for, they were four LDS round trips)
#pragma unroll
  for (int u = 0; u < CC_K1_U; u++) was[u] = atomicMax(kr[u] ? &hmax[cell[u]] : &idle[tid], kr[u]);
#pragma unroll
  for (int u = 0; u < CC_K1_U; u++)
    if (was[u] < kr[u]) {
      int w, sh;
      cc_k1_field(cell[u], n_w3, w, sh);
      atomicOr(&idx3[w], CC_K1_IDX_MASK << sh);
    }
  __syncthreads();
  // step B: which of this lane's points hold their cell's maximum (four reads in flight), then ONE loop in which a lane
  // works off its winners one CAS attempt per turn -- a retry and the next winner's first attempt share a turn
  unsigned pend = 0u;
  {
    unsigned hm[CC_K1_U];
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) hm[u] = hmax[cell[u] >= 0 ? cell[u] : 0];
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) pend |= (cell[u] >= 0 && key[u] == hm[u] && key[u] != KEY_EMPTY) ? (1u << u) : 0u;
  }
  {
    bool busy = false;
    int w = 0, sh = 0;
    unsigned long long j = 0ull, old = 0ull;
    while (pend || busy) {
      if (!busy) {
        const int u = __ffs(pend) - 1;
        pend &= pend - 1u;
        int c = cell[0];
#pragma unroll
        for (int v = 1; v < CC_K1_U; v++) c = u == v ? cell[v] : c;
        cc_k1_field(c, n_w3, w, sh);
        j = (unsigned long long)(j0 + tid + u * nt);
        old = idx3[w];
        busy = true;
      }
      const unsigned long long cur = (old >> sh) & CC_K1_IDX_MASK;
      if (j >= cur) {
        busy = false;
      } else {
        const unsigned long long nw = (old & ~(CC_K1_IDX_MASK << sh)) | (j << sh);
        const unsigned long long got = atomicCAS(&idx3[w], old, nw);
        busy = got != old;
        old = got;
      }
    }
  }
  __syncthreads();
}

// What follows a sweep: the min key, then (PART) the range's grid to the scratch or the output pass.  n_pts: the points this workgroup swept.
template <bool PART, typename LD>
__device__ __forceinline__ void cc_k1_finish(const cc_dev_cfg &cfg, const LD &P, unsigned *hmax, unsigned long long *idx3, unsigned *red, char *emit_tab, int n_w3,
                                             unsigned kmin, int unit, int scan, int n_pts, float *__restrict__ bev_out, float2 *__restrict__ pix_out,
                                             cc_k1_scan_out *__restrict__ scan_out, const cc_k1_part &part, const cc_k1_list_out &list_out, int want_dense,
                                             const int tid, const int nt) {
  const int n_cell = cfg.n_cell;
  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned b2 = (unsigned)__shfl_xor((int)kmin, o);
    kmin = b2 < kmin ? b2 : kmin;
  }
  if ((tid & 63) == 0) atomicMin(&red[1], kmin);
  __syncthreads();

  if (PART) {  // this range's grid to the scratch; cc_k_rasterize_merge combines the ranges
    unsigned *pk = part.key + (size_t)unit * n_cell;
    int *pj = part.idx + (size_t)unit * n_cell;
    unsigned kmx = KEY_EMPTY;
    for (int c = tid; c < n_cell; c += nt) {
      const unsigned k = hmax[c];
      kmx = k > kmx ? k : kmx;
      pk[c] = k;
      int w, sh;
      cc_k1_field(c, n_w3, w, sh);
      pj[c] = k != KEY_EMPTY ? (int)((idx3[w] >> sh) & CC_K1_IDX_MASK) : -1;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned a = (unsigned)__shfl_xor((int)kmx, o);
      kmx = a > kmx ? a : kmx;
    }
    if ((tid & 63) == 0) atomicMax(&red[0], kmx);
    __syncthreads();
    if (tid == 0) {
      part.red[(size_t)unit * 2] = red[0];
      part.red[(size_t)unit * 2 + 1] = red[1];
    }
    return;
  }
  // ---- outputs ----
  float *bev = bev_out + (size_t)scan * n_cell;
  float2 *pix = pix_out + (size_t)scan * n_cell;
  int npix = cc_k1_emit(
      cfg,
      [&](int c) { return hmax[c]; },
      [&](int c) {
        int w, sh;
        cc_k1_field(c, n_w3, w, sh);
        return (int)((idx3[w] >> sh) & CC_K1_IDX_MASK);
      },
      P, bev, pix, list_out, scan, emit_tab, n_pts, want_dense, &red[0]);
  npix = cc_wave_sum(npix);
  if ((tid & 63) == 0) atomicAdd(&red[2], (unsigned)npix);
  __syncthreads();
  if (tid == 0) {
    cc_k1_scan_out o;
    o.max_bin_val = cc_funkey(red[0]);
    o.min_bin_val = cc_funkey(red[1]);
    o.n_pix = (int)red[2];
    o.pad = 0;
    scan_out[scan] = o;
  }
}

// The output pass' loader: the owner of a cell is known by its index within the scan -- its segment is the last one that begins at
// or before it (a search over at most CC_SEG_MAX prefix sums; empty segments share their successor's `first` and are passed over),
// and the point is moved by THAT segment's matrix, per lane, with cc_ld_rec::xyz's operations in its order.
struct cc_ld_segs {
  const cc_k1_seg *T;  // LDS
  int n_seg;
  __device__ __forceinline__ void advance(long long) {}
  __device__ __forceinline__ float2 owner_xy(int j) const {
    int s = 0;
    for (int i = 1; i < n_seg; i++) s += j >= T[i].first ? 1 : 0;
    const cc_k1_seg &g = T[s];
    float x, y, z;
    cc_load3f(g.base + (unsigned)(j - g.first) * g.stride, x, y, z);
    const float tx = ((g.m[0] * x + g.m[1] * y) + g.m[2] * z) + g.m[3];
    const float ty = ((g.m[4] * x + g.m[5] * y) + g.m[6] * z) + g.m[7];
    return g.has_tf ? make_float2(tx, ty) : make_float2(x, y);
  }
};

// The record loader seated on segment s, lo points into it.  Workgroup-uniform like cc_ld_rec's arguments: stride and matrix stay scalars.
__device__ __forceinline__ cc_ld_rec<0> cc_k1_seg_loader(const cc_k1_seg *T, int s, int lo) {
  const cc_k1_seg &g = T[s];
  cc_ld_rec<0> P(cc_uniform_ptr(g.base), cc_uniform_i((int)g.stride), cc_uniform_i(g.has_tf) ? g.m : nullptr, 0);
  P.advance(lo);
  return P;
}

// cc_k1_sweep for a scan of segments.  The workgroup's range of the scan (all of it; PART: one of CC_K1_SPLIT ranges, which may begin
// and end inside segments) is cut into PIECES, one per segment that has points in it, and the chunk loop restarts with every piece:
// stride and matrix are what they are in cc_ld_rec -- scalars, re-seated between pieces -- at the price of one partly filled chunk
// per piece.  The prefetch stays unconditional across pieces: a piece's last chunk requests the first records of the NEXT piece (the
// base, the stride and the clamp are selected as scalars; the load itself is under no branch).  tab_off: where the table goes in smem.
template <int CC_K1_U, bool CC_K1_POW2, bool PART>
__device__ __forceinline__ void cc_k1_sweep_seg(char *smem, int tab_off, const cc_dev_cfg &cfg, const cc_k1_segs &segs, const long long *__restrict__ offsets,
                                                float *__restrict__ bev_out, float2 *__restrict__ pix_out, cc_k1_scan_out *__restrict__ scan_out,
                                                const cc_k1_part &part, const cc_k1_list_out &list_out, int want_dense) {
  const int n_cell = cfg.n_cell;
  unsigned *hmax = (unsigned *)smem;  // (cc_k1_sweep's layout)
  const int n_w3 = (n_cell + 2) / 3;
  unsigned long long *idx3 = (unsigned long long *)(smem + (((size_t)n_cell * 4 + 15) & ~(size_t)15));
  unsigned *red = (unsigned *)(idx3 + n_w3);
  char *emit_tab = (char *)(red + 4);
  unsigned *idle = (unsigned *)(emit_tab + CC_K1_EMIT_TAB_BYTES);
  cc_k1_seg *T = (cc_k1_seg *)(smem + tab_off);

  const int tid = threadIdx.x, nt = blockDim.x;
  const int unit = (int)blockIdx.x;
  const int scan = PART ? unit / CC_K1_SPLIT : unit;
  int n_pts = (int)(offsets[scan + 1] - offsets[scan]);  // of the whole scan: the segments' counts added up
  int idx_base = 0;
  if (PART) {  // the same ranges as cc_k1_sweep's
    const int per = (n_pts + CC_K1_SPLIT - 1) / CC_K1_SPLIT, pi = unit % CC_K1_SPLIT;
    idx_base = pi * per < n_pts ? pi * per : n_pts;
    n_pts = n_pts - idx_base < per ? n_pts - idx_base : per;
  }
  const int n_seg = cc_k1_seg_table(T, segs, scan);
  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  for (int i = tid; i < n_cell; i += nt) hmax[i] = KEY_EMPTY;
  for (int i = tid; i < n_w3; i += nt) idx3[i] = ~0ull;
  idle[tid] = 0u;
  if (tid == 0) {
    red[0] = cc_fkey(CC_BEV_EMPTY);
    red[1] = cc_fkey(-CC_BEV_EMPTY);
    red[2] = 0;
  }
  __syncthreads();

  // the first segment from s on with points in the range: `lo` points into it, cnt of them (n_seg: none left)
  const int q0 = idx_base, q1 = idx_base + n_pts;
  auto piece = [&](int s, int &lo, int &cnt) {
    for (; s < n_seg; s++) {
      const int f = T[s].first, hi = q1 - f < T[s].n ? q1 - f : T[s].n;
      lo = q0 > f ? q0 - f : 0;
      cnt = hi - lo;
      if (cnt > 0) break;
    }
    lo = cc_uniform_i(lo);
    cnt = cc_uniform_i(cnt);
    return cc_uniform_i(s);
  };
  unsigned kmin = cc_fkey(-CC_BEV_EMPTY);
  const int chunk = CC_K1_U * nt;
  int lo = 0, cnt = 0;
  int s = piece(0, lo, cnt);
  if (s < n_seg) {
    cc_ld_rec<0> P = cc_k1_seg_loader(T, s, lo);
    cc_xyz q[CC_K1_U];
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) {
      const int j = tid + u * nt;
      q[u] = P.load(j < cnt - 1 ? j : cnt - 1);
    }
    while (s < n_seg) {
      int lo2 = 0, cnt2 = 0;
      const int s2 = piece(s + 1, lo2, cnt2);
      // what this piece's last chunk prefetches: the next piece's first records (the last piece: its own last record, dropped)
      const char *nB = P.B;
      unsigned nstride = P.stride;
      int nlast = cnt - 1;
      if (s2 < n_seg) {
        nstride = (unsigned)cc_uniform_i((int)T[s2].stride);
        nB = cc_uniform_ptr(T[s2].base) + (long long)lo2 * (long long)nstride;
        nlast = cnt2 - 1;
      }
      const int j_piece = cc_uniform_i(T[s].first) + lo;  // index within the scan of the piece's first point
      for (int base = 0; base < cnt; base += chunk) {
        int cell[CC_K1_U];
        unsigned key[CC_K1_U];
        cc_k1_cells<CC_K1_U, CC_K1_POW2>(cfg, P, q, cnt - base, cell, key, kmin, tid, nt);
        const bool more = base + chunk < cnt;
        const char *lB = more ? P.B : nB;
        const unsigned lstride = more ? P.stride : nstride;
        const int l0 = more ? base + chunk : 0, llast = more ? cnt - 1 : nlast;
#pragma unroll
        for (int u = 0; u < CC_K1_U; u++) {
          const int j = l0 + tid + u * nt;
          cc_load3f(lB + (unsigned)(j < llast ? j : llast) * lstride, q[u].x, q[u].y, q[u].z);
        }
        cc_k1_resolve<CC_K1_U>(hmax, idx3, idle, n_w3, cell, key, j_piece + base, tid, nt);
      }
      s = s2;
      lo = lo2;
      cnt = cnt2;
      if (s < n_seg) P = cc_k1_seg_loader(T, s, lo);
    }
  }
  cc_k1_finish<PART>(cfg, cc_ld_segs{T, n_seg}, hmax, idx3, red, emit_tab, n_w3, kmin, unit, scan, n_pts, bev_out, pix_out, scan_out, part, list_out, want_dense, tid, nt);
}

// ---- a sweep DE-SKEWED by per-point time (cc_ingest_points_motion): every record carries a 4-byte time word, every scan brings
// K <= CC_MOTION_KNOTS_MAX matrices ("knots", piecewise constant over the sweep), and a point is moved by the knot of ITS time bin
//     u = (t - t_begin) * scale   (CC_TIME_U32: (float)(uint32)(w - tb) * scale, the subtraction modulo 2^32)
//     b = trunc(min(max(u, 0), K - 1))     -- NaN counts as 0; clamped BEFORE the conversion, so no out-of-range float -> int
// with cc_ld_rec::xyz's operations in its order.  The scan's knots sit in LDS behind cc_k1_sweep's layout (at most 3 072 B: 161 408 B
// at 150 x 150, still one 1 024-thread workgroup per CU); a point's matrix is three 16-byte LDS reads at a per-lane address.  The
// records of one wave are neighbouring firings: mostly one bin, and equal addresses are a broadcast, not a conflict.
// No interpolation between knots: it would double the LDS reads and add 12 multiply-adds per point to an issue-bound sweep.
#define CC_K1_MOT_KNOTS_MAX 64  // = CC_MOTION_KNOTS_MAX (include/cont2_amd.h; checked where both are seen)
#define CC_K1_MOT_LDS_BYTES (CC_K1_MOT_KNOTS_MAX * 12 * 4)
struct cc_k1_motion {
  const float *time;   // [n_scans][2]: t_begin (CC_TIME_U32: the u32's bits), scale
  const float *knots;  // [n_scans][n_knots][12]
  int t_off;           // byte offset of the time word from the record's x (negative: the time sits in front of xyz)
  int time_u32;        // the time word is a u32 (CC_TIME_U32), not an f32
  int n_knots;
};

// The scan's knots to LDS (a barrier has to follow before xyz() is called: cc_k1_sweep's after it has cleared the grid, the merge kernel's own).
__device__ __forceinline__ void cc_k1_knot_table(float *T, const cc_k1_motion &M, int scan) {
  const float *__restrict__ src = M.knots + (size_t)scan * (size_t)M.n_knots * 12;
  for (int i = threadIdx.x; i < M.n_knots * 12; i += blockDim.x) T[i] = src[i];
}

struct cc_xyzt {
  float x, y, z;
  unsigned w;  // the time word as it lies in the record
};
template <int STRIDE>
struct cc_ld_rec_motion {
  typedef cc_xyzt rec;
  const char *__restrict__ B;  // x of the first point
  unsigned stride;             // bytes (cc_ld_rec's bounds)
  int t_off;
  bool time_u32;               // workgroup-uniform
  float t_begin, scale;        // workgroup-uniform: scalars
  unsigned tb_bits;
  float kmax;                  // n_knots - 1
  const float4 *T;             // LDS: [n_knots][3] rows of the scan's matrices
  __device__ __forceinline__ cc_ld_rec_motion(const char *base, int stride_bytes, const cc_k1_motion &M, int scan, const float *lds_tab)
      : B(base), stride(STRIDE ? (unsigned)STRIDE : (unsigned)stride_bytes), t_off(M.t_off), time_u32(M.time_u32 != 0), T((const float4 *)lds_tab) {
    tb_bits = (unsigned)cc_uniform_i(__float_as_int(M.time[(size_t)scan * 2]));
    t_begin = __int_as_float((int)tb_bits);
    scale = __int_as_float(cc_uniform_i(__float_as_int(M.time[(size_t)scan * 2 + 1])));
    kmax = (float)(M.n_knots - 1);
  }
  __device__ __forceinline__ void advance(long long n) { B += n * (long long)stride; }
  // the coordinates and the time word are requested together, neither under a branch
  __device__ __forceinline__ rec load(int j) const {
    cc_xyzt q;
    const char *p = B + (unsigned)j * stride;
    cc_load3f(p, q.x, q.y, q.z);
    q.w = *(const unsigned *)(p + t_off);
    return q;
  }
  __device__ __forceinline__ static rec zero() { return cc_xyzt{0.f, 0.f, 0.f, 0u}; }
  __device__ __forceinline__ int bin(unsigned w) const {
    float u = time_u32 ? (float)(w - tb_bits) * scale : (__int_as_float((int)w) - t_begin) * scale;
    u = u > 0.f ? u : 0.f;  // (a NaN fails the compare: bin 0)
    u = u < kmax ? u : kmax;
    return (int)u;
  }
  __device__ __forceinline__ void xyz(const rec &q, float &x, float &y, float &z) const {
    const int b = bin(q.w);
    const float4 r0 = T[b * 3], r1 = T[b * 3 + 1], r2 = T[b * 3 + 2];
    x = ((r0.x * q.x + r0.y * q.y) + r0.z * q.z) + r0.w;
    y = ((r1.x * q.x + r1.y * q.y) + r1.z * q.z) + r1.w;
    z = ((r2.x * q.x + r2.y * q.y) + r2.z * q.z) + r2.w;
  }
  __device__ __forceinline__ float2 owner_xy(int j) const {
    float x, y, z;
    xyz(load(j), x, y, z);
    return make_float2(x, y);
  }
};

// ---- a sensor's RANGE IMAGE rasterised in place (cc_ingest_ranges): a scan is H x W range words (u16 / u32 / f32), one per
// (beam, firing) = (row, col); the sensor model -- per-row (cos alt, sin alt, cos az_off, sin az_off), per-column (cos az, sin az,
// knot) -- is a few KB shared by every scan of every call.  A pixel becomes a point by the header's formula (f32, every product and
// sum rounded once: the library is built -ffp-contract=off), is moved by the knot of ITS COLUMN when the call brings knots, and a
// pixel without a return gets x = NaN: cc_point_cell rejects it like any NaN point.  A point's index -- what the 21-bit fields hold
// and the tie rule is about -- is its pixel's storage index j within the scan.
//   load(j)  : the range word (2 or 4 bytes) and the pixel's column entry (ONE 16-byte load), both from the clamped index and
//              neither under a branch; the row goes along in the record (xyz() sees only the record).
//   j -> (row, col): q = j / D with D = n_cols (row-major) or n_rows (col-major), r = j - q * D.  D a power of two: a shift.
//              Otherwise q = (j * M) >> 33 with M = ceil(2^33 / D), a 64-bit product.  Exact for every j < 2^21 and D <= 2^12:
//              M = (2^33 + e) / D with 0 <= e < D, so j * M / 2^33 = j / D + j * e / (D * 2^33), and the second term is below
//              1 / D because j * e < 2^21 * 2^12 = 2^33 -- it cannot carry j / D (whose fraction is at most (D - 1) / D) to the
//              next integer.  M < 2^32 for D >= 3 (D = 1, 2 take the shift), and j * M < 2^53.
// The row table (H x 16 B <= 2 048 B) and the scan's knots (<= 3 072 B) sit in LDS behind cc_k1_sweep's layout: 158 336 + 5 120 =
// 163 456 of 163 840 B at 150 x 150, still one 1 024-thread workgroup per CU.  A wave's 64 pixels are neighbouring firings of one beam
// (row-major) or neighbouring beams of one firing (col-major): row entry and knot are mostly one address -- a broadcast.
#define CC_K1_RNG_ROWS_MAX 128   // = CC_RANGE_ROWS_MAX (include/cont2_amd.h; checked where both are seen)
#define CC_K1_RNG_COLS_MAX 4096  // = CC_RANGE_COLS_MAX
#define CC_K1_RNG_ROW_LDS_BYTES (CC_K1_RNG_ROWS_MAX * 16)
#define CC_K1_RNG_LDS_BYTES (CC_K1_RNG_ROW_LDS_BYTES + CC_K1_MOT_LDS_BYTES)
#define CC_K1_RNG_MAGIC_SHIFT 33
static_assert(((CC_MAX_CELLS * 4 + 15) & ~15) + ((CC_MAX_CELLS + 2) / 3) * 8 + 64 + ((CC_K1_EMIT_LDS_BYTES + 15) & ~15) + CC_K1_RNG_LDS_BYTES <= 160 * 1024,
              "cc_src_rng: grid, index fields, output tables, row table and knots fit a CU's 160 KB of LDS");
enum { CC_K1_WORD_U16 = 0, CC_K1_WORD_U32 = 1, CC_K1_WORD_F32 = 2 };  // = CC_RANGE_U16 / _U32 / _F32
struct cc_k1_range {
  const void *words;    // the call's (chunk's) first range word
  const float4 *row;    // [n_rows]: cos(alt), sin(alt), cos(az_off), sin(az_off)
  const float4 *col;    // [n_cols]: cos(az), sin(az), the knot index's bits, 0
  const float *knots;   // [n_scans][n_knots][12], nullptr when n_knots == 0
  int n_rows, n_cols;
  int col_major;        // j = col * n_rows + row (else row * n_cols + col)
  int div_shift;        // >= 0: the divisor is 1 << div_shift; -1: div_magic
  unsigned div_magic;   // ceil(2^33 / divisor)
  int n_knots;
  float range_scale, origin_n, origin_z;
};

// The row table and the scan's knots to LDS (a barrier has to follow before xyz() is called).  T: CC_K1_RNG_LDS_BYTES.
__device__ __forceinline__ void cc_k1_range_tables(char *T, const cc_k1_range &R, int scan) {
  float4 *rows = (float4 *)T;
  for (int i = threadIdx.x; i < R.n_rows; i += blockDim.x) rows[i] = R.row[i];
  float *kn = (float *)(T + CC_K1_RNG_ROW_LDS_BYTES);
  const float *__restrict__ src = R.knots + (size_t)scan * (size_t)R.n_knots * 12;
  for (int i = threadIdx.x; i < R.n_knots * 12; i += blockDim.x) kn[i] = src[i];
}

struct cc_rng_rec {
  unsigned w;  // the range word as it lies in the image (u16: zero-extended)
  int row;
  float4 c;    // the pixel's column entry
};
template <int WORD>
struct cc_ld_range {
  typedef cc_rng_rec rec;
  const char *__restrict__ B;       // the word of pixel j0 of the scan
  const float4 *__restrict__ C;     // column entries (global: 64 KB at most, L2-resident)
  const float4 *rows;               // LDS
  const float4 *T;                  // LDS: [n_knots][3] rows of the scan's matrices
  long long first;                  // index within the call of the scan's first pixel
  int j0;                           // scan-relative index of the pixel B points at
  int divisor, div_shift;           // workgroup-uniform: scalars
  unsigned div_magic;
  bool col_major, has_knots;
  float range_scale, origin_n, origin_z;
  __device__ __forceinline__ cc_ld_range(const cc_k1_range &R, int scan, const char *lds_tab)
      : B((const char *)R.words), C(R.col), rows((const float4 *)lds_tab), T((const float4 *)(lds_tab + CC_K1_RNG_ROW_LDS_BYTES)),
        first((long long)scan * ((long long)R.n_rows * R.n_cols)), j0(0), divisor(R.col_major ? R.n_rows : R.n_cols), div_shift(R.div_shift),
        div_magic(R.div_magic), col_major(R.col_major != 0), has_knots(R.n_knots > 0), range_scale(R.range_scale), origin_n(R.origin_n),
        origin_z(R.origin_z) {}
  // n: index within the call of the first pixel this workgroup reads (the scan's first, or a part's, in the middle of a row)
  __device__ __forceinline__ void advance(long long n) {
    B += n * (long long)(WORD == CC_K1_WORD_U16 ? 2 : 4);
    j0 = (int)(n - first);
  }
  __device__ __forceinline__ rec load(int j) const {
    cc_rng_rec q;
    if (WORD == CC_K1_WORD_U16) q.w = *(const unsigned short *)(B + (unsigned)j * 2u);
    else q.w = *(const unsigned *)(B + (unsigned)j * 4u);
    const unsigned p = (unsigned)(j0 + j);  // < 2^21
    const unsigned d = div_shift >= 0 ? p >> div_shift : (unsigned)(((unsigned long long)p * (unsigned long long)div_magic) >> CC_K1_RNG_MAGIC_SHIFT);
    const unsigned r = p - d * (unsigned)divisor;
    q.row = (int)(col_major ? r : d);
    q.c = C[col_major ? d : r];
    return q;
  }
  __device__ __forceinline__ static rec zero() { return cc_rng_rec{0u, 0, make_float4(0.f, 0.f, 0.f, 0.f)}; }
  __device__ __forceinline__ void xyz(const rec &q, float &x, float &y, float &z) const {
    const float4 rt = rows[q.row];
    const float ca = rt.x, sa = rt.y, co = rt.z, so = rt.w, ce = q.c.x, se = q.c.y;
    float r;
    bool none;
    if (WORD == CC_K1_WORD_F32) {
      const float f = __int_as_float((int)q.w);
      none = !(f > 0.f);  // zero, negative or NaN: no return
      r = f * range_scale;
    } else {
      none = q.w == 0u;
      r = (float)q.w * range_scale;
    }
    const float d = r - origin_n;
    const float h = d * ca;
    const float dx = (ce * co) - (se * so), dy = (se * co) + (ce * so);
    float px = (h * dx) + (origin_n * ce), py = (h * dy) + (origin_n * se), pz = (d * sa) + origin_z;
    if (has_knots) {  // workgroup-uniform
      const int b = __float_as_int(q.c.z);
      const float4 r0 = T[b * 3], r1 = T[b * 3 + 1], r2 = T[b * 3 + 2];
      const float tx = ((r0.x * px + r0.y * py) + r0.z * pz) + r0.w;
      const float ty = ((r1.x * px + r1.y * py) + r1.z * pz) + r1.w;
      const float tz = ((r2.x * px + r2.y * py) + r2.z * pz) + r2.w;
      px = tx;
      py = ty;
      pz = tz;
    }
    x = none ? __int_as_float(0x7FC00000) : px;  // cc_point_cell rejects a NaN x: the pixel owns nothing and counts nowhere
    y = py;
    z = pz;
  }
  __device__ __forceinline__ float2 owner_xy(int j) const {
    float x, y, z;
    xyz(load(j), x, y, z);
    return make_float2(x, y);
  }
};

// ---- records DROPPED by a word of their own (cc_ingest_points_filtered, include/cont2_amd_filter.h): every record carries a label, ring,
// tag or intensity word, and a rule on that word says whether the record is kept.  A dropped record gets x = NaN after cc_ld_rec::xyz's
// operations, as a range image's pixel without a return does: cc_point_cell rejects it, so it owns no cell, takes part in no tie and
// counts in no minimum -- no new branch, and the result is cc_ingest_points' for the records with those x replaced by NaN.
//   CC_K1_FLT_CLASS : class = (dword >> shift) & mask of the ALIGNED dword that holds the word -- records are 4-byte aligned and
//                     strides multiples of 4, so that dword is in bounds wherever the word is; the host folds the word's byte
//                     position and width into the one shift and the one mask, which makes u8, u16 and u32 words ONE instance.
//                     kept = bit min(class, n_classes) of the call's table: bit n_classes holds keep_other, so a class beyond the
//                     table costs one v_min_u32, not a compare and two selects.  The table (CC_K1_FLT_CLASSES_MAX + 1 bits, 528 B
//                     with the padding) sits in LDS behind cc_k1_sweep's layout: one ds_read_b32 at a per-lane address, a shift and
//                     an AND per point.  The records of a wave are neighbouring firings, mostly of one class: equal addresses are a
//                     broadcast.
//   CC_K1_FLT_RANGE : kept = lo <= v && v <= hi on the f32 word (a NaN fails both compares); no table.
// The stride is a run-time value and has_tf cc_ld_rec's workgroup-uniform switch: 4 sweep instances and 1 merge instance per kind.
#define CC_K1_FLT_CLASSES_MAX 4096  // = CC_FILTER_CLASSES_MAX (include/cont2_amd_filter.h; checked where both are seen)
#define CC_K1_FLT_TAB_WORDS (CC_K1_FLT_CLASSES_MAX / 32 + 1)
#define CC_K1_FLT_LDS_BYTES ((CC_K1_FLT_TAB_WORDS * 4 + 15) & ~15)
static_assert(((CC_MAX_CELLS * 4 + 15) & ~15) + ((CC_MAX_CELLS + 2) / 3) * 8 + 64 + ((CC_K1_EMIT_LDS_BYTES + 15) & ~15) + CC_K1_FLT_LDS_BYTES <= 160 * 1024,
              "cc_src_flt: grid, index fields, output tables and the class table fit a CU's 160 KB of LDS");
enum { CC_K1_FLT_CLASS = 0, CC_K1_FLT_RANGE = 1 };
struct cc_k1_filter {
  const unsigned *bits;  // CLASS: the call's table, CC_K1_FLT_TAB_WORDS words (bit n_classes = keep_other, the bits behind it 0)
  int w_off;             // byte offset from the record's x of the dword the loader reads (negative: the word sits in front of xyz)
  unsigned shift, mask;  // CLASS: class = (dword >> shift) & mask
  unsigned n_classes;
  float lo, hi;          // RANGE
};

// The call's table to LDS (a barrier has to follow before xyz() is called).  T: CC_K1_FLT_LDS_BYTES.
__device__ __forceinline__ void cc_k1_filter_table(unsigned *T, const cc_k1_filter &F) {
  for (int i = threadIdx.x; i < CC_K1_FLT_TAB_WORDS; i += blockDim.x) T[i] = F.bits[i];
}

template <int KIND>
struct cc_ld_rec_flt {
  typedef cc_xyzt rec;         // (w: the filter word's dword as it lies in the record)
  cc_ld_rec<0> R;              // base, run-time stride, the workgroup-uniform transform: cc_ld_rec's, used as they are
  int w_off;
  unsigned shift, mask, n_classes;  // workgroup-uniform: scalars
  float lo, hi;
  const unsigned *T;           // LDS (CLASS)
  __device__ __forceinline__ cc_ld_rec_flt(const char *base, int stride_bytes, const float *__restrict__ tf, int scan, const cc_k1_filter &F, const unsigned *lds_tab)
      : R(base, stride_bytes, tf, scan), w_off(F.w_off), shift(F.shift), mask(F.mask), n_classes(F.n_classes), lo(F.lo), hi(F.hi), T(lds_tab) {}
  __device__ __forceinline__ void advance(long long n) { R.advance(n); }
  // the coordinates and the filter word are requested together, neither under a branch
  __device__ __forceinline__ rec load(int j) const {
    cc_xyzt q;
    const char *p = R.B + (unsigned)j * R.stride;
    cc_load3f(p, q.x, q.y, q.z);
    q.w = *(const unsigned *)(p + w_off);
    return q;
  }
  __device__ __forceinline__ static rec zero() { return cc_xyzt{0.f, 0.f, 0.f, 0u}; }
  __device__ __forceinline__ bool keep(unsigned w) const {
    if (KIND == CC_K1_FLT_RANGE) {
      const float v = __int_as_float((int)w);
      return (lo <= v) & (v <= hi);  // (a NaN fails both)
    }
    unsigned cls = (w >> shift) & mask;
    cls = cls < n_classes ? cls : n_classes;  // <= CC_K1_FLT_CLASSES_MAX: inside the table
    return ((T[cls >> 5] >> (cls & 31u)) & 1u) != 0u;
  }
  __device__ __forceinline__ void xyz(const rec &q, float &x, float &y, float &z) const {
    R.xyz(cc_xyz{q.x, q.y, q.z}, x, y, z);
    x = keep(q.w) ? x : __int_as_float(0x7FC00000);  // cc_point_cell rejects a NaN x: the record owns nothing and counts nowhere
  }
  // (an owner is a kept record: testing it again changes nothing, and the one function keeps the bits the sweep saw)
  __device__ __forceinline__ float2 owner_xy(int j) const {
    float x, y, z;
    xyz(load(j), x, y, z);
    return make_float2(x, y);
  }
};

// ---- typed coordinate STREAMS (cc_ingest_coords, include/cont2_amd_coords.h): x, y and z are three streams of one element type --
// f32, f64 or i32 -- and one stride, which may lie inside one record array (in any order, with anything between them) or in three
// arrays.  A coordinate becomes the f32 everything downstream sees by the header's three steps, each rounded once:
//     X = (double)v [* scale[k] for i32];   D = X - origin[scan][k];   p = (float)D
// The f64 subtraction in front of the narrowing is what a georeferenced cloud needs (an f32 resolves 0.5 m at a UTM northing), and
// the f64 rate to do it per point is there in a sweep bound by HBM and LDS.  The library is built with -ffp-contract=off: the product
// and the difference are never fused.  load() requests the three RAW elements together (3 x 8 bytes for f64, 3 x 4 otherwise), none
// under a branch, and the record carries them raw; the conversion is xyz()'s, which runs when the sweep resolves the chunk, a chunk
// after the loads were issued.  The origin and the scales are workgroup-uniform: scalars.  The per-scan matrix is cc_ld_rec's.
// The stride is a run-time value: 4 sweep instances and 1 merge instance per type.
enum { CC_K1_COORD_F32 = 0, CC_K1_COORD_F64 = 1, CC_K1_COORD_I32 = 2 };  // = CC_COORD_* (checked where both are seen)
struct cc_k1_coords {
  const char *x, *y, *z;  // the first point's elements
  int stride;
  double scale[3];        // I32 (1.0 otherwise: not read)
  const double *origin;   // [n_scans][3], or nullptr: 0.0
  const float *tf;        // [n_scans][12] or nullptr
};
template <int TYPE>
struct cc_coord_elem {
  typedef float t;
};
template <>
struct cc_coord_elem<CC_K1_COORD_F64> {
  typedef double t;
};
template <>
struct cc_coord_elem<CC_K1_COORD_I32> {
  typedef int t;
};
__device__ __forceinline__ double cc_uniform_d(double v) {
#ifndef CC_EMU
  return __hiloint2double(cc_uniform_i(__double2hiint(v)), cc_uniform_i(__double2loint(v)));
#else
  return v;
#endif
}

template <int TYPE>
struct cc_ld_coord {
  typedef typename cc_coord_elem<TYPE>::t elem;
  struct rec {
    elem x, y, z;
  };
  cc_ld_rec<0> R;  // the workgroup-uniform transform alone: cc_ld_rec's, used as it is
  const char *__restrict__ X, *__restrict__ Y, *__restrict__ Z;
  unsigned stride;  // j * stride < 2^29, as for cc_ld_rec
  double s[3], o[3];
  __device__ __forceinline__ cc_ld_coord(const cc_k1_coords &C, int scan) : R(nullptr, 0, C.tf, scan), X(C.x), Y(C.y), Z(C.z), stride((unsigned)C.stride) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      s[k] = C.scale[k];
      o[k] = C.origin ? cc_uniform_d(C.origin[(size_t)scan * 3 + k]) : 0.0;
    }
  }
  __device__ __forceinline__ void advance(long long n) {
    const long long b = n * (long long)stride;
    X += b;
    Y += b;
    Z += b;
  }
  __device__ __forceinline__ rec load(int j) const {
    const unsigned at = (unsigned)j * stride;
    rec q;
    q.x = *(const elem *)(X + at);
    q.y = *(const elem *)(Y + at);
    q.z = *(const elem *)(Z + at);
    return q;
  }
  __device__ __forceinline__ static rec zero() { return rec{(elem)0, (elem)0, (elem)0}; }
  __device__ __forceinline__ float conv(elem v, int k) const {
    double d = (double)v;                       // step 1 (exact for all three types)
    if (TYPE == CC_K1_COORD_I32) d = d * s[k];  //   ... one f64 product
    d = d - o[k];                               // step 2: one f64 subtraction
    return (float)d;                            // step 3: round to nearest even
  }
  __device__ __forceinline__ void xyz(const rec &q, float &x, float &y, float &z) const { R.xyz(cc_xyz{conv(q.x, 0), conv(q.y, 1), conv(q.z, 2)}, x, y, z); }
  __device__ __forceinline__ float2 owner_xy(int j) const {
    float x, y, z;
    xyz(load(j), x, y, z);
    return make_float2(x, y);
  }
};


// ---- point SOURCES: what a call hands the kernels, one by-value struct per family.  A source is the kernel argument and knows how
// to make its family's loader:
//   TAB_BYTES / TAB_ALIGN : the per-scan table the loader reads from LDS (0: none).  The sweep kernel has it in its dynamic LDS
//                           behind cc_k1_sweep's layout, at tab_off = that layout's bytes rounded up to TAB_ALIGN; the merge kernel
//                           in static LDS
//   tables(tab, scan)     : the scan's table to LDS (a barrier has to follow before the loader's xyz() / owner_xy() is called:
//                           cc_k1_sweep's first one, after it has cleared the grid; the merge kernel's own)
//   loader(scan, tab)     : the loader, positioned at the first point of the call's first scan
//   SEGMENTED             : the sweep is cc_k1_sweep_seg (which stages the table itself and re-seats a record loader per piece);
//                           loader() is the output pass' only.  (cc_src_rig, further down, has cc_k1_sweep_rig in the same way.)
// KITTI float4 records, no transform (cc_ingest_batch; the other entry points with the default layout and no transform)
struct cc_src_kitti {
  static constexpr int TAB_BYTES = 0, TAB_ALIGN = 1;
  static constexpr bool SEGMENTED = false;
  const float4 *pts;
  __device__ __forceinline__ void tables(char *, int) const {}
  __device__ __forceinline__ cc_ld_kitti loader(int, const char *) const { return cc_ld_kitti{pts}; }
};
// Records of another shape and / or a per-scan transform (cc_ingest_points and its siblings).  STRIDE: 12 (packed xyz), 16 (KITTI
// records with a transform, or not 16-byte aligned), 0 (run-time stride).  pts: x of the call's first point; tf: [n_scans][12] or nullptr.
template <int STRIDE>
struct cc_src_rec {
  static constexpr int TAB_BYTES = 0, TAB_ALIGN = 1;
  static constexpr bool SEGMENTED = false;
  const char *pts;
  int stride;
  const float *tf;
  __device__ __forceinline__ void tables(char *, int) const {}
  __device__ __forceinline__ cc_ld_rec<STRIDE> loader(int scan, const char *) const { return cc_ld_rec<STRIDE>(pts, stride, tf, scan); }
};
// Records with a time word, de-skewed by the scan's knots (cc_ingest_points_motion).  STRIDE: 16, 32, 0 (run-time stride).
template <int STRIDE>
struct cc_src_mot {
  static constexpr int TAB_BYTES = CC_K1_MOT_LDS_BYTES, TAB_ALIGN = 16;
  static constexpr bool SEGMENTED = false;
  const char *pts;
  int stride;
  cc_k1_motion mot;
  __device__ __forceinline__ void tables(char *tab, int scan) const { cc_k1_knot_table((float *)tab, mot, scan); }
  __device__ __forceinline__ cc_ld_rec_motion<STRIDE> loader(int scan, const char *tab) const {
    return cc_ld_rec_motion<STRIDE>(pts, stride, mot, scan, (const float *)tab);
  }
};
// Records dropped by a word of their own (cc_ingest_points_filtered).  KIND: CC_K1_FLT_CLASS (a table in LDS) / CC_K1_FLT_RANGE (none).
// pts, stride, tf: cc_src_rec<0>'s.
template <int KIND>
struct cc_src_flt {
  static constexpr int TAB_BYTES = KIND == CC_K1_FLT_CLASS ? CC_K1_FLT_LDS_BYTES : 0, TAB_ALIGN = KIND == CC_K1_FLT_CLASS ? 16 : 1;
  static constexpr bool SEGMENTED = false;
  const char *pts;
  int stride;
  const float *tf;
  cc_k1_filter flt;
  __device__ __forceinline__ void tables(char *tab, int) const {
    if (KIND == CC_K1_FLT_CLASS) cc_k1_filter_table((unsigned *)tab, flt);
  }
  __device__ __forceinline__ cc_ld_rec_flt<KIND> loader(int scan, const char *tab) const {
    return cc_ld_rec_flt<KIND>(pts, stride, tf, scan, flt, (const unsigned *)tab);
  }
};
// Typed coordinate streams (cc_ingest_coords).  TYPE: CC_K1_COORD_F32 / _F64 / _I32.  No table.
template <int TYPE>
struct cc_src_coord {
  static constexpr int TAB_BYTES = 0, TAB_ALIGN = 1;
  static constexpr bool SEGMENTED = false;
  cc_k1_coords crd;
  __device__ __forceinline__ void tables(char *, int) const {}
  __device__ __forceinline__ cc_ld_coord<TYPE> loader(int scan, const char *) const { return cc_ld_coord<TYPE>(crd, scan); }
};
// Range images (cc_ingest_ranges).  WORD: CC_K1_WORD_U16 / _U32 / _F32.  offsets: scan i's first pixel = i * n_rows * n_cols.
template <int WORD>
struct cc_src_rng {
  static constexpr int TAB_BYTES = CC_K1_RNG_LDS_BYTES, TAB_ALIGN = 16;
  static constexpr bool SEGMENTED = false;
  cc_k1_range rng;
  __device__ __forceinline__ void tables(char *tab, int scan) const { cc_k1_range_tables(tab, rng, scan); }
  __device__ __forceinline__ cc_ld_range<WORD> loader(int scan, const char *tab) const { return cc_ld_range<WORD>(rng, scan, tab); }
};
// Scans made of segments (cc_ingest_segments)
struct cc_src_seg {
  static constexpr int TAB_BYTES = CC_K1_SEG_LDS_BYTES, TAB_ALIGN = 8;
  static constexpr bool SEGMENTED = true;
  cc_k1_segs segs;
  __device__ __forceinline__ void tables(char *tab, int scan) const { cc_k1_seg_table((cc_k1_seg *)tab, segs, scan); }
  __device__ __forceinline__ cc_ld_segs loader(int scan, const char *tab) const {
    return cc_ld_segs{(const cc_k1_seg *)tab, segs.scan_seg[scan + 1] - segs.scan_seg[scan]};
  }
};

// ---- a RIG's scan (cc_ingest_rig, include/cont2_amd_rig.h): segments as in cc_ingest_segments, and every segment brings a MODE (none,
// a matrix, or its time word and a slice of the scan's knot pool) and the place of its filter word (or none).  It is cc_k1_sweep_seg's
// design carried further: the workgroup's range of Q is cut into pieces, one per segment; the loader is re-seated per piece from the
// LDS table -- base, stride, matrix or (t_begin, scale, slice), the two word offsets and the filter shift are workgroup-uniform
// scalars; a piece's last chunk prefetches the next piece's first records under no branch.  New in the loader:
//   load()  requests x, y, z, the time word and the filter word's dword TOGETHER, none under a branch.  A segment without one of the
//           words aims that load at its x (offset 0): a word it may read anyway, and xyz() never looks at it.
//   xyz()   picks the matrix from the scalars (TF) or from the knot pool in LDS (MOTION: three 16-byte reads at the per-lane address
//           knot0 + bin, the bin clamped to the SEGMENT's n_knots -- cc_ld_rec_motion's steps), then puts NaN into x of a record the
//           rule drops (cc_ld_rec_flt's step).  The mode and "filtered" are scalar branches in the sweep.
// The output pass and the merge kernel map an owner's index to its segment as cc_ld_segs does, seat the SAME loader on that segment's
// entry per lane and re-read the record and both words through the same load() and xyz(): they see the bits the sweep saw.
// ONE source, the rule's kind a run-time workgroup-uniform value (cc_ld_rec's has_tf is the precedent): the class rule costs the sweep
// one LDS read per filtered point under a scalar branch and the range rule two compares; three instances per kind would triple the
// 5 kernels for no register the whole-scan instance lacks (tests/kernel_resources.py: below the 128 VGPR of 16 waves, scratch 0).
// LDS behind cc_k1_sweep's layout: the pool (3 072 B), the class table (528 B), the segment table (CC_K1_RIG_SEG_MAX x 80 B).  At
// 150 x 150 the sweep leaves 5 504 B of the CU's 163 840: 1 904 B for the table, so 16 entries (1 280 B) fit and 32 (2 560 B) do not.
#define CC_K1_RIG_SEG_MAX 16  // = CC_RIG_SEG_MAX (include/cont2_amd_rig.h; checked where both are seen)
enum { CC_K1_RIG_NONE = 0, CC_K1_RIG_TF = 1, CC_K1_RIG_MOTION = 2 };  // = CC_RIG_*
#define CC_K1_RIG_MODE_MASK 3u
#define CC_K1_RIG_TIME_U32 4u   // flags: the time word is a u32
#define CC_K1_RIG_FILTERED 8u   // flags: the segment has a filter word
#define CC_K1_RIG_SHIFT_POS 8   // flags >> 8: class rule, the shift of THIS segment's word inside its dword (byte position and the rule's shift)
struct cc_k1_rseg {
  const char *base;  // x of the segment's first point
  unsigned stride;   // bytes between records
  int first;         // index within the scan of the segment's first point
  int n;             // points (0: the segment is skipped)
  unsigned flags;    // mode | CC_K1_RIG_TIME_U32 | CC_K1_RIG_FILTERED | shift << CC_K1_RIG_SHIFT_POS
  int t_off;         // byte offset from x of the time word (0 without one)
  int w_off;         // byte offset from x of the aligned dword that holds the filter word (0 without one)
  float m[12];       // TF: row-major 3 x 4.  MOTION: [0] t_begin (TIME_U32: the u32's bits), [1] scale, [2] the bits of knot0, [3] of n_knots
};
static_assert(sizeof(cc_k1_rseg) == 80, "cc_k1_rseg: 80 bytes, 16 of them behind the pool and the class table");
struct cc_k1_rig {
  const cc_k1_rseg *seg;  // the call's segments, scan after scan
  const int *scan_seg;    // [n_scans + 1]
  const float *knots;     // [n_scans][n_pool][12], or nullptr (no segment is in motion mode)
  int n_pool;
  int kind;               // CC_K1_FLT_CLASS / CC_K1_FLT_RANGE; -1: no rule (no segment is filtered)
  const unsigned *bits;   // CLASS: cc_k1_filter's table
  unsigned mask, n_classes;
  float lo, hi;           // RANGE
};
#define CC_K1_RIG_SEG_LDS_BYTES (CC_K1_RIG_SEG_MAX * (int)sizeof(cc_k1_rseg))
#define CC_K1_RIG_LDS_BYTES (CC_K1_MOT_LDS_BYTES + CC_K1_FLT_LDS_BYTES + CC_K1_RIG_SEG_LDS_BYTES)
static_assert(((CC_MAX_CELLS * 4 + 15) & ~15) + ((CC_MAX_CELLS + 2) / 3) * 8 + 64 + ((CC_K1_EMIT_LDS_BYTES + 15) & ~15) + CC_K1_RIG_LDS_BYTES <= 160 * 1024,
              "cc_src_rig: grid, index fields, output tables, knot pool, class table and segment table fit a CU's 160 KB of LDS");
static_assert(((CC_MAX_CELLS * 4 + 15) & ~15) + ((CC_MAX_CELLS + 2) / 3) * 8 + 64 + ((CC_K1_EMIT_LDS_BYTES + 15) & ~15) + CC_K1_RIG_LDS_BYTES + CC_K1_RIG_SEG_LDS_BYTES > 160 * 1024,
              "cc_src_rig: CC_K1_RIG_SEG_MAX is the largest power of two that fits");

struct cc_rig_rec {
  float x, y, z;
  unsigned t, w;  // the time word and the filter word's dword as they lie in the record
};
// The call's rule and where the pool and the class table lie in LDS: the same for every segment.
struct cc_rig_env {
  const float4 *K;    // LDS: [n_pool][3] rows of the scan's matrices
  const unsigned *T;  // LDS (CLASS)
  int kind;
  unsigned mask, n_classes;
  float lo, hi;
};
// The loader seated on ONE segment.  UNIFORM: the entry's values are the workgroup's (the sweep: scalars); otherwise per lane (an owner's).
struct cc_ld_rig {
  typedef cc_rig_rec rec;
  const char *B;
  unsigned stride, flags;
  int t_off, w_off;
  float m[12];
  cc_rig_env E;
  template <bool UNIFORM>
  __device__ __forceinline__ static cc_ld_rig seat(const cc_k1_rseg &g, const cc_rig_env &env, int lo) {
    cc_ld_rig P;
    P.E = env;
    if (UNIFORM) {
      P.stride = (unsigned)cc_uniform_i((int)g.stride);
      P.B = cc_uniform_ptr(g.base) + (long long)lo * (long long)P.stride;
      P.flags = (unsigned)cc_uniform_i((int)g.flags);
      P.t_off = cc_uniform_i(g.t_off);
      P.w_off = cc_uniform_i(g.w_off);
#pragma unroll
      for (int i = 0; i < 12; i++) P.m[i] = __int_as_float(cc_uniform_i(__float_as_int(g.m[i])));
    } else {
      P.stride = g.stride;
      P.B = g.base + (long long)lo * (long long)P.stride;
      P.flags = g.flags;
      P.t_off = g.t_off;
      P.w_off = g.w_off;
#pragma unroll
      for (int i = 0; i < 12; i++) P.m[i] = g.m[i];
    }
    return P;
  }
  // the coordinates and the two words are requested together, none under a branch
  __device__ __forceinline__ static rec load_at(const char *p, int t_off, int w_off) {
    cc_rig_rec q;
    cc_load3f(p, q.x, q.y, q.z);
    q.t = *(const unsigned *)(p + t_off);
    q.w = *(const unsigned *)(p + w_off);
    return q;
  }
  __device__ __forceinline__ rec load(int j) const { return load_at(B + (unsigned)j * stride, t_off, w_off); }
  __device__ __forceinline__ bool keep(unsigned w) const {
    if (E.kind == CC_K1_FLT_RANGE) {
      const float v = __int_as_float((int)w);
      return (E.lo <= v) & (v <= E.hi);  // (a NaN fails both)
    }
    unsigned cls = (w >> (flags >> CC_K1_RIG_SHIFT_POS)) & E.mask;
    cls = cls < E.n_classes ? cls : E.n_classes;  // <= CC_K1_FLT_CLASSES_MAX: inside the table
    return ((E.T[cls >> 5] >> (cls & 31u)) & 1u) != 0u;
  }
  __device__ __forceinline__ void xyz(const rec &q, float &x, float &y, float &z) const {
    const unsigned mode = flags & CC_K1_RIG_MODE_MASK;
    x = q.x;
    y = q.y;
    z = q.z;
    if (mode == CC_K1_RIG_MOTION) {  // cc_ld_rec_motion's steps, K = the segment's n_knots, the knot counted from the slice's first
      const unsigned tb_bits = (unsigned)__float_as_int(m[0]);
      const float kmax = (float)(__float_as_int(m[3]) - 1);
      float u = (flags & CC_K1_RIG_TIME_U32) ? (float)(q.t - tb_bits) * m[1] : (__int_as_float((int)q.t) - m[0]) * m[1];
      u = u > 0.f ? u : 0.f;  // (a NaN fails the compare: bin 0)
      u = u < kmax ? u : kmax;
      const int b = __float_as_int(m[2]) + (int)u;  // < knot0 + n_knots <= n_pool: inside the pool
      const float4 r0 = E.K[b * 3], r1 = E.K[b * 3 + 1], r2 = E.K[b * 3 + 2];
      x = ((r0.x * q.x + r0.y * q.y) + r0.z * q.z) + r0.w;
      y = ((r1.x * q.x + r1.y * q.y) + r1.z * q.z) + r1.w;
      z = ((r2.x * q.x + r2.y * q.y) + r2.z * q.z) + r2.w;
    } else if (mode == CC_K1_RIG_TF) {  // cc_ld_rec::xyz's operations in its order
      x = ((m[0] * q.x + m[1] * q.y) + m[2] * q.z) + m[3];
      y = ((m[4] * q.x + m[5] * q.y) + m[6] * q.z) + m[7];
      z = ((m[8] * q.x + m[9] * q.y) + m[10] * q.z) + m[11];
    }
    if (flags & CC_K1_RIG_FILTERED) x = keep(q.w) ? x : __int_as_float(0x7FC00000);  // cc_point_cell rejects a NaN x: the record owns nothing and counts nowhere
  }
};

// The scan's tables to LDS (a barrier has to follow): pool, class table, segments.  Returns the number of its segments.  T: CC_K1_RIG_LDS_BYTES.
__device__ __forceinline__ int cc_k1_rig_tables(char *T, const cc_k1_rig &R, int scan) {
  if (R.knots) {
    float *kn = (float *)T;
    const float *__restrict__ src = R.knots + (size_t)scan * (size_t)R.n_pool * 12;
    for (int i = threadIdx.x; i < R.n_pool * 12; i += blockDim.x) kn[i] = src[i];
  }
  if (R.kind == CC_K1_FLT_CLASS) {
    unsigned *bt = (unsigned *)(T + CC_K1_MOT_LDS_BYTES);
    for (int i = threadIdx.x; i < CC_K1_FLT_TAB_WORDS; i += blockDim.x) bt[i] = R.bits[i];
  }
  const int s0 = R.scan_seg[scan], n_seg = R.scan_seg[scan + 1] - s0;
  const unsigned *__restrict__ src = (const unsigned *)(R.seg + s0);
  unsigned *dst = (unsigned *)(T + CC_K1_MOT_LDS_BYTES + CC_K1_FLT_LDS_BYTES);
  for (int i = threadIdx.x; i < n_seg * (int)(sizeof(cc_k1_rseg) / 4); i += blockDim.x) dst[i] = src[i];
  return n_seg;
}
__device__ __forceinline__ cc_rig_env cc_k1_rig_env(const char *T, const cc_k1_rig &R) {
  return cc_rig_env{(const float4 *)T, (const unsigned *)(T + CC_K1_MOT_LDS_BYTES), R.kind, R.mask, R.n_classes, R.lo, R.hi};
}

// The output pass' loader: cc_ld_segs' search for the owner's segment, then the sweep's loader seated on that entry per lane.
struct cc_ld_rigs {
  const cc_k1_rseg *S;  // LDS
  int n_seg;
  cc_rig_env E;
  __device__ __forceinline__ void advance(long long) {}
  __device__ __forceinline__ float2 owner_xy(int j) const {
    int s = 0;
    for (int i = 1; i < n_seg; i++) s += j >= S[i].first ? 1 : 0;
    const cc_ld_rig P = cc_ld_rig::seat<false>(S[s], E, j - S[s].first);
    float x, y, z;
    P.xyz(P.load(0), x, y, z);
    return make_float2(x, y);
  }
};

// cc_k1_sweep_seg for a rig's scan (its comment has the pieces and the prefetch across them).  tab_off: where the tables go in smem.
template <int CC_K1_U, bool CC_K1_POW2, bool PART>
__device__ __forceinline__ void cc_k1_sweep_rig(char *smem, int tab_off, const cc_dev_cfg &cfg, const cc_k1_rig &rig, const long long *__restrict__ offsets,
                                                float *__restrict__ bev_out, float2 *__restrict__ pix_out, cc_k1_scan_out *__restrict__ scan_out,
                                                const cc_k1_part &part, const cc_k1_list_out &list_out, int want_dense) {
  const int n_cell = cfg.n_cell;
  unsigned *hmax = (unsigned *)smem;  // (cc_k1_sweep's layout)
  const int n_w3 = (n_cell + 2) / 3;
  unsigned long long *idx3 = (unsigned long long *)(smem + (((size_t)n_cell * 4 + 15) & ~(size_t)15));
  unsigned *red = (unsigned *)(idx3 + n_w3);
  char *emit_tab = (char *)(red + 4);
  unsigned *idle = (unsigned *)(emit_tab + CC_K1_EMIT_TAB_BYTES);
  char *tab = smem + tab_off;
  const cc_k1_rseg *T = (const cc_k1_rseg *)(tab + CC_K1_MOT_LDS_BYTES + CC_K1_FLT_LDS_BYTES);

  const int tid = threadIdx.x, nt = blockDim.x;
  const int unit = (int)blockIdx.x;
  const int scan = PART ? unit / CC_K1_SPLIT : unit;
  int n_pts = (int)(offsets[scan + 1] - offsets[scan]);  // of the whole scan: the segments' counts added up
  int idx_base = 0;
  if (PART) {  // the same ranges as cc_k1_sweep's
    const int per = (n_pts + CC_K1_SPLIT - 1) / CC_K1_SPLIT, pi = unit % CC_K1_SPLIT;
    idx_base = pi * per < n_pts ? pi * per : n_pts;
    n_pts = n_pts - idx_base < per ? n_pts - idx_base : per;
  }
  const int n_seg = cc_k1_rig_tables(tab, rig, scan);
  const cc_rig_env env = cc_k1_rig_env(tab, rig);
  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  for (int i = tid; i < n_cell; i += nt) hmax[i] = KEY_EMPTY;
  for (int i = tid; i < n_w3; i += nt) idx3[i] = ~0ull;
  idle[tid] = 0u;
  if (tid == 0) {
    red[0] = cc_fkey(CC_BEV_EMPTY);
    red[1] = cc_fkey(-CC_BEV_EMPTY);
    red[2] = 0;
  }
  __syncthreads();

  // the first segment from s on with points in the range: `lo` points into it, cnt of them (n_seg: none left)
  const int q0 = idx_base, q1 = idx_base + n_pts;
  auto piece = [&](int s, int &lo, int &cnt) {
    for (; s < n_seg; s++) {
      const int f = T[s].first, hi = q1 - f < T[s].n ? q1 - f : T[s].n;
      lo = q0 > f ? q0 - f : 0;
      cnt = hi - lo;
      if (cnt > 0) break;
    }
    lo = cc_uniform_i(lo);
    cnt = cc_uniform_i(cnt);
    return cc_uniform_i(s);
  };
  unsigned kmin = cc_fkey(-CC_BEV_EMPTY);
  const int chunk = CC_K1_U * nt;
  int lo = 0, cnt = 0;
  int s = piece(0, lo, cnt);
  if (s < n_seg) {
    cc_ld_rig P = cc_ld_rig::seat<true>(T[s], env, lo);
    cc_rig_rec q[CC_K1_U];
#pragma unroll
    for (int u = 0; u < CC_K1_U; u++) {
      const int j = tid + u * nt;
      q[u] = P.load(j < cnt - 1 ? j : cnt - 1);
    }
    while (s < n_seg) {
      int lo2 = 0, cnt2 = 0;
      const int s2 = piece(s + 1, lo2, cnt2);
      // what this piece's last chunk prefetches: the next piece's first records (the last piece: its own last record, dropped)
      const char *nB = P.B;
      unsigned nstride = P.stride;
      int nt_off = P.t_off, nw_off = P.w_off, nlast = cnt - 1;
      if (s2 < n_seg) {
        nstride = (unsigned)cc_uniform_i((int)T[s2].stride);
        nB = cc_uniform_ptr(T[s2].base) + (long long)lo2 * (long long)nstride;
        nt_off = cc_uniform_i(T[s2].t_off);
        nw_off = cc_uniform_i(T[s2].w_off);
        nlast = cnt2 - 1;
      }
      const int j_piece = cc_uniform_i(T[s].first) + lo;  // index within the scan of the piece's first point
      for (int base = 0; base < cnt; base += chunk) {
        int cell[CC_K1_U];
        unsigned key[CC_K1_U];
        cc_k1_cells<CC_K1_U, CC_K1_POW2>(cfg, P, q, cnt - base, cell, key, kmin, tid, nt);
        const bool more = base + chunk < cnt;
        const char *lB = more ? P.B : nB;
        const unsigned lstride = more ? P.stride : nstride;
        const int lt_off = more ? P.t_off : nt_off, lw_off = more ? P.w_off : nw_off;
        const int l0 = more ? base + chunk : 0, llast = more ? cnt - 1 : nlast;
#pragma unroll
        for (int u = 0; u < CC_K1_U; u++) {
          const int j = l0 + tid + u * nt;
          q[u] = cc_ld_rig::load_at(lB + (unsigned)(j < llast ? j : llast) * lstride, lt_off, lw_off);
        }
        cc_k1_resolve<CC_K1_U>(hmax, idx3, idle, n_w3, cell, key, j_piece + base, tid, nt);
      }
      s = s2;
      lo = lo2;
      cnt = cnt2;
      if (s < n_seg) P = cc_ld_rig::seat<true>(T[s], env, lo);
    }
  }
  cc_k1_finish<PART>(cfg, cc_ld_rigs{T, n_seg, env}, hmax, idx3, red, emit_tab, n_w3, kmin, unit, scan, n_pts, bev_out, pix_out, scan_out, part, list_out, want_dense, tid, nt);
}

// A rig's scans (cc_ingest_rig)
struct cc_src_rig {
  static constexpr int TAB_BYTES = CC_K1_RIG_LDS_BYTES, TAB_ALIGN = 16;
  static constexpr bool SEGMENTED = false;  // (the sweep is cc_k1_sweep_rig: cc_k1_is_rig below)
  cc_k1_rig rig;
  __device__ __forceinline__ void tables(char *tab, int scan) const { cc_k1_rig_tables(tab, rig, scan); }
  __device__ __forceinline__ cc_ld_rigs loader(int scan, const char *tab) const {
    return cc_ld_rigs{(const cc_k1_rseg *)(tab + CC_K1_MOT_LDS_BYTES + CC_K1_FLT_LDS_BYTES), rig.scan_seg[scan + 1] - rig.scan_seg[scan], cc_k1_rig_env(tab, rig)};
  }
};
template <typename SRC>
struct cc_k1_is_rig {
  static constexpr bool value = false;
};
template <>
struct cc_k1_is_rig<cc_src_rig> {
  static constexpr bool value = true;
};

// The sweep.  grid = n_scans (PART: n_scans * CC_K1_SPLIT), block = multiple of 64; dynamic LDS: tab_off + SRC::TAB_BYTES, tab_off =
// cc_k1_sweep's bytes (n_cell*4 + ((n_cell+2)/3)*8 + 16 + CC_K1_EMIT_LDS_BYTES, the pieces 16-byte aligned) rounded up to SRC::TAB_ALIGN.
template <int CC_K1_U, bool CC_K1_POW2, bool PART, typename SRC>
__global__ void __launch_bounds__(1024)
cc_k_rasterize(cc_dev_cfg cfg, SRC src, int tab_off, const long long *__restrict__ offsets, float *__restrict__ bev_out, float2 *__restrict__ pix_out,
               cc_k1_scan_out *__restrict__ scan_out, cc_k1_part part, cc_k1_list_out list_out, int want_dense) {
  HIP_DYNAMIC_SHARED(char, smem)
  if constexpr (cc_k1_is_rig<SRC>::value) {
    cc_k1_sweep_rig<CC_K1_U, CC_K1_POW2, PART>(smem, tab_off, cfg, src.rig, offsets, bev_out, pix_out, scan_out, part, list_out, want_dense);
  } else if constexpr (SRC::SEGMENTED) {
    cc_k1_sweep_seg<CC_K1_U, CC_K1_POW2, PART>(smem, tab_off, cfg, src.segs, offsets, bev_out, pix_out, scan_out, part, list_out, want_dense);
  } else {
    const int scan = PART ? (int)blockIdx.x / CC_K1_SPLIT : (int)blockIdx.x;
    char *tab = smem + tab_off;
    src.tables(tab, scan);  // (read after cc_k1_sweep's first barrier)
    cc_k1_sweep<CC_K1_U, CC_K1_POW2, PART>(smem, cfg, src.loader(scan, tab), offsets, bev_out, pix_out, scan_out, part, list_out, want_dense);
  }
}

// The merge of a split sweep's ranges.  grid = n_scans, block = multiple of 64.  The owners' re-reads need the scan's table too.
template <typename SRC>
__global__ void __launch_bounds__(1024)
cc_k_rasterize_merge(cc_dev_cfg cfg, SRC src, const long long *__restrict__ offsets, cc_k1_part part, float *__restrict__ bev_out, float2 *__restrict__ pix_out,
                     cc_k1_scan_out *__restrict__ scan_out, cc_k1_list_out list_out, int want_dense) {
  const int scan = (int)blockIdx.x;
  char *tab = nullptr;
  if constexpr (SRC::TAB_BYTES > 0) {
    __shared__ __attribute__((aligned(16))) char T[SRC::TAB_BYTES];
    tab = T;
    src.tables(tab, scan);
    __syncthreads();
  }
  cc_k1_merge(cfg, src.loader(scan, tab), offsets, part, bev_out, pix_out, scan_out, list_out, want_dense);
}
