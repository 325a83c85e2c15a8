// K1 for a caller-made max-height image (cc_ingest_images, include/cont2_amd_images.h): the raster-ordered list of the scan's
// active cells, cc_k1_scan_out and -- when somebody reads them -- the dense image and positions, exactly the fields and meanings
// cc_k1_emit (k_rasterize.h) writes behind a sweep.  There is no sweep here: one workgroup per image, the image read ONCE with
// 16-byte loads per lane, all of them issued before the first use, and kept in registers between the two passes.
//
//   pass 1 : sanitise (row 0 cleared, !(h > -1000) -> empty, so NaN is empty), per cell one ballot of `h > lv_grads[0]` (strict, as
//            cv::threshold is), active cells per chunk to LDS; max / min height key and the occupied count reduced per wave.
//   prefix : over the chunks, one wave.
//   pass 2 : every active cell's list entry at its raster-order place -- (row << 8 | col), level count, height, position.  The
//            position is the caller's (an 8-byte gather, for the cells that need one only), each component replaced by the cell
//            centre's when it is NaN or outside [centre - 0.5, centre + 0.5] (a select, no branch), or the centre without pos_rc.
//   dense  : (want_dense, or more than CC_LIST_CAP entries) the sanitised image -- every cell: the scratch is reused between
//            calls -- and the positions of the occupied cells; hdr.z = 1.
//
// A lane holds four consecutive cells per load, so a wave is on 256 consecutive cells at a time (a CHUNK) and takes four ballots
// per chunk, one per component: the cell 4 * lane + j of the chunk has before it the set bits of all four masks below the lane
// and the lane's own bits of the components before j.  Trip counts are block-uniform wherever a ballot is taken.
// LDS: two u16 per chunk + 5 words (< 0.5 KB); no scratch.  Roofline: HBM, 4 B x cells read + 15 B x list entries written.
#pragma once
#include "cc_dev.h"
#include "cc_group.h"
#include "k_rasterize.h"

#define CC_KI_NCHUNK ((CC_MAX_CELLS / 4 + 63) / 64)  // 256-cell chunks of the largest image: 88

// grid = n_scans, block = BLOCK.  height: the call's first image ([n_scans][n_cell] f32, 16-byte aligned, n_cell a multiple of 4);
// pos: [n_scans][n_cell] (row_f, col_f) or nullptr; min_h: [n_scans] or nullptr (the minimum over the occupied cells then).
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
cc_k_image_list(cc_dev_cfg cfg, const float4 *__restrict__ height, const float2 *__restrict__ pos, const float *__restrict__ min_h, float *__restrict__ bev_out,
                float2 *__restrict__ pix_out, cc_k1_scan_out *__restrict__ scan_out, cc_k1_list_out L, int want_dense) {
  static_assert(BLOCK % 64 == 0 && BLOCK >= 64 && BLOCK <= 1024, "cc_k_image_list: whole waves");
  constexpr int WAVES = BLOCK / 64;
  constexpr int U = (CC_KI_NCHUNK + WAVES - 1) / WAVES;  // chunks per wave: 6 at 1 024 threads (24 cells per lane in registers)
  constexpr int NTAB = U * WAVES;
  __shared__ uint16_t ccnt[NTAB], cbase[NTAB];
  __shared__ int tot[2];       // entries, slots
  __shared__ unsigned red[3];  // max key, min key, occupied cells
  const int scan = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = cc_wave_id();
  const int n_cell = cfg.n_cell, n4 = n_cell >> 2, n_col = cfg.n_col;
  const float lv0 = cfg.lv_grads[0];
  const unsigned KEY_EMPTY = cc_fkey(CC_BEV_EMPTY);
  const float4 *__restrict__ img = height + (size_t)scan * n4;

  // the image: unconditional loads from an index clamped to the last one; a lane past the end drops what it got
  float h[U][4];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int i4 = (u * WAVES + wave) * 64 + lane;
    const float4 v = img[i4 < n4 ? i4 : n4 - 1];
    h[u][0] = v.x;
    h[u][1] = v.y;
    h[u][2] = v.z;
    h[u][3] = v.w;
  }
  if (tid == 0) {
    red[0] = KEY_EMPTY;               // what K1 leaves for a cloud whose points are all rejected: max_bin_val_ starts at -VAL_ABS_INF_
    red[1] = cc_fkey(-CC_BEV_EMPTY);  // ... and min_bin_val_ at +VAL_ABS_INF_ (contour_mng.h:436)
    red[2] = 0;
    tot[1] = 0;
  }
  __syncthreads();

  // ---- pass 1 ----
  unsigned kmx = KEY_EMPTY, kmn = cc_fkey(-CC_BEV_EMPTY);
  int npix = 0;
#pragma unroll
  for (int u = 0; u < U; u++) {  // block-uniform trip count: the ballots see whole waves
    const int q = u * WAVES + wave, i4 = q * 64 + lane, c0 = i4 * 4;
    const bool valid = i4 < n4;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      // occupied: not in row 0 (makeBEV never fills it: rc.first > 0, contour_mng.h:515) and above -1000; NaN fails the compare
      const bool occ = valid & (c0 + j >= n_col) & (h[u][j] > CC_BEV_EMPTY);
      const float hs = occ ? h[u][j] : CC_BEV_EMPTY;
      h[u][j] = hs;
      const unsigned k = cc_fkey(hs);
      kmx = k > kmx ? k : kmx;
      kmn = (occ & (k < kmn)) ? k : kmn;
      npix += occ ? 1 : 0;
      cnt += __popcll(__ballot(occ & (hs > lv0)));
    }
    if (lane == 0) ccnt[q] = (uint16_t)cnt;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned a = (unsigned)__shfl_xor((int)kmx, o), b = (unsigned)__shfl_xor((int)kmn, o);
    kmx = a > kmx ? a : kmx;
    kmn = b < kmn ? b : kmn;
  }
  npix = cc_wave_sum(npix);
  if (lane == 0) {
    atomicMax(&red[0], kmx);
    atomicMin(&red[1], kmn);
    atomicAdd(&red[2], (unsigned)npix);
  }
  __syncthreads();
  if (tid < 64) {  // prefix over the chunks, one wave
    int n_act = 0;
    for (int q0 = 0; q0 < NTAB; q0 += 64) {
      const int b = q0 + lane;
      const int v1 = b < NTAB ? (int)ccnt[b] : 0;
      const int i1 = cc_wave_scan_incl(v1);
      if (b < NTAB) cbase[b] = (uint16_t)(n_act + i1 - v1);
      n_act += cc_wave_scan_total(i1);
    }
    if (lane == 0) tot[0] = n_act;
  }
  __syncthreads();

  // ---- pass 2 ----
  const bool dense = want_dense != 0 || tot[0] > CC_LIST_CAP;
  const bool has_pos = pos != nullptr;  // workgroup-uniform
  const float2 *__restrict__ P = pos + (has_pos ? (size_t)scan * n_cell : (size_t)0);
  float4 *__restrict__ bev4 = (float4 *)(bev_out + (size_t)scan * n_cell);
  float2 *__restrict__ pix = pix_out + (size_t)scan * n_cell;
  uint16_t *l_rc = L.rc + (size_t)scan * CC_LIST_CAP;
  unsigned char *l_lev = L.lev + (size_t)scan * CC_LIST_CAP;
  float *l_h = L.h + (size_t)scan * CC_LIST_CAP;
  float2 *l_pix = L.pix + (size_t)scan * CC_LIST_CAP;
  int nslot = 0;
#pragma unroll
  for (int u = 0; u < U; u++) {  // block-uniform trip count
    const int q = u * WAVES + wave, i4 = q * 64 + lane, c0 = i4 * 4;
    bool act[4], need[4];
    unsigned long long m[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool occ = h[u][j] > CC_BEV_EMPTY;  // (a lane past the end holds empties)
      act[j] = occ & (h[u][j] > lv0);
      need[j] = dense ? occ : act[j];
      m[j] = __ballot(act[j]);
    }
    // the positions of the cells that need one, requested together; every other lane asks for the image's first pair and drops it
    float2 p[4];
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = has_pos ? P[need[j] ? c0 + j : 0] : make_float2(0.f, 0.f);
    if (dense && i4 < n4) bev4[i4] = make_float4(h[u][0], h[u][1], h[u][2], h[u][3]);
    int i = (int)cbase[q] + cc_mbcnt(m[0]) + cc_mbcnt(m[1]) + cc_mbcnt(m[2]) + cc_mbcnt(m[3]);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (need[j]) {
        const int c = c0 + j, r = c / n_col, cl = c - r * n_col;
        const float rf = (float)r, cf = (float)cl;
        float2 rcf;
        rcf.x = (has_pos & (p[j].x >= rf - 0.5f) & (p[j].x <= rf + 0.5f)) ? p[j].x : rf;
        rcf.y = (has_pos & (p[j].y >= cf - 0.5f) & (p[j].y <= cf + 0.5f)) ? p[j].y : cf;
        if (dense) pix[c] = rcf;
        if (act[j]) {
          int lv = 1;
          for (int l = 1; l < CC_NLEV; l++) lv += (h[u][j] > cfg.lv_grads[l]) ? 1 : 0;
          nslot += lv;
          if (i < CC_LIST_CAP) {
            l_rc[i] = (uint16_t)((r << 8) | cl);
            l_lev[i] = (unsigned char)lv;
            l_h[i] = h[u][j];
            l_pix[i] = rcf;
          }
        }
      }
      i += act[j] ? 1 : 0;
    }
  }
  nslot = cc_wave_sum(nslot);
  if (lane == 0 && nslot) atomicAdd(&tot[1], nslot);
  __syncthreads();
  if (tid == 0) {
    L.hdr[scan] = make_int4(tot[0], tot[1], dense ? 1 : 0, 0);
    cc_k1_scan_out o;
    o.max_bin_val = cc_funkey(red[0]);
    o.min_bin_val = min_h ? min_h[scan] : cc_funkey(red[1]);
    o.n_pix = (int)red[2];
    o.pad = 0;
    scan_out[scan] = o;
  }
}
