// Query records from packed records (cc_db_*_submit_packed): the prep stage of a chunk whose query scans exist as the two
// compact records already -- rows of a caller's cc_pack_scans arrays, or the database's own rows.  Where cc_k_pack_hot and
// cc_k_gmm_prep BUILD record i of the chunk from descriptor sel[i], the kernel below COPIES it from record sel[i] of the
// source: the same bytes (both sides of the database are made by those two kernels), 59 448 B per item instead of a
// 169 048 B descriptor read and the auto-correlation sum.
//
// It also does what cc_k_pack_hot does on the side for a chunk (cc_db_api.inc): the chunk's list heads and the per-query
// pass counters are cleared, and a small chunk's epoch records come over from the lane's pinned buffer.
//
// Shape: a pure copy, so it is written for the memory system.  A hot record is 1 153 16-byte units; a record of correlation
// inputs is 41 000 B = 8 mod 16, so every odd record of an array starts 8 bytes off a 16-byte line: it is moved as 5 125 8-byte
// units, which holds for every record whatever its index.  CC_PREPP_SPLIT workgroups share an item: 2 048 lanes, each with one
// 16-byte and up to three 8-byte loads, all issued before the first store, at clamped indices (a lane past the end re-reads
// the last unit and stores nothing), so no load sits under a branch and none waits for another.  A chunk of one item is
// 32 waves; a full chunk is 8 192 workgroups over 61 MB in and 61 MB out.  The hot units go to the low parts, the third
// round of the 8-byte units to the high parts, so that the parts move 24 .. 40 B per lane each.  No LDS, no barrier.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cont2_amd.h"
#include "k_gmm.h"
#include "k_knn.h"

#define CC_PREPP_BLOCK 256
#define CC_PREPP_SPLIT 8                                         // workgroups per item
#define CC_PREPP_STRIDE (CC_PREPP_BLOCK * CC_PREPP_SPLIT)        // lanes per item
#define CC_PREPP_HOT_U ((int)(sizeof(cc_hot_desc_t) / 16))       // 1 153
#define CC_PREPP_FEAT_U ((int)(sizeof(cc_gmm_feat) / 8))         // 5 125
#define CC_PREPP_FEAT_STEPS ((CC_PREPP_FEAT_U + CC_PREPP_STRIDE - 1) / CC_PREPP_STRIDE)
static_assert(sizeof(cc_hot_desc_t) % 16 == 0, "hot records are moved in 16-byte units: every record of a 16-byte aligned array is aligned");
static_assert(sizeof(cc_gmm_feat) % 16 == 8, "the correlation inputs are moved in 8-byte units: record r of a 16-byte aligned array starts at 8 r mod 16");
static_assert(CC_PREPP_HOT_U <= CC_PREPP_STRIDE, "one 16-byte unit per lane brings an item's hot record");
static_assert(sizeof(cc_query_meta) % 16 == 0 && sizeof(cc_query_meta) / 16 <= 64, "one 16-byte unit per lane of a wave brings an epoch record");
static_assert(CC_PREPP_BLOCK >= 128, "the epoch record is the second wave's");

// grid = n * CC_PREPP_SPLIT (part p of item i is workgroup i * CC_PREPP_SPLIT + p), block = CC_PREPP_BLOCK
__global__ void __launch_bounds__(CC_PREPP_BLOCK)
cc_k_prep_packed(const cc_hot_desc_t *__restrict__ src_hot, const cc_gmm_feat *__restrict__ src_feat,
                 const int *__restrict__ sel /*[n] record i of the chunk is record sel[i] of the source*/, int n,
                 cc_hot_desc_t *__restrict__ hot, cc_gmm_feat *__restrict__ feat, int *__restrict__ z_heads /*[CC_N_HEADS]*/,
                 int n_heads, int *__restrict__ z_pass_cnt /*[n][4]*/,
                 const cc_query_meta *__restrict__ meta_src /*small query chunks: the epoch records in pinned host memory, or nullptr*/,
                 cc_query_meta *__restrict__ meta_dst) {
  const int i = blockIdx.x / CC_PREPP_SPLIT, part = blockIdx.x - i * CC_PREPP_SPLIT;
  if (i >= n) return;
  const int tid = threadIdx.x;
  const int r = sel[i];
  const uint4 *sh = (const uint4 *)(src_hot + r);
  const uint2 *sf = (const uint2 *)(src_feat + r);
  uint4 *dh = (uint4 *)(hot + i);
  uint2 *df = (uint2 *)(feat + i);
  const int uh = part * CC_PREPP_BLOCK + tid;                           // this lane's hot unit ...
  const int uf = (CC_PREPP_SPLIT - 1 - part) * CC_PREPP_BLOCK + tid;    // ... and its first unit of the correlation inputs
  // every load of the lane, before its first store
  const uint4 vh = sh[uh < CC_PREPP_HOT_U ? uh : CC_PREPP_HOT_U - 1];
  uint2 vf[CC_PREPP_FEAT_STEPS];
#pragma unroll
  for (int k = 0; k < CC_PREPP_FEAT_STEPS; k++) {
    const int u = uf + k * CC_PREPP_STRIDE;
    vf[k] = sf[u < CC_PREPP_FEAT_U ? u : CC_PREPP_FEAT_U - 1];
  }
  if (part == 0) {  // the side work of cc_k_pack_hot, by the same item's first workgroup
    if (meta_src && tid >= 64 && tid < 64 + (int)(sizeof(cc_query_meta) / 16)) ((uint4 *)(meta_dst + i))[tid - 64] = ((const uint4 *)(meta_src + i))[tid - 64];
    if (tid < 4) z_pass_cnt[i * 4 + tid] = 0;
    if (i == 0 && tid < n_heads) z_heads[tid] = 0;
  }
  if (uh < CC_PREPP_HOT_U) dh[uh] = vh;
#pragma unroll
  for (int k = 0; k < CC_PREPP_FEAT_STEPS; k++) {
    const int u = uf + k * CC_PREPP_STRIDE;
    if (u < CC_PREPP_FEAT_U) df[u] = vf[k];
  }
}
