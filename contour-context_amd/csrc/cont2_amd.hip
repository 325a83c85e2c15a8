// libcont2_amd.so -- C-ABI of the MI355X-native contour-context hot path (include/cont2_amd.h).
// Host code: device memory ownership, launches, the LayerDB bookkeeping timeline.  Kernels live in
// the k_*.h headers next to this file.  Built for gfx950 only:
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -shared -fPIC cont2_amd.hip -o libcont2_amd.so
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdlib>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/cont2_amd.h"
#include "../../include/cont2_amd_images.h"
#include "../../include/cont2_amd_filter.h"
#include "../../include/cont2_amd_coords.h"
#include "../../include/cont2_amd_rig.h"
#include "../../include/cont2_amd_paths.h"
#include "../../include/cont2_amd_cands.h"
#include "../../include/cont2_amd_matches.h"
#include "../../include/cont2_amd_lists.h"
#include "../../include/cont2_amd_keyview.h"
#include "cc_hostcfg.h"
#include "k_rasterize.h"
#include "k_image.h"
#include "k_contours.h"
#include "k_contours_list.h"
#include "k_knn.h"
#include "k_knn_list.h"
#include "k_mask.h"
#include "k_check.h"
#include "k_merge.h"
#include "k_gmm.h"
#include "k_gmm_hess.h"
#include "k_match.h"
#include "k_verify.h"
#include "k_pose.h"
#include "k_prep_packed.h"
#include "cc_hostdb.h"

#ifndef CC_INGEST_BLOCK
#define CC_INGEST_BLOCK 1024  // threads per workgroup of the per-scan ingest kernels
#endif
#ifndef CC_IMAGE_BLOCK
#define CC_IMAGE_BLOCK CC_INGEST_BLOCK  // ... and of cc_k_image_list (256 and 512 measured: DESIGN.md 3.0)
#endif

static thread_local std::string g_err;
static int set_err(int code, const char *what, hipError_t e = hipSuccess) {
  g_err = what;
  if (e != hipSuccess) {
    g_err += ": ";
    g_err += hipGetErrorString(e);
  }
  return code;
}
#define HIPCHK(call)                                          \
  do {                                                        \
    hipError_t e_ = (call);                                   \
    if (e_ != hipSuccess) return set_err(CC_EHIP, #call, e_); \
  } while (0)

struct cc_ctx {
  int device = 0;
  cc_manager_cfg_t mcfg;
  cc_dev_cfg dcfg;
  int max_batch = 0;
  // What ONE ingest launch chain works in.  Calls on the same set are ordered (ev_last: the next call waits, on the device,
  // for the previous one's last kernel when it comes in on another stream); different sets may be in flight together.  The
  // context has the set of the batched calls (`main`, max_batch scans) and, for the per-scan loop, CC_NCHAN one-scan sets
  // (`chan[i]`, made at first use): consecutive scans of the loop are ingested on alternating channels, so the ~0.25 ms one
  // scan's K1 + K2 take overlap with the next scan's instead of queueing behind them.
  struct Scratch {
    int cap = 0;  // scans
    float *d_bev = nullptr;
    float2 *d_pix = nullptr;
    cc_k1_scan_out *d_k1 = nullptr;
    cc_k1_part k1_part;  // scratch of the split rasterisation (calls of <= CC_K1_SPLIT_MAX_SCANS scans), allocated at first use
    cc_k2_scratch *d_scr = nullptr;
    long long *d_offsets = nullptr;
    float *d_tf = nullptr;  // [cap][12]: the per-scan transforms of a call that brings some (cc_ingest_points)
    float *d_mot = nullptr;  // a chunk's [nb][2] times, then its [nb][K][12] knots (cc_ingest_points_motion); allocated at first use
    unsigned *d_flt = nullptr;  // a call's class table (cc_ingest_points_filtered): CC_K1_FLT_TAB_WORDS words; allocated at first use
    double *d_org = nullptr;  // a chunk's [nb][3] origins (cc_ingest_coords); allocated at first use
    char *d_rig = nullptr;  // a chunk's tables of a rig call (cc_ingest_rig): scan_seg, the cc_k1_rseg entries, the knot pools, the class table; allocated at first use
    char *d_seg = nullptr;  // a chunk's segment table (cc_ingest_segments): int scan_seg[cap + 1], then up to cap * CC_SEG_MAX cc_k1_seg; allocated at first use
    // the slow path of K2 (scans with more than CC_MAXC components on a level): queue filled by the fast launch, a few
    // workgroups with CC_NC_BIG-sized tables in global memory
    int n_bigslots = 0;
    cc_k2_big_queue *d_bigq = nullptr;
    cc_k2_big_queue *d_midq = nullptr;  // scans the list kernel hands to the original body (cc_k_contours_mid)
    int *h_mid_seen = nullptr;          // pinned: the queue length the last cc_k_contours_mid launch found (-1: none has run yet)
    cc_k1_list_out list;                // K1 -> K2: the scans' active cells as raster-ordered lists (k_rasterize.h)
    cc_k2_big_slot *d_bigslots = nullptr;
    hipEvent_t ev_last = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_last = false;
  };
  static const int N_BIG_SLOTS = 8;
  Scratch main;
  // pinned staging ring for the per-chunk point offsets (and, behind them, the chunk's 12 floats per scan of a call with
  // transforms, then the 3 doubles per scan of a call with origins): a slot is reused only after the copies that read it have finished
  static const int NSLOT = 4;
  long long *h_off[NSLOT] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t off_ev[NSLOT] = {nullptr, nullptr, nullptr, nullptr};
  bool off_busy[NSLOT] = {false, false, false, false};
  int off_next = 0;
  int off_cap = 0;  // scans a slot holds
  char *h_seg[NSLOT] = {nullptr, nullptr, nullptr, nullptr};  // the same ring's slots for a chunk's segment table (cc_ingest_segments), grown to what a chunk needs
  size_t h_seg_cap[NSLOT] = {0, 0, 0, 0};
  // the per-scan loop (cc_scan_*): own stream, pinned + device point staging, a pool of device descriptor slots
  hipStream_t s_loop = nullptr;       // per-scan loop: descriptor fetches, cc_db_query_scan / cc_db_add_scan
  // per-scan loop: cc_scan_ingest (copy of the points, K1, K2) goes to the next of CC_NCHAN channels -- own stream, device point
  // buffer, one-scan scratch set; a scan's `ready` event is recorded on its channel's stream
  static const int NCHAN = 2;
  struct Channel {
    hipStream_t s = nullptr;
    float *d_pts = nullptr;
    int64_t d_pts_cap = 0;             // points d_pts holds (one staging buffer's worth; CC_SCAN_BATCH_MAX of them once a batch came by)
    cc_scan_desc_t *d_desc_tmp = nullptr;  // [CC_SCAN_BATCH_MAX] where a batch's descriptors are written before they go to their slots
    float *d_bev_copy = nullptr;  // the max-height image of a scan that asked for it (want_bev), until its copy to the host has passed
    Scratch scr;
  };
  Channel chan[NCHAN];
  int chan_next = 0;
  std::mutex slot_mu;                 // slot_free: cc_scan_ingest may run on a helper thread next to cc_scan_offload / cc_scan_release
  // per-scan loop: two pinned staging buffers (the caller may fill the second one -- e.g. read the next scan's file from
  // another thread -- while the first one's scan is in flight), one device point buffer (the stream orders its reuse)
  // Slots 0 and 1 are the caller's to name (cc_stage_points_slot), slot 2 is cc_stage_points' own -- a thread that stages
  // without naming a slot (ContourManager::makeBEV) never gets a buffer a read-ahead helper writes.
  // Round 5: 2 * CC_SCAN_BATCH_MAX caller slots (a read-ahead thread fills one batch of files while the batch before it is on
  // its way: cc_scan_ingest_batch), each allocated when it is first asked for; the last slot is cc_stage_points' own.
  static const int NPTS = 2 * CC_SCAN_BATCH_MAX + 1;
  static const int OWN_SLOT = NPTS - 1;
  float *h_pts[NPTS] = {};
  hipEvent_t pts_ev[NPTS] = {};  // recorded behind a slot's H2D copy: the slot may be rewritten once it has passed
  bool pts_busy[NPTS] = {};
  // Ingest state (the staging slots, d_pts, the offsets ring, the K1/K2 scratch, ev_last) is shared by every call of the
  // context: ing_mu is held inside cc_ingest_batch / cc_stage_points* / cc_scan_ingest.  A slot handed out by
  // cc_stage_points* belongs to the calling thread until that thread's cc_scan_ingest has queued its copy (or the thread
  // stages the slot again); another thread asking for it WAITS (pts_cv) instead of being handed memory that is being filled.
  std::recursive_mutex ing_mu;
  std::condition_variable_any pts_cv;
  bool pts_handed[NPTS] = {};
  std::thread::id pts_owner[NPTS];
  int64_t pts_cap = 0;  // points
  std::vector<cc_scan_desc_t *> slot_free, slot_blocks;
  std::vector<int> slot_block_n;  // slots per block
  size_t lds1 = 0, lds2 = 0;
  // optional per-kernel timing (cc_profile_*)
  bool prof = false;
  std::vector<hipEvent_t> ev;  // triplets (before K1, between, after K2)
  size_t ev_used = 0;
  double ms_acc[2] = {0, 0};
  int launches = 0;
};

static int prof_flush(cc_ctx *c) {
  for (size_t i = 0; i + 3 <= c->ev_used; i += 3) {
    float a = 0, b = 0;
    if (hipEventSynchronize(c->ev[i + 2]) != hipSuccess) return CC_EHIP;
    hipEventElapsedTime(&a, c->ev[i], c->ev[i + 1]);
    hipEventElapsedTime(&b, c->ev[i + 1], c->ev[i + 2]);
    c->ms_acc[0] += a;
    c->ms_acc[1] += b;
    c->launches++;
  }
  c->ev_used = 0;
  return CC_OK;
}


static int scratch_alloc(cc_ctx *c, cc_ctx::Scratch &S, int cap, int n_bigslots) {
  const size_t nc = (size_t)c->dcfg.n_cell;
  S.cap = cap;
  HIPCHK(hipMalloc(&S.d_bev, sizeof(float) * nc * cap));
  HIPCHK(hipMalloc(&S.d_pix, sizeof(float2) * nc * cap));
  HIPCHK(hipMalloc(&S.d_k1, sizeof(cc_k1_scan_out) * cap));
  HIPCHK(hipMalloc(&S.d_scr, sizeof(cc_k2_scratch) * cap));
  HIPCHK(hipMalloc(&S.d_offsets, sizeof(long long) * (cap + 1)));
  HIPCHK(hipMalloc(&S.d_tf, sizeof(float) * 12 * (size_t)cap));
  HIPCHK(hipMalloc(&S.d_bigq, sizeof(cc_k2_big_queue) + sizeof(int) * (size_t)cap));
  HIPCHK(hipMemset(S.d_bigq, 0, sizeof(cc_k2_big_queue)));  // the slow launch leaves it empty again
  HIPCHK(hipMalloc(&S.d_midq, sizeof(cc_k2_big_queue) + sizeof(int) * (size_t)cap));
  HIPCHK(hipMalloc(&S.list.hdr, sizeof(int4) * (size_t)cap));
  HIPCHK(hipMalloc(&S.list.rc, sizeof(uint16_t) * (size_t)CC_LIST_CAP * cap));
  HIPCHK(hipMalloc(&S.list.lev, (size_t)CC_LIST_CAP * cap));
  HIPCHK(hipMalloc(&S.list.h, sizeof(float) * (size_t)CC_LIST_CAP * cap));
  HIPCHK(hipMalloc(&S.list.pix, sizeof(float2) * (size_t)CC_LIST_CAP * cap));
  HIPCHK(hipMemset(S.d_midq, 0, sizeof(cc_k2_big_queue)));
  HIPCHK(hipHostMalloc((void **)&S.h_mid_seen, sizeof(int), hipHostMallocDefault));
  *S.h_mid_seen = -1;
  S.n_bigslots = n_bigslots < cap ? n_bigslots : cap;
  HIPCHK(hipMalloc(&S.d_bigslots, sizeof(cc_k2_big_slot) * S.n_bigslots));
  HIPCHK(hipEventCreateWithFlags(&S.ev_last, hipEventDisableTiming));
  return CC_OK;
}
static void scratch_free(cc_ctx::Scratch &S) {
  hipFree(S.d_bev);
  hipFree(S.d_pix);
  hipFree(S.d_k1);
  hipFree(S.k1_part.key);
  hipFree(S.k1_part.idx);
  hipFree(S.k1_part.red);
  hipFree(S.d_scr);
  hipFree(S.d_offsets);
  hipFree(S.d_tf);
  hipFree(S.d_seg);
  hipFree(S.d_rig);
  hipFree(S.d_mot);
  hipFree(S.d_flt);
  hipFree(S.d_org);
  hipFree(S.d_bigq);
  hipFree(S.d_midq);
  if (S.h_mid_seen) hipHostFree(S.h_mid_seen);
  hipFree(S.list.hdr);
  hipFree(S.list.rc);
  hipFree(S.list.lev);
  hipFree(S.list.h);
  hipFree(S.list.pix);
  hipFree(S.d_bigslots);
  if (S.ev_last) hipEventDestroy(S.ev_last);
  S = cc_ctx::Scratch();
}

// ---- K1's launches.  The sources (k_rasterize.h) the library instantiates the kernels for, ONE list: cc_create sets every instance's
// dynamic-LDS limit from it, and k1_launch refuses (at compile time) a source that is not on it.
template <typename... SRC>
struct k1_list {};
typedef k1_list<cc_src_kitti, cc_src_rec<12>, cc_src_rec<16>, cc_src_rec<0>, cc_src_mot<16>, cc_src_mot<32>, cc_src_mot<0>, cc_src_seg, cc_src_rng<CC_K1_WORD_U16>,
                cc_src_rng<CC_K1_WORD_U32>, cc_src_rng<CC_K1_WORD_F32>, cc_src_flt<CC_K1_FLT_CLASS>, cc_src_flt<CC_K1_FLT_RANGE>, cc_src_coord<CC_K1_COORD_F32>,
                cc_src_coord<CC_K1_COORD_F64>, cc_src_coord<CC_K1_COORD_I32>, cc_src_rig>
    k1_sources;
template <typename S, typename... SRC>
static constexpr bool k1_listed(k1_list<SRC...>) {
  return (std::is_same<S, SRC>::value || ...);
}
// Where SRC's table goes in the sweep's dynamic LDS (behind the layout of the instances without one), and the bytes of the whole.
template <typename SRC>
static size_t k1_tab_off(const cc_ctx *c) {
  return (c->lds1 + (size_t)(SRC::TAB_ALIGN - 1)) & ~(size_t)(SRC::TAB_ALIGN - 1);
}
template <typename SRC>
static size_t k1_lds(const cc_ctx *c) {
  return k1_tab_off<SRC>(c) + (size_t)SRC::TAB_BYTES;
}
template <typename SRC>
static int k1_attr(cc_ctx *c) {
  const int lds = (int)k1_lds<SRC>(c);
  HIPCHK(hipFuncSetAttribute((const void *)cc_k_rasterize<CC_K1_U_DEFAULT, false, false, SRC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIPCHK(hipFuncSetAttribute((const void *)cc_k_rasterize<CC_K1_U_DEFAULT, true, false, SRC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIPCHK(hipFuncSetAttribute((const void *)cc_k_rasterize<CC_K1_U_DEFAULT, false, true, SRC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIPCHK(hipFuncSetAttribute((const void *)cc_k_rasterize<CC_K1_U_DEFAULT, true, true, SRC>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  return CC_OK;
}
template <typename... SRC>
static int k1_attr_all(cc_ctx *c, k1_list<SRC...>) {
  int rc = CC_OK;
  ((rc = rc == CC_OK ? k1_attr<SRC>(c) : rc), ...);
  return rc;
}
// K1 for the nb scans whose offsets are in S.d_offsets.  A handful of scans (the per-scan loop brings one): CC_K1_SPLIT workgroups per
// scan sweep a range of its points each, a second small kernel combines the ranges (first range wins ties: file order).  Otherwise
// one workgroup per scan.
template <typename SRC>
static int k1_launch(cc_ctx *c, cc_ctx::Scratch &S, const SRC &src, int nb, int want_dense, hipStream_t stream) {
  static_assert(k1_listed<SRC>(k1_sources()), "k1_launch: a source cc_create does not prepare (k1_sources)");
  const size_t lds = k1_lds<SRC>(c);
  const int tab_off = (int)k1_tab_off<SRC>(c);
  const long long *off = (const long long *)S.d_offsets;
  if (nb <= CC_K1_SPLIT_MAX_SCANS) {
    if (!S.k1_part.key) {
      const size_t np = (size_t)CC_K1_SPLIT_MAX_SCANS * CC_K1_SPLIT, nc = (size_t)c->dcfg.n_cell;
      HIPCHK(hipMalloc(&S.k1_part.key, sizeof(unsigned) * np * nc));
      HIPCHK(hipMalloc(&S.k1_part.idx, sizeof(int) * np * nc));
      HIPCHK(hipMalloc(&S.k1_part.red, sizeof(unsigned) * np * 2));
    }
    if (c->dcfg.reso_pow2)
      hipLaunchKernelGGL((cc_k_rasterize<CC_K1_U_DEFAULT, true, true, SRC>), dim3(nb * CC_K1_SPLIT), dim3(CC_INGEST_BLOCK), lds, stream, c->dcfg, src, tab_off, off,
                         S.d_bev, S.d_pix, S.d_k1, S.k1_part, S.list, want_dense);
    else
      hipLaunchKernelGGL((cc_k_rasterize<CC_K1_U_DEFAULT, false, true, SRC>), dim3(nb * CC_K1_SPLIT), dim3(CC_INGEST_BLOCK), lds, stream, c->dcfg, src, tab_off, off,
                         S.d_bev, S.d_pix, S.d_k1, S.k1_part, S.list, want_dense);
    hipLaunchKernelGGL((cc_k_rasterize_merge<SRC>), dim3(nb), dim3(1024), 0, stream, c->dcfg, src, off, S.k1_part, S.d_bev, S.d_pix, S.d_k1, S.list, want_dense);
  } else if (c->dcfg.reso_pow2)
    hipLaunchKernelGGL((cc_k_rasterize<CC_K1_U_DEFAULT, true, false, SRC>), dim3(nb), dim3(CC_INGEST_BLOCK), lds, stream, c->dcfg, src, tab_off, off, S.d_bev,
                       S.d_pix, S.d_k1, cc_k1_part(), S.list, want_dense);
  else
    hipLaunchKernelGGL((cc_k_rasterize<CC_K1_U_DEFAULT, false, false, SRC>), dim3(nb), dim3(CC_INGEST_BLOCK), lds, stream, c->dcfg, src, tab_off, off, S.d_bev,
                       S.d_pix, S.d_k1, cc_k1_part(), S.list, want_dense);
  return CC_OK;
}

extern "C" {

const char *cc_last_error(void) { return g_err.c_str(); }
int cc_version(void) { return 100; }

void cc_default_manager_cfg(cc_manager_cfg_t *c) {
  const float g[CC_NLEV] = {1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f};
  for (int i = 0; i < CC_NLEV; i++) c->lv_grads[i] = g[i];
  c->reso_row = c->reso_col = 1.0f;
  c->n_row = c->n_col = 150;
  c->lidar_height = 2.0f;
  c->blind_sq = 9.0f;
  c->min_cont_key_cnt = 9;
  c->min_cont_cell_cnt = 3;
  c->piv_firsts = 6;
  c->dist_firsts = 10;
  c->roi_radius = 10.0f;
  c->min_cell_cov = 4;
  c->point_sigma = 1.0f;
  c->com_bias_thres = 0.5f;
}
void cc_default_db_cfg(cc_db_cfg_t *d) {
  d->nnk = 50;
  d->max_fine_opt = 10;
  d->n_q_levels = 3;
  d->q_levels[0] = 1;
  d->q_levels[1] = 2;
  d->q_levels[2] = 3;
  d->cont_sim.ta_cell_cnt = 6.0f;
  d->cont_sim.tp_cell_cnt = 0.2f;
  d->cont_sim.tp_eigval = 0.2f;
  d->cont_sim.ta_h_bar = 0.3f;
  d->cont_sim.ta_rcom = 0.4f;
  d->cont_sim.tp_rcom = 0.25f;
  d->max_elapse = 25.0;
  d->min_elapse = 15.0;
}
void cc_default_thresholds(cc_score_t *lb, cc_score_t *ub) {
  lb->i_ovlp_sum = lb->i_ovlp_max_one = lb->i_in_ang_rng = lb->i_indiv_sim = 3;
  lb->i_orie_sim = 4;
  lb->correlation = 0.3f;
  lb->area_perc = 0.03f;
  lb->neg_est_dist = -5.01f;
  ub->i_ovlp_sum = ub->i_ovlp_max_one = ub->i_in_ang_rng = ub->i_indiv_sim = ub->i_orie_sim = 6;
  ub->correlation = 0.75f;
  ub->area_perc = 0.15f;
  ub->neg_est_dist = -5.0f;
}

// ---- start of the device runtime, and a per-device pool of streams ----
// Measured on MI355X / ROCm 7.2: the first HIP call of a process takes ~54 ms, loading the code object ~5-20 ms, and
// hipStreamCreateWithFlags 16 / 8.5 / 8.5 / 8.5 ms for the first four streams of a process and 3.4 ms for every further one
// (profiles/r5/stream_probe.cpp) -- a per-scan driver's context + database use 4-7 streams.  cc_runtime_init pays all of that
// in one call a host can make when it starts (the class mirror: the ContourDB / evaluator constructors); contexts and
// databases take their streams from the pool and give them back when they are destroyed.
#define CC_RT_MAX_DEV 64
static std::mutex g_rt_mu;
static std::vector<hipStream_t> g_stream_pool[CC_RT_MAX_DEV];
static hipError_t stream_take(int device, hipStream_t *out) {
  if (device >= 0 && device < CC_RT_MAX_DEV) {
    std::lock_guard<std::mutex> lk(g_rt_mu);
    if (!g_stream_pool[device].empty()) {
      *out = g_stream_pool[device].back();
      g_stream_pool[device].pop_back();
      return hipSuccess;
    }
  }
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
static void stream_give(int device, hipStream_t s) {
  hipStreamSynchronize(s);
  if (device >= 0 && device < CC_RT_MAX_DEV) {
    std::lock_guard<std::mutex> lk(g_rt_mu);
    if (g_stream_pool[device].size() < 32) {
      g_stream_pool[device].push_back(s);
      return;
    }
  }
  hipStreamDestroy(s);
}
int cc_runtime_init(int device, int n_streams) {
  if (device < 0 || n_streams < 0 || n_streams > 32) return set_err(CC_EINVAL, "cc_runtime_init: bad argument (0..32 streams)");
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipFree(nullptr));
  hipFuncAttributes fa;
  HIPCHK(hipFuncGetAttributes(&fa, (const void *)cc_k_contours));  // loads the code object
  for (;;) {
    {
      std::lock_guard<std::mutex> lk(g_rt_mu);
      if (device >= CC_RT_MAX_DEV || (int)g_stream_pool[device].size() >= n_streams) break;
    }
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    std::lock_guard<std::mutex> lk(g_rt_mu);
    g_stream_pool[device].push_back(s);
  }
  return CC_OK;
}

int cc_create(int device, const cc_manager_cfg_t *cfg, int max_batch_scans, cc_ctx **out) {
  if (!cfg || !out || max_batch_scans < 1) return set_err(CC_EINVAL, "cc_create: bad argument");
  cc_dev_cfg dc;
  if (cc_make_dev_cfg(cfg, &dc) != 0)
    return set_err(CC_EINVAL, "cc_create: unsupported ContourManagerConfig (need even n_row/n_col <= 150x150, 6 increasing lv_grads_)");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0 || device < 0 || device >= ndev) return set_err(CC_EHIP, "cc_create: no such HIP device (this library has no CPU path)");
  HIPCHK(hipSetDevice(device));
  cc_ctx *c = new cc_ctx();
#define CREATE_CHK(call)                      \
  do {                                        \
    hipError_t e_ = (call);                   \
    if (e_ != hipSuccess) {                   \
      cc_destroy(c);                          \
      return set_err(CC_EHIP, #call, e_);     \
    }                                         \
  } while (0)
  c->device = device;
  c->mcfg = *cfg;
  c->dcfg = dc;
  c->max_batch = max_batch_scans;
  const size_t nc = (size_t)dc.n_cell;
  if (scratch_alloc(c, c->main, max_batch_scans, cc_ctx::N_BIG_SLOTS) != CC_OK) {
    cc_destroy(c);
    return CC_EHIP;  // (the message is set)
  }
  c->off_cap = max_batch_scans > CC_SCAN_BATCH_MAX ? max_batch_scans : CC_SCAN_BATCH_MAX;
  for (int i = 0; i < cc_ctx::NSLOT; i++) {
    CREATE_CHK(hipHostMalloc((void **)&c->h_off[i], (sizeof(long long) + sizeof(float) * 12 + sizeof(double) * 3) * (size_t)(c->off_cap + 1), hipHostMallocDefault));
    CREATE_CHK(hipEventCreateWithFlags(&c->off_ev[i], hipEventDisableTiming));
  }
  c->lds1 = ((nc * 4 + 15) & ~(size_t)15) + ((nc + 2) / 3) * 8 + 64 + ((CC_K1_EMIT_LDS_BYTES + 15) & ~15);
  c->lds2 = CC_K2_LDS_BYTES(nc);
  if (k1_attr_all(c, k1_sources()) != CC_OK) {  // every K1 instance may have its dynamic LDS
    cc_destroy(c);
    return CC_EHIP;  // (the message is set)
  }
  if (nc > (size_t)CC_MAX_CELLS) {
    cc_destroy(c);
    return set_err(CC_EINVAL, "cc_create: grid larger than 150 x 150 cells");
  }
  if (nc % 4 != 0) {  // (an even grid: cc_make_dev_cfg) image b0 of a cc_ingest_images call starts b0 * n_cell floats in, 16-byte aligned like the base
    cc_destroy(c);
    return set_err(CC_EINVAL, "cc_create: n_row * n_col must be a multiple of 4");
  }
  if (k1_lds<cc_src_rng<CC_K1_WORD_U16>>(c) > 160 * 1024) {
    cc_destroy(c);
    return set_err(CC_EINVAL, "cc_create: the range-image kernels' tables do not fit the LDS behind this grid");
  }
  CREATE_CHK(hipFuncSetAttribute((const void *)cc_k_contours, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CC_K2L_LDS_BYTES));
  CREATE_CHK(hipFuncSetAttribute((const void *)cc_k_contours_mid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds2));
  CREATE_CHK(hipFuncSetAttribute((const void *)cc_k_contours_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds2));
#undef CREATE_CHK
  *out = c;
  return CC_OK;
}

int cc_profile_enable(cc_ctx *c, int on) {
  if (!c) return set_err(CC_EINVAL, "cc_profile_enable: bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (on && c->ev.empty()) {
    c->ev.resize(3 * 64);
    for (auto &e : c->ev) HIPCHK(hipEventCreate(&e));
  }
  c->prof = on != 0;
  return CC_OK;
}
int cc_profile_read(cc_ctx *c, double ms_out[2], int *n_launches) {
  if (!c || !ms_out) return set_err(CC_EINVAL, "cc_profile_read: bad argument");
  HIPCHK(hipSetDevice(c->device));
  if (prof_flush(c) != CC_OK) return set_err(CC_EHIP, "cc_profile_read: event sync failed");
  ms_out[0] = c->ms_acc[0];
  ms_out[1] = c->ms_acc[1];
  if (n_launches) *n_launches = c->launches;
  c->ms_acc[0] = c->ms_acc[1] = 0;
  c->launches = 0;
  return CC_OK;
}

int cc_ingest_path_counts(cc_ctx *c, int32_t out[6]) {
  if (!c || !out) return set_err(CC_EINVAL, "cc_ingest_path_counts: bad argument");
  std::lock_guard<std::recursive_mutex> ing_lk(c->ing_mu);  // no ingest call queues work on a lane while it is read
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < 6; i++) out[i] = 0;
  cc_ctx::Scratch *lanes[1 + cc_ctx::NCHAN] = {&c->main};
  for (int i = 0; i < cc_ctx::NCHAN; i++) lanes[1 + i] = &c->chan[i].scr;
  for (cc_ctx::Scratch *S : lanes) {
    if (S->cap == 0) continue;  // (a channel of the per-scan loop that no scan has come by)
    if (S->has_last) HIPCHK(hipEventSynchronize(S->ev_last));
    cc_k2_big_queue q;  // (the header: the scan indices behind it stay where they are)
    HIPCHK(hipMemcpy(&q, S->d_midq, sizeof(q), hipMemcpyDeviceToHost));
    out[0] += q.total;
    for (int k = 0; k < 4; k++) out[1 + k] += q.why[k];
    HIPCHK(hipMemcpy(&q, S->d_bigq, sizeof(q), hipMemcpyDeviceToHost));
    out[5] += q.total;
  }
  return CC_OK;
}

int cc_destroy(cc_ctx *c) {
  if (!c) return CC_OK;
  hipSetDevice(c->device);
  for (auto &e : c->ev) hipEventDestroy(e);
  for (auto &ch : c->chan) {
    if (ch.s) {
      stream_give(c->device, ch.s);
    }
    hipFree(ch.d_pts);
    hipFree(ch.d_desc_tmp);
    hipFree(ch.d_bev_copy);
    scratch_free(ch.scr);
  }
  scratch_free(c->main);
  for (int i = 0; i < cc_ctx::NSLOT; i++) {
    if (c->h_off[i]) hipHostFree(c->h_off[i]);
    if (c->h_seg[i]) hipHostFree(c->h_seg[i]);
    if (c->off_ev[i]) hipEventDestroy(c->off_ev[i]);
  }
  if (c->s_loop) {
    stream_give(c->device, c->s_loop);
  }
  for (int i = 0; i < cc_ctx::NPTS; i++) {
    if (c->h_pts[i]) hipHostFree(c->h_pts[i]);
    if (c->pts_ev[i]) hipEventDestroy(c->pts_ev[i]);
  }
  for (auto *b : c->slot_blocks) hipFree(b);
  delete c;
  return CC_OK;
}

__global__ void cc_k_fill_f32(float *p, float v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// The layout a call works with: the caller's, or {16, 0}; CC_EINVAL (nothing queued, no state touched) for one the loaders do not take.
// base: the DEVICE pointer the kernels will read (4-byte aligned), or nullptr where the records are copied to device memory first.
static int point_layout(const cc_point_layout_t *layout, const void *base, const char *who, cc_point_layout_t *out) {
  cc_point_layout_t l;
  l.stride_bytes = 16;
  l.xyz_offset = 0;
  if (layout) l = *layout;
  const char *why = nullptr;
  if (l.stride_bytes % 4 != 0 || l.xyz_offset % 4 != 0) why = "stride_bytes and xyz_offset must be multiples of 4";
  else if (l.xyz_offset < 0 || l.stride_bytes < 12 || l.xyz_offset > l.stride_bytes - 12) why = "xyz_offset + 12 must not exceed stride_bytes";
  else if (l.stride_bytes > CC_POINT_STRIDE_MAX) why = "stride_bytes above CC_POINT_STRIDE_MAX";
  else if (((uintptr_t)base & 3u) != 0) why = "the points must be 4-byte aligned";
  if (why) return set_err(CC_EINVAL, (std::string(who) + ": " + why).c_str());
  *out = l;
  return CC_OK;
}
static const cc_point_layout_t CC_LAYOUT_KITTI = {16, 0};
// an error text that names the entry point the caller called (the old entry points are thin calls of the new ones' bodies)
#define CC_WHO(text) (std::string(who) + text).c_str()

// What a call's scans are made of, as ingest_on and scan_ingest_points take it: the arguments of one of the kinds of entry points, as
// the caller gave them until k1_check has passed them.  ingest_on reads DEVICE addresses; the per-scan and the *_host calls are handed
// the caller's host addresses and put the device ones in (k1_rebase) before they pass it on.  A checked SEGMENTS source points into
// its own tables: it is handed on by reference, never copied.
struct k1_source {
  enum kind_t { POINTS, MOTION, RANGES, SEGMENTS, IMAGES, FILTERED, COORDS, RIG } kind;
  const void *points = nullptr;              // POINTS, MOTION: the records; RANGES: the range words (a "point" is a pixel); IMAGES: the heights (a "point" is a cell)
  cc_point_layout_t lay = {16, 0};           // POINTS, MOTION, FILTERED (the caller's, or {16, 0})
  const float *h_tf = nullptr;               // POINTS, FILTERED, COORDS: [n_scans][12] or nullptr
  cc_point_motion_t mot = {};                // MOTION, with
  const float *h_time = nullptr;             //   [n_scans][2]
  const float *h_knots = nullptr;            // MOTION, RANGES: [n_scans][K][12] (RANGES: nullptr iff K == 0)
  const struct cc_range_sensor *sensor = nullptr;  // RANGES; the scans' offsets are the pixels' (i * H * W)
  cc_k1_seg *segs = nullptr;                 // SEGMENTS (k1_check: seg_tab's entries): one entry per segment, `base` the address of its first x;
  const int32_t *scan_segs = nullptr;        //   [n_scans + 1]: the caller's, and once checked relative to segs[0] (seg_scan)
  const cc_point_segment_t *h_segs = nullptr;  //   the caller's entries, and once checked those of the same segments (what the host calls copy from)
  const float *pos_rc = nullptr;             // IMAGES: [n_scans][n_cell][2] or nullptr (the cell centres); the scans' offsets are the cells' (i * n_cell)
  const float *h_min = nullptr;              // IMAGES: [n_scans] or nullptr (the minimum over the occupied cells)
  cc_point_filter_t flt = {};                // FILTERED; the records, layout and h_tf are POINTS'
  cc_coord_src_t crd = {};                   // COORDS: the three streams of the call's point 0, stride, type, scales
  const double *h_origin = nullptr;          //   [n_scans][3] or nullptr
  bool missing = false;                      // MOTION, FILTERED, COORDS: the caller's struct was NULL (k1_check refuses it in its place)
  const cc_rig_segment_t *h_rsegs = nullptr;  // RIG: the caller's entries (once checked: from the call's first segment on); scan_segs, seg_scan, own_off as SEGMENTS';
  int n_pool = 0;                            //   h_knots: [n_scans][n_pool][12] or nullptr; flt: the rule (has_flt: the caller brought one)
  bool has_flt = false;
  std::vector<cc_k1_rseg> rig_tab;           //   rig_check's table
  std::vector<cc_k1_seg> seg_tab;            // SEGMENTS: segs_check's table,
  std::vector<int32_t> seg_scan;             //   the scans' first segments in it,
  std::vector<int64_t> own_off;              //   and the scans' point totals as offsets; RANGES, IMAGES: the pixels' / cells' offsets (k1_check)
};
static k1_source k1_points(const void *points, const cc_point_layout_t *layout, const float *h_tf) {
  k1_source s = {k1_source::POINTS, points, layout ? *layout : CC_LAYOUT_KITTI, h_tf};
  return s;
}
static k1_source k1_motion(const void *points, const cc_point_layout_t *layout, const cc_point_motion_t *mot, const float *h_time, const float *h_knots) {
  k1_source s = {k1_source::MOTION, points, layout ? *layout : CC_LAYOUT_KITTI, nullptr, mot ? *mot : cc_point_motion_t(), h_time, h_knots};
  s.missing = !mot;
  return s;
}
static k1_source k1_ranges(const struct cc_range_sensor *sensor, const void *words, const float *h_knots) {
  k1_source s = {k1_source::RANGES, words, {16, 0}, nullptr, {}, nullptr, h_knots, sensor};
  return s;
}
static k1_source k1_segments(const cc_point_segment_t *h_segs, const int32_t *h_scan_segs) {
  k1_source s = {k1_source::SEGMENTS, nullptr, {16, 0}, nullptr, {}, nullptr, nullptr, nullptr, nullptr, h_scan_segs, h_segs};
  return s;
}
static k1_source k1_images(const float *height, const float *pos_rc, const float *h_min) {
  k1_source s = {k1_source::IMAGES, height};
  s.pos_rc = pos_rc;
  s.h_min = h_min;
  return s;
}
static k1_source k1_filtered(const void *points, const cc_point_layout_t *layout, const float *h_tf, const cc_point_filter_t *flt) {
  k1_source s = {k1_source::FILTERED, points, layout ? *layout : CC_LAYOUT_KITTI, h_tf};
  if (flt) s.flt = *flt;
  s.missing = !flt;
  return s;
}
static k1_source k1_rig(const cc_rig_segment_t *h_segs, const int32_t *h_scan_segs, const float *h_knots, int n_pool, const cc_point_filter_t *flt) {
  k1_source s = {k1_source::RIG};
  s.h_rsegs = h_segs;
  s.scan_segs = h_scan_segs;
  s.h_knots = h_knots;
  s.n_pool = h_knots ? n_pool : 0;
  if (flt) s.flt = *flt;
  s.has_flt = flt != nullptr;
  return s;
}
static k1_source k1_coords(const cc_coord_src_t *crd, const double *h_origin, const float *h_tf) {
  k1_source s = {k1_source::COORDS, crd ? crd->x : nullptr, {16, 0}, h_tf};
  if (crd) s.crd = *crd;
  s.h_origin = h_origin;
  s.missing = !crd;
  return s;
}
static_assert((int)CC_K1_COORD_F32 == (int)CC_COORD_F32 && (int)CC_K1_COORD_F64 == (int)CC_COORD_F64 && (int)CC_K1_COORD_I32 == (int)CC_COORD_I32,
              "k_rasterize.h's coordinate types are the header's");
static_assert(CC_K1_FLT_CLASSES_MAX == CC_FILTER_CLASSES_MAX, "k_rasterize.h's class table holds CC_FILTER_CLASSES_MAX classes");
static_assert(CC_K1_MOT_KNOTS_MAX == CC_MOTION_KNOTS_MAX, "k_rasterize.h's knot table holds CC_MOTION_KNOTS_MAX matrices");
// A range sensor: the checked model with its tables on the device (cc_range_sensor_create).
struct cc_range_sensor {
  cc_ctx *ctx = nullptr;  // compared, never dereferenced once the sensor exists: a sensor may outlive its context until it is destroyed
  int device = 0;
  cc_k1_range kr;   // what the kernels take (words and knots are set per chunk)
  int word_type = 0, word_bytes = 0;
  float4 *d_row = nullptr, *d_col = nullptr;
};
static_assert(CC_K1_RNG_ROWS_MAX == CC_RANGE_ROWS_MAX && CC_K1_RNG_COLS_MAX == CC_RANGE_COLS_MAX && (int)CC_K1_WORD_U16 == (int)CC_RANGE_U16 &&
                  (int)CC_K1_WORD_U32 == (int)CC_RANGE_U32 && (int)CC_K1_WORD_F32 == (int)CC_RANGE_F32,
              "k_rasterize.h's range-image limits and word types are the header's");
// Everything the header promises to check about a cc_*_ranges call that the sensor's creation has not, before anything is queued or read.
// base: the pointer whose alignment counts (device or host words).
static int ranges_check(cc_ctx *c, const cc_range_sensor *s, const void *base, const float *h_knots, const char *who) {
  const char *why = nullptr;
  if (!s || !base) why = "sensor and ranges must not be NULL";
  else if (s->ctx != c) why = "the sensor was created on another context";
  else if (((uintptr_t)base & (uintptr_t)(s->word_bytes - 1)) != 0) why = "the range words must be aligned to their size";
  else if ((h_knots == nullptr) != (s->kr.n_knots == 0)) why = "h_knots must be NULL exactly when the sensor has no knots (n_knots == 0)";
  if (why) return set_err(CC_EINVAL, (std::string(who) + ": " + why).c_str());
  return CC_OK;
}
// Everything the header promises to check about the motion arguments (`lay` has passed point_layout), before anything is queued or read.
static int motion_check(const cc_point_layout_t &lay, const cc_point_motion_t *motion, const float *h_time, const float *h_knots, int n_scans, const char *who) {
  const char *why = nullptr;
  if (!motion || !h_time || !h_knots) why = "motion, h_time and h_knots must not be NULL";
  else if (motion->time_offset < 0 || motion->time_offset % 4 != 0 || motion->time_offset > lay.stride_bytes - 4) why = "time_offset must be a multiple of 4 with time_offset + 4 <= stride_bytes";
  else if (motion->time_offset + 4 > lay.xyz_offset && motion->time_offset < lay.xyz_offset + 12) why = "the time word overlaps x, y, z";
  else if (motion->time_type != CC_TIME_F32 && motion->time_type != CC_TIME_U32) why = "time_type must be CC_TIME_F32 or CC_TIME_U32";
  else if (motion->n_knots < 1 || motion->n_knots > CC_MOTION_KNOTS_MAX) why = "n_knots must be 1 .. CC_MOTION_KNOTS_MAX";
  else
    for (int i = 0; i < n_scans; i++)
      if (!std::isfinite(h_time[(size_t)i * 2 + 1])) why = "every scale must be finite";
  if (why) return set_err(CC_EINVAL, (std::string(who) + ": " + why).c_str());
  return CC_OK;
}
// Everything the header promises to check about the filter (`lay` has passed point_layout), before anything is queued or read.
static int filter_bytes(int type) { return type == CC_FILTER_U8 ? 1 : type == CC_FILTER_U16 ? 2 : 4; }
static int filter_check(const cc_point_layout_t &lay, const cc_point_filter_t *f, const char *who) {
  const char *why = nullptr;
  if (!f) why = "filter must not be NULL";
  else if (f->type != CC_FILTER_U8 && f->type != CC_FILTER_U16 && f->type != CC_FILTER_U32 && f->type != CC_FILTER_F32) why = "type must be CC_FILTER_U8, _U16, _U32 or _F32";
  else {
    const int size = filter_bytes(f->type);
    if (f->offset < 0 || f->offset % size != 0 || f->offset > lay.stride_bytes - size) why = "offset must be a multiple of the word's size with offset + size <= stride_bytes";
    else if (f->offset + size > lay.xyz_offset && f->offset < lay.xyz_offset + 12) why = "the filter word overlaps x, y, z";
    else if (f->type == CC_FILTER_F32) {
      if (std::isnan(f->lo) || std::isnan(f->hi)) why = "lo and hi must not be NaN";
    } else if (f->shift < 0 || f->shift >= 8 * size) why = "shift must be 0 .. the word's bit width - 1";
    else if (f->n_classes < 1 || f->n_classes > CC_FILTER_CLASSES_MAX) why = "n_classes must be 1 .. CC_FILTER_CLASSES_MAX";
    else if (!f->keep_bits) why = "keep_bits must not be NULL for an integer type";
  }
  if (why) return set_err(CC_EINVAL, (std::string(who) + ": " + why).c_str());
  return CC_OK;
}
// Everything the header promises to check about a cc_*_coords call, before anything is queued or read: the source, the origins, and
// what ingest_on refuses about the scans' sizes (the host forms size their copies by them).
static int coord_bytes(int type) { return type == CC_COORD_F64 ? 8 : 4; }
static int coords_check(const cc_coord_src_t *s, const int64_t *h_offsets, int n_scans, const double *h_origin, const char *who) {
  const char *why = nullptr;
  if (!s) why = "src must not be NULL";
  else if (!s->x || !s->y || !s->z) why = "the x, y and z streams must not be NULL";
  else if (s->type != CC_COORD_F32 && s->type != CC_COORD_F64 && s->type != CC_COORD_I32) why = "type must be CC_COORD_F32, _F64 or _I32";
  else {
    const int size = coord_bytes(s->type);
    if (s->stride_bytes < size || s->stride_bytes % size != 0) why = "stride_bytes must be a multiple of the element size and not below it";
    else if (s->stride_bytes > CC_POINT_STRIDE_MAX) why = "stride_bytes above CC_POINT_STRIDE_MAX";
    else if ((((uintptr_t)s->x | (uintptr_t)s->y | (uintptr_t)s->z) & (uintptr_t)(size - 1)) != 0) why = "every stream must be aligned to the element size";
    else if (s->type == CC_COORD_I32 && !(std::isfinite(s->scale[0]) && std::isfinite(s->scale[1]) && std::isfinite(s->scale[2]))) why = "every scale must be finite";
  }
  for (size_t i = 0; !why && h_origin && i < (size_t)n_scans * 3; i++)
    if (!std::isfinite(h_origin[i])) why = "every origin component must be finite";
  for (int i = 0; !why && i < n_scans; i++) {
    const int64_t n = h_offsets[i + 1] - h_offsets[i];
    if (!(n > 10)) why = "scan with <= 10 points (CHECK_GT(size, 10), contour_mng.h:507)";
    else if (n >= (1 << CC_K1_IDX_BITS)) why = "scan with >= 2^21 points";
  }
  if (why) return set_err(CC_EINVAL, (std::string(who) + ": " + why).c_str());
  return CC_OK;
}
static int images_check(const cc_ctx *c, const void *height, const void *out, int n_scans, const char *who) {
  const char *why = nullptr;
  if (!c) why = "ctx must not be NULL";
  else if (!height) why = "height must not be NULL";
  else if (!out) why = "out must not be NULL";
  else if (n_scans < 0) why = "n_scans must not be negative";
  if (why) return set_err(CC_EINVAL, (std::string(who) + ": " + why).c_str());
  return CC_OK;
}
// Everything the header promises to check about a cc_*_segments call, before anything is queued or read.  tab: one entry per segment,
// `base` = the caller's pointer + xyz_offset (the host calls replace it with where the records went on the device); q_off: the scans'
// point totals as offsets.
static int segs_check(const cc_point_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, const char *who, std::vector<cc_k1_seg> &tab,
                      std::vector<int64_t> &q_off) {
  q_off.assign(1, 0);
  for (int i = 0; i < n_scans; i++) {
    const int64_t ns = (int64_t)h_scan_segs[i + 1] - h_scan_segs[i];
    if (h_scan_segs[i] < 0 || ns < 1 || ns > CC_SEG_MAX) return set_err(CC_EINVAL, CC_WHO(": a scan has 1 .. CC_SEG_MAX segments"));
    int64_t total = 0;
    for (int k = h_scan_segs[i]; k < h_scan_segs[i + 1]; k++) {
      const cc_point_segment_t &g = h_segs[k];
      if (g.n_points < 0 || g.n_points >= (1 << CC_K1_IDX_BITS)) return set_err(CC_EINVAL, CC_WHO(": a segment's n_points is negative or >= 2^21"));
      if (g.n_points > 0 && !g.points) return set_err(CC_EINVAL, CC_WHO(": a segment with points has a NULL pointer"));
      cc_point_layout_t lay;
      const bool dflt = g.layout.stride_bytes == 0 && g.layout.xyz_offset == 0;
      const int rcl = point_layout(dflt ? nullptr : &g.layout, g.n_points > 0 ? g.points : nullptr, who, &lay);
      if (rcl != CC_OK) return rcl;
      cc_k1_seg e;
      e.base = (const char *)g.points + lay.xyz_offset;
      e.stride = (unsigned)lay.stride_bytes;
      e.first = (int)total;
      e.n = (int)g.n_points;
      e.has_tf = g.has_tf != 0;
      for (int m = 0; m < 12; m++) e.m[m] = g.has_tf ? g.tf[m] : 0.f;
      tab.push_back(e);
      total += g.n_points;
      if (total >= (1 << CC_K1_IDX_BITS)) return set_err(CC_EINVAL, CC_WHO(": scan with >= 2^21 points"));
    }
    if (!(total > 10)) return set_err(CC_EINVAL, CC_WHO(": scan with <= 10 points (CHECK_GT(size, 10), contour_mng.h:507)"));
    q_off.push_back(q_off.back() + total);
  }
  return CC_OK;
}
static_assert(CC_K1_RIG_SEG_MAX == CC_RIG_SEG_MAX && (int)CC_K1_RIG_NONE == (int)CC_RIG_NONE && (int)CC_K1_RIG_TF == (int)CC_RIG_TF &&
                  (int)CC_K1_RIG_MOTION == (int)CC_RIG_MOTION,
              "k_rasterize.h's rig table and modes are the header's");
// Everything the header promises to check about a cc_*_rig call, before anything is queued or read: per segment what segs_check,
// motion_check and filter_check refuse (against the segment's own layout), then the rig's own rules.  tab, q_off: as segs_check's.
// What the kernels take of the rule -- the class rule's word position and width folded into a shift per segment and one mask, as
// stage_filter does it -- goes into the entries here.
static int rig_check(const k1_source &src, int n_scans, const char *who, std::vector<cc_k1_rseg> &tab, std::vector<int64_t> &q_off) {
  const cc_rig_segment_t *h_segs = src.h_rsegs;
  const int32_t *h_scan_segs = src.scan_segs;
  if (src.h_knots && (src.n_pool < 1 || src.n_pool > CC_MOTION_KNOTS_MAX)) return set_err(CC_EINVAL, CC_WHO(": n_pool must be 1 .. CC_MOTION_KNOTS_MAX"));
  q_off.assign(1, 0);
  for (int i = 0; i < n_scans; i++) {
    const int64_t ns = (int64_t)h_scan_segs[i + 1] - h_scan_segs[i];
    if (h_scan_segs[i] < 0 || ns < 1 || ns > CC_RIG_SEG_MAX) return set_err(CC_EINVAL, CC_WHO(": a scan has 1 .. CC_RIG_SEG_MAX segments"));
    int64_t total = 0;
    for (int k = h_scan_segs[i]; k < h_scan_segs[i + 1]; k++) {
      const cc_rig_segment_t &g = h_segs[k];
      if (g.n_points < 0 || g.n_points >= (1 << CC_K1_IDX_BITS)) return set_err(CC_EINVAL, CC_WHO(": a segment's n_points is negative or >= 2^21"));
      if (g.n_points > 0 && !g.points) return set_err(CC_EINVAL, CC_WHO(": a segment with points has a NULL pointer"));
      cc_point_layout_t lay;
      const bool dflt = g.layout.stride_bytes == 0 && g.layout.xyz_offset == 0;
      int rc = point_layout(dflt ? nullptr : &g.layout, g.n_points > 0 ? g.points : nullptr, who, &lay);
      if (rc != CC_OK) return rc;
      cc_k1_rseg e = {};
      e.base = (const char *)g.points + lay.xyz_offset;
      e.stride = (unsigned)lay.stride_bytes;
      e.first = (int)total;
      e.n = (int)g.n_points;
      if (g.mode == CC_RIG_TF) {
        e.flags = CC_K1_RIG_TF;
        for (int m = 0; m < 12; m++) e.m[m] = g.tf[m];
      } else if (g.mode == CC_RIG_MOTION) {
        if (!src.h_knots) return set_err(CC_EINVAL, CC_WHO(": a segment in motion mode needs h_knots"));
        const cc_point_motion_t mo = {g.time_offset, g.time_type, g.n_knots, 0};
        const float tm[2] = {g.t_begin, g.scale};
        rc = motion_check(lay, &mo, tm, src.h_knots, 1, who);
        if (rc != CC_OK) return rc;
        if (g.knot0 < 0 || (int64_t)g.knot0 + g.n_knots > src.n_pool) return set_err(CC_EINVAL, CC_WHO(": a segment's slice [knot0, knot0 + n_knots) lies outside the pool"));
        e.flags = CC_K1_RIG_MOTION | (g.time_type == CC_TIME_U32 ? CC_K1_RIG_TIME_U32 : 0u);
        e.t_off = g.time_offset - lay.xyz_offset;
        e.m[0] = g.t_begin;
        e.m[1] = g.scale;
        memcpy(&e.m[2], &g.knot0, 4);
        memcpy(&e.m[3], &g.n_knots, 4);
      } else if (g.mode != CC_RIG_NONE) {
        return set_err(CC_EINVAL, CC_WHO(": a segment's mode must be CC_RIG_NONE, CC_RIG_TF or CC_RIG_MOTION"));
      }
      if (g.filter_offset < -1) return set_err(CC_EINVAL, CC_WHO(": a segment's filter_offset must be -1 or an offset inside the record"));
      if (g.filter_offset >= 0) {
        if (!src.has_flt) return set_err(CC_EINVAL, CC_WHO(": a segment with a filter word needs the filter"));
        cc_point_filter_t f = src.flt;
        f.offset = g.filter_offset;
        rc = filter_check(lay, &f, who);
        if (rc != CC_OK) return rc;
        e.flags |= CC_K1_RIG_FILTERED;
        e.w_off = (f.offset & ~3) - lay.xyz_offset;
        if (f.type != CC_FILTER_F32) e.flags |= (unsigned)(8 * (f.offset & 3) + f.shift) << CC_K1_RIG_SHIFT_POS;
      }
      tab.push_back(e);
      total += g.n_points;
      if (total >= (1 << CC_K1_IDX_BITS)) return set_err(CC_EINVAL, CC_WHO(": scan with >= 2^21 points"));
    }
    if (!(total > 10)) return set_err(CC_EINVAL, CC_WHO(": scan with <= 10 points (CHECK_GT(size, 10), contour_mng.h:507)"));
    q_off.push_back(q_off.back() + total);
  }
  if (src.has_flt) {  // the rule itself, also when no segment of this call uses it (its offset is not read: a word that passes every layout)
    cc_point_filter_t f = src.flt;
    f.offset = 0;
    const cc_point_layout_t wide = {CC_POINT_STRIDE_MAX, CC_POINT_STRIDE_MAX - 12};
    const int rc = filter_check(wide, &f, who);
    if (rc != CC_OK) return rc;
  }
  return CC_OK;
}

// The three forms of every family's entry points: the records on the device, a batch of host records (*_host), one scan of the
// per-scan loop (cc_scan_ingest*: n_scans = 1, h_offsets = {0, n_points}).
enum k1_form { K1_DEVICE, K1_HOST, K1_SCAN };
// What is checked of a call before anything is queued, read or touched, once per family: the arguments every form refuses (`out`: where
// the form's results go), then the family's own checks.  The *_host and per-scan forms copy their records to aligned device memory: a
// base's alignment counts in the device forms only (a range word's and a coordinate's in all: their checks read it off the host address).
// An IMAGES call of no scans passes (it is CC_OK and does nothing).  Behind it a SEGMENTS source holds its tables, with h_segs and
// scan_segs those of the call's first segment on, and a RANGES or IMAGES source its scans' offsets (own_off).
static int k1_check(cc_ctx *c, k1_source &src, k1_form form, const int64_t *h_offsets, int n_scans, const void *out, const char *who) {
  const bool few = n_scans < (form == K1_DEVICE ? 0 : 1);
  const void *base = form == K1_DEVICE ? src.points : nullptr;
  int rc = CC_OK;
  switch (src.kind) {
    case k1_source::POINTS:
    case k1_source::MOTION:
    case k1_source::FILTERED:
      if (!c || !src.points || !h_offsets || !out || few || (form == K1_SCAN && h_offsets[1] < 1)) return set_err(CC_EINVAL, CC_WHO(": bad argument"));
      rc = point_layout(&src.lay, base, who, &src.lay);
      if (rc == CC_OK && src.kind == k1_source::MOTION) rc = motion_check(src.lay, src.missing ? nullptr : &src.mot, src.h_time, src.h_knots, n_scans, who);
      if (rc == CC_OK && src.kind == k1_source::FILTERED) rc = filter_check(src.lay, src.missing ? nullptr : &src.flt, who);
      return rc;
    case k1_source::COORDS:
      if (!c || !h_offsets || !out || few) return set_err(CC_EINVAL, CC_WHO(": bad argument"));
      return coords_check(src.missing ? nullptr : &src.crd, h_offsets, n_scans, src.h_origin, who);
    case k1_source::RANGES:
      if (!c || !out || few) return set_err(CC_EINVAL, CC_WHO(": bad argument"));
      rc = ranges_check(c, src.sensor, src.points, src.h_knots, who);
      for (int i = 0; rc == CC_OK && i <= n_scans; i++) src.own_off.push_back((int64_t)src.sensor->kr.n_rows * src.sensor->kr.n_cols * i);
      return rc;
    case k1_source::IMAGES:
      rc = images_check(c, src.points, out, n_scans, who);
      if (rc != CC_OK) return rc;
      if (form == K1_DEVICE && ((uintptr_t)src.points & 15u) != 0) return set_err(CC_EINVAL, CC_WHO(": d_height must be 16-byte aligned"));
      if (form == K1_DEVICE && ((uintptr_t)src.pos_rc & 7u) != 0) return set_err(CC_EINVAL, CC_WHO(": d_pos_rc must be 8-byte aligned"));
      for (int i = 0; i <= n_scans; i++) src.own_off.push_back((int64_t)i * c->dcfg.n_cell);
      return CC_OK;
    case k1_source::SEGMENTS:
      if (!c || !src.h_segs || !src.scan_segs || !out || few) return set_err(CC_EINVAL, CC_WHO(": bad argument"));
      rc = segs_check(src.h_segs, src.scan_segs, n_scans, who, src.seg_tab, src.own_off);
      if (rc != CC_OK) return rc;
      for (int i = 0; i <= n_scans; i++) src.seg_scan.push_back(src.scan_segs[i] - src.scan_segs[0]);  // (seg_tab begins with the call's first segment)
      src.h_segs += src.scan_segs[0];
      src.segs = src.seg_tab.data();
      src.scan_segs = src.seg_scan.data();
      return CC_OK;
    case k1_source::RIG:
      if (!c || !src.h_rsegs || !src.scan_segs || !out || few) return set_err(CC_EINVAL, CC_WHO(": bad argument"));
      rc = rig_check(src, n_scans, who, src.rig_tab, src.own_off);
      if (rc != CC_OK) return rc;
      for (int i = 0; i <= n_scans; i++) src.seg_scan.push_back(src.scan_segs[i] - src.scan_segs[0]);  // (rig_tab begins with the call's first segment)
      src.h_rsegs += src.scan_segs[0];
      src.scan_segs = src.seg_scan.data();
      return CC_OK;
  }
  return CC_OK;
}
// the scans' offsets in points: the caller's, or the checked source's own
static const int64_t *k1_offsets(const k1_source &src, const int64_t *h_offsets) { return src.own_off.empty() ? h_offsets : src.own_off.data(); }

// Where the host bytes of a *_host or per-scan call go in ONE device buffer, and where the source's pointers lie in it then.
struct k1_host_plan {
  struct copy {
    const void *from;
    size_t bytes, at;
  };
  std::vector<copy> copies;
  size_t total = 0;              // the buffer's bytes
  bool zero_out = false;         // the call's descriptors are zeroed before its kernels run
  const void *staged = nullptr;  // the per-scan forms: the address a caller of cc_stage_points* hands over in place of records (nullptr: never staged)
  size_t pos_rc = 0, crd[3] = {0, 0, 0};  // IMAGES: the positions; COORDS: x, y, z of the first point (`points` lies at 0)
  std::vector<size_t> seg_base;  // SEGMENTS: x of every segment's first record
  void add(const void *from, size_t bytes, size_t at) { copies.push_back({from, bytes, at}); }
};
// The plan of `n_points` points from point `first` on of a checked source with host addresses (SEGMENTS: of all its segments).
static k1_host_plan k1_plan(const k1_source &src, k1_form form, int64_t first, int64_t n_points) {
  k1_host_plan p;
  const size_t n = (size_t)n_points;
  switch (src.kind) {
    case k1_source::POINTS:
    case k1_source::MOTION:
    case k1_source::FILTERED: {  // the records travel as they are, in ONE copy
      const size_t stride = (size_t)src.lay.stride_bytes;
      p.add((const char *)src.points + stride * (size_t)first, stride * n, 0);
      p.total = stride * n;
      p.staged = src.points;
      break;
    }
    case k1_source::RANGES: {
      const size_t word = (size_t)src.sensor->word_bytes;
      p.add((const char *)src.points + word * (size_t)first, word * n, 0);
      p.total = word * n;
      p.staged = src.points;
      break;
    }
    case k1_source::IMAGES:  // the heights, and the positions behind them
      p.add((const float *)src.points + first, sizeof(float) * n, 0);
      p.pos_rc = sizeof(float) * n;
      if (src.pos_rc) p.add(src.pos_rc + 2 * first, 2 * sizeof(float) * n, p.pos_rc);
      p.total = sizeof(float) * n * (src.pos_rc ? 3 : 1);
      break;
    case k1_source::COORDS: {
      // Exactly the bytes the streams span.  The highest stream's element within stride_bytes of the lowest stream: ONE record array,
      // one copy from the lowest pointer; otherwise three arrays, three copies, each at a 16-byte boundary of the device buffer.
      const cc_coord_src_t &s = src.crd;
      const size_t stride = (size_t)s.stride_bytes, elem = (size_t)coord_bytes(s.type), run = (n - 1) * stride;
      const char *q[3] = {(const char *)s.x + (size_t)first * stride, (const char *)s.y + (size_t)first * stride, (const char *)s.z + (size_t)first * stride};
      const char *lo = q[0], *hi = q[0];
      for (int k = 1; k < 3; k++) {
        lo = (uintptr_t)q[k] < (uintptr_t)lo ? q[k] : lo;
        hi = (uintptr_t)q[k] > (uintptr_t)hi ? q[k] : hi;
      }
      const size_t span = (size_t)((uintptr_t)hi - (uintptr_t)lo) + elem;
      if (span <= stride) {
        p.add(lo, run + span, 0);
        for (int k = 0; k < 3; k++) p.crd[k] = (size_t)((uintptr_t)q[k] - (uintptr_t)lo);
        p.total = run + span;
      } else {
        const size_t piece = (run + elem + 15) & ~(size_t)15;
        for (int k = 0; k < 3; k++) {
          p.crd[k] = (size_t)k * piece;
          p.add(q[k], run + elem, p.crd[k]);
        }
        p.total = 2 * piece + run + elem;
      }
      break;
    }
    case k1_source::SEGMENTS:  // one segment after the other, each at a 16-byte boundary, whole records
      for (size_t k = 0; k < src.seg_tab.size(); k++) {
        const cc_k1_seg &g = src.seg_tab[k];
        if (g.n > 0) p.add(src.h_segs[k].points, (size_t)g.n * g.stride, p.total);
        p.seg_base.push_back(p.total + (size_t)(g.base - (const char *)src.h_segs[k].points));
        p.total += ((size_t)g.n * g.stride + 15) & ~(size_t)15;
      }
      break;
    case k1_source::RIG:  // as SEGMENTS
      for (size_t k = 0; k < src.rig_tab.size(); k++) {
        const cc_k1_rseg &g = src.rig_tab[k];
        if (g.n > 0) p.add(src.h_rsegs[k].points, (size_t)g.n * g.stride, p.total);
        p.seg_base.push_back(p.total + (size_t)(g.base - (const char *)src.h_rsegs[k].points));
        p.total += ((size_t)g.n * g.stride + 15) & ~(size_t)15;
      }
      break;
  }
  // The rows of a descriptor that its counts do not cover are not written by the kernels, and a pool slot holds an earlier scan's rows:
  // where a form zeroes, its bytes are those of the family's device call into zeroed memory.
  switch (src.kind) {
    case k1_source::SEGMENTS:
    case k1_source::RIG:
    case k1_source::IMAGES:
    case k1_source::COORDS: p.zero_out = true; break;
    case k1_source::FILTERED: p.zero_out = form == K1_HOST; break;  // (the batch form as cc_ingest_images_host does; the per-scan form as POINTS')
    case k1_source::POINTS:
    case k1_source::MOTION:
    case k1_source::RANGES: p.zero_out = false; break;  // (what lies behind the counts is the allocation's, or the pool slot's)
  }
  return p;
}
// The device addresses of a planned source whose buffer lies at d_base.
static void k1_rebase(k1_source &src, const k1_host_plan &plan, const void *d_base) {
  const char *d = (const char *)d_base;
  src.points = d;
  if (src.pos_rc) src.pos_rc = (const float *)(d + plan.pos_rc);
  if (src.kind == k1_source::COORDS) {
    src.crd.x = d + plan.crd[0];
    src.crd.y = d + plan.crd[1];
    src.crd.z = d + plan.crd[2];
  }
  for (size_t k = 0; k < plan.seg_base.size(); k++) {
    if (src.kind == k1_source::RIG) src.rig_tab[k].base = d + plan.seg_base[k];
    else src.seg_tab[k].base = d + plan.seg_base[k];
  }
}

// `bytes` of pinned memory in slot `slot` of the staging ring (the buffer the chunk's segment table, times and knots ride in), grown
// when it is too small; nullptr with the error set when the allocation fails.
static char *slot_stage(cc_ctx *c, int slot, size_t bytes) {
  if (c->h_seg_cap[slot] < bytes) {
    if (c->h_seg[slot]) hipHostFree(c->h_seg[slot]);
    c->h_seg[slot] = nullptr;
    c->h_seg_cap[slot] = 0;
    const hipError_t e = hipHostMalloc((void **)&c->h_seg[slot], bytes * 2, hipHostMallocDefault);
    if (e != hipSuccess) {
      c->h_seg[slot] = nullptr;
      set_err(CC_EHIP, "hipHostMalloc of a staging slot", e);
      return nullptr;
    }
    c->h_seg_cap[slot] = bytes * 2;
  }
  return c->h_seg[slot];
}
// What a chunk's K1 reads on the device besides the points and the offsets: set by the staging functions, read by k1_dispatch.
struct k1_staged {
  const float *d_tf = nullptr;  // POINTS; IMAGES: the chunk's min_height values
  cc_k1_motion mot = {};        // MOTION
  cc_k1_range rng = {};         // RANGES
  cc_k1_segs segs = {};         // SEGMENTS
  cc_k1_filter flt = {};        // FILTERED
  cc_k1_rig rig = {};           // RIG
  const double *d_org = nullptr;  // COORDS: the chunk's origins, or nullptr
};
// What the kernels take of a checked filter.  The class rule reads the aligned dword that holds the word: the word's byte position
// and width go into the shift and the mask, so one instance serves u8, u16 and u32.  Its table rides in slot `slot` of the staging
// ring (the segment tables' buffer: a call has one or the other) to S.d_flt, with keep_other as bit n_classes and zeros behind it.
static int stage_filter(cc_ctx *c, cc_ctx::Scratch &S, int slot, const k1_source &src, hipStream_t stream, cc_k1_filter &kf) {
  const cc_point_filter_t &f = src.flt;
  kf.w_off = (f.offset & ~3) - src.lay.xyz_offset;
  kf.lo = f.lo;
  kf.hi = f.hi;
  if (f.type == CC_FILTER_F32) return CC_OK;
  const int size = filter_bytes(f.type);
  const unsigned typemask = size == 4 ? 0xFFFFFFFFu : ((1u << (8 * size)) - 1u);
  kf.shift = (unsigned)(8 * (f.offset & 3) + f.shift);
  kf.mask = f.mask & (typemask >> f.shift);
  kf.n_classes = (unsigned)f.n_classes;
  const size_t bytes = sizeof(unsigned) * CC_K1_FLT_TAB_WORDS;
  if (!S.d_flt) HIPCHK(hipMalloc(&S.d_flt, bytes));
  if (!slot_stage(c, slot, bytes)) return CC_EHIP;
  unsigned *tab = (unsigned *)c->h_seg[slot];
  const int nw = (f.n_classes + 31) / 32;
  memset(tab, 0, bytes);
  memcpy(tab, f.keep_bits, sizeof(unsigned) * (size_t)nw);
  if (f.n_classes % 32) tab[nw - 1] &= (1u << (f.n_classes % 32)) - 1u;  // (the caller's bits behind n_classes are not part of the table)
  if (f.keep_other) tab[f.n_classes >> 5] |= 1u << (f.n_classes & 31);
  HIPCHK(hipMemcpyAsync(S.d_flt, tab, bytes, hipMemcpyHostToDevice, stream));
  kf.bits = S.d_flt;
  return CC_OK;
}
// A chunk's knots (behind its [nb][2] times when h_time is given) to S.d_mot.  They ride in slot `slot` of the staging ring, in the
// segment tables' buffer: a call has one or the other.
static int stage_knots(cc_ctx *c, cc_ctx::Scratch &S, int slot, const float *h_time, const float *h_knots, int n_knots, int b0, int nb, hipStream_t stream,
                       const float *&d_time, const float *&d_knots) {
  const size_t kf = (size_t)n_knots * 12, nt = h_time ? 2 * (size_t)nb : 0, bytes = sizeof(float) * (nt + kf * (size_t)nb);
  if (!S.d_mot) HIPCHK(hipMalloc(&S.d_mot, sizeof(float) * (2 + (size_t)CC_MOTION_KNOTS_MAX * 12) * (size_t)S.cap));
  if (!slot_stage(c, slot, bytes)) return CC_EHIP;
  float *hm = (float *)c->h_seg[slot];
  if (h_time) memcpy(hm, h_time + (size_t)b0 * 2, sizeof(float) * nt);
  memcpy(hm + nt, h_knots + (size_t)b0 * kf, sizeof(float) * kf * (size_t)nb);
  HIPCHK(hipMemcpyAsync(S.d_mot, hm, bytes, hipMemcpyHostToDevice, stream));
  d_time = S.d_mot;
  d_knots = S.d_mot + nt;
  return CC_OK;
}
// A chunk's segment table to S.d_seg, in the same slot of the ring: scan_seg[nb + 1] relative to the chunk's first segment, then the entries.
static int stage_segments(cc_ctx *c, cc_ctx::Scratch &S, int slot, const k1_source &src, int b0, int nb, hipStream_t stream, cc_k1_segs &d_segs) {
  const int s0 = src.scan_segs[b0], ns = src.scan_segs[b0 + nb] - s0;
  const size_t ent_off = (sizeof(int) * (size_t)(nb + 1) + 7) & ~(size_t)7, bytes = ent_off + sizeof(cc_k1_seg) * (size_t)ns;
  if (!S.d_seg) HIPCHK(hipMalloc(&S.d_seg, ((sizeof(int) * (size_t)(S.cap + 1) + 7) & ~(size_t)7) + sizeof(cc_k1_seg) * CC_SEG_MAX * (size_t)S.cap));
  if (!slot_stage(c, slot, bytes)) return CC_EHIP;
  int *ss = (int *)c->h_seg[slot];
  for (int i = 0; i <= nb; i++) ss[i] = src.scan_segs[b0 + i] - s0;
  memcpy(c->h_seg[slot] + ent_off, src.segs + s0, sizeof(cc_k1_seg) * (size_t)ns);
  HIPCHK(hipMemcpyAsync(S.d_seg, c->h_seg[slot], bytes, hipMemcpyHostToDevice, stream));
  d_segs.scan_seg = (const int *)S.d_seg;
  d_segs.seg = (const cc_k1_seg *)(S.d_seg + ent_off);
  return CC_OK;
}
// A rig chunk's tables to S.d_rig, in the same slot of the ring and in ONE copy: scan_seg[nb + 1] relative to the chunk's first segment,
// the entries, the chunk's knot pools, the rule's class table (stage_filter's: keep_other as bit n_classes, zeros behind it).
static int stage_rig(cc_ctx *c, cc_ctx::Scratch &S, int slot, const k1_source &src, int b0, int nb, hipStream_t stream, cc_k1_rig &kr) {
  const int s0 = src.scan_segs[b0], ns = src.scan_segs[b0 + nb] - s0;
  const bool cls = src.has_flt && src.flt.type != CC_FILTER_F32;
  const size_t pool = sizeof(float) * 12 * (size_t)src.n_pool, tabw = sizeof(unsigned) * CC_K1_FLT_TAB_WORDS;
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t ent_off = up16(sizeof(int) * (size_t)(nb + 1)), kn_off = ent_off + sizeof(cc_k1_rseg) * (size_t)ns, bit_off = up16(kn_off + pool * (size_t)nb),
               bytes = bit_off + (cls ? tabw : 0);
  if (!S.d_rig)
    HIPCHK(hipMalloc(&S.d_rig, up16(sizeof(int) * (size_t)(S.cap + 1)) + (sizeof(cc_k1_rseg) * CC_RIG_SEG_MAX + sizeof(float) * 12 * CC_MOTION_KNOTS_MAX) * (size_t)S.cap + 16 + tabw));
  if (!slot_stage(c, slot, bytes)) return CC_EHIP;
  char *h = c->h_seg[slot];
  int *ss = (int *)h;
  for (int i = 0; i <= nb; i++) ss[i] = src.scan_segs[b0 + i] - s0;
  memcpy(h + ent_off, src.rig_tab.data() + s0, sizeof(cc_k1_rseg) * (size_t)ns);
  if (src.h_knots) memcpy(h + kn_off, src.h_knots + (size_t)b0 * 12 * (size_t)src.n_pool, pool * (size_t)nb);
  kr = cc_k1_rig();
  kr.kind = -1;
  if (src.has_flt) {
    const cc_point_filter_t &f = src.flt;
    kr.kind = cls ? CC_K1_FLT_CLASS : CC_K1_FLT_RANGE;
    kr.lo = f.lo;
    kr.hi = f.hi;
    if (cls) {
      const int size = filter_bytes(f.type);
      const unsigned typemask = size == 4 ? 0xFFFFFFFFu : ((1u << (8 * size)) - 1u);
      kr.mask = f.mask & (typemask >> f.shift);
      kr.n_classes = (unsigned)f.n_classes;
      unsigned *tab = (unsigned *)(h + bit_off);
      const int nw = (f.n_classes + 31) / 32;
      memset(tab, 0, tabw);
      memcpy(tab, f.keep_bits, sizeof(unsigned) * (size_t)nw);
      if (f.n_classes % 32) tab[nw - 1] &= (1u << (f.n_classes % 32)) - 1u;  // (the caller's bits behind n_classes are not part of the table)
      if (f.keep_other) tab[f.n_classes >> 5] |= 1u << (f.n_classes & 31);
      kr.bits = (const unsigned *)(S.d_rig + bit_off);
    }
  }
  HIPCHK(hipMemcpyAsync(S.d_rig, h, bytes, hipMemcpyHostToDevice, stream));
  kr.scan_seg = (const int *)S.d_rig;
  kr.seg = (const cc_k1_rseg *)(S.d_rig + ent_off);
  kr.knots = src.h_knots ? (const float *)(S.d_rig + kn_off) : nullptr;
  kr.n_pool = src.n_pool;
  return CC_OK;
}
// The copies of a chunk's tables (scans b0 .. b0 + nb - 1), queued behind its offsets; off: the ring slot's pinned offsets.
static int k1_stage(cc_ctx *c, cc_ctx::Scratch &S, int slot, long long *off, const k1_source &src, const int64_t *h_offsets, int b0, int nb, hipStream_t stream,
                    k1_staged &st) {
  switch (src.kind) {
    case k1_source::COORDS:
      if (src.h_origin) {  // the chunk's origins ride in the same slot, behind the room of the transforms: 24 bytes per scan
        double *org = (double *)((char *)off + (sizeof(long long) + sizeof(float) * 12) * (size_t)(c->off_cap + 1));
        if (!S.d_org) HIPCHK(hipMalloc(&S.d_org, sizeof(double) * 3 * (size_t)S.cap));
        memcpy(org, src.h_origin + (size_t)b0 * 3, sizeof(double) * 3 * (size_t)nb);
        HIPCHK(hipMemcpyAsync(S.d_org, org, sizeof(double) * 3 * (size_t)nb, hipMemcpyHostToDevice, stream));
        st.d_org = S.d_org;
      }
      [[fallthrough]];  // the transforms: as for POINTS
    case k1_source::FILTERED:
      if (src.kind == k1_source::FILTERED) {
        const int rcf = stage_filter(c, S, slot, src, stream, st.flt);
        if (rcf != CC_OK) return rcf;
      }
      [[fallthrough]];  // the transforms: as for POINTS
    case k1_source::POINTS:
      if (src.h_tf) {  // the chunk's transforms ride in the same slot, behind the offsets
        float *tfs = (float *)(off + c->off_cap + 1);
        memcpy(tfs, src.h_tf + (size_t)b0 * 12, sizeof(float) * 12 * (size_t)nb);
        HIPCHK(hipMemcpyAsync(S.d_tf, tfs, sizeof(float) * 12 * (size_t)nb, hipMemcpyHostToDevice, stream));
        st.d_tf = S.d_tf;
      }
      return CC_OK;
    case k1_source::SEGMENTS:
      return stage_segments(c, S, slot, src, b0, nb, stream, st.segs);
    case k1_source::RIG:
      return stage_rig(c, S, slot, src, b0, nb, stream, st.rig);
    case k1_source::MOTION:
      st.mot.t_off = src.mot.time_offset - src.lay.xyz_offset;
      st.mot.time_u32 = src.mot.time_type == CC_TIME_U32 ? 1 : 0;
      st.mot.n_knots = src.mot.n_knots;
      return stage_knots(c, S, slot, src.h_time, src.h_knots, src.mot.n_knots, b0, nb, stream, st.mot.time, st.mot.knots);
    case k1_source::RANGES: {
      st.rng = src.sensor->kr;
      st.rng.words = (const char *)src.points + (long long)h_offsets[b0] * src.sensor->word_bytes;
      st.rng.knots = nullptr;
      const float *none = nullptr;
      return st.rng.n_knots > 0 ? stage_knots(c, S, slot, nullptr, src.h_knots, st.rng.n_knots, b0, nb, stream, none, st.rng.knots) : CC_OK;
    }
    case k1_source::IMAGES:
      if (src.h_min) {  // the chunk's minima ride where a chunk's transforms do (an image call has none), and wait in S.d_tf
        float *mins = (float *)(off + c->off_cap + 1);
        memcpy(mins, src.h_min + (size_t)b0, sizeof(float) * (size_t)nb);
        HIPCHK(hipMemcpyAsync(S.d_tf, mins, sizeof(float) * (size_t)nb, hipMemcpyHostToDevice, stream));
        st.d_tf = S.d_tf;
      }
      return CC_OK;
  }
  return CC_OK;
}
// The chunk's K1: the instance its source asks for.  KITTI records without a transform take the float4 loader (16-byte loads: the base
// must be aligned for them); everything else one of the record loaders' instances.
static int k1_dispatch(cc_ctx *c, cc_ctx::Scratch &S, const k1_source &src, const k1_staged &st, int64_t first, int nb, int want_dense, hipStream_t stream) {
  const int stride = src.lay.stride_bytes;
  const char *rpts = nullptr;  // POINTS, MOTION: x of the chunk's first point
  if (src.kind == k1_source::POINTS || src.kind == k1_source::MOTION || src.kind == k1_source::FILTERED) rpts = (const char *)src.points + (long long)first * stride + src.lay.xyz_offset;
  switch (src.kind) {
    case k1_source::POINTS:
      if (stride == 16 && src.lay.xyz_offset == 0 && !src.h_tf && ((uintptr_t)src.points & 15u) == 0)
        return k1_launch(c, S, cc_src_kitti{(const float4 *)src.points + first}, nb, want_dense, stream);
      switch (stride) {
        case 12: return k1_launch(c, S, cc_src_rec<12>{rpts, stride, st.d_tf}, nb, want_dense, stream);
        case 16: return k1_launch(c, S, cc_src_rec<16>{rpts, stride, st.d_tf}, nb, want_dense, stream);
        default: return k1_launch(c, S, cc_src_rec<0>{rpts, stride, st.d_tf}, nb, want_dense, stream);
      }
    case k1_source::MOTION:
      switch (stride) {
        case 16: return k1_launch(c, S, cc_src_mot<16>{rpts, stride, st.mot}, nb, want_dense, stream);
        case 32: return k1_launch(c, S, cc_src_mot<32>{rpts, stride, st.mot}, nb, want_dense, stream);
        default: return k1_launch(c, S, cc_src_mot<0>{rpts, stride, st.mot}, nb, want_dense, stream);
      }
    case k1_source::RANGES:
      switch (src.sensor->word_type) {
        case CC_RANGE_U16: return k1_launch(c, S, cc_src_rng<CC_K1_WORD_U16>{st.rng}, nb, want_dense, stream);
        case CC_RANGE_U32: return k1_launch(c, S, cc_src_rng<CC_K1_WORD_U32>{st.rng}, nb, want_dense, stream);
        default: return k1_launch(c, S, cc_src_rng<CC_K1_WORD_F32>{st.rng}, nb, want_dense, stream);
      }
    case k1_source::SEGMENTS:
      return k1_launch(c, S, cc_src_seg{st.segs}, nb, want_dense, stream);
    case k1_source::RIG:
      return k1_launch(c, S, cc_src_rig{st.rig}, nb, want_dense, stream);
    case k1_source::FILTERED:
      if (src.flt.type == CC_FILTER_F32) return k1_launch(c, S, cc_src_flt<CC_K1_FLT_RANGE>{rpts, stride, st.d_tf, st.flt}, nb, want_dense, stream);
      return k1_launch(c, S, cc_src_flt<CC_K1_FLT_CLASS>{rpts, stride, st.d_tf, st.flt}, nb, want_dense, stream);
    case k1_source::COORDS: {
      const long long at = (long long)first * src.crd.stride_bytes;
      cc_k1_coords kc = {(const char *)src.crd.x + at, (const char *)src.crd.y + at, (const char *)src.crd.z + at, src.crd.stride_bytes, {1.0, 1.0, 1.0}, st.d_org, st.d_tf};
      switch (src.crd.type) {
        case CC_COORD_F64: return k1_launch(c, S, cc_src_coord<CC_K1_COORD_F64>{kc}, nb, want_dense, stream);
        case CC_COORD_I32:
          for (int k = 0; k < 3; k++) kc.scale[k] = src.crd.scale[k];
          return k1_launch(c, S, cc_src_coord<CC_K1_COORD_I32>{kc}, nb, want_dense, stream);
        default: return k1_launch(c, S, cc_src_coord<CC_K1_COORD_F32>{kc}, nb, want_dense, stream);
      }
    }
    case k1_source::IMAGES:  // first = b0 * n_cell, a multiple of 4 floats (cc_create): the chunk's base is 16-byte aligned like the call's
      hipLaunchKernelGGL((cc_k_image_list<CC_IMAGE_BLOCK>), dim3(nb), dim3(CC_IMAGE_BLOCK), 0, stream, c->dcfg, (const float4 *)((const float *)src.points + first),
                         src.pos_rc ? (const float2 *)src.pos_rc + first : nullptr, st.d_tf, S.d_bev, S.d_pix, S.d_k1, S.list, want_dense);
      return CC_OK;
  }
  return CC_OK;
}

// An ingest call on the scratch set S (c->ing_mu held by the caller; src holds device addresses).
static int ingest_on(cc_ctx *c, cc_ctx::Scratch &S, const k1_source &src, const int64_t *h_offsets, int n_scans, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg,
                     hipStream_t stream, const char *who) {
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < n_scans && src.kind != k1_source::IMAGES; i++) {  // (an image is the caller's: no rule on points)
    const int64_t n = h_offsets[i + 1] - h_offsets[i];
    if (!(n > 10)) return set_err(CC_EINVAL, CC_WHO(": scan with <= 10 points (CHECK_GT(size, 10), contour_mng.h:507)"));
    if (n >= (1 << CC_K1_IDX_BITS)) return set_err(CC_EINVAL, CC_WHO(": scan with >= 2^21 points"));
  }
  const size_t nc = (size_t)c->dcfg.n_cell;
  if (S.has_last && S.last_stream != stream) HIPCHK(hipStreamWaitEvent(stream, S.ev_last, 0));
  for (int b0 = 0; b0 < n_scans; b0 += S.cap) {
    const int nb = (n_scans - b0 < S.cap) ? n_scans - b0 : S.cap;
    // offsets relative to the chunk's first point, staged in pinned memory: the call only queues work
    const int slot = c->off_next;
    c->off_next = (slot + 1) % cc_ctx::NSLOT;
    if (c->off_busy[slot]) HIPCHK(hipEventSynchronize(c->off_ev[slot]));
    long long *off = c->h_off[slot];
    for (int i = 0; i <= nb; i++) off[i] = (long long)(h_offsets[b0 + i] - h_offsets[b0]);
    HIPCHK(hipMemcpyAsync(S.d_offsets, off, sizeof(long long) * (nb + 1), hipMemcpyHostToDevice, stream));
    k1_staged st;
    const int rcs = k1_stage(c, S, slot, off, src, h_offsets, b0, nb, stream, st);
    if (rcs != CC_OK) return rcs;
    HIPCHK(hipEventRecord(c->off_ev[slot], stream));
    c->off_busy[slot] = true;
    // K1's dense image / positions: for the debug outputs, for a configuration K2's list kernel hands on as a whole
    // (min_cont_cell_cnt_ > 3); otherwise only for scans whose active cells overflow the list
    const int want_dense = ((dbg && (dbg->d_bev || dbg->d_pix_rc)) || c->dcfg.min_cont_cell_cnt > 3) ? 1 : 0;
    if (dbg && dbg->d_pix_rc)
      hipLaunchKernelGGL(cc_k_fill_f32, dim3(512), dim3(256), 0, stream, (float *)S.d_pix, -1.f, nc * 2 * nb);
    hipEvent_t *pe = nullptr;
    if (c->prof) {
      if (c->ev_used + 3 > c->ev.size() && prof_flush(c) != CC_OK) return set_err(CC_EHIP, "profiling event sync failed");
      pe = &c->ev[c->ev_used];
      c->ev_used += 3;
      HIPCHK(hipEventRecord(pe[0], stream));
    }
    const int rck = k1_dispatch(c, S, src, st, h_offsets[b0], nb, want_dense, stream);
    if (rck != CC_OK) return rck;
    if (pe) HIPCHK(hipEventRecord(pe[1], stream));
    int16_t *lab = (dbg && dbg->d_labels) ? dbg->d_labels + (size_t)b0 * CC_NLEV * nc : nullptr;
    hipLaunchKernelGGL(cc_k_contours, dim3(nb), dim3(CC_K2_BLOCK), (size_t)CC_K2L_LDS_BYTES, stream, c->dcfg, (const float *)S.d_bev,
                       (const float2 *)S.d_pix, (const cc_k1_scan_out *)S.d_k1, S.d_scr, d_out + b0, lab, S.d_midq, S.list);
    // the scans the list kernel handed on (more active cells / components than its LDS tables hold): the original body.
    // Its workgroups need 78 KB of LDS each to START, even those that find the queue empty and leave at once: behind a
    // pipelined ingest 512 of them waited 0.13 ms for their turns (the other streams' kernels hold the LDS).  So the
    // launch is sized by what the previous one found: 16 workgroups while the queue stays empty (they take whatever shows
    // up, one scan after the other, and the next launch is a full one again), 512 otherwise and at first.
    const int mid_seen = *(volatile int *)S.h_mid_seen;
    const int mid_wgs = mid_seen == 0 ? 16 : 512;
    hipLaunchKernelGGL(cc_k_contours_mid, dim3(nb < mid_wgs ? nb : mid_wgs), dim3(CC_K2_BLOCK), c->lds2, stream, c->dcfg, S.d_bev, S.d_pix,
                       (const cc_k1_scan_out *)S.d_k1, S.d_scr, S.d_midq, S.d_bigq, d_out + b0, lab, S.h_mid_seen, S.list);
    // the scans the launch above could not number (more than CC_MAXC components on a level): exact, slow, usually none
    hipLaunchKernelGGL(cc_k_contours_big, dim3(nb < S.n_bigslots ? nb : S.n_bigslots), dim3(CC_K2_BLOCK), c->lds2, stream, c->dcfg,
                       (const float *)S.d_bev, (const float2 *)S.d_pix, (const cc_k1_scan_out *)S.d_k1, S.d_bigslots, S.d_bigq, d_out + b0, lab);
    if (pe) HIPCHK(hipEventRecord(pe[2], stream));
    HIPCHK(hipGetLastError());
    if (dbg && dbg->d_bev)
      HIPCHK(hipMemcpyAsync(dbg->d_bev + (size_t)b0 * nc, S.d_bev, sizeof(float) * nc * nb, hipMemcpyDeviceToDevice, stream));
    if (dbg && dbg->d_pix_rc)
      HIPCHK(hipMemcpyAsync(dbg->d_pix_rc + (size_t)b0 * nc * 2, S.d_pix, sizeof(float2) * nc * nb, hipMemcpyDeviceToDevice, stream));
  }
  if (n_scans > 0) {
    HIPCHK(hipEventRecord(S.ev_last, stream));
    S.last_stream = stream;
    S.has_last = true;
  }
  return CC_OK;
}


int cc_ingest_batch(cc_ctx *c, const float *d_xyzi, const int64_t *h_offsets, int n_scans, cc_scan_desc_t *d_out,
                    const cc_ingest_debug_t *dbg, void *stream_) {
  if (!c || !d_xyzi || !h_offsets || !d_out || n_scans < 0) return set_err(CC_EINVAL, "cc_ingest_batch: bad argument");
  std::lock_guard<std::recursive_mutex> ing_lk(c->ing_mu);  // offsets ring, K1/K2 scratch, ev_last: one call at a time
  return ingest_on(c, c->main, k1_points(d_xyzi, nullptr, nullptr), h_offsets, n_scans, d_out, dbg, (hipStream_t)stream_, "cc_ingest_batch");
}

// The body of the device forms: the check, then the call itself on the context's own scratch set.
static int ingest_device(cc_ctx *c, k1_source src, const int64_t *h_offsets, int n_scans, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream_,
                         const char *who) {
  const int rc = k1_check(c, src, K1_DEVICE, h_offsets, n_scans, d_out, who);
  if (rc != CC_OK || n_scans == 0) return rc;  // (no scans: nothing to queue)
  std::lock_guard<std::recursive_mutex> ing_lk(c->ing_mu);
  return ingest_on(c, c->main, src, k1_offsets(src, h_offsets), n_scans, d_out, dbg, (hipStream_t)stream_, who);
}

// the results of a host call back to the host (blocking copies: they wait for the call's kernels); CC_ECAPACITY for an inexact descriptor
static int host_results(const cc_scan_desc_t *d_o, const float *d_b, size_t bev_bytes, int n_scans, cc_scan_desc_t *h_out, float *h_bev, const char *who) {
  hipError_t e = hipMemcpy(h_out, d_o, sizeof(cc_scan_desc_t) * (size_t)n_scans, hipMemcpyDeviceToHost);
  if (e == hipSuccess && h_bev) e = hipMemcpy(h_bev, d_b, bev_bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return set_err(CC_EHIP, CC_WHO(": D2H"), e);
  for (int i = 0; i < n_scans; i++)
    if (h_out[i].flags & (CC_DESC_INEXACT_COMPONENTS | CC_DESC_INEXACT_KEYS))
      return set_err(CC_ECAPACITY, CC_WHO(": a scan exceeds a fixed capacity of the contour kernel (more than CC_MAXC components on "
                                          "a level, or an over-full key RoI): its descriptor is not exact"));
  return CC_OK;
}

// The body of the *_host forms: the check; device memory for the planned copy of the call's records (the scans' offsets made relative to
// the call's first point), for its descriptors and (h_bev) its images; the planned copies; then the call itself, and the results back.
static int ingest_host(cc_ctx *c, k1_source src, const int64_t *h_offsets, int n_scans, cc_scan_desc_t *h_out, float *h_bev, const char *who) {
  const int rcc = k1_check(c, src, K1_HOST, h_offsets, n_scans, h_out, who);
  if (rcc != CC_OK || n_scans == 0) return rcc;  // (an IMAGES call of no scans)
  HIPCHK(hipSetDevice(c->device));
  h_offsets = k1_offsets(src, h_offsets);
  std::vector<int64_t> off(n_scans + 1);
  for (int i = 0; i <= n_scans; i++) off[i] = h_offsets[i] - h_offsets[0];
  const k1_host_plan plan = k1_plan(src, K1_HOST, h_offsets[0], off[n_scans]);
  const size_t bev_bytes = sizeof(float) * (size_t)c->dcfg.n_cell * (size_t)n_scans;
  char *d_x = nullptr;
  float *d_b = nullptr;
  cc_scan_desc_t *d_o = nullptr;
  HIPCHK(hipMalloc(&d_x, plan.total));
  hipError_t e = hipMalloc(&d_o, sizeof(cc_scan_desc_t) * (size_t)n_scans);
  if (e == hipSuccess && h_bev) e = hipMalloc(&d_b, bev_bytes);
  if (e != hipSuccess) {
    hipFree(d_x);
    hipFree(d_o);
    return set_err(CC_EHIP, CC_WHO(": hipMalloc"), e);
  }
  cc_ingest_debug_t dbg;
  dbg.d_bev = d_b;
  dbg.d_pix_rc = nullptr;
  dbg.d_labels = nullptr;
  if (plan.zero_out) e = hipMemsetAsync(d_o, 0, sizeof(cc_scan_desc_t) * (size_t)n_scans, nullptr);
  for (size_t k = 0; k < plan.copies.size() && e == hipSuccess; k++)
    e = hipMemcpy(d_x + plan.copies[k].at, plan.copies[k].from, plan.copies[k].bytes, hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? CC_OK : set_err(CC_EHIP, CC_WHO(": H2D"), e);
  if (rc == CC_OK) {
    k1_rebase(src, plan, d_x);
    std::lock_guard<std::recursive_mutex> ing_lk(c->ing_mu);
    rc = ingest_on(c, c->main, src, off.data(), n_scans, d_o, h_bev ? &dbg : nullptr, nullptr, who);
  }
  if (rc == CC_OK) rc = host_results(d_o, d_b, bev_bytes, n_scans, h_out, h_bev, who);
  hipFree(d_x);
  hipFree(d_o);
  hipFree(d_b);
  return rc;
}

int cc_ingest_host(cc_ctx *c, const float *h_xyzi, const int64_t *h_offsets, int n_scans, cc_scan_desc_t *h_out) {
  return cc_ingest_host_bev(c, h_xyzi, h_offsets, n_scans, h_out, nullptr);
}

int cc_ingest_points(cc_ctx *c, const void *d_points, const cc_point_layout_t *layout, const int64_t *h_offsets, int n_scans, const float *h_tf,
                     cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_points(d_points, layout, h_tf), h_offsets, n_scans, d_out, dbg, stream_, "cc_ingest_points");
}

int cc_ingest_host_bev(cc_ctx *c, const float *h_xyzi, const int64_t *h_offsets, int n_scans, cc_scan_desc_t *h_out, float *h_bev) {
  return ingest_host(c, k1_points(h_xyzi, nullptr, nullptr), h_offsets, n_scans, h_out, h_bev, "cc_ingest_host");
}

int cc_ingest_points_host(cc_ctx *c, const void *h_points, const cc_point_layout_t *layout, const int64_t *h_offsets, int n_scans, const float *h_tf,
                          cc_scan_desc_t *h_out, float *h_bev) {
  return ingest_host(c, k1_points(h_points, layout, h_tf), h_offsets, n_scans, h_out, h_bev, "cc_ingest_points_host");
}

// ---- a sweep de-skewed by per-point time (cc_ingest_points_motion and its siblings) ----
int cc_ingest_points_motion(cc_ctx *c, const void *d_points, const cc_point_layout_t *layout, const cc_point_motion_t *motion, const int64_t *h_offsets,
                            int n_scans, const float *h_time, const float *h_knots, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_motion(d_points, layout, motion, h_time, h_knots), h_offsets, n_scans, d_out, dbg, stream_, "cc_ingest_points_motion");
}

int cc_ingest_points_motion_host(cc_ctx *c, const void *h_points, const cc_point_layout_t *layout, const cc_point_motion_t *motion, const int64_t *h_offsets,
                                 int n_scans, const float *h_time, const float *h_knots, cc_scan_desc_t *h_out, float *h_bev) {
  const char *who = "cc_ingest_points_motion_host";
  if (!motion) return set_err(CC_EINVAL, CC_WHO(": motion, h_time and h_knots must not be NULL"));
  return ingest_host(c, k1_motion(h_points, layout, motion, h_time, h_knots), h_offsets, n_scans, h_out, h_bev, who);
}

// ---- records dropped by a word of their own (include/cont2_amd_filter.h) ----
int cc_ingest_points_filtered(cc_ctx *c, const void *d_points, const cc_point_layout_t *layout, const cc_point_filter_t *filter, const int64_t *h_offsets,
                              int n_scans, const float *h_tf, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_filtered(d_points, layout, h_tf, filter), h_offsets, n_scans, d_out, dbg, stream_, "cc_ingest_points_filtered");
}

int cc_ingest_points_filtered_host(cc_ctx *c, const void *h_points, const cc_point_layout_t *layout, const cc_point_filter_t *filter, const int64_t *h_offsets,
                                   int n_scans, const float *h_tf, cc_scan_desc_t *h_out, float *h_bev) {
  return ingest_host(c, k1_filtered(h_points, layout, h_tf, filter), h_offsets, n_scans, h_out, h_bev, "cc_ingest_points_filtered_host");
}

// ---- f64, scaled-i32 and split-stream coordinates (include/cont2_amd_coords.h) ----
int cc_ingest_coords(cc_ctx *c, const cc_coord_src_t *src, const int64_t *h_offsets, int n_scans, const double *h_origin, const float *h_tf, cc_scan_desc_t *d_out,
                     const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_coords(src, h_origin, h_tf), h_offsets, n_scans, d_out, dbg, stream_, "cc_ingest_coords");
}

int cc_ingest_coords_host(cc_ctx *c, const cc_coord_src_t *src, const int64_t *h_offsets, int n_scans, const double *h_origin, const float *h_tf,
                          cc_scan_desc_t *h_out, float *h_bev) {
  return ingest_host(c, k1_coords(src, h_origin, h_tf), h_offsets, n_scans, h_out, h_bev, "cc_ingest_coords_host");
}

// ---- a sensor's range image rasterised in place (cc_ingest_ranges and its siblings) ----
int cc_range_sensor_create(cc_ctx *c, const cc_range_model_t *m, cc_range_sensor **out) {
  const char *who = "cc_range_sensor_create";
  if (!c || !m || !out) return set_err(CC_EINVAL, CC_WHO(": bad argument"));
  const char *why = nullptr;
  const long long hw = (long long)m->n_rows * (long long)m->n_cols;
  if (m->n_rows < 1 || m->n_rows > CC_RANGE_ROWS_MAX) why = "n_rows must be 1 .. CC_RANGE_ROWS_MAX";
  else if (m->n_cols < 1 || m->n_cols > CC_RANGE_COLS_MAX) why = "n_cols must be 1 .. CC_RANGE_COLS_MAX";
  else if (!(hw > 10)) why = "an image with <= 10 pixels (CHECK_GT(size, 10), contour_mng.h:507)";
  else if (hw >= (1 << CC_K1_IDX_BITS)) why = "an image with >= 2^21 pixels";
  else if (m->word_type != CC_RANGE_U16 && m->word_type != CC_RANGE_U32 && m->word_type != CC_RANGE_F32) why = "word_type must be CC_RANGE_U16, _U32 or _F32";
  else if (m->order != CC_RANGE_ROW_MAJOR && m->order != CC_RANGE_COL_MAJOR) why = "order must be CC_RANGE_ROW_MAJOR or CC_RANGE_COL_MAJOR";
  else if (!std::isfinite(m->range_scale) || !std::isfinite(m->origin_n) || !std::isfinite(m->origin_z)) why = "range_scale, origin_n and origin_z must be finite";
  else if (m->n_knots < 0 || m->n_knots > CC_MOTION_KNOTS_MAX) why = "n_knots must be 0 .. CC_MOTION_KNOTS_MAX";
  else if (!m->row_tab || !m->col_cos_sin) why = "row_tab and col_cos_sin must not be NULL";
  else if (m->col_knot)
    for (int i = 0; i < m->n_cols; i++)
      if (m->col_knot[i] < 0 || m->col_knot[i] > (m->n_knots > 0 ? m->n_knots - 1 : 0)) why = "every col_knot must be in [0, K - 1] (K = 0: 0)";
  if (why) return set_err(CC_EINVAL, CC_WHO((std::string(": ") + why)));
  HIPCHK(hipSetDevice(c->device));
  // device layout: one float4 per row (the model's four values) and ONE float4 per column (cos, sin, the knot's bits, 0): a pixel's
  // column data is one aligned 16-byte load
  std::vector<float4> rows(m->n_rows), cols(m->n_cols);
  for (int i = 0; i < m->n_rows; i++) rows[i] = make_float4(m->row_tab[4 * i], m->row_tab[4 * i + 1], m->row_tab[4 * i + 2], m->row_tab[4 * i + 3]);
  for (int i = 0; i < m->n_cols; i++) {
    const int32_t k = m->col_knot ? m->col_knot[i] : 0;
    float kb;
    memcpy(&kb, &k, 4);
    cols[i] = make_float4(m->col_cos_sin[2 * i], m->col_cos_sin[2 * i + 1], kb, 0.f);
  }
  cc_range_sensor *s = new cc_range_sensor();
  s->ctx = c;
  s->device = c->device;
  s->word_type = m->word_type;
  s->word_bytes = m->word_type == CC_RANGE_U16 ? 2 : 4;
  hipError_t e = hipMalloc(&s->d_row, sizeof(float4) * rows.size());
  if (e == hipSuccess) e = hipMalloc(&s->d_col, sizeof(float4) * cols.size());
  if (e == hipSuccess) e = hipMemcpy(s->d_row, rows.data(), sizeof(float4) * rows.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->d_col, cols.data(), sizeof(float4) * cols.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    hipFree(s->d_row);
    hipFree(s->d_col);
    delete s;
    return set_err(CC_EHIP, CC_WHO(": the sensor's tables"), e);
  }
  cc_k1_range &kr = s->kr;
  kr.words = nullptr;
  kr.row = s->d_row;
  kr.col = s->d_col;
  kr.knots = nullptr;
  kr.n_rows = m->n_rows;
  kr.n_cols = m->n_cols;
  kr.col_major = m->order == CC_RANGE_COL_MAJOR ? 1 : 0;
  // j / D on the device (k_rasterize.h has the proof): a shift for a power of two, else the product with ceil(2^33 / D) >> 33
  const unsigned D = (unsigned)(kr.col_major ? m->n_rows : m->n_cols);
  kr.div_shift = -1;
  kr.div_magic = 0;
  if ((D & (D - 1)) == 0) {
    kr.div_shift = 0;
    while ((1u << kr.div_shift) < D) kr.div_shift++;
  } else {
    kr.div_magic = (unsigned)(((1ull << CC_K1_RNG_MAGIC_SHIFT) + D - 1) / D);  // D >= 3: below 2^32
  }
  kr.n_knots = m->n_knots;
  kr.range_scale = m->range_scale;
  kr.origin_n = m->origin_n;
  kr.origin_z = m->origin_z;
  *out = s;
  return CC_OK;
}

int cc_range_sensor_destroy(cc_range_sensor *s) {
  if (!s) return CC_OK;
  hipSetDevice(s->device);
  hipFree(s->d_row);
  hipFree(s->d_col);
  delete s;
  return CC_OK;
}

int cc_ingest_ranges(cc_ctx *c, const cc_range_sensor *sensor, const void *d_ranges, int n_scans, const float *h_knots, cc_scan_desc_t *d_out,
                     const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_ranges(sensor, d_ranges, h_knots), nullptr, n_scans, d_out, dbg, stream_, "cc_ingest_ranges");
}

int cc_ingest_ranges_host(cc_ctx *c, const cc_range_sensor *sensor, const void *h_ranges, int n_scans, const float *h_knots, cc_scan_desc_t *h_out,
                          float *h_bev) {
  return ingest_host(c, k1_ranges(sensor, h_ranges, h_knots), nullptr, n_scans, h_out, h_bev, "cc_ingest_ranges_host");
}

// ---- descriptors from caller-made max-height images (include/cont2_amd_images.h) ----
int cc_ingest_images(cc_ctx *c, const float *d_height, const float *d_pos_rc, int n_scans, const float *h_min_height, cc_scan_desc_t *d_out,
                     const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_images(d_height, d_pos_rc, h_min_height), nullptr, n_scans, d_out, dbg, stream_, "cc_ingest_images");
}

int cc_ingest_images_host(cc_ctx *c, const float *h_height, const float *h_pos_rc, int n_scans, const float *h_min_height, cc_scan_desc_t *h_out,
                          float *h_bev) {
  return ingest_host(c, k1_images(h_height, h_pos_rc, h_min_height), nullptr, n_scans, h_out, h_bev, "cc_ingest_images_host");
}

// SO(3) in f64 for cc_motion_knots: R row-major 3 x 3.
static void so3_log(const double R[9], double w[3]) {
  const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};  // sin(theta) * axis
  const double sn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), cs = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double th = atan2(sn, cs);
  if (sn > 1e-9) {
    for (int i = 0; i < 3; i++) w[i] = v[i] * (th / sn);
  } else if (cs > 0) {  // theta ~ 0: Log(R) ~ vee(R - R^T) / 2
    for (int i = 0; i < 3; i++) w[i] = v[i];
  } else {  // theta ~ pi: the axis from the diagonal of (R + I) / 2 = a a^T, signs from its largest column
    const double d[3] = {0.5 * (R[0] + 1.0), 0.5 * (R[4] + 1.0), 0.5 * (R[8] + 1.0)};
    const int k = d[0] >= d[1] && d[0] >= d[2] ? 0 : (d[1] >= d[2] ? 1 : 2);
    double a[3];
    for (int i = 0; i < 3; i++) a[i] = 0.25 * (R[3 * i + k] + R[3 * k + i]) + (i == k ? 0.5 : 0.0);
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int i = 0; i < 3; i++) w[i] = a[i] / n * th;
  }
}
static void so3_exp(const double w[3], double R[9]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
  const double A = th > 1e-8 ? sin(th) / th : 1.0 - th2 / 6.0, B = th > 1e-8 ? (1.0 - cos(th)) / th2 : 0.5 - th2 / 24.0;
  const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double ww = 0;
      for (int k = 0; k < 3; k++) ww += W[3 * i + k] * W[3 * k + j];
      R[3 * i + j] = (i == j ? 1.0 : 0.0) + A * W[3 * i + j] + B * ww;
    }
}

void cc_motion_knots(const double pb[12], const double pe[12], double ref, int K, float *knots) {
  if (!pb || !pe || !knots || K < 1) return;
  double D[9], w[3];  // R_b^T R_e and its logarithm
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double a = 0;
      for (int k = 0; k < 3; k++) a += pb[4 * k + i] * pe[4 * k + j];
      D[3 * i + j] = a;
    }
  so3_log(D, w);
  auto pose = [&](double s, double T[12]) {  // T(s)
    const double ws[3] = {s * w[0], s * w[1], s * w[2]};
    double E[9];
    so3_exp(ws, E);
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) {
        double a = 0;
        for (int k = 0; k < 3; k++) a += pb[4 * i + k] * E[3 * k + j];
        T[4 * i + j] = a;
      }
      T[4 * i + 3] = (1.0 - s) * pb[4 * i + 3] + s * pe[4 * i + 3];
    }
  };
  double Tr[12];
  pose(ref, Tr);
  for (int q = 0; q < K; q++) {
    double Tk[12];
    pose((q + 0.5) / K, Tk);
    for (int i = 0; i < 3; i++) {  // T(ref)^-1 T_k = [Rr^T Rk | Rr^T (pk - pr)]
      for (int j = 0; j < 3; j++) {
        double a = 0;
        for (int k = 0; k < 3; k++) a += Tr[4 * k + i] * Tk[4 * k + j];
        knots[(size_t)q * 12 + 4 * i + j] = (float)a;
      }
      double a = 0;
      for (int k = 0; k < 3; k++) a += Tr[4 * k + i] * (Tk[4 * k + 3] - Tr[4 * k + 3]);
      knots[(size_t)q * 12 + 4 * i + 3] = (float)a;
    }
  }
}

// ---- scans made of segments (cc_ingest_segments and its siblings) ----
int cc_ingest_segments(cc_ctx *c, const cc_point_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, cc_scan_desc_t *d_out,
                       const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_segments(h_segs, h_scan_segs), nullptr, n_scans, d_out, dbg, stream_, "cc_ingest_segments");
}

int cc_ingest_segments_host(cc_ctx *c, const cc_point_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, cc_scan_desc_t *h_out, float *h_bev) {
  return ingest_host(c, k1_segments(h_segs, h_scan_segs), nullptr, n_scans, h_out, h_bev, "cc_ingest_segments_host");
}

// ---- a rig's sensors de-skewed, filtered and joined in one sweep (include/cont2_amd_rig.h) ----
int cc_ingest_rig(cc_ctx *c, const cc_rig_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, const float *h_knots, int n_pool,
                  const cc_point_filter_t *filter, cc_scan_desc_t *d_out, const cc_ingest_debug_t *dbg, void *stream_) {
  return ingest_device(c, k1_rig(h_segs, h_scan_segs, h_knots, n_pool, filter), nullptr, n_scans, d_out, dbg, stream_, "cc_ingest_rig");
}

int cc_ingest_rig_host(cc_ctx *c, const cc_rig_segment_t *h_segs, const int32_t *h_scan_segs, int n_scans, const float *h_knots, int n_pool,
                       const cc_point_filter_t *filter, cc_scan_desc_t *h_out, float *h_bev) {
  return ingest_host(c, k1_rig(h_segs, h_scan_segs, h_knots, n_pool, filter), nullptr, n_scans, h_out, h_bev, "cc_ingest_rig_host");
}

void cc_est_sens_tf(const double tf_bev[3], int n_row, int n_col, double tf_sens[3]) {
  // T_to_tsen^-1 * T_delta * T_so_ssen with T_so_ssen = translate(n_row/2 - 0.5, n_col/2 - 0.5)
  const double ox = n_row / 2 - 0.5, oy = n_col / 2 - 0.5;
  const double c = cos(tf_bev[2]), s = sin(tf_bev[2]);
  tf_sens[0] = c * ox - s * oy + tf_bev[0] - ox;
  tf_sens[1] = s * ox + c * oy + tf_bev[1] - oy;
  tf_sens[2] = tf_bev[2];
}

void cc_est_sens_info(const double hess_bev[6], const double tf_bev[3], int n_row, int n_col, double hess_sens[6]) {
  // J = [1 0 a; 0 1 b; 0 0 1] with (a, b) = dR/dtheta * (ox, oy), so J^-1 = [1 0 -a; 0 1 -b; 0 0 1] and J^-T H J^-1 keeps the
  // translation block, shifts the theta column by -(H_xx a + H_xy b, H_xy a + H_yy b) and the corner accordingly
  const double ox = n_row / 2 - 0.5, oy = n_col / 2 - 0.5;
  const double c = cos(tf_bev[2]), s = sin(tf_bev[2]);
  const double a = -s * ox - c * oy, b = c * ox - s * oy;
  const double xx = hess_bev[0], xy = hess_bev[1], xt = hess_bev[2], yy = hess_bev[3], yt = hess_bev[4], tt = hess_bev[5];
  const double nxt = xt - (xx * a + xy * b), nyt = yt - (xy * a + yy * b);
  hess_sens[0] = xx;
  hess_sens[1] = xy;
  hess_sens[2] = nxt;
  hess_sens[3] = yy;
  hess_sens[4] = nyt;
  hess_sens[5] = tt - a * xt - b * yt - a * nxt - b * nyt;
}

// ------------------------------------------------------------------------------------------ per-scan loop
struct cc_scan {
  cc_ctx *ctx = nullptr;
  cc_scan_desc_t *d_desc = nullptr;  // device slot (nullptr once offloaded)
  cc_scan_desc_t *h_desc = nullptr;  // host copy (malloc), fetched on demand
  hipEvent_t ready = nullptr;        // recorded on the ingest stream behind the scan's last kernel / copy
  float *h_bev = nullptr;            // host copy of the max-height image, if it was asked for
  bool bev_pending = false;
};

// n descriptor slots of the pool to out[]; all or none: when the pool cannot grow, the slots taken so far go back.
// The pool grows geometrically (64, 64, 128, 256, ... up to 1 024 slots = 169 MB per block): a hipMalloc synchronises the
// device, and a driver that keeps thousands of scans resident should not pay that every 64 scans of its loop.
static hipError_t slot_take(cc_ctx *c, int n, cc_scan_desc_t **out) {
  std::lock_guard<std::mutex> lk(c->slot_mu);
  for (int i = 0; i < n; i++) {
    if (c->slot_free.empty()) {
      size_t have = 0;
      for (size_t b = 0; b < c->slot_blocks.size(); b++) have += c->slot_block_n[b];
      const int nblk = (int)(have < 64 ? 64 : (have > 1024 ? 1024 : have));
      cc_scan_desc_t *blk = nullptr;
      const hipError_t e_ = hipMalloc(&blk, sizeof(cc_scan_desc_t) * nblk);
      if (e_ != hipSuccess) {
        for (int k = 0; k < i; k++) c->slot_free.push_back(out[k]);
        return e_;
      }
      c->slot_blocks.push_back(blk);
      c->slot_block_n.push_back(nblk);
      for (int k = nblk - 1; k >= 0; k--) c->slot_free.push_back(blk + k);
    }
    out[i] = c->slot_free.back();
    c->slot_free.pop_back();
  }
  return hipSuccess;
}

static int loop_reserve_points(cc_ctx *c, int64_t n_points) {  // ing_mu held
  if (!c->s_loop) HIPCHK(stream_take(c->device, &c->s_loop));
  for (auto &ch : c->chan) {
    if (!ch.s) HIPCHK(stream_take(c->device, &ch.s));
    if (ch.scr.cap == 0) {
      const int rc = scratch_alloc(c, ch.scr, 1, 1);
      if (rc != CC_OK) return rc;
    }
  }
  if (n_points <= c->pts_cap) return CC_OK;
  // growing re-allocates every slot: none may be in another thread's hands (being filled) at that moment
  const std::thread::id me = std::this_thread::get_id();
  for (int i = 0; i < cc_ctx::NPTS; i++)
    if (c->pts_handed[i] && c->pts_owner[i] != me)
      return set_err(CC_EINVAL, "cc_stage_points: the staging buffers must grow while another thread fills one of them (stage the largest "
                                "scan first, or give every thread its own context)");
  for (auto &ch : c->chan) HIPCHK(hipStreamSynchronize(ch.s));
  for (int i = 0; i < cc_ctx::NPTS; i++) {
    if (c->h_pts[i]) hipHostFree(c->h_pts[i]);
    c->h_pts[i] = nullptr;
    c->pts_busy[i] = false;
    c->pts_handed[i] = false;
  }
  for (auto &ch : c->chan) {
    hipFree(ch.d_pts);
    ch.d_pts = nullptr;
    ch.d_pts_cap = 0;
  }
  // a quarter more than was asked for (a sequence's scans differ by a few per cent: the buffers should not grow twice), at least
  // 64 K points; pinned memory costs ~0.2-0.6 ms per MB to allocate, so not readKITTIPointCloudBin's 1 M floats up front
  c->pts_cap = n_points + n_points / 4;
  if (c->pts_cap < 65536) c->pts_cap = 65536;
  c->pts_cap = (c->pts_cap + 4095) / 4096 * 4096;
  for (auto &ch : c->chan) {
    HIPCHK(hipMalloc(&ch.d_pts, sizeof(float) * 4 * (size_t)c->pts_cap));
    ch.d_pts_cap = c->pts_cap;
  }
  return CC_OK;
}
// a slot's pinned buffer (pts_cap points) and copy event exist from its first use on
static int loop_slot_alloc(cc_ctx *c, int slot) {  // ing_mu held
  if (!c->pts_ev[slot]) HIPCHK(hipEventCreateWithFlags(&c->pts_ev[slot], hipEventDisableTiming));
  if (!c->h_pts[slot]) HIPCHK(hipHostMalloc((void **)&c->h_pts[slot], sizeof(float) * 4 * (size_t)c->pts_cap, hipHostMallocDefault));
  return CC_OK;
}

// ing_mu held by `lk`.  Hands slot `slot` to the calling thread: waits while another thread holds it, then for the slot's
// last H2D copy (that copy, not the stream).
static float *stage_slot_locked(cc_ctx *c, int64_t n_points, int slot, std::unique_lock<std::recursive_mutex> &lk) {
  const std::thread::id me = std::this_thread::get_id();
  c->pts_cv.wait(lk, [&] { return !c->pts_handed[slot] || c->pts_owner[slot] == me; });
  if (hipSetDevice(c->device) != hipSuccess) return nullptr;
  if (loop_reserve_points(c, n_points) != CC_OK) return nullptr;
  if (loop_slot_alloc(c, slot) != CC_OK) return nullptr;
  if (c->pts_busy[slot]) {
    if (hipEventSynchronize(c->pts_ev[slot]) != hipSuccess) return nullptr;
    c->pts_busy[slot] = false;
  }
  c->pts_handed[slot] = true;
  c->pts_owner[slot] = me;
  return c->h_pts[slot];
}

float *cc_stage_points_slot(cc_ctx *c, int64_t n_points, int slot) {
  if (!c || n_points < 1 || slot < 0 || slot >= cc_ctx::OWN_SLOT) return nullptr;
  std::unique_lock<std::recursive_mutex> lk(c->ing_mu);
  return stage_slot_locked(c, n_points, slot, lk);
}
float *cc_stage_points(cc_ctx *c, int64_t n_points) {
  if (!c || n_points < 1) return nullptr;
  std::unique_lock<std::recursive_mutex> lk(c->ing_mu);
  return stage_slot_locked(c, n_points, cc_ctx::OWN_SLOT, lk);
}

int cc_stage_points_cancel(cc_ctx *c, const float *staged) {
  if (!c || !staged) return set_err(CC_EINVAL, "cc_stage_points_cancel: bad argument");
  std::unique_lock<std::recursive_mutex> lk(c->ing_mu);
  for (int i = 0; i < cc_ctx::NPTS; i++)
    if (c->h_pts[i] == staged) {
      if (!c->pts_handed[i] || c->pts_owner[i] != std::this_thread::get_id())
        return set_err(CC_EINVAL, "cc_stage_points_cancel: the buffer is not in this thread's hands");
      c->pts_handed[i] = false;
      c->pts_cv.notify_all();
      return CC_OK;
    }
  return set_err(CC_EINVAL, "cc_stage_points_cancel: not a staging buffer of this context");
}

static int scan_ingest_points(cc_ctx *c, k1_source src, int64_t n_points, int want_bev, cc_scan **out, const char *who);

int cc_scan_ingest(cc_ctx *c, const float *h_xyzi, int64_t n_points, int want_bev, cc_scan **out) {
  return scan_ingest_points(c, k1_points(h_xyzi, nullptr, nullptr), n_points, want_bev, out, "cc_scan_ingest");
}

int cc_scan_ingest_points(cc_ctx *c, const void *h_xyzi, const cc_point_layout_t *layout, int64_t n_points, const float *h_tf, int want_bev, cc_scan **out) {
  return scan_ingest_points(c, k1_points(h_xyzi, layout, h_tf), n_points, want_bev, out, "cc_scan_ingest_points");
}

int cc_scan_ingest_segments(cc_ctx *c, const cc_point_segment_t *h_segs, int n_segs, int want_bev, cc_scan **out) {
  const int32_t scan_segs[2] = {0, n_segs};
  return scan_ingest_points(c, k1_segments(h_segs, scan_segs), 0, want_bev, out, "cc_scan_ingest_segments");
}

int cc_scan_ingest_rig(cc_ctx *c, const cc_rig_segment_t *h_segs, int n_segs, const float *h_knots, int n_pool, const cc_point_filter_t *filter, int want_bev,
                       cc_scan **out) {
  const int32_t scan_segs[2] = {0, n_segs};
  return scan_ingest_points(c, k1_rig(h_segs, scan_segs, h_knots, n_pool, filter), 0, want_bev, out, "cc_scan_ingest_rig");
}

int cc_scan_ingest_points_motion(cc_ctx *c, const void *h_points, const cc_point_layout_t *layout, const cc_point_motion_t *motion, int64_t n_points,
                                 const float *h_time, const float *h_knots, int want_bev, cc_scan **out) {
  if (!motion) return set_err(CC_EINVAL, "cc_scan_ingest_points_motion: motion, h_time and h_knots must not be NULL");
  return scan_ingest_points(c, k1_motion(h_points, layout, motion, h_time, h_knots), n_points, want_bev, out, "cc_scan_ingest_points_motion");
}

int cc_scan_ingest_points_filtered(cc_ctx *c, const void *h_points, const cc_point_layout_t *layout, const cc_point_filter_t *filter, int64_t n_points,
                                   const float *h_tf, int want_bev, cc_scan **out) {
  if (!filter) return set_err(CC_EINVAL, "cc_scan_ingest_points_filtered: filter must not be NULL");
  return scan_ingest_points(c, k1_filtered(h_points, layout, h_tf, filter), n_points, want_bev, out, "cc_scan_ingest_points_filtered");
}

int cc_scan_ingest_coords(cc_ctx *c, const cc_coord_src_t *src, int64_t n_points, const double *origin, const float *h_tf, int want_bev, cc_scan **out) {
  return scan_ingest_points(c, k1_coords(src, origin, h_tf), n_points, want_bev, out, "cc_scan_ingest_coords");
}

// (a range image's and a height image's size is the sensor's and the context's: k1_check has it)
int cc_scan_ingest_ranges(cc_ctx *c, const cc_range_sensor *sensor, const void *h_ranges, const float *h_knots, int want_bev, cc_scan **out) {
  return scan_ingest_points(c, k1_ranges(sensor, h_ranges, h_knots), 0, want_bev, out, "cc_scan_ingest_ranges");
}

int cc_scan_ingest_image(cc_ctx *c, const float *h_height, const float *h_pos_rc, const float *h_min_height, int want_bev, cc_scan **out) {
  return scan_ingest_points(c, k1_images(h_height, h_pos_rc, h_min_height), 0, want_bev, out, "cc_scan_ingest_image");
}

// The staging slots of a per-scan call go back to the threads waiting for them when the call ends, however it ends: from where this
// stands on the buffers are no longer the caller's.
struct stage_return {
  cc_ctx *c;
  const int *slot;
  int n;
  ~stage_return() {
    for (int i = 0; i < n; i++) c->pts_handed[slot[i]] = false;
    c->pts_cv.notify_all();
  }
};
// The freshly taken descriptor slots of a per-scan call and their cc_scan handles.  Unless the call has handed them to its caller
// (ready), the slots go back to the pool and the handles are freed, with their events and images.
struct scan_hold {
  cc_ctx *c;
  cc_scan *sc[CC_SCAN_BATCH_MAX] = {};
  int n = 0;
  int take(int n_take, const char *who) {  // all or none
    cc_scan_desc_t *d[CC_SCAN_BATCH_MAX];
    const hipError_t e_ = slot_take(c, n_take, d);
    if (e_ != hipSuccess) return set_err(CC_EHIP, CC_WHO(": descriptor slots"), e_);
    for (; n < n_take; n++) {
      sc[n] = new cc_scan();
      sc[n]->ctx = c;
      sc[n]->d_desc = d[n];
    }
    return CC_OK;
  }
  // The handles' ready events behind everything the call queued on `s` (e_: what queueing the last of it gave), then the handles to
  // out[].  On a failure the stream is drained: the queued kernels write the slots that go back.
  int ready(hipError_t e_, hipStream_t s, const char *what, const char *who, cc_scan **out) {
    for (int i = 0; i < n && e_ == hipSuccess; i++) {
      e_ = hipEventCreateWithFlags(&sc[i]->ready, hipEventDisableTiming);
      if (e_ == hipSuccess) e_ = hipEventRecord(sc[i]->ready, s);
    }
    if (e_ != hipSuccess) {
      hipStreamSynchronize(s);
      return set_err(CC_EHIP, (std::string(who) + what).c_str(), e_);
    }
    for (int i = 0; i < n; i++) out[i] = sc[i];
    n = 0;
    return CC_OK;
  }
  ~scan_hold() {
    {
      std::lock_guard<std::mutex> slk(c->slot_mu);
      for (int i = 0; i < n; i++) c->slot_free.push_back(sc[i]->d_desc);
    }
    for (int i = 0; i < n; i++) {
      if (sc[i]->ready) hipEventDestroy(sc[i]->ready);
      free(sc[i]->h_bev);
      delete sc[i];
    }
  }
};

// One scan of the per-scan loop.  src: the caller's arguments with HOST addresses; n_points: the caller's count where the source has
// none of its own.  The planned copies go through the context's own staging slot to the channel's point buffer -- unless the records
// are a staging buffer that cc_stage_points* handed out, which travels as it is.
static int scan_ingest_points(cc_ctx *c, k1_source src, int64_t n_points, int want_bev, cc_scan **out, const char *who) {
  int64_t off[2] = {0, n_points};
  const int rcc = k1_check(c, src, K1_SCAN, off, 1, out, who);
  if (rcc != CC_OK) return rcc;
  off[1] = k1_offsets(src, off)[1];
  const k1_host_plan plan = k1_plan(src, K1_SCAN, 0, off[1]);
  const int64_t n_stage = (int64_t)((plan.total + 15) / 16);  // the buffers are counted in 16-byte points
  std::unique_lock<std::recursive_mutex> lk(c->ing_mu);  // d_pts, the slots, the scratch behind cc_ingest_batch
  HIPCHK(hipSetDevice(c->device));
  int slot = -1;
  for (int i = 0; i < cc_ctx::NPTS; i++)
    if (c->h_pts[i] && plan.staged == c->h_pts[i]) slot = i;
  if (slot < 0) {
    float *dst = stage_slot_locked(c, n_stage, cc_ctx::OWN_SLOT, lk);  // waits for the slot's holder and its previous copy, grows the buffers if need be
    if (!dst) return set_err(CC_EHIP, CC_WHO(": staging buffer"));
    for (const k1_host_plan::copy &cp : plan.copies) memcpy((char *)dst + cp.at, cp.from, cp.bytes);
    slot = cc_ctx::OWN_SLOT;
  } else if (!c->pts_handed[slot] || c->pts_owner[slot] != std::this_thread::get_id()) {
    return set_err(CC_EINVAL, CC_WHO(": the staging buffer was not handed to this thread by cc_stage_points* (or was ingested already)"));
  } else if (n_stage > c->pts_cap) {
    return set_err(CC_EINVAL, CC_WHO(": more points than were staged"));
  }
  // whatever happens below, the buffer is no longer the caller's: the next thread waiting for the slot may have it once this
  // call has queued (or given up on) the copy
  const stage_return hb{c, &slot, 1};
  // The scan goes to the next channel: its own stream, device point buffer and one-scan scratch set, so that it can run next to
  // the scan before it (a caller may ingest scans i + 1, i + 2 -- from a helper thread, as the evaluator mirror does -- while scan i
  // is queried and added on the loop stream); whoever reads the descriptor waits for `ready`.
  cc_ctx::Channel &ch = c->chan[c->chan_next];
  c->chan_next = (c->chan_next + 1) % cc_ctx::NCHAN;
  if (want_bev && !ch.d_bev_copy) HIPCHK(hipMalloc(&ch.d_bev_copy, sizeof(float) * (size_t)c->dcfg.n_cell));
  HIPCHK(hipMemcpyAsync(ch.d_pts, c->h_pts[slot], plan.total, hipMemcpyHostToDevice, ch.s));
  HIPCHK(hipEventRecord(c->pts_ev[slot], ch.s));
  c->pts_busy[slot] = true;
  scan_hold hold{c};  // from here on every failure path gives the handle and its descriptor slot back
  const int rct = hold.take(1, who);
  if (rct != CC_OK) return rct;
  cc_scan *sc = hold.sc[0];
  cc_ingest_debug_t dbg;
  dbg.d_bev = want_bev ? ch.d_bev_copy : nullptr;
  dbg.d_pix_rc = nullptr;
  dbg.d_labels = nullptr;
  if (plan.zero_out) {
    const hipError_t e_ = hipMemsetAsync(sc->d_desc, 0, sizeof(cc_scan_desc_t), ch.s);
    if (e_ != hipSuccess) return set_err(CC_EHIP, CC_WHO(": hipMemsetAsync"), e_);
  }
  k1_rebase(src, plan, ch.d_pts);
  const int rc = ingest_on(c, ch.scr, src, off, 1, sc->d_desc, want_bev ? &dbg : nullptr, ch.s, who);  // (writes straight into the pool slot)
  if (rc != CC_OK) return rc;
  if (want_bev) {  // the image scratch is shared: bring it over now (asynchronously, into the handle's own buffer)
    sc->h_bev = (float *)malloc(sizeof(float) * (size_t)c->dcfg.n_cell);
    if (!sc->h_bev) return set_err(CC_ENOMEM, CC_WHO(": out of host memory"));
    const hipError_t e_ = hipMemcpyAsync(sc->h_bev, ch.d_bev_copy, sizeof(float) * (size_t)c->dcfg.n_cell, hipMemcpyDeviceToHost, ch.s);
    if (e_ != hipSuccess) return set_err(CC_EHIP, CC_WHO(": copy of the BEV image"), e_);
    sc->bev_pending = true;
  }
  return hold.ready(hipSuccess, ch.s, ": ready event", who, out);
}

// cc_scan_ingest for 1..CC_SCAN_BATCH_MAX staged scans at once: ONE K1/K2 launch chain for all of them on the next channel (a
// single scan's chain takes ~0.2 ms of launch latencies whatever it holds; a loop that reads its files ahead pays that per batch).
// The batch's descriptors are written side by side and then moved to their own slots of the pool by one small kernel, so every
// handle is an ordinary cc_scan afterwards.  All-or-nothing: on an error no handle is returned and every buffer is given back.
struct cc_desc_out_tab {
  cc_scan_desc_t *p[CC_SCAN_BATCH_MAX];
};
#define CC_SCATTER_BLOCKS 16  // workgroups per descriptor
__global__ void __launch_bounds__(256)
cc_k_scatter_desc(cc_desc_out_tab tab, int n, const cc_scan_desc_t *__restrict__ src) {
  const int s = (int)blockIdx.x / CC_SCATTER_BLOCKS, part = (int)blockIdx.x % CC_SCATTER_BLOCKS;
  if (s >= n) return;
  const unsigned long long *__restrict__ in = (const unsigned long long *)(src + s);
  unsigned long long *__restrict__ out = (unsigned long long *)tab.p[s];
  const int nv = (int)(sizeof(cc_scan_desc_t) / 8);
  for (int i = part * 256 + (int)threadIdx.x; i < nv; i += CC_SCATTER_BLOCKS * 256) out[i] = in[i];
}

static int scan_ingest_points_batch(cc_ctx *c, const void *const *h_xyzi, const cc_point_layout_t *layout, const int64_t *n_points, int n, const float *h_tf,
                                    cc_scan **out, const char *who);

int cc_scan_ingest_batch(cc_ctx *c, const float *const *h_xyzi, const int64_t *n_points, int n, cc_scan **out) {
  return scan_ingest_points_batch(c, (const void *const *)h_xyzi, nullptr, n_points, n, nullptr, out, "cc_scan_ingest_batch");
}

int cc_scan_ingest_points_batch(cc_ctx *c, const void *const *h_xyzi, const cc_point_layout_t *layout, const int64_t *n_points, int n, const float *h_tf,
                                cc_scan **out) {
  return scan_ingest_points_batch(c, h_xyzi, layout, n_points, n, h_tf, out, "cc_scan_ingest_points_batch");
}

static int scan_ingest_points_batch(cc_ctx *c, const void *const *h_xyzi, const cc_point_layout_t *layout, const int64_t *n_points, int n, const float *h_tf,
                                    cc_scan **out, const char *who) {
  if (!c || !h_xyzi || !n_points || !out || n < 1 || n > CC_SCAN_BATCH_MAX)
    return set_err(CC_EINVAL, CC_WHO(": bad argument (1..CC_SCAN_BATCH_MAX scans)"));
  cc_point_layout_t lay;
  const int rcl = point_layout(layout, nullptr, who, &lay);  // (staging buffers are aligned)
  if (rcl != CC_OK) return rcl;
  const size_t stride = (size_t)lay.stride_bytes;
  static_assert(sizeof(cc_scan_desc_t) % 8 == 0, "cc_k_scatter_desc copies 8 bytes per lane");
  std::unique_lock<std::recursive_mutex> lk(c->ing_mu);
  HIPCHK(hipSetDevice(c->device));
  const std::thread::id me = std::this_thread::get_id();
  int slot[CC_SCAN_BATCH_MAX];
  int64_t off[CC_SCAN_BATCH_MAX + 1];
  off[0] = 0;
  for (int i = 0; i < n; i++) {
    slot[i] = -1;
    for (int k = 0; k < cc_ctx::NPTS; k++)
      if (c->h_pts[k] && h_xyzi[i] == c->h_pts[k]) slot[i] = k;
    if (slot[i] < 0 || !c->pts_handed[slot[i]] || c->pts_owner[slot[i]] != me)
      return set_err(CC_EINVAL, CC_WHO(": every buffer must be a staging buffer handed to this thread by cc_stage_points*"));
    for (int k = 0; k < i; k++)
      if (slot[k] == slot[i]) return set_err(CC_EINVAL, CC_WHO(": the same staging buffer twice"));
    if (n_points[i] < 1 || (int64_t)(((size_t)n_points[i] * stride + 15) / 16) > c->pts_cap)
      return set_err(CC_EINVAL, CC_WHO(": more points than were staged"));
    if (!(n_points[i] > 10)) return set_err(CC_EINVAL, CC_WHO(": scan with <= 10 points (CHECK_GT(size, 10), contour_mng.h:507)"));
    off[i + 1] = off[i] + n_points[i];
  }
  const stage_return hb{c, slot, n};  // from here on the buffers are no longer the caller's, whatever happens
  cc_ctx::Channel &ch = c->chan[c->chan_next];
  c->chan_next = (c->chan_next + 1) % cc_ctx::NCHAN;
  // the channel's point buffer, scratch set and descriptor row grow to a batch's size the first time a batch comes by
  if (ch.d_pts_cap < (int64_t)((stride * (size_t)off[n] + 15) / 16) || ch.scr.cap < n || !ch.d_desc_tmp) {
    HIPCHK(hipStreamSynchronize(ch.s));
    if (ch.d_pts_cap < (int64_t)CC_SCAN_BATCH_MAX * c->pts_cap) {
      hipFree(ch.d_pts);
      ch.d_pts = nullptr;
      ch.d_pts_cap = 0;
      HIPCHK(hipMalloc(&ch.d_pts, sizeof(float) * 4 * (size_t)c->pts_cap * CC_SCAN_BATCH_MAX));
      ch.d_pts_cap = (int64_t)CC_SCAN_BATCH_MAX * c->pts_cap;
    }
    if (ch.scr.cap < CC_SCAN_BATCH_MAX) {
      scratch_free(ch.scr);
      const int rc = scratch_alloc(c, ch.scr, CC_SCAN_BATCH_MAX, CC_SCAN_BATCH_MAX);
      if (rc != CC_OK) return rc;
    }
    if (!ch.d_desc_tmp) HIPCHK(hipMalloc(&ch.d_desc_tmp, sizeof(cc_scan_desc_t) * CC_SCAN_BATCH_MAX));
  }
  for (int i = 0; i < n; i++) {
    HIPCHK(hipMemcpyAsync((char *)ch.d_pts + stride * (size_t)off[i], c->h_pts[slot[i]], stride * (size_t)n_points[i], hipMemcpyHostToDevice, ch.s));
    HIPCHK(hipEventRecord(c->pts_ev[slot[i]], ch.s));
    c->pts_busy[slot[i]] = true;
  }
  scan_hold hold{c};
  const int rct = hold.take(n, who);
  if (rct != CC_OK) return rct;
  cc_desc_out_tab tab;
  for (int i = 0; i < CC_SCAN_BATCH_MAX; i++) tab.p[i] = i < n ? hold.sc[i]->d_desc : nullptr;
  const int rc = ingest_on(c, ch.scr, k1_points(ch.d_pts, &lay, h_tf), off, n, ch.d_desc_tmp, nullptr, ch.s, who);
  if (rc != CC_OK) return rc;
  hipLaunchKernelGGL(cc_k_scatter_desc, dim3(n * CC_SCATTER_BLOCKS), dim3(256), 0, ch.s, tab, n, (const cc_scan_desc_t *)ch.d_desc_tmp);
  return hold.ready(hipGetLastError(), ch.s, ": launch / ready events", who, out);
}

// 1: the scan's ingest has finished on the device (its descriptor can be read without waiting), 0: still in flight
int cc_scan_ready(const cc_scan *sc) {
  if (!sc) return 0;
  if (!sc->ready) return 1;
  hipSetDevice(sc->ctx->device);
  const hipError_t e_ = hipEventQuery(sc->ready);
  if (e_ != hipSuccess) (void)hipGetLastError();
  return e_ == hipSuccess ? 1 : 0;
}

// the loop stream (or the host) behind the scan's ingest
static int scan_wait_ready(cc_scan *sc, bool host) {
  if (!sc->ready) return CC_OK;
  if (host)
    HIPCHK(hipEventSynchronize(sc->ready));
  else
    HIPCHK(hipStreamWaitEvent(sc->ctx->s_loop, sc->ready, 0));
  return CC_OK;
}

static int scan_fetch(cc_scan *sc) {
  if (sc->h_desc) return CC_OK;
  if (!sc->d_desc) return set_err(CC_EINVAL, "cc_scan: the descriptor is neither on the device nor on the host");
  sc->h_desc = (cc_scan_desc_t *)malloc(sizeof(cc_scan_desc_t));
  if (!sc->h_desc) return set_err(CC_ENOMEM, "cc_scan: out of host memory");
  HIPCHK(hipSetDevice(sc->ctx->device));
  const int rcw = scan_wait_ready(sc, false);
  if (rcw != CC_OK) return rcw;
  HIPCHK(hipMemcpyAsync(sc->h_desc, sc->d_desc, sizeof(cc_scan_desc_t), hipMemcpyDeviceToHost, sc->ctx->s_loop));
  HIPCHK(hipStreamSynchronize(sc->ctx->s_loop));
  sc->bev_pending = false;  // the image copy was queued before `ready`
  return CC_OK;
}

int cc_scan_desc(cc_scan *sc, const cc_scan_desc_t **h_desc) {
  if (!sc || !h_desc) return set_err(CC_EINVAL, "cc_scan_desc: bad argument");
  const int rc = scan_fetch(sc);
  if (rc != CC_OK) return rc;
  *h_desc = sc->h_desc;
  if (sc->h_desc->flags & (CC_DESC_INEXACT_COMPONENTS | CC_DESC_INEXACT_KEYS))
    return set_err(CC_ECAPACITY, "cc_scan_desc: the scan exceeds a fixed capacity of the contour kernel (more than CC_MAXC components on a "
                                 "level, or an over-full key RoI): its descriptor is not exact");
  return CC_OK;
}

int cc_scan_bev(cc_scan *sc, const float **h_bev) {
  if (!sc || !h_bev) return set_err(CC_EINVAL, "cc_scan_bev: bad argument");
  if (!sc->h_bev) return set_err(CC_EINVAL, "cc_scan_bev: the image was not asked for at cc_scan_ingest");
  if (sc->bev_pending) {
    HIPCHK(hipSetDevice(sc->ctx->device));
    const int rcw = scan_wait_ready(sc, true);
    if (rcw != CC_OK) return rcw;
    sc->bev_pending = false;
  }
  *h_bev = sc->h_bev;
  return CC_OK;
}

int cc_scan_offload(cc_scan *sc) {
  if (!sc) return set_err(CC_EINVAL, "cc_scan_offload: bad argument");
  if (!sc->d_desc) return CC_OK;
  const int rc = scan_fetch(sc);
  if (rc != CC_OK) return rc;
  {  // the fetch above synchronised the loop stream: nothing queued reads the slot any more
    std::lock_guard<std::mutex> lk(sc->ctx->slot_mu);
    sc->ctx->slot_free.push_back(sc->d_desc);
  }
  sc->d_desc = nullptr;
  return CC_OK;
}

int cc_scan_on_device(const cc_scan *sc) { return sc && sc->d_desc ? 1 : 0; }

int cc_scan_release(cc_scan *sc) {
  if (!sc) return CC_OK;
  if (sc->d_desc || sc->bev_pending) {
    hipSetDevice(sc->ctx->device);
    if (sc->ready) hipEventSynchronize(sc->ready);               // the ingest may still write the slot / the image
    if (sc->ctx->s_loop) hipStreamSynchronize(sc->ctx->s_loop);  // queued work may still read the slot
    if (sc->d_desc) {
      std::lock_guard<std::mutex> lk(sc->ctx->slot_mu);
      sc->ctx->slot_free.push_back(sc->d_desc);
    }
  }
  if (sc->ready) hipEventDestroy(sc->ready);
  free(sc->h_desc);
  free(sc->h_bev);
  delete sc;
  return CC_OK;
}

#include "cc_db_api.inc"
#include "cc_comm.inc"

}  // extern "C"
