// TEST INFRASTRUCTURE: probe kernels for the pieces every kernel stands on -- the wave / row primitives of csrc/cc_group.h,
// the f64 routines of csrc/cc_fmath.h, cc_gmm_term, the f32 libm / Eigen restatements of csrc/cc_stats.h and the sorts of
// csrc/cc_sort.h and csrc/k_knn.h.  Included after the product's headers by BOTH builds:
//   tests/devprobe/devprobe.hip  hipcc, gfx950, the library's own flags  -> the code the product runs (DPP, readlane, mbcnt, v_rsq_f64)
//   tests/emu/emu_main.cpp       g++, CC_EMU                              -> the shuffle forms the CPU harness runs
// so the two test files (tests/test_gpu_primitives.py, tests/test_emu_primitives.py) drive the same entry points with the
// same cases.  A probe calls the product's function and writes what each lane got; it restates nothing.  Every launcher
// takes device pointers (host pointers on the harness), launches on the null stream and returns hipGetLastError(); every
// access is guarded by the element count the caller passes, and the callers size their arrays from the same count.
#ifdef CC_EMU
#define PROBE_MARK(n) asm volatile("")
#define PROBE_EW_GRID_CAP 8  // one OS thread per workgroup in flight: a few grid-striding workgroups are enough
#else
#define PROBE_MARK(n) asm volatile("; probe branch " #n)  // two branches with different marks cannot be merged into one
#define PROBE_EW_GRID_CAP 4096
#endif

// ---- A. row and wave collectives ---------------------------------------------------------------------------------------
enum {
  PROBE_BALLOT = 0, PROBE_SCAN = 1, PROBE_SUM_I = 2, PROBE_OR_U = 3, PROBE_BEST = 4, PROBE_BCAST = 5, PROBE_SUM_D = 6, PROBE_QUAD = 7,
  PROBE_SHR = 8, PROBE_SHL1 = 9, PROBE_GSUM64 = 10, PROBE_WSCAN = 11, PROBE_MASK = 12, PROBE_BITS = 13
};
struct probe_res {
  int i[4];
  double d;
};
__device__ __forceinline__ void probe_apply(int op, int a, int b, double d, unsigned long long m, probe_res &o) {
  switch (op) {
    case PROBE_BALLOT: o.i[0] = (int)cc_group_ballot((a & 1) != 0); break;
    case PROBE_SCAN: o.i[0] = cc_group_scan_incl(a); break;
    case PROBE_SUM_I: o.i[0] = cc_group_sum_i(a); break;
    case PROBE_OR_U: o.i[0] = (int)cc_group_or_u((unsigned)a); break;
    case PROBE_BEST: {
      int x = a, y = b;
      cc_group_best(x, y);
      o.i[0] = x;
      o.i[1] = y;
    } break;
    case PROBE_BCAST:
      o.i[0] = cc_group_bcast(a, b & 15);
      o.d = cc_group_bcast(d, b & 15);
      break;
    case PROBE_SUM_D: o.d = cc_group_sum_d(d); break;
    case PROBE_QUAD: {
      const float f = __int_as_float(a);
      o.i[0] = __float_as_int(cc_quad_bcast<0>(f));
      o.i[1] = __float_as_int(cc_quad_bcast<1>(f));
      o.i[2] = __float_as_int(cc_quad_bcast<2>(f));
      o.i[3] = __float_as_int(cc_quad_bcast<3>(f));
    } break;
    case PROBE_SHR:
      o.i[0] = cc_row_shr<1>(a);
      o.i[1] = cc_row_shr<2>(a);
      o.i[2] = cc_row_shr<4>(a);
      o.i[3] = cc_row_shr<8>(a);
      break;
    case PROBE_SHL1: o.i[0] = cc_row_shl1(a); break;
    case PROBE_GSUM64: o.d = cc_gsum<64>(d); break;  // whole wave only
    case PROBE_WSCAN: {                              // whole wave only
      const int incl = cc_wave_scan_incl(a);
      o.i[0] = incl;
      o.i[1] = cc_wave_scan_total(incl);
    } break;
    case PROBE_MASK:
      o.i[0] = cc_mbcnt(m);
      o.i[1] = cc_mask_lane(m) ? 1 : 0;
      break;
    case PROBE_BITS:
      o.i[0] = (int)cc_push_sign((unsigned)b, __int_as_float(a));
      o.i[1] = (int)cc_brev((unsigned)a);
      break;
    default: break;
  }
}
// mode 1..15: bit r set = row r of every wave takes part, the other rows return before the call;
// mode 16: even rows and odd rows call the primitive in the two branches of one if / else, each on operands of its own;
// mode 17: the same with row 0 against rows 1-3.  Lanes that do not take part leave their outputs as the caller filled them.
__global__ void probe_k_group(int op, int mode, const int *a0, const int *b0, const double *d0, const int *a1, const int *b1, const double *d1,
                              const unsigned long long *wave_mask, int *oi, double *od) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int row = (int)(threadIdx.x >> 4) & 3;
  const unsigned long long m = wave_mask[t >> 6];  // the same in every lane of a wave
  probe_res o;
  o.i[0] = o.i[1] = o.i[2] = o.i[3] = 0;
  o.d = 0.0;
  if (mode < 16) {
    if (!((mode >> row) & 1)) return;
    probe_apply(op, a0[t], b0[t], d0[t], m, o);
  } else {
    const bool first = mode == 16 ? (row & 1) == 0 : row == 0;
    if (first) {
      probe_apply(op, a0[t], b0[t], d0[t], m, o);
      PROBE_MARK(0);
    } else {
      probe_apply(op, a1[t], b1[t], d1[t], ~m, o);
      PROBE_MARK(1);
    }
  }
  for (int k = 0; k < 4; k++) oi[4 * t + k] = o.i[k];
  od[t] = o.d;
}
// cc_wave_id, cc_uniform_i, cc_uniform_ptr: `vals` holds one int per wave
__global__ void probe_k_uniform(const int *vals, int *out) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int gw = t >> 6;
  out[3 * t + 0] = cc_wave_id();
  out[3 * t + 1] = cc_uniform_i(vals[gw]);
  const int *p = cc_uniform_ptr(vals + gw);
  out[3 * t + 2] = *p;
}
__global__ void probe_k_pk_fma(const float *a, const float *b, const float *c, float *out, long n_pairs) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_pairs; i += (long)gridDim.x * blockDim.x) {
    cc_f2 x, y, z;
    x.x = a[2 * i], x.y = a[2 * i + 1];
    y.x = b[2 * i], y.y = b[2 * i + 1];
    z.x = c[2 * i], z.y = c[2 * i + 1];
    const cc_f2 r = cc_pk_fma(x, y, z);
    out[2 * i] = r.x;
    out[2 * i + 1] = r.y;
  }
}
__global__ void probe_k_load3f(const char *base, int stride, float *out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float x, y, z;
    cc_load3f(base + i * stride, x, y, z);
    out[3 * i] = x;
    out[3 * i + 1] = y;
    out[3 * i + 2] = z;
  }
}

// ---- B. f64 routines -----------------------------------------------------------------------------------------------------
__global__ void probe_k_exp_nonpos(const double *z, double *out, long n) {
  __shared__ double exp_tab[64];
  if (threadIdx.x < 64) exp_tab[threadIdx.x] = __longlong_as_double((long long)cc_exp2_tab64[threadIdx.x]);
  __syncthreads();
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = cc_exp_nonpos(z[i], exp_tab);
}
__global__ void probe_k_rsqrt(const double *x, double *out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = cc_rsqrt(x[i]);
}
__global__ void probe_k_sqrt(const double *x, double *out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = sqrt(x[i]);
}
// raw: 14 f32 per pair (src cov c00 c01 c10 c11 | tgt cov | src mean, tgt mean | w_s, w_t), pose: px py c s c2 s2
__global__ void probe_k_gmm_term(const float *raw, const double *pose, double *out, long n) {
  __shared__ double exp_tab[64];
  if (threadIdx.x < 64) exp_tab[threadIdx.x] = __longlong_as_double((long long)cc_exp2_tab64[threadIdx.x]);
  __syncthreads();
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float *f = raw + 14 * i;
    cc_graw r;
    r.s = make_float4(f[0], f[1], f[2], f[3]);
    r.t = make_float4(f[4], f[5], f[6], f[7]);
    r.m = make_float4(f[8], f[9], f[10], f[11]);
    r.w = make_float2(f[12], f[13]);
    const cc_gpair P = cc_gmm_make_pair(r);
    const double *p = pose + 6 * i;
    const cc_gterm g = cc_gmm_term(P, p[0], p[1], p[2], p[3], p[4], p[5], exp_tab);
    out[4 * i] = g.v;
    out[4 * i + 1] = g.gx;
    out[4 * i + 2] = g.gy;
    out[4 * i + 3] = g.gt;
  }
}

// ---- C. bit-for-bit carriers ---------------------------------------------------------------------------------------------
__global__ void probe_k_atan2f(const float *y, const float *x, float *out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = cc_atan2f_fdlibm(y[i], x[i]);
}
__global__ void probe_k_acosf(const float *x, float *out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = cc_acosf_fdlibm(x[i]);
}
__global__ void probe_k_eigen2f(const float *m, float *out, long n) {  // m: [n][3], out: [n][6] = evals, evecs
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float ev[2], vec[4];
    cc_eigen2f(m[3 * i], m[3 * i + 1], m[3 * i + 2], ev, vec);
    out[6 * i] = ev[0];
    out[6 * i + 1] = ev[1];
    for (int k = 0; k < 4; k++) out[6 * i + 2 + k] = vec[k];
  }
}
// ccsort::std_sort as ONE lane per array: workgroup b sorts arr[offs[b] .. offs[b + 1]) in place, descending by the upper
// 16 bits (K2's size order)
__global__ void probe_k_sort_desc(unsigned *arr, const int *offs) {
  __shared__ unsigned stk[CC_SORT_STACK];
  const int o = offs[blockIdx.x], n = offs[blockIdx.x + 1] - o;
  if (threadIdx.x == 0) ccsort::std_sort(arr + o, n, [](unsigned x, unsigned y) { return (x >> 16) > (y >> 16); }, stk);
}
struct probe_fkey {
  float k;
  int idx;
};
__global__ void probe_k_sort_asc_f(probe_fkey *arr, const int *offs) {
  __shared__ unsigned stk[CC_SORT_STACK];
  const int o = offs[blockIdx.x], n = offs[blockIdx.x + 1] - o;
  if (threadIdx.x == 0) ccsort::std_sort(arr + o, n, [](const probe_fkey &x, const probe_fkey &y) { return x.k < y.k; }, stk);
}
// the wave-parallel std::sort replay (cc_sort.h: std_sort_wave) on one array per workgroup of one wave, as K2's size sort
// uses it; every array has fewer than 4096 elements
__global__ void probe_k_sort_wave(unsigned *arr, const unsigned *pristine, const int *offs) {
  __shared__ unsigned a[4096];
  __shared__ unsigned short st[2 * 4096];
  __shared__ unsigned seg[CC_SORT_STACK];
  const int lane = threadIdx.x;
  const int o = offs[blockIdx.x], n = offs[blockIdx.x + 1] - o;
  if (n >= 4096) return;
  arr += o;
  pristine += o;
  for (int i = lane; i < n; i += 64) a[i] = pristine[i];
  ccsort::std_sort_wave(
      a, n, [](unsigned x) { return 0xFFFFu - (x >> 16); },
      [&]() {
        for (int i = lane; i < n; i += 64) a[i] = pristine[i];
      },
      lane, st, st + 4096, (unsigned *)st, seg);
  for (int i = lane; i < n; i += 64) arr[i] = a[i];
}
// the order kernel's workgroup sort (k_knn.h: cc_block_bitonic_u32), 1024 * R keys
template <int R>
__global__ void __launch_bounds__(1024) probe_k_block_bitonic(unsigned *arr) {
  __shared__ unsigned xch[1024 * R];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned v[R];
  for (int a = 0; a < R; a++) v[a] = arr[(wave * R + a) * 64 + lane];
  cc_block_bitonic_u32<R>(v, xch, tid);
  for (int a = 0; a < R; a++) arr[(wave * R + a) * 64 + lane] = v[a];
}
// and its in-place block scans (cc_block_scan), n a power of two <= 8192
__global__ void __launch_bounds__(1024) probe_k_block_scan(int *arr, int n, int is_max) {
  __shared__ int a[8192];
  __shared__ int wsum[16];
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 1024) a[i] = arr[i];
  __syncthreads();
  if (is_max)
    cc_block_scan<true>(a, n, tid, wsum);
  else
    cc_block_scan<false>(a, n, tid, wsum);
  for (int i = tid; i < n; i += 1024) arr[i] = a[i];
}

static inline unsigned probe_ew_grid(long n) {
  const long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > PROBE_EW_GRID_CAP ? PROBE_EW_GRID_CAP : g));
}
#define PROBE_EW(kernel, n, ...)                                                                     \
  do {                                                                                               \
    if ((n) > 0) hipLaunchKernelGGL(kernel, dim3(probe_ew_grid(n)), dim3(256), 0, nullptr, __VA_ARGS__); \
    return (int)hipGetLastError();                                                                   \
  } while (0)

extern "C" {
// block: 64 or 256 threads; every array holds n_blocks * block elements (oi: four ints per element), wave_mask one word per wave
int probe_group(int op, int mode, int n_blocks, int block, const int *a0, const int *b0, const double *d0, const int *a1, const int *b1,
                const double *d1, const unsigned long long *wave_mask, int *oi, double *od) {
  if (n_blocks <= 0 || (block != 64 && block != 256) || mode < 1 || mode > 17 || op < 0 || op > PROBE_BITS) return -1;
  if ((op == PROBE_GSUM64 || op == PROBE_WSCAN) && mode != 15) return -1;  // whole-wave primitives: every lane takes part
  hipLaunchKernelGGL(probe_k_group, dim3(n_blocks), dim3(block), 0, nullptr, op, mode, a0, b0, d0, a1, b1, d1, wave_mask, oi, od);
  return (int)hipGetLastError();
}
int probe_uniform(int n_blocks, const int *vals, int *out) {  // block = 256: vals [4 * n_blocks], out [256 * n_blocks][3]
  if (n_blocks <= 0) return -1;
  hipLaunchKernelGGL(probe_k_uniform, dim3(n_blocks), dim3(256), 0, nullptr, vals, out);
  return (int)hipGetLastError();
}
int probe_pk_fma(const float *a, const float *b, const float *c, float *out, long n_pairs) { PROBE_EW(probe_k_pk_fma, n_pairs, a, b, c, out, n_pairs); }
int probe_load3f(const char *base, int stride, float *out, long n) { PROBE_EW(probe_k_load3f, n, base, stride, out, n); }
int probe_exp_nonpos(const double *z, double *out, long n) { PROBE_EW(probe_k_exp_nonpos, n, z, out, n); }
int probe_rsqrt(const double *x, double *out, long n) { PROBE_EW(probe_k_rsqrt, n, x, out, n); }
int probe_sqrt(const double *x, double *out, long n) { PROBE_EW(probe_k_sqrt, n, x, out, n); }
int probe_gmm_term(const float *raw, const double *pose, double *out, long n) { PROBE_EW(probe_k_gmm_term, n, raw, pose, out, n); }
int probe_atan2f(const float *y, const float *x, float *out, long n) { PROBE_EW(probe_k_atan2f, n, y, x, out, n); }
int probe_acosf(const float *x, float *out, long n) { PROBE_EW(probe_k_acosf, n, x, out, n); }
int probe_eigen2f(const float *m, float *out, long n) { PROBE_EW(probe_k_eigen2f, n, m, out, n); }
// n_cases arrays side by side, array b = [offs[b], offs[b + 1]); std_sort: every length < 4096 (the caller checks)
int probe_sort_desc(unsigned *arr, const int *offs, int n_cases) {
  if (n_cases > 0) hipLaunchKernelGGL(probe_k_sort_desc, dim3(n_cases), dim3(64), 0, nullptr, arr, offs);
  return (int)hipGetLastError();
}
int probe_sort_asc_f(probe_fkey *arr, const int *offs, int n_cases) {
  if (n_cases > 0) hipLaunchKernelGGL(probe_k_sort_asc_f, dim3(n_cases), dim3(64), 0, nullptr, arr, offs);
  return (int)hipGetLastError();
}
int probe_sort_desc_wave(unsigned *arr, const unsigned *pristine, const int *offs, int n_cases) {
  if (n_cases > 0) hipLaunchKernelGGL(probe_k_sort_wave, dim3(n_cases), dim3(64), 0, nullptr, arr, pristine, offs);
  return (int)hipGetLastError();
}
int probe_block_bitonic(unsigned *arr, int r) {  // arr: 1024 * r keys
  if (r == 1)
    hipLaunchKernelGGL(probe_k_block_bitonic<1>, dim3(1), dim3(1024), 0, nullptr, arr);
  else if (r == 4)
    hipLaunchKernelGGL(probe_k_block_bitonic<4>, dim3(1), dim3(1024), 0, nullptr, arr);
  else if (r == 8)
    hipLaunchKernelGGL(probe_k_block_bitonic<8>, dim3(1), dim3(1024), 0, nullptr, arr);
  else
    return -1;
  return (int)hipGetLastError();
}
int probe_block_scan(int *arr, int n, int is_max) {  // n: a power of two, 64 .. 8192
  if (n < 64 || n > 8192 || (n & (n - 1))) return -1;
  hipLaunchKernelGGL(probe_k_block_scan, dim3(1), dim3(1024), 0, nullptr, arr, n, is_max);
  return (int)hipGetLastError();
}
}
