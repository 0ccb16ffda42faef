// elementwise.hip — the HBM-bound kernels of the UNet++ path (NHWC, 16 B/lane):
//   BatchNorm2d(+ReLU)(+MaxPool2d) forward, BatchNorm/ReLU backward,
//   MaxPool2d(2,2) fwd/bwd, bilinear x2 align_corners upsample fwd/bwd,
//   1x1 heads fwd/bwd, SGD / Adam, loss scaling, weight EMA, gradient clipping, layout helpers.
//   (Losses, metrics and the validation step: loss.hip.)
// Reference arithmetic: finished/archs1.py:17-21,82-83,105-111; trains.py:225-231.
#include <cmath>
#include <stdlib.h>
#include <string.h>

#include "common.h"

static thread_local char g_err[512] = "";
void nunet_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int nunet_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    nunet_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return NUNET_ELAUNCH;
  }
  // NUNET_TRACE_LAUNCH=1 (diagnostic, eager mode only): name every launch on stderr and wait for it, so that a
  // faulting kernel is the last name printed
  static int trace = -1;
  if (trace < 0) { const char* t = getenv("NUNET_TRACE_LAUNCH"); trace = t ? atoi(t) : 0; }
  if (trace) {
    fprintf(stderr, "[nunet] %s ... ", what); fflush(stderr);
    e = hipDeviceSynchronize();
    fprintf(stderr, "%s\n", e == hipSuccess ? "ok" : hipGetErrorString(e)); fflush(stderr);
    if (e != hipSuccess) { nunet_set_error("%s: execution failed: %s", what, hipGetErrorString(e)); return NUNET_ELAUNCH; }
  }
  return NUNET_OK;
}
extern "C" const char* nunet_last_error(void) { return g_err; }
extern "C" int nunet_version(void) { return 104; }

__global__ __launch_bounds__(256) void zero_kernel(u32x4* __restrict__ p16, size_t n16, uint32_t* __restrict__ tail, int ntail) {
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p16[i] = z;
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0u;
}
int nunet_zero_async(void* p, size_t bytes, hipStream_t st) {
  NUNET_REQUIRE(((uintptr_t)p % 16) == 0 && bytes % 4 == 0, "zero: buffer must be 16-byte aligned, size a multiple of 4");
  const size_t n16 = bytes / 16;
  const int ntail = (int)((bytes % 16) / 4);
  NUNET_LAUNCH(zero_kernel, dim3(grid_for((int64_t)n16, 256 * 4, 2048)), dim3(256), 0, st, (u32x4*)p, n16,
                     (uint32_t*)((char*)p + n16 * 16), ntail);
  return nunet_check_launch("zero");
}

// ---------------------------------------------------------------------------
// layout: NCHW fp32 -> NHWC T with zero channel padding
// ---------------------------------------------------------------------------
// One thread per (pixel, 16-byte channel group): consecutive threads write consecutive 16 bytes; blockIdx.y is the image,
// so there is no division in the kernel (the first version spent two 64-bit divisions per 2-byte element).
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, int C, int hw, T* __restrict__ y, int cpad, int gshift) {
  constexpr int EPV = Tr<T>::EPV;
  const int n = blockIdx.y;
  const int groups = 1 << gshift;
  const float* xi = x + (size_t)n * C * hw;
  T* yi = y + (size_t)n * hw * cpad;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < (hw << gshift); j += gridDim.x * blockDim.x) {
    const int pix = j >> gshift, c0 = (j & (groups - 1)) * EPV;
    Vec16<T> v;
#pragma unroll
    for (int e = 0; e < EPV; ++e) v.set(e, c0 + e < C ? xi[(size_t)(c0 + e) * hw + pix] : 0.f);
    st16(yi + (size_t)pix * cpad + c0, v);
  }
}
template <typename T> static int launch_nchw_to_nhwc(const float* x, int N, int C, int H, int W, void* y, int cpad, hipStream_t st) {
  constexpr int EPV = Tr<T>::EPV;
  const int groups = cpad / EPV;
  int gshift = 0;
  while ((1 << gshift) < groups) ++gshift;
  NUNET_REQUIRE(cpad % EPV == 0 && (1 << gshift) == groups && N <= 65535, "nchw_to_nhwc: cpad=%d must be a power-of-two number of 16-byte groups", cpad);
  const long long hw = (long long)H * W;
  NUNET_REQUIRE(hw * groups < (1ll << 31), "nchw_to_nhwc: image too large");
  const int64_t total = (int64_t)N * H * W * cpad;
  ProfScope ps(PC_LAYOUT, 0, (double)total * sizeof(T) + (double)N * C * H * W * 4, st);
  NUNET_LAUNCH((nchw_to_nhwc_kernel<T>), dim3(grid_for(hw * groups, 256, 1024), N), dim3(256), 0, st, x, C, (int)hw, (T*)y, cpad, gshift);
  return nunet_check_launch("nchw_to_nhwc");
}
extern "C" int nunet_nchw_to_nhwc(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t dtype, void* y, int32_t cpad, nunet_stream_t s) {
  NUNET_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0 && cpad >= C, "nchw_to_nhwc: bad args");
  return NUNET_DISPATCH(dtype, launch_nchw_to_nhwc, x, N, C, H, W, y, cpad, (hipStream_t)s);
}

// ---------------------------------------------------------------------------
// BatchNorm (+ReLU) (+2x2 max-pool) forward
// ---------------------------------------------------------------------------
__device__ __forceinline__ void up_taps(int o, float scale, int n_in, int& i0, int& i1, float& l1);
__device__ __forceinline__ float up_lerp(float v00, float v01, float v10, float v11, float ly, float lx);
struct BnFwdP {
  void* up; int PU; int nb_main; Dec4 dcu;     // fused x2 bilinear upsample of the activation (second block role), or up == NULL
  const void* y; int PY;
  const float* conv_bias; const long long* stats; const float* gamma; const float* beta;
  float* rm; float* rv; int64_t* nbt; float* save;
  int training; float momentum, eps;
  void* a; int PA; void* pooled; int PP;
  int N, H, W, C;
};

// (the conv bias is absorbed here, see bn_stat_coeffs in common.h)
__device__ __forceinline__ void bn_channel_coeffs(const BnFwdP& p, int c, float M, float& mean, float& invstd, float& var, float& mean_full) {
  BnStatArgs a; a.fx = p.stats; a.conv_bias = p.conv_bias; a.rm = p.rm; a.rv = p.rv; a.C = p.C; a.training = p.training; a.M = M; a.eps = p.eps;
  bn_stat_coeffs(a, c, mean, invstd, var, mean_full);
}

// per-channel scale / shift tables once per block (not per thread); block 0 also owns the running-stat update and the saved
// mean/invstd for backward. Ends with the barrier that publishes the tables.
__device__ __forceinline__ void bn_fwd_prologue(const BnFwdP& p, float M, float* s_sc, float* s_sh) {
  for (int c = threadIdx.x; c < p.C; c += blockDim.x) {
    float mean, invstd, var, mf;
    bn_channel_coeffs(p, c, M, mean, invstd, var, mf);
    const float sc = p.gamma[c] * invstd;
    s_sc[c] = sc;
    s_sh[c] = __builtin_fmaf(-mean, sc, p.beta[c]);
    if (blockIdx.x == 0 && p.training) {
      p.save[c] = mean;
      p.save[p.C + c] = invstd;
      if (p.rm) bn_running_update(p.rm, p.rv, c, p.momentum, mf, var, M);
    }
  }
  if (blockIdx.x == 0 && p.training && threadIdx.x == 0 && p.nbt) *p.nbt += 1;
  __syncthreads();
}

template <typename T, bool POOL>
__global__ __launch_bounds__(256) void bn_relu_fwd_kernel(BnFwdP p) {
  constexpr int EPV = Tr<T>::EPV;
  __shared__ __attribute__((aligned(16))) float s_sc[2048], s_sh[2048];
  const int G = p.C / EPV;  // channel groups; 256 % G == 0
  const int cg = threadIdx.x % G;
  const float M = (float)p.N * p.H * p.W;
  // first batch of loads ahead of the coefficient prologue (latencies overlap)
  constexpr int U = 4;   // 16-byte loads kept in flight per thread
  const int ppb0 = blockDim.x / G, pl0 = threadIdx.x / G;
  const int64_t npix0 = (int64_t)p.N * p.H * p.W;
  const int nbm = p.up ? p.nb_main : (int)gridDim.x;     // blocks of the BatchNorm role (the rest, if any, upsample)
  const bool main_role = (int)blockIdx.x < nbm;
  const int64_t stride0 = (int64_t)nbm * ppb0;
  Vec16<T> v[U];
  auto load_batch = [&](int64_t p0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pix = p0 + u * stride0;
      if (pix < npix0) v[u] = ld16((const T*)p.y + pix * p.PY + cg * EPV);
    }
  };
  int64_t pix0 = (int64_t)blockIdx.x * ppb0 + pl0;
  if constexpr (!POOL) { if (main_role && pix0 < npix0) load_batch(pix0); }
  const int H2 = p.H / 2, W2 = p.W / 2;
  const int64_t nq = (int64_t)p.N * H2 * W2;
  Vec16<T> vq[4];
  const bool q32 = nq < (1ll << 31);   // 32-bit index decode (a 64-bit division is >100 instructions here)
  auto quad_base = [&](int64_t q) {
    if (q32) {
      const unsigned t = (unsigned)q / (unsigned)W2, qx = (unsigned)q - t * (unsigned)W2;
      const unsigned n = t / (unsigned)H2, qy = t - n * (unsigned)H2;
      return ((int64_t)n * p.H + 2 * qy) * p.W + 2 * qx;
    }
    const int qx = (int)(q % W2);
    const int64_t t = q / W2;
    const int qy = (int)(t % H2);
    const int n = (int)(t / H2);
    return ((int64_t)n * p.H + 2 * qy) * p.W + 2 * qx;
  };
  int64_t p00_cur = 0;                  // base pixel of the quad whose loads are in flight
  auto qload = [&](int64_t q) {
    const int64_t p00 = p00_cur = quad_base(q);
#pragma unroll
    for (int k = 0; k < 4; ++k) vq[k] = ld16((const T*)p.y + (p00 + (k >> 1) * p.W + (k & 1)) * p.PY + cg * EPV);
  };
  const int64_t q0 = (int64_t)blockIdx.x * ppb0 + pl0;
  if constexpr (POOL) { if (main_role && q0 < nq) qload(q0); }
  bn_fwd_prologue(p, M, s_sc, s_sh);
  typedef typename FV<T>::type V;
  if (p.up && (int)blockIdx.x >= p.nb_main) {
    // ---- second role: nn.Upsample(x2, bilinear, align_corners) of the activation (archs1.py:83,116-131), straight from the raw
    // tensor: every tap is relu(bn(y)) ROUNDED to the storage type - the value the first role stores - so the result equals the
    // stand-alone upsample of the stored activation bit for bit, without waiting for it (one launch less per block on the chain)
    const int HO = 2 * p.H, WO = 2 * p.W;
    const float sy = HO > 1 ? (float)(p.H - 1) / (float)(HO - 1) : 0.f;
    const float sx = WO > 1 ? (float)(p.W - 1) / (float)(WO - 1) : 0.f;
    const int64_t total = (int64_t)p.N * HO * WO * G;
    const int64_t nthr = (int64_t)(gridDim.x - p.nb_main) * blockDim.x;
    for (int64_t i = ((int64_t)blockIdx.x - p.nb_main) * blockDim.x + threadIdx.x; i < total; i += nthr) {
      int cgu, ox, oy, n; long long o;
      dec4(p.dcu, i, cgu, o, ox, oy, n);
      int y0, y1, x0, x1; float ly, lx;
      up_taps(oy, sy, p.H, y0, y1, ly);
      up_taps(ox, sx, p.W, x0, x1, lx);
      const T* b = (const T*)p.y + (int64_t)n * p.H * p.W * p.PY + cgu * EPV;
      const Vec16<T> r00 = ld16(b + ((int64_t)y0 * p.W + x0) * p.PY), r01 = ld16(b + ((int64_t)y0 * p.W + x1) * p.PY);
      const Vec16<T> r10 = ld16(b + ((int64_t)y1 * p.W + x0) * p.PY), r11 = ld16(b + ((int64_t)y1 * p.W + x1) * p.PY);
      const V scu = ldf<T>(&s_sc[cgu * EPV]), shu = ldf<T>(&s_sh[cgu * EPV]);
      const Vec16<T> v00 = vec_from_f<T>(bn_relu_apply<V>(vec_to_f<T>(r00), scu, shu)), v01 = vec_from_f<T>(bn_relu_apply<V>(vec_to_f<T>(r01), scu, shu));
      const Vec16<T> v10 = vec_from_f<T>(bn_relu_apply<V>(vec_to_f<T>(r10), scu, shu)), v11 = vec_from_f<T>(bn_relu_apply<V>(vec_to_f<T>(r11), scu, shu));
      Vec16<T> r;
#pragma unroll
      for (int e = 0; e < EPV; ++e) r.set(e, up_lerp(v00.get(e), v01.get(e), v10.get(e), v11.get(e), ly, lx));
      st16((T*)p.up + o * p.PU + cgu * EPV, r);
    }
    return;
  }
  const V sc = ldf<T>(&s_sc[cg * EPV]), sh = ldf<T>(&s_sh[cg * EPV]);
  const int ppb = blockDim.x / G;  // pixels (or quads) per block iteration
  const int pl = threadIdx.x / G;
  if constexpr (!POOL) {
    const int64_t npix = npix0, stride = stride0;
    while (pix0 < npix) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t pix = pix0 + u * stride;
        if (pix < npix) st16((T*)p.a + pix * p.PA + cg * EPV, vec_from_f<T>(bn_relu_apply<V>(vec_to_f<T>(v[u]), sc, sh)));
      }
      pix0 += U * stride;
      if (pix0 < npix) load_batch(pix0);
    }
  } else {
    // (the quad loads of the first iteration were issued ahead of the prologue, see qload)
    int64_t q = q0;
    while (q < nq) {
      const int64_t p00 = p00_cur;
      // the running maximum is taken over the ROUNDED activations (what a later pool would see): converting the stored
      // vector back is exact, and max is order-independent
      V mx;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t pix = p00 + (k >> 1) * p.W + (k & 1);
        const Vec16<T> o = vec_from_f<T>(bn_relu_apply<V>(vec_to_f<T>(vq[k]), sc, sh));
        const V ar = vec_to_f<T>(o);
        mx = (k == 0) ? ar : __builtin_elementwise_max(mx, ar);
        st16((T*)p.a + pix * p.PA + cg * EPV, o);
      }
      st16((T*)p.pooled + q * p.PP + cg * EPV, vec_from_f<T>(mx));
      q += (int64_t)nbm * ppb;
      if (q < nq) qload(q);
    }
  }
}

static BnFwdP bn_fwd_params(const nunet_bn_fwd_desc* d) {
  BnFwdP p;
  p.y = d->y; p.PY = d->PY; p.conv_bias = d->conv_bias; p.stats = (const long long*)d->stats; p.gamma = d->gamma; p.beta = d->beta;
  p.rm = d->running_mean; p.rv = d->running_var; p.nbt = d->num_batches_tracked; p.save = d->save_mean_invstd;
  p.training = d->training; p.momentum = d->momentum; p.eps = d->eps;
  p.a = d->a; p.PA = d->PA; p.pooled = d->pooled; p.PP = d->PP;
  p.N = d->N; p.H = d->H; p.W = d->W; p.C = d->C;
  p.up = nullptr; p.PU = 0; p.nb_main = 0; memset(&p.dcu, 0, sizeof(p.dcu));
  return p;
}
// workgroups of the BatchNorm role without a pool: 256 / G pixels per workgroup and pass, four passes in flight per thread
static int bn_fwd_grid(int64_t npix, int G) { return grid_for(npix, (256 / G) * 4, 2048); }
template <typename T> static int launch_bn_fwd(const nunet_bn_fwd_desc* d, hipStream_t st) {
  BnFwdP p = bn_fwd_params(d);
  const int G = d->C / Tr<T>::EPV;
  const int ppb = 256 / G;
  // optional second role of the launch: the x2 upsample of the activation (extra blocks behind the BatchNorm role's)
  p.up = d->up; p.PU = d->PU;
  const int64_t utotal = (int64_t)d->N * 4 * d->H * d->W * G;
  // (persistent blocks, ~8 outputs per thread: every block pays the coefficient prologue - two dependent global-memory latencies -
  //  so one block per 256 outputs, the stand-alone upsample's grid, made the fused launch twice as long as the two it replaces)
  const int nb_up = d->up ? grid_for(utotal, 256 * 8, 1024) : 0;
  p.dcu = make_dec4(utotal, G, 2 * d->W, 2 * d->H);
  ProfScope ps(PC_BN_FWD, 0, (double)d->N * d->H * d->W * d->C * sizeof(T) * ((d->pooled ? 2.25 : 2.0) + (d->up ? 5.0 : 0.0)), st);
  if (d->pooled) {
    const int64_t nq = (int64_t)d->N * (d->H / 2) * (d->W / 2);
    p.nb_main = grid_for(nq, ppb * 2, 2048);
    NUNET_LAUNCH((bn_relu_fwd_kernel<T, true>), dim3(p.nb_main + nb_up), dim3(256), 0, st, p);
  } else {
    p.nb_main = bn_fwd_grid((int64_t)d->N * d->H * d->W, G);
    NUNET_LAUNCH((bn_relu_fwd_kernel<T, false>), dim3(p.nb_main + nb_up), dim3(256), 0, st, p);
  }
  return nunet_check_launch("bn_relu_fwd");
}
static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// what nunet_bn_relu_fwd and nunet_head_fwd_bn both ask of the descriptor
static int bn_fwd_check(const nunet_bn_fwd_desc* d) {
  NUNET_REQUIRE(d && d->y && d->a && d->gamma && d->beta, "bn_relu_fwd: null pointer");
  const int epv = 16 / dtype_size(d->dtype);
  NUNET_REQUIRE(pow2(d->C) && d->C >= epv && d->C / epv <= 256, "bn_relu_fwd: C=%d must be a power of two in [%d, %d]", d->C, epv, 256 * epv);
  NUNET_REQUIRE(d->PY % epv == 0 && d->PA % epv == 0 && (!d->pooled || d->PP % epv == 0), "bn_relu_fwd: pitch alignment");
  NUNET_REQUIRE(!d->pooled || (d->H % 2 == 0 && d->W % 2 == 0), "bn_relu_fwd: fused pool needs even H, W");
  NUNET_REQUIRE(!d->up || d->PU % epv == 0, "bn_relu_fwd: fused upsample pitch alignment");
  if (d->training) NUNET_REQUIRE(d->stats && d->save_mean_invstd, "bn_relu_fwd: training needs stats and save buffers");
  else NUNET_REQUIRE(d->running_mean && d->running_var, "bn_relu_fwd: eval needs running stats");
  return NUNET_OK;
}
extern "C" int nunet_bn_relu_fwd(const nunet_bn_fwd_desc* d, nunet_stream_t s) {
  const int rc = bn_fwd_check(d);
  if (rc) return rc;
  return NUNET_DISPATCH(d->dtype, launch_bn_fwd, d, (hipStream_t)s);
}

// ---------------------------------------------------------------------------
// BatchNorm (+ReLU) backward: reduce pass and apply pass
// ---------------------------------------------------------------------------
struct BnBwdP {
  const void* da; int PDA; const void* y; int PY;
  const float* mi; const float* gamma; const float* beta;
  long long* sums; float* dgamma; float* dbeta; float* dbias;
  void* dy; int PDY;
  int N, H, W, C;
};

template <typename T, bool APPLY>
__global__ __launch_bounds__(256) void bn_relu_bwd_kernel(BnBwdP p) {
  constexpr int EPV = Tr<T>::EPV;
  constexpr int NV = 2;                             // partial sums per channel (reduce pass)
  __shared__ __attribute__((aligned(16))) float s_co[6 * 2048 / 4];   // coefficient tables, C <= 512: [6][C]
  __shared__ float s_part[APPLY ? 1 : 256 * NV * EPV];   // per-thread partials for the block reduction
  const int G = p.C / EPV;
  const int cg = threadIdx.x % G;
  const int ppb = blockDim.x / G, pl = threadIdx.x / G;
  const float M = (float)p.N * p.H * p.W;
  const int C = p.C;
  // the first batch of activation loads is issued BEFORE the per-channel coefficient prologue, so the two
  // global-memory latencies overlap (the small pyramid levels run exactly one iteration per thread)
  const int64_t npix = (int64_t)p.N * p.H * p.W;
  const int64_t stride = (int64_t)gridDim.x * ppb;
  constexpr int U = 4;   // pixels per thread per iteration: 8 sixteen-byte loads in flight
  Vec16<T> vy[U], vd[U];
  auto load_batch = [&](int64_t p0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pix = p0 + u * stride;
      if (pix < npix) {
        vy[u] = ld16((const T*)p.y + pix * p.PY + cg * EPV);
        vd[u] = ld16((const T*)p.da + pix * p.PDA + cg * EPV);
      }
    }
  };
  int64_t pix0 = (int64_t)blockIdx.x * ppb + pl;
  if (pix0 < npix) load_batch(pix0);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float mean = p.mi[c], istd = p.mi[C + c];
    const float sc = p.gamma[c] * istd;
    s_co[c] = mean; s_co[C + c] = istd; s_co[2 * C + c] = sc; s_co[3 * C + c] = __builtin_fmaf(-mean, sc, p.beta[c]);
    if constexpr (APPLY) {
      const int nrep = bn_sum_replicas(C);
      double t1, t2;
      fx_totals(p.sums, C, nrep, c, t1, t2);
      float A, B;
      bn_bwd_AB(mean, istd, sc, (float)(t1 / (double)M), (float)(t2 / (double)M), A, B);
      s_co[4 * C + c] = A; s_co[5 * C + c] = B;
      if (blockIdx.x == 0) {
        // d beta = sum dz, d gamma = sum dz * xhat; the conv bias in front of the BatchNorm has gradient sum(dy) == 0
        if (p.dbeta) p.dbeta[c] = (float)t1;
        if (p.dgamma) p.dgamma[c] = (float)t2;
        if (p.dbias) p.dbias[c] = 0.f;
      }
    }
  }
  __syncthreads();
  __attribute__((aligned(16))) float sc[EPV], sh[EPV], mean[EPV], istd[EPV], k1[EPV], k2[EPV];   // APPLY: k1, k2 hold A, B (bn_bwd_AB)
#pragma unroll
  for (int e = 0; e < EPV; ++e) {
    const int c = cg * EPV + e;
    mean[e] = s_co[c]; istd[e] = s_co[C + c]; sc[e] = s_co[2 * C + c]; sh[e] = s_co[3 * C + c];
    if constexpr (APPLY) { k1[e] = s_co[4 * C + c]; k2[e] = s_co[5 * C + c]; }
  }
  float a1[APPLY ? 1 : EPV], a2[APPLY ? 1 : EPV];
  if constexpr (!APPLY) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) { a1[e] = 0.f; a2[e] = 0.f; }
  }
  while (pix0 < npix) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pix = pix0 + u * stride;
      if (pix < npix) {
        if constexpr (APPLY) {
          typedef typename FV<T>::type V;
          st16((T*)p.dy + pix * p.PDY + cg * EPV,
               vec_from_f<T>(bn_relu_bwd_apply<V>(vec_to_f<T>(vd[u]), vec_to_f<T>(vy[u]), ldf<T>(sc), ldf<T>(sh), ldf<T>(k1), ldf<T>(k2))));
        } else {
#pragma unroll
          for (int e = 0; e < EPV; ++e) {
            const float yv = vy[u].get(e);
            const float act = __builtin_fmaf(yv, sc[e], sh[e]);
            const float dz = act > 0.f ? vd[u].get(e) : 0.f;
            const float xh = (yv - mean[e]) * istd[e];
            a1[e] += dz; a2[e] += dz * xh;
          }
        }
      }
    }
    pix0 += U * stride;
    if (pix0 < npix) load_batch(pix0);
  }
  if constexpr (!APPLY) {
    // block reduction over the ppb threads that share a channel group (fixed order), then one fixed-point add per channel
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      s_part[(threadIdx.x * NV + 0) * EPV + e] = a1[e];
      s_part[(threadIdx.x * NV + 1) * EPV + e] = a2[e];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NV * C; t += blockDim.x) {
      const int v = t / C, c = t - v * C;
      const int g = c / EPV, e = c - g * EPV;
      float sum = 0.f;
      for (int q = 0; q < ppb; ++q) sum += s_part[((q * G + g) * NV + v) * EPV + e];
      fx_add(p.sums + ((size_t)((blockIdx.x & (bn_sum_replicas(C) - 1)) * 2 + v) * C + c) * NUNET_FX_WORDS, sum);
    }
  }
}

// fat blocks: every block of the reduce pass ends with 2C fixed-point adds (8 pixels per thread, at most 512 / 1024 blocks)
static int bn_bwd_ipb() { return 8; }
static int bn_bwd_cap(bool apply) { return apply ? 1024 : 512; }
template <typename T, bool APPLY> static int launch_bn_bwd_t(const nunet_bn_bwd_desc* d, hipStream_t st) {
  BnBwdP p;
  p.da = d->da; p.PDA = d->PDA; p.y = d->y; p.PY = d->PY; p.mi = d->mean_invstd; p.gamma = d->gamma; p.beta = d->beta;
  p.sums = (long long*)d->sums; p.dgamma = d->dgamma; p.dbeta = d->dbeta; p.dbias = d->dbias; p.dy = d->dy; p.PDY = d->PDY;
  p.N = d->N; p.H = d->H; p.W = d->W; p.C = d->C;
  const int G = d->C / Tr<T>::EPV;
  const int64_t np = (int64_t)d->N * d->H * d->W;
  // fewer, fatter blocks: each block ends with 2C global atomics
  ProfScope ps(APPLY ? PC_BN_BWD_APPLY : PC_BN_BWD_REDUCE, 0, (double)np * d->C * sizeof(T) * (APPLY ? 3.0 : 2.0), st);
  // fat blocks: every block ends with C (2C) same-address global atomics
  NUNET_LAUNCH((bn_relu_bwd_kernel<T, APPLY>), dim3(grid_for(np, (256 / G) * bn_bwd_ipb(), bn_bwd_cap(APPLY))), dim3(256), 0, st, p);
  return nunet_check_launch(APPLY ? "bn_relu_bwd_apply" : "bn_relu_bwd_reduce");
}
template <typename T> static int launch_bn_bwd_reduce(const nunet_bn_bwd_desc* d, hipStream_t st) { return launch_bn_bwd_t<T, false>(d, st); }
template <typename T> static int launch_bn_bwd_apply(const nunet_bn_bwd_desc* d, hipStream_t st) { return launch_bn_bwd_t<T, true>(d, st); }

static int bn_bwd_check(const nunet_bn_bwd_desc* d, bool apply) {
  NUNET_REQUIRE(d && d->da && d->y && d->mean_invstd && d->gamma && d->beta && d->sums, "bn_relu_bwd: null pointer");
  const int epv = 16 / dtype_size(d->dtype);
  NUNET_REQUIRE(pow2(d->C) && d->C >= epv && d->C / epv <= 256 && d->C <= 512, "bn_relu_bwd: C=%d unsupported (power of two <= 512)", d->C);
  NUNET_REQUIRE(d->PY % epv == 0 && d->PDA % epv == 0, "bn_relu_bwd: pitch alignment");
  if (apply) NUNET_REQUIRE(d->dy && d->PDY % epv == 0, "bn_relu_bwd_apply: dy");
  return NUNET_OK;
}
extern "C" int nunet_bn_relu_bwd_reduce(const nunet_bn_bwd_desc* d, nunet_stream_t s) {
  int rc = bn_bwd_check(d, false);
  if (rc) return rc;
  return NUNET_DISPATCH(d->dtype, launch_bn_bwd_reduce, d, (hipStream_t)s);
}
extern "C" int nunet_bn_relu_bwd_apply(const nunet_bn_bwd_desc* d, nunet_stream_t s) {
  int rc = bn_bwd_check(d, true);
  if (rc) return rc;
  return NUNET_DISPATCH(d->dtype, launch_bn_bwd_apply, d, (hipStream_t)s);
}

// ---------------------------------------------------------------------------
// BatchNorm+ReLU backward REDUCE taken by the kernel that COMPLETES a gradient tensor, on the values it has just stored -
// instead of a separate pass (nunet_bn_relu_bwd_reduce) that would read the gradient and the raw conv output again.
// Used by the head backward (the last writer of x0_4's gradient, first kernel of the backward chain). The same fusion in
// the upsample- and pool-backward kernels was measured and dropped: those run thousands of small latency-bound blocks,
// and 2C fixed-point adds per block cost more (fused 21.9 us vs 9.4 + 8.6 us for the plain kernel + the fat-block reduce;
// round 3, again with at most 256 blocks and the list-scheduled executor: fused 17.6-25.9 us against 6.5-15.3 + 9.0-12.4).
// A thread's channel group is fixed (the launch geometry keeps grid stride % G == 0): coefficients and the two partial
// sums of its EPV channels live in registers; the block reduces them in a fixed order, then one fixed-point add each.
// ---------------------------------------------------------------------------
struct BnrP { const void* y; int py; const float* mi; const float* gamma; const float* beta; long long* sums; int C; };
template <typename T> struct BnrAcc {
  static constexpr int EPV = Tr<T>::EPV;
  typedef typename FV<T>::type V;
  V r1, r2;                                   // the only per-thread state: partial sums of this thread's EPV channels
  // LDS: [sc | sh | istd | mean * istd][C] coefficient table (a thread visits one or two elements: per-thread coefficient
  // registers would cost 32 VGPRs and halve the occupancy of a gather kernel that lives on it), then the reduction scratch
  static constexpr int LDS_FLOATS(int) { return 0; }
  __device__ __forceinline__ void init(const BnrP& b, float* s_tab) {
    for (int c = threadIdx.x; c < b.C; c += blockDim.x) {
      const float mean = b.mi[c], istd = b.mi[b.C + c];
      const float sc = b.gamma[c] * istd;
      s_tab[c] = sc; s_tab[b.C + c] = __builtin_fmaf(-mean, sc, b.beta[c]); s_tab[2 * b.C + c] = istd; s_tab[3 * b.C + c] = mean * istd;
    }
    r1 = V(0.f); r2 = V(0.f);
    __syncthreads();
  }
  __device__ __forceinline__ Vec16<T> fetch(const BnrP& b, int cg, long long pix) const { return ld16((const T*)b.y + pix * b.py + cg * EPV); }
  // `stored`: the gradient vector as written (rounded to T); yv: the raw conv output at the same pixel (fetch(), issued early)
  __device__ __forceinline__ void add(const BnrP& b, const float* s_tab, int cg, const Vec16<T>& yv, const Vec16<T>& stored) {
    const V y = vec_to_f<T>(yv), g = vec_to_f<T>(stored);
    const V sc = ldf<T>(&s_tab[cg * EPV]), sh = ldf<T>(&s_tab[b.C + cg * EPV]);
    const V istd = ldf<T>(&s_tab[2 * b.C + cg * EPV]), mis = ldf<T>(&s_tab[3 * b.C + cg * EPV]);
    const V act = __builtin_elementwise_fma(y, sc, sh);
    const V dz = act > V(0.f) ? g : V(0.f);
    r1 += dz;
    r2 += dz * __builtin_elementwise_fma(y, istd, -mis);      // dz * xhat
  }
  // Block reduction in a fixed order, then ONE fixed-point add per channel and sum: lanes of a wave that share a channel
  // group (lane % G when G < 64) are summed with xor-shuffles, the waves meet in LDS (s_part: waves x 2 x C floats).
  // Blocks of 1024 threads keep the number of adds per launch low: every block ends with 2C same-address atomics, and
  // a thousand small blocks hammering 64 cache lines cost more than the kernel itself.
  __device__ __forceinline__ void finish(const BnrP& b, float* s_part, int G) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (G < 64) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        if (off >= G) {
#pragma unroll
          for (int e = 0; e < EPV; ++e) { r1[e] += __shfl_xor(r1[e], off); r2[e] += __shfl_xor(r2[e], off); }
        }
      }
    }
    // after the shuffles lanes 0..min(G,64)-1 hold the wave's sums of channel groups (threadIdx.x % G)
    const int gl = G < 64 ? G : 64;
    if (lane < gl) {
      const int g = threadIdx.x % G;
#pragma unroll
      for (int e = 0; e < EPV; ++e) { s_part[(wv * 2 + 0) * b.C + g * EPV + e] = r1[e]; s_part[(wv * 2 + 1) * b.C + g * EPV + e] = r2[e]; }
    }
    __syncthreads();
    // waves that own channel group g: all of them when G <= 64, else waves wv with (wv * 64) % G == g - (g % 64)
    for (int t = threadIdx.x; t < 2 * b.C; t += blockDim.x) {
      const int v = t / b.C, c = t - v * b.C;
      float sum = 0.f;
      if (G <= 64) { for (int q = 0; q < nw; ++q) sum += s_part[(q * 2 + v) * b.C + c]; }
      else { const int g = c / EPV, per = G / 64; for (int q = (g / 64); q < nw; q += per) sum += s_part[(q * 2 + v) * b.C + c]; }
      fx_add(b.sums + ((size_t)((blockIdx.x & (bn_sum_replicas(b.C) - 1)) * 2 + v) * b.C + c) * NUNET_FX_WORDS, sum);
    }
  }
};
static int bnr_fill(BnrP& b, const nunet_bnr_desc* d, int C, int dtype) {
  b.y = d->y; b.py = d->PY; b.mi = d->mean_invstd; b.gamma = d->gamma; b.beta = d->beta; b.sums = (long long*)d->sums; b.C = C;
  NUNET_REQUIRE(d->y && d->mean_invstd && d->gamma && d->beta && d->sums && d->PY % (16 / dtype_size(dtype)) == 0 && d->PY >= C,
                "fused BN-backward reduce: y, mean/invstd, gamma, beta, sums and an aligned pitch are required");
  return NUNET_OK;
}

// ---------------------------------------------------------------------------
// MaxPool2d(2,2)
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, int PX, T* __restrict__ y, int PY, int N, int H, int W, int C, Dec4 dc) {
  constexpr int EPV = Tr<T>::EPV;
  const int G = C / EPV, H2 = H / 2, W2 = W / 2;
  const int64_t total = (int64_t)N * H2 * W2 * G;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int cg, qx, qy, n; long long q;
    dec4(dc, i, cg, q, qx, qy, n);
    const int64_t p00 = ((int64_t)n * H + 2 * qy) * W + 2 * qx;
    float mx[EPV];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const Vec16<T> v = ld16(x + (p00 + (k >> 1) * W + (k & 1)) * PX + cg * EPV);
#pragma unroll
      for (int e = 0; e < EPV; ++e) mx[e] = k == 0 ? v.get(e) : fmaxf(mx[e], v.get(e));
    }
    Vec16<T> o;
#pragma unroll
    for (int e = 0; e < EPV; ++e) o.set(e, mx[e]);
    st16(y + q * PY + cg * EPV, o);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x, int PX, const T* __restrict__ dy, int PDY, T* __restrict__ dx, int PDX, int accumulate, int N, int H, int W, int C, Dec4 dc) {
  constexpr int EPV = Tr<T>::EPV;
  const int G = C / EPV, H2 = H / 2, W2 = W / 2;
  const int64_t total = (int64_t)N * H2 * W2 * G;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int cg, qx, qy, n; long long q;
    dec4(dc, i, cg, q, qx, qy, n);
    const int64_t p00 = ((int64_t)n * H + 2 * qy) * W + 2 * qx;
    Vec16<T> v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ld16(x + (p00 + (k >> 1) * W + (k & 1)) * PX + cg * EPV);
    const Vec16<T> g = ld16(dy + q * PDY + cg * EPV);
    int am[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      float m = v[0].get(e);
      int a = 0;
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float f = v[k].get(e);
        if (f > m) { m = f; a = k; }  // first maximum wins (PyTorch scan order)
      }
      am[e] = a;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      T* q4 = dx + (p00 + (k >> 1) * W + (k & 1)) * PDX + cg * EPV;
      Vec16<T> o = accumulate ? ld16(q4) : zero16<T>();
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const float base = accumulate ? o.get(e) : 0.f;
        o.set(e, am[e] == k ? base + g.get(e) : base);
      }
      st16(q4, o);
    }
  }
}
template <typename T> static int launch_maxpool_fwd(int N, int H, int W, int C, const void* x, int PX, void* y, int PY, hipStream_t st) {
  const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / Tr<T>::EPV);
  ProfScope ps(PC_POOL, 0, (double)N * H * W * C * sizeof(T) * 1.25, st);
  NUNET_LAUNCH((maxpool_fwd_kernel<T>), dim3(grid_for(total, 256)), dim3(256), 0, st, (const T*)x, PX, (T*)y, PY, N, H, W, C, make_dec4(total, C / Tr<T>::EPV, W / 2, H / 2));
  return nunet_check_launch("maxpool_fwd");
}
template <typename T> static int launch_maxpool_bwd(int N, int H, int W, int C, const void* x, int PX, const void* dy, int PDY, void* dx, int PDX, int acc, hipStream_t st) {
  const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / Tr<T>::EPV);
  ProfScope ps(PC_POOL, 0, (double)N * H * W * C * sizeof(T) * (acc ? 3.25 : 2.25), st);
  NUNET_LAUNCH((maxpool_bwd_kernel<T>), dim3(grid_for(total, 256)), dim3(256), 0, st, (const T*)x, PX, (const T*)dy, PDY, (T*)dx, PDX, acc, N, H, W, C, make_dec4(total, C / Tr<T>::EPV, W / 2, H / 2));
  return nunet_check_launch("maxpool_bwd");
}
static int ew_check(const char* what, int dtype, int N, int H, int W, int C, int p0, int p1) {
  const int epv = 16 / dtype_size(dtype);
  NUNET_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % epv == 0, "%s: bad shape N=%d H=%d W=%d C=%d", what, N, H, W, C);
  NUNET_REQUIRE(p0 % epv == 0 && p1 % epv == 0 && p0 >= C && p1 >= C, "%s: pitch", what);
  return NUNET_OK;
}
extern "C" int nunet_maxpool2x2_fwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* x, int32_t PX, void* y, int32_t PY, nunet_stream_t s) {
  int rc = ew_check("maxpool_fwd", dtype, N, H, W, C, PX, PY);
  if (rc) return rc;
  NUNET_REQUIRE(x && y && H % 2 == 0 && W % 2 == 0, "maxpool_fwd: needs even H, W");
  return NUNET_DISPATCH(dtype, launch_maxpool_fwd, N, H, W, C, x, PX, y, PY, (hipStream_t)s);
}
extern "C" int nunet_maxpool2x2_bwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* x, int32_t PX, const void* dy, int32_t PDY, void* dx, int32_t PDX, int32_t accumulate, nunet_stream_t s) {
  int rc = ew_check("maxpool_bwd", dtype, N, H, W, C, PX, PDX);
  if (rc) return rc;
  NUNET_REQUIRE(x && dy && dx && H % 2 == 0 && W % 2 == 0 && PDY % (16 / dtype_size(dtype)) == 0, "maxpool_bwd: bad args");
  return NUNET_DISPATCH(dtype, launch_maxpool_bwd, N, H, W, C, x, PX, dy, PDY, dx, PDX, accumulate, (hipStream_t)s);
}

// ---------------------------------------------------------------------------
// Upsample x2, bilinear, align_corners=True
// ---------------------------------------------------------------------------
// (contraction off: whether `src - i0` fuses with the multiply into an fma is otherwise decided per call site, and the forward
//  pass, its backward and the form fused into the BatchNorm launch must agree on the weights to the last bit)
__device__ __forceinline__ void up_taps(int dst, float scale, int n_in, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
  const float src = scale * (float)dst;
  i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}
// the four-tap interpolation, one explicit operation order for every kernel that evaluates it (the stand-alone upsample and
// the form fused into the BatchNorm launch must round identically)
__device__ __forceinline__ float up_lerp(float v00, float v01, float v10, float v11, float ly, float lx) {
#pragma clang fp contract(off)
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float top = __builtin_fmaf(lx, v01, hx * v00), bot = __builtin_fmaf(lx, v11, hx * v10);
  return __builtin_fmaf(ly, bot, hy * top);
}
template <typename T>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const T* __restrict__ x, int PX, T* __restrict__ y, int PY, int N, int H, int W, int C, Dec4 dc) {
  constexpr int EPV = Tr<T>::EPV;
  const int G = C / EPV, HO = 2 * H, WO = 2 * W;
  const float sy = HO > 1 ? (float)(H - 1) / (float)(HO - 1) : 0.f;
  const float sx = WO > 1 ? (float)(W - 1) / (float)(WO - 1) : 0.f;
  const int64_t total = (int64_t)N * HO * WO * G;
  // block -> 256 consecutive outputs through xcd_remap: every XCD takes one contiguous range of each pass, so the output rows
  // that interpolate from the same source rows meet in one L2 (dealt round-robin, every L2 fetched nearly the whole source).
  // The map is taken over the blocks a pass really has: a short last pass remapped over the whole grid would land on the
  // first XCD alone (items 0 .. rest - 1 of the map are XCD 0's), which then runs twice as long as the others.
  const int64_t nblk = (total + 255) / 256;
  for (int64_t base = 0; base < nblk; base += gridDim.x) {
    const int gp = (int)(nblk - base < (int64_t)gridDim.x ? nblk - base : (int64_t)gridDim.x);
    if ((int)blockIdx.x >= gp) break;
    const int64_t i = (base + xcd_remap((int)blockIdx.x, gp)) * 256 + threadIdx.x;
    if (i >= total) break;
    int cg, ox, oy, n; long long o;
    dec4(dc, i, cg, o, ox, oy, n);
    int y0, y1, x0, x1; float ly, lx;
    up_taps(oy, sy, H, y0, y1, ly);
    up_taps(ox, sx, W, x0, x1, lx);
    const T* b = x + (int64_t)n * H * W * PX + cg * EPV;
    const Vec16<T> v00 = ld16(b + ((int64_t)y0 * W + x0) * PX), v01 = ld16(b + ((int64_t)y0 * W + x1) * PX);
    const Vec16<T> v10 = ld16(b + ((int64_t)y1 * W + x0) * PX), v11 = ld16(b + ((int64_t)y1 * W + x1) * PX);
    Vec16<T> r;
#pragma unroll
    for (int e = 0; e < EPV; ++e) r.set(e, up_lerp(v00.get(e), v01.get(e), v10.get(e), v11.get(e), ly, lx));
    st16(y + o * PY + cg * EPV, r);
  }
}
// One tap of the backward sum, acc[e] <- acc[e] + w * g[e], with the operation order written out (contraction off, as in up_lerp):
// whether the multiply fuses with the add is otherwise the compiler's choice per call site, and it does not choose the same for
// every tap. The thread-per-output kernel, compiled with `acc[e] += w * g` under the default contraction, came out with fused
// multiply-adds except at a few (tap, element) sites that its vectoriser had split into a multiply and an add; the same statement
// in the tiled kernel split at other sites (1 ulp of fp32: 1 fp32 output in 5, 1 fp16 output in 25000). Every result recorded so
// far was computed with that build, so its sites are kept, in this one function that both backward kernels take every tap through:
// they cannot differ from each other, and a later compiler cannot move a rounding. t = 5 j + k is the tap's index in the window.
// How the table was obtained: from the ISA of the three instantiations of that kernel (hipcc -S --cuda-device-only), following
// each element's accumulator through its 25 v_pk_fma_f32 / v_pk_add_f32(v_mul) steps; bf16 and fp16 have the same sites, fp32
// only the second row. How it was checked: the same walk over the ISA of this file's gather kernel gives the same sites for all
// three types, and bench.py --dump-outputs (which reaches the sites through the tiled kernel) is byte-identical to that build in
// bf16, fp16 and fp32 (profiles/r05_summary.md, 1). t is a constant in the gather kernel. In the tiled kernel, whose row loop is
// rolled, it is a run-time value: the two or four elements with sites compute both forms and select (a scalar branch around that
// for the taps without a site measured slower, 9.9 against 9.1 us per launch, as did unrolling the rows, which spills).
template <int EPV> __device__ __forceinline__ bool up_tap_split(int t, int e) {
  return (e >= EPV - 2 && t >= 14 && t <= 21) || (EPV == 8 && e < 2 && (t == 3 || t == 14));
}
template <typename T> __device__ __forceinline__ void up_bwd_tap(float* acc, int t, float w, const Vec16<T>& g) {
#pragma clang fp contract(off)
  constexpr int EPV = Tr<T>::EPV;
#pragma unroll
  for (int e = 0; e < EPV; ++e) {
    const float ge = g.get(e);
    if (e >= EPV - 2 || (EPV == 8 && e < 2)) {     // the elements that have sites: both forms and a select where t is a run-time value
      const float p = w * ge;
      const float two = acc[e] + p, one = __builtin_fmaf(w, ge, acc[e]);
      acc[e] = up_tap_split<EPV>(t, e) ? two : one;
    } else acc[e] = __builtin_fmaf(w, ge, acc[e]);
  }
}
// The high-res rows that interpolate from low-res row ic have source coordinate in (ic-1, ic+1): an open interval
// of 2/sc = 4 + 2/(n_in-1) < 5 output rows, so it holds at most 5 of them, found among the 6 starting at
// floor((ic-1)/sc). Weights come from the same up_taps() as the forward pass. n_in >= 4. One function for both
// backward kernels: base and weights of a row / column are the same bits in either.
__device__ __forceinline__ void up_window(int ic, float sc, int n_in, int n_out, int& base, float* w5) {
  base = max(0, (int)floorf((float)(ic - 1) / sc));
  float w6[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    int i0, i1; float l;
    up_taps(min(base + j, n_out - 1), sc, n_in, i0, i1, l);
    w6[j] = base + j < n_out ? (i0 == ic ? 1.f - l : 0.f) + (i1 == ic ? l : 0.f) : 0.f;
  }
  const bool shift = w6[0] == 0.f;
#pragma unroll
  for (int j = 0; j < 5; ++j) w5[j] = shift ? w6[j + 1] : w6[j];
  base += shift ? 1 : 0;
}
// gather form of the transposed interpolation: one thread per low-res pixel and 16-byte channel group, every tap a global
// load. Serves extents below 4 (the general loop) and is what the tiled form below is tested against, byte for byte.
template <typename T>
__global__ __launch_bounds__(256) void upsample_bwd_gather_kernel(const T* __restrict__ dy, int PDY, T* __restrict__ dx, int PDX, int accumulate, int N, int H, int W, int C, Dec4 dc) {
  constexpr int EPV = Tr<T>::EPV;
  const int G = C / EPV, HO = 2 * H, WO = 2 * W;
  const float sy = HO > 1 ? (float)(H - 1) / (float)(HO - 1) : 0.f;
  const float sx = WO > 1 ? (float)(W - 1) / (float)(WO - 1) : 0.f;
  const int64_t total = (int64_t)N * H * W * G;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int cg, ix, iy, n; long long o;
    dec4(dc, i, cg, o, ix, iy, n);
    const T* b = dy + (int64_t)n * HO * WO * PDY + cg * EPV;
    float acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;
    if (H >= 4 && W >= 4) {
      // the 5x5 window (up_window) is read with unconditional (clamped, zero-weighted) loads that the compiler can keep in
      // flight together, in the same (oy, ox) order as the general loop below
      int yb, xb; float wy[5], wx[5];
      up_window(iy, sy, H, HO, yb, wy);
      up_window(ix, sx, W, WO, xb, wx);
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int oy = min(yb + j, HO - 1);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int ox = min(xb + k, WO - 1);
          const Vec16<T> g = ld16(b + ((int64_t)oy * WO + ox) * PDY);
          const float w = wy[j] * wx[k];
          up_bwd_tap<T>(acc, 5 * j + k, w, g);
        }
      }
    } else {
    int ylo = 0, yhi = HO - 1, xlo = 0, xhi = WO - 1;
    if (sy > 0.f) { ylo = max(0, (int)floorf((float)(iy - 1) / sy) - 1); yhi = min(HO - 1, (int)ceilf((float)(iy + 1) / sy) + 1); }
    if (sx > 0.f) { xlo = max(0, (int)floorf((float)(ix - 1) / sx) - 1); xhi = min(WO - 1, (int)ceilf((float)(ix + 1) / sx) + 1); }
    for (int oy = ylo; oy <= yhi; ++oy) {
      int y0, y1; float ly;
      up_taps(oy, sy, H, y0, y1, ly);
      const float wy = (y0 == iy ? 1.f - ly : 0.f) + (y1 == iy ? ly : 0.f);
      if (wy == 0.f) continue;
      for (int ox = xlo; ox <= xhi; ++ox) {
        int x0, x1; float lx;
        up_taps(ox, sx, W, x0, x1, lx);
        const float wx = (x0 == ix ? 1.f - lx : 0.f) + (x1 == ix ? lx : 0.f);
        if (wx == 0.f) continue;
        const Vec16<T> g = ld16(b + ((int64_t)oy * WO + ox) * PDY);
        const float w = wy * wx;
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc[e] += w * g.get(e);
      }
    }
    }
    T* q = dx + o * PDX + cg * EPV;
    Vec16<T> r = accumulate ? ld16(q) : zero16<T>();
#pragma unroll
    for (int e = 0; e < EPV; ++e) r.set(e, (accumulate ? r.get(e) : 0.f) + acc[e]);
    st16(q, r);
  }
}
// Tiled form of the transposed interpolation, H >= 4 && W >= 4. A work item is (image, band of <= UPB_TILE low-res rows, band of
// <= UPB_TILE low-res columns, slab of <= UPB_SLAB 16-byte channel groups), items in raster order [N][row band][column band][slab]
// and dealt to the XCDs in contiguous ranges (xcd_remap): the two 64-byte halves of a 128-byte pixel and the halos of neighbouring
// bands are read by workgroups that share an L2. The workgroup stages the high-res window of its item in LDS once, with coalesced
// 16-byte loads that are all in flight together - rows from the first row's window base to min(last row's base + 4, HO - 1),
// columns likewise - and every thread then forms one (low-res pixel, channel group) output from 25 LDS reads: the clamped
// addresses, the weights (up_window, once per row and column of the item, through LDS), the (j, k) order, zero-weight taps
// included (0 * inf must stay NaN: the fp16 overflow check relies on it) and the final read-add-round are those of the gather
// kernel, which read each of those lines from memory up to 25 times from neighbouring threads and 2.7 times from HBM.
// Window extent: the exact base of row ic is floor((ic - 1) (2 + 1 / (n - 1))) + 1 (0 for ic = 0), so over a band of t <= n rows
// it grows by at most 2 (t - 1) + 1 and the window holds at most 2 t + 4 high-res rows; the fp32 coordinate can move a base by
// one while n <= 2^20 (the launcher's condition): UPB_WIN = 2 t + 5 = 21 at t = 8.
// LDS: 21 * 21 * 64 B = 27.6 KB + 0.4 KB of tables: five workgroups fit a CU's 160 KB.
#define UPB_TILE 8
#define UPB_SLAB 4
#define UPB_WIN (2 * UPB_TILE + 5)
#define UPB_STAGE ((UPB_WIN * UPB_WIN * UPB_SLAB + 255) / 256)     // staging loads per thread (7)
#define UPB_GRID_CAP 4096
struct UpbShape { int tiled, TR, TC, SG, nbr, nbc, nsl, grid, passes; long long items; };
static inline UpbShape upb_shape(int N, int H, int W, int G, int PDY, int esize, bool backward, bool force_gather) {
  UpbShape u; memset(&u, 0, sizeof(u));
  // (tiled: 32-bit offsets within an image of dy; the gather kernel takes what is larger)
  if (backward && !force_gather && H >= 4 && W >= 4 && H <= (1 << 20) && W <= (1 << 20) && 4ll * H * W * PDY * esize < (1ll << 31)) {
    u.nbr = ceil_div(H, UPB_TILE); u.TR = ceil_div(H, u.nbr); u.nbr = ceil_div(H, u.TR);     // bands of equal height (the last may be shorter)
    u.nbc = ceil_div(W, UPB_TILE); u.TC = ceil_div(W, u.nbc); u.nbc = ceil_div(W, u.TC);
    u.SG = G < UPB_SLAB ? G : UPB_SLAB; u.nsl = ceil_div(G, u.SG);
    u.items = (long long)N * u.nbr * u.nbc * u.nsl;
    u.tiled = u.items < (1ll << 31) && make_dec4(u.items, u.nsl, u.nbc, u.nbr).fast ? 1 : 0;
  }
  if (!u.tiled) {     // thread per output, 256 outputs a block (the forward kernel and the gather kernel)
    u.TR = u.TC = u.SG = u.nbr = u.nbc = u.nsl = 0;
    u.items = ceil_div64((long long)N * H * W * G * (backward ? 1 : 4), 256);
  }
  u.grid = (int)(u.items > UPB_GRID_CAP ? UPB_GRID_CAP : (u.items < 1 ? 1 : u.items));
  u.passes = (int)ceil_div64(u.items, u.grid);
  return u;
}
template <typename T>
__global__ __launch_bounds__(256, 5) void upsample_bwd_kernel(const T* __restrict__ dy, int PDY, T* __restrict__ dx, int PDX, int accumulate, int N, int H, int W, int C,
                                                           int TR, int TC, int SG, long long items, Dec4 dc) {
  constexpr int EPV = Tr<T>::EPV;
  __shared__ u32x4 s_g[UPB_WIN * UPB_WIN * UPB_SLAB];       // [row][column][UPB_SLAB] of the item's window
  __shared__ float s_w[2][UPB_TILE][5];                     // window weights of the item's rows [0] and columns [1]
  __shared__ int s_b[2][UPB_TILE];                          // ... and their window bases
  const int G = C / EPV, HO = 2 * H, WO = 2 * W;
  const float sy = (float)(H - 1) / (float)(HO - 1);
  const float sx = (float)(W - 1) / (float)(WO - 1);
  const int tid = threadIdx.x;
  const int gl = tid & (UPB_SLAB - 1);                      // channel group within the slab, staging and output alike
  const int lr = tid >> 5, lc = (tid >> 2) & 7;             // output pixel of the thread within the item (8 x 8 x UPB_SLAB threads)
  for (long long base = 0; base < items; base += gridDim.x) {
    // (the map over the workgroups this pass has items for: a short last pass goes to all XCDs, as in upsample_fwd_kernel)
    const int gp = (int)(items - base < (long long)gridDim.x ? items - base : (long long)gridDim.x);
    if ((int)blockIdx.x >= gp) break;
    const long long it = base + xcd_remap((int)blockIdx.x, gp);
    // item -> (slab, column band, row band, image): the multiply form of dec4 alone (upb_shape takes the tiled kernel only
    // where it is exact), the 64-bit divisions of the general form cost registers that a fifth workgroup per CU needs
    const int ii = (int)it;
    const int t0 = dec_div(ii, dc.iG), sl = ii - t0 * dc.G;
    const int t1 = dec_div(t0, dc.iW), bc = t0 - t1 * dc.W;
    const int n = dec_div(t1, dc.iH), br = t1 - n * dc.H;
    const int r0 = br * TR, c0 = bc * TC, g0 = sl * SG;
    const int nr = min(TR, H - r0), nc = min(TC, W - c0), ng = min(SG, G - g0);
    if (tid < nr) {
      int base; float w5[5];
      up_window(r0 + tid, sy, H, HO, base, w5);
      s_b[0][tid] = base;
#pragma unroll
      for (int j = 0; j < 5; ++j) s_w[0][tid][j] = w5[j];
    } else if (tid >= 64 && tid - 64 < nc) {
      int base; float w5[5];
      up_window(c0 + tid - 64, sx, W, WO, base, w5);
      s_b[1][tid - 64] = base;
#pragma unroll
      for (int j = 0; j < 5; ++j) s_w[1][tid - 64][j] = w5[j];
    }
    __syncthreads();
    int y_lo = s_b[0][0], y_hi = y_lo, x_lo = s_b[1][0], x_hi = x_lo;
    for (int j = 1; j < nr; ++j) { y_lo = min(y_lo, s_b[0][j]); y_hi = max(y_hi, s_b[0][j]); }
    for (int j = 1; j < nc; ++j) { x_lo = min(x_lo, s_b[1][j]); x_hi = max(x_hi, s_b[1][j]); }
    y_hi = min(y_hi + 4, HO - 1); x_hi = min(x_hi + 4, WO - 1);
    const int wr = min(y_hi - y_lo + 1, UPB_WIN), wc = min(x_hi - x_lo + 1, UPB_WIN);     // (the min never binds, see above)
    // stage: flat index t = (row * wc + column) * UPB_SLAB + group; row = t / (wc * UPB_SLAB) by a float reciprocal (t < 2048,
    // divisor <= 84: (t + 0.5) / d stays >= 0.5 / 84 away from an integer, fp32 rounding moves it by < 2^-18)
    const int per_row = wc * UPB_SLAB, nst = wr * per_row;
    const float inv_row = 1.f / (float)per_row;
    const T* b = dy + ((int64_t)n * HO * WO) * PDY + g0 * EPV;     // (uniform; an image's byte offsets fit 31 bits, upb_shape)
    Vec16<T> v[UPB_STAGE];
#pragma unroll
    for (int k = 0; k < UPB_STAGE; ++k) {
      const int t = tid + k * 256;
      if (t < nst && gl < ng) {
        const int r = (int)(((float)t + 0.5f) * inv_row);
        const int c = (t - r * per_row) >> 2;
        v[k] = ld16(b + (unsigned)(((y_lo + r) * WO + (x_lo + c)) * PDY + gl * EPV));
      }
    }
#pragma unroll
    for (int k = 0; k < UPB_STAGE; ++k) {
      const int t = tid + k * 256;
      if (t < nst && gl < ng) s_g[t] = v[k].raw;
    }
    const bool live = lr < nr && lc < nc && gl < ng;
    const long long o = ((long long)n * H + (r0 + lr)) * W + (c0 + lc);
    T* q = dx + o * PDX + (g0 + gl) * EPV;
    Vec16<T> r = (accumulate && live) ? ld16(q) : zero16<T>();     // (in flight while the taps are summed)
    __syncthreads();
    if (live) {
      float acc[EPV];
#pragma unroll
      for (int e = 0; e < EPV; ++e) acc[e] = 0.f;
      float wx[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) wx[k] = s_w[1][lc][k];
      const int yb = s_b[0][lr], xb = s_b[1][lc];
      // (one window row at a time: unrolled over j the compiler hoists all 25 reads, 100 registers, and a fifth workgroup no
      //  longer fits the CU)
#pragma unroll 1
      for (int j = 0; j < 5; ++j) {
        const int oy = min(yb + j, HO - 1);
        const float wyj = s_w[0][lr][j];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int ox = min(xb + k, WO - 1);
          Vec16<T> g;
          g.raw = s_g[((oy - y_lo) * wc + (ox - x_lo)) * UPB_SLAB + gl];
          const float w = wyj * wx[k];
          up_bwd_tap<T>(acc, 5 * j + k, w, g);
        }
      }
#pragma unroll
      for (int e = 0; e < EPV; ++e) r.set(e, (accumulate ? r.get(e) : 0.f) + acc[e]);
      st16(q, r);
    }
    __syncthreads();     // the next item rewrites the tables and the window
  }
}
template <typename T> static int launch_up_fwd(int N, int H, int W, int C, const void* x, int PX, void* y, int PY, hipStream_t st) {
  const int64_t total = (int64_t)N * 4 * H * W * (C / Tr<T>::EPV);
  ProfScope ps(PC_UP_FWD, 0, (double)N * H * W * C * sizeof(T) * 5.0, st);
  const UpbShape u = upb_shape(N, H, W, C / Tr<T>::EPV, PX, (int)sizeof(T), false, false);
  NUNET_LAUNCH((upsample_fwd_kernel<T>), dim3(u.grid), dim3(256), 0, st, (const T*)x, PX, (T*)y, PY, N, H, W, C, make_dec4(total, C / Tr<T>::EPV, 2 * W, 2 * H));
  return nunet_check_launch("upsample_fwd");
}
template <typename T> static int launch_up_bwd(int N, int H, int W, int C, const void* dy, int PDY, void* dx, int PDX, int acc, bool force_gather, hipStream_t st) {
  const int64_t total = (int64_t)N * H * W * (C / Tr<T>::EPV);
  ProfScope ps(PC_UP_BWD, 0, (double)N * H * W * C * sizeof(T) * (acc ? 6.0 : 5.0), st);
  const UpbShape u = upb_shape(N, H, W, C / Tr<T>::EPV, PDY, (int)sizeof(T), true, force_gather);
  if (u.tiled)
    NUNET_LAUNCH((upsample_bwd_kernel<T>), dim3(u.grid), dim3(256), 0, st, (const T*)dy, PDY, (T*)dx, PDX, acc, N, H, W, C, u.TR, u.TC, u.SG, u.items,
                 make_dec4(u.items, u.nsl, u.nbc, u.nbr));
  else
    NUNET_LAUNCH((upsample_bwd_gather_kernel<T>), dim3(u.grid), dim3(256), 0, st, (const T*)dy, PDY, (T*)dx, PDX, acc, N, H, W, C, make_dec4(total, C / Tr<T>::EPV, W, H));
  return nunet_check_launch("upsample_bwd");
}
extern "C" int nunet_upsample2x_fwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* x, int32_t PX, void* y, int32_t PY, nunet_stream_t s) {
  int rc = ew_check("upsample_fwd", dtype, N, H, W, C, PX, PY);
  if (rc) return rc;
  NUNET_REQUIRE(x && y, "upsample_fwd: null pointer");
  return NUNET_DISPATCH(dtype, launch_up_fwd, N, H, W, C, x, PX, y, PY, (hipStream_t)s);
}
extern "C" int nunet_upsample2x_bwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* dy, int32_t PDY, void* dx, int32_t PDX, int32_t accumulate, nunet_stream_t s) {
  int rc = ew_check("upsample_bwd", dtype, N, H, W, C, PDY, PDX);
  if (rc) return rc;
  NUNET_REQUIRE(dy && dx, "upsample_bwd: null pointer");
  return NUNET_DISPATCH(dtype, launch_up_bwd, N, H, W, C, dy, PDY, dx, PDX, accumulate, false, (hipStream_t)s);
}
extern "C" int nunet_upsample2x_bwd_gather(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, const void* dy, int32_t PDY, void* dx, int32_t PDX, int32_t accumulate, nunet_stream_t s) {
  int rc = ew_check("upsample_bwd_gather", dtype, N, H, W, C, PDY, PDX);
  if (rc) return rc;
  NUNET_REQUIRE(dy && dx, "upsample_bwd_gather: null pointer");
  return NUNET_DISPATCH(dtype, launch_up_bwd, N, H, W, C, dy, PDY, dx, PDX, accumulate, true, (hipStream_t)s);
}
extern "C" int nunet_upsample_launch_info(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t backward, nunet_upsample_launch_info_t* out) {
  NUNET_REQUIRE(out, "upsample_launch_info: null pointer");
  int rc = ew_check("upsample_launch_info", dtype, N, H, W, C, C, C);
  if (rc) return rc;
  const UpbShape u = upb_shape(N, H, W, C / (16 / dtype_size(dtype)), C, dtype_size(dtype), backward != 0, false);
  out->tiled = u.tiled; out->workgroups = u.grid; out->passes = u.passes; out->items = u.items;
  out->reserved = 0; out->TR = u.TR; out->TC = u.TC; out->SG = u.SG; out->lds_bytes = u.tiled ? (int32_t)(UPB_WIN * UPB_WIN * UPB_SLAB * 16 + 2 * UPB_TILE * 6 * 4) : 0;
  return NUNET_OK;
}
extern "C" int32_t nunet_xcd_remap_host(int32_t b, int32_t G) { return xcd_remap(b, G); }

// ---------------------------------------------------------------------------
// 1x1 heads. Lane = channel: 32-lane half-waves walk pixels.
// ---------------------------------------------------------------------------
#define HEAD_MAXK 8
// A logit is ONE chain acc = fma(x[c], w[k][c], acc) over c ascending from acc = 0, then + b[k]: both forward kernels below
// evaluate exactly that chain, so they leave the same bits.
// Thread per pixel. CT = 32 (the heads of this network): the pixel's 32 / EPV vectors are all requested before the first use,
// fully unrolled; CT = 0: any C <= 64, the same with the vectors beyond C predicated off. (The rolled loop of dependent 16-byte
// loads this replaces moved 1 TB/s.)
template <typename T, int CT>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ x, int PX, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ logits, int N, int H, int W, int C_, int K) {
  constexpr int EPV = Tr<T>::EPV;
  constexpr int NV = (CT ? CT : 64) / EPV;
  const int C = CT ? CT : C_;
  __shared__ float s_w[HEAD_MAXK * 64];
  for (int i = threadIdx.x; i < K * C; i += blockDim.x) s_w[i] = w[i];
  __syncthreads();
  const int64_t hw = (int64_t)H * W, npix = (int64_t)N * hw;
  for (int64_t pix = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; pix < npix; pix += (int64_t)gridDim.x * blockDim.x) {
    Vec16<T> v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (CT || i * EPV < C) v[i] = ld16(x + pix * PX + i * EPV);
    float xf[NV * EPV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
      for (int e = 0; e < EPV; ++e) xf[i * EPV + e] = v[i].get(e);
    }
    const int n = npix < (1ll << 31) ? (int)((unsigned)pix / (unsigned)hw) : (int)(pix / hw);
    const int64_t rem = pix - n * hw;
    // class by class, the weights from LDS (a rolled loop: unrolled over the classes, the compiler keeps all K * C weights in
    // registers across the pixel loop - 256 of them, one wave per SIMD)
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < NV * EPV; ++c)
        if (CT || c < C) acc = __builtin_fmaf(xf[c], s_w[k * C + c], acc);
      logits[((int64_t)n * K + k) * hw + rem] = acc + b[k];
    }
  }
}
// BatchNorm + ReLU of a block output AND the 1x1 head on it, one launch: bn_relu_fwd_kernel's un-pooled role (same thread map:
// the G = C / EPV lanes of a pixel are neighbours, every 16-byte load and store of y and of the slot is part of a dense run;
// same prologue, same bn_relu_apply), then the head from the value as ROUNDED to the storage type - what head_fwd_kernel would
// read back from the slot. The logit's fma chain walks the pixel's G lanes in channel order: lane g takes the sum from lane
// g - 1 (a shuffle), runs its EPV channels and hands it on; lane G - 1 adds the bias and stores. KT = compile-time class count
// (0: K <= HEAD_MAXK at run time).
struct HeadP { const float* w; const float* b; float* logits; int K; };
template <typename T, int KT>
__global__ __launch_bounds__(256) void head_fwd_bn_kernel(BnFwdP p, HeadP h) {
  constexpr int EPV = Tr<T>::EPV;
  constexpr int KM = KT > 0 ? KT : HEAD_MAXK;
  typedef typename FV<T>::type V;
  __shared__ __attribute__((aligned(16))) float s_sc[64], s_sh[64];
  const int G = p.C / EPV;  // 256 % G == 0 and 64 % G == 0: a pixel's lanes sit in one wave
  const int cg = threadIdx.x % G;
  const int K = KT > 0 ? KT : h.K;
  const float M = (float)p.N * p.H * p.W;
  constexpr int U = 4;   // 16-byte loads kept in flight per thread
  const int ppb = blockDim.x / G, pl = threadIdx.x / G;
  const int hw = p.H * p.W;
  const int64_t npix = (int64_t)p.N * hw;      // < 2^31 (checked on the host)
  const int64_t stride = (int64_t)gridDim.x * ppb;
  Vec16<T> v[U];
  auto load_batch = [&](int64_t p0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pix = p0 + u * stride;
      if (pix < npix) v[u] = ld16((const T*)p.y + pix * p.PY + cg * EPV);
    }
  };
  // first batch of loads and the lane's head weights ahead of the coefficient prologue (latencies overlap)
  int64_t pix0 = (int64_t)blockIdx.x * ppb + pl;
  if (pix0 < npix) load_batch(pix0);
  float wk[KM][EPV];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) wk[k][e] = k < K ? h.w[k * p.C + cg * EPV + e] : 0.f;
  }
  bn_fwd_prologue(p, M, s_sc, s_sh);
  const V sc = ldf<T>(&s_sc[cg * EPV]), sh = ldf<T>(&s_sh[cg * EPV]);
  while (pix0 < npix) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pix = pix0 + u * stride;
      const bool live = pix < npix;       // the same in all G lanes of a pixel; the shuffles below run in every lane
      const Vec16<T> o = vec_from_f<T>(bn_relu_apply<V>(vec_to_f<T>(v[u]), sc, sh));
      if (live) st16((T*)p.a + pix * p.PA + cg * EPV, o);
      float acc[KM];
#pragma unroll
      for (int k = 0; k < KM; ++k) acc[k] = 0.f;
      for (int g = 0; g < G; ++g) {
        float t[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) t[k] = g > 0 ? __shfl_up(acc[k], 1) : 0.f;
        if (cg == g) {
#pragma unroll
          for (int k = 0; k < KM; ++k) acc[k] = t[k];
#pragma unroll
          for (int e = 0; e < EPV; ++e) {
            const float xv = o.get(e);
#pragma unroll
            for (int k = 0; k < KM; ++k)
              if (KT > 0 || k < K) acc[k] = __builtin_fmaf(xv, wk[k][e], acc[k]);
          }
        }
      }
      if (live && cg == G - 1) {
        const int n = (int)((unsigned)pix / (unsigned)hw);
        const int rem = (int)pix - n * hw;
#pragma unroll
        for (int k = 0; k < KM; ++k)
          if (KT > 0 || k < K) h.logits[((int64_t)n * K + k) * hw + rem] = acc[k] + h.b[k];
      }
    }
    pix0 += U * stride;
    if (pix0 < npix) load_batch(pix0);
  }
}
template <typename T, int KT, bool BNR>
__global__ __launch_bounds__(256) void head_bwd_kernel(const T* __restrict__ x, int PX, const float* __restrict__ w, const float* __restrict__ dl, T* __restrict__ dx, int PDX, int accumulate, float* __restrict__ dw, int N, int H, int W, int C, int K, BnrP bn) {
  // C == 32. A thread owns one 16-byte channel group (EPV channels) of a pixel; G = 32/EPV threads
  // cover a pixel. dW/db partials live in registers (KT = compile-time class count, 0 = generic)
  // and meet through LDS once per block.
  constexpr int EPV = Tr<T>::EPV;
  constexpr int G = 32 / EPV;
  constexpr int KM = KT > 0 ? KT : HEAD_MAXK;
  __shared__ float s_dw[4 * (HEAD_MAXK * 32 + HEAD_MAXK)];   // per wave
  const int cg = threadIdx.x % G, pl = threadIdx.x / G, ppb = blockDim.x / G;
  __shared__ __attribute__((aligned(16))) float s_part[BNR ? 4096 : 1];   // waves x 2 x C floats (BnrAcc::finish)
  __shared__ __attribute__((aligned(16))) float s_tab[BNR ? 4 * 32 : 1];
  BnrAcc<T> ba;
  if constexpr (BNR) ba.init(bn, s_tab);
  float wk[KM][EPV], aw[KM][EPV], ab[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    ab[k] = 0.f;
#pragma unroll
    for (int e = 0; e < EPV; ++e) { wk[k][e] = k < K ? w[k * C + cg * EPV + e] : 0.f; aw[k][e] = 0.f; }
  }
  const int hw = H * W;
  const int64_t npix = (int64_t)N * hw;
  // U pixels per thread and pass, every load of a pass issued before the first use (the kernel opens the backward
  // pass alone on the device, so its latency is the step's)
  constexpr int U = 4;
  const int64_t stride = (int64_t)gridDim.x * ppb;
  for (int64_t pix0 = (int64_t)blockIdx.x * ppb + pl; pix0 < npix; pix0 += U * stride) {
    Vec16<T> xv[U], ov[U], yb[BNR ? U : 1];
    float d[U][KM];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pix = pix0 + u * stride;
      if (pix < npix) {
        const int n = (int)((unsigned)pix / (unsigned)hw);      // npix < 2^31 (checked on the host)
        const int rem = (int)pix - n * hw;
        xv[u] = ld16(x + pix * PX + cg * EPV);
        if (dx && accumulate) ov[u] = ld16(dx + pix * PDX + cg * EPV);
        if constexpr (BNR) yb[u] = ba.fetch(bn, cg, pix);
#pragma unroll
        for (int k = 0; k < KM; ++k) d[u][k] = (KT > 0 || k < K) ? dl[((int64_t)n * K + k) * hw + rem] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pix = pix0 + u * stride;
      if (pix < npix) {
        float g[EPV];
#pragma unroll
        for (int e = 0; e < EPV; ++e) g[e] = 0.f;
#pragma unroll
        for (int k = 0; k < KM; ++k) {
          if (KT > 0 || k < K) {
            if (cg == 0) ab[k] += d[u][k];
#pragma unroll
            for (int e = 0; e < EPV; ++e) { g[e] += d[u][k] * wk[k][e]; aw[k][e] += d[u][k] * xv[u].get(e); }
          }
        }
        if (dx) {
          Vec16<T> o;
#pragma unroll
          for (int e = 0; e < EPV; ++e) o.set(e, (accumulate ? ov[u].get(e) : 0.f) + g[e]);
          st16(dx + pix * PDX + cg * EPV, o);
          if constexpr (BNR) ba.add(bn, s_tab, cg, yb[u], o);
        }
      }
    }
  }
  // block reduction in a fixed order (bit-reproducible): lanes that own the same channel group are summed with
  // xor-shuffles, the four waves through LDS
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (k < K) {
#pragma unroll
      for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) aw[k][e] += __shfl_xor(aw[k][e], off);
        ab[k] += __shfl_xor(ab[k], off);
      }
      if (lane < G) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) s_dw[wv * (HEAD_MAXK * 33) + k * 32 + lane * EPV + e] = aw[k][e];
        if (lane == 0) s_dw[wv * (HEAD_MAXK * 33) + HEAD_MAXK * 32 + k] = ab[k];
      }
    }
  }
  __syncthreads();
  // per-block slab [K*32 weights | K biases]: plain stores, summed by the caller (no same-address atomics)
  float* slab = dw + (size_t)blockIdx.x * (K * 33);
  for (int i = threadIdx.x; i < K * 33; i += blockDim.x) {
    const int j = i < K * 32 ? i : HEAD_MAXK * 32 + (i - K * 32);
    slab[i] = (s_dw[j] + s_dw[HEAD_MAXK * 33 + j]) + (s_dw[2 * HEAD_MAXK * 33 + j] + s_dw[3 * HEAD_MAXK * 33 + j]);
  }
  if constexpr (BNR) ba.finish(bn, s_part, G);
}
static int head_fwd_grid(int64_t npix) { return grid_for(npix, 256); }   // thread per pixel, grid-stride beyond 4096 workgroups
template <typename T> static int launch_head_fwd(int N, int H, int W, int C, int K, const void* x, int PX, const float* w, const float* b, float* logits, hipStream_t st) {
  ProfScope ps(PC_HEAD, 2.0 * N * H * W * C * K, (double)N * H * W * (C * sizeof(T) + K * 4), st);
  const dim3 grid(head_fwd_grid((int64_t)N * H * W));
  if (C == 32) NUNET_LAUNCH((head_fwd_kernel<T, 32>), grid, dim3(256), 0, st, (const T*)x, PX, w, b, logits, N, H, W, C, K);
  else NUNET_LAUNCH((head_fwd_kernel<T, 0>), grid, dim3(256), 0, st, (const T*)x, PX, w, b, logits, N, H, W, C, K);
  return nunet_check_launch("head_fwd");
}
template <typename T> static int launch_head_fwd_bn(const nunet_bn_fwd_desc* d, int K, const float* w, const float* b, float* logits, hipStream_t st) {
  const BnFwdP p = bn_fwd_params(d);
  const HeadP h = {w, b, logits, K};
  const int64_t np = (int64_t)d->N * d->H * d->W;
  ProfScope ps(PC_BN_FWD, 2.0 * np * d->C * K, (double)np * (2.0 * d->C * sizeof(T) + K * 4), st);
  const dim3 grid(bn_fwd_grid(np, d->C / Tr<T>::EPV));
  if (K == 1) NUNET_LAUNCH((head_fwd_bn_kernel<T, 1>), grid, dim3(256), 0, st, p, h);
  else NUNET_LAUNCH((head_fwd_bn_kernel<T, 0>), grid, dim3(256), 0, st, p, h);
  return nunet_check_launch("head_fwd_bn");
}
template <typename T> static int launch_head_bwd(int N, int H, int W, int C, int K, const void* x, int PX, const float* w, const float* dl, void* dx, int PDX, int acc, float* dw_slabs, int nslabs, const nunet_bnr_desc* bnr, hipStream_t st) {
  ProfScope ps(PC_HEAD, 4.0 * N * H * W * C * K, (double)N * H * W * (C * sizeof(T) * ((acc ? 3 : 2) + (bnr ? 1 : 0)) + K * 4), st);
  const dim3 grid(nslabs), blk(256);
  BnrP b; memset(&b, 0, sizeof(b));
  if (bnr) { NUNET_REQUIRE(dx, "head_bwd: fused BN reduce needs dx"); int rc = bnr_fill(b, bnr, C, Tr<T>::DT); if (rc) return rc; }
#define NUNET_HB(KT, BN_) NUNET_LAUNCH((head_bwd_kernel<T, KT, BN_>), grid, blk, 0, st, (const T*)x, PX, w, dl, (T*)dx, PDX, acc, dw_slabs, N, H, W, C, K, b)
  if (bnr) { if (K == 1) NUNET_HB(1, true); else if (K == 2) NUNET_HB(2, true); else if (K == 4) NUNET_HB(4, true); else NUNET_HB(0, true); }
  else { if (K == 1) NUNET_HB(1, false); else if (K == 2) NUNET_HB(2, false); else if (K == 4) NUNET_HB(4, false); else NUNET_HB(0, false); }
#undef NUNET_HB
  return nunet_check_launch("head_bwd");
}
extern "C" int nunet_head_fwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, const void* x, int32_t PX, const float* w, const float* b, float* logits, nunet_stream_t s) {
  NUNET_REQUIRE(x && w && b && logits, "head_fwd: null pointer");
  NUNET_REQUIRE(C > 0 && C <= 64 && C % (16 / dtype_size(dtype)) == 0 && K >= 1 && K <= HEAD_MAXK, "head_fwd: C=%d K=%d unsupported (C<=64, K<=%d)", C, K, HEAD_MAXK);
  NUNET_REQUIRE(PX % (16 / dtype_size(dtype)) == 0, "head_fwd: pitch");
  return NUNET_DISPATCH(dtype, launch_head_fwd, N, H, W, C, K, x, PX, w, b, logits, (hipStream_t)s);
}
extern "C" int nunet_head_fwd_bn(const nunet_bn_fwd_desc* d, int32_t K, const float* w, const float* b, float* logits, nunet_stream_t s) {
  const int rc = bn_fwd_check(d);
  if (rc) return rc;
  NUNET_REQUIRE(w && b && logits, "head_fwd_bn: null pointer");
  NUNET_REQUIRE(!d->pooled && !d->up, "head_fwd_bn: no fused pool and no fused upsample in this form");
  NUNET_REQUIRE(d->C <= 64 && K >= 1 && K <= HEAD_MAXK, "head_fwd_bn: C=%d K=%d unsupported (C<=64, K<=%d)", d->C, K, HEAD_MAXK);
  NUNET_REQUIRE((int64_t)d->N * d->H * d->W < (1LL << 31), "head_fwd_bn: too many pixels");
  return NUNET_DISPATCH(d->dtype, launch_head_fwd_bn, d, K, w, b, logits, (hipStream_t)s);
}
extern "C" int nunet_head_launch_info(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t with_bn, nunet_loss_launch_info_t* out) {
  NUNET_REQUIRE(out && N > 0 && H > 0 && W > 0, "head_launch_info: bad args");
  NUNET_REQUIRE(dtype >= 0 && dtype <= 2, "bad dtype %d", dtype);
  const int epv = 16 / dtype_size(dtype);
  NUNET_REQUIRE(C >= epv && C <= 64 && C % epv == 0 && (!with_bn || pow2(C)), "head_launch_info: C=%d unsupported", C);
  const int64_t npix = (int64_t)N * H * W;
  // pixels one workgroup covers per pass: a thread per pixel, or C / epv lanes per pixel
  if (with_bn) fill_launch_info(out, bn_fwd_grid(npix, C / epv), 1, 1, npix, 256 / (C / epv));
  else fill_launch_info(out, head_fwd_grid(npix), 1, 1, npix);
  return NUNET_OK;
}
extern "C" int nunet_head_bwd_bnr(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, const void* x, int32_t PX, const float* w, const float* dlogits, void* dx, int32_t PDX, int32_t accumulate, float* dw_slabs, int32_t nslabs, const nunet_bnr_desc* bnr, nunet_stream_t s) {
  NUNET_REQUIRE(x && w && dlogits && dw_slabs && nslabs >= 1 && nslabs <= 4096, "head_bwd: bad args");
  NUNET_REQUIRE(C == 32 && K >= 1 && K <= HEAD_MAXK, "head_bwd: C=%d K=%d unsupported (C==32, K<=%d)", C, K, HEAD_MAXK);
  NUNET_REQUIRE((int64_t)N * H * W < (1LL << 31), "head_bwd: too many pixels");
  return NUNET_DISPATCH(dtype, launch_head_bwd, N, H, W, C, K, x, PX, w, dlogits, dx, PDX, accumulate, dw_slabs, nslabs, bnr, (hipStream_t)s);
}
extern "C" int nunet_head_bwd(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, const void* x, int32_t PX, const float* w, const float* dlogits, void* dx, int32_t PDX, int32_t accumulate, float* dw_slabs, int32_t nslabs, nunet_stream_t s) {
  return nunet_head_bwd_bnr(dtype, N, H, W, C, K, x, PX, w, dlogits, dx, PDX, accumulate, dw_slabs, nslabs, nullptr, s);
}

// ---------------------------------------------------------------------------
// SGD with momentum / weight decay / nesterov (torch.optim.SGD semantics)
// ---------------------------------------------------------------------------
// (the body is a macro so that sgd_ema_kernel below repeats it token for token: a step with a weight EMA must leave the bits of
//  the step without one, and how the compiler contracts this arithmetic depends on the code it is inlined into)
#define SGD_KERNEL_BODY                                                                                                        \
  const float lr = lr_dev[0];                                                                                                  \
  if (!scale_begin(sc, cl, gscale)) return;  /* loss scaling: a skipped step writes nothing; clipping: coef folded in */      \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {              \
    float pv = p[i];                                                                                                           \
    float gv = g[i] * gscale + wd * pv;                                                                                        \
    if (mom != 0.f) {                                                                                                          \
      const float b = first ? gv : mom * m[i] + gv;                                                                            \
      m[i] = b;                                                                                                                \
      gv = nesterov ? gv + mom * b : b;                                                                                        \
    }                                                                                                                          \
    p[i] = pv - lr * gv;                                                                                                       \
  }
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, int64_t n, const float* __restrict__ lr_dev, float mom, float wd, int nesterov, int first, float gscale,
                                                  const nunet_scaler* __restrict__ sc, const nunet_clip* __restrict__ cl) {
  SGD_KERNEL_BODY
}

// ---------------------------------------------------------------------------
// Adam (torch.optim.Adam semantics, amsgrad off; the per-element arithmetic is OptAdam in common.h)
// ---------------------------------------------------------------------------
// One thread: t = ++step (fp32, torch's capturable step), then the step's two scalars from the device lr. torch forms the
// bias corrections from Python floats (double) and hands fp32 kernels scalars rounded once: so does this.
__global__ void adam_prepare_kernel(const float* __restrict__ lr_dev, double b1, double b2, float* __restrict__ step, float* __restrict__ scal,
                                    const nunet_scaler* __restrict__ sc) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (sc && sc->found_inf) return;           // a step skipped by loss scaling does not count
  const float t = step[0] + 1.f;
  step[0] = t;
  const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
  scal[0] = (float)((double)lr_dev[0] / bc1);
  scal[1] = (float)(1.0 / sqrt(bc2));
}
extern "C" int nunet_adam_prepare(const float* lr_dev, double beta1, double beta2, float* step_dev, float* adam_scal, nunet_stream_t s) {
  NUNET_REQUIRE(lr_dev && step_dev && adam_scal, "adam_prepare: null pointer");
  NUNET_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_prepare: betas must lie in [0, 1)");
  NUNET_LAUNCH(adam_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, lr_dev, beta1, beta2, step_dev, adam_scal, (const nunet_scaler*)nullptr);
  return nunet_check_launch("adam_prepare");
}
extern "C" int nunet_adam_prepare_scaled(const float* lr_dev, double beta1, double beta2, float* step_dev, float* adam_scal,
                                         const nunet_scaler* scaler, nunet_stream_t s) {
  NUNET_REQUIRE(lr_dev && step_dev && adam_scal && scaler, "adam_prepare_scaled: null pointer");
  NUNET_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_prepare_scaled: betas must lie in [0, 1)");
  NUNET_LAUNCH(adam_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, lr_dev, beta1, beta2, step_dev, adam_scal, scaler);
  return nunet_check_launch("adam_prepare_scaled");
}

// Flat step: four elements per thread as 16-byte runs when every array is 16-byte aligned, scalar tail for n % 4
// (a macro for the reason SGD_KERNEL_BODY is one: adam_ema_kernel below repeats it token for token)
#define ADAM_KERNEL_BODY                                                                                                       \
  if (!o.begin(gscale)) return;              /* loss scaling: a skipped step writes nothing */                                \
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;                   \
  const int64_t n4 = vec ? n / 4 : 0;                                                                                          \
  for (int64_t i = tid; i < n4; i += nth) {                                                                                    \
    f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];                                                                           \
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];                                                                     \
    f32x4 mv = reinterpret_cast<const f32x4*>(o.st[0])[i], vv = reinterpret_cast<const f32x4*>(o.st[1])[i];                    \
    _Pragma("unroll")                                                                                                          \
    for (int j = 0; j < 4; ++j) {                                                                                              \
      float s[2] = {mv[j], vv[j]};                                                                                             \
      pv[j] = o.one(pv[j], gv[j] * gscale, s);                                                                                 \
      mv[j] = s[0];                                                                                                            \
      vv[j] = s[1];                                                                                                            \
    }                                                                                                                          \
    reinterpret_cast<f32x4*>(o.st[0])[i] = mv;                                                                                 \
    reinterpret_cast<f32x4*>(o.st[1])[i] = vv;                                                                                 \
    reinterpret_cast<f32x4*>(p)[i] = pv;                                                                                       \
  }                                                                                                                            \
  for (int64_t i = 4 * n4 + tid; i < n; i += nth) p[i] = opt_elem(o, p[i], g[i] * gscale, i);
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, OptAdam o, int64_t n, float gscale, int vec) {
  ADAM_KERNEL_BODY
}

// The flat step with a weight EMA (nunet_optim.ema): the body of the step without one - the same tokens, so p and the optimiser
// state are the bits of that step whatever the compiler makes of the arithmetic - and behind it, in the same launch, every
// thread moves the average towards the parameters it has just stored (its own elements, in the same order: four per thread
// as a 16-byte run where the step took them so, single elements else). OptEma (common.h) is unwrapped here: the plan's tile
// kernel is the one that carries the average as a stream of the functor.
__device__ __forceinline__ void ema_follow(float* __restrict__ ema, const float* p, int64_t n, int vec, int evec, float w, bool copy) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t i = tid; i < n4; i += nth) {
    const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
    if (evec) {
      f32x4 ev = reinterpret_cast<const f32x4*>(ema)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) ev[j] = copy ? pv[j] : ev[j] + w * (pv[j] - ev[j]);
      reinterpret_cast<f32x4*>(ema)[i] = ev;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float e = ema[4 * i + j]; ema[4 * i + j] = copy ? pv[j] : e + w * (pv[j] - e); }
    }
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += nth) { const float e = ema[i]; ema[i] = copy ? p[i] : e + w * (p[i] - e); }
}
__global__ __launch_bounds__(256) void sgd_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, int64_t n, const float* __restrict__ lr_dev, float mom, float wd, int nesterov, int first, float gscale,
                                                      const nunet_scaler* __restrict__ sc, const nunet_clip* __restrict__ cl, float* __restrict__ ema,
                                                      const nunet_ema* __restrict__ em) {
  SGD_KERNEL_BODY
  ema_follow(ema, p, n, 0, 0, em->w, em->live == NUNET_EMA_COPY);
}
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, OptAdam o, int64_t n, float gscale, int vec, float* __restrict__ ema,
                                                       int evec, const nunet_ema* __restrict__ em) {
  ADAM_KERNEL_BODY
  ema_follow(ema, p, n, vec, evec, em->w, em->live == NUNET_EMA_COPY);
}

// The flat step (layout 0) of a validated nunet_optim, either kind: one launch of sgd_kernel / adam_kernel, or of
// sgd_ema_kernel / adam_ema_kernel when the descriptor carries an ema
static void launch_flat(float* p, const float* g, const nunet_optim* opt, int64_t n, float grad_scale, int first, hipStream_t st) {
  const dim3 grid(grid_for(n, 256 * 4, 2048)), blk(256);
  opt_dispatch(opt, [&](auto o) {
    using O = decltype(o);
    ProfScope ps(PC_SGD, 0, (double)n * (12 + 8 * O::NS), st);
    if constexpr (std::is_same<O, OptSgd>::value) {
      NUNET_LAUNCH(sgd_kernel, grid, blk, 0, st, p, g, o.st[0], n, o.lr_dev, o.momc, o.wd, o.nesterov, first, grad_scale, o.sc, o.cl);
    } else if constexpr (std::is_same<O, OptAdam>::value) {
      const int vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)o.st[0] | (uintptr_t)o.st[1]) & 15) == 0;
      NUNET_LAUNCH(adam_kernel, grid, blk, 0, st, p, g, o, n, grad_scale, vec);
    } else if constexpr (std::is_same<O, OptEma<OptSgd>>::value) {
      NUNET_LAUNCH(sgd_ema_kernel, grid, blk, 0, st, p, g, o.in.st[0], n, o.in.lr_dev, o.in.momc, o.in.wd, o.in.nesterov, first, grad_scale, o.in.sc, o.in.cl,
                   o.st[1], o.em);
    } else {
      const int vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)o.in.st[0] | (uintptr_t)o.in.st[1]) & 15) == 0;     // (adam_kernel's)
      const int evec = vec && ((uintptr_t)o.st[2] & 15) == 0;
      NUNET_LAUNCH(adam_ema_kernel, grid, blk, 0, st, p, g, o.in, n, grad_scale, vec, o.st[2], evec, o.em);
    }
    return (int)NUNET_OK;
  });
}
extern "C" int nunet_sgd_step(float* p, const float* g, float* mom, int64_t n, const float* lr_dev, float momentum, float weight_decay, int32_t nesterov, int32_t first, float grad_scale, nunet_stream_t s) {
  NUNET_REQUIRE(p && g && n > 0, "sgd_step: bad args");
  nunet_optim o; memset(&o, 0, sizeof(o));
  o.kind = NUNET_OPT_SGD; o.momentum = momentum; o.weight_decay = weight_decay; o.nesterov = nesterov; o.lr = lr_dev; o.state0 = mom;
  if (const int rc = opt_check(&o, "sgd_step", false)) return rc;
  launch_flat(p, g, &o, n, grad_scale, first, (hipStream_t)s);
  return nunet_check_launch("sgd_step");
}
extern "C" int nunet_adam_step(float* p, const float* g, const nunet_optim* opt, int64_t n, float grad_scale, nunet_stream_t s) {
  NUNET_REQUIRE(p && g && opt && n > 0, "adam_step: bad args");
  NUNET_REQUIRE(opt->kind == NUNET_OPT_ADAM, "adam_step: optimiser kind %d is not NUNET_OPT_ADAM", (int)opt->kind);
  NUNET_REQUIRE(!opt->scaler, "adam_step: loss scaling goes through nunet_opt_step");
  NUNET_REQUIRE(!opt->clip, "adam_step: gradient clipping goes through nunet_opt_step");
  NUNET_REQUIRE(!opt->ema, "adam_step: a weight EMA goes through nunet_opt_step");
  if (const int rc = opt_check(opt, "adam_step", false)) return rc;
  launch_flat(p, g, opt, n, grad_scale, 0, (hipStream_t)s);
  return nunet_check_launch("adam_step");
}

// ---------------------------------------------------------------------------
// Dynamic loss scaling (torch.amp.GradScaler on the device; include/nunet.h nunet_scaler)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t nonfinite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }
// found_inf |= any element of g is inf / NaN: 16-byte loads, the exponent test on the raw bits, one workgroup-wide OR, and one
// device-scope atomic per workgroup that found one (none in a clean step)
__global__ __launch_bounds__(256) void scaler_check_kernel(const float* __restrict__ g, int64_t n, int vec, nunet_scaler* __restrict__ sc) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = vec ? n / 4 : 0;
  const u32x4* g4 = reinterpret_cast<const u32x4*>(g);
  uint32_t bad = 0;
  for (int64_t i = tid; i < n4; i += nth) {
    const u32x4 v = g4[i];
    bad |= nonfinite(v[0]) | nonfinite(v[1]) | nonfinite(v[2]) | nonfinite(v[3]);
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += nth) bad |= nonfinite(__float_as_uint(g[i]));
  if (__syncthreads_or((int)bad) && threadIdx.x == 0) atomicOr(&sc->found_inf, 1u);
}
extern "C" int nunet_scaler_check(const float* g, int64_t n, nunet_scaler* scaler, nunet_stream_t s) {
  NUNET_REQUIRE(g && scaler && n > 0, "scaler_check: bad args");
  const int vec = ((uintptr_t)g & 15) == 0;
  ProfScope ps(PC_SGD, 0, (double)n * 4, (hipStream_t)s);
  NUNET_LAUNCH(scaler_check_kernel, dim3(grid_for(vec ? (n + 3) / 4 : n, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)s, g, n, vec, scaler);
  return nunet_check_launch("scaler_check");
}

// One thread, torch's _amp_update_scale_ (the factors are doubles, the products rounded to fp32 once), then the next step's
// inv_scale as torch's unscale_ forms it (double reciprocal, rounded to fp32), the skip count, and found_inf cleared.
__global__ void scaler_update_kernel(nunet_scaler* __restrict__ sc, double growth, double backoff, int interval) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float scale = sc->scale;
  if (sc->found_inf) {
    scale = (float)((double)scale * backoff);
    sc->growth_tracker = 0;
    sc->skipped = sc->skipped + 1;
  } else {
    const int t = sc->growth_tracker + 1;
    if (t == interval) {
      const float grown = (float)((double)scale * growth);
      if (isfinite(grown)) scale = grown;
      sc->growth_tracker = 0;
    } else {
      sc->growth_tracker = t;
    }
  }
  sc->scale = scale;
  sc->inv_scale = (float)(1.0 / (double)scale);
  sc->found_inf = 0u;
}
extern "C" int nunet_scaler_update(nunet_scaler* scaler, double growth_factor, double backoff_factor, int32_t growth_interval, nunet_stream_t s) {
  NUNET_REQUIRE(scaler, "scaler_update: null scaler");
  NUNET_REQUIRE(growth_factor > 1.0 && std::isfinite(growth_factor), "scaler_update: growth_factor must be > 1 (got %g)", growth_factor);
  NUNET_REQUIRE(backoff_factor > 0.0 && backoff_factor < 1.0, "scaler_update: backoff_factor must lie in (0, 1) (got %g)", backoff_factor);
  NUNET_REQUIRE(growth_interval > 0, "scaler_update: growth_interval must be > 0 (got %d)", (int)growth_interval);
  NUNET_LAUNCH(scaler_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, scaler, growth_factor, backoff_factor, (int)growth_interval);
  return nunet_check_launch("scaler_update");
}

// g *= grad_scale * inv_scale in every step, skipped ones included: what torch's unscale_ leaves in p.grad; with a clip,
// * coef on top (1 on a skipped step): what clip_grad_norm_ leaves there. The factor is formed as the functors' begin() forms it.
__global__ __launch_bounds__(256) void unscale_kernel(float* __restrict__ g, int64_t n, float gscale, const nunet_scaler* __restrict__ sc,
                                                      const nunet_clip* __restrict__ cl, int vec) {
  float f = gscale;
  if (sc) f *= sc->inv_scale;
  if (cl) f *= cl->coef;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t i = tid; i < n4; i += nth) reinterpret_cast<f32x4*>(g)[i] = reinterpret_cast<const f32x4*>(g)[i] * f;
  for (int64_t i = 4 * n4 + tid; i < n; i += nth) g[i] = g[i] * f;
}
extern "C" int nunet_opt_step(float* p, float* g, const nunet_optim* opt, int64_t n, float grad_scale, nunet_stream_t s) {
  NUNET_REQUIRE(p && g && opt, "opt_step: bad args");
  if (const int rc = opt_check(opt, "opt_step", false)) return rc;
  NUNET_REQUIRE(n > 0, "opt_step: bad args");
  hipStream_t st = (hipStream_t)s;
  launch_flat(p, g, opt, n, grad_scale, 0, st);
  if (opt->scaler || opt->clip) {   // after the step, which read the scaled, unclipped gradients
    const int vec = ((uintptr_t)g & 15) == 0;
    NUNET_LAUNCH(unscale_kernel, dim3(grid_for(n, 256 * 4, 2048)), dim3(256), 0, st, g, n, grad_scale, opt->scaler, opt->clip, vec);
  }
  return nunet_check_launch("opt_step");
}

// ---------------------------------------------------------------------------
// Weight EMA (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn on the device; include/nunet.h nunet_ema)
// ---------------------------------------------------------------------------
__global__ void ema_init_kernel(nunet_ema* __restrict__ e, double decay, int warmup, int n_averaged) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  e->decay = decay; e->warmup = warmup; e->n_averaged = n_averaged;
  e->w = 0.f; e->live = NUNET_EMA_SKIP; e->reserved[0] = 0; e->reserved[1] = 0;
}
extern "C" int nunet_ema_init(nunet_ema* ema, double decay, int32_t warmup, int32_t n_averaged, nunet_stream_t s) {
  NUNET_REQUIRE(ema && ((uintptr_t)ema & 7) == 0, "ema_init: ema must be a non-null, 8-byte aligned device pointer");
  NUNET_REQUIRE(decay >= 0.0 && decay < 1.0, "ema_init: decay must lie in [0, 1) (got %g)", decay);
  NUNET_REQUIRE(n_averaged >= 0, "ema_init: n_averaged must be >= 0 (got %d)", (int)n_averaged);
  NUNET_LAUNCH(ema_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, ema, decay, warmup ? 1 : 0, (int)n_averaged);
  return nunet_check_launch("ema_init");
}

// One thread: this step's mode and w from n_averaged (the first update copies; then w = float(1 - d_t), the difference formed
// in double and rounded once, as torch's lerp_ receives its Python-float weight), then the bump. A step skipped by loss
// scaling gets mode SKIP and counts nowhere.
__global__ void ema_prepare_kernel(nunet_ema* __restrict__ e, const nunet_scaler* __restrict__ sc) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (sc && sc->found_inf) { e->live = NUNET_EMA_SKIP; return; }
  const int n = e->n_averaged;
  if (n == 0) {
    e->w = 1.f;
    e->live = NUNET_EMA_COPY;
  } else {
    double d = e->decay;
    if (e->warmup) {
      const double dw = (1.0 + (double)n) / (10.0 + (double)n);
      d = dw < d ? dw : d;
    }
    e->w = (float)(1.0 - d);
    e->live = NUNET_EMA_LERP;
  }
  e->n_averaged = n + 1;
}
extern "C" int nunet_ema_prepare(nunet_ema* ema, const nunet_scaler* scaler, nunet_stream_t s) {
  NUNET_REQUIRE(ema && ((uintptr_t)ema & 7) == 0, "ema_prepare: ema must be a non-null, 8-byte aligned device pointer");
  NUNET_REQUIRE(((uintptr_t)scaler & 3) == 0, "ema_prepare: scaler must be 4-byte aligned");
  NUNET_LAUNCH(ema_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, ema, scaler);
  return nunet_check_launch("ema_prepare");
}

// ema <- src (copy mode) or ema + w * (src - ema): 16-byte runs over the middle that starts `head` floats in (where both
// pointers reach a 16-byte boundary; vec 0: they never do together), scalars in front of and behind it
__global__ __launch_bounds__(256) void ema_lerp_kernel(float* __restrict__ ema, const float* __restrict__ src, int64_t n, int64_t head, int vec,
                                                       const nunet_ema* __restrict__ e) {
  const uint32_t mode = e->live;
  if (mode == NUNET_EMA_SKIP) return;        // a step skipped by loss scaling writes nothing
  const bool copy = mode == NUNET_EMA_COPY;
  const float w = e->w;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = vec ? (n - head) / 4 : 0;
  f32x4* e4 = reinterpret_cast<f32x4*>(ema + head);
  const f32x4* s4 = reinterpret_cast<const f32x4*>(src + head);
  for (int64_t i = tid; i < n4; i += nth) {
    const f32x4 sv = s4[i];
    f32x4 ev = e4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) ev[j] = copy ? sv[j] : ev[j] + w * (sv[j] - ev[j]);
    e4[i] = ev;
  }
  for (int64_t i = tid; i < head; i += nth) ema[i] = copy ? src[i] : ema[i] + w * (src[i] - ema[i]);
  for (int64_t i = head + 4 * n4 + tid; i < n; i += nth) ema[i] = copy ? src[i] : ema[i] + w * (src[i] - ema[i]);
}
extern "C" int nunet_ema_lerp(float* ema, const float* src, int64_t n, const nunet_ema* state, nunet_stream_t s) {
  NUNET_REQUIRE(ema && src && state && n > 0, "ema_lerp: bad args");
  NUNET_REQUIRE((((uintptr_t)ema | (uintptr_t)src) & 3) == 0 && ((uintptr_t)state & 7) == 0,
                "ema_lerp: ema and src must be 4-byte aligned, state 8-byte aligned");
  const int vec = ((uintptr_t)ema & 15) == ((uintptr_t)src & 15);
  int64_t head = vec ? (int64_t)(((16 - ((uintptr_t)ema & 15)) & 15) / 4) : 0;     // scalars in front of the first 16-byte boundary
  if (head > n) head = n;
  ProfScope ps(PC_SGD, 0, (double)n * 12, (hipStream_t)s);
  NUNET_LAUNCH(ema_lerp_kernel, dim3(grid_for(n, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)s, ema, src, n, head, vec, state);
  return nunet_check_launch("ema_lerp");
}

// ---------------------------------------------------------------------------
// Gradient-norm clipping (torch.nn.utils.clip_grad_norm_ on the device; include/nunet.h nunet_clip)
// ---------------------------------------------------------------------------
// Square norm of n fp32 values, one double partial per workgroup. The products (double)g * (double)g are exact (48 bits), the
// sums are in double in a fixed order: a thread's grid-stride elements in index order (16-byte loads over the aligned middle,
// then the `head` scalars in front of it and the < 4 behind it), then block256_sum_f64. Plain stores, no atomics.
#define SQNORM_PER_WG (256 * 32)      // values a workgroup takes before the grid stops growing with n
#define SQNORM_MAX_WGS 1024
static int sqnorm_grid(int64_t n) {
  const int64_t g = (n + SQNORM_PER_WG - 1) / SQNORM_PER_WG;
  return (int)(g < 1 ? 1 : g > SQNORM_MAX_WGS ? SQNORM_MAX_WGS : g);
}
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, int64_t n, int64_t head, double* __restrict__ ws) {
  __shared__ double s_w[4];
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = (n - head) / 4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + head);
  double acc = 0.0;
  for (int64_t i = tid; i < n4; i += nth) {
    const f32x4 v = g4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += (double)v[j] * (double)v[j];
  }
  for (int64_t i = tid; i < head; i += nth) acc += (double)g[i] * (double)g[i];
  for (int64_t i = head + 4 * n4 + tid; i < n; i += nth) acc += (double)g[i] * (double)g[i];
  const double tot = block256_sum_f64(acc, s_w);
  if (threadIdx.x == 0) ws[blockIdx.x] = tot;
}
extern "C" size_t nunet_grad_sqnorm_ws_bytes(int64_t n) { return n > 0 ? (size_t)sqnorm_grid(n) * sizeof(double) : 0; }
extern "C" int nunet_grad_sqnorm(const float* g, int64_t n, double* ws, size_t ws_bytes, nunet_stream_t s) {
  NUNET_REQUIRE(g && ws && n > 0, "grad_sqnorm: bad args");
  NUNET_REQUIRE(((uintptr_t)g & 3) == 0 && ((uintptr_t)ws & 7) == 0, "grad_sqnorm: g must be 4-byte aligned, ws 8-byte aligned");
  NUNET_REQUIRE(ws_bytes >= nunet_grad_sqnorm_ws_bytes(n), "grad_sqnorm: workspace of %zu bytes, nunet_grad_sqnorm_ws_bytes = %zu",
                ws_bytes, nunet_grad_sqnorm_ws_bytes(n));
  int64_t head = (int64_t)(((16 - ((uintptr_t)g & 15)) & 15) / 4);     // scalars in front of the first 16-byte boundary
  if (head > n) head = n;
  ProfScope ps(PC_SGD, 0, (double)n * 4, (hipStream_t)s);
  NUNET_LAUNCH(grad_sqnorm_kernel, dim3(sqnorm_grid(n)), dim3(256), 0, (hipStream_t)s, g, n, head, ws);
  return nunet_check_launch("grad_sqnorm");
}

// One workgroup: the partials summed by a fixed tree (thread t takes ws[t], ws[t + 256], ... in order, then
// block256_sum_f64), then thread 0 forms total_norm, coef as torch forms it (fp32: max_norm / (total_norm + 1e-6), clamped
// to 1; a NaN passes through like torch.clamp's) and the statistics. A step skipped by loss scaling gets coef = 1 and
// counts nowhere.
__global__ __launch_bounds__(256) void clip_finalize_kernel(const double* __restrict__ ws, int nparts, float gscale,
                                                            const nunet_scaler* __restrict__ sc, nunet_clip* __restrict__ cl) {
  __shared__ double s_w[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += ws[i];
  const double tot = block256_sum_f64(acc, s_w);
  if (threadIdx.x != 0) return;
  if (sc && sc->found_inf) { cl->coef = 1.f; return; }
  const double f = (double)gscale * (sc ? (double)sc->inv_scale : 1.0);
  const float norm = (float)(sqrt(tot) * f);
  float coef = cl->max_norm / (norm + 1e-6f);
  coef = coef > 1.f ? 1.f : coef;
  cl->coef = coef;
  cl->norm = norm;
  if (!(cl->norm_peak >= norm)) cl->norm_peak = norm;
  cl->norm_sum = cl->norm_sum + (double)norm;
  cl->steps = cl->steps + 1;
  if (coef < 1.f) cl->clipped = cl->clipped + 1;
}
extern "C" int nunet_clip_finalize(const double* ws, int32_t nparts, float grad_scale, const nunet_scaler* scaler, nunet_clip* clip,
                                   nunet_stream_t s) {
  NUNET_REQUIRE(ws && clip && nparts > 0, "clip_finalize: bad args");
  NUNET_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)clip & 7) == 0, "clip_finalize: ws and clip must be 8-byte aligned");
  NUNET_REQUIRE(grad_scale > 0.f && std::isfinite(grad_scale), "clip_finalize: grad_scale must be positive and finite (got %g)", (double)grad_scale);
  NUNET_LAUNCH(clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, ws, (int)nparts, grad_scale, scaler, clip);
  return nunet_check_launch("clip_finalize");
}
