// common.h — shared device/host helpers for libnunet (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <type_traits>

#include "../../include/nunet.h"
#include "../../include/nunet_diag.h"

typedef __bf16 bf16_t;
typedef _Float16 f16_t;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

#define WAVE 64
#define CONV_GROUP_MAX 4      // problem slots of the 3x3 convolution's kernel argument (conv3x3.hip ConvGroup: the host fills one)

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
void nunet_set_error(const char* fmt, ...);
int nunet_check_launch(const char* what);

#define NUNET_REQUIRE(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      nunet_set_error(__VA_ARGS__);         \
      return NUNET_EINVAL;                  \
    }                                       \
  } while (0)

// ---------------------------------------------------------------------------
// optional per-launch timing (bench.py's roofline leg): hipEvents on the launch
// stream around every kernel, aggregated per kernel class. Off by default.
// ---------------------------------------------------------------------------
enum {
  PC_CONV_M256N32 = 0, PC_CONV_M128N64, PC_CONV_M128N32, PC_WGRAD_1x4, PC_WGRAD_2x2, PC_BN_FWD, PC_BN_BWD_REDUCE,
  PC_BN_BWD_APPLY, PC_UP_FWD, PC_UP_BWD, PC_POOL, PC_HEAD, PC_PACK, PC_UNPACK, PC_LOSS, PC_SGD,
  PC_LAYOUT, PC_COUNT
};
extern thread_local bool g_prof_on;
extern thread_local int g_prof_alg_cin;  // >0: algorithmic Cin of the next conv/wgrad (padded first layer)
void nunet_prof_push(int cls, double flops, double bytes);
void nunet_prof_pop();
void nunet_prof_kernel_events(hipEvent_t* e0, hipEvent_t* e1);   // a fresh start/stop pair owned by the innermost open scope (null: none)
struct ProfScope {
  bool on;
  ProfScope(int cls, double flops, double bytes, hipStream_t) : on(g_prof_on) { if (on) nunet_prof_push(cls, flops, bytes); }
  ~ProfScope() { if (on) nunet_prof_pop(); }
};
// Segmented step recording (graph.hip, nunet_seg_*): while a DRY pass runs, launches are skipped - the pass only finds out which
// events are waited on across lanes.
extern thread_local bool g_dry_run;
// Every kernel launch goes through this. Timing off: plain hipLaunchKernelGGL. Timing on (bench.py's roofline leg):
// hipExtLaunchKernelGGL with a start/stop event pair, which carries the DISPATCH's own begin/end timestamps (what
// rocprofv3 --kernel-trace reports) - events recorded around a launch as separate stream markers add ~5 us to a 15 us kernel.
#define NUNET_LAUNCH(kernel, grid, block, shmem, stream, ...)                                                    \
  do {                                                                                                          \
    if (g_dry_run) break;                                                                                       \
    hipEvent_t pe0_ = nullptr, pe1_ = nullptr;                                                                  \
    if (g_prof_on) nunet_prof_kernel_events(&pe0_, &pe1_);                                                      \
    if (pe0_) hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, pe0_, pe1_, 0, __VA_ARGS__);            \
    else hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                   \
  } while (0)

// zero-fill by a kernel on the caller's stream. hipMemsetAsync is NOT used anywhere:
// captured into a hipGraph its memset node ran unordered w.r.t. the neighbouring kernel
// nodes on replay (accumulators were cleared late / early), see DESIGN.md.
int nunet_zero_async(void* p, size_t bytes, hipStream_t st);

// ---------------------------------------------------------------------------
// Segmented recording of a multi-lane step (graph.hip). ROCm 7.2 replays a hipGraph with parallel branches by enqueueing
// node after node with a synchronisation of its own (2.6-5 us per node, tools/graph_gap_probe.py), while a single-stream
// graph replays as one batch of pre-built packets (0.7 us per node). So the plan's lanes are NOT captured as branches of one
// graph: every lane keeps a real stream, its ops are captured into ONE single-stream graph, and the cross-lane
// dependencies become device-side flags inside those graphs. The lane scheduler (sched.hip, Sched) routes its
// stream waits, event records and "about to launch on this stream" through these hooks; they return false when no
// recording is active (the caller then does the real HIP call).
// ---------------------------------------------------------------------------
bool seg_active();
bool seg_wait(hipStream_t st, hipEvent_t ev);      // `st` must wait for `ev` (recorded on another stream)
bool seg_record(hipEvent_t ev, hipStream_t st);    // `ev` marks the current tail of `st`
void seg_touch(hipStream_t st);                    // kernels are about to be launched on `st`

static inline int dtype_size(int dt) { return dt == NUNET_F32 ? 4 : 2; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
// workgroups of a grid-stride launch: one per `block` items, at least 1, at most `cap`
static inline int grid_for(int64_t items, int block, int cap = 256 * 16) {
  int64_t g = ceil_div64(items, block);
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------------------
// storage-type traits: EPV = elements per 16-byte vector
// ---------------------------------------------------------------------------
template <typename T> struct Tr;
template <> struct Tr<float> {
  static constexpr int EPV = 4;
  static constexpr int DT = NUNET_F32;
};
template <> struct Tr<bf16_t> {
  static constexpr int EPV = 8;
  static constexpr int DT = NUNET_BF16;
};
template <> struct Tr<f16_t> {
  static constexpr int EPV = 8;
  static constexpr int DT = NUNET_F16;
};

template <typename T> __device__ __forceinline__ float to_f32(T v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v) { return (T)v; }

// 16-byte vector of T with element access as float
// Replicas of a per-channel sum buffer actually used for C channels (include/nunet.h, NUNET_BN_SUM_REPLICAS):
// contention is a matter of the shallow, wide levels (many workgroups, few channels); deep levels have
// few workgroups and reading 8 x 2 x C values per consumer block would cost more than it saves.
__host__ __device__ __forceinline__ int bn_sum_replicas(int C) {
  const int r = 256 / C;
  return r < 1 ? 1 : (r > NUNET_BN_SUM_REPLICAS ? NUNET_BN_SUM_REPLICAS : r);
}

// Linear index -> (channel group, x, y, n) of an [N][H][W][G] iteration space. The element-wise kernels used three 64-bit
// divisions per element (>100 instructions each on this ISA): with the extents fixed per launch they become multiplies
// by ceil(2^32 / d), exact while index * d < 2^32 (checked on the host; the 64-bit path stays for larger tensors).
struct Dec4 { int G, W, H; unsigned iG, iW, iH; int fast; };
static inline unsigned dec_inv(int d) { return d > 1 ? (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d) : 0u; }
static inline Dec4 make_dec4(long long total, int G, int W, int H) {
  Dec4 d; d.G = G; d.W = W; d.H = H; d.iG = dec_inv(G); d.iW = dec_inv(W); d.iH = dec_inv(H);
  const long long mx = G > W ? (G > H ? G : H) : (W > H ? W : H);
  d.fast = total > 0 && total * mx < (1ll << 32) ? 1 : 0;
  return d;
}
__device__ __forceinline__ int dec_div(int n, unsigned inv) { return inv ? (int)__umulhi((unsigned)n, inv) : n; }
__device__ __forceinline__ void dec4(const Dec4& d, long long i, int& cg, long long& o, int& x, int& y, int& n) {
  if (d.fast) {
    const int ii = (int)i;
    const int oo = dec_div(ii, d.iG); cg = ii - oo * d.G;
    const int t = dec_div(oo, d.iW); x = oo - t * d.W;
    n = dec_div(t, d.iH); y = t - n * d.H;
    o = oo;
  } else {
    cg = (int)(i % d.G); o = i / d.G;
    x = (int)(o % d.W);
    const long long t = o / d.W;
    y = (int)(t % d.H); n = (int)(t / d.H);
  }
}

// XCD-aware placement (for speed only, any placement is correct): workgroups are dealt round-robin over the 8 XCDs, each with its
// own 4 MB L2, so blocks b and b + 8 share an L2 and b, b + 1 never do. Work items that read the same data are CONSECUTIVE in item
// order (the Cout tiles of one pixel tile of a conv; the Cout x Cin tiles of one pixel slice of a weight gradient; neighbouring
// pixel tiles, whose halos overlap; neighbouring rows of an upsample, which interpolate from the same source rows): taking
// item = block would send them to eight different L2s, each of which fetches the tile from memory again. The map below hands
// every XCD one contiguous range of the items instead: block b (XCD b % 8, the (b / 8)-th block that XCD receives) takes item
// base(b % 8) + b / 8. A bijection of [0, G) for every G >= 1 (tests/test_xcd_remap_cpu.py through nunet_xcd_remap_host).
#ifndef NUNET_XCD_REMAP
#define NUNET_XCD_REMAP 1
#endif
__host__ __device__ __forceinline__ int xcd_remap(int b, int G) {
  if (!NUNET_XCD_REMAP) return b;
  const int x = b & 7, l = b >> 3, q = G >> 3, rem = G & 7;
  return (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + l;
}

// ---------------------------------------------------------------------------
// Order-independent per-channel sums (BatchNorm statistics, BatchNorm-backward sums).
// Hundreds of workgroups add one partial sum each to the same channel. fp32 atomics would make the
// result depend on arrival order (run-to-run noise of ~1e-7 relative that the ill-conditioned small
// cases amplify past the 1e-4 parity bound), so an accumulator is 128-bit FIXED POINT in two int64
// words, value = hi * 2^-20 + lo * 2^-60: integer atomics commute, the total is bit-identical from
// run to run and exact to 2^-60 per partial. |partial| is clamped to 2^30 (non-finite -> 2^30).
// ---------------------------------------------------------------------------
#define NUNET_FX_WORDS 2
__device__ __forceinline__ void fx_add(long long* acc, float v) {
  double s = (v == v) ? (double)v : 1073741824.0;
  s = fmin(fmax(s, -1073741824.0), 1073741824.0) * 1048576.0;   // exact scaling
  const double f = floor(s);
  const long long hi = (long long)f;
  const long long lo = (long long)((s - f) * 1099511627776.0);  // [0, 2^40)
  atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)hi);
  atomicAdd(reinterpret_cast<unsigned long long*>(acc) + 1, (unsigned long long)lo);
}
__device__ __forceinline__ double fx_value(long long hi, long long lo) {
  return (double)hi * (1.0 / 1048576.0) + (double)lo * (1.0 / 1152921504606846976.0);
}
// totals of channel c (both values) over the replicas of a [rep][2][C] accumulator array (integer sums: exact, any
// order). All 2 * NUNET_BN_SUM_REPLICAS 16-byte loads are issued before the first use: ONE memory round trip - this
// runs in the prologue of every consumer workgroup, where a loop of dependent loads would cost ~1 us per replica.
typedef __attribute__((ext_vector_type(2))) long long fx2_t;
__device__ __forceinline__ void fx_totals(const long long* acc, int C, int nrep, int c, double& t0, double& t1) {
  fx2_t q[NUNET_BN_SUM_REPLICAS][2];
#pragma unroll
  for (int r = 0; r < NUNET_BN_SUM_REPLICAS; ++r) {
    const int rr = r < nrep ? r : 0;            // (re-reads replica 0 instead of branching; masked below)
#pragma unroll
    for (int v = 0; v < 2; ++v) q[r][v] = *reinterpret_cast<const fx2_t*>(acc + ((size_t)(rr * 2 + v) * C + c) * NUNET_FX_WORDS);
  }
  long long h0 = 0, l0 = 0, h1 = 0, l1 = 0;
#pragma unroll
  for (int r = 0; r < NUNET_BN_SUM_REPLICAS; ++r) {
    const bool on = r < nrep;
    h0 += on ? q[r][0][0] : 0; l0 += on ? q[r][0][1] : 0;
    h1 += on ? q[r][1][0] : 0; l1 += on ? q[r][1][1] : 0;
  }
  t0 = fx_value(h0, l0); t1 = fx_value(h1, l1);
}

// BatchNorm2d forward coefficients of channel c (nn.BatchNorm2d at reference finished/archs1.py:19,21).
// The 3x3 convs store their output WITHOUT the conv bias b (it is absorbed here): the first layers'
// outputs are bias-dominated (inputs are ~1e-2, reference dataset.py:71), so a 16-bit store of acc+b
// would lose the signal. With y = acc + b:  train: bn(y) = gamma*(acc - mean(acc))*invstd + beta (the
// bias cancels and only shifts running_mean);  eval: bn(y) = gamma*(acc - (rm - b))*invstd + beta.
// `mean` is the value to subtract from the STORED tensor; `mean_full` = E[y]. The batch variance is
// combined in double from the exact fixed-point totals (E[x^2] - E[x]^2 in fp32 cancels when |mean| >> std).
struct BnStatArgs {
  const long long* fx;        // training: [rep][2][C] fixed-point sums of the stored tensor
  const float* conv_bias;     // or NULL
  const float* rm; const float* rv;
  int C, training; float M, eps;
};
__device__ __forceinline__ void bn_stat_coeffs(const BnStatArgs& a, int c, float& mean, float& invstd, float& var, float& mean_full) {
  const float b = a.conv_bias ? a.conv_bias[c] : 0.f;
  if (a.training) {
    const int nrep = bn_sum_replicas(a.C);
    double t1, t2;
    fx_totals(a.fx, a.C, nrep, c, t1, t2);
    const double m = t1 / (double)a.M;
    const double v = t2 / (double)a.M - m * m;
    mean = (float)m;
    var = v > 0.0 ? (float)v : 0.f;
    mean_full = mean + b;
  } else {
    mean_full = a.rm[c];
    mean = mean_full - b;
    var = a.rv[c];
  }
  invstd = 1.0f / sqrtf(var + a.eps);
}

// running_mean / running_var update of nn.BatchNorm2d in training mode (momentum form, unbiased variance): ONE operation order for
// every kernel that performs it (contraction off: whether `a * b + c * d` fuses is otherwise decided per call site, and the
// BatchNorm taken in a conv's loader must leave the same bits as the stand-alone kernel)
__device__ __forceinline__ void bn_running_update(float* rm, float* rv, int c, float momentum, float mean_full, float var, float M) {
#pragma clang fp contract(off)
  const float unb = M > 1.f ? var * (M / (M - 1.f)) : var;
  const float keep = 1.f - momentum;
  const float a = keep * rm[c], b = momentum * mean_full;
  rm[c] = a + b;
  const float cc = keep * rv[c], d = momentum * unb;
  rv[c] = cc + d;
}

// byte = number of thresholds <= x (nunet_sigmoid_u8, loss.hip): branch-free 8-step binary search over 255 thresholds in LDS
__device__ __forceinline__ uint32_t sigmoid_byte(const float* s_thr, float x) {
  int lo = 0;                                   // invariant: thr[lo-1] <= x (or lo == 0), answer in [lo, lo + span]
#pragma unroll
  for (int span = 128; span > 0; span >>= 1) {
    const int mid = lo + span;                  // candidate count
    if (mid <= 255 && s_thr[mid - 1] <= x) lo = mid;
  }
  return (uint32_t)lo;
}

template <typename T> struct Vec16 {
  // zero-initialised: set() of a 16-bit element read-modify-writes its 32-bit word, and doing that on an
  // indeterminate word is undefined (it miscompiled for fp16 on the odd elements of words 0 and 1)
  u32x4 raw = {0u, 0u, 0u, 0u};
  __device__ __forceinline__ float get(int i) const {
    if constexpr (std::is_same<T, float>::value) {
      const uint32_t w = raw[i];  // copy first: bit_cast of a vector-element lvalue reads element 0
      return __builtin_bit_cast(float, w);
    } else {
      uint32_t w = raw[i >> 1];
      uint16_t hv = (i & 1) ? (uint16_t)(w >> 16) : (uint16_t)(w & 0xffff);
      return (float)__builtin_bit_cast(T, hv);
    }
  }
  __device__ __forceinline__ void set(int i, float v) {
    if constexpr (std::is_same<T, float>::value) {
      const uint32_t w = __builtin_bit_cast(uint32_t, v);
      raw[i] = w;
    } else {
      uint16_t hv = __builtin_bit_cast(uint16_t, (T)v);
      uint32_t w = raw[i >> 1];
      w = (i & 1) ? ((w & 0x0000ffffu) | ((uint32_t)hv << 16)) : ((w & 0xffff0000u) | hv);
      raw[i >> 1] = w;
    }
  }
};

// Whole-vector conversion between a 16-byte storage vector and fp32 lanes. With ext_vector types the compiler emits
// one shift / v_cvt per element on the way in, v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 per PAIR on the way out and packed
// fp32 math (v_pk_fma_f32) in between - the element-wise get()/set() accessors cost ~3x the VALU instructions, which
// matters where a transform sits between a global load and an LDS write on a conv's critical path.
typedef __attribute__((ext_vector_type(8))) float f32x8;
template <typename T> struct FV { typedef f32x8 type; };
template <> struct FV<float> { typedef f32x4 type; };
template <typename T> __device__ __forceinline__ typename FV<T>::type vec_to_f(const Vec16<T>& v) {
  if constexpr (std::is_same<T, float>::value) return __builtin_bit_cast(f32x4, v.raw);
  else if constexpr (std::is_same<T, bf16_t>::value) return __builtin_convertvector(__builtin_bit_cast(bf16x8, v.raw), f32x8);
  else return __builtin_convertvector(__builtin_bit_cast(f16x8, v.raw), f32x8);
}
template <typename T> __device__ __forceinline__ Vec16<T> vec_from_f(const typename FV<T>::type& f) {
  Vec16<T> v;
  if constexpr (std::is_same<T, float>::value) v.raw = __builtin_bit_cast(u32x4, f);
  else if constexpr (std::is_same<T, bf16_t>::value) v.raw = __builtin_bit_cast(u32x4, __builtin_convertvector(f, bf16x8));
  else v.raw = __builtin_bit_cast(u32x4, __builtin_convertvector(f, f16x8));
  return v;
}
// fp32 lanes <- EPV consecutive floats of a table (LDS or global), 16-byte aligned
template <typename T> __device__ __forceinline__ typename FV<T>::type ldf(const float* p) {
  if constexpr (std::is_same<T, float>::value) return *reinterpret_cast<const f32x4*>(p);
  else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    return f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  }
}
// BatchNorm + ReLU forward / backward-apply on whole vectors; explicit fma so that every kernel that evaluates them
// (stand-alone BN kernels, the convs' input transforms) rounds identically.
//   forward : relu(fma(y, sc, sh))
//   backward: dz = (fma(y, sc, sh) > 0) ? da : 0;  dy = sc * (dz - k1 - xhat * k2) evaluated as fma(sc, dz, -fma(B, y, A))
//             with B = sc * k2 * invstd, A = sc * k1 - B * mean  (bn_bwd_AB)
template <typename V> __device__ __forceinline__ V bn_relu_apply(const V& y, const V& sc, const V& sh) {
  const V z = __builtin_elementwise_fma(y, sc, sh);
  return __builtin_elementwise_max(z, V(0.f));
}
template <typename V> __device__ __forceinline__ V bn_relu_bwd_apply(const V& da, const V& y, const V& sc, const V& sh, const V& A, const V& B) {
  const V act = __builtin_elementwise_fma(y, sc, sh);
  const V dz = act > V(0.f) ? da : V(0.f);
  return __builtin_elementwise_fma(sc, dz, -__builtin_elementwise_fma(B, y, A));
}
__device__ __forceinline__ void bn_bwd_AB(float mean, float istd, float sc, float k1, float k2, float& A, float& B) {
  B = sc * k2 * istd;
  A = __builtin_fmaf(-B, mean, sc * k1);
}

template <typename T> __device__ __forceinline__ Vec16<T> ld16(const T* p) {
  Vec16<T> v;
  v.raw = *reinterpret_cast<const u32x4*>(p);
  return v;
}
template <typename T> __device__ __forceinline__ void st16(T* p, const Vec16<T>& v) {
  *reinterpret_cast<u32x4*>(p) = v.raw;
}
template <typename T> __device__ __forceinline__ Vec16<T> zero16() {
  Vec16<T> v;
  v.raw = u32x4{0u, 0u, 0u, 0u};
  return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Sum of one double per thread over a 256-thread workgroup by a fixed tree: xor butterfly inside each wave (every lane ends
// with the same total), the four wave totals through LDS, added in wave order. Every thread returns the total.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double block256_sum_f64(double v, double* s_w4) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) s_w4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_w4[0] + s_w4[1]) + s_w4[2]) + s_w4[3];
}
// The slab epilogue of the per-block partial sums (loss.hip), in its two halves around the workgroup's one barrier.
// slab_park: NV values of one type per thread, each reduced over its wave by the butterfly of its type (counts: uint32), the
// four wave totals parked in LDS (s_w: [4][NV], the caller's). slab_store, after __syncthreads(): the thread with 0 <= q < NV
// stores ((w0 + w1) + w2) + w3 to dst[q] with a plain store; D != T converts the total on the way out (counts kept as
// float). A kernel that mixes types parks both arrays in one call, one with several slabs parks them all; it syncs once and gives each array its own threads
// through q; block256_slab_store is the whole epilogue of a kernel with one array.
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int NV, typename T>
__device__ __forceinline__ void wave_totals(const T (&v)[NV], T (&w)[NV]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    if constexpr (std::is_same<T, float>::value) w[q] = wave_sum(v[q]);
    else if constexpr (std::is_same<T, double>::value) w[q] = wave_sum_f64(v[q]);
    else w[q] = wave_sum_u32(v[q]);
  }
}
// (all butterflies first, then one branch for the stores: the shuffle chains of all values overlap)
template <int NV, typename T>
__device__ __forceinline__ void slab_park(const T (&v)[NV], T (*s_w)[NV]) {
  T w[NV];
  wave_totals(v, w);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) s_w[threadIdx.x >> 6][q] = w[q];
  }
}
template <int NA, typename TA, int NB, typename TB>     // two arrays of different types
__device__ __forceinline__ void slab_park(const TA (&a)[NA], TA (*s_a)[NA], const TB (&b)[NB], TB (*s_b)[NB]) {
  TA wa[NA]; TB wb[NB];
  wave_totals(a, wa); wave_totals(b, wb);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < NA; ++q) s_a[threadIdx.x >> 6][q] = wa[q];
#pragma unroll
    for (int q = 0; q < NB; ++q) s_b[threadIdx.x >> 6][q] = wb[q];
  }
}
template <int NV, typename T, typename D>
__device__ __forceinline__ void slab_store(T (*s_w)[NV], D* __restrict__ dst, int q) {
  if ((unsigned)q < (unsigned)NV) dst[q] = (D)(((s_w[0][q] + s_w[1][q]) + s_w[2][q]) + s_w[3][q]);
}
template <int NV, typename T, typename D>
__device__ __forceinline__ void block256_slab_store(const T (&v)[NV], T (*s_w)[NV], D* __restrict__ dst) {
  slab_park(v, s_w);
  __syncthreads();
  slab_store(s_w, dst, (int)threadIdx.x);
}

// Foreground counts of the metrics (metrics.py:10-14,31-44): predicted iff x >= thr (NaN: not), labelled iff t > 0.5.
__device__ __forceinline__ void fg_count2(float xv, float tv, float thr, unsigned& inter, unsigned& uni) {
  const bool a = xv >= thr, b = tv > 0.5f;
  inter += (a && b) ? 1u : 0u; uni += (a || b) ? 1u : 0u;
}
__device__ __forceinline__ void fg_count4(float xv, float tv, float thr, unsigned& tp, unsigned& fp, unsigned& fn, unsigned& tn) {
  const bool a = xv >= thr, b = tv > 0.5f;
  tp += (a && b) ? 1u : 0u; fp += (a && !b) ? 1u : 0u; fn += (!a && b) ? 1u : 0u; tn += (!a && !b) ? 1u : 0u;
}

// What one thread of every loss step's last launch writes (trains.py:120-128): the loss of each head (loss_of(k)), their mean -
// added left to right from 0, divided once - and the epoch meters from the last head's IoU intersection and union.
template <class F>
__device__ __forceinline__ void write_losses_meters(float* loss_out, int heads, double* meters, double inter, double uni, F&& loss_of) {
  float mean = 0.f;
  for (int k = 0; k < heads; ++k) {
    const float lk = loss_of(k);
    loss_out[k] = lk;
    mean += lk;
  }
  mean /= (float)heads;
  loss_out[heads] = mean;
  if (meters) {
    meters[0] += (double)mean;
    meters[1] += (inter + 1e-5) / (uni + 1e-5);
    meters[2] = inter; meters[3] = uni;
  }
}

// launch geometry of a grid-stride loop `for (i = block * per_block + lane item; i < items; i += grid.x * per_block)`
// (include/nunet_diag.h): thread 0 of block 0 takes the most trips, the last thread of the last block the fewest
static inline void fill_launch_info(nunet_loss_launch_info_t* out, int gx, int gy, int gz, int64_t items, int per_block = 256) {
  const int64_t per_pass = (int64_t)gx * per_block;
  out->grid_x = gx; out->grid_y = gy; out->grid_z = gz; out->block = 256;
  out->items = items;
  out->trips_max = ceil_div64(items, per_pass);
  out->trips_min = items / per_pass;
}

// dispatch a templated launcher on dtype
#define NUNET_DISPATCH(dt, FN, ...)                                   \
  ((dt) == NUNET_F32    ? FN<float>(__VA_ARGS__)                      \
   : (dt) == NUNET_BF16 ? FN<bf16_t>(__VA_ARGS__)                     \
   : (dt) == NUNET_F16  ? FN<f16_t>(__VA_ARGS__)                      \
                        : (nunet_set_error("bad dtype %d", (int)(dt)), NUNET_EINVAL))

// ---------------------------------------------------------------------------
// Optimiser functors of the fused update kernels (weights.hip) and the flat Adam step (elementwise.hip): the per-element step
// with its state pointers (NS fp32 buffers in flat parameter order). begin(gscale) reads the device scalars once per thread;
// one(p, g, s) takes the (scaled, undecayed) gradient and the element's state, updates the state in place and returns the
// new parameter. Built on the host from a nunet_optim by opt_sgd() / opt_adam() below, which every entry reaches through
// opt_check() + opt_dispatch().
// Loss scaling (sc != NULL, nunet_scaler): begin() returns false when the step is skipped (found_inf) - every thread of the
// launch reads the same word, written by an earlier launch, so the decision is uniform and the caller's workgroup stores no
// parameter, state or packed weight - and otherwise folds inv_scale into the caller's gradient scale. sc == NULL leaves the
// gradient scale untouched: the arithmetic of an unscaled step is unchanged.
// Gradient clipping (cl != NULL, nunet_clip): this step's coef, written by clip_finalize_kernel in an earlier launch, is folded
// into the gradient scale behind inv_scale (1.0f exactly when nothing is clipped). cl == NULL: nothing changes.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool scaler_begin(const nunet_scaler* sc, float& gscale) {
  if (!sc) return true;
  if (sc->found_inf) return false;
  gscale *= sc->inv_scale;
  return true;
}
__device__ __forceinline__ bool scale_begin(const nunet_scaler* sc, const nunet_clip* cl, float& gscale) {
  if (!scaler_begin(sc, gscale)) return false;
  if (cl) gscale *= cl->coef;
  return true;
}
struct OptSgd {   // torch.optim.SGD (reference trains.py:229-231): the arithmetic the SGD kernels always had, bit for bit
  static constexpr int NS = 1;
  float* st[1];
  const float* lr_dev;
  float momc, wd;
  int nesterov;
  const nunet_scaler* sc;
  const nunet_clip* cl;
  float lr;
  __device__ __forceinline__ bool begin(float& gscale) { lr = lr_dev[0]; return scale_begin(sc, cl, gscale); }
  __device__ __forceinline__ float one(float p, float g, float* s) const {
    float gv = g + wd * p;
    if (momc != 0.f) {
      const float b = momc * s[0] + gv;
      s[0] = b;
      gv = nesterov ? gv + momc * b : b;
    }
    return p - lr * gv;
  }
};
struct OptAdam {  // torch.optim.Adam, amsgrad=False, maximize=False, L2 decay in the gradient (reference trains.py:225-227)
  static constexpr int NS = 2;
  float* st[2];             // exp_avg, exp_avg_sq
  const float* scal_dev;    // {lr / (1 - b1^t), 1 / sqrt(1 - b2^t)}, written by adam_prepare_kernel for this step
  float omb1, b2, omb2, eps, wd;   // 1 - beta1, beta2, 1 - beta2 rounded from double once (torch's Python-float scalars)
  const nunet_scaler* sc;
  const nunet_clip* cl;
  float step_size, inv_sqrt_bc2;
  __device__ __forceinline__ bool begin(float& gscale) {
    step_size = scal_dev[0]; inv_sqrt_bc2 = scal_dev[1];
    return scale_begin(sc, cl, gscale);
  }
  __device__ __forceinline__ float one(float p, float g, float* s) const {
    const float gd = g + wd * p;                            // grad.add(param, alpha=wd)
    const float m = s[0] + omb1 * (gd - s[0]);              // exp_avg.lerp_(grad, 1 - beta1)
    const float v = s[1] * b2 + omb2 * (gd * gd);           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    s[0] = m;
    s[1] = v;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;     // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    return p - step_size * (m / denom);                     // param.addcdiv_(exp_avg, denom, value=-step_size)
  }
};
// Weight EMA (nunet_optim.ema != NULL, nunet_ema): a wrapper around either functor with the averaged parameters as one more
// state stream. one() runs the wrapped step, then moves the last stream towards the parameter it returns - copied on the
// first update, lerped with this step's w otherwise; both words were written by ema_prepare_kernel in an earlier launch, so
// the choice is uniform over the launch. A skipped step is the wrapped functor's: begin() returns false and nothing is stored.
// The plan's tile kernel (weights.hip) runs it as it is; the flat step (elementwise.hip launch_flat) unwraps it.
template <typename O> struct OptEma {
  static constexpr int NS = O::NS + 1;
  float* st[O::NS + 1];     // the wrapped functor's streams, then ema_params
  O in;
  const nunet_ema* em;
  float w;
  bool copy;
  __device__ __forceinline__ bool begin(float& gscale) {
    w = em->w; copy = em->live == NUNET_EMA_COPY;
    return in.begin(gscale);
  }
  __device__ __forceinline__ float one(float p, float g, float* s) const {
    const float pn = in.one(p, g, s);
    const float e = s[O::NS];
    s[O::NS] = copy ? pn : e + w * (pn - e);
    return pn;
  }
};
// one element at flat index idx: state in, step, state out; returns the new parameter (the caller stores it)
template <typename O> __device__ __forceinline__ float opt_elem(const O& o, float p, float g, long long idx) {
  float s[O::NS];
#pragma unroll
  for (int k = 0; k < O::NS; ++k) s[k] = o.st[k][idx];
  const float pn = o.one(p, g, s);
#pragma unroll
  for (int k = 0; k < O::NS; ++k) o.st[k][idx] = s[k];
  return pn;
}

// Host side of the functors: one validator, one builder per functor, one dispatcher over nunet_optim.kind. Every entry that
// takes a nunet_optim refuses a bad one here, before it touches the device. need_sgd_state: the plan kernels load the
// momentum buffer unconditionally (opt_elem), the flat sgd_kernel only when momentum != 0.
static inline int opt_check(const nunet_optim* o, const char* what, bool need_sgd_state) {
  NUNET_REQUIRE(o, "%s: null optimiser", what);
  const bool sgd = o->kind == NUNET_OPT_SGD;
  NUNET_REQUIRE(sgd || o->kind == NUNET_OPT_ADAM, "%s: unknown optimiser kind %d", what, (int)o->kind);
  NUNET_REQUIRE(!sgd || (o->lr && (o->state0 || (!need_sgd_state && o->momentum == 0.f))), "%s: SGD needs lr and state0 (momentum buffer)", what);
  NUNET_REQUIRE(sgd || (o->adam_scal && o->state0 && o->state1), "%s: Adam needs adam_scal, state0 (exp_avg) and state1 (exp_avg_sq)", what);
  NUNET_REQUIRE(sgd || (o->beta1 >= 0.0 && o->beta1 < 1.0 && o->beta2 >= 0.0 && o->beta2 < 1.0), "%s: betas must lie in [0, 1)", what);
  NUNET_REQUIRE(sgd || o->eps > 0.f, "%s: eps must be > 0", what);
  NUNET_REQUIRE(!o->ema || o->ema_params, "%s: an ema needs ema_params (the averaged parameters)", what);
  NUNET_REQUIRE(o->ema || !o->ema_params, "%s: ema_params without an ema", what);
  NUNET_REQUIRE(((uintptr_t)o->ema & 7) == 0 && ((uintptr_t)o->ema_params & 3) == 0, "%s: ema must be 8-byte aligned, ema_params 4-byte aligned", what);
  return NUNET_OK;
}
static inline OptSgd opt_sgd(const nunet_optim* d) {
  OptSgd o; memset(&o, 0, sizeof(o));
  o.st[0] = d->state0; o.lr_dev = d->lr; o.momc = d->momentum; o.wd = d->weight_decay; o.nesterov = d->nesterov; o.sc = d->scaler; o.cl = d->clip;
  return o;
}
static inline OptAdam opt_adam(const nunet_optim* d) {
  OptAdam o; memset(&o, 0, sizeof(o));
  o.st[0] = d->state0; o.st[1] = d->state1; o.scal_dev = d->adam_scal; o.eps = d->eps; o.wd = d->weight_decay; o.sc = d->scaler; o.cl = d->clip;
  o.omb1 = (float)(1.0 - d->beta1); o.b2 = (float)d->beta2; o.omb2 = (float)(1.0 - d->beta2);
  return o;
}
template <typename O> static inline OptEma<O> opt_ema(const O& in, const nunet_optim* d) {
  OptEma<O> o; memset(&o, 0, sizeof(o));
  for (int k = 0; k < O::NS; ++k) o.st[k] = in.st[k];
  o.st[O::NS] = d->ema_params; o.in = in; o.em = d->ema;
  return o;
}
// f(functor of o->kind, wrapped in OptEma when o->ema is set); `o` has passed opt_check
template <class F> static inline int opt_dispatch(const nunet_optim* o, F&& f) {
  if (o->ema) return o->kind == NUNET_OPT_ADAM ? f(opt_ema(opt_adam(o), o)) : f(opt_ema(opt_sgd(o), o));
  return o->kind == NUNET_OPT_ADAM ? f(opt_adam(o)) : f(opt_sgd(o));
}
