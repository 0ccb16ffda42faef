// loss.hip — losses, metrics, the validation step and the mask export (fp32 logits and targets, NCHW):
//   BCEDiceLoss fwd/bwd, BCEWithLogitsLoss fwd/bwd, the fused loss step of the training loop (the Lovasz form lives in
//   lovasz.hip), IoU counts, per-class segmentation sums, nunet_eval_step / nunet_eval_step_heads, nunet_sigmoid_u8.
// Reference arithmetic: losses.py:103-117; metrics.py; trains.py:118-128,150-188; val.py:100-105.
//
// Every per-block partial sum in this file leaves its workgroup the same way (common.h, slab_park / slab_store): butterfly inside
// each wave, four wave totals through LDS, one barrier, thread q stores ((w0 + w1) + w2) + w3 into entry q of the block's slab entry with a
// plain store. No pre-zero launch, no same-address atomics; the finalising kernels add the entries in a fixed order, so every
// result is bit-identical from run to run.
#include "common.h"

// ---------------------------------------------------------------------------
// per-element expressions, one definition each
// ---------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// l_i = max(x, 0) - x t + log1p(exp(-|x|)): the BCE term of BCEDiceLoss and all of BCEWithLogitsLoss
__device__ __forceinline__ float bce_logits_term(float xv, float tv) { return fmaxf(xv, 0.f) - xv * tv + log1pf(expf(-fabsf(xv))); }
// d (0.5 * mean BCE + 1 - mean Dice) / d x_i of BCEDiceLoss, with D = P + T + 1e-5, num = 2 I + 1e-5 of the element's image
__device__ __forceinline__ float bce_dice_grad(float xv, float tv, float D, float num, float invD2, float kb, float invN) {
  const float pv = sigmoidf_(xv);
  const float ddice = (2.f * tv * D - num) * invD2 * pv * (1.f - pv);
  return kb * (pv - tv) - invN * ddice;
}

// one check of a loss_kind and of the Lovasz hinge's two side conditions for every entry that takes one (an entry without a
// class axis passes K = 1, hw = 0: the Lovasz forward then refuses an image that is too large, in its own words)
static int loss_kind_check(const char* what, int32_t loss_kind, int32_t K, int64_t hw) {
  NUNET_REQUIRE(loss_kind == NUNET_LOSS_BCE_DICE || loss_kind == NUNET_LOSS_LOVASZ_HINGE || loss_kind == NUNET_LOSS_BCE_LOGITS, "%s: loss_kind %d", what, (int)loss_kind);
  NUNET_REQUIRE(loss_kind != NUNET_LOSS_LOVASZ_HINGE || K == 1, "%s: the Lovasz hinge takes one class (the reference squeezes dim 1), got %d", what, (int)K);
  NUNET_REQUIRE(loss_kind != NUNET_LOSS_LOVASZ_HINGE || hw <= (1ll << 22), "%s: the Lovasz hinge takes up to 2^22 pixels per image, got %lld", what, (long long)hw);
  return NUNET_OK;
}

// ---------------------------------------------------------------------------
// BCEDiceLoss (losses.py:107-117), stand-alone and inside the fused loss step of the training loop (trains.py:118-128,135-136):
// all heads' partial sums + IoU counts in one launch; then the gradients of the head-averaged loss, the loss values and the
// running epoch meters in a second one.
// ---------------------------------------------------------------------------
// Per-block partial sums go to a slab [heads][N][LOSS_GX] x {I, P, T, BCE (, iou-inter, iou-union)}. The stand-alone forward
// is the one-head form without the counts on its own grid rule; its slab sits behind the 3N + 1 header of its workspace
// ({I, P, T} per image, the BCE total), which its final kernel fills and its backward reads.
constexpr int LOSS_GX = 64;     // most blocks per (image, head)
// The grids of the loss, metric and export launches, one helper per entry: the launch and nunet_loss_launch_info
// (include/nunet_diag.h) both call it.
static int bce_dice_fwd_gx(int64_t per) { return grid_for(per, 256 * 4, LOSS_GX); }
static int bce_dice_bwd_gx(int64_t per) { return grid_for(per, 256 * 4, 64); }
static int loss_step_gx(int64_t per) { return grid_for(per, 256, LOSS_GX); }    // one element per thread up to 128x128 images: the step waits on this pair of launches
template <bool IOU>
__global__ __launch_bounds__(256) void bce_dice_partial_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t per, float* __restrict__ slab, int N, float iou_thr) {
  constexpr int W = IOU ? 6 : 4;
  const int n = blockIdx.y, hd = IOU ? blockIdx.z : 0;     // (the stand-alone form has one head: its addresses do not wait for N)
  const float* xs = x + ((int64_t)hd * N + n) * per;
  const float* ts = t + (int64_t)n * per;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  unsigned c[2] = {0u, 0u};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const float xv = xs[i], tv = ts[i];
    const float pv = sigmoidf_(xv);
    a[0] += pv * tv; a[1] += pv; a[2] += tv;
    a[3] += bce_logits_term(xv, tv);
    if constexpr (IOU) fg_count2(xv, tv, iou_thr, c[0], c[1]);
  }
  float* dst = slab + ((((size_t)hd * N + n) * LOSS_GX) + blockIdx.x) * W;
  __shared__ float s_a[4][4];
  __shared__ unsigned s_c[4][2];
  if constexpr (IOU) slab_park(a, s_a, c, s_c);
  else slab_park(a, s_a);
  __syncthreads();
  slab_store(s_a, dst, (int)threadIdx.x);
  if constexpr (IOU) slab_store(s_c, dst + 4, (int)threadIdx.x - 4);    // (counts <= 256 * trip count per wave: exact in fp32 up to 2^24 per block)
}
__global__ void bce_dice_final_kernel(float* __restrict__ ws, int N, int gx, int64_t per, float* __restrict__ loss) {
  // single wave: lane l holds partial l of image n (gx <= 64)
  const int l = threadIdx.x;
  float bce = 0.f, d = 0.f;
  for (int n = 0; n < N; ++n) {
    const float* q = ws + 3 * N + 1 + ((size_t)n * LOSS_GX + l) * 4;
    float v0 = l < gx ? q[0] : 0.f, v1 = l < gx ? q[1] : 0.f, v2 = l < gx ? q[2] : 0.f, v3 = l < gx ? q[3] : 0.f;
    v0 = wave_sum(v0); v1 = wave_sum(v1); v2 = wave_sum(v2); v3 = wave_sum(v3);   // (butterfly: every lane holds the totals)
    if (l == 0) { ws[n * 3] = v0; ws[n * 3 + 1] = v1; ws[n * 3 + 2] = v2; }
    bce += v3;
    d += (2.f * v0 + 1e-5f) / (v1 + v2 + 1e-5f);
  }
  if (l == 0) {
    ws[N * 3] = bce;
    loss[0] = 0.5f * (bce / ((float)N * (float)per)) + (1.f - d / (float)N);
  }
}
// The gradient loop of one (image, head) from its image's sums I, P, T: ds[i] = g * grad_i, and with SEED the loss scale sc as
// the last multiply (exact for powers of two; 1 changes nothing).
template <bool SEED>
__device__ __forceinline__ void bce_dice_grad_loop(const float* __restrict__ xs, const float* __restrict__ ts, float* __restrict__ ds, int64_t per, int N,
                                                   float I, float P, float T, float g, float sc) {
  const float D = P + T + 1e-5f;
  const float kb = 0.5f / ((float)N * (float)per);
  const float num = 2.f * I + 1e-5f;
  const float invD2 = 1.f / (D * D);
  const float invN = 1.f / (float)N;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const float d = g * bce_dice_grad(xs[i], ts[i], D, num, invD2, kb, invN);
    ds[i] = SEED ? d * sc : d;
  }
}
__global__ __launch_bounds__(256) void bce_dice_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t per, const float* __restrict__ ws, const float* __restrict__ gscale, float* __restrict__ dx, int N) {
  const int n = blockIdx.y;
  bce_dice_grad_loop<false>(x + (int64_t)n * per, t + (int64_t)n * per, dx + (int64_t)n * per, per, N, ws[n * 3], ws[n * 3 + 1], ws[n * 3 + 2],
                            gscale ? gscale[0] : 1.f, 1.f);
}
extern "C" size_t nunet_bce_dice_ws_bytes(int32_t N) { return (size_t)(3 * N + 1 + (size_t)N * LOSS_GX * 4) * sizeof(float); }
extern "C" int nunet_bce_dice_fwd(const float* logits, const float* target, int32_t N, int64_t per, float* ws, size_t ws_bytes, float* loss, nunet_stream_t s) {
  NUNET_REQUIRE(logits && target && ws && loss && N > 0 && per > 0, "bce_dice_fwd: bad args");
  NUNET_REQUIRE(ws_bytes >= nunet_bce_dice_ws_bytes(N), "bce_dice_fwd: workspace of %zu bytes, nunet_bce_dice_ws_bytes(%d) = %zu", ws_bytes, (int)N, nunet_bce_dice_ws_bytes(N));
  hipStream_t st = (hipStream_t)s;
  const int gx = bce_dice_fwd_gx(per);
  ProfScope ps(PC_LOSS, 0, (double)N * per * 8, st);
  NUNET_LAUNCH(bce_dice_partial_kernel<false>, dim3(gx, N), dim3(256), 0, st, logits, target, per, ws + 3 * N + 1, N, 0.f);
  NUNET_LAUNCH(bce_dice_final_kernel, dim3(1), dim3(64), 0, st, ws, N, gx, per, loss);
  return nunet_check_launch("bce_dice_fwd");
}
extern "C" int nunet_bce_dice_bwd(const float* logits, const float* target, int32_t N, int64_t per, const float* ws, size_t ws_bytes, const float* gscale, float* dlogits, nunet_stream_t s) {
  NUNET_REQUIRE(logits && target && ws && dlogits && N > 0 && per > 0, "bce_dice_bwd: bad args");
  NUNET_REQUIRE(ws_bytes >= nunet_bce_dice_ws_bytes(N), "bce_dice_bwd: workspace of %zu bytes, nunet_bce_dice_ws_bytes(%d) = %zu", ws_bytes, (int)N, nunet_bce_dice_ws_bytes(N));
  const int gx = bce_dice_bwd_gx(per);
  ProfScope ps(PC_LOSS, 0, (double)N * per * 12, (hipStream_t)s);
  NUNET_LAUNCH(bce_dice_bwd_kernel, dim3(gx, N), dim3(256), 0, (hipStream_t)s, logits, target, per, ws, gscale, dlogits, N);
  return nunet_check_launch("bce_dice_bwd");
}

// Second launch of the loss step: every workgroup adds the <= 64 slab entries of its (image, head) with one wave and runs the
// gradient loop with g = 1 / heads; one workgroup also writes the losses and the meters.
__global__ __launch_bounds__(256) void loss_step_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t per, const float* __restrict__ ws, int gx, int N, int heads, float* __restrict__ dx, float* __restrict__ loss_out, double* __restrict__ meters,
                                                            const float* __restrict__ seed_scale) {
  const int n = blockIdx.y, hd = blockIdx.z;
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  const bool on = l < gx;
  __shared__ float s_img[3];
  __shared__ float s_acc[4][8][2];     // [wave][head] {sum of per-image dice terms, BCE sum}
  __shared__ double s_cnt[4][2];
  auto slab = [&](int k, int q) { return ws + ((((size_t)k * N + q) * LOSS_GX) + l) * 6; };
  if (wv == 0) {
    const float* w = slab(hd, n);
    const float I = wave_sum(on ? w[0] : 0.f), P = wave_sum(on ? w[1] : 0.f), T = wave_sum(on ? w[2] : 0.f);
    if (l == 0) { s_img[0] = I; s_img[1] = P; s_img[2] = T; }
  }
  // one block also owns the loss per head, their mean (trains.py:120-123) and the IoU of the last head
  // (trains.py:124,128): its four waves take four images each per pass, all loads of a pass in flight together
  const bool fin = blockIdx.x == 0 && n == 0 && hd == 0;
  if (fin) {
    double ci_s = 0.0, cu_s = 0.0;
    for (int k = 0; k < heads; ++k) {
      float d = 0.f, bce = 0.f;
      for (int q0 = wv; q0 < N; q0 += 16) {
        float v[4][6];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int q = q0 + 4 * u;
#pragma unroll
          for (int c = 0; c < 6; ++c) v[u][c] = (on && q < N) ? slab(k, q)[c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (q0 + 4 * u < N) {
            const float I = wave_sum(v[u][0]), P = wave_sum(v[u][1]), T = wave_sum(v[u][2]);
            d += (2.f * I + 1e-5f) / (P + T + 1e-5f);
            bce += wave_sum(v[u][3]);
            if (k == heads - 1) { ci_s += (double)wave_sum(v[u][4]); cu_s += (double)wave_sum(v[u][5]); }
          }
        }
      }
      if (l == 0) { s_acc[wv][k][0] = d; s_acc[wv][k][1] = bce; }
    }
    if (l == 0) { s_cnt[wv][0] = ci_s; s_cnt[wv][1] = cu_s; }
  }
  __syncthreads();
  if (fin && threadIdx.x == 0) {
    const double inter = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0], uni = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    write_losses_meters(loss_out, heads, meters, inter, uni, [&](int k) {
      const float d = s_acc[0][k][0] + s_acc[1][k][0] + s_acc[2][k][0] + s_acc[3][k][0];
      const float bce = s_acc[0][k][1] + s_acc[1][k][1] + s_acc[2][k][1] + s_acc[3][k][1];
      return 0.5f * bce / ((float)N * (float)per) + (1.f - d / (float)N);
    });
  }
  const int64_t off = ((int64_t)hd * N + n) * per;
  bce_dice_grad_loop<true>(x + off, t + (int64_t)n * per, dx + off, per, N, s_img[0], s_img[1], s_img[2], 1.f / (float)heads, seed_scale ? seed_scale[0] : 1.f);
}

// ---------------------------------------------------------------------------
// BCEWithLogitsLoss (trains.py:27-28,210-211: torch.nn.BCEWithLogitsLoss(), mean over all elements)
// ---------------------------------------------------------------------------
// d loss / dx_i = (sigmoid(x_i) - t_i) / count depends on no sum, so the stand-alone backward needs no workspace and the loss
// step forms it in the pass that sums l_i.
constexpr int BCEL_GX = 256;    // most blocks of the stand-alone pair: one element per thread up to 65536, a grid-stride loop above
static int bce_logits_gx(int64_t n) { return grid_for(n, 256, BCEL_GX); }
__global__ __launch_bounds__(256) void bce_logits_partial_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t n, float* __restrict__ ws) {
  float a[1] = {0.f};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) a[0] += bce_logits_term(x[i], t[i]);
  __shared__ float s_a[4][1];
  block256_slab_store(a, s_a, ws + blockIdx.x);    // one partial per block
}
__global__ void bce_logits_final_kernel(const float* __restrict__ ws, int gx, int64_t n, float* __restrict__ loss) {
  // single wave: lane l adds partials l, l + 64, ... in that order, then the butterfly (a fixed order: bit-reproducible)
  const int l = threadIdx.x;
  float v = 0.f;
  for (int b = l; b < gx; b += 64) v += ws[b];
  v = wave_sum(v);
  if (l == 0) loss[0] = v / (float)n;
}
__global__ __launch_bounds__(256) void bce_logits_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t n, const float* __restrict__ gscale, float* __restrict__ dx) {
  const float g = gscale ? gscale[0] : 1.f;
  const float k = 1.f / (float)n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dx[i] = (sigmoidf_(x[i]) - t[i]) * k * g;    // the upstream scale is the last multiply: a power of two is exact
}
extern "C" size_t nunet_bce_logits_ws_bytes(int64_t n) { return n > 0 ? (size_t)bce_logits_gx(n) * sizeof(float) : 0; }
extern "C" int nunet_bce_logits_fwd(const float* logits, const float* target, int64_t n, float* ws, size_t ws_bytes, float* loss, nunet_stream_t s) {
  NUNET_REQUIRE(logits && target && ws && loss && n > 0, "bce_logits_fwd: bad args");
  NUNET_REQUIRE(ws_bytes >= nunet_bce_logits_ws_bytes(n), "bce_logits_fwd: workspace of %zu bytes, nunet_bce_logits_ws_bytes(%lld) = %zu", ws_bytes,
                (long long)n, nunet_bce_logits_ws_bytes(n));
  hipStream_t st = (hipStream_t)s;
  const int gx = bce_logits_gx(n);
  ProfScope ps(PC_LOSS, 0, (double)n * 8, st);
  NUNET_LAUNCH(bce_logits_partial_kernel, dim3(gx), dim3(256), 0, st, logits, target, n, ws);
  NUNET_LAUNCH(bce_logits_final_kernel, dim3(1), dim3(64), 0, st, ws, gx, n, loss);
  return nunet_check_launch("bce_logits_fwd");
}
extern "C" int nunet_bce_logits_bwd(const float* logits, const float* target, int64_t n, const float* gscale, float* dlogits, nunet_stream_t s) {
  NUNET_REQUIRE(logits && target && dlogits && n > 0, "bce_logits_bwd: bad args");
  ProfScope ps(PC_LOSS, 0, (double)n * 12, (hipStream_t)s);
  NUNET_LAUNCH(bce_logits_bwd_kernel, dim3(bce_logits_gx(n)), dim3(256), 0, (hipStream_t)s, logits, target, n, gscale, dlogits);
  return nunet_check_launch("bce_logits_bwd");
}

// Loss step, NUNET_LOSS_BCE_LOGITS: one pass over [heads][N][per] on the grid of the BCE-Dice kind reads logits and targets once,
// stores d mean / d logits and leaves per-block slabs [heads][N][LOSS_GX] x {BCE sum, iou-inter, iou-union}; one workgroup then
// adds the slabs in a fixed order and writes the losses and the meters.
__global__ __launch_bounds__(256) void bce_logits_step_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t per, float* __restrict__ ws, int N, int heads, float iou_thr,
                                                              float* __restrict__ dx, const float* __restrict__ seed_scale) {
  const int n = blockIdx.y, hd = blockIdx.z;
  const float* xs = x + ((int64_t)hd * N + n) * per;
  const float* ts = t + (int64_t)n * per;
  float* ds = dx + ((int64_t)hd * N + n) * per;
  const float k = 1.f / ((float)N * (float)per * (float)heads);    // mean over all elements, then over the heads (trains.py:120-123)
  const float sc = seed_scale ? seed_scale[0] : 1.f;                // loss scaling: the last multiply
  float a[1] = {0.f};
  unsigned c[2] = {0u, 0u};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const float xv = xs[i], tv = ts[i];
    ds[i] = (sigmoidf_(xv) - tv) * k * sc;
    a[0] += bce_logits_term(xv, tv);
    fg_count2(xv, tv, iou_thr, c[0], c[1]);
  }
  float* dst = ws + ((((size_t)hd * N + n) * LOSS_GX) + blockIdx.x) * 3;
  __shared__ float s_a[4][1];
  __shared__ unsigned s_c[4][2];
  slab_park(a, s_a, c, s_c);
  __syncthreads();
  slab_store(s_a, dst, (int)threadIdx.x);
  slab_store(s_c, dst + 1, (int)threadIdx.x - 1);    // (counts <= 2^24 per image: exact in fp32)
}
__global__ __launch_bounds__(256) void bce_logits_step_final_kernel(const float* __restrict__ ws, int gx, int N, int heads, int64_t per, float* __restrict__ loss_out, double* __restrict__ meters) {
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ float s_bce[4][8];
  __shared__ double s_cnt[4][2];
  const int64_t slabs = (int64_t)N * gx;     // thread j takes slabs j, j + 256, ... of every head, image-major: a fixed order
  double ci = 0.0, cu = 0.0;
  for (int k = 0; k < heads; ++k) {
    float bce = 0.f;
    for (int64_t j = threadIdx.x; j < slabs; j += 256) {
      const int64_t q = j / gx;
      const float* w = ws + ((((size_t)k * N + q) * LOSS_GX) + (j - q * gx)) * 3;
      bce += w[0];
      if (k == heads - 1) { ci += (double)w[1]; cu += (double)w[2]; }    // IoU of the last head (trains.py:124,128)
    }
    bce = wave_sum(bce);
    if (l == 0) s_bce[wv][k] = bce;
  }
  ci = wave_sum_f64(ci); cu = wave_sum_f64(cu);
  if (l == 0) { s_cnt[wv][0] = ci; s_cnt[wv][1] = cu; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double inter = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0], uni = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    write_losses_meters(loss_out, heads, meters, inter, uni, [&](int k) {
      const float bce = ((s_bce[0][k] + s_bce[1][k]) + s_bce[2][k]) + s_bce[3][k];
      return bce / ((float)N * (float)per);
    });
  }
}

// ---------------------------------------------------------------------------
// nunet_loss_step: the three loss kinds behind one entry
// ---------------------------------------------------------------------------
size_t lovasz_step_ws_bytes(int32_t N, int64_t per, int32_t heads);    // lovasz.hip
int lovasz_loss_step(const float* logits, const float* target, int32_t N, int64_t per, int32_t heads, float* ws, float* dlogits,
                     float* loss_out, double* meters, float iou_thr, const float* seed_scale, hipStream_t st);
extern "C" size_t nunet_loss_step_ws_bytes(int32_t N, int64_t per, int32_t heads, int32_t loss_kind) {
  if (N <= 0 || per <= 0 || heads < 1) return 0;
  if (loss_kind == NUNET_LOSS_LOVASZ_HINGE) return lovasz_step_ws_bytes(N, per, heads);
  return (size_t)heads * N * LOSS_GX * (loss_kind == NUNET_LOSS_BCE_LOGITS ? 3 : 6) * sizeof(float);
}
static int loss_step(const float* logits, const float* target, int32_t N, int64_t per, int32_t heads, int32_t loss_kind, float* ws, size_t ws_bytes,
                     float* dlogits, float* loss_out, double* meters, float iou_logit_threshold, const float* seed_scale, nunet_stream_t s) {
  NUNET_REQUIRE(logits && target && ws && dlogits && loss_out && N > 0 && per > 0 && heads >= 1 && heads <= 8, "loss_step: bad args");
  if (int rc = loss_kind_check("loss_step", loss_kind, 1, 0)) return rc;
  NUNET_REQUIRE(per <= (1ll << 24), "loss_step: image too large");    // per-image IoU counts stay exact in fp32
  NUNET_REQUIRE(ws_bytes >= nunet_loss_step_ws_bytes(N, per, heads, loss_kind), "loss_step: workspace of %zu bytes, nunet_loss_step_ws_bytes = %zu",
                ws_bytes, nunet_loss_step_ws_bytes(N, per, heads, loss_kind));
  hipStream_t st = (hipStream_t)s;
  if (loss_kind == NUNET_LOSS_LOVASZ_HINGE)
    return lovasz_loss_step(logits, target, N, per, heads, ws, dlogits, loss_out, meters, iou_logit_threshold, seed_scale, st);
  const int gx = loss_step_gx(per);
  const dim3 grid(gx, N, heads);
  ProfScope ps(PC_LOSS, 0, (double)N * per * heads * (loss_kind == NUNET_LOSS_BCE_LOGITS ? 12 : 16), st);
  if (loss_kind == NUNET_LOSS_BCE_LOGITS) {
    NUNET_LAUNCH(bce_logits_step_kernel, grid, dim3(256), 0, st, logits, target, per, ws, N, heads, iou_logit_threshold, dlogits, seed_scale);
    NUNET_LAUNCH(bce_logits_step_final_kernel, dim3(1), dim3(256), 0, st, ws, gx, N, heads, per, loss_out, meters);
  } else {
    NUNET_LAUNCH(bce_dice_partial_kernel<true>, grid, dim3(256), 0, st, logits, target, per, ws, N, iou_logit_threshold);
    NUNET_LAUNCH(loss_step_bwd_kernel, grid, dim3(256), 0, st, logits, target, per, ws, gx, N, heads, dlogits, loss_out, meters, seed_scale);
  }
  return nunet_check_launch("loss_step");
}
extern "C" int nunet_loss_step(const float* logits, const float* target, int32_t N, int64_t per, int32_t heads, int32_t loss_kind, float* ws, size_t ws_bytes,
                               float* dlogits, float* loss_out, double* meters, float iou_logit_threshold, nunet_stream_t s) {
  return loss_step(logits, target, N, per, heads, loss_kind, ws, ws_bytes, dlogits, loss_out, meters, iou_logit_threshold, nullptr, s);
}
extern "C" int nunet_loss_step_scaled(const float* logits, const float* target, int32_t N, int64_t per, int32_t heads, int32_t loss_kind, float* ws,
                                      size_t ws_bytes, float* dlogits, float* loss_out, double* meters, float iou_logit_threshold,
                                      const float* seed_scale, nunet_stream_t s) {
  NUNET_REQUIRE(seed_scale, "loss_step_scaled: null seed_scale");
  return loss_step(logits, target, N, per, heads, loss_kind, ws, ws_bytes, dlogits, loss_out, meters, iou_logit_threshold, seed_scale, s);
}

// ---------------------------------------------------------------------------
// iou_score counts (metrics.py:10-14): sigmoid(x) > 0.5  <=>  x >= thr, with thr the smallest fp32 logit whose
// REFERENCE sigmoid (fp32, rounded) exceeds 0.5 - not x > 0: in fp32, sigmoid(x) == 0.5 exactly for 0 < x <~ 6e-8.
// The caller derives thr from the reference's own sigmoid by bisection (metrics.iou_logit_threshold). NaN -> false.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iou_counts_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t n, float thr, unsigned long long* __restrict__ counts) {
  unsigned int ci = 0, cu = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) fg_count2(x[i], t[i], thr, ci, cu);
  ci = wave_sum_u32(ci); cu = wave_sum_u32(cu);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counts[0], (unsigned long long)ci);
    atomicAdd(&counts[1], (unsigned long long)cu);
  }
}
static int iou_counts_gx(int64_t n) { return grid_for(n, 256 * 4, 256); }
extern "C" int nunet_iou_counts(const float* logits, const float* target, int64_t n, float logit_threshold, unsigned long long* counts, nunet_stream_t s) {
  NUNET_REQUIRE(logits && target && counts && n > 0, "iou_counts: bad args");
  ProfScope ps(PC_LOSS, 0, (double)n * 8, (hipStream_t)s);
  NUNET_LAUNCH(iou_counts_kernel, dim3(iou_counts_gx(n)), dim3(256), 0, (hipStream_t)s, logits, target, n, logit_threshold, counts);
  return nunet_check_launch("iou_counts");
}

// ---------------------------------------------------------------------------
// Segmentation sums of HEADS logits tensors [HEADS][N][K][hw] over ONE read of the targets (the rest of the reference's
// metrics.py: numeric_score's FP/FN/TP/TN :31-44, Acc :47-53, dice_coef :21-29) per class, with the foreground rule of
// iou_counts_kernel - so sum tp and sum (tp + fp + fn) over the classes ARE nunet_iou_counts' intersection and union.
// One read of logits and targets on the grid (blocks per plane, class, image): a thread loads its target value once and walks
// the heads' logits over it; every workgroup leaves one partial {soft_i, soft_p, soft_t (double), tp, fp, fn, tn (uint32: a
// plane holds <= 2^24 pixels)} per head, head h's in slab h (ws + h * N * K * SEG_GX) - the partition of a plane's pixels and
// the order of every sum do not depend on HEADS, so slab h holds what the one-head launch leaves for head h's logits alone.
// One workgroup per slab then adds the entries of a class in index order (image-major, thread j takes entries j, j + 256, ...;
// a fixed tree over lanes and waves). nunet_seg_metrics and the last-head eval step are the one-head form.
// ---------------------------------------------------------------------------
constexpr int SEG_GX = 64;      // most blocks per (image, class) plane
#define NUNET_EVAL_MAX_HEADS 4  // most slabs of one launch
struct SegPart { double s[3]; unsigned c[4]; };    // 40 bytes
static int seg_metrics_gx(int64_t hw) { return grid_for(hw, 256, SEG_GX); }
template <int HEADS>
__global__ __launch_bounds__(256) void seg_metrics_partial_heads_kernel(const float* __restrict__ x, const float* __restrict__ t, int64_t hw, float thr, SegPart* __restrict__ ws) {
  const int k = blockIdx.y, n = blockIdx.z, K = gridDim.y;
  const int64_t plane = (int64_t)n * K + k;
  const int64_t n_head = (int64_t)gridDim.z * K * hw;
  const float* xs = x + plane * hw;
  const float* ts = t + plane * hw;
  double d[HEADS][3];       // soft_i, soft_p, soft_t
  unsigned c[HEADS][4];     // tp, fp, fn, tn
#pragma unroll
  for (int h = 0; h < HEADS; ++h) { d[h][0] = 0.0; d[h][1] = 0.0; d[h][2] = 0.0; c[h][0] = 0; c[h][1] = 0; c[h][2] = 0; c[h][3] = 0; }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) {
    const float tv = ts[i];
#pragma unroll
    for (int h = 0; h < HEADS; ++h) {
      const float xv = xs[h * n_head + i];
      const double pv = (double)sigmoidf_(xv);
      d[h][0] += pv * (double)tv; d[h][1] += pv; d[h][2] += (double)tv;
      fg_count4(xv, tv, thr, c[h][0], c[h][1], c[h][2], c[h][3]);
    }
  }
  __shared__ double s_d[HEADS][4][3];
  __shared__ unsigned s_c[HEADS][4][4];
#pragma unroll
  for (int h = 0; h < HEADS; ++h) slab_park(d[h], s_d[h], c[h], s_c[h]);
  __syncthreads();
  const int h = threadIdx.x >> 3, q7 = threadIdx.x & 7;      // eight threads per head: three doubles, four counts
  if (h < HEADS) {
    SegPart* w = ws + ((int64_t)h * gridDim.z * K + plane) * SEG_GX + blockIdx.x;
    slab_store(s_d[h], w->s, q7);
    slab_store(s_c[h], w->c, q7 - 3);
  }
}
// (workgroup blockIdx.x finishes slab blockIdx.x into out[blockIdx.x])
__global__ __launch_bounds__(256) void seg_metrics_final_kernel(const SegPart* __restrict__ ws, int gx, int N, int K, nunet_seg_sums* __restrict__ out, int accumulate) {
  ws += (int64_t)blockIdx.x * N * K * SEG_GX; out += blockIdx.x;
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ double s_d[4][NUNET_EVAL_MAX_CLASSES][3];
  __shared__ unsigned long long s_c[4][NUNET_EVAL_MAX_CLASSES][4];
  const int64_t entries = (int64_t)N * gx;     // of one class, image-major
  for (int k = 0; k < K; ++k) {
    double d[3] = {0.0, 0.0, 0.0};
    unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
    for (int64_t j = threadIdx.x; j < entries; j += 256) {
      const int64_t n = j / gx;
      const SegPart* w = ws + (n * K + k) * SEG_GX + (j - n * gx);
#pragma unroll
      for (int q = 0; q < 3; ++q) d[q] += w->s[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) c[q] += (unsigned long long)w->c[q];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) d[q] = wave_sum_f64(d[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      for (int o = 32; o > 0; o >>= 1) c[q] += __shfl_xor(c[q], o);
    if (l == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) s_d[wv][k][q] = d[q];
#pragma unroll
      for (int q = 0; q < 4; ++q) s_c[wv][k][q] = c[q];
    }
  }
  __syncthreads();
  if (threadIdx.x < NUNET_EVAL_MAX_CLASSES) {     // one thread per class; classes >= K hold zeros after an assigning call
    const int k = threadIdx.x;
    const bool on = k < K;
    double d[3]; unsigned long long c[4];
#pragma unroll
    for (int q = 0; q < 3; ++q) d[q] = on ? ((s_d[0][k][q] + s_d[1][k][q]) + s_d[2][k][q]) + s_d[3][k][q] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = on ? ((s_c[0][k][q] + s_c[1][k][q]) + s_c[2][k][q]) + s_c[3][k][q] : 0ull;
    if (accumulate) {
      if (on) {
        out->tp[k] += c[0]; out->fp[k] += c[1]; out->fn[k] += c[2]; out->tn[k] += c[3];
        out->soft_i[k] += d[0]; out->soft_p[k] += d[1]; out->soft_t[k] += d[2];
      }
    } else {
      out->tp[k] = c[0]; out->fp[k] = c[1]; out->fn[k] = c[2]; out->tn[k] = c[3];
      out->soft_i[k] = d[0]; out->soft_p[k] = d[1]; out->soft_t[k] = d[2];
    }
  }
}
extern "C" size_t nunet_seg_metrics_ws_bytes(int32_t N, int32_t K, int64_t hw) {
  if (N <= 0 || K <= 0 || K > NUNET_EVAL_MAX_CLASSES || hw <= 0) return 0;
  return (size_t)N * K * SEG_GX * sizeof(SegPart);
}
static int seg_metrics_check(const char* what, int32_t N, int32_t K, int64_t hw) {
  NUNET_REQUIRE(N > 0 && N <= 65535, "%s: N = %d (1 .. 65535)", what, (int)N);
  NUNET_REQUIRE(K >= 1 && K <= NUNET_EVAL_MAX_CLASSES, "%s: %d classes (1 .. %d)", what, (int)K, NUNET_EVAL_MAX_CLASSES);
  NUNET_REQUIRE(hw > 0 && hw <= (1ll << 24), "%s: %lld pixels per plane (1 .. 2^24)", what, (long long)hw);
  return NUNET_OK;
}
// both launches for `slabs` (1 .. NUNET_EVAL_MAX_HEADS) logits tensors: slab h of ws into out[h]
static void seg_metrics_launch(const float* logits, const float* target, int32_t N, int32_t K, int64_t hw, float thr, void* ws, nunet_seg_sums* out,
                               int32_t accumulate, int slabs, hipStream_t st) {
  const int gx = seg_metrics_gx(hw);
  const dim3 grid(gx, K, N);
  SegPart* part = (SegPart*)ws;
  ProfScope ps(PC_LOSS, 0, (double)N * K * hw * 4 * (slabs + 1), st);
  switch (slabs) {
    case 1: NUNET_LAUNCH(seg_metrics_partial_heads_kernel<1>, grid, dim3(256), 0, st, logits, target, hw, thr, part); break;
    case 2: NUNET_LAUNCH(seg_metrics_partial_heads_kernel<2>, grid, dim3(256), 0, st, logits, target, hw, thr, part); break;
    case 3: NUNET_LAUNCH(seg_metrics_partial_heads_kernel<3>, grid, dim3(256), 0, st, logits, target, hw, thr, part); break;
    default: NUNET_LAUNCH(seg_metrics_partial_heads_kernel<4>, grid, dim3(256), 0, st, logits, target, hw, thr, part); break;
  }
  NUNET_LAUNCH(seg_metrics_final_kernel, dim3(slabs), dim3(256), 0, st, (const SegPart*)part, gx, N, K, out, accumulate);
}
extern "C" int nunet_seg_metrics(const float* logits, const float* target, int32_t N, int32_t K, int64_t hw, float iou_logit_threshold,
                                 void* ws, size_t ws_bytes, nunet_seg_sums* out, int32_t accumulate, nunet_stream_t s) {
  if (int rc = seg_metrics_check("seg_metrics", N, K, hw)) return rc;
  NUNET_REQUIRE(logits && target && ws && out, "seg_metrics: null pointer");
  NUNET_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0, "seg_metrics: workspace and sums must be 8-byte aligned");
  NUNET_REQUIRE(ws_bytes >= nunet_seg_metrics_ws_bytes(N, K, hw), "seg_metrics: workspace of %zu bytes, nunet_seg_metrics_ws_bytes = %zu", ws_bytes,
                nunet_seg_metrics_ws_bytes(N, K, hw));
  seg_metrics_launch(logits, target, N, K, hw, iou_logit_threshold, ws, out, accumulate, 1, (hipStream_t)s);
  return nunet_check_launch("seg_metrics");
}
extern "C" int nunet_seg_metrics_launch_info(int32_t N, int32_t K, int64_t hw, nunet_loss_launch_info_t* out) {
  NUNET_REQUIRE(out, "seg_metrics launch info: null output");
  if (int rc = seg_metrics_check("seg_metrics launch info", N, K, hw)) return rc;
  fill_launch_info(out, seg_metrics_gx(hw), K, N, hw);
  return NUNET_OK;
}

// ---------------------------------------------------------------------------
// One validation batch without a gradient (trains.py:150-188): the loss of every head BY THE STAND-ALONE FORWARDS (their
// kernels on their grids: loss_out[k] is what the losses.* module returns for head k, bit for bit), the segmentation sums of
// the last head (trains.py:170,174) - or, with head meters, of every head over one read of the targets, so that a validation
// pass shows which depth of a deep-supervision UNet++ would do - and one finalising launch that forms the head mean, the
// batch values and the AverageMeter sums. Both forms make the same number of launches.
// ---------------------------------------------------------------------------
// The workspace, every region 256-byte aligned: per head the forward's own workspace, (Lovasz) the unit-gradient scratch the
// forward writes and nobody reads, one seg_metrics slab and one nunet_seg_sums - per head with head meters, else one of each.
struct EvalLayout {
  size_t head_ws;                   // stride of the heads' loss workspaces, which start at offset 0
  size_t unit, seg, sums, total;    // offsets of the scratch, the slab(s), the batch sums; the size of it all
  EvalLayout(int32_t N, int32_t K, int64_t hw, int32_t heads, int32_t loss_kind, bool per_head) {
    const size_t slabs = per_head ? heads : 1;
    head_ws = align_up(loss_kind == NUNET_LOSS_LOVASZ_HINGE ? nunet_lovasz_ws_bytes(N, hw)
                       : loss_kind == NUNET_LOSS_BCE_LOGITS ? nunet_bce_logits_ws_bytes((int64_t)N * K * hw) : nunet_bce_dice_ws_bytes(N), 256);
    unit = (size_t)heads * head_ws;
    seg = unit + (loss_kind == NUNET_LOSS_LOVASZ_HINGE ? align_up((size_t)N * hw * sizeof(float), 256) : 0);
    sums = seg + align_up(slabs * nunet_seg_metrics_ws_bytes(N, K, hw), 256);
    total = sums + align_up(slabs * sizeof(nunet_seg_sums), 256);
  }
};
// what tells the two entries apart: the name in the messages ("nunet_<name>_ws_bytes" is the entry's workspace function), the
// head limit, and whether every head gets meters (head_meters required) or the last one only (head_meters null)
struct EvalEntry { const char* name; int32_t max_heads; bool per_head; };
static const EvalEntry EVAL_STEP = {"eval_step", 8, false}, EVAL_STEP_HEADS = {"eval_step_heads", NUNET_EVAL_MAX_HEADS, true};
static size_t eval_ws_bytes(const EvalEntry& e, int32_t N, int32_t K, int64_t hw, int32_t heads, int32_t loss_kind) {
  if (N <= 0 || K <= 0 || K > NUNET_EVAL_MAX_CLASSES || hw <= 0 || heads < 1 || heads > e.max_heads) return 0;
  return EvalLayout(N, K, hw, heads, loss_kind, e.per_head).total;
}
extern "C" size_t nunet_eval_step_ws_bytes(int32_t N, int32_t K, int64_t hw, int32_t heads, int32_t loss_kind) { return eval_ws_bytes(EVAL_STEP, N, K, hw, heads, loss_kind); }
extern "C" size_t nunet_eval_step_heads_ws_bytes(int32_t N, int32_t K, int64_t hw, int32_t heads, int32_t loss_kind) {
  return eval_ws_bytes(EVAL_STEP_HEADS, N, K, hw, heads, loss_kind);
}
// one thread: the batch values of one logits tensor from its sums `b`, and the AverageMeter update of `m` with them and `mean`
__device__ __forceinline__ void eval_meter_update(float mean, const nunet_seg_sums* __restrict__ b, nunet_eval_meters* __restrict__ m, int N, int K, int64_t hw) {
#pragma clang fp contract(off)      // sum += value * N as AverageMeter evaluates it: the product rounded, then the add
  unsigned long long tp = 0, fp = 0, fn = 0, tn = 0;
  double si = 0.0, sp = 0.0, st = 0.0;
  for (int k = 0; k < K; ++k) {
    tp += b->tp[k]; fp += b->fp[k]; fn += b->fn[k]; tn += b->tn[k];
    si += b->soft_i[k]; sp += b->soft_p[k]; st += b->soft_t[k];
    m->tp[k] += b->tp[k]; m->fp[k] += b->fp[k]; m->fn[k] += b->fn[k]; m->tn[k] += b->tn[k];
    m->soft_i[k] += b->soft_i[k]; m->soft_p[k] += b->soft_p[k]; m->soft_t[k] += b->soft_t[k];
  }
  const double iou = ((double)tp + 1e-5) / ((double)(tp + fp + fn) + 1e-5);
  const double dice = (2.0 * si + 1e-5) / (sp + st + 1e-5);
  const double acc = (double)(tp + tn) / ((double)N * (double)K * (double)hw);
  const double w = (double)N;                     // AverageMeter.update(value, N)
  m->loss_sum += (double)mean * w; m->iou_sum += iou * w; m->dice_sum += dice * w; m->acc_sum += acc * w;
  m->samples += w;
  m->last_iou = iou; m->last_dice = dice; m->last_acc = acc;
}
__device__ __forceinline__ float eval_head_mean(const float* __restrict__ loss, int heads) {
#pragma clang fp contract(off)
  float mean = loss[0];                           // sum(criterion(o, t) for o in out) / len(out): left to right, one division
  for (int k = 1; k < heads; ++k) mean += loss[k];
  return mean / (float)heads;
}
// The finalising launch. With head meters (hm, heads + 1 workgroups; b: the sums of the heads, [heads]): workgroup h < heads
// updates hm[h] as a one-head step over head h would (its loss is the mean of one value). The last workgroup - the only one
// without head meters, where b is the last head's sums alone - writes the head mean into loss_out[heads] and updates `m` from
// the last head's sums.
__global__ void eval_finalize_heads_kernel(float* __restrict__ loss_out, int heads, const nunet_seg_sums* __restrict__ b, nunet_eval_meters* __restrict__ m,
                                           nunet_eval_meters* __restrict__ hm, int N, int K, int64_t hw) {
  if (threadIdx.x != 0) return;
  const int h = blockIdx.x;
  if (hm && h < heads) {
    eval_meter_update(eval_head_mean(loss_out + h, 1), b + h, hm + h, N, K, hw);
  } else {
    const float mean = eval_head_mean(loss_out, heads);
    loss_out[heads] = mean;
    eval_meter_update(mean, hm ? b + (heads - 1) : b, m, N, K, hw);
  }
}
static int eval_step_impl(const EvalEntry& e, const float* logits, const float* target, int32_t N, int32_t K, int64_t hw,
                          int32_t heads, int32_t loss_kind, void* ws, size_t ws_bytes, float* loss_out, nunet_eval_meters* meters,
                          nunet_eval_meters* head_meters, float iou_logit_threshold, nunet_stream_t s) {
  const char* what = e.name;
  const bool per_head = e.per_head;
  if (int rc = seg_metrics_check(what, N, K, hw)) return rc;
  NUNET_REQUIRE(heads >= 1 && heads <= e.max_heads, "%s: %d heads (1 .. %d)", what, (int)heads, (int)e.max_heads);
  if (int rc = loss_kind_check(what, loss_kind, K, hw)) return rc;
  NUNET_REQUIRE(logits && target && ws && loss_out && meters && (!per_head || head_meters), "%s: null pointer", what);
  NUNET_REQUIRE(((uintptr_t)ws & 255) == 0 && ((uintptr_t)meters & 7) == 0 && (!per_head || ((uintptr_t)head_meters & 7) == 0),
                "%s: workspace must be 256-byte and meters 8-byte aligned", what);
  const EvalLayout lay(N, K, hw, heads, loss_kind, per_head);
  NUNET_REQUIRE(ws_bytes >= lay.total, "%s: workspace of %zu bytes, nunet_%s_ws_bytes = %zu", what, ws_bytes, what, lay.total);
  hipStream_t st = (hipStream_t)s;
  char* base = (char*)ws;
  float* unit = (float*)(base + lay.unit);
  nunet_seg_sums* batch = (nunet_seg_sums*)(base + lay.sums);
  const int64_t per = (int64_t)K * hw, n_head = (int64_t)N * per;
  for (int k = 0; k < heads; ++k) {
    const float* lg = logits + (size_t)k * n_head;
    float* hw_ws = (float*)(base + (size_t)k * lay.head_ws);
    int rc;
    if (loss_kind == NUNET_LOSS_LOVASZ_HINGE) rc = nunet_lovasz_hinge_fwd(lg, target, N, hw, hw_ws, lay.head_ws, unit, loss_out + k, s);
    else if (loss_kind == NUNET_LOSS_BCE_LOGITS) rc = nunet_bce_logits_fwd(lg, target, n_head, hw_ws, lay.head_ws, loss_out + k, s);
    else rc = nunet_bce_dice_fwd(lg, target, N, per, hw_ws, lay.head_ws, loss_out + k, s);
    if (rc) return rc;
  }
  seg_metrics_launch(per_head ? logits : logits + (size_t)(heads - 1) * n_head, target, N, K, hw, iou_logit_threshold, base + lay.seg, batch, 0,
                     per_head ? heads : 1, st);
  NUNET_LAUNCH(eval_finalize_heads_kernel, dim3(per_head ? heads + 1 : 1), dim3(64), 0, st, loss_out, heads, (const nunet_seg_sums*)batch, meters, head_meters, N, K, hw);
  return nunet_check_launch(what);
}
extern "C" int nunet_eval_step(const float* logits, const float* target, int32_t N, int32_t K, int64_t hw, int32_t heads, int32_t loss_kind,
                               void* ws, size_t ws_bytes, float* loss_out, nunet_eval_meters* meters, float iou_logit_threshold, nunet_stream_t s) {
  return eval_step_impl(EVAL_STEP, logits, target, N, K, hw, heads, loss_kind, ws, ws_bytes, loss_out, meters, nullptr, iou_logit_threshold, s);
}
extern "C" int nunet_eval_step_heads(const float* logits, const float* target, int32_t N, int32_t K, int64_t hw, int32_t heads, int32_t loss_kind,
                                     void* ws, size_t ws_bytes, float* loss_out, nunet_eval_meters* meters, nunet_eval_meters* head_meters,
                                     float iou_logit_threshold, nunet_stream_t s) {
  return eval_step_impl(EVAL_STEP_HEADS, logits, target, N, K, hw, heads, loss_kind, ws, ws_bytes, loss_out, meters, head_meters,
                        iou_logit_threshold, s);
}

// ---------------------------------------------------------------------------
// Mask export of the evaluation driver: uint8(sigmoid(logit) * 255), truncating like numpy's astype('uint8')
// (reference val.py:100-105: `(output[i, c] * 255).astype('uint8')` after torch.sigmoid)
// ---------------------------------------------------------------------------
// byte = number of thresholds <= x: thr[k-1] (k = 1..255) is the smallest fp32 logit whose reference byte is >= k, found
// by the caller with the reference's own sigmoid (bisection over fp32 bit patterns, metrics.sigmoid_u8_thresholds), so
// the byte matches `(torch.sigmoid(x) * 255).astype('uint8')` EXACTLY - a device expf one ulp away from the host's would
// flip bytes whose sigmoid * 255 sits next to an integer. Branch-free 8-step binary search in LDS (common.h, sigmoid_byte; the
// stitch kernel of tiles.hip exports its blended logits through the same function).
__global__ __launch_bounds__(256) void sigmoid_u8_kernel(const float* __restrict__ logits, const float* __restrict__ thr, uint8_t* __restrict__ out, int64_t n) {
  __shared__ float s_thr[256];
  if (threadIdx.x < 255) s_thr[threadIdx.x] = thr[threadIdx.x];
  __syncthreads();
  const int64_t n4 = n / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 v = reinterpret_cast<const f32x4*>(logits)[i];
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w |= sigmoid_byte(s_thr, v[e]) << (8 * e);
    reinterpret_cast<uint32_t*>(out)[i] = w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - n4 * 4)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    out[i] = (uint8_t)sigmoid_byte(s_thr, logits[i]);
  }
}
static int sigmoid_u8_gx(int64_t n) { return grid_for(n / 4 + 1, 256, 2048); }
extern "C" int nunet_sigmoid_u8(const float* logits, const float* thresholds, uint8_t* out, int64_t n, nunet_stream_t s) {
  NUNET_REQUIRE(logits && thresholds && out && n > 0, "sigmoid_u8: bad args");
  NUNET_REQUIRE(((uintptr_t)logits & 15) == 0 && ((uintptr_t)out & 3) == 0, "sigmoid_u8: logits must be 16-byte and out 4-byte aligned");
  NUNET_LAUNCH(sigmoid_u8_kernel, dim3(sigmoid_u8_gx(n)), dim3(256), 0, (hipStream_t)s, logits, thresholds, out, n);
  return nunet_check_launch("sigmoid_u8");
}

// Launch geometry of the entries above (include/nunet_diag.h): the grids come from the helpers the launches call.
extern "C" int nunet_loss_launch_info(int32_t entry, int32_t N, int64_t per_or_n, int32_t heads, nunet_loss_launch_info_t* out) {
  NUNET_REQUIRE(out, "loss launch info: null output");
  NUNET_REQUIRE(per_or_n > 0, "loss launch info: %lld elements", (long long)per_or_n);
  int gx = 0, gy = 1, gz = 1;
  int64_t items = per_or_n;
  switch (entry) {
    case NUNET_LOSS_ENTRY_BCE_DICE_FWD:
    case NUNET_LOSS_ENTRY_BCE_DICE_BWD:
      NUNET_REQUIRE(N > 0, "loss launch info: N = %d", (int)N);
      gx = entry == NUNET_LOSS_ENTRY_BCE_DICE_FWD ? bce_dice_fwd_gx(per_or_n) : bce_dice_bwd_gx(per_or_n); gy = N;
      break;
    case NUNET_LOSS_ENTRY_LOSS_STEP:
      NUNET_REQUIRE(N > 0 && heads >= 1 && heads <= 8, "loss launch info: N = %d, heads = %d", (int)N, (int)heads);
      NUNET_REQUIRE(per_or_n <= (1ll << 24), "loss_step: image too large");
      gx = loss_step_gx(per_or_n); gy = N; gz = heads;
      break;
    case NUNET_LOSS_ENTRY_IOU_COUNTS: gx = iou_counts_gx(per_or_n); break;
    case NUNET_LOSS_ENTRY_SIGMOID_U8: gx = sigmoid_u8_gx(per_or_n); items = per_or_n / 4; break;
    case NUNET_LOSS_ENTRY_BCE_LOGITS_FWD:
    case NUNET_LOSS_ENTRY_BCE_LOGITS_BWD: gx = bce_logits_gx(per_or_n); break;
    default: NUNET_REQUIRE(false, "loss launch info: entry %d", (int)entry);
  }
  fill_launch_info(out, gx, gy, gz, items);
  return NUNET_OK;
}
