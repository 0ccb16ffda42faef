// pipeline.h — the device-side sample pipeline (input pipeline): ONE kernel template over a source and a sink.
//   source: how the uint8 bytes of destination pixel (n, y, x) are found - a dense NHWC batch (DenseSrc), the resize of a ragged
//           source (ResizeSrc), a border-reflected tile window (TileSrc); the colour op, where there is one, is part of the source;
//   sink:   where the pixel goes - uint8 NHWC (BytesSink), normalised fp32 NCHW planes (PlanesSink), the plan's padded
//           32-channel image in the storage type (StageSink).
// The entries of include/nunet.h are wrappers that fill one source and one sink and call launch_pipeline: the six stand-alone
// ones in pipeline.hip, the four nunet_plan_stage_u8* in plan.hip. Every combination shares the fetch, the normalise expression,
// the store loop and the grid rule below, so two entries that should agree bit for bit run the same code.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------
// Colour augmentation of the sample pipeline: OneOf([HueSaturationValue(), RandomBrightness(), RandomContrast()], p=1) of the
// reference's train transform (trains.py:260-264), one op per sample from a nunet_color_aug in device memory. The arithmetic
// is this project's definition (input pipeline), modelled on albumentations' uint8 paths and OpenCV's 8-bit
// RGB2HSV / HSV2RGB with hue range 180: integer forward conversion through two division tables, the shifts in double (exact:
// a small integer plus an fp32 value), the inverse in fp32 with every operation rounded on its own. One uint8 RGB pixel in,
// one out, no dependence on position - so it commutes with rot90 / flips and a source applies it to the pixel it has just fetched.
// ---------------------------------------------------------------------------
// sdiv[i] = rint((255 << 12) / (double)i), hdiv[i] = rint((180 << 12) / (6.0 * i)), both 0 at i = 0. Neither quotient has a
// fraction of one half (that needs 2^13 | i resp. 2^14 | i), so rounding the integer quotient to nearest gives the same values.
struct ColorDivTables {
  int32_t sdiv[256], hdiv[256];
  constexpr ColorDivTables() : sdiv{}, hdiv{} {
    for (int i = 1; i < 256; ++i) {
      sdiv[i] = (2 * (255 << 12) + i) / (2 * i);
      hdiv[i] = (2 * (180 << 12) + 6 * i) / (12 * i);
    }
  }
};
static __constant__ const ColorDivTables g_color_div = ColorDivTables();

__device__ __forceinline__ uint8_t color_byte_rn(float x) {   // clamp(rint(x * 255), 0, 255), ties to even
  return (uint8_t)fminf(fmaxf(rintf(__fmul_rn(x, 255.f)), 0.f), 255.f);
}
__device__ __forceinline__ void color_aug_pixel(int op, float p0, float p1, float p2, uint8_t& r8, uint8_t& g8, uint8_t& b8) {
#pragma clang fp contract(off)
  if (op == NUNET_COLOR_BRIGHTNESS || op == NUNET_COLOR_CONTRAST) {
    // albumentations brightness_contrast_adjust, uint8 LUT, beta_by_max: p0 = beta * 255 (BRIGHTNESS) or alpha (CONTRAST)
    const float alpha = op == NUNET_COLOR_CONTRAST ? p0 : 1.f, b255 = op == NUNET_COLOR_BRIGHTNESS ? p0 : 0.f;
    float f[3] = {(float)r8, (float)g8, (float)b8};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (alpha != 1.f) f[c] = f[c] * alpha;
      if (b255 != 0.f) f[c] = f[c] + b255;
      f[c] = fminf(fmaxf(f[c], 0.f), 255.f);
    }
    r8 = (uint8_t)f[0]; g8 = (uint8_t)f[1]; b8 = (uint8_t)f[2];
  } else if (op == NUNET_COLOR_HSV) {
    const int r = r8, g = g8, b = b8;
    const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), diff = v - vmin;
    const int s = (diff * g_color_div.sdiv[v] + 2048) >> 12;
    const int hn = v == r ? g - b : v == g ? b - r + 2 * diff : r - g + 4 * diff;
    int h = (hn * g_color_div.hdiv[diff] + 2048) >> 12;
    if (h < 0) h += 180;
    // the shifts (albumentations' hue / saturation / value LUTs), in double
    const double xh = (double)h + (double)p0;
    const int h2 = (int)(xh < 0.0 ? xh + 180.0 : xh >= 180.0 ? xh - 180.0 : xh);
    const int s2 = (int)fmin(fmax((double)s + (double)p1, 0.0), 255.0);
    const int v2 = (int)fmin(fmax((double)v + (double)p2, 0.0), 255.0);
    // HSV -> RGB in fp32
    float H = (float)h2 * (6.f / 180.f);
    if (H >= 6.f) H = H - 6.f;
    const float S = (float)s2 * (1.f / 255.f), V = (float)v2 * (1.f / 255.f);
    const float secf = floorf(H);
    const bool in6 = secf >= 0.f && secf <= 5.f;          // a sector outside 0..5 (shifts beyond +-180): sector 0, fraction 0
    const int sec = in6 ? (int)secf : 0;
    const float fr = in6 ? H - secf : 0.f;
    const float p = V * (1.f - S);
    const float q = V * (1.f - S * fr);
    const float t = V * (1.f - S * (1.f - fr));
    const float R = sec == 0 || sec == 5 ? V : sec == 1 ? q : sec == 4 ? t : p;
    const float G = sec == 1 || sec == 2 ? V : sec == 0 ? t : sec == 3 ? q : p;
    const float B = sec == 3 || sec == 4 ? V : sec == 2 ? t : sec == 5 ? q : p;
    r8 = color_byte_rn(R); g8 = color_byte_rn(G); b8 = color_byte_rn(B);
  }
}
// the colour op of sample n on one pixel (color != NULL)
__device__ __forceinline__ void color_aug_sample(const nunet_color_aug* __restrict__ color, int n, uint8_t& r, uint8_t& g, uint8_t& b) {
  const nunet_color_aug c = color[n];
  color_aug_pixel(c.op, c.p0, c.p1, c.p2, r, g, b);
}

// ---------------------------------------------------------------------------
// Geometric augmentation, destination-driven: pixel (y, x) of the augmented view <- source pixel (ry, rx) of a [Hs][Ws]
// image: undo the flips, then the rotation. aug = rot90 count (bits 0-1, counter-clockwise like np.rot90) | hflip (bit 2) |
// vflip (bit 3). The view is [Hs][Ws] after an even rot90 count and [Ws][Hs] after an odd one. DenseSrc and ResizeSrc map
// through this one function.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void aug_source_pixel(int a, int Hs, int Ws, int y, int x, int& ry, int& rx) {
  const int k = a & 3;
  const int Hv = (k & 1) ? Ws : Hs, Wv = (k & 1) ? Hs : Ws;
  int sy = y, sx = x;
  if (a & 8) sy = Hv - 1 - sy;
  if (a & 4) sx = Wv - 1 - sx;
  ry = sy; rx = sx;
  if (k == 1) { ry = sx; rx = Ws - 1 - sy; }
  else if (k == 2) { ry = Hs - 1 - sy; rx = Ws - 1 - sx; }
  else if (k == 3) { ry = Hs - 1 - sx; rx = sy; }
}

// ---------------------------------------------------------------------------
// Resize(input_h, input_w) of the reference's transforms (trains.py:265, 269) on ragged uint8 sources: sample n is a tight
// HWC image at pool + samples[n].offset (nunet_u8_sample, device memory). The arithmetic is this project's definition
// (input pipeline), modelled on OpenCV's 8-bit INTER_LINEAR (two passes, 11-bit coefficients) and INTER_NEAREST,
// stated in integers. The reference augments the source and then resizes, so a destination pixel takes its taps in the
// AUGMENTED view, each tap goes back through aug_source_pixel to the source bytes, and the colour op applies to each fetched
// tap (ResizeSrc).
// ---------------------------------------------------------------------------
// One axis, source extent S -> destination extent D, destination index d: taps s0, s1 and the weight a1 of s1 (a0 = 2048 - a1)
__device__ __forceinline__ void resize_axis_taps(int S, int D, int d, int& s0, int& s1, int& a1) {
  const long long num = (2ll * d + 1) * S - D, den = 2ll * D;
  long long s = 0, a = 0;
  if (num >= 0) {
    s = num / den;
    if (s >= S - 1) s = S - 1;
    else a = ((num % den) * 4096 + den) / (2 * den);
  }
  s0 = (int)s; a1 = (int)a;
  s1 = min(s0 + 1, S - 1);
}
struct ResizeTaps {
  long long o[2][2];    // byte offsets into the pool of the source pixels behind the taps (y0|y1, x0|x1); o[0][0] < 0: bad descriptor
  int ax1, ay1;         // weights of the second tap along x and y, 0 .. 2048
};
// a descriptor a thread may read through: inside the pool, extents 1 .. NUNET_RESIZE_MAX_EXTENT
__device__ __forceinline__ bool resize_sample_ok(const nunet_u8_sample& d, int C, long long pool_bytes) {
  return d.H >= 1 && d.W >= 1 && d.H <= NUNET_RESIZE_MAX_EXTENT && d.W <= NUNET_RESIZE_MAX_EXTENT && d.offset >= 0 &&
         d.offset <= pool_bytes && (long long)d.H * d.W * C <= pool_bytes - d.offset;
}
template <bool NEAREST>
__device__ __forceinline__ ResizeTaps resize_taps(const nunet_u8_sample& d, int C, long long pool_bytes, int a, int Hd, int Wd, int y, int x) {
  ResizeTaps t;
  t.ax1 = t.ay1 = 0;
  if (!resize_sample_ok(d, C, pool_bytes)) { t.o[0][0] = t.o[0][1] = t.o[1][0] = t.o[1][1] = -1; return t; }
  const int Hv = (a & 1) ? d.W : d.H, Wv = (a & 1) ? d.H : d.W;
  int vy[2], vx[2];
  if constexpr (NEAREST) {
    vy[0] = vy[1] = (int)min((long long)y * Hv / Hd, (long long)Hv - 1);
    vx[0] = vx[1] = (int)min((long long)x * Wv / Wd, (long long)Wv - 1);
  } else {
    resize_axis_taps(Hv, Hd, y, vy[0], vy[1], t.ay1);
    resize_axis_taps(Wv, Wd, x, vx[0], vx[1], t.ax1);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int ry, rx;
      aug_source_pixel(a, d.H, d.W, vy[j], vx[i], ry, rx);
      t.o[j][i] = d.offset + ((long long)ry * d.W + rx) * C;
    }
  return t;
}
// the two passes on one channel's four bytes
__device__ __forceinline__ uint8_t resize_lerp(int p00, int p01, int p10, int p11, int ax1, int ay1) {
  const int r0 = (p00 * (2048 - ax1) + p01 * ax1) >> 4, r1 = (p10 * (2048 - ax1) + p11 * ax1) >> 4;
  return (uint8_t)(((((2048 - ay1) * r0) >> 16) + ((ay1 * r1) >> 16) + 2) >> 2);
}
// channel c of the destination pixel behind t (no colour op); a bad descriptor gives 0 without a read
template <bool NEAREST>
__device__ __forceinline__ uint8_t resize_channel(const uint8_t* __restrict__ pool, const ResizeTaps& t, int c) {
  if (t.o[0][0] < 0) return 0;
  if constexpr (NEAREST) return pool[t.o[0][0] + c];
  else return resize_lerp(pool[t.o[0][0] + c], pool[t.o[0][1] + c], pool[t.o[1][0] + c], pool[t.o[1][1] + c], t.ax1, t.ay1);
}
// the RGB destination pixel behind t, the colour op of `col` on every fetched tap first (bilinear only)
__device__ __forceinline__ void resize_rgb_color(const uint8_t* __restrict__ pool, const ResizeTaps& t, const nunet_color_aug& col, uint8_t px[3]) {
  px[0] = px[1] = px[2] = 0;
  if (t.o[0][0] < 0) return;
  uint8_t p[2][2][3];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      p[j][i][0] = p[j][i][1] = p[j][i][2] = 0;
      if ((i && t.ax1 == 0) || (j && t.ay1 == 0)) continue;      // a tap of weight 0 (every second tap of an equal-size source): no fetch, no colour op
      const uint8_t* s = pool + t.o[j][i];
      p[j][i][0] = s[0]; p[j][i][1] = s[1]; p[j][i][2] = s[2];
      color_aug_pixel(col.op, col.p0, col.p1, col.p2, p[j][i][0], p[j][i][1], p[j][i][2]);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = resize_lerp(p[0][0][c], p[0][1][c], p[1][0][c], p[1][1][c], t.ax1, t.ay1);
}

// ---------------------------------------------------------------------------
// Tiled inference (include/nunet.h, nunet_tile): pixel (y, x) of tile t <- a byte offset into the pool, or -1 for a pixel that
// reads nothing (null tile, bad sample index, bad descriptor, origin outside the source). TileSrc is its one caller.
// ---------------------------------------------------------------------------
// BORDER_REFLECT_101, repeated, of index i >= 0 into an axis of extent S >= 1 (np.pad(mode='reflect'))
__device__ __forceinline__ int reflect101(int i, int S) {
  if (S == 1) return 0;
  const int p = 2 * (S - 1), m = i % p;
  return m < S ? m : p - m;
}
__device__ __forceinline__ long long tile_pixel_offset(const nunet_u8_sample* __restrict__ samples, int n_samples, const nunet_tile& t, int C,
                                                       long long pool_bytes, int y, int x) {
  if (t.sample < 0 || t.sample >= n_samples) return -1;
  const nunet_u8_sample d = samples[t.sample];
  if (!resize_sample_ok(d, C, pool_bytes)) return -1;
  if (t.y0 < 0 || t.y0 >= d.H || t.x0 < 0 || t.x0 >= d.W) return -1;
  int sy = t.y0 + y, sx = t.x0 + x;              // (y < Th, x < Tw <= NUNET_RESIZE_MAX_EXTENT: no overflow)
  if (sy >= d.H) sy = reflect101(sy, d.H);
  if (sx >= d.W) sx = reflect101(sx, d.W);
  return d.offset + ((long long)sy * d.W + sx) * C;
}

// ---------------------------------------------------------------------------
// Sources: at(n, y, x) returns a handle of destination pixel (y, x) of sample n whose byte(c) is channel c's uint8. A source
// is a kernel argument passed by value. No member pointer is __restrict__: nunet_color_aug_u8 may run in place - its thread
// reads its three bytes (at) before it writes them (the sink), and with no geometric code the source pixel is the destination
// pixel - so DenseSrc::u and BytesSink::out may be the same buffer.
// ---------------------------------------------------------------------------
struct PxMem {          // bytes that sit in memory as they are; s == NULL: a pixel that reads nothing, all zeros
  const uint8_t* s;
  __device__ __forceinline__ uint8_t byte(int c) const { return s ? s[c] : (uint8_t)0; }
};
struct PxRgb {          // three bytes formed at fetch time (the colour sources: C == 3)
  uint8_t v[3];
  __device__ __forceinline__ uint8_t byte(int c) const {
    __builtin_assume(c < 3);      // (a sink's unrolled channel loop ends at 3 instead of carrying mean / stdv of all 32 channels)
    return c == 0 ? v[0] : c == 1 ? v[1] : v[2];
  }
};
template <bool NEAREST> struct PxTaps {      // the taps of a resize, interpolated per channel
  const uint8_t* pool; ResizeTaps t;
  __device__ __forceinline__ uint8_t byte(int c) const { return resize_channel<NEAREST>(pool, t, c); }
};

// a dense [N][H][W][C] batch under the sample's geometric code (H == W when the rot90 count is odd); COLOR: the colour op of
// color[n] on the fetched pixel, C == 3
template <bool COLOR> struct DenseSrc {
  const uint8_t* u; int H, W, C; const int32_t* aug; const nunet_color_aug* color;
  __device__ __forceinline__ auto at(int n, int y, int x) const {
    int ry, rx;
    aug_source_pixel(aug ? aug[n] : 0, H, W, y, x, ry, rx);
    const uint8_t* s = u + (((long long)n * H + ry) * W + rx) * C;
    if constexpr (COLOR) {
      PxRgb p = {{s[0], s[1], s[2]}};
      color_aug_sample(color, n, p.v[0], p.v[1], p.v[2]);
      return p;
    } else {
      return PxMem{s};
    }
  }
};
// ragged sources resized to Hd x Wd: the taps are formed once per pixel; COLOR (bilinear, C == 3): the colour op on every tap
template <bool NEAREST, bool COLOR> struct ResizeSrc {
  const uint8_t* pool; long long pool_bytes; const nunet_u8_sample* samples; int C, Hd, Wd; const int32_t* aug; const nunet_color_aug* color;
  __device__ __forceinline__ auto at(int n, int y, int x) const {
    const ResizeTaps t = resize_taps<NEAREST>(samples[n], C, pool_bytes, aug ? aug[n] : 0, Hd, Wd, y, x);
    if constexpr (COLOR) {
      PxRgb p;
      resize_rgb_color(pool, t, color[n], p.v);
      return p;
    } else {
      return PxTaps<NEAREST>{pool, t};
    }
  }
};
// border-reflected windows of ragged sources: sample n of the launch is tile tiles[n]
struct TileSrc {
  const uint8_t* pool; long long pool_bytes; const nunet_u8_sample* samples; int n_samples; const nunet_tile* tiles; int C;
  __device__ __forceinline__ PxMem at(int n, int y, int x) const {
    const long long o = tile_pixel_offset(samples, n_samples, tiles[n], C, pool_bytes, y, x);
    return PxMem{o < 0 ? nullptr : pool + o};
  }
};

// ---------------------------------------------------------------------------
// Sinks: put(handle, i, n, y, x) stores destination pixel i = (n * H + y) * W + x.
// ---------------------------------------------------------------------------
// albumentations Normalize() (reference trains.py:266) and the extra /255 (dataset.py:71) on one byte
__device__ __forceinline__ float normalize_byte(uint8_t b, float m, float sd, float post_scale) {
  return (((float)b / 255.f - m) / sd) * post_scale;
}
struct BytesSink {       // uint8 NHWC
  uint8_t* out; int C;
  template <class Px> __device__ __forceinline__ void put(const Px& p, long long i, int, int, int) const {
    for (int c = 0; c < C; ++c) out[i * C + c] = p.byte(c);
  }
};
struct PlanesSink {      // normalised fp32 NCHW (HWC -> CHW of dataset.py:72); mean / stdv NULL: 0 / 1
  float* out; int C, H, W; const float* mean; const float* stdv; float post_scale;
  template <class Px> __device__ __forceinline__ void put(const Px& p, long long, int n, int y, int x) const {
    const long long hw = (long long)H * W, o = (long long)y * W + x;
    for (int c = 0; c < C; ++c) out[((long long)n * C + c) * hw + o] = normalize_byte(p.byte(c), mean ? mean[c] : 0.f, stdv ? stdv[c] : 1.f, post_scale);
  }
};
// The plan's image: the padded NHWC pixel the first conv reads, 32 channels in the storage type (zeros beyond C) as 16-byte
// stores. PlanesSink's value followed by nunet_nchw_to_nhwc's rounding, so a staged image is bit-identical to the float path's.
template <typename T> struct StageSink {
  T* img; int C; const float* mean; const float* stdv; float post_scale;
  template <class Px> __device__ __forceinline__ void put(const Px& p, long long i, int, int, int) const {
    constexpr int EPV = Tr<T>::EPV;
    T* dst = img + i * 32;
#pragma unroll
    for (int v = 0; v < 32 / EPV; ++v) {
      Vec16<T> o;
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int c = v * EPV + e;
        o.set(e, c < C ? normalize_byte(p.byte(c), mean ? mean[c] : 0.f, stdv ? stdv[c] : 1.f, post_scale) : 0.f);
      }
      st16(dst + v * EPV, o);
    }
  }
};

// One thread per destination pixel of an [N][H][W] launch, grid-stride.
template <class Src, class Sink>
__global__ __launch_bounds__(256) void pipeline_kernel(Src src, Sink sink, long long npix, int H, int W) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const long long q = i / W;
    const int y = (int)(q % H);
    const int n = (int)(q / H);
    sink.put(src.at(n, y, x), i, n, y, x);
  }
}
// The one grid rule: a workgroup per 256 pixels, at most 4096 workgroups (a launch of more pixels takes further trips).
template <class Src, class Sink>
static int launch_pipeline(const char* name, const Src& src, const Sink& sink, int N, int H, int W, double bytes, hipStream_t st) {
  const long long npix = (long long)N * H * W;
  ProfScope ps(PC_LAYOUT, 0, bytes, st);
  NUNET_LAUNCH((pipeline_kernel<Src, Sink>), dim3(grid_for(npix, 256, 4096)), dim3(256), 0, st, src, sink, npix, H, W);
  return nunet_check_launch(name);
}
// What every entry asks of its arguments: non-null pointers (`ptrs`: the entry's own conjunction), a positive sample and channel
// count and a destination of H x W. dest == NULL: a dense source, any positive extents. Otherwise a pooled source (ragged
// samples, tiles): `dest` names the destination in the message, its extents are 1 .. NUNET_RESIZE_MAX_EXTENT and the pool is
// not empty.
static inline int pipeline_args_ok(const char* what, bool ptrs, int N, int C, int H, int W, const char* dest = nullptr, long long pool_bytes = 1) {
  NUNET_REQUIRE(ptrs, "%s: null pointer", what);
  NUNET_REQUIRE(N > 0 && C > 0 && pool_bytes > 0 && (dest || (H > 0 && W > 0)), "%s: N=%d C=%d H=%d W=%d pool_bytes=%lld must be positive", what, N, C, H, W, pool_bytes);
  NUNET_REQUIRE(!dest || (H >= 1 && W >= 1 && H <= NUNET_RESIZE_MAX_EXTENT && W <= NUNET_RESIZE_MAX_EXTENT), "%s: %s %d x %d: extents are 1 .. %d", what, dest, H, W,
                NUNET_RESIZE_MAX_EXTENT);
  return NUNET_OK;
}
