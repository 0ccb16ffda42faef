// weights.hip — everything that walks the plan's PackTab / UnpackTab (plan.h): fp32 OIHW parameters -> the packed 16-bit
// layouts, native-layout gradient scratch -> flat OIHW gradients, the fused optimiser step, the scratch's square norm, and
// the sum of the weight gradients' K-split slabs. The passes (plan.hip) reach it through plan_pack_weights,
// plan_unpack_grads and launch_reduce.
#include "plan.h"

// ---------------------------------------------------------------------------------------------------------
// The walk every weight-layout kernel below shares. One block per (layer, 32 Cout x 32 Cin tile); PackTab carries a
// prefix sum of tiles per entry for the block -> tile map. A tile lives in LDS as s[co_local][ci_local * 9 + tap]:
// its OIHW rows (parameters, flat gradients) are contiguous runs of 32 * 9 floats, the native gradient scratch
// [tap][co][cinpad] and both packed layouts are contiguous along ci (wf) or co (wd). The unpack kernels' blocks past
// the last tile own one UnpackTab entry each (tail_entry).
// ---------------------------------------------------------------------------------------------------------
constexpr int TILE_LD = 32 * 9 + 1;
struct Tile { int e, co0, ci0, cw, rw; };   // table entry, tile origin; cw / rw: real input channels / output rows in the tile (cw <= 0: pure padding)

__device__ __forceinline__ Tile tile_of(const PackTab& tab, int bid) {
  Tile t;
  t.e = 0;
  while (t.e + 1 < tab.n && bid >= tab.tile0[t.e + 1]) ++t.e;
  const int i = bid - tab.tile0[t.e];
  const int cout = tab.e[t.e].cout, cin = tab.e[t.e].cin, nci = (tab.e[t.e].cinpad + 31) / 32;
  t.co0 = (i / nci) * 32; t.ci0 = (i % nci) * 32;
  t.cw = min(32, cin - t.ci0); t.rw = min(32, cout - t.co0);
  return t;
}

// 1x1 head: [nslab][tot] partial slabs (already OIHW order, tot <= 8 classes * 33 = 264), summed by one block of B = 256 threads in a
// fixed order: B / ne threads share an element's slabs (a single thread walking all 256 slabs is a chain of 256
// dependent-latency loads: that loop alone made the earlier fused kernels 100 us long), thread (part, e) adds slabs part,
// part + parts, ... in order, the parts meet in LDS (B floats) and are added in order q = 0 .. parts - 1. The owning thread
// calls f(element, sum). The order depends on B, so every caller is a 256-thread block.
template <typename F>
__device__ __forceinline__ void head_slab_sum(const float* __restrict__ dw, int tot, int nslab, float* lds, F f) {
  constexpr int B = 256;
  for (int e0 = 0; e0 < tot; e0 += B) {
    const int ne = min(B, tot - e0);
    const int parts = B / ne;                     // threads per element
    const int e = threadIdx.x % ne, part = threadIdx.x / ne;
    float v = 0.f;
    if (part < parts) {
#pragma unroll 8
      for (int sl = part; sl < nslab; sl += parts) v += dw[(long long)sl * tot + e0 + e];
    }
    lds[threadIdx.x] = part < parts ? v : 0.f;
    __syncthreads();
    if ((int)threadIdx.x < ne) {
      float t = 0.f;
      for (int q = 0; q < parts; ++q) t += lds[q * ne + threadIdx.x];
      f(e0 + (int)threadIdx.x, t);
    }
    __syncthreads();
  }
}

// A 256-thread block past the last tile: the slab sum of a 1x1 head, or a conv layer's bias / BatchNorm vectors (they follow the
// weights in the scratch entry and in the flat arenas). f(index relative to the entry's dst, value).
template <typename F>
__device__ __forceinline__ void tail_entry(const UnpackEnt& en, const float* __restrict__ scratch, float* lds, F f) {
  const float* dw = scratch + en.src;
  const int nw = en.cout * en.cin * en.taps;
  if (en.nslab > 1) {
    head_slab_sum(dw, nw + en.nvec * en.cout, en.nslab, lds, f);
    return;
  }
  const float* vsrc = dw + (long long)en.taps * en.cout * en.cinpad;
  for (int i = threadIdx.x; i < en.nvec * en.cout; i += blockDim.x) f(nw + i, vsrc[i]);
}

// scratch dw[tap][co][cinpad] -> LDS tile: 16-byte loads along ci for a full tile (an element-wise gather touches nine
// 128-byte lines per wave load); a ragged tile element-wise, entries outside rw x cw left unwritten
__device__ __forceinline__ void gather_scratch_tile(float (*s)[TILE_LD], const float* __restrict__ dw, const PackEnt& en, const Tile& t) {
  if (t.rw == 32 && t.cw == 32 && en.cinpad % 4 == 0 && ((uintptr_t)dw & 15) == 0) {
    for (int i = threadIdx.x; i < 9 * 32 * 8; i += blockDim.x) {
      const int c4 = i & 7, ro = (i >> 3) & 31, tap = i >> 8;
      const f32x4 v = *reinterpret_cast<const f32x4*>(dw + ((long long)tap * en.cout + t.co0 + ro) * en.cinpad + t.ci0 + c4 * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[ro][(c4 * 4 + j) * 9 + tap] = v[j];
    }
  } else {
    for (int i = threadIdx.x; i < 9 * 32 * 32; i += blockDim.x) {
      const int ci = i & 31, ro = (i >> 5) & 31, tap = i >> 10;
      if (ro < t.rw && ci < t.cw) s[ro][ci * 9 + tap] = dw[((long long)tap * en.cout + t.co0 + ro) * en.cinpad + t.ci0 + ci];
    }
  }
}

// OIHW rows w[co][cin][9] -> LDS tile: 16-byte loads for a full tile; a ragged one (the first layer's) element-wise, zero
// outside rw x cw (the ci >= cin columns are written to wf as zeros)
__device__ __forceinline__ void load_oihw_tile(float (*s)[TILE_LD], const float* __restrict__ w, const PackEnt& en, const Tile& t) {
  const float* wrow = w + ((long long)t.co0 * en.cin + t.ci0) * 9;
  if (t.rw == 32 && t.cw == 32 && en.cin % 4 == 0 && ((uintptr_t)wrow & 15) == 0) {
    for (int i = threadIdx.x; i < 32 * 72; i += blockDim.x) {
      const int ro = i / 72, k4 = i - ro * 72;
      const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + (long long)ro * en.cin * 9 + k4 * 4);
      float* d = &s[ro][k4 * 4];
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  } else {
    for (int i = threadIdx.x; i < 32 * 288; i += blockDim.x) {
      const int ro = i / 288, k = i - ro * 288;      // k = ci_local*9 + tap
      float v = 0.f;
      if (ro < t.rw && k < t.cw * 9) v = wrow[(long long)ro * en.cin * 9 + k];
      s[ro][k] = v;
    }
  }
}

// LDS tile -> both packed layouts of T, wf[tap][co][cinpad] and (en.wd >= 0) the flipped / transposed wd[8 - tap][ci][co]:
// 16-byte stores (8 packed elements per thread) where rows and alignment allow, element-wise otherwise
template <typename T>
__device__ __forceinline__ void store_packed_tile(const float (*s)[TILE_LD], T* __restrict__ arena, const PackEnt& en, const Tile& t) {
  constexpr int EPV = Tr<T>::EPV;
  T* wf = arena + en.wf;
  T* wd = en.wd >= 0 ? arena + en.wd : nullptr;
  if (t.rw == 32 && en.cinpad % 8 == 0 && en.cout % 8 == 0 && ((uintptr_t)wf & 15) == 0 && ((uintptr_t)wd & 15) == 0) {
    for (int i = threadIdx.x; i < 9 * 32 * 4; i += blockDim.x) {    // wf[tap][co][ci], ci fastest: 8 ci per thread
      const int g = i & 3, ro = (i >> 2) & 31, tap = i >> 7;
      if (t.ci0 + g * 8 < en.cinpad) {
        T* q = wf + ((long long)tap * en.cout + t.co0 + ro) * en.cinpad + t.ci0 + g * 8;
#pragma unroll
        for (int h = 0; h < 8 / EPV; ++h) {
          Vec16<T> o;
#pragma unroll
          for (int e = 0; e < EPV; ++e) o.set(e, s[ro][(g * 8 + h * EPV + e) * 9 + tap]);
          st16(q + h * EPV, o);
        }
      }
    }
    if (wd) {
      for (int i = threadIdx.x; i < 9 * 32 * 4; i += blockDim.x) {  // wd[8-tap][ci][co], co fastest: 8 co per thread
        const int g = i & 3, ci = (i >> 2) & 31, tap = i >> 7;
        if (ci < t.cw) {
          T* q = wd + ((long long)(8 - tap) * en.cin + t.ci0 + ci) * en.cout + t.co0 + g * 8;
#pragma unroll
          for (int h = 0; h < 8 / EPV; ++h) {
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < EPV; ++e) o.set(e, s[g * 8 + h * EPV + e][ci * 9 + tap]);
            st16(q + h * EPV, o);
          }
        }
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < 9 * 32 * 32; i += blockDim.x) {   // wf[tap][co][ci], ci fastest
    const int ci = i & 31, ro = (i >> 5) & 31, tap = i >> 10;
    if (ro < t.rw && t.ci0 + ci < en.cinpad)
      wf[((long long)tap * en.cout + t.co0 + ro) * en.cinpad + t.ci0 + ci] = from_f32<T>(s[ro][ci * 9 + tap]);
  }
  if (wd) {
    for (int i = threadIdx.x; i < 9 * 32 * 32; i += blockDim.x) { // wd[8-tap][ci][co], co fastest
      const int ro = i & 31, ci = (i >> 5) & 31, tap = i >> 10;
      if (ro < t.rw && ci < t.cw)
        wd[((long long)(8 - tap) * en.cin + t.ci0 + ci) * en.cout + t.co0 + ro] = from_f32<T>(s[ro][ci * 9 + tap]);
    }
  }
}

// fp32 parameters -> both packed layouts
template <typename T>
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ params, T* __restrict__ arena, PackTab tab) {
  __shared__ float s_t[32][TILE_LD];
  const Tile t = tile_of(tab, blockIdx.x);
  const PackEnt en = tab.e[t.e];
  load_oihw_tile(s_t, params + en.src, en, t);
  __syncthreads();
  store_packed_tile(s_t, arena, en, t);
}

// Gradient scratch -> flat OIHW gradient arena (overwritten or accumulated into), the OIHW rows written as 16-byte runs
__global__ __launch_bounds__(256) void unpack_tiled_kernel(const float* __restrict__ scratch, float* __restrict__ grads, PackTab tab, UnpackTab ut) {
  __shared__ float s_t[32][TILE_LD];
  if ((int)blockIdx.x >= tab.ntiles) {
    const UnpackEnt en = ut.e[(int)blockIdx.x - tab.ntiles];
    float* g = grads + en.dst;
    tail_entry(en, scratch, &s_t[0][0], [&](int i, float v) { g[i] = ut.accumulate ? g[i] + v : v; });
    return;
  }
  const Tile t = tile_of(tab, blockIdx.x);
  if (t.cw <= 0) return;                                 // pure padding tile
  const PackEnt en = tab.e[t.e];
  const UnpackEnt ue = ut.e[t.e];
  float* grow = grads + ue.dst + ((long long)t.co0 * en.cin + t.ci0) * 9;
  gather_scratch_tile(s_t, scratch + ue.src, en, t);
  __syncthreads();
  if (t.rw == 32 && t.cw == 32 && en.cin % 4 == 0 && ((uintptr_t)grow & 15) == 0) {
    for (int i = threadIdx.x; i < 32 * 72; i += blockDim.x) {
      const int ro = i / 72, k4 = i - ro * 72;
      f32x4* q = reinterpret_cast<f32x4*>(grow + (long long)ro * en.cin * 9 + k4 * 4);
      const float* sp = &s_t[ro][k4 * 4];
      f32x4 v = {sp[0], sp[1], sp[2], sp[3]};
      if (ut.accumulate) { const f32x4 o = *q; v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3]; }
      *q = v;
    }
  } else {
    for (int i = threadIdx.x; i < 32 * 288; i += blockDim.x) {
      const int ro = i / 288, k = i - ro * 288;
      if (ro < t.rw && k < t.cw * 9) {
        float* q = grow + (long long)ro * en.cin * 9 + k;
        *q = ut.accumulate ? *q + s_t[ro][k] : s_t[ro][k];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Fused optimiser step (unpack_sgd_tiled_kernel, below): native-layout gradient scratch -> optimiser step on
// the fp32 master parameters, one launch; the next forward repacks the 16-bit weight layouts. torch.optim.SGD
// semantics (reference trains.py:229-231).
// ---------------------------------------------------------------------------------------------------------
struct UpdP { float* params; const float* scratch; float* grads; float gscale; };

// one element of the fused kernels outside the LDS tiles, at flat index idx: the scaled gradient to the flat arena when the
// caller wants it, then the step unless loss scaling skipped it (live false)
template <typename O>
__device__ __forceinline__ void step_elem(const UpdP& u, const O& o, bool live, float gs, long long idx, float g) {
  g *= gs;
  if (u.grads) u.grads[idx] = g;
  if (live) u.params[idx] = opt_elem(o, u.params[idx], g, idx);
}

// Optimiser step straight from the gradient scratch: replaces nunet_plan_backward_phase bit 2 +
// nunet_opt_step; the weights are repacked by the next nunet_plan_forward as usual.
// unpack_tiled_kernel with the optimiser step as the epilogue of its store phase: the tile's gradients meet the OIHW
// parameters and the optimiser state as 16-byte runs, the flat gradient arena is written only when the caller wants it.
template <typename O>
__global__ __launch_bounds__(256) void unpack_sgd_tiled_kernel(UpdP u, O o, PackTab tab, UnpackTab ut) {
  __shared__ float s_t[32][TILE_LD];
  float gs = u.gscale;
  const bool live = o.begin(gs);   // false: a step skipped by loss scaling, which stores the unscaled gradients only
  if (!live && !u.grads) return;
  if ((int)blockIdx.x >= tab.ntiles) {
    const UnpackEnt en = ut.e[(int)blockIdx.x - tab.ntiles];
    tail_entry(en, u.scratch, &s_t[0][0], [&](int i, float g) { step_elem(u, o, live, gs, en.dst + i, g); });
    return;
  }
  const Tile t = tile_of(tab, blockIdx.x);
  if (t.cw <= 0) return;
  const PackEnt en = tab.e[t.e];
  const UnpackEnt ue = ut.e[t.e];
  const long long row0 = ue.dst + ((long long)t.co0 * en.cin + t.ci0) * 9;
  gather_scratch_tile(s_t, u.scratch + ue.src, en, t);
  __syncthreads();
  bool al = ((uintptr_t)(u.params + row0) & 15) == 0 && (!u.grads || ((uintptr_t)(u.grads + row0) & 15) == 0);
#pragma unroll
  for (int q = 0; q < O::NS; ++q) al = al && ((uintptr_t)(o.st[q] + row0) & 15) == 0;
  if (t.rw == 32 && t.cw == 32 && en.cin % 4 == 0 && al) {
    for (int i = threadIdx.x; i < 32 * 72; i += blockDim.x) {
      const int ro = i / 72, k4 = i - ro * 72;
      const long long idx = row0 + (long long)ro * en.cin * 9 + k4 * 4;
      const float* sp = &s_t[ro][k4 * 4];
      f32x4 g = {sp[0] * gs, sp[1] * gs, sp[2] * gs, sp[3] * gs};
      if (!live) {
        *reinterpret_cast<f32x4*>(u.grads + idx) = g;
        continue;
      }
      f32x4 pv = *reinterpret_cast<const f32x4*>(u.params + idx);
      f32x4 sv[O::NS];
#pragma unroll
      for (int q = 0; q < O::NS; ++q) sv[q] = *reinterpret_cast<const f32x4*>(o.st[q] + idx);
      if (u.grads) *reinterpret_cast<f32x4*>(u.grads + idx) = g;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float s[O::NS];
#pragma unroll
        for (int q = 0; q < O::NS; ++q) s[q] = sv[q][j];
        pv[j] = o.one(pv[j], g[j], s);
#pragma unroll
        for (int q = 0; q < O::NS; ++q) sv[q][j] = s[q];
      }
#pragma unroll
      for (int q = 0; q < O::NS; ++q) *reinterpret_cast<f32x4*>(o.st[q] + idx) = sv[q];
      *reinterpret_cast<f32x4*>(u.params + idx) = pv;
    }
  } else {
    for (int i = threadIdx.x; i < 32 * 288; i += blockDim.x) {
      const int ro = i / 288, k = i - ro * 288;
      if (ro < t.rw && k < t.cw * 9) step_elem(u, o, live, gs, row0 + (long long)ro * en.cin * 9 + k, s_t[ro][k]);
    }
  }
}

// Square norm of the gradient scratch for gradient clipping (include/nunet.h nunet_clip): the unpack kernels'
// block -> (layer, 32 x 32 tile | vector tail | head) map, read-only. A conv tile sums the squares of its real [tap][co][ci]
// entries (ci < cin: the padding up to cinpad does not count) straight from the scratch, 16-byte loads along ci; a tail block
// takes the layer's conv bias, gamma and beta; a head block sums the slabs first (head_slab_sum, so in unpack_sgd_tiled_kernel's order) and
// squares the sum. Products exact in double, a thread's elements in index order, then block256_sum_f64: one partial per
// workgroup, plain store (a pure-padding tile stores 0).
__global__ __launch_bounds__(256) void plan_sqnorm_kernel(const float* __restrict__ scratch, PackTab tab, UnpackTab ut, double* __restrict__ ws) {
  __shared__ float s_p[256];
  __shared__ double s_w[4];
  double acc = 0.0;
  if ((int)blockIdx.x >= tab.ntiles) {
    tail_entry(ut.e[(int)blockIdx.x - tab.ntiles], scratch, s_p, [&](int, float g) { acc += (double)g * (double)g; });
  } else {
    const Tile t = tile_of(tab, blockIdx.x);
    const PackEnt en = tab.e[t.e];
    const float* dw = scratch + ut.e[t.e].src;
    if (t.cw > 0 && en.cinpad % 4 == 0 && ((uintptr_t)dw & 15) == 0) {
      for (int i = threadIdx.x; i < 9 * 32 * 8; i += blockDim.x) {
        const int c4 = i & 7, ro = (i >> 3) & 31, tap = i >> 8;
        if (ro >= t.rw || c4 * 4 >= t.cw) continue;      // (t.ci0 + c4 * 4 < cin <= cinpad, a multiple of 4: the run is inside the row)
        const f32x4 v = *reinterpret_cast<const f32x4*>(dw + ((long long)tap * en.cout + t.co0 + ro) * en.cinpad + t.ci0 + c4 * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c4 * 4 + j < t.cw) acc += (double)v[j] * (double)v[j];
      }
    } else if (t.cw > 0) {
      for (int i = threadIdx.x; i < 9 * 32 * 32; i += blockDim.x) {
        const int ci = i & 31, ro = (i >> 5) & 31, tap = i >> 10;
        if (ro < t.rw && ci < t.cw) {
          const float v = dw[((long long)tap * en.cout + t.co0 + ro) * en.cinpad + t.ci0 + ci];
          acc += (double)v * (double)v;
        }
      }
    }
  }
  const double tot = block256_sum_f64(acc, s_w);
  if (threadIdx.x == 0) ws[blockIdx.x] = tot;
}

// Sum of the weight gradients' K-split slabs into the native-layout gradient scratch, all layers of a phase in one
// launch. A block owns 64 float4 outputs of one layer; thread (part, e) adds slabs part, part + 4, ... in order, the
// four parts meet in LDS in order: a fixed summation tree, so the gradient is bit-identical from run to run.
#define MAXRED 40
struct RedEnt { long long slab, dst, stride, n4; int ks, blk0; };
struct RedTab { int n, nblocks; RedEnt e[MAXRED]; };
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ slabs, float* __restrict__ gs, RedTab tab) {
  __shared__ f32x4 s_p[4][64];
  int e = 0;
  while (e + 1 < tab.n && (int)blockIdx.x >= tab.e[e + 1].blk0) ++e;
  const RedEnt en = tab.e[e];
  const int part = threadIdx.x >> 6, el = threadIdx.x & 63;
  const long long i = ((long long)blockIdx.x - en.blk0) * 64 + el;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (i < en.n4) {
    const float* q = slabs + en.slab + i * 4;
#pragma unroll 4
    for (int sl = part; sl < en.ks; sl += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(q + (size_t)sl * en.stride);
      a[0] += v[0]; a[1] += v[1]; a[2] += v[2]; a[3] += v[3];
    }
  }
  s_p[part][el] = a;
  __syncthreads();
  if (part == 0 && i < en.n4) {
    f32x4 r = s_p[0][el];
#pragma unroll
    for (int q = 1; q < 4; ++q) { const f32x4 v = s_p[q][el]; r[0] += v[0]; r[1] += v[1]; r[2] += v[2]; r[3] += v[3]; }
    *reinterpret_cast<f32x4*>(gs + en.dst + i * 4) = r;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Host side: the launches and the entries
// ---------------------------------------------------------------------------------------------------------
// block -> tile prefix table of a PackTab: entry i owns blocks [tile0[i], tile0[i + 1]) of the tile kernels, one per 32 x 32
// (cout, cinpad) tile. Filled once, when the table is built.
void pack_tiles(PackTab& tab) {
  int nt = 0;
  for (int i = 0; i < tab.n; ++i) { tab.tile0[i] = nt; nt += ((tab.e[i].cout + 31) / 32) * ((tab.e[i].cinpad + 31) / 32); }
  tab.tile0[tab.n] = nt; tab.ntiles = nt;
}

template <typename T> static int launch_pack(const float* params, void* arena_t, const PackTab& tab, hipStream_t st) {
  double pb = 0;
  for (int i = 0; i < tab.n; ++i) pb += 9.0 * tab.e[i].cout * tab.e[i].cin * (4 + (tab.e[i].wd >= 0 ? 2 : 1) * sizeof(T));
  ProfScope ps(PC_PACK, 0, pb, st);
  NUNET_LAUNCH((pack_kernel<T>), dim3(tab.ntiles), dim3(256), 0, st, params, (T*)arena_t, tab);
  return nunet_check_launch("pack_weights");
}

extern "C" int nunet_pack_weights(const float* w, int32_t cout, int32_t cin, int32_t cin_pad, int32_t dtype, void* wf, void* wd, nunet_stream_t s) {
  NUNET_REQUIRE(w && wf && cout > 0 && cin > 0 && cin_pad >= cin, "pack_weights: bad args");
  NUNET_REQUIRE(dtype >= 0 && dtype <= 2, "pack_weights: bad dtype");
  PackTab tab; memset(&tab, 0, sizeof(tab));
  tab.n = 1;
  const int es = dtype_size(dtype);
  char* base = (wd && (char*)wd < (char*)wf) ? (char*)wd : (char*)wf;
  NUNET_REQUIRE(((char*)wf - base) % es == 0 && (!wd || ((char*)wd - base) % es == 0), "pack_weights: wf/wd misaligned");
  tab.e[0].src = 0;
  tab.e[0].wf = ((char*)wf - base) / es;
  tab.e[0].wd = wd ? ((char*)wd - base) / es : -1;
  tab.e[0].cout = cout; tab.e[0].cin = cin; tab.e[0].cinpad = cin_pad;
  pack_tiles(tab);
  return NUNET_DISPATCH(dtype, launch_pack, w, (void*)base, tab, (hipStream_t)s);
}

extern "C" int nunet_unpack_wgrad(const float* dw, int32_t cout, int32_t cin, int32_t cin_pad, float* g, int32_t accumulate, nunet_stream_t s) {
  NUNET_REQUIRE(dw && g && cout > 0 && cin > 0 && cin_pad >= cin, "unpack_wgrad: bad args");
  PackTab tab; memset(&tab, 0, sizeof(tab));
  UnpackTab ut; memset(&ut, 0, sizeof(ut));
  tab.n = ut.n = 1; ut.accumulate = accumulate;
  tab.e[0].wd = -1; tab.e[0].cout = cout; tab.e[0].cin = cin; tab.e[0].cinpad = cin_pad;
  ut.e[0].cout = cout; ut.e[0].cin = cin; ut.e[0].cinpad = cin_pad; ut.e[0].taps = 9; ut.e[0].nvec = 0; ut.e[0].nslab = 1;
  pack_tiles(tab);
  NUNET_LAUNCH(unpack_tiled_kernel, dim3(tab.ntiles), dim3(256), 0, (hipStream_t)s, dw, g, tab, ut);   // no vectors: no tail block
  return nunet_check_launch("unpack_wgrad");
}

int plan_pack_weights(const nunet_plan* P, const float* params, void* arena, hipStream_t st) {
  return NUNET_DISPATCH(P->cfg.dtype, launch_pack, params, (void*)AB(arena, P->off_wpack), P->ptab, st);
}

int plan_unpack_grads(nunet_plan* P, void* arena, float* grads, int accumulate, hipStream_t st) {
  P->utab.accumulate = accumulate;
  ProfScope ps(PC_UNPACK, 0, (double)P->nparams * (accumulate ? 12 : 8), st);
  NUNET_LAUNCH(unpack_tiled_kernel, dim3(P->ptab.ntiles + P->utab.n), dim3(256), 0, st, (const float*)AB(arena, P->off_gs), grads, P->ptab, P->utab);
  return nunet_check_launch("unpack_grads");
}

template <typename O> static int launch_unpack_step(nunet_plan* P, void* arena, float* params, const O& o, float grad_scale, float* grads,
                                                    double bytes, hipStream_t st) {
  UpdP u;
  u.params = params; u.scratch = (const float*)AB(arena, P->off_gs); u.grads = grads;
  u.gscale = grad_scale;
  ProfScope ps(PC_SGD, 0, bytes, st);
  NUNET_LAUNCH((unpack_sgd_tiled_kernel<O>), dim3(P->ptab.ntiles + P->utab.n), dim3(256), 0, st, u, o, P->ptab, P->utab);
  return nunet_check_launch("plan_opt_step");
}

// The fused step on the plan's own buffers with any optimiser, gradient scratch -> step -> fp32 master parameters
// (unpack_sgd_tiled_kernel; the next forward repacks). `grads` (flat OIHW arena) is optional: when given it receives the
// (scaled) gradients as nunet_plan_backward would have left them. Adam streams its second state buffer on top.
extern "C" int nunet_plan_opt_step(nunet_plan* P, float* params, const nunet_optim* opt, void* arena, size_t arena_bytes, float grad_scale,
                                   float* grads, nunet_stream_t s) {
  NUNET_REQUIRE(P, "plan_opt_step: null plan");
  CK(opt_check(opt, "plan_opt_step", true));      // (the caller's descriptor first: a bad one is reported whatever the plan is)
  REFUSE_PRUNED("plan_opt_step");
  NUNET_REQUIRE(params && arena, "plan_opt_step: null pointer");
  ARENA_CHECK("plan_opt_step");
  return opt_dispatch(opt, [&](const auto& o) {
    const double bytes = (double)P->nparams * (20.0 + (grads ? 4.0 : 0.0) + 8.0 * (o.NS - 1));
    return launch_unpack_step(P, arena, params, o, grad_scale, grads, bytes, (hipStream_t)s);
  });
}

extern "C" size_t nunet_plan_grad_sqnorm_ws_bytes(const nunet_plan* P) { return (P && !P->depth) ? (size_t)(P->ptab.ntiles + P->utab.n) * sizeof(double) : 0; }
extern "C" int nunet_plan_grad_sqnorm(nunet_plan* P, const void* arena, size_t arena_bytes, double* ws, size_t ws_bytes, nunet_stream_t s) {
  NUNET_REQUIRE(P, "plan_grad_sqnorm: null plan");
  REFUSE_PRUNED("plan_grad_sqnorm");
  NUNET_REQUIRE(arena && ws, "plan_grad_sqnorm: null pointer");
  ARENA_CHECK("plan_grad_sqnorm");
  NUNET_REQUIRE(((uintptr_t)ws & 7) == 0, "plan_grad_sqnorm: ws must be 8-byte aligned");
  NUNET_REQUIRE(ws_bytes >= nunet_plan_grad_sqnorm_ws_bytes(P), "plan_grad_sqnorm: workspace of %zu bytes, nunet_plan_grad_sqnorm_ws_bytes = %zu",
                ws_bytes, nunet_plan_grad_sqnorm_ws_bytes(P));
  ProfScope ps(PC_SGD, 0, (double)P->nparams * 4, (hipStream_t)s);
  NUNET_LAUNCH(plan_sqnorm_kernel, dim3(P->ptab.ntiles + P->utab.n), dim3(256), 0, (hipStream_t)s,
               (const float*)AB(const_cast<void*>(arena), P->off_gs), P->ptab, P->utab, ws);
  return nunet_check_launch("plan_grad_sqnorm");
}

// Repack the 16-bit weight layouts from the fp32 master parameters (what nunet_plan_forward does first unless told
// that they are current): needed before a forward that is told so (bit 1 of its `training` flags).
extern "C" int nunet_plan_repack(nunet_plan* P, const float* params, void* arena, size_t arena_bytes, nunet_stream_t s) {
  NUNET_REQUIRE(P && params && arena, "plan_repack: null pointer");
  ARENA_CHECK("plan_repack");
  return plan_pack_weights(P, params, arena, (hipStream_t)s);
}

// layers of exec nodes [k_lo, k_hi] whose gradient was split (ks > 1; unsplit layers write the scratch directly)
int launch_reduce(nunet_plan* P, void* arena, int k_lo, int k_hi, hipStream_t st) {
  RedTab tab; tab.n = 0; tab.nblocks = 0;
  double bytes = 0;
  for (int k = k_hi; k >= k_lo; --k)
    for (int cv = 1; cv >= 0; --cv) {
      const ConvL& c = cv ? P->exec[k].c2 : P->exec[k].c1;
      if (c.ks <= 1) continue;
      RedEnt& en = tab.e[tab.n++];
      en.slab = c.slab; en.dst = c.gs; en.stride = 9LL * c.cout * c.cinpad; en.n4 = en.stride / 4; en.ks = c.ks; en.blk0 = tab.nblocks;
      tab.nblocks += (int)((en.n4 + 63) / 64);
      bytes += (double)en.stride * 4 * (c.ks + 1);
    }
  if (tab.n == 0) return NUNET_OK;
  ProfScope ps(PC_UNPACK, 0, bytes, st);
  NUNET_LAUNCH(reduce_kernel, dim3(tab.nblocks), dim3(256), 0, st, (const float*)AB(arena, P->off_slab), (float*)AB(arena, P->off_gs), tab);
  return nunet_check_launch("wgrad slab reduce");
}
