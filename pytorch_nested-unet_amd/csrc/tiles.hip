// tiles.hip - full-resolution tiled inference (include/nunet.h, nunet_tile / nunet_tile_grid):
//   nunet_stitch_tiles: the overlapping windows' fp32 logits blended back into masks of the sources' sizes.
// (The way in - fixed-size, border-reflected windows cut out of ragged uint8 sources, nunet_crop_tiles_u8 and
// nunet_plan_stage_u8_tiles - is the sample pipeline's TileSrc: pipeline.h.)
// The kernel is element-wise over its DESTINATION with a capped grid and a grid-stride loop; every descriptor is device
// memory read at run time and none is trusted.
#include "common.h"

// ---------------------------------------------------------------------------
// Stitch. Workgroups (x, y): y walks the samples, x the sample's K * H * W output elements, both with a stride of the grid, so
// samples of any size fit a launch whose shape the host fixes without seeing H or W. Along one axis a pixel p of a source of
// extent S is covered by tile j iff o_j <= p < o_j + T with o_j = min(j * stride, max(S - T, 0)). No tile below
// lo = (p < T ? 0 : (p - T) / stride + 1) reaches p (o_j <= j * stride), none above p / stride starts at or before it unless p
// has reached the clamped origin of the last tile: [lo, hi] is tested tile by tile, which holds for any grid, consistent or not.
// ---------------------------------------------------------------------------
#define STITCH_MAX_WG 2048      // workgroups of one launch (x * y)
struct AxisCover { int lo, hi, last; };
__device__ __forceinline__ AxisCover axis_cover(int p, int S, int T, int stride, int n) {
  AxisCover c;
  c.last = max(S - T, 0);
  c.lo = p < T ? 0 : (p - T) / stride + 1;
  c.hi = min(p / stride, n - 1);
  if ((long long)p >= min((long long)(n - 1) * stride, (long long)c.last)) c.hi = n - 1;
  return c;
}
__device__ __forceinline__ int axis_origin(int j, int stride, int last) { return (int)min((long long)j * stride, (long long)last); }
__device__ __forceinline__ int window_weight(int window, int i, int T) { return window == NUNET_WINDOW_UNIFORM ? 1 : min(i + 1, T - i); }

__global__ __launch_bounds__(256) void stitch_tiles_kernel(const float* __restrict__ tile_logits, int n_tiles, int K, int Th, int Tw,
                                                           const nunet_u8_sample* __restrict__ samples, const nunet_tile_grid* __restrict__ grids,
                                                           int n_samples, int window, const float* __restrict__ thr, float* __restrict__ out_logits,
                                                           uint8_t* __restrict__ out_u8, long long out_elems) {
  __shared__ float s_thr[256];
  if (out_u8) {
    if (threadIdx.x < 255) s_thr[threadIdx.x] = thr[threadIdx.x];
    __syncthreads();
  }
  for (int n = blockIdx.y; n < n_samples; n += gridDim.y) {
    const nunet_u8_sample d = samples[n];
    const nunet_tile_grid g = grids[n];
    if (d.H < 1 || d.W < 1 || d.H > NUNET_RESIZE_MAX_EXTENT || d.W > NUNET_RESIZE_MAX_EXTENT) continue;
    const long long hw = (long long)d.H * d.W, total = hw * K;
    if (g.out_offset < 0 || g.out_offset > out_elems || total > out_elems - g.out_offset) continue;
    const bool grid_ok = g.ny >= 1 && g.nx >= 1 && g.stride_y >= 1 && g.stride_x >= 1 && g.first_tile >= 0 &&
                         (long long)g.ny * g.nx <= (long long)n_tiles - g.first_tile;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
      float v = 0.f;
      bool covered = false;
      if (grid_ok) {
        const int x = (int)(e % d.W);
        const long long q = e / d.W;
        const int y = (int)(q % d.H);
        const int k = (int)(q / d.H);
        const AxisCover cy = axis_cover(y, d.H, Th, g.stride_y, g.ny), cx = axis_cover(x, d.W, Tw, g.stride_x, g.nx);
        float acc = 0.f, wsum = 0.f, one = 0.f;
        int count = 0;
        for (int j = cy.lo; j <= cy.hi; ++j) {
          const int ty = y - axis_origin(j, g.stride_y, cy.last);
          if (ty < 0 || ty >= Th) continue;
          const int wy = window_weight(window, ty, Th);
          for (int i = cx.lo; i <= cx.hi; ++i) {
            const int tx = x - axis_origin(i, g.stride_x, cx.last);
            if (tx < 0 || tx >= Tw) continue;
            const long long t = (long long)g.first_tile + (long long)j * g.nx + i;
            const float l = tile_logits[((t * K + k) * Th + ty) * Tw + tx];
            const float w = (float)(wy * window_weight(window, tx, Tw));
            acc += w * l;
            wsum += w;
            one = l;
            ++count;
          }
        }
        covered = count > 0;
        v = count == 1 ? one : covered ? acc / wsum : 0.f;      // single cover: the tile's own logit, bit for bit
      }
      if (out_logits) out_logits[g.out_offset + e] = v;
      if (out_u8) out_u8[g.out_offset + e] = covered ? (uint8_t)sigmoid_byte(s_thr, v) : (uint8_t)0;
    }
  }
}
extern "C" int nunet_stitch_tiles(const float* tile_logits, int32_t n_tiles, int32_t K, int32_t Th, int32_t Tw, const nunet_u8_sample* samples,
                                  const nunet_tile_grid* grids, int32_t n_samples, int32_t window, const float* thresholds, float* out_logits,
                                  uint8_t* out_u8, int64_t out_elems, nunet_stream_t s) {
  NUNET_REQUIRE(tile_logits && samples && grids, "stitch_tiles: null pointer");
  NUNET_REQUIRE(out_logits || out_u8, "stitch_tiles: neither out_logits nor out_u8 given");
  NUNET_REQUIRE(!out_u8 || thresholds, "stitch_tiles: out_u8 needs the thresholds of nunet_sigmoid_u8");
  NUNET_REQUIRE(n_tiles > 0 && K > 0 && n_samples > 0 && out_elems > 0, "stitch_tiles: n_tiles=%d K=%d n_samples=%d out_elems=%lld must be positive",
                n_tiles, K, n_samples, (long long)out_elems);
  NUNET_REQUIRE(Th >= 1 && Tw >= 1 && Th <= NUNET_RESIZE_MAX_EXTENT && Tw <= NUNET_RESIZE_MAX_EXTENT, "stitch_tiles: tile %d x %d: extents are 1 .. %d",
                Th, Tw, NUNET_RESIZE_MAX_EXTENT);
  NUNET_REQUIRE(window == NUNET_WINDOW_TENT || window == NUNET_WINDOW_UNIFORM, "stitch_tiles: window %d is neither TENT (0) nor UNIFORM (1)", window);
  // every source pixel lies in a tile, so the n_samples sources hold at most n_tiles * Th * Tw pixels: the x extent is sized for
  // the mean sample (larger ones take more trips), capped so that the launch has at most STITCH_MAX_WG workgroups
  const int gy = n_samples < STITCH_MAX_WG ? n_samples : STITCH_MAX_WG;
  const int gx = grid_for(ceil_div64((int64_t)n_tiles * Th * Tw * K, n_samples), 256, STITCH_MAX_WG / gy);
  hipStream_t st = (hipStream_t)s;
  ProfScope ps(PC_LAYOUT, 0, (double)n_tiles * K * Th * Tw * 4, st);
  NUNET_LAUNCH(stitch_tiles_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, tile_logits, n_tiles, K, Th, Tw, samples, grids, n_samples,
               window, thresholds, out_logits, out_u8, (long long)out_elems);
  return nunet_check_launch("stitch_tiles");
}
