// tta.hip — test-time augmentation (Test-time augmentation): the view of an fp32 NCHW batch under a geometric
// code (nunet_dihedral_nchw) and the merge of a view's logits back into the source frame (nunet_tta_merge). `code` is the
// input pipeline's aug: rot90 count (bits 0-1, np.rot90 sense) | hflip (bit 2) | vflip (bit 3). Both kernels map pixels
// through aug_source_pixel (pipeline.h) - view pixel (y, x) <-> source pixel (ry, rx) - so the merge undoes exactly what the
// view did.
//
// One kernel template moves 32 x 32 tiles of the VIEW frame of one plane through LDS. Under an odd rotation count the map is a
// transpose: rx follows the view's y. The phase that touches the source-frame buffer (the load of the dihedral, the store of
// the merge) therefore walks the tile transposed - its lanes run along y - so that global reads run along rows of the buffer
// read and global writes along rows of the buffer written, for every code. The LDS tile is written by rows and read by
// columns in that case: its rows are padded to 33 dwords, so the 32 lanes of a ds_read_b32 / ds_write_b32 group (bank =
// dword address mod 32) hit (33 * lane + c) mod 32 = (lane + c) mod 32: 32 distinct banks. Even codes take the same path
// with a row read (a flip only reverses the order of the lanes' addresses inside a row segment).
#include "pipeline.h"

#define TTA_TILE 32
#define TTA_LD (TTA_TILE + 1)
#define TTA_ROWS 8                      // 256 threads: 8 tile rows of 32 lanes per trip, 4 trips per tile
#define TTA_GRID_CAP 4096               // (launch_pipeline's cap)

enum { TTA_OP_VIEW = 0, TTA_OP_LOGIT = 1, TTA_OP_PROB = 2 };

// the fp32 sigmoid of the loss kernels (loss.hip, sigmoidf_)
__device__ __forceinline__ float tta_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// TTA_OP_VIEW:  in = source planes [H][W], out = view planes [Hv][Wv]:   out[y][x] = in[ry][rx]
// TTA_OP_LOGIT / TTA_OP_PROB: in = view planes [Hv][Wv], out = acc planes [H][W]:   out[ry][rx] (+)= f(in[y][x])
// A workgroup takes (plane, tile) items grid-stride; every thread of it makes the same number of trips (the barriers).
template <int OP>
__global__ __launch_bounds__(256) void tta_tile_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int code, long long planes,
                                                       int first, int last, float views) {
#pragma clang fp contract(off)
  __shared__ float tile[TTA_TILE][TTA_LD];
  const bool odd = code & 1;
  const int Hv = odd ? W : H, Wv = odd ? H : W;
  const int tilesX = (Wv + TTA_TILE - 1) / TTA_TILE, tilesY = (Hv + TTA_TILE - 1) / TTA_TILE;
  const long long per = (long long)tilesX * tilesY, items = planes * per, hw = (long long)H * W;
  const int tx = threadIdx.x & (TTA_TILE - 1), ty = threadIdx.x / TTA_TILE;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long p = it / per;
    const int t = (int)(it % per), y0 = (t / tilesX) * TTA_TILE, x0 = (t % tilesX) * TTA_TILE;
    const float* ip = in + p * hw;
    float* op = out + p * hw;
#pragma unroll
    for (int r = 0; r < TTA_TILE / TTA_ROWS; ++r) {
      const int a = ty + r * TTA_ROWS;
      if constexpr (OP == TTA_OP_VIEW) {
        // rows of the source: under an odd code lane tx walks the view's y
        const int vy = odd ? y0 + tx : y0 + a, vx = odd ? x0 + a : x0 + tx;
        if (vy < Hv && vx < Wv) {
          int ry, rx;
          aug_source_pixel(code, H, W, vy, vx, ry, rx);
          tile[a][tx] = ip[(long long)ry * W + rx];
        }
      } else {
        const int vy = y0 + a, vx = x0 + tx;
        if (vy < Hv && vx < Wv) {
          const float v = ip[(long long)vy * Wv + vx];
          tile[a][tx] = OP == TTA_OP_PROB ? tta_sigmoid(v) : v;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TTA_TILE / TTA_ROWS; ++r) {
      const int a = ty + r * TTA_ROWS;
      if constexpr (OP == TTA_OP_VIEW) {
        const int vy = y0 + a, vx = x0 + tx;
        if (vy < Hv && vx < Wv) op[(long long)vy * Wv + vx] = odd ? tile[tx][a] : tile[a][tx];
      } else {
        // rows of the accumulator: under an odd code lane tx walks the view's y; this thread alone reads and writes (ry, rx)
        const int vy = odd ? y0 + tx : y0 + a, vx = odd ? x0 + a : x0 + tx;
        if (vy < Hv && vx < Wv) {
          int ry, rx;
          aug_source_pixel(code, H, W, vy, vx, ry, rx);
          const long long o = (long long)ry * W + rx;
          float s = odd ? tile[tx][a] : tile[a][tx];
          if (!first) s = op[o] + s;
          if (last) {
            s = s / views;
            if constexpr (OP == TTA_OP_PROB) {
              const float pr = fminf(fmaxf(s, 0x1p-23f), 1.0f - 0x1p-23f);
              s = logf(pr) - log1pf(-pr);
            }
          }
          op[o] = s;
        }
      }
    }
    __syncthreads();      // the tile is free for the next item
  }
}

static int tta_args_ok(const char* what, const void* a, const void* b, int N, int C, int H, int W, int code) {
  NUNET_REQUIRE(a && b, "%s: null pointer", what);
  NUNET_REQUIRE(a != b, "%s: source and destination are the same buffer", what);
  NUNET_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: N=%d C=%d H=%d W=%d must be positive", what, N, C, H, W);
  NUNET_REQUIRE(code >= 0 && code <= 15, "%s: code %d is outside 0 .. 15", what, code);
  NUNET_REQUIRE(!(code & 1) || H == W, "%s: code %d has an odd rot90 count, which needs H == W (got %d x %d)", what, code, H, W);
  return NUNET_OK;
}
static int tta_grid(long long planes, int H, int W) {
  return grid_for(planes * ceil_div(H, TTA_TILE) * ceil_div(W, TTA_TILE), 1, TTA_GRID_CAP);      // (tiles of H x W = tiles of W x H)
}

extern "C" int nunet_dihedral_nchw(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, int32_t code, float* dst, nunet_stream_t s) {
  if (int rc = tta_args_ok("dihedral_nchw", src, dst, N, C, H, W, code)) return rc;
  const long long planes = (long long)N * C;
  hipStream_t st = (hipStream_t)s;
  ProfScope ps(PC_LAYOUT, 0, (double)planes * H * W * 8, st);
  NUNET_LAUNCH((tta_tile_kernel<TTA_OP_VIEW>), dim3(tta_grid(planes, H, W)), dim3(256), 0, st, src, dst, H, W, code, planes, 1, 1, 1.0f);
  return nunet_check_launch("dihedral_nchw");
}

extern "C" int nunet_tta_merge(const float* view, int32_t N, int32_t K, int32_t H, int32_t W, int32_t code, int32_t mode, int32_t view_index,
                               int32_t views, float* acc, nunet_stream_t s) {
  if (int rc = tta_args_ok("tta_merge", view, acc, N, K, H, W, code)) return rc;
  NUNET_REQUIRE(mode == NUNET_TTA_LOGIT || mode == NUNET_TTA_PROB, "tta_merge: mode %d is neither LOGIT (0) nor PROB (1)", mode);
  NUNET_REQUIRE(views >= 1 && view_index >= 0 && view_index < views, "tta_merge: view_index %d of %d views", view_index, views);
  const long long planes = (long long)N * K;
  const int first = view_index == 0, last = view_index == views - 1;
  hipStream_t st = (hipStream_t)s;
  ProfScope ps(PC_LAYOUT, 0, (double)planes * H * W * (first ? 8 : 12), st);
  if (mode == NUNET_TTA_PROB) {
    NUNET_LAUNCH((tta_tile_kernel<TTA_OP_PROB>), dim3(tta_grid(planes, H, W)), dim3(256), 0, st, view, acc, H, W, code, planes, first, last, (float)views);
  } else {
    NUNET_LAUNCH((tta_tile_kernel<TTA_OP_LOGIT>), dim3(tta_grid(planes, H, W)), dim3(256), 0, st, view, acc, H, W, code, planes, first, last, (float)views);
  }
  return nunet_check_launch("tta_merge");
}
