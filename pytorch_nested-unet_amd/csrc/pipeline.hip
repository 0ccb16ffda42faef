// pipeline.hip — the stand-alone entries of the device-side sample pipeline (pipeline.h): each checks its arguments, fills
// one source and one sink and makes one launch of pipeline_kernel. What reference dataset.py:66-74 does on the host after
// decoding — albumentations Normalize() (trains.py:266), the extra /255 (dataset.py:71), HWC -> CHW (dataset.py:72) — plus the
// augmentations of trains.py:258-264 (RandomRotate90 / Flip, the colour OneOf) applied per sample from host-drawn codes,
// Resize (trains.py:265, 269) on ragged sources and the tile crop of full-resolution inference. Input stays uint8 over PCIe.
//   aug[n] = rot90 count (bits 0-1, counter-clockwise like np.rot90) | hflip (bit 2) | vflip (bit 3)
// (The four entries that write a plan's image, nunet_plan_stage_u8*, sit with the plan in plan.hip.)
#include "pipeline.h"

extern "C" int nunet_preprocess_u8(const uint8_t* u8_nhwc, int32_t N, int32_t H, int32_t W, int32_t C, const float* mean, const float* stdv,
                                   const int32_t* aug, float post_scale, float* out_nchw, nunet_stream_t s) {
  if (int rc = pipeline_args_ok("preprocess_u8", u8_nhwc && out_nchw, N, C, H, W)) return rc;
  return launch_pipeline("preprocess_u8", DenseSrc<false>{u8_nhwc, H, W, C, aug, nullptr}, PlanesSink{out_nchw, C, H, W, mean, stdv, post_scale}, N, H, W,
                         (double)N * C * H * W * 5, (hipStream_t)s);
}
extern "C" int nunet_preprocess_u8_color(const uint8_t* u8_nhwc, int32_t N, int32_t H, int32_t W, int32_t C, const float* mean, const float* stdv,
                                         const int32_t* aug, const nunet_color_aug* color, float post_scale, float* out_nchw, nunet_stream_t s) {
  if (int rc = pipeline_args_ok("preprocess_u8_color", u8_nhwc && out_nchw, N, C, H, W)) return rc;
  NUNET_REQUIRE(C == 3 && mean && stdv, "preprocess_u8_color: images only: C=%d must be 3, mean and stdv given", C);
  if (!color) return nunet_preprocess_u8(u8_nhwc, N, H, W, C, mean, stdv, aug, post_scale, out_nchw, s);
  return launch_pipeline("preprocess_u8_color", DenseSrc<true>{u8_nhwc, H, W, C, aug, color}, PlanesSink{out_nchw, C, H, W, mean, stdv, post_scale}, N, H, W,
                         (double)N * H * W * 15, (hipStream_t)s);
}
// (may run in place: pipeline.h, sources)
extern "C" int nunet_color_aug_u8(const uint8_t* src, int32_t N, int32_t H, int32_t W, int32_t C, const nunet_color_aug* color, uint8_t* dst,
                                  nunet_stream_t s) {
  if (int rc = pipeline_args_ok("color_aug_u8", src && dst && color, N, C, H, W)) return rc;
  NUNET_REQUIRE(C == 3, "color_aug_u8: the colour ops are defined on RGB: C=%d must be 3", C);
  return launch_pipeline("color_aug_u8", DenseSrc<true>{src, H, W, C, nullptr, color}, BytesSink{dst, C}, N, H, W, (double)N * H * W * 6, (hipStream_t)s);
}

extern "C" int nunet_resize_u8(const uint8_t* pool, int64_t pool_bytes, const nunet_u8_sample* samples, int32_t N, int32_t C, int32_t Hd,
                               int32_t Wd, int32_t mode, const int32_t* aug, const nunet_color_aug* color, uint8_t* dst, nunet_stream_t s) {
  if (int rc = pipeline_args_ok("resize_u8", pool && samples && dst, N, C, Hd, Wd, "destination", pool_bytes)) return rc;
  NUNET_REQUIRE(mode == NUNET_RESIZE_LINEAR || mode == NUNET_RESIZE_NEAREST, "resize_u8: mode %d is neither LINEAR (0) nor NEAREST (1)", mode);
  NUNET_REQUIRE(!color || (mode == NUNET_RESIZE_LINEAR && C == 3), "resize_u8: the colour ops are defined on RGB images under LINEAR: mode=%d C=%d", mode, C);
  const double bytes = (double)N * Hd * Wd * C * (mode == NUNET_RESIZE_LINEAR ? 5 : 2);
  const BytesSink sink = {dst, C};
  hipStream_t st = (hipStream_t)s;
  if (mode == NUNET_RESIZE_NEAREST) return launch_pipeline("resize_u8", ResizeSrc<true, false>{pool, pool_bytes, samples, C, Hd, Wd, aug, nullptr}, sink, N, Hd, Wd, bytes, st);
  if (color) return launch_pipeline("resize_u8", ResizeSrc<false, true>{pool, pool_bytes, samples, C, Hd, Wd, aug, color}, sink, N, Hd, Wd, bytes, st);
  return launch_pipeline("resize_u8", ResizeSrc<false, false>{pool, pool_bytes, samples, C, Hd, Wd, aug, nullptr}, sink, N, Hd, Wd, bytes, st);
}
extern "C" int nunet_preprocess_u8_resize(const uint8_t* pool, int64_t pool_bytes, const nunet_u8_sample* samples, int32_t N, int32_t C,
                                          int32_t Hd, int32_t Wd, const float* mean, const float* stdv, const int32_t* aug,
                                          float post_scale, float* out_nchw, nunet_stream_t s) {
  if (int rc = pipeline_args_ok("preprocess_u8_resize", pool && samples && out_nchw, N, C, Hd, Wd, "destination", pool_bytes)) return rc;
  return launch_pipeline("preprocess_u8_resize", ResizeSrc<true, false>{pool, pool_bytes, samples, C, Hd, Wd, aug, nullptr},
                         PlanesSink{out_nchw, C, Hd, Wd, mean, stdv, post_scale}, N, Hd, Wd, (double)N * C * Hd * Wd * 5, (hipStream_t)s);
}

extern "C" int nunet_crop_tiles_u8(const uint8_t* pool, int64_t pool_bytes, const nunet_u8_sample* samples, int32_t n_samples,
                                   const nunet_tile* tiles, int32_t N, int32_t C, int32_t Th, int32_t Tw, uint8_t* dst, nunet_stream_t s) {
  if (int rc = pipeline_args_ok("crop_tiles_u8", pool && samples && tiles && dst, N, C, Th, Tw, "tile", pool_bytes)) return rc;
  NUNET_REQUIRE(n_samples > 0, "crop_tiles_u8: n_samples=%d must be positive", n_samples);
  return launch_pipeline("crop_tiles_u8", TileSrc{pool, pool_bytes, samples, n_samples, tiles, C}, BytesSink{dst, C}, N, Th, Tw, (double)N * Th * Tw * C * 2,
                         (hipStream_t)s);
}
