/*
 * nunet_diag.h - diagnostic and test hooks of libnunet.so. NOT part of the product boundary (include/nunet.h):
 * nothing in the package's training / evaluation path calls these; tools/ and tests/ do.
 */
#ifndef NUNET_DIAG_H
#define NUNET_DIAG_H

#include "nunet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* use caller-owned streams as lanes (n >= 1, cycled over the 10 lanes) instead of the plan's own (tools/graph_sched_probe.py) */
int nunet_plan_set_lanes(nunet_plan* p, nunet_stream_t* lanes, int32_t n);
/* Diagnostic: with NUNET_STAMPS=1 in the environment every op the plan schedules is followed by a
 * 1-thread kernel that stores the 100 MHz wall clock; this reads them back (synchronises) for the
 * last forward (pass 0) / backward (pass 1), labels one per line ("L<lane> B<i><j>.<op>").
 * Works inside hipGraph replays, where a profiler's dispatch overhead would distort the timeline. */
int nunet_plan_stamps_read(nunet_plan* plan, int32_t pass, uint64_t* ticks, int32_t cap, int32_t* n_out, char* labels, int32_t label_bytes);
/* Diagnostic: a 1-thread kernel on `stream` stores the chip-wide 100 MHz clock to *dst when it runs (works inside a hipGraph:
 * when did this point of the graph execute, relative to another stamp). */
int nunet_debug_stamp(uint64_t* dst, nunet_stream_t stream);
/* Diagnostic (tools/graph_sched_probe.py): `tag` workgroups, the first spins `us` microseconds. */
int nunet_debug_spin(int32_t us, int32_t tag, nunet_stream_t stream);

/* Launch geometry of a 3x3 convolution / weight-gradient descriptor, from the very code the launch runs (tile policy, tile
 * chooser, K-split and persistent-grid rules). Pure host functions: no GPU call, and no pointer of the descriptor is
 * dereferenced or required - only compared with NULL where the launch itself does (splitk_ws enables the K-split, bn_y the
 * fused BatchNorm-backward reduce, whose tables take LDS and so change the grid). The tests use them to state which kernel
 * instantiation and which loop regime a case reaches. */
typedef struct {
  int32_t tile;                     /* 1 = 128 x 32, 2 = 128 x 64, 3 = 256 x 32, 4 = 256 x 64 (the policy's choice when the descriptor says 0) */
  int32_t BM, BN, HPMAX, NT;        /* pixels, output channels, halo-pixel capacity and threads of a workgroup */
  int32_t NI, TH, TW, SH;           /* images x rows x columns of a pixel tile; SH = H + 1 with stacked-rows tiling, else 0 */
  int32_t tilesX, tilesY, tilesG;   /* pixel tiles along x, y (virtual rows when stacked) and over the batch */
  int32_t nCoT;                     /* Cout / BN */
  int32_t S, nch;                   /* K-split slices (1: none) and 64-byte channel chunks of the input */
  int32_t items;                    /* nCoT * tilesX * tilesY * tilesG * S */
  int32_t grid;                     /* workgroups of the launch; workgroup b runs items b, b + grid, ... (after the XCD remap) */
  int32_t per_cu;                   /* workgroups assumed resident per CU when the grid was sized */
} nunet_conv_launch_info;
int nunet_conv3x3_launch_info(const nunet_conv_desc* d, nunet_conv_launch_info* out);

/* What the HIP runtime reports for the conv3x3 kernel instantiation the descriptor's launch would take (tile policy, K-split,
 * fused BatchNorm-backward reduce, input transform as in nunet_conv3x3_launch_info). Needs a device, launches nothing, and
 * like the query above requires no pointer of the descriptor. The tests hold it against the launch geometry: a kernel that
 * spills (localSizeBytes) or of which fewer workgroups fit a CU than the grid was sized for (occupancy < per_cu) fails there. */
typedef struct {
  int32_t numRegs;                  /* hipFuncGetAttributes: vector registers per lane */
  int32_t localSizeBytes;           /* ... scratch (spill) bytes per lane */
  int32_t sharedSizeBytes;          /* ... static LDS bytes per workgroup */
  int32_t blockSize, dynLdsBytes;   /* threads and dynamic LDS bytes of the launch */
  int32_t occupancy;                /* hipOccupancyMaxActiveBlocksPerMultiprocessor at that block size and dynamic LDS */
  int32_t wg_per_cu;                /* workgroups per CU the instantiation promises by registers (its __launch_bounds__) */
} nunet_conv_kernel_attrs_t;
int nunet_conv_kernel_attrs(const nunet_conv_desc* d, nunet_conv_kernel_attrs_t* out);

typedef struct {
  int32_t A, B;                     /* a work item covers 32 A output x 32 B input channels */
  int32_t NI, TH, TW, SH;           /* pixel tile (at most 128 pixels, 192 with halo), as above */
  int32_t tilesX, tilesY, tilesG;
  int32_t nMT;                      /* pixel tiles = tilesX * tilesY * tilesG */
  int32_t nCoT, nCiT;               /* output / input channel tiles */
  int32_t ksplit;                   /* slices of the pixel-tile loop = nunet_conv3x3_wgrad_slabs(d); slice s walks tiles s, s + ksplit, ... */
  int32_t grid;                     /* nCoT * nCiT * ksplit workgroups */
} nunet_wgrad_launch_info;
int nunet_conv3x3_wgrad_launch_info(const nunet_wgrad_desc* d, nunet_wgrad_launch_info* out);

/* Read-only accessor of the block-output GRADIENT slots, the counterpart of nunet_plan_feature: arena byte offset, pitch and
 * channel count of dL/dx_{i,j} (NHWC, in the plan's STORAGE dtype - fp32, bf16 or fp16 as the plan was created). The gradient
 * level buffers are bump-allocated on their own, beside the feature buffers and apart from every per-block scratch: no
 * kernel of the backward pass writes a slot after its last consumer has accumulated into it, so after nunet_plan_backward
 * every slot still holds the complete gradient its block's backward started from. Returns -1 when the plan has no block (i, j). */
int64_t nunet_plan_feature_grad(const nunet_plan* p, int32_t i, int32_t j, int32_t* pitch, int32_t* channels);
/* Read-only accessor of the staged input image, the sibling of nunet_plan_feature: arena byte offset of the padded NHWC image
 * [N][H][W][32] the first convolution reads (STORAGE dtype), written by a staging entry of the sample pipeline (nunet_plan_stage_u8*:
 * any source under StageSink, csrc/pipeline.h) or by the layout launch of nunet_plan_forward; *pitch = 32, *channels = the plan's input_channels (channels input_channels .. 31 are zeros). Pruned
 * plans have it too. Returns -1 for a NULL plan. */
int64_t nunet_plan_image(const nunet_plan* p, int32_t* pitch, int32_t* channels);
/* a1 = relu(bn1(conv1(input))) of block (i, j), the activation between its two convolutions. No pass stores it: conv2 and the
 * weight gradient of conv2 form it in their loaders from the raw conv output y1, which stays in the arena. This entry
 * materialises it on demand after a TRAINING forward - nunet_bn_relu_fwd on y1 with the block's batch sums and the CURRENT
 * gamma / beta in `params` (the running statistics are not touched) - into `out`, dense [N][H_i][W_i][C] in the plan's storage
 * dtype. With x_{i,j} > 0 it gives a test the ReLU decisions the pass actually took. NUNET_EINVAL when the plan has no block (i, j). */
int nunet_plan_block_act1(nunet_plan* p, const float* params, void* arena, size_t arena_bytes, int32_t i, int32_t j, void* out,
                          nunet_stream_t s);

/* Launch census of the last forward (pass 0) and the last backward (pass 1) the plan issued: one entry per 3x3 convolution
 * (forward conv or input gradient) and one per weight-gradient pair, in the order the plan handed them to its scheduler, with
 * the op label the scheduler gives them ("B<i><j>.conv1", ".conv2", ".dgrad2", ".dgrad1", ".wgrad") and the launch geometry
 * nunet_conv3x3_launch_info / nunet_conv3x3_wgrad_launch_info report for the descriptor the plan actually built (its real
 * K-split workspace, fused BatchNorm-backward reduce, input transform and destination split). Host bookkeeping only: no device
 * work, no synchronisation; a pass replayed from a graph leaves the census of its capture. */
enum { NUNET_CENSUS_CONV = 0, NUNET_CENSUS_WGRAD_PAIR = 1 };
typedef struct {
  char label[32];
  int32_t kind;                     /* NUNET_CENSUS_CONV: `conv` and the descriptor facts below; NUNET_CENSUS_WGRAD_PAIR: `wgrad[0..1]` (conv1, conv2) */
  int32_t N, H, W;
  int32_t C0, C1, D0, D1;           /* conv: source and destination split of the descriptor */
  int32_t in_tf, has_bn_y;          /* conv: input transform (NUNET_TF_*), fused BatchNorm-backward reduce */
  uint32_t acc0_mask;               /* conv: accumulating dst0 slots */
  int64_t splitk_ws_floats;         /* conv: K-split workspace offered (0: none) */
  nunet_conv_launch_info conv;
  nunet_wgrad_launch_info wgrad[2];
  int32_t has_tf_store;             /* conv: the transformed input is also written out (nunet_conv_desc.tf_store) */
  int32_t wgrad_tf[2];              /* weight-gradient pair: operand transforms of conv1's / conv2's problem, bit 0 = x_tf, bit 1 = d_tf */
} nunet_plan_census_entry;
int32_t nunet_plan_census_count(const nunet_plan* p, int32_t pass);
int nunet_plan_census_get(const nunet_plan* p, int32_t pass, int32_t index, nunet_plan_census_entry* out);

/* Launch geometry of the BCE-Dice loss, the fused loss step (NUNET_LOSS_BCE_DICE, and the first launch of NUNET_LOSS_BCE_LOGITS,
 * which runs on the same grid), the IoU counts, the mask export and the stand-alone BCEWithLogitsLoss pair, from
 * the very expressions their launches use. A pure host function: no GPU call, no pointer but `out`. N and heads are read where
 * the entry has them (the BCE-Dice loss and the loss step; heads by the loss step alone), per_or_n is the elements per image of
 * those and the element count of the others. It refuses what the entry itself refuses by size (N, heads, the loss step's 2^24 per image).
 * Every kernel walks its items with one grid-stride loop per (y, z) plane of the grid; the BCE-Dice forward also runs a
 * one-wave final kernel over the grid.x partial slabs of each image. */
enum { NUNET_LOSS_ENTRY_BCE_DICE_FWD = 0, NUNET_LOSS_ENTRY_BCE_DICE_BWD = 1, NUNET_LOSS_ENTRY_LOSS_STEP = 2,
       NUNET_LOSS_ENTRY_IOU_COUNTS = 3, NUNET_LOSS_ENTRY_SIGMOID_U8 = 4, NUNET_LOSS_ENTRY_BCE_LOGITS_FWD = 5,
       NUNET_LOSS_ENTRY_BCE_LOGITS_BWD = 6 };
typedef struct {
  int32_t grid_x, grid_y, grid_z;   /* workgroups: blocks per image (or over all elements) x images x heads */
  int32_t block;                    /* threads of a workgroup */
  int64_t items;                    /* loop items of one (y, z) plane: elements, 4-element vectors for the mask export (its n % 4 tail is apart) */
  int64_t trips_max, trips_min;     /* most and fewest grid-stride trips a thread takes (0: a thread without an item) */
} nunet_loss_launch_info_t;
int nunet_loss_launch_info(int32_t entry, int32_t N, int64_t per_or_n, int32_t heads, nunet_loss_launch_info_t* out);

/* The counterpart for nunet_seg_metrics: its first launch runs grid_x blocks per plane x K classes (grid_y) x N images (grid_z),
 * one grid-stride loop over the hw pixels of a plane; a one-workgroup launch of 256 threads follows, in which thread j adds
 * the entries j, j + 256, ... of the N * grid_x partials of each class. A pure host function; refuses what the entry refuses by size. */
int nunet_seg_metrics_launch_info(int32_t N, int32_t K, int64_t hw, nunet_loss_launch_info_t* out);

/* The x2 bilinear upsample's backward pass by its gather kernel (one thread per output, every tap a global load), whatever the
 * shape: the arguments of nunet_upsample2x_bwd, which takes the LDS-tiled kernel when H >= 4 and W >= 4. The two leave the
 * same bytes; the tests hold one against the other. */
int nunet_upsample2x_bwd_gather(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C,
                                const void* dy, int32_t PDY, void* dx, int32_t PDX, int32_t accumulate, nunet_stream_t stream);
/* Launch geometry of the upsample forward (backward = 0) or backward (1) pass, from the very code the launch runs. A pure host
 * function. Pass p (of `passes`) covers the g = min(workgroups, items - p * workgroups) items from p * workgroups on: workgroup
 * b < g takes item p * workgroups + the XCD remap of (b, g) below. The forward kernel and the gather kernel (which does not
 * remap) count blocks of 256 outputs as items. */
typedef struct {
  int32_t tiled;                    /* backward: 1 = LDS-tiled kernel, 0 = gather kernel; forward: 0 */
  int32_t workgroups, passes;
  int32_t TR, TC, SG;               /* tiled: low-res rows, columns and 16-byte channel groups of a work item (edge items hold fewer) */
  int32_t lds_bytes;                /* tiled: static LDS of a workgroup */
  int32_t reserved;
  int64_t items;
} nunet_upsample_launch_info_t;
int nunet_upsample_launch_info(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t backward, nunet_upsample_launch_info_t* out);
/* Launch geometry of nunet_head_fwd (with_bn = 0: a thread per pixel) or nunet_head_fwd_bn (with_bn = 1: C / (16 bytes) lanes per
 * pixel, the grid of nunet_bn_relu_fwd), from the very expressions the launches use. A pure host function. items = pixels;
 * trips_max / trips_min = the most / fewest pixels one thread (one lane group) walks - nunet_head_fwd_bn takes them four per loop pass. */
int nunet_head_launch_info(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t with_bn, nunet_loss_launch_info_t* out);

/* Forward-pass and scheduler choices of a plan, all bit-identical; each is read when a pass is issued, so set it before the
 * first forward / capture. (Defaults also from the environment at plan creation: NUNET_HEAD_BN, NUNET_BN_UP, NUNET_WAIT_PRUNE.)
 * head_bn (default 1): a head whose slot no block reads in the forward pass - the last head of a full plan, final<L> of a pruned
 *   one - runs with its block's BatchNorm2 + ReLU as ONE launch (nunet_head_fwd_bn); 0: the two launches.
 * bn_up: which blocks' BatchNorm2 launch also writes the x2 upsample their reader concatenates (nunet_bn_fwd_desc.up) instead of
 *   that reader's stand-alone upsample launch: none, the four row ends of the critical chain (B40, B31, B22, B13; every decoder
 *   hop of the plain UNet), or every block that is upsampled.
 * wait_prune (default 1): the lane scheduler drops a cross-lane wait that lane order plus the waits already made imply; 0: every
 *   requested wait is made. */
enum { NUNET_BN_UP_NONE = 0, NUNET_BN_UP_CHAIN = 1, NUNET_BN_UP_ALL = 2 };
int nunet_plan_set_head_bn(nunet_plan* p, int32_t enable);
int nunet_plan_set_bn_up(nunet_plan* p, int32_t mode);
int nunet_plan_set_wait_prune(nunet_plan* p, int32_t enable);
/* The scheduler's wait decision over plain arrays (a pure host function). nops ops in issue order, op b on lane op_lane[b] (lanes
 * are in-order) asks to wait for the ops edge_src[edge_off[b] .. edge_off[b + 1]), each issued before b. keep[e] = 1: the wait is
 * made; 0: it is implied by lane order and the waits kept so far (a producer on b's own lane always is). At most 16 lanes. */
int nunet_wait_prune_host(int32_t nlanes, int32_t nops, const int32_t* op_lane, const int32_t* edge_off, const int32_t* edge_src, uint8_t* keep);
/* The list scheduler's placement over plain arrays (a pure host function: no plan, no HIP call). nops ops in program order, op b
 * of estimated cost cost[b] (us) reads the resource ids rd[rd_off[b] .. rd_off[b + 1]) and writes wr[wr_off[b] .. wr_off[b + 1]);
 * ids are 0..511, at most 12 reads and 8 writes per op. The hazards of that order (read after write, write after write, write
 * after read) form a DAG; order[q] = the op issued q-th (a topological order of the DAG), lane[b] = the lane (0..2) of op b. */
int nunet_list_schedule_host(int32_t nops, const float* cost, const int32_t* rd_off, const int32_t* rd, const int32_t* wr_off, const int32_t* wr,
                             int32_t* order, int32_t* lane);
/* The work item that workgroup b of G takes first (common.h, xcd_remap: one contiguous item range per XCD), evaluated on the host. */
int32_t nunet_xcd_remap_host(int32_t b, int32_t G);

#ifdef __cplusplus
}
#endif
#endif /* NUNET_DIAG_H */
