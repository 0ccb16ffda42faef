// plan.h — what plan.hip (creation, views, passes), weights.hip (the weight-layout kernels) and sched.hip (the lane scheduler)
// share: the plan's static layout, the runtime objects it owns, and the few functions that cross those files.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "common.h"

#define NUNET_INTERNAL __attribute__((visibility("hidden")))   // crosses files, not the library's boundary

static const int NBF[5] = {32, 64, 128, 256, 512};  // archs1.py:78

// batched weight pack / gradient unpack: the tables the plan fills at creation and weights.hip's kernels walk
#define MAXENT 40
#define HEAD_SLABS 256
struct PackEnt { long long src, wf, wd; int cout, cin, cinpad; };
struct PackTab { int n; int ntiles; PackEnt e[MAXENT]; int tile0[MAXENT + 1]; };
struct UnpackEnt { long long src, dst; int cout, cin, cinpad, taps, nvec, nslab; };   // nslab > 1: sum of partial slabs (heads)
struct UnpackTab { int n; int accumulate; UnpackEnt e[MAXENT]; };

struct ConvL {
  int cin, cinpad, cout;
  long long w_off, b_off, g_off, be_off;  // floats into flat params
  long long rm_off, rv_off; int bn_index; // floats into bnbuf / index into nbt
  long long wf, wd;                       // elements of T into the packed-weight region (wd -1: none)
  long long gs;                           // floats into grad scratch: [dw 9*cout*cinpad][db][dgamma][dbeta]
  long long stats, save, bsum;            // floats into the fp32 small-vector regions (x REPLICAS x 2 int64 words in the fixed-point regions)
  long long slab; int ks, wg_target;      // weight-gradient K-split slabs: floats into the slab region, slices, workgroup target
};
struct Node {
  int i, j;
  int in_prefix;   // number of level slots concatenated in front (0: encoder input)
  int out_slot;    // slot of X_i receiving the block output
  int up_slot;     // slot of X_{i+1} that is upsampled into the concat, -1: none
  ConvL c1, c2;
  size_t y1, y2, up, pin;      // arena byte offsets (a1 = relu(bn1(y1)) is never stored: its two readers form it in their loaders)
  size_t dy[2], da1, gup, gpin;   // ... backward scratch (dY of conv2 / conv1) of the BLOCK, so blocks of one level can run on different lanes
  size_t sk; long long sk_floats; // ... fp32 K-split slabs of the BLOCK (blocks of the grid-starved levels; 0 floats: none)
  // backward pass, decided at creation (plan_backward_facts): destinations that an earlier op of the pass wrote first are accumulated into
  unsigned acc0_mask;             // dgrad1: bit q = slot q of the concat prefix's gradient
  int acc_pool, acc_up;           // pool-backward / upsample-backward
  bool bn2_in_head;               // the reduce pass of BatchNorm2's backward rides in a head's backward (Head::bnr_block)
};
struct Head { long long w_off, b_off, gs; int slot; int acc, bnr_block; };   // backward: accumulate flag, block whose BN2 reduce it carries (-1: none)
// what the resource ids of the lane scheduler are laid out for (NestedUNet has 15 blocks, UNet 9)
#define NUNET_MAX_BLOCKS 15
#define NUNET_MAX_HEADS 4

#define NLANES 10
#define STAMP_CAP 512
struct NUNET_INTERNAL PlanRt {  // runtime objects owned by the plan (host side only)
  hipStream_t lanes[NLANES] = {};
  bool lanes_ok = true;
  std::vector<hipEvent_t> events[2];   // [0] forward, [1] backward: an event is never re-recorded within one capture
  size_t events_used[2] = {0, 0};
  int multistream = 1;
  int schedule = NUNET_SCHEDULE_LANES;     // NUNET_SCHEDULE_LANES: an op runs on its block's lane; NUNET_SCHEDULE_LIST: Sched::run_list picks
  int wgrad_dy = 0;                        // nunet_plan_set_wgrad_dy: the weight gradients form dy1 / dy2 in their loaders (no side stores)
  int head_bn = 1;                         // nunet_plan_set_head_bn: BatchNorm2 of a head-only block output rides in the head's launch (default 1)
  int bn_up = NUNET_BN_UP_NONE;            // nunet_plan_set_bn_up: NUNET_BN_UP_* - which producers' BatchNorm2 launch also upsamples
  int wait_prune = 1;                      // nunet_plan_set_wait_prune: cross-lane waits that lane order already implies are dropped (default 1)
  bool lanes_external = false;
  std::vector<hipStream_t> cap_streams;   // never-reused streams for capture-time lane continuation
  size_t cap_next = 0;
  // NUNET_STAMPS=1 diagnostic: a 1-thread kernel after every scheduled op writes the 100 MHz wall clock,
  // so the real timeline of an (unprofiled) hipGraph replay can be read back (tools/stamp_timeline.py)
  unsigned long long* stamps = nullptr;    // device, [2][STAMP_CAP]
  int lane_low_priority = 1;               // side lanes of the flag-synchronised program at the lowest stream priority (default 1)
  int calibrating = 0;                     // nunet_plan_calibrate: single lane + stamps, to measure every op's isolated cost
  std::map<std::string, float> op_cost[2]; // measured cost (us) by op name, per pass; empty: the built-in estimates
  hipStream_t seg_lanes[3] = {};           // side-lane streams of the segmented recording (created together: distinct hardware queues)
  std::vector<hipStream_t> seg_owned;      // every stream seg_pick_lanes created and kept (destroyed with the plan)
  struct Sched* open_sched = nullptr;      // backward pass left open after phase 1 (nunet_plan_backward_phase 1|8): lanes, dependency state
  std::vector<hipEvent_t> b0_events;       // ... and the last-writer events of the first bucket's gradients, for nunet_plan_bucket0_wait
  std::vector<std::string> stamp_labels[2];
  std::vector<nunet_plan_census_entry> census[2];   // nunet_plan_census_*: the convolutions / weight-gradient pairs of the last forward [0] / backward [1]
};
struct nunet_plan {
  nunet_plan_cfg cfg;
  int depth;                    // 0: the whole network; 1..4: pruned to the blocks x_{i,j}, i + j <= depth, that feed head `depth` (eval forward only)
  int es;                       // element size of T
  int hl[5], wl[5]; long long px[5];
  int nslots[5], PX[5];
  std::vector<Node> exec;       // execution order
  std::vector<int> reg;         // registration (parameter) order -> index into exec
  std::vector<Head> heads;
  long long nparams, nbnbuf; int nbn;
  int first_phase_nodes; long long gs_bucket0;   // backward phase 1 = heads + this many last nodes; its gradient-scratch prefix
  // arena regions (byte offsets)
  size_t off_fx, stats_floats;  // fixed-point per-channel sums: [BatchNorm statistics | BatchNorm-backward sums], zeroed by every training forward
  size_t off_gs, gs_floats;     // reduced gradient scratch (native layout, gradient-ready order): what a data-parallel job exchanges
  size_t off_slab; long long slab_floats;   // K-split slabs of the weight gradients (summed into the scratch by reduce_kernel)
  size_t off_save;
  size_t off_wpack; long long wpack_elems;
  size_t off_img;
  size_t X[5], GX[5];
  struct PlanRt* rt;
  size_t total;
  PackTab ptab;
  UnpackTab utab;
};

static size_t fx_region_bytes(const nunet_plan* P) { return P->stats_floats * NUNET_BN_SUM_REPLICAS * NUNET_FX_WORDS * sizeof(long long); }
static long long* fx_of(void* arena, const nunet_plan* P, int region, long long off) {   // region 0: BN statistics, 1: BN-backward sums
  return (long long*)((char*)arena + P->off_fx + (size_t)region * fx_region_bytes(P)) + off * NUNET_BN_SUM_REPLICAS * NUNET_FX_WORDS;
}
static inline char* AB(void* arena, size_t off) { return (char*)arena + off; }

#define CK(expr)                \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != NUNET_OK) return rc_; \
  } while (0)

// every plan entry that touches the arena checks what the caller says it owns against the plan's own layout
#define ARENA_CHECK(what) \
  NUNET_REQUIRE(arena_bytes >= P->total, what ": arena of %zu bytes, nunet_plan_arena_bytes() = %zu", (size_t)arena_bytes, P->total); \
  NUNET_REQUIRE(((uintptr_t)arena & 255) == 0, what ": arena must be 256-byte aligned")

// Entries of the training path on a pruned plan: refused before any launch and before any buffer is looked at
#define REFUSE_PRUNED(what) \
  NUNET_REQUIRE(P->depth == 0, what ": the plan is pruned to depth %d (nunet_plan_create_pruned): it runs eval forwards only", P->depth)

// ---- weights.hip, as the plan's creation and passes reach it -----------------------------------------------------------------
NUNET_INTERNAL void pack_tiles(PackTab& tab);                                                                      // fills the block -> tile prefix of a built table
NUNET_INTERNAL int plan_pack_weights(const nunet_plan* P, const float* params, void* arena, hipStream_t st);       // fp32 parameters -> the arena's packed layouts
NUNET_INTERNAL int plan_unpack_grads(nunet_plan* P, void* arena, float* grads, int accumulate, hipStream_t st);    // gradient scratch -> flat OIHW gradients
NUNET_INTERNAL int launch_reduce(nunet_plan* P, void* arena, int k_lo, int k_hi, hipStream_t st);                  // K-split slabs of exec nodes [k_lo, k_hi] -> scratch
