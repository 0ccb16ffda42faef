// sched.h — the lane scheduler of the plan's passes (sched.hip).
// ---------------------------------------------------------------------------
// Lane scheduler. The x_{i,j} grid has natural concurrency: blocks of level i depend only
// on levels i and i+-1, and weight gradients depend on nothing downstream. Every kernel
// here is latency-bound on its own (short contractions, grid-starved deep levels), so the
// plan issues every op on a stream of its own choosing - a block's ops on the block's lane
// (lane_of: the critical chain on lane 0, the side blocks on lanes 1-3 by anti-diagonal; a
// block's weight gradients on that same lane), or wherever the list scheduler (Sched::run_list)
// places them -, forked from and joined to the caller's stream with events. Exact RAW / WAW /
// WAR dependencies come from a per-buffer tracker (last-writer event, last-reader event per
// lane). Captured by the caller, the lanes become parallel branches of ONE hipGraph.
// ---------------------------------------------------------------------------
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <functional>
#include <initializer_list>

#include "plan.h"

// Resource ids of the tracker in numeric order, with what each range spans (B = NUNET_MAX_BLOCKS blocks)
#define NRES 512
enum {
  R_X = 0, R_GX = 25,                            // 5 levels x 5 slots each: block outputs (slot s of X_l: R_X + 5 l + s); their gradients
  R_BLK = 50,                                    // B x B_STRIDE: the forward buffers of a block (B_*)
  R_IMG = 230, R_LOGITS = 231, R_DLOGITS = 232,  // 1 each
  R_WP = 233,                                    // 5 levels: packed weights
  R_GSW = 240, R_GSV = 280,                      // B x 2 each (conv1, conv2): weight gradients; BatchNorm-backward sums + small-vector gradients
  R_GSH = 310,                                   // NUNET_MAX_HEADS: the gradients of a head
  R_LVL = 330,                                   // B x L_STRIDE: the backward scratch of a block (L_*)
  R_SK = 470                                     // B: split-K workspace
};
enum { B_Y1 = 0, B_Y2, B_UP, B_PIN, B_ST1, B_ST2, B_STRIDE = 8 };
enum { L_DY0 = 0, L_DY1, L_DA1, L_GUP, L_GPIN, L_STRIDE = 8 };
static_assert(B_ST2 < B_STRIDE && L_GPIN < L_STRIDE && R_X + 5 * 5 <= R_GX && R_GX + 5 * 5 <= R_BLK && R_BLK + NUNET_MAX_BLOCKS * B_STRIDE <= R_IMG &&
              R_IMG < R_LOGITS && R_LOGITS < R_DLOGITS && R_DLOGITS < R_WP && R_WP + 5 <= R_GSW && R_GSW + 2 * NUNET_MAX_BLOCKS <= R_GSV &&
              R_GSV + 2 * NUNET_MAX_BLOCKS <= R_GSH && R_GSH + NUNET_MAX_HEADS <= R_LVL && R_LVL + NUNET_MAX_BLOCKS * L_STRIDE <= R_SK &&
              R_SK + NUNET_MAX_BLOCKS <= NRES, "resource-id ranges overlap at this capacity");

// ---- Which cross-lane waits an op still needs -------------------------------------------------------------------------------
// Lanes are in-order (a stream; while capturing, a chain of streams each forked from the lane's tail), and what a kernel wrote
// is visible device-wide once it has ended (flag executor) - so "ends before" is transitive: an op that starts after
// op B has ended, where B started after A had ended, needs no wait of its own for A. Every issued op gets a stamp: its lane, its
// number on that lane, and the vector clock of its lane at that point - per lane, the number of the last op known to have ended
// before this one starts. A requested wait (read after write, write after write, write after read alike) whose producer the
// waiting lane's clock already covers is dropped; so is one that another wait of the same op covers; every wait that is kept
// merges the producer's clock into the lane's. Host bookkeeping only; nunet_wait_prune_host runs it over plain arrays.
#define WP_MAXL 16
static_assert(NLANES <= WP_MAXL, "the wait pruner's clocks cover every lane");
struct LaneStamp { int lane, seq; int clock[WP_MAXL]; };
struct NUNET_INTERNAL WaitPruner {
  int know[WP_MAXL][WP_MAXL], seq[WP_MAXL];
  void reset() { memset(know, 0, sizeof(know)); memset(seq, 0, sizeof(seq)); }
  void absorb(int L, const LaneStamp& s) { for (int l = 0; l < WP_MAXL; ++l) know[L][l] = std::max(know[L][l], s.clock[l]); }
  // the op about to start on lane L asks to wait for c[0..n): keep[q] = 1 for the waits it must make
  void decide(int L, const LaneStamp* const* c, int n, unsigned char* keep) {
    for (int q = 0; q < n; ++q) keep[q] = know[L][c[q]->lane] < c[q]->seq;
    for (int q = 0; q < n; ++q) {
      if (!keep[q]) continue;
      for (int r = 0; r < n && keep[q]; ++r) {
        if (r == q || !keep[r] || c[r]->clock[c[q]->lane] < c[q]->seq) continue;
        const bool same = c[r]->lane == c[q]->lane && c[r]->seq == c[q]->seq;   // the same op asked for twice: the first stays
        if (!same || r < q) keep[q] = 0;
      }
    }
    for (int q = 0; q < n; ++q) if (keep[q]) absorb(L, *c[q]);
  }
  LaneStamp done(int L) {        // the op on lane L has been issued
    LaneStamp s; s.lane = L; s.seq = ++seq[L]; know[L][L] = s.seq;
    memcpy(s.clock, know[L], sizeof(s.clock));
    return s;
  }
};

void graph_tag_tail(hipStream_t st, int lane);   // graph.hip: lane bookkeeping of an active nunet_graph capture

struct NUNET_INTERNAL Sched {
  hipStream_t main_s;
  WaitPruner wp; bool prune;                       // see above; prune off: every requested wait is made (nunet_plan_set_wait_prune)
  std::map<hipEvent_t, LaneStamp> stamp_of;        // the op each event of this pass marks the end of
  hipStream_t lane_s[NLANES];      // stream currently carrying each lane (fixed lanes when not capturing)
  hipEvent_t lane_tail[NLANES];    // event after the last op issued on the lane
  bool multi, capturing, failed;
  bool used[NLANES];
  PlanRt* rt;
  std::vector<hipEvent_t>* pool;
  size_t* pool_used;
  struct Res { hipEvent_t w_ev; hipStream_t w_st; hipEvent_t r_ev[NLANES]; hipStream_t r_st[NLANES]; };
  Res res[NRES];
  int cur_lane; int nreads, nwrites; int reads[16], writes[16];
  hipEvent_t fork_ev;
  hipEvent_t pend[64]; int npend;
  int lane_map[NLANES];
  int pass;
  char cur_name[32];
  void name(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(cur_name, sizeof(cur_name), fmt, ap); va_end(ap);
  }
  void stamp(hipStream_t st, int lane);

  hipEvent_t new_event() {
    if (*pool_used == pool->size()) {
      hipEvent_t e;
      (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
      pool->push_back(e);
    }
    return (*pool)[(*pool_used)++];
  }
  void init(PlanRt* rt, hipStream_t s, int pass);
  // One wait per distinct event, never on an event of the stream itself.
  void want(hipEvent_t ev, hipStream_t ev_st, hipStream_t st) {
    if (!ev) return;
    if (ev_st == st) { if (prune) wp.absorb(cur_lane, stamp_of[ev]); return; }   // (stream order: what that op knew, this one knows)
    for (int k = 0; k < npend; ++k) if (pend[k] == ev) return;
    if (npend < 64) pend[npend++] = ev;
    else failed = true;        // a dropped wait would be a silent race between lanes: reported by the caller after the join
  }
  // ROCm 7.2: inside a stream capture, a stream that waits on an event DESCENDING from its
  // own tail node crashes hipStreamEndCapture (regression test: tests/test_capture_gpu.py). The x_{i,j}
  // grid ping-pongs between levels all the time, so while capturing a lane with cross-lane
  // waits continues on a never-used stream that waits on the lane's tail event AND the
  // cross-lane events (no own tail -> plain fork semantics). Eager issue keeps fixed lanes.
  hipStream_t fresh_stream() {
    if (rt->cap_next >= rt->cap_streams.size()) { failed = true; return nullptr; }
    return rt->cap_streams[rt->cap_next++];
  }
  // stream waits / event records: real HIP calls, or instructions of the segmented program being recorded (graph.hip)
  static void wait_on(hipStream_t st, hipEvent_t ev) { if (!seg_wait(st, ev)) (void)hipStreamWaitEvent(st, ev, 0); }
  static void record_on(hipEvent_t ev, hipStream_t st) { if (!seg_record(ev, st)) (void)hipEventRecord(ev, st); }
  // begin an op on `lane` (already mapped) reading `rd` and writing `wr` resources; returns the stream to launch on
  hipStream_t begin_v(int lane, const int* rd, int nrd, const int* wr, int nwr);

  // ---- deferred ops: the backward pass collects its ops first (descriptors captured by value), then issues them
  struct Op { int lane, leaf; float cost; int nrd, nwr; int rd[12], wr[8]; char name[32]; std::function<int(hipStream_t)> fn; };
  std::vector<Op> ops;
  // launch census (nunet_diag.h): the geometry the launch's own host queries report for the descriptor handed to the scheduler
  void census_conv(const nunet_conv_desc& d);
  void census_wgrad(const nunet_wgrad_desc& a, const nunet_wgrad_desc& b);
  // a 3x3 convolution (forward or input gradient)
  void add_conv(int lane, std::initializer_list<int> rd, std::initializer_list<int> wr, const nunet_conv_desc& d, int alg_cin = 0) {
    census_conv(d);
    const double px = (double)d.N * d.H * d.W;
    add(lane, 0, 6.f + (float)(2.0 * 9 * (d.C0 + d.C1) * (d.D0 + d.D1) * px / 4e8), rd, wr, [d, alg_cin](hipStream_t ls) {
      g_prof_alg_cin = alg_cin; const int r = nunet_conv3x3_fwd(&d, ls); g_prof_alg_cin = 0; return r; });
  }
  void add(int lane, int leaf, float cost, std::initializer_list<int> rd, std::initializer_list<int> wr, std::function<int(hipStream_t)> fn) {
    add_v(lane, leaf, cost, rd.begin(), (int)rd.size(), wr.begin(), (int)wr.size(), std::move(fn));
  }
  void add_v(int lane, int leaf, float cost, const int* rd, int nrd, const int* wr, int nwr, std::function<int(hipStream_t)> fn);
  int issue(const int* order, const int* lane, int n);
  int run_ops();
  int run_list();
  bool list;                           // lanes assigned by a list scheduler over the dependency graph (run_list) instead of by block
  int run() { return (list && multi) ? run_list() : run_ops(); }
  void end();
  void join();
  // the end of a pass that is not left open: rejoin the caller's stream, then report what run() or the tracker could not do
  int finish(int rc, const char* what) {
    join();  // always rejoin the caller's stream (also on error: a capture must not be left forked)
    if (rc == NUNET_OK && failed) { nunet_set_error("%s: lane scheduler overflow (capture stream pool / dependency lists)", what); rc = NUNET_EINVAL; }
    return rc;
  }
};
