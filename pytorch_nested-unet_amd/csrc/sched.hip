// sched.hip — the lane scheduler (sched.h): the resource tracker that turns an op's read / write sets into stream waits, the
// wait pruner, the two ways of placing ops on lanes (by block; by a list schedule over the hazard DAG), and the measured
// choice of the flag-synchronised program's side-lane streams.
#include "sched.h"

__global__ void stamp_kernel(unsigned long long* p) { *p = wall_clock64(); }

extern "C" int nunet_debug_stamp(uint64_t* dst, nunet_stream_t s) {
  NUNET_REQUIRE(dst, "debug_stamp: null pointer");
  NUNET_LAUNCH(stamp_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, (unsigned long long*)dst);
  return nunet_check_launch("debug_stamp");
}

extern "C" int nunet_wait_prune_host(int32_t nlanes, int32_t nops, const int32_t* op_lane, const int32_t* edge_off, const int32_t* edge_src, uint8_t* keep) {
  NUNET_REQUIRE(op_lane && edge_off && keep && nlanes >= 1 && nlanes <= WP_MAXL && nops >= 0, "wait_prune_host: bad args (1..%d lanes)", WP_MAXL);
  WaitPruner wp; wp.reset();
  std::vector<LaneStamp> stamp((size_t)nops);
  std::vector<const LaneStamp*> c;
  for (int b = 0; b < nops; ++b) {
    const int L = op_lane[b], e0 = edge_off[b], e1 = edge_off[b + 1];
    NUNET_REQUIRE(L >= 0 && L < nlanes && e0 <= e1 && (e0 == e1 || edge_src), "wait_prune_host: op %d: lane %d, edges [%d, %d)", b, L, e0, e1);
    c.clear();
    for (int e = e0; e < e1; ++e) {
      NUNET_REQUIRE(edge_src[e] >= 0 && edge_src[e] < b, "wait_prune_host: edge %d of op %d names op %d, which is not issued before it", e, b, edge_src[e]);
      c.push_back(&stamp[edge_src[e]]);
    }
    if (!c.empty()) wp.decide(L, c.data(), (int)c.size(), keep + e0);
    stamp[b] = wp.done(L);
  }
  return NUNET_OK;
}

void Sched::stamp(hipStream_t st, int lane) {
  if (!rt->stamps) return;
  std::vector<std::string>& lab = rt->stamp_labels[pass];
  if ((int)lab.size() >= STAMP_CAP) return;
  NUNET_LAUNCH(stamp_kernel, dim3(1), dim3(1), 0, st, rt->stamps + (size_t)pass * STAMP_CAP + lab.size());
  char b[48]; snprintf(b, sizeof(b), "L%d %s", lane, cur_name);
  lab.push_back(b);
}

hipStream_t Sched::begin_v(int lane, const int* rd, int nrd, const int* wr, int nwr) {
  if (!multi) return main_s;
  cur_lane = lane; nreads = 0; nwrites = 0; npend = 0;
  hipStream_t st = lane_s[lane];      // may be null while capturing (lane not started yet)
  for (int q = 0; q < nrd; ++q) {
    const int r = rd[q];
    reads[nreads++] = r;
    Res& R = res[r];
    want(R.w_ev, R.w_st, st);
  }
  for (int q = 0; q < nwr; ++q) {
    const int w = wr[q];
    writes[nwrites++] = w;
    Res& R = res[w];
    want(R.w_ev, R.w_st, st);
    for (int l = 0; l < NLANES; ++l) want(R.r_ev[l], R.r_st[l], st);
  }
  if (prune && npend > 0) {
    const LaneStamp* c[64]; unsigned char keep[64];
    for (int k = 0; k < npend; ++k) c[k] = &stamp_of[pend[k]];
    wp.decide(lane, c, npend, keep);
    int m = 0;
    for (int k = 0; k < npend; ++k) if (keep[k]) pend[m++] = pend[k];
    npend = m;
  }
  if (capturing) {
    if (!used[lane] || npend > 0) {
      hipStream_t ns = fresh_stream();
      if (!ns) return main_s;   // pool exhausted: flagged, caller gets an error after the join
      if (used[lane] && lane_tail[lane]) (void)hipStreamWaitEvent(ns, lane_tail[lane], 0);
      else (void)hipStreamWaitEvent(ns, fork_ev, 0);
      st = ns; lane_s[lane] = ns; used[lane] = true;
    }
  } else if (!used[lane]) {
    used[lane] = true;
    if (st != main_s) wait_on(st, fork_ev);
  }
  for (int k = 0; k < npend; ++k) wait_on(st, pend[k]);
  seg_touch(st);                       // (segmented recording: the op's launches open / continue this stream's segment)
  return st;
}

void Sched::census_conv(const nunet_conv_desc& d) {
  nunet_plan_census_entry e; memset(&e, 0, sizeof(e));
  memcpy(e.label, cur_name, sizeof(e.label)); e.label[sizeof(e.label) - 1] = 0;
  e.kind = NUNET_CENSUS_CONV; e.N = d.N; e.H = d.H; e.W = d.W;
  e.C0 = d.C0; e.C1 = d.C1; e.D0 = d.D0; e.D1 = d.D1; e.in_tf = d.in_tf; e.has_bn_y = d.bn_y != nullptr; e.acc0_mask = d.acc0_mask;
  e.splitk_ws_floats = d.splitk_ws ? d.splitk_ws_floats : 0; e.has_tf_store = d.tf_store != nullptr;
  if (nunet_conv3x3_launch_info(&d, &e.conv) == NUNET_OK) rt->census[pass & 1].push_back(e);
}
void Sched::census_wgrad(const nunet_wgrad_desc& a, const nunet_wgrad_desc& b) {
  nunet_plan_census_entry e; memset(&e, 0, sizeof(e));
  memcpy(e.label, cur_name, sizeof(e.label)); e.label[sizeof(e.label) - 1] = 0;
  e.kind = NUNET_CENSUS_WGRAD_PAIR; e.N = a.N; e.H = a.H; e.W = a.W;
  e.wgrad_tf[0] = (a.x_tf ? 1 : 0) | (a.d_tf ? 2 : 0); e.wgrad_tf[1] = (b.x_tf ? 1 : 0) | (b.d_tf ? 2 : 0);
  if (nunet_conv3x3_wgrad_launch_info(&a, &e.wgrad[0]) == NUNET_OK && nunet_conv3x3_wgrad_launch_info(&b, &e.wgrad[1]) == NUNET_OK)
    rt->census[pass & 1].push_back(e);
}

void Sched::add_v(int lane, int leaf, float cost, const int* rd, int nrd, const int* wr, int nwr, std::function<int(hipStream_t)> fn) {
  Op o; o.lane = lane_map[lane]; o.leaf = leaf; o.cost = cost; o.nrd = o.nwr = 0;
  for (int q = 0; q < nrd; ++q) if (rd[q] >= 0) { if (o.nrd < 12) o.rd[o.nrd++] = rd[q]; else failed = true; }
  for (int q = 0; q < nwr; ++q) if (wr[q] >= 0) { if (o.nwr < 8) o.wr[o.nwr++] = wr[q]; else failed = true; }
  memcpy(o.name, cur_name, sizeof(o.name)); cur_name[0] = 0;
  // the op's isolated cost as nunet_plan_calibrate measured it (by name), instead of the built-in estimate
  const std::map<std::string, float>& m = rt->op_cost[pass & 1];
  const auto it = o.name[0] ? m.find(o.name) : m.end();
  if (it != m.end()) o.cost = it->second;
  o.fn = std::move(fn);
  ops.push_back(std::move(o));
}

void Sched::end() {
  if (!multi) { stamp(main_s, 0); cur_name[0] = 0; return; }
  hipStream_t st = lane_s[cur_lane];
  if (!st) return;
  stamp(st, cur_lane); cur_name[0] = 0;
  if (capturing) graph_tag_tail(st, cur_lane);
  hipEvent_t ev = new_event();
  record_on(ev, st);
  stamp_of[ev] = wp.done(cur_lane);
  lane_tail[cur_lane] = ev;
  for (int k = 0; k < nreads; ++k) { res[reads[k]].r_ev[cur_lane] = ev; res[reads[k]].r_st[cur_lane] = st; }
  for (int k = 0; k < nwrites; ++k) {
    Res& R = res[writes[k]];
    R.w_ev = ev; R.w_st = st;
    for (int l = 0; l < NLANES; ++l) { R.r_ev[l] = nullptr; R.r_st[l] = nullptr; }
  }
}

void Sched::join() {
  if (!multi) return;
  for (int l = 0; l < NLANES; ++l)
    if (used[l] && lane_tail[l] && lane_s[l] != main_s) wait_on(main_s, lane_tail[l]);
  seg_touch(main_s);                   // what the caller launches next on its stream opens a new segment
}

// Side-lane streams of the segmented program. ROCm maps every stream onto one of 4 hardware queues at creation and offers no way
// to ask which (tools/seg_overlap_probe.py: of 8 fresh streams some pairs share a queue, and two lanes that share a queue run
// strictly one after the other). So the lanes are CHOSEN BY MEASUREMENT: a 100 us single-workgroup spin kernel on two streams at
// once takes 100 us when they sit on different queues and 200 us when not. Three candidates that overlap with the caller's
// stream and with each other become lanes 1-3 (the rest are destroyed). Called outside any capture, once per plan.
int nunet_debug_spin(int32_t us, int32_t tag, nunet_stream_t s);
static void seg_pick_lanes(PlanRt* rt, hipStream_t main_s) {
  const int NC = 12, SPIN_US = 100;
  hipStream_t cand[NC];
  int nc = 0;
  // the side lanes get the LOWEST stream priority: the chain lane's workgroups are dispatched ahead of theirs (+1.4 % on the
  // flag-synchronised step) - unless the caller says otherwise (nunet_plan_set_lane_priority): with RCCL's high-priority stream in
  // the process, lowest-priority lanes are served in time slices (every kernel on one of them took 100-190 us in the
  // data-parallel rehearsal: 3.4-4.4 ms per step against 1.82 at default priority).
  const int side_prio = rt->lane_low_priority;
  int pr_least = 0, pr_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
  // (measured and not kept: side lanes on CU-masked streams - hipExtStreamCreateWithCUMask, 16 to 96 CUs kept free for the chain -
  //  and the chain on a high-priority stream both run the step at 5.3 ms instead of 1.85)
  for (int k = 0; k < NC; ++k) {
    const hipError_t ce = side_prio ? hipStreamCreateWithPriority(&cand[nc], hipStreamNonBlocking, pr_least) : hipStreamCreateWithFlags(&cand[nc], hipStreamNonBlocking);
    if (ce == hipSuccess) ++nc; else (void)hipGetLastError();
  }
  hipEvent_t e0 = nullptr, e1 = nullptr, eb = nullptr;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventCreateWithFlags(&eb, hipEventDisableTiming);
  auto overlap = [&](hipStream_t a, hipStream_t b) {          // true: a and b run side by side
    (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
    (void)hipEventRecord(e0, a);
    (void)nunet_debug_spin(SPIN_US, 1, a);
    (void)nunet_debug_spin(SPIN_US, 1, b);
    (void)hipEventRecord(eb, b);
    (void)hipStreamWaitEvent(a, eb, 0);
    (void)hipEventRecord(e1, a);
    (void)hipStreamSynchronize(a);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { (void)hipGetLastError(); return false; }
    return ms * 1000.f < 1.5f * SPIN_US;
  };
  // A lane must also DISPATCH at the caller's stream's rate: with RCCL initialised in the process, some streams sit on queues that
  // the hardware scheduler serves in time slices - every kernel on such a lane took 100-190 us in the data-parallel rehearsal
  // (4.1 ms per step). Eight back-to-back 2 us kernels, timed on the candidate against the same on the caller's stream.
  auto chain_us = [&](hipStream_t a) {
    (void)hipStreamSynchronize(a);
    (void)nunet_debug_spin(2, 1, a);
    (void)hipEventRecord(e0, a);
    for (int q = 0; q < 8; ++q) (void)nunet_debug_spin(2, 1, a);
    (void)hipEventRecord(e1, a);
    (void)hipStreamSynchronize(a);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { (void)hipGetLastError(); return 1e9f; }
    return ms * 1000.f;
  };
  const float base_us = std::min(chain_us(main_s), chain_us(main_s));
  hipStream_t pick[3]; int np = 0;
  bool usedc[NC] = {false};
  for (int k = 0; k < nc && np < 3; ++k) {
    // (also clear of the process's default stream: the copies of the next batch are usually queued there)
    bool ok = overlap(main_s, cand[k]) && overlap((hipStream_t)nullptr, cand[k]);
    if (ok) { const float c_us = std::min(chain_us(cand[k]), chain_us(cand[k])); ok = c_us < 2.5f * base_us + 20.f; }
    for (int q = 0; q < np && ok; ++q) ok = overlap(pick[q], cand[k]);
    if (ok) { pick[np++] = cand[k]; usedc[k] = true; }
  }
  for (int k = 0; k < nc; ++k) { if (!usedc[k]) (void)hipStreamDestroy(cand[k]); else rt->seg_owned.push_back(cand[k]); }
  // (fewer than three distinct queues found: lanes share a STREAM - never two streams of one queue, which the flag-synchronised
  //  program could not survive: a polling kernel ahead of its signal in the same queue)
  for (int q = 0; q < 3; ++q) rt->seg_lanes[q] = q < np ? pick[q] : (np > 0 ? pick[q % np] : main_s);
  if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); if (eb) (void)hipEventDestroy(eb);
}

void Sched::init(PlanRt* rt_, hipStream_t s, int pass_) {
  const int pass = pass_;
  this->pass = pass_;
  cur_name[0] = 0;
  rt = rt_;
  main_s = s;
  {
    static int want_stamps = -1;
    if (want_stamps < 0) { const char* e = getenv("NUNET_STAMPS"); want_stamps = e ? atoi(e) : 0; }
    hipStreamCaptureStatus cs0 = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cs0);
    if (want_stamps && !rt->stamps && cs0 != hipStreamCaptureStatusActive) {
      if (hipMalloc((void**)&rt->stamps, 2 * STAMP_CAP * sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); rt->stamps = nullptr; }
    }
    rt->stamp_labels[pass].clear();
    rt->census[pass].clear();
    if (rt->stamps) { snprintf(cur_name, sizeof(cur_name), "start"); stamp(s, 0); cur_name[0] = 0; }
  }
  multi = rt->multistream != 0 && rt->lanes_ok && !rt->calibrating;
  list = rt->schedule == NUNET_SCHEDULE_LIST && !rt->calibrating;
  failed = false;
  capturing = false;
  prune = rt->wait_prune != 0; wp.reset(); stamp_of.clear();
  pool = &rt->events[pass]; pool_used = &rt->events_used[pass];
  *pool_used = 0;
  memset(res, 0, sizeof(res));
  cur_lane = 0; nreads = nwrites = 0; npend = 0;
  fork_ev = nullptr;
  if (multi) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive) capturing = true;
    else (void)hipGetLastError();
    if (seg_active()) capturing = false;   // segmented recording: fixed lanes on real streams (the caller's stream is merely inside a segment)
    if (!capturing && rt->cap_streams.empty()) {
      // pool for later captures, created outside any capture (warm-up passes run eagerly first)
      for (int k = 0; k < 320; ++k) {
        hipStream_t q;
        if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
        rt->cap_streams.push_back(q);
      }
    }
    if (capturing && (rt->cap_streams.empty())) multi = false;     // never warmed up eagerly: stay on one stream
    if (capturing && pass == 0) rt->cap_next = 0;                   // forward + backward of one capture share the pool
  }
  // lane of (level 0..4, weight gradients of level 0..4): one lane per pyramid level, weight gradients on their
  // block's lane (measured best on MI355X: separate weight-gradient lanes add cross-queue edges that cost more than the
  // overlap they buy; the exception is the deferral of the shallow chain blocks' weight gradients, see the backward pass)
  for (int l = 0; l < NLANES; ++l) { lane_map[l] = l % 5; lane_s[l] = capturing ? nullptr : rt->lanes[l]; used[l] = false; lane_tail[l] = nullptr; }
  if (multi && seg_active()) {
    // four real streams = ROCm's four hardware queues: the critical chain (lane 0) runs on the caller's stream itself - no
    // fork / join edge on the chain -, the side lanes on three streams of the plan's, the deferred weight gradients share lane 3's
    lane_s[0] = main_s; used[0] = true;
    if (!rt->seg_lanes[0]) {
      // (the dry pass of a recording comes first and captures nothing: the only moment the calibration kernels may run on `s`)
      hipStreamCaptureStatus cs2 = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(main_s, &cs2);
      if (cs2 != hipStreamCaptureStatusActive) { const bool keep = g_dry_run; g_dry_run = false; seg_pick_lanes(rt, main_s); g_dry_run = keep; }
      else for (int q = 0; q < 3; ++q) rt->seg_lanes[q] = rt->lanes[q + 1];
    }
    for (int q = 0; q < 3; ++q) lane_s[q + 1] = rt->seg_lanes[q];
    // (the deferred weight gradients of the chain blocks go to the stream of lane 1: its own block, x0_1, is the LAST of the
    //  level-0 row's backward chain B04 -> B03 -> B02 -> B01, so that stream idles for the first 500 us of the backward pass; on
    //  lane 3's stream they sat in front of B03 and held the whole row back by 280 us)
    lane_s[4] = lane_s[1];
  }
  if (multi) {
    fork_ev = new_event();
    record_on(fork_ev, main_s);
    if (capturing) graph_tag_tail(main_s, -1);   // launches made so far on the caller's stream are not ours to place
  }
}

// Issue the collected ops: op order[q] on lane lane[order[q]], for q = 0 .. n-1; stops at the first launch that fails.
int Sched::issue(const int* order, const int* lane, int n) {
  int rc = NUNET_OK;
  for (int q = 0; q < n && rc == NUNET_OK; ++q) {
    Op& o = ops[order[q]];
    hipStream_t st = begin_v(lane[order[q]], o.rd, o.nrd, o.wr, o.nwr);
    rc = o.fn(st);
    memcpy(cur_name, o.name, sizeof(cur_name));
    end();
  }
  ops.clear();
  return rc;
}

int Sched::run_ops() {
  // ops are issued in program order, each on its block's lane (a simulated list schedule and a rewrite of the captured graph's
  // edge order were both measured slower than the plain capture order on ROCm 7.2, see DESIGN.md, and are not kept)
  const int n = (int)ops.size();
  std::vector<int> order(n), lane(n);
  for (int i = 0; i < n; ++i) { order[i] = i; lane[i] = ops[i].lane; }
  return issue(order.data(), lane.data(), n);
}

// ---- the list schedule's two pure parts (nunet_list_schedule_host runs them over plain arrays) --------------------------------
namespace {
struct OpRW { const int* rd; int nrd; const int* wr; int nwr; };        // what an op reads and writes, as resource ids
struct Dag { std::vector<std::vector<int>> succ, pred; };
struct ListSchedule { std::vector<int> order, lane; std::vector<float> tend; float critical; };   // issue order; lane and simulated end by op
}

// The hazards of the program order (read after write, write after write, write after read) as the edges of a DAG
static Dag hazard_dag(const std::vector<OpRW>& ops) {
  const int n = (int)ops.size();
  Dag g; g.succ.resize(n); g.pred.resize(n);
  std::vector<int> lastw(NRES, -1);
  std::vector<std::vector<int>> readers(NRES);
  auto edge = [&](int a, int b) { if (a >= 0 && a != b && std::find(g.succ[a].begin(), g.succ[a].end(), b) == g.succ[a].end()) { g.succ[a].push_back(b); g.pred[b].push_back(a); } };
  for (int i = 0; i < n; ++i) {
    const OpRW& o = ops[i];
    for (int q = 0; q < o.nrd; ++q) edge(lastw[o.rd[q]], i);
    for (int q = 0; q < o.nwr; ++q) { edge(lastw[o.wr[q]], i); for (int r : readers[o.wr[q]]) edge(r, i); }
    for (int q = 0; q < o.nrd; ++q) readers[o.rd[q]].push_back(i);
    for (int q = 0; q < o.nwr; ++q) { lastw[o.wr[q]] = i; readers[o.wr[q]].clear(); }
  }
  return g;
}

// Lane and issue order of every op from the costs and the DAG alone; false: a dependency cycle (order holds the ops placed)
static bool list_schedule(const float* cost, const Dag& g, ListSchedule& ls) {
  const int n = (int)g.succ.size();
  const std::vector<std::vector<int>>&succ = g.succ, &pred = g.pred;
  // three lanes: measured on MI355X (96x96 bs16, flag-synchronised lanes) 2 / 3 / 4 lanes = 8640 / 9270 / 8950 images/s - the fourth
  // concurrent stream costs the critical chain more than its overlap buys; limiting the summed chip share of the concurrent ops
  // instead (a capacity model over the launch grids) only lost: 1.5 / 2.0 / 2.5 / 3.0 full-chip ops at once = 6610 / 8480 / 8720 /
  // 9260. A crossing dependency costs one sync kernel on each side (XSYNC; 0 / 3 / 10 us in the model: no difference).
  constexpr int NL = 3; constexpr float XSYNC = 3.f;
  std::vector<int> indeg(n, 0);
  for (int i = 0; i < n; ++i) indeg[i] = (int)pred[i].size();
  std::vector<float> prio(n, 0.f);
  std::vector<float>& tend = ls.tend; tend.assign(n, 0.f);
  for (int i = n - 1; i >= 0; --i) { float m = 0.f; for (int s : succ[i]) m = std::max(m, prio[s]); prio[i] = cost[i] + m; }
  // (measured, no effect or worse: a priority bias for the weight gradients (-100 / 0: the same, +300 us: -3 %), the cost of the
  //  grid-starved levels 2-4 scaled by 1.5 / 2 / 3 as a model of their in-step inflation (-0.5 / -2 / -2 %): the isolated costs
  //  schedule best)
  std::vector<int> ready, order;
  std::vector<int>& lane = ls.lane; lane.assign(n, 0);
  float lane_free[NL] = {0.f, 0.f, 0.f};
  for (int i = 0; i < n; ++i) if (indeg[i] == 0) ready.push_back(i);
  // event-driven: the lane that falls idle first takes the most urgent op that could start on it by then; when nothing could, the
  // lane's clock moves on to the next moment something can (so leaf work fills the holes of a lane instead of queueing at its end)
  auto est = [&](int p, int l) { float t = 0.f; for (int q : pred[p]) t = std::max(t, tend[q] + (lane[q] != l ? XSYNC : 0.f)); return t; };
  int guard = 0;
  while (!ready.empty() && guard++ < 100000) {
    int l = 0;
    for (int k = 1; k < NL; ++k) if (lane_free[k] < lane_free[l]) l = k;
    const float T = lane_free[l];
    int best = -1;
    for (int q = 0; q < (int)ready.size(); ++q) {
      if (est(ready[q], l) > T + 0.01f) continue;
      if (best < 0 || prio[ready[q]] > prio[ready[best]] || (prio[ready[q]] == prio[ready[best]] && ready[q] < ready[best])) best = q;
    }
    if (best < 0) {
      // nothing can start on this lane yet: wait for the earliest of (an op becoming startable here, another lane falling idle)
      float nt = 1e30f;
      for (int q : ready) nt = std::min(nt, est(q, l));
      for (int k = 0; k < NL; ++k) if (k != l && lane_free[k] > T) nt = std::min(nt, lane_free[k]);
      lane_free[l] = nt > T ? nt : T + 0.5f;
      continue;
    }
    const int p = ready[best];
    ready.erase(ready.begin() + best);
    lane[p] = l; tend[p] = T + cost[p]; lane_free[l] = tend[p];
    order.push_back(p);
    for (int s2 : succ[p]) if (--indeg[s2] == 0) ready.push_back(s2);
  }
  ls.critical = n ? prio[0] : 0.f;
  ls.order = order;
  if ((int)order.size() != n) return false;
  // issue in simulated start order (stable: a topological order of the hazard DAG)
  std::stable_sort(ls.order.begin(), ls.order.end(), [&](int a, int b) { return tend[a] - cost[a] < tend[b] - cost[b]; });
  // (the sort by start time keeps predecessors first: a successor starts at or after its predecessor's end)
  return true;
}

extern "C" int nunet_list_schedule_host(int32_t nops, const float* cost, const int32_t* rd_off, const int32_t* rd, const int32_t* wr_off, const int32_t* wr,
                                        int32_t* order, int32_t* lane) {
  NUNET_REQUIRE(nops >= 0 && cost && rd_off && wr_off && order && lane, "list_schedule_host: null pointer or negative op count");
  NUNET_REQUIRE(rd_off[0] >= 0 && wr_off[0] >= 0, "list_schedule_host: negative offset");
  std::vector<OpRW> ops((size_t)nops);
  for (int i = 0; i < nops; ++i) {
    const int nrd = rd_off[i + 1] - rd_off[i], nwr = wr_off[i + 1] - wr_off[i];
    NUNET_REQUIRE(nrd >= 0 && nwr >= 0, "list_schedule_host: op %d: offsets are not monotonic", i);
    NUNET_REQUIRE(nrd <= 12 && nwr <= 8, "list_schedule_host: op %d: %d reads / %d writes, an op holds 12 / 8", i, nrd, nwr);
    NUNET_REQUIRE((nrd == 0 || rd) && (nwr == 0 || wr), "list_schedule_host: op %d: null id array", i);
    ops[i] = {rd + rd_off[i], nrd, wr + wr_off[i], nwr};
    for (int q = 0; q < nrd + nwr; ++q) {
      const int r = q < nrd ? ops[i].rd[q] : ops[i].wr[q - nrd];
      NUNET_REQUIRE(r >= 0 && r < NRES, "list_schedule_host: op %d names resource %d, ids are 0..%d", i, r, NRES - 1);
    }
  }
  ListSchedule ls;
  NUNET_REQUIRE(list_schedule(cost, hazard_dag(ops), ls), "list_schedule_host: placed %d of %d ops (dependency cycle)", (int)ls.order.size(), nops);
  std::copy(ls.order.begin(), ls.order.end(), order);
  std::copy(ls.lane.begin(), ls.lane.end(), lane);
  return NUNET_OK;
}

// List schedule: the lane of every op is CHOSEN here instead of following its block. The hazards of the program order (read after
// write, write after write - the accumulation order into the shared gradient slots -, write after read) are the edges of a DAG;
// ops are taken by critical-path priority (cost + longest path to the end) and each goes to the lane on which it can start
// earliest in a simulation with the ops' cost estimates (a dependency that crosses lanes costs XSYNC), then issued in simulated
// start order. Any topological order of that DAG keeps every conflicting pair in program order, so the resource tracker sees
// the same hazards and the results are bit-identical to the block-lane schedule (tests assert it). Meant for lanes that are
// real in-order streams (the flag-synchronised program), where the issue order on a lane IS its execution order: the
// block-lane order put leaf work (weight gradients) in front of critical ops of the same lane.
int Sched::run_list() {
  const int n = (int)ops.size();
  std::vector<OpRW> rw(n);
  std::vector<float> cost(n);
  for (int i = 0; i < n; ++i) { rw[i] = {ops[i].rd, ops[i].nrd, ops[i].wr, ops[i].nwr}; cost[i] = ops[i].cost; }
  ListSchedule ls;
  if (!list_schedule(cost.data(), hazard_dag(rw), ls)) { nunet_set_error("plan: list schedule placed %d of %d ops (dependency cycle)", (int)ls.order.size(), n); ops.clear(); return NUNET_EINVAL; }
  const std::vector<int>&idx = ls.order, &lane = ls.lane;
  const std::vector<float>& tend = ls.tend;
  {
    static int dbg = -1;
    if (dbg < 0) { const char* e = getenv("NUNET_LIST_DEBUG"); dbg = e ? atoi(e) : 0; }
    if (dbg && !g_dry_run) {
      float mk = 0.f; for (int i = 0; i < n; ++i) mk = std::max(mk, tend[i]);
      fprintf(stderr, "list schedule pass %d: %d ops, simulated makespan %.1f us, critical path %.1f us%s\n", pass, n, mk, ls.critical, rt->op_cost[pass & 1].empty() ? " (built-in costs)" : " (measured costs)");
      if (dbg > 1) for (int i : idx) fprintf(stderr, "  %8.1f %6.1f  L%d %s\n", tend[i] - ops[i].cost, ops[i].cost, lane[i], ops[i].name);
    }
  }
  return issue(idx.data(), lane.data(), n);
}
