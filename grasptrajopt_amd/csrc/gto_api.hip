// gto_api.hip — host side of libgto_hip.so: the C ABI declared in include/gto_solver.h.
// Owns all device memory behind the opaque handle; no torch, no CPU fallback.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include <sys/prctl.h>

#include "gto_kernels.h"
#include "gto_depth.h"
#include "gto_cloud.h"
#include "gto_retime.h"
#include "gto_dynamics.h"
#include "gto_forward.h"
#include "gto_observe.h"
#include "gto_held.h"
#include "gto_seed.h"
#include "gto_retrieve.h"
#include "gto_occupancy.h"
#include "gto_selfcheck.h"
#include "gto_selfpairs.h"
#include "gto_heldclear.h"
#include "gto_heldargs.h"
#include "gto_owned.h"
#include "gto_robot.h"

#define GTO_VERSION GTO_ABI_VERSION  // include/gto_solver.h
#ifndef GTO_OBS_DEEP_PD
#define GTO_OBS_DEEP_PD 8
#endif

static std::string g_create_error;

#define GTO_SWEEP_WGS 64   // workgroups of the crew behind an itemized obstacle launch laid out over an estimate (launch_obstacle)

#define GTO_MAX_LANES 8  // lanes of one solve call (streams, list sets, progress words)
#define GTO_BASE_PIN_SLOTS 4  // calls whose small host arrays (n_goals, per-plan bases, the filter's view table) may be in flight at once without the host waiting
#define GTO_STAGE_SLOTS 10  // host arrays of each direction that one host-pointer entry point stages (Staging): gto_track_rollout has ten inputs
#define GTO_NAP_US 50      // the throttle's naps (the host thread of a lane sleep-polls two pinned words); 10-50 us change nothing
#define GTO_NAP_FEW_US 10  // ... in launches with few instances in flight; 50-200 us change nothing either
// the deep-gather obstacle variant only up to this many instances in flight (two workgroups per CU: beyond that the
// five-per-CU variant gets through a launch faster)
#define GTO_OBS_DEEP_MAX 32

// Every knob a GTO_* environment variable sets, with its default.  read_tunables fills it once per handle, in gto_create.
struct Tunables {
  int ahead = 8;           // GTO_AHEAD: rounds the host may enqueue beyond the last one it has seen running
  int ahead_few = 4;       // ... in launches with few instances in flight (short rounds: four of them cover the host's launch time, and every round enqueued beyond the last instance's end runs empty)
  // speculation (gto_kernels.h GTO_KSPEC): candidates a step generates ahead of their evaluation in launches with few
  // instances in flight (more work, fewer dependent rounds).  Every candidate is a job of the next obstacle launch, and
  // that launch stays one wave of workgroups up to about `spec_jobs` jobs: with n instances in flight a step hands out
  // up to spec_jobs / n candidates (at most spec_acc after an accepted evaluation, spec_rej after a round without one);
  // beyond that, after a rejection only, spec_rej_few while at most spec_few are in flight.  spec_deep caps n for the
  // candidates after an accepted evaluation.
  int spec_rej = 4, spec_acc = 4, spec_deep = 32;  // GTO_SPEC_REJ, GTO_SPEC_ACC, GTO_SPEC_DEEP
  int spec_rej_few = 2, spec_jobs = 20;            // GTO_SPEC_REJ_FEW, GTO_SPEC_JOBS
  int spec_streak = 4;  // GTO_SPEC_STREAK: first candidate accepted this many rounds in a row -> one candidate after the next accepted evaluation (0: off)
  // The tail of a LARGE call (more than spec_deep instances from the start) shares the GPU with the other lanes' launches,
  // and there an evaluation that turns out not to be needed costs more than the round it might save: fewer candidates
  // after an accepted evaluation, the single candidate after a shorter run of first-try accepts, three waypoints per
  // obstacle workgroup (GTO_SPEC_ACC_TAIL, GTO_SPEC_STREAK_TAIL, GTO_OBS_TG_FEW_TAIL; the driver's 20-step call 253 -> 262 k).
  // A call that is small from its first round (one grasp, a batch of a few) is alone on the GPU and keeps the settings
  // that give the shortest chain of rounds (one instance: 0.66 ms; with the tail's settings 0.90 ms).
  int spec_acc_tail = 2, spec_streak_tail = 2, obs_tg_few_tail = 3;
  int spec_few = 64;  // GTO_SPEC_FEW: speculation starts once at most this many instances are in flight: before that the GPU is full and every extra evaluation costs time
  int obs_deep = 1;   // GTO_OBS_DEEP: launches with few instances in flight use the obstacle kernel variant with deep gather batches
  int dbg_cut = 0;    // GTO_DEBUG_CUT: cut the obstacle kernel short after a phase (timing experiments: results are garbage)
  int dist_relax = 0;  // GTO_DIST_RELAX: build the distance fields by relaxation sweeps instead of the separable passes
  // GTO_OBS_INTERLEAVE: waypoints of an obstacle workgroup nG apart instead of consecutive, so that the waypoints next to
  // the obstacles (neighbours in time) land in different workgroups: 0 never, 1 always, 2 (default) in launches with few
  // instances in flight, where the longest workgroup decides the round (+5 % for one batch at a time, -2 % at saturation)
  int obs_interleave = 2;
  int static_pos = 1;  // GTO_STATIC_POS=0: every instance draws its list positions from the counters in every round
  int pb_merge = 4;  // GTO_PB_MERGE: chunks of a link under one sphere of the step kernel's broad phase
  int prebroad = 1;  // GTO_PREBROAD=0: every (job, group) gets a workgroup of the obstacle kernel in every round
  int seed_pb = 1;   // GTO_SEED_PB=0: nothing is known about the seed of an instance that takes over a slot, and every group of it is listed (k_seed_broad)
  int seed_pb_all = 1;  // GTO_SEED_PB_ALL=0: the seeds that start in a slot are not tested, and round 0's obstacle launch looks at every group of them
  // GTO_INIT_DEDUP=0: every instance of a solve call runs the init pass itself.  Otherwise the init pass of a call runs once per
  // run of equal start states (k_init_heads, k_ss_fixed_spread) when it is more than init_dedup_min workgroups
  // (GTO_INIT_DEDUP_MIN; four per instance): up to one wave of workgroups, 1280, the two small launches cost more than they save
  int init_dedup = 1, init_dedup_min = 1280;
  double pb_min_gain = 0.10;  // GTO_PB_MIN_GAIN: a call whose step-kernel broad phase settles less than this share of the groups stops running it
  int obs_tg = 3;  // GTO_OBS_TG: waypoints per workgroup of the obstacle kernel: they share the table staging, the FK barriers and the launch overhead
  int obs_tg_few = 2;  // GTO_OBS_TG_FEW: ... when few instances are in flight (one small batch, the tail of a call): lower latency per round; results do not depend on the group size
  int obs_tg_wide = 5;  // GTO_OBS_TG_WIDE: ... for the wide robots (gto_create)
  bool obs_tg_given = false;  // GTO_OBS_TG was set: it is the group size of every robot, the wide ones included
  int few_instances = 192;  // GTO_FEW_INSTANCES: launches with at most this many instances in flight count as few
  int step_nw_few = 8;  // GTO_STEP_NW_FEW: wavefronts per workgroup of the step kernel in launches with few instances in flight (4 or 8)
  int step_texact = 1;  // GTO_STEP_TEXACT=0: no kernel compiled for one trajectory length: at T = GTO_STEP_T_EXACT the choice GTO_STEP_TCLASS makes (tests, A/B runs; same results)
  int step_tclass = 1;  // GTO_STEP_TCLASS=0: the narrow step kernels' 96-waypoint instantiation at every T (tests, A/B runs; same results)
  int slots = 512;  // GTO_SLOTS: instances in flight per lane of a solve call; a finished instance hands its slot to the next one
  // lanes of a solve call (gto_solve_batch_device): at most lanes_max, each with at least lane_min instances; a lane with
  // at most adopt_below instances left hands them to lane 0 (0: never).  gto_set_lanes / GTO_LANES, GTO_LANE_MIN, GTO_ADOPT
  int lanes_max = 1, lane_min = 256, adopt_below = 0;
  int item_hint_forced = 0;  // GTO_ITEM_HINT: the estimate itself (tests of the crew)
  int item_grid = 1;  // GTO_ITEM_GRID=0: itemized launches laid out over the upper bound of their item lists
  bool debug_timing = false;  // GTO_DEBUG_TIMING: phase stamps of the kernels on stderr after every solve call
  bool lane_debug = false;    // GTO_LANE_DEBUG: host-side stamps of a call with lanes on stderr
};

// One row per variable, in the order they are applied: a row may also set up to two more fields (GTO_AHEAD sets both
// aheads, GTO_OBS_TG all three group sizes ...), and a later row overrides them.  Values are clamped to [lo, hi]; a [0, 1]
// row is a switch that any non-zero value turns on.
static void read_tunables(Tunables& t) {
  using F = int Tunables::*;
  struct Row { const char* name; F f, also1, also2; int lo, hi; };
  const int BIG = INT_MAX;
  static const Row rows[] = {
      {"GTO_AHEAD", &Tunables::ahead, &Tunables::ahead_few, nullptr, 1, BIG},
      {"GTO_SPEC_REJ", &Tunables::spec_rej, nullptr, nullptr, 1, GTO_KSPEC},
      {"GTO_SPEC_REJ_FEW", &Tunables::spec_rej_few, nullptr, nullptr, 1, GTO_KSPEC},
      {"GTO_SPEC_STREAK", &Tunables::spec_streak, &Tunables::spec_streak_tail, nullptr, 0, BIG},
      {"GTO_SPEC_STREAK_TAIL", &Tunables::spec_streak_tail, nullptr, nullptr, 0, BIG},
      {"GTO_SPEC_JOBS", &Tunables::spec_jobs, nullptr, nullptr, 1, BIG},
      {"GTO_SPEC_ACC", &Tunables::spec_acc, &Tunables::spec_acc_tail, nullptr, 1, GTO_KSPEC},
      {"GTO_SPEC_ACC_TAIL", &Tunables::spec_acc_tail, nullptr, nullptr, 1, GTO_KSPEC},
      {"GTO_SPEC_DEEP", &Tunables::spec_deep, nullptr, nullptr, 0, BIG},
      {"GTO_SPEC_FEW", &Tunables::spec_few, nullptr, nullptr, 0, BIG},
      {"GTO_OBS_DEEP", &Tunables::obs_deep, nullptr, nullptr, 0, 1},
      {"GTO_PREBROAD", &Tunables::prebroad, nullptr, nullptr, 0, 1},
      {"GTO_SEED_PB", &Tunables::seed_pb, nullptr, nullptr, 0, 1},
      {"GTO_SEED_PB_ALL", &Tunables::seed_pb_all, nullptr, nullptr, 0, 1},
      {"GTO_INIT_DEDUP", &Tunables::init_dedup, nullptr, nullptr, 0, 1},
      {"GTO_INIT_DEDUP_MIN", &Tunables::init_dedup_min, nullptr, nullptr, 0, BIG},
      {"GTO_PB_MERGE", &Tunables::pb_merge, nullptr, nullptr, 1, BIG},
      {"GTO_STATIC_POS", &Tunables::static_pos, nullptr, nullptr, 0, 1},
      {"GTO_OBS_INTERLEAVE", &Tunables::obs_interleave, nullptr, nullptr, 0, 2},
      {"GTO_DIST_RELAX", &Tunables::dist_relax, nullptr, nullptr, 0, 1},
      {"GTO_DEBUG_CUT", &Tunables::dbg_cut, nullptr, nullptr, INT_MIN, INT_MAX},
      {"GTO_ITEM_GRID", &Tunables::item_grid, nullptr, nullptr, 0, 1},
      {"GTO_ITEM_HINT", &Tunables::item_hint_forced, nullptr, nullptr, 0, BIG},
      {"GTO_SLOTS", &Tunables::slots, nullptr, nullptr, 1, BIG},
      {"GTO_LANES", &Tunables::lanes_max, nullptr, nullptr, 1, GTO_MAX_LANES},
      {"GTO_LANE_MIN", &Tunables::lane_min, nullptr, nullptr, 1, BIG},
      {"GTO_ADOPT", &Tunables::adopt_below, nullptr, nullptr, 0, BIG},
      {"GTO_OBS_TG", &Tunables::obs_tg, &Tunables::obs_tg_few, &Tunables::obs_tg_few_tail, 1, GTO_MAX_TG},
      {"GTO_OBS_TG_FEW", &Tunables::obs_tg_few, &Tunables::obs_tg_few_tail, nullptr, 1, GTO_MAX_TG},
      {"GTO_OBS_TG_FEW_TAIL", &Tunables::obs_tg_few_tail, nullptr, nullptr, 1, GTO_MAX_TG},
      {"GTO_OBS_TG_WIDE", &Tunables::obs_tg_wide, nullptr, nullptr, 1, GTO_MAX_TG},
      {"GTO_FEW_INSTANCES", &Tunables::few_instances, nullptr, nullptr, INT_MIN, INT_MAX},
      {"GTO_STEP_TCLASS", &Tunables::step_tclass, nullptr, nullptr, 0, 1},
      {"GTO_STEP_TEXACT", &Tunables::step_texact, nullptr, nullptr, 0, 1},
  };
  for (const Row& r : rows) {
    const char* e = getenv(r.name);
    if (!e) continue;
    int v = atoi(e);
    v = r.lo == 0 && r.hi == 1 ? (v != 0) : std::max(r.lo, std::min(r.hi, v));
    for (F f : {r.f, r.also1, r.also2})
      if (f) t.*f = v;
  }
  t.obs_tg_given = getenv("GTO_OBS_TG") != nullptr;
  if (const char* e = getenv("GTO_STEP_NW_FEW")) t.step_nw_few = atoi(e) == 8 ? 8 : 4;
  if (const char* e = getenv("GTO_PB_MIN_GAIN")) t.pb_min_gain = atof(e);
  t.debug_timing = getenv("GTO_DEBUG_TIMING") != nullptr;
  t.lane_debug = getenv("GTO_LANE_DEBUG") != nullptr;
  if (t.dbg_cut) fprintf(stderr, "[gto] WARNING: GTO_DEBUG_CUT=%d cuts the obstacle kernel short: timing experiments only, RESULTS ARE GARBAGE\n", t.dbg_cut);
}

// Every device and pinned allocation behind the ABI lives in one of these and goes with the object that holds it: a
// handle, a scene's entry, an observation, an occupancy grid, a call's locals (gto_owned.h; DepthPool is the exception)
using DevBuf = Owned<hipFree>;
using PinBuf = Owned<hipHostFree>;

struct gto_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;  // false after gto_set_stream(h, caller's stream)
  std::string err;
  gto_solver_opts opts;
  RobotDev rb;  // host copy
  // the robot's tables on the device, uploaded once by gto_create: the buffers, and what the launches take
  DevBuf rb_buf, px_buf, py_buf, pz_buf, plink_buf, perm_buf, chunks_buf;
  RobotDev* d_rb = nullptr;
  double *d_px = nullptr, *d_py = nullptr, *d_pz = nullptr;
  int32_t *d_plink = nullptr, *d_perm = nullptr;
  Chunk* d_chunks = nullptr;
  std::vector<PbChunk> pbchunks;  // bounding spheres of the chunks of moving links, with their frames (prebroad_tail)
  int pb_C = 0;
  DevBuf d_pbimg;  // their table (floats) for each valid scene (SceneDev::pb_img; sync_pb_images)
  std::vector<SceneDev> scenes;  // host mirror, index = scene id
  // per scene id, the one to six allocations the scene owns; none for a borrowed scene (valid == 2) and an empty slot
  std::vector<std::vector<DevBuf>> scene_bufs;
  DevBuf scenes_buf;  // the table on the device
  SceneDev* d_scenes = nullptr;  // ... as the launches take it (sync_scene_table)
  // solve workspace (grown on demand)
  DevBuf state, Qcur, Qtry, vis, screw, blocks, goalblk, ssfixed, ndone, qf, livebuf, qfs, wrecbuf, itembuf, seedmask, inithead;
  DevBuf counters;  // work counters of a profiled solve
  unsigned long long last_counters[4] = {0, 0, 0, 0};
  PinBuf h_ndone;
  // pinned, device-visible, written by the first workgroup of every step launch: word 0 = call tag << 32 | instances
  // finished, word 1 = call tag << 32 | round of that launch.  The host sizes its launches by the first and stays at most
  // `ahead` rounds in front of the second: no event, no copy, nothing in the stream between the kernels
  PinBuf h_progress;
  unsigned long long* d_progress = nullptr;  // its device address
  unsigned progress_tag = 0;
  Tunables tu;  // the GTO_* knobs, read at gto_create
  int spec_kmax = 1;  // candidates per step the eight-wave step kernel's LDS has room for at this T
  DevBuf dbg;  // GTO_DEBUG_TIMING: the kernels' phase stamps (long long[256])
  std::atomic<int> dbg_step_launches[2] = {{0}, {0}};  // ... and the call's narrow step launches: [1] of k_lm_step_t50, [0] of the others
  // buffers of the scene that the last gto_set_scene replaced: the next replacement of the same size takes them instead of
  // going through hipMalloc / hipFree (fourteen calls of 0.2-0.3 ms each: most of a small scene's upload time)
  std::vector<DevBuf> spare;
  // staging for the host-pointer entry points (Staging)
  DevBuf in[GTO_STAGE_SLOTS], out[GTO_STAGE_SLOTS];
  // pinned twins of the staging buffers: host arrays are copied through them, so that the transfers are real DMA at a
  // steady rate (a hipMemcpyAsync from pageable memory stages inside the runtime: 1-6 ms of jitter per call with four
  // lanes copying at once) and never depend on what kind of memory the caller's arrays live in
  PinBuf pin_in[GTO_STAGE_SLOTS], pin_out[GTO_STAGE_SLOTS];
  // profiling of the dominant kernel
  bool profiling = false;
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_variant;  // kernel variant of launch i (GTO_PROF_*: include/gto_solver.h)
  std::vector<long long> ev_wgs;  // its workgroups
  double last_ms = 0.0;
  int last_launches = 0;
  // per kernel variant of the last profiled solve: milliseconds, launches, workgroups launched, surface points gathered
  double prof_ms[GTO_PROF_VARIANTS] = {};
  long long prof_launches[GTO_PROF_VARIANTS] = {}, prof_wgs[GTO_PROF_VARIANTS] = {};
  unsigned long long prof_points[GTO_PROF_VARIANTS] = {};
  size_t lm_lds = 0;
  int np = GTO_NB;     // block width of the normal equations: 8 (up to eight optimised joints) or 16
  DevBuf zws;          // k_lm_step_wide: block inverses [slots][T-2][np*np]
  hipStream_t lane_stream[GTO_MAX_LANES] = {};
  hipEvent_t lane_event[GTO_MAX_LANES] = {};
  hipStream_t user_lane_stream[GTO_MAX_LANES] = {};  // gto_set_lane_streams: the caller's streams for the lanes
  int n_user_lane_streams = 0;
  // items (job, group pairs with something to gather) per evaluation job: the largest ratio the rounds of the last call
  // published (the prior of the next call's launches until its own counts arrive)
  double items_per_job_prior = 0.0;
  std::mutex* prof_mu = nullptr;  // set while a call with several lanes (host threads) runs: guards the profiling records
  // retiming (gto_retime_paths_device): Thomas factors of the not-a-knot system for every column count, workspace grown on
  // demand
  DevBuf rt_fac, rt_S, rt_flag, rt_P1, rt_P2, rt_cap, rt_X, rt_T, rt_stat;
  // gto_retime_paths_torque: the torque coefficients [B][Nmax][ndof] beside rt_P1 / rt_P2, and the samples [B][M][ndof] that
  // tau_out is computed from where the caller asked for tau_out without them
  DevBuf rt_TA, rt_TB, rt_TG, rt_q, rt_qd, rt_qdd;
  bool rt_fac_ready = false;
  // collision checks against a cloud observation (gto_check_plans_device): world points, votes and per-plan bases of a chunk
  DevBuf ck_xyz, ck_flags, ck_base;
  // the held object's points (gto_check_held_paths_device): the points in link_ee's frame at the grasp [B][P_max][3] and the
  // per-plan bad flags [B]
  DevBuf hd_p, hd_bad;
  // seed choice (gto_seed_goalsets_device): per-waypoint cost sums of the candidates [B][n_max][T]
  DevBuf sd_part;
  // base placement with resident arrays (gto_solve_base_batch_device, gto_base_report_device): the device copy of the
  // caller's n_goals, and the per-set counts when the caller asks for the choice alone
  DevBuf bs_ng, bs_coll;
  PinBuf bs_pin[GTO_BASE_PIN_SLOTS];           // pinned copies of the small host arrays, one per call in flight (pinned_to_device)
  hipEvent_t bs_pin_ev[GTO_BASE_PIN_SLOTS] = {};  // recorded behind the copy that reads slot k
  int bs_pin_next = 0;
  // the grasp filter (gto_filter_grasps_device): the depth objects' views, the uncompacted goals [B][n_max][16], the poses
  // of the cloud objects' rows [B][n_max][16], the counts [B][n_max]
  DevBuf fg_tab, fg_plan, fg_ik, fg_pose, fg_count;
  // the link inertials (gto_set_link_inertials): the table rt_rnea reads; none until the first call
  DevBuf dyn_buf;
  bool has_inertials = false;
  // the link pairs of gto_self_clearance (gto_set_self_pairs; gto_create: every pair of distinct links): travels as a kernel
  // argument, so a call in flight keeps the mask it was launched with
  SelfPairs self_pairs = {};

  // the streams and events the handle created; the buffers above free themselves after this (gto_destroy has set the device)
  ~gto_handle() {
    for (auto e : bs_pin_ev) if (e) (void)hipEventDestroy(e);
    for (auto e : ev) (void)hipEventDestroy(e);
    if (stream && own_stream) (void)hipStreamDestroy(stream);
    for (int l = 0; l < GTO_MAX_LANES; ++l) {
      if (lane_stream[l]) (void)hipStreamDestroy(lane_stream[l]);
      if (lane_event[l]) (void)hipEventDestroy(lane_event[l]);
    }
  }
};

#define HIPCHK(h, call)                                                                              \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) {                                                                          \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                  \
      return GTO_ERR_HIP;                                                                            \
    }                                                                                                \
  } while (0)

static int fail(gto_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  else g_create_error = msg;
  return code;
}

// exactly `bytes` bytes: scenes, whose spares are matched by byte count, and the tables that never grow
static hipError_t dev_alloc(DevBuf& b, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess) b = DevBuf(p, bytes);
  return e;
}
static hipError_t pinned_alloc(PinBuf& b, size_t bytes, unsigned flags = hipHostMallocDefault) {
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, flags);
  if (e == hipSuccess) b = PinBuf(p, bytes);
  return e;
}

// a buffer of at least `bytes` bytes, device or pinned: grown with 25 % + 256 B to spare, contents not kept.  It is regrown by
// free and allocate while earlier calls of the handle may still be queued on its stream with the old pointer in their
// arguments (bs_ng, ck_base, hd_p, the solver workspace: one buffer per handle).  That is safe because hipFree and
// hipHostFree wait for the device before they release anything: a call that regrows is a host synchronisation, and a
// stream-ordered free (hipFreeAsync on another stream) in their place would not be
// (tests/test_gpu_stream_order.py, the runs of six calls).
template <class Buf, class Alloc>
static int ensure_with(gto_handle* h, Buf& b, size_t bytes, Alloc alloc) {
  if (bytes <= b.bytes()) return GTO_OK;
  HIPCHK(h, b.reset());
  HIPCHK(h, alloc(b, bytes + bytes / 4 + 256));
  return GTO_OK;
}
static int ensure(gto_handle* h, DevBuf& b, size_t bytes) { return ensure_with(h, b, bytes, dev_alloc); }
static int ensure(gto_handle* h, PinBuf& b, size_t bytes) {
  return ensure_with(h, b, bytes, [](PinBuf& x, size_t n) { return pinned_alloc(x, n); });
}

extern "C" {

void gto_default_opts(gto_solver_opts* o) {
  o->T = 50;  // gto/gto_planner.py:25
  o->Tmax = 10.0;  // :26
  o->standoff_offset = -10;  // :22
  o->w_obstacle = 10.0;  // :131
  o->w_vel = 0.01;  // :135
  o->max_iter = 100;  // :141
  o->tol_step = 1e-7;
  o->tol_rel_f = 1e-8;  // relative decrease of f below which an accepted step ends the solve (scipy least_squares ftol default)
  o->lambda0 = 1e-3;
  o->grad_mode = GTO_GRAD_CENTRAL_DIFF;
}

int32_t gto_version(void) { return GTO_VERSION; }

const char* gto_last_error(const gto_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static int validate_opts(const gto_solver_opts* o, std::string& why) {
  if (o->T < 4) { why = "T must be >= 4"; return 0; }
  if (o->T > GTO_MAX_T) { why = "T must be <= 96 (GTO_MAX_T)"; return 0; }
  // (NaN fails every comparison: each test is written so that NaN lands in the refusal)
  if (!(o->Tmax > 0) || !std::isfinite(o->Tmax)) { why = "Tmax must be positive and finite"; return 0; }
  if (!(o->w_obstacle >= 0) || !std::isfinite(o->w_obstacle)) { why = "w_obstacle must be >= 0 and finite"; return 0; }
  if (!(o->w_vel >= 0) || !std::isfinite(o->w_vel)) { why = "w_vel must be >= 0 and finite"; return 0; }
  if (!(o->tol_step >= 0) || !std::isfinite(o->tol_step)) { why = "tol_step must be >= 0 and finite"; return 0; }
  if (!(o->tol_rel_f >= 0) || !std::isfinite(o->tol_rel_f)) { why = "tol_rel_f must be >= 0 and finite"; return 0; }
  if (o->max_iter < 0) { why = "max_iter must be >= 0"; return 0; }
  int ts = o->T + o->standoff_offset;
  if (ts < 2 || ts > o->T - 1) { why = "standoff waypoint T+standoff_offset must lie in [2, T-1]"; return 0; }
  if (o->grad_mode != GTO_GRAD_CENTRAL_DIFF && o->grad_mode != GTO_GRAD_ZERO) { why = "unknown grad_mode"; return 0; }
  if (!(o->lambda0 > 0) || !std::isfinite(o->lambda0)) { why = "lambda0 must be positive and finite"; return 0; }
  return 1;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is process-wide per kernel: a handle for a smaller robot or goal set must
// never lower what an earlier handle launches with.  One high-water mark per kernel, only ever raised.
// The attribute belongs to the (function, device) pair of the CURRENT device: the marks are kept per device, and every
// caller has done hipSetDevice(h->device) before.
static hipError_t raise_dynamic_lds(const void* kernel, size_t bytes) {
  struct Mark { int device; const void* kernel; size_t bytes; };
  static std::mutex mu;
  static std::vector<Mark> marks;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  for (auto& m : marks)
    if (m.kernel == kernel && m.device == dev) {
      if (bytes <= m.bytes) return hipSuccess;
      const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (e == hipSuccess) m.bytes = bytes;
      return e;
    }
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) marks.push_back({dev, kernel, bytes});
  return e;
}

// The obstacle kernel variant of a launch: np-wide blocks; deep gather batches (launches with few instances in flight);
// an itemized launch laid out over an estimate, with the crew for the rest at the end of its grid; the hot variants of the
// solve loop's evaluations (central differences: the value-only gather, the init pass's virtual waypoints and the
// static-link bookkeeping compiled out).  The wide robots have two variants, the launches with a crew have two.  gto_create
// raises the dynamic LDS of every variant this returns.
using ObsKernel = decltype(&k_obstacle_gram<GTO_NB>);
static ObsKernel obstacle_kernel(int np, bool deep, bool sweep, bool hot) {
  // [wide, 8-wide, 8-wide deep]; the first reference to a variant decides where the code object places it, so they keep
  // the order they have always had (the launch with a crew where the crew's own kernel was, its hot variant last)
  static const ObsKernel cold[3] = {k_obstacle_gram<16>, k_obstacle_gram<GTO_NB>, k_obstacle_gram<GTO_NB, GTO_OBS_DEEP_PD>};
  static const ObsKernel crew = k_obstacle_gram<GTO_NB, GTO_OBS_MAIN_PD, true>;
  static const ObsKernel warm[3] = {k_obstacle_gram<16, GTO_OBS_MAIN_PD, false, true>, k_obstacle_gram<GTO_NB, GTO_OBS_MAIN_PD, false, true>,
                                    k_obstacle_gram<GTO_NB, GTO_OBS_DEEP_PD, false, true>};
  static const ObsKernel warm_crew = k_obstacle_gram<GTO_NB, GTO_OBS_MAIN_PD, true, true>;
  if (sweep && !deep && np == GTO_NB) return hot ? warm_crew : crew;
  const int i = np != GTO_NB ? 0 : deep ? 2 : 1;
  return hot ? warm[i] : cold[i];
}

int gto_create(const gto_robot_desc* d, const gto_solver_opts* opts, int device, gto_handle** out) {
  if (!d || !opts || !out) return fail(nullptr, GTO_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  std::string why;
  if (!validate_opts(opts, why)) return fail(nullptr, GTO_ERR_INVALID_ARG, why);
  Tunables tu;
  read_tunables(tu);
  std::unique_ptr<RobotTables> t(new RobotTables());
  if (int rc = build_robot(d, tu.pb_merge, *t, why)) return fail(nullptr, rc, why);  // (gto_robot.h: descriptor checks, then the tables)
  const RobotDev& rb = t->rb;
  const int np = rb.n_opt <= GTO_NB ? GTO_NB : 16;
  const size_t lm_lds = np == GTO_NB ? lm_lds_bytes(opts->T, 1) : lm_wide_lds_bytes(opts->T, 16);
  if (lm_lds > 160 * 1024) return fail(nullptr, GTO_ERR_UNSUPPORTED, "T too large for the step kernel's LDS");
  const bool wide = np != GTO_NB;
  // waypoints per obstacle workgroup of the wide robots (GTO_OBS_TG_WIDE; GTO_OBS_TG, when given, is the group size of
  // every robot), fewer if the robot's tables would not fit the CU's LDS.  The fixed part of a 16-wide workgroup (tables,
  // matrix-core prefix, projection onto sixteen screws) is larger than an 8-wide one's, and since round 6 the epilogue
  // projects one waypoint at a time (ObsLds: its scratch no longer grows with the group): configs[4] with 2 / 3 / 4 / 5 /
  // 6 / 8 waypoints per workgroup 29.0 / 33.1 / 35.4 / 36.6 / 34.8 / 28.7 k trajectories/s (until round 6: two, 28.2 k)
  // The 8-wide robots keep room for GTO_MAX_TG waypoints (any GTO_OBS_TG*), and the same shrinking when theirs would not
  // fit: with 26 or more links of 64 points each at 32 frames, eight waypoints' Grams and chunk lists overflow the LDS.
  int tg_w = wide ? tu.obs_tg_wide : GTO_MAX_TG;
  if (wide && tu.obs_tg_given) tg_w = std::max(tg_w, tu.obs_tg);
  while (tg_w > 1 && (size_t)ObsLds(tg_w, rb.n_frames, rb.n_links, tg_w * rb.n_chunks, np).total_doubles * sizeof(double) > 150 * 1024) --tg_w;
  const ObsLds lay(tg_w, rb.n_frames, rb.n_links, tg_w * rb.n_chunks, np);
  if ((size_t)lay.total_doubles * sizeof(double) > 150 * 1024) return fail(nullptr, GTO_ERR_UNSUPPORTED, "robot too large for the obstacle kernel's LDS");
  if (wide) {
    tu.obs_tg = tu.obs_tg_given ? std::min(tu.obs_tg, tg_w) : tg_w;
    tu.obs_tg_few = std::min(tu.obs_tg_few, tu.obs_tg), tu.obs_tg_few_tail = std::min(tu.obs_tg_few_tail, tu.obs_tg);
  } else if (tg_w < GTO_MAX_TG) {
    tu.obs_tg = std::min(tu.obs_tg, tg_w);
    tu.obs_tg_few = std::min(tu.obs_tg_few, tg_w), tu.obs_tg_few_tail = std::min(tu.obs_tg_few_tail, tg_w);
  }
  // candidates per step the eight-wave step kernel's LDS has room for at this T
  int spec_kmax = 1;
  if (!wide)
    while (spec_kmax < GTO_KSPEC && lm_lds_bytes(opts->T, spec_kmax + 1) <= 160 * 1024 - 256) ++spec_kmax;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, GTO_ERR_NO_DEVICE, "no HIP device visible: the GTO solve path has no CPU fallback");
  if (device >= ndev) return fail(nullptr, GTO_ERR_INVALID_ARG, "device index out of range");
  if (device >= 0 && hipSetDevice(device) != hipSuccess) return fail(nullptr, GTO_ERR_HIP, "hipSetDevice failed");

  gto_handle* h = new gto_handle();
  if (device >= 0) h->device = device;
  else (void)hipGetDevice(&h->device);
  h->opts = *opts;
  h->tu = tu;
  std::memcpy(&h->rb, &rb, sizeof rb);
  gto_selfpairs::all_distinct_pairs(rb.n_links, h->self_pairs.rows);
  h->pb_C = t->pb_C;
  h->pbchunks = t->pbchunks;
  h->np = np;
  h->lm_lds = lm_lds;
  h->spec_kmax = spec_kmax;
  if (tu.debug_timing && dev_alloc(h->dbg, 256 * sizeof(long long)) == hipSuccess) (void)hipMemset(h->dbg.get(), 0, h->dbg.bytes());
  auto up = [&](DevBuf& b, const void* src, size_t bytes) -> bool {
    return dev_alloc(b, bytes) == hipSuccess && hipMemcpy(b.get(), src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  const size_t P = t->px.size();
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { gto_destroy(h); return fail(nullptr, GTO_ERR_HIP, "hipStreamCreate failed"); }
  const bool ok = up(h->rb_buf, &h->rb, sizeof h->rb) && up(h->px_buf, t->px.data(), P * sizeof(double)) &&
                  up(h->py_buf, t->py.data(), P * sizeof(double)) && up(h->pz_buf, t->pz.data(), P * sizeof(double)) &&
                  up(h->plink_buf, t->plink.data(), P * sizeof(int32_t)) && up(h->perm_buf, t->perm.data(), P * sizeof(int32_t)) &&
                  up(h->chunks_buf, t->chunks.data(), t->chunks.size() * sizeof(Chunk));
  if (!ok) { gto_destroy(h); return fail(nullptr, GTO_ERR_ALLOC, "device allocation failed in gto_create"); }
  h->d_rb = h->rb_buf.as<RobotDev>(), h->d_chunks = h->chunks_buf.as<Chunk>();
  h->d_px = h->px_buf.as<double>(), h->d_py = h->py_buf.as<double>(), h->d_pz = h->pz_buf.as<double>();
  h->d_plink = h->plink_buf.as<int32_t>(), h->d_perm = h->perm_buf.as<int32_t>();
  // dynamic LDS of every kernel variant the handle can launch (obstacle_kernel, the step kernels)
  const size_t lds = std::min<size_t>((size_t)lay.total_doubles * sizeof(double), 160 * 1024);
  hipError_t e = hipSuccess;
  for (int v = 0; v < 8 && e == hipSuccess; ++v) e = raise_dynamic_lds((const void*)obstacle_kernel(np, v & 1, v & 2, v & 4), lds);
  if (e == hipSuccess) e = wide ? raise_dynamic_lds((const void*)k_lm_step_wide<16>, lm_lds) : raise_dynamic_lds((const void*)k_lm_step<4, 1>, lm_lds);
  if (e == hipSuccess && !wide) e = raise_dynamic_lds((const void*)k_lm_step<8, GTO_KSPEC>, lm_lds_bytes(opts->T, spec_kmax));
  if (e == hipSuccess && !wide) e = raise_dynamic_lds((const void*)k_lm_step_short<4, 1>, lm_lds);
  if (e == hipSuccess && !wide) e = raise_dynamic_lds((const void*)k_lm_step_short<8, GTO_KSPEC>, lm_lds_bytes(opts->T, spec_kmax));
  if (e == hipSuccess && !wide) e = raise_dynamic_lds((const void*)k_lm_step_t50<4, 1>, lm_lds);
  if (e == hipSuccess && !wide) e = raise_dynamic_lds((const void*)k_lm_step_t50<8, GTO_KSPEC>, lm_lds_bytes(opts->T, spec_kmax));
  if (e == hipSuccess && !wide) e = raise_dynamic_lds((const void*)k_seed_broad, lm_lds);
  if (e != hipSuccess) { gto_destroy(h); return fail(nullptr, GTO_ERR_HIP, "hipFuncSetAttribute failed"); }
  *out = h;
  return GTO_OK;
}

void gto_destroy(gto_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;  // ~gto_handle: its streams and events, then every buffer by its owner
}

int gto_set_opts(gto_handle* h, const gto_solver_opts* o) {
  if (!h || !o) return GTO_ERR_INVALID_ARG;
  std::string why;
  if (!validate_opts(o, why)) return fail(h, GTO_ERR_INVALID_ARG, why);
  if (o->T != h->opts.T) return fail(h, GTO_ERR_INVALID_ARG, "T cannot change after gto_create");
  h->opts = *o;
  return GTO_OK;
}

// The step kernel's tail copies its sphere table into LDS as it is (prebroad_tail): per valid scene, the spheres' centres
// and their culling radii in that scene's voxels, then the spheres' frames, rows of four floats.  The radius is the
// expression the tail evaluated per workgroup before, with the fused multiply-add the GPU compiles it to.
static int sync_pb_images(gto_handle* h) {
  const int C = h->pb_C;
  const size_t rows = (size_t)pb_img_rows(C);
  size_t nv = 0;
  for (const SceneDev& s : h->scenes) nv += s.valid ? 1 : 0;
  if (nv * rows * 4 * sizeof(float) > h->d_pbimg.bytes()) {
    HIPCHK(h, h->d_pbimg.reset());
    HIPCHK(h, dev_alloc(h->d_pbimg, std::max<size_t>(16, nv * 2) * rows * 4 * sizeof(float)));
  }
  std::vector<float> img(nv * rows * 4, 0.f);
  const double eps = h->rb.pb_eps;
  size_t k = 0;
  for (SceneDev& s : h->scenes) {
    s.pb_img = nullptr;
    if (!s.valid || rows == 0) continue;
    float* v = img.data() + k * rows * 4;
    for (int c = 0; c < C; ++c) {
      const PbChunk& cc = h->pbchunks[c];
      v[4 * c] = (float)cc.cx, v[4 * c + 1] = (float)cc.cy, v[4 * c + 2] = (float)cc.cz;
      v[4 * c + 3] = (float)((int)std::ceil(std::fma(cc.r + eps, s.rinv, 1e-6)) + GTO_BROAD_MARGIN);
      std::memcpy(v + 4 * C + c, &cc.frame, sizeof(int32_t));
    }
    s.pb_img = h->d_pbimg.as<float>() + k * rows * 4;
    ++k;
  }
  if (!img.empty()) HIPCHK(h, hipMemcpy(h->d_pbimg.get(), img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
  return GTO_OK;
}

static int sync_scene_table(gto_handle* h) {
  size_t n = h->scenes.size();
  if (int rc = sync_pb_images(h)) return rc;
  if (n * sizeof(SceneDev) > h->scenes_buf.bytes()) {
    h->d_scenes = nullptr;
    HIPCHK(h, h->scenes_buf.reset());
    HIPCHK(h, dev_alloc(h->scenes_buf, std::max<size_t>(16, n * 2) * sizeof(SceneDev)));
    h->d_scenes = h->scenes_buf.as<SceneDev>();
  }
  HIPCHK(h, hipMemcpy(h->d_scenes, h->scenes.data(), n * sizeof(SceneDev), hipMemcpyHostToDevice));
  return GTO_OK;
}

// valid: 0 empty, 1 owned by this handle, 2 borrowed from another handle (gto_share_scene)
static int free_scene(gto_handle* h, int32_t id) {
  h->scenes[id].valid = 0;
  std::vector<DevBuf> bufs;
  bufs.swap(h->scene_bufs[id]);  // the entry owns nothing from here on; what a failed free leaves goes with `bufs`
  for (DevBuf& b : bufs) HIPCHK(h, b.reset());
  return GTO_OK;
}

// room for scene `id` in the table and in the list of what the scenes own
static void grow_scene_table(gto_handle* h, int32_t id) {
  if ((size_t)id < h->scenes.size()) return;
  SceneDev z;
  memset(&z, 0, sizeof z);
  h->scenes.resize(id + 1, z);
  h->scene_bufs.resize(id + 1);
}

// a scene id that names a set scene (owned or borrowed)
static bool scene_valid(const gto_handle* h, int32_t id) {
  return id >= 0 && (size_t)id < h->scenes.size() && h->scenes[id].valid;
}

static int check_scene_ids_host(gto_handle* h, const int32_t* ids, int B) {
  for (int b = 0; b < B; ++b)
    if (!scene_valid(h, ids[b])) return fail(h, GTO_ERR_NO_SCENE, "scene_id refers to a scene that was never set");
  for (int b = 0; b < B; ++b)
    if (!h->scenes[ids[b]].r_all)
      return fail(h, GTO_ERR_NO_SCENE, "scene_id refers to a values-only scene (gto_set_scene_values): it serves gto_plan_cost and gto_eval_points only");
  return GTO_OK;
}

int gto_share_scene(gto_handle* dst, int32_t dst_id, gto_handle* src, int32_t src_id) {
  return gto_share_scene_halves(dst, dst_id, src, src_id, 0, 1);
}

int gto_share_scene_halves(gto_handle* dst, int32_t dst_id, gto_handle* src, int32_t src_id, int32_t all_from, int32_t obs_from) {
  if (!dst || !src) return GTO_ERR_INVALID_ARG;
  if ((all_from != 0 && all_from != 1) || (obs_from != 0 && obs_from != 1)) return fail(dst, GTO_ERR_INVALID_ARG, "gto_share_scene_halves: a half is 0 (c_all) or 1 (c_obs)");
  if (dst_id < 0 || dst_id >= 65536) return fail(dst, GTO_ERR_INVALID_ARG, "scene_id out of range [0,65536)");
  if (!scene_valid(src, src_id))
    return fail(dst, GTO_ERR_NO_SCENE, "gto_share_scene: the source scene was never set");
  if (dst->device != src->device) return fail(dst, GTO_ERR_INVALID_ARG, "gto_share_scene: handles live on different devices");
  HIPCHK(dst, hipSetDevice(dst->device));
  HIPCHK(dst, hipStreamSynchronize(dst->stream));
  grow_scene_table(dst, dst_id);
  int rcf = free_scene(dst, dst_id);
  if (rcf) return rcf;
  const SceneDev& ss = src->scenes[src_id];
  SceneDev& ds = dst->scenes[dst_id];
  ds = ss;
  ds.c_all = all_from ? ss.c_obs : ss.c_all, ds.r_all = all_from ? ss.r_obs : ss.r_all, ds.d_all = all_from ? ss.d_obs : ss.d_all;
  ds.c_obs = obs_from ? ss.c_obs : ss.c_all, ds.r_obs = obs_from ? ss.r_obs : ss.r_all, ds.d_obs = obs_from ? ss.d_obs : ss.d_all;
  ds.valid = 2;
  return sync_scene_table(dst);
}

static int set_scene_impl(gto_handle* h, int32_t id, const float* c_all, const float* c_obs, const int32_t shape[3],
                          const double origin[3], double res, bool values_only, hipMemcpyKind kind = hipMemcpyHostToDevice) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!c_all || !shape || !origin) return fail(h, GTO_ERR_INVALID_ARG, "null argument");
  if (id < 0 || id >= 65536) return fail(h, GTO_ERR_INVALID_ARG, "scene_id out of range [0,65536)");
  if (shape[0] < 1 || shape[1] < 1 || shape[2] < 1 || !(res > 0)) return fail(h, GTO_ERR_INVALID_ARG, "bad field geometry");
  // (the gather loop forms the voxel offset with 24-bit multiply-adds: iz + nz (iy + ny ix))
  if ((long long)shape[0] * shape[1] > (1ll << 24) || shape[2] >= (1 << 24) || (long long)shape[0] * shape[1] * shape[2] >= (1ll << 32))
    return fail(h, GTO_ERR_UNSUPPORTED, "field too large: nx ny <= 2^24, nz < 2^24 and fewer than 2^32 voxels");
  const size_t nvox = (size_t)shape[0] * shape[1] * shape[2];
  if (nvox >= ((size_t)1 << 31)) return fail(h, GTO_ERR_UNSUPPORTED, "field larger than 2^31 voxels");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // Build the new scene completely first (fields, voxel records, distance fields), then swap it in and free the old one:
  // a failure half-way leaves the table and the previous scene of this id untouched and frees what was allocated.
  std::vector<DevBuf> built, aside;  // the new scene's buffers; the scratch half of the distance fields
  auto dalloc_in = [&](std::vector<DevBuf>& into, void** p, size_t bytes) {
    into.emplace_back();
    DevBuf& b = into.back();
    hipError_t e = hipSuccess;
    auto fit = std::find_if(h->spare.begin(), h->spare.end(), [&](const DevBuf& sp_) { return sp_.bytes() == bytes; });
    if (fit != h->spare.end()) {  // a buffer of the scene replaced last time
      b = std::move(*fit);
      h->spare.erase(fit);
    } else {
      e = dev_alloc(b, bytes);
    }
    *p = b.get();
    return e;
  };
  auto dalloc = [&](void** p, size_t bytes) { return dalloc_in(built, p, bytes); };
  float *da = nullptr, *dob = nullptr;
  HIPCHK(h, dalloc((void**)&da, nvox * sizeof(float)));
  HIPCHK(h, hipMemcpy(da, c_all, nvox * sizeof(float), kind));
  if (c_obs && c_obs != c_all) {
    HIPCHK(h, dalloc((void**)&dob, nvox * sizeof(float)));
    HIPCHK(h, hipMemcpy(dob, c_obs, nvox * sizeof(float), kind));
  } else {
    dob = da;
  }
  // gather-friendly voxel records (one-time, outside the timed solve); a values-only scene (gto_set_scene_values: seed
  // scoring and point look-ups) stops at the two float fields
  VoxelRec *ra = nullptr, *rob = nullptr;
  uint8_t *dista = nullptr, *distb = nullptr, *scratch = nullptr;
  if (!values_only) {
  HIPCHK(h, dalloc((void**)&ra, nvox * sizeof(VoxelRec)));
  const unsigned nblk = (unsigned)((nvox + 255) / 256);
  hipLaunchKernelGGL(k_build_records, dim3(nblk), dim3(256), 0, h->stream, da, ra, shape[0], shape[1], shape[2]);
  if (dob != da) {
    HIPCHK(h, dalloc((void**)&rob, nvox * sizeof(VoxelRec)));
    hipLaunchKernelGGL(k_build_records, dim3(nblk), dim3(256), 0, h->stream, dob, rob, shape[0], shape[1], shape[2]);
  } else {
    rob = ra;
  }
  // broad-phase distance fields: ping-pong relaxation, the scratch half is freed again
  HIPCHK(h, dalloc_in(aside, (void**)&scratch, nvox));
  for (int which = 0; which < (rob != ra ? 2 : 1); ++which) {
    uint8_t* d0 = nullptr;
    HIPCHK(h, dalloc((void**)&d0, nvox));
    if (h->tu.dist_relax) {  // GTO_DIST_RELAX=1: the reference construction, GTO_DIST_CAP sweeps of 3x3x3 min-plus-one (A/B and tests)
      uint8_t* d1 = scratch;
      hipLaunchKernelGGL(k_dist_init, dim3(nblk), dim3(256), 0, h->stream, which ? rob : ra, d0, (long)nvox);
      for (int it = 0; it < GTO_DIST_CAP; ++it) {
        hipLaunchKernelGGL(k_dist_relax, dim3(nblk), dim3(256), 0, h->stream, d0, d1, shape[0], shape[1], shape[2]);
        std::swap(d0, d1);
      }
      static_assert(GTO_DIST_CAP % 2 == 0, "ping-pong parity: the result is back in the buffer allocated for it");
    } else {  // separable: one exact pass per axis, scratch -> d0 -> scratch -> d0
      hipLaunchKernelGGL(k_dist_init, dim3(nblk), dim3(256), 0, h->stream, which ? rob : ra, scratch, (long)nvox);
      hipLaunchKernelGGL(k_dist_axis, dim3(nblk), dim3(256), 0, h->stream, scratch, d0, shape[0], shape[1], shape[2], 2);
      hipLaunchKernelGGL(k_dist_axis, dim3(nblk), dim3(256), 0, h->stream, d0, scratch, shape[0], shape[1], shape[2], 1);
      hipLaunchKernelGGL(k_dist_axis, dim3(nblk), dim3(256), 0, h->stream, scratch, d0, shape[0], shape[1], shape[2], 0);
    }
    (which ? distb : dista) = d0;
  }
  if (rob == ra) distb = dista;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  grow_scene_table(h, id);
  SceneDev& s = h->scenes[id];
  // what is left of the previous spares did not fit this scene: free it; the scratch half and the replaced scene's buffers
  // become the spares
  h->spare = std::move(aside);
  for (DevBuf& b : h->scene_bufs[id]) h->spare.push_back(std::move(b));
  h->scene_bufs[id] = std::move(built);
  s.c_all = da;
  s.c_obs = dob;
  s.r_all = ra;
  s.r_obs = rob;
  s.d_all = dista;
  s.d_obs = distb;
  s.nx = shape[0];
  s.ny = shape[1];
  s.nz = shape[2];
  s.ox = origin[0];
  s.oy = origin[1];
  s.oz = origin[2];
  s.res = res;
  s.rinv = 1.0 / res;
  s.inv2r = 1.0 / (2.0 * res);
  s.valid = 1;
  return sync_scene_table(h);
}

int gto_set_scene(gto_handle* h, int32_t id, const float* c_all, const float* c_obs, const int32_t shape[3],
                  const double origin[3], double res) {
  return set_scene_impl(h, id, c_all, c_obs, shape, origin, res, false);
}

int gto_set_scene_values(gto_handle* h, int32_t id, const float* c_all, const float* c_obs, const int32_t shape[3],
                         const double origin[3], double res) {
  return set_scene_impl(h, id, c_all, c_obs, shape, origin, res, true);
}

int gto_drop_scene(gto_handle* h, int32_t id) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!scene_valid(h, id)) return fail(h, GTO_ERR_NO_SCENE, "unknown scene");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int rcf = free_scene(h, id);
  if (rcf) return rcf;
  memset(&h->scenes[id], 0, sizeof(SceneDev));
  return sync_scene_table(h);
}

int gto_set_mode(gto_handle* h, int32_t mode) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (mode != GTO_MODE_ROUNDS && mode != GTO_MODE_SINGLE_LAUNCH) return fail(h, GTO_ERR_INVALID_ARG, "unknown solver mode");
  // (the single-launch kernel of rounds 1-3, one workgroup running an instance's whole solve, was 2.4-2.9x slower than the
  // rounds and had been a test-only second implementation since round 3: removed in round 4; the mode number stays reserved)
  if (mode == GTO_MODE_SINGLE_LAUNCH) return fail(h, GTO_ERR_UNSUPPORTED, "GTO_MODE_SINGLE_LAUNCH was removed: the rounds mode is the solver");
  return GTO_OK;
}

int gto_set_lanes(gto_handle* h, int32_t max_lanes, int32_t min_per_lane, int32_t adopt_below) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (max_lanes < 1 || max_lanes > GTO_MAX_LANES || min_per_lane < 1 || adopt_below < 0)
    return fail(h, GTO_ERR_INVALID_ARG, "gto_set_lanes: 1 <= max_lanes <= 8, min_per_lane >= 1, adopt_below >= 0");
  h->tu.lanes_max = max_lanes, h->tu.lane_min = min_per_lane, h->tu.adopt_below = adopt_below;
  return GTO_OK;
}

int gto_set_lane_streams(gto_handle* h, int32_t n, void* const* streams) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (n < 0 || n > GTO_MAX_LANES || (n > 0 && !streams)) return fail(h, GTO_ERR_INVALID_ARG, "gto_set_lane_streams: 0 <= n <= 8 streams");
  for (int i = 0; i < n; ++i)
    if (!streams[i]) return fail(h, GTO_ERR_INVALID_ARG, "gto_set_lane_streams: null stream");
  for (int i = 0; i < n; ++i) h->user_lane_stream[i] = (hipStream_t)streams[i];
  h->n_user_lane_streams = n;
  return GTO_OK;
}

int gto_set_stream(gto_handle* h, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->stream && h->own_stream) HIPCHK(h, hipStreamDestroy(h->stream));
  h->stream = nullptr;
  if (stream) {
    h->stream = (hipStream_t)stream;
    h->own_stream = false;
  } else {
    HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
  }
  return GTO_OK;
}

int gto_last_kernel_work(gto_handle* h, uint64_t* points_gathered, uint64_t* chunk_tests) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (points_gathered) *points_gathered = h->last_counters[0];
  if (chunk_tests) *chunk_tests = h->last_counters[1];
  return GTO_OK;
}

int gto_last_kernel_profile(gto_handle* h, int32_t variant, double* total_ms, int32_t* launches, uint64_t* workgroups, uint64_t* points_gathered) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (variant < 0 || variant >= GTO_PROF_VARIANTS) return fail(h, GTO_ERR_INVALID_ARG, "unknown kernel variant");
  if (total_ms) *total_ms = h->prof_ms[variant];
  if (launches) *launches = (int32_t)h->prof_launches[variant];
  if (workgroups) *workgroups = (uint64_t)h->prof_wgs[variant];
  if (points_gathered) *points_gathered = h->prof_points[variant];
  return GTO_OK;
}

int gto_set_profiling(gto_handle* h, int32_t enabled) {
  if (!h) return GTO_ERR_INVALID_ARG;
  h->profiling = enabled != 0;
  return GTO_OK;
}

int gto_last_kernel_time(gto_handle* h, double* total_ms, int32_t* launches) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (total_ms) *total_ms = h->last_ms;
  if (launches) *launches = h->last_launches;
  return GTO_OK;
}

// -------------------------------------------------------------------------------------------------
static SolveParams make_params(const gto_handle* h, int n_max, bool use_standoff) {
  const gto_solver_opts& o = h->opts;
  SolveParams sp;
  sp.T = o.T;
  sp.ts = o.T + o.standoff_offset;
  sp.use_standoff = use_standoff ? 1 : 0;
  sp.n_max = n_max;
  sp.max_iter = o.max_iter;
  sp.grad_mode = o.grad_mode;
  sp.dt = o.Tmax / (double)(o.T - 1);  // gto/gto_planner.py:27-28
  sp.alpha = o.w_vel / (sp.dt * sp.dt);
  sp.w_obstacle = o.w_obstacle;
  sp.w_vel = o.w_vel;
  sp.tol_step = o.tol_step;
  sp.tol_rel_f = o.tol_rel_f;
  sp.lambda0 = o.lambda0;
  sp.dbg_cut = h->tu.dbg_cut;
  sp.interleave = h->tu.obs_interleave == 1;
  sp.static_pos = 0;
  sp.pb_next = 0, sp.pb_tg = 1, sp.pb_ng = 1, sp.pb_pw = 1, sp.pb_verify = 0;
  sp.pb_C = h->pb_C, sp.pb_tab0 = 0, sp.pb_mC = ObsGeom::magic(std::max(1, h->pb_C)), sp.pb_mF = ObsGeom::magic(h->rb.n_frames);
  sp.pb_eps = h->rb.pb_eps;
  sp.pb_npar = h->rb.pb_npar;
  sp.round = sp.parity = 0;
  sp.kcap = h->np == GTO_NB ? GTO_KSPEC : 1;  // candidate copies of the workspace (the wide step kernel generates one)
  sp.k_acc = sp.k_rej = sp.k_eval = 1;
  sp.spec_streak = h->tu.spec_streak;
  return sp;
}

static int ensure_workspace(gto_handle* h, int B) {
  const RobotDev& rb = h->rb;
  const size_t T = h->opts.T, n = rb.n_opt;
  int rc;
  if ((rc = ensure(h, h->state, (size_t)B * sizeof(InstState)))) return rc;
  if ((rc = ensure(h, h->Qcur, (size_t)B * n * T * sizeof(double)))) return rc;
  const size_t kcap = h->np == GTO_NB ? GTO_KSPEC : 1;
  if ((rc = ensure(h, h->Qtry, kcap * B * n * T * sizeof(double)))) return rc;
  const size_t bstride = (size_t)h->np * h->np + h->np + 8;
  if ((rc = ensure(h, h->blocks, (kcap + 1) * B * T * bstride * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->goalblk, (kcap + 1) * B * 2 * bstride * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->ssfixed, (size_t)B * 4 * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->ndone, 64 * GTO_MAX_LANES))) return rc;  // a finished-counter per lane, a cache line apart
  if ((rc = ensure(h, h->qf, (size_t)B * T * rb.n_frames * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->wrecbuf, (size_t)(kcap + 1) * B * T * 8 * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->seedmask, (size_t)B * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(h, h->inithead, (size_t)B * sizeof(int32_t)))) return rc;
  if (!h->h_ndone) HIPCHK(h, pinned_alloc(h->h_ndone, 64));
  if (!h->h_progress) {
    HIPCHK(h, pinned_alloc(h->h_progress, 64 * GTO_MAX_LANES, hipHostMallocMapped));  // eight words per lane
    std::memset(h->h_progress.get(), 0, 64 * GTO_MAX_LANES);  // every word the solve loop reads carries a call tag (never 0)
    HIPCHK(h, hipHostGetDevicePointer((void**)&h->d_progress, h->h_progress.get(), 0));
  }
  return GTO_OK;
}

static BatchPtrs make_ptrs(gto_handle* h, const int32_t* scene_id, const double* qc, const double* goals,
                           const int32_t* n_goals, const double* standoff, const double* base_pos, const double* Q0) {
  BatchPtrs bp = {};
  bp.scene_id = scene_id;
  bp.qc = qc;
  bp.goals = goals;
  bp.n_goals = n_goals;
  bp.standoff = standoff;
  bp.base_pos = base_pos;
  bp.Q0 = Q0;
  bp.state = h->state.as<InstState>();
  bp.Qcur = h->Qcur.as<double>();
  bp.Qtry = h->Qtry.as<double>();
  bp.blocks = h->blocks.as<double>();
  bp.goalblk = h->goalblk.as<double>();
  bp.ss_fixed = h->ssfixed.as<double>();
  bp.n_done = h->ndone.as<int32_t>();
  bp.qf = h->qf.as<double>();
  bp.live = nullptr;  // the live lists only exist inside the solve loop
  bp.jobs = nullptr;
  bp.nlive = nullptr;
  bp.next = nullptr;
  bp.qfs = nullptr;
  bp.wrec = h->wrecbuf.as<double>();
  bp.items = nullptr;
  bp.scenes = h->d_scenes;
  bp.cap = 0;
  bp.n_total = 0;
  bp.dbg = h->dbg.as<long long>();
  bp.work = nullptr;
  return bp;
}

static inline int obstacle_grid(int B, int nG) { return 8 * ((B + 7) / 8) * nG; }

// profiling (gto_set_profiling): a pair of HIP events on the launch stream around launch number h->last_launches
static int prof_begin(gto_handle* h, hipStream_t st, int variant, long long wgs) {
  if (h->prof_mu) h->prof_mu->lock();  // lanes of one call record into one list: begin .. end is one critical section
  const size_t need = (size_t)(h->last_launches + 1) * 2;
  hipError_t e = hipSuccess;
  while (h->ev.size() < need && e == hipSuccess) {
    hipEvent_t ev_;
    if ((e = hipEventCreate(&ev_)) == hipSuccess) h->ev.push_back(ev_);
  }
  if (e == hipSuccess) {
    if (h->ev_variant.size() <= (size_t)h->last_launches) h->ev_variant.resize(h->last_launches + 1), h->ev_wgs.resize(h->last_launches + 1);
    h->ev_variant[h->last_launches] = variant;
    h->ev_wgs[h->last_launches] = wgs;
    e = hipEventRecord(h->ev[2 * h->last_launches], st);
  }
  if (e != hipSuccess && h->prof_mu) h->prof_mu->unlock();
  HIPCHK(h, e);
  return GTO_OK;
}
static int prof_end(gto_handle* h, hipStream_t st) {
  const hipError_t e = hipEventRecord(h->ev[2 * h->last_launches + 1], st);
  h->last_launches++;
  if (h->prof_mu) h->prof_mu->unlock();
  HIPCHK(h, e);
  return GTO_OK;
}

using InitKernel = decltype(&k_lm_init<GTO_NB>);
static InitKernel lm_init_kernel(int np) { return np == GTO_NB ? k_lm_init<GTO_NB> : k_lm_init<16>; }

// What one obstacle launch covers.  The defaults are an evaluation of waypoints t_begin .. t_begin + nT - 1 of the batch.
struct ObsLaunch {
  int t_begin = 2, nT = 0;
  int fixed_mode = 0;       // 1: the init pass over the four virtual waypoints of the pinned ends (t_begin 0, nT 4)
  bool timed = false;       // profiling events around the launch (gto_set_profiling)
  bool goal_terms = false;  // goal-term workgroups in front of the obstacle workgroups (the solve loop's evaluations)
  int n_jobs = 0;           // evaluation jobs the grid is laid out for (0: the batch)
  int tg = 0;               // waypoints per workgroup (0: GTO_OBS_TG)
  bool deep = false;        // the variant with deep gather batches (few instances in flight)
  bool itemized = false;    // the regular workgroups walk the step kernel's list of (job, group) pairs
  int items_hint = 0;       // estimate of that list's length (0: its upper bound)
  const int32_t* rep = nullptr;  // the init pass: the instance whose start state instance b shares (k_init_heads; null: every instance computes)
};
static ObsLaunch init_pass(const int32_t* rep = nullptr) {
  ObsLaunch o;
  o.t_begin = 0, o.nT = 4, o.fixed_mode = 1, o.rep = rep;
  return o;
}

static int launch_obstacle(gto_handle* h, hipStream_t st, const BatchPtrs& bp, const SolveParams& sp, int B, const ObsLaunch& o) {
  // waypoints per workgroup: groups of h->tu.obs_tg (the two pinned waypoints form one group)
  const int TG = o.fixed_mode ? 1 : std::max(1, std::min(o.tg > 0 ? o.tg : h->tu.obs_tg, o.nT));  // the init pass has 4 virtual waypoints
  const ObsGeom geo(h->rb.n_cframes, h->rb.n_frames, h->rb.fk_rounds_c, h->rb.n_links, h->rb.n_opt, h->rb.n_chunks, TG, o.nT, h->np);
  const int nG = geo.nG;
  const int nb = o.n_jobs > 0 ? o.n_jobs : B;  // workgroups are laid out for the evaluation jobs there can be; B stays the batch (strides)
  int n_regular = obstacle_grid(nb, nG);
  // Itemized launches: laid out over the caller's estimate of the item list's length instead of its upper bound (nine
  // tenths of the workgroups of the upper bound find no item and leave; they cost the other lanes' launches dispatch
  // slots: +7 % trajectories/s without them); a crew of GTO_SWEEP_WGS workgroups at the end of the launch's grid walks
  // whatever the estimate missed (the kernel's SWEEP variant), so the result does not depend on it.
  const bool sweep = o.itemized && o.items_hint > 0 && o.items_hint + GTO_SWEEP_WGS < n_regular && bp.live != nullptr && !o.fixed_mode && !o.deep && h->np == GTO_NB;  // (the wide robots' launches are never itemized)
  if (sweep) n_regular = 8 * ((o.items_hint + 7) / 8);
  const size_t lds = (size_t)geo.lay.total_doubles * sizeof(double);
  const int n_crew = sweep ? GTO_SWEEP_WGS : 0;  // behind the regular workgroups: items n_regular, n_regular + 1, ... of the list, if there are any
  const dim3 grid(n_regular + n_crew + (o.goal_terms ? 8 * ((nb + 31) / 32) : 0));  // goal-term jobs: four to a workgroup, in front, a multiple of eight workgroups
  const bool deep_v = h->np == GTO_NB && o.deep;
  if (o.timed) {
    int rc_ = prof_begin(h, st, deep_v ? GTO_PROF_OBSTACLE_FEW : GTO_PROF_OBSTACLE, (long long)grid.x);
    if (rc_) return rc_;
  }
  BatchPtrs bpl = bp;  // the work counters of this variant (64 cells each)
  if (bpl.work) bpl.work += 64 * (deep_v ? GTO_PROF_OBSTACLE_FEW : GTO_PROF_OBSTACLE);
  // this round's job list and its length (the kernel's first, preloaded, arguments); null outside the solve loop
  const bool listed = bp.live != nullptr && !o.fixed_mode;
  const int32_t* jobs_par = listed ? bp.jobs + (size_t)sp.parity * bp.cap * sp.kcap : nullptr;
  const int32_t* njobs_par = listed ? bp.nlive + GTO_NJOBS(sp.parity) : nullptr;
  // rounds behind a step kernel that ran the broad phase itself: the regular workgroups are laid out over its list of (job, group) pairs
  const size_t items_cap = (size_t)bp.cap * sp.kcap * (sp.T - 2) + GTO_ITEM_SLACK;
  const int2* items_par = listed && o.itemized ? bp.items + (size_t)sp.parity * items_cap : nullptr;
  const int32_t* nitems_par = listed && o.itemized ? bp.nlive + 8 + sp.parity : (o.fixed_mode ? o.rep : nullptr);  // (the init pass has no list: rep[] rides here)
  const bool hot = !o.fixed_mode && sp.grad_mode == GTO_GRAD_CENTRAL_DIFF;
  hipLaunchKernelGGL(obstacle_kernel(h->np, o.deep, sweep, hot), grid, dim3(256), lds, st, jobs_par, njobs_par, items_par, nitems_par, geo.nG, geo.m_nG, n_regular, B,
                     h->d_rb, h->d_px, h->d_py, h->d_pz, h->d_chunks, h->d_scenes, bpl, sp, o.t_begin, o.nT, o.fixed_mode, geo, n_crew);
  if (o.timed) return prof_end(h, st);
  return GTO_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------- the solve loop
// At most W instances per lane are in flight; the step kernel of an instance that finishes puts the next one of its lane
// that has not started into the next round's live list, so every round works on a full house until the lane runs out,
// instead of dragging the tail of its slowest instances through ever emptier rounds.
//
// LANES.  A call's instances are dealt to up to lanes_max lanes (contiguous ranges of at least lane_min), each with a
// stream and lists of its own over the ONE workspace of the call (everything about an instance is indexed by its id in
// the batch): one lane's obstacle launch overlaps another's step launch while the GPU is full.  Each lane has a host
// thread of its own (lane 0: the caller's): a round of a lane with few instances in flight lasts 25-50 us and takes two
// launches to enqueue, which one thread cannot do for four lanes.  Towards the end of the call every lane is down to a
// handful of stragglers whose iterations are one dependent round each; four such chains sharing the command processor
// advance at 35-55 us a round where one alone takes 21-27, so a lane whose remaining instances are all in flight and at
// most adopt_below hands them to lane 0 (k_adopt), which then runs ONE chain for everybody.
struct LaneCtx {
  hipStream_t st = nullptr;
  BatchPtrs bp;
  SolveParams sp;
  int lo = 0, n = 0, W = 0, cap = 0;  // first instance, instances, in flight at the start, list capacity
  int room = 0;                       // positions its lists can have in use: W + what it adopted
  int span_prev = 0;                  // static positions: positions the current lists span (the last one-candidate launch's grid), 0: compact lists
  int n_resp = 0;                     // instances whose end this lane's finished-counter counts (own + adopted)
  int k = 0, known_done = 0, seen_round = -1, k_prev = 1;
  int last_plain = -1;                // the last round whose obstacle launch was not itemized (the length it published is no list's: 0)
  bool items_ready = false, pb_off = false, handed = false;
  bool seed_round0 = false;           // round 0 is itemized from the seed test: the length it publishes is a list's, but of seeds
  double ratio_max = 0.0;  // items per job, the largest the lane's rounds published
  long end_us = 0, few_us = 0;  // (GTO_LANE_DEBUG) when the lane's thread returned / enqueued its first few-instance round, from the start of the threads
  unsigned long long* h_prog = nullptr;
};

// A lane that hands what it has left to lane 0: behind the lane's last launch (its event)
struct Handover { int lane, parity, count, k_prev; };

// What the lanes of one solve call share: the call's shape, and the hand-over between lanes
struct SolveCall {
  gto_handle* h = nullptr;
  int B = 0, L = 1, T = 0, kcap = 1, nF = 0, max_iter = 0;
  int pb_ng = 1;         // waypoint groups of the step kernel's broad phase
  bool pb_able = false;  // that broad phase can run for this robot and call
  size_t lane_zws[GTO_MAX_LANES + 1] = {0};  // first block-inverse slot of each lane (wide robots)
  LaneCtx lanes[GTO_MAX_LANES];
  std::chrono::steady_clock::time_point tp_start;
  std::mutex mu;                     // hand-over requests, the error string, the profiling records
  std::vector<Handover> requests;
  int reserved = 0;                  // instances granted to lane 0 whose k_adopt it has not enqueued yet
  int adopt_limit = 0;
  std::atomic<int> rem0_pub{0}, others_open{0}, failed{0};
};

// (a) the lanes of a call: partition, lists in the call's buffers, streams and events, progress words, the broad phase's
// layout.  sp and bp are the call's; bp.work is set here when the call is profiled.
static int setup_lanes(gto_handle* h, hipStream_t st, SolveParams& sp, BatchPtrs& bp, SolveCall& c) {
  const int B = c.B, T = c.T, kcap = c.kcap, nF = c.nF;
  const int L = c.L = std::max(1, std::min(std::min(h->tu.lanes_max, GTO_MAX_LANES), B / std::max(1, h->tu.lane_min)));
  const int adopt_room = L > 1 ? (L - 1) * std::max(0, h->tu.adopt_below) : 0;
  size_t off_live[GTO_MAX_LANES + 1] = {0}, off_qfs[GTO_MAX_LANES + 1] = {0}, off_items[GTO_MAX_LANES + 1] = {0};
  for (int l = 0; l < L; ++l) {
    LaneCtx& ln = c.lanes[l];
    ln.lo = (int)((long long)B * l / L);
    ln.n = (int)((long long)B * (l + 1) / L) - ln.lo;
    ln.W = std::min(ln.n, h->tu.slots);
    ln.cap = ln.W + (l == 0 ? adopt_room : 0);
    ln.n_resp = ln.n;
    ln.room = ln.W;
    off_live[l + 1] = off_live[l] + 2 * (size_t)(1 + kcap) * ln.cap + 32;
    off_qfs[l + 1] = off_qfs[l] + 2 * (size_t)ln.cap * kcap * T * nF;
    off_items[l + 1] = off_items[l] + 2 * ((size_t)ln.cap * kcap * (T - 2) + GTO_ITEM_SLACK);
    c.lane_zws[l + 1] = c.lane_zws[l] + (size_t)ln.cap;
  }
  int rc;
  if ((rc = ensure(h, h->livebuf, off_live[L] * sizeof(int32_t)))) return rc;
  if ((rc = ensure(h, h->qfs, off_qfs[L] * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->itembuf, off_items[L] * sizeof(int2)))) return rc;
  if (h->np != GTO_NB && (rc = ensure(h, h->zws, c.lane_zws[L] * (size_t)(T - 2) * h->np * h->np * sizeof(double)))) return rc;
  for (int l = 0; l < L; ++l) {
    LaneCtx& ln = c.lanes[l];
    ln.sp = sp;
    ln.bp = bp;
    ln.bp.live = h->livebuf.as<int32_t>() + off_live[l];
    ln.bp.jobs = ln.bp.live + 2 * ln.cap;
    ln.bp.nlive = ln.bp.jobs + 2 * ln.cap * kcap;
    ln.bp.next = ln.bp.nlive + 4;
    ln.bp.qfs = h->qfs.as<double>() + off_qfs[l];
    ln.bp.items = h->np == GTO_NB ? h->itembuf.as<int2>() + off_items[l] : nullptr;
    ln.bp.n_done = h->ndone.as<int32_t>() + 16 * l;
    ln.bp.cap = ln.cap;
    ln.bp.b0 = ln.lo;
    ln.bp.w0 = ln.W;
    ln.bp.n_total = ln.lo + ln.n;
    ln.h_prog = h->h_progress.as<unsigned long long>() + 8 * l;
    ln.bp.progress = h->d_progress + 8 * l;
    // One lane: the caller's stream.  Several: streams of the handle's own, created one after the other -- the runtime deals
    // streams to its few hardware queues (GPU_MAX_HW_QUEUES, default 4) in the order of their creation, and two lanes on
    // one queue run one after the other (the caller's stream next to three new ones: 126 k trajectories/s instead of 225 k);
    // the caller's stream carries the start and the end of the call and waits in between.
    if (L == 1) ln.st = st;
    else if (l < h->n_user_lane_streams) ln.st = h->user_lane_stream[l];  // gto_set_lane_streams
    else {
      if (!h->lane_stream[l]) {
        // Streams of the greatest priority: the runtime gives them hardware queues of their own, one per stream in the
        // order of creation, so four lanes sit behind four dispatcher pipes.  Streams of the default priority share the
        // process's four queues with every other stream it has created, and two lanes whose queues sit behind one pipe
        // split its workgroup dispatch rate (the evaluation launch, five thousand mostly empty workgroups, 75 us instead
        // of 48; rocprofv3 queue ids 1 and 5 in traces of round 5): 118 k instead of 196 k trajectories/s for one call of
        // 1280 instances.
        int lo_p = 0, hi_p = 0;
        HIPCHK(h, hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));  // (least, greatest): greatest is the smaller number
        HIPCHK(h, hipStreamCreateWithPriority(&h->lane_stream[l], hipStreamNonBlocking, hi_p));
      }
      ln.st = h->lane_stream[l];
    }
    if (!h->lane_event[l]) HIPCHK(h, hipEventCreateWithFlags(&h->lane_event[l], hipEventDisableTiming));
  }
  HIPCHK(h, hipMemsetAsync(h->ndone.get(), 0, 16 * sizeof(int32_t) * L, st));
  // the finished-counter and the round counter reach the host through words in pinned memory that the step kernel
  // writes; the tag tells this call's values from what the last launches of the previous call may still be writing
  h->progress_tag = h->progress_tag + 1 ? h->progress_tag + 1 : 1;
  for (int l = 0; l < L; ++l) c.lanes[l].bp.progress_tag = (unsigned long long)h->progress_tag << 32;
  if (h->profiling) {
    if ((rc = ensure(h, h->counters, GTO_PROF_VARIANTS * 64 * sizeof(unsigned long long)))) return rc;
    HIPCHK(h, hipMemsetAsync(h->counters.get(), 0, GTO_PROF_VARIANTS * 64 * sizeof(unsigned long long), st));
    bp.work = h->counters.as<unsigned long long>();  // 64 cells per kernel variant (launch_obstacle picks the variant's)
    for (int l = 0; l < L; ++l) c.lanes[l].bp.work = bp.work;
  }
  // The broad phase ahead of the obstacle launch, in the rounds that fill the GPU: the step kernel settles the waypoint
  // groups none of whose bounding spheres can reach a non-zero voxel record and lists the others (prebroad_tail); the
  // launch is laid out over that list.  Needs: the groups of the launch it feeds (consecutive waypoints), room for one
  // pass in the step kernel's dead LDS, at most GTO_PB_PARK parked frames in its serial walk over the kinematic tree.
  const int pb_tg = std::max(1, std::min(h->tu.obs_tg, T - 2));
  c.pb_ng = (T - 2 + pb_tg - 1) / pb_tg;
  const PbLayout pbl(T, h->rb.n_frames, h->pb_C, h->rb.pb_npar);
  c.pb_able = h->tu.prebroad && h->np == GTO_NB && c.pb_ng <= 64 && h->tu.obs_interleave != 1 && h->rb.n_xst <= GTO_PB_PARK && pbl.pw >= 1 && h->pb_C >= 1;
  for (int l = 0; l < L; ++l) {
    SolveParams& lsp = c.lanes[l].sp;
    lsp.pb_tg = pb_tg, lsp.pb_ng = c.pb_ng, lsp.pb_pw = std::max(1, pbl.pw), lsp.pb_tab0 = pbl.tab0;
    lsp.pb_verify = h->tu.dbg_cut == 10;
  }
  sp.pb_tg = pb_tg, sp.pb_ng = c.pb_ng, sp.pb_pw = std::max(1, pbl.pw), sp.pb_tab0 = pbl.tab0;
  return GTO_OK;
}

// The init pass of a solve call, behind k_lm_init (it indexes the batch directly): ss_fixed of every instance.  A call whose
// init pass is more than init_dedup_min workgroups runs it once per run of equal start states: k_init_heads names every
// instance's representative, the workgroups of the others leave at once, k_ss_fixed_spread hands them the four numbers.
static int run_init_pass(gto_handle* h, hipStream_t st, const BatchPtrs& bp, const SolveParams& sp, int B) {
  if (!h->tu.init_dedup || 4 * (long long)B <= h->tu.init_dedup_min) return launch_obstacle(h, st, bp, sp, B, init_pass());
  int32_t* rep = h->inithead.as<int32_t>();
  hipLaunchKernelGGL(k_init_heads, dim3((B + 255) / 256), dim3(256), 0, st, h->d_rb, bp, sp.T, B, rep);
  const int rc = launch_obstacle(h, st, bp, sp, B, init_pass(rep));
  if (rc) return rc;
  hipLaunchKernelGGL(k_ss_fixed_spread, dim3((B + 255) / 256), dim3(256), 0, st, bp, B, rep);
  return GTO_OK;
}

// The seeds of the instances that wait for a slot, tested against the distance field once, behind the init pass (k_seed_broad
// needs ss_fixed and qf): lanes with more instances than slots whose full rounds run the step kernel's broad phase
// (plan_round's pb_ok).  A call without such a lane launches nothing and keeps null masks: every group of a seed is listed.
static int test_waiting_seeds(gto_handle* h, hipStream_t st, SolveCall& c) {
  if (!c.pb_able || !h->tu.seed_pb) return GTO_OK;
  for (int l = 0; l < c.L; ++l) {
    LaneCtx& ln = c.lanes[l];
    if (ln.n <= ln.W || ln.W <= h->tu.few_instances) continue;
    int rc;
    if (h->profiling && (rc = prof_begin(h, st, GTO_PROF_SEED_TEST, ln.n - ln.W))) return rc;
    hipLaunchKernelGGL(k_seed_broad, dim3(ln.n - ln.W), dim3(256), h->lm_lds, st, h->d_rb, ln.bp, ln.sp, c.B, h->seedmask.as<unsigned long long>(), 0);
    if (h->profiling && (rc = prof_end(h, st))) return rc;
    ln.bp.seed_mask = h->seedmask.as<unsigned long long>();
    // ... and the seeds that start in a slot, which lists what is left of them for round 0: that round is then planned as
    // an itemized launch like every full round behind it (plan_round: the estimate is the previous call's items per job,
    // or the upper bound).  The length round 0 publishes is a list of SEEDS: it says nothing about the lists of trial
    // points behind it (a Fetch whose seed rests in front of the shelf lists a fifth of what it lists eight rounds later,
    // and a crew of 64 walked the rest of a launch laid out over 1.5 x that: 3.1 ms for one round), so no estimate is taken
    // from it (seed_round0), as none was taken from the 0 a plain round 0 publishes
    if (h->tu.seed_pb_all) {
      hipLaunchKernelGGL(k_seed_broad, dim3(ln.W), dim3(256), h->lm_lds, st, h->d_rb, ln.bp, ln.sp, c.B, h->seedmask.as<unsigned long long>(), 1);
      ln.items_ready = ln.seed_round0 = true;
    }
  }
  return GTO_OK;
}

// A round of a lane: one obstacle launch that evaluates the candidate trial trajectories of the instances in flight, one
// step launch that accepts, solves and makes new candidates.
enum StepVariant { STEP_FULL, STEP_FEW, STEP_WIDE };  // k_lm_step<4, 1>, k_lm_step<8, GTO_KSPEC>, k_lm_step_wide<16>
struct RoundPlan {
  int in_flight = 0;
  int span = 0;            // positions this round's lists span: the step launch's grid
  bool few = false;        // at most few_instances in flight
  bool interleave = false;  // SolveParams::interleave
  ObsLaunch obs;           // the obstacle launch
  StepVariant step = STEP_FULL;
  int k_acc = 1, k_rej = 1, spec_streak = 0;  // STEP_FEW: candidates after an accept / a rejection, SolveParams::spec_streak
  bool pb_next = false, static_pos = false;   // STEP_FULL: the broad phase of the next round, static list positions
  int k_next = 1;          // candidates per instance the step launch generates (the next round's k_prev)
  bool pb_off = false;     // the lane's broad phase stays off from now on
  double ratio_max = 0.0;  // the lane's largest items per job so far
};

// (b) what the next round of lane ln launches, from the tunables and the lane's state.  No HIP call, no allocation, no
// lock: rounds with few instances in flight last 25-60 us and are bound by how fast the host enqueues them.
static RoundPlan plan_round(const gto_handle* h, const SolveCall& c, const LaneCtx& ln) {
  const Tunables& tu = h->tu;
  RoundPlan p;
  p.in_flight = std::min(ln.room, ln.n_resp - ln.known_done);
  p.few = p.in_flight <= tu.few_instances;
  // compact lists hold the instances in flight; lists of a launch with static positions keep that launch's span
  // (instances that finished without a successor left void positions behind)
  p.span = ln.span_prev ? ln.span_prev : p.in_flight;
  p.interleave = tu.obs_interleave == 1 || (tu.obs_interleave == 2 && p.few);
  p.pb_off = ln.pb_off;
  p.ratio_max = ln.ratio_max;
  p.k_next = ln.k_prev;
  const bool large_call = ln.n_resp > tu.spec_deep;  // (its tail: the other lanes' launches are on the GPU, too)
  ObsLaunch& o = p.obs;
  o.nT = c.T - 2;
  o.timed = h->profiling;
  o.goal_terms = true;
  o.n_jobs = p.span * ln.k_prev;
  o.tg = p.few ? (large_call ? tu.obs_tg_few_tail : tu.obs_tg_few) : tu.obs_tg;
  o.deep = p.few && tu.obs_deep && p.in_flight <= GTO_OBS_DEEP_MAX;
  o.itemized = ln.items_ready && !p.few;
  // length of this round's item list, estimated: what the lane's step launches published last (a few rounds old; the
  // list changes by a few per cent a round), or, until then, the previous call's ratio of items to jobs
  if (o.itemized && tu.item_grid) {
    const unsigned long long p2 = __atomic_load_n(ln.h_prog + 2, __ATOMIC_RELAXED);
    const int jobs_bound = p.in_flight * ln.k_prev;
    // (a published 0 is a list's length only if the launch that published it was itemized: the word is that of round
    // seen_round - 1 at the earliest.  A call whose seeds k_seed_broad settled whole and whose instances stay clear of
    // the field has empty lists round after round, and its launches are laid out over the estimate's floor, not the bound)
    const bool zero_ok = ln.last_plain < ln.seen_round - 1;
    const bool of_seeds = ln.seed_round0 && ln.seen_round < 2;  // (the word may still be round 0's)
    if ((unsigned)(p2 >> 32) == h->progress_tag && ((p2 & 0xfffffull) > 0 || zero_ok) && !of_seeds && (p2 & 0xfffffull) < 0xfffffull) {
      const double items_seen = (double)(p2 & 0xfffffull), jobs_seen = (double)((p2 >> 20) & 0xfffull);
      o.items_hint = (int)(1.5 * items_seen) + 256;
      if (jobs_seen > 0 && jobs_seen < 4095) p.ratio_max = std::max(p.ratio_max, items_seen / jobs_seen);
    } else if (h->items_per_job_prior > 0.0) {
      o.items_hint = (int)(1.25 * h->items_per_job_prior * jobs_bound) + 256;
    }
    if (tu.item_hint_forced > 0) o.items_hint = tu.item_hint_forced;  // (tests: a launch of a few workgroups, the crew does the rest)
  }
  if (h->np != GTO_NB) {
    p.step = STEP_WIDE;
  } else if (p.few && tu.step_nw_few == 8) {
    // few instances in flight: eight waves per instance and candidate trial points ahead of their evaluation
    p.step = STEP_FEW;
    const int k_budget = std::max(1, tu.spec_jobs / std::max(1, p.in_flight));
    p.k_acc = p.in_flight <= std::min(tu.spec_deep, tu.spec_few) ? std::min(std::min(large_call ? tu.spec_acc_tail : tu.spec_acc, k_budget), h->spec_kmax) : 1;
    p.spec_streak = large_call ? tu.spec_streak_tail : tu.spec_streak;
    p.k_rej = p.in_flight <= tu.spec_few ? std::min(std::max(std::min(tu.spec_rej, k_budget), tu.spec_rej_few), h->spec_kmax) : 1;
    p.k_next = std::max(p.k_acc, p.k_rej);
  } else {
    p.step = STEP_FULL;
    const bool pb_ok = c.pb_able && std::min(ln.W, ln.n) > tu.few_instances;
    // a call in which the broad phase settles next to nothing (a robot inside a shelf) stops running it: the last
    // itemized round the host has seen listed more than 1 - GTO_PB_MIN_GAIN of its (job, group) pairs
    if (pb_ok && !p.pb_off && !ln.sp.pb_verify) {
      const unsigned long long p2 = __atomic_load_n(ln.h_prog + 2, __ATOMIC_RELAXED);
      if ((unsigned)(p2 >> 32) == h->progress_tag) {
        const double jobs_seen = (double)((p2 >> 20) & 0xfffull), items_seen = (double)(p2 & 0xfffffull);
        if (jobs_seen > 0 && items_seen > 0 && jobs_seen < 4095 && ln.k >= 12 && items_seen > (1.0 - tu.pb_min_gain) * jobs_seen * c.pb_ng) p.pb_off = true;
      }
    }
    p.pb_next = pb_ok && !p.pb_off && !p.few;
    p.static_pos = tu.static_pos && c.L == 1 && !p.few;
    p.k_next = 1;
  }
  return p;
}

// (c) enqueues the round the plan describes on the lane's stream, and moves the lane to the next round
static int enqueue_round(gto_handle* h, const SolveCall& c, LaneCtx& ln, int lane_index, const RoundPlan& p) {
  const int B = c.B, T = c.T;
  SolveParams& lsp = ln.sp;
  lsp.interleave = p.interleave;
  lsp.round = ln.k;
  lsp.parity = ln.k & 1;
  lsp.k_eval = ln.k_prev;  // the goal workgroups skip fresh instances themselves: k_lm_init already produced the seed's goal terms
  int rc;
  if ((rc = launch_obstacle(h, ln.st, ln.bp, lsp, B, p.obs))) return rc;
  // the narrow step kernels by class of trajectory length: the instantiation unrolled for GTO_STEP_T_SHORT waypoints where
  // the call's T allows it (same results; GTO_STEP_TCLASS=0: the general one at every T)
  const bool t_short = h->tu.step_tclass && T <= GTO_STEP_T_SHORT;
  // ... and at the one length the reference and every shipped configuration run at, the instantiation with T a constant
  // (k_lm_step_t50: same results; GTO_STEP_TEXACT=0: the choice above)
  const bool t_exact = h->tu.step_texact && T == GTO_STEP_T_EXACT;
  if (h->dbg && p.step != STEP_WIDE) h->dbg_step_launches[t_exact ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
  if (h->profiling && (rc = prof_begin(h, ln.st, p.step == STEP_FEW ? GTO_PROF_STEP_FEW : GTO_PROF_STEP, p.in_flight))) return rc;
  if (p.step == STEP_FEW) {
    lsp.k_acc = p.k_acc, lsp.k_rej = p.k_rej, lsp.spec_streak = p.spec_streak;
    lsp.pb_next = 0, lsp.static_pos = 0;
    if (t_exact) hipLaunchKernelGGL((k_lm_step_t50<8, GTO_KSPEC>), dim3(p.span), dim3(512), lm_lds_bytes(T, p.k_next), ln.st, h->d_rb, ln.bp, lsp, B);
    else if (t_short) hipLaunchKernelGGL((k_lm_step_short<8, GTO_KSPEC>), dim3(p.span), dim3(512), lm_lds_bytes(T, p.k_next), ln.st, h->d_rb, ln.bp, lsp, B);
    else hipLaunchKernelGGL((k_lm_step<8, GTO_KSPEC>), dim3(p.span), dim3(512), lm_lds_bytes(T, p.k_next), ln.st, h->d_rb, ln.bp, lsp, B);
  } else if (p.step == STEP_FULL) {
    lsp.k_acc = lsp.k_rej = 1;
    lsp.pb_next = p.pb_next, lsp.static_pos = p.static_pos;
    if (t_exact) hipLaunchKernelGGL((k_lm_step_t50<4, 1>), dim3(p.span), dim3(256), h->lm_lds, ln.st, h->d_rb, ln.bp, lsp, B);
    else if (t_short) hipLaunchKernelGGL((k_lm_step_short<4, 1>), dim3(p.span), dim3(256), h->lm_lds, ln.st, h->d_rb, ln.bp, lsp, B);
    else hipLaunchKernelGGL((k_lm_step<4, 1>), dim3(p.span), dim3(256), h->lm_lds, ln.st, h->d_rb, ln.bp, lsp, B);
  } else {
    hipLaunchKernelGGL(k_lm_step_wide<16>, dim3(p.in_flight), dim3(GTO_WIDE_NT), h->lm_lds, ln.st, h->d_rb, ln.bp, lsp, B,
                       h->zws.as<double>() + (size_t)c.lane_zws[lane_index] * (T - 2) * h->np * h->np);
  }
  if (h->profiling && (rc = prof_end(h, ln.st))) return rc;
  ln.span_prev = p.static_pos ? p.span : 0;
  if (!p.obs.itemized) ln.last_plain = ln.k;
  ln.items_ready = p.pb_next;
  ln.k_prev = p.k_next;
  ln.pb_off = p.pb_off;
  ln.ratio_max = p.ratio_max;
  ln.k++;
  return GTO_OK;
}

static void read_progress(unsigned tag, LaneCtx& ln) {
  const unsigned long long p0 = __atomic_load_n(ln.h_prog, __ATOMIC_RELAXED), p1 = __atomic_load_n(ln.h_prog + 1, __ATOMIC_RELAXED);
  if ((unsigned)(p0 >> 32) == tag) ln.known_done = std::max(ln.known_done, (int)(p0 & 0xffffffffull));
  if ((unsigned)(p1 >> 32) == tag) ln.seen_round = std::max(ln.seen_round, (int)(p1 & 0xffffffffull));
}

// (d) waits until lane ln may enqueue its next round (throttle: never more than `ahead` rounds in front of the last step
// launch seen running, so that the launches stay sized to what is left and the empty rounds after the last instance
// finishes stay few; sleep-poll, not a blocking wait: the runtime spins in those, one host core per lane)
static int throttle(SolveCall& c, LaneCtx& ln) {
  gto_handle* h = c.h;
  for (long naps = 0;; ++naps) {
    read_progress(h->progress_tag, ln);
    const bool few = std::min(ln.room, ln.n_resp - ln.known_done) <= h->tu.few_instances;
    if (ln.k - ln.seen_round <= (few ? h->tu.ahead_few : h->tu.ahead) + 1 || c.failed.load(std::memory_order_relaxed)) return GTO_OK;
    std::this_thread::sleep_for(std::chrono::microseconds(few ? GTO_NAP_FEW_US : GTO_NAP_US));
    if ((naps & 1023) == 1023) {  // a stream that went idle or failed without reaching the round: do not wait for ever
      const hipError_t qe = hipStreamQuery(ln.st);
      if (qe != hipErrorNotReady) {
        read_progress(h->progress_tag, ln);
        if (ln.k - ln.seen_round > (few ? h->tu.ahead_few : h->tu.ahead) + 1) {
          std::lock_guard<std::mutex> g(c.mu);
          h->err = qe == hipSuccess ? "solve loop: the stream went idle before the rounds it was given ran" : std::string("solve loop: ") + hipGetErrorString(qe);
          return GTO_ERR_HIP;
        }
      }
    }
  }
}

// (d) the host thread of lane l: throttle, hand-overs, rounds until the lane is done
static void lane_main(SolveCall& c, int l) {
  gto_handle* h = c.h;
  LaneCtx& ln = c.lanes[l];
  (void)hipSetDevice(h->device);
  const int old_slack_ = prctl(PR_GET_TIMERSLACK);
  if (l > 0 && old_slack_ > 1000) (void)prctl(PR_SET_TIMERSLACK, 1000UL);
  int rc_ = GTO_OK;
  for (;;) {
    if (c.failed.load(std::memory_order_relaxed)) break;
    if ((rc_ = throttle(c, ln))) break;
    int remaining = ln.n_resp - ln.known_done;
    if (l == 0) {
      // hand-overs granted since the last round: behind the lane's last launch (its event) and behind this lane's
      {
        std::lock_guard<std::mutex> g(c.mu);
        for (const Handover& r : c.requests) {
          LaneCtx& src = c.lanes[r.lane];
          if (hipStreamWaitEvent(ln.st, h->lane_event[r.lane], 0) != hipSuccess) { h->err = "solve loop: hand-over between lanes failed"; rc_ = GTO_ERR_HIP; break; }
          hipLaunchKernelGGL(k_adopt, dim3(1), dim3(256), 0, ln.st, src.bp, r.parity, ln.bp, ln.k & 1, c.kcap, c.T * c.nF, src.n_resp, r.count);
          ln.n_resp += r.count;
          ln.room = std::min(ln.cap, ln.room + r.count);
          ln.k_prev = std::max(ln.k_prev, r.k_prev);
          ln.items_ready = false;
          c.reserved -= r.count;
        }
        c.requests.clear();
        remaining = ln.n_resp - ln.known_done;
        c.rem0_pub.store(std::max(0, remaining), std::memory_order_relaxed);
      }
      if (rc_) break;
      if (remaining <= 0) {
        if (c.others_open.load(std::memory_order_acquire) == 0) {
          std::lock_guard<std::mutex> g(c.mu);
          if (c.requests.empty()) break;
          continue;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(10));
        continue;
      }
    } else {
      if (remaining <= 0) break;
      // hand-over: everything this lane has left is in flight (remaining <= W) and few, and lane 0 has room
      if (h->tu.adopt_below > 0 && remaining <= h->tu.adopt_below && remaining <= ln.W && ln.k > 0) {
        std::lock_guard<std::mutex> g(c.mu);
        const int rem0 = c.rem0_pub.load(std::memory_order_relaxed);
        if (rem0 <= c.lanes[0].W && rem0 + c.reserved + remaining <= c.adopt_limit) {
          if (hipEventRecord(h->lane_event[l], ln.st) != hipSuccess) { h->err = "solve loop: hand-over between lanes failed"; rc_ = GTO_ERR_HIP; break; }
          c.reserved += remaining;
          c.requests.push_back({l, ln.k & 1, remaining, ln.k_prev});
          ln.handed = true;
          break;
        }
      }
    }
    const int max_rounds = ((ln.n_resp + ln.W - 1) / std::max(1, ln.W) + 1) * (c.max_iter + 2) + 8;
    if (ln.k > max_rounds) {
      std::lock_guard<std::mutex> g(c.mu);
      h->err = "solve loop: a lane ran out of rounds";
      rc_ = GTO_ERR_HIP;
      break;
    }
    const RoundPlan plan = plan_round(h, c, ln);
    if (plan.few && !ln.few_us) ln.few_us = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - c.tp_start).count();
    if ((rc_ = enqueue_round(h, c, ln, l, plan))) break;
  }
  if (rc_) c.failed.store(rc_, std::memory_order_relaxed);
  ln.end_us = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - c.tp_start).count();
  if (l > 0) {
    c.others_open.fetch_sub(1, std::memory_order_release);
    if (old_slack_ > 1000) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old_slack_);
  }
}

// (d) runs the lanes (lane 0 on the calling thread) and returns the first error of any of them
static int run_lanes(SolveCall& c) {
  gto_handle* h = c.h;
  const int L = c.L;
  c.rem0_pub.store(c.lanes[0].n), c.others_open.store(L - 1), c.failed.store(0);
  c.adopt_limit = std::min(h->tu.few_instances, c.lanes[0].cap);
  h->prof_mu = L > 1 ? &c.mu : nullptr;
  const auto tp0 = std::chrono::steady_clock::now();
  std::vector<std::thread> workers;
  for (int l = 1; l < L; ++l) workers.emplace_back(lane_main, std::ref(c), l);
  const auto tp1 = std::chrono::steady_clock::now();
  lane_main(c, 0);
  const auto tp2 = std::chrono::steady_clock::now();
  for (auto& w : workers) w.join();
  const auto tp3 = std::chrono::steady_clock::now();
  h->prof_mu = nullptr;
  if (h->tu.lane_debug) {
    auto us = [](auto a, auto b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
    fprintf(stderr, "[gto lanes] B %d L %d: threads started %ld us | lane 0 returned %ld us | joined %ld us | rounds", c.B, L, us(tp0, tp1), us(tp0, tp2), us(tp0, tp3));
    for (int l = 0; l < L; ++l) fprintf(stderr, " %d%s@%ld(few@%ld)", c.lanes[l].k, c.lanes[l].handed ? "h" : "", c.lanes[l].end_us, c.lanes[l].few_us);
    fprintf(stderr, "\n");
  }
  return c.failed.load();
}

// (e) gto_last_kernel_profile / _time / _work of a profiled call: the events and work counters of its launches
static int harvest_profile(gto_handle* h, hipStream_t st, const unsigned long long* work) {
  HIPCHK(h, hipStreamSynchronize(st));
  for (int v = 0; v < GTO_PROF_VARIANTS; ++v) h->prof_ms[v] = 0.0, h->prof_launches[v] = h->prof_wgs[v] = 0, h->prof_points[v] = 0;
  int n_obs = 0;
  for (int i = 0; i < h->last_launches; ++i) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]));
    const int v = h->ev_variant[i];
    h->prof_ms[v] += ms, h->prof_launches[v] += 1, h->prof_wgs[v] += h->ev_wgs[i];
    n_obs += v == GTO_PROF_OBSTACLE || v == GTO_PROF_OBSTACLE_FEW;
  }
  unsigned long long cells[GTO_PROF_VARIANTS * 64];
  HIPCHK(h, hipMemcpy(cells, work, sizeof cells, hipMemcpyDeviceToHost));
  for (int v = 0; v < GTO_PROF_VARIANTS; ++v)
    for (int c = 0; c < 64; ++c) h->prof_points[v] += cells[64 * v + c];
  // gto_last_kernel_time / _work: the obstacle kernel, both variants together (what they always reported)
  h->last_ms = h->prof_ms[GTO_PROF_OBSTACLE] + h->prof_ms[GTO_PROF_OBSTACLE_FEW];
  h->last_launches = n_obs;
  h->last_counters[0] = h->prof_points[GTO_PROF_OBSTACLE] + h->prof_points[GTO_PROF_OBSTACLE_FEW];
  h->last_counters[1] = 0;
  return GTO_OK;
}

// (f) GTO_DEBUG_TIMING: the phase stamps the kernels of the call left in h->dbg
static int print_debug_stamps(gto_handle* h, hipStream_t st) {
  HIPCHK(h, hipStreamSynchronize(st));
  long long t[256];
  HIPCHK(h, hipMemcpy(t, h->dbg.get(), sizeof t, hipMemcpyDeviceToHost));
  fprintf(stderr, "[gto dbg] step-kernel phases (cycles) P0+P1 %lld | P2 %lld | diag %lld | dense %lld | back %lld | P4 %lld | P5 %lld | s_dense %lld\n",
          t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4], t[6] - t[5], t[7] - t[6], t[9]);
  fprintf(stderr, "[gto dbg] narrow step launches of the call: %d of k_lm_step_t50 (T = %d a constant), %d of the others\n",
          h->dbg_step_launches[1].exchange(0), GTO_STEP_T_EXACT, h->dbg_step_launches[0].exchange(0));
  if (h->np != GTO_NB)
    fprintf(stderr, "[gto dbg] wide step kernel, sweeps (cycles): downward: %lld in %lld dense inversions, sweep %lld | upward: %lld in %lld dense inversions, sweep %lld\n",
            t[56], t[57], t[58], t[59], t[60], t[61]);
  fprintf(stderr, "[gto dbg] solve by wave (cycles from the start of P3): downward sweep: diagonal stretch %lld, its dense blocks %lld | upward sweep %lld | meeting block %lld | back substitution from its start: downward wave dense %lld, diagonal stretch %lld | upward wave %lld\n",
          t[3] - t[2], t[41] - t[2], t[17] - t[2], t[42] - t[4], t[18] - t[42], t[19] - t[42], t[26] - t[42]);
  fprintf(stderr, "[gto dbg] sweeps of the other candidates' waves (2..6) done at (cycles from the start of P3, 0 = no candidate): %lld %lld %lld %lld %lld | barrier passed at %lld\n",
          t[43] ? t[43] - t[2] : 0, t[44] ? t[44] - t[2] : 0, t[45] ? t[45] - t[2] : 0, t[46] ? t[46] - t[2] : 0, t[47] ? t[47] - t[2] : 0, t[4] - t[2]);
  fprintf(stderr, "[gto dbg] tail tables fetched by waves 2-3 during the back substitution (cycles from its start): in at %lld %lld | its barrier passed at %lld\n",
          t[51] ? t[51] - t[42] : 0, t[52] ? t[52] - t[42] : 0, t[5] - t[42]);
  fprintf(stderr, "[gto dbg] broad phase in the step kernel's tail (cycles): entry+tables %lld | barrier %lld | A (local transforms, pass 0) %lld | B (chain) %lld | C (sphere tests) %lld | other passes %lld | outputs %lld\n",
          t[33] - t[6], t[34] - t[33], t[35] - t[34], t[36] - t[35], t[37] - t[36], t[38] - t[37], t[39] - t[38]);
  fprintf(stderr, "[gto dbg] P2 split (cycles): loads+barrier %lld | b-vector+masks %lld | blocks %lld | e,y+barrier %lld\n", t[28] - t[1], t[29] - t[28], t[30] - t[29], t[2] - t[30]);
  fprintf(stderr, "[gto dbg] fk_mfma_tree (cycles): local %lld | rounds %lld %lld %lld %lld | outputs %lld\n", t[21] - t[20], t[22] - t[21], t[23] - t[22], t[24] - t[23], t[25] - t[24], t[27] - t[25]);
  // (only with -DGTO_DEBUG_LONGEST_WG: the extra clocks cost the tuned obstacle kernel registers)
  fprintf(stderr, "[gto dbg] longest regular obstacle workgroup of the call: %lld cycles with %lld surviving chunks | goal-term wavefront of instance 0: %lld cycles\n",
          t[40] >> 16, t[40] & 0xffff, t[32] - t[31]);
  if (t[64] || t[65]) {  // -DGTO_DEBUG_LONGEST_WG
    long long tot_ = 0;
    for (int i = 64; i < 128; ++i) tot_ += t[i];
    fprintf(stderr, "[gto dbg] regular obstacle workgroups of the call: %lld, none of whose keys got a contribution: %lld | surviving chunks per workgroup (0,1,2,...,63+):", tot_, t[48]);
    for (int i = 64; i < 128; ++i) fprintf(stderr, " %lld", t[i]);
    fprintf(stderr, "\n");
    fprintf(stderr, "[gto dbg] ticks those workgroups ran, summed by surviving chunks (0,1,2,...,63+):");
    for (int i = 192; i < 256; ++i) fprintf(stderr, " %lld", t[i]);
    fprintf(stderr, "\n");
  }
  fprintf(stderr, "[gto dbg] broad phase of the step kernel (GTO_DEBUG_CUT=10, -DGTO_DEBUG_LONGEST_WG: settled groups are looked at anyway): %lld groups settled, %lld of them with a surviving chunk, %lld with a CONTRIBUTION (must be 0)\n", t[49], t[50], t[55]);
  {
    fprintf(stderr, "[gto dbg] workgroups without a surviving chunk by the index shift their closest chunk tolerates (0,1,2,...,63+):");
    for (int i = 128; i < 192; ++i) fprintf(stderr, " %lld", t[i]);
    fprintf(stderr, "\n");
  }
  fprintf(stderr, "[gto dbg] obstacle WG (b=0,t=T-1) cycles: prologue %lld | broad %lld | loop %lld | epilogue %lld | active chunks %lld | prologue up to the chain %lld\n",
          t[11] - t[10], t[12] - t[11], t[13] - t[12], t[14] - t[13], t[15], t[16] - t[10]);
  return GTO_OK;
}

// ------------------------------------------------------------------------------------------------- host-pointer staging
// The transfers of one call of a host-pointer entry point.  Every input and every output takes the next staging slot of
// its direction (gto_handle::in / out and their pinned twins) in the order it is registered; a null host array takes
// its slot too, gets a null device pointer and costs nothing.  An output states its size once, when it is registered.
// finish() queues the device -> pinned copies in registration order, syncs the stream once and copies pinned -> the
// caller's arrays.  What is to be delivered lives here, not on the handle: a call that returns early delivers nothing.
class Staging {
 public:
  explicit Staging(gto_handle* h) : h_(h) {}

  // n elements from the host, copied to the device on the handle's stream
  template <class T>
  int in(const T* src, size_t n, const T** dptr) {
    *dptr = nullptr;
    if (n_in_ == GTO_STAGE_SLOTS) return too_many();
    const int k = n_in_++;
    if (!src) return GTO_OK;
    const size_t bytes = n * sizeof(T);
    int rc = ensure(h_, h_->in[k], bytes);
    if (rc) return rc;
    if ((rc = ensure(h_, h_->pin_in[k], bytes))) return rc;  // free again: every entry point ends with a stream sync
    memcpy(h_->pin_in[k].get(), src, bytes);
    HIPCHK(h_, hipMemcpyAsync(h_->in[k].get(), h_->pin_in[k].get(), bytes, hipMemcpyHostToDevice, h_->stream));
    *dptr = h_->in[k].as<const T>();
    return GTO_OK;
  }
  // n elements for the host, delivered by finish()
  template <class T>
  int out(T* host, size_t n, T** dptr) { return take_out(host, n * sizeof(T), host != nullptr, dptr); }
  // n elements the kernel writes and nobody fetches
  template <class T>
  int scratch(size_t n, T** dptr) { return take_out((T*)nullptr, n * sizeof(T), true, dptr); }

  int finish() {
    for (int k = 0; k < n_out_; ++k) {
      if (!host_[k]) continue;
      int rc = ensure(h_, h_->pin_out[k], bytes_[k]);
      if (rc) return rc;
      HIPCHK(h_, hipMemcpyAsync(h_->pin_out[k].get(), h_->out[k].get(), bytes_[k], hipMemcpyDeviceToHost, h_->stream));
    }
    HIPCHK(h_, hipStreamSynchronize(h_->stream));
    for (int k = 0; k < n_out_; ++k)
      if (host_[k]) memcpy(host_[k], h_->pin_out[k].get(), bytes_[k]);
    return GTO_OK;
  }

 private:
  template <class T>
  int take_out(T* host, size_t bytes, bool on_device, T** dptr) {
    *dptr = nullptr;
    if (n_out_ == GTO_STAGE_SLOTS) return too_many();
    const int k = n_out_++;
    host_[k] = host;
    bytes_[k] = bytes;
    if (!on_device) return GTO_OK;
    const int rc = ensure(h_, h_->out[k], bytes);
    if (rc) return rc;
    *dptr = h_->out[k].as<T>();
    return GTO_OK;
  }
  int too_many() { return fail(h_, GTO_ERR_UNSUPPORTED, "internal: more than ten staged arrays of one direction"); }

  gto_handle* h_;
  int n_in_ = 0, n_out_ = 0;
  void* host_[GTO_STAGE_SLOTS] = {};  // the caller's array of output slot k (null: not fetched)
  size_t bytes_[GTO_STAGE_SLOTS] = {};
};

extern "C" {

int gto_solve_batch_device(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id, const double* qc,
                           const double* goals, const int32_t* n_goals, const double* standoff, const double* base_pos,
                           const double* Q0, double* Q_out, double* dQ_out, double* cost_out, int32_t* iters_out,
                           int32_t* status_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || n_max < 1) return fail(h, GTO_ERR_INVALID_ARG, "B must be >= 0 and n_max >= 1");
  if (B == 0) return GTO_OK;
  if (B > GTO_JOB_MASK) return fail(h, GTO_ERR_UNSUPPORTED, "more than 16.7 million instances in one call");
  if (!scene_id || !qc || !goals || !n_goals || !base_pos || !Q0) return fail(h, GTO_ERR_INVALID_ARG, "null input array");
  if (h->scenes.empty()) return fail(h, GTO_ERR_NO_SCENE, "no scene has been set");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  int rc = ensure_workspace(h, B);
  if (rc) return rc;
  SolveParams sp = make_params(h, n_max, standoff != nullptr);
  BatchPtrs bp = make_ptrs(h, scene_id, qc, goals, n_goals, standoff, base_pos, Q0);
  h->last_launches = 0;
  h->last_ms = 0.0;
  if (h->dbg) HIPCHK(h, hipMemsetAsync(h->dbg.as<long long>() + 40, 0, 216 * sizeof(long long), st));

  SolveCall c;
  c.h = h, c.B = B, c.T = sp.T, c.kcap = sp.kcap, c.nF = h->rb.n_frames, c.max_iter = sp.max_iter;
  if ((rc = setup_lanes(h, st, sp, bp, c))) return rc;
  const int L = c.L;
  for (int l = 0; l < L; ++l)  // seeds, goal terms of the seeds, the lane's lists of round 0
    hipLaunchKernelGGL(lm_init_kernel(h->np), dim3(c.lanes[l].n), dim3(256), 0, st, h->d_rb, c.lanes[l].bp, c.lanes[l].sp, B, 0);
  if ((rc = run_init_pass(h, st, bp, sp, B))) return rc;
  if ((rc = test_waiting_seeds(h, st, c))) return rc;
  if (L > 1) {
    HIPCHK(h, hipEventRecord(h->lane_event[0], st));
    for (int l = 0; l < L; ++l) HIPCHK(h, hipStreamWaitEvent(c.lanes[l].st, h->lane_event[0], 0));
  }
  // naps of the throttle: tens of microseconds, which the default timer slack of a thread (50 us) would double
  const int old_slack = prctl(PR_GET_TIMERSLACK);
  if (old_slack > 1000) (void)prctl(PR_SET_TIMERSLACK, 1000UL);
  c.tp_start = std::chrono::steady_clock::now();
  int rc_loop = run_lanes(c);
  {
    double r_ = 0.0;
    for (int l = 0; l < L; ++l) r_ = std::max(r_, c.lanes[l].ratio_max);
    if (r_ > 0.0) h->items_per_job_prior = r_;
  }
  // the other lanes' work is behind the finalisation on the caller's stream
  for (int l = 0; l < L && L > 1 && !rc_loop; ++l)
    if (!c.lanes[l].handed) {
      if (hipEventRecord(h->lane_event[l], c.lanes[l].st) != hipSuccess || hipStreamWaitEvent(st, h->lane_event[l], 0) != hipSuccess) {
        h->err = "solve loop: joining the lanes failed";
        rc_loop = GTO_ERR_HIP;
      }
    }
  if (rc_loop)  // leave nothing of this call running on streams the caller does not know about
    for (int l = 0; l < L && L > 1; ++l) (void)hipStreamSynchronize(c.lanes[l].st);
  bp.live = c.lanes[0].bp.live, bp.cap = c.lanes[0].bp.cap;  // (what k_lm_finalize sees: lists are not read there)
  if (old_slack > 1000) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old_slack);
  if (rc_loop) return rc_loop;
  hipLaunchKernelGGL(k_lm_finalize, dim3(B), dim3(64), 0, st, h->d_rb, bp, sp, B, Q_out, dQ_out, cost_out, iters_out, status_out);
  HIPCHK(h, hipGetLastError());
  if (h->dbg && (rc = print_debug_stamps(h, st))) return rc;
  if (h->profiling && (rc = harvest_profile(h, st, bp.work))) return rc;
  return GTO_OK;
}

// k_ik_solve for a goal kind (GTO_IK_GOAL_* count from 0); the first reference to a variant decides where the code object
// places it, and the table keeps the order they have always had
using IkKernel = decltype(&k_ik_solve<GTO_IK_GOAL_POINTS>);
static IkKernel ik_kernel(int kind) {
  static const IkKernel k[3] = {k_ik_solve<GTO_IK_GOAL_POINTS>, k_ik_solve<GTO_IK_GOAL_QUATERNION>, k_ik_solve<GTO_IK_GOAL_RPY>};
  return k[kind];
}

// The launch of k_ik_solve<kind> over B instances whose arrays are on the device, on stream st: what the host-pointer and
// the device-pointer entry points share
static int ik_launch(gto_handle* h, int kind, int32_t B, const int32_t* d_sid, const double* d_q0, const double* d_goals,
                     const double* d_base, int32_t max_iter, double* d_q, double* d_cost, int32_t* d_it, int32_t* d_stat,
                     hipStream_t st) {
  SolveParams sp = make_params(h, 1, false);
  sp.max_iter = max_iter;
  const size_t lds = (size_t)ik_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt) * sizeof(double);
  if (lds > 150 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the IK kernel's LDS");
  const IkKernel kern = ik_kernel(kind);
  HIPCHK(h, raise_dynamic_lds((const void*)kern, lds));
  hipLaunchKernelGGL(kern, dim3(B), dim3(256), lds, st, h->d_rb, h->d_px, h->d_py, h->d_pz, h->d_chunks, h->d_scenes,
                     d_sid, d_q0, d_goals, d_base, sp, B, d_q, d_cost, d_it, d_stat, (int)h->scenes.size());
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

// the checks of every IK entry point that need no array's contents; GTO_OK with *empty set for B == 0
static int ik_check(gto_handle* h, const char* name, int32_t B, int32_t max_iter, bool null_input, bool* empty) {
  *empty = false;
  if (B < 0 || max_iter < 0) return fail(h, GTO_ERR_INVALID_ARG, "B and max_iter must be >= 0");
  if (B == 0) {
    *empty = true;
    return GTO_OK;
  }
  if (null_input) return fail(h, GTO_ERR_INVALID_ARG, "null input array");
  if (h->np != GTO_NB) return fail(h, GTO_ERR_UNSUPPORTED, std::string(name) + " handles up to eight optimised joints");
  return GTO_OK;
}

// gto_solve_ik_batch and gto_solve_ik_pose_batch: goals of one kind, gw doubles each; `name` speaks in the messages
static int ik_batch(gto_handle* h, const char* name, int kind, size_t gw, int32_t B, const int32_t* scene_id,
                    const double* q0, const double* goals, const double* base_pos, int32_t max_iter, double* q_out,
                    double* cost_out, int32_t* iters_out, int32_t* status_out) {
  bool empty;
  int rc = ik_check(h, name, B, max_iter, !q0 || !goals || !q_out, &empty);
  if (rc || empty) return rc;
  if (scene_id && (rc = check_scene_ids_host(h, scene_id, B))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof;
  std::vector<double> zeros;
  if (scene_id && !base_pos) {
    zeros.assign((size_t)B * 3, 0.0);
    base_pos = zeros.data();
  }
  Staging io(h);
  const int32_t* d_sid;
  const double *d_q0, *d_goals, *d_base;
  double *d_q, *d_cost;
  int32_t *d_it, *d_stat;
  if ((rc = io.in(scene_id, B, &d_sid))) return rc;
  if ((rc = io.in(q0, B * ndof, &d_q0))) return rc;
  if ((rc = io.in(goals, B * gw, &d_goals))) return rc;
  if ((rc = io.in(scene_id ? base_pos : nullptr, (size_t)B * 3, &d_base))) return rc;  // (no scene: no base)
  if ((rc = io.out(q_out, B * ndof, &d_q))) return rc;
  if ((rc = io.out(cost_out, B, &d_cost))) return rc;
  if ((rc = io.out(iters_out, B, &d_it))) return rc;
  if ((rc = io.out(status_out, B, &d_stat))) return rc;
  if ((rc = ik_launch(h, kind, B, d_sid, d_q0, d_goals, d_base, max_iter, d_q, d_cost, d_it, d_stat, h->stream))) return rc;
  return io.finish();
}

int gto_solve_ik_batch(gto_handle* h, int32_t B, const int32_t* scene_id, const double* q0, const double* goals,
                       const double* base_pos, int32_t max_iter, double* q_out, double* cost_out, int32_t* iters_out,
                       int32_t* status_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  return ik_batch(h, "gto_solve_ik_batch", GTO_IK_GOAL_POINTS, 16, B, scene_id, q0, goals, base_pos, max_iter, q_out,
                  cost_out, iters_out, status_out);
}

int gto_solve_ik_pose_batch(gto_handle* h, int32_t goal_kind, int32_t B, const int32_t* scene_id, const double* q0,
                            const double* goals, const double* base_pos, int32_t max_iter, double* q_out, double* cost_out,
                            int32_t* iters_out, int32_t* status_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (goal_kind != GTO_IK_GOAL_POINTS && goal_kind != GTO_IK_GOAL_QUATERNION && goal_kind != GTO_IK_GOAL_RPY)
    return fail(h, GTO_ERR_INVALID_ARG, "unknown IK goal kind");
  if (goal_kind == GTO_IK_GOAL_POINTS)  // the same call, launch and results
    return gto_solve_ik_batch(h, B, scene_id, q0, goals, base_pos, max_iter, q_out, cost_out, iters_out, status_out);
  return ik_batch(h, "gto_solve_ik_pose_batch", goal_kind, goal_kind == GTO_IK_GOAL_QUATERNION ? 7 : 6, B, scene_id, q0,
                  goals, base_pos, max_iter, q_out, cost_out, iters_out, status_out);
}

int gto_solve_ik_pose_batch_device(gto_handle* h, int32_t goal_kind, int32_t B, const int32_t* scene_id, const double* q0,
                                   const double* goals, const double* base_pos, int32_t max_iter, double* q_out,
                                   double* cost_out, int32_t* iters_out, int32_t* status_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (goal_kind != GTO_IK_GOAL_POINTS && goal_kind != GTO_IK_GOAL_QUATERNION && goal_kind != GTO_IK_GOAL_RPY)
    return fail(h, GTO_ERR_INVALID_ARG, "unknown IK goal kind");
  bool empty;
  const int rc = ik_check(h, "gto_solve_ik_pose_batch_device", B, max_iter, !q0 || !goals || !q_out, &empty);
  if (rc || empty) return rc;
  if (scene_id && !base_pos) return fail(h, GTO_ERR_INVALID_ARG, "gto_solve_ik_pose_batch_device: scene_id needs base_pos");
  HIPCHK(h, hipSetDevice(h->device));
  return ik_launch(h, goal_kind, B, scene_id, q0, goals, scene_id ? base_pos : nullptr, max_iter, q_out, cost_out, iters_out,
                   status_out, stream ? (hipStream_t)stream : h->stream);
}

int gto_ik_report_device(gto_handle* h, int32_t B, const int32_t* scene_id, const double* q, const double* goals,
                         const double* base_pos, double pos_tol, double rot_tol_deg, double cost_tol, double* err_pos_out,
                         double* err_rot_out, double* cost_out, uint8_t* accept_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0) return fail(h, GTO_ERR_INVALID_ARG, "gto_ik_report_device: B must be >= 0");
  if (B == 0) return GTO_OK;
  if (!q || !goals) return fail(h, GTO_ERR_INVALID_ARG, "gto_ik_report_device: null input array");
  if (scene_id && !base_pos) return fail(h, GTO_ERR_INVALID_ARG, "gto_ik_report_device: scene_id needs base_pos");
  if (h->np != GTO_NB) return fail(h, GTO_ERR_UNSUPPORTED, "gto_ik_report_device handles up to eight optimised joints");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t lds = sizeof(double) * plan_cost_lds_doubles_tg(1, h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  if (lds > 150 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the report kernel's LDS");
  HIPCHK(h, raise_dynamic_lds((const void*)k_ik_report, lds));
  hipLaunchKernelGGL(k_ik_report, dim3(B), dim3(256), lds, stream ? (hipStream_t)stream : h->stream, h->d_rb, h->d_px, h->d_py,
                     h->d_pz, h->d_plink, h->d_scenes, (int)h->scenes.size(), scene_id, q, goals, base_pos, pos_tol, rot_tol_deg,
                     cost_tol, err_pos_out, err_rot_out, cost_out, accept_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

// The closed joints of a retrieve path as the kernels take them: distinct indices in [0, ndof)
static int retrieve_closed(gto_handle* h, const char* who, const int32_t* closed_joints, const double* closed_values, int32_t n_closed,
                           RetrieveClosed* cl) {
  cl->mask = 0u;
  for (int d = 0; d < GTO_MAX_DOF; ++d) cl->value[d] = 0.0;
  if (n_closed < 0 || (n_closed > 0 && (!closed_joints || !closed_values)))
    return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": n_closed >= 0 with both closed arrays is required");
  for (int i = 0; i < n_closed; ++i) {
    const int d = closed_joints[i];
    if (d < 0 || d >= h->rb.ndof || ((cl->mask >> d) & 1u))
      return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": closed_joints must be distinct indices in [0, ndof)");
    cl->mask |= 1u << d;
    cl->value[d] = closed_values[i];
  }
  return GTO_OK;
}

// gto_retrieve_lift and its device variant behind the handle check: the host-side checks (*empty: B = 0) and the arguments
// that travel with the launch
static int retrieve_lift_args(gto_handle* h, const char* who, int32_t B, const double* plans, const double* direction, double distance,
                              int32_t K, const int32_t* closed_joints, const double* closed_values, int32_t n_closed, int32_t max_iter,
                              double pos_tol, double rot_tol_deg, const double* path_out, bool* empty, RetrieveClosed* cl,
                              RetrieveLine* ln) {
  int rc = ik_check(h, who, B, max_iter, false, empty);
  if (rc) return rc;
  if (K < 1 || K > GTO_RETRIEVE_MAX_STEPS) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": 1 <= K <= 64 is required");
  if (!direction || !std::isfinite(distance) || !std::isfinite(direction[0]) || !std::isfinite(direction[1]) || !std::isfinite(direction[2]))
    return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": a finite direction and distance are required");
  if (*empty) return GTO_OK;
  if (!plans || !path_out) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": null plans or path_out");
  if ((rc = retrieve_closed(h, who, closed_joints, closed_values, n_closed, cl))) return rc;
  for (int a = 0; a < 3; ++a) ln->dir[a] = direction[a];
  ln->step = distance / (double)K;
  ln->K = K, ln->pos_tol = pos_tol, ln->rot_tol_deg = rot_tol_deg;
  return GTO_OK;
}

static int retrieve_lift_launch(gto_handle* h, int32_t B, const double* plans, const int32_t* scene_id, const double* base_pos,
                                const RetrieveClosed& cl, const RetrieveLine& ln, int32_t max_iter, double* path_out, double* goals_out,
                                double* err_pos_out, double* err_rot_out, int32_t* iters_out, int32_t* status_out, int32_t* reached_out,
                                hipStream_t st) {
  SolveParams sp = make_params(h, 1, false);  // (what ik_launch hands k_ik_solve)
  sp.max_iter = max_iter;
  const size_t lds = (size_t)retrieve_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt) * sizeof(double);
  if (lds > 150 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the retrieve kernel's LDS");
  HIPCHK(h, raise_dynamic_lds((const void*)k_retrieve_lift, lds));
  hipLaunchKernelGGL(k_retrieve_lift, dim3(B), dim3(256), lds, st, h->d_rb, h->d_px, h->d_py, h->d_pz, h->d_chunks, h->d_scenes,
                     (int)h->scenes.size(), scene_id, plans, (int)h->opts.T, scene_id ? base_pos : nullptr, sp, cl, ln, path_out, goals_out,
                     err_pos_out, err_rot_out, iters_out, status_out, reached_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_retrieve_lift_device(gto_handle* h, int32_t B, const double* plans, const int32_t* scene_id, const double* base_pos,
                             const double* direction, double distance, int32_t K, const int32_t* closed_joints,
                             const double* closed_values, int32_t n_closed, int32_t max_iter, double pos_tol, double rot_tol_deg,
                             double* path_out, double* goals_out, double* err_pos_out, double* err_rot_out, int32_t* iters_out,
                             int32_t* status_out, int32_t* reached_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  bool empty;
  RetrieveClosed cl;
  RetrieveLine ln;
  const int rc = retrieve_lift_args(h, "gto_retrieve_lift_device", B, plans, direction, distance, K, closed_joints, closed_values, n_closed,
                                    max_iter, pos_tol, rot_tol_deg, path_out, &empty, &cl, &ln);
  if (rc || empty) return rc;
  if (scene_id && !base_pos) return fail(h, GTO_ERR_INVALID_ARG, "gto_retrieve_lift_device: scene_id needs base_pos");
  HIPCHK(h, hipSetDevice(h->device));
  return retrieve_lift_launch(h, B, plans, scene_id, base_pos, cl, ln, max_iter, path_out, goals_out, err_pos_out, err_rot_out, iters_out,
                              status_out, reached_out, stream ? (hipStream_t)stream : h->stream);
}

int gto_retrieve_lift(gto_handle* h, int32_t B, const double* plans, const int32_t* scene_id, const double* base_pos,
                      const double* direction, double distance, int32_t K, const int32_t* closed_joints, const double* closed_values,
                      int32_t n_closed, int32_t max_iter, double pos_tol, double rot_tol_deg, double* path_out, double* goals_out,
                      double* err_pos_out, double* err_rot_out, int32_t* iters_out, int32_t* status_out, int32_t* reached_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  bool empty;
  RetrieveClosed cl;
  RetrieveLine ln;
  int rc = retrieve_lift_args(h, "gto_retrieve_lift", B, plans, direction, distance, K, closed_joints, closed_values, n_closed, max_iter,
                              pos_tol, rot_tol_deg, path_out, &empty, &cl, &ln);
  if (rc || empty) return rc;
  if (scene_id && (rc = check_scene_ids_host(h, scene_id, B))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof, T = h->opts.T, k = (size_t)K;
  std::vector<double> zeros;
  if (scene_id && !base_pos) {
    zeros.assign((size_t)B * 3, 0.0);
    base_pos = zeros.data();
  }
  Staging io(h);
  const double *d_plans, *d_base;
  const int32_t* d_sid;
  double *d_path, *d_goals, *d_ep, *d_er;
  int32_t *d_it, *d_stat, *d_reached;
  if ((rc = io.in(plans, B * ndof * T, &d_plans))) return rc;
  if ((rc = io.in(scene_id, B, &d_sid))) return rc;
  if ((rc = io.in(scene_id ? base_pos : nullptr, (size_t)B * 3, &d_base))) return rc;
  if ((rc = io.out(path_out, B * ndof * (k + 1), &d_path))) return rc;
  if ((rc = io.out(goals_out, B * k * 16, &d_goals))) return rc;
  if ((rc = io.out(err_pos_out, B * k, &d_ep))) return rc;
  if ((rc = io.out(err_rot_out, B * k, &d_er))) return rc;
  if ((rc = io.out(iters_out, B * k, &d_it))) return rc;
  if ((rc = io.out(status_out, B * k, &d_stat))) return rc;
  if ((rc = io.out(reached_out, (size_t)B, &d_reached))) return rc;
  if ((rc = retrieve_lift_launch(h, B, d_plans, d_sid, d_base, cl, ln, max_iter, d_path, d_goals, d_ep, d_er, d_it, d_stat, d_reached,
                                 h->stream)))
    return rc;
  return io.finish();
}

int gto_retrieve_path_columns(gto_handle* h) {
  if (!h || h->opts.T + h->opts.standoff_offset - 10 < 0) return -1;
  return 9 - h->opts.standoff_offset;
}

int gto_retrieve_reverse_device(gto_handle* h, int32_t B, const double* plans, const int32_t* closed_joints, const double* closed_values,
                                int32_t n_closed, double* path_out, int32_t* n_cols_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0) return fail(h, GTO_ERR_INVALID_ARG, "gto_retrieve_reverse_device: B must be >= 0");
  const int n_cols = gto_retrieve_path_columns(h);
  if (n_cols < 1) return fail(h, GTO_ERR_INVALID_ARG, "gto_retrieve_reverse_device: the horizon is shorter than the stretch T + standoff_offset - 10 .. T - 2");
  if (n_cols_out) *n_cols_out = n_cols;
  if (B == 0) return GTO_OK;
  if (!plans || !path_out) return fail(h, GTO_ERR_INVALID_ARG, "gto_retrieve_reverse_device: null plans or path_out");
  RetrieveClosed cl;
  if (int rc = retrieve_closed(h, "gto_retrieve_reverse_device", closed_joints, closed_values, n_closed, &cl)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const long long total = (long long)B * h->rb.ndof * n_cols;
  hipLaunchKernelGGL(k_retrieve_reverse, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream ? (hipStream_t)stream : h->stream, plans,
                     (int)h->rb.ndof, (int)h->opts.T, n_cols, total, cl, path_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

// Both seed entry points behind their handle check: the checks, k_seed_score and the choice.  n_seeds = 0: the plain
// choice (k_seed_select); otherwise the ranked one into n_seeds slots per instance.
static int seed_goalsets(gto_handle* h, const std::string& name, int32_t B, int32_t n_max, int32_t n_seeds, const int32_t* scene_id,
                         const double* qc, const double* goals, const int32_t* n_goals, const double* q_solutions,
                         const uint8_t* accept, const double* base_pos, int32_t interpolate, int32_t solutions_f32,
                         double* goals_out, int32_t* n_goals_out, int32_t* n_accepted_out, int32_t* accepted_rows_out,
                         double* Q0_out, int32_t* seed_index_out, double* seed_cost_out, double* seed_dist_out, void* stream) {
  if (B < 0 || n_max < 1) return fail(h, GTO_ERR_INVALID_ARG, name + ": B must be >= 0 and n_max >= 1");
  if (B == 0) return GTO_OK;
  if (!scene_id || !qc || !goals || !n_goals || !q_solutions || !base_pos)
    return fail(h, GTO_ERR_INVALID_ARG, name + ": null input array");
  if (h->np != GTO_NB) return fail(h, GTO_ERR_UNSUPPORTED, name + " handles up to eight optimised joints");
  if (n_max > 65535 || B > 65535) return fail(h, GTO_ERR_UNSUPPORTED, name + ": at most 65535 instances of at most 65535 goals in one call");
  if (n_seeds && (long long)B * n_seeds > 65535) return fail(h, GTO_ERR_UNSUPPORTED, name + ": B * n_seeds must be at most 65535");
  if (h->scenes.empty()) return fail(h, GTO_ERR_NO_SCENE, "no scene has been set");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int T = h->opts.T;
  int rc;
  if ((rc = ensure(h, h->sd_part, (size_t)B * n_max * T * sizeof(double)))) return rc;
  const size_t lds = sizeof(double) * plan_cost_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  if (lds > 150 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the seed-score kernel's LDS");
  HIPCHK(h, raise_dynamic_lds((const void*)k_seed_score, lds));
  hipLaunchKernelGGL(k_seed_score, dim3((unsigned)((T + GTO_PLAN_TG - 1) / GTO_PLAN_TG), n_max, B), dim3(256), lds, st, h->d_rb,
                     h->d_px, h->d_py, h->d_pz, h->d_plink, h->d_scenes, (int)h->scenes.size(), scene_id, qc, n_goals,
                     q_solutions, accept, base_pos, T, n_max, solutions_f32 != 0, h->sd_part.as<double>());
  if (n_seeds)
    hipLaunchKernelGGL(k_seed_select_ranked, dim3(B), dim3(64), 0, st, h->d_rb, qc, goals, n_goals, q_solutions, accept,
                       h->sd_part.as<const double>(), T, T + h->opts.standoff_offset, n_max, interpolate != 0, solutions_f32 != 0,
                       (int)n_seeds, goals_out, n_goals_out, n_accepted_out, accepted_rows_out, Q0_out, seed_index_out,
                       seed_cost_out, seed_dist_out);
  else
    hipLaunchKernelGGL(k_seed_select, dim3(B), dim3(64), 0, st, h->d_rb, qc, goals, n_goals, q_solutions, accept,
                       h->sd_part.as<const double>(), T, T + h->opts.standoff_offset, n_max, interpolate != 0, solutions_f32 != 0,
                       goals_out, n_goals_out, n_accepted_out, Q0_out, seed_index_out, seed_cost_out, seed_dist_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_seed_goalsets_device(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id, const double* qc,
                             const double* goals, const int32_t* n_goals, const double* q_solutions, const uint8_t* accept,
                             const double* base_pos, int32_t interpolate, int32_t solutions_f32, double* goals_out,
                             int32_t* n_goals_out, int32_t* n_accepted_out, double* Q0_out, int32_t* seed_index_out,
                             double* seed_cost_out, double* seed_dist_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  return seed_goalsets(h, "gto_seed_goalsets_device", B, n_max, 0, scene_id, qc, goals, n_goals, q_solutions, accept, base_pos,
                       interpolate, solutions_f32, goals_out, n_goals_out, n_accepted_out, nullptr, Q0_out, seed_index_out,
                       seed_cost_out, seed_dist_out, stream);
}

int gto_seed_goalsets_multi_device(gto_handle* h, int32_t B, int32_t n_max, int32_t n_seeds, const int32_t* scene_id,
                                   const double* qc, const double* goals, const int32_t* n_goals, const double* q_solutions,
                                   const uint8_t* accept, const double* base_pos, int32_t interpolate, int32_t solutions_f32,
                                   double* goals_out, int32_t* n_goals_out, int32_t* n_accepted_out, int32_t* accepted_rows_out,
                                   double* Q0_out, int32_t* seed_index_out, double* seed_cost_out, double* seed_dist_out,
                                   void* stream) {
  // a plain number, looked at before anything else: no handle is needed to refuse it
  if (n_seeds < 1 || n_seeds > GTO_MAX_SEEDS) return fail(h, GTO_ERR_UNSUPPORTED, "gto_seed_goalsets_multi_device: n_seeds must be in [1, 16]");
  if (!h) return GTO_ERR_INVALID_ARG;
  return seed_goalsets(h, "gto_seed_goalsets_multi_device", B, n_max, n_seeds, scene_id, qc, goals, n_goals, q_solutions, accept,
                       base_pos, interpolate, solutions_f32, goals_out, n_goals_out, n_accepted_out, accepted_rows_out, Q0_out,
                       seed_index_out, seed_cost_out, seed_dist_out, stream);
}

int gto_plan_report_device(gto_handle* h, int32_t B, int32_t n_max, const double* goals, const int32_t* n_goals,
                           const double* standoff, const double* Q, int32_t* goal_index_out, double* goal_cost_out,
                           double* err_pos_out, double* err_rot_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || n_max < 1) return fail(h, GTO_ERR_INVALID_ARG, "gto_plan_report_device: B must be >= 0 and n_max >= 1");
  if (h->np != GTO_NB) return fail(h, GTO_ERR_UNSUPPORTED, "gto_plan_report_device handles up to eight optimised joints");
  if (B == 0) return GTO_OK;
  if (!goals || !n_goals || !Q) return fail(h, GTO_ERR_INVALID_ARG, "gto_plan_report_device: null input array");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t lds = sizeof(double) * plan_cost_lds_doubles_tg(1, h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  if (lds > 150 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the report kernel's LDS");
  HIPCHK(h, raise_dynamic_lds((const void*)k_plan_report, lds));
  const int T = h->opts.T;
  hipLaunchKernelGGL(k_plan_report, dim3(B), dim3(256), lds, stream ? (hipStream_t)stream : h->stream, h->d_rb, goals, n_goals,
                     standoff, Q, T, T + h->opts.standoff_offset, (int)n_max, goal_index_out, goal_cost_out, err_pos_out, err_rot_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_select_plans_device(gto_handle* h, int32_t B, int32_t n_seeds, const int32_t* status, const double* cost,
                            const double* err_pos, const double* err_rot, const int32_t* counts, double pos_tol,
                            double rot_tol_deg, int32_t max_points, const double* Q, const double* dQ, int32_t* best_slot_out,
                            int32_t* class_out, double* Q_out, double* dQ_out, void* stream) {
  if (n_seeds < 1 || n_seeds > GTO_MAX_SEEDS) return fail(h, GTO_ERR_UNSUPPORTED, "gto_select_plans_device: n_seeds must be in [1, 16]");
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0) return fail(h, GTO_ERR_INVALID_ARG, "gto_select_plans_device: B must be >= 0");
  if (h->np != GTO_NB) return fail(h, GTO_ERR_UNSUPPORTED, "gto_select_plans_device handles up to eight optimised joints");
  if (B == 0) return GTO_OK;
  if (!status || !cost || !err_pos || !err_rot || (Q_out && !Q) || (dQ_out && !dQ))
    return fail(h, GTO_ERR_INVALID_ARG, "gto_select_plans_device: null input array");
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_select_plans, dim3(B), dim3(256), 0, stream ? (hipStream_t)stream : h->stream, (int)n_seeds, h->opts.T,
                     h->rb.ndof, status, cost, err_pos, err_rot, counts, pos_tol, rot_tol_deg, (int)max_points, Q, dQ,
                     best_slot_out, class_out, Q_out, dQ_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

// What every base-placement entry point checks once its own B check is done; `null_input`: one of the arrays the entry
// point needs is null.  GTO_OK with *empty set for B == 0.
static int base_check(gto_handle* h, const char* name, int32_t B, int32_t n_max, const int32_t* n_goals, bool null_input, bool* empty) {
  *empty = false;
  if (n_max < 1 || n_max > GTO_MAX_BASE_GOALS) return fail(h, GTO_ERR_UNSUPPORTED, "n_max must be in [1, 32]");
  if (h->np != GTO_NB) return fail(h, GTO_ERR_UNSUPPORTED, std::string(name) + " handles up to eight optimised joints");
  if (B == 0) {
    *empty = true;
    return GTO_OK;
  }
  if (null_input) return fail(h, GTO_ERR_INVALID_ARG, "null input array");
  for (int b = 0; b < B; ++b)
    if (n_goals[b] < 1 || n_goals[b] > n_max) return fail(h, GTO_ERR_INVALID_ARG, "n_goals[b] must be in [1, n_max]");
  return GTO_OK;
}

// The launch of k_base_solve over B goal sets whose arrays are on the device, on stream st: what the host-pointer and the
// device-pointer entry points share
static int base_launch(gto_handle* h, int32_t B, int32_t n_max, const double* d_qc, const double* d_goals, const int32_t* d_ng,
                       double effort_weight, int32_t max_iter, const double* d_y0, const double* d_q0, double* d_y, double* d_q,
                       double* d_cost, int32_t* d_it, int32_t* d_stat, hipStream_t st) {
  SolveParams sp = make_params(h, 1, false);
  sp.max_iter = max_iter;
  const size_t lds = (size_t)base_lds_doubles(n_max) * sizeof(double);
  if (lds > 160 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "goal set too large for the base kernel's LDS");
  HIPCHK(h, raise_dynamic_lds((const void*)k_base_solve, lds));
  hipLaunchKernelGGL(k_base_solve, dim3(B), dim3(256), lds, st, h->d_rb, d_qc, d_goals, d_ng, sp, effort_weight, n_max,
                     d_y, d_q, d_cost, d_it, d_stat, d_y0, d_q0);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

// `bytes` bytes of a host array of the caller on the device in `dst` (grown on demand), ordered on `st` in front of the kernel
// that reads them.  The array is copied into a pinned slot of the handle first, so the caller's array is free on return
// whatever memory it lives in, and the transfer is a real asynchronous DMA.  A slot is reused once the copy that read it has
// run (its event; with GTO_BASE_PIN_SLOTS calls in flight the host waits for the oldest).  dst is one device buffer per
// handle: calls on one handle go to one stream, or the caller orders them.
static int pinned_to_device(gto_handle* h, DevBuf& dst, const void* src, size_t bytes, hipStream_t st) {
  int rc = ensure(h, dst, bytes);
  if (rc) return rc;
  const int k = h->bs_pin_next;
  h->bs_pin_next = (k + 1) % GTO_BASE_PIN_SLOTS;
  if (!h->bs_pin_ev[k]) HIPCHK(h, hipEventCreateWithFlags(&h->bs_pin_ev[k], hipEventDisableTiming));
  else HIPCHK(h, hipEventSynchronize(h->bs_pin_ev[k]));
  if ((rc = ensure(h, h->bs_pin[k], bytes))) return rc;
  memcpy(h->bs_pin[k].get(), src, bytes);
  HIPCHK(h, hipMemcpyAsync(dst.get(), h->bs_pin[k].get(), bytes, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipEventRecord(h->bs_pin_ev[k], st));
  return GTO_OK;
}

// The caller's n_goals [B] (host, checked) on the device in bs_ng: pinned_to_device
static int base_counts_to_device(gto_handle* h, int32_t B, const int32_t* n_goals, hipStream_t st, const int32_t** d_ng) {
  if (int rc = pinned_to_device(h, h->bs_ng, n_goals, (size_t)B * sizeof(int32_t), st)) return rc;
  *d_ng = h->bs_ng.as<const int32_t>();
  return GTO_OK;
}

// gto_solve_base_batch and gto_eval_base_objective after their own B check.  A solve starts from qc.  An evaluation passes
// the point (y0, q0) with max_iter 0 and no y_out / q_out: qc is the first goal's configuration of every set in q0, and the
// point k_base_solve writes back stays on the device.
static int base_batch(gto_handle* h, const char* name, int32_t B, int32_t n_max, const int32_t* n_goals, bool null_input,
                      const double* qc, const double* goals, double effort_weight, int32_t max_iter, const double* y0,
                      const double* q0, double* y_out, double* q_out, double* cost_out, int32_t* iters_out,
                      int32_t* status_out) {
  bool empty;
  int rc = base_check(h, name, B, n_max, n_goals, null_input, &empty);
  if (rc || empty) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof, nB = B;
  std::vector<double> qc_eval;
  if (q0) {
    qc_eval.resize(nB * ndof);
    for (size_t b = 0; b < nB; ++b) std::copy(q0 + b * n_max * ndof, q0 + b * n_max * ndof + ndof, qc_eval.begin() + b * ndof);
    qc = qc_eval.data();
  }
  Staging io(h);
  const double *d_qc, *d_goals, *d_y0, *d_q0;
  const int32_t* d_ng;
  double *d_q, *d_y, *d_cost;
  int32_t *d_it, *d_stat;
  if ((rc = io.in(qc, nB * ndof, &d_qc))) return rc;
  if ((rc = io.in(goals, nB * n_max * 16, &d_goals))) return rc;
  if ((rc = io.in(n_goals, nB, &d_ng))) return rc;
  if ((rc = io.in(y0, nB * 3, &d_y0))) return rc;
  if ((rc = io.in(q0, nB * n_max * ndof, &d_q0))) return rc;
  if ((rc = q_out ? io.out(q_out, nB * n_max * ndof, &d_q) : io.scratch(nB * n_max * ndof, &d_q))) return rc;
  if ((rc = y_out ? io.out(y_out, nB * 3, &d_y) : io.scratch(nB * 3, &d_y))) return rc;
  if ((rc = io.out(cost_out, nB, &d_cost))) return rc;
  if ((rc = io.out(iters_out, nB, &d_it))) return rc;
  if ((rc = io.out(status_out, nB, &d_stat))) return rc;
  if ((rc = base_launch(h, B, n_max, d_qc, d_goals, d_ng, effort_weight, max_iter, d_y0, d_q0, d_y, d_q, d_cost, d_it, d_stat, h->stream)))
    return rc;
  return io.finish();
}

int gto_solve_base_batch(gto_handle* h, int32_t B, int32_t n_max, const int32_t* n_goals, const double* qc,
                         const double* goals, double effort_weight, int32_t max_iter, double* y_out, double* q_out,
                         double* cost_out, int32_t* iters_out, int32_t* status_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || max_iter < 0) return fail(h, GTO_ERR_INVALID_ARG, "B and max_iter must be >= 0");
  return base_batch(h, "gto_solve_base_batch", B, n_max, n_goals, !n_goals || !qc || !goals || !y_out || !q_out, qc, goals,
                    effort_weight, max_iter, nullptr, nullptr, y_out, q_out, cost_out, iters_out, status_out);
}

int gto_solve_base_batch_device(gto_handle* h, int32_t B, int32_t n_max, const int32_t* n_goals, const double* qc,
                                const double* goals, double effort_weight, int32_t max_iter, double* y_out, double* q_out,
                                double* cost_out, int32_t* iters_out, int32_t* status_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || max_iter < 0) return fail(h, GTO_ERR_INVALID_ARG, "B and max_iter must be >= 0");
  bool empty;
  int rc = base_check(h, "gto_solve_base_batch_device", B, n_max, n_goals, !n_goals || !qc || !goals || !y_out || !q_out, &empty);
  if (rc || empty) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int32_t* d_ng;
  if ((rc = base_counts_to_device(h, B, n_goals, st, &d_ng))) return rc;
  return base_launch(h, B, n_max, qc, goals, d_ng, effort_weight, max_iter, nullptr, nullptr, y_out, q_out, cost_out, iters_out,
                     status_out, st);
}

#ifdef GTO_DEBUG_BASE_TIMING
// (debug builds only: tools/base_stamps.py) phase stamps of k_base_solve since the last call, then cleared
int gto_debug_base_stamps(long long* out16) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_base_dbg), 16 * sizeof(long long)) != hipSuccess) return GTO_ERR_HIP;
  long long z[16] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_base_dbg), z, sizeof z) == hipSuccess ? GTO_OK : GTO_ERR_HIP;
}
#endif

int gto_eval_base_objective(gto_handle* h, int32_t B, int32_t n_max, const int32_t* n_goals, const double* y,
                            const double* q, const double* goals, double effort_weight, double* cost_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0) return fail(h, GTO_ERR_INVALID_ARG, "B must be >= 0");
  return base_batch(h, "gto_eval_base_objective", B, n_max, n_goals, !n_goals || !y || !q || !goals || !cost_out, nullptr,
                    goals, effort_weight, 0, y, q, nullptr, nullptr, cost_out, nullptr, nullptr);
}

int gto_solve_batch(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id, const double* qc, const double* goals,
                    const int32_t* n_goals, const double* standoff, const double* base_pos, const double* Q0,
                    double* Q_out, double* dQ_out, double* cost_out, int32_t* iters_out, int32_t* status_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || n_max < 1) return fail(h, GTO_ERR_INVALID_ARG, "B must be >= 0 and n_max >= 1");
  if (B == 0) return GTO_OK;
  if (!scene_id || !qc || !goals || !n_goals || !base_pos || !Q0) return fail(h, GTO_ERR_INVALID_ARG, "null input array");
  int rc = check_scene_ids_host(h, scene_id, B);
  if (rc) return rc;
  for (int b = 0; b < B; ++b)
    if (n_goals[b] < 1 || n_goals[b] > n_max) return fail(h, GTO_ERR_INVALID_ARG, "n_goals[b] must be in [1, n_max]");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof, T = h->opts.T;
  Staging io(h);
  const int32_t *d_sid, *d_ng;
  const double *d_qc, *d_goals, *d_so, *d_base, *d_Q0;
  double *d_Q, *d_dQ, *d_cost;
  int32_t *d_it, *d_stat;
  if ((rc = io.in(scene_id, B, &d_sid))) return rc;
  if ((rc = io.in(qc, B * ndof, &d_qc))) return rc;
  if ((rc = io.in(goals, (size_t)B * n_max * 16, &d_goals))) return rc;
  if ((rc = io.in(n_goals, B, &d_ng))) return rc;
  if ((rc = io.in(standoff, (size_t)B * 16, &d_so))) return rc;
  if ((rc = io.in(base_pos, (size_t)B * 3, &d_base))) return rc;
  if ((rc = io.in(Q0, B * ndof * T, &d_Q0))) return rc;
  if ((rc = io.out(Q_out, B * ndof * T, &d_Q))) return rc;
  if ((rc = io.out(dQ_out, B * ndof * (T - 1), &d_dQ))) return rc;
  if ((rc = io.out(cost_out, B, &d_cost))) return rc;
  if ((rc = io.out(iters_out, B, &d_it))) return rc;
  if ((rc = io.out(status_out, B, &d_stat))) return rc;
  rc = gto_solve_batch_device(h, B, n_max, d_sid, d_qc, d_goals, d_ng, d_so, d_base, d_Q0, d_Q, d_dQ, d_cost, d_it, d_stat,
                              nullptr);
  if (rc) return rc;
  return io.finish();
}

// -------------------------------------------------------------------------------------------------
// k_eval_kin over nq configurations on the device: the frames (frames_out) or the links' visual transforms (vis_out)
static int launch_eval_kin(gto_handle* h, int nq, const double* dq, double* frames_out, double* vis_out) {
  const size_t lds = sizeof(double) * eval_kin_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  HIPCHK(h, raise_dynamic_lds((const void*)k_eval_kin, lds));
  hipLaunchKernelGGL(k_eval_kin, dim3((nq + GTO_EVAL_TG - 1) / GTO_EVAL_TG), dim3(256), lds, h->stream, h->d_rb, nq, dq,
                     frames_out, vis_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_eval_fk(gto_handle* h, int32_t nq, const double* q, double* frames_out) {
  if (!h || !q || !frames_out || nq < 0) return h ? fail(h, GTO_ERR_INVALID_ARG, "bad argument") : GTO_ERR_INVALID_ARG;
  if (nq == 0) return GTO_OK;
  HIPCHK(h, hipSetDevice(h->device));
  Staging io(h);
  const double* dq;
  double* dout;
  int rc;
  if ((rc = io.in(q, (size_t)nq * h->rb.ndof, &dq))) return rc;
  if ((rc = io.out(frames_out, (size_t)nq * h->rb.n_frames * 16, &dout))) return rc;
  if ((rc = launch_eval_kin(h, nq, dq, dout, nullptr))) return rc;
  return io.finish();
}

// -------------------------------------------------------------------------------------------------
// inverse dynamics (gto_dynamics.h)
int gto_set_link_inertials(gto_handle* h, const double* mass, const double* com, const double* inertia, const double gravity[3]) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!mass || !com || !inertia) return fail(h, GTO_ERR_INVALID_ARG, "null input array");
  std::string why;
  if (int rc = gto_robot::check_inertials(h->rb.n_frames, mass, com, inertia, gravity, why)) return fail(h, rc, why);
  DynDev dyn;
  gto_robot::fill_inertials(h->rb.n_frames, mass, com, inertia, gravity, dyn);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // launches that read the table it replaces
  if (!h->dyn_buf.get()) HIPCHK(h, dev_alloc(h->dyn_buf, sizeof dyn));
  HIPCHK(h, hipMemcpy(h->dyn_buf.get(), &dyn, sizeof dyn, hipMemcpyHostToDevice));
  h->has_inertials = true;
  return GTO_OK;
}

int gto_inverse_dynamics(gto_handle* h, int32_t n, const double* q, const double* qd, const double* qdd, const double* payload_mass,
                         const double* payload_com, const double* payload_inertia, double* tau_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (n < 0) return fail(h, GTO_ERR_INVALID_ARG, "n must be >= 0");
  if (!h->has_inertials) return fail(h, GTO_ERR_INVALID_ARG, "no link inertials set");
  if (n == 0) return GTO_OK;
  if (!q || !qd || !qdd || !tau_out) return fail(h, GTO_ERR_INVALID_ARG, "null input array");
  if (!payload_mass && (payload_com || payload_inertia)) return fail(h, GTO_ERR_INVALID_ARG, "payload_com / payload_inertia without payload_mass");
  if (payload_mass)
    for (int i = 0; i < n; ++i)
      if (!(payload_mass[i] >= 0) || !std::isfinite(payload_mass[i])) return fail(h, GTO_ERR_INVALID_ARG, "payload mass must be >= 0 and finite");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof;
  Staging io(h);
  const double *dq, *dqd, *dqdd, *dpm, *dpc, *dpi;
  double* dtau;
  int rc;
  if ((rc = io.in(q, (size_t)n * ndof, &dq))) return rc;
  if ((rc = io.in(qd, (size_t)n * ndof, &dqd))) return rc;
  if ((rc = io.in(qdd, (size_t)n * ndof, &dqdd))) return rc;
  if ((rc = io.in(payload_mass, (size_t)n, &dpm))) return rc;  // (a null array: a null device pointer)
  if ((rc = io.in(payload_com, (size_t)n * 3, &dpc))) return rc;
  if ((rc = io.in(payload_inertia, (size_t)n * 6, &dpi))) return rc;
  if ((rc = io.out(tau_out, (size_t)n * ndof, &dtau))) return rc;
  const int rows = rnea_rows_per_block(h->rb.n_frames);
  const size_t lds = sizeof(double) * GTO_RNEA_SLOTS * h->rb.n_frames * rows;
  hipLaunchKernelGGL(k_inverse_dynamics, dim3((unsigned)((n + rows - 1) / rows)), dim3(GTO_WAVE), lds, h->stream, h->d_rb,
                     h->dyn_buf.as<const DynDev>(), n, rows, dq, dqd, dqdd, dpm, dpc, dpi, dtau);
  HIPCHK(h, hipGetLastError());
  return io.finish();
}

}  // extern "C"

// -------------------------------------------------------------------------------------------------
// forward dynamics and the tracking rollout (gto_forward.h)
// The joint lists of a call.  A joint is free when some actuated frame names it and `locked` (HOST [ndof], NULL = every
// joint that is not optimised) does not mark it.  columns_of_named: the mass-matrix columns of every named joint
// (gto_forward_dynamics' M_out) or of the free ones only.
static FdSets fd_sets(const gto_handle* h, const int32_t* locked, bool columns_of_named) {
  FdSets s = {};
  const RobotDev& rb = h->rb;
  s.ndof = rb.ndof;
  bool named[GTO_MAX_DOF] = {};
  for (int f = 0; f < rb.n_frames; ++f)
    if (rb.joint_type[f] != GTO_JOINT_FIXED && rb.q_index[f] >= 0) named[rb.q_index[f]] = true;
  for (int j = 0; j < rb.ndof; ++j) {
    const bool lk = locked ? locked[j] != 0 : rb.opt_of_dof[j] < 0;
    const bool fr = named[j] && !lk;
    s.is_free[j] = fr ? 1 : 0;
    if (fr) s.fr[s.nf++] = j;
    if (columns_of_named ? named[j] : fr) s.col[s.nc++] = j;
  }
  return s;
}

// which payload arrays come together, and the masses where the host sees them (n > 0)
static int payload_check(gto_handle* h, const std::string& f, int32_t n, const double* mass, const double* com, const double* inertia) {
  if (!mass && (com || inertia)) return fail(h, GTO_ERR_INVALID_ARG, f + "payload_com / payload_inertia without payload_mass");
  if (mass)
    for (int32_t i = 0; i < n; ++i)
      if (!(mass[i] >= 0) || !std::isfinite(mass[i])) return fail(h, GTO_ERR_INVALID_ARG, f + "payload mass must be >= 0 and finite");
  return GTO_OK;
}

extern "C" int gto_forward_dynamics(gto_handle* h, int32_t n, const double* q, const double* qd, const double* tau,
                                    const double* payload_mass, const double* payload_com, const double* payload_inertia,
                                    const int32_t* locked, double* qdd_out, double* M_out, int32_t* status_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (n < 0) return fail(h, GTO_ERR_INVALID_ARG, "n must be >= 0");
  if (!h->has_inertials) return fail(h, GTO_ERR_INVALID_ARG, "no link inertials set");
  if (n == 0) return GTO_OK;
  if (!q || !qd || !tau || !qdd_out) return fail(h, GTO_ERR_INVALID_ARG, "null input array");
  int rc;
  if ((rc = payload_check(h, "", n, payload_mass, payload_com, payload_inertia))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof;
  const FdSets sets = fd_sets(h, locked, true);
  Staging io(h);
  const double *dq, *dqd, *dtau, *dpm, *dpc, *dpi;
  double *dqdd, *dM;
  int32_t* dst;
  if ((rc = io.in(q, (size_t)n * ndof, &dq))) return rc;
  if ((rc = io.in(qd, (size_t)n * ndof, &dqd))) return rc;
  if ((rc = io.in(tau, (size_t)n * ndof, &dtau))) return rc;
  if ((rc = io.in(payload_mass, (size_t)n, &dpm))) return rc;  // (a null array: a null device pointer)
  if ((rc = io.in(payload_com, (size_t)n * 3, &dpc))) return rc;
  if ((rc = io.in(payload_inertia, (size_t)n * 6, &dpi))) return rc;
  if ((rc = io.out(qdd_out, (size_t)n * ndof, &dqdd))) return rc;
  if ((rc = io.out(M_out, (size_t)n * ndof * ndof, &dM))) return rc;
  if ((rc = io.out(status_out, (size_t)n, &dst))) return rc;
  const int F = h->rb.n_frames, rows = fd_rows_per_block(F, (int)ndof);
  const size_t lds = sizeof(double) * (GTO_RNEA_SLOTS * F + fd_work_doubles((int)ndof, GTO_FD_VECS)) * rows +
                     sizeof(int) * (3 * GTO_MAX_DOF + rows);
  hipLaunchKernelGGL(k_forward_dynamics, dim3((unsigned)((n + rows - 1) / rows)), dim3(GTO_WAVE), lds, h->stream, h->d_rb,
                     h->dyn_buf.as<const DynDev>(), sets, n, rows, dq, dqd, dtau, dpm, dpc, dpi, dqdd, dM, dst);
  HIPCHK(h, hipGetLastError());
  return io.finish();
}

// the host arrays and scalars of a rollout call, checked into the kernel's arguments
static int track_check(gto_handle* h, int32_t B, int32_t M, const double* kp, const double* kd, const double* tau_max, double dt,
                       double settle, int32_t feedforward, int32_t Mo, const double* const pay[6], TrackParams& prm) {
  const std::string f = "gto_track_rollout: ";
  if (B < 0) return fail(h, GTO_ERR_INVALID_ARG, f + "B must be >= 0");
  if (M < 2 || Mo < 2) return fail(h, GTO_ERR_INVALID_ARG, f + "M and Mo must be >= 2");
  if (!h->has_inertials) return fail(h, GTO_ERR_INVALID_ARG, "no link inertials set");
  if (!kp || !kd || !tau_max) return fail(h, GTO_ERR_INVALID_ARG, f + "null gain or limit array");
  for (int j = 0; j < h->rb.ndof; ++j) {
    if (!(kp[j] >= 0.0) || !std::isfinite(kp[j]) || !(kd[j] >= 0.0) || !std::isfinite(kd[j]))
      return fail(h, GTO_ERR_INVALID_ARG, f + "kp and kd must be finite and >= 0");
    if (!(tau_max[j] > 0.0)) return fail(h, GTO_ERR_INVALID_ARG, f + "tau_max must be > 0 (+inf: no limit)");
    prm.kp[j] = kp[j], prm.kd[j] = kd[j], prm.tau_max[j] = tau_max[j];
  }
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail(h, GTO_ERR_INVALID_ARG, f + "dt must be finite and > 0");
  if (!(settle >= 0.0) || !std::isfinite(settle)) return fail(h, GTO_ERR_INVALID_ARG, f + "settle must be finite and >= 0");
  if (feedforward < 0 || feedforward > 2) return fail(h, GTO_ERR_INVALID_ARG, f + "feedforward must be 0, 1 or 2");
  for (int k = 0; k < 2; ++k)
    if (!pay[3 * k] && (pay[3 * k + 1] || pay[3 * k + 2]))
      return fail(h, GTO_ERR_INVALID_ARG, f + "payload_com / payload_inertia without payload_mass");
  if ((long long)B * std::max(M, Mo) * std::max(h->rb.ndof, 1) > (long long)INT32_MAX * 64)
    return fail(h, GTO_ERR_UNSUPPORTED, f + "batch too large for one call");
  prm.dt = dt, prm.settle = settle, prm.B = B, prm.M = M, prm.Mo = Mo, prm.feedforward = feedforward;
  prm.G = track_group_lanes(h->rb.n_frames, h->rb.ndof);
  prm.P = track_paths_per_block(h->rb.n_frames, h->rb.ndof, prm.G);
  return GTO_OK;
}

// the one launch of a checked call, on `st`
static int track_launch(gto_handle* h, const TrackParams& prm, const FdSets& sets, const TrackRef& ref, const TrackPayloads& pay,
                        const TrackOut& out, hipStream_t st) {
  const int F = h->rb.n_frames, ndof = h->rb.ndof;
  const size_t lds = sizeof(double) * ((size_t)GTO_RNEA_SLOTS * F * prm.P * prm.G + (size_t)fd_work_doubles(ndof, GTO_TR_VECS) * prm.P + 3 * ndof) +
                     sizeof(int) * (3 * GTO_MAX_DOF + 4 * prm.P + 1);
  hipLaunchKernelGGL(k_track_rollout, dim3((unsigned)((prm.B + prm.P - 1) / prm.P)), dim3(GTO_WAVE), lds, st, h->d_rb,
                     h->dyn_buf.as<const DynDev>(), prm, sets, ref, pay, out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

extern "C" int gto_track_rollout_device(gto_handle* h, int32_t B, int32_t M, const double* duration, const double* q_ref,
                                        const double* qd_ref, const double* qdd_ref, const double* kp, const double* kd,
                                        const double* tau_max, double dt, double settle, int32_t feedforward,
                                        const double* model_payload_mass, const double* model_payload_com,
                                        const double* model_payload_inertia, const double* plant_payload_mass,
                                        const double* plant_payload_com, const double* plant_payload_inertia,
                                        const int32_t* locked, int32_t Mo, double* q_out, double* qd_out, double* t_out,
                                        double* err_max, double* err_end, int32_t* sat_steps, int32_t* steps, int32_t* status_out,
                                        void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  const double* const pay[6] = {model_payload_mass, model_payload_com, model_payload_inertia,
                                plant_payload_mass, plant_payload_com, plant_payload_inertia};
  TrackParams prm = {};
  if (int rc = track_check(h, B, M, kp, kd, tau_max, dt, settle, feedforward, Mo, pay, prm)) return rc;
  if (B == 0) return GTO_OK;
  if (!duration || !q_ref || !qd_ref || !qdd_ref) return fail(h, GTO_ERR_INVALID_ARG, "gto_track_rollout: null reference array");
  HIPCHK(h, hipSetDevice(h->device));
  return track_launch(h, prm, fd_sets(h, locked, false), {duration, q_ref, qd_ref, qdd_ref},
                      {pay[0], pay[1], pay[2], pay[3], pay[4], pay[5]},
                      {q_out, qd_out, t_out, err_max, err_end, sat_steps, steps, status_out}, stream ? (hipStream_t)stream : h->stream);
}

extern "C" int gto_track_rollout(gto_handle* h, int32_t B, int32_t M, const double* duration, const double* q_ref, const double* qd_ref,
                                 const double* qdd_ref, const double* kp, const double* kd, const double* tau_max, double dt,
                                 double settle, int32_t feedforward, const double* model_payload_mass,
                                 const double* model_payload_com, const double* model_payload_inertia,
                                 const double* plant_payload_mass, const double* plant_payload_com,
                                 const double* plant_payload_inertia, const int32_t* locked, int32_t Mo, double* q_out,
                                 double* qd_out, double* t_out, double* err_max, double* err_end, int32_t* sat_steps,
                                 int32_t* steps, int32_t* status_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  const double* const pay[6] = {model_payload_mass, model_payload_com, model_payload_inertia,
                                plant_payload_mass, plant_payload_com, plant_payload_inertia};
  TrackParams prm = {};
  int rc;
  if ((rc = track_check(h, B, M, kp, kd, tau_max, dt, settle, feedforward, Mo, pay, prm))) return rc;
  for (int k = 0; k < 2; ++k)
    if ((rc = payload_check(h, "gto_track_rollout: ", B, pay[3 * k], pay[3 * k + 1], pay[3 * k + 2]))) return rc;
  if (B == 0) return GTO_OK;
  if (!duration || !q_ref || !qd_ref || !qdd_ref) return fail(h, GTO_ERR_INVALID_ARG, "gto_track_rollout: null reference array");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B, nd = h->rb.ndof, nM = (size_t)M, nO = (size_t)Mo;
  Staging io(h);
  TrackRef ref = {};
  const double* dp[6];
  TrackOut out = {};
  if ((rc = io.in(duration, nB, &ref.duration))) return rc;
  if ((rc = io.in(q_ref, nB * nM * nd, &ref.q))) return rc;
  if ((rc = io.in(qd_ref, nB * nM * nd, &ref.qd))) return rc;
  if ((rc = io.in(qdd_ref, nB * nM * nd, &ref.qdd))) return rc;
  for (int k = 0; k < 6; ++k)  // (a null array: a null device pointer)
    if ((rc = io.in(pay[k], nB * (k % 3 == 0 ? 1 : k % 3 == 1 ? 3 : 6), &dp[k]))) return rc;
  if ((rc = io.out(q_out, nB * nO * nd, &out.q))) return rc;
  if ((rc = io.out(qd_out, nB * nO * nd, &out.qd))) return rc;
  if ((rc = io.out(t_out, nB * nO, &out.t))) return rc;
  if ((rc = io.out(err_max, nB, &out.err_max))) return rc;
  if ((rc = io.out(err_end, nB, &out.err_end))) return rc;
  if ((rc = io.out(sat_steps, nB, &out.sat_steps))) return rc;
  if ((rc = io.out(steps, nB, &out.steps))) return rc;
  if ((rc = io.out(status_out, nB, &out.status))) return rc;
  if ((rc = track_launch(h, prm, fd_sets(h, locked, false), ref, {dp[0], dp[1], dp[2], dp[3], dp[4], dp[5]}, out, h->stream))) return rc;
  return io.finish();
}

extern "C" {

int gto_eval_points(gto_handle* h, int32_t scene_id, int32_t nq, const double* q, const double* base_pos, int32_t use_obs,
                    double* xyz_out, int32_t* offset_out, double* value_out, double* grad_out) {
  if (!h || !q || !base_pos || nq < 0) return h ? fail(h, GTO_ERR_INVALID_ARG, "bad argument") : GTO_ERR_INVALID_ARG;
  if (nq == 0) return GTO_OK;
  const bool want_field = offset_out || value_out || grad_out;
  if (want_field && !scene_valid(h, scene_id)) return fail(h, GTO_ERR_NO_SCENE, "unknown scene");
  HIPCHK(h, hipSetDevice(h->device));
  const int P = h->rb.n_points, L = h->rb.n_links;
  Staging io(h);
  const double *dq, *dbase;
  double *dx, *dval, *dgrad;
  int32_t* doff;
  int rc;
  if ((rc = io.in(q, (size_t)nq * h->rb.ndof, &dq))) return rc;
  if ((rc = io.in(base_pos, (size_t)nq * 3, &dbase))) return rc;
  if ((rc = ensure(h, h->vis, (size_t)nq * L * 12 * sizeof(double)))) return rc;
  if ((rc = io.out(xyz_out, (size_t)nq * P * 3, &dx))) return rc;
  if ((rc = io.out(offset_out, (size_t)nq * P, &doff))) return rc;
  if ((rc = io.out(value_out, (size_t)nq * P, &dval))) return rc;
  if ((rc = io.out(grad_out, (size_t)nq * P * 3, &dgrad))) return rc;
  if ((rc = launch_eval_kin(h, nq, dq, nullptr, h->vis.as<double>()))) return rc;
  hipLaunchKernelGGL(k_eval_points, dim3((P + 255) / 256, nq), dim3(256), 0, h->stream, h->d_rb, h->d_px, h->d_py, h->d_pz,
                     h->d_plink, h->d_perm, want_field ? h->d_scenes + scene_id : nullptr, nq, h->vis.as<const double>(),
                     dbase, use_obs, dx, doff, dval, dgrad);
  HIPCHK(h, hipGetLastError());
  return io.finish();
}

int gto_eval_points_hessian(gto_handle* h, int32_t scene_id, int32_t nq, const double* q, const double* base_pos, int32_t use_obs,
                            double* hess_out) {
  if (!h || !q || !base_pos || !hess_out || nq < 0) return h ? fail(h, GTO_ERR_INVALID_ARG, "bad argument") : GTO_ERR_INVALID_ARG;
  if (nq == 0) return GTO_OK;
  if (!scene_valid(h, scene_id)) return fail(h, GTO_ERR_NO_SCENE, "unknown scene");
  HIPCHK(h, hipSetDevice(h->device));
  const int P = h->rb.n_points, L = h->rb.n_links;
  Staging io(h);
  const double *dq, *dbase;
  double* dh;
  int rc;
  if ((rc = io.in(q, (size_t)nq * h->rb.ndof, &dq))) return rc;
  if ((rc = io.in(base_pos, (size_t)nq * 3, &dbase))) return rc;
  if ((rc = ensure(h, h->vis, (size_t)nq * L * 12 * sizeof(double)))) return rc;
  if ((rc = io.out(hess_out, (size_t)nq * P * 9, &dh))) return rc;
  if ((rc = launch_eval_kin(h, nq, dq, nullptr, h->vis.as<double>()))) return rc;
  hipLaunchKernelGGL(k_eval_points_hessian, dim3((P + 255) / 256, nq), dim3(256), 0, h->stream, h->d_rb, h->d_px, h->d_py, h->d_pz, h->d_plink,
                     h->d_perm, h->d_scenes + scene_id, nq, h->vis.as<const double>(), dbase, use_obs, dh);
  HIPCHK(h, hipGetLastError());
  return io.finish();
}

// Shared by gto_eval_objective / gto_eval_obstacle_normal_eq: run init (kinematics + goal terms of Q as
// the "trial") and the obstacle kernel over all waypoints, then read the pieces back.
static int eval_common(gto_handle* h, int B, int n_max, const int32_t* scene_id, const double* goals,
                       const int32_t* n_goals, const double* standoff, const double* base_pos, const double* Q,
                       bool with_goals, std::vector<InstState>& states, std::vector<double>& blocks,
                       std::vector<double>& ssfixed) {
  int rc = check_scene_ids_host(h, scene_id, B);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof, T = h->opts.T;
  // a neutral goal set when the caller only wants obstacle terms
  std::vector<double> dummy_goal;
  std::vector<int32_t> dummy_n;
  std::vector<double> qc(B * ndof);
  for (int b = 0; b < B; ++b)
    for (size_t i = 0; i < ndof; ++i) qc[b * ndof + i] = Q[((size_t)b * ndof + i) * T];
  if (!with_goals) {
    n_max = 1;
    dummy_goal.assign((size_t)B * 16, 0.0);
    for (int b = 0; b < B; ++b) dummy_goal[b * 16] = dummy_goal[b * 16 + 5] = dummy_goal[b * 16 + 10] = dummy_goal[b * 16 + 15] = 1.0;
    dummy_n.assign(B, 1);
    goals = dummy_goal.data();
    n_goals = dummy_n.data();
    standoff = nullptr;
  }
  Staging io(h);  // inputs only: the pieces come back below
  const int32_t *d_sid, *d_ng;
  const double *d_qc, *d_goals, *d_so, *d_base, *d_Q0;
  if ((rc = io.in(scene_id, B, &d_sid))) return rc;
  if ((rc = io.in(qc.data(), B * ndof, &d_qc))) return rc;
  if ((rc = io.in(goals, (size_t)B * n_max * 16, &d_goals))) return rc;
  if ((rc = io.in(n_goals, B, &d_ng))) return rc;
  if ((rc = io.in(standoff, (size_t)B * 16, &d_so))) return rc;
  if ((rc = io.in(base_pos, (size_t)B * 3, &d_base))) return rc;
  if ((rc = io.in(Q, B * ndof * T, &d_Q0))) return rc;
  if ((rc = ensure_workspace(h, B))) return rc;
  SolveParams sp = make_params(h, n_max, standoff != nullptr);
  BatchPtrs bp = make_ptrs(h, d_sid, d_qc, d_goals, d_ng, d_so, d_base, d_Q0);
  HIPCHK(h, hipMemsetAsync(bp.n_done, 0, sizeof(int32_t), h->stream));
  hipLaunchKernelGGL(lm_init_kernel(h->np), dim3(B), dim3(256), 0, h->stream, h->d_rb, bp, sp, B, 1 /* raw: evaluate Q as given */);
  if ((rc = run_init_pass(h, h->stream, bp, sp, B))) return rc;
  h->last_launches = 0;
  ObsLaunch ev;
  ev.nT = (int)T - 2, ev.timed = h->profiling;
  if ((rc = launch_obstacle(h, h->stream, bp, sp, B, ev))) return rc;
  if (h->profiling) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms = ms;
  }
  states.resize(B);
  const size_t bstride = (size_t)h->np * h->np + h->np + 8;
  blocks.resize((size_t)B * T * bstride);
  ssfixed.resize((size_t)B * 4);
  HIPCHK(h, hipMemcpyAsync(states.data(), h->state.get(), B * sizeof(InstState), hipMemcpyDeviceToHost, h->stream));
  // trial slot is 1 right after init (slot = 0)
  HIPCHK(h, hipMemcpyAsync(blocks.data(), h->blocks.as<double>() + (size_t)1 * B * T * bstride,
                           blocks.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(ssfixed.data(), h->ssfixed.get(), ssfixed.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_eval_objective(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id, const double* goals,
                       const int32_t* n_goals, const double* standoff, const double* base_pos, const double* Q,
                       double* f_goal, double* f_obs, double* f_vel, int32_t* goal_argmin) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || n_max < 1 || !scene_id || !goals || !n_goals || !base_pos || !Q) return fail(h, GTO_ERR_INVALID_ARG, "bad argument");
  if (B == 0) return GTO_OK;
  std::vector<InstState> st;
  std::vector<double> blocks, ssf;
  int rc = eval_common(h, B, n_max, scene_id, goals, n_goals, standoff, base_pos, Q, true, st, blocks, ssf);
  if (rc) return rc;
  const int T = h->opts.T;
  for (int b = 0; b < B; ++b) {
    double so = ssf[4 * b] + ssf[4 * b + 1];
    const size_t bstride = (size_t)h->np * h->np + h->np + 8, bss = (size_t)h->np * h->np + h->np;
    for (int t = 2; t < T; ++t) so += blocks[((size_t)b * T + t) * bstride + bss];
    if (f_goal) f_goal[b] = st[b].fgoal_try[0];
    if (f_obs) f_obs[b] = h->opts.w_obstacle * so;
    if (f_vel) f_vel[b] = st[b].fvel_try[0];
    if (goal_argmin) goal_argmin[b] = st[b].argmin_try[0];
  }
  return GTO_OK;
}

int gto_eval_obstacle_normal_eq(gto_handle* h, int32_t B, const int32_t* scene_id, const double* base_pos, const double* Q,
                                double* JtJ, double* Jtr, double* sumsq) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || !scene_id || !base_pos || !Q) return fail(h, GTO_ERR_INVALID_ARG, "bad argument");
  if (B == 0) return GTO_OK;
  std::vector<InstState> st;
  std::vector<double> blocks, ssf;
  int rc = eval_common(h, B, 1, scene_id, nullptr, nullptr, nullptr, base_pos, Q, false, st, blocks, ssf);
  if (rc) return rc;
  const int T = h->opts.T, n = h->rb.n_opt;
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t) {
      const int np = h->np;
      const double* blk = &blocks[((size_t)b * T + t) * ((size_t)np * np + np + 8)];
      for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
          if (JtJ) JtJ[(((size_t)b * T + t) * n + i) * n + j] = (t < 2) ? 0.0 : blk[np * i + j];
        if (Jtr) Jtr[((size_t)b * T + t) * n + i] = (t < 2) ? 0.0 : blk[np * np + i];
      }
      if (sumsq) sumsq[(size_t)b * T + t] = (t < 2) ? ssf[4 * b + t] : blk[np * np + np];
    }
  return GTO_OK;
}

int gto_plan_cost(gto_handle* h, int32_t scene_id, int32_t n, const double* plans, const double* base_pos, double* cost_out,
                  double* dist_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (n < 0 || !plans || !base_pos || !cost_out) return fail(h, GTO_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return GTO_OK;
  if (!scene_valid(h, scene_id)) return fail(h, GTO_ERR_NO_SCENE, "unknown scene");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t ndof = h->rb.ndof, T = h->opts.T;
  Staging io(h);
  const double *dplans, *dbase;
  double* dpart;
  int rc;
  if ((rc = io.in(plans, (size_t)n * ndof * T, &dplans))) return rc;
  if ((rc = io.in(base_pos, 3, &dbase))) return rc;
  std::vector<double> part((size_t)n * T);
  if ((rc = io.out(part.data(), part.size(), &dpart))) return rc;
  const size_t pc_lds = sizeof(double) * plan_cost_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  if (pc_lds > 150 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the plan-cost kernel's LDS");
  HIPCHK(h, raise_dynamic_lds((const void*)k_plan_cost, pc_lds));
  hipLaunchKernelGGL(k_plan_cost, dim3((unsigned)((T + GTO_PLAN_TG - 1) / GTO_PLAN_TG), n), dim3(256), pc_lds, h->stream, h->d_rb, h->d_px, h->d_py, h->d_pz, h->d_plink,
                     h->d_scenes + scene_id, (int)T, dplans, dbase, dpart);
  HIPCHK(h, hipGetLastError());
  if ((rc = io.finish())) return rc;
  for (int i = 0; i < n; ++i) {
    double c = 0.0, dd = 0.0;
    for (size_t t = 0; t < T; ++t) c += part[(size_t)i * T + t];  // waypoint order, like the reference loop
    for (size_t j = 0; j < ndof; ++j) {
      double v = plans[((size_t)i * ndof + j) * T] - plans[((size_t)i * ndof + j) * T + T - 1];
      dd += v * v;
    }
    cost_out[i] = c;
    if (dist_out) dist_out[i] = std::sqrt(dd);
  }
  return GTO_OK;
}


// ------------------------------------------------------------------ cost field from a depth image (row f-2)
// Device buffers of gto_depth_sdf_cost are kept between calls (the entry point has no handle to hang them on): a call
// allocates a dozen buffers, and hipMalloc / hipFree cost more than the kernels for the reference's 5 cm grids.  A buffer is
// reused for a request of at most half its size up to its size; at most 1 GiB stays cached per process.
}  // extern "C"

namespace {
// On raw pointers, not owners: the pool has static storage duration, and an owner in it would call hipFree while the
// process exits, when the runtime may be gone already.  What is cached at exit is left to the process's end.
struct DepthPool {
  struct Item { int device; void* p; size_t cap; };
  std::mutex mu;
  std::vector<Item> items;
  size_t cached = 0;
  void* take(int device, size_t bytes, size_t* cap_out) {
    {
      std::lock_guard<std::mutex> lock(mu);
      for (size_t k = 0; k < items.size(); ++k)
        if (items[k].device == device && items[k].cap >= bytes && items[k].cap <= 2 * bytes + 4096) {
          void* p = items[k].p;
          *cap_out = items[k].cap;
          cached -= items[k].cap;
          items.erase(items.begin() + k);
          return p;
        }
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    *cap_out = bytes;
    return p;
  }
  void give(int device, void* p, size_t cap) {
    std::lock_guard<std::mutex> lock(mu);
    items.push_back({device, p, cap});
    cached += cap;
    while (cached > ((size_t)1 << 30) && !items.empty()) {  // oldest first
      (void)hipFree(items.front().p);
      cached -= items.front().cap;
      items.erase(items.begin());
    }
  }
};
DepthPool g_depth_pool;

// GTO_DEPTH_BRUTE / GTO_CLOUD_BRUTE ask for the exhaustive search (the reference construction; the two searches are compared
// in tests), GTO_DEPTH_STATS / GTO_CLOUD_STATS for the [gto] lines on stderr.  An entry-point call reads them once (the
// entry points without a handle have no Tunables that could hold them): with its lease, or by itself where it takes none.
struct SearchEnv { bool depth_brute, depth_stats, cloud_brute, cloud_stats; };
SearchEnv search_env() {
  auto set = [](const char* e) { return e && atoi(e) != 0; };
  return {set(getenv("GTO_DEPTH_BRUTE")), getenv("GTO_DEPTH_STATS") != nullptr, set(getenv("GTO_CLOUD_BRUTE")), getenv("GTO_CLOUD_STATS") != nullptr};
}

// What one call of an entry point (`who`, on handle `h` or none) holds of the pool, and how it reports its errors.  The
// buffers go back when the call ends, however it ends.
struct DepthLease {
  gto_handle* h;
  const char* who;
  int device;
  const SearchEnv env;
  std::vector<std::pair<void*, size_t>> bufs;
  DepthLease(gto_handle* h_, const char* who_, int device_) : h(h_), who(who_), device(device_), env(search_env()) {}
  DepthLease(const DepthLease&) = delete;
  ~DepthLease() { release(); }
  void release() {
    if (bufs.empty()) return;
    (void)hipDeviceSynchronize();  // nothing of this call may still be using them when the next call takes them
    for (auto& b : bufs) g_depth_pool.give(device, b.first, b.second);
    bufs.clear();
  }
  // a buffer of this call that outlives it: it leaves the lease with an owner (a gto_observation, a gto_occupancy)
  DevBuf keep(const void* p) {
    for (size_t k = 0; p && k < bufs.size(); ++k)
      if (bufs[k].first == p) {
        DevBuf b(bufs[k].first, bufs[k].second);
        bufs.erase(bufs.begin() + k);
        return b;
      }
    return DevBuf();
  }
  int no_memory() { return fail(h, GTO_ERR_ALLOC, std::string(who) + ": device allocation failed"); }
  int hip(hipError_t e) { return e == hipSuccess ? GTO_OK : fail(h, GTO_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
  // (the pool serves a request from the buffers of about its size that earlier calls gave back, first come first served: an
  // entry point asks for its buffers in the same order every time, so that each finds its own predecessor again)
  template <class T>
  T* alloc(size_t count) {
    size_t cap = 0;
    void* p = g_depth_pool.take(device, count ? count * sizeof(T) : 8, &cap);
    if (p) bufs.emplace_back(p, cap);
    return (T*)p;
  }
  template <class T>
  int upload(const T* host, size_t count, const T** dev) {  // a host array's copy on the device
    T* d = alloc<T>(count);
    *dev = d;
    if (!d) return no_memory();
    return count ? hip(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice)) : GTO_OK;
  }
  template <class T>
  int download(T* host, const T* dev, size_t count) {  // an output the caller may not have asked for (null), or an empty one
    return host && count ? hip(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost)) : GTO_OK;
  }
  int sync() {  // everything enqueued so far has run, and without an error
    const int rc = hip(hipGetLastError());
    return rc ? rc : hip(hipDeviceSynchronize());
  }
};
#define DEPTH_TRY(rc_expr)                     \
  do {                                         \
    if (const int rc_ = (rc_expr)) return rc_; \
  } while (0)

// The device of an entry point without a handle: `device`, made current, or the current one for a negative `device`
int select_device(int device, int* cur) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, GTO_ERR_NO_DEVICE, "no HIP device");
  if (device >= 0 && hipSetDevice(device) != hipSuccess) return fail(nullptr, GTO_ERR_NO_DEVICE, "hipSetDevice failed");
  *cur = 0;
  (void)hipGetDevice(cur);
  return GTO_OK;
}

// Wall-clock marks between the phases of a scene builder, for its line under GTO_DEPTH_STATS / GTO_CLOUD_STATS: one at
// the start, two of the builder's own, four of finish_scene
struct PhaseClock {
  double t[7];
  int n = 0;
  PhaseClock() { mark(); }
  void mark() { t[n++] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  bool full() const { return n == 7; }
  double ms(int from, int to) const { return t[to] - t[from]; }
};

// The two non-blocking streams of a device that the scene builders' searches run on, kept for the process
hipError_t depth_search_streams(int device, hipStream_t* sa, hipStream_t* sb) {
  static std::mutex mu;
  static std::vector<std::pair<int, std::pair<hipStream_t, hipStream_t>>> streams;
  std::lock_guard<std::mutex> lock(mu);
  for (auto& e : streams)
    if (e.first == device) {
      *sa = e.second.first, *sb = e.second.second;
      return hipSuccess;
    }
  hipError_t e = hipStreamCreateWithFlags(sa, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(sb, hipStreamNonBlocking);
  if (e == hipSuccess) streams.push_back({device, {*sa, *sb}});
  return e;
}

int upload_camera(DepthLease& c, const double* K, const double* Kinv, const double* pose, const double* inv, DepthCamera* cam) {
  double mats[9 + 9 + 16 + 16];
  std::memcpy(mats, K, 9 * sizeof(double));
  std::memcpy(mats + 9, Kinv, 9 * sizeof(double));
  std::memcpy(mats + 18, pose, 16 * sizeof(double));
  std::memcpy(mats + 34, inv, 16 * sizeof(double));
  const double* d;
  DEPTH_TRY(c.upload(mats, sizeof mats / sizeof *mats, &d));
  *cam = {d, d + 9, d + 18, d + 34};
  return GTO_OK;
}

// Depth image (device) + camera + mask -> the back-projected cloud, with its tile hierarchy when `want_tree` (the caller has
// checked that the image is within GTO_BVH_MAX_P), on the null stream.  d_valid [H * W]: the pixels' flags.
int make_depth_cloud(DepthLease& c, const float* d_depth, int H, int W, const DepthCamera& cam, const uint8_t* d_mask, double threshold,
                     bool want_tree, uint8_t* d_valid, DepthCloud* cl) {
  const size_t N = (size_t)H * W;
  const int P = want_tree ? tile_levels(H, W) : 0;
  double* d_p = c.alloc<double>(3 * N);
  double* d_boxes = P ? c.alloc<double>(bvh_box_doubles(P)) : nullptr;
  if (!d_p || (P && !d_boxes)) return c.no_memory();
  *cl = {d_depth, H, W, d_p, d_p + N, d_p + 2 * N, P, d_boxes};
  build_cloud(*cl, cam, d_mask, threshold, d_valid);
  return GTO_OK;
}

// The same from the host's image, camera matrices and mask (null: none), for the entry points that take one image
int upload_depth_cloud(DepthLease& c, const float* depth, int H, int W, const double* K, const double* Kinv, const double* pose,
                       const double* inv, const uint8_t* mask, double threshold, bool want_tree, DepthCamera* cam, uint8_t** d_valid,
                       DepthCloud* cl) {
  const size_t N = (size_t)H * W;
  const float* d_depth;
  const uint8_t* d_mask = nullptr;
  DEPTH_TRY(c.upload(depth, N, &d_depth));
  DEPTH_TRY(upload_camera(c, K, Kinv, pose, inv, cam));
  if (mask) DEPTH_TRY(c.upload(mask, N, &d_mask));
  *d_valid = c.alloc<uint8_t>(N);
  if (!*d_valid) return c.no_memory();
  return make_depth_cloud(c, d_depth, H, W, *cam, d_mask, threshold, want_tree, *d_valid, cl);
}

// Queries in Morton order of their position within a cloud's root box d_root_box (device; lo x y z, hi x y z): coherent
// waves.  30-bit keys, hipCUB radix sort of (key, index) on the null stream
int sort_queries(DepthLease& c, const double* d_root_box, DepthQueries* qs) {
  const long nq = qs->nq;
  if (nq >= ((int64_t)1 << 31)) return fail(c.h, GTO_ERR_UNSUPPORTED, std::string(c.who) + ": more than 2^31 queries");
  unsigned* d_keys = c.alloc<unsigned>((size_t)nq * 4);  // keys in / out, indices in / out
  if (!d_keys) return c.no_memory();
  unsigned *d_keys2 = d_keys + nq, *d_idx = d_keys + 2 * nq, *d_idx2 = d_keys + 3 * nq;
  hipLaunchKernelGGL(k_query_keys, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, 0, qs->q, nq, d_root_box, d_keys, d_idx);
  size_t tmp_bytes = 0;
  DEPTH_TRY(c.hip(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_keys, d_keys2, d_idx, d_idx2, (int)nq, 0, 30, (hipStream_t)0)));
  void* d_tmp = c.alloc<char>(tmp_bytes);
  if (!d_tmp) return c.no_memory();
  qs->order = d_idx2;
  return c.hip(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_keys, d_keys2, d_idx, d_idx2, (int)nq, 0, 30, (hipStream_t)0));
}

// Which search a cloud gets: the tree if it was built with one, unless the call runs under the exhaustive switch.  The tree
// search wants its queries sorted (sort_queries) and the exhaustive one ignores their order; sorting is the caller's step,
// since one order may serve two searches and the collision checks keep the caller's.
bool use_tree(const DepthCloud& cl, const SearchEnv& env) { return cl.P != 0 && !env.depth_brute; }
bool use_tree(const SampleCloud& cl, const SearchEnv& env) { return cl.n_leaves != 0 && !env.cloud_brute; }
void search_depth(const SearchEnv& env, hipStream_t stream, const DepthCloud& cl, const DepthCamera& cam, const DepthQueries& qs, float epsilon,
                  float w_inside, const DepthFields& out, unsigned long long* d_stats, bool cost_only) {
  if (use_tree(cl, env)) search_tree(stream, cl, cam, qs, epsilon, w_inside, out, d_stats, cost_only);
  else search_exhaustive(stream, cl, cam, qs, epsilon, w_inside, out);
}
void search_samples(const SearchEnv& env, hipStream_t stream, const SampleCloud& cl, int k, const DepthQueries& qs, float epsilon, float w_inside,
                    const CloudFields& out) {
  if (use_tree(cl, env)) search_cloud_tree(stream, cl, k, qs, epsilon, w_inside, out);
  else search_cloud_exhaustive(stream, cl, k, qs, epsilon, w_inside, out);
}

// The three counters k_depth_sdf_bvh adds to under GTO_DEPTH_STATS, zeroed (null without it, and when the pool has none left)
int depth_counters(DepthLease& c, unsigned long long** d_stats) {
  *d_stats = c.env.depth_stats ? c.alloc<unsigned long long>(3) : nullptr;
  return *d_stats ? c.hip(hipMemset(*d_stats, 0, 3 * sizeof(unsigned long long))) : GTO_OK;
}

// numpy.arange(start, stop, step) for doubles, value for value: the length is ceil((stop - start) / step), the fill is
// a[i] = start + i * ((start + step) - start) (numpy's DOUBLE_fill takes the increment from the first two elements)
std::vector<double> np_arange(double start, double stop, double step) {
  const double len = std::ceil((stop - start) / step);
  const long n = len > 0 ? (long)len : 0;
  std::vector<double> a((size_t)n);
  const double delta = (start + step) - start;
  for (long i = 0; i < n; ++i) a[i] = i == 0 ? start : (i == 1 ? start + step : start + (double)i * delta);
  return a;
}

// The voxel grid of a scene: the bounding box `bounds` of a cloud plus `margin` at `res` (gto/gto_models.py:155-171,
// numpy.arange's values).  axes: the centres along x, then y, then z.
struct VoxelGrid { double bounds[6]; std::vector<double> axes; int32_t shape[3]; double origin[3]; size_t nq; };
int plan_grid(gto_handle* h, const char* who, const double bounds[6], double margin, double res, VoxelGrid* g) {
  std::memcpy(g->bounds, bounds, sizeof g->bounds);
  g->axes.clear();
  g->nq = 1;
  for (int a = 0; a < 3; ++a) {
    const std::vector<double> ax = np_arange(bounds[a] - margin, bounds[3 + a] + margin, res);
    g->axes.insert(g->axes.end(), ax.begin(), ax.end());
    g->shape[a] = (int32_t)ax.size();
    g->origin[a] = bounds[a] - margin;
    g->nq *= ax.size();
  }
  if (g->nq == 0 || g->nq >= ((size_t)1 << 31)) return fail(h, GTO_ERR_UNSUPPORTED, std::string(who) + ": empty grid or more than 2^31 voxels");
  return GTO_OK;
}
// its voxel centres on the device, x slowest (null stream)
int make_grid_queries(DepthLease& c, const VoxelGrid& g, DepthQueries* qs) {
  const double* d_axes;
  DEPTH_TRY(c.upload(g.axes.data(), g.axes.size(), &d_axes));
  double* d_q = c.alloc<double>(g.nq * 3);
  if (!d_q) return c.no_memory();
  hipLaunchKernelGGL(k_grid_queries, dim3((unsigned)((g.nq + 255) / 256)), dim3(256), 0, 0, d_axes, g.shape[0], g.shape[1], g.shape[2], d_q);
  *qs = {d_q, (long)g.nq, nullptr};
  return GTO_OK;
}

// What both scene builders do once their clouds are built and the voxel centres laid out.  `search(sa, sb)` enqueues the one
// or two searches on the device's two search streams, behind everything the null stream has done so far: they are
// independent and each is bound by its slowest packets (the voxels deep behind the surfaces), so they run side by side.
// `searched()` follows when they are done.  Then the fields d_all / d_obs (null: one field) become scene `scene_id`, with
// their voxel records and distance fields, device to device; the lease goes back; the geometry goes out.  Marks of `clk`:
// searches enqueued from here, searches done, scene installed, lease released.
struct SceneGeometryOut { int32_t* shape; double *origin, *bounds; };  // of the caller; each may be null
template <class Search, class Searched>
int finish_scene(DepthLease& c, PhaseClock& clk, int32_t scene_id, const VoxelGrid& g, double res, const float* d_all, const float* d_obs,
                 const SceneGeometryOut& out, Search search, Searched searched) {
  hipStream_t sa = nullptr, sb = nullptr;
  DEPTH_TRY(c.hip(depth_search_streams(c.device, &sa, &sb)));
  DEPTH_TRY(c.hip(hipStreamSynchronize(0)));
  clk.mark();
  search(sa, sb);
  DEPTH_TRY(c.sync());
  clk.mark();
  DEPTH_TRY(searched());
  const int rc = set_scene_impl(c.h, scene_id, d_all, d_obs, g.shape, g.origin, res, false, hipMemcpyDeviceToDevice);
  clk.mark();
  c.release();
  clk.mark();
  if (rc) return rc;
  if (out.shape) std::memcpy(out.shape, g.shape, sizeof g.shape);
  if (out.origin) std::memcpy(out.origin, g.origin, sizeof g.origin);
  if (out.bounds) std::memcpy(out.bounds, g.bounds, sizeof g.bounds);
  return GTO_OK;
}

// What the sampled-mesh entry points check before any device work.  box_out: bounding box of the n samples (lo x y z, hi x y z).
int check_cloud(gto_handle* h, const char* who, const double* points, const double* normals, int64_t n, int32_t k, double box_out[6]) {
  const std::string w(who);
  if (!points || !normals) return fail(h, GTO_ERR_INVALID_ARG, w + ": null points or normals");
  if (k < 1 || k > GTO_CLOUD_MAX_K) return fail(h, GTO_ERR_INVALID_ARG, w + ": k must be in [1, 16]");
  if (n < k) return fail(h, GTO_ERR_INVALID_ARG, w + ": fewer samples than k");
  if (n > ((int64_t)1 << 28)) return fail(h, GTO_ERR_UNSUPPORTED, w + ": more than 2^28 samples");
  for (int a = 0; a < 3; ++a) box_out[a] = INFINITY, box_out[3 + a] = -INFINITY;
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const double v = points[3 * i + a];
      if (!std::isfinite(v) || !std::isfinite(normals[3 * i + a])) return fail(h, GTO_ERR_INVALID_ARG, w + ": non-finite point or normal");
      box_out[a] = std::min(box_out[a], v), box_out[3 + a] = std::max(box_out[3 + a], v);
    }
  return GTO_OK;
}

// The samples d_points / d_normals [n][3] (device) as a SampleCloud; under their hierarchy, in key order, unless the call
// runs under the exhaustive switch.  box: their bounding box (check_cloud).
int make_sample_cloud(DepthLease& c, const double* d_points, const double* d_normals, int64_t n, const double box[6], SampleCloud* cl) {
  *cl = {d_points, d_normals, (unsigned)n, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr};
  if (c.env.cloud_brute) return GTO_OK;
  // k_query_keys spreads its keys over a box grown by its own extent on every side (queries lie around a cloud): the
  // samples lie within their box, so it is handed the middle third and the keys use all their bits
  double kbox[6];
  for (int a = 0; a < 3; ++a) {
    const double third = (box[3 + a] - box[a]) / 3.0;
    kbox[a] = box[a] + third, kbox[3 + a] = box[3 + a] - third;
  }
  const double* d_kbox;
  DEPTH_TRY(c.upload(kbox, 6, &d_kbox));
  DepthQueries ps = {d_points, (long)n, nullptr};
  DEPTH_TRY(sort_queries(c, d_kbox, &ps));
  cl->n_leaves = cloud_leaf_slots((unsigned)n);
  cl->n_slots = (unsigned)((n + GTO_CLOUD_LEAF - 1) / GTO_CLOUD_LEAF) * GTO_CLOUD_LEAF;
  cl->px = c.alloc<double>((size_t)cl->n_slots * 3);
  cl->pid = c.alloc<unsigned>(cl->n_slots);
  cl->boxes = c.alloc<double>((size_t)2 * cl->n_leaves * 6);
  if (!cl->px || !cl->pid || !cl->boxes) return c.no_memory();
  cl->py = cl->px + cl->n_slots, cl->pz = cl->px + 2 * (size_t)cl->n_slots;
  build_sample_tree(*cl, ps.order);
  return c.hip(hipGetLastError());
}

}  // namespace

extern "C" {

int gto_depth_sdf_cost(int device, const float* depth, int32_t H, int32_t W, const double* K, const double* Kinv,
                       const double* cam_pose, const double* cam_inv, const uint8_t* target_mask, double threshold,
                       const double* query, int64_t nq, float epsilon, float w_inside, float* sdf_out,
                       uint8_t* inside_out, float* cost_out, double* points_out, uint8_t* valid_out) {
  if (!depth || !K || !Kinv || !cam_pose || !cam_inv || H < 1 || W < 1 || nq < 0 || (nq > 0 && !query))
    return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_depth_sdf_cost: null or empty input");
  int cur_dev;
  DEPTH_TRY(select_device(device, &cur_dev));
  DepthLease c(nullptr, "gto_depth_sdf_cost", cur_dev);
  // bounding-box hierarchy over 8 x 4 pixel tiles of the depth image (k_depth_sdf_bvh): the exhaustive search's distances,
  // bit for bit.  No hierarchy, and the exhaustive search itself, on request, and for images with more tiles per side
  // than k_bvh_up builds; none without queries either
  const bool tree = nq && !c.env.depth_brute && tile_levels(H, W) <= GTO_BVH_MAX_P;
  const size_t N = (size_t)H * W;
  DepthQueries qs = {nullptr, (long)nq, nullptr};
  DEPTH_TRY(c.upload(query, (size_t)nq * 3, &qs.q));
  const DepthFields out = {c.alloc<float>((size_t)nq), c.alloc<uint8_t>((size_t)nq), c.alloc<float>((size_t)nq)};
  if (!out.sdf || !out.inside || !out.cost) return c.no_memory();
  DepthCamera cam;
  DepthCloud cloud;
  uint8_t* d_valid;
  DEPTH_TRY(upload_depth_cloud(c, depth, H, W, K, Kinv, cam_pose, cam_inv, target_mask, threshold, tree, &cam, &d_valid, &cloud));
  unsigned long long* d_stats = nullptr;
  if (tree) {
    DEPTH_TRY(depth_counters(c, &d_stats));
    DEPTH_TRY(sort_queries(c, cloud.boxes, &qs));
  }
  if (nq) search_depth(c.env, 0, cloud, cam, qs, epsilon, w_inside, out, d_stats, false);
  if (d_stats) {
    unsigned long long st[3];
    DEPTH_TRY(c.download(st, d_stats, 3));
    fprintf(stderr, "[gto] depth field search: %lld queries, nodes popped per query %.1f, leaves per query %.1f, loop iterations per wave %.1f\n",
            (long long)nq, (double)st[0] / nq, (double)st[1] / nq, (double)st[2] / ((nq + 63) / 64));
  }
  DEPTH_TRY(c.sync());
  DEPTH_TRY(c.download(sdf_out, out.sdf, (size_t)nq));
  DEPTH_TRY(c.download(cost_out, out.cost, (size_t)nq));
  DEPTH_TRY(c.download(inside_out, out.inside, (size_t)nq));
  DEPTH_TRY(c.download(valid_out, d_valid, N));
  if (points_out) {
    std::vector<double> soa(3 * N);
    DEPTH_TRY(c.download(soa.data(), cloud.px, 3 * N));
    for (size_t i = 0; i < N; ++i)
      for (int r = 0; r < 3; ++r) points_out[3 * i + r] = soa[(size_t)r * N + i];
  }
  return GTO_OK;
}

/* include/gto_solver.h: the per-object perception steps of examples/pybullet_gto_planning.py:176-190 in one call, with
 * nothing but the grid geometry coming back to the host.  The depth image goes up once; the cloud of all pixels and the
 * cloud without the target's pixels are back-projected from it; the grid is the bounding box of the first cloud plus
 * `margin` at `grid_res`; both cost fields are searched with ONE ordering of the voxel centres (one key pass, one radix
 * sort) against the two tile hierarchies, and installed as scene `scene_id`. */
int gto_scene_from_depth(gto_handle* h, int32_t scene_id, const float* depth, int32_t H, int32_t W, const double* K,
                         const double* Kinv, const double* cam_pose, const double* cam_inv, const uint8_t* target_mask,
                         const float* depth_obstacle, double threshold, double grid_res, double margin, float epsilon,
                         float w_inside, int32_t* shape_out, double* origin_out, double* bounds_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!depth || !K || !Kinv || !cam_pose || !cam_inv || H < 1 || W < 1 || !(grid_res > 0) || !(margin >= 0))
    return fail(h, GTO_ERR_INVALID_ARG, "gto_scene_from_depth: null or empty input");
  HIPCHK(h, hipSetDevice(h->device));
  PhaseClock clk;
  const size_t N = (size_t)H * W;
  if (tile_levels(H, W) > GTO_BVH_MAX_P) return fail(h, GTO_ERR_UNSUPPORTED, "gto_scene_from_depth: image larger than 8192 x 4096 pixels");
  DepthLease c(h, "gto_scene_from_depth", h->device);
  // the second cloud: the obstacle image (the driver's depth_obstacle, examples/pybullet_gto_planning.py:187-189: the target's
  // pixels pushed to the threshold) without the masked pixels; its visibility test reads the obstacle image
  const bool two = target_mask != nullptr || depth_obstacle != nullptr;
  const float *d_depth, *d_depth_o;
  const uint8_t* d_mask = nullptr;
  DepthCamera cam;
  DEPTH_TRY(c.upload(depth, N, &d_depth));
  d_depth_o = d_depth;
  if (depth_obstacle) DEPTH_TRY(c.upload(depth_obstacle, N, &d_depth_o));
  DEPTH_TRY(upload_camera(c, K, Kinv, cam_pose, cam_inv, &cam));
  if (target_mask) DEPTH_TRY(c.upload(target_mask, N, &d_mask));
  uint8_t* d_valid = c.alloc<uint8_t>(N);
  if (!d_valid) return c.no_memory();
  clk.mark();
  // the hierarchy of the first cloud: its root box is the bounding box of the valid points (gto/gto_models.py:155-157)
  DepthCloud all, obs;
  DEPTH_TRY(make_depth_cloud(c, d_depth, H, W, cam, nullptr, threshold, true, d_valid, &all));
  obs = all;
  if (two) DEPTH_TRY(make_depth_cloud(c, d_depth_o, H, W, cam, d_mask, threshold, true, d_valid, &obs));
  double root[6];
  DEPTH_TRY(c.download(root, all.boxes, 6));  // (synchronises with the null stream)
  clk.mark();
  if (!(root[0] <= root[3]) || !std::isfinite(root[0]) || !std::isfinite(root[3]))
    return fail(h, GTO_ERR_INVALID_ARG, "gto_scene_from_depth: no valid pixel in the depth image");
  VoxelGrid grid;
  DEPTH_TRY(plan_grid(h, c.who, root, margin, grid_res, &grid));
  DepthQueries qs;
  DEPTH_TRY(make_grid_queries(c, grid, &qs));
  const size_t nq = grid.nq;
  float* d_costa = c.alloc<float>(nq);
  float* d_costo = two ? c.alloc<float>(nq) : nullptr;
  uint8_t* d_in = c.alloc<uint8_t>(nq);
  uint8_t* d_in2 = two ? c.alloc<uint8_t>(nq) : nullptr;
  if (!d_costa || !d_in || (two && (!d_costo || !d_in2))) return c.no_memory();
  DEPTH_TRY(sort_queries(c, all.boxes, &qs));
  unsigned long long* d_stats;
  DEPTH_TRY(depth_counters(c, &d_stats));
  if (c.env.depth_stats) DEPTH_TRY(c.hip(hipDeviceSynchronize()));
  const int rc = finish_scene(
      c, clk, scene_id, grid, grid_res, d_costa, d_costo, {shape_out, origin_out, bounds_out},
      [&](hipStream_t sa, hipStream_t sb) {  // (always the tree: the image is within its limit, and a scene is not a reference construction)
        search_tree(sa, all, cam, qs, epsilon, w_inside, {nullptr, d_in, d_costa}, d_stats, true);
        if (two) search_tree(sb, obs, cam, qs, epsilon, w_inside, {nullptr, d_in2, d_costo}, nullptr, true);
      },
      [&]() {
        unsigned long long stv[3];
        const int rc = c.download(stv, d_stats, d_stats ? 3 : 0);
        if (d_stats && !rc)
          fprintf(stderr, "[gto] depth field search (first cloud): %zu queries, nodes popped per wave %.1f, leaves per wave %.1f\n", nq,
                  (double)stv[2] / ((nq + 63) / 64), (double)stv[1] / 64 / ((nq + 63) / 64));
        return rc;
      });
  if (c.env.depth_stats && clk.full())
    fprintf(stderr, "[gto] scene from depth (%d x %d image, %zu voxels), ms: alloc + upload %.3f | back-projection, hierarchies, bounds %.3f | queries, keys, sort %.3f | "
                    "two searches %.3f | records + distance fields %.3f | release %.3f | total %.3f\n",
            H, W, nq, clk.ms(0, 1), clk.ms(1, 2), clk.ms(2, 3), clk.ms(3, 4), clk.ms(4, 5), clk.ms(5, 6), clk.ms(0, 6));
  return rc;
}


// ------------------------------------------------------------------ cost field from a sampled mesh (gto_cloud.h)
int gto_cloud_sdf_cost(int device, const double* points, const double* normals, int64_t n, int32_t k, const double* query,
                       int64_t nq, float epsilon, float w_inside, float* sdf_out, uint8_t* inside_out, float* cost_out,
                       int32_t* nearest_out) {
  double box[6];
  if (int rc = check_cloud(nullptr, "gto_cloud_sdf_cost", points, normals, n, k, box)) return rc;
  if (nq < 0 || (nq > 0 && !query)) return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_cloud_sdf_cost: null or negative query count");
  int cur_dev;
  DEPTH_TRY(select_device(device, &cur_dev));
  if (nq == 0) return GTO_OK;
  DepthLease c(nullptr, "gto_cloud_sdf_cost", cur_dev);
  const double *d_points, *d_normals;
  DepthQueries qs = {nullptr, (long)nq, nullptr};
  DEPTH_TRY(c.upload(points, (size_t)n * 3, &d_points));
  DEPTH_TRY(c.upload(normals, (size_t)n * 3, &d_normals));
  DEPTH_TRY(c.upload(query, (size_t)nq * 3, &qs.q));
  const CloudFields out = {c.alloc<float>((size_t)nq), c.alloc<uint8_t>((size_t)nq), c.alloc<float>((size_t)nq), c.alloc<int32_t>((size_t)nq)};
  if (!out.sdf || !out.inside || !out.cost || !out.nearest) return c.no_memory();
  SampleCloud cl;
  DEPTH_TRY(make_sample_cloud(c, d_points, d_normals, n, box, &cl));
  if (use_tree(cl, c.env)) DEPTH_TRY(sort_queries(c, cl.boxes, &qs));
  search_samples(c.env, 0, cl, k, qs, epsilon, w_inside, out);
  DEPTH_TRY(c.sync());
  DEPTH_TRY(c.download(sdf_out, out.sdf, (size_t)nq));
  DEPTH_TRY(c.download(inside_out, out.inside, (size_t)nq));
  DEPTH_TRY(c.download(cost_out, out.cost, (size_t)nq));
  DEPTH_TRY(c.download(nearest_out, out.nearest, (size_t)nq));
  return GTO_OK;
}

/* include/gto_solver.h: gto_scene_from_depth's counterpart for sampled meshes.  The samples go up once through the handle's
 * staging; the first n_obstacle of them are the second cloud.  One ordering of the voxel centres serves both searches. */
int gto_scene_from_clouds(gto_handle* h, int32_t scene_id, const double* points, const double* normals, int64_t n_all,
                          int64_t n_obstacle, int32_t k, double grid_res, double margin, float epsilon, float w_inside,
                          int32_t* shape_out, double* origin_out, double* bounds_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!(grid_res > 0) || !(margin >= 0)) return fail(h, GTO_ERR_INVALID_ARG, "gto_scene_from_clouds: grid_res must be > 0 and margin >= 0");
  if (n_obstacle > n_all) return fail(h, GTO_ERR_INVALID_ARG, "gto_scene_from_clouds: n_obstacle must be <= n_all");
  double root[6], box_o[6];
  if (int rc = check_cloud(h, "gto_scene_from_clouds", points, normals, n_all, k, root)) return rc;
  const bool two = n_obstacle != n_all;
  if (two)
    if (int rc = check_cloud(h, "gto_scene_from_clouds", points, normals, n_obstacle, k, box_o)) return rc;
  VoxelGrid grid;
  DEPTH_TRY(plan_grid(h, "gto_scene_from_clouds", root, margin, grid_res, &grid));
  HIPCHK(h, hipSetDevice(h->device));
  PhaseClock clk;
  Staging io(h);  // inputs only: nothing but the geometry returns
  const double *d_points, *d_normals;
  DEPTH_TRY(io.in(points, (size_t)n_all * 3, &d_points));
  DEPTH_TRY(io.in(normals, (size_t)n_all * 3, &d_normals));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // the pipeline below runs on the null stream and two search streams
  clk.mark();
  DepthLease c(h, "gto_scene_from_clouds", h->device);
  SampleCloud all, obs;
  DEPTH_TRY(make_sample_cloud(c, d_points, d_normals, n_all, root, &all));
  obs = all;
  if (two) DEPTH_TRY(make_sample_cloud(c, d_points, d_normals, n_obstacle, box_o, &obs));
  if (c.env.cloud_stats) DEPTH_TRY(c.hip(hipDeviceSynchronize()));
  clk.mark();
  DepthQueries qs;
  DEPTH_TRY(make_grid_queries(c, grid, &qs));
  float* d_costa = c.alloc<float>(grid.nq);
  float* d_costo = two ? c.alloc<float>(grid.nq) : nullptr;
  if (!d_costa || (two && !d_costo)) return c.no_memory();
  const bool tree = use_tree(all, c.env);
  if (tree) DEPTH_TRY(sort_queries(c, all.boxes, &qs));  // one key pass and one sort for both fields, over the root box of all samples
  const int rc = finish_scene(
      c, clk, scene_id, grid, grid_res, d_costa, d_costo, {shape_out, origin_out, bounds_out},
      [&](hipStream_t sa, hipStream_t sb) {
        search_samples(c.env, sa, all, k, qs, epsilon, w_inside, {nullptr, nullptr, d_costa, nullptr});
        if (two) search_samples(c.env, sb, obs, k, qs, epsilon, w_inside, {nullptr, nullptr, d_costo, nullptr});
      },
      []() { return (int)GTO_OK; });
  if (c.env.cloud_stats && clk.full())
    fprintf(stderr, "[gto] scene from clouds (%lld + %lld samples, k %d, %zu voxels, %s), ms: upload %.3f | sort + build %.3f | queries, keys, sort %.3f | "
                    "search %.3f | records + distance fields %.3f | total %.3f\n",
            (long long)n_all, (long long)(two ? n_obstacle : 0), (int)k, grid.nq, tree ? "tree" : "exhaustive", clk.ms(0, 1), clk.ms(1, 2), clk.ms(2, 3),
            clk.ms(3, 4), clk.ms(4, 6), clk.ms(0, 6));
  return rc;
}

/* The two cost fields of a resident scene, device to host (float32 [nx ny nz] each; either pointer may be null). */
int gto_get_scene_fields(gto_handle* h, int32_t scene_id, float* c_all_out, float* c_obs_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!scene_valid(h, scene_id)) return fail(h, GTO_ERR_NO_SCENE, "gto_get_scene_fields: the scene was never set");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const SceneDev& s = h->scenes[scene_id];
  const size_t nvox = (size_t)s.nx * s.ny * s.nz;
  if (c_all_out) HIPCHK(h, hipMemcpy(c_all_out, s.c_all, nvox * sizeof(float), hipMemcpyDeviceToHost));
  if (c_obs_out) HIPCHK(h, hipMemcpy(c_obs_out, s.c_obs, nvox * sizeof(float), hipMemcpyDeviceToHost));
  return GTO_OK;
}

// ------------------------------------------------------------------ retiming under joint velocity / acceleration limits
// (convert_plan_to_trajectory_toppra, gto/utils.py:283-323; kernels: gto_retime.h)

// Thomas factors of the not-a-knot system of uniform knots, scaled by 1/h: rows [1 2], [1 4 1] ... [1 4 1], [2 1]
// (scipy.interpolate.CubicSpline's banded system for n >= 4).  Rows 0 .. C-2 do not depend on the number of knots C, so one
// table of interior rows serves every C <= GTO_RETIME_MAX_N.  [4][GTO_RETIME_MAX_N] (GTO_RT_FAC_*): multiplier, reciprocal
// pivot, upper entry and pivot of row i.  The last row of a system of C knots is k_retime_spline's, per lane:
//   lo = 2 / piv[C-2];  piv = 1 - lo * up[C-2];  inv = 1 / piv      (the order of operations of the interior rows below)
static std::vector<double> retime_factors() {
  const int L = GTO_RETIME_MAX_N;
  std::vector<double> f(4 * (size_t)L, 0.0);
  double* lo = f.data() + GTO_RT_FAC_LO * L;
  double* inv = f.data() + GTO_RT_FAC_INV * L;
  double* up = f.data() + GTO_RT_FAC_UP * L;
  double* pv = f.data() + GTO_RT_FAC_PIV * L;
  double piv = 1.0;
  up[0] = 2.0;
  inv[0] = 1.0 / piv;
  pv[0] = piv;
  for (int i = 1; i < L; ++i) {
    up[i] = 1.0;
    lo[i] = 1.0 / piv;
    piv = 4.0 - lo[i] * up[i - 1];
    inv[i] = 1.0 / piv;
    pv[i] = piv;
  }
  return f;
}

// what an entry point calls itself, its column count and its input array in error messages
struct RetimeNames {
  const char *fn, *T, *array;
};
static const RetimeNames RETIME_BATCH = {"gto_retime_batch", "T", "plans"}, RETIME_PATHS = {"gto_retime_paths", "Tp", "paths"};
static const RetimeNames RETIME_CONVEX = {"gto_retime_paths_convex", "Tp", "paths"};
static const RetimeNames RETIME_TORQUE = {"gto_retime_paths_torque", "Tp", "paths"};

// what gto_retime_paths_torque adds to the convex call: the limits (checked, by value), the payload of every path
// (DEVICE [B], [B,3], [B,6], each or all null) and tau_out (DEVICE [B,M,ndof] or null)
// the torque entry points' own arguments as the caller gave them (tau_max HOST; the rest HOST or DEVICE like the call)
struct RetimeTorqueArgs {
  const double *tau_max, *pl_mass, *pl_com, *pl_inertia;
  double* tau_out;
};
struct RetimeTorqueCall {
  RetimeTorque lim;
  const double *pl_mass, *pl_com, *pl_inertia;
  double* tau_out;
};

static int retime_check(gto_handle* h, const RetimeNames& nm, int32_t B, int32_t Tp, const double* vmax, const double* amax,
                        int32_t subdiv, int32_t M, RetimeLimits& lim, RetimeDims& d) {
  const int ndof = h->rb.ndof;
  const std::string f = std::string(nm.fn) + ": ", Tname = nm.T;
  if (B < 0) return fail(h, GTO_ERR_INVALID_ARG, f + "B must be >= 0");
  if (Tp < 2) return fail(h, GTO_ERR_INVALID_ARG, f + Tname + " must be >= 2");
  if (!vmax || !amax) return fail(h, GTO_ERR_INVALID_ARG, f + "null limit array");
  for (int j = 0; j < ndof; ++j) {
    if (!(vmax[j] > 0.0)) return fail(h, GTO_ERR_INVALID_ARG, f + "vmax must be > 0 (+inf: no limit)");
    if (!(amax[j] > 0.0) || !std::isfinite(amax[j])) return fail(h, GTO_ERR_INVALID_ARG, f + "amax must be finite and > 0");
    lim.vmax[j] = vmax[j], lim.amax[j] = amax[j];
  }
  if (subdiv < 1 || M < 2) return fail(h, GTO_ERR_INVALID_ARG, f + "subdiv must be >= 1 and M >= 2");
  const long long N = (long long)subdiv * (Tp - 1) + 1;
  if (N > GTO_RETIME_MAX_N) return fail(h, GTO_ERR_INVALID_ARG, f + "subdiv (" + Tname + "-1) + 1 must be <= 1024");
  if ((long long)B * std::max<long long>(N, M) * std::max(ndof, 1) > (long long)INT32_MAX * 64)
    return fail(h, GTO_ERR_UNSUPPORTED, f + "batch too large for one call");
  d.B = B, d.ndof = ndof, d.Tp = Tp, d.Nmax = (int)N, d.subdiv = subdiv, d.M = M;
  return GTO_OK;
}

// the options of the convex solve
static int retime_convex_check(gto_handle* h, const RetimeNames& nm, const RetimeConvex& cv) {
  const std::string f = std::string(nm.fn) + ": ";
  if (!(cv.gap_tol > 0.0) || !std::isfinite(cv.gap_tol)) return fail(h, GTO_ERR_INVALID_ARG, f + "gap_tol must be finite and > 0");
  if (cv.max_newton < 1) return fail(h, GTO_ERR_INVALID_ARG, f + "max_newton must be >= 1");
  return GTO_OK;
}

// the torque call's own arguments: inertials on the handle, tau_max, and which payload arrays come together
static int retime_torque_check(gto_handle* h, const RetimeNames& nm, const double* tau_max, const double* payload_mass,
                               const double* payload_com, const double* payload_inertia, RetimeTorque& lim) {
  const std::string f = std::string(nm.fn) + ": ";
  if (!h->has_inertials) return fail(h, GTO_ERR_INVALID_ARG, "no link inertials set");
  if (!tau_max) return fail(h, GTO_ERR_INVALID_ARG, f + "null limit array");
  for (int j = 0; j < h->rb.ndof; ++j) {
    if (!(tau_max[j] > 0.0)) return fail(h, GTO_ERR_INVALID_ARG, f + "tau_max must be > 0 (+inf: no limit)");
    lim.tau_max[j] = tau_max[j];
  }
  if (!payload_mass && (payload_com || payload_inertia))
    return fail(h, GTO_ERR_INVALID_ARG, f + "payload_com / payload_inertia without payload_mass");
  return GTO_OK;
}

static unsigned retime_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// the four launches of a checked call (d, lim: retime_check's); n_cols: DEVICE [B] or NULL (every path has Tp columns).
// cv: NULL for the greedy profile (k_retime_pass), else the convex solve's options (k_retime_convex in its place, which
// also fills iters_out).  tq: NULL, or the torque call's additions: k_retime_torque_rows in front of k_retime_convex_torque,
// and k_retime_tau behind the samples when tau_out is asked for.  Without tq the launches are what they were.
static int retime_launch(gto_handle* h, const RetimeDims& d, const RetimeLimits& lim, const double* plans,
                         const int32_t* n_cols, double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out,
                         double* qd_out, double* qdd_out, int32_t* status_out, void* stream,
                         const RetimeConvex* cv = nullptr, int32_t* iters_out = nullptr,
                         const RetimeTorqueCall* tq = nullptr) {
  int rc;
  const int B = d.B, M = d.M;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const size_t T = d.Tp, N = d.Nmax, nd = d.ndof, nB = (size_t)B;
  if (!h->rt_fac_ready) {  // once per handle: the table serves every column count
    const std::vector<double> f = retime_factors();
    if ((rc = ensure(h, h->rt_fac, f.size() * sizeof(double)))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->rt_fac.get(), f.data(), f.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    h->rt_fac_ready = true;
  }
  if ((rc = ensure(h, h->rt_S, nB * nd * T * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->rt_flag, nB * nd * sizeof(int32_t)))) return rc;
  if ((rc = ensure(h, h->rt_P1, nB * N * nd * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->rt_P2, nB * N * nd * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->rt_cap, nB * N * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->rt_X, nB * N * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->rt_T, nB * N * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->rt_stat, nB * sizeof(int32_t)))) return rc;
  if (tq) {
    for (DevBuf* w : {&h->rt_TA, &h->rt_TB, &h->rt_TG})
      if ((rc = ensure(h, *w, nB * N * nd * sizeof(double)))) return rc;
    if (tq->tau_out) {  // the samples tau_out is computed from, where the caller does not take them
      if (!q_out && (rc = ensure(h, h->rt_q, nB * M * nd * sizeof(double)))) return rc;
      if (!qd_out && (rc = ensure(h, h->rt_qd, nB * M * nd * sizeof(double)))) return rc;
      if (!qdd_out && (rc = ensure(h, h->rt_qdd, nB * M * nd * sizeof(double)))) return rc;
      if (!q_out) q_out = h->rt_q.as<double>();
      if (!qd_out) qd_out = h->rt_qd.as<double>();
      if (!qdd_out) qdd_out = h->rt_qdd.as<double>();
    }
  }
  double *S = h->rt_S.as<double>(), *P1 = h->rt_P1.as<double>(), *P2 = h->rt_P2.as<double>(), *cap = h->rt_cap.as<double>();
  double *X = h->rt_X.as<double>(), *Tg = h->rt_T.as<double>();
  int32_t *flag = h->rt_flag.as<int32_t>(), *stat = h->rt_stat.as<int32_t>();
  hipLaunchKernelGGL(k_retime_spline, dim3(retime_blocks((long long)B * nd, 256)), dim3(256), 0, st, plans,
                     h->rt_fac.as<const double>(), n_cols, d, S, flag);
  hipLaunchKernelGGL(k_retime_grid, dim3(retime_blocks((long long)B * N, 256)), dim3(256), 0, st, plans, S, flag, n_cols, lim,
                     d, P1, P2, cap);
  const int rows = rnea_rows_per_block(h->rb.n_frames);
  const size_t rnea_lds = sizeof(double) * GTO_RNEA_SLOTS * h->rb.n_frames * rows;
  if (tq) {
    double *TA = h->rt_TA.as<double>(), *TB = h->rt_TB.as<double>(), *TG = h->rt_TG.as<double>();
    hipLaunchKernelGGL(k_retime_torque_rows, dim3(retime_blocks((long long)B * N, rows)), dim3(GTO_WAVE), rnea_lds, st, h->d_rb,
                       h->dyn_buf.as<const DynDev>(), plans, S, flag, n_cols, P1, P2, tq->pl_mass, tq->pl_com, tq->pl_inertia, d,
                       rows, TA, TB, TG);
    hipLaunchKernelGGL(k_retime_convex_torque, dim3(B), dim3(64), GTO_RT_LDS_ARRAYS * N * sizeof(double), st, P1, P2, cap, flag,
                       n_cols, lim, d, *cv, X, Tg, stat, duration_out, t_grid_out, sd_grid_out, status_out, iters_out, tq->lim,
                       TA, TB, TG);
  } else if (cv)
    hipLaunchKernelGGL(k_retime_convex, dim3(B), dim3(64), GTO_RT_LDS_ARRAYS * N * sizeof(double), st, P1, P2, cap, flag, n_cols, lim, d, *cv,
                       X, Tg, stat, duration_out, t_grid_out, sd_grid_out, status_out, iters_out);
  else
    hipLaunchKernelGGL(k_retime_pass, dim3(B), dim3(64), 0, st, P1, P2, cap, flag, n_cols, lim, d, X, Tg, stat,
                       duration_out, t_grid_out, sd_grid_out, status_out);
  if (q_out || qd_out || qdd_out)
    hipLaunchKernelGGL(k_retime_sample, dim3(retime_blocks((long long)B * M, 256)), dim3(256), 0, st, plans, S, X, Tg, stat,
                       n_cols, d, q_out, qd_out, qdd_out);
  if (tq && tq->tau_out)
    hipLaunchKernelGGL(k_retime_tau, dim3(retime_blocks((long long)B * M, rows)), dim3(GTO_WAVE), rnea_lds, st, h->d_rb,
                       h->dyn_buf.as<const DynDev>(), (long long)B * M, M, rows, q_out, qd_out, qdd_out, tq->pl_mass, tq->pl_com,
                       tq->pl_inertia, tq->tau_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

// the device-pointer entry points: checks, then the launches
static int retime_device(gto_handle* h, const RetimeNames& nm, int32_t B, int32_t Tp, const double* paths,
                         const int32_t* n_cols, const double* vmax, const double* amax, int32_t subdiv, int32_t M,
                         double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out, double* qd_out,
                         double* qdd_out, int32_t* status_out, void* stream, const RetimeConvex* cv = nullptr,
                         int32_t* iters_out = nullptr, const RetimeTorqueArgs* ta = nullptr) {
  if (!h) return GTO_ERR_INVALID_ARG;
  RetimeLimits lim = {};
  RetimeDims d = {};
  RetimeTorqueCall tq = {};
  int rc = retime_check(h, nm, B, Tp, vmax, amax, subdiv, M, lim, d);
  if (rc) return rc;
  if (cv && (rc = retime_convex_check(h, nm, *cv))) return rc;
  if (ta && (rc = retime_torque_check(h, nm, ta->tau_max, ta->pl_mass, ta->pl_com, ta->pl_inertia, tq.lim))) return rc;
  if (B == 0) return GTO_OK;
  if (!paths) return fail(h, GTO_ERR_INVALID_ARG, std::string(nm.fn) + ": null " + nm.array);
  if (ta) tq.pl_mass = ta->pl_mass, tq.pl_com = ta->pl_com, tq.pl_inertia = ta->pl_inertia, tq.tau_out = ta->tau_out;
  return retime_launch(h, d, lim, paths, n_cols, duration_out, t_grid_out, sd_grid_out, q_out, qd_out, qdd_out, status_out,
                       stream, cv, iters_out, ta ? &tq : nullptr);
}

// the host-pointer entry points: n_cols is a HOST array here (or NULL), checked before anything is staged
static int retime_host(gto_handle* h, const RetimeNames& nm, int32_t B, int32_t Tp, const double* paths,
                       const int32_t* n_cols, const double* vmax, const double* amax, int32_t subdiv, int32_t M,
                       double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out, double* qd_out,
                       double* qdd_out, int32_t* status_out, const RetimeConvex* cv = nullptr, int32_t* iters_out = nullptr,
                       const RetimeTorqueArgs* ta = nullptr) {
  if (!h) return GTO_ERR_INVALID_ARG;
  RetimeLimits lim = {};
  RetimeDims d = {};
  RetimeTorqueCall tq = {};
  int rc = retime_check(h, nm, B, Tp, vmax, amax, subdiv, M, lim, d);
  if (rc) return rc;
  if (cv && (rc = retime_convex_check(h, nm, *cv))) return rc;
  if (ta && (rc = retime_torque_check(h, nm, ta->tau_max, ta->pl_mass, ta->pl_com, ta->pl_inertia, tq.lim))) return rc;
  if (ta && ta->pl_mass)
    for (int32_t b = 0; b < B; ++b)
      if (!(ta->pl_mass[b] >= 0) || !std::isfinite(ta->pl_mass[b]))
        return fail(h, GTO_ERR_INVALID_ARG, std::string(nm.fn) + ": payload mass must be >= 0 and finite");
  if (B == 0) return GTO_OK;
  if (!paths) return fail(h, GTO_ERR_INVALID_ARG, std::string(nm.fn) + ": null " + nm.array);
  if (n_cols)
    for (int32_t b = 0; b < B; ++b)
      if (n_cols[b] < 1 || n_cols[b] > Tp)
        return fail(h, GTO_ERR_INVALID_ARG, std::string(nm.fn) + ": n_cols must lie in [1, Tp]");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nB = (size_t)B, nd = d.ndof, T = d.Tp, N = d.Nmax, nM = (size_t)M;
  Staging io(h);
  const double* d_paths;
  const int32_t* d_nc;
  double *d_dur, *d_t, *d_sd, *d_q, *d_qd, *d_qdd;
  int32_t *d_st, *d_it;
  if ((rc = io.in(paths, nB * nd * T, &d_paths))) return rc;
  if ((rc = io.in(n_cols, nB, &d_nc))) return rc;
  if ((rc = io.out(duration_out, nB, &d_dur))) return rc;
  if ((rc = io.out(t_grid_out, nB * N, &d_t))) return rc;
  if ((rc = io.out(sd_grid_out, nB * N, &d_sd))) return rc;
  if ((rc = io.out(q_out, nB * nM * nd, &d_q))) return rc;
  if ((rc = io.out(qd_out, nB * nM * nd, &d_qd))) return rc;
  if ((rc = io.out(qdd_out, nB * nM * nd, &d_qdd))) return rc;
  if ((rc = io.out(status_out, nB, &d_st))) return rc;
  if ((rc = io.out(iters_out, nB, &d_it))) return rc;
  if (ta) {
    if ((rc = io.in(ta->pl_mass, nB, &tq.pl_mass))) return rc;  // (a null array: a null device pointer)
    if ((rc = io.in(ta->pl_com, nB * 3, &tq.pl_com))) return rc;
    if ((rc = io.in(ta->pl_inertia, nB * 6, &tq.pl_inertia))) return rc;
    if ((rc = io.out(ta->tau_out, nB * nM * nd, &tq.tau_out))) return rc;
  }
  if ((rc = retime_launch(h, d, lim, d_paths, d_nc, d_dur, d_t, d_sd, d_q, d_qd, d_qdd, d_st, nullptr, cv, d_it, ta ? &tq : nullptr)))
    return rc;
  return io.finish();
}

int gto_retime_paths_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols,
                            const double* vmax, const double* amax, int32_t subdiv, int32_t M, double* duration_out,
                            double* t_grid_out, double* sd_grid_out, double* q_out, double* qd_out, double* qdd_out,
                            int32_t* status_out, void* stream) {
  return retime_device(h, RETIME_PATHS, B, Tp, paths, n_cols, vmax, amax, subdiv, M, duration_out, t_grid_out,
                       sd_grid_out, q_out, qd_out, qdd_out, status_out, stream);
}

int gto_retime_paths(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols, const double* vmax,
                     const double* amax, int32_t subdiv, int32_t M, double* duration_out, double* t_grid_out,
                     double* sd_grid_out, double* q_out, double* qd_out, double* qdd_out, int32_t* status_out) {
  return retime_host(h, RETIME_PATHS, B, Tp, paths, n_cols, vmax, amax, subdiv, M, duration_out, t_grid_out,
                     sd_grid_out, q_out, qd_out, qdd_out, status_out);
}

// the grid's time optimum in place of the greedy profile (k_retime_convex in place of k_retime_pass)
int gto_retime_paths_convex_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols,
                                   const double* vmax, const double* amax, int32_t subdiv, int32_t M, double gap_tol,
                                   int32_t max_newton, double* duration_out, double* t_grid_out, double* sd_grid_out,
                                   double* q_out, double* qd_out, double* qdd_out, int32_t* status_out, int32_t* iters_out,
                                   void* stream) {
  const RetimeConvex cv = {gap_tol, max_newton};
  return retime_device(h, RETIME_CONVEX, B, Tp, paths, n_cols, vmax, amax, subdiv, M, duration_out, t_grid_out,
                       sd_grid_out, q_out, qd_out, qdd_out, status_out, stream, &cv, iters_out);
}

int gto_retime_paths_convex(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols,
                            const double* vmax, const double* amax, int32_t subdiv, int32_t M, double gap_tol,
                            int32_t max_newton, double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out,
                            double* qd_out, double* qdd_out, int32_t* status_out, int32_t* iters_out) {
  const RetimeConvex cv = {gap_tol, max_newton};
  return retime_host(h, RETIME_CONVEX, B, Tp, paths, n_cols, vmax, amax, subdiv, M, duration_out, t_grid_out,
                     sd_grid_out, q_out, qd_out, qdd_out, status_out, &cv, iters_out);
}

// joint torque limits and the held object on top of the convex program (k_retime_torque_rows, k_retime_convex_torque)
int gto_retime_paths_torque_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols,
                                   const double* vmax, const double* amax, const double* tau_max, const double* payload_mass,
                                   const double* payload_com, const double* payload_inertia, int32_t subdiv, int32_t M,
                                   double gap_tol, int32_t max_newton, double* duration_out, double* t_grid_out,
                                   double* sd_grid_out, double* q_out, double* qd_out, double* qdd_out, double* tau_out,
                                   int32_t* status_out, int32_t* iters_out, void* stream) {
  const RetimeConvex cv = {gap_tol, max_newton};
  const RetimeTorqueArgs ta = {tau_max, payload_mass, payload_com, payload_inertia, tau_out};
  return retime_device(h, RETIME_TORQUE, B, Tp, paths, n_cols, vmax, amax, subdiv, M, duration_out, t_grid_out,
                       sd_grid_out, q_out, qd_out, qdd_out, status_out, stream, &cv, iters_out, &ta);
}

int gto_retime_paths_torque(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols,
                            const double* vmax, const double* amax, const double* tau_max, const double* payload_mass,
                            const double* payload_com, const double* payload_inertia, int32_t subdiv, int32_t M,
                            double gap_tol, int32_t max_newton, double* duration_out, double* t_grid_out, double* sd_grid_out,
                            double* q_out, double* qd_out, double* qdd_out, double* tau_out, int32_t* status_out,
                            int32_t* iters_out) {
  const RetimeConvex cv = {gap_tol, max_newton};
  const RetimeTorqueArgs ta = {tau_max, payload_mass, payload_com, payload_inertia, tau_out};
  return retime_host(h, RETIME_TORQUE, B, Tp, paths, n_cols, vmax, amax, subdiv, M, duration_out, t_grid_out,
                     sd_grid_out, q_out, qd_out, qdd_out, status_out, &cv, iters_out, &ta);
}

// plans of the handle's horizon: gto_retime_paths with Tp = T and every column used
int gto_retime_batch_device(gto_handle* h, int32_t B, const double* plans, const double* vmax, const double* amax,
                            int32_t subdiv, int32_t M, double* duration_out, double* t_grid_out, double* sd_grid_out,
                            double* q_out, double* qd_out, double* qdd_out, int32_t* status_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  return retime_device(h, RETIME_BATCH, B, h->opts.T, plans, nullptr, vmax, amax, subdiv, M, duration_out,
                       t_grid_out, sd_grid_out, q_out, qd_out, qdd_out, status_out, stream);
}

int gto_retime_batch(gto_handle* h, int32_t B, const double* plans, const double* vmax, const double* amax, int32_t subdiv,
                     int32_t M, double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out, double* qd_out,
                     double* qdd_out, int32_t* status_out) {
  if (!h) return GTO_ERR_INVALID_ARG;
  return retime_host(h, RETIME_BATCH, B, h->opts.T, plans, nullptr, vmax, amax, subdiv, M, duration_out,
                     t_grid_out, sd_grid_out, q_out, qd_out, qdd_out, status_out);
}

}  // extern "C"

// ------------------------------------------------------------------ a resident observation and the collision checks (gto_observe.h)
struct gto_observation {
  int device = 0;
  bool is_depth = true;
  std::vector<DevBuf> owned;  // its device buffers
  // depth: image, camera, world points, tile hierarchy (P = 0: none, exhaustive search)
  DepthCloud depth = {};
  DepthCamera cam = {};
  // cloud: samples, normals, the samples in key order under their hierarchy (n_leaves = 0: none), the vote's k
  SampleCloud cloud = {};
  int k = 0;
};

namespace {
void obs_adopt(gto_observation* o, DepthLease& c, std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (DevBuf b = c.keep(p)) o->owned.push_back(std::move(b));
}
ObsDepthView depth_view(const gto_observation* o) { return {o->depth.depth, o->depth.H, o->depth.W, o->cam.K, o->cam.inv}; }

// the vote of the observation's k nearest samples for nq queries in the caller's order (neighbours as they come), on `st`
void obs_cloud_votes(const SearchEnv& env, hipStream_t st, const gto_observation* o, const double* d_q, long nq, uint8_t* d_flags) {
  search_samples(env, st, o->cloud, o->k, {d_q, nq, nullptr}, 0.0f, 0.0f, {nullptr, d_flags, nullptr, nullptr});
}
// queries of a cloud observation per launch chain of a check: bounds the workspace (25 bytes per query)
constexpr long long kCheckChunkQueries = 1ll << 24;
// how many of n items (grasps, plans) of per_item >= 1 queries each go into one launch chain: at least one.  An item count
// can exceed an int (the grasp filter's run of poses): all item arithmetic is long long.
long long chunk_items(long long n, long long per_item) { return std::min(n, std::max(1ll, kCheckChunkQueries / per_item)); }
long long cloud_chunk(long long n_items, int rows_per_item, int P) { return chunk_items(n_items, (long long)rows_per_item * std::max(1, P)); }
// The counts of n_items items of rows_per_item rows of P points each against a cloud observation, on `st`, one launch chain
// per chunk: place(i0, m, d_xyz, count + i0 * rows_per_item) launches the caller's kernel for items [i0, i0 + m), which
// writes their world points [m][rows_per_item][P][3] and marks the rows that report -1; then the votes of the samples'
// normals and their sum per row.  d_xyz / d_flags: room for one chunk (cloud_chunk).
template <class Place>
void cloud_counts(const SearchEnv& env, hipStream_t st, const gto_observation* o, long long n_items, int rows_per_item, int P, double* d_xyz,
                  uint8_t* d_flags, int32_t* count, Place place) {
  const long long chunk = cloud_chunk(n_items, rows_per_item, P);
  for (long long i0 = 0; i0 < n_items; i0 += chunk) {
    const long long m = std::min(chunk, n_items - i0);
    int32_t* cnt = count + (size_t)i0 * rows_per_item;
    place(i0, m, d_xyz, cnt);
    if (P) obs_cloud_votes(env, st, o, d_xyz, (long)(m * rows_per_item * P), d_flags);
    hipLaunchKernelGGL(k_count_flags, dim3((unsigned)(m * rows_per_item)), dim3(256), 0, st, d_flags, P, cnt);
  }
}
// the handle's workspace for one chunk of cloud_counts (ck_xyz, ck_flags: see the header on streams)
int cloud_workspace(gto_handle* h, long long n_items, int rows_per_item, int P, double** d_xyz, uint8_t** d_flags) {
  const size_t q = (size_t)cloud_chunk(n_items, rows_per_item, P) * rows_per_item * P;
  int rc;
  if ((rc = ensure(h, h->ck_xyz, q * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->ck_flags, q))) return rc;
  *d_xyz = h->ck_xyz.as<double>(), *d_flags = h->ck_flags.as<uint8_t>();
  return GTO_OK;
}
// What gto_check_plans and its device variant check before any device work.  *empty: nothing to do (B = 0).
int check_plans_args(gto_handle* h, const gto_observation* o, int32_t B, const double* plans, const double* base_pos, bool* empty) {
  *empty = B == 0;
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!o || B < 0 || !base_pos) return fail(h, GTO_ERR_INVALID_ARG, "gto_check_plans: null observation or base position");
  if (o->device != h->device) return fail(h, GTO_ERR_INVALID_ARG, "gto_check_plans: the observation lives on another device than the handle");
  if (B > 0 && !plans) return fail(h, GTO_ERR_INVALID_ARG, "gto_check_plans: null plans");
  return GTO_OK;
}
// waypoints per workgroup of k_check_plans: GTO_CHECK_TG in the environment (1 .. 4, read by every call; default 4, the
// measured choice: DESIGN.md 7g).  Results do not depend on it.
int check_waypoints_per_group() {
  const char* e = getenv("GTO_CHECK_TG");
  const int v = e ? atoi(e) : GTO_CHECK_TG;
  return v >= 1 && v <= GTO_CHECK_TG ? v : GTO_CHECK_TG;
}
int check_lds_fits(gto_handle* h, size_t lds) {
  return lds > 150 * 1024 ? fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the collision-check kernel's LDS") : GTO_OK;
}
// the launch shape of the path checks (k_check_plans, k_check_held) over T columns: grid (plans, tgroups), lds bytes
struct CheckShape {
  size_t lds;
  int tg;
  unsigned tgroups;
};
int check_shape(gto_handle* h, int T, CheckShape* s) {
  s->lds = sizeof(double) * check_plans_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  s->tg = check_waypoints_per_group();
  s->tgroups = (unsigned)((T + s->tg - 1) / s->tg);
  return check_lds_fits(h, s->lds);
}
// the base of the path checks' plans: (b0, b1, b2) for every plan, or d_base [B][3] on the device
struct CheckBase {
  double b0, b1, b2;
  const double* d_base;
};
int stage_check_base(gto_handle* h, const double* base_pos, int32_t per_plan_base, int32_t B, hipStream_t st, CheckBase* out) {
  *out = {per_plan_base ? 0.0 : base_pos[0], per_plan_base ? 0.0 : base_pos[1], per_plan_base ? 0.0 : base_pos[2], nullptr};
  if (!per_plan_base) return GTO_OK;
  // Through a pinned slot of the handle (pinned_to_device), as n_goals travels: the caller's array is free on return whatever
  // memory it lives in, and the copy is ordered on `st` in front of the kernel.  A hipMemcpyAsync straight from the caller's
  // array was only safe for pageable memory, which the runtime stages before it returns; a page-locked array it reads when
  // the copy RUNS, after the caller has it back (tests/test_gpu_stream_order.py).  ck_base is one buffer per handle: see the
  // header on streams.
  if (int rc = pinned_to_device(h, h->ck_base, base_pos, (size_t)B * 3 * sizeof(double), st)) return rc;
  out->d_base = h->ck_base.as<const double>();
  return GTO_OK;
}
}  // namespace

extern "C" {

int gto_observation_from_depth(int device, const float* depth, int32_t H, int32_t W, const double* K, const double* Kinv,
                               const double* cam_pose, const double* cam_inv, const uint8_t* target_mask, double threshold,
                               gto_observation** out) {
  if (out) *out = nullptr;
  if (!out || !depth || !K || !Kinv || !cam_pose || !cam_inv || H < 1 || W < 1)
    return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_observation_from_depth: null or empty input");
  int cur_dev;
  DEPTH_TRY(select_device(device, &cur_dev));
  std::unique_ptr<gto_observation> o(new gto_observation);
  o->device = cur_dev, o->is_depth = true;
  DepthLease c(nullptr, "gto_observation_from_depth", cur_dev);
  const bool tree = tile_levels(H, W) <= GTO_BVH_MAX_P;  // beyond: the exhaustive search, as gto_depth_sdf_cost
  uint8_t* d_valid;
  DEPTH_TRY(upload_depth_cloud(c, depth, H, W, K, Kinv, cam_pose, cam_inv, target_mask, threshold, tree, &o->cam, &d_valid, &o->depth));
  DEPTH_TRY(c.sync());
  obs_adopt(o.get(), c, {o->depth.depth, o->cam.K, o->depth.px, o->depth.boxes});
  *out = o.release();
  return GTO_OK;
}

int gto_observation_from_cloud(int device, const double* points, const double* normals, int64_t n, int32_t k,
                               gto_observation** out) {
  if (out) *out = nullptr;
  if (!out) return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_observation_from_cloud: null output");
  double box[6];
  if (int rc = check_cloud(nullptr, "gto_observation_from_cloud", points, normals, n, k, box)) return rc;
  int cur_dev;
  DEPTH_TRY(select_device(device, &cur_dev));
  std::unique_ptr<gto_observation> o(new gto_observation);
  o->device = cur_dev, o->is_depth = false, o->k = k;
  DepthLease c(nullptr, "gto_observation_from_cloud", cur_dev);
  const double *d_points, *d_normals;
  DEPTH_TRY(c.upload(points, (size_t)n * 3, &d_points));
  DEPTH_TRY(c.upload(normals, (size_t)n * 3, &d_normals));
  DEPTH_TRY(make_sample_cloud(c, d_points, d_normals, n, box, &o->cloud));
  DEPTH_TRY(c.sync());
  obs_adopt(o.get(), c, {d_points, d_normals, o->cloud.px, o->cloud.pid, o->cloud.boxes});
  *out = o.release();
  return GTO_OK;
}

void gto_observation_destroy(gto_observation* o) {
  if (!o) return;
  int cur = -1;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(o->device);
  (void)hipDeviceSynchronize();  // nothing may still be reading it
  delete o;  // frees its buffers
  if (cur >= 0) (void)hipSetDevice(cur);  // the caller's current device is the caller's
}

int gto_observation_sdf(gto_observation* o, const double* query, int64_t nq, float* sdf_out, uint8_t* inside_out) {
  if (!o || nq < 0 || (nq > 0 && !query)) return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_observation_sdf: null observation or query");
  if (nq == 0) return GTO_OK;
  if (hipSetDevice(o->device) != hipSuccess) return fail(nullptr, GTO_ERR_NO_DEVICE, "hipSetDevice failed");
  DepthLease c(nullptr, "gto_observation_sdf", o->device);
  DepthQueries qs = {nullptr, (long)nq, nullptr};
  DEPTH_TRY(c.upload(query, (size_t)nq * 3, &qs.q));
  float* d_sdf = c.alloc<float>((size_t)nq);
  uint8_t* d_in = c.alloc<uint8_t>((size_t)nq);
  if (!d_sdf || !d_in) return c.no_memory();
  if (o->is_depth) {
    if (use_tree(o->depth, c.env)) DEPTH_TRY(sort_queries(c, o->depth.boxes, &qs));
    search_depth(c.env, 0, o->depth, o->cam, qs, 0.0f, 0.0f, {d_sdf, d_in, nullptr}, nullptr, false);
  } else {
    if (use_tree(o->cloud, c.env)) DEPTH_TRY(sort_queries(c, o->cloud.boxes, &qs));
    search_samples(c.env, 0, o->cloud, o->k, qs, 0.0f, 0.0f, {d_sdf, d_in, nullptr, nullptr});
  }
  DEPTH_TRY(c.sync());
  DEPTH_TRY(c.download(sdf_out, d_sdf, (size_t)nq));
  DEPTH_TRY(c.download(inside_out, d_in, (size_t)nq));
  return GTO_OK;
}

int gto_observation_check_posed(gto_observation* o, const double* points, int32_t P, const double* poses, int32_t n,
                                int32_t* count_out) {
  if (!o || P < 0 || n < 0 || (P > 0 && !points) || (n > 0 && !poses))
    return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_observation_check_posed: null observation, points or poses");
  if (n == 0) return GTO_OK;
  if (hipSetDevice(o->device) != hipSuccess) return fail(nullptr, GTO_ERR_NO_DEVICE, "hipSetDevice failed");
  DepthLease c(nullptr, "gto_observation_check_posed", o->device);
  const double *d_points, *d_poses;
  DEPTH_TRY(c.upload(points, (size_t)P * 3, &d_points));
  DEPTH_TRY(c.upload(poses, (size_t)n * 16, &d_poses));
  int32_t* d_count = c.alloc<int32_t>((size_t)n);
  if (!d_count) return c.no_memory();
  if (o->is_depth) {
    hipLaunchKernelGGL(k_check_posed<true>, dim3((unsigned)n), dim3(256), 0, 0, d_points, (int)P, d_poses, depth_view(o), (double*)nullptr, d_count);
  } else {
    const size_t chunk = (size_t)cloud_chunk(n, 1, P);
    double* d_xyz = c.alloc<double>(chunk * P * 3);
    uint8_t* d_flags = c.alloc<uint8_t>(chunk * P);
    if (!d_xyz || !d_flags) return c.no_memory();
    cloud_counts(c.env, 0, o, n, 1, P, d_xyz, d_flags, d_count, [&](long long i0, long long m, double* xyz, int32_t* cnt) {
      hipLaunchKernelGGL(k_check_posed<false>, dim3((unsigned)m), dim3(256), 0, 0, d_points, (int)P, d_poses + (size_t)i0 * 16, ObsDepthView{}, xyz, cnt);
    });
  }
  DEPTH_TRY(c.sync());
  DEPTH_TRY(c.download(count_out, d_count, (size_t)n));
  return GTO_OK;
}

int gto_check_paths_device(gto_handle* h, gto_observation* o, int32_t B, int32_t Tp, const double* plans, const double* base_pos,
                           int32_t per_plan_base, int32_t* count_out, void* stream) {
  bool empty;
  if (int rc = check_plans_args(h, o, B, plans, base_pos, &empty)) return rc;
  if (Tp < 1) return fail(h, GTO_ERR_INVALID_ARG, "gto_check_paths: Tp must be >= 1");
  if (empty) return GTO_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int T = Tp, P = h->rb.n_points, ndof = h->rb.ndof;
  CheckShape sh;
  CheckBase base;
  int rc;
  if ((rc = check_shape(h, T, &sh))) return rc;
  if ((rc = stage_check_base(h, base_pos, per_plan_base, B, st, &base))) return rc;
  if (o->is_depth) {
    HIPCHK(h, raise_dynamic_lds((const void*)k_check_plans<true>, sh.lds));
    if (count_out)
      hipLaunchKernelGGL(k_check_plans<true>, dim3((unsigned)B, sh.tgroups), dim3(256), sh.lds, st, h->d_rb, h->d_px, h->d_py, h->d_pz, h->d_plink, T,
                         sh.tg, plans, base.b0, base.b1, base.b2, base.d_base, depth_view(o), (double*)nullptr, count_out);
  } else if (count_out) {
    HIPCHK(h, raise_dynamic_lds((const void*)k_check_plans<false>, sh.lds));
    double* d_xyz;
    uint8_t* d_flags;
    if ((rc = cloud_workspace(h, B, T, P, &d_xyz, &d_flags))) return rc;
    cloud_counts(search_env(), st, o, B, T, P, d_xyz, d_flags, count_out, [&](long long i0, long long m, double* xyz, int32_t* cnt) {
      hipLaunchKernelGGL(k_check_plans<false>, dim3((unsigned)m, sh.tgroups), dim3(256), sh.lds, st, h->d_rb, h->d_px, h->d_py, h->d_pz, h->d_plink, T,
                         sh.tg, plans + (size_t)i0 * ndof * T, base.b0, base.b1, base.b2, base.d_base ? base.d_base + (size_t)i0 * 3 : nullptr,
                         ObsDepthView{}, xyz, cnt);
    });
  }
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

// The grasp collision filter on the stream (include/gto_solver.h; kernels: gto_observe.h).  The observations are host facts of
// the call: which of them are depth images decides the launches.
int gto_filter_grasps_device(gto_handle* h, int32_t B, int32_t n_max, gto_observation* const* obs, const double* points, int32_t P,
                             const double* object_pose, const double* grasps, const int32_t* n_grasps, const double* world_to_base,
                             const double* base_pos, const double* check_offset, const double* ik_offset, double max_ratio,
                             int32_t* count_out, uint8_t* keep_out, int32_t* kept_rows_out, int32_t* n_kept_out,
                             int32_t* n_grasps_out, double* plan_goals_out, double* ik_goals_out, void* stream) {
  const char* who = "gto_filter_grasps_device";
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0 || n_max < 1 || P < 1 || !(max_ratio >= 0.0) || !std::isfinite(max_ratio))
    return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": B >= 0, n_max >= 1, P >= 1 and a finite max_ratio >= 0 are required");
  if (B == 0) return GTO_OK;
  if (B > 65535 || n_max > 65535) return fail(h, GTO_ERR_UNSUPPORTED, std::string(who) + ": at most 65535 objects of at most 65535 grasps in one call");
  if (!obs || !points || !object_pose || !grasps || !n_grasps || !check_offset) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": null input array");
  for (int b = 0; b < B; ++b) {
    if (!obs[b]) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": null observation");
    if (obs[b]->device != h->device) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": an observation lives on another device than the handle");
  }
  PoseArg coff, ioff = {};
  for (int e = 0; e < 16; ++e) {
    coff.m[e] = check_offset[e];
    if (ik_offset) ioff.m[e] = ik_offset[e];
    if (!std::isfinite(coff.m[e]) || !std::isfinite(ioff.m[e])) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": non-finite entry in check_offset or ik_offset");
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const size_t rows = (size_t)B * n_max;
  int rc;
  if ((rc = ensure(h, h->fg_plan, rows * 16 * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->fg_ik, rows * 16 * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->fg_count, rows * sizeof(int32_t)))) return rc;
  double *ws_plan = h->fg_plan.as<double>(), *ws_ik = h->fg_ik.as<double>();
  int32_t* ws_count = h->fg_count.as<int32_t>();
  const int has_ik = ik_offset != nullptr;
  // the depth objects: one launch over all of them, each against its own image
  std::vector<FilterDepthItem> items;
  for (int b = 0; b < B; ++b)
    if (obs[b]->is_depth) items.push_back({depth_view(obs[b]), b});
  if (!items.empty()) {
    if ((rc = pinned_to_device(h, h->fg_tab, items.data(), items.size() * sizeof(FilterDepthItem), st))) return rc;
    hipLaunchKernelGGL(k_filter_depth, dim3((unsigned)n_max, (unsigned)items.size()), dim3(256), 0, st, h->fg_tab.as<const FilterDepthItem>(),
                       points, (int)P, (int)n_max, object_pose, grasps, n_grasps, world_to_base, base_pos, coff, ioff, has_ik, ws_plan, ws_ik,
                       ws_count);
  }
  // the cloud objects: every run of consecutive objects that name one observation is one cloud_counts over the run's poses
  if (items.size() < (size_t)B) {
    if ((rc = ensure(h, h->fg_pose, rows * 16 * sizeof(double)))) return rc;
    double* ws_pose = h->fg_pose.as<double>();
    const SearchEnv env = search_env();
    for (int b0 = 0; b0 < B;) {
      int b1 = b0 + 1;
      if (obs[b0]->is_depth) {
        b0 = b1;
        continue;
      }
      while (b1 < B && obs[b1] == obs[b0]) ++b1;
      const long long n = (long long)(b1 - b0) * n_max;  // the run's poses: at most 65535 * 65535
      hipLaunchKernelGGL(k_filter_pose, dim3((unsigned)((n_max + 63) / 64), (unsigned)(b1 - b0)), dim3(64), 0, st, b0, (int)n_max, object_pose, grasps,
                         n_grasps, world_to_base, base_pos, coff, ioff, has_ik, ws_plan, ws_ik, ws_pose);
      double* d_xyz;
      uint8_t* d_flags;
      if ((rc = cloud_workspace(h, n, 1, P, &d_xyz, &d_flags))) return rc;
      const size_t at = (size_t)b0 * n_max;
      cloud_counts(env, st, obs[b0], n, 1, P, d_xyz, d_flags, ws_count + at, [&](long long i0, long long m, double* xyz, int32_t* cnt) {
        hipLaunchKernelGGL(k_check_posed<false>, dim3((unsigned)m), dim3(256), 0, st, points, (int)P, ws_pose + (at + (size_t)i0) * 16, ObsDepthView{},
                           xyz, cnt);
      });
      b0 = b1;
    }
  }
  hipLaunchKernelGGL(k_filter_compact, dim3((unsigned)B), dim3(64), 0, st, (int)n_max, (int)P, max_ratio, n_grasps, (const int32_t*)ws_count,
                     (const double*)ws_plan, (const double*)ws_ik, count_out, keep_out, kept_rows_out, n_kept_out, n_grasps_out, plan_goals_out,
                     ik_goals_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_check_plans_device(gto_handle* h, gto_observation* o, int32_t B, const double* plans, const double* base_pos,
                           int32_t per_plan_base, int32_t* count_out, void* stream) {
  bool empty;
  if (int rc = check_plans_args(h, o, B, plans, base_pos, &empty)) return rc;  // (before the handle's horizon is read)
  return gto_check_paths_device(h, o, B, h->opts.T, plans, base_pos, per_plan_base, count_out, stream);
}

int gto_check_paths(gto_handle* h, gto_observation* o, int32_t B, int32_t Tp, const double* plans, const double* base_pos,
                    int32_t per_plan_base, int32_t* count_out) {
  bool empty;
  if (int rc = check_plans_args(h, o, B, plans, base_pos, &empty)) return rc;
  if (Tp < 1) return fail(h, GTO_ERR_INVALID_ARG, "gto_check_paths: Tp must be >= 1");
  if (empty) return GTO_OK;
  HIPCHK(h, hipSetDevice(h->device));
  Staging io(h);
  const double* d_plans;
  int32_t* d_count;
  int rc;
  if ((rc = io.in(plans, (size_t)B * h->rb.ndof * Tp, &d_plans))) return rc;
  if ((rc = io.out(count_out, (size_t)B * Tp, &d_count))) return rc;
  if ((rc = gto_check_paths_device(h, o, B, Tp, d_plans, base_pos, per_plan_base, d_count, nullptr))) return rc;
  return io.finish();
}

int gto_check_plans(gto_handle* h, gto_observation* o, int32_t B, const double* plans, const double* base_pos,
                    int32_t per_plan_base, int32_t* count_out) {
  bool empty;
  if (int rc = check_plans_args(h, o, B, plans, base_pos, &empty)) return rc;
  return gto_check_paths(h, o, B, h->opts.T, plans, base_pos, per_plan_base, count_out);
}

// ---- the robot's clearance from itself (include/gto_solver.h; kernel: gto_selfcheck.h) ----
int gto_set_self_pairs(gto_handle* h, const int32_t* rows) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!rows) {
    gto_selfpairs::all_distinct_pairs(h->rb.n_links, h->self_pairs.rows);
    return GTO_OK;
  }
  std::string why;
  if (int rc = gto_selfpairs::check_self_pairs(h->rb.n_links, rows, why)) return fail(h, rc, why);
  for (int a = 0; a < GTO_MAX_LINKS; ++a) h->self_pairs.rows[a] = a < h->rb.n_links ? (uint32_t)rows[a] : 0u;
  return GTO_OK;
}

int gto_self_clearance_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, double cutoff, double* d2_out,
                              int32_t* pair_out, void* stream) {
  std::string why;
  if (int rc = gto_selfpairs::check_self_clearance_args(B, Tp, cutoff, why)) return fail(h, rc, why);
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B == 0) return GTO_OK;
  if (!paths || !d2_out || !pair_out) return fail(h, GTO_ERR_INVALID_ARG, "gto_self_clearance: null paths, d2_out or pair_out");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const size_t lds = sizeof(double) * self_clearance_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt, h->rb.n_chunks);
  if (int rc = check_lds_fits(h, lds)) return rc;
  const int tg = check_waypoints_per_group();
  HIPCHK(h, raise_dynamic_lds((const void*)k_self_clearance, lds));
  hipLaunchKernelGGL(k_self_clearance, dim3((unsigned)B, (unsigned)((Tp + tg - 1) / tg)), dim3(256), lds, st, h->d_rb, h->d_px, h->d_py, h->d_pz,
                     h->d_chunks, (int)Tp, tg, paths, h->self_pairs, cutoff, d2_out, pair_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_self_clearance(gto_handle* h, int32_t B, int32_t Tp, const double* paths, double cutoff, double* d2_out,
                       int32_t* pair_out) {
  std::string why;
  if (int rc = gto_selfpairs::check_self_clearance_args(B, Tp, cutoff, why)) return fail(h, rc, why);
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B == 0) return GTO_OK;
  if (!paths || !d2_out || !pair_out) return fail(h, GTO_ERR_INVALID_ARG, "gto_self_clearance: null paths, d2_out or pair_out");
  HIPCHK(h, hipSetDevice(h->device));
  Staging io(h);
  const double* d_paths;
  double* d_d2;
  int32_t* d_pair;
  int rc;
  if ((rc = io.in(paths, (size_t)B * h->rb.ndof * Tp, &d_paths))) return rc;
  if ((rc = io.out(d2_out, (size_t)B * Tp, &d_d2))) return rc;
  if ((rc = io.out(pair_out, (size_t)B * Tp * 2, &d_pair))) return rc;
  if ((rc = gto_self_clearance_device(h, B, Tp, d_paths, cutoff, d_d2, d_pair, nullptr))) return rc;
  return io.finish();
}

// What gto_check_held_paths and its device variant check before any device work (host-side facts only).  *empty: B = 0.
static int check_held_args(gto_handle* h, const gto_observation* o, int32_t B, int32_t Tp, const double* paths, const double* attach,
                           int32_t attach_ld, int32_t attach_col, const double* held_points, int32_t P_max, const int32_t* n_held,
                           const int32_t* labels, const int32_t* held_label, const double* base_pos, const int32_t* count_out,
                           bool* empty) {
  const char* who = "gto_check_held_paths";
  *empty = B == 0;
  if (!h) return GTO_ERR_INVALID_ARG;
  if (!o || !base_pos) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": null observation or base position");
  if (B < 0 || Tp < 1 || P_max < 1) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": B >= 0, Tp >= 1 and P_max >= 1 are required");
  if (o->device != h->device) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": the observation lives on another device than the handle");
  if (attach && (attach_col < 0 || attach_col >= attach_ld))
    return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": attach_col must be in [0, attach_ld)");
  if (labels && !held_label) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": labels without held_label");
  if (B == 0) return GTO_OK;
  if (B > 65535 || P_max > 65535) return fail(h, GTO_ERR_UNSUPPORTED, std::string(who) + ": at most 65535 plans of at most 65535 held points in one call");
  if (!paths || !held_points || !n_held || !count_out) return fail(h, GTO_ERR_INVALID_ARG, std::string(who) + ": null paths, held_points, n_held or count_out");
  return GTO_OK;
}

// The held object's points along the paths (include/gto_solver.h; kernels: gto_held.h)
int gto_check_held_paths_device(gto_handle* h, gto_observation* o, int32_t B, int32_t Tp, const double* paths, const double* attach,
                                int32_t attach_ld, int32_t attach_col, const double* held_points, int32_t P_max,
                                const int32_t* n_held, const double* object_pose, const int32_t* labels, const int32_t* held_label,
                                const double* base_pos, int32_t per_plan_base, int32_t* count_out, void* stream) {
  bool empty;
  if (int rc = check_held_args(h, o, B, Tp, paths, attach, attach_ld, attach_col, held_points, P_max, n_held, labels, held_label, base_pos,
                               count_out, &empty))
    return rc;
  if (empty) return GTO_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int T = Tp, P = P_max, ndof = h->rb.ndof;
  const size_t lds_att = sizeof(double) * held_attach_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  CheckShape sh;
  CheckBase base;
  int rc;
  if ((rc = check_shape(h, T, &sh)) || (rc = check_lds_fits(h, lds_att))) return rc;
  if ((rc = stage_check_base(h, base_pos, per_plan_base, B, st, &base))) return rc;
  if ((rc = ensure(h, h->hd_p, (size_t)B * P * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->hd_bad, (size_t)B * sizeof(int32_t)))) return rc;
  double* d_p = h->hd_p.as<double>();
  int32_t* d_bad = h->hd_bad.as<int32_t>();
  // attach NULL: the paths' own column 0 (the lift, whose column 0 is the plan's last waypoint)
  const double* att = attach ? attach : paths;
  const int att_ld = attach ? attach_ld : T, att_col = attach ? attach_col : 0;
  HIPCHK(h, raise_dynamic_lds((const void*)k_held_attach, lds_att));
  hipLaunchKernelGGL(k_held_attach, dim3((unsigned)B), dim3(256), lds_att, st, h->d_rb, att, att_ld, att_col, base.b0, base.b1, base.b2, base.d_base,
                     held_points, P, n_held, object_pose, d_p, d_bad);
  if (o->is_depth) {
    HIPCHK(h, raise_dynamic_lds((const void*)k_check_held<true>, sh.lds));
    hipLaunchKernelGGL(k_check_held<true>, dim3((unsigned)B, sh.tgroups), dim3(256), sh.lds, st, h->d_rb, T, sh.tg, paths, base.b0, base.b1, base.b2,
                       base.d_base, (const double*)d_p, P, n_held, (const int32_t*)d_bad, depth_view(o), labels, held_label, (double*)nullptr,
                       count_out);
  } else {
    HIPCHK(h, raise_dynamic_lds((const void*)k_check_held<false>, sh.lds));
    double* d_xyz;
    uint8_t* d_flags;
    if ((rc = cloud_workspace(h, B, T, P, &d_xyz, &d_flags))) return rc;
    cloud_counts(search_env(), st, o, B, T, P, d_xyz, d_flags, count_out, [&](long long i0, long long m, double* xyz, int32_t* cnt) {
      hipLaunchKernelGGL(k_check_held<false>, dim3((unsigned)m, sh.tgroups), dim3(256), sh.lds, st, h->d_rb, T, sh.tg, paths + (size_t)i0 * ndof * T,
                         base.b0, base.b1, base.b2, base.d_base ? base.d_base + (size_t)i0 * 3 : nullptr, (const double*)d_p + (size_t)i0 * P * 3, P,
                         n_held + i0, (const int32_t*)d_bad + i0, ObsDepthView{}, (const int32_t*)nullptr, (const int32_t*)nullptr, xyz, cnt);
    });
  }
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_check_held_paths(gto_handle* h, gto_observation* o, int32_t B, int32_t Tp, const double* paths, const double* attach,
                         int32_t attach_ld, int32_t attach_col, const double* held_points, int32_t P_max, const int32_t* n_held,
                         const double* object_pose, const int32_t* labels, const int32_t* held_label, const double* base_pos,
                         int32_t per_plan_base, int32_t* count_out) {
  bool empty;
  if (int rc = check_held_args(h, o, B, Tp, paths, attach, attach_ld, attach_col, held_points, P_max, n_held, labels, held_label, base_pos,
                               count_out, &empty))
    return rc;
  if (empty) return GTO_OK;
  for (int b = 0; b < B; ++b)
    if (n_held[b] < 0 || n_held[b] > P_max) return fail(h, GTO_ERR_INVALID_ARG, "gto_check_held_paths: n_held must be in [0, P_max]");
  HIPCHK(h, hipSetDevice(h->device));
  Staging io(h);
  const size_t nB = (size_t)B, nd = (size_t)h->rb.ndof;
  const bool use_labels = labels && o->is_depth;  // (a cloud observation has no image: both are ignored)
  const double *d_paths, *d_attach, *d_points, *d_pose;
  const int32_t *d_nheld, *d_labels, *d_lab;
  int32_t* d_count;
  int rc;
  if ((rc = io.in(paths, nB * nd * Tp, &d_paths))) return rc;
  if ((rc = io.in(attach, attach ? nB * nd * attach_ld : 0, &d_attach))) return rc;
  if ((rc = io.in(held_points, nB * P_max * 3, &d_points))) return rc;
  if ((rc = io.in(n_held, nB, &d_nheld))) return rc;
  if ((rc = io.in(object_pose, nB * 16, &d_pose))) return rc;
  if ((rc = io.in(use_labels ? labels : nullptr, use_labels ? (size_t)o->depth.H * o->depth.W : 0, &d_labels))) return rc;
  if ((rc = io.in(use_labels ? held_label : nullptr, nB, &d_lab))) return rc;
  if ((rc = io.out(count_out, nB * Tp, &d_count))) return rc;
  if ((rc = gto_check_held_paths_device(h, o, B, Tp, d_paths, d_attach, attach_ld, attach_col, d_points, P_max, d_nheld, d_pose, d_labels, d_lab,
                                        base_pos, per_plan_base, d_count, nullptr)))
    return rc;
  return io.finish();
}

// The held object's clearance from the robot's own links (include/gto_solver.h; kernels: gto_held.h, gto_heldclear.h)
int gto_held_clearance_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const double* attach, int32_t attach_ld,
                              int32_t attach_col, const double* held_points, int32_t P_max, const int32_t* n_held,
                              const double* object_pose, const double* base_pos, int32_t per_plan_base, int32_t link_mask,
                              double cutoff, double* d2_out, int32_t* link_out, int32_t* point_out, void* stream) {
  std::string why;
  bool empty;
  if (int rc = gto_heldargs::check_held_clearance_args(h ? h->rb.n_links : GTO_MAX_LINKS, B, Tp, paths, attach, attach_ld, attach_col,
                                                       held_points, P_max, n_held, base_pos, link_mask, cutoff, d2_out, why, &empty))
    return fail(h, rc, why);
  if (!h) return GTO_ERR_INVALID_ARG;
  if (empty) return GTO_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int T = Tp, P = P_max;
  const size_t lds_att = sizeof(double) * held_attach_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  const size_t lds = sizeof(double) * held_clearance_lds_doubles(h->rb.n_frames, h->rb.n_links, h->rb.n_opt, h->rb.n_chunks);
  CheckBase base;
  int rc;
  if ((rc = check_lds_fits(h, lds_att)) || (rc = check_lds_fits(h, lds))) return rc;
  if ((rc = stage_check_base(h, base_pos, per_plan_base, B, st, &base))) return rc;
  if ((rc = ensure(h, h->hd_p, (size_t)B * P * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(h, h->hd_bad, (size_t)B * sizeof(int32_t)))) return rc;
  double* d_p = h->hd_p.as<double>();
  int32_t* d_bad = h->hd_bad.as<int32_t>();
  // attach NULL: the paths' own column 0, as in gto_check_held_paths_device
  const double* att = attach ? attach : paths;
  const int att_ld = attach ? attach_ld : T, att_col = attach ? attach_col : 0;
  const int tg = check_waypoints_per_group();
  HIPCHK(h, raise_dynamic_lds((const void*)k_held_attach, lds_att));
  HIPCHK(h, raise_dynamic_lds((const void*)k_held_clearance, lds));
  hipLaunchKernelGGL(k_held_attach, dim3((unsigned)B), dim3(256), lds_att, st, h->d_rb, att, att_ld, att_col, base.b0, base.b1, base.b2, base.d_base,
                     held_points, P, n_held, object_pose, d_p, d_bad);
  hipLaunchKernelGGL(k_held_clearance, dim3((unsigned)B, (unsigned)((T + tg - 1) / tg)), dim3(256), lds, st, h->d_rb, h->d_px, h->d_py, h->d_pz,
                     h->d_chunks, T, tg, paths, (const double*)d_p, P, n_held, (const int32_t*)d_bad, (uint32_t)link_mask, cutoff, d2_out,
                     link_out, point_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

int gto_held_clearance(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const double* attach, int32_t attach_ld,
                       int32_t attach_col, const double* held_points, int32_t P_max, const int32_t* n_held, const double* object_pose,
                       const double* base_pos, int32_t per_plan_base, int32_t link_mask, double cutoff, double* d2_out,
                       int32_t* link_out, int32_t* point_out) {
  std::string why;
  bool empty;
  if (int rc = gto_heldargs::check_held_clearance_args(h ? h->rb.n_links : GTO_MAX_LINKS, B, Tp, paths, attach, attach_ld, attach_col,
                                                       held_points, P_max, n_held, base_pos, link_mask, cutoff, d2_out, why, &empty))
    return fail(h, rc, why);
  if (!h) return GTO_ERR_INVALID_ARG;
  if (empty) return GTO_OK;
  for (int b = 0; b < B; ++b)
    if (n_held[b] < 0 || n_held[b] > P_max) return fail(h, GTO_ERR_INVALID_ARG, "gto_held_clearance: n_held must be in [0, P_max]");
  HIPCHK(h, hipSetDevice(h->device));
  Staging io(h);
  const size_t nB = (size_t)B, nd = (size_t)h->rb.ndof;
  const double *d_paths, *d_attach, *d_points, *d_pose;
  const int32_t* d_nheld;
  double* d_d2;
  int32_t *d_link, *d_point;
  int rc;
  if ((rc = io.in(paths, nB * nd * Tp, &d_paths))) return rc;
  if ((rc = io.in(attach, attach ? nB * nd * attach_ld : 0, &d_attach))) return rc;
  if ((rc = io.in(held_points, nB * P_max * 3, &d_points))) return rc;
  if ((rc = io.in(n_held, nB, &d_nheld))) return rc;
  if ((rc = io.in(object_pose, nB * 16, &d_pose))) return rc;
  if ((rc = io.out(d2_out, nB * Tp, &d_d2))) return rc;
  if ((rc = io.out(link_out, link_out ? nB * Tp : 0, &d_link))) return rc;
  if ((rc = io.out(point_out, point_out ? nB * Tp : 0, &d_point))) return rc;
  if ((rc = gto_held_clearance_device(h, B, Tp, d_paths, d_attach, attach_ld, attach_col, d_points, P_max, d_nheld, d_pose, base_pos,
                                      per_plan_base, link_mask, cutoff, d_d2, d_link, d_point, nullptr)))
    return rc;
  return io.finish();
}

}  // extern "C"

// ------------------------------------------------------------------ a resident occupancy grid and the placement report (gto_occupancy.h)
struct gto_occupancy {
  int device = 0;
  double origin[2] = {0, 0}, xlim[2] = {0, 0}, ylim[2] = {0, 0}, res = 0;
  int32_t shape[2] = {0, 0};
  DevBuf grid;  // device, uint8 [nx][ny], 0 / 1
};

namespace {
// what both builders check of their numbers before any device work
int check_occupancy_params(const char* who, double margin, double res, double epsilon) {
  const std::string w(who);
  if (!(res > 0.0) || !std::isfinite(res) || !std::isfinite(margin) || !(epsilon >= 0.0) || !std::isfinite(epsilon))
    return fail(nullptr, GTO_ERR_INVALID_ARG, w + ": margin, resolution > 0 and epsilon >= 0 must be finite");
  if (std::ceil(epsilon / res) > GTO_OCC_MAX_K) return fail(nullptr, GTO_ERR_UNSUPPORTED, w + ": epsilon beyond eight grid steps");
  return GTO_OK;
}
// The grid of GTORobotModel.setup_occupancy_grid (gto/gto_models.py:218-244) from points on the device, on the null stream,
// synchronous.  The lease is the caller's: everything but the grid goes back to the pool with it.
int build_occupancy(DepthLease& c, const OccPoints& pts, double margin, double res, double epsilon, gto_occupancy** out) {
  const std::string w(c.who);
  const int k = (int)std::ceil(epsilon / res);
  const unsigned blocks = (unsigned)std::min<long>(1024, std::max<long>(1, (pts.n + 255) / 256));
  double* d_part = c.alloc<double>((size_t)blocks * GTO_OCC_PART);
  if (!d_part) return c.no_memory();
  hipLaunchKernelGGL(k_occ_bounds, dim3(blocks), dim3(256), 0, 0, pts, d_part);
  DEPTH_TRY(c.sync());
  std::vector<double> part((size_t)blocks * GTO_OCC_PART);
  DEPTH_TRY(c.download(part.data(), d_part, part.size()));
  double xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  bool bad = false;
  for (unsigned i = 0; i < blocks; ++i) {
    const double* p = &part[(size_t)i * GTO_OCC_PART];
    xmax = std::max(xmax, p[0]), ymin = std::min(ymin, p[1]), ymax = std::max(ymax, p[2]), bad = bad || p[3] != 0.0;
  }
  if (!bad && ymin == INFINITY) return fail(nullptr, GTO_ERR_INVALID_ARG, w + ": no point with z > 0.01");
  if (bad || !std::isfinite(xmax)) return fail(nullptr, GTO_ERR_UNSUPPORTED, w + ": the points' bounds are not finite");
  std::unique_ptr<gto_occupancy> o(new gto_occupancy);
  o->device = c.device, o->res = res;
  o->xlim[0] = 0.0, o->xlim[1] = xmax, o->ylim[0] = ymin, o->ylim[1] = ymax;
  o->origin[0] = o->xlim[0] - margin, o->origin[1] = o->ylim[0] - margin;
  // the axes' lengths as numpy.arange counts them, as doubles: a finite but enormous coordinate is refused before anything
  // of that size is allocated
  const double lx = std::ceil(((o->xlim[1] + margin) - (o->xlim[0] - margin)) / res), ly = std::ceil(((o->ylim[1] + margin) - (o->ylim[0] - margin)) / res);
  const double most = (double)((size_t)1 << 26);
  if (!(lx >= 1.0 && ly >= 1.0 && lx <= most && ly <= most && lx * ly <= most))
    return fail(nullptr, GTO_ERR_UNSUPPORTED, w + ": empty grid or more than 2^26 nodes");
  const std::vector<double> xg = np_arange(o->xlim[0] - margin, o->xlim[1] + margin, res);
  const std::vector<double> yg = np_arange(o->ylim[0] - margin, o->ylim[1] + margin, res);
  if (xg.empty() || yg.empty() || xg.size() > ((size_t)1 << 26) || yg.size() > ((size_t)1 << 26) || xg.size() * yg.size() > ((size_t)1 << 26))
    return fail(nullptr, GTO_ERR_UNSUPPORTED, w + ": empty grid or more than 2^26 nodes");
  o->shape[0] = (int32_t)xg.size(), o->shape[1] = (int32_t)yg.size();
  const size_t nodes = xg.size() * yg.size();
  const double *d_xg, *d_yg;
  DEPTH_TRY(c.upload(xg.data(), xg.size(), &d_xg));
  DEPTH_TRY(c.upload(yg.data(), yg.size(), &d_yg));
  uint8_t* d_grid = c.alloc<uint8_t>(nodes);
  if (!d_grid) return c.no_memory();
  DEPTH_TRY(c.hip(hipMemset(d_grid, 0, nodes)));
  hipLaunchKernelGGL(k_occ_mark, dim3((unsigned)((pts.n + 255) / 256)), dim3(256), 0, 0, pts, d_xg, d_yg, o->shape[0], o->shape[1], res,
                     epsilon, k, d_grid);
  DEPTH_TRY(c.sync());
  o->grid = c.keep(d_grid);
  *out = o.release();
  return GTO_OK;
}
}  // namespace

extern "C" {

int gto_occupancy_from_observation(gto_observation* obs, double margin, double resolution, double epsilon, gto_occupancy** out) {
  if (out) *out = nullptr;
  if (!out || !obs) return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_occupancy_from_observation: null observation or output");
  DEPTH_TRY(check_occupancy_params("gto_occupancy_from_observation", margin, resolution, epsilon));
  if (hipSetDevice(obs->device) != hipSuccess) return fail(nullptr, GTO_ERR_NO_DEVICE, "hipSetDevice failed");
  DepthLease c(nullptr, "gto_occupancy_from_observation", obs->device);
  OccPoints pts;
  if (obs->is_depth) pts = {obs->depth.px, obs->depth.py, obs->depth.pz, (long)obs->depth.H * obs->depth.W, 1, 1};
  else pts = {obs->cloud.points, obs->cloud.points + 1, obs->cloud.points + 2, (long)obs->cloud.n, 3, 0};
  return build_occupancy(c, pts, margin, resolution, epsilon, out);
}

int gto_occupancy_from_points(int device, const double* points, int64_t n, double margin, double resolution, double epsilon,
                              gto_occupancy** out) {
  if (out) *out = nullptr;
  if (!out || !points || n < 1) return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_occupancy_from_points: null or empty input");
  if (n > ((int64_t)1 << 28)) return fail(nullptr, GTO_ERR_UNSUPPORTED, "gto_occupancy_from_points: more than 2^28 points");
  DEPTH_TRY(check_occupancy_params("gto_occupancy_from_points", margin, resolution, epsilon));
  int cur_dev;
  DEPTH_TRY(select_device(device, &cur_dev));
  DepthLease c(nullptr, "gto_occupancy_from_points", cur_dev);
  const double* d_p;
  DEPTH_TRY(c.upload(points, (size_t)n * 3, &d_p));
  return build_occupancy(c, {d_p, d_p + 1, d_p + 2, (long)n, 3, 0}, margin, resolution, epsilon, out);
}

int gto_occupancy_geometry(const gto_occupancy* occ, double* origin, int32_t* shape, double* xlim, double* ylim) {
  if (!occ) return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_occupancy_geometry: null occupancy grid");
  if (origin) std::memcpy(origin, occ->origin, sizeof occ->origin);
  if (shape) std::memcpy(shape, occ->shape, sizeof occ->shape);
  if (xlim) std::memcpy(xlim, occ->xlim, sizeof occ->xlim);
  if (ylim) std::memcpy(ylim, occ->ylim, sizeof occ->ylim);
  return GTO_OK;
}

int gto_occupancy_grid(gto_occupancy* occ, uint8_t* out) {
  if (!occ || !out) return fail(nullptr, GTO_ERR_INVALID_ARG, "gto_occupancy_grid: null occupancy grid or output");
  if (hipSetDevice(occ->device) != hipSuccess) return fail(nullptr, GTO_ERR_NO_DEVICE, "hipSetDevice failed");
  const hipError_t e = hipMemcpy(out, occ->grid.get(), (size_t)occ->shape[0] * occ->shape[1], hipMemcpyDeviceToHost);
  return e == hipSuccess ? GTO_OK : fail(nullptr, GTO_ERR_HIP, std::string("gto_occupancy_grid: ") + hipGetErrorString(e));
}

void gto_occupancy_destroy(gto_occupancy* occ) {
  if (!occ) return;
  int cur = -1;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(occ->device);
  (void)hipDeviceSynchronize();  // nothing may still be reading it
  delete occ;  // frees the grid
  if (cur >= 0) (void)hipSetDevice(cur);  // the caller's current device is the caller's
}

int gto_base_report_device(gto_handle* h, gto_occupancy* occ, int32_t B, int32_t n_max, const int32_t* n_goals, const double* qc,
                           const double* goals, const double* y, const double* q, double* err_pos_out, double* err_rot_out,
                           int32_t* collision_out, int32_t* first_free_out, void* stream) {
  if (!h) return GTO_ERR_INVALID_ARG;
  if (B < 0) return fail(h, GTO_ERR_INVALID_ARG, "gto_base_report_device: B must be >= 0");
  if (!occ && (collision_out || first_free_out))
    return fail(h, GTO_ERR_INVALID_ARG, "gto_base_report_device: collision_out and first_free_out need an occupancy grid");
  if (occ && occ->device != h->device)
    return fail(h, GTO_ERR_INVALID_ARG, "gto_base_report_device: the occupancy grid lives on another device than the handle");
  bool empty;
  int rc = base_check(h, "gto_base_report_device", B, n_max, n_goals, !n_goals || !qc || !goals || !y || !q, &empty);
  if (rc || empty) return rc;
  if (B > 65535) return fail(h, GTO_ERR_UNSUPPORTED, "gto_base_report_device: at most 65535 goal sets in one call");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const bool count = occ && (collision_out || first_free_out);
  if (!count && !err_pos_out && !err_rot_out) return GTO_OK;
  const size_t lds = sizeof(double) * plan_cost_lds_doubles_tg(1, h->rb.n_frames, h->rb.n_links, h->rb.n_opt);
  if (lds > 150 * 1024) return fail(h, GTO_ERR_UNSUPPORTED, "robot too large for the report kernel's LDS");
  const int32_t* d_ng;
  if ((rc = base_counts_to_device(h, B, n_goals, st, &d_ng))) return rc;
  if (count && !collision_out) {  // the choice alone: the counts stay in the handle's workspace
    if ((rc = ensure(h, h->bs_coll, (size_t)B * sizeof(int32_t)))) return rc;
    collision_out = h->bs_coll.as<int32_t>();
  }
  OccGridView og = {};
  if (count) og = {occ->grid.as<uint8_t>(), occ->shape[0], occ->shape[1], occ->origin[0], occ->origin[1], occ->res};
  HIPCHK(h, raise_dynamic_lds((const void*)k_base_report, lds));
  hipLaunchKernelGGL(k_base_report, dim3((unsigned)(n_max + (count ? 1 : 0)), (unsigned)B), dim3(256), lds, st, h->d_rb, h->d_px, h->d_py,
                     h->d_pz, h->d_plink, d_ng, qc, goals, y, q, n_max, og, err_pos_out, err_rot_out, count ? collision_out : nullptr);
  if (first_free_out) hipLaunchKernelGGL(k_base_first_free, dim3(1), dim3(64), 0, st, collision_out, B, first_free_out);
  HIPCHK(h, hipGetLastError());
  return GTO_OK;
}

}  // extern "C"
