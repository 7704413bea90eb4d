/*
 * gto_solver.h — C ABI of the MI355X-native GTO inner solver (libgto_hip.so).
 *
 * Drop-in boundary for the ONE hot path of IRVLUTD/GraspTrajOpt: the optimisation solve behind
 *   GTOPlanner.plan_goalset()/plan()            reference gto/gto_planner.py:145-245
 *   -> optas.CasADiSolver("ipopt").solve()      reference optas/solver.py:126-159, 388-400
 * The reference has no native FFI (it is 100 % Python on top of CasADi/IPOPT); the entry points
 * below are what a ctypes binding inside the reference's GTOPlanner would call instead of
 * `self.solver.solve()` (see INTEGRATION.md for the stub).  Each function cites the reference
 * code whose role it takes over.
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; `void* stream` is a hipStream_t passed as an
 *     opaque pointer (NULL = the handle's own stream).
 *   - host arrays are row-major (NumPy default) double / float / int32 unless stated.
 *   - every function returns GTO_OK (0) or a negative error code; gto_last_error() gives text.
 *   - a handle is bound to one HIP device and one stream; it is not thread-safe; host-pointer
 *     calls are synchronous on return (the reference is synchronous single-threaded Python).
 *   - the caller owns all host buffers; the library owns all device memory behind the handle.
 */
#ifndef GTO_SOLVER_H
#define GTO_SOLVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTO_OK 0
#define GTO_ERR_INVALID_ARG (-1)
#define GTO_ERR_HIP (-2)
#define GTO_ERR_NO_DEVICE (-3)
#define GTO_ERR_UNSUPPORTED (-4)
#define GTO_ERR_NO_SCENE (-5)
#define GTO_ERR_ALLOC (-6)

/* compile-time capacity of the kernels */
#define GTO_MAX_FRAMES 32 /* kinematic frames after pruning            */
#define GTO_MAX_LINKS 32  /* collision links carrying surface points   */
#define GTO_MAX_OPT 16    /* optimised joints (Panda/Fetch arm: 7, mobile Fetch: 10); IK / base placement: up to 8 */
#define GTO_MAX_DOF 32    /* actuated joints (Panda 9, Fetch 15)        */
/* Surface points: at most 16384, taken link by link in runs of up to 64 points, at most 256 runs in all (a link of 65 points
 * takes two).  Every robot within these limits is created, at every T from 4 to 96: where a robot's tables
 * leave no room for the obstacle kernel's usual waypoints per workgroup, it runs fewer (same results). */

/* joint types (optas/models.py:850-866) */
#define GTO_JOINT_FIXED 0
#define GTO_JOINT_REVOLUTE 1 /* revolute and continuous */
#define GTO_JOINT_PRISMATIC 2

/* obstacle-gradient source */
#define GTO_GRAD_CENTRAL_DIFF 0 /* gto/sdf_callback.py:90-114 JacFun numerics (shipped default) */
#define GTO_GRAD_ZERO 1         /* what CasADi AD sees through floor()+gather in the reference   */

/* how gto_solve_batch[_device] runs the Levenberg-Marquardt iterations (same algorithm, same results to round-off) */
#define GTO_MODE_ROUNDS 0        /* default: rounds of two launches (evaluate / step) over at most 384 instances in flight,
                                    every evaluation spread over the whole GPU: highest throughput, lowest latency */
#define GTO_MODE_SINGLE_LAUNCH 1 /* reserved: the single-launch kernel of rounds 1-3 (one workgroup runs an instance's whole
                                    solve; 2.4-2.9x slower than the rounds) was removed; gto_set_mode answers
                                    GTO_ERR_UNSUPPORTED */

/* per-instance solver status (mirrors "return the iterate anyway", optas/solver.py:135) */
#define GTO_STATUS_CONVERGED 0
#define GTO_STATUS_MAX_ITER 1
#define GTO_STATUS_NUMERICAL 2
#define GTO_STATUS_INFEASIBLE 3 /* gto_retime_paths_torque only: a joint cannot hold the path at rest under its torque limit */

/*
 * Robot description: the facts the reference pulls from the URDF through optas.RobotModel
 * (optas/models.py:236-321, 826-868) and GTORobotModel (gto/gto_models.py:62-101).
 * Frames are listed parents-before-children; frame i is reached from parent[i] by the fixed
 * origin transform rt2tr(rpy2r(rpy), xyz) followed by the joint motion about/along `axis`.
 * The small end: every count may be 1 (one frame, whose joint then sits on the root itself, one optimised joint, one
 * link, one surface point, one gripper point), frame_ee and frame_gripper may be any two frames, above every optimised
 * joint included, and no link need hang below an optimised joint (tests/small_robots.py).
 * Joint numbering: q_index may number the actuated joints in any order (a URDF may list its joints in any order; the
 * frames' order is not the joints').  opt_index lists distinct joints and need not be ascending, contiguous or in the
 * order of the kinematic chain; parameter joints may lie between optimised ones.  Entry j of opt_index is optimised
 * slot j: lower[j] and upper[j] are the limits of joint opt_index[j], and the blocks of gto_eval_obstacle_normal_eq come
 * in slot order.  Every [ndof] axis of the entry points below is indexed by q_index's numbering.  Renumbering a robot's
 * joints permutes those axes and changes nothing else (tests/renumbered_robots.py).
 */
typedef struct gto_robot_desc {
  int32_t n_frames;
  const int32_t* parent;     /* [n_frames]    -1 for the root                                  */
  const int32_t* joint_type; /* [n_frames]    GTO_JOINT_*                                      */
  const int32_t* q_index;    /* [n_frames]    index into q (0..ndof-1) or -1 for fixed joints  */
  const double* origin_xyz;  /* [n_frames*3]  joint origin (optas/models.py:642-651)           */
  const double* origin_rpy;  /* [n_frames*3]                                                   */
  const double* axis;        /* [n_frames*3]  NOT yet normalised (optas/models.py:653-659)     */
  int32_t ndof;              /* actuated joints, URDF order (optas/models.py:349-354)          */
  int32_t n_opt;             /* optimised joints (optas/models.py:366-386)                     */
  const int32_t* opt_index;  /* [n_opt]       indexes into q: distinct, in any order           */
  const double* lower;       /* [n_opt]       joint limits of the optimised joints, lower[j]   */
  const double* upper;       /* [n_opt]       and upper[j] those of joint opt_index[j]         */
  int32_t n_links;           /* links with surface points (gto/gto_models.py:62-80)            */
  const int32_t* link_frame; /* [n_links]     frame index of each collision link               */
  const double* visual_xyz;  /* [n_links*3]   visual origin (gto/gto_models.py:95-100)         */
  const double* visual_rpy;  /* [n_links*3]                                                    */
  int32_t n_points;
  const double* points;      /* [n_points*3]  surface points in the visual-mesh frame          */
  const int32_t* point_link; /* [n_points]    in [0, n_links)                                  */
  int32_t frame_ee;          /* link_ee      (gto/gto_planner.py:35)                           */
  int32_t frame_gripper;     /* link_gripper (gto/gto_planner.py:36)                           */
  int32_t n_gripper_points;
  const double* gripper_points; /* [n_gripper_points*3] in the gripper LINK frame (:37)        */
} gto_robot_desc;

/* Planner constants the reference hard-codes (gto/gto_planner.py:25-30,131,135,141). */
typedef struct gto_solver_opts {
  int32_t T;               /* waypoints, reference 50                                        */
  double Tmax;             /* reference 10.0 -> dt = Tmax/(T-1)                              */
  int32_t standoff_offset; /* reference -10 -> standoff waypoint T+offset                    */
  double w_obstacle;       /* reference 10                                                   */
  double w_vel;            /* reference 0.01                                                 */
  int32_t max_iter;        /* Gauss-Newton/LM iterations (reference IPOPT cap: 100)          */
  double tol_step;         /* stop when max|dq| of an accepted step is below this [rad]      */
  double tol_rel_f;        /* stop when an accepted step lowers f by less than this * (1+f)  */
  double lambda0;          /* initial LM damping                                             */
  int32_t grad_mode;       /* GTO_GRAD_*                                                     */
} gto_solver_opts;

typedef struct gto_handle gto_handle;

/* Fill opts with the reference's constants and this solver's defaults. */
void gto_default_opts(gto_solver_opts* opts);

/* Library/ABI version (major*1000 + minor): GTO_ABI_VERSION of the header the library was built from.  A binding checks it
 * when it loads the library and refuses another number (grasptrajopt_amd/_capi.py load_library): every change of a
 * signature or of a struct in this header bumps the minor.  Entry points that are only ADDED leave it alone (the occupancy
 * grid and the base placement chain at the end of this header came that way): no existing call changes its meaning, and a
 * binding that needs them refuses a library that lacks them by name (grasptrajopt_amd/_capi.py load_library). */
#define GTO_ABI_VERSION 1012
int32_t gto_version(void);

/*
 * Create a solver bound to HIP device `device` (a negative value keeps the current device).
 * Copies everything it needs out of `desc`.  Fails loudly (GTO_ERR_NO_DEVICE) without a GPU:
 * there is no CPU fallback behind this ABI.
 * Replaces: GTOPlanner.__init__ + setup_optimization graph construction
 *           (gto/gto_planner.py:22-142) and CasADiSolver.setup (optas/solver.py:335-386).
 */
int gto_create(const gto_robot_desc* desc, const gto_solver_opts* opts, int device, gto_handle** out);
void gto_destroy(gto_handle* h);
const char* gto_last_error(const gto_handle* h); /* h may be NULL: error of the last failed create */

/* Change solver options that do not alter problem dimensions (max_iter, tolerances, weights,
 * lambda0, grad_mode, Tmax, standoff_offset). T must stay the same.  The options take effect at the next call; a call
 * reads them once, when it starts.
 * Accepted, here and by gto_create: 4 <= T <= GTO_MAX_T; Tmax and lambda0 positive and finite; w_obstacle, w_vel, tol_step
 * and tol_rel_f finite and >= 0 (a zero weight drops its term, a zero tolerance switches its ending off); max_iter >= 0;
 * T + standoff_offset in [2, T-1]; a known grad_mode.  Anything else is GTO_ERR_INVALID_ARG with a message that names the
 * field, and the handle keeps the options it had. */
int gto_set_opts(gto_handle* h, const gto_solver_opts* opts);

/*
 * Upload (or replace) the voxelised cost fields of scene `scene_id` (0 <= scene_id < 65536).
 * c_all / c_obs: float32 [shape0*shape1*shape2], C order, x slowest (gto/gto_models.py:155-171,
 * 184-186); c_obs may be NULL (then c_obs = c_all).  origin/res: gto/gto_models.py:159,46.
 * Replaces: reset_parameters({"sdf_cost_all":..,"sdf_cost_obstacle":..}) (gto/gto_planner.py:227-236).
 * One-time per scene; not part of the timed solve.
 */
int gto_set_scene(gto_handle* h, int32_t scene_id, const float* c_all, const float* c_obs,
                  const int32_t shape[3], const double origin[3], double res);
/* The same upload without the solver's acceleration structures (voxel records, distance fields: 3.6x the bytes of the
 * two fields and 48 relaxation sweeps): such a scene serves gto_plan_cost and gto_eval_points only (seed scoring of a
 * field that is never solved on: GTORobotModel.compute_plan_cost, gto/gto_models.py:204-215); every solve or
 * objective entry point rejects it with GTO_ERR_NO_SCENE. */
int gto_set_scene_values(gto_handle* h, int32_t scene_id, const float* c_all, const float* c_obs,
                         const int32_t shape[3], const double origin[3], double res);
int gto_drop_scene(gto_handle* h, int32_t scene_id);

/*
 * Solve B independent (scene, goal-set) instances.  Host pointers; synchronous.
 *   scene_id  [B]
 *   qc        [B, ndof]        current configuration (gto/gto_planner.py:47-49,59-62)
 *   goals     [B, n_max, 16]   goal poses of link_ee in the robot-base frame, each 4x4 row-major
 *                              (tf_goal column = RT.flatten(), gto/gto_planner.py:188-191)
 *   n_goals   [B]              1 <= n_goals[b] <= n_max (goal-set min, gto/gto_planner.py:105)
 *   standoff  [B, 16] or NULL  standoff pose S (optas/spatialmath.py:160-183); NULL = use_standoff False
 *   base_pos  [B, 3]           base_position parameter (gto/gto_planner.py:56,116)
 *   Q0        [B, ndof, T]     seed trajectory incl. parameter-joint rows (gto/gto_planner.py:193-224,234)
 * Outputs (any may be NULL):
 *   Q_out [B, ndof, T], dQ_out [B, ndof, T-1], cost_out [B] (objective f, Appendix A of SURVEY.md),
 *   iters_out [B], status_out [B] (GTO_STATUS_*).
 * B may be as large as the caller has work: the solver keeps at most 384 instances in flight (environment
 * GTO_SLOTS when the handle is created) and hands the slot of an instance that finishes to the next one that
 * has not started, so large calls keep the GPU full to the end; every instance gets bit for bit the result it
 * gets in a call of its own.  Device workspace: ~75 KB per instance of the call.
 * Replaces: reset_initial_seed + reset_parameters + solve + solution unpacking
 *           (gto/gto_planner.py:222-245, optas/solver.py:103-159).
 */
int gto_solve_batch(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id,
                    const double* qc, const double* goals, const int32_t* n_goals,
                    const double* standoff, const double* base_pos, const double* Q0,
                    double* Q_out, double* dQ_out, double* cost_out, int32_t* iters_out,
                    int32_t* status_out);

/*
 * Same contract with every array already resident in device memory (HBM) and the work enqueued
 * on `stream` (asynchronous; outputs are valid after the stream is synchronised).
 */
int gto_solve_batch_device(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id,
                           const double* qc, const double* goals, const int32_t* n_goals,
                           const double* standoff, const double* base_pos, const double* Q0,
                           double* Q_out, double* dQ_out, double* cost_out, int32_t* iters_out,
                           int32_t* status_out, void* stream);

/*
 * Let `dst` use scene `src_id` of `src` under the id `dst_id` without a second copy in HBM (fields, voxel
 * records, distance fields: 148 MB for a 128^3 scene).  For handles that work on the same scene side by side
 * (grasptrajopt_amd.parallel.BatchPipeline).  `src` keeps ownership: it must outlive `dst`'s use of the
 * scene, and replacing or dropping the scene in `src` invalidates the borrowed entry.
 */
int gto_share_scene(gto_handle* dst, int32_t dst_id, gto_handle* src, int32_t src_id);
/* The same with a choice of halves: `dst`'s sdf_cost_all is `src`'s field number all_from, its sdf_cost_obstacle `src`'s
 * field number obs_from (0: the source's sdf_cost_all, 1: its sdf_cost_obstacle; gto_share_scene = (0, 1)).  For a
 * caller that holds ONE field of a resident scene and hands it to an entry point that reads the obstacle half
 * (IKSolver.solve_ik and GTORobotModel.compute_plan_cost take `sdf_cost_obstacle`, gto/ik_solver.py:78,
 * gto/gto_models.py:204): whichever half the field is, it is the half the entry point reads. */
int gto_share_scene_halves(gto_handle* dst, int32_t dst_id, gto_handle* src, int32_t src_id, int32_t all_from,
                           int32_t obs_from);

/*
 * Inverse kinematics for B goal poses of link_ee: the pre-step that produces the
 * q_solutions of plan_goalset.  T = 1 problem of gto/ik_solver.py:30-110:
 *   min_q sum_k ||T_g(q) p_k - RT G p_k||^2 + w_obstacle * sum_pts c_obs[off(x(q))],  lo <= q <= hi,
 * seeded at q0 (parameter joints of q0 are kept), solved by the same projected Levenberg-Marquardt as the
 * trajectory problem; the whole iteration runs on the GPU, one workgroup per goal.
 *   scene_id  [B] or NULL.  NULL = no collision term (IKSolver(collision_avoidance=False), :63)
 *   q0        [B][ndof]     seed configurations (:79)
 *   goals     [B][16]       RT of link_ee, row-major 4x4 (:83)
 *   base_pos  [B][3] or NULL (zeros)
 *   max_iter  iteration cap (reference IPOPT cap: 50, :76)
 * Outputs (host, may be NULL except q_out): q_out [B][ndof], cost_out [B] objective value, iters_out,
 * status_out as in gto_solve_batch.  The reference's err_pos / err_rot / plan cost (:88-97) follow from
 * gto_eval_fk and gto_plan_cost.
 * Replaces: IKSolver.setup_optimization + solve_ik (gto/ik_solver.py:30-110).
 */
int gto_solve_ik_batch(gto_handle* h, int32_t B, const int32_t* scene_id, const double* q0, const double* goals,
                       const double* base_pos, int32_t max_iter, double* q_out, double* cost_out, int32_t* iters_out,
                       int32_t* status_out);

/*
 * Inverse kinematics to position + orientation goals of link_ee: the T = 1 problem of gto/ik_solver.py (collision term
 * 10 * sum(sdf_cost_obstacle[offsets]), URDF joint limits, cap 50) with the pose term of
 *   GTO_IK_GOAL_POINTS      gto/ik_solver.py:48-54           goals [B][16]: RT of link_ee, exactly gto_solve_ik_batch
 *   GTO_IK_GOAL_QUATERNION  gto/ik_solver_quaternion.py:50-55 goals [B][7] = x y z qx qy qz qw (tf_goal of :81-84; the
 *                           quaternion is not normalised):  |p - g[0:3]|^2 + 1 - (quat(link_ee) . g[3:7])^2
 *   GTO_IK_GOAL_RPY         gto/ik_solver_rpy.py:53-58       goals [B][6] = x y z roll pitch yaw (tf_goal of :84-89):
 *                           |p - g[0:3]|^2 + |(rpy(link_ee) - g[3:6]) / pi|^2, rpy as optas Quaternion.getrpy (pitch
 *                           +pi/2 whenever |R20| >= 1; no angle wrapping: the term jumps where an angle crosses +-pi)
 * p, quat, rpy: link_ee in the robot-base frame.  Arguments, outputs, max_iter = 0 (the objective at the clipped seed)
 * and the limit of eight optimised joints (GTO_ERR_UNSUPPORTED beyond) as in gto_solve_ik_batch; an unknown goal_kind
 * fails with GTO_ERR_INVALID_ARG.
 * Non-finite inputs.  A seed's optimised joints are clipped to the joint limits first (NaN -> lower, +-Inf -> the limit),
 * so only goals and parameter joints can leave the objective at the seed non-finite.  GTO_IK_GOAL_QUATERNION / RPY:
 * such an instance ends at once with GTO_STATUS_NUMERICAL, 0 iterations, q_out = the clipped seed and its non-finite
 * objective in cost_out (the rule of gto_solve_batch), never GTO_STATUS_CONVERGED.  GTO_IK_GOAL_POINTS returns what
 * gto_solve_ik_batch returns, bit for bit, and that entry point keeps its own ending: its pose term takes a non-finite
 * goal as an infinite objective, every step is rejected until the damping passes 1e15, and the instance comes back
 * GTO_STATUS_CONVERGED after 11 iterations at the clipped seed with cost_out = +Inf (measured; check cost_out).
 * Replaces: IKSolver.setup_optimization + solve_ik of gto/ik_solver_quaternion.py:30-115 and gto/ik_solver_rpy.py:30-121.
 */
#define GTO_IK_GOAL_POINTS 0     /* gto/ik_solver.py: goals [B][16], same as gto_solve_ik_batch */
#define GTO_IK_GOAL_QUATERNION 1 /* gto/ik_solver_quaternion.py: goals [B][7] = x y z qx qy qz qw */
#define GTO_IK_GOAL_RPY 2        /* gto/ik_solver_rpy.py: goals [B][6] = x y z roll pitch yaw */
int gto_solve_ik_pose_batch(gto_handle* h, int32_t goal_kind, int32_t B, const int32_t* scene_id, const double* q0,
                            const double* goals, const double* base_pos, int32_t max_iter, double* q_out, double* cost_out,
                            int32_t* iters_out, int32_t* status_out);

/*
 * Base placement of a mobile manipulator for B goal sets: where to park the base so that
 * every goal of the set is reachable.  Problem of gto/base_planner.py:35-94 with T = goal_size:
 *   min  effort_weight * |(x,y,theta)|^2 + sum_i sum_k | T_g(q_i) p_k - B(x,y,theta) RT_i G p_k |^2 ,
 *   lo <= q_i <= hi (:92),  -pi <= theta <= pi (:55),  B = rt2tr(rotz(theta), [x,y,0]) (:49-51),
 * unknowns: the base pose and ONE arm configuration per goal (:58-60); seeded at the zero pose and at qc
 * for every goal (:104-105).  Same projected Levenberg-Marquardt as the trajectory problem, the whole
 * iteration on the GPU, one workgroup per goal set; the arrow-shaped normal equations are eliminated
 * goal block by goal block onto the 3x3 base block.
 *   n_max     row stride of goals / q_out, 1 <= n_goals[b] <= n_max <= 32
 *   n_goals   [B]
 *   qc        [B][ndof]          current configuration (:96)
 *   goals     [B][n_max][16]     RT_i of link_ee in the CURRENT base frame, row-major 4x4 (:98-101)
 *   max_iter  iteration cap (reference IPOPT cap: 100, :95)
 * Outputs (host): y_out [B][3] = (x, y, theta), the old base in the new base frame (:52);
 * q_out [B][n_max][ndof] arm configuration per goal (rows >= n_goals[b]: qc); cost_out, iters_out,
 * status_out as in gto_solve_batch (may be NULL).  An optimised joint that moves none of the gripper's frame has a zero
 * diagonal entry in every goal block; it is damped by lambda itself, as in gto_solve_ik_batch, and keeps its value of qc.
 * err_pos / err_rot (:127-143) and the occupancy statistic (:146-158)
 * of the solution: gto_base_report_device below (on the host: gto_eval_fk and gto_eval_points' transformed points).
 * Replaces: BasePlanner.setup_optimization + the solve inside plan_goalset (gto/base_planner.py:35-123).
 */
int gto_solve_base_batch(gto_handle* h, int32_t B, int32_t n_max, const int32_t* n_goals, const double* qc,
                         const double* goals, double effort_weight, int32_t max_iter, double* y_out, double* q_out,
                         double* cost_out, int32_t* iters_out, int32_t* status_out);

/* Select the solver mode for the following solves: GTO_MODE_ROUNDS is the only one left. */
int gto_set_mode(gto_handle* h, int32_t mode);

/*
 * Lanes of a solve call.  gto_solve_batch / gto_solve_batch_device deal the instances of a call to up to `max_lanes`
 * lanes (contiguous ranges of at least `min_per_lane` instances), each with a HIP stream and lists of its own over the
 * one workspace of the call and a host thread of the call feeding it (lane 0: the calling thread): one lane's evaluation
 * launch overlaps another's step launch while the GPU is full.  A lane with at most `adopt_below` instances left
 * (0: never) hands them to lane 0, which runs the stragglers of the whole call as one chain of launches.
 * DEFAULTS of a new handle: max_lanes 1, min_per_lane 256, adopt_below 0 (environment: GTO_LANES, GTO_LANE_MIN,
 * GTO_ADOPT) -- one lane, no thread but the caller's, everything on the handle's stream.
 * With ONE lane the call runs on the handle's stream (the `stream` argument of gto_solve_batch_device).  With SEVERAL,
 * every lane -- lane 0 too -- runs on a stream of its own (the handle's, created with the greatest priority, or the
 * caller's: gto_set_lane_streams); the caller's stream only BRACKETS the call: it carries the seeds and the static-link
 * pass in front, the lanes wait for that, and the results are ordered behind all lanes on it.  Results do not depend on
 * any of the three numbers (tests/test_gpu_parity.py).  The reference has no counterpart: gto/gto_planner.py:185-245
 * solves one instance per call.
 */
int gto_set_lanes(gto_handle* h, int32_t max_lanes, int32_t min_per_lane, int32_t adopt_below);
/*
 * The lanes' streams.  By default the handle creates a non-blocking stream per lane.  The runtime deals streams to a few
 * hardware queues (GPU_MAX_HW_QUEUES, default 4) and the queues to the dispatcher's pipes; which stream lands where
 * depends on every stream the process has created, and two lanes behind one pipe run 1.5x slower.  A caller that manages
 * its streams (torch.cuda.Stream, one per lane) hands them over here: lane l of every following call runs on streams[l]
 * (n = 0: the handle's own again).  The streams stay the caller's; they must outlive the calls.
 */
int gto_set_lane_streams(gto_handle* h, int32_t n, void* const* streams);

/*
 * Bind the handle to the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream): every
 * launch and copy of every entry point then goes to that stream and the handle creates none of its
 * own.  NULL gives the handle a private non-blocking stream again (the state after gto_create).
 * The runtime maps streams onto a small number of hardware queues (GPU_MAX_HW_QUEUES, default 4);
 * handles that are meant to overlap on one GPU (grasptrajopt_amd.parallel.BatchPipeline) should each
 * own exactly one stream so that no two of them share a queue.
 */
int gto_set_stream(gto_handle* h, void* stream);

/* Time spent inside the dominant kernel (gto_obstacle_gram) during the most recent solve,
 * measured with HIP events on the launch stream: total milliseconds and launch count. */
int gto_last_kernel_time(gto_handle* h, double* total_ms, int32_t* launches);
/* Work the dominant kernel did during the most recent solve (profiling enabled): surface points it looked up in
 * a field (one 32-B voxel record or one float each; the broad phase skips the rest, which would read exact
 * zeros) and chunk bounding spheres it tested.  bench.py prices the kernel's roofline on the points gathered. */
int gto_last_kernel_work(gto_handle* h, uint64_t* points_gathered, uint64_t* chunk_tests);
/* The same per kernel VARIANT of the solve loop (profiling enabled), so that time, launches and work of one variant are
 * never mixed with another's: launches, their summed HIP-event time, the workgroups they were laid out for and (obstacle
 * variants) the surface points they gathered during the most recent gto_solve_batch[_device] call. */
#define GTO_PROF_OBSTACLE 0      /* k_obstacle_gram<NP,1>: the launches that fill the GPU */
#define GTO_PROF_OBSTACLE_FEW 1  /* k_obstacle_gram<8,8>: launches with few instances in flight */
#define GTO_PROF_STEP 2          /* k_lm_step<4,1> (k_lm_step_wide for nine to sixteen optimised joints) */
#define GTO_PROF_STEP_FEW 3      /* k_lm_step<8,4>: few instances in flight, candidate trial points */
#define GTO_PROF_SEED_TEST 4     /* k_seed_broad: the seeds of the instances that wait for a slot, once per call (none: 0 launches) */
#define GTO_PROF_VARIANTS 5
int gto_last_kernel_profile(gto_handle* h, int32_t variant, double* total_ms, int32_t* launches, uint64_t* workgroups,
                            uint64_t* points_gathered);
/* Enable/disable per-launch event timing of the solve loop's kernels (off by default). */
int gto_set_profiling(gto_handle* h, int32_t enabled);

/* ---- evaluation entry points (host pointers, synchronous): the pieces of the objective the
 * reference evaluates through CasADi Functions; used by the parity tests and by the seed /
 * collision-filter steps around the solve. ---------------------------------------------------- */

/* Global transform of every frame, [nq, n_frames, 16] row-major 4x4
 * (optas/models.py:826-868 get_global_link_transform). */
int gto_eval_fk(gto_handle* h, int32_t nq, const double* q /*[nq,ndof]*/, double* frames_out);

/* World surface points x = visual_tf(q) p + base (gto/gto_planner.py:114-116), their flat voxel
 * offsets (gto/gto_models.py:174-187), nearest-voxel cost values of both fields and the
 * central-difference gradient of the field selected by `use_obs` (gto/sdf_callback.py:43-49,
 * 90-114).  Any output may be NULL.  Points are reported in the caller's original order. */
int gto_eval_points(gto_handle* h, int32_t scene_id, int32_t nq, const double* q /*[nq,ndof]*/,
                    const double* base_pos /*[nq,3]*/, int32_t use_obs,
                    double* xyz_out /*[nq,P,3]*/, int32_t* offset_out /*[nq,P]*/,
                    double* value_out /*[nq,P]*/, double* grad_out /*[nq,P,3]*/);

/* The Hessian of the field selected by `use_obs` at the same surface points, [nq, P, 9] row-major 3x3: mixed central
 * differences (f(i+e_a+e_b) - f(i+e_a-e_b) - f(i-e_a+e_b) + f(i-e_a-e_b)) / (4 res^2) of the nearest-voxel values with every
 * sample's indices clipped on their own (gto/sdf_callback.py:159-183, HesFun.eval / get_value).  The solve never reads it
 * (Gauss-Newton); it completes the SDFCallback / JacFun / HesFun triple of the reference behind this ABI. */
int gto_eval_points_hessian(gto_handle* h, int32_t scene_id, int32_t nq, const double* q /*[nq,ndof]*/,
                            const double* base_pos /*[nq,3]*/, int32_t use_obs, double* hess_out /*[nq,P,9]*/);

/* ---- rigid-body dynamics.  Added without a new ABI number: gto_robot_desc is as it was. ------------------------------ */

/* The inertials of the handle's frames: frame f is the rigid body that joint f moves (the indexing of parent / joint_type /
 * q_index).  mass >= 0 and finite; mass == 0 is a massless frame whose other entries are ignored.  Where mass > 0 the centre
 * of mass is finite and the inertia (about the centre of mass, in the frame's axes) symmetric positive semidefinite.
 * gravity is in the base frame.  Anything else: GTO_ERR_INVALID_ARG with a message, and the handle keeps what it had.  May be
 * repeated; a synchronising upload, like a scene.  A handle without inertials answers gto_inverse_dynamics with
 * GTO_ERR_INVALID_ARG "no link inertials set".
 * Replaces: the <inertial> blocks the reference's URDFs carry and its planner never reads (optas/models.py:1735-1888 takes
 * them from urdf_parser_py). */
int gto_set_link_inertials(gto_handle* h, const double* mass /*[n_frames]*/, const double* com /*[n_frames*3]*/,
                           const double* inertia /*[n_frames*6]: ixx ixy ixz iyy iyz izz*/,
                           const double gravity[3] /*NULL = (0, 0, -9.81)*/);

/* Inverse dynamics tau = M(q) qdd + C(q, qd) qd + g(q) of n rows, by recursive Newton-Euler over the frame tree (fixed base;
 * revolute / continuous, prismatic and fixed joints; branches; the gravity of gto_set_link_inertials).  The payload of a row
 * is a rigid body on frame_ee: its mass (>= 0 and finite, 0 = none), centre of mass in frame_ee's coordinates (NULL = the
 * frame's origin) and inertia about that centre in frame_ee's axes (NULL = a point mass); payload_mass NULL = no payload,
 * and then the other two must be NULL.  tau_out[., j] is the generalised force of actuated joint j (N m, or N for a
 * prismatic joint), 0 for a joint that no frame names.  FP64 throughout; a row's result depends on the row alone, not on n
 * or its position.  Host pointers, synchronous.
 * Replaces: the `alims` stand-in of gto/utils.py:293-298; RobotModel.rnea, optas/models.py:1735-1888 (which takes revolute
 * chains only). */
int gto_inverse_dynamics(gto_handle* h, int32_t n, const double* q, const double* qd, const double* qdd /*[n,ndof] each*/,
                         const double* payload_mass /*[n] or NULL*/, const double* payload_com /*[n,3] or NULL*/,
                         const double* payload_inertia /*[n,6] or NULL*/, double* tau_out /*[n,ndof]*/);

/* Objective terms of SURVEY.md Appendix A at given trajectories Q [B, ndof, T]:
 * f_goal (min over the goal set), f_obs (incl. w_obstacle), f_vel (incl. w_vel), arg-min goal.
 * (gto/gto_planner.py:84-105, 108-131, 133-135.) */
int gto_eval_objective(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id,
                       const double* goals, const int32_t* n_goals, const double* standoff,
                       const double* base_pos, const double* Q, double* f_goal, double* f_obs,
                       double* f_vel, int32_t* goal_argmin);

/* Gauss-Newton normal equations of the obstacle term at Q [B, ndof, T], per waypoint:
 * JtJ [B, T, n_opt, n_opt], Jtr [B, T, n_opt], sumsq [B, T] (unweighted: residual = cost value). */
int gto_eval_obstacle_normal_eq(gto_handle* h, int32_t B, const int32_t* scene_id,
                                const double* base_pos, const double* Q, double* JtJ, double* Jtr,
                                double* sumsq);

/* Base-placement objective of gto/base_planner.py:57-87 at a given point: y [B][3] = (x, y, theta),
 * q [B][n_max][ndof] one arm configuration per goal (parameter joints of row 0 are used for every goal, as the
 * reference's q/p parameter), goals [B][n_max][16]:  effort_weight |y|^2 + sum_i sum_k |A(q_i) p_k - B(y) RT_i G p_k|^2.
 * Evaluated by the solve kernel itself (a run of gto_solve_base_batch's kernel capped at 0 iterations, started
 * at (y, q)): theta is clipped to [-pi, pi] and q to the joint limits first. */
int gto_eval_base_objective(gto_handle* h, int32_t B, int32_t n_max, const int32_t* n_goals, const double* y,
                            const double* q, const double* goals, double effort_weight, double* cost_out);

/* Seed scoring: compute_plan_cost (gto/gto_models.py:204-215): plain sum of c_obs over all
 * waypoints and surface points, and ||q_0 - q_{T-1}||.  plans [n, ndof, T]. */
int gto_plan_cost(gto_handle* h, int32_t scene_id, int32_t n, const double* plans,
                  const double* base_pos /*[3]*/, double* cost_out /*[n]*/, double* dist_out /*[n]*/);

/*
 * Cost field from a depth image: what the reference's DepthPointCloud does with a KD-tree on
 * the CPU (mesh_to_sdf/depth_point_cloud.py:9-141) to produce sdf_cost_all / sdf_cost_obstacle.  Stand-alone
 * (no handle): uses HIP device `device`.
 *   depth [height*width] float32, row-major; K, Kinv 3x3 row-major (the reference inverts with np.linalg.inv;
 *   pass the same inverse for bit parity); cam_pose, cam_inv 4x4 row-major (camera in the world / its inverse);
 *   target_mask [height*width] or NULL (pixels != 0 are dropped, :41-44); threshold: depth cut-off (:13)
 *   query [nq][3] world points (the voxel centres `workspace_points`, gto/gto_models.py:155-171)
 * Outputs (host; each may be NULL): sdf_out [nq] signed distance to the nearest back-projected point (:56-61),
 * inside_out [nq] = !is_outside (:126-141), cost_out [nq] = get_sdf_cost(query, epsilon, w_inside) (:64-91),
 * points_out [height*width][3] + valid_out [height*width]: the back-projected world points in pixel order.
 * Bit-identical to the reference on tests/golden/depth_cost.npz.
 */
int gto_depth_sdf_cost(int device, const float* depth, int32_t height, int32_t width, const double* K, const double* Kinv,
                       const double* cam_pose, const double* cam_inv, const uint8_t* target_mask, double threshold,
                       const double* query, int64_t nq, float epsilon, float w_inside, float* sdf_out,
                       uint8_t* inside_out, float* cost_out, double* points_out, uint8_t* valid_out);

/*
 * The per-object perception steps of examples/pybullet_gto_planning.py:176-190 in ONE call, leaving a scene resident:
 * depth image -> cloud of all pixels and cloud without the target's pixels (mesh_to_sdf/depth_point_cloud.py:9-53) ->
 * grid = bounding box of the first cloud + margin at grid_res (gto/gto_models.py:155-171; numpy.arange's values) ->
 * sdf_cost_all and sdf_cost_obstacle at the voxel centres (depth_point_cloud.py:64-91; bit-identical to two
 * gto_depth_sdf_cost calls) -> scene `scene_id` of the handle with its voxel records and distance fields.  The image is
 * uploaded once, back-projection and query ordering are shared by the two fields, and nothing but the geometry returns
 * to the host: shape_out [3], origin_out [3], bounds_out [6] = (min x, y, z, max x, y, z) of the first cloud.
 * depth_obstacle [height*width] or NULL: the image of the SECOND cloud (the driver's `depth_obstacle`, :187-189: a copy of
 * the depth image with the target's pixels pushed to the threshold); its points are back-projected from it, without the
 * pixels of target_mask, and its visibility test (depth_point_cloud.py:126-141) reads it.  NULL: the second cloud is
 * `depth` without the masked pixels.  target_mask == NULL and depth_obstacle == NULL: one cloud, sdf_cost_obstacle =
 * sdf_cost_all.
 */
int gto_scene_from_depth(gto_handle* h, int32_t scene_id, const float* depth, int32_t H, int32_t W, const double* K,
                         const double* Kinv, const double* cam_pose, const double* cam_inv, const uint8_t* target_mask,
                         const float* depth_obstacle, double threshold, double grid_res, double margin, float epsilon,
                         float w_inside, int32_t* shape_out, double* origin_out, double* bounds_out);
/*
 * Cost field from a sampled triangle mesh: what the reference's SurfacePointCloud does with a KD-tree on the CPU
 * (mesh_to_sdf/surface_point_cloud.py:16-64, the use_depth_buffer=False branch of get_sdf that
 * mesh_to_sdf(..., surface_point_method='sample') takes, mesh_to_sdf/__init__.py:24-42).  Stand-alone (no handle): uses
 * HIP device `device`.
 *   points, normals [n][3]: surface samples and the normals of their faces; k: the reference's sample_count (11), 1..16
 *   query [nq][3] world points
 * Outputs (host; each may be NULL): sdf_out [nq] float32 distance to the nearest sample, negative where more than half
 * of the k nearest samples see the query behind their face (:46-52); inside_out [nq] that vote; cost_out [nq] the cost
 * map of mesh_to_sdf/depth_point_cloud.py:84-89 of that signed distance; nearest_out [nq] index of the nearest sample.
 * Among samples at equal distance the lower index counts as nearer (the reference leaves ties open).  Bit-identical to
 * the reference on tests/golden/surface_cloud.npz.  GTO_ERR_INVALID_ARG for n < k, k outside 1..16, non-finite samples.
 * Non-finite queries are answered, not refused, and change no other query's result.  A query with a NaN coordinate has
 * no nearest sample: sdf = +inf, inside = 0, cost = 0, nearest = -1.  A query with an infinite coordinate and no NaN is
 * infinitely far from every sample, so (distance, index) order makes samples 0 .. k-1 its k nearest: nearest = 0,
 * |sdf| = inf with the sign of their vote (a dot product that is NaN counts as "in front"), cost = the cost map of that
 * value (+inf inside for w_inside > 0, else 0).  The tree search and the
 * exhaustive search (GTO_CLOUD_BRUTE) agree on both, bit for bit.
 */
int gto_cloud_sdf_cost(int device, const double* points, const double* normals, int64_t n, int32_t k, const double* query,
                       int64_t nq, float epsilon, float w_inside, float* sdf_out, uint8_t* inside_out, float* cost_out,
                       int32_t* nearest_out);

/*
 * gto_scene_from_depth for furniture whose meshes are known: sampled meshes -> grid = bounding box of all samples +
 * margin at grid_res (gto/gto_models.py:155-171; numpy.arange's values) -> sdf_cost_all from all n_all samples and
 * sdf_cost_obstacle from the first n_obstacle of them (the scene without the target object) at the voxel centres
 * (surface_point_cloud.py:32-64 + depth_point_cloud.py:84-89; bit-identical to two gto_cloud_sdf_cost calls) -> scene
 * `scene_id` of the handle with its voxel records and distance fields.  n_obstacle == n_all: one field, used as both.
 * Nothing but the geometry returns to the host: shape_out [3], origin_out [3], bounds_out [6] = (min x, y, z, max x, y, z)
 * of all samples.
 */
int gto_scene_from_clouds(gto_handle* h, int32_t scene_id, const double* points, const double* normals, int64_t n_all,
                          int64_t n_obstacle, int32_t k, double grid_res, double margin, float epsilon, float w_inside,
                          int32_t* shape_out, double* origin_out, double* bounds_out);
/* The two float32 cost fields of a resident scene, device to host (either pointer may be NULL). */
int gto_get_scene_fields(gto_handle* h, int32_t scene_id, float* c_all_out, float* c_obs_out);

/*
 * ---- a resident observation and the collision checks against it -----------------------------------
 * The reference keeps what it observed alive as an object: DepthPointCloud owns its KD-tree
 * (mesh_to_sdf/depth_point_cloud.py:25) and is asked many times -- by the grasp collision filter
 * (examples/pybullet_gto_planning.py:203-221, examples/pybullet_gto_planning_mobile.py:307-322) and by the plan collision
 * statistic (examples/pybullet_evaluate_plans.py:219-233).  A gto_observation is that object on the device: it owns its
 * device memory until gto_observation_destroy, is bound to one HIP device and is independent of any handle or scene.
 * Errors of the calls below that take no handle are read with gto_last_error(NULL).
 *
 * gto_observation_from_depth: arguments and meaning of gto_depth_sdf_cost.  Keeps the image, the camera matrices, the
 * back-projected points and the hierarchy over their 8 x 4 pixel tiles.
 * gto_observation_from_cloud: arguments and meaning of gto_cloud_sdf_cost (k: the sample_count of the vote, 1..16).  Keeps
 * the samples, their normals and the hierarchy over the Morton-sorted samples.
 * Both validate in the order of those entry points (GTO_ERR_INVALID_ARG before GTO_ERR_NO_DEVICE).
 */
typedef struct gto_observation gto_observation;
int gto_observation_from_depth(int device, const float* depth, int32_t height, int32_t width, const double* K,
                               const double* Kinv, const double* cam_pose, const double* cam_inv, const uint8_t* target_mask,
                               double threshold, gto_observation** out);
int gto_observation_from_cloud(int device, const double* points, const double* normals, int64_t n, int32_t k,
                               gto_observation** out);
void gto_observation_destroy(gto_observation* obs);

/*
 * Queries.  Pointer outputs may be NULL; a count of zero items returns GTO_OK without a launch; every item's result is bit
 * for bit the same in any batch and at any position in it.
 *
 * "Inside", the property the checks count, per kind of observation:
 *   depth   !is_outside (mesh_to_sdf/depth_point_cloud.py:127-141): the point projects into the image and is not in front
 *           of the surface seen at its pixel.  No nearest-neighbour search is made.
 *   cloud   more than half of the k nearest samples see the point behind their face (mesh_to_sdf/surface_point_cloud.py:46-52).
 * This equals the reference's `get_sdf < 0` (depth_point_cloud.py:57-62) except for a query that coincides with a cloud
 * point: there the reference yields -0, which is not below zero, and the checks here still count the point.
 *
 * gto_observation_sdf: get_sdf (sdf_out [nq] float32) and !is_outside / the vote (inside_out [nq]) at world points
 * query [nq][3]: the bits of gto_depth_sdf_cost / gto_cloud_sdf_cost on the same inputs (ties to the lower index), with the
 * upload and the build already paid.
 */
int gto_observation_sdf(gto_observation* obs, const double* query, int64_t nq, float* sdf_out, uint8_t* inside_out);
/*
 * The grasp collision filter (pybullet_gto_planning.py:203-221): points [P][3] (the open gripper's surface points in the
 * frame the poses place) at poses [n][16] (row-major 4x4), x = R_i p + t_i in FP64 without contraction, the products of
 * a row added in the order numpy.einsum("nij,pj->npi") adds them ((R_i0 p_0 + R_i2 p_2) + R_i1 p_1, numpy 2.2) before the
 * translation: the bits of utils.grasp_collision_ratio's placed points.  count_out [n]: how many of the P
 * points are inside (the driver rejects count / P > 0.01); -1 for a pose with a non-finite entry, which changes no other
 * count.
 */
int gto_observation_check_posed(gto_observation* obs, const double* points, int32_t P, const double* poses, int32_t n,
                                int32_t* count_out);
/*
 * The plan collision statistic (pybullet_evaluate_plans.py:219-233): plans [B][ndof][T] (T: the handle's horizon).  The
 * world surface points x = visual_tf(q_t) p + base come from the device kinematics behind gto_eval_points and are bit-equal
 * to its xyz_out.  count_out [B][T]: how many of the handle's P surface points are inside at waypoint t of plan b (the
 * evaluator calls a plan colliding when some waypoint has more than 5); -1 for a waypoint (or a base) with a non-finite
 * entry, which changes no other count.  base_pos: HOST array in both variants, [3] (per_plan_base == 0) or [B][3]; zeros
 * reproduce the evaluator's is_mobile branch.  It is free on return in both, pageable or page-locked: the device variant copies
 * per-plan bases through pinned memory of the handle, as gto_solve_base_batch_device copies n_goals (with four such calls of a
 * handle still in flight the host waits for the oldest copy).  `obs` on another device than the handle's: GTO_ERR_INVALID_ARG.
 * gto_check_plans_device: plans and count_out in device memory, enqueued on `stream` (NULL = the handle's stream) without a
 * host synchronisation: it takes the Q_out of gto_solve_batch_device on the same stream as it is.  The per-plan bases and
 * (cloud observation) the world points and votes of a call live in one workspace per handle: calls on one handle go to one
 * stream, or the caller orders them (a handle is not thread-safe, and its calls are not stream-safe against each other).
 * GTO_CLOUD_BRUTE (the exhaustive search of gto_cloud_sdf_cost) holds for the votes of every query above as well.
 */
int gto_check_plans(gto_handle* h, gto_observation* obs, int32_t B, const double* plans, const double* base_pos,
                    int32_t per_plan_base, int32_t* count_out);
int gto_check_plans_device(gto_handle* h, gto_observation* obs, int32_t B, const double* plans, const double* base_pos,
                           int32_t per_plan_base, int32_t* count_out, void* stream);

/*
 * Retiming: B plans [B, ndof, T] (T = the handle's horizon; e.g. the Q_out of gto_solve_batch_device) turned into
 * time-optimal trajectories under per-joint velocity and acceleration limits.
 *   1. path: the not-a-knot cubic spline through the T waypoints on s_k = k/(T-1), every joint
 *      (scipy.interpolate.CubicSpline(ss, Q.T, bc_type="not-a-knot")); p1 = q'(s), p2 = q''(s) on a grid of
 *      N = subdiv (T-1) + 1 points (the knots and subdiv-1 even points inside each interval), N <= 1024;
 *   2. TOPP-RA's discretisation, x = sdot^2, u = sddot, Delta = 1/(N-1): x_i <= min_j (vmax_j/|p1_j|)^2 at every gridpoint
 *      (joints with p1_j = 0 or vmax_j = +inf skipped), -amax_j <= p1_j u_i + p2_j x_i <= amax_j at gridpoints 0..N-2
 *      (where |p1_j| is 0 or so small that amax_j/|p1_j| or p2_j/p1_j overflows: |p2_j x_i| <= amax_j),
 *      x_0 = x_{N-1} = 0, x_{i+1} = x_i + 2 Delta u_i;
 *   3. the controllable sets by a backward pass of exact two-variable LPs, 4. the greedy forward pass (TOPP-RA's:
 *      u_i the largest that keeps x_{i+1} in its controllable set), 5. t_{i+1} = t_i + 2 Delta / (sqrt x_i + sqrt x_{i+1}), constant
 *      acceleration between gridpoints, 6. q, qdot = p1 sdot, qddot = p1 sddot + p2 sdot^2 at linspace(0, duration, M).
 *   vmax [ndof]  > 0, +inf = no limit;  amax [ndof]  finite, > 0.  HOST arrays in both variants (they travel as a kernel
 *                argument): invalid limits, subdiv < 1, M < 2 or N > 1024 fail the whole call with GTO_ERR_INVALID_ARG.
 * Outputs (any may be NULL): duration_out [B], t_grid_out [B, N], sd_grid_out [B, N] (sdot at the gridpoints),
 * q_out / qd_out / qdd_out [B, M, ndof], status_out [B]: GTO_STATUS_CONVERGED, or GTO_STATUS_NUMERICAL for a plan with a
 * non-finite entry (its outputs are NaN; no other plan's output changes), or for a plan whose profile rests over a whole
 * segment: x at both of its ends <= 1e-6 x the plan's largest x (sdot below 1e-3 of its largest), where the segment's
 * time, and so the duration, is decided by round-off (infinite when both are exactly 0).  Such a plan's duration, t_grid
 * and sd_grid are returned as computed, its samples are NaN.  The greedy forward pass is not pointwise maximal where a
 * larger x_i lowers the u_i its segment can take, and that is how a profile can come to rest: at gridpoint N-2 after
 * x_{N-3} reached the edge of its controllable set (19 of 16384 random Panda plans).  A plan whose waypoints are all equal has
 * duration 0 and samples at the waypoint with zero derivatives.  Constant joints (parameter rows of a solved plan) have
 * p1 = p2 = 0, so their limits have no effect.  B = 0 returns GTO_OK without a launch.  Every plan's result is bit for bit
 * the same in any batch.
 * Replaces: convert_plan_to_trajectory_toppra (gto/utils.py:283-323): toppra.SplineInterpolator, JointVelocityConstraint,
 *           JointAccelerationConstraint, TOPPRA(..., parametrizer="ParametrizeConstAccel").compute_trajectory() and the
 *           100 samples of q, qd, qdd (the reference's gridpoints are toppra's adaptive ones; here they are fixed).
 */
int gto_retime_batch(gto_handle* h, int32_t B, const double* plans, const double* vmax, const double* amax, int32_t subdiv,
                     int32_t M, double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out, double* qd_out,
                     double* qdd_out, int32_t* status_out);
/* The same with plans and outputs in device memory, enqueued on `stream` (NULL = the handle's stream; asynchronous except
 * for the first call of a handle, which uploads the spline factors and synchronises).  vmax / amax stay host arrays. */
int gto_retime_batch_device(gto_handle* h, int32_t B, const double* plans, const double* vmax, const double* amax,
                            int32_t subdiv, int32_t M, double* duration_out, double* t_grid_out, double* sd_grid_out,
                            double* q_out, double* qd_out, double* qdd_out, int32_t* status_out, void* stream);

/*
 * The stream-ordered chain from grasp poses to a solved plan (the per-object loop of examples/pybullet_gto_planning.py:
 * 242-294 without a host round trip): gto_solve_ik_pose_batch_device -> gto_ik_report_device -> gto_seed_goalsets_device ->
 * gto_solve_batch_device -> gto_check_plans_device -> gto_retime_batch_device on one stream.  The three entry points below
 * take device pointers and `stream` (NULL = the handle's stream), enqueue and return without a host synchronisation; what
 * they validate are host-side facts only (counts, null pointers, n_max, flags).  Handles with more than eight optimised
 * joints: GTO_ERR_UNSUPPORTED.  B = 0 returns GTO_OK without a launch.  Every instance's result is bit for bit the same in
 * any batch and at any position in it.  Their workspace lives on the handle: calls on one handle go to one stream, or the
 * caller orders them (the rule of gto_check_plans_device).
 *
 * gto_solve_ik_pose_batch_device: the contract of gto_solve_ik_pose_batch with resident arrays (q_out required, the other
 * outputs may be NULL); the same kernel and launch, results bit-equal to the host-pointer call.  base_pos may be NULL only
 * when scene_id is NULL.  Scene ids live on the device and are NOT checked on the host: the kernel takes an id that names
 * no scene of the handle (or a values-only scene) as GTO_STATUS_NUMERICAL with 0 iterations, q_out = the clipped seed and
 * cost_out = NaN.
 */
int gto_solve_ik_pose_batch_device(gto_handle* h, int32_t goal_kind, int32_t B, const int32_t* scene_id, const double* q0,
                                   const double* goals, const double* base_pos, int32_t max_iter, double* q_out,
                                   double* cost_out, int32_t* iters_out, int32_t* status_out, void* stream);
/*
 * What the reference reports of an IK solution (gto/ik_solver.py:88-97) and the driver's acceptance test (:262), for B
 * configurations q [B][ndof] against goal poses goals [B][16] (RT of link_ee, row-major 4x4):
 *   err_pos = |RT[:3,3] - T_ee(q)[:3,3]|
 *   err_rot = degrees(arccos(clip((trace(R_RT^T R_ee) - 1) / 2, -1, 1)))   (= the reference's 2 (q1.q2)^2 - 1)
 *   cost    = plain sum of c_obs at the robot's surface points at q (compute_plan_cost of a one-column plan) with the
 *             instance's scene and base_pos [B][3]; 0 when scene_id is NULL (base_pos may then be NULL).  Order of the sum:
 *             thread i of 256 adds points i, i + 256, ... (the handle's link-sorted order), the 64 partial sums of a wave are
 *             added by its lane-swap tree, then the four waves' sums in wave order ((w0 + w1) + w2) + w3: the order of
 *             gto_plan_cost for one waypoint.  A scene id that names no scene: cost = NaN.
 *   accept  = err_pos < pos_tol && err_rot < rot_tol_deg && cost < cost_tol (uint8 0 / 1); false whenever one of the three
 *             is NaN.
 * T_ee comes from the device kinematics behind gto_eval_fk.  Any output pointer may be NULL.
 */
int gto_ik_report_device(gto_handle* h, int32_t B, const int32_t* scene_id, const double* q, const double* goals,
                         const double* base_pos, double pos_tol, double rot_tol_deg, double cost_tol, double* err_pos_out,
                         double* err_rot_out, double* cost_out, uint8_t* accept_out, void* stream);
/*
 * Accepted goal sets and seeds of B goal-set problems (the driver's :267-269 and GTOPlanner.plan_goalset's seed choice,
 * gto/gto_planner.py:193-219), per instance b:
 *   inputs   scene_id [B], qc [B][ndof], goals [B][n_max][16], n_goals [B] (a value < 1 or > n_max is read as clamped to
 *            [1, n_max]: it lives on the device), q_solutions [B][n_max][ndof] (the IK solution of every goal row),
 *            accept [B][n_max] uint8 or NULL (= every row accepted), base_pos [B][3]
 *   compaction  the accepted goals among rows 0..n_goals[b]-1, in their order, to goals_out [b][0..]; n_goals_out [b] =
 *            n_accepted_out [b] = their count; seed_cost_out / seed_dist_out [b][.] are indexed by compacted position; rows
 *            beyond the count are left untouched.  goals_out must not overlap goals.
 *   candidates  for accepted solution j and waypoint t: Q[:, t] = qc + (q_j - qc) h_t, h_t = s s (3 - 2 s), s = (t + 1) /
 *            (T + 1), in FP64 without fused multiply-adds (gto/utils.py:63-82 for two waypoints); rows of parameter joints
 *            are qc's.  solutions_f32 != 0 rounds q_j to float32 and back first (the driver keeps q_solutions in float32).
 *            They are generated in the scoring kernel: no [B][n][ndof][T] array exists.
 *   score    seed_cost = sum of c_obs over all waypoints and surface points with the instance's scene and base (per waypoint
 *            in the order given at gto_ik_report_device, then the waypoints in order), seed_dist = |Q[:, 0] - Q[:, T-1]|:
 *            bit-equal to gto_plan_cost of the same candidates.  A scene id that names no scene: seed_cost = NaN.
 *   choice   seed_index_out [b] = np.lexsort((dist, cost))[0] over the compacted positions: lowest cost, then lowest
 *            distance, then lowest position; a NaN ranks after every number.  Q0_out [b][ndof][T]: the chosen candidate
 *            (interpolate != 0), or qc for t < T + standoff_offset and the candidate's last column from there on (== 0).
 *   no accepted solution (the q_solutions=None branch)  goals_out [b] = the first n_goals[b] goals unchanged, n_goals_out [b]
 *            = n_goals[b], n_accepted_out [b] = 0, seed_index_out [b] = -1, Q0_out [b] = qc in every column: the instance
 *            stays solvable by gto_solve_batch_device, and n_accepted_out tells the caller that it has no feasible grasp.
 * Any output pointer may be NULL.  goals_out, n_goals_out and Q0_out are what gto_solve_batch_device takes as goals, n_goals
 * and Q0.  n_max and B: at most 65535 each.  GTO_ERR_NO_SCENE when the handle has no scene at all.
 */
int gto_seed_goalsets_device(gto_handle* h, int32_t B, int32_t n_max, const int32_t* scene_id, const double* qc,
                             const double* goals, const int32_t* n_goals, const double* q_solutions, const uint8_t* accept,
                             const double* base_pos, int32_t interpolate, int32_t solutions_f32, double* goals_out,
                             int32_t* n_goals_out, int32_t* n_accepted_out, double* Q0_out, int32_t* seed_index_out,
                             double* seed_cost_out, double* seed_dist_out, void* stream);

/*
 * ---- the stream-ordered base placement loop (examples/pybullet_gto_planning_mobile.py:157-202, gto/base_planner.py:96-168) ---
 * The driver draws grasps, places the base for them, and draws again until the robot's footprint at the new base is free:
 * one host round trip per draw.  Here many draws go in and the first free one comes out: gto_solve_base_batch_device ->
 * gto_base_report_device on one stream, against a resident occupancy grid, with one synchronisation at the end.
 *
 * A gto_occupancy is the x-y occupancy grid of GTORobotModel.setup_occupancy_grid (gto/gto_models.py:218-244) on the device:
 * bound to one HIP device, independent of any handle, owner of its device memory until gto_occupancy_destroy.  Of the points
 * with z > 0.01: xlim = [0, max x], ylim = [min y, max y], axes numpy.arange(lim_lo - margin, lim_hi + margin, resolution); a
 * node is 1 when a point lies within epsilon of it (the reference asks a KD-tree per node), FP64 in numpy's order without
 * contraction: the grid is bit-equal to the reference's (tests/golden/occupancy.npz).  Creation is synchronous.
 * gto_occupancy_from_observation: the back-projected points of a depth observation (invalid and masked pixels left out) or
 * the samples of a cloud observation, without a copy through the host.  gto_occupancy_from_points: host points [n][3].
 * GTO_ERR_INVALID_ARG: null or empty input, non-finite margin / resolution / epsilon, resolution <= 0, epsilon < 0, no point
 * with z > 0.01 (numpy raises there).  GTO_ERR_UNSUPPORTED: a non-finite bound, ceil(epsilon / resolution) > 8, more than
 * 2^26 nodes.  Both validate before any device work (GTO_ERR_INVALID_ARG before GTO_ERR_NO_DEVICE); errors are read with
 * gto_last_error(NULL).
 * gto_occupancy_geometry: origin [2], shape [2] = (nx, ny), xlim [2], ylim [2] (each may be NULL).  gto_occupancy_grid: the
 * grid row-major [nx][ny], 0 or 1, device to host.
 */
typedef struct gto_occupancy gto_occupancy;
int gto_occupancy_from_observation(gto_observation* obs, double margin, double resolution, double epsilon, gto_occupancy** out);
int gto_occupancy_from_points(int device, const double* points, int64_t n, double margin, double resolution, double epsilon,
                              gto_occupancy** out);
int gto_occupancy_geometry(const gto_occupancy* occ, double* origin, int32_t* shape, double* xlim, double* ylim);
int gto_occupancy_grid(gto_occupancy* occ, uint8_t* out);
void gto_occupancy_destroy(gto_occupancy* occ);

/*
 * gto_solve_base_batch with qc, goals and the outputs resident in device memory, enqueued on `stream` (NULL = the handle's
 * stream) without a host synchronisation: the same kernel, grid and LDS, results bit-equal to the host-pointer call.  n_goals
 * [B] stays a HOST array (the rule of base_pos / vmax elsewhere): it is checked as in gto_solve_base_batch and copied in front
 * of the launch on `stream` through pinned memory of the handle; the caller's array is free on return (with four such
 * calls of a handle still in flight the host waits for the oldest copy).  y_out and q_out are required; cost_out, iters_out and
 * status_out may be NULL.  The copy of n_goals lives on the handle: calls on one handle go to one stream, or the caller
 * orders them (the rule of gto_check_plans_device).  An optimised joint that moves none of the gripper's frame is damped by
 * lambda itself and keeps its value of qc, as in gto_solve_base_batch.
 */
int gto_solve_base_batch_device(gto_handle* h, int32_t B, int32_t n_max, const int32_t* n_goals, const double* qc,
                                const double* goals, double effort_weight, int32_t max_iter, double* y_out, double* q_out,
                                double* cost_out, int32_t* iters_out, int32_t* status_out, void* stream);
/*
 * What the reference reports of a base placement (gto/base_planner.py:127-162) and the driver's choice among draws, for B
 * goal sets: qc [B][ndof], goals [B][n_max][16], y [B][3] and q [B][n_max][ndof] as gto_solve_base_batch_device wrote them,
 * all in device memory; n_goals [B] a HOST array as there; enqueued on `stream` without a host synchronisation.
 *   per goal i < n_goals[b]   RT = B(y_b) RT_i G(q_i), B = rt2tr(rotz(theta), [x, y, 0]), G = T_ee(q_i)^-1 T_g(q_i) (the
 *       rigid inverse in closed form):  err_pos_out [b][i] = |RT[:3,3] - T_g(q_i)[:3,3]|,  err_rot_out [b][i] =
 *       degrees(arccos(clip((trace(R_RT^T R_g) - 1) / 2, -1, 1))); kinematics behind gto_eval_fk; rows >= n_goals[b] are left
 *       untouched.
 *   per set   the handle's P surface points at qc_b (gto_eval_points' expression with a zero base) in the new
 *       base frame, x' = c (x - y0) + s (yy - y1), y' = -s (x - y0) + c (yy - y1), c, s = cos, sin theta, FP64 without
 *       contraction; their nodes floor((. - origin) / resolution) clipped per axis (points_to_offsets_occupancy_numpy,
 *       gto/gto_models.py:262-273); collision_out [b] = how many of them are marked = the reference's `cost` (the grid is
 *       0 / 1); -1 when y_b or qc_b has a non-finite entry, which changes no other set's result.
 *   the choice   first_free_out [0] = the lowest b with collision_out [b] == 0, or -1: the driver's `if cost == 0: break`
 *       over the draws in order.
 * Any output may be NULL.  occ may be NULL: then collision_out and first_free_out must be NULL too.  `occ` on another device
 * than the handle's: GTO_ERR_INVALID_ARG.  More than eight optimised joints, n_max outside [1, 32], B > 65535:
 * GTO_ERR_UNSUPPORTED.  B = 0: GTO_OK without a launch.  Every set's result is bit for bit the same in any batch and at any
 * position in it.
 */
int gto_base_report_device(gto_handle* h, gto_occupancy* occ, int32_t B, int32_t n_max, const int32_t* n_goals, const double* qc,
                           const double* goals, const double* y, const double* q, double* err_pos_out, double* err_rot_out,
                           int32_t* collision_out, int32_t* first_free_out, void* stream);

/*
 * ---- several seeds per goal set, and the best of their plans --------------------------------------------------------------
 * GTOPlanner.plan_goalset solves from the one seed np.lexsort((dist, cost))[0] names (gto/gto_planner.py:193-219): a local
 * solver started there finds that seed's optimum.  The three entry points below solve a goal set from its n_seeds best
 * seeds and keep the best plan: gto_seed_goalsets_multi_device -> ONE gto_solve_batch_device over B * n_seeds instances ->
 * gto_plan_report_device -> gto_check_plans_device -> gto_select_plans_device, on one stream.  They are additions (the ABI
 * number stays); they take device pointers and `stream` (NULL = the handle's stream), enqueue without a host
 * synchronisation and validate host-side facts only; their workspace lives on the handle (the rule of
 * gto_check_plans_device); B = 0 returns GTO_OK without a launch; handles with more than eight optimised joints:
 * GTO_ERR_UNSUPPORTED; every object's result is bit for bit the same in any batch and at any position in it.
 *
 * gto_seed_goalsets_multi_device: the inputs, compaction, candidates, scores and order of gto_seed_goalsets_device; the first
 * n_seeds entries of np.lexsort((dist, cost)) over the compacted positions come out (cost, then distance, then position, a
 * NaN after every number), one SLOT each.  n_seeds outside [1, GTO_MAX_SEEDS] or B * n_seeds > 65535: GTO_ERR_UNSUPPORTED
 * (n_seeds is looked at first, before the handle).
 *   goals_out [B][n_seeds][n_max][16], n_goals_out [B][n_seeds]   the instance's compacted goals and their count, written once
 *            per slot: with Q0_out the B * n_seeds slots are goals, n_goals and Q0 of B * n_seeds instances of
 *            gto_solve_batch_device
 *   n_accepted_out [B]; accepted_rows_out [B][n_max] int32: the original row of compacted position j (positions at or
 *            beyond the count are left untouched); seed_cost_out, seed_dist_out [B][n_max] as in gto_seed_goalsets_device
 *   Q0_out [B][n_seeds][ndof][T], seed_index_out [B][n_seeds]
 *       slot r < min(n_seeds, n_accepted)   the r-th ranked candidate, built as gto_seed_goalsets_device builds its chosen one
 *       slot r >= n_accepted >= 1           seed_index_out = -1 and Q0 = slot 0's: the solve is a duplicate, which
 *                                           gto_select_plans_device never prefers (ties go to the lower slot)
 *       no accepted solution                the branch of gto_seed_goalsets_device in every slot
 * Any output may be NULL.  With n_seeds = 1 every output is bit-equal to gto_seed_goalsets_device.
 */
#define GTO_MAX_SEEDS 16
int gto_seed_goalsets_multi_device(gto_handle* h, int32_t B, int32_t n_max, int32_t n_seeds, const int32_t* scene_id,
                                   const double* qc, const double* goals, const int32_t* n_goals, const double* q_solutions,
                                   const uint8_t* accept, const double* base_pos, int32_t interpolate, int32_t solutions_f32,
                                   double* goals_out, int32_t* n_goals_out, int32_t* n_accepted_out, int32_t* accepted_rows_out,
                                   double* Q0_out, int32_t* seed_index_out, double* seed_cost_out, double* seed_dist_out,
                                   void* stream);
/*
 * Which goal a plan reached and how closely: B plans Q [B][ndof][T] against goals [B][n_max][16], n_goals [B] (read as at
 * most n_max) and standoff [B][16] or NULL, in the layout of gto_solve_batch_device.
 *   goal_index_out [b]  the goal whose term of the objective is lowest: the point-matching sum at waypoint T - 1, plus the
 *                       standoff term at waypoint T + standoff_offset when standoff is given (gto/gto_planner.py:86-105);
 *                       the lowest index wins ties: goal_argmin of gto_eval_objective (the same device code)
 *   goal_cost_out [b]   that term's value (f_goal of gto_eval_objective)
 *   err_pos_out, err_rot_out [b]   T_ee(q_{T-1}) against that goal's RT, as gto_ik_report_device reports q_{T-1} against it
 *                       (the same device code: the same bits)
 * A plan with a non-finite entry: goal_index = -1, cost and errors NaN; nobody else's result changes.  Any output may be
 * NULL.
 */
int gto_plan_report_device(gto_handle* h, int32_t B, int32_t n_max, const double* goals, const int32_t* n_goals,
                           const double* standoff, const double* Q, int32_t* goal_index_out, double* goal_cost_out,
                           double* err_pos_out, double* err_rot_out, void* stream);
/*
 * The best of every object's n_seeds plans.  status, cost, err_pos, err_rot [B][n_seeds], counts [B][n_seeds][T] or NULL,
 * Q [B][n_seeds][ndof][T] and dQ [B][n_seeds][ndof][T-1] are what gto_solve_batch_device, gto_plan_report_device and
 * gto_check_plans_device wrote for the B * n_seeds instances.  Per slot:
 *   valid    status != GTO_STATUS_NUMERICAL and cost finite
 *   free     counts is NULL, or every waypoint's count is in [0, max_points] (a count of -1 is not free)
 *   reached  err_pos < pos_tol && err_rot < rot_tol_deg (false on NaN)
 *   class    0 valid, free, reached | 1 valid, free | 2 valid, reached | 3 valid | 4 not valid
 * best_slot_out [B]: the lowest class, then the lowest cost (a NaN after every number), then the lowest slot.  class_out [B]:
 * that slot's class; 0 is a plan the evaluator counts as usable.  Q_out [B][ndof][T], dQ_out [B][ndof][T-1]: copies of the
 * chosen slot's rows.  Any output may be NULL (Q / dQ may then be NULL too).  n_seeds outside [1, GTO_MAX_SEEDS]:
 * GTO_ERR_UNSUPPORTED (looked at first, before the handle).
 */
int gto_select_plans_device(gto_handle* h, int32_t B, int32_t n_seeds, const int32_t* status, const double* cost,
                            const double* err_pos, const double* err_rot, const int32_t* counts, double pos_tol,
                            double rot_tol_deg, int32_t max_points, const double* Q, const double* dQ, int32_t* best_slot_out,
                            int32_t* class_out, double* Q_out, double* dQ_out, void* stream);

/*
 * ---- the grasp collision filter on the stream (the driver's checking stage, examples/pybullet_gto_planning.py:203-236) -------
 * Object poses and object-frame grasps go in; the compacted, base-frame goal sets come out in the layout
 * gto_solve_ik_pose_batch_device (ik_goals_out) and gto_seed_goalsets_device (plan_goals_out as goals, n_grasps_out as n_goals)
 * take; every object is tested against its own observation.  An addition (the ABI number stays).  Enqueued on `stream` (NULL =
 * the handle's stream) without a host synchronisation; what is validated are host-side facts only.  It reads no kinematics and
 * works on every handle, whatever its number of optimised joints.
 *   host arguments (read during the call, free on return)
 *     obs [B]            the observation object b is tested against; entries may repeat, depth and cloud observations may be
 *                        mixed; they must outlive the enqueued work
 *     check_offset [16]  the pose the gripper's points are placed at, relative to the grasp (get_standoff_pose(offset, axis))
 *     ik_offset [16] or NULL   the shelf driver's RT @ standoff for IK (:256-259)
 *   device arguments
 *     points [P][3]      the open gripper's surface points in the frame the poses place
 *     object_pose [B][16], grasps [B][n_max][16] (object frame), n_grasps [B] (a value < 1 or > n_max is read as clamped to
 *     [1, n_max]: it lives on the device), world_to_base [B][16] or NULL (the mobile driver's inv(RT_base)), base_pos [B][3]
 *     or NULL, and every output; any output may be NULL; outputs must not overlap inputs
 *   per object b and row i < n_grasps[b]
 *     G = object_pose_b grasp_bi; with world_to_base G = W_b G (the association order of the mobile driver, :313-343)
 *     C = G check_offset; the P points are placed as x = R p + t of C with gto_observation_check_posed's expression, term for
 *     term (the products added in the order x, z, y, then the translation, without contraction)
 *     count_out [b][i]   how many of the placed points are inside obs[b] ("inside" as for gto_observation_check_posed); -1 when
 *                        object_pose_b, grasp_bi or W_b holds a non-finite entry (or C overflows to one), which changes no
 *                        other row
 *     keep_out [b][i]    count >= 0 && (double)count / (double)P <= max_ratio, the division in FP64: the driver's
 *                        "ratio > 0.01 -> in collision"; with P = 100 and max_ratio = 0.01 one point inside is kept, as in numpy
 *     plan goal          A = G with A[r][3] = G[r][3] - base_pos[b][r], r < 3 (:254); unchanged with base_pos NULL
 *     IK goal            A ik_offset; A with ik_offset NULL
 *     rows >= n_grasps[b] are left untouched in count_out and keep_out
 *   products   every product is the full 4x4 product in FP64 without contraction, entry (r, c) =
 *              ((A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c) + A_r3 B_3c (utils.pose_product restates it; numpy.matmul goes through
 *              BLAS and promises no bits)
 *   compaction the kept rows, in their order, to plan_goals_out [b][0..n_kept) and ik_goals_out [b][0..n_kept), both
 *              [B][n_max][16]; kept_rows_out [b][j] = the original row of position j; positions >= n_kept are left untouched;
 *              n_kept_out [b] = the true count (may be 0), n_grasps_out [b] = max(n_kept, 1).  No row kept: position 0 gets
 *              row 0's two goals and kept_rows_out [b][0] = -1: the object stays solvable by the chain and n_kept_out tells
 *              the caller that it had no collision-free grasp (the driver's `continue`, :236), as n_accepted_out does.
 * Depth observations take one launch over all their objects (each workgroup reads its object's image from a table copied in
 * front of the launch through pinned memory of the handle); every run of consecutive objects that name one cloud observation
 * takes the launch chain of gto_observation_check_posed, at most 2^24 queries at a time.  Every row's and every object's
 * result is bit for bit the same in any batch and at any position in it.
 * GTO_ERR_INVALID_ARG: null handle; B < 0, n_max < 1, P < 1, a non-finite or negative max_ratio; null obs, entry of obs,
 * points, object_pose, grasps, n_grasps or check_offset; a non-finite entry of check_offset / ik_offset; an observation on
 * another device than the handle's.  GTO_ERR_UNSUPPORTED: B or n_max above 65535.  B = 0: GTO_OK without a launch.  The
 * workspace lives on the handle: calls on one handle go to one stream, or the caller orders them (the rule of
 * gto_check_plans_device).
 */
int gto_filter_grasps_device(gto_handle* h, int32_t B, int32_t n_max, gto_observation* const* obs, const double* points,
                             int32_t P, const double* object_pose, const double* grasps, const int32_t* n_grasps,
                             const double* world_to_base, const double* base_pos, const double* check_offset,
                             const double* ik_offset, double max_ratio, int32_t* count_out, uint8_t* keep_out,
                             int32_t* kept_rows_out, int32_t* n_kept_out, int32_t* n_grasps_out, double* plan_goals_out,
                             double* ik_goals_out, void* stream);

/*
 * ---- the motion after the grasp (examples/pybullet_gto_planning.py:301-313) ------------------------------------------------
 * The driver executes the plan, closes the gripper and retrieves the object: on a table it lifts link_ee straight up
 * (env.retract(retract_distance), :307-308; pybullet_scenereplica.py:597-613: fingers closed, ten position-only IK steps,
 * each seeded from the one before), in a shelf it runs the plan's last stretch backwards (:309-313).  compute_reward
 * (:574-589) judges the object after this motion.  Additions (the ABI number stays).  The `_device` entry points take device pointers and `stream`
 * (NULL = the handle's stream), enqueue without a host synchronisation and validate host-side facts only; B = 0 returns
 * GTO_OK without a launch; every plan's result is bit for bit the same in any batch and at any position in it.
 *
 * gto_retrieve_lift_device: a Cartesian straight-line chain of K IK steps per plan in ONE launch (one workgroup per plan
 * runs the whole chain; nothing but the step's column and record is written between steps).  Per plan b:
 *   column 0   plans[b][:, T-1] (T: the handle's horizon) with entry closed_joints[i] replaced by closed_values[i] (the
 *              driver closes the fingers to 0); parameter joints keep these values in every column.  closed_joints: distinct
 *              indices in [0, ndof) (GTO_ERR_INVALID_ARG otherwise); n_closed = 0 with NULL arrays closes nothing.
 *   RT0        link_ee's pose at column 0 from the device kinematics behind gto_eval_fk: the bits gto_eval_fk returns
 *   goal k     k = 1..K: RT0's rotation; translation p0[a] + ((double)k * (distance / K)) * direction[a], in FP64 without
 *              contraction; direction [3] is used as given (not normalised), distance and direction finite
 *   step k     the GTO_IK_GOAL_POINTS problem of gto_solve_ik_pose_batch_device to goal k, seeded from column k - 1: the same
 *              projected Levenberg-Marquardt loop (the same device code), the same max_iter and the same optional collision
 *              term (c_obs of scene scene_id[b] at base_pos[b]; scene_id NULL: no collision term, base_pos may then be NULL).
 *              Column k is its solution.  The chain goes on after a step that misses its goal.
 * The path, its iteration counts and statuses are bit-equal to K calls of gto_solve_ik_pose_batch_device driven from the
 * host with the same goals.
 * DEPARTURE from the reference: pybullet's position-only null-space IK is not available and would let the held object tilt;
 * here the gripper's full pose is held, which is the existing point-matching pose term.
 *   path_out [B][ndof][K+1] (required); goals_out [B][K][16]; iters_out, status_out [B][K];
 *   err_pos_out, err_rot_out [B][K]   column k against goal k with the formulas (and the device code) of gto_ik_report_device
 *   reached_out [B]   the number of leading steps with err_pos < pos_tol, err_rot < rot_tol_deg and a status other than
 *                     GTO_STATUS_NUMERICAL
 * Any output but path_out may be NULL.  1 <= K <= 64 (GTO_ERR_INVALID_ARG otherwise); more than eight optimised joints:
 * GTO_ERR_UNSUPPORTED.  A scene id that names no scene behaves as in gto_solve_ik_pose_batch_device at every step: status
 * GTO_STATUS_NUMERICAL, 0 iterations, the column is the clipped column before it; reached = 0.  A plan whose column 0 holds a
 * non-finite entry: every step GTO_STATUS_NUMERICAL with 0 iterations, every column equals column 0, errors and the goals'
 * first three rows are NaN, reached = 0; no other plan's output changes.
 * gto_retrieve_lift: the same with host arrays (scene ids are checked on the host as in gto_solve_ik_batch; base_pos NULL
 * with scene_id given reads as zeros).
 */
#define GTO_RETRIEVE_MAX_STEPS 64
int gto_retrieve_lift_device(gto_handle* h, int32_t B, const double* plans, const int32_t* scene_id, const double* base_pos,
                             const double* direction /*HOST*/, double distance, int32_t K,
                             const int32_t* closed_joints /*HOST*/, const double* closed_values /*HOST*/, int32_t n_closed,
                             int32_t max_iter, double pos_tol, double rot_tol_deg, double* path_out, double* goals_out,
                             double* err_pos_out, double* err_rot_out, int32_t* iters_out, int32_t* status_out,
                             int32_t* reached_out, void* stream);
int gto_retrieve_lift(gto_handle* h, int32_t B, const double* plans, const int32_t* scene_id, const double* base_pos,
                      const double* direction, double distance, int32_t K, const int32_t* closed_joints,
                      const double* closed_values, int32_t n_closed, int32_t max_iter, double pos_tol, double rot_tol_deg,
                      double* path_out, double* goals_out, double* err_pos_out, double* err_rot_out, int32_t* iters_out,
                      int32_t* status_out, int32_t* reached_out);
/*
 * The shelf branch (:309-313): path_out [B][ndof][n] with n = gto_retrieve_path_columns(h) = 9 - standoff_offset (19 at the
 * defaults): columns T + standoff_offset - 10 .. T - 2 of the plan in reverse order (plan[:, arange(standoff_offset - 10,
 * -1)][:, ::-1]), the rows of closed_joints overwritten with closed_values (HOST arrays, as above).  The plan's last waypoint
 * is NOT part of the path, as the reference leaves it out.  T + standoff_offset - 10 < 0 (a horizon too short for the
 * stretch): GTO_ERR_INVALID_ARG, and gto_retrieve_path_columns returns -1 (also for a null handle).  n_cols_out: HOST, may be
 * NULL; receives n.  Works on every handle, whatever its number of optimised joints.
 */
int gto_retrieve_reverse_device(gto_handle* h, int32_t B, const double* plans, const int32_t* closed_joints,
                                const double* closed_values, int32_t n_closed, double* path_out, int32_t* n_cols_out,
                                void* stream);
int gto_retrieve_path_columns(gto_handle* h);
/*
 * The plan collision statistic on paths of any length: the contract of gto_check_plans / gto_check_plans_device with paths
 * [B][ndof][Tp] and count_out [B][Tp], Tp >= 1 passed explicitly (GTO_ERR_INVALID_ARG otherwise): the same kernels, the same
 * workspace rules.  With Tp = the handle's horizon the two return the same bits.
 */
int gto_check_paths(gto_handle* h, gto_observation* obs, int32_t B, int32_t Tp, const double* paths, const double* base_pos,
                    int32_t per_plan_base, int32_t* count_out);
int gto_check_paths_device(gto_handle* h, gto_observation* obs, int32_t B, int32_t Tp, const double* paths,
                           const double* base_pos, int32_t per_plan_base, int32_t* count_out, void* stream);
/*
 * The grasped object's points in collision along the motion after the grasp.  gto_check_paths counts the ROBOT's surface
 * points; during the retrieve motion the robot carries the object, and the object is usually what meets the neighbour on the
 * table or the shelf board above.  Here a per-plan point set rides rigidly with link_ee from the configuration q_att at which
 * the object was grasped, and count_out [B][Tp] is the number of held points inside the observation at every column.  The
 * reference has no counterpart (its judge is the simulator).  Additions (the ABI number stays).
 *   paths [B][ndof][Tp], base_pos, per_plan_base   as gto_check_paths; Tp >= 1
 *   attach, attach_ld, attach_col   q_att[b][j] = attach[((size_t)b * ndof + j) * attach_ld + attach_col].  attach NULL means
 *                 paths, Tp, column 0: the lift, whose column 0 is the plan's last waypoint.  The reverse mode passes the
 *                 solved plans [B][ndof][T] with attach_ld = T and attach_col = T - 1, because its path leaves the grasp
 *                 column out.  With attach given, attach_col outside [0, attach_ld): GTO_ERR_INVALID_ARG.
 *   held_points [B][P_max][3], n_held [B]   plan b's points are rows 0 .. n_held[b] - 1.  gto_check_held_paths_device: n_held
 *                 lives on the device and a value outside [0, P_max] is read as clamped; gto_check_held_paths: such a value
 *                 gives GTO_ERR_INVALID_ARG.
 *   object_pose [B][16] or NULL   NULL: the points are in the observation's world frame at the moment of the grasp.  Given:
 *                 they are in the object's frame and x = R p + t of object_pose_b with gto_observation_check_posed's
 *                 expression, term for term (the products added in the order x, z, y, then the translation).
 *   labels [H][W] int32 or NULL, held_label [B]   the segmentation image of a depth observation (the camera's mask image; the
 *                 driver builds target_mask = mask == object_id from it) and the label of the object plan b holds.  The depth
 *                 visibility test reads the raw image, which contains the held object: a held point at the grasp column lies
 *                 on or behind the object's own seen surface and would always count as inside.  So for plan b a point that
 *                 projects to a pixel whose label equals held_label[b] counts as outside: what was behind the held object was
 *                 never seen.  labels NULL: no pixel is ignored.  Both are ignored for a cloud observation.  labels given
 *                 with held_label NULL: GTO_ERR_INVALID_ARG (for either kind of observation).
 * Per plan b, held point i and column t, in FP64 without contraction; E_t is link_ee's frame at column t from the device
 * kinematics (the bits gto_eval_fk returns for link_ee, rows R | tr), E_a the same at q_att, base the plan's base:
 *   d[a]   = (x[a] - base[a]) - E_a.tr[a]
 *   p[c]   = (E_a.R[0][c]*d[0] + E_a.R[1][c]*d[1]) + E_a.R[2][c]*d[2]
 *   X_t[r] = (((E_t.R[r][0]*p[0] + E_t.R[r][1]*p[1]) + E_t.R[r][2]*p[2]) + E_t.tr[r]) + base[r]
 * count_out [b][t] = the number of i < n_held[b] with X_t inside obs: "inside" as gto_check_plans defines it for the
 * observation's kind, plus the label rule.  n_held[b] = 0 gives zeros.  -1 for a column with a non-finite entry; -1 for EVERY
 * column of plan b when q_att, the base or (if given) object_pose_b holds a non-finite entry; no other plan's count changes.
 * A held point with a non-finite coordinate is not counted and changes no other point's result (for a cloud observation it
 * goes to the search as a NaN query, which the search reports outside).  Every plan's result is bit for bit the same in any
 * batch and at any position in it, and whatever the number of columns a workgroup takes (GTO_CHECK_TG).
 * Two launches for a depth observation (the attach step once per plan, then one workgroup per plan and column group); a
 * cloud observation takes the launch chain of gto_check_paths at Tp * P_max queries per plan, at most 2^24 queries at a time.
 * GTO_ERR_INVALID_ARG: null handle, observation, base_pos, paths, held_points, n_held or count_out; B < 0, Tp < 1, P_max < 1;
 * an observation on another device than the handle's; the cases above.  GTO_ERR_UNSUPPORTED: B or P_max above 65535.  B = 0:
 * GTO_OK without a launch.  Works on every handle, whatever its number of optimised joints.  The _device variant takes device
 * pointers (base_pos: HOST, as gto_check_paths_device) and enqueues on `stream` (NULL = the handle's) without a host
 * synchronisation; the workspace lives on the handle: calls on one handle go to one stream, or the caller orders them (the
 * rule of gto_check_plans_device).  gto_check_held_paths: the same with host arrays.
 */
int gto_check_held_paths(gto_handle* h, gto_observation* obs, int32_t B, int32_t Tp, const double* paths, const double* attach,
                         int32_t attach_ld, int32_t attach_col, const double* held_points, int32_t P_max,
                         const int32_t* n_held, const double* object_pose, const int32_t* labels, const int32_t* held_label,
                         const double* base_pos, int32_t per_plan_base, int32_t* count_out);
int gto_check_held_paths_device(gto_handle* h, gto_observation* obs, int32_t B, int32_t Tp, const double* paths,
                                const double* attach, int32_t attach_ld, int32_t attach_col, const double* held_points,
                                int32_t P_max, const int32_t* n_held, const double* object_pose, const int32_t* labels,
                                const int32_t* held_label, const double* base_pos /*HOST*/, int32_t per_plan_base,
                                int32_t* count_out, void* stream);
/*
 * Retiming on paths of any length, each with its own column count: the contract of gto_retime_batch /
 * gto_retime_batch_device (above) with paths [B][ndof][Tp], Tp passed explicitly, and these differences.  Additions (the ABI
 * number stays).  Works on every handle, whatever its horizon and its number of optimised joints.
 *   Tp       2 <= Tp and Nmax = subdiv (Tp-1) + 1 <= 1024 (GTO_ERR_INVALID_ARG otherwise).
 *   n_cols   [B] or NULL (every path has Tp columns): path b is columns 0 .. C_b-1 of its row, C_b = n_cols[b]; the other
 *            columns are ignored, non-finite values there included.  Its grid has N_b = subdiv (C_b-1) + 1 points on
 *            s_k = k/(C_b-1).  t_grid_out and sd_grid_out are [B][Nmax]; their entries i >= N_b hold the duration and 0
 *            (the path has ended and rests).  C_b == 1 follows the rule of a plan whose waypoints are all equal: duration 0,
 *            GTO_STATUS_CONVERGED, every sample is the waypoint, derivatives and t_grid are 0.
 *            gto_retime_paths_device: a DEVICE array that no host sees; C_b < 1 or C_b > Tp gives GTO_STATUS_NUMERICAL and NaN
 *            outputs for that path (all Nmax grid entries), and no other path's output changes.
 *            gto_retime_paths: a HOST array; such a count fails the whole call with GTO_ERR_INVALID_ARG before any launch.
 *   spline   scipy.interpolate.CubicSpline(..., bc_type="not-a-knot") for every count: the banded system at C >= 4, the
 *            parabola through the three waypoints at C == 3, the straight line (p2 = 0) at C == 2.
 *   N_b == 2 (C_b == 2 with subdiv == 1) has no gridpoint between its two ends, which both rest (x_0 = x_1 = 0): the one
 *            segment's time is infinite, status GTO_STATUS_NUMERICAL by the rule above.  subdiv >= 2 retimes two columns.
 * Every path's result is bit for bit the same in any batch, at any position in it and under any Tp >= C_b.  With n_cols NULL
 * and Tp = the handle's horizon the outputs are gto_retime_batch's bit for bit: that call is this one with Tp = T.  The
 * spline factors of all counts are one table per handle: the first retime call of a handle uploads it and synchronises, no
 * later call does, whatever its Tp.  vmax / amax: HOST arrays in both variants.
 */
int gto_retime_paths(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols, const double* vmax,
                     const double* amax, int32_t subdiv, int32_t M, double* duration_out, double* t_grid_out,
                     double* sd_grid_out, double* q_out, double* qd_out, double* qdd_out, int32_t* status_out);
int gto_retime_paths_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols /*DEVICE*/,
                            const double* vmax /*HOST*/, const double* amax /*HOST*/, int32_t subdiv, int32_t M,
                            double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out, double* qd_out,
                            double* qdd_out, int32_t* status_out, void* stream);
/*
 * Retiming to the grid's time optimum: the contract of gto_retime_paths / gto_retime_paths_device with steps 3 and 4 (the
 * controllable sets and the greedy forward pass, which is not pointwise maximal on a fixed grid and can bring a profile to
 * rest) replaced by a convex program per path.  Additions (the ABI number stays).  For path b with N = subdiv (C_b-1) + 1
 * gridpoints, Delta = 1/(N-1), variables x_1 .. x_{N-2} and x_0 = x_{N-1} = 0:
 *     minimise    T(x) = sum_{i=0}^{N-2} 2 Delta / (sqrt x_i + sqrt x_{i+1})        (convex in x)
 *     subject to  0 <= x_i <= xcap_i, xcap_i the bound of step 2 that does not involve u, and for every gridpoint
 *                 i <= N-2 and every moving joint j whose amax_j/|p1_j| and p2_j/p1_j are finite there (its line),
 *                 -alpha + beta x_i <= (x_{i+1} - x_i)(N-1)/2 <= alpha + beta x_i,  alpha = amax_j/|p1_j|, beta = -p2_j/p1_j
 * (exactly the constraints of steps 1 and 2; a joint without a line is in xcap_i).  The profile returned is a feasible x
 * with T(x) <= (1 + gap_tol) T*, T* the optimum, found by a log-barrier path-following Newton method that stops when its
 * bound on T(x) - T* falls to gap_tol T(x).  Steps 5 and 6 follow unchanged on this x.
 *   gap_tol     finite, > 0 (GTO_ERR_INVALID_ARG otherwise); 1e-8 is the Python layers' default.
 *   max_newton  >= 1 (GTO_ERR_INVALID_ARG otherwise): the cap on Newton steps per path.
 *   iters_out   [B] or NULL: Newton steps taken (0 for a path that needs no solve).
 *   status_out  GTO_STATUS_CONVERGED: the gap is certified.  GTO_STATUS_MAX_ITER: the cap was hit; the profile is still
 *               feasible (every iterate is strictly inside) and its times and samples are valid, the gap is not certified.
 *               GTO_STATUS_NUMERICAL: a non-finite entry or a wild count (NaN outputs), N_b == 2 (no variable: both ends
 *               rest, duration inf, NaN samples, as in gto_retime_paths), or a non-finite iterate (NaN outputs).
 * The rule for a profile that rests over a whole segment is not applied: resting costs infinite time, so an optimal
 * profile does not.  Everything else is gto_retime_paths': the argument checks, HOST vmax / amax, n_cols HOST
 * (gto_retime_paths_convex) or DEVICE with the wild-count rule (gto_retime_paths_convex_device), the fill past a path's own
 * gridpoints, C_b == 1 and all-equal waypoints (duration 0, no solve), results bit for bit the same in any batch, at any
 * position in it and under any Tp >= C_b, the one factor table per handle (shared with the other retime calls), stream order
 * with no synchronisation after a handle's first retime call.  The greedy entry points are unchanged and share the
 * workspace: calls on one handle go to one stream, or the caller orders them.
 */
int gto_retime_paths_convex(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols,
                            const double* vmax, const double* amax, int32_t subdiv, int32_t M, double gap_tol,
                            int32_t max_newton, double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out,
                            double* qd_out, double* qdd_out, int32_t* status_out, int32_t* iters_out);
int gto_retime_paths_convex_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols /*DEVICE*/,
                                   const double* vmax /*HOST*/, const double* amax /*HOST*/, int32_t subdiv, int32_t M,
                                   double gap_tol, int32_t max_newton, double* duration_out, double* t_grid_out,
                                   double* sd_grid_out, double* q_out, double* qd_out, double* qdd_out, int32_t* status_out,
                                   int32_t* iters_out, void* stream);
/*
 * Retiming under joint torque limits with the held object as payload: the program of gto_retime_paths_convex kept whole
 * (variables, objective, xcap, acceleration lines, certificate, statuses) plus, for every gridpoint i <= N-2 and every
 * joint j with a finite tau_max_j,
 *     -tau_max_j <= a_ij c (x_{i+1} - x_i) + b_ij x_i + g_ij <= tau_max_j,        c = (N-1)/2,
 *     g_i = ID(q_i, 0, 0),   a_i = ID(q_i, 0, p1_i) - g_i,   b_i = ID(q_i, p1_i, p2_i) - g_i,
 * ID the inverse dynamics of gto_inverse_dynamics with the path's payload on frame_ee, q_i / p1_i / p2_i the spline's value
 * and derivatives at the gridpoint (p1 = p2 = 0 on a joint that does not move): the generalised force along the path is
 * a u + b x + g exactly.  The rows stand for EVERY joint a frame names, moving or not (a joint that stands still must still
 * hold); a row whose coefficients on x_1 .. x_{N-2} are both zero is left out.  Additions (the ABI number stays).
 *   tau_max          [ndof] HOST: > 0, +inf = no limit (GTO_ERR_INVALID_ARG for a NaN or an entry <= 0).
 *   payload_*        [B], [B,3], [B,6] or NULL, one rigid body per path: the payload rules of gto_inverse_dynamics.
 *                    gto_retime_paths_torque (HOST) refuses a mass that is negative or not finite, and com / inertia
 *                    without a mass; gto_retime_paths_torque_device reads DEVICE arrays that no host sees.
 *   tau_out          [B,M,ndof] or NULL: ID(q, qd, qdd) at the M samples with the path's payload, bit for bit what
 *                    gto_inverse_dynamics gives on those rows; NaN where the samples are NaN.
 *   status_out       those of gto_retime_paths_convex, and GTO_STATUS_INFEASIBLE: a path with finite entries (moving or
 *                    not, C_b == 1 included) with |g_ij| >= tau_max_j at some gridpoint 0 .. N-1 (the last one too: the
 *                    robot holds there) -- x = eps 1 is strictly inside for small eps exactly when there is none.  NaN
 *                    outputs and 0 iterations, as for GTO_STATUS_NUMERICAL; no other path's output changes.  A path with
 *                    a non-finite a, b or g is GTO_STATUS_NUMERICAL (a payload on the device with a NaN in it, or a mass
 *                    that is negative or not finite).
 * A handle without inertials answers GTO_ERR_INVALID_ARG "no link inertials set".  Everything else is
 * gto_retime_paths_convex's: the argument checks (under this call's name), HOST vmax / amax, the n_cols rules, the fill past
 * a path's own gridpoints, results bit for bit the same in any batch and at any position (the payload travels with its
 * path), the shared workspace and factor table, stream order with no synchronisation after a handle's first retime call.
 * The greedy and convex entry points are unchanged, launch for launch.
 * Replaces: the `alims` stand-in of gto/utils.py:293-298 (0.5 rad/s^2 for what a motor can do).
 */
int gto_retime_paths_torque(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols,
                            const double* vmax, const double* amax, const double* tau_max /*[ndof] HOST: > 0, +inf = none*/,
                            const double* payload_mass /*[B] or NULL*/, const double* payload_com /*[B,3] or NULL*/,
                            const double* payload_inertia /*[B,6] or NULL*/, int32_t subdiv, int32_t M, double gap_tol,
                            int32_t max_newton, double* duration_out, double* t_grid_out, double* sd_grid_out, double* q_out,
                            double* qd_out, double* qdd_out, double* tau_out /*[B,M,ndof] or NULL*/, int32_t* status_out,
                            int32_t* iters_out);
int gto_retime_paths_torque_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const int32_t* n_cols /*DEVICE*/,
                                   const double* vmax /*HOST*/, const double* amax /*HOST*/, const double* tau_max /*HOST*/,
                                   const double* payload_mass /*DEVICE*/, const double* payload_com /*DEVICE*/,
                                   const double* payload_inertia /*DEVICE*/, int32_t subdiv, int32_t M, double gap_tol,
                                   int32_t max_newton, double* duration_out, double* t_grid_out, double* sd_grid_out,
                                   double* q_out, double* qd_out, double* qdd_out, double* tau_out, int32_t* status_out,
                                   int32_t* iters_out, void* stream);

/* ---- forward dynamics and the tracking rollout.  Additions (the ABI number stays). ------------------------------------- */

/* Forward dynamics of n rows: the accelerations qdd that the joint forces tau cause at the state (q, qd), with the payload
 * rules of gto_inverse_dynamics (ID below).  A joint is FREE when some actuated frame names it and `locked` does not mark
 * it; locked == NULL locks every joint that is not one of the handle's optimised joints (the parameter joints: Panda's
 * fingers, Fetch's torso and head), and a joint no frame names is always locked.  Locked joints get qdd = 0: a constraint
 * force holds them, and it is not reported.  On the free joints M_ff qdd_f = (tau - c)_f is solved by a Cholesky
 * factorisation in FP64, with c = ID(q, qd, 0) and the mass matrix from M e_j = ID(q, 0, e_j) - ID(q, 0, 0), symmetrised
 * (M_ij <- (M_ij + M_ji) / 2) before it is factored, the free joints in ascending order.
 *   locked      [ndof] HOST or NULL: non-zero = locked.
 *   M_out       [n, ndof, ndof] or NULL: the symmetrised mass matrix, exactly symmetric; the columns of locked joints that a
 *               frame names included, zero rows and columns for joints no frame names.
 *   status_out  [n] or NULL: GTO_STATUS_CONVERGED, or GTO_STATUS_NUMERICAL for a row with a non-finite entry in q, qd or
 *               tau, a pivot <= 0 (a free joint that moves no mass) or a non-finite solution: that row of qdd_out and of
 *               M_out is NaN, and no other row changes.
 * A handle without inertials answers GTO_ERR_INVALID_ARG "no link inertials set"; n < 0, a null q / qd / tau / qdd_out, a
 * payload mass that is negative or not finite, com / inertia without a mass: GTO_ERR_INVALID_ARG before any launch; n = 0:
 * GTO_OK.  A row's result depends on the row alone, bit for bit, at any n and position.  Host pointers, synchronous.
 * Replaces: the simulated robot behind env.robot.execute_plan (examples/pybullet_gto_planning.py:301,313), together with
 * gto_track_rollout. */
int gto_forward_dynamics(gto_handle* h, int32_t n, const double* q, const double* qd, const double* tau /*[n,ndof] each*/,
                         const double* payload_mass /*[n] or NULL*/, const double* payload_com /*[n,3] or NULL*/,
                         const double* payload_inertia /*[n,6] or NULL*/, const int32_t* locked /*[ndof] HOST or NULL*/,
                         double* qdd_out /*[n,ndof]*/, double* M_out /*[n,ndof,ndof] or NULL*/,
                         int32_t* status_out /*[n] or NULL*/);

/*
 * Roll B retimed trajectories forward under a torque-limited joint controller.  The reference of path b is what every
 * retime entry point returns: duration[b] and the samples q_ref, qd_ref, qdd_ref [B, M, ndof] at linspace(0, duration, M),
 * M >= 2.  Between samples q_ref(t) is the cubic Hermite interpolant of (q_m, qd_m), qd_ref(t) its derivative and
 * qdd_ref(t) linear between the qdd_m; from t = duration on (at once when duration = 0) it is the last sample with zero
 * derivatives, for `settle` more seconds.  The controller is evaluated once per control period dt, at the period's start
 * t = k dt, and its torque is held over the period:
 *     tau = clip( ff(t) + kp o (q_ref - q) + kd o (qd_ref - qd), +-tau_max ),
 * ff = 0 (feedforward = 0), ID_model(q_ref, 0, 0) (1) or ID_model(q_ref, qd_ref, qdd_ref) (2).  The plant integrates
 * qdd = FD_plant(q, qd, tau) over the period with one classical RK4 step.  ID_model and FD_plant are gto_inverse_dynamics
 * and gto_forward_dynamics on the handle's inertials with two SEPARATE payloads per path: model_payload_* is what the
 * controller believes, plant_payload_* what the hand really holds (each [B], [B,3], [B,6] or NULL, the payload rules of
 * gto_inverse_dynamics).  The start state is q_ref[0], and qd_ref[0] on the free joints.  Locked joints (the `locked`
 * rule of gto_forward_dynamics) stand at q_ref[0] with zero velocity for the whole rollout, in the plant and in the
 * feedforward alike; whatever else the reference says about them is ignored, and they are left out of every error
 * measure.  Joint limits are not enforced and there is no contact model.  K_b = ceil((duration_b + settle) / dt) steps,
 * 1 <= K_b <= 2^20.
 *   kp, kd      [ndof] HOST: finite, >= 0.       tau_max  [ndof] HOST: > 0, +inf = no limit.
 *   dt > 0, settle >= 0, both finite; feedforward in {0, 1, 2}; M >= 2; Mo >= 2.  Anything else, a handle without inertials
 *   ("no link inertials set"), a null reference array, com / inertia without a mass and (gto_track_rollout, HOST arrays) a
 *   payload mass that is negative or not finite: GTO_ERR_INVALID_ARG before any launch.  B = 0: GTO_OK without one.
 * Outputs, any of which may be NULL:
 *   q_out, qd_out [B, Mo, ndof], t_out [B, Mo]: sample m is the state after step k_m = floor(m K_b / (Mo - 1)) (integer
 *               arithmetic), t = k_m dt; nothing is interpolated.  Sample 0 is the start state, sample Mo - 1 the last.
 *   err_max     [B] the largest |q - q_ref| over the steps and the free joints, measured at the period ends.
 *   err_end     [B] the same at the last step.
 *   sat_steps   [B] the periods in which the clip changed a free joint's torque.
 *   steps       [B] K_b.
 *   status_out  [B] GTO_STATUS_CONVERGED, or GTO_STATUS_NUMERICAL: a duration that is negative or not finite, a non-finite
 *               sample of a free joint (or first position of a locked one), K_b out of range, a payload mass on the device
 *               that is negative or not finite, a pivot <= 0, or a state that stops being finite.  Every output of that
 *               path is NaN then, sat_steps and steps are 0, and no other path changes.
 * gto_track_rollout takes HOST arrays and is synchronous.  gto_track_rollout_device: every per-path array (duration, the
 * samples, the payloads, the outputs) is in DEVICE memory and unseen by the host; kp, kd, tau_max and locked are HOST
 * arrays that travel as kernel arguments; one launch enqueued on `stream` (NULL = the handle's) with no allocation and no
 * synchronisation at all.  Its results are bit for bit the host variant's, and every path's result is bit for bit the same
 * in any batch and at any position in it.
 */
int gto_track_rollout(gto_handle* h, int32_t B, int32_t M, const double* duration /*[B]*/, const double* q_ref,
                      const double* qd_ref, const double* qdd_ref /*[B,M,ndof] each*/, const double* kp, const double* kd,
                      const double* tau_max /*[ndof] HOST each*/, double dt, double settle, int32_t feedforward,
                      const double* model_payload_mass, const double* model_payload_com, const double* model_payload_inertia,
                      const double* plant_payload_mass, const double* plant_payload_com, const double* plant_payload_inertia,
                      const int32_t* locked /*[ndof] HOST or NULL*/, int32_t Mo, double* q_out, double* qd_out /*[B,Mo,ndof]*/,
                      double* t_out /*[B,Mo]*/, double* err_max, double* err_end /*[B]*/, int32_t* sat_steps, int32_t* steps,
                      int32_t* status_out /*[B]*/);
int gto_track_rollout_device(gto_handle* h, int32_t B, int32_t M, const double* duration /*DEVICE*/, const double* q_ref,
                             const double* qd_ref, const double* qdd_ref /*DEVICE*/, const double* kp, const double* kd,
                             const double* tau_max /*HOST*/, double dt, double settle, int32_t feedforward,
                             const double* model_payload_mass, const double* model_payload_com,
                             const double* model_payload_inertia, const double* plant_payload_mass,
                             const double* plant_payload_com, const double* plant_payload_inertia /*DEVICE*/,
                             const int32_t* locked /*HOST*/, int32_t Mo, double* q_out, double* qd_out, double* t_out,
                             double* err_max, double* err_end, int32_t* sat_steps, int32_t* steps, int32_t* status_out,
                             void* stream);
/*
 * The robot's clearance from itself along a path.  Every other check judges a plan against the scene; the solver has no
 * self-collision term and neither has the reference, where a plan that folds the arm into itself shows only when PyBullet
 * executes it (examples/pybullet_gto_planning.py:301): these replace nothing there.  Additions (the ABI number stays).
 * For a column q_t of a path, the handle's pair mask M (symmetric, zero diagonal) and a cutoff c in metres (+inf allowed):
 *   d2(t) = min over points p of link a, p' of link b, a < b, M[a][b] set, of |X_p(q_t) - X_p'(q_t)|^2
 * X is gto_eval_points' world point at base 0 (the base cancels), bit for bit, and the squared distance is
 * (dx*dx + dy*dy) + dz*dz in FP64 without contraction: squared metres on purpose, a pure function of products and sums.
 *   d2_out   [B][Tp]     min(d2, c*c)
 *   pair_out [B][Tp][2]  the closest link pair (a, b), a < b; of two pairs at the same d2 the lexicographically smaller;
 *                        (-1, -1) when nothing is closer than the cutoff or no pair is enabled (d2_out is c*c then)
 * A column with a non-finite entry gives d2_out = NaN and pair_out = (-1, -1) and changes no other column.  Every column's
 * result is bit for bit the same in any batch, at any position, whatever the cutoff culls and whatever the number of
 * columns a workgroup takes (GTO_CHECK_TG): the sphere tests only ever drop pairs that are strictly farther than the answer.
 *   gto_set_self_pairs   rows [n_links] HOST: bit b of rows[a] enables the pair (a, b) (the 32 bits of an unsigned word; the
 *                        header types it int32_t).  GTO_ERR_INVALID_ARG, before any device call and with the handle's mask
 *                        unchanged, for a bit at or above n_links, a set diagonal bit or an asymmetric mask.  NULL: back to
 *                        the mask a new handle has, every pair of distinct links.  Calls already enqueued keep their mask.
 *   paths [B][ndof][Tp], Tp >= 1, as gto_check_paths takes them.  B = 0: GTO_OK without a launch.  Tp < 1, B < 0, a NaN or
 *   non-positive cutoff, a null array: GTO_ERR_INVALID_ARG before any device call.  Works on every handle, whatever its T.
 * gto_self_clearance takes HOST arrays and is synchronous.  gto_self_clearance_device takes DEVICE arrays: one launch on
 * `stream` (NULL = the handle's), no synchronisation, no allocation, no workspace on the handle.
 */
int gto_set_self_pairs(gto_handle* h, const int32_t* rows /*[n_links] HOST*/);
int gto_self_clearance(gto_handle* h, int32_t B, int32_t Tp, const double* paths, double cutoff, double* d2_out,
                       int32_t* pair_out);
int gto_self_clearance_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, double cutoff, double* d2_out,
                              int32_t* pair_out, void* stream);
/*
 * The held object's clearance from the robot's own links along a path.  gto_check_held_paths judges the object's points
 * against the observation and gto_self_clearance the robot's links against each other (the handle's links: the object's
 * points are not robot points); these judge the pair that is left, the object against the arm that carries it.  Nothing in
 * the reference does: a box driven into the forearm shows there when PyBullet executes the plan
 * (examples/pybullet_gto_planning.py:301).  Additions (the ABI number stays).
 * paths, attach, attach_ld, attach_col, held_points, P_max, n_held, object_pose, base_pos and per_plan_base mean exactly
 * what they mean for gto_check_held_paths[_device], with the same limits (65535 plans of 65535 points: GTO_ERR_UNSUPPORTED
 * beyond), the same clamping of a device-resident n_held to [0, P_max] and the same error codes; there is no observation,
 * no labels and no held_label.  For plan b, column t, the link mask m and a cutoff c in metres (+inf allowed), in FP64
 * without contraction:
 *   p        the held point in link_ee's frame at the grasp configuration: the attach step of gto_check_held_paths, term
 *            for term (d[a] = (x[a] - base[a]) - E_a.tr[a]; p[c] = (E_a.R[0][c]*d[0] + E_a.R[1][c]*d[1]) + E_a.R[2][c]*d[2])
 *   Y_t[r] = ((E_t.R[r][0]*p[0] + E_t.R[r][1]*p[1]) + E_t.R[r][2]*p[2]) + E_t.tr[r]
 *            that header's X_t without the final + base: the base cancels against the robot's points
 *   X_p'     gto_eval_points' world point of robot surface point p' at base 0, bit for bit
 *   d2(b,t) = min over held points i < n_held[b] with finite coordinates and robot points p' of the links l with bit l of m
 *            set, of (dx*dx + dy*dy) + dz*dz, d = Y_t,i - X_p'
 *   d2_out    [B][Tp]  min(d2, c*c)
 *   link_out  [B][Tp]  the collision link l and
 *   point_out [B][Tp]  the held point i that attain the minimum; of several at the same d2 the lexicographically smallest
 *                      (l, i); both -1 when nothing is closer than the cutoff.  Either may be NULL.
 * n_held[b] = 0, an empty mask, or enabled links without points: c*c and -1.  A column with a non-finite entry: NaN and -1,
 * and no other column changes.  Every column of a plan whose q_att, base or object pose holds a non-finite entry: NaN and
 * -1.  A held point with a non-finite coordinate is skipped and changes no other point's result.  Every column's result is
 * bit for bit the same in any batch, at any position, whatever the cutoff culls and whatever the number of columns a
 * workgroup takes (GTO_CHECK_TG): the sphere tests only ever drop (held point, chunk) pairs that are strictly farther than
 * the answer.  Works on every handle, whatever its number of optimised joints or its T.
 *   link_mask  bit l enables collision link l of the handle (the 32 bits of an unsigned word; the header types it int32_t,
 *              as gto_set_self_pairs' rows).  0 is legal: everything is far.  RobotDesc.held_links builds the planners' mask.
 *   GTO_ERR_INVALID_ARG before any device call: a mask bit at or above n_links, a NaN or non-positive cutoff, B < 0, Tp < 1,
 *   P_max < 1, attach_col outside [0, attach_ld), a null paths, held_points, n_held, base_pos or d2_out; the host variant
 *   also for an n_held outside [0, P_max].  B = 0: GTO_OK without a launch.
 * gto_held_clearance takes HOST arrays and is synchronous.  gto_held_clearance_device takes DEVICE arrays (base_pos HOST,
 * free on return): two launches on `stream` (NULL = the handle's), the attach step and the clearance kernel, with no
 * synchronisation and no allocation once the handle's workspace has grown to the call's size.  The attach step's workspace
 * is the one gto_check_held_paths_device uses: calls that share a handle go to one stream.
 */
int gto_held_clearance(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const double* attach, int32_t attach_ld,
                       int32_t attach_col, const double* held_points, int32_t P_max, const int32_t* n_held,
                       const double* object_pose, const double* base_pos, int32_t per_plan_base, int32_t link_mask,
                       double cutoff, double* d2_out, int32_t* link_out, int32_t* point_out);
int gto_held_clearance_device(gto_handle* h, int32_t B, int32_t Tp, const double* paths, const double* attach,
                              int32_t attach_ld, int32_t attach_col, const double* held_points, int32_t P_max,
                              const int32_t* n_held, const double* object_pose, const double* base_pos /*HOST*/,
                              int32_t per_plan_base, int32_t link_mask, double cutoff, double* d2_out, int32_t* link_out,
                              int32_t* point_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GTO_SOLVER_H */
