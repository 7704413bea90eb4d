// gto_seed.h — the stream-ordered steps between inverse kinematics and the trajectory solve (gfx950):
//   k_ik_report    what the reference reports of an IK solution (gto/ik_solver.py:88-97) and the driver's acceptance test
//                  (examples/pybullet_gto_planning.py:262), one workgroup per instance
//   k_seed_score   obstacle cost of the seed candidate of every accepted IK solution (gto/gto_planner.py:197-211), the
//                  candidates generated in the kernel; kinematics and sums are k_plan_cost's (plan_cost_kinematics,
//                  plan_cost_gather in gto_kernels.h)
//   k_seed_select  compaction of the accepted goals (:267-269 of the driver), np.lexsort((dist, cost))[0] and the seed of
//                  the trajectory solve (gto/gto_planner.py:212-219), one wave per instance; k_seed_select_ranked: the first
//                  n_seeds entries of that order, one solve instance each
//   k_plan_report  which goal a solved plan reached (the objective's arg-min goal) and how closely, one workgroup per plan
//   k_select_plans the class of every seed's plan (reached, collision-free, valid) and the best of an object's plans
#pragma once
#include "gto_kernels.h"

// a scene id that names a set scene with a c_obs field (all these kernels read)
__device__ __forceinline__ bool seed_scene_ok(const SceneDev* __restrict__ scenes, int n_scenes, int sid) {
  return (unsigned)sid < (unsigned)n_scenes && scenes[sid].valid && scenes[sid].c_obs;
}

// What the report kernels say of a frame against a goal pose g [16] (gto/ik_solver.py:88-97): Xg holds the transposed frames
// plan_cost_kinematics left in LDS
__device__ __forceinline__ void seed_pose_errors(const double* __restrict__ Xg, int frame, const double* __restrict__ g,
                                                 double* err_pos, double* err_rot) {
  double E[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) E[e] = Xg[fkx(frame, 4 * (e & 3) + (e >> 2))];
  const double d0 = g[3] - E[3], d1 = g[7] - E[7], d2 = g[11] - E[11];
  *err_pos = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) tr += g[4 * i + j] * E[4 * i + j];
  double c = (tr - 1.0) / 2.0;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);  // (a NaN stays one, as in np.clip)
  *err_rot = acos(c) * (180.0 / M_PI);
}

__global__ __launch_bounds__(256) void k_ik_report(const RobotDev* __restrict__ rb, const double* __restrict__ px,
                                                   const double* __restrict__ py, const double* __restrict__ pz,
                                                   const int32_t* __restrict__ plink, const SceneDev* __restrict__ scenes,
                                                   int n_scenes, const int32_t* __restrict__ scene_id,
                                                   const double* __restrict__ q, const double* __restrict__ goals,
                                                   const double* __restrict__ base_pos, double pos_tol, double rot_tol_deg,
                                                   double cost_tol, double* __restrict__ err_pos_out,
                                                   double* __restrict__ err_rot_out, double* __restrict__ cost_out,
                                                   uint8_t* __restrict__ accept_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int F = rb->n_frames, ndof = rb->ndof;
  extern __shared__ __attribute__((aligned(16))) double smem_rep[];
  const PlanCostLds m = plan_cost_lds<1>(rb, smem_rep);
  plan_cost_kinematics<1>(rb, m, 1, tid, [&](int, int dq) { return q[(size_t)b * ndof + dq]; });
  double cost = 0.0;
  if (scene_id) {  // (block-uniform: the barrier inside plan_cost_gather is met by all or by none)
    const int sid = scene_id[b];
    if (seed_scene_ok(scenes, n_scenes, sid)) {
      const SceneDev sc = scenes[sid];
      cost = plan_cost_gather<1>(rb, px, py, pz, plink, sc, base_pos[3 * b], base_pos[3 * b + 1], base_pos[3 * b + 2], m, 1, tid);
    } else {
      cost = NAN;
    }
  }
  if (tid != 0) return;
  double err_pos, err_rot;
  seed_pose_errors(m.X + (rb->fk_rounds & 1) * 16 * F /* X_f = G_f^T */, rb->frame_ee, goals + (size_t)b * 16, &err_pos, &err_rot);
  if (err_pos_out) err_pos_out[b] = err_pos;
  if (err_rot_out) err_rot_out[b] = err_rot;
  if (cost_out) cost_out[b] = cost;
  if (accept_out) accept_out[b] = (err_pos < pos_tol && err_rot < rot_tol_deg && cost < cost_tol) ? 1 : 0;
}

// n_goals[b] as every kernel here reads it
__device__ __forceinline__ int seed_goal_count(const int32_t* __restrict__ n_goals, int b, int n_max) {
  return min(max(n_goals[b], 1), n_max);
}

// Joint dq at waypoint t of the seed candidate towards the IK solution qs (gto/gto_planner.py:197-206, gto/utils.py:63-82
// for two waypoints): qc + (q - qc) h_t, h_t = s s (3 - 2 s), s = (t + 1) / (T + 1); a parameter joint keeps qc's value.
// Products and sums stay apart (no fused multiply-add): these are the bits of synthetic.interpolate_waypoints.
__device__ __forceinline__ double seed_joint(const RobotDev* __restrict__ rb, const double* __restrict__ qc,
                                             const double* __restrict__ qs, int dq, int t, int T, int f32) {
#pragma clang fp contract(off)
  const double c = qc[dq];
  if (rb->opt_of_dof[dq] < 0) return c;
  double qj = qs[dq];
  if (f32) qj = (double)(float)qj;
  const double s = (double)(t + 1) / (double)(T + 1);
  const double hh = s * s * (3.0 - 2.0 * s);
  return c + (qj - c) * hh;
}

// numpy's order of floating-point keys: a NaN after every number, NaNs equal among themselves
__device__ __forceinline__ bool seed_key_less(double a, double b) { return a < b || (b != b && a == a); }
// candidate (c1, d1, p1) comes before (c2, d2, p2) in np.lexsort((dist, cost)): cost, then distance, then position
__device__ __forceinline__ bool seed_before(double c1, double d1, int p1, double c2, double d2, int p2) {
  if (seed_key_less(c1, c2)) return true;
  if (seed_key_less(c2, c1)) return false;
  if (seed_key_less(d1, d2)) return true;
  if (seed_key_less(d2, d1)) return false;
  return p1 < p2;
}

// Grid (groups of four waypoints, compacted position j, instance b).  Wave 0 finds the row of the j-th accepted solution
// of the instance (a workgroup without one leaves at once); then the four waypoints of its candidate are generated,
// posed and summed as k_plan_cost does for a stored plan: partial[b][j][t] holds the same bits.
__global__ __launch_bounds__(256) void k_seed_score(const RobotDev* __restrict__ rb, const double* __restrict__ px,
                                                    const double* __restrict__ py, const double* __restrict__ pz,
                                                    const int32_t* __restrict__ plink, const SceneDev* __restrict__ scenes,
                                                    int n_scenes, const int32_t* __restrict__ scene_id,
                                                    const double* __restrict__ qc, const int32_t* __restrict__ n_goals,
                                                    const double* __restrict__ q_solutions, const uint8_t* __restrict__ accept,
                                                    const double* __restrict__ base_pos, int T, int n_max, int f32,
                                                    double* __restrict__ partial /*[B][n_max][T]*/) {
  constexpr int TG = GTO_PLAN_TG;
  const int t0 = blockIdx.x * TG, j = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int ndof = rb->ndof;
  const int ng = min(TG, T - t0);
  __shared__ int s_row;
  if (tid < 64) {
    const int nb = seed_goal_count(n_goals, b, n_max);
    int seen = 0, row = -1;
    for (int r0 = 0; r0 < nb && row < 0; r0 += 64) {
      const int r = r0 + tid;
      const bool ok = r < nb && (!accept || accept[(size_t)b * n_max + r]);
      unsigned long long mask = __ballot(ok);
      const int cnt = __popcll(mask);
      if (seen + cnt > j) {
        for (int k = j - seen; k > 0; --k) mask &= mask - 1ull;
        row = r0 + __builtin_ctzll(mask);
      }
      seen += cnt;
    }
    if (tid == 0) s_row = row;
  }
  __syncthreads();
  const int row = s_row;
  if (row < 0) return;
  extern __shared__ __attribute__((aligned(16))) double smem_ss[];
  const PlanCostLds m = plan_cost_lds<TG>(rb, smem_ss);
  const double* qcb = qc + (size_t)b * ndof;
  const double* qs = q_solutions + ((size_t)b * n_max + row) * ndof;
  plan_cost_kinematics<TG>(rb, m, ng, tid, [&](int kq, int dq) { return seed_joint(rb, qcb, qs, dq, t0 + kq, T, f32); });
  const int sid = scene_id[b];
  double v = NAN;  // an id that names no scene: no cost
  if (seed_scene_ok(scenes, n_scenes, sid)) {
    const SceneDev sc = scenes[sid];
    v = plan_cost_gather<TG>(rb, px, py, pz, plink, sc, base_pos[3 * b], base_pos[3 * b + 1], base_pos[3 * b + 2], m, ng, tid);
  }
  if (tid < ng) partial[((size_t)b * n_max + j) * T + t0 + tid] = v;
}

// One wave per instance.  Rows 0..n_goals[b]-1 are walked 64 at a time: an accepted row's lane copies its goal to the row's
// compacted position, sums its candidate's partial costs in waypoint order, forms the joint distance of the candidate's
// first and last waypoint and keeps the best of its rows; the lanes' bests are folded by seed_before.
// RANKED (gto_seed_goalsets_multi_device): the first n_seeds entries of np.lexsort((dist, cost)) come out, one slot each.
// The walk and the fold are repeated per rank over the candidates that come after the rank before (the order is total: a
// position breaks every tie); the first walk alone writes the compaction and the scores, n_seeds times over for the goals,
// so that slot [b][r] is one instance of gto_solve_batch_device.  n_seeds = 1 writes what the plain form writes.
template <bool RANKED>
__device__ __forceinline__ void seed_select_body(const RobotDev* __restrict__ rb, const double* __restrict__ qc,
                                                 const double* __restrict__ goals, const int32_t* __restrict__ n_goals,
                                                 const double* __restrict__ q_solutions, const uint8_t* __restrict__ accept,
                                                 const double* __restrict__ partial, int T, int ts, int n_max,
                                                 int interpolate, int f32, int n_seeds, double* __restrict__ goals_out,
                                                 int32_t* __restrict__ n_goals_out, int32_t* __restrict__ n_accepted_out,
                                                 int32_t* __restrict__ accepted_rows_out, double* __restrict__ Q0_out,
                                                 int32_t* __restrict__ seed_index_out, double* __restrict__ seed_cost_out,
                                                 double* __restrict__ seed_dist_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int ndof = rb->ndof;
  const int nb = seed_goal_count(n_goals, b, n_max);
  const double* qcb = qc + (size_t)b * ndof;
  const int K = RANKED ? n_seeds : 1;
  double prev_c = 0.0, prev_d = 0.0;
  int prev_p = -1, row0 = 0, total = 0;
  for (int rank = 0; rank < K; ++rank) {
    double best_c = 0.0, best_d = 0.0;
    int best_p = INT_MAX, best_r = -1, seen = 0;
    if (rank == 0 || rank < total) {
      for (int r0 = 0; r0 < nb; r0 += 64) {
        const int r = r0 + lane;
        const bool ok = r < nb && (!accept || accept[(size_t)b * n_max + r]);
        const unsigned long long mask = __ballot(ok);
        if (ok) {
          const int pos = seen + __popcll(mask & ((1ull << lane) - 1ull));
          if (rank == 0 && goals_out)
            for (int k = 0; k < K; ++k)
              for (int e = 0; e < 16; ++e)
                goals_out[(((size_t)b * K + k) * n_max + pos) * 16 + e] = goals[((size_t)b * n_max + r) * 16 + e];
          if (RANKED && rank == 0 && accepted_rows_out) accepted_rows_out[(size_t)b * n_max + pos] = r;
          const double* part = partial + ((size_t)b * n_max + pos) * T;
          double c = 0.0;
          for (int t = 0; t < T; ++t) c += part[t];  // waypoint order, like the reference loop
          const double* qs = q_solutions + ((size_t)b * n_max + r) * ndof;
          double dd = 0.0;
          {
#pragma clang fp contract(off)
            for (int dq = 0; dq < ndof; ++dq) {
              const double v = seed_joint(rb, qcb, qs, dq, 0, T, f32) - seed_joint(rb, qcb, qs, dq, T - 1, T, f32);
              dd += v * v;
            }
          }
          const double d = __dsqrt_rn(dd);
          if (rank == 0 && seed_cost_out) seed_cost_out[(size_t)b * n_max + pos] = c;
          if (rank == 0 && seed_dist_out) seed_dist_out[(size_t)b * n_max + pos] = d;
          const bool open = rank == 0 || seed_before(prev_c, prev_d, prev_p, c, d, pos);  // behind the rank before
          if (open && (best_r < 0 || seed_before(c, d, pos, best_c, best_d, best_p))) best_c = c, best_d = d, best_p = pos, best_r = r;
        }
        seen += __popcll(mask);
      }
      for (int s = 32; s > 0; s >>= 1) {
        const double oc = __shfl_xor(best_c, s, 64), od = __shfl_xor(best_d, s, 64);
        const int op = __shfl_xor(best_p, s, 64), orow = __shfl_xor(best_r, s, 64);
        if (orow >= 0 && (best_r < 0 || seed_before(oc, od, op, best_c, best_d, best_p))) best_c = oc, best_d = od, best_p = op, best_r = orow;
      }
    }
    if (rank == 0) {
      total = seen;
      row0 = best_r;
      if (seen == 0 && goals_out)  // no accepted solution (the q_solutions=None branch): the goal set as it came
        for (int k = 0; k < K; ++k)
          for (int i = lane; i < nb * 16; i += 64) goals_out[((size_t)b * K + k) * n_max * 16 + i] = goals[(size_t)b * n_max * 16 + i];
      if (lane == 0 && n_accepted_out) n_accepted_out[b] = seen;
    }
    prev_c = best_c, prev_d = best_d, prev_p = best_p;
    const bool ranked = rank < total;  // a slot behind the accepted solutions solves slot 0's seed again
    if (lane == 0) {
      if (n_goals_out) n_goals_out[(size_t)b * K + rank] = total ? total : nb;
      if (seed_index_out) seed_index_out[(size_t)b * K + rank] = ranked ? best_p : -1;
    }
    if (!Q0_out) continue;
    const double* qs = q_solutions + ((size_t)b * n_max + (total ? (ranked ? best_r : row0) : 0)) * ndof;
    for (int i = lane; i < ndof * T; i += 64) {
      const int dq = i / T, t = i - dq * T;
      double v = qcb[dq];
      if (total) {
        if (interpolate) v = seed_joint(rb, qcb, qs, dq, t, T, f32);
        else if (t >= ts) v = seed_joint(rb, qcb, qs, dq, T - 1, T, f32);  // gto/gto_planner.py:216-219
      }
      Q0_out[(((size_t)b * K + rank) * ndof + dq) * T + t] = v;
    }
  }
}

__global__ __launch_bounds__(64) void k_seed_select(const RobotDev* __restrict__ rb, const double* __restrict__ qc,
                                                    const double* __restrict__ goals, const int32_t* __restrict__ n_goals,
                                                    const double* __restrict__ q_solutions, const uint8_t* __restrict__ accept,
                                                    const double* __restrict__ partial, int T, int ts, int n_max,
                                                    int interpolate, int f32, double* __restrict__ goals_out,
                                                    int32_t* __restrict__ n_goals_out, int32_t* __restrict__ n_accepted_out,
                                                    double* __restrict__ Q0_out, int32_t* __restrict__ seed_index_out,
                                                    double* __restrict__ seed_cost_out, double* __restrict__ seed_dist_out) {
  seed_select_body<false>(rb, qc, goals, n_goals, q_solutions, accept, partial, T, ts, n_max, interpolate, f32, 1, goals_out,
                          n_goals_out, n_accepted_out, nullptr, Q0_out, seed_index_out, seed_cost_out, seed_dist_out);
}

__global__ __launch_bounds__(64) void k_seed_select_ranked(const RobotDev* __restrict__ rb, const double* __restrict__ qc,
                                                           const double* __restrict__ goals, const int32_t* __restrict__ n_goals,
                                                           const double* __restrict__ q_solutions, const uint8_t* __restrict__ accept,
                                                           const double* __restrict__ partial, int T, int ts, int n_max,
                                                           int interpolate, int f32, int n_seeds, double* __restrict__ goals_out,
                                                           int32_t* __restrict__ n_goals_out, int32_t* __restrict__ n_accepted_out,
                                                           int32_t* __restrict__ accepted_rows_out, double* __restrict__ Q0_out,
                                                           int32_t* __restrict__ seed_index_out, double* __restrict__ seed_cost_out,
                                                           double* __restrict__ seed_dist_out) {
  seed_select_body<true>(rb, qc, goals, n_goals, q_solutions, accept, partial, T, ts, n_max, interpolate, f32, n_seeds, goals_out,
                         n_goals_out, n_accepted_out, accepted_rows_out, Q0_out, seed_index_out, seed_cost_out, seed_dist_out);
}

// ---- the report of a plan and the choice among the plans of an object's seeds (gto_plan_report_device, gto_select_plans_device)
// One workgroup per plan Q [ndof][T].  Wave 0 poses the last and the standoff waypoint and evaluates every goal's term of the
// objective as the solve does (fk_pair_wave, goal_terms_wave: f_goal and goal_argmin of gto_eval_objective); then all 256
// threads pose the last waypoint as k_ik_report does, and thread 0 reports the frame of link_ee against the chosen goal.
// A plan with a non-finite entry is reported as -1 / NaN before any kinematics run.
__global__ __launch_bounds__(256) void k_plan_report(const RobotDev* __restrict__ rb, const double* __restrict__ goals,
                                                     const int32_t* __restrict__ n_goals, const double* __restrict__ standoff,
                                                     const double* __restrict__ Q, int T, int ts, int n_max,
                                                     int32_t* __restrict__ goal_index_out, double* __restrict__ goal_cost_out,
                                                     double* __restrict__ err_pos_out, double* __restrict__ err_rot_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int F = rb->n_frames, ndof = rb->ndof;
  const double* Qb = Q + (size_t)b * ndof * T;
  __shared__ double s_gaff[48];
  __shared__ double s_q[2 * GTO_MAX_DOF];
  __shared__ double s_fr[2 * GTO_MAX_FRAMES * 12];
  __shared__ int s_arg;
  int bad = 0;
  for (int i = tid; i < ndof * T; i += 256) bad |= !isfinite(Qb[i]);
  if (__syncthreads_or(bad)) {  // (block-uniform)
    if (tid == 0) {
      if (goal_index_out) goal_index_out[b] = -1;
      if (goal_cost_out) goal_cost_out[b] = NAN;
      if (err_pos_out) err_pos_out[b] = NAN;
      if (err_rot_out) err_rot_out[b] = NAN;
    }
    return;
  }
  if (tid < 64) {
    const int which = tid >> 5, l = tid & 31;
    const int t = which == 0 ? T - 1 : ts;
    if (l < ndof) s_q[which * GTO_MAX_DOF + l] = Qb[(size_t)l * T + t];
    wave_sync();
    fk_pair_wave(rb, s_q, s_fr, tid);
    const double* fr = s_fr + which * GTO_MAX_FRAMES * 12;
    if (l < 12) {
      s_gaff[24 * which + l] = fr[12 * rb->frame_gripper + l];
      s_gaff[24 * which + 12 + l] = fr[12 * rb->frame_ee + l];
    }
    wave_sync();
    SolveParams sp;
    sp.use_standoff = standoff != nullptr;
    const GoalOut go = goal_terms_wave<GTO_NB>(rb, sp, goals + (size_t)b * n_max * 16, min(n_goals[b], n_max),
                                               standoff ? standoff + (size_t)b * 16 : nullptr, s_gaff, nullptr, nullptr, tid);
    if (tid == 0) {
      s_arg = go.argmin;
      if (goal_index_out) goal_index_out[b] = go.argmin;
      if (goal_cost_out) goal_cost_out[b] = go.f_goal;
    }
  }
  if (!err_pos_out && !err_rot_out) return;  // (uniform)
  extern __shared__ __attribute__((aligned(16))) double smem_pr[];
  // plan_cost_lds<1>'s layout, laid out here as in k_base_report (see there)
  PlanCostLds m;
  m.tab = smem_pr;
  m.sc = m.tab + fk_tab_doubles(F, rb->n_links, rb->n_opt);
  m.X = m.sc + F * 2;
  m.vis = m.X + fk_scratch_doubles(F, 1);
  m.screw = m.vis + rb->n_links * 12;
  m.red = m.screw + screw_rows(rb->n_opt) * 6;
  plan_cost_kinematics<1>(rb, m, 1, tid, [&](int, int dq) { return Qb[(size_t)dq * T + T - 1]; });  // (its barriers publish s_arg)
  if (tid != 0) return;
  double err_pos, err_rot;
  seed_pose_errors(m.X + (rb->fk_rounds & 1) * 16 * F, rb->frame_ee, goals + ((size_t)b * n_max + s_arg) * 16, &err_pos, &err_rot);
  if (err_pos_out) err_pos_out[b] = err_pos;
  if (err_rot_out) err_rot_out[b] = err_rot;
}

// The class of a slot's plan by the evaluator's standard: 0 valid, free and reached; 1 valid and free; 2 valid and reached;
// 3 valid; 4 not valid.  valid: the solve did not end numerically and its cost is finite; free: no waypoint's count is
// outside [0, max_points] (-1 marks a waypoint that could not be checked); reached: within both tolerances (false on NaN).
__device__ __forceinline__ int plan_class(int status, double cost, double err_pos, double err_rot,
                                          const int32_t* __restrict__ counts, int T, double pos_tol, double rot_tol_deg,
                                          int max_points) {
  if (status == GTO_STATUS_NUMERICAL || !isfinite(cost)) return 4;
  bool is_free = true;
  if (counts)
    for (int t = 0; t < T; ++t) is_free = is_free && counts[t] >= 0 && counts[t] <= max_points;
  const bool reached = err_pos < pos_tol && err_rot < rot_tol_deg;
  return (is_free ? 0 : 2) + (reached ? 0 : 1);
}

// One workgroup per object.  Wave 0 makes the choice, lane s holding slot s (n_seeds <= 64): the lowest class, then the
// lowest cost (numpy's order: a NaN after every number), then the lowest slot; all 256 threads copy the chosen slot's rows.
__global__ __launch_bounds__(256) void k_select_plans(int n_seeds, int T, int ndof, const int32_t* __restrict__ status,
                                                      const double* __restrict__ cost, const double* __restrict__ err_pos,
                                                      const double* __restrict__ err_rot, const int32_t* __restrict__ counts,
                                                      double pos_tol, double rot_tol_deg, int max_points,
                                                      const double* __restrict__ Q, const double* __restrict__ dQ,
                                                      int32_t* __restrict__ best_slot_out, int32_t* __restrict__ class_out,
                                                      double* __restrict__ Q_out, double* __restrict__ dQ_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ int s_slot;
  if (tid < 64) {
    int cls = 5, slot = INT_MAX;  // (a lane without a slot loses against every slot)
    double c = NAN;
    if (tid < n_seeds) {
      const size_t i = (size_t)b * n_seeds + tid;
      slot = tid;
      c = cost[i];
      cls = plan_class(status[i], c, err_pos[i], err_rot[i], counts ? counts + i * T : nullptr, T, pos_tol, rot_tol_deg, max_points);
    }
    for (int s = 32; s > 0; s >>= 1) {
      const int ocls = __shfl_xor(cls, s, 64), oslot = __shfl_xor(slot, s, 64);
      const double oc = __shfl_xor(c, s, 64);
      const bool first = ocls != cls ? ocls < cls : (seed_key_less(oc, c) || (!seed_key_less(c, oc) && oslot < slot));
      if (first) cls = ocls, c = oc, slot = oslot;
    }
    if (tid == 0) {
      s_slot = slot;
      if (best_slot_out) best_slot_out[b] = slot;
      if (class_out) class_out[b] = cls;
    }
  }
  __syncthreads();
  const size_t src = (size_t)b * n_seeds + s_slot;
  if (Q_out)
    for (int i = tid; i < ndof * T; i += 256) Q_out[(size_t)b * ndof * T + i] = Q[src * ndof * T + i];
  if (dQ_out)
    for (int i = tid; i < ndof * (T - 1); i += 256) dQ_out[(size_t)b * ndof * (T - 1) + i] = dQ[src * ndof * (T - 1) + i];
}
