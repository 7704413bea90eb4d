// gto_seed.h — the stream-ordered steps between inverse kinematics and the trajectory solve (gfx950):
//   k_ik_report    what the reference reports of an IK solution (gto/ik_solver.py:88-97) and the driver's acceptance test
//                  (examples/pybullet_gto_planning.py:262), one workgroup per instance
//   k_seed_score   obstacle cost of the seed candidate of every accepted IK solution (gto/gto_planner.py:197-211), the
//                  candidates generated in the kernel; kinematics and sums are k_plan_cost's (plan_cost_kinematics,
//                  plan_cost_gather in gto_kernels.h)
//   k_seed_select  compaction of the accepted goals (:267-269 of the driver), np.lexsort((dist, cost))[0] and the seed of
//                  the trajectory solve (gto/gto_planner.py:212-219), one wave per instance
#pragma once
#include "gto_kernels.h"

// a scene id that names a set scene with a c_obs field (all these kernels read)
__device__ __forceinline__ bool seed_scene_ok(const SceneDev* __restrict__ scenes, int n_scenes, int sid) {
  return (unsigned)sid < (unsigned)n_scenes && scenes[sid].valid && scenes[sid].c_obs;
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
  const double* Xg = m.X + (rb->fk_rounds & 1) * 16 * F;  // X_f = G_f^T
  const double* g = goals + (size_t)b * 16;
  double E[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) E[e] = Xg[fkx(rb->frame_ee, 4 * (e & 3) + (e >> 2))];
  const double d0 = g[3] - E[3], d1 = g[7] - E[7], d2 = g[11] - E[11];
  const double err_pos = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) tr += g[4 * i + j] * E[4 * i + j];
  double c = (tr - 1.0) / 2.0;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);  // (a NaN stays one, as in np.clip)
  const double err_rot = acos(c) * (180.0 / M_PI);
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
__global__ __launch_bounds__(64) void k_seed_select(const RobotDev* __restrict__ rb, const double* __restrict__ qc,
                                                    const double* __restrict__ goals, const int32_t* __restrict__ n_goals,
                                                    const double* __restrict__ q_solutions, const uint8_t* __restrict__ accept,
                                                    const double* __restrict__ partial, int T, int ts, int n_max,
                                                    int interpolate, int f32, double* __restrict__ goals_out,
                                                    int32_t* __restrict__ n_goals_out, int32_t* __restrict__ n_accepted_out,
                                                    double* __restrict__ Q0_out, int32_t* __restrict__ seed_index_out,
                                                    double* __restrict__ seed_cost_out, double* __restrict__ seed_dist_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int ndof = rb->ndof;
  const int nb = seed_goal_count(n_goals, b, n_max);
  const double* qcb = qc + (size_t)b * ndof;
  double best_c = 0.0, best_d = 0.0;
  int best_p = INT_MAX, best_r = -1, seen = 0;
  for (int r0 = 0; r0 < nb; r0 += 64) {
    const int r = r0 + lane;
    const bool ok = r < nb && (!accept || accept[(size_t)b * n_max + r]);
    const unsigned long long mask = __ballot(ok);
    if (ok) {
      const int pos = seen + __popcll(mask & ((1ull << lane) - 1ull));
      if (goals_out)
        for (int e = 0; e < 16; ++e) goals_out[((size_t)b * n_max + pos) * 16 + e] = goals[((size_t)b * n_max + r) * 16 + e];
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
      if (seed_cost_out) seed_cost_out[(size_t)b * n_max + pos] = c;
      if (seed_dist_out) seed_dist_out[(size_t)b * n_max + pos] = d;
      if (best_r < 0 || seed_before(c, d, pos, best_c, best_d, best_p)) best_c = c, best_d = d, best_p = pos, best_r = r;
    }
    seen += __popcll(mask);
  }
  for (int s = 32; s > 0; s >>= 1) {
    const double oc = __shfl_xor(best_c, s, 64), od = __shfl_xor(best_d, s, 64);
    const int op = __shfl_xor(best_p, s, 64), orow = __shfl_xor(best_r, s, 64);
    if (orow >= 0 && (best_r < 0 || seed_before(oc, od, op, best_c, best_d, best_p))) best_c = oc, best_d = od, best_p = op, best_r = orow;
  }
  if (seen == 0 && goals_out)  // no accepted solution (the q_solutions=None branch): the goal set as it came
    for (int i = lane; i < nb * 16; i += 64) goals_out[(size_t)b * n_max * 16 + i] = goals[(size_t)b * n_max * 16 + i];
  if (lane == 0) {
    if (n_goals_out) n_goals_out[b] = seen ? seen : nb;
    if (n_accepted_out) n_accepted_out[b] = seen;
    if (seed_index_out) seed_index_out[b] = seen ? best_p : -1;
  }
  if (!Q0_out) return;
  const double* qs = q_solutions + ((size_t)b * n_max + (seen ? best_r : 0)) * ndof;
  for (int i = lane; i < ndof * T; i += 64) {
    const int dq = i / T, t = i - dq * T;
    double v = qcb[dq];
    if (seen) {
      if (interpolate) v = seed_joint(rb, qcb, qs, dq, t, T, f32);
      else if (t >= ts) v = seed_joint(rb, qcb, qs, dq, T - 1, T, f32);  // gto/gto_planner.py:216-219
    }
    Q0_out[((size_t)b * ndof + dq) * T + t] = v;
  }
}
