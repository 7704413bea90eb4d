// gto_observe.h — collision checks against a resident observation (gto_observation_*, gto_check_plans: include/gto_solver.h).
// The grasp collision filter of the planning driver (examples/pybullet_gto_planning.py:203-221,
// examples/pybullet_gto_planning_mobile.py:307-322) and the plan collision statistic of the offline evaluator
// (examples/pybullet_evaluate_plans.py:219-233): surface points of the gripper / the robot are placed in the world and the
// ones with get_sdf < 0 are counted.
//
// Depth observation.  get_sdf is the float32 distance to the cloud, negated where the point fails the visibility test
// (mesh_to_sdf/depth_point_cloud.py:57-62, 127-141), so "get_sdf < 0" is "!is_outside" for every point that does not
// coincide with a cloud point: the count needs no nearest-neighbour search.
//   k_check_plans<true>   one workgroup per (plan, four waypoints): kinematics of the four configurations into LDS
//                         (plan_cost_kinematics, gto_kernels.h), lanes over the surface points in the handle's
//                         per-link order, depth_is_outside (gto_depth.h) per point, ballot + popcount per wave, the four
//                         waves' counts through LDS, one store per waypoint
//   k_check_posed<true>   one workgroup per pose: x = R p + t without contraction, the products added in the order
//                         numpy.einsum("nij,pj->npi") adds them (x, z, y) before the translation; the same counting
// Cloud observation (sampled mesh).  The sign is the vote of the k nearest samples' normals, so there is a search:
//   k_check_plans<false> / k_check_posed<false>  write the world points [item][P][3] instead of counting (and mark the
//                         items with a non-finite entry); consecutive points belong to one link at one waypoint, so the 64
//                         queries of a wave are neighbours in space and k_cloud_knn's packet walk (gto_cloud.h) takes them
//                         in this order, without keys and without a sort
//   k_count_flags         one workgroup per item: the P votes of k_cloud_knn summed (ballot + popcount, LDS across waves)
// An item (waypoint or pose) with a non-finite entry reports -1; its kinematics run on zeros, so nothing non-finite enters
// a matrix-core product or a search.
//
// The grasp filter on the stream (gto_filter_grasps_device; the driver's checking stage, :203-236, for many objects):
//   k_filter_depth        one workgroup per (row, depth object): the object's view from a device table, G = object pose x
//                         grasp (x world_to_base), C = G x check_offset and the two goals once per workgroup (wave-uniform),
//                         then k_check_posed<true>'s placement (place_einsum) and counting against the object's own image
//   k_filter_pose         the same composition for the objects of a cloud observation: C goes to a workspace in the layout
//                         k_check_posed<false> takes, whose launch chain (points, votes, k_count_flags) does the counting
//   k_filter_compact      one wave per object: keep = count / P <= max_ratio, the kept rows' goals to their compacted
//                         positions, 64 rows at a time with a ballot prefix
#pragma once
#include "gto_cloud.h"

// what depth_is_outside reads of a depth observation (all pointers: device)
struct ObsDepthView {
  const float* depth;
  int H, W;
  const double *K, *cam_inv;
};

#define GTO_CHECK_TG GTO_PLAN_TG  // most waypoints per workgroup of k_check_plans (the LDS layout is k_plan_cost's)
__host__ __device__ inline int check_plans_lds_doubles(int F, int L, int n) { return plan_cost_lds_doubles(F, L, n); }

// sum over the workgroup's four waves of a wave-uniform count per group g < TG; s_cnt: [4][TG] ints of LDS
template <int TG>
__device__ __forceinline__ void check_counts_to_lds(const int (&cnt)[TG], int tid, int* s_cnt) {
  if ((tid & 63) == 0) {
#pragma unroll
    for (int g = 0; g < TG; ++g) s_cnt[(tid >> 6) * TG + g] = cnt[g];
  }
}

// x = R p + t for a row-major pose M (3x4 or 4x4), without contraction: numpy.einsum("nij,pj->npi") adds the three
// products of a row in the order x, z, y (numpy 2.2's unrolled inner loop) before the translation: the bits of
// utils.grasp_collision_ratio, which tests/test_gpu_observation.py compares with
__device__ __forceinline__ void place_einsum(const double* M, double x0, double x1, double x2, double* X0, double* X1, double* X2) {
#pragma clang fp contract(off)  // numpy's products and sums, one rounding each
  *X0 = ((M[0] * x0 + M[2] * x2) + M[1] * x1) + M[3];
  *X1 = ((M[4] * x0 + M[6] * x2) + M[5] * x1) + M[7];
  *X2 = ((M[8] * x0 + M[10] * x2) + M[9] * x1) + M[11];
}

// sum over the workgroup's four waves of a wave-uniform count; s_cnt: 4 ints of LDS.  Every thread calls it (a barrier).
__device__ __forceinline__ int wave_counts_sum(int cnt, int tid, int* s_cnt) {
  if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
  __syncthreads();
  return ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
}

// plans [nplans][ndof][T]; tg: waypoints per workgroup, 1..GTO_CHECK_TG (grid.y = ceil(T / tg); results do not depend on
// it: every waypoint's kinematics are a matrix-core block of their own); base: (b0, b1, b2) for every plan, or base_pp [nplans][3].  DEPTH: count_out [nplans][T].
// !DEPTH: xyz_out [nplans][T][P][3] and count_out [nplans][T] = -1 for a waypoint with a non-finite entry, else 0.
// The world point is k_eval_points' expression, term for term (gto_kernels.h): the same bits as gto_eval_points' xyz_out.
template <bool DEPTH>
__global__ __launch_bounds__(256) void k_check_plans(const RobotDev* __restrict__ rb, const double* __restrict__ px,
                                                     const double* __restrict__ py, const double* __restrict__ pz,
                                                     const int32_t* __restrict__ plink, int T, int tg, const double* __restrict__ plans,
                                                     double b0, double b1, double b2, const double* __restrict__ base_pp,
                                                     ObsDepthView dv, double* __restrict__ xyz_out,
                                                     int32_t* __restrict__ count_out) {
  constexpr int TG = GTO_CHECK_TG;
  const int i = blockIdx.x, t0 = blockIdx.y * tg, tid = threadIdx.x;  // tg <= TG waypoints per workgroup (GTO_CHECK_TG)
  const int L = rb->n_links, ndof = rb->ndof, P = rb->n_points;
  const int ng = min(tg, T - t0);
  extern __shared__ __attribute__((aligned(16))) double smem_ck[];
  const PlanCostLds m = plan_cost_lds<TG>(rb, smem_ck);
  const double* s_vis = m.vis;
  int* s_cnt = reinterpret_cast<int*>(m.red);  // [4][TG]
  int* s_bad = s_cnt + 4 * TG;                 // [TG]
  if (tid < TG) s_bad[tid] = 0;
  __syncthreads();
  for (int idx = tid; idx < ng * ndof; idx += 256) {
    const int kq = idx / ndof, j = idx - kq * ndof;
    if (!isfinite(plans[((size_t)i * ndof + j) * T + t0 + kq])) s_bad[kq] = 1;
  }
  __syncthreads();
  plan_cost_kinematics<TG>(rb, m, ng, tid, [&](int kq, int dq) { return s_bad[kq] ? 0.0 : plans[((size_t)i * ndof + dq) * T + t0 + kq]; });
  if (base_pp) b0 = base_pp[3 * (size_t)i], b1 = base_pp[3 * (size_t)i + 1], b2 = base_pp[3 * (size_t)i + 2];
  const bool base_ok = isfinite(b0) && isfinite(b1) && isfinite(b2);
  int cnt[TG];
#pragma unroll
  for (int g = 0; g < TG; ++g) cnt[g] = 0;
  for (int p0 = 0; p0 < P; p0 += 256) {  // uniform trip count: every lane takes part in the ballots
    const int p = p0 + tid;
    const bool live = p < P;
    const double x0 = live ? px[p] : 0.0, x1 = live ? py[p] : 0.0, x2 = live ? pz[p] : 0.0;
    const int l = live ? plink[p] : 0;
#pragma unroll
    for (int g = 0; g < TG; ++g) {
      if (g < ng) {
        const double* V = s_vis + (g * L + l) * 12;
        const double X0 = V[0] * x0 + V[1] * x1 + V[2] * x2 + V[3] + b0;
        const double X1 = V[4] * x0 + V[5] * x1 + V[6] * x2 + V[7] + b1;
        const double X2 = V[8] * x0 + V[9] * x1 + V[10] * x2 + V[11] + b2;
        if constexpr (DEPTH) {
          const bool in = live && !depth_is_outside(X0, X1, X2, dv.depth, dv.H, dv.W, dv.K, dv.cam_inv);
          cnt[g] += __popcll(__ballot(in));
        } else if (live) {
          double* o = xyz_out + (((size_t)i * T + t0 + g) * P + p) * 3;
          const bool ok = base_ok && !s_bad[g];
          o[0] = ok ? X0 : 0.0, o[1] = ok ? X1 : 0.0, o[2] = ok ? X2 : 0.0;
        }
      }
    }
  }
  if constexpr (DEPTH) {
    check_counts_to_lds<TG>(cnt, tid, s_cnt);
    __syncthreads();
    if (tid < ng)
      count_out[(size_t)i * T + t0 + tid] =
          (s_bad[tid] || !base_ok) ? -1 : ((s_cnt[tid] + s_cnt[TG + tid]) + s_cnt[2 * TG + tid]) + s_cnt[3 * TG + tid];
  } else {
    if (tid < ng) count_out[(size_t)i * T + t0 + tid] = (s_bad[tid] || !base_ok) ? -1 : 0;
  }
}

// points [P][3] in the frame the poses place (the open gripper's surface points in the gripper frame), poses [n][16]
// row-major 4x4.  DEPTH: count_out [n].  !DEPTH: xyz_out [n][P][3] and count_out [n] = -1 for a non-finite pose, else 0.
template <bool DEPTH>
__global__ __launch_bounds__(256) void k_check_posed(const double* __restrict__ points, int P, const double* __restrict__ poses,
                                                     ObsDepthView dv, double* __restrict__ xyz_out,
                                                     int32_t* __restrict__ count_out) {
  __shared__ int s_cnt[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const double* M = poses + 16 * (size_t)i;
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 16; ++e) bad = bad || !isfinite(M[e]);  // uniform: every lane reads the same sixteen values
  if (bad) {
    if (tid == 0) count_out[i] = -1;
    if constexpr (DEPTH) return;
  }
  int cnt = 0;
  for (int p0 = 0; p0 < P; p0 += 256) {
    const int p = p0 + tid;
    const bool live = p < P;
    const double x0 = live ? points[3 * (size_t)p] : 0.0, x1 = live ? points[3 * (size_t)p + 1] : 0.0,
                 x2 = live ? points[3 * (size_t)p + 2] : 0.0;
    double X0, X1, X2;
    place_einsum(M, x0, x1, x2, &X0, &X1, &X2);
    if constexpr (DEPTH) {
      const bool in = live && !depth_is_outside(X0, X1, X2, dv.depth, dv.H, dv.W, dv.K, dv.cam_inv);
      cnt += __popcll(__ballot(in));
    } else if (live) {
      double* o = xyz_out + ((size_t)i * P + p) * 3;
      o[0] = bad ? 0.0 : X0, o[1] = bad ? 0.0 : X1, o[2] = bad ? 0.0 : X2;
    }
  }
  if constexpr (DEPTH) {
    const int total = wave_counts_sum(cnt, tid, s_cnt);
    if (tid == 0) count_out[i] = total;
  } else {
    if (tid == 0 && !bad) count_out[i] = 0;
  }
}

// count[item] = number of non-zero flags among flags[item][P]; an item marked -1 keeps its mark
__global__ __launch_bounds__(256) void k_count_flags(const uint8_t* __restrict__ flags, int P, int32_t* __restrict__ count) {
  __shared__ int s_cnt[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (count[i] < 0) return;  // uniform
  int cnt = 0;
  for (int p0 = 0; p0 < P; p0 += 256) {
    const int p = p0 + tid;
    cnt += __popcll(__ballot(p < P && flags[(size_t)i * P + p] != 0));
  }
  const int total = wave_counts_sum(cnt, tid, s_cnt);
  if (tid == 0) count[i] = total;
}

// ---- the grasp filter on the stream (gto_filter_grasps_device) ----
// a host matrix that travels with the launch (check_offset, ik_offset)
struct PoseArg { double m[16]; };
// one depth object of a call: the view of its observation and which object it is
struct FilterDepthItem {
  ObsDepthView dv;
  int32_t obj;
};

// how many rows of object b count: n_grasps lives on the device, so a value outside [1, n_max] is read as clamped (the rule
// of gto_seed_goalsets_device)
__device__ __forceinline__ int filter_row_count(const int32_t* __restrict__ n_grasps, int b, int n_max) {
  return min(max(n_grasps[b], 1), n_max);
}

// C = A B for row-major 4x4 matrices: the full product, entry (r, c) = ((A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c) + A_r3 B_3c,
// FP64 without contraction (utils.pose_product writes the same expression in numpy)
__device__ __forceinline__ void pose_product(const double* A, const double* B, double* C) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

// What a row of the filter is made of: Cm = the pose the gripper's points are placed at, plan / ik = the two goals.
// Returns false for a row that reports -1: a non-finite entry in the object's pose, the grasp or world_to_base, or in Cm.
// Every lane of a workgroup reads the same addresses: the values are wave-uniform.
__device__ __forceinline__ bool filter_compose(int b, int i, int n_max, const double* __restrict__ object_pose,
                                               const double* __restrict__ grasps, const double* __restrict__ world_to_base,
                                               const double* __restrict__ base_pos, const PoseArg& check_off, const PoseArg& ik_off,
                                               bool has_ik_off, double* Cm, double* plan, double* ik) {
#pragma clang fp contract(off)
  double O[16], R[16], G[16];
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    O[e] = object_pose[16 * (size_t)b + e];
    R[e] = grasps[((size_t)b * n_max + i) * 16 + e];
    ok = ok && isfinite(O[e]) && isfinite(R[e]);
  }
  pose_product(O, R, G);
  if (world_to_base) {
    double Wm[16], WG[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      Wm[e] = world_to_base[16 * (size_t)b + e];
      ok = ok && isfinite(Wm[e]);
    }
    pose_product(Wm, G, WG);
#pragma unroll
    for (int e = 0; e < 16; ++e) G[e] = WG[e];
  }
  pose_product(G, check_off.m, Cm);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    ok = ok && isfinite(Cm[e]);
    plan[e] = G[e];
  }
  if (base_pos) {
#pragma unroll
    for (int r = 0; r < 3; ++r) plan[4 * r + 3] = G[4 * r + 3] - base_pos[3 * (size_t)b + r];
  }
  if (has_ik_off) {
    pose_product(plan, ik_off.m, ik);
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) ik[e] = plan[e];
  }
  return ok;
}

// grid (n_max, depth objects).  ws_plan, ws_ik [B][n_max][16]: the uncompacted goals; ws_count [B][n_max].  Rows at or
// beyond the object's n_grasps (clamped to [1, n_max] as gto_seed_goalsets_device reads it) are not touched.
__global__ __launch_bounds__(256) void k_filter_depth(const FilterDepthItem* __restrict__ items, const double* __restrict__ points,
                                                      int P, int n_max, const double* __restrict__ object_pose,
                                                      const double* __restrict__ grasps, const int32_t* __restrict__ n_grasps,
                                                      const double* __restrict__ world_to_base, const double* __restrict__ base_pos,
                                                      PoseArg check_off, PoseArg ik_off, int has_ik_off, double* __restrict__ ws_plan,
                                                      double* __restrict__ ws_ik, int32_t* __restrict__ ws_count) {
  __shared__ int s_cnt[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int b = items[blockIdx.y].obj;
  const ObsDepthView dv = items[blockIdx.y].dv;
  if (i >= filter_row_count(n_grasps, b, n_max)) return;  // uniform
  double M[16], plan[16], ik[16];
  const bool ok = filter_compose(b, i, n_max, object_pose, grasps, world_to_base, base_pos, check_off, ik_off, has_ik_off != 0, M, plan, ik);
  const size_t row = (size_t)b * n_max + i;
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) ws_plan[row * 16 + e] = plan[e], ws_ik[row * 16 + e] = ik[e];
  }
  if (!ok) {  // uniform
    if (tid == 0) ws_count[row] = -1;
    return;
  }
  int cnt = 0;
  for (int p0 = 0; p0 < P; p0 += 256) {  // uniform trip count: every lane takes part in the ballots
    const int p = p0 + tid;
    const bool live = p < P;
    const double x0 = live ? points[3 * (size_t)p] : 0.0, x1 = live ? points[3 * (size_t)p + 1] : 0.0,
                 x2 = live ? points[3 * (size_t)p + 2] : 0.0;
    double X0, X1, X2;
    place_einsum(M, x0, x1, x2, &X0, &X1, &X2);
    const bool in = live && !depth_is_outside(X0, X1, X2, dv.depth, dv.H, dv.W, dv.K, dv.cam_inv);
    cnt += __popcll(__ballot(in));
  }
  const int total = wave_counts_sum(cnt, tid, s_cnt);
  if (tid == 0) ws_count[row] = total;
}

// grid (ceil(n_max / 64), objects of the run), objects b0 .. b0 + gridDim.y - 1 (a run of one cloud observation): one lane
// per row.  ws_pose [B][n_max][16] gets the pose k_check_posed<false> places the points at; a row that reports -1 and the
// rows at or beyond n_grasps get a NaN in entry 0, which that kernel marks -1 (and k_count_flags then leaves alone).
__global__ __launch_bounds__(64) void k_filter_pose(int b0, int n_max, const double* __restrict__ object_pose,
                                                    const double* __restrict__ grasps, const int32_t* __restrict__ n_grasps,
                                                    const double* __restrict__ world_to_base, const double* __restrict__ base_pos,
                                                    PoseArg check_off, PoseArg ik_off, int has_ik_off, double* __restrict__ ws_plan,
                                                    double* __restrict__ ws_ik, double* __restrict__ ws_pose) {
  const int i = blockIdx.x * 64 + threadIdx.x, b = b0 + blockIdx.y;
  if (i >= n_max) return;
  const size_t row = (size_t)b * n_max + i;
  if (i >= filter_row_count(n_grasps, b, n_max)) {
    ws_pose[row * 16] = NAN;
    return;
  }
  double M[16], plan[16], ik[16];
  const bool ok = filter_compose(b, i, n_max, object_pose, grasps, world_to_base, base_pos, check_off, ik_off, has_ik_off != 0, M, plan, ik);
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    ws_plan[row * 16 + e] = plan[e], ws_ik[row * 16 + e] = ik[e];
    ws_pose[row * 16 + e] = (e == 0 && !ok) ? NAN : M[e];
  }
}

// grid B, one wave per object.  Rows 0 .. n_grasps[b] - 1 are walked 64 at a time (n_max may exceed a wave, as in
// k_seed_select): a kept row's lane copies the row's two goals to the compacted position its ballot prefix gives it.
// No row kept: position 0 gets row 0's goals and kept_rows_out [b][0] = -1 (the object stays solvable by the chain).
__global__ __launch_bounds__(64) void k_filter_compact(int n_max, int P, double max_ratio, const int32_t* __restrict__ n_grasps,
                                                       const int32_t* __restrict__ ws_count, const double* __restrict__ ws_plan,
                                                       const double* __restrict__ ws_ik, int32_t* __restrict__ count_out,
                                                       uint8_t* __restrict__ keep_out, int32_t* __restrict__ kept_rows_out,
                                                       int32_t* __restrict__ n_kept_out, int32_t* __restrict__ n_grasps_out,
                                                       double* __restrict__ plan_goals_out, double* __restrict__ ik_goals_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nb = filter_row_count(n_grasps, b, n_max);
  const size_t base = (size_t)b * n_max;
  int seen = 0;
  for (int r0 = 0; r0 < nb; r0 += 64) {
    const int r = r0 + lane;
    const bool live = r < nb;
    const int cnt = live ? ws_count[base + r] : -1;
    const bool keep = live && cnt >= 0 && (double)cnt / (double)P <= max_ratio;
    if (live && count_out) count_out[base + r] = cnt;
    if (live && keep_out) keep_out[base + r] = keep ? 1 : 0;
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const size_t pos = base + seen + __popcll(mask & ((1ull << lane) - 1ull));
      if (kept_rows_out) kept_rows_out[pos] = r;
      for (int e = 0; e < 16; ++e) {
        if (plan_goals_out) plan_goals_out[pos * 16 + e] = ws_plan[(base + r) * 16 + e];
        if (ik_goals_out) ik_goals_out[pos * 16 + e] = ws_ik[(base + r) * 16 + e];
      }
    }
    seen += __popcll(mask);
  }
  if (seen == 0 && lane < 16) {
    if (plan_goals_out) plan_goals_out[base * 16 + lane] = ws_plan[base * 16 + lane];
    if (ik_goals_out) ik_goals_out[base * 16 + lane] = ws_ik[base * 16 + lane];
  }
  if (lane == 0) {
    if (seen == 0 && kept_rows_out) kept_rows_out[base] = -1;
    if (n_kept_out) n_kept_out[b] = seen;
    if (n_grasps_out) n_grasps_out[b] = max(seen, 1);
  }
}
