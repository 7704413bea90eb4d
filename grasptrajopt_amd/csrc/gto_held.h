// gto_held.h — the grasped object's points along the motion after the grasp (gto_check_held_paths[_device]:
// include/gto_solver.h).  gto_check_paths counts the ROBOT's surface points inside the observation at every column of the
// retrieve path; during that motion the robot carries the object, and the object is what meets the neighbour on the table or
// the shelf board above.  The held points ride rigidly with link_ee from the configuration the object was grasped at:
//   k_held_attach        one workgroup per plan: kinematics of q_att (plan_cost_kinematics<1>), the optional placement
//                        of object-frame points (place_einsum), then p = E_a^-1 (x - base) per point into a
//                        workspace [B][P_max][3] and a per-plan bad flag.  Once per plan, not once per column group.
//   k_check_held<true>   one workgroup per (plan, up to GTO_CHECK_TG columns) in k_check_plans' LDS layout: the columns'
//                        kinematics, E_t of link_ee from the tree's frames, lanes over the held points with a uniform trip
//                        count, depth_is_outside plus the label test (a pixel that shows the held object hides nothing that
//                        was seen: such a point counts as outside), ballot + popcount, the four waves' counts through LDS,
//                        one store per column.  No atomics.
//   k_check_held<false>  writes the world points [plan][Tp][P_max][3] (NaN for rows past n_held and for non-finite points:
//                        k_cloud_knn takes a NaN query as outside) for the chain k_cloud_knn -> k_count_flags of gto_observe.h
// All placement arithmetic is FP64 without contraction, in the order the header states.
#pragma once
#include "gto_observe.h"

// plan_cost_lds<1>'s layout, then E_a [12] and the bad flag
__host__ __device__ inline int held_attach_lds_doubles(int F, int L, int n) { return plan_cost_lds_doubles_tg(1, F, L, n) + 16; }

// how many points of plan b count: n_held lives on the device, so a value outside [0, P_max] is read as clamped
__device__ __forceinline__ int held_point_count(const int32_t* __restrict__ n_held, int b, int P_max) {
  return min(max(n_held[b], 0), P_max);
}

// rows 0..2 of link_ee's frame (row-major 3x4: R | tr) of configuration kq from the transposed frames
// plan_cost_kinematics left in s_X: the entries gto_eval_fk writes
__device__ __forceinline__ double held_frame_entry(const RobotDev* __restrict__ rb, const double* __restrict__ s_X, int F, int kq, int e) {
  const double* Xg = s_X + (size_t)kq * 32 * F + (rb->fk_rounds & 1) * 16 * F;
  return Xg[fkx(rb->frame_ee, 4 * (e & 3) + (e >> 2))];
}

// attach: q_att[b][j] = attach[(b * ndof + j) * attach_ld + attach_col].  base: (b0, b1, b2) for every plan, or base_pp
// [B][3].  held_points [B][P_max][3]; object_pose [B][16] or null (the points are world points).  p_out [B][P_max][3]:
// the points in link_ee's frame at q_att (NaN for rows at or beyond n_held and for a point with a non-finite coordinate;
// zeros for a bad plan).  bad_out [B]: 1 when q_att, the base or the object's pose holds a non-finite entry.
__global__ __launch_bounds__(256) void k_held_attach(const RobotDev* __restrict__ rb, const double* __restrict__ attach, int attach_ld,
                                                     int attach_col, double b0, double b1, double b2,
                                                     const double* __restrict__ base_pp, const double* __restrict__ held_points,
                                                     int P_max, const int32_t* __restrict__ n_held,
                                                     const double* __restrict__ object_pose, double* __restrict__ p_out,
                                                     int32_t* __restrict__ bad_out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int F = rb->n_frames, ndof = rb->ndof;
  extern __shared__ __attribute__((aligned(16))) double smem_ha[];
  const PlanCostLds m = plan_cost_lds<1>(rb, smem_ha);
  double* s_E = smem_ha + plan_cost_lds_doubles_tg(1, F, rb->n_links, rb->n_opt);  // [12]
  int* s_bad = reinterpret_cast<int*>(s_E + 12);
  if (tid == 0) s_bad[0] = 0;
  __syncthreads();
  const double* qa = attach + (size_t)b * ndof * attach_ld + attach_col;
  if (tid < ndof && !isfinite(qa[(size_t)tid * attach_ld])) s_bad[0] = 1;
  __syncthreads();
  const bool q_bad = s_bad[0] != 0;
  plan_cost_kinematics<1>(rb, m, 1, tid, [&](int, int dq) { return q_bad ? 0.0 : qa[(size_t)dq * attach_ld]; });
  if (tid < 12) s_E[tid] = held_frame_entry(rb, m.X, F, 0, tid);
  __syncthreads();
  if (base_pp) b0 = base_pp[3 * (size_t)b], b1 = base_pp[3 * (size_t)b + 1], b2 = base_pp[3 * (size_t)b + 2];
  bool bad = q_bad || !(isfinite(b0) && isfinite(b1) && isfinite(b2));
  double M[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) M[e] = 0.0;
  if (object_pose) {  // uniform: every lane reads the same sixteen values
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const double v = object_pose[16 * (size_t)b + e];
      bad = bad || !isfinite(v);
      if (e < 12) M[e] = v;
    }
  }
  if (tid == 0) bad_out[b] = bad ? 1 : 0;
  const int nb = held_point_count(n_held, b, P_max);
  for (int i = tid; i < P_max; i += 256) {
    const size_t o = ((size_t)b * P_max + i) * 3;
    double x0 = held_points[o], x1 = held_points[o + 1], x2 = held_points[o + 2];
    const bool ok = i < nb && isfinite(x0) && isfinite(x1) && isfinite(x2);
    if (object_pose) place_einsum(M, x0, x1, x2, &x0, &x1, &x2);
    const double d0 = (x0 - b0) - s_E[3], d1 = (x1 - b1) - s_E[7], d2 = (x2 - b2) - s_E[11];
    const double p0 = (s_E[0] * d0 + s_E[4] * d1) + s_E[8] * d2;
    const double p1 = (s_E[1] * d0 + s_E[5] * d1) + s_E[9] * d2;
    const double p2 = (s_E[2] * d0 + s_E[6] * d1) + s_E[10] * d2;
    p_out[o] = bad ? 0.0 : (ok ? p0 : NAN);
    p_out[o + 1] = bad ? 0.0 : (ok ? p1 : NAN);
    p_out[o + 2] = bad ? 0.0 : (ok ? p2 : NAN);
  }
}

// paths [nplans][ndof][T]; tg, base: as k_check_plans.  held_p [nplans][P_max][3], n_held, bad_plan [nplans]: what
// k_held_attach wrote.  labels [H][W] or null, held_label [nplans] (read only with labels): the label rule.
// DEPTH: count_out [nplans][T].  !DEPTH: xyz_out [nplans][T][P_max][3] and count_out [nplans][T] = -1 for a column that
// reports -1, else 0.
template <bool DEPTH>
__global__ __launch_bounds__(256) void k_check_held(const RobotDev* __restrict__ rb, int T, int tg, const double* __restrict__ paths,
                                                    double b0, double b1, double b2, const double* __restrict__ base_pp,
                                                    const double* __restrict__ held_p, int P_max, const int32_t* __restrict__ n_held,
                                                    const int32_t* __restrict__ bad_plan, ObsDepthView dv,
                                                    const int32_t* __restrict__ labels, const int32_t* __restrict__ held_label,
                                                    double* __restrict__ xyz_out, int32_t* __restrict__ count_out) {
#pragma clang fp contract(off)
  constexpr int TG = GTO_CHECK_TG;
  const int i = blockIdx.x, t0 = blockIdx.y * tg, tid = threadIdx.x;
  const int F = rb->n_frames, ndof = rb->ndof;
  const int ng = min(tg, T - t0);
  extern __shared__ __attribute__((aligned(16))) double smem_hk[];
  const PlanCostLds m = plan_cost_lds<TG>(rb, smem_hk);
  int* s_cnt = reinterpret_cast<int*>(m.red);  // [4][TG]
  int* s_bad = s_cnt + 4 * TG;                 // [TG]
  if (tid < TG) s_bad[tid] = 0;
  __syncthreads();
  for (int idx = tid; idx < ng * ndof; idx += 256) {
    const int kq = idx / ndof, j = idx - kq * ndof;
    if (!isfinite(paths[((size_t)i * ndof + j) * T + t0 + kq])) s_bad[kq] = 1;
  }
  __syncthreads();
  plan_cost_kinematics<TG>(rb, m, ng, tid, [&](int kq, int dq) { return s_bad[kq] ? 0.0 : paths[((size_t)i * ndof + dq) * T + t0 + kq]; });
  double* s_E = m.screw;  // the kinematics' screws are done with: E_t [TG][12] (TG * screw_rows * 6 >= TG * 12 doubles)
  if (tid < ng * 12) s_E[tid] = held_frame_entry(rb, m.X, F, tid / 12, tid % 12);
  __syncthreads();
  if (base_pp) b0 = base_pp[3 * (size_t)i], b1 = base_pp[3 * (size_t)i + 1], b2 = base_pp[3 * (size_t)i + 2];
  const bool plan_ok = isfinite(b0) && isfinite(b1) && isfinite(b2) && bad_plan[i] == 0;
  const int nb = held_point_count(n_held, i, P_max);
  const int32_t lab = (DEPTH && labels) ? held_label[i] : 0;
  int cnt[TG];
#pragma unroll
  for (int g = 0; g < TG; ++g) cnt[g] = 0;
  for (int p0 = 0; p0 < P_max; p0 += 256) {  // uniform trip count: every lane takes part in the ballots
    const int p = p0 + tid;
    const bool row = p < P_max;
    const size_t o = ((size_t)i * P_max + (row ? p : 0)) * 3;
    const double x0 = held_p[o], x1 = held_p[o + 1], x2 = held_p[o + 2];
    const bool live = row && p < nb && isfinite(x0) && isfinite(x1) && isfinite(x2);
#pragma unroll
    for (int g = 0; g < TG; ++g) {
      if (g < ng) {
        const double* E = s_E + g * 12;
        const double X0 = (((E[0] * x0 + E[1] * x1) + E[2] * x2) + E[3]) + b0;
        const double X1 = (((E[4] * x0 + E[5] * x1) + E[6] * x2) + E[7]) + b1;
        const double X2 = (((E[8] * x0 + E[9] * x1) + E[10] * x2) + E[11]) + b2;
        if constexpr (DEPTH) {
          int pixel;
          const bool outside = depth_is_outside_at(X0, X1, X2, dv.depth, dv.H, dv.W, dv.K, dv.cam_inv, &pixel);
          bool in = live && !outside;  // (not outside: the pixel is in the image)
          if (in && labels) in = labels[pixel] != lab;
          cnt[g] += __popcll(__ballot(in));
        } else if (row) {
          double* w = xyz_out + (((size_t)i * T + t0 + g) * P_max + p) * 3;
          const bool ok = plan_ok && !s_bad[g];
          w[0] = ok ? (live ? X0 : NAN) : 0.0, w[1] = ok ? (live ? X1 : NAN) : 0.0, w[2] = ok ? (live ? X2 : NAN) : 0.0;
        }
      }
    }
  }
  if constexpr (DEPTH) {
    check_counts_to_lds<TG>(cnt, tid, s_cnt);
    __syncthreads();
    if (tid < ng)
      count_out[(size_t)i * T + t0 + tid] =
          (s_bad[tid] || !plan_ok) ? -1 : ((s_cnt[tid] + s_cnt[TG + tid]) + s_cnt[2 * TG + tid]) + s_cnt[3 * TG + tid];
  } else {
    if (tid < ng) count_out[(size_t)i * T + t0 + tid] = (s_bad[tid] || !plan_ok) ? -1 : 0;
  }
}
