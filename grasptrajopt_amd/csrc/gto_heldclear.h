// gto_heldclear.h — the held object's clearance from the robot's own links along a path (gto_held_clearance[_device]:
// include/gto_solver.h).  gto_check_held_paths judges the held points against the observation and gto_self_clearance the
// robot's links against each other; the pair neither sees is the object against the arm that carries it.  The reference
// has no counterpart: there a cracker box driven into the forearm shows when PyBullet executes the plan
// (examples/pybullet_gto_planning.py:301).
//
//   k_held_attach      (gto_held.h, unchanged) the held points in link_ee's frame at the grasp configuration, once per plan
//   k_held_clearance   one workgroup of four waves per (plan, up to GTO_CHECK_TG columns) in k_check_plans' LDS layout: the
//                      columns' kinematics once (plan_cost_kinematics), E_t of link_ee as k_check_held reads it, then column
//                      by column
//                        1. the world centres of the chunk spheres into LDS, as k_self_clearance puts them
//                        2. pass A: lane l holds held point Y = 64 j + l, the four waves share the enabled chunks; the least
//                           UPPER bound (|Y - c_k| + r_k + eps)^2, so that the running minimum starts low without a cutoff
//                        3. pass B: the gap |Y - c_k| - r_k - eps of every (held point, chunk) against the running minimum,
//                           a ballot, and for a chunk with a survivor its at most 64 world points, one per lane, read out of
//                           their lanes by v_readlane against every lane's own held point; FP64, no square root, no
//                           contraction
//                        4. lanes, then waves: the (d2, link, point) minimum in lexicographic order
// The result is a minimum over a set, and the culling only ever drops members that are strictly above it, so it depends
// neither on the order of the walk, nor on the waves, nor on the columns a workgroup takes.  Why a dropped pair is strictly
// above the answer (the point-against-sphere case of DESIGN.md 7z):
//   every point X of chunk k lies, in exact arithmetic, within r_k of the chunk's centre in the link's frame, and the
//   computed X and the computed centre c_k differ from the exact images under the link's transform by less than eps / 2
//   together (self_gap_eps: a thousand times the rounding of three products and sums, the square root's one rounding
//   included).  So the computed |Y - X| >= |Y - c_k| - r_k - eps = gap, for the very Y the exact compare uses.  A pair is
//   dropped only when gap > 0 and gap * gap >= bound, and the bound is never below the answer: it is c * c, or an upper
//   bound (|Y - c_k| + r_k + eps)^2 (1 + 2^-50) of a distance that some point of a non-empty enabled chunk attains, or a
//   squared distance that was computed.  The margin between gap and the true lower bound is a thousand roundings wide, so
//   the computed squared distance of a dropped pair is strictly above gap * gap >= bound >= the answer: it can neither be
//   the minimum nor tie with it, and the (link, point) of the minimum is safe too.
#pragma once
#include "gto_held.h"
#include "gto_selfcheck.h"

// doubles of LDS behind k_check_plans' layout: centres and radii [4][C], the four waves' minima (4 + 2 + 2), the running bound
__host__ __device__ inline int held_clearance_lds_doubles(int F, int L, int n, int C) {
  return check_plans_lds_doubles(F, L, n) + 4 * C + 10;
}

// Y_t[r] of the header: the held point carried by link_ee's frame, k_check_held's X_t without the final + base
__device__ __forceinline__ double held_carry(const double* __restrict__ E, double p0, double p1, double p2) {
#pragma clang fp contract(off)
  return ((E[0] * p0 + E[1] * p1) + E[2] * p2) + E[3];
}

// (d2, link, point) in lexicographic order
__device__ __forceinline__ bool held_key_less(double d, int l, int p, double bd, int bl, int bp) {
  return d < bd || (d == bd && (l < bl || (l == bl && p < bp)));
}

// paths [n][ndof][T]; tg: columns per workgroup, 1..GTO_CHECK_TG (grid (n, ceil(T / tg)); results do not depend on it).
// held_p [n][P_max][3], bad_plan [n]: what k_held_attach wrote (the plan's base and pose are judged there).  link_mask: bit l
// enables collision link l.  d2_out [n][T]; link_out, point_out [n][T] or null.  The robot's world point is
// k_self_clearance's expression, which is k_eval_points' at base 0, under the same contraction setting (gto_selfcheck.h).
__global__ __launch_bounds__(256) void k_held_clearance(const RobotDev* __restrict__ rb, const double* __restrict__ px,
                                                        const double* __restrict__ py, const double* __restrict__ pz,
                                                        const Chunk* __restrict__ chunks, int T, int tg,
                                                        const double* __restrict__ paths, const double* __restrict__ held_p,
                                                        int P_max, const int32_t* __restrict__ n_held,
                                                        const int32_t* __restrict__ bad_plan, uint32_t link_mask, double cutoff,
                                                        double* __restrict__ d2_out, int32_t* __restrict__ link_out,
                                                        int32_t* __restrict__ point_out) {
  constexpr int TG = GTO_CHECK_TG;
  const int i = blockIdx.x, t0 = blockIdx.y * tg, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = rb->n_links, ndof = rb->ndof, C = rb->n_chunks, F = rb->n_frames;
  const int ng = min(tg, T - t0);
  extern __shared__ __attribute__((aligned(16))) double smem_hc[];
  const PlanCostLds m = plan_cost_lds<TG>(rb, smem_hc);
  const double* s_vis = m.vis;
  int* s_bad = reinterpret_cast<int*>(m.red);  // [TG] at the start of the layout's `red` area, as in k_self_clearance
  double* s_cx = smem_hc + check_plans_lds_doubles(F, L, rb->n_opt);
  double *s_cy = s_cx + C, *s_cz = s_cy + C, *s_cr = s_cz + C;
  double* s_wd2 = s_cr + C;                                                        // [4] the waves' minima
  int* s_wlink = reinterpret_cast<int*>(s_wd2 + 4);                                // [4] (two doubles)
  int* s_wpoint = reinterpret_cast<int*>(s_wd2 + 6);                               // [4] (two doubles)
  unsigned long long* s_bound = reinterpret_cast<unsigned long long*>(s_wd2 + 8);  // bits of the running bound (squared)
  if (tid < TG) s_bad[tid] = 0;
  __syncthreads();
  for (int idx = tid; idx < ng * ndof; idx += 256) {
    const int kq = idx / ndof, j = idx - kq * ndof;
    if (!isfinite(paths[((size_t)i * ndof + j) * T + t0 + kq])) s_bad[kq] = 1;
  }
  __syncthreads();
  plan_cost_kinematics<TG>(rb, m, ng, tid, [&](int kq, int dq) { return s_bad[kq] ? 0.0 : paths[((size_t)i * ndof + dq) * T + t0 + kq]; });
  double* s_E = m.screw;  // the kinematics' screws are done with: E_t [TG][12], as in k_check_held
  if (tid < ng * 12) s_E[tid] = held_frame_entry(rb, m.X, F, tid / 12, tid % 12);
  __syncthreads();
  const bool plan_bad = bad_plan[i] != 0;
  const int nb = held_point_count(n_held, i, P_max);
  const int nblk = (nb + 63) >> 6;  // uniform trip count: every lane takes part in the ballots and the readlanes
  const double c2 = cutoff * cutoff;
  for (int g = 0; g < ng; ++g) {  // every branch below is workgroup-uniform
    const size_t o = (size_t)i * T + t0 + g;
    if (s_bad[g] || plan_bad) {
      if (tid == 0) {
        d2_out[o] = NAN;
        if (link_out) link_out[o] = -1;
        if (point_out) point_out[o] = -1;
      }
      continue;
    }
    const double* Vg = s_vis + (size_t)g * L * 12;
    const double* E = s_E + g * 12;
    for (int c = tid; c < C; c += 256) {
      const Chunk ch = chunks[c];
      const double* V = Vg + ch.link * 12;
      s_cx[c] = V[0] * ch.cx + V[1] * ch.cy + V[2] * ch.cz + V[3];
      s_cy[c] = V[4] * ch.cx + V[5] * ch.cy + V[6] * ch.cz + V[7];
      s_cz[c] = V[8] * ch.cx + V[9] * ch.cy + V[10] * ch.cz + V[11];
      s_cr[c] = ch.r;
    }
    if (tid == 0) *s_bound = __double_as_longlong(c2);
    __syncthreads();
    // ---- pass A: an upper bound of the answer from the spheres alone
    double ub2 = INFINITY;
    for (int j = 0; j < nblk; ++j) {
      const int p = 64 * j + lane;
      const size_t ho = ((size_t)i * P_max + (p < nb ? p : 0)) * 3;
      const double h0 = held_p[ho], h1 = held_p[ho + 1], h2 = held_p[ho + 2];
      const bool live = p < nb && isfinite(h0) && isfinite(h1) && isfinite(h2);
      const double Y0 = held_carry(E, h0, h1, h2), Y1 = held_carry(E + 4, h0, h1, h2), Y2 = held_carry(E + 8, h0, h1, h2);
      for (int c = wave; c < C; c += 4) {
        const Chunk ch = chunks[c];
        if (!((link_mask >> ch.link) & 1u) || ch.count < 1) continue;  // wave-uniform
        const double cx = s_cx[c], cy = s_cy[c], cz = s_cz[c];
        const double u = sqrt(self_d2(Y0 - cx, Y1 - cy, Y2 - cz)) + s_cr[c] + self_gap_eps(Y0, Y1, Y2, cx, cy, cz);
        if (live) ub2 = fmin(ub2, u * u * (1.0 + 0x1p-50));
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) ub2 = fmin(ub2, __shfl_xor(ub2, s));
    if (lane == 0) atomicMin(s_bound, (unsigned long long)__double_as_longlong(ub2));  // non-negative doubles order as their bits
    __syncthreads();
    // ---- pass B: sphere gaps against the running bound, the chunks with a survivor exactly
    double best = INFINITY;  // this lane's minimum, its link and its held point
    int blink = 0x7fffffff, bpoint = 0x7fffffff;
    for (int j = 0; j < nblk; ++j) {
      const int p = 64 * j + lane;
      const size_t ho = ((size_t)i * P_max + (p < nb ? p : 0)) * 3;
      const double h0 = held_p[ho], h1 = held_p[ho + 1], h2 = held_p[ho + 2];
      const bool live = p < nb && isfinite(h0) && isfinite(h1) && isfinite(h2);
      const double Y0 = held_carry(E, h0, h1, h2), Y1 = held_carry(E + 4, h0, h1, h2), Y2 = held_carry(E + 8, h0, h1, h2);
      for (int c = wave; c < C; c += 4) {
        const Chunk ch = chunks[c];
        if (!((link_mask >> ch.link) & 1u) || ch.count < 1) continue;  // wave-uniform
        const double bound = __longlong_as_double((long long)*(volatile unsigned long long*)s_bound);
        const double cx = s_cx[c], cy = s_cy[c], cz = s_cz[c];
        const double gap = sqrt(self_d2(Y0 - cx, Y1 - cy, Y2 - cz)) - s_cr[c] - self_gap_eps(Y0, Y1, Y2, cx, cy, cz);
        if (!__ballot(live && !(gap > 0.0 && gap * gap >= bound))) continue;  // wave-uniform
        // lane l computes point l of the chunk; every lane then meets all of them
        const double* Vb = Vg + ch.link * 12;
        const int pb = ch.start + (lane < ch.count ? lane : 0);
        const double b0 = px[pb], b1 = py[pb], b2 = pz[pb];
        const double B0 = Vb[0] * b0 + Vb[1] * b1 + Vb[2] * b2 + Vb[3];
        const double B1 = Vb[4] * b0 + Vb[5] * b1 + Vb[6] * b2 + Vb[7];
        const double B2 = Vb[8] * b0 + Vb[9] * b1 + Vb[10] * b2 + Vb[11];
        double mn = INFINITY;
        for (int k = 0; k < ch.count; ++k) {
          const double d2 = self_d2(Y0 - self_readlane(B0, k), Y1 - self_readlane(B1, k), Y2 - self_readlane(B2, k));
          mn = d2 < mn ? d2 : mn;
        }
        if (!live) mn = INFINITY;
        if (held_key_less(mn, ch.link, p, best, blink, bpoint)) best = mn, blink = ch.link, bpoint = p;
        if (__any(mn < bound)) {  // lower the bound for every wave; it never changes a result
          double w = mn;
#pragma unroll
          for (int s = 32; s >= 1; s >>= 1) w = fmin(w, __shfl_xor(w, s));
          if (lane == 0) atomicMin(s_bound, (unsigned long long)__double_as_longlong(w));
        }
      }
    }
    // ---- the lanes' and then the waves' minima: (d2, link, point) in lexicographic order
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double od = __shfl_xor(best, s);
      const int ol = __shfl_xor(blink, s), op = __shfl_xor(bpoint, s);
      if (held_key_less(od, ol, op, best, blink, bpoint)) best = od, blink = ol, bpoint = op;
    }
    if (lane == 0) s_wd2[wave] = best, s_wlink[wave] = blink, s_wpoint[wave] = bpoint;
    __syncthreads();
    if (tid == 0) {
      double d = s_wd2[0];
      int l = s_wlink[0], p = s_wpoint[0];
      for (int w = 1; w < 4; ++w)
        if (held_key_less(s_wd2[w], s_wlink[w], s_wpoint[w], d, l, p)) d = s_wd2[w], l = s_wlink[w], p = s_wpoint[w];
      const bool near = d < c2;
      d2_out[o] = near ? d : c2;
      if (link_out) link_out[o] = near ? l : -1;
      if (point_out) point_out[o] = near ? p : -1;
    }
    __syncthreads();  // the next column rewrites the centres and the bound
  }
}
