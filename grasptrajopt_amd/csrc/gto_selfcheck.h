// gto_selfcheck.h — the robot's clearance from itself along a path (gto_self_clearance: include/gto_solver.h).
// The reference has no counterpart: its solver has no self-collision term and nothing downstream of the solve looks for one;
// a plan that folds the arm into itself shows when PyBullet executes it (examples/pybullet_gto_planning.py:301).
//
//   k_self_clearance   one workgroup of four waves per (path, up to GTO_CHECK_TG columns) in k_check_plans' LDS layout: the
//                      columns' kinematics once (plan_cost_kinematics), then column by column
//                        1. the world centres of the chunk spheres into LDS (at most 256 chunks: 8 KB)
//                        2. pass A, one lane per chunk pair: the least UPPER bound (|ca - cb| + ra + rb)^2 over the enabled
//                           pairs, so that the running minimum starts low even without a cutoff
//                        3. pass B, one lane per chunk pair: the sphere gap |ca - cb| - ra - rb against the running minimum,
//                           a ballot, and one exact compare per surviving pair by the whole wave: lane l holds point l of
//                           chunk a, the points of chunk b come by v_readlane; FP64, no square root, no contraction
//                        4. the waves' (d2, 32 a + b) minima through LDS
// The result is a minimum over a set, and the culling only ever drops members that are strictly above it (self_gap_eps), so
// it depends neither on the order of the walk, nor on the waves, nor on the columns a workgroup takes.
#pragma once
#include "gto_observe.h"

// the pair mask of a call: bit b of rows[a] enables links (a, b); symmetric, zero diagonal (gto_set_self_pairs)
struct SelfPairs {
  uint32_t rows[GTO_MAX_LINKS];
};

// doubles of LDS behind k_check_plans' layout: centres and radii [4][C], the four waves' minima (4 + 2), the running bound
__host__ __device__ inline int self_clearance_lds_doubles(int F, int L, int n, int C) {
  return check_plans_lds_doubles(F, L, n) + 4 * C + 8;
}

// Widening of the sphere tests, metres.  A world point and a world centre are three products and three sums of terms no
// larger than |c|_1 + r each: an error of at most a few 2^-53 (|c|_1 + r) per coordinate against the exact image under the
// link's transform, and the computed rotation is orthogonal to a few 2^-53 as well, which moves a point of the sphere by as
// much times r.  2^-40 of the two centres' 1-norms is a thousand times that; the constant covers centres at the origin and
// the one rounding of the square root.
__device__ __forceinline__ double self_gap_eps(double ax, double ay, double az, double bx, double by, double bz) {
  return 1e-9 + 0x1p-40 * (((fabs(ax) + fabs(ay)) + fabs(az)) + ((fabs(bx) + fabs(by)) + fabs(bz)));
}

__device__ __forceinline__ double self_readlane(double v, int j) {
  union {
    double d;
    int i[2];
  } u;
  u.d = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], j);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], j);
  return u.d;
}

// the squared distance of the statistic: products and sums, one rounding each
__device__ __forceinline__ double self_d2(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  return (dx * dx + dy * dy) + dz * dz;
}

// paths [n][ndof][T]; tg: columns per workgroup, 1..GTO_CHECK_TG (grid (n, ceil(T / tg)); results do not depend on it).
// d2_out [n][T], pair_out [n][T][2].  The world point is k_eval_points' expression, term for term, at base 0: the same
// source expression under the same contraction setting as k_eval_points, k_check_plans and k_check_held, which is what makes
// the bits equal (the compiler fuses all of them alike; tests/test_gpu_self_clearance.py compares with gto_eval_points'
// xyz_out on every run).  A shared explicit fma chain would remove the dependence, but would change those kernels.
__global__ __launch_bounds__(256) void k_self_clearance(const RobotDev* __restrict__ rb, const double* __restrict__ px,
                                                        const double* __restrict__ py, const double* __restrict__ pz,
                                                        const Chunk* __restrict__ chunks, int T, int tg,
                                                        const double* __restrict__ paths, SelfPairs mask, double cutoff,
                                                        double* __restrict__ d2_out, int32_t* __restrict__ pair_out) {
  constexpr int TG = GTO_CHECK_TG;
  const int i = blockIdx.x, t0 = blockIdx.y * tg, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = rb->n_links, ndof = rb->ndof, C = rb->n_chunks, F = rb->n_frames;
  const int ng = min(tg, T - t0);
  extern __shared__ __attribute__((aligned(16))) double smem_sc[];
  const PlanCostLds m = plan_cost_lds<TG>(rb, smem_sc);
  const double* s_vis = m.vis;
  // [TG] at the start of the layout's `red` area (16 doubles).  k_check_plans keeps its flags behind its [4][TG] counts there;
  // this kernel has no counts, its own reductions live behind the layout (s_wd2 ...), and plan_cost_kinematics never
  // touches `red`, so the flags sit at its start.
  int* s_bad = reinterpret_cast<int*>(m.red);
  double* s_cx = smem_sc + check_plans_lds_doubles(F, L, rb->n_opt);
  double *s_cy = s_cx + C, *s_cz = s_cy + C, *s_cr = s_cz + C;
  double* s_wd2 = s_cr + C;                                             // [4] the waves' minima
  int* s_wcode = reinterpret_cast<int*>(s_wd2 + 4);                     // [4] (two doubles)
  unsigned long long* s_bound = reinterpret_cast<unsigned long long*>(s_wd2 + 6);  // bits of the running bound (squared)
  if (tid < TG) s_bad[tid] = 0;
  __syncthreads();
  for (int idx = tid; idx < ng * ndof; idx += 256) {
    const int kq = idx / ndof, j = idx - kq * ndof;
    if (!isfinite(paths[((size_t)i * ndof + j) * T + t0 + kq])) s_bad[kq] = 1;
  }
  __syncthreads();
  plan_cost_kinematics<TG>(rb, m, ng, tid, [&](int kq, int dq) { return s_bad[kq] ? 0.0 : paths[((size_t)i * ndof + dq) * T + t0 + kq]; });
  const double c2 = cutoff * cutoff;
  const int NB = (C + 62) / 64;  // blocks of 64 partners cb = ca + 1 + 64 j + lane of a chunk ca
  const int n_items = C * NB;
  for (int g = 0; g < ng; ++g) {  // every branch below is workgroup-uniform
    const size_t o = (size_t)i * T + t0 + g;
    if (s_bad[g]) {
      if (tid == 0) d2_out[o] = NAN, pair_out[2 * o] = -1, pair_out[2 * o + 1] = -1;
      continue;
    }
    const double* Vg = s_vis + (size_t)g * L * 12;
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
    for (int it = wave; it < n_items; it += 4) {
      const int ca = it / NB, cb = ca + 1 + 64 * (it - ca * NB) + lane;
      if (cb < C) {
        const int la = chunks[ca].link, lb = chunks[cb].link;
        if ((mask.rows[la] >> lb) & 1u) {
          const double ax = s_cx[ca], ay = s_cy[ca], az = s_cz[ca], bx = s_cx[cb], by = s_cy[cb], bz = s_cz[cb];
          const double u = sqrt(self_d2(ax - bx, ay - by, az - bz)) + (s_cr[ca] + s_cr[cb]) + self_gap_eps(ax, ay, az, bx, by, bz);
          ub2 = fmin(ub2, u * u * (1.0 + 0x1p-50));
        }
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) ub2 = fmin(ub2, __shfl_xor(ub2, s));
    if (lane == 0) atomicMin(s_bound, (unsigned long long)__double_as_longlong(ub2));  // non-negative doubles order as their bits
    __syncthreads();
    // ---- pass B: sphere gaps against the running bound, the survivors exactly
    double best = INFINITY;  // this lane's minimum and its pair code 32 a + b
    int bcode = 0x7fffffff;
    for (int it = wave; it < n_items; it += 4) {
      const int ca = it / NB, cb = ca + 1 + 64 * (it - ca * NB) + lane;
      if (ca + 1 + 64 * (it - ca * NB) >= C) continue;  // wave-uniform
      const Chunk cha = chunks[ca];
      const double bound = __longlong_as_double((long long)*(volatile unsigned long long*)s_bound);
      bool live = false;
      if (cb < C) {
        const int lb = chunks[cb].link;
        if ((mask.rows[cha.link] >> lb) & 1u) {
          const double ax = s_cx[ca], ay = s_cy[ca], az = s_cz[ca], bx = s_cx[cb], by = s_cy[cb], bz = s_cz[cb];
          const double gap = sqrt(self_d2(ax - bx, ay - by, az - bz)) - (s_cr[ca] + s_cr[cb]) - self_gap_eps(ax, ay, az, bx, by, bz);
          live = !(gap > 0.0 && gap * gap >= bound);
        }
      }
      unsigned long long todo = __ballot(live);
      if (!todo) continue;
      // lane l holds point l of chunk a
      const double* Va = Vg + cha.link * 12;
      const bool in_a = lane < cha.count;
      const int pa = cha.start + (in_a ? lane : 0);
      const double a0 = px[pa], a1 = py[pa], a2 = pz[pa];
      const double A0 = Va[0] * a0 + Va[1] * a1 + Va[2] * a2 + Va[3];
      const double A1 = Va[4] * a0 + Va[5] * a1 + Va[6] * a2 + Va[7];
      const double A2 = Va[8] * a0 + Va[9] * a1 + Va[10] * a2 + Va[11];
      while (todo) {
        const int k = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int cbu = __builtin_amdgcn_readfirstlane(ca + 1 + 64 * (it - ca * NB) + k);
        const Chunk chb = chunks[cbu];
        const double* Vb = Vg + chb.link * 12;
        const int pb = chb.start + (lane < chb.count ? lane : 0);
        const double b0 = px[pb], b1 = py[pb], b2 = pz[pb];
        const double B0 = Vb[0] * b0 + Vb[1] * b1 + Vb[2] * b2 + Vb[3];
        const double B1 = Vb[4] * b0 + Vb[5] * b1 + Vb[6] * b2 + Vb[7];
        const double B2 = Vb[8] * b0 + Vb[9] * b1 + Vb[10] * b2 + Vb[11];
        double mn = INFINITY;
        for (int j = 0; j < chb.count; ++j) {
          const double d2 = self_d2(A0 - self_readlane(B0, j), A1 - self_readlane(B1, j), A2 - self_readlane(B2, j));
          mn = d2 < mn ? d2 : mn;
        }
        if (!in_a) mn = INFINITY;
        const int code = 32 * cha.link + chb.link;
        if (mn < best || (mn == best && code < bcode)) best = mn, bcode = code;
        if (__any(mn < bound)) {  // lower the bound for every wave; it never changes a result
          double w = mn;
#pragma unroll
          for (int s = 32; s >= 1; s >>= 1) w = fmin(w, __shfl_xor(w, s));
          if (lane == 0) atomicMin(s_bound, (unsigned long long)__double_as_longlong(w));
        }
      }
    }
    // ---- the waves' minima: (d2, code) in lexicographic order
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double od = __shfl_xor(best, s);
      const int oc = __shfl_xor(bcode, s);
      if (od < best || (od == best && oc < bcode)) best = od, bcode = oc;
    }
    if (lane == 0) s_wd2[wave] = best, s_wcode[wave] = bcode;
    __syncthreads();
    if (tid == 0) {
      double d = s_wd2[0];
      int code = s_wcode[0];
      for (int w = 1; w < 4; ++w)
        if (s_wd2[w] < d || (s_wd2[w] == d && s_wcode[w] < code)) d = s_wd2[w], code = s_wcode[w];
      const bool near = d < c2;
      d2_out[o] = near ? d : c2;
      pair_out[2 * o] = near ? code >> 5 : -1;
      pair_out[2 * o + 1] = near ? code & 31 : -1;
    }
    __syncthreads();  // the next column rewrites the centres and the bound
  }
}
