// gto_retime.h — time-optimal retiming of paths under joint velocity and acceleration limits (gto_retime_paths[_device]
// and gto_retime_batch[_device], include/gto_solver.h).  The reference's convert_plan_to_trajectory_toppra
// (gto/utils.py:283-323): a not-a-knot cubic spline through the C waypoints of a path on s in [0, 1] (C per path: the
// first n_cols[b] of the Tp columns a row holds), TOPP-RA's discretisation on a grid of N = subdiv (C-1) + 1 points
// (x = sdot^2, u = sddot, x_{i+1} = x_i + 2 Delta u_i, constraints at the gridpoints), the controllable sets by a backward
// pass, the greedy forward pass, constant acceleration between gridpoints, M samples of q, qdot, qddot.  FP64 throughout.
//
//   k_retime_spline   one lane per (plan, joint): slopes of the spline at the knots (the two substitutions of the
//                     not-a-knot system, factored once per handle on the host for every count at once; the last row's
//                     three factors per lane), the parabola at C = 3, the chord at C = 2, finite / moving flags
//   k_retime_grid     one lane per (plan, gridpoint): p1 = q'(s), p2 = q''(s) of every joint, the bound on x that does
//                     not involve u (velocity limits; acceleration limits of joints with p1 = 0)
//   k_retime_pass     one wave per plan: backward pass (controllable sets) and forward pass (greedy profile), times.
//                     Each stage is a two-variable LP solved exactly: every upper bound on u (a line in x) is paired with
//                     every lower bound, and the pairs are spread over the lanes and reduced by a cross-lane min.  One
//                     lane per plan (every pair in one lane) measured 0.6-0.1x of this rate and was dropped.
//   k_retime_convex   one wave per plan, in place of k_retime_pass for gto_retime_paths_convex[_device]: the time optimum of
//                     the same grid constraints by a log-barrier Newton method (below, beside the pass)
//   k_retime_torque_rows, k_retime_convex_torque, k_retime_tau   gto_retime_paths_torque[_device]: the inverse dynamics'
//                     coefficients along the path (three rt_rnea passes per gridpoint), the same Newton method with the joint
//                     torque rows added, the joint forces at the samples
//   k_retime_sample   one lane per (plan, sample): binary search over the gridpoint times, evaluation on the spline
// Rows are laid out for the largest count: paths and slopes [B][ndof][Tp], grid arrays [B][Nmax], Nmax = subdiv (Tp-1) + 1.
// Nothing a path's arithmetic uses depends on Tp or on its place in the batch.
#pragma once
#include "gto_device.h"
#include "gto_dynamics.h"

#define GTO_RETIME_MAX_N 1024             // gridpoints per plan (the pass kernel keeps the controllable sets in LDS)
#define GTO_RETIME_LINES (GTO_MAX_DOF + 1)  // bounds on u of each side: one per moving joint, one from the next set
// A profile that rests over a whole segment (x at both of its ends <= GTO_RETIME_STALL * the largest x, i.e. sdot below
// 1e-3 of its largest) spends a time on it that round-off of x alone decides: status GTO_STATUS_NUMERICAL
#define GTO_RETIME_STALL 1e-6

// per-joint limits, passed by value (a kernel argument of 512 B): no upload, no validation on the device
struct RetimeLimits {
  double vmax[GTO_MAX_DOF];  // > 0, +inf = no limit
  double amax[GTO_MAX_DOF];  // finite, > 0
};

struct RetimeDims {
  int B, ndof, Tp, Nmax, subdiv, M;  // Tp columns per row, Nmax = subdiv (Tp-1) + 1 gridpoints per row
};

// rows of the factor table, each GTO_RETIME_MAX_N long (retime_factors, gto_api.hip)
#define GTO_RT_FAC_LO 0
#define GTO_RT_FAC_INV 1
#define GTO_RT_FAC_UP 2
#define GTO_RT_FAC_PIV 3

// Columns of path b: n_cols[b] (NULL: Tp).  A count outside [1, Tp] is a device value no host has seen: 0, and the path
// is flagged GTO_RT_NONFINITE by the spline kernel, so that nothing downstream indexes with it.
__device__ __forceinline__ int rt_cols(const int32_t* __restrict__ n_cols, long long b, int Tp) {
  const int C = n_cols ? n_cols[b] : Tp;
  return C >= 1 && C <= Tp ? C : 0;
}

// flags of a (plan, joint) row
#define GTO_RT_CONST 0
#define GTO_RT_MOVING 1
#define GTO_RT_NONFINITE 2

// Cubic piece of knot interval k at offset r in [0, h]: scipy.interpolate.CubicSpline's coefficients from the values and
// slopes at both ends (c0 r^3 + c1 r^2 + c2 r + c3).  Returns q, q' and q''.
__device__ __forceinline__ void rt_piece(const double* y, const double* s, int k, double r, double invh, double& q,
                                         double& p1, double& p2) {
  const double y0 = y[k], y1 = y[k + 1], s0 = s[k], s1 = s[k + 1];
  const double m = (y1 - y0) * invh;
  const double t = (s0 + s1 - 2.0 * m) * invh;
  const double c0 = t * invh, c1 = (m - s0) * invh - t, c2 = s0;
  q = y0 + r * (c2 + r * (c1 + r * c0));
  p1 = c2 + r * (2.0 * c1 + 3.0 * c0 * r);
  p2 = 2.0 * c1 + 6.0 * c0 * r;
}

// Spline slopes of scipy's CubicSpline(..., bc_type="not-a-knot") through the C waypoints of a row.
// C >= 4: fac [4][GTO_RETIME_MAX_N], the Thomas factors of the not-a-knot system scaled by 1/h (rows [1 2], [1 4 1] ...):
// multiplier, reciprocal pivot, upper entry and pivot of row i as if it were an interior row, which rows 0..C-2 are for
// every C.  The last row [2 1] is eliminated here, in retime_factors' order of operations (a division, a product and a
// difference, a division: each rounded once, so the three values are the ones a table for this C alone would hold).
// C == 3: the parabola through the three waypoints; C == 2: the chord (rt_piece then has c0 = c1 = 0 exactly, p2 = 0);
// C == 1: slope 0.
__global__ __launch_bounds__(256) void k_retime_spline(const double* __restrict__ Q, const double* __restrict__ fac,
                                                       const int32_t* __restrict__ n_cols, RetimeDims d,
                                                       double* __restrict__ S, int32_t* __restrict__ flag) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)d.B * d.ndof) return;
  const int C = rt_cols(n_cols, id / d.ndof, d.Tp);
  if (C == 0) {
    flag[id] = GTO_RT_NONFINITE;
    return;
  }
  const double* y = Q + id * d.Tp;
  double* s = S + id * d.Tp;
  const double invh = (double)(C - 1);
  bool finite = true, moving = false;
  const double y0 = y[0];
  for (int k = 0; k < C; ++k) {
    finite = finite && isfinite(y[k]);
    moving = moving || y[k] != y0;
  }
  flag[id] = !finite ? GTO_RT_NONFINITE : moving ? GTO_RT_MOVING : GTO_RT_CONST;
  if (!finite) return;
  if (C == 1) {
    s[0] = 0.0;
    return;
  }
  double mprev = (y[1] - y[0]) * invh;
  if (C == 2) {
    s[0] = mprev, s[1] = mprev;
    return;
  }
  double mcur = (y[2] - y[1]) * invh;
  if (C == 3) {
    s[0] = 0.5 * (3.0 * mprev - mcur), s[1] = 0.5 * (mprev + mcur), s[2] = 0.5 * (3.0 * mcur - mprev);
    return;
  }
  const double* lo = fac + GTO_RT_FAC_LO * GTO_RETIME_MAX_N;
  const double* inv = fac + GTO_RT_FAC_INV * GTO_RETIME_MAX_N;
  const double* up = fac + GTO_RT_FAC_UP * GTO_RETIME_MAX_N;
  const double lo_last = 2.0 / fac[GTO_RT_FAC_PIV * GTO_RETIME_MAX_N + C - 2];
  const double inv_last = 1.0 / __dsub_rn(1.0, __dmul_rn(lo_last, up[C - 2]));
  // forward substitution into s; right-hand sides from the chord slopes m_k
  double w = 0.5 * (5.0 * mprev + mcur);
  s[0] = w;
  for (int i = 1; i < C - 1; ++i) {
    if (i > 1) mprev = mcur, mcur = (y[i + 1] - y[i]) * invh;
    w = 3.0 * (mprev + mcur) - lo[i] * w;
    s[i] = w;
  }
  w = 0.5 * (mprev + 5.0 * mcur) - lo_last * w;
  // back substitution
  double sn = w * inv_last;
  s[C - 1] = sn;
  for (int i = C - 2; i >= 0; --i) {
    sn = (s[i] - up[i] * sn) * inv[i];
    s[i] = sn;
  }
}

// Bound on u of moving joint j at gridpoint i: upper u <= alpha + beta x, lower u >= -alpha + beta x.  A joint with p1 = 0,
// or with |p1| so small that alpha or beta overflows, has no line (its bound on x alone, |p2 x| <= amax, is in xcap):
// alpha = inf, beta = 0 makes every pair with it void.  Returns whether the joint has a line.
__device__ __forceinline__ bool rt_line(double a, double b, double A, double& alpha, double& beta) {
  alpha = A / fabs(a);
  beta = -b / a;
  if (isfinite(alpha) && isfinite(beta)) return true;
  alpha = INFINITY, beta = 0.0;
  return false;
}

// p1, p2 per (plan, gridpoint, joint) [B][Nmax][ndof] and the x cap per (plan, gridpoint) [B][Nmax]; the points past a
// path's own N = subdiv (C-1) + 1 are left alone (nobody reads them)
__global__ __launch_bounds__(256) void k_retime_grid(const double* __restrict__ Q, const double* __restrict__ S,
                                                     const int32_t* __restrict__ flag, const int32_t* __restrict__ n_cols,
                                                     RetimeLimits lim, RetimeDims d, double* __restrict__ P1,
                                                     double* __restrict__ P2, double* __restrict__ xcap) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)d.B * d.Nmax) return;
  const long long b = id / d.Nmax;
  const int g = (int)(id - b * d.Nmax), T = d.Tp, ndof = d.ndof;
  const int C = rt_cols(n_cols, b, T), N = d.subdiv * (C - 1) + 1;
  if (C == 0 || g >= N) return;
  const int k = max(min(g / d.subdiv, C - 2), 0);  // C == 1: no row is moving, rt_piece is not called
  const double r = (double)(g - k * d.subdiv) / (double)(N - 1);
  const double invh = (double)(C - 1);
  double cap = INFINITY;
  for (int j = 0; j < ndof; ++j) {
    const long long row = b * ndof + j;
    double p1 = 0.0, p2 = 0.0;
    if (flag[row] == GTO_RT_NONFINITE) {
      cap = NAN;
    } else if (flag[row] == GTO_RT_MOVING) {
      double q;
      rt_piece(Q + row * T, S + row * T, k, r, invh, q, p1, p2);
      if (p1 != 0.0 && isfinite(lim.vmax[j])) {
        const double v = lim.vmax[j] / fabs(p1);
        cap = fmin(cap, v * v);
      }
      double al, bl;
      if (!rt_line(p1, p2, lim.amax[j], al, bl) && p2 != 0.0 && g < N - 1)  // |p2 x| <= amax: a bound on x alone
        cap = fmin(cap, lim.amax[j] / fabs(p2));
    }
    P1[id * ndof + j] = p1;
    P2[id * ndof + j] = p2;
  }
  xcap[id] = cap;
}

__device__ __forceinline__ double rt_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

// x at which upper line (au, bu) falls below lower line (al, bl); inf if it never does for x >= 0
__device__ __forceinline__ double rt_pair(double au, double bu, double al, double bl) {
  const double db = bl - bu;
  return db > 0.0 ? (au - al) / db : INFINITY;
}

// One wave per plan.  Lines 0..nm-1: the moving joints (mj); line nm: the link to the next gridpoint,
// upper u <= (X_{i+1} - x) / (2 Delta), lower u >= -x / (2 Delta).  Both passes run over the plan's own N gridpoints; the
// outputs past them hold the duration and 0 (the path has ended and rests).
__global__ __launch_bounds__(64) void k_retime_pass(const double* __restrict__ P1, const double* __restrict__ P2,
                                                    const double* __restrict__ xcap, const int32_t* __restrict__ flag,
                                                    const int32_t* __restrict__ n_cols, RetimeLimits lim, RetimeDims d,
                                                    double* __restrict__ X, double* __restrict__ Tg,
                                                    int32_t* __restrict__ stat, double* __restrict__ duration_out,
                                                    double* __restrict__ t_out, double* __restrict__ sd_out,
                                                    int32_t* __restrict__ status_out) {
  __shared__ double xmax[GTO_RETIME_MAX_N];
  __shared__ double la[GTO_RETIME_LINES], lb[GTO_RETIME_LINES];
  __shared__ int mj[GTO_MAX_DOF];
  const long long b = blockIdx.x;
  const int lane = threadIdx.x, ndof = d.ndof;
  const int N = d.subdiv * (rt_cols(n_cols, b, d.Tp) - 1) + 1;  // a bad count is flagged: N is not used then
  const int f = lane < ndof ? flag[b * ndof + lane] : GTO_RT_CONST;
  const unsigned long long bad = __ballot(f == GTO_RT_NONFINITE), mov = __ballot(f == GTO_RT_MOVING);
  const long long o = b * d.Nmax;
  if (bad) {
    for (int i = lane; i < d.Nmax; i += 64) {
      X[o + i] = NAN, Tg[o + i] = NAN;
      if (t_out) t_out[o + i] = NAN;
      if (sd_out) sd_out[o + i] = NAN;
    }
    if (lane == 0) {
      stat[b] = GTO_STATUS_NUMERICAL;
      if (duration_out) duration_out[b] = NAN;
      if (status_out) status_out[b] = GTO_STATUS_NUMERICAL;
    }
    return;
  }
  const int nm = __popcll(mov), nl = nm + 1;
  if (f == GTO_RT_MOVING) mj[__popcll(mov & ((1ull << lane) - 1ull))] = lane;
  const double c2d = 0.5 * (double)(N - 1), twoD = 2.0 / (double)(N - 1);
  const double* p1 = P1 + o * ndof;
  const double* p2 = P2 + o * ndof;
  __syncthreads();
  // backward pass: K_{N-1} = {0}, K_i = [0, xmax_i]
  double Xn = 0.0;
  if (lane == 0) xmax[N - 1] = 0.0;
  if (nm > 0)
    for (int i = N - 2; i >= 0; --i) {
      if (lane < nm) {
        const int j = mj[lane];
        double al, bl;
        rt_line(p1[(long long)i * ndof + j], p2[(long long)i * ndof + j], lim.amax[j], al, bl);
        la[lane] = al, lb[lane] = bl;
      } else if (lane == nm) {
        la[lane] = Xn * c2d, lb[lane] = -c2d;
      }
      __syncthreads();
      double best = INFINITY;
      int k = lane / nl, m = lane - k * nl;
      for (int p = lane; p < nl * nl; p += 64) {
        best = fmin(best, rt_pair(la[k], lb[k], m == nm ? 0.0 : -la[m], lb[m]));
        for (m += 64; m >= nl; m -= nl) ++k;
      }
      best = rt_wave_min(best);
      Xn = fmax(0.0, fmin(xcap[o + i], best));
      if (lane == 0) xmax[i] = Xn;
      __syncthreads();
    }
  // forward pass: x_0 = 0, u_i = the smallest upper bound at x_i, x_{i+1} clamped into K_{i+1}; times on the way
  double x = 0.0, t = 0.0, xtop = 0.0, rest = INFINITY;  // largest x; smallest max(x_i, x_{i+1}) over the segments
  if (lane == 0) {
    X[o] = 0.0, Tg[o] = 0.0;
    if (t_out) t_out[o] = 0.0;
    if (sd_out) sd_out[o] = 0.0;
  }
  for (int i = 0; i < N - 1; ++i) {
    double xn = 0.0;
    if (nm > 0) {
      const double Xi1 = xmax[i + 1];
      double cand = INFINITY;
      if (lane < nm) {
        const int j = mj[lane];
        double al, bl;
        rt_line(p1[(long long)i * ndof + j], p2[(long long)i * ndof + j], lim.amax[j], al, bl);
        cand = fma(bl, x, al);
      } else if (lane == nm) {
        cand = fma(-c2d, x, Xi1 * c2d);
      }
      const double u = rt_wave_min(cand);
      xn = fmin(fmax(fma(u, twoD, x), 0.0), Xi1);
      t += twoD / (sqrt(x) + sqrt(xn));
      xtop = fmax(xtop, xn);
      rest = fmin(rest, fmax(x, xn));
    }
    x = xn;
    if (lane == 0) {
      X[o + i + 1] = x, Tg[o + i + 1] = t;
      if (t_out) t_out[o + i + 1] = t;
      if (sd_out) sd_out[o + i + 1] = sqrt(x);
    }
  }
  for (int i = N + lane; i < d.Nmax; i += 64) {
    if (t_out) t_out[o + i] = t;
    if (sd_out) sd_out[o + i] = 0.0;
  }
  if (lane == 0) {
    const bool stall = nm > 0 && rest <= GTO_RETIME_STALL * xtop;
    const int32_t s = isfinite(t) && !stall ? GTO_STATUS_CONVERGED : GTO_STATUS_NUMERICAL;
    stat[b] = s;
    if (duration_out) duration_out[b] = t;
    if (status_out) status_out[b] = s;
  }
}

// ------------------------------------------------------------------ the grid's time optimum (gto_retime_paths_convex)
// k_retime_convex stands where k_retime_pass stands: the same inputs from k_retime_spline / k_retime_grid, the same X, Tg
// and stat for k_retime_sample.  It minimises T(x) = sum_i 2 Delta / (sqrt x_i + sqrt x_{i+1}) over x_1 .. x_{N-2}
// (x_0 = x_{N-1} = 0) under 0 <= x_i <= xcap_i and, for every line (alpha, beta) of gridpoint i <= N-2,
// |r| <= alpha with r = c (x_{i+1} - x_i) - beta x_i, c = (N-1)/2, by a log-barrier path-following Newton method:
//   F_mu(x) = T(x) - mu sum_rows log(slack);  every term couples x_i and x_{i+1} only, so the Hessian is symmetric
//   tridiagonal and positive definite.  A step: assemble (one lane per variable, which gathers the rows of the segments on
//   both of its sides, so that nothing is added across lanes), factor and solve, the largest step that stays strictly inside
//   (wave-min), backtracking on F_mu (wave-sums in a fixed order: a plan's result does not depend on its batch).
//   lam^2 = g' H^-1 g / mu is the Newton decrement of F_mu / mu.  At lam < GTO_RT_CENTRED the iterate counts as centred:
//   the gap bound mu (m + (lam + sqrt m) lam / (1 - lam)), m rows (m mu at the centre itself), is compared with
//   gap_tol T(x), and either the solve ends or mu shrinks by GTO_RT_SHRINK.
#define GTO_RT_CENTRED 0.25
#define GTO_RT_SHRINK 0.1
#define GTO_RT_ARMIJO 1e-4
#define GTO_RT_BACKTRACKS 60

#define GTO_RT_LDS_ARRAYS 5  // LDS arrays of Nmax doubles each: 40 KB at Nmax = 1024

struct RetimeConvex {
  double gap_tol;  // finite, > 0
  int max_newton;  // >= 1
};

__device__ __forceinline__ double rt_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Joint torque limits of gto_retime_paths_torque, passed by value like RetimeLimits
struct RetimeTorque {
  double tau_max[GTO_MAX_DOF];  // > 0, +inf = no limit
};
// the torque coefficients of k_retime_torque_rows [Nmax][ndof] of one path (null in the instantiation without them)
struct RetimeTorqueRows {
  const double *ta, *tb, *tg;
};

// Torque row of gridpoint i and joint j (k = i ndof + j) on the interior variables: tau = A1 x_{i+1} + K x_i + g within
// -+ tmax, A1 = a c (0 where x_{i+1} is the end, in1 false), K = b - a c (0 where x_i is the start, in0 false).  Returns
// whether the row is part of the program: a joint without a limit has none, and neither has a row that holds no variable.
__device__ __forceinline__ bool rt_torque_row(const RetimeTorqueRows& tr, long long k, double c, bool in0, bool in1, double tmax,
                                              double& A1, double& K) {
  if (tmax == INFINITY) return false;
  const double ac = tr.ta[k] * c;
  A1 = in1 ? ac : 0.0;
  K = in0 ? tr.tb[k] - ac : 0.0;
  return A1 != 0.0 || K != 0.0;
}

// The row's torque at (x_i, x_{i+1}) = (xi, xn): a c (xn - xi) + b xi + g, which is A1 xn + K xi + g wherever a mask is off
// (x_0 = x_{N-1} = 0).  Written with the difference first and explicit fmas: A1 xn and K xi are each N/2 times the torque and
// cancel, and a slack of 1e-11 tau_max would be lost in their round-off; and every site that evaluates a row (the barrier
// sum, both neighbouring variables' gathers, the step room) gets the same bits, so that the 2x2 block a row adds to the
// Hessian stays the rank-one matrix it is.
__device__ __forceinline__ double rt_torque_tau(const RetimeTorqueRows& tr, long long k, double c, double xi, double xn) {
  return fma(tr.ta[k] * c, xn - xi, fma(tr.tb[k], xi, tr.tg[k]));
}

// T and the barrier sum phi = -sum log(slack) at y = x + eta dx (F_mu = T + mu phi); T = inf where y is not strictly
// inside.  Gridpoint i owns its segment's time, its own two box rows, its lines and (TORQUE) its torque rows.
template <bool TORQUE>
__device__ __forceinline__ void rt_convex_eval(const double* x, const double* dx, double eta, const double* al,
                                               const double* be, const double* cap, int N, int ndof, int lane, double& T,
                                               double& phi, const RetimeTorque& tq, const RetimeTorqueRows& tr) {
  const double c = 0.5 * (double)(N - 1), w = 2.0 / (double)(N - 1);
  double Tl = 0.0, ph = 0.0;
  bool in = true;
  for (int i = lane; i < N - 1; i += 64) {
    const double yi = fma(eta, dx[i], x[i]), yn = fma(eta, dx[i + 1], x[i + 1]);
    Tl += w / (sqrt(yi) + sqrt(yn));
    if (i >= 1) {
      in = in && yi > 0.0;
      ph -= log(yi);
      const double cp = cap[i];
      if (cp != INFINITY) {
        in = in && cp - yi > 0.0;
        ph -= log(cp - yi);
      }
    }
    for (int j = 0; j < ndof; ++j) {
      const double a = al[(long long)i * ndof + j];
      if (a == INFINITY) continue;
      const double r = c * (yn - yi) - be[(long long)i * ndof + j] * yi;
      in = in && a - r > 0.0 && a + r > 0.0;
      ph -= log(a - r) + log(a + r);
    }
    if constexpr (TORQUE)
      for (int j = 0; j < ndof; ++j) {
        const double tm = tq.tau_max[j];
        double A1, K;
        if (!rt_torque_row(tr, (long long)i * ndof + j, c, i >= 1, i + 1 <= N - 2, tm, A1, K)) continue;
        const double r = rt_torque_tau(tr, (long long)i * ndof + j, c, yi, yn);
        in = in && tm - r > 0.0 && tm + r > 0.0;
        ph -= log(tm - r) + log(tm + r);
      }
  }
  T = rt_wave_sum(in ? Tl : INFINITY);
  phi = rt_wave_sum(ph);
}

// H dx = -g for variables 1 .. n, H = tridiag(e, dg, e) (e[v] couples v and v+1).  dg and g are overwritten by the pivots
// and the reduced right-hand side of the L D L' factorisation, which is what the Newton decrement sums: g' H^-1 g =
// sum g[v]^2 / dg[v].
__device__ __forceinline__ void rt_tridiag_serial(double* dg, const double* e, double* g, double* dx, int n, int lane) {
  if (lane == 0) {
    double dp = dg[1], gp = g[1];
    for (int v = 2; v <= n; ++v) {
      const double ev = e[v - 1], m = ev / dp;
      dp = dg[v] - m * ev;
      gp = g[v] - m * gp;
      dg[v] = dp, g[v] = gp;
    }
    double s = -gp / dp;
    dx[n] = s;
    for (int v = n - 1; v >= 1; --v) {
      s = (-g[v] - e[v] * s) / dg[v];
      dx[v] = s;
    }
  }
}

// One wave per plan.  al / be: p1 / p2 of k_retime_grid [B][Nmax][ndof] on entry; the kernel turns them into the lines
// (alpha, beta) of rt_line in place, once, and reads those in every Newton step (alpha = inf: no line).  LDS: five arrays of
// Nmax doubles (x, gradient, diagonal, off-diagonal, step; GTO_RT_LDS_ARRAYS), passed as the launch's dynamic size.
// stat: what k_retime_sample asks, "has a profile" (GTO_STATUS_CONVERGED for GTO_STATUS_MAX_ITER too, whose feasible
// profile is sampled); status_out: the status of the contract.
// TORQUE (k_retime_convex_torque, gto_retime_paths_torque): the torque rows of k_retime_torque_rows join the program --
// TA, TB, TG [B][Nmax][ndof], tau = TA u + TB x + TG at every gridpoint i <= N-2 within -+ tq.tau_max.  Before the solve
// the wave looks at the path's own gridpoints 0 .. N-1 once: a non-finite coefficient is GTO_STATUS_NUMERICAL, a joint that
// cannot hold the path at rest somewhere (|TG| >= tau_max) GTO_STATUS_INFEASIBLE, both with NaN outputs and no Newton step.
// Without TORQUE the body is the one k_retime_convex had before the flag: every addition sits behind `if constexpr`.
template <bool TORQUE>
__device__ __forceinline__ void rt_convex_solve(double* __restrict__ al, double* __restrict__ be, const double* __restrict__ xcap,
                                                const int32_t* __restrict__ flag, const int32_t* __restrict__ n_cols,
                                                const RetimeLimits& lim, const RetimeDims& d, const RetimeConvex& cv,
                                                double* __restrict__ X, double* __restrict__ Tg, int32_t* __restrict__ stat,
                                                double* __restrict__ duration_out, double* __restrict__ t_out,
                                                double* __restrict__ sd_out, int32_t* __restrict__ status_out,
                                                int32_t* __restrict__ iters_out, const RetimeTorque& tq, RetimeTorqueRows tr) {
  extern __shared__ double rt_lds[];
  double *x = rt_lds, *g = x + d.Nmax, *dg = g + d.Nmax, *e = dg + d.Nmax, *dx = e + d.Nmax;
  const long long b = blockIdx.x;
  const int lane = threadIdx.x, ndof = d.ndof;
  const int N = d.subdiv * (rt_cols(n_cols, b, d.Tp) - 1) + 1;  // a bad count is flagged: N is not used then
  const int f = lane < ndof ? flag[b * ndof + lane] : GTO_RT_CONST;
  const bool bad = __ballot(f == GTO_RT_NONFINITE) != 0, moving = __ballot(f == GTO_RT_MOVING) != 0;
  const long long o = b * d.Nmax;
  const double w = 2.0 / (double)(N - 1), c = 0.5 * (double)(N - 1);
  const int n = N - 2;  // variables 1 .. n
  al += o * ndof, be += o * ndof;
  const double* cap = xcap + o;
  int status = GTO_STATUS_CONVERGED, it = 0;
  if (bad) status = GTO_STATUS_NUMERICAL;
  if constexpr (TORQUE) {
    tr.ta += o * ndof, tr.tb += o * ndof, tr.tg += o * ndof;
    if (!bad) {  // the path's own gridpoints, the last one included: the robot holds there too
      bool wild = false, over = false;
      for (int k = lane; k < N * ndof; k += 64) {
        const double gk = tr.tg[k];
        wild = wild || !isfinite(tr.ta[k]) || !isfinite(tr.tb[k]) || !isfinite(gk);
        over = over || fabs(gk) >= tq.tau_max[k % ndof];
      }
      if (__ballot(wild) != 0) status = GTO_STATUS_NUMERICAL;
      else if (__ballot(over) != 0) status = GTO_STATUS_INFEASIBLE;
    }
  }
  for (int i = lane; i < N && !bad; i += 64) x[i] = 0.0, dx[i] = 0.0;
  __syncthreads();
  if ((TORQUE ? status == GTO_STATUS_CONVERGED : !bad) && moving && n >= 1) {
    // the lines, once per plan
    for (int k = lane; k < (N - 1) * ndof; k += 64) {
      double a, bt;
      rt_line(al[k], be[k], lim.amax[k % ndof], a, bt);
      al[k] = a, be[k] = bt;
    }
    __syncthreads();
    // start: x = eps 1, eps half the largest value at which every row holds; m rows
    double top = INFINITY;
    int rows = 0;
    for (int i = lane; i < N - 1; i += 64) {
      if (i >= 1) {
        top = fmin(top, cap[i]);
        rows += cap[i] != INFINITY ? 2 : 1;
      }
      const double in0 = i >= 1 ? 1.0 : 0.0, in1 = i + 1 <= n ? 1.0 : 0.0;
      for (int j = 0; j < ndof; ++j) {
        const double a = al[(long long)i * ndof + j];
        if (a == INFINITY) continue;
        const double k = fabs(c * (in1 - in0) - be[(long long)i * ndof + j] * in0);
        if (k > 0.0) top = fmin(top, a / k);
        rows += 2;
      }
      if constexpr (TORQUE)
        for (int j = 0; j < ndof; ++j) {  // tau = (A1 + K) eps + g at x = eps 1: the side that eps moves it towards
          const double tm = tq.tau_max[j];
          double A1, K;
          if (!rt_torque_row(tr, (long long)i * ndof + j, c, i >= 1, i + 1 <= n, tm, A1, K)) continue;
          const double k = A1 + K, gk = tr.tg[(long long)i * ndof + j];
          if (k > 0.0) top = fmin(top, (tm - gk) / k);
          if (k < 0.0) top = fmin(top, (tm + gk) / -k);
          rows += 2;
        }
    }
    const double eps = 0.5 * rt_wave_min(top), m = rt_wave_sum((double)rows);
    for (int v = 1 + lane; v <= n; v += 64) x[v] = eps;
    __syncthreads();
    double T, phi;
    rt_convex_eval<TORQUE>(x, dx, 0.0, al, be, cap, N, ndof, lane, T, phi, tq, tr);
    double mu = T / m;
    if (!(eps > 0.0) || !isfinite(T) || !isfinite(phi)) status = GTO_STATUS_NUMERICAL;
    while (status == GTO_STATUS_CONVERGED) {
      // gradient, diagonal and off-diagonal of F_mu: variable v gathers the segments v-1 and v
      for (int v = 1 + lane; v <= n; v += 64) {
        const double xm = x[v - 1], x0 = x[v], xp = x[v + 1];
        const double q = sqrt(x0), S1 = sqrt(xm) + q, S2 = q + sqrt(xp), q2 = x0, q3 = x0 * q;
        const double i1 = 1.0 / (S1 * S1), i2 = 1.0 / (S2 * S2);
        double gv = -w * (i1 + i2) / (2.0 * q);
        double dv = w * ((i1 + i2) / (4.0 * q3) + (i1 / S1 + i2 / S2) / (2.0 * q2));
        double ev = v < n ? w * i2 / (2.0 * q * sqrt(xp) * S2) : 0.0;
        gv -= mu / x0;
        dv += mu / (x0 * x0);
        const double cp = cap[v];
        if (cp != INFINITY) {
          const double is = 1.0 / (cp - x0);
          gv += mu * is;
          dv += mu * is * is;
        }
        for (int j = 0; j < ndof; ++j) {  // the lines of gridpoint v-1: r = c (x_v - x_{v-1}) - beta x_{v-1}
          const double a = al[(long long)(v - 1) * ndof + j];
          if (a == INFINITY) continue;
          const double r = c * (x0 - xm) - be[(long long)(v - 1) * ndof + j] * xm;
          const double ip = 1.0 / (a - r), im = 1.0 / (a + r);
          gv += mu * c * (ip - im);
          dv += mu * c * c * (ip * ip + im * im);
        }
        for (int j = 0; j < ndof; ++j) {  // the lines of gridpoint v: r = c (x_{v+1} - x_v) - beta x_v
          const double a = al[(long long)v * ndof + j];
          if (a == INFINITY) continue;
          const double bt = be[(long long)v * ndof + j], k = -(c + bt);
          const double r = c * (xp - x0) - bt * x0;
          const double ip = 1.0 / (a - r), im = 1.0 / (a + r), hh = ip * ip + im * im;
          gv += mu * k * (ip - im);
          dv += mu * k * k * hh;
          if (v < n) ev += mu * k * c * hh;
        }
        if constexpr (TORQUE)
          for (int j = 0; j < ndof; ++j) {
            const double tm = tq.tau_max[j];
            double A1, K;
            // the torque row of gridpoint v-1: coefficient A1 on x_v
            if (rt_torque_row(tr, (long long)(v - 1) * ndof + j, c, v - 1 >= 1, true, tm, A1, K)) {
              const double r = rt_torque_tau(tr, (long long)(v - 1) * ndof + j, c, xm, x0);
              const double ip = 1.0 / (tm - r), im = 1.0 / (tm + r);
              gv += mu * A1 * (ip - im);
              dv += mu * A1 * A1 * (ip * ip + im * im);
            }
            // the torque row of gridpoint v: coefficient K on x_v, A1 on x_{v+1}
            if (rt_torque_row(tr, (long long)v * ndof + j, c, true, v < n, tm, A1, K)) {
              const double r = rt_torque_tau(tr, (long long)v * ndof + j, c, x0, xp);
              const double ip = 1.0 / (tm - r), im = 1.0 / (tm + r), hh = ip * ip + im * im;
              gv += mu * K * (ip - im);
              dv += mu * K * K * hh;
              ev += mu * K * A1 * hh;  // A1 = 0 at v = n
            }
          }
        g[v] = gv, dg[v] = dv, e[v] = ev;
      }
      __syncthreads();
      double dec = 0.0;
      rt_tridiag_serial(dg, e, g, dx, n, lane);
      __syncthreads();
      for (int v = 1 + lane; v <= n; v += 64) dec += g[v] * g[v] / dg[v];
      dec = rt_wave_sum(dec);  // g' H^-1 g = -(g . dx)
      const double lam = sqrt(dec / mu);
      if (!isfinite(lam) || !(mu > 0.0)) {
        status = GTO_STATUS_NUMERICAL;
        break;
      }
      if (lam < GTO_RT_CENTRED) {
        if (mu * (m + (lam + sqrt(m)) * lam / (1.0 - lam)) <= cv.gap_tol * T) break;
        mu *= GTO_RT_SHRINK;  // the next weight, from the same x: not a Newton step
        continue;
      }
      if (it == cv.max_newton) {
        status = GTO_STATUS_MAX_ITER;
        break;
      }
      // the largest step that stays strictly inside
      double room = INFINITY;
      for (int i = lane; i < N - 1; i += 64) {
        const double xi = x[i], xn = x[i + 1], di = dx[i], dn = dx[i + 1];
        if (i >= 1) {
          if (di < 0.0) room = fmin(room, xi / -di);
          if (di > 0.0 && cap[i] != INFINITY) room = fmin(room, (cap[i] - xi) / di);
        }
        for (int j = 0; j < ndof; ++j) {
          const double a = al[(long long)i * ndof + j];
          if (a == INFINITY) continue;
          const double bt = be[(long long)i * ndof + j];
          const double r = c * (xn - xi) - bt * xi, dr = c * (dn - di) - bt * di;
          if (dr > 0.0) room = fmin(room, (a - r) / dr);
          if (dr < 0.0) room = fmin(room, (a + r) / -dr);
        }
        if constexpr (TORQUE)
          for (int j = 0; j < ndof; ++j) {
            const double tm = tq.tau_max[j];
            double A1, K;
            if (!rt_torque_row(tr, (long long)i * ndof + j, c, i >= 1, i + 1 <= n, tm, A1, K)) continue;
            const double r = rt_torque_tau(tr, (long long)i * ndof + j, c, xi, xn);
            const double dr = fma(tr.ta[(long long)i * ndof + j] * c, dn - di, tr.tb[(long long)i * ndof + j] * di);
            if (dr > 0.0) room = fmin(room, (tm - r) / dr);
            if (dr < 0.0) room = fmin(room, (tm + r) / -dr);
          }
      }
      double eta = fmin(1.0, 0.99 * rt_wave_min(room));
      // backtracking on F_mu; a difference below the round-off of F_mu counts as a decrease
      const double F0 = T + mu * phi;
      for (int k = 0; k < GTO_RT_BACKTRACKS; ++k, eta *= 0.5) {
        double Tn, phin;
        rt_convex_eval<TORQUE>(x, dx, eta, al, be, cap, N, ndof, lane, Tn, phin, tq, tr);
        if (Tn + mu * phin <= F0 - GTO_RT_ARMIJO * eta * dec + 4e-16 * fabs(F0)) {
          __syncthreads();
          for (int v = 1 + lane; v <= n; v += 64) x[v] = fma(eta, dx[v], x[v]);
          T = Tn, phi = phin;
          break;
        }
      }
      __syncthreads();
      ++it;
    }
  }
  // times and outputs
  if (status == GTO_STATUS_NUMERICAL || (TORQUE && status == GTO_STATUS_INFEASIBLE)) {
    for (int i = lane; i < d.Nmax; i += 64) {
      X[o + i] = NAN, Tg[o + i] = NAN;
      if (t_out) t_out[o + i] = NAN;
      if (sd_out) sd_out[o + i] = NAN;
    }
    if (lane == 0) {
      stat[b] = GTO_STATUS_NUMERICAL;  // no profile to sample
      if (duration_out) duration_out[b] = NAN;
      if (status_out) status_out[b] = TORQUE ? status : GTO_STATUS_NUMERICAL;
      if (iters_out) iters_out[b] = it;
    }
    return;
  }
  __syncthreads();
  double t = 0.0;
  if (lane == 0) {
    double xi = 0.0;
    X[o] = 0.0, Tg[o] = 0.0;
    if (t_out) t_out[o] = 0.0;
    if (sd_out) sd_out[o] = 0.0;
    for (int i = 1; i < N; ++i) {
      const double xn = x[i];
      if (moving) t += w / (sqrt(xi) + sqrt(xn));
      xi = xn;
      X[o + i] = xn, Tg[o + i] = t;
      if (t_out) t_out[o + i] = t;
      if (sd_out) sd_out[o + i] = sqrt(xn);
    }
  }
  t = __shfl(t, 0, 64);
  for (int i = N + lane; i < d.Nmax; i += 64) {
    if (t_out) t_out[o + i] = t;
    if (sd_out) sd_out[o + i] = 0.0;
  }
  if (lane == 0) {
    const bool ok = isfinite(t);  // N = 2 with a moving joint: no variable, both ends rest, the one segment takes forever
    stat[b] = ok ? GTO_STATUS_CONVERGED : GTO_STATUS_NUMERICAL;
    if (duration_out) duration_out[b] = t;
    if (status_out) status_out[b] = ok ? status : GTO_STATUS_NUMERICAL;
    if (iters_out) iters_out[b] = it;
  }
}

__global__ __launch_bounds__(64) void k_retime_convex(double* __restrict__ al, double* __restrict__ be,
                                                      const double* __restrict__ xcap, const int32_t* __restrict__ flag,
                                                      const int32_t* __restrict__ n_cols, RetimeLimits lim, RetimeDims d,
                                                      RetimeConvex cv, double* __restrict__ X, double* __restrict__ Tg,
                                                      int32_t* __restrict__ stat, double* __restrict__ duration_out,
                                                      double* __restrict__ t_out, double* __restrict__ sd_out,
                                                      int32_t* __restrict__ status_out, int32_t* __restrict__ iters_out) {
  const RetimeTorque none = {};
  rt_convex_solve<false>(al, be, xcap, flag, n_cols, lim, d, cv, X, Tg, stat, duration_out, t_out, sd_out, status_out, iters_out,
                         none, {nullptr, nullptr, nullptr});
}

__global__ __launch_bounds__(64) void k_retime_convex_torque(
    double* __restrict__ al, double* __restrict__ be, const double* __restrict__ xcap, const int32_t* __restrict__ flag,
    const int32_t* __restrict__ n_cols, RetimeLimits lim, RetimeDims d, RetimeConvex cv, double* __restrict__ X,
    double* __restrict__ Tg, int32_t* __restrict__ stat, double* __restrict__ duration_out, double* __restrict__ t_out,
    double* __restrict__ sd_out, int32_t* __restrict__ status_out, int32_t* __restrict__ iters_out, RetimeTorque tq,
    const double* __restrict__ TA, const double* __restrict__ TB, const double* __restrict__ TG) {
  rt_convex_solve<true>(al, be, xcap, flag, n_cols, lim, d, cv, X, Tg, stat, duration_out, t_out, sd_out, status_out, iters_out,
                        tq, {TA, TB, TG});
}

// The torque coefficients of every (path, gridpoint) row id = b Nmax + i, i < N_b: with the path's payload on frame_ee,
//   TG = ID(q, 0, 0),  TA = ID(q, 0, p1) - TG,  TB = ID(q, p1, p2) - TG      [B][Nmax][ndof] each,
// so that tau = TA u + TB x + TG along the path (inverse dynamics is affine in qdd and quadratic in qd, and qd = p1 sd,
// qdd = p1 u + p2 x).  q: the spline's value at the gridpoint (rt_piece; the first waypoint of a row flagged constant, and of
// every row at C = 1); p1, p2: k_retime_grid's, which hold 0 on the constant rows.  One lane per row, `rows` of them per
// 64-lane workgroup with k_inverse_dynamics' LDS layout; three rt_rnea passes over the lane's own column.  A joint that no
// frame names keeps 0.  A path flagged non-finite (a wild count among them) is left alone: k_retime_convex_torque does not
// read its rows.  A payload mass that is negative or not finite (a device value no host has seen) makes the row's TG NaN.
__global__ __launch_bounds__(GTO_WAVE) void k_retime_torque_rows(
    const RobotDev* __restrict__ rb, const DynDev* __restrict__ dyn, const double* __restrict__ Q, const double* __restrict__ S,
    const int32_t* __restrict__ flag, const int32_t* __restrict__ n_cols, const double* __restrict__ P1,
    const double* __restrict__ P2, const double* __restrict__ pl_mass, const double* __restrict__ pl_com,
    const double* __restrict__ pl_inertia, RetimeDims d, int rows, double* __restrict__ TA, double* __restrict__ TB,
    double* __restrict__ TG) {
  extern __shared__ __attribute__((aligned(16))) double smem_rnea[];
  const int lane = threadIdx.x;
  const long long id = (long long)blockIdx.x * rows + lane;
  if (lane >= rows || id >= (long long)d.B * d.Nmax) return;
  const long long b = id / d.Nmax;
  const int g = (int)(id - b * d.Nmax), T = d.Tp, ndof = d.ndof;
  const int C = rt_cols(n_cols, b, T), N = d.subdiv * (C - 1) + 1;
  if (C == 0 || g >= N) return;
  const int32_t* fl = flag + b * ndof;
  for (int j = 0; j < ndof; ++j)
    if (fl[j] == GTO_RT_NONFINITE) return;
  const int k = max(min(g / d.subdiv, C - 2), 0);  // as in k_retime_grid
  const double r = (double)(g - k * d.subdiv) / (double)(N - 1);
  const double invh = (double)(C - 1);
  const double *y = Q + b * ndof * T, *s = S + b * ndof * T;
  const double *p1 = P1 + id * ndof, *p2 = P2 + id * ndof;
  double *ta = TA + id * ndof, *tb = TB + id * ndof, *tg = TG + id * ndof;
  const RneaPayload pl = rnea_payload(pl_mass, pl_com, pl_inertia, (size_t)b);
  const bool mass_ok = pl.m >= 0.0 && isfinite(pl.m);
  for (int j = 0; j < ndof; ++j) ta[j] = 0.0, tb[j] = 0.0, tg[j] = mass_ok ? 0.0 : NAN;
  if (!mass_ok) return;
  auto q = [&](int j) {
    if (fl[j] != GTO_RT_MOVING) return y[(long long)j * T];
    double qv, d1, d2;
    rt_piece(y + (long long)j * T, s + (long long)j * T, k, r, invh, qv, d1, d2);
    return qv;
  };
  auto zero = [](int) { return 0.0; };
  double* st = smem_rnea + lane;
  rt_rnea(rb, dyn, pl, st, rows, q, zero, zero, [&](int j, double v) { tg[j] = v; });
  rt_rnea(rb, dyn, pl, st, rows, q, zero, [&](int j) { return p1[j]; }, [&](int j, double v) { ta[j] = v - tg[j]; });
  rt_rnea(rb, dyn, pl, st, rows, q, [&](int j) { return p1[j]; }, [&](int j) { return p2[j]; },
          [&](int j, double v) { tb[j] = v - tg[j]; });
}

// tau_out [B][M][ndof] of gto_retime_paths_torque: k_inverse_dynamics over the B M sample rows (q, qd, qdd of
// k_retime_sample), the payload of row id being its path's, b = id / M.  The same arithmetic on the same values: the bits of
// gto_inverse_dynamics on these rows with the payload repeated per sample.
__global__ __launch_bounds__(GTO_WAVE) void k_retime_tau(const RobotDev* __restrict__ rb, const DynDev* __restrict__ dyn, long long n,
                                                         int M, int rows, const double* __restrict__ q, const double* __restrict__ qd,
                                                         const double* __restrict__ qdd, const double* __restrict__ pl_mass,
                                                         const double* __restrict__ pl_com, const double* __restrict__ pl_inertia,
                                                         double* __restrict__ tau_out) {
  extern __shared__ __attribute__((aligned(16))) double smem_rnea[];
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * rows + lane;
  if (lane >= rows || row >= n) return;
  const int ndof = rb->ndof;
  const double *qr = q + row * ndof, *qdr = qd + row * ndof, *qddr = qdd + row * ndof;
  double* tr = tau_out + row * ndof;
  for (int j = 0; j < ndof; ++j) tr[j] = 0.0;
  const RneaPayload pl = rnea_payload(pl_mass, pl_com, pl_inertia, (size_t)(row / M));
  rt_rnea(rb, dyn, pl, smem_rnea + lane, rows, [&](int j) { return qr[j]; }, [&](int j) { return qdr[j]; },
          [&](int j) { return qddr[j]; }, [&](int j, double v) { tr[j] = v; });
}

// Samples at linspace(0, duration, M) (numpy's values): the segment i with t_i <= t < t_{i+1}, s and sdot under the
// segment's constant acceleration, q = spline(s), qdot = p1 sdot, qddot = p1 sddot + p2 sdot^2.  [B][M][ndof]
__global__ __launch_bounds__(256) void k_retime_sample(const double* __restrict__ Q, const double* __restrict__ S,
                                                       const double* __restrict__ X, const double* __restrict__ Tg,
                                                       const int32_t* __restrict__ stat,
                                                       const int32_t* __restrict__ n_cols, RetimeDims d,
                                                       double* __restrict__ q_out, double* __restrict__ qd_out,
                                                       double* __restrict__ qdd_out) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)d.B * d.M) return;
  const long long b = id / d.M;
  const int m = (int)(id - b * d.M), T = d.Tp, ndof = d.ndof;
  if (stat[b] != GTO_STATUS_CONVERGED) {  // a bad count among them
    for (int j = 0; j < ndof; ++j) {
      if (q_out) q_out[id * ndof + j] = NAN;
      if (qd_out) qd_out[id * ndof + j] = NAN;
      if (qdd_out) qdd_out[id * ndof + j] = NAN;
    }
    return;
  }
  const int C = rt_cols(n_cols, b, T), N = d.subdiv * (C - 1) + 1;
  if (C == 1) {  // one waypoint: the rule of a plan whose waypoints are all equal
    for (int j = 0; j < ndof; ++j) {
      if (q_out) q_out[id * ndof + j] = Q[(b * ndof + j) * T];
      if (qd_out) qd_out[id * ndof + j] = 0.0;
      if (qdd_out) qdd_out[id * ndof + j] = 0.0;
    }
    return;
  }
  const double* t = Tg + b * d.Nmax;
  const double dur = t[N - 1];
  const double tt = m == d.M - 1 ? dur : (double)m * (dur / (double)(d.M - 1));
  int lo = 0, hi = N - 2;  // the largest i in [0, N-2] with t_i <= tt
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid] <= tt) lo = mid;
    else hi = mid - 1;
  }
  const double x0 = X[b * d.Nmax + lo], x1 = X[b * d.Nmax + lo + 1];
  const double v0 = sqrt(x0), u = (x1 - x0) * (0.5 * (double)(N - 1)), tau = tt - t[lo];
  const double sd = v0 + u * tau;
  double s = (double)lo / (double)(N - 1) + tau * (v0 + 0.5 * u * tau);
  s = fmin(fmax(s, 0.0), 1.0);
  const int k = min(max((int)(s * (double)(C - 1)), 0), C - 2);
  const double r = s - (double)k / (double)(C - 1);
  const double invh = (double)(C - 1);
  for (int j = 0; j < ndof; ++j) {
    const long long row = b * ndof + j;
    double q, p1, p2;
    rt_piece(Q + row * T, S + row * T, k, r, invh, q, p1, p2);
    if (q_out) q_out[id * ndof + j] = q;
    if (qd_out) qd_out[id * ndof + j] = p1 * sd;
    if (qdd_out) qdd_out[id * ndof + j] = p1 * u + p2 * sd * sd;
  }
}
