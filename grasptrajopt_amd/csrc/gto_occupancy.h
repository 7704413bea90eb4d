// gto_occupancy.h — the first half of the mobile driver's per-object loop (examples/pybullet_gto_planning_mobile.py:157-202,
// gto/base_planner.py:96-168) around k_base_solve (gfx950): the x-y occupancy grid of the observed scene, what the reference
// reports of a base placement, and the choice among many draws.  FP64.
//   k_occ_bounds        grid-stride pass over the observed points with z > 0.01: max x, min y, max y per lane, folded over the
//                       wave, one partial per workgroup (the host folds the partials: min / max have no order)
//   k_occ_mark          one lane per point: the grid nodes within epsilon of it get a 1 (GTORobotModel.setup_occupancy_grid,
//                       gto/gto_models.py:218-244; numpy's expression without contraction, so the grid is bit-equal)
//   k_base_report       grid (n_max + 1, B).  Row i < n_max: err_pos / err_rot of goal i of set b (gto/base_planner.py:130-144).
//                       Row n_max: the robot's surface points at qc_b seen from the moved base, counted on the occupancy grid
//                       (:149-162); kinematics are k_plan_cost's (plan_cost_kinematics<1>)
//   k_base_first_free   one wave: the lowest set with no point on an occupied node (the driver's `if cost == 0: break`)
#pragma once
#include "gto_kernels.h"

// Observed points as the two kinds of observation keep them: x[i * stride], y[i * stride], z[i * stride].  skip_inf: a point
// at infinity is an invalid pixel of a depth image (k_depth_backproject), not an observation.
struct OccPoints {
  const double *x, *y, *z;
  long n;
  int stride;
  int skip_inf;
};
// whether point (x, y, z) takes part in the grid: points[:, 2] > 0.01 (a NaN does not)
__device__ __forceinline__ bool occ_point_counts(const OccPoints& pts, double x, double z) {
  return z > 0.01 && !(pts.skip_inf && x == INFINITY && z == INFINITY);
}

#define GTO_OCC_PART 4  // doubles per partial: max x, min y, max y, 1.0 if numpy's bounds are not finite
#define GTO_OCC_MAX_K 8  // ceil(epsilon / resolution) that k_occ_mark walks

// numpy's max propagates a NaN and takes +inf, its min likewise: such a point makes a bound non-finite (flag).  x = -inf
// leaves max x alone, as in numpy.
__global__ __launch_bounds__(256) void k_occ_bounds(OccPoints pts, double* __restrict__ partial) {
  __shared__ double s_part[4][GTO_OCC_PART];
  const int tid = threadIdx.x;
  double xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, bad = 0.0;
  for (long i = (long)blockIdx.x * 256 + tid; i < pts.n; i += (long)gridDim.x * 256) {
    const double x = pts.x[i * pts.stride], y = pts.y[i * pts.stride], z = pts.z[i * pts.stride];
    if (!occ_point_counts(pts, x, z)) continue;
    if (x != x || x == INFINITY || !isfinite(y)) {
      bad = 1.0;
      continue;
    }
    xmax = fmax(xmax, x), ymin = fmin(ymin, y), ymax = fmax(ymax, y);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    xmax = fmax(xmax, __shfl_xor(xmax, s, 64));
    ymin = fmin(ymin, __shfl_xor(ymin, s, 64));
    ymax = fmax(ymax, __shfl_xor(ymax, s, 64));
    bad = fmax(bad, __shfl_xor(bad, s, 64));
  }
  if ((tid & 63) == 0) {
    double* p = s_part[tid >> 6];
    p[0] = xmax, p[1] = ymin, p[2] = ymax, p[3] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    double* o = partial + (size_t)blockIdx.x * GTO_OCC_PART;
    o[0] = fmax(fmax(s_part[0][0], s_part[1][0]), fmax(s_part[2][0], s_part[3][0]));
    o[1] = fmin(fmin(s_part[0][1], s_part[1][1]), fmin(s_part[2][1], s_part[3][1]));
    o[2] = fmax(fmax(s_part[0][2], s_part[1][2]), fmax(s_part[2][2], s_part[3][2]));
    o[3] = fmax(fmax(s_part[0][3], s_part[1][3]), fmax(s_part[2][3], s_part[3][3]));
  }
}

// xgrid [nx], ygrid [ny]: numpy.arange's values (the host computes them once the bounds are back); grid [nx][ny] zeroed.
// A point's nearest node is (rint((x - xgrid[0]) / r), rint((y - ygrid[0]) / r)); the nodes up to k = ceil(epsilon / r) away
// from it are tested.  The node indices are tested as doubles first: a finite but enormous coordinate never reaches an
// integer.  Every writer stores the same byte, so the stores need no order.
__global__ __launch_bounds__(256) void k_occ_mark(OccPoints pts, const double* __restrict__ xgrid, const double* __restrict__ ygrid,
                                                  int nx, int ny, double res, double epsilon, int k, uint8_t* __restrict__ grid) {
#pragma clang fp contract(off)  // numpy's differences, squares, sum and root: one rounding each
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pts.n) return;
  const double x = pts.x[i * pts.stride], y = pts.y[i * pts.stride], z = pts.z[i * pts.stride];
  if (!occ_point_counts(pts, x, z)) return;
  const double fx = rint((x - xgrid[0]) / res), fy = rint((y - ygrid[0]) / res);
  if (!(fx >= (double)-k && fx <= (double)(nx - 1 + k) && fy >= (double)-k && fy <= (double)(ny - 1 + k))) return;  // (a NaN leaves too)
  const int ix0 = (int)fx, iy0 = (int)fy;
  for (int di = -k; di <= k; ++di) {
    const int ix = ix0 + di;
    if (ix < 0 || ix >= nx) continue;
    const double dx = x - xgrid[ix], dx2 = dx * dx;
    for (int dj = -k; dj <= k; ++dj) {
      const int iy = iy0 + dj;
      if (iy < 0 || iy >= ny) continue;
      const double dy = y - ygrid[iy];
      if (__dsqrt_rn(dx2 + dy * dy) < epsilon) grid[(size_t)ix * ny + iy] = 1;
    }
  }
}

// what k_base_report reads of a resident occupancy grid (grid: device)
struct OccGridView {
  const uint8_t* grid;
  int nx, ny;
  double ox, oy, res;
};

// Surface point (X0, X1) of the robot at the old base, in the frame of the new base y = (y0, y1, theta), c = cos theta,
// s = sin theta: the first two rows of inv(rt2tr(rotz(theta), [y0, y1, 0])) applied to it; then its node of the occupancy grid
// as points_to_offsets_occupancy_numpy finds it (gto/gto_models.py:262-273): floor((. - origin) / resolution), clipped per axis.
__device__ __forceinline__ bool occ_point_hits(const OccGridView& g, double X0, double X1, double y0, double y1, double c, double s) {
#pragma clang fp contract(off)
  const double dx = X0 - y0, dy = X1 - y1;
  const double xp = c * dx + s * dy, yp = -s * dx + c * dy;
  double fx = floor((xp - g.ox) / g.res), fy = floor((yp - g.oy) / g.res);
  // clipped in double before any integer conversion (a finite but enormous base pose overflows to +-inf here); should a NaN
  // arise it goes to node 0 of its axis by the form of the test, not by how the hardware converts a NaN
  fx = fx >= 0.0 ? (fx <= (double)(g.nx - 1) ? fx : (double)(g.nx - 1)) : 0.0;
  fy = fy >= 0.0 ? (fy <= (double)(g.ny - 1) ? fy : (double)(g.ny - 1)) : 0.0;
  return g.grid[(size_t)(int)fx * g.ny + (int)fy] != 0;
}

// Rigid transform (3 x 4, row-major) of frame f out of the transposed frames plan_cost_kinematics left in LDS
__device__ __forceinline__ void base_report_frame(const double* __restrict__ Xg, int f, double (&A)[12]) {
#pragma unroll
  for (int e = 0; e < 12; ++e) A[e] = Xg[fkx(f, 4 * (e & 3) + (e >> 2))];
}

// n_goals [B] (device copy of the caller's host array, checked on the host), qc [B][ndof], goals [B][n_max][16], y [B][3],
// q [B][n_max][ndof].  A launch without an occupancy grid has no row n_max (grid.x = n_max).  The surface points are
// k_eval_points' expression with a zero base.
__global__ __launch_bounds__(256) void k_base_report(const RobotDev* __restrict__ rb, const double* __restrict__ px,
                                                     const double* __restrict__ py, const double* __restrict__ pz,
                                                     const int32_t* __restrict__ plink, const int32_t* __restrict__ n_goals,
                                                     const double* __restrict__ qc, const double* __restrict__ goals,
                                                     const double* __restrict__ y, const double* __restrict__ q, int n_max,
                                                     OccGridView og, double* __restrict__ err_pos_out,
                                                     double* __restrict__ err_rot_out, int32_t* __restrict__ collision_out) {
  const int row = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int F = rb->n_frames, ndof = rb->ndof, P = rb->n_points;
  extern __shared__ __attribute__((aligned(16))) double smem_br[];
  // plan_cost_lds<1>'s layout, laid out here and not through the helper: the compiler arranges k_ik_report's code (its
  // register counts are in kernel_resources.txt) differently with every further caller of plan_cost_lds<1>; k_held_attach
  // is one (one scalar register of k_ik_report's: DESIGN.md 7g)
  PlanCostLds m;
  m.tab = smem_br;
  m.sc = m.tab + fk_tab_doubles(F, rb->n_links, rb->n_opt);
  m.X = m.sc + F * 2;
  m.vis = m.X + fk_scratch_doubles(F, 1);
  m.screw = m.vis + rb->n_links * 12;
  m.red = m.screw + screw_rows(rb->n_opt) * 6;
  const double* yb = y + (size_t)b * 3;
  const double* qcb = qc + (size_t)b * ndof;
  __shared__ int s_cnt[4];
  __shared__ int s_bad;
  const bool goal_row = row < n_max;
  if (goal_row ? (row >= n_goals[b] || (!err_pos_out && !err_rot_out)) : !collision_out) return;  // (uniform)
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (!goal_row && tid < ndof + 3 && !isfinite(tid < ndof ? qcb[tid] : yb[tid - ndof])) s_bad = 1;
  __syncthreads();
  const bool bad = s_bad != 0;  // a footprint with a non-finite entry: its kinematics run on zeros, so nothing non-finite enters a matrix-core product
  const double* src = goal_row ? q + ((size_t)b * n_max + row) * ndof : qcb;
  plan_cost_kinematics<1>(rb, m, 1, tid, [&](int, int dq) { return bad ? 0.0 : src[dq]; });
  if (goal_row) {  // ---- goal `row` of set b
    if (tid != 0) return;
    const double* Xg = m.X + (rb->fk_rounds & 1) * 16 * F;
    double E[12], Tg[12], G[12], M[12], RT[12];
    base_report_frame(Xg, rb->frame_ee, E);
    base_report_frame(Xg, rb->frame_gripper, Tg);
    // G = T_ee^-1 T_g, the inverse of a rigid transform in closed form: (R^T, -R^T t)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) G[4 * i + j] = E[i] * Tg[j] + E[4 + i] * Tg[4 + j] + E[8 + i] * Tg[8 + j];
      G[4 * i + 3] = E[i] * (Tg[3] - E[3]) + E[4 + i] * (Tg[7] - E[7]) + E[8 + i] * (Tg[11] - E[11]);
    }
    // M = RT_i G, RT = B(y) M with B = rt2tr(rotz(theta), [x, y, 0])
    const double* g = goals + ((size_t)b * n_max + row) * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        M[4 * i + j] = g[4 * i] * G[j] + g[4 * i + 1] * G[4 + j] + g[4 * i + 2] * G[8 + j] + (j == 3 ? g[4 * i + 3] : 0.0);
    double s, c;
    sincos(yb[2], &s, &c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      RT[j] = c * M[j] - s * M[4 + j] + (j == 3 ? yb[0] : 0.0);
      RT[4 + j] = s * M[j] + c * M[4 + j] + (j == 3 ? yb[1] : 0.0);
      RT[8 + j] = M[8 + j];
    }
    const double d0 = RT[3] - Tg[3], d1 = RT[7] - Tg[7], d2 = RT[11] - Tg[11];
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) tr += RT[4 * i + j] * Tg[4 * i + j];
    double ca = (tr - 1.0) / 2.0;
    ca = ca < -1.0 ? -1.0 : (ca > 1.0 ? 1.0 : ca);  // (a NaN stays one, as in np.clip)
    if (err_pos_out) err_pos_out[(size_t)b * n_max + row] = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    if (err_rot_out) err_rot_out[(size_t)b * n_max + row] = acos(ca) * (180.0 / M_PI);
    return;
  }
  // ---- the footprint of set b
  double s = 0.0, c = 1.0;
  if (!bad) sincos(yb[2], &s, &c);
  const double y0 = bad ? 0.0 : yb[0], y1 = bad ? 0.0 : yb[1];
  int cnt = 0;
  for (int p0 = 0; p0 < P; p0 += 256) {  // uniform trip count: every lane takes part in the ballots
    const int p = p0 + tid;
    const bool live = p < P;
    const double x0 = live ? px[p] : 0.0, x1 = live ? py[p] : 0.0, x2 = live ? pz[p] : 0.0;
    const double* V = m.vis + (live ? plink[p] : 0) * 12;
    const double X0 = V[0] * x0 + V[1] * x1 + V[2] * x2 + V[3];
    const double X1 = V[4] * x0 + V[5] * x1 + V[6] * x2 + V[7];
    cnt += __popcll(__ballot(live && occ_point_hits(og, X0, X1, y0, y1, c, s)));
  }
  if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) collision_out[b] = bad ? -1 : ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
}

// first_free[0] = the lowest b with collision[b] == 0, or -1: one wave, 64 sets per ballot
__global__ __launch_bounds__(64) void k_base_first_free(const int32_t* __restrict__ collision, int B, int32_t* __restrict__ first_free) {
  const int lane = threadIdx.x;
  int first = -1;
  for (int b0 = 0; b0 < B && first < 0; b0 += 64) {
    const int b = b0 + lane;
    const unsigned long long mask = __ballot(b < B && collision[b] == 0);
    if (mask) first = b0 + __builtin_ctzll(mask);
  }
  if (lane == 0) first_free[0] = first;
}
