// gto_forward.h — forward dynamics and the tracking rollout on top of rt_rnea (gfx950): fd_solve, k_forward_dynamics
// (gto_forward_dynamics) and k_track_rollout (gto_track_rollout[_device]).  FP64 throughout, no atomics.
//
// fd_solve is the inverse of the inverse dynamics at one state: with the payload on frame_ee,
//   g = ID(q, 0, 0),  c = ID(q, qd, 0),  column j of the mass matrix = ID(q, 0, e_j) - g  for the joints of a column list,
// every one of them an rt_rnea pass; the matrix is symmetrised (M_ij <- (M_ij + M_ji) / 2), factored by Cholesky on the
// FREE joints and M_ff x_f = (tau - c)_f is solved; x = 0 on every other joint.  A pivot <= 0 (a free joint that moves no
// mass; a NaN pivot among them) or a non-finite solution reports failure.
//
// Who runs what.  The nc + 2 passes are independent, so a GROUP of G lanes shares one evaluation: pass p runs on lane
// p % G of the group in round p / G, on that lane's own rt_rnea column (k_inverse_dynamics' layout
// st[(frame * GTO_RNEA_SLOTS + slot) * stride + lane]: conflict-free).  The passes write into the group's work arrays in
// LDS (the matrix A [ndof][ndof], the vectors g, c), the group symmetrises them pair by pair, lane 0 of the group factors
// and solves in place -- every run-time index is an LDS address, none a register array (those land in
// scratch) -- and everybody reads x.  The factor L overwrites the strict lower triangle of A between the free joints and
// its diagonal goes to ld, so the upper triangle with the diagonal is still M afterwards.  Element i of a work vector is at
// [i * vs]: vs = 1 where a group owns contiguous arrays (k_track_rollout), vs = the lanes of the workgroup where every
// lane is its own group (k_forward_dynamics, G = 1: the rows of a wave then read consecutive doubles).  The result of an
// evaluation does not depend on G or on who else shares the workgroup: a pass touches its own column and its own
// outputs only, and the factorisation is one lane's serial loop over the free joints in ascending order.
//
// sync() separates the steps where G > 1 (a workgroup barrier: every lane of the workgroup calls fd_solve together, the
// ones without work with active = false); with G = 1 a lane only ever reads what it wrote itself and sync is empty.
#pragma once
#include "gto_dynamics.h"

#define GTO_FD_LDS_BYTES (64 * 1024)  // per workgroup, as GTO_RNEA_LDS_BYTES: two workgroups fit the CU's 160 KiB
#define GTO_FD_SHARED_BYTES 2048      // of them: the workgroup's shared tables (joint lists, gains, flags)
#define GTO_FD_VECS 7                 // work vectors of k_forward_dynamics per row: q qd tau g c ld x
#define GTO_TR_VECS 15                // of k_track_rollout per path: those (q, qd the stage's state), the period's state sq sqd, the RK4
                                      // sums aq aqd, the feedforward ff and the reference rq rqd rqdd
#define GTO_TRACK_MAX_STEPS (1 << 20)

// The joint lists of a call, built by the host from `locked` (gto_api.hip, fd_sets): col = the joints whose mass-matrix
// columns are computed, fr = the free joints, both ascending; is_free[j] for every joint.
struct FdSets {
  int32_t ndof, nc, nf;
  int32_t col[GTO_MAX_DOF], fr[GTO_MAX_DOF], is_free[GTO_MAX_DOF];
};
// the same in LDS, where a lane may index them
struct FdLists {
  const int *col, *fr, *is_free;
  int ndof, nc, nf;
};
struct FdWork {
  double *q, *qd, *tau;  // the state and the joint forces (read)
  double *A, *g, *c, *ld;
  double* x;  // the accelerations (written)
  int vs;
};

// doubles of work arrays per row / per path
__host__ __device__ inline int fd_work_doubles(int ndof, int vecs) { return ndof * ndof + vecs * ndof; }
// rows one workgroup of k_forward_dynamics holds (one lane each)
__host__ __device__ inline int fd_rows_per_block(int F, int ndof) {
  const int per = (GTO_RNEA_SLOTS * F + fd_work_doubles(ndof, GTO_FD_VECS)) * (int)sizeof(double) + (int)sizeof(int);
  const int r = (GTO_FD_LDS_BYTES - GTO_FD_SHARED_BYTES) / per;
  return r < GTO_WAVE ? r : GTO_WAVE;
}
// bytes of one path of k_track_rollout at G lanes per path
__host__ __device__ inline int track_path_bytes(int F, int ndof, int G) {
  return (GTO_RNEA_SLOTS * F * G + fd_work_doubles(ndof, GTO_TR_VECS)) * (int)sizeof(double) + 4 * (int)sizeof(int);
}
// lanes per path: 16, or the largest power of two below it at which one path fits the workgroup's LDS
__host__ __device__ inline int track_group_lanes(int F, int ndof) {
  int G = 16;
  while (G > 1 && track_path_bytes(F, ndof, G) > GTO_FD_LDS_BYTES - GTO_FD_SHARED_BYTES) G >>= 1;
  return G;
}
__host__ __device__ inline int track_paths_per_block(int F, int ndof, int G) {
  const int p = (GTO_FD_LDS_BYTES - GTO_FD_SHARED_BYTES) / track_path_bytes(F, ndof, G);
  return p < GTO_WAVE / G ? p : GTO_WAVE / G;
}

struct FdNoSync {
  __device__ void operator()() const {}
};
struct FdBlockSync {
  __device__ void operator()() const { __syncthreads(); }
};

// One evaluation (see the head of the file).  st: the calling lane's rt_rnea column; gl: its index in its group of G;
// ok: the group's flag in LDS.  Returns whether x holds a finite solution.
template <class Sync>
__device__ inline bool fd_solve(const RobotDev* __restrict__ rb, const DynDev* __restrict__ dyn, const RneaPayload& pl, double* st,
                                int stride, int G, int gl, bool active, const FdLists& L, const FdWork& w, int* ok, Sync sync) {
  const int vs = w.vs, ndof = L.ndof, nc = L.nc, nf = L.nf, np = L.nc + 2;
  for (int p0 = 0; p0 < np; p0 += G) {
    const int p = p0 + gl;
    if (!active || p >= np) continue;
    const int ej = p >= 2 ? L.col[p - 2] : -1;
    const bool vel = p == 1;
    rt_rnea(
        rb, dyn, pl, st, stride, [&](int j) { return w.q[j * vs]; }, [&](int j) { return vel ? w.qd[j * vs] : 0.0; },
        [&](int j) { return j == ej ? 1.0 : 0.0; },
        [&](int j, double v) {
          if (p == 0) w.g[j * vs] = v;
          else if (p == 1) w.c[j * vs] = v;
          else w.A[(j * ndof + ej) * vs] = v;
        });
  }
  sync();
  if (active)
    for (int id = gl; id < nc * nc; id += G) {  // one lane per unordered pair of listed joints
      const int a = id / nc, b = id - a * nc;
      if (a > b) continue;
      const int i = L.col[a], j = L.col[b];
      const double m = 0.5 * ((w.A[(i * ndof + j) * vs] - w.g[i * vs]) + (w.A[(j * ndof + i) * vs] - w.g[j * vs]));
      w.A[(i * ndof + j) * vs] = m, w.A[(j * ndof + i) * vs] = m;
    }
  sync();
  if (active && gl == 0) {
    bool good = true;
    for (int j = 0; j < ndof; ++j) w.x[j * vs] = 0.0;
    for (int a = 0; a < nf && good; ++a) {  // L L^T = M_ff, a column at a time; fr ascends: (fr[b], fr[a]) is below the diagonal for b > a
      const int i = L.fr[a];
      double s = w.A[(i * ndof + i) * vs];
      for (int k = 0; k < a; ++k) {
        const double l = w.A[(i * ndof + L.fr[k]) * vs];
        s -= l * l;
      }
      if (!(s > 0.0)) {
        good = false;
        break;
      }
      const double d = sqrt(s);
      w.ld[a * vs] = d;
      for (int b = a + 1; b < nf; ++b) {
        const int r = L.fr[b];
        double t = w.A[(i * ndof + r) * vs];  // above the diagonal: still M
        for (int k = 0; k < a; ++k) t -= w.A[(r * ndof + L.fr[k]) * vs] * w.A[(i * ndof + L.fr[k]) * vs];
        w.A[(r * ndof + i) * vs] = t / d;
      }
    }
    if (good) {
      for (int a = 0; a < nf; ++a) {  // L y = tau - c
        const int i = L.fr[a];
        double y = w.tau[i * vs] - w.c[i * vs];
        for (int k = 0; k < a; ++k) y -= w.A[(i * ndof + L.fr[k]) * vs] * w.x[L.fr[k] * vs];
        w.x[i * vs] = y / w.ld[a * vs];
      }
      for (int a = nf - 1; a >= 0; --a) {  // L^T x = y
        const int i = L.fr[a];
        double y = w.x[i * vs];
        for (int k = a + 1; k < nf; ++k) y -= w.A[(L.fr[k] * ndof + i) * vs] * w.x[L.fr[k] * vs];
        y /= w.ld[a * vs];
        w.x[i * vs] = y;
        good = good && isfinite(y);
      }
    }
    *ok = good ? 1 : 0;
  }
  sync();
  return active && *ok != 0;
}

// the workgroup's copy of the joint lists: lane 0 writes them (uniform indices into the kernel argument), a barrier follows
__device__ inline FdLists fd_lists_to_lds(const FdSets& s, int* ilds, int lane) {
  if (lane == 0)
    for (int j = 0; j < GTO_MAX_DOF; ++j) ilds[j] = s.col[j], ilds[GTO_MAX_DOF + j] = s.fr[j], ilds[2 * GTO_MAX_DOF + j] = s.is_free[j];
  return {ilds, ilds + GTO_MAX_DOF, ilds + 2 * GTO_MAX_DOF, s.ndof, s.nc, s.nf};
}

// gto_forward_dynamics: qdd_out [n][ndof], M_out [n][ndof][ndof] (or null), status_out [n] (or null) of the rows (q, qd, tau)
// [n][ndof].  One lane per row, `rows` per 64-lane workgroup (fd_rows_per_block); dynamic LDS: the rt_rnea columns
// [F * GTO_RNEA_SLOTS][rows], the work arrays [ndof^2 + GTO_FD_VECS ndof][rows], then the ints: three joint lists and
// ok [rows].  sets.col lists every joint some frame names (the columns of M_out), sets.fr the free ones.
__global__ __launch_bounds__(GTO_WAVE) void k_forward_dynamics(const RobotDev* __restrict__ rb, const DynDev* __restrict__ dyn, FdSets sets,
                                                               int n, int rows, const double* __restrict__ q, const double* __restrict__ qd,
                                                               const double* __restrict__ tau, const double* __restrict__ pl_mass,
                                                               const double* __restrict__ pl_com, const double* __restrict__ pl_inertia,
                                                               double* __restrict__ qdd_out, double* __restrict__ M_out,
                                                               int32_t* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) double smem_fd[];
  const int lane = threadIdx.x, ndof = sets.ndof, F = rb->n_frames;
  double* wk = smem_fd + (size_t)GTO_RNEA_SLOTS * F * rows;
  int* ilds = (int*)(wk + (size_t)fd_work_doubles(ndof, GTO_FD_VECS) * rows);
  const FdLists L = fd_lists_to_lds(sets, ilds, lane);
  __syncthreads();
  const size_t row = (size_t)blockIdx.x * rows + lane;
  if (lane >= rows || row >= (size_t)n) return;
  int* ok = ilds + 3 * GTO_MAX_DOF + lane;
  FdWork w;
  w.vs = rows;
  w.A = wk + lane;
  double* v = w.A + (size_t)ndof * ndof * rows;
  w.q = v, w.qd = v + (size_t)ndof * rows, w.tau = v + (size_t)2 * ndof * rows, w.g = v + (size_t)3 * ndof * rows;
  w.c = v + (size_t)4 * ndof * rows, w.ld = v + (size_t)5 * ndof * rows, w.x = v + (size_t)6 * ndof * rows;
  bool finite = true;
  for (int j = 0; j < ndof; ++j) {
    const double a = q[row * ndof + j], b = qd[row * ndof + j], t = tau[row * ndof + j];
    w.q[j * rows] = a, w.qd[j * rows] = b, w.tau[j * rows] = t;
    finite = finite && isfinite(a) && isfinite(b) && isfinite(t);
  }
  for (int e = 0; e < ndof * ndof; ++e) w.A[e * rows] = 0.0;  // the columns of joints no frame names stay 0
  const RneaPayload pl = rnea_payload(pl_mass, pl_com, pl_inertia, row);
  const bool good = fd_solve(rb, dyn, pl, smem_fd + lane, rows, 1, 0, finite, L, w, ok, FdNoSync()) && finite;
  for (int j = 0; j < ndof; ++j) qdd_out[row * ndof + j] = good ? w.x[j * rows] : NAN;
  if (M_out)
    for (int i = 0; i < ndof; ++i)
      for (int j = 0; j < ndof; ++j)
        M_out[(row * ndof + i) * ndof + j] = good ? (i <= j ? w.A[(i * ndof + j) * rows] : w.A[(j * ndof + i) * rows]) : NAN;
  if (status_out) status_out[row] = good ? GTO_STATUS_CONVERGED : GTO_STATUS_NUMERICAL;
}

// The controller and the clock of k_track_rollout, by value as RetimeLimits (copied into LDS by lane 0 before a lane
// indexes them).
struct TrackParams {
  double kp[GTO_MAX_DOF], kd[GTO_MAX_DOF], tau_max[GTO_MAX_DOF];
  double dt, settle;
  int32_t B, M, Mo, feedforward, G, P;  // G lanes per path, P paths per workgroup (track_group_lanes, track_paths_per_block)
};
struct TrackRef {
  const double *duration, *q, *qd, *qdd;  // [B], [B][M][ndof]
};
struct TrackPayloads {
  const double *m_mass, *m_com, *m_inertia, *p_mass, *p_com, *p_inertia;  // model and plant: [B], [B][3], [B][6] or null
};
struct TrackOut {
  double *q, *qd, *t, *err_max, *err_end;
  int32_t *sat_steps, *steps, *status;
};

// The reference of joint j at time t: the cubic Hermite interpolant of the samples (q_m, qd_m) at linspace(0, dur, M), its
// derivative, and the acceleration samples joined by straight lines; from t = dur on (and where dur = 0) the last sample
// at rest.  qr / qdr / qddr: the path's samples of joint j, `ndof` apart.
__device__ inline void track_ref(double t, double dur, int M, int ndof, const double* qr, const double* qdr, const double* qddr,
                                 double& q, double& qd, double& qdd) {
  if (!(t < dur)) {
    q = qr[(size_t)(M - 1) * ndof], qd = 0.0, qdd = 0.0;
    return;
  }
  const double h = dur / (double)(M - 1), s = t / dur * (double)(M - 1);
  int i = (int)s;
  i = i > M - 2 ? M - 2 : i;
  const double u = s - (double)i, u2 = u * u, u3 = u2 * u;
  const double q0 = qr[(size_t)i * ndof], q1 = qr[(size_t)(i + 1) * ndof], v0 = qdr[(size_t)i * ndof], v1 = qdr[(size_t)(i + 1) * ndof];
  const double h00 = 2.0 * u3 - 3.0 * u2 + 1.0, h10 = u3 - 2.0 * u2 + u, h01 = 3.0 * u2 - 2.0 * u3, h11 = u3 - u2;
  const double d00 = 6.0 * u2 - 6.0 * u, d10 = 3.0 * u2 - 4.0 * u + 1.0, d11 = 3.0 * u2 - 2.0 * u;
  q = h00 * q0 + h10 * (h * v0) + h01 * q1 + h11 * (h * v1);
  qd = d00 * (q0 - q1) / h + d10 * v0 + d11 * v1;
  qdd = (1.0 - u) * qddr[(size_t)i * ndof] + u * qddr[(size_t)(i + 1) * ndof];
}

// gto_track_rollout[_device]: path b of the call runs on group b % P of workgroup b / P, G lanes of the one wave.  Per
// control period: the reference and the feedforward (one rt_rnea pass with the MODEL payload, on the group's lane 0), the
// clipped control law, then one classical RK4 step of qdd = FD_plant(q, qd, tau) -- four fd_solve evaluations with the PLANT
// payload, their passes spread over the group.  Every lane of the workgroup walks the same loop to the workgroup's largest
// step count (the barriers inside fd_solve want everybody); a group whose path has ended or failed passes through with
// active = false, which changes nothing for its neighbours.
// Dynamic LDS: rt_rnea columns [F * GTO_RNEA_SLOTS][P G]; per path ndof^2 + GTO_TR_VECS ndof doubles; kp, kd, tau_max;
// then ints: the joint lists, and per path ok, K, sat, spare.
__global__ __launch_bounds__(GTO_WAVE) void k_track_rollout(const RobotDev* __restrict__ rb, const DynDev* __restrict__ dyn, TrackParams prm,
                                                            FdSets sets, TrackRef ref, TrackPayloads pay, TrackOut out) {
  extern __shared__ __attribute__((aligned(16))) double smem_fd[];
  const int lane = threadIdx.x, ndof = sets.ndof, F = rb->n_frames, G = prm.G, P = prm.P, M = prm.M, Mo = prm.Mo;
  const int stride = P * G, grp = lane / G, gl = lane - grp * G;
  const int per_path = fd_work_doubles(ndof, GTO_TR_VECS);
  double* gains = smem_fd + (size_t)GTO_RNEA_SLOTS * F * stride + (size_t)per_path * P;
  int* ilds = (int*)(gains + 3 * ndof);
  const FdLists L = fd_lists_to_lds(sets, ilds, lane);
  if (lane == 0)
    for (int j = 0; j < ndof; ++j) gains[j] = prm.kp[j], gains[ndof + j] = prm.kd[j], gains[2 * ndof + j] = prm.tau_max[j];
  const double *kp = gains, *kd = gains + ndof, *tmax = gains + 2 * ndof;
  const long long b = (long long)blockIdx.x * P + grp;
  const bool valid = grp < P && b < prm.B;
  const int g0 = valid ? grp : 0;  // a lane without a path points at group 0's arrays and never touches them
  int* flags = ilds + 3 * GTO_MAX_DOF + 4 * g0;  // ok, K, sat
  int* kmax = ilds + 3 * GTO_MAX_DOF + 4 * P;
  double* base = smem_fd + (size_t)GTO_RNEA_SLOTS * F * stride + (size_t)per_path * g0;
  FdWork w;
  w.vs = 1;
  w.A = base;
  double* v = base + ndof * ndof;
  double *qs = v, *qds = v + ndof;  // the stage's state: what fd_solve reads
  w.q = qs, w.qd = qds, w.tau = v + 2 * ndof, w.g = v + 3 * ndof, w.c = v + 4 * ndof, w.ld = v + 5 * ndof, w.x = v + 6 * ndof;
  double *sq = v + 7 * ndof, *sqd = v + 8 * ndof, *aq = v + 9 * ndof, *aqd = v + 10 * ndof, *ff = v + 11 * ndof;
  double *rq = v + 12 * ndof, *rqd = v + 13 * ndof, *rqdd = v + 14 * ndof;
  double* st = smem_fd + (valid ? lane : 0);
  const double dt = prm.dt;
  const double* qref = ref.q + (valid ? b : 0) * M * ndof;
  const double* qdref = ref.qd + (valid ? b : 0) * M * ndof;
  const double* qddref = ref.qdd + (valid ? b : 0) * M * ndof;

  // ---- the path's clock and its checks
  double dur = 0.0;
  if (valid && gl == 0) {
    dur = ref.duration[b];
    const double Kd = ceil((dur + prm.settle) / dt);
    bool good = isfinite(dur) && dur >= 0.0 && Kd >= 1.0 && Kd <= (double)GTO_TRACK_MAX_STEPS;
    for (int k = 0; k < 2; ++k) {  // a payload the host never saw
      const double* m = k ? pay.p_mass : pay.m_mass;
      if (m) good = good && m[b] >= 0.0 && isfinite(m[b]);
    }
    flags[0] = good ? 1 : 0, flags[1] = good ? (int)Kd : 0, flags[2] = 0;
  }
  __syncthreads();
  if (valid) {
    dur = ref.duration[b];
    bool fin = true;  // the free joints' samples, and where the locked ones stand
    for (int e = gl; e < M * ndof; e += G) {
      const int j = e % ndof;
      if (L.is_free[j]) fin = fin && isfinite(qref[e]) && isfinite(qdref[e]) && isfinite(qddref[e]);
      else if (e < ndof) fin = fin && isfinite(qref[e]);
    }
    if (!fin) flags[0] = 0;
  }
  __syncthreads();
  const RneaPayload pl_plant = rnea_payload(pay.p_mass, pay.p_com, pay.p_inertia, (size_t)(valid ? b : 0));
  const RneaPayload pl_model = rnea_payload(pay.m_mass, pay.m_com, pay.m_inertia, (size_t)(valid ? b : 0));
  const int K = valid ? flags[1] : 0;
  if (lane == 0) {
    int km = 0;
    for (int p = 0; p < P; ++p) {
      const int* f = ilds + 3 * GTO_MAX_DOF + 4 * p;
      if ((long long)blockIdx.x * P + p < prm.B && f[0] && f[1] > km) km = f[1];
    }
    *kmax = km;
  }
  if (valid && flags[0])
    for (int j = gl; j < ndof; j += G) {
      const bool fr = L.is_free[j] != 0;
      double a, bb, cc;
      track_ref(0.0, dur, M, ndof, qref + j, qdref + j, qddref + j, a, bb, cc);
      sq[j] = qref[j], sqd[j] = fr ? qdref[j] : 0.0;
      rq[j] = fr ? a : qref[j], rqd[j] = fr ? bb : 0.0, rqdd[j] = fr ? cc : 0.0;
      ff[j] = 0.0;
    }
  __syncthreads();
  const int Kmax = *kmax;
  double emax = 0.0, eend = 0.0;
  int sat = 0, m_next = 0;
  // sample m is the state after step floor(m K / (Mo - 1)): the ones that are the start state
  auto emit = [&](int kdone) {
    while (m_next < Mo && (long long)m_next * K / (Mo - 1) == kdone) {
      const size_t o = (size_t)b * Mo + m_next;
      for (int j = gl; j < ndof; j += G) {
        if (out.q) out.q[o * ndof + j] = sq[j];
        if (out.qd) out.qd[o * ndof + j] = sqd[j];
      }
      if (gl == 0 && out.t) out.t[o] = (double)kdone * dt;
      ++m_next;
    }
  };
  if (valid && flags[0]) emit(0);

  for (int k = 0; k < Kmax; ++k) {
    bool run = valid && flags[0] != 0 && k < K;
    // ---- the controller, at the period's start
    if (run && gl == 0 && prm.feedforward != 0) {
      const bool full = prm.feedforward == 2;
      rt_rnea(
          rb, dyn, pl_model, st, stride, [&](int j) { return rq[j]; }, [&](int j) { return full ? rqd[j] : 0.0; },
          [&](int j) { return full ? rqdd[j] : 0.0; }, [&](int j, double val) { ff[j] = val; });
    }
    __syncthreads();
    if (run)
      for (int j = gl; j < ndof; j += G) {
        double t = 0.0;
        if (L.is_free[j]) {
          const double raw = ff[j] + kp[j] * (rq[j] - sq[j]) + kd[j] * (rqd[j] - sqd[j]);
          t = raw != raw ? raw : fmin(fmax(raw, -tmax[j]), tmax[j]);  // (a NaN stays one: the solve reports it)
          if (t != raw && raw == raw) flags[2] = 1;
        }
        w.tau[j] = t;
        qs[j] = sq[j], qds[j] = sqd[j], aq[j] = 0.0, aqd[j] = 0.0;
      }
    // ---- the plant: one RK4 step under the held torque
    for (int s = 0; s < 4; ++s) {
      const bool good = fd_solve(rb, dyn, pl_plant, st, stride, G, gl, run, L, w, flags, FdBlockSync());
      run = run && good;
      if (run) {
        const double wt = (s == 0 || s == 3) ? 1.0 : 2.0, cs = s == 2 ? dt : 0.5 * dt;
        for (int j = gl; j < ndof; j += G) {
          if (!L.is_free[j]) continue;
          const double kq = qds[j], kv = w.x[j];
          aq[j] += wt * kq, aqd[j] += wt * kv;
          if (s < 3) qs[j] = sq[j] + cs * kq, qds[j] = sqd[j] + cs * kv;
          else sq[j] += dt / 6.0 * aq[j], sqd[j] += dt / 6.0 * aqd[j];
        }
      }
    }
    // ---- the period's end: the reference there (the next period's start), the error, the samples
    if (run) {
      const double t1 = (double)(k + 1) * dt;
      for (int j = gl; j < ndof; j += G) {
        if (!L.is_free[j]) continue;
        double a, bb, cc;
        track_ref(t1, dur, M, ndof, qref + j, qdref + j, qddref + j, a, bb, cc);
        rq[j] = a, rqd[j] = bb, rqdd[j] = cc;
      }
    }
    __syncthreads();
    if (run) {
      double e = 0.0;
      bool fin = true;
      for (int a = 0; a < L.nf; ++a) {  // every lane of the group: the same values in the same order
        const int j = L.fr[a];
        fin = fin && isfinite(sq[j]) && isfinite(sqd[j]);
        e = fmax(e, fabs(sq[j] - rq[j]));
      }
      sat += flags[2];
      emax = fmax(emax, e), eend = e;
      if (fin) emit(k + 1);
      run = fin;
    }
    __syncthreads();
    if (valid && gl == 0 && k < K) {
      flags[2] = 0;
      if (!run) flags[0] = 0;
    }
    __syncthreads();
  }

  if (!valid) return;
  const bool good = flags[0] != 0;
  if (!good) {
    for (size_t e = gl; e < (size_t)Mo * ndof; e += G) {
      if (out.q) out.q[(size_t)b * Mo * ndof + e] = NAN;
      if (out.qd) out.qd[(size_t)b * Mo * ndof + e] = NAN;
    }
    for (int m = gl; m < Mo; m += G)
      if (out.t) out.t[(size_t)b * Mo + m] = NAN;
  }
  if (gl == 0) {
    if (out.err_max) out.err_max[b] = good ? emax : NAN;
    if (out.err_end) out.err_end[b] = good ? eend : NAN;
    if (out.sat_steps) out.sat_steps[b] = good ? sat : 0;
    if (out.steps) out.steps[b] = good ? K : 0;
    if (out.status) out.status[b] = good ? GTO_STATUS_CONVERGED : GTO_STATUS_NUMERICAL;
  }
}
