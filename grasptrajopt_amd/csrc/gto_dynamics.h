// gto_dynamics.h — inverse dynamics of the handle's frame tree (gfx950): rt_rnea and the kernel of gto_inverse_dynamics.
//
// Recursive Newton-Euler in each frame's own coordinates, fixed base, FP64 throughout, no atomics.  Frame f is the rigid
// body that joint f moves (DynDev: mass, centre of mass, inertia about it); the payload is a second body on frame_ee.
//
// Layout.  One lane owns one row (a configuration with its velocity and acceleration) and walks the frames serially,
// parents first and then back: the recursion over a tree of at most 32 frames has no parallelism worth a reduction, and a
// row's result then depends on nothing but the row (no position in the launch, no neighbour, no n).  The per-frame state
// is what a later frame may ask of ANY earlier one, so it cannot sit in registers without a run-time index (which would
// put it in scratch memory).  It lives in LDS, GTO_RNEA_SLOTS doubles per frame for the handle's real n_frames:
//   slots 0-8    angular velocity, angular acceleration and the linear acceleration of the frame's origin (forward pass)
//   slots 9-14   force and moment about the frame's origin of the body and, after the backward pass reaches the frame, of
//                everything below it
// as st[(f * GTO_RNEA_SLOTS + slot) * stride + lane]: the lanes of a wave read consecutive doubles of one (frame, slot),
// all at the same frame, so every access is free of bank conflicts.  The joint's sine and cosine are computed again on the
// way back instead of being kept (two more slots per frame cost more rows per workgroup than a sincos costs time).  The
// robot's tables come through scalar loads (uniform addresses).  A lane touches its own column only: no barrier.
#pragma once
#include "gto_device.h"

#define GTO_RNEA_SLOTS 15
#define GTO_RNEA_LDS_BYTES (64 * 1024)  // per workgroup: the rows of a launch are few, more workgroups reach more CUs

// rows one 64-lane workgroup of rt_rnea's callers holds for a tree of F frames
__host__ __device__ inline int rnea_rows_per_block(int F) {
  const int r = GTO_RNEA_LDS_BYTES / (GTO_RNEA_SLOTS * F * (int)sizeof(double));
  return r < GTO_WAVE ? r : GTO_WAVE;
}

struct V3 {
  double x, y, z;
};
__device__ inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// R v and R^T v for the rotation of a row-major 3x4 affine
__device__ inline V3 aff_rot(const double* O, V3 v) {
  return {O[0] * v.x + O[1] * v.y + O[2] * v.z, O[4] * v.x + O[5] * v.y + O[6] * v.z, O[8] * v.x + O[9] * v.y + O[10] * v.z};
}
__device__ inline V3 aff_rot_t(const double* O, V3 v) {
  return {O[0] * v.x + O[4] * v.y + O[8] * v.z, O[1] * v.x + O[5] * v.y + O[9] * v.z, O[2] * v.x + O[6] * v.y + O[10] * v.z};
}
// rotation about the unit axis u by the angle whose sine and cosine are s, c (Rodrigues)
__device__ inline V3 axis_rot(V3 u, double s, double c, V3 v) { return c * v + s * cross(u, v) + ((1.0 - c) * dot(u, v)) * u; }

__device__ inline V3 rnea_load(const double* st, int stride, int f, int slot) {
  const double* p = st + (size_t)(f * GTO_RNEA_SLOTS + slot) * stride;
  return {p[0], p[stride], p[2 * stride]};
}
__device__ inline void rnea_store(double* st, int stride, int f, int slot, V3 v) {
  double* p = st + (size_t)(f * GTO_RNEA_SLOTS + slot) * stride;
  p[0] = v.x, p[stride] = v.y, p[2 * stride] = v.z;
}

// Frame f against its parent: a vector of f reads E v = R_o rot(u, q) v in the parent (R_o the origin's rotation; the joint
// of a prismatic or fixed frame does not turn), and f's origin sits at r in the parent.
struct RneaJoint {
  const double* O;
  V3 u, r;
  double s, c;
  __device__ V3 to_parent(V3 v) const { return aff_rot(O, axis_rot(u, s, c, v)); }
  __device__ V3 to_child(V3 v) const { return axis_rot(u, -s, c, aff_rot_t(O, v)); }
};
__device__ inline RneaJoint rnea_joint(const RobotDev* rb, int f, int jt, double qv) {
  RneaJoint J;
  J.O = rb->origin[f];
  J.u = {rb->axis_unit[f][0], rb->axis_unit[f][1], rb->axis_unit[f][2]};
  J.s = 0.0, J.c = 1.0;
  J.r = {J.O[3], J.O[7], J.O[11]};
  if (jt == GTO_JOINT_REVOLUTE) sincos(qv, &J.s, &J.c);
  else if (jt == GTO_JOINT_PRISMATIC) J.r = J.r + aff_rot(J.O, qv * J.u);
  return J;
}

// Newton and Euler for one rigid body on a frame that turns with w, wd and whose origin accelerates with a: the force on
// the body and its moment about the frame's origin are ADDED to F, N.
__device__ inline void rnea_body(double m, V3 c, double ixx, double ixy, double ixz, double iyy, double iyz, double izz, V3 w, V3 wd,
                                 V3 a, V3& F, V3& N) {
  const V3 ac = a + cross(wd, c) + cross(w, cross(w, c));
  const V3 Fb = m * ac;
  const V3 Iw = {ixx * w.x + ixy * w.y + ixz * w.z, ixy * w.x + iyy * w.y + iyz * w.z, ixz * w.x + iyz * w.y + izz * w.z};
  const V3 Iwd = {ixx * wd.x + ixy * wd.y + ixz * wd.z, ixy * wd.x + iyy * wd.y + iyz * wd.z, ixz * wd.x + iyz * wd.y + izz * wd.z};
  F = F + Fb;
  N = N + Iwd + cross(w, Iw) + cross(c, Fb);
}

// A rigid body in frame_ee's coordinates: mass, centre of mass, inertia about it (ixx ixy ixz iyy iyz izz).
struct RneaPayload {
  double m;
  V3 c;
  double I[6];
};
// row `row` of the entry points' payload arrays, any of which may be null (no payload, centre at the origin, a point mass)
__device__ inline RneaPayload rnea_payload(const double* mass, const double* com, const double* inertia, size_t row) {
  RneaPayload p = {0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
  if (mass) p.m = mass[row];
  if (com) p.c = {com[3 * row], com[3 * row + 1], com[3 * row + 2]};
  if (inertia)
#pragma unroll
    for (int k = 0; k < 6; ++k) p.I[k] = inertia[6 * row + k];
  return p;
}

// Generalised forces of one row.  q, qd, qdd: callables joint index -> value; out: callable (joint index, force), called once
// for the joint of every actuated frame (the caller zeroes the joints no frame names).  st: the calling lane's column of
// the workgroup's state, st[(f * GTO_RNEA_SLOTS + slot) * stride].
template <class Q, class Qd, class Qdd, class Out>
__device__ inline void rt_rnea(const RobotDev* __restrict__ rb, const DynDev* __restrict__ dyn, const RneaPayload& pl, double* st,
                               int stride, Q q, Qd qd, Qdd qdd, Out out) {
  const int F = rb->n_frames, fee = rb->frame_ee;
  const V3 zero = {0.0, 0.0, 0.0};
  const V3 a_base = {-dyn->gravity[0], -dyn->gravity[1], -dyn->gravity[2]};  // a base that falls upwards: gravity on every body
  for (int f = 0; f < F; ++f) {
    const int p = rb->parent[f], jt = rb->joint_type[f], qi = rb->q_index[f];
    const bool act = jt != GTO_JOINT_FIXED && qi >= 0;
    const RneaJoint J = rnea_joint(rb, f, jt, act ? q(qi) : 0.0);
    const V3 wp = p >= 0 ? rnea_load(st, stride, p, 0) : zero, wdp = p >= 0 ? rnea_load(st, stride, p, 3) : zero;
    const V3 ap = p >= 0 ? rnea_load(st, stride, p, 6) : a_base;
    V3 w = J.to_child(wp), wd = J.to_child(wdp);
    V3 a = J.to_child(ap + cross(wdp, J.r) + cross(wp, cross(wp, J.r)));
    if (act) {
      const V3 uv = qd(qi) * J.u, ua = qdd(qi) * J.u;
      if (jt == GTO_JOINT_REVOLUTE) {
        wd = wd + ua + cross(w, uv);
        w = w + uv;
      } else {
        a = a + ua + 2.0 * cross(w, uv);
      }
    }
    rnea_store(st, stride, f, 0, w);
    rnea_store(st, stride, f, 3, wd);
    rnea_store(st, stride, f, 6, a);
    V3 Fb = zero, Nb = zero;
    const double m = dyn->mass[f];
    if (m > 0.0) {
      const double* I = dyn->inertia[f];
      rnea_body(m, {dyn->com[f][0], dyn->com[f][1], dyn->com[f][2]}, I[0], I[1], I[2], I[3], I[4], I[5], w, wd, a, Fb, Nb);
    }
    if (f == fee && pl.m > 0.0) rnea_body(pl.m, pl.c, pl.I[0], pl.I[1], pl.I[2], pl.I[3], pl.I[4], pl.I[5], w, wd, a, Fb, Nb);
    rnea_store(st, stride, f, 9, Fb);
    rnea_store(st, stride, f, 12, Nb);
  }
  for (int f = F - 1; f >= 0; --f) {  // children come after their parents: frame f holds its whole subtree by now
    const int p = rb->parent[f], jt = rb->joint_type[f], qi = rb->q_index[f];
    const bool act = jt != GTO_JOINT_FIXED && qi >= 0;
    const V3 Ff = rnea_load(st, stride, f, 9), Nf = rnea_load(st, stride, f, 12);
    const V3 u = {rb->axis_unit[f][0], rb->axis_unit[f][1], rb->axis_unit[f][2]};
    if (act) out(qi, jt == GTO_JOINT_REVOLUTE ? dot(u, Nf) : dot(u, Ff));
    if (p < 0) continue;
    const RneaJoint J = rnea_joint(rb, f, jt, act ? q(qi) : 0.0);
    const V3 Fp = J.to_parent(Ff);
    rnea_store(st, stride, p, 9, rnea_load(st, stride, p, 9) + Fp);
    rnea_store(st, stride, p, 12, rnea_load(st, stride, p, 12) + J.to_parent(Nf) + cross(J.r, Fp));
  }
}

// gto_inverse_dynamics: tau_out [n][ndof] of the rows (q, qd, qdd) [n][ndof], `rows` of them per workgroup of 64 lanes
// (rnea_rows_per_block), dynamic LDS rows * n_frames * GTO_RNEA_SLOTS doubles.
__global__ __launch_bounds__(GTO_WAVE) void k_inverse_dynamics(const RobotDev* __restrict__ rb, const DynDev* __restrict__ dyn, int n,
                                                               int rows, const double* __restrict__ q, const double* __restrict__ qd,
                                                               const double* __restrict__ qdd, const double* __restrict__ pl_mass,
                                                               const double* __restrict__ pl_com, const double* __restrict__ pl_inertia,
                                                               double* __restrict__ tau_out) {
  extern __shared__ __attribute__((aligned(16))) double smem_rnea[];
  const int lane = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * rows + lane;
  if (lane >= rows || row >= (size_t)n) return;
  const int ndof = rb->ndof;
  const double *qr = q + row * ndof, *qdr = qd + row * ndof, *qddr = qdd + row * ndof;
  double* tr = tau_out + row * ndof;
  for (int j = 0; j < ndof; ++j) tr[j] = 0.0;
  const RneaPayload pl = rnea_payload(pl_mass, pl_com, pl_inertia, row);
  rt_rnea(rb, dyn, pl, smem_rnea + lane, rows, [&](int j) { return qr[j]; }, [&](int j) { return qdr[j]; },
          [&](int j) { return qddr[j]; }, [&](int j, double v) { tr[j] = v; });
}
