// gto_retrieve.h — the motion after the grasp (examples/pybullet_gto_planning.py:301-313), stream-ordered (gfx950):
//   k_retrieve_lift     the tabletop branch (:307-308; pybullet_scenereplica.py:597-613): fingers closed, then K steps of
//                       link_ee along a straight line, each an IK problem seeded from the step before.  One workgroup of
//                       256 per plan runs the whole chain: the FK tables are staged once, RT0 is evaluated, and every step
//                       is ik_lm_loop<GTO_IK_GOAL_POINTS> (k_ik_solve's loop, the same code) on a goal that lives in LDS.
//                       Between steps nothing leaves the chip but the step's column and its record.
//   k_retrieve_reverse  the shelf branch (:309-313): the plan's last stretch backwards, fingers closed; a gather.
// The reference's lift is pybullet's position-only null-space IK, which is not available here and would let the held object
// tilt; this chain holds the gripper's full pose (the point-matching pose term of gto_solve_ik_batch).
#pragma once
#include "gto_seed.h"

// the joints a retrieve path holds closed: bit d of mask set -> actuated joint d takes value[d] in every column
struct RetrieveClosed {
  uint32_t mask;
  double value[GTO_MAX_DOF];
};
struct RetrieveLine {
  double dir[3];  // as given
  double step;    // distance / K
  int K;
  double pos_tol, rot_tol_deg;
};

// the IK kernel's LDS, then RT0 [16] and the goal of the step [16]
__host__ __device__ inline int retrieve_lds_doubles(int F, int L, int n) { return ik_lds_doubles(F, L, n) + 32; }

// translation entry of goal k: one product, one product, one sum, each rounded once
__device__ __forceinline__ double retrieve_goal_entry(double p0, int k, double step, double dir) {
#pragma clang fp contract(off)
  const double s = (double)k * step;
  const double d = s * dir;
  return p0 + d;
}

__global__ __launch_bounds__(256, GTO_IK_MIN_WAVES) void k_retrieve_lift(
    const RobotDev* __restrict__ rb, const double* __restrict__ px, const double* __restrict__ py, const double* __restrict__ pz,
    const Chunk* __restrict__ chunks, const SceneDev* __restrict__ scenes, int n_scenes, const int32_t* __restrict__ scene_id,
    const double* __restrict__ plans /*[B][ndof][T]*/, int T, const double* __restrict__ base_pos, SolveParams sp, RetrieveClosed cl,
    RetrieveLine ln, double* __restrict__ path_out /*[B][ndof][K+1]*/, double* __restrict__ goals_out /*[B][K][16]*/,
    double* __restrict__ err_pos_out, double* __restrict__ err_rot_out, int32_t* __restrict__ iters_out,
    int32_t* __restrict__ status_out /*[B][K]*/, int32_t* __restrict__ reached_out /*[B]*/) {
  extern __shared__ __attribute__((aligned(16))) double smem_rl[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = rb->n_frames, L = rb->n_links, n = rb->n_opt, ndof = rb->ndof, K = ln.K, C = K + 1;
  const IkLds m = ik_lds(smem_rl, F, L, n);
  double* const s_rt0 = smem_rl + ik_lds_doubles(F, L, n);
  double* const s_goal = s_rt0 + 16;
  const bool collide = scene_id != nullptr;
  double* const path = path_out + (size_t)b * ndof * C;
  {
    const int nt = fk_tab_doubles(F, L, n);
    for (int k = tid; k < nt; k += 256) m.tab[k] = rb->fk_tab[k];
    if (tid < L) m.anc[tid] = (int)rb->link_anc[tid];
    if (tid < ndof) {  // column 0: the plan's last waypoint with the fingers closed
      const double v = ((cl.mask >> tid) & 1u) ? cl.value[tid] : plans[((size_t)b * ndof + tid) * T + T - 1];
      m.qf[tid] = v;
      path[(size_t)tid * C] = v;
    }
  }
  __syncthreads();
  bool finite = true;
  for (int d = 0; d < ndof; ++d) finite = finite && isfinite(m.qf[d]);
  if (!finite) {  // (block-uniform) no chain to run: every column is column 0
    for (int i = tid; i < ndof * K; i += 256) {
      const int d = i / K, k = 1 + i - d * K;
      path[(size_t)d * C + k] = m.qf[d];
    }
    for (int i = tid; i < K; i += 256) {
      const size_t o = (size_t)b * K + i;
      if (err_pos_out) err_pos_out[o] = NAN;
      if (err_rot_out) err_rot_out[o] = NAN;
      if (iters_out) iters_out[o] = 0;
      if (status_out) status_out[o] = GTO_STATUS_NUMERICAL;
    }
    if (goals_out)
      for (int i = tid; i < K * 16; i += 256) goals_out[(size_t)b * K * 16 + i] = (i & 15) < 12 ? NAN : ((i & 15) == 15 ? 1.0 : 0.0);
    if (tid == 0 && reached_out) reached_out[b] = 0;
    return;
  }
  SceneDev sc = {};
  double bx = 0.0, by = 0.0, bz = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
  bool no_scene = false;  // an id that names no scene with voxel records: k_ik_solve's rule, at every step
  if (collide) {
    const int sid = scene_id[b];
    no_scene = (unsigned)sid >= (unsigned)n_scenes || !scenes[sid].valid || !scenes[sid].r_obs;
    if (!no_scene) {
      sc = scenes[sid];
      bx = base_pos[3 * b], by = base_pos[3 * b + 1], bz = base_pos[3 * b + 2];
      cx = (bx - sc.ox) * sc.rinv, cy = (by - sc.oy) * sc.rinv, cz = (bz - sc.oz) * sc.rinv;
    }
  }
  // the kinematics of the configuration in m.qf (optimised joints from m.x when from_x), as k_eval_kin and k_ik_report pose
  // one: afterwards the transposed frames are at Xg (fkx), behind a barrier
  const double* const Xg = m.X + (rb->fk_rounds & 1) * 16 * F;
  auto pose = [&](bool from_x) {
    if (tid < F) {
      const int jt = rb->joint_type[tid], dq = rb->q_index[tid];
      double a = 0.0, cs = 1.0;
      if (dq >= 0) {
        const int j = rb->opt_of_dof[dq];
        const double qv = (from_x && j >= 0) ? m.x[j] : m.qf[dq];
        if (jt == GTO_JOINT_REVOLUTE) sincos(qv, &a, &cs);
        else if (jt == GTO_JOINT_PRISMATIC) a = qv;
      }
      m.sc[2 * tid] = a;
      m.sc[2 * tid + 1] = cs;
    }
    __syncthreads();
    fk_mfma_tree(rb, m.tab, 1, m.sc, m.X, reinterpret_cast<int*>(m.X + 32 * F + 64), tid, m.vis, m.screw);
    __syncthreads();
  };
  pose(false);
  if (tid < 16) {  // RT0: link_ee at column 0, the entries gto_eval_fk writes
    double v = Xg[fkx(rb->frame_ee, 4 * (tid & 3) + (tid >> 2))];
    if (tid >= 12) v = (tid == 15) ? 1.0 : 0.0;
    s_rt0[tid] = v;
  }
  int reached = 0;
  bool leading = true;  // (thread 0's)
  for (int k = 1; k <= K; ++k) {
    __syncthreads();  // s_rt0 written; the step before has read its goal
    if (tid < 16) {
      double v = s_rt0[tid];
      if (tid < 12 && (tid & 3) == 3) v = retrieve_goal_entry(v, k, ln.step, ln.dir[tid >> 2]);
      s_goal[tid] = v;
      if (goals_out) goals_out[((size_t)b * K + (k - 1)) * 16 + tid] = v;
    }
    if (tid >= 64 && tid < 72) {  // the seed: column k - 1, clipped as k_ik_solve clips its q0
      const int j = tid - 64;
      double v = 0.0;
      if (j < n) v = fmin(fmax(m.qf[rb->opt_index[j]], rb->lower[j]), rb->upper[j]);
      m.xt[j] = v;
      m.x[j] = v;
    }
    double f = NAN;
    int it = 0, status = GTO_STATUS_NUMERICAL;
    if (no_scene) __syncthreads();
    else ik_lm_loop<GTO_IK_GOAL_POINTS>(rb, px, py, pz, chunks, m, collide, sc, bx, by, bz, cx, cy, cz, s_goal, sp, tid, lane, wave, &f, &it, &status);
    (void)f;
    if (tid < ndof) {  // column k
      const int j = rb->opt_of_dof[tid];
      const double v = j >= 0 ? m.x[j] : m.qf[tid];
      path[(size_t)tid * C + k] = v;
    }
    pose(true);  // (m.qf's optimised entries are read by nobody in it)
    if (tid < ndof) {
      const int j = rb->opt_of_dof[tid];
      if (j >= 0) m.qf[tid] = m.x[j];
    }
    if (tid == 0) {
      double ep, er;
      seed_pose_errors(Xg, rb->frame_ee, s_goal, &ep, &er);
      const size_t o = (size_t)b * K + (k - 1);
      if (err_pos_out) err_pos_out[o] = ep;
      if (err_rot_out) err_rot_out[o] = er;
      if (iters_out) iters_out[o] = it;
      if (status_out) status_out[o] = status;
      leading = leading && ep < ln.pos_tol && er < ln.rot_tol_deg && status != GTO_STATUS_NUMERICAL;
      reached += leading ? 1 : 0;
    }
  }
  if (tid == 0 && reached_out) reached_out[b] = reached;
}

// path_out [B][ndof][n_cols]: column i is column T - 2 - i of the plan (the reference's plan[:, arange(standoff_offset - 10,
// -1)][:, ::-1]: the last waypoint is not part of it), the closed joints' rows overwritten
__global__ __launch_bounds__(256) void k_retrieve_reverse(const double* __restrict__ plans, int ndof, int T, int n_cols, long long total,
                                                          RetrieveClosed cl, double* __restrict__ path_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % n_cols);
  const long long row = i / n_cols;  // b * ndof + d
  const int d = (int)(row % ndof);
  path_out[i] = ((cl.mask >> d) & 1u) ? cl.value[d] : plans[row * T + (T - 2 - c)];
}
