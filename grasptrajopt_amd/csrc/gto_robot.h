// gto_robot.h — the robot tables gto_create uploads, built on the host from the descriptor alone.
//
// Host only: no kernel, no HIP call, nothing of the handle.  build_robot() at the end is the one entry point: it judges the
// descriptor (check_descriptor) and then runs the passes below in order, each of which fills its own fields of RobotTables.
// tests/robot_tables_main.cpp builds this header into a stand-alone program under AddressSanitizer and UBSan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gto_device.h"

// Everything gto_create uploads for a robot.
struct RobotTables {
  RobotDev rb;
  std::vector<double> px, py, pz;  // surface points sorted by link, and inside a link along a Morton curve
  std::vector<int32_t> plink, perm;  // their links, and the descriptor's index of each
  std::vector<Chunk> chunks;  // runs of <= 64 points of one link
  std::vector<PbChunk> pbchunks;  // the step kernel's spheres (one dummy entry if no link moves)
  int pb_C = 0;  // spheres in pbchunks
};

// Rounds of pointer jumping that FK needs over a tree listed parents first: a frame at depth d is the product of d + 1
// local transforms, and r rounds compose 2^r of them.  n <= GTO_MAX_FRAMES.
inline int fk_rounds(const int* parent, int n) {
  int depth[GTO_MAX_FRAMES], maxd = 1, r = 0;
  for (int i = 0; i < n; ++i) {
    depth[i] = parent[i] < 0 ? 0 : depth[parent[i]] + 1;
    maxd = std::max(maxd, depth[i]);
  }
  while ((1 << r) < maxd + 1) ++r;
  return r;
}

namespace gto_robot {

inline double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// Every refusal that needs no table, in the order counts, optimised joints, frames, links, two links on a frame,
// point_link: a descriptor with several faults gets the message of the first.  Reads the descriptor only and fills nothing.
// After it the passes below index freely: every count fits its array, every index names an element.
inline int check_descriptor(const gto_robot_desc* d, std::string& why) {
  auto bad = [&](int code, const char* msg) {
    why = msg;
    return code;
  };
  if (d->n_frames < 1 || d->n_frames > GTO_MAX_FRAMES) return bad(GTO_ERR_UNSUPPORTED, "n_frames out of range (max 32)");
  if (d->n_links < 1 || d->n_links > GTO_MAX_LINKS) return bad(GTO_ERR_UNSUPPORTED, "n_links out of range (max 32)");
  if (d->n_opt < 1 || d->n_opt > GTO_MAX_OPT) return bad(GTO_ERR_UNSUPPORTED, "n_opt out of range (max 16)");
  if (d->ndof < d->n_opt || d->ndof > GTO_MAX_DOF) return bad(GTO_ERR_UNSUPPORTED, "ndof out of range (max 32)");
  if (d->n_points < 1) return bad(GTO_ERR_INVALID_ARG, "robot has no surface points");
  if (d->n_gripper_points < 1) return bad(GTO_ERR_INVALID_ARG, "robot has no gripper points");
  if (d->frame_ee < 0 || d->frame_ee >= d->n_frames || d->frame_gripper < 0 || d->frame_gripper >= d->n_frames)
    return bad(GTO_ERR_INVALID_ARG, "frame_ee / frame_gripper out of range");
  bool optimised[GTO_MAX_DOF] = {}, carries_link[GTO_MAX_FRAMES] = {};
  for (int j = 0; j < d->n_opt; ++j) {
    if (d->opt_index[j] < 0 || d->opt_index[j] >= d->ndof) return bad(GTO_ERR_INVALID_ARG, "opt_index out of range");
    if (optimised[d->opt_index[j]]) return bad(GTO_ERR_INVALID_ARG, "opt_index names a joint twice");
    optimised[d->opt_index[j]] = true;
    if (!(d->lower[j] <= d->upper[j])) return bad(GTO_ERR_INVALID_ARG, "lower > upper");
  }
  for (int i = 0; i < d->n_frames; ++i) {
    const int p = d->parent[i], jt = d->joint_type[i];
    if (p >= i || p < -1) return bad(GTO_ERR_INVALID_ARG, "frames must list parents before children");
    if (jt != GTO_JOINT_FIXED && jt != GTO_JOINT_REVOLUTE && jt != GTO_JOINT_PRISMATIC) return bad(GTO_ERR_UNSUPPORTED, "joint type not supported (optas/models.py:865-866)");
    if (jt != GTO_JOINT_FIXED && (d->q_index[i] < 0 || d->q_index[i] >= d->ndof)) return bad(GTO_ERR_INVALID_ARG, "q_index out of range for an actuated joint");
    if (jt != GTO_JOINT_FIXED && !(norm3(d->axis + 3 * i) > 0)) return bad(GTO_ERR_INVALID_ARG, "zero joint axis");
  }
  for (int l = 0; l < d->n_links; ++l)
    if (d->link_frame[l] < 0 || d->link_frame[l] >= d->n_frames) return bad(GTO_ERR_INVALID_ARG, "link_frame out of range");
  for (int l = 0; l < d->n_links; ++l) {
    if (carries_link[d->link_frame[l]]) return bad(GTO_ERR_INVALID_ARG, "two collision links on one frame");
    carries_link[d->link_frame[l]] = true;
  }
  for (int i = 0; i < d->n_points; ++i)
    if (d->point_link[i] < 0 || d->point_link[i] >= d->n_links) return bad(GTO_ERR_INVALID_ARG, "point_link out of range");
  return GTO_OK;
}

// Joint and frame tables.  Clears rb, then fills the counts, frame_ee / frame_gripper, opt_index, opt_of_dof, lower, upper,
// parent, joint_type, q_index, origin, axis_unit, opt_of_frame, frame_anc, fk_rounds, link_frame, link_anc, vis_origin,
// entry_links, link_of_frame and frame_free_mask (n_chunks is fill_chunks').  Reads the descriptor only.
inline void fill_frames_and_links(const gto_robot_desc* d, RobotDev& rb) {
  std::memset(&rb, 0, sizeof rb);
  rb.n_frames = d->n_frames;
  rb.ndof = d->ndof;
  rb.n_opt = d->n_opt;
  rb.n_links = d->n_links;
  rb.n_points = d->n_points;
  rb.n_gripper_points = d->n_gripper_points;
  rb.frame_ee = d->frame_ee;
  rb.frame_gripper = d->frame_gripper;
  for (int i = 0; i < GTO_MAX_DOF; ++i) rb.opt_of_dof[i] = -1;
  for (int j = 0; j < d->n_opt; ++j) {
    rb.opt_index[j] = d->opt_index[j];
    rb.opt_of_dof[d->opt_index[j]] = j;
    rb.lower[j] = d->lower[j];
    rb.upper[j] = d->upper[j];
  }
  for (int i = 0; i < d->n_frames; ++i) {
    const int p = d->parent[i], jt = d->joint_type[i];
    rb.parent[i] = p;
    rb.joint_type[i] = jt;
    rb.q_index[i] = (jt == GTO_JOINT_FIXED) ? -1 : d->q_index[i];
    double R[9];
    rpy2r(d->origin_rpy + 3 * i, R);
    rt2aff(R, d->origin_xyz + 3 * i, rb.origin[i]);
    const double* ax = d->axis + 3 * i;
    const double nrm = norm3(ax);
    for (int k = 0; k < 3; ++k) rb.axis_unit[i][k] = (nrm > 0) ? ax[k] / nrm : 0.0;
    rb.opt_of_frame[i] = -1;
    uint32_t anc = (p >= 0) ? rb.frame_anc[p] : 0u;
    if (rb.q_index[i] >= 0)
      for (int j = 0; j < d->n_opt; ++j)
        if (d->opt_index[j] == rb.q_index[i]) {
          rb.opt_of_frame[i] = j;
          anc |= 1u << j;
        }
    rb.frame_anc[i] = anc;
  }
  rb.fk_rounds = fk_rounds(rb.parent, d->n_frames);
  for (int l = 0; l < d->n_links; ++l) {
    const int f = d->link_frame[l];
    rb.link_frame[l] = f;
    rb.link_anc[l] = rb.frame_anc[f];
    double R[9];
    rpy2r(d->visual_rpy + 3 * l, R);
    rt2aff(R, d->visual_xyz + 3 * l, rb.vis_origin[l]);
  }
  for (int v = 0; v < 2; ++v) {
    const int NPv = v ? 16 : 8;
    for (int e = 0; e < NPv * NPv + NPv; ++e) {
      const int i = e < NPv * NPv ? e / NPv : e - NPv * NPv, j = e < NPv * NPv ? e % NPv : i;
      uint32_t m = 0u;
      if (i < d->n_opt && j < d->n_opt)
        for (int l = 0; l < d->n_links; ++l) m |= (((rb.link_anc[l] >> i) & (rb.link_anc[l] >> j) & 1u) << l);
      rb.entry_links[v][e] = m;
    }
  }
  for (int i = 0; i < d->n_frames; ++i) rb.link_of_frame[i] = -1;
  for (int l = 0; l < d->n_links; ++l) rb.link_of_frame[rb.link_frame[l]] = l;
  rb.frame_free_mask = 0u;
  for (int i = 0; i < d->n_frames; ++i)
    if (rb.opt_of_frame[i] < 0) rb.frame_free_mask |= 1u << i;
}

// The step kernel's serial walk over the tree (gto_kernels.h, prebroad_tail).  Fills xst_slot, n_xst, pb_ctl, pb_par,
// pb_parf, pb_npar, pb_ft and pb_eps.  Reads the frame and link tables of fill_frames_and_links, and the descriptor's
// origins, visual origins and points for the extent behind pb_eps.
inline void fill_step_walk(const gto_robot_desc* d, RobotDev& rb) {
  rb.n_xst = 0;
  for (int i = 0; i < d->n_frames; ++i) rb.xst_slot[i] = -1;
  for (int i = 0; i < d->n_frames; ++i) {  // a frame that a later, non-adjacent child needs is parked
    const int p = rb.parent[i];
    if (p >= 0 && p != i - 1 && rb.xst_slot[p] < 0) rb.xst_slot[p] = rb.n_xst++;
  }
  for (int i = 0; i < d->n_frames; ++i) {  // control words
    const int p = rb.parent[i], l = rb.link_of_frame[i];
    const int src = p < 0 ? 0 : (p == i - 1 ? 1 : 2 + rb.xst_slot[p]);
    const bool moving_link = l >= 0 && (rb.frame_anc[rb.link_frame[l]] != 0u);
    rb.pb_ctl[i] = (src & 7) | (((rb.xst_slot[i] + 1) & 7) << 4) | ((moving_link ? 1 : 0) << 8);
    rb.pb_par[i] = -1;
    if (rb.joint_type[i] != GTO_JOINT_FIXED && rb.opt_of_frame[i] < 0) rb.pb_par[i] = rb.pb_npar, rb.pb_parf[rb.pb_npar++] = i;
  }
  for (int i = 0; i < d->n_frames; ++i) {  // the frame table the tail copies into its LDS as it is
    for (int e = 0; e < 12; ++e) rb.pb_ft[i][e] = (float)rb.origin[i][e];
    for (int e = 0; e < 3; ++e) rb.pb_ft[i][12 + e] = (float)rb.axis_unit[i][e];
    const int32_t w = rb.joint_type[i] | ((rb.opt_of_frame[i] + 1) << 4) | ((rb.pb_par[i] + 1) << 9);
    std::memcpy(&rb.pb_ft[i][15], &w, sizeof w);
  }
  double D = 0.0, maxp = 0.0;  // no frame origin or surface point is further than D from any other
  for (int i = 0; i < d->n_frames; ++i) {
    D += norm3(d->origin_xyz + 3 * i);
    if (rb.joint_type[i] == GTO_JOINT_PRISMATIC) {
      const int j = rb.opt_of_frame[i];
      D += j >= 0 ? std::max(std::fabs(rb.lower[j]), std::fabs(rb.upper[j])) : 2.0;
    }
  }
  for (int l = 0; l < d->n_links; ++l) maxp = std::max(maxp, norm3(d->visual_xyz + 3 * l));
  double maxr = 0.0;
  for (int i = 0; i < d->n_points; ++i) maxr = std::max(maxr, norm3(d->points + 3 * i));
  D += maxp + maxr;
  rb.pb_eps = 128.0 * d->n_frames * 5.9604644775390625e-08 * D;  // four times the first-order bound 32 F 2^-24 D (gto_kernels.h, PbLayout)
}

// A kinematic tree as write_fk_table reads it: per frame the origin affine, unit axis, joint type, parent and
// optimised-joint slot; per link its frame and visual origin.
struct FkTree {
  int nf;
  const double (*origin)[12];
  const double (*axis_unit)[3];
  const int32_t *joint_type, *parent, *opt_of_frame, *link_frame;
  const double (*vis_origin)[12];
};

// One operand table of fk_mfma_tree (gto_device.h, RobotDev::fk_tab) for a tree of tr.nf frames, L links and n optimised
// joints.  Fills tab and opt_frame_out (the frame of each optimised joint); reads tr only.
inline void write_fk_table(const FkTree& tr, int L, int n, double* tab, int32_t* opt_frame_out) {
  auto hom = [](const double* aff, int a, int c) { return a < 3 ? aff[4 * a + c] : (c == 3 ? 1.0 : 0.0); };
  const int nf = tr.nf;
  std::memset(tab, 0, sizeof RobotDev::fk_tab);
  for (int i = 0; i < nf; ++i) {
    const double* u = tr.axis_unit[i];
    const double K[3][3] = {{0, -u[2], u[1]}, {u[2], 0, -u[0]}, {-u[1], u[0], 0}};
    double* ft = tab + GTO_FK_STRIDE * i;
    for (int a = 0; a < 4; ++a)
      for (int c = 0; c < 4; ++c) {
        const int e = (4 * a + c) ^ (5 * (i & 3));  // bank placement of the frame's entries (gto_device.h, fkx)
        const double uu = (a < 3 && c < 3) ? u[a] * u[c] : 0.0;
        const double dl = (a == c && a < 3) ? 1.0 : 0.0, hh = (a == 3 && c == 3) ? 1.0 : 0.0;
        ft[e] = hom(tr.origin[i], c, a);  // transposed: a row-pattern read gives the B operand O^T (gto_device.h, fkx)
        ft[16 + e] = hh + uu;  // M = c0 + cos c1 + sin K
        ft[32 + e] = dl - uu;
        if (tr.joint_type[i] == GTO_JOINT_PRISMATIC) ft[48 + e] = (a < 3 && c == 3) ? u[a] : 0.0;
        else ft[48 + e] = (a < 3 && c < 3) ? K[a][c] : 0.0;
      }
    if (tr.opt_of_frame[i] >= 0) {
      const int j = tr.opt_of_frame[i];
      opt_frame_out[j] = i;
      double* tu = tab + GTO_FK_STRIDE * nf + 16 * L;
      for (int a = 0; a < 3; ++a) tu[fkx(j, 4 * a)] = u[a];
      tu[fkx(j, 4 * 3 + 1)] = 1.0;
    }
  }
  for (int l = 0; l < L; ++l)
    for (int a = 0; a < 4; ++a)
      for (int c = 0; c < 4; ++c) tab[GTO_FK_STRIDE * nf + fkx(l, 4 * a + c)] = hom(tr.vis_origin[l], a, c);
  double* tI = tab + GTO_FK_STRIDE * nf + 16 * L + 16 * n;
  for (int l = 0; l < L; ++l) tI[l] = tr.link_frame[l];
  for (int j = 0; j < n; ++j) {
    tI[L + j] = opt_frame_out[j];
    tI[L + n + j] = tr.joint_type[opt_frame_out[j]] == GTO_JOINT_PRISMATIC ? 1.0 : 0.0;
  }
  for (int i = 0; i < nf; ++i) tI[L + 2 * n + i] = tr.parent[i];
}

// The compact tree of the obstacle kernel (gto_device.h, RobotDev::fk_tab_c), in the form write_fk_table reads.
struct CompactTree {
  int nc = 0;
  double origin[GTO_MAX_FRAMES][12], axis_unit[GTO_MAX_FRAMES][3], vis_origin[GTO_MAX_LINKS][12];
  int32_t parent[GTO_MAX_FRAMES], opt_of_frame[GTO_MAX_FRAMES], link_frame[GTO_MAX_LINKS];
};

// Folds the frames with fixed joints into the origins of the moving frames below them and into the visual origins of
// their links, and appends a frame that is the world when a link hangs on fixed frames only (or no frame moves).  Fills ct
// and rb.cf_orig, rb.cf_type; reads the frame and link tables of fill_frames_and_links.
inline void fold_fixed_frames(RobotDev& rb, CompactTree& ct) {
  const int F = rb.n_frames, L = rb.n_links;
  int cf[GTO_MAX_FRAMES], nc = 0;
  for (int f = 0; f < F; ++f) cf[f] = rb.joint_type[f] != GTO_JOINT_FIXED ? nc++ : -1;
  for (int f = 0; f < F; ++f) {
    if (cf[f] < 0) continue;
    const int k = cf[f];
    double A[12];
    std::memcpy(A, rb.origin[f], sizeof A);
    int p = rb.parent[f];
    for (; p >= 0 && rb.joint_type[p] == GTO_JOINT_FIXED; p = rb.parent[p]) aff_mul(rb.origin[p], A, A);
    std::memcpy(ct.origin[k], A, sizeof A);
    std::memcpy(ct.axis_unit[k], rb.axis_unit[f], sizeof ct.axis_unit[k]);
    ct.parent[k] = p >= 0 ? cf[p] : -1;
    ct.opt_of_frame[k] = rb.opt_of_frame[f];
    rb.cf_orig[k] = f;
    rb.cf_type[k] = rb.joint_type[f];
  }
  bool need_world = false;
  for (int l = 0; l < L; ++l) {
    double V[12];
    std::memcpy(V, rb.vis_origin[l], sizeof V);
    int g = rb.link_frame[l];
    for (; g >= 0 && rb.joint_type[g] == GTO_JOINT_FIXED; g = rb.parent[g]) aff_mul(rb.origin[g], V, V);
    std::memcpy(ct.vis_origin[l], V, sizeof V);
    ct.link_frame[l] = g >= 0 ? cf[g] : -2;
    need_world = need_world || g < 0;
  }
  if (need_world || nc == 0) {  // links that hang on fixed frames only: a frame that is the world
    const int k = nc++;
    const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(ct.origin[k], I12, sizeof I12);
    ct.axis_unit[k][0] = ct.axis_unit[k][1] = ct.axis_unit[k][2] = 0.0;
    ct.parent[k] = -1, ct.opt_of_frame[k] = -1;
    rb.cf_orig[k] = -1;
    rb.cf_type[k] = GTO_JOINT_FIXED;
    for (int l = 0; l < L; ++l)
      if (ct.link_frame[l] == -2) ct.link_frame[l] = k;
  }
  ct.nc = nc;
}

// Operand tables of fk_mfma_tree: the full tree, and the compact tree of the obstacle kernel.  Fills fk_tab, opt_frame,
// fk_tab_c, n_cframes, fk_rounds_c (and cf_orig, cf_type through fold_fixed_frames); reads the frame and link tables.
inline void fill_fk_tables(RobotDev& rb) {
  static_assert(sizeof rb.fk_tab == sizeof rb.fk_tab_c, "one layout for both tables");
  write_fk_table({rb.n_frames, rb.origin, rb.axis_unit, rb.joint_type, rb.parent, rb.opt_of_frame, rb.link_frame, rb.vis_origin},
                 rb.n_links, rb.n_opt, rb.fk_tab, rb.opt_frame);
  CompactTree ct;
  int32_t opt_frame_c[GTO_MAX_OPT];
  fold_fixed_frames(rb, ct);
  write_fk_table({ct.nc, ct.origin, ct.axis_unit, rb.cf_type, ct.parent, ct.opt_of_frame, ct.link_frame, ct.vis_origin},
                 rb.n_links, rb.n_opt, rb.fk_tab_c, opt_frame_c);
  rb.n_cframes = ct.nc;
  rb.fk_rounds_c = fk_rounds(ct.parent, ct.nc);
}

// Moments of the gripper point cloud: fills grip_count, grip_mu, grip_M (cleared by fill_frames_and_links); reads the
// descriptor's gripper points.
inline void fill_gripper_moments(const gto_robot_desc* d, RobotDev& rb) {
  rb.grip_count = (double)d->n_gripper_points;
  for (int k = 0; k < d->n_gripper_points; ++k) {
    const double* p = d->gripper_points + 3 * k;
    for (int r = 0; r < 3; ++r) {
      rb.grip_mu[r] += p[r];
      for (int c = 0; c < 3; ++c) rb.grip_M[3 * r + c] += p[r] * p[c];
    }
  }
}

// reach[j]: conservative bound on the displacement of any surface point per unit motion of joint j:
// sum of the origin offsets along the chain below the joint (+ travel of prismatic joints below it)
// + visual-origin offset + farthest surface point of the link, maximised over the links it moves.
// Fills reach and reach_link; reads opt_of_frame, joint_type, lower, upper and the descriptor's tree, origins and points.
inline void fill_reach(const gto_robot_desc* d, RobotDev& rb) {
  std::vector<double> maxpt(d->n_links, 0.0);
  for (int i = 0; i < d->n_points; ++i) maxpt[d->point_link[i]] = std::max(maxpt[d->point_link[i]], norm3(d->points + 3 * i));
  for (int j = 0; j < d->n_opt; ++j) rb.reach[j] = 0.0;
  for (int l = 0; l < GTO_MAX_LINKS; ++l)
    for (int j = 0; j < GTO_MAX_OPT; ++j) rb.reach_link[l][j] = 0.0;
  bool ok = true;
  for (int l = 0; l < d->n_links; ++l) {
    double below = norm3(d->visual_xyz + 3 * l) + maxpt[l];  // offsets below the current frame
    for (int f = d->link_frame[l]; f >= 0; f = d->parent[f]) {
      const int j = rb.opt_of_frame[f];
      if (j >= 0) rb.reach[j] = std::max(rb.reach[j], rb.joint_type[f] == GTO_JOINT_PRISMATIC ? 1.0 : below);
      if (j >= 0) rb.reach_link[l][j] = rb.joint_type[f] == GTO_JOINT_PRISMATIC ? 1.0 : below;
      if (rb.joint_type[f] == GTO_JOINT_PRISMATIC) {
        // travel of this joint moves everything below it further from the joints above
        double travel = 1e9;
        if (j >= 0) travel = std::max(std::fabs(rb.lower[j]), std::fabs(rb.upper[j]));
        else travel = 2.0;  // parameter prismatic joints (torso lift, fingers): generous constant
        if (!(travel < 1e3)) ok = false;
        below += travel;
      }
      below += norm3(d->origin_xyz + 3 * f);
    }
  }
  if (!ok) for (int j = 0; j < d->n_opt; ++j) rb.reach[j] = -1.0;
  if (!ok)
    for (int l = 0; l < GTO_MAX_LINKS; ++l)
      for (int j = 0; j < GTO_MAX_OPT; ++j) rb.reach_link[l][j] = -1.0;
}

// Morton (Z-order) code of every surface point in the bounding box of its link's points, 10 bits per axis, isotropic cells.
inline std::vector<uint32_t> morton_codes(const gto_robot_desc* d) {
  const int P = d->n_points;
  std::vector<uint32_t> morton(P, 0);
  std::vector<double> lo(3 * d->n_links, 1e300), hi(3 * d->n_links, -1e300);
  for (int i = 0; i < P; ++i)
    for (int a = 0; a < 3; ++a) {
      lo[3 * d->point_link[i] + a] = std::min(lo[3 * d->point_link[i] + a], d->points[3 * i + a]);
      hi[3 * d->point_link[i] + a] = std::max(hi[3 * d->point_link[i] + a], d->points[3 * i + a]);
    }
  auto spread = [](uint32_t v) {  // 10 bits -> every third bit
    v &= 0x3ff;
    v = (v | (v << 16)) & 0x30000ff;
    v = (v | (v << 8)) & 0x300f00f;
    v = (v | (v << 4)) & 0x30c30c3;
    v = (v | (v << 2)) & 0x9249249;
    return v;
  };
  for (int i = 0; i < P; ++i) {
    const int l = d->point_link[i];
    double ext = 1e-12;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, hi[3 * l + a] - lo[3 * l + a]);
    uint32_t code = 0;
    for (int a = 0; a < 3; ++a) {
      double u = (d->points[3 * i + a] - lo[3 * l + a]) / ext;  // isotropic cells
      uint32_t q = (uint32_t)std::min(1023.0, std::max(0.0, u * 1023.0));
      code |= spread(q) << a;
    }
    morton[i] = code;
  }
  return morton;
}

// Point order: sorted by link (stable), and inside a link along a Morton curve of the link-local coordinates, so that the
// 64 lanes of a chunk (and consecutive chunks) gather from neighbouring voxels/cache lines.  Fills perm, px, py, pz, plink;
// reads the descriptor's points and point_link.
inline void sort_points(const gto_robot_desc* d, RobotTables& t) {
  const int P = d->n_points;
  const std::vector<uint32_t> morton = morton_codes(d);
  t.perm.resize(P);
  for (int i = 0; i < P; ++i) t.perm[i] = i;
  std::stable_sort(t.perm.begin(), t.perm.end(), [&](int a, int b) {
    if (d->point_link[a] != d->point_link[b]) return d->point_link[a] < d->point_link[b];
    return morton[a] < morton[b];
  });
  t.px.resize(P), t.py.resize(P), t.pz.resize(P), t.plink.resize(P);
  for (int i = 0; i < P; ++i) {
    t.px[i] = d->points[3 * t.perm[i]];
    t.py[i] = d->points[3 * t.perm[i] + 1];
    t.pz[i] = d->points[3 * t.perm[i] + 2];
    t.plink[i] = d->point_link[t.perm[i]];
  }
}

// Bounding sphere of the sorted points [i0, i1): centre c = their mean, radius r = the farthest of them (+ a hair).
inline void bounding_sphere(const RobotTables& t, int i0, int i1, double c[3], double& r) {
  double cx = 0, cy = 0, cz = 0, r2 = 0;
  for (int k = i0; k < i1; ++k) cx += t.px[k], cy += t.py[k], cz += t.pz[k];
  cx /= (i1 - i0), cy /= (i1 - i0), cz /= (i1 - i0);
  for (int k = i0; k < i1; ++k) {
    const double dx = t.px[k] - cx, dy = t.py[k] - cy, dz = t.pz[k] - cz;
    r2 = std::max(r2, dx * dx + dy * dy + dz * dz);
  }
  c[0] = cx, c[1] = cy, c[2] = cz;
  r = std::sqrt(r2) * (1.0 + 1e-9) + 1e-12;
}

// Chunks and the step kernel's merged spheres.  Fills chunks, rb.n_chunks, pbchunks, pb_C; reads the sorted points, and
// link_anc, link_frame, vis_origin.  Refuses a robot with more than GTO_MAX_ACTIVE chunks.
inline int fill_chunks(int pb_merge, RobotTables& t, std::string& why) {
  RobotDev& rb = t.rb;
  const int P = (int)t.plink.size();
  t.chunks.clear(), t.pbchunks.clear();
  for (int i = 0; i < P;) {  // runs of <= 64 points of one link
    const int l = t.plink[i];
    int j = i;
    while (j < P && t.plink[j] == l && j - i < GTO_WAVE) ++j;
    double c[3], r;
    bounding_sphere(t, i, j, c, r);
    t.chunks.push_back(Chunk{l, i, j - i, rb.link_anc[l] == 0u ? 1 : 0, c[0], c[1], c[2], r});
    i = j;
  }
  rb.n_chunks = (int)t.chunks.size();
  // The step kernel's spheres: runs of pb_merge consecutive chunks of a moving link under one sphere (the chunks follow a
  // Morton curve, so a run is a compact patch).  Coarser than the obstacle kernel's own test, which stays per chunk and
  // exact: a sphere more lists a group more, never one less.  Centre in the coordinates of the link's FRAME (visual origin
  // applied here, in double: the tail's walk stops at the frames).
  for (size_t ci = 0; ci < t.chunks.size();) {
    const Chunk& first = t.chunks[ci];
    if (first.pad) { ++ci; continue; }
    size_t cj = ci;
    int i1 = first.start;
    while (cj < t.chunks.size() && cj - ci < (size_t)pb_merge && !t.chunks[cj].pad && t.chunks[cj].link == first.link) i1 = t.chunks[cj].start + t.chunks[cj].count, ++cj;
    double c[3], r;
    bounding_sphere(t, first.start, i1, c, r);
    const double* V = rb.vis_origin[first.link];
    t.pbchunks.push_back(PbChunk{V[0] * c[0] + V[1] * c[1] + V[2] * c[2] + V[3], V[4] * c[0] + V[5] * c[1] + V[6] * c[2] + V[7],
                                 V[8] * c[0] + V[9] * c[1] + V[10] * c[2] + V[11], r, rb.link_frame[first.link], 0});
    ci = cj;
  }
  t.pb_C = (int)t.pbchunks.size();
  if (t.pbchunks.empty()) t.pbchunks.push_back(PbChunk{0, 0, 0, 0, 0, 0});  // (a robot none of whose links moves: the table is never read)
  if (rb.n_chunks > GTO_MAX_ACTIVE) {
    why = "too many surface points (max 16384, in at most 256 runs of up to 64 points of one link)";
    return GTO_ERR_UNSUPPORTED;
  }
  return GTO_OK;
}

// Every refusal of gto_set_link_inertials, in the order mass, centre of mass, inertia, gravity: finite masses >= 0; for a
// frame with mass > 0 a finite centre of mass and a finite inertia that is positive semidefinite (Sylvester's principal
// minors, each allowed a relative 1e-12 of the tensor's scale below zero); a finite gravity.  Reads the arrays only
// (gravity may be null) and fills nothing.
inline int check_inertials(int n_frames, const double* mass, const double* com, const double* inertia, const double* gravity,
                           std::string& why) {
  auto bad = [&](const char* msg) {
    why = msg;
    return GTO_ERR_INVALID_ARG;
  };
  for (int f = 0; f < n_frames; ++f)
    if (!(mass[f] >= 0) || !std::isfinite(mass[f])) return bad("link mass must be >= 0 and finite");
  for (int f = 0; f < n_frames; ++f) {
    if (!(mass[f] > 0)) continue;
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(com[3 * f + k])) return bad("non-finite centre of mass");
    const double* I = inertia + 6 * f;
    double scale = 0.0;
    for (int k = 0; k < 6; ++k) {
      if (!std::isfinite(I[k])) return bad("non-finite link inertia");
      scale = std::max(scale, std::fabs(I[k]));
    }
    const double xx = I[0], xy = I[1], xz = I[2], yy = I[3], yz = I[4], zz = I[5];
    const double t1 = 1e-12 * scale, t2 = t1 * scale, t3 = t2 * scale;
    const double m_xy = xx * yy - xy * xy, m_xz = xx * zz - xz * xz, m_yz = yy * zz - yz * yz;
    const double det = xx * m_yz - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
    if (xx < -t1 || yy < -t1 || zz < -t1 || m_xy < -t2 || m_xz < -t2 || m_yz < -t2 || det < -t3)
      return bad("link inertia must be symmetric positive semidefinite");
  }
  if (gravity)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(gravity[k])) return bad("non-finite gravity");
  return GTO_OK;
}

// The inertial table rt_rnea reads (gto_dynamics.h).  Clears dyn, then fills mass, com and inertia of the frames with mass
// (the other entries of a massless frame are ignored: they stay zero) and gravity (null: (0, 0, -9.81)).  Reads arrays that
// check_inertials has passed.
inline void fill_inertials(int n_frames, const double* mass, const double* com, const double* inertia, const double* gravity,
                           DynDev& dyn) {
  std::memset(&dyn, 0, sizeof dyn);
  for (int f = 0; f < n_frames; ++f) {
    if (!(mass[f] > 0)) continue;
    dyn.mass[f] = mass[f];
    for (int k = 0; k < 3; ++k) dyn.com[f][k] = com[3 * f + k];
    for (int k = 0; k < 6; ++k) dyn.inertia[f][k] = inertia[6 * f + k];
  }
  dyn.gravity[2] = -9.81;
  if (gravity)
    for (int k = 0; k < 3; ++k) dyn.gravity[k] = gravity[k];
}

}  // namespace gto_robot

// Validates the descriptor and builds its tables, for step-kernel spheres of up to pb_merge >= 1 chunks.  GTO_OK, or an
// error code with its message in `why` (t is then unspecified).  Safe on any descriptor whose arrays have the lengths its
// counts state.
inline int build_robot(const gto_robot_desc* d, int pb_merge, RobotTables& t, std::string& why) {
  using namespace gto_robot;
  if (int rc = check_descriptor(d, why)) return rc;
  fill_frames_and_links(d, t.rb);
  fill_step_walk(d, t.rb);
  fill_fk_tables(t.rb);
  fill_gripper_moments(d, t.rb);
  fill_reach(d, t.rb);
  sort_points(d, t);
  return fill_chunks(pb_merge, t, why);
}
