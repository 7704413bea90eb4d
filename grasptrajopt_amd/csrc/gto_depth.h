// gto_depth.h — cost field from a depth image (gto_depth_sdf_cost, gto_scene_from_depth: include/gto_solver.h).  The
// reference's DepthPointCloud (mesh_to_sdf/depth_point_cloud.py:9-141): back-projection of the valid pixels into the world,
// the distance from every query to the nearest point of that cloud, its sign by the depth-buffer visibility test, the cost
// map; and the voxel centres of the workspace grid (gto/gto_models.py:155-171) for the per-object perception steps of
// examples/pybullet_gto_planning.py:176-190.  FP64 with FMA contraction off: the reference's values bit for bit.
//
//   k_depth_backproject  one lane per pixel: world point, or a point at infinity for an invalid or masked pixel
//   k_depth_sdf          one lane per query: exhaustive nearest-neighbour search, the cloud streamed through LDS (the
//                        reference construction; GTO_DEPTH_BRUTE, and images beyond the hierarchy's 1024 x 1024 tiles)
//   k_grid_queries       one lane per voxel: the centres of a grid given by its three axes, C order
//   k_bvh_leaves         one lane per tile of 8 x 4 pixels: the leaf boxes of the bounding-box hierarchy, Morton order
//   k_bvh_up             one workgroup: the inner boxes, level by level up to the root (= the cloud's bounding box)
//   k_query_keys         one lane per query: 30-bit Morton key of its position (the host sorts them with hipCUB)
//   k_depth_sdf_bvh      one wave per 64 queries in key order: the same distances by a packet walk of the hierarchy
// Below the kernels: their launches (build_cloud, search_tree, search_exhaustive) and the structs these take, for the two
// entry points in gto_api.hip.  wave_sync_lds is gto_kernels.h's.
#pragma once
#include "gto_device.h"
#include "gto_kernels.h"

// ------------------------------------------------------------------------------------------------
// Cost field from a depth image (mesh_to_sdf/depth_point_cloud.py:9-141): the producer
// of the (F,) cost arrays.  Arithmetic follows the reference's order with FMA contraction switched off
// in these two kernels: the reference values are reproduced bit for bit (tests/golden/depth_cost.npz);
// where the reference's BLAS products could differ in the last bit on another machine, the CPU
// restatement (oracle, -ffp-contract=off) is matched exactly.
// backproject (:32-52) + world transform (:21-23); invalid pixels become points at infinity
__global__ void k_depth_backproject(const float* __restrict__ depth, int H, int W, const double* __restrict__ Kinv,
                                    const double* __restrict__ cam, const uint8_t* __restrict__ target_mask,
                                    double threshold, double* __restrict__ px, double* __restrict__ py,
                                    double* __restrict__ pz, uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)  // plain operators below must stay unfused (HIP's __dmul_rn & co. are no barrier)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const float d = depth[i];
  const bool ok = (d > 0.0f) && ((double)d < threshold) && (!target_mask || target_mask[i] == 0);
  double X[3], P[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double t = (Kinv[3 * r] * (double)x + Kinv[3 * r + 1] * (double)y) + Kinv[3 * r + 2];
    X[r] = (double)d * t;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
    P[r] = ((cam[4 * r] * X[0] + cam[4 * r + 1] * X[1]) + cam[4 * r + 2] * X[2]) + cam[4 * r + 3];
  px[i] = ok ? P[0] : INFINITY;
  py[i] = ok ? P[1] : INFINITY;
  pz[i] = ok ? P[2] : INFINITY;
  valid[i] = ok ? 1 : 0;
}

// get_sdf (:56-61) + is_outside (:126-141) + cost map (:84-89): one query per thread, the cloud streamed
// through LDS in tiles; exact nearest neighbour by exhaustive search in FP64 (the KD-tree of the reference
// returns the same distance), a few ms for 10^5 queries x 3*10^5 points at the FP64 vector rate.
// What follows the nearest-neighbour search of a query (mesh_to_sdf/depth_point_cloud.py:56-141): sign by the depth-buffer
// visibility test, cost map.  best = squared distance to the nearest point of the cloud.
// mesh_to_sdf/depth_point_cloud.py:126-141 is_outside: the query is in front of the surface the depth image saw at its pixel
// (or projects outside the image)
// *pixel: the image index iy * W + ix the query projects to, -1 when it projects outside the image
__device__ __forceinline__ bool depth_is_outside_at(double q0, double q1, double q2, const float* __restrict__ depth, int H, int W,
                                                    const double* __restrict__ K, const double* __restrict__ cam_inv, int* pixel) {
#pragma clang fp contract(off)
  double pc[3], u[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    pc[r] = ((cam_inv[4 * r] * q0 + cam_inv[4 * r + 1] * q1) + cam_inv[4 * r + 2] * q2) + cam_inv[4 * r + 3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    u[r] = (K[3 * r] * pc[0] + K[3 * r + 1] * pc[1]) + K[3 * r + 2] * pc[2];
  const double ux = u[0] / u[2], uy = u[1] / u[2];
  const bool fx = fabs(ux) < 9.0e18, fy = fabs(uy) < 9.0e18;
  const long ix = fx ? (long)ux : LONG_MIN, iy = fy ? (long)uy : LONG_MIN;
  bool outside = true;
  *pixel = -1;
  if (ix >= 0 && iy >= 0 && ix < W && iy < H) {
    outside = pc[2] < (double)depth[iy * W + ix];
    *pixel = (int)(iy * W + ix);
  }
  return outside;
}
__device__ __forceinline__ bool depth_is_outside(double q0, double q1, double q2, const float* __restrict__ depth, int H, int W,
                                                 const double* __restrict__ K, const double* __restrict__ cam_inv) {
  int pixel;
  return depth_is_outside_at(q0, q1, q2, depth, H, W, K, cam_inv, &pixel);
}

// The cost map of mesh_to_sdf/depth_point_cloud.py:84-89 for a signed distance `dist` (negative: inside).  The depth path
// (depth_sdf_finish) and the sampled-mesh path (gto_cloud.h) both end in it.
__device__ __forceinline__ float sdf_cost_map(float dist, bool inside, float epsilon, float w_inside) {
#pragma clang fp contract(off)
  float c = 0.0f;
  if (inside) {
    c = w_inside * (-dist + epsilon / 2.0f);
  } else if (dist > 0.0f && dist < epsilon) {
    const float e = dist - epsilon;
    c = (e * e) / (2.0f * epsilon);
  }
  return c;
}

__device__ __forceinline__ void depth_sdf_finish(bool live, long q, double q0, double q1, double q2, double best,
                                                 const float* __restrict__ depth, int H, int W, const double* __restrict__ K,
                                                 const double* __restrict__ cam_inv, float epsilon, float w_inside,
                                                 float* __restrict__ sdf_out, uint8_t* __restrict__ inside_out,
                                                 float* __restrict__ cost_out) {
#pragma clang fp contract(off)
  if (!live) return;
  float dist = (float)sqrt(best);
  double pc[3], u[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    pc[r] = ((cam_inv[4 * r] * q0 + cam_inv[4 * r + 1] * q1) + cam_inv[4 * r + 2] * q2) + cam_inv[4 * r + 3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    u[r] = (K[3 * r] * pc[0] + K[3 * r + 1] * pc[1]) + K[3 * r + 2] * pc[2];
  const double ux = u[0] / u[2], uy = u[1] / u[2];
  // .astype(int): truncation toward zero; non-finite / out-of-range values become INT64_MIN in NumPy
  const bool fx = fabs(ux) < 9.0e18, fy = fabs(uy) < 9.0e18;
  const long ix = fx ? (long)ux : LONG_MIN, iy = fy ? (long)uy : LONG_MIN;
  bool outside = true;
  if (ix >= 0 && iy >= 0 && ix < W && iy < H) outside = pc[2] < (double)depth[iy * W + ix];
  if (!outside) dist = -dist;
  const float c = sdf_cost_map(dist, !outside, epsilon, w_inside);
  if (sdf_out) sdf_out[q] = dist;
  if (inside_out) inside_out[q] = outside ? 0 : 1;
  if (cost_out) cost_out[q] = c;
}

__global__ __launch_bounds__(256) void k_depth_sdf(const double* __restrict__ px, const double* __restrict__ py,
                                                   const double* __restrict__ pz, int N, const float* __restrict__ depth,
                                                   int H, int W, const double* __restrict__ K,
                                                   const double* __restrict__ cam_inv, const double* __restrict__ query,
                                                   long nq, float epsilon, float w_inside, float* __restrict__ sdf_out,
                                                   uint8_t* __restrict__ inside_out, float* __restrict__ cost_out) {
#pragma clang fp contract(off)  // see k_depth_backproject
  __shared__ double sx[256], sy[256], sz[256];
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = q < nq;
  const double q0 = live ? query[3 * q] : 0.0, q1 = live ? query[3 * q + 1] : 0.0, q2 = live ? query[3 * q + 2] : 0.0;
  double best = INFINITY;
  for (int base = 0; base < N; base += 256) {
    const int j = base + threadIdx.x;
    sx[threadIdx.x] = j < N ? px[j] : INFINITY;
    sy[threadIdx.x] = j < N ? py[j] : INFINITY;
    sz[threadIdx.x] = j < N ? pz[j] : INFINITY;
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 256; ++k) {
      const double dx = q0 - sx[k], dy = q1 - sy[k], dz = q2 - sz[k];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      best = fmin(best, d2);  // NaN (inf - inf never occurs: queries are finite) is ignored by fmin
    }
    __syncthreads();
  }
  depth_sdf_finish(live, q, q0, q1, q2, best, depth, H, W, K, cam_inv, epsilon, w_inside, sdf_out, inside_out, cost_out);
}

// Voxel centres of a grid given by its three axes (axes = xs | ys | zs), C order, x slowest: the workspace_points of
// gto/gto_models.py:159-165 (numpy.meshgrid(..., indexing="ij") reshaped), generated where they are used
__global__ void k_grid_queries(const double* __restrict__ axes, int nx, int ny, int nz, double* __restrict__ query) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (long)nx * ny * nz) return;
  const int iz = (int)(q % nz), iy = (int)((q / nz) % ny), ix = (int)(q / ((long)nz * ny));
  query[3 * q] = axes[ix];
  query[3 * q + 1] = axes[nx + iy];
  query[3 * q + 2] = axes[nx + ny + iz];
}

// ---- the same nearest-neighbour distances without the exhaustive search.  The cloud comes from a depth image, so
// pixels that are close in the image are (mostly) close in space: tiles of 8 x 4 pixels are the leaves of a bounding-box
// hierarchy, the tiles taken in Morton order of their (column, row) so that every node of the implicit complete binary
// tree (heap indexing, P x P leaf slots, P a power of two) covers a rectangle of the image.  No sorting, no copy of
// the points.  A query walks the tree nearer child first and skips every box that cannot hold a closer point.  The
// skip test is exact in floating point: for a point p of a box, |q - p| >= (distance of q to the box) holds per axis
// also after rounding (subtraction, product and sum are monotone), and the box distance is summed in the same order
// as the point distance, so the minimum over the visited points is the minimum over all points, bit for bit.
#define GTO_BVH_TILE_W 8
#define GTO_BVH_TILE_H 4
__host__ __device__ inline unsigned bvh_compact1by1(unsigned v) {
  v &= 0x55555555u;
  v = (v | (v >> 1)) & 0x33333333u;
  v = (v | (v >> 2)) & 0x0f0f0f0fu;
  v = (v | (v >> 4)) & 0x00ff00ffu;
  v = (v | (v >> 8)) & 0x0000ffffu;
  return v;
}
// boxes: [node][6] = lo x, y, z, hi x, y, z; an empty box is (+inf, -inf): its distance from anything is +inf
__global__ void k_bvh_leaves(const double* __restrict__ px, const double* __restrict__ py, const double* __restrict__ pz, int H,
                             int W, int P, double* __restrict__ boxes) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= P * P) return;
  const int cx = (int)bvh_compact1by1((unsigned)s), cy = (int)bvh_compact1by1((unsigned)s >> 1);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int r = 0; r < GTO_BVH_TILE_H; ++r)
    for (int c = 0; c < GTO_BVH_TILE_W; ++c) {
      const int y = cy * GTO_BVH_TILE_H + r, x = cx * GTO_BVH_TILE_W + c;
      if (y >= H || x >= W) continue;
      const size_t j = (size_t)y * W + x;
      const double v[3] = {px[j], py[j], pz[j]};
      if (!(v[0] < INFINITY)) continue;  // invalid pixel (point at infinity)
      for (int k = 0; k < 3; ++k) {
        lo[k] = fmin(lo[k], v[k]);
        hi[k] = fmax(hi[k], v[k]);
      }
    }
  double* b = boxes + (size_t)(P * P - 1 + s) * 6;
  for (int k = 0; k < 3; ++k) b[k] = lo[k], b[3 + k] = hi[k];
}
// inner nodes, level by level from the leaves up (one workgroup: twice the leaf slots are a few ten thousand nodes).
// n_leaves: the leaf slots, a power of two (P x P for an image; gto_cloud.h builds its hierarchy over sorted samples with it)
__global__ __launch_bounds__(1024) void k_bvh_up(int n_leaves, double* __restrict__ boxes) {
  for (int first = (n_leaves - 1) / 2, count = n_leaves / 2; count >= 1; first = (first - 1) / 2, count >>= 1) {
    for (int i = threadIdx.x; i < count; i += 1024) {
      const int n = first + i;
      const double* a = boxes + (size_t)(2 * n + 1) * 6;
      const double* c = boxes + (size_t)(2 * n + 2) * 6;
      double* o = boxes + (size_t)n * 6;
      for (int k = 0; k < 3; ++k) o[k] = fmin(a[k], c[k]), o[3 + k] = fmax(a[3 + k], c[3 + k]);
    }
    __threadfence_block();
    __syncthreads();
    if (count == 1) break;
  }
}
__device__ __forceinline__ double bvh_box_d2(const double* __restrict__ b, double q0, double q1, double q2) {
#pragma clang fp contract(off)
  const double ex = fmax(fmax(b[0] - q0, q0 - b[3]), 0.0), ey = fmax(fmax(b[1] - q1, q1 - b[4]), 0.0),
               ez = fmax(fmax(b[2] - q2, q2 - b[5]), 0.0);
  return (ex * ex + ey * ey) + ez * ez;
}
// Queries are visited in Morton order of their position (30-bit keys over the cloud's bounding box grown by its own
// extent on every side; the sort is hipCUB's radix sort), so that the 64 lanes of a wave ask for neighbouring points
// and walk nearly the same boxes: in the caller's order (a grid in C order: 64 consecutive voxels are a line across
// the whole workspace) the lanes of a wave diverge at every node.
__host__ __device__ inline unsigned bvh_part1by2(unsigned v) {
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__global__ void k_query_keys(const double* __restrict__ query, long nq, const double* __restrict__ boxes, unsigned* __restrict__ keys,
                             unsigned* __restrict__ idx) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  unsigned key = 0u;
  for (int k = 0; k < 3; ++k) {
    const double lo = boxes[k], hi = boxes[3 + k], ext = hi - lo;
    double u = ext > 0.0 && ext < INFINITY ? (query[3 * q + k] - (lo - ext)) / (3.0 * ext) : 0.0;
    u = fmin(fmax(u, 0.0), 1.0);
    key |= bvh_part1by2((unsigned)(u * 1023.0)) << k;
  }
  keys[q] = key;
  idx[q] = (unsigned)q;
}
__global__ __launch_bounds__(256) void k_depth_sdf_bvh(const double* __restrict__ px, const double* __restrict__ py,
                                                       const double* __restrict__ pz, const double* __restrict__ boxes, int P,
                                                       const unsigned* __restrict__ order,
                                                       const float* __restrict__ depth, int H, int W,
                                                       const double* __restrict__ K, const double* __restrict__ cam_inv,
                                                       const double* __restrict__ query, long nq, float epsilon, float w_inside,
                                                       float* __restrict__ sdf_out, uint8_t* __restrict__ inside_out,
                                                       float* __restrict__ cost_out, unsigned long long* __restrict__ stats, int cost_only) {
#pragma clang fp contract(off)
  // cost_only (gto_scene_from_depth: only the COST is wanted): a query in front of the surfaces costs nothing once it is
  // epsilon away from every point ((d - epsilon)^2 / (2 epsilon) for 0 < d < epsilon, else 0: depth_point_cloud.py:86-89),
  // so its search starts from the bound epsilon^2 (a hair above: the float comparison `dist < epsilon` must see every
  // point it could) instead of infinity.  A point within epsilon is still found exactly; without one the cost is the same
  // 0; most voxels of a grid with a 0.4 m margin never leave the root.  (The distance written for such queries is the
  // bound, not the distance: sdf_out is not for cost_only callers.)
  // PACKET traversal: the 64 queries of a wave (neighbours in space, see k_query_keys) walk the tree TOGETHER with one
  // stack; a node is entered when any lane still needs it, and the 32 points of a leaf are fetched once per wave and
  // tried by every lane.  Trying more points than a lane needs cannot change its minimum (they are points of the cloud),
  // so the result is the exhaustive search's; what changes is that a leaf costs one coalesced read per wave instead of
  // one scattered read per lane (per-lane traversal moved 18 KB per query through the caches).
  __shared__ int s_stack[4][64];
  __shared__ double s_sbox[4][64][6];  // the box of every stacked node (read from memory once, when its parent is entered)
  __shared__ double s_pts[4][3][GTO_BVH_TILE_W * GTO_BVH_TILE_H];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long slot = (long)blockIdx.x * 256 + tid;
  const bool live = slot < nq;
  const long q = live ? (long)order[slot] : 0;  // the slot-th query in Morton order
  const double q0 = live ? query[3 * q] : 0.0, q1 = live ? query[3 * q + 1] : 0.0, q2 = live ? query[3 * q + 2] : 0.0;
  double best = INFINITY;
  if (cost_only && live && depth_is_outside(q0, q1, q2, depth, H, W, K, cam_inv)) best = (double)epsilon * (double)epsilon * (1.0 + 1e-6);
  const int first_leaf = P * P - 1;
  int* stk = s_stack[wave];
  int sp = 0;  // wave-uniform
  unsigned n_pop = 0, n_leaf = 0;
  if (lane == 0) stk[0] = 0;
  if (lane < 6) s_sbox[wave][0][lane] = boxes[lane];
  sp = 1;
  wave_sync_lds();
  while (sp > 0) {
    const int n = __builtin_amdgcn_readfirstlane(stk[sp - 1]);
    --sp;
    ++n_pop;
    const bool need = live && bvh_box_d2(s_sbox[wave][sp], q0, q1, q2) < best;
    if (!__any(need)) continue;  // too far for every lane (it may have become so since it was pushed)
    if (n >= first_leaf) {
      ++n_leaf;
      const int s = n - first_leaf;
      const int cx = (int)bvh_compact1by1((unsigned)s), cy = (int)bvh_compact1by1((unsigned)s >> 1);
      if (lane < GTO_BVH_TILE_W * GTO_BVH_TILE_H) {  // one pixel per lane; pixels outside the image count as invalid
        const int y = cy * GTO_BVH_TILE_H + lane / GTO_BVH_TILE_W, x = cx * GTO_BVH_TILE_W + lane % GTO_BVH_TILE_W;
        const bool in = y < H && x < W;
        const size_t j = in ? (size_t)y * W + x : 0;
        s_pts[wave][0][lane] = in ? px[j] : INFINITY;
        s_pts[wave][1][lane] = in ? py[j] : INFINITY;
        s_pts[wave][2][lane] = in ? pz[j] : INFINITY;
      }
      wave_sync_lds();
#pragma unroll 8
      for (int k = 0; k < GTO_BVH_TILE_W * GTO_BVH_TILE_H; ++k) {
        const double dx = q0 - s_pts[wave][0][k], dy = q1 - s_pts[wave][1][k], dz = q2 - s_pts[wave][2][k];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        best = fmin(best, d2);  // invalid pixels are points at infinity: d2 = inf
      }
      wave_sync_lds();  // every lane is done with the tile before the next leaf overwrites it
    } else {
      const int c1 = 2 * n + 1, c2 = c1 + 1;
      const double bx = lane < 12 ? boxes[(size_t)c1 * 6 + lane] : 0.0;  // both children's boxes: twelve consecutive doubles
      const double d1 = bvh_box_d2(boxes + (size_t)c1 * 6, q0, q1, q2), d2 = bvh_box_d2(boxes + (size_t)c2 * 6, q0, q1, q2);
      const bool n1 = live && d1 < best, n2 = live && d2 < best;
      // the child more lanes are closer to is entered first (it is pushed last)
      const bool c1_first = __popcll(__ballot(live && d1 <= d2)) * 2 >= __popcll(__ballot(live));
      const bool any1 = __any(n1), any2 = __any(n2);
      const int firstc = c1_first ? c1 : c2, secondc = c1_first ? c2 : c1;
      const bool any_first = c1_first ? any1 : any2, any_second = c1_first ? any2 : any1;
      // lane l < 12 holds entry l % 6 of child c1 (l < 6) or c2: it files it under the slot its child gets
      const bool mine_is_second = (lane < 6) != c1_first;
      if (any_second) {
        if (lane == 0) stk[sp] = secondc;
        if (lane < 12 && mine_is_second) s_sbox[wave][sp][lane % 6] = bx;
        ++sp;
      }
      if (any_first) {
        if (lane == 0) stk[sp] = firstc;
        if (lane < 12 && !mine_is_second) s_sbox[wave][sp][lane % 6] = bx;
        ++sp;
      }
      wave_sync_lds();
    }
  }
  if (stats) {
    if (lane == 0) {
      atomicAdd(stats, (unsigned long long)n_pop * 64);
      atomicAdd(stats + 1, (unsigned long long)n_leaf * 64);
      atomicAdd(stats + 2, (unsigned long long)n_pop);
    }
  }
  depth_sdf_finish(live, q, q0, q1, q2, best, depth, H, W, K, cam_inv, epsilon, w_inside, sdf_out, inside_out, cost_out);
}

// ---- host side: what the entry points of gto_api.hip hand to the launches below, and the launches.  All pointers: device.
struct DepthCamera { const double *K, *Kinv, *pose, *inv; };
// The world points of an image's pixels and the bounding-box hierarchy over their 8 x 4 pixel tiles (P x P leaf slots;
// P = 0: none, the cloud is for the exhaustive search).  A search of the cloud reads the image again (visibility test).
struct DepthCloud { const float* depth; int H, W; double *px, *py, *pz; int P; double* boxes; };
struct DepthQueries { const double* q; long nq; const unsigned* order; };  // [nq][3]; order: sort_queries (tree search only)
struct DepthFields { float* sdf; uint8_t* inside; float* cost; };          // per query; each may be null

// Leaf slots per side of the hierarchy of an H x W image (a power of two); k_bvh_up's single workgroup builds up to GTO_BVH_MAX_P
#define GTO_BVH_MAX_P 1024
inline int tile_levels(int H, int W) {
  const int tx = (W + GTO_BVH_TILE_W - 1) / GTO_BVH_TILE_W, ty = (H + GTO_BVH_TILE_H - 1) / GTO_BVH_TILE_H;
  int P = 1;
  while (P < tx || P < ty) P <<= 1;
  return P;
}
inline size_t bvh_box_doubles(int P) { return (size_t)(2 * P * P) * 6; }

// back-projection (pixels under `d_mask` and beyond `threshold` left out; d_valid: the flags), leaf boxes, inner boxes
inline void build_cloud(const DepthCloud& cl, const DepthCamera& cam, const uint8_t* d_mask, double threshold, uint8_t* d_valid) {
  const size_t N = (size_t)cl.H * cl.W;
  const int P = cl.P;
  hipLaunchKernelGGL(k_depth_backproject, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, cl.depth, cl.H, cl.W, cam.Kinv, cam.pose, d_mask,
                     threshold, cl.px, cl.py, cl.pz, d_valid);
  if (P) hipLaunchKernelGGL(k_bvh_leaves, dim3((unsigned)((P * P + 255) / 256)), dim3(256), 0, 0, cl.px, cl.py, cl.pz, cl.H, cl.W, P, cl.boxes);
  if (P > 1) hipLaunchKernelGGL(k_bvh_up, dim3(1), dim3(1024), 0, 0, P * P, cl.boxes);
}

inline void search_tree(hipStream_t stream, const DepthCloud& cl, const DepthCamera& cam, const DepthQueries& qs, float epsilon, float w_inside,
                 const DepthFields& out, unsigned long long* d_stats, bool cost_only) {
  hipLaunchKernelGGL(k_depth_sdf_bvh, dim3((unsigned)((qs.nq + 255) / 256)), dim3(256), 0, stream, cl.px, cl.py, cl.pz, cl.boxes, cl.P, qs.order,
                     cl.depth, cl.H, cl.W, cam.K, cam.inv, qs.q, qs.nq, epsilon, w_inside, out.sdf, out.inside, out.cost, d_stats, cost_only ? 1 : 0);
}
inline void search_exhaustive(hipStream_t stream, const DepthCloud& cl, const DepthCamera& cam, const DepthQueries& qs, float epsilon, float w_inside,
                       const DepthFields& out) {
  hipLaunchKernelGGL(k_depth_sdf, dim3((unsigned)((qs.nq + 255) / 256)), dim3(256), 0, stream, cl.px, cl.py, cl.pz, cl.H * cl.W, cl.depth, cl.H, cl.W,
                     cam.K, cam.inv, qs.q, qs.nq, epsilon, w_inside, out.sdf, out.inside, out.cost);
}
