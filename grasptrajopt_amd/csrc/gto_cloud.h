// gto_cloud.h — cost field from a sampled triangle mesh (gto_cloud_sdf_cost, gto_scene_from_clouds: include/gto_solver.h).
// The reference's SurfacePointCloud (mesh_to_sdf/surface_point_cloud.py:16-105, the use_depth_buffer=False branch of
// get_sdf, :46-54): the distance from every query to the nearest sample, its sign by a vote of the normals of the k nearest
// samples (k = sample_count = 11), and the cost map of mesh_to_sdf/depth_point_cloud.py:84-89.  FP64 with FMA contraction
// off, squared distances and dot products summed x, y, z: the reference's values bit for bit wherever the k-th and the
// (k+1)-th distance differ (tests/golden/surface_cloud.npz).
//
// A sampled mesh has no image order, so the tiles of gto_depth.h cannot serve it.  The cloud is ordered instead:
//   k_query_keys (gto_depth.h)  30-bit Morton keys of the samples over their bounding box; hipCUB radix sort (sort_queries)
//   k_cloud_gather              one lane per sorted slot: the samples' coordinates as SoA in key order, the caller's index
//                               beside them; slots behind the last sample are points at infinity
//   k_cloud_leaves              one lane per leaf: the box of GTO_CLOUD_LEAF consecutive sorted samples; the inner boxes are
//                               k_bvh_up's (implicit complete binary tree, heap indexing, a power of two of leaf slots)
//   k_cloud_knn<KCAP>           one wave per 64 queries in Morton order: the k nearest samples by a packet walk of the tree
//   k_cloud_knn_brute<KCAP>     one lane per query: the same by exhaustive search, the cloud streamed through LDS in the
//                               caller's order: no keys, no sort, no tree (GTO_CLOUD_BRUTE; the reference construction)
//
// The k best.  Samples are ordered by (squared distance, caller's index): a strict total order, so "the k best of a set" does
// not depend on the order in which the set is visited, and the tree search and the exhaustive search agree bit for bit, also
// on clouds with duplicated samples.  (The reference's KD-tree leaves ties open: it is matched where there are none.)
// A lane keeps its KCAP >= k best in registers, sorted, every index a compile-time constant (a runtime-indexed per-lane
// array would live in scratch); kth = the squared distance of entry k - 1 is picked by an unrolled select.
//
// The skip test for k > 1.  A box is skipped by a lane when (distance of the query to the box) > kth.  For a sample p of
// the box, |q - p| >= box distance holds per axis after rounding as well (subtraction, product and sum are monotone, and
// both are summed in the same order: gto_depth.h), so p is farther than k samples the lane already holds and cannot be
// among the k best.  A box AT the distance kth is entered: it may hold a sample that ties with entry k - 1 and has the lower
// index.  The packet tries every sample of an entered leaf on every lane; trying more samples than a lane needs cannot
// change the k best of a total order.
#pragma once
#include "gto_depth.h"

#define GTO_CLOUD_LEAF 32     // samples per leaf (one LDS tile of the packet walk)
#define GTO_CLOUD_MAX_K 16    // cap of k (the reference's sample_count is 11)
#define GTO_CLOUD_NO_INDEX 0xffffffffu

// The KCAP best (squared distance, caller's index) of a lane, ascending
template <int KCAP>
struct CloudBest {
  double d[KCAP];
  unsigned i[KCAP];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < KCAP; ++s) d[s] = INFINITY, i[s] = GTO_CLOUD_NO_INDEX;
  }
  __device__ __forceinline__ void offer(double d2, unsigned id) {
    if (d2 < d[KCAP - 1] || (d2 == d[KCAP - 1] && id < i[KCAP - 1])) {
      d[KCAP - 1] = d2, i[KCAP - 1] = id;
#pragma unroll
      for (int s = KCAP - 1; s > 0; --s) {  // one pass of a bubble sort carries the new entry to its place
        const bool swap = d[s] < d[s - 1] || (d[s] == d[s - 1] && i[s] < i[s - 1]);
        const double td = d[s - 1];
        const unsigned ti = i[s - 1];
        d[s - 1] = swap ? d[s] : td, i[s - 1] = swap ? i[s] : ti;
        d[s] = swap ? td : d[s], i[s] = swap ? ti : i[s];
      }
    }
  }
  // squared distance of entry k - 1, every index a constant (a loop over the entries left the list in scratch)
  template <int S>
  __device__ __forceinline__ double pick(int k, double v) const {
    if constexpr (S < 0) return v;
    else return pick<S - 1>(k, (S >= k - 1) ? d[S] : v);
  }
  __device__ __forceinline__ double kth(int k) const { return pick<KCAP - 2>(k, d[KCAP - 1]); }
};

// What follows the search of a query (surface_point_cloud.py:46-54, depth_point_cloud.py:84-89): vote of the k nearest
// samples' normals, signed float32 distance, cost.  points / normals: the caller's arrays [n][3].
template <int KCAP>
__device__ __forceinline__ void cloud_finish(bool live, long q, double q0, double q1, double q2, const CloudBest<KCAP>& best, int k,
                                             const double* __restrict__ points, const double* __restrict__ normals, unsigned n,
                                             float epsilon, float w_inside, float* __restrict__ sdf_out,
                                             uint8_t* __restrict__ inside_out, float* __restrict__ cost_out,
                                             int32_t* __restrict__ nearest_out) {
#pragma clang fp contract(off)
  if (!live) return;
  int votes = 0;
#pragma unroll
  for (int s = 0; s < KCAP; ++s) {
    const unsigned j = best.i[s];
    if (s < k && j < n) {  // (an entry that was never filled -- a query with a NaN coordinate -- names no sample)
      const double dx = q0 - points[3 * (size_t)j], dy = q1 - points[3 * (size_t)j + 1], dz = q2 - points[3 * (size_t)j + 2];
      const double dot = (dx * normals[3 * (size_t)j] + dy * normals[3 * (size_t)j + 1]) + dz * normals[3 * (size_t)j + 2];
      votes += dot < 0.0 ? 1 : 0;
    }
  }
  const bool inside = (double)votes > 0.5 * (double)k;
  float dist = (float)sqrt(best.d[0]);
  if (inside) dist = -dist;
  if (sdf_out) sdf_out[q] = dist;
  if (inside_out) inside_out[q] = inside ? 1 : 0;
  if (cost_out) cost_out[q] = sdf_cost_map(dist, inside, epsilon, w_inside);
  if (nearest_out) nearest_out[q] = best.i[0] < n ? (int32_t)best.i[0] : -1;
}

// order[s] = caller's index of the s-th sample in key order; slots in [n, n_slots) are points at infinity
__global__ void k_cloud_gather(const double* __restrict__ points, unsigned n, unsigned n_slots, const unsigned* __restrict__ order,
                               double* __restrict__ px, double* __restrict__ py, double* __restrict__ pz, unsigned* __restrict__ pid) {
  const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const bool real = s < n;
  const unsigned j = real ? order[s] : 0u;
  px[s] = real ? points[3 * (size_t)j] : INFINITY;
  py[s] = real ? points[3 * (size_t)j + 1] : INFINITY;
  pz[s] = real ? points[3 * (size_t)j + 2] : INFINITY;
  pid[s] = real ? j : GTO_CLOUD_NO_INDEX;
}

// boxes: as gto_depth.h ([node][6], an empty box is (+inf, -inf)); leaf l of n_leaves (a power of two) is node n_leaves - 1 + l
__global__ void k_cloud_leaves(const double* __restrict__ px, const double* __restrict__ py, const double* __restrict__ pz,
                               unsigned n_slots, int n_leaves, double* __restrict__ boxes) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_leaves) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int r = 0; r < GTO_CLOUD_LEAF; ++r) {
    const size_t s = (size_t)l * GTO_CLOUD_LEAF + r;
    if (s >= n_slots) break;
    const double v[3] = {px[s], py[s], pz[s]};
    if (!(v[0] < INFINITY)) continue;  // a slot behind the last sample
    for (int a = 0; a < 3; ++a) lo[a] = fmin(lo[a], v[a]), hi[a] = fmax(hi[a], v[a]);
  }
  double* b = boxes + (size_t)(n_leaves - 1 + l) * 6;
  for (int a = 0; a < 3; ++a) b[a] = lo[a], b[3 + a] = hi[a];
}

// The packet walk of k_depth_sdf_bvh (gto_depth.h) with k best per lane instead of one
template <int KCAP>
__global__ __launch_bounds__(256) void k_cloud_knn(const double* __restrict__ px, const double* __restrict__ py,
                                                   const double* __restrict__ pz, const unsigned* __restrict__ pid,
                                                   unsigned n_slots, const double* __restrict__ boxes, int n_leaves,
                                                   const unsigned* __restrict__ order, const double* __restrict__ points,
                                                   const double* __restrict__ normals, unsigned n, int k,
                                                   const double* __restrict__ query, long nq, float epsilon, float w_inside,
                                                   float* __restrict__ sdf_out, uint8_t* __restrict__ inside_out,
                                                   float* __restrict__ cost_out, int32_t* __restrict__ nearest_out) {
#pragma clang fp contract(off)
  __shared__ int s_stack[4][64];
  __shared__ double s_sbox[4][64][6];
  __shared__ double s_pts[4][3][GTO_CLOUD_LEAF];
  __shared__ unsigned s_pid[4][GTO_CLOUD_LEAF];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long slot = (long)blockIdx.x * 256 + tid;
  const bool live = slot < nq;
  const long q = live ? (order ? (long)order[slot] : slot) : 0;  // no order: the caller's (queries that are neighbours as they come)
  const double q0 = live ? query[3 * q] : 0.0, q1 = live ? query[3 * q + 1] : 0.0, q2 = live ? query[3 * q + 2] : 0.0;
  CloudBest<KCAP> best;
  best.clear();
  double kth = INFINITY;
  const int first_leaf = n_leaves - 1;
  int* stk = s_stack[wave];
  int sp = 0;  // wave-uniform; at most (levels + 1) entries: the tree has at most 27 levels (gto_api.hip caps the cloud)
  if (lane == 0) stk[0] = 0;
  if (lane < 6) s_sbox[wave][0][lane] = boxes[lane];
  sp = 1;
  wave_sync_lds();
  while (sp > 0) {
    const int node = __builtin_amdgcn_readfirstlane(stk[sp - 1]);
    --sp;
    const bool need = live && bvh_box_d2(s_sbox[wave][sp], q0, q1, q2) <= kth;
    if (!__any(need)) continue;
    if (node >= first_leaf) {
      const size_t s = (size_t)(node - first_leaf) * GTO_CLOUD_LEAF + lane;
      if (lane < GTO_CLOUD_LEAF) {
        const bool in = s < n_slots;
        s_pts[wave][0][lane] = in ? px[s] : INFINITY;
        s_pts[wave][1][lane] = in ? py[s] : INFINITY;
        s_pts[wave][2][lane] = in ? pz[s] : INFINITY;
        s_pid[wave][lane] = in ? pid[s] : GTO_CLOUD_NO_INDEX;
      }
      wave_sync_lds();
#pragma unroll 4
      for (int r = 0; r < GTO_CLOUD_LEAF; ++r) {
        const double dx = q0 - s_pts[wave][0][r], dy = q1 - s_pts[wave][1][r], dz = q2 - s_pts[wave][2][r];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        best.offer(d2, s_pid[wave][r]);  // a point at infinity: (inf, no index) is never below an entry
      }
      kth = best.kth(k);
      wave_sync_lds();
    } else {
      const int c1 = 2 * node + 1, c2 = c1 + 1;
      const double bx = lane < 12 ? boxes[(size_t)c1 * 6 + lane] : 0.0;
      const double d1 = bvh_box_d2(boxes + (size_t)c1 * 6, q0, q1, q2), d2 = bvh_box_d2(boxes + (size_t)c2 * 6, q0, q1, q2);
      const bool n1 = live && d1 <= kth, n2 = live && d2 <= kth;
      const bool c1_first = __popcll(__ballot(live && d1 <= d2)) * 2 >= __popcll(__ballot(live));
      const bool any1 = __any(n1), any2 = __any(n2);
      const int firstc = c1_first ? c1 : c2, secondc = c1_first ? c2 : c1;
      const bool any_first = c1_first ? any1 : any2, any_second = c1_first ? any2 : any1;
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
  cloud_finish<KCAP>(live, q, q0, q1, q2, best, k, points, normals, n, epsilon, w_inside, sdf_out, inside_out, cost_out, nearest_out);
}

// The exhaustive search: the caller's arrays as they are
template <int KCAP>
__global__ __launch_bounds__(256) void k_cloud_knn_brute(const double* __restrict__ points, const double* __restrict__ normals,
                                                         unsigned n, int k, const double* __restrict__ query, long nq,
                                                         float epsilon, float w_inside, float* __restrict__ sdf_out,
                                                         uint8_t* __restrict__ inside_out, float* __restrict__ cost_out,
                                                         int32_t* __restrict__ nearest_out) {
#pragma clang fp contract(off)
  __shared__ double sx[256], sy[256], sz[256];
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = q < nq;
  const double q0 = live ? query[3 * q] : 0.0, q1 = live ? query[3 * q + 1] : 0.0, q2 = live ? query[3 * q + 2] : 0.0;
  CloudBest<KCAP> best;
  best.clear();
  for (unsigned base = 0; base < n; base += 256) {
    const unsigned j = base + threadIdx.x;
    sx[threadIdx.x] = j < n ? points[3 * (size_t)j] : INFINITY;
    sy[threadIdx.x] = j < n ? points[3 * (size_t)j + 1] : INFINITY;
    sz[threadIdx.x] = j < n ? points[3 * (size_t)j + 2] : INFINITY;
    __syncthreads();
    const unsigned m = n - base < 256u ? n - base : 256u;
#pragma unroll 4
    for (unsigned r = 0; r < m; ++r) {
      const double dx = q0 - sx[r], dy = q1 - sy[r], dz = q2 - sz[r];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      best.offer(d2, base + r);
    }
    __syncthreads();
  }
  cloud_finish<KCAP>(live, q, q0, q1, q2, best, k, points, normals, n, epsilon, w_inside, sdf_out, inside_out, cost_out, nearest_out);
}

// ---- host side.  All pointers: device.
// A cloud as the caller gave it (points, normals [n][3]) and, for the tree search, its samples in key order with the
// hierarchy over them (n_leaves = 0: none)
struct SampleCloud {
  const double *points, *normals;
  unsigned n;
  double *px, *py, *pz;
  unsigned* pid;
  unsigned n_slots;
  int n_leaves;
  double* boxes;
};
struct CloudFields { float* sdf; uint8_t* inside; float* cost; int32_t* nearest; };  // per query; each may be null

inline int cloud_leaf_slots(unsigned n) {  // a power of two of leaves of GTO_CLOUD_LEAF samples
  const unsigned leaves = (n + GTO_CLOUD_LEAF - 1) / GTO_CLOUD_LEAF;
  int p = 1;
  while ((unsigned)p < leaves) p <<= 1;
  return p;
}

// samples into key order, leaf boxes, inner boxes; `order`: the samples' indices sorted by key (sort_queries)
inline void build_sample_tree(const SampleCloud& cl, const unsigned* order) {
  hipLaunchKernelGGL(k_cloud_gather, dim3((cl.n_slots + 255) / 256), dim3(256), 0, 0, cl.points, cl.n, cl.n_slots, order, cl.px, cl.py, cl.pz, cl.pid);
  hipLaunchKernelGGL(k_cloud_leaves, dim3((unsigned)((cl.n_leaves + 255) / 256)), dim3(256), 0, 0, cl.px, cl.py, cl.pz, cl.n_slots, cl.n_leaves, cl.boxes);
  if (cl.n_leaves > 1) hipLaunchKernelGGL(k_bvh_up, dim3(1), dim3(1024), 0, 0, cl.n_leaves, cl.boxes);
}

// the smallest compiled list that holds k entries
#define GTO_CLOUD_DISPATCH(k, CALL) \
  do {                              \
    if ((k) <= 1) { CALL(1); }      \
    else if ((k) <= 12) { CALL(12); } \
    else { CALL(16); }              \
  } while (0)

inline void search_cloud_tree(hipStream_t stream, const SampleCloud& cl, int k, const DepthQueries& qs, float epsilon, float w_inside,
                              const CloudFields& out) {
#define GTO_CLOUD_TREE_CALL(KCAP)                                                                                                        \
  hipLaunchKernelGGL(k_cloud_knn<KCAP>, dim3((unsigned)((qs.nq + 255) / 256)), dim3(256), 0, stream, cl.px, cl.py, cl.pz, cl.pid, cl.n_slots, \
                     cl.boxes, cl.n_leaves, qs.order, cl.points, cl.normals, cl.n, k, qs.q, qs.nq, epsilon, w_inside, out.sdf, out.inside,   \
                     out.cost, out.nearest)
  GTO_CLOUD_DISPATCH(k, GTO_CLOUD_TREE_CALL);
#undef GTO_CLOUD_TREE_CALL
}
inline void search_cloud_exhaustive(hipStream_t stream, const SampleCloud& cl, int k, const DepthQueries& qs, float epsilon, float w_inside,
                                    const CloudFields& out) {
#define GTO_CLOUD_BRUTE_CALL(KCAP)                                                                                                    \
  hipLaunchKernelGGL(k_cloud_knn_brute<KCAP>, dim3((unsigned)((qs.nq + 255) / 256)), dim3(256), 0, stream, cl.points, cl.normals, cl.n, k, \
                     qs.q, qs.nq, epsilon, w_inside, out.sdf, out.inside, out.cost, out.nearest)
  GTO_CLOUD_DISPATCH(k, GTO_CLOUD_BRUTE_CALL);
#undef GTO_CLOUD_BRUTE_CALL
}
