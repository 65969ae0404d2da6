// Mesh simplification for the mesh exports (include/umhs_hip.h, "Mesh simplification"): vertex clustering on a uniform grid whose
// representatives minimise the cluster's plane quadric, with the colour, material label and abundances of the rows carried along.
// include/umhs_hip.h states the rules as THE definition; tests/simplify_ref.py restates them in numpy.
//
// The passes follow umhs_pointcloud.hip's and umhs_mesh.hip's "count, scan, emit", three times over (cluster heads, kept faces, used
// clusters): a flag per element, its count per chunk of 256 (ballot), the caller's scan of the chunk counts, the rank of every element
// (ballot below the lane + waves below + chunk offset).  The caller also does the three stable sorts (vertices by key, faces by their
// canonical triple, corner records by cluster): after them a cluster's members, a face's duplicates and a cluster's corner records are
// contiguous runs, so nothing here searches, hashes or uses an atomic, and every result is a function of the inputs alone.
//
//   sp_unpack_kernel    ONE VERTEX PER LANE: the 12 position bytes of a row (rows start at any byte address: byte loads) -> [V,3] floats,
//                       and the largest finite coordinate per axis of the chunk (wave max by shuffles, wave results through LDS).
//   sp_keys_kernel      one vertex per lane: two rounded float32 operations and a floor per axis, an int64 key.
//   sp_heads / flag_count / flag_rank / members / faces / dedup / emit   one element per lane, integers only, coalesced but for the
//                       gathers through a sorted order.
//   sp_clusters_kernel  ONE CLUSTER PER LANE, only the clusters a kept face names.  A lane walks its members and its corner records --
//                       both contiguous in their sorted orders, so the lanes of a wave read neighbouring runs of the two order arrays --
//                       and keeps the sums in registers: 9 float64 of the quadric, 3 of the mean, the bounding box, 3 integer colour sums
//                       and, with classes, 15 label counts (and one for the label -1) and 15 float64 abundance sums; then the 3 x 3
//                       Cholesky solve, the clamp, the one rounding to float32 and the row.  The sums are taken in member / record order by one lane: the same bits on
//                       every run, and the order tests/simplify_ref.py uses.  (A lane per record with a segmented wave scan would read
//                       the order arrays fully coalesced and balance the rare long run; it needs a carry across wave and workgroup
//                       borders for a 9- and a 36-value payload.  The positions behind the records are gathers either way.  DESIGN.md 7.)
//
// The unit is compiled with contraction off: the float32 steps of the key are single rounded operations (umhs_exact.h), and the float64
// sums are the plain products and sums the restatement forms, never fused.
#pragma clang fp contract(off)
#include <limits.h>

#include "umhs_common.h"
#include "umhs_exact.h"
#include "umhs_affine.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_CLASSES = 15;
constexpr int64_t SP_NO_KEY = INT64_MAX;
constexpr int32_t SP_NO_CLUSTER = INT32_MAX;
constexpr double SP_RHO = 1e-3;

__device__ __forceinline__ uint32_t sp_load32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ void sp_store32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

// cell of coordinate p along an axis of n cells: min((int)floor((p - g) / e), n - 1), clamped below at 0 (p finite)
__device__ __forceinline__ int sp_cell(float p, float g, float e, int n) {
  const float f = floorf(xf_div(xf_sub(p, g), e));
  if (!(f > 0.0f)) return 0;
  if (f >= 2147483648.0f) return n - 1;
  const int i = (int)f;
  return i < n - 1 ? i : n - 1;
}

__global__ __launch_bounds__(SP_THREADS) void sp_unpack_kernel(const uint8_t* __restrict__ rows, int64_t V, int row_bytes,
                                                               float* __restrict__ positions, float* __restrict__ chunk_max) {
  __shared__ float wmax[SP_THREADS / UMHS_WAVE][3];
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  float m[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < V) {
    const uint8_t* row = rows + i * (int64_t)row_bytes;
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = __uint_as_float(sp_load32(row + 4 * k)), positions[3 * i + k] = p[k];
    if (xf_finite(p[0]) && xf_finite(p[1]) && xf_finite(p[2])) m[0] = p[0], m[1] = p[1], m[2] = p[2];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m[k] = fmaxf(m[k], __shfl_xor(m[k], d, 64));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) wmax[threadIdx.x >> 6][k] = m[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float r = wmax[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < SP_THREADS / UMHS_WAVE; ++w) r = fmaxf(r, wmax[w][threadIdx.x]);
    chunk_max[3 * (int64_t)blockIdx.x + threadIdx.x] = r;
  }
}

struct sp_grid {
  float g[3], e;
  int n[3];
};

__global__ __launch_bounds__(SP_THREADS) void sp_keys_kernel(const float* __restrict__ positions, int64_t V, sp_grid G,
                                                             int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= V) return;
  const float p0 = positions[3 * i], p1 = positions[3 * i + 1], p2 = positions[3 * i + 2];
  int64_t key = SP_NO_KEY;
  if (xf_finite(p0) && xf_finite(p1) && xf_finite(p2)) {
    const int ix = sp_cell(p0, G.g[0], G.e, G.n[0]), iy = sp_cell(p1, G.g[1], G.e, G.n[1]), iz = sp_cell(p2, G.g[2], G.e, G.n[2]);
    key = ((int64_t)iz * G.n[1] + iy) * G.n[0] + ix;
  }
  keys[i] = key;
}

__global__ __launch_bounds__(SP_THREADS) void sp_heads_kernel(const int64_t* __restrict__ sorted_keys, int64_t V,
                                                              uint8_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= V) return;
  const int64_t k = sorted_keys[i];
  head[i] = (k != SP_NO_KEY && (i == 0 || sorted_keys[i - 1] != k)) ? 1 : 0;
}

__global__ __launch_bounds__(SP_THREADS) void sp_flag_count_kernel(const uint8_t* __restrict__ flags, int64_t n,
                                                                   int32_t* __restrict__ counts) {
  __shared__ int wave_total[SP_THREADS / UMHS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  const int c = __popcll(__ballot(i < n && flags[i] != 0));
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
}

__global__ __launch_bounds__(SP_THREADS) void sp_flag_rank_kernel(const uint8_t* __restrict__ flags, int64_t n,
                                                                  const int64_t* __restrict__ offsets, int32_t* __restrict__ rank) {
  __shared__ int wave_total[SP_THREADS / UMHS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long ballot = __ballot(i < n && flags[i] != 0);
  if (lane == 0) wave_total[wave] = __popcll(ballot);
  __syncthreads();
  int below = __popcll(ballot & ((1ull << lane) - 1ull));  // set flags below this lane: lane order is element order
#pragma unroll
  for (int k = 0; k < SP_THREADS / UMHS_WAVE - 1; ++k) below += (k < wave) ? wave_total[k] : 0;
  if (i < n) rank[i] = (int32_t)(offsets[blockIdx.x] + below);
}

__global__ __launch_bounds__(SP_THREADS) void sp_members_kernel(const int64_t* __restrict__ sorted_keys,
                                                                const int64_t* __restrict__ order, const uint8_t* __restrict__ head,
                                                                const int32_t* __restrict__ head_rank, int64_t V,
                                                                int32_t* __restrict__ vertex_cluster, int32_t* __restrict__ cluster_start) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= V) return;
  const int64_t v = order[i];
  if ((uint64_t)v >= (uint64_t)V) return;  // (never with a permutation of [0, V))
  if (sorted_keys[i] == SP_NO_KEY) {
    vertex_cluster[v] = -1;
    return;
  }
  const int64_t c = (int64_t)head_rank[i] + head[i] - 1;  // (the first keyed position is a head: c >= 0; c < V)
  if (c < 0 || c >= V) return;
  vertex_cluster[v] = (int32_t)c;
  if (head[i]) cluster_start[c] = (int32_t)i;
  if (i + 1 == V || sorted_keys[i + 1] == SP_NO_KEY) cluster_start[c + 1] = (int32_t)(i + 1);  // the end of the last cluster
}

__global__ __launch_bounds__(SP_THREADS) void sp_faces_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                              const int32_t* __restrict__ vertex_cluster, int64_t V,
                                                              int32_t* __restrict__ face_cluster, int64_t* __restrict__ key_hi,
                                                              int32_t* __restrict__ key_lo) {
  const int64_t f = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (f >= F) return;
  const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  int32_t ca = SP_NO_CLUSTER, cb = SP_NO_CLUSTER, cc = SP_NO_CLUSTER;
  int64_t hi = SP_NO_KEY;
  int32_t lo = 0;
  if ((uint64_t)(uint32_t)a < (uint64_t)V && (uint64_t)(uint32_t)b < (uint64_t)V && (uint64_t)(uint32_t)c < (uint64_t)V) {
    const int32_t ka = vertex_cluster[a], kb = vertex_cluster[b], kc = vertex_cluster[c];
    if (ka >= 0 && kb >= 0 && kc >= 0) {
      ca = ka, cb = kb, cc = kc;
      if (ka != kb && kb != kc && ka != kc) {  // the smallest cluster to the front, the orientation kept
        int32_t c0 = ka, c1 = kb, c2 = kc;
        if (kb < ka && kb < kc) c0 = kb, c1 = kc, c2 = ka;
        else if (kc < ka && kc < kb) c0 = kc, c1 = ka, c2 = kb;
        hi = ((int64_t)c0 << 31) | (int64_t)c1;
        lo = c2;
      }
    }
  }
  face_cluster[3 * f] = ca, face_cluster[3 * f + 1] = cb, face_cluster[3 * f + 2] = cc;
  key_hi[f] = hi, key_lo[f] = lo;
}

__global__ __launch_bounds__(SP_THREADS) void sp_dedup_kernel(const int64_t* __restrict__ key_hi, const int32_t* __restrict__ key_lo,
                                                              const int64_t* __restrict__ perm, const int32_t* __restrict__ face_cluster,
                                                              int64_t F, int64_t n_clusters, uint8_t* __restrict__ keep,
                                                              uint8_t* __restrict__ used) {
  const int64_t j = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (j >= F) return;
  const int64_t f = perm[j];
  if ((uint64_t)f >= (uint64_t)F) return;  // (never with a permutation of [0, F))
  const int64_t hi = key_hi[f];
  bool kept = hi != SP_NO_KEY;
  if (kept && j > 0) {  // equal faces are neighbours, the first in input order first (the sorts are stable)
    const int64_t g = perm[j - 1];
    if ((uint64_t)g < (uint64_t)F && key_hi[g] == hi && key_lo[g] == key_lo[f]) kept = false;
  }
  keep[f] = kept ? 1 : 0;
  if (kept && used) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int32_t c = face_cluster[3 * f + t];
      if ((uint64_t)(uint32_t)c < (uint64_t)n_clusters) used[c] = 1;  // (every writer stores the same byte)
    }
  }
}

__global__ __launch_bounds__(SP_THREADS) void sp_emit_faces_kernel(const int32_t* __restrict__ face_cluster,
                                                                   const uint8_t* __restrict__ keep, const int32_t* __restrict__ face_rank,
                                                                   const int32_t* __restrict__ cluster_rank, int64_t F, int64_t n_clusters,
                                                                   int32_t* __restrict__ faces_out, int64_t cap) {
  const int64_t f = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (f >= F || !keep[f]) return;
  const int64_t at = face_rank[f];
  if (at < 0 || at >= cap) return;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int32_t c = face_cluster[3 * f + t];
    faces_out[3 * at + t] = (uint64_t)(uint32_t)c < (uint64_t)n_clusters ? cluster_rank[c] : -1;
  }
}

__global__ __launch_bounds__(SP_THREADS) void sp_emit_vertices_kernel(const int32_t* __restrict__ vertex_cluster,
                                                                      const uint8_t* __restrict__ used,
                                                                      const int32_t* __restrict__ cluster_rank, int64_t V, int64_t n_clusters,
                                                                      int32_t* __restrict__ vertex_out) {
  const int64_t v = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (v >= V) return;
  const int32_t c = vertex_cluster[v];
  vertex_out[v] = ((uint64_t)(uint32_t)c < (uint64_t)n_clusters && used[c]) ? cluster_rank[c] : -1;
}

__global__ __launch_bounds__(SP_THREADS) void sp_clusters_kernel(umhs_simplify_args P, xf_world Wd) {
#pragma clang fp contract(off)
  const int64_t c = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (c >= P.n_clusters || !P.used[c]) return;
  const int64_t at = P.cluster_rank[c];
  if (at < 0 || at >= P.cap) return;
  const int64_t V = P.n_vertices, F = P.n_faces;
  const int C = P.n_classes;
  const int row_bytes = C > 0 ? 19 + 4 * C : 15;
  const uint8_t* rows = reinterpret_cast<const uint8_t*>(P.rows);
  int64_t ms = P.cluster_start[c], me = P.cluster_start[c + 1];
  ms = ms < 0 ? 0 : (ms > V ? V : ms);
  me = me < ms ? ms : (me > V ? V : me);
  if (me == ms) return;  // (never: a cluster has its head)
  // the cell, from the first member (every member has the same one)
  double o[3], lo[3], hi[3];
  {
    const int64_t v0 = P.member_order[ms];
    if ((uint64_t)v0 >= (uint64_t)V) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = sp_cell(P.positions[3 * v0 + k], P.origin[k], P.edge, P.dims[k]);
      const double g = (double)P.origin[k], e = (double)P.edge;
      o[k] = g + ((double)i + 0.5) * e;
      lo[k] = g + (double)i * e;
      hi[k] = g + ((double)i + 1.0) * e;
    }
  }
  // members: mean offset, bounding box, colour sums, label counts, abundance sums
  double sm[3] = {0.0, 0.0, 0.0};
  unsigned long long col[3] = {0ull, 0ull, 0ull};
  int hist[SP_MAX_CLASSES + 1];  // bin 0: label -1, a vertex nobody tinted (umhs_mesh_vertices)
  double ab[SP_MAX_CLASSES];
#pragma unroll
  for (int k = 0; k < SP_MAX_CLASSES; ++k) hist[k + 1] = 0, ab[k] = 0.0;
  hist[0] = 0;
  for (int64_t j = ms; j < me; ++j) {
    const int64_t v = P.member_order[j];
    if ((uint64_t)v >= (uint64_t)V) continue;
    const uint8_t* row = rows + v * (int64_t)row_bytes;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double p = (double)P.positions[3 * v + k];
      sm[k] += p - o[k];
      lo[k] = p < lo[k] ? p : lo[k];
      hi[k] = p > hi[k] ? p : hi[k];
      col[k] += row[12 + k];
    }
    if (C > 0) {
      int label = (int)sp_load32(row + 15);
      label = label < -1 ? -1 : (label > C - 1 ? C - 1 : label);
      hist[0] += label == -1 ? 1 : 0;
#pragma unroll
      for (int k = 0; k < SP_MAX_CLASSES; ++k) {
        if (k < C) {
          hist[k + 1] += label == k ? 1 : 0;
          ab[k] += (double)__uint_as_float(sp_load32(row + 19 + 4 * k));
        }
      }
    }
  }
  const int64_t n = me - ms;
  const double m[3] = {sm[0] / (double)n, sm[1] / (double)n, sm[2] / (double)n};
  // corner records: the quadric of the planes of every valid input face at this cluster
  int64_t cs = P.corner_start[c], ce = P.corner_start[c + 1];
  cs = cs < 0 ? 0 : (cs > 3 * F ? 3 * F : cs);
  ce = ce < cs ? cs : (ce > 3 * F ? 3 * F : ce);
  double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int64_t j = cs; j < ce; ++j) {
    const int64_t r = P.corner_order[j];
    if ((uint64_t)r >= (uint64_t)(3 * F)) continue;
    const int64_t f = r / 3;
    const int32_t ia = P.faces[3 * f], ib = P.faces[3 * f + 1], ic = P.faces[3 * f + 2];
    if ((uint64_t)(uint32_t)ia >= (uint64_t)V || (uint64_t)(uint32_t)ib >= (uint64_t)V || (uint64_t)(uint32_t)ic >= (uint64_t)V) continue;
    double a[3], u[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = (double)P.positions[3 * (int64_t)ia + k];
      u[k] = (double)P.positions[3 * (int64_t)ib + k] - a[k];
      w[k] = (double)P.positions[3 * (int64_t)ic + k] - a[k];
    }
    const double n0 = u[1] * w[2] - u[2] * w[1], n1 = u[2] * w[0] - u[0] * w[2], n2 = u[0] * w[1] - u[1] * w[0];
    const double d = (n0 * (a[0] - o[0]) + n1 * (a[1] - o[1])) + n2 * (a[2] - o[2]);
    A00 += n0 * n0, A01 += n0 * n1, A02 += n0 * n2, A11 += n1 * n1, A12 += n1 * n2, A22 += n2 * n2;
    b0 += n0 * d, b1 += n1 * d, b2 += n2 * d;
  }
  const double tr = (A00 + A11) + A22;
  double x[3] = {m[0], m[1], m[2]};
  if (tr > 0.0) {  // (A + lambda I) x = b + lambda m, Cholesky: the matrix is positive definite with condition <= 1 + 3 / rho
    const double lam = (SP_RHO * tr) / 3.0;
    const double M00 = A00 + lam, M11 = A11 + lam, M22 = A22 + lam;
    const double r0 = b0 + lam * m[0], r1 = b1 + lam * m[1], r2 = b2 + lam * m[2];
    const double l00 = sqrt(M00), l10 = A01 / l00, l20 = A02 / l00;
    const double l11 = sqrt(M11 - l10 * l10), l21 = (A12 - l20 * l10) / l11;
    const double l22 = sqrt((M22 - l20 * l20) - l21 * l21);
    const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = ((r2 - l20 * y0) - l21 * y1) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = ((y0 - l10 * x[1]) - l20 * x[2]) / l00;
  }
  float p[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double y = o[k] + x[k];
    y = y < lo[k] ? lo[k] : (y > hi[k] ? hi[k] : y);
    p[k] = (float)y;
    P.positions_out[3 * at + k] = p[k];
  }
  xf_world_apply(Wd, p, w);
  uint8_t* out = reinterpret_cast<uint8_t*>(P.rows_out) + at * (int64_t)row_bytes;
#pragma unroll
  for (int k = 0; k < 3; ++k) sp_store32(out + 4 * k, __float_as_uint(w[k]));
#pragma unroll
  for (int k = 0; k < 3; ++k) out[12 + k] = (uint8_t)((2ull * col[k] + (unsigned long long)n) / (2ull * (unsigned long long)n));
  if (C > 0) {
    int best = hist[0], arg = -1;
#pragma unroll
    for (int k = 0; k < SP_MAX_CLASSES; ++k) {
      if (k < C && hist[k + 1] > best) best = hist[k + 1], arg = k;  // the first of the most frequent
    }
    sp_store32(out + 15, (uint32_t)arg);
#pragma unroll
    for (int k = 0; k < SP_MAX_CLASSES; ++k) {
      if (k < C) sp_store32(out + 19 + 4 * k, __float_as_uint((float)(ab[k] / (double)n)));
    }
  }
}

inline bool sp_blocks(int64_t n, unsigned& blocks) {
  const int64_t b = (n + SP_THREADS - 1) / SP_THREADS;
  if (b > 0x7fffffff) return false;
  blocks = (unsigned)b;
  return true;
}

inline bool sp_row_bytes_ok(int row_bytes) {
  return row_bytes == 15 || (row_bytes >= 23 && row_bytes <= 19 + 4 * SP_MAX_CLASSES && (row_bytes - 19) % 4 == 0);
}

}  // namespace

#define SP_LAUNCH(kernel, n, ...)                                                                        \
  do {                                                                                                   \
    unsigned blocks_;                                                                                    \
    if (!sp_blocks((n), blocks_)) return UMHS_ERR_UNSUPPORTED;                                           \
    hipLaunchKernelGGL(kernel, dim3(blocks_), dim3(SP_THREADS), 0, umhs_s(stream), __VA_ARGS__);         \
    UMHS_CHECK_LAUNCH();                                                                                 \
  } while (0)

extern "C" int umhs_simplify_unpack(const void* rows, int64_t n_vertices, int row_bytes, float* positions, float* chunk_max,
                                    umhs_stream_t stream) {
  if (n_vertices < 0 || !sp_row_bytes_ok(row_bytes)) return UMHS_ERR_ARG;
  if (n_vertices >= (1LL << 31)) return UMHS_ERR_UNSUPPORTED;
  if (n_vertices == 0) return UMHS_OK;
  if (!rows || !positions || !chunk_max) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_unpack_kernel, n_vertices, reinterpret_cast<const uint8_t*>(rows), n_vertices, row_bytes, positions, chunk_max);
  return UMHS_OK;
}

extern "C" int umhs_simplify_keys(const float* positions, int64_t n_vertices, const float* origin_host3, float edge,
                                  const int32_t* dims_host3, int64_t* keys, umhs_stream_t stream) {
  if (n_vertices < 0 || !origin_host3 || !dims_host3 || !(edge > 0.0f) || !xf_finite(edge)) return UMHS_ERR_ARG;
  sp_grid G;
  double cells = 1.0;
  for (int k = 0; k < 3; ++k) {
    if (!xf_finite(origin_host3[k]) || dims_host3[k] < 1) return UMHS_ERR_ARG;
    G.g[k] = origin_host3[k], G.n[k] = dims_host3[k];
    cells *= (double)dims_host3[k];
  }
  G.e = edge;
  if (cells >= 4611686018427387904.0) return UMHS_ERR_UNSUPPORTED;  // 2^62
  if (n_vertices == 0) return UMHS_OK;
  if (!positions || !keys) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_keys_kernel, n_vertices, positions, n_vertices, G, keys);
  return UMHS_OK;
}

extern "C" int umhs_simplify_heads(const int64_t* sorted_keys, int64_t n_vertices, uint8_t* head, umhs_stream_t stream) {
  if (n_vertices < 0) return UMHS_ERR_ARG;
  if (n_vertices == 0) return UMHS_OK;
  if (!sorted_keys || !head) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_heads_kernel, n_vertices, sorted_keys, n_vertices, head);
  return UMHS_OK;
}

extern "C" int umhs_simplify_flag_count(const uint8_t* flags, int64_t n, int32_t* counts, umhs_stream_t stream) {
  if (n < 0) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  if (!flags || !counts) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_flag_count_kernel, n, flags, n, counts);
  return UMHS_OK;
}

extern "C" int umhs_simplify_flag_rank(const uint8_t* flags, int64_t n, const int64_t* offsets, int32_t* rank, umhs_stream_t stream) {
  if (n < 0) return UMHS_ERR_ARG;
  if (n >= (1LL << 31)) return UMHS_ERR_UNSUPPORTED;
  if (n == 0) return UMHS_OK;
  if (!flags || !offsets || !rank) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_flag_rank_kernel, n, flags, n, offsets, rank);
  return UMHS_OK;
}

extern "C" int umhs_simplify_members(const int64_t* sorted_keys, const int64_t* member_order, const uint8_t* head, const int32_t* head_rank,
                                     int64_t n_vertices, int32_t* vertex_cluster, int32_t* cluster_start, umhs_stream_t stream) {
  if (n_vertices < 0) return UMHS_ERR_ARG;
  if (n_vertices >= (1LL << 31)) return UMHS_ERR_UNSUPPORTED;
  if (n_vertices == 0) return UMHS_OK;
  if (!sorted_keys || !member_order || !head || !head_rank || !vertex_cluster || !cluster_start) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_members_kernel, n_vertices, sorted_keys, member_order, head, head_rank, n_vertices, vertex_cluster, cluster_start);
  return UMHS_OK;
}

extern "C" int umhs_simplify_faces(const int32_t* faces, int64_t n_faces, const int32_t* vertex_cluster, int64_t n_vertices,
                                   int32_t* face_cluster, int64_t* key_hi, int32_t* key_lo, umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0) return UMHS_ERR_ARG;
  if (n_vertices >= (1LL << 31) || n_faces >= (1LL << 31) / 3) return UMHS_ERR_UNSUPPORTED;
  if (n_faces == 0) return UMHS_OK;
  if (!faces || !face_cluster || !key_hi || !key_lo || (n_vertices > 0 && !vertex_cluster)) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_faces_kernel, n_faces, faces, n_faces, vertex_cluster, n_vertices, face_cluster, key_hi, key_lo);
  return UMHS_OK;
}

extern "C" int umhs_simplify_dedup(const int64_t* key_hi, const int32_t* key_lo, const int64_t* perm, const int32_t* face_cluster,
                                   int64_t n_faces, int64_t n_clusters, uint8_t* keep, uint8_t* used, umhs_stream_t stream) {
  if (n_faces < 0 || n_clusters < 0) return UMHS_ERR_ARG;
  if (n_faces == 0) return UMHS_OK;
  if (!key_hi || !key_lo || !perm || !face_cluster || !keep) return UMHS_ERR_ARG;
  SP_LAUNCH(sp_dedup_kernel, n_faces, key_hi, key_lo, perm, face_cluster, n_faces, n_clusters, keep, used);
  return UMHS_OK;
}

extern "C" int umhs_simplify_clusters(const umhs_simplify_args* a, umhs_stream_t stream) {
  if (!a || a->n_vertices < 0 || a->n_faces < 0 || a->n_clusters < 0 || a->cap < 0) return UMHS_ERR_ARG;
  if (a->n_classes < 0 || a->n_classes > SP_MAX_CLASSES) return UMHS_ERR_ARG;
  if (a->n_vertices >= (1LL << 31) || a->n_faces >= (1LL << 31) / 3) return UMHS_ERR_UNSUPPORTED;
  if (!(a->edge > 0.0f) || !xf_finite(a->edge)) return UMHS_ERR_ARG;
  for (int k = 0; k < 3; ++k)
    if (!xf_finite(a->origin[k]) || a->dims[k] < 1) return UMHS_ERR_ARG;
  if (a->n_clusters == 0 || a->cap == 0) return UMHS_OK;
  if (a->n_clusters > a->n_vertices) return UMHS_ERR_ARG;
  if (!a->rows || !a->positions || !a->member_order || !a->cluster_start || !a->corner_start || !a->used || !a->cluster_rank ||
      !a->rows_out || !a->positions_out || (a->n_faces > 0 && (!a->faces || !a->corner_order)))
    return UMHS_ERR_ARG;
  xf_world w = xf_world_from_host(a->has_world ? a->world : nullptr);
  SP_LAUNCH(sp_clusters_kernel, a->n_clusters, *a, w);
  return UMHS_OK;
}

extern "C" int umhs_simplify_emit(const int32_t* face_cluster, const uint8_t* keep, const int32_t* face_rank, const int32_t* vertex_cluster,
                                  const uint8_t* used, const int32_t* cluster_rank, int64_t n_faces, int64_t n_vertices, int64_t n_clusters,
                                  int32_t* faces_out, int64_t cap, int32_t* vertex_out, umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_clusters < 0 || cap < 0) return UMHS_ERR_ARG;
  if (n_clusters > 0 && (!used || !cluster_rank)) return UMHS_ERR_ARG;
  if (n_faces > 0 && cap > 0) {
    if (!face_cluster || !keep || !face_rank || !faces_out) return UMHS_ERR_ARG;
    SP_LAUNCH(sp_emit_faces_kernel, n_faces, face_cluster, keep, face_rank, cluster_rank, n_faces, n_clusters, faces_out, cap);
  }
  if (n_vertices > 0) {
    if (!vertex_cluster || !vertex_out) return UMHS_ERR_ARG;
    SP_LAUNCH(sp_emit_vertices_kernel, n_vertices, vertex_cluster, used, cluster_rank, n_vertices, n_clusters, vertex_out);
  }
  return UMHS_OK;
}
