// Connected components of an exported mesh (include/umhs_hip.h, "Mesh components"): labelling, per-component face / vertex counts and
// area, and the compacting emit of the kept components.  include/umhs_hip.h states the rules as THE definition; tests/components_ref.py
// restates them in numpy.
//
// LABELLING.  parent[v] starts as v.  Two invariants hold after every store: parent[v] <= v, and parent[v] is a vertex of v's own
// component (every stored value is a parent that was read at a corner of a face the target is joined to, or an ancestor of the target).
// parent[] is only ever lowered, and only by atomicMin, so a value read at any time -- from memory, from another XCD's L2 or from a
// CU's L1 that no other CU's store refreshes -- is the current value or an older, LARGER one that satisfies the same invariants.  The
// kernels below never wait on one another: a stale read costs a round, never a wrong label.
//   cc_hook_kernel   ONE FACE PER LANE: m = the smallest of the three corners' parents; atomicMin(parent[x], m) for every corner's
//                    parent x above m (the parent of the corner's current parent) and for the corner itself.
//   cc_jump_kernel   ONE VERTEX PER LANE: chase the parents for at most CC_CHASE steps (the only data-dependent loop, capped) and
//                    atomicMin(parent[v], what the chase reached).
// Every atomicMin that returned a larger value than it stored sets this round's bit of one device word (one atomicOr per wave).  The
// launches of a round are ordered by the stream, and a kernel boundary is the only synchronisation: a round whose bit stayed clear
// read exactly the state at its launch, in which every tree is a star (the jump lowered nothing) and every face has one root (the hook
// lowered nothing), so every component has ONE root r with parent[r] = r <= every member: its smallest vertex.
// Rounds needed: after round k every vertex within k faces of the component's smallest vertex s has parent s (the hook lowers the
// corners themselves, and s can never be lowered), so at most V - 1 rounds change anything; the caller stops at V + 1.
//
// STATISTICS.  The caller sorts the face component ids (stable) and the vertex component ids; a component's faces and vertices are
// runs found by binary search.  Areas: float32 per face, every step one rounded operation (umhs_exact.h), widened to float64 and
// summed in face order: the sorted face list is cut at the multiples of 256 positions and at the component borders, ONE LANE sums a
// chunk's pieces element by element, then ONE LANE PER COMPONENT adds its pieces in order.  No float atomics: the same bits every run.
//
// EMIT.  Count, scan (the flag count / rank pair of umhs_simplify.hip, the caller's scan between them), emit: rows are copied byte for
// byte (15- and 43-byte rows are not 4-byte aligned), xyz through umhs_affine.h.
#pragma clang fp contract(off)
#include "umhs_common.h"
#include "umhs_exact.h"
#include "umhs_affine.h"

namespace {

constexpr int CC_THREADS = 256;  // faces / vertices / sorted positions per workgroup, and the positions of one piece chunk
constexpr int CC_CHASE = 16;     // parent-chase steps of one jump
constexpr int CC_MAX_ROUNDS = 32;  // rounds per call: the bits of the changed word
constexpr int CC_MAX_CLASSES = 15;

__device__ __forceinline__ bool cc_in(int32_t i, int64_t n) { return (uint64_t)(uint32_t)i < (uint64_t)n; }

__device__ __forceinline__ uint32_t cc_load32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ void cc_store32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

// parent[x] = min(parent[x], m); true iff that lowered it
__device__ __forceinline__ bool cc_lower(int32_t* parent, int32_t x, int32_t m) { return atomicMin(parent + x, m) > m; }

__device__ __forceinline__ void cc_report(bool lowered, uint32_t* changed, uint32_t bit) {
  if (__ballot(lowered) != 0ull && (threadIdx.x & 63) == 0) atomicOr(changed, bit);
}

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(int32_t* __restrict__ parent, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v < V) parent[v] = (int32_t)v;
}

__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, int32_t* parent,
                                                             uint32_t* changed, uint32_t bit) {
  const int64_t f = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  bool lowered = false;
  if (f < F) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (cc_in(a, V) && cc_in(b, V) && cc_in(c, V)) {
      const int32_t pa = parent[a], pb = parent[b], pc = parent[c];
      if (cc_in(pa, V) && cc_in(pb, V) && cc_in(pc, V)) {  // (always: parent[] holds vertex indices)
        const int32_t m = min(pa, min(pb, pc));
        if (pa > m) lowered |= cc_lower(parent, pa, m), lowered |= cc_lower(parent, a, m);
        if (pb > m) lowered |= cc_lower(parent, pb, m), lowered |= cc_lower(parent, b, m);
        if (pc > m) lowered |= cc_lower(parent, pc, m), lowered |= cc_lower(parent, c, m);
      }
    }
  }
  cc_report(lowered, changed, bit);
}

__global__ __launch_bounds__(CC_THREADS) void cc_jump_kernel(int64_t V, int32_t* parent, uint32_t* changed, uint32_t bit) {
  const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  bool lowered = false;
  if (v < V) {
    const int32_t p = parent[v];
    int32_t r = p;
    for (int k = 0; k < CC_CHASE; ++k) {
      if (!cc_in(r, V)) break;  // (never)
      const int32_t n = parent[r];
      if (n >= r || n < 0) break;
      r = n;
    }
    if (r < p && r >= 0) lowered = cc_lower(parent, (int32_t)v, r);
  }
  cc_report(lowered, changed, bit);
}

__global__ __launch_bounds__(CC_THREADS) void cc_roots_kernel(const int32_t* __restrict__ parent, int64_t V, uint8_t* __restrict__ root) {
  const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v < V) root[v] = parent[v] == (int32_t)v ? 1 : 0;
}

__global__ __launch_bounds__(CC_THREADS) void cc_vertex_ids_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ root_rank,
                                                                   int64_t V, int64_t K, int32_t* __restrict__ vertex_component) {
  const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int32_t r = parent[v];
  int32_t id = -1;
  if (cc_in(r, V)) {
    const int32_t k = root_rank[r];
    if (cc_in(k, K)) id = k;
  }
  vertex_component[v] = id;  // (never -1: after the labelling parent[v] is a root)
}

__global__ __launch_bounds__(CC_THREADS) void cc_face_ids_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V,
                                                                 const int32_t* __restrict__ vertex_component,
                                                                 int32_t* __restrict__ face_component) {
  const int64_t f = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (f >= F) return;
  const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  face_component[f] = (cc_in(a, V) && cc_in(b, V) && cc_in(c, V)) ? vertex_component[a] : -1;
}

// area of a face in float32, one rounded operation per step: u = b - a, w = c - a, n = u x w, 0.5 sqrt((n0 n0 + n1 n1) + n2 n2)
__global__ __launch_bounds__(CC_THREADS) void cc_areas_kernel(const float* __restrict__ positions, int64_t V,
                                                              const int32_t* __restrict__ faces, int64_t F, float* __restrict__ area) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (f >= F) return;
  const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  float out = 0.0f;
  if (cc_in(ia, V) && cc_in(ib, V) && cc_in(ic, V)) {
    float a[3], u[3], w[3];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = positions[3 * (int64_t)ia + k];
      const float bk = positions[3 * (int64_t)ib + k], ck = positions[3 * (int64_t)ic + k];
      finite = finite && xf_finite(a[k]) && xf_finite(bk) && xf_finite(ck);
      u[k] = xf_sub(bk, a[k]);
      w[k] = xf_sub(ck, a[k]);
    }
    if (finite) {
      const float n0 = xf_sub(xf_mul(u[1], w[2]), xf_mul(u[2], w[1]));
      const float n1 = xf_sub(xf_mul(u[2], w[0]), xf_mul(u[0], w[2]));
      const float n2 = xf_sub(xf_mul(u[0], w[1]), xf_mul(u[1], w[0]));
      out = xf_mul(0.5f, xf_sqrt(xf_add(xf_add(xf_mul(n0, n0), xf_mul(n1, n1)), xf_mul(n2, n2))));
    }
  }
  area[f] = out;
}

// ONE CHUNK OF 256 SORTED POSITIONS PER LANE.  A piece that opens a component's run goes to first[c], the piece that continues a run
// from the chunk before to head[chunk] (0 where the chunk opens with a new run).  Positions of id -1 (invalid faces, sorted first) are
// skipped.
__global__ __launch_bounds__(CC_THREADS) void cc_pieces_kernel(const int32_t* __restrict__ sorted_ids, const int64_t* __restrict__ order,
                                                               const float* __restrict__ area, int64_t F, int64_t K, int64_t n_chunks,
                                                               double* __restrict__ head, double* __restrict__ first) {
  const int64_t b = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (b >= n_chunks) return;
  const int64_t j0 = b * CC_THREADS, j1 = (j0 + CC_THREADS < F) ? j0 + CC_THREADS : F;
  int32_t cur = sorted_ids[j0];
  bool opens = j0 == 0 || sorted_ids[j0 - 1] != cur;
  double sum = 0.0, head_sum = 0.0;
  for (int64_t j = j0; j < j1; ++j) {
    const int32_t id = sorted_ids[j];
    if (id != cur) {
      if (opens) {
        if (cc_in(cur, K)) first[cur] = sum;
      } else {
        head_sum = sum;
      }
      cur = id, opens = true, sum = 0.0;
    }
    const int64_t f = order[j];
    sum += (uint64_t)f < (uint64_t)F ? (double)area[f] : 0.0;
  }
  if (opens) {
    if (cc_in(cur, K)) first[cur] = sum;
  } else {
    head_sum = sum;
  }
  head[b] = head_sum;
}

// first position of `sorted` [n] (ascending) that holds a value >= key
__device__ __forceinline__ int64_t cc_lower_bound(const int32_t* __restrict__ sorted, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  for (int k = 0; k < 40 && lo < hi; ++k) {  // (n < 2^31: at most 31 halvings)
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(CC_THREADS) void cc_stats_kernel(const int32_t* __restrict__ sorted_face_ids, int64_t F,
                                                              const int32_t* __restrict__ sorted_vertex_ids, int64_t V,
                                                              const double* __restrict__ head, const double* __restrict__ first, int64_t K,
                                                              int64_t* __restrict__ n_faces, int64_t* __restrict__ n_vertices,
                                                              double* __restrict__ area) {
  const int64_t c = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (c >= K) return;
  n_vertices[c] = cc_lower_bound(sorted_vertex_ids, V, c + 1) - cc_lower_bound(sorted_vertex_ids, V, c);
  const int64_t s = cc_lower_bound(sorted_face_ids, F, c), e = cc_lower_bound(sorted_face_ids, F, c + 1);
  n_faces[c] = e - s;
  double sum = 0.0;
  if (e > s) {
    sum = first[c];
    for (int64_t b = s / CC_THREADS + 1; b <= (e - 1) / CC_THREADS; ++b) sum += head[b];
  }
  area[c] = sum;
}

// face_keep[f] = the face's component is kept; the corners of a kept face are flagged in `used` (plain stores of 1, zeroed by the caller)
__global__ __launch_bounds__(CC_THREADS) void cc_mark_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ face_component,
                                                             const uint8_t* __restrict__ keep, int64_t F, int64_t V, int64_t K,
                                                             uint8_t* __restrict__ face_keep, uint8_t* __restrict__ used) {
  const int64_t f = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (f >= F) return;
  const int32_t c = face_component[f];
  const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  const bool kept = cc_in(c, K) && keep[c] != 0 && cc_in(ia, V) && cc_in(ib, V) && cc_in(ic, V);
  face_keep[f] = kept ? 1 : 0;
  if (kept) used[ia] = 1, used[ib] = 1, used[ic] = 1;  // (every writer stores the same byte)
}

__global__ __launch_bounds__(CC_THREADS) void cc_emit_faces_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_keep,
                                                                   const int32_t* __restrict__ face_rank,
                                                                   const int32_t* __restrict__ vertex_rank, int64_t F, int64_t V,
                                                                   int32_t* __restrict__ faces_out, int64_t face_cap) {
  const int64_t f = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (f >= F || !face_keep[f]) return;
  const int64_t at = face_rank[f];
  if (at < 0 || at >= face_cap) return;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int32_t i = faces[3 * f + t];
    faces_out[3 * at + t] = cc_in(i, V) ? vertex_rank[i] : -1;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_emit_vertices_kernel(const uint8_t* __restrict__ rows, int row_bytes,
                                                                      const uint8_t* __restrict__ used,
                                                                      const int32_t* __restrict__ vertex_rank, int64_t V, xf_world Wd,
                                                                      uint8_t* __restrict__ rows_out, float* __restrict__ positions_out,
                                                                      int64_t vertex_cap, int32_t* __restrict__ vertex_map) {
  const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int64_t at = used[v] ? (int64_t)vertex_rank[v] : -1;
  if (at < 0 || at >= vertex_cap) {
    vertex_map[v] = -1;
    return;
  }
  vertex_map[v] = (int32_t)at;
  const uint8_t* row = rows + v * (int64_t)row_bytes;
  uint8_t* out = rows_out + at * (int64_t)row_bytes;
  float p[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = __uint_as_float(cc_load32(row + 4 * k)), positions_out[3 * at + k] = p[k];
  if (Wd.has) {
    xf_world_apply(Wd, p, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) cc_store32(out + 4 * k, __float_as_uint(w[k]));
  } else {  // the bytes as they are (a NaN keeps its payload)
    for (int k = 0; k < 12; ++k) out[k] = row[k];
  }
  for (int k = 12; k < row_bytes; ++k) out[k] = row[k];
}

inline bool cc_blocks(int64_t n, unsigned& blocks) {
  const int64_t b = (n + CC_THREADS - 1) / CC_THREADS;
  if (b > 0x7fffffff) return false;
  blocks = (unsigned)b;
  return true;
}

inline bool cc_row_bytes_ok(int row_bytes) {
  return row_bytes == 15 || (row_bytes >= 23 && row_bytes <= 19 + 4 * CC_MAX_CLASSES && (row_bytes - 19) % 4 == 0);
}

inline bool cc_sizes_ok(int64_t V, int64_t F) { return V < (1LL << 31) && F < (1LL << 31) / 3; }

}  // namespace

#define CC_LAUNCH(kernel, n, ...)                                                                        \
  do {                                                                                                   \
    unsigned blocks_;                                                                                    \
    if (!cc_blocks((n), blocks_)) return UMHS_ERR_UNSUPPORTED;                                           \
    hipLaunchKernelGGL(kernel, dim3(blocks_), dim3(CC_THREADS), 0, umhs_s(stream), __VA_ARGS__);         \
    UMHS_CHECK_LAUNCH();                                                                                 \
  } while (0)

extern "C" int umhs_components_init(int32_t* parent, int64_t n_vertices, umhs_stream_t stream) {
  if (n_vertices < 0) return UMHS_ERR_ARG;
  if (n_vertices >= (1LL << 31)) return UMHS_ERR_UNSUPPORTED;
  if (n_vertices == 0) return UMHS_OK;
  if (!parent) return UMHS_ERR_ARG;
  CC_LAUNCH(cc_init_kernel, n_vertices, parent, n_vertices);
  return UMHS_OK;
}

extern "C" int umhs_components_rounds(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* parent, uint32_t* changed,
                                      int n_rounds, umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_rounds < 0 || n_rounds > CC_MAX_ROUNDS) return UMHS_ERR_ARG;
  if (!cc_sizes_ok(n_vertices, n_faces)) return UMHS_ERR_UNSUPPORTED;
  if (n_faces == 0 || n_vertices == 0 || n_rounds == 0) return UMHS_OK;
  if (!faces || !parent || !changed) return UMHS_ERR_ARG;
  for (int r = 0; r < n_rounds; ++r) {
    CC_LAUNCH(cc_hook_kernel, n_faces, faces, n_faces, n_vertices, parent, changed, 1u << r);
    CC_LAUNCH(cc_jump_kernel, n_vertices, n_vertices, parent, changed, 1u << r);
  }
  return UMHS_OK;
}

extern "C" int umhs_components_roots(const int32_t* parent, int64_t n_vertices, uint8_t* root, umhs_stream_t stream) {
  if (n_vertices < 0) return UMHS_ERR_ARG;
  if (n_vertices >= (1LL << 31)) return UMHS_ERR_UNSUPPORTED;
  if (n_vertices == 0) return UMHS_OK;
  if (!parent || !root) return UMHS_ERR_ARG;
  CC_LAUNCH(cc_roots_kernel, n_vertices, parent, n_vertices, root);
  return UMHS_OK;
}

extern "C" int umhs_components_ids(const int32_t* parent, const int32_t* root_rank, const int32_t* faces, int64_t n_faces,
                                   int64_t n_vertices, int64_t n_components, int32_t* vertex_component, int32_t* face_component,
                                   umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_components < 0 || n_components > n_vertices) return UMHS_ERR_ARG;
  if (!cc_sizes_ok(n_vertices, n_faces)) return UMHS_ERR_UNSUPPORTED;
  if (n_vertices > 0) {
    if (!parent || !root_rank || !vertex_component) return UMHS_ERR_ARG;
    CC_LAUNCH(cc_vertex_ids_kernel, n_vertices, parent, root_rank, n_vertices, n_components, vertex_component);
  }
  if (n_faces > 0) {
    if (!faces || !face_component || (n_vertices > 0 && !vertex_component)) return UMHS_ERR_ARG;
    CC_LAUNCH(cc_face_ids_kernel, n_faces, faces, n_faces, n_vertices, vertex_component, face_component);
  }
  return UMHS_OK;
}

extern "C" int umhs_components_areas(const float* positions, int64_t n_vertices, const int32_t* faces, int64_t n_faces, float* area,
                                     umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0) return UMHS_ERR_ARG;
  if (!cc_sizes_ok(n_vertices, n_faces)) return UMHS_ERR_UNSUPPORTED;
  if (n_faces == 0) return UMHS_OK;
  if (!faces || !area || (n_vertices > 0 && !positions)) return UMHS_ERR_ARG;
  CC_LAUNCH(cc_areas_kernel, n_faces, positions, n_vertices, faces, n_faces, area);
  return UMHS_OK;
}

extern "C" int umhs_components_stats(const int32_t* sorted_face_ids, const int64_t* face_order, const float* area, int64_t n_faces,
                                     const int32_t* sorted_vertex_ids, int64_t n_vertices, int64_t n_components, double* head,
                                     double* first, int64_t* faces_out, int64_t* vertices_out, double* area_out, umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_components < 0 || n_components > n_vertices) return UMHS_ERR_ARG;
  if (!cc_sizes_ok(n_vertices, n_faces)) return UMHS_ERR_UNSUPPORTED;
  if (n_components == 0) return UMHS_OK;
  if (!sorted_vertex_ids || !faces_out || !vertices_out || !area_out) return UMHS_ERR_ARG;
  if (n_faces > 0) {
    if (!sorted_face_ids || !face_order || !area || !head || !first) return UMHS_ERR_ARG;
    const int64_t n_chunks = (n_faces + CC_THREADS - 1) / CC_THREADS;
    CC_LAUNCH(cc_pieces_kernel, n_chunks, sorted_face_ids, face_order, area, n_faces, n_components, n_chunks, head, first);
  }
  CC_LAUNCH(cc_stats_kernel, n_components, sorted_face_ids, n_faces, sorted_vertex_ids, n_vertices, head, first, n_components, faces_out,
            vertices_out, area_out);
  return UMHS_OK;
}

extern "C" int umhs_components_mark(const int32_t* faces, const int32_t* face_component, const uint8_t* keep, int64_t n_faces,
                                    int64_t n_vertices, int64_t n_components, uint8_t* face_keep, uint8_t* used, umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || n_components < 0) return UMHS_ERR_ARG;
  if (!cc_sizes_ok(n_vertices, n_faces)) return UMHS_ERR_UNSUPPORTED;
  if (n_faces == 0) return UMHS_OK;
  if (!faces || !face_component || !face_keep || (n_components > 0 && !keep) || (n_vertices > 0 && !used)) return UMHS_ERR_ARG;
  CC_LAUNCH(cc_mark_kernel, n_faces, faces, face_component, keep, n_faces, n_vertices, n_components, face_keep, used);
  return UMHS_OK;
}

extern "C" int umhs_components_emit(const void* rows, int row_bytes, const int32_t* faces, const uint8_t* face_keep,
                                    const int32_t* face_rank, const uint8_t* used, const int32_t* vertex_rank, int64_t n_faces,
                                    int64_t n_vertices, const float* world_host12, void* rows_out, float* positions_out,
                                    int64_t vertex_cap, int32_t* faces_out, int64_t face_cap, int32_t* vertex_map, umhs_stream_t stream) {
  if (n_faces < 0 || n_vertices < 0 || vertex_cap < 0 || face_cap < 0 || !cc_row_bytes_ok(row_bytes)) return UMHS_ERR_ARG;
  if (!cc_sizes_ok(n_vertices, n_faces)) return UMHS_ERR_UNSUPPORTED;
  if (n_faces > 0 && face_cap > 0) {
    if (!faces || !face_keep || !face_rank || !faces_out || (n_vertices > 0 && !vertex_rank)) return UMHS_ERR_ARG;
    CC_LAUNCH(cc_emit_faces_kernel, n_faces, faces, face_keep, face_rank, vertex_rank, n_faces, n_vertices, faces_out, face_cap);
  }
  if (n_vertices > 0) {
    if (!rows || !used || !vertex_rank || !vertex_map || (vertex_cap > 0 && (!rows_out || !positions_out))) return UMHS_ERR_ARG;
    CC_LAUNCH(cc_emit_vertices_kernel, n_vertices, reinterpret_cast<const uint8_t*>(rows), row_bytes, used, vertex_rank, n_vertices,
              xf_world_from_host(world_host12), reinterpret_cast<uint8_t*>(rows_out), positions_out, vertex_cap, vertex_map);
  }
  return UMHS_OK;
}
