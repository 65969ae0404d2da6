// Point-cloud export (what ``ns-export pointcloud`` does for a trained model): rendered rays -> packed PLY rows, and the exact
// k-nearest-neighbour pass of statistical outlier removal over the kept points.  include/umhs_hip.h states the arithmetic as THE
// definition; tests/pointcloud_ref.py restates it in numpy.
//
// Rows.  umhs_pc_flag_count evaluates the keep rule per ray and writes one count per chunk of PC_THREADS rays; the caller scans the
// few hundred counts (exclusive) and keeps the running total of the earlier batches as a DEVICE scalar; umhs_pc_emit recomputes the
// flag, ranks the kept rays of a chunk in ray order (a ballot per wave gives the rank inside the wave, the wave totals go through LDS)
// and writes ray r's row at rows + (base + chunk_offsets[chunk] + rank) * row_bytes, its model-frame point and its ordinal beside it.
// No atomics: where a row lands is a function of the rays alone, so the file is a function of checkpoint, scene and seed.  A row index
// outside [0, cap) is never written.  Every source is read in place at its own row stride.  A row is 4 or 5 + C dwords at a 4-byte
// aligned address, stored as dwords: consecutive kept lanes write consecutive rows, i.e. one contiguous piece of memory per wave.
// The point, the box test and the world affine are one rounded float32 operation per step: the unit is compiled with contraction off
// and written with the xf_* operations of umhs_exact.h (which says why the __f*_rn intrinsics do not give that).
//
// Neighbours.  The kept points are binned into a uniform grid over their bounding box (umhs_pc_cell_keys; the sort by key and the
// cell-start table are the caller's), and umhs_knn_mean_dist is handed them IN CELL ORDER: thread i owns sorted point i, so the lanes
// of a wave sit in the same or in adjacent cells and walk the same candidates -- their loads hit the same cache lines (the candidates
// are read through the cache, nothing is staged in LDS: see DESIGN.md section 7).  A query scans its own cell, then Chebyshev rings of
// cells r = 1, 2, ...  A ring is walked row by row: with key = (z * ny + y) * nx + x the cells of a row that are adjacent in x are
// adjacent in the sorted array, so a row on the ring's top / bottom / front / back face is ONE range of points
// [start[key(x0)], start[key(x1) + 1]), and a row through its interior contributes its two end cells.
// The running k smallest squared distances live in registers: K (a template parameter) slots kept ascending by an unrolled
// compare-exchange chain -- min / max per slot, every index a compile-time constant, so nothing goes to scratch.  k < K, or fewer than
// k points, is padding: the first K - k_eff slots start at -1, below every squared distance, and stay where they are; the last slot
// is then the k_eff-th smallest, and the mean is taken over the last k_eff slots.
// Stop rule.  With f = (p - lo) / edge per axis (the arithmetic of the binning, so query and candidates agree on the cells), every point
// outside the scanned block of cells [c - r, c + r] is farther from the query than
//   b = min over the axes and both sides of  f - (c - r)  and  (c + r + 1) - f,  a side taken only where the block ends INSIDE the grid,
// in units of the edge.  The result is final once the k-th distance is <= (b - 2^-8) * edge, or once the block covers the grid.
// The 2^-8 pays for the rounding of f: no dimension exceeds 4,096 cells, so f and the candidates' f are each off by less than 2^-11.
// Points clamped into a border cell lie farther out than the cell's nominal face, never nearer, so the bound holds for ANY lo / edge
// the caller chooses: exactness does not depend on the grid, only the time does.
// Every loop is bounded by the arguments: rings <= the largest dimension, rows clipped to the grid, points per range from the table
// (clamped to [0, m]).  No loop waits on data.
#pragma clang fp contract(off)
#include "umhs_common.h"
#include "umhs_exact.h"
#include "umhs_camera.h"

#define PC_THREADS 256
#define PC_MAX_CLASSES 16
#define PC_MAX_CELLS (1LL << 21)
#define PC_MAX_DIM 4096
#define KNN_THREADS 256

// the keep rule of ray r and its model-frame point
__device__ __forceinline__ bool pc_keep(const umhs_pc_args& A, int64_t r, float p[3]) {
  const float* o = A.origins + r * (int64_t)A.origins_stride;
  const float* d = A.directions + r * (int64_t)A.directions_stride;
  const float t = A.depth[r * (int64_t)A.depth_stride];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = xf_add(xf_mul(d[k], t), o[k]);
  bool keep = A.accumulation[r * (int64_t)A.accumulation_stride] > A.threshold;  // (NaN is not greater)
#pragma unroll
  for (int k = 0; k < 3; ++k) keep = keep && xf_finite(p[k]);
  if (A.has_box) {
    const float e0 = xf_sub(p[0], A.box_center[0]), e1 = xf_sub(p[1], A.box_center[1]), e2 = xf_sub(p[2], A.box_center[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // q = R^T (p - T)
      const float q = cam_rt_row(A.box_rotation, k, e0, e1, e2);
      const float h = xf_mul(A.box_scale[k], 0.5f);
      keep = keep && (q < h) && (q > -h);
    }
  }
  return keep;
}

__global__ __launch_bounds__(PC_THREADS) void pc_flag_count_kernel(umhs_pc_args A, int64_t n_rays, int32_t* __restrict__ chunk_counts) {
  __shared__ int wave_total[PC_THREADS / UMHS_WAVE];
  const int64_t r = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
  float p[3];
  const bool keep = r < n_rays && pc_keep(A, r, p);
  const int c = __popcll(__ballot(keep));
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) chunk_counts[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
}

__global__ __launch_bounds__(PC_THREADS) void pc_emit_kernel(umhs_pc_args A, int64_t n_rays, const int64_t* __restrict__ chunk_offsets,
                                                             const int64_t* __restrict__ base, int64_t ordinal0,
                                                             uint32_t* __restrict__ rows, float* __restrict__ points,
                                                             int64_t* __restrict__ kept, int64_t cap) {
  __shared__ int wave_total[PC_THREADS / UMHS_WAVE];
  const int64_t r = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float p[3];
  const bool keep = r < n_rays && pc_keep(A, r, p);
  const unsigned long long ballot = __ballot(keep);
  if (lane == 0) wave_total[wave] = __popcll(ballot);
  __syncthreads();
  int rank = __popcll(ballot & ((1ull << lane) - 1ull));  // kept lanes below this one: lane order is ray order
#pragma unroll
  for (int k = 0; k < PC_THREADS / UMHS_WAVE - 1; ++k) rank += (k < wave) ? wave_total[k] : 0;
  if (!keep) return;
  const int64_t at = base[0] + chunk_offsets[blockIdx.x] + rank;
  if (at < 0 || at >= cap) return;  // the surplus of the last batch, and offsets that do not fit: never written
  const int C = A.n_classes;
  uint32_t* row = rows + at * (int64_t)(C > 0 ? 5 + C : 4);
  float w[3] = {p[0], p[1], p[2]};
  if (A.has_world) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      w[i] = xf_add(xf_add(xf_add(xf_mul(A.world[4 * i], p[0]), xf_mul(A.world[4 * i + 1], p[1])), xf_mul(A.world[4 * i + 2], p[2])),
                     A.world[4 * i + 3]);
  }
  const float* c = A.rgb + r * (int64_t)A.rgb_stride;
  row[0] = __float_as_uint(w[0]), row[1] = __float_as_uint(w[1]), row[2] = __float_as_uint(w[2]);
  row[3] = xf_byte(c[0]) | (xf_byte(c[1]) << 8) | (xf_byte(c[2]) << 16) | (xf_byte(A.accumulation[r * (int64_t)A.accumulation_stride]) << 24);
  if (C > 0) {
    const float* sp = A.seg_probs + r * (int64_t)A.seg_probs_stride;
    const float* ab = A.abundances + r * (int64_t)A.abundances_stride;
    float mx = -INFINITY;
    int arg = 0;
    for (int k = 0; k < C; ++k) {  // the first of the largest, as umhs_ray_epilogue_fwd picks seg_raw; a NaN never wins
      const float v = sp[k];
      if (v > mx) mx = v, arg = k;
    }
    row[4] = (uint32_t)arg;
    for (int k = 0; k < C; ++k) row[5 + k] = __float_as_uint(ab[k]);
  }
  points[3 * at] = p[0], points[3 * at + 1] = p[1], points[3 * at + 2] = p[2];
  kept[at] = ordinal0 + r;
}

extern "C" int64_t umhs_pc_chunks(int64_t n_rays) { return n_rays < 1 ? 0 : (n_rays + PC_THREADS - 1) / PC_THREADS; }

static int pc_check(const umhs_pc_args* a, int64_t n_rays) {
  if (!a || n_rays < 0) return UMHS_ERR_ARG;
  if (!a->origins || !a->directions || !a->depth || !a->accumulation || !a->rgb) return UMHS_ERR_ARG;
  if (a->n_classes < 0 || (a->n_classes > 0 && (!a->abundances || !a->seg_probs))) return UMHS_ERR_ARG;
  if (a->origins_stride < 3 || a->directions_stride < 3 || a->depth_stride < 1 || a->accumulation_stride < 1 || a->rgb_stride < 3)
    return UMHS_ERR_ARG;
  if (a->n_classes > 0 && (a->abundances_stride < a->n_classes || a->seg_probs_stride < a->n_classes)) return UMHS_ERR_ARG;
  if (a->n_classes > PC_MAX_CLASSES || umhs_pc_chunks(n_rays) > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;
  return UMHS_OK;
}

extern "C" int umhs_pc_flag_count(const umhs_pc_args* args, int64_t n_rays, int32_t* chunk_counts, umhs_stream_t stream) {
  const int rc = pc_check(args, n_rays);
  if (rc != UMHS_OK) return rc;
  if (n_rays == 0) return UMHS_OK;
  if (!chunk_counts) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(pc_flag_count_kernel, dim3((unsigned)umhs_pc_chunks(n_rays)), dim3(PC_THREADS), 0, umhs_s(stream), *args, n_rays,
                     chunk_counts);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_pc_emit(const umhs_pc_args* args, int64_t n_rays, const int64_t* chunk_offsets, const int64_t* base,
                            int64_t ordinal0, void* rows, float* points, int64_t* kept, int64_t cap, umhs_stream_t stream) {
  const int rc = pc_check(args, n_rays);
  if (rc != UMHS_OK) return rc;
  if (cap < 0) return UMHS_ERR_ARG;
  if (n_rays == 0) return UMHS_OK;
  if (!chunk_offsets || !base || !rows || !points || !kept || ((uintptr_t)rows & 3)) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(pc_emit_kernel, dim3((unsigned)umhs_pc_chunks(n_rays)), dim3(PC_THREADS), 0, umhs_s(stream), *args, n_rays,
                     chunk_offsets, base, ordinal0, reinterpret_cast<uint32_t*>(rows), points, kept, cap);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------------
struct pc_grid {
  float lo[3], edge;
  int dim[3];
};

// cell coordinate of one axis and f = (x - lo) / edge; anything below the grid (and a NaN) goes to cell 0, anything above to the last
__device__ __forceinline__ int pc_cell(float x, float lo, float edge, int dim, float& f) {
  f = xf_div(xf_sub(x, lo), edge);
  if (!(f >= 0.0f)) return 0;
  return f < (float)dim ? (int)f : dim - 1;
}

__global__ __launch_bounds__(256) void pc_cell_keys_kernel(const float* __restrict__ points, int64_t m, pc_grid g, int32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  float f;
  const int cx = pc_cell(points[3 * i], g.lo[0], g.edge, g.dim[0], f);
  const int cy = pc_cell(points[3 * i + 1], g.lo[1], g.edge, g.dim[1], f);
  const int cz = pc_cell(points[3 * i + 2], g.lo[2], g.edge, g.dim[2], f);
  keys[i] = (cz * g.dim[1] + cy) * g.dim[0] + cx;
}

static int pc_grid_check(const float* lo3, float edge, const int32_t* dims3, pc_grid& g) {
  if (!lo3 || !dims3 || !(edge > 0.0f) || !xf_finite(edge)) return UMHS_ERR_ARG;
  int64_t cells = 1;
  for (int k = 0; k < 3; ++k) {
    if (dims3[k] < 1 || !xf_finite(lo3[k])) return UMHS_ERR_ARG;
    if (dims3[k] > PC_MAX_DIM) return UMHS_ERR_UNSUPPORTED;
    cells *= dims3[k];
    g.lo[k] = lo3[k], g.dim[k] = dims3[k];
  }
  g.edge = edge;
  return cells > PC_MAX_CELLS ? UMHS_ERR_UNSUPPORTED : UMHS_OK;
}

extern "C" int umhs_pc_cell_keys(const float* points, int64_t m, const float* lo_host3, float edge, const int32_t* dims_host3,
                                 int32_t* keys, umhs_stream_t stream) {
  pc_grid g;
  if (m < 0) return UMHS_ERR_ARG;
  const int rc = pc_grid_check(lo_host3, edge, dims_host3, g);
  if (rc != UMHS_OK) return rc;
  if (m == 0) return UMHS_OK;
  if (!points || !keys) return UMHS_ERR_ARG;
  if ((m + 255) / 256 > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pc_cell_keys_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, umhs_s(stream), points, m, g, keys);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// ---- k nearest neighbours ---------------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void knn_scan(const float* __restrict__ pts, int a, int b, float qx, float qy, float qz, float (&t)[K]) {
  for (int j = a; j < b; ++j) {
    const float dx = xf_sub(pts[3 * j], qx), dy = xf_sub(pts[3 * j + 1], qy), dz = xf_sub(pts[3 * j + 2], qz);
    float d = xf_add(xf_add(xf_mul(dx, dx), xf_mul(dy, dy)), xf_mul(dz, dz));
    if (d < t[K - 1]) {  // (a NaN distance is never taken)
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const float lo = fminf(t[i], d);
        d = fmaxf(t[i], d);
        t[i] = lo;
      }
    }
  }
}

template <int K>
__global__ __launch_bounds__(KNN_THREADS) void knn_mean_dist_kernel(const float* __restrict__ pts, int m, const int32_t* __restrict__ cell_start,
                                                                    pc_grid g, int k, float* __restrict__ mean) {
  const int i = blockIdx.x * KNN_THREADS + threadIdx.x;
  if (i >= m) return;
  const int k_eff = k < m ? k : m, pad = K - k_eff;
  float t[K];
#pragma unroll
  for (int s = 0; s < K; ++s) t[s] = s < pad ? -1.0f : INFINITY;
  const float qx = pts[3 * i], qy = pts[3 * i + 1], qz = pts[3 * i + 2];
  float f[3];
  const int cx = pc_cell(qx, g.lo[0], g.edge, g.dim[0], f[0]);
  const int cy = pc_cell(qy, g.lo[1], g.edge, g.dim[1], f[1]);
  const int cz = pc_cell(qz, g.lo[2], g.edge, g.dim[2], f[2]);
  const int c[3] = {cx, cy, cz};
  const int nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
  const int r_max = max(nx, max(ny, nz)) - 1;  // at r_max the block covers the grid from any cell
  for (int r = 0; r <= r_max; ++r) {
    const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
    const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * ny + y) * nx;
        const bool face = (z - cz == r) || (cz - z == r) || (y - cy == r) || (cy - y == r);
        if (face) {  // the whole run of cells of this row is on the ring: one range of the sorted points
          const int a = min(max(cell_start[row + x0], 0), m), b = min(max(cell_start[row + x1 + 1], 0), m);
          knn_scan<K>(pts, a, b, qx, qy, qz, t);
        } else {  // its two ends only (r >= 1 here)
          if (cx - r >= 0) {
            const int a = min(max(cell_start[row + cx - r], 0), m), b = min(max(cell_start[row + cx - r + 1], 0), m);
            knn_scan<K>(pts, a, b, qx, qy, qz, t);
          }
          if (cx + r < nx) {
            const int a = min(max(cell_start[row + cx + r], 0), m), b = min(max(cell_start[row + cx + r + 1], 0), m);
            knn_scan<K>(pts, a, b, qx, qy, qz, t);
          }
        }
      }
    }
    // everything outside the block [c - r, c + r] is farther than bound * edge
    float bound = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (c[a] - r > 0) bound = fminf(bound, xf_sub(f[a], (float)(c[a] - r)));
      if (c[a] + r + 1 < g.dim[a]) bound = fminf(bound, xf_sub((float)(c[a] + r + 1), f[a]));
    }
    if (bound == INFINITY) break;  // the block covers the grid
    bound = xf_mul(xf_sub(bound, 0.00390625f), g.edge);
    if (bound > 0.0f && t[K - 1] <= xf_mul(bound, bound)) break;
  }
  float sum = 0.0f;
#pragma unroll
  for (int s = 0; s < K; ++s)
    if (s >= pad) sum = xf_add(sum, sqrtf(t[s]));  // ascending; sqrtf is correctly rounded
  mean[i] = xf_div(sum, (float)k_eff);
}

extern "C" int umhs_knn_mean_dist(const float* sorted_points, int64_t m, const int32_t* cell_start, const float* lo_host3, float edge,
                                  const int32_t* dims_host3, int k, float* mean, umhs_stream_t stream) {
  pc_grid g;
  if (m < 0 || k < 2) return UMHS_ERR_ARG;
  if (k > 32) return UMHS_ERR_UNSUPPORTED;
  const int rc = pc_grid_check(lo_host3, edge, dims_host3, g);
  if (rc != UMHS_OK) return rc;
  if (m == 0) return UMHS_OK;
  if (!sorted_points || !cell_start || !mean) return UMHS_ERR_ARG;
  if (m > 0x7fffffffLL / 4) return UMHS_ERR_UNSUPPORTED;  // 3 * j is an int
  const dim3 grid((unsigned)((m + KNN_THREADS - 1) / KNN_THREADS)), block(KNN_THREADS);
  if (k == 20)
    hipLaunchKernelGGL(knn_mean_dist_kernel<20>, grid, block, 0, umhs_s(stream), sorted_points, (int)m, cell_start, g, k, mean);
  else
    hipLaunchKernelGGL(knn_mean_dist_kernel<32>, grid, block, 0, umhs_s(stream), sorted_points, (int)m, cell_start, g, k, mean);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
