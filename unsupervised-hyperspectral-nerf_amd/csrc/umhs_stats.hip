// Per-segment statistics of a flat float32 buffer (the trainer's --log-gradients: one pass over flat.grad instead of a .norm() and a
// host read per named parameter).  Segment k = elements [bounds[k], bounds[k+1]); per segment, in float64: the sum of x^2 and the
// maximum of |x| over the finite elements, and the number of non-finite ones.  Contract and arithmetic: include/umhs_hip.h.
//
// Partition (fixed by n, K and bounds alone, so the same input gives the same bits on every launch):
//   tile      ST_TILE = 8192 consecutive elements of ONE segment, counted from the segment's start (the last tile of a segment is
//             short; no tile straddles a boundary).  Global tile index = tiles of the earlier segments + index inside the segment.
//   workgroup 256 threads.  A tile starts at any element offset: the elements up to the first 16-byte boundary (at most 3) go one each
//             to threads 0..2, then thread t takes the 16-byte pieces t, t + 256, ... (at most 8, four elements each, in order), and
//             the at most 3 elements behind the last whole piece go one each to threads 0..2.  A thread's chain: <= 1 + 32 + 1 additions.
//   wave      __shfl_down tree, 6 levels; the four waves' sums are added in order, 3 additions.  The partial goes to the workspace.
//   finish    one wave per segment: lane l adds partials l, l + 64, ... of its segment in index order, then the same 6-level tree.
// Longest chain of additions an element passes through: 34 + 6 + 3 + ceil(ceil(len / 8192) / 64) + 6 (tests/stats_f64.py).
// x^2 of a float32 is exact in float64, so a contracted fma changes nothing.  No atomics, no allocation, no synchronisation.
#include "umhs_common.h"

constexpr int ST_THREADS = 256, ST_PIECES = 8;
constexpr int64_t ST_TILE = (int64_t)ST_THREADS * 4 * ST_PIECES;  // 8192 elements = 32 KiB
constexpr int ST_MAX_BLOCKS = 2048;                               // 8 workgroups per CU keep the loads of 256 CUs in flight

struct st_acc {
  double s;
  float m;
  int c;
};

__device__ __forceinline__ void st_add(st_acc& a, float v) {
  if ((__float_as_uint(v) & 0x7f800000u) != 0x7f800000u) {  // finite (the exponent of NaN and +-Inf is all ones)
    const double d = (double)v;
    a.s += d * d;
    a.m = fmaxf(a.m, fabsf(v));
  } else {
    ++a.c;
  }
}

// clamped segment k of a bounds array the host has validated: a stale device copy can still never address outside [0, n)
__device__ __forceinline__ void st_segment(const int64_t* __restrict__ bounds, int k, int64_t n, int64_t& lo, int64_t& hi) {
  lo = bounds[k], hi = bounds[k + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
}

__device__ __forceinline__ int64_t st_tiles(int64_t lo, int64_t hi) { return (hi - lo + ST_TILE - 1) / ST_TILE; }

__device__ __forceinline__ void st_wave_reduce(st_acc& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.s += __shfl_down(a.s, o);
    a.m = fmaxf(a.m, __shfl_down(a.m, o));
    a.c += __shfl_down(a.c, o);
  }
}

__global__ __launch_bounds__(ST_THREADS) void segment_stats_tiles_kernel(const float* __restrict__ x, int64_t n,
                                                                         const int64_t* __restrict__ bounds, int K,
                                                                         double* __restrict__ partial) {
  __shared__ double sm_s[4];
  __shared__ float sm_m[4];
  __shared__ int sm_c[4];
  const int tid = threadIdx.x;
  int k = 0;
  int64_t first = 0, lo, hi;  // first: global index of segment k's first tile
  st_segment(bounds, 0, n, lo, hi);
  int64_t nt = st_tiles(lo, hi);
  for (int64_t t = blockIdx.x;; t += gridDim.x) {  // (everything that steers this loop is uniform over the workgroup)
    while (k < K && t >= first + nt) {
      first += nt;
      if (++k < K) {
        st_segment(bounds, k, n, lo, hi);
        nt = st_tiles(lo, hi);
      }
    }
    if (k >= K) break;
    const int64_t a = lo + (t - first) * ST_TILE;
    const int64_t len = (hi - a < ST_TILE) ? hi - a : ST_TILE;
    const float* p = x + a;
    const int mis = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);  // float32 elements are 4-byte aligned
    int head = (4 - mis) & 3;
    if (head > len) head = (int)len;
    const int nv = (int)((len - head) >> 2), tail = (int)(len - head) - 4 * nv;
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    st_acc acc = {0.0, 0.0f, 0};
    float4 v[ST_PIECES];
#pragma unroll
    for (int i = 0; i < ST_PIECES; ++i)
      if (tid + ST_THREADS * i < nv) v[i] = p4[tid + ST_THREADS * i];
    if (tid < head) st_add(acc, p[tid]);
#pragma unroll
    for (int i = 0; i < ST_PIECES; ++i)
      if (tid + ST_THREADS * i < nv) st_add(acc, v[i].x), st_add(acc, v[i].y), st_add(acc, v[i].z), st_add(acc, v[i].w);
    if (tid < tail) st_add(acc, p[head + 4 * nv + tid]);
    st_wave_reduce(acc);
    __syncthreads();  // the previous tile's reads of sm_* are done
    if ((tid & 63) == 0) sm_s[tid >> 6] = acc.s, sm_m[tid >> 6] = acc.m, sm_c[tid >> 6] = acc.c;
    __syncthreads();
    if (tid == 0) {
      partial[3 * t] = ((sm_s[0] + sm_s[1]) + sm_s[2]) + sm_s[3];
      partial[3 * t + 1] = (double)fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
      partial[3 * t + 2] = (double)(sm_c[0] + sm_c[1] + sm_c[2] + sm_c[3]);
    }
  }
}

__global__ __launch_bounds__(64) void segment_stats_finish_kernel(int64_t n, const int64_t* __restrict__ bounds, int K,
                                                                  const double* __restrict__ partial, double* __restrict__ out) {
  const int k = blockIdx.x, lane = threadIdx.x;
  int64_t first = 0, lo, hi;
  for (int j = 0; j < k; ++j) {
    st_segment(bounds, j, n, lo, hi);
    first += st_tiles(lo, hi);
  }
  st_segment(bounds, k, n, lo, hi);
  const int64_t nt = st_tiles(lo, hi);
  double s = 0.0, m = 0.0, c = 0.0;  // (counts are whole numbers far below 2^53: exact in float64)
  for (int64_t i = lane; i < nt; i += 64) {
    const double* q = partial + 3 * (first + i);
    s += q[0], m = fmax(m, q[1]), c += q[2];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o), m = fmax(m, __shfl_down(m, o)), c += __shfl_down(c, o);
  if (lane == 0) out[3 * k] = s, out[3 * k + 1] = m, out[3 * k + 2] = c;
}

static int64_t st_max_tiles(int64_t n, int64_t K) { return (n + ST_TILE - 1) / ST_TILE + K; }  // every segment ends in <= 1 short tile

extern "C" size_t umhs_segment_stats_workspace_bytes(int64_t n, int n_segments) {
  if (n < 0 || n_segments < 1) return 0;
  return (size_t)st_max_tiles(n, n_segments) * 3 * sizeof(double);
}

extern "C" int umhs_segment_stats_tile(void) { return (int)ST_TILE; }

extern "C" int umhs_segment_stats(const float* x, int64_t n, const int64_t* bounds, const int64_t* bounds_host, int n_segments,
                                  double* out, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n < 0 || n_segments < 1 || !bounds || !bounds_host || !out || (!x && n > 0)) return UMHS_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(x) & 3) != 0) return UMHS_ERR_ARG;
  if (bounds_host[0] < 0 || bounds_host[n_segments] > n) return UMHS_ERR_ARG;  // would read outside the buffer
  for (int k = 0; k < n_segments; ++k)
    if (bounds_host[k + 1] < bounds_host[k]) return UMHS_ERR_ARG;  // descending
  if (!workspace || workspace_bytes < umhs_segment_stats_workspace_bytes(n, n_segments)) return UMHS_ERR_WORKSPACE;
  int64_t tiles = 0;
  for (int k = 0; k < n_segments; ++k) tiles += (bounds_host[k + 1] - bounds_host[k] + ST_TILE - 1) / ST_TILE;
  if (tiles > 0) {
    const unsigned grid = (unsigned)(tiles < ST_MAX_BLOCKS ? tiles : ST_MAX_BLOCKS);
    hipLaunchKernelGGL(segment_stats_tiles_kernel, dim3(grid), dim3(ST_THREADS), 0, umhs_s(stream), x, n, bounds, n_segments,
                       static_cast<double*>(workspace));
    UMHS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(segment_stats_finish_kernel, dim3((unsigned)n_segments), dim3(64), 0, umhs_s(stream), n, bounds, n_segments,
                     static_cast<const double*>(workspace), out);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
