// Material edits inside a box or a sphere (include/umhs_hip.h, "Regional material edits"): the memory-bound passes a regional edit
// adds to a global one.  None touches the field kernels: umhs_field_heads_fwd takes (ray_indices, packed_info) as a partition of the
// sample stream into contiguous runs and forms one set of sums per run, so it is handed the SEGMENT partition built here (maximal
// runs of one ray's samples in one region) and returns the sums split by region in its single pass.
//
//   region_classify_kernel       ONE SAMPLE PER LANE.  A block's 256 positions are one contiguous run of 768 floats: loaded lane after
//                                lane into LDS, then each lane walks the region table (a kernel argument: uniform, scalar loads) in
//                                file order.  Exact float32: the box rule is pc_keep's (umhs_pointcloud.hip), every step one xf_*.
//   region_head_count_kernel     head flag of every sample (first of its ray, or another region than its predecessor), ballot per
//   region_block_scan_kernel     wave, count per block of 256; ONE block then scans the block counts in order (1,024 per round, an
//   region_emit_kernel           int64 carry between rounds) and leaves the total S; the emit pass recomputes the flags and ranks
//   region_finish_kernel         them (ballot below the lane + waves below + block offset): segment id, first sample and layer;
//                                the finish pass forms the counts and the per-ray (first segment, number).  Integers only, no atomics.
//   material_sigma_regions_kernel  material_sigma_kernel with the gain row of the sample's layer (the table, <= 135 floats, in LDS).
//   segment_sum_kernel           LANES ALONG k.  Persistent blocks over tiles of 32 rays (one contiguous run of 32 k outputs); a lane
//                                adds its ray's segment rows in segment order.
//   material_remix_regions_*     LANES ALONG BANDS, tiles of 32 rays, persistent blocks.  Per (ray, band): for each segment in order
//                                the fmaf chain of material_remix against the dictionary of the segment's layer, then one rounded
//                                add.  As many whole layers as fit REGION_LDS_BYTES are staged in LDS, the others are read through
//                                the cache; 16-byte pieces when B % 4 == 0 and every row array is aligned, else one float per lane.
//                                Every form evaluates the same chain per element: the same bits.
#pragma clang fp contract(off)
#include "umhs_common.h"
#include "umhs_exact.h"
#include "umhs_camera.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_SCAN_THREADS = 1024;
constexpr int RG_RAYS = 32;                 // rays per tile of the per-ray kernels
constexpr size_t REGION_LDS_BYTES = 48 << 10;  // dictionaries staged per block (three resident blocks per CU)

struct region_table {
  float rec[UMHS_MAX_REGIONS][16];  // T[3], R[9] row-major, S[3] (sphere: radius in S[0]), kind (0 box, 1 sphere)
};

__global__ __launch_bounds__(RG_THREADS) void region_classify_kernel(const float* __restrict__ wpos, int64_t n, region_table T, int K,
                                                                     uint8_t* __restrict__ region) {
  __shared__ float sP[RG_THREADS * 3];
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * RG_THREADS;
  const int64_t rows = n - first < RG_THREADS ? n - first : RG_THREADS;
  const int count = (int)rows * 3;
  const float* src = wpos + first * 3;
  for (int k = tid; k < count; k += RG_THREADS) sP[k] = src[k];
  __syncthreads();
  if (tid >= rows) return;
  const float p0 = sP[3 * tid], p1 = sP[3 * tid + 1], p2 = sP[3 * tid + 2];
  int id = 0;
  for (int k = 0; k < K && id == 0; ++k) {
    const float* r = T.rec[k];
    const float e0 = xf_sub(p0, r[0]), e1 = xf_sub(p1, r[1]), e2 = xf_sub(p2, r[2]);
    bool in = true;
    if (r[15] != 0.0f) {  // sphere.  (A NaN compares false everywhere below: in no region.)
      in = xf_add(xf_add(xf_mul(e0, e0), xf_mul(e1, e1)), xf_mul(e2, e2)) < xf_mul(r[12], r[12]);
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) {  // q = R^T (p - T)
        const float q = cam_rt_row(r + 3, a, e0, e1, e2);
        const float h = xf_mul(r[12 + a], 0.5f);
        in = in && (q < h) && (q > -h);
      }
    }
    if (in) id = k + 1;
  }
  region[first + tid] = (uint8_t)id;
}

// sample i starts a segment: the first sample of all, another ray than its predecessor, or another region
__device__ __forceinline__ bool region_head(const uint8_t* __restrict__ region, const int64_t* __restrict__ ray_of, int64_t i, int64_t n) {
  if (i >= n) return false;
  if (i == 0) return true;
  return ray_of[i] != ray_of[i - 1] || region[i] != region[i - 1];
}

__global__ __launch_bounds__(RG_THREADS) void region_head_count_kernel(const uint8_t* __restrict__ region,
                                                                       const int64_t* __restrict__ ray_of, int64_t n,
                                                                       int32_t* __restrict__ block_counts) {
  __shared__ int wave_total[RG_THREADS / UMHS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
  const int c = __popcll(__ballot(region_head(region, ray_of, i, n)));
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
}

// one block: exclusive offsets of the block counts, in order, and the total
__global__ __launch_bounds__(RG_SCAN_THREADS) void region_block_scan_kernel(const int32_t* __restrict__ counts, int64_t nb,
                                                                            int64_t* __restrict__ offsets, int64_t* __restrict__ total) {
  __shared__ int wave_total[RG_SCAN_THREADS / UMHS_WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < nb; base += RG_SCAN_THREADS) {  // (nb is uniform: every lane takes every round and both barriers)
    const int64_t i = base + tid;
    const int v = i < nb ? counts[i] : 0;
    int inc = v;  // a round holds at most 1,024 * 256 heads
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < RG_SCAN_THREADS / UMHS_WAVE; ++k) {
      const int t = wave_total[k];
      before += k < wave ? t : 0, all += t;
    }
    if (i < nb) offsets[i] = carry + before + (inc - v);
    carry += all;
    __syncthreads();  // wave_total is rewritten by the next round
  }
  if (tid == 0) total[0] = carry;
}

__global__ __launch_bounds__(RG_THREADS) void region_emit_kernel(const uint8_t* __restrict__ region, const int64_t* __restrict__ ray_of,
                                                                 int64_t n, const int64_t* __restrict__ block_offsets,
                                                                 int64_t* __restrict__ seg_of, int64_t* __restrict__ seg_info,
                                                                 int32_t* __restrict__ seg_layer) {
  __shared__ int wave_total[RG_THREADS / UMHS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool head = region_head(region, ray_of, i, n);
  const unsigned long long ballot = __ballot(head);
  if (lane == 0) wave_total[wave] = __popcll(ballot);
  __syncthreads();
  int upto = __popcll(ballot & ((2ull << lane) - 1ull));  // heads at or below this lane: lane order is sample order
#pragma unroll
  for (int k = 0; k < RG_THREADS / UMHS_WAVE - 1; ++k) upto += (k < wave) ? wave_total[k] : 0;
  if (i >= n) return;
  const int64_t id = block_offsets[blockIdx.x] + upto - 1;  // (sample 0 is a head: upto >= 1 everywhere; id < S <= n)
  seg_of[i] = id;
  if (head) seg_info[2 * id] = i, seg_layer[id] = (int32_t)region[i];
}

__global__ __launch_bounds__(RG_THREADS) void region_finish_kernel(const int64_t* __restrict__ seg_of, const int64_t* __restrict__ pinfo,
                                                                   int64_t n, int64_t R, const int64_t* __restrict__ total,
                                                                   int64_t* seg_info, int64_t* __restrict__ ray_seg) {
  const int64_t i = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
  const int64_t S = total[0];
  if (i < S) {  // (S <= n; reads first samples, writes counts: disjoint elements)
    const int64_t next = i + 1 < S ? seg_info[2 * (i + 1)] : n;
    seg_info[2 * i + 1] = next - seg_info[2 * i];
  }
  if (i < R) {
    int64_t s0 = pinfo[2 * i], cnt = pinfo[2 * i + 1];
    s0 = s0 < 0 ? 0 : (s0 > n ? n : s0);
    cnt = cnt < 0 ? 0 : (cnt > n - s0 ? n - s0 : cnt);
    const int64_t first = s0 < n ? seg_of[s0] : S;  // the segments that start before the ray's first sample
    ray_seg[2 * i] = first;
    ray_seg[2 * i + 1] = cnt > 0 ? seg_of[s0 + cnt - 1] - first + 1 : 0;
  }
}

__global__ __launch_bounds__(RG_THREADS) void material_sigma_regions_kernel(const float* sigma, const float* __restrict__ abund,
                                                                            const uint8_t* __restrict__ region,
                                                                            const float* __restrict__ gain, int64_t n, int C, int K,
                                                                            float* sigma_out) {
  extern __shared__ float sA[];  // [256][C] the block's rows as they lie in memory, then [(K+1)][C] gains
  float* sG = sA + RG_THREADS * C;
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * RG_THREADS;
  const int64_t rows = n - first < RG_THREADS ? n - first : RG_THREADS;
  const int count = (int)rows * C;
  const float* src = abund + first * C;
  for (int k = tid; k < count; k += RG_THREADS) sA[k] = src[k];
  for (int k = tid; k < (K + 1) * C; k += RG_THREADS) sG[k] = gain[k];
  __syncthreads();
  if (tid >= rows) return;
  int layer = region[first + tid];
  layer = layer > K ? 0 : layer;  // (ids above K are not made by umhs_region_classify; they never index past the table)
  const float* g = sG + layer * C;
  float acc = 0.0f;
  for (int c = 0; c < C; ++c) acc = fmaf(g[c] - 1.0f, sA[tid * C + c], acc);
  sigma_out[first + tid] = sigma[first + tid] * fmaxf(0.0f, 1.0f + acc);
}

// a ray's (first segment, number of segments) clamped into the S rows that exist
__device__ __forceinline__ void ray_segments(const int64_t* __restrict__ ray_seg, int64_t r, int64_t S, int64_t& j0, int64_t& nj) {
  j0 = ray_seg[2 * r], nj = ray_seg[2 * r + 1];
  j0 = j0 < 0 ? 0 : (j0 > S ? S : j0);
  nj = nj < 0 ? 0 : (nj > S - j0 ? S - j0 : nj);
}

__global__ __launch_bounds__(RG_THREADS) void segment_sum_kernel(const float* __restrict__ values, const int64_t* __restrict__ ray_seg,
                                                                 int64_t S, int64_t R, int k, float* __restrict__ out) {
  const int64_t tiles = (R + RG_RAYS - 1) / RG_RAYS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * RG_RAYS;
    const int nr = R - r0 < RG_RAYS ? (int)(R - r0) : RG_RAYS;
    for (int q = threadIdx.x; q < nr * k; q += RG_THREADS) {
      const int r = q / k, col = q - r * k;
      int64_t j0, nj;
      ray_segments(ray_seg, r0 + r, S, j0, nj);
      float acc = 0.0f;
      if (nj > 0) acc = values[j0 * k + col];  // the first row as it is
      for (int64_t j = 1; j < nj; ++j) acc += values[(j0 + j) * k + col];
      out[r0 * k + q] = acc;
    }
  }
}

// V = 4: B % 4 == 0 and every row array 16-byte aligned (a piece never straddles two rows); V = 1: any B, any alignment.  The inputs
// have S rows and the outputs R: they are distinct arrays (checked on the host), unlike material_remix's specular.
template <int V>
__global__ __launch_bounds__(RG_THREADS) void material_remix_regions_kernel(
    const float* __restrict__ mix16, const float* __restrict__ comp_specular, const int32_t* __restrict__ seg_layer,
    const int64_t* __restrict__ ray_seg, const float* __restrict__ E, const float* __restrict__ sgain, int64_t S, int64_t R, int B, int C,
    int K, int staged, float* __restrict__ spectral, float* __restrict__ spectral2, float* __restrict__ specular) {
  extern __shared__ __align__(16) float sE[];  // [staged][C][B]
  const int CB = C * B;
  for (int k = threadIdx.x; k < staged * CB; k += RG_THREADS) sE[k] = E[k];
  __syncthreads();
  const int per_row = B / V;
  const int64_t tiles = (R + RG_RAYS - 1) / RG_RAYS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * RG_RAYS;
    const int nr = R - r0 < RG_RAYS ? (int)(R - r0) : RG_RAYS;
    for (int q = threadIdx.x; q < nr * per_row; q += RG_THREADS) {
      const int r = q / per_row, b = (q - r * per_row) * V;
      int64_t j0, nj;
      ray_segments(ray_seg, r0 + r, S, j0, nj);
      float mix[V], spc[V];
#pragma unroll
      for (int v = 0; v < V; ++v) mix[v] = 0.0f, spc[v] = 0.0f;
      for (int64_t j = 0; j < nj; ++j) {
        const int64_t seg = j0 + j;
        int layer = seg_layer[seg];
        layer = (layer < 0 || layer > K) ? 0 : layer;
        const float* m = mix16 + seg * 16;
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0f;
        if (layer < staged) {
          const float* e = sE + layer * CB + b;
          for (int c = 0; c < C; ++c) {
            const float mc = m[c];
            if constexpr (V == 4) {
              const float4 e4 = *reinterpret_cast<const float4*>(e + c * B);
              acc[0] = fmaf(mc, e4.x, acc[0]), acc[1] = fmaf(mc, e4.y, acc[1]), acc[2] = fmaf(mc, e4.z, acc[2]),
              acc[3] = fmaf(mc, e4.w, acc[3]);
            } else {
              acc[0] = fmaf(mc, e[c * B], acc[0]);
            }
          }
        } else {
          const float* e = E + (int64_t)layer * CB + b;
          for (int c = 0; c < C; ++c) {
            const float mc = m[c];
            if constexpr (V == 4) {
              const float4 e4 = *reinterpret_cast<const float4*>(e + c * B);
              acc[0] = fmaf(mc, e4.x, acc[0]), acc[1] = fmaf(mc, e4.y, acc[1]), acc[2] = fmaf(mc, e4.z, acc[2]),
              acc[3] = fmaf(mc, e4.w, acc[3]);
            } else {
              acc[0] = fmaf(mc, e[c * B], acc[0]);
            }
          }
        }
        float sp[V];
#pragma unroll
        for (int v = 0; v < V; ++v) sp[v] = 0.0f;
        if (comp_specular) {
          const float s = sgain[layer];
          const float* in = comp_specular + seg * B + b;
          if constexpr (V == 4) {
            const float4 v4 = *reinterpret_cast<const float4*>(in);
            sp[0] = s * v4.x, sp[1] = s * v4.y, sp[2] = s * v4.z, sp[3] = s * v4.w;
          } else {
            sp[0] = s * in[0];
          }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {  // the first segment as it is, every later one a rounded add
          mix[v] = j == 0 ? acc[v] : mix[v] + acc[v];
          spc[v] = j == 0 ? sp[v] : spc[v] + sp[v];
        }
      }
      const int64_t at = (r0 + r) * B + b;
      if constexpr (V == 4) {
        if (comp_specular) {
          *reinterpret_cast<float4*>(specular + at) = make_float4(spc[0], spc[1], spc[2], spc[3]);
          *reinterpret_cast<float4*>(spectral2 + at) = make_float4(mix[0], mix[1], mix[2], mix[3]);
          *reinterpret_cast<float4*>(spectral + at) =
              make_float4(mix[0] + spc[0], mix[1] + spc[1], mix[2] + spc[2], mix[3] + spc[3]);
        } else {
          *reinterpret_cast<float4*>(spectral + at) = make_float4(mix[0], mix[1], mix[2], mix[3]);
        }
      } else {
        if (comp_specular) {
          specular[at] = spc[0], spectral2[at] = mix[0], spectral[at] = mix[0] + spc[0];
        } else {
          spectral[at] = mix[0];
        }
      }
    }
  }
}

inline unsigned tile_grid(int64_t R) {
  const int64_t tiles = (R + RG_RAYS - 1) / RG_RAYS;
  return (unsigned)(tiles < 2048 ? tiles : 2048);
}

}  // namespace

extern "C" int umhs_region_classify(const float* world_pos, int64_t n, const float* regions_host16, int n_regions, uint8_t* region,
                                    umhs_stream_t stream) {
  if (n < 0 || n_regions < 0 || n_regions > UMHS_MAX_REGIONS || (n_regions > 0 && !regions_host16)) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  if (!world_pos || !region) return UMHS_ERR_ARG;
  const int64_t blocks = (n + RG_THREADS - 1) / RG_THREADS;
  if (blocks > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  region_table T = {};
  for (int k = 0; k < n_regions; ++k)
    for (int i = 0; i < 16; ++i) T.rec[k][i] = regions_host16[16 * k + i];  // copied at the call, as obb_host15 is
  hipLaunchKernelGGL(region_classify_kernel, dim3((unsigned)blocks), dim3(RG_THREADS), 0, umhs_s(stream), world_pos, n, T, n_regions,
                     region);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" size_t umhs_region_segments_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  const size_t nb = (size_t)((n + RG_THREADS - 1) / RG_THREADS);
  return nb * sizeof(int64_t) + nb * sizeof(int32_t) + 64;  // [offsets int64][counts int32]
}

extern "C" int umhs_region_segments(const uint8_t* region, const int64_t* ray_indices, const int64_t* packed_info, int64_t n,
                                    int64_t n_rays, int64_t* seg_of, int64_t* seg_info, int32_t* seg_layer, int64_t* ray_seg,
                                    int64_t* n_segments, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n < 0 || n_rays < 0) return UMHS_ERR_ARG;
  if (n == 0 || n_rays == 0) return UMHS_OK;  // no sample, no segment: nothing is launched, nothing written
  if (!region || !ray_indices || !packed_info || !seg_of || !seg_info || !seg_layer || !ray_seg || !n_segments) return UMHS_ERR_ARG;
  const int64_t nb = (n + RG_THREADS - 1) / RG_THREADS, rb = (n_rays + RG_THREADS - 1) / RG_THREADS;
  if (nb > 0x7fffffff || rb > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < umhs_region_segments_workspace_bytes(n)) return UMHS_ERR_WORKSPACE;
  int64_t* offsets = reinterpret_cast<int64_t*>(workspace);
  int32_t* counts = reinterpret_cast<int32_t*>(offsets + nb);
  hipLaunchKernelGGL(region_head_count_kernel, dim3((unsigned)nb), dim3(RG_THREADS), 0, umhs_s(stream), region, ray_indices, n, counts);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(region_block_scan_kernel, dim3(1), dim3(RG_SCAN_THREADS), 0, umhs_s(stream), (const int32_t*)counts, nb, offsets,
                     n_segments);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(region_emit_kernel, dim3((unsigned)nb), dim3(RG_THREADS), 0, umhs_s(stream), region, ray_indices, n,
                     (const int64_t*)offsets, seg_of, seg_info, seg_layer);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(region_finish_kernel, dim3((unsigned)(nb > rb ? nb : rb)), dim3(RG_THREADS), 0, umhs_s(stream),
                     (const int64_t*)seg_of, packed_info, n, n_rays, (const int64_t*)n_segments, seg_info, ray_seg);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_material_sigma_regions(const float* sigma, const float* abundances, const uint8_t* region, const float* density_gain,
                                           int64_t n, int n_classes, int n_regions, float* sigma_out, umhs_stream_t stream) {
  if (n < 0 || n_classes < 1 || n_classes > 15 || n_regions < 0 || n_regions > UMHS_MAX_REGIONS) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  if (!sigma || !abundances || !region || !density_gain || !sigma_out) return UMHS_ERR_ARG;
  const int64_t blocks = (n + RG_THREADS - 1) / RG_THREADS;
  if (blocks > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  const size_t lds = ((size_t)RG_THREADS + n_regions + 1) * n_classes * sizeof(float);
  hipLaunchKernelGGL(material_sigma_regions_kernel, dim3((unsigned)blocks), dim3(RG_THREADS), lds, umhs_s(stream), sigma, abundances,
                     region, density_gain, n, n_classes, n_regions, sigma_out);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_segment_sum(const float* values, const int64_t* ray_seg, int64_t n_segments, int64_t n_rays, int k, float* out,
                                umhs_stream_t stream) {
  if (n_segments < 0 || n_rays < 0 || k < 1) return UMHS_ERR_ARG;
  if (k > 256) return UMHS_ERR_UNSUPPORTED;
  if (n_rays == 0) return UMHS_OK;
  if (!ray_seg || !out || (n_segments > 0 && !values)) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(segment_sum_kernel, dim3(tile_grid(n_rays)), dim3(RG_THREADS), 0, umhs_s(stream), values, ray_seg, n_segments, n_rays,
                     k, out);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_material_remix_regions(const float* mix16_seg, const float* comp_specular_seg, const int32_t* seg_layer,
                                           const int64_t* ray_seg, const float* endmembers_edit, const float* specular_gain,
                                           int64_t n_segments, int64_t n_rays, int n_bands, int n_classes, int n_regions,
                                           float* spectral, float* spectral2, float* specular, umhs_stream_t stream) {
  if (n_segments < 0 || n_rays < 0 || n_bands < 1 || n_classes < 1 || n_classes > 15 || n_regions < 0 || n_regions > UMHS_MAX_REGIONS)
    return UMHS_ERR_ARG;
  if (n_bands > 256) return UMHS_ERR_UNSUPPORTED;
  if (comp_specular_seg ? (!spectral2 || !specular || !specular_gain) : (spectral2 || specular)) return UMHS_ERR_ARG;
  if (n_rays == 0) return UMHS_OK;
  if (!ray_seg || !endmembers_edit || !spectral || (n_segments > 0 && (!mix16_seg || !seg_layer))) return UMHS_ERR_ARG;
  if (comp_specular_seg && (comp_specular_seg == specular || comp_specular_seg == spectral2 || comp_specular_seg == spectral))
    return UMHS_ERR_ARG;  // [S,B] in, [R,B] out: never the same array
  const size_t layer_bytes = (size_t)n_classes * n_bands * sizeof(float);
  size_t staged = REGION_LDS_BYTES / layer_bytes;
  if (staged > (size_t)n_regions + 1) staged = (size_t)n_regions + 1;
  const size_t lds = staged * layer_bytes;
  const uintptr_t all = (uintptr_t)comp_specular_seg | (uintptr_t)endmembers_edit | (uintptr_t)spectral | (uintptr_t)spectral2 |
                        (uintptr_t)specular;
  if (n_bands % 4 == 0 && (all & 15) == 0)
    hipLaunchKernelGGL(material_remix_regions_kernel<4>, dim3(tile_grid(n_rays)), dim3(RG_THREADS), lds, umhs_s(stream), mix16_seg,
                       comp_specular_seg, seg_layer, ray_seg, endmembers_edit, specular_gain, n_segments, n_rays, n_bands, n_classes,
                       n_regions, (int)staged, spectral, spectral2, specular);
  else
    hipLaunchKernelGGL(material_remix_regions_kernel<1>, dim3(tile_grid(n_rays)), dim3(RG_THREADS), lds, umhs_s(stream), mix16_seg,
                       comp_specular_seg, seg_layer, ray_seg, endmembers_edit, specular_gain, n_segments, n_rays, n_bands, n_classes,
                       n_regions, (int)staged, spectral, spectral2, specular);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
