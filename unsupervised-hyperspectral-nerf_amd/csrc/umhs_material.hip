// Material edits at render time (include/umhs_hip.h, "Material edits"): the two elementwise passes an edited render adds to the
// gradient-free path.  Neither touches the field kernels: both read what umhs_field_heads_fwd already leaves behind (the per-sample
// abundances and the per-ray sums mix16).
//
//   material_sigma_kernel  ONE SAMPLE PER LANE.  A block's 256 abundance rows are one contiguous run of 256 C floats: they are loaded
//                          lane after lane (coalesced) into LDS and each lane then walks its own row there, c ascending.  4 (C + 2)
//                          bytes per sample, nothing else: bandwidth bound.
//   material_remix_*       LANES ALONG BANDS.  A block takes tiles of 32 rays; a tile's outputs are one contiguous run of 32 B floats,
//                          so consecutive lanes hold consecutive addresses.  Two forms, chosen on the host, that evaluate the same
//                          fmaf chain (the bits do not depend on which one ran): 16-byte pieces when B % 4 == 0 and every row array
//                          is 16-byte aligned, else one float per lane with the lane's dictionary column held in registers.  The
//                          edited dictionary (C B floats, at most 15 KB) is staged in LDS once per block and the blocks are
//                          persistent (grid-stride over the tiles), the tile's 32 x C sums once per tile.  64 + 4 B bytes read and
//                          4 B or 12 B written per ray; no atomics, no cross-lane arithmetic: the result is a function of the
//                          inputs alone.
#include "umhs_common.h"

// the only fused operations are the explicit fmaf chains: spectral is the ROUNDED specular added to the mixing term, on either lane form
#pragma clang fp contract(off)

namespace {

constexpr int MAT_THREADS = 256;
constexpr int REMIX_RAYS = 32;  // rays per tile

__global__ __launch_bounds__(MAT_THREADS) void material_sigma_kernel(const float* sigma, const float* __restrict__ abund,
                                                                    const float* __restrict__ gain, int64_t n, int C, float* sigma_out) {
  extern __shared__ float sA[];  // [256][C], the block's rows as they lie in memory
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * MAT_THREADS;
  const int64_t rows = n - first < MAT_THREADS ? n - first : MAT_THREADS;
  const int count = (int)rows * C;
  const float* src = abund + first * C;
  for (int k = tid; k < count; k += MAT_THREADS) sA[k] = src[k];
  __syncthreads();
  if (tid >= rows) return;
  float acc = 0.0f;
  for (int c = 0; c < C; ++c) acc = fmaf(gain[c] - 1.0f, sA[tid * C + c], acc);  // all gains 1: every term and the sum are exactly 0
  sigma_out[first + tid] = sigma[first + tid] * fmaxf(0.0f, 1.0f + acc);
}

// Dynamic LDS of both remix kernels: [C][B] dictionary, then (16-byte aligned) [32][16] per-ray sums of the tile in flight.
__host__ __device__ inline int remix_sums_offset(int C, int B) { return (C * B + 3) & ~3; }

__device__ __forceinline__ void remix_stage_dictionary(float* sE, float* sM, const float* __restrict__ E, int CB) {
  for (int k = threadIdx.x; k < CB; k += MAT_THREADS) sE[k] = E[k];
  // columns >= C of the sums stay 0 for the whole launch: they are never loaded from memory (the heads kernel does not promise what
  // they hold) and never enter the arithmetic
  for (int k = threadIdx.x; k < REMIX_RAYS * 16; k += MAT_THREADS) sM[k] = 0.0f;
}

__device__ __forceinline__ void remix_stage_sums(float* sM, const float* __restrict__ mix16, int64_t r0, int nr, int C) {
  __syncthreads();  // the previous tile's sums are consumed (first pass: dictionary and zeros are in place)
  for (int k = threadIdx.x; k < nr * 16; k += MAT_THREADS)
    if ((k & 15) < C) sM[k] = mix16[r0 * 16 + k];
  __syncthreads();
}

// 16-byte form: B % 4 == 0 and every row array 16-byte aligned, so a piece never straddles two rays and every access is aligned.  A
// lane takes pieces q, q + 256, ... of the tile's run.  comp_specular may be the same array as specular (each lane reads its piece
// before it writes it), hence no __restrict__ on those.
__global__ __launch_bounds__(MAT_THREADS) void material_remix_vec4_kernel(const float* __restrict__ mix16, const float* comp_specular,
                                                                         const float* __restrict__ E, float s, int64_t R, int B, int C,
                                                                         float* spectral, float* spectral2, float* specular) {
  extern __shared__ __align__(16) float smem[];
  float *sE = smem, *sM = smem + remix_sums_offset(C, B);
  remix_stage_dictionary(sE, sM, E, C * B);
  const int tid = threadIdx.x, per_row = B >> 2;
  const int64_t tiles = (R + REMIX_RAYS - 1) / REMIX_RAYS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * REMIX_RAYS;
    const int nr = R - r0 < REMIX_RAYS ? (int)(R - r0) : REMIX_RAYS;
    remix_stage_sums(sM, mix16, r0, nr, C);
    const float4* sp_in = reinterpret_cast<const float4*>(comp_specular ? comp_specular + r0 * B : nullptr);
    float4* o_spec = reinterpret_cast<float4*>(spectral + r0 * B);
    float4* o_mix = reinterpret_cast<float4*>(spectral2 ? spectral2 + r0 * B : nullptr);
    float4* o_sp = reinterpret_cast<float4*>(specular ? specular + r0 * B : nullptr);
    for (int q = tid; q < nr * per_row; q += MAT_THREADS) {
      const int r = q / per_row, b = (q - r * per_row) << 2;
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int c = 0; c < C; ++c) {
        const float m = sM[r * 16 + c];
        const float4 e = *reinterpret_cast<const float4*>(sE + c * B + b);
        acc.x = fmaf(m, e.x, acc.x), acc.y = fmaf(m, e.y, acc.y), acc.z = fmaf(m, e.z, acc.z), acc.w = fmaf(m, e.w, acc.w);
      }
      if (sp_in) {
        const float4 v = sp_in[q];
        const float4 sp = make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
        o_sp[q] = sp, o_mix[q] = acc;
        o_spec[q] = make_float4(acc.x + sp.x, acc.y + sp.y, acc.z + sp.z, acc.w + sp.w);
      } else {
        o_spec[q] = acc;
      }
    }
  }
}

// One-float form (any B, any alignment): a lane owns ONE band for the whole launch and keeps that column of the dictionary in
// registers; 256 / B rays are in flight per pass, lane t = slot * B + band, so a pass touches one contiguous run of floats.  Per element
// the LDS is read four times (the ray's 16 sums as 16-byte broadcasts) instead of 2 C times; with both operands in LDS the 31-band
// frame ran 3.1x off a copy of its bytes, bound by LDS issue.
__global__ __launch_bounds__(MAT_THREADS) void material_remix_band_kernel(const float* __restrict__ mix16, const float* comp_specular,
                                                                         const float* __restrict__ E, float s, int64_t R, int B, int C,
                                                                         float* spectral, float* spectral2, float* specular) {
  extern __shared__ __align__(16) float smem[];
  float *sE = smem, *sM = smem + remix_sums_offset(C, B);
  remix_stage_dictionary(sE, sM, E, C * B);
  __syncthreads();
  const int tid = threadIdx.x, slots = MAT_THREADS / B;
  const int slot = tid / B, b = tid - slot * B;
  const bool active = slot < slots;
  float e[15];
#pragma unroll
  for (int c = 0; c < 15; ++c) e[c] = (active && c < C) ? sE[c * B + b] : 0.0f;
  const int64_t tiles = (R + REMIX_RAYS - 1) / REMIX_RAYS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * REMIX_RAYS;
    const int nr = R - r0 < REMIX_RAYS ? (int)(R - r0) : REMIX_RAYS;
    remix_stage_sums(sM, mix16, r0, nr, C);
    if (!active) continue;  // (the barriers above are reached by every lane of the block in every round)
    for (int r = slot; r < nr; r += slots) {
      const float4* m4 = reinterpret_cast<const float4*>(sM + r * 16);
      const float4 m0 = m4[0], m1 = m4[1], m2 = m4[2], m3 = m4[3];
      const float m[15] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w, m3.x, m3.y, m3.z};
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < 15; ++c)
        if (c < C) acc = fmaf(m[c], e[c], acc);  // the same chain as the 16-byte form: the same bits
      const int64_t at = (r0 + r) * B + b;
      if (comp_specular) {
        const float sp = s * comp_specular[at];
        specular[at] = sp, spectral2[at] = acc, spectral[at] = acc + sp;
      } else {
        spectral[at] = acc;
      }
    }
  }
}

}  // namespace

extern "C" int umhs_material_sigma(const float* sigma, const float* abundances, const float* density_gain, int64_t n, int n_classes,
                                   float* sigma_out, umhs_stream_t stream) {
  if (n < 0 || n_classes < 1 || n_classes > 15) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  if (!sigma || !abundances || !density_gain || !sigma_out) return UMHS_ERR_ARG;
  const int64_t blocks = (n + MAT_THREADS - 1) / MAT_THREADS;
  if (blocks > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(material_sigma_kernel, dim3((unsigned)blocks), dim3(MAT_THREADS), (size_t)MAT_THREADS * n_classes * sizeof(float),
                     umhs_s(stream), sigma, abundances, density_gain, n, n_classes, sigma_out);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_material_remix(const float* mix16, const float* comp_specular, const float* endmembers_edit, float specular_gain,
                                   int64_t n_rays, int n_bands, int n_classes, float* spectral, float* spectral2, float* specular,
                                   umhs_stream_t stream) {
  if (n_rays < 0 || n_bands < 1 || n_classes < 1 || n_classes > 15) return UMHS_ERR_ARG;
  if (n_bands > 256) return UMHS_ERR_UNSUPPORTED;
  if (comp_specular ? (!spectral2 || !specular) : (spectral2 || specular)) return UMHS_ERR_ARG;
  if (n_rays == 0) return UMHS_OK;
  if (!mix16 || !endmembers_edit || !spectral) return UMHS_ERR_ARG;
  const int64_t tiles = (n_rays + REMIX_RAYS - 1) / REMIX_RAYS;
  const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);  // 8 resident blocks on each of the 256 CUs
  const size_t lds = ((size_t)remix_sums_offset(n_classes, n_bands) + REMIX_RAYS * 16) * sizeof(float);
  const uintptr_t all = (uintptr_t)comp_specular | (uintptr_t)spectral | (uintptr_t)spectral2 | (uintptr_t)specular;
  if (n_bands % 4 == 0 && (all & 15) == 0)
    hipLaunchKernelGGL(material_remix_vec4_kernel, dim3(grid), dim3(MAT_THREADS), lds, umhs_s(stream), mix16, comp_specular,
                       endmembers_edit, specular_gain, n_rays, n_bands, n_classes, spectral, spectral2, specular);
  else
    hipLaunchKernelGGL(material_remix_band_kernel, dim3(grid), dim3(MAT_THREADS), lds, umhs_s(stream), mix16, comp_specular,
                       endmembers_edit, specular_gain, n_rays, n_bands, n_classes, spectral, spectral2, specular);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
