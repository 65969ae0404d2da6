// What the kernels that stream an OPERAND IMAGE share (umhs_library.hip: the match; umhs_statistics.hip: the centred projection): the
// image's layout, the rows a wave keeps as B operands of v_mfma_f32_32x32x2_f32 and the walk over the image's tiles.
//
//   image      [tile of 32 entries][k-step][64 lanes]: lane l of a k-step holds entry 32 tile + (l & 31), band 2 step + (l >> 5), zeros
//              past the last entry and past B (umhs_library_prepare makes it).
//   rows       a block is 4 waves; a wave owns T tiles of 32 rows for the whole launch and keeps them in NK registers each (row on
//              lane & 31, band 2 step + (lane >> 5), zeros past B and past R).
//   walk       tile by tile: the tile's image is copied to LDS once and read by all four waves; dot^T[entry][row] = image x rows^T on
//              the exact fp32 MFMA, whose k order is the band order, whose accumulator starts at 0 and for which a padded step adds an
//              exact 0 x 0: dot[r,l] is the fmaf chain over b ascending whatever tile, row or lane the entry sits on.  The epilogue
//              gets (tile, acc[T]): element e of acc[t] on lane (j, h) is entry 32 tile + lib_acc_row(e, h) of row ray0 + 32 t + j.
#pragma once
#include "umhs_common.h"

typedef float v16f __attribute__((ext_vector_type(16)));

namespace {

constexpr int LIB_THREADS = 256;  // 4 waves
constexpr int LIB_MAX_BANDS = 256;

__host__ __device__ inline int lib_ksteps(int B) { return (B + 1) >> 1; }
__host__ __device__ inline int lib_tiles(int L) { return (L + 31) >> 5; }
__device__ __forceinline__ int lib_acc_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }  // ascending in e

// the first row of the wave's T tiles
__device__ __forceinline__ int64_t lib_wave_row0(int wave, int T) { return ((int64_t)blockIdx.x * (LIB_THREADS / 64) + wave) * (32 * T); }

// x[t][s] = row (ray0 + 32 t + j), band 2 s + h, minus centre[band] when CENTRE (one float32 subtraction); 0 past R and past B
template <int NK, int T, bool CENTRE>
__device__ __forceinline__ void lib_load_rows(const float* __restrict__ spectra, int64_t stride, int64_t R, int B, int64_t ray0, int j, int h,
                                              const float* __restrict__ centre, float (&x)[T][NK]) {
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t r = ray0 + 32 * t + j;
    const float* row = spectra + (r < R ? r : 0) * stride;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      const int b = 2 * s + h;
      if (CENTRE) x[t][s] = (r < R && b < B) ? row[b] - centre[b] : 0.0f;
      else x[t][s] = (r < R && b < B) ? row[b] : 0.0f;
    }
  }
}

// sA: NK * 64 floats of LDS; its steps >= ceil(B / 2) are zeroed once, before the walk, and stay 0
template <int NK>
__device__ __forceinline__ void lib_zero_tail(float* sA, int ks) {
  for (int k = ks * 64 + threadIdx.x; k < NK * 64; k += LIB_THREADS) sA[k] = 0.0f;
}

template <int NK, int T, class Epilogue>
__device__ __forceinline__ void lib_tile_walk(const float* __restrict__ image, int ks, int tiles, float* sA, const float (&x)[T][NK],
                                              Epilogue&& epilogue) {
  const int tid = threadIdx.x, lane = tid & 63;
  for (int tile = 0; tile < tiles; ++tile) {
    __syncthreads();  // every wave is done with the previous tile
    const float* src = image + (size_t)tile * ks * 64;
    for (int k = tid; k < ks * 64; k += LIB_THREADS) sA[k] = src[k];
    __syncthreads();
    v16f acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      const float a = sA[s * 64 + lane];
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[t][s], acc[t], 0, 0, 0);
    }
    epilogue(tile, acc);
  }
}

// the (NK, T) a launch takes: NK the k-steps a wave keeps per row tile (>= ks; the surplus multiplies zeros), two row tiles per wave
// while they fit 256 registers with the accumulators.  CASE(NK, T) is expanded for the first NK >= ks; OTHERWISE when there is none.
#define LIB_DISPATCH(ks, CASE, OTHERWISE)                                                                                      \
  if ((ks) <= 8) { CASE(8, 2) } else if ((ks) <= 16) { CASE(16, 2) } else if ((ks) <= 24) { CASE(24, 2) }                       \
  else if ((ks) <= 32) { CASE(32, 2) } else if ((ks) <= 48) { CASE(48, 2) } else if ((ks) <= 64) { CASE(64, 2) }                \
  else if ((ks) <= 72) { CASE(72, 2) } else if ((ks) <= 96) { CASE(96, 1) } else if ((ks) <= 128) { CASE(128, 1) }              \
  else { OTHERWISE }

}  // namespace
