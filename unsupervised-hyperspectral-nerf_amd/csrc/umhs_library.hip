// Spectral library matching (include/umhs_hip.h, "Spectral library matching"): per ray the two library entries of largest cosine
// with the ray's spectrum (SAM classification), fused: R B floats are read, 16 bytes per ray are written, the [R,L] matrix of
// cosines never exists.
//
//   library_prepare_kernel  re-lays the unit rows [L,B] once as an OPERAND IMAGE: [tile of 32 entries][k-step][64 lanes], the A
//                           operand of v_mfma_f32_32x32x2_f32 (lane l holds entry 32 tile + (l & 31), band 2 step + (l >> 5)), zeros
//                           past L and past B.  A k-step of a tile is then one coalesced run of 64 dwords.
//   library_match_kernel    dot^T[entry][ray] = image x spectra^T on the exact fp32 MFMA.  A block is 4 waves; a wave owns T tiles
//                           of 32 rays for the whole launch and keeps them as B operands in NK registers each (ray on lane & 31, band
//                           2 step + (lane >> 5), zeros past B and past R).  The block walks the library tile by tile: the tile's
//                           image is copied to LDS once and read by all four waves, so a tile fetched from L2 serves 128 T rays.
//                           The MFMA's k order is the band order, its accumulator starts at 0 and a padded step adds an exact 0 x 0:
//                           dot[r,l] is the fmaf chain of the header whatever tile, row or lane the entry sits on.  (The rows and
//                           the walk are umhs_library_tile.h's: the centred projection of umhs_statistics.hip is the same walk.)
//   top-2                   A lane's 16 accumulator rows are 16 entries in ascending index, tile after tile, so a lane inserts with
//                           strict comparisons into ITS running (best, second) and ties stay with the smaller index.  The division
//                           is skipped, exactly, for an entry whose dot is not above the dot of the lane's current second (a
//                           correctly rounded quotient by one positive divisor is monotone).  The two lanes that share a ray merge
//                           at the end by (cosine descending, index ascending).  No atomics: the same bits on every run.
#include "umhs_library_tile.h"  // the operand image's layout, the rows a wave keeps and the tile walk (shared with umhs_statistics.hip)

namespace {

constexpr int LIB_MAX_ENTRIES = 65536;

__global__ __launch_bounds__(256) void library_prepare_kernel(const float* __restrict__ unit, int L, int B, float* __restrict__ image,
                                                               int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int ks = lib_ksteps(B);
  const int lane = (int)(i & 63);
  const int64_t ts = i >> 6;
  const int s = (int)(ts % ks), tile = (int)(ts / ks);
  const int l = 32 * tile + (lane & 31), b = 2 * s + (lane >> 5);
  image[i] = (l < L && b < B) ? unit[(size_t)l * B + b] : 0.0f;
}

struct Top2 {
  float c0, c1, d0, d1;  // cosines of the best and the second, and the dots they came from
  int i0, i1;
};

// (cosine descending, index ascending); an empty slot (index -1, cosine -inf) loses to every entry
__device__ __forceinline__ bool lib_before(float ca, int ia, float cb, int ib) {
  return ib < 0 || (ia >= 0 && (ca > cb || (ca == cb && ia < ib)));
}

template <int NK, int T>
__global__ __launch_bounds__(LIB_THREADS, 2) void library_match_kernel(const float* __restrict__ spectra, int64_t stride, int64_t R,
                                                                      const float* __restrict__ image, int L, int B,
                                                                      int* __restrict__ index, float* __restrict__ cosine) {
  __shared__ float sA[NK * 64];  // the library tile in flight: [k-step][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  lib_zero_tail<NK>(sA, lib_ksteps(B));

  // the wave's ray tiles, as B operands
  const int64_t ray0 = lib_wave_row0(wave, T);
  float x[T][NK], rs[T];
  bool ok[T];
  Top2 best[T];
  lib_load_rows<NK, T, false>(spectra, stride, R, B, ray0, j, h, nullptr, x);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    float ss = 0.0f;  // the chain of s_b^2, b ascending: even bands sit on this lane or on its partner, odd ones on the other
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      const float other = __shfl_xor(x[t][s], 32, 64);
      const float even = h ? other : x[t][s], odd = h ? x[t][s] : other;
      ss = fmaf(even, even, ss);
      ss = fmaf(odd, odd, ss);
    }
    ok[t] = ss > 0.0f && ss <= 3.402823466e38f;  // not 0, not NaN, not Inf
    rs[t] = sqrtf(ss);
    best[t] = Top2{-INFINITY, -INFINITY, -INFINITY, -INFINITY, -1, -1};
  }

  lib_tile_walk<NK, T>(image, lib_ksteps(B), lib_tiles(L), sA, x, [&](int tile, const v16f (&acc)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      Top2& p = best[t];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int l = 32 * tile + lib_acc_row(e, h);
        const float d = acc[t][e];
        if (l < L && d > p.d1) {
          const float c = d / rs[t];
          if (c > p.c0) {
            p.c1 = p.c0, p.i1 = p.i0, p.d1 = p.d0;
            p.c0 = c, p.i0 = l, p.d0 = d;
          } else if (c > p.c1) {
            p.c1 = c, p.i1 = l, p.d1 = d;
          }
        }
      }
    }
  });

#pragma unroll
  for (int t = 0; t < T; ++t) {
    const Top2& p = best[t];
    const float q0 = __shfl_xor(p.c0, 32, 64), q1 = __shfl_xor(p.c1, 32, 64);
    const int k0 = __shfl_xor(p.i0, 32, 64), k1 = __shfl_xor(p.i1, 32, 64);
    float c0, c1;
    int i0, i1;
    if (lib_before(p.c0, p.i0, q0, k0)) {
      c0 = p.c0, i0 = p.i0;
      if (lib_before(p.c1, p.i1, q0, k0)) c1 = p.c1, i1 = p.i1; else c1 = q0, i1 = k0;
    } else {
      c0 = q0, i0 = k0;
      if (lib_before(p.c0, p.i0, q1, k1)) c1 = p.c0, i1 = p.i0; else c1 = q1, i1 = k1;
    }
    if (!ok[t] || i0 < 0) i0 = -1, i1 = -1, c0 = 0.0f, c1 = 0.0f;
    else if (i1 < 0) c1 = -1.0f;
    const int64_t r = ray0 + 32 * t + j;
    if (h == 0 && r < R) {
      index[2 * r] = i0, index[2 * r + 1] = i1;
      cosine[2 * r] = c0, cosine[2 * r + 1] = c1;
    }
  }
}

template <int NK, int T>
void library_launch(const float* spectra, int64_t stride, int64_t R, const float* image, int L, int B, int* index, float* cosine,
                    hipStream_t stream) {
  const int64_t per_block = (int64_t)(LIB_THREADS / 64) * 32 * T;
  const int64_t blocks = (R + per_block - 1) / per_block;
  hipLaunchKernelGGL((library_match_kernel<NK, T>), dim3((unsigned)blocks), dim3(LIB_THREADS), 0, stream, spectra, stride, R, image, L, B,
                     index, cosine);
}

}  // namespace

extern "C" size_t umhs_library_image_bytes(int n_entries, int n_bands) {
  if (n_entries < 1 || n_bands < 1 || n_entries > LIB_MAX_ENTRIES || n_bands > LIB_MAX_BANDS) return 0;
  return (size_t)lib_tiles(n_entries) * lib_ksteps(n_bands) * 64 * sizeof(float);
}

extern "C" int umhs_library_prepare(const float* unit, int n_entries, int n_bands, float* image, umhs_stream_t stream) {
  if (n_entries < 1 || n_bands < 1) return UMHS_ERR_ARG;
  if (n_entries > LIB_MAX_ENTRIES || n_bands > LIB_MAX_BANDS) return UMHS_ERR_UNSUPPORTED;
  if (!unit || !image) return UMHS_ERR_ARG;
  const int64_t n = (int64_t)lib_tiles(n_entries) * lib_ksteps(n_bands) * 64;
  hipLaunchKernelGGL(library_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, umhs_s(stream), unit, n_entries, n_bands,
                     image, n);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_library_match(const float* spectra, int64_t stride, int64_t n_rays, const float* image, int n_entries, int n_bands,
                                  int32_t* index, float* cosine, umhs_stream_t stream) {
  if (n_entries < 1 || n_bands < 1 || n_rays < 0 || stride < n_bands) return UMHS_ERR_ARG;
  if (n_entries > LIB_MAX_ENTRIES || n_bands > LIB_MAX_BANDS) return UMHS_ERR_UNSUPPORTED;
  if (n_rays == 0) return UMHS_OK;
  if (!spectra || !image || !index || !cosine) return UMHS_ERR_ARG;
  if ((n_rays + 127) / 128 > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  const int ks = lib_ksteps(n_bands);
  hipStream_t s = umhs_s(stream);
#define LIB_CASE(NK, T) library_launch<NK, T>(spectra, stride, n_rays, image, n_entries, n_bands, index, cosine, s);
  LIB_DISPATCH(ks, LIB_CASE, return UMHS_ERR_UNSUPPORTED;)
#undef LIB_CASE
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
