// Scene statistics (include/umhs_hip.h, "Scene statistics"): the second-order statistics of the valid spectra of a scene -- count,
// shifted sum and shifted Gram matrix -- and the centred projection that turns them into PCA components and RX scores.
//
//   gram_chunk_kernel    one block (4 waves) per chunk of UMHS_GRAM_CHUNK rows.  The chunk goes through LDS in slabs of 32 rows: a wave
//                        loads whole rows (a coalesced run per row), decides validity once per row (every value finite and
//                        accumulation > 0.5) and stores c = x - shift, or zeros for an invalid row, so the row adds an exact 0 x 0
//                        to every chain.  g = c^T c on v_mfma_f32_32x32x2_f32 with the ROW as the k dimension: lane l reads
//                        c[2 s + (l >> 5)][32 t + (l & 31)], and the same read serves as the A operand of band tile i and as the B
//                        operand of band tile j.  The upper-triangle tile pairs (36 at B = 256) are dealt round-robin to the four waves;
//                        a pair's fp32 accumulator lives in registers for the whole chunk, so g[a,b] is the fmaf chain over the
//                        chunk's rows ascending (the MFMA's k order is the row order, its accumulator starts at 0).  s[b] is summed
//                        by thread b from the same LDS rows in the same order.  The next slab's loads are in flight under the MFMAs.
//                        The block writes the chunk's (count, s, upper-triangle g) as float32 to its own slot of the workspace.
//   gram_reduce_kernel   one thread per element of acc: the slots of a pass added in float64, chunks ascending, onto acc; an element
//                        above the diagonal is written to both places (the mirror).  No atomics anywhere: the same bits on every run.
//   spectral_project_kernel  the library match kernel's walk (umhs_library_tile.h) on centred rows, with another epilogue: the first P
//                        entries of a row are stored, and the squares of all K are chained in k order -- a lane holds entries
//                        8 g + 4 h .. + 3 of each group g of 8, so the chain passes between the two lanes of a row group by group.
#include "umhs_library_tile.h"

namespace {

constexpr int GRAM_THREADS = 256, GRAM_SLAB = 32, GRAM_ROWS_PER_WAVE = GRAM_SLAB / 4;
constexpr int GRAM_PASS = 512;  // chunks per pass: the workspace holds one slot per chunk of a pass
constexpr float FLT_BIG = 3.402823466e38f;

__host__ __device__ inline int64_t gram_slot_floats(int B) { return 1 + (int64_t)B + (int64_t)B * B; }

template <int NT>  // band tiles of 32
__global__ __launch_bounds__(GRAM_THREADS) void gram_chunk_kernel(const float* __restrict__ spectra, int64_t stride, int64_t R, int B,
                                                                  const float* __restrict__ shift, const float* __restrict__ accumulation,
                                                                  int64_t first_chunk, float* __restrict__ partial) {
  constexpr int LD = NT * 32, NV = (NT + 1) / 2, NP = NT * (NT + 1) / 2, PPW = (NP + 3) / 4;
  __shared__ float sC[GRAM_SLAB * LD];  // the slab in flight: [row][band], zeros past B and in invalid rows
  __shared__ int sCount[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t row0 = (first_chunk + blockIdx.x) * (int64_t)UMHS_GRAM_CHUNK;
  const int64_t row1 = row0 + UMHS_GRAM_CHUNK < R ? row0 + UMHS_GRAM_CHUNK : R;

  // the wave's tile pairs (i <= j), row-major over the upper triangle, dealt round-robin; a surplus slot repeats pair (0, 0) unwritten
  int pi[PPW], pj[PPW];
#pragma unroll
  for (int p = 0; p < PPW; ++p) {
    int q = wave + 4 * p, i = 0;
    if (q >= NP) q = 0;
    while (q >= NT - i) q -= NT - i, ++i;
    pi[p] = i, pj[p] = i + q;
  }
  float sh[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) sh[v] = (lane + 64 * v < B) ? shift[lane + 64 * v] : 0.0f;

  v16f acc[PPW];
#pragma unroll
  for (int p = 0; p < PPW; ++p)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[p][e] = 0.0f;
  float sum = 0.0f;
  int count = 0;

  float xr[GRAM_ROWS_PER_WAVE][NV], av[GRAM_ROWS_PER_WAVE];
  auto load_slab = [&](int64_t base) {
#pragma unroll
    for (int i = 0; i < GRAM_ROWS_PER_WAVE; ++i) {
      const int64_t r = base + wave + 4 * i;
      const bool in = r < row1;
      const float* row = spectra + (in ? r : row0) * stride;
#pragma unroll
      for (int v = 0; v < NV; ++v) xr[i][v] = (in && lane + 64 * v < B) ? row[lane + 64 * v] : 0.0f;
      av[i] = !in ? 0.0f : accumulation ? accumulation[r] : 1.0f;
    }
  };

  load_slab(row0);
  for (int64_t base = row0; base < row1; base += GRAM_SLAB) {
#pragma unroll
    for (int i = 0; i < GRAM_ROWS_PER_WAVE; ++i) {
      bool finite = true;
#pragma unroll
      for (int v = 0; v < NV; ++v) finite = finite && fabsf(xr[i][v]) <= FLT_BIG;  // (not NaN, not Inf; the padding is 0)
      const bool valid = __all(finite) && av[i] > 0.5f;  // (av is 0 past the chunk's last row)
      count += valid ? 1 : 0;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int b = lane + 64 * v;
        if (b < LD) sC[(wave + 4 * i) * LD + b] = (valid && b < B) ? xr[i][v] - sh[v] : 0.0f;
      }
    }
    __syncthreads();
    if (base + GRAM_SLAB < row1) load_slab(base + GRAM_SLAB);  // in flight under the MFMAs
#pragma unroll 4
    for (int s = 0; s < GRAM_SLAB / 2; ++s) {
      const float* at = sC + (2 * s + h) * LD + j;
#pragma unroll
      for (int p = 0; p < PPW; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(at[32 * pi[p]], at[32 * pj[p]], acc[p], 0, 0, 0);
    }
    if (tid < B) {
#pragma unroll 8
      for (int r = 0; r < GRAM_SLAB; ++r) sum += sC[r * LD + tid];
    }
    __syncthreads();  // the slab is free again
  }

  float* slot = partial + (int64_t)blockIdx.x * gram_slot_floats(B);
  if (lane == 0) sCount[wave] = count;  // (validity is decided per wave: every lane of a wave holds the same count)
  __syncthreads();
  if (tid == 0) slot[0] = (float)(sCount[0] + sCount[1] + sCount[2] + sCount[3]);  // <= 1024: exact
  if (tid < B) slot[1 + tid] = sum;
#pragma unroll
  for (int p = 0; p < PPW; ++p) {
    if (wave + 4 * p >= NP) continue;
    const int b = 32 * pj[p] + j;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int a = 32 * pi[p] + lib_acc_row(e, h);
      if (a < B && b < B) slot[1 + B + a * B + b] = acc[p][e];
    }
  }
}

__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ partial, int chunks, int B, double* __restrict__ acc) {
  const int64_t n = gram_slot_floats(B), idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  int a = 0, b = 0;
  if (idx > B) {
    a = (int)((idx - 1 - B) / B), b = (int)((idx - 1 - B) % B);
    if (a > b) return;  // written by (b, a)
  }
  double v = acc[idx];
  for (int c = 0; c < chunks; ++c) v += (double)partial[c * n + idx];
  acc[idx] = v;
  if (a < b) acc[1 + B + (int64_t)b * B + a] = v;
}

template <int NT>
void gram_launch(const float* spectra, int64_t stride, int64_t R, int B, const float* shift, const float* accumulation, int64_t first_chunk,
                 int chunks, float* partial, hipStream_t stream) {
  hipLaunchKernelGGL((gram_chunk_kernel<NT>), dim3((unsigned)chunks), dim3(GRAM_THREADS), 0, stream, spectra, stride, R, B, shift,
                     accumulation, first_chunk, partial);
}

template <int NK, int T>
__global__ __launch_bounds__(LIB_THREADS, 2) void spectral_project_kernel(const float* __restrict__ spectra, int64_t stride, int64_t R,
                                                                         const float* __restrict__ mean, const float* __restrict__ image,
                                                                         int K, int B, int P, float* __restrict__ components,
                                                                         float* __restrict__ score) {
  __shared__ float sA[NK * 64];  // the tile of W in flight: [k-step][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  lib_zero_tail<NK>(sA, lib_ksteps(B));
  const int64_t ray0 = lib_wave_row0(wave, T);
  float x[T][NK], ss[T];
  lib_load_rows<NK, T, true>(spectra, stride, R, B, ray0, j, h, mean, x);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    bool finite = true;
#pragma unroll
    for (int s = 0; s < NK; ++s) finite = finite && fabsf(x[t][s]) <= FLT_BIG;
    const int partner = __shfl_xor((int)finite, 32, 64);  // the row's other bands sit on the partner lane (every lane takes part)
    finite = finite && partner != 0;
    if (!finite) {  // the row projects to exact zeros
#pragma unroll
      for (int s = 0; s < NK; ++s) x[t][s] = 0.0f;
    }
    ss[t] = 0.0f;
  }

  lib_tile_walk<NK, T>(image, lib_ksteps(B), lib_tiles(K), sA, x, [&](int tile, const v16f (&acc)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int64_t r = ray0 + 32 * t + j;
      if (32 * tile < P && r < R) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int k = 32 * tile + lib_acc_row(e, h);
          if (k < P) components[r * P + k] = acc[t][e];
        }
      }
      if (score) {  // entries past K are exact zeros: fmaf(0, 0, ss) = ss
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float lo[4], hi[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float mine = acc[t][4 * g + i], other = __shfl_xor(mine, 32, 64);
            lo[i] = h ? other : mine, hi[i] = h ? mine : other;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) ss[t] = fmaf(lo[i], lo[i], ss[t]);
#pragma unroll
          for (int i = 0; i < 4; ++i) ss[t] = fmaf(hi[i], hi[i], ss[t]);
        }
      }
    }
  });

  if (score && h == 0) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int64_t r = ray0 + 32 * t + j;
      if (r < R) score[r] = ss[t];
    }
  }
}

template <int NK, int T>
void project_launch(const float* spectra, int64_t stride, int64_t R, const float* mean, const float* image, int K, int B, int P,
                    float* components, float* score, hipStream_t stream) {
  const int64_t per_block = (int64_t)(LIB_THREADS / 64) * 32 * T;
  const int64_t blocks = (R + per_block - 1) / per_block;
  hipLaunchKernelGGL((spectral_project_kernel<NK, T>), dim3((unsigned)blocks), dim3(LIB_THREADS), 0, stream, spectra, stride, R, mean, image,
                     K, B, P, components, score);
}

}  // namespace

extern "C" int umhs_gram_chunk(void) { return UMHS_GRAM_CHUNK; }

extern "C" size_t umhs_gram_workspace_bytes(int64_t n_rows, int n_bands) {
  if (n_rows < 1 || n_bands < 1 || n_bands > LIB_MAX_BANDS) return 0;
  const int64_t chunks = (n_rows + UMHS_GRAM_CHUNK - 1) / UMHS_GRAM_CHUNK;
  return (size_t)(chunks < GRAM_PASS ? chunks : GRAM_PASS) * gram_slot_floats(n_bands) * sizeof(float);
}

extern "C" int umhs_gram_accumulate(const float* spectra, int64_t stride, int64_t n_rows, int n_bands, const float* shift,
                                    const float* accumulation, double* acc, void* workspace, size_t workspace_bytes,
                                    umhs_stream_t stream) {
  if (n_bands < 1 || n_rows < 0 || stride < n_bands) return UMHS_ERR_ARG;
  if (n_bands > LIB_MAX_BANDS) return UMHS_ERR_UNSUPPORTED;
  if (n_rows == 0) return UMHS_OK;
  if (!spectra || !shift || !acc || !workspace) return UMHS_ERR_ARG;
  if (workspace_bytes < umhs_gram_workspace_bytes(n_rows, n_bands) || ((uintptr_t)workspace & 3)) return UMHS_ERR_ARG;
  const int64_t chunks = (n_rows + UMHS_GRAM_CHUNK - 1) / UMHS_GRAM_CHUNK;
  const int B = n_bands, tiles = (B + 31) >> 5;
  const unsigned reduce_blocks = (unsigned)((gram_slot_floats(B) + 255) / 256);
  float* partial = (float*)workspace;
  hipStream_t s = umhs_s(stream);
  for (int64_t first = 0; first < chunks; first += GRAM_PASS) {
    const int n = (int)(chunks - first < GRAM_PASS ? chunks - first : GRAM_PASS);
    switch (tiles) {
#define GRAM_CASE(NT) \
  case NT: gram_launch<NT>(spectra, stride, n_rows, B, shift, accumulation, first, n, partial, s); break;
      GRAM_CASE(1) GRAM_CASE(2) GRAM_CASE(3) GRAM_CASE(4) GRAM_CASE(5) GRAM_CASE(6) GRAM_CASE(7) GRAM_CASE(8)
#undef GRAM_CASE
      default: return UMHS_ERR_UNSUPPORTED;
    }
    UMHS_CHECK_LAUNCH();
    hipLaunchKernelGGL(gram_reduce_kernel, dim3(reduce_blocks), dim3(256), 0, s, partial, n, B, acc);
    UMHS_CHECK_LAUNCH();
  }
  return UMHS_OK;
}

extern "C" int umhs_spectral_project(const float* spectra, int64_t stride, int64_t n_rows, const float* mean, const float* image,
                                     int n_components, int n_bands, int n_stored, float* components, float* score,
                                     umhs_stream_t stream) {
  if (n_bands < 1 || n_components < 1 || n_rows < 0 || stride < n_bands || n_stored < 0 || n_stored > n_components) return UMHS_ERR_ARG;
  if (n_bands > LIB_MAX_BANDS || n_components > 256) return UMHS_ERR_UNSUPPORTED;
  if (n_rows == 0) return UMHS_OK;
  if (!spectra || !mean || !image || (n_stored > 0 && !components)) return UMHS_ERR_ARG;
  if ((n_rows + 127) / 128 > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  const int ks = lib_ksteps(n_bands);
  hipStream_t s = umhs_s(stream);
#define PROJECT_CASE(NK, T) \
  project_launch<NK, T>(spectra, stride, n_rows, mean, image, n_components, n_bands, n_stored, components, score, s);
  LIB_DISPATCH(ks, PROJECT_CASE, return UMHS_ERR_UNSUPPORTED;)
#undef PROJECT_CASE
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
