// Sparse unmixing (include/umhs_hip.h, "Sparse unmixing"): per row the non-negative lasso against a whole library of L <= 128 entries,
// by ADMM: hundreds of [L x L] . [L] products per row with a threshold in between.  One launch, specialised on T = ceil(L / 32).
//
//   block      4 waves; a wave owns ONE tile of 32 rows for the whole solve and never waits for another wave after the first barrier.
//              At T = 4 a wave keeps c, z, d and the accumulators in 4 x 64 registers (one wave per SIMD), so a CU holds one block.
//   M          resident in LDS for the whole launch (64 KB at L = 128), in the layout umhs_sparse_prepare makes: the A operands of
//              four consecutive k-steps of one (output tile, input tile) pair side by side per lane -- one ds_read_b128 feeds four MFMAs.
//   products   v_mfma_f32_32x32x2_f32, which is bitwise an fmaf chain in k order.  c = Q x streams the operand image of Q from global
//              memory, one band pair per step, exactly as the library match forms its dot.  In the loop the accumulator of output tile
//              `to` starts from c and takes, for every input tile ti and e = 0 .. 15, the step whose two k are the entries
//              32 ti + lib_acc_row(e, 0) and 32 ti + lib_acc_row(e, 1): lane (row, h) holds exactly those entries of its row in element
//              e of its accumulators, so z - d is the B operand as it lies -- the state never leaves its registers and no lane
//              exchanges anything but the two maxima of the stopping rule.
//   stop       a row that is done is frozen (its z and d are no longer replaced); the wave leaves the loop when all its rows are done
//              or at max_iterations.  Rows past R and invalid rows are done from the start.
//   residual   only when asked for: b = A x and w = G z by the same two products (G's image read from global memory once).
#include "umhs_library_tile.h"

#pragma clang fp contract(off)  // (t - tau and epsilon * s are single operations; the chains are written as fmaf)

typedef float v4f __attribute__((ext_vector_type(4)));

namespace {

constexpr int SP_THREADS = 256;  // 4 waves, 32 rows each
constexpr int SP_MAX_L = UMHS_SPARSE_MAX_ENTRIES;
constexpr float SP_FLT_MAX = 3.402823466e38f;

__host__ __device__ inline int sp_image_floats(int T) { return T * T * 1024; }

__global__ void sparse_prepare_kernel(const float* __restrict__ m, int L, int T, float* __restrict__ image) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sp_image_floats(T)) return;
  const int q = i & 3, lane = (i >> 2) & 63, e = 4 * ((i >> 8) & 3) + q, pair = i >> 10, ti = pair % T, to = pair / T;
  const int row = 32 * to + (lane & 31), col = 32 * ti + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
  image[i] = (row < L && col < L) ? m[row * L + col] : 0.0f;
}

// acc[t] += image (an operand image of [32 T entries][B]) x rows^T, band pairs ascending; -> this lane's chain of x_b^2
template <int T>
__device__ __forceinline__ float sp_band_products(const float* __restrict__ image, const float* __restrict__ row, bool inside, int B, int ks,
                                                  int lane, int h, v16f (&acc)[T]) {
  float own = 0.0f;
  for (int s = 0; s < ks; ++s) {
    const int b = 2 * s + h;
    const float x = (inside && b < B) ? row[b] : 0.0f;
    own = fmaf(x, x, own);
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(image[((size_t)t * ks + s) * 64 + lane], x, acc[t], 0, 0, 0);
  }
  return own;
}

template <int T>
__global__ __launch_bounds__(SP_THREADS, 1) void sparse_kernel(const float* __restrict__ spectra, int64_t stride, int64_t R,
                                                             const float* __restrict__ q_image, const float* __restrict__ m_image,
                                                             const float* __restrict__ a_image, const float* __restrict__ g_image, int L,
                                                             int B, float theta, float epsilon, int max_iterations,
                                                             float* __restrict__ abundances, float* __restrict__ residual,
                                                             int* __restrict__ status) {
  extern __shared__ v4f sM[];  // [to][ti][e / 4][lane] x 4
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5, ks = lib_ksteps(B);
  {
    float* dst = reinterpret_cast<float*>(sM);
    for (int i = tid; i < sp_image_floats(T); i += SP_THREADS) dst[i] = m_image[i];
  }
  __syncthreads();  // the only barrier: from here on a wave is on its own
  const int64_t r = ((int64_t)blockIdx.x * (SP_THREADS / 64) + (tid >> 6)) * 32 + j;
  const bool inside = r < R;
  const float* row = spectra + (inside ? r : 0) * stride;

  v16f c[T], z[T], d[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) c[t][e] = 0.0f, z[t][e] = 0.0f, d[t][e] = 0.0f;
  const float own = sp_band_products<T>(q_image, row, inside, B, ks, lane, h, c);
  const float other = __shfl_xor(own, 32, 64);
  const float ss = h ? other + own : own + other;  // even + odd, the same bits on both lanes of a row
  const bool valid = inside && ss > 0.0f && ss <= SP_FLT_MAX;  // not 0, not NaN, not Inf
  float smax = 0.0f;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) smax = fmaxf(smax, fabsf(c[t][e]));
  smax = fmaxf(smax, __shfl_xor(smax, 32, 64));
  const float es = epsilon * smax, tau = theta * sqrtf(ss);

  bool done = !valid;
  int iterations = 0;
  for (int it = 1; it <= max_iterations; ++it) {
    if (__ballot(!done) == 0) break;
    v16f acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = c[t];
#pragma unroll
    for (int ti = 0; ti < T; ++ti)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = z[ti][4 * s4 + q] - d[ti][4 * s4 + q];
#pragma unroll
        for (int to = 0; to < T; ++to) {
          const v4f m = sM[((to * T + ti) * 4 + s4) * 64 + lane];
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(m[q], v[q], acc[to], 0, 0, 0);
        }
      }
    float primal = 0.0f, dual = 0.0f;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float a = acc[t][e], sum = a + d[t][e], u = sum - tau;
        const float zn = u > 0.0f ? u : 0.0f;
        const float dn = sum - zn;
        primal = fmaxf(primal, fabsf(a - zn));
        dual = fmaxf(dual, fabsf(zn - z[t][e]));
        z[t][e] = done ? z[t][e] : zn;
        d[t][e] = done ? d[t][e] : dn;
      }
    primal = fmaxf(primal, __shfl_xor(primal, 32, 64));
    dual = fmaxf(dual, __shfl_xor(dual, 32, 64));
    if (!done) {
      iterations = it;
      done = primal <= es && dual <= es;
    }
  }

#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float a = z[t][e];
      z[t][e] = (valid && a > 0.0f && a <= SP_FLT_MAX) ? a : 0.0f;  // finite and >= +0, whatever happened above
      const int k = 32 * t + lib_acc_row(e, h);
      if (abundances && inside && k < L) abundances[r * L + k] = z[t][e];
    }
  if (status && inside && h == 0) status[r] = !valid ? -1 : done ? iterations : -2;
  if (!residual) return;

  v16f acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
  sp_band_products<T>(a_image, row, inside, B, ks, lane, h, acc);
  float p = 0.0f, q = 0.0f;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      p = fmaf(acc[t][e], z[t][e], p);
      acc[t][e] = 0.0f;
    }
#pragma unroll
  for (int ti = 0; ti < T; ++ti)
#pragma unroll
    for (int e = 0; e < 16; ++e)
#pragma unroll
      for (int to = 0; to < T; ++to)
        acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(g_image[(((to * T + ti) * 4 + (e >> 2)) * 64 + lane) * 4 + (e & 3)], z[ti][e], acc[to], 0,
                                                       0, 0);
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) q = fmaf(z[t][e], acc[t][e], q);
  const float po = __shfl_xor(p, 32, 64), qo = __shfl_xor(q, 32, 64);
  const float ps = h ? po + p : p + po, qs = h ? qo + q : q + qo;
  if (inside && h == 0) residual[r] = valid ? fmaxf(0.0f, fmaf(-2.0f, ps, ss) + qs) : 0.0f;
}

template <int T>
void sparse_launch(const float* spectra, int64_t stride, int64_t R, const float* q_image, const float* m_image, const float* a_image,
                   const float* g_image, int L, int B, float theta, float epsilon, int max_iterations, float* abundances, float* residual,
                   int* status, hipStream_t stream) {
  hipLaunchKernelGGL((sparse_kernel<T>), dim3((unsigned)((R + 127) / 128)), dim3(SP_THREADS), sp_image_floats(T) * sizeof(float), stream,
                     spectra, stride, R, q_image, m_image, a_image, g_image, L, B, theta, epsilon, max_iterations, abundances, residual,
                     status);
}

}  // namespace

extern "C" size_t umhs_sparse_image_bytes(int n_entries) {
  if (n_entries < 1 || n_entries > SP_MAX_L) return 0;
  return (size_t)sp_image_floats(lib_tiles(n_entries)) * sizeof(float);
}

extern "C" int umhs_sparse_prepare(const float* matrix, int n_entries, float* image, umhs_stream_t stream) {
  if (n_entries < 1) return UMHS_ERR_ARG;
  if (n_entries > SP_MAX_L) return UMHS_ERR_UNSUPPORTED;
  if (!matrix || !image) return UMHS_ERR_ARG;
  const int T = lib_tiles(n_entries);
  hipLaunchKernelGGL(sparse_prepare_kernel, dim3((unsigned)((sp_image_floats(T) + 255) / 256)), dim3(256), 0, umhs_s(stream), matrix,
                     n_entries, T, image);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_sparse_unmix(const float* spectra, int64_t stride, int64_t n_rows, const float* q_image, const float* m_image,
                                 const float* a_image, const float* g_image, int n_entries, int n_bands, float theta, float epsilon,
                                 int max_iterations, float* abundances, float* residual, int32_t* status, umhs_stream_t stream) {
  if (n_bands < 1 || n_entries < 1 || n_rows < 0 || stride < n_bands || max_iterations < 1 || !(epsilon > 0.0f) || !(theta >= 0.0f))
    return UMHS_ERR_ARG;
  if (n_bands > LIB_MAX_BANDS || n_entries > SP_MAX_L) return UMHS_ERR_UNSUPPORTED;
  if (n_rows == 0) return UMHS_OK;
  if (!spectra || !q_image || !m_image || (residual && (!a_image || !g_image))) return UMHS_ERR_ARG;
  if ((n_rows + 127) / 128 > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  hipStream_t s = umhs_s(stream);
#define SPARSE_CASE(T)                                                                                                                   \
  sparse_launch<T>(spectra, stride, n_rows, q_image, m_image, a_image, g_image, n_entries, n_bands, theta, epsilon, max_iterations, \
                   abundances, residual, status, s);
  switch (lib_tiles(n_entries)) {
    case 1: SPARSE_CASE(1) break;
    case 2: SPARSE_CASE(2) break;
    case 3: SPARSE_CASE(3) break;
    default: SPARSE_CASE(4) break;
  }
#undef SPARSE_CASE
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
