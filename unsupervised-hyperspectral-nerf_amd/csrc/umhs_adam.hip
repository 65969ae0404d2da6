// gfx950 kernels for the fused Adam step over the flat "fields" parameter buffer: dense, selected rows, rows + a dense range.
// The update expression is in umhs_adam.h, shared with the hash grid's backward.
#include "umhs_adam.h"

// Dense: the flat "fields" parameter buffer (28 B/param of pure HBM streaming, float4 lanes)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr_bc1,
                                                   float b1, float b2, float eps, float sqrt_bc2, float gscale,
                                                   int64_t cb, int64_t ce) {
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      float4 pp = *reinterpret_cast<float4*>(p + i), gg = *reinterpret_cast<const float4*>(g + i);
      float4 mm = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
      float* pa = reinterpret_cast<float*>(&pp);
      float* ga = reinterpret_cast<float*>(&gg);
      float* ma = reinterpret_cast<float*>(&mm);
      float* va = reinterpret_cast<float*>(&vv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        adam_update(pa[k], ma[k], va[k], ga[k] * gscale, lr_bc1, b1, b2, eps, sqrt_bc2);
        if (i + k >= cb && i + k < ce) pa[k] = adam_clamp01(pa[k]);
      }
      *reinterpret_cast<float4*>(p + i) = pp;
      *reinterpret_cast<float4*>(m + i) = mm;
      *reinterpret_cast<float4*>(v + i) = vv;
    } else {
      for (int64_t j = i; j < n; ++j) {
        float mk = m[j], vk = v[j], pk = p[j];
        adam_update(pk, mk, vk, g[j] * gscale, lr_bc1, b1, b2, eps, sqrt_bc2);
        if (j >= cb && j < ce) pk = adam_clamp01(pk);
        p[j] = pk, m[j] = mk, v[j] = vk;
      }
    }
  }
}

// Adam on selected 2-float rows only (the live rows of the sparse coarse hash levels: every other row of those levels has
// g = m = v = 0 for ever, so its update is exactly zero and it is not touched).  Same arithmetic as adam_kernel.
__global__ __launch_bounds__(256) void adam_rows_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, const int64_t* __restrict__ rows, int64_t n_rows,
                                                        float lr_bc1, float b1, float b2, float eps, float sqrt_bc2, float gscale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t o = rows[i] * 2;
  float2 pp = *reinterpret_cast<float2*>(p + o), mm = *reinterpret_cast<float2*>(m + o), vv = *reinterpret_cast<float2*>(v + o);
  const float2 gg = *reinterpret_cast<const float2*>(g + o);
  float* pa = reinterpret_cast<float*>(&pp);
  float* ma = reinterpret_cast<float*>(&mm);
  float* va = reinterpret_cast<float*>(&vv);
  const float ga[2] = {gg.x, gg.y};
#pragma unroll
  for (int k = 0; k < 2; ++k) adam_update(pa[k], ma[k], va[k], ga[k] * gscale, lr_bc1, b1, b2, eps, sqrt_bc2);
  *reinterpret_cast<float2*>(p + o) = pp;
  *reinterpret_cast<float2*>(m + o) = mm;
  *reinterpret_cast<float2*>(v + o) = vv;
}

extern "C" int umhs_adam_step_rows(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* rows,
                                   int64_t n_rows, float lr, float beta1, float beta2, float eps, int64_t step,
                                   float grad_scale, umhs_stream_t stream) {
  if (n_rows < 0 || step < 1 || !params || !grads || !exp_avg || !exp_avg_sq || (n_rows > 0 && !rows)) return UMHS_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 7) return UMHS_ERR_ARG;
  if (n_rows == 0) return UMHS_OK;
  const AdamBias bc = adam_bias(lr, beta1, beta2, step);
  hipLaunchKernelGGL(adam_rows_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, umhs_s(stream), params, grads,
                     exp_avg, exp_avg_sq, rows, n_rows, bc.lr_bc1, beta1, beta2, eps, bc.sqrt_bc2, grad_scale);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// adam_rows_kernel and adam_kernel in one launch: the first row_blocks workgroups take the rows, the others the dense range
// [t0, t0 + tn) (what is left for the optimizer when the dense hash levels were updated inside the backward: the live rows of the
// coarse levels and the MLP / endmember tail -- two ~6 us launches at the very end of the step).
__global__ __launch_bounds__(256) void adam_rows_range_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, const int64_t* __restrict__ rows, int64_t n_rows,
                                                              int row_blocks, int64_t t0, int64_t tn, float lr_bc1, float b1, float b2,
                                                              float eps, float sqrt_bc2, float gscale, int64_t cb, int64_t ce) {
  if ((int)blockIdx.x < row_blocks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t o = rows[i] * 2;
    float2 pp = *reinterpret_cast<float2*>(p + o), mm = *reinterpret_cast<float2*>(m + o), vv = *reinterpret_cast<float2*>(v + o);
    const float2 gg = *reinterpret_cast<const float2*>(g + o);
    adam_update(pp.x, mm.x, vv.x, gg.x * gscale, lr_bc1, b1, b2, eps, sqrt_bc2);
    adam_update(pp.y, mm.y, vv.y, gg.y * gscale, lr_bc1, b1, b2, eps, sqrt_bc2);
    *reinterpret_cast<float2*>(p + o) = pp;
    *reinterpret_cast<float2*>(m + o) = mm;
    *reinterpret_cast<float2*>(v + o) = vv;
    return;
  }
  const int64_t nblk = (int64_t)gridDim.x - row_blocks;
  for (int64_t j = (((int64_t)blockIdx.x - row_blocks) * 256 + threadIdx.x); j < tn; j += nblk * 256) {
    const int64_t e = t0 + j;
    float pk = p[e], mk = m[e], vk = v[e];
    adam_update(pk, mk, vk, g[e] * gscale, lr_bc1, b1, b2, eps, sqrt_bc2);
    if (e >= cb && e < ce) pk = adam_clamp01(pk);
    p[e] = pk, m[e] = mk, v[e] = vk;
  }
}

extern "C" int umhs_adam_step_rows_range(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* rows,
                                         int64_t n_rows, int64_t range_begin, int64_t range_count, float lr, float beta1, float beta2,
                                         float eps, int64_t step, float grad_scale, int64_t clamp_begin, int64_t clamp_end,
                                         umhs_stream_t stream) {
  if (n_rows < 0 || range_begin < 0 || range_count < 0 || step < 1 || !params || !grads || !exp_avg || !exp_avg_sq ||
      (n_rows > 0 && !rows))
    return UMHS_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 7) return UMHS_ERR_ARG;
  if (n_rows == 0 && range_count == 0) return UMHS_OK;
  const AdamBias bc = adam_bias(lr, beta1, beta2, step);
  const int64_t row_blocks = (n_rows + 255) / 256;
  int64_t range_blocks = (range_count + 255) / 256;
  if (range_blocks > 1024) range_blocks = 1024;
  if (row_blocks + range_blocks > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(adam_rows_range_kernel, dim3((unsigned)(row_blocks + range_blocks)), dim3(256), 0, umhs_s(stream), params, grads,
                     exp_avg, exp_avg_sq, rows, n_rows, (int)row_blocks, range_begin, range_count, bc.lr_bc1, beta1, beta2, eps,
                     bc.sqrt_bc2, grad_scale, clamp_begin, clamp_end);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                              float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                              int64_t clamp_begin, int64_t clamp_end, umhs_stream_t stream) {
  if (n < 0 || step < 1 || !params || !grads || !exp_avg || !exp_avg_sq) return UMHS_ERR_ARG;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  const AdamBias bc = adam_bias(lr, beta1, beta2, step);
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, umhs_s(stream), params, grads, exp_avg,
                     exp_avg_sq, n, bc.lr_bc1, beta1, beta2, eps, bc.sqrt_bc2, grad_scale, clamp_begin, clamp_end);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
