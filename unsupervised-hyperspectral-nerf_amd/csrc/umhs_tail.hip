// gfx950 kernels for the per-ray end of the UMHS step: spectrum->sRGB fwd/bwd (R14), the ray epilogue, the losses and the fused
// training tail (R14-R16).  Reference citations are in include/umhs_hip.h.
#include "umhs_common.h"

// =============================================================================================
// R14: spectrum -> sRGB (one thread per ray; M [B,3] is tiny and stays in L1/scalar cache)
// =============================================================================================
#define GAMMA_KNEE 0.0031308f

__device__ __forceinline__ float srgb_gamma(float x) {
  return x < GAMMA_KNEE ? 12.92f * x : 1.055f * powf(fmaxf(x, 1e-6f), 1.0f / 2.4f) - 0.055f;
}

__global__ __launch_bounds__(256) void spec2rgb_fwd_kernel(const float* __restrict__ spec,
                                                           const float* __restrict__ M, int64_t n_rays, int B,
                                                           float* __restrict__ rgb) {
  int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  const float* row = spec + r * B;
  float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
  for (int b = 0; b < B; ++b) {
    float s = row[b];
    x0 += s * M[3 * b], x1 += s * M[3 * b + 1], x2 += s * M[3 * b + 2];
  }
  rgb[3 * r] = fminf(fmaxf(srgb_gamma(x0), 0.0f), 1.0f);
  rgb[3 * r + 1] = fminf(fmaxf(srgb_gamma(x1), 0.0f), 1.0f);
  rgb[3 * r + 2] = fminf(fmaxf(srgb_gamma(x2), 0.0f), 1.0f);
}

__device__ __forceinline__ float srgb_gamma_grad(float x) {
  // d/dx of clamp(gamma(x), 0, 1): torch passes the clamp gradient where 0 <= y <= 1
  float y = srgb_gamma(x);
  if (!(y >= 0.0f && y <= 1.0f)) return 0.0f;
  if (x < GAMMA_KNEE) return 12.92f;
  return 1.055f * (1.0f / 2.4f) * powf(fmaxf(x, 1e-6f), 1.0f / 2.4f - 1.0f);
}

__global__ __launch_bounds__(256) void spec2rgb_bwd_kernel(const float* __restrict__ spec,
                                                           const float* __restrict__ M,
                                                           const float* __restrict__ d_rgb, int64_t n_rays, int B,
                                                           float* __restrict__ d_spec, int accumulate) {
  int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  const float* row = spec + r * B;
  float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
  for (int b = 0; b < B; ++b) {
    float s = row[b];
    x0 += s * M[3 * b], x1 += s * M[3 * b + 1], x2 += s * M[3 * b + 2];
  }
  float g0 = d_rgb[3 * r] * srgb_gamma_grad(x0);
  float g1 = d_rgb[3 * r + 1] * srgb_gamma_grad(x1);
  float g2 = d_rgb[3 * r + 2] * srgb_gamma_grad(x2);
  float* drow = d_spec + r * B;
  for (int b = 0; b < B; ++b) {
    float v = g0 * M[3 * b] + g1 * M[3 * b + 1] + g2 * M[3 * b + 2];
    drow[b] = accumulate ? drow[b] + v : v;
  }
}

extern "C" int umhs_spec2rgb_fwd(const float* spec, const float* M, int64_t n_rays, int B, float* rgb,
                                 umhs_stream_t stream) {
  if (n_rays < 0 || B < 1 || !spec || !M || !rgb) return UMHS_ERR_ARG;
  if (n_rays == 0) return UMHS_OK;
  hipLaunchKernelGGL(spec2rgb_fwd_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), spec,
                     M, n_rays, B, rgb);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_spec2rgb_bwd(const float* spec, const float* M, const float* d_rgb, int64_t n_rays, int B,
                                 float* d_spec, int accumulate, umhs_stream_t stream) {
  if (n_rays < 0 || B < 1 || !spec || !M || !d_rgb || !d_spec) return UMHS_ERR_ARG;
  if (n_rays == 0) return UMHS_OK;
  hipLaunchKernelGGL(spec2rgb_bwd_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), spec,
                     M, d_rgb, n_rays, B, d_spec, accumulate);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// =============================================================================================
// R14-R16 fused per-ray epilogue and loss.  The reference runs ~85 tiny torch kernels per step for these
// (depth clip with a global min/max, ColourSystem, ClusterLookup + argmax + label colours, random-background
// blend, two MSE losses and their autograd); here they are one forward kernel each and the loss kernel also
// writes the gradients of both losses (the upstream gradient of a loss is a scalar, applied by the caller).
// =============================================================================================
__device__ __forceinline__ uint32_t f2ord(float f) {  // order-preserving float -> uint (for atomicMin/Max)
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// min/max of the sample mid-points t_mid = (t0+t1)/2 over the whole batch (DepthRenderer's clip bounds)
__global__ __launch_bounds__(256) void tmid_minmax_kernel(const float* __restrict__ t0, const float* __restrict__ t1, int64_t n,
                                                          uint32_t* __restrict__ mm) {
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float m = (t0[i] + t1[i]) / 2.0f;
    lo = fminf(lo, m), hi = fmaxf(hi, m);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) lo = fminf(lo, __shfl_xor(lo, d, 64)), hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  __shared__ float plo[4], phi[4];
  if ((threadIdx.x & 63) == 0) plo[threadIdx.x >> 6] = lo, phi[threadIdx.x >> 6] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {  // one atomic pair per workgroup (memory-side atomics on two words serialise)
    atomicMin(&mm[0], f2ord(fminf(fminf(plo[0], plo[1]), fminf(plo[2], plo[3]))));
    atomicMax(&mm[1], f2ord(fmaxf(fmaxf(phi[0], phi[1]), fmaxf(phi[2], phi[3]))));
  }
}

__global__ void tmid_init_kernel(uint32_t* mm) { mm[0] = 0xffffffffu, mm[1] = 0u; }

extern "C" int umhs_tmid_minmax(const float* t_starts, const float* t_ends, int64_t n, float* minmax2, umhs_stream_t stream) {
  if (n < 0 || !minmax2 || (n > 0 && (!t_starts || !t_ends))) return UMHS_ERR_ARG;
  // identity of (min, max) in the ordered encoding; a 1-thread kernel, not a host-to-device copy of a stack variable (that blit
  // queued behind whatever else the device was running: 70 us on a side stream)
  hipLaunchKernelGGL(tmid_init_kernel, dim3(1), dim3(1), 0, umhs_s(stream), reinterpret_cast<uint32_t*>(minmax2));
  if (n == 0) {
    UMHS_CHECK_LAUNCH();
    return UMHS_OK;
  }
  // (one atomic pair per workgroup: 512 same-line device atomics serialise at ~12 ns each = ~6 us behind the kernel's 2 MB read, on the
  // side stream.  Fewer, longer workgroups were tried in round 4 -- 32 x 8192 elements: 63 us at C2 and 1 ms on an eval image's 18 M
  // candidates, a serial chain of loads per thread -- and reverted.)
  int64_t blocks = (n + 2047) / 2048;
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(tmid_minmax_kernel, dim3((unsigned)blocks), dim3(256), 0, umhs_s(stream), t_starts, t_ends, n,
                     reinterpret_cast<uint32_t*>(minmax2));
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// one thread per ray: rgb = ColourSystem(spectral); depth clip; ClusterLookup(alpha) against the endmembers;
// seg_raw = argmax * [acc > 0.5]; seg_pred = class colour * [acc > 0.5]
__global__ __launch_bounds__(256) void ray_epilogue_kernel(const float* __restrict__ spec, const float* __restrict__ M,
                                                           const float* __restrict__ E, const float* __restrict__ acc,
                                                           const float* __restrict__ depth_in, const uint32_t* __restrict__ mm,
                                                           const float* __restrict__ colors, int64_t n_rays, int B, int C,
                                                           float alpha, float* __restrict__ rgb, float* __restrict__ depth_out,
                                                           float* __restrict__ seg_probs, float* __restrict__ seg_raw,
                                                           float* __restrict__ seg_pred) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  const float* row = spec + r * B;
  float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, ss = 0.0f;
  float ip[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) ip[c] = 0.0f;
  for (int b = 0; b < B; ++b) {
    const float s = row[b];
    x0 += s * M[3 * b], x1 += s * M[3 * b + 1], x2 += s * M[3 * b + 2];
    ss += s * s;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < C) ip[c] += s * E[c * B + b];
  }
  if (rgb) {
    rgb[3 * r] = fminf(fmaxf(srgb_gamma(x0), 0.0f), 1.0f);
    rgb[3 * r + 1] = fminf(fmaxf(srgb_gamma(x1), 0.0f), 1.0f);
    rgb[3 * r + 2] = fminf(fmaxf(srgb_gamma(x2), 0.0f), 1.0f);
  }
  if (depth_out) depth_out[r] = fminf(fmaxf(depth_in[r], ord2f(mm[0])), ord2f(mm[1]));
  if (seg_probs) {
    // F.normalize: x / max(||x||, 1e-12) for the ray spectrum and for every endmember row (utils/clusterprobe.py:20-25)
    const float inv_x = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    float mx = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      if (c < C) {
        float ee = 0.0f;
        for (int b = 0; b < B; ++b) ee += E[c * B + b] * E[c * B + b];
        ip[c] = ip[c] * inv_x / fmaxf(sqrtf(ee), 1e-12f);
        if (ip[c] > mx) mx = ip[c], arg = c;
      }
    }
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < C) ip[c] = expf(alpha * (ip[c] - mx)), sum += ip[c];
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c < C) seg_probs[r * C + c] = ip[c] / sum;
    const float on = acc[r] > 0.5f ? 1.0f : 0.0f;
    if (seg_raw) seg_raw[r] = (float)arg * on;
    if (seg_pred) {
      seg_pred[3 * r] = colors[3 * arg] * on, seg_pred[3 * r + 1] = colors[3 * arg + 1] * on;
      seg_pred[3 * r + 2] = colors[3 * arg + 2] * on;
    }
  }
}

extern "C" int umhs_ray_epilogue_fwd(const float* spectral, const float* M, const float* endmembers, const float* accumulation,
                                     const float* depth, const float* tmid_minmax2, const float* class_colors, int64_t n_rays,
                                     int n_bands, int n_classes, float alpha, float* rgb, float* depth_clipped, float* seg_probs,
                                     float* seg_raw, float* seg_pred, umhs_stream_t stream) {
  if (n_rays < 0 || n_bands < 1 || !spectral || !M) return UMHS_ERR_ARG;
  if (seg_probs && (!endmembers || !accumulation || n_classes < 1)) return UMHS_ERR_ARG;
  if (seg_pred && !class_colors) return UMHS_ERR_ARG;
  if (depth_clipped && (!depth || !tmid_minmax2)) return UMHS_ERR_ARG;
  if (n_classes > 16) return UMHS_ERR_UNSUPPORTED;
  if (n_rays == 0) return UMHS_OK;
  hipLaunchKernelGGL(ray_epilogue_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), spectral, M,
                     endmembers, accumulation, depth, reinterpret_cast<const uint32_t*>(tmid_minmax2), class_colors, n_rays,
                     n_bands, n_classes, alpha, rgb, depth_clipped, seg_probs, seg_raw, seg_pred);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// losses[0] = w_spec * mean((spec - gt_spec)^2)             (umhs_model.py:366-369)
// losses[1] = w_rgb  * mean((rgb + bg*(1-acc) - gt_rgb)^2)  (umhs_model.py:358-370, random background blend)
// Forward call: losses != NULL, d_* == NULL.  Backward call: d_* != NULL, g_up = upstream gradients of the two
// losses (device [2], NULL = 1): writes d_spec [R,B], d_rgb [R,3], d_acc [R].  One wave per ray.
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ spec, const float* __restrict__ gt_spec,
                                                   const float* __restrict__ rgb, const float* __restrict__ acc,
                                                   const float* __restrict__ bg, const float* __restrict__ gt_rgb,
                                                   int64_t n_rays, int B, float w_spec, float w_rgb,
                                                   const float* __restrict__ g_up, float* __restrict__ losses,
                                                   float* __restrict__ d_spec, float* __restrict__ d_rgb,
                                                   float* __restrict__ d_acc) {
  const int lane = threadIdx.x & 63;
  float ls = 0.0f, lr = 0.0f;
  const float gs = g_up ? g_up[0] : 1.0f, gr = g_up ? g_up[1] : 1.0f;
  const float cs = gs * w_spec * 2.0f / ((float)n_rays * (float)B);
  for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < n_rays; r0 += (int64_t)gridDim.x * 4) {  // wave-uniform trip count
    const int64_t r = r0 + (threadIdx.x >> 6);
    const bool live = r < n_rays;
    float ga = 0.0f;
    if (live) {
      for (int b = lane; b < B; b += 64) {
        const float d = spec[r * B + b] - gt_spec[r * B + b];
        ls += d * d;
        if (d_spec) d_spec[r * B + b] = cs * d;
      }
      if (rgb && lane < 3) {
        const float beta = bg ? bg[3 * r + lane] : 0.0f;
        const float d = rgb[3 * r + lane] + beta * (1.0f - acc[r]) - gt_rgb[3 * r + lane];
        lr += d * d;
        const float g = gr * w_rgb * 2.0f / ((float)n_rays * 3.0f) * d;
        if (d_rgb) d_rgb[3 * r + lane] = g;
        ga = -g * beta;  // d/d acc of beta*(1-acc)
      }
    }
    ga = wave_reduce_sum(ga);
    if (live && rgb && d_acc && lane == 0) d_acc[r] = ga;
  }
  if (!losses) return;
  ls = wave_reduce_sum(ls), lr = wave_reduce_sum(lr);
  __shared__ float part[2][4];
  if (lane == 0) part[0][threadIdx.x >> 6] = ls, part[1][threadIdx.x >> 6] = lr;
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&losses[0], (part[0][0] + part[0][1] + part[0][2] + part[0][3]) * (w_spec / ((float)n_rays * (float)B)));
    if (rgb) atomicAdd(&losses[1], (part[1][0] + part[1][1] + part[1][2] + part[1][3]) * (w_rgb / ((float)n_rays * 3.0f)));
  }
}

extern "C" int umhs_loss_fwd(const float* spectral, const float* gt_spectral, const float* rgb, const float* accumulation,
                             const float* background, const float* gt_rgb, int64_t n_rays, int n_bands, float w_spectral,
                             float w_rgb, float* losses2, umhs_stream_t stream) {
  if (n_rays < 1 || n_bands < 1 || !spectral || !gt_spectral || !losses2) return UMHS_ERR_ARG;
  if (rgb && (!accumulation || !gt_rgb)) return UMHS_ERR_ARG;
  if (hipMemsetAsync(losses2, 0, 8, umhs_s(stream)) != hipSuccess) return UMHS_ERR_LAUNCH;
  hipLaunchKernelGGL(loss_kernel, dim3((unsigned)((n_rays + 3) / 4 < 256 ? (n_rays + 3) / 4 : 256)), dim3(256), 0,
                     umhs_s(stream), spectral, gt_spectral, rgb, accumulation, background, gt_rgb, n_rays, n_bands,
                     w_spectral, w_rgb, (const float*)nullptr,
                     losses2, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_loss_bwd(const float* spectral, const float* gt_spectral, const float* rgb, const float* accumulation,
                             const float* background, const float* gt_rgb, int64_t n_rays, int n_bands, float w_spectral,
                             float w_rgb, const float* grad_losses2, float* d_spectral, float* d_rgb, float* d_accumulation,
                             umhs_stream_t stream) {
  if (n_rays < 1 || n_bands < 1 || !spectral || !gt_spectral || !d_spectral) return UMHS_ERR_ARG;
  if (rgb && (!accumulation || !gt_rgb || !d_rgb || !d_accumulation)) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(loss_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, umhs_s(stream), spectral, gt_spectral,
                     rgb, accumulation, background, gt_rgb, n_rays, n_bands, w_spectral, w_rgb, grad_losses2,
                     (float*)nullptr, d_spectral, d_rgb, d_accumulation);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// =============================================================================================
// Training tail of one step, fused: ray epilogue (rgb, depth clip, cluster probe) + both losses + their backward down to
// d_spectral / d_accumulation (loss_bwd with unit upstream gradients + spec2rgb_bwd).  Four launches of per-ray work on
// R = 4096 rays (16 workgroups each, ~60 us together, almost all of it latency) become one with 16 lanes per ray.
// Loss sums: per-block partials, added in block order by the last block to finish (reproducible); the arrival counter
// in `scratch` is left at zero again.
// =============================================================================================
__device__ __forceinline__ float red16(float v) {  // sum over the 16 lanes of a ray group (= a DPP row), result in every lane
  // four rotate-and-add steps on the VALU (v_add_f32_dpp row_ror:8/4/2/1); __shfl_xor compiles to ds_bpermute here, an LDS round
  // trip per step in kernels that are nothing but chains of such reductions
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));
  return v;
}

struct TailArgs {
  const float *spec, *M, *E, *acc, *depth, *colors, *gt_spec, *gt_rgb, *bg;
  const uint32_t* mm;
  int64_t n_rays;
  int B, C, rgb_loss;
  float alpha, w_spec, w_rgb;
  float *rgb, *depth_out, *seg_probs, *seg_raw, *seg_pred, *losses, *d_spec, *d_acc;
  float* partial;     // [gridDim.x][2]
  uint32_t* counter;  // zero on entry, zero on exit
};

__global__ __launch_bounds__(256) void ray_train_tail_kernel(TailArgs a) {
  __shared__ float ee_inv[16];
  __shared__ float part[2][16];
  __shared__ bool last;
  const int tid = threadIdx.x, l = tid & 15, grp = tid >> 4;
  const int B = a.B, C = a.C;
  {  // 1 / max(||E_c||, 1e-12): F.normalize of the endmember rows (clusterprobe.py:20-25), once per block, 16 lanes per class
    float ee = 0.0f;
    if (grp < C)
      for (int b = l; b < B; b += 16) ee += a.E[grp * B + b] * a.E[grp * B + b];
    ee = red16(ee);
    if (l == 0) ee_inv[grp] = 1.0f / fmaxf(sqrtf(ee), 1e-12f);
  }
  __syncthreads();
  const float cs = a.w_spec * 2.0f / ((float)a.n_rays * (float)B);
  const float cr = a.w_rgb * 2.0f / ((float)a.n_rays * 3.0f);
  const float tlo = ord2f(a.mm[0]), thi = ord2f(a.mm[1]);
  float ls = 0.0f, lr = 0.0f;
  for (int64_t r0 = (int64_t)blockIdx.x * 16; r0 < a.n_rays; r0 += (int64_t)gridDim.x * 16) {  // block-uniform trip count
    const int64_t r = r0 + grp;
    const bool live = r < a.n_rays;
    const int64_t rc = live ? r : a.n_rays - 1;
    const float* row = a.spec + rc * B;
    const float* grow = a.gt_spec + rc * B;
    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, ss = 0.0f, dl = 0.0f;
    float ip[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) ip[c] = 0.0f;
    for (int b = l; b < B; b += 16) {
      const float s = row[b], d = s - grow[b];
      x0 += s * a.M[3 * b], x1 += s * a.M[3 * b + 1], x2 += s * a.M[3 * b + 2];
      ss += s * s, dl += d * d;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < C) ip[c] += s * a.E[c * B + b];
    }
    x0 = red16(x0), x1 = red16(x1), x2 = red16(x2), ss = red16(ss);
    if (live) ls += dl;  // per-lane partial; reduced once at the end
    const float x[3] = {x0, x1, x2};
    float rgbv[3], g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k) rgbv[k] = fminf(fmaxf(srgb_gamma(x[k]), 0.0f), 1.0f);
    const float accv = a.acc[rc];
    if (a.rgb_loss) {
      float ga = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float beta = a.bg ? a.bg[3 * rc + k] : 0.0f;
        const float d = rgbv[k] + beta * (1.0f - accv) - a.gt_rgb[3 * rc + k];
        if (live && l == 0) lr += d * d;
        const float gk = cr * d;
        ga -= gk * beta;
        g[k] = gk * srgb_gamma_grad(x[k]);
      }
      if (live && l == 0 && a.d_acc) a.d_acc[r] = ga;
    }
    if (live) {
      float* drow = a.d_spec + r * B;
      for (int b = l; b < B; b += 16)
        drow[b] = cs * (row[b] - grow[b]) + (g[0] * a.M[3 * b] + g[1] * a.M[3 * b + 1] + g[2] * a.M[3 * b + 2]);
      if (l < 3 && a.rgb) a.rgb[3 * r + l] = rgbv[l];
      if (l == 3 && a.depth_out) a.depth_out[r] = fminf(fmaxf(a.depth[r], tlo), thi);
    }
    if (a.seg_probs) {
      const float inv_x = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
      float mx = -INFINITY, mine = 0.0f;
      int arg = 0;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        if (c < C) {
          const float v = red16(ip[c]) * inv_x * ee_inv[c];
          if (v > mx) mx = v, arg = c;
          if (c == l) mine = v;
        }
      }
      const float e = l < C ? expf(a.alpha * (mine - mx)) : 0.0f;
      const float sum = red16(e);
      if (live) {
        if (l < C) a.seg_probs[r * C + l] = e / sum;
        const float on = accv > 0.5f ? 1.0f : 0.0f;
        if (l == 0 && a.seg_raw) a.seg_raw[r] = (float)arg * on;
        if (l < 3 && a.seg_pred) a.seg_pred[3 * r + l] = a.colors[3 * arg + l] * on;
      }
    }
  }
  ls = red16(ls), lr = red16(lr);
  if (l == 0) part[0][grp] = ls, part[1][grp] = lr;
  __syncthreads();
  if (tid == 0) {
    float s0 = 0.0f, s1 = 0.0f;
    for (int i = 0; i < 16; ++i) s0 += part[0][i], s1 += part[1][i];
    a.partial[2 * blockIdx.x] = s0, a.partial[2 * blockIdx.x + 1] = s1;
    __threadfence();
    last = atomicAdd(a.counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (last) {  // block-wide tree over the (<= 256) partials: fixed order, no serial chain of L2 round trips
    __threadfence();
    float s0 = 0.0f, s1 = 0.0f;
    for (unsigned i = tid; i < gridDim.x; i += 256) s0 += a.partial[2 * i], s1 += a.partial[2 * i + 1];  // (<= 1024 partials)
    s0 = red16(s0), s1 = red16(s1);
    __syncthreads();
    if (l == 0) part[0][grp] = s0, part[1][grp] = s1;
    __syncthreads();
    if (tid == 0) {
      s0 = 0.0f, s1 = 0.0f;
      for (int i = 0; i < 16; ++i) s0 += part[0][i], s1 += part[1][i];
      a.losses[0] = s0 * (a.w_spec / ((float)a.n_rays * (float)B));
      a.losses[1] = a.rgb_loss ? s1 * (a.w_rgb / ((float)a.n_rays * 3.0f)) : 0.0f;
      *a.counter = 0u;
    }
  }
}

constexpr int TAIL_MAX_BLOCKS = 1024;  // 16 rays per workgroup iteration: up to 16 k rays get a workgroup each (4 resident per CU)
extern "C" size_t umhs_ray_train_tail_scratch_bytes(void) { return TAIL_MAX_BLOCKS * 2 * sizeof(float) + 64; }

extern "C" int umhs_ray_train_tail(const float* spectral, const float* M, const float* endmembers, const float* accumulation,
                                   const float* depth, const float* tmid_minmax2, const float* class_colors,
                                   const float* gt_spectral, const float* gt_rgb, const float* background, int64_t n_rays,
                                   int n_bands, int n_classes, float alpha, float w_spectral, float w_rgb, int rgb_loss,
                                   float* rgb, float* depth_clipped, float* seg_probs, float* seg_raw, float* seg_pred,
                                   float* losses2, float* d_spectral, float* d_accumulation, void* scratch,
                                   size_t scratch_bytes, umhs_stream_t stream) {
  if (n_rays < 1 || n_bands < 1 || !spectral || !M || !gt_spectral || !accumulation || !tmid_minmax2 || !losses2 || !d_spectral ||
      !scratch)
    return UMHS_ERR_ARG;
  if (rgb_loss && (!gt_rgb || !d_accumulation)) return UMHS_ERR_ARG;
  if (depth_clipped && !depth) return UMHS_ERR_ARG;
  if (seg_probs && (!endmembers || n_classes < 1)) return UMHS_ERR_ARG;
  if (seg_pred && (!class_colors || !seg_probs)) return UMHS_ERR_ARG;
  if (n_classes > 16) return UMHS_ERR_UNSUPPORTED;
  if (scratch_bytes < umhs_ray_train_tail_scratch_bytes() || ((uintptr_t)scratch & 3)) return UMHS_ERR_WORKSPACE;
  TailArgs a;
  a.spec = spectral, a.M = M, a.E = endmembers, a.acc = accumulation, a.depth = depth, a.colors = class_colors;
  a.gt_spec = gt_spectral, a.gt_rgb = gt_rgb, a.bg = background, a.mm = reinterpret_cast<const uint32_t*>(tmid_minmax2);
  a.n_rays = n_rays, a.B = n_bands, a.C = seg_probs ? n_classes : 0, a.rgb_loss = rgb_loss, a.alpha = alpha;
  a.w_spec = w_spectral, a.w_rgb = w_rgb, a.rgb = rgb, a.depth_out = depth_clipped, a.seg_probs = seg_probs;
  a.seg_raw = seg_raw, a.seg_pred = seg_pred, a.losses = losses2, a.d_spec = d_spectral, a.d_acc = d_accumulation;
  a.counter = reinterpret_cast<uint32_t*>(scratch), a.partial = reinterpret_cast<float*>(scratch) + 16;
  const int64_t blocks = (n_rays + 15) / 16;
  hipLaunchKernelGGL(ray_train_tail_kernel, dim3((unsigned)(blocks < TAIL_MAX_BLOCKS ? blocks : TAIL_MAX_BLOCKS)), dim3(256), 0,
                     umhs_s(stream), a);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
