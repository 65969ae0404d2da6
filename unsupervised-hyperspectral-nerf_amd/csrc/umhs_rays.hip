// gfx950 kernels for the packed ray samples of the UMHS hot path: sample positions (R1 prefix), pack_info, packed transmittance +
// per-ray band accumulation fwd/bwd (R11-R13).  No parameters live here.  Reference citations are in include/umhs_hip.h.
#include "umhs_common.h"

// =============================================================================================
// R1 prefix: positions
// =============================================================================================
__global__ __launch_bounds__(256) void positions_kernel(const float* __restrict__ origins,
                                                        const float* __restrict__ directions,
                                                        const float* __restrict__ starts,
                                                        const float* __restrict__ ends,
                                                        const float* __restrict__ world_in, int64_t n,
                                                        int contraction, float ax, float ay, float az, float bx,
                                                        float by, float bz, float* __restrict__ world_out,
                                                        float* __restrict__ pos01, float* __restrict__ selector) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float p[3];
  if (world_in) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = world_in[3 * i + c];
  } else {
    float t = starts[i] + ends[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = origins[3 * i + c] + directions[3 * i + c] * t / 2.0f;
  }
  if (world_out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) world_out[3 * i + c] = p[c];
  }
  float q[3];
  if (contraction) {
    float mag = fmaxf(fabsf(p[0]), fmaxf(fabsf(p[1]), fabsf(p[2])));
    if (mag < 1.0f) {
      q[0] = p[0], q[1] = p[1], q[2] = p[2];
    } else {
      float sc = 2.0f - (1.0f / mag);
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] = sc * (p[c] / mag);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = (q[c] + 2.0f) / 4.0f;
  } else {
    q[0] = (p[0] - ax) / (bx - ax);
    q[1] = (p[1] - ay) / (by - ay);
    q[2] = (p[2] - az) / (bz - az);
  }
  bool sel = q[0] > 0.0f && q[0] < 1.0f && q[1] > 0.0f && q[1] < 1.0f && q[2] > 0.0f && q[2] < 1.0f;
  float sf = sel ? 1.0f : 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) pos01[3 * i + c] = q[c] * sf;
  if (selector) selector[i] = sf;
}

extern "C" int umhs_positions_fwd(const float* origins, const float* directions, const float* starts,
                                  const float* ends, const float* world_pos_in, int64_t n, int contraction,
                                  const float* aabb, float* world_pos_out, float* pos01_out, float* selector_out,
                                  umhs_stream_t stream) {
  if (n < 0 || !pos01_out) return UMHS_ERR_ARG;
  if (!world_pos_in && (!origins || !directions || !starts || !ends)) return UMHS_ERR_ARG;
  if (!contraction && !aabb) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  float a[6] = {-1, -1, -1, 1, 1, 1};
  if (aabb)
    for (int i = 0; i < 6; ++i) a[i] = aabb[i];
  dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(positions_kernel, grid, dim3(256), 0, umhs_s(stream), origins, directions, starts, ends,
                     world_pos_in, n, contraction, a[0], a[1], a[2], a[3], a[4], a[5], world_pos_out, pos01_out,
                     selector_out);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// =============================================================================================
// R11: pack_info  (ray_indices sorted ascending -> (start, count) per ray, by binary search)
// =============================================================================================
__device__ __forceinline__ int64_t lower_bound_i64(const int64_t* a, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void pack_info_kernel(const int64_t* __restrict__ ray_indices, int64_t n,
                                                        int64_t n_rays, int64_t* __restrict__ packed) {
  int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  int64_t s = lower_bound_i64(ray_indices, n, r);
  int64_t e = lower_bound_i64(ray_indices, n, r + 1);
  packed[2 * r] = s;
  packed[2 * r + 1] = e - s;
}

extern "C" int umhs_pack_info(const int64_t* ray_indices, int64_t n, int64_t n_rays, int64_t* packed_info,
                              umhs_stream_t stream) {
  if (n < 0 || n_rays < 0 || !packed_info || (n > 0 && !ray_indices)) return UMHS_ERR_ARG;
  if (n_rays == 0) return UMHS_OK;
  hipLaunchKernelGGL(pack_info_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream),
                     ray_indices, n, n_rays, packed_info);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// =============================================================================================
// R11-R13: compositing.  One wavefront per ray; lane = sample for the transmittance scan (64-lane
// shuffle prefix sum with a carry across 64-sample chunks), then lane = band for the accumulation so
// every [N,K] row is read as one coalesced run.  Accumulation order is the sample order: results are
// bitwise reproducible (the reference's index_add_ is not).
// =============================================================================================
struct CompStreams {
  int n;
  int k[UMHS_MAX_STREAMS];
  const float* v[UMHS_MAX_STREAMS];
  float* out[UMHS_MAX_STREAMS];
};

__global__ __launch_bounds__(256) void composite_fwd_kernel(const float* __restrict__ sigma,
                                                            const float* __restrict__ t0,
                                                            const float* __restrict__ t1,
                                                            const int64_t* __restrict__ pinfo, int64_t n_rays,
                                                            CompStreams st, float* __restrict__ weights,
                                                            float* __restrict__ acc_out,
                                                            float* __restrict__ depth_out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (r >= n_rays) return;
  const int64_t start = pinfo[2 * r];
  const int cnt = (int)pinfo[2 * r + 1];
  float carry = 0.0f, acc = 0.0f, dnum = 0.0f;
  for (int base = 0; base < cnt || base == 0; base += 64) {
    const int i = base + lane;
    const bool valid = i < cnt;
    const int64_t nidx = start + i;
    float a = 0.0f, b = 0.0f, x = 0.0f;
    if (valid) {
      a = t0[nidx], b = t1[nidx];
      x = sigma[nidx] * (b - a);
    }
    float incl = wave_inclusive_scan(x, lane);
    float T = expf(-(carry + (incl - x)));
    float alpha = 1.0f - expf(-x);
    float w = valid ? alpha * T : 0.0f;
    if (valid) weights[nidx] = w;
    acc += w;
    dnum += w * ((a + b) / 2.0f);
    carry += __shfl(incl, 63, 64);
    const int nvalid = min(64, cnt - base);
    for (int s = 0; s < st.n;) {
      // two streams of <= 32 values share the wave (lanes 0-31 / 32-63): at the reference's 21-31 bands a single stream would leave
      // half the lanes idle, and this loop is latency-bound -- the number of row-load rounds is what it costs.  (Round 4 tried rows as
      // float4 pieces, 64 / ceil(K / 4) rows per load instruction -- 8 instead of 64 load instructions per chunk at 31 bands, partial
      // sums joined by xor-shuffles: 25.6 vs 20.5 us at C2, 189 vs 159 us with 128-band streams.  4-byte-aligned dwordx4 rows and the
      // 12 extra shuffles cost more than the load rounds they save.  Reverted.)
      const bool pair = s + 1 < st.n && st.k[s] <= 32 && st.k[s + 1] <= 32;
      const int half = pair ? (lane >> 5) : 0;
      const int K = half ? st.k[s + 1] : st.k[s];
      const float* __restrict__ v = (half ? st.v[s + 1] : st.v[s]) + (start + base) * (int64_t)K;
      float* __restrict__ outp = half ? st.out[s + 1] : st.out[s];
      const int kspan = pair ? 32 : 64, klane = pair ? (lane & 31) : lane;
      const int kmax = pair ? 32 : st.k[s];
      for (int kc = 0; kc < kmax; kc += kspan) {
        const int k = kc + klane;
        const bool kv = k < K;
        // the per-ray sum runs in sample order: 64 dependent-free row loads, 16 of them in flight per lane
        float p0 = 0.0f, p1 = 0.0f;
        const float* __restrict__ vk = v + (kv ? k : 0);
        int j = 0;
        for (; j + 15 < nvalid; j += 16) {
          float x[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) x[u] = vk[(int64_t)(j + u) * K];
#pragma unroll
          for (int u = 0; u < 16; u += 2) p0 += __shfl(w, j + u, 64) * x[u], p1 += __shfl(w, j + u + 1, 64) * x[u + 1];
        }
        for (; j + 7 < nvalid; j += 8) {  // (same association of the partial sums as ever: blocks of 8 alternate p0 / p1, the tail is p0)
          float x[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) x[u] = vk[(int64_t)(j + u) * K];
#pragma unroll
          for (int u = 0; u < 8; u += 2) p0 += __shfl(w, j + u, 64) * x[u], p1 += __shfl(w, j + u + 1, 64) * x[u + 1];
        }
        for (; j < nvalid; ++j) p0 += __shfl(w, j, 64) * vk[(int64_t)j * K];
        if (!kv) p0 = p1 = 0.0f;
        if (kv) {
          float* o = outp + r * K + k;
          *o = (base == 0) ? (p0 + p1) : (*o + (p0 + p1));
        }
      }
      s += pair ? 2 : 1;
    }
    if (cnt == 0) break;
  }
  acc = wave_reduce_sum(acc);
  dnum = wave_reduce_sum(dnum);
  if (lane == 0) {
    if (acc_out) acc_out[r] = acc;
    if (depth_out) depth_out[r] = dnum / (acc + 1e-10f);
  }
}

extern "C" int umhs_composite_fwd(const float* sigma, const float* t_starts, const float* t_ends,
                                  const int64_t* packed_info, int64_t n_rays, int64_t n,
                                  const umhs_value_streams* streams, float* weights, float* accumulation,
                                  float* depth, umhs_stream_t stream) {
  if (n_rays < 0 || n < 0 || !packed_info || !weights) return UMHS_ERR_ARG;
  if (n > 0 && (!sigma || !t_starts || !t_ends)) return UMHS_ERR_ARG;
  CompStreams st;
  st.n = streams ? streams->n_streams : 0;
  if (st.n < 0 || st.n > UMHS_MAX_STREAMS) return UMHS_ERR_ARG;
  for (int s = 0; s < UMHS_MAX_STREAMS; ++s) {
    st.k[s] = 0, st.v[s] = nullptr, st.out[s] = nullptr;
    if (s < st.n) {
      st.k[s] = streams->k[s], st.v[s] = streams->values[s], st.out[s] = streams->out[s];
      if (st.k[s] < 1 || !st.out[s] || (n > 0 && !st.v[s])) return UMHS_ERR_ARG;
    }
  }
  if (n_rays == 0) return UMHS_OK;
  hipLaunchKernelGGL(composite_fwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, umhs_s(stream), sigma,
                     t_starts, t_ends, packed_info, n_rays, st, weights, accumulation, depth);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

struct CompGrads {
  int n;
  int k[UMHS_MAX_STREAMS];
  const float* v[UMHS_MAX_STREAMS];
  const float* dout[UMHS_MAX_STREAMS];
  float* dv[UMHS_MAX_STREAMS];
};

// w_n = alpha_n T_n,  alpha = 1-exp(-x_n),  T_n = exp(-X_n),  X_n = sum_{m<n} x_m,  x = sigma*delta
//   dL/dx_n = dw_n * T_n * exp(-x_n)  -  sum_{m>n} dw_m w_m
// pass 1 walks the ray forward and parks exp(-(X_n + x_n)) in d_sigma[n]; pass 2 walks it backward with a
// suffix scan of dw*w.  The lane<->sample mapping is identical in both passes (same-thread RAW only).
__global__ __launch_bounds__(256) void composite_bwd_kernel(const float* __restrict__ sigma,
                                                            const float* __restrict__ t0,
                                                            const float* __restrict__ t1,
                                                            const int64_t* __restrict__ pinfo, int64_t n_rays,
                                                            const float* __restrict__ weights, CompGrads gr,
                                                            const float* __restrict__ d_acc, int grad_scaling,
                                                            float* __restrict__ d_sigma, const float* __restrict__ dots) {
  const int lane = threadIdx.x & 63;
  __shared__ float lds_tile[4][64 * 33 + 64 + 32];  // per wave: [64][33] value tile, 64 weights, 32 upstream gradients
  float* const tile = lds_tile[threadIdx.x >> 6];
  float* const wsl = tile + 64 * 33;
  float* const dl = wsl + 64;
  const int64_t r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (r >= n_rays) return;
  const int64_t start = pinfo[2 * r];
  const int cnt = (int)pinfo[2 * r + 1];
  if (cnt == 0) return;
  const int nchunks = (cnt + 63) >> 6;
  float carry = 0.0f;
  for (int c = 0; c < nchunks; ++c) {
    const int i = c * 64 + lane;
    const bool valid = i < cnt;
    const int64_t nidx = start + i;
    float x = valid ? sigma[nidx] * (t1[nidx] - t0[nidx]) : 0.0f;
    float incl = wave_inclusive_scan(x, lane);
    if (valid) d_sigma[nidx] = expf(-(carry + incl));
    carry += __shfl(incl, 63, 64);
  }
  const float dacc = d_acc ? d_acc[r] : 0.0f;
  float carry_after = 0.0f;
  for (int c = nchunks - 1; c >= 0; --c) {
    const int i = c * 64 + lane;
    const bool valid = i < cnt;
    const int64_t nidx = start + i;
    float dw = 0.0f, w = 0.0f, delta = 0.0f, scale = 1.0f, tnext = 0.0f;
    if (valid) {
      float a = t0[nidx], b = t1[nidx];
      delta = b - a;
      if (grad_scaling) {
        float m = (a + b) / 2.0f;
        scale = fminf(fmaxf(m * m, 0.0f), 1.0f);
      }
      w = weights[nidx];
      tnext = d_sigma[nidx];
      dw = dacc;
      if (dots) dw += dots[nidx];  // sum_k d_out[r][k] v[n][k], formed by the caller (umhs_composite_bwd_dots)
    }
    const int nvalid = min(64, cnt - c * 64);
    // The chunk's [nvalid x K] rows are one contiguous block.  K <= 32: read it with full 256-byte wave loads into an LDS tile
    // (row stride K|1: odd, so the per-lane row walk below is bank-conflict free) instead of 64 rows x K strided dwords.  Wider
    // streams (128 / 141 bands) walk 32-band slices of the block the same way, two 128-byte row segments per wave load (the
    // row-per-lane loop they used to take ran at a third of the narrow streams' rate: 289 us at C3, 463 us at C5).
    for (int s = 0; s < gr.n; ++s) {
      const int K = gr.k[s];
      const int KS = K <= 32 ? (K | 1) : 33;
      const float* __restrict__ vb = gr.v[s] + (start + c * 64) * (int64_t)K;
      const float* __restrict__ drow = gr.dout[s] + r * (int64_t)K;
      for (int k0 = 0; k0 < K; k0 += 32) {
        const int kw = min(32, K - k0);
        if (K <= 32) {
          const int tot = nvalid * K;
          for (int e = lane; e < tot; e += 64) {
            const int jj = e / K;
            tile[jj * KS + (e - jj * K)] = vb[e];
          }
        } else {
          const int col = lane & 31;
          for (int jj = lane >> 5; jj < nvalid; jj += 2)
            if (col < kw) tile[jj * 33 + col] = vb[(int64_t)jj * K + k0 + col];
        }
        if (lane < kw) dl[lane] = drow[k0 + lane];
        if (valid) {
          float d0 = 0.0f, d1 = 0.0f;
          int k = 0;
          for (; k + 1 < kw; k += 2) {
            d0 += dl[k] * tile[lane * KS + k];
            d1 += dl[k + 1] * tile[lane * KS + k + 1];
          }
          if (k < kw) d0 += dl[k] * tile[lane * KS + k];
          dw += d0 + d1;
        }
      }
    }
    float p = dw * w;
    float suf = wave_inclusive_scan_rev(p, lane);
    float S = carry_after + (suf - p);
    if (valid) d_sigma[nidx] = (dw * tnext - S) * delta * scale;
    carry_after += __shfl(suf, 0, 64);
    // d_values[n][k] = scale_n * w_n * d_out[r][k]   (lane = band: coalesced row stores)
    const float ws = w * scale;
    wsl[lane] = ws;
    for (int s = 0; s < gr.n; ++s) {
      if (!gr.dv[s]) continue;
      const int K = gr.k[s];
      float* __restrict__ dv = gr.dv[s] + (start + c * 64) * (int64_t)K;
      const float* __restrict__ drow = gr.dout[s] + r * (int64_t)K;
      if (K <= 32) {  // the [nvalid x K] block of d_values is contiguous too: full-wave stores
        if (lane < K) dl[lane] = drow[lane];
        const int tot = nvalid * K;
        for (int e = lane; e < tot; e += 64) {
          const int jj = e / K;
          dv[e] = wsl[jj] * dl[e - jj * K];
        }
        continue;
      }
      for (int kc = 0; kc < K; kc += 64) {
        const int k = kc + lane;
        const bool kv = k < K;
        const float d = kv ? drow[k] : 0.0f;
        for (int j = 0; j < nvalid; ++j)
          if (kv) dv[(int64_t)j * K + k] = wsl[j] * d;  // 256-byte row segments; the row's weight comes from LDS
      }
    }
  }
}

extern "C" int umhs_composite_bwd(const float* sigma, const float* t_starts, const float* t_ends,
                                  const int64_t* packed_info, int64_t n_rays, int64_t n, const float* weights,
                                  const umhs_value_grads* grads, const float* d_accumulation, int grad_scaling,
                                  float* d_sigma, umhs_stream_t stream) {
  if (n_rays < 0 || n < 0 || !packed_info || !d_sigma) return UMHS_ERR_ARG;
  if (n > 0 && (!sigma || !t_starts || !t_ends || !weights)) return UMHS_ERR_ARG;
  CompGrads gr;
  gr.n = grads ? grads->n_streams : 0;
  if (gr.n < 0 || gr.n > UMHS_MAX_STREAMS) return UMHS_ERR_ARG;
  for (int s = 0; s < UMHS_MAX_STREAMS; ++s) {
    gr.k[s] = 0, gr.v[s] = nullptr, gr.dout[s] = nullptr, gr.dv[s] = nullptr;
    if (s < gr.n) {
      gr.k[s] = grads->k[s], gr.v[s] = grads->values[s], gr.dout[s] = grads->d_out[s], gr.dv[s] = grads->d_values[s];
      if (gr.k[s] < 1 || !gr.dout[s] || (n > 0 && !gr.v[s])) return UMHS_ERR_ARG;
    }
  }
  if (n_rays == 0 || n == 0) return UMHS_OK;
  hipLaunchKernelGGL(composite_bwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, umhs_s(stream), sigma,
                     t_starts, t_ends, packed_info, n_rays, weights, gr, d_accumulation, grad_scaling, d_sigma, (const float*)nullptr);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// The density half of umhs_composite_bwd when the caller has already formed dots[n] = sum over streams and bands of
// d_out[ray(n)][k] * value[n][k] (the field backward does, from values it recomputes): d_sigma only, no [N,k] array read or written.
extern "C" int umhs_composite_bwd_dots(const float* sigma, const float* t_starts, const float* t_ends, const int64_t* packed_info,
                                       int64_t n_rays, int64_t n, const float* weights, const float* dots,
                                       const float* d_accumulation, int grad_scaling, float* d_sigma, umhs_stream_t stream) {
  if (n_rays < 0 || n < 0 || !packed_info || !d_sigma) return UMHS_ERR_ARG;
  if (n > 0 && (!sigma || !t_starts || !t_ends || !weights || !dots)) return UMHS_ERR_ARG;
  if (n_rays == 0 || n == 0) return UMHS_OK;
  CompGrads gr = {};
  hipLaunchKernelGGL(composite_bwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, umhs_s(stream), sigma, t_starts, t_ends,
                     packed_info, n_rays, weights, gr, d_accumulation, grad_scaling, d_sigma, dots);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// ---- accumulate with caller-provided weights (SpectralRenderer.forward called stand-alone) -----------------
__global__ __launch_bounds__(256) void accumulate_fwd_kernel(const float* __restrict__ weights,
                                                             const int64_t* __restrict__ pinfo, int64_t n_rays,
                                                             CompStreams st) {
  const int lane = threadIdx.x & 63;
  const int64_t r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (r >= n_rays) return;
  const int64_t start = pinfo[2 * r];
  const int cnt = (int)pinfo[2 * r + 1];
  for (int s = 0; s < st.n; ++s) {
    const int K = st.k[s];
    for (int kc = 0; kc < K; kc += 64) {
      const int k = kc + lane;
      if (k >= K) continue;
      const float* __restrict__ v = st.v[s] + start * (int64_t)K + k;
      float p0 = 0.0f, p1 = 0.0f;
      int j = 0;
      for (; j + 1 < cnt; j += 2) {
        p0 += weights[start + j] * v[(int64_t)j * K];
        p1 += weights[start + j + 1] * v[(int64_t)(j + 1) * K];
      }
      if (j < cnt) p0 += weights[start + j] * v[(int64_t)j * K];
      st.out[s][r * K + k] = p0 + p1;
    }
  }
}

__global__ __launch_bounds__(256) void accumulate_bwd_kernel(const float* __restrict__ weights,
                                                             const int64_t* __restrict__ pinfo, int64_t n_rays,
                                                             CompGrads gr, float* __restrict__ d_weights) {
  const int lane = threadIdx.x & 63;
  const int64_t r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (r >= n_rays) return;
  const int64_t start = pinfo[2 * r];
  const int cnt = (int)pinfo[2 * r + 1];
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    const bool valid = i < cnt;
    const int64_t nidx = start + i;
    float w = valid ? weights[nidx] : 0.0f, dw = 0.0f;
    if (valid) {
      for (int s = 0; s < gr.n; ++s) {
        const int K = gr.k[s];
        const float* __restrict__ vrow = gr.v[s] + nidx * (int64_t)K;
        const float* __restrict__ drow = gr.dout[s] + r * (int64_t)K;
        for (int k = 0; k < K; ++k) dw += drow[k] * vrow[k];
      }
      if (d_weights) d_weights[nidx] = dw;
    }
    const int nvalid = min(64, cnt - base);
    for (int s = 0; s < gr.n; ++s) {
      if (!gr.dv[s]) continue;
      const int K = gr.k[s];
      float* __restrict__ dv = gr.dv[s] + (start + base) * (int64_t)K;
      const float* __restrict__ drow = gr.dout[s] + r * (int64_t)K;
      for (int kc = 0; kc < K; kc += 64) {
        const int k = kc + lane;
        const bool kv = k < K;
        const float d = kv ? drow[k] : 0.0f;
        for (int j = 0; j < nvalid; ++j) {
          const float wj = __shfl(w, j, 64);
          if (kv) dv[(int64_t)j * K + k] = wj * d;
        }
      }
    }
  }
}

static int fill_streams(const umhs_value_streams* streams, int64_t n, CompStreams* st) {
  st->n = streams ? streams->n_streams : 0;
  if (st->n < 0 || st->n > UMHS_MAX_STREAMS) return UMHS_ERR_ARG;
  for (int s = 0; s < UMHS_MAX_STREAMS; ++s) {
    st->k[s] = 0, st->v[s] = nullptr, st->out[s] = nullptr;
    if (s < st->n) {
      st->k[s] = streams->k[s], st->v[s] = streams->values[s], st->out[s] = streams->out[s];
      if (st->k[s] < 1 || !st->out[s] || (n > 0 && !st->v[s])) return UMHS_ERR_ARG;
    }
  }
  return UMHS_OK;
}

static int fill_grads(const umhs_value_grads* grads, int64_t n, CompGrads* gr) {
  gr->n = grads ? grads->n_streams : 0;
  if (gr->n < 0 || gr->n > UMHS_MAX_STREAMS) return UMHS_ERR_ARG;
  for (int s = 0; s < UMHS_MAX_STREAMS; ++s) {
    gr->k[s] = 0, gr->v[s] = nullptr, gr->dout[s] = nullptr, gr->dv[s] = nullptr;
    if (s < gr->n) {
      gr->k[s] = grads->k[s], gr->v[s] = grads->values[s], gr->dout[s] = grads->d_out[s], gr->dv[s] = grads->d_values[s];
      if (gr->k[s] < 1 || !gr->dout[s] || (n > 0 && !gr->v[s])) return UMHS_ERR_ARG;
    }
  }
  return UMHS_OK;
}

extern "C" int umhs_accumulate_fwd(const float* weights, const int64_t* packed_info, int64_t n_rays, int64_t n,
                                   const umhs_value_streams* streams, umhs_stream_t stream) {
  if (n_rays < 0 || n < 0 || !packed_info || (n > 0 && !weights)) return UMHS_ERR_ARG;
  CompStreams st;
  int rc = fill_streams(streams, n, &st);
  if (rc) return rc;
  if (n_rays == 0 || st.n == 0) return UMHS_OK;
  hipLaunchKernelGGL(accumulate_fwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, umhs_s(stream), weights,
                     packed_info, n_rays, st);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_accumulate_bwd(const float* weights, const int64_t* packed_info, int64_t n_rays, int64_t n,
                                   const umhs_value_grads* grads, float* d_weights, umhs_stream_t stream) {
  if (n_rays < 0 || n < 0 || !packed_info || (n > 0 && !weights)) return UMHS_ERR_ARG;
  CompGrads gr;
  int rc = fill_grads(grads, n, &gr);
  if (rc) return rc;
  if (n_rays == 0 || n == 0) return UMHS_OK;
  hipLaunchKernelGGL(accumulate_bwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, umhs_s(stream), weights,
                     packed_info, n_rays, gr, d_weights);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
