// Vertex Component Analysis (Nascimento & Dias) on the resident hyperspectral stack: the three passes of the reference's
// data/utils/vca.py that touch every pixel.  rows [N,B] fp32 = the pixels of the [n,H,W,B] hs_image stack as it lies in HBM.
//   umhs_vca_moments  sum[b] = sum_n y_nb and S[i][j] = sum_n y_ni y_nj (vca.py:77-79,122: mean, Y_o Y_o^T, Y Y^T all follow from them)
//   umhs_vca_project  y [N,16] = the projected pixels the recursion looks at (vca.py:112-116 / :124-129)
//   umhs_vca_argmax   argmax_n |f^T y_n|, lowest index on a tie (vca.py:151-153)
// The B x B eigen-problem and the R x R pseudo-inverses between the passes are host work in float64 (umhsnerf/data/utils/vca.py).
// One-shot initialiser: nothing here runs in a training step.  No float atomics anywhere: every result is bitwise reproducible.
#include "umhs_common.h"

#define VCA_K 128       // rows per fp32 partial of the moments (a multiple of VCA_SUB); what umhs_vca_rows_per_partial() reports:
                        // 128 keeps the fp32 error of S, hence of the basis, below the reference's own fp32 distance from float64
#define VCA_NP 4        // 32x32 tile pairs (= independent MFMA accumulators) per wave
#define VCA_MAX_B 256
#define VCA_MAX_R 15
#define VCA_BLOCKS 512   // workgroups the moments aim at: two per CU (256 registers a wave, 36 KB of LDS a workgroup)

typedef float v16f __attribute__((ext_vector_type(16)));

// ---- moments ------------------------------------------------------------------------------------------------------------------
// S = Y^T Y is a tall-skinny SYRK: with v_mfma_f32_32x32x2_f32 the A operand of band tile t (lane l: y[row + (l >> 5)][32 t + (l & 31)])
// is also its B operand.  A workgroup streams its rows through LDS in sub-tiles of VCA_SUB rows: 256 threads copy the contiguous
// VCA_SUB * B floats once (coalesced; the next sub-tile waits in registers while this one is multiplied), and the four waves -- each
// owning VCA_NP of the upper triangle's 32x32 tile pairs -- read their operands from it (a wave-wide 4-byte global load per operand
// made the texture path, not the matrix pipe, the limit).  The LDS row pitch is 32 (mod 64) floats, so the two rows of a step fall
// into different bank halves, and the columns from B up to the pitch hold zeros, so no operand needs a mask.  A wave accumulates
// VCA_K rows in fp32 (exact products, one rounding per addition: an fmaf chain), adds that partial to float64 registers, and leaves
// one float64 partial per row group; vca_moments_finish_kernel adds the groups in ascending order.
#define VCA_SUB 16                                  // rows per LDS sub-tile (VCA_K is a multiple of it)
#define VCA_PITCH_MAX (VCA_MAX_B + 32)              // 8 band tiles + the odd-pitch pad
#define VCA_THREADS 256                             // four waves x VCA_NP pairs: the 16 pairs of a workgroup share one LDS tile
#define VCA_STAGE ((VCA_SUB * VCA_MAX_B + VCA_THREADS - 1) / VCA_THREADS)  // floats a thread carries from global memory to LDS per sub-tile, at most

struct VcaPlan {
  int T, P, groups_y, pitch;  // band tiles, tile pairs, workgroups along y (4 waves x VCA_NP pairs each), LDS row pitch in floats
  int64_t chunks, chunks_per_group, G;
};

static VcaPlan vca_plan(int64_t n, int B) {
  VcaPlan p;
  p.T = (B + 31) / 32;
  p.P = p.T * (p.T + 1) / 2;
  p.pitch = 32 * (p.T | 1);
  p.groups_y = (p.P + 4 * VCA_NP - 1) / (4 * VCA_NP);
  const int64_t target = VCA_BLOCKS / p.groups_y > 0 ? VCA_BLOCKS / p.groups_y : 1;
  p.chunks = (n + VCA_K - 1) / VCA_K;
  p.chunks_per_group = (p.chunks + target - 1) / target;
  if (p.chunks_per_group < 1) p.chunks_per_group = 1;
  p.G = (p.chunks + p.chunks_per_group - 1) / p.chunks_per_group;
  return p;
}

__device__ __forceinline__ void vca_pair(int p, int T, int& ti, int& tj) {  // p-th pair (ti <= tj) of the upper triangle, row-major
  ti = 0;
  while (p >= T - ti) p -= T - ti, ++ti;
  tj = ti + p;
}

__global__ __launch_bounds__(VCA_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void vca_moments_kernel(
    const float* __restrict__ rows, int64_t n, int B, int T, int P, int pitch, int64_t chunks, int64_t chunks_per_group,
    double* __restrict__ part, double* __restrict__ psum) {
  __shared__ float tile[2][VCA_SUB * VCA_PITCH_MAX];
  const int tid = threadIdx.x, lane = tid & 63;
  const int pg = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * 4 + (tid >> 6)));  // wave-uniform: MFMAs ignore EXEC
  const int64_t g = blockIdx.x;
  const int c = lane & 31, h = lane >> 5;
  bool on[VCA_NP];
  int oa[VCA_NP], ob[VCA_NP], ti[VCA_NP], tj[VCA_NP];
#pragma unroll
  for (int q = 0; q < VCA_NP; ++q) {
    const int p = pg * VCA_NP + q;
    on[q] = p < P;  // (a wave without pairs still carries its share of the rows to LDS)
    vca_pair(on[q] ? p : 0, T, ti[q], tj[q]);
    oa[q] = h * pitch + 32 * ti[q] + c, ob[q] = h * pitch + 32 * tj[q] + c;
  }
  double acc64[VCA_NP][16], sum64[VCA_NP];
#pragma unroll
  for (int q = 0; q < VCA_NP; ++q) {
    sum64[q] = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc64[q][e] = 0.0;
  }
  for (int k = tid; k < 2 * VCA_SUB * VCA_PITCH_MAX; k += VCA_THREADS) (&tile[0][0])[k] = 0.0f;  // the pad columns stay zero for good
  // element k of this thread in a sub-tile: float tid + VCA_THREADS k of its VCA_SUB * B contiguous floats
  const int per = (VCA_SUB * B + VCA_THREADS - 1) / VCA_THREADS, d_row = VCA_THREADS / B, d_col = VCA_THREADS % B;
  const int row0 = tid / B, col0 = tid % B;
  const int64_t total = n * B;
  float stg[VCA_STAGE];
  auto fetch = [&](int64_t st) {
    const int64_t base = st * VCA_SUB * B + tid;
#pragma unroll
    for (int k = 0; k < VCA_STAGE; ++k) {
      if (k < per) {  // (wave-uniform; the element test below is a select on the address and on the value, not a branch)
        const bool ok = tid + VCA_THREADS * k < VCA_SUB * B && base + VCA_THREADS * k < total;  // rows past the end enter as zeros
        const float v = rows[ok ? base + VCA_THREADS * k : 0];
        stg[k] = ok ? v : 0.0f;
      }
    }
  };
  auto stash = [&](float* dst) {
    int row = row0, col = col0;
#pragma unroll
    for (int k = 0; k < VCA_STAGE; ++k) {
      if (k < per) {
        if (row < VCA_SUB) dst[row * pitch + col] = stg[k];
        row += d_row, col += d_col;
        if (col >= B) col -= B, ++row;
      }
    }
  };
  const int64_t st0 = g * chunks_per_group * (VCA_K / VCA_SUB);
  const int64_t last_chunk = g * chunks_per_group + chunks_per_group < chunks ? g * chunks_per_group + chunks_per_group : chunks;
  const int64_t st1 = last_chunk * (VCA_K / VCA_SUB);
  __syncthreads();
  fetch(st0);
  stash(tile[0]);
  __syncthreads();
  v16f acc[VCA_NP];
  float s[VCA_NP];
  int cur = 0;
  for (int64_t st = st0; st < st1; ++st) {
    if (st + 1 < st1) fetch(st + 1);
    const int phase = (int)((st - st0) % (VCA_K / VCA_SUB));
    if (phase == 0) {
#pragma unroll
      for (int q = 0; q < VCA_NP; ++q) {
        s[q] = 0.0f;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.0f;
      }
    }
    const float* t = tile[cur];
#pragma unroll
    for (int step = 0; step < VCA_SUB / 2; ++step) {
#pragma unroll
      for (int q = 0; q < VCA_NP; ++q) {
        if (on[q]) {
          const float a = t[2 * step * pitch + oa[q]], b = t[2 * step * pitch + ob[q]];
          acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[q], 0, 0, 0);
          s[q] += a;
        }
      }
    }
    if (phase == VCA_K / VCA_SUB - 1) {
#pragma unroll
      for (int q = 0; q < VCA_NP; ++q) {
        sum64[q] += (double)s[q];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc64[q][e] += (double)acc[q][e];
      }
    }
    if (st + 1 < st1) stash(tile[cur ^ 1]);
    __syncthreads();
    cur ^= 1;
  }
#pragma unroll
  for (int q = 0; q < VCA_NP; ++q) {
    if (!on[q]) continue;
    double* dst = part + ((g * P + pg * VCA_NP + q) * 16) * 64 + lane;
#pragma unroll
    for (int e = 0; e < 16; ++e) dst[e * 64] = acc64[q][e];
    if (ti[q] == tj[q]) psum[(g * T + ti[q]) * 64 + lane] = sum64[q];  // the diagonal pair of a tile owns its band sums
  }
}

// sum_g src[g * stride] in one fixed order: eight interleaved running sums (eight loads in flight instead of one), then a fixed tree
__device__ __forceinline__ double vca_sum_groups(const double* __restrict__ src, int64_t stride, int64_t G) {
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int64_t g = 0;
  for (; g + 8 <= G; g += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += src[(g + k) * stride];
  }
  for (int k = 0; g < G; ++g, ++k) v[k] += src[g * stride];
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// element (reg e, lane l) of a 32x32 accumulator: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31
__global__ __launch_bounds__(256) void vca_moments_finish_kernel(const double* __restrict__ part, const double* __restrict__ psum,
                                                                 int B, int T, int P, int64_t G, int accumulate,
                                                                 double* __restrict__ sum, double* __restrict__ S) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_s = (int64_t)P * 1024;
  if (idx < n_s) {
    const int p = (int)(idx >> 10), e = (int)(idx >> 6) & 15, l = (int)idx & 63;
    int ti, tj;
    vca_pair(p, T, ti, tj);
    const int i = 32 * ti + (e & 3) + 8 * (e >> 2) + 4 * (l >> 5), j = 32 * tj + (l & 31);
    if (i >= B || j >= B || i > j) return;  // (diagonal tiles hold both halves: the upper one is kept and mirrored)
    const double v = vca_sum_groups(part + (int64_t)p * 1024 + (idx & 1023), (int64_t)P * 1024, G);
    const double r = accumulate ? S[(int64_t)i * B + j] + v : v;
    S[(int64_t)i * B + j] = r;
    S[(int64_t)j * B + i] = r;
  } else if (idx < n_s + 32 * T) {
    const int t = (int)(idx - n_s) >> 5, cc = (int)(idx - n_s) & 31;
    if (32 * t + cc >= B) return;
    const double v = vca_sum_groups(psum + t * 64 + cc, (int64_t)T * 64, G) + vca_sum_groups(psum + t * 64 + 32 + cc, (int64_t)T * 64, G);  // even + odd rows
    sum[32 * t + cc] = accumulate ? sum[32 * t + cc] + v : v;
  }
}

extern "C" int umhs_vca_rows_per_partial(void) { return VCA_K; }

extern "C" size_t umhs_vca_moments_workspace_bytes(int64_t n_rows, int n_bands) {
  if (n_rows < 1 || n_bands < 1 || n_bands > VCA_MAX_B) return 0;
  const VcaPlan p = vca_plan(n_rows, n_bands);
  return (size_t)p.G * ((size_t)p.P * 1024 + (size_t)p.T * 64) * sizeof(double);
}

extern "C" int umhs_vca_moments(const float* rows, int64_t n_rows, int n_bands, int accumulate, double* sum, double* S,
                                void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n_rows == 0) return UMHS_OK;  // nothing to add (the caller zeroes sum / S when it does not accumulate)
  if (n_rows < 0 || n_bands < 1 || !rows || !sum || !S) return UMHS_ERR_ARG;
  if (n_bands > VCA_MAX_B) return UMHS_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < umhs_vca_moments_workspace_bytes(n_rows, n_bands) || ((uintptr_t)workspace & 7)) return UMHS_ERR_WORKSPACE;
  const VcaPlan p = vca_plan(n_rows, n_bands);
  double* part = (double*)workspace;
  double* psum = part + (size_t)p.G * p.P * 1024;
  hipLaunchKernelGGL(vca_moments_kernel, dim3((unsigned)p.G, (unsigned)p.groups_y), dim3(VCA_THREADS), 0, umhs_s(stream), rows, n_rows, n_bands,
                     p.T, p.P, p.pitch, p.chunks, p.chunks_per_group, part, psum);
  UMHS_CHECK_LAUNCH();
  const int64_t threads = (int64_t)p.P * 1024 + 32 * p.T;
  hipLaunchKernelGGL(vca_moments_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, umhs_s(stream), part, psum,
                     n_bands, p.T, p.P, p.G, accumulate, sum, S);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------
// x^T [16 components x 16 pixels] = basis^T [16 x B] . rows^T [B x 16] on v_mfma_f32_16x16x4_f32, one wave per tile of 16 pixels.
// Lane l (j = l & 15, g = l >> 4) reads pixel j's bands 16 it + 4 g .. + 3 as ONE 16-byte load per iteration (a pixel row is read
// in 64-byte pieces by four lanes, every byte once) and feeds the four MFMAs of the iteration with its .x .y .z .w: MFMA s of
// iteration it contracts the bands {16 it + 4 g + s}, whose basis rows lie in LDS in exactly that order.  The accumulator leaves
// components 4 g .. 4 g + 3 of pixel j on lane l: one 16-byte store.  All loads of a tile are issued before its first MFMA.
// Projective form (vca.py:124-129): column 15 of the basis is Ud u, so the denominator u^T x arrives as the 16th component.
// Affine form (:112-116): the mean (LDS) is subtracted on load and max_n |x_n|^2 is kept per lane (a maximum is exact in any
// order).  HBM-bound: reads 4 N B bytes, writes 64 N.
#define VCA_PROJ_BLOCKS 1024
#define VCA_PROJ_ITERS (VCA_MAX_B / 16)

typedef float v4f __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) VcaRow4 {  // four consecutive bands of a pixel: 4-byte aligned only (B need not be a multiple of 4)
  float x, y, z, w;
};

__global__ __launch_bounds__(256) void vca_project_kernel(const float* __restrict__ rows, int64_t n, int B,
                                                          const float* __restrict__ basis, const float* __restrict__ mean,
                                                          int affine, float* __restrict__ y, float* __restrict__ pmax) {
#pragma clang fp contract(off)
  __shared__ float wl[VCA_PROJ_ITERS * 4 * 64];  // [it][s][g][i] = basis[16 it + 4 g + s][i]
  __shared__ __attribute__((aligned(16))) float ml[VCA_MAX_B];
  const int nit = (B + 15) / 16;  // (a kernel argument: wave-uniform, the MFMAs below sit under scalar branches)
  for (int k = threadIdx.x; k < nit * 256; k += 256) {
    const int it = k >> 8, s = (k >> 6) & 3, g = (k >> 4) & 3, i = k & 15, b = 16 * it + 4 * g + s;
    wl[k] = b < B ? basis[b * 16 + i] : 0.0f;
  }
  for (int k = threadIdx.x; k < VCA_MAX_B; k += 256) ml[k] = (mean && k < B) ? mean[k] : 0.0f;
  __syncthreads();
  const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
  const int64_t tiles = (n + 15) / 16;
  float best = 0.0f;
  for (int64_t tile = gw; tile < tiles; tile += nw) {
    const int64_t r = tile * 16 + j;
    const bool live = r < n;
    const float* row = rows + (live ? r : 0) * B;
    v4f in[VCA_PROJ_ITERS];
#pragma unroll
    for (int it = 0; it < VCA_PROJ_ITERS; ++it) {
      if (it < nit) {
        const int b0 = 16 * it + 4 * g;
        if (live && b0 + 3 < B) {
          const VcaRow4 t = *reinterpret_cast<const VcaRow4*>(row + b0);
          in[it] = v4f{t.x, t.y, t.z, t.w};
        } else {  // the end of a pixel row (never read past it: the next bytes are the next pixel, or nothing), or no pixel
          in[it] = v4f{live && b0 < B ? row[b0] : 0.0f, live && b0 + 1 < B ? row[b0 + 1] : 0.0f,
                       live && b0 + 2 < B ? row[b0 + 2] : 0.0f, 0.0f};
        }
      }
    }
    v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int it = 0; it < VCA_PROJ_ITERS; ++it) {
      if (it < nit) {
        const int b0 = 16 * it + 4 * g;
        const v4f m = *reinterpret_cast<const v4f*>(ml + b0);  // (zeros past B and in the projective form: x - 0 is exact)
        const v4f c = in[it] - m;
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[(it * 4 + s) * 64 + lane], c[s], acc, 0, 0, 0);
      }
    }
    if (affine) {
      float sq = ((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]) + acc[3] * acc[3];
      sq += __shfl_xor(sq, 16, 64);
      sq += __shfl_xor(sq, 32, 64);
      if (live) best = fmaxf(best, sq);
    } else {
      const float den = __shfl(acc[3], 48 + j, 64) + 1e-6f;
      acc = v4f{acc[0] / den, acc[1] / den, acc[2] / den, g == 3 ? 0.0f : acc[3] / den};
    }
    if (live) *reinterpret_cast<v4f*>(y + r * 16 + 4 * g) = acc;
  }
  if (affine) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = fmaxf(best, __shfl_xor(best, d, 64));
    if (lane == 0) pmax[gw] = best;
  }
}

__global__ __launch_bounds__(256) void vca_max_finish_kernel(const float* __restrict__ pmax, int n, float* __restrict__ out) {
  __shared__ float sh[4];
  float best = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) best = fmaxf(best, pmax[i]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = fmaxf(best, __shfl_xor(best, d, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

static int vca_project_blocks(int64_t n) {
  const int64_t want = (n + 63) / 64;  // a wave per tile of 16 pixels
  return (int)(want < VCA_PROJ_BLOCKS ? (want < 1 ? 1 : want) : VCA_PROJ_BLOCKS);
}

extern "C" size_t umhs_vca_project_workspace_bytes(int64_t n_rows) {
  return n_rows < 1 ? 0 : (size_t)vca_project_blocks(n_rows) * 4 * sizeof(float);
}

extern "C" int umhs_vca_project(const float* rows, int64_t n_rows, int n_bands, const float* basis16, const float* mean,
                                int n_classes, int affine, float* y, float* max_sq, void* workspace, size_t workspace_bytes,
                                umhs_stream_t stream) {
  if (n_rows == 0) return UMHS_OK;
  if (n_rows < 0 || n_bands < 1 || n_classes < 1 || !rows || !basis16 || !y || ((uintptr_t)y & 15) || (affine && (!mean || !max_sq)))
    return UMHS_ERR_ARG;
  if (n_bands > VCA_MAX_B || n_classes > VCA_MAX_R) return UMHS_ERR_UNSUPPORTED;
  if (affine && (!workspace || workspace_bytes < umhs_vca_project_workspace_bytes(n_rows) || ((uintptr_t)workspace & 3))) return UMHS_ERR_WORKSPACE;
  const int blocks = vca_project_blocks(n_rows);
  hipLaunchKernelGGL(vca_project_kernel, dim3((unsigned)blocks), dim3(256), 0, umhs_s(stream), rows, n_rows, n_bands, basis16,
                     affine ? mean : (const float*)nullptr, affine, y, (float*)workspace);
  UMHS_CHECK_LAUNCH();
  if (affine) {
    hipLaunchKernelGGL(vca_max_finish_kernel, dim3(1), dim3(256), 0, umhs_s(stream), (const float*)workspace, blocks * 4, max_sq);
    UMHS_CHECK_LAUNCH();
  }
  return UMHS_OK;
}

// ---- arg-max ------------------------------------------------------------------------------------------------------------------
// v_n = |bias + f^T y_n| as one fmaf chain per row (bias = f_d c of the affine form, whose constant component is not stored);
// the larger value wins, the LOWER index on equal values (numpy.argmax), in the thread, the wave, the block and the final block.
struct VcaF {
  float f[16];
};

__device__ __forceinline__ void vca_better(float& v, int64_t& i, float ov, int64_t oi) {
  if (ov > v || (ov == v && oi < i)) v = ov, i = oi;
}

__device__ __forceinline__ void vca_block_best(float& v, int64_t& i, float* sv, int64_t* si) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(v, d, 64);
    const int lo = __shfl_xor((int)(i & 0xffffffffLL), d, 64), hi = __shfl_xor((int)(i >> 32), d, 64);
    vca_better(v, i, ov, ((int64_t)hi << 32) | (uint32_t)lo);
  }
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v, si[threadIdx.x >> 6] = i;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) vca_better(v, i, sv[k], si[k]);
  }
}

__global__ __launch_bounds__(256) void vca_argmax_kernel(const float4* __restrict__ y, int64_t n, VcaF f, float bias,
                                                         float* __restrict__ pval, int64_t* __restrict__ pidx) {
  __shared__ float sv[4];
  __shared__ int64_t si[4];
  float best = -1.0f;
  int64_t bi = INT64_MAX;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    float v = bias;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 t = y[r * 4 + k];
      v = fmaf(f.f[4 * k], t.x, v), v = fmaf(f.f[4 * k + 1], t.y, v), v = fmaf(f.f[4 * k + 2], t.z, v), v = fmaf(f.f[4 * k + 3], t.w, v);
    }
    v = fabsf(v);
    if (v > best) best = v, bi = r;  // rows ascend within a thread: the first of equal values stays
  }
  vca_block_best(best, bi, sv, si);
  if (threadIdx.x == 0) pval[blockIdx.x] = best, pidx[blockIdx.x] = bi;
}

__global__ __launch_bounds__(256) void vca_argmax_finish_kernel(const float* __restrict__ pval, const int64_t* __restrict__ pidx,
                                                                int parts, const float* __restrict__ y, int64_t n,
                                                                int64_t* __restrict__ index, float* __restrict__ row,
                                                                float* __restrict__ value) {
  __shared__ float sv[4];
  __shared__ int64_t si[4];
  __shared__ int64_t winner;
  float best = -1.0f;
  int64_t bi = INT64_MAX;
  for (int k = threadIdx.x; k < parts; k += 256) vca_better(best, bi, pval[k], pidx[k]);
  vca_block_best(best, bi, sv, si);
  if (threadIdx.x == 0) {
    if (bi < 0 || bi >= n) bi = 0;  // (every |v| was NaN: no row won)
    winner = bi, index[0] = bi;
    if (value) value[0] = best;
  }
  __syncthreads();
  if (threadIdx.x < 16) row[threadIdx.x] = y[winner * 16 + threadIdx.x];
}

#define VCA_ARGMAX_BLOCKS 1024

static int vca_argmax_blocks(int64_t n) {
  const int64_t want = (n + 255) / 256;
  return (int)(want < VCA_ARGMAX_BLOCKS ? (want < 1 ? 1 : want) : VCA_ARGMAX_BLOCKS);
}

extern "C" size_t umhs_vca_argmax_workspace_bytes(int64_t n_rows) {
  return n_rows < 1 ? 0 : (size_t)vca_argmax_blocks(n_rows) * (sizeof(int64_t) + sizeof(float));
}

extern "C" int umhs_vca_argmax(const float* y, int64_t n_rows, const float* f_host16, float bias, int64_t* index, float* row,
                               float* value, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n_rows == 0) return UMHS_OK;
  if (n_rows < 0 || !y || !f_host16 || !index || !row || ((uintptr_t)y & 15)) return UMHS_ERR_ARG;
  if (!workspace || workspace_bytes < umhs_vca_argmax_workspace_bytes(n_rows) || ((uintptr_t)workspace & 7)) return UMHS_ERR_WORKSPACE;
  const int blocks = vca_argmax_blocks(n_rows);
  VcaF f;
  for (int k = 0; k < 16; ++k) f.f[k] = f_host16[k];
  int64_t* pidx = (int64_t*)workspace;
  float* pval = (float*)(pidx + blocks);
  hipLaunchKernelGGL(vca_argmax_kernel, dim3((unsigned)blocks), dim3(256), 0, umhs_s(stream), (const float4*)y, n_rows, f, bias, pval, pidx);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(vca_argmax_finish_kernel, dim3(1), dim3(256), 0, umhs_s(stream), (const float*)pval, (const int64_t*)pidx, blocks, y,
                     n_rows, index, row, value);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
