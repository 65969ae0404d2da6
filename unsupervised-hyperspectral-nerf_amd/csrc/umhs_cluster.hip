// Spectral clustering (include/umhs_hip.h, "Spectral clustering"): one Lloyd iteration's pass over the rows, fused -- every row is
// assigned to its nearest centre (spectral angle or Euclidean) and, in the same pass, the rows of each cluster are summed.  R B floats
// are read once; the [R,K] matrix of distances never exists.
//
//   cluster_chunk_kernel   one block (4 waves) per chunk of UMHS_CLUSTER_CHUNK rows.  The chunk goes through LDS in slabs of 32 rows
//                          (a wave loads whole rows, a coalesced run per row; the next slab's loads are in flight under the MFMAs).
//     assign               wave t < ceil(K / 32) takes entry tile t of the centres' operand image (umhs_library_tile.h's layout; copied
//                          to LDS once per chunk where it fits beside the slab, else read from cache): dot^T[entry][row] = image x rows^T on
//                          v_mfma_f32_32x32x2_f32, the slab read from LDS as the B operand (row on lane & 31, band 2 step + (lane >> 5)).
//                          The MFMA's k order is the band order and its accumulator starts at 0: dot is the fmaf chain of
//                          umhs_library_match.  A lane's 16 accumulator rows are 16 entries in ascending index, so it keeps its best
//                          with strict comparisons; the two lanes of a row, then the two tiles, merge by (value descending, index
//                          ascending).  For ANGLE the division is skipped, exactly, for an entry whose dot is not above the dot of
//                          the lane's best (a correctly rounded quotient by one positive divisor is monotone).
//     finalise             thread j < 32 decides row j: validity, label, score, objective term; label and score go to global.
//     members              the slab is rewritten in place as v: x / sqrtf(ss) for ANGLE, x for EUCLIDEAN, ZEROS for an invalid row
//                          (a NaN times the one-hot's 0 would poison the chain).
//     sums                 s = onehot^T v on the same MFMA with the ROW as the k dimension: the A operand is the one-hot of the slab's
//                          labels, built in registers (lane l holds label[2 s + (l >> 5)] == 32 t + (l & 31)), the B operand the
//                          slab's v.  A product by an exact 0 or 1 is exact, so the chain is the float32 sum of the members' v in row
//                          order.  One accumulator per (cluster tile, band tile) -- at most 2 x 8 -- lives in registers for the whole
//                          chunk; they are dealt round-robin to the four waves.  Counts and the objective are taken from the LDS
//                          labels / terms by single threads, in row order.
//                          The block writes the chunk's (valid, objective, n, s) as float32 to its own slot of the workspace.
//   cluster_reduce_kernel  one thread per element of acc: the slots of a pass added in float64, chunks ascending, onto acc.
// No atomics anywhere: the same bits on every run.  With acc == NULL the chunk kernel stops after finalise (one launch, no workspace).
#include "umhs_library_tile.h"

namespace {

constexpr int CL_THREADS = 256, CL_SLAB = 32, CL_ROWS_PER_WAVE = CL_SLAB / 4;
constexpr int CL_PASS = 512;  // chunks per pass: the workspace holds one slot per chunk of a pass
constexpr float CL_FLT_BIG = 3.402823466e38f;

__host__ __device__ inline int64_t cluster_slot_floats(int K, int B) { return 2 + (int64_t)K + (int64_t)K * B; }

template <int NT, int CT>  // band tiles of 32, cluster tiles of 32
__global__ __launch_bounds__(CL_THREADS) void cluster_chunk_kernel(const float* __restrict__ spectra, int64_t stride, int64_t R,
                                                                   const float* __restrict__ mask, const float* __restrict__ image,
                                                                   const float* __restrict__ half_norm, int K, int B, int metric,
                                                                   int64_t first_chunk, int32_t* __restrict__ label,
                                                                   float* __restrict__ score, float* __restrict__ partial) {
  constexpr int LD = NT * 32, LDP = LD + 2, NV = (NT + 1) / 2, NP = NT * CT, PPW = (NP + 3) / 4;
  // the centres' image stays in LDS for the whole chunk where it fits the 64 KB beside the slab (up to 64 x 160 or 32 x 224);
  // above that it is read from cache
  constexpr int IMAGE_FLOATS = CT * NT * 16 * 64;
  constexpr bool IMAGE_IN_LDS = (IMAGE_FLOATS + CL_SLAB * LDP) * 4 + 2048 <= 65536;
  __shared__ float sImage[IMAGE_IN_LDS ? IMAGE_FLOATS : 1];
  __shared__ float sX[CL_SLAB * LDP];  // the slab in flight: [row][band], zeros past B; rewritten as v before the sums
  __shared__ float sHn[64], sSS[CL_SLAB], sRs[CL_SLAB], sObj[CL_SLAB], sBestV[CT][CL_SLAB];
  __shared__ int sBestI[CT][CL_SLAB], sLabel[CL_SLAB], sMask[CL_SLAB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const bool angle = metric == UMHS_CLUSTER_ANGLE, sums = partial != nullptr;
  const int ks = lib_ksteps(B);
  const int64_t row0 = (first_chunk + blockIdx.x) * (int64_t)UMHS_CLUSTER_CHUNK;
  const int64_t row1 = row0 + UMHS_CLUSTER_CHUNK < R ? row0 + UMHS_CLUSTER_CHUNK : R;

  if (tid < 64) sHn[tid] = (!angle && tid < K) ? half_norm[tid] : 0.0f;
  if (IMAGE_IN_LDS) {
    for (int k = tid; k < CT * ks * 64; k += CL_THREADS) sImage[k] = image[k];  // (read after the first barrier)
  }

  // the wave's (cluster tile, band tile) pairs, dealt round-robin; a surplus slot repeats pair (0, 0) unwritten
  int pc[PPW], pb[PPW];
#pragma unroll
  for (int p = 0; p < PPW; ++p) {
    int q = wave + 4 * p;
    if (q >= NP) q = 0;
    pc[p] = q / NT, pb[p] = q % NT;
  }
  v16f acc[PPW];
#pragma unroll
  for (int p = 0; p < PPW; ++p)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[p][e] = 0.0f;
  float objective = 0.0f;         // (thread 128's)
  int count = 0, valid_rows = 0;  // (thread k < K: the cluster's rows; thread 192: the valid rows)

  float xr[CL_ROWS_PER_WAVE][NV], mv[CL_ROWS_PER_WAVE];
  auto load_slab = [&](int64_t base) {
#pragma unroll
    for (int i = 0; i < CL_ROWS_PER_WAVE; ++i) {
      const int64_t r = base + wave + 4 * i;
      const bool in = r < row1;
      const float* row = spectra + (in ? r : row0) * stride;
#pragma unroll
      for (int v = 0; v < NV; ++v) xr[i][v] = (in && lane + 64 * v < B) ? row[lane + 64 * v] : 0.0f;
      mv[i] = !in ? 0.0f : mask ? mask[r] : 1.0f;
    }
  };

  load_slab(row0);
  for (int64_t base = row0; base < row1; base += CL_SLAB) {
#pragma unroll
    for (int i = 0; i < CL_ROWS_PER_WAVE; ++i) {
      const int64_t r = base + wave + 4 * i;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int b = lane + 64 * v;
        if (b < LD) sX[(wave + 4 * i) * LDP + b] = xr[i][v];  // (zeros past B and past the chunk's last row)
      }
      if (lane == 0) sMask[wave + 4 * i] = (r < row1 && !(mv[i] <= 0.5f)) ? 1 : 0;
    }
    __syncthreads();
    if (base + CL_SLAB < row1) load_slab(base + CL_SLAB);  // in flight under the MFMAs

    // ---- assign: wave t takes entry tile t
    if (wave < CT) {
      const float* xt = sX + j * LDP + h;
      v16f dot;
#pragma unroll
      for (int e = 0; e < 16; ++e) dot[e] = 0.0f;
      float ss = 0.0f;  // the chain of x_b^2, b ascending: even bands sit on this lane or on its partner, odd ones on the other
      // four steps' operands are fetched before the first of their MFMAs; a step past the last adds an exact 0 x 0
      auto walk = [&](const float* at) {
        for (int s0 = 0; s0 < ks; s0 += 4) {
          float a[4], x[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool on = s0 + i < ks;
            a[i] = on ? at[(s0 + i) * 64] : 0.0f;
            x[i] = on ? xt[2 * (s0 + i)] : 0.0f;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            dot = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], x[i], dot, 0, 0, 0);
            const float other = __shfl_xor(x[i], 32, 64);
            const float even = h ? other : x[i], odd = h ? x[i] : other;
            ss = fmaf(even, even, ss);
            ss = fmaf(odd, odd, ss);
          }
        }
      };
      if (IMAGE_IN_LDS) walk(sImage + wave * ks * 64 + lane);
      else walk(image + (size_t)wave * ks * 64 + lane);
      const float rs = sqrtf(ss);
      float bv = -INFINITY, bd = -INFINITY;
      int bi = -1;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = 32 * wave + lib_acc_row(e, h);
        const float d = dot[e];
        if (k < K) {
          if (angle) {
            if (d > bd) {
              const float c = d / rs;
              if (c > bv) bv = c, bi = k, bd = d;
            }
          } else {
            const float g = d - sHn[k];
            if (g > bv) bv = g, bi = k;
          }
        }
      }
      const float ov = __shfl_xor(bv, 32, 64);
      const int oi = __shfl_xor(bi, 32, 64);
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
      if (h == 0) {
        sBestV[wave][j] = bv, sBestI[wave][j] = bi;
        if (wave == 0) sSS[j] = ss;
      }
    }
    __syncthreads();

    // ---- finalise: thread j decides row j
    if (tid < CL_SLAB) {
      float bv = sBestV[0][tid];
      int bi = sBestI[0][tid];
      if (CT > 1) {  // (tile 1's entries all have larger indices: it wins only when strictly larger)
        const float ov = sBestV[CT - 1][tid];
        const int oi = sBestI[CT - 1][tid];
        if (oi >= 0 && (bi < 0 || ov > bv)) bv = ov, bi = oi;
      }
      const float ss = sSS[tid];
      const bool valid = sMask[tid] != 0 && ss > 0.0f && ss <= CL_FLT_BIG && bi >= 0;  // not 0, not NaN, not Inf
      const float sc = angle ? bv : fmaxf(0.0f, fmaf(-2.0f, bv, ss));
      const int64_t r = base + tid;
      if (r < row1) {
        if (label) label[r] = valid ? bi : -1;
        if (score) score[r] = valid ? sc : 0.0f;
      }
      sLabel[tid] = valid ? bi : -1;
      sRs[tid] = sqrtf(ss);
      sObj[tid] = !valid ? 0.0f : angle ? 1.0f - sc : sc;
    }
    __syncthreads();
    if (!sums) continue;  // (the next slab's stores come after every read of this one)

    // ---- members: the slab becomes v, zeros in invalid rows
    for (int k = tid; k < CL_SLAB * LD; k += CL_THREADS) {
      const int r = k / LD, b = k - r * LD;
      const float x = sX[r * LDP + b];
      sX[r * LDP + b] = sLabel[r] < 0 ? 0.0f : angle ? x / sRs[r] : x;
    }
    __syncthreads();

    // ---- sums: onehot^T v, rows on the k dimension
#pragma unroll 4
    for (int s = 0; s < CL_SLAB / 2; ++s) {
      const int l = sLabel[2 * s + h];
      const float* bt = sX + (2 * s + h) * LDP + j;
#pragma unroll
      for (int p = 0; p < PPW; ++p)
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(l == 32 * pc[p] + j ? 1.0f : 0.0f, bt[32 * pb[p]], acc[p], 0, 0, 0);
    }
    if (tid < K) {
#pragma unroll 8
      for (int r = 0; r < CL_SLAB; ++r) count += sLabel[r] == tid ? 1 : 0;
    }
    if (tid == 128) {
#pragma unroll 8
      for (int r = 0; r < CL_SLAB; ++r) objective += sObj[r];  // (an invalid row's +0 changes no bit)
    }
    if (tid == 192) {
#pragma unroll 8
      for (int r = 0; r < CL_SLAB; ++r) valid_rows += sLabel[r] >= 0 ? 1 : 0;
    }
    __syncthreads();  // the slab is free again
  }

  if (!sums) return;
  float* slot = partial + (int64_t)blockIdx.x * cluster_slot_floats(K, B);
  if (tid == 192) slot[0] = (float)valid_rows;  // <= 1024: exact
  if (tid == 128) slot[1] = objective;
  if (tid < K) slot[2 + tid] = (float)count;  // <= 1024: exact
#pragma unroll
  for (int p = 0; p < PPW; ++p) {
    if (wave + 4 * p >= NP) continue;
    const int b = 32 * pb[p] + j;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k = 32 * pc[p] + lib_acc_row(e, h);
      if (k < K && b < B) slot[2 + K + (int64_t)k * B + b] = acc[p][e];
    }
  }
}

__global__ __launch_bounds__(256) void cluster_reduce_kernel(const float* __restrict__ partial, int chunks, int64_t n,
                                                             double* __restrict__ acc) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  double v = acc[idx];
  int c = 0;
  for (; c + 32 <= chunks; c += 32) {  // 32 loads in flight; the additions stay in chunk order
    float t[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) t[i] = partial[(c + i) * n + idx];
#pragma unroll
    for (int i = 0; i < 32; ++i) v += (double)t[i];
  }
  for (; c < chunks; ++c) v += (double)partial[c * n + idx];
  acc[idx] = v;
}

template <int NT, int CT>
void cluster_launch(const float* spectra, int64_t stride, int64_t R, const float* mask, const float* image, const float* half_norm, int K,
                    int B, int metric, int64_t first_chunk, int64_t chunks, int32_t* label, float* score, float* partial,
                    hipStream_t stream) {
  hipLaunchKernelGGL((cluster_chunk_kernel<NT, CT>), dim3((unsigned)chunks), dim3(CL_THREADS), 0, stream, spectra, stride, R, mask, image,
                     half_norm, K, B, metric, first_chunk, label, score, partial);
}

}  // namespace

extern "C" int umhs_cluster_chunk(void) { return UMHS_CLUSTER_CHUNK; }

extern "C" size_t umhs_cluster_workspace_bytes(int64_t n_rows, int n_clusters, int n_bands) {
  if (n_rows < 1 || n_bands < 1 || n_clusters < 1 || n_bands > LIB_MAX_BANDS || n_clusters > UMHS_CLUSTER_MAX) return 0;
  const int64_t chunks = (n_rows + UMHS_CLUSTER_CHUNK - 1) / UMHS_CLUSTER_CHUNK;
  return (size_t)(chunks < CL_PASS ? chunks : CL_PASS) * cluster_slot_floats(n_clusters, n_bands) * sizeof(float);
}

extern "C" int umhs_cluster_step(const float* spectra, int64_t stride, int64_t n_rows, const float* mask, const float* image,
                                 const float* half_norm, int n_clusters, int n_bands, int metric, int32_t* label, float* score,
                                 double* acc, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n_clusters < 1 || n_bands < 1 || n_rows < 0 || stride < n_bands) return UMHS_ERR_ARG;
  if (metric != UMHS_CLUSTER_ANGLE && metric != UMHS_CLUSTER_EUCLIDEAN) return UMHS_ERR_ARG;
  if (n_bands > LIB_MAX_BANDS || n_clusters > UMHS_CLUSTER_MAX) return UMHS_ERR_UNSUPPORTED;
  if (n_rows == 0) return UMHS_OK;
  if (!spectra || !image) return UMHS_ERR_ARG;
  if (metric == UMHS_CLUSTER_EUCLIDEAN && !half_norm) return UMHS_ERR_ARG;
  if (acc && (!workspace || workspace_bytes < umhs_cluster_workspace_bytes(n_rows, n_clusters, n_bands) || ((uintptr_t)workspace & 3)))
    return UMHS_ERR_ARG;
  const int64_t chunks = (n_rows + UMHS_CLUSTER_CHUNK - 1) / UMHS_CLUSTER_CHUNK;
  if (chunks > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  const int K = n_clusters, B = n_bands, nt = (B + 31) >> 5, ct = (K + 31) >> 5;
  const int64_t n = cluster_slot_floats(K, B);
  float* partial = acc ? (float*)workspace : nullptr;
  hipStream_t s = umhs_s(stream);
  const int64_t pass = acc ? CL_PASS : chunks;  // assigning alone is one launch
  for (int64_t first = 0; first < chunks; first += pass) {
    const int64_t m = chunks - first < pass ? chunks - first : pass;
    switch (2 * nt + ct - 3) {  // (nt 1..8, ct 1..2) -> 0..15
#define CLUSTER_CASE(NT)                                                                                                              \
  case 2 * NT - 2: cluster_launch<NT, 1>(spectra, stride, n_rows, mask, image, half_norm, K, B, metric, first, m, label, score, partial, s); break; \
  case 2 * NT - 1: cluster_launch<NT, 2>(spectra, stride, n_rows, mask, image, half_norm, K, B, metric, first, m, label, score, partial, s); break;
      CLUSTER_CASE(1) CLUSTER_CASE(2) CLUSTER_CASE(3) CLUSTER_CASE(4) CLUSTER_CASE(5) CLUSTER_CASE(6) CLUSTER_CASE(7) CLUSTER_CASE(8)
#undef CLUSTER_CASE
      default: return UMHS_ERR_UNSUPPORTED;
    }
    UMHS_CHECK_LAUNCH();
    if (acc) {
      hipLaunchKernelGGL(cluster_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, partial, (int)m, n, acc);
      UMHS_CHECK_LAUNCH();
    }
  }
  return UMHS_OK;
}
