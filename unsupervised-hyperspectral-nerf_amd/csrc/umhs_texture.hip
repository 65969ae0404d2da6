// Textured mesh export (what ``ns-export tsdf --texture-method nerf`` does for a trained model): a per-face texture atlas
// (umhs_texture_atlas / umhs_texture_uv) and, for every texel of it, the short ray through the surface that the model renders into
// that texel (umhs_texture_rays).  include/umhs_hip.h states the layout and the arithmetic as THE definition; tests/texture_ref.py
// restates both in numpy.
//
// Rays.  One thread owns one texel; x runs along the lanes, so the 64 texels of a wave are (pieces of) one atlas row and belong to
// at most 2 * ceil(64 / p) + 2 faces.  Every lane reads its face's three indices and nine coordinates itself: the p * p / 2 texels of
// a face sit in p consecutive rows of one square, their reads hit the same few cache lines, and what reaches HBM is at most 12 + 36 =
// 48 bytes per face against 36 (48 with the barycentric weights) bytes WRITTEN per texel, i.e. against >= 8 texels per face the
// kernel is bound by its stores.  A per-face pre-pass would only move those 48 bytes once more.  The [n, 3] outputs go through LDS:
// a workgroup's 256 rows of 12 bytes are one contiguous run of 768 dwords, stored as consecutive dwords by consecutive lanes instead
// of as three stores of stride 12 per lane.  No atomics, no workspace, no texel written by two threads: a range split anywhere gives
// the same bits.
//
// A vertex index is compared as an unsigned number against V BEFORE the position it names is loaded; a face that fails is written
// as a miss and nothing of it is dereferenced.
//
// The unit is compiled with contraction off: every weight, point, normal and origin is one rounded float32 operation per step, the
// xf_* operations of umhs_exact.h.
#pragma clang fp contract(off)
#include "umhs_common.h"
#include "umhs_exact.h"

#define TEX_THREADS 256
#define TEX_MAX_SIDE 16384  // 2 T < 2^24: the vt numerators are exact in float32; T^2 <= 2^28

// Q = the least integer with Q^2 >= S, T = Q p, in integers.  UMHS_OK, or the code the entries return.
static int tex_atlas(int64_t n_faces, int px, int64_t& Q, int64_t& T) {
  if (px < 4 || n_faces < 1) return UMHS_ERR_ARG;
  const int64_t S = n_faces / 2 + (n_faces & 1);
  if (S > (int64_t)TEX_MAX_SIDE * TEX_MAX_SIDE) return UMHS_ERR_UNSUPPORTED;  // (Q > 16384 already with p = 1)
  int64_t q = 1;
  while (q * q < S) q <<= 1;  // S <= 2^28: at most 14 doublings, then a bisection of [q / 2, q]
  int64_t lo = q >> 1, hi = q;  // lo^2 < S <= hi^2 (or S = 1 = hi)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (mid * mid >= S) hi = mid; else lo = mid;
  }
  Q = hi;
  T = Q * (int64_t)px;
  return T > TEX_MAX_SIDE ? UMHS_ERR_UNSUPPORTED : UMHS_OK;
}

extern "C" int umhs_texture_atlas(int64_t n_faces, int px, int32_t* squares_per_side, int32_t* side) {
  if (!squares_per_side || !side) return UMHS_ERR_ARG;
  int64_t Q, T;
  const int rc = tex_atlas(n_faces, px, Q, T);
  if (rc != UMHS_OK) return rc;
  *squares_per_side = (int32_t)Q;
  *side = (int32_t)T;
  return UMHS_OK;
}

// ---- vt ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TEX_THREADS) void texture_uv_kernel(int n_faces, int p, int Q, int T, float* __restrict__ uv) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * TEX_THREADS + threadIdx.x;
  if (f >= n_faces) return;
  const int s = f >> 1, odd = f & 1;
  const int sy = s / Q, sx = s - sy * Q;
  const int e = p - 3;
  // corner c of the even face (0,0) (e,0) (0,e); of the odd face (p-1,p-1) (2,p-1) (p-1,2)
  const int ci[3] = {odd ? p - 1 : 0, odd ? 2 : e, odd ? p - 1 : 0};
  const int cj[3] = {odd ? p - 1 : 0, odd ? p - 1 : 0, odd ? 2 : e};
  const float den = (float)(2 * T);
  float* o = uv + (size_t)f * 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[2 * c + 0] = xf_div((float)(2 * (sx * p + ci[c]) + 1), den);
    o[2 * c + 1] = xf_div((float)(2 * (T - (sy * p + cj[c])) - 1), den);
  }
}

extern "C" int umhs_texture_uv(int64_t n_faces, int px, float* uv, umhs_stream_t stream) {
  int64_t Q, T;
  const int rc = tex_atlas(n_faces, px, Q, T);
  if (rc != UMHS_OK) return rc;
  if (!uv) return UMHS_ERR_ARG;
  const unsigned blocks = (unsigned)((n_faces + TEX_THREADS - 1) / TEX_THREADS);  // n_faces <= 2 Q^2 <= 2^25
  hipLaunchKernelGGL(texture_uv_kernel, dim3(blocks), dim3(TEX_THREADS), 0, umhs_s(stream), (int)n_faces, px, (int)Q, (int)T, uv);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// ---- texel rays --------------------------------------------------------------------------------------------------------------------
// the workgroup's `count` rows of 3 floats, staged in `stage`, to out[3 * base ..): consecutive dwords by consecutive lanes
__device__ __forceinline__ void tex_store_rows(const float* stage, float* __restrict__ out, int64_t base, int count) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int idx = k * TEX_THREADS + (int)threadIdx.x;
    if (idx < 3 * count) out[3 * base + idx] = stage[idx];
  }
}

__global__ __launch_bounds__(TEX_THREADS) void texture_rays_kernel(const float* __restrict__ positions, uint32_t n_vertices,
                                                                    const int32_t* __restrict__ faces, int n_faces, int p, int Q, int T,
                                                                    float ray_length, int texel_begin, int n_texels,
                                                                    float* __restrict__ origins, float* __restrict__ directions,
                                                                    float* __restrict__ nears, float* __restrict__ fars,
                                                                    int32_t* __restrict__ texel_face, float* __restrict__ bary) {
#pragma clang fp contract(off)
  __shared__ float stage_o[3 * TEX_THREADS], stage_d[3 * TEX_THREADS], stage_w[3 * TEX_THREADS];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * TEX_THREADS;  // the workgroup's first output row
  const int count = (int)(n_texels - base < TEX_THREADS ? n_texels - base : TEX_THREADS);
  const bool mine = tid < count;

  // a miss, as the crop path writes one
  float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 1.0f}, w[3] = {0.0f, 0.0f, 0.0f};
  float near = 1e10f, far = 1e10f;
  int face = -1;
  if (mine) {
    const int t = texel_begin + (int)base + tid;  // < T^2 <= 2^28
    const int row = t / T, col = t - row * T;
    const int sx = col / p, i = col - sx * p;
    const int sy = row / p, j = row - sy * p;
    const int odd = i + j >= p ? 1 : 0;
    const int f = 2 * (sy * Q + sx) + odd;
    if (f < n_faces) {
      const uint32_t i0 = (uint32_t)faces[3 * (int64_t)f + 0], i1 = (uint32_t)faces[3 * (int64_t)f + 1],
                     i2 = (uint32_t)faces[3 * (int64_t)f + 2];
      if (i0 < n_vertices && i1 < n_vertices && i2 < n_vertices) {  // (unsigned: a negative index fails too) -- before any load
        float v0[3], v1[3], v2[3], a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v0[c] = positions[3 * (size_t)i0 + c];
          v1[c] = positions[3 * (size_t)i1 + c];
          v2[c] = positions[3 * (size_t)i2 + c];
          a[c] = xf_sub(v1[c], v0[c]);
          b[c] = xf_sub(v2[c], v0[c]);
        }
        float n[3];
        n[0] = xf_sub(xf_mul(a[1], b[2]), xf_mul(a[2], b[1]));
        n[1] = xf_sub(xf_mul(a[2], b[0]), xf_mul(a[0], b[2]));
        n[2] = xf_sub(xf_mul(a[0], b[1]), xf_mul(a[1], b[0]));
        const float q = xf_add(xf_add(xf_mul(n[0], n[0]), xf_mul(n[1], n[1])), xf_mul(n[2], n[2]));
        if (q > 0.0f && xf_finite(q)) {  // (a NaN fails the first test)
          const int e = p - 3;
          const int n1 = odd ? p - 1 - i : i, n2 = odd ? p - 1 - j : j, n0 = e - n1 - n2;
          const float fe = (float)e;
          w[0] = xf_div((float)n0, fe);
          w[1] = xf_div((float)n1, fe);
          w[2] = xf_div((float)n2, fe);
          const float r = xf_sqrt(q);
          const float half = xf_mul(0.5f, ray_length);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float pc = xf_add(xf_add(xf_mul(w[0], v0[c]), xf_mul(w[1], v1[c])), xf_mul(w[2], v2[c]));
            const float nh = xf_div(n[c], r);
            d[c] = -nh;
            o[c] = xf_add(pc, xf_mul(half, nh));
          }
          near = 0.0f;
          far = ray_length;
          face = f;
        }
      }
    }
    nears[base + tid] = near;
    fars[base + tid] = far;
    texel_face[base + tid] = face;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    stage_o[3 * tid + c] = o[c];
    stage_d[3 * tid + c] = d[c];
    stage_w[3 * tid + c] = w[c];
  }
  __syncthreads();
  tex_store_rows(stage_o, origins, base, count);
  tex_store_rows(stage_d, directions, base, count);
  if (bary) tex_store_rows(stage_w, bary, base, count);
}

extern "C" int umhs_texture_rays(const float* positions, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int px,
                                 float ray_length, int64_t texel_begin, int64_t texel_end, float* origins, float* directions,
                                 float* nears, float* fars, int32_t* texel_face, float* bary, umhs_stream_t stream) {
  int64_t Q, T;
  const int rc = tex_atlas(n_faces, px, Q, T);
  if (rc != UMHS_OK) return rc;
  if (!(ray_length > 0.0f) || !xf_finite(ray_length)) return UMHS_ERR_ARG;
  if (texel_begin < 0 || texel_end < texel_begin || texel_end > T * T) return UMHS_ERR_ARG;
  if (n_vertices < 1) return UMHS_ERR_ARG;
  if (n_vertices > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;  // (int32 indices cannot name more)
  if (!positions || !faces || !origins || !directions || !nears || !fars || !texel_face) return UMHS_ERR_ARG;
  const int64_t n = texel_end - texel_begin;  // <= 2^28
  if (n == 0) return UMHS_OK;
  const unsigned blocks = (unsigned)((n + TEX_THREADS - 1) / TEX_THREADS);
  hipLaunchKernelGGL(texture_rays_kernel, dim3(blocks), dim3(TEX_THREADS), 0, umhs_s(stream), positions, (uint32_t)n_vertices, faces,
                     (int)n_faces, px, (int)Q, (int)T, ray_length, (int)texel_begin, (int)n, origins, directions, nears, fars,
                     texel_face, bary);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
