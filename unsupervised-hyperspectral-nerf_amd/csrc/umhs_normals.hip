// Density-gradient normals (include/umhs_hip.h, "Density-gradient normals"): per sample, the analytic gradient of the density with
// respect to the WORLD position -- the trilinear hash grid differentiated with respect to pos01, mlp_base (32 -> 64 -> 16, output 0)
// differentiated with respect to its input, and the Jacobian of the scene contraction (or of the box normalisation) -- and
// nerfstudio's normal -grad / (|grad| + 1e-10).  No gradient-free path of the package needs d/d(position) otherwise; the backward
// kernels stop at the table and the weights.
//
// Shape: ONE SAMPLE PER LANE, 64 per wave, nothing shared between lanes -- no barrier, no atomics, nothing of size [N, 32, 3] ever
// stored.  Per lane:
//   1. the 32 hash features: read from the level-major enc the render path has gathered, or gathered here with the forward's own
//      hash_corners / hash_gather8 / hash_trilerp (umhs_hash.h: the same expression tree, contraction off, so the same bits);
//   2. ONE pass over the 64 hidden units: h_k = b0[k] + W0[k,:] . enc (an fma chain in j order), c_k = h_k > 0 ? W1[0,k] : 0,
//      sigma_raw += c_k h_k, q += c_k W0[k,:].  h is never stored: the ReLU mask is consumed by the unit that produced it.  The weights
//      are wave-uniform, so hipcc reads each row with scalar loads (the scalar cache holds all 8.5 KB) and every v_fma_f32 takes its
//      weight as an SGPR operand;
//   3. a walk over the 16 levels: the 8 corners again, the three axis derivatives of the blend for both features,
//      g01 += scale_l (q_{2l} d_0 + q_{2l+1} d_1).  This walk is what the kernel's time is made of (a lane that visits
//      all sixteen levels keeps sixteen tables in play, where the level-by-level gather kernel keeps one);
//   4. Jacobian, trunc_exp' = exp(clamp(sigma_raw, -15, 15)), selector, normal.
// Why the vector ALU and not the fp32 MFMA chain of umhs_rgb.hip: v_mfma_f32_16x16x4_f32 runs at the f32 VECTOR rate on gfx950
// (64 FLOP/clk/SIMD either way), so the matrix core buys no time for exact fp32, while the MFMA form costs an LDS weight image, a
// 16-sample tile shape that has to be transposed into the 64-sample gather shape twice (enc in, q out), and 64 live h registers for the
// mask.  Here both products are 2 x 2048 v_fma_f32 per sample, as many FLOP as the MFMA chain issues.
#include "umhs_hash.h"

namespace {

constexpr int NH = 64;   // hidden width of mlp_base
constexpr int NE = 32;   // 16 levels x 2 features
constexpr int NL = 16;

struct NormalsArgs {
  const float *pos01, *wpos, *sel, *enc, *scalings;
  const float2* table;
  int64_t n;
  int log2_T, contraction;
  float ax, ay, az, bx, by, bz;
  float *grad, *normal, *g01;
};

// d(blend)/d(offset) on the three axes for one feature: the forward's blend tree with the two corners of an axis replaced by their
// difference (ceil - floor).  Where ceil == floor on an axis both corners are the same slot and the difference is an exact 0.
__device__ __forceinline__ void hash_dblend(const float (&f)[8], float ox, float oy, float oz, float& dx, float& dy, float& dz) {
#pragma clang fp contract(off)
  const float rx = 1.0f - ox, ry = 1.0f - oy, rz = 1.0f - oz;
  dx = ((f[0] - f[3]) * oy + (f[1] - f[2]) * ry) * oz + ((f[4] - f[7]) * oy + (f[5] - f[6]) * ry) * rz;
  dy = ((f[0] - f[1]) * ox + (f[3] - f[2]) * rx) * oz + ((f[4] - f[5]) * ox + (f[7] - f[6]) * rx) * rz;
  dz = ((f[0] - f[4]) * ox + (f[3] - f[7]) * rx) * oy + ((f[1] - f[5]) * ox + (f[2] - f[6]) * rx) * ry;
}

// Both level walks are ROLLED loops (one level's 8 corners in flight per lane; unrolled, hipcc sinks all sixteen blends below the last
// fetch and keeps 16 x 24 corner registers alive -- it spilled).  A rolled loop cannot index a register array by the level, so the
// lane's 32 features, and later its 32 q values, pass through a lane-private LDS column col[j][thread] (conflict-free, no barrier:
// no lane reads another lane's column).  32 KB per block, 5 blocks per CU.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void density_normals_kernel(
    NormalsArgs a, const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1, const float* __restrict__ b1) {
  // (w0 [64][32], b0 [64], w1 [16][64]: row 0 is read, b1 [16]: element 0 is read.  Parameters of their own, const and restrict:
  // that is what lets hipcc read them with scalar loads)
  __shared__ float col[NE][256];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  if (i >= a.n) return;
  const float px = a.pos01[3 * i], py = a.pos01[3 * i + 1], pz = a.pos01[3 * i + 2];
  const uint32_t mask = (1u << a.log2_T) - 1u;

  // 1. the features
  float enc[NE];
  if (a.enc) {
    const float2* e2 = reinterpret_cast<const float2*>(a.enc);
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const float2 v = e2[(int64_t)l * a.n + i];
      enc[2 * l] = v.x, enc[2 * l + 1] = v.y;
    }
  } else {
#pragma unroll 1
    for (int l = 0; l < NL; ++l) {
      const HashCorners h = hash_corners(px, py, pz, a.scalings[l], mask, (uint32_t)l << a.log2_T);
      float2 f[8];
      hash_gather8(a.table, h, f);
      const float2 v = hash_trilerp(f, h.ox, h.oy, h.oz);
      col[2 * l][tid] = v.x, col[2 * l + 1][tid] = v.y;
    }
#pragma unroll
    for (int j = 0; j < NE; ++j) enc[j] = col[j][tid];
  }

  // 2. mlp_base: sigma_raw and q = W0^T (1[h > 0] . W1[0,:])
  float q[NE];
#pragma unroll
  for (int j = 0; j < NE; ++j) q[j] = 0.0f;
  float sigma = b1[0];
#pragma unroll 1
  for (int k = 0; k < NH; ++k) {
    const float* __restrict__ wr = w0 + k * NE;
    float h = b0[k];
#pragma unroll
    for (int j = 0; j < NE; ++j) h = fmaf(wr[j], enc[j], h);
    const float c = h > 0.0f ? w1[k] : 0.0f;
    sigma = fmaf(c, h, sigma);
#pragma unroll
    for (int j = 0; j < NE; ++j) q[j] = fmaf(c, wr[j], q[j]);
  }

  // 3. g01 = sum_j q_j d enc_j / d pos01
#pragma unroll
  for (int j = 0; j < NE; ++j) col[j][tid] = q[j];
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll 1
  for (int l = 0; l < NL; ++l) {
    const float s = a.scalings[l];
    const HashCorners h = hash_corners(px, py, pz, s, mask, (uint32_t)l << a.log2_T);
    float2 f[8];
    hash_gather8(a.table, h, f);
    float f0[8], f1[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) f0[c] = f[c].x, f1[c] = f[c].y;
    float dx0, dy0, dz0, dx1, dy1, dz1;
    hash_dblend(f0, h.ox, h.oy, h.oz, dx0, dy0, dz0);
    hash_dblend(f1, h.ox, h.oy, h.oz, dx1, dy1, dz1);
    const float q0 = col[2 * l][tid], q1 = col[2 * l + 1][tid];
    gx = fmaf(s, fmaf(q1, dx1, q0 * dx0), gx);
    gy = fmaf(s, fmaf(q1, dy1, q0 * dy0), gy);
    gz = fmaf(s, fmaf(q1, dz1, q0 * dz0), gz);
  }
  if (a.g01) a.g01[3 * i] = gx, a.g01[3 * i + 1] = gy, a.g01[3 * i + 2] = gz;
  if (!a.grad && !a.normal) return;

  // 4. position Jacobian (transposed onto g01), trunc_exp', selector, normal
  float wx, wy, wz;
  if (a.contraction) {
    const float x0 = a.wpos[3 * i], x1 = a.wpos[3 * i + 1], x2 = a.wpos[3 * i + 2];
    const float a0 = fabsf(x0), a1 = fabsf(x1), a2 = fabsf(x2);
    const float m = fmaxf(a0, fmaxf(a1, a2));
    if (m < 1.0f) {
      wx = gx * 0.25f, wy = gy * 0.25f, wz = gz * 0.25f;
    } else {
      const int k = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);  // ties of the maximum: the lowest index wins
      const float r = 1.0f / m, r2 = r * r;
      const float s = 2.0f * r - r2, t = 2.0f * r2 * r - 2.0f * r2;
      const float xk = k == 0 ? x0 : (k == 1 ? x1 : x2);
      const float dot = fmaf(x2, gz, fmaf(x1, gy, x0 * gx));
      const float e = t * dot * (xk < 0.0f ? -1.0f : 1.0f);
      wx = fmaf(s, gx, k == 0 ? e : 0.0f) * 0.25f;
      wy = fmaf(s, gy, k == 1 ? e : 0.0f) * 0.25f;
      wz = fmaf(s, gz, k == 2 ? e : 0.0f) * 0.25f;
    }
  } else {
    wx = gx / (a.bx - a.ax), wy = gy / (a.by - a.ay), wz = gz / (a.bz - a.az);
  }
  const bool live = a.sel[i] != 0.0f;
  const float ex = expf(fminf(fmaxf(sigma, -15.0f), 15.0f));
  const float dgx = live ? ex * wx : 0.0f, dgy = live ? ex * wy : 0.0f, dgz = live ? ex * wz : 0.0f;  // sel == 0: exactly +0
  if (a.grad) a.grad[3 * i] = dgx, a.grad[3 * i + 1] = dgy, a.grad[3 * i + 2] = dgz;
  if (a.normal) {
    const float len = sqrtf(fmaf(dgz, dgz, fmaf(dgy, dgy, dgx * dgx))) + 1e-10f;
    a.normal[3 * i] = live ? -dgx / len : 0.0f;
    a.normal[3 * i + 1] = live ? -dgy / len : 0.0f;
    a.normal[3 * i + 2] = live ? -dgz / len : 0.0f;
  }
}

}  // namespace

extern "C" int umhs_density_normals(const float* pos01, const float* wpos, const float* sel, const float* enc, const float* table,
                                    const float* scalings, int log2_T, const float* w0, const float* b0, const float* w1,
                                    const float* b1, int contraction, const float* aabb, int64_t n, float* grad_out,
                                    float* normal_out, float* g01_out, umhs_stream_t stream) {
  if (n < 0 || !table || !scalings || !w0 || !b0 || !w1 || !b1 || log2_T < 1 || log2_T > 27) return UMHS_ERR_ARG;
  if (!grad_out && !normal_out && !g01_out) return UMHS_ERR_ARG;
  if (!contraction && !aabb && (grad_out || normal_out)) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  if (!pos01 || ((grad_out || normal_out) && (!sel || (contraction && !wpos)))) return UMHS_ERR_ARG;
  if (((uintptr_t)table & 15) || (enc && ((uintptr_t)enc & 7))) return UMHS_ERR_ARG;
  NormalsArgs a;
  a.pos01 = pos01, a.wpos = wpos, a.sel = sel, a.enc = enc, a.scalings = scalings;
  a.table = reinterpret_cast<const float2*>(table);
  a.n = n, a.log2_T = log2_T, a.contraction = contraction;
  a.ax = a.ay = a.az = -1.0f, a.bx = a.by = a.bz = 1.0f;
  if (aabb) a.ax = aabb[0], a.ay = aabb[1], a.az = aabb[2], a.bx = aabb[3], a.by = aabb[4], a.bz = aabb[5];
  a.grad = grad_out, a.normal = normal_out, a.g01 = g01_out;
  hipLaunchKernelGGL(density_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, umhs_s(stream), a, w0, b0, w1, b1);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
