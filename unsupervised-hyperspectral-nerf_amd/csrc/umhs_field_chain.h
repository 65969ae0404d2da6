// Fused per-sample UMHS field for gfx950 (R3-R9, R18): mlp_base MLP, NeRF/SH encodings, mlp_head,
// feature_mlp, mlp_directional, sigmoid / temperature-softmax and endmember mixing, forward and
// backward, on the f32-input MFMA (v_mfma_f32_16x16x4_f32: exact f32 fmaf chain, needed for the 1e-4
// radiance parity).  Reference: umhs_field.py:151-261,300-329.
//
// Data flow ("samples on lanes"): every GEMM is computed transposed, Y^T[out][sample] = W[out][in] X^T,
// with the WEIGHTS as the MFMA A operand and the ACTIVATIONS as the B operand.  A 16x16 result tile
// then has its 16 samples on lane&15 and its 16 output features on (lane>>4, reg) -- which is exactly
// the B-operand shape of the next layer (k-slot <-> lane>>4), so an accumulator register feeds the
// next MFMA directly: no LDS transpose, no cross-lane traffic between layers.  The price is a permuted
// k order, paid once by packing each weight matrix in the matching order (fwd image in LDS; the
// transposed images for dX come from global/L2).  Bias rides in as the initial accumulator.
//
// This header: what the forward and the backward kernels share -- layer / pack descriptors and the pack images, the fp32 MFMA GEMM
// (gemm_pack) and its three-piece bf16 form (gemm_bf), encodings and head epilogue, FieldIO, the LDS image copy.  The kernels are in
// umhs_field.hip (forward, small kernels, host side) and umhs_field_bwd.h (backward).
#pragma once

#include "umhs_common.h"

typedef float v4f __attribute__((ext_vector_type(4)));

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

enum InKind { IN_ENC = 0, IN_HID64 = 1, IN_HID16 = 2, IN_27 = 3, IN_DIR28 = 4, IN_MIX = 5 };
enum LayerId { L_B0 = 0, L_B1, L_H0, L_H1, L_H2, L_F0, L_F1, L_F2, L_D0, L_D1, L_MX, NLAYERS };

struct LayerDesc {
  const float* W;  // [OUT][IN] row-major (L_MX: endmembers [C][B], addressed transposed)
  const float* b;  // [OUT] or null
  int kind, KS, OT, OUT, IN;
  int off_w, off_b;  // float offsets in the forward pack image
};
struct PackDesc {
  LayerDesc L[NLAYERS];
  int total_w, total;  // floats
};

// k-slot (step s, lane quarter q) -> column of the reference weight matrix, or -1
__device__ __forceinline__ int kmap_in(int kind, int s, int q) {
  switch (kind) {
    case IN_ENC: return 8 * q + s;
    case IN_HID64: return 16 * (s >> 2) + 4 * q + (s & 3);
    case IN_HID16: return 4 * q + s;
    case IN_27: {
      if (s < 3) return 3 * q + s;            // positional encoding p = 3q+s
      int e = 4 * q + (s - 3) - 1;            // base-MLP output slot 4q+r, slot 0 is sigma_raw
      return e >= 0 ? 12 + e : -1;
    }
    case IN_DIR28: return s < 4 ? 4 * q + s : 16 + 3 * q + (s - 4);
    default: return 4 * q + s;  // IN_MIX: class index
  }
}

// forward pack image: for each layer, A-operand values in the exact order the waves consume them:
//   w[off_w + ((t*KS4 + s4)*64 + lane)*4 + ss] = W[16t + (lane&15)][kmap(4*s4+ss, lane>>4)]
__device__ __forceinline__ float fwd_pack_value(const PackDesc& pd, int idx) {
  int li = 0;
  while (li + 1 < NLAYERS && idx >= pd.L[li + 1].off_w) ++li;
  const LayerDesc& L = pd.L[li];
  const int rel = idx - L.off_w;
  const int ss = rel & 3, ln = (rel >> 2) & 63, blk = rel >> 8;
  const int KS4 = (L.KS + 3) >> 2;
  const int t = blk / KS4, s = (blk % KS4) * 4 + ss;
  const int out = 16 * t + (ln & 15), q = ln >> 4;
  if (s >= L.KS || out >= L.OUT) return 0.0f;
  const int in = kmap_in(L.kind, s, q);
  if (li == L_MX) return (in >= 0 && in < L.IN) ? L.W[(size_t)in * L.OUT + out] : 0.0f;  // E[c][b]
  return (in >= 0 && in < L.IN) ? L.W[(size_t)out * L.IN + in] : 0.0f;
}

__device__ __forceinline__ void build_fwd_image(float* lds, const PackDesc& pd) {
  for (int idx = threadIdx.x; idx < pd.total_w; idx += blockDim.x) lds[idx] = fwd_pack_value(pd, idx);
  for (int li = 0; li < NLAYERS; ++li) {
    const LayerDesc& L = pd.L[li];
    if (li == L_MX) continue;
    for (int o = threadIdx.x; o < 16 * L.OT; o += blockDim.x) lds[L.off_b + o] = (L.b && o < L.OUT) ? L.b[o] : 0.0f;
  }
}

// LDS image = image[first .. total): copy when a prebuilt image is given, else gather-build in place
__device__ __forceinline__ void load_fwd_image(float* lds, const PackDesc& pd, const float* __restrict__ image, int first) {
  if (image) {
    const int n4 = (pd.total - first + 3) >> 2;  // first and the image buffer are 16-byte aligned
    for (int i = threadIdx.x; i < n4; i += blockDim.x)
      reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(image + first)[i];
  } else {
    build_fwd_image(lds - first, pd);
  }
}

// acc[ct][t] (+)= W-pack(t, :) x B-operand regs b[ct][:]   (A from LDS or global, 16 B per lane per 4 k-steps)
// INIT: 0 = accumulate into acc, 1 = start from zero, 2 = start from the bias (compile-time: a runtime `if (bias)` is a
// real branch -- LDS address 0 is valid -- and every branch ends a scheduling region, pinning the operand loads to
// their gemm instead of letting them be hoisted over the previous one)
// Software pipeline: the A fragments (one ds_read_b128 = 4 k-steps of one output tile) are consumed in bundles of G; the
// next bundle's reads are issued BEFORE the current bundle's MFMAs (the compiler on its own emits read -> s_waitcnt
// lgkmcnt(0) -> MFMAs, exposing the LDS latency once per fragment), and inside a bundle the MFMAs alternate between
// >= 2 accumulators so that none waits on its predecessor (32-cycle issue vs 40-cycle dependent issue).
// SWAP: operands exchanged -> the TRANSPOSED tile D[sample 4q+r][feature lane&15] (the same pack image serves: lane l holds
// W[out = l&15][in = l>>4] either way); used for the last layers so that output rows are written 16 consecutive floats
// per quarter-wave instead of one float per row.
template <int OT, int KS, int NT, int INIT, bool SWAP = false>
__device__ __forceinline__ void gemm_pack(v4f (&acc)[NT][OT], const float (&b)[NT][KS], const float* __restrict__ w,
                                          const float* __restrict__ bias, int lane) {
  constexpr int KS4 = (KS + 3) / 4;
  constexpr int NF = KS4 * OT;                 // fragment f = s4 * OT + t
  constexpr bool SPLIT = (OT == 1 && NT == 1 && KS4 >= 2);  // one tile, one column block: split K over two accumulators
  constexpr int G = (NT >= 2) ? 1 : 2;
  constexpr int NBUN = (NF + G - 1) / G;
  if (INIT != 0) {
#pragma unroll
    for (int t = 0; t < OT; ++t) {
      v4f bv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (INIT == 2 && !SWAP) bv = *reinterpret_cast<const v4f*>(bias + 16 * t + 4 * (lane >> 4));
      if (INIT == 2 && SWAP) {
        const float bj = bias[16 * t + (lane & 15)];
        bv = v4f{bj, bj, bj, bj};
      }
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) acc[ct][t] = bv;
    }
  }
  v4f acc2 = {0.0f, 0.0f, 0.0f, 0.0f};
  v4f a[2][G];
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (g < NF) a[0][g] = *reinterpret_cast<const v4f*>(w + (((g % OT) * KS4 + g / OT) * 64 + lane) * 4);
#pragma unroll
  for (int bun = 0; bun < NBUN; ++bun) {
    if (bun + 1 < NBUN) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int f = (bun + 1) * G + g;
        if (f < NF) a[(bun + 1) & 1][g] = *reinterpret_cast<const v4f*>(w + (((f % OT) * KS4 + f / OT) * 64 + lane) * 4);
      }
    }
    __builtin_amdgcn_sched_barrier(0x7ff & ~0x180);  // everything but LDS reads may move across: the prefetch stays ahead
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int f = bun * G + g, s4 = f / OT, t = f % OT;
        if (f < NF && s4 * 4 + ss < KS) {
          if (SPLIT && (f & 1)) {
            acc2 = SWAP ? MFMA(b[0][s4 * 4 + ss], a[bun & 1][g][ss], acc2) : MFMA(a[bun & 1][g][ss], b[0][s4 * 4 + ss], acc2);
          } else {
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
              acc[ct][t] = SWAP ? MFMA(b[ct][s4 * 4 + ss], a[bun & 1][g][ss], acc[ct][t])
                                : MFMA(a[bun & 1][g][ss], b[ct][s4 * 4 + ss], acc[ct][t]);
          }
        }
      }
    }
  }
  if (SPLIT) acc[0][0] += acc2;
}

// relu as ONE integer max on the bit pattern (negative floats are negative ints; +NaN stays NaN like torch.relu);
// fmaxf() on an MFMA result costs two instructions because hipcc first canonicalises a possible sNaN
__device__ __forceinline__ float relu1(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

template <int OT, int NT>
__device__ __forceinline__ void relu_to(float (&x)[NT][OT * 4], const v4f (&acc)[NT][OT]) {
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int t = 0; t < OT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[ct][4 * t + r] = relu1(acc[ct][t][r]);
}

// exp via v_exp_f32 (2^x) and reciprocal via v_rcp_f32: ~1e-7..1e-6 relative error for the |x| <~ 30 seen here, an
// order of magnitude inside the parity budget, and ~10x fewer instructions than the IEEE sequences between MFMAs
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sigmoidf_(float x) { return frcp(1.0f + fexp(-x)); }
// Reductions over the 4 lane quarters (lanes l, l^16, l^32, l^48).  gfx950's v_permlane16_swap / v_permlane32_swap exchange the odd
// 16-lane rows (resp. the upper 32 lanes) of one operand with the even rows (lower half) of the other: called with v for both,
// the two results are v's even-row and odd-row (lower / upper half) copies, i.e. {v, v from the partner quarter} in every lane --
// pure VALU, where __shfl_xor compiles to ds_bpermute_b32 and pays an LDS round trip (9 of them per tile of the backward, with
// nothing else on the SIMD to cover them).  Same values, same association as the shuffles they replace.
typedef unsigned v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float xq_max(float v) {
  v2u a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
__device__ __forceinline__ float xq_sum(float v) {
  v2u a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
// sum over the 16 lanes of a DPP row (the lanes that share a quarter q), result in every lane: four rotate-and-add steps on the
// VALU (row_ror 8 / 4 / 2 / 1) -- __shfl_xor compiles to ds_bpermute here, ~100 cycles of LDS latency per step that a kernel at one
// wave per SIMD cannot hide (part 0 of the backward: +14 us at C2 with four of those per value)
__device__ __forceinline__ float row_sum16(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));  // row_ror:8
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));  // row_ror:4
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));  // row_ror:2
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));  // row_ror:1
  return v;
}
__device__ __forceinline__ float sel4(const v4f& v, int r) { return r == 0 ? v[0] : (r == 1 ? v[1] : (r == 2 ? v[2] : v[3])); }

struct FieldIO {
  const float* enc;
  int64_t sn, sl;
  const float *wpos, *dirs, *sel;
  int64_t n;
  int B, C, TB;
  float temperature;
  // forward outputs
  float *sigma, *sigma_raw, *emb, *spectral, *spectral2, *specular, *abund;
  // backward
  const float *d_sigma, *d_spectral, *d_emb;
  float* d_enc;
  const float *emb_in, *sigma_raw_in;  // saved forward outputs (heads / base backward)
  float* d_bo;                         // [N,16] gradient w.r.t. the base MLP's outputs (heads -> base)
  float* feat_logits;                  // forward: optional [N,16] feature_mlp logits (rows 0..C), saved for the split backward
  const float* feat_logits_in;         // split backward, part 0
  float* d_fl;                         // [N,16] gradient w.r.t. the feature logits (part 0 -> part 1)
  float* d_bo2;                        // [N,16] part 1's share of d_bo (base kernel adds the two)
  // heads-only forward with the per-ray band sums taken inside the kernel (field_fwd_kernel<.., HEADS = true>)
  const float* weights;                // [N] rendering weights of the samples
  const int64_t* ray_of;               // [N] ray of each sample (non-decreasing)
  float* part;                         // per-16-sample-tile partial sums, see HeadsComp
  float* comp[3];                      // [R,B] band sums of spectral / spectral2 / specular (rays inside one tile are written here directly)
  int n_streams;                       // 1 without the specular head, else 3
  float* part_m;                       // w m (mixing input): per-tile partials [(g*2 + az)*16 + c]
  float* mix16;                        // [R,16] per-ray sums of w m (written here for rays strictly inside a tile, else by the finish pass)
  float* part_ab;                      // abundances: per-tile partials [(g*2 + az)*16 + c]
  float* comp_ab;                      // [R,C] per-ray abundance sums (or null)
  float* bo16;                         // density half: the base MLP's 16 outputs as aligned rows [N,16] (slot 0 = sigma_raw), or null
  const float* bo16_in;                // heads forward / backward part 0: read emb from such rows instead of [N,15]
  // transpose-free backward, part 0 with the compositing backward's value half folded in (FUSED): d_spectral[n][b] =
  // scale_n * weights[n] * d_comp[ray(n)][b] is formed on the fly, and dots[n] = sum_b d_comp[ray(n)][b] * spectral[n][b] goes out for
  // umhs_composite_bwd_dots (mixing half: sum_c m[c] (d_comp E^T)[c], which the kernel's d m accumulator already is; specular half
  // from the sigmoids it computes anyway)
  const float* d_comp;                 // [R,B] gradient w.r.t. the per-ray band sums of spectral
  const float* mix_g;                  // [R,16] G[r][c] = sum_b d_comp[r][b] E[c][b] (field_mix_grad_kernel): d m_n = ws_n G[ray(n)]
  float* part_ms;                      // per-tile partials of ws_n m_n [(g*2 + az)*16 + c] (-> dE = (sum_n ws_n m_n)^T d_comp per ray)
  float* mws16;                        // [R,16] the same sums for rays strictly inside one tile
  const float *t0, *t1;                // [N] sample intervals (gradient scaling by distance), or null
  float* dots;                         // [N]
};

// NeRF positional encoding slots of quarter q (3 per lane) and SH slots (4 per lane)
__device__ __forceinline__ void pe_slots(float (&pe)[3], float x, float y, float z, int q) {
  const bool odd = q & 1;
  const float c0 = odd ? y : x, c1 = odd ? z : x, c2 = odd ? z : y;
  const float f0 = odd ? 2.0f : 1.0f, f1 = odd ? 1.0f : 2.0f, f2 = odd ? 2.0f : 1.0f;
  // sin(2 pi x f [+ pi/2]) as v_sin_f32 of the phase in revolutions (x f [+ 1/4], reduced by v_fract): ~1e-6 absolute, an
  // order of magnitude inside the parity budget; the libm sinf it replaces was ~6 % of the forward kernel (range reduction)
  float r0 = c0 * f0, r1 = c1 * f1, r2 = c2 * f2;
  if (q >= 2) r0 += 0.25f, r1 += 0.25f, r2 += 0.25f;
  pe[0] = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(r0));
  pe[1] = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(r1));
  pe[2] = __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(r2));
}

__device__ __forceinline__ void sh_slots(float (&sh)[4], float dx, float dy, float dz, int q) {
  const float x = (dx + 1.0f) / 2.0f, y = (dy + 1.0f) / 2.0f, z = (dz + 1.0f) / 2.0f;
  const float xx = x * x, yy = y * y, zz = z * z;
  if (q == 0) {
    sh[0] = 0.28209479177387814f, sh[1] = 0.4886025119029199f * y, sh[2] = 0.4886025119029199f * z;
    sh[3] = 0.4886025119029199f * x;
  } else if (q == 1) {
    sh[0] = 1.0925484305920792f * x * y, sh[1] = 1.0925484305920792f * y * z;
    sh[2] = 0.9461746957575601f * zz - 0.31539156525251999f, sh[3] = 1.0925484305920792f * x * z;
  } else if (q == 2) {
    sh[0] = 0.5462742152960396f * (xx - yy), sh[1] = 0.5900435899266435f * y * (3.0f * xx - yy);
    sh[2] = 2.890611442640554f * x * y * z, sh[3] = 0.4570457994644658f * y * (5.0f * zz - 1.0f);
  } else {
    sh[0] = 0.3731763325901154f * z * (5.0f * zz - 3.0f), sh[1] = 0.4570457994644658f * x * (5.0f * zz - 1.0f);
    sh[2] = 1.445305721320277f * z * (xx - yy), sh[3] = 0.5900435899266435f * x * (xx - 3.0f * yy);
  }
}

// Everything the heads need, recomputed per 16-sample column tile (NT tiles per wave).
template <int NT>
struct HeadState {
  float m[NT][4];   // sigmoid(head) * softmax(feat/T)   (rows c = 4q+r, zero for c >= C)
  float sg[NT][4];  // sigmoid(head)
  float ab[NT][4];  // abundances
  float s1[NT];     // sigmoid of the extra feature logit (specular gate)
};

template <int NT, bool SPEC>
__device__ __forceinline__ void head_epilogue(HeadState<NT>& hs, const v4f (&hd4)[NT][1], const v4f (&fl4)[NT][1], int C,
                                              float temperature, int lane) {
  const int q = lane >> 4;
  const float inv_t = 1.0f / temperature;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    float z[4], zmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      z[r] = fl4[ct][0][r] * inv_t;
      if (4 * q + r < C) zmax = fmaxf(zmax, z[r]);
    }
    zmax = xq_max(zmax);
    float e[4], sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      e[r] = (4 * q + r < C) ? fexp(z[r] - zmax) : 0.0f;
      sum += e[r];
    }
    sum = frcp(xq_sum(sum));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool v = 4 * q + r < C;
      hs.ab[ct][r] = e[r] * sum;
      hs.sg[ct][r] = v ? sigmoidf_(hd4[ct][0][r]) : 0.0f;
      hs.m[ct][r] = hs.sg[ct][r] * hs.ab[ct][r];
    }
    if (SPEC) {
      const float mine = sel4(fl4[ct][0], C & 3);
      hs.s1[ct] = sigmoidf_(__shfl(mine, ((C >> 2) << 4) | (lane & 15), 64));
    } else {
      hs.s1[ct] = 0.0f;
    }
  }
}

template <int NT>
__device__ __forceinline__ void store_density(const FieldIO& io, const v4f (&bo4)[NT][1], const int64_t (&nn)[NT],
                                              const bool (&ok)[NT], int q) {
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    if (ok[ct]) {
      if (q == 0) {
        const float raw = bo4[ct][0][0];
        io.sigma[nn[ct]] = expf(raw) * io.sel[nn[ct]];
        if (io.sigma_raw) io.sigma_raw[nn[ct]] = raw;
      }
      if (io.emb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = 4 * q + r - 1;
          if (e >= 0) io.emb[nn[ct] * 15 + e] = bo4[ct][0][r];
        }
      }
      if (io.bo16) *reinterpret_cast<v4f*>(io.bo16 + nn[ct] * 16 + 4 * q) = bo4[ct][0];  // one 64-byte row per sample
    }
  }
}

// =============================================================================================
// Shared by the forward and the transpose-free backward: LDS image segments, the three-piece bf16 form of the fp32 GEMM chain
// =============================================================================================
struct ImgSegs {
  int n, src[6], dst[6], len[6];  // float offsets / lengths, multiples of 4
};
__device__ __forceinline__ void copy_segs(float* dst, const float* __restrict__ src, const ImgSegs& sg) {
  // Every workgroup of a launch copies the SAME image at the same moment: walking it in the same order queues all CUs of an XCD on
  // one L2 channel at a time (stamps: 21 k cycles from kernel start to the barrier behind the copy of ~100 KB, 6 % of the backward
  // kernels; 15-19 k with each workgroup starting at its own rotation of the chunk sequence; 8 unconditional loads in flight per
  // thread: 21 k again, 4-8 conditional ones 26-31 k).
  for (int k = 0; k < sg.n; ++k) {
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + sg.src[k]);
    float4* d4 = reinterpret_cast<float4*>(dst + sg.dst[k]);
    const int n4 = sg.len[k] >> 2, bd = blockDim.x;
    const int nfull = n4 / bd;  // whole chunks of blockDim float4s: copied without a condition, 4 loads in flight, rotated start
    const int c0 = nfull ? (int)((blockIdx.x * 7u) % (unsigned)nfull) : 0;
    int c = 0;
    for (; c + 4 <= nfull; c += 4) {
      float4 v[4];
      int idx[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int cc = c0 + c + u;
        cc = cc >= nfull ? cc - nfull : cc;
        idx[u] = cc * bd + (int)threadIdx.x;
        v[u] = s4[idx[u]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) d4[idx[u]] = v[u];
    }
    for (; c < nfull; ++c) {
      int cc = c0 + c;
      cc = cc >= nfull ? cc - nfull : cc;
      d4[cc * bd + threadIdx.x] = s4[cc * bd + threadIdx.x];
    }
    const int i = nfull * bd + threadIdx.x;  // the partial last chunk
    if (i < n4) d4[i] = s4[i];
  }
}

enum TLayerId { T_B1 = 0, T_B0, T_H2, T_H1, T_H0, T_F2, T_F1, T_F0, T_D1, T_MX, NTLAYERS };

typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
typedef float v2f __attribute__((ext_vector_type(2)));
// two floats -> their bf16 roundings (nearest even) in one dword (v_cvt_pk_bf16_f32), low half = a
__device__ __forceinline__ uint32_t cvt_pk_bf(float a, float b) {
  const v2f v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, v2bf));
}
// (x0, x1) -> packed bf16 pieces: h = rne(x), m = rne(x - h) [, l = rne(x - h - m)]; the subtractions are exact.  The transposes of
// the dW operands and the chain's three-piece products call this on the same registers: the compiler keeps one computation.
__device__ __forceinline__ void bf_split_pair(float x0, float x1, uint32_t& h, uint32_t& m, float& r0, float& r1) {
  h = cvt_pk_bf(x0, x1);
  r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = cvt_pk_bf(r0, r1);
}
__device__ __forceinline__ void bf_split_pair3(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l) {
  float r0, r1;
  bf_split_pair(x0, x1, h, m, r0, r1);
  l = cvt_pk_bf(r0 - __uint_as_float(m << 16), r1 - __uint_as_float(m & 0xffff0000u));
}

// ---- the exact fp32 chain on the bf16 MFMA: x = hi + mid + lo (three bf16 pieces, |x - hi - mid - lo| <= 2^-25 |x|), a product
// a*b = hh + hm + mh + hl + lh + mm (the three terms left out are <= 2^-24 |ab|: fp32's own rounding), exact bf16 products,
// fp32 accumulation.  v_mfma_f32_16x16x32_bf16 issues in half the cycles of v_mfma_f32_16x16x4_f32 for 8x its K, so a 64-wide
// layer costs 12 bf16 MFMAs per output tile instead of 16 fp32 ones at half the cycles each: 0.375x the matrix time.
// Pack images: the fp32 images re-laid for K = 32 (lane (out, q) holds the weights of k-slots 8S+u, u < 8: the SAME k-slots as
// steps 8S .. 8S+7 of the fp32 form, so the activation registers are used in the order they are) and split into the three pieces:
//   wbf[off + ((((t*K8 + S)*3 + piece)*64 + lane)*4 + u/2] = pack(piece(w(t, 8S+u, lane)), piece(w(t, 8S+u+1, lane)))      (dwords)
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

struct BfConv {  // one converted layer: where its fp32 pack sits in its source image, where the bf16x3 pack goes
  int src_img, src_off, KS4, OT, dst_off;  // src_img 0: forward pack image, 1: transposed pack image
};
struct BfPlan {
  int n, total;  // dwords
  BfConv c[16];
};
__device__ __forceinline__ void bf_split3_scalar(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
  const __bf16 bh = (__bf16)x;
  const float r1 = x - (float)bh;
  const __bf16 bm = (__bf16)r1;
  const float r2 = r1 - (float)bm;
  const __bf16 bl = (__bf16)r2;
  h = (uint16_t)__builtin_bit_cast(short, bh), m = (uint16_t)__builtin_bit_cast(short, bm), l = (uint16_t)__builtin_bit_cast(short, bl);
}
// acc[ct][t] (+)= W-pack(t, :) x b[ct][:] with the three-piece bf16 products (same INIT meaning and result tile layout as gemm_pack
// -- the C/D map of the MFMA does not depend on the input type; the NT sample tiles share every weight fragment)
template <int OT, int KS, int NT, int INIT>
__device__ __forceinline__ void gemm_bf(v4f (&acc)[NT][OT], const float (&b)[NT][KS], const uint32_t* __restrict__ w,
                                        const float* __restrict__ bias, int lane) {
  constexpr int K8 = (KS + 7) / 8;
  constexpr int NF = OT * K8;  // fragment f = S * OT + t (k-step major), three 16-byte pieces each
  constexpr int PF = 2 < NF ? 2 : NF;  // requested PF fragments ahead
  v4u A[PF + 1][3];
  auto load = [&](int f, int slot) __attribute__((always_inline)) {
    const int t = f % OT, S = f / OT;
    const uint32_t* pw = w + (((t * K8 + S) * 3) * 64 + lane) * 4;
#pragma unroll
    for (int p = 0; p < 3; ++p) A[slot][p] = *reinterpret_cast<const v4u*>(pw + p * 256);
  };
  // Stamps of the backward (tools/stamp_fbwd.py) gave 33-42 cycles per v_mfma_f32_16x16x32 in every gemm of a one-wave-per-SIMD kernel,
  // against the pipe's 16: the ISA had each fragment's ds_read_b128s right in front of its MFMAs with s_waitcnt lgkmcnt(0) in between --
  // under register pressure the scheduler sinks the reads this loop requests ahead down to their uses (a barrier that masked only the
  // LDS reads kept their order, no more).  So every step is a scheduling region of its own, [reads of fragment f + PF] [products of
  // fragment f], and the first PF fragments (and the bias tile) are requested BEFORE the bf16 splits of the B operand, ~70 VALU
  // instructions that cover their latency: 19-20 cycles per MFMA.
  v4f bv[OT];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int f = 0; f < PF; ++f) load(f, f);
  if (INIT == 2) {
#pragma unroll
    for (int t = 0; t < OT; ++t) bv[t] = *reinterpret_cast<const v4f*>(bias + 16 * t + 4 * (lane >> 4));
  }
  __builtin_amdgcn_sched_barrier(0);
  v4u B[NT][3][K8];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
#pragma unroll
    for (int S = 0; S < K8; ++S)
#pragma unroll
      for (int up = 0; up < 4; ++up) {
        const int s0 = 8 * S + 2 * up;  // KS is even or the last slot is a zero pad
        uint32_t h, m, l;
        bf_split_pair3(s0 < KS ? b[ct][s0 < KS ? s0 : 0] : 0.0f, s0 + 1 < KS ? b[ct][s0 + 1 < KS ? s0 + 1 : 0] : 0.0f, h, m, l);
        B[ct][0][S][up] = h, B[ct][1][S][up] = m, B[ct][2][S][up] = l;
      }
  if (INIT != 0) {
#pragma unroll
    for (int t = 0; t < OT; ++t) {
      v4f bvt = {0.0f, 0.0f, 0.0f, 0.0f};
      if (INIT == 2) bvt = bv[t];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) acc[ct][t] = bvt;
    }
  }
  auto mf = [](const v4u& a, const v4u& bb, const v4f& c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, bb), c, 0, 0, 0);
  };
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    __builtin_amdgcn_sched_barrier(0);
    if (f + PF < NF) load(f + PF, (f + PF) % (PF + 1));
    __builtin_amdgcn_sched_barrier(0);
    const int t = f % OT, S = f / OT, k = f % (PF + 1);
    constexpr int PA[6] = {0, 0, 1, 0, 2, 1}, PB[6] = {0, 1, 0, 2, 0, 1};  // hh, hm, mh, hl, lh, mm
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) acc[ct][t] = mf(A[k][PA[p]], B[ct][PB[p]][S], acc[ct][t]);
  }
  __builtin_amdgcn_sched_barrier(0);
}

struct BfOffs {  // LDS dword offsets (from the bf16 region) of the converted layers' bf16x3 packs, -1: layer keeps its fp32 pack
  int f[NLAYERS], t[NTLAYERS];
};

// =============================================================================================
// Transposed pack images (A operands of the backward's dX chain), built once per call in global memory (L2-resident).
// =============================================================================================
struct TDesc {
  const float* W;
  int OUT, IN, KS, OT, rowmap, off;  // rowmap 0: in = rho, 1: emb slots of the 27-d input, 2: L_MX (E[c=rho][b=k])
};
struct TPackDesc {
  TDesc L[NTLAYERS];
  int total;
};

//   wT[off + ((t*KS4 + s4)*64 + lane)*4 + ss] = W[k(4*s4+ss, lane>>4)][rowmap(16t + (lane&15))]
__device__ __forceinline__ float t_pack_value(const TPackDesc& td, int idx) {
  int li = 0;
  while (li + 1 < NTLAYERS && idx >= td.L[li + 1].off) ++li;
  const TDesc& L = td.L[li];
  const int rel = idx - L.off;
  const int ss = rel & 3, ln = (rel >> 2) & 63, blk = rel >> 8;
  const int KS4 = (L.KS + 3) >> 2;
  const int t = blk / KS4, s = (blk % KS4) * 4 + ss;
  const int rho = 16 * t + (ln & 15), q = ln >> 4;
  const int k = 16 * (s >> 2) + 4 * q + (s & 3);  // dZ row held by (step s, quarter q)
  float v = 0.0f;
  if (L.rowmap == 2) {
    if (rho < L.OUT && k < L.IN) v = L.W[(size_t)rho * L.IN + k];  // E[c][b], OUT=C, IN=B
  } else if (s < L.KS && k < L.OUT) {
    int in = rho;
    if (L.rowmap == 1) in = (rho >= 1 && rho <= 15) ? 12 + rho - 1 : -1;
    if (in >= 0 && in < L.IN) v = L.W[(size_t)k * L.IN + in];
  }
  return v;
}
