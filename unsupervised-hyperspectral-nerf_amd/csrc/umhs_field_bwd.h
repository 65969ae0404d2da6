// Device code of the field's transpose-free backward: swapped bf16 tiles and the dW products on them, the fp32-chain kernel
// (field_bwd_tf_kernel) and, through umhs_field_zip.h, the zipped bf16x3-chain kernels; then the launcher macros of the three
// translation units that instantiate them (umhs_field_bwd_p0z.hip, umhs_field_bwd_p0f.hip, umhs_field_bwd_p1.hip).
#pragma once

#include "umhs_field_launch.h"

// =============================================================================================
// Backward recomputes the forward per 16-sample tile (saved: hash features, sigma_raw, emb, feature logits), runs the dX chain the
// same way with transposed packs, and forms dW = dZ X^T (contraction over samples, i.e. over lanes) from tiles transposed by an
// identity MFMA, as three bf16 products into accumulators every wave keeps in AGPRs for the whole launch; per-workgroup slabs are
// folded and summed by two small kernels (umhs_field.hip).  Two main kernels, no LDS staging and no barrier inside their loops:
//   PART 0: mlp_head + mlp_directional + mixing.  Reads the forward's emb and feature logits, emits d_fl [N,16] (gradient of
//           the feature logits) and d_bo [N,16] (its share of the gradient of the base MLP's outputs).
//   PART 1: feature_mlp + mlp_base.  Recomputes the base MLP from the hash features (so it needs no saved emb / sigma_raw),
//           consumes d_fl, d_bo, d_sigma, writes d_enc.
//
// The dX chain and the forward recompute are the exact fp32 MFMA chain of the forward (or its three-piece bf16 form).  The hard part
// is dW = dZ^T X, the contraction over samples (= over lanes in the "samples on lanes" layout).  Staging both operands through LDS
// to transpose them ([sample][feature] rows written with ds_write_b128, read back column-wise) was, by the PMC and the
// section ablations, ~100 us of staging and ~20 us of barriers for 58 us of MFMA work at C2.  Here a tile is transposed ON THE
// MATRIX PIPE: an fp32 value is split into two bf16 pieces (x = hi + lo + O(2^-17 x)), and one v_mfma_f32_16x16x16_bf16 of a
// piece against an identity B operand (every lane builds its fragment from its own id) yields the "swapped" tile -- lane =
// (feature l&15, quarter q), register r <-> sample 4q+r -- exactly, because the products are x * 1.  Two swapped tiles ARE the
// A and B operands of dW[out][in] += sum_s dZ[s][out] X[s][in] on the bf16 MFMA (k-slot <-> sample), evaluated as
// hi*hi + hi*lo + lo*hi with fp32 accumulation: 2^-16 relative per product, unbiased (round-to-nearest pieces), summed over
// 262 k samples -- well inside the 5e-5 gradient budget (tests/test_hip_parity.py::test_field_bwd, test_hip_trajectory.py).
// The bf16 MFMA issues in half the cycles of the fp32 one for 4x its K, so transposes + dW cost ~1/4 of the fp32 dW they replace.
// Consequence: every wave owns ALL dW tiles of its part for its own samples (148 / 174 accumulator registers at C2, 238 in
// part 0 at 192 bands) -- one wave per SIMD with the accumulators in AGPRs, four independent waves per workgroup, every weight
// pack (forward and transposed) LDS-resident for any band count the forward supports.
// =============================================================================================
typedef short v4s __attribute__((ext_vector_type(4)));
#define MFMA_BF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k((a), (b), (c), 0, 0, 0)

struct STile {  // swapped 16-feature x 16-sample tile in bf16 pieces: lane (feature c = l&15, q = l>>4), element r <-> sample 4q+r
  v4s hi, lo;
};

__device__ __forceinline__ v4s ident_frag(int lane) {  // B operand of the transposing MFMA: I[k = 4q+u][col c] = (k == c)
  const int c = lane & 15, q = lane >> 4;
  v4s f;
#pragma unroll
  for (int u = 0; u < 4; ++u) f[u] = ((c >> 2) == q && (c & 3) == u) ? (short)0x3F80 : (short)0;
  return f;
}
__device__ __forceinline__ v4s pack_hi16(const v4f& v) {  // the four values ARE bf16 numbers: keep their upper halves
  const uint32_t a = __builtin_amdgcn_perm(__float_as_uint(v[1]), __float_as_uint(v[0]), 0x07060302u);
  const uint32_t b = __builtin_amdgcn_perm(__float_as_uint(v[3]), __float_as_uint(v[2]), 0x07060302u);
  return __builtin_bit_cast(v4s, make_uint2(a, b));
}

// "samples on lanes" tiles (4 registers each: features 4q+r of a 16-feature tile, this lane's sample) -> swapped bf16 tiles.
// NTILE tiles at once, in three phases -- split every value into its bf16 pieces (VALU), all 2*NTILE transposing MFMAs back to
// back, then pack the results: with one wave per SIMD nothing else hides an MFMA's latency, so a tile-by-tile split -> MFMA ->
// pack chain would stall on every tile (PMC of the first version: SQ_WAIT_INST_ANY 36-44 % of the wave cycles).
// COLSUM: also adds each lane's share of the column sums (sum over its 4 samples; the 4 lane quarters are added by the reduce).
template <int NTILE, bool COLSUM>
__device__ __forceinline__ void to_swapped_n(STile* __restrict__ out, const float* __restrict__ x, const v4s& ident,
                                             float* __restrict__ colsum = nullptr) {
  v4s hi[NTILE], lo[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) {
    uint32_t h[2], m[2];
    float r0, r1;
#pragma unroll
    for (int e = 0; e < 2; ++e) bf_split_pair(x[4 * t + 2 * e], x[4 * t + 2 * e + 1], h[e], m[e], r0, r1);
    hi[t] = __builtin_bit_cast(v4s, make_uint2(h[0], h[1])), lo[t] = __builtin_bit_cast(v4s, make_uint2(m[0], m[1]));
  }
  const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};
  v4f dh[NTILE], dl[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) dh[t] = MFMA_BF(hi[t], ident, z);
#pragma unroll
  for (int t = 0; t < NTILE; ++t) dl[t] = MFMA_BF(lo[t], ident, z);
#pragma unroll
  for (int t = 0; t < NTILE; ++t) {
    if (COLSUM) colsum[t] += ((dh[t][0] + dh[t][1]) + (dh[t][2] + dh[t][3])) + ((dl[t][0] + dl[t][1]) + (dl[t][2] + dl[t][3]));
    out[t].hi = pack_hi16(dh[t]), out[t].lo = pack_hi16(dl[t]);
  }
}
template <bool COLSUM>
__device__ __forceinline__ STile to_swapped(const float* __restrict__ x4, const v4s& ident, float* colsum = nullptr) {
  STile s;
  to_swapped_n<1, COLSUM>(&s, x4, ident, colsum);
  return s;
}

// acc[to * TI + ti] += Z[to]^T X[ti]: three bf16 products per tile pair (hi*hi, hi*lo, lo*hi), the passes run over the ti's of a row so
// that no MFMA waits for the one before it on the same accumulator.
// These MFMAs are written as inline asm with the accumulators constrained to AGPRs ("+a"), and the field units are compiled with
// -amdgpu-mfma-vgpr-form: a kernel whose register budget exceeds 256 otherwise gets the AGPR form of EVERY MFMA, and each result the
// VALU touches (every ReLU input, every transposed tile: 516 of the 2,066 instructions of part 1's loop) is first copied out of the
// accumulator file with v_accvgpr_read.  With the flag the builtin MFMAs (fp32 chain, transposes) write VGPRs; only the dW
// accumulators, which nothing but these MFMAs touches until the end of the launch, live in AGPRs.
// Hazards the compiler cannot see inside the string: the A / B operands come out of v_perm_b32 (VALU write -> MFMA read: 2 wait
// states = the leading s_nop 1); an MFMA accumulating onto the previous one's D needs none; D is next read by v_accvgpr_read after
// the loop.
template <int TI>
__device__ __forceinline__ void dw_row(v4f* __restrict__ acc, const STile& z, const STile* __restrict__ X);
template <>
__device__ __forceinline__ void dw_row<1>(v4f* __restrict__ acc, const STile& z, const STile* __restrict__ X) {
  asm volatile(
      "s_nop 1\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %1, %3, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %1, %4, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %2, %3, %0"
      : "+a"(acc[0])
      : "v"(z.hi), "v"(z.lo), "v"(X[0].hi), "v"(X[0].lo));
}
template <>
__device__ __forceinline__ void dw_row<2>(v4f* __restrict__ acc, const STile& z, const STile* __restrict__ X) {
  asm volatile(
      "s_nop 1\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %2, %4, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %1, %2, %6, %1\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %2, %5, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %1, %2, %7, %1\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %3, %4, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %1, %3, %6, %1"
      : "+a"(acc[0]), "+a"(acc[1])
      : "v"(z.hi), "v"(z.lo), "v"(X[0].hi), "v"(X[0].lo), "v"(X[1].hi), "v"(X[1].lo));
}
template <>
__device__ __forceinline__ void dw_row<4>(v4f* __restrict__ acc, const STile& z, const STile* __restrict__ X) {
  asm volatile(
      "s_nop 1\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %4, %6, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %1, %4, %8, %1\n\t"
      "v_mfma_f32_16x16x16_bf16 %2, %4, %10, %2\n\t"
      "v_mfma_f32_16x16x16_bf16 %3, %4, %12, %3\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %4, %7, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %1, %4, %9, %1\n\t"
      "v_mfma_f32_16x16x16_bf16 %2, %4, %11, %2\n\t"
      "v_mfma_f32_16x16x16_bf16 %3, %4, %13, %3\n\t"
      "v_mfma_f32_16x16x16_bf16 %0, %5, %6, %0\n\t"
      "v_mfma_f32_16x16x16_bf16 %1, %5, %8, %1\n\t"
      "v_mfma_f32_16x16x16_bf16 %2, %5, %10, %2\n\t"
      "v_mfma_f32_16x16x16_bf16 %3, %5, %12, %3"
      : "+a"(acc[0]), "+a"(acc[1]), "+a"(acc[2]), "+a"(acc[3])
      : "v"(z.hi), "v"(z.lo), "v"(X[0].hi), "v"(X[0].lo), "v"(X[1].hi), "v"(X[1].lo), "v"(X[2].hi), "v"(X[2].lo), "v"(X[3].hi),
        "v"(X[3].lo));
}
template <int TO, int TI>
__device__ __forceinline__ void dw_pairs(v4f* __restrict__ acc, const STile (&Z)[TO], const STile (&X)[TI]) {
#pragma unroll
  for (int to = 0; to < TO; ++to) dw_row<TI>(acc + to * TI, Z[to], X);
}

// A lane's four bands of every band tile out of one row of d_comp / d_spectral: ``rowp`` = the row + 4q.  One 16-byte request per band
// tile with an immediate offset (rows are only 4-byte aligned when B is not a multiple of 4: dword-aligned dwordx4 is a legal global
// access) instead of four 4-byte loads with a 64-bit address each: at 128 bands the 32 scalar loads and their ~300 address
// instructions were 3.1 k cycles at the top of every 20 k-cycle tile (stamps, round 3).  Quads that straddle the end of the row (the
// last band tile when B % 4 != 0) and lanes without a sample keep the element-wise, predicated form.
struct __attribute__((packed, aligned(4))) F4u {
  float v[4];
};
template <int TBMAX>
__device__ __forceinline__ void band_row_load(float (&dall)[TBMAX][4], const float* __restrict__ rowp, bool live, int q, int TB, int B) {
#pragma unroll
  for (int t = 0; t < TBMAX; ++t) {
    const int b0 = 16 * t + 4 * q;
    if (live && t < TB && b0 + 3 < B) {
      const F4u v = *reinterpret_cast<const F4u*>(rowp + 16 * t);
#pragma unroll
      for (int r = 0; r < 4; ++r) dall[t][r] = v.v[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) dall[t][r] = (live && t < TB && b0 + r < B) ? rowp[16 * t + r] : 0.0f;
    }
  }
}

// In-kernel phase stamps of the transpose-free backward (tools/stamp_fbwd.py builds the field sources as one unit with -DUMHS_TF_STAMP
// into its own library): s_memtime at the phase boundaries of every tile, pinned by scheduling barriers, summed per phase by wave 0 of
// workgroup 0.
#ifdef UMHS_TF_STAMP
__device__ unsigned long long g_tf_stamp[2][24];
#define TF_STAMP(k_)                                  \
  do {                                                \
    __builtin_amdgcn_sched_barrier(0);                \
    stamp_[k_] = __builtin_readcyclecounter();        \
    __builtin_amdgcn_sched_barrier(0);                \
  } while (0)
extern "C" int umhs_debug_tf_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tf_stamp), sizeof(unsigned long long) * 48);
}
extern "C" int umhs_debug_tf_stamps_clear() {
  unsigned long long z[48] = {};
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_tf_stamp), z, sizeof(z));
}
#else
#define TF_STAMP(k_) \
  do {               \
  } while (0)
#endif

// The chain (forward recompute + dX) runs on the fp32 MFMA here (v_mfma_f32_16x16x4_f32: UMHS_BWD_TF=1, and the shapes whose bf16x3
// kernels do not hold their registers); the three-piece bf16 form of the chain lives in umhs_field_zip.h.
// (Two waves per SIMD for the part-0 kernel without specular head and with the per-ray mixing -- its accumulators alone would fit --
// was tried: 128 + 128 registers, 103 spilled, 654 vs 485 us at 141 bands.)
template <int PART, bool SPEC, int TBMAX, bool FUSED = false>
__global__ __launch_bounds__(256, 1) void field_bwd_tf_kernel(FieldIO io, PackDesc pd, TPackDesc td, const float* __restrict__ image,
                                                              const float* __restrict__ wT_image, ImgSegs seg_f, ImgSegs seg_t,
                                                              int wt_off, const float* __restrict__ bf_image, ImgSegs seg_b, int bf_off,
                                                              BfOffs bo, float* __restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  typedef TfSlots<TBMAX> SL;
#ifdef UMHS_TF_STAMP
  const unsigned long long k_t0 = __builtin_readcyclecounter();
#endif
  copy_segs(lds, image, seg_f);  // pd / td carry offsets local to this part's LDS image
#ifdef UMHS_TF_STAMP
  __builtin_amdgcn_s_waitcnt(0);
  const unsigned long long k_ta = __builtin_readcyclecounter();
#endif
  copy_segs(lds + wt_off, wT_image, seg_t);
#ifdef UMHS_TF_STAMP
  __builtin_amdgcn_s_waitcnt(0);
  const unsigned long long k_tb = __builtin_readcyclecounter();
#endif
#ifdef UMHS_TF_STAMP
  __builtin_amdgcn_s_waitcnt(0);
  const unsigned long long k_tc = __builtin_readcyclecounter();
#endif
  __syncthreads();
#ifdef UMHS_TF_STAMP
  const unsigned long long k_td = __builtin_readcyclecounter();
  if (blockIdx.x == 0 && threadIdx.x == 0)
    g_tf_stamp[PART][16] = k_ta - k_t0, g_tf_stamp[PART][17] = k_tb - k_ta, g_tf_stamp[PART][19] = k_tc - k_tb, g_tf_stamp[PART][23] = k_td - k_tc;
#endif
  const float* const wT = lds + wt_off;
#define TF_GEMM_F(OT_, KS_, INIT_, ACC_, B_, LID_) gemm_pack<OT_, KS_, NT, INIT_>(ACC_, B_, lds + pd.L[LID_].off_w, lds + pd.L[LID_].off_b, lane)
#define TF_GEMM_T(OT_, KS_, INIT_, ACC_, B_, TID_) gemm_pack<OT_, KS_, NT, INIT_>(ACC_, B_, wT + td.L[TID_].off, nullptr, lane)
  constexpr int NT = 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const v4s ident = ident_frag(lane);
  constexpr int A0 = SL::acc0(PART), NA = SL::acc1(PART) - A0, DB0 = 4 * SL::dbv0(PART), NDBP = 4 * (SL::dbv1(PART) - SL::dbv0(PART));
  v4f acc_[NA];
  float db_[NDBP];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc_[i] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < NDBP; ++i) db_[i] = 0.0f;
  // acc_ / db_ are indexed with the absolute slots of TfSlots minus this part's first slot (compile-time indices only)
  const int C = io.C, B = io.B, TB = io.TB;
  const int64_t ntiles = (io.n + 63) / 64;
  // One wave per SIMD: nothing else hides a global load, so every per-sample input of a tile is requested one tile ahead.
  struct TileIn {
    float w[3], d[3];
    float2 e[PART == 1 ? 4 : 1];
    v4f x0, x1;  // part 0: saved feature logits, -;  part 1: d_fl, d_bo (from part 0)
    float emb[4], dsig, sel, demb[4];
    float ws, tm0, tm1;  // FUSED: weights[n] (scaled by scale_n once the tile is current), the sample's interval
    int64_t ray;         // FUSED: the sample's ray
  };
  auto fetch = [&](int64_t tile, TileIn& in) {
    int64_t n = tile * 64 + wave * 16 + j;
    const bool ok = n < io.n;
    if (!ok) n = io.n - 1;
#pragma unroll
    for (int s = 0; s < 3; ++s) in.w[s] = io.wpos[3 * n + s];
    if (PART == 0) {
      if (SPEC) {
#pragma unroll
        for (int s = 0; s < 3; ++s) in.d[s] = io.dirs[3 * n + s];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 4 * q + r - 1;
        in.emb[r] = (e >= 0 && !io.bo16_in) ? io.emb_in[n * 15 + e] : 0.0f;  // slot 0 (sigma_raw) meets a zero weight column
      }
      if (io.bo16_in) {  // the aligned-row form of the saved base outputs (one 16-byte load)
        const v4f b4 = *reinterpret_cast<const v4f*>(io.bo16_in + n * 16 + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) in.emb[r] = (q == 0 && r == 0) ? 0.0f : b4[r];
      }
      in.x0 = *reinterpret_cast<const v4f*>(io.feat_logits_in + n * 16 + 4 * q);
      if (FUSED) {  // raw loads only: arithmetic on a prefetched value would make the wave wait for it here, a tile too early
        in.ws = io.weights[n];
        in.tm0 = io.t0 ? io.t0[n] : 1.0f, in.tm1 = io.t0 ? io.t1[n] : 1.0f;  // (t_mid = 1: scale 1)
        in.ray = io.ray_of[n];
      }
    } else {
#pragma unroll
      for (int lv = 0; lv < 4; ++lv) in.e[lv] = *reinterpret_cast<const float2*>(io.enc + n * io.sn + (int64_t)(4 * q + lv) * io.sl);
      const v4f z = {0.0f, 0.0f, 0.0f, 0.0f};
      // rows past the end carry zero upstream gradients: every dZ of theirs is then zero
      in.x0 = ok ? *reinterpret_cast<const v4f*>(io.d_fl + n * 16 + 4 * q) : z;
      in.x1 = ok ? *reinterpret_cast<const v4f*>(io.d_bo + n * 16 + 4 * q) : z;
      in.sel = io.sel[n];
      in.dsig = ok ? io.d_sigma[n] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = 4 * q + r - 1;
        in.demb[r] = (io.d_emb && ok && e >= 0) ? io.d_emb[n * 15 + e] : 0.0f;
      }
    }
  };
  TileIn cur, nxt;
#ifdef UMHS_TF_STAMP
  const unsigned long long k_t1 = __builtin_readcyclecounter();
#endif
  if ((int64_t)blockIdx.x < ntiles) fetch(blockIdx.x, cur);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t n = tile * 64 + wave * 16 + j;
    const bool ok = n < io.n;
    if (!ok) n = io.n - 1;
    if (tile + gridDim.x < ntiles) fetch(tile + gridDim.x, nxt);
#ifdef UMHS_TF_STAMP
    unsigned long long stamp_[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) stamp_[k] = 0;
#endif
    TF_STAMP(0);
    v4f t4[NT][4];
    float in27[NT][7];
    float pe[3];
    pe_slots(pe, cur.w[0], cur.w[1], cur.w[2], q);
#pragma unroll
    for (int s = 0; s < 3; ++s) in27[0][s] = pe[s];
    v4f dbo4[NT][1];
    dbo4[0][0] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    // one 27->64->64->out MLP (head or feature): dW of its three layers, dX down to the base-MLP slots.  x27S: swapped
    // forms of the MLP's input; input layers keep their operand order, so a swapped tile's column c = 4q'+u is whatever lane
    // quarter q' holds in slot u (tf_col() maps it back in the slab reduce): [0] positional encoding 3q'+u (u < 3), [1] base-MLP
    // output slot c.
    auto mlp3_bwd = [&](const float(&dzo)[NT][4], const float(&a2)[NT][16], const float(&a1)[NT][16], const STile(&x27S)[2],
                        v4f* __restrict__ acc2, v4f* __restrict__ acc1, v4f* __restrict__ acc0, float* __restrict__ db2,
                        float* __restrict__ db1, float* __restrict__ db0, int t2, int t1, int t0) __attribute__((always_inline)) {
      STile zS[4], xS[4];
      STile z1[1];
      z1[0] = to_swapped<true>(dzo[0], ident, db2);
      to_swapped_n<4, false>(xS, a2[0], ident);
      dw_pairs<1, 4>(acc2, z1, xS);
      TF_STAMP(8);
      v4f g4[NT][4];
      gemm_pack<4, 4, NT, 1>(g4, dzo, wT + td.L[t2].off, nullptr, lane);
      float dz1[NT][16];
#pragma unroll
      for (int i = 0; i < 16; ++i) dz1[0][i] = a2[0][i] > 0.0f ? g4[0][i >> 2][i & 3] : 0.0f;
      TF_STAMP(9);
      to_swapped_n<4, true>(zS, dz1[0], ident, db1);
      to_swapped_n<4, false>(xS, a1[0], ident);
      TF_STAMP(10);
      dw_pairs<4, 4>(acc1, zS, xS);
      TF_STAMP(11);
      TF_GEMM_T(4, 16, 1, g4, dz1, t1);
      float dz0[NT][16];
#pragma unroll
      for (int i = 0; i < 16; ++i) dz0[0][i] = a1[0][i] > 0.0f ? g4[0][i >> 2][i & 3] : 0.0f;
      TF_STAMP(12);
      to_swapped_n<4, true>(zS, dz0[0], ident, db0);
      dw_pairs<4, 2>(acc0, zS, x27S);
      TF_STAMP(13);
      TF_GEMM_T(1, 16, 0, dbo4, dz0, t0);
      TF_STAMP(14);
    };
    if constexpr (PART == 0) {
      // This tile's upstream gradients, all band tiles: requested here, consumed after the head MLP's forward recompute (with one
      // wave per SIMD a load issued next to its use costs its whole latency: one band tile ahead was 585 us at 128 bands)
      float dall[TBMAX][4];  // FUSED: the ray's d_comp row (unscaled; [R,B] stays in L2), else this sample's d_spectral row
      band_row_load<TBMAX>(dall, FUSED ? io.d_comp + cur.ray * B + 4 * q : io.d_spectral + n * B + 4 * q,
                           FUSED ? (SPEC && ok) : ok, q, TB, B);  // (FUSED: only the specular tail needs the row)
      // FUSED: G[ray][4q .. 4q+3], requested here with the ray index the previous tile's prefetch brought (a load that depends on
      // another load inside the prefetch stalls the wave for a whole memory latency per tile: +14 us at C2) and consumed after the band loop
      v4f g4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if (FUSED) {
        g4 = *reinterpret_cast<const v4f*>(io.mix_g + cur.ray * 16 + 4 * q);
        const float tm = (cur.tm0 + cur.tm1) / 2.0f;  // scale_gradients_by_distance_squared: clamp(t_mid^2, 0, 1)
        cur.ws = ok ? cur.ws * fminf(fmaxf(tm * tm, 0.0f), 1.0f) : 0.0f;
      }
      float dotacc = 0.0f;
      // =================== forward recompute: head MLP, directional hidden layer (feature logits come from the forward) ===
#pragma unroll
      for (int r = 0; r < 4; ++r) in27[0][3 + r] = cur.emb[r];
      float dir28[NT][7];
      if (SPEC) {
        float sh[4];
        sh_slots(sh, cur.d[0], cur.d[1], cur.d[2], q);
#pragma unroll
        for (int s = 0; s < 4; ++s) dir28[0][s] = sh[s];
#pragma unroll
        for (int s = 0; s < 3; ++s) dir28[0][4 + s] = pe[s];
      }
      float a1h[NT][16], a2h[NT][16];
      v4f hd4[NT][1], fl4[NT][1];
      TF_GEMM_F(4, 7, 2, t4, in27, L_H0);
      relu_to<4, NT>(a1h, t4);
      TF_GEMM_F(4, 16, 2, t4, a1h, L_H1);
      relu_to<4, NT>(a2h, t4);
      TF_GEMM_F(1, 16, 2, hd4, a2h, L_H2);
      TF_STAMP(1);
      fl4[0][0] = cur.x0;
      HeadState<NT> hs;
      head_epilogue<NT, SPEC>(hs, hd4, fl4, C, io.temperature, lane);
      float hdir[NT][4];
      if (SPEC) {
        v4f d4[NT][1];
        TF_GEMM_F(1, 7, 2, d4, dir28, L_D0);
        relu_to<1, NT>(hdir, d4);
      }
      STile x27S[2], dirS[2], hdirS[1], mS[1];  // dirS[0]: SH c, dirS[1]: the positional encoding again
      {
        const float pe4[4] = {pe[0], pe[1], pe[2], 0.0f};
        x27S[0] = to_swapped<false>(pe4, ident);
        x27S[1] = to_swapped<false>(&in27[0][3], ident);
        mS[0] = to_swapped<false>(hs.m[0], ident);
        if (SPEC) {
          dirS[0] = to_swapped<false>(&dir28[0][0], ident);
          dirS[1] = x27S[0];
          hdirS[0] = to_swapped<false>(hdir[0], ident);
        }
      }
      TF_STAMP(2);
      // =================== band tiles: mixing and the specular tail (the next tile's gradients are requested a tile ahead) ===
      // (two accumulators each for d m and d hdir, even / odd band tiles: consecutive tiles do not wait for each other's MFMAs)
      v4f dm4[NT][1], dhd4[NT][1], dm4b[NT][1], dhd4b[NT][1];
      dm4[0][0] = dhd4[0][0] = dm4b[0][0] = dhd4b[0][0] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
      float ds1 = 0.0f;
#pragma unroll
      for (int t = 0; t < TBMAX; ++t) {
        if (t < TB) {
          float dsp[NT][4];
#pragma unroll
          for (int r = 0; r < 4; ++r) dsp[0][r] = FUSED ? cur.ws * dall[t][r] : dall[t][r];
          if (!FUSED) {
            // (FUSED: d_spectral[n] = ws_n d_comp[ray(n)] is one vector per RAY times a scalar per sample, and the mixing term is
            // linear -- d m_n = ws_n (d_comp E^T)[ray] and dE = sum_rays (sum_n ws_n m_n)^T d_comp[ray] are formed per ray by
            // field_mix_grad_kernel / field_mix_dE_kernel, nothing of the mixing term is left per sample and band tile)
            gemm_pack<1, 4, NT, 0>((t & 1) ? dm4b : dm4, dsp, wT + td.L[T_MX].off + t * 256, nullptr, lane);
            STile dspS[1];
            dspS[0] = to_swapped<false>(dsp[0], ident);
            dw_pairs<1, 1>(&acc_[SL::A_MX - A0 + t], dspS, mS);  // dE^T[b][c] += sum_n d_spectral[n][b] m[n][c]
          }
          if (SPEC) {
            v4f sc[NT][1];
            gemm_pack<1, 4, NT, 2>(sc, hdir, lds + pd.L[L_D1].off_w + t * 256, lds + pd.L[L_D1].off_b + 16 * t, lane);
            float dzd[NT][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float sp = sigmoidf_(sc[0][0][r]);
              if (FUSED) dotacc += dall[t][r] * (hs.s1[0] * sp);
              ds1 += dsp[0][r] * sp;
              dzd[0][r] = dsp[0][r] * hs.s1[0] * sp * (1.0f - sp);
            }
            gemm_pack<1, 4, NT, 0>((t & 1) ? dhd4b : dhd4, dzd, wT + td.L[T_D1].off + t * 256, nullptr, lane);
            STile dzdS[1];
            dzdS[0] = to_swapped<true>(dzd[0], ident, &db_[SL::D_D1 - DB0 + t]);
            dw_pairs<1, 1>(&acc_[SL::A_D1 - A0 + t], dzdS, hdirS);
          }
        }
      }
      TF_STAMP(3);
      dm4[0][0] += dm4b[0][0], dhd4[0][0] += dhd4b[0][0];
      if (FUSED) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dotacc += hs.m[0][r] * g4[r];  // classes 4q+r (m is zero from class C on)
        dotacc = xq_sum(dotacc);
        if (ok && q == 0) io.dots[n] = dotacc;
#pragma unroll
        for (int r = 0; r < 4; ++r) dm4[0][0][r] = cur.ws * g4[r];
        // per-ray sums of ws_n m_n for dE: this 16-sample tile's share of its first / last ray, rays strictly inside written directly
        const int rayj = (int)cur.ray;
        const int rf = __builtin_amdgcn_readlane(rayj, 0), rl = __builtin_amdgcn_readlane(rayj, 15);
        const int64_t g = tile * 4 + wave;
        auto row_sum = [&](int ray, float(&out)[4]) __attribute__((always_inline)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            out[r] = row_sum16((rayj == ray) ? cur.ws * hs.m[0][r] : 0.0f);
          }
        };
        if (tile * 64 + wave * 16 < io.n) {
          float a[4];
          row_sum(rf, a);
          if (j == 0) *reinterpret_cast<v4f*>(io.part_ms + (g * 2 + 0) * 16 + 4 * q) = v4f{a[0], a[1], a[2], a[3]};
          if (rl != rf) {
            row_sum(rl, a);
            if (j == 0) *reinterpret_cast<v4f*>(io.part_ms + (g * 2 + 1) * 16 + 4 * q) = v4f{a[0], a[1], a[2], a[3]};
            for (int m = rf + 1; m < rl; ++m) {
              row_sum(m, a);
              if (j == 0) *reinterpret_cast<v4f*>(io.mws16 + (int64_t)m * 16 + 4 * q) = v4f{a[0], a[1], a[2], a[3]};
            }
          }
        }
      }
      ds1 = xq_sum(ds1);
      // =================== head outputs: sigmoid scalars, temperature softmax, specular gate ==========================
      float dhs[NT][4], dfl[NT][4];
      {
        const float inv_t = 1.0f / io.temperature;
        float da[4], dot = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float dmr = dm4[0][0][r];
          const float dsg = dmr * hs.ab[0][r];
          dhs[0][r] = dsg * hs.sg[0][r] * (1.0f - hs.sg[0][r]);
          da[r] = (4 * q + r < C) ? dmr * hs.sg[0][r] : 0.0f;
          dot += hs.ab[0][r] * da[r];
        }
        dot = xq_sum(dot);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 4 * q + r;
          float g = (c < C) ? hs.ab[0][r] * (da[r] - dot) * inv_t : 0.0f;
          if (SPEC && c == C) g = ds1 * hs.s1[0] * (1.0f - hs.s1[0]);
          dfl[0][r] = g;
          if (c >= C) dhs[0][r] = 0.0f;
        }
      }
      if (ok) *reinterpret_cast<v4f*>(io.d_fl + n * 16 + 4 * q) = v4f{dfl[0][0], dfl[0][1], dfl[0][2], dfl[0][3]};
      if (SPEC) {  // mlp_directional hidden layer
        float dz[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) dz[r] = hdir[0][r] > 0.0f ? dhd4[0][0][r] : 0.0f;
        STile dzS[1];
        dzS[0] = to_swapped<true>(dz, ident, &db_[SL::D_D0 - DB0]);
        dw_pairs<1, 2>(&acc_[SL::A_D0 - A0], dzS, dirS);
      }
      TF_STAMP(7);
      mlp3_bwd(dhs, a2h, a1h, x27S, &acc_[SL::A_H2 - A0], &acc_[SL::A_H1 - A0], &acc_[SL::A_H0 - A0], &db_[SL::D_H2 - DB0], &db_[SL::D_H1 - DB0], &db_[SL::D_H0 - DB0], T_H2,
               T_H1, T_H0);
      if (ok) *reinterpret_cast<v4f*>(io.d_bo + n * 16 + 4 * q) = dbo4[0][0];
    } else {
      // =================== forward recompute: mlp_base (its outputs are the feature MLP's inputs), feature MLP's hidden layers ===
      float encf[NT][8];
#pragma unroll
      for (int lv = 0; lv < 4; ++lv) encf[0][2 * lv] = cur.e[lv].x, encf[0][2 * lv + 1] = cur.e[lv].y;
      float h[NT][16];
      TF_GEMM_F(4, 8, 2, t4, encf, L_B0);
      relu_to<4, NT>(h, t4);
      v4f bo4[NT][1];
      TF_GEMM_F(1, 16, 2, bo4, h, L_B1);
#pragma unroll
      for (int r = 0; r < 4; ++r) in27[0][3 + r] = bo4[0][0][r];  // slot 0 (sigma_raw) meets a zero weight column
      TF_STAMP(1);
      float a1f[NT][16], a2f[NT][16];
      TF_GEMM_F(4, 7, 2, t4, in27, L_F0);
      relu_to<4, NT>(a1f, t4);
      TF_GEMM_F(4, 16, 2, t4, a1f, L_F1);
      relu_to<4, NT>(a2f, t4);
      TF_STAMP(2);
      STile x27S[2];
      {
        const float pe4[4] = {pe[0], pe[1], pe[2], 0.0f};
        x27S[0] = to_swapped<false>(pe4, ident);
        x27S[1] = to_swapped<false>(&in27[0][3], ident);
      }
      float dfl[NT][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) dfl[0][r] = cur.x0[r];
      TF_STAMP(7);
      mlp3_bwd(dfl, a2f, a1f, x27S, &acc_[SL::A_F2 - A0], &acc_[SL::A_F1 - A0], &acc_[SL::A_F0 - A0], &db_[SL::D_F2 - DB0], &db_[SL::D_F1 - DB0], &db_[SL::D_F0 - DB0], T_F2,
               T_F1, T_F0);
      // =================== mlp_base ======================================================================================
      float dzb1[NT][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) dzb1[0][r] = ok ? (dbo4[0][0][r] + cur.x1[r]) + cur.demb[r] : 0.0f;
      if (q == 0) {  // slot 0: d sigma_raw = d sigma * selector * exp(clamp(raw, -15, 15))   (trunc_exp backward)
        dzb1[0][0] = cur.dsig * cur.sel * expf(fminf(fmaxf(bo4[0][0][0], -15.0f), 15.0f));
      }
      {
        STile z1[1], hS[4];
        z1[0] = to_swapped<true>(dzb1[0], ident, &db_[SL::D_B1 - DB0]);
        to_swapped_n<4, false>(hS, h[0], ident);
        dw_pairs<1, 4>(&acc_[SL::A_B1 - A0], z1, hS);
      }
      TF_STAMP(15);
      v4f g4[NT][4];
      gemm_pack<4, 4, NT, 1>(g4, dzb1, wT + td.L[T_B1].off, nullptr, lane);
      float dzb0[NT][16];
#pragma unroll
      for (int i = 0; i < 16; ++i) dzb0[0][i] = h[0][i] > 0.0f ? g4[0][i >> 2][i & 3] : 0.0f;
      {
        STile zS[4], eS[2];
        to_swapped_n<4, true>(zS, dzb0[0], ident, &db_[SL::D_B0 - DB0]);
        to_swapped_n<2, false>(eS, encf[0], ident);  // column c = 4q'+u <-> hash feature 8q'+u ([0]) / 8q'+4+u ([1])
        dw_pairs<4, 2>(&acc_[SL::A_B0 - A0], zS, eS);
      }
      TF_STAMP(16);
      v4f de4[NT][2];
      TF_GEMM_T(2, 16, 1, de4, dzb0, T_B0);
      TF_STAMP(17);
      if (ok && io.d_enc) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const int lv = 8 * t + 2 * q + rr;  // feature e = 16t+4q+r -> level e>>1, component e&1
            *reinterpret_cast<float2*>(io.d_enc + n * io.sn + (int64_t)lv * io.sl) = make_float2(de4[0][t][2 * rr], de4[0][t][2 * rr + 1]);
          }
      }
    }
    TF_STAMP(18);
#ifdef UMHS_TF_STAMP
    if (blockIdx.x == 0 && tid == 0) {
      unsigned long long last = stamp_[0];
      for (int k = 1; k < 19; ++k)
        if (stamp_[k]) g_tf_stamp[PART][k] += stamp_[k] - last, last = stamp_[k];
      g_tf_stamp[PART][0] += 1;
    }
#endif
    cur = nxt;
  }
  // =================== sum the four waves' accumulators through LDS (the pack images are dead), one slab per workgroup ======
#ifdef UMHS_TF_STAMP
  const unsigned long long k_t2 = __builtin_readcyclecounter();
#endif
  float* const slab = slabs + (size_t)blockIdx.x * (SL::NITEMS * 256);
  constexpr int NMINE = NA + NDBP / 4;  // this part's items: its accumulators, then its bias-sum quadruples
#pragma unroll
  for (int c0 = 0; c0 < NMINE; c0 += TF_CHUNK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TF_CHUNK; ++i) {
      const int it = c0 + i;
      if (it < NMINE) {
        v4f v;
        if (it < NA) {
          v = acc_[it < NA ? it : 0];
        } else {
          const int k = it < NA ? 0 : 4 * (it - NA);
          v = v4f{db_[k], db_[k + 1], db_[k + 2], db_[k + 3]};
        }
        *reinterpret_cast<v4f*>(lds + ((wave * TF_CHUNK + i) * 64 + lane) * 4) = v;
      }
    }
    __syncthreads();
    const int nit = NMINE - c0 < TF_CHUNK ? NMINE - c0 : TF_CHUNK;
    for (int e = tid; e < nit * 64; e += 256) {
      v4f s = *reinterpret_cast<const v4f*>(lds + e * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) s += *reinterpret_cast<const v4f*>(lds + (w * TF_CHUNK * 64 + e) * 4);
      const int it = c0 + (e >> 6);  // this part's item -> absolute slab item
      const int abs_item = it < NA ? A0 + it : SL::NACC + SL::dbv0(PART) + (it - NA);
      *reinterpret_cast<v4f*>(slab + (abs_item * 64 + (e & 63)) * 4) = s;
    }
  }
#ifdef UMHS_TF_STAMP
  if (blockIdx.x == 0 && tid == 0) {
    const unsigned long long k_t3 = __builtin_readcyclecounter();
    g_tf_stamp[PART][20] += k_t1 - k_t0, g_tf_stamp[PART][21] += k_t2 - k_t1, g_tf_stamp[PART][22] += k_t3 - k_t2;
  }
#endif
}
#undef TF_GEMM_F
#undef TF_GEMM_T

#include "umhs_field_zip.h"

// ---- launchers: one kernel instance = raise its LDS limit (once), launch it on the part's LDS image ------------------------------------------
#define TF_ARGS_ a.io, pt.pd, pt.td, a.img, a.wT, pt.seg_f, pt.seg_t, pt.wt_off, a.bfimg, pt.seg_b, pt.bf_off, pt.bo, a.slabs
#define LAUNCH_K_(...)                                                                                          \
  do {                                                                                                          \
    int rc_ = set_lds(__VA_ARGS__, pt.lds);                                                                     \
    if (rc_) return rc_;                                                                                        \
    hipLaunchKernelGGL((__VA_ARGS__), dim3(a.grid), dim3(256), pt.lds, umhs_s(a.stream), TF_ARGS_);             \
    return UMHS_OK;                                                                                             \
  } while (0)
#define INSTANTIATE_(fn_, ...)         \
  template int fn_<2>(__VA_ARGS__);    \
  template int fn_<4>(__VA_ARGS__);    \
  template int fn_<8>(__VA_ARGS__);    \
  template int fn_<12>(__VA_ARGS__);   \
  template int fn_<16>(__VA_ARGS__)
// (instantiated: what run_field_bwd can select -- the zipped part 0 with the specular head up to 4 band tiles, 8 in the folded form
// only; the fp32 chain with it up to 12)
