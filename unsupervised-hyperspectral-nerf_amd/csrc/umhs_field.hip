// Fused per-sample UMHS field for gfx950: the forward kernel, the pack-image kernel, the small kernels of the backward (mixing term
// per ray, slab fold / reduce, zero gradients, heads finish) and the whole host side of the field's C ABI.  The GEMM chain both
// directions share is umhs_field_chain.h; the two main backward kernels live in umhs_field_bwd.h / umhs_field_zip.h and compile in
// translation units of their own (umhs_field_bwd_p0z.hip, _p0f.hip, _p1.hip), reached here through the launchers declared in
// umhs_field_launch.h.
#include <cstdlib>

#include "umhs_field_launch.h"

// =============================================================================================
// Forward
// =============================================================================================
// BF: the layers with >= 7 k-steps (everything but the band tiles and the directional hidden layer) run as three-piece bf16
// products (gemm_bf): 6 v_mfma_f32_16x16x32_bf16 per 8 k-slots instead of 8 v_mfma_f32_16x16x4_f32 at twice the cycles each.  Their
// bf16x3 packs (1.5x the fp32 bytes) make the image ~110 KB: one 8-wave workgroup per CU instead of two 4-wave ones.
struct FwdBfArgs {
  ImgSegs seg_f, seg_b;  // fp32 part (packs of the other layers + every bias) and bf16x3 part of the LDS image
  int bf_off;            // dword offset of the bf16x3 part in LDS
  BfOffs bo;
  const float* bf_image;
};
// HEADS: the kernel starts from the base MLP's saved outputs (emb) instead of the hash features -- the density half ran as its own
// launch, so the rendering weights of every sample are known -- and forms the per-ray band sums of its outputs itself (HeadsComp
// below): the [N,B] streams that carry no loss (spectral2, specular) are never written, the third only if the caller wants it.
//
// Per-ray sums without atomics, same bits every run: a wave's 16-sample tile g = n/16 covers at most a tail of one ray, whole rays,
// and a head of another.  It stores  A[g][stream][b] = sum over the samples of the tile's FIRST sample's ray,
// Z[g][stream][b] = the same for its LAST sample's ray (when that is another ray), and writes rays that lie strictly inside the
// tile straight to comp (no other tile contributes to them).  field_heads_finish_kernel then adds, for every other ray, the A / Z
// entries of its tiles in tile order.  part[((g*2 + az)*n_streams + stream)*16*TB + b].
template <bool SPEC, bool DENSITY_ONLY, int NT, int WAVES, bool BF = false, bool HEADS = false>
__global__ __launch_bounds__(64 * WAVES, BF ? WAVES / 4 : (2 * WAVES) / 4) void field_fwd_kernel(FieldIO io, PackDesc pd,
                                                                                        const float* __restrict__ image, FwdBfArgs fb) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (BF) {
    copy_segs(lds, image, fb.seg_f);  // pd carries offsets local to this compact image
    copy_segs(lds + fb.bf_off, fb.bf_image, fb.seg_b);
  } else {
    load_fwd_image(lds, pd, image, 0);
  }
  __syncthreads();
  const uint32_t* const wbf = reinterpret_cast<const uint32_t*>(lds + fb.bf_off);
#define FWD_GEMM(OT_, KS_, ACC_, B_, LID_)                                                                     \
  do {                                                                                                          \
    if constexpr (BF)                                                                                           \
      gemm_bf<OT_, KS_, NT, 2>(ACC_, B_, wbf + fb.bo.f[LID_], lds + pd.L[LID_].off_b, lane);                    \
    else                                                                                                        \
      gemm_pack<OT_, KS_, NT, 2>(ACC_, B_, lds + pd.L[LID_].off_w, lds + pd.L[LID_].off_b, lane);               \
  } while (0)
  constexpr int TILE = 16 * NT * WAVES;  // samples per workgroup iteration
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int64_t ntiles = (io.n + TILE - 1) / TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t nn[NT];
    bool ok[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      int64_t n = tile * TILE + wave * (16 * NT) + ct * 16 + j;
      ok[ct] = n < io.n;
      nn[ct] = ok[ct] ? n : io.n - 1;
    }
    float encf[NT][8];
    if (HEADS) {
      // nothing to load here: the base MLP's outputs are read below
    } else {
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int lv = 0; lv < 4; ++lv) {
          const float2 v = *reinterpret_cast<const float2*>(io.enc + nn[ct] * io.sn + (int64_t)(4 * q + lv) * io.sl);
          encf[ct][2 * lv] = v.x, encf[ct][2 * lv + 1] = v.y;
        }
    }
    // ---- encodings first (sinf's slow path and the loads branch; keep them out of the gemm chain) --------
    float pe_[NT][3], sh_[NT][4];
    if (!DENSITY_ONLY) {
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        pe_slots(pe_[ct], io.wpos[3 * nn[ct]], io.wpos[3 * nn[ct] + 1], io.wpos[3 * nn[ct] + 2], q);
        if (SPEC) sh_slots(sh_[ct], io.dirs[3 * nn[ct]], io.dirs[3 * nn[ct] + 1], io.dirs[3 * nn[ct] + 2], q);
      }
    }
    // ---- mlp_base: 32 -> 64 -> 16 -------------------------------------------------------------
    v4f bo4[NT][1];
    if constexpr (HEADS) {
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = 4 * q + r - 1;
          bo4[ct][0][r] = (e >= 0 && !io.bo16_in) ? io.emb_in[nn[ct] * 15 + e] : 0.0f;  // slot 0 (sigma_raw) meets a zero weight column
        }
      if (io.bo16_in) {
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          bo4[ct][0] = *reinterpret_cast<const v4f*>(io.bo16_in + nn[ct] * 16 + 4 * q);
          if (q == 0) bo4[ct][0][0] = 0.0f;
        }
      }
    } else {
      v4f h4[NT][4];
      FWD_GEMM(4, 8, h4, encf, L_B0);
      float h[NT][16];
      relu_to<4, NT>(h, h4);
      FWD_GEMM(1, 16, bo4, h, L_B1);
    }
    if (DENSITY_ONLY) {
      store_density<NT>(io, bo4, nn, ok, q);
      continue;
    }
    float in27[NT][7], dir28[NT][7];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
#pragma unroll
      for (int s = 0; s < 3; ++s) in27[ct][s] = pe_[ct][s];
#pragma unroll
      for (int r = 0; r < 4; ++r) in27[ct][3 + r] = bo4[ct][0][r];
      if (SPEC) {
#pragma unroll
        for (int s = 0; s < 4; ++s) dir28[ct][s] = sh_[ct][s];
#pragma unroll
        for (int s = 0; s < 3; ++s) dir28[ct][4 + s] = pe_[ct][s];
      }
    }
    // ---- mlp_head / feature_mlp: 27 -> 64 -> 64 -> C(+1) ----------------------------------------
    v4f t4[NT][4], hd4[NT][1], fl4[NT][1];
    float a1[NT][16], a2[NT][16];
    FWD_GEMM(4, 7, t4, in27, L_H0);
    relu_to<4, NT>(a1, t4);
    FWD_GEMM(4, 16, t4, a1, L_H1);
    relu_to<4, NT>(a2, t4);
    FWD_GEMM(1, 16, hd4, a2, L_H2);
    FWD_GEMM(4, 7, t4, in27, L_F0);
    relu_to<4, NT>(a1, t4);
    FWD_GEMM(4, 16, t4, a1, L_F1);
    relu_to<4, NT>(a2, t4);
    FWD_GEMM(1, 16, fl4, a2, L_F2);
    if (io.feat_logits) {  // saved for the split backward: [N,16] rows 4q..4q+3 of the logit tile, 64 B per sample
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
        if (ok[ct]) *reinterpret_cast<v4f*>(io.feat_logits + nn[ct] * 16 + 4 * q) = fl4[ct][0];
    }
    HeadState<NT> hs;
    head_epilogue<NT, SPEC>(hs, hd4, fl4, io.C, io.temperature, lane);
    // ---- mlp_directional hidden: 28 -> 16 ---------------------------------------------------------
    float hdir[NT][4];
    if (SPEC) {
      v4f d4[NT][1];
      gemm_pack<1, 7, NT, 2>(d4, dir28, lds + pd.L[L_D0].off_w, lds + pd.L[L_D0].off_b, lane);
      relu_to<1, NT>(hdir, d4);
    }
    // ---- per 16-band tile: mixing (K = classes) and specular (K = 16 hidden) -------------------------
    if constexpr (!HEADS) {
#pragma unroll 1  // a runtime loop: left alone hipcc unrolls the (small) no-specular body 8x and spills 200+ registers
      for (int t = 0; t < io.TB; ++t) {
        // transposed tiles: rows = samples 4q+r of the column tile, lanes&15 = bands 16t..16t+15 -> 64-byte row segments
        v4f sp[NT][1], sc[NT][1];
        gemm_pack<1, 4, NT, 1, true>(sp, hs.m, lds + pd.L[L_MX].off_w + t * 256, nullptr, lane);
        if (SPEC) gemm_pack<1, 4, NT, 2, true>(sc, hdir, lds + pd.L[L_D1].off_w + t * 256, lds + pd.L[L_D1].off_b + 16 * t, lane);
        const int b = 16 * t + j;
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const int64_t nb = tile * TILE + wave * (16 * NT) + ct * 16 + 4 * q;  // first sample of this lane's 4 rows
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float s1r = SPEC ? __shfl(hs.s1[ct], 4 * q + r, 64) : 0.0f;  // s1 lives on lane&15 = sample
            if (nb + r < io.n && b < io.B) {
              const float spec = sp[ct][0][r];
              const float spl = SPEC ? s1r * sigmoidf_(sc[ct][0][r]) : 0.0f;
              const int64_t o = (nb + r) * io.B + b;
              io.spectral[o] = SPEC ? spec + spl : spec;
              if (SPEC && io.spectral2) io.spectral2[o] = spec;
              if (SPEC && io.specular) io.specular[o] = spl;
            }
          }
        }
      }
      // ---- per-sample scalars last (conditional stores = branches) -----------------------------------
      store_density<NT>(io, bo4, nn, ok, q);
    }
    if (io.abund) {
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ok[ct] && 4 * q + r < io.C) io.abund[nn[ct] * io.C + 4 * q + r] = hs.ab[ct][r];
    }
    if constexpr (HEADS) {
      // Per-ray sums inside the kernel.  The mixing term is linear in m: sum_n w_n (m_n E) = (sum_n w_n m_n) E, so the kernel sums
      // w_n m_n (16 classes) per ray and the finish pass multiplies by E once per RAY -- no mixing product per sample and band tile at
      // all; only the specular term (a sigmoid per sample and band) is formed per band tile.  Abundances are a third 16-wide stream.
      float w4[NT][4], wj[NT];
      int r4[NT][4], rj[NT], rfirst[NT], rlast[NT];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int64_t nb0 = tile * TILE + wave * (16 * NT) + ct * 16;  // first sample of the tile
        const int64_t last = nb0 + 15 < io.n ? nb0 + 15 : io.n - 1;
        rfirst[ct] = nb0 < io.n ? __builtin_amdgcn_readfirstlane((int)io.ray_of[nb0]) : -1;
        rlast[ct] = nb0 < io.n ? __builtin_amdgcn_readfirstlane((int)io.ray_of[last]) : -1;
        const bool vj = nb0 + j < io.n;
        wj[ct] = vj ? io.weights[nb0 + j] : 0.0f;  // this lane's sample (samples-on-lanes tiles) ...
        rj[ct] = vj ? (int)io.ray_of[nb0 + j] : -2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // ... and the four rows 4q..4q+3 it holds of a transposed band tile
          w4[ct][r] = __shfl(wj[ct], 4 * q + r, 64);
          r4[ct][r] = __shfl(rj[ct], 4 * q + r, 64);
        }
      }
      if (SPEC) {
#pragma unroll 1
        for (int t = 0; t < io.TB; ++t) {
          v4f sc[NT][1];
          gemm_pack<1, 4, NT, 2, true>(sc, hdir, lds + pd.L[L_D1].off_w + t * 256, lds + pd.L[L_D1].off_b + 16 * t, lane);
          const int b = 16 * t + j, BP = 16 * io.TB;
#pragma unroll
          for (int ct = 0; ct < NT; ++ct) {
            if (rfirst[ct] < 0) continue;
            const int64_t g = (tile * TILE + wave * (16 * NT) + ct * 16) >> 4;
            float val[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) val[r] = w4[ct][r] * (__shfl(hs.s1[ct], 4 * q + r, 64) * sigmoidf_(sc[ct][0][r]));
            auto col_sum = [&](int ray) __attribute__((always_inline)) {
              float a = 0.0f;
#pragma unroll
              for (int r = 0; r < 4; ++r) a += (r4[ct][r] == ray) ? val[r] : 0.0f;
              return xq_sum(a);
            };
            const float a = col_sum(rfirst[ct]);
            if (q == 0) io.part[(g * 2 + 0) * BP + b] = a;
            if (rlast[ct] != rfirst[ct]) {  // wave-uniform
              const float z = col_sum(rlast[ct]);
              if (q == 0) io.part[(g * 2 + 1) * BP + b] = z;
              for (int m = rfirst[ct] + 1; m < rlast[ct]; ++m) {  // rays strictly inside this tile (short rays; rare)
                const float v = col_sum(m);
                if (q == 0 && b < io.B) io.comp[2][(int64_t)m * io.B + b] = v;
              }
            }
          }
        }
      }
      // the two 16-wide streams (w m and w abundances): samples on lanes (lane = (sample j, q), reg r <-> class 4q+r) -- the sum
      // over a tile's samples is a reduction over the 16 lanes of a row, masked by the sample's ray
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (rfirst[ct] < 0) continue;
        const int64_t g = (tile * TILE + wave * (16 * NT) + ct * 16) >> 4;
        auto row_sum = [&](const float(&x)[4], int ray, float(&out)[4]) __attribute__((always_inline)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            out[r] = row_sum16((rj[ct] == ray) ? wj[ct] * x[r] : 0.0f);
          }
        };
        auto stream16 = [&](const float(&x)[4], float* __restrict__ part16, float* __restrict__ direct, int width) __attribute__((always_inline)) {
          float a[4];
          row_sum(x, rfirst[ct], a);
          if (j == 0) *reinterpret_cast<v4f*>(part16 + (g * 2 + 0) * 16 + 4 * q) = v4f{a[0], a[1], a[2], a[3]};
          if (rlast[ct] != rfirst[ct]) {
            row_sum(x, rlast[ct], a);
            if (j == 0) *reinterpret_cast<v4f*>(part16 + (g * 2 + 1) * 16 + 4 * q) = v4f{a[0], a[1], a[2], a[3]};
            for (int m = rfirst[ct] + 1; m < rlast[ct]; ++m) {
              row_sum(x, m, a);
              if (j == 0 && direct) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                  if (4 * q + r < width) direct[(int64_t)m * width + 4 * q + r] = a[r];
              }
            }
          }
        };
        stream16(hs.m[ct], io.part_m, io.mix16, 16);
        if (io.part_ab) stream16(hs.ab[ct], io.part_ab, io.comp_ab, io.C);
      }
    }
  }
}
#undef FWD_GEMM

// Every weight image of one direction in ONE launch, each dword computed straight from the parameters: the fp32 forward image
// (weights + biases), the transposed image, the bf16x3 image of the converted layers.  (As three dependent launches -- fp32 images,
// then the bf16x3 image read back from them -- the packs of a step cost 26 us of small kernels; 2 x 6 us like this.)
struct PackJob {
  PackDesc pd;
  TPackDesc td;
  BfPlan bp;
  float* img;    // [pd.total] or null
  float* wT;     // [td.total] or null
  uint32_t* bf;  // [bp.total] or null
};
__global__ __launch_bounds__(256) void field_pack_all_kernel(PackJob jb) {
  const int n_img = jb.img ? jb.pd.total : 0, n_wT = jb.wT ? jb.td.total : 0, n_bf = jb.bf ? jb.bp.total : 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_img + n_wT + n_bf; i += gridDim.x * 256) {
    if (i < n_img) {
      float v = 0.0f;
      if (i < jb.pd.total_w) {
        v = fwd_pack_value(jb.pd, i);
      } else {
        int li = 0;
        while (li + 1 < NLAYERS && i >= jb.pd.L[li + 1].off_b) ++li;  // off_b is non-decreasing (L_MX has no bias tile)
        const LayerDesc& L = jb.pd.L[li];
        const int o = i - L.off_b;
        v = (li != L_MX && L.b && o < L.OUT) ? L.b[o] : 0.0f;
      }
      jb.img[i] = v;
    } else if (i < n_img + n_wT) {
      jb.wT[i - n_img] = t_pack_value(jb.td, i - n_img);
    } else {
      const int idx = i - n_img - n_wT;
      int ci = 0;
      while (ci + 1 < jb.bp.n && idx >= jb.bp.c[ci + 1].dst_off) ++ci;
      const BfConv& c = jb.bp.c[ci];
      const int rel = idx - c.dst_off;
      const int up = rel & 3, lane = (rel >> 2) & 63, blk = rel >> 8;  // blk = (t*K8 + S)*3 + piece
      const int piece = blk % 3, ts = blk / 3;
      const int K8 = (c.KS4 + 1) >> 1, t = ts / K8, S = ts % K8;
      uint32_t out = 0;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int u = 2 * up + e, s4 = 2 * S + (u >> 2);
        float w = 0.0f;
        if (s4 < c.KS4) {
          const int src = c.src_off + ((t * c.KS4 + s4) * 64 + lane) * 4 + (u & 3);
          w = c.src_img ? t_pack_value(jb.td, src) : fwd_pack_value(jb.pd, src);
        }
        uint32_t h, m, l;
        bf_split3_scalar(w, h, m, l);
        out |= (piece == 0 ? h : (piece == 1 ? m : l)) << (16 * e);
      }
      jb.bf[idx] = out;
    }
  }
}

static unsigned tf_grid(int64_t n) {
  const int64_t ntiles = (n + 63) / 64;
  return (unsigned)(ntiles < 256 ? ntiles : 256);
}

// ---- the mixing term of the folded compositing backward, per RAY (umhs_field_bwd_composited) ---------------------------------
// G[r][c] = sum_b d_comp[r][b] E[c][b]   (c < C, zero above): d m_n = ws_n G[ray(n)]
__global__ __launch_bounds__(256) void field_mix_grad_kernel(const float* __restrict__ d_comp, const float* __restrict__ E, int64_t R,
                                                            int B, int C, float* __restrict__ G) {
  // 16 rays per workgroup: the rays' gradient rows and the endmembers staged in LDS (odd row stride: the 16 class rows a wave reads
  // sit in 16 banks), thread = (ray, class)
  extern __shared__ float sm[];
  const int BS = B | 1;
  float* sE = sm;             // [16][BS]
  float* sD = sm + 16 * BS;   // [16][BS]
  const int tid = threadIdx.x;
  const int64_t ray0 = (int64_t)blockIdx.x * 16;
  for (int i = tid; i < 16 * B; i += 256) {
    const int r = i / B, b = i - r * B;
    sE[r * BS + b] = r < C ? E[(int64_t)r * B + b] : 0.0f;
    sD[r * BS + b] = ray0 + r < R ? d_comp[(ray0 + r) * B + b] : 0.0f;
  }
  __syncthreads();
  const int rr = tid >> 4, c = tid & 15;
  float a0 = 0.0f, a1 = 0.0f;
  int b = 0;
  for (; b + 1 < B; b += 2) a0 += sD[rr * BS + b] * sE[c * BS + b], a1 += sD[rr * BS + b + 1] * sE[c * BS + b + 1];
  if (b < B) a0 += sD[rr * BS + b] * sE[c * BS + b];
  if (ray0 + rr < R) G[(ray0 + rr) * 16 + c] = a0 + a1;
}
// dE[c][b] = sum_r M[r][c] d_comp[r][b] with M[r][c] = sum over the samples of ray r of ws_n m_n[c] (finished here from part 0's tile
// partials, as field_heads_finish_kernel does).  Stage 1: one workgroup per 32 rays -> partial[chunk][c][b]; stage 2 adds the chunks.
constexpr int MIX_CHUNK = 32;
__global__ __launch_bounds__(256) void field_mix_dE_kernel(const float* __restrict__ part_ms, const float* __restrict__ mws16,
                                                          const int64_t* __restrict__ ray_of, const int64_t* __restrict__ pinfo,
                                                          int64_t n, int64_t R, const float* __restrict__ d_comp, int B, int C,
                                                          float* __restrict__ partial) {
  __shared__ float sM[MIX_CHUNK][16];
  const int tid = threadIdx.x;
  const int64_t ray0 = (int64_t)blockIdx.x * MIX_CHUNK;
  {
    const int64_t ray = ray0 + (tid >> 3);
    const int c0 = 2 * (tid & 7);
    float acc[2] = {0.0f, 0.0f};
    if (ray < R) {
      const int64_t s0 = pinfo[2 * ray], cnt = pinfo[2 * ray + 1];
      if (cnt > 0) {
        const int64_t ts = s0 >> 4, te = (s0 + cnt - 1) >> 4;
        const bool first = ray_of[16 * ts] == ray;
        bool inside = false;
        if (ts == te) {
          const int64_t l = 16 * ts + 15 < n ? 16 * ts + 15 : n - 1;
          inside = !first && ray_of[l] != ray;
        }
        if (inside) {
          acc[0] = mws16[ray * 16 + c0], acc[1] = mws16[ray * 16 + c0 + 1];
        } else {
          for (int64_t t = ts; t <= te; ++t) {
            const float2 v = *reinterpret_cast<const float2*>(part_ms + (t * 2 + ((t == ts && !first) ? 1 : 0)) * 16 + c0);
            acc[0] += v.x, acc[1] += v.y;
          }
        }
      }
    }
    sM[tid >> 3][c0] = acc[0], sM[tid >> 3][c0 + 1] = acc[1];
  }
  __syncthreads();
  const int nr = (int)(R - ray0 < MIX_CHUNK ? R - ray0 : MIX_CHUNK);
  for (int i = tid; i < C * B; i += 256) {
    const int c = i / B, b = i - c * B;
    float a0 = 0.0f, a1 = 0.0f;
    int rr = 0;
    for (; rr + 1 < nr; rr += 2) {
      a0 += sM[rr][c] * d_comp[(ray0 + rr) * B + b];
      a1 += sM[rr + 1][c] * d_comp[(ray0 + rr + 1) * B + b];
    }
    if (rr < nr) a0 += sM[rr][c] * d_comp[(ray0 + rr) * B + b];
    partial[(size_t)blockIdx.x * C * B + i] = a0 + a1;
  }
}
__global__ __launch_bounds__(1024) void field_mix_dE_sum_kernel(const float* __restrict__ partial, int nchunks, int CB,
                                                               float* __restrict__ dE) {
  // 64 outputs per workgroup, 16 waves each adding a sixteenth of the chunks (in chunk order), then one fixed-order sum
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, pw = threadIdx.x >> 6, i = blockIdx.x * 64 + lane;
  const int per = (nchunks + 15) / 16, k0 = pw * per, k1 = min(nchunks, k0 + per);
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  if (i < CB) {
    int k = k0;
    for (; k + 3 < k1; k += 4) {
      a0 += partial[(size_t)k * CB + i], a1 += partial[(size_t)(k + 1) * CB + i];
      a2 += partial[(size_t)(k + 2) * CB + i], a3 += partial[(size_t)(k + 3) * CB + i];
    }
    for (; k < k1; ++k) a0 += partial[(size_t)k * CB + i];
  }
  part[pw][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (pw != 0 || i >= CB) return;
  float sacc = 0.0f;
#pragma unroll
  for (int k = 0; k < 16; k += 4) sacc += (part[k][lane] + part[k + 1][lane]) + (part[k + 2][lane] + part[k + 3][lane]);
  dE[i] = sacc;
}

struct GradPtrs {
  float* W[NLAYERS];
  float* b[NLAYERS];
};

// slab -> gradient tensors of the transpose-free kernels.  item -> (layer, to, ti); a swapped input tile's column c of layer kind
// `kind` is reference input column tf_col(kind, ti, c) (or -1: a padding slot).
struct TfMap {
  int nacc, ndb, nitems;
  short layer[128], to[128], ti[128];  // per accumulator item
  short db_layer[64], db_tile[64];     // per bias-sum tile
};
__device__ __forceinline__ int tf_col(int kind, int ti, int c) {
  const int qq = c >> 2, u = c & 3;
  switch (kind) {
    case IN_ENC: return 8 * qq + 4 * ti + u;
    case IN_27: return ti == 0 ? (u < 3 ? 3 * qq + u : -1) : (c >= 1 ? 12 + c - 1 : -1);
    case IN_DIR28: return ti == 0 ? c : (u < 3 ? 16 + 3 * qq + u : -1);
    default: return 16 * ti + c;  // IN_HID64 / IN_HID16 / IN_MIX: natural order
  }
}

// First pass of the slab reduction: workgroup (item, g) adds slabs [g * TF_FOLD, (g + 1) * TF_FOLD) of one item (64 lanes x 4 floats) in a
// fixed order and writes it as item `item` of slab g of `out`.  field_reduce_tf_kernel alone has one workgroup per item, ~76 of them: 76
// CUs pulling 19.5 MB at ~30 GB/s each took 16.7 us; folded by all 256 CUs first, the two passes take half of that.
constexpr int TF_FOLD = 16;
__global__ __launch_bounds__(256) void field_slab_fold_kernel(const float* __restrict__ slabs, int nslabs, int nitems, float* __restrict__ out) {
  __shared__ v4f part[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, item = blockIdx.x, g = blockIdx.y;
  const size_t stride = (size_t)nitems * 256, off = (size_t)item * 256 + lane * 4;
  v4f x[TF_FOLD / 4];
#pragma unroll
  for (int k = 0; k < TF_FOLD / 4; ++k) {
    const int sl = g * TF_FOLD + wv * (TF_FOLD / 4) + k;
    x[k] = sl < nslabs ? *reinterpret_cast<const v4f*>(slabs + (size_t)sl * stride + off) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
  }
  part[wv][lane] = (x[0] + x[1]) + (x[2] + x[3]);
  static_assert(TF_FOLD == 16, "four slabs per wave");
  __syncthreads();
  if (wv == 0) *reinterpret_cast<v4f*>(out + (size_t)g * stride + off) = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// 64 outputs per workgroup; its 16 waves each sum a sixteenth of the slabs (8 loads in flight), LDS combines (one thread per output
// walking all 256 slabs was 82 us at 128 bands: 90 workgroups of serial loads)
__global__ __launch_bounds__(1024) void field_reduce_tf_kernel(const float* __restrict__ slabs, int nslabs, TfMap mp, PackDesc pd,
                                                              GradPtrs gp) {
  // Workgroups [0, nacc): one accumulator item (64 lanes x 4 floats = 1 KiB per slab) each -- a wave reads the whole item of a slab
  // with one 16-byte load per lane, 16 waves take a sixteenth of the slabs each (8 loads in flight), LDS combines in a fixed order.
  // Workgroups from nacc on: 64 bias columns each (sum over the slabs and the 4 lane quarters).
  __shared__ v4f part4[16][64];
  const int lane = threadIdx.x & 63, pw = threadIdx.x >> 6;
  const size_t stride = (size_t)mp.nitems * 256;
  const int per = (nslabs + 15) / 16, w0 = pw * per, w1 = min(nslabs, w0 + per);
  if ((int)blockIdx.x < mp.nacc) {
    const int item = blockIdx.x, l = mp.layer[item];
    if (l < 0) return;  // an unused slot (workgroup-uniform)
    const size_t off = (size_t)item * 256 + lane * 4;
    v4f a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    int w = w0;
    for (; w + 7 < w1; w += 8) {
      v4f x[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = *reinterpret_cast<const v4f*>(slabs + (size_t)(w + k) * stride + off);
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k & 3] += x[k];
    }
    for (; w < w1; ++w) a[0] += *reinterpret_cast<const v4f*>(slabs + (size_t)w * stride + off);
    part4[pw][lane] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (pw != 0) return;
    v4f s4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 16; k += 4) s4 += (part4[k][lane] + part4[k + 1][lane]) + (part4[k + 2][lane] + part4[k + 3][lane]);
    const LayerDesc& L = pd.L[l];
    if (!gp.W[l]) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int out = 16 * mp.to[item] + 4 * (lane >> 4) + r;
      if (l == L_MX) {  // dE^T[b][c]
        const int cls = lane & 15;
        if (out < L.OUT && cls < L.IN) gp.W[l][(size_t)cls * L.OUT + out] = s4[r];
      } else {
        const int in = tf_col(L.kind, mp.ti[item], lane & 15);
        if (out < L.OUT && in >= 0 && in < L.IN) gp.W[l][(size_t)out * L.IN + in] = s4[r];
      }
    }
    return;
  }
  float(*part)[64] = reinterpret_cast<float(*)[64]>(&part4[0][0]);
  const int k = ((int)blockIdx.x - mp.nacc) * 64 + lane, nb = mp.ndb * 16;
  float a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = 0.0f;
  const int T = k >> 4, c = k & 15;  // bias tile T (slot in db[]), column c
  if (k < nb) {
    const size_t off = (size_t)(mp.nacc + (T >> 2)) * 256 + (T & 3);
    for (int w = w0; w < w1; ++w) {
      const float* p = slabs + (size_t)w * stride + off;
      a[w & 7] += (p[(c)*4] + p[(16 + c) * 4]) + (p[(32 + c) * 4] + p[(48 + c) * 4]);
    }
  }
  part[pw][lane] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (pw != 0 || k >= nb) return;
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 16; i += 4) s += (part[i][lane] + part[i + 1][lane]) + (part[i + 2][lane] + part[i + 3][lane]);
  const int l = mp.db_layer[T];
  if (l < 0) return;
  const int o = 16 * mp.db_tile[T] + c;
  if (o < pd.L[l].OUT && gp.b[l]) gp.b[l][o] = s;
}

// A backward over no samples: the parameter gradients are still OVERWRITTEN (umhs_field_bwd's contract), with zeros.  One workgroup
// per tensor (blockIdx.x = layer, blockIdx.y = weight / bias).
__global__ __launch_bounds__(256) void field_zero_grads_kernel(GradPtrs gp, PackDesc pd) {
  const int l = blockIdx.x;
  float* const p = blockIdx.y ? gp.b[l] : gp.W[l];
  const int len = blockIdx.y ? pd.L[l].OUT : pd.L[l].OUT * pd.L[l].IN;
  if (!p) return;
  for (int i = threadIdx.x; i < len; i += 256) p[i] = 0.0f;
}

// =============================================================================================
// host side
// =============================================================================================
static int round16(int x) { return (x + 15) & ~15; }

static int build_pack_desc(const umhs_field_cfg* cfg, const umhs_field_params* p, PackDesc* pd, int* TB_out, int part = 0) {
  // part 0: every layer, 1: mlp_base only, 2: heads only (backward kernels)
  const int B = cfg->n_bands, C = cfg->n_classes, spec = cfg->pred_specular != 0, dens = cfg->density_only != 0;
  const int TB = dens ? 0 : (B + 15) / 16;
  *TB_out = TB;
  auto set = [&](int l, const float* W, const float* b, int kind, int KS, int OT, int OUT, int IN) {
    pd->L[l].W = W, pd->L[l].b = b, pd->L[l].kind = kind, pd->L[l].KS = KS, pd->L[l].OT = OT, pd->L[l].OUT = OUT,
    pd->L[l].IN = IN;
  };
  set(L_B0, p->base_w0, p->base_b0, IN_ENC, 8, 4, 64, 32);
  set(L_B1, p->base_w1, p->base_b1, IN_HID64, 16, 1, 16, 64);
  const int h = dens ? 0 : 1;
  set(L_H0, p->head_w0, p->head_b0, IN_27, 7, 4 * h, 64, 27);
  set(L_H1, p->head_w1, p->head_b1, IN_HID64, 16, 4 * h, 64, 64);
  set(L_H2, p->head_w2, p->head_b2, IN_HID64, 16, 1 * h, C, 64);
  set(L_F0, p->feat_w0, p->feat_b0, IN_27, 7, 4 * h, 64, 27);
  set(L_F1, p->feat_w1, p->feat_b1, IN_HID64, 16, 4 * h, 64, 64);
  set(L_F2, p->feat_w2, p->feat_b2, IN_HID64, 16, 1 * h, spec ? C + 1 : C, 64);
  const int d = (!dens && spec) ? 1 : 0;
  set(L_D0, p->dir_w0, p->dir_b0, IN_DIR28, 7, 1 * d, 16, 28);
  set(L_D1, p->dir_w1, p->dir_b1, IN_HID16, 4, TB * d, B, 16);
  set(L_MX, p->endmembers, nullptr, IN_MIX, 4, TB * h, B, C);  // "W" = E [C][B]: OUT = B, IN = C
  for (int l = 0; l < NLAYERS; ++l)
    if ((part == 1 && l > L_B1) || (part == 2 && l <= L_B1)) pd->L[l].OT = 0;
  int off = 0;
  for (int l = 0; l < NLAYERS; ++l) {
    pd->L[l].off_w = off;
    off += pd->L[l].OT * ((pd->L[l].KS + 3) / 4) * 256;
  }
  pd->total_w = off;
  for (int l = 0; l < NLAYERS; ++l) {
    pd->L[l].off_b = off;
    if (l != L_MX) off += 16 * pd->L[l].OT;
  }
  pd->total = off;
  // pointers required for the layers in use
  for (int l = 0; l < NLAYERS; ++l)
    if (pd->L[l].OT > 0 && (!pd->L[l].W || (l != L_MX && !pd->L[l].b))) return UMHS_ERR_ARG;
  return UMHS_OK;
}

static int check_cfg(const umhs_field_cfg* cfg) {
  if (!cfg) return UMHS_ERR_ARG;
  if (cfg->density_only) return UMHS_OK;
  if (cfg->n_bands < 1 || cfg->n_classes < 1 || !(cfg->temperature > 0.0f)) return UMHS_ERR_ARG;
  if (cfg->n_classes > 15 || cfg->n_bands > 256) return UMHS_ERR_UNSUPPORTED;
  return UMHS_OK;
}

// ---- forward on the bf16x3 chain: which layers convert, the compact LDS image, the global bf16x3 image ---------------------------
struct FwdBfPlan {
  PackDesc pd;  // offsets local to the compact fp32 part
  FwdBfArgs args;
  BfPlan bp;
  size_t lds;
};
static bool fwd_bf_plan(const PackDesc& pd_all, FwdBfPlan* fp, bool base_only = false) {
  // base_only: the LDS image of the density half run from the FULL image (umhs_field_base_fwd): mlp_base's two packs and biases
  const int conv[] = {L_B0, L_B1, L_H0, L_H1, L_H2, L_F0, L_F1, L_F2};
  fp->pd = pd_all;
  BfOffs& bo = fp->args.bo;
  for (int l = 0; l < NLAYERS; ++l) bo.f[l] = -1;
  for (int l = 0; l < NTLAYERS; ++l) bo.t[l] = -1;
  fp->bp.n = 0;
  int off = 0;
  for (int l : conv) {
    const LayerDesc& L = pd_all.L[l];
    if (L.OT == 0) continue;
    const int KS4 = (L.KS + 3) / 4;
    fp->bp.c[fp->bp.n++] = BfConv{0, L.off_w, KS4, L.OT, off};
    bo.f[l] = off, off += L.OT * ((KS4 + 1) / 2) * 3 * 256;
  }
  fp->bp.total = off;
  ImgSegs& sf = fp->args.seg_f;
  sf.n = 0;
  bool ok = true;
  auto add = [&](int src, int dst, int len) {
    if (len == 0) return;
    if (sf.n && sf.src[sf.n - 1] + sf.len[sf.n - 1] == src && sf.dst[sf.n - 1] + sf.len[sf.n - 1] == dst) {
      sf.len[sf.n - 1] += len;
      return;
    }
    if (sf.n == 6) {
      ok = false;
      return;
    }
    sf.src[sf.n] = src, sf.dst[sf.n] = dst, sf.len[sf.n] = len, ++sf.n;
  };
  int cur = 0;
  for (int l = 0; l < NLAYERS; ++l) {
    const LayerDesc& L = pd_all.L[l];
    if (bo.f[l] >= 0 || L.OT == 0 || base_only) continue;
    const int len = L.OT * ((L.KS + 3) / 4) * 256;
    add(L.off_w, cur, len);
    fp->pd.L[l].off_w = cur, cur += len;
  }
  for (int l = 0; l < NLAYERS; ++l) {
    const LayerDesc& L = pd_all.L[l];
    if (l == L_MX || L.OT == 0 || (base_only && l > L_B1)) continue;
    add(L.off_b, cur, 16 * L.OT);
    fp->pd.L[l].off_b = cur, cur += 16 * L.OT;
  }
  fp->args.bf_off = (cur + 3) & ~3;
  if (base_only) off = bo.f[L_H0] >= 0 ? bo.f[L_H0] : off;  // mlp_base's packs open the bf16x3 image
  fp->args.seg_b.n = 1, fp->args.seg_b.src[0] = 0, fp->args.seg_b.dst[0] = 0, fp->args.seg_b.len[0] = off;
  fp->args.bf_image = nullptr;
  fp->lds = (size_t)(fp->args.bf_off + off) * 4;
  return ok && fp->lds <= 160 * 1024;
}
// workspace of the forward: [fp32 pack image][bf16x3 image of the converted layers]
static size_t fwd_ws_need(const PackDesc& pd, bool dens) {
  size_t need = (size_t)((pd.total + 63) & ~63) * 4 + 512;
  if (!dens) {
    FwdBfPlan fp;
    fwd_bf_plan(pd, &fp);
    need += (size_t)fp.bp.total * 4;
  }
  return need;
}
static void launch_fwd_packs(const PackDesc& pd, bool dens, float* img, umhs_stream_t stream) {
  PackJob jb = {};
  jb.pd = pd, jb.img = img;
  int n = pd.total;
  if (!dens) {
    FwdBfPlan fp;
    fwd_bf_plan(pd, &fp);
    jb.bp = fp.bp, jb.bf = reinterpret_cast<uint32_t*>(img + ((pd.total + 63) & ~63)), n += fp.bp.total;
  }
  hipLaunchKernelGGL(field_pack_all_kernel, dim3((n + 255) / 256), dim3(256), 0, umhs_s(stream), jb);
}

extern "C" size_t umhs_field_fwd_workspace_bytes(const umhs_field_cfg* cfg) {
  if (check_cfg(cfg)) return 0;
  umhs_field_params dummy = {};
  const float one = 0.0f;
  const float** pp = reinterpret_cast<const float**>(&dummy);
  for (size_t i = 0; i < sizeof(dummy) / sizeof(float*); ++i) pp[i] = &one;  // layout only, never dereferenced
  PackDesc pd;
  int TB;
  if (build_pack_desc(cfg, &dummy, &pd, &TB)) return 0;
  return fwd_ws_need(pd, cfg->density_only != 0);
}

// Builds the forward pack image into the workspace ahead of time (depends on the parameters only); pass pack_ready = 1 and
// the same workspace to umhs_field_fwd afterwards.
extern "C" int umhs_field_fwd_prepare(const umhs_field_cfg* cfg, const umhs_field_params* params, void* workspace,
                                      size_t workspace_bytes, umhs_stream_t stream) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!params || !workspace) return UMHS_ERR_ARG;
  PackDesc pd;
  int TB;
  rc = build_pack_desc(cfg, params, &pd, &TB);
  if (rc) return rc;
  if (workspace_bytes < fwd_ws_need(pd, cfg->density_only != 0)) return UMHS_ERR_WORKSPACE;
  float* img = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  launch_fwd_packs(pd, cfg->density_only != 0, img, stream);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

static int run_field_fwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc,
                         int64_t stride_n, int64_t stride_l, const float* world_pos, const float* directions,
                         const float* selector, int64_t n, float* sigma, float* sigma_raw, float* emb,
                         float* spectral, float* spectral2, float* specular, float* abundances, float* feat_logits,
                         void* workspace, size_t workspace_bytes, int pack_ready, umhs_stream_t stream) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (!params || !enc || !selector || !sigma || n < 0) return UMHS_ERR_ARG;
  if (((stride_n & 1) || (stride_l & 1) || ((uintptr_t)enc & 7))) return UMHS_ERR_ARG;
  const bool dens = cfg->density_only != 0, spec = cfg->pred_specular != 0;
  if (!dens && (!world_pos || !spectral || (spec && !directions))) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  PackDesc pd;
  int TB;
  rc = build_pack_desc(cfg, params, &pd, &TB);
  if (rc) return rc;
  FieldIO io = {};
  io.enc = enc, io.sn = stride_n, io.sl = stride_l, io.wpos = world_pos, io.dirs = directions, io.sel = selector;
  io.n = n, io.B = cfg->n_bands, io.C = cfg->n_classes, io.TB = TB, io.temperature = cfg->temperature;
  io.sigma = sigma, io.sigma_raw = sigma_raw, io.emb = emb, io.spectral = spectral, io.spectral2 = spectral2;
  io.specular = specular, io.abund = abundances, io.feat_logits = dens ? nullptr : feat_logits;
  const size_t lds_bytes = (size_t)((pd.total + 3) & ~3) * 4;
  // (one shape per case: the bf16x3 chain as 8 waves x 2 sample tiles wherever a prebuilt image exists and its packs fit the LDS, else
  // the fp32 chain as 4 x 2.  The 12 x 1 / 16 x 1 / fp32 8 x 1 forms of round 2 were measured -- 16 x 1: 90 vs 97 us alone, 0.875 vs
  // 0.846 ms inside the step, where it starves the side-stream kernels -- and removed in round 3.)
  const float* image = nullptr;
  if (workspace) {  // optional: prebuilt pack image (without it every workgroup gathers the image itself)
    if (workspace_bytes < fwd_ws_need(pd, dens)) return UMHS_ERR_WORKSPACE;
    float* img = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (!pack_ready) {  // else: umhs_field_fwd_prepare already built it in this workspace
      launch_fwd_packs(pd, dens, img, stream);
      UMHS_CHECK_LAUNCH();
    }
    image = img;
  }
  FwdBfPlan fp;
  FwdBfArgs no_bf = {};
  const bool bf = !dens && image && fwd_bf_plan(pd, &fp);  // no image: each workgroup gathers fp32 packs
  if (bf) fp.args.bf_image = image + ((pd.total + 63) & ~63);
  // samples per workgroup iteration: 16 x NT x waves
  const int tile_samples = bf ? 256 : 128;
  const int64_t ntiles = (n + tile_samples - 1) / tile_samples;
  const int blocks_per_cu = bf ? 1 : (lds_bytes <= 78 * 1024 ? 2 : 1);
  const unsigned grid = (unsigned)(ntiles < 256 * blocks_per_cu ? ntiles : 256 * blocks_per_cu);
  const size_t lds_launch = bf ? fp.lds : lds_bytes;
#define LAUNCH_FWD(S, D, NT_, W_, ...)                                                                                       \
  do {                                                                                                                       \
    rc = set_lds(field_fwd_kernel<S, D, NT_, W_, ##__VA_ARGS__>, lds_launch);                                                 \
    if (rc) return rc;                                                                                                       \
    hipLaunchKernelGGL((field_fwd_kernel<S, D, NT_, W_, ##__VA_ARGS__>), dim3(grid), dim3(64 * W_), lds_launch, umhs_s(stream), \
                       io, bf ? fp.pd : pd, image, bf ? fp.args : no_bf);                                                    \
  } while (0)
  if (dens)
    LAUNCH_FWD(false, true, 2, 4);
  else if (spec) {
    if (bf)
      LAUNCH_FWD(true, false, 2, 8, true);
    else
      LAUNCH_FWD(true, false, 2, 4);
  } else {
    if (bf)
      LAUNCH_FWD(false, false, 2, 8, true);
    else
      LAUNCH_FWD(false, false, 2, 4);
  }
#undef LAUNCH_FWD
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_field_fwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc,
                              int64_t stride_n, int64_t stride_l, const float* world_pos, const float* directions,
                              const float* selector, int64_t n, float* sigma, float* sigma_raw, float* emb,
                              float* spectral, float* spectral2, float* specular, float* abundances, float* feat_logits,
                              void* workspace, size_t workspace_bytes, int pack_ready, umhs_stream_t stream) {
  return run_field_fwd(cfg, params, enc, stride_n, stride_l, world_pos, directions, selector, n, sigma, sigma_raw, emb,
                       spectral, spectral2, specular, abundances, feat_logits, workspace, workspace_bytes, pack_ready, stream);
}

// ---- the forward as two launches with the rendering weights known in between (training step) --------------------------------
// umhs_field_base_fwd: mlp_base only (sigma, sigma_raw, emb) from the FULL configuration's prepared workspace (the same pack
// images umhs_field_heads_fwd uses, built once by umhs_field_fwd_prepare).
extern "C" int umhs_field_base_fwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc, int64_t stride_n,
                                   int64_t stride_l, const float* selector, int64_t n, float* sigma, float* sigma_raw, float* emb,
                                   float* base16, void* workspace, size_t workspace_bytes, int pack_ready, umhs_stream_t stream) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cfg->density_only) return UMHS_ERR_UNSUPPORTED;
  if (!params || !enc || !selector || !sigma || !workspace || n < 0) return UMHS_ERR_ARG;
  if ((stride_n & 1) || (stride_l & 1) || ((uintptr_t)enc & 7)) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  PackDesc pd;
  int TB;
  rc = build_pack_desc(cfg, params, &pd, &TB);
  if (rc) return rc;
  if (workspace_bytes < fwd_ws_need(pd, false)) return UMHS_ERR_WORKSPACE;
  float* img = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  if (!pack_ready) {
    launch_fwd_packs(pd, false, img, stream);
    UMHS_CHECK_LAUNCH();
  }
  FwdBfPlan fp;
  if (!fwd_bf_plan(pd, &fp, true)) return UMHS_ERR_UNSUPPORTED;
  fp.args.bf_image = img + ((pd.total + 63) & ~63);
  FieldIO io = {};
  io.enc = enc, io.sn = stride_n, io.sl = stride_l, io.sel = selector, io.n = n, io.B = cfg->n_bands, io.C = cfg->n_classes, io.TB = 0;
  io.temperature = cfg->temperature, io.sigma = sigma, io.sigma_raw = sigma_raw, io.emb = emb, io.bo16 = base16;
  if (base16 && ((uintptr_t)base16 & 15)) return UMHS_ERR_ARG;
  const int64_t ntiles = (n + 127) / 128;
  // One workgroup per CU.  Alone the kernel is fastest with 4 (33 us at 524 k samples; 44 us with 1) -- inside the training
  // step ONE is 45-50 us faster end to end (C3 1.67 vs 1.72 ms, C5 1.49 vs 1.54, three A/B pairs): the bucket histogram of the hash-grid
  // backward runs on the side stream at that moment, and a kernel that fills every CU pushes it under the heads kernel instead.
  const unsigned grid = (unsigned)(ntiles < 256 ? ntiles : 256);
  rc = set_lds(field_fwd_kernel<false, true, 2, 4, true>, fp.lds);
  if (rc) return rc;
  hipLaunchKernelGGL((field_fwd_kernel<false, true, 2, 4, true>), dim3(grid), dim3(256), fp.lds, umhs_s(stream), io, fp.pd,
                     (const float*)img, fp.args);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// Finishes the per-ray sums of umhs_field_heads_fwd (see field_fwd_kernel, HEADS): one workgroup per ray.  Adds the ray's tile
// partials in tile order (only its first tile can hold it as that tile's LAST ray, every later tile starts with it; a ray strictly
// inside one tile was written by the heads kernel), then mixes once per ray: spectral2[b] = sum_c (sum_n w_n m_n[c]) E[c][b].
__global__ __launch_bounds__(256) void field_heads_finish_kernel(const float* __restrict__ part_spec, const float* __restrict__ part_m,
                                                                const float* __restrict__ part_ab, const int64_t* __restrict__ ray_of,
                                                                const int64_t* __restrict__ pinfo, int64_t n, int64_t R, int B, int BP,
                                                                int C, const float* __restrict__ E, float* __restrict__ mix16,
                                                                float* __restrict__ c_spectral, float* __restrict__ c_mix,
                                                                float* __restrict__ c_specular, float* __restrict__ cab) {
  // four rays per workgroup (one wave each): four independent chains of dependent loads in flight instead of one
  __shared__ float sM[4][16];
  const int tid = threadIdx.x, sub = tid >> 6, lane = tid & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + sub;
  const bool live = ray < R;
  int64_t ts = 0, te = -1;
  bool inside = false;  // strictly inside one tile: the heads kernel wrote this ray's sums itself
  int az0 = 0;
  if (live) {
    const int64_t s0 = pinfo[2 * ray], cnt = pinfo[2 * ray + 1];
    ts = s0 >> 4, te = cnt > 0 ? (s0 + cnt - 1) >> 4 : ts - 1;
    if (cnt > 0) {
      const bool first = ray_of[16 * ts] == ray;
      if (ts == te) {
        const int64_t l = 16 * ts + 15 < n ? 16 * ts + 15 : n - 1;
        inside = !first && ray_of[l] != ray;
      }
      az0 = first ? 0 : 1;
    }
  }
  if (live && lane < 16) {
    float acc = 0.0f;
    if (inside) {
      acc = mix16[ray * 16 + lane];
    } else {
      for (int64_t t = ts; t <= te; ++t) acc += part_m[(t * 2 + (t == ts ? az0 : 0)) * 16 + lane];
      mix16[ray * 16 + lane] = acc;
    }
    sM[sub][lane] = lane < C ? acc : 0.0f;
  } else if (live && lane < 32 && cab && !inside && lane - 16 < C) {
    float acc = 0.0f;
    for (int64_t t = ts; t <= te; ++t) acc += part_ab[(t * 2 + (t == ts ? az0 : 0)) * 16 + (lane - 16)];
    cab[ray * C + (lane - 16)] = acc;
  }
  __syncthreads();
  if (!live) return;
  for (int b = lane; b < B; b += 64) {
    float mix = 0.0f;
    for (int c = 0; c < C; ++c) mix += sM[sub][c] * E[(int64_t)c * B + b];
    if (part_spec) {  // specular head: spectral = mixing + specular
      float sp = 0.0f;
      if (inside) {
        sp = c_specular[ray * B + b];
      } else {
        for (int64_t t = ts; t <= te; ++t) sp += part_spec[(t * 2 + (t == ts ? az0 : 0)) * BP + b];
        c_specular[ray * B + b] = sp;
      }
      c_mix[ray * B + b] = mix;
      c_spectral[ray * B + b] = mix + sp;
    } else {
      c_spectral[ray * B + b] = mix;
    }
  }
}

// 1 when umhs_field_base_fwd / umhs_field_heads_fwd can serve this configuration (every pack of the bf16x3 forward LDS-resident).
extern "C" int umhs_field_heads_fwd_supported(const umhs_field_cfg* cfg) {
  if (check_cfg(cfg) || cfg->density_only) return 0;
  umhs_field_params dummy = {};
  const float zero = 0.0f;
  const float** pp = reinterpret_cast<const float**>(&dummy);
  for (size_t i = 0; i < sizeof(dummy) / sizeof(float*); ++i) pp[i] = &zero;  // layout only, never dereferenced
  PackDesc pd;
  int TB;
  if (build_pack_desc(cfg, &dummy, &pd, &TB)) return 0;
  FwdBfPlan fp;
  return fwd_bf_plan(pd, &fp, true) && fwd_bf_plan(pd, &fp) ? 1 : 0;
}

// scratch of umhs_field_heads_fwd: [specular partials G*2*BP (specular head only)][w m partials G*2*16][abundance partials G*2*16]
// [mix16 R*16], G = ceil(n / 16) tiles
static size_t heads_scratch_floats(const umhs_field_cfg* cfg, int64_t n, int64_t n_rays, size_t (&off)[4]) {
  const size_t G = (size_t)((n + 15) / 16), BP = 16 * (size_t)((cfg->n_bands + 15) / 16);
  off[0] = 0;
  off[1] = off[0] + (cfg->pred_specular ? G * 2 * BP : 0);
  off[2] = off[1] + G * 2 * 16;
  off[3] = off[2] + G * 2 * 16;
  return off[3] + (size_t)n_rays * 16;
}
extern "C" size_t umhs_field_heads_fwd_scratch_bytes(const umhs_field_cfg* cfg, int64_t n, int64_t n_rays) {
  if (check_cfg(cfg) || cfg->density_only || n < 0 || n_rays < 0) return 0;
  size_t off[4];
  return heads_scratch_floats(cfg, n, n_rays, off) * sizeof(float) + 256;
}
// Byte offset of mix16 [n_rays,16] inside that scratch (the per-ray sums of w m the finish pass leaves there: what a material edit
// re-mixes, umhs_material.hip), or -1 for a configuration the forward refuses.  Host arithmetic only.
extern "C" int64_t umhs_field_heads_fwd_mix_offset(const umhs_field_cfg* cfg, int64_t n, int64_t n_rays) {
  if (check_cfg(cfg) || cfg->density_only || n < 0 || n_rays < 0) return -1;
  size_t off[4];
  heads_scratch_floats(cfg, n, n_rays, off);
  return (int64_t)(off[3] * sizeof(float));
}

// umhs_field_heads_fwd: everything after mlp_base from its saved outputs (emb [N,15] or the aligned [N,16] rows), with the per-ray
// sums comp_*[r] = sum over the samples n of ray r of weights[n] * stream[n] formed inside the kernel + the finish pass.  No [N,B]
// array exists: the mixing term is summed per ray as w m (16 classes) and multiplied by the endmembers once per ray, the specular
// term per band tile.  ray_indices [N] non-decreasing, packed_info [R,2] = (first sample, count) as umhs_pack_info makes them.
extern "C" int umhs_field_heads_fwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* emb, int emb_stride,
                                    const float* world_pos, const float* directions, int64_t n, const float* weights,
                                    const int64_t* ray_indices, const int64_t* packed_info, int64_t n_rays, float* abundances,
                                    float* feat_logits, float* comp_spectral, float* comp_spectral2, float* comp_specular,
                                    float* comp_abundances, void* scratch, size_t scratch_bytes, void* workspace,
                                    size_t workspace_bytes, int pack_ready, umhs_stream_t stream) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cfg->density_only) return UMHS_ERR_UNSUPPORTED;
  const bool spec = cfg->pred_specular != 0;
  if (!params || !params->endmembers || !workspace || n < 0 || n_rays < 0 || !packed_info || !comp_spectral || !scratch)
    return UMHS_ERR_ARG;
  if (spec && (!comp_spectral2 || !comp_specular)) return UMHS_ERR_ARG;
  if (n > 0 && (!emb || !world_pos || !weights || !ray_indices || (spec && !directions))) return UMHS_ERR_ARG;
  if ((emb_stride != 15 && emb_stride != 16) || (emb_stride == 16 && ((uintptr_t)emb & 15))) return UMHS_ERR_ARG;
  if (n_rays == 0) return UMHS_OK;
  PackDesc pd;
  int TB;
  rc = build_pack_desc(cfg, params, &pd, &TB);
  if (rc) return rc;
  if (workspace_bytes < fwd_ws_need(pd, false)) return UMHS_ERR_WORKSPACE;
  if (scratch_bytes < umhs_field_heads_fwd_scratch_bytes(cfg, n, n_rays) || ((uintptr_t)scratch & 15)) return UMHS_ERR_WORKSPACE;
  float* img = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  if (!pack_ready) {
    launch_fwd_packs(pd, false, img, stream);
    UMHS_CHECK_LAUNCH();
  }
  size_t off[4];
  heads_scratch_floats(cfg, n, n_rays, off);
  float* const sc = reinterpret_cast<float*>(scratch);
  float *part_spec = spec ? sc + off[0] : nullptr, *part_m = sc + off[1], *part_ab = sc + off[2], *mix16 = sc + off[3];
  if (n > 0) {
    FwdBfPlan fp;
    if (!fwd_bf_plan(pd, &fp)) return UMHS_ERR_UNSUPPORTED;
    fp.args.bf_image = img + ((pd.total + 63) & ~63);
    FieldIO io = {};
    io.wpos = world_pos, io.dirs = directions, io.n = n, io.B = cfg->n_bands, io.C = cfg->n_classes, io.TB = TB;
    io.temperature = cfg->temperature, io.emb_in = emb, io.abund = abundances, io.feat_logits = feat_logits;
    if (emb_stride == 16) io.bo16_in = emb;
    io.weights = weights, io.ray_of = ray_indices, io.part = part_spec, io.part_m = part_m, io.mix16 = mix16;
    io.part_ab = comp_abundances ? part_ab : nullptr, io.comp_ab = comp_abundances;
    io.comp[0] = comp_spectral, io.comp[1] = comp_spectral2, io.comp[2] = comp_specular, io.n_streams = spec ? 3 : 1;
    const int64_t ntiles = (n + 255) / 256;
    const unsigned grid = (unsigned)(ntiles < 256 ? ntiles : 256);
    if (spec) {
      rc = set_lds(field_fwd_kernel<true, false, 2, 8, true, true>, fp.lds);
      if (rc) return rc;
      hipLaunchKernelGGL((field_fwd_kernel<true, false, 2, 8, true, true>), dim3(grid), dim3(512), fp.lds, umhs_s(stream), io,
                         fp.pd, (const float*)img, fp.args);
    } else {
      rc = set_lds(field_fwd_kernel<false, false, 2, 8, true, true>, fp.lds);
      if (rc) return rc;
      hipLaunchKernelGGL((field_fwd_kernel<false, false, 2, 8, true, true>), dim3(grid), dim3(512), fp.lds, umhs_s(stream), io,
                         fp.pd, (const float*)img, fp.args);
    }
    UMHS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(field_heads_finish_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, umhs_s(stream), (const float*)part_spec,
                     (const float*)part_m, (const float*)part_ab, ray_indices, packed_info, n, n_rays, cfg->n_bands, 16 * TB, cfg->n_classes,
                     params->endmembers, mix16, comp_spectral, comp_spectral2, comp_specular, comp_abundances);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

struct BwdPlan {
  int TB;
  PackDesc pd_all;
  TPackDesc td;
};

static int build_bwd_plan(const umhs_field_cfg* cfg, const umhs_field_params* p, BwdPlan* pl) {
  const int B = cfg->n_bands, C = cfg->n_classes, spec = cfg->pred_specular != 0;
  int TB;
  int rc = build_pack_desc(cfg, p, &pl->pd_all, &TB, 0);
  if (rc) return rc;
  pl->TB = TB;
  // with the specular head the backward serves up to 192 bands (12 band tiles): beyond, part 0's kernel does not hold its registers
  // (110 dwords spilled at 16 tiles) and has no test behind it -- reported, and the callers keep what they can (known limits)
  if (spec && TB > 12) return UMHS_ERR_UNSUPPORTED;

  TPackDesc* td = &pl->td;
  auto sett = [&](int l, const float* W, int OUT, int IN, int KS, int OT, int rowmap) {
    td->L[l].W = W, td->L[l].OUT = OUT, td->L[l].IN = IN, td->L[l].KS = KS, td->L[l].OT = OT, td->L[l].rowmap = rowmap;
  };
  sett(T_B1, p->base_w1, 16, 64, 4, 4, 0);
  sett(T_B0, p->base_w0, 64, 32, 16, 2, 0);
  sett(T_H2, p->head_w2, C, 64, 4, 4, 0);
  sett(T_H1, p->head_w1, 64, 64, 16, 4, 0);
  sett(T_H0, p->head_w0, 64, 27, 16, 1, 1);
  sett(T_F2, p->feat_w2, spec ? C + 1 : C, 64, 4, 4, 0);
  sett(T_F1, p->feat_w1, 64, 64, 16, 4, 0);
  sett(T_F0, p->feat_w0, 64, 27, 16, 1, 1);
  sett(T_D1, p->dir_w1, B, 16, 4 * TB, spec ? 1 : 0, 0);
  sett(T_MX, p->endmembers, C, B, 4 * TB, 1, 2);  // E [C][B]
  int off = 0;
  for (int l = 0; l < NTLAYERS; ++l) {
    td->L[l].off = off;
    off += td->L[l].OT * ((td->L[l].KS + 3) / 4) * 256;
  }
  td->total = off;

  return UMHS_OK;
}

// ---- transpose-free backward: per-part LDS images and launch ------------------------------------------------------------
static int tf_tbmax(int TB) { return TB <= 2 ? 2 : (TB <= 4 ? 4 : (TB <= 8 ? 8 : (TB <= 12 ? 12 : (TB <= 16 ? 16 : 0)))); }
static int tf_nitems(int tbmax) {
  switch (tbmax) {
    case 2: return TfSlots<2>::NITEMS;
    case 4: return TfSlots<4>::NITEMS;
    case 8: return TfSlots<8>::NITEMS;
    case 12: return TfSlots<12>::NITEMS;
    default: return TfSlots<16>::NITEMS;
  }
}
static size_t bwd_slab_floats(const BwdPlan& pl, int64_t n) {  // the per-workgroup slabs
  const size_t tf = (size_t)(tf_grid(n) + (tf_grid(n) + 15) / 16) * tf_nitems(tf_tbmax(pl.TB) ? tf_tbmax(pl.TB) : 16) * 256;  // + the folded set
  return tf;
}
static int bf_image_dwords(const BwdPlan& pl);
static size_t bwd_workspace_need(const BwdPlan& pl, int64_t n) {
  return ((size_t)pl.td.total + bwd_slab_floats(pl, n) + (size_t)n * 48 + pl.pd_all.total + bf_image_dwords(pl)) * 4 + 4096 + 1024;
}

// The layers whose products run as three-piece bf16 MFMAs (every layer with >= 7 k-steps), in the order of the global bf16x3 image:
// part 0's first (head MLP, directional hidden layer, their transposes), then part 1's.
static const int BF_F0[] = {L_H0, L_H1, L_H2, L_D0}, BF_T0[] = {T_H1, T_H0};
static const int BF_F1[] = {L_B0, L_B1, L_F0, L_F1}, BF_T1[] = {T_B0, T_F1, T_F0};
static void build_bf_plan(const BwdPlan& pl, BfPlan* bp, int (&dst_f)[NLAYERS], int (&dst_t)[NTLAYERS], int (&part_range)[2][2]) {
  for (int l = 0; l < NLAYERS; ++l) dst_f[l] = -1;
  for (int l = 0; l < NTLAYERS; ++l) dst_t[l] = -1;
  bp->n = 0;
  int off = 0;
  auto addf = [&](int l) {
    const LayerDesc& L = pl.pd_all.L[l];
    if (L.OT == 0) return;
    const int KS4 = (L.KS + 3) / 4;
    bp->c[bp->n++] = BfConv{0, L.off_w, KS4, L.OT, off};
    dst_f[l] = off, off += L.OT * ((KS4 + 1) / 2) * 3 * 256;
  };
  auto addt = [&](int l) {
    const TDesc& T = pl.td.L[l];
    if (T.OT == 0) return;
    const int KS4 = (T.KS + 3) / 4;
    bp->c[bp->n++] = BfConv{1, T.off, KS4, T.OT, off};
    dst_t[l] = off, off += T.OT * ((KS4 + 1) / 2) * 3 * 256;
  };
  part_range[0][0] = off;
  for (int l : BF_F0) addf(l);
  for (int l : BF_T0) addt(l);
  part_range[0][1] = part_range[1][0] = off;
  for (int l : BF_F1) addf(l);
  for (int l : BF_T1) addt(l);
  part_range[1][1] = off;
  bp->total = off;
}
static int bf_image_dwords(const BwdPlan& pl) {
  BfPlan bp;
  int df[NLAYERS], dt[NTLAYERS], pr[2][2];
  build_bf_plan(pl, &bp, df, dt, pr);
  return bp.total;
}

static bool tf_part(const BwdPlan& pl, int part, bool bf, TfPart* pp) {
  const int fl0[] = {L_H0, L_H1, L_H2, L_D0, L_D1}, tl0[] = {T_H2, T_H1, T_H0, T_D1, T_MX};
  const int fl1[] = {L_B0, L_B1, L_F0, L_F1}, tl1[] = {T_B1, T_B0, T_F2, T_F1, T_F0};
  const int* fl = part == 0 ? fl0 : fl1;
  const int nfl = part == 0 ? 5 : 4;
  const int* tl = part == 0 ? tl0 : tl1;
  const int ntl = 5;
  pp->pd = pl.pd_all, pp->td = pl.td;
  pp->seg_f.n = pp->seg_t.n = pp->seg_b.n = 0;
  BfPlan bp;
  int dst_f[NLAYERS], dst_t[NTLAYERS], pr[2][2];
  build_bf_plan(pl, &bp, dst_f, dst_t, pr);
  for (int l = 0; l < NLAYERS; ++l) pp->bo.f[l] = (bf && dst_f[l] >= pr[part][0] && dst_f[l] < pr[part][1]) ? dst_f[l] - pr[part][0] : -1;
  for (int l = 0; l < NTLAYERS; ++l) pp->bo.t[l] = (bf && dst_t[l] >= pr[part][0] && dst_t[l] < pr[part][1]) ? dst_t[l] - pr[part][0] : -1;
  bool ok = true;
  auto add = [&](ImgSegs& sg, int src, int dst, int len) {
    if (len == 0) return;
    if (sg.n && sg.src[sg.n - 1] + sg.len[sg.n - 1] == src && sg.dst[sg.n - 1] + sg.len[sg.n - 1] == dst) {
      sg.len[sg.n - 1] += len;
      return;
    }
    if (sg.n == 6) {
      ok = false;
      return;
    }
    sg.src[sg.n] = src, sg.dst[sg.n] = dst, sg.len[sg.n] = len, ++sg.n;
  };
  int cur = 0;
  for (int i = 0; i < nfl; ++i) {  // fp32 weights (of the layers that keep them), then biases, in the kernel's own compact image
    const LayerDesc& L = pl.pd_all.L[fl[i]];
    if (pp->bo.f[fl[i]] >= 0) continue;
    const int len = L.OT * ((L.KS + 3) / 4) * 256;
    add(pp->seg_f, L.off_w, cur, len);
    pp->pd.L[fl[i]].off_w = cur, cur += len;
  }
  for (int i = 0; i < nfl; ++i) {
    const LayerDesc& L = pl.pd_all.L[fl[i]];
    add(pp->seg_f, L.off_b, cur, 16 * L.OT);
    pp->pd.L[fl[i]].off_b = cur, cur += 16 * L.OT;
  }
  pp->wt_off = (cur + 3) & ~3;
  cur = 0;
  for (int i = 0; i < ntl; ++i) {
    const TDesc& T = pl.td.L[tl[i]];
    if (pp->bo.t[tl[i]] >= 0) continue;
    const int len = T.OT * ((T.KS + 3) / 4) * 256;
    add(pp->seg_t, T.off, cur, len);
    pp->td.L[tl[i]].off = cur, cur += len;
  }
  pp->bf_off = (pp->wt_off + cur + 3) & ~3;
  cur = 0;
  if (bf) add(pp->seg_b, pr[part][0], 0, pr[part][1] - pr[part][0]), cur = pr[part][1] - pr[part][0];
  pp->lds = (size_t)(pp->bf_off + cur) * 4;
  if (pp->lds < (size_t)4 * TF_CHUNK * 256 * 4) pp->lds = (size_t)4 * TF_CHUNK * 256 * 4;  // the end-of-launch reduction's rounds
  return ok && pp->lds <= 160 * 1024;
}

template <int TBMAX>
static void fill_tf_map(TfMap* mp, bool spec, int TB) {
  typedef TfSlots<TBMAX> SL;
  static_assert(SL::NACC <= 128 && SL::NDB <= 64, "TfMap tables");
  mp->nacc = SL::NACC, mp->ndb = SL::NDB, mp->nitems = SL::NITEMS;
  for (int i = 0; i < 128; ++i) mp->layer[i] = -1, mp->to[i] = 0, mp->ti[i] = 0;
  for (int i = 0; i < 64; ++i) mp->db_layer[i] = -1, mp->db_tile[i] = 0;
  auto pairs = [&](int base, int layer, int TO, int TI) {
    for (int to = 0; to < TO; ++to)
      for (int ti = 0; ti < TI; ++ti) {
        const int i = base + to * TI + ti;
        mp->layer[i] = (short)layer, mp->to[i] = (short)to, mp->ti[i] = (short)ti;
      }
  };
  pairs(SL::A_B0, L_B0, 4, 2), pairs(SL::A_B1, L_B1, 1, 4);
  pairs(SL::A_H0, L_H0, 4, 2), pairs(SL::A_H1, L_H1, 4, 4), pairs(SL::A_H2, L_H2, 1, 4);
  pairs(SL::A_F0, L_F0, 4, 2), pairs(SL::A_F1, L_F1, 4, 4), pairs(SL::A_F2, L_F2, 1, 4);
  if (spec) pairs(SL::A_D0, L_D0, 1, 2);
  for (int t = 0; t < TB; ++t) {
    if (spec) mp->layer[SL::A_D1 + t] = L_D1, mp->to[SL::A_D1 + t] = (short)t;
    mp->layer[SL::A_MX + t] = L_MX, mp->to[SL::A_MX + t] = (short)t;
  }
  auto bias = [&](int base, int layer, int TO) {
    for (int t = 0; t < TO; ++t) mp->db_layer[base + t] = (short)layer, mp->db_tile[base + t] = (short)t;
  };
  bias(SL::D_B0, L_B0, 4), bias(SL::D_B1, L_B1, 1), bias(SL::D_H0, L_H0, 4), bias(SL::D_H1, L_H1, 4), bias(SL::D_H2, L_H2, 1);
  bias(SL::D_F0, L_F0, 4), bias(SL::D_F1, L_F1, 4), bias(SL::D_F2, L_F2, 1);
  if (spec) bias(SL::D_D0, L_D0, 1), bias(SL::D_D1, L_D1, TB);
}

// The compositing backward folded between the two parts (umhs_field_bwd_composited): part 0 forms d_spectral on the fly and emits the
// dot products, umhs_composite_bwd_dots turns them into d_sigma, part 1 consumes it.
struct BwdComp {
  const float *sigma, *t0, *t1, *weights, *d_comp, *d_acc;
  const int64_t *packed_info, *ray_of;
  int64_t n_rays;
  int grad_scaling;
  float *d_sigma, *dots;
  bool emb16;  // emb is the aligned [N,16] form umhs_field_base_fwd writes (slot 0 = sigma_raw)
  // per-ray mixing term: scratch [G R*16][part_ms tiles*2*16][mws16 R*16][dE partials chunks*C*B]
  float *mix_g, *part_ms, *mws16, *dE_part;
  const float* E;  // endmembers [C][B]
  float* dE;       // their gradient
  int B, C;
};

template <int TBMAX>
static int launch_tf(const BwdPlan& pl, const TfPart (&part)[2], int bf_mask, FieldIO io, bool spec, const float* img, const float* wT,
                     const float* bfimg, float* slabs, const GradPtrs& gp, int64_t n, umhs_stream_t stream, const BwdComp* bc) {
  typedef TfSlots<TBMAX> SL;
  const unsigned grid = tf_grid(n);
  const TfLaunch la = {io, img, wT, bfimg, slabs, grid, stream};
  int rc;
  if (bc) {
    hipLaunchKernelGGL(field_mix_grad_kernel, dim3((unsigned)((bc->n_rays + 15) / 16)), dim3(256), (size_t)32 * (bc->B | 1) * 4,
                       umhs_s(stream), bc->d_comp, bc->E, bc->n_rays, bc->B, bc->C, bc->mix_g);
    rc = (bf_mask & 1) ? launch_tf_p0z<TBMAX>(part[0], la, spec, true) : launch_tf_p0f<TBMAX>(part[0], la, spec, true);
    if (rc) return rc;
    UMHS_CHECK_LAUNCH();
    rc = umhs_composite_bwd_dots(bc->sigma, bc->t0, bc->t1, bc->packed_info, bc->n_rays, n, bc->weights, bc->dots, bc->d_acc,
                                 bc->grad_scaling, bc->d_sigma, stream);
    if (rc) return rc;
  } else {
    rc = (bf_mask & 1) ? launch_tf_p0z<TBMAX>(part[0], la, spec, false) : launch_tf_p0f<TBMAX>(part[0], la, spec, false);
    if (rc) return rc;
  }
  rc = launch_tf_p1<TBMAX>(part[1], la, bf_mask >> 1 & 1);
  if (rc) return rc;
  UMHS_CHECK_LAUNCH();
  TfMap mp;
  fill_tf_map<TBMAX>(&mp, spec, pl.TB);
  if (bc)  // the endmember gradient comes from the per-ray pass below, not from the slabs
    for (int t = 0; t < TBMAX; ++t) mp.layer[SL::A_MX + t] = -1;
  const float* rslabs = slabs;
  int nrs = (int)grid;
  if (grid > 2 * TF_FOLD) {  // fold the slabs 16 : 1 on every CU first (the workspace holds room for the folded set behind the slabs)
    float* folded = slabs + (size_t)grid * SL::NITEMS * 256;
    nrs = (int)((grid + TF_FOLD - 1) / TF_FOLD);
    hipLaunchKernelGGL(field_slab_fold_kernel, dim3(SL::NITEMS, (unsigned)nrs), dim3(256), 0, umhs_s(stream), (const float*)slabs, (int)grid,
                       SL::NITEMS, folded);
    rslabs = folded;
  }
  hipLaunchKernelGGL(field_reduce_tf_kernel, dim3(SL::NACC + (SL::NDB * 16 + 63) / 64), dim3(1024), 0, umhs_s(stream), rslabs, nrs, mp,
                     pl.pd_all, gp);
  UMHS_CHECK_LAUNCH();
  if (bc && bc->dE) {
    const int nchunks = (int)((bc->n_rays + MIX_CHUNK - 1) / MIX_CHUNK), CB = bc->C * bc->B;
    hipLaunchKernelGGL(field_mix_dE_kernel, dim3((unsigned)nchunks), dim3(256), 0, umhs_s(stream), (const float*)bc->part_ms,
                       (const float*)bc->mws16, bc->ray_of, bc->packed_info, n, bc->n_rays, bc->d_comp, bc->B, bc->C, bc->dE_part);
    hipLaunchKernelGGL(field_mix_dE_sum_kernel, dim3((unsigned)((CB + 63) / 64)), dim3(1024), 0, umhs_s(stream),
                       (const float*)bc->dE_part, nchunks, CB, bc->dE);
    UMHS_CHECK_LAUNCH();
  }
  return UMHS_OK;
}

static void launch_bwd_packs(const BwdPlan& pl, float* wT, float* img, float* bfimg, umhs_stream_t stream) {
  PackJob jb = {};
  jb.pd = pl.pd_all, jb.td = pl.td, jb.img = img, jb.wT = wT;
  int df[NLAYERS], dt[NTLAYERS], pr[2][2];
  build_bf_plan(pl, &jb.bp, df, dt, pr);
  if (jb.bp.total > 0) jb.bf = reinterpret_cast<uint32_t*>(bfimg);
  const int n = pl.pd_all.total + pl.td.total + jb.bp.total;
  hipLaunchKernelGGL(field_pack_all_kernel, dim3((n + 255) / 256), dim3(256), 0, umhs_s(stream), jb);
}

// The weight images of the backward (transposed packs + forward pack image) depend on the parameters only: a caller may build
// them ahead of time (e.g. on a side stream during the forward pass) and pass packs_ready = 1 to umhs_field_bwd with the SAME
// workspace.  The parameters must not change in between.
extern "C" int umhs_field_bwd_prepare(const umhs_field_cfg* cfg, const umhs_field_params* params, void* workspace,
                                      size_t workspace_bytes, umhs_stream_t stream) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cfg->density_only) return UMHS_ERR_UNSUPPORTED;
  if (!params) return UMHS_ERR_ARG;
  BwdPlan pl;
  rc = build_bwd_plan(cfg, params, &pl);
  if (rc) return rc;
  if (!workspace || workspace_bytes < bwd_workspace_need(pl, 1)) return UMHS_ERR_WORKSPACE;
  float* wT = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* img = wT + ((pl.td.total + 63) & ~63);
  float* bfimg = img + ((pl.pd_all.total + 63) & ~63);
  launch_bwd_packs(pl, wT, img, bfimg, stream);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" size_t umhs_field_bwd_workspace_bytes(const umhs_field_cfg* cfg, int64_t n) {
  if (check_cfg(cfg) || cfg->density_only || n <= 0) return 0;
  umhs_field_params dummy = {};
  const float one = 0.0f;
  const float** pp = reinterpret_cast<const float**>(&dummy);
  for (size_t i = 0; i < sizeof(dummy) / sizeof(float*); ++i) pp[i] = &one;  // layout only, never dereferenced
  BwdPlan pl;
  if (build_bwd_plan(cfg, &dummy, &pl)) return 0;
  return bwd_workspace_need(pl, n);
}

static int run_field_bwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc,
                         int64_t stride_n, int64_t stride_l, const float* world_pos, const float* directions,
                         const float* selector, const float* sigma_raw, const float* emb, const float* feat_logits,
                         int64_t n, const float* d_sigma, const float* d_spectral, const float* d_emb_ext, float* d_enc,
                         const umhs_field_grads* grads, void* workspace, size_t workspace_bytes, int packs_ready,
                         umhs_stream_t stream, BwdComp* bc) {
  int rc = check_cfg(cfg);
  if (rc) return rc;
  if (cfg->density_only) return UMHS_ERR_UNSUPPORTED;
  if (!params || !grads || n < 0 || (bc && bc->n_rays < 0)) return UMHS_ERR_ARG;
  // (n == 0: no per-sample array is read or written, and an empty torch tensor hands out NULL)
  if (n > 0 && (!enc || !selector || !world_pos || !sigma_raw || !emb || !feat_logits || !d_sigma || (!bc && !d_spectral)))
    return UMHS_ERR_ARG;
  if (bc && n > 0 && (!bc->sigma || !bc->t0 || !bc->t1 || !bc->weights || !bc->d_comp || !bc->packed_info || !bc->ray_of))
    return UMHS_ERR_ARG;
  const bool spec = cfg->pred_specular != 0;
  if (spec && n > 0 && !directions) return UMHS_ERR_ARG;
  if ((stride_n & 1) || (stride_l & 1) || ((uintptr_t)enc & 7) || ((uintptr_t)d_enc & 7)) return UMHS_ERR_ARG;
  BwdPlan pl;
  rc = build_bwd_plan(cfg, params, &pl);
  if (rc) return rc;
  GradPtrs gp;
  {
    float* const gw[NLAYERS] = {grads->base_w0, grads->base_w1, grads->head_w0, grads->head_w1, grads->head_w2,
                                grads->feat_w0, grads->feat_w1, grads->feat_w2, grads->dir_w0,  grads->dir_w1,
                                grads->endmembers};
    float* const gb[NLAYERS] = {grads->base_b0, grads->base_b1, grads->head_b0, grads->head_b1, grads->head_b2,
                                grads->feat_b0, grads->feat_b1, grads->feat_b2, grads->dir_b0,  grads->dir_b1,
                                nullptr};
    for (int l = 0; l < NLAYERS; ++l) gp.W[l] = gw[l], gp.b[l] = gb[l];
  }
  if (n == 0) {  // (no workspace needed: umhs_field_bwd_workspace_bytes is 0 here)
    hipLaunchKernelGGL(field_zero_grads_kernel, dim3(NLAYERS, 2), dim3(256), 0, umhs_s(stream), gp, pl.pd_all);
    UMHS_CHECK_LAUNCH();
    return UMHS_OK;
  }
  if (!workspace || workspace_bytes < bwd_workspace_need(pl, n)) return UMHS_ERR_WORKSPACE;
  // workspace: [transposed packs][forward pack image][bf16x3 images] (independent of n: umhs_field_bwd_prepare fills them) [slabs][d_bo]
  float* wT = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* img = wT + ((pl.td.total + 63) & ~63);
  float* bfimg = img + ((pl.pd_all.total + 63) & ~63);
  float* slabs = bfimg + ((bf_image_dwords(pl) + 63) & ~63);
  float* d_bo = slabs + ((bwd_slab_floats(pl, n) + 63) & ~(size_t)63);
  float* d_bo2 = d_bo + (((size_t)n * 16 + 63) & ~(size_t)63);
  float* d_fl = d_bo2 + (((size_t)n * 16 + 63) & ~(size_t)63);
  if (!packs_ready) {
    launch_bwd_packs(pl, wT, img, bfimg, stream);
    UMHS_CHECK_LAUNCH();
  }
  FieldIO io = {};
  io.enc = enc, io.sn = stride_n, io.sl = stride_l, io.wpos = world_pos, io.dirs = directions, io.sel = selector;
  io.n = n, io.B = cfg->n_bands, io.C = cfg->n_classes, io.TB = pl.TB, io.temperature = cfg->temperature;
  io.d_sigma = d_sigma, io.d_spectral = d_spectral, io.d_emb = d_emb_ext, io.d_enc = d_enc;
  io.emb_in = emb, io.sigma_raw_in = sigma_raw, io.d_bo = d_bo;
  // Two kernels (umhs_field_bwd needs the forward's feature logits: part 0 starts from them, part 1 from part 0's d_fl).  The chain runs
  // as three-piece bf16 products (the kernels of umhs_field_zip.h) wherever those hold their registers, else on the fp32 MFMA
  // (field_bwd_tf_kernel); UMHS_BWD_TF=1 (A/B knob) forces the fp32 chain everywhere.  (The LDS-staged kernels of round 1 -- 351 vs
  // 228 us at C2, 1454 vs 577 us at 128 bands -- were removed in round 3.)
  static const bool fp32_chain = getenv("UMHS_BWD_TF") && atoi(getenv("UMHS_BWD_TF")) == 1;
  const int tbmax = tf_tbmax(pl.TB);
  if (tbmax == 0) return UMHS_ERR_UNSUPPORTED;  // more than 256 bands
  {
    // bf16x3: part 1 always (part 0: up to 7 band tiles with the specular head, 8 in the folded form only -- its 8-tile per-sample kernel spills to scratch --
    // and any band count without it)
    const bool p0 = spec ? (tbmax < 8 || (tbmax == 8 && bc != nullptr)) : (tbmax < 16 || bc != nullptr);
    int bf_mask = fp32_chain ? 0 : (2 | (p0 ? 1 : 0));
    TfPart part[2];
    bool ok = true;
    for (int p = 0; p < 2; ++p) {
      if ((bf_mask >> p & 1) && !tf_part(pl, p, true, &part[p])) bf_mask &= ~(1 << p);  // LDS: fall back to the fp32 chain
      if (!(bf_mask >> p & 1)) ok = ok && tf_part(pl, p, false, &part[p]);
    }
    if (ok) {
      io.feat_logits_in = feat_logits, io.d_fl = d_fl;
      if (bc) {
        bc->dots = d_bo2;  // [N] of the (unused here) second hand-off buffer
        io.weights = bc->weights, io.ray_of = bc->ray_of, io.d_comp = bc->d_comp, io.dots = bc->dots;
        io.mix_g = bc->mix_g, io.part_ms = bc->part_ms, io.mws16 = bc->mws16;
        bc->E = params->endmembers, bc->dE = grads->endmembers, bc->B = cfg->n_bands, bc->C = cfg->n_classes;
        if (bc->emb16) io.bo16_in = emb;
        io.t0 = bc->grad_scaling ? bc->t0 : nullptr, io.t1 = bc->grad_scaling ? bc->t1 : nullptr;
      }
      switch (tbmax) {
        case 2: return launch_tf<2>(pl, part, bf_mask, io, spec, img, wT, bfimg, slabs, gp, n, stream, bc);
        case 4: return launch_tf<4>(pl, part, bf_mask, io, spec, img, wT, bfimg, slabs, gp, n, stream, bc);
        case 8: return launch_tf<8>(pl, part, bf_mask, io, spec, img, wT, bfimg, slabs, gp, n, stream, bc);
        case 12: return launch_tf<12>(pl, part, bf_mask, io, spec, img, wT, bfimg, slabs, gp, n, stream, bc);
        default: return launch_tf<16>(pl, part, bf_mask, io, spec, img, wT, bfimg, slabs, gp, n, stream, bc);
      }
    }
  }
  return UMHS_ERR_UNSUPPORTED;  // (a part whose weight images exceed the LDS in either arithmetic: no configuration check_cfg admits)
}

extern "C" int umhs_field_bwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc,
                              int64_t stride_n, int64_t stride_l, const float* world_pos, const float* directions,
                              const float* selector, const float* sigma_raw, const float* emb, const float* feat_logits,
                              int64_t n, const float* d_sigma, const float* d_spectral, const float* d_emb_ext, float* d_enc,
                              const umhs_field_grads* grads, void* workspace, size_t workspace_bytes, int packs_ready,
                              umhs_stream_t stream) {
  return run_field_bwd(cfg, params, enc, stride_n, stride_l, world_pos, directions, selector, sigma_raw, emb, feat_logits, n, d_sigma,
                       d_spectral, d_emb_ext, d_enc, grads, workspace, workspace_bytes, packs_ready, stream, nullptr);
}

// 1 when umhs_field_bwd_composited can serve this configuration (the transpose-free kernels with every pack LDS-resident).
extern "C" int umhs_field_bwd_composited_supported(const umhs_field_cfg* cfg) {
  if (check_cfg(cfg) || cfg->density_only) return 0;
  umhs_field_params dummy = {};
  const float zero = 0.0f;
  const float** pp = reinterpret_cast<const float**>(&dummy);
  for (size_t i = 0; i < sizeof(dummy) / sizeof(float*); ++i) pp[i] = &zero;  // layout only, never dereferenced
  BwdPlan pl;
  if (build_bwd_plan(cfg, &dummy, &pl) || tf_tbmax(pl.TB) == 0) return 0;
  TfPart part;
  return tf_part(pl, 0, false, &part) && tf_part(pl, 1, false, &part) ? 1 : 0;
}

extern "C" size_t umhs_field_bwd_composited_scratch_bytes(const umhs_field_cfg* cfg, int64_t n, int64_t n_rays) {
  if (check_cfg(cfg) || cfg->density_only || n < 0 || n_rays < 0) return 0;
  const size_t G = (size_t)((n + 15) / 16), chunks = (size_t)((n_rays + 31) / 32);
  return ((size_t)n_rays * 32 + G * 32 + chunks * cfg->n_classes * cfg->n_bands) * sizeof(float) + 256;
}

// umhs_field_bwd with the value half of the compositing backward folded in (training step after umhs_field_heads_fwd): instead of
// d_spectral [N,B] it takes the gradient of the per-ray band sums d_comp_spectral [R,B] (+ d_accumulation [R]) and what the
// renderer knows -- sigma, intervals, packed_info, ray_indices, weights -- and returns d_sigma [N] besides everything umhs_field_bwd
// returns.  Per sample: d_spectral[n][b] = scale_n weights[n] d_comp[ray(n)][b] on the fly; spectral[n][b] recomputed for
// dw_n = d_acc[r] + sum_b d_comp[r][b] spectral[n][b]; umhs_composite_bwd_dots; then the density half of the field backward.
// Neither spectral nor d_spectral exists as an [N,B] array.  feat_logits is required.
extern "C" int umhs_field_bwd_composited(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc,
                                         int64_t stride_n, int64_t stride_l, const float* world_pos, const float* directions,
                                         const float* selector, const float* sigma_raw, const float* emb, int emb_stride,
                                         const float* feat_logits, int64_t n, const float* sigma, const float* t_starts, const float* t_ends,
                                         const int64_t* packed_info, int64_t n_rays, const int64_t* ray_indices, const float* weights,
                                         const float* d_comp_spectral, const float* d_accumulation, int grad_scaling, float* d_sigma,
                                         float* d_enc, const umhs_field_grads* grads, void* scratch, size_t scratch_bytes,
                                         void* workspace, size_t workspace_bytes, int packs_ready, umhs_stream_t stream) {
  if (!cfg || n < 0 || n_rays < 0 || !scratch || ((uintptr_t)scratch & 15)) return UMHS_ERR_ARG;
  if (scratch_bytes < umhs_field_bwd_composited_scratch_bytes(cfg, n, n_rays)) return UMHS_ERR_WORKSPACE;
  BwdComp bc = {};
  {
    float* sc = reinterpret_cast<float*>(scratch);
    const size_t G = (size_t)((n + 15) / 16);
    bc.mix_g = sc, bc.part_ms = bc.mix_g + (size_t)n_rays * 16, bc.mws16 = bc.part_ms + G * 2 * 16;
    bc.dE_part = bc.mws16 + (size_t)n_rays * 16;
  }
  bc.sigma = sigma, bc.t0 = t_starts, bc.t1 = t_ends, bc.weights = weights, bc.d_comp = d_comp_spectral, bc.d_acc = d_accumulation;
  bc.packed_info = packed_info, bc.ray_of = ray_indices, bc.n_rays = n_rays, bc.grad_scaling = grad_scaling, bc.d_sigma = d_sigma;
  if ((emb_stride != 15 && emb_stride != 16) || (emb_stride == 16 && ((uintptr_t)emb & 15))) return UMHS_ERR_ARG;
  bc.emb16 = emb_stride == 16;
  return run_field_bwd(cfg, params, enc, stride_n, stride_l, world_pos, directions, selector, sigma_raw, emb, feat_logits, n, d_sigma,
                       nullptr, nullptr, d_enc, grads, workspace, workspace_bytes, packs_ready, stream, &bc);
}
