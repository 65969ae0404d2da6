/*
 * umhs_hip.h -- C ABI of libumhs_hip.so: the MI355X (gfx950) implementation of the UMHS
 * volumetric-rendering hot path (hash-grid encode, density/spectral MLPs + endmember mixing,
 * per-ray alpha compositing over B bands, spectrum->sRGB, fused Adam).
 *
 * The reference (Factral/unsupervised-hyperspectral-nerf) has no C ABI: its boundary is the
 * nerfstudio plugin API in Python, and the native code it reaches lives in tiny-cuda-nn / nerfacc.
 * This header sits where those libraries' Python bindings used to sit; each entry point cites the
 * reference call site (file:line relative to the reference repo) it replaces.  The Python mirror of
 * the plugin surface (UMHSField, SpectralRenderer, ColourSystem, UMHSModel ...) binds these symbols
 * with ctypes -- see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns UMHS_OK (0) or a negative error code (umhs_strerror), never throws;
 *   - never allocates, never synchronises the stream; workspaces are caller-provided and sized by
 *     the matching *_workspace_bytes query;
 *   - all pointers are DEVICE pointers to contiguous row-major fp32 unless stated (int64 for
 *     ray_indices / packed_info, exactly the dtypes nerfacc hands out);
 *   - `stream` is a hipStream_t (NULL = default stream); calls are re-entrant on distinct streams;
 *   - no torch types anywhere in the signatures.
 */
#ifndef UMHS_HIP_H
#define UMHS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UMHS_ABI_VERSION 11

enum {
  UMHS_OK = 0,
  UMHS_ERR_ARG = -1,         /* NULL / negative / inconsistent argument            */
  UMHS_ERR_UNSUPPORTED = -2, /* shape outside what the gfx950 kernels are built for */
  UMHS_ERR_WORKSPACE = -3,   /* workspace missing or too small                     */
  UMHS_ERR_LAUNCH = -4       /* hipGetLastError() != hipSuccess after a launch      */
};

typedef void* umhs_stream_t; /* hipStream_t */

const char* umhs_strerror(int code);
int umhs_abi_version(void);

/* ------------------------------------------------------------------------------------------ */
/* R1 (prefix): sample positions.  Replaces Frustums.get_positions + SceneContraction(L-inf) +  */
/* (p+2)/4 + in-box selector of UMHSField.get_density, umhs_field.py:302-310.                   */
/* Either (origins,directions,starts,ends) [N,3],[N,3],[N],[N] or world_pos_in [N,3] is given   */
/* (the latter is the density_fn(positions) path used by the occupancy grid,                    */
/* umhs_model.py:208,553).  contraction != 0 -> L-inf contraction then (p+2)/4;                 */
/* contraction == 0 -> (p - aabb_min)/(aabb_max-aabb_min) with aabb = 6 HOST floats.            */
/* Outputs: world_pos_out [N,3] (optional), pos01_out [N,3] (already multiplied by selector),   */
/* selector_out [N] (1.0f / 0.0f).                                                              */
/* ------------------------------------------------------------------------------------------ */
int umhs_positions_fwd(const float* origins, const float* directions, const float* starts, const float* ends,
                       const float* world_pos_in, int64_t n, int contraction, const float* aabb_host6,
                       float* world_pos_out, float* pos01_out, float* selector_out, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* R2: multiresolution hash-grid encode.  Replaces nerfstudio HashEncoding.forward (torch path) */
/* / tcnn HashGrid reached through self.mlp_base(positions_flat), umhs_field.py:320.            */
/* pos01 [N,3]; table [L*T, 2]; scalings [L] (device, = floor(16*g^l) as float32);              */
/* enc element (n,l,f) is written at enc[n*stride_n + l*stride_l + f] (f in {0,1}):             */
/*   stride_n=2L, stride_l=2  -> the reference's [N, L*F] layout;                               */
/*   stride_n=2,  stride_l=2N -> level-major [L][N][2] (what the fused field kernels prefer).   */
/* hashgrid_bwd: overwrite == 0 ACCUMULATES (d_table[idx] += w_corner * d_enc, caller zeroes   */
/* it); overwrite != 0 writes the whole [L*T,2] gradient (no memset / read-modify-write needed).*/
/* With a workspace (umhs_hashgrid_bwd_workspace_bytes; 0 = not available for this shape) the   */
/* scatter is atomics-free (radix partition into LDS-sized slot buckets); with workspace ==     */
/* NULL it falls back to global float atomics (no workspace, ~20x slower at N = 262k).          */
/* ------------------------------------------------------------------------------------------ */
int umhs_hashgrid_fwd(const float* pos01, const float* table, const float* scalings, int64_t n, int n_levels,
                      int log2_table_size, float* enc, int64_t stride_n, int64_t stride_l, umhs_stream_t stream);
/* Level-major feature compaction enc_out[l][i] = enc_in[l][index[i]] ([L][M][2] -> [L][N][2]): lets a caller that has already  */
/* encoded a superset of the samples (the sampler's density query) reuse those features instead of encoding the survivors again.  */
int umhs_enc_gather(const float* enc_in, const int64_t* index, int64_t m, int64_t n, int n_levels, float* enc_out,
                    umhs_stream_t stream);
size_t umhs_hashgrid_bwd_workspace_bytes(int64_t n, int n_levels, int log2_table_size);
/* Levels [level_begin, level_begin + n_levels) are processed (d_enc / d_table / scalings are indexed with the     */
/* absolute level): callers may run the backward per level group, e.g. to all-reduce finished slabs early.          */
int umhs_hashgrid_bwd(const float* pos01, const float* d_enc, int64_t stride_n, int64_t stride_l,
                      const float* scalings, int64_t n, int level_begin, int n_levels, int log2_table_size,
                      float* d_table, int overwrite, void* workspace, size_t workspace_bytes, umhs_stream_t stream);
/* The partitioned backward in two halves.  prepare: bucket histogram + scan, from the positions alone (may run on a side   */
/* stream while the forward pass is in flight).  apply: scatter + per-bucket reduction of levels [level_begin, +n_levels),  */

/* umhs_hashgrid_fwd for the workspace's level range [0, n_levels) AND the histogram pass of umhs_hashgrid_bwd_prepare for the same   */
/* positions, in one launch (the gather has hashed every (sample, level) anyway and leaves the vector ALU idle);                     */
/* umhs_hashgrid_bwd_prepare_counted then runs only the two small scans.  Together they equal umhs_hashgrid_fwd +                    */
/* umhs_hashgrid_bwd_prepare(level_begin 0) bit for bit.  workspace: umhs_hashgrid_bwd_workspace_bytes(n, n_levels, log2_T).          */
int umhs_hashgrid_fwd_count(const float* pos01, const float* table, const float* scalings, int64_t n, int n_levels, int log2_T,
                            float* enc, int64_t stride_n, int64_t stride_l, void* workspace, size_t workspace_bytes,
                            umhs_stream_t stream);
int umhs_hashgrid_bwd_prepare_counted(const float* pos01, const float* scalings, int64_t n, int n_levels, int log2_T, void* workspace,
                                      size_t workspace_bytes, umhs_stream_t stream);

/* a sub-range of the prepared [ws_level_begin, +ws_n_levels) in the same workspace; each level once per prepare.          */
int umhs_hashgrid_bwd_prepare(const float* pos01, const float* scalings, int64_t n, int level_begin, int n_levels, int log2_T,
                              void* workspace, size_t workspace_bytes, umhs_stream_t stream);
int umhs_hashgrid_bwd_apply(const float* pos01, const float* d_enc, int64_t stride_n, int64_t stride_l, const float* scalings,
                            int64_t n, int level_begin, int n_levels, int ws_level_begin, int ws_n_levels, int log2_T,
                            float* d_table, int overwrite, void* workspace, size_t workspace_bytes, umhs_stream_t stream);
/* umhs_hashgrid_bwd_apply in overwrite mode + the Adam step (umhs_adam_step arithmetic, grad_scale 1) of the table entries of    */
/* levels >= adam_level_begin, executed in the epilogue of the bucket reduce where their gradient is final.  For a single-GPU      */
/* trainer whose optimizer.step() follows the backward (UMHSAdam skips the range it is told was done): the HBM-bound update hides   */
/* inside the LDS-bound reduce and the gradient is not read back.  d_table still receives the gradient.  n > 0.                     */
int umhs_hashgrid_bwd_apply_adam(const float* pos01, const float* d_enc, int64_t stride_n, int64_t stride_l,
                                 const float* scalings, int64_t n, int level_begin, int n_levels, int ws_level_begin,
                                 int ws_n_levels, int log2_T, float* d_table, void* workspace, size_t workspace_bytes,
                                 float* table_params, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                                 float eps, int64_t step, int adam_level_begin, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* R3-R9, R18: fused per-sample field.  Replaces mlp_base's MLP, NeRFEncoding, SHEncoding,      */
/* mlp_head, feature_mlp, mlp_directional, softmax/sigmoid and the [N,B,C] endmember mixing of  */
/* UMHSField.get_density / get_outputs, umhs_field.py:160-261,320-328 (tcnn.Network /           */
/* nerfstudio MLP call sites :211,:219,:250).                                                   */
/* Weights are the reference's nn.Linear tensors as they sit in the state dict: W [out,in]      */
/* row-major, b [out].  hidden = 64, geo_feat_dim = 15, 16 hash levels x 2 features are fixed   */
/* (NerfactoField defaults); n_classes <= 15, n_bands <= 256.                                   */
/* ------------------------------------------------------------------------------------------ */
typedef struct umhs_field_cfg {
  int32_t n_bands;       /* B: wavelengths                                   */
  int32_t n_classes;     /* C: endmembers ("num_classes")                    */
  int32_t pred_specular; /* 1: feature_mlp has C+1 outputs, mlp_directional used */
  int32_t density_only;  /* 1: hash features -> sigma, emb only (density_fn)  */
  float temperature;     /* softmax(logits / temperature), umhs_field.py:226  */
} umhs_field_cfg;

typedef struct umhs_field_params {
  const float *base_w0, *base_b0, *base_w1, *base_b1;                       /* 32->64->16            */
  const float *head_w0, *head_b0, *head_w1, *head_b1, *head_w2, *head_b2;   /* 27->64->64->C         */
  const float *feat_w0, *feat_b0, *feat_w1, *feat_b1, *feat_w2, *feat_b2;   /* 27->64->64->C(+1)     */
  const float *dir_w0, *dir_b0, *dir_w1, *dir_b1;                           /* 28->16->B (specular)  */
  const float* endmembers;                                                  /* [C,B]                 */
} umhs_field_params;

typedef struct umhs_field_grads {
  float *base_w0, *base_b0, *base_w1, *base_b1;
  float *head_w0, *head_b0, *head_w1, *head_b1, *head_w2, *head_b2;
  float *feat_w0, *feat_b0, *feat_w1, *feat_b1, *feat_w2, *feat_b2;
  float *dir_w0, *dir_b0, *dir_w1, *dir_b1;
  float* endmembers;
} umhs_field_grads;

/* Forward.  enc is addressed with (stride_n, stride_l) as above.  world_pos [N,3] (raw, for the */
/* NeRF positional encoding, umhs_field.py:183-184), directions [N,3] (raw; (d+1)/2 applied     */
/* inside, :160), selector [N].  Outputs (any may be NULL except sigma):                        */
/*   sigma [N] = trunc_exp(raw)*selector (:327-328); sigma_raw [N]; emb [N,15];                 */
/*   spectral [N,B] (= spec + s1*specular when pred_specular, else spec), spectral2 [N,B] (spec),*/
/*   specular [N,B] (s1*specular), abundances [N,C].                                            */
/* workspace (optional, umhs_field_fwd_workspace_bytes): room for the packed weight image built once per call;   */
/* with workspace == NULL every workgroup gathers the image itself (~60 us slower per launch).                   */
size_t umhs_field_fwd_workspace_bytes(const umhs_field_cfg* cfg);
int umhs_field_fwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc, int64_t stride_n,
                   int64_t stride_l, const float* world_pos, const float* directions, const float* selector,
                   int64_t n, float* sigma, float* sigma_raw, float* emb, float* spectral, float* spectral2,
                   float* specular, float* abundances, float* feat_logits, void* workspace, size_t workspace_bytes,
                   int pack_ready, umhs_stream_t stream);
/* density_fn (SURVEY 8a R1-R3 for the sampler / occupancy-grid callers, umhs_model.py:208,553) = umhs_hashgrid_fwd followed by   */
/* umhs_field_fwd with cfg->density_only.  (A one-launch form with the gather inside the MLP kernel existed up to ABI 7: it took  */
/* as long as the two launches -- both are bound by the gather's L2 request rate -- and spilled registers; removed.)              */
/* The training step's forward as two launches with the rendering weights known in between (umhs_model.py:239-327: field ->    */
/* renderers; here the per-ray band sums of the [N,B] outputs are formed inside the heads kernel, so spectral2 / specular --     */
/* which carry no loss, umhs_model.py:373-374 -- never exist per sample):                                                        */
/*   umhs_field_base_fwd : mlp_base only (sigma, sigma_raw, emb as umhs_field_fwd writes them) from the FULL configuration's      */
/*                         workspace (umhs_field_fwd_workspace_bytes / umhs_field_fwd_prepare: one set of pack images for both).  */
/*   umhs_composite_fwd with no value streams: weights, accumulation, depth.                                                     */
/*   umhs_field_heads_fwd: everything after mlp_base from emb [N,15]; comp_*[r][b] = sum_{n in ray r} weights[n] stream[n][b]    */
/*                         (SpectralRenderer, renderers.py:18-53) for spectral / spectral2 / specular ([R,B]; the last two NULL   */
/*                         without the specular head), abundances, feat_logits [N,16]; no [N,B] array is ever written.            */
/*                         ray_indices [N] non-decreasing; packed_info [R,2] as umhs_pack_info.  The sums are taken in a          */
/*                         fixed order (per 16-sample tile, then tile by tile): same bits every run.                             */
int umhs_field_base_fwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc, int64_t stride_n,
                        int64_t stride_l, const float* selector, int64_t n, float* sigma, float* sigma_raw, float* emb,
                        float* base16, void* workspace, size_t workspace_bytes, int pack_ready, umhs_stream_t stream);
size_t umhs_field_heads_fwd_scratch_bytes(const umhs_field_cfg* cfg, int64_t n, int64_t n_rays);
/* 1 when the two-launch forward can serve this configuration (else both entries return UMHS_ERR_UNSUPPORTED and the caller keeps   */
/* umhs_field_fwd + umhs_composite_fwd, which serve every configuration check_cfg admits).                                          */
int umhs_field_heads_fwd_supported(const umhs_field_cfg* cfg);
/* emb / base16: the base MLP's outputs either as the reference's [N,15] embedding (emb, emb_stride 15; any of emb / base16 may be    */
/* NULL in umhs_field_base_fwd) or as aligned rows base16 [N,16] with sigma_raw in slot 0 (emb_stride 16: one 64-byte row per sample  */
/* instead of 15 dword stores / loads).  The mixing term is linear in the mixing input m: the kernel sums w_n m_n (16 classes) per   */
/* ray and the finish pass multiplies by the endmembers once per RAY; only the specular term is formed per sample and band.          */
/* comp_spectral2 / comp_specular: required with the specular head, ignored without.  comp_abundances [R,C], abundances [N,C],      */
/* feat_logits [N,16]: optional.  scratch: umhs_field_heads_fwd_scratch_bytes, 16-byte aligned.                                      */
int umhs_field_heads_fwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* emb, int emb_stride,
                         const float* world_pos, const float* directions, int64_t n, const float* weights,
                         const int64_t* ray_indices, const int64_t* packed_info, int64_t n_rays, float* abundances,
                         float* feat_logits, float* comp_spectral, float* comp_spectral2, float* comp_specular,
                         float* comp_abundances, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes,
                         int pack_ready, umhs_stream_t stream);
/* feat_logits ([N,16]): the feature_mlp logits, saved because umhs_field_bwd runs its heads as two kernels (head MLP +    */
/* directional + mixing / feature MLP + mlp_base), the second one starting from the logits.  Optional in the forward,       */
/* REQUIRED by umhs_field_bwd (NULL there: UMHS_ERR_ARG; there is no single-kernel backward any more, ABI 7).                */
/* builds the pack image ahead of time (parameters only): then pass pack_ready = 1 with the same workspace */
int umhs_field_fwd_prepare(const umhs_field_cfg* cfg, const umhs_field_params* params, void* workspace,
                           size_t workspace_bytes, umhs_stream_t stream);

/* Backward.  Recomputes the activations per tile; the only saved forward tensors are enc, sigma_raw [N],       */
/* emb [N,15] and feat_logits [N,16] (all outputs of umhs_field_fwd).  d_sigma [N] and d_spectral [N,B] are the gradients w.r.t. the   */
/* forward's sigma / spectral outputs; d_emb_ext [N,15] (optional) is an extra gradient on emb.  Writes d_enc     */
/* (same strides as enc) and the parameter gradients (OVERWRITTEN, not accumulated; zeros when n == 0, where the  */
/* per-sample pointers may be NULL).                                                                             */
/* workspace: umhs_field_bwd_workspace_bytes.                                                                    */
size_t umhs_field_bwd_workspace_bytes(const umhs_field_cfg* cfg, int64_t n);
int umhs_field_bwd(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc, int64_t stride_n,
                   int64_t stride_l, const float* world_pos, const float* directions, const float* selector,
                   const float* sigma_raw, const float* emb, const float* feat_logits, int64_t n, const float* d_sigma,
                   const float* d_spectral, const float* d_emb_ext, float* d_enc, const umhs_field_grads* grads,
                   void* workspace, size_t workspace_bytes, int packs_ready, umhs_stream_t stream);
/* umhs_field_bwd with the value half of the compositing backward (nerfacc accumulate_along_rays backward through               */
/* SpectralRenderer, umhs_renderer.py:28-30) folded in -- the training step after umhs_field_heads_fwd.  Takes d_comp_spectral       */
/* [R,B] (gradient of the per-ray band sums) + d_accumulation [R] and the renderer's sigma / intervals / packed_info /              */
/* ray_indices / weights instead of d_spectral [N,B]; returns d_sigma [N] as well.  Per sample d_spectral = scale_n weights[n]      */
/* d_comp[ray(n)] is formed on the fly and spectral is recomputed for dw_n: neither exists as an [N,B] array.  feat_logits          */
/* required.  umhs_field_bwd_composited_supported: 1 when this configuration can take the path (else UMHS_ERR_UNSUPPORTED).         */
int umhs_field_bwd_composited_supported(const umhs_field_cfg* cfg);
size_t umhs_field_bwd_composited_scratch_bytes(const umhs_field_cfg* cfg, int64_t n, int64_t n_rays);
int umhs_field_bwd_composited(const umhs_field_cfg* cfg, const umhs_field_params* params, const float* enc, int64_t stride_n,
                              int64_t stride_l, const float* world_pos, const float* directions, const float* selector,
                              const float* sigma_raw, const float* emb, int emb_stride, const float* feat_logits, int64_t n,
                              const float* sigma,
                              const float* t_starts, const float* t_ends, const int64_t* packed_info, int64_t n_rays,
                              const int64_t* ray_indices, const float* weights, const float* d_comp_spectral,
                              const float* d_accumulation, int grad_scaling, float* d_sigma, float* d_enc,
                              const umhs_field_grads* grads, void* scratch, size_t scratch_bytes, void* workspace,
                              size_t workspace_bytes, int packs_ready, umhs_stream_t stream);
/* builds the transposed packs + forward image ahead of time (parameters only): then pass packs_ready = 1, same workspace */
int umhs_field_bwd_prepare(const umhs_field_cfg* cfg, const umhs_field_params* params, void* workspace,
                           size_t workspace_bytes, umhs_stream_t stream);

/* ---- method="rgb" (the reference's default method, umhs_field.py:280-294 = nerfstudio NerfactoField; BASELINE configs[0]) ---------- */
/* The two MLPs of the rgb field as gfx950 kernels (exact fp32 MFMA), replacing the torch.nn.functional.linear calls of rounds 1-3.     */
/*   base: hash features enc [N,32] (sample-major) -> 64 ReLU -> 16: density = trunc_exp(out0) * selector (selector NULL: 1),           */
/*         emb = out1..15 [N,15] (NULL: not written), sigma_raw = out0 [N] (NULL: not written)        -- mlp_base, umhs_field.py:51,320-327 */
/*   head: [SHEncoding(levels=4)((directions + 1) / 2) | emb15] -> 64 ReLU -> 64 ReLU -> 3, Sigmoid -> rgb [N,3]   -- NerfactoField.mlp_head */
/* Weights in torch.nn.Linear layout ([out][in] row-major, bias [out]).  The backward entries recompute the forward, write the input     */
/* gradient (d_enc [N,32] / d_emb [N,15]) and the parameter gradients (accumulate != 0: += ), bitwise reproducibly; workspace:           */
/* umhs_rgb_mlp_bwd_workspace_bytes(head, n), 16-byte aligned.  n == 0: no-op.                                                          */
size_t umhs_rgb_mlp_bwd_workspace_bytes(int head, int64_t n);
int umhs_rgb_base_fwd(const float* enc, const float* selector, const float* w0, const float* b0, const float* w1, const float* b1,
                      int64_t n, float* density, float* emb, float* sigma_raw, umhs_stream_t stream);
int umhs_rgb_head_fwd(const float* directions, const float* emb, const float* w0, const float* b0, const float* w1, const float* b1,
                      const float* w2, const float* b2, int64_t n, float* rgb, umhs_stream_t stream);
int umhs_rgb_base_bwd(const float* enc, const float* selector, const float* w0, const float* b0, const float* w1, const float* b1,
                      const float* d_density, const float* d_emb, int64_t n, float* d_enc, float* d_w0, float* d_b0, float* d_w1,
                      float* d_b1, int accumulate, void* workspace, size_t workspace_bytes, umhs_stream_t stream);
int umhs_rgb_head_bwd(const float* directions, const float* emb, const float* w0, const float* b0, const float* w1, const float* b1,
                      const float* w2, const float* b2, const float* d_rgb, int64_t n, float* d_emb, float* d_w0, float* d_b0,
                      float* d_w1, float* d_b1, float* d_w2, float* d_b2, int accumulate, void* workspace, size_t workspace_bytes,
                      umhs_stream_t stream);


/* ------------------------------------------------------------------------------------------ */
/* R11: packed transmittance/weights.  Replaces nerfacc.pack_info + render_weight_from_density, */
/* umhs_model.py:245-252 (dense twin: get_weights_spectral, umhs_renderer.py:117-139).          */
/* R12/R13: per-ray accumulation.  Replaces nerfacc.accumulate_along_rays behind                */
/* SpectralRenderer.forward (umhs_renderer.py:28-30) and nerfstudio's Accumulation/Depth        */
/* renderers (umhs_model.py:254-258).  ray_indices must be sorted ascending (nerfacc invariant). */
/* ------------------------------------------------------------------------------------------ */
int umhs_pack_info(const int64_t* ray_indices, int64_t n, int64_t n_rays, int64_t* packed_info, umhs_stream_t stream);

#define UMHS_MAX_STREAMS 4
typedef struct umhs_value_streams {
  int32_t n_streams;                     /* 0..4 value tensors composited with the same weights */
  int32_t k[UMHS_MAX_STREAMS];           /* channels of each [N,k] tensor                       */
  const float* values[UMHS_MAX_STREAMS]; /* [N,k]                                               */
  float* out[UMHS_MAX_STREAMS];          /* [R,k]                                               */
} umhs_value_streams;

/* weights [N] (out), accumulation [R] (out, optional), depth [R] (out, optional: sum w*t_mid /  */
/* (acc+1e-10), NOT yet clipped to [min t_mid, max t_mid] -- that global clip is the caller's).  */
int umhs_composite_fwd(const float* sigma, const float* t_starts, const float* t_ends, const int64_t* packed_info,
                       int64_t n_rays, int64_t n, const umhs_value_streams* streams, float* weights,
                       float* accumulation, float* depth, umhs_stream_t stream);

typedef struct umhs_value_grads {
  int32_t n_streams;
  int32_t k[UMHS_MAX_STREAMS];
  const float* values[UMHS_MAX_STREAMS]; /* [N,k] forward inputs                    */
  const float* d_out[UMHS_MAX_STREAMS];  /* [R,k] gradient of the composited output */
  float* d_values[UMHS_MAX_STREAMS];     /* [N,k] (out)                             */
} umhs_value_grads;

/* d_accumulation [R] optional.  grad_scaling != 0 multiplies d_sigma and d_values by              */
/* clamp(((t0+t1)/2)^2, 0, 1) (scale_gradients_by_distance_squared, umhs_model.py:241-242).        */
int umhs_composite_bwd(const float* sigma, const float* t_starts, const float* t_ends, const int64_t* packed_info,
                       int64_t n_rays, int64_t n, const float* weights, const umhs_value_grads* grads,
                       const float* d_accumulation, int grad_scaling, float* d_sigma, umhs_stream_t stream);
/* The density half alone, for a caller that has already formed dots[n] = sum over streams and bands of d_out[ray(n)][k] *    */
/* value[n][k] itself (umhs_field_bwd_composited does): d_sigma only, no [N,k] array read or written.                           */
int umhs_composite_bwd_dots(const float* sigma, const float* t_starts, const float* t_ends, const int64_t* packed_info,
                            int64_t n_rays, int64_t n, const float* weights, const float* dots, const float* d_accumulation,
                            int grad_scaling, float* d_sigma, umhs_stream_t stream);

/* R12 stand-alone: accumulate with caller-provided weights [N] -- SpectralRenderer.forward(spectral, weights,  */
/* ray_indices, num_rays) called on its own (umhs_renderer.py:15-30; dino / abundance renders,                  */
/* umhs_model.py:299-317).  out[r,:] = sum_n w[n] v[n,:];  bwd: d_weights[n] = sum_k d_out[r,k] v[n,k] (rays     */
/* with no samples leave their d_weights untouched: caller zero-fills), d_values[n,:] = w[n] d_out[r,:].         */
int umhs_accumulate_fwd(const float* weights, const int64_t* packed_info, int64_t n_rays, int64_t n,
                        const umhs_value_streams* streams, umhs_stream_t stream);
int umhs_accumulate_bwd(const float* weights, const int64_t* packed_info, int64_t n_rays, int64_t n,
                        const umhs_value_grads* grads, float* d_weights, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* R14: spectrum -> sRGB.  Replaces ColourSystem.forward, utils/spec_to_rgb.py:103-127:         */
/* rgb = clamp(gamma(spec @ M), 0, 1), M [B,3].  bwd writes d_spec [R,B] (accumulate != 0: +=). */
/* ------------------------------------------------------------------------------------------ */
int umhs_spec2rgb_fwd(const float* spec, const float* M, int64_t n_rays, int n_bands, float* rgb, umhs_stream_t stream);
int umhs_spec2rgb_bwd(const float* spec, const float* M, const float* d_rgb, int64_t n_rays, int n_bands,
                      float* d_spec, int accumulate, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* R13/R15/R16 fused per-ray epilogue + losses (the ~85 tiny torch kernels of umhs_model.py:254-313,358-370).     */
/* umhs_tmid_minmax: min / max over all samples of (t0+t1)/2 -- DepthRenderer's clip bounds (global over the      */
/*   batch); minmax2 = 2 device words in an order-preserving encoding consumed by umhs_ray_epilogue_fwd only.     */
/* umhs_ray_epilogue_fwd: rgb = ColourSystem(spectral) (spec_to_rgb.py:112-127); depth_clipped; seg_probs =       */
/*   softmax(alpha * cos(spectral, endmembers)) (clusterprobe.py:17-38, alpha = 0.2 at umhs_model.py:307);        */
/*   seg_raw = argmax * [acc > 0.5]; seg_pred = class_colors[argmax] * [acc > 0.5] (:308-313).  Any output NULL   */
/*   = skipped.  n_classes <= 16.  Gradient flows through rgb only (umhs_spec2rgb_bwd).                           */
/* umhs_loss_fwd: losses2[0] = w_spectral * MSE(spectral, gt_spectral); losses2[1] = w_rgb * MSE(rgb +           */
/*   background*(1-acc), gt_rgb) (rgb == NULL: skipped).  umhs_loss_bwd: their gradients scaled by the upstream    */
/*   gradients grad_losses2 (device [2], NULL = 1).                                                               */
/* ------------------------------------------------------------------------------------------ */
int umhs_tmid_minmax(const float* t_starts, const float* t_ends, int64_t n, float* minmax2, umhs_stream_t stream);
int umhs_ray_epilogue_fwd(const float* spectral, const float* M, const float* endmembers, const float* accumulation,
                          const float* depth, const float* tmid_minmax2, const float* class_colors, int64_t n_rays,
                          int n_bands, int n_classes, float alpha, float* rgb, float* depth_clipped, float* seg_probs,
                          float* seg_raw, float* seg_pred, umhs_stream_t stream);
int umhs_loss_fwd(const float* spectral, const float* gt_spectral, const float* rgb, const float* accumulation,
                  const float* background, const float* gt_rgb, int64_t n_rays, int n_bands, float w_spectral, float w_rgb,
                  float* losses2, umhs_stream_t stream);
int umhs_loss_bwd(const float* spectral, const float* gt_spectral, const float* rgb, const float* accumulation,
                  const float* background, const float* gt_rgb, int64_t n_rays, int n_bands, float w_spectral, float w_rgb,
                  const float* grad_losses2, float* d_spectral, float* d_rgb, float* d_accumulation, umhs_stream_t stream);

/* umhs_ray_train_tail: the per-ray tail of a TRAINING step in one launch = umhs_ray_epilogue_fwd + umhs_loss_fwd +      */
/*   umhs_loss_bwd with unit upstream gradients + umhs_spec2rgb_bwd accumulated into d_spectral (umhs_model.py:254-313,   */
/*   358-370 and their autograd).  rgb_loss = 0: method "spectral" (no rgb term, d_accumulation unused).  scratch:        */
/*   umhs_ray_train_tail_scratch_bytes() bytes, ZERO before the first call (the kernel leaves it zeroed again).          */
size_t umhs_ray_train_tail_scratch_bytes(void);
int umhs_ray_train_tail(const float* spectral, const float* M, const float* endmembers, const float* accumulation,
                        const float* depth, const float* tmid_minmax2, const float* class_colors, const float* gt_spectral,
                        const float* gt_rgb, const float* background, int64_t n_rays, int n_bands, int n_classes, float alpha,
                        float w_spectral, float w_rgb, int rgb_loss, float* rgb, float* depth_clipped, float* seg_probs,
                        float* seg_raw, float* seg_pred, float* losses2, float* d_spectral, float* d_accumulation,
                        void* scratch, size_t scratch_bytes, umhs_stream_t stream);
/* ------------------------------------------------------------------------------------------ */
/* occupancy-grid ray marcher.  Replaces nerfacc.OccGridEstimator.sampling (traverse_grids +        */
/* render_visibility_from_density, CUDA only) behind nerfstudio's VolumetricSampler, umhs_model.py:201-209,229-237. */
/* binaries: uint8 [levels][res][res][res] (x-major); level l covers the roi enlarged 2^l about its centre;          */
/* roi_aabb_host6 = 6 HOST floats (min xyz, max xyz).  Samples have size dt = max(t*cone_angle, step_size) and are   */
/* emitted while their mid-point lies in an occupied voxel; a run restarts at the voxel entry after empty space.     */
/* nears / fars: optional per-ray planes [R] (stratified jitter, collider).                                          */
/* umhs_march_walk (optional, in front of the entry points below): the voxel sequence of every ray -- pure geometry, it never     */
/* looks at the occupancy -- with one WAVE per ray: lane j starts somewhere inside the ray's range, falls onto the sequential       */
/* walk at its first voxel face and must land exactly on lane j+1's start (else the window ends there), so the lists are the        */
/* one-thread-per-ray walk bit for bit (occupied voxels only).  `walked`: umhs_march_walk_workspace_bytes(n_rays) bytes (4.6 KB per ray); pass it to*/
/* count / write / scratch, which then only replay it (walked == NULL: they walk the grid themselves, one thread per ray).          */
/* Two passes: umhs_march_count -> counts [R] (caller scans them into packed_info), umhs_march_write -> packed        */
/* t_starts / t_ends [N] fp32 and ray_indices [N] int64.  umhs_visibility: mask[n] = T_n >= early_stop_eps &&         */
/* (alpha_thre <= 0 || alpha_n >= alpha_thre) with sigma from the density-only field forward.                        */
/* ------------------------------------------------------------------------------------------ */
size_t umhs_march_walk_workspace_bytes(int64_t n_rays);
int umhs_march_walk(const float* origins, const float* directions, int64_t n_rays, const uint8_t* binaries,
                    const float* roi_aabb_host6, int levels, int resolution, float near_plane, float far_plane, const float* nears,
                    const float* fars, const float* jitter, float jitter_step, void* walked, size_t walked_bytes,
                    umhs_stream_t stream);
int umhs_march_count(const float* origins, const float* directions, int64_t n_rays, const uint8_t* binaries,
                     const float* roi_aabb_host6, int levels, int resolution, float near_plane, float far_plane,
                     float step_size, float cone_angle, const float* nears, const float* fars, const float* jitter,
                     float jitter_step, int64_t* counts, const void* walked, size_t walked_bytes, umhs_stream_t stream);
int umhs_march_write(const float* origins, const float* directions, int64_t n_rays, const uint8_t* binaries,
                     const float* roi_aabb_host6, int levels, int resolution, float near_plane, float far_plane,
                     float step_size, float cone_angle, const float* nears, const float* fars, const float* jitter,
                     float jitter_step, const int64_t* packed_info, float* t_starts, float* t_ends, int64_t* ray_indices,
                     const void* walked, size_t walked_bytes, umhs_stream_t stream);
/* Single pass instead of count + write: umhs_march_scratch counts AND parks the first `cap` samples of ray r in             */
/* scratch_t0/t1[r*cap + i]; after the caller's scan, umhs_march_compact moves them to their packed places.  A count > cap     */
/* means that ray overflowed its row (whose last slot then holds garbage): fall back to umhs_march_write for the batch.       */
int umhs_march_scratch(const float* origins, const float* directions, int64_t n_rays, const uint8_t* binaries,
                       const float* roi_aabb_host6, int levels, int resolution, float near_plane, float far_plane,
                       float step_size, float cone_angle, const float* nears, const float* fars, const float* jitter,
                       float jitter_step, int cap, int64_t* counts, float* scratch_t0, float* scratch_t1, const void* walked,
                       size_t walked_bytes, umhs_stream_t stream);
int umhs_march_compact(const int64_t* packed_info, int64_t n_rays, int cap, const float* scratch_t0, const float* scratch_t1,
                       float* t_starts, float* t_ends, int64_t* ray_indices, umhs_stream_t stream);
int umhs_visibility(const float* sigma, const float* t_starts, const float* t_ends, const int64_t* packed_info,
                    int64_t n_rays, int64_t n, float early_stop_eps, float alpha_thre, uint8_t* mask, umhs_stream_t stream);
/* `jitter` [R] or NULL (all three march entry points): the near plane of ray r is nears[r] (or near_plane) + jitter[r] *      */
/* jitter_step -- nerfacc's stratified start, folded into the walk instead of two fills, a multiply and an add in front of it.  */
/* umhs_visibility_count also returns kept[R], the survivors per ray; umhs_ray_prefix turns per-ray counts into packed_info     */
/* [R,2] = (exclusive prefix, count) and stats[2] = (total, longest) -- used for the marched candidates and for the survivors;   */
/* umhs_sample_midpoints = origins[ri] + directions[ri] * (t_starts + t_ends) / 2 (VolumetricSampler's sigma_fn positions);     */
/* umhs_compact_samples moves the survivors (order within the ray kept) to their packed places and gathers their ray's origin,   */
/* direction and camera index (camera_indices / out_camera_indices both NULL or both set); out_sel[j] = candidate index of       */
/* survivor j.  Together: the sampler's torch.nonzero + 3 index_select + 3 gathers + pack_info as one launch after its host sync. */
int umhs_visibility_count(const float* sigma, const float* t_starts, const float* t_ends, const int64_t* packed_info,
                          int64_t n_rays, int64_t n, float early_stop_eps, float alpha_thre, uint8_t* mask, int64_t* kept,
                          umhs_stream_t stream);
int umhs_ray_prefix(const int64_t* counts, int64_t n_rays, int64_t* packed_info, int64_t* stats, umhs_stream_t stream);
int umhs_sample_midpoints(const float* origins, const float* directions, const int64_t* ray_indices, const float* t_starts,
                          const float* t_ends, int64_t n, float* positions, umhs_stream_t stream);
int umhs_compact_samples(const uint8_t* mask, const int64_t* packed_in, const int64_t* packed_out, int64_t n_rays,
                         const float* t_starts, const float* t_ends, const float* origins, const float* directions,
                         const int64_t* camera_indices, int64_t* out_ray_indices, float* out_t_starts, float* out_t_ends,
                         float* out_origins, float* out_directions, int64_t* out_camera_indices, int64_t* out_sel,
                         umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* pixel sampler, ray generator and ground-truth gather (images resident in HBM, --images-on-gpu).    */
/* Replaces, under UMHSDataManager.next_train (umhs_datamanager.py:95-108), nerfstudio's PixelSampler.sample          */
/* (indices = long(rand[R,3] * (n, H, W)); batch[key] = stack[c, y, x]) and RayGenerator -> Cameras.generate_rays     */
/* (perspective, no distortion: d = R_c2w * ((x+.5-cx)/fx, -(y+.5-cy)/fy, -1) normalised, origin = t_c2w,             */
/* pixel_area from the +x / +y neighbour directions).  indices [R,3] int64 rows (camera, y, x); c2w [n,3,4];          */
/* intrinsics [n,4] = (fx, fy, cx, cy); stack [n,H,W,K] fp32 or uint8 (scaled by 1/255); pixel_area /                 */
/* directions_norm [R] optional.                                                                                      */
/* umhs_raygen_distorted: the same with OpenCV lens distortion (COLMAP's OPENCV camera model), distortion [n,6] =     */
/* (k1, k2, k3, k4, p1, p2) per camera, nerfstudio's order.  The pixel and its +x / +y neighbours are undistorted by  */
/* the 10 fixed Newton steps of nerfstudio's camera_utils.radial_and_tangential_undistort in OpenCV image-plane        */
/* coordinates ((x+.5-cx)/fx, (y+.5-cy)/fy), y DOWN; y is negated after the solve.  A camera whose row is all zero     */
/* gives exactly the bits of umhs_raygen.  Same argument checks, clamping and never-throw / alloc / sync rules.        */
/* umhs_raygen_frame: the rays of rows [row0, row0 + n_rows) of ONE camera's frame, without an index tensor: ray i is   */
/* pixel (y, x) = (row0 + i / width, i % width), one thread per pixel.  camera_type (the viewer's three; nerfstudio     */
/* Cameras._generate_rays_from_coords): with u = (px - cx) / fx, v = -(py - cy) / fy of the pixel centre and its +x /    */
/* +y neighbour the camera-frame direction is                                                                           */
/*   0 perspective:     (u, v, -1); with `distortion` [n_cams,6] the points are undistorted as umhs_raygen_distorted     */
/*   1 fisheye:         t = clamp(sqrt(u^2 + v^2), 0, pi), s = sin t / t (1 at t == 0): (u s, v s, -cos t)               */
/*   2 equirectangular: t = -pi u, p = pi (0.5 - v): (-sin t sin p, cos p, -cos t sin p)                                 */
/* (sinf / cosf, not the fast intrinsics), then umhs_raygen's arithmetic.  At camera_type 0 without a box every output  */
/* carries the bits umhs_raygen / umhs_raygen_distorted write for the same pixels.                                      */
/* obb_host15: NULL, or 15 HOST floats T[3], R[9] row-major, S[3] (copied at the call) -- a crop box, nerfstudio's       */
/* intersect_obb: o' = R^T (o - T), d' = R^T d (unit d); per axis a = (-S/2 - o') / d', b = (S/2 - o') / d' (IEEE: a     */
/* zero d' divides to +-inf; min / max ignore a NaN); t_min = max_k min(a, b), t_max = min_k max(a, b), both clamped to  */
/* [0, 1e10]; t_max <= t_min is a miss: nears = fars = 1e10; else nears = max(t_min, near_floor), fars = t_max.         */
/* nears / fars [n_rows*width]: both NULL or both set, required with a box (without one they are left untouched).       */
/* pixel_area / directions_norm optional.  UMHS_ERR_ARG, before anything is launched, for: a NULL required pointer,      */
/* camera outside 0 .. n_cams-1, camera_type outside 0 .. 2, distortion with a non-perspective type, rows outside the    */
/* frame, nears without fars or the reverse, a box without them, a scale that is not positive, near_floor < 0.          */
/* ------------------------------------------------------------------------------------------ */
int umhs_pixel_indices(const float* uniform, int64_t n_rays, int64_t n_images, int64_t height, int64_t width,
                       int64_t* indices, umhs_stream_t stream);
int umhs_raygen(const int64_t* indices, const float* c2w, const float* intrinsics, int64_t n_rays, int64_t n_cams,
                float* origins, float* directions, float* pixel_area, float* directions_norm, umhs_stream_t stream);
int umhs_raygen_distorted(const int64_t* indices, const float* c2w, const float* intrinsics, const float* distortion,
                          int64_t n_rays, int64_t n_cams, float* origins, float* directions, float* pixel_area,
                          float* directions_norm, umhs_stream_t stream);
int umhs_raygen_frame(const float* c2w, const float* intrinsics, const float* distortion, int64_t n_cams, int64_t camera,
                      int camera_type, int64_t height, int64_t width, int64_t row0, int64_t n_rows,
                      const float* obb_host15, float near_floor, float* origins, float* directions, float* pixel_area,
                      float* directions_norm, float* nears, float* fars, umhs_stream_t stream);
int umhs_pixel_gather(const int64_t* indices, const void* stack, int src_is_u8, int64_t n_images, int64_t height,
                      int64_t width, int n_channels, int64_t n_rays, float* out, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Per-frame masks (mask_path): the pixel sampler draws only where the mask is non-zero, uniformly over the set pixels  */
/* of the whole stack, with replacement (nerfstudio's mask-aware PixelSampler picks rows of nonzero(mask)).  At load a  */
/* uint8 mask stack [n, H*W] (a pixel is set iff its byte is non-zero) is compacted into                                */
/*   off [n+1] int64: exclusive prefix sum of the per-image counts, M = off[n];                                        */
/*   list [M] int32: flat ids y*W + x of the set pixels, ascending within an image, images in order.                   */
/* umhs_mask_count: chunk_counts [n_images * umhs_mask_chunks(H*W)] int32 = set pixels per chunk, image-major (a chunk   */
/*   never spans two images; which pixels a chunk holds depends on the alignment of `mask`, so count and compact must   */
/*   be given the same pointer).  The caller sums them per image (off) and scans them (chunk_offsets).                  */
/* umhs_mask_compact: writes the ids of chunk c, ascending, at list[chunk_offsets[c] ...]; chunk_offsets are positions   */
/*   in the WHOLE list, so a stack can be fed in pieces (one frame at a time from host memory) and ends with the same   */
/*   bits.  Writes outside [0, list_len) are dropped.  Deterministic: no atomics.  H*W > 2^24: UMHS_ERR_UNSUPPORTED.    */
/* umhs_pixel_indices_masked: for ray r, with u0 = uniform[r][0], u1 = uniform[r][1] (uniform[r][2] is unused), each     */
/*   product ONE float32 multiplication:  t = min((int64)(u0 * (float)M), M-1);  image i with off[i] <= t < off[i+1]     */
/*   (binary search; an image with an empty mask is never chosen);  cnt = off[i+1] - off[i];                            */
/*   k = min((int64)(u1 * (float)cnt), cnt-1);  p = list[off[i] + k];  indices[r] = (i, p / width, p % width).          */
/*   M == 0 gives rows of zeros (the caller refuses such a stack).  None of these allocates or synchronises.            */
/* ------------------------------------------------------------------------------------------ */
int64_t umhs_mask_chunks(int64_t pixels_per_image);
int umhs_mask_count(const uint8_t* mask, int64_t n_images, int64_t pixels_per_image, int32_t* chunk_counts,
                    umhs_stream_t stream);
int umhs_mask_compact(const uint8_t* mask, int64_t n_images, int64_t pixels_per_image, const int64_t* chunk_offsets,
                      int32_t* list, int64_t list_len, umhs_stream_t stream);
int umhs_pixel_indices_masked(const float* uniform, int64_t n_rays, int64_t n_images, int64_t width, const int64_t* off,
                              const int32_t* list, int64_t* indices, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* image metrics of the eval path, get_image_metrics_and_images (umhs_model.py:407-453), on channel-last */
/* images [H*W, K] as rendered.  umhs_pixel_metrics: partial[b] = {sum (p-g)^2, sum of finite spectral angles          */
/* acos(clamp(<p,g>/(|p||g|))), count of finite angles} per block b < n_partial (PSNR :430,444, RMSE :452, SAM :447).   */
/* umhs_ssim: torchmetrics==1.5.2 structural_similarity_index_measure (:431,445; 11x11 gaussian sigma 1.5, k1 .01,      */
/* k2 .03): partial[] = per-block sums of the SSIM index over the (H-10)(W-10)K windows inside the image;               */
/* data_range = DEVICE float (max(a.max-a.min, b.max-b.min) for the default data_range=None).                           */
/* The caller adds the partials (fixed order: reproducible) and divides.                                                */
/* Which slot holds what (tests/metrics_f64.py relies on it):                                                           */
/*   umhs_pixel_metrics: block b owns the pixels p with (p / 256) % n_partial == b.  Every slot b < n_partial is        */
/*     written and nothing past it; a block without pixels writes zeros.  An all-zero or non-finite spectrum gives no   */
/*     angle (not counted); its squared error is still added, so a NaN / Inf value makes its block's first sum so.      */
/*   umhs_ssim: slot (c * GY + by) * GX + bx holds the windows (oy, ox), 8 by <= oy < 8 by + 8 and                      */
/*     32 bx <= ox < 32 bx + 32, of channel c (window (oy, ox) covers rows oy..oy+10, columns ox..ox+10);               */
/*     GX = ceil((W - 10) / 32), GY = ceil((H - 10) / 8), umhs_ssim_partials = GX * GY * K slots (0: image < 11 x 11).  */
/*     Both variances are clamped at 0 before the index is formed; nothing is contracted into an fma.                   */
/* ------------------------------------------------------------------------------------------ */
int umhs_pixel_metrics(const float* pred, const float* gt, int64_t n_pixels, int n_channels, double* partial, int n_partial,
                       umhs_stream_t stream);
int64_t umhs_ssim_partials(int height, int width, int n_channels);
int umhs_ssim(const float* a, const float* b, int height, int width, int n_channels, const float* data_range,
              double* partial, int64_t n_partial, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Material segmentation against ground-truth labels (the reference's seg_image, hs_dataloader.py:60-64): the confusion  */
/* table of the labels the model emitted.  seg_raw / accumulation [n_pixels] fp32 as umhs_ray_epilogue_fwd writes them,  */
/* labels [n_pixels] uint8 at ANY byte alignment, counts [(n_classes + 1) * n_labels] int64, ADDED to.  Per pixel:        */
/*   p = accumulation > 0.5f ? (int)seg_raw : n_classes   (the last row is "nothing rendered"; NaN is not > 0.5)         */
/*   k = labels[i];   counts[p * n_labels + k] += 1                                                                      */
/* A pixel is skipped, and never indexes the table, when k == ignore_label (-1: no label is ignored), k >= n_labels, or   */
/* it is rendered and seg_raw is not an integer of [0, n_classes).  Integer counts: exact, independent of order.  One      */
/* table in LDS per workgroup, one 64-bit atomic per non-zero bin and workgroup at the end; no per-pixel global atomic.    */
/* n_classes > 16 or n_labels > 32: UMHS_ERR_UNSUPPORTED.  Does not allocate or synchronise.                              */
/* ------------------------------------------------------------------------------------------ */
int umhs_seg_confusion(const float* seg_raw, const float* accumulation, const uint8_t* labels, int64_t n_pixels,
                       int n_classes, int n_labels, int ignore_label, int64_t* counts, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Frame composition for camera-path rendering (the reference's scripts/render.sh: ns-render camera-path                   */
/* --rendered-output-names ...): per-ray float outputs -> one uint8 frame [height, n_panels * width, 3], the panels side   */
/* by side (nerfstudio: apply_colormap per output, np.concatenate(axis=1), x255, cast).  Sources are read in place at      */
/* (stride, channel): wv_7 is `spectral` with stride B and channel 7.  `panels` is a HOST array, copied at the call.        */
/* The result is integers, so the arithmetic is fixed to the bit: every operation below is ONE rounded float32 operation,   */
/* nothing is contracted into an fma, and every clamp keeps a NaN a NaN.                                                    */
/*   q(c)   : t = (c * 255) + 0.5, clamped to [0, 255], truncated; NaN -> 0   (torchvision's save_image)                    */
/*   RGB    : q of the three channels at `channel`.                                                                         */
/*   SCALAR : (1) with normalize: v = (x - lo) / ((hi - lo) + 1e-9f);  (2) unless cmin == 0 && cmax == 1:                   */
/*            v = v * (cmax - cmin) + cmin, the subtraction, the product and the sum each rounded;  (3) clamp to [0, 1];    */
/*            (4) with invert: v = 1 - v;  (5) NaN -> 0;  (6) i = (int)(v * 255), truncated;  (7) bytes q(lut[i][0..2]).    */
/*   DEPTH  : v = (x - lo) / ((hi - lo) + 1e-10f), clamped to [0, 1]; then SCALAR (2)..(6); c = lut[i]; with                */
/*            `accumulation` a: c = c * a + (1 - a) per channel (three rounded operations); bytes q(c).                     */
/* `frame` may start at ANY byte address: the interior of every panel's part of a frame row is written as aligned 16-byte  */
/* words, only the up to 15 bytes at either end of it as dwords and bytes.  src / range / accumulation / lut are 4-byte    */
/* aligned.  n_panels > 16 (or                                                                                              */
/* n_panels * width >= 2^31): UMHS_ERR_UNSUPPORTED; height * width == 0: UMHS_OK, nothing is launched.  One launch; does    */
/* not allocate or synchronise.                                                                                             */
/* ------------------------------------------------------------------------------------------ */
enum { UMHS_PANEL_RGB = 0, UMHS_PANEL_SCALAR = 1, UMHS_PANEL_DEPTH = 2 };
typedef struct umhs_frame_panel {
  const float* src;          /* DEVICE rows [H*W, stride] fp32                                   */
  const float* range;        /* DEVICE 2 floats (lo, hi): DEPTH always, SCALAR with normalize    */
  const float* accumulation; /* DEVICE [H*W] or NULL: DEPTH is blended over white with it         */
  int32_t stride, channel;   /* floats per row of src; first channel read (RGB reads 3)          */
  int32_t kind, flags;       /* flags bit0 normalize, bit1 invert                                */
  float cmin, cmax;          /* colormap_min / colormap_max (0, 1 = identity, no arithmetic)     */
} umhs_frame_panel;
int umhs_frame_compose(const umhs_frame_panel* panels /* HOST */, int n_panels /* 1..16 */, const float* lut /* DEVICE [256,3] */,
                       int height, int width, uint8_t* frame /* DEVICE [height, n_panels*width, 3], ANY byte alignment */,
                       umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Point-cloud export (ns-export pointcloud; nerfstudio's exporter_utils.generate_point_cloud and Open3D's                    */
/* remove_statistical_outlier, restated): rendered rays -> packed binary-PLY rows, and the exact k-nearest-neighbour mean       */
/* distances of the kept points.  `args` is a HOST struct, copied at the call; its sources are DEVICE rows read in place at     */
/* their own stride (floats per row).  Integers come out, so the arithmetic is fixed to the bit: every step is ONE rounded      */
/* float32 operation, nothing is contracted into an fma.                                                                        */
/*   point   : p_k = (d_k * depth) + o_k                                                        (model frame)                   */
/*   keep    : accumulation > threshold (strict; NaN is not greater)  and  |p_k| <= FLT_MAX for k = 0, 1, 2  and, with a box,    */
/*             e_j = p_j - T_j;  q_k = ((R[0][k] * e_0) + (R[1][k] * e_1)) + (R[2][k] * e_2)  (q = R^T (p - T), R row-major);    */
/*             h_k = S_k * 0.5f;  q_k < h_k and q_k > -h_k   (nerfstudio's OrientedBox.within: a point on a face is outside)     */
/*   xyz     : p, or with has_world  w_i = (((A[i][0] * p_0) + (A[i][1] * p_1)) + (A[i][2] * p_2)) + A[i][3], A = world [3,4]    */
/*             row-major.  Only the written xyz is transformed: the box test, `points` and the neighbour search see p.          */
/*   byte    : b(v) = (uint8)(clamp(v, 0, 1) * 255.0f), truncated, NaN -> 0;  red, green, blue = b(rgb[0..2]),                   */
/*             alpha = b(accumulation)                                                                                          */
/*   material: the first index of the largest of seg_probs[0 .. C) (a NaN never wins), what umhs_ray_epilogue_fwd's seg_raw      */
/*             holds before its fold with accumulation > 0.5                                                                    */
/* A row is 16 bytes with n_classes == 0 (float x, y, z; uchar red, green, blue, alpha) and 20 + 4 C bytes otherwise (the same, */
/* int32 material, float abundances[0 .. C)); rows are written as dwords, `rows` is 4-byte aligned.  A chunk is 256 rays.        */
/* umhs_pc_flag_count: chunk_counts [umhs_pc_chunks(n_rays)] int32 = kept rays per chunk.  The caller scans them (exclusive:     */
/*   chunk_offsets, int64) and holds the number of rows of the earlier batches in the DEVICE scalar `base`.                      */
/* umhs_pc_emit: kept ray r of rank j inside its chunk (ray order) goes to row at = base[0] + chunk_offsets[chunk] + j:          */
/*   rows[at], points[at] = p (float [cap,3]), kept[at] = ordinal0 + r (int64 [cap]).  at outside [0, cap) is never written.     */
/*   No atomics: the result is a function of the inputs alone.  n_classes > 16: UMHS_ERR_UNSUPPORTED.                            */
/* umhs_pc_cell_keys: keys[i] = (c_z * dims[1] + c_y) * dims[0] + c_x of points [m,3] in a uniform grid, per axis                */
/*   f = (x - lo) / edge (two rounded operations), c = f >= 0 ? (f < dims ? (int)f : dims - 1) : 0.  lo / dims are HOST arrays;  */
/*   every dimension in [1, 4096], at most 2^21 cells (UMHS_ERR_UNSUPPORTED beyond).  A degenerate axis has one cell.            */
/* umhs_knn_mean_dist: mean[i] = (sum of the k_eff = min(k, m) smallest sqrt(d2(i, j)), j over ALL m points, i itself            */
/*   included -- as Open3D's SearchKNN returns the query first) / k_eff, for sorted_points [m,3] = the points in ascending key    */
/*   order and cell_start [cells + 1] int32 = first sorted index of every cell (cell_start[cells] = m).  d2 = ((dx*dx) + (dy*dy)) */
/*   + (dz*dz) in float32; the square roots are added in ascending order, then one division.  Exact (not approximate) for ANY     */
/*   lo / edge / dims consistent with the keys: the grid decides the time, not the result.  2 <= k <= 32 (k > 32:                */
/*   UMHS_ERR_UNSUPPORTED).  The k smallest live in registers (K = 20, and K = 32 padded for every other k); no scratch.          */
/* None of these allocates or synchronises; each is one launch (none for n_rays == 0 / m == 0).                                  */
/* ------------------------------------------------------------------------------------------ */
typedef struct umhs_pc_args {
  const float *origins, *directions, *depth, *accumulation, *rgb; /* DEVICE rows; 3, 3, 1, 1, 3 floats read per row     */
  const float *abundances, *seg_probs;                            /* DEVICE rows of n_classes floats; unused if n_classes == 0 */
  int32_t origins_stride, directions_stride, depth_stride, accumulation_stride, rgb_stride, abundances_stride, seg_probs_stride;
  int32_t n_classes;                                              /* C; 0 = the 16-byte row                              */
  float threshold;                                                /* opacity threshold                                   */
  int32_t has_box, has_world;
  float box_center[3], box_rotation[9], box_scale[3];             /* T, R (row-major), S of the oriented box             */
  float world[12];                                                /* [3,4] row-major affine applied to the written xyz   */
} umhs_pc_args;
int64_t umhs_pc_chunks(int64_t n_rays);
int umhs_pc_flag_count(const umhs_pc_args* args /* HOST */, int64_t n_rays, int32_t* chunk_counts, umhs_stream_t stream);
int umhs_pc_emit(const umhs_pc_args* args /* HOST */, int64_t n_rays, const int64_t* chunk_offsets, const int64_t* base,
                 int64_t ordinal0, void* rows, float* points, int64_t* kept, int64_t cap, umhs_stream_t stream);
int umhs_pc_cell_keys(const float* points, int64_t m, const float* lo_host3, float edge, const int32_t* dims_host3, int32_t* keys,
                      umhs_stream_t stream);
int umhs_knn_mean_dist(const float* sorted_points, int64_t m, const int32_t* cell_start, const float* lo_host3, float edge,
                       const int32_t* dims_host3, int k, float* mean, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Mesh export (ns-export tsdf, restated): rendered depth maps -> a truncated signed distance volume -> a triangle mesh whose   */
/* vertices carry colour, material label and abundances.  The structs are HOST structs, copied at the call.  Integers and bits  */
/* come out, so the arithmetic is fixed: every step below is ONE rounded float32 operation in the order the brackets give,      */
/* nothing is contracted into an fma; sqrt and every division are correctly rounded.                                            */
/* Volume: lattice points p = lo + (x, y, z) * h, i.e. p_k = lo_k + ((float)x_k * h), index i = (z * ny + y) * nx + x,            */
/*   N = nx ny nz <= 2^28.  D [N] mean truncated distance, W [N] its weight, Wc [N] the weight of the attributes, A [n_attr, N]  */
/*   attribute PLANES, n_attr = 3 + 2 C: rgb, abundances[0 .. C), seg_probs[0 .. C); C <= 16.  All float32 DEVICE arrays, zero   */
/*   before the first call.                                                                                                      */
/* umhs_tsdf_integrate: one thread per lattice point, the cameras 0 .. n_cameras-1 (<= 16 per call) in order; per camera with    */
/*   rotation R (row-major, camera-to-world, the camera looks down -z) and origin t:                                             */
/*   1. e = p - t;  pc_j = ((R[0][j] e_0) + (R[1][j] e_1)) + (R[2][j] e_2);  zc = -pc_2;  skipped unless zc > 0                   */
/*   2. x = pc_0 / zc, y = (-pc_1) / zc (image plane, y down); with `distorted` the forward OpenCV model, k = (k1, k2, k3, k4,    */
/*      p1, p2):  r = (x x) + (y y);  d = 1 + (r (k1 + (r (k2 + (r (k3 + (r k4)))))));                                            */
/*      x' = ((d x) + (((2 p1) x) y)) + (p2 (r + ((2 x) x)));  y' = ((d y) + (((2 p2) x) y)) + (p1 (r + ((2 y) y)))  -- the terms   */
/*      umhs_raygen_distorted's Newton steps subtract the distorted point from, so projection and ray generation are one model   */
/*   3. u = (fx x) + cx, v = (fy y) + cy; skipped unless 0 <= u < width and 0 <= v < height; pixel ((int)u, (int)v)               */
/*   4. d = depth, a = accumulation of that pixel of image c; skipped unless |d| <= FLT_MAX                                       */
/*   5. a <= threshold: free space, obs = 1, no tint.  Otherwise (a NaN included) a hit:                                          */
/*      dist = sqrt(((e_0 e_0) + (e_1 e_1)) + (e_2 e_2));  sdf = d - dist;  skipped if sdf < -truncation;                          */
/*      obs = min(1, sdf / truncation);  tint iff |sdf| <= truncation                                                             */
/*   6. D = ((D W) + obs) / (W + 1);  W = W + 1                                                                                   */
/*   7. with tint, for every attribute: A = ((A Wc) + attr) / (Wc + 1);  then Wc = Wc + 1                                        */
/*   Images: depth / accumulation [n, H, W], rgb [n, H, W, 3], abundances / seg_probs [n, H, W, C] read in place; *_strides =    */
/*   floats between images, rows and pixels; channels are adjacent.  No point is written by two threads, no atomics: fusing the  */
/*   cameras in one call or in calls split anywhere gives the same bits.                                                         */
/* Extraction: marching tetrahedra on the Kuhn decomposition.  A point is valid iff W > 0 and inside iff D < 0.  Point i owns    */
/*   the 7 edges towards +(100, 010, 001, 110, 101, 011, 111) (slots 0 .. 6, x first); an edge carries a vertex iff it stays     */
/*   inside the lattice, both ends are valid and exactly one is inside.  Cell i (x < nx-1, y < ny-1, z < nz-1; its corner 000 is */
/*   point i) emits iff all 8 corners are valid; it is cut into 6 tetrahedra, one per permutation (a, b, c) of the axes in       */
/*   lexicographic order, with corners v0 = 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = 111.  A chunk is 256 lattice indices.         */
/* umhs_mesh_mark: edge_mask [N] uint8 (bit s = slot s carries a vertex), vertex_counts / triangle_counts [umhs_mesh_chunks(N)]  */
/*   int32.  The caller scans both (exclusive, int64).                                                                           */
/* umhs_mesh_vertices: vertex ids ascend by (i, slot); vertex_base [N] int32 = id of point i's first vertex (written for every    */
/*   point).  With a = point i, b = the other end:  t = D_a / (D_a - D_b);  pos_k = pa_k + (t (pb_k - pa_k)), pa / pb by the      */
/*   lattice formula; with world_host12 (HOST [3,4] row-major, or NULL) the written xyz is                                        */
/*   (((A[r][0] pos_0) + (A[r][1] pos_1)) + (A[r][2] pos_2)) + A[r][3].  Attributes: both ends with Wc > 0: A_a + (t (A_b - A_a)); */
/*   one end: that end's; none: zeros and material -1.  material = first index of the largest interpolated seg_probs (a NaN      */
/*   never wins).  Row = float x, y, z; uchar red, green, blue (the point-cloud byte); and with C > 0 int32 material, float       */
/*   abundances[0 .. C): 15 or 19 + 4 C bytes at ANY byte address.  Rows at or beyond cap are not written.                        */
/* umhs_mesh_triangles: faces [cap, 3] int32 in (cell, tetrahedron, triangle) order; the normal (right-hand rule) points to the   */
/*   non-negative side.  e(i, j) = the vertex on the edge of corners v_i, v_j = vertex_base[owner] + popcount(edge_mask[owner]    */
/*   & ((1 << slot) - 1)), owner = the lower corner.  sigma = the permutation's parity (odd: tetrahedra 1, 2, 5).                 */
/*   One corner p apart from the others q0 < q1 < q2 (1 or 3 inside): (e(p,q0), e(p,q1), e(p,q2)), the last two swapped iff        */
/*   (p odd) xor sigma xor (3 inside).  Two inside p0 < p1, two outside q0 < q1: the quad a = e(p0,q0), b = e(p0,q1),               */
/*   c = e(p1,q1), d = e(p1,q0) is split along a-c into (a, b, c) and (a, c, d), the last two of each swapped iff                  */
/*   (number of pairs p_i > q_j is odd) xor sigma.                                                                                */
/* None of these allocates or synchronises; each is one launch.  Arguments are checked before anything is launched.               */
/* ------------------------------------------------------------------------------------------ */
#define UMHS_TSDF_MAX_CAMERAS 16
typedef struct umhs_tsdf_volume {
  float *D, *W, *Wc, *A; /* DEVICE [N], [N], [N], [n_attr, N]                               */
  int32_t dims[3];       /* nx, ny, nz                                                      */
  int32_t n_attr;        /* 3 + 2 C                                                         */
  float lo[3], h;        /* first lattice point, voxel edge                                 */
} umhs_tsdf_volume;
typedef struct umhs_tsdf_camera {
  float rotation[9], origin[3]; /* camera-to-world [3,3] row-major, camera position         */
  float fx, fy, cx, cy;
  float distortion[6];          /* k1 k2 k3 k4 p1 p2                                         */
  int32_t distorted;            /* 0: steps 2's model is skipped                             */
} umhs_tsdf_camera;
typedef struct umhs_tsdf_images {
  const float *depth, *accumulation, *rgb, *abundances, *seg_probs; /* DEVICE                                */
  int64_t depth_strides[3], accumulation_strides[3], rgb_strides[3], abundances_strides[3], seg_probs_strides[3];
  int32_t n_cameras, height, width, n_classes;
  float threshold, truncation;
  umhs_tsdf_camera cameras[UMHS_TSDF_MAX_CAMERAS];
} umhs_tsdf_images;
int64_t umhs_mesh_chunks(int64_t n_points);
int umhs_tsdf_integrate(const umhs_tsdf_volume* volume /* HOST */, const umhs_tsdf_images* images /* HOST */, umhs_stream_t stream);
int umhs_mesh_mark(const umhs_tsdf_volume* volume /* HOST */, uint8_t* edge_mask, int32_t* vertex_counts, int32_t* triangle_counts,
                   umhs_stream_t stream);
int umhs_mesh_vertices(const umhs_tsdf_volume* volume /* HOST */, const uint8_t* edge_mask, const int64_t* vertex_offsets,
                       const float* world_host12, int32_t* vertex_base, void* rows, int64_t cap, umhs_stream_t stream);
int umhs_mesh_triangles(const umhs_tsdf_volume* volume /* HOST */, const uint8_t* edge_mask, const int32_t* vertex_base,
                        const int64_t* triangle_offsets, int32_t* faces, int64_t cap, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Textured mesh export (ns-export tsdf --texture-method nerf, restated; csrc/umhs_texture.hip): a per-face texture atlas and, for */
/* every texel, the short ray through the surface that the model renders into it.  The layout is this project's own, modelled on    */
/* nerfstudio's "custom" per-triangle unwrap [upstream-recalled, in spirit only: two triangles per square of px_per_uv_triangle      */
/* texels].  Integers and bits come out, so layout and arithmetic are fixed: every float step below is ONE rounded float32           */
/* operation in the order the brackets give, nothing is contracted into an fma; sqrt and every division are correctly rounded.       */
/* Sizes: F >= 1 faces, p = px >= 4, e = p - 3, S = ceil(F / 2) squares, Q = the least integer with Q Q >= S (integer arithmetic),    */
/*   atlas side T = Q p, a square atlas of T T texels.  T <= 16384 (so 2 T < 2^24 and T T <= 2^28), UMHS_ERR_UNSUPPORTED above.       */
/* Owner: texel t = row T + col, row 0 the TOP row of the image.  sx = col / p, sy = row / p, i = col % p, j = row % p,               */
/*   s = sy Q + sx, k = (i + j >= p), face f = 2 s + k; f >= F: an empty texel.  So every texel of a used square has exactly one      */
/*   owner: the even face owns i + j <= p - 1, the odd face the rest.                                                                  */
/* Corners, in the square's texel-centre lattice (i, j):  even face: corner 0 = (0, 0), 1 = (e, 0), 2 = (0, e);  odd face: corner     */
/*   0 = (p-1, p-1), 1 = (2, p-1), 2 = (p-1, 2).  A corner is a texel centre.  The bilinear footprint of a point inside the even      */
/*   triangle has lattice sums <= e + 2 = p - 1, of one inside the odd triangle >= (p + 1) - 1 = p, and neither leaves the square:    */
/*   the texels of the footprint that carry weight belong to the face.  Owned texels outside the triangle are a gutter, filled by     */
/*   extrapolation (below).                                                                                                            */
/* umhs_texture_uv: uv [F, 3, 2] float32, (u, v) of corner c = (i_c, j_c) of face f, v upwards as OBJ's vt:                            */
/*   u = (float)(2 (sx p + i_c) + 1) / (float)(2 T);  v = (float)(2 (T - (sy p + j_c)) - 1) / (float)(2 T)  -- exact integers,         */
/*   one rounded division each.                                                                                                        */
/* umhs_texture_rays, for texels [texel_begin, texel_end), outputs indexed from texel_begin; V_k = positions[faces[f][k]]:             */
/*   1. n1 = i, n2 = j (even) or n1 = p-1-i, n2 = p-1-j (odd); n0 = e - n1 - n2 (integers, negative or above e in the gutter);          */
/*      w_k = (float)n_k / (float)e                                                                                                    */
/*   2. P_c = ((w0 V0_c) + (w1 V1_c)) + (w2 V2_c)                                                                                       */
/*   3. a = V1 - V0, b = V2 - V0;  n = ((a_y b_z) - (a_z b_y), (a_z b_x) - (a_x b_z), (a_x b_y) - (a_y b_x));                           */
/*      q = ((n_x n_x) + (n_y n_y)) + (n_z n_z);  r = sqrt(q);  n^_c = n_c / r                                                          */
/*   4. direction = -n^;  origin_c = P_c + ((0.5 L) n^_c), L = ray_length;  nears = 0, fars = L: the ray starts half its length        */
/*      outside the surface (faces are oriented, the right-hand normal points outwards) and runs through it                            */
/*   5. a face is dead if one of its indices is outside [0, V) -- compared as unsigned numbers BEFORE anything is loaded through it    */
/*      -- or if q is not a finite positive number                                                                                     */
/*   6. texels of dead faces and empty texels are misses, as the crop path of umhs_raygen_frame writes a miss: texel_face = -1,         */
/*      origin = 0, direction = (0, 0, 1), nears = fars = 1e10f, bary = 0.  Live texels: texel_face = f, bary = (w0, w1, w2).           */
/*   origins / directions [n, 3], nears / fars [n], texel_face [n] int32, bary [n, 3] or NULL, n = texel_end - texel_begin.  One        */
/*   launch, no workspace, no atomics; no texel is written twice, so a range split anywhere gives the same bits.  An empty range:     */
/*   UMHS_OK, nothing is launched.                                                                                                     */
/* Checked before anything is launched, in this order: px < 4 or n_faces < 1: UMHS_ERR_ARG; T > 16384: UMHS_ERR_UNSUPPORTED;            */
/*   ray_length not finite or not positive, a range outside [0, T T], n_vertices < 1, a NULL required pointer: UMHS_ERR_ARG             */
/*   (n_vertices >= 2^31, more than an int32 index names: UMHS_ERR_UNSUPPORTED).                                                       */
/* umhs_texture_atlas is host arithmetic (Q and T of the sizes above); its two outputs are written only with UMHS_OK.                  */
/* ------------------------------------------------------------------------------------------ */
int umhs_texture_atlas(int64_t n_faces, int px, int32_t* squares_per_side /* HOST */, int32_t* side /* HOST */);
int umhs_texture_uv(int64_t n_faces, int px, float* uv, umhs_stream_t stream);
int umhs_texture_rays(const float* positions, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int px, float ray_length,
                      int64_t texel_begin, int64_t texel_end, float* origins, float* directions, float* nears, float* fars,
                      int32_t* texel_face, float* bary, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Mesh simplification (csrc/umhs_simplify.hip): vertex clustering (Rossignac-Borrel) whose representatives minimise the cluster's */
/* plane quadric (Lindstrom 2000), on the rows and faces umhs_mesh_vertices / umhs_mesh_triangles write.  Faces, labels and colour  */
/* bytes come out, so those rules are fixed to the bit (float32 steps are ONE rounded operation each, never contracted); positions   */
/* and abundances are float64 sums rounded once to float32 (tests/simplify_ref.py holds their bound).  No float atomics anywhere.    */
/* Input: rows [V, row_bytes] uint8 at ANY byte address (row_bytes = 15, or 19 + 4 C with 1 <= C <= 15), faces [F, 3] int32.          */
/* Grid: origin g (3 floats), edge e > 0 (HOST values).  Per axis q_a = (p_a - g_a) / e,  i_a = min((int)floor(q_a), n_a - 1),        */
/*   clamped below at 0;  n_a = (int)floor((M_a - g_a) / e) + 1 (at least 1) with M_a the largest coordinate over the finite          */
/*   vertices.  key = (i_z n_y + i_y) n_x + i_x.  The key is an int64 and the caller refuses a grid of 2^62 cells or more, or an      */
/*   axis of 2^31 or more, before any launch.  (An int32 key and a 2^31-cell limit, as first planned, cannot hold the grid that      */
/*   separates every vertex of even a 24^3 mesh, which the identity property below needs.)                                            */
/* A vertex with a coordinate that is not finite joins no cluster (key INT64_MAX).  A face with such a vertex, or with an index       */
/*   outside [0, V) -- compared as unsigned numbers before anything is loaded through it -- is invalid and dropped.                   */
/* Clusters: the vertices that share a key; members in ascending input index (a stable sort by key); cluster ids ascend by key.      */
/* Faces: every index is replaced by its cluster; a face with two equal corners is dropped; of the faces that are equal after         */
/*   rotating the smallest cluster to the front (same orientation) the first in input order is kept; an opposite twin is kept.        */
/*   Kept faces stay in input order with their corner order.  Clusters no kept face names are dropped, the rest numbered by key.      */
/* Position of a cluster, float64, relative to its cell centre o_a = g_a + (i_a + 0.5) e (g, e converted to float64 first):           */
/*   for every VALID input face (a, b, c) -- dropped or not -- in ascending (face, corner) order per cluster: n = (b - a) x (c - a);  */
/*   A += n n^T, b += n (n . (a - o)) for each corner's cluster.  m = (sum of the members' p - o) / count;  lambda = 1e-3 tr(A) / 3; */
/*   x solves (A + lambda I) x = b + lambda m (Cholesky; condition <= 3001);  tr(A) = 0: x = m.  o + x is clamped per axis to the     */
/*   union of the cell's box [g + i e, g + (i + 1) e] and the members' bounding box, then rounded to float32; with world_host12 the   */
/*   written xyz is umhs_mesh_vertices' affine of that float32 (the same helper, csrc/umhs_affine.h).  A cluster of one vertex        */
/*   returns that vertex bit for bit.                                                                                                 */
/* Attributes: colour byte (2 S + n) / (2 n) in integers (S the members' byte sum, n their number); material = the most frequent      */
/*   member label after clamping into [-1, C - 1] (-1, "nobody tinted this vertex", is a label umhs_mesh_vertices writes: it keeps     */
/*   its own count, so a cluster of one vertex returns its label), ties to the smallest; abundances = (float64 sum in member order)    */
/*   / n, rounded.                                                                                                                     */
/* The passes (each entry is one launch unless it says otherwise; none allocates or synchronises; arguments are checked first):       */
/*   umhs_simplify_unpack   positions [V, 3] float32 and, per chunk of 256 vertices, the largest finite coordinate per axis           */
/*                          (chunk_max [umhs_mesh_chunks(V), 3], -inf where a chunk has none); the caller reduces the chunks.         */
/*   umhs_simplify_keys     keys [V] int64.                                                                                           */
/*   (the caller sorts the keys, stable)                                                                                              */
/*   umhs_simplify_heads    head [V] uint8: sorted position i starts a cluster.                                                       */
/*   umhs_simplify_flag_count / umhs_simplify_flag_rank   counts of set flags per chunk of 256 / the exclusive rank of every          */
/*                          element given the caller's exclusive int64 scan of the counts: used for heads, kept faces, used clusters. */
/*   umhs_simplify_members  vertex_cluster [V] int32 (-1: none), cluster_start [n_clusters + 1] int32 (sorted positions).             */
/*   umhs_simplify_faces    face_cluster [F, 3] int32 (INT32_MAX x 3 for an invalid face: the corner records' sort key), and the      */
/*                          canonical triple as key_hi [F] int64 = c0 2^31 + c1, key_lo [F] int32 = c2 (INT64_MAX / 0 for a dropped    */
/*                          face).  The caller sorts (key_hi, key_lo) lexicographically, stable, and the 3 F corner records by        */
/*                          cluster, stable.                                                                                          */
/*   umhs_simplify_dedup    keep [F] uint8 from the sorted order `perm`; with `used` [n_clusters] uint8 (zeroed by the caller, or     */
/*                          NULL) the clusters of kept faces are flagged (plain stores of 1).                                         */
/*   umhs_simplify_clusters one thread per cluster that a kept face names walks its members and its corner records (both contiguous  */
/*                          in their sorted orders), solves and writes row cluster_rank[c] of rows_out and positions_out.             */
/*   umhs_simplify_emit     TWO launches: faces_out [cap, 3] of the kept faces, vertex_out [V] (output vertex of every input vertex   */
/*                          or -1).                                                                                                   */
/* ------------------------------------------------------------------------------------------ */
typedef struct umhs_simplify_args {
  const void* rows;              /* DEVICE [V, row_bytes] uint8                                   */
  const float* positions;        /* DEVICE [V, 3] (umhs_simplify_unpack)                          */
  const int32_t* faces;          /* DEVICE [F, 3]                                                 */
  const int64_t* member_order;   /* DEVICE [V]: input index of sorted position i                  */
  const int32_t* cluster_start;  /* DEVICE [n_clusters + 1]                                       */
  const int64_t* corner_order;   /* DEVICE [3 F]: record 3 f + corner of sorted position j        */
  const int32_t* corner_start;   /* DEVICE [n_clusters + 1]: first sorted record of every cluster */
  const uint8_t* used;           /* DEVICE [n_clusters]                                           */
  const int32_t* cluster_rank;   /* DEVICE [n_clusters]: exclusive rank of `used`                 */
  void* rows_out;                /* DEVICE [cap, row_bytes] uint8, any byte address               */
  float* positions_out;          /* DEVICE [cap, 3]: model frame, before `world`                  */
  int64_t n_vertices, n_faces, n_clusters, cap;
  int32_t n_classes, has_world;
  int32_t dims[3], pad;
  float origin[3], edge;
  float world[12];
} umhs_simplify_args;
int umhs_simplify_unpack(const void* rows, int64_t n_vertices, int row_bytes, float* positions, float* chunk_max, umhs_stream_t stream);
int umhs_simplify_keys(const float* positions, int64_t n_vertices, const float* origin_host3, float edge, const int32_t* dims_host3,
                       int64_t* keys, umhs_stream_t stream);
int umhs_simplify_heads(const int64_t* sorted_keys, int64_t n_vertices, uint8_t* head, umhs_stream_t stream);
int umhs_simplify_flag_count(const uint8_t* flags, int64_t n, int32_t* counts, umhs_stream_t stream);
int umhs_simplify_flag_rank(const uint8_t* flags, int64_t n, const int64_t* offsets, int32_t* rank, umhs_stream_t stream);
int umhs_simplify_members(const int64_t* sorted_keys, const int64_t* member_order, const uint8_t* head, const int32_t* head_rank,
                          int64_t n_vertices, int32_t* vertex_cluster, int32_t* cluster_start, umhs_stream_t stream);
int umhs_simplify_faces(const int32_t* faces, int64_t n_faces, const int32_t* vertex_cluster, int64_t n_vertices, int32_t* face_cluster,
                        int64_t* key_hi, int32_t* key_lo, umhs_stream_t stream);
int umhs_simplify_dedup(const int64_t* key_hi, const int32_t* key_lo, const int64_t* perm, const int32_t* face_cluster, int64_t n_faces,
                        int64_t n_clusters, uint8_t* keep, uint8_t* used, umhs_stream_t stream);
int umhs_simplify_clusters(const umhs_simplify_args* args /* HOST */, umhs_stream_t stream);
int umhs_simplify_emit(const int32_t* face_cluster, const uint8_t* keep, const int32_t* face_rank, const int32_t* vertex_cluster,
                       const uint8_t* used, const int32_t* cluster_rank, int64_t n_faces, int64_t n_vertices, int64_t n_clusters,
                       int32_t* faces_out, int64_t cap, int32_t* vertex_out, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Mesh components (csrc/umhs_components.hip): the connected components of an indexed mesh, their sizes, and the mesh of the kept     */
/* ones -- what removes floaters and crumbs from an export.  Rows and faces as in "Mesh simplification" (rows at ANY byte address).   */
/* A face is VALID when its three indices lie in [0, V) (compared as unsigned numbers before anything is loaded through them).  A      */
/*   component is a maximal set of vertices joined through the edges of valid faces; a face with repeated indices is valid and joins   */
/*   what it names; an invalid face joins nothing, has face_component -1 and is never emitted.  A vertex no valid face names is a      */
/*   component of its own.  The LABEL of a component is its smallest vertex index; component ids 0 .. K - 1 number the labels in        */
/*   ascending order.  Nothing here depends on scheduling.                                                                              */
/* Labelling: parent[v] = v; a ROUND is two launches, a hook (per valid face, m = the smallest of the corners' parents; the parent of  */
/*   every corner's parent, and of the corner, is lowered to m by atomicMin) and a jump (per vertex, a parent chase of at most 16       */
/*   steps, then atomicMin).  parent[] only ever falls and every value is a vertex of the same component, so a stale read is an older,  */
/*   larger, valid value.  Round r of a call sets bit r of *changed (zeroed by the caller) iff one of its atomicMin calls lowered a     */
/*   value; a round that lowered nothing leaves parent[v] = the label of v.  At most V - 1 rounds lower anything (after round k every   */
/*   vertex within k faces of a component's smallest vertex carries it); the caller stops, and refuses the result, beyond V + 1.        */
/* Statistics per component: faces = its valid faces (a valid face belongs to the component of its first corner, which is that of all  */
/*   three), vertices, area.  Face area, float32, every step ONE rounded operation: u = b - a, w = c - a, n = u x w (each component     */
/*   a difference of two products), 0.5 * sqrt((n0 n0 + n1 n1) + n2 n2); 0 for a face with a corner that is not finite (it is still     */
/*   counted and still connects).  The areas are widened to float64 and summed in face order: the stable sort of the faces by           */
/*   component (the caller's) is cut at the multiples of 256 sorted positions and at the component borders, every piece is summed       */
/*   element by element, and a component's pieces are added in order.  No float atomics: two runs give the same bits.                  */
/* Emit, given keep [K] uint8: the valid faces of kept components and the vertices they name, both in input order, faces re-indexed;   */
/*   a vertex no emitted face names is dropped.  A row is copied byte for byte; with world_host12 its xyz is umhs_mesh_vertices'       */
/*   affine of the row's float32 position (csrc/umhs_affine.h).  positions_out holds the model-frame xyz, vertex_map [V] the new index  */
/*   or -1.  Writes beyond vertex_cap rows / face_cap faces are dropped.                                                                */
/* The passes (none allocates or synchronises; arguments are checked first; empty inputs launch nothing):                              */
/*   umhs_components_init    parent [V] int32 = 0 .. V - 1.                                                                             */
/*   umhs_components_rounds  n_rounds <= 32 rounds, 2 launches each; *changed is a uint32 on the device.                                */
/*   umhs_components_roots   root [V] uint8 = (parent[v] == v); ranked with umhs_simplify_flag_count / _rank.                           */
/*   umhs_components_ids     TWO launches: vertex_component [V] = root_rank[parent[v]], face_component [F].                             */
/*   umhs_components_areas   area [F] float32 from positions [V, 3] (umhs_simplify_unpack).                                             */
/*   umhs_components_stats   TWO launches: the pieces (head [umhs_mesh_chunks(F)], first [K] float64 scratch), then one thread per      */
/*                           component: its runs in sorted_face_ids [F] and sorted_vertex_ids [V] by binary search, its pieces added.   */
/*   umhs_components_mark    face_keep [F] uint8, and used [V] uint8 (zeroed by the caller; plain stores of 1).                         */
/*   umhs_components_emit    TWO launches, given the exclusive ranks of face_keep and used: faces_out, then rows_out / positions_out /  */
/*                           vertex_map.                                                                                                */
/* ------------------------------------------------------------------------------------------ */
int umhs_components_init(int32_t* parent, int64_t n_vertices, umhs_stream_t stream);
int umhs_components_rounds(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* parent, uint32_t* changed, int n_rounds,
                           umhs_stream_t stream);
int umhs_components_roots(const int32_t* parent, int64_t n_vertices, uint8_t* root, umhs_stream_t stream);
int umhs_components_ids(const int32_t* parent, const int32_t* root_rank, const int32_t* faces, int64_t n_faces, int64_t n_vertices,
                        int64_t n_components, int32_t* vertex_component, int32_t* face_component, umhs_stream_t stream);
int umhs_components_areas(const float* positions, int64_t n_vertices, const int32_t* faces, int64_t n_faces, float* area,
                          umhs_stream_t stream);
int umhs_components_stats(const int32_t* sorted_face_ids, const int64_t* face_order, const float* area, int64_t n_faces,
                          const int32_t* sorted_vertex_ids, int64_t n_vertices, int64_t n_components, double* head, double* first,
                          int64_t* faces_out, int64_t* vertices_out, double* area_out, umhs_stream_t stream);
int umhs_components_mark(const int32_t* faces, const int32_t* face_component, const uint8_t* keep, int64_t n_faces, int64_t n_vertices,
                         int64_t n_components, uint8_t* face_keep, uint8_t* used, umhs_stream_t stream);
int umhs_components_emit(const void* rows, int row_bytes, const int32_t* faces, const uint8_t* face_keep, const int32_t* face_rank,
                         const uint8_t* used, const int32_t* vertex_rank, int64_t n_faces, int64_t n_vertices, const float* world_host12,
                         void* rows_out, float* positions_out, int64_t vertex_cap, int32_t* faces_out, int64_t face_cap,
                         int32_t* vertex_map, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Optimizer: torch.optim.Adam step for param group "fields" (AdamOptimizerConfig(lr=2e-2,      */
/* eps=1e-15), umhs_config.py:59-64) over one flat fp32 buffer, with the clamp_endmembers        */
/* callback (umhs_model.py:568-572) fused for elements [clamp_begin, clamp_end).  grad_scale     */
/* multiplies the gradient first (1/world_size for averaged DDP gradients).                      */
/* ------------------------------------------------------------------------------------------ */
int umhs_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, int64_t step, float grad_scale, int64_t clamp_begin,
                   int64_t clamp_end, umhs_stream_t stream);
/* The same update on selected 2-float rows of the buffers only (rows: device int64 [n_rows], row r = elements 2r, 2r+1): the   */
/* coarse hash levels use a small fixed subset of their slots; every other row has g = m = v = 0 for ever and is skipped.       */
int umhs_adam_step_rows(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* rows,
                        int64_t n_rows, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                        umhs_stream_t stream);
/* umhs_adam_step_rows on `rows` and umhs_adam_step on elements [range_begin, range_begin + range_count) of the same flat buffers  */
/* (clamp range in absolute elements) in ONE launch: what is left for the optimizer when the dense hash levels were updated by     */
/* umhs_hashgrid_bwd_apply_adam.                                                                                                   */
int umhs_adam_step_rows_range(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* rows,
                              int64_t n_rows, int64_t range_begin, int64_t range_count, float lr, float beta1, float beta2,
                              float eps, int64_t step, float grad_scale, int64_t clamp_begin, int64_t clamp_end,
                              umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Endmember initialisation: the three passes of Vertex Component Analysis (data/utils/vca.py, run by                       */
/* hs_dataloader.py:52-58 on the first frame) that touch every pixel.  rows [N,B] fp32 = pixels of the resident             */
/* hs_image stack, B <= 256, R = n_classes <= 15; the B x B eigen-problem and the R x R pseudo-inverses between the         */
/* passes are host work (umhsnerf/data/utils/vca.py).  Every result is bitwise reproducible (no float atomics).             */
/* umhs_vca_moments: sum[b] (+)= sum_n y_nb, S[i][j] (+)= sum_n y_ni y_nj, float64 [B] / [B,B] (both triangles):            */
/*   fp32 MFMA partials over umhs_vca_rows_per_partial() rows each, combined in float64 in a fixed order; accumulate != 0   */
/*   adds to what sum / S hold (a host-resident stack is fed one frame at a time).  n_rows == 0 writes nothing.             */
/* umhs_vca_project: y [N,16] from rows and basis16 [B,16] fp32.  affine == 0 (vca.py:124-129): columns < R hold Ud,        */
/*   column 15 holds Ud u; y_k = x_k / (x_15 + 1e-6) for k < 15, y_15 = 0.  affine != 0 (:112-116): x = basis^T (row -       */
/*   mean), y = x (the constant R-th component is not stored: see bias below), max_sq[0] = max_n |x_n|^2.                    */
/*   The workspace is needed by the affine form only.                                                                       */
/* umhs_vca_argmax: index[0] = argmax_n |bias + sum_k f[k] y[n][k]|, the lowest n among equal values (numpy.argmax);        */
/*   row[16] = y[index], value[0] = that maximum (optional).  f_host16 is a HOST pointer to 16 floats (passed by value).     */
/* ------------------------------------------------------------------------------------------ */
int umhs_vca_rows_per_partial(void);
size_t umhs_vca_moments_workspace_bytes(int64_t n_rows, int n_bands);
int umhs_vca_moments(const float* rows, int64_t n_rows, int n_bands, int accumulate, double* sum, double* S, void* workspace,
                     size_t workspace_bytes, umhs_stream_t stream);
size_t umhs_vca_project_workspace_bytes(int64_t n_rows);
int umhs_vca_project(const float* rows, int64_t n_rows, int n_bands, const float* basis16, const float* mean, int n_classes,
                     int affine, float* y, float* max_sq, void* workspace, size_t workspace_bytes, umhs_stream_t stream);
size_t umhs_vca_argmax_workspace_bytes(int64_t n_rows);
int umhs_vca_argmax(const float* y, int64_t n_rows, const float* f_host16, float bias, int64_t* index, float* row, float* value,
                    void* workspace, size_t workspace_bytes, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Density-gradient normals (csrc/umhs_normals.hip).  The normal of a density field is the direction of -grad(density); for this  */
/* field the gradient with respect to the WORLD position is analytic.  Per sample, with wpos, pos01 and sel exactly as            */
/* umhs_positions_fwd produces them (the same float32 bits):                                                                      */
/*  1. Grid coordinate and offsets.  As in the hash encode, scaled_l = pos01 * scale_l is ONE float32 product; floor, ceil and    */
/*     offset = scaled - floor are exact.  The cell and the three offsets are DEFINED by those float32 values.                    */
/*  2. Grid derivative.  d enc_{l,f} / d pos01_x = scale_l * (blend over y, z of (f_ceil-x - f_floor-x)) with the forward's y, z  */
/*     weights; y and z follow the same pattern.  Where ceil == floor on an axis (integer coordinate) both corners are the same   */
/*     slot, so that axis' derivative is an exact 0 -- what autograd of the reference expression gives.                           */
/*  3. MLP derivative.  h = W0 enc + b0, sigma_raw = W1[0,:] . relu(h) + b1[0], q = W0^T (1[h > 0] * W1[0,:]) (32 values),        */
/*     g01 = sum_j q_j d enc_j / d pos01 (3 values).                                                                              */
/*  4. Position Jacobian.  contraction == 0: gw = g01 / (aabb_max - aabb_min) per axis.  contraction != 0: pos01 = (c(x) + 2) / 4 */
/*     with c = the L-inf scene contraction.  |x|inf < 1: gw = g01 / 4.  Otherwise, with m = |x_k| the largest component,          */
/*     s = 2/m - 1/m^2 and t = -2/m^2 + 2/m^3:  gw_j = (s g01_j + t (x . g01) sign(x_k) delta_jk) / 4.  Ties of the maximum: the   */
/*     LOWEST index k wins.                                                                                                        */
/*  5. Density gradient.  grad = sel * exp(clamp(sigma_raw, -15, 15)) * gw: what autograd of the reference's density gives         */
/*     through trunc_exp (umhs_field.py:17,327).  sel == 0 gives exactly +0.                                                       */
/*  6. Sample normal.  n = -grad / (|grad| + 1e-10): nerfstudio's -safe_normalize(grad density) [upstream-recalled: nerfstudio    */
/*     1.1.5 Field.get_normals].  sel == 0 gives exactly +0.                                                                       */
/*  7. Per ray (host side, umhs_model.py): N = sum_i w_i n_i with the rendering weights, n^ = N / (|N| + 1e-10)                    */
/*     [upstream-recalled: NormalsRenderer, normalize=True]; the model output is normals = (n^ + 1) / 2 in [0, 1]                  */
/*     [upstream-recalled: NormalsShader without weights, as nerfacto emits it and generate_point_cloud expects before its * 2 - 1];*/
/*     a ray with no samples gives (0.5, 0.5, 0.5).                                                                                */
/* enc: the level-major [L][N][2] features of the same samples, or NULL: the kernel then gathers them itself (the same bits).     */
/* table [16 << log2_T, 2], 16-byte aligned; w0 [64,32], b0 [64], w1 [16,64] (row 0 is read), b1 [16] (element 0 is read): the     */
/* mlp_base of UMHSField and of the rgb field alike.  aabb: 6 HOST floats (contraction == 0).  Outputs [N,3] each, any of them     */
/* NULL (at least one is not): grad_out (5), normal_out (6), g01_out (3; needs neither wpos nor sel).  No workspace, no atomics.   */
/* ------------------------------------------------------------------------------------------ */
int umhs_density_normals(const float* pos01, const float* wpos, const float* sel, const float* enc, const float* table,
                         const float* scalings, int log2_table_size, const float* w0, const float* b0, const float* w1,
                         const float* b1, int contraction, const float* aabb_host6, int64_t n, float* grad_out, float* normal_out,
                         float* g01_out, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Material edits (csrc/umhs_material.hip).  The field mixes a learned dictionary E [C,B]: per sample the spectrum is             */
/* sum_c scalar_c a_c E_c (+ the specular term), and umhs_field_heads_fwd leaves, per ray, mix16[r,c] = sum_n w_n scalar_n,c a_n,c */
/* in its scratch and multiplies by E once per ray.  An edit gives every material c a replacement spectrum E'_c, a gain g_c and a   */
/* density factor d_c, and the specular term one gain s.  A gradient-free render applies them without touching the field kernels:  */
/*  1. Density.  sigma'_n = sigma_n * max(0, 1 + sum_c (d_c - 1) a_n,c), c ascending, float32, with the abundances a of the         */
/*     UNEDITED field (umhs_field_heads_fwd's optional [N,C] output).  All d_c == 1: every term is an exact 0 and sigma' is sigma,   */
/*     bit for bit.  The clamp: a softmax row may sum to 1 + ulp, and all d_c == 0 must not give a negative density.                */
/*  2. Weights, accumulation and depth follow from sigma' by the ordinary transmittance scan (umhs_composite_fwd); the heads pass   */
/*     under those weights gives mix16, the composited specular term and the composited abundances with the model's own E.          */
/*  3. Dictionary.  E''_c = g_c E'_c (host side, one float32 product per element).  mix_term[r,b] = sum_{c<C} mix16[r,c] E''[c,b],  */
/*     an fmaf chain from 0, c ascending.  With the specular head: specular = s * comp_specular (one rounded product),               */
/*     spectral2 = mix_term, spectral = mix_term + specular (one rounded sum).  Without: spectral = mix_term.                        */
/*  Segmentation (umhs_ray_epilogue_fwd) keeps the model's own E and the unedited composited spectrum of step 2: it says which of   */
/*  the ORIGINAL materials is seen, and does not drift with a recoloured dictionary.                                                */
/*                                                                                                                                  */
/* umhs_field_heads_fwd_mix_offset: byte offset of mix16 [n_rays,16] inside the scratch of umhs_field_heads_fwd for the same (cfg,  */
/*   n, n_rays); -1 for a configuration that entry refuses.  Host arithmetic, no launch.  The rows are valid from that call to the  */
/*   next one on the same scratch; columns c >= n_classes hold nothing that may be relied on.                                       */
/* umhs_material_sigma: step 1.  abundances [n,C], density_gain = DEVICE [C], sigma_out [n] (== sigma allowed).  n == 0: UMHS_OK,    */
/*   nothing is launched.  n_classes outside 1..15, n < 0 or a NULL pointer with n > 0: UMHS_ERR_ARG.                                */
/* umhs_material_remix: step 3.  mix16 [R,16] (columns >= n_classes are never read), endmembers_edit = DEVICE [C,B] = E'',            */
/*   comp_specular [R,B] or NULL; with it spectral2 and specular are required (specular == comp_specular allowed), without it both   */
/*   must be NULL (UMHS_ERR_ARG otherwise, before anything is launched).  n_rays == 0: UMHS_OK.  n_bands > 256:                      */
/*   UMHS_ERR_UNSUPPORTED.  The dictionary is staged in LDS, lanes run along the bands (16-byte accesses when n_bands % 4 == 0 and   */
/*   every row array is 16-byte aligned; the same bits either way).  No workspace, no atomics: the same bits on every run.           */
/* ------------------------------------------------------------------------------------------ */
int64_t umhs_field_heads_fwd_mix_offset(const umhs_field_cfg* cfg, int64_t n, int64_t n_rays);
int umhs_material_sigma(const float* sigma, const float* abundances, const float* density_gain, int64_t n, int n_classes,
                        float* sigma_out, umhs_stream_t stream);
int umhs_material_remix(const float* mix16, const float* comp_specular, const float* endmembers_edit, float specular_gain,
                        int64_t n_rays, int n_bands, int n_classes, float* spectral, float* spectral2, float* specular,
                        umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Regional material edits (csrc/umhs_region.hip): the edit above, restricted to boxes and spheres.  THE definition:                */
/*  Regions.  An edit file carries up to UMHS_MAX_REGIONS = 8 regions, each an oriented box -- center T[3], rotation (Euler angles  */
/*   in radians, the convention of the --obb-* options: R = Rz Ry Rx), scale S[3] (full extents, each > 0) -- or a sphere -- center */
/*   T[3], radius r > 0 -- in the MODEL's frame: the frame of --obb-* and of a camera path's crop, what umhs_positions returns as   */
/*   world_pos.  Each region carries a COMPLETE edit of its own (materials and specular_gain, as the top level); it REPLACES the    */
/*   top-level edit for the samples inside it and does not compose with it.  The top-level edit is layer 0, region k is layer k.    */
/*  Region of a sample: the first region in file order that contains its world_pos, numbered 1..K; 0 if none does.  Membership is   */
/*   a decision, so it is exact float32, every step one rounded operation, nothing contracted:  e = p - T;                          */
/*     box:    q_k = (R[k] e0 + R[3+k] e1) + R[6+k] e2  (component k of R^T e, R row-major),  h_k = S_k * 0.5;                      */
/*             inside iff q_k < h_k && q_k > -h_k for k = 0, 1, 2   (the keep rule of the point-cloud export's box);                */
/*     sphere: inside iff (e0 e0 + e1 e1) + e2 e2 < r r.                                                                            */
/*   A point on a face or at the radius is outside.  A NaN position fails every comparison: it is in no region.                     */
/*  Segment: a maximal run of consecutive samples of ONE ray with the same region id.  Rays without samples have no segment.        */
/*   Segments are numbered in sample order; S is their number.  ray_seg[r] = (the number of segments that start before sample      */
/*   packed_info[r,0], the number of segments of ray r).                                                                            */
/*  Density.  sigma'_n = sigma_n * max(0, 1 + sum_c (d[k_n][c] - 1) a_n,c), k_n the sample's layer, the fmaf chain of               */
/*   umhs_material_sigma (c ascending, from 0).                                                                                     */
/*  Weights, accumulation, depth and normals come from sigma' on the REAL ray partition, exactly as for a global edit.              */
/*  Mixing.  umhs_field_heads_fwd uses (ray_indices, packed_info) only as a partition of the sample stream into contiguous runs and */
/*   forms one set of sums per run; handed (seg_of, seg_info, S) with the true per-ray weights it returns mix16, comp_specular,     */
/*   comp_abundances and comp_spectral per SEGMENT, in its one pass.  Per segment j of layer k_j:                                   */
/*     m_j[b] = sum_{c<C} mix16_seg[j,c] E''[k_j][c,b], the fmaf chain from 0 of umhs_material_remix, c ascending.                  */
/*   spectral2[r,b] = the m_j of the ray's segments added in segment order, one rounded add each (the first taken as it is);        */
/*   specular[r,b]  = likewise over s[k_j] * comp_specular_seg[j,b], one rounded product each;                                      */
/*   spectral = spectral2 + specular, one rounded sum; without the specular head spectral is the mixing term.                       */
/*   A ray without segments gives exact zeros.                                                                                      */
/*  Segmentation keeps the model's own dictionary: the unedited per-ray spectrum and the per-ray abundances are the ordered sums    */
/*   (umhs_segment_sum) of the per-segment comp_spectral / comp_abundances rows.                                                    */
/*                                                                                                                                  */
/* umhs_region_classify: world_pos [n,3]; regions_host16 = HOST [n_regions,16] = T[3], R[9] row-major, S[3] (sphere: r in S[0]),    */
/*   kind (0 box, 1 sphere), copied at the call; region [n] uint8.  n_regions 0..8 (0: every id is 0).                              */
/* umhs_region_segments: region [n], ray_indices [n] non-decreasing, packed_info [R,2] -> seg_of [n] int64 (non-decreasing: what    */
/*   umhs_field_heads_fwd takes as ray_indices), seg_info [S,2] int64 (first sample, count: what it takes as packed_info),          */
/*   seg_layer [S] int32, ray_seg [R,2] int64, n_segments = DEVICE int64 [1] = S.  seg_info and seg_layer need room for n rows      */
/*   (S <= n); rows >= S are not written.  Head flags, one ordered scan of the per-block counts, writes: four launches, integers    */
/*   only, no atomics, the same bytes on every run.  workspace: umhs_region_segments_workspace_bytes(n), 8-byte aligned             */
/*   (UMHS_ERR_WORKSPACE otherwise).  n == 0 or n_rays == 0: nothing is launched and nothing written (S is 0: the caller's).       */
/* umhs_material_sigma_regions: umhs_material_sigma with region [n] and density_gain = DEVICE [(n_regions+1), C].                   */
/* umhs_segment_sum: values [S,k] -> out [R,k], out[r] = the rows ray_seg[r] names added in order (none: zeros).  k 1..256.         */
/* umhs_material_remix_regions: mix16_seg [S,16] (columns >= n_classes never read), comp_specular_seg [S,B] or NULL, seg_layer,     */
/*   ray_seg, endmembers_edit = DEVICE [(n_regions+1),C,B], specular_gain = DEVICE [n_regions+1] (required with comp_specular_seg)  */
/*   -> spectral, spectral2, specular [R,B]; the NULL rules of umhs_material_remix, and an output may not be an input array.        */
/*   Lanes run along the bands (16-byte accesses when B % 4 == 0 and every row array is 16-byte aligned); as many whole layers of   */
/*   the dictionary as fit the launch's dynamic LDS are staged there, the others are read through the cache.  The same bits either  */
/*   way.  Segment numbers read from ray_seg / seg_layer are clamped into what exists.                                              */
/* All five: n or n_rays == 0 returns UMHS_OK and launches nothing; a NULL pointer, n_regions outside 0..8 or n_classes outside    */
/*   1..15: UMHS_ERR_ARG before any launch; n_bands or k > 256: UMHS_ERR_UNSUPPORTED.                                               */
/* ------------------------------------------------------------------------------------------ */
#define UMHS_MAX_REGIONS 8
int umhs_region_classify(const float* world_pos, int64_t n, const float* regions_host16 /* HOST */, int n_regions, uint8_t* region,
                         umhs_stream_t stream);
size_t umhs_region_segments_workspace_bytes(int64_t n);
int umhs_region_segments(const uint8_t* region, const int64_t* ray_indices, const int64_t* packed_info, int64_t n, int64_t n_rays,
                         int64_t* seg_of, int64_t* seg_info, int32_t* seg_layer, int64_t* ray_seg, int64_t* n_segments /* DEVICE [1] */,
                         void* workspace, size_t workspace_bytes, umhs_stream_t stream);
int umhs_material_sigma_regions(const float* sigma, const float* abundances, const uint8_t* region, const float* density_gain,
                                int64_t n, int n_classes, int n_regions, float* sigma_out, umhs_stream_t stream);
int umhs_segment_sum(const float* values, const int64_t* ray_seg, int64_t n_segments, int64_t n_rays, int k, float* out,
                     umhs_stream_t stream);
int umhs_material_remix_regions(const float* mix16_seg, const float* comp_specular_seg, const int32_t* seg_layer,
                                const int64_t* ray_seg, const float* endmembers_edit, const float* specular_gain, int64_t n_segments,
                                int64_t n_rays, int n_bands, int n_classes, int n_regions, float* spectral, float* spectral2,
                                float* specular, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Segment statistics (csrc/umhs_stats.hip): what the stand-alone trainer's --log-gradients reads off the flat gradient, in one     */
/* pass.  x [n] float32 (any 4-byte aligned address); bounds = DEVICE int64 [n_segments + 1], ascending element offsets, segment k   */
/* = [bounds[k], bounds[k+1]) at any element offset (equal neighbours: an empty segment); bounds_host = the same values in HOST      */
/* memory, read by the argument checks and the grid size only.  out = DEVICE float64 [n_segments, 3], per segment                    */
/*   [0] the sum of x^2 over the finite elements   [1] the maximum of |x| over the finite elements   [2] the number of NaN / +-Inf   */
/* (an empty segment: 0, 0, 0).  Elements outside [bounds[0], bounds[n_segments]) are never read.                                    */
/* Arithmetic: x^2 is exact in float64; sums are float64 over a partition fixed by (n, bounds): tiles of umhs_segment_stats_tile()   */
/* elements counted from each segment's start (none straddles a boundary), per-tile partials in the workspace, one wave per segment  */
/* adding its partials in index order.  No atomics: the same input gives the same bits on every launch.  An element passes through   */
/* at most 34 + 6 + 3 + ceil(ceil(len / tile) / 64) + 6 additions, so the sum is within that many times 2^-53 (relative) of the      */
/* exact one; the maximum and the count are exact.  The kernel clamps every offset it reads into [0, n].                             */
/* Errors, before anything is launched: n < 0, n_segments < 1, a NULL pointer, bounds_host descending, bounds_host[0] < 0 or         */
/* bounds_host[n_segments] > n: UMHS_ERR_ARG; a workspace below umhs_segment_stats_workspace_bytes(n, n_segments):                   */
/* UMHS_ERR_WORKSPACE.  Two launches on the stream (tiles, finish); no allocation, no synchronisation.                               */
/* ------------------------------------------------------------------------------------------ */
size_t umhs_segment_stats_workspace_bytes(int64_t n, int n_segments);
int umhs_segment_stats_tile(void);
int umhs_segment_stats(const float* x, int64_t n, const int64_t* bounds, const int64_t* bounds_host, int n_segments, double* out,
                       void* workspace, size_t workspace_bytes, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Baseline-JPEG frame encoder (csrc/umhs_jpeg.hip): the composed frame uint8 [height, width, 3] (what umhs_frame_compose writes,      */
/* at ANY byte address) -> one complete JFIF file in a caller-provided DEVICE buffer.  height, width 1..65535 and restart_mcus          */
/* 1..65535 (larger: UMHS_ERR_UNSUPPORTED); quality 1..100; subsampling UMHS_JPEG_444 or UMHS_JPEG_420.                                 */
/* The file, in this order: SOI; APP0/JFIF 1.01, density 1 x 1 without unit; two DQT (8-bit, zigzag order: table 0 luminance, 1         */
/* chrominance); SOF0 with three components, ids 1 / 2 / 3, sampling 0x11 or 0x22 for Y and 0x11 for Cb / Cr, tables 0 / 1 / 1; four     */
/* DHT, the typical tables of Annex K (DC 0, AC 0, DC 1, AC 1); DRI = restart_mcus; SOS; the entropy-coded data, RSTm (m counts modulo  */
/* 8) between restart intervals; EOI.  The header is 629 bytes and depends on (height, width, quality, subsampling, restart_mcus) only. */
/* Quantisation tables: libjpeg's scaling of the Annex-K tables, s = 5000 / quality below 50, else 200 - 2 quality (integers);          */
/* (base * s + 50) / 100, clamped to 1..255.                                                                                            */
/* Stage A, the transform.  The result is integers, so the arithmetic is fixed to the bit: every operation below is ONE rounded float32  */
/* operation and nothing is contracted into an fma.                                                                                     */
/*   padding : a pixel outside the frame reads (min(y, height - 1), min(x, width - 1)).                                                 */
/*   colour  : Y  = ((0.299 R + 0.587 G) + 0.114 B) - 128                                                                               */
/*             Cb = ((-0.168736 R) + (-0.331264 G)) + 0.5 B          Cr = (0.5 R + (-0.418688 G)) + (-0.081312 B)                       */
/*             (chroma's +128 and the level shift cancel; nothing is rounded to 8 bits in between).                                     */
/*   4:2:0   : a chroma sample is ((a + b) + (c + d)) * 0.25 over its 2 x 2 pixels, a b the upper row.                                  */
/*   DCT     : direct form, T[u][x] = fl32(1/2 c(u) cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt 2, else 1.  Row pass G[y][v] = sum_x       */
/*             f[y][x] T[v][x], summed in ascending x from the first product; column pass F[u][v] = sum_y T[u][y] G[y][v], in           */
/*             ascending y the same way.                                                                                                */
/*   quantise: v = F / Q; k = sign(v) trunc(|v| + 0.5); AC clamped to +-1023, DC to [-1024, 1023].                                      */
/* umhs_jpeg_coefficients exports this stage: int16 [n_mcus, blocks per MCU, 64], 16-byte aligned: MCUs in raster order, the blocks     */
/* of an MCU in scan order (4:4:4: Y Cb Cr; 4:2:0: Y00 Y01 Y10 Y11 Cb Cr), the 64 values in zigzag order.  umhs_jpeg_blocks: n_mcus *   */
/* blocks per MCU.                                                                                                                      */
/* Stage B, entropy coding, on the device.  A restart interval (restart_mcus MCUs in raster order, across MCU rows; the last may be     */
/* shorter) is an independent byte-aligned piece: DC prediction restarts at 0 for each component, bits are packed MSB first, the last   */
/* partial byte is padded with 1-bits, every 0xFF data byte is followed by 0x00.  The stream is a function of the coefficients alone:   */
/* no launch geometry, wave scheduling or atomic order enters it.  umhs_jpeg_entropy runs this stage on given coefficients (values      */
/* outside the clamps above are clamped into them); umhs_jpeg_encode runs both.                                                         */
/* *length (DEVICE int64) receives the length of the file.  Nothing is written at or past out[capacity]: when *length > capacity the   */
/* buffer holds the first `capacity` bytes and *length is the size needed.  umhs_jpeg_max_bytes is an upper bound on *length for ANY    */
/* content (every block at 1,660 bits, every byte stuffed).  The workspace (umhs_jpeg_workspace_bytes, 16-byte aligned: the             */
/* coefficients and 8 bytes per interval; umhs_jpeg_entropy alone needs the 8 bytes per interval, 8-byte aligned) does not depend on    */
/* the content.  Four launches (transform; interval lengths; scan + header; write); no allocation, no synchronisation.                  */
/* ------------------------------------------------------------------------------------------ */
enum { UMHS_JPEG_444 = 0, UMHS_JPEG_420 = 1 };
size_t umhs_jpeg_workspace_bytes(int height, int width, int subsampling, int restart_mcus);
size_t umhs_jpeg_max_bytes(int height, int width, int subsampling, int restart_mcus);
int64_t umhs_jpeg_blocks(int height, int width, int subsampling);
int umhs_jpeg_coefficients(const uint8_t* frame, int height, int width, int quality, int subsampling, int16_t* coefficients,
                           umhs_stream_t stream);
int umhs_jpeg_entropy(const int16_t* coefficients, int height, int width, int quality, int subsampling, int restart_mcus, uint8_t* out,
                      int64_t capacity, int64_t* length, void* workspace, size_t workspace_bytes, umhs_stream_t stream);
int umhs_jpeg_encode(const uint8_t* frame, int height, int width, int quality, int subsampling, int restart_mcus, uint8_t* out,
                     int64_t capacity, int64_t* length, void* workspace, size_t workspace_bytes, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* PNG frame encoder (csrc/umhs_png.hip): a frame uint8 [height, width, channels] (channels 3: RGB, colour type 2; 1: grey, colour     */
/* type 0; bit depth 8, no interlace; at ANY byte address) -> one complete PNG file in a caller-provided DEVICE buffer.  height,        */
/* width and stripe_rows 1..65535 (larger: UMHS_ERR_UNSUPPORTED, as is a piece -- stripe_rows rows -- so large that its chunk could     */
/* pass PNG's 2^31 - 1 bytes).  THE definition of the stream:                                                                           */
/* Stage A, filtering.  Row y becomes 1 + width * channels bytes: the filter type t, then x - predictor_t (mod 256) of every byte, with */
/*   a the byte `channels` to the left, b the byte above, c the byte above a; bytes left of the row and above row 0 are 0.  Types:      */
/*   0 None (0), 1 Sub (a), 2 Up (b), 3 Average ((a + b) >> 1 on the 9-bit sum), 4 Paeth (p = a + b - c; the one of a, b, c nearest to  */
/*   p, ties in the order a, b, c).  filter = UMHS_PNG_FILTER_NONE .. _PAETH uses that type for every row; UMHS_PNG_FILTER_ADAPTIVE      */
/*   gives each row the type whose cost, the sum of min(f, 256 - f) over its filtered bytes f, is least, the smallest type on ties.     */
/*   umhs_png_filter exports this stage: uint8 [height, 1 + width * channels].                                                          */
/* Stage B, deflate with matches of distance 1 only.  The filtered bytes of stripe_rows consecutive rows (the last piece may have      */
/*   fewer) are one piece, a flat byte string; pieces are independent.                                                                  */
/*   Tokens: a maximal run of n equal bytes inside the piece (it may cross rows) is one literal, then, with m = n - 1 bytes left,       */
/*   matches of distance 1 and length min(m, 258) while m >= 3, then the last 0..2 bytes as literals.                                   */
/*   Code lengths of the literal/length alphabet, from the piece's histogram with end-of-block counted once: the used symbols are       */
/*   sorted by (count, symbol); a two-queue Huffman merge (the sorted leaves in one queue, merged nodes in the order they are made in   */
/*   the other; each step joins the two lightest queue heads, the leaf first when a leaf and a node weigh the same) gives every leaf a  */
/*   depth; N[l] = leaves at depth l, depths above 15 counted at 15; K = sum N[l] 2^(15 - l) - 2^15; while K > 0, one leaf of the       */
/*   largest l < 15 with N[l] > 0 moves to l + 1 (K -= 2^(14 - l)); while K < 0, one leaf of level 15 moves to 14 (K += 1); then the    */
/*   sorted symbols take the levels from the deepest: the first N[15] get length 15, the next N[14] length 14, ...  Codes are           */
/*   canonical (RFC 1951 3.2.2).                                                                                                        */
/*   Bits of a piece, packed least significant bit first, Huffman codes most significant bit first, extra bits least significant first: */
/*   BFINAL 0, BTYPE 2, HLIT = (last used symbol + 1) - 257, HDIST 0, HCLEN 15; the 19 code-length-code lengths 0 0 0 4 4 .. 4 (symbols  */
/*   16 17 18 unused, 0..15 four bits each, so a length's code is the length itself); HLIT + 257 lengths; the distance tree's single    */
/*   length 1; the tokens (a match: length code, its extra bits, the 1-bit distance code 0); end of block; an empty stored block: 000,  */
/*   zero bits to the byte, 00 00 FF FF.  Every piece therefore ends on a byte.                                                         */
/* The file: the 8-byte signature; IHDR; one IDAT per piece, in order -- the first one's data begins with the zlib header 78 01, the   */
/*   last one's ends with 03 00 (an empty final fixed block) and the Adler-32 of all filtered bytes; IEND.  A chunk is its data length, */
/*   type, data and the CRC-32 of type and data.  The file is a function of the pixels and (channels, filter, stripe_rows) alone: no    */
/*   launch geometry, wave scheduling or atomic order enters it.  umhs_png_deflate runs stage B and the container on GIVEN filtered     */
/*   rows (any type bytes); umhs_png_encode runs both stages.                                                                           */
/* *length (DEVICE int64) receives the length of the file.  Nothing is written at or past out[capacity]: when *length > capacity the   */
/* buffer holds the first `capacity` bytes and *length is the size needed.                                                              */
/* umhs_png_max_bytes is an upper bound on *length for ANY content: per piece of n bytes 74 + 4 * 287 header bits, 15 bits per byte (a  */
/* code is at most 15 bits; a match spends at most 15 + 5 + 1 on three bytes or more), 15 + 3 bits, the rounding, 4 bytes; 12 per       */
/* chunk; 33 + 2 + 6 + 12 around them.  The workspace (umhs_png_workspace_bytes, 16-byte aligned: the filtered rows rounded up to 16    */
/* bytes, then 1,184 bytes per piece; umhs_png_deflate alone takes the 1,184 bytes per piece, 8-byte aligned) does not depend on the    */
/* content.  Five launches (filter; piece statistics and codes; scan + container; write; chunk CRCs), four for umhs_png_deflate; no     */
/* allocation, no synchronisation.                                                                                                      */
/* ------------------------------------------------------------------------------------------ */
enum {
  UMHS_PNG_FILTER_NONE = 0,
  UMHS_PNG_FILTER_SUB = 1,
  UMHS_PNG_FILTER_UP = 2,
  UMHS_PNG_FILTER_AVERAGE = 3,
  UMHS_PNG_FILTER_PAETH = 4,
  UMHS_PNG_FILTER_ADAPTIVE = 5
};
size_t umhs_png_workspace_bytes(int height, int width, int channels, int stripe_rows);
size_t umhs_png_max_bytes(int height, int width, int channels, int stripe_rows);
int umhs_png_filter(const uint8_t* frame, int height, int width, int channels, int filter, uint8_t* filtered, umhs_stream_t stream);
int umhs_png_deflate(const uint8_t* filtered, int height, int width, int channels, int stripe_rows, uint8_t* out, int64_t capacity,
                     int64_t* length, void* workspace, size_t workspace_bytes, umhs_stream_t stream);
int umhs_png_encode(const uint8_t* frame, int height, int width, int channels, int filter, int stripe_rows, uint8_t* out,
                    int64_t capacity, int64_t* length, void* workspace, size_t workspace_bytes, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Spectral library matching (csrc/umhs_library.hip): for every ray the two entries of a spectral library whose spectral angle to    */
/* the ray's spectrum is smallest (SAM classification), without ever forming the [R,L] matrix.  THE definition:                      */
/*  Inputs.  spectra: float32 rows [R] of B bands, row r at spectra + r * stride floats (stride >= B; a column slice of a wider       */
/*   array works; any 4-byte aligned address; columns >= B of a row are never read).  unit: float32 [L,B], the library rows ALREADY  */
/*   of unit length (the host normalises in float64 and rounds once).  1 <= B <= 256, 1 <= L <= 65,536.                               */
/*  Arithmetic, all float32:                                                                                                          */
/*   dot[r,l] = the fmaf chain  fmaf(s_b, e_b, .)  over b ascending from 0, starting at +0;                                           */
/*   ss[r]    = the same chain of s_b s_b;                                                                                            */
/*   cos[r,l] = dot[r,l] / sqrtf(ss[r]), division and root correctly rounded.                                                         */
/*   The value for (r, l) does not depend on where l sits in the library: two identical rows give identical bits.                     */
/*  Outputs.  index int32 [R,2] and cos float32 [R,2]: the entry of largest cosine and the one of second largest, ordered by          */
/*   (cosine descending, index ascending): ties go to the smaller index, and the second is another entry than the first.  A NaN       */
/*   cosine never wins (nor does one of -Inf).  With L == 1 (or no second candidate) the second is (-1, -1.0f).  A row whose ss is   */
/*   0, NaN or +Inf -- an empty pixel, a NaN or an Inf anywhere in it -- gives index (-1, -1) and cos (0, 0), exactly; so does a      */
/*   row for which no entry has a cosine above -Inf.                                                                                  */
/*  A float32 cosine near 1 moves in steps of 6e-8, i.e. it does not resolve angles below about 1e-3 rad: entries closer to each      */
/*   other than that tie, and the earlier one wins.                                                                                   */
/*                                                                                                                                    */
/* umhs_library_image_bytes: size of the operand image of an (L, B) library, at least L * B * 4; 0 for an (L, B) outside the limits.  */
/* umhs_library_prepare: unit [L,B] -> image, the rows re-laid once (zero padded to 32 entries and 2 bands) as the matrix-core        */
/*   operand the match kernel streams.  One launch.                                                                                   */
/* umhs_library_match: one launch, no workspace, no atomics: the same bits on every run.                                              */
/* Errors, before anything is launched: L < 1, B < 1, R < 0, stride < B: UMHS_ERR_ARG; B > 256 or L > 65,536: UMHS_ERR_UNSUPPORTED;   */
/*   then R == 0: UMHS_OK whatever the pointers; then a NULL pointer: UMHS_ERR_ARG.                                                   */
/* ------------------------------------------------------------------------------------------ */
size_t umhs_library_image_bytes(int n_entries, int n_bands);
int umhs_library_prepare(const float* unit, int n_entries, int n_bands, float* image, umhs_stream_t stream);
int umhs_library_match(const float* spectra, int64_t stride, int64_t n_rays, const float* image, int n_entries, int n_bands,
                       int32_t* index, float* cosine, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Scene statistics (csrc/umhs_statistics.hip): the count, the sum and the Gram matrix of a scene's valid spectra about a fixed      */
/* shift -- what a mean and a B x B covariance are made of -- and the centred projection y = W (x - mean) that turns them into       */
/* principal components and RX (Mahalanobis) scores.  THE definition:                                                                */
/*  Inputs of both.  spectra: float32 rows [R] of B bands, row r at spectra + r * stride floats, by the rules of                     */
/*   umhs_library_match (stride >= B, any 4-byte aligned address, columns >= B of a row are never read).  1 <= B <= 256, R >= 0.     */
/*                                                                                                                                    */
/* umhs_gram_accumulate.  shift: float32 [B], fixed by the caller for the whole accumulation.  accumulation: float32 [R] or NULL.    */
/*   acc: float64 [1 + B + B B] = (count, s[B], G[B,B]), zeroed by the caller before the first call; calls add to it.                */
/*  A row is VALID when every one of its B values is finite and accumulation is NULL or accumulation[r] > 0.5 (the rule of           */
/*   seg_pred).  An invalid row contributes exactly nothing and is not counted.                                                       */
/*  Arithmetic.  c[r,b] = x[r,b] - shift[b], one float32 subtraction.  The call's rows are cut into chunks of UMHS_GRAM_CHUNK rows:  */
/*   chunk j is rows [j CH, (j + 1) CH) of THIS call.  Within a chunk g[a,b] is the float32 fmaf chain  fmaf(c[r,a], c[r,b], .)      */
/*   over the valid r ascending, starting at +0, and s[b] the float32 sum of c[r,b] in the same order.  The chunk results are added  */
/*   to acc in float64, chunks ascending: acc[0] += count, acc[1 + b] += s[b], acc[1 + B + a B + b] += g[a,b].                        */
/*   g[a,b] and g[b,a] are the same bits (one triangle is computed and mirrored), so G stays exactly symmetric.                      */
/*  No atomics; nothing depends on the grid or on occupancy: the same bits on every run and on every device.                         */
/*  Workspace: umhs_gram_workspace_bytes(R, B) = min(ceil(R / CH), 512) (1 + B + B B) 4 bytes, 4-byte aligned, plain scratch: it     */
/*   grows with R up to 512 chunks and then stays (34 MB at B = 128, 135 MB at B = 256); 0 for R < 1 or a B outside the limits.      */
/*   Two launches per 512 chunks (chunk partials; their float64 sum onto acc).                                                       */
/*  Errors, before anything is launched: B < 1, R < 0, stride < B: UMHS_ERR_ARG; B > 256: UMHS_ERR_UNSUPPORTED; then R == 0:          */
/*   UMHS_OK whatever the pointers; then a NULL spectra, shift, acc or workspace, or a workspace too small: UMHS_ERR_ARG.             */
/*                                                                                                                                    */
/* umhs_spectral_project.  mean: float32 [B].  image: the operand image umhs_library_prepare makes from W [K,B] float32              */
/*   (umhs_library_image_bytes(K, B) bytes).  1 <= K <= 256, 0 <= P <= K.                                                             */
/*  Arithmetic, all float32.  c[b] = x[r,b] - mean[b], one subtraction;  y[r,k] = the fmaf chain  fmaf(c[b], W[k,b], .)  over b       */
/*   ascending from +0 (the dot of umhs_library_match, on the centred row);  score[r] = the fmaf chain  fmaf(y[r,k], y[r,k], .)       */
/*   over k ascending from +0, all K components.                                                                                      */
/*  Outputs.  components: float32 [R,P], y for k < P (NULL allowed when P == 0).  score: float32 [R] (NULL allowed: not computed).   */
/*   A row with a NaN or an Inf anywhere (or whose centred value overflows) gives exactly 0 in both.                                  */
/*  One launch, no workspace, no atomics: the same bits on every run.                                                                 */
/*  Errors, before anything is launched: B < 1, K < 1, R < 0, stride < B, P < 0 or P > K: UMHS_ERR_ARG; B or K > 256:                 */
/*   UMHS_ERR_UNSUPPORTED; then R == 0: UMHS_OK whatever the pointers; then a NULL spectra, mean or image, or a NULL components with  */
/*   P > 0: UMHS_ERR_ARG.                                                                                                             */
/* ------------------------------------------------------------------------------------------ */
#define UMHS_GRAM_CHUNK 1024
int umhs_gram_chunk(void); /* UMHS_GRAM_CHUNK, for callers that cannot read this header */
size_t umhs_gram_workspace_bytes(int64_t n_rows, int n_bands);
int umhs_gram_accumulate(const float* spectra, int64_t stride, int64_t n_rows, int n_bands, const float* shift, const float* accumulation,
                         double* acc, void* workspace, size_t workspace_bytes, umhs_stream_t stream);
int umhs_spectral_project(const float* spectra, int64_t stride, int64_t n_rows, const float* mean, const float* image, int n_components,
                          int n_bands, int n_stored, float* components, float* score, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Spectral unmixing (csrc/umhs_unmix.hip): classical constrained linear unmixing of every row against K endmembers E [K,B]: the     */
/* abundances a >= 0 that minimise |x - E^T a|^2 (NNLS), with sum a = 1 as well (FCLS).  THE definition:                             */
/*  Inputs.  spectra: float32 rows [R] of B bands, row r at spectra + r * stride floats, by the rules of umhs_library_match          */
/*   (stride >= B, any 4-byte aligned address, columns >= B of a row are never read).  image: the operand image                      */
/*   umhs_library_prepare makes from E [K,B] float32, NOT normalised.  gram: float32 [K,K] = E E^T, formed on the host in float64    */
/*   from the float32 E and rounded once.  mode: UMHS_UNMIX_NNLS or UMHS_UNMIX_FCLS.  1 <= B <= 256, 1 <= K <= 16, R >= 0.            */
/*  ss = (the fmaf chain of x_b x_b over the even b ascending from +0) + (the same chain over the odd b).  A row is INVALID when ss  */
/*   is 0, NaN or +Inf -- an empty pixel, a NaN or an Inf anywhere in it, a sum of squares that overflows.  It gives abundances of   */
/*   exact +0, residual 0 and status -1.                                                                                              */
/*  Arithmetic, all float32.  b[k] = the fmaf chain  fmaf(E[k,b], x_b, .)  over b ascending from +0 (the dot of umhs_library_match).  */
/*   The normal equations (gram, b) are solved per row by an active-set method (Lawson-Hanson) on a symmetric sweep tableau M = gram  */
/*   with two right-hand columns, b and ones:                                                                                         */
/*    sweep(k)  p = M_kk, r = 1 / p;  M_ij = fmaf(-(M_ik r), M_kj, M_ij) for all i, j != k, columns included;  row k becomes          */
/*              M_kj r when k enters the passive set P and -M_kj r when it leaves;  M_kk = -r.  With P swept in, column b holds       */
/*              u = G_PP^-1 b_P on P and b - G u off P; column ones holds v = G_PP^-1 1 on P and 1 - G v off P.  An index whose pivot  */
/*              is not positive does not enter.                                                                                       */
/*    solve     lambda = (sum u - 1) / sum v for FCLS, 0 for NNLS (sums over P ascending);  z = u - lambda v on P.                     */
/*    start     every endmember in P (swept in ascending);  a = 0 (NNLS) or 1 / K (FCLS).                                             */
/*    step      if some z_i <= 0, i in P:  alpha = min(1, min a_i / (a_i - z_i)) over them, a_i = max(0, a_i + alpha (z_i - a_i)) on  */
/*              P, the first minimiser's a_i = 0, and every such i with a_i <= 0 leaves P.  Otherwise a = z, and the index off P      */
/*              (ties: the smallest) of largest w_i = (column b)_i - lambda (column ones)_i enters if w_i > 2^-21 max_k |b[k]|; if    */
/*              none does, the row is done and status = the number of solves.                                                         */
/*    guard     an index that enters and has z <= 0 at the next solve leaves again and cannot enter until another one has entered     */
/*              and stayed (the anti-cycling rule).                                                                                   */
/*    cap       3 K + 3 solves.  A row that would need another one returns its last feasible a with status -2.  A row never hangs.    */
/*   Every returned a_k is finite and >= +0: whatever is not in (0, FLT_MAX] is written as +0.                                        */
/*   residual = max(0, ss - 2 b.a + a.(gram a)), chains over k ascending: |x - E^T a|^2 up to rounding relative to ss.                */
/*  Outputs.  abundances: float32 [R,K].  residual: float32 [R] or NULL.  status: int32 [R] or NULL.                                  */
/*  One launch, no atomics, nothing depends on the grid: the same bits on every run, and the bits of row r depend neither on R nor    */
/*   on the other rows.  umhs_unmix_workspace_bytes is 0 (the tableau lives in LDS); workspace may be NULL.                           */
/*  Conditioning is the CALLER's: float32 normal equations lose cond_2(gram) u of the abundances (umhsnerf.unmix refuses endmember    */
/*   sets for which that exceeds 0.01).                                                                                               */
/*  Errors, before anything is launched: B < 1, K < 1, R < 0, stride < B, a mode that is neither: UMHS_ERR_ARG; B > 256 or K > 16:    */
/*   UMHS_ERR_UNSUPPORTED; then R == 0: UMHS_OK whatever the pointers; then a NULL spectra, image, gram or abundances: UMHS_ERR_ARG.  */
/* ------------------------------------------------------------------------------------------ */
enum { UMHS_UNMIX_NNLS = 0, UMHS_UNMIX_FCLS = 1 };
#define UMHS_UNMIX_MAX_ENDMEMBERS 16
size_t umhs_unmix_workspace_bytes(int64_t n_rows, int n_endmembers, int n_bands);
int umhs_unmix(const float* spectra, int64_t stride, int64_t n_rows, const float* image, const float* gram, int n_endmembers, int n_bands,
               int mode, float* abundances, float* residual, int32_t* status, void* workspace, size_t workspace_bytes,
               umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Continuum removal (csrc/umhs_continuum.hip): every row divided by its continuum -- the upper convex hull of the spectrum over      */
/* wavelength -- and depth, centre and area of up to 8 absorption features.  THE definition:                                          */
/*  Inputs.  spectra: float32 rows [R] of B bands, row r at spectra + r * stride floats, by the rules of umhs_library_match          */
/*   (stride >= B, any 4-byte aligned address, columns >= B of a row are never read).  wavelengths: DEVICE float32 [B], finite and    */
/*   strictly increasing (the CALLER's to check).  feature_ranges: HOST int32 [F][2], inclusive band indices lo <= hi of at least 3   */
/*   bands; they travel as kernel arguments (no copy, no sync).  1 <= B <= 256, 0 <= F <= 8, R >= 0.                                  */
/*  A row is INVALID when it holds a NaN or an Inf in any of its B bands: removed 0, every feature number 0, status -1.               */
/*  Continuum over a band range [lo, hi]: the upper convex hull of the points (lambda_b, x_b), lo <= b <= hi, by the monotone chain   */
/*   left to right: before b is pushed the last vertex p1 is popped while, with p0 the vertex under it,                               */
/*    cross = (l1 - l0) * (x_b - x0) - (x1 - x0) * (l_b - l0)                                                                         */
/*   is not < 0 (the turn p0 -> p1 -> b is not strictly clockwise): points on or below the chord are dropped, the vertices are        */
/*   strict, lo and hi are always vertices.  Between consecutive vertices i < j,                                                      */
/*    c_b = x_i + ((l_b - l_i) / (l_j - l_i)) * (x_j - x_i),   and c_b = x_b at a vertex.                                             */
/*   A range of one band has c = x.  r_b = x_b / c_b where c_b > 0, else r_b = 1 (so r = 1 at every vertex of a finite row).          */
/*  Arithmetic: float32, every operation above and below rounded once, in the order written (nothing is contracted to an fma).        */
/*  removed [R,B]: r over the FULL range [0, B - 1].  status [R]: the number of vertices of the full-range hull (-1: invalid).        */
/*  features [R,F,3]: feature f uses the LOCAL hull over its own range, independent of the rest of the row:                           */
/*    depth  = 1 - min_b r_b                                                                                                          */
/*    centre = l_m, m the first band attaining that minimum (l_lo where the depth is 0)                                               */
/*    area   = the trapezoid rule of q = 1 - r:  from +0, for b = lo + 1 .. hi:  area += (0.5 * (l_b - l_{b-1})) * (q_{b-1} + q_b)    */
/*  Outputs.  removed, features, status: each may be NULL (features NULL: as F = 0).  The full-range hull is skipped when neither     */
/*   removed nor status is wanted.                                                                                                    */
/*  One launch, no atomics, nothing depends on the grid: the same bits on every run, and the bits of row r depend neither on R, nor   */
/*   on the other rows, nor on the row's place, nor on stride.  umhs_continuum_workspace_bytes is 0 (rows, hull stacks and            */
/*   wavelengths live in LDS); workspace may be NULL.                                                                                 */
/*  Errors, before anything is launched and without touching the device, all UMHS_ERR_ARG: B outside 1..256, F outside 0..8, R < 0,  */
/*   stride < B, F > 0 with a NULL feature_ranges; a range with lo < 0, hi >= B, lo > hi or fewer than 3 bands; then R == 0:          */
/*   UMHS_OK whatever the pointers; then a NULL spectra or wavelengths.                                                               */
/* ------------------------------------------------------------------------------------------ */
#define UMHS_CONTINUUM_MAX_BANDS 256
#define UMHS_CONTINUUM_MAX_FEATURES 8
size_t umhs_continuum_workspace_bytes(int64_t n_rows, int n_bands, int n_features);
int umhs_continuum(const float* spectra, int64_t stride, int64_t n_rows, const float* wavelengths, int n_bands,
                   const int32_t* feature_ranges, int n_features, float* removed, float* features, int32_t* status, void* workspace,
                   size_t workspace_bytes, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Spectral clustering (csrc/umhs_cluster.hip): one pass of Lloyd's algorithm (k-means, or spherical k-means by spectral angle) over  */
/* the rows: every row is given the nearest of K centres and, in the same pass, the rows of each cluster are summed.  THE definition: */
/*  Inputs.  spectra: float32 rows [R] of B bands, row r at spectra + r * stride floats, by the rules of umhs_library_match          */
/*   (stride >= B, any 4-byte aligned address, columns >= B of a row are never read).  mask: float32 [R] or NULL.  image: the         */
/*   operand image umhs_library_prepare makes from the centres c [K,B] float32 (umhs_library_image_bytes(K, B) bytes): for ANGLE     */
/*   rows ALREADY of unit length (the host normalises in float64 and rounds once), for EUCLIDEAN the centres as they are.            */
/*   half_norm: float32 [K] = |c_k|^2 / 2, formed on the host in float64 from the float32 centres and rounded once; NULL for ANGLE   */
/*   (it is not read).  1 <= B <= 256, 1 <= K <= UMHS_CLUSTER_MAX, R >= 0.                                                            */
/*  Per row, all float32.  dot[r,k] = the fmaf chain  fmaf(x_b, c_kb, .)  over b ascending from +0 and ss[r] = the same chain of     */
/*   x_b x_b: exactly the chains of umhs_library_match.  A row is INVALID when ss is 0, NaN or +Inf -- an empty pixel, a NaN or an   */
/*   Inf anywhere in it, a sum of squares that overflows -- or when mask is given and mask[r] <= 0.5.  An invalid row gives          */
/*   label -1 and score 0, and contributes exactly nothing to acc.                                                                    */
/*   ANGLE      c_k = dot[r,k] / sqrtf(ss), division and root correctly rounded.  label = the k of largest c_k; ties go to the        */
/*              smaller index; a NaN never wins, nor does -Inf: a row for which no k has c_k > -Inf is invalid as above.              */
/*              score = c_label.  (These are the bits of index[r,0] and cos[r,0] of umhs_library_match on the same image.)           */
/*              member vector v[r,b] = x[r,b] / sqrtf(ss), one correctly rounded division;  objective term o[r] = 1 - score.          */
/*   EUCLIDEAN  g_k = dot[r,k] - half_norm[k], one subtraction.  label = the k of largest g_k, by the same rules (ties to the         */
/*              smaller index, no k with g_k > -Inf: invalid).  score = fmaxf(0, fmaf(-2, g_label, ss)), the squared distance.        */
/*              v[r,b] = x[r,b];  o[r] = score.                                                                                       */
/*  Accumulation, when acc != NULL.  acc: float64 [2 + K + K B] = (valid rows, objective, n[K], s[K,B]), zeroed by the caller before  */
/*   the first call; calls add to it.  The call's rows are cut into chunks of UMHS_CLUSTER_CHUNK rows: chunk j is rows               */
/*   [j CH, (j + 1) CH) of THIS call.  Within a chunk n[k] counts the rows of label k; s[k,b] is the float32 chain                    */
/*   fmaf(m[r,k], v[r,b], .)  over r ascending from +0, m = 1 where label[r] == k and 0 otherwise, v = 0 in invalid rows -- the       */
/*   float32 sum of the members' v in row order; the objective is the float32 sum of o[r] over the valid r ascending from +0.        */
/*   The chunk results are added onto acc in float64, chunks ascending: acc[0] += valid, acc[1] += objective, acc[2 + k] += n[k],    */
/*   acc[2 + K + k B + b] += s[k,b].  So a call split at a multiple of CH rows leaves the same bits in acc as one call.              */
/*  Outputs.  label int32 [R] and score float32 [R]: each may be NULL.  With acc == NULL the call only assigns: one launch, and      */
/*   workspace may be NULL.                                                                                                           */
/*  No atomics; nothing depends on the grid or on occupancy: the same bits on every run and on every device; the label and score of  */
/*   row r depend neither on R nor on the other rows.                                                                                 */
/*  Workspace: umhs_cluster_workspace_bytes(R, K, B) = min(ceil(R / CH), 512) (2 + K + K B) 4 bytes, 4-byte aligned, plain scratch;  */
/*   0 for R < 1 or a K or B outside the limits.  Two launches per 512 chunks (chunk partials; their float64 sum onto acc).          */
/*  Errors, before anything is launched: B < 1, K < 1, R < 0, stride < B, a metric that is neither: UMHS_ERR_ARG; B > 256 or          */
/*   K > UMHS_CLUSTER_MAX: UMHS_ERR_UNSUPPORTED; then R == 0: UMHS_OK whatever the pointers; then a NULL spectra or image:            */
/*   UMHS_ERR_ARG; then EUCLIDEAN with a NULL half_norm: UMHS_ERR_ARG; then acc set with a NULL or too small workspace: UMHS_ERR_ARG. */
/* ------------------------------------------------------------------------------------------ */
enum { UMHS_CLUSTER_ANGLE = 0, UMHS_CLUSTER_EUCLIDEAN = 1 };
#define UMHS_CLUSTER_MAX 64
#define UMHS_CLUSTER_CHUNK 1024
int umhs_cluster_chunk(void); /* UMHS_CLUSTER_CHUNK, for callers that cannot read this header */
size_t umhs_cluster_workspace_bytes(int64_t n_rows, int n_clusters, int n_bands);
int umhs_cluster_step(const float* spectra, int64_t stride, int64_t n_rows, const float* mask, const float* image,
                      const float* half_norm, int n_clusters, int n_bands, int metric, int32_t* label, float* score, double* acc,
                      void* workspace, size_t workspace_bytes, umhs_stream_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Sparse unmixing (csrc/umhs_sparse.hip): every row against a WHOLE spectral library A [L,B]: the few entries, with non-negative     */
/* abundances, that explain the row -- the non-negative lasso, solved per row by ADMM as in SUnSAL (Bioucas-Dias and Figueiredo,      */
/* 2010).  Per row a minimises  f(a) = 1/2 |x - A^T a|^2 + lambda_r sum a  over a >= 0, lambda_r = lambda sqrt(ss).  THE definition:  */
/*  Inputs.  spectra: float32 rows [R] of B bands, row r at spectra + r * stride floats, by the rules of umhs_library_match          */
/*   (stride >= B, any 4-byte aligned address, columns >= B of a row are never read).  The library A: float32 [L,B], NOT normalised.  */
/*   1 <= B <= 256, 1 <= L <= UMHS_SPARSE_MAX_ENTRIES, R >= 0; epsilon > 0, max_iterations >= 1, theta >= 0.                          */
/*  Host preparation, once per (A, lambda, mu), mu > 0, in float64 from the float32 A, each result rounded to float32 once:           */
/*   G = A A^T,  F = (G + mu I)^-1,  Q = F A [L,B],  M = mu F [L,L],  theta = lambda / mu.                                            */
/*   q_image and a_image: the operand images umhs_library_prepare makes from Q and from A.  m_image and g_image: what                 */
/*   umhs_sparse_prepare makes from M and from G (umhs_sparse_image_bytes(L) bytes each).                                             */
/*  ss = (the fmaf chain of x_b x_b over the even b ascending from +0) + (the same chain over the odd b): the ss of umhs_unmix.  A    */
/*   row is INVALID when ss is 0, NaN or +Inf: abundances of exact +0, residual 0 and status -1.                                      */
/*  Iteration, all float32, from z = d = 0:                                                                                           */
/*   c_k  = the fmaf chain  fmaf(Q[k,b], x_b, .)  over b ascending from +0 (the dot of umhs_library_match);  s = max_k |c_k|;         */
/*   tau  = theta * sqrtf(ss), root correctly rounded, one multiplication;                                                            */
/*   a_k  = the fmaf chain  fmaf(M[k,j], v_j, .)  that starts from c_k, v_j = z_j - d_j (one subtraction), over j in THIS order:      */
/*          the tiles of 32 entries ascending; within tile t, for e = 0 .. 15: j = 32 t + (e & 3) + 8 (e >> 2), then that j + 4       */
/*          (0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, ...).  Entries >= L are skipped (they would add an exact 0 x 0).                   */
/*   t_k  = a_k + d_k;  u_k = t_k - tau;  z'_k = u_k if u_k > 0, else +0 (never -0, never a NaN);  d'_k = t_k - z'_k.                  */
/*   A row is DONE after the first iteration at which  max_k |a_k - z'_k| <= epsilon * s  and  max_k |z'_k - z_k| <= epsilon * s      */
/*   (epsilon * s one multiplication).  From then on the row is frozen: its result is that z' and its status the number of that       */
/*   iteration (1 ..).  A row with s = 0 is done by iteration 1 with all zeros.  A row that is not done after max_iterations          */
/*   returns its last z' with status -2.  A row never hangs.  Every returned a_k is finite and >= +0: whatever is not in              */
/*   (0, FLT_MAX] is written as +0.                                                                                                   */
/*   residual = max(0, fmaf(-2, p, ss) + q):  b_k = the chain fmaf(A[k,b], x_b, .) as c;  w_k = the chain fmaf(G[k,j], z_j, .) from    */
/*   +0 over j in the order above;  p = p0 + p1 and q = q0 + q1, where p_h is the chain fmaf(b_k, z_k, .) and q_h the chain            */
/*   fmaf(z_k, w_k, .) from +0 over the k ascending whose bit 2 is h:  |x - A^T z|^2 up to rounding relative to ss.                   */
/*  Outputs.  abundances: float32 [R,L] or NULL.  residual: float32 [R] or NULL (a_image and g_image are read only for it).           */
/*   status: int32 [R] or NULL.                                                                                                       */
/*  One launch, no workspace, no atomics, nothing depends on the grid: the same bits on every run, and the bits of row r depend       */
/*   neither on R nor on the other rows (which is why a finished row freezes).  A wave leaves the loop when its 32 rows are done.      */
/*  Errors, before anything is launched: B < 1, L < 1, R < 0, stride < B, max_iterations < 1, an epsilon that is not > 0, a theta     */
/*   that is not >= 0: UMHS_ERR_ARG; B > 256 or L > UMHS_SPARSE_MAX_ENTRIES: UMHS_ERR_UNSUPPORTED; then R == 0: UMHS_OK whatever      */
/*   the pointers; then a NULL spectra, q_image or m_image, or a residual without a_image and g_image: UMHS_ERR_ARG.                  */
/*                                                                                                                                    */
/* umhs_sparse_image_bytes: 4096 T^2 bytes, T = ceil(L / 32); 0 for an L outside the limits.                                          */
/* umhs_sparse_prepare: a DEVICE float32 [L,L] -> the image the kernel keeps in LDS: for the output tile to and the input tile ti,    */
/*   element ((((to T + ti) 4 + e / 4) 64 + lane) 4 + e % 4) = m[32 to + (lane & 31)][32 ti + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)],  */
/*   zeros past L.  One launch.  Errors: L < 1: UMHS_ERR_ARG; L > UMHS_SPARSE_MAX_ENTRIES: UMHS_ERR_UNSUPPORTED; a NULL: ARG.        */
/* ------------------------------------------------------------------------------------------ */
#define UMHS_SPARSE_MAX_ENTRIES 128
size_t umhs_sparse_image_bytes(int n_entries);
int umhs_sparse_prepare(const float* matrix, int n_entries, float* image, umhs_stream_t stream);
int umhs_sparse_unmix(const float* spectra, int64_t stride, int64_t n_rows, const float* q_image, const float* m_image,
                      const float* a_image, const float* g_image, int n_entries, int n_bands, float theta, float epsilon,
                      int max_iterations, float* abundances, float* residual, int32_t* status, umhs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UMHS_HIP_H */
