// gfx950 kernels for the multires hash-grid encode of the UMHS hot path (R2): gather fwd (+ the backward's bucket histogram), the
// atomic backward, enc_gather, and the host side of the partitioned backward (device code: umhs_hashgrid_part.h).
#include <atomic>
#include <cstdlib>

#include "umhs_hashgrid_part.h"

// =============================================================================================
// R2: multires hash grid.  One thread per (sample, level); grid.y = level, so blocks are dispatched
// level-major and the resident waves of an XCD gather from one 4 MiB level slab (= one XCD L2) at
// a time instead of from the whole 64 MiB table.
// =============================================================================================
// the feature pair of sample i at level l into enc: one 8-byte store where the strides keep it aligned (enc itself is: host check)
__device__ __forceinline__ void hash_store_pair(float* __restrict__ enc, int64_t i, int l, int64_t stride_n, int64_t stride_l, float2 r) {
  float* o = enc + i * stride_n + (int64_t)l * stride_l;
  if (((stride_n | stride_l) & 1) == 0) {
    *reinterpret_cast<float2*>(o) = r;
  } else {
    o[0] = r.x, o[1] = r.y;
  }
}

__global__ __launch_bounds__(256) void hashgrid_fwd_kernel(const float* __restrict__ pos01,
                                                           const float2* __restrict__ table,
                                                           const float* __restrict__ scalings, int64_t n, int n_levels,
                                                           int log2_T, float* __restrict__ enc, int64_t stride_n,
                                                           int64_t stride_l) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float px = pos01[3 * i], py = pos01[3 * i + 1], pz = pos01[3 * i + 2];
  const int l = (int)blockIdx.y;
  HashCorners h = hash_corners(px, py, pz, scalings[l], (1u << log2_T) - 1u, (uint32_t)l << log2_T);
  float2 f[8];
  hash_gather8(table, h, f);
  hash_store_pair(enc, i, l, stride_n, stride_l, hash_trilerp(f, h.ox, h.oy, h.oz));
}

// levels [level_begin, +n_levels) inside the grid's 32 and a table size the kernels index (the partition forms buckets from log2_T
// >= 2 on; the gather alone takes 1)
static inline bool hg_range_ok(int level_begin, int n_levels, int log2_T, int min_log2_T = 2) {
  return n_levels >= 1 && level_begin + n_levels <= 32 && log2_T >= min_log2_T && log2_T <= 24;
}

extern "C" int umhs_hashgrid_fwd(const float* pos01, const float* table, const float* scalings, int64_t n,
                                 int n_levels, int log2_T, float* enc, int64_t stride_n, int64_t stride_l,
                                 umhs_stream_t stream) {
  if (n < 0 || !table || !scalings) return UMHS_ERR_ARG;
  if (!hg_range_ok(0, n_levels, log2_T, 1)) return UMHS_ERR_UNSUPPORTED;
  if (n == 0) return UMHS_OK;  // (an empty batch has no per-sample arrays: torch hands out NULL for them)
  if (!pos01 || !enc) return UMHS_ERR_ARG;
  if (((uintptr_t)table & 15) || ((uintptr_t)enc & 7)) return UMHS_ERR_ARG;  // (16-byte slot pairs are fetched with one load)
  const float2* t2 = reinterpret_cast<const float2*>(table);
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_levels);
  hipLaunchKernelGGL(hashgrid_fwd_kernel, grid, dim3(256), 0, umhs_s(stream), pos01, t2, scalings, n, n_levels, log2_T, enc, stride_n, stride_l);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// Backward v1: memory-side float atomics, one (sample, level) per thread, level-major grid.
__global__ __launch_bounds__(256) void hashgrid_bwd_kernel(const float* __restrict__ pos01,
                                                           const float* __restrict__ d_enc, int64_t stride_n,
                                                           int64_t stride_l, const float* __restrict__ scalings,
                                                           int64_t n, int log2_T, float* __restrict__ d_table, int level0) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int l = level0 + blockIdx.y;
  const float* g = d_enc + i * stride_n + (int64_t)l * stride_l;
  float g0 = g[0], g1 = g[1];
  if (g0 == 0.0f && g1 == 0.0f) return;  // masked / zero-weight samples contribute exact zeros
  HashCorners h = hash_corners(pos01[3 * i], pos01[3 * i + 1], pos01[3 * i + 2], scalings[l],
                               (1u << log2_T) - 1u, (uint32_t)l << log2_T);
  float w[8];
  hash_corner_weights(h.ox, h.oy, h.oz, w);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (w[c] != 0.0f) {
      atomicAdd(d_table + 2 * (size_t)h.idx[c], w[c] * g0);
      atomicAdd(d_table + 2 * (size_t)h.idx[c] + 1, w[c] * g1);
    }
  }
}

// hashgrid_fwd_kernel + the backward's bucket histogram: one workgroup = one run of HB_RUN samples of one level (the scatter pass's
// unit), one sample per thread
static_assert(HB_RUN == 512, "hashgrid_fwd_count_kernel's workgroup is one run of the partition");
__global__ __launch_bounds__(HB_RUN) void hashgrid_fwd_count_kernel(const float2* __restrict__ table, float* __restrict__ enc, int64_t stride_n,
                                                                 int64_t stride_l, HbArgs a) {
  __shared__ uint32_t cursor[HB_MAX_NB];
  const int tid = threadIdx.x, lane = tid & 63, wg = blockIdx.x, l = blockIdx.y;  // (workspace range starts at level 0: lev == l)
  if (tid < HB_MAX_NB) cursor[tid] = 0;
  __syncthreads();
  const int64_t i = (int64_t)wg * HB_RUN + tid;
  const bool act = i < a.n;
  const int64_t ii = act ? i : a.n - 1;
  const uint32_t mask = (1u << a.log2_T) - 1u, base = (uint32_t)l << a.log2_T;
  const HashCorners h = hash_corners(a.pos01[3 * ii], a.pos01[3 * ii + 1], a.pos01[3 * ii + 2], a.scalings[l], mask, base);
  HashGather hg;
  hash_gather8_issue(table, h, hg);  // the loads are in flight while the wave counts
  __builtin_amdgcn_sched_barrier(0);
  uint32_t slot[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) slot[c] = h.idx[c] - base;
  hb_count_sample(slot, hb_cell_key(h, act, lane), act, a.bucket_bits, lane, cursor);
  __syncthreads();
  if (tid < a.nb) a.wg_counts[((size_t)l * a.nwg + wg) * a.nb + tid] = cursor[tid];
  __builtin_amdgcn_sched_barrier(0);
  float2 f[8];
  hash_gather8_select(h, hg, f);
  const float2 r = hash_trilerp(f, h.ox, h.oy, h.oz);
  if (act) hash_store_pair(enc, i, l, stride_n, stride_l, r);
}

static inline int hb_scatter_wgs(int n_levels) {  // workgroups per level of the scatter pass (a multiple of 8); UMHS_HB_WGS: measurement knob
  static const int forced = [] {
    const char* e = getenv("UMHS_HB_WGS");
    return e ? atoi(e) : 0;
  }();
  int w = forced > 0 ? forced : 1024 / (n_levels > 0 ? n_levels : 1);
  w = (w + 7) / 8 * 8;
  return w < 8 ? 8 : w;
}

// The workspace of the partitioned backward: sizes, and the byte offset of every region from the workspace's 256-byte aligned base.
// Written once for umhs_hashgrid_bwd_workspace_bytes (total) and hb_args (the pointers).  total == 0: shape not supported.
struct HbLayout {
  int bucket_bits, nb, nwg;
  size_t cap;  // records per level: HB_CAP_PER_SAMPLE per sample, a multiple of 8 (the level regions start on 128-byte lines)
  size_t counts, offsets, lmax, wg_counts, wg_prefix, recs, total;
};

static HbLayout hb_layout(int64_t n, int n_levels, int log2_T) {
  HbLayout w{};
  if (n <= 0 || n_levels < 1 || log2_T < 2) return w;
  w.bucket_bits = log2_T < HB_BUCKET_BITS ? log2_T : HB_BUCKET_BITS, w.nb = 1 << (log2_T - w.bucket_bits);
  if (w.nb > HB_MAX_NB) return w;  // larger tables: only the atomic path is available
  w.nwg = (int)((n + HB_RUN - 1) / HB_RUN);
  w.cap = ((size_t)n * HB_CAP_PER_SAMPLE + 7) & ~(size_t)7;
  if (w.cap >= ((size_t)1 << 28)) return w;  // byte offsets inside a level's record region are 32-bit (53 M samples per call)
  const auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t m = (size_t)n_levels * w.nb, wg_bytes = align((size_t)n_levels * w.nwg * w.nb * 4);
  w.counts = 0, w.offsets = m * 4, w.lmax = 2 * m * 4;
  w.wg_counts = align((2 * m + (size_t)n_levels * HB_LMAX_PARTS) * 4);
  w.wg_prefix = w.wg_counts + wg_bytes;
  w.recs = w.wg_prefix + wg_bytes;
  w.total = 256 + w.recs + align((size_t)n_levels * w.cap * 16);  // (256: the base is the workspace pointer rounded up)
  return w;
}

extern "C" size_t umhs_hashgrid_bwd_workspace_bytes(int64_t n, int n_levels, int log2_T) { return hb_layout(n, n_levels, log2_T).total; }

static int hb_args(HbArgs* a, const float* pos01, const float* scalings, int64_t n, int ws_begin, int ws_levels, int log2_T,
                   void* workspace, size_t workspace_bytes) {
  const HbLayout w = hb_layout(n, ws_levels, log2_T);
  if (w.total == 0) return UMHS_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < w.total) return UMHS_ERR_WORKSPACE;
  a->pos01 = pos01, a->d_enc = nullptr, a->sn = 0, a->sl = 0, a->scalings = scalings, a->n = n;
  a->log2_T = log2_T, a->bucket_bits = w.bucket_bits, a->nb = w.nb, a->level0 = ws_begin;
  a->nlev = ws_levels, a->lev_off = 0, a->overwrite = 0, a->grad_mask = 0;
  a->adam = HbAdam{};
  a->nwg = w.nwg, a->cap = (uint32_t)w.cap;
  char* const base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  a->counts = reinterpret_cast<uint32_t*>(base + w.counts), a->offsets = reinterpret_cast<uint32_t*>(base + w.offsets);
  a->lmax = reinterpret_cast<uint32_t*>(base + w.lmax);
  a->wg_counts = reinterpret_cast<uint32_t*>(base + w.wg_counts), a->wg_prefix = reinterpret_cast<uint32_t*>(base + w.wg_prefix);
  a->recs = reinterpret_cast<uint4*>(base + w.recs);
  return UMHS_OK;
}

// histogram (count_wgs workgroups per level; 0 = one per run of samples), per-workgroup prefix, bucket scan
static int hb_run_prepare(const HbArgs& a, int n_levels, int count_wgs, umhs_stream_t stream) {
  // The histogram pass reads the gradient only in the one-call form (grad_mask): a prepare half built from hb_args() has
  // d_enc == nullptr, and a pass that dereferenced it anyway is the nil-address GPU fault recorded in DESIGN.md section 9.
  if (a.grad_mask && !a.d_enc) return UMHS_ERR_ARG;
  if (n_levels != a.nlev) return UMHS_ERR_ARG;  // (the scans walk the whole workspace range)
  dim3 pgrid((unsigned)(count_wgs > 0 && count_wgs < a.nwg ? count_wgs : a.nwg), (unsigned)n_levels);
  hipLaunchKernelGGL(hg_count_kernel, pgrid, dim3(256), 0, umhs_s(stream), a);
  hipLaunchKernelGGL(hg_wgscan_kernel, dim3((unsigned)a.nb, (unsigned)n_levels), dim3(256), 0, umhs_s(stream), a);
  hipLaunchKernelGGL(hg_scan_kernel, dim3((unsigned)n_levels), dim3(64), 0, umhs_s(stream), a);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

static int hb_run_apply(const HbArgs& a, int n_levels, float* d_table, umhs_stream_t stream) {  // scatter + bucket reduce
  if (!a.d_enc || !d_table || !a.pos01 || !a.scalings) return UMHS_ERR_ARG;  // every pointer the two kernels dereference
  // persistent workgroups: the 1024 that 256 CUs hold at four each, spread over the levels of this launch (16 levels: 64 per level =
  // 8 per XCD; a level group of 8 -- the multi-GPU exchange applies the levels in groups -- 128 per level)
  int per_level = hb_scatter_wgs(n_levels);
  if (per_level > HB_LMAX_PARTS) per_level = HB_LMAX_PARTS;  // (one max-|value| word per workgroup and level)
  if (per_level > ((a.nwg + 7) / 8) * 8) per_level = ((a.nwg + 7) / 8) * 8;
  dim3 pgrid((unsigned)per_level, (unsigned)n_levels);
  hipLaunchKernelGGL(hg_scatter_kernel, pgrid, dim3(256), 0, umhs_s(stream), a);
  const size_t lds = (size_t)(2 << a.bucket_bits) * 8;
  {  // raise the dynamic-LDS limit once per device, not per call (the driver call is a bubble in front of the launch)
    static std::atomic<size_t> granted[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
    if (dev < 0 || granted[dev].load(std::memory_order_relaxed) < lds) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(hg_reduce_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds) != hipSuccess)
        return UMHS_ERR_LAUNCH;
      if (dev >= 0) granted[dev].store(lds, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)a.nb, (unsigned)n_levels), dim3(1024), lds, umhs_s(stream), a, d_table);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// overwrite mode where no reduce pass runs over the levels (no samples; the atomic path): their d_table slabs are zeroed here
static bool hg_clear_levels(float* d_table, int level_begin, int n_levels, int log2_T, umhs_stream_t stream) {
  return hipMemsetAsync(d_table + (((size_t)level_begin << log2_T) * 2), 0, ((size_t)n_levels << log2_T) * 8, umhs_s(stream)) == hipSuccess;
}

extern "C" int umhs_hashgrid_bwd(const float* pos01, const float* d_enc, int64_t stride_n, int64_t stride_l,
                                 const float* scalings, int64_t n, int level_begin, int n_levels, int log2_T,
                                 float* d_table, int overwrite, void* workspace, size_t workspace_bytes,
                                 umhs_stream_t stream) {
  if (n < 0 || !scalings || !d_table || level_begin < 0) return UMHS_ERR_ARG;
  if (n > 0 && (!pos01 || !d_enc)) return UMHS_ERR_ARG;  // (an empty batch has no per-sample arrays)
  // only the partitioned path writes every slot itself
  if (overwrite && (!workspace || n == 0) && !hg_clear_levels(d_table, level_begin, n_levels, log2_T, stream)) return UMHS_ERR_LAUNCH;
  if (!hg_range_ok(level_begin, n_levels, log2_T)) return UMHS_ERR_UNSUPPORTED;
  if (n == 0) return UMHS_OK;
  if (!workspace) {  // v1: memory-side float atomics (no workspace needed; fine for small N)
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_levels);
    hipLaunchKernelGGL(hashgrid_bwd_kernel, grid, dim3(256), 0, umhs_s(stream), pos01, d_enc, stride_n, stride_l,
                       scalings, n, log2_T, d_table, level_begin);
    UMHS_CHECK_LAUNCH();
    return UMHS_OK;
  }
  // one-call form: the histogram pass may look at the gradient too, so zero-gradient samples are skipped in both passes
  HbArgs a;
  int rc = hb_args(&a, pos01, scalings, n, level_begin, n_levels, log2_T, workspace, workspace_bytes);
  if (rc) return rc;
  if ((uintptr_t)d_table & 15) return UMHS_ERR_WORKSPACE;
  a.d_enc = d_enc, a.sn = stride_n, a.sl = stride_l, a.overwrite = overwrite, a.grad_mask = 1;
  rc = hb_run_prepare(a, n_levels, 0, stream);
  if (rc) return rc;
  return hb_run_apply(a, n_levels, d_table, stream);
}

// Gradient-independent half of the partitioned backward (bucket histogram + exclusive scan): needs only the positions, so
// a caller may run it on a side stream while the forward pass is still in flight.  (Every sample emits records in this
// form; the one-call umhs_hashgrid_bwd skips samples whose gradient is exactly zero.)
extern "C" int umhs_hashgrid_bwd_prepare(const float* pos01, const float* scalings, int64_t n, int level_begin, int n_levels,
                                         int log2_T, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n < 0 || !scalings || level_begin < 0) return UMHS_ERR_ARG;
  if (!hg_range_ok(level_begin, n_levels, log2_T)) return UMHS_ERR_UNSUPPORTED;
  if (n == 0) return UMHS_OK;
  if (!pos01) return UMHS_ERR_ARG;
  HbArgs a;
  int rc = hb_args(&a, pos01, scalings, n, level_begin, n_levels, log2_T, workspace, workspace_bytes);
  if (rc) return rc;
  const int throttle = 16;  // workgroups per level of the hidden histogram pass (unthrottled it delays the forward's workgroups)
  return hb_run_prepare(a, n_levels, throttle, stream);
}

// umhs_hashgrid_fwd for ALL levels of the workspace range [0, n_levels) + the histogram pass of umhs_hashgrid_bwd_prepare for the same
// positions in one launch; umhs_hashgrid_bwd_prepare_counted then only runs the two small scans (a caller may put it on a side stream).
extern "C" int umhs_hashgrid_fwd_count(const float* pos01, const float* table, const float* scalings, int64_t n, int n_levels, int log2_T,
                                       float* enc, int64_t stride_n, int64_t stride_l, void* workspace, size_t workspace_bytes,
                                       umhs_stream_t stream) {
  if (n < 0 || !table || !scalings) return UMHS_ERR_ARG;
  if (!hg_range_ok(0, n_levels, log2_T)) return UMHS_ERR_UNSUPPORTED;
  if (n == 0) return UMHS_OK;
  if (!pos01 || !enc) return UMHS_ERR_ARG;
  if (((uintptr_t)table & 15) || ((uintptr_t)enc & 7)) return UMHS_ERR_ARG;
  HbArgs a;
  int rc = hb_args(&a, pos01, scalings, n, 0, n_levels, log2_T, workspace, workspace_bytes);
  if (rc) return rc;
  hipLaunchKernelGGL(hashgrid_fwd_count_kernel, dim3((unsigned)a.nwg, (unsigned)n_levels), dim3(HB_RUN), 0, umhs_s(stream),
                     reinterpret_cast<const float2*>(table), enc, stride_n, stride_l, a);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_hashgrid_bwd_prepare_counted(const float* pos01, const float* scalings, int64_t n, int n_levels, int log2_T,
                                                 void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n < 0 || !pos01 || !scalings) return UMHS_ERR_ARG;
  if (!hg_range_ok(0, n_levels, log2_T)) return UMHS_ERR_UNSUPPORTED;
  if (n == 0) return UMHS_OK;
  HbArgs a;
  int rc = hb_args(&a, pos01, scalings, n, 0, n_levels, log2_T, workspace, workspace_bytes);
  if (rc) return rc;
  hipLaunchKernelGGL(hg_wgscan_kernel, dim3((unsigned)a.nb, (unsigned)n_levels), dim3(256), 0, umhs_s(stream), a);
  hipLaunchKernelGGL(hg_scan_kernel, dim3((unsigned)n_levels), dim3(64), 0, umhs_s(stream), a);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// Gradient-dependent half: scatter the records of levels [level_begin, +n_levels) into their buckets and reduce every bucket
// into its d_table slab.  The workspace must hold a umhs_hashgrid_bwd_prepare of [ws_level_begin, +ws_n_levels) for the SAME
// positions, and that range must contain the levels applied; each level may be applied once per prepare.
static int hb_apply(const float* pos01, const float* d_enc, int64_t stride_n, int64_t stride_l, const float* scalings, int64_t n,
                    int level_begin, int n_levels, int ws_level_begin, int ws_n_levels, int log2_T, float* d_table, int overwrite,
                    const HbAdam* adam, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  if (n < 0 || !scalings || !d_table || level_begin < 0) return UMHS_ERR_ARG;
  if (n > 0 && (!pos01 || !d_enc)) return UMHS_ERR_ARG;
  // (the applied levels lie inside the workspace range, which is therefore not empty either)
  if (n_levels < 1 || level_begin < ws_level_begin || level_begin + n_levels > ws_level_begin + ws_n_levels ||
      !hg_range_ok(ws_level_begin, ws_n_levels, log2_T))
    return UMHS_ERR_UNSUPPORTED;
  if ((uintptr_t)d_table & 15) return UMHS_ERR_WORKSPACE;
  if (n == 0) return (overwrite && !hg_clear_levels(d_table, level_begin, n_levels, log2_T, stream)) ? UMHS_ERR_LAUNCH : UMHS_OK;
  HbArgs a;
  int rc = hb_args(&a, pos01, scalings, n, ws_level_begin, ws_n_levels, log2_T, workspace, workspace_bytes);
  if (rc) return rc;
  a.d_enc = d_enc, a.sn = stride_n, a.sl = stride_l, a.lev_off = level_begin - ws_level_begin, a.overwrite = overwrite;
  if (adam) a.adam = *adam;
  return hb_run_apply(a, n_levels, d_table, stream);
}

extern "C" int umhs_hashgrid_bwd_apply(const float* pos01, const float* d_enc, int64_t stride_n, int64_t stride_l,
                                       const float* scalings, int64_t n, int level_begin, int n_levels, int ws_level_begin,
                                       int ws_n_levels, int log2_T, float* d_table, int overwrite, void* workspace,
                                       size_t workspace_bytes, umhs_stream_t stream) {
  return hb_apply(pos01, d_enc, stride_n, stride_l, scalings, n, level_begin, n_levels, ws_level_begin, ws_n_levels, log2_T, d_table,
                  overwrite, nullptr, workspace, workspace_bytes, stream);
}

// umhs_hashgrid_bwd_apply (overwrite mode) + the Adam step of the table entries of levels >= adam_level_begin in the epilogue of
// the bucket reduce, where their gradient is final: for a single-GPU trainer whose optimizer step follows the backward anyway.
// table_params / exp_avg / exp_avg_sq: [L*T,2] like d_table; hyper-parameters as umhs_adam_step (grad_scale 1).  The gradient is
// still written to d_table.  n must be > 0 (with no samples there is no reduce pass to ride on).
extern "C" int umhs_hashgrid_bwd_apply_adam(const float* pos01, const float* d_enc, int64_t stride_n, int64_t stride_l,
                                            const float* scalings, int64_t n, int level_begin, int n_levels, int ws_level_begin,
                                            int ws_n_levels, int log2_T, float* d_table, void* workspace, size_t workspace_bytes,
                                            float* table_params, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                            float beta2, float eps, int64_t step, int adam_level_begin, umhs_stream_t stream) {
  if (!table_params || !exp_avg || !exp_avg_sq || step < 1 || adam_level_begin < 0) return UMHS_ERR_ARG;
  if (((uintptr_t)table_params | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return UMHS_ERR_ARG;
  if (n <= 0) return UMHS_ERR_UNSUPPORTED;
  const AdamBias bc = adam_bias(lr, beta1, beta2, step);
  HbAdam ad;
  ad.p = table_params, ad.m = exp_avg, ad.v = exp_avg_sq, ad.lr_bc1 = bc.lr_bc1, ad.b1 = beta1, ad.b2 = beta2, ad.eps = eps;
  ad.sqrt_bc2 = bc.sqrt_bc2, ad.level_begin = adam_level_begin;
  return hb_apply(pos01, d_enc, stride_n, stride_l, scalings, n, level_begin, n_levels, ws_level_begin, ws_n_levels, log2_T, d_table,
                  1, &ad, workspace, workspace_bytes, stream);
}

// Compaction of level-major hash features: out[l][i] = in[l][idx[i]].  The sampler already encoded every candidate sample for
// its density query; the survivors' features are gathered (128 B per sample, near-sequential: idx ascends) instead of hashed
// and gathered again from the table (1 KiB per sample, random).
__global__ __launch_bounds__(256) void enc_gather_kernel(const float2* __restrict__ in, const int64_t* __restrict__ idx, int64_t m,
                                                         int64_t n, float2* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t j = idx[i];
  j = j < 0 ? 0 : (j >= m ? m - 1 : j);
  const int l = blockIdx.y;
  out[(int64_t)l * n + i] = in[(int64_t)l * m + j];
}

extern "C" int umhs_enc_gather(const float* enc_in, const int64_t* index, int64_t m, int64_t n, int n_levels, float* enc_out,
                               umhs_stream_t stream) {
  if (m < 0 || n < 0 || n_levels < 1 || n_levels > 64) return UMHS_ERR_ARG;
  if (n == 0) return UMHS_OK;
  if (m < 1 || !enc_in || !index || !enc_out || (((uintptr_t)enc_in | (uintptr_t)enc_out) & 7)) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(enc_gather_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_levels), dim3(256), 0, umhs_s(stream),
                     reinterpret_cast<const float2*>(enc_in), index, m, n, reinterpret_cast<float2*>(enc_out));
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
