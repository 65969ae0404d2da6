// Device code of the multires hash grid's partitioned backward (R2): the record plan, its histogram and scatter passes, the two scans
// and the bucket reduce with its optional Adam epilogue.  Included by umhs_hashgrid.hip only, which holds the host side.
#pragma once
#include "umhs_adam.h"
#include "umhs_hash.h"

// ---------------------------------------------------------------------------------------------
// Backward v2 (default): no global atomics.  MI355X executes global float atomics at the memory side at
// ~20 G requests/s whatever the schedule, so 8 corners x 16 levels x N scattered adds cost ~6 ms at
// N = 262k.  Instead each level's contributions are radix-partitioned by the high bits of their hash
// slot into buckets of 2^13 slots, every (level, bucket) tile is accumulated in LDS by one workgroup
// and added to d_table with plain coalesced stores:
//   count   : per (level, 512-sample run) LDS histogram of the bucket ids of its records (the record plan) -> per-workgroup counts
//   scan    : exclusive prefix over the workgroups of a level (hg_wgscan) and over its buckets (hg_scan)
//   scatter : recompute the corners and the plan, order the run's records by bucket in LDS, write them out
//   reduce  : one workgroup per (level, bucket): stream its records into an LDS tile, flush (+ Adam)
// Round 4 (in-kernel stamps, profiles/r04/hg_stamps_*.json): neither pass was bound where rounds 1-3 said.  The scatter pass spent
// 40 % of its wave time writing records out and 47 % waiting on its few loads behind those stores (hashing + run merging: 3 %); the
// reduce pass 42-55 % waiting for record loads and 39 % in the Adam stream, 7 % in LDS atomics (the LDS unit alone would do the whole
// pass in 30 us: tools/mb_lds_atomics2.hip).  What cost the time was the SHAPE of the record stream: {uint16 slot, float2 value} in
// two arrays = a 2-byte and an 8-byte access per record (MI355X_MICROARCH.md: short stores cost 12.5x, dwordx2 2.7x the dwordx4 time
// per byte).  Records are now ONE 16-byte word each and there are half as many:
//   * the two x-neighbours of a corner pair hash to slots s and s ^ (xf ^ xc), i.e. into the same bucket (xf ^ xc < 2^13 for every
//     resolution below 8192), and their values are g*wyz*(1-ox) and g*wyz*ox: one PAIR record {g.x*wyz, g.y*wyz, ox, meta} serves
//     both corners (meta = slot_low | k << 13, xf ^ xc = 2^(k+1) - 1) -- 4 records of 16 B per (sample, level) instead of 8 of 10 B,
//     one dwordx4 store / load each, half the LDS placement work; the reduce pass forms the two corner values;
//   * a run of samples that share a cell (coarse / mid levels of a real ray batch: merged by a wave segmented scan as before) emits
//     its 8 corner sums as SINGLE records {v.x, v.y, 0, meta} (k = 15: no partner); so do the (x-integer) and the (partner in another
//     bucket: resolutions >= 8192 only) cases.
// Two MI355X-specific choices kept from round 1 (tools/mb_lds_atomics2.hip): LDS float atomics cost 81 ns per wave-instruction but
// 64-bit INTEGER ones 7.5, so the tile is int64 fixed point (scale from the level's max |value| and the bucket's record count:
// >= 46 bits below the level maximum) -- which also makes every sum exact and order-independent, i.e. bitwise reproducible,
// unlike the reference's index_put_/atomics.
// ---------------------------------------------------------------------------------------------
#define HB_BUCKET_BITS 13
#define HB_MAX_NB 128  // buckets per level the partition kernels can handle (two per lane of wave 0)
#define HB_SPT 2  // samples per thread -> 512 samples per workgroup (<= 2048 pair records staged in 32 KiB of LDS)
#define HB_RUN (256 * HB_SPT)  // samples per run = per workgroup of the partition kernels; the unit of wg_counts / wg_prefix
#define HB_CAP_PER_SAMPLE 5  // record capacity per (sample, level): 4 pair records, or <= 4 per sample from merged runs; the fifth is
                             // slack for pairs split over two buckets (resolutions >= 8192); a level that overflows gets NaN gradients
#define HB_MERGE_MIN 16  // lanes of a wave that must continue a run of equal cells for the wave to merge runs
#define HB_POISON 0xffffffffu
// One word per scatter workgroup and level for the level's max |value|, reduced by the readers.  Rounds 1-3 (and the first round-4
// builds) did `atomicMax(&lmax[level])` once per workgroup run: 8192 device-scope atomics on 16 words of ONE cache line serialise at
// the memory side at ~12 ns each = 100 us -- the whole scatter pass, whatever else it did (ablation builds, profiles/r04/scatter_ablation*.txt:
// 98 us with every store, LDS placement and the write-out removed, 16 us once the maximum stayed zero).
#define HB_LMAX_PARTS 128

struct HbAdam {  // optional optimizer step in the epilogue of the bucket reduce (one GPU: the gradient is final there)
  float *p, *m, *v;  // hash table parameters / exp_avg / exp_avg_sq, [L*T, 2] like d_table; p == nullptr: off
  float lr_bc1, b1, b2, eps, sqrt_bc2;
  int level_begin;   // absolute level from which on the update is applied (the sparse coarse levels keep their row-wise kernel)
};

struct HbArgs {
  HbAdam adam;
  const float* pos01;
  const float* d_enc;
  int64_t sn, sl;
  const float* scalings;
  int64_t n;
  int log2_T, bucket_bits, nb, level0, nlev;  // level0: first level of the WORKSPACE range; nlev: its size
  int lev_off;                                 // this launch covers workspace levels [lev_off, lev_off + gridDim.y)
  int grad_mask;  // 1: samples whose gradient is exactly zero emit no records (both passes then need d_enc); 0: every sample does
  uint32_t *counts, *offsets;       // [nlev * nb]: records per (level, bucket) and their exclusive prefix INSIDE the level
  uint32_t *wg_counts, *wg_prefix;  // [nlev][nwg][nb]: per-workgroup bucket histogram, and (hg_wgscan) its exclusive prefix over
  int nwg;                          // the workgroups of the level = each workgroup's private, atomics-free place in every bucket
  uint32_t* lmax;                   // [nlev][HB_LMAX_PARTS] bits of the max |record value| seen by each scatter workgroup of the level
                                    // ([..][0] = HB_POISON, set by hg_scan: the level's records do not fit its region)
  uint4* recs;                      // [nlev][cap] 16-byte records
  uint32_t cap;                     // record capacity per level
  int overwrite;                    // reduce: d_table slab = tile (zeros where untouched) instead of +=
};

// DPP row_shr:D -- lane l receives the value of lane l-D of its 16-lane row (0 when l%16 < D).  Pure VALU: unlike
// __shfl_up (ds_bpermute) it does not go through the LDS unit, which this kernel already loads with its atomics.
template <int D>
__device__ __forceinline__ float row_shr(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + D, 0xF, 0xF, true));
}
template <int D>
__device__ __forceinline__ uint32_t row_shr_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + D, 0xF, 0xF, true);
}
__device__ __forceinline__ int row_shl1(int v) {  // lane l <- lane l+1 of its row (0 at the row end)
  return __builtin_amdgcn_update_dpp(0, v, 0x101, 0xF, 0xF, true);
}
// 64-lane inclusive prefix sum on the VALU alone (gfx9 DPP: four shifts inside the 16-lane rows, then row_bcast:15 into rows 1 and 3
// and row_bcast:31 into the upper half): the scatter pass is bound by VALU + LDS issue, and a __shfl_up scan is six ds_bpermute
// round trips through the LDS unit per 64 values.
__device__ __forceinline__ uint32_t wave_scan_incl_dpp(uint32_t v) {
  v += row_shr_u<1>(v);
  v += row_shr_u<2>(v);
  v += row_shr_u<4>(v);
  v += row_shr_u<8>(v);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  return v;
}
// maximum over the 64 lanes, uniform result (row-wise DPP, then the four row results through readlane)
__device__ __forceinline__ uint32_t wave_max_u32_dpp(uint32_t v) {
  v = max(v, row_shr_u<1>(v)), v = max(v, row_shr_u<2>(v)), v = max(v, row_shr_u<4>(v)), v = max(v, row_shr_u<8>(v));  // lane 15 of a row: its max (values >= 0)
  return max(max((uint32_t)__builtin_amdgcn_readlane((int)v, 15), (uint32_t)__builtin_amdgcn_readlane((int)v, 31)),
             max((uint32_t)__builtin_amdgcn_readlane((int)v, 47), (uint32_t)__builtin_amdgcn_readlane((int)v, 63)));
}
template <int D>
__device__ __forceinline__ void seg_scan_step(float2 (&val)[8], bool& f, int l16) {
  const bool take = l16 >= D && !f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float px = row_shr<D>(val[c].x), py = row_shr<D>(val[c].y);
    if (take) val[c].x += px, val[c].y += py;
  }
  const int pf = (int)row_shr_u<D>((uint32_t)f);
  if (l16 >= D) f = f || pf;
}

// In-kernel phase stamps of the partitioned backward (tools/stamp_hg.py builds the hash grid unit with -DUMHS_HG_STAMP into its own library;
// no stamp executes in the product).  Every wave sums the cycles between consecutive stamps per phase and adds them to
// g_hg_stamp[kernel][level][phase] once, at its end; [..][15] counts the waves.  HG_STAMP_DRAIN also waits for the wave's outstanding
// vector-memory operations first, so that a phase that issues loads or stores is charged with their completion.
#ifdef UMHS_HG_STAMP
__device__ unsigned long long g_hg_stamp[2][16][16];
#define HG_STAMP_DECL unsigned long long hgs_acc_[15] = {}, hgs_t_ = hg_now_(false)
__device__ __forceinline__ unsigned long long hg_now_(bool drain) {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  if (drain) {
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  } else {
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  }
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define HG_STAMP(k_)                              \
  do {                                            \
    const unsigned long long n_ = hg_now_(false); \
    hgs_acc_[k_] += n_ - hgs_t_, hgs_t_ = n_;     \
  } while (0)
#define HG_STAMP_DRAIN(k_)                       \
  do {                                           \
    const unsigned long long n_ = hg_now_(true); \
    hgs_acc_[k_] += n_ - hgs_t_, hgs_t_ = n_;    \
  } while (0)
#define HG_STAMP_FLUSH(kern_, lev_)                                                                                     \
  do {                                                                                                                  \
    if ((threadIdx.x & 63) == 0) {                                                                                      \
      _Pragma("unroll") for (int q_ = 0; q_ < 15; ++q_) if (hgs_acc_[q_]) atomicAdd(&g_hg_stamp[kern_][(lev_) & 15][q_], hgs_acc_[q_]); \
      atomicAdd(&g_hg_stamp[kern_][(lev_) & 15][15], 1ull);                                                             \
    }                                                                                                                   \
  } while (0)
extern "C" int umhs_debug_hg_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hg_stamp), sizeof(unsigned long long) * 2 * 16 * 16);
}
extern "C" int umhs_debug_hg_stamps_clear() {
  static unsigned long long z[2 * 16 * 16] = {};
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_hg_stamp), z, sizeof(z));
}
#else
#define HG_STAMP_DECL \
  do {                \
  } while (0)
#define HG_STAMP(k_) \
  do {               \
  } while (0)
#define HG_STAMP_DRAIN(k_) \
  do {                     \
  } while (0)
#define HG_STAMP_FLUSH(kern_, lev_) \
  do {                              \
  } while (0)
#endif

// record meta word: [23:0] slot index inside the level (its bits above bucket_bits = the bucket), [27:24] k: the partner slot is
// slot ^ (2^(k+1) - 1); 15: no partner

// Everything a workgroup reads from memory for one run of HB_RUN samples.  Requested in ONE batch (hb_load), a whole run ahead
// of its use by the scatter pass's persistent workgroups: the stamps of round 4 showed the pass as a chain of dependent memory
// latencies per workgroup (level flag -> bucket counts / prefix -> barrier -> gradient -> position: 47 % of a wave's time at 12-16
// waves per CU) behind the CU's own queue of record stores, not as bandwidth.  Lanes past the end load the last sample
// (unconditional loads stay batched; a load under a per-lane condition compiles to a branch + s_waitcnt vmcnt(0)).
struct HbIn {
  float g[HB_SPT][2], p[HB_SPT][3];
  uint32_t c[2], mb[2];  // wave 0: this workgroup's record count in buckets lane / lane + 64 and where its slice of them starts
};

// the per-sample part; grad == false (the histogram pass of a prepare/apply pair runs before any gradient exists): zeros, d_enc unread
__device__ __forceinline__ void hb_load_samples(const HbArgs& a, const int wg, const int l, const bool grad, HbIn& in) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < HB_SPT; ++k) {
    const int64_t i = (int64_t)wg * HB_RUN + k * 256 + tid, ii = i < a.n ? i : a.n - 1;
    in.g[k][0] = in.g[k][1] = 0.0f;
    if (grad) {
      const float* g = a.d_enc + ii * a.sn + (int64_t)l * a.sl;
      if (((a.sn | a.sl) & 1) == 0 && (((uintptr_t)a.d_enc) & 7) == 0) {
        const float2 g2 = *reinterpret_cast<const float2*>(g);
        in.g[k][0] = g2.x, in.g[k][1] = g2.y;
      } else {
        in.g[k][0] = g[0], in.g[k][1] = g[1];
      }
    }
    in.p[k][0] = a.pos01[3 * ii], in.p[k][1] = a.pos01[3 * ii + 1], in.p[k][2] = a.pos01[3 * ii + 2];
  }
}

__device__ __forceinline__ void hb_load(const HbArgs& a, const int wg, const int lev, const int l, HbIn& in) {
  const int tid = threadIdx.x;
  hb_load_samples(a, wg, l, true, in);
  in.c[0] = in.c[1] = in.mb[0] = in.mb[1] = 0u;
  if (tid < 64) {  // the histogram pass left this workgroup's bucket counts and hg_wgscan its place in every bucket
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int bk = tid + 64 * h;
      if (bk < a.nb) {
        const size_t o = ((size_t)lev * a.nwg + wg) * a.nb + bk;
        in.c[h] = a.wg_counts[o];
        in.mb[h] = a.offsets[lev * a.nb + bk] + a.wg_prefix[o];
      }
    }
  }
}

// The record plan: which records a (sample, level) emits.  The histogram sizes every workgroup's slice of every bucket and the
// scatter pass fills the slices without a bounds check, so both take every decision from the helpers from here to hb_pair_split.
// Of the thread mapping it depends only on which samples share a wave (64 consecutive ones, aligned) and a 16-lane row.
// grad_mask (the one-call form, where the gradient exists before the histogram): a sample whose gradient is exactly zero emits nothing
__device__ __forceinline__ bool hb_active(const HbArgs& a, const int64_t i, const float g0, const float g1) {
  return i < a.n && (!a.grad_mask || g0 != 0.0f || g1 != 0.0f);
}

// cell identity: floor coordinates + "coordinate is an exact integer" flags (ceil == floor); unique per lane when inactive
struct HbKey { uint32_t x, y, z, f; };
__device__ __forceinline__ HbKey hb_cell_key(const HashCorners& h, const bool act, const int lane) {
  const uint32_t kx = act ? h.fx : 0xffffffffu, ky = act ? h.fy : 0u, kz = act ? h.fz : 0u;
  const uint32_t kf = act ? (h.eqx | (h.eqy << 1) | (h.eqz << 2)) : (0x80000000u | (uint32_t)lane);
  return HbKey{kx, ky, kz, kf};
}

// Runs of equal cells inside each 16-lane DPP row (all lanes execute it).  merging: the wave merges runs into 8 corner sums, emitted
// as singles; head: first lane of its run; tail: last lane of a run of active samples, which emits; solo: ... for a run of one: pairs
struct HbPlan { bool merging, head, tail, solo; };
__device__ __forceinline__ HbPlan hb_plan(const HbKey k, const bool act, const int lane) {
  HbPlan p;
  const int l16 = lane & 15;
  p.head = (l16 == 0) | (row_shr_u<1>(k.x) != k.x) | (row_shr_u<1>(k.y) != k.y) | (row_shr_u<1>(k.z) != k.z) | (row_shr_u<1>(k.f) != k.f);
  // Merging is a wave-wide decision (the scatter pass's segmented scan is ~450 VALU instructions per sample for all 64 lanes): taken
  // where it removes records in earnest -- a quarter of the wave's samples continue a run -- else every sample is a run of its own.
  p.merging = __builtin_popcountll(__builtin_amdgcn_ballot_w64(!p.head)) >= HB_MERGE_MIN;
  if (!p.merging) p.head = true;
  const int nhead = p.merging ? row_shl1((int)p.head) : 1;
  p.tail = act && (l16 == 15 || nhead);
  p.solo = p.head && p.tail;
  return p;
}

// the x-neighbours of all four pairs of a sample differ by the same pattern (xf ^ xc) & mask = 2^(k+1) - 1, or 0 where x is an integer
__device__ __forceinline__ uint32_t hb_pair_xor(const uint32_t (&slot)[8]) { return slot[HASH_FI[0]] ^ slot[HASH_CI[0]]; }
// ... and so live in two buckets all four or not at all (never below resolution 8192): every pair then becomes two single records
__device__ __forceinline__ bool hb_pair_split(const uint32_t (&slot)[8], const int bb) { return (hb_pair_xor(slot) >> bb) != 0; }

// The histogram of ONE sample per lane: the records the plan gives it, counted into the workgroup's bucket counters.  Called by
// hg_count_kernel below and by hashgrid_fwd_count_kernel: the gather has hashed every (sample, level) anyway and is bound by the vector-
// memory path, so the histogram pass -- 45 us, hidden on the side stream but 16 us of the step all the same -- rides along for free.
__device__ __forceinline__ void hb_count_sample(const uint32_t (&slot)[8], const HbKey key, const bool act, const int bb, const int lane,
                                                uint32_t* __restrict__ cursor) {
  const HbPlan pl = hb_plan(key, act, lane);
  if (pl.tail) {
    // a record per floor-x corner (pair or single), and per ceil-x corner where it does not ride in its partner's pair record
    // (written out: left as loops the compiler kept them rolled and moved slot[] into LDS for the dynamic index)
    atomicAdd(&cursor[slot[HASH_FI[0]] >> bb], 1u), atomicAdd(&cursor[slot[HASH_FI[1]] >> bb], 1u);
    atomicAdd(&cursor[slot[HASH_FI[2]] >> bb], 1u), atomicAdd(&cursor[slot[HASH_FI[3]] >> bb], 1u);
    if (!pl.solo || hb_pair_split(slot, bb)) {
      atomicAdd(&cursor[slot[HASH_CI[0]] >> bb], 1u), atomicAdd(&cursor[slot[HASH_CI[1]] >> bb], 1u);
      atomicAdd(&cursor[slot[HASH_CI[2]] >> bb], 1u), atomicAdd(&cursor[slot[HASH_CI[3]] >> bb], 1u);
    }
  }
}

// Histogram pass as a kernel of its own: gridDim.x workgroups per level walk the runs -- a caller that hides the pass under other
// kernels launches few, so that it takes a small, steady share of the CUs instead of flooding the dispatcher in front of them.
__global__ __launch_bounds__(256) void hg_count_kernel(HbArgs a) {
  __shared__ uint32_t cursor[HB_MAX_NB];
  const int tid = threadIdx.x, lane = tid & 63, lev = a.lev_off + blockIdx.y, l = a.level0 + lev;
  const float s = a.scalings[l];
  const uint32_t mask = (1u << a.log2_T) - 1u;
  for (int wg = blockIdx.x; wg < a.nwg; wg += gridDim.x) {
    HbIn in;
    hb_load_samples(a, wg, l, a.grad_mask != 0, in);  // (in flight over the barrier)
    if (tid < HB_MAX_NB) cursor[tid] = 0;             // (by the thread that has just written the entry out)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < HB_SPT; ++k) {
      const bool act = hb_active(a, (int64_t)wg * HB_RUN + k * 256 + tid, in.g[k][0], in.g[k][1]);
      const HashCorners h = hash_corners(in.p[k][0], in.p[k][1], in.p[k][2], s, mask, 0u);
      hb_count_sample(h.idx, hb_cell_key(h, act, lane), act, a.bucket_bits, lane, cursor);
    }
    __syncthreads();
    if (tid < a.nb) a.wg_counts[((size_t)lev * a.nwg + wg) * a.nb + tid] = cursor[tid];
  }
}

// Scatter pass, one run of HB_RUN samples: place the run's records by bucket in LDS, then write them into the workgroup's slices.
__device__ __forceinline__ void hg_scatter_body(const HbArgs& a, const int wg, const int lev, const int l, const float s, const HbIn& in,
                                                uint32_t& wgmax) {
  // cursor[b]: where the next record of bucket b goes in the LDS staging array (starts at the run's first place, so a returning
  // atomic add IS the place).  delta[b]: (global place) - (staged place) of bucket b.
  __shared__ uint32_t cursor[HB_MAX_NB];
  __shared__ uint32_t delta[HB_MAX_NB];
  __shared__ uint32_t ltotal;
  // records are first ordered by bucket in LDS, then written out with consecutive lanes on consecutive records
  // (tools/mb_scatter_store.hip: 5.7 TB/s in this shape, 3.2 TB/s with every lane storing its own record where it belongs)
  constexpr int MAXREC = HB_RUN * 4;
  __shared__ uint4 stage[MAXREC];
  const int tid = threadIdx.x, lane = tid & 63;
  HG_STAMP_DECL;
  // nothing is counted again and no global cursor is touched -- wave 0 turns the workgroup's bucket counts into LDS offsets
  if (tid < 64) {
    uint32_t carry = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int bk = tid + 64 * h;
      const uint32_t c = in.c[h], mb = in.mb[h];
      const uint32_t incl = wave_scan_incl_dpp(c);
      const uint32_t first = carry + incl - c;
      carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      // this workgroup's slice of the bucket: bucket start + the records of the workgroups before it -- no cursor atomics
      cursor[bk] = first, delta[bk] = mb - first;
    }
    if (tid == 0) ltotal = carry;
  }
  __syncthreads();
  const uint32_t mask = (1u << a.log2_T) - 1u;
  const int bb = a.bucket_bits;
  uint4* const __restrict__ out = a.recs + (size_t)lev * a.cap;
  const bool staged = ltotal <= (uint32_t)MAXREC;  // (pairs split over two buckets can exceed 4 per sample: then straight to memory)
  HG_STAMP_DRAIN(0);
  // max |record value| of the level as raw bits: for non-negative floats the integer order is the float order, and an Inf / NaN
  // pattern (>= 0x7f800000) beats every finite one -- hg_reduce turns a level that saw one into NaN gradients instead of
  // an arbitrary fixed-point conversion (fmaxf would silently drop a NaN; the reference's index_add propagates it)
  uint32_t vmax = 0u;
  auto put = [&](const uint32_t b, const uint32_t pos, const uint32_t meta, const float vx, const float vy, const float ox) {
    const uint4 r = make_uint4(__float_as_uint(vx), __float_as_uint(vy), __float_as_uint(ox), meta);
    if (staged)
      stage[pos] = r;
    else
      out[delta[b] + pos] = r;
  };
  auto emit = [&](const uint32_t meta, const float vx, const float vy, const float ox) {  // meta = slot index | k << 24
    const uint32_t b = __builtin_amdgcn_ubfe(meta, (uint32_t)bb, (uint32_t)(24 - bb));
    put(b, atomicAdd(&cursor[b], 1u), meta, vx, vy, ox);
  };
#pragma unroll
  for (int k = 0; k < HB_SPT; ++k) {
    const int64_t i = (int64_t)wg * HB_RUN + k * 256 + tid;
    HG_STAMP_DRAIN(1);
    const float g0 = in.g[k][0], g1 = in.g[k][1];
    const bool act = hb_active(a, i, g0, g1);
    HashCorners h{};  // (an inactive lane emits nothing: its slots and offsets are never used)
    if (act) h = hash_corners(in.p[k][0], in.p[k][1], in.p[k][2], s, mask, 0u);  // base 0: idx = the slot inside the level
    const float ox = h.ox, oy = h.oy, oz = h.oz;
    const HbKey key = hb_cell_key(h, act, lane);
    HG_STAMP(2);
    const HbPlan pl = hb_plan(key, act, lane);
    const float rx = 1.0f - ox, ry = 1.0f - oy, rz = 1.0f - oz;
    float2 val[8];
    // the 8 corner sums of a merged run: segmented inclusive scan over the row, (f, v) (+) (pf, pv) = (f | pf, f ? v : v + pv)
    if (pl.merging) {
      const int l16 = lane & 15;
      float w[8];
      hash_corner_weights(ox, oy, oz, w);
#pragma unroll
      for (int c = 0; c < 8; ++c) val[c] = act ? make_float2(w[c] * g0, w[c] * g1) : make_float2(0.0f, 0.0f);
      bool f = pl.head;
      seg_scan_step<1>(val, f, l16), seg_scan_step<2>(val, f, l16);
      seg_scan_step<4>(val, f, l16), seg_scan_step<8>(val, f, l16);
    }
    HG_STAMP(3);
    if (pl.tail) {
      const uint32_t single = 15u << 24;
      if (pl.solo) {
        const float wyz[4] = {oy * oz, ry * oz, oy * rz, ry * rz};  // (y, z) weight of x-pair p: (c,c) (f,c) (c,f) (f,f)
        vmax = max(vmax, max(__float_as_uint(fabsf(g0)), __float_as_uint(fabsf(g1))));  // |g wyz| <= |g|: one maximum per sample
        if (!hb_pair_split(h.idx, bb)) {  // both corners in one bucket: one record, the reduce pass splits it
          const uint32_t pm = hb_pair_xor(h.idx);
          const uint32_t km = (pm ? (uint32_t)(31 - __clz((int)pm)) : 15u) << 24;  // (pm == 0: x is an integer, ox == 0, all weight on the floor slot)
          // (the four places first, then the four records: four returning LDS atomics in flight instead of one round trip per record)
          uint32_t meta[4], pos[4], bk[4];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            meta[p] = h.idx[HASH_FI[p]] | km;
            bk[p] = __builtin_amdgcn_ubfe(meta[p], (uint32_t)bb, (uint32_t)(24 - bb));
            pos[p] = atomicAdd(&cursor[bk[p]], 1u);
          }
#pragma unroll
          for (int p = 0; p < 4; ++p) put(bk[p], pos[p], meta[p], g0 * wyz[p], g1 * wyz[p], ox);
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const float gx = g0 * wyz[p], gy = g1 * wyz[p];
            emit(h.idx[HASH_FI[p]] | single, gx * rx, gy * rx, 0.0f);
            emit(h.idx[HASH_CI[p]] | single, gx * ox, gy * ox, 0.0f);
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          vmax = max(vmax, max(__float_as_uint(fabsf(val[c].x)), __float_as_uint(fabsf(val[c].y))));
          emit(h.idx[c] | single, val[c].x, val[c].y, 0.0f);
        }
      }
    }
    HG_STAMP(4);
  }
  vmax = wave_max_u32_dpp(vmax);
  if (lane == 0 && vmax > 0u) atomicMax(&wgmax, vmax);  // (LDS; the kernel writes the workgroup's maximum out once, after its last run)
  HG_STAMP(5);
  __syncthreads();
  HG_STAMP(6);
  if (staged) {
    // byte offsets inside the level's record region fit 32 bits (umhs_hashgrid_bwd_workspace_bytes): scalar base + 32-bit offset stores
    char* const ob = reinterpret_cast<char*>(out);
    const uint32_t total = ltotal;
    for (uint32_t i = tid; i < total; i += 256) {
      const uint4 r = stage[i];
      const uint32_t b = __builtin_amdgcn_ubfe(r.w, (uint32_t)bb, (uint32_t)(24 - bb));
      *reinterpret_cast<uint4*>(ob + (size_t)((delta[b] + i) << 4)) = r;
    }
  }
  HG_STAMP_DRAIN(7);
  HG_STAMP_FLUSH(0, l);
}

// Scatter pass: PERSISTENT workgroups, gridDim.x (a multiple of 8) per level; each walks its runs of samples with the next run's
// inputs in flight (hb_load above).  Which runs: workgroups go to the 8 XCDs round-robin by their linear index, and the runs wg,
// wg + 1 write ADJACENT record runs in every bucket (short ones on the coarse levels: most 128-byte lines of the record stream are
// shared by neighbouring runs) -- XCD x takes the CONTIGUOUS runs [x * per, (x + 1) * per) and its workgroups interleave inside
// that range, so that neighbouring runs are written through the same L2 at about the same time and their partial lines combine
// there (tools/mb_scatter_store.hip: 16-byte pieces 3.3 vs 1.3 TB/s, 32-byte 5.7 vs 2.7).
__global__ __launch_bounds__(256) void hg_scatter_kernel(HbArgs a) {
  const int lev = a.lev_off + blockIdx.y, l = a.level0 + lev;
  const float s = a.scalings[l];
  __shared__ uint32_t wgmax;
  HbIn cur;
  if (threadIdx.x == 0) wgmax = 0;  // (ordered before its first use by the barrier inside the body)
  const int per = (a.nwg + 7) >> 3, q = (int)(gridDim.x >> 3);  // runs per XCD, workgroups per XCD (and level)
  const int x = (int)(blockIdx.x & 7u), end = min(a.nwg, (x + 1) * per);
  int wg = x * per + (int)(blockIdx.x >> 3);
  const uint32_t lmax0 = a.lmax[(size_t)lev * HB_LMAX_PARTS];
  if (wg >= end) return;
  hb_load(a, wg, lev, l, cur);
  if (lmax0 == HB_POISON) return;  // (uniform) the level's records do not fit its region: hg_reduce writes NaN
  while (true) {
    const int nxt = wg + q;
    HbIn nx;
    if (nxt < end) hb_load(a, nxt, lev, l, nx);  // (uniform branch)
    hg_scatter_body(a, wg, lev, l, s, cur, wgmax);
    if (nxt >= end) break;
    cur = nx, wg = nxt;
    __syncthreads();  // the write-out of this run has read the staged records before the next run's placement overwrites them
  }
  __syncthreads();
  // a plain store into the workgroup's own word (hg_scan zeroed them): no atomic, nothing shared
  if (threadIdx.x == 0 && wgmax) a.lmax[(size_t)lev * HB_LMAX_PARTS + (blockIdx.x % HB_LMAX_PARTS)] = wgmax;
}

// Per (level, bucket): exclusive prefix of the per-workgroup bucket counts over the level's workgroups, and the bucket total.
// One 256-thread workgroup per (bucket, level): a thread sums its run of consecutive workgroups, the runs are scanned across the
// block, and the thread writes its run's prefixes.  Also clears the level's max-|value| word for the scatter pass.
__global__ __launch_bounds__(256) void hg_wgscan_kernel(HbArgs a) {
  __shared__ uint32_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x, lev = blockIdx.y;
  const int per = (a.nwg + 255) / 256, w0 = min(a.nwg, tid * per), w1 = min(a.nwg, w0 + per);
  const uint32_t* __restrict__ col = a.wg_counts + (size_t)lev * a.nwg * a.nb + b;
  uint32_t* __restrict__ pre = a.wg_prefix + (size_t)lev * a.nwg * a.nb + b;
  uint32_t sum = 0;
  for (int w = w0; w < w1; ++w) sum += col[(size_t)w * a.nb];
  uint32_t incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  uint32_t run = incl - sum, total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < wv) run += wsum[k];
    total += wsum[k];
  }
  for (int w = w0; w < w1; ++w) {
    pre[(size_t)w * a.nb] = run;
    run += col[(size_t)w * a.nb];
  }
  if (tid == 0) a.counts[lev * a.nb + b] = total;
}

// One wave per level: exclusive scan of the level's bucket counts (nb <= 128: two per lane) -> offsets inside the level's record
// region; sets the level's max-|value| word to 0, or to HB_POISON when its records exceed the region.
__global__ void hg_scan_kernel(HbArgs a) {
  const int lane = threadIdx.x, lev = blockIdx.x;
  uint32_t carry = 0;
  for (int b0 = 0; b0 < a.nb; b0 += 64) {
    const int b = b0 + lane;
    const uint32_t c = b < a.nb ? a.counts[lev * a.nb + b] : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (b < a.nb) a.offsets[lev * a.nb + b] = carry + incl - c;
    carry += __shfl(incl, 63, 64);
  }
  for (int j = lane; j < HB_LMAX_PARTS; j += 64) a.lmax[(size_t)lev * HB_LMAX_PARTS + j] = (j == 0 && carry > a.cap) ? HB_POISON : 0u;
}

// x = value * 2^(k - 32) -> floor(value * 2^k) as a 64-bit two's complement integer: hi = floor(x) (signed), lo = (x - floor(x)) * 2^32
// Six VALU instructions; __float2ll_rn(ldexpf(v, k)) compiles to fourteen, and the record phase of the reduce pass -- four
// conversions per record -- was bound by exactly that plus the LDS atomics (round 4: records stream at 3.2 TB/s, the Adam epilogue at
// the HBM rate).  The same result for every order of the addends.  Error per addend, in units of the tile (2^-32 of x, 2^-kfix of the
// value): below 1 (the floor) for x >= 0 and for x <= -1, where the remainder x - floorf(x) is exact; UP TO 128 for -1 < x < 0, where
// the remainder 1 + x is rounded to float32's spacing of 2^-24 below 1 (-7.8 units become -1, -197 units become -256) -- and where it
// rounds to 1.0f, 2^32 is converted to uint32_t, which is out of range in C++ and right only because v_cvt_u32_f32 saturates to
// 2^32 - 1.  With kfix = 62 - hb - e that is <= 2^(hb - 54) of the level's largest record per addend: 2^-39 of it in a bucket of
// 8192..16383 records (hb = 15), not the 2^-46 the unit alone suggests.  Harmless in absolute terms, but a slot fed only by negative
// addends of that size has a relative error of up to 100 %; tests/hash_f64.py carries 128 units per addend in its per-slot rule and
// tests/test_hash_f64_bounds_cpu.py sweeps an emulation of this function to hold the figure.  Inlined into hg_reduce_kernel, where x
// is a product v * w and contraction is on, hipcc forms the remainder as ONE v_fma_f32(v, w, -fl): from the unrounded product.  That
// costs nothing (the remainder is then closer to the true product than x is), but where rounding carried x up to an integer the
// remainder is slightly negative and the conversion saturates at its other end, to 0: both ends of v_cvt_u32_f32 are relied on.
__device__ __forceinline__ unsigned long long hb_fixed(const float x) {
  const float fl = floorf(x);
  const int hi = (int)fl;
  const uint32_t lo = (uint32_t)((x - fl) * 4294967296.0f);
  return ((unsigned long long)(uint32_t)hi << 32) | lo;
}

// 16-byte accesses with the non-temporal hint (global_load / global_store_dwordx4 ... nt), for the reduce pass's streams that nothing
// touches again this step: the records (written once by the scatter pass, read once here) and the gradient slab, exp_avg and
// exp_avg_sq as they are stored.  NOT for the parameters, which the next step's gather reads.  Measured on one MI355X
// (profiles/hashgrid/reduce_overlap_ab.json): hg_reduce_kernel in the C2 step 124 -> 105 us, most of it from the hint on the record loads; the
// supposed reason -- 591 MB pass through an L2 of 4 MiB per XCD, and lines nobody reads again stop displacing the others -- has not
// been checked against counters.
typedef uint32_t hb_u32x4 __attribute__((ext_vector_type(4)));
typedef float hb_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 hb_load_stream(const uint4* p) {
  const hb_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const hb_u32x4*>(p));
  return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void hb_store_stream(float* p, const float4& v) {
  const hb_f32x4 t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<hb_f32x4*>(p));
}

__global__ __launch_bounds__(1024) void hg_reduce_kernel(HbArgs a, float* __restrict__ d_table) {
  extern __shared__ __attribute__((aligned(16))) long long tile[];  // [2 << bucket_bits] int64 fixed point
  // (levels in dispatch order.  Last level first -- the records the scatter pass wrote last are the likeliest to sit in the 256 MiB
  // Infinity Cache -- was measured in round 4: 211-220 vs 186-204 us at C2, 361-382 vs 325-347 us at C5.  Dropped.)
  const int tid = threadIdx.x, b = blockIdx.x, lev = a.lev_off + blockIdx.y, l = a.level0 + lev;
  HG_STAMP_DECL;
  const uint32_t start = a.offsets[lev * a.nb + b], cnt = a.counts[lev * a.nb + b];
  const int nsl = 2 << a.bucket_bits;
  const size_t slab = 2 * (((size_t)l << a.log2_T) + ((size_t)b << a.bucket_bits));  // element offset of this (level, bucket)
  const bool adam = a.adam.p != nullptr && l >= a.adam.level_begin;
  auto step4 = [&](const float4& g, float4& pp, float4& mm, float4& vv) {  // Adam on 4 consecutive table entries whose final gradient is g
    adam_update(pp.x, mm.x, vv.x, g.x, a.adam.lr_bc1, a.adam.b1, a.adam.b2, a.adam.eps, a.adam.sqrt_bc2);
    adam_update(pp.y, mm.y, vv.y, g.y, a.adam.lr_bc1, a.adam.b1, a.adam.b2, a.adam.eps, a.adam.sqrt_bc2);
    adam_update(pp.z, mm.z, vv.z, g.z, a.adam.lr_bc1, a.adam.b1, a.adam.b2, a.adam.eps, a.adam.sqrt_bc2);
    adam_update(pp.w, mm.w, vv.w, g.w, a.adam.lr_bc1, a.adam.b1, a.adam.b2, a.adam.eps, a.adam.sqrt_bc2);
  };
  // epilogue of every path: the slab's gradient (+ its Adam step) as float4 lanes; the optimizer operands of a thread's (up to)
  // four chunks are requested before anything is computed -- three loads in flight per chunk, not three per thread
  // the level's max |value| = max over its scatter workgroups' words (one word per lane, L2 hits; every wave computes it for itself)
  const uint32_t lmax_bits =
      wave_max_u32_dpp(max(a.lmax[(size_t)lev * HB_LMAX_PARTS + (tid & 63)], a.lmax[(size_t)lev * HB_LMAX_PARTS + 64 + (tid & 63)]));
  // a non-finite gradient reached this level: the slabs its records land in are NaN, as after the reference's index_add; a level
  // whose records did not fit its region (HB_POISON) is NaN everywhere
  const bool nan_level = lmax_bits >= 0x7f800000u && (cnt != 0 || lmax_bits == HB_POISON);
  const bool from_tile = cnt != 0 && !nan_level;
  if (!from_tile && !a.overwrite && !nan_level) return;  // nothing lands in this slab and it is not ours to zero
  int kfix = 0;
  if (from_tile) {
    for (int i = tid; i < nsl; i += 1024) tile[i] = 0;
    // fixed-point scale 2^k:  |v| <= vmax < 2^e, at most cnt < 2^hb addends  =>  |sum| * 2^k < 2^62
    int e;
    (void)frexpf(__uint_as_float(lmax_bits), &e);
    const int hb = 33 - __clz(cnt);  // cnt < 2^(32-clz) ; one spare bit
    kfix = min(62 - hb - e, 150);  // (2^(kfix - 32) must be a finite float: levels whose largest |value| is below 2^-60)
    __syncthreads();
    const uint4* __restrict__ rp = a.recs + (size_t)lev * a.cap + start;
    typedef unsigned long long u64;
    u64* ut = reinterpret_cast<u64*>(tile);
    const uint32_t lowmask = (1u << a.bucket_bits) - 1u;
    const float fscale = ldexpf(1.0f, kfix - 32);
    auto add = [&](const uint4& r) {
      const float vx = __uint_as_float(r.x), vy = __uint_as_float(r.y), ox = __uint_as_float(r.z);
      const uint32_t s = r.w & lowmask, kk = (r.w >> 24) & 15u;
      const float rx = (1.0f - ox) * fscale, oxs = ox * fscale;  // the weights carry the fixed-point scale 2^(kfix - 32)
      atomicAdd(&ut[2 * s], hb_fixed(vx * rx)), atomicAdd(&ut[2 * s + 1], hb_fixed(vy * rx));
      if (kk != 15u) {
        const uint32_t cs = s ^ (((2u << kk) - 1u) & lowmask);
        atomicAdd(&ut[2 * cs], hb_fixed(vx * oxs)), atomicAdd(&ut[2 * cs + 1], hb_fixed(vy * oxs));
      }
    };
    uint32_t i = tid;
    HG_STAMP(0);
    // 4 records per thread and batch, the NEXT batch requested before this one is accumulated (every record slot past the end
    // re-reads the bucket's last record and is dropped: unconditional loads stay batched).  Two register sets in turn, no copies:
    // with `r = n` moves at the loop's end hipcc waits for vmcnt(0) at its top -- in front of the next requests -- and nothing overlaps.
    const uint32_t last = cnt - 1;
    auto load4 = [&](uint4 (&r)[4], const uint32_t at) {
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = hb_load_stream(rp + min(at + 1024u * u, last));
    };
    auto add4 = [&](const uint4 (&r)[4], const uint32_t at) {
      add(r[0]);
#pragma unroll
      for (int u = 1; u < 4; ++u)
        if (at + 1024u * u < cnt) add(r[u]);
    };
    uint4 ra[4], rb[4];
    if (i < cnt) {
      load4(ra, i);
      while (true) {
        HG_STAMP_DRAIN(1);
        load4(rb, i + 4096u);
        add4(ra, i);
        HG_STAMP(3);
        i += 4096u;
        if (i >= cnt) break;
        HG_STAMP_DRAIN(1);
        load4(ra, i + 4096u);
        add4(rb, i);
        HG_STAMP(3);
        i += 4096u;
        if (i >= cnt) break;
      }
    }
    HG_STAMP_DRAIN(3);
    __syncthreads();
    HG_STAMP(4);
  }
  float* const dst = d_table + slab;
  const float qnan = __uint_as_float(0x7fc00000u);
  for (int j0 = tid * 4; j0 < nsl; j0 += 4 * 4096) {
    float4 pp[4], mm[4], vv[4], dd[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = min(j0 + c * 4096, nsl - 4);  // (chunks past the slab re-read its last float4 and are not stored)
      if (adam) {
        pp[c] = *reinterpret_cast<const float4*>(a.adam.p + slab + j), mm[c] = *reinterpret_cast<const float4*>(a.adam.m + slab + j);
        vv[c] = *reinterpret_cast<const float4*>(a.adam.v + slab + j);
      }
      if (!a.overwrite) dd[c] = *reinterpret_cast<const float4*>(dst + j);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + c * 4096;
      if (j < nsl) {
        float4 d = a.overwrite ? make_float4(0.f, 0.f, 0.f, 0.f) : dd[c];
        if (nan_level) {
          d = make_float4(qnan, qnan, qnan, qnan);
        } else if (from_tile) {
          d.x += (float)ldexp((double)tile[j], -kfix), d.y += (float)ldexp((double)tile[j + 1], -kfix);
          d.z += (float)ldexp((double)tile[j + 2], -kfix), d.w += (float)ldexp((double)tile[j + 3], -kfix);
        }
        hb_store_stream(dst + j, d);
        // The gradient of these entries is final here (one GPU, overwrite mode): update them in place of a separate pass -- the
        // 67 MB gradient is not read back and the stand-alone Adam launch shrinks to the MLP tail + the sparse rows.  (A slab no
        // record lands in still steps: with a zero gradient the moments decay and move the entry.)
        if (adam) {
          step4(d, pp[c], mm[c], vv[c]);
          *reinterpret_cast<float4*>(a.adam.p + slab + j) = pp[c];
          hb_store_stream(a.adam.m + slab + j, mm[c]);
          hb_store_stream(a.adam.v + slab + j, vv[c]);
        }
      }
    }
  }
  HG_STAMP_DRAIN(5);
  HG_STAMP_FLUSH(1, l);
}
