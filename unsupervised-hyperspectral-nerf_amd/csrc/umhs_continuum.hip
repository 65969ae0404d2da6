// Continuum removal (include/umhs_hip.h, "Continuum removal"): per row the upper convex hull of (lambda_b, x_b) over a band range, the
// row divided by it, and depth / centre / area of up to 8 absorption features, each on the hull of its own range.  One launch.
//
//   block      ONE wave and its 64 rows, lane l <-> row l of the tile; nothing is shared between waves.  A hull is a data-dependent
//              sequential walk, so a row is one lane's work from start to end and its result depends on nothing but the row.
//   LDS        the tile's rows (coalesced loads: lane l takes element l + 64 k of the 64 x B tile), beside each row its hull stack
//              -- band indices, one byte each -- and the wavelengths once: 5 B bytes per row plus padding.  A row's pitch is B | 1
//              dwords and a stack's an odd number of dwords: lanes that stand at the same band (or the same stack depth) then hit 32
//              different banks (ds_read_b32 / ds_write_b32 / byte accesses: bank = dword mod 32 within each 32-lane half).  At
//              B = 256 the padding would not leave room for two workgroups in 160 KiB, so there the pitches are 256 and 64 dwords and
//              lane l keeps band b at dword (b + l) mod 256 of its row and stack byte d at byte (d + 4 l) mod 256: the same banks.
//              B = 31: 10 KiB per workgroup, 16 of them per CU; B = 256: 80 KiB, two.  The wavelengths join the LDS image when two
//              workgroups still fit with them (B <= 252); above that they are read from global memory (1 KiB, resident in L1).
//   walk       monotone chain, written as ONE loop: a trip either pops the last vertex or pushes the band and advances, so a lane does
//              at most 2 n - 3 trips over n bands and lanes that diverge never run nested loops of different trip counts.  The two
//              top vertices live in registers (index, wavelength, value); a pop reloads the one under them by its stack byte.
//   evaluate   one loop over the bands of the range, the same trip count on every lane, with a per-lane segment pointer into the
//              stack: c_b, r_b, the running minimum and the trapezoid sum.  The full range is evaluated LAST and writes r over x in
//              place (a band is read before it is written; the segment's ends are in registers), so `removed` leaves through the
//              same coalesced mapping the rows came in by.  The features go out lane by lane (3 F floats per row).
//   arithmetic plain operators with contraction OFF for this unit (the pragma below: no product and sum are fused into an fma; the
//              only fmas in the object are those of the IEEE division expansions), so every float32 operation is rounded once, in
//              the order of include/umhs_hip.h, and a float32 replay on the host gives the same bits.
#include "umhs_common.h"

#include <atomic>

#pragma clang fp contract(off)

namespace {

constexpr int CR_MAX_B = UMHS_CONTINUUM_MAX_BANDS, CR_MAX_F = UMHS_CONTINUUM_MAX_FEATURES, CR_ROWS = 64;
constexpr int CR_STAGE = 16;  // loads in flight per lane while a tile is staged
constexpr size_t CR_LDS_PER_CU = 160 * 1024;
constexpr float CR_FLT_MAX = 3.402823466e38f;

struct CrRanges {  // inclusive band ranges: [0] the full range, [1 + f] feature f
  int lo[CR_MAX_F + 1], hi[CR_MAX_F + 1];
};

inline __host__ __device__ int cr_row_pitch(int B) { return B == 256 ? 256 : (B | 1); }                    // dwords
inline __host__ __device__ int cr_stack_pitch(int B) { return B == 256 ? 64 : (((B + 3) >> 2) | 1); }     // dwords
inline size_t cr_lds_bytes(int B, bool lam_lds) {
  return (size_t)CR_ROWS * 4 * (cr_row_pitch(B) + cr_stack_pitch(B)) + (lam_lds ? 4 * (size_t)B : 0);
}
inline bool cr_lam_in_lds(int B) { return 2 * cr_lds_bytes(B, true) <= CR_LDS_PER_CU; }

struct CrLane {  // one lane's view of its row, its stack and the wavelengths
  float* x;
  unsigned char* st;
  const float* lam;
  int xrot, srot, mask;  // (B = 256: lane, 4 lane, 255; else 0, 0, all ones)
  __device__ __forceinline__ float X(int b) const { return x[(b + xrot) & mask]; }
  __device__ __forceinline__ void setX(int b, float v) const { x[(b + xrot) & mask] = v; }
  __device__ __forceinline__ int S(int d) const { return st[(d + srot) & mask]; }
  __device__ __forceinline__ void setS(int d, int b) const { st[(d + srot) & mask] = (unsigned char)b; }
};

// The vertices of the upper hull of bands lo..hi, ascending, into the stack; -> how many.
__device__ __forceinline__ int cr_hull(const CrLane& L, int lo, int hi) {
  int top = 1, i0 = lo, i1 = lo, b = lo + 1;
  float l1 = L.lam[lo], x1 = L.X(lo), l0 = l1, x0 = x1, lb = l1, xb = x1;
  L.setS(0, lo);
  if (b <= hi) lb = L.lam[b], xb = L.X(b);
  while (b <= hi) {
    bool pop = false;
    if (top >= 2) {  // the turn p0 -> p1 -> b is strictly clockwise when this is < 0
      const float cross = (l1 - l0) * (xb - x0) - (x1 - x0) * (lb - l0);
      pop = !(cross < 0.0f);
    }
    if (pop) {
      --top, i1 = i0, l1 = l0, x1 = x0;
      if (top >= 2) i0 = L.S(top - 2), l0 = L.lam[i0], x0 = L.X(i0);
    } else {
      L.setS(top, b);
      ++top, i0 = i1, l0 = l1, x0 = x1, i1 = b, l1 = lb, x1 = xb, ++b;
      if (b <= hi) lb = L.lam[b], xb = L.X(b);
    }
  }
  return top;
}

// c, r over lo..hi from the stack's `depth` vertices: the minimum of r, its first band, the trapezoid sum of 1 - r; WRITE: r over x
template <bool WRITE>
__device__ __forceinline__ void cr_eval(const CrLane& L, int lo, int hi, int depth, float& rmin, int& m, float& area) {
  int i = lo, j = hi + 1, s = 1;
  float li = L.lam[lo], xi = L.X(lo), lj = li, xj = xi;
  if (depth >= 2) j = L.S(1), lj = L.lam[j], xj = L.X(j);
  rmin = INFINITY, m = lo, area = 0.0f;
  float qprev = 0.0f, lprev = li;
  for (int b = lo; b <= hi; ++b) {
    if (b == j) {  // the next segment
      i = j, li = lj, xi = xj, ++s;
      if (s < depth) j = L.S(s), lj = L.lam[j], xj = L.X(j);
      else j = hi + 1;
    }
    const float lb = L.lam[b];
    float xb = xi, c = xi;
    if (b != i) {
      xb = L.X(b);
      c = xi + ((lb - li) / (lj - li)) * (xj - xi);
    }
    const float r = c > 0.0f ? xb / c : 1.0f;
    if (WRITE) L.setX(b, r);
    if (r < rmin) rmin = r, m = b;
    const float q = 1.0f - r;
    if (b > lo) area = area + (0.5f * (lb - lprev)) * (qprev + q);
    qprev = q, lprev = lb;
  }
}

template <bool LAM_LDS>
__global__ __launch_bounds__(CR_ROWS) void continuum_kernel(const float* __restrict__ spectra, int64_t stride, int64_t R,
                                                            const float* __restrict__ wavelengths, int B, CrRanges rg, int F,
                                                            float* __restrict__ removed, float* __restrict__ features,
                                                            int* __restrict__ status) {
  extern __shared__ float cr_lds[];
  const int lane = threadIdx.x, P = cr_row_pitch(B), SP = cr_stack_pitch(B);
  const bool rot = B == 256;
  float* sX = cr_lds;
  unsigned char* sS = reinterpret_cast<unsigned char*>(cr_lds + CR_ROWS * P);
  float* sL = cr_lds + CR_ROWS * (P + SP);
  const int64_t row0 = (int64_t)blockIdx.x * CR_ROWS;
  const int mask = rot ? 255 : 0x7fffffff, step_r = CR_ROWS / B, step_b = CR_ROWS % B;

  {  // the tile in: lane l takes elements l, l + 64, .. of the 64 x B tile, row-major; CR_STAGE loads are in flight before the first
     // LDS store waits for one (a load and its store per trip left a lone wave waiting out the whole memory latency B times)
    int r = lane / B, b = lane - r * B;
    for (int k0 = 0; k0 < B; k0 += CR_STAGE) {
      float v[CR_STAGE];
      int at[CR_STAGE];
#pragma unroll
      for (int u = 0; u < CR_STAGE; ++u) {
        const bool in = k0 + u < B;
        const int64_t gr = row0 + r;
        at[u] = in ? r * P + ((b + (rot ? r : 0)) & mask) : -1;
        v[u] = (in && gr < R) ? spectra[gr * stride + b] : 0.0f;
        b += step_b, r += step_r;
        if (b >= B) b -= B, ++r;
      }
#pragma unroll
      for (int u = 0; u < CR_STAGE; ++u)
        if (at[u] >= 0) sX[at[u]] = v[u];
    }
    if (LAM_LDS)
      for (int b2 = lane; b2 < B; b2 += CR_ROWS) sL[b2] = wavelengths[b2];
  }
  __syncthreads();

  const int64_t r = row0 + lane;
  if (r < R) {
    const CrLane L = {sX + lane * P, sS + lane * SP * 4, LAM_LDS ? sL : wavelengths, rot ? lane : 0, rot ? 4 * lane : 0, mask};
    bool valid = true;
    for (int b = 0; b < B; ++b) valid = valid && fabsf(L.X(b)) <= CR_FLT_MAX;  // (false for a NaN)
    if (valid) {
      float rmin, area;
      int m;
      for (int f = 0; f < F; ++f) {
        const int lo = rg.lo[1 + f], hi = rg.hi[1 + f];
        const int depth = cr_hull(L, lo, hi);
        cr_eval<false>(L, lo, hi, depth, rmin, m, area);
        float* out = features + (r * F + f) * 3;
        out[0] = 1.0f - rmin, out[1] = L.lam[m], out[2] = area;
      }
      if (removed || status) {
        const int depth = cr_hull(L, rg.lo[0], rg.hi[0]);
        if (removed) cr_eval<true>(L, rg.lo[0], rg.hi[0], depth, rmin, m, area);
        if (status) status[r] = depth;
      }
    } else {
      for (int f = 0; f < 3 * F; ++f) features[r * F * 3 + f] = 0.0f;
      if (removed)
        for (int b = 0; b < B; ++b) L.setX(b, 0.0f);
      if (status) status[r] = -1;
    }
  }
  if (!removed) return;  // (uniform)
  __syncthreads();
  {  // r out, by the mapping the rows came in by
    int r2 = lane / B, b = lane - r2 * B;
    for (int k0 = 0; k0 < B; k0 += CR_STAGE) {
      float v[CR_STAGE];
      int64_t to[CR_STAGE];
#pragma unroll
      for (int u = 0; u < CR_STAGE; ++u) {
        const int64_t gr = row0 + r2;
        const bool in = k0 + u < B && gr < R;
        to[u] = in ? gr * B + b : -1;
        v[u] = in ? sX[r2 * P + ((b + (rot ? r2 : 0)) & mask)] : 0.0f;
        b += step_b, r2 += step_r;
        if (b >= B) b -= B, ++r2;
      }
#pragma unroll
      for (int u = 0; u < CR_STAGE; ++u)
        if (to[u] >= 0) removed[to[u]] = v[u];
    }
  }
}

// Raises the kernel's dynamic-LDS limit once per instantiation and device (B = 256 takes 80 KiB).  The template parameter is the
// kernel's own: both instantiations have one pointer type, and a cache keyed by that type would let one's grant stand for the other.
template <bool LAM_LDS>
int cr_set_lds(size_t bytes) {
  const auto kernel = continuum_kernel<LAM_LDS>;
  static std::atomic<size_t> granted[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
  if (dev >= 0 && granted[dev].load(std::memory_order_relaxed) >= bytes) return UMHS_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return UMHS_ERR_LAUNCH;
  if (dev >= 0) granted[dev].store(bytes, std::memory_order_relaxed);
  return UMHS_OK;
}

template <bool LAM_LDS>
int cr_launch(const float* spectra, int64_t stride, int64_t R, const float* wavelengths, int B, const CrRanges& rg, int F, float* removed,
              float* features, int* status, hipStream_t stream) {
  const size_t lds = cr_lds_bytes(B, LAM_LDS);
  if (lds > 48 * 1024) {
    const int rc = cr_set_lds<LAM_LDS>(lds);
    if (rc != UMHS_OK) return rc;
  }
  hipLaunchKernelGGL((continuum_kernel<LAM_LDS>), dim3((unsigned)((R + CR_ROWS - 1) / CR_ROWS)), dim3(CR_ROWS), lds, stream, spectra, stride, R,
                     wavelengths, B, rg, F, removed, features, status);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

}  // namespace

extern "C" size_t umhs_continuum_workspace_bytes(int64_t, int, int) { return 0; }  // rows, stacks and wavelengths live in LDS

extern "C" int umhs_continuum(const float* spectra, int64_t stride, int64_t n_rows, const float* wavelengths, int n_bands,
                              const int32_t* feature_ranges, int n_features, float* removed, float* features, int32_t* status, void*,
                              size_t, umhs_stream_t stream) {
  if (n_bands < 1 || n_bands > CR_MAX_B || n_features < 0 || n_features > CR_MAX_F || n_rows < 0 || stride < n_bands ||
      (n_features > 0 && !feature_ranges))
    return UMHS_ERR_ARG;
  CrRanges rg = {};
  rg.hi[0] = n_bands - 1;
  for (int f = 0; f < n_features; ++f) {
    const int lo = feature_ranges[2 * f], hi = feature_ranges[2 * f + 1];
    if (lo < 0 || hi >= n_bands || lo > hi || hi - lo + 1 < 3) return UMHS_ERR_ARG;
    rg.lo[1 + f] = lo, rg.hi[1 + f] = hi;
  }
  if (n_rows == 0) return UMHS_OK;
  if (!spectra || !wavelengths) return UMHS_ERR_ARG;
  if ((n_rows + CR_ROWS - 1) / CR_ROWS > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  if (!features) n_features = 0;  // (every output is optional)
  if (!removed && !status && n_features == 0) return UMHS_OK;  // nothing is asked for
  hipStream_t s = umhs_s(stream);
  return cr_lam_in_lds(n_bands) ? cr_launch<true>(spectra, stride, n_rows, wavelengths, n_bands, rg, n_features, removed, features, status, s)
                                : cr_launch<false>(spectra, stride, n_rows, wavelengths, n_bands, rg, n_features, removed, features, status, s);
}
