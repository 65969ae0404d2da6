// Spectral unmixing (include/umhs_hip.h, "Spectral unmixing"): per row the abundances a >= 0 (FCLS: sum a = 1) that minimise
// |x - E^T a|^2 against K <= 16 endmembers, by an active-set solve of the normal equations (G, b = E x).  One launch, two phases.
//
//   block      ONE wave and its 64 rows; nothing is shared between waves, so there is no block-wide state to wait for and the LDS a
//              wave needs (below) decides how many of them a CU holds: 3 at K = 16.
//   products   the rows and the MFMA of the library match (umhs_library_tile.h: lib_load_rows, v_mfma_f32_32x32x2_f32 whose k order is
//              the band order), on the one 32-entry tile an endmember set is.  The image's k-steps are read straight from global
//              memory (a coalesced run of 64 dwords each, read once per wave: there is no second wave to share an LDS copy with).
//              b[r,k] is the fmaf chain over b ascending; ss = (the chain of the even bands' x_b^2) + (that of the odd ones).  In the accumulator
//              layout row 32 t + j has its entries on lanes (j, 0) and (j, 1): both store their part to the row's LDS column.
//   solve      lane l solves row l.  The active set differs per lane, so the pivot index is lane-dynamic: the tableau -- the packed
//              lower triangle of the swept G (K (K + 1) / 2 floats) and the two right-hand columns b and ones (2 K) -- lives in LDS,
//              lane-minor: element e of lane l at sT[e * 64 + l].  A ds_read_b32 / ds_write_b32 of one element is then conflict-free
//              (bank = lane mod 32; the two 32-lane halves do not conflict) whatever e each lane asks for.  Only the pivot's column is
//              addressed dynamically (K reads into registers c[0..K), K writes); the K (K + 1) / 2 + 2 K updates run over static
//              (i, j) with immediate offsets -- they also touch row k, which the K writes then overwrite.  a, z and the columns of
//              a solve are registers in fully unrolled loops over a static k, guarded by k < K: no dynamic register index, no scratch.
//   loop       one sweep or one solve per trip, so the lanes of a wave stay together as far as their active sets allow; every trip
//              either shrinks `pending` or counts a solve, and the solves are capped: a row cannot hang.
#include "umhs_library_tile.h"

namespace {

constexpr int UNMIX_MAX_K = UMHS_UNMIX_MAX_ENDMEMBERS;
constexpr float UNMIX_FLT_MAX = 3.402823466e38f;
constexpr float UNMIX_TOL = 4.76837158203125e-07f;  // 2^-21, relative to max |b|

__host__ __device__ inline int unmix_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
// the triangle takes the place of the image (NK k-steps, zeros past the image's own) once the products are formed
__host__ __device__ inline int unmix_lds_floats(int K, int NK) {
  const int KK = K * (K + 1) / 2;
  return (2 * K + (KK > NK ? KK : NK)) * 64;
}

// b of the wave's 64 rows into their LDS columns sB[k * 64 + row], T row tiles at a time; -> the ss of row `lane`
template <int NK, int T>
__device__ __forceinline__ float unmix_products(const float* __restrict__ spectra, int64_t stride, int64_t R, int B, int K,
                                                const float* __restrict__ image, int64_t row0, int lane, float* sA, float* sB) {
  const int j = lane & 31, h = lane >> 5, ks = lib_ksteps(B);
  for (int s = 0; s < NK; ++s) sA[s * 64 + lane] = s < ks ? image[s * 64 + lane] : 0.0f;  // the one tile of the image: [k-step][lane]
  __syncthreads();
  float mine = 0.0f;
#pragma unroll 1  // (T == 1: the second tile's rows must not be loaded beside the first's -- they are T == 1 because they do not fit)
  for (int g = 0; g < 2 / T; ++g) {
    float x[T][NK];
    int first = 32 * T * g;
    asm volatile("" : "+s"(first));  // (opaque: else every load's address becomes an induction variable of this loop, two registers each)
    lib_load_rows<NK, T, false>(spectra, stride, R, B, row0 + first, j, h, nullptr, x);
    v16f acc[T];
    float ss[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      float own = 0.0f;  // the chain of this lane's bands (the even ones on h = 0, the odd ones on h = 1), ascending
#pragma unroll
      for (int s = 0; s < NK; ++s) own = fmaf(x[t][s], x[t][s], own);
      const float other = __shfl_xor(own, 32, 64);
      ss[t] = h ? other + own : own + other;  // even + odd, the same bits on both lanes
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
    }
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      const float a = sA[s * 64 + lane];  // (an immediate offset; the steps past ks hold zeros)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[t][s], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (h == T * g + t) mine = ss[t];  // (both lanes of a row hold it; row 32 tile + j is solved by lane 32 tile + j)
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // (entries 16..31 of the tile are padding)
        const int k = lib_acc_row(e, h);
        if (k < K) sB[k * 64 + 32 * (T * g + t) + j] = acc[t][e];
      }
  }
  return mine;
}

template <int NK, int T>
__global__ __launch_bounds__(64, 2) void unmix_kernel(const float* __restrict__ spectra, int64_t stride, int64_t R,
                                                   const float* __restrict__ image, const float* __restrict__ gram, int K, int B,
                                                   int mode, float* __restrict__ abundances, float* __restrict__ residual,
                                                   int* __restrict__ status) {
  extern __shared__ float sT[];  // [element][lane]: column b, column ones, then the packed triangle -- and under it, first, the image
  const int lane = threadIdx.x;
  float* sCb = sT + lane;
  float* sC1 = sCb + K * 64;
  float* sM = sC1 + K * 64;
  const int64_t row0 = (int64_t)blockIdx.x * 64, r = row0 + lane;

  const float ss = unmix_products<NK, T>(spectra, stride, R, B, K, image, row0, lane, sT + 2 * K * 64, sT);
  __syncthreads();  // (one wave: a row's two MFMA lanes wrote the column its solver lane reads; the image is dead, the triangle takes its place)
  if (r >= R) return;
  const bool valid = ss > 0.0f && ss <= UNMIX_FLT_MAX;  // not 0, not NaN, not Inf

  float bq[UNMIX_MAX_K], a[UNMIX_MAX_K];
  float bmax = 0.0f;
#pragma unroll
  for (int k = 0; k < UNMIX_MAX_K; ++k) {
    bq[k] = (valid && k < K) ? sCb[k * 64] : 0.0f;
    bmax = fmaxf(bmax, fabsf(bq[k]));
    a[k] = (mode == UMHS_UNMIX_FCLS && k < K) ? 1.0f / (float)K : 0.0f;
  }
  int solves = 0, state = -1;
  if (valid) {
#pragma unroll
    for (int i = 0; i < UNMIX_MAX_K; ++i)
      if (i < K) {  // (a guard, not a break: a loop with a run-time exit is not unrolled, and its arrays would go to scratch)
#pragma unroll
        for (int j = 0; j <= i; ++j) sM[(i * (i + 1) / 2 + j) * 64] = gram[i * K + j];
        sC1[i * 64] = 1.0f;
      }
    const float tol = UNMIX_TOL * bmax;
    const int cap = 3 * K + 3;
    unsigned P = 0, banned = 0, pending = (1u << K) - 1u;
    int entering = -1;
    for (;;) {
      if (pending) {  // one sweep: k enters P, or leaves it
        const int k = __ffs(pending) - 1;
        pending &= pending - 1;
        const bool leaving = (P >> k) & 1u;
        const float p = sM[unmix_tri(k, k) * 64];
        if (!leaving && !(p > 0.0f)) {
          banned |= 1u << k;
        } else {
          const float rp = 1.0f / p;
          float c[UNMIX_MAX_K];
#pragma unroll
          for (int i = 0; i < UNMIX_MAX_K; ++i) c[i] = i < K ? sM[unmix_tri(i, k) * 64] : 0.0f;
          const float bk = sCb[k * 64], ok = sC1[k * 64];
#pragma unroll
          for (int i = 0; i < UNMIX_MAX_K; ++i)
            if (i < K) {
              const float t = -(c[i] * rp);
#pragma unroll
              for (int j = 0; j <= i; ++j) {
                float* m = sM + (i * (i + 1) / 2 + j) * 64;
                *m = fmaf(t, c[j], *m);
              }
              sCb[i * 64] = fmaf(t, bk, sCb[i * 64]);
              sC1[i * 64] = fmaf(t, ok, sC1[i * 64]);
            }
          const float rs = leaving ? -rp : rp;
#pragma unroll
          for (int i = 0; i < UNMIX_MAX_K; ++i)
            if (i < K) sM[unmix_tri(i, k) * 64] = c[i] * rs;
          sM[unmix_tri(k, k) * 64] = -rp;
          sCb[k * 64] = bk * rs;
          sC1[k * 64] = ok * rs;
          P ^= 1u << k;
        }
        if (pending) continue;
      }
      if (solves >= cap) {
        state = -2;
        break;
      }
      ++solves;
      float cb[UNMIX_MAX_K], c1[UNMIX_MAX_K], z[UNMIX_MAX_K];
#pragma unroll
      for (int i = 0; i < UNMIX_MAX_K; ++i) {
        cb[i] = i < K ? sCb[i * 64] : 0.0f;
        c1[i] = i < K ? sC1[i * 64] : 0.0f;
      }
      float lam = 0.0f;
      if (mode == UMHS_UNMIX_FCLS) {
        float su = 0.0f, sv = 0.0f;
#pragma unroll
        for (int i = 0; i < UNMIX_MAX_K; ++i)
          if ((P >> i) & 1u) su += cb[i], sv += c1[i];
        lam = (su - 1.0f) / sv;
      }
      unsigned neg = 0;
#pragma unroll
      for (int i = 0; i < UNMIX_MAX_K; ++i) {
        const bool in = (P >> i) & 1u;
        z[i] = in ? fmaf(-lam, c1[i], cb[i]) : 0.0f;
        if (in && !(z[i] > 0.0f)) neg |= 1u << i;
      }
      if (entering >= 0) {
        const unsigned bit = 1u << entering;
        entering = -1;
        if (P & neg & bit) {  // it entered and is not positive: out again, and banned until another one stays
          pending = bit;
          banned |= bit;
          continue;
        }
        if (P & bit) banned = 0;
      }
      if (neg) {  // a step toward z, up to the first bound
        float best = 2.0f;
        int imin = 0;
#pragma unroll
        for (int i = 0; i < UNMIX_MAX_K; ++i)
          if ((neg >> i) & 1u) {
            const float den = a[i] - z[i];
            const float ratio = den > 0.0f ? a[i] / den : 0.0f;
            if (ratio < best) best = ratio, imin = i;
          }
        const float alpha = fminf(best, 1.0f);
        unsigned drop = 0;
#pragma unroll
        for (int i = 0; i < UNMIX_MAX_K; ++i) {
          a[i] = ((P >> i) & 1u) ? fmaxf(fmaf(alpha, z[i] - a[i], a[i]), 0.0f) : 0.0f;
          if (i == imin) a[i] = 0.0f;
          if (((neg >> i) & 1u) && a[i] <= 0.0f) drop |= 1u << i;
        }
        pending = drop;
        continue;
      }
      float wbest = -INFINITY;
      int t = 0;
#pragma unroll
      for (int i = 0; i < UNMIX_MAX_K; ++i) {
        a[i] = z[i];
        if (i < K && !(((P | banned) >> i) & 1u)) {
          const float w = fmaf(-lam, c1[i], cb[i]);
          if (w > wbest) wbest = w, t = i;
        }
      }
      if (!(wbest > tol)) {
        state = solves;
        break;
      }
      pending = 1u << t;
      entering = t;
    }
  }

  float ba = 0.0f, aga = 0.0f;
#pragma unroll
  for (int k = 0; k < UNMIX_MAX_K; ++k) {
    a[k] = (valid && a[k] > 0.0f && a[k] <= UNMIX_FLT_MAX) ? a[k] : 0.0f;  // finite and >= +0, whatever happened above
    if (k < K) abundances[r * K + k] = a[k];
  }
  if (residual) {
#pragma unroll
    for (int i = 0; i < UNMIX_MAX_K; ++i)
      if (i < K) {
        float ga = 0.0f;
#pragma unroll
        for (int j = 0; j < UNMIX_MAX_K; ++j)
          if (j < K) ga = fmaf(gram[i * K + j], a[j], ga);
        ba = fmaf(bq[i], a[i], ba);
        aga = fmaf(a[i], ga, aga);
      }
    residual[r] = valid ? fmaxf(0.0f, fmaf(-2.0f, ba, ss) + aga) : 0.0f;
  }
  if (status) status[r] = state;
}

template <int NK, int T>
void unmix_launch(const float* spectra, int64_t stride, int64_t R, const float* image, const float* gram, int K, int B, int mode,
                  float* abundances, float* residual, int* status, hipStream_t stream) {
  hipLaunchKernelGGL((unmix_kernel<NK, T>), dim3((unsigned)((R + 63) / 64)), dim3(64), unmix_lds_floats(K, NK) * sizeof(float), stream, spectra,
                     stride, R, image, gram, K, B, mode, abundances, residual, status);
}

}  // namespace

extern "C" size_t umhs_unmix_workspace_bytes(int64_t, int, int) { return 0; }  // the tableau lives in LDS

extern "C" int umhs_unmix(const float* spectra, int64_t stride, int64_t n_rows, const float* image, const float* gram, int n_endmembers,
                          int n_bands, int mode, float* abundances, float* residual, int32_t* status, void*, size_t,
                          umhs_stream_t stream) {
  if (n_bands < 1 || n_endmembers < 1 || n_rows < 0 || stride < n_bands || (mode != UMHS_UNMIX_NNLS && mode != UMHS_UNMIX_FCLS))
    return UMHS_ERR_ARG;
  if (n_bands > LIB_MAX_BANDS || n_endmembers > UNMIX_MAX_K) return UMHS_ERR_UNSUPPORTED;
  if (n_rows == 0) return UMHS_OK;
  if (!spectra || !image || !gram || !abundances) return UMHS_ERR_ARG;
  if ((n_rows + 63) / 64 > 0x7fffffff) return UMHS_ERR_UNSUPPORTED;
  const int ks = lib_ksteps(n_bands);
  hipStream_t s = umhs_s(stream);
#define UNMIX_CASE(NK, T) \
  unmix_launch<NK, T>(spectra, stride, n_rows, image, gram, n_endmembers, n_bands, mode, abundances, residual, status, s);
  LIB_DISPATCH(ks, UNMIX_CASE, return UMHS_ERR_UNSUPPORTED;)
#undef UNMIX_CASE
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
