// Frame composition for camera-path rendering: per-ray float outputs -> one displayable uint8 frame [height, n_panels * width, 3],
// the panels side by side (nerfstudio's render loop: apply_colormap per output, np.concatenate(axis=1), x255, cast).  One launch per
// frame; every source is read in place at (stride, channel) -- ``wv_7`` is ``spectral`` with stride B and channel 7, no column copy.
//
// Arithmetic (include/umhs_hip.h states it as THE definition): the result is integers, so every operation is one rounded float32
// operation and nothing may be contracted into an fma: the xf_* operations of umhs_exact.h (which says why the __f*_rn intrinsics of
// the HIP headers do not give that), and the whole unit is compiled with contraction off as well.
//
// Stores.  A pixel is three bytes and the frame starts at ANY byte address, so no pixel-per-lane store is aligned or wider than a
// byte; per byte, a dword store costs about six times and a short store twelve times a dwordx4 (MI355X store table).  The unit of
// work is therefore a WINDOW: `window` bytes (a multiple of 16, at most FRAME_WINDOW_BYTES) at a 16-byte ALIGNED address inside one
// panel's part of one frame row (3 * width bytes, a "segment").  The lanes compute the at most 252 pixels that touch the window, one
// each -- consecutive lanes read consecutive rows of the source --, drop their bytes into an LDS image of the window, and the image
// goes out as aligned dwordx4 stores, consecutive lanes to consecutive 16 bytes.  Only the first and the last 16-byte piece of a
// segment can be partial (its neighbour is another panel's segment): there the aligned dwords inside the segment are written as
// dwords and the up to three bytes on either side as bytes.  A pixel that straddles two windows is computed by both.
//
// A workgroup takes window xt of row r for ALL panels, one after the other, and stores them together.  Panels that are columns of one
// tensor (wv_0 .. wv_20 of `spectral`, 124-byte rows) then fetch the same cache lines back to back from the same CU; with one panel
// per workgroup every panel pulled the whole tensor through L2 again -- 1280 x 720 x 16 bands took 206 us that way (now 116), against
// 27 us for seven panels of 12- and 24-byte rows (now 35: a lane's panels are dependent load -> LDS chains, one after the other).  The grid is strided over height x windows-per-segment tiles, at most FRAME_MAX_BLOCKS
// workgroups; the windows of a segment are cut to equal size (256 pixels wide: two windows of 400 bytes, not 752 + 31).
//
// The panel descriptions arrive as kernel arguments (768 bytes) and are copied to LDS once per workgroup, because they are indexed
// by a loop counter.  The colour table (3 KB) is copied to LDS as well: a colormapped pixel gathers three floats of it, and with the
// table in global memory those three loads -- 64 lanes on up to 24 different cache lines each -- were three of the four
// vector-memory gathers per pixel.
#pragma clang fp contract(off)
#include "umhs_common.h"
#include "umhs_exact.h"

#define FRAME_THREADS 256
#define FRAME_WINDOW_BYTES 752  // 47 pieces of 16 bytes: at most 252 pixels touch a window, one per lane
#define FRAME_PAD 16            // bytes in front of a window's LDS image: a pixel may start up to 2 bytes before the window
#define FRAME_SLOT (FRAME_PAD + FRAME_WINDOW_BYTES + 16)  // LDS bytes per panel (a multiple of 16)
#define FRAME_MAX_PANELS 16
// four per CU of a 256-CU part.  Eight (every wave slot; a lane's panels are dependent load -> LDS chains) were measured: seven panels
// at 1280 x 720 went from 34 to 29 us, but 16 bands of `spectral` from 117 to 204 us -- with twice the rows in flight the 16 passes of
// a workgroup over its rows stop hitting in L2.
#define FRAME_MAX_BLOCKS 1024
#define FRAME_PANEL_WORDS (sizeof(umhs_frame_panel) / 4)

struct frame_panels {
  umhs_frame_panel p[FRAME_MAX_PANELS];
};

// clamp to [0, 1]; a NaN fails both comparisons and stays NaN
__device__ __forceinline__ float frame_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// q(c): (c * 255) + 0.5, clamped to [0, 255], truncated; NaN -> 0
__device__ __forceinline__ uint32_t frame_q(float c) {
  float t = xf_add(xf_mul(c, 255.0f), 0.5f);
  if (!(t > 0.0f)) t = 0.0f;  // (NaN lands here)
  if (t > 255.0f) t = 255.0f;
  return (uint32_t)(int)t;
}

// the three bytes of one pixel of one panel, packed r | g << 8 | b << 16; pix = row * width + x of the source
__device__ __forceinline__ uint32_t frame_pixel(const umhs_frame_panel& P, const float* lut /* LDS */, int64_t pix) {
  const float* s = P.src + pix * (int64_t)P.stride + P.channel;
  if (P.kind == UMHS_PANEL_RGB) return frame_q(s[0]) | (frame_q(s[1]) << 8) | (frame_q(s[2]) << 16);
  float v = s[0];
  if (P.kind == UMHS_PANEL_DEPTH) {
    const float lo = P.range[0], hi = P.range[1];
    v = frame_clamp01(xf_div(xf_sub(v, lo), xf_add(xf_sub(hi, lo), 1e-10f)));
  } else if (P.flags & 1) {
    const float lo = P.range[0], hi = P.range[1];
    v = xf_div(xf_sub(v, lo), xf_add(xf_sub(hi, lo), 1e-9f));
  }
  if (!(P.cmin == 0.0f && P.cmax == 1.0f)) v = xf_add(xf_mul(v, xf_sub(P.cmax, P.cmin)), P.cmin);
  v = frame_clamp01(v);
  if (P.flags & 2) v = xf_sub(1.0f, v);
  if (v != v) v = 0.0f;
  const int i = (int)xf_mul(v, 255.0f);  // v in [0, 1]: i in [0, 255]
  float c0 = lut[3 * i], c1 = lut[3 * i + 1], c2 = lut[3 * i + 2];
  if (P.kind == UMHS_PANEL_DEPTH && P.accumulation) {
    const float a = P.accumulation[pix], w = xf_sub(1.0f, a);
    c0 = xf_add(xf_mul(c0, a), w), c1 = xf_add(xf_mul(c1, a), w), c2 = xf_add(xf_mul(c2, a), w);
  }
  return frame_q(c0) | (frame_q(c1) << 8) | (frame_q(c2) << 16);
}

// segment (r, k) = frame bytes [3 * width * (r * n_panels + k), + 3 * width); its windows start at the 16-byte boundary at or below
// its first byte; n_xt windows of `window` bytes cover every segment at every alignment; n_tiles = height * n_xt
__global__ __launch_bounds__(FRAME_THREADS) void frame_compose_kernel(frame_panels args, int n_panels, const float* __restrict__ lut,
                                                                      int64_t width, uint8_t* __restrict__ frame, int window, int n_xt,
                                                                      int64_t n_tiles) {
  __shared__ umhs_frame_panel sp[FRAME_MAX_PANELS];
  __shared__ float slut[256 * 3];
  __shared__ __attribute__((aligned(16))) uint8_t image[FRAME_MAX_PANELS * FRAME_SLOT];
  {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(&args);
    uint32_t* d = reinterpret_cast<uint32_t*>(sp);
    for (int i = threadIdx.x; i < n_panels * (int)FRAME_PANEL_WORDS; i += FRAME_THREADS) d[i] = a[i];
    for (int i = threadIdx.x; i < 256 * 3; i += FRAME_THREADS) slut[i] = lut[i];
  }
  __syncthreads();
  const int64_t seg_bytes = 3 * width;
  const int pieces = window / 16;

  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {  // (the same trips for every lane of a workgroup: barriers inside)
    const int64_t r = t / n_xt;
    const int xt = (int)(t - r * n_xt);
    for (int k = 0; k < n_panels; ++k) {
      const int64_t seg0 = seg_bytes * (r * n_panels + k);                            // frame byte of the segment's first byte
      const int64_t w0 = (int64_t)xt * window - (int)((uintptr_t)(frame + seg0) & 15);  // segment byte at which the window starts
      const int64_t lo = w0 > 0 ? w0 : 0, hi = w0 + window < seg_bytes ? w0 + window : seg_bytes;
      if (lo >= hi) continue;                                                         // (the last window of a well-aligned segment)
      const int64_t p_lo = lo / 3;
      const int n_pix = (int)((hi + 2) / 3 - p_lo);                                   // <= 252
      if ((int)threadIdx.x < n_pix) {
        const int64_t x = p_lo + threadIdx.x;
        const uint32_t px = frame_pixel(sp[k], slut, r * width + x);
        uint8_t* o = image + k * FRAME_SLOT + FRAME_PAD + (int)(3 * x - w0);          // offset in [-2, window)
        o[0] = (uint8_t)px, o[1] = (uint8_t)(px >> 8), o[2] = (uint8_t)(px >> 16);
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n_panels * pieces; j += FRAME_THREADS) {
      const int k = j / pieces, c = j - k * pieces;
      const int64_t seg0 = seg_bytes * (r * n_panels + k);
      const int64_t s = (int64_t)xt * window - (int)((uintptr_t)(frame + seg0) & 15) + 16 * c;  // segment byte of this aligned piece
      const uint8_t* src = image + k * FRAME_SLOT + FRAME_PAD + 16 * c;
      uint8_t* dst = frame + seg0 + s;
      if (s >= 0 && s + 16 <= seg_bytes) {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
      } else if (s + 16 > 0 && s < seg_bytes) {  // the head or the tail of the segment (or both, in a narrow one)
        for (int w = 0; w < 4; ++w) {
          const int64_t sw = s + 4 * w;
          if (sw >= 0 && sw + 4 <= seg_bytes) {
            *reinterpret_cast<uint32_t*>(dst + 4 * w) = *reinterpret_cast<const uint32_t*>(src + 4 * w);
          } else {
            for (int b = 0; b < 4; ++b)
              if (sw + b >= 0 && sw + b < seg_bytes) dst[4 * w + b] = src[4 * w + b];
          }
        }
      }
    }
    __syncthreads();  // the images are rewritten by the next tile
  }
}

extern "C" int umhs_frame_compose(const umhs_frame_panel* panels, int n_panels, const float* lut, int height, int width,
                                  uint8_t* frame, umhs_stream_t stream) {
  if (!panels || !lut || !frame || n_panels < 1 || height < 0 || width < 0 || ((uintptr_t)lut & 3)) return UMHS_ERR_ARG;
  if (n_panels > FRAME_MAX_PANELS) return UMHS_ERR_UNSUPPORTED;
  frame_panels args;
  for (int k = 0; k < n_panels; ++k) {
    const umhs_frame_panel& P = panels[k];
    if (P.kind != UMHS_PANEL_RGB && P.kind != UMHS_PANEL_SCALAR && P.kind != UMHS_PANEL_DEPTH) return UMHS_ERR_ARG;
    if (!P.src || ((uintptr_t)P.src & 3) || P.channel < 0 || P.stride < P.channel + (P.kind == UMHS_PANEL_RGB ? 3 : 1)) return UMHS_ERR_ARG;
    const bool needs_range = P.kind == UMHS_PANEL_DEPTH || (P.kind == UMHS_PANEL_SCALAR && (P.flags & 1));
    if ((needs_range && !P.range) || ((uintptr_t)P.range & 3) || ((uintptr_t)P.accumulation & 3)) return UMHS_ERR_ARG;
    args.p[k] = P;
  }
  for (int k = n_panels; k < FRAME_MAX_PANELS; ++k) args.p[k] = umhs_frame_panel{};
  if ((int64_t)n_panels * width >= (1LL << 31)) return UMHS_ERR_UNSUPPORTED;
  if (height == 0 || width == 0) return UMHS_OK;
  // windows of equal size: as few as cover a segment at its worst alignment (15 bytes in front of it), then as small as that allows
  const int64_t seg_pieces = (3 * (int64_t)width + 15 + 15) / 16;
  const int64_t n_xt = (seg_pieces + FRAME_WINDOW_BYTES / 16 - 1) / (FRAME_WINDOW_BYTES / 16);
  const int window = 16 * (int)((seg_pieces + n_xt - 1) / n_xt);
  const int64_t n_tiles = height * n_xt;
  const int64_t blocks = n_tiles < FRAME_MAX_BLOCKS ? n_tiles : FRAME_MAX_BLOCKS;
  hipLaunchKernelGGL(frame_compose_kernel, dim3((unsigned)blocks), dim3(FRAME_THREADS), 0, umhs_s(stream), args, n_panels, lut,
                     (int64_t)width, frame, window, (int)n_xt, n_tiles);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
