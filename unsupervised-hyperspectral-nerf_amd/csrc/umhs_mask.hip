// Per-frame masks (``mask_path`` of transforms.json) for the pixel sampler: nerfstudio's mask-aware PixelSampler draws training pixels
// only where the mask is non-zero -- it takes nonzero(mask) over the whole [n,H,W] stack and picks rows of it  [upstream-recalled].
// Here the set pixels of a uint8 mask stack are compacted ONCE, at load, into
//   off  [n+1] int64: exclusive prefix sum of the per-image counts of non-zero pixels, M = off[n]
//   list [M]   int32: the flat ids y*W + x of the set pixels, ascending within an image, images in order
//                     (the second column of torch.nonzero(mask.view(n, -1))),
// and umhs_pixel_indices_masked turns the same torch.rand((R,3)) block the unmasked sampler draws into rows (image, y, x) that are
// uniform over those M pixels, with replacement (tests/mask_ref.py restates it; every product is ONE float32 multiplication).
//
// Compaction is two launches around a scan of per-chunk counts (the scan is the caller's: a few thousand integers, once per split):
// mask_count_kernel counts the set pixels of every chunk, mask_compact_kernel recomputes the count per thread, ranks the threads of a
// chunk by an exclusive scan (wave shuffles, then the four wave totals through LDS) and writes each thread's ids in ascending order at
// chunk_offsets[chunk] + rank.  No atomics: where an id lands is a function of the mask alone.
//
// A chunk is 256 threads x one 16-byte ALIGNED granule of one image.  An image's first byte (mask + i*H*W) is not 16-byte aligned when
// H*W is odd, so the granules are those of the address space, not of the image: granule q of image i starts at ((base_i >> 4) + q) << 4
// and its byte b is pixel 16 q + b - (base_i & 15) when that lies in [0, H*W).  The first and last granule of an image can thus reach up
// to 15 bytes outside it; those bytes are loaded and dropped.  An aligned 16-byte load never crosses a page and the granule holds at
// least one byte of the image, so the load cannot fault.  Both kernels are one pass over the mask at 16 B per lane.
#include "umhs_common.h"

#define MASK_THREADS 256
#define MASK_CHUNK_BYTES (MASK_THREADS * 16)
#define MASK_MAX_PIXELS (1LL << 24)  // ids are int32 and ranks come from one float32 uniform: 24 bits

// chunks per image for H*W pixels: the granules of an image whose first byte sits at offset 15 of its granule
static inline int64_t mask_chunks(int64_t pixels) { return ((pixels + 15 + 15) / 16 + MASK_THREADS - 1) / MASK_THREADS; }

// the 16 bytes of this thread's granule as 0 / 1 flags in bits 0..15, bytes outside the image dropped; pix0 = pixel id of byte 0
// (negative in an image's first granule when the image does not start on a 16-byte boundary)
__device__ __forceinline__ uint32_t mask_granule_bits(const uint8_t* __restrict__ mask, int64_t pixels, int64_t chunks_per_image,
                                                      int64_t& pix0) {
  const int64_t image = blockIdx.x / chunks_per_image, chunk = blockIdx.x - image * chunks_per_image;
  const uintptr_t base = (uintptr_t)(mask + image * pixels);
  const int64_t mis = (int64_t)(base & 15), q = chunk * MASK_THREADS + threadIdx.x;
  pix0 = q * 16 - mis;
  if (pix0 >= pixels) return 0u;  // (pix0 + 15 >= 0 always: mis <= 15)
  const uint4 v = *reinterpret_cast<const uint4*>((base & ~(uintptr_t)15) + (uintptr_t)q * 16);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t bits = 0;
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const int64_t p = pix0 + b;
    if (((w[b >> 2] >> (8 * (b & 3))) & 0xffu) != 0u && p >= 0 && p < pixels) bits |= 1u << b;
  }
  return bits;
}

__global__ __launch_bounds__(MASK_THREADS) void mask_count_kernel(const uint8_t* __restrict__ mask, int64_t pixels,
                                                                  int64_t chunks_per_image, int32_t* __restrict__ chunk_counts) {
  __shared__ int wave_total[MASK_THREADS / UMHS_WAVE];
  int64_t pix0;
  int c = __popc(mask_granule_bits(mask, pixels, chunks_per_image, pix0));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) chunk_counts[blockIdx.x] = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
}

__global__ __launch_bounds__(MASK_THREADS) void mask_compact_kernel(const uint8_t* __restrict__ mask, int64_t pixels,
                                                                    int64_t chunks_per_image,
                                                                    const int64_t* __restrict__ chunk_offsets,
                                                                    int32_t* __restrict__ list, int64_t list_len) {
  __shared__ int wave_total[MASK_THREADS / UMHS_WAVE];
  int64_t pix0;
  uint32_t bits = mask_granule_bits(mask, pixels, chunks_per_image, pix0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = __popc(bits);
  int incl = c;  // inclusive scan over the wave: lanes hold consecutive granules, so lane order is pixel order
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  int before = incl - c;
#pragma unroll
  for (int k = 0; k < MASK_THREADS / UMHS_WAVE - 1; ++k) before += (k < wave) ? wave_total[k] : 0;
  int64_t at = chunk_offsets[blockIdx.x] + before;
  while (bits) {  // lowest set bit first: ascending ids
    const int b = __ffs(bits) - 1;
    bits &= bits - 1;
    if (at >= 0 && at < list_len) list[at] = (int32_t)(pix0 + b);  // offsets that do not fit the mask never write outside the list
    ++at;
  }
}

extern "C" int64_t umhs_mask_chunks(int64_t pixels_per_image) { return pixels_per_image < 1 ? 0 : mask_chunks(pixels_per_image); }

static int mask_args(const void* mask, int64_t n_images, int64_t pixels, const void* a, const void* b) {
  if (n_images < 0 || pixels < 1 || !mask || !a || !b) return UMHS_ERR_ARG;
  if (pixels > MASK_MAX_PIXELS || n_images * mask_chunks(pixels) > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;
  return UMHS_OK;
}

extern "C" int umhs_mask_count(const uint8_t* mask, int64_t n_images, int64_t pixels_per_image, int32_t* chunk_counts,
                               umhs_stream_t stream) {
  if (n_images == 0) return UMHS_OK;
  const int rc = mask_args(mask, n_images, pixels_per_image, chunk_counts, chunk_counts);
  if (rc != UMHS_OK) return rc;
  const int64_t cpi = mask_chunks(pixels_per_image);
  hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)(n_images * cpi)), dim3(MASK_THREADS), 0, umhs_s(stream), mask,
                     pixels_per_image, cpi, chunk_counts);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_mask_compact(const uint8_t* mask, int64_t n_images, int64_t pixels_per_image, const int64_t* chunk_offsets,
                                 int32_t* list, int64_t list_len, umhs_stream_t stream) {
  if (n_images == 0) return UMHS_OK;
  if (list_len < 0) return UMHS_ERR_ARG;
  const int rc = mask_args(mask, n_images, pixels_per_image, chunk_offsets, list);
  if (rc != UMHS_OK) return rc;
  const int64_t cpi = mask_chunks(pixels_per_image);
  hipLaunchKernelGGL(mask_compact_kernel, dim3((unsigned)(n_images * cpi)), dim3(MASK_THREADS), 0, umhs_s(stream), mask,
                     pixels_per_image, cpi, chunk_offsets, list, list_len);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// One thread per ray: a dependent chain of ~log2(n) + 3 loads, against R of a few thousand.
//   t = min((int64)(u0 * (float)M), M - 1);  image i: off[i] <= t < off[i+1] (an image with an empty mask is never chosen);
//   k = min((int64)(u1 * (float)cnt_i), cnt_i - 1);  p = list[off[i] + k];  row = (i, p / W, p % W).
// Rank and image come from separate uniforms: one float32 has 24 bits and a stack has more pixels than that.
__global__ __launch_bounds__(256) void pixel_indices_masked_kernel(const float* __restrict__ u, int64_t n_rays, int64_t n_images,
                                                                   int64_t width, const int64_t* __restrict__ off,
                                                                   const int32_t* __restrict__ list,
                                                                   int64_t* __restrict__ indices) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  const int64_t M = off[n_images];
  int64_t i = 0, p = 0;
  if (M > 0) {  // (an all-zero stack is refused when the split is built; never read the empty list)
    int64_t t = (int64_t)(u[3 * r] * (float)M);
    t = t < 0 ? 0 : (t > M - 1 ? M - 1 : t);
    int64_t lo = 0, hi = n_images;  // off[lo] <= t < off[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= t) lo = mid; else hi = mid;
    }
    const int64_t first = off[lo], cnt = off[lo + 1] - first;
    int64_t k = (int64_t)(u[3 * r + 1] * (float)cnt);
    k = k < 0 ? 0 : (k > cnt - 1 ? cnt - 1 : k);
    i = lo, p = list[first + k];
  }
  indices[3 * r] = i, indices[3 * r + 1] = p / width, indices[3 * r + 2] = p % width;
}

extern "C" int umhs_pixel_indices_masked(const float* uniform, int64_t n_rays, int64_t n_images, int64_t width, const int64_t* off,
                                         const int32_t* list, int64_t* indices, umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_images < 1 || width < 1 || !uniform || !off || !list || !indices) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(pixel_indices_masked_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), uniform, n_rays,
                     n_images, width, off, list, indices);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
