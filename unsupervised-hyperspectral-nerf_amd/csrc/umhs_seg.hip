// Material segmentation scored on the GPU: the confusion table of the labels the model emitted (seg_raw of umhs_ray_epilogue_fwd,
// umhs_tail.hip) against a ground-truth label image (``seg_file_path`` of transforms.json, the reference's seg_image).
//
//   row    p = accumulation > 0.5f ? (int)seg_raw : n_classes      the last row is "nothing rendered": seg_raw folds it into class 0
//   column k = labels[i]
//   counts[p * n_labels + k] += 1, unless k == ignore_label, k >= n_labels, or the pixel is rendered and seg_raw is not an integer
//   of [0, n_classes) (NaN, negative, too large, fractional): such a pixel never indexes the table.  A NaN accumulation is not > 0.5.
//
// Counts are integers: the table is exact and does not depend on the order of the adds.
//
// One persistent launch, grid-strided, at most SEG_MAX_BLOCKS workgroups (four per CU of a 256-CU part).  Every workgroup keeps the
// whole table -- at most 17 x 32 bins of 32 bits -- in LDS and hands its non-zero bins to the global int64 table once, at the end, with
// one 64-bit atomic per bin: there is no per-pixel global atomic (8,192 device-scope atomics on one cache line cost this project
// 100 us in the hash grid).  A workgroup step is SEG_STEP_PIXELS = 1,024 pixels, so a 256 x 256 frame runs as 64 workgroups of one step:
// measured on MI355X, 4.9-5.3 us (a single bin: 3.4-3.9) against 10.2-10.7 (6.4-7.0) for 16 workgroups of four steps with the loads of
// all four issued ahead -- at this size the kernel is bound by the latency of one workgroup, not by the flush (64 x 544 atomics in the
// worst case) nor by bandwidth (590 KB).
//
// A label image is a handful of flat regions, so the lanes of a wave mostly hold the same key.  Equal keys are combined in the wave
// before they reach LDS: the lowest lane still waiting is the leader, a ballot finds the lanes that hold the leader's key, and the
// leader adds their number.  SEG_PEEL such rounds serve a wave that straddles up to SEG_PEEL regions with one LDS add per key; lanes
// left after that (a noisy image: nearly every lane holds a key of its own, and a round per key would be 64 rounds) add 1 each.
//
// Loads: a lane takes four consecutive pixels per step -- one float4 of seg_raw, one of accumulation and four label bytes.  The quads
// are cut where BOTH float streams are 16-byte aligned (they are when the two pointers share their alignment, as two contiguous
// tensors do); the label bytes of a quad then start at any byte offset s of an
// aligned word and come from that word and, when s != 0, the next one, shifted together.  Both words hold a byte of the quad, and an
// aligned word never crosses a page, so neither load can fault.  The pixels in front of the first quad and behind the last, and every
// pixel when the float pointers do not share an alignment, go through the scalar loop.
#include "umhs_common.h"

#define SEG_THREADS 256
#define SEG_MAX_CLASSES 16
#define SEG_MAX_LABELS 32
#define SEG_BINS ((SEG_MAX_CLASSES + 1) * SEG_MAX_LABELS)
#define SEG_MAX_BLOCKS 1024
#define SEG_STEP_PIXELS (SEG_THREADS * 4)  // pixels of one workgroup step
#define SEG_PEEL 4
// a launch covers at most 2^40 pixels: 2^30 per workgroup at SEG_MAX_BLOCKS, so a 32-bit bin cannot wrap (the host loops beyond that)
#define SEG_LAUNCH_PIXELS (1LL << 40)

// bin of a pixel, or -1 for a pixel that is not scored
__device__ __forceinline__ int seg_key(float raw, float acc, uint32_t label, int n_classes, int n_labels, int ignore_label) {
  if ((int)label == ignore_label || (int)label >= n_labels) return -1;
  int p = n_classes;
  if (acc > 0.5f) {
    if (!(raw >= 0.0f && raw < (float)n_classes)) return -1;  // (NaN fails both comparisons)
    p = (int)raw;
    if ((float)p != raw) return -1;
  }
  return p * n_labels + (int)label;
}

// every lane of the wave that is active calls this together; key < 0: nothing to add
__device__ __forceinline__ void seg_add(uint32_t* bins, int key, int lane) {
  uint64_t todo = __ballot(key >= 0);
#pragma unroll 1
  for (int round = 0; todo != 0 && round < SEG_PEEL; ++round) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int k = __shfl(key, leader, 64);
    const uint64_t same = __ballot(key == k);  // (k >= 0, so lanes that sit out never match)
    if (lane == leader) atomicAdd(&bins[k], (uint32_t)__popcll((unsigned long long)same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1) atomicAdd(&bins[key], 1u);
}

// pixels [begin, end), one per lane and step; the trip count is the same for every lane of a workgroup
__device__ __forceinline__ void seg_scalar_range(const float* __restrict__ raw, const float* __restrict__ acc,
                                                 const uint8_t* __restrict__ labels, int64_t begin, int64_t end, int n_classes,
                                                 int n_labels, int ignore_label, uint32_t* bins, int lane) {
  for (int64_t base = begin + (int64_t)blockIdx.x * SEG_THREADS; base < end; base += (int64_t)gridDim.x * SEG_THREADS) {
    const int64_t i = base + threadIdx.x;
    int key = -1;
    if (i < end) key = seg_key(raw[i], acc[i], labels[i], n_classes, n_labels, ignore_label);
    seg_add(bins, key, lane);
  }
}

__global__ __launch_bounds__(SEG_THREADS) void seg_confusion_kernel(const float* __restrict__ raw, const float* __restrict__ acc,
                                                                    const uint8_t* __restrict__ labels, int64_t n, int n_classes,
                                                                    int n_labels, int ignore_label,
                                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[SEG_BINS];
  const int lane = threadIdx.x & 63, n_bins = (n_classes + 1) * n_labels;
  for (int b = threadIdx.x; b < n_bins; b += SEG_THREADS) bins[b] = 0u;
  __syncthreads();

  // head: the pixels in front of the first 16-byte boundary of the float streams; no quads when the two differ in alignment
  const int mis_raw = (int)(((uintptr_t)raw >> 2) & 3), mis_acc = (int)(((uintptr_t)acc >> 2) & 3);
  int64_t head = (4 - mis_raw) & 3, quads = 0;
  if (mis_raw != mis_acc) head = 0;
  else if (head > n) head = n;
  if (mis_raw == mis_acc) quads = (n - head) / 4;
  const int64_t tail = head + 4 * quads;

  seg_scalar_range(raw, acc, labels, 0, head, n_classes, n_labels, ignore_label, bins, lane);

  const float4* raw4 = reinterpret_cast<const float4*>(raw + head);
  const float4* acc4 = reinterpret_cast<const float4*>(acc + head);
  const uintptr_t lab0 = (uintptr_t)(labels + head);
  const uint32_t* lab4 = reinterpret_cast<const uint32_t*>(lab0 & ~(uintptr_t)3);
  const int shift = 8 * (int)(lab0 & 3);
  for (int64_t q0 = (int64_t)blockIdx.x * SEG_THREADS; q0 < quads; q0 += (int64_t)gridDim.x * SEG_THREADS) {  // same trips for every lane
    const int64_t q = q0 + threadIdx.x;
    int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
    if (q < quads) {
      const float4 r = raw4[q], a = acc4[q];
      const uint32_t w0 = lab4[q], w1 = shift ? lab4[q + 1] : 0u;
      const uint32_t l = (uint32_t)((((uint64_t)w1 << 32) | w0) >> shift);
      k0 = seg_key(r.x, a.x, l & 0xffu, n_classes, n_labels, ignore_label);
      k1 = seg_key(r.y, a.y, (l >> 8) & 0xffu, n_classes, n_labels, ignore_label);
      k2 = seg_key(r.z, a.z, (l >> 16) & 0xffu, n_classes, n_labels, ignore_label);
      k3 = seg_key(r.w, a.w, l >> 24, n_classes, n_labels, ignore_label);
    }
    seg_add(bins, k0, lane), seg_add(bins, k1, lane), seg_add(bins, k2, lane), seg_add(bins, k3, lane);
  }

  seg_scalar_range(raw, acc, labels, tail, n, n_classes, n_labels, ignore_label, bins, lane);

  __syncthreads();
  for (int b = threadIdx.x; b < n_bins; b += SEG_THREADS) {
    const uint32_t v = bins[b];
    if (v) atomicAdd(&counts[b], (unsigned long long)v);
  }
}

extern "C" int umhs_seg_confusion(const float* seg_raw, const float* accumulation, const uint8_t* labels, int64_t n_pixels,
                                  int n_classes, int n_labels, int ignore_label, int64_t* counts, umhs_stream_t stream) {
  if (!seg_raw || !accumulation || !labels || !counts || n_pixels < 0 || n_classes < 1 || n_labels < 1) return UMHS_ERR_ARG;
  if ((((uintptr_t)seg_raw | (uintptr_t)accumulation) & 3) || ((uintptr_t)counts & 7)) return UMHS_ERR_ARG;
  if (n_classes > SEG_MAX_CLASSES || n_labels > SEG_MAX_LABELS) return UMHS_ERR_UNSUPPORTED;
  for (int64_t first = 0; first < n_pixels; first += SEG_LAUNCH_PIXELS) {
    const int64_t n = n_pixels - first < SEG_LAUNCH_PIXELS ? n_pixels - first : SEG_LAUNCH_PIXELS;
    int64_t blocks = (n + SEG_STEP_PIXELS - 1) / SEG_STEP_PIXELS;
    if (blocks > SEG_MAX_BLOCKS) blocks = SEG_MAX_BLOCKS;
    hipLaunchKernelGGL(seg_confusion_kernel, dim3((unsigned)blocks), dim3(SEG_THREADS), 0, umhs_s(stream), seg_raw + first,
                       accumulation + first, labels + first, n, n_classes, n_labels, ignore_label,
                       reinterpret_cast<unsigned long long*>(counts));
    UMHS_CHECK_LAUNCH();
  }
  return UMHS_OK;
}
