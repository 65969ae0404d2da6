// What the host side of the field (umhs_field.hip) and the translation units of its transpose-free backward kernels
// (umhs_field_bwd_p0z.hip, umhs_field_bwd_p0f.hip, umhs_field_bwd_p1.hip) share: the slab layout, one kernel's launch description
// and the launchers those units define.  No kernel bodies.
#pragma once

#include <atomic>

#include "umhs_field_chain.h"

// accumulator / bias-sum slots of a wave (items of 64 lanes x 4 floats; the slab keeps this order).  Part 0 owns the accumulator
// items [0, A1) and the bias tiles [0, D1S); part 1 the rest.
template <int TBMAX>
struct TfSlots {
  static constexpr int A_H0 = 0, A_H1 = 8, A_H2 = 24, A_D0 = 28, A_D1 = 30, A_MX = 30 + TBMAX, A1 = 30 + 2 * TBMAX;
  static constexpr int A_F0 = A1, A_F1 = A1 + 8, A_F2 = A1 + 24, A_B0 = A1 + 28, A_B1 = A1 + 36, NACC = A1 + 40;
  static constexpr int D_H0 = 0, D_H1 = 4, D_H2 = 8, D_D0 = 9, D_D1 = 10, D1S = 4 * ((10 + TBMAX + 3) / 4);
  static constexpr int D_F0 = D1S, D_F1 = D1S + 4, D_F2 = D1S + 8, D_B0 = D1S + 9, D_B1 = D1S + 13, NDB = 4 * ((D1S + 14 + 3) / 4);
  static constexpr int NITEMS = NACC + NDB / 4;
  // part p's accumulator items [acc0(p), acc1(p)) and bias v4f items [dbv0(p), dbv1(p)) (absolute item = NACC + dbv)
  static constexpr int acc0(int p) { return p == 0 ? 0 : A1; }
  static constexpr int acc1(int p) { return p == 0 ? A1 : NACC; }
  static constexpr int dbv0(int p) { return p == 0 ? 0 : D1S / 4; }
  static constexpr int dbv1(int p) { return p == 0 ? D1S / 4 : NDB / 4; }
};
constexpr int TF_CHUNK = 32;  // items per round of the end-of-launch reduction over the 4 waves (4 x 32 x 1 KiB = 128 KiB of LDS)

// Raises a kernel's dynamic-LDS limit; remembered per kernel instantiation and device, so the driver call (which showed up as
// a ~6 us bubble in front of every launch it preceded) is made once, not on every step.
template <typename K>
static int set_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) return UMHS_ERR_UNSUPPORTED;
  static std::atomic<size_t> granted[16];  // per instantiation (a function-local static of a template) x device
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
  if (dev >= 0 && granted[dev].load(std::memory_order_relaxed) >= bytes) return UMHS_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
      hipSuccess)
    return UMHS_ERR_LAUNCH;
  if (dev >= 0) granted[dev].store(bytes, std::memory_order_relaxed);
  return UMHS_OK;
}

struct TfPart {  // one transpose-free kernel: descriptors rebased to its own LDS image + how to assemble that image
  PackDesc pd;
  TPackDesc td;
  ImgSegs seg_f, seg_t, seg_b;
  BfOffs bo;
  int wt_off, bf_off;
  size_t lds;
};

// ---- the two main kernels of the backward, per band-tile bound TBMAX; each launcher is defined (and its kernels are instantiated)
// in a translation unit of its own
// zipped: the three-piece bf16 chain = the kernels with the zipped instruction schedule (umhs_field_zip.h); else the fp32 chain
// (field_bwd_tf_kernel).  Measured (rocprofv3, C2) against the unzipped bf16x3 kernels they replaced: part 0 114.9 -> 110.9 us,
// part 1 114.5 -> 106.9 us; whole backward C3 604 -> 577 us, C5 457 -> 433 us.
struct TfLaunch {
  FieldIO io;
  const float *img, *wT, *bfimg;
  float* slabs;
  unsigned grid;
  umhs_stream_t stream;
};
template <int TBMAX>
int launch_tf_p0z(const TfPart& pt, const TfLaunch& a, bool spec, bool fused);  // zipped (three-piece bf16 chain)
template <int TBMAX>
int launch_tf_p0f(const TfPart& pt, const TfLaunch& a, bool spec, bool fused);  // fp32 chain
template <int TBMAX>
int launch_tf_p1(const TfPart& pt, const TfLaunch& a, bool zipped);
