// Exact float32 arithmetic for the kernels whose results are bytes, rows of a file or decisions (frame composition, point-cloud and
// mesh export): include/umhs_hip.h states their arithmetic as THE definition, every step one rounded float32 operation, and nothing
// may be contracted into an fma.
//
// The __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn of the HIP headers do not guarantee that: their bodies are plain ``x * y`` /
// ``x + y`` compiled under the command line's contraction mode, and once inlined hipcc did fuse the sum of frame_q() with its product
// into one v_fma_f32 when umhs_frame.hip was written with them.  The xf_* functions below are the same operations, each compiled
// with contraction off by a pragma of its own (it governs the function's body wherever that is inlined), and the units that use them
// are compiled that way as a whole as well (a file-scope pragma in each: this header does not replace it).  The disassembly of their
// kernels holds no fma outside the expansions of the (correctly rounded) float division and of the integer divisions.
#pragma once
#include "umhs_common.h"

// one rounded float32 operation each, never contracted with a neighbour
__device__ __forceinline__ float xf_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float xf_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float xf_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float xf_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}
// (sqrtf is correctly rounded under the build's flags, as the division is; like the division, its expansion holds fmas of its own,
// which are not contractions)
__device__ __forceinline__ float xf_sqrt(float a) {
#pragma clang fp contract(off)
  return sqrtf(a);
}

// (uint8)(clamp(v, 0, 1) * 255.0f), truncated; NaN -> 0: the colour and alpha bytes of the exported rows
__device__ __forceinline__ uint32_t xf_byte(float v) {
  if (!(v > 0.0f)) return 0u;  // (NaN lands here)
  if (v > 1.0f) v = 1.0f;
  return (uint32_t)(int)xf_mul(v, 255.0f);
}

// neither an infinity nor a NaN
__host__ __device__ __forceinline__ bool xf_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }
