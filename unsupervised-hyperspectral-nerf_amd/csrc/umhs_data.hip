// pixel sampler / ray generator / ground-truth gather for gfx950.
// Replaces what UMHSDataManager.next_train (umhs_datamanager.py:95-108) reaches in nerfstudio==1.1.5 with
// --images-on-gpu: PixelSampler.sample (indices (camera, y, x) -> rows of the cached image stacks) and RayGenerator ->
// Cameras.generate_rays (perspective; raygen_kernel without lens distortion, raygen_distorted_kernel with the OpenCV radial /
// tangential model that COLMAP's OPENCV cameras carry).  nerfstudio's source is not available offline; the arithmetic below
// restates its published behaviour (oracle/torch_ref.py generate_rays / gather_pixels; the undistortion is
// camera_utils.radial_and_tangential_undistort  [upstream-recalled]: undistort_opencv in umhs_camera.h, which also holds the forward
// model and the box / camera rotation the exporters share; restated in tests/raygen_f64.py).  All kernels are HBM-bound:
// ray generation moves 24 B in + 28 B out per ray (the distorted one adds ~2 k flops of Newton steps per ray, still far below the
// roofline's ridge), the gather one (B+3)-float row per ray from a stack of n*H*W rows.  raygen_frame_kernel makes the rays of a whole
// frame (perspective, fisheye, equirectangular; optional crop box -> per-ray nears / fars) from the thread index alone: no index tensor.
#include "umhs_common.h"
#include "umhs_camera.h"

// ---- the arithmetic every ray generator below shares (one body each: the frame kernel's perspective rays carry the bits of the
// sampled-pixel kernels because they run these very functions) ----------------------------------------------------------------------
// the three image-plane points of a ray, y DOWN: the pixel centre (x, y), its +x and its +y neighbour (pixel_area = |d - dx| * |d - dy|)
__device__ __forceinline__ void rg_plane_points(float x, float y, float fx, float fy, float cx, float cy, float px[3], float py[3]) {
#pragma clang fp contract(off)
  px[0] = (x - cx) / fx, px[1] = (x - cx + 1.0f) / fx, px[2] = (x - cx) / fx;
  py[0] = (y - cy) / fy, py[1] = (y - cy) / fy, py[2] = (y - cy + 1.0f) / fy;
}

// camera-frame directions cam[s] of the three points -> unit world directions d[s] through the pose's 3x3 block; returns the norm of
// the centre direction, floored at float32 eps
__device__ __forceinline__ float rg_world_directions(const float cam[3][3], const float* __restrict__ M, float d[3][3]) {
#pragma clang fp contract(off)
  float nrm0 = 0.0f;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    float v[3], sq = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = (cam[s][0] * M[4 * k] + cam[s][1] * M[4 * k + 1]) + cam[s][2] * M[4 * k + 2];
      // the squares are accumulated as torch.linalg.vector_norm accumulates them on the CPU the oracle runs on -- v0 * v0, then one
      // fused multiply-add per further component -- so that directions and directions_norm carry the oracle's bits (the plain
      // float32 sum was one unit in the last place off in ~11 % of the components)
      sq = k == 0 ? v[k] * v[k] : fmaf(v[k], v[k], sq);
    }
    const float nrm = fmaxf(sqrtf(sq), 1.1920928955078125e-07f);
    if (s == 0) nrm0 = nrm;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[s][k] = v[k] / nrm;
  }
  return nrm0;
}

__device__ __forceinline__ float rg_pixel_area(const float d[3][3]) {
#pragma clang fp contract(off)
  float dx = 0.0f, dy = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = d[0][k] - d[1][k], b = d[0][k] - d[2][k];
    dx += a * a, dy += b * b;
  }
  return sqrtf(dx) * sqrtf(dy);
}

// The body of the two sampled-pixel kernels.  indices [R,3] int64 (camera, y, x); c2w [n,3,4]; intr [n,4] = (fx, fy, cx, cy).  DIST:
// dist [n,6] = (k1, k2, k3, k4, p1, p2) per camera; the pixel, its +x and its +y neighbour are each undistorted in OpenCV image-plane
// coordinates ((x-cx)/fx, (y-cy)/fy), y down (umhs_camera.h), and y is negated afterwards (camera y is up).  Everything else is the
// same statements, so a camera whose six parameters are all zero gives the bits of the kernel without distortion.
template <bool DIST>
__device__ __forceinline__ void raygen_body(const int64_t* __restrict__ indices, const float* __restrict__ c2w,
                                            const float* __restrict__ intr, const float* __restrict__ dist, int64_t n_rays,
                                            int64_t n_cams, float* __restrict__ origins, float* __restrict__ directions,
                                            float* __restrict__ pixel_area, float* __restrict__ dir_norm) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  int64_t c = indices[3 * r];
  c = c < 0 ? 0 : (c >= n_cams ? n_cams - 1 : c);  // indices are validated on the host; never read out of bounds
  const float y = (float)indices[3 * r + 1] + 0.5f, x = (float)indices[3 * r + 2] + 0.5f;  // pixel centres
  const float fx = intr[4 * c], fy = intr[4 * c + 1], cx = intr[4 * c + 2], cy = intr[4 * c + 3];
  const float* M = c2w + 12 * c;
  // the camera looks down -z and its y is up: (u, v, -1) with v the negated y-down coordinate
  float px[3], py[3], cam[3][3], d[3][3];
  rg_plane_points(x, y, fx, fy, cx, cy, px, py);
  if constexpr (DIST) undistort_plane_points(dist, c, px, py);
#pragma unroll
  for (int s = 0; s < 3; ++s) cam[s][0] = px[s], cam[s][1] = -py[s], cam[s][2] = -1.0f;
  const float nrm0 = rg_world_directions(cam, M, d);  // (torch.linalg.vector_norm's order and roundings: see there)
#pragma unroll
  for (int k = 0; k < 3; ++k) origins[3 * r + k] = M[4 * k + 3], directions[3 * r + k] = d[0][k];
  if (pixel_area) pixel_area[r] = rg_pixel_area(d);
  if (dir_norm) dir_norm[r] = nrm0;
}

__global__ __launch_bounds__(256) void raygen_kernel(const int64_t* __restrict__ indices, const float* __restrict__ c2w,
                                                     const float* __restrict__ intr, int64_t n_rays, int64_t n_cams,
                                                     float* __restrict__ origins, float* __restrict__ directions,
                                                     float* __restrict__ pixel_area, float* __restrict__ dir_norm) {
  raygen_body<false>(indices, c2w, intr, nullptr, n_rays, n_cams, origins, directions, pixel_area, dir_norm);
}

// raygen_kernel with OpenCV lens distortion
__global__ __launch_bounds__(256) void raygen_distorted_kernel(const int64_t* __restrict__ indices, const float* __restrict__ c2w,
                                                               const float* __restrict__ intr, const float* __restrict__ dist,
                                                               int64_t n_rays, int64_t n_cams, float* __restrict__ origins,
                                                               float* __restrict__ directions, float* __restrict__ pixel_area,
                                                               float* __restrict__ dir_norm) {
  raygen_body<true>(indices, c2w, intr, dist, n_rays, n_cams, origins, directions, pixel_area, dir_norm);
}

extern "C" int umhs_raygen(const int64_t* indices, const float* c2w, const float* intrinsics, int64_t n_rays,
                           int64_t n_cams, float* origins, float* directions, float* pixel_area, float* directions_norm,
                           umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_cams < 1 || !indices || !c2w || !intrinsics || !origins || !directions) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(raygen_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), indices, c2w,
                     intrinsics, n_rays, n_cams, origins, directions, pixel_area, directions_norm);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_raygen_distorted(const int64_t* indices, const float* c2w, const float* intrinsics, const float* distortion,
                                     int64_t n_rays, int64_t n_cams, float* origins, float* directions, float* pixel_area,
                                     float* directions_norm, umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_cams < 1 || !indices || !c2w || !intrinsics || !distortion || !origins || !directions) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(raygen_distorted_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), indices, c2w,
                     intrinsics, distortion, n_rays, n_cams, origins, directions, pixel_area, directions_norm);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// ---- whole-frame rays (camera paths, crop boxes) ------------------------------------------------------------------------------------
// What the host knows of a frame launch travels by value: the camera, the row range, and the crop box (T, R row-major, S / 2).
struct FrameRays {
  int64_t camera, width, first, n_rays;  // first = row0 * width: ray i is pixel first + i of the frame
  int has_dist, has_box;
  float T[3], R[9], half[3], near_floor;
};

// nerfstudio intersect_obb / intersect_aabb: the ray o + t d (unit d) against the box in the box's own frame.  A zero component of d'
// divides to +-inf (IEEE); fminf / fmaxf ignore a NaN (0 / 0: an origin on a slab's face, parallel to it), which is all the special
// casing there is.
__device__ __forceinline__ void rg_intersect_obb(const float o[3], const float d[3], const FrameRays& a, float& near, float& far) {
#pragma clang fp contract(off)
  const float e[3] = {o[0] - a.T[0], o[1] - a.T[1], o[2] - a.T[2]};
  float t_min = -INFINITY, t_max = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ob = cam_rt_row(a.R, k, e[0], e[1], e[2]);  // (R^T (o - T))_k
    const float db = cam_rt_row(a.R, k, d[0], d[1], d[2]);
    const float ta = (-a.half[k] - ob) / db, tb = (a.half[k] - ob) / db;
    t_min = fmaxf(t_min, fminf(ta, tb)), t_max = fminf(t_max, fmaxf(ta, tb));
  }
  t_min = fminf(fmaxf(t_min, 0.0f), 1e10f), t_max = fminf(fmaxf(t_max, 0.0f), 1e10f);
  const bool miss = t_max <= t_min;
  near = miss ? 1e10f : fmaxf(t_min, a.near_floor), far = miss ? 1e10f : t_max;
}

// One thread per pixel, 256 pixels per block.  The kernel only writes (~40 B per ray): the [R,3] rows go out as whole dwords in ray
// order -- thread t stores floats t, t + 256, t + 512 of the block's 768 -- the directions through LDS (a stride of 3 dwords is free of
// bank conflicts), the origins straight from the pose (float j of any block is translation component j % 3: 768 is a multiple of 3).
template <int TYPE>
__global__ __launch_bounds__(256) void raygen_frame_kernel(const float* __restrict__ c2w, const float* __restrict__ intr,
                                                           const float* __restrict__ dist, const FrameRays a,
                                                           float* __restrict__ origins, float* __restrict__ directions,
                                                           float* __restrict__ pixel_area, float* __restrict__ dir_norm,
                                                           float* __restrict__ nears, float* __restrict__ fars) {
#pragma clang fp contract(off)
  __shared__ float rows[768];
  const int64_t base = (int64_t)blockIdx.x * 256, r = base + threadIdx.x;
  const int64_t c = a.camera;
  const float* M = c2w + 12 * c;
  if (r < a.n_rays) {
    const int64_t p = a.first + r;
    int64_t iy, ix;
    if ((uint64_t)p >> 32) {
      iy = p / a.width, ix = p - iy * a.width;
    } else {  // (a 64-bit division is a subroutine on this hardware; a frame's pixel count fits 32 bits unless it is enormous)
      const uint32_t q = (uint32_t)p / (uint32_t)a.width;
      iy = q, ix = (uint32_t)p - q * (uint32_t)a.width;
    }
    const float y = (float)iy + 0.5f, x = (float)ix + 0.5f;  // pixel centres
    const float fx = intr[4 * c], fy = intr[4 * c + 1], cx = intr[4 * c + 2], cy = intr[4 * c + 3];
    float px[3], py[3], cam[3][3], d[3][3];
    rg_plane_points(x, y, fx, fy, cx, cy, px, py);
    if constexpr (TYPE == 0) {
      if (a.has_dist) undistort_plane_points(dist, c, px, py);  // raygen_distorted_kernel's steps
#pragma unroll
      for (int s = 0; s < 3; ++s) cam[s][0] = px[s], cam[s][1] = -py[s], cam[s][2] = -1.0f;
    } else if constexpr (TYPE == 1) {  // fisheye (equidistant): the image-plane radius IS the angle from the axis
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const float u = px[s], v = -py[s];
        const float theta = fminf(fmaxf(sqrtf(u * u + v * v), 0.0f), 3.14159265358979323846f);
        const float sc = theta == 0.0f ? 1.0f : sinf(theta) / theta;  // (upstream divides 0 by 0 at the principal point)
        cam[s][0] = u * sc, cam[s][1] = v * sc, cam[s][2] = -cosf(theta);
      }
    } else {  // equirectangular: longitude across the frame, latitude down it
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const float u = px[s], v = -py[s];
        const float theta = -3.14159265358979323846f * u, phi = 3.14159265358979323846f * (0.5f - v);
        const float sp = sinf(phi);
        cam[s][0] = -sinf(theta) * sp, cam[s][1] = cosf(phi), cam[s][2] = -cosf(theta) * sp;
      }
    }
    const float nrm0 = rg_world_directions(cam, M, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) rows[3 * threadIdx.x + k] = d[0][k];
    if (pixel_area) pixel_area[r] = rg_pixel_area(d);
    if (dir_norm) dir_norm[r] = nrm0;
    if (a.has_box) {
      const float o[3] = {M[3], M[7], M[11]};
      float near, far;
      rg_intersect_obb(o, d[0], a, near, far);
      nears[r] = near, fars[r] = far;
    }
  }
  __syncthreads();
  const int64_t left = a.n_rays - base;  // rays of this block: >= 1
  const int n_floats = 3 * (int)(left < 256 ? left : 256);
#pragma unroll
  for (int j = threadIdx.x; j < 768; j += 256) {
    if (j < n_floats) {
      directions[3 * base + j] = rows[j];
      origins[3 * base + j] = M[4 * (j % 3) + 3];
    }
  }
}

extern "C" int umhs_raygen_frame(const float* c2w, const float* intrinsics, const float* distortion, int64_t n_cams, int64_t camera,
                                 int camera_type, int64_t height, int64_t width, int64_t row0, int64_t n_rows,
                                 const float* obb_host15, float near_floor, float* origins, float* directions, float* pixel_area,
                                 float* directions_norm, float* nears, float* fars, umhs_stream_t stream) {
  if (!c2w || !intrinsics || !origins || !directions) return UMHS_ERR_ARG;
  if (n_cams < 1 || camera < 0 || camera >= n_cams || camera_type < 0 || camera_type > 2) return UMHS_ERR_ARG;
  if (distortion && camera_type != 0) return UMHS_ERR_ARG;
  if (height < 1 || width < 1 || row0 < 0 || n_rows < 0 || row0 > height || n_rows > height - row0) return UMHS_ERR_ARG;
  if ((nears == nullptr) != (fars == nullptr) || (obb_host15 && !nears)) return UMHS_ERR_ARG;
  if (!(near_floor >= 0.0f)) return UMHS_ERR_ARG;
  if (width > 0x7fffffffLL || height > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;  // (rows * width stays far inside int64)
  FrameRays a;
  a.camera = camera, a.width = width, a.first = row0 * width, a.n_rays = n_rows * width;
  a.has_dist = distortion != nullptr, a.has_box = obb_host15 != nullptr, a.near_floor = near_floor;
  for (int i = 0; i < 3; ++i) a.T[i] = 0.0f, a.half[i] = 0.0f;
  for (int i = 0; i < 9; ++i) a.R[i] = 0.0f;
  if (obb_host15) {
    for (int i = 0; i < 3; ++i) {
      if (!(obb_host15[12 + i] > 0.0f)) return UMHS_ERR_ARG;  // (a NaN scale is refused too)
      a.T[i] = obb_host15[i], a.half[i] = 0.5f * obb_host15[12 + i];
    }
    for (int i = 0; i < 9; ++i) a.R[i] = obb_host15[3 + i];
  }
  if (a.n_rays == 0) return UMHS_OK;
  const int64_t blocks = (a.n_rays + 255) / 256;
  if (blocks > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(256);
  if (camera_type == 0)
    hipLaunchKernelGGL(raygen_frame_kernel<0>, grid, block, 0, umhs_s(stream), c2w, intrinsics, distortion, a, origins, directions,
                       pixel_area, directions_norm, nears, fars);
  else if (camera_type == 1)
    hipLaunchKernelGGL(raygen_frame_kernel<1>, grid, block, 0, umhs_s(stream), c2w, intrinsics, distortion, a, origins, directions,
                       pixel_area, directions_norm, nears, fars);
  else
    hipLaunchKernelGGL(raygen_frame_kernel<2>, grid, block, 0, umhs_s(stream), c2w, intrinsics, distortion, a, origins, directions,
                       pixel_area, directions_norm, nears, fars);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// out[r, :] = stack[c, y, x, :]  (stack [n,H,W,K] fp32, or uint8 scaled by 1/255 as nerfstudio's get_image_float32 does)
template <typename SRC>
__global__ __launch_bounds__(256) void pixel_gather_kernel(const int64_t* __restrict__ indices, const SRC* __restrict__ stack,
                                                           int64_t n, int64_t H, int64_t W, int K, int64_t n_rays,
                                                           float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rays * K) return;
  const int64_t r = i / K;
  const int k = (int)(i - r * K);
  int64_t c = indices[3 * r], y = indices[3 * r + 1], x = indices[3 * r + 2];
  c = c < 0 ? 0 : (c >= n ? n - 1 : c), y = y < 0 ? 0 : (y >= H ? H - 1 : y), x = x < 0 ? 0 : (x >= W ? W - 1 : x);
  const SRC v = stack[((c * H + y) * W + x) * K + k];
  if constexpr (sizeof(SRC) == 1)
    out[i] = (float)v / 255.0f;
  else
    out[i] = v;
}

extern "C" int umhs_pixel_gather(const int64_t* indices, const void* stack, int src_is_u8, int64_t n_images, int64_t height,
                                 int64_t width, int n_channels, int64_t n_rays, float* out, umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_images < 1 || height < 1 || width < 1 || n_channels < 1 || !indices || !stack || !out) return UMHS_ERR_ARG;
  const int64_t total = n_rays * n_channels;
  if ((total + 255) / 256 > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (src_is_u8)
    hipLaunchKernelGGL(pixel_gather_kernel<uint8_t>, grid, dim3(256), 0, umhs_s(stream), indices, (const uint8_t*)stack,
                       n_images, height, width, n_channels, n_rays, out);
  else
    hipLaunchKernelGGL(pixel_gather_kernel<float>, grid, dim3(256), 0, umhs_s(stream), indices, (const float*)stack, n_images,
                       height, width, n_channels, n_rays, out);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// indices[r] = (long)(u[r] * (n, H, W))  -- PixelSampler.sample_method; u from torch.rand so the stream of draws is torch's
__global__ __launch_bounds__(256) void pixel_indices_kernel(const float* __restrict__ u, int64_t n_rays, float n, float H,
                                                            float W, int64_t* __restrict__ indices) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * n_rays) return;
  const int k = (int)(i % 3);
  indices[i] = (int64_t)(u[i] * (k == 0 ? n : (k == 1 ? H : W)));
}

extern "C" int umhs_pixel_indices(const float* uniform, int64_t n_rays, int64_t n_images, int64_t height, int64_t width,
                                  int64_t* indices, umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_images < 1 || height < 1 || width < 1 || !uniform || !indices) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(pixel_indices_kernel, dim3((unsigned)((3 * n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), uniform,
                     n_rays, (float)n_images, (float)height, (float)width, indices);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
