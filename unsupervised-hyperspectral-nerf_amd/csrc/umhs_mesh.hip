// Mesh export (what ``ns-export tsdf`` does for a trained model): rendered depth maps -> a truncated signed distance volume
// (umhs_tsdf_integrate), and the volume -> a triangle mesh whose vertices carry colour, material label and abundances
// (umhs_mesh_mark / umhs_mesh_vertices / umhs_mesh_triangles).  include/umhs_hip.h states the arithmetic as THE definition;
// tests/mesh_ref.py restates it in numpy.
//
// Fusion.  One thread owns one lattice point and walks the cameras of the call in order: D, W and Wc live in registers across the
// walk, the attribute planes are touched only by the sightings inside the truncation band (a few per cent of the lattice), so a
// call reads and writes D / W / Wc once and the images where the lattice projects into them.  x runs along the lanes: the 64 points
// of a wave are one lattice row (or two pieces of rows), which a perspective camera maps onto a short line of pixels -- the image
// reads of a wave fall into a handful of cache lines -- and D / W / Wc and every attribute plane are read and written as consecutive
// dwords.  The cameras are part of the kernel's argument block: every lane reads the same one, i.e. scalar loads, no global read per
// point and camera.  No point is written by two threads and nothing is atomic: the volume is a function of the inputs alone, and
// because every update reads exactly what the previous one wrote (a rounded float32 either in a register or in memory), fusing n
// cameras in one call or in several calls split anywhere gives the same bits.
//
// Extraction is marching tetrahedra on the Kuhn decomposition: a cell is cut into the six tetrahedra around its main diagonal, one
// per permutation (a, b, c) of the axes, with corners  v0 = 000, v1 = v0 + e_a, v2 = v1 + e_b, v3 = 111.  Every tetrahedron edge joins
// a lattice point to one of its 7 neighbours towards +(100, 010, 001, 110, 101, 011, 111): the lower end owns the edge, in that slot
// order.  The passes follow umhs_pointcloud.hip's "count, scan, emit": umhs_mesh_mark writes the 7-bit mask of the edges a point
// owns that carry a vertex and the vertex / triangle counts per chunk of 256 lattice indices; the caller scans the counts;
// umhs_mesh_vertices ranks the points of a chunk (wave scan, wave totals through LDS), writes every point's vertex base and the rows;
// umhs_mesh_triangles ranks the cells the same way and writes the index triples, a vertex id being the owner's base plus the number
// of mask bits below the slot.  No search, no hash, no atomics.  The vertex rows are 15 or 19 + 4 C bytes (no alpha byte), so they
// start at any byte address and are stored as bytes.
//
// The unit is compiled with contraction off: every position, t and attribute is one rounded float32 operation per step, the xf_*
// operations of umhs_exact.h (which says why the __f*_rn intrinsics do not give that); the camera model is umhs_camera.h's.
#pragma clang fp contract(off)
#include "umhs_common.h"
#include "umhs_exact.h"
#include "umhs_camera.h"
#include "umhs_affine.h"

#define MESH_THREADS 256
#define MESH_MAX_CLASSES 16
#define MESH_MAX_POINTS (1LL << 28)  // 7 vertices per point stay below 2^31

// exclusive prefix of v over the 256 threads of a workgroup, in thread order; total = the workgroup's sum.  Every thread calls it.
__device__ __forceinline__ int ms_block_exclusive(int v, int* wave_total, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(s, d, 64);
    if (lane >= d) s += o;
  }
  if (lane == 63) wave_total[wave] = s;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < MESH_THREADS / UMHS_WAVE; ++k) {
    const int t = wave_total[k];
    before += k < wave ? t : 0;
    total += t;
  }
  return before + s - v;
}

// ---- fusion ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MESH_THREADS) void tsdf_integrate_kernel(umhs_tsdf_volume V, umhs_tsdf_images I) {
#pragma clang fp contract(off)
  const int nx = V.dims[0], ny = V.dims[1];
  const int64_t N = (int64_t)nx * ny * V.dims[2];
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= N) return;
  const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((int64_t)nx * ny));
  const float p0 = xf_add(V.lo[0], xf_mul((float)x, V.h)), p1 = xf_add(V.lo[1], xf_mul((float)y, V.h)),
              p2 = xf_add(V.lo[2], xf_mul((float)z, V.h));
  float D = V.D[i], W = V.W[i], Wc = V.Wc[i];
  const int C = I.n_classes;
  const float trunc = I.truncation;
  for (int c = 0; c < I.n_cameras; ++c) {
    const umhs_tsdf_camera& cam = I.cameras[c];
    const float e0 = xf_sub(p0, cam.origin[0]), e1 = xf_sub(p1, cam.origin[1]), e2 = xf_sub(p2, cam.origin[2]);
    // pc = R^T e: world -> camera
    const float pcx = cam_rt_row(cam.rotation, 0, e0, e1, e2), pcy = cam_rt_row(cam.rotation, 1, e0, e1, e2),
                pcz = cam_rt_row(cam.rotation, 2, e0, e1, e2);
    const float zc = -pcz;
    if (!(zc > 0.0f)) continue;
    float px = xf_div(pcx, zc), py = xf_div(-pcy, zc);  // image plane, y down
    if (cam.distorted) {  // the very function undistort_opencv's residual subtracts (xd, yd) from
      const cam_distorted pd = distort_opencv(px, py, cam.distortion);
      px = pd.x, py = pd.y;
    }
    const float u = xf_add(xf_mul(cam.fx, px), cam.cx), v = xf_add(xf_mul(cam.fy, py), cam.cy);
    if (!(u >= 0.0f && u < (float)I.width && v >= 0.0f && v < (float)I.height)) continue;  // (a NaN is outside)
    const int iu = (int)u, iv = (int)v;  // u, v >= 0: truncation is floor; pixel centres sit at +0.5
    if (iu >= I.width || iv >= I.height) continue;
    const float depth = I.depth[c * I.depth_strides[0] + iv * I.depth_strides[1] + iu * I.depth_strides[2]];
    if (!xf_finite(depth)) continue;
    const float acc = I.accumulation[c * I.accumulation_strides[0] + iv * I.accumulation_strides[1] + iu * I.accumulation_strides[2]];
    float obs = 1.0f;
    bool tint = false;
    if (!(acc <= I.threshold)) {  // a hit
      const float dist = sqrtf(xf_add(xf_add(xf_mul(e0, e0), xf_mul(e1, e1)), xf_mul(e2, e2)));
      const float sdf = xf_sub(depth, dist);
      if (sdf < -trunc) continue;
      obs = fminf(1.0f, xf_div(sdf, trunc));
      tint = fabsf(sdf) <= trunc;
    }
    D = xf_div(xf_add(xf_mul(D, W), obs), xf_add(W, 1.0f));
    W = xf_add(W, 1.0f);
    if (tint) {
      const float w1 = xf_add(Wc, 1.0f);
      const float* rgb = I.rgb + c * I.rgb_strides[0] + iv * I.rgb_strides[1] + iu * I.rgb_strides[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float* a = V.A + k * N + i;
        *a = xf_div(xf_add(xf_mul(*a, Wc), rgb[k]), w1);
      }
      if (C > 0) {
        const float* ab = I.abundances + c * I.abundances_strides[0] + iv * I.abundances_strides[1] + iu * I.abundances_strides[2];
        const float* sp = I.seg_probs + c * I.seg_probs_strides[0] + iv * I.seg_probs_strides[1] + iu * I.seg_probs_strides[2];
        for (int k = 0; k < C; ++k) {
          float* a = V.A + (3 + k) * N + i;
          *a = xf_div(xf_add(xf_mul(*a, Wc), ab[k]), w1);
          float* s = V.A + (3 + C + k) * N + i;
          *s = xf_div(xf_add(xf_mul(*s, Wc), sp[k]), w1);
        }
      }
      Wc = w1;
    }
  }
  V.D[i] = D, V.W[i] = W, V.Wc[i] = Wc;
}

static int volume_check(const umhs_tsdf_volume* v, int64_t& n) {
  if (!v) return UMHS_ERR_ARG;
  n = 1;
  for (int k = 0; k < 3; ++k) {
    if (v->dims[k] < 1) return UMHS_ERR_ARG;
    if (v->dims[k] > MESH_MAX_POINTS) return UMHS_ERR_UNSUPPORTED;
    n *= v->dims[k];
    if (n > MESH_MAX_POINTS) return UMHS_ERR_UNSUPPORTED;
    if (!xf_finite(v->lo[k])) return UMHS_ERR_ARG;
  }
  if (!(v->h > 0.0f) || !xf_finite(v->h)) return UMHS_ERR_ARG;
  if (!v->D || !v->W || !v->Wc) return UMHS_ERR_ARG;
  if (v->n_attr < 3 || ((v->n_attr - 3) & 1)) return UMHS_ERR_ARG;
  if ((v->n_attr - 3) / 2 > MESH_MAX_CLASSES) return UMHS_ERR_UNSUPPORTED;
  if (!v->A) return UMHS_ERR_ARG;
  return UMHS_OK;
}

static bool strides_ok(const int64_t s[3]) { return s[0] >= 0 && s[1] >= 0 && s[2] >= 0; }

extern "C" int64_t umhs_mesh_chunks(int64_t n_points) { return n_points < 1 ? 0 : (n_points + MESH_THREADS - 1) / MESH_THREADS; }

extern "C" int umhs_tsdf_integrate(const umhs_tsdf_volume* volume, const umhs_tsdf_images* images, umhs_stream_t stream) {
  int64_t n;
  const int rc = volume_check(volume, n);
  if (rc != UMHS_OK) return rc;
  if (!images || images->n_cameras < 0 || images->n_classes < 0) return UMHS_ERR_ARG;
  if (images->n_cameras > UMHS_TSDF_MAX_CAMERAS || images->n_classes > MESH_MAX_CLASSES) return UMHS_ERR_UNSUPPORTED;
  if (volume->n_attr != 3 + 2 * images->n_classes) return UMHS_ERR_ARG;
  if (images->n_cameras == 0) return UMHS_OK;
  if (images->height < 1 || images->width < 1 || images->height > (1 << 24) || images->width > (1 << 24)) return UMHS_ERR_ARG;
  if (!images->depth || !images->accumulation || !images->rgb) return UMHS_ERR_ARG;
  if (images->n_classes > 0 && (!images->abundances || !images->seg_probs)) return UMHS_ERR_ARG;
  if (!strides_ok(images->depth_strides) || !strides_ok(images->accumulation_strides) || !strides_ok(images->rgb_strides)) return UMHS_ERR_ARG;
  if (images->n_classes > 0 && (!strides_ok(images->abundances_strides) || !strides_ok(images->seg_probs_strides))) return UMHS_ERR_ARG;
  if (!(images->truncation > 0.0f) || !xf_finite(images->truncation) || images->threshold != images->threshold) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)umhs_mesh_chunks(n)), dim3(MESH_THREADS), 0, umhs_s(stream), *volume, *images);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// ---- extraction --------------------------------------------------------------------------------------------------------------------
// corner o of a cell, o = bit 0: +x, bit 1: +y, bit 2: +z
__device__ __forceinline__ int64_t ms_corner(int64_t i, int o, int nx, int64_t nxy) {
  return i + (o & 1) + ((o >> 1) & 1) * (int64_t)nx + ((o >> 2) & 1) * nxy;
}

// slot of the edge towards offset o (1..7): 100 -> 0, 010 -> 1, 001 -> 2, 110 -> 3, 101 -> 4, 011 -> 5, 111 -> 6
__device__ __forceinline__ int ms_slot(int o) { return (int)((0x65423100u >> (4 * o)) & 7u); }

// the two axes a, b of tetrahedron t (permutations of (0,1,2) in lexicographic order); odd permutations: 1, 2, 5
__device__ __forceinline__ void ms_tet(int t, int& o1, int& o2, int& odd) {
  const int a = t >> 1;                                     // 0 0 1 1 2 2
  const int b = (0x102021 >> (4 * t)) & 3;                  // 1 2 0 2 0 1
  o1 = 1 << a, o2 = o1 | (1 << b);
  odd = (0x26 >> t) & 1;                                    // t = 1, 2, 5
}

// inside bits of the 8 corners (bit o) of cell i, or -1 if the cell emits nothing (outside the lattice's cells, or a corner with W = 0)
__device__ __forceinline__ int ms_cell_signs(const umhs_tsdf_volume& V, int64_t i, int64_t N) {
  const int nx = V.dims[0], ny = V.dims[1], nz = V.dims[2];
  if (i >= N) return -1;
  const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((int64_t)nx * ny));
  if (x + 1 >= nx || y + 1 >= ny || z + 1 >= nz) return -1;
  int in = 0;
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int64_t j = ms_corner(i, o, nx, (int64_t)nx * ny);
    if (!(V.W[j] > 0.0f)) return -1;
    in |= (V.D[j] < 0.0f ? 1 : 0) << o;
  }
  return in;
}

// inside code of tetrahedron t: bit k = corner v_k inside
__device__ __forceinline__ int ms_tet_code(int in, int o1, int o2) {
  return (in & 1) | (((in >> o1) & 1) << 1) | (((in >> o2) & 1) << 2) | (((in >> 7) & 1) << 3);
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_mark_kernel(umhs_tsdf_volume V, uint8_t* __restrict__ edge_mask,
                                                                 int32_t* __restrict__ vertex_counts, int32_t* __restrict__ triangle_counts) {
  __shared__ int wt[MESH_THREADS / UMHS_WAVE];
  const int nx = V.dims[0], ny = V.dims[1], nz = V.dims[2];
  const int64_t nxy = (int64_t)nx * ny, N = nxy * nz;
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  int mask = 0, tris = 0;
  if (i < N) {
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / nxy);
    if (V.W[i] > 0.0f) {
      const bool in = V.D[i] < 0.0f;
#pragma unroll
      for (int o = 1; o < 8; ++o) {
        if (x + (o & 1) >= nx || y + ((o >> 1) & 1) >= ny || z + ((o >> 2) & 1) >= nz) continue;
        const int64_t j = ms_corner(i, o, nx, nxy);
        if (V.W[j] > 0.0f && (V.D[j] < 0.0f) != in) mask |= 1 << ms_slot(o);
      }
    }
    edge_mask[i] = (uint8_t)mask;
    const int signs = ms_cell_signs(V, i, N);
    if (signs >= 0) {
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        int o1, o2, odd;
        ms_tet(t, o1, o2, odd);
        const int n = __popc(ms_tet_code(signs, o1, o2));
        tris += n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
      }
    }
  }
  int total;
  ms_block_exclusive(__popc(mask), wt, total);
  if (threadIdx.x == 0) vertex_counts[blockIdx.x] = total;
  __syncthreads();
  ms_block_exclusive(tris, wt, total);
  if (threadIdx.x == 0) triangle_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_vertices_kernel(umhs_tsdf_volume V, const uint8_t* __restrict__ edge_mask,
                                                                     const int64_t* __restrict__ vertex_offsets, xf_world Wd,
                                                                     int32_t* __restrict__ vertex_base, uint8_t* __restrict__ rows, int64_t cap) {
#pragma clang fp contract(off)
  __shared__ int wt[MESH_THREADS / UMHS_WAVE];
  const int nx = V.dims[0], ny = V.dims[1];
  const int64_t nxy = (int64_t)nx * ny, N = nxy * V.dims[2];
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  const int mask = i < N ? edge_mask[i] & 0x7f : 0;
  int total;
  const int rank = ms_block_exclusive(__popc(mask), wt, total);
  if (i >= N) return;
  const int64_t base = vertex_offsets[blockIdx.x] + rank;
  vertex_base[i] = (int32_t)base;
  if (!mask) return;
  const int C = (V.n_attr - 3) / 2;
  const int row_bytes = C > 0 ? 19 + 4 * C : 15;
  const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / nxy);
  const float Da = V.D[i];
  const bool ca = V.Wc[i] > 0.0f;
  const float pa[3] = {xf_add(V.lo[0], xf_mul((float)x, V.h)), xf_add(V.lo[1], xf_mul((float)y, V.h)),
                       xf_add(V.lo[2], xf_mul((float)z, V.h))};
  int id = 0;
  for (int s = 0; s < 7; ++s) {  // (slot order is not offset order: walk the slots)
    if (!((mask >> s) & 1)) continue;
    const int64_t at = base + id;
    ++id;
    if (at < 0 || at >= cap) continue;
    const int o = (int)((0x7653421u >> (4 * s)) & 7u);  // offset of slot s: 1, 2, 4, 3, 5, 6, 7
    if (x + (o & 1) >= nx || y + ((o >> 1) & 1) >= ny || z + ((o >> 2) & 1) >= V.dims[2]) continue;  // (never with umhs_mesh_mark's mask)
    const int64_t j = ms_corner(i, o, nx, nxy);
    const float Db = V.D[j];
    const bool cb = V.Wc[j] > 0.0f;
    const float t = xf_div(Da, xf_sub(Da, Db));
    const float pb[3] = {xf_add(V.lo[0], xf_mul((float)(x + (o & 1)), V.h)), xf_add(V.lo[1], xf_mul((float)(y + ((o >> 1) & 1)), V.h)),
                         xf_add(V.lo[2], xf_mul((float)(z + ((o >> 2) & 1)), V.h))};
    float p[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = xf_add(pa[k], xf_mul(t, xf_sub(pb[k], pa[k])));
    xf_world_apply(Wd, p, w);
    // attribute k of the vertex: both ends tinted -> a + t (b - a); one -> that end; none -> 0
    auto attr = [&](int k) -> float {
      const float a = ca ? V.A[k * N + i] : 0.0f, b = cb ? V.A[k * N + j] : 0.0f;
      return (ca && cb) ? xf_add(a, xf_mul(t, xf_sub(b, a))) : ca ? a : b;
    };
    uint8_t* row = rows + at * (int64_t)row_bytes;
    auto put = [&](int byte, uint32_t v) {
      row[byte] = (uint8_t)v, row[byte + 1] = (uint8_t)(v >> 8), row[byte + 2] = (uint8_t)(v >> 16), row[byte + 3] = (uint8_t)(v >> 24);
    };
#pragma unroll
    for (int k = 0; k < 3; ++k) put(4 * k, __float_as_uint(w[k]));
#pragma unroll
    for (int k = 0; k < 3; ++k) row[12 + k] = (uint8_t)xf_byte(attr(k));
    if (C > 0) {
      int arg = -1;
      if (ca || cb) {
        float mx = -INFINITY;
        arg = 0;
        for (int k = 0; k < C; ++k) {  // the first of the largest; a NaN never wins
          const float v = attr(3 + C + k);
          if (v > mx) mx = v, arg = k;
        }
      }
      put(15, (uint32_t)arg);
      for (int k = 0; k < C; ++k) put(19 + 4 * k, __float_as_uint(attr(3 + k)));
    }
  }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_triangles_kernel(umhs_tsdf_volume V, const uint8_t* __restrict__ edge_mask,
                                                                      const int32_t* __restrict__ vertex_base,
                                                                      const int64_t* __restrict__ triangle_offsets, int32_t* __restrict__ faces,
                                                                      int64_t cap) {
  __shared__ int wt[MESH_THREADS / UMHS_WAVE];
  const int nx = V.dims[0], ny = V.dims[1];
  const int64_t nxy = (int64_t)nx * ny, N = nxy * V.dims[2];
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  const int signs = ms_cell_signs(V, i, N);
  int tris = 0;
  if (signs >= 0) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      int o1, o2, odd;
      ms_tet(t, o1, o2, odd);
      const int n = __popc(ms_tet_code(signs, o1, o2));
      tris += n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
    }
  }
  int total;
  const int rank = ms_block_exclusive(tris, wt, total);
  if (!tris) return;
  int64_t at = triangle_offsets[blockIdx.x] + rank;
  for (int t = 0; t < 6; ++t) {
    int o1, o2, odd;
    ms_tet(t, o1, o2, odd);
    const int ov[4] = {0, o1, o2, 7};
    const int code = ms_tet_code(signs, o1, o2);
    const int n = __popc(code);
    if (n == 0 || n == 4) continue;
    // the vertex on the edge between corners a < b of this tetrahedron
    auto vid = [&](int a, int b) -> int32_t {
      const int64_t owner = ms_corner(i, ov[a], nx, nxy);
      const int slot = ms_slot(ov[b] ^ ov[a]);
      return vertex_base[owner] + __popc((int)edge_mask[owner] & ((1 << slot) - 1));
    };
    auto edge = [&](int a, int b) -> int32_t { return a < b ? vid(a, b) : vid(b, a); };
    auto emit = [&](int32_t a, int32_t b, int32_t c, bool flip) {
      if (at >= 0 && at < cap) {
        faces[3 * at] = a, faces[3 * at + 1] = flip ? c : b, faces[3 * at + 2] = flip ? b : c;
      }
      ++at;
    };
    if (n == 2) {
      int p[2], q[2], np = 0, nq = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((code >> k) & 1) p[np++] = k;
        else q[nq++] = k;
      }
      const int inv = (p[0] > q[0]) + (p[0] > q[1]) + (p[1] > q[0]) + (p[1] > q[1]);
      const bool flip = ((inv & 1) ^ odd) != 0;
      const int32_t a = edge(p[0], q[0]), b = edge(p[0], q[1]), c = edge(p[1], q[1]), d = edge(p[1], q[0]);
      emit(a, b, c, flip);
      emit(a, c, d, flip);
    } else {
      const int lone = n == 1 ? code : (~code & 15);
      const int p = __ffs(lone) - 1;
      int q[3], nq = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k != p) q[nq++] = k;
      const bool flip = (((p & 1) ^ odd ^ (n == 3 ? 1 : 0)) & 1) != 0;
      emit(edge(p, q[0]), edge(p, q[1]), edge(p, q[2]), flip);
    }
  }
}

extern "C" int umhs_mesh_mark(const umhs_tsdf_volume* volume, uint8_t* edge_mask, int32_t* vertex_counts, int32_t* triangle_counts,
                              umhs_stream_t stream) {
  int64_t n;
  const int rc = volume_check(volume, n);
  if (rc != UMHS_OK) return rc;
  if (!edge_mask || !vertex_counts || !triangle_counts) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(mesh_mark_kernel, dim3((unsigned)umhs_mesh_chunks(n)), dim3(MESH_THREADS), 0, umhs_s(stream), *volume, edge_mask,
                     vertex_counts, triangle_counts);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_mesh_vertices(const umhs_tsdf_volume* volume, const uint8_t* edge_mask, const int64_t* vertex_offsets,
                                  const float* world_host12, int32_t* vertex_base, void* rows, int64_t cap, umhs_stream_t stream) {
  int64_t n;
  const int rc = volume_check(volume, n);
  if (rc != UMHS_OK) return rc;
  if (cap < 0 || !edge_mask || !vertex_offsets || !vertex_base || (cap > 0 && !rows)) return UMHS_ERR_ARG;
  const xf_world w = xf_world_from_host(world_host12);
  hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)umhs_mesh_chunks(n)), dim3(MESH_THREADS), 0, umhs_s(stream), *volume, edge_mask,
                     vertex_offsets, w, vertex_base, reinterpret_cast<uint8_t*>(rows), cap);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_mesh_triangles(const umhs_tsdf_volume* volume, const uint8_t* edge_mask, const int32_t* vertex_base,
                                   const int64_t* triangle_offsets, int32_t* faces, int64_t cap, umhs_stream_t stream) {
  int64_t n;
  const int rc = volume_check(volume, n);
  if (rc != UMHS_OK) return rc;
  if (cap < 0 || !edge_mask || !vertex_base || !triangle_offsets || (cap > 0 && !faces)) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(mesh_triangles_kernel, dim3((unsigned)umhs_mesh_chunks(n)), dim3(MESH_THREADS), 0, umhs_s(stream), *volume, edge_mask,
                     vertex_base, triangle_offsets, faces, cap);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
