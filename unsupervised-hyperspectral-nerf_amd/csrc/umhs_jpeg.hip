// Baseline-JPEG frame encoder: the composed uint8 frame [H, Wf, 3] on the device -> one complete JFIF file in a device buffer, so that
// only compressed bytes cross to the host and no host thread encodes (camera-path rendering, --jpeg-encoder gpu / --output-format
// video).  include/umhs_hip.h states the format and the arithmetic as THE definition; this comment says how it is laid out on the GPU.
//
// Stage A (jpeg_coef_kernel): one lane per 8 x 8 block of one component, blocks numbered in scan order (MCU after MCU, inside an MCU
// Y .. Cb Cr).  The result is integers, so every operation is one rounded float32 operation through umhs_exact.h and the unit is
// compiled with contraction off, as umhs_frame.hip is.  The row pass runs as the rows are read (8 samples live at a time), the column
// pass out of 64 registers; both fully unrolled, the matrix folded into literals.  A block's 64 int16 go out as eight 16-byte stores.
//
// Stage B (jpeg_entropy_kernel): one wavefront per restart interval -- an interval is an independent, byte-aligned piece of the stream.
// The wave takes the interval's blocks 64 at a time, one per lane.  Per chunk: every lane walks its block once to find its code
// length (the DC predictor is the previous block of the same component, read from the coefficients: no serial chain), a wave scan
// gives bit offsets, every lane walks its block again and deposits its bits into an LDS image of the chunk with 32-bit OR atomics
// (OR commutes: the image does not depend on their order), the image's 0xFF bytes are counted word by word with a second scan, and the
// stuffed bytes of 64 words at a time are laid into a 1 KB LDS ring at the output's own 16-byte phase, from which every complete
// 16-byte piece leaves at once as an aligned dwordx4 store (bytes only in the interval's first and last piece, and at the capacity;
// a whole-chunk second image, 26 KB for the worst case, held the kernel to three wavefronts per CU: the write pass took 67 - 183 us
// for seven panels at 1280 x 720 where the counting pass took 32 - 73).  The up to 7 bits of a chunk's last partial byte are carried
// into the next chunk's image; the interval's last byte is padded with 1-bits and its RSTm / EOI marker is appended to the image.
//
// Count, scan, then write: the kernel runs twice.  The first pass (WRITE = false) builds the bit image as well -- the stuffed length
// depends on the bytes -- but keeps only each interval's length; jpeg_scan_kernel (one workgroup) turns the lengths into offsets,
// writes the header and the length word; the second pass writes every interval at its offset.  The alternative -- write once into a
// worst-case workspace, then compact -- needs 415 bytes per block (a block reaches 1,660 bits, every byte of which may be stuffed),
// 6 to 13 times the raw frame, and still moves every byte twice; this way the workspace is the coefficients plus 8 bytes per interval
// whatever the content, and the stream is a function of the coefficients alone.
#pragma clang fp contract(off)
#include <initializer_list>

#include "umhs_common.h"
#include "umhs_exact.h"

#define JPEG_HEADER_BYTES 629
#define JPEG_COEF_THREADS 256
#define JPEG_CHUNK 64                   // blocks per chunk: one per lane
#define JPEG_BLOCK_MAX_BITS 1660        // DC: 11-bit code + 11 bits; 63 AC: 16-bit code + 10 bits each
#define JPEG_IMG_WORDS 3328             // >= (7 + 64 * 1660 + 31) / 32 + 1 = 3322
#define JPEG_RING_BYTES 1024            // staging of the stuffed bytes: a power of two, >= 15 + 512 + what is being flushed (<= 512)
#define JPEG_SCAN_THREADS 1024

// ---- tables (host and compile time) -----------------------------------------------------------------------------------------------------
static constexpr uint8_t JPEG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static constexpr uint8_t JPEG_BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,  69,  56,  14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K typical Huffman tables: BITS (codes per length 1..16) and HUFFVAL; [0] luminance, [1] chrominance
static constexpr uint8_t JPEG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static constexpr uint8_t JPEG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static constexpr uint8_t JPEG_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// code << 8 | length of every symbol (Annex C); a symbol without a code is 0.  dc[t][category], ac[t][run << 4 | size]
struct jpeg_huff {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};
#define JPEG_HUFF_WORDS (sizeof(jpeg_huff) / 4)

constexpr jpeg_huff jpeg_make_huff() {
  jpeg_huff h{};
  for (int t = 0; t < 2; ++t) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < JPEG_DC_BITS[t][len - 1]; ++i) h.dc[t][k++] = (code++ << 8) | (uint32_t)len;  // HUFFVAL of the DC tables is 0 .. 11
      code <<= 1;
    }
    code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < JPEG_AC_BITS[t][len - 1]; ++i) h.ac[t][JPEG_AC_VALS[t][k++]] = (code++ << 8) | (uint32_t)len;
      code <<= 1;
    }
  }
  return h;
}
__device__ const jpeg_huff jpeg_huff_table = jpeg_make_huff();

// T[u][x] = fl32(1/2 c(u) cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt 2
__device__ const float JPEG_T[8][8] = {
    {0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f},
    {0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f},
    {0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f},
    {0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f},
    {0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f},
    {0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f},
    {0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f},
    {0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f}};

struct jpeg_inverse_zigzag {
  uint8_t pos[64];  // zigzag position of natural index 8 u + v
};
constexpr jpeg_inverse_zigzag jpeg_make_inverse_zigzag() {
  jpeg_inverse_zigzag z{};
  for (int i = 0; i < 64; ++i) z.pos[JPEG_ZIGZAG[i]] = (uint8_t)i;
  return z;
}
__device__ const jpeg_inverse_zigzag JPEG_IZZ = jpeg_make_inverse_zigzag();

struct jpeg_quant {
  float q[2][64];  // divisors in natural order: [0] luminance, [1] chrominance
};
struct jpeg_header {
  uint8_t b[632];  // JPEG_HEADER_BYTES used
};

struct jpeg_geometry {
  int64_t mcu_cols, n_mcus, n_blocks, n_intervals;
  int bpm;  // blocks per MCU: 3 (4:4:4) or 6 (4:2:0)
};

static bool jpeg_geometry_of(int height, int width, int subsampling, int restart_mcus, jpeg_geometry* g) {
  if (height < 1 || width < 1 || height > 65535 || width > 65535 || restart_mcus < 1 || restart_mcus > 65535) return false;
  if (subsampling != UMHS_JPEG_444 && subsampling != UMHS_JPEG_420) return false;
  const int m = subsampling == UMHS_JPEG_420 ? 16 : 8;
  g->bpm = subsampling == UMHS_JPEG_420 ? 6 : 3;
  g->mcu_cols = (width + m - 1) / m;
  g->n_mcus = g->mcu_cols * (int64_t)((height + m - 1) / m);
  g->n_blocks = g->n_mcus * g->bpm;
  g->n_intervals = (g->n_mcus + restart_mcus - 1) / restart_mcus;
  return true;
}

static void jpeg_quant_tables(int quality, uint8_t q[2][64] /* natural order */) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = (JPEG_BASE_Q[t][i] * s + 50) / 100;
      q[t][i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

static void jpeg_build_header(int height, int width, int quality, int subsampling, int restart_mcus, jpeg_header* h) {
  uint8_t q[2][64];
  jpeg_quant_tables(quality, q);
  uint8_t* p = h->b;
  auto put = [&p](std::initializer_list<int> bytes) {
    for (int v : bytes) *p++ = (uint8_t)v;
  };
  put({0xFF, 0xD8});
  put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xDB, 0, 67, t});
    for (int i = 0; i < 64; ++i) *p++ = q[t][JPEG_ZIGZAG[i]];
  }
  put({0xFF, 0xC0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3});
  put({1, subsampling == UMHS_JPEG_420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xC4, 0, 19 + 12, t});
    for (int i = 0; i < 16; ++i) *p++ = JPEG_DC_BITS[t][i];
    for (int i = 0; i < 12; ++i) *p++ = (uint8_t)i;
    put({0xFF, 0xC4, 0, 19 + 162, 0x10 | t});
    for (int i = 0; i < 16; ++i) *p++ = JPEG_AC_BITS[t][i];
    for (int i = 0; i < 162; ++i) *p++ = JPEG_AC_VALS[t][i];
  }
  put({0xFF, 0xDD, 0, 4, restart_mcus >> 8, restart_mcus & 255});
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  while (p < h->b + sizeof(h->b)) *p++ = 0;
}

// ---- stage A: transform ---------------------------------------------------------------------------------------------------------------
// one component of the pixel at (min(y, H - 1), min(x, W - 1)): ((k0 R + k1 G) + k2 B) - off, five rounded operations (off is 128 for Y
// and 0 for the chroma components: x - 0 is x)
__device__ __forceinline__ float jpeg_pixel(const uint8_t* __restrict__ frame, int H, int W, int y, int x, float k0, float k1, float k2, float off) {
  y = y < H - 1 ? y : H - 1, x = x < W - 1 ? x : W - 1;
  const uint8_t* p = frame + ((int64_t)y * W + x) * 3;
  const float R = (float)p[0], G = (float)p[1], B = (float)p[2];
  return xf_sub(xf_add(xf_add(xf_mul(k0, R), xf_mul(k1, G)), xf_mul(k2, B)), off);
}

__global__ __launch_bounds__(JPEG_COEF_THREADS) void jpeg_coef_kernel(const uint8_t* __restrict__ frame, int H, int W, int64_t mcu_cols,
                                                                      int64_t n_blocks, int bpm, jpeg_quant quant,
                                                                      int16_t* __restrict__ coefs) {
  __shared__ float sq[128];
  if (threadIdx.x < 128) sq[threadIdx.x] = (&quant.q[0][0])[threadIdx.x];
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * JPEG_COEF_THREADS + threadIdx.x;
  if (b >= n_blocks) return;
  const int64_t mcu = b / bpm;
  const int j = (int)(b - mcu * bpm), n_y = bpm - 2;
  const int comp = j < n_y ? 0 : j - n_y + 1;
  const int my = (int)(mcu / mcu_cols), mx = (int)(mcu - (int64_t)my * mcu_cols);
  const bool sub = bpm == 6 && comp > 0;  // a chroma block of 4:2:0: every sample is the mean of 2 x 2 pixels
  int y0, x0;
  if (bpm == 6) {
    y0 = my * 16 + (comp == 0 ? (j >> 1) * 8 : 0), x0 = mx * 16 + (comp == 0 ? (j & 1) * 8 : 0);
  } else {
    y0 = my * 8, x0 = mx * 8;
  }
  const float k0 = comp == 0 ? 0.299f : (comp == 1 ? -0.168736f : 0.5f);
  const float k1 = comp == 0 ? 0.587f : (comp == 1 ? -0.331264f : -0.418688f);
  const float k2 = comp == 0 ? 0.114f : (comp == 1 ? 0.5f : -0.081312f);
  const float off = comp == 0 ? 128.0f : 0.0f;

  float G[8][8];  // row pass: G[y][v] = sum_x f[y][x] T[v][x], ascending x from the first product
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    float f[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      if (sub) {
        const int py = y0 + 2 * y, px = x0 + 2 * x;
        const float a = jpeg_pixel(frame, H, W, py, px, k0, k1, k2, off), bb = jpeg_pixel(frame, H, W, py, px + 1, k0, k1, k2, off);
        const float c = jpeg_pixel(frame, H, W, py + 1, px, k0, k1, k2, off), d = jpeg_pixel(frame, H, W, py + 1, px + 1, k0, k1, k2, off);
        f[x] = xf_mul(xf_add(xf_add(a, bb), xf_add(c, d)), 0.25f);
      } else {
        f[x] = jpeg_pixel(frame, H, W, y0 + y, x0 + x, k0, k1, k2, off);
      }
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float s = xf_mul(f[0], JPEG_T[v][0]);
#pragma unroll
      for (int x = 1; x < 8; ++x) s = xf_add(s, xf_mul(f[x], JPEG_T[v][x]));
      G[y][v] = s;
    }
  }
  const float* q = sq + (comp > 0 ? 64 : 0);
  uint32_t packed[32] = {};  // 64 int16 in zigzag order
#pragma unroll
  for (int u = 0; u < 8; ++u) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {  // column pass: F[u][v] = sum_y T[u][y] G[y][v], ascending y
      float s = xf_mul(JPEG_T[u][0], G[0][v]);
#pragma unroll
      for (int y = 1; y < 8; ++y) s = xf_add(s, xf_mul(JPEG_T[u][y], G[y][v]));
      const float r = xf_div(s, q[8 * u + v]);
      float k = truncf(xf_add(fabsf(r), 0.5f));  // sign(v) trunc(|v| + 0.5)
      if (k > 1023.0f) k = (u | v) == 0 && r < 0.0f ? (k > 1024.0f ? 1024.0f : k) : 1023.0f;
      const int ki = r < 0.0f ? -(int)k : (int)k;
      const int z = JPEG_IZZ.pos[8 * u + v];
      packed[z >> 1] |= ((uint32_t)ki & 0xFFFFu) << (16 * (z & 1));
    }
  }
  uint4* o = reinterpret_cast<uint4*>(coefs + b * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = make_uint4(packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]);
}

// ---- stage B: entropy coding ----------------------------------------------------------------------------------------------------------
struct jpeg_sink {
  uint64_t acc;   // pending bits, the oldest at bit 63
  int n;          // how many (below 32 between calls)
  uint32_t* w;    // LDS word the oldest pending bit belongs to
  uint32_t bits;  // bits put so far
};

// append `len` (1 .. 27) bits; words are big-endian bit containers, so the byte image is the MSB-first stream
template <bool EMIT>
__device__ __forceinline__ void jpeg_put(jpeg_sink& s, uint32_t code, int len) {
  s.bits += (uint32_t)len;
  if (EMIT) {
    s.acc |= (uint64_t)code << (64 - s.n - len);
    s.n += len;
    if (s.n >= 32) {
      atomicOr(s.w++, __builtin_bswap32((uint32_t)(s.acc >> 32)));
      s.acc <<= 32, s.n -= 32;
    }
  }
}

// Huffman code of `sym` followed by the `size` low bits of the value (a negative value v is sent as v - 1)
template <bool EMIT>
__device__ __forceinline__ void jpeg_put_symbol(jpeg_sink& s, uint32_t entry, int value, int size) {
  const uint32_t vbits = (uint32_t)(value < 0 ? value - 1 : value) & ((1u << size) - 1u);
  jpeg_put<EMIT>(s, ((entry >> 8) << size) | vbits, (int)(entry & 255u) + size);
}

__device__ __forceinline__ int jpeg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one block: 64 zigzag coefficients (values outside the legal range are clamped into it, as stage A does), DC predictor `pred`
template <bool EMIT>
__device__ void jpeg_block(jpeg_sink& s, const uint4* __restrict__ src, int pred, const uint32_t* dc, const uint32_t* ac) {
  uint32_t run = 0;
#pragma unroll 1
  for (int i = 0; i < 8; ++i) {
    const uint4 q = src[i];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      int c = (int)(int16_t)(w[t >> 1] >> (16 * (t & 1)));
      if (i == 0 && t == 0) {
        const int diff = jpeg_clamp(c, -1024, 1023) - pred;
        const int size = diff == 0 ? 0 : 32 - __clz(diff < 0 ? -diff : diff);  // at most 11
        jpeg_put_symbol<EMIT>(s, dc[size], diff, size);
        continue;
      }
      if (c == 0) {
        ++run;
        continue;
      }
      c = jpeg_clamp(c, -1023, 1023);
      while (run > 15) {
        jpeg_put<EMIT>(s, ac[0xF0] >> 8, (int)(ac[0xF0] & 255u));  // ZRL: sixteen zeros
        run -= 16;
      }
      const int size = 32 - __clz(c < 0 ? -c : c);  // 1 .. 10
      jpeg_put_symbol<EMIT>(s, ac[(run << 4) | (uint32_t)size], c, size);
      run = 0;
    }
  }
  if (run) jpeg_put<EMIT>(s, ac[0] >> 8, (int)(ac[0] & 255u));  // EOB (none after a nonzero coefficient 63)
}

__device__ __forceinline__ uint32_t jpeg_wave_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// WRITE = false: table[i] = bytes of interval i, its marker included.  WRITE = true: table[i] = the offset of interval i behind the
// header; the bytes go to out[JPEG_HEADER_BYTES + table[i] ...], nothing at or past `capacity`.
template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const int16_t* __restrict__ coefs, int64_t n_mcus, int bpm, int64_t restart_mcus,
                                                          int64_t n_intervals, uint64_t* __restrict__ table, uint8_t* __restrict__ out,
                                                          int64_t capacity) {
  __shared__ uint32_t huff[JPEG_HUFF_WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t img[JPEG_IMG_WORDS];
  __shared__ __attribute__((aligned(16))) uint8_t ring[WRITE ? JPEG_RING_BYTES : 16];
  const int lane = threadIdx.x;
  {
    const uint32_t* h = reinterpret_cast<const uint32_t*>(&jpeg_huff_table);
    for (int i = lane; i < (int)JPEG_HUFF_WORDS; i += 64) huff[i] = h[i];
  }
  const int64_t interval = blockIdx.x;
  const int64_t first = interval * restart_mcus, last = first + restart_mcus < n_mcus ? first + restart_mcus : n_mcus;
  const int64_t nb = (last - first) * bpm, b0 = first * bpm;  // this interval's blocks: b0 .. b0 + nb
  const int n_y = bpm - 2;
  const uint32_t marker = interval == n_intervals - 1 ? 0xD9u : 0xD0u + (uint32_t)(interval & 7);
  // WRITE: positions are counted from `base`, the 16-byte boundary at or below the interval's first byte, which is at `phase`; bytes
  // [flushed, staged) wait in the ring, at their position modulo its size (a 16-byte piece never wraps)
  const int64_t gpos = WRITE ? JPEG_HEADER_BYTES + (int64_t)table[interval] : 0;
  const uint32_t phase = WRITE ? (uint32_t)((uintptr_t)(out + gpos) & 15) : 0u;
  uint8_t* const base = out + gpos - phase;
  const int64_t room = capacity - (gpos - phase);  // bytes of `base` below the capacity
  uint32_t staged = phase, flushed = 0;
  // the complete 16-byte pieces of [flushed, staged) -> the output, a piece per lane (bytes in the interval's first piece when it
  // starts inside it, and at the capacity); `last`: the bytes behind the last complete piece as well
  auto flush = [&](bool last_bytes) {
    const uint32_t end = staged & ~15u;
    for (uint32_t lo = flushed + 16 * lane; lo < end; lo += 16 * 64) {
      const uint8_t* src = ring + (lo & (JPEG_RING_BYTES - 1));
      if (lo >= phase && (int64_t)lo + 16 <= room) {
        *reinterpret_cast<uint4*>(base + lo) = *reinterpret_cast<const uint4*>(src);
      } else {
        for (uint32_t k = 0; k < 16; ++k)
          if (lo + k >= phase && (int64_t)(lo + k) < room) base[lo + k] = src[k];
      }
    }
    flushed = end;
    if (last_bytes) {
      const uint32_t p = end + lane;
      if (p < staged && p >= phase && (int64_t)p < room) base[p] = ring[p & (JPEG_RING_BYTES - 1)];
    }
  };
  uint64_t total_bytes = 0;  // (!WRITE) the interval's bytes so far
  uint32_t carry_bits = 0, carry_byte = 0;  // the partial last byte of the previous chunk
  __syncthreads();

  for (int64_t c0 = 0; c0 < nb; c0 += JPEG_CHUNK) {  // (the same trips for every lane: barriers inside)
    const int64_t j = c0 + lane;
    const bool active = j < nb;
    const bool final_chunk = c0 + JPEG_CHUNK >= nb;
    const uint4* src = reinterpret_cast<const uint4*>(coefs + (b0 + (active ? j : 0)) * 64);
    int pred = 0, chroma = 0;
    if (active) {
      const int64_t m = j / bpm;
      const int k = (int)(j - m * bpm);
      chroma = k >= n_y;
      // the previous block of the same component: the Y block before this one (the previous MCU's last one for k == 0), the same
      // chroma block of the previous MCU; none in the interval's first MCU
      const int64_t prev = chroma ? (m > 0 ? j - bpm : -1) : (k > 0 ? j - 1 : (m > 0 ? j - 3 : -1));
      if (prev >= 0) pred = jpeg_clamp((int)coefs[(b0 + prev) * 64], -1024, 1023);
    }
    const uint32_t* dc = huff + 12 * chroma;
    const uint32_t* ac = huff + 24 + 256 * chroma;
    jpeg_sink s{0, 0, nullptr, 0};
    if (active) jpeg_block<false>(s, src, pred, dc, ac);
    const uint32_t mine = s.bits;
    const uint32_t incl = jpeg_wave_scan(mine, lane);
    const uint32_t n_bits = carry_bits + __shfl(incl, 63, 64);  // bits of the image, the carried ones included
    const uint32_t start = carry_bits + incl - mine;

    for (uint32_t w = lane; w < (n_bits + 31) / 32 + 1; w += 64) img[w] = w == 0 ? carry_byte : 0u;
    __syncthreads();
    if (active) {
      jpeg_sink e{0, (int)(start & 31u), img + (start >> 5), 0};
      jpeg_block<true>(e, src, pred, dc, ac);
      if (e.n > 0) atomicOr(e.w, __builtin_bswap32((uint32_t)(e.acc >> 32)));
    }
    __syncthreads();
    uint32_t n_bytes = n_bits >> 3;
    const uint32_t rem = n_bits & 7u;
    if (final_chunk) {
      if (rem) {  // pad the interval's last byte with 1-bits
        if (lane == 0) atomicOr(img + (n_bytes >> 2), (0xFFu >> rem) << (8 * (n_bytes & 3u)));
        ++n_bytes;
        __syncthreads();
      }
    } else {
      carry_bits = rem;
      carry_byte = rem ? (img[n_bytes >> 2] >> (8 * (n_bytes & 3u))) & 0xFFu : 0u;
    }

    // stuffing: 64 words at a time, a scan over (bytes + 0xFF bytes) of each lane's word: at most 512 bytes into the ring, which then
    // gives up its complete pieces (it holds at most 15 + 512 of its 1,024 bytes: what is being read is not what is written next)
    for (uint32_t w0 = 0; w0 < (n_bytes + 3) / 4; w0 += 64) {
      const uint32_t w = w0 + lane;
      const uint32_t have = 4 * w < n_bytes ? (n_bytes - 4 * w < 4 ? n_bytes - 4 * w : 4u) : 0u;
      const uint32_t v = have ? img[w] : 0u;
      uint32_t cnt = have;
      for (uint32_t k = 0; k < have; ++k) cnt += ((v >> (8 * k)) & 0xFFu) == 0xFFu;
      const uint32_t scan = jpeg_wave_scan(cnt, lane);
      const uint32_t all = __shfl(scan, 63, 64);
      if (WRITE) {
        uint32_t p = staged + scan - cnt;
        for (uint32_t k = 0; k < have; ++k) {
          const uint32_t byte = (v >> (8 * k)) & 0xFFu;
          ring[p++ & (JPEG_RING_BYTES - 1)] = (uint8_t)byte;
          if (byte == 0xFFu) ring[p++ & (JPEG_RING_BYTES - 1)] = 0;
        }
        staged += all;
        __syncthreads();
        flush(false);
      } else {
        total_bytes += all;
      }
    }
    if (final_chunk) {  // the interval's marker goes out with its last bytes
      if (WRITE) {
        if (lane == 0) ring[staged & (JPEG_RING_BYTES - 1)] = 0xFF, ring[(staged + 1) & (JPEG_RING_BYTES - 1)] = (uint8_t)marker;
        staged += 2;
        __syncthreads();
        flush(true);
      } else {
        total_bytes += 2;
      }
    }
    __syncthreads();  // the image is rewritten by the next chunk
  }
  if (!WRITE && lane == 0) table[interval] = total_bytes;
}

// lengths -> exclusive offsets (in place), the header, and the length of the file; one workgroup
__global__ __launch_bounds__(JPEG_SCAN_THREADS) void jpeg_scan_kernel(jpeg_header header, uint64_t* __restrict__ table, int64_t n_intervals,
                                                                      uint8_t* __restrict__ out, int64_t capacity,
                                                                      int64_t* __restrict__ length) {
  __shared__ unsigned long long wave_total[JPEG_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long carry = 0;
  for (int64_t base = 0; base < n_intervals; base += JPEG_SCAN_THREADS) {
    const int64_t i = base + tid;
    const unsigned long long v = i < n_intervals ? table[i] : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int k = 0; k < JPEG_SCAN_THREADS / 64; ++k) {
      if (k < wave) before += wave_total[k];
      all += wave_total[k];
    }
    if (i < n_intervals) table[i] = carry + before + incl - v;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) *length = JPEG_HEADER_BYTES + (int64_t)carry;
  for (int k = tid; k < JPEG_HEADER_BYTES; k += JPEG_SCAN_THREADS)  // (629 bytes at any address, once per frame: byte stores)
    if (k < capacity) out[k] = header.b[k];
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
static size_t jpeg_coef_bytes(const jpeg_geometry& g) { return ((size_t)g.n_blocks * 128 + 15) & ~(size_t)15; }

extern "C" size_t umhs_jpeg_workspace_bytes(int height, int width, int subsampling, int restart_mcus) {
  jpeg_geometry g;
  if (!jpeg_geometry_of(height, width, subsampling, restart_mcus, &g)) return 0;
  return jpeg_coef_bytes(g) + 8 * (size_t)g.n_intervals;
}

extern "C" size_t umhs_jpeg_max_bytes(int height, int width, int subsampling, int restart_mcus) {
  jpeg_geometry g;
  if (!jpeg_geometry_of(height, width, subsampling, restart_mcus, &g)) return 0;
  // per block 1,660 bits = 207.5 bytes, every one of which may be stuffed; per interval the rounding up to a byte, that byte's stuffing
  // and the marker
  return JPEG_HEADER_BYTES + 415 * (size_t)g.n_blocks + 4 * (size_t)g.n_intervals;
}

extern "C" int64_t umhs_jpeg_blocks(int height, int width, int subsampling) {
  jpeg_geometry g;
  return jpeg_geometry_of(height, width, subsampling, 1, &g) ? g.n_blocks : 0;
}

static int jpeg_check(int height, int width, int quality, int subsampling, int restart_mcus, jpeg_geometry* g) {
  if (height < 1 || width < 1 || quality < 1 || quality > 100 || restart_mcus < 1) return UMHS_ERR_ARG;
  if (subsampling != UMHS_JPEG_444 && subsampling != UMHS_JPEG_420) return UMHS_ERR_ARG;
  if (height > 65535 || width > 65535 || restart_mcus > 65535) return UMHS_ERR_UNSUPPORTED;
  return jpeg_geometry_of(height, width, subsampling, restart_mcus, g) ? UMHS_OK : UMHS_ERR_ARG;
}

extern "C" int umhs_jpeg_coefficients(const uint8_t* frame, int height, int width, int quality, int subsampling, int16_t* coefficients,
                                      umhs_stream_t stream) {
  jpeg_geometry g;
  const int rc = jpeg_check(height, width, quality, subsampling, 1, &g);
  if (rc != UMHS_OK) return rc;
  if (!frame || !coefficients || ((uintptr_t)coefficients & 15)) return UMHS_ERR_ARG;
  uint8_t q[2][64];
  jpeg_quant_tables(quality, q);
  jpeg_quant quant;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) quant.q[t][i] = (float)q[t][i];
  const int64_t blocks = (g.n_blocks + JPEG_COEF_THREADS - 1) / JPEG_COEF_THREADS;
  hipLaunchKernelGGL(jpeg_coef_kernel, dim3((unsigned)blocks), dim3(JPEG_COEF_THREADS), 0, umhs_s(stream), frame, height, width, g.mcu_cols,
                     g.n_blocks, g.bpm, quant, coefficients);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_jpeg_entropy(const int16_t* coefficients, int height, int width, int quality, int subsampling, int restart_mcus,
                                 uint8_t* out, int64_t capacity, int64_t* length, void* workspace, size_t workspace_bytes,
                                 umhs_stream_t stream) {
  jpeg_geometry g;
  const int rc = jpeg_check(height, width, quality, subsampling, restart_mcus, &g);
  if (rc != UMHS_OK) return rc;
  if (!coefficients || ((uintptr_t)coefficients & 15) || !out || capacity < 0 || !length || ((uintptr_t)length & 7)) return UMHS_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < 8 * (size_t)g.n_intervals) return UMHS_ERR_WORKSPACE;
  jpeg_header header;
  jpeg_build_header(height, width, quality, subsampling, restart_mcus, &header);
  uint64_t* table = static_cast<uint64_t*>(workspace);
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)g.n_intervals), dim3(64), 0, umhs_s(stream), coefficients, g.n_mcus, g.bpm,
                     (int64_t)restart_mcus, g.n_intervals, table, out, capacity);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(JPEG_SCAN_THREADS), 0, umhs_s(stream), header, table, g.n_intervals, out, capacity, length);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)g.n_intervals), dim3(64), 0, umhs_s(stream), coefficients, g.n_mcus, g.bpm,
                     (int64_t)restart_mcus, g.n_intervals, table, out, capacity);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_jpeg_encode(const uint8_t* frame, int height, int width, int quality, int subsampling, int restart_mcus, uint8_t* out,
                                int64_t capacity, int64_t* length, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  jpeg_geometry g;
  int rc = jpeg_check(height, width, quality, subsampling, restart_mcus, &g);
  if (rc != UMHS_OK) return rc;
  if (!frame || !out || capacity < 0 || !length || ((uintptr_t)length & 7)) return UMHS_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < jpeg_coef_bytes(g) + 8 * (size_t)g.n_intervals) return UMHS_ERR_WORKSPACE;
  int16_t* coefs = static_cast<int16_t*>(workspace);
  rc = umhs_jpeg_coefficients(frame, height, width, quality, subsampling, coefs, stream);
  if (rc != UMHS_OK) return rc;
  return umhs_jpeg_entropy(coefs, height, width, quality, subsampling, restart_mcus, out, capacity, length,
                           static_cast<uint8_t*>(workspace) + jpeg_coef_bytes(g), 8 * (size_t)g.n_intervals, stream);
}
