// PNG frame encoder: a uint8 frame [H, W, C] (C = 3 or 1) on the device -> one complete PNG file in a device buffer, so that a lossless
// frame crosses to the host as compressed bytes and no host thread deflates (camera-path rendering, --png-encoder gpu; the atlases of
// the textured-mesh export).  include/umhs_hip.h states the stream as THE definition; this comment says how it is laid out on the GPU.
//
// Stage A (png_filter_kernel): one workgroup per row.  A first pass over the row sums min(f, 256 - f) of all five filters per thread,
// the five sums are reduced with wave shuffles and integer LDS adds, every thread takes the same least type and a second pass writes
// the row under it (a fixed filter skips the first pass).  The raw row above is all a row needs: the rows are independent.
//
// Stage B works piece by piece (stripe_rows filtered rows), a workgroup per piece, the piece in tiles of 3,824 bytes plus 272 bytes of
// look-ahead in LDS, 16 consecutive bytes per thread.  A byte is a run head when it differs from its predecessor.  What a byte emits
// depends on (a) how far it is behind its run's head, modulo 258 -- a max-scan of head positions over the workgroup, carried from
// tile to tile as that phase alone -- and (b) for the byte at phase 0, how many equal bytes follow, up to 258 -- a min-scan of head
// positions from the right; 258 bytes of look-ahead are all it ever needs.  There is no match search.  (png_tokens is the one
// place the token rule is written; the statistics and the write kernel both call it.)
//   png_stats_kernel: the tokens into a 286-bin LDS histogram (integer adds), the Adler-32 partial sums of the piece, then the code
//     lengths: a parallel rank sort by (count, symbol), the two-queue Huffman merge on one thread (at most 285 steps), leaf depths
//     counted per level, the Kraft fix-up for the 15-bit limit, the levels handed back to the sorted symbols, canonical codes.  The
//     bit-reversed codes go to the workspace, with the piece's exact byte count.
//   png_scan_kernel (one workgroup): chunk offsets by a prefix sum of the byte counts; signature, IHDR, every IDAT's length and type,
//     the zlib header, the final block with the combined Adler-32, IEND; *length.
//   png_write_kernel: the tokens again; per-thread bit counts, a workgroup scan for bit offsets, the codes OR-ed into an LDS image
//     of the tile's bits (OR commutes: the image does not depend on the order) that is laid at the output's own 4-byte phase, so
//     that every complete word leaves as one aligned dword store (bytes only at the piece's two ends and at the capacity); up to
//     31 bits are carried into the next tile's image.
//   png_crc_kernel: the CRC-32 of every IDAT chunk, read back from the output: each thread a contiguous slice, its register
//     multiplied by x^(8 * bytes behind the slice) mod P, the products XOR-ed together (XOR commutes as well).
// Count, scan, then write, as the JPEG encoder does: the workspace is the filtered bytes plus 1,184 bytes per piece whatever the
// content, and the stream is a function of the pixels and the parameters alone.
#include "umhs_common.h"

#define PNG_THREADS 256
#define PNG_SEG 16                          // bytes of a tile per thread
#define PNG_TILE (PNG_THREADS * PNG_SEG)    // bytes in LDS
#define PNG_HALO 272                        // look-ahead: >= 258, whole segments
#define PNG_MAIN (PNG_TILE - PNG_HALO)      // bytes a tile emits tokens for
#define PNG_SYMS 286
#define PNG_TABLE_WORDS 288                 // per piece: reversed code << 8 | length of every literal/length symbol
#define PNG_MAX_BITS 15
#define PNG_RUN 258                         // longest match
#define PNG_IMG_WORDS 1800                  // >= (31 + PNG_MAIN * 15) / 32 + 2
#define PNG_HEADER_BITS 74                  // block header in front of the code lengths (4 bits each)
#define PNG_EOB 256
#define PNG_ADLER 65521u
#define PNG_CRC_POLY 0xEDB88320u

struct png_piece {       // workspace record of one piece
  uint64_t bytes;        // its deflate bytes, the empty stored block included
  uint64_t offset;       // where they start in the file (png_scan_kernel)
  uint32_t s1, s2;       // sum of its bytes, and of (n - i) * byte i, modulo 65521
  uint32_t nlit, pad;    // literal/length codes sent (HLIT + 257)
};

struct png_header {
  uint8_t b[36];  // signature and IHDR: 33 bytes
};

struct png_geometry {
  int64_t row_bytes, total, n_pieces;
  int bpp;
};

// the most bytes a piece of n filtered bytes can take: header 74 + 4 * 287 bits, 15 bits per byte (a match spends at most 21 on
// three bytes or more), the end-of-block code, 3 bits, the rounding, 4 bytes of stored block
static int64_t png_piece_max(int64_t n) { return (15 * n + 1240 + 7) / 8 + 4; }

static int png_geometry_of(int height, int width, int channels, int stripe_rows, png_geometry* g) {
  if (height < 1 || width < 1 || stripe_rows < 1 || (channels != 1 && channels != 3)) return UMHS_ERR_ARG;
  if (height > 65535 || width > 65535 || stripe_rows > 65535) return UMHS_ERR_UNSUPPORTED;
  g->bpp = channels;
  g->row_bytes = 1 + (int64_t)width * channels;
  g->total = g->row_bytes * height;
  g->n_pieces = (height + stripe_rows - 1) / stripe_rows;
  const int64_t rows = stripe_rows < height ? stripe_rows : height;
  if (png_piece_max(rows * g->row_bytes) + 8 > 0x7FFFFFFFll) return UMHS_ERR_UNSUPPORTED;  // a chunk's length is 31 bits
  return UMHS_OK;
}

static size_t png_filtered_bytes(const png_geometry& g) { return ((size_t)g.total + 15) & ~(size_t)15; }
static size_t png_piece_bytes(const png_geometry& g) { return (size_t)g.n_pieces * (sizeof(png_piece) + 4 * PNG_TABLE_WORDS); }

static uint32_t png_host_crc(const uint8_t* p, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? PNG_CRC_POLY : 0u);
  }
  return ~c;
}

static void png_build_header(int height, int width, int channels, png_header* h) {
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  uint8_t* p = h->b;
  for (int i = 0; i < 8; ++i) *p++ = sig[i];
  const uint8_t ihdr[21] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', 0, 0, (uint8_t)(width >> 8), (uint8_t)width, 0, 0, (uint8_t)(height >> 8),
                            (uint8_t)height, 8, (uint8_t)(channels == 3 ? 2 : 0), 0, 0, 0};
  for (int i = 0; i < 21; ++i) *p++ = ihdr[i];
  const uint32_t crc = png_host_crc(h->b + 12, 17);
  for (int i = 0; i < 4; ++i) *p++ = (uint8_t)(crc >> (24 - 8 * i));
  while (p < h->b + sizeof(h->b)) *p++ = 0;
}

// ---- workgroup primitives (PNG_THREADS threads; `scratch`: 4 words of LDS, free again when the call returns) -----------------------------
// the greatest value of the threads before this one, `seed` for thread 0
__device__ __forceinline__ int png_scan_max_before(int v, int seed, int* scratch, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = v > o ? v : o;
  }
  if (lane == 63) scratch[wave] = v;
  int before = __shfl_up(v, 1, 64);
  if (lane == 0) before = seed;
  __syncthreads();
  for (int k = 0; k < wave; ++k) before = before > scratch[k] ? before : scratch[k];
  before = before > seed ? before : seed;
  __syncthreads();
  return before;
}

// the least value of the threads behind this one, `seed` for the last thread
__device__ __forceinline__ int png_scan_min_behind(int v, int seed, int* scratch, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_down(v, d, 64);
    if (lane + d < 64) v = v < o ? v : o;
  }
  if (lane == 0) scratch[wave] = v;
  int behind = __shfl_down(v, 1, 64);
  if (lane == 63) behind = seed;
  __syncthreads();
  for (int k = wave + 1; k < PNG_THREADS / 64; ++k) behind = behind < scratch[k] ? behind : scratch[k];
  behind = behind < seed ? behind : seed;
  __syncthreads();
  return behind;
}

// the sum of the threads before this one; *total: of all
__device__ __forceinline__ uint32_t png_scan_sum_before(uint32_t v, uint32_t* total, int* scratch, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) scratch[wave] = (int)incl;
  __syncthreads();
  uint32_t before = incl - v, all = 0;
  for (int k = 0; k < PNG_THREADS / 64; ++k) {
    if (k < wave) before += (uint32_t)scratch[k];
    all += (uint32_t)scratch[k];
  }
  __syncthreads();
  *total = all;
  return before;
}

// ---- stage A: filtering ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int png_predict(int t, int a, int b, int c) {
  return t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
}

__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(const uint8_t* __restrict__ frame, int64_t n /* W * C */, int bpp, int filter,
                                                                 uint8_t* __restrict__ filtered) {
  __shared__ uint32_t cost[5];
  const int tid = threadIdx.x, y = blockIdx.x;
  const uint8_t* row = frame + (int64_t)y * n;
  const uint8_t* up = y > 0 ? row - n : row;  // (read only when y > 0)
  int type = filter;
  if (filter == UMHS_PNG_FILTER_ADAPTIVE) {
    if (tid < 5) cost[tid] = 0;
    __syncthreads();
    uint32_t s[5] = {0, 0, 0, 0, 0};
#pragma unroll 4
    for (int64_t i = tid; i < n; i += PNG_THREADS) {
      const int x = row[i], a = i >= bpp ? row[i - bpp] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= bpp) ? up[i - bpp] : 0;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const uint32_t f = (uint32_t)(x - png_predict(t, a, b, c)) & 255u;
        s[t] += f < 256u - f ? f : 256u - f;
      }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      uint32_t v = s[t];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      if ((tid & 63) == 0) atomicAdd(&cost[t], v);
    }
    __syncthreads();
    type = 0;
    for (int t = 1; t < 5; ++t)
      if (cost[t] < cost[type]) type = t;  // (ties: the smallest type)
  }
  uint8_t* o = filtered + (int64_t)y * (n + 1);
  if (tid == 0) o[0] = (uint8_t)type;
#pragma unroll 4
  for (int64_t i = tid; i < n; i += PNG_THREADS) {
    const int x = row[i], a = i >= bpp ? row[i - bpp] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= bpp) ? up[i - bpp] : 0;
    o[1 + i] = (uint8_t)(x - png_predict(type, a, b, c));
  }
}

// ---- stage B: tokens ------------------------------------------------------------------------------------------------------------------
// (symbol, number of extra bits, their value) of a match length 3 .. 258
__device__ __forceinline__ void png_length_symbol(int length, int* sym, int* nextra, uint32_t* extra) {
  if (length <= 10) {
    *sym = 254 + length, *nextra = 0, *extra = 0;
  } else if (length == PNG_RUN) {
    *sym = 285, *nextra = 0, *extra = 0;
  } else {
    const int x = length - 3, e = 29 - __clz(x);  // x = 8 .. 254: e = floor(log2 x) - 2
    *sym = 265 + 4 * (e - 1) + ((x >> e) & 3), *nextra = e, *extra = (uint32_t)x & ((1u << e) - 1u);
  }
}

struct png_tile {
  uint32_t heads;  // bit k: byte k of this thread's segment is a run head (or lies behind the piece's end)
  int before;      // the last head before the segment, in tile coordinates (below 0: as far back as the carried phase says)
  int behind;      // the first head behind the segment (PNG_TILE: none in sight, which is farther than any match reaches)
  int limit;       // tokens are emitted for tile positions below it
};

// Loads tile bytes [tile_off - 1, tile_off + PNG_TILE) of the piece into buf[0 .. PNG_TILE] and works out this thread's png_tile.
// *phase: the phase the tile's first byte has if it is no head; replaced by the next tile's.
__device__ __forceinline__ png_tile png_load_tile(const uint8_t* __restrict__ src, int64_t n, int64_t tile_off, uint8_t* buf, int* phase,
                                                  int* scratch, int tid) {
  {  // (all of a thread's loads are issued before the first is waited for: one memory latency per tile, not seventeen)
    uint8_t v[PNG_SEG];
#pragma unroll
    for (int j = 0; j < PNG_SEG; ++j) {
      const int64_t pos = tile_off - 1 + tid + j * PNG_THREADS;
      v[j] = (pos >= 0 && pos < n) ? src[pos] : 0;
    }
    const int64_t end = tile_off - 1 + PNG_TILE;
    const uint8_t tail = (tid == 0 && end < n) ? src[end] : 0;
#pragma unroll
    for (int j = 0; j < PNG_SEG; ++j) buf[tid + j * PNG_THREADS] = v[j];
    if (tid == 0) buf[PNG_TILE] = tail;
  }
  __syncthreads();
  png_tile t;
  t.heads = 0;
  const int q0 = tid * PNG_SEG;
  int last = INT32_MIN, first = PNG_TILE;
#pragma unroll
  for (int k = 0; k < PNG_SEG; ++k) {
    const int64_t pos = tile_off + q0 + k;
    const bool head = pos == 0 || pos >= n || buf[1 + q0 + k] != buf[q0 + k];
    if (head) {
      t.heads |= 1u << k;
      last = q0 + k;
      if (first == PNG_TILE) first = q0 + k;
    }
  }
  const int seed = -1 - *phase;
  t.before = png_scan_max_before(last, seed, scratch, tid);  // (its barriers: every thread has read *phase)
  t.behind = png_scan_min_behind(first, PNG_TILE, scratch, tid);
  const int64_t left = n - tile_off;
  t.limit = left < PNG_MAIN ? (int)left : PNG_MAIN;
  if (tid == PNG_MAIN / PNG_SEG) *phase = (PNG_MAIN - t.before - 1) % PNG_RUN;
  return t;
}

// THE token rule.  A head is a literal.  A byte j bytes behind the first byte after its head (j = 0, 1, ..), with j = 258 q + phase:
// at phase 0, r = the equal bytes from here on (itself included), at most 258: a match of r when r >= 3, else a literal; at phase 1
// a literal when the run ends with it (r was 2); otherwise it is inside a match.  literal(byte), match(length).
template <class L, class M>
__device__ __forceinline__ void png_tokens(const uint8_t* buf, const png_tile& t, int tid, L&& literal, M&& match) {
  const int q0 = tid * PNG_SEG;
  int s = t.before;
#pragma unroll
  for (int k = 0; k < PNG_SEG; ++k) {
    const int q = q0 + k;
    if (q >= t.limit) break;
    const int byte = buf[1 + q];
    if ((t.heads >> k) & 1u) {
      s = q;
      literal(byte);
      continue;
    }
    const int phase = (q - s - 1) % PNG_RUN;
    if (phase > 1) continue;
    const uint32_t above = t.heads >> (k + 1);
    const int next = above ? q + 1 + (__ffs(above) - 1) : t.behind;
    if (phase == 0) {
      const int r = next - q < PNG_RUN ? next - q : PNG_RUN;
      if (r >= 3) match(r); else literal(byte);
    } else if (next == q + 1) {
      literal(byte);
    }
  }
}

// ---- stage B: statistics and the code of a piece --------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_THREADS) void png_stats_kernel(const uint8_t* __restrict__ filtered, int64_t row_bytes, int height, int stripe_rows,
                                                                png_piece* __restrict__ pieces, uint32_t* __restrict__ tables) {
  __shared__ uint8_t buf[PNG_TILE + 16];
  __shared__ uint32_t hist[PNG_SYMS], leaf_w[PNG_SYMS], node_w[PNG_SYMS], level[PNG_MAX_BITS + 2], next_code[PNG_MAX_BITS + 2];
  __shared__ uint16_t sorted[PNG_SYMS], leaf_parent[PNG_SYMS], node_parent[PNG_SYMS], node_depth[PNG_SYMS];
  __shared__ uint8_t len[PNG_SYMS];
  __shared__ int scratch[4], phase, n_used, n_lit;
  __shared__ uint32_t tile_s1, adler_a, adler_b;
  __shared__ unsigned long long tile_s2, bits;
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x, r0 = p * stripe_rows;
  const int64_t rows = r0 + stripe_rows < height ? stripe_rows : height - r0;
  const int64_t n = rows * row_bytes;
  const uint8_t* src = filtered + r0 * row_bytes;
  for (int s = tid; s < PNG_SYMS; s += PNG_THREADS) hist[s] = 0, len[s] = 0;
  if (tid < PNG_MAX_BITS + 2) level[tid] = 0;
  if (tid == 0) phase = 0, n_used = 0, n_lit = 0, tile_s1 = 0, adler_a = 0, adler_b = 0, tile_s2 = 0, bits = 0;
  __syncthreads();

  uint32_t extra_bits = 0;  // this thread's extra and distance bits (a piece is below 2^31 bytes)
  for (int64_t tile_off = 0; tile_off < n; tile_off += PNG_MAIN) {
    const png_tile t = png_load_tile(src, n, tile_off, buf, &phase, scratch, tid);
    png_tokens(
        buf, t, tid, [&](int byte) { atomicAdd(&hist[byte], 1u); },
        [&](int length) {
          int sym, ne;
          uint32_t ev;
          png_length_symbol(length, &sym, &ne, &ev);
          atomicAdd(&hist[sym], 1u);
          extra_bits += (uint32_t)ne + 1u;
        });
    uint32_t s1 = 0, s2 = 0;  // Adler-32 of the tile: sum of d, sum of (limit - q) d
    for (int k = 0; k < PNG_SEG; ++k) {
      const int q = tid * PNG_SEG + k;
      if (q < t.limit) s1 += buf[1 + q], s2 += (uint32_t)(t.limit - q) * buf[1 + q];
    }
    atomicAdd(&tile_s1, s1);
    atomicAdd(&tile_s2, (unsigned long long)s2);
    __syncthreads();
    if (tid == 0) {  // (every operand below 2^32 after its reduction: 64-bit sums cannot overflow)
      adler_b = (uint32_t)((adler_b + (unsigned long long)t.limit * adler_a + tile_s2) % PNG_ADLER);
      adler_a = (adler_a + tile_s1) % PNG_ADLER;
      tile_s1 = 0, tile_s2 = 0;
    }
    __syncthreads();  // (buf and the sums are written again by the next tile)
  }
  if (tid == 0) hist[PNG_EOB] += 1;
  atomicAdd(&bits, (unsigned long long)extra_bits);
  __syncthreads();

  // the used symbols sorted by (count, symbol): every symbol counts the ones in front of it
  for (int s = tid; s < PNG_SYMS; s += PNG_THREADS) {
    const uint32_t c = hist[s];
    if (c == 0) continue;
    int rank = 0;
    for (int u = 0; u < PNG_SYMS; ++u) {
      const uint32_t cu = hist[u];
      rank += cu != 0 && (cu < c || (cu == c && u < s));
    }
    sorted[rank] = (uint16_t)s, leaf_w[rank] = c;
    atomicAdd(&n_used, 1);
    atomicMax(&n_lit, s + 1);
  }
  __syncthreads();
  const int nu = n_used;  // >= 2: a literal and the end of block
  if (tid == 0) {
    // two-queue merge: the leaves in sorted order, the merged nodes in the order they were made; the lighter head goes first, the leaf
    // when both weigh the same
    int li = 0, ii = 0;
    for (int k = 0; k < nu - 1; ++k) {
      uint32_t w = 0;
      for (int j = 0; j < 2; ++j) {
        if (li < nu && (ii >= k || leaf_w[li] <= node_w[ii])) {
          w += leaf_w[li], leaf_parent[li++] = (uint16_t)k;
        } else {
          w += node_w[ii], node_parent[ii++] = (uint16_t)k;
        }
      }
      node_w[k] = w;
    }
    node_depth[nu - 2] = 0;
    for (int k = nu - 3; k >= 0; --k) node_depth[k] = node_depth[node_parent[k]] + 1;
  }
  __syncthreads();
  for (int i = tid; i < nu; i += PNG_THREADS) {
    const int d = node_depth[leaf_parent[i]] + 1;
    atomicAdd(&level[d < PNG_MAX_BITS ? d : PNG_MAX_BITS], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    // Kraft sum in units of 2^-15 against 2^15: above it, a leaf of the deepest level above the last moves a level down; below it,
    // a leaf of the last level moves a level up
    int kraft = -(1 << PNG_MAX_BITS);
    for (int l = 1; l <= PNG_MAX_BITS; ++l) kraft += (int)level[l] << (PNG_MAX_BITS - l);
    while (kraft > 0) {
      int l = PNG_MAX_BITS - 1;
      while (level[l] == 0) --l;
      level[l] -= 1, level[l + 1] += 1, kraft -= 1 << (PNG_MAX_BITS - l - 1);
    }
    while (kraft < 0) level[PNG_MAX_BITS] -= 1, level[PNG_MAX_BITS - 1] += 1, kraft += 1;
    uint32_t code = 0;
    level[0] = 0;
    for (int l = 1; l <= PNG_MAX_BITS; ++l) {
      code = (code + level[l - 1]) << 1;
      next_code[l] = code;
    }
  }
  __syncthreads();
  for (int i = tid; i < nu; i += PNG_THREADS) {  // the sorted symbols take the levels from the deepest
    int l = PNG_MAX_BITS;
    uint32_t first = 0;
    while (l > 1 && (uint32_t)i >= first + level[l]) first += level[l--];
    len[sorted[i]] = (uint8_t)l;
  }
  __syncthreads();
  unsigned long long mine = 0;
  for (int s = tid; s < PNG_TABLE_WORDS; s += PNG_THREADS) {
    uint32_t entry = 0;
    if (s < PNG_SYMS && len[s]) {
      const int l = len[s];
      uint32_t code = next_code[l];
      for (int u = 0; u < s; ++u) code += len[u] == l;
      entry = ((__brev(code) >> (32 - l)) << 8) | (uint32_t)l;
      mine += (unsigned long long)hist[s] * l;
    }
    tables[p * PNG_TABLE_WORDS + s] = entry;
  }
  atomicAdd(&bits, mine);
  __syncthreads();
  if (tid == 0) {
    const unsigned long long all = bits + PNG_HEADER_BITS + 4ull * (n_lit + 1) + 3ull;
    png_piece rec;
    rec.bytes = (all + 7) / 8 + 4, rec.offset = 0, rec.s1 = adler_a, rec.s2 = adler_b, rec.nlit = (uint32_t)n_lit, rec.pad = 0;
    pieces[p] = rec;
  }
}

// ---- the container --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void png_put8(uint8_t* out, int64_t capacity, int64_t pos, uint32_t v) {
  if (pos < capacity) out[pos] = (uint8_t)v;
}
__device__ __forceinline__ void png_put32(uint8_t* out, int64_t capacity, int64_t pos, uint32_t v) {  // big-endian
  for (int k = 0; k < 4; ++k) png_put8(out, capacity, pos + k, v >> (24 - 8 * k));
}

// byte counts -> offsets; everything of the file that is not deflate data or an IDAT's CRC; the length of the file
__global__ __launch_bounds__(PNG_THREADS) void png_scan_kernel(png_header header, png_piece* __restrict__ pieces, int64_t n_pieces, int64_t row_bytes,
                                                               int height, int stripe_rows, uint8_t* __restrict__ out, int64_t capacity,
                                                               int64_t* __restrict__ length) {
  __shared__ unsigned long long wave_total[PNG_THREADS / 64], sum_a, sum_b;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t total = row_bytes * height;
  if (tid == 0) sum_a = 0, sum_b = 0;
  unsigned long long carry = 33, a = 0, b = 0;
  for (int64_t base = 0; base < n_pieces; base += PNG_THREADS) {
    const int64_t i = base + tid;
    const bool live = i < n_pieces;
    unsigned long long data = 0;  // the chunk's data bytes
    if (live) data = pieces[i].bytes + (i == 0 ? 2 : 0) + (i == n_pieces - 1 ? 6 : 0);
    const unsigned long long v = live ? data + 12 : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int k = 0; k < PNG_THREADS / 64; ++k) {
      if (k < wave) before += wave_total[k];
      all += wave_total[k];
    }
    if (live) {
      const int64_t at = (int64_t)(carry + before + incl - v);
      png_put32(out, capacity, at, (uint32_t)data);
      png_put32(out, capacity, at + 4, 0x49444154u);  // IDAT
      int64_t start = at + 8;
      if (i == 0) png_put8(out, capacity, start, 0x78), png_put8(out, capacity, start + 1, 0x01), start += 2;
      pieces[i].offset = (uint64_t)start;
      // Adler-32 of the whole: a = 1 + sum of s1; b = total + sum of (s2 + (bytes behind the piece) * s1), all modulo 65521
      const int64_t end_row = (i + 1) * stripe_rows < height ? (i + 1) * stripe_rows : height;
      const unsigned long long behind = (unsigned long long)(total - end_row * row_bytes) % PNG_ADLER;
      a = (a + pieces[i].s1) % PNG_ADLER;
      b = (b + pieces[i].s2 + behind * pieces[i].s1) % PNG_ADLER;
    }
    carry += all;
    __syncthreads();
  }
  atomicAdd(&sum_a, a);
  atomicAdd(&sum_b, b);
  __syncthreads();
  if (tid == 0) {
    const uint32_t fa = (uint32_t)((1 + sum_a) % PNG_ADLER), fb = (uint32_t)(((unsigned long long)total % PNG_ADLER + sum_b) % PNG_ADLER);
    int64_t at = (int64_t)carry - 10;  // behind the last piece's deflate bytes: the final block, the Adler-32 (then that chunk's CRC)
    png_put8(out, capacity, at, 0x03), png_put8(out, capacity, at + 1, 0x00);
    png_put32(out, capacity, at + 2, (fb << 16) | fa);
    at = (int64_t)carry;
    png_put32(out, capacity, at, 0u), png_put32(out, capacity, at + 4, 0x49454E44u), png_put32(out, capacity, at + 8, 0xAE426082u);  // IEND
    *length = at + 12;
  }
  for (int k = tid; k < 33; k += PNG_THREADS) png_put8(out, capacity, k, header.b[k]);
}

// ---- stage B: writing -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void png_or_bits(uint32_t* img, uint32_t pos, uint32_t v, int n) {  // n <= 21 bits of v at bit `pos`, LSB first
  const uint32_t w = pos >> 5, sh = pos & 31u;
  atomicOr(&img[w], v << sh);
  if (sh + (uint32_t)n > 32u) atomicOr(&img[w + 1], v >> (32u - sh));
}

__global__ __launch_bounds__(PNG_THREADS) void png_write_kernel(const uint8_t* __restrict__ filtered, int64_t row_bytes, int height, int stripe_rows,
                                                                const png_piece* __restrict__ pieces, const uint32_t* __restrict__ tables,
                                                                uint8_t* __restrict__ out, int64_t capacity) {
  __shared__ uint8_t buf[PNG_TILE + 16];
  __shared__ uint32_t img[PNG_IMG_WORDS], table[PNG_TABLE_WORDS];
  __shared__ int scratch[4], phase;
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x, r0 = p * stripe_rows;
  const int64_t rows = r0 + stripe_rows < height ? stripe_rows : height - r0;
  const int64_t n = rows * row_bytes;
  const uint8_t* src = filtered + r0 * row_bytes;
  const png_piece rec = pieces[p];
  const int nlit = (int)rec.nlit;
  for (int s = tid; s < PNG_TABLE_WORDS; s += PNG_THREADS) table[s] = tables[p * PNG_TABLE_WORDS + s];
  for (int w = tid; w < PNG_IMG_WORDS; w += PNG_THREADS) img[w] = 0;
  if (tid == 0) phase = 0;
  // the image's bit 0 is the first bit of the aligned word that holds the piece's first byte; bytes of [lo, hi) are this piece's to write
  const uintptr_t lo = (uintptr_t)out + rec.offset;
  const uintptr_t piece_end = lo + rec.bytes, cap_end = (uintptr_t)out + (uintptr_t)capacity;
  const uintptr_t hi = piece_end < cap_end ? piece_end : cap_end;
  uintptr_t word = lo & ~(uintptr_t)3;  // address of img[0]
  uint32_t have = (uint32_t)(lo & 3) * 8;  // bits of the image in front of what comes next
  // the image's first n_bits leave: every complete word (all of them when `final`); the rest is carried to the front of the next image
  auto flush = [&](uint32_t n_bits, bool final) {
    __syncthreads();
    const uint32_t words = final ? (n_bits + 31) >> 5 : n_bits >> 5;
    for (uint32_t w = tid; w < words; w += PNG_THREADS) {
      const uint32_t v = img[w];
      const uintptr_t at = word + 4 * (uintptr_t)w;
      if (at >= lo && at + 4 <= hi) {
        *reinterpret_cast<uint32_t*>(at) = v;
      } else {
        for (int k = 0; k < 4; ++k)
          if (at + k >= lo && at + k < hi) *reinterpret_cast<uint8_t*>(at + k) = (uint8_t)(v >> (8 * k));
      }
    }
    const uint32_t rest = final ? 0u : img[words];
    __syncthreads();
    for (uint32_t w = tid; w <= words; w += PNG_THREADS) img[w] = w == 0 ? rest : 0u;
    word += 4 * (uintptr_t)words, have = final ? 0u : n_bits & 31u;
    __syncthreads();
  };
  __syncthreads();

  // the block header: BFINAL 0, BTYPE 2, HLIT, HDIST 0, HCLEN 15; the code-length code: 16 17 18 unused, 0 .. 15 four bits each; the
  // literal/length code lengths and the distance tree's single length 1 under it (a 4-bit code is its symbol, MSB first)
  if (tid == 0) png_or_bits(img, have, 4u | ((uint32_t)(nlit - 257) << 3) | (15u << 13), 17);
  if (tid < 19) png_or_bits(img, have + 17 + 3 * tid, tid < 3 ? 0u : 4u, 3);
  for (int s = tid; s <= nlit; s += PNG_THREADS) {
    const uint32_t l = s < nlit ? table[s] & 255u : 1u;
    png_or_bits(img, have + PNG_HEADER_BITS + 4 * s, __brev(l) >> 28, 4);
  }
  flush(have + PNG_HEADER_BITS + 4 * (uint32_t)(nlit + 1), false);

  for (int64_t tile_off = 0; tile_off < n; tile_off += PNG_MAIN) {
    const png_tile t = png_load_tile(src, n, tile_off, buf, &phase, scratch, tid);
    uint32_t mine = 0;
    png_tokens(
        buf, t, tid, [&](int byte) { mine += table[byte] & 255u; },
        [&](int length) {
          int sym, ne;
          uint32_t ev;
          png_length_symbol(length, &sym, &ne, &ev);
          mine += (table[sym] & 255u) + (uint32_t)ne + 1u;
        });
    uint32_t total;
    uint32_t at = have + png_scan_sum_before(mine, &total, scratch, tid);
    png_tokens(
        buf, t, tid,
        [&](int byte) {
          const uint32_t e = table[byte];
          png_or_bits(img, at, e >> 8, (int)(e & 255u));
          at += e & 255u;
        },
        [&](int length) {
          int sym, ne;
          uint32_t ev;
          png_length_symbol(length, &sym, &ne, &ev);
          const uint32_t e = table[sym], l = e & 255u;
          png_or_bits(img, at, (e >> 8) | (ev << l), (int)l + ne + 1);  // (the distance code is one 0 bit)
          at += l + (uint32_t)ne + 1u;
        });
    flush(have + total, false);  // (its barriers: buf may be loaded again)
  }

  // end of block; the empty stored block: 000, zeros to the byte, 00 00 FF FF
  uint32_t n_bits = have + (table[PNG_EOB] & 255u) + 3u;
  n_bits = (n_bits + 7u) & ~7u;
  if (tid == 0) {
    png_or_bits(img, have, table[PNG_EOB] >> 8, (int)(table[PNG_EOB] & 255u));
    png_or_bits(img, n_bits + 16, 0xFFFFu, 16);
  }
  flush(n_bits + 32, true);
}

// ---- CRC-32 of the IDAT chunks --------------------------------------------------------------------------------------------------------
// a, b: polynomials over GF(2), bit 31 the coefficient of x^0 (the reflected form the CRC register is in) -> a b mod P
__device__ __forceinline__ uint32_t png_gf_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) r ^= b;
    b = (b >> 1) ^ ((b & 1u) ? PNG_CRC_POLY : 0u);
  }
  return r;
}

__device__ __forceinline__ uint32_t png_x_pow_8n(uint64_t n) {  // x^(8 n) mod P
  uint32_t r = 0x80000000u, base = 0x00800000u;
  for (; n; n >>= 1) {
    if (n & 1) r = png_gf_mul(r, base);
    base = png_gf_mul(base, base);
  }
  return r;
}

__global__ __launch_bounds__(PNG_THREADS) void png_crc_kernel(const png_piece* __restrict__ pieces, int64_t n_pieces, uint8_t* __restrict__ out,
                                                              int64_t capacity) {
  __shared__ uint32_t crc_table[256], wave_x[PNG_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x;
  {
    uint32_t c = (uint32_t)tid;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? PNG_CRC_POLY : 0u);
    crc_table[tid] = c;
  }
  __syncthreads();
  const int64_t start = (int64_t)pieces[p].offset - (p == 0 ? 2 : 0);  // the chunk's data
  const int64_t len = (int64_t)pieces[p].bytes + (p == 0 ? 2 : 0) + (p == n_pieces - 1 ? 6 : 0);
  // register(0xFFFFFFFF, type . data) = register(0xFFFFFFFF, type) x^(8 len) + sum over the slices of register(0, slice) x^(8 bytes behind it)
  const int64_t per = (len + PNG_THREADS - 1) / PNG_THREADS;
  const int64_t a = tid * per < len ? tid * per : len, b = a + per < len ? a + per : len;
  uint32_t c = 0;
  for (int64_t i = a; i < b; ++i) {
    const uint32_t byte = start + i < capacity ? out[start + i] : 0u;  // (past the capacity the file is cut short anyway)
    c = crc_table[(c ^ byte) & 255u] ^ (c >> 8);
  }
  uint32_t x = b > a ? png_gf_mul(c, png_x_pow_8n((uint64_t)(len - b))) : 0u;
  if (tid == 0) {
    uint32_t s = 0xFFFFFFFFu;
    const uint32_t type = 0x49444154u;  // IDAT
    for (int k = 0; k < 4; ++k) s = crc_table[(s ^ (type >> (24 - 8 * k))) & 255u] ^ (s >> 8);
    x ^= png_gf_mul(s, png_x_pow_8n((uint64_t)len));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x ^= __shfl_xor(x, d, 64);
  if ((tid & 63) == 0) wave_x[tid >> 6] = x;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < PNG_THREADS / 64; ++k) x ^= wave_x[k];
    png_put32(out, capacity, start + len, ~x);
  }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t umhs_png_workspace_bytes(int height, int width, int channels, int stripe_rows) {
  png_geometry g;
  if (png_geometry_of(height, width, channels, stripe_rows, &g) != UMHS_OK) return 0;
  return png_filtered_bytes(g) + png_piece_bytes(g);
}

extern "C" size_t umhs_png_max_bytes(int height, int width, int channels, int stripe_rows) {
  png_geometry g;
  if (png_geometry_of(height, width, channels, stripe_rows, &g) != UMHS_OK) return 0;
  // signature and IHDR; per piece the chunk's 12 bytes and png_piece_max; the zlib header, the final block, the Adler-32; IEND
  const int64_t full = height / stripe_rows, rest = height % stripe_rows;
  int64_t bytes = 33 + full * (12 + png_piece_max(stripe_rows * g.row_bytes)) + 2 + 6 + 12;
  if (rest) bytes += 12 + png_piece_max(rest * g.row_bytes);
  return (size_t)bytes;
}

extern "C" int umhs_png_filter(const uint8_t* frame, int height, int width, int channels, int filter, uint8_t* filtered, umhs_stream_t stream) {
  png_geometry g;
  const int rc = png_geometry_of(height, width, channels, 1, &g);
  if (rc != UMHS_OK) return rc;
  if (!frame || !filtered || filter < UMHS_PNG_FILTER_NONE || filter > UMHS_PNG_FILTER_ADAPTIVE) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)height), dim3(PNG_THREADS), 0, umhs_s(stream), frame, g.row_bytes - 1, g.bpp, filter,
                     filtered);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_png_deflate(const uint8_t* filtered, int height, int width, int channels, int stripe_rows, uint8_t* out, int64_t capacity,
                                int64_t* length, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  png_geometry g;
  const int rc = png_geometry_of(height, width, channels, stripe_rows, &g);
  if (rc != UMHS_OK) return rc;
  if (!filtered || !out || capacity < 0 || !length || ((uintptr_t)length & 7)) return UMHS_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < png_piece_bytes(g)) return UMHS_ERR_WORKSPACE;
  png_header header;
  png_build_header(height, width, channels, &header);
  png_piece* pieces = static_cast<png_piece*>(workspace);
  uint32_t* tables = reinterpret_cast<uint32_t*>(pieces + g.n_pieces);
  const dim3 grid((unsigned)g.n_pieces), block(PNG_THREADS);
  hipLaunchKernelGGL(png_stats_kernel, grid, block, 0, umhs_s(stream), filtered, g.row_bytes, height, stripe_rows, pieces, tables);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(png_scan_kernel, dim3(1), block, 0, umhs_s(stream), header, pieces, g.n_pieces, g.row_bytes, height, stripe_rows, out,
                     capacity, length);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(png_write_kernel, grid, block, 0, umhs_s(stream), filtered, g.row_bytes, height, stripe_rows, pieces, tables, out, capacity);
  UMHS_CHECK_LAUNCH();
  hipLaunchKernelGGL(png_crc_kernel, grid, block, 0, umhs_s(stream), pieces, g.n_pieces, out, capacity);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

extern "C" int umhs_png_encode(const uint8_t* frame, int height, int width, int channels, int filter, int stripe_rows, uint8_t* out,
                               int64_t capacity, int64_t* length, void* workspace, size_t workspace_bytes, umhs_stream_t stream) {
  png_geometry g;
  int rc = png_geometry_of(height, width, channels, stripe_rows, &g);
  if (rc != UMHS_OK) return rc;
  if (!frame || !out || capacity < 0 || !length || ((uintptr_t)length & 7) || filter < UMHS_PNG_FILTER_NONE || filter > UMHS_PNG_FILTER_ADAPTIVE)
    return UMHS_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < png_filtered_bytes(g) + png_piece_bytes(g)) return UMHS_ERR_WORKSPACE;
  uint8_t* filtered = static_cast<uint8_t*>(workspace);
  rc = umhs_png_filter(frame, height, width, channels, filter, filtered, stream);
  if (rc != UMHS_OK) return rc;
  return umhs_png_deflate(filtered, height, width, channels, stripe_rows, out, capacity, length, filtered + png_filtered_bytes(g),
                          png_piece_bytes(g), stream);
}
