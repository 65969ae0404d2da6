"""The baseline-JPEG frame format of ``umhs_jpeg_*`` (include/umhs_hip.h) restated once, on the host: the tables, the float32 transform
in numpy with the header's operation order (every numpy float32 operation is one rounded operation), the same transform in float64, a
pure-Python entropy coder with restart intervals and 0xFF stuffing, the header writer and a small RIFF reader.  Not a test.

Layout of the coefficients (what ``umhs_jpeg_coefficients`` writes): int16 [n_mcus, blocks_per_mcu, 64], MCUs in raster order, the
blocks of an MCU in scan order -- 4:4:4: Y, Cb, Cr; 4:2:0: Y(0,0), Y(0,1), Y(1,0), Y(1,1), Cb, Cr -- and the 64 values in zigzag order.

The float64 section derives the bound on |F32 - F64| from the operation count of the definition (``f64_bound``)."""
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])  # natural index (8 * u + v, u the vertical frequency) of each zigzag position
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                      87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                        99, 99, 99, 99] + [99] * 32)
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = list(bytes.fromhex(
    "00010203110405213106124151076171132232810814" "4291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344454647"
    "48494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
    "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
S444, S420 = "444", "420"
HEADER_BYTES = 629


def quant_tables(quality):
    """libjpeg's scaling of the Annex-K tables -> (luma, chroma), natural order, each entry 1..255."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255).astype(np.int64) for base in (BASE_LUMA, BASE_CHROMA))


def huff_codes(bits, vals):
    """Annex C: symbol -> (code, length)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def dct_matrix(dtype):
    """T[u][x] = 1/2 c(u) cos((2x + 1) u pi / 16), computed in float64 and rounded to ``dtype``."""
    u, x = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
    c = np.where(u == 0, 1.0 / np.sqrt(2.0), 1.0)
    return (0.5 * c * np.cos((2 * x + 1) * u * np.pi / 16)).astype(dtype)


def mcu_grid(H, W, subsampling):
    """-> (MCU rows, MCU columns, MCU size in pixels, blocks per MCU)."""
    m = 16 if subsampling == S420 else 8
    return (H + m - 1) // m, (W + m - 1) // m, m, 6 if subsampling == S420 else 3


def _planes(frame, subsampling, dtype):
    H, W, _ = frame.shape
    my, mx, m, _ = mcu_grid(H, W, subsampling)
    yy, xx = np.minimum(np.arange(my * m), H - 1), np.minimum(np.arange(mx * m), W - 1)
    px = frame[yy][:, xx].astype(dtype)  # a pixel outside the frame reads (min(y, H - 1), min(x, W - 1))
    R, G, B = px[..., 0], px[..., 1], px[..., 2]
    c = lambda v: dtype(v)
    Y = ((c(0.299) * R + c(0.587) * G) + c(0.114) * B) - c(128)
    Cb = ((c(-0.168736) * R) + (c(-0.331264) * G)) + c(0.5) * B
    Cr = (c(0.5) * R + (c(-0.418688) * G)) + (c(-0.081312) * B)
    if subsampling == S420:
        down = lambda p: ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])) * c(0.25)
        Cb, Cr = down(Cb), down(Cr)
    return Y, Cb, Cr


def _dct(plane, dtype):
    """[h, w] -> F [h / 8, w / 8, 8 (u), 8 (v)], both passes summed in ascending index from the first product."""
    T = dct_matrix(dtype)
    f = plane.reshape(plane.shape[0] // 8, 8, plane.shape[1] // 8, 8).transpose(0, 2, 1, 3)  # [by, bx, y, x]
    G = None
    for x in range(8):  # G[y][v] = sum_x f[y][x] T[v][x]
        term = f[..., :, x, None] * T[None, :, x]
        G = term if G is None else G + term
    F = None
    for y in range(8):  # F[u][v] = sum_y T[u][y] G[y][v]
        term = T[:, y, None] * G[..., y, None, :]
        F = term if F is None else F + term
    assert F.dtype == dtype
    return F


def _quantise(F, Q, dtype):
    """-> (k int16 [by, bx, 64] zigzag, v = F / Q [by, bx, 64] zigzag)."""
    v = F.reshape(*F.shape[:2], 64) / Q.astype(dtype)
    k = np.sign(v) * np.trunc(np.abs(v) + dtype(0.5))
    k[..., 1:] = np.clip(k[..., 1:], -1023, 1023)
    k[..., 0] = np.clip(k[..., 0], -1024, 1023)
    return k[..., ZIGZAG].astype(np.int16), v[..., ZIGZAG]


def coefficients(frame, quality, subsampling, dtype=np.float32, with_v=False):
    """The transform stage: uint8 [H, W, 3] -> int16 [n_mcus, blocks_per_mcu, 64] (module docstring); ``with_v``: also v = F / Q in the
    same layout, in ``dtype``."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    my, mx, _, bpm = mcu_grid(frame.shape[0], frame.shape[1], subsampling)
    ql, qc = quant_tables(quality)
    Y, Cb, Cr = _planes(frame, subsampling, dtype)
    ky, vy = _quantise(_dct(Y, dtype), ql, dtype)
    kb, vb = _quantise(_dct(Cb, dtype), qc, dtype)
    kr, vr = _quantise(_dct(Cr, dtype), qc, dtype)

    def lay(y, b, r):
        if subsampling == S420:  # [2 my, 2 mx, 64] -> [my, mx, 4, 64], the four Y blocks of an MCU in raster order
            y = y.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        else:
            y = y[:, :, None, :]
        return np.concatenate([y, b[:, :, None, :], r[:, :, None, :]], axis=2).reshape(my * mx, bpm, 64)

    k = lay(ky, kb, kr)
    return (k, lay(vy, vb, vr)) if with_v else k


def divisors(quality, subsampling):
    """Q of every coefficient of one MCU, [blocks_per_mcu, 64] in zigzag order."""
    ql, qc = quant_tables(quality)
    n_y = 4 if subsampling == S420 else 1
    return np.stack([ql[ZIGZAG]] * n_y + [qc[ZIGZAG]] * 2).astype(np.float64)


# ---- float64 comparison: the bound on |F32 - F64| ------------------------------------------------------------------------------------
U32 = 2.0 ** -24  # unit roundoff of float32


def f64_bound(subsampling):
    """Bound on |F32 - F64| for one DCT coefficient of 8-bit input, from the operation count of the definition (u = 2^-24; the float64
    evaluation's own error, of the order 1e-13, and terms of order u^2 are covered by the final factor 1.01).

    Colour: every constant is rounded to float32 (relative u) and every product rounded again: 2 u |c| 255 per product, and the |c| of
    one component sum to 1 (Y: .299 + .587 + .114; Cb and Cr: .5 + .5): 510 u.  Two additions whose results are at most 255 in
    magnitude: 255 u each.  The level shift (Y only; taken for all): a result of at most 128: 128 u.  So df = 1148 u.
    4:2:0 chroma: the mean of four values carries at most their error; (a + b) and (c + d) are at most 256: 256 u each; their sum at
    most 512: 512 u; times 0.25 (exact): 256 u more.
    A pass of the DCT is a dot product of 8 terms with a rounded constant: its error is at most S (error of its inputs) +
    (gamma_8 + u) S (bound of its inputs), gamma_8 = 8 u / (1 - 8 u), S = max_v sum_x |T[v][x]| (= 2 sqrt 2).  The inputs of the row
    pass are at most 128, those of the column pass at most 128 S."""
    S = float(np.abs(dct_matrix(np.float64)).sum(axis=1).max())
    g8 = 8 * U32 / (1 - 8 * U32)
    df = 1148 * U32 + (256 * U32 if subsampling == S420 else 0.0)
    dG = S * df + (g8 + U32) * S * 128.0
    dF = S * dG + (g8 + U32) * S * (128.0 * S)
    return 1.01 * dF


def tie_band(quality, subsampling):
    """[blocks_per_mcu, 64]: how far the float32 v = F / Q, and then |v| + 0.5, may lie from the float64 ones: the bound on F over Q,
    one rounding of the division (|v| <= 1024 / Q) and one of the sum (|v| + 0.5 <= 1024 / Q + 0.5)."""
    Q = divisors(quality, subsampling)
    return f64_bound(subsampling) / Q + 1.01 * U32 * (2 * 1024.0 / Q + 0.5)


def in_tie_band(v64, band):
    """Where the float64 v is within ``band`` of a rounding tie (|v| = n + 1/2)."""
    a = np.abs(v64)
    return np.abs(a - np.floor(a) - 0.5) <= band


# ---- entropy coding --------------------------------------------------------------------------------------------------------------------
_DC = (huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS))
_AC = (huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def _category(v):
    return int(abs(v)).bit_length()


def _value_bits(v, size):
    return v if v >= 0 else v + (1 << size) - 1


def block_bits(block, pred, chroma):
    """-> (bits as an int, number of bits) of one block of 64 zigzag coefficients with DC predictor ``pred``."""
    acc = n = 0

    def put(code, length):
        nonlocal acc, n
        acc, n = (acc << length) | code, n + length

    diff = int(block[0]) - pred
    size = _category(diff)
    put(*_DC[chroma][size])
    if size:
        put(_value_bits(diff, size), size)
    run, ac = 0, _AC[chroma]
    for k in range(1, 64):
        c = int(block[k])
        if c == 0:
            run += 1
            continue
        while run > 15:
            put(*ac[0xF0])
            run -= 16
        size = _category(c)
        put(*ac[(run << 4) | size])
        put(_value_bits(c, size), size)
        run = 0
    if run:
        put(*ac[0x00])
    return acc, n


def interval_bits(coefs, first_mcu, last_mcu, subsampling):
    """-> (bits as an int, number of bits) of the MCUs [first, last) as one restart interval: DC predictors from 0, MSB first."""
    n_y = 4 if subsampling == S420 else 1
    pred, acc, n = [0, 0, 0], 0, 0
    for m in range(first_mcu, last_mcu):
        for j in range(n_y + 2):
            comp = 0 if j < n_y else j - n_y + 1
            bits, length = block_bits(coefs[m, j], pred[comp], comp > 0)
            pred[comp] = int(coefs[m, j, 0])
            acc, n = (acc << length) | bits, n + length
    return acc, n


def interval_bytes(coefs, first_mcu, last_mcu, subsampling, stuffed=True):
    """One restart interval: ``interval_bits``, the last byte padded with 1-bits, then 0xFF -> 0xFF 0x00."""
    acc, n = interval_bits(coefs, first_mcu, last_mcu, subsampling)
    pad = -n % 8
    acc, n = (acc << pad) | ((1 << pad) - 1), n + pad
    raw = acc.to_bytes(n // 8, "big")
    return raw.replace(b"\xff", b"\xff\x00") if stuffed else raw


def header(H, W, quality, subsampling, restart_mcus):
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i, q in enumerate((ql, qc)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(int(x) for x in q[ZIGZAG])
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, H, W, 3) + bytes([1, 0x22 if subsampling == S420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                              (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc_th) + bytes(bits) + bytes(vals)
    out += b"\xff\xdd" + struct.pack(">HH", 4, restart_mcus)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def intervals(coefs, subsampling, restart_mcus, stuffed=True):
    n = coefs.shape[0]
    return [interval_bytes(coefs, a, min(a + restart_mcus, n), subsampling, stuffed) for a in range(0, n, restart_mcus)]


def encode_coefficients(coefs, H, W, quality, subsampling, restart_mcus):
    """The whole file from coefficients: header, intervals with RSTm (m counts modulo 8) between them, EOI."""
    out = header(H, W, quality, subsampling, restart_mcus)
    parts = intervals(coefs, subsampling, restart_mcus)
    for i, p in enumerate(parts):
        out += p + (b"\xff\xd9" if i == len(parts) - 1 else bytes([0xFF, 0xD0 + i % 8]))
    return out


def encode(frame, quality, subsampling, restart_mcus):
    frame = np.asarray(frame)
    return encode_coefficients(coefficients(frame, quality, subsampling), frame.shape[0], frame.shape[1], quality, subsampling, restart_mcus)


# ---- RIFF reader -------------------------------------------------------------------------------------------------------------------------
def riff_chunks(data, begin=0, end=None):
    """[(fourcc, payload offset, size, children or None)] of the chunks in data[begin:end]; RIFF and LIST chunks carry their children
    (their list type is appended to the fourcc: ``LIST:movi``).  Chunks are padded to even sizes."""
    end, out, p = len(data) if end is None else end, [], begin
    while p + 8 <= end:
        cc, size = data[p:p + 4].decode("latin1"), struct.unpack("<I", data[p + 4:p + 8])[0]
        assert p + 8 + size <= end, f"chunk {cc} at {p} runs past its parent"
        if cc in ("RIFF", "LIST"):
            out.append((f"{cc}:{data[p + 8:p + 12].decode('latin1')}", p + 8, size, riff_chunks(data, p + 12, p + 8 + size)))
        else:
            out.append((cc, p + 8, size, None))
        p += 8 + size + (size & 1)
    assert p == end, f"{end - p} stray bytes after the last chunk"
    return out


def riff_find(chunks, name):
    for c in chunks:
        if c[0] == name:
            return c
        if c[3] is not None:
            hit = riff_find(c[3], name)
            if hit is not None:
                return hit
    return None
