"""The PNG stream of ``umhs_png_*`` (include/umhs_hip.h) restated once, on the host, in numpy and plain Python: the five filters and
the adaptive choice, the distance-1 tokens, the rule that turns a piece's histogram into code lengths, the bits of a piece, the
chunks of the file.  Checksums come from ``zlib`` (crc32, adler32), which the device encoder does not use.  Also a chunk parser that
checks every CRC.  Unfiltering is not restated: PIL is the decoder.  Not a test."""
import struct
import zlib

import numpy as np

FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
ZLIB_HEADER = b"\x78\x01"
MAX_BITS = 15
END_OF_BLOCK = 256
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- stage A -------------------------------------------------------------------------------------------------------------------------
def filter_candidates(frame):
    """uint8 [5, H, W * C]: the rows of ``frame`` [H, W, C] under None, Sub, Up, Average, Paeth (bpp = C; zeros left and above)."""
    H, W, C = frame.shape
    x = frame.reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, C:] = x[:-1, :-C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def filter_costs(candidates):
    """int64 [5, H]: sum over the row of min(f, 256 - f)."""
    f = candidates.astype(np.int64)
    return np.minimum(f, 256 - f).sum(axis=2)


def filter_rows(frame, filter="adaptive"):
    """uint8 [H, 1 + W * C]: every row's filter type and its filtered bytes.  ``adaptive``: the type of least cost, the smallest on ties."""
    frame = np.ascontiguousarray(frame)
    if frame.ndim == 2:
        frame = frame[..., None]
    cand = filter_candidates(frame)
    H = frame.shape[0]
    t = FILTERS[filter]
    types = np.argmin(filter_costs(cand), axis=0) if t == 5 else np.full(H, t)  # (argmin: the first of equal minima)
    out = np.empty((H, 1 + cand.shape[2]), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(H)]
    return out


# ---- stage B: tokens -----------------------------------------------------------------------------------------------------------------
def length_symbol(length):
    """(symbol, number of extra bits, extra value) of a match length 3..258."""
    if length <= 10:
        return 254 + length, 0, 0
    if length == 258:
        return 285, 0, 0
    x = length - 3
    e = x.bit_length() - 3
    return 265 + 4 * (e - 1) + ((x >> e) & 3), e, x & ((1 << e) - 1)


def tokens(piece):
    """The tokens of one piece (bytes): ('lit', byte) and ('len', length); every match has distance 1."""
    d = np.frombuffer(bytes(piece), np.uint8)
    heads = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    ends = np.concatenate([heads[1:], [len(d)]])
    out = []
    for h, n in zip(heads.tolist(), (ends - heads).tolist()):
        v = int(d[h])
        out.append(("lit", v))
        m = n - 1
        while m >= 3:
            k = min(m, 258)
            out.append(("len", k))
            m -= k
        out.extend([("lit", v)] * m)
    return out


def histogram(toks):
    h = [0] * 286
    for kind, v in toks:
        h[v if kind == "lit" else length_symbol(v)[0]] += 1
    h[END_OF_BLOCK] += 1
    return h


# ---- stage B: the length rule --------------------------------------------------------------------------------------------------------
def huffman_depth_counts(counts):
    """(symbols sorted by (count, symbol), leaves per UNLIMITED depth): the two-queue merge.  The leaves wait in sorted order, the merged
    nodes in the order they were made; each step takes the lighter of the two queue heads twice, the leaf when they weigh the same."""
    order = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    n = len(order)
    assert n >= 2
    lw = [counts[s] for s in order]
    iw, lparent, iparent = [], [0] * n, [0] * (n - 1)
    li = ii = 0
    for k in range(n - 1):
        w = 0
        for _ in range(2):
            if li < n and (ii >= len(iw) or lw[li] <= iw[ii]):
                w, lparent[li], li = w + lw[li], k, li + 1
            else:
                w, iparent[ii], ii = w + iw[ii], k, ii + 1
        iw.append(w)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[iparent[k]] + 1
    per_depth = {}
    for i in range(n):
        d = depth[lparent[i]] + 1
        per_depth[d] = per_depth.get(d, 0) + 1
    return order, per_depth


def code_lengths(counts):
    """Code length of every symbol (0: unused).  Leaves deeper than 15 are counted at 15; while the Kraft sum (in units of 2^-15) is
    above 2^15, one leaf of the deepest level above 15's that has one moves a level down; while it is below, one leaf of level 15
    moves a level up.  Then the sorted symbols take the levels from the deepest: the lightest symbols get the longest codes."""
    order, per_depth = huffman_depth_counts(counts)
    bl = [0] * (MAX_BITS + 1)
    for d, k in per_depth.items():
        bl[min(d, MAX_BITS)] += k
    kraft = sum(bl[l] << (MAX_BITS - l) for l in range(1, MAX_BITS + 1)) - (1 << MAX_BITS)
    while kraft > 0:
        l = max(l for l in range(1, MAX_BITS) if bl[l])
        bl[l], bl[l + 1], kraft = bl[l] - 1, bl[l + 1] + 1, kraft - (1 << (MAX_BITS - l - 1))
    while kraft < 0:
        bl[MAX_BITS], bl[MAX_BITS - 1], kraft = bl[MAX_BITS] - 1, bl[MAX_BITS - 1] + 1, kraft + 1
    lengths, r = [0] * len(counts), 0
    for l in range(MAX_BITS, 0, -1):
        for s in order[r:r + bl[l]]:
            lengths[s] = l
        r += bl[l]
    assert r == len(order) and sum(1 << (MAX_BITS - l) for l in lengths if l) == 1 << MAX_BITS
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2: symbol -> code (as an integer whose most significant bit goes out first)."""
    bl = [0] * (MAX_BITS + 2)
    for l in lengths:
        bl[l] += l > 0
    nxt, code = [0] * (MAX_BITS + 2), 0
    for l in range(1, MAX_BITS + 1):
        code = (code + bl[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s], nxt[l] = nxt[l], nxt[l] + 1
    return codes


# ---- stage B: bits -------------------------------------------------------------------------------------------------------------------
def _reverse(code, n):
    return int(format(code, f"0{n}b")[::-1], 2) if n else 0


def piece_fields(piece):
    """[(value, bits)] of one piece in stream order, every value least significant bit first (Huffman codes already reversed): the
    dynamic block, its end-of-block code and the three header bits of the empty stored block."""
    toks = tokens(piece)
    lengths = code_lengths(histogram(toks))
    codes = canonical_codes(lengths)
    nlit = max(s for s in range(286) if lengths[s]) + 1
    assert nlit >= 257
    f = [(0, 1), (2, 2), (nlit - 257, 5), (0, 5), (15, 4)]
    f += [(0 if s >= 16 else 4, 3) for s in CL_ORDER]
    f += [(_reverse(lengths[s], 4), 4) for s in range(nlit)] + [(_reverse(1, 4), 4)]  # the one distance code has length 1
    for kind, v in toks:
        if kind == "lit":
            f.append((_reverse(codes[v], lengths[v]), lengths[v]))
        else:
            s, e, x = length_symbol(v)
            f.append((_reverse(codes[s], lengths[s]) | (x << lengths[s]), lengths[s] + e + 1))  # (the distance code: one 0 bit)
    f.append((_reverse(codes[END_OF_BLOCK], lengths[END_OF_BLOCK]), lengths[END_OF_BLOCK]))
    f.append((0, 3))
    return f


def pack_fields(fields):
    values = np.array([v for v, _ in fields], np.uint64)
    bits = np.array([n for _, n in fields], np.int64)
    start = np.cumsum(bits) - bits
    idx = np.arange(int(bits.sum())) - np.repeat(start, bits)
    stream = ((np.repeat(values, bits) >> idx.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(stream, bitorder="little").tobytes()


def deflate_piece(piece):
    """The bytes of one piece: byte-aligned, so pieces can be concatenated."""
    return pack_fields(piece_fields(piece)) + b"\x00\x00\xff\xff"


# ---- the file ------------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode_filtered(filtered, width, channels, stripe_rows):
    """The file of given filtered rows uint8 [H, 1 + W * C]: signature, IHDR, one IDAT per piece (the first begins with the zlib header,
    the last ends with the empty final fixed block 03 00 and the Adler-32 of all filtered bytes), IEND."""
    filtered = np.ascontiguousarray(filtered, np.uint8)
    H = filtered.shape[0]
    assert filtered.shape[1] == 1 + width * channels and channels in (1, 3)
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", width, H, 8, 2 if channels == 3 else 0, 0, 0, 0))]
    starts = list(range(0, H, stripe_rows))
    for k, r0 in enumerate(starts):
        data = deflate_piece(filtered[r0:r0 + stripe_rows].tobytes())
        if k == 0:
            data = ZLIB_HEADER + data
        if k == len(starts) - 1:
            data += b"\x03\x00" + struct.pack(">I", zlib.adler32(filtered.tobytes()))
        out.append(chunk(b"IDAT", data))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def encode(frame, filter="adaptive", stripe_rows=16):
    frame = np.ascontiguousarray(frame)
    if frame.ndim == 2:
        frame = frame[..., None]
    return encode_filtered(filter_rows(frame, filter), frame.shape[1], frame.shape[2], stripe_rows)


def parse_chunks(data):
    """[(type, payload)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND."""
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, payload = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert len(payload) == n
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + payload), f"CRC of chunk {len(out)} ({kind})"
        out.append((kind, payload))
        pos += 12 + n
    assert out[-1][0] == b"IEND" and pos == len(data)
    return out


def idat_payload(data):
    return b"".join(p for k, p in parse_chunks(data) if k == b"IDAT")
