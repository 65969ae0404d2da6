"""CPU restatement of the point-cloud export (include/umhs_hip.h, "Point-cloud export"): the keep rule and the row packing in numpy
float32, one rounded operation per step and in the header's order; the k-nearest-neighbour mean in float64 on scipy's cKDTree (the
reference the kernel is held to) and in emulated float32 (the kernel's arithmetic, for the bound); the outlier rule; a PLY reader; and
the inputs the CPU and GPU tests share."""
import functools

import numpy as np

F = np.float32
FMAX = np.finfo(np.float32).max
U = 2.0 ** -24  # unit roundoff of float32


# ---- keep rule and rows ------------------------------------------------------------------------------------------------------------
def points_of(o, d, depth):
    """p_k = (d_k * depth) + o_k, two rounded float32 operations."""
    with np.errstate(all="ignore"):
        return (d.astype(F) * depth.astype(F).reshape(-1, 1)).astype(F) + o.astype(F)


def box_coordinates(p, box):
    """q = R^T (p - T): e_j = p_j - T_j; q_k = ((R[0][k] * e_0) + (R[1][k] * e_1)) + (R[2][k] * e_2)."""
    T, R, S = (np.asarray(v, dtype=F) for v in box)
    with np.errstate(all="ignore"):
        e = p - T.reshape(1, 3)
        return np.stack([((R[0, k] * e[:, 0]) + (R[1, k] * e[:, 1])) + (R[2, k] * e[:, 2]) for k in range(3)], axis=1).astype(F)


def keep_rule(p, acc, threshold=0.5, box=None):
    with np.errstate(all="ignore"):
        keep = (acc.astype(F).reshape(-1) > F(threshold)) & (np.abs(p) <= FMAX).all(axis=1)
        if box is not None:
            h = (np.asarray(box[2], dtype=F) * F(0.5)).reshape(1, 3)
            q = box_coordinates(p, box)
            keep &= ((q < h) & (q > -h)).all(axis=1)
    return keep


def byte_of(v):
    """(uint8)(clamp(v, 0, 1) * 255.0f), truncated; NaN -> 0."""
    v = np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        c = np.where(v > 0, np.minimum(v, F(1.0)), F(0.0)).astype(F)  # (NaN > 0 is false)
        return (c * F(255.0)).astype(F).astype(np.int32).astype(np.uint8)


def material_of(probs):
    """First index of the largest value; a NaN never wins (mx starts at -inf, arg at 0)."""
    n, C = probs.shape
    mx, arg = np.full(n, -np.inf, dtype=F), np.zeros(n, dtype=np.int32)
    with np.errstate(all="ignore"):
        for k in range(C):
            win = probs[:, k] > mx
            mx, arg = np.where(win, probs[:, k], mx), np.where(win, k, arg).astype(np.int32)
    return arg


def world_of(p, A):
    """w_i = (((A[i][0] * p_0) + (A[i][1] * p_1)) + (A[i][2] * p_2)) + A[i][3]."""
    A = np.asarray(A, dtype=F).reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.stack([(((A[i, 0] * p[:, 0]) + (A[i, 1] * p[:, 1])) + (A[i, 2] * p[:, 2])) + A[i, 3] for i in range(3)], axis=1).astype(F)


def row_bytes(C):
    return 16 if C == 0 else 20 + 4 * C


def emit(o, d, depth, acc, rgb, abund=None, probs=None, threshold=0.5, box=None, world=None, ordinal0=0):
    """-> (rows uint8 [K, row_bytes], points float32 [K,3], kept int64 [K]) of the K kept rays, in ray order."""
    p = points_of(o, d, depth)
    keep = keep_rule(p, acc, threshold, box)
    idx = np.nonzero(keep)[0]
    C = 0 if abund is None else abund.shape[1]
    rows = np.zeros((idx.size, row_bytes(C)), dtype=np.uint8)
    pk = p[idx]
    xyz = pk if world is None else world_of(pk, world)
    rows[:, 0:12] = np.ascontiguousarray(xyz.astype("<f4")).view(np.uint8).reshape(-1, 12)
    rows[:, 12:15] = byte_of(rgb[idx, :3])
    rows[:, 15] = byte_of(acc.reshape(-1)[idx])
    if C:
        rows[:, 16:20] = np.ascontiguousarray(material_of(probs[idx]).astype("<i4")).view(np.uint8).reshape(-1, 4)
        rows[:, 20:] = np.ascontiguousarray(abund[idx].astype("<f4")).view(np.uint8).reshape(-1, 4 * C)
    return rows, pk, idx.astype(np.int64) + ordinal0


# ---- the file ----------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4"}


def read_ply(path):
    """A binary little-endian PLY with one ``vertex`` element of scalar properties -> (structured array [M], raw rows uint8 [M, row])."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    count, fields = None, []
    for ln in lines[2:]:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            count = int(w[2])
        elif w[0] == "element":
            raise ValueError(f"unexpected element {ln!r}")
        elif w[0] == "property":
            assert count is not None and len(w) == 3, ln
            fields.append((w[2], _PLY_TYPES[w[1]]))
    dt = np.dtype(fields)
    body = blob[end:]
    assert len(body) == count * dt.itemsize, (len(body), count, dt.itemsize)
    return np.frombuffer(body, dtype=dt), np.frombuffer(body, dtype=np.uint8).reshape(count, dt.itemsize)


# ---- neighbours --------------------------------------------------------------------------------------------------------------------
def knn_mean64(points, k):
    """float64 [M]: mean distance to the min(k, M) nearest points, the point itself included (cKDTree on the float32 points)."""
    from scipy.spatial import cKDTree

    p = np.asarray(points, dtype=np.float64)
    kk = min(k, p.shape[0])
    d, _ = cKDTree(p).query(p, k=kk)
    return d.reshape(p.shape[0], kk).mean(axis=1)


def knn_mean32(points, k):
    """The kernel's arithmetic in numpy float32, by brute force: d2 = ((dx*dx) + (dy*dy)) + (dz*dz), the k_eff smallest, their square
    roots added in ascending order, one division."""
    p = np.asarray(points, dtype=F)
    m = p.shape[0]
    kk = min(k, m)
    out = np.empty(m, dtype=F)
    for a in range(0, m, 512):
        q = p[a:a + 512]
        dx, dy, dz = (p[None, :, c] - q[:, None, c] for c in range(3))
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        small = np.sqrt(np.sort(np.partition(d2, kk - 1, axis=1)[:, :kk], axis=1)).astype(F)
        s = np.zeros(q.shape[0], dtype=F)
        for j in range(kk):
            s = s + small[:, j]
        out[a:a + 512] = s / F(kk)
    return out


def knn_bound(mean64, k):
    """|float32 result - float64 result| <= (k + 8) * 2^-24 * mean64.  A distance takes three differences (one rounding each), three
    products, two additions and a square root: 2 * (1 + 1/2 + 1) / 2 + 1 <= 3.5 roundings of relative size 2^-24 after the root; the
    k_eff - 1 additions of the mean and its division add at most k; a near-tie resolved the other way exchanges two distances that differ
    by less than their own rounding.  (k + 4.5 rounded up generously: k + 8.)"""
    return (k + 8) * U * np.asarray(mean64, dtype=np.float64)


def outlier_rule(means, std_ratio):
    """Open3D's rule on float64 means -> (mu, sigma with divisor M - 1 (0 for M < 2), threshold, keep)."""
    m = np.asarray(means, dtype=np.float64)
    mu = m.mean()
    sigma = m.std(ddof=1) if m.size > 1 else 0.0
    thr = mu + std_ratio * sigma
    return mu, sigma, thr, (m > 0) & (m < thr)


KNN_SETS = ("cube", "plane", "clusters", "identical", "copies")
KNN_M = (1, 5, 20, 21, 333, 4096)
KNN_K = (2, 20, 32)


def knn_cases():
    """(set, M, k): every set at every size and k; "copies" (64 copies of one point inside a uniform set) needs more than 64 points."""
    return [(s, m, k) for s in KNN_SETS for m in KNN_M for k in KNN_K if s != "copies" or m > 64]


@functools.lru_cache(maxsize=None)
def knn_points(name, m):
    """float32 [m,3], read-only.  cube: uniform in [-1, 1]^3.  plane: z = 0.25 exactly (one grid dimension of 1).  clusters: two
    clusters of radius 1e-3 at (-40, 3, 7) and (55, -2, 9) and max(1, m // 50) stragglers spread over the box between them (many empty
    rings to cross).  identical: one point m times.  copies: 64 copies of one point, the rest uniform."""
    rng = np.random.default_rng(1000 + m)
    if name == "cube":
        p = rng.uniform(-1, 1, (m, 3))
    elif name == "plane":
        p = np.concatenate([rng.uniform(-2, 2, (m, 2)), np.full((m, 1), 0.25)], axis=1)
    elif name == "clusters":
        ns = max(1, m // 50) if m > 2 else 0
        na = (m - ns) // 2
        a = np.array([-40.0, 3.0, 7.0]) + 1e-3 * rng.normal(size=(na, 3))
        b = np.array([55.0, -2.0, 9.0]) + 1e-3 * rng.normal(size=(m - ns - na, 3))
        s = rng.uniform([-40, -2, 7], [55, 3, 9], (ns, 3))
        p = np.concatenate([a, b, s])[rng.permutation(m)]
    elif name == "identical":
        p = np.tile(np.array([[0.3, -1.7, 2.9]]), (m, 1))
    elif name == "copies":
        p = rng.uniform(-1, 1, (m, 3))
        p[rng.choice(m, 64, replace=False)] = np.array([0.125, -0.5, 0.75])
    else:
        raise KeyError(name)
    p = np.ascontiguousarray(p.astype(F))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def knn_reference(name, m, k):
    out = knn_mean64(knn_points(name, m), k)
    out.setflags(write=False)
    return out


# ---- inputs of the emit tests ------------------------------------------------------------------------------------------------------
AXIS_BOX = (np.array([0.25, -0.75, 0.125], dtype=F), np.eye(3, dtype=F), np.array([2.0, 1.0, 1.5], dtype=F))


def rotated_box():
    a, b = 0.6, -0.35
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return np.array([0.1, 0.2, -0.3], dtype=F), (Rz @ Rx).astype(F), np.array([1.5, 2.5, 1.0], dtype=F)


WORLD = np.array([[0.8, -0.1, 0.3, 2.0], [0.2, 1.1, -0.4, -1.0], [-0.3, 0.25, 0.9, 0.5]], dtype=F)


def emit_inputs(n, C, pattern="mixed", box=None, seed=0):
    """Rays and rendered outputs of n rays.  pattern: "all" (every accumulation above the threshold, no special value), "none",
    "alternate" (every other ray above), "mixed": random accumulations and, at fixed positions modulo 32, NaN / +inf / -inf depths, NaN
    and inf origins, accumulation at exactly 0.5, at nextafter(0.5, 1) and NaN, colours outside [0, 1] and NaN, equal and NaN cluster
    probabilities, and -- with a box -- points exactly on a face of it and one float32 step to either side (depth 0: p = o)."""
    rng = np.random.default_rng(seed + 7 * n + C)
    o = rng.uniform(-0.3, 0.3, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    depth = rng.uniform(0.0, 1.2, (n, 1)).astype(F)
    rgb = rng.uniform(-0.1, 1.1, (n, 3)).astype(F)
    acc = {"all": np.full((n, 1), 0.9), "none": np.full((n, 1), 0.3), "alternate": np.where(np.arange(n) % 2 == 0, 0.9, 0.1).reshape(n, 1),
           "mixed": rng.uniform(0.0, 1.0, (n, 1))}[pattern].astype(F)
    abund = rng.uniform(0, 1, (n, C)).astype(F) if C else None
    probs = rng.uniform(0, 1, (n, C)).astype(F) if C else None
    if pattern == "mixed":
        i = np.arange(n)
        for r, v in ((3, np.nan), (4, np.inf), (5, -np.inf)):
            depth[i % 32 == r] = v
        o[i % 32 == 6, 1] = np.nan
        o[i % 32 == 7, 2] = np.inf
        acc[i % 32 == 8] = 0.5
        acc[i % 32 == 9] = np.nextafter(F(0.5), F(1.0))
        acc[i % 32 == 10] = np.nan
        acc[i % 32 == 11] = 1.5
        rgb[i % 32 == 12] = [np.nan, 1.0, 0.0]
        rgb[i % 32 == 13] = [F(0.999999), F(1 / 255), np.nextafter(F(1 / 255), F(0))]
        if C:
            probs[i % 32 == 14] = 0.5
            probs[i % 32 == 15, 0] = np.nan
            if C > 2:
                probs[i % 32 == 16, 1:3] = 2.0
            abund[i % 32 == 17, 0] = np.nan
        if box is not None:
            T, R, S = (np.asarray(v, dtype=F) for v in box)
            face = (T + R[:, 0] * (S[0] * F(0.5))).astype(F)  # centre of the +x face
            for r, step in ((18, 0.0), (19, -np.inf), (20, np.inf)):
                sel = i % 32 == r
                o[sel] = face if step == 0.0 else np.nextafter(face, F(step) * np.sign(R[:, 0] + F(1e-30)))
                depth[sel], acc[sel] = 0.0, 0.9
            sel = i % 32 == 21  # on the -y face
            o[sel] = (T - R[:, 1] * (S[1] * F(0.5))).astype(F)
            depth[sel], acc[sel] = 0.0, 0.9
    return dict(o=o, d=d, depth=depth, acc=acc, rgb=rgb, abund=abund, probs=probs)
