"""Mesh export: numpy restatements of csrc/umhs_mesh.hip, the bound of the fusion and the case builders (plain helper module, no tests).

Used by tests/test_mesh_cpu.py (the restatements alone: topology, convergence, planted faults, the bound's K) and tests/test_hip_mesh.py
(the kernels against them).  include/umhs_hip.h is the definition; this file follows it operation for operation.

Fusion, ``fuse``: the walk of umhs_tsdf_integrate over the cameras, vectorised over the lattice, in float32 (``F=np.float32``: numpy's
element-wise float32 operations are single rounded operations, nothing is fused -- the kernel's arithmetic) or in float64 on the same
float32 inputs (the truth).  The float64 run also returns, per lattice point, the envelopes of the bound and the edge flags.

ONE RULE for D and every attribute plane, as tests/rays_f64.py does it:   |got - ref64| <= K u (mag + tiny),   u = 2^-24, with
  m_i      = |lo_i| + |x_i h| + |t_i| + |e_i|               what one component of e = p - t is made of (the cancellation is real)
  mag_dist = sum_i (m_i + 2 |e_i|) |e_i| / |p - t| + |p - t|
  mag_obs  = (|d| + mag_dist) / trunc + |obs|                 (0 for a free-space sighting: obs = 1 exactly)
  mag_D'   = (W mag_D + mag_obs) / (W + 1) + (W |D| + |obs|) / (W + 1)        the running mean: its terms, then its own roundings
  mag_A'   = (Wc mag_A) / (Wc + 1) + (Wc |A| + |attr|) / (Wc + 1)             (attr is an input: exact)
and tiny = 2^-126.  W and Wc are counts: exact.  K_FUSE = max(8, 4 x the float32 restatement's worst ratio, rounded up to a power of
two); measured worst ratios over the committed cases (tests/test_mesh_cpu.py re-measures and asserts 4 x worst <= K_FUSE):
  D 0.35 | attributes 0.93     -> K_FUSE = 8.
Edges.  A float32 evaluation may legitimately decide otherwise where the float64 value is within EDGE = 64 u, relative to its envelope,
of a pixel boundary (u or v at an integer, while within a pixel of the image), of zc = 0, of sdf = -trunc or of |sdf| = trunc.  A point
with any such camera is left out of every comparison; at most 2 % of a case may be left out (asserted on the float64 run alone).

Extraction, ``extract``: marking, vertex order, rows and triangles of the three mesh kernels -> (rows uint8 [V, row_bytes], faces int32
[F,3], positions float32 [V,3], edge mask, vertex base).  Integer results, float32 positions and attributes: compared with ``==``."""
from __future__ import annotations

import itertools

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
EDGE = 64 * U
K_FUSE = 8.0
SLOT_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: the six tetrahedra
PERM_ODD = (0, 1, 1, 0, 0, 1)
WORLD = np.array([[0.5, -0.25, 0.125, 1.5], [0.25, 0.5, -0.75, -2.25], [-0.125, 0.75, 0.5, 0.375]], dtype=np.float32)


def row_bytes(C: int) -> int:
    return 15 if C == 0 else 19 + 4 * C


# ---- the lattice -------------------------------------------------------------------------------------------------------------------
def lattice_xyz(dims):
    nx, ny, nz = dims
    i = np.arange(nx * ny * nz, dtype=np.int64)
    return np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], 1)


def lattice_points(lo, h, dims, F=np.float32):
    """p_k = lo_k + ((float)x_k * h) per lattice point, [N,3] in F (lo, h are float32 values)."""
    xyz = lattice_xyz(dims).astype(F)
    return np.asarray(lo, dtype=np.float32).astype(F)[None, :] + xyz * F(np.float32(h))


# ---- fusion ------------------------------------------------------------------------------------------------------------------------
def camera(c2w, fx, fy, cx, cy, dist=None):
    c2w = np.asarray(c2w, dtype=np.float32).reshape(3, 4)
    d = None if dist is None or not np.any(np.asarray(dist) != 0) else np.asarray(dist, dtype=np.float32)
    return dict(R=c2w[:, :3].copy(), t=c2w[:, 3].copy(), fx=np.float32(fx), fy=np.float32(fy), cx=np.float32(cx), cy=np.float32(cy), dist=d)


def distort(x, y, k):
    """The forward OpenCV model (distort_opencv in csrc/umhs_camera.h, which undistort_opencv's residual subtracts (xd, yd) from); the
    dtype of x decides the arithmetic."""
    F = x.dtype.type
    k1, k2, k3, k4, p1, p2 = (F(v) for v in k)
    two = F(2.0)
    r = x * x + y * y
    d = F(1.0) + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    xd = (d * x + ((two * p1) * x) * y) + p2 * (r + (two * x) * x)
    yd = (d * y + ((two * p2) * x) * y) + p1 * (r + (two * y) * y)
    return xd, yd


def empty_state(n, K, F=np.float32):
    return dict(D=np.zeros(n, F), W=np.zeros(n, F), Wc=np.zeros(n, F), A=np.zeros((K, n), F))


def fuse(lo, h, dims, cams, depth, acc, rgb, abund=None, probs=None, threshold=0.5, trunc=0.1, F=np.float32, state=None, fault=None):
    """Fuse the cameras in order into ``state`` (a new empty one if None) -> state.  Images: float32 [n,H,W] / [n,H,W,c].  F=float64
    adds ``mag_D``, ``mag_A`` [K,N] and ``edge`` [N] bool to the state.  ``fault``: a planted fault (tests): "camera_z", "pixel",
    "colour_w"."""
    n = int(np.prod(dims))
    C = 0 if abund is None else abund.shape[-1]
    K = 3 + 2 * C
    f64 = F is np.float64
    st = empty_state(n, K, F) if state is None else state
    if f64 and "mag_D" not in st:
        st.update(mag_D=np.zeros(n), mag_A=np.zeros((K, n)), edge=np.zeros(n, bool))
    p = lattice_points(lo, h, dims, F)
    xyz = lattice_xyz(dims).astype(np.float64)
    thr, tr = np.float32(threshold), F(np.float32(trunc))
    H, Wd = depth.shape[1], depth.shape[2]
    attrs = [rgb[..., k] for k in range(3)] + [abund[..., k] for k in range(C)] + [probs[..., k] for k in range(C)]
    with np.errstate(all="ignore"):
        for c, cam in enumerate(cams):
            R, t = cam["R"].astype(F), cam["t"].astype(F)
            e = p - t[None, :]
            pc = [(R[0, j] * e[:, 0] + R[1, j] * e[:, 1]) + R[2, j] * e[:, 2] for j in range(3)]
            zc = -pc[2]
            ok = zc > 0
            x, y = pc[0] / zc, (-pc[1]) / zc
            xu, yu = x, y
            if cam["dist"] is not None:
                x, y = distort(x, y, cam["dist"])
            u, v = F(cam["fx"]) * x + F(cam["cx"]), F(cam["fy"]) * y + F(cam["cy"])
            ok &= (u >= 0) & (u < F(Wd)) & (v >= 0) & (v < F(H))
            iu, iv = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
            if fault == "pixel":
                iu = np.minimum(iu + 1, Wd - 1)
            d, a = depth[c, iv, iu].astype(F), acc[c, iv, iu]
            ok &= np.abs(d) <= np.finfo(np.float32).max
            hit = ~(a <= thr)
            dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
            sdf = d - (zc if fault == "camera_z" else dist)
            ok &= ~(hit & (sdf < -tr))
            obs = np.where(hit, np.minimum(F(1.0), sdf / tr), F(1.0))
            tint = ok & hit & (np.abs(sdf) <= tr)
            D, W, Wc = st["D"], st["W"], st["Wc"]
            one = F(1.0)
            if f64:  # envelopes and edges, before the state moves
                lo64, h64 = np.asarray(lo, np.float32).astype(np.float64), float(np.float32(h))
                m = np.abs(lo64)[None, :] + np.abs(xyz * h64) + np.abs(t)[None, :] + np.abs(e)
                mag_pc = [sum(abs(R[i, j]) * (m[:, i] + 2 * np.abs(e[:, i])) for i in range(3)) for j in range(3)]
                front = zc > 0
                edge = np.abs(zc) <= EDGE * mag_pc[2]
                mag_x = mag_pc[0] / zc + np.abs(xu) * mag_pc[2] / zc + np.abs(xu)
                mag_y = mag_pc[1] / zc + np.abs(yu) * mag_pc[2] / zc + np.abs(yu)
                if cam["dist"] is not None:
                    k1, k2, k3, k4, p1, p2 = (float(q) for q in cam["dist"])
                    r = xu * xu + yu * yu
                    dr = abs(k1) + r * (2 * abs(k2) + r * (3 * abs(k3) + r * 4 * abs(k4)))
                    dd = 1 + r * (abs(k1) + r * (abs(k2) + r * (abs(k3) + r * abs(k4))))
                    J = dd + 2 * r * dr + 6 * (abs(p1) + abs(p2)) * (np.abs(xu) + np.abs(yu))
                    mag_x, mag_y = (mag_x + mag_y) * J + 8 * np.abs(x), (mag_x + mag_y) * J + 8 * np.abs(y)
                mag_u = abs(float(cam["fx"])) * mag_x + np.abs(u) + abs(float(cam["cx"]))
                mag_v = abs(float(cam["fy"])) * mag_y + np.abs(v) + abs(float(cam["cy"]))
                near = front & (u > -1) & (u < Wd + 1) & (v > -1) & (v < H + 1)
                edge |= near & ((np.abs(u - np.rint(u)) <= EDGE * mag_u) | (np.abs(v - np.rint(v)) <= EDGE * mag_v))
                mag_dist = ((m + 2 * np.abs(e)) * np.abs(e)).sum(1) / np.maximum(dist, TINY) + dist
                mag_sdf = np.abs(d) + mag_dist
                inimg = front & (u >= 0) & (u < Wd) & (v >= 0) & (v < H) & (np.abs(d) <= np.finfo(np.float32).max) & hit
                edge |= inimg & ((np.abs(sdf + tr) <= EDGE * mag_sdf) | (np.abs(np.abs(sdf) - tr) <= EDGE * mag_sdf))
                st["edge"] |= edge
                mag_obs = np.where(hit, mag_sdf / tr + np.abs(obs), 0.0)
                st["mag_D"] = np.where(ok, (W * st["mag_D"] + mag_obs) / (W + 1) + (W * np.abs(D) + np.abs(obs)) / (W + 1), st["mag_D"])
                for k in range(K):
                    at = attrs[k][c, iv, iu].astype(F)
                    st["mag_A"][k] = np.where(tint, (Wc * st["mag_A"][k]) / (Wc + 1) + (Wc * np.abs(st["A"][k]) + np.abs(at)) / (Wc + 1),
                                              st["mag_A"][k])
            wa = W if fault == "colour_w" else Wc
            for k in range(K):
                at = attrs[k][c, iv, iu].astype(F)
                st["A"][k] = np.where(tint, ((st["A"][k] * wa) + at) / (wa + one), st["A"][k])
            st["D"] = np.where(ok, ((D * W) + obs) / (W + one), D)
            st["W"] = np.where(ok, W + one, W)
            st["Wc"] = np.where(tint, Wc + one, Wc)
    return st


def fuse_ratios(got, ref64):
    """Worst |got - ref64| / (u (mag + tiny)) over the points off every edge -> {"D": r, "A": r}, and the share of points left out."""
    keep = ~ref64["edge"]
    out = {}
    for name, mag in (("D", "mag_D"), ("A", "mag_A")):
        err = np.abs(got[name].astype(np.float64) - ref64[name])[..., keep]
        bound = U * (ref64[mag][..., keep] + TINY)
        out[name] = float((err / bound).max()) if err.size else 0.0
    return out, float((~keep).mean())


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """[3,4] camera-to-world of a camera at ``eye`` looking down its -z at ``target`` (x right, y up)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return np.concatenate([np.stack([r, u, -f], 1), eye[:, None]], 1).astype(np.float32)


DISTORTION = (-0.11, 0.035, -0.004, 0.0005, 0.0011, -0.0007)


def fusion_case(dims=(13, 10, 9), C=3, seed=0):
    """Three cameras of 24 x 16 pixels around a small lattice: the first sees a depth wall that occludes half of the volume and has
    NaN depths, the second is distorted and has background pixels, the third stands behind the volume's far side and looks away.
    Poses, lo and h are generic (no lattice plane projects onto a pixel boundary)."""
    rng = np.random.default_rng(seed)
    H, Wd = 16, 24
    h = np.float32(0.0537)
    lo = np.array([-0.3313, -0.2471, -0.2209], dtype=np.float32)
    centre = lo.astype(np.float64) + 0.5 * (np.array(dims) - 1) * float(h)
    eyes = [centre + np.array([2.13, 0.37, 0.51]), centre + np.array([-0.41, -1.93, 0.77]), centre + np.array([0.3, 2.4, -0.2])]
    targets = [centre + np.array([0.013, -0.021, 0.017]), centre + np.array([-0.019, 0.011, 0.023]), centre + np.array([0.4, 6.0, -0.3])]
    foc = np.float32(31.7)
    cams = [camera(look_at(eyes[0], targets[0]), foc, foc * np.float32(1.01), 12.13, 7.91),
            camera(look_at(eyes[1], targets[1]), foc, foc, 11.87, 8.09, DISTORTION),
            camera(look_at(eyes[2], targets[2]), foc, foc, 12.0, 8.0)]
    yy, xx = np.meshgrid(np.arange(H), np.arange(Wd), indexing="ij")
    depth = np.empty((3, H, Wd), np.float32)
    for c in range(3):
        base = np.linalg.norm(eyes[c] - centre)
        depth[c] = (base + 0.11 * np.sin(0.5 * xx + c) * np.cos(0.4 * yy) + 0.01 * rng.standard_normal((H, Wd))).astype(np.float32)
    depth[0, :, :11] = np.float32(1.2)  # the wall: everything behind it is skipped
    depth[0, 3, 14] = depth[0, 9, 17] = np.nan
    depth[0, 5, 20] = np.inf
    acc = (0.55 + 0.45 * rng.random((3, H, Wd))).astype(np.float32)
    acc[1, ::3, 1::4] = np.float32(0.2)  # background: free space along the whole ray
    acc[1, 7, 7] = np.float32(0.5)  # exactly the threshold: not a hit
    rgb = rng.random((3, H, Wd, 3)).astype(np.float32)
    abund = rng.random((3, H, Wd, C)).astype(np.float32) if C else None
    probs = rng.random((3, H, Wd, C)).astype(np.float32) if C else None
    return dict(lo=lo, h=h, dims=tuple(dims), cams=cams, depth=depth, acc=acc, rgb=rgb, abund=abund, probs=probs, threshold=0.5,
                trunc=float(np.float32(5.0) * h), C=C)


def fuse_case(case, F=np.float32, cameras=None, state=None, fault=None):
    idx = list(range(len(case["cams"]))) if cameras is None else list(cameras)
    pick = lambda a: None if a is None else a[idx]
    return fuse(case["lo"], case["h"], case["dims"], [case["cams"][i] for i in idx], pick(case["depth"]), pick(case["acc"]),
                pick(case["rgb"]), pick(case["abund"]), pick(case["probs"]), case["threshold"], case["trunc"], F, state, fault)


# ---- projection and rays (the round trip) ------------------------------------------------------------------------------------------
def project(cam, pts):
    """float64 projection of points [M,3] by the fusion's model -> (u, v, zc)."""
    e = pts.astype(np.float64) - cam["t"].astype(np.float64)[None, :]
    pc = e @ cam["R"].astype(np.float64)
    zc = -pc[:, 2]
    x, y = pc[:, 0] / zc, -pc[:, 1] / zc
    if cam["dist"] is not None:
        x, y = distort(x, y, cam["dist"])
    return float(cam["fx"]) * x + float(cam["cx"]), float(cam["fy"]) * y + float(cam["cy"]), zc


def undistort64(xd, yd, k, steps=10):
    """umhs_raygen_distorted's Newton solve (undistort_opencv in csrc/umhs_camera.h), in float64."""
    k1, k2, k3, k4, p1, p2 = (float(v) for v in k)
    x, y = xd.copy(), yd.copy()
    for _ in range(steps):
        r = x * x + y * y
        d = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        fx = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x) - xd
        fy = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y) - yd
        d_r = k1 + r * (2 * k2 + r * (3 * k3 + r * 4 * k4))
        d_x, d_y = 2 * x * d_r, 2 * y * d_r
        fx_x = d + d_x * x + 2 * p1 * y + 6 * p2 * x
        fx_y = d_y * x + 2 * p1 * x + 2 * p2 * y
        fy_x = d_x * y + 2 * p2 * y + 2 * p1 * x
        fy_y = d + d_y * y + 2 * p2 * x + 6 * p1 * y
        den = fy_x * fx_y - fx_x * fy_y
        ok = np.abs(den) > 1e-3
        x = x + np.where(ok, (fx * fy_y - fy * fx_y) / den, 0.0)
        y = y + np.where(ok, (fy * fx_x - fx * fy_x) / den, 0.0)
    return x, y


def pixel_rays(cam, H, Wd):
    """Origins and normalised directions of the pixel centres of a camera, as umhs_raygen(_distorted) forms them, in float64."""
    yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(Wd) + 0.5, indexing="ij")
    x, y = (xx.ravel() - float(cam["cx"])) / float(cam["fx"]), (yy.ravel() - float(cam["cy"])) / float(cam["fy"])
    if cam["dist"] is not None:
        x, y = undistort64(x, y, cam["dist"])
    d = np.stack([x, -y, -np.ones_like(x)], 1) @ cam["R"].astype(np.float64).T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.broadcast_to(cam["t"].astype(np.float64), d.shape), d


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def quantise(v):
    """(uint8)(clamp(v, 0, 1) * 255.0f), truncated; NaN -> 0."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(v > 0, np.minimum(v, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return (c * np.float32(255.0)).astype(np.int32).astype(np.uint8)


def _popcount_below(mask, slot):
    m = mask.astype(np.int64) & ((1 << slot) - 1)
    return sum((m >> b) & 1 for b in range(7))


def extract(D, W, Wc, A, lo, h, dims, world=None, swap_winding=False):
    """-> dict(rows, faces, pos, mask, vbase).  ``A`` [3 + 2 C, N]; everything float32.  ``swap_winding``: a planted fault."""
    nx, ny, nz = dims
    N = nx * ny * nz
    C = (A.shape[0] - 3) // 2
    D, W, Wc, A = (np.asarray(a, np.float32) for a in (D, W, Wc, A))
    xyz = lattice_xyz(dims)
    valid, inside = W > 0, D < 0
    idx = np.arange(N)
    step = lambda o: o[0] + o[1] * nx + o[2] * nx * ny
    fits = lambda o: (xyz[:, 0] + o[0] < nx) & (xyz[:, 1] + o[1] < ny) & (xyz[:, 2] + o[2] < nz)
    bits = np.zeros((N, 7), bool)
    for s, o in enumerate(SLOT_OFFSETS):
        f = fits(o)
        j = np.where(f, idx + step(o), 0)
        bits[:, s] = f & valid & valid[j] & (inside != inside[j])
    mask = (bits * (1 << np.arange(7))).sum(1).astype(np.uint8)
    per_point = bits.sum(1)
    vbase = (np.cumsum(per_point) - per_point).astype(np.int32)
    own, slot = np.nonzero(bits)  # ascending (point, slot): the vertex order
    V = len(own)
    off = np.array(SLOT_OFFSETS)[slot]
    other = own + off[:, 0] + off[:, 1] * nx + off[:, 2] * nx * ny
    F = np.float32
    lo32, h32 = np.asarray(lo, F), F(h)
    with np.errstate(all="ignore"):
        t = D[own] / (D[own] - D[other])
        pa = lo32[None, :] + xyz[own].astype(F) * h32
        pb = lo32[None, :] + (xyz[own] + off).astype(F) * h32
        pos = pa + t[:, None] * (pb - pa)
        w = pos
        if world is not None:
            Aw = np.asarray(world, F)
            w = np.stack([((Aw[r, 0] * pos[:, 0] + Aw[r, 1] * pos[:, 1]) + Aw[r, 2] * pos[:, 2]) + Aw[r, 3] for r in range(3)], 1)
        ca, cb = Wc[own] > 0, Wc[other] > 0
        a, b = A[:, own], A[:, other]
        attr = np.where(ca & cb, a + t[None, :] * (b - a), np.where(ca, a, np.where(cb, b, F(0.0)))).astype(F)
    rb = row_bytes(C)
    rows = np.zeros((V, rb), np.uint8)
    rows[:, :12] = np.ascontiguousarray(w.astype(F)).view(np.uint8).reshape(V, 12)
    for k in range(3):
        rows[:, 12 + k] = quantise(attr[k])
    if C:
        probs = attr[3 + C:]
        best, arg = np.full(V, -np.inf, F), np.zeros(V, np.int32)
        for k in range(C):
            with np.errstate(invalid="ignore"):
                win = probs[k] > best
            best, arg = np.where(win, probs[k], best), np.where(win, k, arg).astype(np.int32)
        arg = np.where(ca | cb, arg, -1).astype(np.int32)
        rows[:, 15:19] = arg.view(np.uint8).reshape(V, 4)
        rows[:, 19:] = np.ascontiguousarray(attr[3:3 + C].T).view(np.uint8).reshape(V, 4 * C)
    # triangles
    cell = (xyz[:, 0] + 1 < nx) & (xyz[:, 1] + 1 < ny) & (xyz[:, 2] + 1 < nz)
    for o in itertools.product((0, 1), repeat=3):
        cell &= valid[np.where(fits(o), idx + step(o), 0)]
    cells = idx[cell]
    tri = np.zeros((len(cells), 6, 2, 3), np.int32)
    have = np.zeros((len(cells), 6, 2), bool)
    for ti, perm in enumerate(PERMS):
        offs = [np.zeros(3, int)]
        for ax in perm:
            o = offs[-1].copy()
            o[ax] += 1
            offs.append(o)
        offs = [offs[0], offs[1], offs[2], np.ones(3, int)]
        corner = [cells + step(o) for o in offs]
        code = sum(inside[corner[k]].astype(int) << k for k in range(4))

        def eid(sel, i, j):
            i, j = min(i, j), max(i, j)
            s = SLOT_OFFSETS.index(tuple(offs[j] - offs[i]))
            owner = corner[i][sel]
            return vbase[owner] + _popcount_below(mask[owner], s)

        for cd in range(1, 15):
            sel = np.nonzero(code == cd)[0]
            if not len(sel):
                continue
            ins = [k for k in range(4) if (cd >> k) & 1]
            outs = [k for k in range(4) if not (cd >> k) & 1]
            if len(ins) == 2:
                inv = sum(p > q for p in ins for q in outs)
                flip = bool((inv & 1) ^ PERM_ODD[ti]) ^ swap_winding
                qa, qb, qc, qd = eid(sel, ins[0], outs[0]), eid(sel, ins[0], outs[1]), eid(sel, ins[1], outs[1]), eid(sel, ins[1], outs[0])
                tri[sel, ti, 0] = np.stack([qa, qc, qb] if flip else [qa, qb, qc], 1)
                tri[sel, ti, 1] = np.stack([qa, qd, qc] if flip else [qa, qc, qd], 1)
                have[sel, ti, :] = True
            else:
                p = ins[0] if len(ins) == 1 else outs[0]
                q = [k for k in range(4) if k != p]
                flip = bool((p & 1) ^ PERM_ODD[ti] ^ (len(ins) == 3)) ^ swap_winding
                e0, e1, e2 = eid(sel, p, q[0]), eid(sel, p, q[1]), eid(sel, p, q[2])
                tri[sel, ti, 0] = np.stack([e0, e2, e1] if flip else [e0, e1, e2], 1)
                have[sel, ti, 0] = True
    faces = tri[have].reshape(-1, 3).astype(np.int32)
    return dict(rows=rows, faces=faces, pos=pos.astype(F), mask=mask, vbase=vbase, n_classes=C)


# ---- mesh measures -----------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)


def closed_and_oriented(faces, n_vertices):
    """Every undirected edge lies in exactly two triangles, once in each direction."""
    de = directed_edges(faces)
    key = de[:, 0] * n_vertices + de[:, 1]
    rev = de[:, 1] * n_vertices + de[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(np.sort(rev), uniq))


def euler(faces, n_vertices):
    de = np.sort(directed_edges(faces), 1)
    return n_vertices - len(np.unique(de[:, 0] * n_vertices + de[:, 1])) + len(faces)


def volume_area(pos, faces):
    a, b, c = (pos[faces[:, k]].astype(np.float64) for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0), float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)


# ---- fields ------------------------------------------------------------------------------------------------------------------------
def cube_lattice(n, half=1.0):
    """n^3 lattice over [-half, half]^3 (shifted by an irrational-looking offset so no level set passes through a lattice point)."""
    h = np.float32(2.0 * half / (n - 1))
    lo = np.array([-half + 0.00317, -half - 0.00213, -half + 0.00129], np.float32)
    return lo, h, (n, n, n)


def field(name, lo, h, dims, C=3, seed=0):
    """Analytic and synthetic volumes -> (D, W, Wc, A) float32."""
    p = lattice_points(lo, h, dims, np.float64)
    n = len(p)
    rng = np.random.default_rng(seed)
    W = np.ones(n, np.float32)
    if name == "sphere":
        D = np.linalg.norm(p, axis=1) - 0.6
    elif name == "torus":
        D = np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.55) ** 2 + p[:, 2] ** 2) - 0.23
    elif name == "two_spheres":  # touching at the origin
        D = np.minimum(np.linalg.norm(p - [0.4, 0, 0], axis=1), np.linalg.norm(p + [0.4, 0, 0], axis=1)) - 0.4
    elif name == "outside":
        D = 0.25 + rng.random(n)
    elif name == "random":  # random signs, a fifth of the points never seen
        D = rng.standard_normal(n)
        W = (rng.random(n) > 0.2).astype(np.float32) * rng.integers(1, 5, n).astype(np.float32)
    elif name == "slab":  # a tilted plane that cuts every lattice row along x: the surface crosses every chunk border
        D = p @ np.array([0.92, 0.23, 0.31]) - (p.mean(0) @ np.array([0.92, 0.23, 0.31])) + 0.0071
    else:
        raise KeyError(name)
    Wc = ((rng.random(n) > 0.15) * rng.integers(1, 4, n)).astype(np.float32)
    A = rng.random((3 + 2 * C, n)).astype(np.float32)
    A[0, ::7] = 1.5  # beyond the byte's range
    A[1, ::11] = -0.25
    if C:
        A[3 + C, ::13] = np.nan  # a NaN never wins the label
        A[3 + C:, ::17] = 0.5  # ties: the first wins
    return D.astype(np.float32), W, Wc, A


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------
def read_mesh_ply(path):
    """A hand-written reader of the binary little-endian PLY the export writes -> (vertex table, raw vertex rows uint8 [V,rb],
    faces int32 [F,3])."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    np_type = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    elements, cur = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            cur = (w[1], int(w[2]), [])
            elements.append(cur)
        elif w[0] == "property":
            cur[2].append(w[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    _, nv, vprops = elements[0]
    _, nf, fprops = elements[1]
    assert fprops == [["list", "uchar", "int", "vertex_indices"]]
    vdt = np.dtype([(name, np_type[t]) for t, name in vprops])
    body = raw[end:]
    assert len(body) == nv * vdt.itemsize + nf * 13, (len(body), nv, vdt.itemsize, nf)
    table = np.frombuffer(body, vdt, nv)
    rows = np.frombuffer(body, np.uint8, nv * vdt.itemsize).reshape(nv, vdt.itemsize)
    frows = np.frombuffer(body, np.uint8, nf * 13, nv * vdt.itemsize).reshape(nf, 13)
    assert (frows[:, 0] == 3).all()
    faces = np.ascontiguousarray(frows[:, 1:]).view("<i4").reshape(nf, 3)
    return table, rows, faces
