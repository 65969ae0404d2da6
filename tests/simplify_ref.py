"""Mesh simplification: a numpy restatement of csrc/umhs_simplify.hip, its bounds and the case builders (plain helper module, no tests).

Used by tests/test_simplify_cpu.py (the restatement alone: identity, topology, volume, planted faults) and tests/test_hip_simplify.py
(the kernels against it).  include/umhs_hip.h ("Mesh simplification") is the definition; this file follows it rule for rule.

Keys, faces, colours and labels are integers formed through float32 operations (numpy's element-wise float32 operations are single
rounded operations): compared with ``==``.  Positions and abundances are float64 sums rounded once to float32.

THE POSITION BOUND.  Kernel and restatement solve the same 3 x 3 system (A + lambda I) x = b + lambda m in float64; its condition is
at most 1 + 3 / rho = 3001 (A is positive semi-definite with largest eigenvalue <= tr A, lambda = rho tr A / 3).  They may differ
  * in the order of the float64 sums and in the solver (Cholesky there, LU here).  A sum of L terms carries a relative error of at
    most L 2^-53 of the sum of the magnitudes; the entries of A are sums of L = (corner records of the cluster) products n_i n_j, each
    with 3 roundings behind it (the edge vectors are exact differences of float32 values, the cross product rounds once per component,
    the product once): |dA| <= (L + 3) 2^-53 tr A, and likewise |db| <= (L + 6) 2^-53 tr A r with r the largest |a - o| of a record
    (d = n . (a - o) adds 3 roundings).  m is a mean of M members: |dm| <= (M + 2) 2^-53 r.  A backward-stable 3 x 3 solve adds about
    16 2^-53 |A| |x|.  With |x| <= r' (the solution is a point of the regularised least-squares problem, within the reach r' =
    max(r, |m|) of the data), the first-order perturbation bound gives
        |dx| <= cond ((L + 3) + (L + 6) + (M + 2) + 16) 2^-53 r'  <=  3001 (2 L + M + 27) 2^-53 r'
    for ONE evaluation; two evaluations differ by at most twice that.  Written as the issue asks, proportional to 3001 2^-53 e:
        F64_TERM = K64 3001 2^-53 e,    K64 = 2 (2 L_max + M_max + 27) (r'_max / e),
    L_max, M_max and r'_max taken over the clusters of the case (the restatement returns them: they are properties of the input).
  * in the one rounding to float32: half a float32 ulp of the largest coordinate magnitude the clamp box allows (the clamp maps both
    float64 values into the same box, and clamping never increases a difference).
  ->  |got32 - x64| <= ulp32(box magnitude) / 2 + F64_TERM, per component, against the restatement's float64 position.
Abundances: the float64 means differ by a few 2^-53 relative, far below float32's 2^-24; only the final rounding can differ:
  |got - want| <= 1 float32 ulp of |want| (ABUND_ULPS = 1)."""
from __future__ import annotations

import numpy as np

RHO = 1e-3
COND_MAX = 1.0 + 3.0 / RHO  # 3001
ABUND_ULPS = 1
NO_KEY = np.iinfo(np.int64).max
FAULTS = ("skip_dedup", "no_regulariser", "label_tie_last")


def row_bytes(C: int) -> int:
    return 15 if C == 0 else 19 + 4 * C


def positions_of(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    return np.ascontiguousarray(rows[:, :12]).view("<f4").reshape(-1, 3)


def grid_dims(pos, origin, edge):
    """(nx, ny, nz): (int)floor((M - g) / e) + 1 per axis in float32, M over the finite vertices; one cell without any."""
    g, e = np.asarray(origin, np.float32), np.float32(edge)
    fin = np.isfinite(pos).all(1)
    if not fin.any():
        return (1, 1, 1)
    with np.errstate(all="ignore"):
        q = np.floor((pos[fin].max(0).astype(np.float32) - g) / e)
    if not (q < 2.0 ** 31 - 1).all():
        raise ValueError("an axis of 2^31 cells or more")
    dims = tuple(max(int(v), 0) + 1 for v in q)
    if dims[0] * dims[1] * dims[2] >= 1 << 62:
        raise ValueError("a grid of 2^62 cells or more")
    return dims


def cell_indices(pos, origin, edge, dims):
    """[V,3] int64 cell of every vertex (rows of non-finite vertices are meaningless) and the finite mask."""
    g, e = np.asarray(origin, np.float32), np.float32(edge)
    fin = np.isfinite(pos).all(1)
    with np.errstate(all="ignore"):
        q = np.floor((np.where(fin[:, None], pos, np.float32(0)).astype(np.float32) - g[None, :]) / e)
    idx = np.clip(q, 0, np.asarray(dims, np.float64)[None, :] - 1).astype(np.int64)
    return idx, fin


def ulp32(x):
    """The float32 ulp at magnitude x (x > 0 normal)."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def apply_world(world, pos32):
    A = np.asarray(world, np.float32)
    p = np.asarray(pos32, np.float32)
    return np.stack([((A[r, 0] * p[:, 0] + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]) + A[r, 3] for r in range(3)], 1).astype(np.float32)


def kept_faces(fc, valid, fault=None):
    """bool [F]: the faces that survive, given their clusters ``fc`` [F,3] and validity."""
    F = len(fc)
    live = valid & (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    r = np.argmin(np.where(live[:, None], fc, 0), 1)
    can = np.stack([fc[np.arange(F), (r + k) % 3] for k in range(3)], 1)
    keep = live.copy()
    if fault != "skip_dedup" and live.any():
        idx = np.nonzero(live)[0]
        order = idx[np.lexsort((idx, can[idx, 2], can[idx, 1], can[idx, 0]))]  # equal triples adjacent, the first in input order first
        same = np.zeros(len(order), bool)
        same[1:] = (can[order[1:]] == can[order[:-1]]).all(1)
        keep[order[same]] = False
    return keep


def count(rows, faces, C, origin, edge):
    return int(simplify(rows, faces, C, origin, edge, faces_only=True)["faces"].shape[0])


def simplify(rows, faces, C, origin, edge, world=None, fault=None, faces_only=False):
    """-> dict(rows uint8 [V', rb], faces int32 [F', 3], positions float32 [V', 3], pos64 [V', 3] (before the rounding), cluster int32 [V],
    n_classes, abund64 [V', C], pos_bound [V', 3], cond (worst condition of a solved system), tr0 (used clusters with tr A = 0),
    L_max, M_max, reach_max).  ``fault``: a planted fault (tests), one of FAULTS."""
    assert fault is None or fault in FAULTS
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, row_bytes(C))
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = len(rows), len(faces)
    pos = positions_of(rows)
    dims = grid_dims(pos, origin, edge)
    idx, fin = cell_indices(pos, origin, edge, dims)
    key = np.where(fin, (idx[:, 2] * dims[1] + idx[:, 1]) * dims[0] + idx[:, 0], NO_KEY)
    ukeys, cl = np.unique(key[fin], return_inverse=True)  # clusters ascend by key
    Nc = len(ukeys)
    vc = np.full(V, -1, np.int64)
    vc[fin] = cl
    f64i = faces.astype(np.int64)
    valid = ((f64i >= 0) & (f64i < V)).all(1)
    safe = np.where(valid[:, None], f64i, 0)
    valid &= (vc[safe] >= 0).all(1) if F else valid
    fc = np.where(valid[:, None], vc[safe], -1)
    keep = kept_faces(fc, valid, fault)
    used = np.zeros(Nc, bool)
    used[fc[keep].reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    out_faces = new_id[fc[keep]].astype(np.int32).reshape(-1, 3)
    cluster = np.where((vc >= 0) & used[np.maximum(vc, 0)], new_id[np.maximum(vc, 0)], -1).astype(np.int32)
    out = dict(faces=out_faces, cluster=cluster, n_classes=C, dims=dims)
    if faces_only:
        return out
    g64, e64 = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(edge))
    members = np.nonzero(fin)[0]  # ascending input index; np.add.at adds in this order
    cidx = np.zeros((Nc, 3), np.int64)
    cidx[cl] = idx[members]
    o = g64[None, :] + (cidx + 0.5) * e64
    P = pos.astype(np.float64)
    n_mem = np.bincount(cl, minlength=Nc).astype(np.int64)
    sm = np.zeros((Nc, 3))
    np.add.at(sm, cl, P[members] - o[cl])
    m = sm / np.maximum(n_mem, 1)[:, None]
    lo, hi = g64[None, :] + cidx * e64, g64[None, :] + (cidx + 1.0) * e64
    np.minimum.at(lo, cl, P[members])
    np.maximum.at(hi, cl, P[members])
    # the quadrics: every valid face, dropped or not, in (face, corner) order
    vf = np.nonzero(valid)[0]
    a, u, w = P[faces[vf, 0]], P[faces[vf, 1]] - P[faces[vf, 0]], P[faces[vf, 2]] - P[faces[vf, 0]]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    rec_c = fc[vf].reshape(-1)  # record 3 f + corner
    rec_n, rec_a = np.repeat(n, 3, 0), np.repeat(a, 3, 0)
    q = rec_a - o[rec_c]
    d = (rec_n[:, 0] * q[:, 0] + rec_n[:, 1] * q[:, 1]) + rec_n[:, 2] * q[:, 2]
    A = np.zeros((Nc, 3, 3))
    b = np.zeros((Nc, 3))
    np.add.at(A, rec_c, rec_n[:, :, None] * rec_n[:, None, :])
    np.add.at(b, rec_c, rec_n * d[:, None])
    tr = (A[:, 0, 0] + A[:, 1, 1]) + A[:, 2, 2]
    lam = (RHO * tr) / 3.0
    x = m.copy()
    ok = tr > 0
    cond = 1.0
    if ok.any():
        if fault == "no_regulariser":
            Mx, rhs = A[ok], b[ok]
            x[ok] = np.stack([np.linalg.lstsq(Mx[i], rhs[i], rcond=None)[0] for i in range(len(Mx))])
        else:
            Mx, rhs = A[ok] + lam[ok, None, None] * np.eye(3), b[ok] + lam[ok, None] * m[ok]
            x[ok] = np.linalg.solve(Mx, rhs[..., None])[..., 0]
        with np.errstate(all="ignore"):
            cond = float(np.linalg.cond(Mx[used[ok]]).max()) if used[ok].any() else 1.0
    pos64 = np.clip(o + x, lo, hi)
    pos32 = pos64.astype(np.float32)
    # attributes
    S = np.zeros((Nc, 3), np.int64)
    np.add.at(S, cl, rows[members, 12:15].astype(np.int64))
    colour = ((2 * S + n_mem[:, None]) // np.maximum(2 * n_mem[:, None], 1)).astype(np.uint8)
    rb = row_bytes(C)
    sel = np.nonzero(used)[0]
    Vo = len(sel)
    out_rows = np.zeros((Vo, rb), np.uint8)
    written = pos32[sel] if world is None else apply_world(world, pos32[sel])
    out_rows[:, :12] = np.ascontiguousarray(written.astype("<f4")).view(np.uint8).reshape(Vo, 12)
    out_rows[:, 12:15] = colour[sel]
    abund64 = np.zeros((Vo, C))
    if C:
        label = np.clip(np.ascontiguousarray(rows[members, 15:19]).view("<i4").reshape(-1), -1, C - 1)  # (-1: nobody tinted the vertex)
        hist = np.zeros((Nc, C + 1), np.int64)
        np.add.at(hist, (cl, label + 1), 1)
        arg = ((C - np.argmax(hist[:, ::-1], 1)) if fault == "label_tie_last" else np.argmax(hist, 1)) - 1  # argmax: the first of the largest
        out_rows[:, 15:19] = np.ascontiguousarray(arg[sel].astype("<i4")).view(np.uint8).reshape(Vo, 4)
        ab = np.ascontiguousarray(rows[members, 19:]).view("<f4").reshape(-1, C).astype(np.float64)
        sa = np.zeros((Nc, C))
        np.add.at(sa, cl, ab)
        abund64 = (sa / np.maximum(n_mem, 1)[:, None])[sel]
        with np.errstate(all="ignore"):
            out_rows[:, 19:] = np.ascontiguousarray(abund64.astype("<f4")).view(np.uint8).reshape(Vo, 4 * C)
    # the bound's ingredients (properties of the input)
    L = np.bincount(rec_c, minlength=Nc)
    reach = np.zeros(Nc)
    if len(rec_c):
        np.maximum.at(reach, rec_c, np.linalg.norm(q, axis=1))
    reach = np.maximum(reach, np.linalg.norm(m, axis=1))
    L_max, M_max = (int(L[sel].max()), int(n_mem[sel].max())) if Vo else (0, 0)
    reach_max = float(reach[sel].max()) if Vo else 0.0
    K64 = 2.0 * (2 * L_max + M_max + 27) * (reach_max / e64)
    f64_term = K64 * COND_MAX * 2.0 ** -53 * e64
    box_mag = np.maximum(np.abs(lo[sel]), np.abs(hi[sel]))
    out.update(rows=out_rows, positions=pos32[sel], pos64=pos64[sel], abund64=abund64, pos_bound=0.5 * ulp32(box_mag) + f64_term,
               f64_term=f64_term, cond=cond, tr0=int((~ok[sel]).sum()) if Vo else 0, L_max=L_max, M_max=M_max, reach_max=reach_max)
    return out


def abundances_of(rows, C):
    return np.ascontiguousarray(np.asarray(rows, np.uint8)[:, 19:]).view("<f4").reshape(-1, C)


def abund_within(got_rows, want, C) -> bool:
    """Every abundance of ``got_rows`` within ABUND_ULPS float32 ulps of the float64 mean's rounding."""
    if not C or not len(got_rows):
        return True
    got = abundances_of(got_rows, C).astype(np.float64)
    w32 = want["abund64"].astype(np.float32).astype(np.float64)
    return bool((np.abs(got - w32) <= ABUND_ULPS * ulp32(w32)).all())


# ---- the search of --simplify-faces (restated) ---------------------------------------------------------------------------------------
def ladder_edge(h, k):
    return np.float32(float(np.float32(h)) * 2.0 ** (k / 4.0))


def rung_origin(lo, e):
    return (np.asarray(lo, np.float32) - np.float32(e) * np.float32(0.5)).astype(np.float32)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def volume_mesh(name, n=24, C=3):
    """The marching-tetrahedra mesh of a tests/mesh_ref.py volume on the n^3 cube lattice -> (rows, faces, lo, h)."""
    import mesh_ref as M

    lo, h, dims = M.cube_lattice(n)
    D, W, Wc, A = M.field(name, lo, h, dims, C=C)
    ex = M.extract(D, W, Wc, A, lo, h, dims)
    return ex["rows"], ex["faces"], lo, h


def hand_mesh(C=3):
    """About 20 faces with everything the rules name: a duplicate, a rotated duplicate, an opposite twin, a face degenerate on input, an
    index >= V and a negative one, a NaN vertex, an unused vertex, label ties, a label outside [0, C), and two zero-area faces whose
    three clusters have tr A = 0.  Grid: origin (0, 0, 0), edge 1; the vertices sit well inside their cells.
    -> (rows, faces, origin, edge)."""
    P = [
        (0.25, 0.25, 0.25), (0.5, 0.25, 0.375),      # 0 1   cell (0,0,0)
        (1.25, 0.25, 0.25), (1.5, 0.5, 0.25),        # 2 3   cell (1,0,0)
        (0.25, 1.25, 0.25), (0.5, 1.5, 0.375),       # 4 5   cell (0,1,0)
        (0.25, 0.25, 1.25),                          # 6     cell (0,0,1)
        (1.25, 1.25, 0.25), (1.5, 1.5, 0.5),         # 7 8   cell (1,1,0)
        (1.25, 0.25, 1.25),                          # 9     cell (1,0,1)
        (0.25, 1.25, 1.25),                          # 10    cell (0,1,1)
        (np.nan, 0.5, 0.5),                          # 11    NaN: no cluster
        (2.5, 2.5, 2.5),                             # 12    used by no face
        (3.25, 0.5, 0.5), (4.25, 0.5, 0.5), (5.25, 0.5, 0.5),  # 13 14 15  collinear: zero-area faces, tr A = 0
        (1.75, 1.25, 1.25),                          # 16    cell (1,1,1)
    ]
    Fs = [
        (0, 2, 4), (1, 3, 5),        # the same cluster triple: a duplicate (the first is kept)
        (5, 0, 3),                   # a rotated duplicate
        (0, 4, 2),                   # the opposite twin: kept
        (0, 0, 6), (2, 2, 2),        # degenerate on input
        (0, 1, 6),                   # degenerate after clustering
        (0, 17, 2), (0, -1, 2), (0, 2, 1 << 30),  # indices outside [0, V)
        (0, 11, 2),                  # a NaN vertex
        (13, 14, 15), (15, 14, 13),  # zero area, distinct clusters: tr A = 0 for the three
        (2, 7, 9), (4, 10, 7), (6, 9, 10), (7, 16, 9), (10, 16, 7), (9, 16, 10), (3, 8, 9), (5, 10, 8),
        (0, 6, 2), (2, 6, 9), (4, 6, 10),
    ]
    V = len(P)
    rng = np.random.default_rng(5)
    rb = row_bytes(C)
    rows = np.zeros((V, rb), np.uint8)
    rows[:, :12] = np.asarray(P, "<f4").view(np.uint8).reshape(V, 12)
    rows[:, 12:15] = rng.integers(0, 256, (V, 3))
    rows[0, 12:15], rows[1, 12:15] = (255, 0, 1), (254, 1, 2)  # sums that round up and down
    if C:
        label = rng.integers(0, C, V).astype("<i4")
        label[0], label[1] = 2, 1      # a tie of two members: the smaller label wins
        label[2], label[3] = C + 5, 0  # outside [0, C): clamped to C - 1, then a tie with 0
        label[4], label[5] = -7, 1     # below -1: clamped to -1 ("nobody tinted this vertex"), then a tie with 1
        rows[:, 15:19] = label.view(np.uint8).reshape(V, 4)
        rows[:, 19:] = rng.random((V, C)).astype("<f4").view(np.uint8).reshape(V, 4 * C)
    return rows, np.asarray(Fs, np.int32), np.zeros(3, np.float32), np.float32(1.0)
