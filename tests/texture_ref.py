"""The texture atlas and the texel rays of the textured mesh export, restated in numpy (include/umhs_hip.h is THE definition).

Layout.  F >= 1 faces, p = px_per_uv_triangle >= 4, e = p - 3, S = ceil(F / 2) squares, Q = the least integer with Q^2 >= S, atlas side
T = Q p <= 16384.  Texel t = row T + col (row 0 on top) lies in square s = (row // p) Q + col // p at (i, j) = (col % p, row % p) and
belongs to face 2 s + (i + j >= p); a face index >= F is an empty texel.  Corners (texel centres): even face (0,0) (e,0) (0,e); odd
face (p-1,p-1) (2,p-1) (p-1,2).  The layout is this project's own, modelled on nerfstudio's per-triangle "custom" unwrap
[upstream-recalled, in spirit only].

``inset`` and ``swap`` exist for the planted faults of tests/test_texture_cpu.py: the definition is ``inset = 3, swap = False``.

Rays.  ``rays(..., F=np.float32)`` replays umhs_texture_rays operation for operation (numpy rounds every float32 operation once and
fuses nothing; its float32 sqrt and division are correctly rounded); ``F=np.float64`` evaluates the same definition in float64."""
import numpy as np

MAX_SIDE = 16384
MISS = np.float32(1e10)


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def atlas(n_faces: int, p: int):
    """-> (Q, T); ValueError for p < 4, F < 1 (the C entry's UMHS_ERR_ARG), OverflowError for T > 16384 (UMHS_ERR_UNSUPPORTED)."""
    if p < 4 or n_faces < 1:
        raise ValueError((n_faces, p))
    S = (n_faces + 1) // 2
    Q = 1
    while Q * Q < S and Q <= MAX_SIDE:  # a walk on purpose: the definition, not a formula for it
        Q += 1
    T = Q * p
    if T > MAX_SIDE:
        raise OverflowError(T)
    return Q, T


def owner_map(n_faces: int, p: int, swap: bool = False) -> np.ndarray:
    """int32 [T, T]: the face of every texel, -1 where nobody owns it."""
    Q, T = atlas(n_faces, p)
    row, col = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    i, j = col % p, row % p
    k = (i + j >= p).astype(np.int64)
    if swap:
        k = 1 - k
    f = 2 * ((row // p) * Q + col // p) + k
    return np.where(f < n_faces, f, -1).astype(np.int32)


def corners_local(odd: int, p: int, inset: int = 3):
    """The three corners (i, j) of a face in its square."""
    e = p - inset
    return [(p - 1, p - 1), (p - 1 - e, p - 1), (p - 1, p - 1 - e)] if odd else [(0, 0), (e, 0), (0, e)]


def square_of(f: int, Q: int):
    s = f // 2
    return s % Q, s // Q  # (sx, sy)


def numerators(i, j, odd, p: int, inset: int = 3):
    """Barycentric numerators (n0, n1, n2) over e = p - inset of lattice point (i, j) for the even / odd face of a square."""
    e = p - inset
    n1 = np.where(odd, p - 1 - i, i)
    n2 = np.where(odd, p - 1 - j, j)
    return e - n1 - n2, n1, n2


def uv(n_faces: int, p: int) -> np.ndarray:
    """float32 [F, 3, 2]: one rounded float32 division of exact integers each."""
    Q, T = atlas(n_faces, p)
    out = np.empty((n_faces, 3, 2), np.float32)
    den = np.float32(2 * T)
    for f in range(n_faces):
        sx, sy = square_of(f, Q)
        for c, (ic, jc) in enumerate(corners_local(f & 1, p)):
            out[f, c, 0] = np.float32(2 * (sx * p + ic) + 1) / den
            out[f, c, 1] = np.float32(2 * (T - (sy * p + jc)) - 1) / den
    return out


# ---- the properties ----------------------------------------------------------------------------------------------------------------
def check_single_owner(n_faces: int, p: int) -> None:
    """Every texel has at most one owner, every texel of a used square exactly one, and the even face owns i + j <= p - 1."""
    Q, T = atlas(n_faces, p)
    own = owner_map(n_faces, p)
    assert own.shape == (T, T) and own.max() == n_faces - 1
    counts = np.bincount(own[own >= 0], minlength=n_faces)
    assert (counts[0::2] == p * (p + 1) // 2).all() and (counts[1::2] == p * (p - 1) // 2).all()  # (sums to p^2 per full square)
    for f in range(n_faces):
        sx, sy = square_of(f, Q)
        sq = own[sy * p:(sy + 1) * p, sx * p:(sx + 1) * p]
        assert set(np.unique(sq).tolist()) <= {2 * (f // 2), 2 * (f // 2) + 1, -1}


def check_corners(n_faces: int, p: int, inset: int = 3, swap: bool = False) -> None:
    """Each face's three corners are texel centres it owns, with numerators (e,0,0), (0,e,0), (0,0,e)."""
    Q, T = atlas(n_faces, p)
    own = owner_map(n_faces, p, swap)
    e = p - inset
    for f in range(n_faces):
        sx, sy = square_of(f, Q)
        for c, (ic, jc) in enumerate(corners_local(f & 1, p, inset)):
            assert 0 <= ic < p and 0 <= jc < p
            assert own[sy * p + jc, sx * p + ic] == f, (f, c, ic, jc, int(own[sy * p + jc, sx * p + ic]))
            n = [int(v) for v in numerators(ic, jc, bool(f & 1), p, inset)]
            assert n == [e if k == c else 0 for k in range(3)], (f, c, n)


def check_bilinear(n_faces: int, p: int, inset: int = 3, swap: bool = False, grid: int = 12) -> None:
    """For a dense rational grid of points of each UV triangle (barycentric numerators a + b + c = grid, edges and corners included)
    every texel of the bilinear footprint that carries weight is owned by the face and lies in its square.  Coordinates are exact
    fractions over ``grid``: a point on a lattice line has one neighbour on that axis, not two."""
    Q, T = atlas(n_faces, p)
    own = owner_map(n_faces, p, swap)
    for f in range(n_faces):
        sx, sy = square_of(f, Q)
        (i0, j0), (i1, j1), (i2, j2) = corners_local(f & 1, p, inset)
        for a in range(grid + 1):
            for b in range(grid + 1 - a):
                c = grid - a - b
                xn, yn = a * i0 + b * i1 + c * i2, a * j0 + b * j1 + c * j2  # coordinates times grid
                xs = [xn // grid] if xn % grid == 0 else [xn // grid, xn // grid + 1]
                ys = [yn // grid] if yn % grid == 0 else [yn // grid, yn // grid + 1]
                for x in xs:
                    for y in ys:
                        assert 0 <= x < p and 0 <= y < p, (f, x, y)
                        assert own[sy * p + y, sx * p + x] == f, (f, (a, b, c), (x, y), int(own[sy * p + y, sx * p + x]))


# ---- texel rays --------------------------------------------------------------------------------------------------------------------
def rays(positions, faces, p: int, ray_length, begin: int = 0, end=None, F=np.float32):
    """-> {"origins", "directions" [n,3], "nears", "fars" [n], "texel_face" int32 [n], "bary" [n,3], "point" [n,3] (P of step 2),
    "normal" [n,3] (the unit normal), "mag" [n,3] (sum_k |w_k| |V_kc|)} in precision F, outputs indexed from ``begin``."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nF, V = len(faces), len(positions)
    Q, T = atlas(nF, p)
    end = T * T if end is None else end
    assert 0 <= begin <= end <= T * T
    t = np.arange(begin, end, dtype=np.int64)
    n = len(t)
    row, col = t // T, t % T
    i, j = col % p, row % p
    odd = i + j >= p
    f = 2 * ((row // p) * Q + col // p) + odd
    owned = f < nF
    fc = np.where(owned, f, 0)
    idx = faces[fc].astype(np.int64)
    inside = owned & ((idx >= 0) & (idx < V)).all(1)
    idx = np.where(inside[:, None], idx, 0)
    with np.errstate(all="ignore"):
        v0, v1, v2 = (positions[idx[:, k]].astype(F) for k in range(3))
        a, b = v1 - v0, v2 - v0
        nrm = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        q = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        live = inside & (q > 0) & np.isfinite(q)
        r = np.sqrt(q)
        unit = nrm / r[:, None]
        e = F(p - 3)
        w = np.stack([num.astype(F) / e for num in numerators(i, j, odd, p)], 1)
        point = (w[:, 0:1] * v0 + w[:, 1:2] * v1) + w[:, 2:3] * v2
        mag = (np.abs(w[:, 0:1] * v0) + np.abs(w[:, 1:2] * v1)) + np.abs(w[:, 2:3] * v2)
        L = F(np.float32(ray_length))
        origin = point + (F(0.5) * L) * unit
    lv = live[:, None]
    out = {"origins": np.where(lv, origin, F(0)), "directions": np.where(lv, -unit, np.array([0, 0, 1], F)),
           "nears": np.where(live, F(0), F(MISS)), "fars": np.where(live, L, F(MISS)),
           "texel_face": np.where(live, f, -1).astype(np.int32), "bary": np.where(lv, w, F(0)),
           "point": np.where(lv, point, F(0)), "normal": np.where(lv, unit, F(0)), "mag": np.where(lv, mag, F(0))}
    assert all(v.shape[0] == n for v in out.values())
    return {k: (v if k == "texel_face" else v.astype(F)) for k, v in out.items()}


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    """4 vertices, 4 faces, right-hand normals outwards."""
    pos = np.array([[0.31, 0.07, 0.93], [0.87, -0.41, -0.29], [-0.77, -0.53, -0.37], [0.05, 0.91, -0.43]], np.float32)
    faces = np.array([[0, 1, 3], [0, 3, 2], [0, 2, 1], [1, 2, 3]], np.int32)
    centre = pos.mean(0)
    for fa in faces:  # (the fixture's own orientation check)
        nrm = np.cross(pos[fa[1]] - pos[fa[0]], pos[fa[2]] - pos[fa[0]])
        assert nrm @ (pos[fa].mean(0) - centre) > 0
    return pos, faces


def dead_mesh():
    """F = 7 (the last square half empty), V = 6: faces 1, 3, 4 and 6 are dead -- zero area (collinear), a repeated vertex, an index
    equal to V, an index of -1."""
    pos = np.array([[0.1, 0.2, 0.3], [1.1, 0.2, 0.3], [2.1, 0.2, 0.3], [0.3, 1.4, -0.2], [-0.6, 0.5, 0.9], [0.8, -0.7, 1.3]], np.float32)
    faces = np.array([[0, 1, 3], [0, 1, 2], [1, 4, 5], [3, 3, 5], [0, 6, 2], [2, 5, 4], [-1, 1, 3]], np.int32)
    return pos, faces, [1, 3, 4, 6]


def sphere_mesh(n: int = 12):
    """The marching-tetrahedra sphere of tests/mesh_ref.py on an n^3 lattice -> (positions float32 [V,3], faces int32 [F,3])."""
    import mesh_ref as M

    lo, h, dims = M.cube_lattice(n)
    D, W, Wc, A = M.field("sphere", lo, h, dims, C=0)
    got = M.extract(D, W, Wc, A, lo, h, dims)
    pos = np.ascontiguousarray(got["rows"][:, :12]).view("<f4").reshape(-1, 3)
    return pos.astype(np.float32), np.ascontiguousarray(got["faces"], dtype=np.int32)


# ---- files -------------------------------------------------------------------------------------------------------------------------
def read_textured_obj(path):
    """A hand-written reader of the OBJ the export writes -> {"mtllib", "usemtl", "v" float32 [V,3], "vt" float32 [3F,2], "f" int64
    [F,3], "ft" int64 [F,3] (0-based), "tokens": the float tokens as written}."""
    out = {"mtllib": None, "usemtl": None, "tokens": []}
    v, vt, f, ft = [], [], [], []
    for ln in open(path, "r", encoding="ascii").read().splitlines():
        w = ln.split()
        if w[0] in ("mtllib", "usemtl"):
            assert out[w[0]] is None and len(w) == 2
            out[w[0]] = w[1]
        elif w[0] == "v":
            assert len(w) == 4 and not vt and not f
            v.append([np.float32(x) for x in w[1:]])
            out["tokens"] += w[1:]
        elif w[0] == "vt":
            assert len(w) == 3 and not f
            vt.append([np.float32(x) for x in w[1:]])
            out["tokens"] += w[1:]
        elif w[0] == "f":
            assert len(w) == 4
            pairs = [x.split("/") for x in w[1:]]
            assert all(len(pr) == 2 for pr in pairs)
            f.append([int(pr[0]) - 1 for pr in pairs])
            ft.append([int(pr[1]) - 1 for pr in pairs])
        else:
            raise AssertionError(ln)
    out.update(v=np.array(v, np.float32).reshape(-1, 3), vt=np.array(vt, np.float32).reshape(-1, 2), f=np.array(f, np.int64).reshape(-1, 3),
               ft=np.array(ft, np.int64).reshape(-1, 3))
    return out


def read_mtl(path):
    """-> {"newmtl": name, "map_Kd": file}."""
    out = {}
    for ln in open(path, "r", encoding="ascii").read().splitlines():
        w = ln.split()
        if w and w[0] in ("newmtl", "map_Kd"):
            out[w[0]] = w[1]
    return out
