"""Mesh components: a numpy restatement of csrc/umhs_components.hip, the float64 area oracle with its bound, and the case builders (plain
helper module, no tests).

Used by tests/test_components_cpu.py (the restatement against a flood fill, the float32 areas against the oracle, the keep rules) and
tests/test_hip_components.py (the kernels against it).  include/umhs_hip.h ("Mesh components") is the definition; this file follows it
rule for rule.  Labels, ids, counts, faces, the vertex map and row bytes are integers or copies: compared with ``==``.

THE AREA BOUND.  The kernel forms a face's area in float32, one rounded operation per step (u = 2^-24, the unit roundoff):
  * edge differences  e1 = fl(b - a), e2 = fl(c - a): each component carries a relative error of at most u;
  * cross product     n_x = fl(fl(e1y e2z) - fl(e1z e2y)): either product carries 2 u from its factors and u of its own, 3 u (|p| + |q|)
                      together, and the difference adds u |n_x| <= u (|p| + |q|):  |dn_x| <= 4 u (|e1y e2z| + |e1z e2y|) <= 4 u |e1| |e2|
                      (Cauchy-Schwarz), hence |dn| <= 4 sqrt(3) u |e1| |e2| < 6.93 u |e1| |e2| over the three components;
  * squares and sums  (n_x n_x + n_y n_y) + n_z n_z: three products and two sums of non-negative terms, a relative error of at most 3 u
                      of the squared norm, 1.5 u of the norm;
  * square root       correctly rounded: u of the norm.  The factor 0.5 is exact.
  |n| <= |e1| |e2|, so to first order  |area32 - area| <= 0.5 (6.93 + 2.5) u |e1| |e2| = 4.72 u |e1| |e2|; AREA_K = 6 covers the terms of
  second order (below 1e-6 of the first).  Squares of components below 2^-75 leave the normal range: an absolute 2^-72 per face covers
  what that can cost the norm.  Slivers cancel in the cross product, so the bound is in |e1| |e2| and never relative to the area.
A component's area is a float64 sum of n widened float32 values, in the kernel and here: either carries at most n 2^-53 of the sum.
  ->  |got - area64| <= sum over the faces of (AREA_K 2^-24 |e1| |e2| + 2^-72)  +  n 2^-52 area64,  per component (``area_oracle`` returns both)."""
from __future__ import annotations

import numpy as np

import simplify_ref as S

CHUNK = 256       # sorted positions per piece chunk, and faces / vertices per workgroup (ops.COMPONENTS_CHUNK)
AREA_K = 6.0
AREA_ABS = 2.0 ** -72
TABLE_ROWS = 16


def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def labels(V, faces):
    """int64 [V]: the smallest vertex of every vertex's component.  Union-find over the valid faces, the smaller root wins."""
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    for a, b, c in f[valid_faces(f, V)].tolist():
        ra, rb, rc = find(a), find(b), find(c)
        m = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = m
    return np.asarray([find(v) for v in range(V)], np.int64)


def face_areas32(pos, faces):
    """float32 [F]: the kernel's face area operation by operation (numpy's element-wise float32 operations round once each); 0 for an
    invalid face and for a face with a corner that is not finite."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, len(pos))
    g = np.where(ok[:, None], f, 0)
    if len(pos) == 0:
        return np.zeros(len(f), np.float32)
    a, b, c = pos[g[:, 0]], pos[g[:, 1]], pos[g[:, 2]]
    ok &= np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    with np.errstate(all="ignore"):
        u, w = b - a, c - a
        n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        area = np.float32(0.5) * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    assert area.dtype == np.float32
    return np.where(ok, area, np.float32(0)).astype(np.float32)


def _sequential_sum(x):
    return float(np.cumsum(np.asarray(x, np.float64))[-1]) if len(x) else 0.0  # (cumsum adds element by element)


def components(rows, faces, C):
    """-> dict(label int64 [V], vertex_component int32 [V], face_component int32 [F], n_components, faces int64 [K], vertices int64 [K],
    area float64 [K] (the kernel's sum: pieces cut at multiples of CHUNK sorted positions, added in order), face_area float32 [F])."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, S.row_bytes(C))
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V, F = len(rows), len(faces)
    lab = labels(V, faces)
    roots = np.nonzero(lab == np.arange(V))[0]
    rank = np.full(V, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    vc = rank[lab] if V else np.zeros(0, np.int64)
    ok = valid_faces(faces, V)
    fc = np.where(ok, vc[np.where(ok, faces[:, 0].astype(np.int64), 0)], -1) if V else np.full(F, -1, np.int64)
    K = len(roots)
    area32 = face_areas32(S.positions_of(rows), faces)
    order = np.argsort(fc, kind="stable")
    sorted_ids, a64 = fc[order], area32[order].astype(np.float64)
    start, end = np.searchsorted(sorted_ids, np.arange(K)), np.searchsorted(sorted_ids, np.arange(K) + 1)
    area = np.zeros(K)
    for c in np.nonzero(end > start)[0]:
        s, e = int(start[c]), int(end[c])
        cuts = [s] + list(range((s // CHUNK + 1) * CHUNK, e, CHUNK)) + [e]
        total = _sequential_sum(a64[cuts[0]:cuts[1]])
        for p, q in zip(cuts[1:-1], cuts[2:]):
            total = total + _sequential_sum(a64[p:q])
        area[c] = total
    return dict(label=lab, vertex_component=vc.astype(np.int32), face_component=fc.astype(np.int32), n_components=K,
                faces=(end - start).astype(np.int64), vertices=np.bincount(vc, minlength=K).astype(np.int64), area=area, face_area=area32)


def area_oracle(rows, faces, C, face_component, K):
    """(area64 [K], bound [K]): the areas in float64 from the float32 coordinates, and the bound of the module text."""
    pos = S.positions_of(np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, S.row_bytes(C))).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fc = np.asarray(face_component, np.int64)
    ok = fc >= 0
    g = np.where(ok[:, None], f, 0)
    area, per_face = np.zeros(K), np.zeros(K)
    if len(pos) == 0 or not ok.any():
        return area, per_face
    a, b, c = pos[g[:, 0]], pos[g[:, 1]], pos[g[:, 2]]
    fin = ok & np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        A = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
        term = AREA_K * 2.0 ** -24 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) + AREA_ABS
    np.add.at(area, fc[fin], A[fin])
    np.add.at(per_face, fc[fin], term[fin])
    n = np.bincount(fc[ok], minlength=K)
    return area, per_face + n * 2.0 ** -52 * area


# ---- the keep rules and the emit -----------------------------------------------------------------------------------------------------
def keep_mask(n_faces, min_component_faces=None, min_component_fraction=None, keep_largest_components=None):
    """bool [K]: a component is kept iff it has a face and meets every criterion given (export.component_keep_mask)."""
    nf = np.asarray(n_faces, np.int64)
    keep = nf > 0
    if len(nf) == 0:
        return keep
    if min_component_faces is not None:
        keep &= nf >= int(min_component_faces)
    if min_component_fraction is not None:
        keep &= np.asarray([int(n) >= float(min_component_fraction) * float(int(nf.max())) for n in nf], bool)
    if keep_largest_components is not None:
        by_size = sorted(range(len(nf)), key=lambda c: (-int(nf[c]), c))[:int(keep_largest_components)]  # ties: the smaller id
        top = np.zeros(len(nf), bool)
        top[by_size] = True
        keep &= top
    return keep


def table(comp, keep):
    """The summary's component table: the TABLE_ROWS largest kept components by faces, ties to the smaller id."""
    ids = sorted(np.nonzero(keep)[0].tolist(), key=lambda c: (-int(comp["faces"][c]), c))[:TABLE_ROWS]
    return [{"faces": int(comp["faces"][c]), "vertices": int(comp["vertices"][c]), "area": float(comp["area"][c])} for c in ids]


def emit(rows, faces, C, comp, keep, world=None):
    """-> dict(rows uint8 [V', rb], faces int32 [F', 3], positions float32 [V', 3] (model frame), vertex_map int32 [V])."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, S.row_bytes(C))
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(rows)
    fc = np.asarray(comp["face_component"], np.int64)
    keep = np.asarray(keep).astype(bool)
    fk = (fc >= 0) & (keep[np.maximum(fc, 0)] if len(keep) else False)
    used = np.zeros(V, bool)
    used[faces[fk].reshape(-1)] = True
    vmap = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    out = rows[used].copy()
    pos = S.positions_of(rows)[used] if V else np.zeros((0, 3), np.float32)
    if world is not None and len(out):
        with np.errstate(all="ignore"):
            out[:, :12] = np.ascontiguousarray(S.apply_world(world, pos).astype("<f4")).view(np.uint8).reshape(-1, 12)
    return dict(rows=out, faces=vmap[faces[fk]].astype(np.int32).reshape(-1, 3), positions=pos, vertex_map=vmap)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def random_rows(V, C, seed=0, scale=1.0):
    """V vertex rows of random positions in [-scale, scale]^3, colours, labels and abundances."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((V, S.row_bytes(C)), np.uint8)
    rows[:, :12] = (scale * (2.0 * rng.random((V, 3)) - 1.0)).astype("<f4").view(np.uint8).reshape(V, 12)
    rows[:, 12:15] = rng.integers(0, 256, (V, 3))
    if C:
        rows[:, 15:19] = rng.integers(0, C, V).astype("<i4").view(np.uint8).reshape(V, 4)
        rows[:, 19:] = rng.random((V, C)).astype("<f4").view(np.uint8).reshape(V, 4 * C)
    return rows


def strip_faces(n_faces, first=0, step=1):
    """A triangle strip: face i = (v_i, v_i+1, v_i+2) over the vertices first, first + step, ..."""
    i = first + step * np.arange(n_faces, dtype=np.int64)
    return np.stack([i, i + step, i + 2 * step], 1).astype(np.int32)


def permuted_strip(n_faces, C=3, seed=7):
    """A strip whose vertex indices are a seeded random permutation: one component, deep chains of falling labels."""
    V = n_faces + 2
    perm = np.random.default_rng(seed).permutation(V).astype(np.int32)
    return random_rows(V, C, seed), perm[strip_faces(n_faces)]


def fan(n_faces, C=0, seed=3):
    """n_faces round one hub, the LAST vertex: in the first round every face lowers the hub's parent."""
    V = n_faces + 2
    i = np.arange(n_faces, dtype=np.int32)
    return random_rows(V, C, seed), np.stack([np.full(n_faces, V - 1, np.int32), i, i + 1], 1)


def interleaved_strips(n_faces_each, C=3, seed=11):
    """Two strips, one over the even vertices and one over the odd: two components, labels 0 and 1."""
    V = 2 * (n_faces_each + 2)
    both = np.empty((2 * n_faces_each, 3), np.int32)
    both[0::2], both[1::2] = strip_faces(n_faces_each, 0, 2), strip_faces(n_faces_each, 1, 2)
    return random_rows(V, C, seed), both


def hand_mesh(C=3):
    """14 vertices with everything the rules name: an isolated vertex, a duplicate face, faces with repeated indices, an index >= V and a
    negative one (their faces join nothing), a NaN vertex (its face has area 0, is counted and connects), a component joined from a
    high index.  Components by smallest vertex: {0, 1, 2, 3, 13}, {4}, {5, 6}, {7}, {8, 9, 10}, {11}, {12}."""
    P = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0.25),   # 0..3  a bent quad
         (5, 5, 5),                                        # 4     isolated
         (2, 0, 0), (3, 0, 1),                             # 5 6   joined by a face with a repeated index
         (4, 4, 0),                                        # 7     named only by (7, 7, 7)
         (0, 0, 3), (np.nan, 1, 3), (1, 0, 3.5),           # 8 9 10  9 is not finite
         (6, 0, 0), (6, 1, 0),                             # 11 12 named only by invalid faces
         (0.5, 2, 0.125)]                                  # 13    joins the quad
    Fs = [(0, 1, 2), (0, 2, 3), (0, 1, 2),                 # the quad, one face twice
          (5, 5, 6), (7, 7, 7),                            # repeated indices: valid
          (8, 9, 10),                                      # a NaN corner
          (11, 12, 14), (11, -1, 12), (12, 11, 1 << 30),   # indices outside [0, V): invalid
          (13, 2, 3), (10, 8, 10)]
    V = len(P)
    rows = random_rows(V, C, seed=5)
    rows[:, :12] = np.asarray(P, "<f4").view(np.uint8).reshape(V, 12)
    return rows, np.asarray(Fs, np.int32)


# the meshes tests/test_hip_components.py labels, by name -> (rows, faces, C); built on demand, once
_CASES = {
    "random_c0": lambda: (*S.volume_mesh("random", 24, 0)[:2], 0),
    "random_c3": lambda: (*S.volume_mesh("random", 24, 3)[:2], 3),
    "sphere": lambda: (*S.volume_mesh("sphere", 24, 3)[:2], 3),
    "two_spheres": lambda: (*S.volume_mesh("two_spheres", 24, 3)[:2], 3),
    "permuted_strip": lambda: (*permuted_strip(8192, 3), 3),
    "fan": lambda: (*fan(10000, 0), 0),
    "interleaved_strips": lambda: (*interleaved_strips(700, 3), 3),
    "strip_chunk_minus_1": lambda: (random_rows(CHUNK + 1, 0, 1), strip_faces(CHUNK - 1), 0),
    "strip_chunk": lambda: (random_rows(CHUNK + 2, 0, 2), strip_faces(CHUNK), 0),
    "strip_chunk_plus_1": lambda: (random_rows(CHUNK + 3, 3, 3), strip_faces(CHUNK + 1), 3),
    "hand_c0": lambda: (*hand_mesh(0), 0),
    "hand_c3": lambda: (*hand_mesh(3), 3),
}
CASE_NAMES = tuple(_CASES)
_built = {}


def case(name):
    """(rows, faces, C, restatement) of a named case."""
    if name not in _built:
        rows, faces, C = _CASES[name]()
        _built[name] = (rows, faces, C, components(rows, faces, C))
    return _built[name]
