"""Regional material edits: the float32 replay of the membership rule, the numpy segment builder, the cases, their float32 / float64
oracle runs, the comparators and the float64 regional render (plain helper module, no tests in it).  It mirrors tests/material_f64.py
for csrc/umhs_region.hip.

Used by tests/test_hip_region.py (the five kernels and the regional render on the GPU) and tests/test_region_cpu.py (the parser, the
replay against float64, the comparators on the float32 oracle and on planted faults; K is measured there).

Statements (include/umhs_hip.h, "Regional material edits"):
  membership   exact float32, every step one rounded operation: ``classify32`` replays it with numpy float32 scalars-in-arrays (numpy
               never fuses a product with a sum).  A decision, compared bit for bit.
  segments     maximal runs of one ray's samples with one region id: ``build_segments``.  Integers, compared for equality.
  sigma        sigma'[n] = sigma[n] max(0, 1 + sum_c (d[k_n][c] - 1) a[n,c])
  segment_sum  out[r] = the rows ray_seg[r] names, added in order
  remix        m_j[b] = sum_{c<C} mix16_seg[j,c] E''[k_j][c,b];  spectral2[r] = sum_j m_j;  specular[r] = sum_j s[k_j] comp_specular_seg[j];
               spectral = spectral2 + specular  (without the specular head: spectral = the mixing term)

ONE RULE for every output element:   |got - ref64| <= K u (mag + tiny),   u = 2^-24,   tiny = 2^-126,   mag = the sum of the absolute
terms (sigma: |sigma| (1 + sum_c |(d - 1) a|), as tests/material_f64.py).

K per family = max(8, 4 x the float32 CPU oracle's worst ratio over the committed cases, rounded up to a power of two).  Measured on the
CPU (``measure_worst``: float32 oracle, worst |diff| / (u (mag + tiny)) over all cases; tests/test_region_cpu.py re-measures and asserts
4 x worst <= K):
  remix spectral 2.97 | spectral2 2.96 | specular 4.26 | segment_sum 4.68 | sigma 3.18
so K = 32 for remix (one K for the family: 4 x 4.26 = 17.0, the specular sum of up to 17 rounded products of one sign) and for
segment_sum (4 x 4.68 = 18.7), 16 for sigma (4 x 3.18 = 12.7).  None is taken from the kernels.

Teeth: at least 90 % of the elements on rays with segments (remix, segment_sum) / of all elements (sigma) have |ref64| > 16 x bound;
checked on the float64 run alone (``teeth_failures``): remix >= 0.9993, segment_sum 1.0, sigma >= 0.968 in every case.

The regional render (``regional_render``) is composed from oracle/torch_ref.py as tests/material_f64.edited_render is, with the
per-sample layer (from the float32 replay: membership is a definition) choosing the density gains, the dictionary and the specular gain."""
from __future__ import annotations

import copy
from typing import Dict, List, Optional

import numpy as np
import torch

from material_f64 import REMIX_CASES, make_sigma_case, teeth_failures  # noqa: F401
from oracle import torch_ref as T
from rays_f64 import TINY, U, check  # noqa: F401

K_REMIX = 32.0
K_SIGMA = 16.0
K_SEGSUM = 32.0
MARGIN = 1e-5  # float32 and float64 membership agree for every point farther than this from a face (coordinates within +-4)
SEGMENTS_PER_RAY = (1, 0, 2, 5, 17)  # cycled over the rays of a case
REGION_KS = (1, 8)
BIG_CASE = (9, 256, 15, True)  # (K = 8: nine dictionaries of 15 KB, more than is staged in LDS)
SIGMA_NS = (0, 1, 63, 64, 65, 1000, 4099)


# ------------------------------------------------------------------------------------------------------------------------------ #
# membership
# ------------------------------------------------------------------------------------------------------------------------------ #
def rotation(rx: float, ry: float, rz: float) -> np.ndarray:
    """R = Rz Ry Rx in float64, rounded once to float32 (export.obb_from_params)."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def box_record(center, rot, scale) -> np.ndarray:
    rec = np.zeros(16, np.float32)
    rec[0:3], rec[3:12], rec[12:15] = center, rotation(*rot).reshape(9), scale
    return rec


def sphere_record(center, radius) -> np.ndarray:
    rec = np.zeros(16, np.float32)
    rec[0:3], rec[3:12], rec[12], rec[15] = center, np.eye(3, dtype=np.float32).reshape(9), radius, 1.0
    return rec


def make_table(K: int, seed: int = 0) -> np.ndarray:
    """K overlapping regions around the origin, boxes (rotated) and spheres alternating."""
    rng = np.random.default_rng(100 + 7 * K + seed)
    recs = []
    for k in range(K):
        c = rng.uniform(-0.6, 0.6, 3)
        if k % 2 == 0:
            recs.append(box_record(c, rng.uniform(-1.0, 1.0, 3), rng.uniform(0.5, 1.4, 3)))
        else:
            recs.append(sphere_record(c, rng.uniform(0.4, 0.9)))
    return np.stack(recs)


def _inside32(p: np.ndarray, rec: np.ndarray) -> np.ndarray:
    f = np.float32
    p, rec = p.astype(f), rec.astype(f)
    with np.errstate(invalid="ignore", over="ignore"):
        e = [p[:, i] - rec[i] for i in range(3)]
        if rec[15] != 0:
            return ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) < rec[12] * rec[12]
        R = rec[3:12]
        ok = np.ones(len(p), bool)
        for k in range(3):
            q = (R[k] * e[0] + R[3 + k] * e[1]) + R[6 + k] * e[2]
            h = rec[12 + k] * f(0.5)
            ok &= (q < h) & (q > -h)
        return ok


def classify32(p: np.ndarray, table: np.ndarray) -> np.ndarray:
    """The definition, every step rounded to float32: the first region that contains the point (1..K), 0 for none."""
    out = np.zeros(len(p), np.uint8)
    for k in range(len(table) - 1, -1, -1):
        out[_inside32(p, table[k])] = k + 1
    return out


def classify64(p: np.ndarray, table: np.ndarray):
    """The same rule in float64 on the float32 inputs -> (ids, distance of each point to the nearest face of any region)."""
    p, table = p.astype(np.float64), table.astype(np.float64)
    out, dist = np.zeros(len(p), np.uint8), np.full(len(p), np.inf)
    for k in range(len(table) - 1, -1, -1):
        rec = table[k]
        e = p - rec[0:3]
        if rec[15] != 0:
            r = np.sqrt((e * e).sum(1))
            inside, d = r < rec[12], np.abs(r - rec[12])
        else:
            q = e @ rec[3:12].reshape(3, 3)  # q_k = column k of R against e
            h = rec[12:15] * 0.5
            inside, d = (np.abs(q) < h).all(1), np.abs(np.abs(q) - h).min(1)
        out[inside] = k + 1
        dist = np.minimum(dist, d)
    return out, dist


def on_face_points(table: np.ndarray) -> np.ndarray:
    """Points whose float32 replay lands EXACTLY on a face (q == h) or at the radius (|e|^2 == r^2): axis-aligned boxes and spheres
    with dyadic numbers, where every step is exact."""
    pts = []
    for rec in table:
        if rec[15] != 0:
            pts += [rec[0:3] + np.float32(rec[12]) * np.array(a, np.float32) for a in ((1, 0, 0), (0, -1, 0), (0, 0, 1))]
        elif np.array_equal(rec[3:12].reshape(3, 3), np.eye(3, dtype=np.float32)):
            for k in range(3):
                for sgn in (1.0, -1.0):
                    v = rec[0:3].copy()
                    v[k] += np.float32(sgn) * rec[12 + k] * np.float32(0.5)
                    pts.append(v)
    return np.asarray(pts, np.float32).reshape(-1, 3)


DYADIC_TABLE = np.stack([box_record((0.25, -0.5, 0.125), (0.0, 0.0, 0.0), (1.0, 0.5, 2.0)), sphere_record((-0.5, 0.25, 0.0), 0.75),
                         box_record((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (4.0, 4.0, 4.0))])


def make_points(n: int, table: np.ndarray, seed: int = 0) -> np.ndarray:
    """n positions in [-1.5, 1.5]^3 with NaN rows, an infinite row and, where the table has them, points exactly on faces."""
    rng = np.random.default_rng(5 + n + seed)
    p = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    planted = on_face_points(table)
    m = min(len(planted), n // 4)
    if m:
        p[1:1 + m] = planted[:m]
    if n >= 8:
        p[n // 2, 1] = np.nan
        p[n // 2 + 1] = np.nan
        p[n - 1, 0] = np.inf
    return p


# ------------------------------------------------------------------------------------------------------------------------------ #
# segments
# ------------------------------------------------------------------------------------------------------------------------------ #
def build_segments(region: np.ndarray, ray_indices: np.ndarray, packed_info: np.ndarray) -> Dict[str, np.ndarray]:
    n, R = len(region), len(packed_info)
    head = np.zeros(n, bool)
    if n:
        head[0] = True
        head[1:] = (ray_indices[1:] != ray_indices[:-1]) | (region[1:] != region[:-1])
    seg_of = np.cumsum(head).astype(np.int64) - 1
    first = np.flatnonzero(head).astype(np.int64)
    S = len(first)
    seg_info = np.stack([first, np.diff(np.append(first, n))], 1).astype(np.int64).reshape(S, 2)
    ray_seg = np.zeros((R, 2), np.int64)
    for r in range(R):
        s0 = int(np.clip(packed_info[r, 0], 0, n))
        cnt = int(np.clip(packed_info[r, 1], 0, n - s0))
        f = int(seg_of[s0]) if s0 < n else S
        ray_seg[r] = (f, int(seg_of[s0 + cnt - 1]) - f + 1 if cnt > 0 else 0)
    return dict(seg_of=seg_of, seg_info=seg_info, seg_layer=region[first].astype(np.int32), ray_seg=ray_seg, S=S)


def make_stream(counts, pattern: str, K: int = 3, seed: int = 0):
    """A sample stream with ``counts[r]`` samples on ray r -> (region [N] uint8, ray_indices [N], packed_info [R,2]).
    ``pattern``: "alternate" (another id on every sample: S = N), "single" (one id throughout: S = the non-empty rays), "runs"
    (random run lengths of 1..200: runs cross wave and block boundaries)."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    ray = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    pinfo = np.stack([np.cumsum(counts) - counts, counts], 1).astype(np.int64).reshape(len(counts), 2)
    rng = np.random.default_rng(17 + n + seed)
    if pattern == "alternate":
        region = (np.arange(n) % 2 + 1).astype(np.uint8)
    elif pattern == "single":
        region = np.full(n, 2, np.uint8)
    else:
        region = np.zeros(n, np.uint8)
        i = 0
        while i < n:
            run = int(rng.integers(1, 201))
            region[i:i + run] = rng.integers(0, K + 1)
            i += run
    return region, ray, pinfo


def ray_counts(n: int, seed: int = 0) -> np.ndarray:
    """Per-ray sample counts adding up to n: empty rays at the start, in the middle and at the end, one-sample rays, long rays."""
    rng = np.random.default_rng(3 + n + seed)
    counts, left = [0, 0], n
    while left > 0:
        c = int(min(left, rng.choice([1, 1, 3, 40, 300, 700])))
        counts += [c] + ([0] if rng.random() < 0.3 else [])
        left -= c
    return np.asarray(counts + [0, 0], np.int64)


# ------------------------------------------------------------------------------------------------------------------------------ #
# sigma, segment_sum, remix
# ------------------------------------------------------------------------------------------------------------------------------ #
def make_sigma_regions_case(n: int, C: int, K: int, seed: int = 0) -> Dict:
    case = make_sigma_case(n, C, seed)
    g = torch.Generator().manual_seed(77 + n + 5 * C + K)
    case["region"] = torch.randint(0, K + 1, (n,), generator=g).to(torch.uint8)
    gains = torch.tensor([0.0, 1.0, 2.5, 0.5])[torch.randint(0, 4, (K + 1, C), generator=g)]
    gains[:, 0] = torch.tensor([2.5, 0.5])[torch.arange(K + 1) % 2]  # (no layer removes everything: a whole layer of zeros has no teeth)
    case["gain"], case["K"] = gains, K
    return case


def sigma_regions_oracle(case: Dict, dtype, layer_of=None) -> torch.Tensor:
    k = (case["region"] if layer_of is None else layer_of).long()
    a, d = case["a"].to(dtype), case["gain"].to(dtype)[k]
    acc = torch.zeros(case["n"], dtype=dtype)
    for c in range(case["C"]):
        acc = acc + (d[:, c] - 1.0) * a[:, c]
    return case["sigma"].to(dtype) * (1.0 + acc).clamp(min=0.0)


def sigma_regions_envelope(case: Dict) -> torch.Tensor:
    a, d = case["a"].double(), case["gain"].double()[case["region"].long()]
    return case["sigma"].double().abs() * (1.0 + ((d - 1.0) * a).abs().sum(1)) + TINY


def check_sigma_regions(case: Dict, got, r64, report=None) -> List[str]:
    fails = check("sigma", got, r64, sigma_regions_envelope(case), K_SIGMA, report)
    if bool((got.detach().cpu() < 0).any()):
        fails.append("sigma: negative densities")
    return fails


def region_case_id(c) -> str:
    return f"R{c[0]}-B{c[1]}-C{c[2]}-{'spec' if c[3] else 'nospec'}-K{c[4]}"


REGION_CASES = [c + (K,) for c in REMIX_CASES for K in REGION_KS] + [BIG_CASE + (8,)]


def make_region_case(R: int, B: int, C: int, specular: bool, K: int, seed: int = 0) -> Dict:
    """Per-segment sums with NaN in the mix columns >= C, 0 / 1 / 2 / 5 / 17 segments per ray, a layer per segment, K + 1 dictionaries
    with rows of both signs, the per-segment specular term and K + 1 specular gains."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + 3 * B + C + 13 * K)
    nseg = torch.tensor([SEGMENTS_PER_RAY[r % 5] for r in range(R)], dtype=torch.int64)
    first = torch.cumsum(nseg, 0) - nseg
    S = int(nseg.sum())
    mix = torch.rand(S, 16, generator=g) * 3.0
    mix[:, C:] = float("nan")
    E = torch.rand(K + 1, C, B, generator=g) * 2.0 - 0.5
    if C > 1:
        E[:, ::2] *= -1.0
    layer = torch.randint(0, K + 1, (S,), generator=g).to(torch.int32)
    cs = torch.rand(S, B, generator=g) if specular else None
    s = (torch.rand(K + 1, generator=g) * 1.5 + 0.25) if specular else torch.ones(K + 1)
    return dict(R=R, B=B, C=C, K=K, S=S, mix=mix, E=E, comp_specular=cs, s=s, seg_layer=layer,
                ray_seg=torch.stack([first, nseg], 1).reshape(R, 2), empty=nseg == 0)


def ordered_sum(rows: torch.Tensor, ray_seg: torch.Tensor) -> torch.Tensor:
    """out[r] = rows[first], then + rows[first + 1], ... in ``rows``' dtype, one rounded add each; no segment: zeros."""
    R = ray_seg.shape[0]
    out = torch.zeros((R,) + tuple(rows.shape[1:]), dtype=rows.dtype)
    first, num = ray_seg[:, 0], ray_seg[:, 1]
    for t in range(int(num.max()) if R else 0):
        on = num > t
        term = rows[first[on] + t]
        out[on] = term if t == 0 else out[on] + term
    return out


def remix_regions_oracle(case: Dict, dtype, seg_layer=None, ray_seg=None) -> Dict[str, torch.Tensor]:
    """The statement in ``dtype``.  ``seg_layer`` / ``ray_seg``: other tables (planted faults)."""
    layer = (case["seg_layer"] if seg_layer is None else seg_layer).long()
    rs = case["ray_seg"] if ray_seg is None else ray_seg
    mix, E = case["mix"].to(dtype), case["E"].to(dtype)[layer]  # [S,C,B]
    m = torch.zeros(case["S"], case["B"], dtype=dtype)
    for c in range(case["C"]):
        m = m + mix[:, c:c + 1] * E[:, c]
    term = ordered_sum(m, rs)
    if case["comp_specular"] is None:
        return {"spectral": term}
    sp = ordered_sum(case["s"].to(dtype)[layer][:, None] * case["comp_specular"].to(dtype), rs)
    return {"spectral": term + sp, "spectral2": term, "specular": sp}


def remix_regions_envelopes(mix, E, comp_specular, s, seg_layer, ray_seg) -> Dict[str, torch.Tensor]:
    """``mag + tiny`` per output, float64 (takes arrays: the model tests call it on what a render handed the kernel)."""
    layer, rs = seg_layer.detach().cpu().long(), ray_seg.detach().cpu()
    E = E.detach().double().cpu()
    C = E.shape[1]
    m = torch.einsum("sc,scb->sb", mix.detach().double().cpu()[:, :C].abs(), E[layer].abs())
    m = ordered_sum(m, rs)
    if comp_specular is None:
        return {"spectral": m + TINY}
    sp = ordered_sum((s.detach().double().cpu()[layer][:, None] * comp_specular.detach().double().cpu()).abs(), rs)
    return {"spectral": m + sp + TINY, "spectral2": m + TINY, "specular": sp + TINY}


def check_remix_regions(case: Dict, got: Dict, r64: Dict, report=None, prefix="") -> List[str]:
    env = remix_regions_envelopes(case["mix"], case["E"], case["comp_specular"], case["s"], case["seg_layer"], case["ray_seg"])
    live = ~case["empty"][:, None]
    if sorted(got) != sorted(r64):
        return [f"{prefix}outputs {sorted(got)}, want {sorted(r64)}"]
    fails: List[str] = []
    for k in r64:
        fails += check(prefix + k, got[k], r64[k], env[k], K_REMIX, report, teeth_mask=live)
        if case["R"] and bool((got[k].detach().cpu()[case["empty"]] != 0).any()):
            fails.append(f"{prefix}{k}: a ray without segments did not give an exact 0")
    return fails


def make_segsum_case(R: int, k: int, seed: int = 0) -> Dict:
    g = torch.Generator().manual_seed(9 * R + k + seed)
    nseg = torch.tensor([SEGMENTS_PER_RAY[r % 5] for r in range(R)], dtype=torch.int64)
    first = torch.cumsum(nseg, 0) - nseg
    S = int(nseg.sum())
    values = torch.rand(S, k, generator=g) * 2.0 - 0.25  # mostly positive, some negative: sums keep their teeth
    return dict(R=R, k=k, S=S, values=values, ray_seg=torch.stack([first, nseg], 1).reshape(R, 2), empty=nseg == 0)


def segsum_oracle(case: Dict, dtype, ray_seg=None) -> torch.Tensor:
    return ordered_sum(case["values"].to(dtype), case["ray_seg"] if ray_seg is None else ray_seg)


def check_segsum(case: Dict, got, r64, report=None) -> List[str]:
    env = ordered_sum(case["values"].double().abs(), case["ray_seg"]) + TINY
    fails = check("segment_sum", got, r64, env, K_SEGSUM, report, teeth_mask=~case["empty"][:, None])
    if case["R"] and bool((got.detach().cpu()[case["empty"]] != 0).any()):
        fails.append("segment_sum: a ray without segments did not give an exact 0")
    return fails


SEGSUM_CASES = [(c[0], k) for c in REMIX_CASES for k in (c[1], c[2])]
SIGMA_CASES = [(n, C, K) for n in SIGMA_NS for C, K in ((1, 1), (3, 8), (15, 8), (15, 1))]


def measure_worst() -> Dict[str, float]:
    """The float32 oracle's worst |diff| / (u (mag + tiny)) per family over the committed cases (what K is chosen from)."""
    worst = {"spectral": 0.0, "spectral2": 0.0, "specular": 0.0, "segment_sum": 0.0, "sigma": 0.0}
    for c in REGION_CASES:
        case, report = make_region_case(*c), {}
        assert not check_remix_regions(case, remix_regions_oracle(case, torch.float32), remix_regions_oracle(case, torch.float64), report)
        for k, v in report.items():
            worst[k] = max(worst[k], v["worst"])
    for c in SEGSUM_CASES:
        case, report = make_segsum_case(*c), {}
        assert not check_segsum(case, segsum_oracle(case, torch.float32), segsum_oracle(case, torch.float64), report)
        worst["segment_sum"] = max(worst["segment_sum"], report["segment_sum"]["worst"])
    for c in SIGMA_CASES:
        case, report = make_sigma_regions_case(*c), {}
        assert not check_sigma_regions(case, sigma_regions_oracle(case, torch.float32), sigma_regions_oracle(case, torch.float64), report)
        worst["sigma"] = max(worst["sigma"], report["sigma"]["worst"])
    return worst


# ------------------------------------------------------------------------------------------------------------------------------ #
# the regional render
# ------------------------------------------------------------------------------------------------------------------------------ #
def regional_render(p: T.FieldParams, E_all: torch.Tensor, d_all: torch.Tensor, s_all: torch.Tensor, layer: torch.Tensor, origins,
                    directions, starts, ends, ray_indices, num_rays: int, temperature: float, colour_M,
                    contraction: bool = True) -> Dict[str, torch.Tensor]:
    """tests/material_f64.edited_render with a layer per sample: ``E_all`` [(K+1),C,B], ``d_all`` [(K+1),C], ``s_all`` [K+1],
    ``layer`` [N] (0 = the top-level edit)."""
    dt = p.hash_table.dtype
    o, d, t0, t1 = (x.detach().cpu().to(dt) for x in (origins, directions, starts, ends))
    t0, t1 = t0.view(-1, 1), t1.view(-1, 1)
    ri, layer = ray_indices.detach().cpu().long(), layer.detach().cpu().long()
    E_all, d_all, s_all = (x.detach().cpu().float().to(dt) for x in (E_all, d_all, s_all))
    with torch.no_grad():
        density, emb, _, _ = T.field_density(p, o, d, t0, t1, contraction)
        fo = T.field_outputs(p, o, d, t0, t1, emb, temperature)
        N, C = o.shape[0], p.C
        key = "spectral2" if p.pred_specular else "spectral"
        mixing = torch.zeros_like(fo[key])
        for k in range(E_all.shape[0]):
            pe = copy.deepcopy(p)
            pe.endmembers.copy_(E_all[k])
            fe = T.field_outputs(pe, o, d, t0, t1, emb, temperature)
            mixing[layer == k] = fe[key][layer == k]
        a = fo["abundances"].reshape(N, C)
        factor = (1.0 + ((d_all[layer] - 1.0) * a).sum(1)).clamp(min=0.0)
        density = density * factor[:, None]
        pinfo = T.pack_info(ri, num_rays)
        weights = T.render_weight_from_density(t0[..., 0], t1[..., 0], density[..., 0], pinfo)[0][..., None]
        out = {"depth": T.render_depth_expected(weights, t0, t1, ri, num_rays),
               "accumulation": T.accumulate_along_rays(weights[..., 0], None, ri, num_rays), "weights": weights}
        if p.pred_specular:
            out["spectral2"] = T.spectral_renderer(mixing, weights, ri, num_rays)
            out["specular"] = T.spectral_renderer(s_all[layer].reshape(-1, 1) * fo["specular"].reshape(N, -1), weights, ri, num_rays)
            out["spectral"] = out["spectral2"] + out["specular"]
        else:
            out["spectral"] = T.spectral_renderer(mixing, weights, ri, num_rays)
        unedited = T.spectral_renderer(fo["spectral"], weights, ri, num_rays)
        out["rgb"] = T.colour_system(out["spectral"], colour_M.detach().cpu().to(dt))
        out["abundances"] = T.spectral_renderer(fo["abundances"], weights, ri, num_rays)
        _, probs = T.cluster_lookup(unedited, 0.2, p.endmembers)
        out["seg_probs"] = probs
        out["seg_raw"] = probs.argmax(1) * (out["accumulation"] > 0.5).to(dt).squeeze(-1)
        out["unedited_spectral"] = unedited
    return out
