"""Spectral-clustering cases, their float32 replay / float64 runs and the comparators (plain helper module, no tests in it).  It mirrors
tests/library_f64.py for csrc/umhs_cluster.hip and umhsnerf/cluster.py.

Used by tests/test_hip_cluster.py (the kernel and the fit on the GPU) and tests/test_cluster_bounds_cpu.py (the comparators pass the
float32 replay and reject planted faults; the constants, the tie cap and the teeth are measured there).

Statement (include/umhs_hip.h, "Spectral clustering"), on float32 rows x [R,B], float32 centres c [K,B] (unit rows for ANGLE) and
float32 half_norm h [K] = |c|^2 / 2 (EUCLIDEAN):
  ANGLE      val[r,k] = (sum_b x_b c_kb) / sqrt(sum_b x_b^2);  label = argmax_k val, ties to the smaller k;  score = val[label];
             member vector v = x / |x|;  objective term o = 1 - score.
  EUCLIDEAN  val[r,k] = sum_b x_b c_kb - h_k;  label likewise;  score = max(0, |x|^2 - 2 val[label]);  v = x;  o = score.
  A row that is all zero, holds a NaN / Inf or has mask <= 0.5 gives (-1, 0) and adds nothing.
  acc = (valid rows, sum o, n[K], s[K,B]): float32 sums in row order within chunks of 1024 rows, the chunks added in float64.
The float64 run (the truth) takes the SAME float32 inputs.  The cases are library_f64.make_case(R, B, K), unchanged, its library rows
the centres (its unit rows for ANGLE).

RULES, u = 2^-24, tiny = 2^-126:
  label      lies in the float64 TIED SET: the k whose val64 is within EDGE x (mag + mag_best) of the best, EDGE = 64 u (rays_f64);
             mag[r,k] = sum_b |x_b c_kb| / |x| + 2 |val64|  for ANGLE  (library_f64's),
             mag[r,k] = sum_b |x_b c_kb| + |h_k| + 2 |val64|  for EUCLIDEAN.
  score      |got - score64 at the reported label| <= K_S u (mag + tiny).
  counts     acc's valid rows and n[k] equal the count / bincount of the code's OWN returned labels, exactly.
  sums       |s[k,b] - s64[k,b]| <= K_SUM u sum_members |v[r,b]|, s64 summed in float64 over the code's own labels (v in float64).
  objective  |obj - obj64| <= K_OBJ u sum |o64|, likewise.
Exact properties beside the rules: dead rows give exactly (-1, 0); of the two DUPLICATED centres (dup_a < dup_b, identical bits) dup_b
is never a label.

Each K_* = max(8, 4 x the float32 CPU replay's worst ratio over the cases and both metrics, rounded up to a power of two) -- the
project's standing 4 x margin.  The replay is one rounding per operation in the header's order (products and sums rounded separately;
the kernel's fmaf chains round less often).  Measured on the CPU (tests/test_cluster_bounds_cpu.py re-measures and asserts
4 x worst <= K), pass-boundary case included:
  score      worst 15.51 (euclidean R600-B256-K40, whose mag leaves |x|^2 out; angle 4.79 at the same shape)  -> K_S   = 64
  sums       worst  9.56 (euclidean R600-B256-K40; angle 8.73 at R1100-B31-K6)                                 -> K_SUM = 64
  objective  worst 10.94 (angle R300-B31-K16; euclidean 5.75 at R300-B31-K17)                                  -> K_OBJ = 64

Conditions on the cases, asserted on the float64 run alone with dup_b left out (it ties by construction):
  tie cap  at most 2 % of a case's live rows have more than one k in the tied set.
  teeth    at least 90 % of the live rows have |val_best - val_second| > 16 x (K_S u (mag_best + tiny)).
  (130, 65, 33) is the empty-cluster case: clusters without a row under the float64 labels.

THE FIT.  planted(R, B, K, metric) makes rows gain (centre_k + 0.02 randn), gain in [0.5, 1.5] for ANGLE and 1 for EUCLIDEAN, cut into
three frames of unequal size.  lloyd(...) is Lloyd's algorithm on the host from given initial centres, in float64 (the truth) or as the
float32 replay (the header's step in float32, the update as umhsnerf.cluster does it).  K_CENTRE bounds the centres of a float32 fit
against the float64 fit's, elementwise: |c - c64| <= K_CENTRE u max_b |c64[k,b]|, while both visit the same partitions; measured with
the replay over FIT_CASES x both metrics x seeds 0..2: worst 5.05 (angle (3000, 141, 6)) -> K_CENTRE = 32.  (Seeds at which the float64 fit itself stops in a local
minimum are not used: euclidean seed 0 at (4000, 8, 3) recovers 67 % and at (3000, 141, 6) 84 %.)  objective_margin: the objective of iteration
i + 1 is at most that of iteration i plus both iterations' rounding -- the objective rule's K_OBJ u sum |o| for the sum, and for ANGLE
the terms' own K_S u mag each, mag <= 3 (|x.c| / |x| <= 1 for unit c): a term 1 - score near 0 carries the score's absolute error."""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import library_f64 as LF
from rays_f64 import EDGE, TEETH, TINY, U  # noqa: F401  (one rule, one edge margin)

ANGLE, EUCLIDEAN = 0, 1
METRICS = {"angle": ANGLE, "euclidean": EUCLIDEAN}
CHUNK = 1024
K_S, K_SUM, K_OBJ, K_CENTRE = 64.0, 64.0, 64.0, 32.0
TIE_CAP = 0.02
MIN_TEETH = 0.9
FLT_MAX = 3.4028234663852886e38

CASES = [(0, 5, 3), (1, 1, 1), (257, 2, 2), (300, 4, 33), (257, 8, 15), (300, 31, 16), (300, 31, 17), (130, 65, 33), (1100, 31, 6),
         (2100, 141, 64), (600, 256, 40)]
BOUNDARY_CASE = (513 * 1024 + 3, 2, 2)  # more chunks than one pass holds
EMPTY_CASE = (130, 65, 33)
FIT_CASES = {(4000, 31, 5): {"angle": 0, "euclidean": 1}, (4000, 8, 3): {"angle": 0, "euclidean": 1},
             (3000, 141, 6): {"angle": 0, "euclidean": 1}}  # shape -> the k-means++ seed per metric


def case_id(c) -> str:
    return f"R{c[0]}-B{c[1]}-K{c[2]}"


def k_for(worst: float) -> float:
    return max(8.0, 2.0 ** math.ceil(math.log2(4.0 * worst))) if worst > 0 else 8.0


def half_norm(centres: torch.Tensor) -> torch.Tensor:
    """float32 [K] = |c|^2 / 2, formed in float64 from the float32 centres and rounded once."""
    return (centres.double().pow(2).sum(1) / 2).float()


@functools.lru_cache(maxsize=None)
def problem(R: int, B: int, K: int, metric: str) -> Dict:
    """The case as the step takes it: x, centres (float32), h, the dead rows and the duplicated pair."""
    case = LF.make_case(R, B, K)
    centres = case["unit"] if metric == "angle" else case["library"]
    return dict(R=R, B=B, K=K, metric=metric, x=case["spectra"], centres=centres, h=half_norm(centres) if metric == "euclidean" else None,
                dead=case["degenerate"], dup=case["dup"])


def _argbest(val: torch.Tensor, larger_index: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(best value [R], its index [R], -1 where no entry is above -Inf) by the header's rule whatever torch's own tie order is."""
    R, K = val.shape
    v = torch.where(torch.isnan(val), torch.full_like(val, float("-inf")), val)
    m = v.max(1).values if K else torch.full((R,), float("-inf"), dtype=val.dtype)
    ar = torch.arange(K)[None, :]
    at = torch.where(v == m[:, None], ar, -1).max(1).values if larger_index else torch.where(v == m[:, None], ar, K).min(1).values
    return m, torch.where(m > float("-inf"), at, torch.full_like(at, -1))


def step(x: torch.Tensor, centres: torch.Tensor, h: Optional[torch.Tensor], metric: str, dtype=torch.float32,
         mask: Optional[torch.Tensor] = None, want_acc: bool = True, fault: Optional[str] = None, chunk: int = CHUNK) -> Dict:
    """The header's step in ``dtype``, one rounding per operation, in its order -> {"label" int64 [R], "score" [R], "acc" float64
    [2 + K + K B]}.  ``fault``: a planted fault ("last band", "half norm", "larger index", "chunk", "invalid counted", "division")."""
    R, B = x.shape
    K = centres.shape[0]
    angle = METRICS[metric] == ANGLE
    xs, c = x.to(dtype), centres.to(dtype)
    dot, ss = torch.zeros(R, K, dtype=dtype), torch.zeros(R, dtype=dtype)
    for b in range(B - (1 if fault == "last band" else 0)):
        dot = dot + xs[:, b:b + 1] * c[None, :, b]
        ss = ss + xs[:, b] * xs[:, b]
    rs = torch.sqrt(ss)
    if angle:
        val = dot / rs[:, None]
    else:
        val = dot if fault == "half norm" else dot - h.to(dtype)[None, :]
    best, label = _argbest(val, larger_index=fault == "larger index")
    invalid = ~((ss > 0) & (ss <= FLT_MAX)) | (label < 0)
    if mask is not None:
        invalid = invalid | (mask.reshape(-1) <= 0.5)
    score = best if angle else torch.clamp(ss - 2 * best, min=0)  # (2 g is exact: one rounding, as fmaf(-2, g, ss))
    v = xs if (not angle or fault == "division") else xs / rs[:, None]
    o = 1 - score if angle else score
    zero = torch.zeros((), dtype=dtype)
    would = label.clamp(min=0)
    label = torch.where(invalid, torch.full_like(label, -1), label)
    score = torch.where(invalid, zero, score)
    out = {"label": label, "score": score, "acc": None}
    if not want_acc:
        return out
    v = torch.where(invalid[:, None], zero, v)
    o = torch.where(invalid, zero, o)
    chunks = (R + chunk - 1) // chunk
    pad = chunks * chunk - R
    lab = torch.cat([label, torch.full((pad,), -1, dtype=label.dtype)]).view(chunks, chunk)
    vp = torch.cat([v, torch.zeros(pad, B, dtype=dtype)]).view(chunks, chunk, B)
    op = torch.cat([o, torch.zeros(pad, dtype=dtype)]).view(chunks, chunk)
    s, obj = torch.zeros(chunks, K, B, dtype=dtype), torch.zeros(chunks, dtype=dtype)
    ar = torch.arange(K)[None, :]
    for i in range(min(chunk, R)):
        onehot = (lab[:, i:i + 1] == ar).to(dtype)
        s = s + onehot[:, :, None] * vp[:, i, None, :]  # (a product by an exact 0 or 1 is exact)
        obj = obj + op[:, i]
    n = torch.stack([(lab == k).sum(1) for k in range(K)], 1).double() if K else torch.zeros(chunks, 0, dtype=torch.float64)
    valid = (lab >= 0).sum(1).double()
    if fault == "invalid counted":
        bad = torch.cat([invalid, torch.zeros(pad, dtype=torch.bool)]).view(chunks, chunk)
        wp = torch.cat([would, torch.zeros(pad, dtype=would.dtype)]).view(chunks, chunk)
        valid = valid + bad.sum(1)
        n = n + torch.stack([(bad & (wp == k)).sum(1) for k in range(K)], 1)
    acc = torch.zeros(2 + K + K * B, dtype=torch.float64)
    for j in range(chunks):  # onto acc in float64, chunks ascending
        if fault == "chunk" and j == chunks // 2:
            continue
        acc += torch.cat([valid[j:j + 1], obj[j:j + 1].double(), n[j], s[j].double().reshape(-1)])
    out["acc"] = acc
    return out


def ref64(x: torch.Tensor, centres: torch.Tensor, h: Optional[torch.Tensor], metric: str, dead: torch.Tensor) -> Dict:
    """float64 on the float32 inputs: val [R,K], mag + tiny [R,K], ss [R], v [R,B] (rows of ``dead`` hold nothing that is looked at)."""
    xs, c = x.double(), centres.double()
    xs = torch.where(dead[:, None], torch.ones_like(xs), xs)
    ss = xs.pow(2).sum(1)
    if METRICS[metric] == ANGLE:
        ns = ss.sqrt()[:, None]
        val = (xs @ c.T) / ns
        return dict(val=val, mag=(xs.abs() @ c.abs().T) / ns + 2 * val.abs() + TINY, ss=ss, v=xs / ns)
    val = xs @ c.T - h.double()[None, :]
    return dict(val=val, mag=xs.abs() @ c.abs().T + h.double().abs()[None, :] + 2 * val.abs() + TINY, ss=ss, v=xs)


@functools.lru_cache(maxsize=None)
def reference(R: int, B: int, K: int, metric: str) -> Tuple[Dict, Dict]:
    """(problem, float64 run), computed once per shape and metric and shared; neither is to be changed."""
    p = problem(R, B, K, metric)
    return p, ref64(p["x"], p["centres"], p["h"], metric, p["dead"])


def tied_set(val: torch.Tensor, mag: torch.Tensor) -> torch.Tensor:
    """bool [R,K]: within EDGE x (mag + mag_best) of the best (the best included)."""
    best = val.argmax(1, keepdim=True)
    tied = (val.gather(1, best) - val) < EDGE * (mag + mag.gather(1, best))
    tied.scatter_(1, best, True)
    return tied


def _ratio(d: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    r = torch.where(d == 0, torch.zeros_like(d), d / (U * scale))
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)


def check_step(p: Dict, out: Dict, r64: Dict, dead: Optional[torch.Tensor] = None, report: Optional[Dict] = None,
               ks: Sequence[float] = (K_S, K_SUM, K_OBJ), prefix: str = "") -> List[str]:
    """Every rule of the module docstring on ``out`` = {"label", "score", "acc" or None}; ``dead`` overrides the problem's dead rows
    (a mask adds to them); report[prefix + "score" / "sums" / "objective"] = the worst ratio."""
    R, B, K = p["x"].shape[0], p["x"].shape[1], p["centres"].shape[0]
    angle = METRICS[p["metric"]] == ANGLE
    dead = p["dead"] if dead is None else dead
    live = ~dead
    fails: List[str] = []
    label = out["label"].detach().cpu().long() if out.get("label") is not None else None
    score = out["score"].detach().cpu().double() if out.get("score") is not None else None
    if label is not None and tuple(label.shape) != (R,) or score is not None and tuple(score.shape) != (R,):
        return [f"{prefix}shapes, want ({R},)"]
    if label is not None and bool((label[dead] != -1).any()) or score is not None and bool((score[dead] != 0).any()):
        fails.append(f"{prefix}a dead row (all zero, NaN / Inf, masked) did not give label -1 and score 0")
    if label is None:
        return fails
    lab = label[live]
    n_live = int(lab.shape[0])
    if bool(((lab < 0) | (lab >= K)).any()):
        return fails + [f"{prefix}label outside 0..{K - 1} on {int(((lab < 0) | (lab >= K)).sum())} live rows"]
    val, mag = r64["val"][live], r64["mag"][live]
    if n_live:
        outside = ~tied_set(val, mag).gather(1, lab[:, None])[:, 0]
        if bool(outside.any()):
            i = int(outside.nonzero()[0])
            fails.append(f"{prefix}label: {int(outside.sum())} of {n_live} live rows outside the float64 tied set (first: live row {i}, "
                         f"cluster {int(lab[i])})")
        if p.get("dup") is not None and bool((lab == p["dup"][1]).any()):
            fails.append(f"{prefix}centre {p['dup'][1]} duplicates centre {p['dup'][0]}: the earlier one must win")
    at = val.gather(1, lab[:, None])[:, 0]
    s64 = at if angle else torch.clamp(r64["ss"][live] - 2 * at, min=0)
    if score is not None and n_live:
        ratio = _ratio((score[live] - s64).abs(), mag.gather(1, lab[:, None])[:, 0])
        worst = float(ratio.max())
        if report is not None:
            report[prefix + "score"] = worst
        if worst > ks[0]:
            i = int(ratio.argmax())
            fails.append(f"{prefix}score: live row {i}: {float(score[live][i]):.9g} vs float64 {float(s64[i]):.9g} = {worst:.3g} u mag "
                         f"(K_S = {ks[0]:g}; {int((ratio > ks[0]).sum())} of {n_live} over)")
    if out.get("acc") is None:
        return fails
    acc = out["acc"].detach().cpu().double()
    if tuple(acc.shape) != (2 + K + K * B,):
        return fails + [f"{prefix}acc has shape {tuple(acc.shape)}, want ({2 + K + K * B},)"]
    counts = torch.bincount(lab, minlength=K).double()
    if float(acc[0]) != float((label >= 0).sum()) or not torch.equal(acc[2:2 + K], counts):
        fails.append(f"{prefix}counts: valid {float(acc[0]):g} and n {acc[2:2 + K].tolist()} are not the count / bincount of the returned "
                     f"labels ({int((label >= 0).sum())}, {counts.tolist()})")
    v = r64["v"][live]
    sums64 = torch.zeros(K, B, dtype=torch.float64).index_add_(0, lab, v)
    scale = torch.zeros(K, B, dtype=torch.float64).index_add_(0, lab, v.abs())
    ratio = _ratio((acc[2 + K:].view(K, B) - sums64).abs(), scale)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if report is not None:
        report[prefix + "sums"] = worst
    if worst > ks[1]:
        k, b = divmod(int(ratio.argmax()), B)
        fails.append(f"{prefix}sums: s[{k},{b}] = {float(acc[2 + K + k * B + b]):.9g} vs float64 {float(sums64[k, b]):.9g} = {worst:.3g} u "
                     f"sum |v| (K_SUM = {ks[1]:g})")
    o64 = 1 - s64 if angle else s64
    worst = float(_ratio((acc[1] - o64.sum()).abs().reshape(1), o64.abs().sum().reshape(1) + TINY)[0])
    if report is not None:
        report[prefix + "objective"] = worst
    if worst > ks[2]:
        fails.append(f"{prefix}objective: {float(acc[1]):.12g} vs float64 {float(o64.sum()):.12g} = {worst:.3g} u sum |o| (K_OBJ = {ks[2]:g})")
    return fails


def conditions(p: Dict, r64: Dict) -> Dict:
    """{"tied": share of live rows with more than one k in the tied set, "teeth": share with |best - second| > 16 x the score bound,
    "live": n, "empty": clusters without a row under the float64 labels}, with dup_b left out; None where there is nothing to measure."""
    live = ~p["dead"]
    val, mag = r64["val"][live], r64["mag"][live]
    K = val.shape[1]
    empty = int((torch.bincount(_argbest(val)[1].clamp(min=0), minlength=K) == 0).sum()) if val.shape[0] else None
    if p["dup"] is not None:
        keep = torch.ones(K, dtype=torch.bool)
        keep[p["dup"][1]] = False
        val, mag = val[:, keep], mag[:, keep]
    n = val.shape[0]
    if n == 0 or val.shape[1] < 2:
        return {"tied": 0.0 if n else None, "teeth": None, "live": n, "empty": empty}
    tied = tied_set(val, mag).sum(1) > 1
    best = val.argmax(1)
    top = val.topk(2, dim=1).values
    bound = K_S * U * mag.gather(1, best[:, None])[:, 0]
    return {"tied": float(tied.sum()) / n, "teeth": float(((top[:, 0] - top[:, 1]) > TEETH * bound).sum()) / n, "live": n, "empty": empty}


# ---- the fit -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(R: int, B: int, K: int, metric: str, seed: int = 3) -> Dict:
    """Rows gain (centre_k + 0.02 randn) around K planted centres, as three frames of unequal size -> {"frames": [float32 [r_i,B]],
    "truth" int64 [R], "centres" float32 [K,B]}."""
    g = torch.Generator().manual_seed(7000 * seed + 11 * R + 5 * B + K + (0 if metric == "angle" else 1))
    centres = LF.make_library(K, B, g)
    truth = torch.randint(0, K, (R,), generator=g)
    gain = 0.5 + torch.rand(R, 1, generator=g) if metric == "angle" else torch.ones(R, 1)
    x = (gain * (centres[truth] + 0.02 * torch.randn(R, B, generator=g))).float()
    cuts = [0, R // 5, R // 5 + R // 2, R]
    return dict(frames=[x[a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])], truth=truth, centres=centres, x=x)


def update_centres(centres: torch.Tensor, acc: torch.Tensor, K: int, B: int, metric: str) -> Tuple[torch.Tensor, int]:
    """The host update of umhsnerf.cluster in float64: s / |s| (ANGLE) or s / n (EUCLIDEAN); an empty cluster keeps its centre."""
    n, s = acc[2:2 + K], acc[2 + K:].view(K, B)
    new = s / s.norm(dim=1, keepdim=True) if METRICS[metric] == ANGLE else s / n[:, None]
    keep = (n == 0) | ~torch.isfinite(new).all(1)
    return torch.where(keep[:, None], centres.double(), new), int((n == 0).sum())


def lloyd(frames: Sequence[torch.Tensor], init: torch.Tensor, metric: str, dtype, iterations: int = 50, tolerance: float = 1e-4) -> Dict:
    """Lloyd's algorithm from ``init`` [K,B].  float64: the truth (centres stay float64).  float32: the replay -- the header's step in
    float32 on centres rounded once per iteration, acc over the frames in order, the update in float64.  -> {"centres" float64 [K,B],
    "labels" int64 [R] (of the last assignment), "objective": [per iteration], "partitions": [labels per iteration]}."""
    K, B = init.shape
    angle = METRICS[metric] == ANGLE
    centres = init.double()
    objective, partitions = [], []
    for _ in range(iterations):
        used = centres / centres.norm(dim=1, keepdim=True) if angle else centres  # (as SpectralClusters.device_centres)
        used = used.float() if dtype == torch.float32 else used
        h = (used.double().pow(2).sum(1) / 2).to(used.dtype) if not angle else None
        acc, labels = torch.zeros(2 + K + K * B, dtype=torch.float64), []
        for f in frames:
            if dtype == torch.float32:
                out = step(f, used, h, metric, torch.float32)
                acc += out["acc"]
                labels.append(out["label"])
            else:
                r = ref64(f, used, h, metric, torch.zeros(f.shape[0], dtype=torch.bool))
                best, lab = _argbest(r["val"])
                o = 1 - best if angle else torch.clamp(r["ss"] - 2 * best, min=0)
                acc[0] += f.shape[0]
                acc[1] += o.sum()
                acc[2:2 + K] += torch.bincount(lab, minlength=K)
                acc[2 + K:] += torch.zeros(K, B, dtype=torch.float64).index_add_(0, lab, r["v"]).reshape(-1)
                labels.append(lab)
        objective.append(float(acc[1]))
        partitions.append(torch.cat(labels))
        new, _ = update_centres(used, acc, K, B, metric)
        same = torch.equal(new.to(used.dtype), used)
        centres = new
        if same or (len(objective) > 1 and objective[-2] - objective[-1] <= tolerance * objective[-2]):
            break
    return dict(centres=centres, labels=partitions[-1], objective=objective, partitions=partitions)


def objective_margin(metric: str, rows: int) -> Tuple[float, float]:
    """(relative, absolute): objective[i + 1] <= objective[i] (1 + relative) + absolute."""
    return 2 * K_OBJ * U, (2 * K_S * U * 3.0 * rows if METRICS[metric] == ANGLE else 0.0)


def partition_agreement(labels: torch.Tensor, truth: torch.Tensor, K: int) -> float:
    """Share of rows on which ``labels`` equals ``truth`` after each found cluster is given the planted cluster most of its rows have."""
    table = torch.zeros(K, K, dtype=torch.int64).index_put_((labels.clamp(min=0), truth), torch.ones_like(truth), accumulate=True)
    return float(table.max(1).values.sum()) / max(int(truth.numel()), 1)


def centre_ratio(centres: torch.Tensor, centres64: torch.Tensor) -> float:
    """max over (k, b) of |c - c64| / (u max_b |c64[k,b]|)."""
    return float(_ratio((centres.double() - centres64).abs(), centres64.abs().max(1, keepdim=True).values.expand_as(centres64)).max())
