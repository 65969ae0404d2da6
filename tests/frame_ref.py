"""numpy float32 restatement of ``umhs_frame_compose`` (include/umhs_hip.h states the arithmetic; this file restates it, one array
operation per rounded step, so that numpy rounds exactly where the kernel must), and the generator of the cases the GPU tests run.
Not a test file.

A panel is a dict: ``kind`` (0 RGB, 1 SCALAR, 2 DEPTH), ``rows`` float32 [n, stride] (the tensor the kernel reads in place), ``channel``,
``range`` float32 [2] or None, ``acc`` float32 [n] or None, ``normalize``, ``invert``, ``cmin``, ``cmax``."""
import numpy as np

RGB, SCALAR, DEPTH = 0, 1, 2
F = np.float32


def q(c):
    """(c * 255) + 0.5, clamped to [0, 255], truncated; NaN -> 0."""
    with np.errstate(all="ignore"):
        t = np.asarray(c, dtype=F) * F(255.0)
        t = t + F(0.5)
        t = np.where(t > 0, t, F(0.0))  # (NaN lands here)
        t = np.where(t > 255, F(255.0), t)
        return t.astype(np.int32).astype(np.uint8)


def clamp01(v):
    """Clamp to [0, 1]; a NaN stays a NaN."""
    with np.errstate(all="ignore"):
        return np.where(v < 0, F(0.0), np.where(v > 1, F(1.0), v)).astype(F)


def panel_bytes(p, lut):
    """uint8 [n, 3] of one panel."""
    lut = np.asarray(lut, dtype=F)
    ch = p["channel"]
    if p["kind"] == RGB:
        return q(p["rows"][:, ch:ch + 3])
    with np.errstate(all="ignore"):
        v = p["rows"][:, ch].astype(F)
        if p["kind"] == DEPTH or p["normalize"]:
            lo, hi = F(p["range"][0]), F(p["range"][1])
            num = v - lo
            den = F(hi - lo) + (F(1e-10) if p["kind"] == DEPTH else F(1e-9))
            v = (num / den).astype(F)
            if p["kind"] == DEPTH:
                v = clamp01(v)
        cmin, cmax = F(p["cmin"]), F(p["cmax"])
        if not (cmin == 0 and cmax == 1):
            v = v * F(cmax - cmin)
            v = v + cmin
        v = clamp01(v)
        if p["invert"]:
            v = F(1.0) - v
        v = np.where(np.isnan(v), F(0.0), v).astype(F)
        i = (v * F(255.0)).astype(np.int32)
        c = lut[i]
        if p["kind"] == DEPTH and p["acc"] is not None:
            a = p["acc"].astype(F)[:, None]
            c = c * a
            c = c + (F(1.0) - a)
        return q(c)


def compose(panels, lut, height, width):
    """uint8 [height, K * width, 3]: the panels side by side."""
    return np.concatenate([panel_bytes(p, lut).reshape(height, width, 3) for p in panels], axis=1)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _neighbours(x):
    x = np.asarray(x, dtype=F)
    return np.concatenate([np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))])


def special_values():
    """Every k / 255 and its two float neighbours (the colour-table index and q() turn over there), the .5 ties of q -- (k + 0.5) / 255
    and neighbours --, values below 0 and above 1, NaN and +-inf."""
    k = np.arange(256, dtype=F)
    return np.concatenate([_neighbours(k / F(255.0)), _neighbours((k + F(0.5)) / F(255.0)),
                           np.array([-1.0, -1e-3, -0.0, 1.0 + 1e-3, 2.0, 300.0, -300.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, 3e38], dtype=F)])


def values(n, rng, lo=0.0, hi=1.0):
    """n float32 values: the special values mapped onto [lo, hi] (all of them when n allows, a random draw of them otherwise) among
    uniform draws of [lo - 0.2 (hi - lo), hi + 0.2 (hi - lo)], in random order."""
    sp = special_values()
    sp = rng.permutation(sp)[:max(1, min(len(sp), n if n >= len(sp) else (n + 1) // 2))]
    x = (rng.random(n) * 1.4 - 0.2).astype(F)
    x[:len(sp)] = sp
    x = rng.permutation(x)
    with np.errstate(all="ignore"):  # (3e38 and the infinities stay what they are)
        return x if (lo, hi) == (0.0, 1.0) else (F(lo) + x * F(hi - lo)).astype(F)


def _finite_range(x):
    f = x[np.isfinite(x)]
    return np.array([f.min(), f.max()] if f.size else [0.0, 1.0], dtype=F)


def _accumulation(n, rng):
    a = rng.random(n).astype(F)
    a[rng.random(n) < 0.2] = 0.0
    a[rng.random(n) < 0.2] = 1.0
    if n >= 2:
        a[0], a[1] = 0.0, 1.0
    return a


def make_panel(variant, n, rng):
    """One of eight panels that between them take every path of the kernel, on sources that are real column views."""
    variant %= 8
    kind, stride, ch = [(RGB, 3, 0), (SCALAR, 31, 7), (DEPTH, 1, 0), (SCALAR, 5, 4), (RGB, 5, 1), (DEPTH, 31, 7), (SCALAR, 1, 0),
                        (SCALAR, 5, 4)][variant]
    rows = rng.random((n, stride)).astype(F)
    p = dict(kind=kind, rows=rows, channel=ch, range=None, acc=None, normalize=False, invert=False, cmin=0.0, cmax=1.0)
    if kind == RGB:
        rows[:, ch:ch + 3] = values(3 * n, rng).reshape(n, 3)
    elif variant == 1:  # plain colormap
        rows[:, ch] = values(n, rng)
    elif variant == 2:  # depth over the frame's own range, blended with accumulation (exact 0 and 1 among it)
        rows[:, ch] = values(n, rng, 2.0, 6.0)
        p.update(range=_finite_range(rows[:, ch]), acc=_accumulation(n, rng))
    elif variant == 3:  # normalized, inverted, squeezed into [0.1, 0.8]
        rows[:, ch] = values(n, rng, -3.0, 5.0)
        p.update(range=_finite_range(rows[:, ch]), normalize=True, invert=True, cmin=0.1, cmax=0.8)
    elif variant == 5:  # depth with lo == hi given as planes, no accumulation, inverted, colormap_min only
        rows[:, ch] = values(n, rng, 1.0, 3.0)
        p.update(range=np.array([2.0, 2.0], dtype=F), invert=True, cmin=0.2, cmax=1.0)
    elif variant == 6:  # normalize with lo == hi
        rows[:, ch] = values(n, rng)
        p.update(range=np.array([0.5, 0.5], dtype=F), normalize=True)
    else:  # inverted only: NaN and +-inf with invert
        rows[:, ch] = values(n, rng)
        p.update(invert=True)
    return p


def make_case(height, width, n_panels, seed=0, first_variant=0):
    rng = np.random.default_rng([seed, height, width, n_panels])
    return [make_panel(first_variant + k, height * width, rng) for k in range(n_panels)]
