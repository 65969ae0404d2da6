"""The rgb-method MLP kernels' cases, their float32 / float64 oracle runs, the envelopes and the comparators (plain helper module, no
tests in it).

Used by tests/test_hip_rgb_f64.py (csrc/umhs_rgb.hip on the GPU: mlp_base 32 -> 64 -> 16 with trunc_exp and the selector, mlp_head
[SH16 | emb15] -> 64 -> 64 -> 3 with a sigmoid, each with a forward, a recomputing backward, per-wave slabs of parameter gradients and
rgb_mlp_reduce_kernel) and tests/test_rgb_f64_bounds_cpu.py (the comparators pass the float32 oracle and reject planted faults; K is
measured there).  It is tests/rays_f64.py's scheme on the one kernel file that had no float64 oracle.

The oracle is oracle/torch_ref.py as it is (mlp_forward, trunc_exp, sh_encoding_deg4, torch.sigmoid, autograd), run twice on the same
float32 inputs: in float32 (the reference's arithmetic) and in float64 (the truth).

ONE RULE for every output element:   |got - ref64| <= K u (mag + tiny),   u = 2^-24,  tiny = 2^-126.
``mag`` is the SINGLE-LEVEL envelope: the float64 sum of the absolute values of the terms that make up the element, times the growth of
the argument of its exp / sigmoid.  (Pushing every layer's own error on through |W| of the layers behind it is 50-300 x looser and has no
teeth; it is not used.)  With x the layer-0 input, a_l = W_l h_{l-1} + b_l, h_l = relu(a_l), m_l = sum |W_l h_{l-1}| + |b_l| (the
dot product's own magnitude), r_l = [a_l > 0] in float64:
 base forward   z = a_1[0]:   sigma_raw  m_1[0];   emb[f]  m_1[f + 1];   density  exp(z) (m_1[0] + 1) sel
 head forward   y = sigmoid(a_2):   rgb   mag_y = y (1 - y) m_2 + y
 cotangents     base  |dz_1[0]| = |g sel| exp(clamp(z, -15, 15)) (1 + [|z| <= 15] m_1[0])   (trunc_exp's clamped derivative: beyond the
                      clamp the factor is the constant e^+-15 and z's own error does not reach it),  |dz_1[f + 1]| = |d_emb[f]|
                head  |dz_2| = |g| (|1 - 2 y| mag_y + y (1 - y))   (the sigmoid's derivative y (1 - y) formed from a y that carries its
                      forward envelope: 1 - y has the absolute error of y, which is what a float32 evaluation does at y -> 1)
                down  |dz_{l-1}| = (|dz_l| |W_l|) r_{l-1}
 gradients      d_W_l[o, i] = sum_n |dz_l[n, o]| X_l[n, i],   d_b_l[o] = sum_n |dz_l[n, o]|,   d_enc / d_emb = |dz_0| |W_0|  (the
                head's d_emb: its columns 16..30).  X_l = m_{l-1} r_{l-1}, the activation's own dot-product magnitude: a unit that
                is barely on is u of its terms away from float64, not u of itself (with |h| in its place d_w1 of a 15-sample case
                is 1200 u off in float32).  Layer 0 of the base: X = |enc|; of the head: X = [sh_mag | |emb|], sh_mag the sum of
                the absolute values of the monomials of each harmonic in t = (d + 1) / 2 (0.946 t_z^2 + 0.315 for the coefficient
                0.946 t_z^2 - 0.315: where a harmonic cancels, its float32 value is u of its terms away, not u of itself).
ReLU edges.  A sample with any hidden pre-activation within RELU_MARGIN = 1e-5 (tests/field_f64.py's) of zero relative to its own m_l
has a unit that is on in one float32 evaluation order and off in another.  The case builder makes such samples INERT in the gradient
comparison: zero cotangents, and for base also selector 0 where there is a selector.  Their forward outputs are compared like every
other sample's.  At most 2 % of a case may be inert (asserted on the float64 run alone; measured: about 0.4 % at the large sizes).

K per output family = max(8, 4 x the float32 CPU oracle's worst ratio over the committed cases, rounded up to a power of two), the
convention of tests/rays_f64.py: the floor of 8 allows for device expf and for association, the factor 4 is the margin over a float32
evaluation in another order.  Measured on the CPU (worst |diff| / (u (mag + tiny)) over every regime x size;
tests/test_rgb_f64_bounds_cpu.py re-measures and asserts that K is what the rule gives):
  base   density 4.72 | emb 6.84 | sigma_raw 6.07 | d_enc 4.55 | d_w0 6.01 | d_b0 2.07 | d_w1 1.46 | d_b1 1.10
  head   rgb 6.26 | d_emb 0.88 | d_w0 0.69 | d_b0 0.29 | d_w1 1.37 | d_b1 1.32 | d_w2 0.53 | d_b2 1.12
so K = 32 for the forward outputs of both MLPs (64-term dot products of both signs in one fixed order) and for base d_enc and d_w0
(worst in the spread regime, where a few cotangents near e^15 dominate a sum), 16 for base d_b0, and 8 for base d_w1, d_b1 and every
gradient of the head.  K is never tuned against the kernels.  tests/test_hip_rgb_f64.py writes the kernels' own worst ratios per
family, case and output to rgb_f64.json in rays_f64.report_dir(); measured on an MI355X, in the order of the table above:
  base   4.28 | 5.28 | 5.28 | 5.46 | 5.81 | 3.05 | 1.70 | 0.91          head   7.18 | 0.83 | 0.83 | 0.32 | 1.06 | 1.00 | 0.99 | 0.72

Teeth: the share of elements with |ref64| > 16 x bound -- there a missing or misplaced term must show.  Condition: in every case with
N >= 1013 at least 90 % of the elements of every gradient tensor has teeth (asserted on the float64 run alone).

Sizes N (every regime runs at every N, every regime x size has its own seed), with grid_for() = min(256, ceil(tiles / 4)) workgroups of
4 waves and 16 samples per wave and trip:
  1                one live lane; three waves of the workgroup write all-zero slabs
  15, 16, 17       the tile boundary
  63, 64, 65       the workgroup boundary; at 65 a second workgroup holds one live lane and three idle waves
  1013             the shape of tests/test_hip_rgb_method.py's kernel-only test
  16384            the grid cap reached exactly, one tile per wave
  16385            one wave's second trip holds a single sample
  22789            some waves take two tiles and others one, with a ragged last tile
  40000            2500 tiles over 1024 waves: two or three trips per wave
Regimes (teeth: whether the 90 % condition is held):
  base plain       teeth   selector with about 10 % zeros, the present test's weight scales
  base spread      teeth   w1[0] *= 14, b1[0] = 2: sigma_raw spreads to |z| of about 45-70, both clamps of trunc_exp's backward are hit
                           (asserted from N = 1013 on: more than 2 % of the samples beyond +-15, some on each side; |z| < 80 always, so exp
                           stays finite)
  base zero_sel    no      all-zero selector: density and every gradient that flows through it are exactly 0 (mag = 0, so the rule
                           asks for |got| <= K u 2^-126: zero); row 0 of d_w1 and d_b1[0] cannot have teeth
  base no_sel      teeth   selector == NULL
  head unit        teeth   random unit directions
  head planted     teeth   rows 0.. hold the six axis directions, (0, 0, 0) and a non-normalised direction (neither the kernel nor the
                           oracle normalises)
  head saturated   no      w2 x 12: outputs saturate the sigmoid on both sides (y = 1 and y < 1e-7 in float32); the gradients are
                           y (1 - y) small and sums of few live terms"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch

import rays_f64 as RF
from field_f64 import RELU_MARGIN
from oracle import torch_ref as T

U, TINY = RF.U, RF.TINY
SIZES = (1, 15, 16, 17, 63, 64, 65, 1013, 16384, 16385, 22789, 40000)
BASE_REGIMES = ("plain", "spread", "zero_sel", "no_sel")
HEAD_REGIMES = ("unit", "planted", "saturated")
NO_TEETH = {("base", "zero_sel"), ("head", "saturated")}
TEETH_FROM_N = 1013
MAX_INERT = 0.02
SATURATION = 12.0  # the saturated regime's scale of w2
CASES = [("base", r, n) for r in BASE_REGIMES for n in SIZES] + [("head", r, n) for r in HEAD_REGIMES for n in SIZES]

BASE_GRADS = ("d_enc", "d_w0", "d_b0", "d_w1", "d_b1")
HEAD_GRADS = ("d_emb", "d_w0", "d_b0", "d_w1", "d_b1", "d_w2", "d_b2")
FAMILIES = tuple("base." + k for k in ("density", "emb", "sigma_raw") + BASE_GRADS) + tuple("head." + k for k in ("rgb",) + HEAD_GRADS)
# measured worst ratio of the float32 CPU oracle per family, and K by the rule (the docstring's table)
MEASURED = {"base.density": 4.72, "base.emb": 6.84, "base.sigma_raw": 6.07, "base.d_enc": 4.55, "base.d_w0": 6.01, "base.d_b0": 2.07,
            "base.d_w1": 1.46, "base.d_b1": 1.10, "head.rgb": 6.26, "head.d_emb": 0.88, "head.d_w0": 0.69, "head.d_b0": 0.29,
            "head.d_w1": 1.37, "head.d_b1": 1.32, "head.d_w2": 0.53, "head.d_b2": 1.12}
K = {"base.density": 32.0, "base.emb": 32.0, "base.sigma_raw": 32.0, "base.d_enc": 32.0, "base.d_w0": 32.0, "base.d_b0": 16.0,
     "base.d_w1": 8.0, "base.d_b1": 8.0, "head.rgb": 32.0, "head.d_emb": 8.0, "head.d_w0": 8.0, "head.d_b0": 8.0, "head.d_w1": 8.0,
     "head.d_b1": 8.0, "head.d_w2": 8.0, "head.d_b2": 8.0}

PLANTED_DIRS = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0], [0, 0, 0], [3.0, -2.0, 0.5]])


def rule_k(worst: float) -> float:
    """max(8, 4 x worst rounded up to a power of two)."""
    k = 8.0
    while k < 4.0 * worst:
        k *= 2.0
    return k


def case_id(c) -> str:
    return f"{c[0]}-{c[1]}-{c[2]}"


def report_dir(root: str) -> str:
    return RF.report_dir(root)


@dataclass
class Case:
    mlp: str  # "base" | "head"
    regime: str
    n: int
    inputs: Dict[str, Optional[torch.Tensor]]  # base: enc, sel (None: NULL); head: dirs, emb
    weights: List[torch.Tensor]  # w0, b0, w1, b1 (, w2, b2)
    cots: Dict[str, torch.Tensor]  # base: d_density, d_emb; head: d_rgb
    inert: torch.Tensor  # [n] bool

    @property
    def grads(self):
        return BASE_GRADS if self.mlp == "base" else HEAD_GRADS

    @property
    def teeth(self) -> bool:
        return self.n >= TEETH_FROM_N and (self.mlp, self.regime) not in NO_TEETH


def _seed(mlp: str, regime: str, n: int) -> int:
    regs = BASE_REGIMES if mlp == "base" else HEAD_REGIMES
    return 53000 + (0 if mlp == "base" else 500) + 41 * regs.index(regime) + 7919 * SIZES.index(n)


def _margins(x64: torch.Tensor, layers) -> torch.Tensor:
    """float64: per sample, the smallest |a_l| / m_l over the hidden layers (every layer but the last)."""
    worst = torch.full((x64.shape[0],), float("inf"), dtype=torch.float64)
    h = x64
    for w, b in layers[:-1]:
        a = h @ w.T + b
        m = h.abs() @ w.abs().T + b.abs()
        worst = torch.minimum(worst, (a.abs() / m).min(1).values)
        h = torch.relu(a)
    return worst


def head_input(dirs: torch.Tensor, emb: torch.Tensor, sh: Callable = T.sh_encoding_deg4) -> torch.Tensor:
    return torch.cat([sh((dirs + 1.0) / 2.0), emb], dim=-1)


def make_case(mlp: str, regime: str, n: int) -> Case:
    """The first draw, counted from the case's own seed, that is what its regime says (decided on float64 quantities alone): at most
    2 % inert samples and a live last sample; base: |z| < 70, and in the spread regime from N = 1013 on at least 1 % of the samples
    beyond each clamp; saturated head: the sigmoid's argument above -75, and from N = 1013 on at least 1 % of the outputs saturated on
    each side.  (The spread row's sign balance and range depend on sixty-four weights; one draw in three is one-sided.)"""
    for attempt in range(37):
        case, ok = _draw(mlp, regime, n, _seed(mlp, regime, n) + attempt)
        if ok:
            return case
    raise RuntimeError(f"no draw of {mlp}-{regime}-{n} meets its regime")


def _draw(mlp: str, regime: str, n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    big = n >= TEETH_FROM_N
    if mlp == "base":
        enc = torch.rand(n, 32, generator=g) - 0.5
        sel = (torch.rand(n, generator=g) > 0.1).float()
        w0, b0 = torch.randn(64, 32, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1
        w1, b1 = torch.randn(16, 64, generator=g) * 0.3, torch.randn(16, generator=g) * 0.1
        d_density, d_emb = torch.randn(n, generator=g), torch.randn(n, 15, generator=g)
        if regime == "spread":
            b1[0] = 2.0
            w1[0] *= 14.0
        sel[-1] = 1.0  # (the last sample is live: the planted faults of a ragged tail need its gradient)
        if regime == "zero_sel":
            sel = torch.zeros(n)
        W = [w0, b0, w1, b1]
        inert = _margins(enc.double(), [(w0.double(), b0.double()), (w1.double(), b1.double())]) <= RELU_MARGIN
        sel[inert] = 0
        d_density[inert] = 0
        d_emb[inert] = 0
        z = T.mlp_forward(enc.double(), [w0.double(), w1.double()], [b0.double(), b1.double()])[:, 0]
        ok = float(inert.double().mean()) <= MAX_INERT and not bool(inert[-1]) and float(z.abs().max()) < 70
        if regime == "spread" and big:
            ok = ok and min(float((z > 15).double().mean()), float((z < -15).double().mean())) >= 0.01
        inputs = {"enc": enc, "sel": None if regime == "no_sel" else sel}
        return Case(mlp, regime, n, inputs, W, {"d_density": d_density, "d_emb": d_emb}, inert), ok
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    emb = torch.randn(n, 15, generator=g) * 0.5
    W = [torch.randn(64, 31, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1, torch.randn(64, 64, generator=g) * 0.2,
         torch.randn(64, generator=g) * 0.1, torch.randn(3, 64, generator=g) * 0.3, torch.randn(3, generator=g) * 0.1]
    d_rgb = torch.randn(n, 3, generator=g)
    if regime == "planted":
        k = min(n, PLANTED_DIRS.shape[0])
        dirs[:k] = PLANTED_DIRS[:k]
    if regime == "saturated":
        W[4] = W[4] * SATURATION
    Wd = [t.double() for t in W]
    x = head_input(dirs.double(), emb.double())
    inert = _margins(x, [(Wd[0], Wd[1]), (Wd[2], Wd[3]), (Wd[4], Wd[5])]) <= RELU_MARGIN
    d_rgb[inert] = 0
    ok = float(inert.double().mean()) <= MAX_INERT and not bool(inert[-1])
    if regime == "saturated":
        o = T.mlp_forward(x, Wd[0::2], Wd[1::2])
        ok = ok and float(o.min()) > -75 and (not big or min(float((o > 17).double().mean()), float((o < -17).double().mean())) >= 0.01)
    return Case(mlp, regime, n, {"dirs": dirs, "emb": emb}, W, {"d_rgb": d_rgb}, inert), ok


# ------------------------------------------------------------------------------------------------------------------------------ #
# oracle
# ------------------------------------------------------------------------------------------------------------------------------ #
def oracle(case: Case, dtype, cot_weight: Optional[torch.Tensor] = None, exp: Callable = T.trunc_exp, sh: Callable = T.sh_encoding_deg4,
           emb_shift: bool = False, drop_bias_tile: Optional[int] = None, sigmoid_at_pre_relu: bool = False) -> Dict[str, torch.Tensor]:
    """Forward outputs and every gradient from oracle/torch_ref.py in ``dtype``.  The keyword arguments plant faults
    (tests/test_rgb_f64_bounds_cpu.py): ``cot_weight`` [n] scales each sample's cotangents, ``exp`` replaces trunc_exp, ``sh`` the SH
    encoding, ``emb_shift`` feeds emb[f - 1] for emb[f], ``drop_bias_tile`` zeroes b0[16 t : 16 t + 16] in the forward,
    ``sigmoid_at_pre_relu`` forms the sigmoid's derivative from the layer-1 pre-activation without its ReLU."""
    cv = lambda t: t.to(dtype)
    cw = torch.ones(case.n, dtype=dtype) if cot_weight is None else cv(cot_weight)
    W = [cv(t).clone().requires_grad_() for t in case.weights]
    b0 = W[1]
    if drop_bias_tile is not None:
        keep = torch.ones(64, dtype=dtype)
        keep[16 * drop_bias_tile: 16 * drop_bias_tile + 16] = 0
        b0 = W[1] * keep
    if case.mlp == "base":
        enc = cv(case.inputs["enc"]).clone().requires_grad_()
        sel = case.inputs["sel"]
        out = T.mlp_forward(enc, [W[0], W[2]], [b0, W[3]])
        density = exp(out[:, 0]) * (cv(sel) if sel is not None else 1.0)
        emb = out[:, 1:]
        g = torch.autograd.grad([density, emb], [enc] + W, [cv(case.cots["d_density"]) * cw, cv(case.cots["d_emb"]) * cw[:, None]])
        r = {"density": density.detach(), "emb": emb.detach(), "sigma_raw": out[:, 0].detach()}
        r.update(zip(BASE_GRADS, g))
        return r
    emb = cv(case.inputs["emb"]).clone().requires_grad_()
    x = head_input(cv(case.inputs["dirs"]), torch.roll(emb, 1, dims=1) if emb_shift else emb, sh)
    h1 = torch.relu(torch.nn.functional.linear(x, W[0], b0))
    rgb = torch.sigmoid(T.mlp_forward(h1, [W[2], W[4]], [W[3], W[5]]))
    d_rgb = cv(case.cots["d_rgb"]) * cw[:, None]
    if sigmoid_at_pre_relu:
        a2 = torch.nn.functional.linear(h1, W[2], W[3])
        yp = torch.sigmoid(torch.nn.functional.linear(a2, W[4], W[5])).detach()
        o = T.mlp_forward(h1, [W[2], W[4]], [W[3], W[5]])
        g = torch.autograd.grad(o, [emb] + W, d_rgb * yp * (1 - yp))
    else:
        g = torch.autograd.grad(rgb, [emb] + W, d_rgb)
    r = {"rgb": rgb.detach()}
    r.update(zip(HEAD_GRADS, g))
    return r


# ------------------------------------------------------------------------------------------------------------------------------ #
# envelopes
# ------------------------------------------------------------------------------------------------------------------------------ #
def sh_mag(t: torch.Tensor) -> torch.Tensor:
    """Sum of the absolute values of the monomials of each degree-4 harmonic at t = (d + 1) / 2 (float64)."""
    x, y, z = t[:, 0].abs(), t[:, 1].abs(), t[:, 2].abs()
    xx, yy, zz = x * x, y * y, z * z
    c = torch.zeros(t.shape[0], 16, dtype=torch.float64)
    c[:, 0] = 0.28209479177387814
    c[:, 1], c[:, 2], c[:, 3] = 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x
    c[:, 4], c[:, 5], c[:, 7] = 1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 1.0925484305920792 * x * z
    c[:, 6] = 0.9461746957575601 * zz + 0.31539156525251999
    c[:, 8] = 0.5462742152960396 * (xx + yy)
    c[:, 9] = 0.5900435899266435 * y * (3 * xx + yy)
    c[:, 10] = 2.890611442640554 * x * y * z
    c[:, 11] = 0.4570457994644658 * y * (5 * zz + 1)
    c[:, 12] = 0.3731763325901154 * z * (5 * zz + 3)
    c[:, 13] = 0.4570457994644658 * x * (5 * zz + 1)
    c[:, 14] = 1.445305721320277 * z * (xx + yy)
    c[:, 15] = 0.5900435899266435 * x * (xx + 3 * yy)
    return c


def envelopes(case: Case) -> Dict[str, torch.Tensor]:
    """``mag + tiny`` of every output (module docstring), float64."""
    f = lambda t: t.double()
    W = [f(t) for t in case.weights]
    if case.mlp == "base":
        x = f(case.inputs["enc"])
        sel = f(case.inputs["sel"]) if case.inputs["sel"] is not None else torch.ones(case.n, dtype=torch.float64)
        a0 = x @ W[0].T + W[1]
        h0, r0 = torch.relu(a0), (a0 > 0).double()
        m0 = (x.abs() @ W[0].abs().T + W[1].abs()) * r0
        a1 = h0 @ W[2].T + W[3]
        m1 = h0 @ W[2].abs().T + W[3].abs()
        z = a1[:, 0]
        env = {"sigma_raw": m1[:, 0], "emb": m1[:, 1:], "density": torch.exp(z) * (m1[:, 0] + 1) * sel}
        inside = ((z.abs() - 15) <= RF.EDGE * m1[:, 0]).double()
        dz1 = torch.cat([((f(case.cots["d_density"]) * sel).abs() * torch.exp(z.clamp(-15, 15)) * (1 + inside * m1[:, 0]))[:, None],
                         f(case.cots["d_emb"]).abs()], 1)
        dz0 = (dz1 @ W[2].abs()) * r0
        env.update(d_w1=dz1.T @ m0, d_b1=dz1.sum(0), d_w0=dz0.T @ x.abs(), d_b0=dz0.sum(0), d_enc=dz0 @ W[0].abs())
    else:
        dirs, emb = f(case.inputs["dirs"]), f(case.inputs["emb"])
        x = head_input(dirs, emb)
        xm = torch.cat([sh_mag((dirs + 1.0) / 2.0), emb.abs()], 1)
        a0 = x @ W[0].T + W[1]
        h0, r0 = torch.relu(a0), (a0 > 0).double()
        m0 = (xm @ W[0].abs().T + W[1].abs()) * r0
        a1 = h0 @ W[2].T + W[3]
        h1, r1 = torch.relu(a1), (a1 > 0).double()
        m1 = (h0 @ W[2].abs().T + W[3].abs()) * r1
        a2 = h1 @ W[4].T + W[5]
        m2 = h1 @ W[4].abs().T + W[5].abs()
        y = torch.sigmoid(a2)
        y1y = y * torch.sigmoid(-a2)  # y (1 - y) without the cancellation at y -> 1
        mag_y = y1y * m2 + y
        env = {"rgb": mag_y}
        dz2 = f(case.cots["d_rgb"]).abs() * ((1 - 2 * y).abs() * mag_y + y1y)
        dz1 = (dz2 @ W[4].abs()) * r1
        dz0 = (dz1 @ W[2].abs()) * r0
        env.update(d_w2=dz2.T @ m1, d_b2=dz2.sum(0), d_w1=dz1.T @ m0, d_b1=dz1.sum(0), d_w0=dz0.T @ xm, d_b0=dz0.sum(0),
                   d_emb=(dz0 @ W[0].abs())[:, 16:31])
    return {k: v + TINY for k, v in env.items()}


# ------------------------------------------------------------------------------------------------------------------------------ #
# comparators
# ------------------------------------------------------------------------------------------------------------------------------ #
def check_forward(case: Case, got: Dict, r64: Dict, env: Dict, report=None, prefix="") -> List[str]:
    """got: any of density, emb, sigma_raw (base) / rgb (head)."""
    fails = []
    for k in (("density", "emb", "sigma_raw") if case.mlp == "base" else ("rgb",)):
        if got.get(k) is not None:
            fails += RF.check(prefix + k, got[k], r64[k], env[k], K[f"{case.mlp}.{k}"], report)
    return fails


def check_backward(case: Case, got: Dict, r64: Dict, env: Dict, report=None, prefix="") -> List[str]:
    """got: the gradients of ``case.grads`` (inert samples carry zero cotangents on both sides, so their rows are exact zeros)."""
    fails = []
    for k in case.grads:
        if got.get(k) is not None:
            fails += RF.check(prefix + k, got[k], r64[k], env[k], K[f"{case.mlp}.{k}"], report)
    return fails


def condition_failures(case: Case, r64: Dict, env: Dict) -> List[str]:
    """The two conditions every case carries, from the float64 run alone: at most 2 % inert samples; with ``case.teeth``, at least
    90 % of the elements of every gradient tensor further than 16 x bound from zero."""
    fails = []
    share = float(case.inert.double().mean())
    if share > MAX_INERT:
        fails.append(f"{share:.4f} of the samples is inert")
    if case.mlp == "base":
        z = r64["sigma_raw"]
        if not float(z.abs().max()) < 80:
            fails.append(f"|sigma_raw| reaches {float(z.abs().max()):.1f}")
        if case.regime == "spread" and case.n >= TEETH_FROM_N:
            hi, lo = float((z > 15).double().mean()), float((z < -15).double().mean())
            if min(hi, lo) < 0.002 or hi + lo < 0.02:
                fails.append(f"only {hi:.4f} / {lo:.4f} of the samples is beyond the clamps")
    elif case.regime == "saturated":
        y = r64["rgb"]
        if not float(torch.log(y).min()) > -80:
            fails.append(f"the sigmoid's argument reaches {float(torch.log(y).min()):.1f}")
        if case.n >= TEETH_FROM_N and (float((y.float() == 1).float().mean()) < 0.01 or float((y < 1e-7).double().mean()) < 0.01):
            fails.append("the sigmoid does not saturate on both sides")
    if case.teeth:
        for k in case.grads:
            t = float((r64[k].abs() > RF.TEETH * K[f"{case.mlp}.{k}"] * U * env[k]).double().mean())
            if t < 0.9:
                fails.append(f"{k}: only {t:.3f} of the elements has teeth")
    return fails
