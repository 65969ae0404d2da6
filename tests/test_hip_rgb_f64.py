"""The rgb-method MLP kernels (csrc/umhs_rgb.hip: rgb_mlp_fwd_kernel / rgb_mlp_bwd_kernel for mlp_base and mlp_head, rgb_mlp_reduce_kernel)
against a float64 oracle, element by element: cases, oracle runs, envelopes and the constants K are tests/rgb_f64.py's (its docstring
says which size selects which path of the tile loop and which regime which branch); tests/test_rgb_f64_bounds_cpu.py shows that the
comparators reject planted faults.

The kernels are called through umhsnerf.ops (rgb_base_fwd, rgb_head_fwd, RgbBaseFn, RgbHeadFn) with every output NaN before the launch
(``nan_prefill``), and through _hip.lib() where ops has no way in: NULL cotangents, accumulate = 1, buffers with sentinels behind them,
the refusals.  Figures measured on the way go to rgb_f64.json in G.report_dir(): per case and output, the worst |diff| / (u mag) and the
share of elements with teeth."""
import ctypes as C
import json
import os

import pytest
import torch

import rgb_f64 as G
from test_hip_rays_f64 import DEV, nan_prefill

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
SENTINEL = -12345.5
PAD = 64
OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    worst = {}
    for name, rep in REPORT.items():
        for k, v in rep.items():
            fam = f"{name.split('-')[0]}.{k.split('.')[-1]}"
            worst[fam] = max(worst.get(fam, 0.0), v["worst"])
    with open(os.path.join(G.report_dir(ROOT), "rgb_f64.json"), "w") as f:
        json.dump({"worst_ratio_per_family": worst, "K": G.K, "cases": REPORT}, f, indent=1)


def _mods():
    from umhsnerf import _hip, ops

    return ops, _hip


def _dev(case):
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    return {k: d(v) for k, v in case.inputs.items()}, [d(t) for t in case.weights], {k: d(v) for k, v in case.cots.items()}


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------ #
# every regime x size against float64
# ------------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spec", G.CASES, ids=G.case_id)
def test_rgb_mlp_kernels_against_float64(spec):
    ops, _ = _mods()
    case = G.make_case(*spec)
    r64, env = G.oracle(case, torch.float64), G.envelopes(case)
    cond = G.condition_failures(case, r64, env)
    assert not cond, cond
    report = REPORT.setdefault(G.case_id(spec), {})
    x, W, cot = _dev(case)
    if case.mlp == "base":
        with nan_prefill():
            density, emb, raw = ops.rgb_base_fwd(x["enc"], x["sel"], *W, want_emb=True, want_raw=True)
            only, no_emb, no_raw = ops.rgb_base_fwd(x["enc"], x["sel"], *W, want_emb=False)  # density_fn's form
            d3, no_emb3, raw3 = ops.rgb_base_fwd(x["enc"], x["sel"], *W, want_emb=False, want_raw=True)  # the normals path's form
        fails = G.check_forward(case, {"density": density, "emb": emb, "sigma_raw": raw}, r64, env, report)
        assert no_emb is None and no_raw is None and no_emb3 is None
        assert _same(only, density) and _same(d3, density) and _same(raw3, raw), "want_emb / want_raw changed density or sigma_raw"
        leaves = [x["enc"].clone().requires_grad_()] + [t.clone().requires_grad_() for t in W]
        sel = x["sel"] if x["sel"] is not None else torch.ones(case.n, device=DEV)  # (the autograd wrapper has no NULL selector)
        with nan_prefill():
            dens2, emb2 = ops.RgbBaseFn.apply(leaves[0], sel, *leaves[1:])
            grads = torch.autograd.grad([dens2, emb2], leaves, [cot["d_density"], cot["d_emb"]])
        assert _same(dens2.detach(), density) and _same(emb2.detach(), emb)
        if x["sel"] is None:  # selector == NULL in the backward: the C entry point, the same bits as a selector of ones
            d = Direct(case)
            assert d.backward() == OK
            null_sel = _shape_like(case, d.grads())
            fails += G.check_backward(case, dict(zip(case.grads, null_sel)), r64, env, report, prefix="null_selector.")
            assert all(_same(a, b) for a, b in zip(null_sel, grads))
    else:
        with nan_prefill():
            rgb = ops.rgb_head_fwd(x["dirs"], x["emb"], *W)
        fails = G.check_forward(case, {"rgb": rgb}, r64, env, report)
        leaves = [x["emb"].clone().requires_grad_()] + [t.clone().requires_grad_() for t in W]
        with nan_prefill():
            rgb2 = ops.RgbHeadFn.apply(x["dirs"], *leaves)
            grads = torch.autograd.grad(rgb2, leaves, cot["d_rgb"])
        assert _same(rgb2.detach(), rgb)
    fails += G.check_backward(case, dict(zip(case.grads, grads)), r64, env, report)
    print(G.case_id(spec), {k: (round(v["worst"], 3), v["teeth"]) for k, v in report.items()})
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------------ #
# the C entry points directly
# ------------------------------------------------------------------------------------------------------------------------------ #
class Direct:
    """One case's buffers for umhs_rgb_{base,head}_bwd / _fwd as ops.py calls them, every output with PAD sentinel floats behind it and
    the workspace with PAD sentinel floats behind umhs_rgb_mlp_bwd_workspace_bytes."""

    def __init__(self, case):
        self.ops, self._hip = _mods()
        self.lib, self.ptr = self._hip.lib(), self._hip.ptr
        self.case, self.head, self.n = case, case.mlp == "head", case.n
        self.x, self.W, self.cot = _dev(case)
        self.need = int(self.lib.umhs_rgb_mlp_bwd_workspace_bytes(int(self.head), self.n))
        assert self.need % 4 == 0
        self.ws = self.padded(self.need // 4)
        self.d_in = self.padded(self.n * (15 if self.head else 32))
        self.g = [self.padded(t.numel()) for t in self.W]
        fwd_cols = {"rgb": 3} if self.head else {"density": 1, "emb": 15, "sigma_raw": 1}
        self.out = {k: self.padded(self.n * c) for k, c in fwd_cols.items()}

    @staticmethod
    def padded(numel):
        return torch.full((numel + PAD,), SENTINEL, device=DEV, dtype=torch.float32)

    def forward(self, n=None):
        n, p, s = self.n if n is None else n, self.ptr, self._hip.stream()
        if self.head:
            return self.lib.umhs_rgb_head_fwd(p(self.x["dirs"]), p(self.x["emb"]), *[p(t) for t in self.W], n, p(self.out["rgb"]), s)
        return self.lib.umhs_rgb_base_fwd(p(self.x["enc"]), p(self.x["sel"]), *[p(t) for t in self.W], n, p(self.out["density"]),
                                          p(self.out["emb"]), p(self.out["sigma_raw"]), s)

    def backward(self, accumulate=0, cots=None, ws_ptr=None, ws_bytes=None, n=None):
        """``cots``: base (d_density | None, d_emb | None), head (d_rgb,)."""
        n, p, s = self.n if n is None else n, self.ptr, self._hip.stream()
        ws_ptr = p(self.ws) if ws_ptr is None else ws_ptr
        ws_bytes = self.need if ws_bytes is None else ws_bytes
        if self.head:
            (dr,) = (self.cot["d_rgb"],) if cots is None else cots
            return self.lib.umhs_rgb_head_bwd(p(self.x["dirs"]), p(self.x["emb"]), *[p(t) for t in self.W], p(dr), n, p(self.d_in),
                                              *[p(t) for t in self.g], accumulate, ws_ptr, ws_bytes, s)
        dd, de = (self.cot["d_density"], self.cot["d_emb"]) if cots is None else cots
        return self.lib.umhs_rgb_base_bwd(p(self.x["enc"]), p(self.x["sel"]), *[p(t) for t in self.W], p(dd), p(de), n, p(self.d_in),
                                          *[p(t) for t in self.g], accumulate, ws_ptr, ws_bytes, s)

    def grads(self):
        """d_in and the parameter gradients without their sentinels, in case.grads' order."""
        return [self.d_in[:-PAD].clone()] + [g[:-PAD].clone() for g in self.g]

    def untouched(self):
        """Names of the buffers whose sentinels were written over."""
        every = {"workspace": self.ws, "d_in": self.d_in, **{f"g{i}": g for i, g in enumerate(self.g)}, **self.out}
        return [k for k, t in every.items() if not bool((t[-PAD:] == SENTINEL).all())]

    def all_sentinel(self):
        every = [self.ws, self.d_in] + self.g + list(self.out.values())
        return all(bool((t == SENTINEL).all()) for t in every)


def _shape_like(case, flat):
    shapes = [(case.n, 15 if case.mlp == "head" else 32)] + [tuple(t.shape) for t in case.weights]
    return [t.view(s) for t, s in zip(flat, shapes)]


@pytest.mark.parametrize("n", [1, 17, 65, 16385])
@pytest.mark.parametrize("mlp,regime", [("base", "plain"), ("head", "planted")])
def test_nothing_is_written_behind_row_n_or_behind_the_workspace(mlp, regime, n):
    case = G.make_case(mlp, regime, n)
    r64, env = G.oracle(case, torch.float64), G.envelopes(case)
    d = Direct(case)
    assert d.forward() == OK and d.backward() == OK
    torch.cuda.synchronize()
    assert d.untouched() == []
    got = {k: v[:-PAD].view(r64[k].shape) for k, v in d.out.items()}
    got.update(zip(case.grads, _shape_like(case, d.grads())))
    fails = G.check_forward(case, got, r64, env) + G.check_backward(case, got, r64, env)  # (and the rows in front of them are right)
    assert not fails, fails


@pytest.mark.parametrize("mlp,regime", [("base", "spread"), ("head", "unit")])
def test_two_backward_runs_over_1024_slabs_are_identical(mlp, regime):
    d = Direct(G.make_case(mlp, regime, 40000))
    assert d.backward() == OK
    first = d.grads()
    d.ws.fill_(SENTINEL)
    assert d.backward() == OK
    assert all(_same(a, b) for a, b in zip(first, d.grads())), "the slab reduce sums in a fixed order"


@pytest.mark.parametrize("n", [17, 22789])
@pytest.mark.parametrize("mlp,regime", [("base", "spread"), ("head", "unit")])
def test_accumulate_adds_the_gradient_to_what_is_there(mlp, regime, n):
    """accumulate = 1: every parameter gradient becomes float32(prefill + g), g the accumulate = 0 result of the same launch order;
    the input gradient is overwritten either way."""
    d = Direct(G.make_case(mlp, regime, n))
    assert d.backward(accumulate=0) == OK
    plain = d.grads()
    gen = torch.Generator().manual_seed(n)
    prefill = [torch.randn(t.numel() - PAD, generator=gen).to(DEV) * float(g.abs().max()) for t, g in zip(d.g, plain[1:])]
    for t, p in zip(d.g, prefill):
        t[:-PAD] = p
    d.d_in.fill_(SENTINEL)
    assert d.backward(accumulate=1) == OK
    got = d.grads()
    assert _same(got[0], plain[0])
    for name, a, p, g in zip(d.case.grads[1:], got[1:], prefill, plain[1:]):
        assert _same(a, p + g), f"{name}: accumulate = 1 is not prefill + gradient"
    assert d.untouched() == []


@pytest.mark.parametrize("n", [17, 22789])
def test_a_null_cotangent_is_a_zero_cotangent(n):
    """umhs_rgb_base_bwd with d_density = NULL gives the bits of a zero d_density, and the same for d_emb (autograd materialises
    zeros, so ops never passes NULL)."""
    case = G.make_case("base", "spread", n)
    d = Direct(case)
    dd, de = d.cot["d_density"], d.cot["d_emb"]
    for cots, zeros in (((None, de), (torch.zeros_like(dd), de)), ((dd, None), (dd, torch.zeros_like(de)))):
        assert d.backward(cots=zeros) == OK
        want = d.grads()
        for t in [d.d_in] + d.g:
            t.fill_(SENTINEL)
        assert d.backward(cots=cots) == OK
        assert all(_same(a, b) for a, b in zip(want, d.grads()))
        assert bool((want[0] != 0).any())


@pytest.mark.parametrize("mlp,regime", [("base", "plain"), ("head", "unit")])
def test_refusals_return_before_any_launch(mlp, regime):
    d = Direct(G.make_case(mlp, regime, 65))
    assert d.backward(ws_bytes=d.need - 1) == ERR_WORKSPACE  # one byte short
    assert d.backward(ws_ptr=C.c_void_p(d.ws.data_ptr() + 4), ws_bytes=d.need) == ERR_WORKSPACE  # misaligned by 4 bytes
    assert d.backward(ws_ptr=C.c_void_p(0)) == ERR_WORKSPACE  # no workspace at all
    if mlp == "base":
        assert d.backward(cots=(None, None)) == ERR_ARG
    assert d.forward(n=0) == OK and d.backward(n=0) == OK  # an empty batch: nothing to do
    assert d.forward(n=-1) == ERR_ARG and d.backward(n=-1) == ERR_ARG
    torch.cuda.synchronize()
    assert d.all_sentinel(), "a refused or empty call wrote something"
    assert int(d.lib.umhs_rgb_mlp_bwd_workspace_bytes(int(d.head), 0)) == 0


def test_density_fn_is_get_density_at_the_same_positions():
    """20,000 positions (313 workgroups' worth: the capped grid's second trip): the occupancy grid's density_fn (want_emb = False, no
    autograd) and get_density (RgbBaseFn) give the same bits."""
    from umhsnerf._ns_compat import packed_ray_samples
    from umhsnerf.umhs_model import UMHSConfig

    bands = [400.0 + 10 * i for i in range(31)]
    m = UMHSConfig(log2_hashmap_size=14).setup(scene_box=None, num_train_data=1, metadata={"wavelengths": bands, "num_classes": 6},
                                               num_classes=6, seed=5).to(DEV)
    n = 20000
    pos = ((torch.rand(n, 3, generator=torch.Generator().manual_seed(3)) - 0.5) * 3.0).to(DEV)  # some outside the box
    z3, z1 = torch.zeros(n, 3, device=DEV), torch.zeros(n, 1, device=DEV)
    m.eval()
    with torch.no_grad():
        a = m.field.density_fn(pos)
        b, _ = m.field.get_density(packed_ray_samples(pos, z3, z1, z1))  # origin + 0 x direction: the position itself
    assert a.shape == b.shape == (n, 1) and bool(torch.isfinite(a).all()) and float(a.max()) > 0
    assert _same(a, b)
