"""CPU checks of tests/adam_f64.py: the replay on hand-made elements whose float32 arithmetic is exact, one step against
torch.optim.Adam in float64, ``bias`` against 1 - b^step by hand, the comparator against the mutants it has to catch and at the edge
of the envelope, and the host-side argument checks of the three entry points (nothing is launched)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import adam_f64 as A

F32 = np.float32
NAN, INF = float("nan"), float("inf")
f32 = lambda *x: np.array(x, F32)
bits = lambda a: np.asarray(a, F32).view(np.int32).tolist()


def test_replay_on_hand_made_elements_in_exact_float32_arithmetic():
    """b1 = 1/2, b2 = 3/4, step 1: bc1 = 1/2, bc2 = 1/4, so lr = 1/4 gives lr_bc1 = 1/2 and sqrt_bc2 = 1/2; eps = 2.  Every
    intermediate below is a dyadic number of a few bits: no operation rounds."""
    h = A.Hyper(0.25, 0.5, 0.75, 2.0, 1)
    assert A.bias(*h[:3], h.step) == (F32(0.5), F32(0.5))
    #          first step           g = 0, moments alive   all zero: p keeps its bits     clamp range [6, 9): both ends
    p = f32(1.0,    1.0,   0.5,     0.5,                   0.3, -0.0,                     0.0625, 0.5,  1.0,     0.0625, 1.0)
    g = f32(2.0,   -2.0,   0.0,    -0.0,                   0.0,  0.0,                     2.0,    2.0, -2.0,     2.0,   -2.0)
    m = f32(0.0,    0.0,  -8.0,     8.0,                   0.0,  0.0,                     0.0,    0.0,  0.0,     0.0,    0.0)
    v = f32(0.0,    0.0,  12.0,    12.0,                   0.0,  0.0,                     0.0,    0.0,  0.0,     0.0,    0.0)
    rp, rm, rv = A.replay(p, m, v, g, h, 1.0, (6, 9))
    # g = +-2: m' = +-1, v' = 4 / 4 = 1, denom = 1 / (1/2) + 2 = 4, p' = p -+ (1/2)(1/4)
    # g = 0, m = -+8, v = 12: m' = -+4, v' = 9, denom = 3 / (1/2) + 2 = 8, p' = p +- (1/2)(4/8): the parameter moves without a gradient
    assert rm.tolist() == [1.0, -1.0, -4.0, 4.0, 0.0, 0.0, 1.0, 1.0, -1.0, 1.0, -1.0]
    assert rv.tolist() == [1.0, 1.0, 9.0, 9.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert rp.tolist() == [0.875, 1.125, 0.75, 0.25, float(F32(0.3)), -0.0,    0.0, 0.375, 1.0,    -0.0625, 1.125]
    assert bits(rp[4:6]) == bits(p[4:6]) and bits(rm[4:6]) == bits(rv[4:6]) == [0, 0]  # -0.0 stays -0.0
    # grad_scale: g = 4 scaled by 1/2 is the first element again; a scale of 1/4 gives m' = 1/2, v' = 1/4, denom = 3, one rounded quotient
    assert [a.tolist() for a in A.replay(f32(1.0), f32(0.0), f32(0.0), f32(4.0), h, 0.5)] == [[0.875], [1.0], [1.0]]
    rp, rm, rv = A.replay(f32(1.0), f32(0.0), f32(0.0), f32(4.0), h, 0.25)
    assert (rm[0], rv[0]) == (0.5, 0.25) and rp[0] == F32(1.0) - F32(0.5) * (F32(0.5) / F32(3.0))
    # the clamp is torch.clamp_'s: a NaN stays, inside the range as outside it; +-Inf gradients give Inf moments and a NaN parameter
    rp, rm, rv = A.replay(f32(0.5, 0.5, 0.5, 0.5), f32(0, 0, 0, 0), f32(0, 0, 0, 0), f32(NAN, NAN, INF, -INF), h, 1.0, (0, 3))
    assert np.isnan(rp).all() and np.isnan(rm[:2]).all() and np.isnan(rv[:2]).all()
    assert bits(A.replay(f32(-0.0, -0.0), f32(0, 0), f32(0, 0), f32(0, 0), h, 1.0, (0, 1))[0]) == bits(f32(-0.0, -0.0))  # and -0 stays -0
    assert rm[2:].tolist() == [INF, -INF] and rv[2:].tolist() == [INF, INF]


@pytest.mark.parametrize("betas,lr,slack", [((0.5, 0.75), 2.0 ** -6, 0.0), ((0.9, 0.999), 2e-2, 2.01)])
def test_one_step_from_zero_moments_against_torch_adam_in_float64(betas, lr, slack):
    """torch.optim.Adam on float64 tensors with the float32-rounded hyper-parameters: the replay lies within the oracle's envelope of
    it.  With betas (1/2, 3/4) and lr = 2^-6 the two bias factors are exact in float32 and nothing is added; with the project's betas
    float32(lr / bc1) and float32(sqrt(bc2)) each round once (relative 2^-24) where torch keeps doubles -- two roundings of the step
    lr_bc1 (m / denom), allowed for as 2.01 U |p' - p| -- which the oracle, given the kernel's float32 factors, has no term for."""
    n = 4096
    p, m, v, g = A.elements(n, 7, "zero")
    h = A.Hyper(lr, betas[0], betas[1], 1e-15, 1)
    tp = torch.from_numpy(p.astype(np.float64)).requires_grad_()
    opt = torch.optim.Adam([tp], lr=float(F32(lr)), betas=(float(F32(betas[0])), float(F32(betas[1]))), eps=float(F32(h.eps)))
    tp.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    want = {"p": tp.detach().numpy(), "m": opt.state[tp]["exp_avg"].numpy(), "v": opt.state[tp]["exp_avg_sq"].numpy()}
    got = dict(zip("pmv", A.replay(p, m, v, g, h)))
    orc = dict(zip("pmv", A.oracle(p, m, v, g, h)))
    step = np.abs(want["p"] - p.astype(np.float64))
    for k in "pmv":
        ref, env = orc[k]
        allowed = env + (slack * A.U * step if k == "p" else 0.0)
        assert np.isfinite(want[k]).all() and np.isfinite(ref).all()
        same = 1e-12 * (np.abs(want[k]) + step) + (slack * A.U * step if k == "p" else 0.0)
        assert (np.abs(ref - want[k]) <= same).all(), k  # the oracle IS torch's update, up to the order of double operations
        assert (np.abs(got[k].astype(np.float64) - want[k]) <= allowed).all(), k
    assert float(np.median(orc["p"][1] / np.spacing(np.abs(got["p"])))) < 4.0  # the envelope is a few ulp of p, not a loose bound


def test_bias_is_one_minus_beta_to_the_step_in_double():
    lr, b1, b2 = 2e-2, 0.9, 0.999
    lrf, b1f, b2f = float(F32(lr)), float(F32(b1)), float(F32(b2))
    assert (lrf, b1f, b2f) != (lr, b1, b2)  # the float32 arguments are not the Python doubles
    for step in (1, 2):  # exact rationals: b^1 and b^2 (48 bits) are doubles
        bc1, bc2 = float(1 - Fraction(b1f) ** step), float(1 - Fraction(b2f) ** step)
        assert A.bias(lr, b1, b2, step) == (F32(lrf / bc1), F32(math.sqrt(bc2))), step
    assert A.bias(lr, b1, b2, 1)[0] == F32(lrf / (1.0 - b1f)) and abs(float(A.bias(lr, b1, b2, 1)[0]) - 0.2) < 1e-7
    assert A.bias(lr, b1, b2, 1000) == (F32(lrf / (1 - b1f ** 1000)), F32(math.sqrt(1 - b2f ** 1000)))
    assert 0.79 < float(A.bias(lr, b1, b2, 1000)[1]) < 0.80  # sqrt(1 - e^-1)
    # step 30000: 0.9^30000 underflows to 0, bc1 is exactly 1; 0.999^30000 = 9e-14, sqrt(bc2) rounds to 1 in float32
    assert b1f ** 30000 == 0.0 and 0 < b2f ** 30000 < 1e-13
    assert A.bias(lr, b1, b2, 30000) == (F32(lr), F32(1.0))
    assert b2f ** (2 ** 31 + 1) == 0.0 and A.bias(lr, b1, b2, 2 ** 31 + 1) == (F32(lr), F32(1.0))
    assert all(type(x) is np.float32 for x in A.bias(lr, b1, b2, 7))


def test_the_true_replay_passes_every_case_and_the_cases_hold_what_they_promise():
    seen = {"steps": set(), "scales": set(), "eps": set(), "zero moments": 0, "alive": 0, "NaN in the clamp range": 0}
    for name in A.CASES:
        c = A.case(name)
        rep = {}
        assert A.check(*c.expected(), c, rep) == [], name
        r = rep[name]
        assert max(r["p_worst"], r["m_worst"], r["v_worst"]) <= 1.0 and r["p_bits_differ"] == r["m_bits_differ"] == r["v_bits_differ"] == 0
        seen["steps"].add(c.hyper.step), seen["scales"].add(c.grad_scale), seen["eps"].add(c.hyper.eps)
        t = c.mask
        seen["zero moments" if not c.m[t].any() else "alive"] += 1
        assert (c.p[~t] != 0).all() and (c.m[~t] != 0).all() and (c.v[~t] != 0).all() and (c.g[~t] != 0).all()  # sentinels, never zeros
        if r["n"] >= 64:
            g, m, v = c.g[t], c.m[t], c.v[t]
            p0, (p1, m1, v1) = c.p[t], (a[t] for a in c.expected())
            assert np.isnan(g).any() and (g == INF).any() and (g == -INF).any() and (g == 0).any() and np.signbit(g[g == 0]).any()
            assert np.isnan(p1[~np.isfinite(g)]).all()  # (inside the clamp range too)
            assert np.isnan(m1[np.isnan(g)]).all() and np.isnan(v1[np.isnan(g)]).all()
            still = (g == 0) & (m == 0) & (v == 0) & (p0 >= 0) & (p0 <= 1)  # (inside the clamp range the others would be clamped)
            assert still.any() and bits(p1[still]) == bits(p0[still])
            moves = (g == 0) & (m != 0)
            assert moves.any() and (p1[moves] != p0[moves]).any()
            assert (v[v > 0].min() < 2.0 ** -126 or not v.any()) and np.abs(g[np.isfinite(g)]).max() >= 1e17
        cb, ce = c.clamp
        if ce - cb >= 5 and t[cb + 2]:
            assert np.isnan(c.g[cb + 2]) and np.isnan(c.expected()[0][cb + 2])
            seen["NaN in the clamp range"] += 1
        if ce - cb >= 2 and t[cb:ce].all():  # both ends of the range have an element that the clamp alone holds in [0, 1]
            free = A.replay(c.p, c.m, c.v, c.g, c.hyper, c.grad_scale)[0]
            assert free[cb] < 0 and free[ce - 1] > 1 and c.expected()[0][cb] == 0 and c.expected()[0][ce - 1] == 1
            for i in (cb - 1, ce):
                if 0 <= i < t.size and t[i]:
                    assert not 0 <= free[i] <= 1 and c.expected()[0][i] == free[i]
    assert seen["steps"] == set(A.STEPS) and seen["scales"] == set(A.SCALES) and seen["eps"] == set(A.EPSS)
    assert seen["zero moments"] >= 4 and seen["alive"] >= 4 and seen["NaN in the clamp range"] >= 8
    assert {A.SPECS[n][1] for n in A.CASES if n.startswith("dense")} == {1, 3, 4, 5, 1023, 1025, 262147, 2097159}
    assert A.RANGE_BEGIN % 2 == 1 and all(A.case(n).call["rows"].max() * 2 + 1 < A.RANGE_BEGIN for n in A.CASES if n.startswith("rows_range/3"))


MUTANT_CASES = ("dense/1023/tail", "dense/1025/straddle", "rows/255", "rows_range/257+255/inside", "dense/262147/tail", "dense/262147/straddle",
                "dense/1025/tail")


def _mutant(c, kind, monkeypatch):
    """(p, m, v) of the whole buffers as a kernel with the named fault would leave them, or None where the case cannot show it."""
    h, clamp = c.hyper, c.clamp
    if kind == "b2 = 0.99":
        h = h._replace(b2=0.99 if h.b2 != 0.99 else 0.999)
    elif kind == "eps = 1e-8":
        h = h._replace(eps=1e-8 if h.eps != 1e-8 else 1e-15)
    elif kind == "step + 1":
        if h.step >= 30000:  # both bias terms are 1 from there on
            return None
        h = h._replace(step=h.step + 1)
    elif kind == "no sqrt_bc2":
        if h.step >= 30000:
            return None
        true_bias = A.bias
        monkeypatch.setattr(A, "bias", lambda *a: (true_bias(*a)[0], F32(1.0)))
    elif kind == "clamp off by one element":
        if clamp[1] <= clamp[0]:
            return None
        clamp = (clamp[0] + 1, clamp[1] + 1)
    out = A.replay(c.p, c.m, c.v, c.g, h, c.grad_scale, clamp)
    monkeypatch.undo()
    t = c.mask
    out = [np.where(t, new, old) for new, old in zip(out, (c.p, c.m, c.v))]
    if kind == "moment not written back":
        out[1] = c.m.copy()
    return out


@pytest.mark.parametrize("kind", ["b2 = 0.99", "no sqrt_bc2", "eps = 1e-8", "step + 1", "moment not written back", "clamp off by one element"])
def test_check_reports_every_mutant(kind, monkeypatch):
    shown = 0
    for name in MUTANT_CASES:
        c = A.case(name)
        got = _mutant(c, kind, monkeypatch)
        if got is None:
            continue
        shown += 1
        fails = A.check(*got, c)
        assert fails, (kind, name)
        if kind in ("no sqrt_bc2", "eps = 1e-8", "step + 1"):  # m and v are right: it is the envelope of p (and its bits) that speaks
            assert all(": p: " in f for f in fails) and any("outside the float64 envelope" in f for f in fails), fails
            lenient = A.check(*got, c, p_bits=False)
            assert lenient and all("envelope" in f or "NaN" in f or "Inf" in f for f in lenient), (kind, name, lenient)  # without the bit rule too
        if kind == "b2 = 0.99":
            assert any(": v: " in f and "bits" in f for f in fails) and not any(": m: " in f for f in fails)
        if kind == "moment not written back":
            assert all(": m: " in f for f in fails)
    assert shown >= 3, kind


def test_check_at_the_edge_of_the_envelope_and_outside_the_call():
    c = A.case("dense/1023/empty")
    p, m, v = (a.copy() for a in c.expected())
    (po, pe), (mo, me), (vo, ve) = c.oracle()
    t = c.mask
    i = int(np.nonzero(t & np.isfinite(po) & (pe > 8 * np.spacing(np.abs(p))))[0][0])  # an envelope of several float32 steps
    inside = p.copy()
    inside[i] = F32(po[i] + 0.5 * pe[i])
    rep = {}
    fails = A.check(inside, m, v, c, rep)  # 0.5 x the envelope: the envelope accepts it, only the bit rule speaks
    assert len(fails) == 1 and "differ from the replay in bits" in fails[0] and 0.4 < rep[c.name]["p_worst"] <= 1.0
    assert A.check(inside, m, v, c, p_bits=False) == [] and rep[c.name]["p_bits_differ"] == 1 and rep[c.name]["p_max_ulp"] >= 1
    for sign in (1.0, -1.0):
        edge = F32(po[i] + sign * pe[i])
        out = np.nextafter(edge, F32(sign * INF), dtype=F32)  # one float32 step outside
        assert abs(float(out) - po[i]) > pe[i]
        bad = p.copy()
        bad[i] = out
        fails = A.check(bad, m, v, c, p_bits=False)
        assert len(fails) == 1 and "outside the float64 envelope" in fails[0], fails
    # m and v: one ulp off is a bit failure whether or not the envelope (about one ulp itself) still holds it; far off is both
    j = int(np.nonzero(t & np.isfinite(mo) & (m != 0))[0][0])
    bad = m.copy()
    bad[j] = np.nextafter(m[j], F32(INF), dtype=F32)
    fails = A.check(p, bad, v, c)
    assert 1 <= len(fails) <= 2 and ": m: " in fails[0] and "bits" in fails[0] and "(up to 1 ulp)" in fails[0]
    bad = v.copy()
    bad[j] = v[j] * F32(1.001) + F32(1e-30)
    assert len(A.check(p, m, bad, c)) == 2
    # a NaN where the replay has a number, a number where it has a NaN, an Inf of the other sign
    nan_at, inf_at = int(np.nonzero(t & np.isnan(m))[0][0]), int(np.nonzero(t & (m == INF))[0][0])
    for at, value in ((j, NAN), (nan_at, 1.0), (inf_at, -INF), (inf_at, NAN)):
        bad = m.copy()
        bad[at] = value
        assert A.check(p, bad, v, c), (at, value)
    # outside the call: one bit of a neighbour
    for k, buf in enumerate((p, m, v)):
        for at in (A.LEAD - 1, A.LEAD + 1023):
            bad = [p, m, v]
            bad[k] = buf.copy()
            bad[k][at] = np.nextafter(buf[at], F32(0), dtype=F32)
            fails = A.check(*bad, c)
            assert len(fails) == 1 and "outside the call changed" in fails[0]
    assert A.check(p, m, v, c) == [] and A.check(torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v), c) == []


def test_the_clamped_oracle_accepts_either_side_within_the_envelope():
    h = A.Hyper(0.25, 0.5, 0.75, 2.0, 1)  # (exact arithmetic: the first test) p' = p - 1/8 for g = 2
    c = A.Case("edge", f32(0.125, 1.0, 0.125), f32(0, 0, 0), f32(0, 0, 0), f32(2.0, -2.0, 2.0), h, 1.0, (0, 2))
    p, m, v = c.expected()
    assert p.tolist() == [0.0, 1.0, 0.0] and A.check(p, m, v, c) == []
    for i in (0, 2):  # the other zero: inside the envelope, but not the replay's bits -- inside the clamp range as outside it
        neg = p.copy()
        neg[i] = -0.0
        assert len(A.check(neg, m, v, c)) == 1 and A.check(neg, m, v, c, p_bits=False) == []
    env = float(c.oracle()[0][1][0])  # the oracle's p' is exactly 0 before the clamp: its envelope reaches to both sides of the bound
    assert 2.0 ** -26 < env < 2.0 ** -22 and c.oracle()[0][0].tolist() == [0.0, 1.0, 0.0]
    for value, ok in ((0.5 * env, True), (-0.5 * env, True), (2 * env, False), (-2 * env, False)):
        near = p.copy()
        near[0] = value
        assert (A.check(near, m, v, c, p_bits=False) == []) == ok, value
        assert A.check(near, m, v, c)  # (the bit rule refuses all four)


def test_argument_errors_arrive_before_any_launch(built_library):
    from umhsnerf import _hip

    lib = _hip.lib()
    OK, ARG = 0, -1
    d, rows = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # never dereferenced
    hyper = (1e-2, 0.9, 0.999, 1e-15)

    def dense(n=16, step=1, p=d, g=d, m=d, v=d):
        return lib.umhs_adam_step(p, g, m, v, n, *hyper, step, 1.0, 0, 0, None)

    def by_rows(n_rows=4, step=1, p=d, g=d, m=d, v=d, r=rows):
        return lib.umhs_adam_step_rows(p, g, m, v, r, n_rows, *hyper, step, 1.0, None)

    def rows_range(n_rows=4, begin=9, count=5, step=1, p=d, g=d, m=d, v=d, r=rows):
        return lib.umhs_adam_step_rows_range(p, g, m, v, r, n_rows, begin, count, *hyper, step, 1.0, 0, 0, None)

    for call in (dense, by_rows, rows_range):
        assert call(step=0) == ARG and call(step=-3) == ARG
        for name in "pgmv":
            assert call(**{name: None}) == ARG, (call.__name__, name)
            assert call(**{name: ctypes.c_void_p(4096 + 4)}) == ARG, (call.__name__, name)  # off 8 (and 16) bytes
    assert dense(n=-1) == ARG and by_rows(n_rows=-1) == ARG
    assert rows_range(n_rows=-1) == ARG and rows_range(begin=-1) == ARG and rows_range(count=-1) == ARG
    assert by_rows(r=None) == ARG and rows_range(r=None) == ARG  # null rows with n_rows > 0
    for name in "pgmv":  # 8 bytes off a 16-byte boundary: the dense call's float4 lanes refuse it, the float2 rows take it
        off8 = {name: ctypes.c_void_p(4096 + 8)}
        assert dense(**off8) == ARG and by_rows(n_rows=0, **off8) == OK and rows_range(n_rows=0, count=0, **off8) == OK
    # nothing to do: OK without a launch (and without a rows pointer)
    assert dense(n=0) == OK and by_rows(n_rows=0) == OK and by_rows(n_rows=0, r=None) == OK
    assert rows_range(n_rows=0, count=0) == OK and rows_range(n_rows=0, count=0, r=None) == OK
    assert dense(n=0, step=0) == ARG and by_rows(n_rows=0, step=0) == ARG and rows_range(n_rows=0, count=0, step=0) == ARG
