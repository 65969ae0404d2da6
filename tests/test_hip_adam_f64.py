"""The Adam kernels of csrc/umhs_adam.hip (``ops.adam_step``, ``ops.adam_step_rows``, ``ops.adam_step_rows_range``) and
``UMHSAdam.step`` on the GPU against tests/adam_f64.py: m and v bit for bit with the float32 replay of the kernel's expression, p, m and v
within the float64 oracle's envelope, p bit for bit with the replay, NaN / Inf where the replay has them, and every element outside
the call with its bits kept.  Cases, shapes and rules are adam_f64's (its docstring says which shape reaches which path);
tests/test_adam_f64_bounds_cpu.py shows that the comparator rejects planted faults, tests/test_adam_partition_cpu.py runs the
scenarios of ``UMHSAdam.step`` with a counting stand-in for the kernels.

Figures measured on the way go to adam_f64.json in A.report_dir(): per case the worst |got - oracle| / envelope of p, m and v and the
number of elements whose bits differ from the replay's."""
import json
import os

import numpy as np
import pytest
import torch

import adam_f64 as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    worst = lambda k: max([r[f"{k}_worst"] for r in REPORT.values()] or [0.0])
    total = lambda k: sum(r[k] for r in REPORT.values())
    summary = {"cases": len(REPORT), "worst envelope ratio": {k: worst(k) for k in "pmv"},
               "not bit-equal to the replay": {k: total(f"{k}_bits_differ") for k in "pmv"},
               "largest distance of p from the replay in ulps": max([r["p_max_ulp"] for r in REPORT.values()] or [0]),
               "untouched elements changed": sum(total(f"{k}_untouched_changed") for k in "pmv")}
    with open(os.path.join(A.report_dir(ROOT), "adam_f64.json"), "w") as f:
        json.dump({"u": {"mul add sub": A.U, "sqrt div": A.U2, "subnormal": A.T}, "summary": summary, "cases": REPORT}, f, indent=1)


@pytest.fixture(scope="module")
def ops():
    from umhsnerf import ops as O

    return O


def _to_dev(c):
    return [torch.from_numpy(a.copy()).to(DEV) for a in (c.p, c.g, c.m, c.v)]


def _launch(ops, c, p, g, m, v):
    """The call the case describes, on device buffers that hold the case's state."""
    h, call = c.hyper, c.call
    kw = dict(betas=(h.b1, h.b2), eps=h.eps, grad_scale=c.grad_scale)
    if "n" in call:  # dense: a slice that starts 48 bytes into the allocation
        sl = slice(call["begin"], call["begin"] + call["n"])
        assert p[sl].data_ptr() % 16 == 0 and p[sl].data_ptr() != p.data_ptr()
        ops.adam_step(p[sl], g[sl], m[sl], v[sl], h.step, h.lr, clamp_range=call["clamp"], **kw)
        return
    rows = torch.from_numpy(call["rows"]).to(DEV)
    if "begin" in call:
        assert call["begin"] % 2 == 1
        ops.adam_step_rows_range(p, g, m, v, rows, call["begin"], call["end"], h.step, h.lr, clamp_range=call["clamp"], **kw)
    else:
        ops.adam_step_rows(p, g, m, v, rows, h.step, h.lr, **kw)


def _same_bits(a, b) -> bool:
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", A.CASES)
def test_every_case_against_the_replay_and_the_float64_envelope(ops, name):
    c = A.case(name)
    p, g, m, v = _to_dev(c)
    g0 = g.clone()
    _launch(ops, c, p, g, m, v)
    fails = A.check(p, m, v, c, REPORT)
    r = REPORT[name]
    print(f"{name}: worst |got - float64| / envelope p {r['p_worst']:.3f} m {r['m_worst']:.3f} v {r['v_worst']:.3f}; bits differ p {r['p_bits_differ']} "
          f"(up to {r['p_max_ulp']} ulp) m {r['m_bits_differ']} v {r['v_bits_differ']} of {r['n']}")
    assert not fails, fails
    assert _same_bits(g, g0), "the gradient was written"


@pytest.mark.parametrize("kind", ["dense/1025/straddle", "rows/257", "rows_range/257+255/inside"])
def test_five_consecutive_steps_on_device_resident_state(ops, kind):
    """Zero moments, steps 1..5 with the scheduler's learning rate and a new gradient each: every step through ``check`` from the
    state the device held before it, and the state after the fifth against five replay steps from the start, bit for bit -- a kernel
    that does not write a moment back fails at step 2."""
    base = A.case(kind)
    n = base.p.size
    hp, hm, hv = base.p.copy(), np.where(base.mask, np.float32(0), base.m), np.where(base.mask, np.float32(0), base.v)  # the replay chain, on the host
    p, m, v = (torch.from_numpy(a.copy()).to(DEV) for a in (hp, hm, hv))
    for step in range(1, 6):
        hyper = A.Hyper(A.exp_decay_lr(step - 1), 0.9, 0.999, 1e-15, step)
        g_host = np.clip(A.elements(n, 900 + step)[3], -1e3, 1e3)
        c = A.Case(f"trajectory/{kind}/step{step}", p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), g_host, hyper, base.grad_scale, base.clamp,
                   base.mask, base.call)
        g = torch.from_numpy(g_host.copy()).to(DEV)
        _launch(ops, c, p, g, m, v)
        fails = A.check(p, m, v, c, REPORT)
        assert not fails, fails
        chain = A.Case("chain", hp, hm, hv, g_host, hyper, base.grad_scale, base.clamp, base.mask)
        hp, hm, hv = chain.expected()
    for what, got, want in (("p", p, hp), ("m", m, hm), ("v", v, hv)):
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), f"{kind}: {what} after five steps is not the replay's"
    assert np.abs(hm[base.mask]).min() > 0  # (every moment is alive after five steps)


@pytest.mark.parametrize("clamp", A.PART_CLAMPS, ids=lambda c: f"clamp{c[0]}-{c[1]}")
@pytest.mark.parametrize("name", ["a", "b", "c", "e", "g"])
def test_umhsadam_step_on_the_device(ops, name, clamp, monkeypatch):
    """The scenarios of tests/test_adam_partition_cpu.py with the real kernels: only the sink and ``world`` are faked (scenario g calls no
    collective: its segments cover the buffer).  Two consecutive steps, each against ONE replay of the whole buffer."""
    import umhsnerf.optim as optim

    monkeypatch.setattr(optim, "world", lambda: (0, A.PART_SCENARIOS[name]["world"]))

    def fused_update(p, g, m, v, hyper, done, clamp):  # what the bucket reduce's epilogue does to [a, b) before step() runs
        a, b = done
        rel = (max(clamp[0], a) - a, min(clamp[1], b) - a) if clamp[0] < b and clamp[1] > a else (0, 0)
        ops.adam_step(p[a:b], g[a:b], m[a:b], v[a:b], hyper.step, hyper.lr, (hyper.b1, hyper.b2), hyper.eps, clamp_range=rel)

    steps = 0
    for before, p, m, v in A.partition_steps(name, clamp, DEV, fused_update):
        fails = A.check(p, m, v, before, REPORT)
        assert not fails, fails
        steps += 1
    assert steps == 2
