"""``UMHSAdam.step`` (umhsnerf/optim.py) updates every element of the flat buffer exactly once, however it cuts the buffer: live rows,
rows plus a range, the pieces around what a backward already updated, the segments of an early-reduced gradient -- with the clamp
range re-based for each piece.  ``umhsnerf.optim.ops`` is replaced by a stand-in that applies tests/adam_f64.py's replay in place to
CPU tensors, counts the touches of every element and records the arguments of every call; the result is held, bit for bit, against
ONE replay of the whole buffer with the same clamp.  Layout, scenarios and driver are adam_f64's (PART_*, partition_steps); the GPU
runs the same scenarios through the real kernels in tests/test_hip_adam_f64.py."""
import numpy as np
import pytest
import torch

import adam_f64 as A

N, SPARSE_END = A.PART_N, A.PART_SPARSE_END


class ReplayOps:
    """adam_step, adam_step_rows and adam_step_rows_range of umhsnerf.ops on CPU tensors that view one flat buffer of N elements."""

    def __init__(self):
        self.touch, self.calls = np.zeros(N, np.int64), []

    @staticmethod
    def _offset(t) -> int:
        """The element of its flat buffer at which the view ``t`` begins."""
        off, rem = divmod(t.data_ptr() - t.untyped_storage().data_ptr(), 4)
        assert rem == 0 and 0 <= off and off + t.numel() <= N
        return off

    def _apply(self, p, g, m, v, at, hyper, scale, clamp):
        """The replay on elements ``at`` of p, g, m, v (views that begin at the same element); ``clamp`` in elements of the views."""
        pn, gn, mn, vn = (t.numpy() for t in (p, g, m, v))
        inside = np.zeros(pn.size, bool)
        inside[max(clamp[0], 0):max(min(clamp[1], pn.size), 0)] = True
        new = A.replay(pn[at], mn[at], vn[at], gn[at], hyper, scale)
        pn[at], mn[at], vn[at] = np.where(inside[at], A.clamp01(new[0]), new[0]), new[1], new[2]
        self.touch[self._offset(p) + at] += 1

    def adam_step(self, p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-15, grad_scale=1.0, clamp_range=(0, 0)):
        offs = {self._offset(t) for t in (p, g, m, v)}
        assert len(offs) == 1 and len({t.numel() for t in (p, g, m, v)}) == 1, "the four views cover the same elements"
        assert p.data_ptr() % 16 == 0, "the dense kernel needs 16-byte alignment"
        x = offs.pop()
        self.calls.append(("dense", x, x + p.numel(), step, lr, grad_scale, tuple(clamp_range)))
        self._apply(p, g, m, v, np.arange(p.numel()), A.Hyper(lr, betas[0], betas[1], eps, step), grad_scale, clamp_range)

    def adam_step_rows(self, p, g, m, v, rows, step, lr, betas=(0.9, 0.999), eps=1e-15, grad_scale=1.0):
        assert self._offset(p) == 0 and p.numel() == N
        self.calls.append(("rows", rows.tolist(), step, lr, grad_scale))
        r = rows.numpy()
        self._apply(p, g, m, v, np.stack([2 * r, 2 * r + 1], 1).reshape(-1), A.Hyper(lr, betas[0], betas[1], eps, step), grad_scale, (0, 0))

    def adam_step_rows_range(self, p, g, m, v, rows, begin, end, step, lr, betas=(0.9, 0.999), eps=1e-15, grad_scale=1.0, clamp_range=(0, 0)):
        assert self._offset(p) == 0 and p.numel() == N and 0 <= begin <= end <= N
        self.calls.append(("rows_range", rows.tolist(), begin, end, step, lr, grad_scale, tuple(clamp_range)))
        r = rows.numpy()
        hyper = A.Hyper(lr, betas[0], betas[1], eps, step)
        self._apply(p, g, m, v, np.stack([2 * r, 2 * r + 1], 1).reshape(-1), hyper, grad_scale, (0, 0))
        self._apply(p, g, m, v, np.arange(begin, end), hyper, grad_scale, clamp_range)  # the clamp: absolute elements, the range only


def _run(name, clamp, monkeypatch, **kw):
    """-> [(ops' calls of the step, touch counts of the step, Case before the step, p, m, v after it)] for two consecutive steps."""
    import umhsnerf.optim as optim

    fake = ReplayOps()
    monkeypatch.setattr(optim, "ops", fake)
    monkeypatch.setattr(optim, "world", lambda: (0, A.PART_SCENARIOS[name]["world"]))

    def fused_update(p, g, m, v, hyper, done, clamp):  # the backward's own Adam on [a, b): one touch each, the clamp where it reaches
        a, b = done
        fake._apply(p, g, m, v, np.arange(a, b), hyper, 1.0, clamp)

    out = []
    for before, p, m, v in A.partition_steps(name, clamp, "cpu", fused_update, **kw):
        out.append((fake.calls, fake.touch.copy(), before, p.numpy().copy(), m.numpy().copy(), v.numpy().copy()))
        fake.calls, fake.touch[:] = [], 0
    return out


def _clamped(x, y, clamp):
    """The absolute elements of [x, y) that a clamp range covers."""
    return set(range(max(clamp[0], x), min(clamp[1], y)))


ROWS = A.partition_rows().tolist()
# scenario -> the calls of one step: ("dense", begin, end) | ("rows",) | ("rows_range", begin, end)
EXPECTED_CALLS = {
    "a": [("dense", 0, 715)],
    "b": [("rows",), ("dense", 256, 715)],
    "c": [("rows_range", 512, 715)],
    "d": [("rows",)],
    "e": [("dense", 0, 128), ("dense", 384, 715)],
    "g": [("dense", 512, 715), ("rows",), ("dense", 256, 384), ("dense", 384, 512)],
}


def test_the_layout_is_what_the_scenarios_assume():
    assert len(ROWS) == 40 == len(set(ROWS)) and ROWS != sorted(ROWS) and min(ROWS) == 0 and max(ROWS) == 127
    live = A.partition_live()
    assert live[SPARSE_END:].all() and int(live[:SPARSE_END].sum()) == 80
    p, m, v, g = A.partition_state()
    assert not m[~live].any() and not v[~live].any() and not g[~live].any() and p.all() and m[live].all() and v[live].all() and g[live].all()
    assert (A.partition_state(1)[3] != g)[live].mean() > 0.9  # another gradient in the second step (but for those at the cap)
    assert A.partition_hyper(5).lr != A.partition_hyper(6).lr and A.partition_hyper(5).lr < A.PART_LR


@pytest.mark.parametrize("clamp", A.PART_CLAMPS, ids=lambda c: f"clamp{c[0]}-{c[1]}")
@pytest.mark.parametrize("name", list(EXPECTED_CALLS))
def test_every_element_is_updated_exactly_once(name, clamp, monkeypatch):
    sc = A.PART_SCENARIOS[name]
    live = A.partition_live() if sc["sparse"] else np.ones(N, bool)
    steps = _run(name, clamp, monkeypatch)
    assert len(steps) == 2
    for k, (calls, touch, before, p, m, v) in enumerate(steps):
        step, scale = A.PART_STEP0 + 1 + k, 1.0 / sc["world"]
        lr = A.partition_hyper(step).lr
        assert before.hyper.step == step and before.grad_scale == scale
        # once each: live rows, dense levels, tail; never: the other rows of the sparse levels
        assert (touch[live] == 1).all() and (touch[~live] == 0).all(), (name, step, np.nonzero(touch != live)[0][:10], touch[touch != live][:10])
        # one replay of the whole buffer, the same clamp
        assert A.check(p, m, v, before) == [], (name, step)
        # the arguments of every call
        assert [(c[0],) + tuple(c[1:3] if c[0] == "dense" else c[2:4] if c[0] == "rows_range" else ()) for c in calls] == EXPECTED_CALLS[name], calls
        done = _clamped(*sc["done"], clamp) if sc["done"] else set()
        seen = set(done)
        for c in calls:
            if c[0] == "dense":
                _, x, y, s, l, gs, (c0, c1) = c
                covered = set(range(x + max(c0, 0), x + min(c1, y - x)))
                assert covered == _clamped(x, y, clamp), (name, c)
                assert 0 <= c0 and c1 <= y - x  # re-based into the piece, not merely cut off by the kernel's own bounds
            elif c[0] == "rows":
                _, rows, s, l, gs = c
                assert rows == ROWS
                covered = set()
            else:
                _, rows, x, y, s, l, gs, (c0, c1) = c
                assert rows == ROWS
                covered = set(range(max(c0, x), min(c1, y)))
                assert covered == _clamped(x, y, clamp), (name, c)
            assert (s, l, gs) == (step, lr, scale), (name, c)
            assert not covered & seen
            seen |= covered
        assert seen == _clamped(0, N, clamp) - set(np.nonzero(~live)[0].tolist())  # every clamped element was clamped by exactly one piece


def test_a_fused_step_of_another_step_number_is_refused(monkeypatch):
    """Scenario f: adam_done carries another step number."""
    for name in ("c", "e"):
        with pytest.raises(RuntimeError, match="does not belong to this optimizer step"):
            _run(name, (0, 0), monkeypatch, wrong_step=True)


def test_moments_of_a_fresh_optimizer_start_at_zero(monkeypatch):
    """No state yet: step() creates zero moments and counts from step 1 (the driver above starts from a state of four steps)."""
    import umhsnerf.optim as optim

    fake = ReplayOps()
    monkeypatch.setattr(optim, "ops", fake)
    p0, _, _, g = A.partition_state()
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    param.grad = torch.from_numpy(g.copy())
    opt = optim.UMHSAdam([param], lr=2e-2, clamp_range=(600, 650))
    opt.step()
    st = opt.state[param]
    before = A.Case("fresh", p0, np.zeros(N, np.float32), np.zeros(N, np.float32), g, A.Hyper(2e-2, 0.9, 0.999, 1e-15, 1), 1.0, (600, 650))
    assert st["step"] == 1 and A.check(param.data, st["exp_avg"], st["exp_avg_sq"], before) == [] and (fake.touch == 1).all()
    assert fake.calls == [("dense", 0, N, 1, 2e-2, 1.0, (600, 650))]
