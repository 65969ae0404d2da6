"""Float64 NumPy restatement of Vertex Component Analysis as the reference's ``umhsnerf/data/utils/vca.py`` computes it (Nascimento &
Dias), the synthetic cubes the VCA tests share, and float64 stand-ins for the three GPU passes -- in the style of field_f64.py:
plain arithmetic on whole arrays, no shortcut through the moments, so it checks the package's split from the outside.

The branch below the SNR threshold (projection to R-1 dimensions) is restated from the published algorithm: the reference's own
lines for it sit under ``if verbose:`` and cannot run (tests/golden/make_golden_vca.py records the exception)."""
import numpy as np


def make_cube(shape, bands, num_classes, snr_db, seed):
    """Linear mixtures with one pure pixel per endmember: R Gaussian-bump spectra 0.15 + 0.7 exp(-((l - c_k) / 0.18)^2) on l in
    [0, 1] (c_k evenly spread), Dirichlet(0.6) abundances, white noise at ``snr_db``, clipped to [0, 1], float32 [*shape, bands]."""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    lam = np.linspace(0.0, 1.0, bands)
    centres = (np.arange(num_classes) + 0.5) / num_classes
    M = 0.15 + 0.7 * np.exp(-(((lam[None, :] - centres[:, None]) / 0.18) ** 2))
    a = rs.dirichlet(0.6 * np.ones(num_classes), n)
    a[rs.choice(n, num_classes, replace=False)] = np.eye(num_classes)
    y = a @ M
    sigma = np.sqrt(np.mean(y ** 2) / 10 ** (snr_db / 10))
    y = y + sigma * rs.randn(n, bands)
    return np.clip(y, 0, 1).astype(np.float32).reshape(*shape, bands)


def draws_from_seed(num_classes, seed):
    """What the reference's loop draws after ``np.random.seed(seed)``: R calls of ``rand(R, 1)``; column i = w_i."""
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.rand(num_classes, 1) for _ in range(num_classes)], axis=1)


def vca_f64(Y, R, draws):
    """Y [B,N] (pixels as columns), draws [R,R] -> (Ae [B,R], indices [R], info {snr, snr_th, branch, margins [R]}); margins[i] =
    (top1 - top2) / top1 of |v| at step i: how far an fp32 evaluation may move |v| before it picks another pixel."""
    Y = np.asarray(Y, np.float64)
    B, N = Y.shape
    m = np.mean(Y, axis=1, keepdims=True)
    Yo = Y - m
    Ud = np.linalg.svd(Yo @ Yo.T / N)[0][:, :R]
    xp = Ud.T @ Yo
    P_y = np.sum(Y ** 2) / N
    P_x = np.sum(xp ** 2) / N + np.sum(m ** 2)
    snr = 10 * np.log10((P_x - R / B * P_y) / (P_y - P_x))
    snr_th = 15 + 10 * np.log10(R)
    if snr < snr_th:
        branch, d = "affine", R - 1
        Ud = Ud[:, :d]
        x = Ud.T @ Yo
        Yp = Ud @ x + m
        c = np.sqrt(np.max(np.sum(x ** 2, axis=0)))
        y = np.vstack([x, c * np.ones((1, N))])
    else:
        branch = "projective"
        Ud = np.linalg.svd(Y @ Y.T / N)[0][:, :R]
        x = Ud.T @ Y
        Yp = Ud @ x
        u = np.mean(x, axis=1, keepdims=True)
        y = x / (u.T @ x + 1e-6)
    A = np.zeros((R, R))
    A[-1, 0] = 1
    indices, margins = np.zeros(R, np.int64), np.zeros(R)
    for i in range(R):
        w = np.asarray(draws, np.float64)[:, i : i + 1]
        f = w - A @ (np.linalg.pinv(A) @ w)
        f = f / np.linalg.norm(f) + 1e-6
        v = np.abs(f.T @ y)[0]
        indices[i] = np.argmax(v)
        top = np.sort(v)[-2:]
        margins[i] = (top[1] - top[0]) / top[1]
        A[:, i] = y[:, indices[i]]
    return Yp[:, indices], indices, dict(snr=float(snr), snr_th=float(snr_th), branch=branch, margins=margins)


class F64Passes:
    """NumPy stand-ins for the three GPU passes (what ``umhsnerf.data.utils.vca.HipPasses`` does on the device), float64: the
    package's host half runs on them unchanged."""

    def __init__(self, rows):
        self.rows = np.asarray(rows, np.float64)  # [N,B]
        self.y = None

    def moments(self):
        return self.rows.sum(0), self.rows.T @ self.rows, self.rows.shape[0]

    def project(self, plan):
        basis = plan["basis16"]
        if plan["branch"] == "affine":
            self.y = (self.rows - plan["mean"]) @ basis
            return float(np.max(np.sum(self.y ** 2, axis=1)))
        x = self.rows @ basis
        self.y = x / (x[:, 15:16] + 1e-6)
        self.y[:, 15] = 0
        return None

    def argmax(self, f16, bias):
        i = int(np.argmax(np.abs(bias + self.y @ np.asarray(f16, np.float64))))
        return i, self.y[i]

    def pixels(self, indices):
        return self.rows[np.asarray(indices)]
