"""The device side of a tests/field_f64.py case: parameters in the flat layout, inputs level-major and sample-major, and one method per
entry point of the field kernels (plain helper module, no tests in it).  Used by tests/test_hip_field_variants.py,
tests/field_tf_child.py (through it) and tests/test_hip_render_scale.py."""
import ctypes as C

import torch

import field_f64 as F

DEV = "cuda:0"


def _ops():
    from umhsnerf import ops

    return ops


class Hip:
    """One case on the device: parameters in the flat layout, inputs level-major and sample-major."""

    def __init__(self, case: F.Case):
        ops = _ops()
        self.case, n = case, case.n
        self.layout = ops.FieldLayout(case.C, case.B, case.spec, 12)
        flat = torch.zeros(self.layout.total)
        for k, v in case.p.reference_state_dict().items():
            self.layout.view(flat, k).copy_(v)
        self.flat = flat.to(DEV)
        self.fs = ops.FieldSpec(self.layout, case.temp, True, scalings=ops.hash_scalings().to(DEV))
        self.enc_lm = case.enc.view(n, 16, 2).permute(1, 0, 2).contiguous().to(DEV)
        self.enc_sm = case.enc.contiguous().to(DEV)
        self.wpos, self.dirs, self.sel = case.wpos.to(DEV), case.dirs.to(DEV), case.sel.to(DEV)
        self.t0, self.t1 = case.t0.to(DEV), case.t1.to(DEV)
        self.pinfo, self.ray_idx = case.packed_info().to(DEV), case.ray_indices().to(DEV)
        self._fwd = None

    def grads(self, d_flat):
        return {k: self.layout.view(d_flat, F.PARAM_KEYS[k]).cpu() for k, _ in F._params(self.case.p)}

    def fwd(self):
        if self._fwd is None:
            self._fwd = _ops().field_fwd(self.fs, self.flat, self.enc_lm, True, self.wpos, self.dirs, self.sel, want_emb=True, want_logits=True)
        return self._fwd

    def fwd_no_workspace(self):
        """umhs_field_fwd with workspace == NULL (every workgroup gathers its fp32 packs: the fp32 chain)."""
        ops = _ops()
        from umhsnerf import _hip
        from umhsnerf._hip import ptr

        n = self.case.n
        o = ops.field_fwd_outputs(self.fs, n, self.sel.device, want_emb=True, want_logits=True)
        cfg, pp = self.fs.cfg(False), self.layout.c_struct(self.flat, _hip.FieldParams)
        sn, sl = ops.enc_strides(n, True)
        _hip.check(_hip.lib().umhs_field_fwd(C.byref(cfg), C.byref(pp), ptr(self.enc_lm), sn, sl, ptr(self.wpos), ptr(self.dirs), ptr(self.sel), n,
                                             ptr(o["sigma"]), ptr(o["sigma_raw"]), ptr(o["emb"]), ptr(o["spectral"]), ptr(o["spectral2"]),
                                             ptr(o["specular"]), ptr(o["abundances"]), ptr(o["feat_logits"]), None, 0, 0, _hip.stream()),
                   "umhs_field_fwd")
        return o

    def two_launch(self):
        ops = _ops()
        assert ops.field_heads_fwd_supported(self.fs)
        base = ops.field_base_fwd(self.fs, self.flat, self.enc_lm, True, self.sel)
        w = ops.composite_fwd(base["sigma"], self.t0, self.t1, self.pinfo, [])[0]
        ho = ops.field_heads_fwd(self.fs, self.flat, base["emb"], self.wpos, self.dirs, w, self.ray_idx, self.pinfo, pack_ready=True, release=False,
                                 want_abundances=True)
        return base, w, ho

    def density(self):
        return _ops().field_fwd(self.fs, self.flat, self.enc_lm, True, None, None, self.sel, density_only=True)

    def bwd_plain(self, level_major: bool):
        c, o = self.case, self.fwd()
        d_flat = torch.zeros_like(self.flat)
        enc = self.enc_lm if level_major else self.enc_sm
        d_enc = _ops().field_bwd(self.fs, self.flat, enc, level_major, self.wpos, self.dirs, self.sel, o["sigma_raw"], o["emb"], c.cot_d.to(DEV),
                                 c.cot_s.to(DEV), c.cot_e.to(DEV), d_flat, feat_logits=o["feat_logits"])
        d_enc = d_enc.permute(1, 0, 2).reshape(c.n, 32) if level_major else d_enc
        return {"d_enc": d_enc.cpu(), "grads": self.grads(d_flat), "flat": d_flat.cpu()}

    def bwd_folded(self, grad_scaling: bool):
        ops, c, o = _ops(), self.case, self.fwd()
        w = ops.composite_fwd(o["sigma"], self.t0, self.t1, self.pinfo, [])[0]
        cp = dict(sigma=o["sigma"], t0=self.t0, t1=self.t1, packed_info=self.pinfo, ray_indices=self.ray_idx, weights=w, d_comp=c.d_comp.to(DEV),
                  d_acc=c.d_acc.to(DEV), grad_scaling=grad_scaling)
        d_flat = torch.zeros_like(self.flat)
        d_enc = ops.field_bwd(self.fs, self.flat, self.enc_lm, True, self.wpos, self.dirs, self.sel, o["sigma_raw"], o["emb"], None, None, None,
                              d_flat, feat_logits=o["feat_logits"], comp=cp)
        return {"d_enc": d_enc.permute(1, 0, 2).reshape(c.n, 32).cpu(), "d_sigma": cp["d_sigma"].cpu(), "grads": self.grads(d_flat),
                "flat": d_flat.cpu()}


def _logits(o, case):
    return o["feat_logits"][:, : case.C + int(case.spec)]
