"""The yardstick of the clipping / LAMB tests: the definitions of include/vt_amd.h ("gradient norm, clipping, LAMB")
restated with torch tensors in whatever dtype the caller hands in -- float64 is the reference, float32 the "plain-f32
restatement" whose distance from float64 the CPU tests hold below half of every bound the GPU tests use -- plus the
inputs (oracle.filler) and the counted bounds both sides share.

The counted bounds, in units of u = 2^-24 (half an ulp of a float32, relative):
  C_NORM = 10.  A lane of vt_grad_sumsq adds at most 16 terms with fmaf(x, x, acc): 16 roundings on the way to a sum of
    non-negative terms, i.e. at most 16 u relative on the sum; everything above the lane (wave butterfly, the four waves,
    the partials) is double and contributes ~1e-16 per level; the square root halves the relative error (8 u), its own
    rounding and the product with grad_scale are double, and the store of N as a float32 adds 1 u: 9 u, counted as 10.
  C_SUM = 18.  A tensor's sum of p^2 (or of u^2, GIVEN the float32 u): the same 16 roundings per lane and double above,
    counted as 18 with the double levels.
  C_U = 7.  One u = fmaf(wd, p, (m / bc1) / (sqrtf(v) / bc2s + eps)) from float32 m, v, p: five correctly rounded
    operations in the quotient term (m / bc1, sqrt, / bc2s, + eps, the outer division) and the fused multiply-add's one:
    |u32 - u64| <= (5 |q| + |u|) u <= 6 (|q| + |wd p|) u, counted as 7.  With Cauchy-Schwarz the sum of u^2 moves by at
    most 2 sqrt(sum u^2) * C_U u * sqrt(sum (|q| + |wd p|)^2), which sum_u_bound adds to C_SUM u * sum u^2.
The elementwise bound of m, v and p is the AdamW kernel's rtol = atol = 1e-6 (tests/test_adamw_gpu.py): the same class of
arithmetic, one more factor (r) on the step."""
import math

import torch

from oracle import filler
from vision_toolbox import _native as N

U24 = 2.0 ** -24
C_NORM, C_SUM, C_U = 10, 18, 7
RTOL = ATOL = 1e-6
I = N.VT_OPT_ITEM

SUMSQ_LENGTHS = [4, 68, I - 4, I, I + 4, 3 * I + 8, 1_000_000]
LAMB_SIZES = [64, 64, I - 64, I, I + 64, 3 * I + 192, 128, 128, 256]
# per segment: weight decay; segment 1 has p = 0 (r = 1), segment 6 zero g and zero state, segment 4 wd = 0 between adapted ones
LAMB_WD = [0.05, 0.05, 0.01, 0.05, 0.0, 0.05, 0.02, 0.01, 0.05]
LAMB_ZERO_P, LAMB_ZERO_G, LAMB_PLAIN = 1, 6, 4
LAMB_SCALES = [1.0, -0.5, 2.0, 0.25, -1.5]  # a different gradient each step, as tests/test_adamw_gpu.py
LAMB_PAD = 192  # NaN-filled elements in front of and behind the table's range


def threshold_on(t) -> bool:
    return t is not None and t > 0 and not math.isinf(t)


def clip_factors(norm: float, C, M):
    """(c1, c2) of the definitions; `norm` = N, the norm of the averaged gradient"""
    c1 = 1.0
    if threshold_on(C):
        q = C / (norm + 1e-6)
        c1 = 1.0 if q > 1.0 else q  # NaN stays NaN
    c2 = 1.0
    if threshold_on(M):
        n1 = c1 * norm
        if n1 > M:
            c2 = n1 / M
    return c1, c2


def grad_norm(grads, s: float = 1.0):
    """N = s * sqrt(sum g^2) in the dtype of the gradients (a 0-d tensor)"""
    tot = sum((g.reshape(-1) * g.reshape(-1)).sum() for g in grads)
    return s * tot.sqrt()


def lamb_u(p, m, v, bc1, bc2s, eps, wd):
    return (m / bc1) / (v.sqrt() / bc2s + eps) + wd * p


class Lamb:
    """LAMB over a list of tensors (timm.optim.Lamb's form as vt_amd.h states it); works in the dtype of `params`"""

    def __init__(self, params, wds, lr, betas=(0.9, 0.999), eps=1e-6, s=1.0, C=None, M=1.0, trust_clip=False,
                 always_adapt=False):
        self.p = [p.clone() for p in params]
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.wds, self.lr, self.betas, self.eps, self.s, self.C, self.M = list(wds), lr, betas, eps, s, C, M
        self.trust_clip, self.always_adapt, self.t = trust_clip, always_adapt, 0
        self.info = {}

    def step(self, grads):
        dt = self.p[0].dtype
        self.t += 1
        b1, b2 = self.betas
        # the device keeps 1 - beta1^t and sqrt(1 - beta2^t) as float32 values made in double (vt_adam_tick); the float64
        # reference uses the exact ones -- the difference is part of what the 1e-6 bound covers, as for AdamW
        bc1, bc2s = 1.0 - b1 ** self.t, math.sqrt(1.0 - b2 ** self.t)
        if dt == torch.float32:
            bc1, bc2s = float(torch.tensor(bc1, dtype=dt)), float(torch.tensor(bc2s, dtype=dt))
        norm = float(grad_norm([g.double() for g in grads], self.s))
        c1, c2 = clip_factors(norm, self.C, self.M)
        factor = self.s * c1 / c2
        if dt == torch.float32:
            factor = float(torch.tensor(factor, dtype=dt))
        used, rs, sp, su = [], [], [], []
        for k, g in enumerate(grads):
            gg = g.to(dt) * factor
            used.append(gg)
            self.m[k] = b1 * self.m[k] + (1 - b1) * gg
            self.v[k] = b2 * self.v[k] + (1 - b2) * gg * gg
            u = lamb_u(self.p[k], self.m[k], self.v[k], bc1, bc2s, self.eps, self.wds[k])
            p2, u2 = float((self.p[k].double() ** 2).sum()), float((u.double() ** 2).sum())
            r = 1.0
            if self.wds[k] != 0 or self.always_adapt:
                if p2 > 0 and u2 > 0:
                    r = math.sqrt(p2) / math.sqrt(u2)
                if self.trust_clip:
                    r = min(r, 1.0)
            self.p[k] = self.p[k] - self.lr * r * u
            rs.append(r), sp.append(p2), su.append(u2)
        self.info = dict(norm=norm, c1=c1, c2=c2, factor=factor, used=used, r=rs, sum_p2=sp, sum_u2=su)
        return self.info


def sum_u_bound(p, m, v, bc1, bc2s, eps, wd) -> float:
    """absolute bound on a tensor's sum of u^2 as the kernel forms it, against the float64 sum of the float64 u of the SAME
    float32 operands (module docstring: C_SUM and C_U)"""
    p, m, v = p.double(), m.double(), v.double()
    q = (m / bc1) / (v.sqrt() / bc2s + eps)
    s_u = float(((q + wd * p) ** 2).sum())
    s_a = float(((q.abs() + (wd * p).abs()) ** 2).sum())
    return U24 * (C_SUM * s_u + 2 * C_U * math.sqrt(s_u * s_a)) + 1e-300


# ---- inputs ---------------------------------------------------------------------------------------------------------
def sumsq_input(n: int) -> torch.Tensor:
    return filler.tensor(f"lamb.sumsq.{n}", (n,))


def lamb_inputs():
    """(p0 per segment, [gradients per segment] per step) of the nine-segment table"""
    p0 = [filler.tensor(f"lamb.p.{k}", (n,)) for k, n in enumerate(LAMB_SIZES)]
    p0[LAMB_ZERO_P].zero_()
    grads = []
    for step, sc in enumerate(LAMB_SCALES):
        g = [sc * filler.tensor(f"lamb.g{step}.{k}", (n,)) for k, n in enumerate(LAMB_SIZES)]
        g[LAMB_ZERO_G].zero_()
        grads.append(g)
    return p0, grads


def lamb_offsets():
    offs, o = [], LAMB_PAD
    for n in LAMB_SIZES:
        offs.append(o)
        o += n
    return offs, o + LAMB_PAD  # (offsets, length of the flat buffers)


LAMB_VARIANTS = {  # name -> (trust_clip, always_adapt, M)
    "plain": (False, False, None),
    "trust_clip": (True, False, None),
    "always_adapt": (False, True, None),
    "max_norm": (False, False, 1.0),
    "all": (True, True, 1.0),
}
LAMB_LR, LAMB_BETAS, LAMB_EPS = 1e-3, (0.9, 0.999), 1e-6
