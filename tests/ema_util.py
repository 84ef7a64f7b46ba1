"""The weight EMA of include/vt_amd.h restated in float64, for tests/test_ema_*.py.

Steps are numbered s = 0, 1, ..; step s updates the average iff s % period == 0; update 0 copies, every later update is
e <- e + alpha * (p - e) with alpha the f32 rounding of the double 1 - decay.

The bound: a blend of the kernel rounds twice, d = fl(p - e) and e' = fl(alpha * d + e) (one fma).  With |delta| <= u = 2^-24,
    |e'_got - e'_exact| <= alpha * u * |p - e| + u * |e'| <= C_BLEND * u * (|e| + |p|),   C_BLEND = 2
(alpha <= 1 and e' lies between e and p).  An error already in e enters the next blend multiplied by 1 - alpha, so over t
blends the sum of the per-blend terms bounds the total: at most min(t, 1 / alpha) of the largest term.  A copy is exact.
"""
from __future__ import annotations

import numpy as np
import torch

U24 = 2.0 ** -24
C_BLEND = 2  # roundings of one blend, in units of u * (|e| + |p|)

SKIP, COPY, BLEND = 0, 1, 2


def alpha_f32(decay: float) -> float:
    """alpha as the device holds it: 1 - decay in double, rounded to f32 once"""
    return float(np.float32(1.0 - float(decay)))


def modes(n_steps: int, period: int) -> list[int]:
    out, updates = [], 0
    for s in range(n_steps):
        if s % period == 0:
            out.append(COPY if updates == 0 else BLEND)
            updates += 1
        else:
            out.append(SKIP)
    return out


def run(ps, alpha: float, period: int = 1):
    """ps: the f32 (or f64) snapshots p_0, p_1, .. the steps see -> [(e, bound)] after every step, both float64 tensors
    (None, None in front of the first update).  `alpha` is a float: pass alpha_f32(decay)."""
    e, bound, out = None, None, []
    for mode, p in zip(modes(len(ps), period), ps):
        p = p.double()
        if mode == COPY:
            e, bound = p.clone(), torch.zeros_like(p)
        elif mode == BLEND:
            bound = bound * (1.0 - alpha) + C_BLEND * U24 * (e.abs() + p.abs())
            e = e + alpha * (p - e)
        out.append((e, bound))
    return out


def closed_form(e0, p, alpha: float, t: int):
    """t blends towards a CONSTANT p: e_t = p + (e_0 - p) * (1 - alpha)^t"""
    return p.double() + (e0.double() - p.double()) * (1.0 - alpha) ** t
