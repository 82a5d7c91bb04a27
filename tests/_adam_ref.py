"""The arithmetic of include/vsr_hip_opt.h restated in numpy: one numpy operation per rounded operation of the header, every array
float32; the scalars are formed in Python floats (float64) and rounded once.  Also the float64 squared norm (exact: math.fsum of exact
products) and the clip coefficient.  tests/test_adam_ref_helper.py pins it against torch.optim.Adam(foreach=False) on the CPU; the GPU
tests hold the kernels to it bit for bit."""
import math

import numpy as np

F = np.float32


def scalars(lr, beta1, beta2, eps, wd, t):
    """(omb1, b2, omb2, step_size, rs, eps, wd) as float32, each from a float64 expression rounded once."""
    return (F(1.0 - beta1), F(beta2), F(1.0 - beta2), F(lr / (1.0 - beta1 ** t)), F(math.sqrt(1.0 - beta2 ** t)), F(eps), F(wd))


def adam_step(p, g, m, v, lr, beta1, beta2, eps, wd, t, c=None):
    """One step at step count `t` (1 for the first).  p, g, m, v: float32 arrays; c: None or the float32 clip coefficient.
    -> (p', m', v'); nothing is modified in place."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    omb1, b2, omb2, step_size, rs, eps, wd = scalars(lr, beta1, beta2, eps, wd, t)
    with np.errstate(all="ignore"):
        g1 = g * F(c) if c is not None else g
        g2 = g1 + wd * p if wd != 0 else g1
        m1 = m + omb1 * (g2 - m)
        v1 = b2 * v + omb2 * (g2 * g2)
        d = np.sqrt(v1) / rs + eps
        p1 = p - step_size * (m1 / d)
    assert p1.dtype == m1.dtype == v1.dtype == d.dtype == np.float32
    return p1, m1, v1


def sumsq(grads):
    """The squared norm of float32 arrays, correctly rounded: every product of two float32 values is exact in float64 and math.fsum
    adds exactly."""
    return math.fsum(float(x) for g in grads for x in (g.astype(np.float64).ravel() ** 2))


def clip_coefficient(sumsq_value, max_norm):
    """(float)min(1.0, max_norm / (sqrt(sumsq) + 1e-6)), in float64."""
    return F(min(1.0, max_norm / (math.sqrt(sumsq_value) + 1e-6)))


def gradient_family(rs, n, clamp=False):
    """N(0,1) x 10^U(-6,2), one element in 16 exactly 0.  clamp: the magnitudes taken into [1e-6, 1e2] (no float32 denormal can then
    arise in a step: the smallest intermediate is omb2 * g^2 = 1e-15)."""
    g = rs.standard_normal(n) * 10.0 ** rs.uniform(-6.0, 2.0, n)
    if clamp:
        g = np.sign(g) * np.clip(np.abs(g), 1e-6, 1e2)
    g = g.astype(np.float32)
    g[rs.randint(0, 16, n) == 0] = 0.0
    return g
