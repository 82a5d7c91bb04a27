"""tests/_adam_ref.py (the numpy restatement of include/vsr_hip_opt.h that the GPU tests compare bits with) against
torch.optim.Adam(foreach=False) on the CPU: n = 200,003, p0 ~ N(0,1), g = N(0,1) x 10^U(-6,2) with one element in 16 exactly 0, drawn
anew at each of 8 steps, lr in {1e-3, 1e-1}, wd in {0, 1e-2}.  The bar, per tensor, for p, m and v:
max|ours - torch| <= 16 x 2^-23 x max|torch|.  (The restatement and torch differ in how they group the same operations -- torch forms
v with addcmul, p with addcdiv -- so they agree to a few float32 roundings of the largest element, not in their bits; measured on this
family with another seed: 9.9 (p), 1.4 (m) and 1.0 (v) of those units.  ULP distance is not used: m crosses zero.)"""
import math

import numpy as np
import pytest
import torch

import _adam_ref as R

N, STEPS, BAR = 200003, 8, 16 * 2.0 ** -23


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("lr", [1e-3, 1e-1])
def test_restatement_against_torch_adam_on_the_cpu(lr, wd):
    rs = np.random.RandomState(20261018)
    p = rs.standard_normal(N).astype(np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=lr, weight_decay=wd, foreach=False)
    for t in range(1, STEPS + 1):
        g = R.gradient_family(rs, N)
        assert (g == 0).mean() > 0.04
        p, m, v = R.adam_step(p, g, m, v, lr, 0.9, 0.999, 1e-8, wd, t)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
    st = opt.state[tp]
    units = {}
    for name, ours, ref in (("p", p, tp.detach().numpy()), ("m", m, st["exp_avg"].numpy()), ("v", v, st["exp_avg_sq"].numpy())):
        units[name] = np.abs(ours.astype(np.float64) - ref.astype(np.float64)).max() / (2.0 ** -23 * np.abs(ref).max())
    print(f"lr {lr} wd {wd}: units of 2^-23 x max|torch|: " + ", ".join(f"{k} {u:.2f}" for k, u in units.items()))
    for name, u in units.items():
        assert u * 2.0 ** -23 <= BAR, (name, u)
    assert float(st["step"]) == STEPS


def test_restatement_rounds_every_operation_in_float32():
    """Planted defects: the same step with one operation evaluated in float64 (what a contraction or a wider intermediate would do) is
    a different result, so the bit tests built on the restatement can see such a defect."""
    rs = np.random.RandomState(5)
    n = 4099
    p, g = rs.standard_normal(n).astype(np.float32), R.gradient_family(rs, n)
    m, v = (rs.standard_normal(n) * 0.1).astype(np.float32), (rs.uniform(0, 1, n) ** 2).astype(np.float32)
    p1, m1, v1 = R.adam_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3)
    omb1, b2, omb2, step_size, r, eps, wd = (np.float64(x) for x in R.scalars(1e-3, 0.9, 0.999, 1e-8, 1e-2, 3))
    g2 = g + (np.float32(wd) * p)
    v_fused = (b2 * v + omb2 * (g2.astype(np.float64) ** 2)).astype(np.float32)     # one rounding instead of four
    assert not np.array_equal(v_fused, v1)
    m_fused = (m + omb1 * (g2.astype(np.float64) - m)).astype(np.float32)
    assert not np.array_equal(m_fused, m1)
    # the scalars: rounded once from float64 (beta2 = 0.999 is not a float32 number; 1 - (float)0.999 != (float)(1 - 0.999))
    assert R.scalars(1e-3, 0.9, 0.999, 1e-8, 0, 1)[2] != np.float32(1.0) - np.float32(0.999)
    assert R.scalars(1e-3, 0.9, 0.999, 1e-8, 0, 2)[3] == np.float32(1e-3 / (1 - 0.81)) and \
        R.scalars(1e-3, 0.9, 0.999, 1e-8, 0, 2)[4] == np.float32(math.sqrt(1 - 0.999 ** 2))


def test_norm_and_coefficient():
    rs = np.random.RandomState(6)
    ints = [rs.randint(-15, 16, n).astype(np.float32) for n in (1, 5, 4097)]
    assert R.sumsq(ints) == float(sum(int((a.astype(np.int64) ** 2).sum()) for a in ints))
    assert R.clip_coefficient(4.0, 1.0) == np.float32(1.0 / (2.0 + 1e-6)) and R.clip_coefficient(4.0, 3.0) == np.float32(1.0)
    assert R.clip_coefficient(0.0, 1.0) == np.float32(1.0)
