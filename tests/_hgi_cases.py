"""Cases of the one-launch inception block (tests/test_gpu_hg_inception.py) that need no GPU: the block signatures, the exact and the
Gaussian operands, and their float64 references.  tests/test_hgi_cases_helper.py checks on the CPU that every exact case stays inside
the reference's own budget."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _exact as X
from _round_cases import two_taps as _two_taps
from video_super_resolution_amd.depth import _A, _B, _C, _D, _E, _F, _G

SIGS = {"A": _A, "B": _B, "C": _C, "D": _D, "E": _E, "F": _F, "G": _G}
# 1x1, 3x5, 7x9: smaller than the 11x11 kernel; 9x17: one 8 x 16 tile plus ragged edges; 17x33: several ragged tiles
SIZES = [(1, 1), (3, 5), (7, 9), (9, 17), (17, 33)]
BIG_SIZES = [(33, 60), (67, 120)]
NREF = 3


def parts(node):
    _, cin, o0, *rest = node
    return cin, o0, rest


# ---------------------------------------------------------------------------------------------------------------- exact
@functools.lru_cache(maxsize=None)
def exact_weights(name):
    """Sparse integer weights: about 6 non-zero taps per 1x1 row and 60 per k x k row keep every mid value and every output a small
    integer (an fp16 value; the references check it) while every tap of every 32-channel chunk carries weight in some row; biases are
    non-zero integers."""
    cin, o0, rest = parts(SIGS[name])
    rs = np.random.RandomState(sum(map(ord, name)))

    def bias(n):
        return torch.from_numpy((rs.randint(1, 3, size=n) * (rs.randint(0, 2, size=n) * 2 - 1)).astype(np.float64))

    w0 = X.sparse_weights(rs, (o0, cin, 1, 1), density=6.0 / cin)
    branches = []
    for mid, k, out in rest:
        branches.append((X.sparse_weights(rs, (mid, cin, 1, 1), density=6.0 / cin), bias(mid),
                         X.sparse_weights(rs, (out, mid, k, k), density=60.0 / (mid * k * k)), bias(out)))
    return (w0, bias(o0)), branches


def exact_input(name, hw):
    """[NREF,cin,H,W] integers in -3..3, float64."""
    return X.ints(np.random.RandomState(hw[0] * 100 + hw[1]), (NREF, parts(SIGS[name])[0]) + tuple(hw))


def exact_ref(wts, x):
    """float64: cat(relu(1x1) | relu(k x k(relu(1x1))) x 3), every sum inside the float32 budget, every mid and output an fp16 value."""
    (w0, b0), branches = wts
    outs = [F.relu(X.conv_ref(x, w0, b0, what="plain 1x1", store=torch.float16))]
    for j, (w1, b1, wk, bk) in enumerate(branches):
        mid = F.relu(X.conv_ref(x, w1, b1, what=f"branch {j} 1x1", store=torch.float16))
        k = wk.shape[-1]
        outs.append(F.relu(X.conv_ref(mid, wk, bk, padding=(k - 1) // 2, what=f"branch {j} {k}x{k}", store=torch.float16)))
        if float((mid != 0).double().mean()) <= 0.1:
            raise X.BudgetError(f"branch {j}: degenerate mid map")
    y = torch.cat(outs, 1)
    if float((y != 0).double().mean()) <= 0.1:
        raise X.BudgetError("degenerate output")
    return y


# ---------------------------------------------------------------------------------------------------------------- Gaussian
@functools.lru_cache(maxsize=None)
def gauss_weights(name):
    cin, o0, rest = parts(SIGS[name])
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 7)

    def w(co, ci, k):
        return torch.randn((co, ci, k, k), generator=g, dtype=torch.float64) * (2.0 / (ci * k * k)) ** 0.5

    def b(n):
        return torch.randn(n, generator=g, dtype=torch.float64) * 0.25

    return (w(o0, cin, 1), b(o0)), [(w(mid, cin, 1), b(mid), w(out, mid, k), b(out)) for mid, k, out in rest]


def gauss_ref(wts, x16):
    """float64 with the kernels' operands: weights rounded to fp16, biases to float32, the mid maps rounded to fp16 after ReLU."""
    X._threads()
    (w0, b0), branches = wts

    def h(w):
        return w.to(torch.float16).double()

    def f(b):
        return b.to(torch.float32).double()

    outs = [F.relu(F.conv2d(x16, h(w0), f(b0)))]
    for w1, b1, wk, bk in branches:
        mid = F.relu(F.conv2d(x16, h(w1), f(b1))).to(torch.float16).double()
        outs.append(F.relu(F.conv2d(mid, h(wk), f(bk), padding=(wk.shape[-1] - 1) // 2)))
    return torch.cat(outs, 1)


# ---------------------------------------------------------------------------------------------------------------- rounding
# The Gaussian cases round their mid maps, but a float64 Gaussian sum is never half-way between two fp16 values and the 2 x bar above
# is a tolerance.  These cases keep the float32 budget of tests/_exact.py and make the sums 13 to 15 bits wide: each mid map and each
# output is the ONE round-to-nearest-even of an exact float32 sum behind its ReLU, ties included (`_exact.check_rounds`).
ROUND_SIZES = [(17, 33), (33, 60)]      # (on smaller maps most taps of an 11 x 11 row fall into the padding: too few sums round)


@functools.lru_cache(maxsize=None)
def round_weights(name):
    """1x1 rows: integers in +-8 on a share of the inputs that puts the sums of inputs in +-255 near 5000; k x k rows: two weights of +-1
    on the ROUNDED mid map (a sum of two 11-bit values and an integer bias rounds again and stays inside the fp16 range)."""
    cin, o0, rest = parts(SIGS[name])
    rs = np.random.RandomState(sum(map(ord, name)) + 11)
    dens = min(1.0, 5000.0 ** 2 / (255 * 256 / 3.0 * 25.5 * cin))

    def bias(n):
        return X.ints(rs, (n,), -2000, 2000)

    w0 = X.sparse_weights(rs, (o0, cin, 1, 1), dens, 8)
    branches = []
    for mid, k, out in rest:
        branches.append((X.sparse_weights(rs, (mid, cin, 1, 1), dens, 8), bias(mid), _two_taps(rs, out, mid * k * k).reshape(out, mid, k, k), bias(out)))
    return (w0, bias(o0)), branches


def round_input(name, hw):
    """[NREF,cin,H,W] integers in +-255, float64."""
    return X.ints(np.random.RandomState(hw[0] * 100 + hw[1] + 5), (NREF, parts(SIGS[name])[0]) + tuple(hw), -255, 255)


def round_ref(wts, x):
    """float64 sums inside the float32 budget, ReLU in float32, ONE rounding to fp16 at each of the two storage points; the k x k
    convolutions read the rounded mid maps.  Every pre-rounding map meets `check_rounds`.  -> (output, list of the pre-rounding maps)."""
    (w0, b0), branches = wts
    pres = [X.conv_ref(x, w0, b0, what="plain 1x1")]
    outs = [X.act_round_ref(pres[0], 1)]
    for j, (w1, b1, wk, bk) in enumerate(branches):
        m0 = X.conv_ref(x, w1, b1, what=f"branch {j} 1x1")
        mid = X.act_round_ref(m0, 1)
        k = wk.shape[-1]
        o0 = X.conv_ref(mid, wk, bk, padding=(k - 1) // 2, what=f"branch {j} {k}x{k}")
        outs.append(X.act_round_ref(o0, 1))
        pres += [m0, o0]
    for i, p in enumerate(pres):
        X.check_rounds(p, f"inception pre-rounding map {i}")
    return torch.cat(outs, 1), pres
