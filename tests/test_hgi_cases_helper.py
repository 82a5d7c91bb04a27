"""The exact cases of tests/test_gpu_hg_inception.py stay inside their reference's own budget -- checked here on the CPU, with the very
operands the GPU test uses -- and the budget test is alive."""
import numpy as np
import pytest

import _exact as X
import _hgi_cases as C


@pytest.mark.parametrize("name", sorted(C.SIGS))
def test_every_exact_case_is_inside_the_budget(name):
    wts = C.exact_weights(name)
    (w0, b0), branches = wts
    assert bool((b0 != 0).all()) and all(bool((b1 != 0).all()) and bool((bk != 0).all()) for _, b1, _, bk in branches)   # non-zero biases
    for _, _, wk, _ in branches:   # every tap and both mid chunks carry weight somewhere
        assert bool((wk.abs().sum(0).reshape(-1, 32, wk.shape[-1] ** 2).sum(1) > 0).all())
    for hw in C.SIZES:
        y = C.exact_ref(wts, C.exact_input(name, hw))
        assert tuple(y.shape) == (C.NREF, C.parts(C.SIGS[name])[1] + sum(o for _, _, o in C.parts(C.SIGS[name])[2])) + tuple(hw)


def test_the_budget_test_catches_a_mid_that_would_round():
    (w0, b0), branches = C.exact_weights("A")
    bad = [(w1 + 2.0 ** -12, b1, wk, bk) for (w1, b1, wk, bk) in branches]
    with pytest.raises(X.BudgetError):
        C.exact_ref(((w0, b0), bad), X.ints(np.random.RandomState(0), (1, 128, 9, 17)))


@pytest.mark.parametrize("name", sorted(C.SIGS))
def test_every_rounding_case_is_inside_the_budget_and_rounds(name):
    """The rounding cases of tests/test_gpu_rounding.py: float32 budget, `check_rounds` on every mid map and every output sum (both run
    inside `round_ref`), and a block that read its UNROUNDED mid maps would move 5 % of the output."""
    import torch
    wts = C.round_weights(name)
    for hw in C.ROUND_SIZES:
        x = C.round_input(name, hw)
        y, pres = C.round_ref(wts, x)
        assert len(pres) == 1 + 2 * len(wts[1])
        outs = [X.act_round_ref(pres[0], 1)]
        for j, (w1, b1, wk, bk) in enumerate(wts[1]):
            k = wk.shape[-1]
            outs.append(X.act_round_ref(X.conv_ref(torch.relu(pres[1 + 2 * j]), wk, bk, padding=(k - 1) // 2), 1))
        other = torch.cat(outs, 1)
        assert int((other != y).sum()) >= 0.05 * y.numel(), (name, hw)
