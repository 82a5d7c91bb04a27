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
