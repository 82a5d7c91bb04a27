"""Host-side checks of video_super_resolution_amd.optim.Adam (no GPU): its groups and state are torch.optim.Adam's, state_dicts pass
both ways and training continues from them, the object pickles through the driver's checkpoint functions without its buffers, and
what the device path does not implement raises instead of falling back."""
import copy
import pickle

import numpy as np
import pytest
import torch

from video_super_resolution_amd import driver, optim
from video_super_resolution_amd._lib import VsrHipError


def _params(seed=0, shapes=((3, 5), (7,), (1,))):
    rs = np.random.RandomState(seed)
    return [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(s).astype(np.float32))) for s in shapes]


def _stock_steps(opt, params, seed, steps):
    rs = np.random.RandomState(seed)
    for _ in range(steps):
        for p in params:
            p.grad = torch.from_numpy(rs.standard_normal(tuple(p.shape)).astype(np.float32))
        opt.step()


def _with_state(ours):
    """An optim.Adam over CPU parameters given a state as two steps of torch.optim.Adam leave it (its own step() needs the device)."""
    stock = torch.optim.Adam(_params(), lr=ours.param_groups[0]["lr"], foreach=False)
    _stock_steps(stock, stock.param_groups[0]["params"], 1, 2)
    sd = stock.state_dict()
    sd["param_groups"] = ours.state_dict()["param_groups"]
    ours.load_state_dict(sd)
    return stock


def test_group_keys_defaults_and_state_dict_keys_are_torch_adams():
    stock = torch.optim.Adam(_params())
    ours = optim.Adam(_params(), max_grad_norm=2.0)
    assert list(ours.param_groups[0].keys()) == list(stock.param_groups[0].keys())
    assert ours.defaults == stock.defaults
    assert "max_grad_norm" not in ours.param_groups[0] and ours.max_grad_norm == 2.0
    custom = optim.Adam(_params(), lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
    g = custom.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (3e-4, (0.8, 0.99), 1e-6, 0.1)
    _with_state(ours)
    _stock_steps(stock, stock.param_groups[0]["params"], 1, 2)
    a, b = ours.state_dict(), stock.state_dict()
    assert a.keys() == b.keys() and a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert list(a["state"][k].keys()) == list(b["state"][k].keys()) == ["step", "exp_avg", "exp_avg_sq"]
        st = a["state"][k]["step"]
        assert st.dtype == torch.float32 and st.device.type == "cpu" and st.dim() == 0
    assert "max_grad_norm" not in str(a["param_groups"])
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(weight_decay=-1.0),
                dict(max_grad_norm=0.0), dict(max_grad_norm=float("nan")), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            optim.Adam(_params(), **bad)


def test_load_state_dict_both_ways_and_training_continues():
    # torch -> ours -> torch: the state survives unchanged, and the stock optimizer continues from it as if nothing had happened
    straight = torch.optim.Adam(_params(), lr=1e-2, foreach=False)
    _stock_steps(straight, straight.param_groups[0]["params"], 1, 2)
    ours = optim.Adam(_params(), lr=1e-2)
    ours.load_state_dict(copy.deepcopy(straight.state_dict()))
    for p in ours.param_groups[0]["params"]:
        st = ours.state[p]
        assert float(st["step"]) == 2.0 and st["step"].device.type == "cpu" and st["exp_avg"].shape == p.shape
    resumed_params = [torch.nn.Parameter(p.detach().clone()) for p in straight.param_groups[0]["params"]]
    resumed = torch.optim.Adam(resumed_params, lr=1e-2, foreach=False)
    resumed.load_state_dict(ours.state_dict())                        # ours -> torch
    _stock_steps(straight, straight.param_groups[0]["params"], 7, 3)
    _stock_steps(resumed, resumed_params, 7, 3)
    for a, b in zip(straight.param_groups[0]["params"], resumed_params):
        assert torch.equal(a, b)
    for a, b in zip(straight.state_dict()["state"].values(), resumed.state_dict()["state"].values()):
        assert float(a["step"]) == float(b["step"]) == 5.0
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])


def test_pickle_round_trip_through_the_drivers_checkpoint(tmp_path):
    class Holder(torch.nn.Module):   # what checkpoint_state / load_checkpoint touch of a VSR: `.model`
        def __init__(self):
            super().__init__()
            self.model = torch.nn.Linear(3, 2)
    m = Holder()
    ours = optim.Adam(m.parameters(), lr=2e-3, weight_decay=1e-2, max_grad_norm=0.5)
    stock = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in m.parameters()], lr=2e-3, foreach=False)
    _stock_steps(stock, stock.param_groups[0]["params"], 3, 2)
    sd = stock.state_dict()
    sd["param_groups"] = ours.state_dict()["param_groups"]
    ours.load_state_dict(sd)
    ours._plans["stale"] = object()          # what a step would have left: none of it may travel
    ours._ctl = torch.zeros(2, dtype=torch.float64)
    ours.launches = 3
    state = ours.__getstate__()
    assert sorted(state) == ["defaults", "max_grad_norm", "param_groups", "state"]
    name = driver.save_checkpoint(driver.checkpoint_state(m, 4, optimizer=ours), False, str(tmp_path), "t")
    with pytest.raises(RuntimeError, match="trusted=True"):
        driver.load_checkpoint(Holder(), name)
    ckpt = driver.load_checkpoint(Holder(), name, trusted=True)
    back = ckpt["optimizer"]
    assert isinstance(back, optim.Adam) and ckpt["epoch"] == 4
    assert back.max_grad_norm == 0.5 and back.launches == 0 and len(back._plans) == 0 and back._ctl is None
    assert back.last_grad_norm_sq is None and back._pin == [None, None]
    a, b = back.state_dict(), ours.state_dict()
    assert a["param_groups"] == b["param_groups"]
    for k in b["state"]:
        for name_ in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][k][name_], b["state"][k][name_])
    again = pickle.loads(pickle.dumps(back))
    assert again.state_dict()["param_groups"] == b["param_groups"] and again.max_grad_norm == 0.5
    again.zero_grad()                         # the unpickled object is a working Optimizer


def test_step_on_cpu_parameters_raises():
    ps = _params()
    ours = optim.Adam(ps)
    assert ours.step() is None                # no gradient anywhere: nothing to do, as torch
    ps[1].grad = torch.ones_like(ps[1])
    before = [p.detach().clone() for p in ps]
    with pytest.raises(VsrHipError, match="CPU tensor"):
        ours.step()
    assert all(torch.equal(a, b) for a, b in zip(before, ps)) and len(ours.state[ps[1]]) == 0   # nothing was updated on the side
    with pytest.raises(VsrHipError, match="CPU tensor"):
        optim.Adam(ps, max_grad_norm=1.0).step()


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay"])
def test_each_unsupported_flag_raises_at_step(flag):
    ps = _params()
    ours = optim.Adam(ps)
    assert flag in ours.param_groups[0] and ours.param_groups[0][flag] is False
    ours.param_groups[0][flag] = True
    ps[0].grad = torch.ones_like(ps[0])
    with pytest.raises(VsrHipError, match=f"{flag}=True is not implemented"):
        ours.step()
    # ... also when the flag arrives in a loaded state_dict
    ours2 = optim.Adam(_params())
    sd = ours2.state_dict()
    sd["param_groups"][0][flag] = True
    ours2.load_state_dict(sd)
    ours2.param_groups[0]["params"][0].grad = torch.ones(3, 5)
    with pytest.raises(VsrHipError, match=flag):
        ours2.step()
