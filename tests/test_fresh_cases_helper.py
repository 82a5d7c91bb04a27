"""tests/_fresh_cases.py on the CPU: the live sets it finds are pinned, its groups cover them, every mutation changes every element, and
every cache key of the package (sr._weights_key, TrunkExecCache.key, trunk_f32._Packed / _Folded, GraphedVSR._key) moves with each of
them and with nothing else; optim.mark_updated moves a version without touching a value."""
import copy

import pytest
import torch
import torch.nn as nn

import _fresh_cases as C
from video_super_resolution_amd import GraphedVSR, optim, trunk_f32
from video_super_resolution_amd.trunk_exec import TrunkExecCache

CPU_KINDS = [k for k in C.mutations if k not in C.GPU_ONLY]


@pytest.mark.parametrize("scale", [4, 2, 3])
def test_live_set_is_pinned_and_the_dead_tensors_are_the_ones_the_dataflow_leaves_out(scale):
    """91 tensors, 83 live at every scale (the geometry of the (de)convolutions does not change the dataflow).  The eight others, found
    by the helper: hr[5] has no consumer (six groups: no downtran slice reads it), so upBlocks.5 (weight, bias, slope) and
    uptranBlocks.4, which only feeds it, have no path to the output; group 0 reads zeros, so the WEIGHTS of upBlocks.0 and
    downBlocks.0 have a zero gradient while their biases and slopes are live through the constant map."""
    m = C.sr_master(scale)
    live, dead = C.live_tensors(m), C.dead_tensors(m)
    assert len(C.named_tensors(m)) == 91 and len(live) == 83 and len(dead) == 8
    assert sorted(live + list(dead)) == sorted(C.named_tensors(m)) and not set(live) & set(dead)
    assert {n for n, why in dead.items() if why == "no path to the output"} == {
        "block.upBlocks.5.0.weight", "block.upBlocks.5.0.bias", "block.upBlocks.5.1.weight",
        "block.uptranBlocks.4.0.weight", "block.uptranBlocks.4.0.bias", "block.uptranBlocks.4.1.weight"}
    assert {n for n, why in dead.items() if why == "its gradient is zero everywhere"} == {"block.upBlocks.0.0.weight", "block.downBlocks.0.0.weight"}
    assert all(n in live for n in ("sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias"))   # frozen: found by perturbation


@pytest.mark.parametrize("scale", [4, 2, 3])
def test_groups_cover_the_live_set_once(scale):
    m = C.sr_master(scale)
    g = C.groups(m)
    flat = [n for names in g.values() for n in names]
    assert sorted(flat) == sorted(C.live_tensors(m)) and len(flat) == len(set(flat))
    assert tuple(g) == C.GROUP_NAMES
    assert len(g["slopes"]) == 25 and len(g["chain0"]) == len(g["chain3"]) == 6 and g["post"] == ["block.uptranBlocks.3.0.weight", "block.uptranBlocks.3.0.bias"]
    assert C.chain_group(m) == ["block.upBlocks.1.0.weight", "block.upBlocks.1.0.bias", "block.downBlocks.2.0.weight", "block.downBlocks.2.0.bias",
                                "block.downtranBlocks.1.0.weight", "block.downtranBlocks.1.0.bias"]


@pytest.mark.parametrize("kind", CPU_KINDS)
def test_every_mutation_changes_every_element_and_nothing_else(kind):
    m = copy.deepcopy(C.sr_master(4))
    names = C.chain_group(m) + ["conv_out.0.weight"] + ([] if kind in C.OPTIMIZER_KINDS else ["sub_mean.weight", "add_mean.bias"])
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    grads = {n: t.grad for n, t in C.named_tensors(m).items()}
    C.mutations[kind](m, names)
    after = m.state_dict()
    for k in before:
        if k in names:
            assert C.changed_everywhere(m, k, before[k], after[k]), (kind, k)
        else:
            assert torch.equal(before[k], after[k]), (kind, k)
    now = C.named_tensors(m)
    assert list(now) == list(grads) and all(now[n].grad is grads[n] for n in grads)
    assert all(now[n].requires_grad == (not n.startswith(("sub_mean", "add_mean"))) for n in now)
    if kind in C.OPTIMIZER_KINDS:
        with pytest.raises(ValueError):
            C.mutations[kind](m, ["sub_mean.bias"])


def test_the_new_value_survives_fp16_rounding_at_every_magnitude():
    m = C.sr_master(4)
    w = torch.cat((torch.zeros(1), 2.0 ** torch.arange(-24, 15, dtype=torch.float32), -(2.0 ** torch.arange(-24, 15, dtype=torch.float32)),
                   torch.tensor([65504.0 / 1.3, -0.0625, 0.0625, 1.0 - 2.0 ** -11])))
    new = C.new_value(m, "conv_out.0.bias", w)
    assert bool((new.half() != w.half()).all()) and bool((new.abs() > w.abs()).all()) and bool(torch.isfinite(new.half()).all())
    eye = C.new_value(m, "sub_mean.weight", m.sub_mean.weight)
    assert bool((eye.reshape(3, 3)[~torch.eye(3, dtype=torch.bool)] == 0).all()) and bool((torch.diagonal(eye.reshape(3, 3)) != 1).all())


# ---------------------------------------------------------------------------------------------------------------- the keys
def _keys(vsr, graphed, data):
    """Every key that guards a packed copy of `vsr`'s weights."""
    return {"sr": vsr.model._weights_key(), "flow": vsr._flow_exec.key(), "depth": vsr._depth_exec.key(), "vos": vsr._vos_exec.key(),
            "graph": graphed._key(data, None)}


@pytest.fixture(scope="module")
def vsr_copy(cpu_vsr):
    return copy.deepcopy(cpu_vsr)


def test_keys_are_equal_after_no_mutation(vsr_copy):
    g, data = GraphedVSR(vsr_copy), torch.zeros((3, 8, 8, 3))
    assert _keys(vsr_copy, g, data) == _keys(vsr_copy, g, data)
    with torch.no_grad():
        vsr_copy.model.conv_out[0].weight.sum()       # reading a weight is no change
    assert _keys(vsr_copy, g, data) == _keys(vsr_copy, g, data)


@pytest.mark.parametrize("kind", CPU_KINDS)
def test_each_mutation_of_one_sr_tensor_moves_the_sr_key_and_the_graph_key_only(vsr_copy, kind):
    g, data = GraphedVSR(vsr_copy), torch.zeros((3, 8, 8, 3))
    k0 = _keys(vsr_copy, g, data)
    C.mutations[kind](vsr_copy.model, ["block.downBlocks.2.0.weight"])
    k1 = _keys(vsr_copy, g, data)
    assert k1["sr"] != k0["sr"] and k1["graph"] != k0["graph"]
    assert all(k1[t] == k0[t] for t in ("flow", "depth", "vos"))
    assert _keys(vsr_copy, g, data) == k1


@pytest.mark.parametrize("kind", [k for k in CPU_KINDS if k not in C.OPTIMIZER_KINDS])
@pytest.mark.parametrize("trunk", ["flow", "depth", "vos"])
def test_each_mutation_of_one_trunk_tensor_moves_that_trunks_key_and_the_graph_key(vsr_copy, trunk, kind):
    g, data = GraphedVSR(vsr_copy), torch.zeros((3, 8, 8, 3))
    cache = {"flow": vsr_copy._flow_exec, "depth": vsr_copy._depth_exec, "vos": vsr_copy._vos_exec}[trunk]
    names = [C.mid_tensor(cache.master, 4)] + ([C.mid_tensor(cache.master, 1)] if trunk == "depth" else [])    # (the hourglass: a buffer too)
    for name in names:
        k0 = _keys(vsr_copy, g, data)
        C.mutations[kind](cache.master, [name])
        k1 = _keys(vsr_copy, g, data)
        assert k1[trunk] != k0[trunk] and k1["graph"] != k0["graph"], name
        assert all(k1[t] == k0[t] for t in k0 if t not in (trunk, "graph")), name


@pytest.mark.parametrize("kind", CPU_KINDS)
def test_each_mutation_moves_the_per_layer_keys_of_the_float32_trunk(kind):
    """trunk_f32._Packed (the packed weight of one layer) and _Folded (bias + eval-mode BatchNorm as scale / shift): rebuilt after each
    mutation of a tensor they read, kept otherwise; the folded values are those of the new tensors."""
    net = nn.Sequential(trunk_f32.Conv2dF32(3, 4, 3), nn.BatchNorm2d(4)).eval()
    with torch.no_grad():
        net[1].running_var.uniform_(0.5, 2.0)
        net[1].running_mean.normal_()
    packed, folded, built = trunk_f32._Packed(), trunk_f32._Folded(), []
    make = lambda: built.append(1) or object()
    a = packed.get(net[0].weight, make)
    assert packed.get(net[0].weight, make) is a and len(built) == 1
    f = folded.get(net[0], net[1])
    assert folded.get(net[0], net[1]) is f
    C.mutations[kind](net, ["0.weight"])
    b = packed.get(net[0].weight, make)
    assert b is not a and len(built) == 2 and packed.get(net[0].weight, make) is b
    touched = ["0.bias", "1.weight", "1.bias"] + ([] if kind in C.OPTIMIZER_KINDS else ["1.running_mean", "1.running_var"])
    for name in touched:
        old = folded.get(net[0], net[1])
        C.mutations[kind](net, [name])
        new = folded.get(net[0], net[1])
        assert new is not old and folded.get(net[0], net[1]) is new, name
        scale = net[1].weight / torch.sqrt(net[1].running_var + net[1].eps)
        shift = net[1].bias + (net[0].bias - net[1].running_mean) * scale
        assert torch.allclose(new[0], scale.detach(), rtol=1e-6, atol=0) and torch.allclose(new[1], shift.detach(), rtol=1e-5, atol=1e-7), name
    if kind != "load_state_dict" and kind != "load_state_dict_assign":     # (those two touch every tensor of the module)
        assert packed.get(net[0].weight, make) is b and len(built) == 2


def test_executor_cache_rebuilds_once_per_mutation():
    net = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Sequential(nn.Conv2d(4, 2, 1, bias=False)))
    built = []
    cache = TrunkExecCache(net, lambda m: built.append(1) or object())
    last = cache.get()
    for i, kind in enumerate(CPU_KINDS):
        C.mutations[kind](net, ["2.0.weight"])
        new = cache.get()
        assert new is not last and cache.get() is new and len(built) == i + 2, kind
        last = new


# ---------------------------------------------------------------------------------------------------------------- mark_updated
def test_mark_updated_moves_the_version_of_a_leaf_that_requires_grad_and_no_value():
    p = nn.Parameter(torch.arange(6, dtype=torch.float32).reshape(2, 3))
    p.grad = torch.ones_like(p)
    m, v = torch.zeros(2, 3), torch.ones(2, 3)
    other = nn.Parameter(torch.ones(2))
    before = [t._version for t in (p, m, v, other, p.grad)]
    values = [t.detach().clone() for t in (p, m, v)]
    with torch.no_grad():
        optim.mark_updated(t for t in (p, m, v))        # (a generator, as step() passes it)
    optim.mark_updated([p])                             # ... and with autograd on, as a caller outside step() may
    after = [t._version for t in (p, m, v, other, p.grad)]
    assert all(a != b for a, b in zip(after[:3], before[:3])) and after[3:] == before[3:]
    assert all(torch.equal(t.detach(), old) for t, old in zip((p, m, v), values))
    assert p.requires_grad and p.is_leaf and p.grad is not None and torch.equal(p.grad, torch.ones_like(p))
    optim.mark_updated([])
