"""Updated weights reach every packed copy the inference kernels read.

No inference kernel reads an `nn.Parameter`: each reads a copy packed for it and cached under the (address, version) of the tensors --
the SR net's `_packed()` dictionary (blobs, fragments, PReLU slopes as Python floats, the constant maps), the `shared` maps of two SR
calls, the trunk executors of `VSR`, of loss.py and of `frames.truth_flows`, trunk_f32's per-layer `_Packed` / `_Folded`, the graphs
of `GraphedVSR`, and `VSR.temporal_cache`'s depth maps and flow pictures.  Here a weight is changed in every way a weight changes
(tests/_fresh_cases.py `mutations`, the raw-pointer step of optim.Adam among them) after the copies were built, and the next call is held to

    a FRESH module: a new object, `load_state_dict` of the changed state, its first forward -- `torch.equal`, no tolerance
    (the same kernels on the same weights; tests/test_gpu_tail_s3.py and tests/test_gpu_yuv.py rely on the same),

and must differ from the call before the change, or the case would prove nothing.  Which tensors of the SR net can move its output
at all is found on the CPU restatement by `_fresh_cases.live_tensors` (83 of 91; tests/test_fresh_cases_helper.py pins them); the
sweep below takes every one of them."""
import copy
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _fresh_cases as C  # noqa: E402
from video_super_resolution_amd import GraphedVSR, driver, optim  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- the SR net
def sr_module(scale, precision, **switches):
    m = copy.deepcopy(C.sr_master(scale)).cuda().eval()
    m.precision = precision
    for k, v in switches.items():
        setattr(m, k, v)
    return m


def fwd(m, x, **kw):
    with torch.no_grad():
        return m(x, **kw).clone()


def check_fresh(m, x, before, what, **kw):
    """The call after a change: equal to a fresh module's first call, finite, not the frame of before the change.  -> the frame."""
    got = fwd(m, x, **kw)
    want = fwd(C.fresh_sr(m), x)
    assert bool(torch.isfinite(got).all()), what
    assert torch.equal(got, want), (what, "stale: max |got - fresh| =", float((got - want).abs().max()))
    assert not torch.equal(got, before), (what, "the frame did not move with the weights")
    return got


N_CHUNKS = 12   # of the per-tensor sweep: tensors chunk, chunk + 12, ... of the live set (seven each, six in the last)


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_sr_x4_fp16_every_live_tensor_in_turn(chunk):
    """The headline configuration at [8,3,7,9]: the first forward builds the pack; then every live tensor of this chunk in turn is
    changed in place (the changes add up inside a chunk) and the next forward is held to a fresh module."""
    live = C.live_tensors(C.sr_master(4))
    chunks = [live[c::N_CHUNKS] for c in range(N_CHUNKS)]
    assert len(live) == 83 and sorted(n for c in chunks for n in c) == sorted(live)      # no live tensor is left out
    m = sr_module(4, "fp16")
    x = C.sr_input().cuda()
    prev = fwd(m, x)
    assert m._pack is not None and "utd4" in m._pack
    for name in chunks[chunk]:
        C.mutations["in_place"](m, [name])
        prev = check_fresh(m, x, prev, name)


CONFIGS = {   # scale, precision, switches, input size
    "x4_fp32": (4, "fp32", {}, C.HW),
    "x2_fp16": (2, "fp16", {}, C.HW_WIDE),                    # fused stage (k_utd_s2 with the uptran slice) and one-launch tail
    "x2_fp32": (2, "fp32", {}, C.HW),
    "x3_fp16_post": (3, "fp16", dict(fuse_uptran=True, fold_chain=False, fused_tail_s3=True), C.HW_WIDE),
    "x3_fp16_fold_chain": (3, "fp16", dict(fuse_uptran=True, fold_chain=True, fused_tail_s3=True), C.HW_WIDE),
    "x3_fp32": (3, "fp32", {}, C.HW),
}


@pytest.mark.parametrize("group", C.GROUP_NAMES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_sr_every_group_in_the_other_configurations(config, group):
    scale, precision, switches, hw = CONFIGS[config]
    names = C.groups(C.sr_master(scale))[group]
    m = sr_module(scale, precision, **switches)
    x = C.sr_input(hw).cuda()
    before = fwd(m, x)
    P = m._pack
    assert P is not None
    if config == "x2_fp16":
        assert "tail_s2" in P and P["stage"][0].has_post
    if config.startswith("x3_fp16"):
        assert "tail_s3" in P and 0 in P["stage_post"] and 0 in P["stage_pre"]
    C.mutations["in_place"](m, names)
    check_fresh(m, x, before, (config, group))
    assert m._pack is not P


@pytest.mark.parametrize("target", ["chain0", "conv_out"])
@pytest.mark.parametrize("kind", list(C.mutations))
@pytest.mark.parametrize("config", ["x4_fp16", "x2_fp16"])
def test_sr_every_way_a_weight_changes(config, kind, target):
    scale, hw = (4, C.HW) if config == "x4_fp16" else (2, C.HW_WIDE)
    names = C.groups(C.sr_master(scale))[target]
    m = sr_module(scale, "fp16")
    x = C.sr_input(hw).cuda()
    before = fwd(m, x)
    old = {n: t.detach().clone() for n, t in C.named_tensors(m).items()}
    C.mutations[kind](m, names)
    now = C.named_tensors(m)
    assert all(C.changed_everywhere(m, n, old[n], now[n]) if n in names else torch.equal(old[n], now[n]) for n in old)
    check_fresh(m, x, before, (config, kind, target))


# ---------------------------------------------------------------------------------------------------------------- the optimizer
@pytest.mark.parametrize("max_grad_norm", [None, 1.0], ids=["plain", "clipped"])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_sr_two_steps_of_optim_adam_each_reach_the_inference_kernels(gpu_vsr, precision, max_grad_norm):
    """optim.Adam.step() writes p, exp_avg and exp_avg_sq through raw pointers (vsr_opt_adam_f32); the no-grad forward after each of
    two steps must be the stepped weights'.  Before `optim.mark_updated` the versions stood still and this case failed at step 1 --
    the pack of before the step answered: 'stale: max |got - fresh| =' 7.12 (fp32), 7.11 (fp32, clipped), 7.28 (fp16), 7.28 (fp16, clipped)
    on frames up to 66."""
    m = copy.deepcopy(gpu_vsr.model)
    m.precision = precision
    x = torch.from_numpy(np.random.RandomState(51).randint(0, 256, (8, 3, 7, 9)).astype(np.float32)).cuda()
    prev = fwd(m.eval(), x)
    assert m._pack is not None
    params = list(m.parameters())
    opt = optim.Adam(params, lr=1e-3, max_grad_norm=max_grad_norm)
    for step in (1, 2):
        m.train()
        opt.zero_grad(set_to_none=True)
        (m(x) ** 2).mean().backward()
        versions = [(p._version, p.grad is None) for p in params]
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        opt.step()
        assert opt.launches == (1 if max_grad_norm is None else 3)
        prev = check_fresh(m.eval(), x, prev, f"step {step}")
        for p, (v, no_grad), g in zip(params, versions, grads):
            assert (p._version == v) == no_grad                          # a parameter without a gradient keeps its version
            assert g is None or torch.equal(p.grad, g)                   # .grad is read only


# ---------------------------------------------------------------------------------------------------------------- the `shared` maps
@pytest.mark.parametrize("how", ["first_call_f16", "precompute_f16", "precompute_f32"])
def test_shared_maps_do_not_outlive_the_weights(how):
    """A `shared` dict that outlives a weight change: `live` (the first call's or precompute_shared's), `prefc_all` (precompute_shared
    with a tail buffer) and `prefc_f32` (the float32 path) belong to the pack they were made under.  The call after the change
    evaluates every plane and refreshes them; the call after that reuses the refreshed maps."""
    m = sr_module(4, "fp32" if how == "precompute_f32" else "fp16")
    h = w = 16
    a = C.sr_input((h, w)).cuda()
    b, c = a.clone(), a.clone()
    b[3:], c[3:] = C.sr_input((h, w), seed=1).cuda()[3:], C.sr_input((h, w), seed=2).cuda()[3:]
    before = fwd(m, b)
    shared = {"n": 3}
    if how == "first_call_f16":
        fwd(m, a, shared=shared)
    elif how == "precompute_f16":
        live = {k: torch.empty((8, h * w, 32), dtype=torch.float16, device="cuda") for k in (3, 6)}
        live["prefc"] = torch.empty((8, 3, 4 * h, 4 * w), dtype=torch.float32, device="cuda")
        m.precompute_shared(a[:3].contiguous(), shared, live)
        assert shared.get("prefc_all") is live["prefc"]
    else:
        m.precompute_shared(a[:3].contiguous(), shared, None)
    kept = "prefc_f32" if how == "precompute_f32" else "live"
    key = "key_f32" if how == "precompute_f32" else "key"
    old_key, old_kept = shared[key], (shared[kept] if how == "precompute_f32" else shared[kept][3])
    assert old_key[0] == m._pack_key
    assert torch.equal(fwd(m, b, shared=shared), before)                  # (the kept maps serve the unchanged weights)
    C.mutations["in_place"](m, C.chain_group(C.sr_master(4)))
    got = check_fresh(m, b, before, (how, "the call after the change"), shared=shared)
    new_kept = shared[kept] if how == "precompute_f32" else shared[kept][3]
    assert shared[key] != old_key and shared[key][0] == m._pack_key and new_kept is not old_kept and new_kept.data_ptr() != old_kept.data_ptr()
    check_fresh(m, c, got, (how, "the call that reuses the refreshed maps"), shared=shared)
    assert "prefc_all" not in shared                                      # (it belonged to the maps that were replaced)


# ---------------------------------------------------------------------------------------------------------------- the whole model
H, W, S = 66, 70, 4


def window(n=3, seed=0):
    """[n,66,70,3] float32 frames: a smooth scene that moves (the flow and depth trunks see structure)."""
    from scipy.ndimage import gaussian_filter
    base = gaussian_filter(np.random.RandomState(60 + seed).uniform(0, 255, size=(H + 16, W + 32, 3)).astype(np.float32), sigma=(2, 2, 0))
    return torch.from_numpy(np.stack([np.floor(base[k:k + H, 2 * k:2 * k + W]) for k in range(n)]).astype(np.float32)).cuda()


def hr_frames(n, seed):
    return torch.from_numpy(np.random.RandomState(70 + seed).randint(0, 256, (n, S * H, S * W, 3)).astype(np.float32)).cuda()


@pytest.fixture
def vsr(request, gpu_vsr, gpu_vsr_f16):
    """A copy of the session's model in the precision the case names (a copy has executors, streams and caches of its own)."""
    return copy.deepcopy(gpu_vsr_f16 if request.param == "fp16" else gpu_vsr)


both = pytest.mark.parametrize("vsr", ["fp16", "fp32"], indirect=True)


def fresh_vsr(cpu_vsr, m):
    f = copy.deepcopy(cpu_vsr).cuda().eval()
    f.load_state_dict(m.state_dict())
    f.precision = f.model.precision = m.precision
    return f


def infer(m, data, est=None):
    with torch.no_grad():
        out, loss = m(data, None, None, est, train=False)
    assert loss is None
    return out.clone()


def check_fresh_vsr(cpu_vsr, m, data, before, what):
    got = infer(m, data)
    want = infer(fresh_vsr(cpu_vsr, m), data)
    assert bool(torch.isfinite(got).all()), what
    assert torch.equal(got, want), (what, "stale: max |got - fresh| =", float((got - want).abs().max()))
    assert not torch.equal(got, before), (what, "the frame did not move with the weights")
    return got


def adam_train_step(m, data):
    """main.py:206-210 with optim.Adam on the device: one driver.train_step; the model stays in training mode, as in driver.run_c1_train."""
    m.train()
    opt = optim.Adam(m.parameters(), lr=1e-3)
    opt.zero_grad()
    driver.train_step(m, opt, data, hr_frames(1, 0), hr_frames(3, 1), None)
    assert opt.launches == 1


@both
def test_vsr_inference_after_a_train_step_with_optim_adam(cpu_vsr, vsr):
    """driver.run_c1_train from its second step on: the no-grad windows after a step read the stepped SR net."""
    data = window()
    before = infer(vsr, data)
    adam_train_step(vsr, data)
    check_fresh_vsr(cpu_vsr, vsr, data, before, "after train_step")


def trunk_of(m, trunk):
    return {"flow": m.FlowModule.net, "depth": m.DepthModule.model.netG, "vos": m.VOSModule.net}[trunk]


@both
@pytest.mark.parametrize("trunk", ["flow", "depth", "vos"])
def test_vsr_a_weight_deep_inside_a_guidance_trunk(cpu_vsr, vsr, trunk):
    """The executors of the fp16 configuration (TrunkExecCache) and the per-layer packs of the float32 one (trunk_f32._Packed, and
    _Folded for the hourglass, whose BatchNorm running_var is changed as well there)."""
    data = window()
    before = infer(vsr, data)
    net = trunk_of(vsr, trunk)
    names = [C.mid_tensor(net, 4)] + ([C.mid_tensor(net, 1)] if trunk == "depth" and vsr.precision == "fp32" else [])
    C.mutations["in_place"](net, names)
    check_fresh_vsr(cpu_vsr, vsr, data, before, (trunk, names))


@both
def test_vsr_temporal_cache_does_not_serve_the_old_weights_maps(cpu_vsr, vsr):
    """Window t, a hourglass weight changes, window t + 1 on views of the same clip tensor: the depth maps of the two shared frames
    were computed under the old weights and must not be served.  Before the cache remembered the executors' keys the frame was 6.67
    away from the fresh model's (both precisions).

    The frame is held to a fresh model's in three ways: its first call on window t + 1 with the cache off, the same with the cache
    on, and -- the reference this case was asked for -- its streaming run over windows t and t + 1.  The third asks more than
    freshness: the fresh model serves window t + 1 from ITS cache, so the two agree only if a prediction does not depend on the batch
    it was computed in.  The fp16 launchers see to that (`_lib.route_batch`).  The float32 trunks choose by the batch they are given
    (trunk_f32._route, the stock operator): while float32 kept entries, the fresh model's streaming run was 2.838 of 255 away from
    this frame AND from its own cache-off run, with no stale copy involved.  The float32 configuration therefore keeps no entries
    (vsr.py) and every one of its windows is the per-window evaluation."""
    clip = window(4)
    before = infer(vsr, clip[1:4])
    vsr.temporal_cache = True
    infer(vsr, clip[0:3])
    kept = (3, 2) if vsr.precision == "fp16" else (0, 0)
    assert (len(vsr._tcache["depth"]), len(vsr._tcache["flow"])) == kept
    net = trunk_of(vsr, "depth")
    C.mutations["in_place"](net, [C.mid_tensor(net, 4)])
    got = infer(vsr, clip[1:4])
    assert not torch.equal(got, before)
    first = fresh_vsr(cpu_vsr, vsr)
    assert torch.equal(got, infer(first, clip[1:4]))            # a fresh model, cache off
    first.temporal_cache = True
    assert torch.equal(got, infer(first, clip[1:4]))            # ... and its first streaming call: the batches the emptied cache gives
    f = fresh_vsr(cpu_vsr, vsr)
    f.temporal_cache = True
    infer(f, clip[0:3])
    want = infer(f, clip[1:4])
    print(f"{vsr.precision}: max |got - fresh streaming run| = {float((got - want).abs().max())!r}")
    assert torch.equal(got, want), float((got - want).abs().max())


@both
def test_graph_replay_captures_afresh_after_an_optim_adam_step(cpu_vsr, vsr):
    """GraphedVSR._key holds (address, version) of every weight: after a train step with optim.Adam the next call captures a second graph
    and returns the stepped weights' frame (before optim.mark_updated: one graph, replayed with the weights of before the step)."""
    m = vsr
    data = window()
    g = GraphedVSR(m)
    before, _ = g(data, None, None, None, train=False)
    assert len(g._graphs) == 1 and torch.equal(before, infer(m, data))
    adam_train_step(m, data)
    m.eval()
    got, _ = g(data, None, None, None, train=False)
    assert len(g._graphs) == 2
    want = infer(fresh_vsr(cpu_vsr, m), data)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert not torch.equal(got, before)


@both
def test_truth_flows_after_a_flownet_weight_change(cpu_vsr, vsr):
    """frames.truth_flows keeps a FlowNet2 executor of its own per model (fp16) or runs the per-layer packs (fp32)."""
    from scipy.ndimage import gaussian_filter
    base = gaussian_filter(np.random.RandomState(80).uniform(0, 255, size=(132, 136, 3)).astype(np.float32), sigma=(2, 2, 0))
    a, b = (torch.from_numpy(np.floor(base[k:k + 128, 2 * k:2 * k + 128]).copy()).cuda() for k in (0, 2))

    def flows(m):   # (the fp16 maps are the executor's own buffers, read in place: copies)
        fw, bw, crop = driver.truth_flows(m, a, b)
        torch.cuda.synchronize()
        return fw.clone(), bw.clone(), crop
    before = flows(vsr)
    net = trunk_of(vsr, "flow")
    C.mutations["in_place"](net, [C.mid_tensor(net, 4)])
    got, want = flows(vsr), flows(fresh_vsr(cpu_vsr, vsr))
    assert got[2] == want[2] == (0, 0, 128, 128)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], before[0]) and not torch.equal(got[1], before[1])


@both
def test_load_checkpoint_into_a_model_that_has_run(cpu_vsr, vsr, tmp_path):
    data = window()
    before = infer(vsr, data)
    other = copy.deepcopy(C.sr_master(4))
    C.mutations["in_place"](other, C.chain_group(C.sr_master(4)) + ["conv_out.0.weight", "block.compress_in.1.weight"])
    path = driver.save_checkpoint(driver.checkpoint_state(types.SimpleNamespace(model=other), 3), False, str(tmp_path), "fresh")
    ckpt = driver.load_checkpoint(vsr, path, map_location="cuda")
    assert ckpt["epoch"] == 3 and all(torch.equal(v.cpu(), other.state_dict()[k]) for k, v in vsr.model.state_dict().items())
    check_fresh_vsr(cpu_vsr, vsr, data, before, "after load_checkpoint")


def test_loss_executors_after_a_vgg_weight_change(cpu_vsr, gpu_vsr_f16):
    """The fp16 configuration's loss runs VGG16 and OSVOS on executors of their own (loss.py): the `train=True` call after a change of a
    VGG weight returns the fresh model's loss."""
    m = copy.deepcopy(gpu_vsr_f16)
    data, y = window(), hr_frames(1, 0)

    def loss_of(model):
        with torch.no_grad():
            _, loss = model(data, y, hr_frames(3, 1), None)
        return loss.detach().cpu().clone()
    before = loss_of(m)
    for net in (m.SR_loss.loss_network, m.Flow_loss.SR_loss.loss_network):
        C.mutations["in_place"](net, [C.mid_tensor(net, 4)])
    got, want = loss_of(m), loss_of(fresh_vsr(cpu_vsr, m))
    assert bool(torch.isfinite(got)) and torch.equal(got, want) and not torch.equal(got, before), (float(before), float(got), float(want))
