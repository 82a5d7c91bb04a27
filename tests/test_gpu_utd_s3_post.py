"""k_utd_s3_post (csrc/sr_utd_s3.h with POST, csrc/sr_utd_s3p.hip, libvsr_hip_s3p.so): the fused x3 FeedbackBlock stage that also applies
the NEXT group's uptran slice (1x1 + PReLU) to its finished output rows

  * against the two launches it replaces -- vsr_s3_sr_utd_f16, then the one-stage 1x1 chain launch on its output -- bit for bit on
    BOTH tensors, over strip edges, one-row segments (every row is then a segment's last row) and plane counts,
  * with uptran slopes above 1 and below 0 (select build) and a stage slope above 1 beside a post slope below,
  * in exact arithmetic (tests/_exact.py) against a float64 evaluation, with one planted unit in one weight of the fused 1x1,
  * on poisoned, guard-banded buffers (tests/_poison.py),
  * inside SRProjectionModule(upscale_factor=3) and VSR(upscale_factor=3): `fuse_uptran` on == off, with a count of the launches
    that proves the new entry ran and the chain launch between the two stages of a step is gone.

Every comparison is an equality (the one fixture comparison uses the bar tests/test_gpu_sr_scale3.py applies to the same fixture)."""
import numpy as np
import pytest
import torch

import _exact as E

pytestmark = pytest.mark.gpu

from _poison import poisoned  # noqa: E402
from test_gpu_exact_sr import gen_stage, module  # noqa: E402
from test_gpu_poisoned_buffers import _sr_inputs, run_poisoned  # noqa: E402
from test_gpu_sr_scale3 import _stage_input, rel, sr3  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402


def sr3p(**attrs):
    """A fresh x3 module (seeded weights, fp16, fused stage: it packs the POST build beside the plain one); `attrs` set further switches."""
    m = sr3()
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _nan(N, h, w):
    return torch.full((N, h, w, 32), float("nan"), dtype=torch.float16, device="cuda")


def _launch_post(sp, a, rps, le1):
    N, h, w, _ = a.shape
    out, post = _nan(N, h, w), _nan(N, h, w)
    lib = L.load_s3p()
    L.check(lib.vsr_s3p_sr_utd_post_f16(L.dptr(a, torch.float16), L.dptr(sp.blob, torch.uint8), L.dptr(out, torch.float16), L.dptr(post, torch.float16),
                                        N, h, w, rps, int(le1), L.stream()), "sr_utd_s3_post_f16", lib=lib)
    return out, post


def _two_launches(m, a):
    """What the POST entry replaces: the plain stage's launch, then `m._chain([ut(3)])` on its output (sr.py:_forward_f16)."""
    N, h, w, _ = a.shape
    P = m._packed()
    st = P["stage"][0]
    assert type(st).__name__ == "_FusedStageS3" and not st.has_post
    out = _nan(N, h, w)
    lib = L.load_s3()
    L.check(lib.vsr_s3_sr_utd_f16(L.dptr(a, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, 0, int(st.slopes_le_one), L.stream()),
            "sr_utd_s3_f16", lib=lib)
    post = _nan(N, h, w).view(N, h * w, 32)
    m._chain([dict(ins=[(out.view(N, h * w, 32), P["ut_w"][3], 32 * 4)], bias=P["ut_b"][3], slope=P["ut_a"][3])], N, h * w, keep=[True], outs=[post])
    return out, post.view(N, h, w, 32)


def _stage_post(m):
    P = m._packed()
    assert sorted(P["stage_post"]) == [0], "six groups: the first stage of a step is the one another stage follows"
    sp = P["stage_post"][0]
    assert type(sp).__name__ == "_FusedStageS3Post" and sp.has_post
    assert torch.equal(sp.blob[:P["stage"][0].blob.numel()], P["stage"][0].blob)
    return sp


# widths 1, 7, 29, 30, 31 (a strip holds 30 columns), 61 and 95; heights 1, 2, 3 and 35; N 1, 2, 5
SHAPES = [(1, 1, 1), (2, 2, 7), (1, 3, 29), (5, 1, 30), (2, 3, 31), (1, 2, 61), (2, 35, 95), (5, 3, 7), (1, 35, 31)]


@pytest.mark.parametrize("shape", SHAPES)
def test_post_entry_equals_the_two_launches_it_replaces(shape):
    N, h, w = shape
    m = sr3p()
    sp = _stage_post(m)
    a = _stage_input(N, h, w, N * 1000 + h * 10 + w)
    with torch.no_grad():
        want_out, want_post = _two_launches(m, a)
        assert torch.isfinite(want_out.float()).all() and torch.isfinite(want_post.float()).all()
        assert sp.post_slopes_le_one and m._packed()["slopes_le_one"]
        # row segmentations: 1 (every row is a segment's last row), 3, 16, one march (0); max and select build
        for rps in (1, 3, 16, 0):
            for le1 in (1, 0):
                out, post = _launch_post(sp, a, rps, le1)
                assert torch.equal(out, want_out), (rps, le1)
                assert torch.equal(post, want_post), (rps, le1)
        # the wrapper's own choice of segments, fresh outputs and a caller's destination
        out, post = sp(a, m._chain)
        assert torch.equal(out, want_out) and torch.equal(post, want_post)
        dst = _nan(N, h, w)
        out2, post2 = sp(a, m._chain, out=dst)
        assert out2 is dst and torch.equal(dst, want_out) and torch.equal(post2, want_post)
        # the planes of a launch are independent: N planes at once == N launches of one plane
        if N > 1:
            ones = [_launch_post(sp, a[i:i + 1].contiguous(), 0, 1) for i in range(N)]
            assert torch.equal(torch.cat([o for o, _ in ones]), want_out) and torch.equal(torch.cat([p for _, p in ones]), want_post)


@pytest.mark.parametrize("slopes", [((0.25, 0.25, 0.25), 1.5), ((0.25, 0.25, 0.25), -0.5), ((0.25, 0.25, 3.0), 0.25), ((1.5, -0.5, 0.25), 0.5),
                                    ((0.25, 2.0, 0.25), 2.5)])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 33, 31)])
def test_post_entry_slopes_of_any_sign_and_size(shape, slopes):
    """The uptran slope at 1.5 and at -0.5 (select build: `post_slopes_le_one` false for 1.5), a stage slope above 1 beside a post
    slope <= 1, and both above 1: set on the module before packing, compared with the two launches bit for bit."""
    stage_slopes, post_slope = slopes
    N, h, w = shape
    m = sr3p()
    b = m.block
    with torch.no_grad():
        b.upBlocks[1][1].weight.fill_(stage_slopes[0])
        b.downtranBlocks[1][1].weight.fill_(stage_slopes[1])
        b.downBlocks[2][1].weight.fill_(stage_slopes[2])
        b.uptranBlocks[3][1].weight.fill_(post_slope)
    P = m._packed()
    sp = _stage_post(m)
    assert P["slopes_le_one"] == all(s <= 1.0 for s in stage_slopes)
    assert sp.post_slopes_le_one == (P["slopes_le_one"] and post_slope <= 1.0)
    a = _stage_input(N, h, w, h * 7 + w)
    with torch.no_grad():
        want_out, want_post = _two_launches(m, a)
        neg = (want_out.float() < 0).float().mean().item()
        assert 0.05 < neg < 0.95            # both sides of the post PReLU's input are exercised
        out, post = _launch_post(sp, a, 4, 0)
        assert torch.equal(out, want_out) and torch.equal(post, want_post)
        out, post = sp(a, m._chain)         # (the wrapper passes the module's own post_slopes_le_one)
        assert torch.equal(out, want_out) and torch.equal(post, want_post)


# ---------------------------------------------------------------------------------------------------------------- exact arithmetic
@pytest.mark.parametrize("profile", ["up", "dt", "dn"])
@pytest.mark.parametrize("shape", [(1, 1, 29), (1, 2, 30), (2, 37, 31), (2, 5, 61), (1, 1, 1)])
def test_post_entry_equals_float64(shape, profile):
    """Operands inside the budget tests/_exact.py checks: both outputs equal the float64 evaluation bit for bit, over whole marches,
    segments and one-row segments."""
    N, h, w = shape
    c, ref = gen_stage(N * 1000 + h * 10 + w + 3, 3, shape, profile=profile)
    a = E.nhwc(c["a"]).cuda()
    m = module(3, c)
    sp = _stage_post(m)
    what = f"x3 POST {shape} {profile}"
    out, post = sp(a, m._chain)
    E.assert_exact(E.nchw64(out), ref["out"], what + " out (wrapper)")
    E.assert_exact(E.nchw64(post), ref["post"], what + " post (wrapper)")
    for rps in (0, 16, 3, 1):
        for le1 in (1, 0):
            out, post = _launch_post(sp, a, rps, le1)
            E.assert_exact(E.nchw64(out), ref["out"], f"{what} out rps {rps} le1 {le1}")
            E.assert_exact(E.nchw64(post), ref["post"], f"{what} post rps {rps} le1 {le1}")


@pytest.mark.parametrize("post_slope", [2.0, -0.5])
def test_post_entry_select_build_equals_float64(post_slope):
    shape = (2, 9, 33)
    c, ref = gen_stage(300 + int(post_slope * 8), 3, shape, profile="dt", post_slope=post_slope)
    a = E.nhwc(c["a"]).cuda()
    m = module(3, c)
    sp = _stage_post(m)
    assert not sp.post_slopes_le_one if post_slope > 1 else sp.post_slopes_le_one
    out, post = sp(a, m._chain)
    E.assert_exact(E.nchw64(out), ref["out"], f"x3 POST slope {post_slope} out")
    E.assert_exact(E.nchw64(post), ref["post"], f"x3 POST slope {post_slope} post")
    out, post = _launch_post(sp, a, 2, 0)
    E.assert_exact(E.nchw64(post), ref["post"], f"x3 POST slope {post_slope} post (select build)")


@pytest.mark.parametrize("idx", [(0, 0), (31, 31), (17, 8), (5, 23)])      # (out channel, in channel): both A fragments, all four lane groups
def test_one_unit_in_one_weight_of_the_fused_1x1_is_seen_with_its_footprint(idx):
    """The kernel's uptran weights differ from the reference's by ONE unit in ONE element: the second output differs exactly where a
    float64 evaluation of the changed weight differs (one out-channel, the pixels whose input channel is non-zero), the first output
    not at all."""
    shape = (2, 7, 33)
    c, ref = gen_stage(30, 3, shape, slopes=(1.0, 1.0, 1.0), profile="dt", post_slope=1.0)   # (slopes 1: nothing is clipped away)
    c2 = dict(c)
    c2["post_w"] = c["post_w"].clone()
    c2["post_w"][idx] += 1.0
    p0 = E.conv_ref(ref["out"], c2["post_w"].reshape(32, 32, 1, 1), c["post_b"], what="planted POST 1x1", store=torch.float16)
    planted = E.check_storable(E.prelu_ref(p0, 1.0), torch.float16, "planted POST after PReLU")
    pred = planted != ref["post"]
    only = torch.zeros_like(pred)
    only[:, idx[0]] = True
    assert pred.any() and not (pred & ~only).any()
    assert torch.equal(pred[:, idx[0]], ref["out"][:, idx[1]] != 0)
    a = E.nhwc(c["a"]).cuda()
    m = module(3, c2)
    out, post = _stage_post(m)(a, m._chain)
    E.assert_exact(E.nchw64(out), ref["out"], f"planted post_w{idx}: the first output is untouched")
    got = E.nchw64(post)
    E.assert_exact(got, planted, f"planted post_w{idx}: the kernel follows its own weights")
    with pytest.raises(AssertionError, match="differ from the float64 evaluation"):
        E.assert_exact(got, ref["post"], "planted")
    assert torch.equal(E.diff_mask(got, ref["post"]), pred)


# ---------------------------------------------------------------------------------------------------------------- poisoned buffers
def test_post_entry_poisoned_outputs_are_fully_written_and_bands_intact():
    """The launch itself on arena buffers with a ragged strip and a ragged segment: every element of both outputs written, no byte
    outside either; then a caller's `out=` destination written in place through the wrapper."""
    m = sr3p()
    sp = _stage_post(m)
    a = _stage_input(2, 11, 37, 5)
    with torch.no_grad():
        want_out, want_post = _two_launches(m, a)
    with poisoned() as arena:
        out = torch.empty((2, 11, 37, 32), dtype=torch.float16, device="cuda")
        post = torch.empty((2, 11, 37, 32), dtype=torch.float16, device="cuda")
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(post).all())
        lib = L.load_s3p()
        L.check(lib.vsr_s3p_sr_utd_post_f16(L.dptr(a, torch.float16), L.dptr(sp.blob, torch.uint8), L.dptr(out, torch.float16), L.dptr(post, torch.float16),
                                            2, 11, 37, 4, 1, L.stream()), "sr_utd_s3_post_f16", lib=lib)
        torch.cuda.synchronize()
        arena.assert_written(out, "out")
        arena.assert_written(post, "out_post")
        assert torch.equal(out, want_out) and torch.equal(post, want_post)
        arena.check()
        dst = torch.empty((2, 11, 37, 32), dtype=torch.float16, device="cuda")
        o, p = sp(a, m._chain, out=dst)
        torch.cuda.synchronize()
        assert o is dst
        arena.assert_written(dst, "out=")
        arena.assert_written(p, "out_post of the wrapper")
        assert torch.equal(dst, want_out) and torch.equal(p, want_post)
        arena.check()


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 9, 40), (3, 37, 33)])
def test_post_stage_on_poisoned_buffers(shape):
    N, h, w = shape
    a, b = _stage_input(N, h, w, 11 + h), _stage_input(N, h, w, 12 + w)

    def call(m, x):
        with torch.no_grad():
            return list(_stage_post(m)(x, m._chain))
    run_poisoned(sr3p, call, (a,), (b,), what=f"x3 POST stage {shape}")


@pytest.mark.parametrize("hw", [(9, 40), (37, 33)])
def test_x3_network_with_post_on_poisoned_buffers(hw):
    rs = np.random.RandomState(hw[0] * 31 + hw[1])

    def call(m, x, _):
        assert m.fuse_uptran
        with torch.no_grad():
            (full, dec), n = _counted(lambda: [m(x), m(x, decimate=True)])
        assert n["post"] == 2 * m.num_steps
        return [full, dec]
    run_poisoned(sr3p, call, _sr_inputs(rs, *hw), _sr_inputs(rs, *hw), what=f"x3 SR net with POST {hw}")


# ---------------------------------------------------------------------------------------------------------------- module level
def _counted(fn):
    """fn() with the launch timer on -> (result, counts): `post` = launches of the new entry, `plain` = of the plain x3 stage, `chain1` =
    one-stage 1x1 chain launches (what the POST build replaces between the two stages of a step), `p1` / `p2` = stage launches of either
    build on one / two planes."""
    old = (L.TIMER.enabled, L.TIMER.only)
    L.TIMER.reset()
    L.TIMER.enabled, L.TIMER.only = True, None
    try:
        r = fn()
        torch.cuda.synchronize()
        s = L.TIMER.summary()
    finally:
        L.TIMER.enabled, L.TIMER.only = old
        L.TIMER.reset()
    return r, dict(post=sum(v[0] for k, v in s.items() if k.startswith("sr_utd_s3_post_f16")),
                   plain=sum(v[0] for k, v in s.items() if k.startswith("sr_utd_s3_f16")),
                   chain1=s.get("sr_chain1x1_f16 x1", (0, 0.0))[0],
                   p1=sum(v[0] for k, v in s.items() if k.startswith("sr_utd_s3") and "_p1" in k),     # stage launches on ONE plane / on TWO planes:
                   p2=sum(v[0] for k, v in s.items() if k.startswith("sr_utd_s3") and "_p2" in k))     # only `precompute_rows` issues them in a forward


def _on_off(run, steps_on, make=sr3p):
    """run(m) with fuse_uptran on and off on fresh modules: equal results; the new entry ran `steps_on` times, the plain stage that many
    times less and the one-stage chain launch that many times less (one per step) -- a silent fall-back fails here."""
    m_on, m_off = make(fuse_uptran=True), make(fuse_uptran=False)
    with torch.no_grad():
        r_on, n_on = _counted(lambda: run(m_on))
        r_off, n_off = _counted(lambda: run(m_off))
    assert n_off["post"] == 0 and n_on["post"] == steps_on > 0, (n_on, n_off)
    assert n_on["chain1"] == n_off["chain1"] - steps_on, (n_on, n_off)
    assert n_on["plain"] == n_off["plain"] - steps_on, (n_on, n_off)
    assert len(r_on) == len(r_off)
    for i, (a, b) in enumerate(zip(r_on, r_off)):
        assert a.shape == b.shape and torch.isfinite(a).all()
        assert torch.equal(a, b), i
    return r_on


def _frames(seed, hw):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (8, 3) + tuple(hw)).astype(np.float32)).cuda()


@pytest.mark.parametrize("hw", [(9, 33), (37, 45), (1, 7)])
def test_module_fuse_uptran_on_equals_off_full_and_decimated(hw):
    x = _frames(hw[0] * 3 + hw[1], hw)
    steps = sr3p().num_steps
    full, dec = _on_off(lambda m: [m(x), m(x, decimate=True)], 2 * steps)
    assert torch.equal(dec, full[..., ::3, ::3])


@pytest.mark.parametrize("ahead", ["kept", "precompute_shared", "precompute_rows"])
@pytest.mark.parametrize("hw", [(9, 40), (37, 33)])
def test_module_fuse_uptran_on_equals_off_with_shared_planes(hw, ahead):
    """Two calls that share their first three planes: kept by the first call, evaluated ahead by `precompute_shared` (with the
    pre-fusion planes), and with plane 7 ahead as well (`precompute_rows`): each goes through the stage loop with a destination."""
    h, w = hw
    x = _frames(h * 17 + w, hw)
    x2 = x.clone()
    x2[3:] = _frames(h * 17 + w + 1, hw)[3:]
    steps = sr3p().num_steps

    def run(m):
        shared = {"n": 3}
        if ahead != "kept":
            live = {k: torch.empty((8, h * w, 32), dtype=torch.float16, device="cuda") for k in (3, 6)}
            live["prefc"] = torch.empty((8, 3, 3 * h, 3 * w), dtype=torch.float32, device="cuda")
            m.precompute_shared(x[:3].contiguous(), shared, live)
        if ahead == "precompute_rows":
            m.precompute_rows(x[7:8].contiguous(), live, 7)
            shared["todo"] = (3, 7)
        first = m(x, decimate=True, shared=shared)
        shared.pop("todo", None)
        return [first, m(x2, shared=shared)]
    r = _on_off(run, {"kept": 2, "precompute_shared": 3, "precompute_rows": 4}[ahead] * steps)
    with torch.no_grad():      # ... and equal to the calls that share nothing
        plain = sr3p()
        assert torch.equal(r[0], plain(x, decimate=True)) and torch.equal(r[1], plain(x2))


def test_module_fuse_uptran_on_equals_off_with_an_uptran_slope_above_one():
    x = _frames(77, (12, 35))

    def make(**attrs):
        m = sr3p(**attrs)
        with torch.no_grad():
            m.block.uptranBlocks[3][1].weight.fill_(1.75)
        return m
    steps = sr3p().num_steps
    _on_off(lambda m: [m(x)], steps, make=make)
    m = make()
    assert m._packed()["slopes_le_one"] and not m._packed()["stage_post"][0].post_slopes_le_one


def test_module_taps_are_what_they_were():
    """The `taps` path (intermediate maps for the parity tests) with the POST build equals the one without."""
    x = _frames(5, (6, 10))
    ta, tb = {}, {}
    with torch.no_grad():
        a = sr3p(fuse_uptran=True)(x, taps=ta)
        b = sr3p(fuse_uptran=False)(x, taps=tb)
    assert torch.equal(a, b) and sorted(ta) == sorted(tb) and len(ta) > 3
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k


def test_module_fixture_with_post(golden):
    g = golden("g8_sr_x3_6x10")
    x = torch.from_numpy(g["x"]).cuda()
    m = sr3p()
    with torch.no_grad():
        (out,), n = _counted(lambda: [m(x)])
    assert n["post"] == m.num_steps and n["plain"] == m.num_steps
    assert rel(out, g["out"]) < 2e-3          # (the bar of tests/test_gpu_sr_scale3.py::test_fused_and_unfused_x3_networks_agree)


# ---------------------------------------------------------------------------------------------------------------- VSR.forward
def _vsr(cpu_vsr, scale=3, **sr_attrs):
    from video_super_resolution_amd import VSR
    m = VSR(upscale_factor=scale).eval()
    m.load_state_dict({k: v for k, v in cpu_vsr.state_dict().items() if not k.startswith("model.")}, strict=False)
    fill_module_(m.model, seed=0, prefix="model.")
    m = m.cuda()
    m.precision = m.model.precision = "fp16"
    for k, v in sr_attrs.items():
        setattr(m.model, k, v)
    return m


def _two_calls(m, data, S):
    h, w = data.shape[1:3]
    hf = torch.zeros(3, S * h, S * w, 3, device="cuda")
    outs = []
    with torch.no_grad():
        for k in range(2):   # estimated_image = None, then the recurrent call
            out, loss = m(data, None, hf, None if k == 0 else outs[0], train=False)
            assert loss is None and torch.isfinite(out).all()
            outs.append(out.clone())
    return outs


def test_vsr_forward_x3_fuse_uptran_on_equals_off(cpu_vsr):
    data = torch.from_numpy(np.random.RandomState(33).randint(0, 256, (3, 66, 70, 3)).astype(np.float32)).cuda()
    (on, n_on) = _counted(lambda: _two_calls(_vsr(cpu_vsr, fuse_uptran=True), data, 3))
    (off, n_off) = _counted(lambda: _two_calls(_vsr(cpu_vsr, fuse_uptran=False), data, 3))
    assert n_on["post"] > 0 and n_off["post"] == 0
    assert n_on["chain1"] == n_off["chain1"] - n_on["post"] and n_on["plain"] == n_off["plain"] - n_on["post"], (n_on, n_off)
    for a, b in zip(on, off):
        assert a.shape == (1, 198, 210, 3) and torch.equal(a, b)


@pytest.mark.parametrize("level", [1, 2, 3])
def test_vsr_forward_x3_early_planes_on_a_fresh_model(cpu_vsr, level):
    """early_scales = (4, 3) against (4,) at early_planes 1, 2, 3, each on a FRESH model: level 3 evaluates planes on the main stream while
    the packed weights and constant maps of the first call are still being produced on the side stream."""
    data = torch.from_numpy(np.random.RandomState(34).randint(0, 256, (3, 66, 70, 3)).astype(np.float32)).cuda()
    ref = _vsr(cpu_vsr)
    ref.early_scales, ref.early_planes = (4,), level
    want, n_ref = _counted(lambda: _two_calls(ref, data, 3))
    m = _vsr(cpu_vsr)
    m.early_scales, m.early_planes = (4, 3), level
    got, n = _counted(lambda: _two_calls(m, data, 3))
    assert n["post"] > 0 and n_ref["post"] > 0
    # the early route was taken at x3 and only there.  Plane 7 of either pass goes through the stages alone: two stage launches x steps x
    # two passes x two calls.  From level 2 on the two depth planes of pass 2 go ahead as a pair and pass 2's own call is left with the
    # other pair (planes 3, 4): two pairs per forward; at level 3 the same in pass 1 (the flow-picture planes ahead, the depth planes in
    # the call): four pairs.  With early_scales = (4,) a forward launches the stages on 3 and on 5 planes only.
    steps = m.model.num_steps
    assert n_ref["p1"] == 0 and n_ref["p2"] == 0, n_ref
    assert n["p1"] == 2 * steps * 2 * 2, n
    assert n["p2"] == 2 * steps * 2 * {1: 0, 2: 2, 3: 4}[level], n
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("scale", [4, 2])
def test_x4_and_x2_forwards_do_not_load_the_post_library(scale):
    """A fresh interpreter (this one has loaded the library long ago): VSR.forward at x4 / x2 and nothing of libvsr_hip_s3p.so."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import os, sys
os.environ.setdefault('MIOPEN_FIND_MODE', '2'); os.environ.setdefault('MIOPEN_LOG_LEVEL', '2')
sys.path.insert(0, {root!r})
import numpy as np, torch
from video_super_resolution_amd import VSR, _lib
from video_super_resolution_amd.weights import fill_module_
m = fill_module_(VSR(upscale_factor={scale}).eval(), 0).cuda()
m.precision = m.model.precision = 'fp16'
data = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (3, 66, 70, 3)).astype(np.float32)).cuda()
with torch.no_grad():
    out, _ = m(data, None, None, None, train=False)
    out, _ = m(data, None, None, out, train=False)
torch.cuda.synchronize()
assert torch.isfinite(out).all()
assert _lib._s3plib is None, "an x{scale} forward loaded libvsr_hip_s3p.so"
assert 'libvsr_hip_s3p' not in open('/proc/self/maps').read()
print('ok')
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
