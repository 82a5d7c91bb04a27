"""k_utd_s3_pre (csrc/sr_utd_s3.h with PRE, csrc/sr_utd_s3f.hip, libvsr_hip_s3f.so): the fused x3 FeedbackBlock stage with the 1x1
chain that opens a step -- compress_out -> compress_in -> first uptran slice (PRE3), at step 0 compress_in -> uptran slice (PRE2) --
folded into its LR load path

  * against the launches it replaces -- the chain launch `_forward_f16` issues, then vsr_s3p_sr_utd_post_f16 (or, without POST,
    vsr_s3_sr_utd_f16) on its output -- bit for bit on BOTH tensors, over strip edges and halos on the image border, one-row segments
    and plane counts, max and select builds, both modes,
  * with biases and a constant map that make the chain's value of zero operands large: the ring's padding pixels must hold zeros,
  * with slopes above 1 and below 0 in each of the three 1x1s,
  * in exact arithmetic (tests/_exact.py) against a float64 evaluation, with one planted unit in compress_out, in each half of
    compress_in and in the uptran slice,
  * on poisoned, guard-banded buffers (tests/_poison.py),
  * inside SRProjectionModule(upscale_factor=3), VSR(upscale_factor=3) and GraphedVSR: `fold_chain` on == off, with a count of the
    launches that proves the new entry ran and the step-opening chain launch is gone.

Every comparison is an equality (the one fixture comparison uses the bar tests/test_gpu_sr_scale3.py applies to the same fixture)."""
import numpy as np
import pytest
import torch

import _exact as E

pytestmark = pytest.mark.gpu

from _poison import poisoned  # noqa: E402
from test_gpu_exact_sr import module  # noqa: E402
from test_gpu_poisoned_buffers import _sr_inputs, run_poisoned  # noqa: E402
from test_gpu_sr_scale3 import rel, sr3  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd._lib import load_s3f  # noqa: E402  (absent without the feature: the module fails at import)
from video_super_resolution_amd.weights import fill_module_  # noqa: E402


def sr3f(**attrs):
    """A fresh x3 module (seeded weights, fp16, fused stage: it packs the PRE build beside the plain and the POST one)."""
    m = sr3()
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _nan(N, h, w):
    return torch.full((N, h, w, 32), float("nan"), dtype=torch.float16, device="cuda")


def _inputs(N, h, w, seed, scale=1.0):
    """feat, a, b [N,h,w,32] fp16 and the constant map [h w, 32] fp32."""
    rs = np.random.RandomState(seed)
    f, a, b = (torch.from_numpy((rs.randn(N, h, w, 32) * scale).astype(np.float16)).cuda() for _ in range(3))
    return f, a, b, torch.from_numpy((rs.randn(h * w, 32) * scale).astype(np.float32)).cuda()


def _stage_pre(m):
    P = m._packed()
    assert sorted(P["stage_pre"]) == [0], "six groups: the step's first stage"
    sp = P["stage_pre"][0]
    assert type(sp).__name__ == "_FusedStageS3Pre"
    assert torch.equal(sp.blob[:P["stage_post"][0].blob.numel()], P["stage_post"][0].blob)
    return sp


def _launch_pre(sp, ops, mode, rps, le1, post=True):
    feat, a, b, cmap = ops
    N, h, w, _ = feat.shape
    out, o2 = _nan(N, h, w), (_nan(N, h, w) if post else None)
    lib = load_s3f()
    p3 = mode == 3
    L.check(lib.vsr_s3f_sr_utd_pre_f16(L.dptr(feat, torch.float16), L.optr(a if p3 else None, torch.float16), L.optr(b if p3 else None, torch.float16),
                                       L.optr(cmap if p3 else None), L.dptr(sp.blob, torch.uint8), L.dptr(out, torch.float16), L.optr(o2, torch.float16),
                                       N, h, w, rps, int(le1), L.stream()), "sr_utd_s3_pre_f16", lib=lib)
    return out, o2


def _chain_launch(m, ops, mode):
    """The step-opening chain launch exactly as sr.py:_forward_f16 issues it without the fold -> the stage's input [N,h,w,32]."""
    feat, a, b, cmap = ops
    N, h, w, _ = feat.shape
    P, hp = m._packed(), h * w
    f, a, b = (t.view(N, hp, 32) for t in (feat, a, b))
    ut0 = dict(ins=[], prev=(P["ut_w"][0], 32), bias=P["ut_b"][0], slope=P["ut_a"][0])
    if mode == 3:
        co = dict(ins=[(a, P["co_w"], 64), (b, P["co_w"], 160)], bias=P["co_b"], slope=P["co_a"], cmap=cmap)
        ci = dict(ins=[(f, P["ci_w"], 0)], prev=(P["ci_w"], 32), bias=P["ci_b"], slope=P["ci_a"])
        x = m._chain([co, ci, ut0], N, hp, keep=[False, False, True])[-1]
    else:
        ci = dict(ins=[(f, P["ci_w"], 0), (f, P["ci_w"], 32)], bias=P["ci_b"], slope=P["ci_a"])
        x = m._chain([ci, ut0], N, hp, keep=[False, True])[-1]
    return x.view(N, h, w, 32)


def _replaced(m, ops, mode, post=True):
    """What the PRE entry replaces: the chain launch, then the POST stage's launch (post=False: the plain stage's) on its output."""
    x = _chain_launch(m, ops, mode)
    N, h, w, _ = x.shape
    P = m._packed()
    out = _nan(N, h, w)
    if post:
        o2 = _nan(N, h, w)
        sp, lib = P["stage_post"][0], L.load_s3p()
        L.check(lib.vsr_s3p_sr_utd_post_f16(L.dptr(x, torch.float16), L.dptr(sp.blob, torch.uint8), L.dptr(out, torch.float16), L.dptr(o2, torch.float16),
                                            N, h, w, 0, int(sp.post_slopes_le_one), L.stream()), "sr_utd_s3_post_f16", lib=lib)
        return out, o2
    st, lib = P["stage"][0], L.load_s3()
    L.check(lib.vsr_s3_sr_utd_f16(L.dptr(x, torch.float16), L.dptr(st.blob, torch.uint8), L.dptr(out, torch.float16), N, h, w, 0, int(st.slopes_le_one), L.stream()),
            "sr_utd_s3_f16", lib=lib)
    return out, None


def _eq(got, want, what):
    for g, w_, name in zip(got, want, ("out", "out_post")):
        assert (g is None) == (w_ is None), (what, name)
        if g is not None:
            assert torch.equal(g, w_), (what, name, int((g != w_).sum()))


# widths 1, 2, 29, 30, 31, 32 (a strip holds 30 columns and stages 34: x0 - 2 .. x0 + 31), 61 and 95; heights 1 .. 35; N 1, 2, 5
SHAPES = [(1, 1, 1), (2, 2, 2), (1, 3, 29), (5, 1, 30), (2, 3, 31), (1, 4, 32), (1, 2, 61), (2, 35, 95), (5, 3, 7), (1, 35, 31), (2, 17, 32)]


@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_pre_entry_equals_the_launches_it_replaces(shape, mode):
    N, h, w = shape
    m = sr3f()
    sp = _stage_pre(m)
    ops = _inputs(N, h, w, N * 1000 + h * 10 + w + mode)
    with torch.no_grad():
        assert sp.post_slopes_le_one and sp.slopes_le_one
        for post in (True, False):
            want = _replaced(m, ops, mode, post)
            assert all(torch.isfinite(t.float()).all() for t in want if t is not None)
            # row segmentations: 1 (every row is a segment's first and last row), 3, 16, one march (0); max and select build
            for rps in (1, 3, 16, 0):
                for le1 in (1, 0):
                    _eq(_launch_pre(sp, ops, mode, rps, le1, post), want, (rps, le1, post))
            # the wrapper's own choice of segments, fresh outputs and a caller's destination
            f, a, b, cmap = ops if mode == 3 else (ops[0], None, None, None)
            r = sp(f, a, b, cmap, post=post)
            _eq(r if post else (r, None), want, ("wrapper", post))
            dst = _nan(N, h, w)
            r = sp(f, a, b, cmap, out=dst, post=post)
            assert (r[0] if post else r) is dst
            _eq(r if post else (r, None), want, ("wrapper out=", post))
        # the planes of a launch are independent: N planes at once == N launches of one plane
        if N > 1:
            ones = [_launch_pre(sp, tuple(t[i:i + 1].contiguous() for t in ops[:3]) + (ops[3],), mode, 0, 1) for i in range(N)]
            _eq((torch.cat([o for o, _ in ones]), torch.cat([p for _, p in ones])), want if want[1] is not None else _replaced(m, ops, mode), "plane by plane")


@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 4, 61), (1, 1, 30)])
def test_padding_pixels_hold_zeros_not_the_chain_of_zero_operands(shape, mode):
    """Large biases and a large constant map: the chain maps zero operands to values far from zero, so a ring whose out-of-image pixels
    held the folded value instead of zeros would change every output near the border."""
    N, h, w = shape
    m = sr3f()
    b = m.block
    with torch.no_grad():
        b.compress_out[0].bias.add_(6.0)
        b.compress_in[0].bias.add_(5.0)
        b.uptranBlocks[0][0].bias.add_(7.0)
    sp = _stage_pre(m)
    ops = _inputs(N, h, w, 77 + w)
    ops = ops[:3] + (ops[3] + 9.0,)
    zeros = tuple(torch.zeros_like(t) for t in ops[:3]) + (torch.zeros_like(ops[3]),)
    with torch.no_grad():
        pad = _chain_launch(m, zeros, mode).float()      # what a padding pixel must NOT hold
        assert float((pad != 0).float().mean()) > 0.9 and float(pad.abs().max()) > 1.0
        want = _replaced(m, ops, mode)
        assert all(torch.isfinite(t.float()).all() for t in want)
        for rps in (0, 1, 2):
            _eq(_launch_pre(sp, ops, mode, rps, 1), want, rps)


@pytest.mark.parametrize("slopes", [(1.5, 0.25, 0.25), (0.25, -0.5, 0.25), (0.25, 0.25, 2.5), (-0.75, 1.25, -0.5), (0.5, 3.0, 0.125)])
@pytest.mark.parametrize("mode", [3, 2])
def test_pre_entry_slopes_of_any_sign_and_size(mode, slopes):
    """Slopes (compress_out, compress_in, uptran slice 0) above 1 and below 0, set on the module before packing: the wrapper passes the
    module's own promise, the select build is launched directly."""
    N, h, w = 2, 9, 33
    m = sr3f()
    b = m.block
    with torch.no_grad():
        b.compress_out[1].weight.fill_(slopes[0])
        b.compress_in[1].weight.fill_(slopes[1])
        b.uptranBlocks[0][1].weight.fill_(slopes[2])
    sp = _stage_pre(m)
    assert sp.post_slopes_le_one == sp.slopes_le_one == all(s <= 1.0 for s in slopes)
    ops = _inputs(N, h, w, 5 + mode)
    with torch.no_grad():
        for post in (True, False):
            want = _replaced(m, ops, mode, post)
            _eq(_launch_pre(sp, ops, mode, 4, 0, post), want, ("select", post))
            f, a, b_, cmap = ops if mode == 3 else (ops[0], None, None, None)
            r = sp(f, a, b_, cmap, post=post)
            _eq(r if post else (r, None), want, ("wrapper", post))


# ---------------------------------------------------------------------------------------------------------------- exact arithmetic
def _gen(seed, shape, profile):
    """Exact operands: the chain's (small integers, sparse unit weights), the stage's as test_gpu_exact_sr.gen_stage draws them, the
    POST slice's.  Integer-preserving chain slopes (0, 1, 2, -1) keep the stage's input integral."""
    N, h, w = shape
    rs = np.random.RandomState(seed)
    P, k, S = h * w, 7, 3
    c = dict(feat=E.ints(rs, (N, 32, P), -1, 1), la=E.ints(rs, (N, 32, P), -1, 1), lb=E.ints(rs, (N, 32, P), -1, 1), cmap=E.ints(rs, (32, P), -1, 1),
             co_wa=E.sparse_weights(rs, (32, 32), 0.05, 1), co_wb=E.sparse_weights(rs, (32, 32), 0.05, 1), co_b=E.ints(rs, (32,), -1, 1),
             ci_wf=E.sparse_weights(rs, (32, 32), 0.05, 1), ci_wp=E.sparse_weights(rs, (32, 32), 0.05, 1), ci_b=E.ints(rs, (32,), -1, 1),
             ut_w=E.sparse_weights(rs, (32, 32), 0.05, 1), ut_b=E.ints(rs, (32,), -1, 1))
    t1, t3 = 32.0 * (k / S) ** 2, 32.0 * k * k
    d1, d2, d3 = {"up": (24.0 / t1, 0.12, 3.0 / t3), "dt": (3.0 / t1, 1.0, 4.0 / t3), "dn": (0.5 / t1, 0.03, 0.12)}[profile]
    c.update(up_w=E.sparse_weights(rs, (32, 32, k, k), min(1.0, d1), 1), up_b=E.ints(rs, (32,), -2, 2), dt_w=E.sparse_weights(rs, (32, 32), d2, 1),
             dt_b=E.ints(rs, (32,), -2, 2), dn_w=E.sparse_weights(rs, (32, 32, k, k), d3, 1), dn_b=E.ints(rs, (32,), -3, 3),
             post_w=E.sparse_weights(rs, (32, 32), 0.06, 1), post_b=E.ints(rs, (32,), -2, 2))
    return c


def _ref(c, shape, mode, cs, ss=(0.5, 0.5, 0.5), ps=0.5, live=True):
    """float64 evaluation (the budget of every sum and every stored value checked by tests/_exact.py) -> dict(x, out, post)."""
    N, h, w = shape
    if mode == 3:
        st = [dict(ins=[(c["la"], c["co_wa"]), (c["lb"], c["co_wb"])], bias=c["co_b"], cmap=c["cmap"], slope=cs[0]),
              dict(ins=[(c["feat"], c["ci_wf"])], prev=c["ci_wp"], bias=c["ci_b"], slope=cs[1])]
    else:
        st = [dict(ins=[(c["feat"], c["ci_wf"]), (c["feat"], c["ci_wp"])], bias=c["ci_b"], slope=cs[1])]
    st.append(dict(ins=[], prev=c["ut_w"], bias=c["ut_b"], slope=cs[2]))
    x = E.chain_ref(st, live=live)[-1].reshape(N, 32, h, w)
    ref = E.stage_ref(x, c["up_w"], c["up_b"], ss[0], c["dt_w"], c["dt_b"], ss[1], c["dn_w"], c["dn_b"], ss[2], 3, live=live, min_distinct=100)
    p0 = E.conv_ref(ref["out"], c["post_w"].reshape(32, 32, 1, 1), c["post_b"], what="POST 1x1", store=torch.float16)
    return dict(x=x, out=ref["out"], post=E.check_storable(E.prelu_ref(p0, ps), torch.float16, "POST after PReLU"))


def _case(seed, shape, mode, profile, cs, live=True):
    """The first seed from `seed` on whose float64 evaluation stays inside the budget (the reference decides, not the kernel)."""
    for s in range(seed, seed + 40):
        c = _gen(s, shape, profile)
        try:
            return c, _ref(c, shape, mode, cs, live=live)
        except E.BudgetError:
            continue
    raise AssertionError(f"no operands inside the budget for {shape} {mode} {profile} {cs}")


def _module(c, cs, ss=(0.5, 0.5, 0.5), ps=0.5):
    """tests/test_gpu_exact_sr.module with the stage's and the POST slice's weights, + the three 1x1s of the chain."""
    m = module(3, dict(up_w=c["up_w"], up_b=c["up_b"], up_a=ss[0], dt_w=c["dt_w"], dt_b=c["dt_b"], dt_a=ss[1], dn_w=c["dn_w"], dn_b=c["dn_b"], dn_a=ss[2],
                       post_w=c["post_w"], post_b=c["post_b"], post_a=ps))
    b = m.block
    with torch.no_grad():
        assert b.compress_out[0].weight.shape[1] == 192 and b.compress_in[0].weight.shape[1] == 64 and b.uptranBlocks[0][0].weight.shape[1] >= 64
        b.compress_out[0].weight[:, 64:96, 0, 0] = c["co_wa"].float().cuda()
        b.compress_out[0].weight[:, 160:192, 0, 0] = c["co_wb"].float().cuda()
        b.compress_out[0].bias.copy_(c["co_b"])
        b.compress_out[1].weight.fill_(cs[0])
        b.compress_in[0].weight[:, 0:32, 0, 0] = c["ci_wf"].float().cuda()
        b.compress_in[0].weight[:, 32:64, 0, 0] = c["ci_wp"].float().cuda()
        b.compress_in[0].bias.copy_(c["ci_b"])
        b.compress_in[1].weight.fill_(cs[1])
        b.uptranBlocks[0][0].weight[:, 32:64, 0, 0] = c["ut_w"].float().cuda()
        b.uptranBlocks[0][0].bias.copy_(c["ut_b"])
        b.uptranBlocks[0][1].weight.fill_(cs[2])
    return m


def _exact_ops(c, shape):
    N, h, w = shape
    t = lambda x: E.nhwc(x.reshape(N, 32, h, w)).cuda()
    return t(c["feat"]), t(c["la"]), t(c["lb"]), c["cmap"].t().contiguous().float().cuda()


@pytest.mark.parametrize("cs", [(0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (2.0, 1.0, -1.0), (-1.0, 2.0, 0.0)])
@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("shape,profile", [((1, 1, 29), "up"), ((1, 2, 30), "dt"), ((2, 37, 31), "dn"), ((2, 5, 61), "up"), ((1, 1, 1), "dt"), ((2, 9, 33), "dn")])
def test_pre_entry_equals_float64(shape, profile, mode, cs):
    c, ref = _case(shape[0] * 1000 + shape[1] * 10 + shape[2] + 7 * mode, shape, mode, profile, cs, live=shape != (1, 1, 1))
    m = _module(c, cs)
    sp = _stage_pre(m)
    ops = _exact_ops(c, shape)
    what = f"x3 PRE{mode} {shape} {profile} {cs}"
    f, a, b, cmap = ops if mode == 3 else (ops[0], None, None, None)
    out, post = sp(f, a, b, cmap)
    E.assert_exact(E.nchw64(out), ref["out"], what + " out (wrapper)")
    E.assert_exact(E.nchw64(post), ref["post"], what + " post (wrapper)")
    E.assert_exact(E.nchw64(sp(f, a, b, cmap, post=False)), ref["out"], what + " out (wrapper, no POST)")
    for rps in (0, 3, 1):
        out, post = _launch_pre(sp, ops, mode, rps, 0)
        E.assert_exact(E.nchw64(out), ref["out"], f"{what} out rps {rps}")
        E.assert_exact(E.nchw64(post), ref["post"], f"{what} post rps {rps}")


PLANTS = [("co_wa", (3, 0)), ("co_wb", (31, 31)), ("ci_wf", (17, 8)), ("ci_wp", (5, 23)), ("ci_wp", (30, 2)), ("ut_w", (0, 0)), ("ut_w", (21, 29))]


@pytest.mark.parametrize("which,idx", PLANTS)
@pytest.mark.parametrize("mode", [3, 2])
def test_one_unit_in_one_weight_of_the_folded_chain_is_seen_with_its_footprint(mode, which, idx):
    """The kernel's chain weights differ from the reference's by ONE unit in ONE element (compress_out, either half of compress_in, the
    uptran slice): both outputs equal the float64 evaluation of the CHANGED weights, differ from the unchanged one, and differ exactly
    where the two evaluations differ.  (compress_out is not part of PRE2: planted there, nothing may change.)"""
    shape, cs = (2, 7, 33), (1.0, 1.0, 1.0)      # (slopes 1: nothing is clipped away)
    for seed in range(40, 90):
        c = _gen(seed, shape, "up")
        c2 = dict(c)
        c2[which] = c[which].clone()
        c2[which][idx] += 1.0
        try:
            ref, planted = _ref(c, shape, mode, cs), _ref(c2, shape, mode, cs)
            break
        except E.BudgetError:
            continue
    else:
        raise AssertionError("no operands inside the budget")
    pred_out, pred_post = planted["out"] != ref["out"], planted["post"] != ref["post"]
    m = _module(c2, cs)
    ops = _exact_ops(c, shape)
    f, a, b, cmap = ops if mode == 3 else (ops[0], None, None, None)
    out, post = _stage_pre(m)(f, a, b, cmap)
    got_out, got_post = E.nchw64(out), E.nchw64(post)
    E.assert_exact(got_out, planted["out"], f"planted {which}{idx}: the kernel follows its own weights (out)")
    E.assert_exact(got_post, planted["post"], f"planted {which}{idx}: the kernel follows its own weights (post)")
    if mode == 2 and which.startswith("co_"):
        assert not pred_out.any() and not pred_post.any()
        return
    assert pred_out.any() and (planted["x"] != ref["x"]).any()
    with pytest.raises(AssertionError, match="differ from the float64 evaluation"):
        E.assert_exact(got_out, ref["out"], "planted")
    assert torch.equal(E.diff_mask(got_out, ref["out"]), pred_out)
    assert torch.equal(E.diff_mask(got_post, ref["post"]), pred_post)


# ---------------------------------------------------------------------------------------------------------------- poisoned buffers
@pytest.mark.parametrize("mode", [3, 2])
def test_pre_entry_poisoned_outputs_are_fully_written_and_bands_intact(mode):
    """The launch itself on arena buffers with a ragged strip and a ragged segment: every element of both outputs written, no byte
    outside either; then through the wrapper with a caller's `out=` destination, with and without POST."""
    m = sr3f()
    sp = _stage_pre(m)
    ops = _inputs(2, 11, 37, 5)
    with torch.no_grad():
        want, want_plain = _replaced(m, ops, mode), _replaced(m, ops, mode, post=False)
    f, a, b, cmap = ops if mode == 3 else (ops[0], None, None, None)
    with poisoned() as arena:
        out = torch.empty((2, 11, 37, 32), dtype=torch.float16, device="cuda")
        post = torch.empty((2, 11, 37, 32), dtype=torch.float16, device="cuda")
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(post).all())
        lib = load_s3f()
        L.check(lib.vsr_s3f_sr_utd_pre_f16(L.dptr(f, torch.float16), L.optr(a, torch.float16), L.optr(b, torch.float16), L.optr(cmap), L.dptr(sp.blob, torch.uint8),
                                           L.dptr(out, torch.float16), L.dptr(post, torch.float16), 2, 11, 37, 4, 1, L.stream()), "sr_utd_s3_pre_f16", lib=lib)
        torch.cuda.synchronize()
        arena.assert_written(out, "out")
        arena.assert_written(post, "out_post")
        _eq((out, post), want, "arena")
        arena.check()
        dst = torch.empty((2, 11, 37, 32), dtype=torch.float16, device="cuda")
        o, p = sp(f, a, b, cmap, out=dst)
        torch.cuda.synchronize()
        assert o is dst
        arena.assert_written(dst, "out=")
        arena.assert_written(p, "out_post of the wrapper")
        _eq((dst, p), want, "arena wrapper")
        o = sp(f, a, b, cmap, post=False)
        torch.cuda.synchronize()
        arena.assert_written(o, "out without POST")
        _eq((o, None), want_plain, "arena wrapper without POST")
        arena.check()


@pytest.mark.parametrize("hw", [(9, 40), (37, 33)])
def test_x3_network_with_the_fold_on_poisoned_buffers(hw):
    rs = np.random.RandomState(hw[0] * 31 + hw[1])

    def call(m, x, _):
        assert m.fold_chain
        with torch.no_grad():
            (full, dec), n = _counted(lambda: [m(x), m(x, decimate=True)])
        assert n["pre"] == 2 * m.num_steps
        return [full, dec]
    run_poisoned(lambda: sr3f(fold_chain=True), call, _sr_inputs(rs, *hw), _sr_inputs(rs, *hw), what=f"x3 SR net with the fold {hw}")


# ---------------------------------------------------------------------------------------------------------------- module level
def _counted(fn):
    """fn() with the launch timer on -> (result, counts): `pre` = launches of the new entry, `post` / `plain` = of the POST / plain x3
    stage, `chain` = 1x1 chain launches of any length, `chain3` / `chain2` = the three-stage / two-stage ones (what the fold replaces)."""
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
    cnt = lambda pre: sum(v[0] for k, v in s.items() if k.startswith(pre))
    return r, dict(pre=cnt("sr_utd_s3_pre_f16"), post=cnt("sr_utd_s3_post_f16"), plain=cnt("sr_utd_s3_f16"), chain=cnt("sr_chain1x1_f16"),
                   chain3=cnt("sr_chain1x1_f16 x3"), chain2=cnt("sr_chain1x1_f16 x2"))


def _on_off(run, folded, make=sr3f, uptran=True):
    """run(m) with fold_chain on and off on fresh modules: equal results; the new entry ran `folded` times, there is one chain launch
    fewer per folded step and the stage launch it absorbed is gone -- a silent fall-back fails here."""
    m_on, m_off = make(fold_chain=True, fuse_uptran=uptran), make(fold_chain=False, fuse_uptran=uptran)
    with torch.no_grad():
        r_on, n_on = _counted(lambda: run(m_on))
        r_off, n_off = _counted(lambda: run(m_off))
    assert n_off["pre"] == 0 and n_on["pre"] == folded > 0, (n_on, n_off)
    assert n_on["chain"] == n_off["chain"] - folded, (n_on, n_off)
    assert n_on["chain3"] + n_on["chain2"] == 0 and n_off["chain3"] + n_off["chain2"] == folded, (n_on, n_off)
    absorbed = "post" if uptran else "plain"
    assert n_on[absorbed] == n_off[absorbed] - folded, (n_on, n_off)
    assert len(r_on) == len(r_off)
    for i, (a, b) in enumerate(zip(r_on, r_off)):
        assert a.shape == b.shape and torch.isfinite(a).all()
        assert torch.equal(a, b), i
    return r_on


def _frames(seed, hw):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (8, 3) + tuple(hw)).astype(np.float32)).cuda()


def test_the_switch_exists_and_packs_the_pre_build():
    from video_super_resolution_amd import SRProjectionModule
    assert isinstance(SRProjectionModule.fold_chain, bool)
    P = sr3f()._packed()
    assert sorted(P["stage_pre"]) == [0] and sorted(P["stage_post"]) == [0] and sorted(P["stage"]) == [0, 3]


@pytest.mark.parametrize("uptran", [True, False])
@pytest.mark.parametrize("hw", [(9, 33), (37, 45), (1, 7)])
def test_module_fold_chain_on_equals_off_full_and_decimated(hw, uptran):
    x = _frames(hw[0] * 3 + hw[1], hw)
    steps = sr3f().num_steps
    full, dec = _on_off(lambda m: [m(x), m(x, decimate=True)], 2 * steps, uptran=uptran)
    assert torch.equal(dec, full[..., ::3, ::3])


@pytest.mark.parametrize("ahead", ["kept", "precompute_shared", "precompute_rows"])
@pytest.mark.parametrize("hw", [(9, 40), (37, 33)])
def test_module_fold_chain_on_equals_off_with_shared_planes(hw, ahead):
    """Two calls that share their first three planes: kept by the first call, evaluated ahead by `precompute_shared` (with the
    pre-fusion planes), and with plane 7 ahead as well (`precompute_rows`): each goes through the stage loop with a destination."""
    h, w = hw
    x = _frames(h * 17 + w, hw)
    x2 = x.clone()
    x2[3:] = _frames(h * 17 + w + 1, hw)[3:]
    steps = sr3f().num_steps

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
        plain = sr3f(fold_chain=False)
        assert torch.equal(r[0], plain(x, decimate=True)) and torch.equal(r[1], plain(x2))


def test_module_fold_chain_with_slopes_above_one_in_the_chain():
    x = _frames(77, (12, 35))

    def make(**attrs):
        m = sr3f(**attrs)
        with torch.no_grad():
            m.block.compress_in[1].weight.fill_(1.75)
            m.block.uptranBlocks[0][1].weight.fill_(-0.25)
        return m
    _on_off(lambda m: [m(x)], sr3f().num_steps, make=make)
    sp = make()._packed()["stage_pre"][0]
    assert not sp.post_slopes_le_one and not sp.slopes_le_one


def test_module_taps_path_falls_back_to_the_chain_launch():
    """`taps` needs the chain's intermediate tensors: with the switch on the chain launches run and the new entry does not."""
    x = _frames(5, (6, 10))
    ta, tb = {}, {}
    with torch.no_grad():
        m = sr3f(fold_chain=True)
        a, n = _counted(lambda: m(x, taps=ta))
        b = sr3f(fold_chain=False)(x, taps=tb)
    assert n["pre"] == 0 and n["chain3"] + n["chain2"] == m.num_steps
    assert torch.equal(a, b) and sorted(ta) == sorted(tb) and len(ta) > 3
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k


def test_module_fixture_with_the_fold(golden):
    g = golden("g8_sr_x3_6x10")
    x = torch.from_numpy(g["x"]).cuda()
    m = sr3f(fold_chain=True)
    with torch.no_grad():
        (out,), n = _counted(lambda: [m(x)])
    assert n["pre"] == m.num_steps and n["plain"] == m.num_steps and n["post"] == 0 and n["chain3"] + n["chain2"] == 0
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


def test_vsr_forward_x3_fold_chain_on_equals_off(cpu_vsr):
    data = torch.from_numpy(np.random.RandomState(33).randint(0, 256, (3, 66, 70, 3)).astype(np.float32)).cuda()
    (on, n_on) = _counted(lambda: _two_calls(_vsr(cpu_vsr, fold_chain=True), data, 3))
    (off, n_off) = _counted(lambda: _two_calls(_vsr(cpu_vsr, fold_chain=False), data, 3))
    assert n_on["pre"] > 0 and n_off["pre"] == 0
    assert n_on["chain"] == n_off["chain"] - n_on["pre"] and n_on["post"] == n_off["post"] - n_on["pre"], (n_on, n_off)
    assert n_on["chain3"] + n_on["chain2"] == 0 and n_off["chain3"] + n_off["chain2"] == n_on["pre"]
    for a, b in zip(on, off):
        assert a.shape == (1, 198, 210, 3) and torch.equal(a, b)


def test_graphed_vsr_recaptures_when_the_switch_flips(cpu_vsr):
    from video_super_resolution_amd import GraphedVSR
    data = torch.from_numpy(np.random.RandomState(35).randint(0, 256, (3, 66, 70, 3)).astype(np.float32)).cuda()
    m = _vsr(cpu_vsr, fold_chain=False)
    g = GraphedVSR(m)
    with torch.no_grad():
        ref, _ = m(data, None, None, None, train=False)
        a, _ = g(data, None, None, None, train=False)
        assert len(g._graphs) == 1 and torch.equal(a, ref)
        k_off = g._key(data, None)
        m.model.fold_chain = True
        assert g._key(data, None) != k_off
        b, _ = g(data, None, None, None, train=False)                          # a new capture
        assert len(g._graphs) == 2 and torch.equal(b, ref)
        c, _ = g(data, None, None, None, train=False)                          # a replay
        assert len(g._graphs) == 2 and torch.equal(c, ref)
        m.model.fold_chain = False
        d, _ = g(data, None, None, None, train=False)
        assert len(g._graphs) == 2 and torch.equal(d, ref)
    torch.cuda.synchronize()


@pytest.mark.parametrize("scale", [4, 2])
def test_x4_and_x2_forwards_do_not_load_the_pre_library(scale):
    """A fresh interpreter (this one has loaded the library long ago): VSR.forward at x4 / x2, with the switch ON, and nothing of
    libvsr_hip_s3f.so."""
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
m.model.fold_chain = True
data = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (3, 66, 70, 3)).astype(np.float32)).cuda()
with torch.no_grad():
    out, _ = m(data, None, None, None, train=False)
    out, _ = m(data, None, None, out, train=False)
torch.cuda.synchronize()
assert torch.isfinite(out).all()
assert _lib._s3flib is None, "an x{scale} forward loaded libvsr_hip_s3f.so"
assert 'libvsr_hip_s3f' not in open('/proc/self/maps').read()
print('ok')
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
