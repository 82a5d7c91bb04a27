"""libvsr_hip_opt.so on the GPU (include/vsr_hip_opt.h), optim.Adam and driver.train_step.

The kernels are held to tests/_adam_ref.py (the header's formulas in numpy float32, pinned against torch.optim.Adam on the CPU by
tests/test_adam_ref_helper.py) BIT FOR BIT: p, m and v after each of three consecutive steps, aligned and misaligned, with and without
weight decay and clipping.  The norm is exact on integers, the same bits in every run, correctly rounded to within n x 2^-53.  The
optimizer is held to torch.optim.Adam(foreach=False) on CPU copies to the bar of the helper test, 16 x 2^-23 x max|torch| per tensor
(torch groups the same operations differently: addcmul, addcdiv).  Every case is seeded and takes seconds."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _adam_ref as R  # noqa: E402
from _poison import poisoned  # noqa: E402
from video_super_resolution_amd import _lib, driver, optim  # noqa: E402

SIZES = [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8195]    # one plan of eleven tensors: 14 chunks, short and whole, odd tails
BAR = 16 * 2.0 ** -23
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def dev(a, misaligned=False):
    """The array on the device: a fresh allocation (16-byte aligned), or the [1:] view of one (4-byte aligned only)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misaligned:
        out = torch.empty(t.shape, dtype=t.dtype, device="cuda")
        out.copy_(t)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:].copy_(t)
    out = buf[1:]
    assert out.data_ptr() % 16 == 4
    return out


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(t, a):
    return torch.equal(bits(t), torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32))


class Plan:
    """A plan image for [(p, g, m, v)], uploaded; keeps the tensors alive."""

    def __init__(self, entries):
        self.L = L = _lib.load_opt()
        self.entries = entries
        n = len(entries)
        sizes = (ctypes.c_ulonglong * n)(*(e[0].numel() for e in entries))
        self.bytes = L.vsr_opt_plan_bytes(n, sizes)
        assert self.bytes > 0, L.vsr_opt_last_error()
        table = (_lib.OptTensor * n)(*(_lib.OptTensor(*(t.data_ptr() for t in e), e[0].numel()) for e in entries))
        self.host = ctypes.create_string_buffer(self.bytes)
        _lib.check(L.vsr_opt_plan_fill(self.host, self.bytes, n, table), "opt_plan_fill", lib=L)
        self.dev = torch.from_numpy(np.frombuffer(self.host.raw, dtype=np.uint8).copy()).cuda()
        self.n_chunks = L.vsr_opt_norm_ws_bytes(self.host) // 8

    def adam(self, t, wd, ctl=None):
        sc = optim.adam_scalars(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], wd, float(t))
        assert [np.float32(x) for x in sc] == list(R.scalars(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], wd, t))
        _lib.check(self.L.vsr_opt_adam_f32(self.host, self.dev.data_ptr(), None if ctl is None else ctl.data_ptr(), *sc, _lib.stream()),
                   "opt_adam_f32", lib=self.L)

    def norm(self, max_norm, ctl=None, ws=None):
        ctl = torch.empty(2, dtype=torch.float64, device="cuda") if ctl is None else ctl
        ws = torch.empty(self.n_chunks, dtype=torch.float64, device="cuda") if ws is None else ws
        _lib.check(self.L.vsr_opt_grad_norm(self.host, self.dev.data_ptr(), float(max_norm), ctl.data_ptr(), ws.data_ptr(), _lib.stream()),
                   "opt_grad_norm", lib=self.L)
        return ctl, ws


def read_ctl(ctl):
    """(c float32, pad float32, sumsq float64) of a device vsr_opt_ctl_t."""
    raw = ctl.cpu().numpy().tobytes()
    c, pad = np.frombuffer(raw[:8], dtype=np.float32)
    return c, pad, float(np.frombuffer(raw[8:], dtype=np.float64)[0])


def state0(seed, sizes=SIZES):
    rs = np.random.RandomState(seed)
    return rs, [rs.standard_normal(n).astype(np.float32) for n in sizes]


def grads_like(tensors, entries):
    """A zero-valued plan entry per tensor: only g matters to the norm."""
    return [(torch.zeros_like(g), g, torch.zeros_like(g), torch.zeros_like(g)) for g in tensors] if entries is None else entries


# ------------------------------------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned16", "aligned4"])
def test_adam_equals_the_restatement_bit_for_bit(misaligned, wd):
    rs, p = state0(11)
    m, v = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    dp, dm, dv = ([dev(a, misaligned) for a in arrs] for arrs in (p, m, v))
    dg = [dev(np.zeros_like(a), misaligned) for a in p]
    plan = Plan(list(zip(dp, dg, dm, dv)))
    assert plan.n_chunks == 9 + 2 + 3
    for t in (1, 2, 3):
        g = [R.gradient_family(rs, a.size, clamp=True) for a in p]
        for d, a in zip(dg, g):
            d.copy_(torch.from_numpy(a))
        plan.adam(t, wd)
        for i, n in enumerate(SIZES):
            p[i], m[i], v[i] = R.adam_step(p[i], g[i], m[i], v[i], wd=wd, t=t, **HYPER)
            assert same_bits(dp[i], p[i]), ("p", n, t)
            assert same_bits(dm[i], m[i]), ("m", n, t)
            assert same_bits(dv[i], v[i]), ("v", n, t)
            assert same_bits(dg[i], g[i]), ("g is read only", n, t)
    assert all(np.isfinite(a).all() for a in p + m + v)


def test_non_finite_gradients_propagate_as_the_formulas_say():
    rs, p = state0(12, [9])
    g = R.gradient_family(rs, 9, clamp=True)
    g[2], g[5] = np.inf, np.nan
    m, v = np.zeros(9, np.float32), np.zeros(9, np.float32)
    dp, dg, dm, dv = dev(p[0]), dev(g), dev(m), dev(v)
    Plan([(dp, dg, dm, dv)]).adam(1, 0.0)
    p1, m1, v1 = R.adam_step(p[0], g, m, v, wd=0.0, t=1, **HYPER)
    got = dp.cpu().numpy()
    assert np.isnan(got[[2, 5]]).all() and np.isnan(p1[[2, 5]]).all()
    keep = np.ones(9, bool)
    keep[[2, 5]] = False
    assert np.array_equal(got[keep].view(np.int32), p1[keep].view(np.int32))
    assert np.array_equal(np.isnan(dm.cpu().numpy()), np.isnan(m1)) and np.array_equal(np.isinf(dv.cpu().numpy()), np.isinf(v1))


# ------------------------------------------------------------------------------------------------ 2. the norm
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned16", "aligned4"])
def test_norm_is_exact_on_integers(misaligned):
    rs = np.random.RandomState(21)
    g = [rs.randint(-15, 16, n).astype(np.float32) for n in SIZES]
    dg = [dev(a, misaligned) for a in g]
    ctl, _ = Plan(grads_like(dg, None)).norm(1.0)
    c, pad, sumsq = read_ctl(ctl)
    exact = sum(int((a.astype(np.int64) ** 2).sum()) for a in g)
    assert sumsq == float(exact) and pad == 0.0
    want = R.clip_coefficient(float(exact), 1.0)
    assert abs(float(c) - float(want)) <= float(np.spacing(want)) and c < 1.0


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned16", "aligned4"])
def test_norm_bits_repeat_round_correctly_and_ignore_appended_zeros(misaligned):
    rs = np.random.RandomState(22)
    sizes = SIZES + [300007]                                          # 74 more chunks, 88 in all: pass 2 adds at most one partial per thread
    g = [R.gradient_family(rs, n) for n in sizes]
    dg = [dev(a, misaligned) for a in g]
    plan = Plan(grads_like(dg, None))
    ref = R.sumsq(g)
    n = sum(sizes)
    runs = [read_ctl(plan.norm(1.0)[0]) for _ in range(2)]
    assert runs[0] == runs[1]
    c, pad, sumsq = runs[0]
    print(f"sumsq {sumsq!r} against fsum {ref!r}: {abs(sumsq - ref) / ref / 2.0 ** -53:.2f} x 2^-53 (bar {n})")
    assert abs(sumsq - ref) <= n * 2.0 ** -53 * ref
    # the other alignment adds in the same order: the same bits
    other = Plan(grads_like([dev(a, not misaligned) for a in g], None))
    assert read_ctl(other.norm(1.0)[0]) == runs[0]
    # the same tensors with tensors of zeros behind them (short, whole and many chunks: 300 partials make pass 2 loop)
    zeros = [torch.zeros(k, device="cuda") for k in (1, 4096, 5000, 4096 * 200 + 3)]
    beside = Plan(grads_like(dg + zeros, None))
    assert beside.n_chunks > 256 > plan.n_chunks
    assert read_ctl(beside.norm(1.0)[0]) == runs[0]
    # the coefficient, above and below max_norm: within one float32 ulp of the float64 restatement
    norm = math.sqrt(ref)
    for max_norm in (norm * 0.37, norm * 2.5, 1e-3, 1e30):
        c = read_ctl(plan.norm(max_norm)[0])[0]
        want = R.clip_coefficient(ref, max_norm)
        assert abs(float(c) - float(want)) <= float(np.spacing(want)), (max_norm, c, want)
        assert (c < 1.0) == (max_norm < norm)
    assert read_ctl(plan.norm(float("inf"))[0])[0] == 1.0


def test_norm_with_more_partials_than_threads():
    """Pass 2's strided loop: 515 chunks, so threads 0..2 add three partials and the others two."""
    rs = np.random.RandomState(23)
    g = [rs.randint(-15, 16, n).astype(np.float32) for n in (4096 * 300 + 17, 4096 * 213 + 1)]
    plan = Plan(grads_like([dev(a) for a in g], None))
    assert plan.n_chunks == 515
    _, _, sumsq = read_ctl(plan.norm(1.0)[0])
    assert sumsq == float(sum(int((a.astype(np.int64) ** 2).sum()) for a in g))


# ------------------------------------------------------------------------------------------------ 3. bits with clipping
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned16", "aligned4"])
def test_clipped_adam_equals_the_restatement_fed_the_devices_coefficient(misaligned, wd):
    rs, p = state0(31)
    m, v = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    dp, dm, dv = ([dev(a, misaligned) for a in arrs] for arrs in (p, m, v))
    dg = [dev(np.zeros_like(a), misaligned) for a in p]
    plan = Plan(list(zip(dp, dg, dm, dv)))
    for t in (1, 2, 3):
        g = [R.gradient_family(rs, a.size, clamp=True) for a in p]
        for d, a in zip(dg, g):
            d.copy_(torch.from_numpy(a))
        ctl, _ = plan.norm(50.0)
        plan.adam(t, wd, ctl)
        c, _, sumsq = read_ctl(ctl)
        assert 0.0 < c < 1.0 and abs(sumsq - R.sumsq(g)) <= sum(SIZES) * 2.0 ** -53 * sumsq
        for i, n in enumerate(SIZES):
            p[i], m[i], v[i] = R.adam_step(p[i], g[i], m[i], v[i], wd=wd, t=t, c=c, **HYPER)
            assert same_bits(dp[i], p[i]) and same_bits(dm[i], m[i]) and same_bits(dv[i], v[i]), (n, t)
            assert same_bits(dg[i], g[i]), ("g is read only", n, t)


# ------------------------------------------------------------------------------------------------ 4. poisoned buffers
def test_poisoned_buffers_every_output_written_and_nothing_beyond():
    rs, p = state0(41)
    g = [R.gradient_family(rs, a.size, clamp=True) for a in p]
    with poisoned(package_state=False) as arena:
        def guarded(a):   # [poison | payload]: the view [1:] of an arena block, so the element before the view is a canary too
            buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
            assert arena.find(buf) is not None
            buf[1:].copy_(torch.from_numpy(a))
            return buf
        bp, bg = [guarded(a) for a in p], [guarded(a) for a in g]
        bm, bv = [guarded(np.zeros_like(a)) for a in p], [guarded(np.zeros_like(a)) for a in p]
        plan = Plan([tuple(b[1:] for b in row) for row in zip(bp, bg, bm, bv)])
        ctl = torch.empty(2, dtype=torch.float64, device="cuda")
        ws = torch.empty(plan.n_chunks, dtype=torch.float64, device="cuda")
        assert arena.find(ctl) is not None and arena.find(ws) is not None
        plan.norm(50.0, ctl, ws)
        arena.assert_written(ctl, "ctl")
        arena.assert_written(ctl.view(torch.float32), "ctl as floats")       # c and the pad
        arena.assert_written(ws, "the workspace partials")
        c, pad, sumsq = read_ctl(ctl)
        assert pad == 0.0 and torch.isfinite(ws).all() and float(ws.sum()) == pytest.approx(sumsq, rel=1e-12)
        plan.adam(1, 1e-2, ctl)
        for i, n in enumerate(SIZES):
            p1, m1, v1 = R.adam_step(p[i], g[i], np.zeros_like(p[i]), np.zeros_like(p[i]), wd=1e-2, t=1, c=c, **HYPER)
            assert same_bits(bp[i][1:], p1) and same_bits(bm[i][1:], m1) and same_bits(bv[i][1:], v1), n
            assert same_bits(bg[i][1:], g[i]), n
            for b in (bp[i], bg[i], bm[i], bv[i]):
                assert int(b[:1].view(torch.int32)) == -1, ("the element before the tensor was written", n)
        arena.check()


# ------------------------------------------------------------------------------------------------ 5. the optimizer
def _cpu_twin(model):
    """CPU copies of the module's parameters, in order, under torch.optim.Adam(foreach=False)."""
    twins = [torch.nn.Parameter(p.detach().cpu().clone(), requires_grad=p.requires_grad) for p in model.parameters()]
    return twins, torch.optim.Adam(twins, lr=1e-3, foreach=False)


SMALL = 32   # elements: below this a tensor's m is held to the scale of its operands (see the optimizer test)


def _units(ours, ref, floor=0.0):
    """max|ours - torch| in units of 2^-23 x max(max|torch|, floor) of the tensor (the bar is 16 of them)."""
    scale = max(ref.abs().max().item(), floor)
    err = (ours.detach().cpu().double() - ref.detach().double()).abs().max().item()
    return 0.0 if err == 0.0 else err / (2.0 ** -23 * scale) if scale > 0 else math.inf


def test_optimizer_follows_torch_adam_over_the_sr_nets_parameters(gpu_vsr):
    """Five steps of optim.Adam on the device beside torch.optim.Adam(foreach=False) on CPU copies fed the same gradients.  After EVERY
    step p, m and v of every tensor are within 16 x 2^-23 x max|torch| -- with one deviation, for m of tensors of fewer than 32 elements.

    31 of the 87 tensors have one or three elements (PReLU slopes, the colour biases).  For them max|torch| is the value itself, and
    m' = m + omb1 * (g - m) with g and m of opposite sign leaves a small result that carries the roundings of its larger operands: the
    kernel (every operation rounded, bit-equal to tests/_adam_ref.py) and torch's lerp then differ by a rounding of the OPERANDS, which
    is any number of units of the result.  Measured on the device with the scale max|torch|: 22.7 units in m of tensor 46 (one element,
    0.0426; 1.15e-7 absolute = one ulp at 1) after step 4; on the CPU 0.06 % .. 0.7 % of single elements exceed 16 units of their own
    value at a given step (LAB_NOTES "Adam step", C).  For those tensors the scale of m is therefore max(max|torch m|, G), G the largest
    |g| the tensor has seen so far (|m| <= G always: m is a convex combination of the gradients).  Why 16 units of it hold: one step
    rounds g - m, its product and the sum, at most 2^-24 x (2G + 0.2G + G) = 1.6 units of 2^-23 G; torch commits at most as much; the
    difference is carried on with the factor beta1, so after five steps at most 3.2 x (1 + 0.9 + ... + 0.9^4) = 13.1 units.  p and v keep
    the issue's scale at every size: v sums non-negative terms, and m's difference reaches p as lr x (1e-7 G) / d with d of the order of G:
    1e-10, below a rounding of any parameter larger than 1e-3."""
    m = copy.deepcopy(gpu_vsr.model).train()
    assert m.upscale_factor == 4
    x = torch.from_numpy(np.random.RandomState(51).randint(0, 256, (8, 3, 7, 9)).astype(np.float32)).cuda()
    params = list(m.parameters())
    opt = optim.Adam(params, lr=1e-3)
    twins, ref = _cpu_twin(m)
    held, seen = [], {}     # seen: per tensor the largest |g| so far
    for step in range(1, 6):
        if step == 3:
            held = [p.grad for p in params if p.grad is not None]   # kept alive: the next gradients cannot take their addresses
        opt.zero_grad(set_to_none=True)
        (m(x) ** 2).mean().backward()
        for p, q in zip(params, twins):
            q.grad = None if p.grad is None else p.grad.detach().cpu().clone()
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        plans = len(opt._plans)
        opt.step()
        ref.step()
        assert opt.launches == 1
        if step == 1:
            assert plans == 0 and len(opt._plans) == 1
        if step == 3:
            assert len(opt._plans) == plans + 1, "new gradient addresses must miss the plan cache"
        n_live, last = 0, {}
        for i, (p, q) in enumerate(zip(params, twins)):
            if p.grad is None:
                assert p not in opt.state or len(opt.state[p]) == 0
                assert torch.equal(p.detach().cpu(), q.detach())        # a parameter without a gradient keeps its value
                continue
            n_live += 1
            assert torch.equal(p.grad, grads[i])                         # .grad is read only
            st, rt = opt.state[p], ref.state[q]
            assert st["step"].device.type == "cpu" and float(st["step"]) == float(rt["step"]) == step
            seen[i] = max(seen.get(i, 0.0), q.grad.abs().max().item())
            last[("p", i, p.numel())] = _units(p, q)
            last[("m", i, p.numel())] = _units(st["exp_avg"], rt["exp_avg"], seen[i] if p.numel() < SMALL else 0.0)
            last[("v", i, p.numel())] = _units(st["exp_avg_sq"], rt["exp_avg_sq"])
        assert 60 <= n_live <= 87 and len(params) == 91
        worst = {k: max((u, key) for key, u in last.items() if key[0] == k) for k in "pmv"}
        print(f"step {step}: worst units of the bar's scale (quantity, tensor, elements): " +
              ", ".join(f"{k} {u:.2f} {key[1:]}" for k, (u, key) in worst.items()))
        over = {key: round(u, 2) for key, u in last.items() if not u <= 16}
        assert not over, (step, over)
    del held


def test_optimizer_clips_in_three_launches_and_skips_what_has_no_gradient(gpu_vsr):
    m = copy.deepcopy(gpu_vsr.model).train()
    x = torch.from_numpy(np.random.RandomState(52).randint(0, 256, (8, 3, 7, 9)).astype(np.float32)).cuda()
    params = list(m.parameters())
    (m(x) ** 2).mean().backward()
    grads = {i: p.grad.detach().clone() for i, p in enumerate(params) if p.grad is not None}
    sumsq = sum(float((g.double() ** 2).sum()) for g in grads.values())
    no_grad = [i for i, p in enumerate(params) if p.grad is None]
    assert no_grad
    # two groups, one step value each: the norm spans both: its two launches and one update per group
    half = len(params) // 2
    before = [p.detach().clone() for p in params]
    opt = optim.Adam([{"params": params[:half]}, {"params": params[half:], "lr": 1e-4}], max_grad_norm=math.sqrt(sumsq) / 4)
    opt.step()
    assert opt.launches == 4
    assert float(opt.last_grad_norm_sq) == pytest.approx(sumsq, rel=1e-12)
    for i, p in enumerate(params):
        if i in grads:
            assert torch.equal(p.grad, grads[i])                        # clipping scales what the update reads, never .grad
            assert not torch.equal(p.detach(), before[i]) or not grads[i].any()
            assert float(opt.state[p]["step"]) == 1.0
        else:
            assert torch.equal(p.detach(), before[i]) and len(opt.state[p]) == 0
    # one group: the norm's plan is the update's: three launches, one plan
    m2 = copy.deepcopy(gpu_vsr.model).train()
    p2 = list(m2.parameters())
    for p, g in zip(p2, (grads.get(i) for i in range(len(p2)))):
        p.grad = None if g is None else g.clone()
    one = optim.Adam(p2, max_grad_norm=math.sqrt(sumsq) / 4)
    one.step()
    assert one.launches == 3 and len(one._plans) == 1
    assert float(one.last_grad_norm_sq) == pytest.approx(sumsq, rel=1e-12)
    # clipped to a quarter: the first step of Adam is scale free up to eps, so p moves like the unclipped step; m is a quarter
    free = optim.Adam([torch.nn.Parameter(before[i].clone()) for i in grads], lr=1e-3)
    for q, i in zip(free.param_groups[0]["params"], grads):
        q.grad = grads[i].clone()
    free.step()
    assert free.launches == 1 and free.last_grad_norm_sq is None
    i0 = max(grads, key=lambda i: grads[i].numel())
    a, b = one.state[p2[i0]]["exp_avg"], free.state[free.param_groups[0]["params"][list(grads).index(i0)]]["exp_avg"]
    c = (math.sqrt(sumsq) / 4) / (math.sqrt(sumsq) + 1e-6)
    assert 0.2 < c <= 0.25 and torch.allclose(a / c, b, rtol=1e-5, atol=0)
    # a non-contiguous or half parameter: refused, no fallback
    w = torch.nn.Parameter(torch.zeros(4, 6, device="cuda").t())
    w.grad = torch.ones_like(w)
    with pytest.raises(_lib.VsrHipError, match="contiguous"):
        optim.Adam([w]).step()
    h = torch.nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float16))
    h.grad = torch.ones_like(h)
    with pytest.raises(_lib.VsrHipError, match="float32"):
        optim.Adam([h]).step()


# ------------------------------------------------------------------------------------------------ 6. the driver
def test_driver_train_step_updates_only_the_sr_net_and_repeats_its_bits(golden, gpu_vsr):
    g = golden("g10_loss")
    data, target, high_frames = driver.ingest_item(torch.from_numpy(g["hr"]).unsqueeze(0).cuda(), 4)
    x, y, high_frame = data[0], target[0], high_frames[0]
    results = []
    for run in range(2):
        model = copy.deepcopy(gpu_vsr)
        model.train()                                         # main.py:178
        optimizer = optim.Adam(model.parameters(), lr=1e-3, max_grad_norm=1.0)
        optimizer.zero_grad()
        with torch.no_grad():                                 # main.py:199-203
            estimated_image, real_loss = model(x, y, high_frame, None)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        output, loss = driver.train_step(model, optimizer, x, y, high_frame, estimated_image, loss_value=real_loss.data)
        after = model.state_dict()
        changed = {k.split(".")[0] for k in before if not torch.equal(before[k], after[k])}
        assert changed == {"model"}, changed
        assert not torch.equal(before["model.conv_in.0.weight"], after["model.conv_in.0.weight"])
        assert torch.equal(before["model.sub_mean.bias"], after["model.sub_mean.bias"])
        assert float(loss) == float(real_loss) and loss.dim() == 0 and not output.requires_grad and output.shape == estimated_image.shape
        assert optimizer.launches == 3 and float(optimizer.last_grad_norm_sq) > 0
        results.append({k: v.detach().clone() for k, v in after.items()})
    assert all(torch.equal(results[0][k], results[1][k]) for k in results[0])
    # ... and the function takes the stock optimizer too
    model = copy.deepcopy(gpu_vsr)
    model.train()
    stock = torch.optim.Adam(model.parameters(), lr=1e-3)
    _, loss = driver.train_step(model, stock, x, y, high_frame, None)
    assert loss.requires_grad and float(loss) > 0 and len(stock.state) > 0
