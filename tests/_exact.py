"""Exact-arithmetic test cases: operands on which every kernel route must equal a float64 evaluation BIT FOR BIT.

If activations, weights and biases are small integers (or dyadic fractions: multiples of a power of two `g`), every product and
every partial sum of a convolution is a multiple of g*g below 2^24 g*g and therefore a float32 value: the result does not depend
on summation order, split-K, tile shape, MFMA shape or wave assignment.  If every value that a kernel stores as fp16 is an fp16
value as well, fp16 storage does not round either.  Inside that budget a kernel equals the float64 CPU evaluation exactly, and one
wrong element anywhere is a hard failure with coordinates instead of a fraction of a range-relative bar.

This module holds
  * seeded operand generators (`ints`, `sparse_weights`, `slopes`),
  * float64 references on stock torch.nn.functional operators, each CHECKING its budget (`conv_ref`, `deconv_ref`, `stage_ref`, and for
    the two ends of the SR net `head_ref`, `chain_ref`, `fold_ref`, `tail_ref`, `bilinear_up_ref`, `fusion_ref`;
    `BudgetError` names the offending coordinate: a case outside its budget is a mistake in the test, never a reason for a tolerance),
  * float64 references of the train step's GRADIENTS by autograd over the same stock operators (`grads_ref`, `prelu_grads_ref`,
    `mlp_grads_ref`), every backward sum under the same budget,
  * the trunk glue: `osvos_head_ref` (OSVOS's four transposed convolutions, crops, concat and fuse as stock float64 operators, the budget
    of the FOLDED sum the kernel forms checked) and `nearest_resize_ref` (pure data movement: ATen's float32 nearest resize on the CPU),
  * `assert_exact` / `diff_mask` / `bbox`, which report the number of differing elements, the first one and their bounding box.

The sign of a zero is not compared (`-0.0 == +0.0`): `0 * negative` in a PReLU with slope 0 is -0.0 in one formulation and +0.0 in
another, and no consumer can tell.  Everything else is compared as bits.

What these cases cannot see is rounding and overflow to infinity: no stored value ever needs either.  The ROUNDING cases at the end of
this module (`round_f16`, `act_round_ref`, `prelu_f16_ref`, `check_rounds`, the `*_round_ref` references; tests/_round_cases.py,
tests/test_gpu_rounding.py) keep the float32 budget, make the sums 13 to 15 bits wide and require the one round-to-nearest-even
fp16 value of each, again bit for bit.
"""
import numpy as np
import torch
import torch.nn.functional as F

MAX_THREADS = 16

SLOPES_LE_ONE = (0.0, 0.25, 0.5, 1.0)   # the `max(v, a v)` builds
SLOPES_SELECT = (2.0, -0.5)             # the select builds (`v < 0 ? a v : v`)


class BudgetError(Exception):
    """The case leaves the exact regime (a test-construction error)."""


def _threads():
    if torch.get_num_threads() > MAX_THREADS:
        torch.set_num_threads(MAX_THREADS)


# ---------------------------------------------------------------------------------------------------------------- operands
def ints(rs, shape, lo=-3, hi=3, step=1.0):
    """Values step * {lo..hi}, float64 tensor (step = 1: integers; step = 0.25: the dyadic regime)."""
    return torch.from_numpy(rs.randint(lo, hi + 1, size=shape).astype(np.float64) * step)


def sparse_weights(rs, shape, density=0.2, mag=2, step=1.0):
    """Weights step * {-mag..mag} \\ {0} on a `density` share of the elements, zero elsewhere."""
    v = rs.randint(1, mag + 1, size=shape) * (rs.randint(0, 2, size=shape) * 2 - 1)
    keep = rs.random_sample(size=shape) < density
    return torch.from_numpy((v * keep).astype(np.float64) * step)


def slopes(rs, n, pool=SLOPES_LE_ONE):
    return [float(pool[i]) for i in rs.randint(0, len(pool), size=n)]


def granularity(*tensors):
    """The largest power of two of which every element of every tensor is a multiple (1.0 for integers)."""
    g = 1.0
    for t in tensors:
        if t is None:
            continue
        t = torch.as_tensor(t, dtype=torch.float64)
        while g > 2.0 ** -40 and bool((torch.remainder(t, g) != 0).any()):
            g /= 2
    return g


# ---------------------------------------------------------------------------------------------------------------- checks
def _coord(mask):
    idx = torch.nonzero(mask)
    return tuple(int(i) for i in idx[0])


def check_sum_budget(abs_sum, gran, what):
    """abs_sum = sum |x| |w| + |b| per output; every partial sum in every order is a multiple of `gran` of magnitude <= abs_sum, so it is a
    float32 value when abs_sum < 2^24 gran."""
    bad = abs_sum >= (2.0 ** 24) * gran
    if bool(bad.any()):
        c = _coord(bad)
        raise BudgetError(f"{what}: sum |x||w| + |b| = {float(abs_sum[c])} at {c} is not below 2^24 * {gran}: partial sums may round in float32")


def check_storable(t, dtype, what):
    """Every element survives float64 -> dtype -> float64."""
    bad = t.to(dtype).to(torch.float64) != t
    if bool(bad.any()):
        c = _coord(bad)
        raise BudgetError(f"{what}: {float(t[c])!r} at {c} is not a {str(dtype).replace('torch.', '')} value (stored it becomes "
                          f"{float(t.to(dtype)[c])!r})")
    return t


def check_live(t, what, min_nonzero=0.5, min_distinct=200, both_signs=True):
    """The case is not degenerate: a share of the values non-zero, both signs present, a few hundred distinct values."""
    nz = float((t != 0).double().mean())
    if nz < min_nonzero:
        raise BudgetError(f"{what}: only {nz:.0%} of the values are non-zero (minimum {min_nonzero:.0%})")
    if both_signs and not (bool((t > 0).any()) and bool((t < 0).any())):
        raise BudgetError(f"{what}: one sign only")
    nd = int(torch.unique(t).numel())
    if nd < min(min_distinct, t.numel() // 8):
        raise BudgetError(f"{what}: {nd} distinct values (minimum {min(min_distinct, t.numel() // 8)})")
    return t


# ---------------------------------------------------------------------------------------------------------------- references
def local_granularity(x, w, stride=1, padding=0):
    """Per OUTPUT of conv2d(x, w): the granule of the finest input element that a non-zero weight of that output reads (1.0 where all of
    them are integers or the output reads nothing), times granularity(w).  A map whose small values carry fine granules beside large
    coarse ones (a rounded map behind a slope such as fp16(0.2)) has a global granularity far below what any one sum needs."""
    nz = (w != 0).to(torch.float64)
    g = torch.ones_like(F.conv2d(x, nz, None, stride=stride, padding=padding))
    step = 1.0
    for _ in range(40):
        need = torch.remainder(x, step) != 0          # elements finer than `step`
        if not bool(need.any()):
            break
        step /= 2
        g = torch.where(F.conv2d(need.to(torch.float64), nz, None, stride=stride, padding=padding) > 0, torch.full_like(g, step), g)
    return g * granularity(w)


def conv_ref(x, w, b=None, stride=1, padding=0, what="conv", store=None, local=False):
    """float64 conv2d of exact operands (all float64 tensors), its float32 budget checked; `store`: a dtype the result must fit.
    `local`: the budget per output on `local_granularity` instead of the granularity of the whole map."""
    _threads()
    y = F.conv2d(x, w, b, stride=stride, padding=padding)
    a = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), stride=stride, padding=padding)
    if local:
        g = local_granularity(x, w, stride, padding)
        g = g if b is None else torch.minimum(g, torch.full_like(g, granularity(b)))
        bad = a >= (2.0 ** 24) * g
        if bool(bad.any()):
            c = _coord(bad)
            raise BudgetError(f"{what}: sum |x||w| + |b| = {float(a[c])} at {c} is not below 2^24 * {float(g[c])}: partial sums may round in float32")
        return y if store is None else check_storable(y, store, what)
    check_sum_budget(a, granularity(x) * granularity(w) if b is None else min(granularity(x) * granularity(w), granularity(b)), what)
    if store is not None:
        check_storable(y, store, what)
    return y


def deconv_ref(x, w, b=None, stride=1, padding=0, what="deconv", store=None):
    """float64 conv_transpose2d (w [Cin, Cout, k, k]) of exact operands, its float32 budget checked."""
    _threads()
    y = F.conv_transpose2d(x, w, b, stride=stride, padding=padding)
    a = F.conv_transpose2d(x.abs(), w.abs(), None if b is None else b.abs(), stride=stride, padding=padding)
    check_sum_budget(a, granularity(x) * granularity(w) if b is None else min(granularity(x) * granularity(w), granularity(b)), what)
    if store is not None:
        check_storable(y, store, what)
    return y


def prelu_ref(v, slope):
    """v > 0 ? v : slope v, float64 (one slope for all channels, as every PReLU of the SR net)."""
    return torch.where(v > 0, v, v * float(slope))


def leaky_tenth_f16(v):
    """LeakyReLU with the product's default slope 0.1, which is not dyadic: the reference restates the kernel's own operation
    (csrc/conv_igemm.hip `fmaxf(x, 0) + nslope * fminf(x, 0)` / `t >= 0 ? t : t * p.slope`, csrc/conv_tile.hip:187, conv_patch.h:36;
    csrc/flow_ops.hip k_corr_mfma `s > 0 ? s : 0.1f * s`): the exact sum (a float32 value by the budget), ONE float32 multiply by
    float32(0.1) on the negative side -- for a negative x the other summand is +0, so a fused multiply-add gives the same --
    and one round-to-nearest-even to fp16 (`act_round_ref` with slope 0.1).  -> float64 tensor of fp16 values."""
    return act_round_ref(v, 2, 0.1)


def leaky_tenth_f32(v):
    """The float32 routes' LeakyReLU 0.1: one float32 multiply on the negative side (csrc/conv_f32_nchw.hip epilogue)."""
    x = check_storable(v, torch.float32, "leaky 0.1 input").to(torch.float32)
    return torch.where(x >= 0, x, x * torch.tensor(0.1, dtype=torch.float32)).to(torch.float64)


def act_ref(v, act, slope=0.1, store=torch.float16):
    """act: 0 none, 1 ReLU, 2 LeakyReLU(slope) as igemm.ACT_*; the result checked to fit `store`."""
    if act == 0:
        y = v
    elif act == 1:
        y = F.relu(v)
    elif slope == 0.1:
        return leaky_tenth_f16(v) if store == torch.float16 else leaky_tenth_f32(v)
    else:
        y = F.leaky_relu(v, slope)
    return check_storable(y, store, f"activation {act} output")


def stage_ref(a, up_w, up_b, up_a, dt_w, dt_b, dt_a, dn_w, dn_b, dn_a, S, live=True, min_distinct=200):
    """One FeedbackBlock stage in float64: ConvTranspose2d(k S+4, s S, p 2) -> PReLU -> the live 32-column slice of the downtran 1x1
    -> PReLU -> Conv2d(k S+4, s S, p 2) -> PReLU.  a [N,32,h,w]; up_w [32,32,k,k] (in, out); dt_w [32,32] (out, in: the slice);
    dn_w [32,32,k,k] (out, in).  The fused kernels convert the two inner sums to fp16 FIRST and apply PReLU on packed fp16 values with an
    fp16 slope (csrc/sr_f16_common.h); the output sum takes its PReLU in float32 and is converted behind it.  In the exact regime both
    orders agree: each of the three sums and each of the three PReLU results is checked to be an fp16 value, and the slopes too
    (`stage_round_ref` tells the orders apart).  -> dict(hr, t, out) of float64 maps."""
    for s in (up_a, dt_a, dn_a):
        check_storable(torch.tensor([float(s)], dtype=torch.float64), torch.float16, "PReLU slope")
    k = S + 4
    hr0 = deconv_ref(a, up_w, up_b, stride=S, padding=2, what="stage deconvolution", store=torch.float16)
    hr = check_storable(prelu_ref(hr0, up_a), torch.float16, "stage deconvolution after PReLU")
    t0 = conv_ref(hr, dt_w.reshape(32, 32, 1, 1), dt_b, what="stage downtran 1x1", store=torch.float16)
    t = check_storable(prelu_ref(t0, dt_a), torch.float16, "stage downtran after PReLU")
    o0 = conv_ref(t, dn_w, dn_b, stride=S, padding=2, what="stage strided convolution", store=torch.float16)
    out = check_storable(prelu_ref(o0, dn_a), torch.float16, "stage output after PReLU")
    assert dn_w.shape[-1] == k and up_w.shape[-1] == k
    if live:
        check_live(hr0, "stage deconvolution sum", min_distinct=4)      # (the intermediates: both signs before every PReLU)
        check_live(t0, "stage downtran sum", min_distinct=4)
        check_live(o0, "stage strided-convolution sum", min_distinct=min_distinct)
    return dict(hr=hr, t=t, out=out)


# ---------------------------------------------------------------------------------------------------------------- the SR net's two ends
def _slope_ok(*slopes, dtype=torch.float16):
    for s in slopes:
        check_storable(torch.tensor([float(s)], dtype=torch.float64), dtype, "PReLU slope")


def bilinear_up_ref(x, S, what="bilinear skip"):
    """ATen upsample_bilinear2d with align_corners=False as the fusion kernels restate it (csrc/sr_scale.hip `bil`, `lerp4`): source
    coordinate (dst + 0.5) / S - 0.5 clamped at 0, taps i0 = floor and i1 = min(i0 + 1, n - 1), weights (1 - l, l) with l = src - i0;
    x [N,C,h,w] float64 -> [N,C,Sh,Sw].  For S = 2 and 4 the weights are k/4 and k/8: every product and sum of the kernel is a multiple
    of gran(x) / (2S)^2 and exact in float32 when max|x| is below 2^24 of those (checked).  Any other S has no exact regime."""
    if S not in (2, 4):
        raise BudgetError(f"{what}: the bilinear weights of factor {S} are not dyadic; no exact regime (restate the kernel's float32 arithmetic instead)")
    N, C, h, w = x.shape

    def taps(n):
        src = ((torch.arange(S * n, dtype=torch.float64) + 0.5) / S - 0.5).clamp(min=0.0)
        i0 = src.floor().long()
        return i0, torch.where(i0 < n - 1, i0 + 1, i0), src - i0.double()

    y0, y1, ly = taps(h)
    x0, x1, lx = taps(w)
    g = granularity(x) / (2 * S) ** 2
    if x.numel() and float(x.abs().max()) >= (2.0 ** 24) * g:
        raise BudgetError(f"{what}: max |x| = {float(x.abs().max())} is not below 2^24 * {g}: a lerp may round in float32")
    lx, ly = lx.view(1, 1, 1, -1), ly.view(1, 1, -1, 1)
    rows0, rows1 = x[:, :, y0], x[:, :, y1]
    top = lx * rows0[..., x1] + (1.0 - lx) * rows0[..., x0]
    bot = lx * rows1[..., x1] + (1.0 - lx) * rows1[..., x0]
    return check_storable(ly * bot + (1.0 - ly) * top, torch.float32, what)


def tail_ref(hid, out_w, out_b, out_a, cv_w, cv_b, S, live=True):
    """The tail in float64: `out` ConvTranspose2d(k S+4, s S, p 2) -> fp16 -> PReLU -> fp16 -> conv_out 3x3 (32 -> 3) + bias in float32.
    hid [N,32,h,w]; out_w [32,32,k,k] (in, out); cv_w [3,32,3,3].  -> dict(hr, raw [N,3,Sh,Sw], dec = raw[..., ::S, ::S])."""
    _slope_ok(out_a)
    assert out_w.shape[-1] == S + 4 and tuple(cv_w.shape) == (3, 32, 3, 3)
    check_storable(cv_w, torch.float16, "conv_out weight (fp16 fragments)")
    hr0 = deconv_ref(hid, out_w, out_b, stride=S, padding=2, what="tail deconvolution", store=torch.float16)
    hr = check_storable(prelu_ref(hr0, out_a), torch.float16, "tail deconvolution after PReLU")
    raw = conv_ref(hr, cv_w, cv_b, padding=1, what="conv_out", store=torch.float32)
    if live:
        check_live(hr0, "tail deconvolution sum", min_distinct=4)
        check_live(raw, "conv_out sum", min_distinct=50)
    return dict(hr=hr, raw=raw, dec=raw[..., ::S, ::S].contiguous())


def fold_ref(lr_a, lr_b, cmap, co_w, co_b, co_a, live=True):
    """The FeedbackBlock's last compress_out as the FOLD tails apply it: 1x1 over two LR maps (co_w [32,64]: columns 0..31 read lr_a,
    32..63 lr_b) + bias + the constant map cmap [32,h,w] (float32) -> fp16 -> PReLU -> fp16.  -> hid [N,32,h,w]."""
    _slope_ok(co_a)
    check_storable(cmap, torch.float32, "constant map")
    x = torch.cat((lr_a, lr_b), 1)
    s0 = conv_ref(x, co_w.reshape(32, 64, 1, 1), co_b, what="compress_out")
    a = F.conv2d(x.abs(), co_w.abs().reshape(32, 64, 1, 1), co_b.abs()) + cmap.abs().unsqueeze(0)
    check_sum_budget(a, min(granularity(x) * granularity(co_w), granularity(co_b), granularity(cmap)), "compress_out + constant map")
    s0 = check_storable(s0 + cmap.unsqueeze(0), torch.float16, "compress_out sum")
    if live:
        check_live(s0, "compress_out sum", min_distinct=4)
    return check_storable(prelu_ref(s0, co_a), torch.float16, "compress_out after PReLU")


def chain_ref(stages, live=True):
    """Up to three chained 32-channel 1x1 stages (csrc/sr_f16.hip k_chain1x1_h).  Each stage: dict(ins=[(x [N,32,P], w [32,32])...],
    prev=w [32,32] or None (reads the previous stage's output), bias [32], cmap [32,P] float32 or None, slope).  The sum (float32) is
    stored as fp16, PReLU is applied on fp16 values, the result is an fp16 value.  -> list of outputs [N,32,P]."""
    _threads()
    outs, last = [], None
    for s, st in enumerate(stages):
        _slope_ok(st["slope"])
        terms = list(st["ins"]) + ([(last, st["prev"])] if st.get("prev") is not None else [])
        if not terms or (st.get("prev") is not None and last is None):
            raise ValueError(f"stage {s} has no input")
        acc = st["bias"].view(1, 32, 1).clone()
        mag = st["bias"].abs().view(1, 32, 1).clone()
        gran = granularity(st["bias"])
        if st.get("cmap") is not None:
            check_storable(st["cmap"], torch.float32, f"stage {s} constant map")
            acc, mag, gran = acc + st["cmap"].unsqueeze(0), mag + st["cmap"].abs().unsqueeze(0), min(gran, granularity(st["cmap"]))
        for x, w in terms:
            check_storable(w, torch.float16, f"stage {s} weight (fp16 fragments)")
            check_storable(x, torch.float16, f"stage {s} input")
            acc = acc + torch.einsum("oc,ncp->nop", w, x)
            mag = mag + torch.einsum("oc,ncp->nop", w.abs(), x.abs())
            gran = min(gran, granularity(x) * granularity(w))
        check_sum_budget(mag, gran, f"chain stage {s}")
        check_storable(acc, torch.float16, f"chain stage {s} sum")
        if live:
            check_live(acc, f"chain stage {s} sum", min_distinct=4)
        last = check_storable(prelu_ref(acc, st["slope"]), torch.float16, f"chain stage {s} after PReLU")
        outs.append(last)
    return outs


def head_ref(x, sub, w_in, b_in, a_in, w_feat, b_feat, a_feat, store=torch.float16, live=True):
    """The head in float64: sub_mean (x * scale + bias per channel, sub = (scale [3], bias [3])) -> zero padding -> conv_in 3x3
    (3 -> 128) + bias -> PReLU -> feat_in 1x1 (128 -> 32) + bias -> PReLU.  k_head_h (store = fp16) converts the mean-shifted
    pixels and both weight tensors to fp16 for the matrix cores, and each of the two sums to fp16 BEFORE its PReLU (act_pack /
    prelu_h2 on packed fp16 with an fp16 slope): the shifted pixels, both sums and both PReLU results must be values of `store`.
    The float32 head (store = float32) keeps float32 throughout.  x [N,3,h,w], w_in [128,3,3,3], w_feat [32,128] -> [N,32,h,w]."""
    _slope_ok(a_in, a_feat, dtype=store)
    s, b = sub
    t = check_storable(x * s.view(1, 3, 1, 1) + b.view(1, 3, 1, 1), store, "mean-shifted pixels")
    if store == torch.float16:
        check_storable(w_in, store, "conv_in weight (fp16 fragments)")
        check_storable(w_feat, store, "feat_in weight (fp16 fragments)")
    m0 = conv_ref(t, w_in, b_in, padding=1, what="conv_in", store=store)
    mid = check_storable(prelu_ref(m0, a_in), store, "conv_in after PReLU")
    f0 = conv_ref(mid, w_feat.reshape(32, -1, 1, 1), b_feat, what="feat_in", store=store)
    if live:
        check_live(m0, "conv_in sum", min_distinct=4)
        check_live(f0, "feat_in sum", min_distinct=50)
    return check_storable(prelu_ref(f0, a_feat), store, "feat_in after PReLU")


def planes_ref(raw, x, sub, add, S, decimate=False):
    """What the fusion MLP reads: (bilinear xS of sub_mean(x) + raw) * add_scale + add_bias per plane and channel, every float32
    operation of it exact.  raw [N,3,Sh,Sw] (or [N,3,h,w] with `decimate`: the pixels (S i, S j)); x [N,3,h,w].  -> like raw."""
    (ss, sb), (as_, ab) = sub, add
    t = check_storable(x * ss.view(1, 3, 1, 1) + sb.view(1, 3, 1, 1), torch.float32, "mean-shifted pixels")
    skip = bilinear_up_ref(t, S)
    if decimate:
        skip = skip[..., ::S, ::S]
    v = check_storable(skip + raw, torch.float32, "skip + raw")
    check_storable(v * as_.view(1, 3, 1, 1), torch.float32, "(skip + raw) * add_scale")
    return check_storable(v * as_.view(1, 3, 1, 1) + ab.view(1, 3, 1, 1), torch.float32, "plane after add_mean")


def mlp_ref(planes, fc, live=True):
    """The fusion MLP over the plane axis: relu(w2 . relu(W1 v + b1) + b2), v = planes[:, c, y, x].  fc = (w1 [hidden, n], b1, w2 [hidden],
    b2 [1]); both sums inside the float32 budget in any order.  planes [n,3,H,W] -> [1,3,H,W]."""
    _threads()
    w1, b1, w2, b2 = fc
    h0 = torch.einsum("jn,ncyx->jcyx", w1, planes) + b1.view(-1, 1, 1, 1)
    a0 = torch.einsum("jn,ncyx->jcyx", w1.abs(), planes.abs()) + b1.abs().view(-1, 1, 1, 1)
    g1 = min(granularity(w1) * granularity(planes), granularity(b1))
    check_sum_budget(a0, g1, "fusion MLP layer 1")
    hid = F.relu(h0)
    o0 = torch.einsum("j,jcyx->cyx", w2, hid) + b2.view(1, 1, 1)
    a1 = torch.einsum("j,jcyx->cyx", w2.abs(), hid) + b2.abs().view(1, 1, 1)
    check_sum_budget(a1, min(granularity(w2) * g1, granularity(b2)), "fusion MLP layer 2")
    if live:
        check_live(h0, "fusion MLP hidden sum", min_distinct=50)
        check_live(o0, "fusion MLP output sum", min_distinct=50)
    return check_storable(F.relu(o0), torch.float32, "fused frame").unsqueeze(0)


def fusion_ref(raw, x, sub, add, fc, S, decimate=False, live=True):
    """Skip + add_mean + fusion MLP on the raw planes (vsr_sr_fc_planes_skip_f32 and its siblings): `planes_ref` then `mlp_ref`.
    Choose the MeanShift values dyadic (mean (0.5, 0.25, 0.375), std 1: 255 * mean is a multiple of 1/8) and the MLP's weights small
    integers or eighths, so that every float32 product and sum is exact in any order."""
    return mlp_ref(planes_ref(raw, x, sub, add, S, decimate), fc, live=live)


# ---------------------------------------------------------------------------------------------------------------- the train step's gradients
def grads_ref(fn, operands, gy, what="operator"):
    """Forward and every gradient of a multilinear stock operator in float64.  `fn`: a closure over F.conv2d / F.conv_transpose2d taking
    the operands (float64 tensors, e.g. x, w, b) in order; `gy`: the incoming gradient.  -> (y, [gradient per operand]).
    The same `fn` on |operands| with |gy| gives, for such an operator, exactly the sum of |terms| of every forward and backward sum; each
    is held below 2^24 of the product of all granularities (a multiple of which every term of every sum is), so float32 evaluates all of
    them without rounding in any order."""
    _threads()
    gran = granularity(gy)
    for t in operands:
        gran *= granularity(t)

    def run(ops, g):
        leaves = [t.detach().clone().requires_grad_() for t in ops]
        y = fn(*leaves)
        return y.detach(), [t.detach() for t in torch.autograd.grad(y, leaves, g)]

    y, grads = run(operands, gy)
    ya, ga = run([t.abs() for t in operands], gy.abs())
    check_sum_budget(ya, gran, f"{what} forward")
    for i, a in enumerate(ga):
        check_sum_budget(a, gran, f"{what} gradient of operand {i}")
    return y, grads


def prelu_grads_ref(v, g, slope, what="PReLU backward"):
    """gv = g where v > 0, else g * slope; dslope = sum g * min(v, 0): ATen's conventions (v == 0 is on the slope side).
    -> (gv, dslope [1]), float64.  sum |g||v| below 2^24 granularities: the slope gradient is exact in any order; gv a float32 value."""
    _slope_ok(slope, dtype=torch.float32)
    gv = check_storable(torch.where(v > 0, g, g * float(slope)), torch.float32, f"{what}: input gradient")
    check_sum_budget((g.abs() * v.abs()).sum().reshape(1), granularity(g) * granularity(v), f"{what}: slope gradient")
    return gv, (g * v.clamp(max=0.0)).sum().reshape(1)


def mlp_grads_ref(planes, fc, go, live=True):
    """Gradients of `mlp_ref`'s formulation relu(w2 . relu(W1 v + b1) + b2) by float64 autograd (a ReLU passes nothing at 0).  planes
    [n,3,H,W], fc = (w1 [hidden, n], b1, w2 [hidden], b2 [1]), go [1,3,H,W] -> dv [n,3,H,W], dW1 [hidden, n], db1, dw2 [hidden], db2 [1].
    The forward budget is `mlp_ref`'s; each of the five backward sums is held below 2^24 granularities by its absolute-value counterpart."""
    mlp_ref(planes, fc, live=live)
    leaves = [t.detach().clone().requires_grad_() for t in (planes,) + tuple(fc)]
    v, w1, b1, w2, b2 = leaves
    hs = torch.einsum("jn,ncyx->jcyx", w1, v) + b1.view(-1, 1, 1, 1)
    hid = F.relu(hs)
    out = F.relu(torch.einsum("j,jcyx->cyx", w2, hid) + b2.view(1, 1, 1)).unsqueeze(0)
    grads = [t.detach() for t in torch.autograd.grad(out, leaves, go)]
    with torch.no_grad():
        w1a, w2a, va = fc[0].abs(), fc[2].abs(), planes.abs()
        ago = go[0].abs() * (out[0] > 0)                                     # |go| behind the output gate [3,H,W]
        agh = ago.unsqueeze(0) * w2a.view(-1, 1, 1, 1) * (hs > 0)            # |gh| [hidden,3,H,W]
        g_go, g_gh = granularity(go), granularity(go) * granularity(fc[2])
        g_hid = min(granularity(fc[0]) * granularity(planes), granularity(fc[1]))
        check_storable(agh, torch.float32, "fusion MLP hidden gradient")
        check_sum_budget(torch.einsum("jcyx,jn->ncyx", agh, w1a), g_gh * granularity(fc[0]), "fusion MLP dv")
        check_sum_budget(torch.einsum("jcyx,ncyx->jn", agh, va), g_gh * granularity(planes), "fusion MLP dW1")
        check_sum_budget(agh.sum((1, 2, 3)), g_gh, "fusion MLP db1")
        check_sum_budget(torch.einsum("cyx,jcyx->j", ago, hid.detach()), g_go * g_hid, "fusion MLP dw2")
        check_sum_budget(ago.sum().reshape(1), g_go, "fusion MLP db2")
    return grads


# ---------------------------------------------------------------------------------------------------------------- the trunk glue
def osvos_sizes(h, w, nbranch=4):
    """Side-map sizes of an h x w frame: MaxPool2d(2, 2, ceil_mode=True) once per VGG stage, branch b behind b + 1 of them."""
    out = []
    for _ in range(nbranch):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def osvos_head_ref(sides, up_w, fuse_w, bias, hw, dweff=None, live=True):
    """OSVOS's head in float64 as vos.OSVOS.forward words it: per branch F.conv_transpose2d(side_b, up_b, stride = k_b / 2) -> centre crop
    to hw (vos._center_crop) -> cat -> F.conv2d with the fuse row + bias.  sides [N,16,hs_b,ws_b], up_w [16 (in),16 (out),k_b,k_b], fuse_w
    [16 nb], bias a number -> [N,1,h,w].
    The kernel does not evaluate that composition: it sums side * weff over 2 x 2 source pixels x 16 channels per branch, with
    weff_b[ci][ky][kx] = sum_co fuse[16 b + co] * up_b[ci][co][ky][kx] stored as fp16.  So the budget is the folded sum's: every side
    value and every folded weight an fp16 value, and sum |side| |weff| + |bias| (the folded weights as 16 -> 1 transposed convolutions of
    |side|, cropped alike) below 2^24 granularities.
    `dweff`: per branch None or a [16,1,k_b,k_b] term ADDED to the folded weight (a planted defect): its own transposed convolution is
    added to the result and enters both budget checks."""
    from video_super_resolution_amd.vos import _center_crop
    _threads()
    h, w = hw
    nb = len(sides)
    assert len(up_w) == nb and fuse_w.numel() == 16 * nb
    ups, mags, gran = [], [], granularity(torch.tensor([float(bias)], dtype=torch.float64))
    extra = torch.zeros((sides[0].shape[0], 1, h, w), dtype=torch.float64)
    for b in range(nb):
        s = up_w[b].shape[-1] // 2
        assert tuple(up_w[b].shape) == (16, 16, 2 * s, 2 * s) and sides[b].shape[1] == 16
        check_storable(sides[b], torch.float16, f"side map {b}")
        ups.append(_center_crop(F.conv_transpose2d(sides[b], up_w[b], stride=s), h, w))
        weff = torch.einsum("iokl,o->ikl", up_w[b], fuse_w[16 * b:16 * b + 16]).unsqueeze(1)      # [16,1,k,k]: for the budget only
        if dweff is not None and dweff[b] is not None:
            extra = extra + _center_crop(F.conv_transpose2d(sides[b], dweff[b], stride=s), h, w)
            weff = weff + dweff[b]
        check_storable(weff, torch.float16, f"folded weight of branch {b}")
        mags.append(_center_crop(F.conv_transpose2d(sides[b].abs(), weff.abs(), stride=s), h, w))
        gran = min(gran, granularity(sides[b]) * granularity(weff))
        if tuple(ups[-1].shape[2:]) != (h, w):
            raise BudgetError(f"branch {b}: a {tuple(sides[b].shape[2:])} side map upsamples to less than {h}x{w}")
    check_sum_budget(sum(mags) + abs(float(bias)), gran, "OSVOS head")
    out = F.conv2d(torch.cat(ups, 1), fuse_w.reshape(1, 16 * nb, 1, 1), torch.tensor([float(bias)], dtype=torch.float64)) + extra
    if live:
        check_live(out, "OSVOS head sum", min_distinct=50)
    return check_storable(out, torch.float32, "OSVOS logit")


def nearest_resize_ref(x, size):
    """F.interpolate(x, size) in its default mode (nearest) on the CPU in FLOAT32: pure data movement, so the values come back in x's
    dtype unchanged.  float32 on purpose: ATen forms the source index as floor(dst * (in / out)) in the tensor's compute type, which is
    what the kernels restate; at some sizes (26 -> 22, 14 -> 46, 21 -> 69 among them) that is not the rational floor(dst * in / out), and
    an operator computing its scale in double need not agree either.  x [N,C,H,W]."""
    y = F.interpolate(x.detach().cpu().to(torch.float32), size=tuple(size))
    return y.to(x.dtype)


def nearest_sources(n_in, n_out, dtype=torch.float32):
    """The source index per destination index that ATen's nearest resize picks along one axis, read off the operator itself."""
    ramp = torch.arange(n_in, dtype=dtype).view(1, 1, n_in, 1)
    return F.interpolate(ramp, size=(n_out, 1))[0, 0, :, 0].long()


def nearest_differs_from_rational(n_in, n_out):
    """True where the float32 operator's source differs from floor(dst * n_in / n_out) in integers, at one destination or more."""
    exact = (torch.arange(n_out, dtype=torch.int64) * n_in) // n_out
    return bool((nearest_sources(n_in, n_out) != exact).any())


# ---------------------------------------------------------------------------------------------------------------- rounding cases
# The float32 budget above, WITHOUT the requirement that stored values are fp16 values: the float32 sum is still exact in any order,
# and what a kernel stores is the one round-to-nearest-even of it.  One right answer per element, no tolerance.
def _f16_parts(t, what="value"):
    """|t| = (q + rem / 2^s) * 2^qexp with integers q, 0 <= rem < 2^s, where 2^qexp is the fp16 spacing at |t| (2^(e-11) for a
    normal result, 2^-24 below 2^-14: gradual underflow).  t: float64 tensor of finite float32 values (checked), so that the
    significand M = |t| / 2^(e-24) is an integer below 2^24.  -> (q, rem, half = 2^(s-1), qexp), int64 tensors."""
    t = torch.as_tensor(t, dtype=torch.float64)
    if not bool(torch.isfinite(t).all()):
        raise BudgetError(f"{what}: not finite at {_coord(~torch.isfinite(t))}")
    check_storable(t, torch.float32, what)
    mant, e = torch.frexp(t.abs())                      # |t| = mant * 2^e, mant in [0.5, 1) (0, 0 for zero)
    m = mant * 2.0 ** 24
    mi = m.to(torch.int64)
    if bool((mi.to(torch.float64) != m).any()):
        raise BudgetError(f"{what}: {float(t[_coord(mi.to(torch.float64) != m)])!r} has more than 24 significant bits")
    e = e.to(torch.int64)
    qexp = torch.clamp(e - 11, min=-24)
    s = torch.clamp(qexp - (e - 24), max=40)            # 13 for a normal result; beyond 25 everything is remainder below the half
    q = mi >> s
    rem = mi - (q << s)
    half = torch.ones_like(s) << (s - 1)
    return q, rem, half, qexp


def _round_parts(t, up_rule, overflow, what):
    q, rem, half, qexp = _f16_parts(t, what)
    n = q + up_rule(q, rem, half).to(torch.int64)
    r = n.to(torch.float64) * torch.pow(torch.full_like(n, 2.0, dtype=torch.float64), qexp.to(torch.float64))
    r = torch.where(r >= 65536.0, torch.full_like(r, overflow), r)
    return torch.where(torch.as_tensor(t, dtype=torch.float64) < 0, -r, r)


def round_f16(t, what="round_f16 input"):
    """The fp16 value nearest to each element, ties to the even significand (IEEE 754 roundTiesToEven), as float64: in integer
    arithmetic on the 24-bit significand (frexp, shift, half-to-even on the remainder), independent of any library cast.
    Magnitudes of 65520 and above give +-inf; below 2^-14 the spacing stays 2^-24 (gradual underflow).  t: float64 tensor whose
    elements are finite float32 values (checked)."""
    return _round_parts(t, lambda q, rem, half: (rem > half) | ((rem == half) & ((q & 1) == 1)), float("inf"), what)


def round_f16_alt(t, mode):
    """A WRONG fp16 rounding, to prove that a case tells it from `round_f16` -- never a reference.  "rtz": truncation (what a
    v_cvt_pkrtz-style conversion does; a finite overflow stays 65504); "away": ties away from zero."""
    if mode == "rtz":
        return torch.clamp(_round_parts(t, lambda q, rem, half: torch.zeros_like(q, dtype=torch.bool), 65504.0, "round_f16_alt input"), -65504.0, 65504.0)
    if mode == "away":
        return _round_parts(t, lambda q, rem, half: rem >= half, float("inf"), "round_f16_alt input")
    raise ValueError(mode)


def rounding_profile(pre):
    """Masks over `pre` (float64 tensor of float32 values): `inexact` (not an fp16 value), `tie` (exactly between two fp16 values),
    `tie_up` / `tie_down` (the tie goes to the neighbour of larger / smaller magnitude under nearest-even)."""
    q, rem, half, _ = _f16_parts(pre, "pre-rounding value")
    tie = rem == half
    return dict(inexact=rem != 0, tie=tie, tie_up=tie & ((q & 1) == 1), tie_down=tie & ((q & 1) == 0))


def check_rounds(pre, what, pool=None, min_inexact=0.25, min_ties=0.05, min_each=16):
    """The liveness condition of a rounding case, on the values about to be rounded to fp16: at least 25 % are not fp16 values, at
    least 5 % are exact ties, at least 16 ties resolve upward in magnitude and at least 16 downward, and no magnitude reaches 65520
    (overflow has its own cases).  A map below 512 elements cannot meet the counts alone: it is appended to `pool` (a list) instead,
    and the test calls `check_rounds_pool(pool, what)` once over all of its cases.  Conditions on the INPUTS, not tolerances."""
    pre = torch.as_tensor(pre, dtype=torch.float64)
    if bool((pre.abs() >= 65520.0).any()):
        raise BudgetError(f"{what}: |{float(pre[_coord(pre.abs() >= 65520.0)])}| at {_coord(pre.abs() >= 65520.0)} overflows fp16")
    if pool is not None:
        pool.append(pre.reshape(-1))
    if pre.numel() < 512:
        if pool is None:
            raise BudgetError(f"{what}: {pre.numel()} elements are too few for the rounding counts; pool the cases of the test")
        return pre
    p = rounding_profile(pre)
    n = pre.numel()
    fi, ft, nu, nd = int(p["inexact"].sum()) / n, int(p["tie"].sum()) / n, int(p["tie_up"].sum()), int(p["tie_down"].sum())
    if fi < min_inexact or ft < min_ties or nu < min_each or nd < min_each:
        raise BudgetError(f"{what}: {fi:.1%} of the values need rounding (minimum {min_inexact:.0%}), {ft:.1%} are ties (minimum {min_ties:.0%}), "
                          f"{nu} ties go up and {nd} down (minimum {min_each} each)")
    return pre


def check_rounds_pool(pool, what):
    """`check_rounds` over the small maps a test collected; the pool as a whole has to reach 512 elements."""
    allv = torch.cat(pool) if pool else torch.zeros(0, dtype=torch.float64)
    if allv.numel() < 512:
        raise BudgetError(f"{what}: the pooled cases hold {allv.numel()} elements, fewer than 512")
    return check_rounds(allv, what)


def act_f32(pre, act, slope=0.1):
    """The trunk activation as ONE float32 operation on a float32 value (act: 0 none, 1 ReLU, 2 Leaky: x >= 0 ? x : x * float32(slope)),
    not yet rounded to fp16.  -> float64 tensor of float32 values."""
    x = check_storable(torch.as_tensor(pre, dtype=torch.float64), torch.float32, "activation input").to(torch.float32)
    if act == 0:
        y = x
    elif act == 1:
        y = torch.clamp(x, min=0.0)
    else:
        y = torch.where(x >= 0, x, x * torch.tensor(float(slope), dtype=torch.float32))
    return y.to(torch.float64)


def act_round_ref(pre, act, slope=0.1):
    """The trunk kernels' epilogue order: the activation in float32 on the exact sum, THEN one round-to-nearest-even to fp16.
    act: 0 none, 1 ReLU, 2 LeakyReLU(slope) as igemm.ACT_*.  The activation restates csrc/conv_igemm.hip `fmaxf(x, 0) + nslope *
    fminf(x, 0)` / `t >= 0 ? t : t * p.slope`, csrc/conv_tile.hip:187 and conv_patch.h:36: on the negative side ONE float32 multiply
    by float32(slope), rounded to float32 (exact for a dyadic slope and a short sum, one rounding for 0.1), before the fp16 rounding.
    A contracted fma(nslope, min(x, 0), max(x, 0)) gives the same value, because one of the two addends is zero.
    pre: float64 tensor of float32 values (checked).  -> float64 tensor of fp16 values (+-inf from 65520)."""
    return round_f16(act_f32(pre, act, slope), "activation output")


def prelu_f16_ref(v16, slope, build="max"):
    """The SR kernels' PReLU on packed fp16 (csrc/sr_f16_common.h prelu_h2 / act_stage): the slope (any float32 parameter) rounded to
    fp16 by the packer, m = v * a rounded ONCE to fp16 (the exact product of two 11-bit significands has 22 bits: a float32 value),
    then `max(v, m)` in the builds for slopes <= 1 ("max"), `min(v, m)` for a slope above 1 ("min"), `v < 0 ? m : v` in the select
    builds ("select").  v16: float64 tensor of finite fp16 values (checked).  The sign of a zero is not compared, as elsewhere."""
    v16 = check_storable(torch.as_tensor(v16, dtype=torch.float64), torch.float16, "PReLU input")
    s32 = torch.tensor([float(slope)], dtype=torch.float32).to(torch.float64)
    a = float(round_f16(s32, "PReLU slope"))
    m = round_f16(v16 * a, "PReLU product")
    if build == "max":
        return torch.maximum(v16, m)
    if build == "min":
        return torch.minimum(v16, m)
    if build == "select":
        return torch.where(v16 < 0, m, v16)
    raise ValueError(build)


def store_f16(pre, slope, build, name=None):
    """What an SR kernel stores for a float32 sum: one rounding to fp16, then the packed-fp16 PReLU.  The `*_round_ref` references take a
    replacement (`store=`) so that tests/test_exact_helper.py can evaluate a case under a DEFECT and count what it moves; `name` tells the
    replacement which storage point it is at."""
    return prelu_f16_ref(round_f16(pre), slope, build)


def store_f32act(pre, slope, build, name=None):
    """What a fused stage stores for its OUTPUT sum (csrc/sr_utd4.hip red_stage, sr_utd_s2.hip reduce_store and their siblings: "slope
    multiply, max / select, 2 converts"): the PReLU in float32 with the float32 slope on the float32 sum, then ONE rounding to fp16 --
    `act_round_ref`.  The max form fmaxf(s, s a) and the select form s >= 0 ? s : s a give the same value for a <= 1."""
    return act_round_ref(pre, 2, slope)


def stage_round_ref(a, up_w, up_b, up_a, dt_w, dt_b, dt_a, dn_w, dn_b, dn_a, S, live=("up", "dt", "dn"), weights_f16=True, store=store_f16,
                    store_out=store_f32act):
    """`stage_ref` with rounding.  The two sums that stay inside the kernel (deconvolution, downtran 1x1) are rounded ONCE to fp16
    (`round_f16`) and their PReLU runs on the fp16 value with the fp16 slope and one fp16 rounding of the product (`prelu_f16_ref`); the
    OUTPUT sum takes its PReLU in float32 with the float32 slope and is rounded once behind it (`store_f32act`: the kernels' reduce
    stages).  The next layer reads those rounded values -- its float32
    budget checked on their actual granularity.  `live`: which of the three sums must meet `check_rounds` (none for a map of a few pixels).  -> dict(hr, t, out) plus
    the pre-rounding sums (hr0, t0, o0)."""
    b = "max" if all(float(s) <= 1.0 for s in (up_a, dt_a, dn_a)) else "select"      # (one flag per launch: csrc/sr_utd*.hip slopes_le_one)
    check_storable(a, torch.float16, "stage input")
    for w_ in (up_w, dt_w, dn_w) if weights_f16 else ():
        check_storable(w_, torch.float16, "stage weight (fp16 fragments)")
    hr0 = deconv_ref(a, up_w, up_b, stride=S, padding=2, what="stage deconvolution")
    hr = store(hr0, up_a, b, "up")
    t0 = conv_ref(hr, dt_w.reshape(32, 32, 1, 1), dt_b, what="stage downtran 1x1")
    t = store(t0, dt_a, b, "dt")
    o0 = conv_ref(t, dn_w, dn_b, stride=S, padding=2, what="stage strided convolution")
    out = store_out(o0, dn_a, b, "dn")
    for name, s0 in (("up", hr0), ("dt", t0), ("dn", o0)):
        if name in live:
            check_rounds(s0, f"stage {name} sum")
            check_live(s0, f"stage {name} sum", min_distinct=4)
    return dict(hr=hr, t=t, out=out, hr0=hr0, t0=t0, o0=o0)


def tail_round_ref(hid, out_w, out_b, out_a, cv_w, cv_b, S, live=True, local=False, store=store_f16):
    """`tail_ref` with rounding: the deconvolution sum rounds once to fp16, the fp16 PReLU (any float32 slope), then conv_out (float32
    output, no fp16 store) reads the rounded map inside its float32 budget (`local`: per output, see `conv_ref`)."""
    assert out_w.shape[-1] == S + 4 and tuple(cv_w.shape) == (3, 32, 3, 3)
    check_storable(hid, torch.float16, "tail input")
    check_storable(out_w, torch.float16, "tail weight (fp16 fragments)")
    check_storable(cv_w, torch.float16, "conv_out weight (fp16 fragments)")
    hr0 = deconv_ref(hid, out_w, out_b, stride=S, padding=2, what="tail deconvolution")
    if live:
        check_rounds(hr0, "tail deconvolution sum")
        check_live(hr0, "tail deconvolution sum", min_distinct=4)
    hr = store(hr0, out_a, "max" if float(out_a) <= 1.0 else "select", "out")
    raw = conv_ref(hr, cv_w, cv_b, padding=1, what="conv_out", store=torch.float32, local=local)
    if live:
        check_live(raw, "conv_out sum", min_distinct=50)
    return dict(hr=hr, hr0=hr0, raw=raw, dec=raw[..., ::S, ::S].contiguous())


def fold_round_ref(lr_a, lr_b, cmap, co_w, co_b, co_a, live=True, store=store_f16):
    """`fold_ref` with rounding: 1x1 over two LR maps + bias + the float32 constant map, ONE rounding to fp16, the fp16 PReLU.
    -> (hid, the pre-rounding sum)."""
    check_storable(cmap, torch.float32, "constant map")
    x = torch.cat((lr_a, lr_b), 1)
    check_storable(x, torch.float16, "compress_out input")
    check_storable(co_w, torch.float16, "compress_out weight (fp16 fragments)")
    s0 = conv_ref(x, co_w.reshape(32, 64, 1, 1), co_b, what="compress_out")
    a = F.conv2d(x.abs(), co_w.abs().reshape(32, 64, 1, 1), co_b.abs()) + cmap.abs().unsqueeze(0)
    check_sum_budget(a, min(granularity(x) * granularity(co_w), granularity(co_b), granularity(cmap)), "compress_out + constant map")
    s0 = s0 + cmap.unsqueeze(0)
    if live:
        check_rounds(s0, "compress_out sum")
    return store(s0, co_a, "max" if float(co_a) <= 1.0 else "select", "co"), s0


def chain_round_ref(stages, pool=None, live=True, store=store_f16):
    """`chain_ref` with rounding: every stage's float32 sum rounds once to fp16, PReLU on fp16 values (csrc/sr_f16.hip k_chain1x1_h
    takes the max form for a slope <= 1 and the min form above).  -> (outputs, pre-rounding sums)."""
    _threads()
    outs, pres, last = [], [], None
    for s, st in enumerate(stages):
        terms = list(st["ins"]) + ([(last, st["prev"])] if st.get("prev") is not None else [])
        if not terms or (st.get("prev") is not None and last is None):
            raise ValueError(f"stage {s} has no input")
        acc = st["bias"].view(1, 32, 1).clone()
        mag = st["bias"].abs().view(1, 32, 1).clone()
        gran = granularity(st["bias"])
        if st.get("cmap") is not None:
            check_storable(st["cmap"], torch.float32, f"stage {s} constant map")
            acc, mag, gran = acc + st["cmap"].unsqueeze(0), mag + st["cmap"].abs().unsqueeze(0), min(gran, granularity(st["cmap"]))
        for x, w in terms:
            check_storable(w, torch.float16, f"stage {s} weight (fp16 fragments)")
            check_storable(x, torch.float16, f"stage {s} input")
            acc = acc + torch.einsum("oc,ncp->nop", w, x)
            mag = mag + torch.einsum("oc,ncp->nop", w.abs(), x.abs())
            gran = min(gran, granularity(x) * granularity(w))
        check_sum_budget(mag, gran, f"chain stage {s}")
        if live:
            check_rounds(acc, f"chain stage {s} sum", pool=pool)
            check_live(acc, f"chain stage {s} sum", min_distinct=4)
        last = store(acc, st["slope"], "max" if float(st["slope"]) <= 1.0 else "min", f"s{s}")
        outs.append(last)
        pres.append(acc)
    return outs, pres


def head_round_ref(x, sub, w_in, b_in, a_in, w_feat, b_feat, a_feat, live=True, store=store_f16):
    """`head_ref` (fp16) with rounding: both sums of k_head_h round once to fp16 before their packed-fp16 PReLU.  The mean-shifted pixels
    stay fp16 values (that conversion has no sum behind it).  -> (out, conv_in sum, feat_in sum)."""
    s, b = sub
    t = check_storable(x * s.view(1, 3, 1, 1) + b.view(1, 3, 1, 1), torch.float16, "mean-shifted pixels")
    check_storable(w_in, torch.float16, "conv_in weight (fp16 fragments)")
    check_storable(w_feat, torch.float16, "feat_in weight (fp16 fragments)")
    m0 = conv_ref(t, w_in, b_in, padding=1, what="conv_in")
    if live:
        check_rounds(m0, "conv_in sum")
    mid = store(m0, a_in, "max" if float(a_in) <= 1.0 else "select", "in")
    f0 = conv_ref(mid, w_feat.reshape(32, -1, 1, 1), b_feat, what="feat_in")
    if live:
        check_rounds(f0, "feat_in sum")
    return store(f0, a_feat, "max" if float(a_feat) <= 1.0 else "select", "feat"), m0, f0


# ---------------------------------------------------------------------------------------------------------------- comparison
def _canon(t):
    t = t.detach().cpu()
    if t.is_floating_point():
        t = t + 0.0   # -0.0 -> +0.0
    return t.contiguous()


_INT_OF = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def diff_mask(got, want):
    """Boolean tensor: where the bits of `got` differ from `want` converted to got's dtype (the conversion is exact by the budget; it is
    checked here once more).  NaNs differ from everything, themselves included."""
    got = _canon(got)
    want = want.detach().cpu()
    if tuple(got.shape) != tuple(want.shape):
        raise AssertionError(f"shape {tuple(got.shape)} against {tuple(want.shape)}")
    if want.dtype != got.dtype:
        check_storable(want.to(torch.float64), got.dtype, "reference in the output dtype")
    want = _canon(want.to(got.dtype))
    it = _INT_OF.get(got.dtype)
    m = (got.view(it) != want.view(it)) if it is not None else (got != want)
    if got.is_floating_point():
        m = m | torch.isnan(got) | torch.isnan(want)
    return m


def bbox(mask):
    """[(first, last)] per dimension of the True elements; None when there is none."""
    idx = torch.nonzero(mask)
    if idx.numel() == 0:
        return None
    return [(int(idx[:, d].min()), int(idx[:, d].max())) for d in range(idx.shape[1])]


def assert_exact(got, want, what, names="ncyx"):
    """Equality of bits.  The failure message gives the number of differing elements, the first one with got / want, and the bounding
    box of all of them per dimension (a tile seam, a strip edge or a channel chunk is visible from the message alone)."""
    m = diff_mask(got, want)
    n = int(m.sum())
    if n == 0:
        return
    c = _coord(m)
    g, w = _canon(got), want.detach().cpu()
    names = names if len(names) == m.dim() else "".join(chr(ord("a") + i) for i in range(m.dim()))
    box = ", ".join(f"{names[d]} {lo}..{hi}" for d, (lo, hi) in enumerate(bbox(m)))
    at = ", ".join(f"{names[d]}={c[d]}" for d in range(m.dim()))
    raise AssertionError(f"{what}: {n} of {m.numel()} elements differ from the float64 evaluation; first at ({at}): got {float(g[c])!r}, "
                         f"want {float(w[c])!r}; all inside [{box}]")


def nhwc(t, dtype=torch.float16, cp=None):
    """[N,C,H,W] float64 -> [N,H,W,cp] of dtype, zero padded (CPU tensor; exact by construction, checked)."""
    N, C, H, W = t.shape
    check_storable(t, dtype, "NHWC operand")
    out = torch.zeros((N, H, W, cp or C), dtype=dtype)
    out[..., :C] = t.permute(0, 2, 3, 1).to(dtype)
    return out


def nchw64(t, c=None):
    """[N,H,W,Cp] device tensor -> [N,c,H,W] CPU tensor of the same dtype."""
    t = t.detach().cpu()
    return t[..., :(c or t.shape[3])].permute(0, 3, 1, 2).contiguous()
