"""The rounding cases of tests/test_gpu_rounding.py, built without a GPU so that tests/test_exact_helper.py can run every reference,
budget, liveness condition and discrimination check on the CPU.

A case keeps the float32 budget of tests/_exact.py (sum |x||w| + |b| below 2^24 granules: the float32 sum is exact in any order) and
drops the requirement that the stored value is an fp16 value: inputs are integers up to +-255, weights sparse integers up to +-8 with
a density that puts the standard deviation of the sums near 2^13, biases up to +-2000.  Sums of 13 to 15 bits: more than half need
rounding to fp16's 11 bits, a fifth are exact ties.  `_exact.check_rounds` holds every case to that."""
import numpy as np
import torch

import _exact as E

NONE, RELU, LEAKY = 0, 1, 2                                          # igemm.ACT_*
ACTS = ((NONE, 0.1), (RELU, 0.1), (LEAKY, 0.75), (LEAKY, 0.1))        # none, ReLU, Leaky with a three-bit slope, Leaky 0.1
SIGMA = 8000.0

# ---------------------------------------------------------------------------------------------------------------- the case lists
GATHER = [(1, 33, 6, 11, 17, 3, 1, 1), (1, 65, 7, 5, 65, 1, 1, 0), (1, 32, 3, 43, 64, 3, 1, 1), (2, 128, 17, 13, 128, 5, 2, 2)]
SPLITK = [(1, 1026, 16, 16, 2, 3, 1, 1), (1, 473, 8, 16, 256, 3, 1, 1)]
TILE = [(1, 33, 11, 12, 65, 3, 1, 1), (1, 32, 8, 16, 64, 3, 1, 1), (2, 128, 17, 13, 128, 5, 2, 2)]
PATCH = [(1, 31, 5, 17, 13, 5), (1, 96, 13, 19, 17, 3), (1, 64, 17, 16, 32, 7), (2, 64, 8, 50, 129, 3)]      # stride 1, pad k // 2
ONE = [(1, 128, 241, 272, 208), (1, 96, 258, 255, 77)]      # 1x1 (N, cin, H, W, cout): the streaming builds serve 65536 pixels and more
STEM = [(2, 3, 13, 17, 128, 7, 1, 3, RELU, 0.1), (2, 3, 20, 30, 64, 7, 2, 3, LEAKY, 0.1)]
PAIR = [(2, 12, 16, 24, 64, 7, 3), (1, 12, 37, 50, 64, 7, 3)]
DECONV = [(1, 64, 7, 9, 32), (2, 1026, 4, 5, 129)]
FLOW_HEAD = [(2, 1024, 8, 15, 0, True, True), (1, 33, 21, 50, 0, True, True)]
HG_FRONT = [(2, 9, 11, 48), (1, 16, 32, 8)]


def make_round_conv(seed, N, cin, H, W, cout, k, stride, pad, act=NONE, slope=0.1, transposed=False, mag_x=255, mag_w=8, mag_b=2000, sigma=SIGMA,
                    pool=None, scale=(0, 0)):
    """Operands, pre-activation sum and rounded reference of one trunk layer.  x integers in +-mag_x, w integers in +-mag_w on a share
    of the elements chosen for a standard deviation `sigma` of the sum (per term: E x^2 E w^2), dense in channel 0 and the ragged last
    32-chunk as in `make_conv`; bias in +-mag_b.  `scale` = (ex, ew): x times 2^ex, w times 2^ew, b times 2^(ex + ew) -- every float32
    operation is then the same operation on the same significands (the underflow cases).  `pool`: see `_exact.check_rounds`."""
    rs = np.random.RandomState(seed)
    # ReLU and Leaky 0.1 leave ties on the positive side only (0.1 x in float32 is almost never half-way).  Those cases lift the mean of
    # the sums to about half a standard deviation (inputs from -mag_x + 32, half of the negative weights turned positive), so that two thirds of the
    # outputs are positive and a wrong tie rule still moves well above 5 % of the map.  Leaky 0.1 takes half that lift: its negative
    # side is where an activation on the wrong side of the rounding shows.
    lift = 0.5 if act == RELU else 0.25 if (act == LEAKY and slope == 0.1) else 0.0
    x = E.ints(rs, (N, cin, H, W), -mag_x + (32 if lift else 0), mag_x)
    taps = (k // stride) ** 2 if transposed else k * k
    ex2, ew2 = mag_x * (mag_x + 1) / 3.0, (mag_w + 1) * (2 * mag_w + 1) / 6.0
    dens = min(1.0, sigma ** 2 / (ex2 * ew2 * cin * taps))
    shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = E.sparse_weights(rs, shape, dens, mag_w)
    if lift:
        w = torch.where(torch.from_numpy(rs.random_sample(size=shape) < lift), w.abs(), w)
    dense = E.sparse_weights(rs, shape, 1.0, 1)
    last = 32 * ((cin - 1) // 32)
    if dens < 1.0 and (cin - last < 32 or cin == 32):
        idx = [0] + list(range(last, cin)) if cin % 32 else [0, cin - 1]
        for c in idx:
            if transposed:
                w[c] = torch.where(w[c] == 0, dense[c], w[c])
            else:
                w[:, c] = torch.where(w[:, c] == 0, dense[:, c], w[:, c])
    b = E.ints(rs, (cout,), -mag_b, mag_b)
    fx, fw = 2.0 ** scale[0], 2.0 ** scale[1]
    x, w, b = x * fx, w * fw, b * (fx * fw)
    what = f"rounding case {(N, cin, H, W, cout, k, stride, pad)}"
    E.check_storable(x, torch.float16, what + " input")
    E.check_storable(w, torch.float16, what + " weight")
    pre = (E.deconv_ref if transposed else E.conv_ref)(x, w, b, stride=stride, padding=pad, what=what)
    if scale == (0, 0):
        E.check_rounds(pre, what, pool=pool)
    want = E.act_round_ref(pre, act, slope)
    return dict(x=x, w=w, b=b, pre=pre, want=want, cout=cout, cin=cin, stride=stride, pad=pad, act=act, slope=slope, transposed=transposed)


# ---------------------------------------------------------------------------------------------------------------- every trunk case, by name
def trunk_cases():
    """name -> a thunk building the case (operands are built on demand and cached by the callers: `case(name)`)."""
    out = {}
    for i, s in enumerate(GATHER):
        out[f"gather{i}"] = lambda i=i, s=s: make_round_conv(1100 + i, *s, act=ACTS[i % 4][0], slope=ACTS[i % 4][1])
    for i, s in enumerate(SPLITK):
        out[f"splitk{i}"] = lambda i=i, s=s: make_round_conv(1200 + i, *s, act=ACTS[(i + 2) % 4][0], slope=ACTS[(i + 2) % 4][1])
    for i, s in enumerate(TILE):
        out[f"tile{i}"] = lambda i=i, s=s: make_round_conv(1300 + i, *s, act=ACTS[(i + 1) % 4][0], slope=ACTS[(i + 1) % 4][1])
    for i, (N, cin, H, W, cout, k) in enumerate(PATCH):
        out[f"patch{i}"] = lambda i=i, s=(N, cin, H, W, cout, k, 1, k // 2): make_round_conv(1400 + i, *s, act=ACTS[(i + 2) % 4][0], slope=ACTS[(i + 2) % 4][1])
    for i, (N, cin, H, W, cout) in enumerate(ONE):
        out[f"one{i}"] = lambda i=i, s=(N, cin, H, W, cout, 1, 1, 0): make_round_conv(1500 + i, *s, act=ACTS[(i + 3) % 4][0], slope=ACTS[(i + 3) % 4][1])
    for i, (N, cin, H, W, cout, k, st, p, act, slope) in enumerate(STEM):
        out[f"stem{i}"] = lambda i=i, s=(N, cin, H, W, cout, k, st, p), a=(act, slope): make_round_conv(1600 + i, *s, act=a[0], slope=a[1])
    for i, (N, cin, H, W, cout, k, pad) in enumerate(PAIR):
        out[f"pair{i}"] = lambda i=i, s=(N, cin, H, W, cout, k, 2, pad): make_round_conv(1700 + i, *s, act=LEAKY, slope=0.1)
    for i, (N, cin, H, W, cout) in enumerate(DECONV):
        out[f"deconv{i}"] = lambda i=i, s=(N, cin, H, W, cout, 4, 2, 1): make_round_conv(1800 + i, *s, act=LEAKY, slope=(0.75, 0.1)[i], transposed=True)
    return out


_CASES = trunk_cases()
_cache = {}


def case(name):
    """The named trunk case, built once per process and never modified by its users."""
    if name not in _cache:
        _cache[name] = _CASES[name]()
    return _cache[name]


def names(prefix=""):
    return [n for n in _CASES if n.startswith(prefix)]


def flow_head_case(i):
    """HFlowHead: predict_flow (3x3, 2 outputs) rounds; the fused ConvTranspose2d(2, 2, 4, 2, 1) reads the ROUNDED flow and rounds again.
    The two flow maps are small (480 and 2100 elements) and are pooled for `check_rounds`; the upsampled maps are held to it singly."""
    if ("flow", i) not in _cache:
        pool = []
        cs = [make_round_conv(2100 + j, N, cin, H, W, 2, 3, 1, 1, sigma=4000.0, pool=pool) for j, (N, cin, H, W, _, _, _) in enumerate(FLOW_HEAD)]
        E.check_rounds_pool(pool, "flow head: the flow maps of both cases")
        for j, c in enumerate(cs):
            rs = np.random.RandomState(2150 + j)
            wu, bu = E.sparse_weights(rs, (2, 2, 4, 4), 1.0, 2, 0.25), E.ints(rs, (2,), -2000, 2000)
            up0 = E.deconv_ref(c["want"], wu, bu, stride=2, padding=1, what="flow upsampling")
            E.check_rounds(up0, f"flow upsampling {j}")
            _cache[("flow", j)] = dict(c, wu=wu, bu=bu, up0=up0, up=E.round_f16(up0))
    return _cache[("flow", i)]


def hg_front_case(i):
    """HHourglassFront: 7x7 stem (3 -> 128) + ReLU rounds; the 2x2 max pool (exact) and the 1x1 + ReLU read the ROUNDED stem; the 1x1 sum
    rounds again.  The stem's sums are kept near 3000 so that a few of them add up inside the fp16 range."""
    if ("hg", i) not in _cache:
        N, H, W, c2 = HG_FRONT[i]
        s = make_round_conv(2200 + i, N, 3, H, W, 128, 7, 1, 3, act=RELU, sigma=3000.0)
        rs = np.random.RandomState(2250 + i)
        w1 = E.sparse_weights(rs, (c2, 128, 1, 1), 6.0 / 128, 1)
        b1 = E.ints(rs, (c2,), -2000, 2000)
        one0 = E.conv_ref(s["want"], w1, b1, what="hourglass 1x1")
        E.check_rounds(one0, f"hourglass 1x1 {i}")
        _cache[("hg", i)] = dict(stem=s, w1=w1, b1=b1, one0=one0, one=E.act_round_ref(one0, RELU), pool=torch.nn.functional.max_pool2d(s["want"], 2, 2))
    return _cache[("hg", i)]


def avg_pool_case(shape):
    """Gaussian fp16 values [N,H,W,C + 8] (the pool reads the slice from channel 8) and the reference of pool2x2's average: the float32
    sum of four fp16 values, times 0.25 (exact), one rounding.  The sum is exact in any order while 4 max |x| stays below 2^24 of the
    finest granule, so magnitudes below 2^-6 (granule 2^-16) are raised to 2^-6: 4 max |x| < 2^8 is checked."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn((N, H, W, C + 8), generator=g, dtype=torch.float64) * 3.0
    x = torch.where(x.abs() < 2.0 ** -6, torch.where(x < 0, -1.0, 1.0) * 2.0 ** -6, x)
    x16 = x.to(torch.float16)
    x = x16.double()[..., 8:].permute(0, 3, 1, 2)
    if not 4.0 * float(x16.double().abs().max()) < 2.0 ** 8 or float(x16.double().abs().min()) < 2.0 ** -6:
        raise E.BudgetError("average pool: the sum of four values may round in float32")
    s4 = torch.nn.functional.avg_pool2d(x, 2, 2) * 4.0
    E.check_storable(s4, torch.float32, "sum of four fp16 values")
    p = E.rounding_profile(s4 * 0.25)
    if float(p["inexact"].double().mean()) < 0.25 or int(p["tie"].sum()) < 32:
        raise E.BudgetError("average pool: too few values need rounding")
    return x16, E.round_f16(s4 * 0.25)


# ---------------------------------------------------------------------------------------------------------------- wrong evaluations
def alternatives(c):
    """The same layer evaluated under each defect -> dict name -> float64 map.  Never a reference: tests/test_exact_helper.py
    counts how many elements of `c["want"]` each one moves, which is how many the device comparison would report for that defect.
      rtz / away      another rounding at the one store;
      act_after       rounded first, the activation on the fp16 value, rounded again (the SR order in a trunk kernel);
      slope16         the slope rounded to fp16 where the kernel keeps it in float32 (cases whose slope is no fp16 value: Leaky 0.1);
      partial         the first half of the input channels summed and parked in fp16 before the final add (two roundings)."""
    pre, act, slope = c["pre"], c["act"], c["slope"]
    y = E.act_f32(pre, act, slope)
    out = dict(rtz=E.round_f16_alt(y, "rtz"), away=E.round_f16_alt(y, "away"))
    if act == LEAKY:
        out["act_after"] = E.act_round_ref(E.round_f16(pre), act, slope)
        s16 = float(E.round_f16(torch.tensor([float(slope)], dtype=torch.float32).to(torch.float64)))
        if s16 != float(torch.tensor(float(slope), dtype=torch.float32)):
            out["slope16"] = E.act_round_ref(pre, act, s16)
    half = c["cin"] // 2
    if half:
        fn = torch.nn.functional.conv_transpose2d if c["transposed"] else torch.nn.functional.conv2d
        wa = c["w"][:half] if c["transposed"] else c["w"][:, :half]
        part = fn(c["x"][:, :half], wa, None, stride=c["stride"], padding=c["pad"])
        out["partial"] = E.act_round_ref(E.round_f16(part) + (pre - part), act, slope)
    return out


def moved(c, alt):
    """Number of elements in which `alt` differs from the case's reference."""
    return int((alt != c["want"]).sum())


# ---------------------------------------------------------------------------------------------------------------- overflow and underflow
EDGE_SHAPES = {  # family -> (N, cin, H, W, cout, k, stride, pad): one single-layer case per family, a few hundred pixels each
    "gather": (1, 33, 12, 22, 17, 3, 1, 1), "tile": (1, 33, 11, 24, 65, 3, 1, 1), "patch_r8": (1, 96, 13, 19, 17, 3, 1, 1),
    "conv1x1_stream": (1, 128, 241, 272, 72, 1, 1, 0), "splitk": (1, 473, 16, 16, 256, 3, 1, 1),
}


def overflow_case(family):
    """A rounding case in which four output channels (the first two and the last two) carry a large bias, so that their sums straddle
    65504 .. 65536.  IEEE: magnitudes of 65520 and above store +-inf, magnitudes strictly between 65504 and 65520 store +-65504.
    That window is 15 integers wide.  With a bias of +-61440 and sums of a few thousand on top, a map of some hundred pixels puts less
    than one element inside it, so the bias is +-65512 (61440 + 4072, the middle of the window; a float32 bias need not be an fp16
    value) and the four weight rows are thin (two weights of +-1: a spread of about 200).  At least 8 elements fall on each side of the
    threshold (checked).  The other channels round as in every other case."""
    shape = EDGE_SHAPES[family]
    rs = np.random.RandomState(sum(shape))
    c = make_round_conv(1900 + shape[1], *shape, act=NONE)
    cout, cin, k = shape[4], shape[1], shape[5]
    b, w = c["b"].clone(), c["w"].clone()
    chans = [0, 1, cout - 2, cout - 1]
    for j, ch in enumerate(chans):
        sign = 1.0 if j % 2 == 0 else -1.0
        w[ch] = 0.0
        for _ in range(2):
            w[ch, rs.randint(0, cin), rs.randint(0, k), rs.randint(0, k)] = float(rs.randint(0, 2) * 2 - 1)
        b[ch] = sign * (61440.0 + 4072.0)
    pre = E.conv_ref(c["x"], w, b, stride=c["stride"], padding=c["pad"], what=f"overflow case {family}")
    c = dict(c, w=w)
    sel = pre[:, chans].abs()
    n_inf, n_max = int((sel >= 65520.0).sum()), int(((sel > 65504.0) & (sel < 65520.0)).sum())
    if n_inf < 8 or n_max < 8:
        raise E.BudgetError(f"overflow case {family}: {n_inf} elements at or above 65520 and {n_max} strictly between 65504 and 65520 (minimum 8 each)")
    want = E.round_f16(pre)
    assert int(torch.isinf(want).sum()) == n_inf
    return dict(c, b=b, pre=pre, want=want, n_inf=n_inf, n_max=n_max)


def underflow_case(family):
    """A rounding case scaled by 2^-28 in total: x by 2^-14 (inputs stay normal fp16 values), w by 2^-14, b by 2^-28.  The sums of 13 to
    15 bits land in fp16's subnormal range, where the spacing is 2^-24: at least 25 % of the outputs are subnormals that need rounding
    (checked); the reference is IEEE gradual underflow."""
    shape = EDGE_SHAPES[family]
    c = make_round_conv(2000 + shape[1], *shape, act=NONE, scale=(-14, -14))
    E.check_rounds(c["pre"] * 2.0 ** 28, f"underflow case {family} (unscaled)")
    sub = (c["pre"].abs() < 2.0 ** -14) & (c["pre"] != 0) & (c["want"] != c["pre"])
    share = float(sub.double().mean())
    if share < 0.25:
        raise E.BudgetError(f"underflow case {family}: {share:.1%} of the outputs are subnormals that need rounding (minimum 25%)")
    return dict(c, n_sub=int(sub.sum()))


# ---------------------------------------------------------------------------------------------------------------- the SR net
# A layer that reads a ROUNDED map (11-bit significands at magnitudes of thousands) cannot add many of them inside the fp16 range, and
# finer weights than +-1 would leave no ties.  So behind the first, wide layer of a case every further layer has TWO weights of +-1 per
# output row (and a bias up to +-2000): its sum of two rounded values and an integer needs rounding again, ties included, the standard
# deviation grows by about a fifth per layer, and with three-bit slopes the granularity falls by two or three bits per layer -- all
# three sums of a stage (and the POST 1x1 behind them) round inside ONE budget; no fallback to one rounding point per profile is needed.
SR_SIGMA = 5000.0
SLOPES_MAX = (0.75, 0.625, 0.75)          # fp16 values of at most three significant bits, no powers of two: the builds for slopes <= 1
SLOPES_SEL = (1.5, -0.75, 0.75)           # a slope above 1 in the deconvolution's PReLU: the select builds (the last slope stays 0.2 / 0.1)
SR_SHAPES = {4: [(1, 2, 2), (2, 37, 45), (1, 9, 65)], 2: [(1, 2, 2), (2, 37, 95), (2, 47, 3)], 3: [(1, 2, 30), (2, 37, 31), (1, 5, 61)]}


def wide_weights(rs, shape, terms, x, sigma=SR_SIGMA, mag=8):
    """Integer weights in +-mag on a share of `shape` such that a sum of `terms` products with the values of `x` has about `sigma`."""
    ex2 = float((x * x).mean())
    dens = min(1.0, sigma ** 2 / (ex2 * (mag + 1) * (2 * mag + 1) / 6.0 * terms))
    return E.sparse_weights(rs, shape, dens, mag)


def two_taps(rs, rows, fan):
    """[rows, fan]: two weights of +-1 per row, zero elsewhere."""
    w = np.zeros((rows, fan))
    for r in range(rows):
        w[r, rs.choice(fan, size=2, replace=False)] = rs.randint(0, 2, size=2) * 2 - 1
    return torch.from_numpy(w)


def two_taps_deconv(rs, S):
    """[32 (in), 32 (out), k, k] for ConvTranspose2d(k = S + 4, s = S, p = 2): per out-channel and per output phase two weights of +-1
    (a tap (ky, kx) feeds the outputs of phase ((ky - 2) mod S, (kx - 2) mod S) only)."""
    k = S + 4
    w = np.zeros((32, 32, k, k))
    for co in range(32):
        for py in range(S):
            for px in range(S):
                kys, kxs = [ky for ky in range(k) if (ky - 2) % S == py], [kx for kx in range(k) if (kx - 2) % S == px]
                for _ in range(2):
                    w[rs.randint(0, 32), co, kys[rs.randint(0, len(kys))], kxs[rs.randint(0, len(kxs))]] = rs.randint(0, 2) * 2 - 1
    return torch.from_numpy(w)


SMALL = {}      # storage point -> {case: its pre-rounding sums}: the maps below 512 elements, which meet `check_rounds` as a pool


def liveness(key, maps):
    """`_exact.check_rounds` on every pre-rounding map of a case that holds 512 elements; a smaller one joins the pool of its storage point
    (`SMALL`), which tests/test_exact_helper.py holds to the same numbers over all the small cases."""
    for name, pre in maps.items():
        if pre.numel() >= 512:
            E.check_rounds(pre, name)
            E.check_live(pre, name, min_distinct=4)
        else:
            SMALL.setdefault(name, {})[key] = pre.reshape(-1)


def small_cases():
    """Builds every case of the GPU tests that holds a map below 512 elements -> `SMALL`."""
    for S in (4, 2):
        for select, post in ((False, False), (False, True), (True, False), (True, True)):
            gen_round_stage(S, (1, 2, 2), select=select, post=post)
        for fold in ((False, True) if S == 4 else (True,)):
            for last in (False, True):
                gen_round_tail(S, (1, 2, 2), fold=fold, last=last)
    for slopes in ((0.75, 0.2), (1.5, 0.1)):
        gen_round_head((3, 2, 2), slopes=slopes)
    return SMALL


STAGE_KEYS = ("a", "up_w", "up_b", "up_a", "dt_w", "dt_b", "dt_a", "dn_w", "dn_b", "dn_a", "S")


def eval_stage(c, post, live=False, store=E.store_f16, store_out=E.store_f32act, weights_f16=True):
    """The stage case `c` (and with `post` the uptran 1x1 behind it) under `_exact.stage_round_ref`; `store` / `store_out` replace what is
    stored at the inner / the output points (a defect, for the discrimination checks)."""
    ref = E.stage_round_ref(**{k: c[k] for k in STAGE_KEYS}, live=("up", "dt", "dn") if live else (), store=store, store_out=store_out, weights_f16=weights_f16)
    if post:
        p0 = E.conv_ref(ref["out"], c["post_w"].reshape(32, 32, 1, 1), c["post_b"], what="POST 1x1")
        if live:
            E.check_rounds(p0, "POST 1x1 sum")
        ref["p0"] = p0
        ref["post"] = store(p0, c["post_a"], "max" if c["post_a"] <= 1.0 else "select", "post")
    return ref


def gen_round_stage(S, shape, select=False, post=False, seed=0):
    """One FeedbackBlock stage in which ALL storage points round: the deconvolution (inputs +-255, weights +-8), the downtran 1x1 and
    the strided convolution (two taps each), and with `post` the next group's uptran 1x1 behind them.  The last PReLU of the case takes a
    slope that is no fp16 value (0.2 without POST, 0.1 on the POST output, in the select cases too): nothing reads its result under a budget, and it pins what
    becomes of the slope -- rounded to fp16 by the packer for the packed-fp16 PReLU of the POST output, kept in float32 for the stage's
    own output, whose PReLU is a float32 operation in front of the one conversion.  -> (case as test_gpu_exact_sr.gen_stage lays it out, reference dict(hr, t, out[, post]))."""
    key = ("stage", S, shape, select, post, seed)
    if key in _cache:
        return _cache[key]
    N, h, w = shape
    k = S + 4
    rs = np.random.RandomState(3000 + S * 100 + N * 1000 + h * 10 + w + seed)
    sl = SLOPES_SEL if select else SLOPES_MAX
    a = E.ints(rs, (N, 32, h, w), -255, 255)
    # (a slope of 1.5 widens every later sum: the select cases start narrower, so that the POST sum stays inside the fp16 range -- but not
    # on the 2 x 2 map, where most HR pixels see a quarter of the taps and a narrower start would leave too few sums to round)
    c = dict(a=a, up_w=wide_weights(rs, (32, 32, k, k), 32.0 * (k / S) ** 2, a, sigma=3000.0 if (select and h * w > 4) else SR_SIGMA), up_b=E.ints(rs, (32,), -2000, 2000), up_a=sl[0],
             dt_w=two_taps(rs, 32, 32), dt_b=E.ints(rs, (32,), -2000, 2000), dt_a=sl[1],
             dn_w=two_taps(rs, 32, 32 * k * k).reshape(32, 32, k, k), dn_b=E.ints(rs, (32,), -2000, 2000), dn_a=sl[2] if post else 0.2, S=S)
    c.update(post_w=two_taps(rs, 32, 32), post_b=E.ints(rs, (32,), -2000, 2000), post_a=0.1)
    if not post:      # (the module still packs a POST slice: harmless weights)
        c.update(post_w=c["post_w"] * 0.0, post_b=c["post_b"] * 0.0, post_a=0.5)
    ref = eval_stage(c, post)
    liveness(key, {"stage deconvolution sum": ref["hr0"], "stage downtran sum": ref["t0"], "stage output sum": ref["o0"], **({"POST 1x1 sum": ref["p0"]} if post else {})})
    _cache[key] = (c, ref)
    return c, ref


def gen_round_tail(S, shape, fold=False, last=False, seed=0):
    """The tail with its deconvolution sum rounding: hid +-255 and weights +-8 (or, with `fold`, the folded compress_out rounding first --
    two LR maps +-255, weights +-8, a float32 constant map -- and the deconvolution reading its ROUNDED output through two taps per
    output phase), the fp16 PReLU, then conv_out in float32 on the rounded map inside its budget.
    `last` False: slope 0.625 (0.75 behind a fold) and a sparse conv_out (weights +-4 on a tenth of the taps).  `last` True: slope 0.2, which is no fp16 value;
    its products have granules down to 2^-13 beside values of thousands, so conv_out gets ONE weight of +-1 per row and no bias -- a sum
    of one term is exact -- and the case pins the packer's slope and the single rounding of the product."""
    key = ("tail", S, shape, fold, last, seed)
    if key in _cache:
        return _cache[key]
    N, h, w = shape
    k = S + 4
    rs = np.random.RandomState(4000 + S * 100 + N * 1000 + h * 10 + w + seed + 7 * fold + 13 * last)
    c = dict(S=S, out_a=0.2 if last else 0.75 if fold else 0.625)     # (0.75 behind the fold: two bits of granularity, conv_out's budget holds)
    if fold:
        la, lb = E.ints(rs, (N, 32, h, w), -255, 255), E.ints(rs, (N, 32, h, w), -255, 255)
        c.update(lr_a=la, lr_b=lb, co_w=wide_weights(rs, (32, 64), 64.0, la), co_b=E.ints(rs, (32,), -1000, 1000), co_a=0.75,
                 cmap=E.ints(rs, (32, h, w), -1000, 1000))
        c["hid"], c["co0"] = E.fold_round_ref(la, lb, c["cmap"], c["co_w"], c["co_b"], c["co_a"], live=False)
        c["out_w"] = two_taps_deconv(rs, S)
    else:
        c["hid"] = E.ints(rs, (N, 32, h, w), -255, 255)
        c["out_w"] = wide_weights(rs, (32, 32, k, k), 32.0 * (k / S) ** 2, c["hid"])
    c["out_b"] = E.ints(rs, (32,), -2000, 2000)
    if last:
        cv = np.zeros((3, 32 * 9))
        cv[np.arange(3), rs.randint(0, 32 * 9, size=3)] = rs.randint(0, 2, size=3) * 2 - 1
        c.update(cv_w=torch.from_numpy(cv).reshape(3, 32, 3, 3), cv_b=torch.zeros(3, dtype=torch.float64))
    else:
        c.update(cv_w=E.sparse_weights(rs, (3, 32, 3, 3), 0.1, 4), cv_b=E.ints(rs, (3,), -2000, 2000))
    c["local"] = last
    ref = eval_tail(c)
    liveness(key, {"tail deconvolution sum": ref["hr0"], **({"compress_out sum": c["co0"]} if fold else {})})
    if ref["raw"].numel() >= 512:
        E.check_live(ref["raw"], "conv_out sum", min_distinct=50)
    _cache[key] = (c, ref)
    return c, ref


def eval_tail(c, live=False, store=E.store_f16):
    """The tail case `c` under `_exact.tail_round_ref` (behind `fold_round_ref` where it has a folded compress_out)."""
    hid = c["hid"]
    if "co_w" in c and store is not E.store_f16:
        hid = E.fold_round_ref(c["lr_a"], c["lr_b"], c["cmap"], c["co_w"], c["co_b"], c["co_a"], live=False, store=store)[0]
    return E.tail_round_ref(hid, c["out_w"], c["out_b"], c["out_a"], c["cv_w"], c["cv_b"], c["S"], live=live, local=c["local"], store=store)


HEAD_SUB = ((1.0, 0.5, 2.0), (-31.5, -16.0, -63.0))      # per-channel scales and biases that differ (halves), pixels 0..63


def gen_round_head(shape, slopes=(0.75, 0.2), seed=0):
    """k_head_h with both sums rounding: 6-bit pixels, mean shifts in halves, conv_in weights +-64 dense (27 terms: sums near 2^13
    halves), feat_in two taps per row on the rounded mid map.  The second slope (0.2) is no fp16 value."""
    key = ("head", shape, slopes, seed)
    if key in _cache:
        return _cache[key]
    N, h, w = shape
    rs = np.random.RandomState(5000 + N * 1000 + h * 10 + w + seed)
    sub = (torch.tensor(HEAD_SUB[0], dtype=torch.float64), torch.tensor(HEAD_SUB[1], dtype=torch.float64))
    c = dict(x=E.ints(rs, (N, 3, h, w), 0, 63), sub=sub, w_in=E.sparse_weights(rs, (128, 3, 3, 3), 1.0, 64), b_in=E.ints(rs, (128,), -1000, 1000), a_in=slopes[0],
             w_feat=two_taps(rs, 32, 128), b_feat=E.ints(rs, (32,), -2000, 2000), a_feat=slopes[1])
    ref = eval_head(c)
    liveness(key, {"conv_in sum": ref["m0"], "feat_in sum": ref["f0"]})
    _cache[key] = (c, ref)
    return _cache[key]


def eval_head(c, live=False, store=E.store_f16):
    out, m0, f0 = E.head_round_ref(c["x"], c["sub"], c["w_in"], c["b_in"], c["a_in"], c["w_feat"], c["b_feat"], c["a_feat"], live=live, store=store)
    return dict(out=out, m0=m0, f0=f0)


def gen_round_chain(spec, N, P, slopes=(0.75, 0.625, 0.2), seed=0, pool=None):
    """k_chain1x1_h / vsr_sr_conv1x1_f16 with every stage's sum rounding.  spec: per stage (memory inputs, reads the previous stage,
    constant map) as tests/test_gpu_exact_sr_ends.CHAIN_SPECS.  The first stage is wide (inputs +-255, weights +-8); a later stage reads
    the previous, ROUNDED output through two taps per row and its memory inputs through narrow weights (a standard deviation of 1500).
    The last slope (0.2) is no fp16 value."""
    key = ("chain", tuple(spec), N, P, slopes, seed)
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(6000 + N * 100 + P + 17 * len(spec) + seed)
    stages = []
    for s, (nin, prev, cm) in enumerate(spec):
        xs = [E.ints(rs, (N, 32, P), -255, 255) for _ in range(nin)]
        sig = SR_SIGMA if s == 0 else 1500.0
        stages.append(dict(ins=[(x, wide_weights(rs, (32, 32), 32.0 * nin, x, sigma=sig)) for x in xs], prev=two_taps(rs, 32, 32) if prev else None,
                           bias=E.ints(rs, (32,), -1000, 1000), cmap=E.ints(rs, (32, P), -1000, 1000) if cm else None,
                           slope=slopes[s] if s < len(spec) - 1 else slopes[-1]))
    outs, pres = E.chain_round_ref(stages, pool=pool)
    _cache[key] = (stages, outs, pres)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------- weights that are no fp16 values
def make_round_conv_w32(seed, N, cin, H, W, cout, k, stride, pad, act=NONE, slope=0.1):
    """A trunk layer whose float32 weights have 12 to 13 significant bits (integers 2049 .. 8191, half of the 12-bit ones odd: exact ties
    of the float32 -> fp16 conversion): the packer rounds them, the reference uses `round_f16(w)`.  Six weights per output row and inputs
    in +-2 keep the sums near 2^13 (granule 2: the rounded weights are even)."""
    rs = np.random.RandomState(seed)
    x = E.ints(rs, (N, cin, H, W), -2, 2)
    fan = cin * k * k
    w = np.zeros((cout, fan))
    for r in range(cout):
        idx = rs.choice(fan, size=min(6, fan), replace=False)
        w[r, idx] = rs.randint(2049, 4096, size=len(idx)) * (rs.randint(0, 2, size=len(idx)) * 2 - 1)
        w[r, idx[0]] = rs.randint(4097, 8192) * (rs.randint(0, 2) * 2 - 1)
    w = torch.from_numpy(w).reshape(cout, cin, k, k)
    w16 = E.round_f16(w, "float32 weight")
    moved = int((w16 != w).sum())
    p = E.rounding_profile(w[w != 0])
    if moved < 0.4 * int((w != 0).sum()) or int(p["tie_up"].sum()) < 16 or int(p["tie_down"].sum()) < 16:
        raise E.BudgetError("float32 weights: too few of them round, or too few ties")
    b = E.ints(rs, (cout,), -1000, 1000) * 2.0
    what = f"float32-weight case {(N, cin, H, W, cout, k, stride, pad)}"
    pre = E.conv_ref(x, w16, b, stride=stride, padding=pad, what=what)
    E.check_rounds(pre, what)
    unrounded = E.act_round_ref(E.conv_ref(x, w, b, stride=stride, padding=pad, what=what), act, slope)
    return dict(x=x, w=w, w16=w16, b=b, pre=pre, want=E.act_round_ref(pre, act, slope), cout=cout, cin=cin, stride=stride, pad=pad, act=act, slope=slope,
                transposed=False, unrounded=unrounded)


def w32_case(family, shape):
    if ("w32", family) not in _cache:
        _cache[("w32", family)] = make_round_conv_w32(7000 + shape[1] + shape[4], *shape, act=LEAKY, slope=0.75)
    return _cache[("w32", family)]


def gen_round_stage_w32(S, shape):
    """A stage whose DECONVOLUTION weights are float32 values of 12 to 13 significant bits (integers 2049 .. 8191, ties among them): the
    packer rounds them to fp16, the reference uses `round_f16(w)`.  Three weights per out-channel and output phase on inputs in +-1; the
    layers behind have two taps as in `gen_round_stage`.  -> (case with the FLOAT32 weights, reference)."""
    key = ("stage_w32", S, shape)
    if key in _cache:
        return _cache[key]
    N, h, w = shape
    k = S + 4
    rs = np.random.RandomState(7100 + S)
    up = np.zeros((32, 32, k, k))
    for co in range(32):
        for py in range(S):
            for px in range(S):
                kys, kxs = [ky for ky in range(k) if (ky - 2) % S == py], [kx for kx in range(k) if (kx - 2) % S == px]
                for j in range(3):
                    hi = 8192 if j == 0 else 4096
                    up[rs.randint(0, 32), co, kys[rs.randint(0, len(kys))], kxs[rs.randint(0, len(kxs))]] = rs.randint(hi // 2 + 1, hi) * (rs.randint(0, 2) * 2 - 1)
    up = torch.from_numpy(up)
    up16 = E.round_f16(up, "float32 weight")
    p = E.rounding_profile(up[up != 0])
    if int((up16 != up).sum()) < 0.4 * int((up != 0).sum()) or int(p["tie_up"].sum()) < 16 or int(p["tie_down"].sum()) < 16:
        raise E.BudgetError("float32 stage weights: too few of them round, or too few ties")
    c = dict(a=E.ints(rs, (N, 32, h, w), -1, 1), up_b=E.ints(rs, (32,), -1000, 1000) * 2.0, up_a=SLOPES_MAX[0],
             dt_w=two_taps(rs, 32, 32), dt_b=E.ints(rs, (32,), -2000, 2000), dt_a=SLOPES_MAX[1],
             dn_w=two_taps(rs, 32, 32 * k * k).reshape(32, 32, k, k), dn_b=E.ints(rs, (32,), -2000, 2000), dn_a=0.2, S=S)
    ref = E.stage_round_ref(up_w=up16, **c)
    other = E.stage_round_ref(up_w=up, **c, live=(), weights_f16=False)
    if int((other["out"] != ref["out"]).sum()) < 0.05 * ref["out"].numel():
        raise E.BudgetError("float32 stage weights: unrounded weights would move less than 5 % of the output")
    c.update(up_w=up, post_w=torch.zeros(32, 32, dtype=torch.float64), post_b=torch.zeros(32, dtype=torch.float64), post_a=0.5)
    _cache[key] = (c, ref)
    return c, ref


# ---------------------------------------------------------------------------------------------------------------- wrong evaluations of the SR cases
def _combine(v, m, build):
    return torch.maximum(v, m) if build == "max" else torch.minimum(v, m) if build == "min" else torch.where(v < 0, m, v)


def sr_defect(kind, parts=None, only=None):
    """-> (store, store_out): what the SR references store at the packed-fp16 points / at a stage's float32-PReLU output under a defect.
      rtz / away   another rounding of the sum (the product's rounding stays);
      act_side     the activation on the other side of the conversion: float32 PReLU and one rounding where the kernel converts first, and
                   the reverse at a stage's output;
      slope        the slope in the other format: float32 where the packer rounds it to fp16 (the product then rounds twice), fp16 at a
                   stage's output;
      partial      `parts[name]`, a partial sum of the storage point `name`, parked in fp16 before the final add.
    `only`: the one storage point (by name) that has the defect; every other point stores what the kernels store."""
    f32 = lambda s: torch.tensor(float(s), dtype=torch.float32)

    def store(pre, slope, build, name=None):
        if only is not None and name != only:
            return E.store_f16(pre, slope, build)
        if kind in ("rtz", "away"):
            return E.prelu_f16_ref(E.round_f16_alt(pre, kind), slope, build)
        if kind == "act_side":
            return E.store_f32act(pre, slope, build)
        if kind == "slope":
            v = E.round_f16(pre)
            return _combine(v, E.round_f16((v.to(torch.float32) * f32(slope)).to(torch.float64)), build)
        if kind == "partial" and parts and name in parts:
            return E.store_f16(E.round_f16(parts[name]) + (pre - parts[name]), slope, build)
        return E.store_f16(pre, slope, build)

    def store_out(pre, slope, build, name=None):
        if only is not None and name != only:
            return E.store_f32act(pre, slope, build)
        x = pre.to(torch.float32)
        if kind in ("rtz", "away"):
            return E.round_f16_alt(torch.where(x >= 0, x, x * f32(slope)).to(torch.float64), kind)
        if kind == "act_side":
            return E.store_f16(pre, slope, build)
        if kind == "slope":
            return E.act_round_ref(pre, 2, float(E.round_f16(f32(slope).to(torch.float64).reshape(1))))
        return E.store_f32act(pre, slope, build)

    return store, store_out


DEFECTS = ("rtz", "away", "act_side", "slope", "partial")


def has_float32_slope(*slopes):
    return any(float(E.round_f16(torch.tensor([float(s)], dtype=torch.float32).to(torch.float64))) != float(torch.tensor(float(s), dtype=torch.float32)) for s in slopes)


# ---------------------------------------------------------------------------------------------------------------- the x3 stage behind the folded chain
PRE_SHAPES = [(1, 2, 30), (2, 37, 31)]
PRE_CHAIN_SLOPES = (1.0, 0.0, 2.0)       # integer-preserving: the chain stays in the exact regime


def gen_round_pre(shape, mode, seed=0):
    """The x3 stage with the step-opening 1x1 chain folded into its LR load path (tests/test_gpu_utd_s3_pre.py lays the case out).  The
    chain (compress_out -> compress_in -> uptran, `mode` 3; compress_in -> uptran, `mode` 2) stays in the exact regime -- integers in
    +-255, two unit weights per row, integer-preserving slopes: its output is an integer map of a few hundred, an fp16 value -- and ALL
    storage points of the stage behind it round as in `gen_round_stage` with POST.  The chain's own roundings are what
    `gen_round_chain` covers on the chain kernel; inside this build they are not reached.  -> (case, dict(x, out, post))."""
    key = ("pre", shape, mode, seed)
    if key in _cache:
        return _cache[key]
    N, h, w = shape
    P, k, S = h * w, 7, 3
    rs = np.random.RandomState(8000 + N * 1000 + h * 10 + w + mode + seed)
    one = lambda: two_taps(rs, 32, 32)
    c = dict(feat=E.ints(rs, (N, 32, P), -255, 255), la=E.ints(rs, (N, 32, P), -255, 255), lb=E.ints(rs, (N, 32, P), -255, 255), cmap=E.ints(rs, (32, P), -100, 100),
             co_wa=one() * (torch.arange(32).view(32, 1) % 2 == 0), co_wb=one() * (torch.arange(32).view(32, 1) % 2 == 1), co_b=E.ints(rs, (32,), -100, 100),
             ci_wf=one() * (torch.arange(32).view(32, 1) % 2 == 0), ci_wp=one() * (torch.arange(32).view(32, 1) % 2 == 1), ci_b=E.ints(rs, (32,), -100, 100),
             ut_w=one(), ut_b=E.ints(rs, (32,), -100, 100))
    cs = PRE_CHAIN_SLOPES
    if mode == 3:
        st = [dict(ins=[(c["la"], c["co_wa"]), (c["lb"], c["co_wb"])], bias=c["co_b"], cmap=c["cmap"], slope=cs[0]),
              dict(ins=[(c["feat"], c["ci_wf"])], prev=c["ci_wp"], bias=c["ci_b"], slope=cs[1])]
    else:
        st = [dict(ins=[(c["feat"], c["ci_wf"]), (c["feat"], c["ci_wp"])], bias=c["ci_b"], slope=cs[1])]
    st.append(dict(ins=[], prev=c["ut_w"], bias=c["ut_b"], slope=cs[2]))
    x = E.chain_ref(st)[-1].reshape(N, 32, h, w)
    sl = SLOPES_MAX
    c.update(a=x, up_w=wide_weights(rs, (32, 32, k, k), 32.0 * (k / S) ** 2, x), up_b=E.ints(rs, (32,), -2000, 2000), up_a=sl[0],
             dt_w=two_taps(rs, 32, 32), dt_b=E.ints(rs, (32,), -2000, 2000), dt_a=sl[1],
             dn_w=two_taps(rs, 32, 32 * k * k).reshape(32, 32, k, k), dn_b=E.ints(rs, (32,), -2000, 2000), dn_a=sl[2], S=S,
             post_w=two_taps(rs, 32, 32), post_b=E.ints(rs, (32,), -2000, 2000), post_a=0.1)
    ref = eval_stage(c, True)
    liveness(key, {"stage deconvolution sum": ref["hr0"], "stage downtran sum": ref["t0"], "stage output sum": ref["o0"], "POST 1x1 sum": ref["p0"]})
    ref["x"] = x
    _cache[key] = (c, ref)
    return c, ref
