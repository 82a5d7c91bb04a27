"""k_tail_s3 (csrc/sr_tail_s3.hip, libvsr_hip_s3t.so): the x3 tail -- `out` deconvolution k7 s3 p2 + PReLU -> conv_out 3x3 -- in one launch

  * values against a float64 composition with the HR map rounded to fp16 where the kernel rounds, and against the unfused route,
  * bit for bit against itself across row segmentations, plane counts, `dec`, the select build and the folded compress_out,
  * with PReLU slopes above 1 and below 0,
  * in exact arithmetic (tests/_exact.py): equal to float64 on dyadic operands, one planted unit seen with its footprint,
  * on poisoned, guard-banded buffers (tests/_poison.py),
  * inside the x3 SR net (fixture g8_sr_x3_6x10) and VSR.forward, with the tail fused and unfused, share_tail on and off.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _exact as E  # noqa: E402
from _poison import poisoned  # noqa: E402
from test_gpu_exact_sr_ends import _cmap_nhwc, _planted, _raw, gen_tail, tail_module  # noqa: E402
from test_gpu_poisoned_buffers import _sr_inputs, run_poisoned  # noqa: E402
from video_super_resolution_amd import SRProjectionModule  # noqa: E402
from video_super_resolution_amd import _lib as L  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

_master = {}

# one row, one column, strips of 29 / 30 / 31 / 61 columns, rows that the segment does not divide, 1 / 3 / 8 planes
SHAPES = [(1, 1, 40), (2, 23, 1), (1, 7, 29), (3, 6, 30), (1, 13, 31), (2, 11, 61), (8, 12, 30), (1, 1, 1), (3, 37, 33)]


def sr3(tail=True):
    """A fresh x3 module with the seeded weights on the GPU (tests set slopes and switches on it)."""
    if "m" not in _master:
        _master["m"] = fill_module_(SRProjectionModule(upscale_factor=3).eval(), seed=0, prefix="model.")
    m = copy.deepcopy(_master["m"]).cuda().eval()
    m.precision = "fp16"
    m.fused_tail_s3 = tail
    return m


def _hid(N, h, w, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).randn(N, h, w, 32) * scale).astype(np.float16)).cuda()


def _tail(P, hid, rps, dec=False, le1=None, fold=None):
    """The entry itself on a NaN-filled output.  fold = (lr3, lr6, cmap): the fold entry (`hid` gives the shape only)."""
    N, h, w, _ = hid.shape
    raw = _raw(N, h if dec else 3 * h, w if dec else 3 * w)
    lib = L.load_s3t()
    le1 = int(P["slopes_le_one"]) if le1 is None else le1
    if fold is not None:
        L.check(lib.vsr_s3t_sr_tail_fold_f16(L.dptr(fold[0], torch.float16), L.dptr(fold[1], torch.float16), L.dptr(fold[2]), L.dptr(P["tail_s3"], torch.uint8),
                                             L.dptr(raw), N, h, w, rps, le1, int(dec), L.stream()), "sr_tail_s3_fold_f16", lib=lib)
    else:
        L.check(lib.vsr_s3t_sr_tail_f16(L.dptr(hid, torch.float16), L.dptr(P["tail_s3"], torch.uint8), L.dptr(raw), N, h, w, rps, le1, int(dec), L.stream()),
                "sr_tail_s3_f16", lib=lib)
    return raw


def _reference(m, hid):
    """float64: conv_transpose2d -> fp16 -> PReLU -> fp16 -> conv2d, on the fp16 weights the kernel multiplies by."""
    x = hid.permute(0, 3, 1, 2).double().cpu()
    a = float(m.out[1].weight.detach())
    q = F.conv_transpose2d(x, m.out[0].weight.detach().cpu().half().double(), m.out[0].bias.detach().cpu().double(), stride=3, padding=2).half().double()
    hr = torch.where(q >= 0, q, (q * float(np.float16(a))).half().double())
    return F.conv2d(hr, m.conv_out[0].weight.detach().cpu().half().double(), m.conv_out[0].bias.detach().cpu().double(), padding=1)


def _close(got, want, bar, what):
    err = (got.double().cpu() - want.double().cpu()).abs().max().item()
    assert torch.isfinite(got).all() and err <= bar * want.abs().max().item(), (what, err, want.abs().max().item())


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_x3_tail_values(shape):
    N, h, w = shape
    m, mu = sr3(True), sr3(False)
    P, Pu = m._packed(), mu._packed()
    assert "tail_s3" in P and P["tail_s3_fold"] and "tail_s3" not in Pu and "out_deconv" in P
    hid = _hid(N, h, w, 7 * h + w)
    want = _reference(m, hid)
    full = _tail(P, hid, 0)
    dec = _tail(P, hid, 0, dec=True)
    _close(full, want, 2e-3, f"x3 tail {shape} against float64")
    assert torch.equal(dec, full[..., ::3, ::3])
    for d in (False, True):   # the module's route, fused and unfused, on identical inputs
        got, unf = _raw(N, h if d else 3 * h, w if d else 3 * w), _raw(N, h if d else 3 * h, w if d else 3 * w)
        m._tail_raw(hid, P, d, got)
        mu._tail_raw(hid, Pu, d, unf)
        assert torch.equal(got, dec if d else full)
        _close(got, unf, 1e-3, f"x3 tail {shape} dec {d} against the unfused route")


@pytest.mark.parametrize("shape", [(1, 7, 29), (3, 13, 31), (2, 11, 61), (8, 12, 30), (2, 23, 1)])
def test_fused_x3_tail_bit_identical_across_segments_planes_and_builds(shape):
    N, h, w = shape
    m = sr3()
    P = m._packed()
    hid = _hid(N, h, w, 3 * h + w)
    ref = _tail(P, hid, 0)
    ref_dec = _tail(P, hid, 0, dec=True)
    assert torch.equal(ref_dec, ref[..., ::3, ::3])
    for rps in sorted({1, 2, 5, h, int(m._rows_per_segment(N, h, w, cus=512, strip=30))}):
        assert torch.equal(_tail(P, hid, rps), ref), rps
        assert torch.equal(_tail(P, hid, rps, dec=True), ref_dec), rps
    for n in range(N):   # plane by plane
        assert torch.equal(_tail(P, hid[n:n + 1].contiguous(), 0), ref[n:n + 1]), n
    assert P["slopes_le_one"]
    assert torch.equal(_tail(P, hid, 2, le1=0), ref) and torch.equal(_tail(P, hid, 0, dec=True, le1=0), ref_dec)   # the select build


@pytest.mark.parametrize("hw", [(16, 16), (9, 40), (37, 33), (2, 2), (1, 7)])
@pytest.mark.parametrize("decimate", [False, True])
def test_x3_tail_with_folded_compress_out_bit_identical(hw, decimate):
    """compress_out inside k_tail_s3's LR load path against its own chain launch followed by the plain build, through the module; then
    with a compress_out slope above 1."""
    m = sr3()
    h, w = hw
    x = torch.from_numpy(np.random.RandomState(h * 17 + w).randint(0, 256, (8, 3, h, w)).astype(np.float32)).cuda()
    names = []
    L.TIMER.enabled, L.TIMER.only = True, None
    L.TIMER.reset()
    try:
        with torch.no_grad():
            m.fold_tail = True
            got = m(x, decimate=decimate).clone()
            torch.cuda.synchronize()
            names.append(L.TIMER.summary())
            L.TIMER.reset()
            m.fold_tail = False
            ref = m(x, decimate=decimate).clone()
            torch.cuda.synchronize()
            names.append(L.TIMER.summary())
            m.block.compress_out[1].weight.fill_(1.25)
            ref2 = m(x, decimate=decimate).clone()
            m.fold_tail = True
            got2 = m(x, decimate=decimate).clone()
    finally:
        L.TIMER.enabled = False
        L.TIMER.reset()
    tname = "sr_tail_s3_dec_f16" if decimate else "sr_tail_s3_f16"
    assert tname in names[0] and tname in names[1] and "sr_convout_planes_f16" not in list(names[0]) + list(names[1])
    assert names[1]["sr_chain1x1_f16 x1"][0] == names[0].get("sr_chain1x1_f16 x1", (0, 0.0))[0] + 1   # the launch the fold replaces
    assert torch.isfinite(got).all() and torch.equal(got, ref) and torch.equal(got2, ref2)


@pytest.mark.parametrize("slope", [1.5, 3.0, -0.5, -1.5])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 33, 31)])
def test_fused_x3_tail_slopes_of_any_sign_and_size(shape, slope):
    N, h, w = shape
    m = sr3()
    with torch.no_grad():
        m.out[1].weight.fill_(slope)
    P = m._packed()
    assert P["slopes_le_one"] == (slope <= 1.0)
    hid = _hid(N, h, w, 5 * h + w)
    got = _tail(P, hid, 0)
    _close(got, _reference(m, hid), 2e-3, f"x3 tail {shape} slope {slope}")
    assert torch.equal(_tail(P, hid, 3, le1=0), got)   # the select build is right for every slope
    raw = _raw(N, 3 * h, 3 * w)
    m._tail_raw(hid, P, False, raw)
    assert torch.equal(raw, got)


def test_mixed_slopes_of_tail_and_folded_compress_out():
    """out slope <= 1 with compress_out slope > 1 and the reverse: the folded 1x1 looks at its own slope."""
    x = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (8, 3, 9, 33)).astype(np.float32)).cuda()
    for a_out, a_co in ((0.25, 1.75), (2.0, -0.5)):
        m = sr3()
        with torch.no_grad():
            m.out[1].weight.fill_(a_out)
            m.block.compress_out[1].weight.fill_(a_co)
            m.fold_tail = True
            got = m(x).clone()
            m.fold_tail = False
            assert torch.equal(m(x), got), (a_out, a_co)


# ---------------------------------------------------------------------------------------------------------------- exact arithmetic
@pytest.mark.parametrize("profile", ("dense", "out", "cv"))
@pytest.mark.parametrize("shape", [(1, 1, 29), (1, 2, 2), (2, 13, 31), (8, 6, 10), (2, 17, 3), (1, 1, 1), (1, 5, 61)])
def test_x3_fused_tail_equals_float64(shape, profile):
    N, h, w = shape
    slope = E.SLOPES_LE_ONE[(N + h + w + 2) % 4]
    c, ref = gen_tail(N * 1000 + h * 10 + w + 3, 3, shape, slope=slope, profile=profile)
    m = tail_module(c)
    P = m._packed()
    assert "tail_s3" in P
    hid = E.nhwc(c["hid"]).cuda()
    for dec in (False, True):
        want = ref["dec" if dec else "raw"]
        for rps in sorted({0, 1, min(h, 5)}):
            E.assert_exact(_tail(P, hid, rps, dec=dec), want, f"x3 fused tail {shape} {profile} rows {rps} dec {dec}")
        raw = _raw(N, h if dec else 3 * h, w if dec else 3 * w)
        m._tail_raw(hid, P, dec, raw)
        E.assert_exact(raw, want, f"x3 fused tail through _tail_raw {shape} {profile} dec {dec}")


@pytest.mark.parametrize("slope,co_slope", [(0.5, 0.25), (2.0, 0.5), (0.25, -0.5), (-0.5, 2.0)])
def test_x3_folded_tail_equals_float64(slope, co_slope):
    shape = (2, 9, 33)
    N, h, w = shape
    c, ref = gen_tail(77, 3, shape, slope=slope, profile="dense", fold=True, co_slope=co_slope)
    m = tail_module(c)
    P = m._packed()
    assert P["tail_s3_fold"]
    a, b, cm = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"])
    for dec in (False, True):
        want = ref["dec" if dec else "raw"]
        E.assert_exact(_tail(P, a, 4, dec=dec, fold=(a, b, cm)), want, f"x3 folded tail slope {slope} co slope {co_slope} dec {dec}")
        E.assert_exact(_tail(P, E.nhwc(c["hid"]).cuda(), 0, dec=dec), want, f"x3 plain tail on the float64 hid, dec {dec}")
        raw = _raw(N, h if dec else 3 * h, w if dec else 3 * w)
        m._tail_raw(a, P, dec, raw, fold=(a, b, cm))
        E.assert_exact(raw, want, f"x3 folded tail through _tail_raw dec {dec}")


# a 9-tap phase (1, 1), a 6-tap phase (0, 1), a 4-tap phase (2, 2); conv_out; the folded compress_out
_PLANTS = [("out_w", (5, 9, 3, 3)), ("out_w", (31, 0, 2, 6)), ("out_w", (0, 30, 1, 4)), ("cv_w", (1, 31, 2, 0)), ("co_w", (5, 63))]


@pytest.mark.parametrize("which,idx", _PLANTS)
def test_one_unit_in_one_x3_tail_weight_is_seen_with_its_footprint(which, idx):
    shape = (2, 7, 33)
    N, h, w = shape
    fold = which == "co_w"
    c, ref = gen_tail(30 + len(which) + idx[-1], 3, shape, slope=1.0, profile="dense", fold=fold, co_slope=1.0)
    c2 = dict(c)
    c2[which] = c[which].clone()
    c2[which][idx] += 1.0
    if fold:
        c2["hid"] = E.fold_ref(c2["lr_a"], c2["lr_b"], c2["cmap"], c2["co_w"], c2["co_b"], c2["co_a"], live=False)
    planted = E.tail_ref(c2["hid"], c2["out_w"], c2["out_b"], c2["out_a"], c2["cv_w"], c2["cv_b"], 3, live=False)
    P = tail_module(c2)._packed()
    if fold:
        a, b, cm = E.nhwc(c["lr_a"]).cuda(), E.nhwc(c["lr_b"]).cuda(), _cmap_nhwc(c["cmap"])
        got = _tail(P, a, 3, fold=(a, b, cm))
    else:
        got = _tail(P, E.nhwc(c["hid"]).cuda(), 3)
    mask = _planted(got, planted["raw"], ref["raw"], f"x3 fused tail planted {which}{idx}")
    if which == "cv_w":
        assert E.bbox(mask)[1] == (idx[0], idx[0])                      # one output channel
    elif which == "out_w":
        hr_diff = planted["hr"] != ref["hr"]
        assert not bool(hr_diff[:, [ch for ch in range(32) if ch != idx[1]]].any())      # one HR channel ...
        ys, xs = torch.nonzero(hr_diff.any(0).any(0), as_tuple=True)
        assert bool(((ys + 2 - idx[2]) % 3 == 0).all()) and bool(((xs + 2 - idx[3]) % 3 == 0).all())   # ... at the tap's phase
        box = E.bbox(mask)
        assert box[2][0] >= max(0, int(ys.min()) - 1) and box[2][1] <= min(3 * h - 1, int(ys.max()) + 1)
        assert box[3][0] >= max(0, int(xs.min()) - 1) and box[3][1] <= min(3 * w - 1, int(xs.max()) + 1)
    else:
        assert not bool((c2["hid"] != c["hid"])[:, [ch for ch in range(32) if ch != idx[0]]].any())   # one channel of the 1x1's output


# ---------------------------------------------------------------------------------------------------------------- poisoned buffers
@pytest.mark.parametrize("mode", ["full", "dec", "fold"])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 9, 40), (3, 37, 33)])
def test_x3_tail_poisoned_output_is_fully_written_and_bands_intact(shape, mode):
    N, h, w = shape
    m = sr3()
    P = m._packed()
    hid, lr6 = _hid(N, h, w, 11 + h), _hid(N, h, w, 12 + w)
    cm = torch.from_numpy(np.random.RandomState(h).randn(h * w, 32).astype(np.float32)).cuda()
    dec = mode == "dec"
    fold = (hid, lr6, cm) if mode == "fold" else None
    want = _tail(P, hid, 4, dec=dec, fold=fold)
    assert torch.isfinite(want).all()
    with poisoned() as arena:
        raw = torch.empty((N, 3, h if dec else 3 * h, w if dec else 3 * w), dtype=torch.float32, device="cuda")
        lib = L.load_s3t()
        if fold:
            rc = lib.vsr_s3t_sr_tail_fold_f16(L.dptr(hid, torch.float16), L.dptr(lr6, torch.float16), L.dptr(cm), L.dptr(P["tail_s3"], torch.uint8), L.dptr(raw),
                                              N, h, w, 4, 1, 0, L.stream())
        else:
            rc = lib.vsr_s3t_sr_tail_f16(L.dptr(hid, torch.float16), L.dptr(P["tail_s3"], torch.uint8), L.dptr(raw), N, h, w, 4, 1, int(dec), L.stream())
        L.check(rc, "sr_tail_s3", lib=lib)
        torch.cuda.synchronize()
        arena.assert_written(raw)
        assert torch.equal(raw, want)
        arena.check()


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 9, 40), (3, 37, 33)])
def test_x3_tail_route_on_poisoned_buffers(shape):
    """`_tail_raw` (plain, decimated, folded) on arena buffers; a second call with other inputs on the same module equals a fresh module."""
    N, h, w = shape
    ins = [(_hid(N, h, w, s), _hid(N, h, w, s + 1)) for s in (21 + h, 41 + w)]
    cm = torch.from_numpy(np.random.RandomState(w).randn(h * w, 32).astype(np.float32)).cuda()

    def call(m, a, b):
        P = m._packed()
        assert "tail_s3" in P
        outs = []
        for dec, fold in ((False, None), (True, None), (False, (a, b, cm)), (True, (a, b, cm))):
            raw = torch.empty((N, 3, h if dec else 3 * h, w if dec else 3 * w), dtype=torch.float32, device="cuda")
            m._tail_raw(a, P, dec, raw, fold=fold)
            outs.append(raw)
        return outs
    run_poisoned(sr3, call, ins[0], ins[1], what=f"x3 tail route {shape}")


@pytest.mark.parametrize("hw", [(9, 40), (37, 33)])
def test_x3_network_with_fused_tail_on_poisoned_buffers(hw):
    rs = np.random.RandomState(hw[0] * 31 + hw[1])

    def call(m, x, _):
        with torch.no_grad():
            r = [m(x), m(x, decimate=True)]
        assert "tail_s3" in m._packed()
        return r
    run_poisoned(sr3, call, _sr_inputs(rs, *hw), _sr_inputs(rs, *hw), what=f"x3 SR net, fused tail {hw}")


# ---------------------------------------------------------------------------------------------------------------- network and frame
def test_x3_networks_with_fused_and_unfused_tail_agree(golden):
    g = golden("g8_sr_x3_6x10")
    x = torch.from_numpy(g["x"]).cuda()
    m, mu = sr3(True), sr3(False)
    with torch.no_grad():
        fused, unfused = m(x), mu(x)
        dec, dec_u = m(x, decimate=True), mu(x, decimate=True)
    assert "tail_s3" in m._packed() and "tail_s3" not in mu._packed()
    rel = lambda a, ref: float((a.cpu() - torch.as_tensor(ref)).abs().max() / torch.as_tensor(ref).abs().max())
    assert rel(fused, g["out"]) < 2e-3 and rel(unfused, g["out"]) < 2e-3
    assert rel(fused, unfused.cpu()) < 1e-3 and rel(dec, dec_u.cpu()) < 1e-3
    assert torch.equal(dec, fused[..., ::3, ::3])


def test_x3_tail_entries_refuse_bad_arguments_without_launching():
    m = sr3()
    P = m._packed()
    a, b = _hid(1, 4, 6, 1), _hid(1, 4, 6, 2)
    cm = torch.zeros((24, 32), dtype=torch.float32, device="cuda")
    raw = _raw(1, 12, 18)
    lib = L.load_s3t()
    pa, pb, pc, pw, pr, null = L.dptr(a, torch.float16), L.dptr(b, torch.float16), L.dptr(cm), L.dptr(P["tail_s3"], torch.uint8), L.dptr(raw), ctypes.c_void_p(0)
    odd = ctypes.c_void_p(pa.value + 8)
    plain = [((null, pw, pr, 1, 4, 6, 4, 1, 0), b"null"), ((pa, null, pr, 1, 4, 6, 4, 1, 0), b"null"), ((pa, pw, null, 1, 4, 6, 4, 1, 0), b"null"),
             ((pa, pw, pr, 0, 4, 6, 4, 1, 0), b"bad shape"), ((pa, pw, pr, 1, -4, 6, 4, 1, 0), b"bad shape"), ((pa, pw, pr, 1, 4, 0, 4, 1, 0), b"bad shape"),
             ((pa, pw, pr, 1, 4, 6, -1, 1, 0), b"bad shape"), ((odd, pw, pr, 1, 4, 6, 4, 1, 0), b"aligned"),
             ((pa, pw, ctypes.c_void_p(pa.value), 1, 4, 6, 4, 1, 0), b"overlap"), ((pa, pw, ctypes.c_void_p(pa.value + 64), 1, 4, 6, 4, 1, 1), b"overlap")]
    fold = [((pa, null, pc, pw, pr, 1, 4, 6, 4, 1, 0), b"null"), ((pa, pb, null, pw, pr, 1, 4, 6, 4, 1, 0), b"null"),
            ((pa, pb, pc, pw, pr, 1, 4, 6, -2, 1, 0), b"bad shape"), ((pa, pb, pc, pw, ctypes.c_void_p(pb.value), 1, 4, 6, 4, 1, 0), b"overlap"),
            ((pa, pb, pc, pw, ctypes.c_void_p(pc.value), 1, 4, 6, 4, 1, 0), b"overlap")]
    for fn, cases in ((lib.vsr_s3t_sr_tail_f16, plain), (lib.vsr_s3t_sr_tail_fold_f16, fold)):
        for args, word in cases:
            rc = fn(*args, L.stream())
            assert rc < 0 and word in lib.vsr_s3t_last_error(), (args[3:], rc, lib.vsr_s3t_last_error())
            with pytest.raises(L.VsrHipError):
                L.check(rc, "sr_tail_s3_f16", lib=lib)
    torch.cuda.synchronize()
    assert bool(torch.isnan(raw).all())      # nothing was launched
    assert torch.isfinite(_tail(P, a, 4)).all()


def _vsr3(cpu_vsr):
    from video_super_resolution_amd import VSR
    m = VSR(upscale_factor=3).eval()
    m.load_state_dict({k: v for k, v in cpu_vsr.state_dict().items() if not k.startswith("model.")}, strict=False)
    fill_module_(m.model, seed=0, prefix="model.")
    m = m.cuda()
    m.precision = m.model.precision = "fp16"
    return m


def test_vsr_forward_x3_share_tail_bit_identical_and_fused_against_unfused_tail(cpu_vsr):
    """VSR.forward at LR 66 x 70, x3, fp16, first and recurrent call.  share_tail on (the three LR-frame planes' raw tail evaluated once,
    beside the pass-1 trunks) equals share_tail off bit for bit.  The fused tail against the unfused one: pass 2's guidance is discrete,
    so final frames are compared by PSNR (the bar of test_vsr_forward_x3_fused_against_unfused) and pass 1 on identical planes."""
    m = _vsr3(cpu_vsr)
    data = torch.from_numpy(np.random.RandomState(34).randint(0, 256, (3, 66, 70, 3)).astype(np.float32)).cuda()

    def run(tail, share, est1=None):
        m.model.fused_tail_s3, m.share_tail = tail, share
        m.model._pack = None
        outs, taps = [], []
        hf = torch.zeros(3, 198, 210, 3, device="cuda")
        L.TIMER.enabled, L.TIMER.only = True, None
        L.TIMER.reset()
        try:
            with torch.no_grad():
                for k in range(2):
                    m.plane_taps = {}
                    est = None if k == 0 else (est1 if est1 is not None else outs[0])
                    out, loss = m(data, None, hf, est, train=False)
                    assert loss is None
                    outs.append(out.clone())
                    taps.append(dict(m.plane_taps))
            torch.cuda.synchronize()
            names = L.TIMER.summary()
        finally:
            m.plane_taps = None
            L.TIMER.enabled = False
            L.TIMER.reset()
        assert ("tail_s3" in m.model._packed()) == tail
        return outs, taps, names
    on, t_on, n_on = run(True, True)
    off, t_off, n_off = run(True, False)
    for i in range(2):
        assert on[i].shape == (1, 198, 210, 3) and torch.isfinite(on[i]).all()
        assert torch.equal(on[i], off[i]), i
    # shared: one more launch per frame (the three planes ahead at full resolution, then the others in either pass)
    launches = lambda n: sum(v[0] for k, v in n.items() if k.startswith("sr_tail_s3"))
    assert launches(n_on) > launches(n_off) > 0 and not any(k.startswith("sr_convout_planes") for k in list(n_on) + list(n_off))
    uo, t_u, n_u = run(False, True, est1=on[0])
    assert launches(n_u) == 0 and any(k.startswith("sr_convout_planes") for k in n_u)
    for i in range(2):
        f, u = on[i], uo[i]
        assert torch.equal(t_on[i]["pass1_input"], t_u[i]["pass1_input"])
        a, b = t_on[i]["pass1_decimated"], t_u[i]["pass1_decimated"]
        assert (a - b).abs().max().item() <= 1e-3 * b.abs().max().item()
        psnr = 10 * np.log10(255.0 ** 2 / max(float(((f - u) ** 2).mean()), 1e-20))
        print(f"[x3 VSR.forward call {i}] fused vs unfused tail: PSNR(255) {psnr:.1f} dB, max {(f - u).abs().max().item():.3f}")
        assert psnr > 55.0, psnr
