"""Launches of one SRProjectionModule forward on the fp16 path, per timer name, against a recorded table.

Which kernels a forward launches, and how often, is pure host logic (sr.py: the route rule, the plane chunks, the tail choice), so the
comparison is equality.  `EXPECTED` was recorded with this file's `_counts` at the commit before the host path was folded into one
stage launcher / one route rule (the parent of the commit that added this file) and pasted in as literals.

Shapes: LR height 5, LR width = the scale's strip width + 3 (a ragged second strip).  The forward takes the 8 planes the fusion MLP is
defined over (`vsr_sr_fc_planes_skip*` refuses any other count); the sharing cases evaluate the first 3 of them ahead, so the timer
names carry `_p3_side` and `_p5`.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_H = 5
_TAPS, _PLAIN = "taps", "plain"


def _cases():
    """(scale, num_groups, fuse_uptran, fold_chain, taps, decimate, ahead)"""
    out = []
    for scale in (2, 3, 4):
        for fold in ((False, True) if scale == 3 else (False,)):
            for uptran in (True, False):
                for taps in (False, True):
                    for decimate in (False, True):
                        out.append((scale, 6, uptran, fold, taps, decimate, False))
        out.append((scale, 9, True, False, False, False, False))      # compress_out with three live inputs
        out.append((scale, 6, True, False, False, False, True))       # precompute_shared, then the call that shares
    out.append((3, 6, True, True, False, False, True))
    return out


_modules = {}


def _module(scale, groups):
    from video_super_resolution_amd import SRProjectionModule
    from video_super_resolution_amd.weights import fill_module_
    if (scale, groups) not in _modules:
        _modules[scale, groups] = fill_module_(SRProjectionModule(upscale_factor=scale, num_groups=groups).eval(), seed=0, prefix="model.").cuda()
    return _modules[scale, groups]


def _width(scale):
    from video_super_resolution_amd import _lib as L
    if scale == 3:
        return int(L.load_s3().vsr_s3_query(L.Q_S3_STRIP_WIDTH)) + 3
    return int(L.load().vsr_sr_query(L.Q_UTD_S2_STRIP_WIDTH if scale == 2 else L.Q_UTD_STRIP_WIDTH)) + 3


def _counts(case):
    """{timer name: launches} of the forward(s) of `case`."""
    from video_super_resolution_amd import _lib as L
    scale, groups, uptran, fold, taps, decimate, ahead = case
    m = _module(scale, groups)
    m.fuse_uptran, m.fold_chain = uptran, fold
    w = _width(scale)
    x = torch.from_numpy(np.random.RandomState(scale).randint(0, 256, (8, 3, _H, w)).astype(np.float32)).cuda()
    with torch.no_grad():
        m(x)   # packs the weights and evaluates the constant map: neither belongs to the count
        torch.cuda.synchronize()
        L.TIMER.reset()
        L.TIMER.enabled, L.TIMER.only = True, None
        try:
            if ahead:
                shared = {"n": 3}
                live = {k: torch.empty((8, _H * w, 32), dtype=torch.float16, device="cuda") for k in (3, 6)}
                live["prefc"] = torch.empty((8, 3, scale * _H, scale * w), dtype=torch.float32, device="cuda")
                m.precompute_shared(x[:3].contiguous(), shared, live)
                m(x, decimate=decimate, shared=shared)
            else:
                m(x, taps={} if taps else None, decimate=decimate)
            torch.cuda.synchronize()
            return {k: v[0] for k, v in sorted(L.TIMER.summary().items())}
        finally:
            L.TIMER.enabled = False
            L.TIMER.reset()


def _id(case):
    scale, groups, uptran, fold, taps, decimate, ahead = case
    return f"x{scale}-g{groups}-{'post' if uptran else 'chain'}-{'fold' if fold else 'nofold'}-{_TAPS if taps else _PLAIN}-{'dec' if decimate else 'full'}" + ("-ahead" if ahead else "")


EXPECTED = {
    "x2-g6-post-nofold-plain-full": {"sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g6-post-nofold-plain-dec": {"sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_dec_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g6-post-nofold-taps-full": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g6-post-nofold-taps-dec": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_dec_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g6-chain-nofold-plain-full": {"sr_chain1x1_f16 x1": 3, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g6-chain-nofold-plain-dec": {"sr_chain1x1_f16 x1": 3, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_dec_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g6-chain-nofold-taps-full": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g6-chain-nofold-taps-dec": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_dec_f16": 1, "sr_utd_s2_f16": 6},
    "x2-g9-post-nofold-plain-full": {"sr_chain1x1_f16 x2": 3, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s2_f16": 1, "sr_utd_s2_f16": 9},
    "x2-g6-post-nofold-plain-full-ahead": {"sr_chain1x1_f16 x2": 2, "sr_chain1x1_f16 x3": 4, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 2, "sr_tail_s2_f16": 2, "sr_utd_s2_f16_p3_side": 6, "sr_utd_s2_f16_p5": 6},
    "x3-g6-post-nofold-plain-full": {"sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_post_f16": 3},
    "x3-g6-post-nofold-plain-dec": {"sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_post_f16": 3},
    "x3-g6-post-nofold-taps-full": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_post_f16": 3},
    "x3-g6-post-nofold-taps-dec": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_post_f16": 3},
    "x3-g6-chain-nofold-plain-full": {"sr_chain1x1_f16 x1": 3, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 6},
    "x3-g6-chain-nofold-plain-dec": {"sr_chain1x1_f16 x1": 3, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 6},
    "x3-g6-chain-nofold-taps-full": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 6},
    "x3-g6-chain-nofold-taps-dec": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 6},
    "x3-g6-post-fold-plain-full": {"sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_pre_f16": 3},
    "x3-g6-post-fold-plain-dec": {"sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_pre_f16": 3},
    "x3-g6-post-fold-taps-full": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_post_f16": 3},
    "x3-g6-post-fold-taps-dec": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_post_f16": 3},
    "x3-g6-chain-fold-plain-full": {"sr_chain1x1_f16 x1": 3, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_pre_f16": 3},
    "x3-g6-chain-fold-plain-dec": {"sr_chain1x1_f16 x1": 3, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_pre_f16": 3},
    "x3-g6-chain-fold-taps-full": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 6},
    "x3-g6-chain-fold-taps-dec": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_dec_f16": 1, "sr_utd_s3_f16": 6},
    "x3-g9-post-nofold-plain-full": {"sr_chain1x1_f16 x2": 3, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 1, "sr_tail_s3_f16": 1, "sr_utd_s3_f16": 3, "sr_utd_s3_post_f16": 6},
    "x3-g6-post-nofold-plain-full-ahead": {"sr_chain1x1_f16 x2": 2, "sr_chain1x1_f16 x3": 4, "sr_fc_planes_skip_scale": 1, "sr_head_f16": 2, "sr_tail_s3_f16": 2, "sr_utd_s3_f16_p3_side": 3, "sr_utd_s3_f16_p5": 3, "sr_utd_s3_post_f16_p3_side": 3, "sr_utd_s3_post_f16_p5": 3},
    "x4-g6-post-nofold-plain-full": {"sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip": 1, "sr_head_f16": 1, "sr_tail_f16": 1, "sr_utd_f16": 6},
    "x4-g6-post-nofold-plain-dec": {"sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_dec": 1, "sr_head_f16": 1, "sr_tail_dec_f16": 1, "sr_utd_f16": 6},
    "x4-g6-post-nofold-taps-full": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_head_f16": 1, "sr_tail_f16": 1, "sr_utd_f16": 6},
    "x4-g6-post-nofold-taps-dec": {"sr_chain1x1_f16 x1": 1, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_head_f16": 1, "sr_tail_dec_f16": 1, "sr_utd_f16": 6},
    "x4-g6-chain-nofold-plain-full": {"sr_chain1x1_f16 x1": 3, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip": 1, "sr_head_f16": 1, "sr_tail_f16": 1, "sr_utd_f16": 6},
    "x4-g6-chain-nofold-plain-dec": {"sr_chain1x1_f16 x1": 3, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_fc_planes_skip_dec": 1, "sr_head_f16": 1, "sr_tail_dec_f16": 1, "sr_utd_f16": 6},
    "x4-g6-chain-nofold-taps-full": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_head_f16": 1, "sr_tail_f16": 1, "sr_utd_f16": 6},
    "x4-g6-chain-nofold-taps-dec": {"sr_chain1x1_f16 x1": 4, "sr_chain1x1_f16 x2": 1, "sr_chain1x1_f16 x3": 2, "sr_head_f16": 1, "sr_tail_dec_f16": 1, "sr_utd_f16": 6},
    "x4-g9-post-nofold-plain-full": {"sr_chain1x1_f16 x2": 3, "sr_fc_planes_skip": 1, "sr_head_f16": 1, "sr_tail_f16": 1, "sr_utd_f16": 9},
    "x4-g6-post-nofold-plain-full-ahead": {"sr_chain1x1_f16 x2": 2, "sr_chain1x1_f16 x3": 4, "sr_fc_planes_skip": 1, "sr_head_f16": 2, "sr_tail_f16_p3": 1, "sr_tail_f16_p5": 1, "sr_utd_f16_p3_side": 6, "sr_utd_f16_p5": 6},
    "x3-g6-post-fold-plain-full-ahead": {"sr_fc_planes_skip_scale": 1, "sr_head_f16": 2, "sr_tail_s3_f16": 2, "sr_utd_s3_f16_p3_side": 3, "sr_utd_s3_f16_p5": 3, "sr_utd_s3_pre_f16_p3_side": 3, "sr_utd_s3_pre_f16_p5": 3},
}


def test_table_covers_every_case():
    assert sorted(EXPECTED) == sorted(_id(c) for c in _cases())


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_launch_counts(case):
    assert _counts(case) == EXPECTED[_id(case)]
