"""The case tables of the exact-arithmetic trunk convolution tests (tests/test_gpu_exact_conv.py) as DATA, readable without a GPU:
tests/test_conv_build_census.py plans every row on the CPU and compares the kernel builds the rows reach with the builds the trunks
launch (tests/golden/g14_trunk_layers.json).

`exact_rows()` flattens the tables into rows (entry kind, shape, switch set, activation) exactly as the tests pair them; `plan_args`
turns a row's shape into the 23 arguments of `vsr_conv2d_plan`, built the way igemm.HConv / HConvStem / HDeconv4s2 / HConvPairS2 call
their entry for a dense destination of their own."""
from video_super_resolution_amd.igemm import ACT_LEAKY as LEAKY, ACT_NONE as NONE, ACT_RELU as RELU, _cout_pad, pad32

CONV, STEM, DECONV, PAIR = 0, 1, 2, 3   # entry kinds: vsr_conv2d_plan's codes; PAIR is the conv entry as igemm.HConvPairS2 calls it
ENTRY = {CONV: 0, STEM: 1, DECONV: 2, PAIR: 0}
ACTS = ((NONE, 0.1), (RELU, 0.1), (LEAKY, 0.25), (LEAKY, 0.1))     # none, ReLU, Leaky with a dyadic slope, Leaky 0.1 (restated, _exact.leaky_tenth_f16)

# ---------------------------------------------------------------------------------------------------------------- the gather kernel
SHAPES = [  # (N, cin, H, W, cout, k, stride, pad): ragged in every dimension the kernels tile
    (1, 1, 5, 7, 1, 3, 1, 1), (2, 31, 9, 6, 2, 3, 1, 1), (1, 33, 6, 11, 17, 3, 1, 1), (1, 65, 7, 5, 65, 1, 1, 0), (1, 97, 4, 9, 129, 3, 2, 1),
    (1, 64, 1, 23, 32, 3, 1, 1),      # one row
    (1, 32, 19, 1, 16, 5, 1, 2),      # one column
    (1, 16, 2, 2, 8, 7, 1, 3),        # an image smaller than the kernel's padding
    (3, 40, 5, 6, 24, 3, 1, 1),       # batch 3, a different image in each slot
    (1, 32, 8, 16, 64, 3, 1, 1),      # exactly one 128-pixel tile
    (1, 32, 3, 43, 64, 3, 1, 1),      # one tile plus one pixel
    (1, 1026, 4, 6, 2, 3, 1, 1),      # K = 9234: predict_flow (last chunk: channels 1024, 1025)
    (1, 473, 8, 16, 256, 3, 1, 1),    # FlowNetC conv3_1 (odd channel count), split-K by default
    (1, 1056, 6, 10, 128, 3, 1, 1),   # 32 k + 0 with a long K
    (2, 128, 17, 13, 128, 5, 2, 2),   # 5x5 stride 2
    (1, 12, 11, 9, 64, 11, 1, 5),     # 11x11
]

GATHER_ROUTES = {  # name -> (switches, pattern of the route string)
    "default": ((), r"(gather|tile)<"),
    "gather64": ((2000, 11), r"gather<(16|32|64)>"),
    "gather128": ((2000, 10), r"gather<"),
    "first_build": ((8,), r"gather<(16|32|64)>"),
    "ring5": ((2000, 11, 8002), r"gather<(16|32|64)>"),
}

SPLIT_K_SHAPES = [(1, 1026, 4, 6, 2, 3, 1, 1), (1, 473, 8, 16, 256, 3, 1, 1), (2, 512, 7, 9, 320, 3, 2, 1), (1, 97, 4, 9, 129, 3, 2, 1)]
SPLIT_K_FILLS = (1000, 1016, 1064, 1128, 1300, 1999)   # each under (2000, 11, fill)

# ---------------------------------------------------------------------------------------------------------------- the tile kernel
TILE_SHAPES = [
    (1, 256, 9, 13, 512, 3, 2, 1), (1, 473, 8, 16, 256, 3, 1, 1), (1, 33, 11, 12, 65, 3, 1, 1), (3, 160, 9, 7, 192, 1, 1, 0), (1, 1056, 6, 10, 128, 3, 1, 1),
    (1, 32, 8, 16, 64, 3, 1, 1), (1, 32, 3, 43, 64, 3, 1, 1), (1, 64, 1, 23, 64, 3, 1, 1), (1, 32, 19, 1, 128, 5, 1, 2), (2, 128, 17, 13, 128, 5, 2, 2),
    (1, 31, 20, 21, 70, 7, 1, 3),
]
TILE_WIDTHS, TILE_SPLITS = (64, 128), (1, 2, 3, 7)   # each under (2003, 4000 + width, 5000 + splits)

# ---------------------------------------------------------------------------------------------------------------- the LDS-patch kernels
PATCH_SHAPES = [  # (N, cin, H, W, cout, k): stride 1, pad k // 2; at least 4 x 16 outputs (the launcher's condition), ragged tiles
    (1, 64, 9, 21, 16, 11), (2, 33, 7, 40, 16, 7), (1, 31, 5, 17, 13, 5), (1, 96, 13, 19, 17, 3), (2, 65, 9, 33, 1, 3), (1, 194, 6, 18, 2, 3),
    (1, 64, 17, 16, 32, 7), (1, 64, 19, 33, 65, 5), (2, 64, 8, 50, 129, 3), (1, 32, 4, 16, 64, 3), (3, 97, 5, 17, 48, 3),
]
PATCH_ROUTES = {
    "patch_r8": ((2, 2000, 6000, 9000), r"patch_r8<|patch_rows<|patch<"),
    "patch_lw": ((2, 2000, 6002, 9000), r"patch_lw<|patch_r8<|patch_rows<|patch<"),
    "patch_pf64": ((2, 2000, 9002), r"patch_pf<|patch_r8<|patch_rows<|patch<"),
    "patch_pf32": ((2, 2000, 9003), r"patch_pf<|patch_r8<|patch_rows<|patch<"),
    "patch_rows": ((6, 2000), r"patch_rows<|patch<"),
    "patch": ((7, 2000), r"patch<"),
}

# ---------------------------------------------------------------------------------------------------------------- 1x1 streaming
C1_CASES = [  # (N, cin, H, W, cout, act, slope, out_coff, channels beyond the slice): each under 7000 and 7001
    (1, 128, 259, 271, 208, RELU, 0.1, 0, 0), (1, 96, 300, 230, 77, LEAKY, 0.1, 0, 0), (1, 128, 270, 250, 224, LEAKY, 0.5, 32, 32),
    (3, 33, 160, 140, 129, NONE, 0.1, 0, 0)]

# ---------------------------------------------------------------------------------------------------------------- other fp16 layers
STEM_CASES = [  # (N, cin, H, W, cout, k, stride, pad, act, slope)
    (2, 3, 13, 17, 128, 7, 1, 3, RELU, 0.1), (2, 3, 20, 30, 64, 7, 2, 3, LEAKY, 0.1), (1, 1, 9, 8, 17, 3, 1, 1, NONE, 0.1),
    (1, 4, 1, 20, 16, 5, 1, 2, LEAKY, 0.5), (1, 3, 270, 250, 128, 7, 1, 3, RELU, 0.1), (3, 2, 5, 1, 65, 7, 1, 3, NONE, 0.1)]
PAIR_CASES = [(2, 12, 16, 24, 64, 7, 3), (1, 12, 37, 50, 64, 7, 3), (1, 16, 20, 34, 33, 5, 2), (1, 5, 9, 8, 16, 3, 1), (3, 1, 2, 2, 1, 3, 1)]   # (N, cin, H, W, cout, k, pad): stride 2, Leaky 0.1
DECONV_SHAPES = [(1, 64, 7, 9, 32), (2, 1026, 4, 5, 129), (1, 33, 1, 30, 64), (1, 31, 19, 1, 2), (1, 32, 97, 130, 2), (2, 96, 11, 13, 192)]   # (N, cin, H, W, cout): Leaky 0.1
DECONV_MODES = ((), (1,), (2003,))

# ---------------------------------------------------------------------------------------------------------------- the route plan
PLAN_CONV = ([(SHAPES[i], m) for i, m in ((3, ()), (4, ()), (7, ()), (12, ()), (13, ()), (14, ()), (12, (2000, 11)), (13, (2000, 10)), (9, (8,)), (12, (2000, 11, 1300)))]
             + [(TILE_SHAPES[i], m) for i, m in ((0, (2003,)), (4, (2003, 4128, 5003)), (9, (2003, 4064, 5001)))]
             + [(PATCH_SHAPES[i] + (1, PATCH_SHAPES[i][5] // 2), PATCH_ROUTES[r][0]) for i, r in ((0, "patch_r8"), (6, "patch_lw"), (8, "patch_lw"), (7, "patch_pf64"),
                                                                                                (3, "patch_pf32"), (4, "patch_rows"), (1, "patch_rows"), (5, "patch"), (10, "patch_r8"))]
             + [((2, 64, 128, 240, 16, 3, 1, 1), ()), ((2, 32, 128, 240, 64, 3, 1, 1), ()),      # the smallest map with the patch family by heuristic: H * W >= 8192
                ((1, 128, 259, 271, 208, 1, 1, 0), ()), ((1, 128, 259, 271, 208, 1, 1, 0), (7001,))])
PLAN_STEM = [(2, 3, 13, 17, 128, 7, 1, 3), (2, 3, 20, 30, 64, 7, 2, 3), (1, 3, 270, 250, 128, 7, 1, 3)]
PLAN_DECONV = [((1, 64, 7, 9, 32), ()), ((2, 1026, 4, 5, 129), ()), ((2, 1026, 4, 5, 129), (1,)), ((2, 96, 11, 13, 192), (2003,)), ((1, 32, 97, 130, 2), ())]

# ---------------------------------------------------------------------------------------------------------------- one case per build
# One case per kernel build that the trunks launch (g14_trunk_layers.json) and no table above plans to: the smallest shape found with
# the plan function on the CPU that still has a ragged last tile in both directions and, where the kernel walks 32-channel chunks, a
# ragged last chunk.  (entry kind, shape, switch set, (activation, slope)); shape: CONV / STEM (N, cin, H, W, cout, k, stride, pad),
# DECONV (N, cin, H, W, cout).  tests/test_conv_build_census.py says which build a row is here for.
_R8 = PATCH_ROUTES["patch_r8"][0]
BUILD_CASES = [
    # k_conv_patch_r8's 16 x 32 output tile on 17 x 33 outputs (four tiles, the last of each direction one pixel wide); 13 -> 16 out-channels: MT 1
    (CONV, (1, 33, 17, 33, 13, 3, 1, 1), _R8, (RELU, 0.1)),                             # patch_r8<3,1>
    (CONV, (2, 33, 17, 33, 13, 7, 1, 3), _R8, (LEAKY, 0.25)),                           # patch_r8<7,1>
    (CONV, (1, 33, 17, 33, 13, 11, 1, 5), _R8, (LEAKY, 0.1)),                           # patch_r8<11,1>: the largest halo
    (CONV, (2, 33, 17, 33, 17, 11, 1, 5), _R8, (NONE, 0.1)),                            # patch_r8<11,2>
    (CONV, (1, 33, 17, 33, 33, 3, 1, 1), PATCH_ROUTES["patch_lw"][0], (RELU, 0.1)),     # patch_lw<3,4>: 33 -> 64 out-channels per workgroup
    # the gather kernel without split-K (1000: fill threshold 0) at the widths and (kh, stride) the trunks run it with; two 128-pixel tiles
    (CONV, (1, 33, 5, 17, 17, 1, 1, 0), (), (LEAKY, 0.1)),                              # gather<32> k1 s1
    (CONV, (1, 33, 9, 17, 65, 1, 1, 0), (2000, 10), (LEAKY, 0.25)),                     # gather<128> k1 s1
    (CONV, (1, 33, 9, 17, 65, 3, 1, 1), (2000, 10, 1000), (NONE, 0.1)),                 # gather<128> k3 s1
    (CONV, (2, 33, 19, 33, 65, 3, 2, 1), (2000, 10, 1000), (RELU, 0.1)),                # gather<128> k3 s2
    (CONV, (1, 33, 19, 33, 65, 5, 2, 2), (2000, 10, 1000), (LEAKY, 0.1)),               # gather<128> k5 s2
    (STEM, (1, 3, 9, 17, 33, 3, 1, 1), (), (RELU, 0.1)),                                # gather<64,stem> k3 s1
    # the tile kernel without split-K (5001)
    (CONV, (1, 40, 9, 17, 65, 1, 1, 0), (2003,), (RELU, 0.1)),                          # tile<128> k1 s1 (K too short to split)
    (CONV, (1, 33, 19, 33, 33, 3, 2, 1), (2003, 5001), (LEAKY, 0.1)),                   # tile<64> k3 s2
    (PAIR, (1, 12, 19, 34, 64, 7, 2, 3), (2003, 5001), (LEAKY, 0.1)),                   # tile<64> k7 s2: FlowNetS conv1 on pixel pairs
    (DECONV, (2, 33, 7, 19, 65), (2003,), (LEAKY, 0.1)),                                # deconv4s2 tile<128>
    (DECONV, (1, 129, 5, 9, 65), (2003,), (LEAKY, 0.1)),                                # deconv4s2 tile<128>+splitk
    # eight 32-channel chunks; the streaming build is chosen from 65,536 pixels and more than 64 out-channels
    (CONV, (1, 225, 259, 271, 65, 1, 1, 0), (), (RELU, 0.1)),                           # conv1x1_stream<8>
]


def exact_rows(build_cases=None):
    """Every (entry kind, shape, switch set, (activation, slope)) the exact tests run, shapes as 8-tuples (DECONV: 5-tuples; PAIR: stride 2)
    -- plus, for the 1x1 cases, (out_coff, channels beyond the slice) as a fifth element."""
    rows = []
    for name, (modes, _) in GATHER_ROUTES.items():
        rows += [(CONV, s, modes, ACTS[i % 4]) for i, s in enumerate(SHAPES)]
    rows += [(CONV, s, (2000, 11, fill), (LEAKY, 0.1)) for s in SPLIT_K_SHAPES for fill in SPLIT_K_FILLS]
    rows += [(CONV, s, (2003, 4000 + bn, 5000 + sp), ACTS[(i + 1) % 4]) for i, s in enumerate(TILE_SHAPES) for bn in TILE_WIDTHS for sp in TILE_SPLITS]
    for name, (modes, _) in PATCH_ROUTES.items():
        rows += [(CONV, s + (1, s[5] // 2), modes, ACTS[(i + 2) % 4]) for i, s in enumerate(PATCH_SHAPES)]
    for N, cin, H, W, cout, act, slope, coff, extra in C1_CASES:
        rows += [(CONV, (N, cin, H, W, cout, 1, 1, 0), (mode,), (act, slope), (coff, extra)) for mode in (7000, 7001)]
    rows += [(CONV, s, m, ACTS[i % 4]) for i, (s, m) in enumerate(PLAN_CONV)]
    rows += [(STEM, c[:8], (), c[8:]) for c in STEM_CASES] + [(STEM, c, (), (RELU, 0.1)) for c in PLAN_STEM]
    rows += [(PAIR, (N, cin, H, W, cout, k, 2, pad), (), (LEAKY, 0.1)) for N, cin, H, W, cout, k, pad in PAIR_CASES]
    rows += [(DECONV, s, m, (LEAKY, 0.1)) for s in DECONV_SHAPES for m in DECONV_MODES] + [(DECONV, s, m, (LEAKY, 0.1)) for s, m in PLAN_DECONV]
    return rows + list(BUILD_CASES if build_cases is None else build_cases)


def plan_args(kind, shape, out_coff=0, out_extra=0):
    """The 23 shape arguments of vsr_conv2d_plan (the header's order) for a row's shape, as the igemm class of its kind passes them."""
    if kind == DECONV:
        N, cin, H, W, cout = shape
        return (pad32(cin), N, H, W, pad32(cin), H, W, cout, _cout_pad(cout), 2, 2, 1, 0, 1, 1, pad32(out_coff + cout) + out_extra, out_coff, 2 * H, 2 * W, 2, 0, 2, 0)
    N, cin, H, W, cout, k, stride, pad = shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out_ld = pad32(out_coff + cout) + out_extra
    if kind == STEM:
        return (4, N, H, W, 32, Ho, Wo, cout, _cout_pad(cout), k, k, stride, 0, pad, pad, out_ld, out_coff, Ho, Wo, 1, 0, 1, 0)
    if kind == PAIR:   # pixel pairs: [N, H, W / 2, 32], the kernel columns folded into (pair tap, parity)
        p2 = (pad + 1) // 2
        kwp = (k - 1 + 2 * p2 - pad) // 2 + 1
        return (32, N, H, W // 2, 32, Ho, Wo, cout, _cout_pad(cout), k, kwp, 2, 1, pad, p2, out_ld, out_coff, Ho, Wo, 1, 0, 1, 0)
    return (pad32(cin), N, H, W, pad32(cin), Ho, Wo, cout, _cout_pad(cout), k, k, stride, 0, pad, pad, out_ld, out_coff, Ho, Wo, 1, 0, 1, 0)
