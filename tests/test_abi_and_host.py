"""CPU-side checks: the C-ABI library builds for gfx950, loads, and exports every symbol include/vsr_hip.h declares
(no compute without a GPU); host logic of the product modules (state_dict layout, caches, error behaviour)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from video_super_resolution_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_libraries_build_and_export_exactly_what_their_headers_declare():
    """libvsr_hip.so exports every entry include/vsr_hip.h declares (shipping kernels only: 66 -- round 4's 60 + vsr_sr_utd_post_f16,
    vsr_sr_utd4_f16, vsr_sr_utd_s2w_f16, vsr_sr_utd_s2_post_f16, vsr_sr_tail_s2_fold_f16 and vsr_conv2d_route_batch, all called by the package) and NONE of the cross-check surface; libvsr_hip_xcheck.so exports both
    headers' entries."""
    path = _lib.build()
    assert os.path.exists(path) and os.path.exists(_lib.XLIB_PATH)
    lib, xlib = ctypes.CDLL(path), ctypes.CDLL(_lib.XLIB_PATH)
    declared, xdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True)
    assert 20 <= len(declared) <= 66 and "vsr_resample2d_f32" in declared and "vsr_sr_utd_f16" in declared, len(declared)
    assert "vsr_conv2d_tuning" in xdeclared and "vsr_sr_utd_variant" in xdeclared and not set(declared) & set(xdeclared)
    assert not [s for s in declared if not hasattr(lib, s)]
    assert not [s for s in declared + xdeclared if not hasattr(xlib, s)]
    assert not [s for s in xdeclared if hasattr(lib, s)]            # the shipping library holds no switch, no superseded build
    exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    extra = sorted(set(ln.split()[-1] for ln in exported.splitlines() if " T vsr_" in ln) - set(declared))
    assert not extra, extra                                          # ... and nothing the header does not declare
    assert lib.vsr_abi_version() == 3 and xlib.vsr_abi_version() == 3
    lib.vsr_sr_query.restype = ctypes.c_size_t
    assert lib.vsr_sr_query(_lib.Q_UTD_BLOB_BYTES) % 16 == 0 and lib.vsr_sr_query(_lib.Q_UTD_STRIP_WIDTH) == 31
    # code object is built for gfx950 only
    out = subprocess.run(["strings", path], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_argument_validation_without_a_gpu():
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    assert lib.vsr_resample2d_f32(null, null, null, 1, 3, 8, 8, 1, 1, null) == -1  # VSR_E_ARG, nothing launched
    assert b"null" in lib.vsr_last_error()
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.vsr_correlation_out_shape(64, 120, 20, 1, 20, 1, 2, ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oc.value, oh.value, ow.value) == (441, 64, 120)  # reference correlation_cuda.cc:31-34 at 960x512 / 8


def test_conv_launcher_refuses_an_image_beyond_its_32_bit_offsets():
    """The gather kernels address their input with 32-bit byte offsets: a batch beyond 4 GiB is split into whole images
    by the launcher, and ONE image beyond 4 GiB is refused before anything is launched (it used to wrap)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)   # never dereferenced on the host; the call must fail before any launch
    H = W = 32768                    # 32768^2 pixels x 32 channels x 2 bytes = 64 GiB
    rc = lib.vsr_conv2d_nhwc_sx_f16(fake, 32, 0, fake, None, fake, 32, 0, 1, H, W, 32, H // 2, W // 2, 32, 32, 3, 3, 2, 0, 1, 1,
                                    H // 2, W // 2, 1, 0, 1, 0, 0, ctypes.c_float(0.0), None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"4 GiB" in lib.vsr_last_error()
    ph = (ctypes.c_void_p * 4)(0x1000, 0x1000, 0x1000, 0x1000)
    rc = lib.vsr_deconv4s2_nhwc_f16(fake, 32, 0, ph, None, fake, 32, 0, 1, H, W, 32, 32, 32, 0, ctypes.c_float(0.0), None,
                                    ctypes.c_size_t(0), None)
    assert rc == -1 and b"4 GiB" in lib.vsr_last_error()


def test_osvos_fuse_refuses_bad_branch_lists_before_any_launch():
    """vsr_osvos_fuse_f16: 0 or 5 branches, a leading dimension of 12, a branch whose upsampled size (hs + 1) s is below the output -- each
    is VSR_E_ARG with its own text (a launch would have returned 0 or VSR_E_LAUNCH)."""
    lib = _lib.load()
    vp, ip = ctypes.c_void_p * 5, ctypes.c_int * 5
    ptrs, out = vp(*[0x1000] * 5), ctypes.c_void_p(0x1000)   # never dereferenced on the host
    hs, ws, st = ip(9, 5, 3, 2, 1), ip(17, 9, 5, 3, 2), ip(2, 4, 8, 16, 32)

    def call(nb, ld=16, h=17, w=33, hs=hs):
        return lib.vsr_osvos_fuse_f16(ptrs, hs, ws, ld, ptrs, st, nb, ctypes.c_float(0.0), out, 2, h, w, None)
    for nb in (0, 5):
        assert call(nb) == -1 and b"osvos_fuse: bad arguments" in lib.vsr_last_error()
    assert call(4, ld=12) == -1 and b"osvos_fuse: bad arguments" in lib.vsr_last_error()
    assert call(4, hs=ip(9, 3, 3, 2, 1)) == -1 and b"branch 1 upsamples to 16x40 < 17x33" in lib.vsr_last_error()
    assert call(4, w=37) == -1 and b"branch 0 upsamples to 20x36 < 17x37" in lib.vsr_last_error()


def test_resize_add_segs_refuses_bad_segment_lists_before_any_launch():
    """vsr_resize_add_segs_nhwc_f16: an upsampled addend with an odd output size or without an addend, 5 segments, a segment width that is
    not a multiple of 8, a channel offset beyond the leading dimension -- each is VSR_E_ARG with its own text, nothing launched."""
    lib = _lib.load()
    vp, ip = ctypes.c_void_p * 5, ctypes.c_int * 5
    ptrs, out = vp(*[0x1000] * 5), ctypes.c_void_p(0x1000)

    def call(a_nseg=2, b_nseg=2, b_up2=0, H=10, W=12, C=32, a_lds=ip(*[24] * 5), a_coffs=ip(*[8] * 5), b_lds=ip(*[40] * 5), b_coffs=ip(*[16] * 5)):
        return lib.vsr_resize_add_segs_nhwc_f16(ptrs, a_lds, a_coffs, a_nseg, 5, 6, 0, ptrs if b_nseg else None, b_lds if b_nseg else None,
                                                b_coffs if b_nseg else None, b_nseg, b_up2, out, 1, H, W, C, None)
    for kw in (dict(b_up2=1, H=11), dict(b_up2=1, W=13), dict(b_up2=1, b_nseg=0)):
        assert call(**kw) == -1 and b"resize_add_segs: up2 flags" in lib.vsr_last_error(), kw
    for kw in (dict(a_nseg=5), dict(b_nseg=5)):
        assert call(**kw) == -1 and b"resize_add_segs: bad segment lists" in lib.vsr_last_error(), kw
    for kw in (dict(a_nseg=4, C=48), dict(b_nseg=4, C=48), dict(a_nseg=1, b_nseg=1, C=20)):
        assert call(**kw) == -1 and b"multiple of 8" in lib.vsr_last_error(), kw
    assert call(a_coffs=ip(8, 16, 8, 8, 8)) == -1 and b"resize_add_segs: segment 1 of a" in lib.vsr_last_error()      # 16 + 16 > 24
    assert call(b_coffs=ip(32, 16, 16, 16, 16)) == -1 and b"resize_add_segs: segment 0 of b" in lib.vsr_last_error()  # 32 + 16 > 40
    assert call(a_lds=ip(24, 24, 24, 24, 24), a_coffs=ip(8, 32, 8, 8, 8)) == -1 and b"segment 1 of a" in lib.vsr_last_error()  # coff beyond ld


def test_sr_state_dict_has_the_reference_layout(cpu_vsr):
    sd = cpu_vsr.model.state_dict()
    expect = {"sub_mean.weight": (3, 3, 1, 1), "conv_in.0.weight": (128, 3, 3, 3), "conv_in.1.weight": (1,),
              "feat_in.0.weight": (32, 128, 1, 1), "block.compress_in.0.weight": (32, 64, 1, 1),
              "block.upBlocks.5.0.weight": (32, 32, 8, 8), "block.downBlocks.0.0.bias": (32,),
              "block.uptranBlocks.4.0.weight": (32, 192, 1, 1), "block.downtranBlocks.0.0.weight": (32, 64, 1, 1),
              "block.compress_out.0.weight": (32, 192, 1, 1), "out.0.weight": (32, 32, 8, 8), "out.1.weight": (1,),
              "conv_out.0.weight": (3, 32, 3, 3), "add_mean.bias": (3,), "fc.0.weight": (32, 8), "fc.2.weight": (1, 32)}
    for k, shp in expect.items():
        assert tuple(sd[k].shape) == shp, k
    assert sum(v.numel() for v in sd.values()) == 910871
    # the whole module tree, loss networks included: 1246 entries / 228,750,548 parameters, key for key the reference's
    # `VSR().state_dict()` (compared with the imported reference in the development container)
    assert len(cpu_vsr.state_dict()) == 1246 and {"model", "FlowModule", "DepthModule", "VOSModule", "SR_loss", "Flow_loss",
                                                  "loss4object"} == {k.split(".")[0] for k in cpu_vsr.state_dict()}
    assert sum(p.numel() for p in cpu_vsr.parameters()) == 228750548


def test_synthetic_weights_are_name_keyed_and_reproducible(cpu_vsr):
    from video_super_resolution_amd import SRProjectionModule
    from video_super_resolution_amd.weights import fill_module_
    a = fill_module_(SRProjectionModule(), seed=0, prefix="model.").state_dict()
    for k, v in a.items():
        assert torch.equal(v, cpu_vsr.model.state_dict()[k]), k
    b = fill_module_(SRProjectionModule(), seed=1, prefix="model.").state_dict()
    assert not torch.equal(a["conv_in.0.weight"], b["conv_in.0.weight"])
    assert torch.equal(a["sub_mean.bias"], b["sub_mean.bias"])  # frozen MeanShift is never regenerated


def test_product_refuses_cpu_execution(cpu_vsr):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu_vsr(torch.zeros(3, 64, 64, 3), None, None, None, train=False)
    with pytest.raises(_lib.VsrHipError):
        cpu_vsr.model(torch.zeros(8, 3, 4, 4))
    with pytest.raises(ValueError):
        cpu_vsr(torch.zeros(2, 64, 64, 3), None, None, None, train=False)


def test_unsupported_geometries_fail_loudly():
    from video_super_resolution_amd import SRProjectionModule
    with pytest.raises(NotImplementedError):
        SRProjectionModule(upscale_factor=8)  # 4 = the reference; 2 / 3 = the scale extension (tests/test_gpu_sr_scale.py)
    with pytest.raises(NotImplementedError):
        SRProjectionModule(num_features=16)


def test_import_path_shim_and_train_mode_keeps_guidance_frozen(cpu_vsr):
    from network.video_super_resolution import VSR
    assert VSR is type(cpu_vsr)
    import copy
    m = copy.copy(cpu_vsr)
    m.train()
    assert not m.DepthModule.training and not m.FlowModule.training and not m.VOSModule.training
    m.eval()


def test_chunk_channel_order_is_a_permutation():
    from video_super_resolution_amd.sr_pack import _chunk_channel_order
    p = _chunk_channel_order("cpu")
    assert sorted(p.reshape(-1).tolist()) == list(range(32))
    assert p[1].tolist() == [4, 5, 6, 7, 20, 21, 22, 23]


def test_batchnorm_folding_is_exact(cpu_vsr):
    """The trunk executors fold eval-mode BatchNorm into the preceding conv (trunk_exec._fold): same function."""
    import torch.nn as nn
    import torch.nn.functional as F
    from video_super_resolution_amd.trunk_exec import _fold
    netg = cpu_vsr.DepthModule.model.netG
    assert sum(isinstance(m, nn.BatchNorm2d) for m in netg.modules()) == 155
    conv, bn = netg[0], netg[1]  # stem: affine BatchNorm
    blk = netg[3][0][0][1][1]    # an inception branch: conv -> BN(affine=False) -> ReLU -> conv -> BN -> ReLU
    x = torch.from_numpy(np.random.RandomState(0).randn(1, 3, 12, 14).astype(np.float32))
    with torch.no_grad():
        for c, b, inp in ((conv, bn, x), (blk[0], blk[1], torch.randn(1, 128, 6, 7)), (blk[3], blk[4], torch.randn(1, 32, 6, 7))):
            w, bias = _fold(c, b)
            ref = b(c(inp))
            got = F.conv2d(inp, w, bias, padding=c.padding)
            assert (ref - got).abs().max() <= 1e-5 * ref.abs().max()


def test_package_never_touches_the_checker():
    """The product may not import, call or even name `oracle/` (test infrastructure): a product path that routes through
    the checker would void every parity claim.  Plain-word search over every source file of the package."""
    import re
    pkg = os.path.join(ROOT, "video_super_resolution_amd")
    hits = []
    for dirpath, _, files in os.walk(pkg):
        if "__pycache__" in dirpath or os.sep + "build" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".c", "Makefile")):
                with open(os.path.join(dirpath, f), errors="replace") as fh:
                    for n, line in enumerate(fh, 1):
                        if re.search(r"\boracle\b", line, re.I):
                            hits.append(f"{os.path.relpath(os.path.join(dirpath, f), ROOT)}:{n}")
    assert not hits, hits


def test_video_dataset_takes_one_clip_as_one_clip():
    """VideoDataset(videos=<one ndarray [T,H,W,3]>) is ONE clip, not T one-frame clips."""
    from video_super_resolution_amd import driver
    clip = np.zeros((40, 8, 8, 3), np.uint8)
    ds = driver.VideoDataset(clip)
    assert len(ds) == 21
    item = ds[0]
    assert len(item) == 2 and np.asarray(item[0]).shape == (3, 8, 8, 3)


def test_float32_trunk_host_logic_on_the_cpu():
    """trunk_f32 without a GPU: the router's decisions on the layers it was tuned on, FusedSequential == nn.Sequential on CPU tensors
    (child by child: no own kernel runs there), the folded BatchNorm's scale / shift, the fused downtran's fragment layout."""
    import torch
    import torch.nn as nn
    from video_super_resolution_amd import depth, trunk_f32
    from video_super_resolution_amd.sr import pack_dt_frags
    R = trunk_f32._route
    assert R(4, 64, 540, 960, 16, 11, 11, 1, 5, 5) == trunk_f32.SPATIAL_K      # thin 11x11 at full resolution
    assert R(4, 32, 270, 480, 32, 7, 7, 1, 3, 3) == trunk_f32.SPATIAL_K        # 32 out-channels from 5x5 up
    assert R(4, 32, 270, 480, 32, 3, 3, 1, 1, 1) == trunk_f32.FLAT             # ... not 3x3
    assert R(2, 512, 68, 120, 512, 3, 3, 1, 1, 1) == trunk_f32.FLAT            # thick layers: the flat kernel
    assert R(2, 1024, 8, 15, 1024, 3, 3, 1, 1, 1) == trunk_f32.STOCK           # a few dozen workgroups: the stock operator
    assert R(2, 1026, 16, 30, 2, 3, 3, 1, 1, 1) == trunk_f32.FLAT              # predict_flow: the K-sharing head kernel behind the flat route
    assert R(4, 3, 540, 960, 128, 7, 7, 1, 3, 3) == trunk_f32.SPATIAL_K        # the hourglass stem
    assert R(2, 64, 512, 960, 64, 3, 3, 2, 1, 1) == trunk_f32.FLAT             # stride 2 never goes to the spatial kernels
    torch.manual_seed(0)
    blk = depth._build(depth._H).eval()
    ref = nn.Sequential(*[nn.Sequential(*list(b)) for b in blk])               # the same children as plain containers
    x = torch.randn(1, 128, 9, 11)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
        assert torch.equal(blk(x), torch.cat([b(x) for b in ref], 1))
        conv, bn = blk[1][3], blk[1][4]
        scale, shift = trunk_f32._Folded().get(conv, bn)
        y = conv(blk[1][:3](x))
        assert torch.allclose(bn(y), (y - conv.bias.view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), atol=1e-5)
    w = torch.arange(32 * 96, dtype=torch.float32).view(32, 96)
    fr = pack_dt_frags(w, 32)
    assert fr.shape == (16, 64)
    for r, lane in ((0, 0), (5, 37), (15, 63), (9, 31)):
        assert fr[r, lane] == w[lane % 32, 32 + 8 * (r // 4) + 4 * (lane // 32) + r % 4]


def test_executor_cache_sees_in_place_updates_and_replaced_parameters():
    """TrunkExecCache (one look-up per trunk call, ~6 per frame): the executor is rebuilt when a parameter / buffer is updated in place
    (version counter), when a Parameter object is replaced, and not otherwise."""
    import torch.nn as nn
    from video_super_resolution_amd.trunk_exec import TrunkExecCache
    net = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Sequential(nn.Conv2d(4, 2, 1, bias=False)))
    built = []
    cache = TrunkExecCache(net, lambda m: built.append(1) or object())
    a = cache.get()
    assert cache.get() is a and len(built) == 1
    with torch.no_grad():
        net[2][0].weight.mul_(2.0)                        # optimizer-style in-place update
    b = cache.get()
    assert b is not a and cache.get() is b and len(built) == 2
    net[1].running_mean.add_(1.0)                         # a buffer
    assert cache.get() is not b and len(built) == 3
    net[0].bias = nn.Parameter(torch.zeros(4))            # a replaced Parameter object
    c = cache.get()
    assert len(built) == 4 and cache.get() is c
    net.load_state_dict(net.state_dict())                 # copies in place: every version moves
    assert cache.get() is not c and len(built) == 5


def test_graph_replay_wrapper_refuses_what_it_cannot_replay(cpu_vsr):
    """GraphedVSR is for inference calls on the GPU: a training call, a target, streaming mode or CPU tensors fail loudly (no eager or CPU
    fallback behind it)."""
    from video_super_resolution_amd import GraphedVSR
    g = GraphedVSR(cpu_vsr)
    data = torch.zeros((3, 8, 8, 3))
    with pytest.raises(ValueError):
        g(data, None, None, None, train=True)
    with pytest.raises(ValueError):
        g(data, torch.zeros((1, 32, 32, 3)), None, None, train=False)
    with pytest.raises(RuntimeError):
        g(data, None, None, None, train=False)
    cpu_vsr.temporal_cache = True
    try:
        with pytest.raises(ValueError):
            g(data, None, None, None, train=False)
    finally:
        cpu_vsr.temporal_cache = False
