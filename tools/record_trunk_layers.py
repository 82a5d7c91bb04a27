"""Records tests/golden/g14_trunk_layers.json: every distinct launch the three fp16 guidance executors (FlowNet2Exec, HourglassExec,
OSVOSExec) make through the trunk convolution entries at the sizes and batches of the BASELINE configurations C3-A, C3-B and C5, as
`VSR.forward` calls them -- the first call of a clip (no estimate yet), the recurrent call, and streaming mode (VSR.temporal_cache:
the trunks on a part of their batch under `_lib.route_batch`).

The three ctypes entries `vsr_conv2d_nhwc_sx_f16`, `vsr_conv2d_stem_f16` and `vsr_deconv4s2_nhwc_f16` are wrapped on the loaded library
object; a row is

    [entry kind (0 conv, 1 stem, 2 deconv4s2), the 23 non-pointer arguments in vsr_conv2d_plan's order, [route batch num, den],
     a split-K workspace was passed (0 / 1), its bytes, vsr_last_route() after the launch]

and the file holds the distinct rows, sorted, beside the routes that callers name themselves through `_lib.ROUTES` (`flow_head<..>`,
`hg_front`, `hg_inception<..>`).  A batch whose input exceeds what one launch addresses runs as sub-batches of whole images
(csrc/conv_igemm.hip for_sub_batches): the row then holds the batch of the LAST sub-batch, whose route `vsr_last_route()` names.

tests/test_conv_build_census.py replays the rows through the plan function on the CPU; run this again (and commit the file) when a
trunk, a trunk size or a routing rule changes -- the census says so.  Run by hand on a machine with the GPU; nothing in the suite runs
at these sizes.

    python tools/record_trunk_layers.py [--out tests/golden/g14_trunk_layers.json] [--configs C3A,C3B,C5]
"""
import argparse
import json
import os
import re
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "2")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch

from video_super_resolution_amd import VSR, _lib as L
from video_super_resolution_amd.weights import fill_module_

CONFIGS = {"C3A": (540, 960, 4), "C3B": (1080, 1920, 2), "C5": (2160, 3840, 2)}   # LR h, LR w, scale (bench.py CONFIGS)
SELF_NAMED = re.compile(r"flow_head<|hg_front$|hg_inception<")
GATHER_LIMIT = 0xFFFFFFFF   # csrc/conv_igemm.hip kGatherLimit

rows = set()
batch = [0, 0]


def _v(a):
    return a.value if hasattr(a, "value") else a


def _last_sub_batch(N, H, W, in_ld):
    """The batch of the last sub-batch for_sub_batches runs (N itself when the whole batch is one launch)."""
    img = H * W * in_ld
    per = (GATHER_LIMIT - 1) // (img * 2) if img * 2 * N >= GATHER_LIMIT else N
    return N - (N - 1) // per * per


def _wrap(lib, name, kind, plan_args):
    fn = getattr(lib, name)

    def entry(*a):
        rc = fn(*a)
        if rc == 0:
            args, ws, ws_bytes = plan_args([_v(x) for x in a])
            rows.add((kind, tuple(int(x) for x in args), tuple(batch), 1 if ws else 0, int(ws_bytes) if ws else 0, lib.vsr_last_route().decode()))
        return rc
    setattr(lib, name, entry)


def _conv(a):   # in, in_ld, in_coff, w, bias, out, out_ld, out_coff, N, H, W, cin, Ho, Wo, cout, cout_pad, kh, kw, stride, stride_x, pad_y, pad_x, outH, outW, oy.., ox.., act, slope, ws, bytes, stream
    in_ld, out_ld, out_coff, N, H, W = a[1], a[6], a[7], a[8], a[9], a[10]
    return [in_ld, _last_sub_batch(N, H, W, in_ld), H, W] + a[11:22] + [out_ld, out_coff] + a[22:28], a[30], a[31]


def _stem(a):   # in4, w, bias, out, out_ld, out_coff, N, H, W, Ho, Wo, cout, cout_pad, kh, kw, stride, pad_y, pad_x, act, slope, stream
    out_ld, out_coff, N, H, W, Ho, Wo, cout, cout_pad, kh, kw, stride, pad_y, pad_x = a[4:18]
    return [4, N, H, W, 32, Ho, Wo, cout, cout_pad, kh, kw, stride, 0, pad_y, pad_x, out_ld, out_coff, Ho, Wo, 1, 0, 1, 0], 0, 0


def _deconv(a):   # in, in_ld, in_coff, w4, bias, out, out_ld, out_coff, N, H, W, cin, cout, cout_pad, act, slope, ws, bytes, stream
    in_ld, out_ld, out_coff, N, H, W, cin, cout, cout_pad = a[1], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13]
    return [in_ld, _last_sub_batch(N, H, W, in_ld), H, W, cin, H, W, cout, cout_pad, 2, 2, 1, 0, 1, 1, out_ld, out_coff, 2 * H, 2 * W, 2, 0, 2, 0], a[16], a[17]


def _wrap_route_batch(lib):
    fn = lib.vsr_conv2d_route_batch

    def entry(num, den):
        rc = fn(num, den)
        if rc == 0:
            batch[:] = [int(num), int(den)]
        return rc
    lib.vsr_conv2d_route_batch = entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g14_trunk_layers.json"))
    ap.add_argument("--configs", default="C3A,C3B,C5")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    lib = L.load()
    _wrap(lib, "vsr_conv2d_nhwc_sx_f16", 0, _conv)
    _wrap(lib, "vsr_conv2d_stem_f16", 1, _stem)
    _wrap(lib, "vsr_deconv4s2_nhwc_f16", 2, _deconv)
    _wrap_route_batch(lib)
    L.ROUTES.enabled = True
    names = [c for c in args.configs.split(",") if c]
    for name in names:
        h, w, scale = CONFIGS[name]
        model = fill_module_(VSR(upscale_factor=scale).eval(), seed=0).to(dev)
        model.precision = model.model.precision = "fp16"
        clip = torch.randint(0, 256, (6, h, w, 3), generator=torch.Generator().manual_seed(1234), dtype=torch.int32).float().to(dev)
        hf = torch.zeros((3, scale * h, scale * w, 3), dtype=torch.float32, device=dev)
        with torch.no_grad():
            est, _ = model(clip[0:3], None, hf, None, train=False)        # the first call of a clip: plane 7 is frame 0
            est, _ = model(clip[1:4], None, hf, est, train=False)         # the recurrent call
            model.temporal_cache = True                                    # streaming: windows that share two frames with the one before
            for t in range(3):
                est, _ = model(clip[t:t + 3], None, hf, est, train=False)
            model.temporal_cache = False
            model.reset_temporal_cache()
        torch.cuda.synchronize()
        print(f"{name}: {len(rows)} distinct launches so far", flush=True)
        del model, clip, hf, est
        torch.cuda.empty_cache()
    named = sorted({r for _, r in L.ROUTES.calls if SELF_NAMED.match(r)})
    out = [[kind, list(a), list(b), has_ws, ws_bytes, route] for kind, a, b, has_ws, ws_bytes, route in sorted(rows)]
    with open(args.out, "w") as f:   # (one row per line)
        f.write('{"configs": %s,\n "self_named": %s,\n "rows": [\n' % (json.dumps(names), json.dumps(named)))
        f.write(",\n".join("  " + json.dumps(r) for r in out))
        f.write("\n ]}\n")
    print(f"{len(out)} rows, {len(named)} self-named routes -> {args.out}")


if __name__ == "__main__":
    main()
