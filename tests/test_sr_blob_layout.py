"""The weight blobs of the fused SR kernels, byte for byte, against tests/golden/g12_sr_blobs.json: the SHA-256, shape and dtype of every
blob `SRProjectionModule._packed()` builds for upscale factors 4, 2, 3 and 3, 6, 9 groups (x2 also with the wide stage build), and of the
two packers it does not reach.  A blob's byte layout is the contract with a hand-scheduled kernel that reads its fragments from fixed
offsets; the table was recorded BEFORE the packers moved out of sr.py, from the seeded synthetic weights (all non-zero: a misplaced
section changes a digest).  No kernel of the project runs; packing needs the main library and the x3 side libraries for their sizes."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from video_super_resolution_amd import SRProjectionModule
from video_super_resolution_amd.sr_pack import pack_dt_frags, pack_utd_s3_post_blob
from video_super_resolution_amd.weights import fill_module_

_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_sr_blobs.json")


def _entry(t):
    raw = t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()
    return {"sha256": hashlib.sha256(raw).hexdigest(), "shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", "")}


def _record(out, name, v):
    v = getattr(v, "blob", v)   # a stage object carries its blob
    if torch.is_tensor(v) and v.dtype in (torch.uint8, torch.float16):
        assert name not in out
        out[name] = _entry(v)


def _module(S, G, device):
    return fill_module_(SRProjectionModule(upscale_factor=S, num_groups=G).eval(), seed=0, prefix="model.").to(device)


def collect(device):
    """{name: {"sha256", "shape", "dtype"}} of every packed blob, e.g. "x3/G6/stage_pre[0]"; "x2w": x2 with utd_s2_build = 2."""
    out = {}
    for S, wide in ((4, False), (2, False), (2, True), (3, False)):
        for G in (3, 6, 9):
            m = _module(S, G, device)
            if wide:
                m.utd_s2_build = 2   # the layout=4 fragments of k_utd_s2w
            P = m._packed()
            prefix = f"x{S}{'w' if wide else ''}/G{G}"
            for k, v in P.items():
                if isinstance(v, dict):
                    for j, e in v.items():
                        _record(out, f"{prefix}/{k}[{j}]", e)
                else:
                    _record(out, f"{prefix}/{k}", v)
            if (S, G) == (3, 6):
                # the POST blob packed in one call equals the one the module appends to its plain stage
                b = m.block
                up, dn = b.upBlocks[1], b.downBlocks[2]
                direct = pack_utd_s3_post_blob(up[0].weight, up[0].bias, P["up_a"][1], P["dt_w"][1], 64, P["dt_b"][1], P["dt_a"][1],
                                               dn[0].weight, dn[0].bias, P["dn_a"][2], post=(P["ut_w"][3], 128, P["ut_b"][3], P["ut_a"][3]))
                assert torch.equal(direct, P["stage_post"][0].blob)
                out["direct/utd_s3_post"] = _entry(direct)
    w = torch.from_numpy(np.random.RandomState(12).uniform(-1.0, 1.0, (32, 96)).astype(np.float32)).to(device)
    for col in (32, 64):
        out[f"direct/dt_frags[{col}]"] = _entry(pack_dt_frags(w, col))
    return out


def _compare(got):
    with open(_TABLE) as f:
        want = json.load(f)
    assert set(got) == set(want), f"only packed: {sorted(set(got) - set(want))}; only recorded: {sorted(set(want) - set(got))}"
    differ = {n: (got[n], want[n]) for n in sorted(want) if got[n] != want[n]}
    assert not differ, "\n".join(f"{n}: packed {g}, recorded {w}" for n, (g, w) in differ.items())


def test_blobs_are_the_bytes_recorded_before_the_packers_moved():
    _compare(collect("cpu"))


_TAP_TABLE_MAIN = r"""
#include <cstdio>
#include "sr_s3_taps.h"
int main() {
    const int ds[3] = {1, 0, -1};
    for (int wv = 0; wv < 4; ++wv)
        for (int p = 0; p < ph_cnt(wv); ++p)
            for (int dy : ds)
                for (int dx : ds) {
                    const int r = ph_r(wv, p), c = ph_c(wv, p);
                    if (tap_ok(r, dy) && tap_ok(c, dx)) std::printf("%d %d %d %d\n", wv, tap_slot(wv, p, dy, dx), r + 2 - 3 * dy, c + 2 - 3 * dx);
                }
    return 0;
}
"""


def test_x3_tap_table_of_the_kernels_header_is_the_packers_slot_order(tmp_path):
    """csrc/sr_s3_taps.h (the one statement of the x3 phase sets and tap slots both x3 kernels compile) against sr_pack._s3_slots (the
    order the packers fill the slots in): a plain C++17 host program prints (wave, slot, ky, kx) of every live tap from the header's
    constexpr functions; the 13 + 12 + 12 + 12 = 49 rows are the packers', each exactly once.  No kernel and no library is involved."""
    from video_super_resolution_amd import _lib, sr_pack
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    src, exe = tmp_path / "tap_table.cpp", tmp_path / "tap_table"
    src.write_text(_TAP_TABLE_MAIN)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # the compiler _lib.build() runs through csrc/Makefile
    subprocess.run([hipcc, "-std=c++17", "-x", "c++", "-Wall", "-I", csrc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    want = list(sr_pack._s3_slots())
    assert len(want) == 49 and [sum(1 for r in want if r[0] == wv) for wv in range(4)] == [13, 12, 12, 12]
    assert len(set(rows)) == len(rows) == 49
    assert sorted(rows) == sorted(want)
    assert rows == want   # and in the packers' order: a wave's slots ascend as its phases, rows and columns are walked


@pytest.mark.gpu
def test_gpu_blobs_packed_on_the_device_are_the_same_bytes():
    """The product packs on the device: the index arithmetic and the fp32 -> fp16 rounding there give the bytes the CPU gives."""
    _compare(collect("cuda"))
