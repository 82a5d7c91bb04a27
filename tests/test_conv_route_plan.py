"""The route plan of the trunk convolution launchers (csrc/conv_igemm.hip: plan_conv / plan_stem / plan_deconv behind the dry entry
`vsr_conv2d_plan` of the cross-check library) against tests/golden/g11_conv_routes.json: 1500 (switches, route batch, layer, workspace)
rows with the route the launchers took BEFORE the plan existed, recorded from `vsr_last_route()` of the old ladder.  Nothing is launched
and no HIP call is made, so this runs on any machine."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from video_super_resolution_amd import _lib as L

pytestmark = pytest.mark.xcheck

_DEFAULTS = (0, 1128, 2001, 4000, 5000, 6001, 7000, 8000, 9001)   # every knob of vsr_conv2d_tuning at its default (as in test_gpu_exact_conv.py)
_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_conv_routes.json")
WS_BYTES = 64 << 20
KINDS = ("gather<64>", "gather<64,stem>", "tile<", "deconv4s2 gather<", "deconv4s2 tile<", "deconv4s2_patch", "stem7_rows", "patch_pf<", "patch_lw<",
         "patch_r8<", "patch<", "patch_rows<", "conv1x1_stream<", "conv1x1_t", "+splitk")
SWITCHES = (1, 2, 3, 5, 6, 7, 8, 10, 11, 1064, 2000, 2003, 4064, 4128, 5004, 6000, 6002, 7001, 8001, 8002, 9000, 9002, 9003)


def plan_route(lib, kind, args, has_ws=1, ws_bytes=WS_BYTES):
    """vsr_conv2d_plan -> the route string.  kind: 0 conv, 1 stem, 2 deconv4s2; args: the 23 shape arguments in the header's order."""
    L.check(lib.vsr_conv2d_plan(kind, *args, has_ws, ctypes.c_size_t(ws_bytes)), "conv2d_plan", lib=lib)
    return lib.vsr_last_route().decode()


def _rows():
    with open(_TABLE) as f:
        return json.load(f)["rows"]


def _mismatches(rows):
    """[(row index, recorded route, planned route)] of the rows the plan answers differently; every switch back at its default after."""
    lib = L.load_xcheck()
    bad = []
    try:
        for i, (switches, (num, den), kind, args, has_ws, ws_bytes, want) in enumerate(rows):
            for m in _DEFAULTS + tuple(switches):
                lib.vsr_conv2d_tuning(m)
            L.check(lib.vsr_conv2d_route_batch(num, den), lib=lib)
            got = plan_route(lib, kind, args, has_ws, ws_bytes)
            if got != want:
                bad.append((i, want, got))
    finally:
        for m in _DEFAULTS:
            lib.vsr_conv2d_tuning(m)
        lib.vsr_conv2d_route_batch(0, 0)
    return bad


def test_plan_takes_the_routes_recorded_before_it_existed():
    rows = _rows()
    assert len(rows) == 1500
    routes = {r[6] for r in rows}
    for k in KINDS:   # every kind of route, with and without split-K
        assert any(k in r if k.startswith("+") else r.startswith(k) for r in routes), k
    assert {s for r in rows for s in r[0]} >= set(SWITCHES)
    assert {tuple(r[1]) for r in rows} == {(0, 0), (4, 2), (2, 1)} and {r[2] for r in rows} == {0, 1, 2}
    assert {(r[4], r[5]) for r in rows} == {(1, WS_BYTES), (0, 0), (1, 1 << 20)}
    bad = _mismatches(rows)
    assert not bad, f"{len(bad)} of {len(rows)} rows, first: {[(rows[i][:6], want, got) for i, want, got in bad[:5]]}"


def test_a_wrong_row_is_reported():
    """Three planted rows -- another tile width, another split count, another kernel -- come back, and only they."""
    rows = _rows()[::10]
    idx = [next(i for i, r in enumerate(rows) if re.fullmatch(pat, r[6])) for pat in (r"gather<64>", r"gather<\d+>\+splitk8", r"patch_r8<3,2>")]
    assert len(set(idx)) == 3
    planted = [list(r) for r in rows]
    for i, wrong in zip(idx, ("gather<128>", rows[idx[1]][6].replace("splitk8", "splitk7"), "patch_lw<3,2>")):
        planted[i][6] = wrong
    bad = _mismatches(planted)
    assert [(i, want) for i, want, _ in bad] == sorted((i, planted[i][6]) for i in idx)
    assert [got for _, _, got in bad] == [rows[i][6] for i, _, _ in bad]


def test_plan_reports_the_entries_argument_errors():
    lib = L.load_xcheck()
    ok = [32, 1, 16, 30, 32, 16, 30, 16, 16, 3, 3, 1, 0, 1, 1, 32, 0, 16, 30, 1, 0, 1, 0]
    assert plan_route(lib, 0, ok) == "gather<16>"
    for kind, pos, value, text in ((0, 4, 33, "conv2d: input channels 33 must be padded to a multiple of 32"), (0, 17, 15, "conv2d: output window exceeds"),
                                   (0, 2, 1 << 22, "4 GiB"), (1, 10, 9, "conv2d_stem: bad shape"), (2, 8, 8, "deconv4s2: output slice"), (3, 0, 32, "conv2d_plan: kind 3")):
        args = list(ok)
        args[pos] = value
        assert lib.vsr_conv2d_plan(kind, *args, 1, ctypes.c_size_t(WS_BYTES)) == -1
        assert text in lib.vsr_last_error().decode()


_KWALK_MAIN = r"""
// The K-walk table of the gather / tile kernels (csrc/conv_kwalk.h, host part): the entry counts the kernels write and the launchers
// reserve, and the largest index each kernel's loop reads, replayed from the loop bounds in the kernel text.
#include <cassert>
#include <cstdio>
#include "conv_kwalk.h"
using namespace vsrc;

// k_conv_igemm_d<.., D>: en = tab[0], tab[1]; D - 1 requests before the loop, then whole groups of D steps, one request each; request
// number j (1-based) ends with q = 2 j and reads tab[q], tab[q + 1].  n = nk - ks0 live steps (<= ks_per; <= 0: the loop does not run).
static int last_read_gather(int n, int D) {
    int requests = D - 1;
    for (int ks = 0; ks < n; ks += D) requests += D;
    return 2 * requests + 1;
}
// k_conv_igemm (first build): two requests before the loop, groups of two steps
static int last_read_first(int n) {
    int requests = 2;
    for (int ks = 0; ks < n; ks += 2) requests += 2;
    return 2 * requests + 1;
}
// k_conv_tile: stage(0) before the loop, stage(buf ^ 1) in every step but the last
static int last_read_tile(int n) {
    int requests = 1;
    for (int ks = 0; ks < n; ++ks)
        if (ks + 1 < n) ++requests;
    return 2 * requests + 1;
}

int main() {
    static_assert(kwalk_entries(7, kwalk_gather_lookahead(3)) == 2 * (7 + 5), "gather D = 3");
    long checked = 0;
    for (int ks_per = 1; ks_per <= 4096; ++ks_per) {
        const int g3 = kwalk_entries(ks_per, kwalk_gather_lookahead(3)), g5 = kwalk_entries(ks_per, kwalk_gather_lookahead(5));
        const int f = kwalk_entries(ks_per, KWALK_FIRST_LOOKAHEAD), t = kwalk_entries(ks_per, KWALK_TILE_LOOKAHEAD);
        assert(g3 == 2 * (ks_per + 5));
        assert(g5 == 2 * (ks_per + 9));
        assert(f == 2 * (ks_per + 5));
        assert(t == 2 * (ks_per + 2));
        for (int n = 0; n <= ks_per; n += (ks_per > 64 && n > 8 && n + 9 < ks_per ? 7 : 1)) {   // every n near both ends, every 7th between
            assert(last_read_gather(n, 3) < g3);
            assert(last_read_gather(n, 5) < g5);
            assert(last_read_first(n) < f);
            assert(last_read_tile(n) < t);
            ++checked;
        }
        // the gather bound is tight: a range that ends one step into a group of D reads the table's last entry
        if (ks_per % 3 == 1) assert(last_read_gather(ks_per, 3) == g3 - 1);
        if (ks_per % 5 == 1) assert(last_read_gather(ks_per, 5) == g5 - 1);
        assert(last_read_tile(ks_per) == t - 3);
    }
    // the launchers' helper: pairs, steps and steps per split (conv: kh kw cin/32 pairs; stem: one per kernel row)
    const KSteps a = k_steps(false, 3, 3, 256, 4), s = k_steps(true, 7, 7, 32, 1);
    assert(a.nchunk == 8 && a.npair == 72 && a.nk_all == 36 && a.ks_per == 9);
    assert(s.nchunk == 1 && s.npair == 7 && s.nk_all == 4 && s.ks_per == 4);
    std::printf("kwalk ok %ld\n", checked);
    return 0;
}
"""


def test_kwalk_table_holds_every_entry_the_kernels_read(tmp_path):
    """csrc/conv_kwalk.h's `kwalk_entries` (the count the gather / tile kernels write and their launchers reserve in LDS) gives the four
    formulas the kernels had before the header existed, for 1..4096 steps per workgroup, and the largest index each kernel's loop reads
    (its requests before the loop, its groups of D steps, the one-step read-ahead `tab[q + 1]`) stays below it.  A plain C++17 host
    program, built with the address and undefined-behaviour sanitizers (host code only: nothing here is compiled for or run on a GPU)
    and run on its own."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc")
    src, exe = tmp_path / "kwalk_table.cpp", tmp_path / "kwalk_table"
    src.write_text(_KWALK_MAIN)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # the compiler _lib.build() runs through csrc/Makefile
    subprocess.run([hipcc, "-std=c++17", "-x", "c++", "-Wall", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("kwalk ok ")
