"""A census of kernel BUILDS, on the CPU: every build of the trunk convolution launchers that the three fp16 trunks launch at the BASELINE
sizes (tests/golden/g14_trunk_layers.json, recorded on the device by tools/record_trunk_layers.py) must be reached by a case of the
exact-arithmetic tests (tests/_conv_cases.py, run by test_gpu_exact_conv.py) and by a case of the poisoned-buffer tests
(test_gpu_poisoned_buffers.py).  Both sides are planned with `vsr_conv2d_plan` of the cross-check library: nothing is launched and no
HIP call is made, so this runs on any machine.

A build's KEY is its route string with the split count removed (`+splitk8` -> `+splitk`): the template arguments stay, because
`k_conv_patch_r8<7, 2>` and `k_conv_patch_r8<7, 1>` are separate kernels with their own LDS layout, register tiling and epilogue.  The
gather and tile families (their `deconv4s2` and `stem` forms too) take the kernel size and the stride as run-time arguments, so their
keys carry `(kh, stride)` as well.  There is no exemption list: UNREACHABLE below may name at most two keys that no case of at most
75,000 output pixels plans to under any switch set, each with its reason -- it is empty."""
import json
import os
import re

import pytest

import _conv_cases as CC
from test_conv_route_plan import _DEFAULTS, plan_route
from video_super_resolution_amd import _lib as L, igemm

pytestmark = pytest.mark.xcheck

_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_trunk_layers.json")
UNREACHABLE = {}   # key -> reason; at most two (see above)


def build_key(route, kh, stride):
    r = re.sub(r"(?<=splitk)\d+", "", route)
    return f"{r} k{kh} s{stride}" if re.match(r"(deconv4s2 )?(gather|tile)<", r) else r


def planned_keys(rows):
    """rows: (entry, the 23 plan arguments, switches, (route batch num, den), has_ws, ws_bytes) -> [(route, key)] in order; every switch
    back at its default after."""
    lib = L.load_xcheck()
    out = []
    try:
        for entry, args, switches, (num, den), has_ws, ws_bytes in rows:
            for m in _DEFAULTS + tuple(switches):
                lib.vsr_conv2d_tuning(m)
            L.check(lib.vsr_conv2d_route_batch(num, den), lib=lib)
            route = plan_route(lib, entry, args, has_ws, ws_bytes)
            out.append((route, build_key(route, args[9], args[11])))
    finally:
        for m in _DEFAULTS:
            lib.vsr_conv2d_tuning(m)
        lib.vsr_conv2d_route_batch(0, 0)
    return out


def case_keys(cases):
    """Keys of (entry kind, shape, switch set, activation[, (out_coff, channels beyond the slice)]) rows of tests/_conv_cases.py, as the
    igemm classes launch them: with the split-K workspace."""
    rows = [(CC.ENTRY[c[0]], CC.plan_args(c[0], c[1], *(c[4] if len(c) > 4 else ())), c[2], (0, 0), 1, igemm._WS_BYTES) for c in cases]
    return [k for _, k in planned_keys(rows)]


def _fixture():
    with open(_TABLE) as f:
        return json.load(f)


def production_keys():
    """-> (keys, [(row, planned route)] of the rows the current code plans differently from the recording)."""
    rows = _fixture()["rows"]
    got = planned_keys([(kind, args, (), batch, has_ws, ws_bytes) for kind, args, batch, has_ws, ws_bytes, _ in rows])
    stale = [(row, route) for row, (route, _) in zip(rows, got) if route != row[5]]
    return {k for _, k in got}, stale


def poison_cases():
    """The fp16 trunk convolution cases of test_gpu_poisoned_buffers.py as rows of the same form: test_conv_default_route,
    test_conv_forced_route, test_conv_forced_patch_route, the stem, pair, transposed and 1x1 cases, and BUILD_CASES (which it runs too)."""
    import test_gpu_poisoned_buffers as P
    TC = P.TC
    act = (CC.NONE, 0.1)
    rows = [(CC.CONV, c[:8], (), act) for c in TC.CASES + [c for c in TC.TILE_CASES if c not in TC.CASES]]
    rows += [(CC.CONV, c[:8], modes, act) for modes, cases in P.FORCED.values() for c in cases]
    rows += [(CC.CONV, c[:6] + (1, c[5] // 2), modes, act) for modes, cases in P.PATCH_FORCED.values() for c in cases]
    rows += [(CC.STEM, c[:8], (), act) for c in P._params(TC.test_stem_conv_matches_torch, "case")]
    rows += [(CC.PAIR, c[:6] + (2, c[6]), (), act) for c in P._params(TC.test_pair_conv_stride2, "case")]
    for s in P._params(TC.test_transposed_conv_k4s2, "shape"):
        rows += [(CC.DECONV, s, m, act) for m in ((), (1,)) + (((2003,),) if s[4] > 32 else ())]
    for N, H, W, cout, _, extra, coff in P._params(TC.test_conv1x1_transposing_build, "case"):
        rows += [(CC.CONV, (N, 128, H, W, cout, 1, 1, 0), (mode,), act, (coff, extra)) for mode in (7001, 7000)]
    return rows


def missing_keys(cases):
    prod, _ = production_keys()
    return sorted(prod - set(case_keys(cases)) - set(UNREACHABLE))


def test_fixture_holds_settings_and_results_only():
    doc = _fixture()
    assert doc["configs"] == ["C3A", "C3B", "C5"] and sorted(doc) == ["configs", "rows", "self_named"]
    rows = doc["rows"]
    assert rows == sorted(rows) and len({json.dumps(r) for r in rows}) == len(rows) > 100
    for kind, args, batch, has_ws, ws_bytes, route in rows:
        assert kind in (0, 1, 2) and len(args) == 23 and all(type(a) is int for a in args) and len(batch) == 2 and has_ws in (0, 1) and type(ws_bytes) is int
        assert re.fullmatch(r"[a-z0-9_ ]+(<[0-9a-z,]+>)?(\+splitk\d+)?", route), route
    assert {k for k, *_ in rows} == {0, 1, 2} and {tuple(b) for _, _, b, *_ in rows} > {(0, 0)}   # (streaming mode: a route batch in force)
    assert all(re.fullmatch(r"(flow_head|hg_front|hg_inception)(<[0-9,]+>)?", r) for r in doc["self_named"]) and len(doc["self_named"]) >= 3


def test_current_code_plans_the_recorded_routes():
    _, stale = production_keys()
    assert not stale, (f"{len(stale)} rows of g14_trunk_layers.json are planned differently by the current code (first: {stale[:3]}): the fixture is stale, "
                       "record it again with tools/record_trunk_layers.py")


def test_exact_cases_reach_every_build_the_trunks_launch():
    prod, _ = production_keys()
    exact = set(case_keys(CC.exact_rows()))
    print(f"kernel-build census: {len(prod)} production keys, {len(exact)} exact keys")
    assert len(UNREACHABLE) <= 2 and set(UNREACHABLE) <= prod
    missing = sorted(prod - exact - set(UNREACHABLE))
    assert not missing, f"builds the trunks launch and no exact-arithmetic case plans to: {missing}"


def test_poisoned_buffer_cases_reach_every_build_the_trunks_launch():
    prod, _ = production_keys()
    poison = set(case_keys(poison_cases() + CC.BUILD_CASES))
    print(f"kernel-build census: {len(prod)} production keys, {len(poison)} poisoned-buffer keys")
    missing = sorted(prod - poison - set(UNREACHABLE))
    assert not missing, f"builds the trunks launch and no poisoned-buffer case plans to: {missing}"


def test_every_build_case_is_there_for_a_build_nothing_else_reaches():
    """BUILD_CASES emptied: the census names exactly the keys of its rows (for the exact tables or for the poisoned-buffer lists), one row each."""
    keys = case_keys(CC.BUILD_CASES)
    assert len(set(keys)) == len(keys), sorted(k for k in keys if keys.count(k) > 1)
    without = set(missing_keys(CC.exact_rows(build_cases=[]))) | set(missing_keys(poison_cases()))
    print(f"kernel-build census: without BUILD_CASES {len(without)} keys are missing: {sorted(without)}")
    assert without == set(keys), (sorted(without - set(keys)), sorted(set(keys) - without))


@pytest.mark.parametrize("which", [0, -1, "patch_r8<11,2>", "deconv4s2 tile<128> k2 s1", "tile<64> k3 s2"])
def test_a_planted_gap_is_reported(which):
    """One BUILD_CASES row removed -- the first, the last, the 11 x 11 build with the largest halo, one that both suites lacked, one that
    only the poisoned-buffer lists lacked --: each census reports that row's key if it depended on the row, and nothing else."""
    keys = case_keys(CC.BUILD_CASES)
    i = keys.index(which) if isinstance(which, str) else range(len(keys))[which]
    planted = CC.BUILD_CASES[:i] + CC.BUILD_CASES[i + 1:]
    lacked = [keys[i] in missing_keys(cases) for cases in (CC.exact_rows(build_cases=[]), poison_cases())]
    assert any(lacked)
    assert missing_keys(CC.exact_rows(build_cases=planted)) == [keys[i]] * lacked[0]
    assert missing_keys(poison_cases() + planted) == [keys[i]] * lacked[1]
    if isinstance(which, str):
        assert lacked == [which != "tile<64> k3 s2", which != "patch_r8<11,2>"]
