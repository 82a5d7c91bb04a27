"""Host logic of the fp16 SR path that needs no GPU: the stage route rule against the if / elif ladder it replaced, the plane chunks
of the strip-marching launches, and the one loader of the side libraries."""
import itertools
import subprocess

import pytest

from video_super_resolution_amd import _lib
from video_super_resolution_amd.sr import _plane_chunks, _stage_route


def _ladder(scale, j, G, fold, fuse_uptran, utd_build, use_x, has_post, in_stage_post, in_utd_post):
    """The ladder of SRProjectionModule._forward_f16 before the route rule, branch for branch (each branch names the call it made)."""
    if fold and j == 0:
        return "pre", bool(fuse_uptran)                  # P["stage_pre"][0](.., post=self.fuse_uptran)
    elif scale == 4 and utd_build == 4 and not use_x:
        if fuse_uptran and j + 6 <= G:
            return "utd4", True                          # self._utd4(a, P["utd4"][j], .., post=True)
        else:
            return "utd4", False                         # self._utd4(a, P["utd4"][j], ..)
    elif scale == 4 and fuse_uptran and in_utd_post and not use_x:
        return "utd_post", True                          # self._utd_post(a, P["utd_post"][j], ..)
    elif scale != 4 and fuse_uptran and has_post and not use_x:
        return "stage", True                             # P["stage"][j](.., post=True)
    elif scale == 3 and fuse_uptran and in_stage_post and not use_x:
        return "stage_post", True                        # P["stage_post"][j](.., post=True)
    else:
        return ("utd" if scale == 4 else "stage"), False   # self._utd(a, P["utd"][j], ..) / P["stage"][j](..)


def _route_inputs():
    for scale, j, G, fuse_uptran, utd_build, use_x, has_post, in_stage_post, in_utd_post in itertools.product(
            (2, 3, 4), (0, 3), (6, 9), (0, 1), (3, 4), (0, 1), (0, 1), (0, 1), (0, 1)):
        for fold in ((0, 1) if (scale, G, j) == (3, 6, 0) else (0,)):   # (what `fold_chain` can set)
            yield scale, j, G, fold, fuse_uptran, utd_build, use_x, has_post, in_stage_post, in_utd_post


def test_stage_route_equals_the_ladder_it_replaced():
    cases = list(_route_inputs())
    assert len(cases) == 3 * 2 * 2 * 2 ** 6 + 2 ** 6
    seen = set()
    for c in cases:
        got = _stage_route(*c)
        assert got == _ladder(*c), c
        assert isinstance(got[1], bool)
        seen.add(got)
    assert seen == {("pre", True), ("pre", False), ("utd4", True), ("utd4", False), ("utd_post", True), ("utd", False), ("stage", True),
                    ("stage", False), ("stage_post", True)}


def test_plane_chunks():
    assert _plane_chunks(8, 720, 1280) == [(0, 8)]
    assert _plane_chunks(8, 2160, 3840) == [(0, 8)]
    assert _plane_chunks(20, 2160, 3840) == [(0, 8), (8, 8), (16, 4)]
    assert _plane_chunks(3, 40000, 40000) == [(0, 1), (1, 1), (2, 1)]   # one plane is beyond the limit: the entry refuses it
    assert _plane_chunks(1, 5, 33) == [(0, 1)]


_SIDE = {"grad": ("load_grad", "GLIB_PATH", 5), "s3": ("load_s3", "S3LIB_PATH", 4), "s3t": ("load_s3t", "S3TLIB_PATH", 5),
         "s3p": ("load_s3p", "S3PLIB_PATH", 4), "s3f": ("load_s3f", "S3FLIB_PATH", 4)}


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(set(ln.split()[-1] for ln in out.splitlines() if " T vsr_" in ln))


@pytest.mark.parametrize("name", sorted(_SIDE))
def test_side_library_loader(name):
    loader, path, count = _SIDE[name]
    _lib.build()
    lib = getattr(_lib, loader)()
    assert getattr(_lib, loader)() is lib
    assert lib._name == getattr(_lib, path)
    prefix = "vsr_" + name
    assert lib.vsr_last_error() == getattr(lib, prefix + "_last_error")() and isinstance(lib.vsr_last_error(), bytes)
    declared = _lib.declared_symbols(**{name: True})
    assert len(declared) == count and declared == _exported(getattr(_lib, path))
    assert all(s.startswith(prefix + "_") for s in declared)


def test_declared_symbols_of_the_main_and_cross_check_headers():
    _lib.build()
    declared, xdeclared = _lib.declared_symbols(), _lib.declared_symbols(xcheck=True)
    assert len(declared) == 66 and _exported(_lib.LIB_PATH) == declared
    assert _exported(_lib.XLIB_PATH) == sorted(set(declared) | set(xdeclared))
