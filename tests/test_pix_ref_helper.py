"""tests/_pix_ref.py pinned on the CPU: its 4:2:2 formulas against tests/_yuv_ref.py's 4:2:0 ones on frames where the two must agree
exactly, its 4:4:4 formulas against hand-worked values, and the conditions on the inputs of tests/test_gpu_pix.py (the share of
samples near a tie, the size of the partial sums) for the very seeds that file uses."""
import numpy as np
import pytest

import _pix_ref as P
import _yuv_ref as Y
from video_super_resolution_amd import frames

COLOUR = [(m, fr) for m in ("bt601", "bt709", "bt2020") for fr in (False, True)]
PAIRS = [("yuv422p", "yuv420p"), ("yuv422p10le", "yuv420p10le")]


@pytest.mark.parametrize("fmt422,fmt420", PAIRS)
def test_422_ingest_equals_the_420_reference_where_all_chroma_rows_are_equal(fmt422, fmt420):
    """Every chroma row of both frames is one row: the 4:2:0 vertical weights then meet equal samples everywhere (w c + (1 - w) c = c
    exactly, the weights being dyadic), and what is left of the 4:2:0 rule is the horizontal rule, which is the 4:2:2 one."""
    F, H, W = 2, 6, 10
    rs = np.random.RandomState(3)
    top = 2 ** P.depth(fmt422)
    Yc = rs.randint(0, top, (F, H, W))
    cb, cr = rs.randint(0, top, (F, 1, W // 2)), rs.randint(0, top, (F, 1, W // 2))
    f420 = Y.pack(Yc, np.repeat(cb, H // 2, 1), np.repeat(cr, H // 2, 1), fmt420)
    f422 = P.pack(Yc, np.repeat(cb, H, 1), np.repeat(cr, H, 1), fmt422)
    assert f422.shape == (F, P.frame_bytes(fmt422, H, W)) and f420.shape == (F, Y.frame_bytes(fmt420, H, W))
    for matrix, full_range in COLOUR:
        coef = frames.pix_coefficients(fmt422, matrix, full_range, inverse=True)
        assert np.array_equal(coef, frames.yuv_coefficients(fmt420, matrix, full_range, inverse=True))
        for siting in P.SITINGS:
            a = P.ingest(f422, fmt422, coef, siting, H, W, 3, 5)
            b = Y.ingest(f420, fmt420, coef, siting, H, W, 3, 5)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # ... and the two sitings do differ on such a frame (the comparison is not vacuous)
    assert not np.array_equal(P.ingest(f422, fmt422, coef, "left", H, W)[1], P.ingest(f422, fmt422, coef, "center", H, W)[1])


@pytest.mark.parametrize("fmt422,fmt420", PAIRS)
def test_422_write_equals_the_420_reference_where_rows_come_in_equal_pairs(fmt422, fmt420):
    """RGB rows 2k and 2k+1 equal: the 4:2:0 filter's vertical step is (r + r) / 2 = r (LEFT) or folds into ((a + b) + (a + b)) / 4 =
    (a + b) / 2 (CENTER), both exact; the sums of three float32 values in 0..255 are exact in float64 in any order.  So the 4:2:2 chroma
    rows 2k and 2k+1 equal the 4:2:0 chroma row k bit for bit, before and after rounding, and the luma planes are equal."""
    F, H, W = 2, 6, 10
    rs = np.random.RandomState(4)
    half = rs.uniform(-20, 280, (F, H // 2, W, 3)).astype(np.float32)
    half.reshape(-1)[:6] = P.SPECIAL
    rgb = np.repeat(half, 2, axis=1)
    for matrix, full_range in COLOUR:
        coef = frames.pix_coefficients(fmt422, matrix, full_range)
        for siting in P.SITINGS:
            y2, cb2, cr2 = P.write_values(rgb, coef, siting, fmt422)
            y0, cb0, cr0 = Y.write_values(rgb, coef, siting)
            assert np.array_equal(y2, y0)
            for c2, c0 in ((cb2, cb0), (cr2, cr0)):
                assert c2.shape == (F, H, W // 2) and c0.shape == (F, H // 2, W // 2)
                assert np.array_equal(c2[:, 0::2], c0) and np.array_equal(c2[:, 1::2], c0)
            got = P.unpack(P.write(rgb, fmt422, coef, siting), fmt422, H, W)
            want = Y.unpack(Y.write(rgb, fmt420, coef, siting), fmt420, H, W)
            assert np.array_equal(got[0], want[0])
            assert np.array_equal(got[1][:, 0::2], want[1]) and np.array_equal(got[2][:, 1::2], want[2])


def test_444_and_the_422_taps_by_hand():
    # 4:4:4: the samples at the pixel, whatever the siting
    Yc = np.array([[[10, 20, 30]]])
    Cb, Cr = np.array([[[100, 110, 120]]]), np.array([[[200, 190, 180]]])
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)
    f = P.pack(Yc, Cb, Cr, "yuv444p")
    assert f.tolist() == [[10, 20, 30, 100, 110, 120, 200, 190, 180]] and P.frame_bytes("yuv444p", 1, 3) == 9
    for siting in P.SITINGS:
        _, hr, _ = P.ingest(f, "yuv444p", ident, siting, 1, 3)
        assert hr.tolist() == [[[[10, 100, 200], [20, 110, 190], [30, 120, 180]]]]
    # 4:2:2, one row of 3 chroma samples 8, 16, 40: LEFT 8, 12, 16, 28, 40, 40; CENTER 8, 10, 14, 22, 34, 40
    c = np.array([[[8, 16, 40]]])
    assert P.upsample(c, "left", "yuv422p").tolist() == [[[8, 12, 16, 28, 40, 40]]]
    assert P.upsample(c, "center", "yuv422p").tolist() == [[[8, 10, 14, 22, 34, 40]]]
    # write-out filter of one row 0, 4, 8, 16, 32, 64: LEFT ((p[-1 -> 0] + p[1]) + 2 p[0]) / 4 = 1, (4 + 16 + 16) / 4 = 9, (16 + 64 + 64) / 4 = 36
    row = np.array([0, 4, 8, 16, 32, 64], dtype=np.float64).reshape(1, 1, 6, 1).repeat(3, axis=3)
    assert P.filtered(row, "left", "yuv422p")[0, 0, :, 0].tolist() == [1, 9, 36]
    assert P.filtered(row, "center", "yuv422p")[0, 0, :, 0].tolist() == [2, 12, 48]
    assert P.filtered(row, "left", "yuv444p") is row
    # 10 bit: two bytes per sample, little-endian, the mask drops bits 10..15
    f10 = P.pack(np.array([[[1023]]]), np.array([[[1]]]), np.array([[[512]]]), "yuv444p10le")
    assert f10.tolist() == [[0xFF, 0x03, 0x01, 0x00, 0x00, 0x02]]
    f10[0, 1] |= 0xFC
    assert [int(v[0, 0, 0]) for v in P.unpack(f10, "yuv444p10le", 1, 1)] == [1023, 1, 512]
    assert [P.frame_bytes(n, 3, 6) for n in P.FORMATS] == [36, 54, 72, 108]


@pytest.mark.parametrize("fmt", P.FORMATS)
def test_the_gpu_tests_inputs_meet_their_conditions(fmt):
    """The write-out test allows one code of difference within eps of a tie and caps such samples at 2 % of a case: that cap is a
    condition on the inputs, met by the reference alone for the seeds the GPU test uses.  The ingest bound assumes partial sums below
    1024: the largest over the corners of the code cube, for every coefficient set."""
    eps = 2.0 ** (P.depth(fmt) - 8) * 5e-5
    for matrix, full_range in COLOUR:
        coef = frames.pix_coefficients(fmt, matrix, full_range)
        for F, H, W in P.write_shapes(fmt):
            rgb = P.write_case(F, H, W)
            for siting in P.SITINGS:
                vals = P.write_values(rgb, coef, siting, fmt)
                near = sum(int(P.near_tie(v, eps).sum()) for v in vals)
                assert near <= 0.02 * sum(v.size for v in vals), (matrix, full_range, F, H, W, siting, near)
        inv = frames.pix_coefficients(fmt, matrix, full_range, inverse=True)
        top = 2 ** P.depth(fmt) - 1
        corners = np.array([[a, b, c] for a in (0, top) for b in (0, top) for c in (0, top)])
        f = P.pack(corners[:, 0].reshape(8, 1, 1), corners[:, 1].reshape(8, 1, 1), corners[:, 2].reshape(8, 1, 1), fmt.replace("422", "444"))
        assert P.ingest(f, fmt.replace("422", "444"), inv, "left", 1, 1)[2] < 1024.0
