"""The float64 restatements of tests/_yuv_ref.py against values worked by hand (CPU): layouts, up-sampling taps, filters."""
import numpy as np

import _yuv_ref as R


def test_pack_unpack_layouts():
    Y = np.arange(8).reshape(1, 2, 4) + 10
    Cb, Cr = np.array([[[1, 2]]]), np.array([[[3, 4]]])
    assert R.pack(Y, Cb, Cr, "yuv420p").tolist() == [[10, 11, 12, 13, 14, 15, 16, 17, 1, 2, 3, 4]]
    assert R.pack(Y, Cb, Cr, "nv12").tolist() == [[10, 11, 12, 13, 14, 15, 16, 17, 1, 3, 2, 4]]
    assert R.pack(Y + 500, Cb, Cr, "yuv420p10le")[0, :4].tolist() == [510 & 255, 510 >> 8, 511 & 255, 511 >> 8]
    p = R.pack(Y + 500, Cb, Cr, "p010le")
    assert p[0, :2].tolist() == [(510 << 6) & 255, (510 << 6) >> 8] and p[0, 16:20].tolist() == [64, 0, 192, 0]
    for fmt in R.FORMATS:
        b = R.pack(Y + 500 * (R.depth(fmt) == 10), Cb, Cr, fmt)
        assert b.dtype == np.uint8 and b.shape == (1, R.frame_bytes(fmt, 2, 4))
        y, cb, cr = R.unpack(b, fmt, 2, 4)
        assert np.array_equal(y, Y + 500 * (R.depth(fmt) == 10)) and np.array_equal(cb, Cb) and np.array_equal(cr, Cr)
    g = R.pack(Y, Cb, Cr, "yuv420p10le").copy()
    g[:, 1::2] |= 0xFC   # bits 10..15
    assert np.array_equal(R.unpack(g, "yuv420p10le", 2, 4)[0], Y)


def test_upsample_taps():
    c = np.array([[[0.0, 8.0, 16.0], [32.0, 40.0, 48.0]]])   # 2 x 3 chroma -> 4 x 6 luma
    left, center = R.upsample(c, "left"), R.upsample(c, "center")
    # rows: midway for both sitings: 0 -> c[0] (clamped), 1 -> 3/4 c[0] + 1/4 c[1], 2 -> 1/4 c[0] + 3/4 c[1], 3 -> c[1] (clamped)
    assert left[0, :, 0].tolist() == [0.0, 8.0, 24.0, 32.0]
    # columns, co-sited: the sample on even positions, the mean on odd ones, the last odd one clamped
    assert left[0, 0].tolist() == [0.0, 4.0, 8.0, 12.0, 16.0, 16.0]
    # columns, midway
    assert center[0, 0].tolist() == [0.0, 2.0, 6.0, 10.0, 14.0, 16.0]
    assert center[0, 1, 1] == 0.75 * (0.75 * 0 + 0.25 * 8) + 0.25 * (0.75 * 32 + 0.25 * 40)


def test_filters_and_rounding():
    rgb = np.zeros((1, 2, 4, 3))
    rgb[0, :, :, 0] = [[1, 2, 3, 4], [5, 6, 7, 9]]
    assert R.filtered(rgb, "center")[0, 0, :, 0].tolist() == [3.5, 5.75]
    # left: (1,2,1)/4 over columns 2cx-1 (clamped at 0), 2cx, 2cx+1, then the mean of the two rows
    assert R.filtered(rgb, "left")[0, 0, :, 0].tolist() == [((1 + 2 + 2) / 4 + (5 + 10 + 6) / 4) / 2, ((2 + 6 + 4) / 4 + (6 + 14 + 9) / 4) / 2]
    assert R.quantise(np.array([0.5, 1.5, 2.5, -3.0, 255.5, 300.0, 1023.5]), "nv12").tolist() == [0, 2, 2, 0, 255, 255, 255]
    assert R.quantise(np.array([255.5, 1023.5, 2000.0]), "p010le").tolist() == [256, 1023, 1023]
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    x = np.array([[[[-3.2, 0, 255], [255.49, 300, np.nan]], [[1, 2, 3], [4, 5, 6]]]], dtype=np.float32)
    y, cb, cr = R.write_values(x, ident, "center")
    assert y.tolist() == [[[0.0, 255.0], [1.0, 4.0]]]   # (255.49 is clamped to 255 before the matrix)
    assert cb.tolist() == [[[(0 + 255 + 2 + 5) / 4]]]
    assert cr.tolist() == [[[(255 + 0 + 3 + 6) / 4]]]
    assert R.aten_nearest_index(18, 4).tolist() == [0, 4, 9, 13] and R.aten_nearest_index(34, 11).tolist()[-1] == 30
