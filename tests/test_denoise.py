"""The denoiser without a GPU: the NULL check and two properties of the numpy reference (tests/denoise_ref.py)."""
import numpy as np

import denoise_ref as DR
from lumo_amd import _ffi


def test_null_context_is_invalid():
    buf = np.zeros(4)
    p = buf.ctypes.data_as(_ffi.c_double_p)
    args = _ffi.DenoiseIn(1, 1, p, p, p, p, None)
    assert _ffi.load().lumo_denoise(None, args, None, p, None) == 1


def test_constant_frame_is_returned():
    """Constant guides and colour: every weighted mean is one division of equal sums: 1e-15 relative."""
    one = np.ones((21, 37, 1))
    colour, albedo = np.array([0.8, 0.3, 1.7]), np.array([0.5, 0.25, 0.9])
    planes = [np.concatenate([v * one * 1.5, one * 1.5], axis=-1) for v in (colour, albedo, np.array([0.0, 0.6, 0.8]))]
    planes.append(np.concatenate([4.0 * one, one, 0.0 * one, one], axis=-1) * 1.5)
    assert np.abs(DR.denoise(*planes)[0] / colour - 1.0).max() <= 1e-15


def test_rows_beyond_reach_change_nothing():
    """Rows appended below the frame leave the rows out of their reach bit for bit as they were.  Two
    iterations reach 2 x 2 + 2 x 1 rows, the variance window 3 more, and one more row sees the new
    rows through a clamped neighbour (the depth slope, the variance's binomial): 10 rows."""
    small, big = DR.frame(19, 16, 5), DR.frame(19, 30, 6)
    big = [np.concatenate([s, b[16:]], axis=0) for s, b in zip(small, big)]
    a, va = DR.denoise(*small, iterations=2)
    b, vb = DR.denoise(*big, iterations=2)
    keep = 16 - 10
    np.testing.assert_array_equal(a[:keep].view(np.uint64), b[:keep].view(np.uint64))
    np.testing.assert_array_equal(va[:keep].view(np.uint64), vb[:keep].view(np.uint64))
    assert (a[keep:].view(np.uint64) != b[keep:16].view(np.uint64)).any()
