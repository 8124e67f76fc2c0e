"""The firefly clamp without a GPU: the NULL checks, and that the GPU test's frames make the reference
(tests/denoise_firefly_ref.py) clamp what they are meant to."""
import denoise_ref as DR
import pytest
from test_gpu_denoise_firefly import SETTINGS, SPIKES, reference, spiked

from lumo_amd import _ffi


def test_null_context_is_invalid():
    assert _ffi.load().lumo_denoise_set_firefly(None, None) == 1
    assert _ffi.load().lumo_denoise_firefly_info(None, None) == 1


@pytest.mark.parametrize("size", [s for s in SPIKES if s != (1, 1)], ids=lambda s: "%dx%d" % s)
def test_frames_meet_their_conditions(size):
    """At the first setting some hit pixels are clamped and not all, every firefly on a surface among them; the L of
    three equal ones (rank 2: each has two equals beside it) and the one among the misses stay."""
    film, feat, add = spiked(size)
    c = DR.ratio(film.pixels[..., :3], film.pixels[..., 3:4]) + add
    c1, count = reference(film, feat, add, SETTINGS[0])
    assert 0 < count < int((feat.coverage() > 0.0).sum())
    changed = (c1 != c).any(-1)
    assert count == changed.sum()
    for name, pix in SPIKES[size].items():
        stays = name in ("ell", "miss")
        assert [bool(changed[y, x]) for x, y in pix] == [not stays] * len(pix), name
    # (1, 8, 8): a corner has 3 neighbours, so its firefly stays there; one neighbour is enough at (1, 1, 1)
    for setting, clamped in ((SETTINGS[3], False), (SETTINGS[1], True)):
        x, y = SPIKES[size]["corner"][0]
        assert (reference(film, feat, add, setting)[0][y, x] != c[y, x]).any() == clamped
