"""numpy f64 reference for the feature buffers (tests/test_features.py pins it to the oracle):

    color_rgb    Color::xyz (color.rs:97-105) from the scene description's dense spectra, then the
                 camera description's white balance and XYZ -> RGB matrices (film/tile.rs:65-66)
    film_tile    FilmTile::add_sample (film/tile.rs:65-111) over a task's samples in pass order
    first_hits   bounce 0 of oracle_debug_trace for every (pass, pixel) of a task

Only exp and cosh differ from the device's lmath (a few ulp, tests/test_lmath.py)."""
import ctypes as C
import math

import numpy as np

import oracle_ffi as O
from lumo_amd import _ffi

Y_INTEGRAL = 106.856895  # xyz.rs:34
SVI = 253.819            # wavelength.rs SAMPLE_VISIBLE_INTEGRAL
STEP = (830.0 - 360.0) / (95.0 - 1.0)


def dense_tables(scene_desc, n=3):
    """The first n 95-bin dense spectra of the description (0, 1, 2: the CIE x, y, z curves)."""
    return np.ctypeslib.as_array(scene_desc.dense_spectra, shape=(scene_desc.num_dense_spectra, 95))[:n].copy()


def dense_sample(table, lam):
    """DenseSpectrum::sample (dense_spectrum.rs:77-97) of one table at an array of wavelengths."""
    lam = np.asarray(lam, dtype=np.float64)
    b1 = np.maximum(np.ceil((lam - 360.0) / STEP), 0.0).astype(np.int64)
    l1 = 360.0 + STEP * b1
    b1 = np.minimum(b1, 94)
    b0 = np.where(b1 == 0, 0, b1 - 1)
    x1 = (lam - (l1 - STEP)) / STEP
    v = table[b0] * (1.0 - x1) + table[b1] * x1
    v = np.where(lam == l1, table[b1], v)
    return np.where(lam == 0.0, 0.0, v)


def wl_pdf(lam):
    """ColorWavelength::pdf (wavelength.rs:62-75) for unterminated wavelengths."""
    lam = np.asarray(lam, dtype=np.float64)
    c = np.cosh(0.0072 * (lam - 538.05))
    return np.where((lam < 360.0) | (lam > 830.0), 0.0, 1.0 / (SVI * (c * c)))


def color_xyz(scene_desc, color, lam):
    """Color::xyz (color.rs:97-105): color, lam of shape (n, 4) -> (n, 3)."""
    t = dense_tables(scene_desc)
    color, lam = np.asarray(color, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    pdf = wl_pdf(lam)
    out = np.empty((len(color), 3))
    for k in range(3):
        term = dense_sample(t[k], lam) * color / pdf
        s = term[:, 0]
        for i in range(1, 4):  # Color::mean: the samples summed in order
            s = s + term[:, i]
        out[:, k] = s / 4.0
    return out / Y_INTEGRAL


def color_rgb(scene_desc, camera_desc, color, lam):
    """The film's colour pipeline without a tone map: XYZ, white balance, colour space."""
    def mul(m, v):  # Mat3 * Vec3 row by row, each row summed left to right
        m = np.array(list(m)).reshape(3, 3)
        return np.stack([m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1] + m[r, 2] * v[:, 2] for r in range(3)], axis=1)
    return mul(camera_desc.xyz_to_rgb, mul(camera_desc.white_balance, color_xyz(scene_desc, color, lam)))


def gauss(x, sigma):
    """PixelFilter::Gaussian's gaussian (filter.rs)."""
    return math.exp(-(x * x) / (2.0 * sigma * sigma)) / math.sqrt(max(2.0 * math.pi * sigma * sigma, 0.0))


def film_tile(task, camera_desc, raster, values, with_abs=False):
    """FilmTile::add_sample (film/tile.rs:65-111) for the samples of `task` in the order given
    (pass-major, pixels in raster order): raster (n, 2), values (n, 3).  Returns the tile as
    (H, W, 4): the weighted sums and the weight sum; with_abs also the (H, W, 3) sums of w |value|."""
    fr, fsig = camera_desc.filter_radius, camera_desc.filter_sigma
    x0, y0, x1, y1 = task.px_min[0], task.px_min[1], task.px_max[0], task.px_max[1]
    r = int(math.ceil(fr - 0.5))
    gr = gauss(fr, fsig)
    tile = np.zeros((y1 - y0, x1 - x0, 4))
    mag = np.zeros((y1 - y0, x1 - x0, 3))
    for (rx, ry), v in zip(np.asarray(raster, dtype=np.float64), np.asarray(values, dtype=np.float64)):
        px, py = max(int(math.floor(rx)), 0), max(int(math.floor(ry)), 0)
        for fy in range(max(py - r, y0), min(py + r, y1 - 1) + 1):
            wy = max(gauss(ry - (0.5 + fy), fsig) - gr, 0.0)
            for fx in range(max(px - r, x0), min(px + r, x1 - 1) + 1):
                w = max(gauss(rx - (0.5 + fx), fsig) - gr, 0.0) * wy
                if w != 0.0:
                    tile[fy - y0, fx - x0, :3] += v * w
                    tile[fy - y0, fx - x0, 3] += w
                    mag[fy - y0, fx - x0] += np.abs(v) * w
    return (tile, mag) if with_abs else tile


def _debug_trace():
    lib = O.load()
    fn = lib.oracle_debug_trace
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(_ffi.SceneDesc), C.POINTER(_ffi.CameraDesc), C.POINTER(_ffi.TileTask), C.c_int, C.c_int,
                   _ffi.c_double_p, C.POINTER(C.c_int)]
    return lib, fn


def first_hits(scene_desc, camera_desc, task, sampler=0, accel=0):
    """Record 0 of oracle_debug_trace (the camera ray's Scene::hit) for every sample of `task`,
    pass-major: dict of hit (bool; False: the path logged no bounce), kind, object, t, p, ng,
    backface.  The oracle re-renders the task per call: keep tasks at 16 x 16 @ 3 or below."""
    lib, fn = _debug_trace()
    P = (task.px_max[0] - task.px_min[0]) * (task.px_max[1] - task.px_min[1])
    m = P * task.samples
    out = dict(hit=np.zeros(m, dtype=bool), kind=np.zeros(m, dtype=np.int32), object=np.full(m, -1, dtype=np.int32),
               t=np.zeros(m), p=np.zeros((m, 3)), ng=np.zeros((m, 3)), backface=np.zeros(m, dtype=np.int32))
    rec = np.zeros(64 * 20)
    n = C.c_int(0)
    lib.oracle_set_integrator(0)
    lib.oracle_set_sampler(int(sampler))
    lib.oracle_set_accel(int(accel))
    try:
        for s in range(task.samples):
            for j in range(P):
                st = fn(C.byref(scene_desc), C.byref(camera_desc), C.byref(task), s, j,
                        rec.ctypes.data_as(_ffi.c_double_p), C.byref(n))
                assert st == 0, st
                if n.value == 0:
                    continue
                o = s * P + j
                assert rec[0] == 0.0  # the record of bounce 0
                out["hit"][o] = True
                out["kind"][o], out["object"][o], out["t"][o] = int(rec[1]), int(rec[2]), rec[4]
                out["p"][o], out["ng"][o], out["backface"][o] = rec[11:14], rec[14:17], int(rec[18])
    finally:
        lib.oracle_set_sampler(0)
        lib.oracle_set_accel(0)
    return out
