"""ctypes/numpy front-end of the fused-SSIM CPU oracle (oracle/sks_ssim_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/.  The product package (skelsplat_amd/) never imports this module.

Two builds of one source: `f32` is the oracle the HIP kernels are held to bit for bit, `f64` is the same text in double
(held to an independent float64 conv2d SSIM by tests/test_ssim_oracle_cpu.py).  Every function takes `real="f32"|"f64"`.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sks_ssim_oracle.c")
_LIBS = {}
_TYPES = {"f32": (np.float32, C.c_float), "f64": (np.float64, C.c_double)}

# flags returned by forward(): which output of a pixel has a quotient outside the range in which the kernels' division
# sequence is IEEE `/` (a nonzero |n| < 2^-100, or d outside [2^-100, 2^100))
FLAG_MAP, FLAG_DMU1, FLAG_DSIGMA1_SQ, FLAG_DSIGMA12 = 1, 2, 4, 8


def build(force=False):
    sos = {k: os.path.join(_HERE, f"libsks_ssim_oracle_{k}.so") for k in _TYPES}
    if force or any(not os.path.exists(s) or os.path.getmtime(_SRC) > os.path.getmtime(s) for s in sos.values()):
        subprocess.check_call(["make", "-C", _HERE, "-s"] + [os.path.basename(s) for s in sos.values()])
    return sos


def lib(real="f32"):
    if real not in _LIBS:
        L = C.CDLL(build()[real])
        assert L.ssim_oracle_sizeof_real() == np.dtype(_TYPES[real][0]).itemsize
        L.ssim_oracle_mean.restype = C.c_float
        _LIBS[real] = L
    return _LIBS[real]


def _a(x, real):
    return np.ascontiguousarray(x, dtype=_TYPES[real][0])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _shape(img):
    assert img.ndim == 4, img.shape
    return [C.c_int(int(s)) for s in img.shape]


def forward(img1, img2, C1=0.01 ** 2, C2=0.03 ** 2, train=True, real="f32"):
    """-> dict(map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, flags, ulp_sum, outside_documented).  `flags` is a uint8 mask
    per pixel (FLAG_*), `ulp_sum` the sum of ulp(q_i) over dm_dmu1's four quotients, `outside_documented` the number of
    quotients outside d in [2^-40, 2^8), |n| in [2^-60, 2^12) or n = 0."""
    dt, ct = _TYPES[real]
    img1, img2 = _a(img1, real), _a(img2, real)
    assert img1.shape == img2.shape
    out = dict(map=np.empty_like(img1), flags=np.zeros(img1.shape, np.uint8), ulp_sum=np.zeros_like(img1))
    for k in ("dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12"):
        out[k] = np.empty_like(img1) if train else None
    outside = C.c_int64(0)
    rc = lib(real).ssim_oracle_forward(*_shape(img1), ct(C1), ct(C2), _p(img1), _p(img2), _p(out["map"]), _p(out["dm_dmu1"]),
                                       _p(out["dm_dsigma1_sq"]), _p(out["dm_dsigma12"]), _p(out["flags"]),
                                       _p(out["ulp_sum"]), C.byref(outside))
    assert rc == 0, rc
    out["outside_documented"] = int(outside.value)
    return out


def backward(img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, real="f32"):
    img1 = _a(img1, real)
    args = [_a(x, real) for x in (img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12)]
    assert all(a.shape == img1.shape for a in args)
    out = np.empty_like(img1)
    rc = lib(real).ssim_oracle_backward(*_shape(img1), _p(img1), *[_p(a) for a in args], _p(out))
    assert rc == 0, rc
    return out


def backward_uniform(img1, img2, dL_value, dL_scale, crop, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, real="f32"):
    _, ct = _TYPES[real]
    img1 = _a(img1, real)
    args = [_a(x, real) for x in (dm_dmu1, dm_dsigma1_sq, dm_dsigma12)]
    out = np.empty_like(img1)
    rc = lib(real).ssim_oracle_backward_uniform(*_shape(img1), _p(img1), _p(_a(img2, real)), ct(dL_value), ct(dL_scale),
                                                C.c_int(int(crop)), *[_p(a) for a in args], _p(out))
    assert rc == 0, rc
    return out


def mean(ssim_map, crop=0, real="f32"):
    m = _a(ssim_map, real)
    return np.float32(lib(real).ssim_oracle_mean(*_shape(m), _p(m), C.c_int(int(crop))))
