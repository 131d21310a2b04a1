"""ctypes/numpy front-end of the REFERENCE's rasterizer compiled for the host (oracle/ref_build.py -> oracle/_ref/).

TEST INFRASTRUCTURE ONLY.  forward() / backward() / mark_visible() take what oracle.forward / oracle.backward /
oracle.mark_visible take and return the same dictionary keys, so a test can hold either to the other key by key.  What runs
underneath is not a restatement: it is the reference's own forward.cu / backward.cu / rasterizer_impl.cu, one block at a
time on one thread (oracle/ref_shim/ref_shim.h).  The libraries are built by __graft_entry__.build() where the reference
tree is present and only read anywhere else.
"""
import ctypes as C
import os

import numpy as np

from . import oracle as orc
from . import ref_build

CHANNELS = tuple(ref_build.VARIANTS)     # 17 (h36m), 19 (panoptic), 15 (op)
_LIBS = {}
_EXPF = None


class MissingReferenceLibrary(RuntimeError):
    pass


def lib(channels):
    """The library whose NUM_CHANNELS is `channels`; never builds (that is __graft_entry__.build()'s part)."""
    global _EXPF
    if channels not in _LIBS:
        so = ref_build.lib_path(channels)
        if channels not in ref_build.VARIANTS or not os.path.exists(so):
            raise MissingReferenceLibrary(
                "%s is missing: run __graft_entry__.build() where the reference tree is present (oracle/ref_build.py "
                "compiles the reference's rasterizer for the CPU; channel counts built: %s)" % (so, sorted(ref_build.VARIANTS)))
        L = C.CDLL(so)
        L.ref_forward.restype = C.c_void_p
        L.ref_num_rendered.restype = C.c_int
        L.ref_num_channels.restype = C.c_int
        assert L.ref_num_channels() == channels, (so, L.ref_num_channels())
        if _EXPF is None:
            _EXPF = C.cast(orc.lib().orc_expf, C.c_void_p)      # the one expf the oracle and the kernels share
        L.ref_shim_set_expf(_EXPF)
        _LIBS[channels] = L
    return _LIBS[channels]


_p, _f32 = orc._p, orc._f32


class _State:
    def __init__(self, L, handle):
        self.L, self.handle = L, C.c_void_p(handle)

    def __del__(self):
        if self.handle:
            self.L.ref_free(self.handle)
            self.handle = None


def _bg(bg, Cn):
    """>= NUM_CHANNELS floats: the reference's backward reads bg_color[ch] for every channel."""
    out = np.zeros(Cn, np.float32)
    if bg is not None:
        b = np.asarray(bg, np.float32).reshape(-1)
        out[:min(Cn, b.size)] = b[:Cn]
    return out


def forward(means3D, features, opacities, scales, rotations, cov3D_precomp, cam, scale_modifier=1.0, antialiasing=False,
            bg=None):
    means3D, features = _f32(means3D), _f32(features)
    P, Cn = features.shape
    L = lib(Cn)
    W, H = cam.W, cam.H
    gx, gy = cam.grid
    color = np.zeros((Cn, H, W), np.float32)
    invdepth = np.zeros((1, H, W), np.float32)
    radii = np.zeros(P, np.int32)
    scales, rotations, cov3D_precomp = _f32(scales), _f32(rotations), _f32(cov3D_precomp)
    h = L.ref_forward(C.c_int(P), C.c_int(W), C.c_int(H), _p(_bg(bg, Cn)), _p(means3D), _p(features),
                      _p(_f32(opacities).reshape(-1)), _p(scales), C.c_float(scale_modifier), _p(rotations), _p(cov3D_precomp),
                      _p(cam.view), _p(cam.proj), _p(cam.campos), C.c_float(cam.tanfovx), C.c_float(cam.tanfovy),
                      C.c_int(int(antialiasing)), _p(color), _p(invdepth), _p(radii))
    st = _State(L, h)
    R = L.ref_num_rendered(st.handle)
    out = dict(color=color, invdepth=invdepth, radii=radii, R=R, _state=st,
               n_contrib=np.zeros((H, W), np.uint32), final_T=np.zeros((H, W), np.float32),
               ranges=np.zeros((gx * gy, 2), np.uint32), point_list=np.zeros(R, np.uint32),
               xy=np.zeros((P, 2), np.float32), depths=np.zeros(P, np.float32), cov3D=np.zeros((P, 6), np.float32),
               conic_opacity=np.zeros((P, 4), np.float32), tiles_touched=np.zeros(P, np.uint32),
               point_offsets=np.zeros(P, np.uint32))
    L.ref_state_read(st.handle, *(_p(out[k]) for k in ("n_contrib", "final_T", "ranges", "point_list", "xy", "depths", "cov3D",
                                                       "conic_opacity", "tiles_touched", "point_offsets")))
    return out


def backward(fwd, means3D, features, opacities, scales, rotations, cov3D_precomp, cam, dL_dcolor, dL_dinvdepth=None,
             bg=None, scale_modifier=1.0, antialiasing=False):
    means3D, features = _f32(means3D), _f32(features)
    P, Cn = features.shape
    st = fwd["_state"]
    scales, rotations, cov3D_precomp = _f32(scales), _f32(rotations), _f32(cov3D_precomp)
    dL_dcolor, dL_dinvdepth = _f32(dL_dcolor), _f32(dL_dinvdepth)
    z = lambda *s: np.full(s, np.nan, np.float32)       # the glue zeroes them: a NaN left over is its bug
    dm2, dcon, dop, dcol = z(P, 3), z(P, 4), z(P, 1), z(P, Cn)
    dinv = z(P) if dL_dinvdepth is not None else None
    dmeans, dcov, dsh, dsc, drot = z(P, 3), z(P, 6), z(P, Cn), z(P, 3), z(P, 4)
    st.L.ref_backward(st.handle, _p(_bg(bg, Cn)), _p(means3D), _p(features), _p(_f32(opacities).reshape(-1)), _p(scales),
                      C.c_float(scale_modifier), _p(rotations), _p(cov3D_precomp), _p(cam.view), _p(cam.proj), _p(cam.campos),
                      C.c_float(cam.tanfovx), C.c_float(cam.tanfovy), C.c_int(int(antialiasing)), _p(dL_dcolor),
                      _p(dL_dinvdepth), _p(dm2), _p(dcon), _p(dop), _p(dcol), _p(dinv), _p(dmeans), _p(dcov), _p(dsh), _p(dsc),
                      _p(drot))
    # dL_dsh is NOT returned: the reference's SH backward runs over the feature buffer as if it were vec3 SH coefficients
    # and reads flags its forward never wrote; the true dL/dfeature is dL_dcolors.
    return dict(dL_dmeans2D=dm2, dL_dconic=dcon, dL_dopacity=dop, dL_dcolors=dcol, dL_dinvdepths=dinv, dL_dmeans3D=dmeans,
                dL_dcov3D=dcov, dL_dscales=dsc if scales is not None else None,
                dL_drotations=drot if scales is not None else None)


def mark_visible(means3D, cam, channels=CHANNELS[0]):
    means3D = _f32(means3D)
    P = means3D.shape[0]
    out = np.zeros(P, np.uint8)
    lib(channels).ref_mark_visible(C.c_int(P), _p(means3D), _p(cam.view), _p(cam.proj), _p(out))
    return out.astype(bool)
