"""The optimised Gaussians read back as the pose's uncertainty, on the device (csrc/sks_uncertainty.hip): what the reference's
analysis scripts take from the covariance a scene leaves behind.

joint_uncertainty    per joint the covariance, its eigenvalues, trace, determinant and anisotropy, and the squared Mahalanobis
                     distance of the ground truth (utils/analize_error_confidence_correlation.py:38-60, 117-143);
covariance_matrices  the (..,3,3) matrices of the six stored entries (unpack_covariance, utils/general_utils.py:144-165);
view_footprints      per (view, joint) the two variances of the blob the pseudo-GT is drawn with and their ratio
                     (utils/analize_2D_anisotropy.py:50);
calibration          the share of ground-truth joints inside the k-sigma ellipsoids, overall and per joint
                     (percent_inside_sigmas, percent_inside_sigmas_per_joint);
SequenceGaussians    what FrameBatchLoop / FramePipeline(keep_gaussians=True) keep of every frame of a sequence.

Everything takes device tensors, enqueues one launch on the current stream and never synchronises.  The eigenvalues are analytic
(the squared standard deviations the model stores, sorted) and the Mahalanobis distance is formed by whitening: DESIGN.md."""
import collections
import ctypes

import torch

from . import _lib

JointUncertainty = collections.namedtuple("JointUncertainty", "cov6 eigenvalues trace det anisotropy d2")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _block(t, name, last, what, lead=None):
    """`t` as a contiguous float32 (N,P,last) tensor on a ROCm device (a single (P,last) pose gains the frame axis)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what}: `{name}` must be a tensor on a ROCm device")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: `{name}` must be float32, got {t.dtype}")
    if t.dim() not in (2, 3) or t.shape[-1] != last or t.numel() == 0:
        raise ValueError(f"{what}: `{name}` must be (N,P,{last}) or (P,{last}), got {tuple(t.shape)}")
    t = (t[None] if t.dim() == 2 else t).contiguous()
    if lead is not None and (tuple(t.shape[:2]) != tuple(lead.shape[:2]) or t.device != lead.device):
        raise ValueError(f"{what}: `{name}` is {tuple(t.shape)} on {t.device}, the joints are {tuple(lead.shape)} on {lead.device}")
    return t


def joint_uncertainty(xyz, scaling_raw, rotation_raw, scaling_modifier=1.0, gt=None):
    """xyz (N,P,3), scaling_raw (N,P,3) -- the model's `_scaling`: its logarithms --, rotation_raw (N,P,4), all float32 on the
    device; gt (N,P,3) or None -> JointUncertainty of
      cov6 (N,P,6)         xx, xy, xz, yy, yz, zz of Sigma = R S S^T R^T, S = scaling_modifier * exp(scaling_raw), R from the
                           normalised quaternion (GaussianModel.get_covariance), in the heat-map generator's float sequence;
      eigenvalues (N,P,3)  l1 >= l2 >= l3 = the squared diagonal of S, sorted;
      trace, det, anisotropy (N,P)   (xx + yy) + zz, (l1 l2) l3, l1 / l3;
      d2 (N,P) or None     the squared Mahalanobis distance of `gt` from `xyz` under Sigma.
    A single (P,..) pose comes back without the frame axis.  One launch (sks_joint_uncertainty) behind torch.exp."""
    what = "joint_uncertainty"
    single = torch.is_tensor(xyz) and xyz.dim() == 2
    x = _block(xyz, "xyz", 3, what)
    s = _block(scaling_raw, "scaling_raw", 3, what, x)
    q = _block(rotation_raw, "rotation_raw", 4, what, x)
    g = None if gt is None else _block(gt, "gt", 3, what, x)
    N, P = x.shape[:2]
    dev = x.device
    act = torch.exp(s)      # (as loop.py activates the scales for the heat-maps)
    cov6 = torch.empty((N, P, 6), dtype=torch.float32, device=dev)
    spec = torch.empty((N, P, 6), dtype=torch.float32, device=dev)
    d2 = None if g is None else torch.empty((N, P), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sks_joint_uncertainty(N, P, x.data_ptr(), act.data_ptr(), q.data_ptr(), float(scaling_modifier),
                                               None if g is None else g.data_ptr(), cov6.data_ptr(), spec.data_ptr(),
                                               None if d2 is None else d2.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_joint_uncertainty")
    out = (cov6, spec[..., 0:3], spec[..., 3], spec[..., 4], spec[..., 5], d2)
    if single:
        out = tuple(None if t is None else t[0] for t in out)
    return JointUncertainty(*out)


def covariance_matrices(cov6):
    """(..,6) xx, xy, xz, yy, yz, zz -> (..,3,3) symmetric matrices (unpack_covariance, general_utils.py:144-165)."""
    if not torch.is_tensor(cov6) or cov6.shape[-1] != 6:
        raise ValueError(f"covariance_matrices: cov6 must be a (..,6) tensor, got {tuple(cov6.shape) if torch.is_tensor(cov6) else type(cov6).__name__}")
    return cov6[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(tuple(cov6.shape[:-1]) + (3, 3))


def view_footprints(xyz, scaling_raw, rotation_raw, cameras=None, views=None, scaling_modifier=1.0, frames=1):
    """Per (view, joint) the variances l1 >= l2, in px^2, of the blob that view's pseudo-GT heat-map is drawn with -- the numbers
    sks_heatmap_factors forms before its square roots, bit for bit -- and their ratio (analize_2D_anisotropy.py:50).
    xyz (J,3), scaling_raw (J,3), rotation_raw (J,4); `cameras` (a list of V) or `views` (a ViewBatch of them, reused; with
    `views.table` set -- a loop over a rig bank -- the per-view scalars are read from the device, sks_view_footprints' second
    form).  `frames` > 1: V = frames x Vf views frame-major, parameters stacked (frames,J,..).
    Returns (lambdas (V,J,2), anisotropy (V,J))."""
    from ._base import ViewBatch
    what = "view_footprints"
    if (cameras is None) == (views is None):
        raise ValueError("view_footprints takes either cameras= or views= (a ViewBatch)")
    if views is None:
        if not torch.is_tensor(xyz) or not xyz.is_cuda:
            raise ValueError("view_footprints: `xyz` must be a tensor on a ROCm device")
        views = ViewBatch.from_cameras([c.to(xyz.device) for c in cameras], allow_mixed=True)
    frames = int(frames)
    V = views.V
    stacked = torch.is_tensor(xyz) and xyz.dim() == 3
    if frames < 1 or V % frames or (frames > 1 and (not stacked or xyz.shape[0] != frames)) or (frames == 1 and stacked and xyz.shape[0] != 1):
        raise ValueError(f"view_footprints: frames = {frames} needs frames x Vf views (got {V}) and parameters stacked (frames,J,..)")
    x = _block(xyz, "xyz", 3, what)
    s = _block(scaling_raw, "scaling_raw", 3, what, x)
    q = _block(rotation_raw, "rotation_raw", 4, what, x)
    dev = x.device
    if views.viewmatrix.device != dev:
        raise ValueError(f"view_footprints: the views are on {views.viewmatrix.device}, the joints on {dev}")
    J = x.shape[1]
    act = torch.exp(s)
    lam = torch.empty((V, J, 2), dtype=torch.float32, device=dev)
    host = views.table is None
    with torch.cuda.device(dev):
        rc = _lib.load().sks_view_footprints(V, J, views.W, views.H, x.data_ptr(), act.data_ptr(), q.data_ptr(),
                                             float(scaling_modifier), views.viewmatrix.data_ptr(),
                                             views.tanfovx if host else None, views.tanfovy if host else None,
                                             views.wh if host else None, None if host else views.table.data_ptr(), frames,
                                             lam.data_ptr(), _stream(dev))
    _lib.check(rc, "sks_view_footprints")
    return lam, lam[..., 0] / lam[..., 1]


def calibration(d2, ks=(1, 2, 3), valid=None):
    """d2 (N,P) float32 on the device (joint_uncertainty's), `ks` up to 8 sigma levels, `valid` (N,) bool or None (frames with
    False are left out) -> dict of
      overall (K,)     float64: the share of entries with d2 <= k^2 (percent_inside_sigmas);
      per_joint (P,K)  float64: the same per joint (percent_inside_sigmas_per_joint);
      counts (1+P,K+1) int32: the counts behind them, row 0 overall, the last column the entries counted at all.
    NaN distances are not counted; a row without entries gives NaN.  One launch (sks_calibration), exact integer counts."""
    what = "calibration"
    if not torch.is_tensor(d2) or not d2.is_cuda:
        raise ValueError(f"{what}: `d2` must be a tensor on a ROCm device")
    if d2.dtype != torch.float32 or d2.dim() != 2 or d2.numel() == 0:
        raise ValueError(f"{what}: `d2` must be float32 (N,P), got {d2.dtype} {tuple(d2.shape)}")
    levels = [float(k) for k in ks]
    K = len(levels)
    if not 1 <= K <= _lib.SKS_CALIBRATION_MAX_K:
        raise ValueError(f"{what}: {K} sigma levels, 1 .. {_lib.SKS_CALIBRATION_MAX_K} (SKS_CALIBRATION_MAX_K)")
    if any(not (k > 0.0) or k == float("inf") for k in levels):
        raise ValueError(f"{what}: ks = {tuple(ks)!r}: every level must be finite and > 0")
    d2 = d2.contiguous()
    N, P = d2.shape
    dev = d2.device
    mask = None
    if valid is not None:
        mask = torch.as_tensor(valid)
        if tuple(mask.shape) != (N,):
            raise ValueError(f"{what}: valid must be (N,) = ({N},), got {tuple(mask.shape)}")
        mask = mask.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8)
    counts = torch.empty((1 + P, K + 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sks_calibration(N, P, d2.data_ptr(), None if mask is None else mask.data_ptr(), K,
                                         ctypes.cast((ctypes.c_float * K)(*levels), ctypes.c_void_p), counts.data_ptr(),
                                         _stream(dev))
    _lib.check(rc, "sks_calibration")
    frac = counts[:, :K].to(torch.float64) / counts[:, K:].to(torch.float64)
    return dict(overall=frac[0], per_joint=frac[1:], counts=counts)


class SequenceGaussians:
    """What `optimize_sequence` of a FrameBatchLoop / FramePipeline built with keep_gaussians=True keeps of all N frames: xyz
    (N,P,3), scaling (N,P,3), rotation (N,P,4), opacity (N,P,1) -- the raw parameters scene.save_h36m writes
    (scene/gaussian_model.py:250-281), float32 on the device, each batch's rows copied on the batch's own stream like the
    joints.  With early stopping a frame's rows are its parameters at its stopping iteration."""

    def __init__(self, joints):
        """`joints`: the (N,P,3) tensor optimize_sequence returns -- `xyz` IS that tensor, so keeping the Gaussians adds three
        copies per batch (scaling, rotation, opacity) to the one of the joints."""
        N, P, dev = joints.shape[0], joints.shape[1], joints.device
        new = lambda k: torch.empty((N, P, k), dtype=torch.float32, device=dev)
        self.xyz, self.scaling, self.rotation, self.opacity = joints, new(3), new(4), new(1)

    def take(self, loop, b, n):
        """Frames b .. b + n of the sequence are the first n frames of `loop`'s batch (on the current stream, behind the copy of
        the joints)."""
        self.scaling[b:b + n] = loop.scaling[:n]
        self.rotation[b:b + n] = loop.rotation[:n]
        self.opacity[b:b + n] = loop.opacity[:n]

    def uncertainty(self, gt=None, scaling_modifier=1.0):
        """joint_uncertainty of every frame's Gaussians (gt (N,P,3) or None)."""
        return joint_uncertainty(self.xyz, self.scaling, self.rotation, scaling_modifier, gt)

    def footprints(self, cameras_or_views, frame=0, scaling_modifier=1.0):
        """view_footprints of ONE frame's Gaussians in a list of cameras or a ViewBatch."""
        from ._base import ViewBatch
        kw = {"views": cameras_or_views} if isinstance(cameras_or_views, ViewBatch) else {"cameras": cameras_or_views}
        return view_footprints(self.xyz[frame], self.scaling[frame], self.rotation[frame], scaling_modifier=scaling_modifier, **kw)
