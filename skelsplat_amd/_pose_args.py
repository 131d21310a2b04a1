"""The argument handling the pose entry points share -- triangulation.triangulate_sequence, initial_guess.fuse_predictions,
reprojection.reproject and refine_triangulation, and reprojection.SequenceReprojection: what they accept (arrays or tensors,
cameras or projection matrices, one frame or N), what they refuse, what the library is handed, and how results go back."""
import numpy as np
import torch

MAX_VIEWS = 64      # SKS_MAX_VIEWS


def as_tensor(a):
    """(tensor, as_array): a tensor stays where it is; anything else becomes a CPU tensor and the caller gets arrays back."""
    return (a, False) if torch.is_tensor(a) else (torch.as_tensor(np.asarray(a)), True)


def projections(proj_or_cameras, dev):
    """A tensor, an ndarray, a list of matrices or a list of cameras (through triangulation.projection_matrices) -> a float64
    tensor (V,3,4) or (N,V,3,4) on `dev`."""
    if torch.is_tensor(proj_or_cameras):
        return proj_or_cameras.to(device=dev, dtype=torch.float64)
    if not isinstance(proj_or_cameras, np.ndarray):
        from .triangulation import projection_matrices
        seq = list(proj_or_cameras)
        proj_or_cameras = np.asarray(seq) if seq and not hasattr(seq[0], "K") else projection_matrices(seq)
    return torch.as_tensor(proj_or_cameras, dtype=torch.float64).to(dev)


def check_shapes(P, N, V, J):
    if N < 1 or J < 1:
        raise ValueError(f"N = {N} frames of J = {J} joints: at least one of each")
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"{V} views: a joint takes 1 .. {MAX_VIEWS} (SKS_MAX_VIEWS)")
    if tuple(P.shape) not in ((V, 3, 4), (N, V, 3, 4)):
        raise ValueError(f"projection matrices must be (V,3,4) = {(V, 3, 4)} or (N,V,3,4) = {(N, V, 3, 4)}, got {tuple(P.shape)}")


def check_valid(valid, single, dev, shape):
    """`valid` -> None or a contiguous bool tensor of `shape` = (N,V,J) on `dev`; one frame (`single`) comes as (V,J)."""
    if valid is None:
        return None
    valid = as_tensor(valid)[0].to(device=dev, dtype=torch.bool)
    valid = valid[None] if single else valid
    if tuple(valid.shape) != shape:
        raise ValueError(f"valid must be (N,V,J) = {shape}, got {tuple(valid.shape)}")
    return valid.contiguous()


def as_real(t):
    """float64 stays, everything else is read as float32 (the two forms the library takes), contiguous."""
    return (t if t.dtype == torch.float64 else t.to(torch.float32)).contiguous()


def pointers(t):
    """(float pointer, double pointer) of a float32 / float64 tensor, or (None, None)."""
    if t is None:
        return None, None
    return (None, t.data_ptr()) if t.dtype == torch.float64 else (t.data_ptr(), None)


def byte_pointer(t):
    """The pointer of a contiguous bool / uint8 tensor as the library reads it, or None."""
    return None if t is None else t.view(torch.uint8).data_ptr()


def rig_stride(P, V):
    """Doubles between two frames' matrices: V * 12 for (N,V,3,4), one rig per frame; 0 for (V,3,4), one rig for all."""
    return V * 12 if P.dim() == 4 else 0


def check_out(out, shape, dtypes, dev, single=False, name="`out`"):
    """`out` as a view of `shape` = (N,..): it must be a contiguous tensor of that shape -- or, for one frame (`single`), of
    shape[1:] -- with one of `dtypes` on `dev`."""
    want = tuple(shape[1:] if single and torch.is_tensor(out) and out.dim() == len(shape) - 1 else shape)
    if (not torch.is_tensor(out) or tuple(out.shape) != want or out.dtype not in dtypes or out.device != dev
            or not out.is_contiguous()):
        kinds = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{name} must be a contiguous {kinds} tensor of shape {want} on {dev}")
    return out.view(shape)


def finish(t, single, as_array):
    """A result as the caller gets it: without the frame axis for one frame, an array for a caller who gave arrays."""
    t = t[0] if single else t
    return t.numpy() if as_array else t


def results(res, out, single, as_array, extras=()):
    """The return tail: `out` itself when it was given, else `res` finished; the `extras` asked for appended."""
    ret = out if out is not None else finish(res, single, as_array)
    extras = [finish(t, single, as_array) for t in extras]
    return (ret, *extras) if extras else ret
