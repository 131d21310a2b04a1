"""Result writer / evaluator compatible with the reference's per-scene .ply files and eval.py.

save_ply: scene/gaussian_model.py:250-281 (fields x,y,z,nx,ny,nz,f_dc_*,f_rest_*,opacity,scale_*,rot_*; binary little
endian, float32) without the plyfile dependency; read_ply_xyz: what eval.py:32-33 reads through open3d;
mpjpe / mpjpe_root_relative: eval.py:123-139; similarity_transform / pa_mpjpe / n_mpjpe: the aligned metrics the
reference does not report (the host counterparts of report.align_poses / report.evaluate_sequence_aligned); evaluate: eval.py:91-171 (the directory walk around them);
write_png_gray / read_png_gray: the 8-bit grey files of train.py:279-304 (save_images / save_heatmaps) without the PIL dependency."""
import os
import struct
import zlib

import numpy as np


def attribute_names(n_dc, n_rest, n_scale=3, n_rot=4):
    names = ["x", "y", "z", "nx", "ny", "nz"]
    names += [f"f_dc_{i}" for i in range(n_dc)]
    names += [f"f_rest_{i}" for i in range(n_rest)]
    names.append("opacity")
    names += [f"scale_{i}" for i in range(n_scale)]
    names += [f"rot_{i}" for i in range(n_rot)]
    return names


def save_ply(path, gm):
    """gm: object with _xyz (P,3), _features_dc (P,1,C), _features_rest (P,R,C), _opacity (P,1), _scaling, _rotation."""
    save_ply_arrays(path, gm, gm._xyz, gm._scaling, gm._rotation, gm._opacity)


def save_ply_arrays(path, gm, xyz, scaling, rotation, opacity):
    """The file save_ply writes for a model that holds ONE frame's xyz (P,3), scaling (P,3), rotation (P,4), opacity (P,1) --
    host arrays or host / device tensors, e.g. a row of a loop's `gaussians` (uncertainty.SequenceGaussians) -- with the features
    of the template `gm` (the loops' `gaussians` argument: _features_dc (P,1,C), _features_rest (P,R,C)).  Byte for byte
    save_ply of that model."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    t = lambda x: (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)).astype(np.float32)
    xyz, scaling, rotation, opacity = t(xyz), t(scaling), t(rotation), t(opacity)
    P = xyz.shape[0]
    for name, a, k in (("xyz", xyz, 3), ("scaling", scaling, None), ("rotation", rotation, None), ("opacity", opacity, 1)):
        if a.ndim != 2 or a.shape[0] != P or (k is not None and a.shape[1] != k):
            raise ValueError(f"save_ply_arrays: `{name}` must be (P,{k or 'k'}) with P = {P} (one frame), got {a.shape}")
    f_dc = t(gm._features_dc.transpose(1, 2).flatten(start_dim=1))
    f_rest = t(gm._features_rest.transpose(1, 2).flatten(start_dim=1))
    if f_dc.shape[0] != P:
        raise ValueError(f"save_ply_arrays: the template model has {f_dc.shape[0]} Gaussians, the frame {P}")
    cols = np.concatenate((xyz, np.zeros_like(xyz), f_dc, f_rest, opacity, scaling, rotation), axis=1)
    names = attribute_names(f_dc.shape[1], f_rest.shape[1], scaling.shape[1], rotation.shape[1])
    assert cols.shape[1] == len(names)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {xyz.shape[0]}"]
    header += [f"property float {n}" for n in names] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(cols, dtype="<f4").tobytes())


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png_gray(path, array_u8):
    """An (H,W) uint8 array as an 8-bit greyscale, non-interlaced PNG (what PIL's Image.fromarray(..).save writes for such an
    array, train.py:290-291, as far as the decoded pixels go).  Every row goes out with filter type 0 (none)."""
    a = np.asarray(array_u8.detach().cpu().numpy() if hasattr(array_u8, "detach") else array_u8)
    if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
        raise ValueError(f"write_png_gray: an (H,W) uint8 array is needed, got {a.dtype} {a.shape}")
    h, w = a.shape
    raw = np.zeros((h, w + 1), dtype=np.uint8)      # column 0: the filter byte of each row
    raw[:, 1:] = a
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
                + _png_chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def read_png_gray(path):
    """The (H,W) uint8 array of a file write_png_gray wrote (8-bit grey, non-interlaced, filter type 0 on every row); anything
    else is refused."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"read_png_gray: {path} is not a PNG file")
    pos, idat, shape = 8, [], None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(kind + body) & 0xffffffff:
            raise ValueError(f"read_png_gray: {path}: bad checksum in chunk {kind!r}")
        if kind == b"IHDR":
            w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if (depth, colour, comp, filt, lace) != (8, 0, 0, 0, 0):
                raise ValueError(f"read_png_gray: {path} is not an 8-bit greyscale, non-interlaced PNG")
            shape = (h, w)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if shape is None or not idat:
        raise ValueError(f"read_png_gray: {path} has no image")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != shape[0] * (shape[1] + 1):
        raise ValueError(f"read_png_gray: {path}: {raw.size} bytes of image data for {shape[1]} x {shape[0]} pixels")
    raw = raw.reshape(shape[0], shape[1] + 1)
    if raw[:, 0].any():
        raise ValueError(f"read_png_gray: {path} uses row filters (only files written by write_png_gray are read)")
    return raw[:, 1:].copy()


def read_ply_xyz(path):
    """Vertex positions of a binary-little-endian (or ascii) float PLY."""
    with open(path, "rb") as f:
        names, n, fmt = [], 0, None
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("format"):
                fmt = line.split()[1]
            elif line.startswith("element vertex"):
                n = int(line.split()[2])
            elif line.startswith("property"):
                names.append(line.split()[2])
            elif line == "end_header":
                break
        if fmt == "binary_little_endian":
            data = np.frombuffer(f.read(n * len(names) * 4), dtype="<f4").reshape(n, len(names))
        elif fmt == "ascii":
            data = np.loadtxt(f, dtype=np.float32).reshape(n, len(names))
        else:
            raise ValueError(f"unsupported PLY format {fmt}")
    ix = [names.index(k) for k in ("x", "y", "z")]
    return data[:, ix].astype(np.float64)


def mpjpe(pred, gt):
    """eval.py:123-124: mean over frames and joints of the Euclidean error; pred, gt (..., J, 3)."""
    return float(np.mean(np.linalg.norm(np.asarray(gt) - np.asarray(pred), axis=-1)))


def mpjpe_root_relative(pred, gt):
    """eval.py:133-139: both poses translated so that joint 0 is the origin."""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    return mpjpe(pred - pred[..., 0:1, :], gt - gt[..., 0:1, :])


def similarity_transform(pred, gt, valid=None, scale=True):
    """One pose: (s, R (3,3), t (3,)) minimising sum ||gt_i - (s R pred_i + t)||^2 over the joints with `valid` (all when None), R
    a proper rotation (Umeyama 1991: the SVD of the cross-covariance with the reflection repaired); `scale=False`: s = 1.
    Without a valid joint the identity.  numpy float64; on the device: report.align_poses."""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    if pred.shape != gt.shape or pred.ndim != 2 or pred.shape[1] != 3:
        raise ValueError(f"similarity_transform: pred and gt must both be (P,3), got {pred.shape} and {gt.shape}")
    v = np.ones(len(pred), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    if not v.any():
        return 1.0, np.eye(3), np.zeros(3)
    mx, my = pred[v].mean(axis=0), gt[v].mean(axis=0)
    x, y = pred[v] - mx, gt[v] - my
    U, S, Vt = np.linalg.svd(x.T @ y)
    d = np.array([1.0, 1.0, -1.0 if np.linalg.det(Vt.T @ U.T) < 0 else 1.0])
    R = (Vt.T * d) @ U.T
    sxx = float(np.sum(x * x))
    s = float(np.sum(S * d)) / sxx if scale and sxx != 0 else 1.0
    return s, R, my - s * (R @ mx)


def _frames(pred, gt, valid, what):
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    if pred.shape != gt.shape or pred.ndim not in (2, 3) or pred.shape[-1] != 3:
        raise ValueError(f"{what}: pred and gt must both be (N,P,3) or (P,3), got {pred.shape} and {gt.shape}")
    pred, gt = pred.reshape((-1,) + pred.shape[-2:]), gt.reshape((-1,) + gt.shape[-2:])
    v = np.ones(pred.shape[:2], dtype=bool) if valid is None else np.asarray(valid).astype(bool).reshape(pred.shape[:2])
    return pred, gt, v


def pa_mpjpe(pred, gt, valid=None):
    """PA-MPJPE ("Protocol #2"): the mean over frames and valid joints of the error after each frame's best similarity transform;
    pred, gt (N,J,3) or (J,3), valid (N,J) or None.  NaN without a valid joint.  On the device: report.evaluate_sequence_aligned."""
    pred, gt, v = _frames(pred, gt, valid, "pa_mpjpe")
    errs = []
    for p, g, m in zip(pred, gt, v):
        s, R, t = similarity_transform(p, g, m)
        errs.append(np.linalg.norm(g - (s * p @ R.T + t), axis=-1)[m])
    errs = np.concatenate(errs)
    return float(errs.mean()) if errs.size else float("nan")


def n_mpjpe(pred, gt, valid=None):
    """N-MPJPE: both poses relative to joint 0, the prediction scaled per frame by s = sum <x, y> / sum <x, x> over the valid
    joints (1 when the denominator is 0); the mean over frames and valid joints.  A frame whose joint 0 is masked out is NaN."""
    pred, gt, v = _frames(pred, gt, valid, "n_mpjpe")
    errs = []
    for p, g, m in zip(pred, gt, v):
        if not m.any():
            continue
        x, y = p - p[0], g - g[0]
        den = float(np.sum(x[m] * x[m]))
        s = float(np.sum(x[m] * y[m])) / den if den != 0 else 1.0
        errs.append(np.linalg.norm(y - s * x, axis=-1)[m] if m[0] else np.full(int(m.sum()), np.nan))
    errs = np.concatenate(errs) if errs else np.zeros(0)
    return float(errs.mean()) if errs.size else float("nan")


H36M_ACTIVITIES = ("Directions Discussion Eating Greeting Phoning Posing Purchases Sitting SittingDown Smoking Photo "
                   "Waiting Walking WalkDog WalkTogether").split()                     # eval.py:112-114
_S9_BROKEN = ("SittingDown 1", "Waiting 1", "Greeting")                                  # eval.py:27-28, 60-61


def _scene_entries(ply_dir, dataset):
    """eval.py:97-107: scene files of one iteration as sorted [subject, activity, frame-with-extension] triples."""
    entries = os.listdir(ply_dir)
    if dataset == "panoptic":
        parts = [[e.split("_")[0], e.split("_")[1] + "_" + e.split("_")[2], e.split("_")[-1]] for e in entries]
    elif dataset == "occlusion-person":
        parts = [[e.split("_")[0], e.split("_")[1], e.split("_")[-1]] for e in entries]
    else:
        parts = [e.split("_") for e in entries]
    return sorted(parts)


def _gt_poses(gt_path, dataset, absolute, nviews=4):
    """eval.py:54-88: ground-truth poses in sorted subject / activity order (H36M: every 64th frame; S9's three broken
    sequences are left out of the absolute metric)."""
    out = []
    for subject in sorted(os.listdir(gt_path)):
        if not subject.startswith("S"):
            continue
        for activity in sorted(os.listdir(f"{gt_path}/{subject}")):
            if dataset == "h36m":
                if absolute and subject == "S9" and activity in _S9_BROKEN:
                    continue
                out.append(np.load(f"{gt_path}/{subject}/{activity}/poses.npz")["poses"][::64])
            elif dataset == "panoptic":
                out.append(np.load(f"{gt_path}/{subject}/{activity}/poses_filtered_{nviews}.npz", allow_pickle=True)["poses"])
            else:
                out.append(np.load(f"{gt_path}/{subject}/{activity}/poses.npz", allow_pickle=True)["poses3d"])
    return np.concatenate(out, axis=0)


def evaluate(gt_path, output_path, iteration, start_id=0, end_id=10 ** 9):
    """eval.py:91-171 for one iteration: reads <output_path>/point_cloud/iteration_<it>/<scene>.ply (the files the loop's
    results are saved as, scene/__init__.py:112-114) and the dataset's ground truth under gt_path; returns a dict with
    `abs` / `rel` (absolute and root-relative MPJPE over scenes [start_id, end_id)) and, for H36M, the per-activity means
    `abs_activities` / `rel_activities` in the order of H36M_ACTIVITIES (NaN for an activity without scenes).
    Quirk kept: the relative block widens end_id to all predictions (eval.py:133-134, 160-161)."""
    dataset = "panoptic" if "panoptic" in gt_path else "occlusion-person" if "occlusion-person" in gt_path else "h36m"
    ply_dir = f"{output_path}/point_cloud/iteration_{iteration}"
    entries = _scene_entries(ply_dir, dataset)
    res = {}
    for absolute in (True, False):
        gt = _gt_poses(gt_path, dataset, absolute)
        pred, acts = [], []
        for subject, activity, frame in entries:
            if dataset == "h36m" and absolute and subject == "S9" and activity in _S9_BROKEN:
                continue
            pred.append(read_ply_xyz(f"{ply_dir}/{subject}_{activity}_{frame}"))
            acts.append(activity.split(" ")[0])
        pred, acts = np.array(pred), np.array(acts)
        if absolute:
            if end_id > pred.shape[0]:
                end_id = pred.shape[0]
        else:
            if end_id < pred.shape[0]:
                end_id = pred.shape[0]
            gt = gt - gt[:, 0, np.newaxis]
            pred = pred - pred[:, 0, np.newaxis]
        err = np.linalg.norm(gt[start_id:end_id, ...] - pred[start_id:end_id, ...], axis=-1)
        key = "abs" if absolute else "rel"
        res[key] = float(np.mean(err))
        if dataset == "h36m":
            with np.errstate(invalid="ignore"):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    res[key + "_activities"] = np.array([np.mean(err[a == acts]) for a in H36M_ACTIVITIES])
    return res
