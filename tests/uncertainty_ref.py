"""float64 numpy references for csrc/sks_uncertainty.hip and the rounding allowances its float results are held to.  No torch, no
device.  Inputs are the float32 values the kernel reads, widened exactly; `modifier` is widened from float32 too.

The allowances are counted from the kernels' float sequences (csrc/sks_gauss.h gaussian_sigma, k_joint_uncertainty), u = 2^-24,
first order in u with the next integer taken for the second-order terms:

  R, a rotation entry.  |q|^2 = ((q0^2 + q1^2) + q2^2) + q3^2: four roundings on a sum of positive terms, 4u; its root halves
    that and rounds, 3u; a normalised component q_i / |q| 4u.  A product of two of them 9u; y^2 + z^2 10u of a sum <= 1, doubled
    exactly; 1 - 2(y^2 + z^2) is off by 10u x 2 + u = 21u ABSOLUTE.  x y - r z: 9u (|xy| + |rz|) + u, and |xy| + |rz| <= 1/2, doubled:
    10u.  K_R = 22: |R_float - R| <= 22u for every entry, absolute (a small entry has no relative accuracy).
  cov6, entry ab = sum_k (R_ak sd_k)(R_bk sd_k), sd_k = modifier x s_k.  The two rotation entries: 22u (|R_ak| + |R_bk|) sd_k^2; the
    roundings of the term itself -- sd_k twice, the two products L, their product, two additions -- 7u |R_ak R_bk| sd_k^2, K_TERM = 8:
        allowance_ab = u sum_k sd_k^2 (22 (|R_ak| + |R_bk|) + 8 |R_ak R_bk|)
  trace = (xx + yy) + zz: the three diagonal allowances and two additions of positive numbers, 2u x trace (K_TRACE_SUM = 3).
  eigenvalues: fl(fl(modifier s_k)^2), no allowance -- they are compared BIT for bit with the same two float32 products in numpy.
  det = (l1 l2) l3: three eigenvalues at 3u (sd_k rounded, counted twice, and the square), two products: 11u, K_DET = 12.
  anisotropy = l1 / l3: 3u + 3u + u, K_ANISO = 8.
  d2.  n_k = (R_0k d_0 + R_1k d_1) + R_2k d_2 with d = gt - xyz: the rotation entries 22u |d|_1, the subtractions u |d|_1, three
    products and two additions 3u |d|_1: 26u |d|_1.  w_k = n_k / sd_k adds sd_k's rounding and the division's, 2u |w_k|, and
    |w_k| <= |d|_1 / sd_k =: B_k: 28u B_k.  w_k^2: 2 |w_k| x 28u B_k + u w_k^2 <= 57u B_k^2; two additions of positive numbers 2u:
        allowance = K_D2 u sum_k B_k^2,  K_D2 = 60."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
K_R, K_TERM, K_TRACE_SUM, K_DET, K_ANISO, K_D2 = 22.0, 8.0, 3.0, 12.0, 8.0, 60.0


def _f64(a):
    return np.asarray(a, np.float64)


def rotation_ref(q):
    """(..,4) raw quaternions (r, x, y, z) -> (..,3,3) rotation of the normalised quaternion (general_utils.py:87-108)."""
    q = _f64(q)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    r, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def sigmas_ref(scales, modifier=1.0):
    """The standard deviations sd_k = modifier x s_k in float64 (modifier as the float32 the kernel receives)."""
    return float(np.float32(modifier)) * _f64(scales)


def covariance_ref(scales, q, modifier=1.0):
    """(..,3,3) Sigma = R diag(sd)^2 R^T (gaussian_model.py:33-37)."""
    R, sd = rotation_ref(q), sigmas_ref(scales, modifier)
    L = R * sd[..., None, :]
    return L @ np.swapaxes(L, -1, -2)


def cov6_of(cov):
    """(..,3,3) -> (..,6) xx, xy, xz, yy, yz, zz (strip_symmetric, general_utils.py:73-85)."""
    return np.stack([cov[..., 0, 0], cov[..., 0, 1], cov[..., 0, 2], cov[..., 1, 1], cov[..., 1, 2], cov[..., 2, 2]], -1)


def matrices_of(cov6):
    """(..,6) -> (..,3,3) (unpack_covariance, general_utils.py:144-165)."""
    cov6 = np.asarray(cov6)
    return cov6[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(cov6.shape[:-1] + (3, 3))


def cov6_allowance(scales, q, modifier=1.0):
    """(..,6), in absolute terms (U32 included)."""
    R, sd2 = np.abs(rotation_ref(q)), sigmas_ref(scales, modifier) ** 2
    out = []
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append((sd2 * (K_R * (R[..., a, :] + R[..., b, :]) + K_TERM * R[..., a, :] * R[..., b, :])).sum(-1))
    return U32 * np.stack(out, -1)


def eigenvalues_ref(scales, modifier=1.0):
    """(..,3) l1 >= l2 >= l3 in float64: the squared standard deviations, sorted."""
    return np.sort(sigmas_ref(scales, modifier) ** 2, axis=-1)[..., ::-1]


def eigenvalues_f32(scales, modifier=1.0):
    """What the kernel stores, bit for bit: the float32 products fl(fl(modifier s_k)^2), sorted."""
    sd = np.float32(modifier) * np.asarray(scales, np.float32)
    assert sd.dtype == np.float32
    return np.sort(sd * sd, axis=-1)[..., ::-1]


def trace_ref(scales, modifier=1.0):
    return (sigmas_ref(scales, modifier) ** 2).sum(-1)


def trace_allowance(scales, q, modifier=1.0):
    a6 = cov6_allowance(scales, q, modifier)
    return a6[..., 0] + a6[..., 3] + a6[..., 5] + K_TRACE_SUM * U32 * trace_ref(scales, modifier)


def det_ref(scales, modifier=1.0):
    return (sigmas_ref(scales, modifier) ** 2).prod(-1)


def d2_ref(xyz, gt, scales, q, modifier=1.0):
    """Squared Mahalanobis distance by whitening: w = diag(sd)^-1 R^T (gt - xyz), d2 = |w|^2."""
    d = _f64(gt) - _f64(xyz)
    w = np.einsum("...ik,...i->...k", rotation_ref(q), d) / sigmas_ref(scales, modifier)
    return (w * w).sum(-1)


def d2_inverse_ref(xyz, gt, cov):
    """The reference's form (analize_error_confidence_correlation.py:48-54): delta^T inv(cov) delta."""
    d = _f64(gt) - _f64(xyz)
    return np.einsum("...i,...ij,...j->...", d, np.linalg.inv(_f64(cov)), d)


def d2_basis(xyz, gt, scales, modifier=1.0):
    """sum_k (|delta|_1 / sd_k)^2, the sum of |terms| the d2 allowance is stated in."""
    d1 = np.abs(_f64(gt) - _f64(xyz)).sum(-1, keepdims=True)
    return ((d1 / sigmas_ref(scales, modifier)) ** 2).sum(-1)


def d2_basis_tight(xyz, gt, scales, q, modifier=1.0):
    """sum_k ((|R|^T |delta|)_k / sd_k)^2 <= d2_basis: the tighter basis measurements are reported in."""
    d = np.abs(_f64(gt) - _f64(xyz))
    n = np.einsum("...ik,...i->...k", np.abs(rotation_ref(q)), d)
    return ((n / sigmas_ref(scales, modifier)) ** 2).sum(-1)


def d2_allowance(xyz, gt, scales, modifier=1.0):
    return K_D2 * U32 * d2_basis(xyz, gt, scales, modifier)


def calibration_counts_ref(d2, ks, valid=None):
    """d2 (N,P) -> counts (1 + P, K + 1) int64 as sks_calibration defines them: entries of valid frames that are not NaN, compared
    with k x k -- in the dtype of d2: float32 d2 against the float32 product, the kernel's comparison exactly."""
    d2 = np.asarray(d2)
    N, P = d2.shape
    ok = ~np.isnan(d2)
    if valid is not None:
        ok &= np.asarray(valid, bool)[:, None]
    K = len(ks)
    per = np.zeros((P, K + 1), np.int64)
    with np.errstate(invalid="ignore"):
        for i, k in enumerate(ks):
            t = np.asarray(k, d2.dtype) * np.asarray(k, d2.dtype)
            per[:, i] = ((d2 <= t) & ok).sum(0)
    per[:, K] = ok.sum(0)
    return np.concatenate([per.sum(0, keepdims=True), per], 0)


def fractions_of(counts):
    """(overall (K,), per_joint (P,K)) float64 = counts[:, k] / counts[:, K]; a row without entries gives NaN."""
    counts = np.asarray(counts, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = counts[:, :-1] / counts[:, -1:]
    return f[0], f[1:]
