"""Every scene of tests/fused_loss_cases.py through the CPU reference alone (tests/fused_loss_ref.py): the case must hold what its
recipe claims -- renders above 1 and below 0, saturated pixels, rects of more than 16 tiles, a culled lowest index, negative
heat-map pixels no rect covers -- so that no test in tests/test_fused_loss_gpu.py passes without having reached its branch.
Conditions, not measurements: the seeds in fused_loss_cases.CASES were picked so that they hold; the counts are printed."""
import numpy as np
import pytest

from tests import fused_loss_cases as FC
from tests import fused_loss_ref as FR

refs_of = FR.refs_of


def _uncovered_negatives(ref, gt):
    """Negative heat-map pixels in tiles that no Gaussian's rect touches (the oracle's per-tile ranges are empty there)."""
    C, H, W = gt.shape
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rg = ref.fwd["ranges"].reshape(gy, gx, 2)
    empty = np.repeat(np.repeat(rg[..., 1] <= rg[..., 0], 16, axis=0), 16, axis=1)[:H, :W]
    return int(((gt < 0) & empty[None]).sum())


@pytest.mark.parametrize("name", FC.NAMES)
def test_case_reaches_what_it_claims(name):
    case, refs = refs_of(name)
    assert case.P <= 64 and case.C <= 32 and len(case.gt) == case.V
    over = sum(int((r.fwd["color"] > 1).sum()) for r in refs)
    under = sum(int((r.fwd["color"] < 0).sum()) for r in refs)
    sat = sum(int((r.fwd["final_T"] < 1e-3).sum()) for r in refs)
    tiles = max(int(r.fwd["tiles_touched"].max()) for r in refs)
    visible = [int((r.fwd["radii"] > 0).sum()) for r in refs]
    moving = [int((np.abs(r.bwd["dL_dmeans3D"]).max(axis=1) > 0).sum()) for r in refs]
    print(f"{name}: P={case.P} C={case.C} sizes={case.sizes} N={[r.N for r in refs]} S={[round(r.S, 3) for r in refs]} "
          f"render>1: {over}  render<0: {under}  final_T<1e-3: {sat}  largest rect: {tiles} tiles  visible: {visible}  "
          f"Gaussians with a means3D gradient: {moving}")
    for v, r in enumerate(refs):
        assert r.fwd["color"].shape == case.gt[v].shape
        if "empty" in case.claims:
            assert r.N == 0 and r.S == 0.0 and visible[v] == 0 and not np.any(r.bwd["dL_dmeans3D"])
            continue
        assert 0 < r.N < case.gt[v].size, (v, r.N)
        assert visible[v] > 0 and np.abs(r.bwd["dL_dmeans3D"]).max() > 0, v
        assert moving[v] >= visible[v] // 2, (v, moving[v], visible[v])     # (transparent and hidden Gaussians have none)
        for k, arr in r.bwd.items():
            assert arr is None or k == "bound" or np.isfinite(arr).all(), (v, k)
    if "clamp" in case.claims:
        assert over >= 50, over
    if "signed" in case.claims:
        assert under >= 500, under
    if "saturated" in case.claims:
        assert sat >= 50, sat
    if "big-rect" in case.claims:
        assert tiles > 16, tiles
        cut = []
        for v, r in enumerate(refs):
            xy, rad, (W, H) = r.fwd["xy"], r.fwd["radii"], case.sizes[v]
            out = (xy[:, 0] - rad < 0) | (xy[:, 1] - rad < 0) | (xy[:, 0] + rad > W) | (xy[:, 1] + rad > H)
            cut.append(int((out & (rad > 0)).sum()))
        print(f"  rects cut by the image border: {cut}")
        assert min(cut) > 0
    if "culled" in case.claims:
        for v, r in enumerate(refs):
            rad = r.fwd["radii"]
            assert rad[0] == 0 and (rad[1:] > 0).any() and r.fwd["R"] > 0, v
        assert refs[0].fwd["radii"][1] == 0      # behind camera 0
    if "signed-gt" in case.claims:
        n = [_uncovered_negatives(r, case.gt[v]) for v, r in enumerate(refs)]
        print(f"  negative heat-map pixels outside every rect: {n}; on covered tiles: "
              f"{[int((case.gt[v] < 0).sum()) - n[v] for v in range(case.V)]}")
        assert min(n) >= 100, n
    if case.bg is not None:     # the background moves the backward and nothing else (quirk Q2)
        plain = FR.view_reference(case.params, case.ocams[0], case.gt[0], fwd=refs[0].fwd)
        assert plain.N == refs[0].N and plain.S == refs[0].S
        assert not np.array_equal(plain.bwd["dL_dopacity"], refs[0].bwd["dL_dopacity"])


def test_cases_are_reproducible_and_cover_the_channel_groups():
    a, b = FC.draw("signed"), FC.draw("signed")
    assert all(np.array_equal(x, y) for x, y in zip(a.params + tuple(a.gt), b.params + tuple(b.gt)))
    groups = {4 if c <= 4 else 16 if c <= 16 else 20 if c <= 20 else 32 for c in (FC.draw(n).C for n in FC.NAMES)}
    assert groups >= {4, 20, 32}      # (CG 16 and 20 are the bench scenes': tests/test_fullsize_gpu.py)
    assert FC.draw("lanes64").P == 64 and FC.draw("lanes64").V * 64 > 400      # 8 workgroups per pair by default
    sizes = FC.draw("mixed").sizes
    assert len(set(sizes)) == 2 and sizes[1][0] == sizes[0][0] + 2
    assert FC.draw_hard(5).name == FC.NAMES[5] and FC.draw_hard(5).seed == 5
