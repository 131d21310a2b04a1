"""The sparse fused-loss step (sks_geometry + sks_backward_fused_loss: k_render_bwd_wave<.., LOSS = true, ..> + k_geom_bwd) against
the CPU reference (tests/fused_loss_ref.py: oracle render, clamp, masked L2, oracle backward) on the scenes of
tests/fused_loss_cases.py -- what the bench scenes of tests/test_fullsize_gpu.py never reach: the CG 4 and CG 32 instantiations
(planes and factors), renders above 1 and below 0, several Gaussians per channel and channels per Gaussian, P != C up to 64, a
background, cov3D_precomp, scale_modifier, antialiasing, rects of more than 16 tiles cut by the border, saturated lists, a culled
lowest index, per-view sizes, heat-maps with negative entries, a view that sees nothing.  tests/test_fused_loss_cpu.py shows, on
the reference alone, that every case reaches what it is here for.

Per case (fuzz_cases.run_hard_loss_case): mask counts exactly -- the kernel re-composites the forward's sum in the forward's
order, so every mask and clamp decision is the oracle's; the loss sum within 1e-5; gradients (UNSCALED, as the entry returns them)
at rtol 1e-3 / 1e-5 of the largest entry, `big` and `culled` against the oracle's computed rounding bound like the `extreme` fuzz
cases; the same bits with 16, 8 and 4 workgroups per (view, Gaussian) and from run to run (the default picks 16 up to 400
(view, Gaussian) pairs -- every case but `lanes64`, whose 512 pairs get 8); the dense device path at rtol 1e-4; planes against
factors (same bits, S within 1e-6) where the planes come from generate_heatmaps.

`signed-gt-*`: sks_gt_tile_stats used to add gt^2 of every pixel to the totals, negative ones included, which the masked L2 of
an all-zero render leaves out; S then exceeded the reference by the sum of gt^2 over the negative pixels the render does not
cover.  These two cases fail on S, and only on S, with that kernel."""
import pytest

from tests import fused_loss_cases as FC
from tests.fuzz_cases import run_hard_loss_case
from tests.fused_loss_ref import refs_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", FC.NAMES)
def test_fused_loss_step_against_the_reference(device, name):
    case, refs = refs_of(name)
    seen = run_hard_loss_case(case.seed, device, case=case, refs=refs)
    print(f"{name}: largest |dS| / S {seen['s_ratio']:.2e}; largest gradient excess {seen['grad_excess']:.3f} "
          f"({'x 2^-24 x sum|terms|' if case.bounds else 'of rtol 1e-3 + 1e-5 max'}); default workgroups {seen['wg']:.0f}")
    assert seen["wg"] == (8 if name == "lanes64" else 16)
    if "empty" not in case.claims:
        assert seen["mask_pixels"] > 0
