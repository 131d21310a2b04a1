"""Randomised cases of the binned path against the CPU oracle (tests/fuzz_cases.py).  The sweep found what the hand-written cases
had missed: a list longer than a wavefront whose first half-tile saturates early left its later entries without strip masks, and
the backward skipped them in the other half (seeds 1017, 1033, 2034 below)."""
import pytest

from tests.fuzz_cases import run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [1007, 1017, 1033, 2034, 2110, 2135, 2164, 2173])
def test_cases_the_sweep_once_failed(device, seed):
    run_case(seed, device)


@pytest.mark.parametrize("block", range(6))
def test_random_binned_cases_match_the_oracle(device, block):
    for seed in range(5000 + 25 * block, 5000 + 25 * (block + 1)):
        run_case(seed, device)


@pytest.mark.parametrize("block", range(3))
def test_extreme_cases_within_the_computed_rounding_allowance(device, block):
    """Every 5th seed is `extreme` (Gaussians behind the cameras, sub-pixel, image-sized needles, sheets, opacity 0 / 1 / 1/255):
    their gradients cancel to 1e-5 of their terms, so they are held to rtol 1e-3 plus util.BOUND_KAPPA x 2^-24 x the oracle's
    sum of |terms| (oracle.backward(bounds=True)) -- a computed allowance, ~5 x the largest excess measured over 4 000
    such cases (tools/fuzz_bound_calib.py, profiles/r05_fuzz_bound_calib.txt), quaternion gradients included; the forward stays
    bit for bit.  No fraction of the tensor's largest entry anywhere."""
    from tests import util
    stats = {}
    for seed in range(20000 + 100 * block, 20000 + 100 * (block + 1), 5):
        run_case(seed, device, stats=stats)
    assert stats and max(stats.values()) <= util.BOUND_KAPPA      # (what the cases needed of the allowance)


@pytest.mark.parametrize("block", range(3))
def test_random_one_call_steps_equal_the_two_calls_bit_for_bit(device, block):
    from tests.fuzz_cases import run_one_call_case
    live = 0
    for seed in range(700 + 20 * block, 700 + 20 * (block + 1)):
        r = run_one_call_case(seed, device)
        live += r["visible"] > 0 and r["grad"] > 0
    assert live >= 15


@pytest.mark.parametrize("block", range(4))
def test_random_fused_loss_steps_match_the_dense_path(device, block):
    from tests.fuzz_cases import run_fused_loss_case
    live = 0
    for seed in range(300 + 25 * block, 300 + 25 * (block + 1)):
        r = run_fused_loss_case(seed, device)
        live += r["mask_pixels"] > 100 and r["grad"] > 0
    assert live >= 20     # (the cases are not vacuous)


@pytest.mark.parametrize("block", range(3))
def test_random_production_loops_match_the_dense_loop(device, block):
    from tests.fuzz_cases import run_loop_case
    live = 0
    for seed in range(100 + 20 * block, 100 + 20 * (block + 1)):
        live += run_loop_case(seed, device)["moved_mm"] > 1.0    # (one camera: scene extent 0, the joints do not move)
    assert live >= 12


@pytest.mark.parametrize("block", range(2))
def test_random_frame_batches_equal_separate_loops_bit_for_bit(device, block):
    from tests.fuzz_cases import run_frames_case
    live = 0
    for seed in range(100 + 20 * block, 100 + 20 * (block + 1)):
        live += run_frames_case(seed, device)["moved_mm"] > 1.0
    assert live >= 12


@pytest.mark.parametrize("block", range(2))
def test_random_models_through_the_drop_in_surface_fast_vs_literal_activations(device, block):
    from tests.fuzz_cases import run_dropin_case
    for seed in range(100 + 25 * block, 100 + 25 * (block + 1)):
        assert run_dropin_case(seed, device)["visible"] > 0


@pytest.mark.parametrize("block", range(2))
def test_random_shapes_through_the_smaller_ops(device, block):
    from tests.fuzz_cases import run_ops_case
    for seed in range(100 + 30 * block, 100 + 30 * (block + 1)):
        run_ops_case(seed, device)


@pytest.mark.parametrize("seed", range(400, 412))
def test_random_shapes_at_the_geometry_boundaries(device, seed):
    """Shapes drawn around the launch-regime thresholds (tests/geometry_cases.py fuzz_case: +- a tile, +- a pixel, every W mod 4)."""
    from tests.geometry_cases import run_case as run_geom_case
    r = run_geom_case(seed, device)
    assert r["visible"] > 0 and r["grad"] > 0


@pytest.mark.parametrize("seed", range(600, 612))
def test_random_list_lengths_at_the_sorter_thresholds(device, seed):
    """Tile lists drawn around the lengths at which the binned path changes sorter (tests/list_length_cases.py fuzz_case: +- 1,
    +- 64; equal depths, a half-tile that saturates early, every channel form)."""
    from tests.list_length_cases import run_case as run_lists_case
    r = run_lists_case(seed, device)
    assert r["n_contrib"] > 0.75 * r["longest"] and r["grad"] > 0
