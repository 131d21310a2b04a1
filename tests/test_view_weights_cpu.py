"""View agreement (include/skelsplat_hip.h "View agreement") without a GPU: the op-by-op restatement the GPU tests compare bits with
is held to what the REFERENCE's own utils/similarity_utils.py returned (tests/golden/reference_similarity.npz) and to a float64
restatement; the loops' tensor-op tail is held to it; view-sharded ranks agree in every bit; the C ABI's tables are the header's."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from skelsplat_amd import _lib, view_agreement
from tests import view_weight_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_similarity.npz"))

# The reference's own path from the cosines to a weight, counted like K_* of view_weight_ref (units of 2**-24): the row sum of four
# entries <= 1 in size (three additions of sums <= 4: 4 each), minus the diagonal (<= 3), divided by 3 (the errors so far / 3, + 1);
# then log(s + 2) in fp32: the addition (<= 3), logf at 1 ulp of a value <= 1.1 (2 x 1.1), / log 3, x 0.54, + 0.46 (1 each; the
# slopes are all < 1 and are taken as 1).
K_S_REF = (3 * 4 + 3) / 3 + 1
K_W_REF = 3 + 2 * 1.1 + 1 + 1 + 1


def test_restatement_equals_the_references_functions_within_counted_roundings():
    """pairwise_cosine_similarity / compute_scaling_weights / identify_consistent_views on (4,17,3) and (4,19,3) gradients of
    magnitude 1e-6 .. 1e-2 with a zero view and an opposed view: cosines within K_COS roundings of quantities <= 1 (torch.norm and
    torch.dot sum in their own order), `scale` weights within the two paths' counted roundings, `select` exactly -- where no cosine
    sits within the cosines' allowance of the threshold, which is asserted for the fixture."""
    thr = float(GOLD["threshold"])
    for name in GOLD["names"]:
        g = GOLD[f"{name}_grads"]
        assert g.shape[0] == 4 and not g[2, 0:3].any() and np.array_equal(g[3, 3:6], -g[0, 3:6])
        mags = np.linalg.norm(g.astype(np.float64), axis=-1)
        assert 1e-6 <= mags[mags > 0].min() and mags.max() <= 1e-2
        c = REF.similarity32(g)
        dc = np.abs(c.astype(np.float64) - GOLD[f"{name}_similarity"]).max() / EPS32
        allow_c = REF.K_COS
        w = REF.scale_weights32(c)
        dw = np.abs(w.astype(np.float64) - GOLD[f"{name}_scale"]).max() / EPS32
        allow_w = REF.K_COS + max(REF.K_S(4), K_S_REF) + max(REF.K_W, K_W_REF)
        print(f"{name}: cosines {dc:.1f} of {allow_c} units of 2^-24 (ratio {dc / allow_c:.3f}); "
              f"scale weights {dw:.1f} of {allow_w:.1f} (ratio {dw / allow_w:.3f})")
        assert dc <= allow_c and dw <= allow_w
        off = ~np.eye(4, dtype=bool)[None]
        assert (np.abs(GOLD[f"{name}_similarity"] - thr)[np.broadcast_to(off, c.shape)] > allow_c * EPS32).all()
        assert np.array_equal(REF.select_weights32(c, thr).T != 0, GOLD[f"{name}_select"])
        assert GOLD[f"{name}_select"].any() and not GOLD[f"{name}_select"].all()        # some kept, some dropped


def test_identical_views_the_stated_deviation():
    """Four identical gradient rows: where the reference's mean cosine rounds above 1 its weight_function returns 0; this
    project clamps and gives the weight of perfect agreement, 1 within an ulp."""
    g, ref_w = GOLD["same_grads"], GOLD["same_scale"]
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[0], g[3])
    zero = (ref_w == 0).all(0)
    assert zero.sum() >= 8 and (~zero).sum() >= 8                    # both kinds of joint are in the fixture
    w = REF.scale_weights32(REF.similarity32(g))
    assert np.abs(w.astype(np.float64) - 1.0).max() <= 2 * EPS32
    assert np.abs(ref_w[:, ~zero].astype(np.float64) - 1.0).max() <= (REF.K_COS + K_S_REF + K_W_REF) * EPS32
    out = REF.view_weighting32(g, "scale")
    assert np.abs(out["merged"].astype(np.float64) - g[0]).max() <= 8 * EPS32 * np.abs(g[0]).max()


def _random_slots(V, P, seed, kind="random"):
    rng = np.random.default_rng(seed)
    g = (rng.normal(size=(V, P, 3)) * 10.0 ** rng.uniform(-6, -2, size=(V, P, 1))).astype(np.float32)
    if kind == "agree":
        g = (g[:1] * rng.uniform(0.5, 2.0, size=(V, 1, 1)) + 0.2 * g).astype(np.float32)
    return g


@pytest.mark.parametrize("V,P", [(2, 1), (3, 17), (4, 17), (9, 64), (31, 19)])
def test_float32_restatement_against_float64(V, P):
    """Cosines and weights at their counted allowances; the merged gradient at the weights' allowance carried through the sum
    plus the sum's own roundings; `select` wherever no cosine is within the allowance of the threshold."""
    for kind in ("random", "agree"):
        g = _random_slots(V, P, 100 * V + P, kind)
        r32, r64 = REF.view_weighting32(g, "scale"), REF.view_weighting64(g, "scale")
        assert np.abs(r32["similarity"] - r64["similarity"]).max() <= REF.K_COS * EPS32
        s64 = (r64["similarity"].sum(2) - 1.0) / max(V - 1, 1)
        smooth = (np.abs(s64) > 64 * EPS32).T                      # (the two branches meet with a step of 7e-4 at s = 0)
        allow_w = REF.weight_allowance(r64["similarity"], V)
        assert (np.abs(r32["weights"] - r64["weights"])[smooth] <= allow_w * EPS32).all()
        mag = (np.abs(r64["weights"])[..., None] * np.abs(g.astype(np.float64))).sum(0) / V
        allow_m = (allow_w + 1 + V + 1) * mag * EPS32 + 1e-45
        assert (np.abs(r32["merged"] - r64["merged"])[smooth.all(0)] <= allow_m[smooth.all(0)]).all()
        t32, t64 = REF.view_weighting32(g, "select", 0.5), REF.view_weighting64(g, "select", 0.5)
        clear = (np.abs(r64["similarity"] - 0.5) > REF.K_COS * EPS32).all(axis=(1, 2))
        assert clear.sum() >= P - 1 and np.array_equal(t32["weights"][:, clear], t64["weights"][:, clear])
        mag = np.abs(g.astype(np.float64)).sum(0) / np.maximum(t64["weights"].sum(0), 1)[:, None]
        assert (np.abs(t32["merged"] - t64["merged"])[clear] <= ((V + 1) * mag * EPS32 + 1e-45)[clear]).all()
    if V < 3:
        assert not REF.view_weighting32(g, "select", -2.0)["weights"].any()       # nobody has two others: the plain mean
        plain = np.zeros((P, 3), np.float32)
        for v in range(V):
            plain = plain + g[v]
        assert np.array_equal(REF.view_weighting32(g, "select", -2.0)["merged"], plain / np.float32(V))
    if V < 2:
        assert (r32["weights"] == 1).all()


@pytest.mark.parametrize("mode", ["scale", "select"])
def test_tensor_op_definition_equals_the_restatement_bit_for_bit(mode):
    """skelsplat_amd.view_agreement (what the loops' tensor-op tail runs) on the CPU == the numpy restatement in every bit,
    hard rows included: a zero view, an opposed view, identical views, an infinite entry."""
    for V, P in ((1, 3), (2, 5), (4, 17), (9, 20)):
        g = _random_slots(V, P, 7 * V + P)
        if V >= 4:
            g[1, 0] = 0.0
            g[2, 1] = -g[0, 1]
            g[:, 2] = g[0, 2]
            g[3, 3, 1] = np.inf
        want = REF.view_weighting32(g, mode, 0.3)
        merged, w, c = view_agreement.weighted_mean(torch.from_numpy(g), mode, 0.3)
        for got, key in ((merged, "merged"), (w, "weights"), (c, "similarity")):
            assert np.array_equal(got.numpy().view(np.uint32), want[key].view(np.uint32)), (V, P, key)


def _synthetic_view_grads(loop):
    """A view_grad_fn without a renderer: seeded raw-parameter gradients per (view, iteration); view 1 opposes view 0."""
    rows = []
    for v in loop.local_ids:
        src = 0 if v == 1 else v
        gen = torch.Generator().manual_seed(1000 * (loop.iteration // loop.acc_steps) + src)
        common = torch.randn((loop.P, 11), generator=torch.Generator().manual_seed(loop.iteration // loop.acc_steps)) * 1e-3
        row = common + torch.randn((loop.P, 11), generator=gen) * 3e-4
        rows.append(-row if v == 1 else row)
    return torch.stack(rows), torch.zeros(len(rows))


def _scene(V, dataset="h36m"):
    from skelsplat_amd.scene import GaussianModel, SyntheticScene
    sc = SyntheticScene(dataset, n_views=V, seed=3, W=32, H=24)
    J = sc.pose_3d_init.shape[0]
    gm = GaussianModel().create_from_points(sc.pose_3d_init, sc.spatial_lr_scale, J, scaling=3.9,
                                            **({"scene_type": "panoptic"} if dataset == "panoptic" else {}))
    gm.training_setup()
    return sc, gm, torch.zeros((V, J, 24, 32))


@pytest.mark.parametrize("mode", ["scale", "select"])
def test_host_tail_of_the_loop_equals_the_restatement(mode):
    """MultiViewLoop(view_weighting=mode) under a view_grad_fn: the xyz gradient Adam sees is the restatement's merge of the
    loop's own slots (first step: exp_avg = (1 - beta1) g in one rounding), its `view_weights` / `view_similarity` are the
    restatement's, and the result differs from the plain mean's."""
    from skelsplat_amd.loop import MultiViewLoop
    outs = {}
    for vw in (None, mode):
        sc, gm, hm = _scene(5)
        loop = MultiViewLoop(gm, sc.cameras, hm, dataset="h36m", accumulation_steps=5, lambda_consistency=1e-5,
                             view_grad_fn=_synthetic_view_grads, view_weighting=vw, view_threshold=0.4)
        loop.step_group()
        outs[vw] = gm._xyz.detach().clone()
        if vw is None:
            assert loop.view_weights is None and loop.view_similarity is None
            continue
        want = REF.view_weighting32(loop.accumulated_grads.numpy(), mode, 0.4)
        assert np.array_equal(loop.view_weights.numpy(), want["weights"])
        assert np.array_equal(loop.view_similarity.numpy(), want["similarity"])
        m = gm.optimizer.state[gm._xyz]["exp_avg"].numpy()
        beta1 = gm.optimizer.param_groups[0]["betas"][0]
        assert np.allclose(m, (1.0 - beta1) * want["merged"].astype(np.float64), rtol=4 * EPS32, atol=0)
        w = want["weights"]
        assert (w[1] < w[0]).any()                          # the opposed view is weighted down / dropped somewhere
    assert not torch.equal(outs[None], outs[mode])
    with pytest.raises(ValueError, match="view_weighting"):
        MultiViewLoop(gm, sc.cameras, hm, view_grad_fn=_synthetic_view_grads, view_weighting="mean")


def _sharded_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from skelsplat_amd.loop import MultiViewLoop
    out = {}
    for mode in ("scale", "select"):
        sc, gm, hm = _scene(11, "panoptic")
        loop = MultiViewLoop(gm, sc.cameras, [hm[v] for v in range(11)], dataset="panoptic", accumulation_steps=11,
                             lambda_consistency=1e-5, view_grad_fn=_synthetic_view_grads, view_weighting=mode, view_threshold=0.4)
        xyz = loop.run(33)
        out[mode] = (xyz.numpy().copy(), loop.view_weights.numpy().copy(), loop.view_similarity.numpy().copy())
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, {k: [a.tobytes() for a in v] for k, v in out.items()})
        if rank == 0:
            ret.put((out, gathered))
        dist.barrier()
        dist.destroy_process_group()
    else:
        ret.put((out, None))


def test_view_sharded_ranks_take_identical_weights():
    """11 views over 8 processes (shards 2,2,2,1,1,1,1,1; the padded all_gather rows): every rank merges the gathered table by
    the same definition -- weights, cosines and parameters agree in every bit across the ranks and with one process."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sharded_worker, args=(r, 8, port, ret)) for r in range(8)]
    for p in procs:
        p.start()
    w8, gathered = ret.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _sharded_worker(0, 1, port + 1, ret)
    w1, _ = ret.get(timeout=10)
    for mode in ("scale", "select"):
        for a8, a1 in zip(w8[mode], w1[mode]):
            assert a8.tobytes() == a1.tobytes(), mode
        for g in gathered:
            assert g[mode] == [a.tobytes() for a in w8[mode]], mode
        assert 0 < w8[mode][1].min() < w8[mode][1].max() if mode == "scale" else set(np.unique(w8[mode][1])) <= {0.0, 1.0}


def test_vw_tables_are_the_headers():
    """The three entry points added for view agreement take their signatures from tables of skelsplat_amd._lib: the header's
    prototypes name for name, type for type, in order; each is its early-stopping sibling with VW_PARAMS in front of `stream`;
    STEP_PARAMS / DV_PARAMS keep their keys; the version did not move and every declared symbol is exported."""
    raw = open(os.path.join(ROOT, "include", "skelsplat_hip.h")).read()
    assert "csrc/sks_loop_dev.h; added to sks_version 14: the number did not move" in re.sub(r"\s*\n \*\s*", " ", raw)
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    scalars = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
               "unsigned long long": ctypes.c_ulonglong}

    def prototype(symbol):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, hdr).group(1)
        out = []
        for param in proto.split(","):
            ctype, name = re.fullmatch(r"\s*(.*?)(\w+)\s*", param, flags=re.S).groups()
            out.append((name, ctypes.c_void_p if "*" in ctype else scalars[" ".join(ctype.split())]))
        return out

    assert set(_lib.VW_STEP_PARAMS) == {"sks_loop_adam_step_vw", "sks_loop_fused_step_vw", "sks_loop_fused_step_vw_dv"}
    assert [n for n, _ in _lib.VW_PARAMS] == ["vw_mode", "vw_threshold", "vw_weights", "vw_similarity"]
    lib = _lib.load()
    for symbol, sibling in (("sks_loop_adam_step_vw", "sks_loop_adam_step_es"), ("sks_loop_fused_step_vw", "sks_loop_fused_step_es"),
                            ("sks_loop_fused_step_vw_dv", "sks_loop_fused_step_es_dv")):
        table = _lib.VW_STEP_PARAMS[symbol]
        assert prototype(symbol) == list(table), symbol
        assert prototype(symbol) == prototype(sibling)[:-1] + list(_lib.VW_PARAMS) + [("stream", ctypes.c_void_p)], symbol
        assert _lib.SIGNATURES[symbol] == (ctypes.c_int, [ct for _, ct in table])
        assert hasattr(lib, symbol)
    assert set(_lib.STEP_PARAMS) == {"sks_loop_adam_step", "sks_loop_adam_step_es", "sks_loop_fused_step", "sks_loop_fused_step_es"}
    assert not set(_lib.VW_STEP_PARAMS) & (set(_lib.STEP_PARAMS) | set(_lib.DV_PARAMS))
    declared = set(re.findall(r"\b(sks_[a-z0-9_]+)\s*\(", raw))
    assert all(hasattr(lib, name) for name in declared) and declared == set(_lib.SIGNATURES)
    assert lib.sks_version() == 14
    assert _lib.vw_mode(None) == 0 and _lib.vw_mode("scale") == 1 and _lib.vw_mode("select") == 2
    with pytest.raises(ValueError):
        _lib.vw_mode("mean")
    assert REF.regime(4, 17) == ("lds", "narrow") and REF.regime(31, 19) == ("lds", "wide") and REF.regime(64, 64)[0] == "walk"
