"""Interleaved sweep of forced prefill plane counts on the H36M two-call step (4 x 1000 x 1000, P = C = 17):
    [SKS_PREFILL_PB=n] [SWEEP_RULE=1] python tools/sweep_prefill.py TAG nw,ng [nw,ng ...]  >  lines.jsonl
One Workspace(prefill=(nw, ng)) per pair (0,0 = prefill off), 5 rounds of 2000 steps each, the pairs interleaved round-robin; SWEEP_RULE
adds a workspace that follows the library's rule (sks_prefill_planes).  Passes per prefill block are read once per process
(SKS_PREFILL_PB), so that knob is swept over processes.  Prints one JSON line per (pair, round) -- the lines of profiles/r08_prefill_sweep.jsonl --, then a summary in `#` lines."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from skelsplat_amd import _lib, rasterizer as R
from tools.tune_fwd import setup

tag = sys.argv[1]
configs = [tuple(int(x) for x in a.split(",")) for a in sys.argv[2:]]
steps, rounds = 2000, 5
# passes per prefill block: SKS_PREFILL_PB, else the build's SKS_PREFILL_PASSES -- SWEEP_BUILD_PB says what that is when it is not the
# committed 2 (a -DSKS_PREFILL_PASSES=n variant build)
PB = int(os.environ.get("SKS_PREFILL_PB") or os.environ.get("SWEEP_BUILD_PB") or 2)
RULE = list(_lib.prefill_planes(4, 17, 17, 1000, 1000, 0))
scene, views, params, dL = setup("h36m", 4)
wss = {c: R.Workspace(prefill=(c if sum(c) else 0)) for c in configs}
if os.environ.get("SWEEP_RULE"):
    configs.append("rule"); wss["rule"] = R.Workspace()

def step(ws):
    c, i, r, st = R.forward_views(views, *params, workspace=ws)
    return R.backward_views(st, *params, dL, workspace=ws, want_mean=True)

for c in configs:
    for _ in range(300):
        step(wss[c])
torch.cuda.synchronize()
res = {c: [] for c in configs}
for r in range(rounds):
    for c in configs:
        ws = wss[c]
        for _ in range(50):
            step(ws)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(ws)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / steps * 1e6
        res[c].append(us)
        line = {"process": tag, "passes_per_block": PB, "planes_wave_geom": c, "round": r, "us_per_step": round(us, 3)}
        if c == "rule":
            line["rule_planes"] = RULE
        print(json.dumps(line), flush=True)
for c in configs:
    v = sorted(res[c])
    print(f"# {tag} pb={PB} {c}: min {v[0]:.2f} med {v[len(v)//2]:.2f} max {v[-1]:.2f}", flush=True)
print("# rule:", _lib.prefill_planes(4, 17, 17, 1000, 1000, 0))
