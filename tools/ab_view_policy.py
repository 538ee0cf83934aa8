"""The active view's two policy numbers (options "view_rho", "view_ratio", per mille) on
the bench's frames, in one process: whole fits of 5000 centers at every point of
rho x ratio, the points alternating inside each of REPS rounds after WARM warm-up fits;
prints ms per fit and view_stats of each and, per point, the median and the spread
(profiles/view_rebuild/README.md).

    python3 tools/ab_view_policy.py templates|walk N_TEMPLATES REPS
"""
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
import torch
from enspara_amd.device import FrameStore
from enspara_amd import synth

RHO = (600, 750, 900)
RATIO = (700, 800, 900)
WARM = 5      # (as bench.py warms up: the first fits of a process run slower)

data, templates, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
args = types.SimpleNamespace(templates=templates, atoms=300, seed=1, frames=1_000_000)
if data == "walk":
    x = synth.walk(args.frames, args.atoms, args.seed)
else:
    x = bench.make_shard(args, 0, args.frames, args.frames, 16)
st = FrameStore(args.frames, args.atoms)
st.load(x)
st.sync()
st.set_option("candidates", -1)
st.set_option("active_view", 1)
points = [(r, q) for r in RHO for q in RATIO]
out = {"data": data, "templates": templates, "runs": []}
last = None
for rep in range(reps + 1):
    for rho, ratio in (points if rep else [(750, 800)] * WARM):
        st.set_option("view_rho", rho)
        st.set_option("view_ratio", ratio)
        st.reset_state()
        st.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx, cd, mx = st.kcenters_run(0, 5000, 0.0)
        st.sync()
        ms = (time.perf_counter() - t0) * 1e3
        if last is not None:
            assert idx[-1] == last, "the policy changed a result"
        last = idx[-1]
        if rep:
            out["runs"].append({"rho": rho, "ratio": ratio, "ms": ms,
                                "view_stats": st.view_stats()})
            print(json.dumps(out["runs"][-1]), flush=True)
st.close()
out["points"] = []
for rho, ratio in points:
    v = sorted(r["ms"] for r in out["runs"] if (r["rho"], r["ratio"]) == (rho, ratio))
    out["points"].append({"rho": rho, "ratio": ratio, "ms": v, "median_ms": v[len(v) // 2],
                          "spread": (v[-1] - v[0]) / v[len(v) // 2]})
print(json.dumps(out))
