"""Active view A/B in one process (profiles/active_view/README.md): the bench's frames in
one store, whole fits of 5000 centers with the option "active_view" 0 and 1 alternating
after one warm-up pair; prints ms per fit, view_stats and the rounds' mix of each, and
whether the two give the same centers, labels and distances.

    python3 tools/ab_active_view.py templates|walk N_TEMPLATES REPS
"""
import json
import os
import sys
import time
import types

import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
import torch
from enspara_amd.device import FrameStore
from enspara_amd import synth

data, templates, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
args = types.SimpleNamespace(templates=templates, atoms=300, seed=1, frames=1_000_000)
t0 = time.perf_counter()
if data == "walk":
    x = synth.walk(args.frames, args.atoms, args.seed)
else:
    x = bench.make_shard(args, 0, args.frames, args.frames, 16)
print("synth %.1f s" % (time.perf_counter() - t0), flush=True)
st = FrameStore(args.frames, args.atoms)
st.load(x)
st.sync()
st.set_option("candidates", -1)
out = {"data": data, "templates": templates, "runs": []}
ref = None
for rep in range(reps + 1):
    for opt in (0, 1):
        st.set_option("active_view", opt)
        st.reset_state()
        st.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx, cd, mx = st.kcenters_run(0, 5000, 0.0)
        st.sync()
        ms = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            d, a = st.download_state()
            cur = (np.asarray(idx).copy(), np.asarray(cd).copy(), d, a, mx)
            if ref is None:
                ref = cur
            else:
                same = all(np.array_equal(p, q) for p, q in zip(ref[:4], cur[:4])) and ref[4] == cur[4]
                out["option1_equals_option0"] = bool(same)
            continue        # (the first pair warms up)
        out["runs"].append({"active_view": opt, "ms": ms, "view_stats": st.view_stats(),
                            "rounds": {str(k): v for k, v in st.run_stats().items() if v[0]}})
        print(json.dumps(out["runs"][-1]), flush=True)
st.close()
for opt in (0, 1):
    v = sorted(r["ms"] for r in out["runs"] if r["active_view"] == opt)
    out["median_ms_option%d" % opt] = v[len(v) // 2]
print(json.dumps(out))
