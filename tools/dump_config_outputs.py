"""Per-pod results of one BASELINE config at bench size, as .npy files.

    KSG_LIB=path/to/libksg.so python tools/dump_config_outputs.py CFG DIR

bench.py --dump-outputs writes the headline's (cfg2) results only; this writes the
same four arrays (selected, feasible, status, total; float64, queue length) for
cfg CFG from bench.py's generator (generate_native, default size), after a warm
pass and a reset.  Two libraries compute the same when the files of their DIRs
are byte-identical (cmp).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-scheduler-simulator-p9_amd"))
from ksg import Scheduler, generator as g  # noqa: E402

cfg, out = int(sys.argv[1]), sys.argv[2]
blob = g.generate_native(cfg)
s = Scheduler(json.loads(blob)["profile"])
s.load_cluster(blob)
s.schedule()
s.reset()
s.schedule()
res = s.results()
os.makedirs(out, exist_ok=True)
for name in ("selected", "feasible", "status", "total"):
    np.save(os.path.join(out, name + ".npy"), np.array([getattr(r, name) for r in res], dtype=np.float64))
print("cfg", cfg, "nodes", s.n_nodes, "pods", len(res), "window_runs", s.window_runs(),
      "scheduled", sum(1 for r in res if r.status == 0))
