#!/usr/bin/env python3
"""Diagnostic (the -DSOARM_DIAG_SUPPORT build via SOARM_SIM_LIB): run the contact workload for T
env-steps and print, per mesh geom, how many support queries repeated the lane's previous query's
cube-map cell or answer vertex on that geom (the batch prints its counters when freed).

    python -c "import soarm_pkg; from lerobot_mujoco_sim2real_amd import build; \
build.compile_lib('tools/_ab/lib_diag.so', defines=['-DSOARM_DIAG_SUPPORT'])"
    SOARM_SIM_LIB=tools/_ab/lib_diag.so python tools/support_repeat.py T

DEVICE=-1 N=256 runs the CPU backend, whose diagnostic build also counts, per pair, the distinct
climbing records one narrowphase call loads and how many of them the same (pair, env) loaded in
its previous call (SOARM_DIAG_REPEAT_JSON=file: the counts as json, written when the process
ends) -- what a replay of the last substep's records could prefetch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import soarm_pkg  # noqa: E402,F401
from lerobot_mujoco_sim2real_amd import workloads as W  # noqa: E402
from lerobot_mujoco_sim2real_amd.sim import BatchSim  # noqa: E402

n, T = int(os.environ.get("N", "4096")), int(sys.argv[1])
device = int(os.environ.get("DEVICE", "0"))
cm = W.model("contact", ccd=os.environ.get("CCD", W.BENCH_CCD))
print({g: name for g, name in enumerate(cm.geom_names)}, flush=True)
print({p: (int(cm.desc.pair_geom1[p]), int(cm.desc.pair_geom2[p])) for p in range(cm.desc.npair)}, flush=True)
ids = np.arange(n)
sim = BatchSim(cm, n, device)
q0 = W.initial_qpos(cm, ids, 0)
sim.reset(init_qpos=q0[:, :5], extra_qpos=q0, seed=0)
tab = {k: (torch.as_tensor(v, dtype=torch.float32, device=sim.device) if isinstance(v, np.ndarray) else v)
       for k, v in W.chirp_tables(ids, 0).items()}
for t in range(T):
    sim.step(W.chirp_action(tab, float(t), lib=torch))
if device >= 0:
    torch.cuda.synchronize()
sim.close()
