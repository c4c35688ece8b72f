#!/usr/bin/env python3
"""Time a chained sim_ik_box call against the per-frame sim_ik_dls loop that generate() runs.

    python tools/bench_ik_box.py [--n 4096] [--frames 300] [--repeats 10]
                                 [--resusage FILE.json] [--out profiles/ik_box.json]

Needs a GPU.  The work: `--n` envs, each following the reference's Fig8 path (position targets,
`control/TrajectoryGenerator.py:138-166`) over `--frames` points from its own phase offset,
warm-started from qpos0 and chained frame to frame.

(a) one `sim_ik_box` call with nframe = frames: the frames are chained inside the kernel.
(b) the way `CartesianTrajectoryGenerator.generate()` produces a path: one `sim_ik_dls` launch per
    frame, `ok` read back to the host after each, failed envs put back to their last solution.

The two solve different problems ((a) the casadi_ik cost inside the joint ranges, tol 1e-4 on the
projected gradient; (b) unconstrained DLS to |err| < 1e-6), so the pair is not a like-for-like
speed-up: the only claim it supports or refutes is that (a) is not slower than (b).

Timing: warm-up runs first; (a) device events around the launch, (b) the host clock around the
loop (it synchronises every frame), ending in a synchronise; the median, minimum and maximum of
`--repeats` runs.  One JSON line: both times, the per-solve iteration histograms, the fraction of
solves that converged, and k_ik_box's register / scratch counts (tools/resusage.py; `--resusage`
takes a file written earlier by `--dump-resusage`, so the compile need not run on the GPU box).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import soarm_pkg  # noqa: F401,E402


def ik_box_resusage(path=None):
    if path:
        rows = json.load(open(path))
    else:
        import resusage
        rows = resusage.rows(["soarm_sim.hip"])
    for r in rows:
        if "k_ik_box" in r["name"]:
            return {"vgpr": int(r["VGPRs"]), "agpr": int(r["AGPRs"]), "sgpr": int(r["TotalSGPRs"]),
                    "vgpr_spill": int(r["VGPRs Spill"]), "sgpr_spill": int(r["SGPRs Spill"]),
                    "scratch_bytes_per_lane": int(r["ScratchSize [bytes/lane]"])}
    return None


def hist(it):
    return np.bincount(np.asarray(it).ravel()).tolist()


def spread(ms):
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--resusage", default=None, help="JSON written by --dump-resusage")
    ap.add_argument("--dump-resusage", default=None, help="compile, write the kernels' resource rows here, exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_box.json"))
    a = ap.parse_args()
    if a.dump_resusage:
        import resusage
        json.dump(resusage.rows(["soarm_sim.hip"]), open(a.dump_resusage, "w"), indent=1)
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ik_box needs a GPU (no CPU timing is meaningful)")
    from lerobot_mujoco_sim2real_amd import build, mjcf
    from lerobot_mujoco_sim2real_amd.control.TrajectoryGenerator import IK_DEFAULTS
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    from lerobot_mujoco_sim2real_amd.SOARM101.SOARM101_DataCollection import cartesian_targets
    build.build()
    n, F = a.n, a.frames
    cm = mjcf.compile_mjcf(mjcf.SCENE_XML)
    S = BatchSim(cm, n, 0)
    rng = np.random.default_rng(0)
    # generate()'s parameter 1.6 + 0.02 k, k = 0 .. 5 per second, from a per-env phase offset
    tpar = 1.6 + 0.02 * np.arange(F)[:, None] + rng.uniform(0.0, 2.0 * np.pi, n)[None, :]
    tgt = torch.as_tensor(cartesian_targets("Fig8", tpar).astype(np.float32), device=S.device).contiguous()  # [F, n, 3]
    q0 = torch.zeros((S.nq, n), dtype=torch.float32, device=S.device)
    q0[:] = torch.as_tensor(cm.qpos0().astype(np.float32), device=S.device).reshape(-1, 1)

    def run_box():
        q = q0.clone()
        return S.ik_bounded(tgt, q=q, ndof=5)

    def run_dls():
        q = q0.clone()
        oks, its = [], []
        for f in range(F):
            last = q.clone()
            q, ok, it = S.ik(tgt[f], q=q, ndof=5, **IK_DEFAULTS)
            okh = ok.cpu().numpy().astype(bool)  # (generate() reads ok back after every point)
            if not okh.all():
                bad = torch.as_tensor(~okh, device=S.device)
                q[:, bad] = last[:, bad]
            oks.append(okh)
            its.append(it.cpu().numpy())
        return q, np.array(oks), np.array(its)

    for _ in range(a.warmup):
        _, ok_a, it_a, _ = run_box()
        _, ok_b, it_b = run_dls()
    torch.cuda.synchronize()
    ms_a, ms_b = [], []
    for _ in range(a.repeats):
        q = q0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        S.ik_bounded(tgt, q=q, ndof=5)
        e1.record()
        e1.synchronize()
        ms_a.append(e0.elapsed_time(e1))
    for _ in range(max(3, a.repeats // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_dls()
        torch.cuda.synchronize()
        ms_b.append((time.perf_counter() - t0) * 1e3)
    ok_a, it_a = ok_a.cpu().numpy(), it_a.cpu().numpy()
    rec = {"n": n, "frames": F, "path": "Fig8, position targets, per-env phase offset",
           "ik_box_chained": dict(spread(ms_a), solves_per_s=n * F / (statistics.median(ms_a) * 1e-3),
                                  ok_fraction=float(ok_a.mean()), iterations_histogram=hist(it_a)),
           "ik_dls_per_frame": dict(spread(ms_b), solves_per_s=n * F / (statistics.median(ms_b) * 1e-3),
                                    ok_fraction=float(ok_b.mean()), iterations_histogram=hist(it_b)),
           "ratio_dls_loop_to_chained": statistics.median(ms_b) / statistics.median(ms_a),
           "resources": ik_box_resusage(a.resusage) if a.resusage else None,
           "library": build.library_info()}
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
