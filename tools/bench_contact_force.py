#!/usr/bin/env python3
"""Time one contact-force readout (sim_contact_forces) beside the same batch's env-step.

    python tools/bench_contact_force.py [--envs 4096] [--warmup 20] [--steps 100] [--solver pgs|newton]
                                        [--out profiles/contact_force_pgs.json]

Needs a GPU.  The batch is bench.py's `contact` workload (the pick scene, chirp actions, the same
seed and initial poses): it is stepped `--warmup` env-steps, the env-step is timed over `--steps`
steps (host clock around a loop that ends in a synchronise, as bench.py times it), and at the states
reached one readout is timed with device events around every launch -- warm-up first, the median of
30 launches.  The yardstick is bench.py --config contact's ms_per_step; the record holds both times
and their ratio, and the mean contacts per env at the timed states.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
import soarm_pkg  # noqa: F401,E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--solver", default="pgs", choices=["pgs", "newton"])
    p.add_argument("--launches", type=int, default=30)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import numpy as np
    import torch
    from lerobot_mujoco_sim2real_amd import build, workloads as W
    from lerobot_mujoco_sim2real_amd.sim import BatchSim

    build.build()
    n = args.envs
    ids = np.arange(n)
    cm = W.model("contact", solver=args.solver)
    sim = BatchSim(cm, n, 0)
    q0 = W.initial_qpos(cm, ids, args.seed)
    sim.reset(init_qpos=q0[:, :5], extra_qpos=q0, seed=args.seed)
    tab = {k: (torch.as_tensor(v, dtype=torch.float32, device=sim.device) if isinstance(v, np.ndarray) else v)
           for k, v in W.chirp_tables(ids, args.seed).items()}
    acts = torch.stack([W.chirp_action(tab, float(t), lib=torch) for t in range(args.warmup + args.steps)])
    act = sim.action_buffer()
    for t in range(args.warmup):
        act.copy_(acts[t])
        sim.step(act)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.warmup, args.warmup + args.steps):
        act.copy_(acts[t])
        sim.step(act)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / args.steps * 1e3

    for _ in range(5):
        con, frc, nc = sim.contact_forces()
    torch.cuda.synchronize()
    ms = []
    for _ in range(max(args.launches, 20)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        con, frc, nc = sim.contact_forces()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    read_ms = statistics.median(ms)
    rec = {"envs": n, "solver": args.solver, "warmup": args.warmup, "steps": args.steps,
           "env_step_ms": step_ms, "contact_forces_ms": read_ms, "readout_over_env_step": read_ms / step_ms,
           "contacts_per_env": float(nc.float().mean().item()), "finite": bool(torch.isfinite(frc).all().item()),
           "largest_normal_force_N": float(frc[:, :, 0].max().item())}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
