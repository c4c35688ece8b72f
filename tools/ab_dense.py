#!/usr/bin/env python3
"""Diagnostic: drive the two dense constraint solves (the CPU backend's step and readout, the
device's contact-force readout kernel) with the library SOARM_SIM_LIB names, on states that reach
every row kind, and save every result, so two builds can be compared bit for bit.

    SOARM_SIM_LIB=tools/_ab/lib_X.so python tools/ab_dense.py DEVICE OUT.npz    (DEVICE: -1 or 0)
    python tools/ab_dense.py --compare A.npz B.npz

Cases, for the PGS and the Newton model each: the pick scene on the overflow fixture's `shallow`,
`deep` (up to and past 16 contacts) and `fill` sets and on the joint-limit pool (active limit rows,
lower and upper); the arm-only scene on contact_forces_ref.arm_states and on the pool's arm
coordinates; each of them plain, with per-env friction / mass / damping scales
(joint_limits_ref.dr_params) and with a non-zero qfrc_applied; and 64 envs of the bench's `contact`
workload after 40 env-steps.  Per case one contact_forces() at the loaded state, then one env-step
(frame_skip 4); saved: the readout's contacts, force and ncon, and qpos, qvel, qacc_warmstart,
status, ncon, obs after the step.  --compare asserts np.array_equal on the arrays' bytes, array by
array, and prints the count.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

FIELDS = ("qpos", "qvel", "qacc_warmstart", "status", "ncon", "obs")
FRAME_SKIP = 4


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
    for k in a.files:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        same = np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
        assert same, (k, int((x != y).sum()), float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))))
    print(f"{len(a.files)} arrays bit-identical: {pa} {pb}")


def load_state(S, st):
    import torch
    for name, key in (("qpos", "qpos"), ("qvel", "qvel"), ("qacc_warmstart", "warm"), ("ctrl", "ctrl")):
        getattr(S, name).copy_(torch.as_tensor(st[key].T, dtype=torch.float32))
    S.status.zero_()
    S.ncon.zero_()


def record(out, tag, S, readout):
    import torch
    if not S.cpu:
        torch.cuda.synchronize()
    for k, v in zip(("con", "force", "nc"), readout):
        out[f"{tag}/{k}"] = v.detach().cpu().numpy()
    for k in FIELDS:
        out[f"{tag}/{k}"] = getattr(S, k).detach().cpu().numpy()


def main():
    if sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    device, path = int(sys.argv[1]), sys.argv[2]
    import torch

    import soarm_pkg  # noqa: F401
    import contact_forces_ref as F
    import contact_overflow_ref as R
    import joint_limits_ref as J
    from lerobot_mujoco_sim2real_amd import workloads as W
    from lerobot_mujoco_sim2real_amd.sim import BatchSim

    out = {}
    for solver in ("PGS", "Newton"):
        pick, arm = R.model(solver), F.arm_model(solver)
        fx, pool = R.fixture(), J.states("pool")
        sets = [("pick_shallow", pick, fx["shallow"]), ("pick_deep", pick, fx["deep"]), ("pick_fill", pick, fx["fill"]),
                ("pick_pool", pick, J.for_model(pick, pool)), ("arm_states", arm, F.arm_states(solver)),
                ("arm_pool", arm, J.for_model(arm, pool))]
        for name, cm, st in sets:
            n = len(st["qpos"])
            for variant in ("plain", "dr", "applied"):
                S = BatchSim(cm, n, device)
                load_state(S, st)
                if variant == "dr":
                    S.set_params(**J.dr_params(n)[0])
                if variant == "applied":  # a few percent of the servo's torque on the arm, of the cube's weight on it
                    push = np.random.default_rng(5).uniform(-1, 1, (n, cm.desc.nv))
                    push[:, :6] *= 0.2
                    push[:, 6:] *= 0.02
                    S.enable_qfrc_applied().copy_(torch.as_tensor(push.T, dtype=torch.float32))
                readout = S.contact_forces()
                S.step(st["ctrl"][:, :S.nact].astype(np.float32), frame_skip=FRAME_SKIP)
                record(out, f"{solver}/{name}/{variant}", S, readout)
                S.close()
        cm = W.model("contact", solver=solver)
        n, ids = 64, np.arange(64)
        S = BatchSim(cm, n, device)
        q0 = W.initial_qpos(cm, ids, 0)
        S.reset(init_qpos=q0[:, :5], extra_qpos=q0, seed=0)
        tab = W.chirp_tables(ids, 0)
        for t in range(40):
            S.step(W.chirp_action(tab, float(t)).astype(np.float32))
        record(out, f"{solver}/bench_contact", S, S.contact_forces())
        S.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays -> {path}", flush=True)


if __name__ == "__main__":
    main()
