#!/usr/bin/env python3
"""Diagnostic: drive every Koopman entry point with the library named by SOARM_SIM_LIB and save all
outputs, so two builds can be compared bit for bit (a change that moves code or shares a helper
must leave them identical).  usage: ab_koopman.py TAG [OUTDIR]  ->  OUTDIR/abkoopman_TAG.npz (OUTDIR:
bench_out/ by default, which git ignores); `ab_koopman.py --compare A B [out.json]` compares two
dumps (no GPU).

Rows ref, odd, tiny, nz64 of tests/koopman_shapes_ref.py, both MPC kinds; n = 65 for the kernels of
16 envs per wave (two workgroups, a ragged last wave), n = 2 epw + 1 for those of one wave per env.
Inputs: koopman_box_ref.inputs (states, lifted reference windows, u_prev) and koopman_shapes_ref."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402

ROWS = ("ref", "odd", "tiny", "nz64")
N16, T_PRED = 65, 6


def compare(a, b, out=None):
    A, B = np.load(a), np.load(b)
    keys = sorted(set(A.files) | set(B.files))
    differ = [k for k in keys if k not in A.files or k not in B.files or A[k].dtype != B[k].dtype or
              A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    res = {"a": os.path.basename(a), "b": os.path.basename(b), "arrays": len(keys), "identical": len(keys) - len(differ),
           "differ": differ}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 1 if differ else 0


def main(tag, outdir=os.path.join(ROOT, "bench_out")):
    import torch

    import koopman_box_ref as R
    import koopman_shapes_ref as S
    import soarm_pkg  # noqa: F401
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer, KoopmanTrainer
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController

    out = {}
    dev = "cuda"
    t64 = lambda a: torch.as_tensor(np.array(a, np.float64, order="C"), device=dev)  # noqa: E731  (a copy: inputs are frozen)

    def keep(key, *tensors):
        for i, t in enumerate(tensors):
            out[f"{key}/{i}"] = t.detach().cpu().numpy().copy()

    for name in ROWS:
        row = S.ROWS[name]
        xd, ud, nz, H = S.dims(row)
        c = R.inputs(name)
        nw = 2 * S.EPW[name] + 1

        def batch(n):  # x [n, xd] f32, z0 [nz, n], window [H, nz, n], u_prev [ud, n]
            return (torch.as_tensor(c["x"][:n].copy(), device=dev), t64(c["z0"][:n].T), t64(c["ref"][:n].transpose(1, 2, 0)),
                    t64(c["up"][:n].T))

        # a rollout [T + 1, n, ud + xd] of [u | x] rows for predict and the trainers
        rng = S._rng(row, 31)
        roll = np.concatenate([rng.uniform(-0.5, 0.5, (T_PRED + 1, N16, ud)),
                               S.states(rng, (T_PRED + 1) * N16, xd).reshape(T_PRED + 1, N16, xd)], 2).astype(np.float32)
        roll = torch.as_tensor(roll, device=dev)
        for kind in S.KINDS:
            ctl = MPCController(S.make_net(name), S.Args(row, kind), horizon=H)
            x, z0, win, up = batch(N16)
            keep(f"{name}/{kind}/encode", ctl.encode(x))
            ff = ctl.feedforward(win)  # the window's H rows as a reference of H frames
            keep(f"{name}/{kind}/feedforward", ff)
            for key, xx, zz in (("x", x, None), ("z0", None, z0)):
                u = up.clone()
                keep(f"{name}/{kind}/mpc_step_{key}", ctl.step(xx, ff[0].contiguous(), u, z0=zz), u)
            ctl.set_box()
            u, plan = up.clone(), torch.zeros((H, ud, N16), dtype=torch.float64, device=dev)
            keep(f"{name}/{kind}/box_step_cold", *ctl.step_box(x, win, u, plan=plan), u, plan)
            u = up.clone()  # the same frame again from the plan: the warm start
            keep(f"{name}/{kind}/box_step_warm", *ctl.step_box(None, win, u, z0=z0, plan=plan, warm=True), u, plan)
            for rl in (0, 1):
                keep(f"{name}/{kind}/predict_{rl}", *ctl.predict(roll, relift=bool(rl), npos=min(3, xd)))
            del ctl
            ctl = MPCController(S.make_net(name, "DBKN"), S.Args(row, kind, "DBKN"), horizon=H)
            x, z0, win, up = batch(nw)
            u = up.clone()
            keep(f"{name}/{kind}/bilinear_step", ctl.step_bilinear(x, win, u), u)
            u, plan = up.clone(), torch.zeros((H, ud, nw), dtype=torch.float64, device=dev)
            keep(f"{name}/{kind}/bilinear_box_step", *ctl.step_box_bilinear(None, win, u, z0=z0, plan=plan), u, plan)
            for rl in (0, 1):
                keep(f"{name}/{kind}/predict_dbkn_{rl}", *ctl.predict(roll, relift=bool(rl), npos=min(3, xd)))
            del ctl
        for model, cls in (("DKUC", KoopmanTrainer), ("DBKN", BilinearKoopmanTrainer)):
            tr = cls(S.make_net(name, model), N16, pre_length=5, npos=min(3, xd - 1))
            for step in range(2):
                keep(f"{name}/train_{model}/losses_{step}", tr.step(roll, None, step, 1e-3))
            torch.cuda.synchronize()
            out[f"{name}/train_{model}/params"] = tr.get_params()
            del tr
    torch.cuda.synchronize()
    os.makedirs(outdir, exist_ok=True)
    np.savez_compressed(os.path.join(outdir, f"abkoopman_{tag}.npz"), **out)
    print(tag, "done:", len(out), "arrays", flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    sys.exit(main(*sys.argv[1:3]))
