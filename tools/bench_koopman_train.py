#!/usr/bin/env python3
"""Time the fused Koopman training step (sim_koopman_train_step) against the eager torch step it
replaces, and run a short train() on a rollout of the project's own generator.

    python tools/bench_koopman_train.py [--model DKUC|DBKN] [--loss mse|nmse|weighted_mse] [--batches 128,4096]
                                        [--steps 200] [--windows 7] [--epochs 20] [--out profiles/koopman_train.json]

Needs a GPU.  Per batch size, on a random [T+1, N, 13] fp32 rollout (T = 20):

* fused: `KoopmanTrainer.step` (two launches, no host synchronisation between steps); with
  `--model DBKN` `BilinearKoopmanTrainer.step` on a `KoopmanBlinear` whose `H` is 0.05 randn (a zero `H`
  would time the bilinear products on zeros and let the agreement check pass without them), and the
  default --out is profiles/koopman_train_dbkn.json; with `--loss nmse` / `weighted_mse` the trainer's loss_name
  (nmse: four launches), the eager step's BaseLoss written out the same way, and the default --out
  profiles/koopman_train_<loss>.json (`_dbkn_<loss>` for DBKN);
* eager: this project's `Koopmanlinear().double()` (`KoopmanBlinear` for DBKN) on the same GPU, the section-2 loss of
  include/koopman_mpc.h written with torch ops (six encoder calls, P model steps, the MSE
  reductions), `loss.backward()` and `torch.optim.Adam.step()` -- the parent has no HIP path for
  this step, so this is what a user would run;
* both: warm-up first, then `--windows` windows of `--steps` steps each, a host clock around a window
  that ends in a device synchronise, the two alternating; the median window is reported, with the
  windows' min and max;
* the fused and the eager parameters after the same 3 steps from the same start must agree (1e-9
  relative to each block's max) before a time is recorded.

The sanity line: `train()` for --epochs epochs on 512 trajectories x 50 steps from
SOARM101DataGenerator.rollout_device, evaluated (MPCController.evaluate) on 128 others, before and
after.  One JSON object goes to --out.
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

LAYERS = [8, 64, 64, 64, 64, 24]
XD, UD, P, GAMMA, T = 8, 5, 5, 0.8, 20


class _Args:
    x_dim, u_dim, MPC_type, layers, model = XD, UD, "delta_mpc", LAYERS, "DKUC"


def make_net(seed=0, model="DKUC", hscale=0.05):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear, Koopmanlinear
    torch.manual_seed(seed)
    if model == "DKUC":
        return Koopmanlinear(XD, UD, LAYERS).double()
    net = KoopmanBlinear(XD, UD, LAYERS).double()
    with torch.no_grad():  # (H is zero-initialised: hscale = 0 keeps the reference's start)
        net.H.weight.copy_(hscale * torch.randn(net.H.weight.shape, generator=torch.Generator().manual_seed(seed + 100),
                                                dtype=torch.float64))
    return net


def base_loss(loss, preds, labels):
    """the reference's BaseLoss (models/losses.py:35-52), written out"""
    import torch
    import torch.nn.functional as F
    if loss == "nmse":
        return F.mse_loss(preds, labels) / torch.square(labels).mean()
    if loss == "weighted_mse":
        return (F.mse_loss(preds[:, :3], labels[:, :3]) + 9 * F.mse_loss(preds[:, 3:], labels[:, 3:])) / 10
    return torch.mean((preds - labels) ** 2)


def eager_loss(net, rows, idx, t0, loss="mse"):
    w = rows[t0:t0 + P + 1].index_select(1, idx).double()
    x, u = w[:, :, UD:], w[:, :, :UD]
    beta = [GAMMA ** i for i in range(P)]
    z = net.x_encoder(x[0])
    koop = pred = 0.0
    for i in range(P):
        z = net.koopman_operation(z, u[i])
        koop = koop + beta[i] * base_loss(loss, z, net.x_encoder(x[i + 1]))
        pred = pred + beta[i] * base_loss(loss, net.x_decoder(z), x[i + 1])
    return (koop + pred) / sum(beta)


def bench_batch(n, steps, windows, model="DKUC", loss="mse"):
    import numpy as np
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer, KoopmanTrainer, params_from_net
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    rows = (torch.rand((T + 1, n, XD + UD), generator=g) - 0.5).to(dev)
    idx = torch.randperm(n, generator=g).to(dev)
    idx32 = idx.to(torch.int32)
    t0s = [int(v) for v in torch.randint(0, T - P, (steps,), generator=g)]
    net = make_net(model=model).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    tr = (KoopmanTrainer if model == "DKUC" else BilinearKoopmanTrainer)(make_net(model=model), n, pre_length=P, gamma=GAMMA,
                                                                          loss_name=loss)
    losses = torch.empty(6, dtype=torch.float64, device=dev)

    def eager(k):
        for t0 in t0s[:k]:
            opt.zero_grad(set_to_none=True)
            eager_loss(net, rows, idx, t0, loss).backward()
            opt.step()
        torch.cuda.synchronize()

    def fused(k):
        for t0 in t0s[:k]:
            tr.step(rows, idx32, t0, 1e-3, losses=losses)
        torch.cuda.synchronize()

    eager(3), fused(3)  # the same three steps from the same start: the results must agree
    pe, pf = params_from_net(net.cpu()), tr.get_params()
    net.to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    agree = float(np.abs(pe - pf).max() / np.abs(pe).max())
    if not agree < 1e-9:
        raise SystemExit(f"batch {n}: fused and eager parameters differ by {agree:.2e} after 3 steps")
    eager(10), fused(10)  # warm-up
    te, tf = [], []
    for _ in range(windows):
        a = time.perf_counter()
        fused(steps)
        b = time.perf_counter()
        eager(steps)
        c = time.perf_counter()
        tf.append((b - a) / steps * 1e3), te.append((c - b) / steps * 1e3)
    rec = dict(batch=n, steps_per_window=steps, windows=windows, agree_after_3_steps=agree,
               fused_ms_per_step=statistics.median(tf), fused_ms_min=min(tf), fused_ms_max=max(tf),
               eager_ms_per_step=statistics.median(te), eager_ms_min=min(te), eager_ms_max=max(te))
    rec["eager_over_fused"] = rec["eager_ms_per_step"] / rec["fused_ms_per_step"]
    return rec


def sanity_train(epochs, model="DKUC", loss="mse"):
    import torch
    from lerobot_mujoco_sim2real_amd import mjcf
    from lerobot_mujoco_sim2real_amd.args import Args
    from lerobot_mujoco_sim2real_amd.control.koopman_train import train
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    from lerobot_mujoco_sim2real_amd.SOARM101.SOARM101_DataCollection import SOARM101DataGenerator
    gen = SOARM101DataGenerator(Args([]), model=mjcf.compile_mjcf(mjcf.SCENE_XML, disable_contact=True))
    data = gen.rollout_device(n=512, steps=50, input_type="random", seed=1)
    held = gen.rollout_device(n=128, steps=50, input_type="random", seed=2)
    net = make_net(7, model, hscale=0.0)
    before = MPCController(net, _Args).evaluate(held)
    torch.cuda.synchronize()
    a = time.perf_counter()
    hist = train(net, data, args=_Args, epochs=epochs, batch_size=128, lr=1e-3, seed=0, eval_rollout=held,
                 eval_interval=max(1, epochs // 4), loss_name=loss)
    torch.cuda.synchronize()
    wall = time.perf_counter() - a
    after = MPCController(net, _Args).evaluate(held)
    keys = ("avg_error", "dis_error", "angle_error")
    return dict(trajectories=512, steps=50, epochs=epochs, batch_size=128, wall_s=wall,
                first_epoch_loss=hist["train_loss"][0][0], last_epoch_loss=hist["train_loss"][-1][0],
                best_epoch=hist["best_epoch"], before={k: before[k] for k in keys}, after={k: after[k] for k in keys})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,4096")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--model", choices=("DKUC", "DBKN"), default="DKUC")
    ap.add_argument("--loss", choices=("mse", "nmse", "weighted_mse"), default="mse")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        name = "koopman_train" + ("" if a.model == "DKUC" else "_dbkn") + ("" if a.loss == "mse" else "_" + a.loss)
        a.out = os.path.join(ROOT, "profiles", name + ".json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_koopman_train needs a GPU")
    out = dict(device=torch.cuda.get_device_name(0), layers=LAYERS, pre_length=P,
               step=[bench_batch(int(b), a.steps, a.windows, a.model, a.loss) for b in a.batches.split(",")])
    if a.model != "DKUC":
        out["model"] = a.model
    if a.loss != "mse":
        out["loss"] = a.loss
    for r in out["step"]:
        print(f"batch {r['batch']}: fused {r['fused_ms_per_step']:.4f} ms/step ({r['fused_ms_min']:.4f}..{r['fused_ms_max']:.4f}), "
              f"eager {r['eager_ms_per_step']:.4f} ms/step ({r['eager_ms_min']:.4f}..{r['eager_ms_max']:.4f}), "
              f"ratio {r['eager_over_fused']:.1f}x, agree {r['agree_after_3_steps']:.1e}", flush=True)
    if a.epochs > 0:
        out["train"] = s = sanity_train(a.epochs, a.model, a.loss)
        print(f"train(): {s['epochs']} epochs in {s['wall_s']:.2f} s, loss {s['first_epoch_loss']:.4e} -> {s['last_epoch_loss']:.4e}, "
              f"evaluate avg_error {s['before']['avg_error']:.4f} -> {s['after']['avg_error']:.4f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(a.out, ROOT))


if __name__ == "__main__":
    main()
