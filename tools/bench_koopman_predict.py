#!/usr/bin/env python3
"""Time the fused open-loop prediction (sim_koopman_predict) against the torch loop it replaces.

    python tools/bench_koopman_predict.py [--n 4096] [--steps 199] [--launches 30]
                                          [--resusage FILE.json] [--out profiles/koopman_predict.json]

Needs a GPU.  Cases: DKUC relift=1 (what evaluate() runs), DKUC relift=0, DBKN relift=1, at N
trajectories x T steps of a random [T+1, N, 13] fp32 rollout.  Per case:

* the fused launch with 1, 2 and 4 waves per workgroup (SOARM_KPREDICT_WAVES, read by
  sim_koopman_set_model) and with the library's default (4): device events around every launch,
  warm-up first, the median of `--launches` (>= 20) launches;
* `control.koopman.open_loop_prediction` + `prediction_errors` on the same GPU in float64 -- how the
  metric is computed without the kernel (T rounds of small float64 torch ops): host clock around a
  run that ends in a synchronise, median of 5;
* the two must agree (1e-9) before a time is recorded.

One JSON record per case goes to --out: ms, trajectory-steps/s, the ratio to the torch loop, waves
per workgroup, the kernel's VGPR / AGPR / spill counts (tools/resusage.py; --resusage takes a file
written earlier by `--dump-resusage`, so the compile need not run on the GPU box), and the achieved
share of the f64 MFMA rate.  The share is the algorithm's flops (encoder and model products at their
true sizes, 2 flops per multiply-add) over 78.6 TFLOP/s, the MI355X's published FP64 matrix peak;
`mfma_issue_share` counts the padded 16x16x4 MFMAs the kernel actually issues.
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
sys.path.insert(0, HERE)
import soarm_pkg  # noqa: F401,E402

F64_MFMA_PEAK = 78.6e12  # flop/s, MI355X FP64 matrix (published peak)
LAYERS = [8, 64, 64, 64, 64, 24]
XD, UD = 8, 5


class _Args:
    x_dim, u_dim, MPC_type, layers = XD, UD, "delta_mpc", LAYERS

    def __init__(self, model):
        self.model = model


def make_net(model):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear, Koopmanlinear
    torch.manual_seed(0)
    if model == "DKUC":
        return Koopmanlinear(XD, UD, LAYERS).double()
    net = KoopmanBlinear(XD, UD, LAYERS).double()
    with torch.no_grad():
        net.H.weight.normal_(0.0, 0.02)
    return net


def flops_per_traj_step(model, relift):
    """(algorithmic flops, flops of the MFMAs issued) per trajectory and step."""
    nz, ntl = XD + LAYERS[-1], (LAYERS[-1] + 15) // 16
    enc = sum(2 * a * b for a, b in zip(LAYERS[:-1], LAYERS[1:]))
    rows = XD if relift else nz
    alg = 2 * rows * (nz + UD) + (2 * rows * nz * UD + nz * UD if model == "DBKN" else 0) + (enc if relift else 0)
    mf = 2 * 16 * 16 * 4 / 16  # one 16x16x4 MFMA serves 16 trajectories
    tiles = 1 if relift else 1 + ntl
    n_mfma = tiles * (2 + 4 * ntl + 2) + (tiles * UD * (2 + 4 * ntl) if model == "DBKN" else 0)
    if relift:
        n_mfma += 4 * 2 + (len(LAYERS) - 3) * 4 * 16 + ntl * 16
    return alg, n_mfma * mf


def predict_resusage(path=None):
    """{(relift): {VGPRs, AGPRs, spill, scratch}} of k_predict at the reference shape (NTL = 2)."""
    if path:
        rows = json.load(open(path))
    else:
        import resusage
        rows = resusage.rows(["koopman_predict.hip"])
    out = {}
    for r in rows:
        for rl in (0, 1):
            if f"k_predictILi2ELb{rl}EE" in r["name"]:
                out[rl] = {"vgpr": int(r["VGPRs"]), "agpr": int(r["AGPRs"]), "vgpr_spill": int(r["VGPRs Spill"]),
                           "scratch_bytes_per_lane": int(r["ScratchSize [bytes/lane]"])}
    return out


def time_fused(ctl, rollout, relift, launches, warmup=5):
    import torch
    for _ in range(warmup):
        ctl.predict(rollout, relift=relift)
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctl.predict(rollout, relift=relift)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def time_torch(net, x, u, relift, reps=5):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman import open_loop_prediction, prediction_errors
    pred = open_loop_prediction(net, x, u, relift=relift)  # warm-up
    prediction_errors(pred, x)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pred = open_loop_prediction(net, x, u, relift=relift)
        m = prediction_errors(pred, x)  # (float(): ends in a synchronise)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), pred, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=199)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--resusage", default=None, help="JSON written by --dump-resusage")
    ap.add_argument("--dump-resusage", default=None, help="compile, write the kernels' resource rows here, exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "koopman_predict.json"))
    a = ap.parse_args()
    if a.dump_resusage:
        import resusage
        json.dump(resusage.rows(["koopman_predict.hip"]), open(a.dump_resusage, "w"), indent=1)
        return
    if a.launches < 20:
        ap.error("--launches must be >= 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_koopman_predict needs a GPU (no CPU timing is meaningful)")
    from lerobot_mujoco_sim2real_amd import build
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    build.build()
    res = predict_resusage(a.resusage)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    n, T = a.n, a.steps
    rollout = torch.cat([torch.rand((T + 1, n, UD), generator=g) - 0.5,
                         torch.rand((T + 1, n, 3), generator=g) * 0.3 + 0.1,
                         torch.rand((T + 1, n, 5), generator=g) * 2 - 1], -1).float().to(dev).contiguous()
    r = rollout.transpose(0, 1)
    x, u = r[:, :, UD:], r[:, :, :UD]
    records = []
    for model, relift in (("DKUC", 1), ("DKUC", 0), ("DBKN", 1)):
        net = make_net(model)
        net_dev = make_net(model).to(dev)
        torch_ms, tpred, tm = time_torch(net_dev, x, u, bool(relift))
        by_waves = {}
        for w in (1, 2, 4, "auto"):
            if w == "auto":
                os.environ.pop("SOARM_KPREDICT_WAVES", None)
            else:
                os.environ["SOARM_KPREDICT_WAVES"] = str(w)
            ctl = MPCController(net, _Args(model))
            pred, err = ctl.predict(rollout, relift=bool(relift))
            dmax = float((pred.transpose(0, 1) - tpred).abs().max())
            ev = ctl.evaluate(rollout, relift=bool(relift))
            assert dmax < 1e-9 and abs(ev["avg_error"] - tm["avg_error"]) < 1e-9 * max(1.0, tm["avg_error"]), (model, relift, w, dmax)
            med, lo, hi = time_fused(ctl, rollout, bool(relift), a.launches)
            by_waves[str(w)] = {"ms": med, "ms_min": lo, "ms_max": hi}
            del ctl
        os.environ.pop("SOARM_KPREDICT_WAVES", None)
        auto_w = 4  # the library's default (sim_koopman_set_model)
        ms = by_waves["auto"]["ms"]
        alg, issued = flops_per_traj_step(model, relift)
        rec = {"case": f"{model} relift={relift}", "model": model, "relift": relift, "n": n, "steps": T,
               "ms": ms, "traj_steps_per_s": n * T / (ms * 1e-3), "torch_loop_ms": torch_ms,
               "ratio_to_torch_loop": torch_ms / ms, "waves_per_workgroup": auto_w, "by_waves_per_workgroup": by_waves,
               "launches": a.launches, "max_abs_diff_to_torch_loop": dmax,
               "f64_mfma_share": n * T * alg / (ms * 1e-3) / F64_MFMA_PEAK,
               "mfma_issue_share": n * T * issued / (ms * 1e-3) / F64_MFMA_PEAK,
               "resources": res.get(relift), "library": build.library_info()}
        print(json.dumps(rec))
        records.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
