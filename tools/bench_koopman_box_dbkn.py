#!/usr/bin/env python3
"""Time the constrained DBKN control step (sim_koopman_bilinear_box_step) beside the unconstrained one
it extends (sim_koopman_bilinear_step), and compare the untouched entry points with a parent build.

    python tools/bench_koopman_box_dbkn.py [--n 4096] [--launches 30] [--frames 12]
                                           [--parent-lib PATH/libsoarm_sim.so] [--out profiles/koopman_box_dbkn.json]

Needs a GPU.  Reference shape (encoder [8, 64, 64, 64, 64, 24], u_dim 5, H 10: N = 50), 'delta_mpc', a
DBKN net whose bilinear layer is drawn from N(0, 0.02), n envs.  Inputs:

* `interior`: every env's unconstrained minimiser lies in the box (the window is the model's free
  response from the env's state plus small noise, u_prev small).  The kernel does not factorise, so
  these envs are iterated to tol like every other;
* `tracking`: the lifted states, windows and u_prev of a KoopmanMPCTracking(constrained=True) run of
  the prepared DBKN controller on the arm scene, the saturating figure-eight references of
  tools/bench_koopman_box.py, recorded at its last frame; also timed with max_iter = 1 (the build of
  P_e and g_e plus one sweep), which splits the step's time into the build and the sweeps.

Beside each: sim_koopman_bilinear_step on the same z0, window and u_prev, from the library given with
--parent-lib (a build of the parent commit, loaded beside this tree's), else from this tree's.  Device
events around every launch, 10 warm-up launches, the median of --launches (>= 20); u_prev is restored
before every launch.  Per input: ms per step, the ratio, mean and max iters, ok share and the share of
envs with an active bound.

With --parent-lib the outputs of the untouched entry points -- sim_koopman_mpc_step,
sim_koopman_bilinear_step, sim_koopman_box_step; rows ref, odd and nz64 of tests/koopman_shapes_ref.py
on the inputs of tests/koopman_box_ref.py; both kinds -- are compared bitwise between the two libraries
and the count of equal arrays is recorded.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)
import soarm_pkg  # noqa: F401,E402

LAYERS = [8, 64, 64, 64, 64, 24]
XD, UD, H = 8, 5, 10


class _Args:
    x_dim, u_dim, MPC_type, layers, model = XD, UD, "delta_mpc", LAYERS, "DBKN"


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class RawController:
    """The entry points that exist in the parent commit, bound by hand on any build of the library, on
    the weights, gains and model matrices of an MPCController `ctl`."""

    def __init__(self, ctl, path, layers, horizon):
        from lerobot_mujoco_sim2real_amd import abi
        self.ctl, self.lib = ctl, C.CDLL(path)
        vp, ip, dbl = C.c_void_p, C.c_int, C.c_double
        L = self.lib
        L.sim_koopman_create.argtypes = [C.POINTER(abi.KoopmanDesc), vp, vp, ip, C.POINTER(vp)]
        L.sim_koopman_free.argtypes = [vp]
        L.sim_koopman_free.restype = None
        L.sim_koopman_mpc_step.argtypes = [vp, ip, vp, vp, vp, vp, vp, vp]
        L.sim_koopman_set_bilinear.argtypes = [vp, vp, vp, vp, ip, dbl, dbl]
        L.sim_koopman_bilinear_step.argtypes = [vp, ip, vp, vp, vp, vp, vp]
        L.sim_koopman_set_box.argtypes = [vp, vp, vp, ip, dbl, dbl, vp]
        L.sim_koopman_box_step.argtypes = [vp, ip, vp, vp, vp, vp, vp, ip, vp, vp, vp, vp]
        d = abi.KoopmanDesc()
        d.x_dim, d.u_dim, d.nlayer, d.horizon, d.u_clip = layers[0], ctl.u_dim, len(layers) - 1, horizon, ctl.u_clip
        for i, w in enumerate(layers):
            d.width[i] = w
        self.h = C.c_void_p()
        self._ok(L.sim_koopman_create(C.byref(d), _vp(ctl._w), _vp(ctl._g), ctl.device.index, C.byref(self.h)), "create")
        delta = int(ctl.MPC_type == "delta_mpc")
        if ctl.bilinear:
            self._ok(L.sim_koopman_set_bilinear(self.h, _vp(ctl._Ah), _vp(ctl._Bh), _vp(ctl._Hh), delta, 50.0, 0.5), "set_bilinear")
        else:
            self._ok(L.sim_koopman_set_box(self.h, _vp(ctl._Ah), _vp(ctl._Bh), delta, 50.0, 0.5, None), "set_box")

    @staticmethod
    def _ok(rc, what):
        if rc:
            raise RuntimeError(f"{what} returned {rc}")

    def bilinear_step(self, z0, win, up, act):
        self._ok(self.lib.sim_koopman_bilinear_step(self.h, up.shape[1], _p(z0), _p(win), _p(up), _p(act), self.ctl._stream()),
                 "bilinear_step")

    def mpc_step(self, x, up, act):
        self._ok(self.lib.sim_koopman_mpc_step(self.h, up.shape[1], _p(x), None, None, _p(up), _p(act), self.ctl._stream()),
                 "mpc_step")

    def box_step(self, x, win, up, plan, act, ok, iters):
        self._ok(self.lib.sim_koopman_box_step(self.h, up.shape[1], _p(x), None, _p(win), _p(up), _p(plan), 0, _p(act), _p(ok),
                                               _p(iters), self.ctl._stream()), "box_step")

    def close(self):
        self.lib.sim_koopman_free(self.h)


def median_ms(fn, restore, launches, warmup=10):
    import torch
    for _ in range(warmup):
        restore()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def measure(ctl, parent, tag, z0, win, up0, launches):
    """One input: the constrained step, then the parent's bilinear_step on the same z0 and window."""
    import torch
    n = up0.shape[1]
    up = up0.clone()
    plan = torch.zeros((H, UD, n), dtype=torch.float64, device=z0.device)
    act = torch.empty((n, UD), dtype=torch.float32, device=z0.device)
    out = {}

    def restore():
        up.copy_(up0)

    def box():
        out["r"] = ctl.step_box_bilinear(None, win, up, act, z0=z0, plan=plan)
    ms = median_ms(box, restore, launches)
    _, ok, iters = out["r"]
    active = float(((plan.abs() >= ctl._box_bilinear[0]).any(0).any(0)).double().mean())
    base = median_ms(lambda: parent.bilinear_step(z0, win, up, act), restore, launches)
    return dict(input=tag, n=n, max_iter=ctl._box_bilinear[2], box_ms=ms[0], box_ms_min=ms[1], box_ms_max=ms[2],
                bilinear_step_ms=base[0], ratio_to_bilinear_step=ms[0] / base[0], iters_mean=float(iters.double().mean()),
                iters_max=int(iters.max()), ok_share=float(ok.double().mean()), active_share=active, launches=launches)


def compare_untouched(parent_path):
    """Outputs of mpc_step, bilinear_step and box_step from this tree's library and the parent's, bitwise."""
    import numpy as np
    import torch
    import koopman_box_ref as R
    import koopman_shapes_ref as S
    from lerobot_mujoco_sim2real_amd import abi
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    equal, total, detail = 0, 0, []
    for name in ("ref", "odd", "nz64"):
        row = S.ROWS[name]
        inp = R.inputs(name)
        n = inp["up"].shape[0]
        for kind in S.KINDS:
            for model in ("DKUC", "DBKN"):
                ctl = MPCController(S.make_net(name, model), S.Args(row, kind, model), horizon=row.H)
                dev = ctl.device
                t = lambda a: torch.as_tensor(np.array(a, order="C"), device=dev)  # noqa: E731
                outs = []
                for path in (abi.LIB_PATH, parent_path):
                    raw = RawController(ctl, path, list(row.layers), row.H)
                    x, z0, win = t(inp["x"]), t(inp["z0"].T), t(inp["ref"].transpose(1, 2, 0))
                    act = torch.zeros((n, row.u_dim), dtype=torch.float32, device=dev)
                    got = {}
                    if model == "DBKN":
                        up = t(inp["up"].T)
                        raw.bilinear_step(z0, win, up, act)
                        got.update(bilinear_step_u_prev=up.clone(), bilinear_step_action=act.clone())
                    else:
                        up = t(inp["up"].T)
                        raw.mpc_step(x, up, act)
                        got.update(mpc_step_u_prev=up.clone(), mpc_step_action=act.clone())
                        up = t(inp["up"].T)
                        plan = torch.zeros((row.H, row.u_dim, n), dtype=torch.float64, device=dev)
                        ok = torch.zeros((n,), dtype=torch.int32, device=dev)
                        iters = torch.zeros((n,), dtype=torch.int32, device=dev)
                        raw.box_step(x, win, up, plan, act, ok, iters)
                        got.update(box_step_u_prev=up.clone(), box_step_action=act.clone(), box_step_plan=plan.clone(),
                                   box_step_iters=iters.clone())
                    torch.cuda.synchronize()
                    raw.close()
                    outs.append(got)
                for key in outs[0]:
                    same = bool(torch.equal(outs[0][key], outs[1][key]))
                    equal, total = equal + same, total + 1
                    if not same:
                        detail.append(f"{name} {kind} {key}")
    return dict(arrays=total, equal=equal, differing=detail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "koopman_box_dbkn.json"))
    a = ap.parse_args()
    if a.launches < 20:
        ap.error("--launches must be >= 20")
    import numpy as np
    import torch
    from lerobot_mujoco_sim2real_amd import abi, build, mjcf
    from lerobot_mujoco_sim2real_amd.Koopman_MPC import KoopmanMPCTracking
    from lerobot_mujoco_sim2real_amd.control.MPC_Controler import MPCController
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear
    build.build()
    torch.manual_seed(0)
    net = KoopmanBlinear(XD, UD, LAYERS, False).double()
    with torch.no_grad():
        net.H.weight.normal_(0.0, 0.02)
    ctl = MPCController(net, _Args())
    ctl.set_box_bilinear()
    parent = RawController(ctl, a.parent_lib or abi.LIB_PATH, LAYERS, H)
    n, dev = a.n, ctl.device
    rng = np.random.default_rng(5)
    recs = []
    # (a) interior: the window is the free response of the env's own lifted state plus small noise
    x = torch.as_tensor(np.concatenate([rng.uniform([0.1, -0.2, 0.0], [0.45, 0.2, 0.35], (n, 3)),
                                        rng.uniform(-1.0, 1.0, (n, 5))], 1), dtype=torch.float32, device=dev)
    z0 = ctl.encode(x)
    A = torch.as_tensor(ctl.Ad, device=dev)
    rows, z = [], z0
    for _ in range(H):
        z = A @ z
        rows.append(z + 1e-3 * torch.randn_like(z))
    win = torch.stack(rows).contiguous()
    up0 = torch.as_tensor(rng.uniform(-0.05, 0.05, (UD, n)), device=dev)
    r = measure(ctl, parent, "interior", z0, win, up0, a.launches)
    assert r["active_share"] == 0.0 and r["ok_share"] == 1.0, r
    recs.append(r)
    # (b) the saturating figure-eight tracking run of tools/bench_koopman_box.py: its last frame's inputs
    T = a.frames + H
    t = np.linspace(0, 2 * np.pi, T)
    phase = rng.uniform(0, 2 * np.pi, n)
    amp = rng.choice([0.5, 2.0, 4.0, 8.0], n)
    cart = np.stack([0.3 + 0.05 * amp * np.sin(2 * (t[:, None] + phase)), 0.1 * amp * np.cos(t[:, None] + phase),
                     0.15 + 0.05 * amp * np.sin(t[:, None] + phase)], -1)
    jq = rng.uniform(-0.3, 0.3, (1, n, 5)) + 0.1 * amp[None, :, None] * np.sin(t[:, None, None] + phase[None, :, None])
    run = KoopmanMPCTracking(ctl, mjcf.compile_mjcf(mjcf.SCENE_XML), cart, jq, constrained=True)
    run.runBefore()
    it_max, it_sum = 0, 0.0
    for k in range(a.frames):
        if k == a.frames - 1:
            zs, ups = ctl.encode(run.state).clone(), run.u_prev.clone()
            wins = run.zpad[k + 1:k + 1 + H].clone()
        run.runFunc()
        assert int(run.ok.min()) == 1
        it_max, it_sum = max(it_max, int(run.iters.max())), it_sum + float(run.iters.double().mean())
    r = measure(ctl, parent, "tracking", zs, wins, ups, a.launches)
    r.update(tracking_frames=a.frames, tracking_iters_max=it_max, tracking_iters_mean=it_sum / a.frames)
    recs.append(r)
    ctl.set_box_bilinear(max_iter=1)
    recs.append(measure(ctl, parent, "tracking, build + one sweep", zs, wins, ups, a.launches))
    parent.close()
    meta = dict(shape=dict(layers=LAYERS, u_dim=UD, horizon=H, N=H * UD, kind="delta_mpc", model="DBKN"),
                parent_lib="a build of the parent commit" if a.parent_lib else "this tree's library",
                device=torch.cuda.get_device_name(dev))
    if a.parent_lib:
        meta["untouched_entry_points_bitwise"] = compare_untouched(a.parent_lib)
    with open(a.out, "w") as f:
        json.dump(dict(meta=meta, records=recs), f, indent=1)
        f.write("\n")
    print(json.dumps(meta))
    for r in recs:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
