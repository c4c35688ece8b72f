"""bench.py's command line: --dump-outputs writes float arrays within its size budget; a plain run
times --steps steps and leaves the side measurements to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    """Small arrays are written whole (float32 / float64 kept, anything else as float64); an array over
    its share of the budget becomes a fixed, seeded sample of its elements, the same on every call."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 400)  # 400 bytes per array
    g = torch.Generator().manual_seed(1)
    outs = {"a": torch.rand((7, 5), generator=g), "b": torch.rand((3, 4), generator=g, dtype=torch.float64),
            "c": torch.arange(1000, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / "x"), outs, 0, seed=3)
    bench.dump_outputs(str(tmp_path / "y"), outs, 0, seed=3)
    got = {k: np.load(tmp_path / "x" / f"{k}.npy") for k in outs}
    assert got["a"].dtype == np.float32 and np.array_equal(got["a"], outs["a"].numpy())
    assert got["b"].dtype == np.float64 and np.array_equal(got["b"], outs["b"].numpy())
    c = got["c"]
    assert c.dtype == np.float64 and c.shape == (50,) and len(np.unique(c)) == 50
    assert np.all(np.diff(c) > 0) and np.all(c == np.round(c)) and c.min() >= 0 and c.max() < 1000
    assert sum(v.nbytes for v in got.values()) <= 3 * 400
    for k in outs:
        assert np.array_equal(got[k], np.load(tmp_path / "y" / f"{k}.npy"))
    bench.dump_outputs(str(tmp_path / "x"), {"a": outs["a"]}, 2, seed=3)
    assert np.array_equal(np.load(tmp_path / "x" / "a.rank2.npy"), got["a"])
    # the budget is the whole run's: each of `world` ranks gets 1/world of it
    bench.dump_outputs(str(tmp_path / "z"), {"c": outs["c"]}, 1, seed=3, world=2)
    assert np.load(tmp_path / "z" / "c.rank1.npy").nbytes == 3 * 400 // 2


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "64", "--steps", "3",
                        "--warmup", "2"] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain_run(gpu_lib, tmp_path_factory):
    """One plain run of the headline config (64 envs, 3 timed steps after 2): (result line, dump)."""
    d = tmp_path_factory.mktemp("plain") / "out"
    return _bench("--dump-outputs", str(d)), _load(d)


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_last_step(plain_run):
    """A plain run prints one result line with the headline fields and none of --full's side
    measurements, and --dump-outputs holds the state after step 5: the same workload stepped here
    through BatchSim gives the same arrays."""
    from lerobot_mujoco_sim2real_amd import workloads as W
    from lerobot_mujoco_sim2real_amd.sim import BatchSim
    line, got = plain_run
    assert line["metric"] == bench.METRIC and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 2
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(64 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("roofline", "steady_state", "other_solver", "cpu_baseline"):
        assert line[k] is None, k

    n, ids = 64, np.arange(64)
    cm = W.model("contact")
    sim = BatchSim(cm, n, 0)
    q0 = W.initial_qpos(cm, ids, 0)
    sim.reset(init_qpos=q0[:, :5], extra_qpos=q0, seed=0)
    # the bench's input stream, built as it builds it (fp32 chirp rows on the device): the library is
    # deterministic, so the arrays are equal bit for bit
    tab = {k: (torch.as_tensor(v, dtype=torch.float32, device="cuda:0") if isinstance(v, np.ndarray) else v)
           for k, v in W.chirp_tables(ids, 0).items()}
    act = sim.action_buffer()
    for t in range(5):
        act.copy_(W.chirp_action(tab, float(t), lib=torch))
        obs = sim.step(act)
    want = {"obs": obs, "qpos": sim.qpos, "qvel": sim.qvel}
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == np.float32 and np.isfinite(got[k]).all()
        assert np.array_equal(got[k], v.cpu().numpy()), k


@pytest.mark.gpu
def test_full_run_adds_side_measurements_and_dumps_the_timed_step(plain_run, tmp_path):
    """--full fills the side measurements (here the replay's roofline and the steady window) and its
    dump, written before those replays overwrite the state, equals the plain run's bit for bit."""
    line0, want = plain_run
    line = _bench("--full", "--no-cpu-baseline", "--no-other-solver", "--dump-outputs", str(tmp_path / "out"))
    assert line["metric"] == line0["metric"] and line["steps"] == 3 and line["warmup"] == 2
    assert line["roofline"]["kernel_ms_per_step"] and line["steady_state"]["window"] == "env-steps 20-120"
    got = _load(tmp_path / "out")
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["rollout", "mpc"])
def test_dump_of_rollout_and_mpc_configs(gpu_lib, tmp_path, config):
    """The configs with outputs of their own: the rollout's recorded rows ([u | obs] per timed step,
    the last obs row being the returned observation) and IK state, the MPC's last control."""
    line = _bench("--config", config, "--dump-outputs", str(tmp_path / "out"))
    assert line["config"]["config"] == config and line["validity"]["state_finite"]
    got = _load(tmp_path / "out")
    nq, nv = got["qpos"].shape[0], got["qvel"].shape[0]
    shapes = {"obs": (64, 8), "qpos": (nq, 64), "qvel": (nv, 64)}
    if config == "rollout":
        shapes.update(rollout_u=(3, 64, 5), rollout_obs=(4, 64, 8), qstar=got["qstar"].shape[:1] + (64,))
    else:
        shapes["u_prev"] = (5, 64)
    assert {k: v.shape for k, v in got.items()} == shapes
    for k, v in got.items():
        assert v.dtype == (np.float64 if k == "u_prev" else np.float32) and np.isfinite(v).all(), k
    if config == "rollout":
        assert np.array_equal(got["rollout_obs"][-1], got["obs"])
        assert not np.array_equal(got["rollout_obs"][0], got["rollout_obs"][-1]) and np.abs(got["rollout_u"]).max() > 0
    else:
        assert np.abs(got["u_prev"]).max() > 0
