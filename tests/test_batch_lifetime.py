"""Batch and device-model lifetime (soarm_sim.hip): a model's device copy is uploaded by the first
batch on a device, reused by every later one and freed with the model, after its batches."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def second_batch_matches_first(n=64):
    """Pick scene, n envs: a batch is created, reset (fixed seed), stepped once, read and freed;
    a second batch of the same model on the same device (it finds the cached device model) repeats
    that bit for bit; the batch is freed before the model."""
    import torch  # noqa: F401  (before the library, as BatchSim does: one HIP runtime per process, torch's)
    from lerobot_mujoco_sim2real_amd import abi, workloads as W
    from lerobot_mujoco_sim2real_amd.sim import BatchSim, SimModel
    lib = abi.load_lib()
    cm = W.model("contact")
    ids = np.arange(n)
    q0 = W.initial_qpos(cm, ids, 0)
    act = W.chirp_action(W.chirp_tables(ids, 0), 0)
    handle = SimModel(cm, lib)

    def run():
        S = BatchSim(cm, n, 0, model_handle=handle)
        S.reset(init_qpos=q0[:, :5], extra_qpos=q0, seed=7)
        S.step(act)
        out = [x.detach().cpu().numpy().copy() for x in (S.obs, S.qpos, S.qvel)]
        assert int((S.status != 0).sum()) == 0
        S.close()
        return out

    first, second = run(), run()
    for name, a, b in zip(("obs", "qpos", "qvel"), first, second):
        assert np.isfinite(a).all() and np.array_equal(a, b), name
    assert np.abs(first[2]).max() > 0  # (the step moved something)
    lib.sim_model_free(handle.ptr)
    handle.ptr = None


@pytest.mark.gpu
def test_second_batch_reuses_device_model_rs(gpu_lib, monkeypatch):
    """The row-space substep kernel (64 envs: below rs_cap)."""
    monkeypatch.setenv("SOARM_RS", "1")
    second_batch_matches_first()


@pytest.mark.gpu
def test_second_batch_reuses_device_model_quad(gpu_lib):
    """The quad kernel (SOARM_RS=0), in a fresh process: SOARM_RS is read per call, but the child
    keeps this process's graph cache out of the comparison."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import soarm_pkg, test_batch_lifetime as T; "
            "T.second_batch_matches_first(); print('second-batch-ok')" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SOARM_RS="0"), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "second-batch-ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
