"""The Koopman training step (include/koopman_mpc.h sim_koopman_trainer_*, sim_koopman_loss_grad,
sim_koopman_train_step; control/koopman_train.py) for the DKUC model under "mse", against the float64
reference of koopman_train_ref.py, whose docstring states the reference and the tolerance rule.

Measured over the GPU tests' inputs (reference encoder and [8, 64, 64, 40], n = 1 .. 130, P = 1 and 5):
gradient spreads <= 1.1e-15 per block, so the bars are 2.2e-14 .. 1.1e-13; loss spreads (the reversed run
reverses the loss sums too) <= 4.8e-16 (bar <= 4.8e-14); parameter spreads after 1 and after 5 Adam steps
<= 6.1e-15 per block (bars <= 6.1e-13); the least pre-activation 7.8e-8.  Measured on an MI355X against
those bars: gradient error <= 1.3e-15, loss error <= 8.0e-16, parameter error <= 3.1e-15 -- at most 3% of
its bar in every block.  Every figure is printed beside its bar.
"""
import ctypes as C

import numpy as np
import pytest

import koopman_train_ref as kr
from koopman_train_ref import DKUC, LAYERS, LAYERS3, T, UD, XD


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("layers,n,P", [(LAYERS, 17, 5), (LAYERS3, 5, 1), (LAYERS, 1, 5)])
def test_reference_gradient_equals_autograd(layers, n, P):
    kr.check_reference_gradient_equals_autograd(DKUC, 0, layers, n, P, "mse")


def test_params_round_trip():
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, params_to_net
    net = kr.make_net(DKUC, 3, LAYERS3)
    p = params_from_net(net)
    assert p.dtype == np.float64 and p.size == kr.blocks(DKUC, LAYERS3)[-1][2]
    Ws, bs, A, B = kr.unpack(p, LAYERS3)
    assert np.array_equal(A, net.lA.weight.detach().numpy()) and np.array_equal(B, net.lB.weight.detach().numpy())
    assert np.array_equal(Ws[1], net.x_encode_net.linear_1.weight.detach().numpy())
    assert np.array_equal(bs[2], net.x_encode_net.linear_2.bias.detach().numpy())
    other = kr.fresh_net(DKUC, 4, LAYERS3)
    assert not np.array_equal(params_from_net(other), p)
    params_to_net(p, other)
    assert np.array_equal(params_from_net(other), p)
    assert torch.equal(other.lC.weight, net.lC.weight)
    with pytest.raises(ValueError):
        params_to_net(p[:-1], other)


def test_schedule_is_a_pure_function_of_its_seed():
    from lerobot_mujoco_sim2real_amd.control.koopman_train import schedule
    a, b, c = schedule(5, 37, 20, 5, 16, 3), schedule(5, 37, 20, 5, 16, 3), schedule(6, 37, 20, 5, 16, 3)
    assert len(a) == 3 and all(len(ep) == 3 for ep in a)
    for ea, eb in zip(a, b):
        for (ia, ta), (ib, tb) in zip(ea, eb):
            assert np.array_equal(ia, ib) and ta == tb and ia.dtype == np.int32
    assert any(not np.array_equal(x[0], y[0]) for ea, ec in zip(a, c) for x, y in zip(ea, ec))
    for ep in a:
        assert sorted(np.concatenate([i for i, _ in ep]).tolist()) == list(range(37))
        assert [len(i) for i, _ in ep] == [16, 16, 5]
        assert all(0 <= t0 <= 20 - 5 - 1 for _, t0 in ep)
    assert a[0][0][0].tolist() != a[1][0][0].tolist()


def test_trainer_entry_points_are_exported():
    from lerobot_mujoco_sim2real_amd import abi, build
    names = ["sim_koopman_trainer_nparam", "sim_koopman_trainer_create", "sim_koopman_trainer_free",
             "sim_koopman_trainer_get_params", "sim_koopman_trainer_set_params", "sim_koopman_loss_grad",
             "sim_koopman_train_step"]
    for name in names:
        assert name in abi.EXPORTS
    build.build()
    lib = abi.load_lib()
    assert len(lib.sim_koopman_loss_grad.argtypes) == 13 and len(lib.sim_koopman_train_step.argtypes) == 13
    d, o = kr.desc_opts()
    assert o.struct_size == C.sizeof(abi.KoopmanTrainOpts) == 48 and o.abi_version == abi.ABI_VERSION
    assert lib.sim_koopman_trainer_nparam(C.byref(d)) == kr.blocks(DKUC, LAYERS)[-1][2]
    import torch
    if not torch.cuda.is_available():  # no GPU: creation fails loudly, as sim_koopman_create does
        from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
        p, h = params_from_net(kr.make_net()), C.c_void_p()
        assert lib.sim_koopman_trainer_create(C.byref(d), p.ctypes.data_as(C.c_void_p), 16, C.byref(o), 0, C.byref(h)) == -4
        assert not h
    rows = np.zeros((2, 1, 13), np.float32)
    rp = rows.ctypes.data_as(C.c_void_p)
    assert lib.sim_koopman_loss_grad(None, 1, 1, 1, rp, 13, 5, 0, None, 0, None, None, None) == abi.E_ARG
    assert lib.sim_koopman_train_step(None, 1, 1, 1, rp, 13, 5, 0, None, 0, 1e-3, None, None) == abi.E_ARG


def test_unbuilt_models_and_losses_are_refused():
    from lerobot_mujoco_sim2real_amd.control.koopman import KoopmanBlinear
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer
    with pytest.raises(NotImplementedError, match="DBKN"):
        KoopmanTrainer(KoopmanBlinear(XD, UD, list(LAYERS)).double(), 16)
    with pytest.raises(NotImplementedError, match="mse"):
        KoopmanTrainer(kr.make_net(), 16, loss_name="mae")


# ------------------------------------------------------------------------------------------- GPU
CASES = [(layers, n, P, last) for layers in (LAYERS, LAYERS3) for n in (1, 16, 17, 65, 130) for P in (1, 5)
         for last in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("layers,n,P,last", CASES,
                         ids=[f"{'ref' if c[0] is LAYERS else 'nl3'}-n{c[1]}-P{c[2]}-{'tail' if c[3] else 't0'}" for c in CASES])
def test_loss_grad_matches_reference(layers, n, P, last):
    """traj_idx NULL / a permutation with repeats into a larger N and the in-place / second layout alternate
    over the cases so that each meets every n and both P."""
    k = (1, 16, 17, 65, 130).index(n)
    use_idx, alt = bool((k + last) % 2), bool((k + P // 5 + (layers is LAYERS3)) % 2)
    kr.check_loss_grad_matches_reference(DKUC, layers, n, P, last, 0, use_idx, alt)


@pytest.mark.gpu
def test_loss_grad_is_reproducible_and_keeps_to_its_buffer():
    tr, rows, _, _ = kr.check_reproducible_and_keeps_to_its_buffer(DKUC, 0)
    kr.check_null_outputs(tr, rows, 5, None)


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [LAYERS, LAYERS3], ids=["ref", "nl3"])
def test_train_steps_match_reference_adam(layers):
    kr.check_train_steps_match_reference_adam(DKUC, layers, 0)


@pytest.mark.gpu
def test_queued_steps_equal_synchronised_steps_and_reset():
    _, b, fresh, r, ix, p0 = kr.check_queued_steps_and_reset(DKUC)
    # without the reset the optimizer's state carries over
    b.set_params(p0, reset_optimizer=False)
    b.step(r, ix, 2, 1e-3)
    assert b.get_params().tobytes() != fresh.get_params().tobytes()


@pytest.mark.gpu
def test_round_trip_and_trained_model_feeds_the_controller():
    from lerobot_mujoco_sim2real_amd.control.koopman_train import KoopmanTrainer, params_from_net
    net = kr.fresh_net(DKUC, 2, LAYERS)
    tr = KoopmanTrainer(net, 32)
    assert np.array_equal(tr.get_params(), params_from_net(net))
    hist, _, e, _ = kr.check_train_end_to_end(net)
    assert not np.array_equal(hist["best_params"], tr.get_params())
    assert tuple(e["all_preds"].shape) == (40, T + 1, XD)


@pytest.mark.gpu
def test_argument_errors():
    kr.check_argument_errors(DKUC)
