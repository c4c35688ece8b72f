"""The bilinear (DBKN) Koopman training step (include/koopman_mpc.h sim_koopman_trainer_create_bilinear,
sim_koopman_trainer_nparam_bilinear; control/koopman_train.py BilinearKoopmanTrainer) under "mse", for both
u_z, against the float64 reference of koopman_train_ref.py, whose docstring states the reference (the H
term and its adjoint), the nets and the tolerance rule; H is one more block under that rule.

Measured over the GPU tests' inputs (both encoders, both u_z, n = 1 .. 130, P = 1 and 5):
gradient spreads <= 1.03e-15 per block (H: <= 9.2e-16), so the bars are 2.2e-14 .. 1.03e-13; loss spreads
(the reversed run reverses the loss sums too) <= 4.4e-16 (bar <= 4.4e-14); parameter spreads after 1 and after 5 Adam steps <= 1.6e-14 per block (H: 5.1e-16;
bars <= 1.6e-12); the least pre-activation 3.9e-7; max |dH| >= 3.8e-3 in every case (not a near-zero block).
Measured on an MI355X against those bars:
gradient error <= 1.6e-15 (H: 1.5e-15), loss error <= 6.1e-16, parameter error <= 1.1e-14 (H: 5.1e-16) -- at
most 5% of its bar in every block.  With H = 0 the losses and the W, b, A, B blocks equal the DKUC trainer's
bit for bit (the test asks only for the bar).
"""
import ctypes as C

import numpy as np
import pytest

import koopman_train_ref as kr
from koopman_train_ref import DBKN, DKUC, LAYERS, LAYERS3, T, UD, XD


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("u_z", [0, 1])
@pytest.mark.parametrize("layers,n,P", [(LAYERS, 17, 5), (LAYERS3, 5, 1), (LAYERS, 1, 5)])
def test_reference_gradient_equals_autograd(layers, n, P, u_z):
    kr.check_reference_gradient_equals_autograd(DBKN, u_z, layers, n, P, "mse")


@pytest.mark.parametrize("u_z", [0, 1])
def test_params_round_trip(u_z):
    import torch
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net, params_to_net
    net = kr.make_net(DBKN, 3, LAYERS3, u_z)
    p = params_from_net(net)
    bl = kr.blocks(DBKN, LAYERS3)
    nz, nlin = XD + LAYERS3[-1], kr.blocks(DKUC, LAYERS3)[-1][2]
    assert p.dtype == np.float64 and p.size == bl[-1][2] == nlin + nz * nz * UD and bl[-1][1] == nlin
    assert np.array_equal(p[nlin:].reshape(nz, nz * UD), net.H.weight.detach().numpy())
    assert np.abs(p[nlin:]).max() > 0
    _, _, A, B = kr.unpack(p, LAYERS3)
    assert np.array_equal(A, net.lA.weight.detach().numpy()) and np.array_equal(B, net.lB.weight.detach().numpy())
    other = kr.fresh_net(DBKN, 4, LAYERS3, u_z)
    assert not np.array_equal(params_from_net(other)[nlin:], p[nlin:])
    params_to_net(p, other)
    assert np.array_equal(params_from_net(other), p)
    assert torch.equal(other.H.weight, net.H.weight) and torch.equal(other.lC.weight, net.lC.weight)
    with pytest.raises(ValueError):
        params_to_net(p[:-1], other)
    with pytest.raises(ValueError):  # a DKUC vector is too short for a DBKN net
        params_to_net(p[:nlin], other)
    # a Koopmanlinear's vector is what it was: no H block
    assert params_from_net(kr.make_net(DKUC, 3, LAYERS3)).size == nlin
    with pytest.raises(ValueError):
        params_to_net(p, kr.fresh_net(DKUC, 4, LAYERS3))


def test_bilinear_entry_points_are_exported():
    from lerobot_mujoco_sim2real_amd import abi, build
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_from_net
    for name in ("sim_koopman_trainer_nparam_bilinear", "sim_koopman_trainer_create_bilinear"):
        assert name in abi.EXPORTS
    build.build()
    lib = abi.load_lib()
    assert len(lib.sim_koopman_trainer_create_bilinear.argtypes) == 7
    d, o = kr.desc_opts()
    assert C.sizeof(abi.KoopmanTrainOpts) == 48 and abi.ABI_VERSION == 2
    nlin = lib.sim_koopman_trainer_nparam(C.byref(d))
    assert nlin == kr.blocks(DKUC, LAYERS)[-1][2]
    assert lib.sim_koopman_trainer_nparam_bilinear(C.byref(d)) == nlin + 32 * 32 * 5 == kr.blocks(DBKN, LAYERS)[-1][2]
    assert lib.sim_koopman_trainer_nparam_bilinear(None) == abi.E_ARG
    p, h = params_from_net(kr.make_net(DBKN)), C.c_void_p()
    pp = p.ctypes.data_as(C.c_void_p)
    for bad in (2, -1):  # u_z is 0 or 1
        assert lib.sim_koopman_trainer_create_bilinear(C.byref(d), pp, bad, 16, C.byref(o), 0, C.byref(h)) == abi.E_ARG
        assert not h and b"u_z" in lib.sim_last_error()
    import torch
    if not torch.cuda.is_available():  # no GPU: creation fails loudly, as sim_koopman_trainer_create does
        for u_z in (0, 1):
            assert lib.sim_koopman_trainer_create_bilinear(C.byref(d), pp, u_z, 16, C.byref(o), 0, C.byref(h)) == -4
            assert not h


def test_bilinear_trainer_refuses_other_nets_and_losses():
    from lerobot_mujoco_sim2real_amd.control.koopman_train import BilinearKoopmanTrainer, KoopmanTrainer
    assert issubclass(BilinearKoopmanTrainer, KoopmanTrainer)
    with pytest.raises(NotImplementedError, match="KoopmanBlinear"):
        BilinearKoopmanTrainer(kr.make_net(DKUC), 16)
    with pytest.raises(NotImplementedError, match="mse"):
        BilinearKoopmanTrainer(kr.make_net(DBKN), 16, loss_name="mae")
    with pytest.raises(NotImplementedError, match="DBKN"):  # and the DKUC trainer still refuses a net with H
        KoopmanTrainer(kr.make_net(DBKN), 16)


# ------------------------------------------------------------------------------------------- GPU
def _cases():
    """(layers, n, P, last, u_z, use_idx, alt): every (encoder, n, P) once, the four alternatives as parities
    of the three indices chosen so that each value of each meets every n, both P and both encoders;
    then four more with the window position and u_z flipped."""
    ns, out = (1, 16, 17, 65, 130), []
    for ei, layers in enumerate((LAYERS, LAYERS3)):
        for k, n in enumerate(ns):
            for pi, P in enumerate((1, 5)):
                out.append((layers, n, P, (pi + ei + (k >> 1)) % 2, (k + pi + ei) % 2, (k + pi) % 2, (k + ei) % 2))
    for layers, n, P in ((LAYERS, 130, 5), (LAYERS3, 130, 1), (LAYERS, 17, 1), (LAYERS3, 65, 5)):
        c = next(c for c in out if c[:3] == (layers, n, P))
        out.append((layers, n, P, 1 - c[3], 1 - c[4], c[5], c[6]))
    for j, name in ((3, "last"), (4, "u_z"), (5, "use_idx"), (6, "alt")):  # the coverage the docstring promises
        for v in (0, 1):
            got = [c for c in out if c[j] == v]
            assert {c[1] for c in got} == set(ns) and {c[2] for c in got} == {1, 5} and {c[0] for c in got} == {LAYERS, LAYERS3}, name
    return out


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("layers,n,P,last,u_z,use_idx,alt", CASES,
                         ids=[f"{'ref' if c[0] is LAYERS else 'nl3'}-n{c[1]}-P{c[2]}-{'tail' if c[3] else 't0'}-uz{c[4]}-"
                              f"{'idx' if c[5] else 'all'}-{'ld16' if c[6] else 'ld13'}" for c in CASES])
def test_loss_grad_matches_reference(layers, n, P, last, u_z, use_idx, alt):
    kr.check_loss_grad_matches_reference(DBKN, layers, n, P, last, u_z, use_idx, alt)


@pytest.mark.gpu
def test_loss_grad_is_reproducible_and_keeps_to_its_buffer():
    kr.check_reproducible_and_keeps_to_its_buffer(DBKN, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("u_z", [0, 1])
def test_train_steps_match_reference_adam(u_z):
    kr.check_train_steps_match_reference_adam(DBKN, LAYERS, u_z)


@pytest.mark.gpu
def test_queued_steps_equal_synchronised_steps_and_reset():
    a, _, _, _, _, p0 = kr.check_queued_steps_and_reset(DBKN)
    with pytest.raises(ValueError):  # a DKUC-sized vector is not this trainer's
        a.set_params(p0[:kr.blocks(DKUC, LAYERS)[-1][2]])


@pytest.mark.gpu
@pytest.mark.parametrize("u_z", [0, 1])
def test_zero_h_agrees_with_the_linear_trainer(u_z):
    """H = 0: DBKN is DKUC.  Losses and the W, b, A, B gradient blocks against KoopmanTrainer on the same
    linear part and inputs, within the bar of the bilinear reference; the H block (not zero: dH does not
    depend on H at P = 1 and only through lambda beyond) against the reference's."""
    from lerobot_mujoco_sim2real_amd.control.koopman_train import params_to_net
    n, P, t0 = 65, 5, 1
    rows, idx, p, l64, g64, gs, ls = kr.reference(DBKN, LAYERS, n, P, t0, True, u_z, hscale=0.0)
    nlin = kr.blocks(DKUC, LAYERS)[-1][2]
    assert not p[nlin:].any() and np.abs(g64[nlin:]).max() > 0
    tl = kr.trainer(DKUC, LAYERS, 130, P, net=params_to_net(np.array(p[:nlin]), kr.fresh_net(DKUC, 5, LAYERS)))
    tb = kr.trainer(DBKN, LAYERS, 130, P, u_z, hscale=0.0)
    assert np.array_equal(tl.get_params(), tb.get_params()[:nlin])
    ll, gl = kr.abi_loss_grad(tl, rows, idx, t0)
    lb, gb = kr.abi_loss_grad(tb, rows, idx, t0)
    kr.assert_losses(lb, ll, ls, "mse", 3, "losses (H = 0) against the linear trainer")
    kr.assert_losses(lb, l64, ls, "mse", 3, "losses (H = 0)")
    kr.assert_blocks(kr.blocks(DKUC, LAYERS), gb, gl, gs, "grad(H=0) against the linear trainer", scale_from=g64)
    kr.assert_blocks(kr.blocks(DBKN, LAYERS), gb, g64, gs, "grad(H=0)")


@pytest.mark.gpu
def test_trained_dbkn_model_feeds_the_controller():
    import torch
    net = kr.fresh_net(DBKN, 2, LAYERS, 0, 0.0)  # H starts at zero, as the reference's does
    assert not net.H.weight.any()
    hist, ctl, _, rows = kr.check_train_end_to_end(net)
    assert hist["best_params"].size == kr.blocks(DBKN, LAYERS)[-1][2]
    Hw = net.H.weight.detach()
    assert float(Hw.abs().max()) > 0 and bool(torch.isfinite(Hw).all())
    assert ctl.bilinear
    # one control step of the trained model through k_bilinear
    n, dev = 40, rows.device
    zref = ctl.lift_reference(rows[:, :, UD:])                       # [T+1, nz, n]
    window = torch.zeros((ctl.H, ctl.Nkoopman, n), dtype=torch.float64, device=dev)
    window[:T] = zref[1:T + 1]
    u_prev = torch.zeros((UD, n), dtype=torch.float64, device=dev)
    action = ctl.step_bilinear(rows[0, :, UD:], window, u_prev)
    torch.cuda.synchronize()
    assert tuple(action.shape) == (n, UD) and bool(torch.isfinite(action).all()) and bool(torch.isfinite(u_prev).all())


@pytest.mark.gpu
def test_argument_errors():
    kr.check_argument_errors(DBKN)
