"""Training the DKUC and DBKN Koopman models on the device: the fused loss / gradient / Adam step.

Reference: ``train()`` (``train.py:89-266``) over ``k_linear_loss`` (``models/losses.py:54-129``,
``loss_name`` ``"mse"``, ``"nmse"`` or ``"weighted_mse"``: ``BaseLoss``, ``models/losses.py:35-52``) with
``torch.optim.Adam`` and ``ExponentialLR(0.99)``.  One step there is six encoder calls, five ``lA`` / ``lB``
steps, about fifteen loss reductions, their autograd backward and the optimizer; here it is two kernel
launches (four for ``nmse``, whose normalisers are sums over the minibatch that every backward needs;
``include/koopman_mpc.h`` ``sim_koopman_train_step``, ``csrc/koopman_train.hip``) that read the rollout in place:

* :class:`KoopmanTrainer` -- the device trainer of one ``Koopmanlinear``: :meth:`loss_grad`,
  :meth:`step`, :meth:`get_params` / :meth:`set_params`, :meth:`to_net`;
* :class:`BilinearKoopmanTrainer` -- the same for one ``KoopmanBlinear`` (DBKN: the step gains
  ``H vec(z ⊗ u)``, the reference's ``koopman_operation``, ``models/KoopmanBase.py:62-78``);
* :func:`params_from_net` / :func:`params_to_net` -- the flat parameter vector
  ``[W_0 | b_0 | ... | A | B]`` (``| H`` for DBKN) of a net and back;
* :func:`schedule` / :func:`train` -- the reference's loop: shuffled minibatches from a seeded
  generator, a window start drawn per step, ``lr * 0.99^epoch``, ``MPCController.evaluate`` every
  ``eval_interval`` epochs, the best parameters kept; the trainer is picked by the net's type.

Built: DKUC and the bilinear DBKN (``net.H``, both ``u_z`` orders) with the reference's three training
losses.  Under ``weighted_mse`` the logged ``dis`` (and ``angle`` when ``x_dim - npos <= 3``) is NaN, as the
reference's is: the slice has no column past its third.  The DKN / DKAC input encoders, ``mae`` (the
reference's evaluation metric, not among its training choices) and the two regularisers ``k_linear_loss``
leaves out of ``total_loss`` (DBKN's ``‖H‖₁`` among them) are refused, not ignored.  :class:`KoopmanTrainer` itself
still refuses a net with ``H``: a DBKN net trained as DKUC would silently lose its bilinear term.
There is no CPU path.
"""
import ctypes as C

import numpy as np

from .. import abi

LOSS_NAMES = ("total", "koopman", "pred", "recon", "dis", "angle")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _has_h(net):
    import torch

    return isinstance(getattr(net, "H", None), torch.nn.Module)


def _check_net(net):
    if _has_h(net):
        raise NotImplementedError("KoopmanTrainer: DKUC only; the bilinear DBKN model (net.H) is trained by "
                                  "BilinearKoopmanTrainer")
    _check_common(net, "KoopmanTrainer", "DKUC")


def _check_bilinear_net(net):
    from .koopman import KoopmanBlinear

    if not isinstance(net, KoopmanBlinear) or not _has_h(net):
        raise NotImplementedError("BilinearKoopmanTrainer: the net must be a KoopmanBlinear (DBKN); a Koopmanlinear "
                                  "is trained by KoopmanTrainer")
    want = (net.Nkoopman, net.Nkoopman * net.u_dim)
    if tuple(net.H.weight.shape) != want or net.H.bias is not None:
        raise ValueError(f"net.H must be Linear({want[1]} -> {want[0]}, bias=False)")
    _check_common(net, "BilinearKoopmanTrainer", "DBKN")


def _check_common(net, who, model):
    import torch

    if not isinstance(getattr(net, "u_encode_net", None), torch.nn.Identity):
        raise NotImplementedError(f"{who}: an input encoder (DKN / DKAC) is not built; {model} only")
    lC = net.lC.weight.detach().double().cpu().numpy()
    if not np.array_equal(lC, np.eye(net.x_dim, net.Nkoopman)):
        raise ValueError("net.lC.weight must be the frozen decoder [I | 0]")


def params_from_net(net):
    """The flat float64 parameter vector of a ``Koopmanlinear``:
    ``[W_0 | b_0 | ... | W_{nl-1} | b_{nl-1} | lA (nz x nz) | lB (nz x u_dim)]``, row-major; a
    ``KoopmanBlinear``'s ends with ``H (nz x nz u_dim)``, ``net.H.weight`` in the net's own ``u_z`` order."""
    parts = []
    for W, b in net.encoder_layers():
        parts += [W.ravel(), b]
    parts += [net.lA.weight.detach().double().cpu().numpy().ravel(), net.lB.weight.detach().double().cpu().numpy().ravel()]
    if _has_h(net):
        parts.append(net.H.weight.detach().double().cpu().numpy().ravel())
    return np.ascontiguousarray(np.concatenate(parts), np.float64)


def params_to_net(params, net):
    """Write a flat parameter vector (:func:`params_from_net`'s layout) into ``net``, in place."""
    import torch

    p = np.asarray(params, np.float64).ravel()
    mods = [m for m in net.x_encode_net if isinstance(m, torch.nn.Linear)]
    tail = [net.lA.weight, net.lB.weight] + ([net.H.weight] if _has_h(net) else [])
    want = sum(m.weight.numel() + m.bias.numel() for m in mods) + sum(t.numel() for t in tail)
    if p.size != want:
        raise ValueError(f"params_to_net: {p.size} parameters given, the net has {want}")
    o = 0
    with torch.no_grad():
        for t in [x for m in mods for x in (m.weight, m.bias)] + tail:
            k = t.numel()
            t.copy_(torch.as_tensor(p[o:o + k].reshape(tuple(t.shape)), dtype=t.dtype))
            o += k
    return net


class KoopmanTrainer:
    """The device trainer of one DKUC model (``sim_koopman_trainer``).

    ``net``: this project's ``Koopmanlinear``; it is read at construction and not touched again
    (:meth:`to_net` writes the trained parameters back).  ``max_batch``: the largest minibatch.
    ``pre_length``, ``npos``, ``gamma`` as the reference's args (5, 3, 0.8); ``betas``, ``eps``
    Adam's.  ``loss_name``: ``"mse"``, ``"nmse"`` or ``"weighted_mse"`` (``x_dim >= 4``)."""

    _check = staticmethod(_check_net)

    def _nparam(self, d):
        return self.lib.sim_koopman_trainer_nparam(C.byref(d))

    def _create(self, d, p, max_batch, o, device):
        return self.lib.sim_koopman_trainer_create(C.byref(d), p.ctypes.data_as(C.c_void_p), int(max_batch), C.byref(o),
                                                   device, C.byref(self._h))

    def __init__(self, net, max_batch, device=0, pre_length=5, npos=3, gamma=0.8, betas=(0.9, 0.999), eps=1e-8,
                 loss_name="mse"):
        import torch

        if loss_name not in abi.KLOSS:
            raise NotImplementedError(f"{type(self).__name__}: loss_name {loss_name!r} is not built; "
                                      "'mse', 'nmse', 'weighted_mse' only")
        self._h = None
        self._check(net)
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.torch, self.net = torch, net
        self.device = torch.device("cuda", device)
        self.x_dim, self.u_dim, self.pre_length = net.x_dim, net.u_dim, int(pre_length)
        layers = net.encoder_layers()
        widths = [layers[0][0].shape[1]] + [W.shape[0] for W, _ in layers]
        d = abi.KoopmanDesc()
        d.x_dim, d.u_dim, d.nlayer, d.horizon, d.u_clip = net.x_dim, net.u_dim, len(layers), 10, 0.5
        for i, w in enumerate(widths):
            d.width[i] = w
        o = abi.KoopmanTrainOpts()
        o.pre_length, o.npos, o.gamma = int(pre_length), int(npos), float(gamma)
        o.beta1, o.beta2, o.eps = float(betas[0]), float(betas[1]), float(eps)
        self.lib = abi.load_lib()
        p = params_from_net(net)
        n = self._nparam(d)
        if n < 0:
            abi.check(self.lib, n)
        if n != p.size:
            raise ValueError(f"{type(self).__name__}: the net has {p.size} parameters, the library expects {n}")
        self.nparam, self.max_batch = n, int(max_batch)
        self._h = C.c_void_p()
        abi.check(self.lib, self._create(d, p, max_batch, o, device))
        rc = self.lib.sim_koopman_trainer_set_loss(self._h, abi.KLOSS[loss_name])
        if rc == abi.E_ARG:
            raise ValueError(f"{type(self).__name__}: {self.lib.sim_last_error().decode()}")
        abi.check(self.lib, rc)

    @property
    def loss_name(self):
        """The trainer's loss, by the reference's name."""
        k = self.lib.sim_koopman_trainer_get_loss(self._h)
        return next(name for name, v in abi.KLOSS.items() if v == k)

    def __del__(self):
        try:
            if self._h:
                self.lib.sim_koopman_trainer_free(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _data(self, rollout, idx):
        """(rows, N, T, idx, n) of a device rollout [T+1, N, u_dim + x_dim] ([u | x] rows) and a
        minibatch (int32 device tensor of trajectory numbers, or None for all of them)."""
        torch = self.torch
        r = torch.as_tensor(rollout)
        ld = self.u_dim + self.x_dim
        if r.dim() != 3 or r.shape[2] != ld or r.shape[0] < 1:
            raise ValueError(f"rollout must be [T+1, N, {ld}] ([u | x] rows); got {tuple(r.shape)}")
        r = r.to(device=self.device, dtype=torch.float32).contiguous()
        if idx is not None:
            idx = torch.as_tensor(idx).to(device=self.device, dtype=torch.int32).contiguous()
        n = r.shape[1] if idx is None else int(idx.numel())
        return r, r.shape[1], r.shape[0] - 1, idx, n

    def loss_grad(self, rollout, idx, t0, want_grad=True):
        """The loss of the windows ``t0 .. t0 + pre_length`` of trajectories ``idx`` and its gradient:
        (losses [6] float64: total, koopman, pred, recon, dis, angle; grad [nparam] float64 or None),
        device tensors; asynchronous on the current stream.  Changes no trainer state."""
        torch = self.torch
        r, N, T, idx, n = self._data(rollout, idx)
        losses = torch.empty(6, dtype=torch.float64, device=self.device)
        grad = torch.empty(self.nparam, dtype=torch.float64, device=self.device) if want_grad else None
        abi.check(self.lib, self.lib.sim_koopman_loss_grad(self._h, n, N, T, _ptr(r), self.u_dim + self.x_dim, self.u_dim, 0,
                                                           _ptr(idx), int(t0), _ptr(losses), _ptr(grad), self._stream()))
        return losses, grad

    def step(self, rollout, idx, t0, lr, losses=None):
        """One Adam step on the same loss; returns the losses [6] before the update (a device
        tensor; pass ``losses`` to reuse one).  Asynchronous: no host synchronisation."""
        torch = self.torch
        r, N, T, idx, n = self._data(rollout, idx)
        if losses is None:
            losses = torch.empty(6, dtype=torch.float64, device=self.device)
        abi.check(self.lib, self.lib.sim_koopman_train_step(self._h, n, N, T, _ptr(r), self.u_dim + self.x_dim, self.u_dim, 0,
                                                            _ptr(idx), int(t0), float(lr), _ptr(losses), self._stream()))
        return losses

    def get_params(self):
        """The parameter vector [nparam] float64 (numpy; synchronises)."""
        p = np.empty(self.nparam, np.float64)
        abi.check(self.lib, self.lib.sim_koopman_trainer_get_params(self._h, p.ctypes.data_as(C.c_void_p)))
        return p

    def set_params(self, params, reset_optimizer=False):
        p = np.ascontiguousarray(params, np.float64).ravel()
        if p.size != self.nparam:
            raise ValueError(f"set_params: {p.size} parameters given, the trainer has {self.nparam}")
        abi.check(self.lib, self.lib.sim_koopman_trainer_set_params(self._h, p.ctypes.data_as(C.c_void_p),
                                                                    int(bool(reset_optimizer))))

    def to_net(self, net=None, params=None):
        """The trained parameters (or ``params``) written into ``net`` (default: the construction
        net), which then feeds ``MPCController`` unchanged."""
        return params_to_net(self.get_params() if params is None else params, self.net if net is None else net)


class BilinearKoopmanTrainer(KoopmanTrainer):
    """The device trainer of one DBKN model: a ``KoopmanBlinear`` (either ``u_z``) with the identity
    input encoder and the frozen ``lC``.  The methods are :class:`KoopmanTrainer`'s; the parameter
    vector ends with ``H`` (:func:`params_from_net`)."""

    _check = staticmethod(_check_bilinear_net)

    def _nparam(self, d):
        return self.lib.sim_koopman_trainer_nparam_bilinear(C.byref(d))

    def _create(self, d, p, max_batch, o, device):
        return self.lib.sim_koopman_trainer_create_bilinear(C.byref(d), p.ctypes.data_as(C.c_void_p), int(bool(self.net.u_z)),
                                                            int(max_batch), C.byref(o), device, C.byref(self._h))


def schedule(seed, n_traj, steps, pre_length, batch_size, epochs):
    """The minibatches and window starts of :func:`train`, a pure function of its arguments:
    a list over epochs of lists of (idx int32 numpy, t0); every epoch a fresh permutation of the
    trajectories cut into ``batch_size`` pieces (the last may be short), ``t0`` uniform in
    ``0 .. steps - pre_length - 1`` as the reference's ``random.randint`` (``steps`` = T)."""
    if steps - pre_length - 1 < 0:
        raise ValueError(f"schedule: the rollout's {steps} steps are too few for pre_length {pre_length}")
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(epochs):
        perm = rng.permutation(n_traj).astype(np.int32)
        ep = []
        for b in range(0, n_traj, batch_size):
            ep.append((perm[b:b + batch_size], int(rng.integers(0, steps - pre_length))))
        out.append(ep)
    return out


def train(net, rollout, args=None, epochs=10, batch_size=128, lr=1e-3, lr_decay=0.99, seed=0, eval_rollout=None,
          eval_interval=1, device=0, pre_length=5, gamma=0.8, npos=3, loss_name="mse"):
    """The reference's training loop on a device rollout [T+1, N, u_dim + x_dim] (``rollout_device``).

    Adam at ``lr`` decayed by ``lr_decay`` per epoch (``ExponentialLR``), the minibatches and window
    starts of :func:`schedule`, one fused step per minibatch with no host synchronisation inside an
    epoch.  Every ``eval_interval`` epochs the model is written into ``net`` and evaluated with
    ``MPCController.evaluate`` on ``eval_rollout`` (default: ``rollout``); the parameters with the
    lowest ``avg_error`` are kept and are in ``net`` on return.  ``args``: the controller's args
    (x_dim, u_dim, MPC_type); default from the net.  Returns the history dict: ``train_loss`` [epochs][6]
    (the mean of the epoch's step losses under ``loss_name``; its dis column is NaN for ``weighted_mse`` at npos <= 3), ``lr``, ``eval`` [(epoch, avg, dis, angle)], ``best_epoch``,
    ``best_error``, ``best_params``."""
    import torch

    from .MPC_Controler import MPCController

    if args is None:
        class args:  # noqa: N801
            x_dim, u_dim, MPC_type = net.x_dim, net.u_dim, "delta_mpc"
    dev = torch.device("cuda", device)
    r = torch.as_tensor(rollout).to(device=dev, dtype=torch.float32).contiguous()
    ev = r if eval_rollout is None else torch.as_tensor(eval_rollout).to(device=dev, dtype=torch.float32).contiguous()
    T, N = r.shape[0] - 1, r.shape[1]
    cls = BilinearKoopmanTrainer if _has_h(net) else KoopmanTrainer  # DBKN / DKUC
    tr = cls(net, min(batch_size, N), device=device, pre_length=pre_length, npos=npos, gamma=gamma, loss_name=loss_name)
    sched = schedule(seed, N, T, pre_length, batch_size, epochs)
    hist = dict(train_loss=[], lr=[], eval=[], best_epoch=-1, best_error=float("inf"), best_params=tr.get_params())
    for ep, batches in enumerate(sched):
        cur = lr * lr_decay ** ep
        losses = torch.empty((len(batches), 6), dtype=torch.float64, device=dev)
        idx = [torch.as_tensor(b, device=dev) for b, _ in batches]
        for k, (_, t0) in enumerate(batches):
            tr.step(r, idx[k], t0, cur, losses=losses[k])
        hist["train_loss"].append(losses.mean(0).tolist())
        hist["lr"].append(cur)
        if (ep + 1) % eval_interval == 0 or ep + 1 == epochs:
            p = tr.get_params()
            e = MPCController(tr.to_net(params=p), args, device=device).evaluate(ev)
            hist["eval"].append((ep, e["avg_error"], e["dis_error"], e["angle_error"]))
            if e["avg_error"] < hist["best_error"]:
                hist["best_error"], hist["best_epoch"], hist["best_params"] = e["avg_error"], ep, p
    params_to_net(hist["best_params"], net)
    return hist
