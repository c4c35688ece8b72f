"""The Koopman model the MPC controller lifts states with.

Reference: ``models/KoopmanBase.py:12-60`` (``Koopmanlinear``, the ``DKUC`` model that
``init_model`` builds, ``models/init_model.py:4-10``) with ``encode_layers = [x_dim, 64, 64, 64,
64, 24]`` (``args.py:103``), so ``Nkoopman = 24 + x_dim = 32``.  Only what the controller needs
is kept: the encoder ``x_encoder(x) = cat([x, MLP(x)])``, the Koopman matrices ``lA``
(Nkoopman x Nkoopman, initialised as 0.9 x an orthogonalised Gaussian draw) and ``lB``
(Nkoopman x u_dim), and the fixed decoder ``lC = [I | 0]``.  Training either model (``train.py``,
``models/losses.py``) is ``control/koopman_train.py`` (the fused device step); its evaluation -- the
multi-step open-loop prediction error of ``evaluate()`` -- is :func:`open_loop_prediction` /
:func:`prediction_errors` here and ``MPCController.predict`` / ``evaluate`` on the device.  Parameter names are the reference's
(``x_encode_net.linear_{i}``, ``lA``, ``lB``, ``lC``, DBKN's ``H``), so a state_dict the reference
saved loads with ``load_state_dict(..., strict=True)`` (``tests/test_koopman_mpc.py``).

The bilinear ``DBKN`` model (``KoopmanBlinear``, ``:62-110``) adds ``H (z ⊗ u)`` to the step;
the MPC linearises it at the frame's lifted state, ``B_total = Bd + Σ_j z0_j Ĥ_j``
(``MPC_Controler.py:46-63``), so its QP differs per env and frame: :func:`bilinear_first_move`
solves those QPs batched in float64 on the device.
"""
from collections import OrderedDict

import numpy as np
import torch
from torch import nn


class Koopmanlinear(nn.Module):
    """DKUC: z_{k+1} = lA z_k + lB u_k with z = [x, MLP(x)]."""

    def __init__(self, x_dim, u_dim, encode_layers):
        super().__init__()
        self.x_dim, self.u_dim = x_dim, u_dim
        self.Nkoopman = encode_layers[-1] + x_dim
        # named modules linear_{i} / relu_{i} as KoopmanBase.py:20-27, so the reference's saved
        # state_dict (x_encode_net.linear_0.weight, ...) loads strictly (Koopman_MPC.py:262-265)
        mods = OrderedDict()
        for i, (a, b) in enumerate(zip(encode_layers[:-1], encode_layers[1:])):
            mods[f"linear_{i}"] = nn.Linear(a, b)
            if i + 2 < len(encode_layers):
                mods[f"relu_{i}"] = nn.ReLU()
        self.x_encode_net = nn.Sequential(mods)
        self.u_encode_net = nn.Identity()
        nk = self.Nkoopman
        self.lA = nn.Linear(nk, nk, bias=False)
        g = torch.randn(nk, nk) / nk  # N(0, (1/nk)^2) as gaussian_init_ (KoopmanBase.py:7-10)
        U, _, V = torch.svd(g)
        self.lA.weight.data = (U @ V.t()) * 0.9
        self.lB = nn.Linear(u_dim, nk, bias=False)
        self.lC = nn.Linear(nk, x_dim, bias=False)
        with torch.no_grad():
            self.lC.weight.zero_()
            self.lC.weight[:, :x_dim] = torch.eye(x_dim)
        self.lC.weight.requires_grad = False

    def x_encoder(self, x):
        return torch.cat([x, self.x_encode_net(x)], dim=-1)

    def x_decoder(self, x_emb):
        return self.lC(x_emb)

    def koopman_operation(self, x_emb, u_emb):
        return self.lA(x_emb) + self.lB(u_emb)

    def u_encoder(self, x, u):
        return self.u_encode_net(u)

    def u_decoder(self, u_emb):
        return u_emb

    def encoder_layers(self):
        """[(W [out, in], b [out]) float64 numpy] of x_encode_net, in order."""
        return [(m.weight.detach().double().cpu().numpy(), m.bias.detach().double().cpu().numpy())
                for m in self.x_encode_net if isinstance(m, nn.Linear)]


class KoopmanBlinear(Koopmanlinear):
    """DBKN (``KoopmanBase.py:62-110``): z_{k+1} = lA z + lB u + H vec(z ⊗ u) (``u_z``: vec(u ⊗ z)),
    H: Linear(Nkoopman * u_dim -> Nkoopman), zero-initialised."""

    def __init__(self, x_dim, u_dim, encode_layers, u_z=False):
        super().__init__(x_dim, u_dim, encode_layers)
        self.H = nn.Linear(self.Nkoopman * self.u_dim, self.Nkoopman, bias=False)
        nn.init.zeros_(self.H.weight)
        self.u_z = u_z

    def koopman_operation(self, x_emb, u_emb):
        lin = self.lA(x_emb) + self.lB(u_emb)
        if self.u_z:
            kron = torch.einsum("bi,bj->bij", u_emb, x_emb).reshape(x_emb.shape[0], -1)
        else:
            kron = torch.einsum("bi,bj->bij", x_emb, u_emb).reshape(x_emb.shape[0], -1)
        return lin + self.H(kron)

    def build_permutation_matrix(self, n, m):
        """P with P vec(u ⊗ z) = vec(z ⊗ u) when u_z (identity otherwise), ``:84-95``."""
        if not self.u_z:
            return np.eye(n * m)
        P = np.zeros((n * m, n * m))
        for i in range(n):
            for j in range(m):
                P[j * n + i, i * m + j] = 1
        return P

    def get_Hi_numpy(self):
        """[Ĥ_j (Nkoopman x u_dim) for j < Nkoopman]: H vec(z ⊗ u) = Σ_j z_j Ĥ_j u (``:104-110``)."""
        P = self.build_permutation_matrix(self.u_dim, self.Nkoopman)
        Hd = self.H.weight.detach().double().cpu().numpy() @ P.T
        return [Hd[:, j * self.u_dim:(j + 1) * self.u_dim].copy() for j in range(self.Nkoopman)]


def init_model(args):
    """``models/init_model.py:2-21``: DKUC (linear) or DBKN (bilinear, ``args.u_z``)."""
    if args.model == "DKUC":
        return Koopmanlinear(args.x_dim, args.u_dim, args.layers)
    if args.model == "DBKN":
        return KoopmanBlinear(args.x_dim, args.u_dim, args.layers, bool(getattr(args, "u_z", False)))
    raise ValueError(f"Model {args.model} not implemented!")


def open_loop_prediction(net, x, u, relift=True):
    """Multi-step open-loop prediction of n recorded trajectories, float64 torch on x's device.

    x [N, T+1, x_dim], u [N, >= T, u_dim].  x̂_0 = x_0, z = Psi(x_0); for t < T:
    z ← koopman_operation(z, u_t) (A z + (B + Σ_j z_j Ĥ_j) u_t), x̂_{t+1} = z[:x_dim] (the frozen
    decoder lC = [I | 0]) and, with ``relift``, z ← Psi(x̂_{t+1}).  ``relift=True`` is the
    reference's ``pred_and_eval_loss_old`` (``models/losses.py:132-173``, what ``evaluate()``
    runs, ``train.py:35-87``); ``relift=False`` its ``pred_and_eval_loss_new`` (``:175-215``).
    Returns pred [N, T+1, x_dim].  The literal loop: the cross-check of
    ``MPCController.predict`` (``koopman_predict.hip`` ``k_predict``), which runs it in one launch."""
    if net.lA.weight.dtype != torch.float64:
        raise ValueError("open_loop_prediction runs in float64: call net.double() first (Koopman_MPC.py:263)")
    with torch.no_grad():
        x = torch.as_tensor(x).to(torch.float64)
        u = torch.as_tensor(u).to(device=x.device, dtype=torch.float64)
        xd = net.x_dim
        xh = x[:, 0, :]
        z = net.x_encoder(xh)
        pred = [xh]
        for t in range(x.shape[1] - 1):
            z = net.koopman_operation(z, net.u_encoder(xh, u[:, t, :]))
            xh = z[:, :xd]
            pred.append(xh)
            if relift:
                z = net.x_encoder(xh)
        return torch.stack(pred, dim=1)


def prediction_errors(pred, x, npos=3):
    """The reference's evaluation metrics (``train.py:79-82`` over ``losses.py:158-172``) of a
    prediction pred [N, T+1, x_dim] against x: the mean absolute error over trajectories, the T
    predicted steps and dims -- all of x (``avg_error``), x[:npos] (``dis_error``, the end-effector
    position) and x[npos:] (``angle_error``, the joint angles).  Floats."""
    pred = torch.as_tensor(pred)
    d = (pred[:, 1:, :].double() - torch.as_tensor(x)[:, 1:, :].to(device=pred.device, dtype=torch.float64)).abs()
    return dict(avg_error=float(d.mean()), dis_error=float(d[:, :, :npos].mean()),
                angle_error=float(d[:, :, npos:].mean()))


_TOEPLITZ = {}


def _toeplitz_index(H, device):
    """Index tensors of bilinear_first_move's block sums (cached per H and device)."""
    import torch

    key = (H, str(device))
    if key not in _TOEPLITZ:
        D = 2 * H - 1
        da = np.zeros((D, H), np.int64)
        db = np.zeros((D, H), np.int64)
        dm = np.zeros((D, H))
        for di, d in enumerate(range(-(H - 1), H)):
            for a in range(H):
                b = a - d
                if 0 <= b < H:
                    da[di, a], db[di, a], dm[di, a] = a, b, 1.0
        hd = np.zeros((H, H), np.int64)
        ha = np.zeros((H, H), np.int64)
        for s1 in range(H):
            for s2 in range(H):
                hd[s1, s2] = (s2 - s1) + H - 1
                ha[s1, s2] = H - 1 - s1  # (terms with a < max(0, d) are zero-masked)
        ra = np.zeros((H, H), np.int64)
        rt = np.zeros((H, H), np.int64)
        rm = np.zeros((H, H))
        for s in range(H):
            for j, t in enumerate(range(s, H)):
                ra[s, j], rt[s, j], rm[s, j] = t - s, t, 1.0
        T = lambda x: torch.as_tensor(x, device=device)  # noqa: E731
        _TOEPLITZ[key] = {"da": T(da), "db": T(db), "dm": T(dm).double()[None, :, :, None, None],
                          "hd": T(hd), "ha": T(ha), "ra": T(ra), "rt": T(rt),
                          "rm": T(rm).double()[None, :, :, None]}
    return _TOEPLITZ[key]


def bilinear_first_move(A, B, Hhat, z0, window, u_prev, kind, H, q=50.0, r=0.5):
    """First move u0 of the DBKN MPC for n envs (``MPC_Controler.py:46-141``, state_full), float64
    torch tensors on one device: B_total = B + Σ_j z0_j Ĥ_j per env (the reference's
    linearize_B), then the unconstrained QP of the condensed prediction solved exactly.

    A [nz, nz], B [nz, nu], Hhat [nz(j), nz, nu], z0 [nz, n], window [H, nz, n] (lifted reference
    rows k+1 .. k+H, zero past the end), u_prev [nu, n].  Returns u0 = v*_0 + u_prev [nu, n].

    Block structure (no [H nz, H nu] matrix per env): with M_k = A^k B_total, the prediction's
    input blocks are X_{t-s} (X = M for 'mpc', the running sums C_k = Σ_{i<=k} M_i for
    'delta_mpc'), so Hess[s1, s2] = q Σ_{t >= max(s1, s2)} X_{t-s1}' X_{t-s2} + r I and
    rhs[s] = q Σ_{t >= s} X_{t-s}' e_t with e_t = ref_t - A^{t+1} z0 - c_t u_prev (c_t = C_t for
    'delta_mpc': u_prev held, else 0)."""
    import torch

    nz, nu = B.shape
    n = z0.shape[1]
    Bt = B.unsqueeze(0) + torch.einsum("jn,jrk->nrk", z0, Hhat)           # [n, nz, nu]
    P = [torch.eye(nz, dtype=A.dtype, device=A.device)]
    for _ in range(H):
        P.append(A @ P[-1])
    P = torch.stack(P)                                                   # A^0 .. A^H
    M = torch.einsum("kab,nbc->nkac", P[:H], Bt)                         # [n, H, nz, nu]
    C = torch.cumsum(M, dim=1)
    if kind == "delta_mpc":
        X, cu = C, C
    elif kind == "mpc":
        X, cu = M, None
    else:
        raise ValueError(f"MPC_type {kind!r}: 'mpc' or 'delta_mpc'")
    idx = _toeplitz_index(H, A.device)
    W = torch.einsum("nkab,nlac->nklbc", X, X)                           # X_k' X_l [n, H, H, nu, nu]
    # Hess[s1, s2] = q Σ_{t >= max(s1, s2)} W[t - s1, t - s2]: running sums along each diagonal
    # d = s2 - s1 of W (a = t - s1 runs from max(0, d) to H - 1 - s1), gathered per block
    Wd = W[:, idx["da"], idx["db"]] * idx["dm"]                          # [n, 2H-1, H, nu, nu]
    Sd = torch.cumsum(Wd, dim=2)
    Hs = q * Sd[:, idx["hd"], idx["ha"]]                                 # [n, H, H, nu, nu] (s1, s2)
    Hs = Hs.permute(0, 1, 3, 2, 4).reshape(n, H * nu, H * nu)
    Hs = Hs + r * torch.eye(H * nu, dtype=A.dtype, device=A.device)
    Az = torch.einsum("tab,bn->nta", P[1:H + 1], z0)                    # A^{t+1} z0 [n, H, nz]
    e = window.permute(2, 0, 1) - Az                                     # [n, H, nz]
    if cu is not None:
        e = e - torch.einsum("ntab,bn->nta", cu, u_prev)
    # rhs[s] = q Σ_{t >= s} X_{t-s}' e_t
    Y = torch.einsum("nkab,nta->nktb", X, e)                             # X_k' e_t [n, H(k), H(t), nu]
    rhs = q * (Y[:, idx["ra"], idx["rt"]] * idx["rm"]).sum(2)            # [n, H(s), nu]
    rhs = rhs.reshape(n, H * nu)
    L = torch.linalg.cholesky(Hs)
    v = torch.cholesky_solve(rhs.unsqueeze(-1), L)[..., 0]
    return v[:, :nu].T + u_prev


def _powers(A, H):
    """[I, A, A^2, ..., A^H]."""
    P = [np.eye(A.shape[0])]
    for _ in range(H):
        P.append(A @ P[-1])
    return P


def _prediction(A, B, H):
    """The stacked prediction Z = Phi z0 + Gam U over t = 0..H-1: (A's powers [I .. A^H],
    Phi = [A; A^2; ...; A^H], Gam[t, s] = A^(t-s) B for s <= t)."""
    nz, nu = B.shape
    P = _powers(A, H)
    Phi = np.vstack(P[1:])
    Gam = np.zeros((H * nz, H * nu))
    for t in range(H):
        for s in range(t + 1):
            Gam[t * nz:(t + 1) * nz, s * nu:(s + 1) * nu] = P[t - s] @ B
    return P, Phi, Gam


def _move_penalty(kind, H, nu):
    """The input term's matrix of the constrained steps, in the model inputs w: D'D ('delta_mpc': D the
    block first difference) or I ('mpc')."""
    if kind == "delta_mpc":
        D = np.kron(np.eye(H) - np.eye(H, k=-1), np.eye(nu))
        return D.T @ D
    if kind == "mpc":
        return np.eye(H * nu)
    raise ValueError(f"MPC_type {kind!r}: 'mpc' or 'delta_mpc'")


def condensed_gains(A, B, H, kind, q=50.0, r=0.5):
    """Closed-form first move of the unconstrained MPC QP (MPC_Controler.py:65-141, state_full).

    Stacked prediction over t = 0..H-1:  Z = Phi z0 + Gamma U,  Phi = [A; A^2; ...; A^H],
    Gamma[t, s] = A^(t-s) B (s <= t).  'mpc': U are the inputs; 'delta_mpc': U = u_prev 1 + S dU
    with S the block lower-triangular identity.  Minimising
    (Z - Rbar)' (q I) (Z - Rbar) + V' (r I) V  (V = U or dU) gives V* = K (Rbar - Phi z0 - c u_prev)
    and the applied input u0 = V*_0 + u_prev (get_control, :147).  Returns (Gr [nu, H nz],
    Gz [nu, nz], Gu [nu, nu]) with u0 = Gr Rbar + Gz z0 + Gu u_prev."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    nz, nu = B.shape
    _, Phi, Gam = _prediction(A, B, H)
    if kind == "delta_mpc":
        S = np.kron(np.tril(np.ones((H, H))), np.eye(nu))
        Gd = Gam @ S
        cu = Gam @ np.kron(np.ones((H, 1)), np.eye(nu))  # response to u_prev held
    elif kind == "mpc":
        Gd = Gam
        cu = np.zeros((H * nz, nu))
    else:
        raise ValueError(f"MPC_type {kind!r}: 'mpc' or 'delta_mpc'")
    Hs = q * Gd.T @ Gd + r * np.eye(H * nu)
    K = np.linalg.solve(Hs, q * Gd.T)[:nu]  # first move only
    Gr = K
    Gz = -K @ Phi
    Gu = np.eye(nu) - K @ cu
    return Gr, Gz, Gu


# ------------------------------------------------------------------ input-constrained MPC (DKUC)
BOX_ALPHA = 1.6  # ADMM over-relaxation of the constrained step (csrc/koopman_box.hip uses the same)


def box_problem(A, B, H, kind, q=50.0, r=0.5):
    """The horizon QP of the DKUC controller in the model inputs w (N = H nu), for the step with
    input limits (``sim_koopman_box_step``): the reference's cost (``MPC_Controler.py:80-86`` /
    ``:115-127``, state_full) is  1/2 w' P w - g' w + const  with

      'delta_mpc'  w_t = u_prev + sum_{i<=t} du_i (the inputs the model is driven with; u0 = w_0)
      'mpc'        w_t = v_t (u0 = v_0 + u_prev)

    Z = Phi z0 + Gam w for both kinds (Gam[t, s] = A^(t-s) B), the move penalty is r |D w - E0 u_prev|^2
    (D the block first difference) for 'delta_mpc' and r |w|^2 for 'mpc', so
    P = 2 (q Gam' Gam + r D'D | r I) depends on the model only and g = Gw rbar + Gz z0 + Gu u_prev
    (rbar the H lifted reference rows stacked).  Returns a dict: P, Lhat = ||P||_inf, mu / lmax (P's
    extreme eigenvalues), rho = sqrt(mu lmax) and Mrho = rho (P + rho I)^-1 (the ADMM step of
    :func:`box_plan`), Gw [N, H nz], Gz [N, nz], Gu [N, nu], Kw / Kz / Ku = P^-1 of those (the
    unconstrained minimiser's gains) and `shift`: 1 when block 0's bounds are shifted by -u_prev
    ('mpc': the limit is on what is applied, v_0 + u_prev), else 0."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    nz, nu = B.shape
    N = H * nu
    _, Phi, Gam = _prediction(A, B, H)
    Rm = _move_penalty(kind, H, nu)
    Gu = np.zeros((N, nu))
    if kind == "delta_mpc":
        Gu[:nu] = 2.0 * r * np.eye(nu)
    P = 2.0 * (q * Gam.T @ Gam + r * Rm)
    P = 0.5 * (P + P.T)
    Gw = 2.0 * q * Gam.T
    Gz = -Gw @ Phi
    ev = np.linalg.eigvalsh(P)
    mu, lmax = float(ev[0]), float(ev[-1])
    rho = float(np.sqrt(mu * lmax))
    Kall = np.linalg.solve(P, np.hstack([Gw, Gz, Gu]))
    return dict(P=P, Lhat=float(np.abs(P).sum(1).max()), mu=mu, lmax=lmax, rho=rho,
                Mrho=rho * np.linalg.inv(P + rho * np.eye(N)), Gw=Gw, Gz=Gz, Gu=Gu,
                Kw=Kall[:, :H * nz], Kz=Kall[:, H * nz:H * nz + nz], Ku=Kall[:, H * nz + nz:],
                shift=int(kind == "mpc"), nu=nu, H=H, N=N, kind=kind)


def box_bounds(prob, u_prev, u_max):
    """(lo, hi) [n, N] of :func:`box_problem`'s variables for u_prev [n, nu]."""
    u_prev = np.atleast_2d(np.asarray(u_prev, np.float64))
    lo = np.full((u_prev.shape[0], prob["N"]), -float(u_max))
    hi = -lo
    if prob["shift"]:
        lo[:, :prob["nu"]] -= u_prev
        hi[:, :prob["nu"]] -= u_prev
    return lo, hi


def box_plan(prob, z0, window, u_prev, u_max=0.5, tol=1e-9, max_iter=256, plan=None):
    """The constrained control step in float64 numpy: what ``sim_koopman_box_step`` computes, by the
    same iteration, for n envs.  z0 [n, nz], window [n, H, nz] (lifted reference rows, zero past the
    end), u_prev [n, nu], plan [n, N] or None (a warm start).  Returns (w [n, N], u0 [n, nu],
    ok [n] int32, iters [n] int32).

    Contract: with res(w) = w - clip(w - (P w - g) / Lhat, lo, hi), an env is done (ok = 1, iters =
    the iterations it took) when ||res(w)||_inf <= tol; one that reaches max_iter returns its last
    iterate (every iterate is a projection: inside the box) with ok = 0.  An env whose unconstrained
    minimiser wu = P^-1 g lies in the box returns it with iters = 0, warm start or not.

    Iteration (ADMM on  min 1/2 x'Px - g'x + I_box(z), x = z, scaled dual y, over-relaxed):
      start  z = clip(wu), or clip(plan) where res(clip(plan)) < res(clip(wu)) mu / (4 Lhat) (or <= tol): the natural
             residual bounds the distance to the solution from both sides, res / 2 <= ||z - z*|| <=
             2 (Lhat / mu) res, so the plan is taken exactly when it is provably the closer start (the
             iteration's own cold start is a good one: a plan merely near the solution does not beat it);
             y = -(P z - g) / rho where z sits on a bound the gradient pushes
             against, else 0 (the multiplier estimate of the start: a solution is a fixed point)
      x = wu + Mrho (z - y - wu)      (= (P + rho I)^-1 (g + rho (z - y)));  xh = alpha x + (1 - alpha) z
      z <- clip(xh + y);  y <- y + xh - z
    and P z - g = P (z - wu): g itself is never formed."""
    P, N = prob["P"], prob["N"]
    z0 = np.atleast_2d(np.asarray(z0, np.float64))
    n = z0.shape[0]
    u_prev = np.atleast_2d(np.asarray(u_prev, np.float64)).reshape(n, -1)
    s = np.hstack([np.asarray(window, np.float64).reshape(n, -1), z0, u_prev])
    wu = s @ np.hstack([prob["Kw"], prob["Kz"], prob["Ku"]]).T
    lo, hi = box_bounds(prob, u_prev, u_max)
    invL, rho, alpha = 1.0 / prob["Lhat"], prob["rho"], BOX_ALPHA
    zc = np.clip(wu, lo, hi)
    interior = (zc == wu).all(1)

    def resid(z):
        grad = (z - wu) @ P.T
        return grad, np.abs(z - np.clip(z - grad * invL, lo, hi)).max(1)

    z = zc
    grad, rr = resid(z)
    if plan is not None:  # the plan is the start where it is provably the closer one (see above)
        zp = np.clip(np.asarray(plan, np.float64).reshape(n, N), lo, hi)
        gp, rp = resid(zp)
        take = ((rp <= tol) | (rp < rr * (prob["mu"] / (4.0 * prob["Lhat"])))) & ~interior
        z, grad, rr = np.where(take[:, None], zp, z), np.where(take[:, None], gp, grad), np.where(take, rp, rr)
    done = rr <= tol
    iters = np.zeros(n, np.int32)
    y = np.where(((z <= lo) & (grad > 0)) | ((z >= hi) & (grad < 0)), -grad / rho, 0.0)
    for it in range(1, int(max_iter) + 1):
        if done.all():
            break
        x = wu + (z - y - wu) @ prob["Mrho"].T
        xh = alpha * x + (1.0 - alpha) * z
        zn = np.clip(xh + y, lo, hi)
        yn = y + xh - zn
        live = ~done
        z = np.where(live[:, None], zn, z)
        y = np.where(live[:, None], yn, y)
        grad, rr = resid(z)
        new = live & (rr <= tol)
        iters[new] = it
        done |= new
    iters[~done] = int(max_iter)
    u0 = z[:, :prob["nu"]] + (u_prev if prob["shift"] else 0.0)
    if prob["shift"]:
        u0 = np.clip(u0, -float(u_max), float(u_max))
    return z, u0, done.astype(np.int32), iters


# ------------------------------------------------------------------ input-constrained MPC (DBKN)
def box_plan_bilinear(A, B, Hhat, z0, window, u_prev, kind, H, u_max=0.5, tol=1e-9, max_iter=128, q=50.0, r=0.5):
    """The constrained DBKN control step in float64 numpy: what ``sim_koopman_bilinear_box_step``
    computes (``koopman_bilinear.hip`` ``k_bilinear_box``), by the same iteration, for n envs.  A [nz, nz],
    B [nz, nu], Hhat [nz(j), nz, nu], z0 [n, nz], window [n, H, nz] (lifted reference rows, zero past the
    end), u_prev [n, nu].  Returns (w [n, N] the model inputs in natural order, u0 [n, nu], ok [n] int32,
    iters [n] int32).

    Per env, with B_total = B + Σ_j z0_j Ĥ_j and Gam[t, s] = A^(t-s) B_total, the problem of
    :func:`box_problem` in the kernel's scale (half of it):  min 1/2 w'P w - g'w,  lo <= w <= hi,
    P = q Gam'Gam + r (D'D | I),  g = q Gam'(rbar - Phi z0) + r u_prev on block 0 ('delta_mpc').

    Iteration: projected Gauss-Seidel from w = clip(0) with the gradient gr = P w - g maintained; a sweep
    visits the entries in the kernel's lane order -- the time blocks from the last to the first, the
    inputs of a block in order -- and step i does  wn = clip(w_i - gr_i / P_ii), gr += P[:, i] (wn - w_i),
    w_i = wn.  Stop test after every sweep: res = w - clip(w - gr / Lhat, lo, hi), Lhat = ||P||_inf of
    the env, done when ||res||_inf <= tol: ok = 1, iters = the sweeps it took (>= 1: there is no
    factorisation, so an env whose unconstrained minimiser is interior is iterated too).  At max_iter:
    ok = 0, iters = max_iter, the last iterate (every entry a projection: inside the box)."""
    if kind not in ("mpc", "delta_mpc"):
        raise ValueError(f"MPC_type {kind!r}: 'mpc' or 'delta_mpc'")
    A, B, Hhat = np.asarray(A, np.float64), np.asarray(B, np.float64), np.asarray(Hhat, np.float64)
    nz, nu = B.shape
    N = H * nu
    z0 = np.atleast_2d(np.asarray(z0, np.float64))
    n = z0.shape[0]
    u_prev = np.atleast_2d(np.asarray(u_prev, np.float64)).reshape(n, nu)
    rbar = np.asarray(window, np.float64).reshape(n, H, nz)
    Bt = B[None] + np.einsum("nj,jik->nik", z0, Hhat)                      # [n, nz, nu]
    Pw = _powers(A, H)
    Mk = np.stack([Pw[k] @ Bt for k in range(H)], 1)                        # A^k B_total [n, H, nz, nu]
    Gam = np.zeros((n, H, nz, H, nu))
    for t in range(H):
        for s in range(t + 1):
            Gam[:, t, :, s, :] = Mk[:, t - s]
    Gam = Gam.reshape(n, H * nz, N)
    e = rbar - np.stack([z0 @ Pw[t + 1].T for t in range(H)], 1)            # ref_t - A^(t+1) z0
    g = q * np.einsum("nka,nk->na", Gam, e.reshape(n, H * nz))
    Rm = _move_penalty(kind, H, nu)
    if kind == "delta_mpc":
        g[:, :nu] += r * u_prev
    P = q * np.einsum("nka,nkb->nab", Gam, Gam) + r * Rm[None]
    P = 0.5 * (P + P.transpose(0, 2, 1))
    lo = np.full((n, N), -float(u_max))
    hi = -lo
    if kind == "mpc":
        lo[:, :nu] -= u_prev
        hi[:, :nu] -= u_prev
    order = [(H - 1 - a // nu) * nu + a % nu for a in range(N)]             # lane a -> natural index
    idg = 1.0 / np.einsum("nii->ni", P)
    ilh = 1.0 / np.abs(P).sum(2).max(1)
    w = np.clip(np.zeros((n, N)), lo, hi)
    gr = np.einsum("nab,nb->na", P, w) - g
    live = np.ones(n, bool)
    iters = np.zeros(n, np.int32)
    for it in range(1, int(max_iter) + 1):
        for i in order:
            wn = np.clip(w[:, i] - gr[:, i] * idg[:, i], lo[:, i], hi[:, i])
            d = np.where(live, wn - w[:, i], 0.0)
            w[:, i] = np.where(live, wn, w[:, i])
            gr += P[:, :, i] * d[:, None]
        res = np.abs(w - np.clip(w - gr * ilh[:, None], lo, hi)).max(1)
        new = live & (res <= tol)
        iters[new] = it
        live &= ~new
        if not live.any():
            break
    iters[live] = int(max_iter)
    u0 = w[:, :nu].copy()
    if kind == "mpc":
        u0 = np.clip(u0 + u_prev, -float(u_max), float(u_max))
    return w, u0, (~live).astype(np.int32), iters
