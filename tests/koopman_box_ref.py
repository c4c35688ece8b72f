"""The float64 reference of the constrained DKUC control step (sim_koopman_box_step) and the frozen
inputs of tests/test_koopman_box.py.  Not collected: it holds no test.

The reference uses no project code.  The problem is the oracle's own quadratic
(oracle/koopman_mpc.py: prepare -- the Hessian Hs and the affine pieces of the reference's cost loop
in its decision vector v) mapped to the model inputs w:

    'delta_mpc'  v = du,  w_t = u_prev + sum_{i<=t} du_i:  v = D w - E0 u_prev  (D the block first
                 difference, E0 u_prev = [u_prev; 0; ..])
    'mpc'        v = w (D = I, E0 = 0)

so J = 1/2 v'Hs v + go'v + c becomes 1/2 w'Pw - g'w with P = D'Hs D and g = D'(Hs E0 u_prev - go), go
the gradient at v = 0 exactly as KO.solve forms it.  Bounds: |w| <= u_max, and for 'mpc' block 0 is
shifted by -u_prev (|v_0 + u_prev| <= u_max: what is applied).  It is solved by projected Gauss-Seidel
to ||res||_inf <= 1e-14, res(w) = w - clip(w - (Pw - g) / Lhat, lo, hi), Lhat = ||P||_inf.

Inputs: per row, 130 envs (several workgroups of 64; n = 1 and n = 17 are its leading envs), states and
reference windows from koopman_shapes_ref.states scaled per env by SCALE[row] x {1/2, 1, 2} (drawn; nz3:
FREE_NOISE below),
u_prev uniform in +-0.4.  SCALE was picked per row, from the reference alone, so that both kinds meet
test_inputs_exercise_the_bounds: >= 25% of envs with a bound active on the first move, >= 10% with
none at all, and at least one with a bound active only at some t >= 1.
"""
import functools

import numpy as np

import koopman_mpc as KO
import koopman_shapes_ref as S

BOX_ROWS = ("ref", "odd", "tiny", "nz64", "nz3")
U_MAX, TOL = 0.5, 1e-9
N_ENV = 130
SIZES = (1, 17, N_ENV)
FLOOR = 1e-11  # the float64 floor of the shape tests
SCALE = {"ref": 1.2, "odd": 2.0, "tiny": 4.0, "nz64": 1.8, "nz3": 0.35}
# nz3's encoder [2, 1, 1] has one feature, dominated by its bias: z0 and the lifted reference differ by
# a constant that no input scale moves, and every env saturates.  Its window is instead the model's
# free response A^(t+1) z0 plus FREE_NOISE["nz3"] x the per-env amplitude x unit Gaussian noise.
FREE_NOISE = {"nz3": 0.4}
ALPHA = 1.6    # the over-relaxation of the kernel's ADMM (first_iterate restates one iteration)


@functools.lru_cache(maxsize=None)
def quadratic(name, kind):
    """P, Lhat, mu, lmax and the oracle pieces (qp, Hs, D) of a row's QP in w."""
    row = S.ROWS[name]
    xd, nu, nz, H = S.dims(row)
    A, B, _ = S.mats(S.make_net(name))
    qp = KO.prepare(A, B, H, kind)
    Hs = qp[5]
    N = H * nu
    D = np.kron(np.eye(H) - np.eye(H, k=-1), np.eye(nu)) if kind == "delta_mpc" else np.eye(N)
    P = D.T @ Hs @ D
    P = 0.5 * (P + P.T)
    ev = np.linalg.eigvalsh(P)
    return S._freeze(dict(A=A, B=B, H=H, nu=nu, nz=nz, N=N, kind=kind, qp=qp, Hs=Hs, D=D, P=P,
                          Lhat=float(np.abs(P).sum(1).max()), mu=float(ev[0]), lmax=float(ev[-1])))


def linear_term(Q, z0, ref, up):
    """g [n, N] of 1/2 w'Pw - g'w for z0 [n, nz], ref [n, H, nz], up [n, nu]."""
    n = z0.shape[0]
    go = np.zeros((n, Q["N"]))
    for t, (Mz, Pz, Pu) in enumerate(Q["qp"][6]):
        go += 2 * Q["qp"][4] * (z0 @ Pz.T + up @ Pu.T - ref[:, t]) @ Mz   # as KO.solve
    e0 = np.zeros((n, Q["N"]))
    if Q["kind"] == "delta_mpc":
        e0[:, :Q["nu"]] = up
    return (e0 @ Q["Hs"] - go) @ Q["D"]


def bounds(Q, up, u_max=U_MAX):
    lo = np.full((up.shape[0], Q["N"]), -float(u_max))
    hi = -lo
    if Q["kind"] == "mpc":
        lo[:, :Q["nu"]] -= up
        hi[:, :Q["nu"]] -= up
    return lo, hi


def residual(Q, w, g, lo, hi):
    """||w - clip(w - (Pw - g) / Lhat, lo, hi)||_inf per env."""
    return np.abs(w - np.clip(w - (w @ Q["P"] - g) / Q["Lhat"], lo, hi)).max(1)


def to_v(Q, w, up):
    """The oracle's decision vector of the model inputs w (D w - E0 u_prev)."""
    v = w @ Q["D"].T
    if Q["kind"] == "delta_mpc":
        v[:, :Q["nu"]] -= up
    return v


def applied(Q, w, up, u_max=U_MAX):
    """u0: w_0, or v_0 + u_prev for 'mpc' (clipped: the sum may round one ulp past the limit)."""
    u0 = w[:, :Q["nu"]]
    return u0.copy() if Q["kind"] == "delta_mpc" else np.clip(u0 + up, -u_max, u_max)


def pgs(Q, g, lo, hi, stop=1e-14, max_sweeps=20000):
    """Projected Gauss-Seidel from clip(0) for every env at once; asserts the stop test is met."""
    P = Q["P"]
    w = np.clip(np.zeros_like(g), lo, hi)
    dg = np.diag(P).copy()
    for _ in range(max_sweeps):
        for i in range(P.shape[0]):
            w[:, i] = np.clip((g[:, i] - w @ P[i] + dg[i] * w[:, i]) / dg[i], lo[:, i], hi[:, i])
        if residual(Q, w, g, lo, hi).max() <= stop:
            return w
    raise AssertionError(f"the reference did not reach {stop}: {residual(Q, w, g, lo, hi).max():.2e}")


def solve(name, kind, z0, ref, up, u_max=U_MAX):
    """The reference's (w, u0) for given inputs."""
    Q = quadratic(name, kind)
    lo, hi = bounds(Q, up, u_max)
    w = pgs(Q, linear_term(Q, z0, ref, up), lo, hi)
    return w, applied(Q, w, up, u_max)


def error_bound(Q, tol=TOL):
    """||w - w*||_2 <= 2 (Lhat / mu) sqrt(N) tol + 1e-11: the error bound of the natural residual for a
    mu-strongly-convex, L-smooth problem with step 1 / Lhat <= 1 / L, and the float64 floor."""
    return 2.0 * (Q["Lhat"] / Q["mu"]) * np.sqrt(Q["N"]) * tol + FLOOR


@functools.lru_cache(maxsize=None)
def inputs(name):
    """x [130, xd] float32, z0, ref [130, H, nz], up [130, nu]; the same for both kinds."""
    row = S.ROWS[name]
    xd, nu, nz, H = S.dims(row)
    _, _, layers = S.mats(S.make_net(name))
    rng = S._rng(row, 21)
    amp = SCALE[name] * rng.choice([0.5, 1.0, 2.0], N_ENV)
    x = (amp[:, None] * S.states(rng, N_ENV, xd)).astype(np.float32)
    z0 = KO.encode(layers, x.astype(np.float64))
    ref = KO.encode(layers, np.repeat(amp, H)[:, None] * S.states(rng, N_ENV * H, xd)).reshape(N_ENV, H, nz)
    if name in FREE_NOISE:
        A = S.mats(S.make_net(name))[0]
        zt = z0
        for t in range(H):
            zt = zt @ A.T
            ref[:, t] = zt + FREE_NOISE[name] * amp[:, None] * rng.normal(0.0, 1.0, (N_ENV, nz))
    up = rng.uniform(-0.4, 0.4, (N_ENV, nu))
    return S._freeze(dict(x=x, z0=z0, ref=ref, up=up))


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """The inputs of a row with the reference's answer: g, lo, hi, w, u0, the unconstrained minimiser
    wu (KO.solve mapped to w) and the active sets."""
    Q = quadratic(name, kind)
    c = dict(inputs(name))
    z0, ref, up = c["z0"], c["ref"], c["up"]
    g = linear_term(Q, z0, ref, up)
    lo, hi = bounds(Q, up)
    w = pgs(Q, g, lo, hi)
    v = KO.solve(Q["A"], Q["B"], z0, ref, up, kind, Q["H"], qp=Q["qp"]).reshape(N_ENV, -1)
    wu = from_v(Q, v, up)
    act = (w <= lo) | (w >= hi)
    c.update(g=g, lo=lo, hi=hi, w=w, u0=applied(Q, w, up), wu=wu, act=act,
             act0=act[:, :Q["nu"]].any(1), act_any=act.any(1))
    return S._freeze(c)


def from_v(Q, v, up):
    """Model inputs w of the oracle's decision vector v (the inverse of to_v)."""
    v = v.copy()
    if Q["kind"] == "delta_mpc":
        v[:, :Q["nu"]] += up
        return np.cumsum(v.reshape(v.shape[0], Q["H"], Q["nu"]), 1).reshape(v.shape[0], -1)
    return v


def first_iterate(Q, wu, lo, hi, tol=TOL):
    """What max_iter = 1 can reach: the residual of the cold start clip(wu) and of the kernel's first
    ADMM iterate from it (its iteration restated on the oracle's P: rho = sqrt(mu lmax), multiplier
    estimate y = -grad / rho on the bounds the gradient pushes against, over-relaxation ALPHA).
    Returns (r0, r1) per env."""
    P, N = Q["P"], Q["N"]
    rho = np.sqrt(Q["mu"] * Q["lmax"])
    z = np.clip(wu, lo, hi)
    grad = (z - wu) @ P
    r0 = np.abs(z - np.clip(z - grad / Q["Lhat"], lo, hi)).max(1)
    y = np.where(((z <= lo) & (grad > 0)) | ((z >= hi) & (grad < 0)), -grad / rho, 0.0)
    x = wu + (z - y - wu) @ (rho * np.linalg.inv(P + rho * np.eye(N))).T
    xh = ALPHA * x + (1 - ALPHA) * z
    z1 = np.clip(xh + y, lo, hi)
    grad = (z1 - wu) @ P
    r1 = np.abs(z1 - np.clip(z1 - grad / Q["Lhat"], lo, hi)).max(1)
    return r0, r1
