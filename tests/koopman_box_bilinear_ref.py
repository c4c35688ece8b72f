"""The float64 reference of the constrained DBKN control step (sim_koopman_bilinear_box_step) and the
frozen inputs of tests/test_koopman_box_bilinear.py.  Not collected: it holds no test.

The reference uses no project code.  Per env e the input matrix is the oracle's linearisation
Bt = KO.b_total(B, Hhat, z0[e]) and the problem is the oracle's own quadratic for (A, Bt)
(KO.prepare), mapped to the model inputs w exactly as tests/koopman_box_ref.py maps the DKUC one:
P_e = D'Hs_e D, g_e from its linear_term, the bounds from its bounds, and per env Lhat_e = ||P_e||_inf
and mu_e = lambda_min(P_e).  It is solved to ||res||_inf <= 1e-14 by that file's projected Gauss-Seidel
-- `pgs` below is koopman_box_ref.pgs with a matrix per env, all envs at once (the same start clip(0),
the same update, entry by entry in natural order; test_batched_pgs_is_the_box_refs_pgs holds the two to
each other on single envs).

Inputs: koopman_box_ref.inputs(row) -- 130 envs, n = 1 and n = 17 its leading envs -- on the DBKN nets
koopman_shapes_ref.make_net(row, "DBKN", u_z).  The step takes z0 and the window as given, so the
inputs' lifted states are used as they are.  Rows: ref with both Kronecker orders (the static
instantiation), odd (N 21, nz 29), nz64 (N 64, u_dim 8, 2 envs per workgroup), tiny (H 20, u_dim 1) and
nz3 (N 6).  koopman_box_ref.SCALE meets test_inputs_exercise_the_bounds on every one of them, so no
row's scale is changed here.
"""
import functools

import numpy as np

import koopman_box_ref as R
import koopman_mpc as KO
import koopman_shapes_ref as S

ROWS = (("ref", False), ("ref", True), ("odd", False), ("nz64", False), ("tiny", False), ("nz3", False))
CASES = [(name, u_z, kind) for name, u_z in ROWS for kind in S.KINDS]
IDS = [f"{name}{'-uz' if u_z else ''}-{kind}" for name, u_z, kind in CASES]
U_MAX, TOL, N_ENV, SIZES = R.U_MAX, R.TOL, R.N_ENV, R.SIZES


def model(name, u_z):
    """(A, B, Hhat [nz (j), nz, nu]) of the row's DBKN net, float64, C-contiguous."""
    net = S.make_net(name, "DBKN", u_z)
    A, B, _ = S.mats(net)
    return np.ascontiguousarray(A), np.ascontiguousarray(B), np.ascontiguousarray(np.stack(net.get_Hi_numpy()), np.float64)


def residual(P, Lhat, w, g, lo, hi):
    """||w - clip(w - (P_e w - g) / Lhat_e, lo, hi)||_inf per env."""
    grad = np.einsum("nab,nb->na", P, w) - g
    return np.abs(w - np.clip(w - grad / Lhat[:, None], lo, hi)).max(1)


def pgs(P, Lhat, g, lo, hi, stop=1e-14, max_sweeps=20000):
    """koopman_box_ref.pgs with P [n, N, N] per env: projected Gauss-Seidel from clip(0)."""
    w = np.clip(np.zeros_like(g), lo, hi)
    dg = np.einsum("nii->ni", P).copy()
    for _ in range(max_sweeps):
        for i in range(P.shape[1]):
            w[:, i] = np.clip((g[:, i] - (w * P[:, i]).sum(1) + dg[:, i] * w[:, i]) / dg[:, i], lo[:, i], hi[:, i])
        if residual(P, Lhat, w, g, lo, hi).max() <= stop:
            return w
    raise AssertionError(f"the reference did not reach {stop}: {residual(P, Lhat, w, g, lo, hi).max():.2e}")


def env_quadratic(A, B, Hhat, z0e, H, kind):
    """koopman_box_ref.quadratic's dict for ONE env: the oracle's quadratic at Bt = b_total(z0e)."""
    nz, nu = B.shape
    N = H * nu
    Bt = KO.b_total(B, Hhat, z0e)
    qp = KO.prepare(A, Bt, H, kind)
    Hs = qp[5]
    D = np.kron(np.eye(H) - np.eye(H, k=-1), np.eye(nu)) if kind == "delta_mpc" else np.eye(N)
    P = D.T @ Hs @ D
    P = 0.5 * (P + P.T)
    return dict(A=A, B=Bt, H=H, nu=nu, nz=nz, N=N, kind=kind, qp=qp, Hs=Hs, D=D, P=P,
                Lhat=float(np.abs(P).sum(1).max()), mu=float(np.linalg.eigvalsh(P)[0]))


def problem(A, B, Hhat, z0, ref, up, H, kind, u_max=U_MAX):
    """P [n, N, N], Lhat [n], mu [n], g, lo, hi [n, N] of the n envs' problems."""
    n = z0.shape[0]
    Qs = [env_quadratic(A, B, Hhat, z0[e], H, kind) for e in range(n)]
    g = np.stack([R.linear_term(Qs[e], z0[e:e + 1], ref[e:e + 1], up[e:e + 1])[0] for e in range(n)])
    lo, hi = R.bounds(Qs[0], up, u_max)
    return (np.stack([q["P"] for q in Qs]), np.array([q["Lhat"] for q in Qs]), np.array([q["mu"] for q in Qs]),
            g, lo, hi)


def solve(A, B, Hhat, z0, ref, up, H, kind, u_max=U_MAX):
    """The reference's (w, u0, bound [n]) for given inputs."""
    P, Lhat, mu, g, lo, hi = problem(A, B, Hhat, z0, ref, up, H, kind, u_max)
    w = pgs(P, Lhat, g, lo, hi)
    Q0 = dict(kind=kind, nu=B.shape[1], N=H * B.shape[1])
    return w, R.applied(Q0, w, up, u_max), error_bound(Lhat, mu, Q0["N"])


def error_bound(Lhat, mu, N, tol=TOL):
    """koopman_box_ref.error_bound per env: 2 (Lhat_e / mu_e) sqrt(N) tol + 1e-11."""
    return 2.0 * (Lhat / mu) * np.sqrt(N) * tol + R.FLOOR


@functools.lru_cache(maxsize=None)
def case(name, u_z, kind):
    """The inputs of a row with the reference's answer: P, Lhat, mu, g, lo, hi, w, u0, the unconstrained
    minimiser wu, the per-env error bound and the active sets."""
    row = S.ROWS[name]
    _, nu, nz, H = S.dims(row)
    A, B, Hhat = model(name, u_z)
    c = dict(R.inputs(name))
    z0, ref, up = c["z0"], c["ref"], c["up"]
    P, Lhat, mu, g, lo, hi = problem(A, B, Hhat, z0, ref, up, H, kind)
    w = pgs(P, Lhat, g, lo, hi)
    Q0 = dict(kind=kind, nu=nu, N=H * nu)
    act = (w <= lo) | (w >= hi)
    c.update(A=A, B=B, Hhat=Hhat, H=H, nu=nu, nz=nz, N=H * nu, kind=kind, P=P, Lhat=Lhat, mu=mu, g=g, lo=lo, hi=hi,
             w=w, u0=R.applied(Q0, w, up), wu=np.linalg.solve(P, g[:, :, None])[:, :, 0], bound=error_bound(Lhat, mu, H * nu),
             grad=np.einsum("nab,nb->na", P, w) - g, act=act, act0=act[:, :nu].any(1), act_any=act.any(1))
    return S._freeze(c)
