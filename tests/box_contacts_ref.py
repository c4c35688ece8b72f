"""Shared checks of the two narrowphases that emit more than one contact per pair: box_box
(table - cube) and plane_box (floor - cube), soarm_collide.h, and of the 2-bit count word that
carries their contact count from k_collide to the constraint solve (soarm_pgs.h).

Every other device test leaves the cube where conftest.cube_qpos puts it: identity orientation,
flat on the table, 35 cm from the nearest table edge -- box_box's fast path with 4 corners and
count word 3 of the table pair, nothing else.  The poses here (seeded, fp32-rounded, N envs per
regime, REGIMES) tilt the cube, push it over the table's edge and corner, lean it on the rim, the
top corner and the side face, and drop it on the floor.

Two references, both float64: the C oracle (Oracle.forward, Oracle.step), and the plain numpy of
this module (plane_box_ref, sat), which shares no code with the oracle or the kernel.

Every check takes `make_sim(cm, n)`; tests/test_box_contacts.py runs them on the library's CPU
backend without a GPU and, marked `gpu`, on the device.
"""
import functools

import numpy as np

from oracle import Oracle
from contact_overflow_ref import GRAZING, QVEL_BARS, assert_same_bits, rows, snapshot, to_np

N = 96                        # envs per regime
H = 0.015                     # the cube's half size
TABLE_H = np.array([0.61, 0.37, 0.1])
TABLE_C = np.array([0.0, 0.0, -0.1009])
TOP, FLOOR = -0.0009, -0.75   # the table top's and the floor's z
# one fp32 ulp of a coordinate of at most 1 m is 1.2e-7, and a contact is a few dozen operations
# from qpos: 5e-6 m for distance and position, 1e-5 for the (unit) normal
BAR, NBAR = 5e-6, 1e-5
LEAVE_OUT = 0.03              # of a regime (test_gpu_parity.test_contacts_match_oracle's cap)
REGIMES = ("tilt", "small_tilt", "edge", "corner", "rim", "vertex", "side", "floor", "floor_small_tilt")
SEED = {r: 100 + i for i, r in enumerate(REGIMES)}
# (regime, ccd) of the contact checks: every regime under MPR, and two under the native GJK/EPA
# (the primitive narrowphases must not depend on the convex-convex template argument)
CONTACT_CASES = [(r, "mpr") for r in REGIMES] + [("edge", "native"), ("small_tilt", "native")]


@functools.lru_cache(maxsize=None)
def model(solver="PGS", ccd="mpr"):
    from lerobot_mujoco_sim2real_amd import mjcf
    return mjcf.compile_mjcf(mjcf.CUBE_SCENE_XML, solver=solver, ccd=ccd)


def geoms(cm):
    g = cm.geom_names
    return g.index("floor"), g.index("table"), g.index("cube")


# ----------------------------------------------------------------------------------------- the poses
def quat_mat(q):
    """Rotation matrices [n, 3, 3] of quaternions [n, 4] (w, x, y, z), normalised first."""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def axis_angle_quat(axis, ang):
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    return np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], -1)


def rest_z(quat, plane_z, depth, rng):
    """The centre height at which the cube's lowest corner is `depth` below the plane z = plane_z:
    the support height of a box along z is h * sum |R[2, :]|.  A small tilt leaves the other bottom
    corners close to the plane, and with a uniform depth 3 to 4 % of the envs have one within GRAZING
    of it, more than the checks may leave out: the depth (modified in place) is drawn again, from
    the same range, while a corner is within 5e-5 of the plane."""
    Rz = quat_mat(quat)[:, 2, :]
    sgn = np.array([[1 if i & 1 else -1, 1 if i & 2 else -1, 1 if i & 4 else -1] for i in range(8)], float)
    for _ in range(16):
        z = plane_z + H * np.abs(Rz).sum(-1) - depth
        height = z[:, None] + H * Rz @ sgn.T - plane_z
        bad = (np.abs(height) < 5e-5).any(1)
        if not bad.any():
            break
        depth[bad] = rng.uniform(2e-4, 2e-3, int(bad.sum()))
    return z


@functools.lru_cache(maxsize=None)
def poses(regime, n=N):
    """qpos [n, nq] of a regime (float64 array of fp32 values).  Not to be modified."""
    rng = np.random.default_rng(SEED[regime])
    cm = model()
    q = np.tile(cm.qpos0(), (n, 1))
    q[:, 1], q[:, 2] = -1.57, 1.57  # the arm folded up, away from table, floor and cube
    x, y = 0.25 + rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)  # conftest.cube_qpos
    rand = rng.normal(size=(n, 4))
    small = axis_angle_quat(rng.normal(size=(n, 3)), rng.uniform(0, 0.05, n))
    yaw = axis_angle_quat(np.tile([0.0, 0.0, 1.0], (n, 1)), rng.uniform(-np.pi, np.pi, n))
    depth = rng.uniform(2e-4, 2e-3, n)
    if regime == "tilt":
        quat, z = rand, None
    elif regime == "small_tilt":
        quat, z = small, None
    elif regime == "edge":
        quat, z = yaw, None
        x, y = 0.61 + rng.uniform(-0.015, 0.015, n), rng.uniform(-0.3, 0.3, n)
    elif regime == "corner":
        quat, z = yaw, None
        x, y = 0.61 + rng.uniform(-0.012, 0.012, n), 0.37 + rng.uniform(-0.012, 0.012, n)
    elif regime == "rim":
        quat = rand
        x, y, z = 0.61 + rng.uniform(0, 0.02, n), rng.uniform(-0.3, 0.3, n), TOP + rng.uniform(0, 0.02, n)
    elif regime == "vertex":
        # the table's top corner pokes into a face of the cube: the cube is the reference box
        quat = rand
        x, y, z = 0.61 + rng.uniform(0, 0.012, n), 0.37 + rng.uniform(0, 0.012, n), TOP + rng.uniform(0, 0.012, n)
    elif regime == "side":
        quat = rand
        x, y, z = 0.61 + rng.uniform(0.01, 0.025, n), rng.uniform(-0.3, 0.3, n), np.full(n, -0.1)
    elif regime in ("floor", "floor_small_tilt"):
        quat = rand if regime == "floor" else small
        x, y = rng.uniform(0.7, 1.0, n), rng.uniform(-0.3, 0.3, n)
        z = rest_z(quat, FLOOR, depth, rng)
    else:
        raise KeyError(regime)
    quat = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    if z is None:
        z = rest_z(quat, TOP, depth, rng)
    q[:, 6], q[:, 7], q[:, 8], q[:, 9:13] = x, y, z, quat
    q = q.astype(np.float32).astype(np.float64)
    q.setflags(write=False)
    return q


def flat_poses(n, seed=7, lifted=False):
    """The usual pose of the suite (conftest.cube_qpos, 1 mm deep: 4 table contacts), or lifted 5 cm
    (no contact), the arm folded up as in `poses`."""
    rng = np.random.default_rng(seed)
    q = np.tile(model().qpos0(), (n, 1))
    q[:, 1], q[:, 2] = -1.57, 1.57
    q[:, 6] = 0.25 + rng.uniform(-0.05, 0.05, n)
    q[:, 7] = rng.uniform(-0.05, 0.05, n)
    q[:, 8] = TOP + H + (0.05 if lifted else -1e-3)
    return q.astype(np.float32).astype(np.float64)


def state_of(q):
    cm = model()
    n = len(q)
    return dict(qpos=np.array(q), qvel=np.zeros((n, cm.desc.nv)), warm=np.zeros((n, cm.desc.nv)),
                ctrl=np.zeros((n, cm.desc.nu)), status=np.zeros(n, np.int32), ncon=np.zeros(n))


def ulp_moved(x, k, rng):
    """x (fp32 values) with every component moved by +k or -k fp32 ulps."""
    u = np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)
    return x + k * rng.choice([-1.0, 1.0], x.shape) * u


# ------------------------------------------------------------------------------- the oracle's contacts
@functools.lru_cache(maxsize=None)
def oracle_contacts(regime, ccd="mpr"):
    """Per env the oracle's contact list [k, 9] (dist, pos, normal, geom1, geom2) of a regime, and
    the leave-out mask, decided by the oracle alone: an oracle contact shallower than GRAZING, or
    ill-conditioned -- on one of 4 copies of the qpos moved by +-2 fp32 ulps the count changes or a
    contact moves by more than a quarter of the bar.  Not to be modified."""
    q = poses(regime)
    orc = Oracle(model("PGS", ccd))
    rng = np.random.default_rng(SEED[regime] + 1000)
    cons, out = [], np.zeros(len(q), bool)
    moved = [ulp_moved(q, 2, rng) for _ in range(4)]
    for e in range(len(q)):
        c = orc.forward(q[e])["contacts"].copy()
        cons.append(c)
        if len(c) and np.abs(c[:, 0]).min() < GRAZING:
            out[e] = True
        for m in moved:
            k = orc.forward(m[e])["contacts"]
            if len(k) != len(c) or not (k[:, 7:] == c[:, 7:]).all():
                out[e] = True
            elif len(c) and (np.abs(k[:, :4] - c[:, :4]).max() > BAR / 4 or np.abs(k[:, 4:7] - c[:, 4:7]).max() > NBAR / 4):
                out[e] = True
    return cons, out


def pair_counts(cons, cm):
    """Contact count per env of the floor-cube and the table-cube pair, [n, 2]."""
    fl, tb, cu = geoms(cm)
    return np.array([[int(((c[:, 7] == g) & (c[:, 8] == cu)).sum()) for g in (fl, tb)] for c in cons])


# ------------------------------------------------------------------------- the numpy float64 reference
def corners(c, R, h):
    """The 8 corners of a box, corner i at (+-h0, +-h1, +-h2) by the bits of i."""
    s = np.array([[1 if i & 1 else -1, 1 if i & 2 else -1, 1 if i & 4 else -1] for i in range(8)], float)
    return c + (s * h) @ R.T


def plane_box_ref(c, R, plane_z=FLOOR):
    """The contacts of the cube on a horizontal plane [k, 7]: the corners below the plane (the first
    4 in corner order), dist the corner's signed height, pos the corner moved half way back."""
    nrm = np.array([0.0, 0.0, 1.0])
    out = []
    for p in corners(c, R, np.full(3, H)):
        d = p[2] - plane_z
        if d < 0 and len(out) < 4:
            out.append(np.concatenate([[d], p - 0.5 * d * nrm, nrm]))
    return np.array(out).reshape(-1, 7)


def clip_halfplane(poly, a, lim):
    """The part of a convex polygon (list of points; whatever coordinates they carry besides those
    `a` selects are interpolated along) with x . a <= lim."""
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        sp, sq = p @ a - lim, q @ a - lim
        if sp <= 0:
            out.append(p)
        if sp * sq < 0:
            out.append(p + (q - p) * sp / (sp - sq))
    return out


def sat(c2, R2, c1=TABLE_C, R1=np.eye(3), h1=TABLE_H, h2=np.full(3, H), code=None):
    """Brute-force 15-axis separating-axis test of box 1 (the table) against box 2 (the cube).
    None if an axis separates them, else a dict: `score` and unit `axis` per candidate axis (nan
    where two edges are parallel; the axis points from box 1 to box 2), `code` of the minimum
    (0..2 faces of box 1, 3..5 faces of box 2, 6.. = 6 + 3 i + j edge i x edge j; an edge axis has
    to be 5 % better than a face axis, as the oracle asks), its `overlap`, and the class: `branch`
    (fast / clip / edge), `ref` (table / cube), `face` (the reference box's axis), `nclip` (vertices
    of the incident face clipped to the reference face, before the cut to 4 contacts), `verts` (the
    contact (dist, pos) each of those vertices would give) and `deep_in` (the incident box's deepest
    corner lies over the reference face)."""
    A, B = R1.T, R2.T  # rows: the boxes' axes
    t = c2 - c1
    cand = [A[i] for i in range(3)] + [B[i] for i in range(3)] + [np.cross(A[i], B[j]) for i in range(3) for j in range(3)]
    score, ov, axis = np.full(15, np.nan), np.full(15, np.nan), np.full((15, 3), np.nan)
    for k, L in enumerate(cand):
        ln = np.linalg.norm(L)
        if ln < 1e-6:
            continue
        L = L / ln
        o = h1 @ np.abs(A @ L) + h2 @ np.abs(B @ L) - abs(t @ L)
        if o < 0:
            return None
        ov[k], score[k] = o, (o if k < 6 else 1.05 * o + 1e-9)
        axis[k] = L if t @ L >= 0 else -L
    code = int(np.nanargmin(score)) if code is None else code  # (code given: the class as if that axis had won)
    res = dict(score=score, axis=axis, code=code, overlap=float(ov[code]), normal=axis[code])
    if code >= 6:
        res.update(branch="edge", ref=None, face=None, nclip=0, deep_in=False)
        return res
    ref1 = code < 3
    fa = code % 3
    cr, Ar, hr, ci, Ai, hi = (c1, A, h1, c2, B, h2) if ref1 else (c2, B, h2, c1, A, h1)
    nr = axis[code] if ref1 else -axis[code]  # outward of the reference face, towards the incident box
    ia = int(np.argmax(np.abs(Ai @ nr)))
    s = -np.sign(Ai[ia] @ nr)
    u, v = (ia + 1) % 3, (ia + 2) % 3
    fc = cr + nr * hr[fa]
    face = [ci + s * hi[ia] * Ai[ia] + a * hi[u] * Ai[u] + b * hi[v] * Ai[v] for a, b in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    ra, rb = (fa + 1) % 3, (fa + 2) % 3
    # the incident face in the reference face's coordinates (along its two sides, height over it)
    poly = [np.array([(p - fc) @ Ar[ra], (p - fc) @ Ar[rb], (p - fc) @ nr]) for p in face]
    inside = all(abs(p[0]) <= hr[ra] and abs(p[1]) <= hr[rb] for p in poly)
    for a, lim in (((1, 0, 0), hr[ra]), ((-1, 0, 0), hr[ra]), ((0, 1, 0), hr[rb]), ((0, -1, 0), hr[rb])):
        poly = clip_halfplane(poly, np.array(a, float), lim) if poly else poly
    deep = min(corners(ci, Ai.T, hi), key=lambda p: (p - fc) @ nr)
    # the contacts a vertex of the clipped face gives: (dist, pos) with pos half way back to the face
    verts = np.array([np.concatenate([[p[2]], fc + p[0] * Ar[ra] + p[1] * Ar[rb] + 0.5 * p[2] * nr]) for p in poly]).reshape(-1, 4)
    res.update(branch="fast" if inside else "clip", ref="table" if ref1 else "cube", face=fa, nclip=len(poly), verts=verts,
               deep_in=bool(abs((deep - fc) @ Ar[ra]) <= hr[ra] - BAR and abs((deep - fc) @ Ar[rb]) <= hr[rb] - BAR))
    return res


def edge_contact_pos(s, c2, R2, c1=TABLE_C, R1=np.eye(3), h1=TABLE_H, h2=np.full(3, H)):
    """The position of an edge-edge contact: midway between the closest points of box 1's edge along
    its axis i that lies farthest along the normal and box 2's edge along j farthest against it."""
    i, j = divmod(s["code"] - 6, 3)
    A, B, n = R1.T, R2.T, s["normal"]
    p1 = c1 + sum(np.sign(A[k] @ n) * h1[k] * A[k] for k in range(3) if k != i)
    p2 = c2 - sum(np.sign(B[k] @ n) * h2[k] * B[k] for k in range(3) if k != j)
    # closest points of the lines p1 + x A[i] and p2 + y B[j]: least squares, then on the edges
    x, y = np.linalg.lstsq(np.stack([A[i], -B[j]], 1), p2 - p1, rcond=None)[0]
    x, y = np.clip(x, -h1[i], h1[i]), np.clip(y, -h2[j], h2[j])
    return 0.5 * (p1 + x * A[i] + p2 + y * B[j])


def in_box(p, c, R, h, slack):
    return bool((np.abs(R.T @ (p - c)) <= h + slack).all())


def cube_frame(q):
    return q[6:9], quat_mat(q[None, 9:13])[0]


@functools.lru_cache(maxsize=None)
def classify(regime):
    """sat() of every env of a regime (None where the table and the cube are apart)."""
    return [sat(*cube_frame(q)) for q in poses(regime)]


def check_plane_box(k, q):
    """A list [k, 7] of floor-cube contacts against plane_box_ref."""
    ref = plane_box_ref(*cube_frame(q))
    assert len(k) == len(ref), (len(k), len(ref))
    if len(k):
        assert np.abs(k[:, :4] - ref[:, :4]).max() <= BAR, (k, ref)
        assert np.abs(k[:, 4:7] - ref[:, 4:7]).max() <= NBAR, (k, ref)


def check_face_vertices(k, verts):
    """Face contacts [k, 7] against the vertices (dist, pos) of the numpy clipped incident face."""
    v = verts[verts[:, 0] < 0]
    v = v[np.argsort(v[:, 0], kind="stable")]
    taken = set()
    for row in k:
        near = [j for j in range(len(v)) if j not in taken and np.abs(v[j] - row[:4]).max() <= BAR]
        assert near, ("no such vertex", row, v)
        taken.add(near[0])
    if not (np.abs(verts[:, 0]) < GRAZING).any():
        assert len(k) == min(4, len(v)), (k, v)
        assert np.abs(k[:, 0] - v[:len(k), 0]).max() <= BAR, (k, v)


def check_box_box(k, q):
    """A list [k, 7] of table-cube contacts against the numpy SAT: a unit normal along the
    minimum-score axis, from the table to the cube; an edge contact's dist minus the overlap and
    its point midway between the two edges; face contacts deepest first, none deeper than the
    overlap and the deepest exactly that deep where the incident box's deepest corner lies over the
    reference face (elsewhere the clip cuts it away), each a vertex of the clipped incident face;
    every point inside both boxes inflated by |dist| / 2 plus the bar."""
    c, R = cube_frame(q)
    s = sat(c, R)
    if s is None:
        assert len(k) == 0, k
        return
    if len(k) == 0:
        # a face contact whose incident face has no penetrating vertex over the reference face
        assert s["branch"] == "clip", s
        return
    nrm = k[0, 4:7]
    assert np.abs(k[:, 4:7] - nrm).max() == 0, k                 # one normal per pair
    assert abs(np.linalg.norm(nrm) - 1) <= NBAR, nrm
    assert nrm @ (c - TABLE_C) > 0, nrm                          # from the table to the cube
    # the minimum-score axis (or one tied with it within the bar)
    tied = np.flatnonzero(s["score"] <= np.nanmin(s["score"]) + BAR)
    gap = min(np.abs(nrm - s["axis"][j]).max() for j in tied)
    assert gap <= NBAR, (nrm, s["axis"][tied], s["score"])
    ovs = [(s["score"][j] if j < 6 else (s["score"][j] - 1e-9) / 1.05) for j in tied]
    if all(j >= 6 for j in tied):
        assert len(k) == 1 and abs(k[0, 0] + s["overlap"]) <= BAR, (k, s["overlap"])
    elif all(j < 6 for j in tied):
        assert 1 <= len(k) <= 4 and (k[:, 0] < 0).all() and (np.diff(k[:, 0]) >= 0).all(), k  # deepest first
        # no vertex of the incident face is deeper than the overlap, and the deepest corner is that
        # deep: it is a contact wherever it lies over the reference face (not clipped away)
        assert k[0, 0] >= -max(ovs) - BAR, (k, ovs)
        if s["deep_in"] and len(tied) == 1:
            assert abs(k[0, 0] + s["overlap"]) <= BAR, (k, s["overlap"])
    if len(tied) == 1 and s["code"] >= 6:
        assert np.abs(k[0, 1:4] - edge_contact_pos(s, c, R)).max() <= BAR, (k, edge_contact_pos(s, c, R))
    if all(j < 6 for j in tied):
        # every contact is a penetrating vertex of the clipped incident face, each vertex once; all of
        # them if there are at most 4 (none of them grazing), else 4 that are as deep as the deepest 4
        # (two face axes tied within the bar, as the table's and the flat cube's z: either reference)
        errs = []
        for j in tied:
            try:
                check_face_vertices(k, sat(c, R, code=int(j))["verts"])
            except AssertionError as err:
                errs.append(err.args)
        assert len(errs) < len(tied), errs
    for row in k:
        slack = abs(row[0]) / 2 + BAR
        assert in_box(row[1:4], TABLE_C, np.eye(3), TABLE_H, slack), ("outside the table", row)
        assert in_box(row[1:4], c, R, np.full(3, H), slack), ("outside the cube", row)


# ------------------------------------------------------------------------------------ the library side
def set_qpos(S, q):
    import torch
    S.qpos.copy_(torch.as_tensor(np.ascontiguousarray(q.T), dtype=torch.float32, device=S.device))


def load_state(S, st):
    import torch
    for f, k in (("qpos", "qpos"), ("qvel", "qvel"), ("qacc_warmstart", "warm"), ("ctrl", "ctrl")):
        getattr(S, f).copy_(torch.as_tensor(np.ascontiguousarray(st[k].T), dtype=torch.float32, device=S.device))


def lib_contacts(S, cm):
    """Per env the library's contact list [k, 9] in the oracle's layout."""
    import torch
    out, nc = S.contacts()
    if not S.cpu:
        torch.cuda.synchronize()
    pid = out[..., 7].contiguous().view(torch.int32).cpu().numpy()
    out, nc = to_np(out), to_np(nc).astype(int)
    d = cm.desc
    res = []
    for e in range(len(nc)):
        k = np.zeros((nc[e], 9))
        k[:, :7] = out[e, :nc[e], :7]
        k[:, 7] = [d.pair_geom1[p] for p in pid[e, :nc[e]]]
        k[:, 8] = [d.pair_geom2[p] for p in pid[e, :nc[e]]]
        res.append(k)
    return res


def contacts_bits(S):
    """(contact list, count) of the batch as int32 bit patterns; the slots past an env's count are
    zeroed by BatchSim.contacts."""
    import torch
    out, nc = S.contacts()
    if not S.cpu:
        torch.cuda.synchronize()
    return out.contiguous().view(torch.int32).cpu(), nc.cpu()


# ---------------------------------------------------------------------------------- a. contact parity
def check_contact_parity(make_sim, regime, ccd="mpr"):
    """The library's contacts of a regime against the oracle's: the same pairs in the same order
    (so the same count per pair), dist and pos within BAR and the normal within NBAR, on every env
    the oracle does not leave out.  Returns the largest gaps (dist, pos, normal)."""
    cm, q = model("PGS", ccd), poses(regime)
    cons, out = oracle_contacts(regime, ccd)
    assert out.sum() <= LEAVE_OUT * len(q), (regime, np.flatnonzero(out))
    S = make_sim(cm, len(q))
    set_qpos(S, q)
    got = lib_contacts(S, cm)
    gd = gp = gn = 0.0
    for e in np.flatnonzero(~out):
        k, c = got[e], cons[e]
        assert len(k) == len(c) and (k[:, 7:] == c[:, 7:]).all(), (regime, e, k, c)
        if len(c):
            gd = max(gd, np.abs(k[:, 0] - c[:, 0]).max())
            gp = max(gp, np.abs(k[:, 1:4] - c[:, 1:4]).max())
            gn = max(gn, np.abs(k[:, 4:7] - c[:, 4:7]).max())
    print(f"{regime} {ccd}: {len(q)} envs, {int(out.sum())} left out, pair counts (floor, table) "
          f"{[np.bincount(x, minlength=5).tolist() for x in pair_counts(cons, cm).T]}, "
          f"gap dist {gd:.2e} pos {gp:.2e} normal {gn:.2e}")
    assert gd <= BAR and gp <= BAR and gn <= NBAR, (regime, gd, gp, gn)
    return gd, gp, gn


# -------------------------------------------------------------------------------------- b. invariants
def check_invariants(make_sim, regime, ccd="mpr"):
    """The numpy reference's checks on the library's own contacts (the oracle is used for the
    leave-out set only): plane_box_ref for the floor pair, check_box_box for the table pair; the
    folded arm has no contact."""
    cm, q = model("PGS", ccd), poses(regime)
    _, out = oracle_contacts(regime, ccd)
    fl, tb, cu = geoms(cm)
    S = make_sim(cm, len(q))
    set_qpos(S, q)
    got = lib_contacts(S, cm)
    for e in np.flatnonzero(~out):
        k = got[e]
        on_floor = (k[:, 7] == fl) & (k[:, 8] == cu)
        on_table = (k[:, 7] == tb) & (k[:, 8] == cu)
        assert (on_floor | on_table).all(), (regime, e, k)
        try:
            check_plane_box(k[on_floor, :7], q[e])
            check_box_box(k[on_table, :7], q[e])
        except AssertionError as err:
            raise AssertionError((regime, ccd, "env", int(e)) + err.args) from None


# ------------------------------------------------------------------------------------------ c. census
CENSUS_MIN = 8


def census():
    """The classes the poses reach, from the two references alone: {class: envs} over all regimes,
    and the table per regime (printed)."""
    cm = model()
    total = {}
    for r in REGIMES:
        cons, out = oracle_contacts(r)
        pc = pair_counts(cons, cm)
        row = {}
        for j, name in enumerate(("floor", "table")):
            for c in (1, 2, 3, 4):
                row[f"{name} count {c}"] = int((pc[:, j] == c).sum())
        cl = [s for s in classify(r) if s is not None]
        row["fast face"] = sum(s["branch"] == "fast" for s in cl)
        row["clipped face"] = sum(s["branch"] == "clip" for s in cl)
        row["edge-edge"] = sum(s["branch"] == "edge" for s in cl)
        row["clipped polygon > 4"] = sum(s["nclip"] > 4 for s in cl)
        row["reference cube"] = sum(s["ref"] == "cube" for s in cl)
        row["reference table side"] = sum(s["ref"] == "table" and s["face"] != 2 for s in cl)
        row["left out"] = int(out.sum())
        print(f"{r:17s}", " ".join(f"{v:3d}" for v in row.values()))
        for k, v in row.items():
            total[k] = total.get(k, 0) + v
    print("columns:", ", ".join(total))
    print(f"{'all':17s}", " ".join(f"{v:3d}" for v in total.values()))
    return total


@functools.lru_cache(maxsize=None)
def composition_targets():
    """(regime, env) of one env of each table-pair count 1..4 and one edge-edge env, none left out."""
    cm = model()
    found = {}
    for r in REGIMES:
        cons, out = oracle_contacts(r)
        pc, cl = pair_counts(cons, cm), classify(r)
        for e in np.flatnonzero(~out):
            if cl[e] is None:
                continue
            key = "edge" if cl[e]["branch"] == "edge" else int(pc[e, 1])
            if key != 0:
                found.setdefault(key, (r, int(e)))
    return [found[k] for k in (1, 2, 3, 4, "edge")]


# ------------------------------------------------------------------------------------ d. stale counts
def check_stale_counts(make_sim, solver="PGS"):
    """The count word of a slot is rewritten by every collide pass: contacts() and one substep at
    count 1..2 (tilted cube) in slots that held count 4 (flat cube), and at table contacts in slots
    that held floor contacts, give a fresh batch's bits."""
    cm = model(solver)
    n = 16
    flat, tilt, floor = flat_poses(n), poses("tilt")[:n], poses("floor_small_tilt")[:n]
    for first, second, c1, c2 in ((flat, tilt, {4}, {1, 2}), (floor, tilt, {1, 2, 3, 4}, {1, 2})):
        fresh = make_sim(cm, n)
        set_qpos(fresh, second)
        want = contacts_bits(fresh)
        S = make_sim(cm, n)
        set_qpos(S, first)
        _, nc = S.contacts()
        assert set(to_np(nc).astype(int)) <= c1, nc
        set_qpos(S, second)
        got = contacts_bits(S)
        assert set(got[1].numpy().tolist()) <= c2, got[1]
        assert bool((got[0] == want[0]).all()) and bool((got[1] == want[1]).all()), "contacts() after other counts"
        # the same through the substep: step from `first`, load `second`, step
        F = make_sim(cm, n)
        load_state(F, state_of(second))
        F.status.zero_(), F.ncon.zero_()
        F.substeps(1)
        F.observe()
        S = make_sim(cm, n)
        load_state(S, state_of(first))
        S.status.zero_(), S.ncon.zero_()
        S.substeps(1)
        assert set(to_np(S.ncon).astype(int)) <= c1, S.ncon
        load_state(S, state_of(second))
        S.status.zero_(), S.ncon.zero_(), S.obs.zero_()
        S.substeps(1)
        S.observe()
        assert set(to_np(S.ncon).astype(int)) <= c2, S.ncon
        assert_same_bits(snapshot(S), snapshot(F), what="a substep after other counts in the same slots")


# ------------------------------------------------------------------------------- e. batch composition
def check_batch_composition(make_sim, solver="PGS"):
    """One env of each count 1..4 and one edge-edge env give the same contacts() and one-substep
    bits alone, as first and last of 5, and as last of 68 among lifted-cube envs."""
    cm = model(solver)
    tq = np.stack([poses(r)[e] for r, e in composition_targets()])
    lifted = flat_poses(67, lifted=True)

    def run(q):
        S = make_sim(cm, len(q))
        set_qpos(S, q)
        con = contacts_bits(S)
        S = make_sim(cm, len(q))
        load_state(S, state_of(q))
        S.status.zero_(), S.ncon.zero_()
        S.substeps(1)
        S.observe()
        return con, snapshot(S)

    for i in range(len(tq)):
        x = tq[i:i + 1]
        (c1, n1), s1 = run(x)
        assert int(n1[0]) >= 1
        others = np.delete(tq, i, axis=0)[:3]
        layouts = [(np.concatenate([x, others, x]), (0, 4)), (np.concatenate([lifted, x]), (67,))]
        for q, at in layouts:
            (c, nc), s = run(q)
            for k in at:
                what = ("target", i, "env", k, "of", len(q))
                assert bool((c[k] == c1[0]).all()) and int(nc[k]) == int(n1[0]), what
                assert_same_bits(rows(s, [k]), rows(s1, [0]), what=what)


# --------------------------------------------------------------------------------------- f. one substep
@functools.lru_cache(maxsize=None)
def oracle_substep(solver, regime):
    """One oracle substep from a regime's states (zero qvel, warm start and ctrl), and the per-env
    qvel envelope of fp32-sized state noise, from the oracle alone (the one-substep analogue of
    conftest.fp32_noise_envelope): the largest qvel deviation, over the dofs and 4 trials, of the
    oracle stepped from the state moved by +-8 fp32 ulps per component.  Not to be modified."""
    orc = Oracle(model(solver))
    st0 = state_of(poses(regime))
    ref = {k: v.copy() for k, v in st0.items()}
    orc.step(ref, None, nsub=1, nthreads=8)
    rng = np.random.default_rng(SEED[regime] + 2000)
    env = np.zeros(len(st0["qpos"]))
    for _ in range(4):
        c = {k: v.copy() for k, v in st0.items()}
        for k in ("qpos", "qvel", "warm"):
            u = np.spacing(np.abs(c[k].astype(np.float32))).astype(np.float64)
            c[k] = c[k] + rng.integers(-8, 9, c[k].shape) * u
        orc.step(c, None, nsub=1, nthreads=8)
        env = np.maximum(env, np.abs(c["qvel"] - ref["qvel"]).max(1))
    return ref, env


def check_substep(make_sim, solver, regime):
    """One substep from a regime's states: ncon and status per env equal the oracle's, qpos within
    BAR, and the qvel gap per regime within bars from the oracle alone: p50 and p99 within
    max(QVEL_BARS entry, 10 x the envelope's same percentile) (the factor test_trajectory_shadowing
    gives fp32 arithmetic over fp32 state noise), at most 2 % of the envs over QVEL_BARS[2], each
    of those over QVEL_BARS[2] / 10 in the envelope too.  Returns (gaps, envelope)."""
    cm = model(solver)
    ref, env = oracle_substep(solver, regime)
    S = make_sim(cm, len(env))
    load_state(S, state_of(poses(regime)))
    S.status.zero_(), S.ncon.zero_()
    S.substeps(1)
    dv = np.abs(to_np(S.qvel).T - ref["qvel"]).max(1)
    dq = np.abs(to_np(S.qpos).T - ref["qpos"]).max()
    pc = lambda a, p: float(np.percentile(a, p))
    print(f"substep {solver} {regime}: ncon {np.bincount(ref['ncon'].astype(int)).tolist()}, qpos gap {dq:.2e}, qvel gap "
          f"p50 {pc(dv, 50):.2e} p99 {pc(dv, 99):.2e} max {dv.max():.2e} | envelope p50 {pc(env, 50):.2e} "
          f"p99 {pc(env, 99):.2e} max {env.max():.2e} | over {QVEL_BARS[2]:.1e}: {int((dv > QVEL_BARS[2]).sum())}")
    ncon, stat = to_np(S.ncon), to_np(S.status).astype(int)
    assert (ncon == ref["ncon"]).all(), (np.flatnonzero(ncon != ref["ncon"]), ncon, ref["ncon"])
    assert (stat == ref["status"]).all(), (stat, ref["status"])
    assert dq <= BAR, dq
    assert np.isfinite(dv).all()
    p50, p99 = max(QVEL_BARS[0], 10 * pc(env, 50)), max(QVEL_BARS[1], 10 * pc(env, 99))
    assert pc(dv, 50) <= p50 and pc(dv, 99) <= p99, (pc(dv, 50), pc(dv, 99), "bars", p50, p99)
    tail = dv > QVEL_BARS[2]
    assert tail.sum() <= 0.02 * len(dv), (np.flatnonzero(tail), dv[tail])
    assert (env[tail] > QVEL_BARS[2] / 10).all(), (np.flatnonzero(tail), dv[tail], env[tail])
    return dv, env


# ------------------------------------------------------------------------- g. the Newton corner envs
# Cubes that overhang the table's corner (x, y, z, quaternion w and z; yaw only, 3 or 4 clipped
# contacts) from which the CPU backend's Newton solve ended 1.0e-3 to 2.1e-3 in qvel from the
# oracle's (PGS on the same states: under 1e-6; the oracle's own envelope there: 2e-6 to 1.2e-5): it took
# its stopping test's improvement from the difference of two fp32 costs, which is rounding noise
# long before the cube's light rotational dofs have converged.
NEWTON_CORNER = (
    (0.59830797, 0.360823, 0.012691738, 0.8851738, -0.46526048),
    (0.60825413, 0.36081812, 0.01294045, 0.70660794, -0.7076053),
    (0.60534805, 0.3651116, 0.012653039, 0.9895473, -0.14420858),
    (0.6105153, 0.36508274, 0.012656302, 0.99361044, 0.11286401),
    (0.61008894, 0.37786877, 0.013107613, 0.8200724, 0.5722597),
    (0.607302, 0.36842108, 0.013874679, 0.37241644, -0.9280657),
    (0.60135573, 0.370442, 0.01222359, 0.06904002, 0.9976139),
    (0.61177903, 0.36110187, 0.013824544, 0.1863011, 0.9824927),
)


def newton_corner_poses():
    c = np.array(NEWTON_CORNER)
    q = np.tile(model().qpos0(), (len(c), 1))
    q[:, 1], q[:, 2] = -1.57, 1.57
    q[:, 6:9], q[:, 9], q[:, 10:12], q[:, 12] = c[:, :3], c[:, 3], 0.0, c[:, 4]
    return q.astype(np.float32).astype(np.float64)


def check_newton_corner(make_sim, solver):
    """One substep from the NEWTON_CORNER states: every env is well conditioned (the oracle's
    envelope of +-8 fp32 ulps of state noise, 4 trials, is under QVEL_BARS[1] / 10), so every env's
    qvel is within QVEL_BARS[1] of the oracle's, and qpos within BAR."""
    cm, orc = model(solver), Oracle(model(solver))
    st0 = state_of(newton_corner_poses())
    ref = {k: v.copy() for k, v in st0.items()}
    orc.step(ref, None, nsub=1)
    rng = np.random.default_rng(1)
    env = np.zeros(len(st0["qpos"]))
    for _ in range(4):
        c = {k: v.copy() for k, v in st0.items()}
        c["qpos"] = c["qpos"] + rng.integers(-8, 9, c["qpos"].shape) * np.spacing(np.abs(c["qpos"].astype(np.float32))).astype(np.float64)
        orc.step(c, None, nsub=1)
        env = np.maximum(env, np.abs(c["qvel"] - ref["qvel"]).max(1))
    S = make_sim(cm, len(env))
    load_state(S, st0)
    S.status.zero_(), S.ncon.zero_()
    S.substeps(1)
    dv = np.abs(to_np(S.qvel).T - ref["qvel"]).max(1)
    print(f"newton corner envs {solver}: ncon {ref['ncon'].astype(int).tolist()}, qvel gap {np.array2string(dv, precision=2)}, "
          f"envelope {np.array2string(env, precision=2)}")
    assert (ref["ncon"] >= 3).all() and (env < QVEL_BARS[1] / 10).all(), (ref["ncon"], env)
    assert (to_np(S.ncon) == ref["ncon"]).all() and (to_np(S.status) == 0).all()
    assert np.abs(to_np(S.qpos).T - ref["qpos"]).max() <= BAR
    assert (dv <= QVEL_BARS[1]).all(), dv
