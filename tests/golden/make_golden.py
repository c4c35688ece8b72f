"""Generate the committed oracle fixtures (run: python tests/golden/make_golden.py).

There are no golden vectors in the reference: the
fixtures here are produced by this repository's float64 oracle and pin it
against regressions; the GPU parity tests compare the HIP path with them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import soarm_pkg  # noqa: E402,F401
from lerobot_mujoco_sim2real_amd import mjcf  # noqa: E402
from oracle import Oracle  # noqa: E402


def main():
    rng = np.random.default_rng(20251212)
    cm = mjcf.compile_mjcf(mjcf.SCENE_XML, disable_contact=True)
    orc = Oracle(cm)
    n, T = 8, 12
    iq = rng.uniform(-0.3, 0.3, (n, 5))
    acts = rng.uniform(-0.5, 0.5, (T, n, 5))
    st = orc.new_state(n)
    obs = [orc.reset(st, init_qpos=iq)]
    for a in acts:
        obs.append(orc.step(st, a))
    np.savez_compressed(os.path.join(HERE, "oracle_arm_random.npz"), init_qpos=iq, actions=acts,
                        obs=np.stack(obs))


def contact_overflow_states(seed=5, n=1024):
    """tests/golden/contact_overflow_states.npz: pick-scene states with 7..16 contacts per env and
    past the cap of 16, for tests/contact_overflow_ref.py (which documents the classes).  From the
    float64 oracle alone, default PGS model, zero action; fp32-rounded qpos, qvel, warm, ctrl.

    Poses: contact_overflow_ref.overflow_poses (the arm lying on the table), the cube placed by
    conftest.cube_qpos.
      deep    -- 1 env-step after placement.  Candidates: 7+ contacts, none grazing (|dist| > 20 um,
                 so fp32 and fp64 list the same contacts), no status bit but overflow, and a float64
                 substep that moves by at most QVEL_BARS[2] / 10 when qpos, qvel and the warm start
                 move by +-8 fp32 ulps (an env more sensitive than that cannot be held to a bar in
                 fp32 by any solver).  Taken calmest first, by the largest constraint force of the
                 oracle's forward: the rounding error of an fp32 solve grows with the forces it sums
                 (tens to 1500 N here, on links of a few grams), and among 878 candidates every env
                 where the CPU backend is over QVEL_BARS[2] has a force over 175 N, with either solver.
                 10 past the cap, 10 with exactly 16, and among the rest 12 with the block in LDS, 20
                 straddling slot 6, 20 in the slab; 6 with 8 contacts, 3 at each count 9..15, topped
                 up to 96.  (Every env past the cap or at 16 carries over 150 N: those classes cannot
                 be had calm.)
      shallow -- 25 env-steps of settling, then the depth filter of test_contacts_match_oracle (every
                 contact between 20 um and 5 mm deep), 7+ contacts, status 0: the first 28.  The block
                 is in LDS in every one of them: under the depth filter no env of this recipe (nor of
                 1, 3, 8, 50, 100 or 150 settle steps) has 3+ arm-table contacts ahead of the block
                 without one of them deeper than 5 mm (7 or 8 contacts is all the filter passes); nor
                 do flatter (shoulder 1.2..1.7, elbow 0.8..1.6), wider (every range about doubled) or
                 folded (wrist flex -1.6..0.3) pose ranges at 10, 25 and 50 settle steps.  So the
                 straddling and in-slab classes are covered by the deep set only.
      fill    -- test_rs_solve_loop._mixed_states' recipe: 16 resting cubes (4 contacts), 8 lifted
                 5 cm clear (0 contacts), arm poses in +-0.3 rad.
    """
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import contact_overflow_ref as R
    from conftest import cube_qpos
    cm = R.model()
    orc = Oracle(cm)

    def settled(steps):
        rng = np.random.default_rng(seed)
        q = R.overflow_poses(rng, n)
        st = orc.new_state(n)
        orc.reset(st, init_qpos=q[:, :5], extra_qpos=cube_qpos(cm, n, rng, q))
        st["qpos"][:, :6] = q
        for _ in range(steps):
            orc.step(st, np.zeros((n, 5)), nthreads=8)
        sticky = st["status"].copy()
        st = R.f32(st)
        st["status"][:] = 0
        st["ncon"][:] = 0
        return st, sticky

    def sensitivity(st, cen, kulp=8, trials=2):
        rng = np.random.default_rng(seed + 1)
        out = np.zeros(len(st["qpos"]))
        for _ in range(trials):
            b = {k: v.copy() for k, v in st.items()}
            for k in ("qpos", "qvel", "warm"):
                x = b[k].astype(np.float32)
                b[k][:] = x.astype(np.float64) + rng.integers(-kulp, kulp + 1, x.shape) * np.spacing(np.abs(x)).astype(np.float64)
            orc.step(b, None, nsub=1, nthreads=8)
            out = np.maximum(out, np.abs(b["qvel"] - cen["qvel"]).max(1))
        return out

    # ---- deep
    st, _ = settled(1)
    cen = R.census(cm, orc, st)
    cls = R.classes(cen)
    ok = (cen["ncon"] > R.LDS_CON) & (cen["graze"] > R.GRAZING) & np.isfinite(cen["qvel"]).all(1)
    ok &= (cen["status"] & ~8) == 0
    ok &= sensitivity(st, cen) <= R.QVEL_BARS[2] / 10
    pick = []
    calmest = np.argsort(cen["fmax"], kind="stable")

    def add(mask, k):
        ids = [int(i) for i in calmest if (mask & ok)[i] and i not in pick]
        pick.extend(ids[:k])

    add(cls["over"], 10)
    add(cls["full"], 10)
    rest = ~cls["over"] & ~cls["full"]
    add(cls["lds"] & rest, 12)
    add(cls["straddle"] & rest, 20)
    add(cls["slab"] & rest, 20)
    add(cen["ncon"] == 8, 6)
    for c in range(9, 16):
        add(cen["ncon"] == c, max(0, 3 - int((cen["ncon"][pick] == c).sum())))
    add(np.ones(n, bool), 96 - len(pick))
    deep = R.take(st, sorted(pick))
    # ---- shallow
    st, sticky = settled(25)
    cen = R.census(cm, orc, st)
    ok = (cen["ncon"] > R.LDS_CON) & (cen["graze"] > R.GRAZING) & (cen["deepest"] > -R.DEEPEST)
    ok &= (cen["status"] == 0) & (sticky == 0) & np.isfinite(cen["qvel"]).all(1)
    shallow = R.take(st, np.flatnonzero(ok)[:28])
    # ---- fill
    nf = 24
    rng = np.random.default_rng(seed + 2)
    st = orc.new_state(nf)
    orc.reset(st, init_qpos=rng.uniform(-0.3, 0.3, (nf, 5)), extra_qpos=cube_qpos(cm, nf, rng))
    for _ in range(5):  # settle the cubes onto the table
        orc.step(st, rng.uniform(-0.5, 0.5, (nf, 5)))
    st["qpos"][16:, 8] += 0.05
    fill = R.f32(st)
    out = {}
    for name, s in (("shallow", shallow), ("deep", deep), ("fill", fill)):
        for k in R.KEYS:
            out[f"{name}_{k}"] = s[k].astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "contact_overflow_states.npz"), **out)
    print({k: v.shape for k, v in out.items()})


def joint_limit_states(seed=11, n=2048):
    """tests/golden/joint_limit_states.npz: pick-scene states with active joint-limit rows, for
    tests/joint_limits_ref.py (which documents the sets; test_joint_limits.test_fixture_census pins
    the counts).  From the float64 oracle alone, stock PGS model; fp32-rounded qpos, qvel, warm, ctrl.

    Every candidate is placed (arm pose, arm qvel, ctrl = the pose +-0.2 rad, the cube by
    conftest.cube_qpos lowered 0.1 mm onto the table or lifted 5 cm) and then stepped 2 oracle
    substeps, so that qvel, the warm start and the cube's contacts are those of a trajectory with the
    limit rows in it.  A candidate is kept when its status is 0, no contact is grazing (20 um) or
    deeper than 5 mm, and one float64 substep moves by at most SENS when qpos, qvel and the warm
    start move by +-8 fp32 ulps (an env more sensitive than that cannot be held to a bar in fp32).
      past    -- 1..6 joints 1.5e-4..2.5e-2 rad past a random side, qvel in +-1 rad/s, or 1..2.5
                 rad/s out of the limit (the row that carries no force); the free joints folded
                 clear of the table (shoulder_lift -1.2..-0.2), or, with shoulder_lift past its upper
                 side, elbow and wrist drawn over their whole range and the census left to choose.
                 No arm contact.  elbow_flex upper has no env, here or in `near`: from 1.6 rad on
                 the base touches the lower arm, and at the range's end (1.69) it is 8..12 mm inside
                 it at every shoulder and wrist pose, past the 5 mm bound; shoulder_lift upper is had
                 free of contact with the elbow folded.  Picked in candidate order: 7 per (joint, side) with force > 0, 16
                 with a zero-force row, 6 with all six joints limited, 10 with 4 or 5, topped up to
                 32 at each of nlim = 1, 2, 3 and to 160 in all.
      near    -- 1..4 joints 0.006..0.04 rad inside a random side, qvel in +-0.5 rad/s; kept when
                 every joint is inside its range and one is within 0.045 rad.  3 per (joint, side),
                 16 with three or more such joints, topped up to 48.
      coupled -- a limit row, at least one arm-table or arm-cube contact, at most 6 contacts.  Two
                 pools of contact_overflow_ref.overflow_poses (the arm lying on the table): placed as
                 above with 1..2 joints past a side (17 of 4096 pass the depth bound: a freshly
                 placed arm lies deep), and held 15 env-steps at the pose first, then shoulder_pan,
                 wrist_roll or the gripper moved past a side (they leave the table contacts where
                 they are; 378 of 2048 pass).  The 2 calmest per (joint, side) with force, by the
                 oracle's largest constraint force, then the calmest up to 32.  No draw gave
                 shoulder_lift (either side) or elbow_flex upper with force here: 9 of the 12 pairs.
    """
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import contact_overflow_ref as R
    import joint_limits_ref as J
    from conftest import cube_qpos
    cm = J.model()
    orc = Oracle(cm)
    rg = np.array([list(cm.desc.jnt_range[j]) for j in range(J.NA)])
    SENS = R.QVEL_BARS[2] / 10

    def folded(rng, m):
        q = rng.uniform(-0.4, 0.4, (m, 6))
        q[:, 1] = rng.uniform(-1.2, -0.2, m)
        q[:, 5] = rng.uniform(0.0, 1.0, m)
        return q

    def push(rng, q, v, e, j, side, lo, hi, leaving):
        """Joint j of env e to lo..hi (log-uniform) past `side` (negative: inside it)."""
        pen = np.exp(rng.uniform(np.log(abs(lo)), np.log(abs(hi)))) * np.sign(lo)
        q[e, j] = rg[j, side] + (pen if side else -pen)
        if leaving:
            q[e, j] = rg[j, side] + (1 if side else -1) * rng.uniform(8e-3, 2.2e-2)
            v[e, j] = (-1 if side else 1) * rng.uniform(1.0, 2.5)

    def evolve(rng, q, v, lifted, settled=None):
        m = len(q)
        full = cube_qpos(cm, m, rng, q)
        full[:, 8] -= 1e-4
        full[lifted, 8] += 0.05
        st = orc.new_state(m)
        orc.reset(st, init_qpos=full[:, :5], extra_qpos=full)
        st["qpos"][:, :6] = q
        if settled is not None:
            for _ in range(15):
                orc.step(st, q[:, :5], nthreads=8)
            q, v = st["qpos"][:, :6].copy(), st["qvel"][:, :6].copy()
            settled(rng, q, v)
            st["qpos"][:, :6] = q
        st["qvel"][:, :6] = v
        st["ctrl"][:] = np.clip(q + rng.uniform(-0.2, 0.2, (m, 6)), rg[:, 0], rg[:, 1])
        orc.step(st, None, nsub=2, nthreads=8)
        sticky = st["status"].copy()
        st = R.f32(st)
        st["status"][:] = 0
        st["ncon"][:] = 0
        cen = J.census(cm, orc, st)
        ok = (cen["status"] == 0) & (sticky == 0) & np.isfinite(cen["qvel"]).all(1)
        ok &= (cen["graze"] > R.GRAZING) & (cen["deepest"] > -R.DEEPEST)
        return st, cen, ok, J.sensitivity(orc, st, cen["qvel"], seed=seed + 1)

    def chooser(ok):
        pick = []

        def add(mask, k):
            ids = [int(i) for i in np.flatnonzero(mask & ok) if i not in pick]
            pick.extend(ids[:max(0, k)])
        return pick, add

    # ---- past
    rng = np.random.default_rng(seed)
    q, v = folded(rng, n), rng.uniform(-1, 1, (n, 6))
    nk = rng.choice([1, 2, 3, 4, 5, 6], n, p=[0.22, 0.22, 0.22, 0.1, 0.08, 0.16])
    for e in range(n):
        js = rng.choice(6, nk[e], replace=False)
        sides = rng.integers(0, 2, 6)
        if 1 in js and sides[1] == 1:  # shoulder_lift upper: the arm reaches down to the table
            q[e, 2:4] = rng.uniform(rg[2:4, 0] + 0.1, rg[2:4, 1] - 0.1)
        for j in js:
            push(rng, q, v, e, j, sides[j], 1.5e-4, 2.5e-2, leaving=rng.random() < 0.15)
    st, cen, ok, sens = evolve(rng, q, v, rng.random(n) < 0.5)
    viol = np.where(cen["present"], -cen["dist"], np.nan)
    ok &= (cen["nlim"] >= 1) & (cen["ncon"] == cen["nblk"]) & np.isin(cen["ncon"], (0, 4)) & (sens <= SENS)
    ok &= (np.nan_to_num(viol, nan=1e-3) >= J.VIOL[0]).all((1, 2)) & (np.nan_to_num(viol, nan=1e-3) <= J.VIOL[1]).all((1, 2))
    active = cen["present"] & (cen["force"] > 0)
    idle = (cen["present"] & (cen["force"] == 0)).any((1, 2))
    pick, add = chooser(ok)
    for j in range(6):
        for s in range(2):
            add(active[:, j, s] & (cen["nlim"] <= 3), 7)
            add(active[:, j, s], 7 - int(active[pick, j, s].sum()))
    add(idle, 16 - int(idle[pick].sum()))
    add(cen["nlim"] == 6, 6 - int((cen["nlim"][pick] == 6).sum()))
    add((cen["nlim"] == 4) | (cen["nlim"] == 5), 10 - int(np.isin(cen["nlim"][pick], (4, 5)).sum()))
    for k in (1, 2, 3):
        add(cen["nlim"] == k, 32 - int((cen["nlim"][pick] == k).sum()))
    add(np.ones(n, bool), 160 - len(pick))
    print("past: candidates", int(ok.sum()), "of", n, "picked", len(pick), "nlim", np.bincount(cen["nlim"][pick]),
          "active per pair", active[pick].sum(0).ravel(), "idle", int(idle[pick].sum()), "ncon", np.bincount(cen["ncon"][pick]),
          "sens max", sens[pick].max(), "force max", cen["force"][pick].max())
    past = R.take(st, sorted(pick))
    # ---- near
    rng = np.random.default_rng(seed + 2)
    m = n // 4
    q, v = folded(rng, m), rng.uniform(-0.5, 0.5, (m, 6))
    for e in range(m):
        for j in rng.choice(6, rng.integers(1, 5), replace=False):
            push(rng, q, v, e, j, rng.integers(0, 2), -0.006, -0.04, leaving=False)
    st, cen, ok, sens = evolve(rng, q, v, rng.random(m) < 0.5)
    close = (cen["dist"] < J.NEAR)
    ok &= (cen["dist"] > 0).all((1, 2)) & close.any((1, 2)) & (cen["nlim"] == 0) & (sens <= SENS)
    ok &= (cen["ncon"] == cen["nblk"]) & np.isin(cen["ncon"], (0, 4))
    pick, add = chooser(ok)
    for j in range(6):
        for s in range(2):
            add(close[:, j, s], 3)
    add(close.sum((1, 2)) >= 3, 16 - int((close[pick].sum((1, 2)) >= 3).sum()))
    add(np.ones(m, bool), 48 - len(pick))
    print("near: candidates", int(ok.sum()), "of", m, "picked", len(pick), "close per pair", close[pick].sum(0).ravel(),
          "3+", int((close[pick].sum((1, 2)) >= 3).sum()), "ncon", np.bincount(cen["ncon"][pick]))
    near = R.take(st, sorted(pick))
    # ---- coupled: A, placed like the others; B, held 15 env-steps at the pose first (the arm settles
    # on the table), then shoulder_pan, wrist_roll or the gripper moved past a side
    rng = np.random.default_rng(seed + 3)
    m = 2 * n
    q, v = R.overflow_poses(rng, m), rng.uniform(-0.5, 0.5, (m, 6))
    for e in range(m):
        for j in rng.choice(6, rng.integers(1, 3), replace=False):
            push(rng, q, v, e, j, 1 if j == 1 else rng.integers(0, 2), 1.5e-4, 2.5e-2, leaving=False)
    A = evolve(rng, q, v, np.zeros(m, bool))

    def moved(rng, q, v):
        for e in range(len(q)):
            for j in rng.choice([0, 4, 5], rng.integers(1, 3), replace=False):
                push(rng, q, v, e, j, rng.integers(0, 2), 1.5e-4, 2.5e-2, leaving=False)
                if v[e, j] == 0.0:
                    v[e, j] = rng.uniform(-0.5, 0.5)
    B = evolve(rng, R.overflow_poses(rng, n), np.zeros((n, 6)), np.zeros(n, bool), settled=moved)
    st = R.concat(A[0], B[0])
    cen = {k: np.concatenate([A[1][k], B[1][k]]) for k in A[1]}
    ok, sens = np.concatenate([A[2], B[2]]), np.concatenate([A[3], B[3]])
    ok &= (cen["nlim"] >= 1) & (cen["ncon"] > cen["nblk"]) & (cen["ncon"] <= R.LDS_CON) & (sens <= SENS)
    ok &= cen["ncon_step"] == cen["ncon"]
    active = cen["present"] & (cen["force"] > 0)
    calmest = np.argsort(cen["fmax"], kind="stable")
    pick = []
    for j in range(6):
        for s in range(2):
            pick.extend([int(i) for i in calmest if ok[i] and active[i, j, s] and i not in pick][:2])
    pick.extend([int(i) for i in calmest if ok[i] and i not in pick][:32 - len(pick)])
    print("coupled: candidates", int(ok[:m].sum()), "of", m, "placed,", int(ok[m:].sum()), "of", n, "settled; picked", len(pick),
          "nlim", np.bincount(cen["nlim"][pick]), "ncon", np.bincount(cen["ncon"][pick]), "arm contacts",
          np.bincount((cen["ncon"] - cen["nblk"])[pick]), "active per pair", active[pick].sum(0).ravel(),
          "fmax", cen["fmax"][pick].max(), "sens max", sens[pick].max())
    coupled = R.take(st, sorted(pick))
    out = {}
    for name, s in (("past", past), ("near", near), ("coupled", coupled)):
        for k in R.KEYS:
            out[f"{name}_{k}"] = s[k].astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "joint_limit_states.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    if sys.argv[1:] == ["contact_overflow"]:
        contact_overflow_states()
    elif sys.argv[1:] == ["joint_limit_states"]:
        joint_limit_states()
    else:
        main()
        contact_overflow_states()
        joint_limit_states()
