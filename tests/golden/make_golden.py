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


if __name__ == "__main__":
    if sys.argv[1:] == ["contact_overflow"]:
        contact_overflow_states()
    else:
        main()
        contact_overflow_states()
