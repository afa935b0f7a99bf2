"""Generate tests/golden/env_smplx.npz: the reference's own env functions at the 52 bodies of the SMPL-X / SMPL-H humanoid.

    python tools/gen_golden_smplx.py [--out DIR]

Needs the reference tree (oracle/refload.py reads its functions at run time; nothing of its text is kept here).  The committed
fixture holds OUTPUTS only, each written by a reference function; the inputs are redrawn from the seed by ``inputs()`` (the tests
call it too -- with every input stored as well the file would pass the size limit for a committed file) and the fixture carries
their float64 sums, so a generator that draws other numbers is noticed.

Inputs (seed 5252): 33 envs of ``syn.rigid_body_state(g, 33, 52)`` -- the distribution of the 24-body fixtures -- and references
NEAR the simulated state, so that no reward term saturates: positions + 0.06 N(0, 1) with every third env's reference moved 0.3 m
in x (those envs fall), rotations normalise(body + 0.15 N(0, 1)), velocities + 1.5 N(0, 1), progress uniform in 0 .. 9, pass_time
with probability 0.2.  One draw of three future samples serves the task observation (T = 3; its first sample is the T = 1
reference) and an independent draw the reward / reset.

The generator FAILS unless the fixture can tell a wrong kernel from a right one: every raw reward term inside (0.01, 0.99) for at
least half the envs, between 15 % and 85 % of the envs terminated, and no reset distance within 1e-4 of the threshold.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pulse_amd import synthetic as syn  # noqa: E402

SEED, N, T = 5252, 33, 3
TERM_DIST = 0.25
POWER_COEF = 0.0005
SPECS = {"k_pos": 100.0, "k_rot": 10.0, "k_vel": 0.1, "k_ang_vel": 0.1, "w_pos": 0.5, "w_rot": 0.3, "w_vel": 0.1, "w_ang_vel": 0.1}
SK = syn.SKELETONS["smplx"]
J, ND = SK["num_bodies"], SK["num_dof"]
TRACK_VR = [SK["body_names"].index(b) for b in ("Head", "L_Wrist", "R_Wrist")]
# pelvis, both hips and knees, the spine chain, both arms down to the wrists
RESET_NAMES = ["Pelvis", "L_Hip", "L_Knee", "R_Hip", "R_Knee", "Torso", "Spine", "Chest", "Neck", "Head",
               "L_Thorax", "L_Shoulder", "L_Elbow", "L_Wrist", "R_Thorax", "R_Shoulder", "R_Elbow", "R_Wrist"]
RESET_IDS = [SK["body_names"].index(b) for b in RESET_NAMES]


def near_reference(g, rb, samples=1, move_every=3, pos_sigma=0.06, rot_sigma=0.15, vel_sigma=1.5, move=0.3):
    """References near ``rb`` (n, j, 13) by the recipe above -> dict pos / rot / vel / ang, each (n * samples, j, .), env-major."""
    n, j, _ = rb.shape
    x = rb[:, None].expand(n, samples, j, 13)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    pos = x[..., 0:3] + pos_sigma * randn(n, samples, j, 3)
    pos[::move_every, :, :, 0] += move
    rot = x[..., 3:7] + rot_sigma * randn(n, samples, j, 4)
    rot = rot / rot.norm(dim=-1, keepdim=True)
    vel = x[..., 7:10] + vel_sigma * randn(n, samples, j, 3)
    ang = x[..., 10:13] + vel_sigma * randn(n, samples, j, 3)
    return {k: v.reshape(n * samples, j, -1).contiguous() for k, v in (("pos", pos), ("rot", rot), ("vel", vel), ("ang", ang))}


def inputs(n=N, j=J, seed=SEED, samples=T):
    """Everything one post-physics step reads, for n envs of a j-body humanoid."""
    g = syn.make_generator(seed)
    rb = syn.rigid_body_state(g, n, j)
    ref_now = near_reference(g, rb)
    ref_next = near_reference(g, rb, samples)
    nd = 3 * (j - 1)
    return {"rb": rb, "ref_now": ref_now, "ref_next": ref_next,
            "dof_force": 50.0 * torch.randn(n, nd, generator=g), "dof_vel": torch.randn(n, nd, generator=g),
            "progress": torch.randint(0, 10, (n,), generator=g, dtype=torch.int64), "pass_time": torch.rand(n, generator=g) < 0.2}


def first_sample(ref, n, samples=T):
    """The T = 1 reference: sample 0 of every env."""
    return {k: v.view(n, samples, *v.shape[1:])[:, 0].contiguous() for k, v in ref.items()}


def input_sums(d):
    flat = {"rb": d["rb"], "dof_force": d["dof_force"], "dof_vel": d["dof_vel"], "progress": d["progress"], "pass_time": d["pass_time"]}
    flat.update({f"ref_now_{k}": v for k, v in d["ref_now"].items()})
    flat.update({f"ref_next_{k}": v for k, v in d["ref_next"].items()})
    return {f"sum_{k}": v.double().sum() for k, v in flat.items()}


def check_conditions(raw, terminate, dist, threshold=TERM_DIST):
    """The conditions that keep a fixture (or a test's own draw) from hiding a failure; AssertionError otherwise."""
    n = raw.shape[0]
    for c in range(4):
        inside = ((raw[:, c] > 0.01) & (raw[:, c] < 0.99)).sum().item()
        assert 2 * inside >= n, f"raw reward term {c} saturates: only {inside} of {n} envs inside (0.01, 0.99)"
    share = terminate.double().mean().item()
    assert 0.15 <= share <= 0.85, f"terminated share {share:.2f} outside [0.15, 0.85]"
    gap = (dist - threshold).abs().min().item()
    assert gap >= 1e-4, f"a reset distance sits {gap:.2e} from the threshold: the flag would hang on rounding"


def reference_v6_three_samples_upright():
    """The one variant the fixture does not hold: compute_imitation_observations_v6 at T = 3 with upright start.  Its 494 KB would take the
    file past the size limit for a committed file, so the CPU test evaluates it here when the reference is present (and holds the oracle to
    it bit for bit), and the GPU test compares the kernel with the oracle."""
    from oracle import refload
    fn = refload.env_functions()
    d = inputs()
    rb, rx = d["rb"], d["ref_next"]
    bp, br, bv, ba = (rb[..., a:b].contiguous() for a, b in ((0, 3), (3, 7), (7, 10), (10, 13)))
    return fn["compute_imitation_observations_v6"](bp[:, 0], br[:, 0], bp, br, bv, ba, rx["pos"], rx["rot"], rx["vel"], rx["ang"], T, True).numpy()


def generate():
    from oracle import refload
    fn = refload.env_functions()
    d = inputs()
    rb = d["rb"]
    bp, br, bv, ba = (rb[..., a:b].contiguous() for a, b in ((0, 3), (3, 7), (7, 10), (10, 13)))
    rn, rx3 = d["ref_now"], d["ref_next"]
    rx1 = first_sample(rx3, N)
    empty = torch.zeros(N, 0)
    sub = lambda x, ids: x[:, ids].contiguous()
    out = dict(input_sums(d))
    for up in (True, False):
        tag = "" if up else "_noup"
        out["self_obs" + tag] = fn["compute_humanoid_observations_smpl_max"](bp, br, bv, ba, empty, empty, True, True, up, False, False)
        for t, rx in ((1, rx1), (3, rx3)):
            if t == 1 or not up:       # T = 3 upright (494 KB more) is not stored: reference_v6_three_samples_upright
                out[f"v6_T{t}{tag}"] = fn["compute_imitation_observations_v6"](bp[:, 0], br[:, 0], bp, br, bv, ba, rx["pos"], rx["rot"], rx["vel"],
                                                                               rx["ang"], t, up)
            tb = TRACK_VR
            out[f"v7_T{t}_vr{tag}"] = fn["compute_imitation_observations_v7"](bp[:, 0], br[:, 0], sub(bp, tb), sub(bv, tb), sub(rx["pos"], tb),
                                                                              sub(rx["vel"], tb), t, up)
    rew, raw = fn["compute_imitation_reward"](bp[:, 0], br[:, 0], bp, br, bv, ba, rn["pos"], rn["rot"], rn["vel"], rn["ang"], dict(SPECS))
    # the power term as HumanoidIm._compute_reward forms it (humanoid_im.py:908-917), 153 dofs
    power = torch.abs(torch.multiply(d["dof_force"], d["dof_vel"])).sum(dim=-1)
    power_reward = -POWER_COEF * power
    power_reward[d["progress"] <= 3] = 0
    out.update({"reward_im": rew, "reward_raw_im": raw, "reward": rew + power_reward, "reward_raw": torch.cat([raw, power_reward[:, None]], dim=-1)})
    term_dist = torch.full((1, J), TERM_DIST)
    rid = RESET_IDS
    for use_mean, tag in ((False, ""), (True, "_mean")):
        reset, terminate = fn["compute_humanoid_im_reset"](torch.zeros(N, dtype=torch.int64), d["progress"], torch.zeros(N, J, 3), torch.tensor([7, 3, 8, 4]),
                                                           sub(bp, rid), sub(rn["pos"], rid), d["pass_time"], True, term_dist[..., rid], False, use_mean)
        out["reset" + tag], out["terminate" + tag] = reset, terminate
    dist = torch.norm(sub(bp, rid) - sub(rn["pos"], rid), dim=-1)
    check_conditions(raw, out["terminate"], torch.cat([dist.flatten(), dist.mean(dim=-1)]))
    print(f"raw reward terms in [{raw.min().item():.3f}, {raw.max().item():.3f}]; terminated {out['terminate'].double().mean().item():.2f}, "
          f"reset {out['reset'].double().mean().item():.2f}; smallest |distance - {TERM_DIST}| {(dist - TERM_DIST).abs().min().item():.2e}")
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    path = os.path.join(a.out, "env_smplx.npz")
    np.savez_compressed(path, **generate())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
