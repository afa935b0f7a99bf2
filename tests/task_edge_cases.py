"""Seeded inputs for the edge tests of the task / terrain step kernels (test_task_edges_oracle.py pins the CPU oracle to the reference on them,
test_task_edges_gpu.py holds pulse_task_step / pulse_traj_step / pulse_traj_generate to the oracle on them).  CPU tensors only.

Flags are compared bit for bit, which is only meaningful when no input sits on a decision threshold: the builders move random values out
of a band around each threshold and the ``*_margins`` functions assert, in fp64, that every thresholded quantity is at least 1e-3
(relative; absolute for the threshold 0) away from it."""
import numpy as np
import torch

from oracle import task_oracle as TO
from pulse_amd import synthetic as syn

MAP_ROWS, MAP_COLS, HSCALE, VSCALE = 260, 300, 0.1, 0.005              # syn.synthetic_height_field: 26 m x 30 m in cells of 0.1 m
HEAD = syn.SMPL_BODY_NAMES.index("Head")
CONTACT_IDS = torch.tensor([7, 3, 8, 4])
STRIKE_IDS = torch.tensor([23, 22, 21])
TERM_H = 0.15
REL = 1e-3


def pad3(p):
    return torch.cat([p, torch.zeros(p.shape[0], 1)], 1) if p.shape[1] == 2 else p


def push_off(x, thr, band=5e-3):
    """Every value whose magnitude lies within ``band`` (relative) of ``thr`` grows by 1 %: at least 0.49 % past the threshold."""
    return torch.where((x.abs() - thr).abs() < band * thr, x * 1.01, x)


def assert_off(x, thr, what):
    x = x.double()
    gap = (x - thr).abs().min().item() if x.numel() else float("inf")
    assert gap >= REL * (abs(thr) if thr else 1.0), f"{what}: an input sits {gap:.3e} from the threshold {thr}"


def _nonfoot(t):
    keep = torch.ones(t.shape[1], dtype=torch.bool)
    keep[CONTACT_IDS] = False
    return t[:, keep]


# ---------------------------------------------------------------------------------------------------------------------
# pulse_task_step: speed / reach / strike, n = 300 = one full 256-thread block and a ragged one of 44
# ---------------------------------------------------------------------------------------------------------------------
CASE_BLOCKS = (10, 260)                   # first env of the deliberate cases in the first and in the second block


def task_inputs(n=300, seed=556):
    """As oracle/gen_golden.py: gen_tasks builds its inputs, with its deliberate cases placed once per block (CASE_BLOCKS + k):
    k 0-4 upright strike targets, 5-9 knocked-over ones, 10-11 the root moving away from the target (dir_speed <= 0), 12-14 a fall at progress
    0 / 1 / 2, 15-17 progress 298 / 299 / 304 without a fall, 18 a body below its termination height without a contact, 19 with a non-foot
    contact, 20 a target contact with a non-strike contact, 21 a target contact with a contact on a strike body only."""
    g = syn.make_generator(seed)
    rb_rand = syn.rigid_body_state(g, n)
    root = rb_rand[:, 0].clone()
    prev_root = root[:, 0:3] + 0.02 * torch.randn(n, 3, generator=g)
    tar_speed = 1.0 + 2.0 * torch.rand(n, generator=g)
    tar_pos = root[:, 0:3] + torch.randn(n, 3, generator=g)
    tar_states = syn.rigid_body_state(g, n)[:, 0].clone()
    contact = torch.randn(n, 24, 3, generator=g) * (torch.rand(n, 24, 1, generator=g) < 0.3)
    contact[::4] *= 100.0
    tar_contact = torch.randn(n, 3, generator=g) * 60.0
    progress = torch.randint(0, 305, (n,), generator=g)
    body_pos = rb_rand[..., 0:3].clone()
    body_pos[::3, 5, 2] = 0.05
    for o in CASE_BLOCKS:
        tar_states[o:o + 5, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0])
        tar_states[o + 5:o + 10, 3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0])
        away = slice(o + 10, o + 12)
        d = torch.nn.functional.normalize(tar_states[away, 0:2] - root[away, 0:2], dim=-1)
        prev_root[away, 0:2] = root[away, 0:2] + 0.03 * d
        quiet = slice(o + 12, o + 22)
        contact[quiet], tar_contact[quiet], progress[quiet] = 0.0, 0.0, 50
        body_pos[quiet, :, 2] = 0.5
        progress[o + 12:o + 18] = torch.tensor([0, 1, 2, 298, 299, 304])
        body_pos[o + 12:o + 15, 5, 2] = 0.05
        contact[o + 12:o + 15, 10] = torch.tensor([0.5, 0.0, 0.0])
        body_pos[o + 18, 5, 2] = 0.05
        body_pos[o + 19, 5, 2] = 0.05
        contact[o + 19, 10] = torch.tensor([0.0, 0.5, 0.0])
        tar_contact[o + 20] = torch.tensor([70.0, 0.0, 0.0])
        contact[o + 20, 11] = torch.tensor([0.0, 80.0, 0.0])
        tar_contact[o + 21] = torch.tensor([0.0, -70.0, 0.0])
        contact[o + 21, 23] = torch.tensor([0.0, 0.0, 100.0])
    contact = push_off(push_off(contact, 0.1), 50.0)
    tar_contact = push_off(tar_contact, 50.0)
    z = body_pos[..., 2]
    body_pos[..., 2] = torch.where((z - TERM_H).abs() < 5e-3 * TERM_H, z + 0.01, z)
    rb = torch.zeros(n, 24, 13)
    rb[..., 0:3] = body_pos
    rb[:, 0] = root
    rb[:, 23, 7:10] = rb_rand[:, 23, 7:10]
    return {"n": n, "rb": rb, "prev_root_pos": prev_root, "tar_speed": tar_speed, "tar_pos": tar_pos, "tar_states": tar_states, "contact": contact,
            "tar_contact": tar_contact, "progress": progress, "term_h": torch.full((24,), TERM_H), "dt": 1.0 / 30.0}


def _strike_scalars(d, dtype):
    """tar_rot_err and tar_dir_speed as compute_strike_reward forms them (humanoid_strike.py:305-318)."""
    ts, root, prev = d["tar_states"].to(dtype), d["rb"][:, 0].to(dtype), d["prev_root_pos"].to(dtype)
    up = torch.zeros_like(ts[:, 0:3])
    up[:, 2] = 1
    rot_err = torch.sum(up * TO._quat_rotate_isaac(ts[:, 3:7], up), dim=-1)
    tar_dir = torch.nn.functional.normalize(ts[:, 0:2] - root[:, 0:2], dim=-1)
    return rot_err, torch.sum(tar_dir * ((root[:, 0:3] - prev) / d["dt"])[:, :2], dim=-1)


def task_margins(d):
    c = _nonfoot(d["contact"]).abs()
    assert_off(c, 0.1, "contact force")
    assert_off(c, 50.0, "contact force")
    assert_off(d["tar_contact"][:, 0:2].abs(), 50.0, "target contact force")
    assert_off(_nonfoot(d["rb"][..., 2]), TERM_H, "body height")
    rot_err, dir_speed = _strike_scalars(d, torch.float64)
    assert_off(rot_err, 0.2, "strike rot_err")
    assert_off(dir_speed, 0.0, "strike dir_speed")


def task_expected(d):
    rb, prev, dt = d["rb"], d["prev_root_pos"], d["dt"]
    root, bp, z0 = rb[:, 0], rb[..., 0:3], torch.zeros(d["n"], dtype=torch.long)
    e = {"speed_obs": TO.speed_observations(root, d["tar_speed"]),
         "speed_rew": TO.speed_reward(root[:, 0:3], prev, root[:, 3:7], d["tar_speed"], dt),
         "reach_obs": TO.location_observations(root, d["tar_pos"]),
         "reach_rew": TO.reach_reward(bp[:, 23], root[:, 3:7], d["tar_pos"], 1.0, dt),
         "strike_obs": TO.strike_observations(root, d["tar_states"]),
         "strike_rew": TO.strike_reward(d["tar_states"][:, 0:3], d["tar_states"][:, 3:7], root, prev, rb[:, 23, 7:10], dt, 1.4)}
    e["reset"], e["terminated"] = TO.humanoid_reset(z0, d["progress"], d["contact"], CONTACT_IDS, bp, 300.0, True, d["term_h"])
    e["reset_noearly"], _ = TO.humanoid_reset(z0, d["progress"], d["contact"], CONTACT_IDS, bp, 300.0, False, d["term_h"])
    e["strike_reset"], e["strike_terminated"] = TO.strike_reset(z0, d["progress"], d["contact"], CONTACT_IDS, bp, d["tar_contact"], STRIKE_IDS, 300.0,
                                                                True, d["term_h"])
    return e


def power_inputs(n, num_dof, seed=3):
    g = syn.make_generator(seed + num_dof)
    df, dv = torch.randn(n, num_dof, generator=g) * 50, torch.randn(n, num_dof, generator=g)
    return df, dv, -0.0005 * (df.double() * dv.double()).abs().sum(-1)


# ---------------------------------------------------------------------------------------------------------------------
# pulse_traj_step: 48 humanoids around the border of the height field
# ---------------------------------------------------------------------------------------------------------------------
def edge_placement(seed=77):
    """(48, 24, 13) rigid-body states whose root stands at seeded, non-round positions: five per border of the 26 m x 30 m map (a +-2 m
    sensor grid straddles it), three per corner, three far outside on the negative and on the positive side, ten well inside."""
    X, Y = MAP_ROWS * HSCALE, MAP_COLS * HSCALE
    groups = [(0.0, Y / 2, 1.2, 9.0, 5), (X, Y / 2, 1.2, 9.0, 5), (X / 2, 0.0, 8.0, 1.2, 5), (X / 2, Y, 8.0, 1.2, 5),
              (0.0, 0.0, 1.2, 1.2, 3), (X, Y, 1.2, 1.2, 3), (0.0, Y, 1.2, 1.2, 3), (X, 0.0, 1.2, 1.2, 3),
              (-40.0, -35.0, 3.0, 3.0, 3), (60.0, 70.0, 3.0, 3.0, 3), (X / 2, Y / 2, 8.0, 10.0, 10)]
    g = syn.make_generator(seed)
    n = sum(k for *_, k in groups)
    rb = syn.rigid_body_state(g, n)
    u = 2 * torch.rand(n, 2, generator=g) - 1
    anchor = torch.tensor([[ax, ay] for ax, ay, _, _, k in groups for _ in range(k)])
    jitter = torch.tensor([[jx, jy] for _, _, jx, jy, k in groups for _ in range(k)])
    rb[:, :, 0:2] += (anchor + jitter * u - rb[:, 0, 0:2])[:, None, :]
    return rb


def sensor_points(rb, hp, sensor_body, upright):
    return TO.terrain_sample_points(rb[:, sensor_body, 0:7], pad3(hp), upright)


def center_points_world(rb, cp, upright):
    """World positions of get_center_heights' grid, as TO.terrain_center_heights forms them."""
    q = TO._base_rot(rb[:, 0, 3:7], upright).clone()
    q[:, :2] = 0.0
    q = q / q.norm(p=2, dim=-1).clamp(min=1e-9).unsqueeze(-1)
    n, p = rb.shape[0], cp.shape[0]
    pts = TO.quat_apply(q.unsqueeze(1).expand(n, p, 4).reshape(-1, 4), pad3(cp).unsqueeze(0).expand(n, p, 3).reshape(-1, 3)).view(n, p, 3)
    return pts + rb[:, 0, :3].unsqueeze(1)


def on_edge(pts, hscale=HSCALE):
    """Per sample: does its fp32 cell coordinate lie within 8 ulps of an integer in x or y?  Only such a sample can land in the neighbouring
    cell when the rotation of the sensor grid is evaluated with another sinf / cosf / atan2f."""
    u = (pts[..., :2] / hscale).numpy()
    return torch.from_numpy((np.abs(u - np.rint(u)) <= 8 * np.spacing(np.abs(u))).any(-1))


def unclipped(pts, hscale=HSCALE, rows=MAP_ROWS, cols=MAP_COLS):
    """Per sample: is its truncated cell index inside [0, size - 2] in x and in y (neither clip of world_points_to_map acts)?"""
    c = (pts[..., :2] / hscale).long()
    return (c[..., 0] >= 0) & (c[..., 0] <= rows - 2) & (c[..., 1] >= 0) & (c[..., 1] <= cols - 2)


def traj_draws(n, num_verts, seed):
    g = syn.make_generator(seed)
    u = {"dtheta": torch.rand(n, num_verts - 1, generator=g), "sharp": torch.rand(n, num_verts - 1, generator=g)}
    u["sharp_mask"] = torch.rand(n, num_verts - 1, generator=g) < 0.02
    u["heading"], u["dspeed"], u["speed0"] = torch.rand(n, generator=g), torch.rand(n, num_verts - 1, generator=g), torch.rand(n, generator=g)
    return u


def verts_from_draws(root_pos, u, traj_dt, dtheta_max=2.0, accel_max=2.0, speed_min=0.0, speed_max=3.0):
    """The uniform draws mapped as TrajGenerator.reset maps them (traj_generator.py:66-88), then TO.traj_from_draws."""
    import math
    dtheta = (2 * u["dtheta"] - 1.0) * (dtheta_max * traj_dt)
    sharp = math.pi * (2 * u["sharp"] - 1.0)
    dtheta[u["sharp_mask"]] = sharp[u["sharp_mask"]]
    dtheta[:, 0] = math.pi * (2 * u["heading"] - 1.0)
    dspeed = (2 * u["dspeed"] - 1.0) * (accel_max * traj_dt)
    dspeed[:, 0] = (speed_max - speed_min) * u["speed0"] + speed_min
    return TO.traj_from_draws(root_pos, dtheta, dspeed, traj_dt, speed_min, speed_max)


EPISODE_DUR, NUM_VERTS, STEP_DT, FAIL_DIST = 300 * (2.0 / 60.0), 101, 2.0 / 60.0, 4.0


def terrain_scene(seed=78):
    """The edge placement with a trajectory per env (the golden's vertex count, speeds and duration), a clock and the reset inputs of
    oracle/gen_golden.py: gen_terrain (a foot contact, a summed non-foot contact above 50 N, a light non-foot contact on a low body)."""
    rb = edge_placement()
    n = rb.shape[0]
    traj_dt = EPISODE_DUR / (NUM_VERTS - 1)
    verts = verts_from_draws(rb[:, 0, 0:3], traj_draws(n, NUM_VERTS, seed), traj_dt)
    g = syn.make_generator(seed + 1)
    progress = torch.randint(0, 300, (n,), generator=g)
    progress[:3] = torch.tensor([0, 1, 299])
    progress[-3:] = torch.tensor([2, 298, 304])
    contact = torch.zeros(n, 24, 3)
    contact[::3, 7] = torch.tensor([10.0, 0.0, 400.0])
    contact[1::4, 12] = torch.tensor([30.0, 30.0, 30.0])
    contact[2::5, 16] = torch.tensor([0.3, 0.0, 0.0])
    rb = rb.clone()
    rb[2::5, 16, 2] = 0.05
    z = rb[..., 2]
    rb[..., 2] = torch.where((z - TERM_H).abs() < 5e-3 * TERM_H, z + 0.01, z)
    return {"n": n, "rb": rb, "verts": verts, "progress": progress, "contact": contact, "term_h": torch.full((24,), TERM_H), "traj_dt": traj_dt,
            "hs": syn.synthetic_height_field()}


def traj_margins(rb, tar_pos64, contact, fail_dist):
    """The thresholds of both compute_humanoid_reset variants (humanoid_pedestrian_terrain.py:1476-1531, humanoid_traj.py:267-301)."""
    nf = _nonfoot(contact).double()
    assert_off(nf.abs(), 0.1, "contact force")
    assert_off(torch.sqrt(torch.square(nf.sum(dim=-2).abs()).sum(dim=-1)), 50.0, "summed contact force")
    assert_off(_nonfoot(rb[..., 2]), TERM_H, "body height")
    d = tar_pos64[:, 0:2] - rb[:, 0, 0:2].double()
    assert_off((d * d).sum(-1), fail_dist * fail_dist, "squared distance to the target")
