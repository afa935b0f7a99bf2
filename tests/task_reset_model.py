"""Plain-torch model of the reference-state reset of the downstream tasks (TEST INFRASTRUCTURE -- never imported by pulse_amd).

The four _sample_ref_state / _reset_ref_state_init variants of the reference, statement for statement on oracle.rotations,
oracle.motion_oracle.OracleMotionLib and oracle.task_oracle.terrain_center_heights:
  none            HumanoidAMP                  phc/env/tasks/humanoid_amp.py:447-488     (HumanoidTraj)
  zero_xy         HumanoidReach / Strike       humanoid_reach.py:46-49, humanoid_strike.py:147-150
  remove_heading  HumanoidSpeed                humanoid_speed.py:251-270
  terrain         HumanoidPedestrianTerrain    humanoid_pedestrian_terrain.py:488-589
``ref_state`` returns
  * the ROOT STATE the reference hands to the simulator (root_pos / root_rot / root_vel / root_ang_vel), dof_pos / dof_vel, ids and times:
    tests/test_task_reset_cpu.py pins these to the reference's own method bodies bit for bit;
  * ``cache``: the bodies the reference writes into its transient _rigid_body_* cache (rb_pos, rb_rot, body_vel, body_ang_vel);
  * ``records`` (n, J, 13): what pulse_task_ref_state_init writes -- body 0 is that root state, every other body is carried rigidly by
    the same root transform.  It differs from ``cache`` in three documented places (include/pulse_hip.h): speed turns body_ang_vel too;
    reach / strike translate the bodies with the root; terrain lifts the bodies with the root.
fix_trans_height (_get_fixed_smpl_state_from_motionlib: SMPL mesh parsers) is out of scope: the motion's heights are used as they are.
"""
import torch

from oracle import rotations as R
from oracle import task_oracle as TO
from oracle.env_oracle import remove_base_rot

TRANSFORMS = ("none", "zero_xy", "remove_heading", "terrain")


def ref_state(lib, motion_ids, motion_times, transform, upright=True, new_root_xy=None, heightsamples=None, center_points=None,
              horizontal_scale=0.1, vertical_scale=0.005):
    """``lib``: an OracleMotionLib; ``center_points`` (P, 3) with zero z, as get_center_heights holds them."""
    assert transform in TRANSFORMS
    st = lib.get_motion_state(motion_ids, motion_times)
    root_pos, root_rot, dof_pos = st["root_pos"].clone(), st["root_rot"].clone(), st["dof_pos"].clone()
    root_vel, root_ang_vel, dof_vel = st["root_vel"].clone(), st["root_ang_vel"].clone(), st["dof_vel"].clone()
    rb_pos, rb_rot, body_vel, body_ang_vel = st["rg_pos"].clone(), st["rb_rot"].clone(), st["body_vel"].clone(), st["body_ang_vel"].clone()
    n, j = rb_pos.shape[0], rb_pos.shape[1]
    # the rigidly carried bodies start from the motion's and follow the root transform below
    c_pos, c_rot, c_vel, c_ang = rb_pos.clone(), rb_rot.clone(), body_vel.clone(), body_ang_vel.clone()
    center_height = torch.zeros(n)
    if transform == "zero_xy":
        c_pos[..., 0:2] = c_pos[..., 0:2] - root_pos[:, None, 0:2]
        root_pos[..., :2] = 0.0                                                   # humanoid_reach.py:48
    elif transform == "remove_heading":
        h_inv = R.heading_q_inv(root_rot if upright else remove_base_rot(root_rot))                 # humanoid_speed.py:255-258
        h_rep = h_inv[:, None].repeat(1, j, 1)
        rep = lambda f, x: f(h_rep.reshape(-1, 4), x.reshape(-1, x.shape[-1])).view(x.shape)
        root_rot = R.qmul(h_inv, root_rot).clone()
        rb_pos = rep(TO.quat_apply, rb_pos - root_pos[:, None, :]).clone() + root_pos[:, None, :]
        rb_rot = rep(R.qmul, rb_rot).clone()
        root_ang_vel = TO.quat_apply(h_inv, root_ang_vel).clone()
        root_vel = TO.quat_apply(h_inv, root_vel).clone()
        body_vel = rep(TO.quat_apply, body_vel).clone()
        c_pos, c_rot, c_vel = rb_pos.clone(), rb_rot.clone(), body_vel.clone()
        c_ang = rep(TO.quat_apply, body_ang_vel)                                  # (the reference returns body_ang_vel as it was)
    elif transform == "terrain":
        diff_xy = new_root_xy - root_pos[:, 0:2]                                  # humanoid_pedestrian_terrain.py:553-563
        root_pos[:, 0:2] = new_root_xy
        root_states = torch.cat([root_pos, root_rot], dim=1)
        if heightsamples is not None:
            center_height = TO.terrain_center_heights(heightsamples, root_states, center_points, horizontal_scale, vertical_scale, upright).mean(dim=-1)
        root_pos[:, 2] += center_height
        rb_pos[..., 0:2] += diff_xy[:, None, :]                                   # :566 (never lifted; key_pos is lifted twice instead)
        c_pos = rb_pos.clone()
        c_pos[..., 2] += center_height[:, None]
    records = torch.cat([c_pos, c_rot, c_vel, c_ang], dim=-1)
    records[:, 0] = torch.cat([root_pos, root_rot, root_vel, root_ang_vel], dim=-1)
    return {"motion_ids": motion_ids, "motion_times": motion_times, "root_pos": root_pos, "root_rot": root_rot, "root_vel": root_vel,
            "root_ang_vel": root_ang_vel, "dof_pos": dof_pos, "dof_vel": dof_vel, "records": records, "center_height": center_height,
            "cache": {"rb_pos": rb_pos, "rb_rot": rb_rot, "body_vel": body_vel, "body_ang_vel": body_ang_vel},
            "motion": {"rb_pos": st["rg_pos"], "rb_rot": st["rb_rot"], "body_vel": st["body_vel"], "body_ang_vel": st["body_ang_vel"]}}


def heading_axis_xy(lib, motion_ids, motion_times, upright=True):
    """Length of the horizontal projection of every root's heading axis (calc_heading takes atan2 of it; undefined at 0)."""
    q = lib.get_motion_state(motion_ids, motion_times)["root_rot"]
    if not upright:
        q = remove_base_rot(q)
    x = torch.zeros(q.shape[0], 3)
    x[:, 0] = 1.0
    return R.qrot(q, x)[:, 0:2].norm(dim=-1)


def center_sample_cells(root_states, center_points, horizontal_scale=0.1, upright=True):
    """Cell coordinates (n, P, 2) of get_center_heights' grid points, as TO.terrain_center_heights forms them (before truncation)."""
    q = (root_states[:, 3:7] if upright else remove_base_rot(root_states[:, 3:7])).clone()
    q[:, :2] = 0.0
    q = q / q.norm(p=2, dim=-1).clamp(min=1e-9).unsqueeze(-1)
    n, p = root_states.shape[0], center_points.shape[0]
    pts = TO.quat_apply(q.unsqueeze(1).expand(n, p, 4).reshape(-1, 4), center_points.unsqueeze(0).expand(n, p, 3).reshape(-1, 3)).view(n, p, 3)
    pts = pts + root_states[:, :3].unsqueeze(1)
    return pts[..., 0:2] / horizontal_scale
