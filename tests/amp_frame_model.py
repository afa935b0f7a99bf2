"""Plain-torch restatement of the AMP frame in all its configured forms (TEST INFRASTRUCTURE -- never imported by pulse_amd).

  * ``amp_frame``: build_amp_observations_smpl (phc/env/tasks/humanoid_amp.py:925-969) and build_amp_observations_smpl_v2 (:973-1017) in one
    function: remove_base_rot for a non-upright start (:929-930; humanoid.py:1617-1620), the heading-local key-body velocities of version 2
    (:999, 1009), the shape / limb rows behind everything else (:963-966).  Same operations in the same order on oracle.rotations, so it is
    held to tests/golden/env_amp_variants.npz (written by the reference's own functions) BIT FOR BIT (tests/test_amp_variants_cpu.py).
  * ``AmpWindow``: the (N, S, W) window of HumanoidAMP over it -- _compute_amp_observations (:632-667), _update_hist_amp_obs (:622-631),
    _init_amp_obs_ref (:535-563, the MOTION's rows) / _init_amp_obs_default (:530-533) -- and build_amp_obs_demo (:253-284).
"""
import torch

from oracle import env_oracle as E
from oracle import rotations as R


def remove_base_rot(quat):
    """humanoid.py:1617-1620."""
    base_rot = R.qconj(torch.tensor([[0.5, 0.5, 0.5, 0.5]]).to(quat))
    return R.qmul(quat, base_rot.repeat(quat.shape[0], 1))


def non_upright_tables(tables):
    """Motion tables of a humanoid WITHOUT upright start: the root's rotations carry the base rotation remove_base_rot takes off again
    (root_rot = upright_rot * (0.5, 0.5, 0.5, 0.5)).  The upright tables themselves would be degenerate input for the non-upright frame:
    remove_base_rot turns the heading's reference axis of an upright root into the vertical, where the heading angle is atan2(~0, ~0)."""
    base = torch.tensor([[0.5, 0.5, 0.5, 0.5]])
    out = dict(tables)
    for k in ("grs", "lrs"):
        t = tables[k].clone()
        t[:, 0] = R.qmul(t[:, 0], base.repeat(t.shape[0], 1))
        out[k] = t
    return out


def amp_frame(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_body_pos, key_body_vel=None, shape_params=None, limb_weights=None,
              dof_subset=None, local_root_obs=True, root_height_obs=True, upright=True, version=1):
    """``shape_params`` is the already truncated (B, 11) view (smpl_params[:, :-6], :672); None = has_shape_obs_disc False."""
    if not upright:
        root_rot = remove_base_rot(root_rot)
    h_inv = R.heading_q_inv(root_rot)
    rot6 = R.q_to_tan_norm(R.qmul(h_inv, root_rot) if local_root_obs else root_rot)
    lvel = R.qrot(h_inv, root_vel)
    lang = R.qrot(h_inv, root_ang_vel)
    rel = key_body_pos - root_pos.unsqueeze(-2)
    nk = rel.shape[1]
    h_e = h_inv.unsqueeze(-2).repeat((1, nk, 1)).view(-1, 4)
    parts = [root_pos[:, 2:3]] if root_height_obs else []
    if dof_subset is not None:
        dof_vel = dof_vel[:, dof_subset]
        dof_pos = dof_pos[:, dof_subset]
    parts += [rot6, lvel, lang, E.dof_to_obs_smpl(dof_pos), dof_vel, R.qrot(h_e, rel.reshape(-1, 3)).view(rel.shape[0], nk * 3)]
    if version == 2:
        parts.append(R.qrot(h_e, key_body_vel.reshape(-1, 3)).view(rel.shape[0], nk * 3))
    if shape_params is not None:
        parts.append(shape_params)
    if limb_weights is not None:
        parts.append(limb_weights)
    return torch.cat(parts, dim=-1)


def frame_from_records(rb, dof_pos, dof_vel, key, shape_params=None, limb_weights=None, **kw):
    """``amp_frame`` on (B, bodies, 13) rigid-body records (root = body 0)."""
    key = torch.as_tensor(key, dtype=torch.long)
    return amp_frame(rb[:, 0, 0:3], rb[:, 0, 3:7], rb[:, 0, 7:10], rb[:, 0, 10:13], dof_pos, dof_vel, rb[:, key, 0:3], rb[:, key, 7:10],
                     shape_params, limb_weights, **kw)


def frame_width(num_joints=23, num_key_bodies=4, root_height_obs=True, version=1, has_dof_subset=False, has_shape_obs_disc=False, has_limb_weight_obs_disc=False,
                subset_dofs=57):
    """_num_amp_obs_per_step, humanoid_amp.py:299-314, statement by statement (smpl_humanoid.xml: 11 shape columns)."""
    dof_obs_size, num_dof_names = 6 * num_joints, num_joints
    w = 13 + dof_obs_size + num_dof_names * 3 + (3 if version == 1 else 6) * num_key_bodies
    if not root_height_obs:
        w -= 1
    if has_dof_subset:
        w -= (6 + 3) * int((num_dof_names * 3 - subset_dofs) / 3)
    if has_shape_obs_disc:
        w += 11
    if has_limb_weight_obs_disc:
        w += 10
    return w


class AmpWindow:
    """The AMP observation window of HumanoidAMP.  ``lib``: an OracleMotionLib; ``motion_bodies`` (M, 17) / ``motion_limb_weights`` (M, 10):
    the motions' rows; ``shapes`` (N, 17) / ``limbs`` (N, 10): the envs' rows (humanoid_shapes / humanoid_limb_and_weights)."""

    def __init__(self, lib, motion_ids, num_steps, dt, key_body_ids, dof_subset=None, shapes=None, limbs=None, motion_bodies=None, motion_limb_weights=None,
                 has_shape_obs_disc=False, has_limb_weight_obs_disc=False, **frame_kw):
        self.lib, self.ids, self.s, self.dt, self.key = lib, motion_ids, num_steps, dt, torch.as_tensor(key_body_ids, dtype=torch.long)
        self.kw = dict(frame_kw, dof_subset=dof_subset)
        self.shapes = shapes[:, :-6] if has_shape_obs_disc and shapes is not None else None
        self.limbs = limbs if has_limb_weight_obs_disc else None
        self.m_shapes = motion_bodies[:, :-6] if has_shape_obs_disc and motion_bodies is not None else None
        self.m_limbs = motion_limb_weights if has_limb_weight_obs_disc and motion_limb_weights is not None else None
        self.buf = None

    def _sim_frame(self, rb, dof_pos, dof_vel, env_ids=slice(None)):
        return frame_from_records(rb[env_ids], dof_pos[env_ids], dof_vel[env_ids], self.key, self.shapes[env_ids] if self.shapes is not None else None,
                                  self.limbs[env_ids] if self.limbs is not None else None, **self.kw)

    def motion_frames(self, motion_ids, times):
        """Frames of reference motion (one per id / time), wearing the motion's rows (:243-250, 548-555)."""
        st = self.lib.get_motion_state(motion_ids, times)
        recs = torch.cat([st["rg_pos"], st["rb_rot"], st["body_vel"], st["body_ang_vel"]], dim=-1)
        return frame_from_records(recs, st["dof_pos"], st["dof_vel"], self.key, self.m_shapes[motion_ids] if self.m_shapes is not None else None,
                                  self.m_limbs[motion_ids] if self.m_limbs is not None else None, **self.kw)

    def step(self, rb, dof_pos, dof_vel):
        self.buf[:, 1:] = self.buf[:, 0:self.s - 1].clone()
        self.buf[:, 0] = self._sim_frame(rb, dof_pos, dof_vel)
        return self.buf.view(self.buf.shape[0], -1)

    def reset(self, env_ids, rb, dof_pos, dof_vel, start_times, from_motion=True):
        if len(env_ids) == 0:
            return
        cur = self._sim_frame(rb, dof_pos, dof_vel, env_ids)
        if self.buf is None:
            self.buf = torch.zeros(rb.shape[0], self.s, cur.shape[1])
        self.buf[env_ids, 0] = cur
        if from_motion:
            k = self.s - 1
            ids = self.ids[env_ids].repeat_interleave(k)
            times = (start_times[env_ids].unsqueeze(-1) + (-self.dt * (torch.arange(0, k) + 1))).view(-1)
            self.buf[env_ids, 1:] = self.motion_frames(ids, times).view(len(env_ids), k, -1)
        else:
            self.buf[env_ids, 1:] = cur.unsqueeze(-2)

    def demo(self, motion_ids, times0):
        """build_amp_obs_demo (:253-284) without the input noise."""
        ids = motion_ids.repeat_interleave(self.s)
        times = (times0.unsqueeze(-1) + (-self.dt * torch.arange(0, self.s))).view(-1)
        return self.motion_frames(ids, times).view(motion_ids.shape[0], -1)
