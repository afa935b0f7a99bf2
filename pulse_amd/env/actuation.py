"""The actuation stage of the env step: the PD-target table and the one launch that turns the policy's action into PD targets.

Mirrors
  Humanoid._build_pd_action_offset_scale   phc/env/tasks/humanoid.py:1037-1111   per-dof offset / scale from the joint limits (bias_offset both
                                                                                  ways, the min(1.2 max|lim|, pi) cap, knee scale 5, the
                                                                                  has_smpl_pd_offset shoulder offsets, upright and not)
  Humanoid.pre_physics_step                humanoid.py:1222-1247                  freeze_hand / freeze_toe zero those joints' targets
  _action_to_pd_targets                    humanoid.py:1392-1394, humanoid_im.py:1096-1101
  the agent's action clamp                 phc/learning/im_amp.py:68-73            clamp(actions, -1, 1) before the env step (VecTaskPythonWrapper's clip_actions, handed down)
The table is built once on the host; the stage itself is ops.pd_targets (csrc/pd_targets.hip).

The joint limits come from the injected simulator: ``sim.dof_limits_lower`` / ``sim.dof_limits_upper`` ((D,) float32; Isaac's
get_actor_dof_properties in the reference, humanoid.py:867-896).  A simulator that publishes none leaves the table at offset 0 / scale 1.
"""
import numpy as np
import torch

from .. import ops
from . import robot_keys


def pd_action_offset_scale(skeleton, lim_low, lim_high, *, bias_offset=False, has_smpl_pd_offset=False, upright=True):
    """_build_pd_action_offset_scale (humanoid.py:1037-1111) for a humanoid whose joints all have three dofs (smpl / smplh / smplx:
    _dof_offsets = 0, 3, 6, ..., humanoid.py:644): (offset, scale), two (D,) float32 numpy arrays.  The limits are float32 arrays there
    (float32 tensors' .cpu().numpy(), :1040-1041) and so is every array statement, the whole bias_offset branch included: restated here
    statement for statement in float32.  The one scalar path, 1.2 * max|lim| against pi (:1050-1054), meets a numpy float32 SCALAR, which
    numpy 1.x (the reference's: it still uses np.int) promotes to float64 and numpy 2 keeps in float32: it is done in Python floats (float64)
    and rounded by the store into the float32 array, numpy 1.x's result under any numpy."""
    names = skeleton["body_names"][1:]                                            # _dof_names (humanoid.py:393)
    lo = np.array(lim_low, dtype=np.float32)
    hi = np.array(lim_high, dtype=np.float32)
    if lo.shape != (3 * len(names),) or hi.shape != lo.shape:
        raise ValueError(f"dof limits: two ({3 * len(names)},) arrays expected, got {lo.shape} and {hi.shape}")
    # (a Python float beside a float32 ARRAY gives a float32 loop in both numpys: 0.5 and 0.7 below act as float32)
    for j in range(len(names)):
        s = slice(3 * j, 3 * j + 3)
        if not bias_offset:
            curr_scale = max([float(np.max(np.abs(lo[s]))), float(np.max(np.abs(hi[s])))])
            curr_scale = min([1.2 * curr_scale, np.pi])
            lo[s], hi[s] = -curr_scale, curr_scale
        else:
            # the action range reaches a bit beyond the joint limits so that the motors keep their strength near the limits
            curr_mid = 0.5 * (hi[s] + lo[s])
            curr_scale = 0.7 * (hi[s] - lo[s])
            lo[s], hi[s] = curr_mid - curr_scale, curr_mid + curr_scale
    offset = 0.5 * (hi + lo)
    scale = 0.5 * (hi - lo)
    scale[names.index("L_Knee") * 3 + 1] = 5                                      # :1094-1099 (stronger knees)
    scale[names.index("R_Knee") * 3 + 1] = 5
    if has_smpl_pd_offset:                                                        # :1101-1109
        ls, rs = names.index("L_Shoulder") * 3, names.index("R_Shoulder") * 3
        if upright:
            offset[ls], offset[rs] = -np.pi / 2, np.pi / 2
        else:
            offset[ls], offset[ls + 2] = -np.pi / 6, -np.pi / 2
            offset[rs], offset[rs + 2] = -np.pi / 3, np.pi / 2
    return offset, scale


def freeze_mask(skeleton, *, freeze_hand=False, freeze_toe=False):
    """(D,) uint8 numpy array: 1 on the dofs whose target pre_physics_step sets to 0 (humanoid.py:1239-1244)."""
    names = skeleton["body_names"][1:]
    mask = np.zeros(3 * len(names), dtype=np.uint8)
    for on, bodies in ((freeze_hand, ("L_Hand", "R_Hand")), (freeze_toe, ("L_Toe", "R_Toe"))):
        if on:
            for b in bodies:
                mask[names.index(b) * 3:names.index(b) * 3 + 3] = 1
    return mask


class Actuation:
    """What a task class keeps of the stage: the table, the freeze mask and the action clip, and the launch."""

    def __init__(self, skeleton, robot, sim, device, *, upright=True):
        sw = robot_keys.actuation_switches(robot)
        d = skeleton["num_dof"]
        lo, hi = getattr(sim, "dof_limits_lower", None), getattr(sim, "dof_limits_upper", None)
        if (lo is None) != (hi is None):
            raise ValueError("the simulator publishes one of dof_limits_lower / dof_limits_upper: both or neither")
        if lo is not None:
            offset, scale = pd_action_offset_scale(skeleton, torch.as_tensor(lo).detach().cpu().numpy(), torch.as_tensor(hi).detach().cpu().numpy(),
                                                   bias_offset=sw["bias_offset"], has_smpl_pd_offset=sw["has_smpl_pd_offset"], upright=upright)
        else:
            if sw["bias_offset"] or sw["has_smpl_pd_offset"]:
                raise ValueError("bias_offset / has_smpl_pd_offset shape the PD-target table built from the joint limits (humanoid.py:1037-1111): the "
                                 "injected simulator publishes no dof_limits_lower / dof_limits_upper")
            offset, scale = np.zeros(d, dtype=np.float32), np.ones(d, dtype=np.float32)
        self.offset = torch.from_numpy(offset).to(device)
        self.scale = torch.from_numpy(scale).to(device)
        mask = freeze_mask(skeleton, freeze_hand=sw["freeze_hand"], freeze_toe=sw["freeze_toe"])
        self.freeze = torch.from_numpy(mask).to(device) if mask.any() else None
        self.clip = float("inf")                                                  # VecTaskPythonWrapper hands its clip_actions down

    def __call__(self, actions, ref_dof_pos=None, sim_dof_pos=None):
        """(clamped actions, PD targets), fresh tensors, one launch."""
        return ops.pd_targets(actions, self.scale, clip=self.clip, offset=self.offset, freeze=self.freeze, ref_dof_pos=ref_dof_pos,
                              sim_dof_pos=sim_dof_pos)
