"""Every ``cfg.robot`` key the reference's task classes read, and what this implementation does with it.

The reference reads its robot options with ``cfg.robot.get(key, default)`` in two places of the task class chain
(phc/env/tasks/humanoid.py:247, 266-279, 355-365) plus ``cfg.robot.asset`` (humanoid.py:626, 685, 734-735, 929; humanoid_amp.py:294).  A key that
is silently ignored here would change what a configuration computes without anybody noticing: the hole env_keys.py closes for ``cfg["env"]``.
``audit`` sorts EVERY key of a robot dict into one of three classes:

  HONOURED   this package reads the key and does what the reference does with it;
  INERT      the key configures the simulator's asset (mesh, geometry, weights, joint-limit mode, collision filter: all consumed by SMPL_Robot /
             Isaac Gym asset creation, out of scope by contract); accepted and ignored, with the reason recorded below;
  UNBUILT    the reference acts on the key, this package does not: accepted ONLY at the value for which the reference's behaviour is the one built
             here, anything else raises NotImplementedError naming the key and the reference lines.

A key in none of the three (motion_sym_loss, sym_loss_coef in the shipped files) is one the reference does not read either; it is reported once
through ``warnings``.

DEFAULTS OF THE ACTUATION SWITCHES.  The reference's ``.get`` defaults are freeze_toe = True and freeze_hand = True (humanoid.py:279, 362-363).
They cannot be reached through its entry point: hydra always composes a robot file (phc/data/cfg/config.yaml:4, ``robot: smpl_humanoid``) and all
three shipped robot files (robot/smpl_humanoid.yaml, smpl_humanoid_shape.yaml, smplx_humanoid.yaml) set freeze_toe, freeze_hand, bias_offset and
has_smpl_pd_offset to false.  An ABSENT key therefore reads here as the shipped robot files have it (``ACTUATION_DEFAULTS``), not as the ``.get``
default: every configuration that ran before these switches were built keeps its targets.
"""
import warnings

# bias_offset, has_smpl_pd_offset: _build_pd_action_offset_scale (humanoid.py:1037-1111); freeze_hand, freeze_toe: pre_physics_step (:1239-1244)
ACTUATION_DEFAULTS = {"bias_offset": False, "has_smpl_pd_offset": False, "freeze_toe": False, "freeze_hand": False}

HONOURED = {
    "humanoid_type",                                                                                       # humanoid.py:247 (check_humanoid_options)
    "has_upright_start", "has_dof_subset", "has_shape_obs", "has_weight_obs", "has_shape_obs_disc", "has_weight_obs_disc",
    "bias_offset", "has_smpl_pd_offset", "freeze_toe", "freeze_hand",                                       # env/actuation.py
}

_ASSET = ("consumed by SMPL_Robot / Isaac Gym asset creation (humanoid.py:743-763, 867-1031; closed-source physics: out of scope, SURVEY.md "
          "section 2 #20, #36): the simulator is injected with its actors built")

INERT = {
    "asset": "asset root / file name (humanoid.py:626, 685, 734-735, 929; humanoid_amp.py:294): " + _ASSET,
    "has_mesh": _ASSET, "replace_feet": _ASSET, "has_jt_limit": _ASSET, "remove_toe": _ASSET, "big_ankle": _ASSET, "box_body": _ASSET,
    "real_weight": _ASSET, "real_weight_porpotion_capsules": _ASSET, "real_weight_porpotion_boxes": _ASSET, "master_range": _ASSET,
    "has_self_collision": "collision filter of the actors (humanoid.py:919, 1019-1031): " + _ASSET,
    # has_shape_variation (humanoid.py:697-700, 783-826, 987-990): per-env betas go into the generated asset files and scale the asset's PD gains;
    # what the task classes see of it afterwards is humanoid_shapes / humanoid_limb_and_weights, which this package takes from the injected
    # simulator (sim.humanoid_shapes) or draws (shape_seed)
    "has_shape_variation": "per-env body shapes are drawn while the assets are generated and the gains are scaled in the asset's dof properties "
                           "(humanoid.py:697-700, 783-826, 987-990): " + _ASSET,
}

# key -> (values at which the reference's behaviour is what is built here, where the reference implements the rest)
UNBUILT = {
    # self.action_idx IS assigned (humanoid.py:368-371, two hard-coded index lists), so the reference can run reduce_action: the policy then has
    # len(action_idx) = 47 (65 with masterfoot) outputs that are scattered into a zero (N, 69) action before _action_to_pd_targets, and the freeze
    # switches are skipped
    "reduce_action": ((False,), "humanoid.py:365-371, 647-648, 1232-1235 (47 policy outputs scattered into the 69 dofs through action_idx)"),
    # masterfoot asks SMPL_Robot for a humanoid with articulated feet (humanoid.py:753; the action_idx list of :369 reaches dof 83 of such a
    # humanoid): more bodies and dofs than the 24 / 52-body tables of synthetic.SKELETONS describe
    "masterfoot": ((False,), "humanoid.py:278, 368-369, 753 (the articulated-foot SMPL humanoid: more bodies and dofs than the 24-body tables)"),
}

ALL_KNOWN = HONOURED | set(INERT) | set(UNBUILT)
_warned = set()


def actuation_switches(robot):
    """The four actuation switches of a robot dict (None / not a dict: none given), absent ones at the shipped robot files' value."""
    robot = robot if isinstance(robot, dict) else {}
    return {k: bool(robot.get(k, d)) for k, d in ACTUATION_DEFAULTS.items()}


# HONOURED keys the downstream task classes (env/humanoid_tasks.py) do not read: their observation carries no shape / limb-weight rows
# (humanoid.py:266-268, 657-661 add 11 / 10 columns to the self observation), so those tasks accept them only switched off
TASK_UNREAD = ("has_shape_obs", "has_weight_obs")


def audit(robot, where="HumanoidIm", body_names=None, unread=()):
    """Raise NotImplementedError if ``robot`` (cfg.robot; None / not a dict: nothing to audit) switches on behaviour of the reference that is not
    built; warn (once per key) about keys the reference does not read.  ``body_names``: the humanoid's bodies, for the switches that look a body up
    by name.  ``unread``: HONOURED keys the calling class does not read (TASK_UNREAD): switched on they raise by name too."""
    if not isinstance(robot, dict):
        return
    on = [k for k in unread if robot.get(k, False)]
    if on:
        raise NotImplementedError(f"{where}: robot option(s) {on} are switched on but this task class does not build them: the shape / limb-weight "
                                  "rows of the self observation (phc/env/tasks/humanoid.py:266-268, 657-661) are built by HumanoidIm only")
    bad = [k for k in robot if k in UNBUILT and not any(robot[k] == v for v in UNBUILT[k][0])]
    if bad:
        lines = [f"  {k} = {robot[k]!r}: not built (accepted: {UNBUILT[k][0]}); reference: phc/env/tasks/{UNBUILT[k][1]}" for k in bad]
        raise NotImplementedError(f"{where}: robot option(s) the reference acts on but this implementation does not:\n" + "\n".join(lines))
    if body_names is not None:
        for key, bodies in (("freeze_hand", ("L_Hand", "R_Hand")), ("freeze_toe", ("L_Toe", "R_Toe"))):
            missing = [b for b in bodies if b not in body_names]
            if robot.get(key, ACTUATION_DEFAULTS[key]) and missing:
                raise NotImplementedError(f"{where}: robot option {key} = {robot[key]!r} with humanoid_type {robot.get('humanoid_type', 'smpl')!r}: the "
                                          f"reference looks {missing} up in its dof names (phc/env/tasks/humanoid.py:1239-1244), which this humanoid "
                                          "does not have (a ValueError there)")
    unknown = sorted(k for k in robot if k not in ALL_KNOWN and k not in _warned)
    if unknown:
        _warned.update(unknown)
        warnings.warn(f"{where}: robot key(s) {unknown} are not read by the reference's task classes either; ignored", stacklevel=3)
