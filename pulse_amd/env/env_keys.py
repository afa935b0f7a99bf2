"""Every ``cfg["env"]`` key the reference's task classes read, and what this implementation does with it.

The reference reads its env options with ``cfg["env"].get(key, default)`` scattered over the task class chain
(phc/env/tasks/humanoid.py:245-350, humanoid_amp.py:76-135, humanoid_im.py:30-100, 496-527, humanoid_z.py:20-80, humanoid_im_getup.py,
humanoid_im_distill.py, humanoid_speed.py / _reach.py / _strike.py / _traj.py / _pedestrian_terrain.py, base_task.py:60-131).  A key that is
silently ignored here would change what a shipped configuration computes without anybody noticing (round 5 shipped exactly that hole:
``zero_out_far``).  ``audit`` therefore sorts EVERY key of an env dict into one of three classes:

  HONOURED   this package reads the key and does what the reference does with it;
  INERT      the key configures a subsystem that is out of scope by contract (Isaac Gym scene / asset creation, the viewer, reading motion files from disk)
             or is read by the reference into an attribute nothing consumes; accepted and ignored, with the reason recorded below;
  UNBUILT    the reference acts on the key, this package does not: accepted ONLY at the value(s) for which the reference's behaviour is the
             one built here, anything else raises NotImplementedError naming the key and the reference lines that implement it.

A key in none of the three is one the reference does not read on this path either (legacy spellings, notes): ignoring it IS the
reference's behaviour; it is reported once through ``warnings`` so typos are visible.  tests/test_env_keys.py re-derives the set of keys the
reference reads from its sources (when /root/reference is mounted) and fails if one is missing here, and walks every shipped
``phc/data/cfg/env/*.yaml``.
"""
import warnings

# ---------------------------------------------------------------------------------------------------------------------------------------
HONOURED = {
    # observation / reward / reset switches of the imitation task
    "obs_v", "self_obs_v", "past_track_steps", "force_sensor_joints", "fut_tracks", "numTrajSamples", "trajSampleTimestepInv",
    "local_root_obs", "root_height_obs", "full_body_reward", "power_reward", "power_coefficient", "reward_specs",
    "enableEarlyTermination", "episode_length", "cycle_motion", "trackBodies", "reset_bodies", "terminationDistance", "stateInit",
    "controlFrequencyInv", "strict_eval", "cycle_motion_xp", "fut_tracks_dropout", "add_obs_noise", "res_action",
    "occl_training", "occl_training_prob",
    # what resample_motions hands to MotionLib.load_motions on a library built from raw motion data (humanoid_im.py:366-367)
    "max_len", "seq_motions",
    # zero_out_far (humanoid.py:311-329)
    "zero_out_far", "zero_out_far_train", "zero_out_far_steps", "close_distance", "far_distance",
    # robot switches the env dict may carry (robot/*.yaml merged by the caller)
    "has_upright_start", "has_dof_subset", "has_shape_obs", "has_weight_obs", "has_shape_obs_disc", "has_weight_obs_disc",
    # AMP observations
    "enable_amp_obs", "numAMPObsSteps", "ampRootHeightObs", "key_bodies", "add_amp_input_noise",
    # PULSE / distillation attributes the agent reads off the task (amp_agent.py:59-63, 773-832)
    "temp_running_mean", "kin_lr", "save_kin_info", "only_kin_loss", "distill", "z_type", "kld_coefficient", "kld_coefficient_min",
    "ar1_coefficient", "kld_anneal", "use_ar1_prior", "use_vae_prior", "use_vae_prior_regu", "embedding_size", "embedding_norm",
    "use_vae_clamped_prior", "vae_var_clamp_max", "proj_norm",
    # prior / posterior variants of the PULSE VAE (amp_network_z_builder.py:40-46, 118-119, 226-241, 514-533; amp_agent.py:785-789;
    # humanoid_z.py:44-48, 101-107).  use_vae_sphere_prior acts inside the fixed-prior branch only (:237-239): beside a learned prior, or
    # with no prior at all, the reference ignores it and so does this package (accepted without effect).  When both use_vae_prior and
    # use_vae_fixed_prior are on, the learned branch wins (if / elif in both places).
    "use_vae_fixed_prior", "use_vae_sphere_prior", "use_vae_sphere_posterior", "vae_prior_fixed_logvar",
    "auto_pmcp", "auto_pmcp_soft", "shape_resampling_interval", "fitting", "models",
    # MCP composer stage (humanoid_im_mcp.py:16-28): the action is a weight vector over num_prim frozen PNN primitives (env/humanoid_im_mcp.py)
    "num_prim", "discrete_moe", "has_pnn", "has_lateral", "z_activation",
    # get-up task (humanoid_im_getup.py:42-66)
    "recoveryEpisodeProb", "recoverySteps", "fallInitProb", "getup_schedule", "getup_udpate_epoch",
    # downstream tasks (humanoid_speed.py / _reach.py / _strike.py / _traj.py / _pedestrian_terrain.py)
    "enableTaskObs", "tarSpeedMin", "tarSpeedMax", "speedChangeStepsMin", "speedChangeStepsMax", "tarChangeStepsMin", "tarChangeStepsMax",
    "tarDistMax", "tarHeightMin", "tarHeightMax", "reachBodyName", "strikeBodyNames", "terminationHeight", "contact_bodies",
    "trajSampleTimestep", "speedMin", "speedMax", "accelMax", "sharpTurnProb", "sensor_extent", "sensor_res", "fuzzy_target",
    "terrain", "terrain_obs", "terrain_obs_type", "terrain_obs_root", "use_center_height",
    "power_usage_reward", "power_usage_coefficient",      # read by the speed / strike tasks only (humanoid_speed.py:43-53, humanoid_strike.py:37-40)
    # crowd variant of the terrain task (humanoid.py:256-261; humanoid_pedestrian_terrain.py:35, 253-293, 385-439, 718-772, 1200-1276,
    # 1700-1753): contiguous env groups, the 5-neighbour 'people' observation, people stamped into the height map, and the [h, vx, vy]
    # height block (env/humanoid_tasks.py: HumanoidPedestrianTerrain; csrc/crowd_obs.hip).  Only that task class acts on them, here as in
    # the reference.  What stays out of scope raises where it would be used: the point-net branch of amp_sept (learning/network_sept.py),
    # _compute_flip_task_obs, Isaac collision groups (humanoid.py:919), the 'fov' sensor types (terrain_obs_type).
    "divide_group", "group_obs", "disable_group_obs", "num_env_group", "velocity_map",
    # keys of THIS package (no reference counterpart): seeds of the synthetic stand-ins, stand-in selection
    "motion_clock_seed", "obs_noise_seed", "occl_seed", "shape_seed", "task_seed", "getup_seed", "amp_seed", "physics", "contactBodies", "tarDistMin", "nearDist", "nearProb",
}

_SIM = "Isaac Gym scene / actor / asset creation (closed-source physics: out of scope, SURVEY.md section 2 #20, #36)"
_LOAD = ("consumed where the reference opens its motion file and builds the library (humanoid_im.py:320-345: joblib pickles, smpl_sim): the caller hands "
         "over a built MotionLib -- MotionLib.from_motion_data takes the loaded data dict and min_length as arguments")
_VIEW = "viewer / debug drawing (out of scope)"
_DEAD = "the reference stores it in an attribute that nothing on the training path reads"
_TEACH = ("steers which PNN column trains / loads (amp_network_pnn_builder.py:36-38): read by the amp_pnn network (learning/network_pnn.py) from "
          "cfg['env'], not by the env")

INERT = {
    "task": "selects the task class (utils/parse_task.py:57-70): the caller instantiates the class",
    "project_name": "run metadata", "notes": "run metadata",
    "num_envs": "taken from the injected simulator (checked against it when given)",
    "env_spacing": _SIM, "plane": _SIM, "kp_scale": _SIM, "kd_scale": _SIM, "power_scale": _SIM, "pd_control": _SIM,
    "default_humanoid_mass": _SIM, "numActions": _SIM, "numObservations": _SIM, "numStates": _SIM, "asset": _SIM,
    "enable_debug_vis": _VIEW, "show_sensors": _VIEW, "is_flag_run": _DEAD,
    "motion_file": _LOAD, "min_length": _LOAD, "hard_negative": _LOAD,
    "eval_full": _DEAD, "kin_policy": _DEAD, "partial_running_mean": _DEAD, "vae_reader": _DEAD, "z_model": _DEAD, "z_read": _DEAD,
    "z_uniform": _DEAD, "use_vae_prior_loss": _DEAD, "tarSpeed": _DEAD,
    "training_prim": _TEACH, "actors_to_load": _TEACH,
    "distill_model_config": "structure of the frozen PULSE networks: HumanoidZ.initialize_z_models takes the checkpoint and network params as arguments",
    "hybridInitProb": "only read when stateInit is Hybrid (humanoid_amp.py:490-505), which raises here",
    "dict_size": "VQ dictionary size: only read for z_type vq_vae variants, which raise here",
    "embedding_partion": "VQ partition count: only read for z_type vq_vae variants, which raise here",
    "small_terrain": "debug switch of the terrain mesh creation (" + _SIM + ")",
}

# key -> (values at which the reference's behaviour is what is built here, where the reference implements the rest)
UNBUILT = {
    "addInputNoise": ((False,), "vec_task / task input noise"),
    "remove_disc_rot": ((False,), "humanoid.py:413-416 (discriminator dof subset without global rotation)"),
    # amp_obs_v 2 (build_amp_observations_smpl_v2) is built in the AMP frame (amp_obs.hip, HumanoidIm with enable_amp_obs); the reference's task
    # chain builds that frame unconditionally, so an env dict that asks for it where no AMP frame is built would drop it silently: it raises
    "amp_obs_v": ((1, "2 with enable_amp_obs"), "humanoid_amp.py:300-314, 670-680 (the v2 AMP frame: built by HumanoidIm's AMP observation, enable_amp_obs)"),
    "numAMPEncObsSteps": ("==numAMPObsSteps", "humanoid_amp.py:94, 834-880 (CALM encoder windows)"),
    "enableHistObs": ((False,), "humanoid_amp.py:320, 509-517"),
    "is_discrete": ((False,), "base_task.py:90; amp_agent.py:42-44 (discrete action heads)"),
    "control_mode": (("isaac_pd",), "humanoid.py:1250-1290 (torques computed in Python for control_mode pd)"),
    "z_readout": ((False,), "amp_network_z_builder.py:63, amp_network_z_reader_builder.py:36"),
    "z_all": ((False,), "amp_network_z_builder.py:37 (z fed to every decoder layer)"),
    "vae_prior_policy": ((False,), "amp_network_z_reader_builder.py:38-57"),
    "distill_z_model": ((False,), "humanoid_im_distill.py:43-63, 186-231 (a PULSE model as the distillation teacher)"),
}

ALL_KNOWN = HONOURED | set(INERT) | set(UNBUILT)
_warned = set()


def _inactive(key, value, env):
    ok, _ = UNBUILT[key]
    if ok == "==numAMPObsSteps":
        return int(value) == int(env.get("numAMPObsSteps", 10))
    if key == "amp_obs_v":
        return value == 1 or (value == 2 and bool(env.get("enable_amp_obs", False)))
    return any(value == v for v in ok)


def check_vae_options(env, where="HumanoidIm"):
    """Combinations of the VAE switches the reference itself cannot run.  use_vae_prior_regu without a prior: _optimize_kin reads
    ``prior_mu`` / ``prior_log_var`` that were never assigned (amp_agent.py:810-813 after the else branch of :785-789)."""
    if env.get("use_vae_prior_regu", False) and not env.get("use_vae_prior", False) and not env.get("use_vae_fixed_prior", False):
        raise NotImplementedError(f"{where}: use_vae_prior_regu without use_vae_prior / use_vae_fixed_prior: the regulariser reads the prior's mean "
                                  "and log-variance, which do not exist without a prior; reference: phc/learning/amp_agent.py:810-813 "
                                  "(prior_mu is unassigned there)")


def audit(env, where="HumanoidIm"):
    """Raise NotImplementedError if ``env`` switches on behaviour of the reference that is not built; warn (once per key) about keys
    the reference does not read on this path."""
    check_vae_options(env, where)
    bad = [k for k in env if k in UNBUILT and not _inactive(k, env[k], env)]
    if bad:
        lines = [f"  {k} = {env[k]!r}: not built (accepted: {UNBUILT[k][0]}); reference: phc/.../{UNBUILT[k][1]}" for k in bad]
        raise NotImplementedError(f"{where}: env option(s) the reference acts on but this implementation does not:\n" + "\n".join(lines))
    unknown = sorted(k for k in env if k not in ALL_KNOWN and k not in _warned)
    if unknown:
        _warned.update(unknown)
        warnings.warn(f"{where}: env key(s) {unknown} are not read by the reference's task classes on this path either; ignored", stacklevel=3)
