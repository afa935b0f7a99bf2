"""The BASELINE.json configurations as concrete configs (values from the reference's YAML files).

learning/im.yaml:46-91 hyper-parameters; env/env_im.yaml env switches.  ``make_agent`` wires a
recorded synthetic rollout (pulse_amd/env/sim.py) to HumanoidIm and a CommonAgent.
"""
import copy

NETWORK_IM = {            # phc/data/cfg/learning/im.yaml:12-44
    "name": "amp", "separate": True,
    "space": {"continuous": {"mu_activation": "None", "sigma_activation": "None", "mu_init": {"name": "default"},
                             "sigma_init": {"name": "const_initializer", "val": -2.9}, "fixed_sigma": True, "learn_sigma": False}},
    "mlp": {"units": [1024, 512], "activation": "relu", "d2rl": False, "initializer": {"name": "default"}},
    "disc": {"units": [1024, 512], "activation": "relu", "initializer": {"name": "default"}},
}

PPO_IM = {                # phc/data/cfg/learning/im.yaml:46-91
    "name": "Humanoid", "multi_gpu": False, "ppo": True, "mixed_precision": False, "normalize_input": True,
    "normalize_value": True, "reward_shaper": {"scale_value": 1}, "normalize_advantage": True, "gamma": 0.99, "tau": 0.95,
    "learning_rate": 2e-5, "lr_schedule": "constant", "entropy_coef": 0.0, "truncate_grads": True, "grad_norm": 50.0,
    "e_clip": 0.2, "horizon_length": 32, "minibatch_size": 16384, "mini_epochs": 6, "critic_coef": 5, "clip_value": False,
    "bounds_loss_coef": 10,
    # AMP (learning/im.yaml:78-91)
    "amp_obs_demo_buffer_size": 200000, "amp_replay_buffer_size": 200000, "amp_replay_keep_prob": 0.01, "amp_batch_size": 512,
    "amp_minibatch_size": 4096, "disc_coef": 5, "disc_logit_reg": 0.01, "disc_grad_penalty": 5, "disc_reward_scale": 2,
    "disc_weight_decay": 0.0001, "normalize_amp_input": True, "task_reward_w": 0.5, "disc_reward_w": 0.5,
}

ENV_IM = {"obs_v": 6, "self_obs_v": 1, "power_reward": True, "local_root_obs": True, "root_height_obs": True,
          "enableEarlyTermination": True, "terminationDistance": 0.25, "episode_length": 300}

NETWORK_Z = {             # phc/data/cfg/learning/im_z_fit.yaml:12-50 (network: amp_z)
    "name": "amp_z", "separate": True,
    "space": {"continuous": {"mu_activation": "None", "sigma_activation": "None", "mu_init": {"name": "default"},
                             "sigma_init": {"name": "const_initializer", "val": -2.9}, "fixed_sigma": True, "learn_sigma": False}},
    "mlp": {"units": [3096, 2048, 1024], "activation": "silu", "d2rl": False, "initializer": {"name": "default"}},
    "task_mlp": {"units": [1536, 1024, 512], "activation": "silu", "d2rl": False, "initializer": {"name": "default"}},
}

ENV_IM_VAE = dict(ENV_IM, **{   # phc/data/cfg/env/env_im_vae.yaml:19-55 (PULSE distillation)
    "embedding_norm": 1, "embedding_size": 32, "z_type": "vae", "use_vae_prior": True, "use_ar1_prior": True,
    "use_vae_clamped_prior": True, "vae_var_clamp_max": 2, "kld_coefficient": 0.01, "kld_coefficient_min": 0.001, "kld_anneal": True,
    "ar1_coefficient": 0.005, "only_kin_loss": True, "distill": True, "save_kin_info": True, "cycle_motion": True})

# Prior / posterior variants of the PULSE VAE (amp_network_z_builder.py:40-46, 118-119, 226-241, 514-533): env-dict overrides on top of
# ENV_IM_VAE, e.g. make_agent("cfg3_small", env_overrides=vae_variant_env("fixed_sphere_post")).  No shipped config switches them on;
# embedding_norm 2 and a non-zero fixed log-variance keep the variants apart from their defaults.
VAE_VARIANTS = {
    "learned": {},
    "none": {"use_vae_prior": False},
    "fixed": {"use_vae_prior": False, "use_vae_fixed_prior": True, "vae_prior_fixed_logvar": -0.5},
    "fixed_sphere": {"use_vae_prior": False, "use_vae_fixed_prior": True, "vae_prior_fixed_logvar": -0.5, "use_vae_sphere_prior": True, "embedding_norm": 2},
    "sphere_post": {"use_vae_sphere_posterior": True, "embedding_norm": 2},
    "none_sphere_post": {"use_vae_prior": False, "use_vae_sphere_posterior": True, "embedding_norm": 2},
    "fixed_sphere_post": {"use_vae_prior": False, "use_vae_fixed_prior": True, "vae_prior_fixed_logvar": -0.5, "use_vae_sphere_prior": True,
                          "use_vae_sphere_posterior": True, "embedding_norm": 2},
}


def vae_variant_env(name, **extra):
    """The env-dict overrides of a VAE_VARIANTS entry (a copy), for make_agent / make_env's ``env_overrides``."""
    return dict(VAE_VARIANTS[name], **extra)


# Crowd variant of the terrain task (humanoid.py:256-261, humanoid_pedestrian_terrain.py:253-293, 385-439, 718-772, 1200-1276): env-dict
# overrides on top of ENV_TERRAIN_Z, e.g. make_agent("terrain_z_crowd_small", env_overrides=crowd_env("stamps_velocity", num_env_group=16)).
# No shipped config switches them on.  'group_obs' and the two velocity kinds change the detail keys of the task observation, which rules
# amp_sept out (learning/network_sept.py); 'stamps' leaves the widths alone.
CROWD_ENVS = {
    "group_obs": {"divide_group": True, "group_obs": True},                      # + the 165-float 'people' block
    "stamps": {"divide_group": True},                                            # people stamped into the group's height map
    "stamps_velocity": {"divide_group": True, "velocity_map": True},             # ... and the velocity of whoever covers a sample
    "velocity": {"velocity_map": True},                                          # no groups: minus the own velocity on both channels
}


def crowd_env(kind, **extra):
    """The env-dict overrides of a CROWD_ENVS entry (a copy), for make_agent / make_env's ``env_overrides``."""
    return dict(CROWD_ENVS[kind], **extra)


# Maps for the terrain task (env/terrain.py:Terrain; the ``terrain`` block of env_pulse_terrain.yaml:75-90), small enough for tests: the
# curriculum layout over the tile kinds that need no isaacgym.terrain_utils generator -- 'poles' (synthetic.synthetic_poles stands in for
# poles_terrain) and flat.  make_agent("terrain_z_amp_small", terrain="poles_small") resets its humanoids onto the valid start cells.
TERRAINS = {
    # 2 levels x 4 terrains of 8 m (small_terrain, humanoid_pedestrian_terrain.py:817-819): terrains 0, 1 poles, 2, 3 flat
    "poles_small": {"terrainType": "trimesh", "curriculum": True, "mapLength": 8., "mapWidth": 8., "numLevels": 2, "numTerrains": 4,
                    "terrainProportions": [0., 0., 0., 0., 0., 0., 0.5, 0.5], "slopeTreshold": 0.9},
}


def terrain_env(kind, **extra):
    """The env-dict overrides of a TERRAINS entry (its ``terrain`` block, a copy), for make_agent / make_env's ``env_overrides``."""
    return {"terrain": dict(TERRAINS[kind], **extra)}


def make_terrain(kind, num_robots, device, seed=1234, **extra):
    """The Terrain of a TERRAINS entry on ``device``; its poles are drawn from a generator seeded with ``seed``."""
    from . import synthetic as syn
    from .env.terrain import Terrain
    g = syn.make_generator(seed + 83)
    return Terrain.from_config(dict(TERRAINS[kind], **extra), num_robots, {"poles": lambda terrain, difficulty: syn.synthetic_poles(terrain, difficulty, g)},
                               device)


NETWORK_Z_READER = {      # phc/data/cfg/learning/pulse_z_task.yaml:10-44 (network: amp_z_reader)
    "name": "amp_z_reader", "separate": True,
    "space": {"continuous": {"mu_activation": "None", "sigma_activation": "None", "mu_init": {"name": "default"},
                             "sigma_init": {"name": "const_initializer", "val": -1.0}, "fixed_sigma": True, "learn_sigma": False}},
    "mlp": {"units": [2048, 1024, 512], "activation": "silu", "d2rl": False, "initializer": {"name": "default"}},
    "disc": {"units": [1024, 512], "activation": "relu", "initializer": {"name": "default"}},       # :35-40; built when the env hands out AMP windows
}

NETWORK_SEPT = {          # phc/data/cfg/learning/pulse_z_terrain.yaml:12-51 (network: amp_sept)
    "name": "amp_sept", "separate": True,
    "space": {"continuous": {"mu_activation": "None", "sigma_activation": "None", "mu_init": {"name": "default"},
                             "sigma_init": {"name": "const_initializer", "val": -1.0}, "fixed_sigma": True, "learn_sigma": False}},
    "mlp": {"units": [2048, 1024, 512], "activation": "silu", "d2rl": False, "initializer": {"name": "default"}},
    "task_mlp": {"units": [512, 256], "activation": "silu", "d2rl": False, "initializer": {"name": "default"}},
    "disc": {"units": [1024, 512], "activation": "relu", "initializer": {"name": "default"}},       # :46-51; built when the env hands out AMP windows
}

NETWORK_MCP = {           # phc/data/cfg/learning/im_mcp.yaml:11-45 (network: amp_mcp; ending_act is read by nothing in the reference)
    "name": "amp_mcp", "separate": True, "discrete": False, "has_softmax": False, "ending_act": True,
    "space": {"continuous": {"mu_activation": "None", "sigma_activation": "None", "mu_init": {"name": "default"},
                             "sigma_init": {"name": "const_initializer", "val": -2.9}, "fixed_sigma": True, "learn_sigma": False}},
    "mlp": {"units": [1024, 512], "activation": "relu", "d2rl": False, "initializer": {"name": "default"}},
    "disc": {"units": [1024, 512], "activation": "relu", "initializer": {"name": "default"}},
}

NETWORK_PNN = {           # phc/data/cfg/learning/im_pnn.yaml:11-43 (network: amp_pnn)
    "name": "amp_pnn", "separate": True, "discrete": False,
    "space": {"continuous": {"mu_activation": "None", "sigma_activation": "None", "mu_init": {"name": "default"},
                             "sigma_init": {"name": "const_initializer", "val": -2.9}, "fixed_sigma": True, "learn_sigma": False}},
    "mlp": {"units": [1024, 512], "activation": "relu", "d2rl": False, "initializer": {"name": "default"}},
    "disc": {"units": [1024, 512], "activation": "relu", "initializer": {"name": "default"}},
}

# phc/data/cfg/env/phc_kp_mcp_iccv.yaml:23-80 (task HumanoidImMCPGetup): the switches this package reads; ``models`` is the synthetic PNN
# checkpoint make_env builds (the shipped file names output/phc_kp_pnn_iccv/Humanoid.pth)
ENV_MCP = {"fut_tracks": False, "obs_v": 7, "has_pnn": True, "fitting": True, "num_prim": 4, "training_prim": 2, "actors_to_load": 4,
           "has_lateral": False, "zero_out_far": True, "zero_out_far_train": False, "cycle_motion": False, "getup_udpate_epoch": 95000,
           "getup_schedule": True, "recoverySteps": 90, "zero_out_far_steps": 90, "recoveryEpisodeProb": 0.5, "fallInitProb": 0.3,
           "power_reward": True, "power_coefficient": 0.00005, "shape_resampling_interval": 500, "controlFrequencyInv": 2, "stateInit": "Random",
           "enableEarlyTermination": True, "terminationDistance": 0.25, "numTrajSamples": 3, "trajSampleTimestepInv": 3, "enableTaskObs": True,
           "episode_length": 300}

# the keypoint-driven demos (humanoid_im_mcp_demo.py, humanoid_im_demo.py): the MCP composer's switches without the get-up task's, and the plain
# imitation env at obs_v 7; both with the far masking their task observation applies (close_distance is the class's own: 0.5 / 0.25)
ENV_MCP_DEMO = {k: v for k, v in ENV_MCP.items() if k not in ("getup_schedule", "getup_udpate_epoch", "recoverySteps", "recoveryEpisodeProb", "fallInitProb")}
ENV_IM_DEMO = dict(ENV_IM, obs_v=7, zero_out_far=True, zero_out_far_train=False)

ENV_TERRAIN_Z = {"local_root_obs": True, "root_height_obs": True, "enableEarlyTermination": True, "episode_length": 300, "enableTaskObs": True,
                 "numTrajSamples": 10, "trajSampleTimestep": 0.5, "speedMin": 0.0, "speedMax": 3.0, "accelMax": 2.0, "sharpTurnProb": 0.02,
                 "terrain_obs": True, "terrain_obs_type": "square", "terrain_obs_root": "head", "use_center_height": True, "power_reward": False,
                 "terrain": {"terrainType": "trimesh"}, "embedding_size": 32, "z_type": "vae"}   # phc/data/cfg/env/env_pulse_terrain.yaml

ENV_SPEED_Z = {"local_root_obs": True, "root_height_obs": True, "enableEarlyTermination": True, "episode_length": 300, "enableTaskObs": True,
               "tarSpeedMin": 0.0, "tarSpeedMax": 5.0, "speedChangeStepsMin": 100, "speedChangeStepsMax": 200, "power_reward": True,
               "embedding_size": 32, "z_type": "vae"}     # phc/data/cfg/env/env_pulse_amp.yaml (HumanoidSpeedZ)

# the AMP layer of the downstream tasks: env switches (env_pulse_amp.yaml:66) and the learning keys of pulse_z_task.yaml:90-91
ENV_AMP_TASK = {"enable_amp_obs": True, "numAMPObsSteps": 10}
AMP_TASK_SMALL = {"task_reward_w": 1, "disc_reward_w": 0, "amp_minibatch_size": 64, "amp_obs_demo_buffer_size": 4096, "amp_replay_buffer_size": 4096,
                  "amp_batch_size": 128}

CONFIGS = {
    # BASELINE.json configs[0]: 64-env synthetic rollout (horizon 16), 2x512 MLP, one PPO+GAE epoch
    "cfg1": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "units": [512, 512]},
    # BASELINE.json configs[1]: 4096 SMPL humanoids, horizon 32, imitation reward/obs + PPO
    "cfg2": {"num_envs": 4096, "horizon_length": 32, "minibatch_size": 16384, "units": [1024, 512]},
    # BASELINE.json configs[2]: 8192 envs, PULSE VAE encoder/decoder in the policy head (latent 32); kin/VAE loss (PULSE training)
    "cfg3": {"num_envs": 8192, "horizon_length": 32, "minibatch_size": 16384, "network": "amp_z", "env": "vae", "agent": "amp",
             "extra": {"use_seq_rl": True}},
    # same network trained with the PPO loss (SURVEY.md 8d cfg 3, first variant)
    "cfg3_ppo": {"num_envs": 8192, "horizon_length": 32, "minibatch_size": 16384, "network": "amp_z", "env": "vae_ppo", "agent": "amp"},
    # BASELINE.json configs[4]: AMP discriminator + PPO, 8192 envs, bf16: training GEMMs on the bf16 MFMA over fp32 master weights
    "cfg5": {"num_envs": 8192, "horizon_length": 32, "minibatch_size": 16384, "units": [1024, 512], "env": "amp", "agent": "amp",
             "extra": {"enable_disc": True, "mixed_precision": True}},
    "cfg5_f32": {"num_envs": 8192, "horizon_length": 32, "minibatch_size": 16384, "units": [1024, 512], "env": "amp", "agent": "amp",
                 "extra": {"enable_disc": True}},
    "cfg5_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "units": [512, 512], "env": "amp", "agent": "amp",
                   "extra": {"enable_disc": True, "amp_minibatch_size": 64, "amp_obs_demo_buffer_size": 4096, "amp_replay_buffer_size": 4096,
                             "amp_batch_size": 128}},
    # downstream task on a frozen PULSE decoder: HumanoidSpeedZ, policy = amp_z_reader (learning=pulse_z_task), latent action 32
    "speed_z": {"num_envs": 4096, "horizon_length": 32, "minibatch_size": 16384, "network": "amp_z_reader", "env": "speed_z", "agent": "amp"},
    "speed_z_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_z_reader", "env": "speed_z", "agent": "amp",
                      "units": [256, 128]},
    # terrain traversal on a frozen PULSE decoder: HumanoidPedestrianTerrainZ, policy = amp_sept (learning=pulse_z_terrain; env_pulse_terrain.yaml: 1536 envs)
    "terrain_z": {"num_envs": 1536, "horizon_length": 32, "minibatch_size": 16384, "network": "amp_sept", "env": "terrain_z", "agent": "amp"},
    "terrain_z_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_sept", "env": "terrain_z", "agent": "amp",
                        "units": [256, 128]},
    # the same two tasks with the HumanoidAMP layer (enable_amp_obs): state init from the motion library, the 10-step AMP window and the
    # discriminator training beside the policy at task_reward_w 1 / disc_reward_w 0 (pulse_z_task.yaml:90-91, pulse_z_terrain.yaml:100-101:
    # its gradients enter the same optimiser step and the same grad_norm clip); the small ring sizes of cfg5_small
    "speed_z_amp_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_z_reader", "env": "speed_z", "agent": "amp",
                          "units": [256, 128], "extra": dict(AMP_TASK_SMALL), "env_overrides": dict(ENV_AMP_TASK)},
    "terrain_z_amp_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_sept", "env": "terrain_z", "agent": "amp",
                            "units": [256, 128], "extra": dict(AMP_TASK_SMALL), "env_overrides": dict(ENV_AMP_TASK)},
    # the crowd variant of the terrain task: 4 groups of 16, the 'people' neighbour block; amp_z_reader, a flat network (the detail keys of
    # the crowd observations rule amp_sept out); other kinds: env_overrides=crowd_env(kind, num_env_group=16)
    "terrain_z_crowd_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_z_reader", "env": "terrain_z",
                              "agent": "amp", "units": [256, 128], "env_overrides": dict(CROWD_ENVS["group_obs"], num_env_group=16)},
    # PHC's second stage (learning=im_mcp, env=phc_kp_mcp_iccv): the composer over 4 frozen PNN primitives, HumanoidImMCPGetup, 1536 envs
    "mcp": {"num_envs": 1536, "horizon_length": 32, "minibatch_size": 16384, "network": "amp_mcp", "env": "mcp", "agent": "amp"},
    "mcp_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_mcp", "env": "mcp", "agent": "amp",
                  "units": [256, 128]},
    # a trained tracker driven by streamed keypoints (HumanoidImMCPDemo / HumanoidImDemo on the recorded physics stand-in: the data path only)
    "mcp_demo_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_mcp", "env": "mcp_demo", "agent": "amp",
                       "units": [256, 128]},
    "im_demo_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "units": [512, 512], "env": "im_demo"},
    # PHC's first stage (learning=im_pnn, env=phc_kp_pnn_iccv): column training_prim of num_prim progressive columns trains, the AMP
    # discriminator beside it.  ``pnn`` is cfg5's shape, env, discriminator and mixed_precision with the amp_pnn network: the same launches
    "pnn": {"num_envs": 8192, "horizon_length": 32, "minibatch_size": 16384, "units": [1024, 512], "network": "amp_pnn", "env": "amp", "agent": "amp",
            "extra": {"enable_disc": True, "mixed_precision": True},
            "env_overrides": {"num_prim": 4, "training_prim": 0, "actors_to_load": 0, "has_lateral": False}},
    "pnn_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "units": [512, 512], "network": "amp_pnn", "env": "amp", "agent": "amp",
                  "extra": {"enable_disc": True, "amp_minibatch_size": 64, "amp_obs_demo_buffer_size": 4096, "amp_replay_buffer_size": 4096,
                            "amp_batch_size": 128},
                  "env_overrides": {"num_prim": 4, "training_prim": 0, "actors_to_load": 0, "has_lateral": False}},
    # a later column with lateral links into it (graph path, fp32): the concatenated second layer reads 3 x 36 = 108 columns
    "pnn_lateral_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "units": [36, 32], "network": "amp_pnn", "env": "amp",
                          "agent": "amp",
                          "extra": {"enable_disc": True, "amp_minibatch_size": 64, "amp_obs_demo_buffer_size": 4096, "amp_replay_buffer_size": 4096,
                                    "amp_batch_size": 128},
                          "env_overrides": {"num_prim": 3, "training_prim": 2, "actors_to_load": 2, "has_lateral": True}},
    # small shapes of the same graphs for tests
    "cfg3_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_z", "env": "vae", "agent": "amp",
                   "extra": {"use_seq_rl": True}},
    "cfg3_ppo_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "network": "amp_z", "env": "vae_ppo", "agent": "amp"},
    # the 52-body SMPL-X humanoid (robot/smplx_humanoid.yaml: non-upright rest pose) on the imitation env: observation 778 + 1248 = 2026 columns
    # (row pitch 2048), 153 actions
    "smplx_small": {"num_envs": 64, "horizon_length": 16, "minibatch_size": 256, "units": [512, 512], "humanoid": "smplx"},
}

# cfg.robot of the two shipped humanoids (robot/smpl_humanoid.yaml, robot/smplx_humanoid.yaml: humanoid_type and has_upright_start)
ROBOTS = {"smpl": {"humanoid_type": "smpl", "has_upright_start": True}, "smplx": {"humanoid_type": "smplx", "has_upright_start": False},
          "smplh": {"humanoid_type": "smplh", "has_upright_start": False}}
# the actuation switches as all three shipped robot files spell them (robot/smpl_humanoid.yaml:2, 8, 19-20 and the same lines of the other two):
# robot_config() carries them explicitly, so what a config computes does not hang on a default (env/robot_keys.py, "defaults")
ROBOT_ACTUATION = {"bias_offset": False, "has_smpl_pd_offset": False, "freeze_toe": False, "freeze_hand": False}


def robot_config(humanoid="smpl", **overrides):
    """cfg.robot of a shipped humanoid with the actuation switches spelled out, plus ``overrides``."""
    if humanoid not in ROBOTS:
        raise NotImplementedError(f"humanoid {humanoid!r}: 'smpl', 'smplh' and 'smplx' are built")
    return {**ROBOTS[humanoid], **ROBOT_ACTUATION, **overrides}


def agent_config(name, **overrides):
    c = CONFIGS[name]
    if c.get("network") == "amp_z":
        net = copy.deepcopy(NETWORK_Z)
    elif c.get("network") == "amp_sept":
        net = copy.deepcopy(NETWORK_SEPT)
        if "units" in c:
            net["mlp"]["units"] = list(c["units"])
    elif c.get("network") == "amp_mcp":
        net = copy.deepcopy(NETWORK_MCP)
        if "units" in c:
            net["mlp"]["units"] = list(c["units"])
    elif c.get("network") == "amp_pnn":
        net = copy.deepcopy(NETWORK_PNN)
        if "units" in c:
            net["mlp"]["units"] = list(c["units"])
    elif c.get("network") == "amp_z_reader":
        net = copy.deepcopy(NETWORK_Z_READER)
        if "units" in c:
            net["mlp"]["units"] = list(c["units"])
    else:
        net = copy.deepcopy(NETWORK_IM)
        net["mlp"]["units"] = list(c["units"])
    cfg = copy.deepcopy(PPO_IM)
    cfg.update({"horizon_length": c["horizon_length"], "minibatch_size": c["minibatch_size"], "network": net})
    cfg.update(c.get("extra", {}))
    cfg.update(overrides)
    cfg["_env_kind"], cfg["_agent_kind"], cfg["_humanoid"] = c.get("env", "im"), c.get("agent", "common"), c.get("humanoid", "smpl")
    cfg["_env_overrides"] = dict(c.get("env_overrides", {}))          # cfg["env"] keys the config itself sets (amp_pnn reads its four switches there)
    return cfg, c["num_envs"]


def make_env(num_envs, horizon, device, seed=1234, rank=0, rollout=None, env_kind="im", reference="recorded", env_overrides=None, humanoid="smpl",
             num_clips=None, robot_overrides=None, dof_limits=None, terrain=None):
    """``humanoid``: 'smpl' (24 bodies) | 'smplx' / 'smplh' (52 bodies) -- the robot config handed to the task as cfg.robot.
    ``reference``: 'recorded' = pre-recorded rigid-body / reference frames (RecordedRollout, what the CPU oracle agent replays);
    'motion_lib' = reference motion queried from the HBM-resident MotionLib every step, physics stand-in tracking it;
    'motion_data' = the same, with the library built on the device from synthetic RAW clips (MotionLib.from_motion_data: one resident clip per
    env out of ``num_clips`` unique ones -- min(num_envs, 1024) / 2 + 1 unless given -- re-drawn by resample_motions);
    'smpl_data' = the same one step earlier: synthetic raw SMPL pose sequences (axis-angle poses at 30 / 60 / 120 Hz) converted on the device by
    MotionLib.from_smpl_data (SMPL humanoid only);
    'mdm_data' = the same from synthetic GENERATED motion (per-joint Euler angles in degrees, 196 jittery frames a clip, as a text-to-motion
    model emits it): converted, sign-corrected and smoothed on the device by MotionLib.from_mdm_data (SMPL humanoid only).
    ``robot_overrides``: cfg.robot keys on top of the humanoid's (bias_offset, has_smpl_pd_offset, freeze_toe, freeze_hand, ...).
    ``dof_limits``: the joint limits the stand-in simulator publishes -- None (none: the PD-target table stays offset 0 / scale 1), True
    (synthetic.synthetic_dof_limits of the humanoid) or a (lower, upper) pair.
    ``env_kind`` 'mcp_demo' / 'im_demo': HumanoidImMCPDemo / HumanoidImDemo (env/humanoid_im_demo.py) over a KeypointStream the caller feeds, on
    RecordedSim / RecordedRollout -- the recorded stand-in does not follow the keypoints: it exercises the data path only.
    ``terrain`` (env_kind 'terrain_z'): a TERRAINS name or an env/terrain.py:Terrain the simulator publishes as ``sim.terrain`` -- the task
    then walks on its height field and resets onto its valid start cells."""
    from .env.humanoid_im import HumanoidIm, VecTaskPythonWrapper, check_humanoid_options
    robot = robot_config(humanoid, **(robot_overrides or {}))
    if terrain is not None and env_kind != "terrain_z":
        raise ValueError(f"make_env: terrain= belongs to env_kind 'terrain_z', not {env_kind!r}")
    if dof_limits is True:
        from . import synthetic as _syn
        dof_limits = _syn.synthetic_dof_limits(humanoid)
    if env_kind in ("speed_z", "reach_z", "strike_z", "terrain_z"):
        # HumanoidSpeedZ & co: synthetic task physics, the frozen decoder initialised from a (random-init) PULSE checkpoint
        import torch
        from .env import humanoid_tasks as HT
        from .learning.network_z import AMPZNetwork
        env_cfg = dict(ENV_TERRAIN_Z if env_kind == "terrain_z" else ENV_SPEED_Z)
        env_cfg.update(env_overrides or {})
        if isinstance(terrain, str):
            env_cfg.update(terrain_env(terrain))
            terrain = make_terrain(terrain, num_envs, device, seed=seed)
        # the terrain task's humanoids walk inside the synthetic height field (cells of 0.1 m): start them near its middle
        amp = bool(env_cfg.get("enable_amp_obs", False))
        sim = HT.SyntheticTaskSim(num_envs, horizon + 1, device, seed=seed, rank=rank, xy_offset=(13.0, 15.0) if env_kind == "terrain_z" else (0.0, 0.0),
                                  dof_pos_bank=amp, dof_limits=dof_limits, terrain=terrain)
        motion = None
        if amp:                                          # the HumanoidAMP layer resets from, looks back into and demonstrates with a motion library
            from . import synthetic as syn
            from .env.motion_lib import MotionLib
            motion = MotionLib.from_tables(syn.synthetic_motion_library(syn.make_generator(seed + 5, rank), min(num_envs, 1024)), device)
        cls = {"speed_z": HT.HumanoidSpeedZ, "reach_z": HT.HumanoidReachZ, "strike_z": HT.HumanoidStrikeZ,
               "terrain_z": HT.HumanoidPedestrianTerrainZ}[env_kind]
        task = cls({"env": env_cfg, "robot": robot}, sim, device=device, motion_lib=motion)
        znet = AMPZNetwork(NETWORK_Z, actions_num=69, self_obs_size=task.get_self_obs_size(), task_obs_size=576,
                           task_obs_size_detail=dict({"embedding_size": 32, "z_type": "vae", "use_vae_prior": True, "use_vae_clamped_prior": True,
                                                      "vae_var_clamp_max": 2}, **task._z_detail), device=device)   # (the env dict's prior / posterior variant)
        rms = {"running_mean": torch.zeros(934, dtype=torch.float64), "running_var": torch.ones(934, dtype=torch.float64)}
        task.initialize_z_models({"model": znet.state_dict(), "running_mean_std": rms}, NETWORK_Z)
        return VecTaskPythonWrapper(task, rl_device=device), None
    if env_kind == "mcp":
        # HumanoidImMCPGetup over the motion library (the get-up task needs its reference-state init) with a synthetic PNN checkpoint of
        # num_prim primitives sized to the env's observation
        from . import synthetic as syn
        from .env.humanoid_im_mcp import HumanoidImMCPGetup, check_mcp_options
        from .env.motion_lib import MotionLib
        from .env.sim import KinematicSim, PdSim
        env_cfg = dict(ENV_MCP)
        env_cfg.update(env_overrides or {})
        cfg = {"env": env_cfg, "robot": robot}
        opts = check_mcp_options(cfg, "HumanoidImMCPGetup")
        motion = MotionLib.from_tables(syn.synthetic_motion_library(syn.make_generator(seed + 5, rank), min(num_envs, 1024)), device)
        sim_cls = PdSim if env_cfg.pop("physics", "tracking") == "pd" else KinematicSim
        sim = sim_cls(num_envs, horizon + 1, device, seed=seed, rank=rank, dof_limits=dof_limits)
        # env.models given: that checkpoint (path or dict); otherwise the synthetic one, sized once the env knows its observation width
        make = None if env_cfg.get("models") else (lambda t: syn.synthetic_pnn_checkpoint(opts["num_prim"], in_dim=t.num_obs, seed=seed + 11,
                                                                                          has_lateral=opts["has_lateral"]))
        task = HumanoidImMCPGetup(cfg, sim, motion, device=device, pnn_checkpoint=make)
        return VecTaskPythonWrapper(task, rl_device=device), None
    if env_kind in ("mcp_demo", "im_demo"):
        # HumanoidImMCPDemo / HumanoidImDemo: the reference is a KeypointStream the caller feeds (task.push_keypoints), the physics the recorded
        # stand-in -- it does NOT follow the keypoints: this exercises the data path (stream -> observation -> policy -> PD targets) only.
        # The MCP demo gets the synthetic PNN checkpoint as "mcp" does.
        from . import synthetic as syn
        from .env.humanoid_im_demo import HumanoidImDemo, HumanoidImMCPDemo, check_demo_options
        from .env.humanoid_im_mcp import check_mcp_options
        from .env.sim import RecordedRollout, RecordedSim
        env_cfg = dict(ENV_MCP_DEMO if env_kind == "mcp_demo" else ENV_IM_DEMO)
        env_cfg.update(env_overrides or {})
        cfg = {"env": env_cfg, "robot": robot}
        name = "HumanoidImMCPDemo" if env_kind == "mcp_demo" else "HumanoidImDemo"
        check_demo_options(cfg, name)                   # an unbuilt combination raises by name before anything is allocated
        if syn.skeleton(humanoid) is not syn.SKELETONS["smpl"]:
            raise NotImplementedError(f"make_env: env_kind {env_kind!r} streams 24 SMPL keypoints; humanoid {humanoid!r} is not built")
        make = None
        if env_kind == "mcp_demo":
            opts = check_mcp_options(cfg, name)
            make = None if env_cfg.get("models") else (lambda t: syn.synthetic_pnn_checkpoint(opts["num_prim"], in_dim=t.num_obs, seed=seed + 11,
                                                                                              has_lateral=opts["has_lateral"]))
        if rollout is None:
            rollout = RecordedRollout(num_envs, horizon + 1, seed=seed, rank=rank, humanoid=humanoid)
        rollout.to(device)
        sim = RecordedSim(rollout, dof_limits=dof_limits)
        task = HumanoidImMCPDemo(cfg, sim, device=device, pnn_checkpoint=make) if env_kind == "mcp_demo" else HumanoidImDemo(cfg, sim, device=device)
        return VecTaskPythonWrapper(task, rl_device=device), rollout
    env_cfg = dict(ENV_IM_VAE) if env_kind in ("vae", "vae_ppo") else dict(ENV_IM)
    if env_kind == "vae_ppo":
        env_cfg.update({"only_kin_loss": False, "save_kin_info": False, "distill": False})
    if env_kind == "amp":
        env_cfg.update({"enable_amp_obs": True, "numAMPObsSteps": 10})
    env_cfg.update(env_overrides or {})
    if reference in ("motion_lib", "motion_data", "smpl_data", "mdm_data"):
        from . import synthetic as syn
        from .env.motion_lib import MotionLib
        from .env.sim import KinematicSim, PdSim
        cfg = {"env": env_cfg, "robot": robot}
        check_humanoid_options(cfg)                     # an unbuilt combination raises by name before anything is allocated
        disc_rows = any(bool(dict(robot, **env_cfg).get(k, False)) for k in ("has_shape_obs_disc", "has_weight_obs_disc"))
        if reference == "motion_data":
            g = syn.make_generator(seed + 5, rank)
            data, trees = syn.synthetic_motion_data(g, min(num_envs, 1024) // 2 + 1 if num_clips is None else int(num_clips), humanoid=humanoid,
                                                    num_slots=num_envs)
            bodies, limb = syn.motion_shape_rows(syn.make_generator(7117), num_envs)
            motion = MotionLib.from_motion_data(data, trees, gender_betas=bodies, limb_weights=limb, device=device, generator=g)
        elif reference == "smpl_data":
            if syn.skeleton(humanoid) is not syn.SKELETONS["smpl"]:
                raise NotImplementedError(f"make_env: reference 'smpl_data' converts SMPL pose sequences; humanoid {humanoid!r} is not built")
            g = syn.make_generator(seed + 5, rank)
            clips = min(num_envs, 1024) // 2 + 1 if num_clips is None else int(num_clips)
            data, trees = syn.synthetic_smpl_data(g, clips, framerate=[(30, 60, 120)[c % 3] for c in range(clips)], num_slots=num_envs)
            bodies, limb = syn.motion_shape_rows(syn.make_generator(7117), num_envs)
            motion = MotionLib.from_smpl_data(data, trees, gender_betas=bodies, limb_weights=limb, device=device, generator=g)
        elif reference == "mdm_data":
            if syn.skeleton(humanoid) is not syn.SKELETONS["smpl"]:
                raise NotImplementedError(f"make_env: reference 'mdm_data' converts generated SMPL motion; humanoid {humanoid!r} is not built")
            g = syn.make_generator(seed + 5, rank)
            clips = min(num_envs, 1024) // 2 + 1 if num_clips is None else int(num_clips)
            result, trees = syn.synthetic_mdm_result(g, clips, jitter=1.0, num_slots=num_envs)
            bodies, limb = syn.motion_shape_rows(syn.make_generator(7117), num_envs)
            motion = MotionLib.from_mdm_data(result, trees, gender_betas=bodies, limb_weights=limb, device=device, generator=g)
        else:
            tables = syn.synthetic_motion_library(syn.make_generator(seed + 5, rank), min(num_envs, 1024), humanoid=humanoid, shape_rows=disc_rows)
            motion = MotionLib.from_tables(tables, device)
        sim_cls = PdSim if env_cfg.pop("physics", "tracking") == "pd" else KinematicSim        # "pd": action-dependent stand-in
        sim = sim_cls(num_envs, horizon + 1, device, seed=seed, rank=rank, humanoid=humanoid, dof_limits=dof_limits)
        task = HumanoidIm(cfg, sim, motion, device=device)
        return VecTaskPythonWrapper(task, rl_device=device), None
    from .env.sim import RecordedMotion, RecordedRollout, RecordedSim
    cfg = {"env": env_cfg, "robot": robot}
    check_humanoid_options(cfg)
    if rollout is None:
        rollout = RecordedRollout(num_envs, horizon + 1, seed=seed, rank=rank, humanoid=humanoid)
    rollout.to(device)
    sim = RecordedSim(rollout, dof_limits=dof_limits)
    motion = RecordedMotion(rollout, sim)
    task = HumanoidIm(cfg, sim, motion, device=device)
    task.progress_buf.copy_(rollout.init_progress)
    return VecTaskPythonWrapper(task, rl_device=device), rollout


def make_agent(name="cfg2", device="cuda:0", seed=1234, rank=0, rollout=None, reference="recorded", env_overrides=None, humanoid=None, terrain=None,
               **overrides):
    from .learning.amp_agent import AMPAgent
    from .learning.common_agent import CommonAgent
    num_envs_override = overrides.pop("num_envs_override", None)
    cfg, num_envs = agent_config(name, **overrides)
    if num_envs_override is not None:
        num_envs = int(num_envs_override)
    vec_env, rollout = make_env(num_envs, cfg["horizon_length"], device, seed=seed, rank=rank, rollout=rollout, env_kind=cfg["_env_kind"],
                                reference=reference, env_overrides=dict(cfg["_env_overrides"], **(env_overrides or {})) or None, humanoid=humanoid if humanoid is not None else cfg["_humanoid"],
                                terrain=terrain)
    cfg.update({"vec_env": vec_env, "device": device, "seed": seed})
    cls = AMPAgent if cfg["_agent_kind"] == "amp" else CommonAgent
    return cls("pulse_amd", cfg), rollout


def make_player(name="cfg3_small", device="cuda:0", seed=1234, rank=0, rollout=None, reference="recorded", env_overrides=None, humanoid=None,
                z_source="posterior", prior_logvar=None, player=None, **overrides):
    """A player (learning/players.py) on the config ``name``, built as make_agent builds the agent.  ``z_source`` / ``prior_logvar``: where an
    amp_z policy's latent comes from -- make_player("cfg3_small", z_source="prior").generate(300, record=True) is motion generated from the
    PULSE prior alone (amp_network_z_builder.py:101-119).  ``player``: further config["player"] keys.  The options are validated against the
    config's network and env dict before the env or any device buffer is built."""
    from .learning import players
    num_envs_override = overrides.pop("num_envs_override", None)
    cfg, num_envs = agent_config(name, **overrides)
    if num_envs_override is not None:
        num_envs = int(num_envs_override)
    env_over = dict(cfg["_env_overrides"], **(env_overrides or {}))
    cfg["player"] = dict(player or {}, z_source=z_source, prior_logvar=prior_logvar)
    env = dict(ENV_IM_VAE if cfg["_env_kind"] in ("vae", "vae_ppo") else {}, **env_over)
    if "use_vae_fixed_prior" in env:                    # (as the env builds its task_obs_size_detail, env/humanoid_im.py)
        env.setdefault("use_vae_prior", False)
    players.check_z_source_options(cfg, detail=env)
    vec_env, _ = make_env(num_envs, cfg["horizon_length"], device, seed=seed, rank=rank, rollout=rollout, env_kind=cfg["_env_kind"],
                          reference=reference, env_overrides=env_over or None, humanoid=humanoid if humanoid is not None else cfg["_humanoid"])
    cfg.update({"vec_env": vec_env, "device": device, "seed": seed})
    cls = players.AMPPlayerContinuous if cfg["_agent_kind"] == "amp" else players.CommonPlayer
    return cls(cfg)
