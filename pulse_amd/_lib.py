"""ctypes binding of libpulse_hip.so (the C ABI declared in include/pulse_hip.h).

The library is the product: there is NO CPU / PyTorch fallback.  If the shared
object is missing or cannot be loaded every op raises ``PulseLibraryError``
loudly (build it with ``python pulse_amd/csrc/build.py`` or
``__graft_entry__.build()``).
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# PULSE_HIP_LIB: another build of the SAME library (tools/im_step_repro.py compares compile variants); default = the in-tree build
LIB_PATH = os.environ.get("PULSE_HIP_LIB") or os.path.join(_HERE, "csrc", "libpulse_hip.so")
ABI_VERSION = 36

PULSE_IM_SELF_OBS = 1
PULSE_IM_TASK_OBS = 2
PULSE_IM_REWARD = 4
PULSE_IM_RESET = 8
PULSE_IM_DEBUG_POISON_LDS = 0x80000000   # debug: the step kernel pre-fills its LDS with NaN
PULSE_IM_FORCE_WIDE = 0x40000000         # debug: 64-lane groups whatever the body count (bit-identical at <= 32 bodies)


class PulseLibraryError(RuntimeError):
    pass


class RewardSpecs(Structure):
    _fields_ = [("k_pos", c_float), ("k_rot", c_float), ("k_vel", c_float), ("k_ang_vel", c_float),
                ("w_pos", c_float), ("w_rot", c_float), ("w_vel", c_float), ("w_ang_vel", c_float),
                ("power_coef", c_float), ("power_reward", c_int32)]


class MotionTables(Structure):
    _fields_ = [("frames", c_void_p), ("frame_stride", c_int64), ("total_frames", c_int64), ("num_bodies", c_int32),
                ("off_gts", c_int32), ("off_grs", c_int32), ("off_lrs", c_int32), ("off_gvs", c_int32), ("off_gavs", c_int32),
                ("off_dvs", c_int32),
                ("motion_lengths", c_void_p), ("motion_dt", c_void_p), ("motion_num_frames", c_void_p), ("length_starts", c_void_p),
                ("num_motions", c_int32)]


class MotionBuildArgs(Structure):
    _fields_ = [("src_rot", c_void_p), ("src_trans", c_void_p), ("src_frames", c_int64), ("num_clips", c_int32), ("num_bodies", c_int32),
                ("clip_src_start", c_void_p), ("clip_crop_start", c_void_p), ("clip_out_start", c_void_p), ("clip_frames_host", c_void_p),
                ("clip_dt", c_void_p), ("clip_heading", c_void_p), ("local_translation", c_void_p), ("parent_indices_host", c_void_p),
                ("frames", c_void_p), ("total_frames", c_int64), ("frame_stride", c_int64),
                ("off_gts", c_int32), ("off_grs", c_int32), ("off_lrs", c_int32), ("off_gvs", c_int32), ("off_gavs", c_int32), ("off_dvs", c_int32),
                ("filter_w", c_float * 9)]


class MotionIngestArgs(Structure):
    _fields_ = [("src_pose", c_void_p), ("src_trans", c_void_p), ("src_frames", c_int64), ("num_clips", c_int32), ("num_bodies", c_int32),
                ("clip_src_start", c_void_p), ("clip_skip", c_void_p), ("clip_mirror", c_void_p), ("clip_out_start", c_void_p),
                ("clip_src_start_host", c_void_p), ("clip_skip_host", c_void_p), ("clip_frames_host", c_void_p), ("parent_indices_host", c_void_p),
                ("joint_map", c_int32 * 32), ("mirror_map", c_int32 * 32), ("upright_start", c_int32), ("root_offset", c_float * 3),
                ("out_rot", c_void_p), ("out_trans", c_void_p), ("out_pose_quat", c_void_p), ("out_pose_aa", c_void_p), ("out_trans_orig", c_void_p),
                ("total_frames", c_int64)]


class MotionEulerPoseArgs(Structure):
    _fields_ = [("src_theta", c_void_p), ("src_trans", c_void_p), ("total_frames", c_int64), ("num_clips", c_int32), ("reserved", c_int32),
                ("clip_start", c_void_p), ("clip_frames_host", c_void_p), ("root_quat", c_double * 4), ("trans_matrix", c_double * 9),
                ("floor_height", c_double), ("out_pose", c_void_p), ("out_trans", c_void_p)]


class MotionSmoothArgs(Structure):
    _fields_ = [("in_rot", c_void_p), ("in_trans", c_void_p), ("total_frames", c_int64), ("num_clips", c_int32), ("num_bodies", c_int32),
                ("clip_start", c_void_p), ("clip_frames_host", c_void_p), ("parent_indices_host", c_void_p), ("sign_words", c_void_p),
                ("radius_rot", c_int32), ("radius_trans", c_int32), ("w_rot", c_double * 13), ("w_trans", c_double * 13),
                ("out_rot", c_void_p), ("out_trans", c_void_p), ("out_pose_quat", c_void_p)]


class MotionExportArgs(Structure):
    _fields_ = [("rb", c_void_p), ("rb_stride_t", c_int64), ("rb_stride_n", c_int64), ("rb_stride_b", c_int64),
                ("dof_pos", c_void_p), ("dof_stride_t", c_int64), ("dof_stride_n", c_int64), ("num_steps", c_int64),
                ("num_envs", c_int32), ("num_bodies", c_int32), ("num_segments", c_int32), ("upright_start", c_int32),
                ("seg_env", c_void_p), ("seg_t0", c_void_p), ("seg_out_start", c_void_p),
                ("seg_env_host", c_void_p), ("seg_t0_host", c_void_p), ("seg_frames_host", c_void_p), ("parent_indices_host", c_void_p),
                ("joint_map", c_int32 * 32), ("root_offset", c_float * 3), ("reserved", c_int32),
                ("out_rot", c_void_p), ("out_trans", c_void_p), ("out_pose_quat", c_void_p), ("out_pose_aa", c_void_p), ("out_trans_orig", c_void_p),
                ("out_body_quat", c_void_p), ("out_dof_pos", c_void_p), ("total_frames", c_int64)]


class KeypointPushArgs(Structure):
    _fields_ = [("j3d", c_void_p), ("j3d_stride_n", c_int64), ("j3d_stride_j", c_int64), ("num_envs", c_int32), ("num_bodies", c_int32),
                ("history", c_int32), ("dt", c_float), ("env_mask", c_void_p), ("taps", c_void_p), ("joint_map", c_int32 * 32),
                ("parent_indices", c_int32 * 32), ("mean_limb_lengths", c_float * 5), ("frame", c_float * 9), ("reserved", c_int32 * 2),
                ("root_ring", c_void_p), ("body_ring", c_void_p), ("count", c_void_p), ("prev_pos", c_void_p),
                ("pos", c_void_p), ("vel", c_void_p), ("raw", c_void_p)]


class ImEvalArgs(Structure):
    _fields_ = [("rb", c_void_p), ("rb_env_stride", c_int64), ("ref_pos", c_void_p), ("ref_env_stride", c_int64), ("num_envs", c_int32),
                ("num_bodies", c_int32), ("num_steps", c_void_p), ("step", c_int32), ("env_mask", c_void_p), ("ring", c_void_p),
                ("accum", c_void_p), ("accum_stride", c_int64)]


class ImStepArgs(Structure):
    _fields_ = [
        ("rb", c_void_p), ("rb_env_stride", c_int64), ("num_envs", c_int32), ("num_bodies", c_int32),
        ("env_ids", c_void_p), ("num_ids", c_int32), ("env_mask", c_void_p),
        ("ref_now_pos", c_void_p), ("ref_now_rot", c_void_p), ("ref_now_vel", c_void_p), ("ref_now_ang", c_void_p),
        ("ref_next_pos", c_void_p), ("ref_next_rot", c_void_p), ("ref_next_vel", c_void_p), ("ref_next_ang", c_void_p),
        ("time_steps", c_int32),
        ("dof_force", c_void_p), ("dof_vel", c_void_p), ("num_dof", c_int32),
        ("progress", c_void_p), ("pass_time", c_void_p), ("cycle_counter", c_void_p),
        ("track_ids", c_void_p), ("num_track", c_int32), ("reset_ids", c_void_p), ("num_reset", c_int32),
        ("term_dist", c_void_p), ("reset_use_mean", c_int32), ("full_body_reward", c_int32),
        ("what", c_uint32), ("obs_version", c_int32), ("local_root_obs", c_int32), ("root_height_obs", c_int32),
        ("specs", RewardSpecs),
        ("upright_start", c_int32), ("enable_early_termination", c_int32), ("self_obs_version", c_int32), ("hist_steps", c_int32),
        ("force_sensor", c_void_p), ("force_sensor_width", c_int32), ("dof_pos", c_void_p), ("ref_next_dof_pos", c_void_p),
        ("obs", c_void_p), ("obs_stride", c_int64), ("obs_cols", c_int32),
        ("rew", c_void_p), ("rew_raw", c_void_p), ("reset", c_void_p), ("terminate", c_void_p),
        ("progress_rw", c_void_p), ("progress_inc", c_int32), ("clock_dt", c_float),
        ("clock_start_times", c_void_p), ("clock_start_offsets", c_void_p), ("clock_motion_len", c_void_p),
        ("cycle_motion", c_int32), ("max_episode_length", c_int32), ("pass_time_out", c_void_p),
        ("use_motion", c_int32), ("motion", MotionTables), ("motion_ids", c_void_p), ("motion_offset", c_void_p), ("traj_dt", c_float),
        ("track_rb", c_void_p), ("track_rb_stride", c_int64), ("track_dof_pos", c_void_p), ("track_dof_vel", c_void_p),
        ("smpl_params", c_void_p), ("smpl_params_width", c_int32), ("smpl_params_stride", c_int64),
        ("limb_weights", c_void_p), ("limb_weights_width", c_int32), ("limb_weights_stride", c_int64),
        ("recovery_counter", c_void_p),
        ("zero_out_far", c_int32), ("close_distance", c_float), ("far_distance", c_float), ("point_goal", c_void_p),
        ("occl_bits", c_void_p), ("occl_reset", c_int32),
        ("obs_copy", c_void_p), ("obs_copy_stride", c_int64),
    ]


class TaskStepArgs(Structure):
    _fields_ = [
        ("task", c_int32), ("what", c_uint32), ("num_envs", c_int32), ("env_ids", c_void_p), ("num_ids", c_int32), ("env_mask", c_void_p),
        ("rb", c_void_p), ("rb_env_stride", c_int64), ("num_bodies", c_int32), ("prev_root_pos", c_void_p), ("dt", c_float),
        ("tar_speed", c_void_p), ("tar_pos", c_void_p), ("reach_body_id", c_int32), ("tar_states", c_void_p),
        ("tar_contact_forces", c_void_p), ("strike_body_ids", c_void_p), ("num_strike", c_int32),
        ("contact_forces", c_void_p), ("contact_body_ids", c_void_p), ("num_contact_ids", c_int32), ("termination_heights", c_void_p),
        ("progress", c_void_p), ("max_episode_length", c_float), ("enable_early_termination", c_int32),
        ("dof_force", c_void_p), ("dof_vel", c_void_p), ("num_dof", c_int32), ("power_coef", c_float), ("power_reward", c_int32),
        ("obs", c_void_p), ("obs_stride", c_int64), ("obs_offset", c_int32),
        ("rew", c_void_p), ("rew_raw", c_void_p), ("rew_raw_width", c_int32), ("reset", c_void_p), ("terminate", c_void_p),
    ]


TASK_SPEED, TASK_REACH, TASK_STRIKE = 1, 2, 3
TASK_OBS, TASK_REWARD, TASK_RESET = 1, 2, 4


class AmpObsArgs(Structure):
    _fields_ = [("rb", c_void_p), ("rb_env_stride", c_int64), ("dof_pos", c_void_p), ("dof_vel", c_void_p), ("num_dof", c_int32),
                ("num_envs", c_int32), ("env_ids", c_void_p), ("num_ids", c_int32), ("env_mask", c_void_p),
                ("joint_ids", c_void_p), ("num_joints", c_int32), ("zero_joint_mask", c_uint32),
                ("key_body_ids", c_void_p), ("num_key_bodies", c_int32), ("local_root_obs", c_int32), ("root_height_obs", c_int32),
                ("out", c_void_p), ("out_stride", c_int64),
                ("hist_steps", c_int32), ("window_out", c_void_p), ("window_stride", c_int64),
                ("upright_start", c_int32), ("version", c_int32),
                ("shape_params", c_void_p), ("shape_stride", c_int64), ("num_shape", c_int32),
                ("limb_weights", c_void_p), ("limb_stride", c_int64), ("num_limb", c_int32)]


class B16Transpose(Structure):
    _fields_ = [("in_", c_void_p), ("ld_in", c_int64), ("rows", c_int32), ("cols", c_int32), ("out", c_void_p), ("ld_out", c_int64),
                ("batch", c_int32), ("reserved", c_int32), ("stride_in", c_int64), ("stride_out", c_int64)]


class AmpHistArgs(Structure):
    _fields_ = [("tab", MotionTables), ("motion_ids", c_void_p), ("start_times", c_void_p), ("dt", c_float),
                ("num_envs", c_int32), ("env_mask", c_void_p), ("hist_steps", c_int32),
                ("joint_ids", c_void_p), ("num_joints", c_int32), ("key_body_ids", c_void_p), ("num_key_bodies", c_int32),
                ("local_root_obs", c_int32), ("root_height_obs", c_int32),
                ("hist", c_void_p), ("env_stride", c_int64), ("step_stride", c_int64),
                ("upright_start", c_int32), ("version", c_int32),
                ("shape_params", c_void_p), ("shape_stride", c_int64), ("num_shape", c_int32),
                ("limb_weights", c_void_p), ("limb_stride", c_int64), ("num_limb", c_int32)]


TASK_RESET_NONE, TASK_RESET_ZERO_XY, TASK_RESET_REMOVE_HEADING, TASK_RESET_TERRAIN = 0, 1, 2, 3      # PULSE_TASK_RESET_*


class TaskResetArgs(Structure):
    _fields_ = [("tab", MotionTables), ("num_envs", c_int32), ("transform", c_int32), ("upright_start", c_int32),
                ("env_mask", c_void_p), ("motion_ids", c_void_p), ("times", c_void_p),
                ("new_root_xy", c_void_p),
                ("heightsamples", c_void_p), ("map_rows", c_int32), ("map_cols", c_int32), ("horizontal_scale", c_float), ("vertical_scale", c_float),
                ("center_points", c_void_p), ("num_center_points", c_int32),
                ("rb", c_void_p), ("rb_env_stride", c_int64), ("dof_pos", c_void_p), ("dof_vel", c_void_p),
                ("start_times", c_void_p), ("sampled_ids", c_void_p),
                ("clear0", c_void_p), ("clear1", c_void_p), ("clear2", c_void_p)]


class MotionStateArgs(Structure):
    _fields_ = [("tab", MotionTables), ("n", c_int64), ("motion_ids", c_void_p), ("motion_times", c_void_p),
                ("progress", c_void_p), ("step_shift", c_int32), ("dt", c_float), ("start_times", c_void_p), ("start_offsets", c_void_p),
                ("time_steps", c_int32), ("traj_dt", c_float), ("offset", c_void_p), ("root_only", c_int32),
                ("rg_pos", c_void_p), ("rb_rot", c_void_p), ("body_vel", c_void_p), ("body_ang_vel", c_void_p),
                ("dof_pos", c_void_p), ("dof_vel", c_void_p), ("root_pos", c_void_p),
                ("rb_records", c_void_p), ("rb_query_stride", c_int64),
                ("frame_idx0", c_void_p), ("frame_idx1", c_void_p), ("blend", c_void_p),
                ("reset_mask", c_void_p), ("reset_phase", c_void_p), ("reset_start_times", c_void_p), ("reset_progress", c_void_p),
                ("reset_clear0", c_void_p), ("reset_clear1", c_void_p), ("reset_time_interval", c_int32),
                ("reset_start_offsets", c_void_p), ("reset_global_offset", c_void_p), ("reset_clear2", c_void_p)]


class RolloutRecordArgs(Structure):
    _fields_ = [("num_envs", c_int32), ("rewards", c_void_p), ("reward_scale", c_float), ("reward_shift", c_float),
                ("dones", c_void_p), ("terminate", c_void_p), ("value_raw", c_void_p), ("value_stride", c_int64),
                ("value_mean", c_void_p), ("value_var", c_void_p), ("value_eps", c_float),
                ("buf_rewards", c_void_p), ("buf_next_values", c_void_p), ("buf_dones", c_void_p), ("env_stride", c_int64),
                ("current_rewards", c_void_p), ("current_lengths", c_void_p), ("meter_rewards", c_void_p), ("meter_lengths", c_void_p),
                ("meter_max_size", c_float), ("done_mask", c_void_p), ("buf_terminate", c_void_p),
                ("meter_partials", c_void_p), ("meter_blocks", c_int32)]


class PdSimArgs(Structure):
    _fields_ = [("num_envs", c_int64), ("num_bodies", c_int32), ("target_rb", c_void_p), ("target_dof_pos", c_void_p), ("target_dof_vel", c_void_p),
                ("action", c_void_p), ("noise_acc", c_void_p), ("sag", c_void_p), ("lever_dir", c_void_p),
                ("kp", c_float), ("kd", c_float), ("dt", c_float), ("action_scale", c_float), ("lever", c_float), ("substeps", c_int32),
                ("err", c_void_p), ("err_vel", c_void_p), ("rb", c_void_p), ("dof_pos", c_void_p), ("dof_vel", c_void_p), ("dof_force", c_void_p),
                ("reset_mask", c_void_p)]


class TrajStepArgs(Structure):
    _fields_ = [("what", c_uint32), ("num_envs", c_int32), ("env_ids", c_void_p), ("num_ids", c_int32), ("env_mask", c_void_p),
                ("rb", c_void_p), ("rb_env_stride", c_int64), ("num_bodies", c_int32), ("upright_start", c_int32),
                ("progress", c_void_p), ("dt", c_float),
                ("verts", c_void_p), ("num_verts", c_int32), ("traj_dur", c_float), ("num_samples", c_int32), ("sample_timestep", c_float),
                ("heightsamples", c_void_p), ("map_rows", c_int32), ("map_cols", c_int32), ("horizontal_scale", c_float), ("vertical_scale", c_float),
                ("height_points", c_void_p), ("num_height_points", c_int32), ("sensor_body", c_int32),
                ("center_points", c_void_p), ("num_center_points", c_int32), ("use_center_height", c_int32), ("height_meas_scale", c_float),
                ("dof_force", c_void_p), ("dof_vel", c_void_p), ("num_dof", c_int32), ("power_coef", c_float), ("power_reward", c_int32),
                ("fuzzy_target", c_int32),
                ("contact_forces", c_void_p), ("contact_body_ids", c_void_p), ("num_contact_ids", c_int32), ("termination_heights", c_void_p),
                ("max_episode_length", c_float), ("fail_dist", c_float), ("enable_early_termination", c_int32), ("terrain_reset", c_int32),
                ("disable_collision", c_int32),
                ("obs", c_void_p), ("obs_stride", c_int64), ("obs_offset", c_int32), ("rew", c_void_p), ("rew_raw", c_void_p),
                ("reset", c_void_p), ("terminate", c_void_p)]


class TrajGenArgs(Structure):
    _fields_ = [("num_envs", c_int32), ("num_verts", c_int32), ("env_mask", c_void_p), ("rb", c_void_p), ("rb_env_stride", c_int64),
                ("u_dtheta", c_void_p), ("u_sharp", c_void_p), ("sharp_mask", c_void_p), ("u_heading", c_void_p), ("u_dspeed", c_void_p),
                ("u_speed0", c_void_p), ("dtheta_scale", c_float), ("dspeed_scale", c_float), ("seg_dt", c_float), ("speed_min", c_float),
                ("speed_max", c_float), ("verts", c_void_p)]


class CrowdGroupObsArgs(Structure):
    _fields_ = [("num_envs", c_int32), ("group_size", c_int32), ("env_ids", c_void_p), ("num_ids", c_int32), ("env_mask", c_void_p),
                ("rb", c_void_p), ("rb_env_stride", c_int64), ("num_bodies", c_int32), ("upright_start", c_int32),
                ("obs", c_void_p), ("obs_stride", c_int64), ("obs_offset", c_int32)]


class CrowdStampArgs(Structure):
    _fields_ = [("num_envs", c_int32), ("group_size", c_int32), ("rb", c_void_p), ("rb_env_stride", c_int64),
                ("map_rows", c_int32), ("map_cols", c_int32), ("horizontal_scale", c_float),
                ("owner", c_void_p), ("cells", c_void_p), ("clear", c_int32)]


class CrowdHeightsArgs(Structure):
    _fields_ = [("num_envs", c_int32), ("group_size", c_int32), ("env_ids", c_void_p), ("num_ids", c_int32), ("env_mask", c_void_p),
                ("rb", c_void_p), ("rb_env_stride", c_int64), ("num_bodies", c_int32), ("upright_start", c_int32),
                ("heightsamples", c_void_p), ("map_rows", c_int32), ("map_cols", c_int32), ("horizontal_scale", c_float), ("vertical_scale", c_float),
                ("owner", c_void_p), ("stamp_raise", c_int32),
                ("height_points", c_void_p), ("num_height_points", c_int32), ("sensor_body", c_int32),
                ("center_points", c_void_p), ("num_center_points", c_int32), ("use_center_height", c_int32), ("height_meas_scale", c_float),
                ("velocity_map", c_int32),
                ("obs", c_void_p), ("obs_stride", c_int64), ("obs_offset", c_int32)]


class TerrainWalkableArgs(Structure):
    _fields_ = [("rows", c_int32), ("cols", c_int32), ("heights", c_void_p), ("tile_flags", c_void_p), ("tile_rows", c_int32),
                ("tile_cols", c_int32), ("border", c_int32), ("length_px", c_int32), ("width_px", c_int32), ("obstacle_mask", c_void_p),
                ("iterations", c_int32), ("walkable", c_void_p)]


class TerrainValidArgs(Structure):
    _fields_ = [("rows", c_int32), ("cols", c_int32), ("walkable", c_void_p), ("horizontal_scale", c_float), ("border_scaled", c_float),
                ("row_extents", c_void_p), ("row_offsets", c_void_p), ("coord_x", c_void_p), ("coord_y", c_void_p), ("capacity", c_int64),
                ("count", c_void_p)]


class TerrainSampleArgs(Structure):
    _fields_ = [("num_envs", c_int32), ("env_mask", c_void_p), ("coord_x", c_void_p), ("coord_y", c_void_p), ("num_samples", c_int64),
                ("idx", c_void_p), ("group_num_people", c_int32), ("extent_x", c_float), ("extent_y", c_float),
                ("u_center", c_void_p), ("u_dx", c_void_p), ("u_dy", c_void_p), ("out", c_void_p)]


TERRAIN_MAX_DILATION = 16                            # PULSE_TERRAIN_MAX_DILATION
CROWD_GROUP_OBS, CROWD_ROOT_POINTS = 165, 200        # PULSE_CROWD_GROUP_OBS, PULSE_CROWD_ROOT_POINTS


class VaeEmbedArgs(Structure):
    _fields_ = [("heads", c_void_p), ("heads_stride", c_int64), ("eps", c_void_p), ("eps_stride", c_int64), ("x", c_void_p), ("x_stride", c_int64),
                ("ain", c_void_p), ("ain_stride", c_int64), ("cin", c_void_p), ("cin_stride", c_int64),
                ("rows", c_int32), ("embedding_size", c_int32), ("self_obs_size", c_int32), ("z_col", c_int32),
                ("clamp_logvar", c_int32), ("clamp_max", c_float), ("sphere_posterior", c_int32), ("embedding_norm", c_float)]


class VaeEmbedPriorArgs(Structure):
    _fields_ = [("pheads", c_void_p), ("pheads_stride", c_int64), ("eps", c_void_p), ("eps_stride", c_int64), ("x", c_void_p), ("x_stride", c_int64),
                ("ain", c_void_p), ("ain_stride", c_int64), ("cin", c_void_p), ("cin_stride", c_int64), ("z_out", c_void_p), ("z_out_stride", c_int64),
                ("rows", c_int32), ("embedding_size", c_int32), ("self_obs_size", c_int32), ("z_col", c_int32),
                ("prior_mode", c_int32), ("prior_fixed_logvar", c_float), ("clamp_logvar", c_int32), ("clamp_max", c_float),
                ("logvar_override", c_int32), ("logvar_override_value", c_float),
                ("sphere_prior", c_int32), ("sphere_posterior", c_int32), ("embedding_norm", c_float)]


class VaeKinArgs(Structure):
    _fields_ = [("pred", c_void_p), ("pred_stride", c_int64), ("gt", c_void_p), ("gt_stride", c_int64),
                ("zheads", c_void_p), ("zheads_stride", c_int64), ("pheads", c_void_p), ("pheads_stride", c_int64), ("progress", c_void_p),
                ("rows", c_int32), ("num_actions", c_int32), ("embedding_size", c_int32), ("horizon", c_int32),
                ("clamp_logvar", c_int32), ("clamp_max", c_float), ("use_ar1", c_int32), ("use_regu", c_int32),
                ("dmu", c_void_p), ("dmu_stride", c_int64), ("partials", c_void_p), ("num_blocks", c_int32),
                ("prior_mode", c_int32), ("prior_fixed_logvar", c_float), ("sphere_prior", c_int32), ("embedding_norm", c_float)]


class VaeHeadBwdArgs(Structure):
    _fields_ = [("zheads", c_void_p), ("zheads_stride", c_int64), ("pheads", c_void_p), ("pheads_stride", c_int64),
                ("eps", c_void_p), ("eps_stride", c_int64), ("dz", c_void_p), ("dz_stride", c_int64), ("progress", c_void_p),
                ("rows", c_int32), ("embedding_size", c_int32), ("horizon", c_int32), ("clamp_logvar", c_int32), ("clamp_max", c_float),
                ("c_kl", c_float), ("c_ar1", c_float), ("c_regu", c_float),
                ("dzheads", c_void_p), ("dzheads_stride", c_int64), ("dpheads", c_void_p), ("dpheads_stride", c_int64),
                ("prior_mode", c_int32), ("prior_fixed_logvar", c_float), ("sphere_prior", c_int32), ("sphere_posterior", c_int32),
                ("embedding_norm", c_float)]


class GemmX3pDesc(Structure):
    _fields_ = [("A", c_void_p), ("a_plane_stride", c_int64), ("lda", c_int32),
                ("B", c_void_p), ("b_plane_stride", c_int64), ("ldb", c_int32),
                ("a_layout", c_int32), ("b_layout", c_int32),
                ("C", c_void_p), ("ldc", c_int32),
                ("Cp", c_void_p), ("c_plane_stride", c_int64), ("ldcp", c_int32),
                ("C2", c_void_p), ("ldc2", c_int32),
                ("bias", c_void_p), ("aux", c_void_p), ("ldaux", c_int32),
                ("M", c_int32), ("N", c_int32), ("K", c_int32), ("batch", c_int32),
                ("stride_a", c_int64), ("stride_b", c_int64), ("stride_c", c_int64), ("stride_cp", c_int64), ("stride_c2", c_int64),
                ("stride_bias", c_int64), ("stride_aux", c_int64),
                ("split_k", c_int32), ("split_stride", c_int64), ("activation", c_int32), ("epilogue", c_int32),
                ("rowsum", c_void_p), ("stride_rowsum", c_int64), ("planes", c_int32), ("aux_is_bf16", c_int32),
                ("out_colsum", c_void_p), ("stride_out_colsum", c_int64), ("ld_out_colsum", c_int32),
                ("relu_mask8", c_void_p), ("ld_mask8", c_int32), ("stride_mask8", c_int64)]


class GemmDesc(Structure):
    _fields_ = [
        ("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("C2", c_void_p), ("bias", c_void_p), ("aux", c_void_p),
        ("M", c_int32), ("N", c_int32), ("K", c_int32),
        ("lda", c_int32), ("ldb", c_int32), ("ldc", c_int32), ("ldc2", c_int32), ("ldaux", c_int32),
        ("a_layout", c_int32), ("b_layout", c_int32), ("batch", c_int32),
        ("stride_a", c_int64), ("stride_b", c_int64), ("stride_c", c_int64), ("stride_c2", c_int64),
        ("stride_bias", c_int64), ("stride_aux", c_int64),
        ("split_k", c_int32), ("split_stride", c_int64), ("activation", c_int32), ("epilogue", c_int32),
        ("rowsum", c_void_p), ("stride_rowsum", c_int64),
        ("compute_type", c_int32), ("round_output_bf16", c_int32),
        ("relu_mask", c_void_p), ("ld_mask", c_int32), ("stride_mask", c_int64),
    ]


class PpoLossArgs(Structure):
    _fields_ = [
        ("mu", c_void_p), ("mu_stride", c_int64), ("value", c_void_p), ("value_stride", c_int64), ("logstd", c_void_p),
        ("idx", c_void_p), ("actions", c_void_p), ("actions_stride", c_int64), ("old_mu", c_void_p), ("old_mu_stride", c_int64),
        ("old_logstd", c_void_p), ("old_neglogp", c_void_p), ("advantages", c_void_p), ("old_values", c_void_p), ("returns", c_void_p),
        ("rows", c_int32), ("num_actions", c_int32),
        ("e_clip", c_float), ("critic_coef", c_float), ("bounds_loss_coef", c_float), ("clip_value", c_int32), ("has_bounds_loss", c_int32),
        ("dmu", c_void_p), ("dmu_stride", c_int64), ("dvalue", c_void_p), ("dvalue_stride", c_int64),
        ("partials", c_void_p), ("num_blocks", c_int32),
        ("dmu16", c_void_p), ("dmu16_stride", c_int64), ("dvalue16", c_void_p), ("dvalue16_stride", c_int64),
    ]


GEMM_RED_CONTIG, GEMM_OUT_CONTIG = 0, 1
GEMM_COMPUTE_F32, GEMM_COMPUTE_BF16, GEMM_COMPUTE_F32X3 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_SILU, ACT_SILU_D = 0, 1, 2, 3          # SILU_D: C2 receives d silu / d z instead of z (backward: EPI_MUL_AUX)
EPI_BIAS_ACT, EPI_RELU_GRAD, EPI_SILU_GRAD, EPI_MUL_AUX = 0, 1, 2, 3

P = c_void_p  # every device pointer crosses the ABI as void*
c_double = ctypes.c_double

# name -> (restype, argtypes); must list EVERY symbol of include/pulse_hip.h
SIGNATURES = {
    "pulse_abi_version": (c_int, []),
    "pulse_last_error": (c_char_p, []),
    "pulse_quat_mul": (c_int, [P, P, P, c_int64, P]),
    "pulse_quat_conjugate": (c_int, [P, P, c_int64, P]),
    "pulse_quat_rotate": (c_int, [P, P, P, c_int64, P]),
    "pulse_quat_to_angle_axis": (c_int, [P, P, P, c_int64, P]),
    "pulse_quat_to_exp_map": (c_int, [P, P, c_int64, P]),
    "pulse_quat_to_tan_norm": (c_int, [P, P, c_int64, P]),
    "pulse_exp_map_to_quat": (c_int, [P, P, c_int64, P]),
    "pulse_slerp": (c_int, [P, P, P, P, c_int64, P]),
    "pulse_calc_heading": (c_int, [P, P, c_int64, P]),
    "pulse_calc_heading_quat": (c_int, [P, P, c_int64, c_int, P]),
    "pulse_sizeof_im_step_args": (c_int, []),
    "pulse_self_obs_width": (c_int, [c_int, c_int]),
    "pulse_task_obs_width": (c_int, [c_int, c_int, c_int]),
    "pulse_self_obs_width_ex": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "pulse_im_step": (c_int, [POINTER(ImStepArgs), P]),
    "pulse_sizeof_task_step_args": (c_int, []),
    "pulse_task_obs_size": (c_int, [c_int]),
    "pulse_task_step": (c_int, [POINTER(TaskStepArgs), P]),
    "pulse_gemm_set_option": (c_int, [c_int, c_int]),
    "pulse_gemm_set_debug_buffer": (c_int, [P]),
    "pulse_gemm_last_tile": (c_int, []),
    "pulse_gemm_x3_mode": (c_int, []),
    "pulse_sizeof_amp_obs_args": (c_int, []),
    "pulse_amp_obs_width": (c_int, [c_int, c_int, c_int]),
    "pulse_amp_obs_width_v": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "pulse_amp_obs": (c_int, [POINTER(AmpObsArgs), P]),
    "pulse_sizeof_amp_hist_args": (c_int, []),
    "pulse_amp_hist_init": (c_int, [POINTER(AmpHistArgs), P]),
    "pulse_sizeof_task_reset_args": (c_int, []),
    "pulse_task_ref_state_init": (c_int, [POINTER(TaskResetArgs), P]),
    "pulse_sizeof_rollout_record_args": (c_int, []),
    "pulse_rollout_record": (c_int, [POINTER(RolloutRecordArgs), P]),
    "pulse_rollout_meters": (c_int, [P, c_int32, c_int32, P, P, c_float, P]),
    "pulse_kinematic_sim_step": (c_int, [P, P, P, c_int64, c_int32, P, P, P, P, P, P, P, P, c_int32, P]),
    "pulse_sizeof_pd_sim_args": (c_int, []),
    "pulse_pd_sim_step": (c_int, [POINTER(PdSimArgs), P]),
    "pulse_sizeof_motion_state_args": (c_int, []),
    "pulse_motion_state": (c_int, [POINTER(MotionStateArgs), P]),
    "pulse_sizeof_motion_build_args": (c_int, []),
    "pulse_motion_build": (c_int, [POINTER(MotionBuildArgs), P]),
    "pulse_sizeof_motion_ingest_args": (c_int, []),
    "pulse_motion_ingest": (c_int, [POINTER(MotionIngestArgs), P]),
    "pulse_sizeof_motion_euler_pose_args": (c_int, []),
    "pulse_motion_euler_pose": (c_int, [POINTER(MotionEulerPoseArgs), P]),
    "pulse_sizeof_motion_smooth_args": (c_int, []),
    "pulse_motion_smooth": (c_int, [POINTER(MotionSmoothArgs), P]),
    "pulse_sizeof_motion_export_args": (c_int, []),
    "pulse_motion_export": (c_int, [POINTER(MotionExportArgs), P]),
    "pulse_sizeof_keypoint_push_args": (c_int, []),
    "pulse_keypoint_push": (c_int, [POINTER(KeypointPushArgs), P]),
    "pulse_sizeof_im_eval_args": (c_int, []),
    "pulse_im_eval_accum": (c_int, [POINTER(ImEvalArgs), P]),
    "pulse_gae": (c_int, [P, P, P, P, c_int32, c_int32, c_int64, c_int64, c_float, c_float, P, P, P]),
    "pulse_sizeof_gemm_desc": (c_int, []),
    "pulse_gemm_f32": (c_int, [POINTER(GemmDesc), P]),
    "pulse_gemm_x3p": (c_int, [POINTER(GemmX3pDesc), P]),
    "pulse_gemm_x3p_row_tiles": (c_int, [c_int32, c_int32, c_int32]),
    "pulse_traj_step": (c_int, [POINTER(TrajStepArgs), P]),
    "pulse_sizeof_traj_step_args": (c_int, []),
    "pulse_traj_generate": (c_int, [POINTER(TrajGenArgs), P]),
    "pulse_sizeof_crowd_group_obs_args": (c_int, []),
    "pulse_crowd_group_obs": (c_int, [POINTER(CrowdGroupObsArgs), P]),
    "pulse_sizeof_crowd_stamp_args": (c_int, []),
    "pulse_crowd_stamp": (c_int, [POINTER(CrowdStampArgs), P]),
    "pulse_sizeof_crowd_heights_args": (c_int, []),
    "pulse_crowd_heights": (c_int, [POINTER(CrowdHeightsArgs), P]),
    "pulse_sizeof_terrain_walkable_args": (c_int, []),
    "pulse_terrain_walkable": (c_int, [POINTER(TerrainWalkableArgs), P]),
    "pulse_sizeof_terrain_valid_args": (c_int, []),
    "pulse_terrain_valid_cells": (c_int, [POINTER(TerrainValidArgs), P]),
    "pulse_sizeof_terrain_sample_args": (c_int, []),
    "pulse_terrain_sample": (c_int, [POINTER(TerrainSampleArgs), P]),
    "pulse_vae_embed": (c_int, [POINTER(VaeEmbedArgs), P]),
    "pulse_vae_embed_prior": (c_int, [POINTER(VaeEmbedPriorArgs), P]),
    "pulse_sizeof_vae_embed_prior_args": (c_int, []),
    "pulse_vae_project": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_float, P]),
    "pulse_vae_kin_loss": (c_int, [POINTER(VaeKinArgs), P]),
    "pulse_vae_head_backward": (c_int, [POINTER(VaeHeadBwdArgs), P]),
    "pulse_sizeof_vae_embed_args": (c_int, []),
    "pulse_sizeof_vae_kin_args": (c_int, []),
    "pulse_sizeof_vae_head_bwd_args": (c_int, []),
    "pulse_mcp_compose": (c_int, [P, c_int64, P, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, P, c_int64, P]),
    "pulse_mcp_head_forward": (c_int, [P, c_int64, c_int32, c_int32, P, c_int64, P]),
    "pulse_mcp_head_backward": (c_int, [P, c_int64, P, c_int64, P, c_int64, c_int32, c_int32, c_int32, P, c_int64, P]),
    "pulse_pd_targets": (c_int, [P, c_int64, c_int32, c_int32, c_float, P, P, P, P, c_int64, P, c_int64, P, c_int64, P, c_int64, P]),
    "pulse_sizeof_gemm_x3p_desc": (c_int, []),
    "pulse_split_planes": (c_int, [P, c_int64, c_int32, c_int32, P, c_int64, c_int32, c_int32, P, P]),
    "pulse_reduce_slabs": (c_int, [P, c_int32, c_int64, c_int64, P, c_float, P]),
    "pulse_colsum_partial": (c_int, [P, c_int32, c_int32, c_int32, c_int32, P, c_int64, P]),
    "pulse_rms_normalize": (c_int, [P, c_int64, P, c_int32, c_int32, P, P, c_float, c_float, c_int32, P, c_int64, c_int32, P, c_int32, P]),
    "pulse_rms_normalize_copy": (c_int, [P, c_int64, P, c_int32, c_int32, P, P, c_float, c_float, P, c_int64, c_int32, P, c_int32, P, c_int64, P]),
    "pulse_rms_normalize_planes": (c_int, [P, c_int64, P, c_int32, c_int32, P, P, c_float, c_float, P, c_int64, c_int32, P, c_int32, P, c_int64, c_int64, P]),
    "pulse_rms_normalize_b16": (c_int, [P, c_int64, P, c_int32, c_int32, P, P, c_float, c_float, P, c_int64, c_int32, P, c_int32, P]),
    "pulse_transpose_to_b16": (c_int, [P, c_int64, c_int32, c_int32, P, c_int64, c_int32, c_int64, c_int64, P]),
    "pulse_colsum_partial_b16": (c_int, [P, c_int32, c_int32, c_int64, c_int32, P, c_int64, P]),
    "pulse_colsum_weighted_b16": (c_int, [P, c_int32, c_int32, c_int64, P, c_int64, c_int32, P, c_int64, P]),
    "pulse_disc_penalty": (c_int, [P, c_int64, c_int32, c_int32, c_float, P, c_int64, P, c_int64, P, c_int32, P]),
    "pulse_disc_reg": (c_int, [P, P, c_int32, POINTER(c_int64), POINTER(c_int64), POINTER(c_float), P, c_int32, P]),
    "pulse_sizeof_b16_transpose": (c_int, []),
    "pulse_weights_to_b16": (c_int, [P, c_int64, P, c_int32, POINTER(B16Transpose), P]),
    "pulse_reduce_grads": (c_int, [P, c_int64, c_int32, POINTER(c_int64), POINTER(c_int64), POINTER(c_int32), POINTER(c_float), POINTER(ctypes.c_void_p),
                                   POINTER(c_int64), P, c_float, P, P, P, c_int32, P]),
    "pulse_disc_reward": (c_int, [P, c_int64, c_int64, c_float, P, c_int64, P]),
    "pulse_disc_head_b16": (c_int, [P, c_int64, c_int32, c_float, P, c_int64, P, c_int64, P, P, P]),
    "pulse_rms_update": (c_int, [P, P, P, P, c_int32, c_int32, c_double, c_double, P]),
    "pulse_policy_sample": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, P, c_int32, c_int32, P, c_int64, P, c_int64, P, c_int64, P, c_int64, P, c_int64, P]),
    "pulse_sizeof_ppo_loss_args": (c_int, []),
    "pulse_ppo_loss": (c_int, [POINTER(PpoLossArgs), P]),
    "pulse_advantage_moments": (c_int, [P, P, c_int64, P, P, c_int32, P]),
    "pulse_advantage_normalize": (c_int, [P, c_int64, P, c_int32, P]),
    "pulse_sqnorm_partial": (c_int, [P, c_int64, P, c_int32, P]),
    "pulse_disc_head": (c_int, [P, c_int64, c_int32, c_float, P, c_int64, P, P]),
    "pulse_adam_step": (c_int, [P, P, P, P, c_int64, c_float, c_float, c_float, c_float, c_float, c_int32, c_float, P, c_int32, P, P]),
    "pulse_adam_step_multi": (c_int, [c_int32, POINTER(ctypes.c_void_p), POINTER(ctypes.c_void_p), POINTER(ctypes.c_void_p), POINTER(ctypes.c_void_p),
                                      POINTER(c_int64), c_float, c_float, c_float, c_float, c_float, c_int32, c_float, P, c_int32, P, P]),
}

_lib = None
_load_error = None


def load():
    """Load (once) and return the ctypes library handle; raise loudly if unavailable."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise _load_error
    try:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} does not exist")
        # PyTorch ships its own libamdhip64; it must be the HIP runtime of the process (the streams and device pointers handed to
        # this library are torch's).  Loading libpulse_hip.so first would pull in the system ROCm runtime instead and every launch
        # would then fail with "no ROCm-capable device is detected".
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        v = lib.pulse_abi_version()
        if v != ABI_VERSION:
            raise OSError(f"ABI version mismatch: library {v}, binding {ABI_VERSION}")
    except (OSError, AttributeError) as exc:
        _load_error = PulseLibraryError(
            "pulse_amd: the HIP extension libpulse_hip.so is required and could not be loaded "
            f"({exc}). There is no CPU fallback. Build it with `python pulse_amd/csrc/build.py`.")
        raise _load_error from exc
    _lib = lib
    return lib


def check(status, what=""):
    if status != 0:
        msg = load().pulse_last_error()
        raise PulseLibraryError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")
