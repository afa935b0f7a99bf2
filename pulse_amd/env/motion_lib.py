"""Reference-motion library resident in HBM (mirrors the query surface of phc/utils/motion_lib_base.py).

What the reference does per env step (humanoid_im.py:708-735, 853-861, 950-964): twice, gather two frames from six flat
tables (gts, grs, lrs, gvs, gavs, dvs; motion_lib_base.py:297-304) for every env, lerp / slerp them, turn the local
rotations into exp-map dof positions and add the per-env offset -- ~60 small launches and twelve scattered gathers.

Here the tables are packed into one record per frame (include/pulse_hip.h section 2b:
[grs | lrs | gts | gvs | gavs | dvs | pad], 480 floats = 1920 B for SMPL) and ``get_motion_state`` is one launch of
``pulse_motion_state`` that reads two contiguous records per query.

Two ways in.  ``from_tables`` takes finished tables (pulse_amd/synthetic.py:synthetic_motion_library) and keeps every clip
resident.  ``from_motion_data`` takes the reference's raw-data dict, key -> {pose_quat_global (F, J, 4), root_trans_offset (F, 3),
fps, [pose_aa, beta]} (what MotionLibBase.load_data reads from its motion file, motion_lib_base.py:129-156), stages every clip on the
device once as fp32, and ``load_motions`` (motion_lib_base.py:179-318) then draws one clip per skeleton slot from ``_sampling_prob``
and builds the records of the drawn clips for each slot's own bone offsets with ``pulse_motion_build`` (csrc/motion_build.hip): heading
randomisation, local rotations, forward kinematics, np.gradient + Gaussian-filtered velocities and dof velocities -- what
MotionLibSMPL.load_motion_with_skeleton (motion_lib_smpl.py:101-174) does clip by clip with poselib in worker processes.  Out of
scope: ``fix_trans_height`` (needs SMPL model files; the reference itself adds 0 when data/smpl is absent), reading pickles or
directories of pickles from disk, ``real_traj`` quest data and the multi-process loader.

A third way in, one step earlier: ``from_smpl_data`` takes raw SMPL pose sequences (axis-angle ``poses`` / ``pose_aa``, ``trans``, ``betas``,
``gender``, ``mocap_framerate``) and converts them on the device in one launch of ``pulse_motion_ingest`` (csrc/motion_ingest.hip) -- what the
reference's scripts/data_process/convert_amass_data.py and convert_amass_isaac.py do with smpl_sim, scipy and poselib -- into the staging
buffers ``load_motions`` reads; ``motion_data()`` hands the converted dict back.

A fourth, for GENERATED motion: ``from_mdm_data`` takes a text-to-motion model's result (per-joint Euler angles in degrees, a root translation) and does
what scripts/data_process/convert_data_mdm.py does -- Euler poses to rotation vectors (``pulse_motion_euler_pose``), the conversion above, then the sign
correction along every clip and the Gaussian smoothing of rotations and root translation (``pulse_motion_smooth``, csrc/motion_smooth.hip);
``from_smpl_data(..., smooth=True)`` applies the last step to raw SMPL clips.

Same names and return keys as MotionLibBase: ``get_motion_state``, ``get_root_pos_smpl``, ``get_motion_length``,
``get_motion_num_steps``, ``sample_motions``, ``sample_time``, ``sample_time_interval``, ``num_motions``,
``get_total_length``; attributes ``_motion_lengths``, ``_motion_fps``, ``_motion_dt``, ``_motion_num_frames``,
``length_starts``, ``_sampling_prob``.
"""
import ctypes
import math

import torch

from .._lib import MotionStateArgs
from .._marshal import Filler, launch, mask_u8


def _round4(n):
    return (n + 3) // 4 * 4


# ---- host-side logic of load_data / load_motions that needs no device (pure functions)
def filter_motion_data(data, min_length=-1, im_eval=False):
    """MotionLibBase.load_data in file mode (motion_lib_base.py:139-149): the keys of the data set in the order the library numbers them.
    ``min_length`` keeps the clips of at least that many frames (and then ignores ``im_eval``, as the reference's if / elif does);
    ``im_eval`` orders them longest first (stable, like ``sorted``)."""
    if min_length != -1:
        return [k for k, v in data.items() if len(v["pose_quat_global"]) >= min_length]
    if im_eval:
        return [k for k, _ in sorted(data.items(), key=lambda entry: len(entry[1]["pose_quat_global"]), reverse=True)]
    return list(data.keys())


def draw_motion_ids(sampling_prob, num_slots, random_sample=True, start_idx=0, generator=None):
    """Which clip each of ``num_slots`` skeleton slots loads (:205-208): a multinomial draw with replacement from ``sampling_prob`` (on the CPU,
    so that a ``torch.Generator`` makes it repeatable), or the clips start_idx, start_idx + 1, ... wrapping around the data set."""
    p = torch.as_tensor(sampling_prob).detach().cpu()
    if random_sample:
        return torch.multinomial(p, num_samples=num_slots, replacement=True, generator=generator)
    return torch.remainder(torch.arange(num_slots) + start_idx, p.numel())


def batch_sampling_prob(sampling_prob, ids):
    """_sampling_batch_prob (:214): the data-set distribution restricted to the loaded clips, renormalised."""
    p = sampling_prob[ids.to(sampling_prob.device)]
    return p / p.sum()


def crop_ranges(num_frames, max_len=-1, generator=None):
    """(start, length) per clip as load_motion_with_skeleton crops (motion_lib_smpl.py:117-122): the whole clip when max_len is -1 or the
    clip is shorter than max_len, otherwise max_len frames from a start drawn uniformly in [0, frames - max_len]."""
    n = torch.as_tensor(num_frames, dtype=torch.int64)
    if max_len == -1:
        return torch.zeros_like(n), n.clone()
    room = (n - max_len).clamp(min=0)
    u = torch.rand(n.shape, dtype=torch.float64, generator=generator)
    start = torch.minimum((u * (room + 1).double()).long(), room)
    return start, torch.where(n < max_len, n, torch.full_like(n, max_len))


def _parse_skeleton_trees(skeleton_trees):
    """(parents list, local_translation (M, J, 3) float32 CPU) from one (parents, (M, J, 3)) pair or a sequence of objects that carry
    ``parent_indices`` and ``local_translation`` (poselib's SkeletonTree does; nothing of poselib is imported)."""
    if isinstance(skeleton_trees, tuple) and len(skeleton_trees) == 2 and not hasattr(skeleton_trees[0], "parent_indices"):
        parents, lt = skeleton_trees
        lt = torch.as_tensor(lt, dtype=torch.float32)
    else:
        parents = skeleton_trees[0].parent_indices
        lt = torch.stack([torch.as_tensor(t.local_translation, dtype=torch.float32) for t in skeleton_trees])
        for t in skeleton_trees:
            if [int(p) for p in t.parent_indices] != [int(p) for p in parents]:
                raise ValueError("skeleton_trees: every slot must have the same parent_indices (body shape changes the bone offsets only)")
    parents = [int(p) for p in parents]
    if lt.dim() != 3 or tuple(lt.shape[1:]) != (len(parents), 3):
        raise ValueError(f"skeleton_trees: local_translation (M, {len(parents)}, 3) expected, got {tuple(lt.shape)}")
    return parents, lt.contiguous()


SMPL_MIN_FRAMES = 10                     # convert_amass_data.py:101: shorter clips are skipped


def _smpl_field(entry, *names):
    """The first of ``names`` the raw SMPL entry carries (both spellings occur: pose_aa / poses, beta / betas), as a tensor."""
    for n in names:
        if n in entry:
            return torch.as_tensor(entry[n])
    raise KeyError(f"a raw SMPL clip needs one of {names}, got {sorted(entry)}")


def plan_smpl_clips(data, bounds=None, mirror=False, min_length=-1, im_eval=False):
    """What ``from_smpl_data`` will build, decided on the host: (clips, dropped keys).  Every clip: key, source (the key of its raw data), raw_frames,
    skip = int(mocap_framerate / 30), frames = len(range(0, raw, skip))[:bound], mirror.  Clips left with fewer than SMPL_MIN_FRAMES frames are
    dropped (convert_amass_data.py:88-102); a mirrored copy follows its original under key + "_1"; then ``filter_motion_data``'s selection
    and order (min_length, im_eval) over the converted lengths."""
    clips, dropped = [], []
    for key, entry in data.items():
        pose, trans = _smpl_field(entry, "pose_aa", "poses"), torch.as_tensor(entry["trans"])
        if pose.dim() != 2 or pose.shape[1] < 72 or tuple(trans.shape) != (pose.shape[0], 3):
            raise ValueError(f"clip {key!r}: pose_aa / poses (F, >= 72) and trans (F, 3) expected, got {tuple(pose.shape)} and {tuple(trans.shape)}")
        _smpl_field(entry, "beta", "betas")
        rate = float(torch.as_tensor(entry["mocap_framerate"]).item()) if "mocap_framerate" in entry else 30.0
        if not math.isfinite(rate) or rate < 30:
            raise ValueError(f"clip {key!r}: mocap_framerate {rate} is not a finite rate of at least 30 (the decimation step int(framerate / 30) would be 0)")
        skip = int(rate / 30)
        n = -(-pose.shape[0] // skip)
        bound = int((bounds or {}).get(key, 0))
        if bound < 0:
            raise ValueError(f"clip {key!r}: bound {bound} is negative")
        n = min(n, bound) if bound else n
        if n < SMPL_MIN_FRAMES:
            dropped.append(key)
            continue
        for m in range(2 if mirror else 1):
            clips.append({"key": f"{key}_1" if m else key, "source": key, "raw_frames": int(pose.shape[0]), "skip": skip, "frames": n, "mirror": bool(m)})
    keys = [c["key"] for c in clips]
    if len(set(keys)) != len(keys):
        raise ValueError("from_smpl_data: a mirrored copy's key (key + '_1') collides with another clip's key")
    order = filter_motion_data({c["key"]: {"pose_quat_global": range(c["frames"])} for c in clips}, min_length, im_eval)
    by_key = {c["key"]: c for c in clips}
    return [by_key[k] for k in order], dropped


def plan_mdm_clips(result, min_length=-1, im_eval=False):
    """What ``from_mdm_data`` will build, decided on the host: (clips, dropped keys, thetas, roots).  ``result``: {thetas: B sequences of (F, 24, 3) or
    (F, 72), root_translation: B sequences of (F, 3)} (convert_data_mdm.py:48-51).  Sequence i becomes key str(i), 30 fps, skip 1, never mirrored;
    ``plan_smpl_clips``' ten-frame minimum and selection apply.  thetas / roots: key -> float32 CPU tensor (F, 72) / (F, 3)."""
    if not isinstance(result, dict) or "thetas" not in result or "root_translation" not in result:
        raise KeyError("from_mdm_data: result needs 'thetas' and 'root_translation' (the json_file layout of the generator's output)")
    if len(result["thetas"]) != len(result["root_translation"]):
        raise ValueError(f"from_mdm_data: {len(result['thetas'])} thetas sequences but {len(result['root_translation'])} root_translation sequences")
    thetas, roots, data = {}, {}, {}
    for i in range(len(result["thetas"])):
        th, tr = torch.as_tensor(result["thetas"][i]).to(torch.float32), torch.as_tensor(result["root_translation"][i]).to(torch.float32)
        if not ((th.dim() == 3 and tuple(th.shape[1:]) == (24, 3)) or (th.dim() == 2 and th.shape[1] == 72)) or tuple(tr.shape) != (th.shape[0], 3):
            raise ValueError(f"clip {str(i)!r}: thetas (F, 24, 3) or (F, 72) and root_translation (F, 3) expected, got {tuple(th.shape)} and {tuple(tr.shape)}")
        thetas[str(i)], roots[str(i)] = th.reshape(th.shape[0], 72), tr
        data[str(i)] = {"pose_aa": thetas[str(i)], "trans": tr, "beta": torch.zeros(10)}
    clips, dropped = plan_smpl_clips(data, None, False, min_length, im_eval)
    return clips, dropped, thetas, roots


class MotionLib:
    FIELDS = ("gts", "grs", "lrs", "gvs", "gavs", "dvs")

    @staticmethod
    def record_layout(num_bodies):
        """(offsets, frame_stride) of the packed frame record of a ``num_bodies`` humanoid, in floats.  Quaternion fields first, so that they
        sit on 16-B boundaries for any body count: [grs | lrs | gts | gvs | gavs | dvs | pad to a multiple of 4]."""
        j = num_bodies
        widths = {"grs": j * 4, "lrs": j * 4, "gts": j * 3, "gvs": j * 3, "gavs": j * 3, "dvs": (j - 1) * 3}
        offsets, off = {}, 0
        for k, w in widths.items():
            offsets[k] = off
            off += w
        return offsets, _round4(off), widths

    def __init__(self, tables, device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("MotionLib lives in HBM (pulse_amd has no CPU path)")
        self._device = dev
        gts = tables["gts"]
        total, j = gts.shape[0], gts.shape[1]
        self.num_bodies = j
        self.num_dof = (j - 1) * 3
        self.offsets, self.frame_stride, widths = self.record_layout(j)
        order = tuple(widths)
        frames = torch.zeros(total, self.frame_stride, dtype=torch.float32, device=dev)
        for k in order:
            t = tables[k]
            if t.shape[0] != total or t.dtype != torch.float32:
                raise ValueError(f"table {k}: expected ({total}, ...) float32")
            frames[:, self.offsets[k]:self.offsets[k] + widths[k]] = t.reshape(total, -1).to(dev)
        self.frames = frames
        self._motion_lengths = tables["motion_lengths"].to(dev, torch.float32).contiguous()
        self._motion_fps = tables["motion_fps"].to(dev, torch.float32).contiguous()
        self._motion_dt = tables["motion_dt"].to(dev, torch.float32).contiguous()
        self._motion_num_frames = tables["motion_num_frames"].to(dev, torch.int64).contiguous()
        lengths_shifted = self._motion_num_frames.roll(1)                      # motion_lib_base.py:311-314
        lengths_shifted[0] = 0
        self.length_starts = lengths_shifted.cumsum(0).contiguous()
        self._num_motions = self._motion_lengths.shape[0]
        self.motion_ids = torch.arange(self._num_motions, dtype=torch.long, device=dev)
        self._sampling_prob = torch.ones(self._num_motions, device=dev) / self._num_motions      # :205, uniform until re-weighted
        self._sampling_batch_prob = self._sampling_prob
        self._lengths_host = None
        # PMCP bookkeeping over the data set's clips (motion_lib_base.py:196-206): here every clip of the tables is resident, so the
        # "unique motions" of the data set and the loaded batch coincide
        self._num_unique_motions = self._num_motions
        keys = tables.get("motion_data_keys")
        self._motion_data_keys = list(keys) if keys is not None else [str(i) for i in range(self._num_motions)]
        self._termination_history = torch.zeros(self._num_unique_motions, device=dev)
        # optional per-motion body-shape rows (motion_lib_base.py:289, 294, 515-516: _motion_bodies (M, 17), _motion_limb_weights (M, 10)); the
        # AMP frames of reference motion carry them under has_shape_obs_disc / has_weight_obs_disc (humanoid_amp.py:243-250, 548-555)
        self.motion_bodies = self._shape_rows(tables, "motion_bodies", 17)
        self.motion_limb_weights = self._shape_rows(tables, "motion_limb_weights", 10)
        self._src = None                                   # staged raw clips: only a library built by from_motion_data reloads
        self._smpl = None
        self._generation = 0

    def _shape_rows(self, tables, key, width):
        t = tables.get(key)
        if t is None:
            return None
        if tuple(t.shape) != (self._num_motions, width) or t.dtype != torch.float32:
            raise ValueError(f"table {key}: expected ({self._num_motions}, {width}) float32")
        return t.to(self._device).contiguous()

    @classmethod
    def from_tables(cls, tables, device="cuda:0"):
        return cls(tables, device)

    @classmethod
    def from_motion_data(cls, data, skeleton_trees, gender_betas=None, limb_weights=None, device="cuda:0", min_length=-1, im_eval=False,
                         generator=None):
        """A library over the reference's raw-data dict (module docstring).  ``skeleton_trees``: one tree per resident slot (env), or one
        (parents, local_translation (M, J, 3)) pair.  ``generator``: the CPU torch.Generator every draw of this library comes from (which
        clips load, heading angles, crop starts).  Ends with a first ``load_motions``."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("MotionLib lives in HBM (pulse_amd has no CPU path)")
        self = cls.__new__(cls)
        self._device = dev
        keys = filter_motion_data(data, min_length, im_eval)
        if not keys:
            raise ValueError("from_motion_data: no clip left" + (f" with at least {min_length} frames" if min_length != -1 else ""))
        self._motion_data_keys = keys
        self._num_unique_motions = len(keys)
        rot = [torch.as_tensor(data[k]["pose_quat_global"]) for k in keys]
        j = rot[0].shape[1]
        for k, r in zip(keys, rot):
            t = torch.as_tensor(data[k]["root_trans_offset"])
            if r.dim() != 3 or tuple(r.shape[1:]) != (j, 4) or tuple(t.shape) != (r.shape[0], 3):
                raise ValueError(f"clip {k!r}: pose_quat_global (F, {j}, 4) and root_trans_offset (F, 3) expected, got {tuple(r.shape)} and {tuple(t.shape)}")
            if r.shape[0] < 2:
                raise ValueError(f"clip {k!r} has {r.shape[0]} frame(s): at least 2 are needed (np.gradient raises below 2)")
        frames = torch.tensor([r.shape[0] for r in rot], dtype=torch.int64)
        src = {
            "rot": torch.cat([r.to(torch.float32) for r in rot]).contiguous().to(dev),
            "trans": torch.cat([torch.as_tensor(data[k]["root_trans_offset"]).to(torch.float32) for k in keys]).contiguous().to(dev),
            "start": torch.cumsum(frames, 0) - frames, "frames": frames,
            "fps": torch.tensor([float(data[k].get("fps", 30)) for k in keys], dtype=torch.float64),             # curr_file.get("fps", 30), motion_lib_smpl.py:150
            "has_beta": torch.tensor(["beta" in data[k] for k in keys]),
        }
        return self._finish_staged(src, j, im_eval, generator, skeleton_trees, gender_betas, limb_weights)

    def _finish_staged(self, src, j, im_eval, generator, skeleton_trees, gender_betas, limb_weights):
        """The rest of a library over staged clips (``_src``), however they were staged: layout, sampling weights, a first ``load_motions``."""
        dev = self._device
        self._src = src
        self.num_bodies, self.num_dof = j, (j - 1) * 3
        self.offsets, self.frame_stride, _ = self.record_layout(j)
        self._im_eval, self._generator = bool(im_eval), generator
        self._sampling_prob = torch.ones(self._num_unique_motions, device=dev) / self._num_unique_motions       # setup_constants, :162-168
        self._termination_history = torch.zeros(self._num_unique_motions, device=dev)
        self._curr_motion_ids = None
        self._generation = 0
        self._last_load = {"skeleton_trees": None, "gender_betas": None, "limb_weights": None}
        self.load_motions(skeleton_trees, gender_betas, limb_weights)
        return self

    @staticmethod
    def _smooth_sigmas(smooth, upright_start, what):
        """``smooth`` of from_smpl_data / from_mdm_data -> None or (sigma_rot, sigma_trans), refused by name where it cannot run."""
        if smooth is None or smooth is False:
            return None
        if smooth is True:
            smooth = {}
        if not isinstance(smooth, dict) or set(smooth) - {"sigma_rot", "sigma_trans"}:
            raise ValueError(f"{what}: smooth is None, True or a dict with sigma_rot / sigma_trans, got {smooth!r}")
        if not upright_start:
            raise ValueError(f"{what}: smooth requires upright_start=True: convert_data_mdm.py filters in that branch only (:125-141), its other branch does not run")
        from .. import kernels
        sigmas = (float(smooth.get("sigma_rot", 2.0)), float(smooth.get("sigma_trans", 3.0)))
        for s in sigmas:
            if s != 0.0:
                kernels.gaussian_taps(s)                   # a negative sigma or more than 12 taps a side: refused here, before anything is staged
        return sigmas

    @classmethod
    def from_smpl_data(cls, data, skeleton_trees, *, upright_start=True, mirror=False, bounds=None, root_offset=None, gender_betas=None,
                       limb_weights=None, device="cuda:0", min_length=-1, im_eval=False, generator=None, smooth=None):
        """A library over RAW SMPL pose sequences, as motion data sets ship them: ``data`` maps key -> {pose_aa | poses (F, >= 72) axis-angle in SMPL
        joint order, trans (F, 3), beta | betas, gender, [mocap_framerate]}, numpy or torch, fp32 or fp64.  What the reference's
        scripts/data_process/convert_amass_data.py:88-141 and convert_amass_isaac.py:85-137 do on the CPU first happens here in ONE launch of
        ``pulse_motion_ingest`` (csrc/motion_ingest.hip) over every frame of every clip, straight into the staging buffers ``load_motions`` reads;
        everything after that is ``from_motion_data``'s (the remaining arguments are the same).

          * a clip is decimated by skip = int(mocap_framerate / 30) and then labelled 30 fps WHATEVER framerate / skip is -- 100 Hz data becomes
            33.3 fps data called 30, as in the reference;
          * a clip WITHOUT mocap_framerate is taken as 30 Hz data and kept whole, as convert_amass_isaac.py takes its input; convert_amass_data.py:81-82
            skips such a clip instead;
          * ``bounds``: key -> number of decimated frames to keep (the occlusion file's ``idxes[0]``); a clip left with fewer than 10 frames is
            dropped (convert_amass_data.py:101) with a warning that names it;
          * ``mirror``: every clip is followed by its left-right mirrored copy under ``key + "_1"`` -- the spelling convert_amass_isaac.py:118 has
            commented out; its live line (:119) reuses the key, so that the copy overwrites the original;
          * ``root_offset``: three floats added to ``trans`` (default: local_translation[0] of skeleton slot 0, :114);
          * ``upright_start=False`` leaves the (0.5, 0.5, 0.5, 0.5)^-1 factor out; the reference has no runnable counterpart (both scripts
            hard-code True);
          * ``smooth``: None (default: nothing below happens, the staged bits are what they were), True or {"sigma_rot": 2, "sigma_trans": 3}:
            what scripts/data_process/convert_data_mdm.py:128-141 does to generated motion after the conversion, in the three launches of
            ``pulse_motion_smooth`` (csrc/motion_smooth.hip) -- quat_correct per body along every clip, gaussian_filter1d(sigma_rot,
            mode="nearest") on the global quaternions and renormalisation, gaussian_filter1d(sigma_trans) on root_trans_offset.  A sigma of 0
            leaves that filter out.  ``motion_data()`` then hands back the filtered pose_quat_global / root_trans_offset and pose_quat = the
            local rotations of the clip's OWN filtered globals -- for a mirrored clip too, where the unsmoothed path keeps the unmirrored
            clip's pose_quat; pose_aa and trans_orig stay unfiltered (:146-150).  Needs ``upright_start=True``.
        The humanoid is SMPL (24 bodies): SMPL-X / SMPL-H sources, reading .npz trees from disk and fix_trans_height are out of scope."""
        import warnings
        from .. import kernels, synthetic
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("MotionLib lives in HBM (pulse_amd has no CPU path)")
        sigmas = cls._smooth_sigmas(smooth, upright_start, "from_smpl_data")
        parents, lt = _parse_skeleton_trees(skeleton_trees)
        clips, dropped = plan_smpl_clips(data, bounds, mirror, min_length, im_eval)
        if dropped:
            warnings.warn(f"from_smpl_data: dropped {len(dropped)} clip(s) left with fewer than {SMPL_MIN_FRAMES} frames: {', '.join(map(str, dropped))}")
        if not clips:
            raise ValueError("from_smpl_data: no clip left" + (f" with at least {min_length} frames" if min_length != -1 else ""))
        joint_map = synthetic.smpl_joint_map()
        if len(parents) != len(joint_map):
            raise ValueError(f"from_smpl_data: the skeleton trees have {len(parents)} bodies, the SMPL humanoid {len(joint_map)}")
        self = cls.__new__(cls)
        self._device = dev
        self._motion_data_keys = [c["key"] for c in clips]
        self._num_unique_motions = len(clips)
        # the raw arrays, staged once as fp32: one copy per source clip (a mirrored copy reads its original's rows)
        sources, src_start, at = {}, [], 0
        for c in clips:
            if c["source"] not in sources:
                sources[c["source"]] = at
                at += c["raw_frames"]
            src_start.append(sources[c["source"]])
        pose = torch.cat([_smpl_field(data[k], "pose_aa", "poses")[:, :72].to(torch.float32) for k in sources]).contiguous().to(dev)
        trans = torch.cat([torch.as_tensor(data[k]["trans"]).to(torch.float32) for k in sources]).contiguous().to(dev)
        # beta: zeros of the input's length (a (1, n) row counts as n, convert_amass_isaac.py:62-64, 96)
        beta_len = [int(_smpl_field(data[c["source"]], "beta", "betas").shape[-1]) for c in clips]
        off = lt[0, 0].tolist() if root_offset is None else [float(v) for v in root_offset]
        return self._ingest_staged(pose, trans, clips, src_start, beta_len, parents, upright_start, off, sigmas, im_eval, generator, skeleton_trees,
                                   gender_betas, limb_weights)

    def _ingest_staged(self, pose, trans, clips, src_start, beta_len, parents, upright_start, root_offset, sigmas, im_eval, generator, skeleton_trees,
                       gender_betas, limb_weights):
        """Staged SMPL pose rows -> the staging buffers of ``load_motions``: the ingest launch, the smoothing launches when ``sigmas`` is given
        (ingest then writes scratch buffers: the filters read their neighbours' unfiltered values), ``_finish_staged``."""
        from .. import kernels, synthetic
        dev = self._device
        frames = torch.tensor([c["frames"] for c in clips], dtype=torch.int64)
        total, j = int(frames.sum()), len(parents)
        src = {"rot": torch.empty(total, j, 4, dtype=torch.float32, device=dev), "trans": torch.empty(total, 3, dtype=torch.float32, device=dev),
               "start": torch.cumsum(frames, 0) - frames, "frames": frames, "fps": torch.full((len(clips),), 30.0, dtype=torch.float64),
               "has_beta": torch.ones(len(clips), dtype=torch.bool)}              # the converted file always carries a (zeroed) beta
        self._smpl = {"pose_quat": torch.empty(total, j, 4, dtype=torch.float32, device=dev), "pose_aa": torch.empty(total, 72, dtype=torch.float32, device=dev),
                      "trans_orig": torch.empty(total, 3, dtype=torch.float32, device=dev), "beta_len": beta_len}
        rot, rto = (src["rot"], src["trans"]) if sigmas is None else (torch.empty_like(src["rot"]), torch.empty_like(src["trans"]))
        kernels.motion_ingest(rot, rto, src_pose=pose, src_trans=trans, clip_src_start=torch.tensor(src_start, dtype=torch.int64),
                              clip_skip=torch.tensor([c["skip"] for c in clips], dtype=torch.int64), clip_frames=frames, parents=parents,
                              joint_map=synthetic.smpl_joint_map(), mirror_map=synthetic.mirror_body_map(),
                              clip_mirror=torch.tensor([c["mirror"] for c in clips]), upright_start=upright_start, root_offset=root_offset,
                              out_pose_quat=self._smpl["pose_quat"] if sigmas is None else None, out_pose_aa=self._smpl["pose_aa"],
                              out_trans_orig=self._smpl["trans_orig"])
        if sigmas is not None:
            kernels.motion_smooth(src["rot"], src["trans"], in_rot=rot, in_trans=rto, clip_frames=frames, parents=parents, sigma_rot=sigmas[0],
                                  sigma_trans=sigmas[1], out_pose_quat=self._smpl["pose_quat"])
        return self._finish_staged(src, j, im_eval, generator, skeleton_trees, gender_betas, limb_weights)

    @classmethod
    def from_mdm_data(cls, result, skeleton_trees, *, floor_height=0.92, smooth=True, root_offset=None, gender_betas=None, limb_weights=None,
                      device="cuda:0", min_length=-1, im_eval=False, generator=None):
        """A library over GENERATED motion, as a text-to-motion model (MDM) hands it back: ``result`` is the ``res_data["json_file"]`` layout
        scripts/data_process/convert_data_mdm.py:48-51 reads -- ``thetas``: B sequences of (F, 24, 3) or (F, 72) per-joint Euler 'XYZ' angles in
        DEGREES, SMPL joint order; ``root_translation``: B sequences of (F, 3), y up.  What the script does on the CPU happens here on the device:
        one launch of ``pulse_motion_euler_pose`` (:48-61: angles -> rotation vectors, the root turned by +90 degrees about x, the translation
        turned with it and its first frame set on ``floor_height``), the ``pulse_motion_ingest`` launch (:102-126) and, with ``smooth`` (True or
        {"sigma_rot": 2, "sigma_trans": 3}; None leaves it out), the three launches of ``pulse_motion_smooth`` (:128-141, see ``from_smpl_data``).
        Keys are "0", "1", ...; 30 fps, no decimation; beta is zeros(10) and gender "neutral" (:110); a sequence of fewer than 10 frames is
        dropped with a warning that names it.  The remaining arguments are ``from_smpl_data``'s.  The transport to the model (the reference's
        scripts/mdm_test.py) is the caller's."""
        import warnings
        from .. import kernels, synthetic
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("MotionLib lives in HBM (pulse_amd has no CPU path)")
        sigmas = cls._smooth_sigmas(smooth, True, "from_mdm_data")
        parents, lt = _parse_skeleton_trees(skeleton_trees)
        if len(parents) != len(synthetic.smpl_joint_map()):
            raise ValueError(f"from_mdm_data: the skeleton trees have {len(parents)} bodies, the SMPL humanoid {len(synthetic.smpl_joint_map())}")
        clips, dropped, thetas, roots = plan_mdm_clips(result, min_length, im_eval)
        if dropped:
            warnings.warn(f"from_mdm_data: dropped {len(dropped)} clip(s) left with fewer than {SMPL_MIN_FRAMES} frames: {', '.join(map(str, dropped))}")
        if not clips:
            raise ValueError("from_mdm_data: no clip left" + (f" with at least {min_length} frames" if min_length != -1 else ""))
        self = cls.__new__(cls)
        self._device = dev
        self._motion_data_keys = [c["key"] for c in clips]
        self._num_unique_motions = len(clips)
        frames = torch.tensor([c["frames"] for c in clips], dtype=torch.int64)
        theta = torch.cat([thetas[c["key"]] for c in clips]).contiguous().to(dev)
        raw = torch.cat([roots[c["key"]] for c in clips]).contiguous().to(dev)
        pose, trans = torch.empty_like(theta), torch.empty_like(raw)
        kernels.motion_euler_pose(pose, trans, src_theta=theta, src_trans=raw, clip_frames=frames, floor_height=floor_height)
        off = lt[0, 0].tolist() if root_offset is None else [float(v) for v in root_offset]
        src_start = (torch.cumsum(frames, 0) - frames).tolist()
        return self._ingest_staged(pose, trans, clips, src_start, [10] * len(clips), parents, True, off, sigmas, im_eval, generator, skeleton_trees,
                                   gender_betas, limb_weights)

    def motion_data(self):
        """The converted motion data of a library built by ``from_smpl_data`` or ``from_mdm_data``, in the layout the reference's scripts dump (convert_amass_isaac.py:129-138)
        as CPU numpy arrays: key -> {pose_quat_global, pose_quat, trans_orig, root_trans_offset, beta (zeros of the input's length), gender "neutral",
        pose_aa, fps}.  A mirrored clip carries the unmirrored pose_quat / pose_aa / trans_orig, as the reference leaves them.
        ``from_motion_data(lib.motion_data(), ...)`` stages the same bits."""
        import numpy as np
        if self._src is None or getattr(self, "_smpl", None) is None:
            raise ValueError("motion_data: only a library built by from_smpl_data holds converted motion data")
        host = {k: v.cpu().numpy() for k, v in (("rot", self._src["rot"]), ("trans", self._src["trans"]), ("pose_quat", self._smpl["pose_quat"]),
                                                 ("pose_aa", self._smpl["pose_aa"]), ("trans_orig", self._smpl["trans_orig"]))}
        out = {}
        for i, key in enumerate(self._motion_data_keys):
            s = slice(int(self._src["start"][i]), int(self._src["start"][i]) + int(self._src["frames"][i]))
            out[key] = {"pose_quat_global": host["rot"][s].copy(), "pose_quat": host["pose_quat"][s].copy(), "trans_orig": host["trans_orig"][s].copy(),
                        "root_trans_offset": host["trans"][s].copy(), "beta": np.zeros(self._smpl["beta_len"][i]), "gender": "neutral",
                        "pose_aa": host["pose_aa"][s].copy(), "fps": 30}
        return out

    def eval_twin(self):
        """The evaluation library of this one (humanoid_im.py:336-339: the same motion file under ``im_eval``): the same clips numbered longest
        first (stable, as filter_motion_data orders them), no heading draw, its own sampling weights and termination history.  The staged
        device buffers are shared, only the per-clip tables are reordered; nothing is resident until its first ``load_motions``.  A library
        built from finished tables cannot reload and is its own twin."""
        if self._src is None:
            return self
        src = self._src
        order = sorted(range(self._num_unique_motions), key=lambda i: int(src["frames"][i]), reverse=True)
        idx = torch.tensor(order, dtype=torch.int64)
        twin = type(self).__new__(type(self))
        twin._device, twin.num_bodies, twin.num_dof = self._device, self.num_bodies, self.num_dof
        twin.offsets, twin.frame_stride = self.offsets, self.frame_stride
        twin._motion_data_keys = [self._motion_data_keys[i] for i in order]
        twin._num_unique_motions = self._num_unique_motions
        twin._src = {"rot": src["rot"], "trans": src["trans"], "start": src["start"][idx], "frames": src["frames"][idx], "fps": src["fps"][idx],
                     "has_beta": src["has_beta"][idx]}
        twin._im_eval, twin._generator = True, self._generator
        twin._sampling_prob = torch.ones(twin._num_unique_motions, device=self._device) / twin._num_unique_motions
        twin._termination_history = torch.zeros(twin._num_unique_motions, device=self._device)
        twin._curr_motion_ids, twin._generation, twin._lengths_host = None, 0, None
        twin._last_load = dict(self._last_load)
        twin._num_motions = self._num_motions
        return twin

    def release(self):
        """Drop the resident records of a library that reloads (the evaluation library between two sweeps): the next ``load_motions`` builds
        them again.  A library built from finished tables has nothing else and keeps them."""
        if self._src is not None:
            self.frames = None

    @property
    def reloads(self):
        """True for a library built from raw data: ``load_motions`` re-draws which clips are resident and rebuilds the records."""
        return self._src is not None

    # ---- table views (reference attribute names), strided views into the packed records
    def _field(self, k, inner):
        j = self.num_bodies if k != "dvs" else self.num_bodies - 1
        return self.frames[:, self.offsets[k]:self.offsets[k] + j * inner].view(self.frames.shape[0], j, inner)

    gts = property(lambda self: self._field("gts", 3))
    grs = property(lambda self: self._field("grs", 4))
    lrs = property(lambda self: self._field("lrs", 4))
    gvs = property(lambda self: self._field("gvs", 3))
    gavs = property(lambda self: self._field("gavs", 3))
    dvs = property(lambda self: self._field("dvs", 3))

    def tables(self):
        """The library's tables in the reference's layout (motion_lib_base.py:287-316), copied to the CPU: what ``from_tables`` takes."""
        c = lambda x: x.detach().cpu().contiguous()
        out = {k: c(getattr(self, k)) for k in self.FIELDS}
        out.update({"motion_lengths": c(self._motion_lengths), "motion_fps": c(self._motion_fps), "motion_dt": c(self._motion_dt),
                    "motion_num_frames": c(self._motion_num_frames), "length_starts": c(self.length_starts)})
        return out

    # ---- bookkeeping queries (motion_lib_base.py:325-432)
    def num_motions(self):
        return self._num_motions

    def get_total_length(self):
        if self._lengths_host is None:
            self._lengths_host = float(self._motion_lengths.sum().item())
        return self._lengths_host

    def get_motion_length(self, motion_ids=None):
        return self._motion_lengths if motion_ids is None else self._motion_lengths[motion_ids]

    def get_motion_num_steps(self, motion_ids=None):
        if motion_ids is None:
            return (self._motion_num_frames * 30 / self._motion_fps).int()
        return (self._motion_num_frames[motion_ids] * 30 / self._motion_fps).int()

    # ---- PMCP sampling weights (motion_lib_base.py:348-393; IMAmpAgent.update_training_data, im_amp.py:126-132).  In the reference
    # _sampling_prob steers which clips load_motions makes resident (:212-222) and the batch distribution follows from it; with every
    # clip resident, load_motions here only refreshes the batch distribution from the weights.
    def update_hard_sampling_weight(self, failed_keys):
        """auto_pmcp: train only on the sequences that failed evaluation (:348-360)."""
        if len(failed_keys) > 0:
            indexes = [self._motion_data_keys.index(k) for k in failed_keys]
            self._sampling_prob[:] = 0
            self._sampling_prob[indexes] = 1 / len(indexes)
        else:
            self._sampling_prob = torch.ones(self._num_unique_motions, device=self._device) / self._num_unique_motions

    def update_soft_sampling_weight(self, failed_keys):
        """auto_pmcp_soft: sampling weight proportional to how often a sequence failed evaluation (:362-376)."""
        if len(failed_keys) > 0:
            indexes = [self._motion_data_keys.index(k) for k in failed_keys]
            self._termination_history[indexes] += 1
            self.update_sampling_prob(self._termination_history)
        else:
            self._sampling_prob = torch.ones(self._num_unique_motions, device=self._device) / self._num_unique_motions

    def update_sampling_prob(self, termination_history):
        """:378-384."""
        termination_history = torch.as_tensor(termination_history, dtype=torch.float32, device=self._device)
        if len(termination_history) == len(self._termination_history) and termination_history.sum() > 0:
            self._sampling_prob[:] = termination_history / termination_history.sum()
            self._termination_history = termination_history
            return True
        return False

    def load_motions(self, skeleton_trees=None, gender_betas=None, limb_weights=None, random_sample=True, start_idx=0, max_len=-1):
        """MotionLibBase.load_motions (:179-318).  A library built from tables keeps every clip resident: what survives there is the batch
        distribution, the data-set distribution restricted to the loaded clips and renormalised (:214).  A library built from raw data
        (``from_motion_data``) draws one clip per skeleton slot and rebuilds the records for the slot's own skeleton on the device;
        arguments left None reuse the ones last given."""
        if self._src is None:
            if skeleton_trees is not None or gender_betas is not None or limb_weights is not None or not random_sample or start_idx != 0 or max_len != -1:
                raise ValueError("load_motions: this library was built from finished tables, every clip stays resident (from_motion_data builds one that reloads)")
            self._sampling_batch_prob = self._sampling_prob / self._sampling_prob.sum()
            return
        from .. import kernels
        dev, src, last = self._device, self._src, self._last_load
        for name, value in (("skeleton_trees", skeleton_trees), ("gender_betas", gender_betas), ("limb_weights", limb_weights)):
            if value is not None:
                last[name] = value
        if last["skeleton_trees"] is None:
            raise ValueError("load_motions: skeleton_trees are needed once")
        parents, lt = _parse_skeleton_trees(last["skeleton_trees"])
        m = lt.shape[0]
        if len(parents) != self.num_bodies:
            raise ValueError(f"skeleton_trees have {len(parents)} bodies, the motion data {self.num_bodies}")
        ids = draw_motion_ids(self._sampling_prob, m, random_sample, start_idx, self._generator)
        self._curr_motion_ids = ids.to(dev)
        self.curr_motion_keys = [self._motion_data_keys[i] for i in ids.tolist()]
        self._sampling_batch_prob = batch_sampling_prob(self._sampling_prob, self._curr_motion_ids)
        crop_start, num_frames = crop_ranges(src["frames"][ids], max_len, self._generator)
        fps = src["fps"][ids]
        dt = 1.0 / fps                                                                                    # python doubles in the reference, rounded once (:287-292)
        self._motion_fps, self._motion_dt = fps.float().to(dev), dt.float().to(dev)
        self._motion_lengths = (dt * (num_frames - 1).double()).float().to(dev)                           # curr_len, :263
        self._motion_num_frames = num_frames.to(dev)
        out_start = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(num_frames, 0)])
        self.length_starts = out_start[:-1].to(dev).contiguous()                                          # :311-314
        self._num_motions = m
        self.motion_ids = torch.arange(m, dtype=torch.long, device=dev)
        self._lengths_host = None
        has_beta = src["has_beta"][ids]
        betas = torch.zeros(m, 17) if last["gender_betas"] is None else torch.as_tensor(last["gender_betas"], dtype=torch.float32).reshape(m, 17).cpu()
        self.motion_bodies = torch.where(has_beta[:, None], betas, torch.zeros(m, 17)).to(dev).contiguous()      # :266-271
        lw = last["limb_weights"]
        self.motion_limb_weights = None if lw is None else torch.as_tensor(lw, dtype=torch.float32).reshape(m, -1).to(dev).contiguous()   # :294
        heading = None
        if not self._im_eval:                                                                              # motion_lib_smpl.py:131-140
            heading = (math.pi * (2.0 * torch.rand(m, dtype=torch.float64, generator=self._generator) - 1.0)).float().to(dev)
        self.motion_heading = heading
        total = int(out_start[-1])
        frames = torch.empty(total, self.frame_stride, dtype=torch.float32, device=dev)                  # every column is written by the kernels
        kernels.motion_build(frames, self.offsets, src_rot=src["rot"], src_trans=src["trans"], clip_src_start=src["start"][ids].to(dev),
                             clip_crop_start=crop_start.to(dev) if max_len != -1 else None, clip_out_start=out_start.to(dev),
                             clip_frames=num_frames.contiguous(), clip_dt=self._motion_dt, local_translation=lt.to(dev), parents=parents,
                             clip_heading=heading)
        self.frames = frames
        self._generation += 1

    def sample_motions(self, n, generator=None):
        return torch.multinomial(self._sampling_batch_prob, num_samples=n, replacement=True, generator=generator).to(self._device)

    def sample_time(self, motion_ids, truncate_time=None, generator=None):
        phase = torch.rand(motion_ids.shape, device=self._device, generator=generator)
        motion_len = self._motion_lengths[motion_ids]
        if truncate_time is not None:
            assert truncate_time >= 0.0
            motion_len = motion_len - truncate_time
        return phase * motion_len

    def sample_time_interval(self, motion_ids, truncate_time=None, generator=None):
        phase = torch.rand(motion_ids.shape, device=self._device, generator=generator)
        motion_len = self._motion_lengths[motion_ids]
        if truncate_time is not None:
            assert truncate_time >= 0.0
            motion_len = motion_len - truncate_time
        curr_fps = 1 / 30
        return ((phase * motion_len) / curr_fps).long() * curr_fps

    # ---- the hot query
    def launch_signature(self):
        """Identity of the device tables a cached launch points at (ops._launch_sig)."""
        return (id(self), self.frames.data_ptr(), tuple(self.frames.shape), self._motion_lengths.data_ptr(), self._motion_dt.data_ptr(),
                self._motion_num_frames.data_ptr(), self.length_starts.data_ptr(), self._num_motions, self._generation)

    def fill_tables(self, t):
        """Fill a pulse_motion_tables struct (by reference) with this library's device pointers."""
        t.frames, t.frame_stride, t.total_frames, t.num_bodies = self.frames.data_ptr(), self.frame_stride, self.frames.shape[0], self.num_bodies
        o = self.offsets
        t.off_gts, t.off_grs, t.off_lrs, t.off_gvs, t.off_gavs, t.off_dvs = o["gts"], o["grs"], o["lrs"], o["gvs"], o["gavs"], o["dvs"]
        t.motion_lengths, t.motion_dt = self._motion_lengths.data_ptr(), self._motion_dt.data_ptr()
        t.motion_num_frames, t.length_starts, t.num_motions = self._motion_num_frames.data_ptr(), self.length_starts.data_ptr(), self._num_motions

    def query(self, motion_ids, motion_times=None, offset=None, *, progress=None, step_shift=0, dt=0.0, start_times=None,
              start_offsets=None, time_steps=1, traj_dt=0.0, out=None, root_only=False, with_frames=False, with_records=False,
              reset=None, fields=None):
        """One launch.  Times either given (``motion_times``) or built in-kernel from the episode clock
        ((progress + step_shift) * dt + start_times + start_offsets).  ``out``: dict of preallocated outputs to reuse."""
        dev = self._device
        P = Filler(not_gpu=TypeError)                      # (this method answers a tensor of the wrong kind, device or dtype with TypeError)
        f32 = torch.float32
        ne = motion_ids.numel()                            # per-env arrays
        n = ne if motion_times is not None else ne * int(time_steps)
        j, nd = self.num_bodies, self.num_dof
        a = MotionStateArgs()
        self.fill_tables(a.tab)
        a.n, a.motion_ids = n, P(motion_ids, "motion_ids", torch.int64)
        if reset is not None:
            # reset mode (include/pulse_hip.h 2b): masked envs get a new start time and their reference state in one launch
            a.reset_mask, a.step_shift, a.dt = P(mask_u8(reset["mask"]), "reset.mask", torch.uint8), int(step_shift), float(dt)
            a.reset_phase = P(reset.get("phase"), "reset.phase", f32, (ne,))
            a.reset_time_interval = int(bool(reset.get("time_interval", False)))
            for field, key, dt_ in (("reset_start_times", "start_times", torch.float32), ("reset_progress", "progress", torch.int64),
                                    ("reset_clear0", "clear0", torch.int64), ("reset_clear1", "clear1", torch.int64),
                                    ("reset_clear2", "clear2", torch.int64), ("reset_start_offsets", "zero_start_offsets", torch.float32),
                                    ("reset_global_offset", "zero_global_offset", torch.float32)):
                t_ = reset.get(key)
                if t_ is not None:
                    if t_.dtype != dt_ or not t_.is_contiguous() or t_.numel() != (3 * ne if key == "zero_global_offset" else ne):
                        raise TypeError(f"reset.{key}: contiguous {dt_} tensor of {ne} elements expected")
                    setattr(a, field, t_.data_ptr())
            a.start_offsets = P(start_offsets, "start_offsets", f32, (ne,))
        elif motion_times is not None:
            a.motion_times = P(motion_times, "motion_times", f32, (n,))
        else:
            if progress is None:
                raise TypeError("query needs motion_times or an int64 progress tensor")
            a.progress, a.step_shift, a.dt = P(progress, "progress", torch.int64), int(step_shift), float(dt)
            a.time_steps, a.traj_dt = int(time_steps), float(traj_dt)
            a.start_times, a.start_offsets = P(start_times, "start_times", f32, (ne,)), P(start_offsets, "start_offsets", f32, (ne,))
        a.offset = P(offset, "offset", f32, (ne, 3))
        res = {} if out is None else out
        e = lambda key, *shape, dtype=torch.float32: res[key] if key in res else res.setdefault(key, torch.empty(*shape, dtype=dtype, device=dev))
        if root_only:
            a.root_only = 1
            a.root_pos = e("root_pos", n, 3).data_ptr()
        else:
            shapes = {"rg_pos": (n, j, 3), "rb_rot": (n, j, 4), "body_vel": (n, j, 3), "body_ang_vel": (n, j, 3), "dof_pos": (n, nd),
                      "dof_vel": (n, nd), "rb_records": (n, j, 13)}
            want = fields if fields is not None else ("rg_pos", "rb_rot", "body_vel", "body_ang_vel", "dof_pos", "dof_vel") + (("rb_records",) if with_records else ())
            for k in want:
                t_ = e(k, *shapes[k])
                if tuple(t_.shape) != shapes[k] or t_.dtype != torch.float32 or not t_.is_contiguous():
                    raise ValueError(f"out[{k}]: contiguous float32 {shapes[k]} expected")
                setattr(a, k, t_.data_ptr())
                if k == "rb_records":
                    a.rb_query_stride = t_.stride(0)
        if with_frames:
            a.frame_idx0, a.frame_idx1 = e("frame_idx0", n, dtype=torch.int64).data_ptr(), e("frame_idx1", n, dtype=torch.int64).data_ptr()
            a.blend = e("blend", n).data_ptr()
        launch("pulse_motion_state", ctypes.byref(a))
        return res

    def get_motion_state(self, motion_ids, motion_times, offset=None, out=None):
        """MotionLibBase.get_motion_state (motion_lib_base.py:434-517).  Root entries are views of body 0 (the reference
        clones them); motion_aa / motion_bodies / motion_limb_weights (SMPL shape metadata) are not carried."""
        res = self.query(motion_ids, motion_times, offset, out=out)
        res["root_pos"], res["root_rot"] = res["rg_pos"][:, 0], res["rb_rot"][:, 0]
        res["root_vel"], res["root_ang_vel"] = res["body_vel"][:, 0], res["body_ang_vel"][:, 0]
        return res

    def get_root_pos_smpl(self, motion_ids, motion_times):
        return self.query(motion_ids, motion_times, root_only=True)
