"""A numpy / torch restatement of the actuation stage, independent of pulse_amd/env/actuation.py and of the kernel, plus the inputs and the cases of
tests/golden/pd_targets.npz (tools/gen_golden_pd_targets.py records what the REFERENCE's own method bodies give for them).

  offset_scale   Humanoid._build_pd_action_offset_scale, phc/env/tasks/humanoid.py:1037-1111, all joints with three dofs.  The reference's limits
                 are float32 arrays: the bias_offset branch is float32 array arithmetic throughout (torch float32 here: the same IEEE operations);
                 the cap of the other branch, min(1.2 max|lim|, pi), is a SCALAR computation that numpy 1.x -- the reference's numpy -- does in
                 float64 and rounds on the store, which is what float64 here does
  targets        clamp -> Humanoid.pre_physics_step (:1222-1247) over _action_to_pd_targets (:1392-1394; humanoid_im.py:1096-1101), eager torch on
                 the CPU: every operation is exact or correctly rounded, so the kernel has to give the same bits
"""
import numpy as np
import torch

from pulse_amd import synthetic as syn

N = 5
HUMANOIDS = {24: "smpl", 52: "smplx"}
ACTION_SIGMA = 1.5            # N(0, 1.5^2): P(|a| > 1) = 0.505
POSE_SIGMA = 0.3              # reference and simulated dof positions, rad
OFFSET_MODES = ("none", "upright", "not_upright")            # has_smpl_pd_offset off | on with upright start | on without
CLIP = 1.0


def dof_names(nb):
    return syn.skeleton(HUMANOIDS[nb])["body_names"][1:]


def freeze_combos(nb):
    """(freeze_hand, freeze_toe) pairs the reference can run: the 52-body humanoids have no L_Hand / R_Hand dof (humanoid.py:1240 raises)."""
    return [(h, t) for h in ((False, True) if "L_Hand" in dof_names(nb) else (False,)) for t in (False, True)]


def inputs(nb, n=N, seed=0):
    """The redrawn inputs of the golden cases: joint limits, raw action, reference and simulated dof positions (float32 CPU tensors)."""
    lo, hi = syn.synthetic_dof_limits(HUMANOIDS[nb], seed)
    g = torch.Generator().manual_seed(4400 + 7 * nb + seed)
    d = 3 * (nb - 1)
    action = ACTION_SIGMA * torch.randn(n, d, generator=g)
    ref = POSE_SIGMA * torch.randn(n, d, generator=g)
    sim = ref + POSE_SIGMA * torch.randn(n, d, generator=g)
    return {"lim_low": lo, "lim_high": hi, "action": action, "ref_dof_pos": ref, "sim_dof_pos": sim}


def input_sums(inp):
    """float64 sums of the inputs, stored in the golden so that a changed draw is noticed."""
    return np.array([inp[k].double().sum().item() for k in ("lim_low", "lim_high", "action", "ref_dof_pos", "sim_dof_pos")], dtype=np.float64)


def offset_scale(nb, lim_low, lim_high, bias_offset, offset_mode):
    names = dof_names(nb)
    lo, hi = lim_low.float().clone(), lim_high.float().clone()
    if bias_offset:
        mid, half = 0.5 * (hi + lo), 0.7 * (hi - lo)                       # float32 tensors: every statement rounds to float32, as :1076-1087
        lo, hi = mid - half, mid + half
    else:
        peak = torch.maximum(lo.abs(), hi.abs()).view(-1, 3).max(dim=1).values.double()
        cap = torch.clamp(1.2 * peak, max=np.pi).float()                  # float64 product and min, one rounding (:1050-1057 under numpy 1.x)
        hi = cap.repeat_interleave(3)
        lo = -hi
    offset, scale = 0.5 * (hi + lo), 0.5 * (hi - lo)
    for knee in ("L_Knee", "R_Knee"):
        scale[names.index(knee) * 3 + 1] = 5
    ls, rs = names.index("L_Shoulder") * 3, names.index("R_Shoulder") * 3
    if offset_mode == "upright":
        offset[ls], offset[rs] = -np.pi / 2, np.pi / 2
    elif offset_mode == "not_upright":
        offset[ls], offset[ls + 2], offset[rs], offset[rs + 2] = -np.pi / 6, -np.pi / 2, -np.pi / 3, np.pi / 2
    return offset, scale


def freeze_columns(nb, freeze_hand, freeze_toe):
    names = dof_names(nb)
    mask = torch.zeros(3 * len(names), dtype=torch.bool)
    for b in (("L_Hand", "R_Hand") if freeze_hand else ()) + (("L_Toe", "R_Toe") if freeze_toe else ()):
        mask[names.index(b) * 3:names.index(b) * 3 + 3] = True
    return mask


def targets(action, clip, offset, scale, freeze=None, ref_dof_pos=None, sim_dof_pos=None):
    """(clamped action, PD targets) on the CPU."""
    a = torch.clamp(action, -clip, clip)
    if ref_dof_pos is not None:
        t = ref_dof_pos + scale * a
        t = torch.maximum(torch.minimum(t, sim_dof_pos + np.pi / 2), sim_dof_pos - np.pi / 2)
    else:
        t = offset + scale * a
    if freeze is not None:
        t = torch.where(freeze.bool()[None, :], torch.zeros_like(t), t)
    return a, t


def cases(nb):
    """(key, bias_offset, offset_mode, freeze_hand, freeze_toe, res_action) of the golden's target cases: every table with nothing frozen and the
    plain form; every freeze combination, plain and residual, on the shipped table."""
    out = [(f"{nb}/b{int(b)}_{m}/f00/plain", b, m, False, False, False) for b in (False, True) for m in OFFSET_MODES]
    for h, t in freeze_combos(nb):
        for res in (False, True):
            key = f"{nb}/b0_none/f{int(h)}{int(t)}/{'res' if res else 'plain'}"
            if key not in [c[0] for c in out]:
                out.append((key, False, "none", h, t, res))
    return out


def fixture_conditions(nb, inp, scale_res):
    """The conditions that keep the fixture from hiding a failure; returns the measured figures, asserts the bounds."""
    lo, hi = inp["lim_low"].double(), inp["lim_high"].double()
    peak = torch.maximum(lo.abs(), hi.abs()).view(-1, 3).max(dim=1).values
    capped, free = int((1.2 * peak > np.pi).sum()), int((1.2 * peak <= np.pi).sum())
    assert capped >= 1 and free >= 1, (capped, free)                       # the min(1.2 max|lim|, pi) cap acts on some joints and not on others
    asym = float(((lo + hi).abs() > 1e-3).double().mean())
    assert asym >= 1.0 / 3.0, asym                                         # the two bias_offset branches differ
    outside = float((inp["action"].abs() > CLIP).double().mean())
    assert 0.2 <= outside <= 0.8, outside                                  # the clamp acts, and not everywhere
    _, t = targets(inp["action"], CLIP, None, scale_res, None, inp["ref_dof_pos"], inp["sim_dof_pos"])
    bound = float(((t == inp["sim_dof_pos"] + np.pi / 2) | (t == inp["sim_dof_pos"] - np.pi / 2)).double().mean())
    assert 0.1 <= bound <= 0.9, bound                                      # the +- pi / 2 window acts, and not everywhere
    return {"capped_joints": capped, "uncapped_joints": free, "asymmetric_dofs": asym, "actions_outside": outside, "on_bound": bound}
