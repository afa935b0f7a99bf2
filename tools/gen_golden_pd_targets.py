"""Record tests/golden/pd_targets.npz: the actuation stage computed by the REFERENCE's own text.

    python tools/gen_golden_pd_targets.py            (needs the reference tree, oracle/refload.py: PULSE_REFERENCE_ROOT)

Executed as reference text on stubs (oracle.refload: AST-extracted, nothing copied into this repository):
  Humanoid._build_pd_action_offset_scale     phc/env/tasks/humanoid.py:1037-1111
  Humanoid.pre_physics_step                  humanoid.py:1222-1247   with a stub ``gym`` whose set_dof_position_target_tensor records the tensor
  Humanoid._action_to_pd_targets             humanoid.py:1392-1394
  HumanoidIm._action_to_pd_targets           phc/env/tasks/humanoid_im.py:1096-1101   (res_action)
The stub's ``dof_limits_lower / upper`` are float32 tensors, as the reference's are (:895-896), so ``.cpu().numpy()`` gives the method float32
arrays: the bias_offset tables are the reference's float32 array arithmetic, the same under every numpy.  The other branch has ONE scalar path,
1.2 * max|lim| against pi (:1050-1054), where a numpy float32 scalar meets Python floats: numpy 1.x -- the reference's, it still uses np.int --
promotes it to float64, numpy 2 keeps float32 and gives another last bit.  For the bias_offset = False tables only, the stub therefore hands out
float64 copies of the float32 limits (``_Limits``): the scalar path then runs in float64 under any numpy, and nothing else changes, because that
branch's array statements only store the scalar and halve exact sums.  Run under numpy 1.x both stubs give the same bias_offset = False tables.
The action pre_physics_step is handed is torch.clamp(raw, -1, 1), the agent's clamp (phc/learning/im_amp.py:68-73).

The file holds outputs only (tables, the kept actions, the targets), plus float64 sums of the inputs tests/pd_targets_model.py redraws.  The 52-body
humanoids have no L_Hand / R_Hand dof: the reference's freeze_hand lookup raises ValueError for them, which is asserted here, and their cases
freeze the toes only.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pd_targets_model as M                                # noqa: E402
from oracle import refload                                  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pd_targets.npz")


def _reference():
    ns = refload._namespace()
    ns["gymtorch"] = types.SimpleNamespace(unwrap_tensor=lambda t: t)
    ns["flags"] = types.SimpleNamespace(debug=False)
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid.py")
    names = ["_build_pd_action_offset_scale", "pre_physics_step", "_action_to_pd_targets"]
    for name, text in refload._extract(path, names, methods_of="Humanoid").items():
        exec(compile(text, f"<reference:Humanoid.{name}>", "exec"), ns)
    f = {k: ns[k] for k in names}
    f["im_action_to_pd_targets"] = refload.humanoid_im_methods()["_action_to_pd_targets"]
    return f


class _Limits:
    """dof_limits_lower / upper of the bias_offset = False stub: ``.cpu().numpy()`` gives a float64 copy of the float32 limits, which makes the
    branch's one scalar path float64 as under numpy 1.x (module docstring).  The bias_offset = True stub gets the float32 tensors themselves."""

    def __init__(self, t):
        self.t = t

    def cpu(self):
        return self

    def numpy(self):
        return self.t.numpy().astype(np.float64)


def reference_table(f, nb, inp, bias_offset, offset_mode):
    names = M.dof_names(nb)
    env = refload.stub_self(_dof_offsets=np.linspace(0, len(names) * 3, len(names) + 1).astype(int), _dof_names=names, device="cpu",
                            dof_limits_lower=inp["lim_low"].clone() if bias_offset else _Limits(inp["lim_low"]),
                            dof_limits_upper=inp["lim_high"].clone() if bias_offset else _Limits(inp["lim_high"]), _bias_offset=bias_offset,
                            humanoid_type=M.HUMANOIDS[nb], _has_smpl_pd_offset=offset_mode != "none", _has_upright_start=offset_mode == "upright")
    f["_build_pd_action_offset_scale"](env)
    assert env._pd_action_offset.dtype == torch.float32 and env._pd_action_scale.dtype == torch.float32
    return env._pd_action_offset, env._pd_action_scale


def reference_step(f, nb, inp, offset, scale, freeze_hand, freeze_toe, res_action):
    """(self.actions, the tensor handed to gym.set_dof_position_target_tensor) of Humanoid.pre_physics_step on a stub."""
    seen = []
    env = refload.stub_self(device="cpu", _pd_control=True, humanoid_type=M.HUMANOIDS[nb], reduce_action=False, _freeze_hand=freeze_hand,
                            _freeze_toe=freeze_toe, _dof_names=M.dof_names(nb), sim=None, _pd_action_offset=offset, _pd_action_scale=scale,
                            _res_action=res_action, ref_dof_pos=inp["ref_dof_pos"].clone(), _dof_pos=inp["sim_dof_pos"].clone(),
                            gym=types.SimpleNamespace(set_dof_position_target_tensor=lambda sim, t: seen.append(t)))
    # the imitation task overrides _action_to_pd_targets (humanoid_im.py:1096); the residual form exists there only
    to_targets = f["im_action_to_pd_targets"] if res_action else f["_action_to_pd_targets"]
    env._action_to_pd_targets = lambda a: to_targets(env, a)
    f["pre_physics_step"](env, torch.clamp(inp["action"], -M.CLIP, M.CLIP))
    assert len(seen) == 1
    return env.actions, seen[0]


def generate():
    f = _reference()
    out = {}
    for nb in sorted(M.HUMANOIDS):
        inp = M.inputs(nb)
        out[f"{nb}/input_sums"] = M.input_sums(inp)
        tables = {}
        for b in (False, True):
            for m in M.OFFSET_MODES:
                o, s = reference_table(f, nb, inp, b, m)
                tables[(b, m)] = (o, s)
                out[f"{nb}/b{int(b)}_{m}/offset"], out[f"{nb}/b{int(b)}_{m}/scale"] = o.numpy(), s.numpy()
        figures = M.fixture_conditions(nb, inp, tables[(False, "none")][1])
        assert not torch.equal(tables[(False, "none")][0], tables[(True, "none")][0])            # the bias_offset branches differ
        print(f"{nb} bodies: {figures}")
        for key, b, m, h, t, res in M.cases(nb):
            o, s = tables[(b, m)]
            acts, tar = reference_step(f, nb, inp, o, s, h, t, res)
            out[key + "/actions"], out[key + "/target"] = acts.numpy(), tar.numpy()
        if "L_Hand" not in M.dof_names(nb):
            try:
                reference_step(f, nb, inp, *tables[(False, "none")], True, False, False)
            except ValueError:
                pass
            else:
                raise AssertionError("freeze_hand ran on a humanoid without L_Hand")
    return out


if __name__ == "__main__":
    if not refload.available():
        sys.exit(f"the reference tree is not at {refload.REFERENCE_ROOT}")
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(arrays)} arrays, {os.path.getsize(OUT)} bytes")
