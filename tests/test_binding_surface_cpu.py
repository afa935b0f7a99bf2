"""The binding layer's public surface and the identity of a cached im_step launch.

tests/golden/binding_surface.json was recorded before the wrappers of ``pulse_amd.ops`` / ``pulse_amd.kernels`` were rebuilt on
``pulse_amd._marshal``: every public callable's ``str(inspect.signature(...))`` and every public class's public methods.  Callers pass almost
everything by keyword, so a renamed, reordered or re-defaulted parameter is a behaviour change; new names are allowed.
(Re-record:  python tests/test_binding_surface_cpu.py > tests/golden/binding_surface.json)
"""
import inspect
import json
import os

import pytest
import torch

from pulse_amd import kernels, ops

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "binding_surface.json")


def _surface():
    out = {}
    for mod in (ops, kernels):
        for name, obj in sorted(vars(mod).items()):
            if name.startswith("_") or getattr(obj, "__module__", None) != mod.__name__:
                continue
            if inspect.isclass(obj):
                for m, f in sorted(vars(obj).items()):
                    if inspect.isfunction(f) and (m == "__init__" or not m.startswith("_")):
                        out[f"{mod.__name__}.{name}.{m}"] = str(inspect.signature(f))
            elif inspect.isfunction(obj):
                out[f"{mod.__name__}.{name}"] = str(inspect.signature(obj))
    return out


def test_every_recorded_public_signature_is_unchanged():
    with open(FIXTURE) as f:
        recorded = json.load(f)
    assert len(recorded) > 100                      # (the fixture really lists the two modules)
    now = _surface()
    missing = sorted(set(recorded) - set(now))
    assert not missing, f"public names that disappeared: {missing}"
    changed = {k: (recorded[k], now[k]) for k in recorded if recorded[k] != now[k]}
    assert not changed, f"signatures that changed (recorded, now): {changed}"


# --------------------------------------------------------------------------- #
# the launch cache's signature: computed from everything im_step's body receives
# --------------------------------------------------------------------------- #
N, J = 3, 4


def _t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


class _Lib:
    """Stands in for a MotionLib: _launch_sig asks an object for its launch_signature()."""

    def __init__(self, gen):
        self.gen = gen

    def launch_signature(self):
        return ("lib", self.gen)


def _base():
    ref = lambda: {"pos": _t(N, J, 3), "rot": _t(N, J, 4), "vel": _t(N, J, 3), "ang": _t(N, J, 3)}
    return dict(
        what=7, ref_now=ref(), ref_next=ref(), time_steps=1, dof_force=_t(N, 9), dof_vel=_t(N, 9), progress=_t(N, dtype=torch.int64),
        pass_time=_t(N, dtype=torch.bool), cycle_counter=_t(N, dtype=torch.int64), track_ids=[1, 2], reset_ids=[0, 1], term_dist=_t(J),
        reset_use_mean=False, full_body_reward=True, obs_version=6, local_root_obs=True, root_height_obs=True, specs={"k_pos": 100.0},
        power_coef=0.0005, power_reward=True, env_ids=_t(2, dtype=torch.int64), env_mask=_t(N, dtype=torch.bool), obs=_t(N, 64), obs_cols=64,
        rew=_t(N), rew_raw=_t(N, 5), reset=_t(N, dtype=torch.int64), terminate=_t(N, dtype=torch.int64),
        clock={"progress_rw": _t(N, dtype=torch.int64), "inc": 1, "dt": 1 / 30}, motion={"lib": _Lib(0), "ids": _t(N, dtype=torch.int64)},
        upright=True, enable_early_termination=True, self_obs_version=1, force_sensor=_t(N, 6), dof_pos=_t(N, 9), ref_next_dof_pos=_t(N, 9),
        smpl_params=_t(N, 11), limb_weights=_t(N, 10), recovery_counter=_t(N, dtype=torch.int32),
        zero_out_far={"point_goal": _t(N), "close_distance": 0.25}, occl_bits=_t(N, dtype=torch.int32), occl_reset=False)


def _changed(name, v):
    """Another value for one argument: tensors -> another tensor, flags flipped, dicts with one changed entry."""
    if isinstance(v, torch.Tensor):
        return torch.zeros_like(v)                  # a fresh allocation: another address
    if isinstance(v, bool):
        return not v
    if isinstance(v, dict):
        k = next(iter(v))
        return dict(v, **{k: _changed(k, v[k])})
    if isinstance(v, list):
        return v + [3]
    if isinstance(v, _Lib):
        return _Lib(v.gen + 1)
    if isinstance(v, (int, float)):
        return v + 1
    raise AssertionError(f"no way to change im_step argument {name!r} of type {type(v).__name__}: add a case")


IM_STEP_PARAMS = [p for p in inspect.signature(ops.im_step).parameters if p not in ("cache", "obs_copy")]


def test_equal_arguments_give_equal_signatures_and_obs_copy_is_not_part_of_them():
    rb, kw = _t(N, J, 13), _base()
    sig = ops._im_step_signature(rb, **kw)
    assert sig == ops._im_step_signature(rb, **dict(kw))
    hash(sig)                                       # (compared and stored by the cache: plain nested tuples)
    assert "obs_copy" not in inspect.signature(ops._im_step_signature).parameters
    # im_step itself takes obs_copy (and cache) off before it computes the signature: its body's parameters are im_step's minus those two
    assert sorted(IM_STEP_PARAMS) == sorted(inspect.signature(ops._im_step_fill).parameters)


@pytest.mark.parametrize("name", IM_STEP_PARAMS)
def test_changing_one_argument_changes_the_signature(name):
    rb, kw = _t(N, J, 13), _base()
    assert name == "rb" or name in kw, f"im_step has a parameter this test does not know: {name!r} -- add it to _base()"
    base = ops._im_step_signature(rb, **kw)
    if name == "rb":
        assert ops._im_step_signature(_t(N, J, 13), **kw) != base
        assert ops._im_step_signature(rb[:, :, :].transpose(0, 1), **kw) != base         # same storage, another layout
    else:
        assert ops._im_step_signature(rb, **dict(kw, **{name: _changed(name, kw[name])})) != base


def test_the_debug_bits_are_part_of_the_signature(monkeypatch):
    rb, kw = _t(N, J, 13), _base()
    base = ops._im_step_signature(rb, **kw)
    monkeypatch.setattr(ops, "_IM_DEBUG_BITS", ops._IM_DEBUG_BITS ^ 0x80000000)
    assert ops._im_step_signature(rb, **kw) != base


if __name__ == "__main__":
    print(json.dumps(_surface(), indent=1, sort_keys=True))
