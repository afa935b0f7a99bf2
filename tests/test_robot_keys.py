"""CPU: no robot option the reference reads can be dropped silently (pulse_amd/env/robot_keys.py).

  * the set of ``cfg.robot`` keys read by the reference's task classes (re-derived from its sources where the reference checkout is present, the
    recorded set elsewhere: oracle/refrecord.py) -- every one of them must be classified (HONOURED / INERT / UNBUILT), the classes disjoint;
  * every key classified HONOURED is actually read somewhere in pulse_amd/env, pulse_amd/learning or configs.py;
  * the three shipped phc/data/cfg/robot/*.yaml pass the audit and spell the actuation switches as ACTUATION_DEFAULTS has them;
  * switching any UNBUILT option on raises by name; freeze_hand raises for the humanoids without hands;
  * the task classes call the audit.
"""
import glob
import os
import re
import warnings

import pytest
import yaml

from oracle import refload
from oracle.refrecord import RefRecord
from pulse_amd import configs
from pulse_amd import synthetic as syn
from pulse_amd.env import robot_keys as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_keys():
    pat = re.compile(r"""cfg\.robot(?:\.get\(['"]([A-Za-z_0-9]+)['"]|\.([A-Za-z_][A-Za-z_0-9]*)|\[['"]([A-Za-z_0-9]+)['"]\])""")
    keys = set()
    for f in glob.glob(os.path.join(refload.REFERENCE_ROOT, "phc", "**", "*.py"), recursive=True):
        with open(f) as fh:
            for m in pat.finditer(fh.read()):
                keys.add(next(g for g in m.groups() if g))
    keys.discard("get")
    return keys


def _shipped_robot_configs():
    out = {}
    for f in sorted(glob.glob(os.path.join(refload.REFERENCE_ROOT, "phc", "data", "cfg", "robot", "*.yaml"))):
        with open(f) as fh:
            out[os.path.basename(f)] = yaml.safe_load(fh)
    return out


def test_every_key_the_reference_reads_is_classified(request):
    with RefRecord(request) as R:
        keys = set(R.obj("keys", lambda: sorted(_reference_keys())))
    assert len(keys) >= 26, "the source scan found implausibly few keys"
    assert {"freeze_toe", "freeze_hand", "bias_offset", "has_smpl_pd_offset", "reduce_action", "asset", "humanoid_type"} <= keys
    missing = sorted(keys - K.ALL_KNOWN)
    assert not missing, f"robot keys read by the reference but not classified in robot_keys.py: {missing}"
    assert not (K.HONOURED & set(K.INERT)) and not (K.HONOURED & set(K.UNBUILT)) and not (set(K.INERT) & set(K.UNBUILT))
    extra = sorted(K.ALL_KNOWN - keys)
    assert not extra, f"classified but not read by the reference: {extra}"
    for k in ("has_mesh", "replace_feet", "has_jt_limit", "remove_toe", "big_ankle", "box_body", "real_weight", "real_weight_porpotion_capsules",
              "real_weight_porpotion_boxes", "master_range", "has_self_collision", "asset"):
        assert k in K.INERT and K.INERT[k], k
    assert set(K.ACTUATION_DEFAULTS) <= K.HONOURED


def test_honoured_keys_are_really_read():
    src = ""
    for d in ("env", "learning"):
        for f in glob.glob(os.path.join(ROOT, "pulse_amd", d, "*.py")):
            if not f.endswith("robot_keys.py"):
                with open(f) as fh:
                    src += fh.read()
    with open(os.path.join(ROOT, "pulse_amd", "configs.py")) as fh:
        src += fh.read()
    unread = sorted(k for k in K.HONOURED if not re.search(r"""['"]%s['"]""" % re.escape(k), src))
    assert not unread, f"classified HONOURED but never read by pulse_amd: {unread}"
    # the four actuation switches are read THROUGH robot_keys (actuation_switches walks ACTUATION_DEFAULTS): the stage must call it
    with open(os.path.join(ROOT, "pulse_amd", "env", "actuation.py")) as fh:
        act = fh.read()
    assert "robot_keys.actuation_switches(robot)" in act
    for k in K.ACTUATION_DEFAULTS:
        assert re.search(r"""sw\[['"]%s['"]\]""" % k, act), k


def test_the_shipped_robot_files_pass_and_spell_the_defaults(request):
    R = RefRecord(request)
    robots = R.obj("robot_configs", _shipped_robot_configs)
    assert sorted(robots) == ["smpl_humanoid.yaml", "smpl_humanoid_shape.yaml", "smplx_humanoid.yaml"]
    for name, robot in robots.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                   # (motion_sym_loss / sym_loss_coef: read by nothing)
            K.audit(robot, name, syn.skeleton(robot["humanoid_type"])["body_names"])
        assert {k: robot[k] for k in K.ACTUATION_DEFAULTS} == K.ACTUATION_DEFAULTS, name       # why an absent key reads as False
        assert K.actuation_switches(robot) == K.ACTUATION_DEFAULTS
    assert K.actuation_switches(None) == K.ACTUATION_DEFAULTS == configs.ROBOT_ACTUATION
    for h in configs.ROBOTS:
        assert {k: configs.robot_config(h)[k] for k in K.ACTUATION_DEFAULTS} == K.ACTUATION_DEFAULTS
    assert configs.robot_config("smpl", freeze_toe=True)["freeze_toe"] is True
    R.close()


@pytest.mark.parametrize("key", sorted(K.UNBUILT))
def test_unbuilt_options_raise_by_name(key):
    ok, where = K.UNBUILT[key]
    with pytest.raises(NotImplementedError, match=key) as e:
        K.audit({key: True}, "test")
    assert "humanoid.py" in str(e.value) and where in str(e.value)
    K.audit({key: ok[0]}, "test")


def test_freeze_switches_need_the_bodies_they_name():
    names = syn.skeleton("smplx")["body_names"]
    with pytest.raises(NotImplementedError, match="freeze_hand"):
        K.audit({"humanoid_type": "smplx", "freeze_hand": True}, "test", names)
    K.audit({"humanoid_type": "smplx", "freeze_toe": True, "freeze_hand": False}, "test", names)
    K.audit({"humanoid_type": "smpl", "freeze_toe": True, "freeze_hand": True}, "test", syn.skeleton("smpl")["body_names"])
    K.audit(None, "test")


def test_keys_a_task_class_does_not_read_raise_when_switched_on():
    """The downstream tasks build no shape / limb-weight rows: robot/smpl_humanoid_shape.yaml's has_shape_obs must not pass them silently."""
    for key in K.TASK_UNREAD:
        assert key in K.HONOURED
        with pytest.raises(NotImplementedError, match=key):
            K.audit({key: True}, "HumanoidSpeed", unread=K.TASK_UNREAD)
        K.audit({key: False}, "HumanoidSpeed", unread=K.TASK_UNREAD)
        K.audit({key: True}, "HumanoidIm")
    from pulse_amd.env import humanoid_tasks as HT
    with pytest.raises(NotImplementedError, match="has_shape_obs"):
        HT.HumanoidSpeed({"env": {}, "robot": {"humanoid_type": "smpl", "has_shape_obs": True}}, None)


def test_unknown_keys_warn_once():
    K._warned.discard("definitely_not_a_key")
    with pytest.warns(UserWarning, match="definitely_not_a_key"):
        K.audit({"definitely_not_a_key": 1}, "test")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        K.audit({"definitely_not_a_key": 1}, "test")


def test_the_task_classes_audit_cfg_robot():
    """HumanoidIm, HumanoidImGetup (through HumanoidIm's constructor) and HumanoidTask raise for an unbuilt robot option before they touch the
    simulator (none is handed over here)."""
    from pulse_amd.env import humanoid_tasks as HT
    from pulse_amd.env.humanoid_im import HumanoidIm
    from pulse_amd.env.humanoid_im_getup import HumanoidImGetup
    cfg = {"env": {}, "robot": {"humanoid_type": "smpl", "reduce_action": True}}
    for make in (lambda: HumanoidIm(cfg, None, None), lambda: HumanoidImGetup(cfg, None, None), lambda: HT.HumanoidSpeed(cfg, None)):
        with pytest.raises(NotImplementedError, match="reduce_action"):
            make()
