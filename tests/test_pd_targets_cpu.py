"""CPU: the actuation stage's golden fixture (tests/golden/pd_targets.npz, written by tools/gen_golden_pd_targets.py from the reference's own
method bodies) against the restatement tests/pd_targets_model.py and the package's table builder, bit for bit.

  * the redrawn inputs are the recorded ones (float64 sums) and meet the conditions that keep the fixture from hiding a failure;
  * every table (bias_offset both ways, has_smpl_pd_offset off / upright / not upright; 24 and 52 bodies) and every target case (the freeze
    combinations the reference can run, res_action on and off) of the model equals the golden;
  * pulse_amd.env.actuation builds the same tables and freeze masks;
  * with the reference present, the generator reproduces the committed file key by key.
(The kernel and the envs against the model: tests/test_pd_targets_gpu.py.)"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pd_targets_model as M
from oracle import refload
from pulse_amd import synthetic as syn
from pulse_amd.env import actuation as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("pd_targets.npz")


@pytest.mark.parametrize("nb", sorted(M.HUMANOIDS))
def test_inputs_are_the_recorded_ones_and_meet_the_fixture_conditions(gold, nb):
    inp = M.inputs(nb)
    assert inp["action"].shape == (M.N, 3 * (nb - 1))
    assert np.array_equal(gold.np(f"{nb}/input_sums"), M.input_sums(inp)), "the redrawn inputs are not the ones the golden was recorded with"
    figures = M.fixture_conditions(nb, inp, gold.t(f"{nb}/b0_none/scale"))
    print(nb, figures)
    assert not same_bits(gold.np(f"{nb}/b0_none/offset"), gold.np(f"{nb}/b1_none/offset"))          # the bias_offset branches differ
    assert not same_bits(gold.np(f"{nb}/b0_none/scale"), gold.np(f"{nb}/b1_none/scale"))


@pytest.mark.parametrize("nb", sorted(M.HUMANOIDS))
def test_tables_of_the_model_and_of_the_package_equal_the_golden(gold, nb):
    inp, sk = M.inputs(nb), syn.skeleton(M.HUMANOIDS[nb])
    for b in (False, True):
        for m in M.OFFSET_MODES:
            key = f"{nb}/b{int(b)}_{m}"
            o, s = M.offset_scale(nb, inp["lim_low"], inp["lim_high"], b, m)
            assert same_bits(o.numpy(), gold.np(key + "/offset")) and same_bits(s.numpy(), gold.np(key + "/scale")), key
            po, ps = A.pd_action_offset_scale(sk, inp["lim_low"].numpy(), inp["lim_high"].numpy(), bias_offset=b, has_smpl_pd_offset=m != "none",
                                              upright=m == "upright")
            assert same_bits(po, gold.np(key + "/offset")) and same_bits(ps, gold.np(key + "/scale")), key
    # the shipped table: symmetric range, the cap, the knees
    o, s = gold.np(f"{nb}/b0_none/offset"), gold.np(f"{nb}/b0_none/scale")
    names = M.dof_names(nb)
    assert not o.any() and s.max() == 5.0 and s[names.index("L_Knee") * 3 + 1] == 5.0 and s[names.index("R_Knee") * 3 + 1] == 5.0
    assert (np.delete(s, [names.index(k) * 3 + 1 for k in ("L_Knee", "R_Knee")]) <= np.float32(np.pi)).all() and (s == np.float32(np.pi)).any()
    up, nu = gold.np(f"{nb}/b0_upright/offset"), gold.np(f"{nb}/b0_not_upright/offset")
    assert np.count_nonzero(up) == 2 and np.count_nonzero(nu) == 4


@pytest.mark.parametrize("nb", sorted(M.HUMANOIDS))
def test_targets_of_the_model_equal_the_golden(gold, nb):
    inp, sk = M.inputs(nb), syn.skeleton(M.HUMANOIDS[nb])
    keys = [c[0] for c in M.cases(nb)]
    assert len(keys) == len(set(keys)) == 6 + 2 * len(M.freeze_combos(nb)) - 1
    for key, b, m, h, t, res in M.cases(nb):
        o, s = M.offset_scale(nb, inp["lim_low"], inp["lim_high"], b, m)
        fz = M.freeze_columns(nb, h, t)
        assert np.array_equal(fz.numpy().astype(np.uint8), A.freeze_mask(sk, freeze_hand=h, freeze_toe=t))
        a, tar = M.targets(inp["action"], M.CLIP, o, s, fz, inp["ref_dof_pos"] if res else None, inp["sim_dof_pos"] if res else None)
        assert same_bits(a.numpy(), gold.np(key + "/actions")) and same_bits(tar.numpy(), gold.np(key + "/target")), key
        assert (tar[:, fz] == 0).all() and int(fz.sum()) == 6 * (int(h) + int(t))
    # the cases differ from one another where they should: a frozen column, the residual form
    assert not same_bits(gold.np(f"{nb}/b0_none/f00/plain/target"), gold.np(f"{nb}/b0_none/f01/plain/target"))
    assert not same_bits(gold.np(f"{nb}/b0_none/f00/plain/target"), gold.np(f"{nb}/b0_none/f00/res/target"))


def test_the_52_body_humanoids_cannot_freeze_hands():
    assert M.freeze_combos(24) == [(False, False), (False, True), (True, False), (True, True)]
    assert M.freeze_combos(52) == [(False, False), (False, True)]
    with pytest.raises(ValueError):
        A.freeze_mask(syn.skeleton("smplx"), freeze_hand=True)


def test_limits_shape_and_pairing_are_checked():
    sk = syn.skeleton("smpl")
    lo, hi = syn.synthetic_dof_limits("smpl")
    assert lo.dtype == torch.float32 and lo.shape == (69,) and (lo < hi).all()
    assert syn.synthetic_dof_limits("smplx")[0].shape == (153,)
    assert not torch.equal(lo, syn.synthetic_dof_limits("smpl", seed=1)[0])
    with pytest.raises(ValueError, match="dof limits"):
        A.pd_action_offset_scale(sk, lo.numpy()[:-1], hi.numpy()[:-1])


def test_table_switches_without_published_limits_raise():
    """bias_offset / has_smpl_pd_offset act on a table built from the limits: a simulator that publishes none cannot honour them (raised before
    any tensor is made, so no device is needed); the freeze switches need no limits."""
    import types
    sk = syn.skeleton("smpl")
    for key in ("bias_offset", "has_smpl_pd_offset"):
        with pytest.raises(ValueError, match="dof_limits"):
            A.Actuation(sk, {key: True}, types.SimpleNamespace(), "cpu")
    with pytest.raises(ValueError, match="both or neither"):
        A.Actuation(sk, {}, types.SimpleNamespace(dof_limits_lower=torch.zeros(69)), "cpu")
    act = A.Actuation(sk, {"freeze_toe": True}, types.SimpleNamespace(), "cpu")
    assert not act.offset.any() and (act.scale == 1).all() and int(act.freeze.sum()) == 6 and act.clip == float("inf")
    assert A.Actuation(sk, None, types.SimpleNamespace(), "cpu").freeze is None


@pytest.mark.skipif(not refload.available(), reason="re-derivation needs the reference checkout")
def test_generator_reproduces_the_committed_golden(gold):
    spec = importlib.util.spec_from_file_location("gen_golden_pd_targets", os.path.join(ROOT, "tools", "gen_golden_pd_targets.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    arrays = gen.generate()
    assert set(arrays) == set(gold.z.files)
    for k, v in arrays.items():
        g = gold.np(k)
        assert g.dtype == v.dtype and g.shape == v.shape and np.array_equal(g.view(np.int64 if v.dtype == np.float64 else np.int32),
                                                                            v.view(np.int64 if v.dtype == np.float64 else np.int32)), k
