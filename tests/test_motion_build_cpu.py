"""CPU: the fixture pulse_motion_build is held to (tests/golden/motion_build.npz, tools/gen_golden_motion_build.py), the synthetic raw
motion data, the host-side logic of MotionLib.from_motion_data / load_motions that needs no device, and the env keys resample_motions
now reads.

Where the reference checkout is present the fixture is regenerated from the reference's own loader and must match the committed file
bit for bit; elsewhere its keys, shapes and bands are checked."""
import os
import sys

import numpy as np
import torch

from oracle import refload
from pulse_amd import synthetic as syn
from pulse_amd.env import env_keys as K
from pulse_amd.env import motion_lib as ML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "motion_build.npz")
FIELDS = ("gts", "grs", "lrs", "gvs", "gavs", "dvs")
# group -> (bodies, frames per clip, has heading)
GROUPS = {"lengths": (24, [2, 3, 8, 9, 16, 17, 18, 40], False), "smplx": (52, [5, 20], False), "chain": (33, [12], False), "star": (64, [12], False),
          "fps": (24, [10, 10], False), "heading": (24, [10, 10, 10], True), "still": (24, [12], False), "sign": (24, [8], False)}


def _generator():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_golden_motion_build
    return gen_golden_motion_build


def test_fixture_contents():
    assert os.path.getsize(PATH) <= 1 << 20
    z = np.load(PATH)
    assert [str(g) for g in z["groups"]] == list(GROUPS)
    for name, (j, frames, heading) in GROUPS.items():
        total = sum(frames)
        assert z[f"{name}_frames"].tolist() == frames and z[f"{name}_parents"].shape == (j,) and z[f"{name}_parents"][0] == -1
        assert all(0 <= p < b for b, p in enumerate(z[f"{name}_parents"].tolist()) if b > 0)
        assert z[f"{name}_rot"].shape == (total, j, 4) and z[f"{name}_rot"].dtype == np.float32
        assert z[f"{name}_trans"].shape == (total, 3) and z[f"{name}_local_translation"].shape == (len(frames), j, 3)
        assert (f"{name}_heading" in z.files) == heading
        for k in FIELDS:
            e = z[f"{name}_{k}_expected"]
            assert e.dtype == np.float32 and np.isfinite(e).all()
            assert e.shape == (total, j - 1 if k == "dvs" else j, 4 if k in ("grs", "lrs") else 3), (name, k)
    assert z["chain_parents"].tolist() == [b - 1 for b in range(33)] and z["star_parents"].tolist() == [-1] + [0] * 63
    assert z["smplx_parents"].tolist() == syn.SMPLX_PARENTS and z["lengths_parents"].tolist() == syn.SMPL_PARENTS
    assert sorted(set(z["fps_fps"].tolist())) == [30.0, 60.0] and z["heading_heading"].tolist() == [2.5, -2.5, 0.0]
    assert (z["still_rot"][3:7] == z["still_rot"][3]).all() and (z["still_trans"][3:7] == z["still_trans"][3]).all()
    for k in FIELDS:
        assert 0.0 < float(z[f"band_{k}"]) <= 1e-4, k
        big = max(np.abs(z[f"{name}_{k}_expected"].astype(np.float64)).max() for name in GROUPS)
        assert abs(float(z[f"max_{k}"]) - big) <= 1e-6 * big, k                                       # the fp64 maximum, the stored values rounded to fp32
    # the still stretch: the unfiltered angular velocity is exactly zero there, what is expected comes from the filter alone
    assert np.abs(z["still_gavs_expected"][3:6]).max() > 0


def test_fixture_regenerates_bit_for_bit_where_the_reference_is_present():
    if not refload.available():
        return                                                    # the committed fixture is checked by test_fixture_contents
    gen = _generator()
    out = gen.generate(verbose=False)
    z = np.load(PATH)
    assert sorted(out) == sorted(z.files)
    for k in z.files:
        a, b = np.asarray(out[k]), z[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_generator_cases_are_the_fixture_inputs():
    """The inputs need no reference: the generator's draw (which holds its own angle condition) is the committed one -- integers exactly, floats
    to 1e-6 (the draw goes through the host's sin / cos / exp, whose last bit may differ between CPUs; the committed bytes are what the GPU test reads)."""
    gen = _generator()
    z = np.load(PATH)
    for name, case in gen.cases().items():
        for k, v in case.items():
            w = z[f"{name}_{k}"]
            assert v.shape == w.shape and v.dtype == w.dtype, (name, k)
            if v.dtype.kind == "f":
                assert np.abs(v.astype(np.float64) - w.astype(np.float64)).max() <= 1e-6, (name, k)
            else:
                assert np.array_equal(v, w), (name, k)


def test_synthetic_motion_data_is_deterministic_per_seed():
    a, (pa, la) = syn.synthetic_motion_data(syn.make_generator(7), 5, frames=[4, 9, 30, 2, 7], fps=[30, 60, 30, 30, 30], num_slots=3)
    b, (pb, lb) = syn.synthetic_motion_data(syn.make_generator(7), 5, frames=[4, 9, 30, 2, 7], fps=[30, 60, 30, 30, 30], num_slots=3)
    c, _ = syn.synthetic_motion_data(syn.make_generator(8), 5, frames=[4, 9, 30, 2, 7], fps=[30, 60, 30, 30, 30], num_slots=3)
    assert list(a) == list(b) and pa == pb == syn.SMPL_PARENTS and torch.equal(la, lb) and la.shape == (3, 24, 3)
    for k in a:
        assert np.array_equal(a[k]["pose_quat_global"], b[k]["pose_quat_global"]) and torch.equal(a[k]["root_trans_offset"], b[k]["root_trans_offset"])
        assert a[k]["pose_quat_global"].dtype == np.float32 and a[k]["pose_aa"].shape == (a[k]["pose_quat_global"].shape[0], 72)
    assert not np.array_equal(a["clip_0002"]["pose_quat_global"], c["clip_0002"]["pose_quat_global"])
    assert [v["pose_quat_global"].shape[0] for v in a.values()] == [4, 9, 30, 2, 7] and [v["fps"] for v in a.values()] == [30, 60, 30, 30, 30]
    assert ["beta" in v for v in a.values()] == [True, False, True, False, True]
    n = np.linalg.norm(a["clip_0002"]["pose_quat_global"], axis=-1)
    assert np.abs(n - 1).max() < 1e-6
    d52, (p52, l52) = syn.synthetic_motion_data(syn.make_generator(7), 2, humanoid="smplx", frames=[3, 4])
    assert d52["clip_0000"]["pose_quat_global"].shape == (3, 52, 4) and l52.shape == (2, 52, 3) and p52 == syn.SMPLX_PARENTS


def _data(lengths):
    return {f"k{i}": {"pose_quat_global": np.zeros((f, 3, 4), dtype=np.float32)} for i, f in enumerate(lengths)}


def test_min_length_filter_and_im_eval_order():
    data = _data([5, 12, 7, 12, 3])
    assert ML.filter_motion_data(data) == ["k0", "k1", "k2", "k3", "k4"]
    assert ML.filter_motion_data(data, min_length=7) == ["k1", "k2", "k3"]
    assert ML.filter_motion_data(data, im_eval=True) == ["k1", "k3", "k2", "k0", "k4"]              # longest first, ties in file order (sorted is stable)
    assert ML.filter_motion_data(data, min_length=7, im_eval=True) == ["k1", "k2", "k3"]            # the reference's if / elif: min_length wins


def test_sequential_ids_wrap_and_batch_prob():
    p = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.0])
    ids = ML.draw_motion_ids(p, 4, random_sample=False, start_idx=3)
    assert ids.tolist() == [3, 4, 0, 1] and ids.dtype == torch.int64
    assert ML.draw_motion_ids(p, 7, random_sample=False, start_idx=0).tolist() == [0, 1, 2, 3, 4, 0, 1]
    bp = ML.batch_sampling_prob(p, torch.tensor([3, 0, 1, 1]))
    assert torch.allclose(bp, torch.tensor([0.4, 0.1, 0.2, 0.2]) / 0.9) and abs(bp.sum().item() - 1.0) < 1e-6
    keys = ["a", "b", "c", "d", "e"]
    assert [keys[i] for i in ids.tolist()] == ["d", "e", "a", "b"]                                    # curr_motion_keys = _motion_data_keys[sample_idxes]
    # the random draw: repeatable from a generator, never a clip of weight zero
    hard = torch.tensor([0.0, 0.5, 0.0, 0.5, 0.0])
    a = ML.draw_motion_ids(hard, 64, generator=torch.Generator().manual_seed(3))
    b = ML.draw_motion_ids(hard, 64, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, b) and set(a.tolist()) == {1, 3}


def test_crop_ranges():
    start, n = ML.crop_ranges([4, 9, 30, 8], -1)
    assert start.tolist() == [0, 0, 0, 0] and n.tolist() == [4, 9, 30, 8]
    seen = set()
    for s in range(40):
        start, n = ML.crop_ranges([4, 9, 30, 8], 8, torch.Generator().manual_seed(s))
        assert n.tolist() == [4, 8, 8, 8] and start[0] == 0 and start[3] == 0 and 0 <= start[1] <= 1 and 0 <= start[2] <= 22
        seen.add(int(start[1]))
    assert seen == {0, 1}                                                                              # random.randint(0, seq_len - max_len) includes both ends


def test_skeleton_trees_are_duck_typed():
    class Tree:
        def __init__(self, scale):
            self.parent_indices = torch.tensor([-1, 0, 1])
            self.local_translation = scale * torch.ones(3, 3)
    parents, lt = ML._parse_skeleton_trees([Tree(1.0), Tree(2.0)])
    assert parents == [-1, 0, 1] and lt.shape == (2, 3, 3) and lt[1, 2, 0] == 2.0
    parents, lt = ML._parse_skeleton_trees(([-1, 0, 0], np.zeros((4, 3, 3))))
    assert parents == [-1, 0, 0] and lt.shape == (4, 3, 3) and lt.dtype == torch.float32


def test_env_keys_classification():
    for k in ("max_len", "seq_motions"):
        assert k in K.HONOURED and k not in K.INERT and k not in K.UNBUILT
    for k in ("motion_file", "min_length", "hard_negative"):
        assert k in K.INERT
    K.audit({"max_len": 300, "seq_motions": True})
