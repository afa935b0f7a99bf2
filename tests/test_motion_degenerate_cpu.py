"""CPU: the degenerate-clip fixture the motion-query kernels are held to (tests/golden/motion_degenerate.npz, oracle/gen_golden.py:
gen_motion_degenerate) -- still, frozen, identity, slow and sign-flipped joints, clips of 2 and 3 frames, queried at every exact frame time
and clip edge.

The reference's slerp is discontinuous for slow joints and which side a pair falls on depends on the summation order of a dot product
(profiles/motion_degenerate_branches.txt).  The fixture is built so that the reference alone is stable on every input
(oracle/degenerate_clips.py: classify, query_conditions); here that is PROVEN of the committed bytes, the oracle restatement is held
to the reference's outputs by the rule of test_motion_lib.py, and every branch is shown to occur."""
import os

import numpy as np
import pytest
import torch

from oracle import degenerate_clips as D
from oracle import refload
from oracle.motion_oracle import OracleMotionLib

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "motion_degenerate.npz")
EXACT = ("rg_pos", "body_vel", "body_ang_vel", "dof_vel", "root_pos", "root_vel", "root_ang_vel")
ROT = ("rb_rot", "root_rot", "dof_pos")


def load():
    return D.load_fixture(GOLDEN)


def test_fixture_is_small_and_holds_the_planned_clips():
    assert os.path.getsize(GOLDEN) <= 1 << 20
    z, tabs, info = load()
    assert tabs["motion_num_frames"].tolist() == [c[0] for c in D.CLIPS] and tabs["motion_fps"].tolist() == [c[1] for c in D.CLIPS]
    assert set(tabs["motion_num_frames"].tolist()) == {2, 3, 9, 17} and set(tabs["motion_fps"].tolist()) == {30.0, 60.0}
    assert torch.equal(tabs["length_starts"], torch.cumsum(tabs["motion_num_frames"], 0) - tabs["motion_num_frames"])
    assert 350 <= z["motion_ids"].shape[0] <= 450
    D._check_kinds(tabs, info)                                  # frozen = same bits, identity = (0, 0, 0, 1), moving >= 4e-3, the still clip, ...
    kinds = info["kinds"]
    from pulse_amd import synthetic as syn
    hands = [syn.SMPL_BODY_NAMES.index(n) for n in ("L_Hand", "R_Hand")]
    assert (kinds[:, hands] == D.IDENTITY).all()
    what = [c[2] for c in D.CLIPS]
    for m, w in enumerate(what):
        if w != "still":
            assert set(kinds[m].tolist()) >= {D.MOVING, D.FROZEN, D.IDENTITY, D.SLOW}, m
            assert D.FLIPPED in kinds[m] or D.FLIPPED_ALT in kinds[m], m
    assert kinds[what.index("root-flipped"), 0] == D.FLIPPED and (kinds[what.index("alternate")] == D.FLIPPED_ALT).sum() == 1
    # the stretch: frames 5 .. 9 of that clip hold the same bits in every table, inside a clip that moves before and after
    s = int(tabs["length_starts"][what.index("stretch")])
    a, b = D.STRETCH
    for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs"):
        t = tabs[k][s + a:s + b + 1]
        assert torch.equal(t, t[:1].expand_as(t)), k
    assert not torch.equal(tabs["lrs"][s + a - 1], tabs["lrs"][s + a]) and not torch.equal(tabs["lrs"][s + b], tabs["lrs"][s + b + 1])
    # grs is the fp32 forward-kinematics product of lrs: unit length, the root's own rotation at body 0
    assert torch.allclose(tabs["grs"].norm(dim=-1), torch.ones(()), atol=1e-6)
    np.testing.assert_allclose(tabs["grs"][:, 0].numpy(), tabs["lrs"][:, 0].numpy(), atol=1.2e-7, rtol=0)


def test_queries_hit_every_frame_and_clip_edge():
    z, tabs, _ = load()
    ids, times = torch.from_numpy(z["motion_ids"]), torch.from_numpy(z["motion_times"])
    assert torch.isfinite(times).all() and ids.min() == 0 and ids.max() == len(D.CLIPS) - 1
    inf = torch.tensor(float("inf"))
    for m, (n, dt, length) in enumerate(zip(tabs["motion_num_frames"].tolist(), tabs["motion_dt"], tabs["motion_lengths"])):
        t = times[ids == m]
        f0, f1, blend = z["frame_idx0"][z["motion_ids"] == m], z["frame_idx1"][z["motion_ids"] == m], z["blend"][z["motion_ids"] == m]
        for k in range(n):
            assert (t == k * dt).any(), (m, k)                                           # every exact frame time, 0 and the last included
        for edge in (length, torch.nextafter(length, inf), torch.nextafter(length, -inf)):
            assert (t == edge).any(), m
        assert (t < 0).sum() >= 2 and (t > length * 1.1).any()
        assert set(f0.tolist()) == set(range(n)) and (f0 == f1).any() and (blend == 0).any() and ((blend > 0) & (blend < 1)).any()
        assert ((t > 0) & (t < length)).sum() >= 5 * (n - 1)                             # mid-blend times


def test_oracle_reproduces_reference_fixture():
    """The rule of test_oracle_reproduces_reference_golden: lerp'd fields, frame indices and blend bit for bit; slerp / exp-map fields to 2e-6."""
    z, tabs, _ = load()
    o = OracleMotionLib(tabs)
    ids, times, off = (torch.from_numpy(z[k]) for k in ("motion_ids", "motion_times", "offset"))
    r = o.get_motion_state(ids, times, off)
    for k in EXACT:
        assert np.array_equal(r[k].numpy(), z[k]), k
    for k in ROT:
        np.testing.assert_allclose(r[k].numpy(), z[k], atol=2e-6, rtol=0, err_msg=k)
    base = tabs["length_starts"][ids].numpy()
    assert np.array_equal(r["frame_idx0"].numpy() - base, z["frame_idx0"])
    assert np.array_equal(r["frame_idx1"].numpy() - base, z["frame_idx1"])
    assert np.array_equal(r["blend"].numpy(), z["blend"])
    assert np.array_equal(o.get_motion_state(ids, times)["rg_pos"].numpy(), z["rg_pos_no_offset"])
    assert np.array_equal(o.get_root_pos_smpl(ids, times)["root_pos"].numpy(), z["root_pos_smpl"])


def test_fixture_is_stable_on_every_pair_and_every_query():
    """The conditions under which the reference alone is well defined hold on the committed bytes: none of the 380 x 24 cells is left out."""
    z, tabs, info = load()
    assert D.unstable_pairs(tabs) == []
    lab = D.pair_labels(tabs)
    for k in ("pair_rows", "lrs_labels", "grs_labels"):
        assert np.array_equal(lab[k], info[k]), k
    assert lab["lrs_stable"].all() and lab["grs_stable"].all()
    ids, times = torch.from_numpy(z["motion_ids"]), torch.from_numpy(z["motion_times"])
    assert D.query_conditions(tabs, ids, times) == []
    # the reference's own outputs say the same: dof_pos of an identity joint is exactly zero, nothing else is
    dof = z["dof_pos"].reshape(len(ids), -1, 3)
    ident = info["kinds"][z["motion_ids"]][:, 1:] == D.IDENTITY
    assert (dof[ident] == 0).all() and (np.abs(dof[~ident]).max(-1) > 1e-3).all()


def test_every_branch_occurs():
    z, tabs, info = load()
    ids, times = torch.from_numpy(z["motion_ids"]), torch.from_numpy(z["motion_times"])
    cell_l, cell_g = D.cell_labels(tabs, info, ids, times)
    rows = info["pair_rows"]
    for name, labels in (("lrs pairs", info["lrs_labels"][rows]), ("grs pairs", info["grs_labels"][rows]), ("lrs cells", cell_l), ("grs cells", cell_g)):
        counts = D.label_counts(labels)
        print(f"{name}: {counts}")
        for branch, c in counts.items():
            assert c > 0, (name, branch)
    # a flip occurs together with the general branch (the only one where the sign of q1 matters to more than round-off)
    assert ((info["lrs_labels"] >= D.FLIP) & (info["lrs_labels"] % D.FLIP == D.GEN)).any()


def test_classify_on_hand_made_pairs():
    q = np.array([0.0, 0.6, 0.0, 0.8], dtype=np.float32)
    ident = np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32)

    def rot(h):
        return np.array([np.sin(h), 0.0, 0.0, np.cos(h)], dtype=np.float32)
    stable, label = D.classify(np.stack([q, ident, ident, ident, ident]), np.stack([q, ident, rot(0.3), -rot(0.3), rot(7.5e-4)]))
    assert stable.tolist() == [True] * 5
    assert label.tolist() == [D.Q0, D.IDENT, D.GEN, D.GEN + D.FLIP, D.MID]
    # on a threshold: not stable.  c = 1 - 8 ulp puts sqrt(1 - c c) within an ulp of 0.001; a half turn puts c at 0; q against -q puts |c|
    # at 1 without the bits being the same
    stable, _ = D.classify(np.stack([ident, ident, ident]), np.stack([rot(9.77e-4), np.array([1.0, 0.0, 0.0, 0.0], dtype=np.float32), -ident]))
    assert stable.tolist() == [False, False, False]


def test_slow_pairs_without_the_predicate_disagree_between_summation_orders():
    """Why the predicate exists: random pairs at slow half-angles take DIFFERENT slerp branches under different association orders of the
    same fp32 dot product (tools/motion_degenerate_branches.py, the rows of profiles/motion_degenerate_branches.txt), and the two results
    then differ by 0.5 |q1 - q0|: two orders of magnitude above the 2e-6 the query is held to.  Inside the band the builder draws from,
    the orders agree on most pairs but a good share sits within 2 ulp of a threshold: every drawn pair is checked, the band is not trusted."""
    rng = np.random.default_rng(5)
    n = 50000
    for h, gap_floor in ((1e-4, 4e-5), (3e-4, 1.2e-4), (5e-4, 2e-4), (9e-4, 4e-4)):
        q0, q1 = D.draw_pairs(rng, n, h)
        branches = np.stack([D.branch_of(c) for c in D.dot_forms(q0, q1)])
        differ = (branches != branches[0]).any(0)
        stable, _ = D.classify(q0, q1)
        gap = np.abs(0.5 * (q1 - q0))[differ].max()
        print(f"half-angle {h:g}: {100 * differ.mean():.3f} % of pairs differ between orders, max gap {gap:.2e}, {100 * stable.mean():.1f} % stable")
        assert differ.any() and gap > gap_floor > 10 * 2e-6, h
        assert not (stable & differ).any(), h                    # the predicate rejects every pair on which the orders disagree
    for h in D.SLOW_HALF_ANGLE:
        stable, label = D.classify(*D.draw_pairs(rng, n, h))
        print(f"half-angle {h:g}: {100 * stable.mean():.1f} % stable")
        assert 0.5 < stable.mean() < 1.0 and (label[stable] == D.MID).all(), h
    stable, label = D.classify(*D.draw_pairs(rng, n, D.MOVING_MIN_HALF_ANGLE))
    assert stable.all() and (label == D.GEN).all()              # a moving pair is on the general branch whatever the order


@pytest.mark.parametrize("humanoid", [33, "smplx", 64])
def test_builder_on_the_wide_trees(humanoid):
    """build() asserts the stability of every pair itself; here also that every kind and branch survives on the other trees."""
    tabs, info = D.build(11, humanoid)
    j = len(D.tree(humanoid)["parents"])
    assert tabs["lrs"].shape == (62, j, 4) and tabs["dvs"].shape == (62, j - 1, 3)
    ids, times, _ = D.queries(tabs, 11)
    assert D.query_conditions(tabs, ids, times) == []
    for labels in (info["lrs_labels"][info["pair_rows"]], info["grs_labels"][info["pair_rows"]]):
        assert all(c > 0 for c in D.label_counts(labels).values())
    again, _ = D.build(11, humanoid)
    assert all(torch.equal(tabs[k], again[k]) for k in tabs)


def test_fixture_regenerates_bit_for_bit_where_the_reference_is_present():
    if not refload.available():
        return                                                    # the committed fixture is checked by the tests above
    from oracle import gen_golden
    out = gen_golden.motion_degenerate()
    z = np.load(GOLDEN)
    assert sorted(out) == sorted(z.files)
    for k in z.files:
        a, b = np.asarray(out[k]), z[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
