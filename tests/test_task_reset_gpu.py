"""GPU: pulse_task_ref_state_init (csrc/task_reset.hip, ops.task_ref_state_init) against tests/task_reset_model.py, which
tests/test_task_reset_cpu.py pins to the reference's own _sample_ref_state / _reset_ref_state_init bodies.

Every transform, upright both ways for the heading removal, 1 / 9 / 33 envs (less than a workgroup's eight, one more than a workgroup, more
than four workgroups with a ragged last one), masks all / none / alternating / last env only, times 0, a clip's exact length, past its
end and random.  Tolerances are the project's figures for these outputs: with no transform the lerped quantities bit for bit and the
rotations to 2e-6 (the motion query, tests/test_smplx_gpu.py:235-238); transformed states to 1e-5 absolute (the env kernels,
tests/test_amp_variants_gpu.py:4); ids, times and clears exactly.  Rows outside the mask keep their poison in every output.

Terrain: a centre-grid sample within 1e-4 m of a cell edge may take the neighbouring cell on the device (its sinf / cosf differ from libm
by an ulp), as the height map of tests/test_terrain_gpu.py; such samples are counted and held to that file's cap of 2e-3 of the samples.
The new locations are chosen so that the model's own samples stay inside the cap (asserted), so a lift that differs must be explained by
an edge sample or fails.  (explain_height_differences itself walks a sensor grid turned by a body's HEADING; the centre grid is turned by
the root's yaw-only quaternion, so the count is taken here on the model's cell coordinates.)
"""
import numpy as np
import pytest
import torch

import task_reset_model as M
from amp_frame_model import non_upright_tables
from oracle import task_oracle as TO
from oracle.motion_oracle import OracleMotionLib
from pulse_amd import _lib, ops, synthetic as syn
from pulse_amd.env.motion_lib import MotionLib

pytestmark = pytest.mark.gpu

HSCALE, VSCALE = 0.1, 0.005
EDGE = 1e-4                          # metres from a cell edge inside which the device may take the neighbouring cell
CASES = [("none", True), ("zero_xy", True), ("remove_heading", True), ("remove_heading", False), ("terrain", True)]
_shared = {}


def _tables(upright):
    if upright not in _shared:
        tabs = syn.synthetic_motion_library(syn.make_generator(2), 5, 12, 30)
        _shared[upright] = tabs if upright else non_upright_tables(tabs)
    return _shared[upright]


def _near_edge(cells):
    return ((cells - cells.round()).abs() <= EDGE / HSCALE).any(dim=-1)           # (n, P): the sample's x or y cell coordinate is near an integer


def _inputs(n, upright):
    """ids, times (0, exact length, past the end, random), new locations away from cell edges -- computed once per (n, upright) and shared."""
    key = ("in", n, upright)
    if key in _shared:
        return _shared[key]
    tabs = _tables(upright)
    lib = OracleMotionLib(tabs)
    g = syn.make_generator(100 + n)
    ids = torch.randint(0, 5, (n,), generator=g)
    length = tabs["motion_lengths"][ids]
    times = torch.rand(n, generator=g) * length
    kind = torch.arange(n) % 4
    times = torch.where(kind == 0, torch.zeros(n), torch.where(kind == 1, length, torch.where(kind == 2, length + 0.7, times)))
    hs, cp = syn.synthetic_height_field(), torch.cat([syn.center_height_points(), torch.zeros(9, 1)], dim=1)
    xy = 3.0 + torch.rand(n, 2, generator=g) * torch.tensor([20.0, 24.0])
    root_rot = lib.get_motion_state(ids, times)["root_rot"]
    for _ in range(50):                                                            # move the locations whose centre grid touches a cell edge
        bad = _near_edge(M.center_sample_cells(torch.cat([xy, torch.zeros(n, 1), root_rot], dim=1), cp, HSCALE, upright)).any(dim=-1)
        if not bad.any():
            break
        xy = torch.where(bad[:, None], 3.0 + torch.rand(n, 2, generator=g) * torch.tensor([20.0, 24.0]), xy)
    _shared[key] = (lib, ids, times, hs, cp, xy)
    return _shared[key]


def _model(transform, n, upright):
    key = ("model", transform, n, upright)
    if key not in _shared:
        lib, ids, times, hs, cp, xy = _inputs(n, upright)
        _shared[key] = M.ref_state(lib, ids, times, transform, upright=upright, new_root_xy=xy, heightsamples=hs, center_points=cp,
                                   horizontal_scale=HSCALE, vertical_scale=VSCALE)
    return _shared[key]


def _masks(n):
    alt = torch.arange(n) % 2 == 0
    last = torch.zeros(n, dtype=torch.bool)
    last[-1] = True
    return {"all": torch.ones(n, dtype=torch.bool), "none": torch.zeros(n, dtype=torch.bool), "alternating": alt, "last": last}


def _poisoned(n, j, dev):
    nan = float("nan")
    return {"rb": torch.full((n, j, 13), nan, device=dev), "dof_pos": torch.full((n, 3 * (j - 1)), nan, device=dev),
            "dof_vel": torch.full((n, 3 * (j - 1)), nan, device=dev), "start_times": torch.full((n,), nan, device=dev),
            "sampled_ids": torch.full((n,), -7, dtype=torch.int64, device=dev),
            "clears": tuple(torch.full((n,), 5 + i, dtype=torch.int64, device=dev) for i in range(3))}


def _launch(lib, ids, times, mask, out, dev, **kw):
    ops.task_ref_state_init(lib, ids.to(dev), times.to(dev), mask.to(dev), out["rb"], out["dof_pos"], out["dof_vel"], out["start_times"],
                            out["sampled_ids"], clears=out["clears"], **kw)


def _untouched(out, rows):
    for k in ("rb", "dof_pos", "dof_vel", "start_times"):
        assert torch.isnan(out[k][rows]).all(), k
    assert (out["sampled_ids"][rows] == -7).all()
    for i, c in enumerate(out["clears"]):
        assert (c[rows] == 5 + i).all()


@pytest.mark.parametrize("n", [1, 9, 33])
@pytest.mark.parametrize("transform,upright", CASES, ids=[f"{t}-{'up' if u else 'noup'}" for t, u in CASES])
def test_reset_kernel_matches_model(dev, transform, upright, n):
    cpu_lib, ids, times, hs, cp, xy = _inputs(n, upright)
    assert M.heading_axis_xy(cpu_lib, ids, times, upright).min() >= 0.1            # input condition: the heading is atan2 of this projection
    m = _model(transform, n, upright)
    lib = MotionLib.from_tables(_tables(upright), dev)
    kw = {"transform": transform, "upright": upright}
    samples = n * cp.shape[0]
    if transform == "terrain":
        kw.update(new_root_xy=xy.to(dev), heightsamples=hs.to(dev), horizontal_scale=HSCALE, vertical_scale=VSCALE, center_points=cp[:, :2].contiguous().to(dev))
        moved = torch.cat([m["root_pos"], m["root_rot"]], dim=1)
        near = _near_edge(M.center_sample_cells(moved, cp, HSCALE, upright))
        assert near.sum().item() <= 2e-3 * samples                                 # the inputs keep the model itself inside the cap
    want = m["records"]
    for name, mask in _masks(n).items():
        out = _poisoned(n, 24, dev)
        _launch(lib, ids, times, mask, out, dev, **kw)
        sel = mask.nonzero().flatten()
        _untouched(out, (~mask).nonzero().flatten().to(dev))
        if sel.numel() == 0:
            continue
        got = out["rb"].cpu()[sel]
        w = want[sel]
        assert torch.equal(out["sampled_ids"].cpu()[sel], ids[sel]) and torch.equal(out["start_times"].cpu()[sel], times[sel]), name
        for c in out["clears"]:
            assert (c.cpu()[sel] == 0).all(), name
        assert torch.equal(out["dof_vel"].cpu()[sel], m["dof_vel"][sel]), name     # a lerp, never transformed
        assert (out["dof_pos"].cpu()[sel] - m["dof_pos"][sel]).abs().max().item() <= 2e-6, name
        if transform == "none":
            for lo, hi in ((0, 3), (7, 10), (10, 13)):                             # lerped: position, linear and angular velocity
                assert torch.equal(got[..., lo:hi], w[..., lo:hi]), (name, lo)
            assert (got[..., 3:7] - w[..., 3:7]).abs().max().item() <= 2e-6, name  # slerped
            continue
        if transform == "terrain":
            # a lift that differs is the lift of a neighbouring cell under an edge sample: counted, capped; every other env to 1e-5
            dz = (got[:, 0, 2] - w[:, 0, 2]).abs()
            flipped = dz > 1e-5
            assert not (flipped & ~near[sel].any(dim=-1)).any(), f"{name}: a centre height differs although no sample sits on a cell edge"
            flips = int(near[sel][flipped].sum())
            print(f"[task reset] terrain n={n} mask={name}: {flips} of {samples} centre samples sit on a cell edge and may take the neighbouring cell")
            assert flips <= 2e-3 * samples
            assert (dz[flipped] <= 0.5).all()                                      # one cell's step of the synthetic field, not garbage
            got, w = got[~flipped], w[~flipped]
            assert torch.equal(got[:, 0, 0:2], xy[sel][~flipped])                  # the root stands exactly on the new location
        err = (got - w).abs().max().item()
        print(f"[task reset] {transform} upright={upright} n={n} mask={name}: max abs error {err:.3e}")
        assert err <= 1e-5, (name, err)
        if transform == "zero_xy":
            assert (got[:, 0, 0:2] == 0).all()


def test_terrain_centre_samples_one_by_one(dev):
    """The nine centre samples separately (a one-point centre grid per launch): every sample's height against the model's, so the mean of
    the full grid cannot hide a wrong cell; and the plane (no height field): moved, not lifted."""
    n, upright = 33, True
    cpu_lib, ids, times, hs, cp, xy = _inputs(n, upright)
    lib = MotionLib.from_tables(_tables(upright), dev)
    m = _model("terrain", n, upright)
    moved = torch.cat([m["root_pos"], m["root_rot"]], dim=1)
    each = TO.terrain_center_heights(hs, moved, cp, HSCALE, VSCALE, upright)                # (n, 9)
    base = _model("none", n, upright)["records"][:, 0, 2]
    mask = torch.ones(n, dtype=torch.bool)
    for k in range(cp.shape[0]):
        out = _poisoned(n, 24, dev)
        _launch(lib, ids, times, mask, out, dev, transform="terrain", new_root_xy=xy.to(dev), heightsamples=hs.to(dev), horizontal_scale=HSCALE,
                vertical_scale=VSCALE, center_points=cp[k:k + 1, :2].contiguous().to(dev))
        assert ((out["rb"][:, 0, 2].cpu() - base) - each[:, k]).abs().max().item() <= 1e-5, k
    out = _poisoned(n, 24, dev)
    _launch(lib, ids, times, mask, out, dev, transform="terrain", new_root_xy=xy.to(dev))
    flat = M.ref_state(cpu_lib, ids, times, "terrain", new_root_xy=xy)["records"]
    assert (out["rb"].cpu() - flat).abs().max().item() <= 1e-5 and torch.equal(out["rb"][:, :, 2].cpu(), _model("none", n, upright)["records"][:, :, 2])


def test_too_many_bodies_is_an_argument_error(dev):
    """num_bodies = 33: one lane per body inside a 32-lane half-wave does not fit; reported by name, nothing is launched."""
    sk = {"parents": [-1] + [(b - 1) // 2 for b in range(1, 33)]}
    tabs = syn.synthetic_motion_library(syn.make_generator(3), 2, 12, 20, humanoid=sk)
    lib = MotionLib.from_tables(tabs, dev)
    assert lib.num_bodies == 33
    n = 3
    out = _poisoned(n, 33, dev)
    with pytest.raises(_lib.PulseLibraryError, match=r"num_bodies 33 not in \[2,32\]"):
        _launch(lib, torch.zeros(n, dtype=torch.int64), torch.zeros(n), torch.ones(n, dtype=torch.bool), out, dev)
    torch.cuda.synchronize()
    _untouched(out, torch.arange(n, device=dev))


def test_wrapper_validates_its_tensors(dev):
    lib = MotionLib.from_tables(_tables(True), dev)
    n = 4
    ids, times, mask = torch.zeros(n, dtype=torch.int64), torch.zeros(n), torch.ones(n, dtype=torch.bool)
    out = _poisoned(n, 24, dev)
    with pytest.raises(ValueError, match="transform"):
        _launch(lib, ids, times, mask, out, dev, transform="spin")
    with pytest.raises(TypeError, match="new_root_xy"):
        _launch(lib, ids, times, mask, out, dev, transform="terrain")
    with pytest.raises(TypeError, match="sampled_ids"):
        _launch(lib, ids, times, mask, dict(out, sampled_ids=out["sampled_ids"].int()), dev)
    with pytest.raises(ValueError, match="dof_pos"):
        _launch(lib, ids, times, mask, dict(out, dof_pos=torch.zeros(n, 138, device=dev)[:, ::2]), dev)
    with pytest.raises(ValueError, match="start_times"):
        ops.task_ref_state_init(lib, ids.to(dev), times.to(dev), mask.to(dev), out["rb"], out["dof_pos"], out["dof_vel"], out["start_times"].cpu(),
                                out["sampled_ids"])
    # an id outside the library leaves its env untouched (the kernel never reads a table row it was not given)
    bad = torch.tensor([0, 5, -1, 1])
    _launch(lib, bad, times, mask, out, dev)
    _untouched(out, torch.tensor([1, 2], device=dev))
    assert not torch.isnan(out["rb"][[0, 3]]).any()
    assert np.isfinite(out["start_times"][[0, 3]].cpu().numpy()).all()
