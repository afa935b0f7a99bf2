"""Generate tests/golden/env_amp_variants.npz: the reference's own AMP frame functions in every configured form.

    python tools/gen_golden_amp_variants.py [--out DIR]

Needs the reference tree (oracle/refload.py reads its functions at run time; nothing of its text is kept here).  The committed fixture
holds OUTPUTS only, each written by the reference's build_amp_observations_smpl / build_amp_observations_smpl_v2
(phc/env/tasks/humanoid_amp.py:925-969, 973-1017); the inputs are redrawn from the seed by ``inputs()`` (the tests call it too) and the
fixture carries their float64 sums, so a generator that draws other numbers is noticed.

Inputs (seed 7341): 37 envs of ``syn.rigid_body_state``; dofs as oracle/gen_golden.py:gen_env_amp draws them (0.7 N(0, 1), a zero exp-map
row and a 1e-6 one); key bodies [7, 3, 22, 17]; shapes (37, 17) = [gender, 16 N(0, 1)] with the gender alternating and limb rows (37, 10)
= 0.5 + U(0, 1), so every column of both is non-constant.

Variants (``VARIANTS``): {v1, v2} x {upright, not} x {all 23 joints with root height, the 19-joint subset without} with no rows, and v1
with the shape row, the limb row and both (upright and not) on the shipped shape-aware frame (19-joint subset with root height: 207 /
206 / 217 columns).

Layout: the variants' outputs side by side in ONE array ``frames`` (37, sum of widths), in the order of ``VARIANTS`` (``widths`` holds the
split; ``load()`` returns them by name).  The variants share their dof columns byte for byte, and side by side those repeats fall inside
the compressor's window: 49 KB instead of 418 KB for one array per variant.

The generator FAILS unless the fixture can tell a wrong kernel from a right one: every non-upright output differs from its upright twin in
the rotation, velocity and key-body columns of every env, and the extra columns of every v2 output are non-zero.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pulse_amd import synthetic as syn  # noqa: E402

SEED, N = 7341, 37
KEY = [7, 3, 22, 17]                                                # R_Ankle, L_Ankle, R_Wrist, L_Wrist (env_im.yaml:35)
JOINTS19 = [j for j in range(23) if j not in (3, 7, 17, 22)]        # drop toes / hands (dofs 9:12, 21:24, 51:54, 66:69)
SUBSET = [3 * j + k for j in JOINTS19 for k in range(3)]
MAX_BYTES = 400 * 1024


def _variants():
    out = {}
    for v in (1, 2):
        for up in (True, False):
            for full in (True, False):
                out[f"v{v}_{'up' if up else 'noup'}_{'full23_h' if full else 'sub19_noh'}"] = dict(
                    version=v, upright=up, subset=not full, height=full, shape=False, limb=False)
    for up in (True, False):
        for tag, (sh, lw) in (("shape", (True, False)), ("limb", (False, True)), ("both", (True, True))):
            out[f"v1_{'up' if up else 'noup'}_sub19_h_{tag}"] = dict(version=1, upright=up, subset=True, height=True, shape=sh, limb=lw)
    return out


VARIANTS = _variants()      # name -> dict(version, upright, subset, height, shape, limb)


def inputs(n=N, seed=SEED):
    """Everything one AMP frame reads, for n envs of the 24-body humanoid."""
    g = syn.make_generator(seed)
    rb = syn.rigid_body_state(g, n)
    dof_pos = torch.randn(n, 69, generator=g) * 0.7
    dof_pos[0, 0:3] = 0.0                                   # zero exp-map -> masked branch
    if n > 1:
        dof_pos[1, 3:6] = torch.tensor([0.0, 0.0, 1e-6])
    dof_vel = torch.randn(n, 69, generator=g)
    shapes = torch.cat([(torch.arange(n) % 2).float()[:, None], torch.randn(n, 16, generator=g)], dim=-1)
    limbs = torch.rand(n, 10, generator=g) + 0.5
    return {"rb": rb, "dof_pos": dof_pos, "dof_vel": dof_vel, "shapes": shapes, "limbs": limbs}


def input_sums(d):
    return {f"sum_{k}": v.double().sum() for k, v in d.items()}


def columns(spec, num_key=len(KEY)):
    """Column ranges of a variant's frame: dict name -> slice."""
    nj = len(JOINTS19) if spec["subset"] else 23
    h0 = 1 if spec["height"] else 0
    c = {"rot": slice(h0, h0 + 6), "vel": slice(h0 + 6, h0 + 9), "ang": slice(h0 + 9, h0 + 12)}
    key0 = h0 + 12 + 9 * nj
    c["key"] = slice(key0, key0 + 3 * num_key)
    end = key0 + 3 * num_key
    if spec["version"] == 2:
        c["key_vel"] = slice(end, end + 3 * num_key)
        end += 3 * num_key
    c["rows"] = slice(end, end + 11 * spec["shape"] + 10 * spec["limb"])
    c["width"] = end + 11 * spec["shape"] + 10 * spec["limb"]
    return c


def reference_functions():
    """build_amp_observations_smpl from oracle.refload's table; the v2 function is not in it: read from the reference tree with the same helpers."""
    from oracle import refload
    fn = dict(refload.env_functions())
    ns = refload._namespace()
    ns.update(fn)
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid_amp.py")
    for name, text in refload._extract(path, ["build_amp_observations_smpl_v2"]).items():
        exec(compile(text, f"<reference:{name}>", "exec"), ns)
        fn[name] = ns[name]
    return fn


def check_conditions(outs):
    """The conditions that keep the fixture from hiding a failure; AssertionError otherwise."""
    for name, spec in VARIANTS.items():
        c = columns(spec)
        assert outs[name].shape == (N, c["width"]), f"{name}: shape {tuple(outs[name].shape)}, expected width {c['width']}"
        if not spec["upright"]:
            twin = outs[name.replace("_noup_", "_up_")]
            for part in ("rot", "vel", "ang", "key") + (("key_vel",) if spec["version"] == 2 else ()):
                same = (outs[name][:, c[part]] == twin[:, c[part]]).all(dim=-1)
                assert not same.any(), f"{name}: the {part} columns of env(s) {torch.where(same)[0].tolist()} equal the upright twin's"
        if spec["version"] == 2:
            assert (outs[name][:, c["key_vel"]] != 0).all(), f"{name}: a key-body velocity column is zero"


def generate():
    fn = reference_functions()
    d = inputs()
    rb = d["rb"]
    bp, br, bv, ba = rb[..., 0:3], rb[..., 3:7], rb[..., 7:10], rb[..., 10:13]
    subset, none_subset = torch.tensor(SUBSET, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    outs = {}
    for name, s in VARIANTS.items():
        tail = (subset if s["subset"] else none_subset, True, s["height"], s["subset"], s["shape"], s["limb"], s["upright"])
        if s["version"] == 1:              # the caller truncates the shapes for v1 (humanoid_amp.py:672)
            outs[name] = fn["build_amp_observations_smpl"](bp[:, 0], br[:, 0], bv[:, 0], ba[:, 0], d["dof_pos"], d["dof_vel"], bp[:, KEY],
                                                           d["shapes"][:, :-6], d["limbs"], *tail)
        else:
            outs[name] = fn["build_amp_observations_smpl_v2"](bp[:, 0], br[:, 0], bv[:, 0], ba[:, 0], d["dof_pos"], d["dof_vel"], bp[:, KEY], bv[:, KEY],
                                                              d["shapes"], d["limbs"], *tail)
    check_conditions(outs)
    packed = {"frames": torch.cat([outs[k] for k in VARIANTS], dim=-1), "widths": torch.tensor([outs[k].shape[1] for k in VARIANTS])}
    packed.update(input_sums(d))
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in packed.items()}


def load(path=None):
    """The fixture as {variant name: (37, W) array, 'sum_*': float64}."""
    z = np.load(path or os.path.join(ROOT, "tests", "golden", "env_amp_variants.npz"))
    widths = z["widths"].tolist()
    assert len(widths) == len(VARIANTS) and z["frames"].shape == (N, sum(widths))
    out = dict(zip(VARIANTS, np.split(z["frames"], np.cumsum(widths)[:-1], axis=1)))
    out.update({k: z[k] for k in z.files if k.startswith("sum_")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    path = os.path.join(a.out, "env_amp_variants.npz")
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay under {MAX_BYTES}"


if __name__ == "__main__":
    main()
