"""Which slerp branch a slow joint takes depends on the summation order of a dot product: the table of
profiles/motion_degenerate_branches.txt.  CPU only (numpy + torch CPU), no device involved.

    python tools/motion_degenerate_branches.py            # 200 000 random unit-quaternion pairs per half-angle, seed 5

For every half-angle h the pairs of oracle/degenerate_clips.py:draw_pairs (q0 uniform on the sphere, q1 = dq q0 with dq a rotation of
half-angle h about a uniform axis; fp64, rounded to fp32).  The fp32 dot product is formed in the orders of oracle/degenerate_clips.py:dot_forms (three association orders, torch.sum,
fp64 rounded to fp32) and the branch of the reference's slerp (q0 | midpoint | general) is taken from each.  Columns: the share of
pairs whose branch differs between the orders; the largest component of 0.5 (q1 - q0) among them (what two implementations then
differ by when one returns q0 and the other the midpoint); the share of pairs oracle/degenerate_clips.py:classify calls stable."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import degenerate_clips as D  # noqa: E402

HALF_ANGLES = (0.0, 1e-4, 3e-4, 5e-4, 6.5e-4, 7.5e-4, 8e-4, 8.5e-4, 9e-4, 1.2e-3, 1.5e-3, 2e-3)


def row(rng, n, h):
    q0, q1 = D.draw_pairs(rng, n, h)
    branches = np.stack([D.branch_of(c) for c in D.dot_forms(q0, q1)])
    differ = (branches != branches[0]).any(0)
    gap = float(np.abs(0.5 * (q1 - q0))[differ].max()) if differ.any() else 0.0
    stable, _ = D.classify(q0, q1)
    return float(differ.mean()), gap, float(stable.mean())


def main(n=200000, seed=5):
    rng = np.random.default_rng(seed)
    print(f"CPU, {n} pairs per row, seed {seed}")
    print("half-angle   branch differs between orders   max |0.5 (q1 - q0)| among them   stable by classify")
    for h in HALF_ANGLES:
        share, gap, stable = row(rng, n, h)
        print(f"{h:<12g} {100 * share:>10.4f} %                   {gap:>12.2e}                   {100 * stable:>8.2f} %")


if __name__ == "__main__":
    main()
