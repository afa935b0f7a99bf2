"""The walkable map of the terrain task restated in numpy / torch: what tests/test_terrain_map_cpu.py holds to the reference's own method
bodies (Terrain.__init__, curiculum, randomized_terrain, sample_valid_locations; phc/env/tasks/humanoid_pedestrian_terrain.py:1114-1189,
1307-1471) and what tests/test_terrain_map_gpu.py holds the kernels of csrc/terrain_map.hip to.  CPU only; draws are arguments.

Also here: the recording stand-ins for the six isaacgym.terrain_utils generators that both sides of the CPU test are run with."""
import numpy as np
import torch
from scipy import ndimage

H_SCALE, V_SCALE = 0.1, 0.005


# ---------------------------------------------------------------------------------------------------------------- layout
class Sub:
    """What a generator is handed: a square int16 field and the two scales."""

    def __init__(self, name, width, length, vertical_scale, horizontal_scale):
        self.terrain_name, self.width, self.length = name, width, length
        self.vertical_scale, self.horizontal_scale = vertical_scale, horizontal_scale
        self.height_field_raw = np.zeros((width, length), dtype=np.int16)


def geometry(cfg, border_size=50):
    g = {"width_px": int(cfg["mapWidth"] / H_SCALE), "length_px": int(cfg["mapLength"] / H_SCALE), "border": int(border_size / H_SCALE)}
    g["tot_cols"] = int(cfg["numTerrains"] * g["width_px"]) + 2 * g["border"]
    g["tot_rows"] = int(cfg["numLevels"] * g["length_px"]) + 2 * g["border"]
    g["sample_extent_x"] = int((g["tot_rows"] - g["border"] * 2) * H_SCALE)
    g["sample_extent_y"] = int((g["tot_cols"] - g["border"] * 2) * H_SCALE)
    return g


def kind_of(choice, cum):
    """The if / elif chain over the cumulative proportions; a trailing '-' is the sign flip (slope) or stairs down."""
    table = [(cum[0], "smooth_slope", 0.05), (cum[1], "rough_slope", 0.15), (cum[3], "stairs", cum[2]), (cum[4], "discrete", None),
             (cum[5], "stepping", None), (cum[6], "poles", None)]
    for bound, kind, flip in table:
        if choice < bound:
            return kind + ("-" if flip is not None and choice < flip else "")
    return "flat"


def layout(cfg, gens, border_size=50, rng=None):
    """Heights, poles flags per tile, kinds and env origins of the curriculum (terrains outer, levels inner) or the randomized layout
    (row-major tiles, two uniform draws each)."""
    g = geometry(cfg, border_size)
    rows, cols, b, px = cfg["numLevels"], cfg["numTerrains"], g["border"], g["width_px"]
    assert g["length_px"] == px
    cum = [np.sum(cfg["terrainProportions"][:i + 1]) for i in range(len(cfg["terrainProportions"]))]
    if cfg["curriculum"]:
        order = [(i, j, j / cols, i / rows) for j in range(cols) for i in range(rows)]
    else:
        order = []
        for k in range(rows * cols):
            choice = rng.uniform(0, 1)
            order.append((k // cols, k % cols, choice, rng.uniform(0.1, 1)))
    heights = np.zeros((g["tot_rows"], g["tot_cols"]), dtype=np.int16)
    flags = np.zeros((rows, cols), dtype=np.uint8)
    kinds = [[None] * cols for _ in range(rows)]
    origins = np.zeros((rows, cols, 3))
    for i, j, choice, difficulty in order:
        sub = Sub("terrain", px, px, V_SCALE, H_SCALE)
        kind = kinds[i][j] = kind_of(choice, cum)
        sign = -1 if kind.endswith("-") else 1
        base = kind.rstrip("-")
        if base in ("smooth_slope", "rough_slope"):
            slope = difficulty * 0.7
            if sign < 0:
                slope *= -1
            gens["pyramid_sloped"](sub, slope=slope, platform_size=3.)
            if base == "rough_slope":
                gens["random_uniform"](sub, min_height=-0.1, max_height=0.1, step=0.025, downsampled_scale=0.2)
        elif base == "stairs":
            step_height = 0.05 + 0.175 * difficulty
            if sign < 0:
                step_height *= -1
            gens["pyramid_stairs"](sub, step_width=0.31, step_height=step_height, platform_size=3.)
        elif base == "discrete":
            gens["discrete_obstacles"](sub, 0.025 + difficulty * 0.15, 1., 2., 40, platform_size=3.)
        elif base == "stepping":
            gens["stepping_stones"](sub, stone_size=2 - 1.8 * difficulty, stone_distance=0.1, max_height=0., platform_size=3.)
        elif base == "poles":
            gens["poles"](terrain=sub, difficulty=difficulty)
            flags[i, j] = 1
        heights[b + i * px:b + (i + 1) * px, b + j * px:b + (j + 1) * px] = sub.height_field_raw
        lo, hi = int((cfg["mapLength"] / 2. - 1) / H_SCALE), int((cfg["mapLength"] / 2. + 1) / H_SCALE)
        lo_y, hi_y = int((cfg["mapWidth"] / 2. - 1) / H_SCALE), int((cfg["mapWidth"] / 2. + 1) / H_SCALE)
        origins[i, j] = [(i + 0.5) * cfg["mapLength"], (j + 0.5) * cfg["mapWidth"], np.max(sub.height_field_raw[lo:hi, lo_y:hi_y]) * V_SCALE]
    return dict(g, heights=heights, tile_flags=flags, kinds=kinds, env_origins=origins)


# ---------------------------------------------------------------------------------------------------------------- obstacle field
def obstacles(heights, tile_flags=None, border=0, length_px=1, width_px=1, mask=None):
    """(rows, cols) bool: the non-zero heights of the flagged tiles -- tile (i, j) covers rows border + i * length_px .., columns
    border + j * width_px .., cut off at the array's end; cells before the border or past the last tile belong to none -- or the caller's
    mask."""
    shape = heights.shape if heights is not None else mask.shape
    out = np.zeros(shape, dtype=bool)
    if tile_flags is not None:
        flags = np.asarray(tile_flags) != 0
        ti, tj = (np.arange(shape[0]) - border) // length_px, (np.arange(shape[1]) - border) // width_px
        in_r, in_c = (ti >= 0) & (ti < flags.shape[0]), (tj >= 0) & (tj < flags.shape[1])
        flagged = flags[np.clip(ti, 0, flags.shape[0] - 1)][:, np.clip(tj, 0, flags.shape[1] - 1)] & in_r[:, None] & in_c[None, :]
        out = flagged & (heights != 0)
    if mask is not None:
        out = out | (np.asarray(mask) != 0)
    return out


def walkable(obstacle, iterations=3):
    """ndimage.binary_dilation with its default cross and zero border (iterations < 1 would mean 'until nothing changes' to scipy)."""
    if iterations == 0:
        return obstacle.astype(np.uint8)
    return ndimage.binary_dilation(obstacle, iterations=iterations).astype(np.uint8)


def walkable_l1(obstacle, iterations):
    """The same field from its definition: some obstacle within L1 distance ``iterations``, inside the array."""
    r, c = obstacle.shape
    pad = np.zeros((r + 2 * iterations, c + 2 * iterations), dtype=bool)
    pad[iterations:iterations + r, iterations:iterations + c] = obstacle
    out = np.zeros((r, c), dtype=bool)
    for dr in range(-iterations, iterations + 1):
        for dc in range(-(iterations - abs(dr)), iterations - abs(dr) + 1):
            out |= pad[iterations + dr:iterations + dr + r, iterations + dc:iterations + dc + c]
    return out.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- valid cells
def valid_cells(walkable_field, border):
    """(coord_x_scale, coord_y_scale) float32 in torch.where's order, data-dependent bounds, float32 arithmetic: an int64 tensor times a
    Python float is a float32 product, a 0-dim float32 tensor minus a Python float rounds the float to float32 first."""
    w = torch.as_tensor(np.asarray(walkable_field))
    x, y = torch.where(w == 0)
    xs, ys = x * H_SCALE, y * H_SCALE
    if xs.numel() == 0:
        return xs, ys
    b = border * H_SCALE
    keep = (ys < ys.max() - b) & (xs < xs.max() - b) & (ys > ys.min() + b) & (xs > xs.min() + b)
    return xs[keep], ys[keep]


# ---------------------------------------------------------------------------------------------------------------- sampling
def sample_table(coord_x, coord_y, idx):
    return torch.stack([coord_x[idx], coord_y[idx]], dim=-1)


def sample_groups(extent_x, extent_y, u_cx, u_cy, u_dx, u_dy):
    """u_cx / u_cy (G,), u_dx / u_dy (G, P) uniforms; torch_rand_float(lo, hi) = (hi - lo) * u + lo.  -> (G * P, 2), env e = group e // P."""
    centres = torch.stack([(extent_x - 0.) * u_cx + 0., (extent_y - 0.) * u_cy + 0.], dim=-1)
    diffs = torch.stack([(8 - -8.) * u_dx + -8., (-8 - 8.) * u_dy + 8.], dim=-1)
    return (centres[:, None] + diffs).reshape(u_dx.numel(), -1)


# ---------------------------------------------------------------------------------------------------------------- generator stand-ins
def recording_generators(log):
    """The six generators as deterministic stand-ins that log what they were called with.  Every kind leaves non-zero heights; the poles put
    discs on the tile's corner and edges as well as inside it, so that the dilation has tile and map borders to cross."""
    def heights_of(sub, salt):
        w, l = sub.height_field_raw.shape
        r, c = np.meshgrid(np.arange(w), np.arange(l), indexing="ij")
        return ((r * 7 + c * 13 + salt * 29 + len(log)) % 41 - 9).astype(np.int16)

    def plain(key, salt):
        def gen(terrain, *args, **kw):
            log.append([key, [float(a) for a in args], {k: float(v) for k, v in sorted(kw.items())}])
            terrain.height_field_raw[:] = terrain.height_field_raw + heights_of(terrain, salt)
            return terrain
        return gen

    def poles(terrain, difficulty):
        log.append(["poles", [], {"difficulty": float(difficulty)}])
        w, l = terrain.height_field_raw.shape
        r, c = np.meshgrid(np.arange(w), np.arange(l), indexing="ij")
        k = len(log)
        for cr, cc, rad in ((0, 0, 2.5), (w - 1, (11 * k) % l, 1.5), ((17 * k) % w, l - 1, 3.0), (w // 3, (2 * l) // 3, 4.0), ((5 * k) % w, (3 * k) % l, 0.5)):
            terrain.height_field_raw[np.hypot(r - cr, c - cc) <= rad] = 300 + k
        return terrain

    gens = {k: plain(k, i) for i, k in enumerate(("pyramid_sloped", "random_uniform", "pyramid_stairs", "discrete_obstacles", "stepping_stones"))}
    gens["poles"] = poles
    return gens
