"""Terrain (phc/env/tasks/humanoid_pedestrian_terrain.py:1114-1189, 1307-1471): the map of the terrain task -- geometry, the tile layout of
the curriculum / the randomized layout, the obstacle field behind the 'poles' tiles, the table of valid start cells and the draw from it.

Host side: the layout loop (a few hundred tiles, once).  Device side (csrc/terrain_map.hip): the obstacle field and its dilation
(pulse_terrain_walkable), the valid-cell table (pulse_terrain_valid_cells) and the reset draw (pulse_terrain_sample).

Built: everything ``Terrain.__init__`` and ``sample_valid_locations`` compute, for generators the caller plugs in.  Not built:
  * the sub-terrain generators themselves -- ``isaacgym.terrain_utils`` is a closed third-party package; ``generators`` takes callables with
    its signatures (synthetic.synthetic_poles is a stand-in for ``poles_terrain``);
  * ``convert_heightfield_to_trimesh`` and anything PhysX (:1156): a height field is all the kernels read;
  * ``MeshTerrain`` (:975-1112, a scanned city mesh read from a pickle);
  * the ``flags.fixed`` / ``flags.server_mode`` placements of _reset_ref_state_init (:535-549).
"""
import types

import numpy as np
import torch

HORIZONTAL_SCALE, VERTICAL_SCALE = 0.1, 0.005                    # Terrain.__init__ :1121-1122
DILATION = 3                                                     # ndimage.binary_dilation(..., iterations=3), :1380 / :1471

# generator key -> the isaacgym.terrain_utils function it stands for and where the reference calls it (randomized_terrain / curiculum)
GENERATORS = {
    "pyramid_sloped": ("pyramid_sloped_terrain", ":1332, 1336, 1409, 1415"),
    "random_uniform": ("random_uniform_terrain", ":1337, 1418"),
    "pyramid_stairs": ("pyramid_stairs_terrain", ":1345, 1426"),
    "discrete_obstacles": ("discrete_obstacles_terrain", ":1350, 1431"),
    "stepping_stones": ("stepping_stones_terrain", ":1357, 1438"),
    "poles": ("poles_terrain", ":1363, 1444"),
}


class SubTerrain:
    """isaacgym.terrain_utils.SubTerrain as the generators see it: a (width, length) int16 height field and the two scales."""

    def __init__(self, terrain_name="terrain", width=256, length=256, vertical_scale=1.0, horizontal_scale=1.0):
        self.terrain_name = terrain_name
        self.vertical_scale, self.horizontal_scale = vertical_scale, horizontal_scale
        self.width, self.length = width, length
        self.height_field_raw = np.zeros((self.width, self.length), dtype=np.int16)


def tile_kind(choice, proportions):
    """(kind, flipped) of a tile from the cumulative ``proportions``, exactly as the if / elif chain of :1329-1368 / :1406-1449 reads them:
    ``flipped`` is the slope's sign flip (choice < 0.05 on a smooth slope, < 0.15 on a rough one) or stairs down (choice < proportions[2]).
    A choice past every proportion builds nothing: flat."""
    p = proportions
    if choice < p[0]:
        return "smooth_slope", bool(choice < 0.05)
    if choice < p[1]:
        return "rough_slope", bool(choice < 0.15)
    if choice < p[3]:
        return "stairs", bool(choice < p[2])
    if choice < p[4]:
        return "discrete", False
    if choice < p[5]:
        return "stepping", False
    if choice < p[6]:
        return "poles", False
    return "flat", False


def _generator(generators, key):
    fn = (generators or {}).get(key)
    if fn is None:
        name, lines = GENERATORS[key]
        raise NotImplementedError(f"Terrain: the layout selects a tile that needs generators[{key!r}] -- the reference calls isaacgym.terrain_utils."
                                  f"{name} there (phc/env/tasks/humanoid_pedestrian_terrain.py{lines}), a closed third-party package: pass a "
                                  "callable with its signature")
    return fn


def build_layout(cfg, num_robots, generators=None, rng=None, border_size=50.0):
    """Terrain.__init__ :1121-1153 with curiculum (:1382-1469) or randomized_terrain (:1307-1379), up to but not including the dilation.
    Returns what the loop leaves on the host as a namespace: the geometry under the reference's names, ``height_field_raw`` (tot_rows,
    tot_cols) int16, ``tile_flags`` (env_rows, env_cols) uint8 (1 = a poles tile), ``tile_kinds`` and ``env_origins`` (env_rows, env_cols,
    3) float64."""
    L = types.SimpleNamespace()
    L.horizontal_scale, L.vertical_scale, L.border_size = HORIZONTAL_SCALE, VERTICAL_SCALE, border_size
    L.env_length, L.env_width = cfg["mapLength"], cfg["mapWidth"]
    if L.env_length != L.env_width:
        raise ValueError(f"Terrain: mapLength {L.env_length} != mapWidth {L.env_width}: the reference builds square sub-terrains "
                         "(length=self.width_per_env_pixels, phc/env/tasks/humanoid_pedestrian_terrain.py:1320, 1390) and its own slice "
                         "assignment of them into the map fails otherwise")
    L.proportions = [np.sum(cfg["terrainProportions"][:i + 1]) for i in range(len(cfg["terrainProportions"]))]
    if len(L.proportions) < 7:
        raise ValueError(f"Terrain: terrainProportions needs at least 7 entries (smooth slope, rough slope, stairs up, stairs down, discrete, "
                         f"stepping, poles[, flat]), got {len(L.proportions)}")
    L.env_rows, L.env_cols = cfg["numLevels"], cfg["numTerrains"]
    L.num_maps = L.env_rows * L.env_cols
    L.env_origins = np.zeros((L.env_rows, L.env_cols, 3))
    L.width_per_env_pixels = int(L.env_width / L.horizontal_scale)
    L.length_per_env_pixels = int(L.env_length / L.horizontal_scale)
    L.border = int(L.border_size / L.horizontal_scale)
    L.tot_cols = int(L.env_cols * L.width_per_env_pixels) + 2 * L.border
    L.tot_rows = int(L.env_rows * L.length_per_env_pixels) + 2 * L.border
    L.height_field_raw = np.zeros((L.tot_rows, L.tot_cols), dtype=np.int16)
    L.tile_flags = np.zeros((L.env_rows, L.env_cols), dtype=np.uint8)
    L.tile_kinds = [[None] * L.env_cols for _ in range(L.env_rows)]
    L.sample_extent_x = int((L.tot_rows - L.border * 2) * L.horizontal_scale)
    L.sample_extent_y = int((L.tot_cols - L.border * 2) * L.horizontal_scale)
    L.curriculum = bool(cfg["curriculum"])
    if L.curriculum:
        # curiculum: terrains outer, levels inner (num_robots only splits robots over maps there, :1383-1384, 1454-1456: nothing reads it)
        tiles = [(i, j, j / L.env_cols, i / L.env_rows) for j in range(L.env_cols) for i in range(L.env_rows)]
    else:
        rng = np.random if rng is None else rng
        tiles = []
        for k in range(L.num_maps):
            i, j = np.unravel_index(k, (L.env_rows, L.env_cols))
            choice = rng.uniform(0, 1)
            tiles.append((int(i), int(j), choice, rng.uniform(0.1, 1)))
    for i, j, choice, difficulty in tiles:
        _build_tile(L, i, j, choice, difficulty, generators)
    return L


def _build_tile(L, i, j, choice, difficulty, generators):
    terrain = SubTerrain("terrain", width=L.width_per_env_pixels, length=L.width_per_env_pixels, vertical_scale=L.vertical_scale,
                         horizontal_scale=L.horizontal_scale)
    slope = difficulty * 0.7
    step_height = 0.05 + 0.175 * difficulty
    discrete_obstacles_height = 0.025 + difficulty * 0.15
    stepping_stones_size = 2 - 1.8 * difficulty
    kind, flipped = tile_kind(choice, L.proportions)
    if kind in ("smooth_slope", "rough_slope"):
        if flipped:
            slope *= -1
        _generator(generators, "pyramid_sloped")(terrain, slope=slope, platform_size=3.)
        if kind == "rough_slope":
            _generator(generators, "random_uniform")(terrain, min_height=-0.1, max_height=0.1, step=0.025, downsampled_scale=0.2)
    elif kind == "stairs":
        if flipped:
            step_height *= -1
        _generator(generators, "pyramid_stairs")(terrain, step_width=0.31, step_height=step_height, platform_size=3.)
    elif kind == "discrete":
        _generator(generators, "discrete_obstacles")(terrain, discrete_obstacles_height, 1., 2., 40, platform_size=3.)
    elif kind == "stepping":
        _generator(generators, "stepping_stones")(terrain, stone_size=stepping_stones_size, stone_distance=0.1, max_height=0., platform_size=3.)
    elif kind == "poles":
        _generator(generators, "poles")(terrain=terrain, difficulty=difficulty)
        L.tile_flags[i, j] = 1
    L.tile_kinds[i][j] = kind + ("-" if flipped else "")
    start_x = L.border + i * L.length_per_env_pixels
    end_x = L.border + (i + 1) * L.length_per_env_pixels
    start_y = L.border + j * L.width_per_env_pixels
    end_y = L.border + (j + 1) * L.width_per_env_pixels
    L.height_field_raw[start_x:end_x, start_y:end_y] = terrain.height_field_raw
    env_origin_x = (i + 0.5) * L.env_length                                               # :1372-1379 / :1458-1469
    env_origin_y = (j + 0.5) * L.env_width
    x1 = int((L.env_length / 2. - 1) / L.horizontal_scale)
    x2 = int((L.env_length / 2. + 1) / L.horizontal_scale)
    y1 = int((L.env_width / 2. - 1) / L.horizontal_scale)
    y2 = int((L.env_width / 2. + 1) / L.horizontal_scale)
    env_origin_z = np.max(terrain.height_field_raw[x1:x2, y1:y2]) * L.vertical_scale
    L.env_origins[i, j] = [env_origin_x, env_origin_y, env_origin_z]


def border_scaled(border, horizontal_scale=HORIZONTAL_SCALE):
    """``self.border * self.horizontal_scale`` (:1164-1165) as the reference's float32 comparison sees it: the double product rounded once."""
    return float(np.float32(border * horizontal_scale))


def check_height_field(height_field_raw, border, tile_flags, tile_shape, obstacle_mask):
    """The argument errors of Terrain.from_height_field, before anything touches a device.  Returns (tile_flags as a uint8 array or None,
    (length_px, width_px) or None)."""
    h = height_field_raw
    if not isinstance(h, (np.ndarray, torch.Tensor)) or h.ndim != 2 or str(h.dtype).split(".")[-1] != "int16":
        raise TypeError("Terrain.from_height_field: height_field_raw must be a (rows, cols) int16 array or tensor")
    if int(border) != border or border < 0:
        raise ValueError(f"Terrain.from_height_field: border must be a non-negative number of cells, got {border!r}")
    if tile_flags is None and obstacle_mask is None:
        raise ValueError("Terrain.from_height_field: tile_flags (with tile_shape) or obstacle_mask is required: without either no cell is an obstacle "
                         "and the walkable map has nothing to say")
    if obstacle_mask is not None and tuple(obstacle_mask.shape) != tuple(h.shape):
        raise ValueError(f"Terrain.from_height_field: obstacle_mask {tuple(obstacle_mask.shape)} is not the height field's shape {tuple(h.shape)}")
    if tile_flags is None:
        return None, None
    flags = np.ascontiguousarray(np.asarray(tile_flags.cpu() if isinstance(tile_flags, torch.Tensor) else tile_flags) != 0, dtype=np.uint8)
    if flags.ndim != 2 or tile_shape is None or len(tile_shape) != 2 or min(tile_shape) < 1:
        raise ValueError("Terrain.from_height_field: tile_flags must be (tile_rows, tile_cols) and come with tile_shape = (length_px, width_px)")
    need = (2 * border + flags.shape[0] * tile_shape[0], 2 * border + flags.shape[1] * tile_shape[1])
    if need != tuple(h.shape):
        raise ValueError(f"Terrain.from_height_field: {flags.shape[0]} x {flags.shape[1]} tiles of {tile_shape[0]} x {tile_shape[1]} cells inside a "
                         f"border of {border} make a {need[0]} x {need[1]} map, the height field is {h.shape[0]} x {h.shape[1]}")
    return flags, (int(tile_shape[0]), int(tile_shape[1]))


class Terrain:
    """The reference's Terrain on the device.  Attributes (the reference's names): ``heightsamples`` (tot_rows, tot_cols) int16,
    ``walkable_field`` uint8 (0 / 1), ``coord_x_scale`` / ``coord_y_scale`` (num_samples,) float32 in torch.where's order, ``num_samples``
    (a Python int, read back once here), ``border``, ``tot_rows`` / ``tot_cols``, ``sample_extent_x`` / ``_y``, ``horizontal_scale`` /
    ``vertical_scale`` and, from a config, ``env_origins``, ``width_per_env_pixels`` / ``length_per_env_pixels``, ``tile_kinds``."""

    @classmethod
    def from_config(cls, cfg_terrain, num_robots, generators, device, rng=None, border_size=50.0):
        """Terrain.__init__ (:1114-1172) for ``cfg_terrain`` (the env config's ``terrain`` block).  ``generators``: see GENERATORS; a tile
        kind the proportions select without one raises NotImplementedError, the flat kind needs none.  ``rng``: the source of the two
        uniform draws per tile of the randomized layout (default ``np.random``, as in the reference).  ``border_size``: the reference's
        constant 50 m; a keyword only so that kernel tests can use tiny maps."""
        if cfg_terrain.get("terrainType", "trimesh") in ("none", "plane"):
            raise ValueError(f"Terrain.from_config: terrainType {cfg_terrain['terrainType']!r} has no map (Terrain.__init__ returns before "
                             "building one, :1119-1120)")
        L = build_layout(cfg_terrain, num_robots, generators, rng=rng, border_size=border_size)
        self = cls(L.height_field_raw, L.border, L.tile_flags, (L.length_per_env_pixels, L.width_per_env_pixels), None, device)
        for k in ("env_origins", "width_per_env_pixels", "length_per_env_pixels", "tile_kinds", "env_rows", "env_cols", "env_length", "env_width",
                  "proportions", "border_size"):
            setattr(self, k, getattr(L, k))
        return self

    @classmethod
    def from_height_field(cls, height_field_raw, *, border, tile_flags=None, tile_shape=None, obstacle_mask=None, device):
        """For a caller who already has the int16 field (a real simulator's): obstacles are the non-zero cells of the tiles ``tile_flags``
        (tile_rows, tile_cols) marks -- tiles of ``tile_shape`` = (length_px, width_px) cells inside ``border`` cells of margin -- and / or
        the set cells of ``obstacle_mask`` (rows, cols), the caller's own field (before dilation)."""
        flags, shape = check_height_field(height_field_raw, border, tile_flags, tile_shape, obstacle_mask)
        return cls(height_field_raw, int(border), flags, shape, obstacle_mask, device)

    def __init__(self, height_field_raw, border, tile_flags, tile_shape, obstacle_mask, device):
        """The device side, from checked host arrays: use from_config or from_height_field."""
        from .. import ops
        self.device = device
        self.horizontal_scale, self.vertical_scale, self.border = HORIZONTAL_SCALE, VERTICAL_SCALE, border
        self.heightsamples = torch.as_tensor(height_field_raw).to(device).contiguous()
        self.tot_rows, self.tot_cols = self.heightsamples.shape
        self.sample_extent_x = int((self.tot_rows - border * 2) * self.horizontal_scale)          # :1157-1158
        self.sample_extent_y = int((self.tot_cols - border * 2) * self.horizontal_scale)
        kw = {}
        if tile_flags is not None:
            self.tile_flags = torch.as_tensor(tile_flags).to(device)
            kw.update(tile_flags=self.tile_flags, border=border, length_px=tile_shape[0], width_px=tile_shape[1])
        if obstacle_mask is not None:
            kw["obstacle_mask"] = (torch.as_tensor(obstacle_mask) != 0).to(device).contiguous()
        self.walkable_field = ops.terrain_walkable(self.heightsamples, iterations=DILATION, **kw)
        scales = dict(border_scaled=border_scaled(border, self.horizontal_scale), horizontal_scale=self.horizontal_scale)
        self.num_samples = int(ops.terrain_valid_cells(self.walkable_field, **scales)[2].item())  # count only; the one read-back
        if self.num_samples == 0:
            raise ValueError(f"Terrain: no valid start cell: of the {self.tot_rows} x {self.tot_cols} map nothing walkable lies more than the "
                             f"border ({border} cells) inside the walkable cells' extent (Terrain.__init__ :1160-1172 would leave an empty table "
                             "and np.random.randint(0, 0) raise at the first reset)")
        self.coord_x_scale, self.coord_y_scale = (torch.empty(self.num_samples, device=device) for _ in range(2))
        ops.terrain_valid_cells(self.walkable_field, coord_x=self.coord_x_scale, coord_y=self.coord_y_scale, **scales)
        self._draws = {}

    # ---- the draw
    def _buffers(self, n, p):
        """Persistent draw buffers for ``n`` envs: (N,) int64 indices, or one float32 block [centres (2, G) | x offsets (G, P) | y offsets]."""
        b = self._draws.get((n, p))
        if b is None:
            b = self._draws[(n, p)] = (torch.empty(2 * (n // p) + 2 * n, device=self.device) if p else
                                        torch.empty(n, dtype=torch.int64, device=self.device))
        return b

    def sample_into(self, out_xy, env_mask, generator, group_num_people=0):
        """The reset path: new locations for the envs of ``env_mask`` (N,) into ``out_xy`` (N, 2), the other rows untouched, nothing read
        back.  One fixed-size draw for all N envs into a persistent buffer -- ``torch.randint(0, num_samples)`` for np.random.randint (:1186),
        or one uniform block for the three torch_rand_float calls of the group mode (``group_num_people`` P > 0, :1176-1183) -- then
        pulse_terrain_sample.  The reference draws len(env_ids) values from numpy's global stream (torch's in group mode, and there for all
        envs): the RNG streams are not the reference's and never were comparable."""
        from .. import ops
        n, p = out_xy.shape[0], int(group_num_people)
        if p:
            if n % p != 0:
                raise ValueError(f"Terrain: {n} envs are not a multiple of group_num_people {p}: the reference's reshape of (num_groups, "
                                 "group_num_people, 2) to (max_num_envs, -1) (:1180) has no meaning there")
            g = n // p
            u = self._buffers(n, p).uniform_(generator=generator)
            return ops.terrain_sample(out_xy, env_mask=env_mask, group_num_people=p, extent_x=self.sample_extent_x, extent_y=self.sample_extent_y,
                                      u_center=u[:2 * g].view(2, g), u_dx=u[2 * g:2 * g + n].view(g, p), u_dy=u[2 * g + n:].view(g, p))
        idx = torch.randint(0, self.num_samples, (n,), generator=generator, out=self._buffers(n, 0))
        return ops.terrain_sample(out_xy, coord_x=self.coord_x_scale, coord_y=self.coord_y_scale, idx=idx, env_mask=env_mask)

    def sample_valid_locations(self, max_num_envs, env_ids, group_num_people=16, sample_groups=False, generator=None):
        """Terrain.sample_valid_locations (:1175-1189), for surface parity: (len(env_ids), 2) locations -- table rows, or with
        ``sample_groups`` the group formula for all ``max_num_envs`` envs indexed by ``env_ids`` (all when None).  Draws as sample_into."""
        if sample_groups:
            if max_num_envs % group_num_people != 0:
                raise ValueError(f"Terrain.sample_valid_locations: max_num_envs {max_num_envs} is not a multiple of group_num_people "
                                 f"{group_num_people} (the reshape of :1180)")
            out = torch.empty(max_num_envs, 2, device=self.device)
            self.sample_into(out, None, generator, group_num_people=group_num_people)
            return out if env_ids is None else out[env_ids]
        out = torch.empty(env_ids.shape[0], 2, device=self.device)
        return self.sample_into(out, None, generator)
