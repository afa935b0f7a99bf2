"""HumanoidImMCP on MI355X: the imitation env whose action is a weight vector over frozen PNN primitives (PHC's second training stage).

Mirrors phc/env/tasks/humanoid_im_mcp.py:13-93 (env files phc_kp_mcp_iccv.yaml, phc_shape_mcp_iccv.yaml, env_im_getup_mcp.yaml):
  __init__                    :15-32   num_prim (default 3), discrete_moe, has_pnn, has_lateral, z_activation (default "relu"); with has_pnn the
                                       ONE checkpoint of ``models`` gives the primitives (load_pnn) and the observation statistics
  _setup_character_props      :34-37   the action is the num_prim-wide weight vector
  get_task_obs_size_detail    :39-42   + num_prim (the amp_mcp network sizes its composer from it)
  step                        :44-71   obs -> clamp((obs - mean) / sqrt(var + 1e-5), +-5) -> primitives -> [one_hot(argmax) of the weights when
                                       discrete_moe] -> actions = sum_k weights[:, k, None] * x_k -> the ordinary step phases
``has_pnn: False`` reads ``self.actors`` (:65), which nothing in the reference defines: it raises here by name.
The primitives run as the frozen forward plan of learning/teacher.py (PnnTeacher without a composer); the normalisation is the
pulse_rms_normalize kernel and the mixture pulse_mcp_compose (csrc/mcp.hip).
"""
import torch

from .. import ops
from ..learning.teacher import PnnTeacher
from .humanoid_im import HumanoidIm, _env_dict, check_humanoid_options
from .humanoid_im_getup import HumanoidImGetup


def check_mcp_options(cfg, task="HumanoidImMCP"):
    """The MCP switches of an env dict; raises by name for what is not built.  Needs no device."""
    check_humanoid_options(cfg, task)                                           # SMPL-X / SMPL-H: the primitives are 24-body PHC policies
    env = _env_dict(cfg)
    opts = {"num_prim": int(env.get("num_prim", 3)), "discrete_moe": bool(env.get("discrete_moe", False)), "has_pnn": bool(env.get("has_pnn", False)),
            "has_lateral": bool(env.get("has_lateral", False)), "z_activation": env.get("z_activation", "relu")}
    if not opts["has_pnn"]:
        raise NotImplementedError(f"{task}: has_pnn = False is not built -- the reference's other branch mixes self.actors (humanoid_im_mcp.py:65), "
                                  "which nothing defines")
    if not 1 <= opts["num_prim"] <= 32:
        raise NotImplementedError(f"{task}: num_prim = {opts['num_prim']}: pulse_mcp_compose holds 1 .. 32 primitives")
    if opts["z_activation"] not in ("relu", "silu"):
        raise NotImplementedError(f"{task}: z_activation {opts['z_activation']!r}: relu / silu are built")
    return opts


class HumanoidImMCP(HumanoidIm):
    def __init__(self, cfg, sim, motion_lib, device="cuda:0", pnn_checkpoint=None):
        """``pnn_checkpoint``: the PNN checkpoint dict ({'model', 'running_mean_std'}) handed over directly, or a function of the constructed
        task that returns it; otherwise the one entry of env.models is loaded (a path, or the dict itself)."""
        opts = check_mcp_options(cfg, type(self).__name__)
        self.num_prim, self.discrete_mcp, self.has_pnn = opts["num_prim"], opts["discrete_moe"], opts["has_pnn"]
        self.has_lateral, self.z_activation = opts["has_lateral"], opts["z_activation"]
        if pnn_checkpoint is None:
            pnn_checkpoint = getattr(self, "_pnn_checkpoint_arg", None)
        super().__init__(cfg, sim, motion_lib, device=device)
        if callable(pnn_checkpoint):                                            # sized to the env: fn(task) -> checkpoint dict
            pnn_checkpoint = pnn_checkpoint(self)
        if pnn_checkpoint is None:
            if len(self.models_path) != 1:                                      # assert (len(self.models_path) == 1), :25
                raise ValueError(f"{type(self).__name__}: env.models must name exactly one PNN checkpoint, got {len(self.models_path)}")
            pnn_checkpoint = self.models_path[0]
            if not isinstance(pnn_checkpoint, dict):
                pnn_checkpoint = torch.load(pnn_checkpoint, map_location=self.device, weights_only=False)     # torch_ext.load_checkpoint, :26
        else:
            self.models_path = [pnn_checkpoint]                                 # (fitting: the agent takes the normaliser statistics from models[0])
        self._pnn = PnnTeacher(pnn_checkpoint, None, num_prim=self.num_prim, num_envs=self.num_envs, activation=self.z_activation,
                               has_lateral=self.has_lateral, device=self.device)
        if self._pnn.in_dim != self.num_obs or self._pnn.num_actions != self._dof_size:
            raise ValueError(f"{type(self).__name__}: the primitives map {self._pnn.in_dim} observations to {self._pnn.num_actions} actions, "
                             f"the env has {self.num_obs} and {self._dof_size}")
        self.running_mean, self.running_var = self._pnn.running_mean, self._pnn.running_var           # :28
        self._mcp_actions = torch.zeros(self.num_envs, self._dof_size, device=self.device)
        self.num_actions = self.num_prim                                        # _setup_character_props, :34-37

    def get_task_obs_size_detail(self):
        d = dict(super().get_task_obs_size_detail())
        d["num_prim"] = self.num_prim
        return d

    def compose_actions(self, weights):
        """:51-67 on the current observation buffer -> the (N, 69) joint targets (a persistent buffer)."""
        pnn = self._pnn
        pnn.normalize(self._obs_store)
        x_all = pnn.primitives()
        ops.mcp_compose(weights, x_all, self._mcp_actions, num_actions=self._dof_size, discrete=self.discrete_mcp)
        return self._mcp_actions

    def set_action_clip(self, clip):
        """The wrapper's clip_actions bounds the composer's weights, not the composed PD action: the clamp stays in the wrapper."""
        return False

    def step(self, weights):
        super().step(self.compose_actions(weights))


class HumanoidImMCPGetup(HumanoidImGetup, HumanoidImMCP):
    """phc/env/tasks/humanoid_im_mcp_getup.py: the get-up task's episode logic over the MCP step."""

    def __init__(self, cfg, sim, motion_lib, device="cuda:0", fall_state_source=None, pnn_checkpoint=None):
        check_mcp_options(cfg, type(self).__name__)
        self._pnn_checkpoint_arg = pnn_checkpoint                               # HumanoidImGetup.__init__ forwards the common arguments only
        super().__init__(cfg, sim, motion_lib, device=device, fall_state_source=fall_state_source)
