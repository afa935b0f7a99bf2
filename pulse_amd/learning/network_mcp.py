"""The MCP composer policy network (``network: amp_mcp``) on the gfx950 kernels.

Mirrors AMPMCPBuilder.Network, phc/learning/amp_network_mcp_builder.py:23-87 (registered at run_hydra.py:262; configs
phc/data/cfg/learning/im_mcp.yaml / im_mcp_big.yaml): PHC's second training stage, in which the policy emits ``num_prim`` mixture weights and
HumanoidImMCP.step (env/humanoid_im_mcp.py) blends the frozen PNN primitives with them.

  * ``AMPBuilder.Network.__init__`` runs first (:37) and creates actor_mlp, critic_mlp, value, mu, sigma (and the discriminator, which lives in
    learning/disc.py here); then the composer (:41-51): ``_build_mlp(units + [num_prim], activation)`` -- EVERY layer activated, the last one
    too -- and, when ``has_softmax`` (default True, :33; both shipped files say False), an ``nn.Softmax(dim=1)`` behind it (:53-55).
  * ``eval_actor`` (:64-86) is obs -> composer -> mu, sigma = the fixed ``sigma_init.val``.  ``actor_mlp`` and ``mu`` are therefore never
    evaluated: they are parameters of the checkpoint (created in the reference's order, carried through state_dict) that receive zero gradient
    and never move.  No launch touches them.
  * ``num_prim`` comes from ``task_obs_size_detail["num_prim"]``, default 4 (:39).
  * ``ending_act`` (im_mcp.yaml:16) is read by nothing in the reference (the composer's trailing activation is unconditional): ignored here too.
  * the critic is the plain critic MLP + value head (AMPBuilder.Network.eval_critic).

Backward: the critic like network_sept; the actor goes dmu -> pulse_mcp_head_backward (softmax backward when has_softmax, then the last
layer's activation derivative: graph.py fuses a derivative into the NEXT layer's input-gradient GEMM and the composer's last layer has none)
-> dz of the last Linear -> the composer's backward plan.
"""
import torch

from .. import kernels as K
from .._lib import ACT_RELU, ACT_SILU, ACT_SILU_D
from . import graph as G_
from .graph import GraphModel, GraphNetwork, Linear


def mcp_parameter_layout(units, num_prim, obs_size):
    """[(reference name, shape)] in the reference's creation order -- computable without a device (tests pin it against the torch twin)."""
    out = []
    for prefix in ("a2c_network.actor_mlp", "a2c_network.critic_mlp"):
        k = obs_size
        for i, u in enumerate(units):
            out += [(f"{prefix}.{2 * i}.weight", (u, k)), (f"{prefix}.{2 * i}.bias", (u,))]
            k = u
    out += [("a2c_network.value.weight", (1, units[-1])), ("a2c_network.value.bias", (1,)),
            ("a2c_network.mu.weight", (num_prim, units[-1])), ("a2c_network.mu.bias", (num_prim,))]
    k = obs_size
    for i, u in enumerate(list(units) + [num_prim]):
        out += [(f"a2c_network.composer.{2 * i}.weight", (u, k)), (f"a2c_network.composer.{2 * i}.bias", (u,))]
        k = u
    return out


class AMPMCPNetwork(GraphNetwork):
    def __init__(self, params, *, actions_num, self_obs_size, task_obs_size, task_obs_size_detail, device="cuda:0", split_k=8):
        d = dict(task_obs_size_detail or {})
        self.num_prim = int(d.get("num_prim", 4))                                     # :39
        if not 1 <= self.num_prim <= 32:
            raise NotImplementedError(f"amp_mcp with num_prim = {self.num_prim}: the composer head kernels hold 1 .. 32 primitives")
        if int(actions_num) != self.num_prim:
            raise ValueError(f"amp_mcp: the env's action is the {actions_num}-wide weight vector but task_obs_size_detail['num_prim'] = {self.num_prim} "
                             "(mu = the composer's output, amp_network_mcp_builder.py:81)")
        if not params["space"]["continuous"].get("fixed_sigma", True):
            raise NotImplementedError("amp_mcp with fixed_sigma: False (sigma(a_out), amp_network_mcp_builder.py:85; no shipped config)")
        self.has_softmax = bool(params.get("has_softmax", True))                      # :33
        # params["ending_act"]: read by nothing in the reference (the trailing activation is unconditional) -- ignored
        self.units = [int(u) for u in params["mlp"]["units"]]
        if params["mlp"]["activation"] not in ("relu", "silu"):
            raise NotImplementedError(f"amp_mcp activation {params['mlp']['activation']!r}: relu / silu are built")
        self.act = K.ACTIVATIONS[params["mlp"]["activation"]]
        super().__init__(params, actions_num=actions_num, self_obs_size=self_obs_size, task_obs_size=task_obs_size, device=device, split_k=split_k)

    def _build(self, m, x=None):
        U, P = self.units, self.num_prim
        g, book = self._new_graph(m, x), self.book
        lins = {}
        # AMPBuilder.Network order: actor_mlp, critic_mlp, value, mu (network_builder.py:245-261), then the composer (amp_network_mcp_builder.py:41-51).
        # actor_mlp and mu are parameters only: eval_actor (:64-86) never calls them, so they get no activation buffers and no launches
        k, lins["actor_mlp"] = self.obs_size, []
        for i, u in enumerate(U):
            lins["actor_mlp"].append(Linear(book, f"a2c_network.actor_mlp.{2 * i}", k, u, self.act))
            k = u
        names_c = [f"c{i + 1}" for i in range(len(U))]
        lins["critic_mlp"] = g.mlp("a2c_network.critic_mlp", "x", self.obs_size, U, self.act, names_c, tag="critic")
        g.buffer("value", 1)
        lins["value"] = g.linear(Linear(book, "a2c_network.value", U[-1], 1), names_c[-1], "value", grad_ranges=[(0, U[-1], self.act, names_c[-1], 0)], tag="critic")
        lins["mu"] = Linear(book, "a2c_network.mu", U[-1], P)
        # composer = Sequential(Linear, act, ..., Linear(units[-1], num_prim), act): the last layer is activated like the others
        names_p = [f"p{i + 1}" for i in range(len(U))] + ["h"]
        lins["composer"] = g.mlp("a2c_network.composer", "x", self.obs_size, U + [P], self.act, names_p, tag="composer")
        if self.has_softmax:
            g.buffer("mu", P)
        return {"graph": g, "lins": lins}

    def _plans(self, g):
        return {"fwd_actor": g.forward_plan({"composer"}), "fwd_critic": g.forward_plan({"critic"}),
                "bwd_actor": g.backward_plan({"composer"}), "bwd_critic": g.backward_plan({"critic"})}

    def unused_ranges(self):
        """Flat ranges of actor_mlp / mu: no pass writes their gradient slabs, the gradient reduce writes zeros there."""
        spans = []
        for lin in self.lins["actor_mlp"] + [self.lins["mu"]]:
            for p in (lin.w, lin.b):
                lo, hi = p.off, p.off + p.rows * p.pitch
                if spans and spans[-1][1] == lo:
                    spans[-1] = (spans[-1][0], hi)
                else:
                    spans.append((lo, hi))
        return spans


class AMPMCPModel(GraphModel):
    """The model interface CommonAgent / AMPAgent drive (workspace / forward / eval_critic / backward over one flat buffer)."""
    network = AMPMCPNetwork

    def _fill_workspace(self, ws, m):
        g, P = ws["g"], self.actions_num
        # without the softmax mu IS the composer's activated output (:81)
        ws["mu"] = g.act_bufs["mu" if self.net.has_softmax else "h"][:, :P]
        ws["dmu"] = torch.zeros(m, self.a_pitch, device=self.device)[:, :P]
        ws["unused"] = self.net.unused_ranges()

    def forward_actor(self, ws, m):
        ws["G"]["fwd_actor"].run()
        if self.net.has_softmax:
            g = ws["g"]
            K.mcp_head_forward(g.act_bufs["h"], g.act_bufs["mu"], rows=m, num_prim=self.actions_num)

    def forward(self, ws, m):
        self.forward_actor(ws, m)
        ws["G"]["fwd_critic"].run()

    def eval_critic(self, ws, m):
        ws["G"]["fwd_critic"].run()

    def backward(self, ws, m, grad_scale=1.0, sq_partials=None, on_bucket=None):
        """d loss / d (mu, value) are in ws['dmu'] / ws['dval'].  The composer's tail (softmax, last activation) is one launch that leaves
        d loss / d z of the last Linear where the backward plan reads it; actor_mlp / mu are in no plan and reduce to zero gradient."""
        net, g = self.net, ws["g"]
        act, aux = net.act, None
        if act == ACT_RELU:
            aux = g.act_bufs["h"]
        elif act == ACT_SILU:
            # a SiLU layer of a training pass keeps d silu / d z instead of z (graph.forward_plan, PULSE_SILU_DERIV)
            aux, act = g.pre("h"), (ACT_SILU_D if G_.SILU_DERIV else ACT_SILU)
        K.mcp_head_backward(ws["dmu"], g.grad("h"), rows=m, num_prim=self.actions_num, mu=g.act_bufs["mu"] if net.has_softmax else None,
                            aux=aux, activation=act)
        ws["G"]["bwd_actor"].run()
        ws["G"]["bwd_critic"].run()
        return self._reduce(grad_scale, ws["unused"], sq_partials)
