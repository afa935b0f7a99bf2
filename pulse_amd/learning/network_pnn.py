"""The PHC primitives' policy network (``network: amp_pnn``): ``num_prim`` progressive columns, ONE of which trains.

Mirrors AMPPNNBuilder.Network, phc/learning/amp_network_pnn_builder.py:25-89 (registered at run_hydra.py:261; config
phc/data/cfg/learning/im_pnn.yaml) over PNN, phc/learning/pnn.py:13-131 -- PHC's first training stage, whose checkpoint ``load_pnn``
(network_loader.py:54-73), learning/teacher.py and env/humanoid_im_mcp.py read:

  * ``AMPBuilder.Network.__init__`` runs first (:43) and creates actor_mlp, critic_mlp, value, mu, sigma; ``actor_mlp`` is then DELETED (:52);
    ``self.pnn = PNN(actor_mlp_args, output_size=actions_num, numCols=num_prim, has_lateral=...)`` and ``freeze_pnn(training_prim)`` follow.
  * ``eval_actor`` (:62-89) is ``mu = pnn(obs, idx=training_prim)[0]``, ``sigma = mu * 0 + sigma``.  ``a2c_network.mu`` is therefore never
    evaluated: it stays in the checkpoint (``load_pnn`` reads the action size off ``a2c_network.mu.bias``) and never moves.
  * a column is ``Sequential(Linear, act, ..., Linear(units[-1], actions))``.  Without laterals ``forward(x, idx)`` is ``actors[idx](x)``.  With
    laterals (pnn.py:85-124, two hidden layers only, :98) column c's second layer adds ``sum_{j<c} u[c-1][j][0](h1_j)`` in front of its activation:
    only the FIRST hidden activations of the earlier columns enter; ``u[..][1]`` is dead (:104-107); ``idx == 0`` is the plain column.
  * ``freeze_pnn(idx)`` (:41-46) clears requires_grad on ``actors[:idx]`` and ``u[:idx - 1]``.  The columns behind ``idx`` (and, through the slice's
    negative end, some lateral rows for idx 0) keep requires_grad but are not evaluated: no gradient reaches them and they do not move either.
  * the four switches reach the network through ``task_obs_size_detail`` (humanoid_im.py:503-506): num_prim 2, training_prim 1, actors_to_load 2,
    has_lateral True by default; every shipped env file says ``has_lateral: False``.  ``actors_to_load`` / ``models_path`` are read into
    attributes nothing uses (``load_base_net`` is commented out, :56).

Two paths:

  AMPPNNNetwork          no laterals (or column 0 with them): the trained column IS an actor MLP and the critic is the plain critic, so the class
                         is A2CNetwork with another checkpoint surface.  Column ``training_prim`` lives in the actor slots of the flat buffer
                         (hidden layers = ``actors.<k>.<2i>``, last Linear = the mu head slot): every launch plan -- the wide x3 tile, the batched
                         actor + critic layers, the skinny heads, ``mixed_precision`` on bf16 storage -- is A2CNetwork's own.  The other columns,
                         the lateral links and the reference's unused ``a2c_network.mu.*`` are carried OUTSIDE the flat buffer: no launch, no
                         Adam, no all-reduce touches them.
  AMPPNNLateralModel     ``has_lateral`` with ``training_prim`` >= 1, on graph.GraphNetwork / GraphModel with learning/teacher.py's layout: the first
                         layers of columns 0 .. k write side by side into one ``h1all`` buffer and column k's second layer is ONE GEMM over
                         [h1_0 .. h1_k] against [u[k-1][0] | .. | u[k-1][k-1] | W2_k].  The whole concatenated weight trains; of ``h1all`` only slice
                         k takes an input gradient; the earlier columns' first layers are forward-only; every other parameter sits in the flat
                         buffer with a zero gradient (``unused_ranges``, as amp_mcp keeps actor_mlp).  fp32 only.

Initialisation: both draw every tensor in the reference's construction order (actor_mlp drawn and dropped, critic_mlp, value, mu, then the
columns, then the lateral links) with the biases zeroed -- the columns' too, where the reference leaves nn.Linear's own bias draw on the PNN
(it is created after network_builder.py:273-277 ran) -- so a shared seed reproduces tests/pnn_model.py.
"""
import math
import re

import torch

from .. import kernels as K
from .graph import GraphModel, GraphNetwork, Linear
from .network import A2CNetwork

PNN_DEFAULTS = {"num_prim": 2, "training_prim": 1, "actors_to_load": 2, "has_lateral": True}          # humanoid_im.py:503-506


def pnn_options(env_cfg, detail=None):
    """``task_obs_size_detail`` as the reference's HumanoidIm hands it to the network: the four PNN keys read from ``cfg["env"]`` with the
    reference's defaults, merged over the task's own detail dict (which does not carry them: the env does not act on them)."""
    out = dict(detail or {})
    for k, default in PNN_DEFAULTS.items():
        out[k] = type(default)(env_cfg.get(k, default))
    return out


def check_pnn_options(params, detail, actions_num, env_actions=None, mixed_precision=False):
    """Validate by name, before anything is allocated.  Returns (num_prim, training_prim, has_lateral, lateral_path)."""
    d = pnn_options(detail or {})
    num_prim, training_prim, has_lateral = d["num_prim"], d["training_prim"], d["has_lateral"]
    if not 1 <= num_prim <= 32:
        raise NotImplementedError(f"amp_pnn with num_prim = {num_prim}: pulse_mcp_compose blends 1 .. 32 primitives")
    if not 0 <= training_prim < num_prim:
        raise ValueError(f"amp_pnn: training_prim = {training_prim} names no column of num_prim = {num_prim} (0 <= training_prim < num_prim)")
    if env_actions is not None and int(env_actions) != int(actions_num):
        raise ValueError(f"amp_pnn: actions_num = {actions_num} but the env's action is {env_actions} wide (a column's last Linear emits the env's action)")
    if not params["space"]["continuous"].get("fixed_sigma", True):
        raise NotImplementedError("amp_pnn with fixed_sigma: False (sigma(a_out), amp_network_pnn_builder.py:86; no shipped config)")
    units = [int(u) for u in params["mlp"]["units"]]
    if has_lateral and len(units) != 2:
        raise NotImplementedError(f"amp_pnn with has_lateral and {len(units)} hidden layers: lateral columns have exactly two (pnn.py:98)")
    lateral_path = has_lateral and training_prim > 0                  # idx == 0 is the plain column (pnn.py:88-90)
    if lateral_path and mixed_precision:
        raise NotImplementedError("amp_pnn: mixed_precision with has_lateral (training_prim >= 1): the lateral graph runs fp32; "
                                  "set mixed_precision: False or has_lateral: False")
    return num_prim, training_prim, has_lateral, lateral_path


def pnn_parameter_layout(units, num_prim, obs_size, actions_num, has_lateral=False):
    """[(reference name, shape)] in the reference's creation order -- computable without a device (tests pin it against the torch twin).
    No ``a2c_network.actor_mlp.*``: the reference deletes it (:52)."""
    units = [int(u) for u in units]
    out, k = [], obs_size
    for i, u in enumerate(units):
        out += [(f"a2c_network.critic_mlp.{2 * i}.weight", (u, k)), (f"a2c_network.critic_mlp.{2 * i}.bias", (u,))]
        k = u
    out += [("a2c_network.value.weight", (1, units[-1])), ("a2c_network.value.bias", (1,)),
            ("a2c_network.mu.weight", (actions_num, units[-1])), ("a2c_network.mu.bias", (actions_num,))]
    for c in range(num_prim):
        k = obs_size
        for i, u in enumerate(units + [actions_num]):
            out += [(f"a2c_network.pnn.actors.{c}.{2 * i}.weight", (u, k)), (f"a2c_network.pnn.actors.{c}.{2 * i}.bias", (u,))]
            k = u
    if has_lateral:                                                    # pnn.py:27-39: bias-free, u[i] holds i + 1 links
        for i in range(num_prim - 1):
            for j in range(i + 1):
                k = units[0]
                for l, u in enumerate(units[1:] + [actions_num]):
                    out.append((f"a2c_network.pnn.u.{i}.{j}.{l}.weight", (u, k)))
                    k = u
    return out


def _draw(units, num_prim, obs_size, actions_num, has_lateral, generator=None):
    """Every tensor of the layout, nn.Linear's default init drawn on the CPU in the reference's construction order, biases zeroed."""
    def lin(o, i, bias=True):
        w = torch.empty(o, i)
        torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5), generator=generator)
        if bias:
            bound = 1 / math.sqrt(i)
            torch.empty(o).uniform_(-bound, bound, generator=generator)            # nn.Linear draws its bias too
        return w
    k = obs_size
    for u in units:                                                                # actor_mlp: created first, deleted (:52)
        lin(u, k)
        k = u
    sd = {}
    for name, shape in pnn_parameter_layout(units, num_prim, obs_size, actions_num, has_lateral):
        if name.endswith(".bias"):
            sd[name] = torch.zeros(shape)
        else:
            sd[name] = lin(shape[0], shape[1], bias=".pnn.u." not in name)
    return sd


def _ordered(layout, get, sigma):
    sd = {}
    for name, _ in layout:
        sd[name] = get(name)
        if name == "a2c_network.mu.bias":
            sd["a2c_network.sigma"] = sigma.clone()                                 # network_builder.py:262-267: created behind mu
    return sd


class AMPPNNNetwork(A2CNetwork):
    """No laterals (or column 0): A2CNetwork's flat buffer and launch plans, the PNN's checkpoint surface."""

    def __init__(self, params, *, actions_num, input_shape, task_obs_size_detail=None, value_size=1, device="cuda:0", split_k=8):
        self.num_prim, self.training_prim, self.has_lateral, lateral = check_pnn_options(params, task_obs_size_detail, actions_num)
        if lateral:
            raise ValueError("amp_pnn: has_lateral with training_prim >= 1 is AMPPNNLateralModel's")
        self.carried = None            # reference name -> tensor: the columns that do not train, the lateral links, a2c_network.mu.* (checkpoint only)
        super().__init__(params, actions_num=actions_num, input_shape=input_shape, value_size=value_size, device=device, split_k=split_k)

    @property
    def layout(self):
        return pnn_parameter_layout(self.units, self.num_prim, self.in_dim, self.actions_num, self.has_lateral)

    def _flat_names(self, buf=None):
        """reference name -> view of the flat buffer: the critic, the value head, and column ``training_prim`` in the actor / mu-head slots."""
        flat = A2CNetwork.named_parameters(self, buf)
        t, L = self.training_prim, len(self.units)
        out = {k: v for k, v in flat.items() if ".critic_mlp." in k or ".value." in k}
        for p in ("weight", "bias"):
            for l in range(L):
                out[f"a2c_network.pnn.actors.{t}.{2 * l}.{p}"] = flat[f"a2c_network.actor_mlp.{2 * l}.{p}"]
            out[f"a2c_network.pnn.actors.{t}.{2 * L}.{p}"] = flat[f"a2c_network.mu.{p}"]
        return out

    def named_parameters(self, buf=None):
        """Reference names in the reference's order.  Of another buffer (the gradients) only the flat buffer's parameters exist."""
        own = self._flat_names(buf)
        if buf is not None and buf is not self.flat:
            return {k: own[k] for k, _ in self.layout if k in own}
        return {k: own[k] if k in own else self.carried[k] for k, _ in self.layout}

    def state_dict(self):
        p = self.named_parameters()
        return _ordered(self.layout, lambda k: p[k].clone(), self.sigma)

    def reset_parameters(self, generator=None):
        own = self._flat_names()
        if self.carried is None:
            self.carried = {k: torch.zeros(s, dtype=torch.float32, device=self.device) for k, s in self.layout if k not in own}
        self.flat.zero_()
        self.load_state_dict(_draw(self.units, self.num_prim, self.in_dim, self.actions_num, self.has_lateral, generator))
        si = self.space_config.get("sigma_init", {"name": "const_initializer", "val": 0.0})
        self.sigma.fill_(float(si.get("val", 0.0)))


def _spans(params):
    spans = []
    for p in sorted(params, key=lambda q: q.off):
        lo, hi = p.off, p.off + p.rows * p.pitch
        if spans and spans[-1][1] == lo:
            spans[-1] = (spans[-1][0], hi)
        else:
            spans.append((lo, hi))
    return spans


class AMPPNNLateralNetwork(GraphNetwork):
    """``has_lateral`` with ``training_prim`` >= 1.  Book parameters: the reference's names, except that column c's second layer and the lateral
    links into it are ONE matrix ``pnn_cat.<c>.weight`` = [u[c-1][0][0] | .. | u[c-1][c-1][0] | actors.<c>.2.weight] (bias = actors.<c>.2.bias);
    state_dict / load_state_dict split and join it."""

    def __init__(self, params, *, actions_num, self_obs_size, task_obs_size, task_obs_size_detail=None, device="cuda:0", split_k=8):
        self.num_prim, self.training_prim, self.has_lateral, lateral = check_pnn_options(params, task_obs_size_detail, actions_num)
        if not lateral:
            raise ValueError("amp_pnn without laterals (or with training_prim 0) is AMPPNNNetwork's")
        self.units = [int(u) for u in params["mlp"]["units"]]
        if self.units[0] % 4:
            raise NotImplementedError("amp_pnn with has_lateral: the first hidden width must be a multiple of 4 floats (the columns' slices of h1all)")
        if params["mlp"]["activation"] not in ("relu", "silu"):
            raise NotImplementedError(f"amp_pnn activation {params['mlp']['activation']!r}: relu / silu are built")
        self.act = K.ACTIVATIONS[params["mlp"]["activation"]]
        super().__init__(params, actions_num=actions_num, self_obs_size=self_obs_size, task_obs_size=task_obs_size, device=device, split_k=split_k)

    @property
    def layout(self):
        return pnn_parameter_layout(self.units, self.num_prim, self.obs_size, self.actions_num, True)

    def _build(self, m, x=None):
        (u0, u1), A, P, t, act = self.units, self.actions_num, self.num_prim, self.training_prim, self.act
        g, book = self._new_graph(m, x), self.book
        lins = {}
        names_c = ["c1", "c2"]
        lins["critic_mlp"] = g.mlp("a2c_network.critic_mlp", "x", self.obs_size, self.units, act, names_c, tag="critic")
        g.buffer("value", 1)
        lins["value"] = g.linear(Linear(book, "a2c_network.value", u1, 1), "c2", "value", grad_ranges=[(0, u1, act, "c2", 0)], tag="critic")
        lins["mu"] = Linear(book, "a2c_network.mu", u1, A)                         # never evaluated (:62-89)
        g.buffer("h1all", (t + 1) * u0)
        g.buffer("h2", u1)
        g.buffer("mu", A)
        lins["first"], lins["cat"], lins["last"] = [], [], []
        for c in range(P):
            # every column's first layer reads the observation; columns 0 .. t land in their slices of h1all, the ones behind t are not evaluated.
            # Columns < t are frozen: forward only
            lin = Linear(book, f"a2c_network.pnn.actors.{c}.0", self.obs_size, u0, act)
            lins["first"].append(lin)
            if c <= t:
                g.linear(lin, "x", "h1all", dst_col=c * u0, tag="actor" if c == t else "frozen")
        for c in range(P):
            cat = Linear(book, f"pnn_cat.{c}", (c + 1) * u0, u1, act)
            last = Linear(book, f"a2c_network.pnn.actors.{c}.4", u1, A)
            lins["cat"].append(cat)
            lins["last"].append(last)
            if c == t:
                # ONE GEMM over [h1_0 .. h1_t]; the whole concatenated weight trains, only slice t of h1all takes an input gradient
                g.linear(cat, "h1all", "h2", grad_ranges=[(t * u0, (t + 1) * u0, act, "h1all", 0)], tag="actor")
                g.linear(last, "h2", "mu", grad_ranges=[(0, u1, act, "h2", 0)], tag="actor")
        for i in range(P - 1):                                                      # the action-space links: dead in the reference (pnn.py:104-107), carried
            for j in range(i + 1):
                book.add(f"a2c_network.pnn.u.{i}.{j}.1.weight", A, u1)
        return {"graph": g, "lins": lins}

    def _plans(self, g):
        return {"fwd_actor": g.forward_plan({"frozen", "actor"}), "fwd_critic": g.forward_plan({"critic"}),
                "bwd_actor": g.backward_plan({"actor"}), "bwd_critic": g.backward_plan({"critic"})}

    def unused_ranges(self):
        """Flat ranges of everything no backward pass visits -- the frozen columns, the columns behind training_prim, their lateral links, the
        dead action-space links, a2c_network.mu: the gradient reduce writes zeros there."""
        t, L = self.training_prim, self.lins
        trained = L["critic_mlp"] + [L["value"], L["first"][t], L["cat"][t], L["last"][t]]
        names = {n for lin in trained for n in (lin.w.name, lin.b.name)}
        return _spans([p for p in self.book.params.values() if p.name not in names])

    # ------------------------------------------------------------------ reference names <-> book parameters
    def _view(self, name, buf=None):
        u0, b = self.units[0], self.book
        m = re.fullmatch(r"a2c_network\.pnn\.actors\.(\d+)\.2\.(weight|bias)", name)
        if m:
            c = int(m.group(1))
            return b.get(f"pnn_cat.{c}.weight", buf)[:, c * u0:(c + 1) * u0] if m.group(2) == "weight" else b.logical(f"pnn_cat.{c}.bias", buf)
        m = re.fullmatch(r"a2c_network\.pnn\.u\.(\d+)\.(\d+)\.0\.weight", name)
        if m:
            i, j = int(m.group(1)), int(m.group(2))
            return b.get(f"pnn_cat.{i + 1}.weight", buf)[:, j * u0:(j + 1) * u0]
        return b.logical(name, buf)

    def state_dict(self, buf=None):
        return _ordered(self.layout, lambda k: self._view(k, buf).clone(), self.sigma)

    def load_state_dict(self, sd, strict=True):
        for name, shape in self.layout:
            if name not in sd:
                if strict:
                    raise KeyError(name)
                continue
            if tuple(sd[name].shape) != tuple(shape):
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)} != {tuple(shape)}")
            self._view(name).copy_(sd[name].to(self.device, torch.float32))
        if "a2c_network.sigma" in sd:
            self.sigma.copy_(sd["a2c_network.sigma"].to(self.device, torch.float32))

    def reset_parameters(self, generator=None):
        self.book.flat.zero_()
        self.load_state_dict(_draw(self.units, self.num_prim, self.obs_size, self.actions_num, True, generator))


class AMPPNNLateralModel(GraphModel):
    """The model interface CommonAgent / AMPAgent drive (workspace / forward / eval_critic / backward over one flat buffer)."""
    network = AMPPNNLateralNetwork

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.num_prim, self.training_prim, self.has_lateral = self.net.num_prim, self.net.training_prim, True

    def _fill_workspace(self, ws, m):
        super()._fill_workspace(ws, m)
        ws["unused"] = self.net.unused_ranges()

    def forward(self, ws, m):
        ws["G"]["fwd_actor"].run()
        ws["G"]["fwd_critic"].run()

    def eval_critic(self, ws, m):
        ws["G"]["fwd_critic"].run()

    def backward(self, ws, m, grad_scale=1.0, sq_partials=None, on_bucket=None):
        """d loss / d (mu, value) are in ws['dmu'] / ws['dval'] (the graph's gradient buffers of its un-activated outputs)."""
        ws["G"]["bwd_actor"].run()
        ws["G"]["bwd_critic"].run()
        return self._reduce(grad_scale, ws["unused"], sq_partials)


def build_pnn_model(params, *, task, actions_num, input_shape, device, split_k=8, mixed_precision=False):
    """What CommonAgent._build_model resolves ``amp_pnn`` to.  Everything is validated by name before anything is allocated."""
    env = task.cfg.get("env", task.cfg)
    detail = pnn_options(env, task.get_task_obs_size_detail() if hasattr(task, "get_task_obs_size_detail") else {})
    _, _, _, lateral = check_pnn_options(params, detail, actions_num, env_actions=getattr(task, "num_actions", None), mixed_precision=mixed_precision)
    if lateral:
        return AMPPNNLateralModel(params, actions_num=actions_num, self_obs_size=task.get_self_obs_size(), task_obs_size=task.get_task_obs_size(),
                                  task_obs_size_detail=detail, device=device, split_k=split_k)
    return AMPPNNNetwork(params, actions_num=actions_num, input_shape=input_shape, task_obs_size_detail=detail, device=device, split_k=split_k)
