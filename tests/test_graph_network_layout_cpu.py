"""The graph-built policy networks (amp_z, amp_sept, amp_mcp) keep their parameter layout, names, launch graph and init order.

tests/golden/graph_network_layout.json was recorded by ``python tests/test_graph_network_layout_cpu.py --record`` at the commit BEFORE the
networks moved onto graph.GraphNetwork; this module only uses API both sides have.  Per network the fixture holds every Param
(name, rows, cols, off, pitch, colmap) in registration order, n_flat, the state_dict keys with shapes in order, and the ops of
``_build(8)["graph"]``.  The networks construct on the CPU without the HIP library (no plan is built here).
"""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from pulse_amd.learning.network_mcp import AMPMCPNetwork  # noqa: E402
from pulse_amd.learning.network_sept import AMPSeptNetwork  # noqa: E402
from pulse_amd.learning.network_z import AMPZNetwork  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_network_layout.json")
SPACE = {"continuous": {"sigma_init": {"name": "const_initializer", "val": -2.9}, "fixed_sigma": True}}


def _amp_z():
    p = {"name": "amp_z", "separate": True, "space": SPACE, "mlp": {"units": [48, 32], "activation": "silu"},
         "task_mlp": {"units": [40, 24], "activation": "silu"}}
    return AMPZNetwork(p, actions_num=69, self_obs_size=358, task_obs_size=576, device="cpu",
                       task_obs_size_detail={"embedding_size": 32, "z_type": "vae", "use_vae_prior": True, "use_vae_clamped_prior": True,
                                             "vae_var_clamp_max": 2})


def _amp_sept():
    p = {"name": "amp_sept", "separate": True, "space": SPACE, "mlp": {"units": [48, 32], "activation": "silu"},
         "task_mlp": {"units": [40, 24], "activation": "silu"}}
    return AMPSeptNetwork(p, actions_num=32, self_obs_size=358, task_obs_size=1044, task_obs_size_detail={"traj": 20, "heightmap": 1024},
                          device="cpu")


def _amp_mcp(has_softmax, activation):
    p = {"name": "amp_mcp", "separate": True, "space": SPACE, "mlp": {"units": [96, 64], "activation": activation}, "has_softmax": has_softmax}
    return AMPMCPNetwork(p, actions_num=4, self_obs_size=358, task_obs_size=576, task_obs_size_detail={"num_prim": 4}, device="cpu")


CASES = {"amp_z": _amp_z, "amp_sept": _amp_sept, "amp_mcp_softmax_relu": lambda: _amp_mcp(True, "relu"),
         "amp_mcp_plain_silu": lambda: _amp_mcp(False, "silu")}


def describe(net):
    """What the fixture holds for one network, in JSON's own types (tuples become lists)."""
    book = net.book
    out = {"params": [[p.name, p.rows, p.cols, p.off, p.pitch, p.colmap] for p in book.params.values()], "n_flat": book.n_flat,
           "state_dict": [[k, list(v.shape)] for k, v in net.state_dict().items()],
           "ops": [[op["lin"].name, op["src"], op["dst"], op["src_col"], op["dst_col"], op["grad_ranges"], op["tag"]]
                   for op in net._build(8)["graph"].ops]}
    return json.loads(json.dumps(out))


@pytest.fixture(scope="module")
def layout():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    return request.param, CASES[request.param]()


def test_layout_names_and_ops_match_the_recording(case, layout):
    name, net = case
    got, want = describe(net), layout[name]
    assert got["params"] == want["params"]
    assert got["n_flat"] == want["n_flat"]
    assert got["state_dict"] == want["state_dict"]
    assert got["ops"] == want["ops"]


def test_reset_parameters_draws_in_registration_order(case, layout):
    """nn.Linear's default init per layer -- kaiming_uniform_(a = sqrt 5) on empty(out, in), then the bias draw (discarded: biases are
    zeroed) -- in the fixture's parameter order, from one generator: any other order gives other weights."""
    name, net = case
    net.reset_parameters(torch.Generator().manual_seed(7))
    gen = torch.Generator().manual_seed(7)
    seen = 0
    for pname, rows, cols, *_ in layout[name]["params"]:
        if pname.endswith(".bias"):
            assert torch.count_nonzero(net.book.get(pname)) == 0, pname
            continue
        w = torch.empty(rows, cols)
        torch.nn.init.kaiming_uniform_(w, a=math.sqrt(5), generator=gen)
        torch.empty(rows).uniform_(-1 / math.sqrt(cols), 1 / math.sqrt(cols), generator=gen)
        assert torch.equal(net.book.get(pname), w), pname
        seen += 1
    assert seen == len(layout[name]["params"]) // 2


def test_state_dict_round_trip_is_bit_identical(case):
    name, net = case
    net.reset_parameters(torch.Generator().manual_seed(11))
    gen = torch.Generator().manual_seed(12)
    for p in net.book.params.values():
        if p.name.endswith(".bias"):
            net.book.set(p.name, torch.rand(p.cols, generator=gen))
    before = net.book.flat.clone()
    sd = net.state_dict()
    if name == "amp_z":                                         # the stacked heads travel as the reference's split keys
        assert "a2c_network.z_mu.weight" in sd and "a2c_network.z_prior_logvar.bias" in sd and "a2c_network.z_heads.weight" not in sd
    net.book.flat.zero_()
    net.load_state_dict(sd)
    assert torch.equal(net.book.flat, before)
    assert torch.count_nonzero(before) > 0


def test_strict_loading_names_the_missing_key(case):
    name, net = case
    sd = net.state_dict()
    missing = "a2c_network.z_mu.weight" if name == "amp_z" else "a2c_network.value.bias"
    del sd[missing]
    with pytest.raises(KeyError, match=missing.replace(".", r"\.")):
        net.load_state_dict(sd, strict=True)
    if name == "amp_z":                                         # (the halves of a stacked matrix come or go together)
        del sd["a2c_network.z_logvar.weight"]
    before = net.book.flat.clone()
    net.load_state_dict(sd, strict=False)
    assert torch.equal(net.book.flat, before)


def test_graphs_of_every_batch_size_share_one_flat_buffer(case):
    name, net = case
    ptr, n_flat, count = net.book.flat.data_ptr(), net.book.n_flat, len(net.book.params)
    a, b = net._build(8)["graph"], net._build(16)["graph"]
    assert a.book.flat.data_ptr() == b.book.flat.data_ptr() == net.book.flat.data_ptr() == ptr
    assert a.book.n_flat == b.book.n_flat == net.book.n_flat == n_flat and len(net.book.params) == count
    for op_a, op_b in zip(a.ops, b.ops):
        assert op_a["lin"].w is op_b["lin"].w is net.book.params[op_a["lin"].w.name]


def test_registering_a_known_name_with_another_shape_raises(case):
    name, net = case
    book = net.book
    p = book.params["a2c_network.value.weight"]
    assert book.add(p.name, p.rows, p.cols, p.colmap) is p
    for rows, cols, colmap, align in ((p.rows + 1, p.cols, None, 4), (p.rows, p.cols + 1, None, 4), (p.rows, p.cols, list(range(4, 4 + p.cols)), 4),
                                      (p.rows, p.cols, None, 128)):
        with pytest.raises(ValueError, match="a2c_network.value.weight"):
            book.add(p.name, rows, cols, colmap, pitch_align=align)
    assert book.n_flat == net.parameters_count() and book.params[p.name] is p


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_graph_network_layout_cpu.py --record")
    with open(GOLDEN, "w") as f:
        json.dump({k: describe(make()) for k, make in CASES.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
