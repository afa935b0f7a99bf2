"""CPU: the hand-written model of the discriminator's update pass (tests/disc_update_model.py) against torch autograd on the oracle's
restatement of AMPAgent._disc_loss (create_graph=True), both in fp64; and AMPAgent._disc_info on the model's raw 20-float row."""
import types

import pytest
import torch

from oracle import agent_oracle as AO
from tests import disc_update_model as DM

UNITS, AMP_DIM = (64, 32), 70
COEFS = {"reg": 0.01, "pen": 5.0, "wd": 0.0001, "scale": 5.0}
GAP, REDRAWS = 2e-5, 40            # every pre-activation of the fp64 oracle at least GAP from zero, the seed redrawn at most REDRAWS times
RTOL = 1e-12                       # relative to the largest magnitude of the tensor compared


def _close(got, want, what):
    got, want = got.detach().double().reshape(-1), want.detach().double().reshape(-1)
    assert got.shape == want.shape, what
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= RTOL * scale, f"{what}: max err {err:.3e} at scale {scale:.3e}"


_CASES = {}


def _case(b):
    """(weights, rows, fp64 model with its own masks, oracle info, oracle parameter gradients of scale * disc_loss) -- computed once per b."""
    if b not in _CASES:
        w, rows, _ = DM.draw_case(b, AMP_DIM, UNITS, seed=b, gap=GAP, max_redraws=REDRAWS)
        model = DM.disc_update_model(w, rows, COEFS)
        ref = AO.OracleDisc(AMP_DIM, units=UNITS).double()
        ref.load_state_dict({k[len("a2c_network."):]: v.double() for k, v in DM.to_state_dict(w).items()})
        info = AO.oracle_disc_loss(ref, *(r.double() for r in rows), COEFS["reg"], COEFS["pen"], COEFS["wd"])
        (COEFS["scale"] * info["disc_loss"]).backward()
        grads = {k: dict(ref.named_parameters())[DM.REF_NAMES[k][len("a2c_network."):]].grad for k in DM.NAMES}
        _CASES[b] = (w, rows, model, info, grads)
    return _CASES[b]


def _oracle_reported(info):
    """The seven reported numbers.  The oracle takes its accuracies as fp32 means (``.float()``), whatever dtype it runs in: they are checked
    to be the fp32 value of the count ratio, and the ratio itself, taken from the oracle's logits in fp64, goes into the comparison."""
    acc = [(info["disc_agent_logit"] < 0).double().mean(), (info["disc_demo_logit"] > 0).double().mean()]
    for got, want in zip((info["disc_agent_acc"], info["disc_demo_acc"]), acc):
        assert got.dtype == torch.float32 and abs(got.item() - want.item()) <= 2.0 ** -24
    return torch.stack([info["disc_loss"].detach(), info["disc_grad_penalty"], info["disc_logit_loss"], acc[0], acc[1],
                        info["disc_agent_logit"].mean(), info["disc_demo_logit"].mean()])


@pytest.mark.parametrize("b", [1, 5, 37, 48, 96])
def test_model_matches_autograd_fp64(b):
    w, rows, model, info, grads = _case(b)
    assert min(model["pre1"].abs().min().item(), model["pre2"].abs().min().item()) >= GAP
    _close(model["logits"][:2 * b], info["disc_agent_logit"], "agent / replay logits")
    _close(model["logits"][2 * b:], info["disc_demo_logit"], "demo logits")
    for k in DM.NAMES:
        _close(model["grads"][k], grads[k], f"grad {k}")
    _close(model["penalty"], info["disc_grad_penalty"], "penalty")
    _close(model["sq"]["w3"], info["disc_logit_loss"], "logit loss")
    want = _oracle_reported(info)
    for i, name in enumerate(DM.REPORTED):
        _close(model["reported"][i], want[i], name)
    # the raw row is consistent with what the model reports from it
    assert torch.equal(model["raw"][:8], model["stats"]) and model["raw"][8] == model["penalty_sum"] and (model["raw"][15:] == 0).all()


@pytest.mark.parametrize("b", [1, 5, 37, 48, 96])
@pytest.mark.parametrize("wd", [0.0001, 0.0])
def test_disc_info_on_the_models_raw_row(b, wd):
    """AMPAgent._disc_info is the only place the reported numbers are put together on the device path: run it, as it stands, on the model's
    raw row (fp64, so the comparison keeps its 1e-12)."""
    from pulse_amd.learning.amp_agent import AMPAgent
    w, rows, model, info, _ = _case(b)
    if wd != COEFS["wd"]:
        ref = AO.OracleDisc(AMP_DIM, units=UNITS).double()
        ref.load_state_dict({k[len("a2c_network."):]: v.double() for k, v in DM.to_state_dict(w).items()})
        info = AO.oracle_disc_loss(ref, *(r.double() for r in rows), COEFS["reg"], COEFS["pen"], wd)
    ns = types.SimpleNamespace(_disc_logit_reg=COEFS["reg"], _disc_grad_penalty=COEFS["pen"], _disc_weight_decay=wd)
    raw = torch.stack([model["raw"], torch.zeros(20, dtype=torch.float64)])              # a second, empty row: the function works row by row
    out = AMPAgent._disc_info(ns, raw, b, out=torch.full((2, 7), float("nan"), dtype=torch.float64))
    want = _oracle_reported(info)
    for i, name in enumerate(DM.REPORTED):
        _close(out[0, i], want[i], name)
    assert (out[1] == 0).all()


def test_bf16_storage_mode_rounds_only_what_is_stored():
    """The second mode of the model: the quantities the device stores as (or hands on rounded to) bf16 are bf16 values, the gradients and the
    sums of squared parameters are not rounded."""
    w, rows, model, _, _ = _case(5)
    m16 = DM.disc_update_model(w, rows, COEFS, storage="bf16")
    for k in ("dlogits", "dg", "logits", "G"):
        assert torch.equal(DM.bf16_rne(m16[k]), m16[k]) and not torch.equal(DM.bf16_rne(model[k]), model[k]), k
    for k in ("W1", "W2", "w3", "b1", "b2"):                                 # gradients are fp32 sums: not bf16 values
        assert not torch.equal(DM.bf16_rne(m16["grads"][k]), m16["grads"][k]), k
    assert m16["sq"]["W1"] == model["sq"]["W1"] and torch.equal(m16["raw"][9:15], model["raw"][9:15])
    # rounding moves the result by about 2^-9 relative, not more than a few of them and not nothing
    for k in DM.NAMES:
        e = (m16["grads"][k] - model["grads"][k]).abs().max().item() / model["grads"][k].abs().max().item()
        assert 1e-6 < e < 5e-2, (k, e)


def test_summation_orders_agree_in_fp64_and_differ_in_fp32():
    w, rows, model, _, _ = _case(37)
    masks = (model["m1"], model["m2"])
    for name, mm in DM.SUM_ORDERS.items():
        m64 = DM.disc_update_model(w, rows, COEFS, masks=masks, mm=mm)
        for k in DM.NAMES:
            _close(m64["grads"][k], model["grads"][k], f"{name} grad {k}")
    a = DM.disc_update_model(w, rows, COEFS, masks=masks, dtype=torch.float32, mm=DM.mm_k_ascending)
    c = DM.disc_update_model(w, rows, COEFS, masks=masks, dtype=torch.float32, mm=DM.mm_eight_partials)
    assert a["grads"]["W1"].dtype == torch.float32 and not torch.equal(a["grads"]["W1"], c["grads"]["W1"])
    err = (a["grads"]["W1"].double() - model["grads"]["W1"]).abs().max().item()
    assert 0 < err <= 1e-4 * model["grads"]["W1"].abs().max().item()
