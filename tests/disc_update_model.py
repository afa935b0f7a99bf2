"""The discriminator's update pass written out by hand on the CPU, from the formulas of pulse_amd/learning/disc.py's module docstring:

    D(x) = w3 . relu(W2 relu(W1 x + b1) + b2) + b3
    loss = scale * (0.5 (BCE(D(agent U replay), 0) + BCE(D(demo), 1)) + reg ||w3||^2 + pen mean_demo ||dD/dx||^2
                    + wd (||W1||^2 + ||W2||^2 + ||w3||^2))

No autograd: the penalty's double backward is the mask-gated linear chain of the docstring.  The dtype, the matrix product (``mm``: its
summation order) and the two ReLU masks are parameters.  Masks are inputs because a pre-activation within fp32 round-off of zero flips a
ReLU on a correct kernel: a test hands the model the masks the device used and checks separately that they differ from the model's own only
where the pre-activation is that close to zero.

``storage="bf16"`` rounds to nearest even wherever the device's bf16-storage path stores bf16 -- X, the weights and their transposes, H1,
H2, Z1, Z2 (BCE and penalty rows alike), the logit gradients and dg -- and also the logits and G: they are stored as fp32, but an unsplit
GEMM on bf16 operands hands its output on rounded to bf16 (what an autocast Linear gives the next op) wherever it is stored.  Every
accumulation, the weight and bias gradients, the biases, the regulariser terms and the sums of squares stay in the model's dtype.
"""
import numpy as np
import torch

NAMES = ("W1", "b1", "W2", "b2", "w3", "b3")
REF_NAMES = {"W1": "a2c_network._disc_mlp.0.weight", "b1": "a2c_network._disc_mlp.0.bias", "W2": "a2c_network._disc_mlp.2.weight",
             "b2": "a2c_network._disc_mlp.2.bias", "w3": "a2c_network._disc_logits.weight", "b3": "a2c_network._disc_logits.bias"}
REPORTED = ("disc_loss", "disc_grad_penalty", "disc_logit_loss", "disc_agent_acc", "disc_demo_acc", "disc_agent_logit", "disc_demo_logit")


def bf16_rne(t):
    """Round to the nearest bf16 (ties to even), kept in t's dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def mm_torch(a, b):
    return a @ b


def mm_k_ascending(a, b):
    """sum_k a[:, k] b[k, :] with k ascending, one rounding per term."""
    if a.shape[0] == 1 and b.shape[1] == 1:                      # a dot product (sums of squares over whole matrices): numpy's accumulate
        prod = (a.reshape(-1) * b.reshape(-1)).numpy()           # adds strictly in order, in the array's own dtype
        return torch.from_numpy(np.add.accumulate(prod)[-1:].copy()).reshape(1, 1) if prod.size else torch.zeros(1, 1, dtype=a.dtype)
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
    for k in range(a.shape[1]):
        acc.addcmul_(a[:, k:k + 1], b[k:k + 1, :])
    return acc


def mm_eight_partials(a, b):
    """Eight contiguous k ranges summed on their own, then added in order: what a split-K launch with an ordered reduce does."""
    k = a.shape[1]
    step = max(1, -(-k // 8))
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
    for k0 in range(0, k, step):
        acc += a[:, k0:k0 + step] @ b[k0:k0 + step, :]
    return acc


SUM_ORDERS = {"torch": mm_torch, "k_ascending": mm_k_ascending, "eight_partials": mm_eight_partials}


def weights_from_state_dict(sd):
    """Reference-named tensors -> {W1 (u1, k0), b1 (u1,), W2 (u2, u1), b2 (u2,), w3 (1, u2), b3 (1,)}."""
    return {k: sd[REF_NAMES[k]].detach().clone().reshape(-1) if k.startswith("b") else sd[REF_NAMES[k]].detach().clone() for k in NAMES}


def disc_update_model(weights, rows, coefs, masks=None, dtype=torch.float64, storage="exact", mm=mm_torch):
    """weights: dict of NAMES; rows: (agent, replay, demo), each (b, k0); coefs: dict reg / pen / wd / scale (logit regulariser, gradient
    penalty, weight decay, disc_coef); masks: (m1 (3b, u1), m2 (3b, u2)) bool, or None for the model's own (pre-activation > 0).

    Returns a dict: logits (3b,), stats (8,), dlogits (3b,), G (b, k0), penalty_sum, penalty, dg (b, k0), grads {name: tensor, regulariser
    and weight decay included}, sq {W1, W2, w3: sums of squared weights}, raw (the 20-float row AMPAgent._disc_info reads), reported (7,),
    pre1 / pre2 (the pre-activations), m1 / m2 (the masks used)."""
    if storage not in ("exact", "bf16"):
        raise ValueError(storage)
    rnd = bf16_rne if storage == "bf16" else (lambda t: t)
    W = {k: weights[k].detach().to(dtype) for k in NAMES}
    W1, W2, w3 = W["W1"], W["W2"], W["w3"].reshape(1, -1)
    b1, b2, b3 = W["b1"].reshape(-1), W["b2"].reshape(-1), W["b3"].reshape(-1)
    W1s, W2s, w3s = rnd(W1), rnd(W2), rnd(w3)                 # what the GEMMs read; the regulariser reads the parameters themselves
    b = rows[0].shape[0]
    na, n = 2 * b, 3 * b
    reg, pen, wd, scale = (float(coefs[k]) for k in ("reg", "pen", "wd", "scale"))
    # every sum of the pass is a product with a vector of ones (or of a vector with itself), so that ``mm`` sets its order too
    colsum = lambda t: mm(torch.ones(1, t.shape[0], dtype=dtype), t.reshape(t.shape[0], -1)).reshape(-1)
    total = lambda t: colsum(t.reshape(-1, 1)).reshape(())
    sumsq = lambda t: mm(t.reshape(1, -1), t.reshape(-1, 1)).reshape(())
    X = rnd(torch.cat([r.detach().to(dtype) for r in rows], 0))
    # ---- forward over the 3b rows
    pre1 = mm(X, W1s.t().contiguous()) + b1
    m1 = (pre1 > 0) if masks is None else masks[0].bool()
    H1 = rnd(torch.where(m1, pre1, torch.zeros((), dtype=dtype)))
    pre2 = mm(H1, W2s.t().contiguous()) + b2
    m2 = (pre2 > 0) if masks is None else masks[1].bool()
    H2 = rnd(torch.where(m2, pre2, torch.zeros((), dtype=dtype)))
    logits = rnd(mm(H2, w3s.t().contiguous()) + b3).reshape(-1)
    # ---- head: prediction loss, its logit gradients, accuracies, logit means
    sp = torch.clamp(logits, min=0) + torch.log1p(torch.exp(-logits.abs()))          # softplus = BCEWithLogits(x, 0); BCE(x, 1) = softplus - x
    sg = torch.sigmoid(logits)
    la, ld = total(sp[:na]) / na, total(sp[na:] - logits[na:]) / b
    pred = 0.5 * (la + ld)
    stats = torch.stack([pred, la, ld, total((logits[:na] < 0).to(dtype)) / na, total((logits[na:] > 0).to(dtype)) / b, total(logits[:na]) / na,
                         total(logits[na:]) / b, torch.zeros((), dtype=dtype)])
    dl_exact = torch.cat([scale * 0.5 / na * sg[:na], scale * 0.5 / b * (sg[na:] - 1.0)])
    dl = rnd(dl_exact)
    # ---- BCE path over the 3b rows
    zero = torch.zeros((), dtype=dtype)
    Z2 = rnd(torch.where(m2, dl.reshape(-1, 1) * w3s, zero))
    Z1 = rnd(torch.where(m1, mm(Z2, W2s), zero))
    # ---- penalty forward on the demo rows: G = dD/dx
    m1d, m2d = m1[na:], m2[na:]
    u2 = rnd(torch.where(m2d, w3s.expand(b, -1), zero))
    u1 = rnd(torch.where(m1d, mm(u2, W2s), zero))
    G = rnd(mm(u1, W1s))
    pen_sum = sumsq(G)
    c = 2.0 * pen * scale / b
    dg = rnd(c * G)
    # ---- penalty backward
    dt1 = rnd(torch.where(m1d, mm(dg, W1s.t().contiguous()), zero))
    t2 = rnd(torch.where(m2d, mm(dt1, W2s.t().contiguous()), zero))
    # ---- weight gradients: both paths stacked along the batch dimension, rows [0, 3b) BCE, [3b, 4b) penalty
    ones = torch.ones(b, dtype=dtype)
    gW1 = mm(torch.cat([Z1, u1], 0).t().contiguous(), torch.cat([X, dg], 0))
    gW2 = mm(torch.cat([Z2, u2], 0).t().contiguous(), torch.cat([H1, dt1], 0))
    gw3 = mm(torch.cat([dl, ones], 0).reshape(1, -1), torch.cat([H2, t2], 0))
    grads = {"W1": gW1 + 2.0 * scale * wd * W1, "b1": colsum(Z1), "W2": gW2 + 2.0 * scale * wd * W2, "b2": colsum(Z2),
             "w3": gw3 + 2.0 * scale * (wd + reg) * w3, "b3": total(dl).reshape(1)}
    sq = {"W1": sumsq(W1), "W2": sumsq(W2), "w3": sumsq(w3)}
    raw = torch.zeros(20, dtype=dtype)
    raw[:8] = stats
    raw[8] = pen_sum
    raw[9], raw[10], raw[11], raw[12], raw[13], raw[14] = sq["W1"], sumsq(b1), sq["W2"], sumsq(b2), sq["w3"], sumsq(b3)
    penalty = pen_sum / b
    loss = pred + reg * sq["w3"] + pen * penalty
    if wd != 0:
        loss = loss + wd * (sq["W1"] + sq["W2"] + sq["w3"])
    reported = torch.stack([loss, penalty, sq["w3"], stats[3], stats[4], stats[5], stats[6]])
    return {"logits": logits, "stats": stats, "dlogits": dl, "G": G, "penalty_sum": pen_sum, "penalty": penalty, "dg": dg, "grads": grads, "sq": sq,
            "raw": raw, "reported": reported, "pre1": pre1, "pre2": pre2, "m1": m1, "m2": m2}


def draw_case(b, amp_dim, units, seed, gap=0.0, max_redraws=0):
    """Weights (nn.Linear's own init, w3 scaled by 0.2, b3 = 0.05, small nonzero b1 / b2) and three row blocks.  With ``gap`` > 0 the seed is
    redrawn, at most ``max_redraws`` times, until every pre-activation of the fp64 model is at least ``gap`` from zero.
    -> (weights (fp32 tensors), rows (fp32), redraws used)."""
    from oracle import agent_oracle as AO
    for attempt in range(max_redraws + 1):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        state = torch.random.get_rng_state()
        torch.manual_seed(seed + 1000 * attempt)
        ref = AO.OracleDisc(amp_dim, units=tuple(units))
        torch.random.set_rng_state(state)
        w = weights_from_state_dict(ref.state_dict_ref())
        w["w3"] = w["w3"] * 0.2
        w["b3"] = torch.full((1,), 0.05)
        w["b1"] = torch.randn(units[0], generator=g) * 0.05
        w["b2"] = torch.randn(units[1], generator=g) * 0.05
        rows = tuple(torch.randn(b, amp_dim, generator=g).clamp(-5, 5) for _ in range(3))
        if gap <= 0:
            return w, rows, attempt
        m = disc_update_model(w, rows, {"reg": 0.0, "pen": 0.0, "wd": 0.0, "scale": 1.0})
        if min(m["pre1"].abs().min().item(), m["pre2"].abs().min().item()) >= gap:
            return w, rows, attempt
    raise AssertionError(f"no draw with every pre-activation {gap:g} from zero in {max_redraws + 1} attempts (b = {b})")


def to_state_dict(weights):
    return {REF_NAMES[k]: weights[k].detach().clone().reshape(1, -1) if k == "w3" else weights[k].detach().clone() for k in NAMES}
