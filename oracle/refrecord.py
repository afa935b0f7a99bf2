"""Record / replay of what the reference's own code computed inside a test.

The tests that pin the oracle to the reference's method bodies (oracle/refload.py) need the reference checkout, which only
the machine the project is developed on has.  Each such test names every value the reference side produces
(``R.t("reward/3", lambda: task.rew_buf)``) and runs the reference code only under ``if R.live:``:

  * live (checkout present): the reference code runs; the values are returned as computed and checked bit for bit against
    the stored vectors, so a stale fixture fails loudly.  PULSE_REF_RECORD=1 (re)writes the vectors instead;
  * replay (no checkout, or PULSE_REF_REPLAY=1): the values are read from tests/golden/ref/<module>/<test>.npz.

A large tensor that is only compared (``R.matches``) is stored as its digest and a seeded sample, which keeps the fixtures small.

The oracle side of every test runs in both modes on the same seeded inputs.  Live, both sides run in one process and are
compared bit for bit (``R.equal``).  Replayed, the oracle runs on another host than the one that recorded the reference, and
torch's CPU kernels differ in the last bits with the SIMD width they dispatch to (transcendentals, reduction order, GEMM
blocking): a floating-point tensor then agrees to REPLAY_RTOL of its largest magnitude (+ REPLAY_ATOL), integers and flags
still exactly.
"""
import hashlib
import json
import os
import re

import numpy as np
import torch

from . import refload

GOLDEN_REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ref")


REPLAY_RTOL, REPLAY_ATOL = 3e-5, 1e-6
SAMPLE = 8192                      # elements of a large compared tensor that are stored beside its digest (RefRecord.matches)


def close_across_hosts(a, b):
    """A CPU oracle result against a stored golden written on another host: integers / flags bit for bit, floating point to
    REPLAY_RTOL of the golden's largest magnitude (+ REPLAY_ATOL).  On the host that wrote the golden the two are equal."""
    a = torch.as_tensor(np.asarray(a)) if not isinstance(a, torch.Tensor) else a
    b = torch.as_tensor(np.asarray(b)) if not isinstance(b, torch.Tensor) else b
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point() or a.numel() == 0:
        return torch.equal(a, b)
    a, b = a.double(), b.double()
    return bool(torch.equal(a.isnan(), b.isnan()) and
                (a - b).nan_to_num().abs().max() <= REPLAY_RTOL * b.nan_to_num().abs().max() + REPLAY_ATOL)


def _sample_index(n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(0))[:SAMPLE].sort().values


def live():
    return refload.available() and not os.environ.get("PULSE_REF_REPLAY")


class RefRecord:
    def __init__(self, request):
        mod = request.node.module.__name__.split(".")[-1]
        name = re.sub(r"[^A-Za-z0-9_.\-]+", "_", request.node.name)
        self.path = os.path.join(GOLDEN_REF, mod, name + ".npz")
        self.live = live()
        self.rec = {}
        if not self.live:
            assert os.path.exists(self.path), f"no recorded reference values at {self.path} (record them with PULSE_REF_RECORD=1 where the reference is present)"
            with np.load(self.path, allow_pickle=False) as z:
                self.stored = {k: z[k] for k in z.files}

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None and self.live:
            self._close()
        return False

    def close(self):
        self.__exit__(None, None, None)

    def equal(self, a, b):
        """Bit for bit when live; to the cross-host floor when replayed (floating point only)."""
        if self.live or not (a.is_floating_point() or b.is_floating_point()):
            return torch.equal(a, b)
        return close_across_hosts(a, b)

    def t(self, key, fn):
        """A tensor the reference computed: ``fn()`` when live, the stored copy otherwise."""
        assert "\0" not in key and key not in self.rec, key
        if self.live:
            v = fn()
            v = v.detach().cpu().clone() if isinstance(v, torch.Tensor) else torch.as_tensor(v)
            self.rec[key] = v
            return v
        self.rec[key] = None
        return torch.from_numpy(self.stored[key].copy())

    def matches(self, key, fn, got):
        """Does the oracle's ``got`` equal what the reference computes (``fn()``)?  Live: bit for bit on the whole tensor.  A tensor of
        more than SAMPLE elements is recorded as the SHA-256 of its bytes, its shape, its largest magnitude and a fixed, seeded sample
        of SAMPLE elements.  Replayed, ``got`` passes bit for bit on the digest or, on a host whose CPU kernels round differently, on
        the sample to the cross-host floor (scaled by the whole tensor's largest magnitude)."""
        got = got.detach().cpu().contiguous()
        small = key in self.stored if not self.live else None
        if self.live:
            want = fn().detach().cpu().contiguous()
            small = want.numel() <= SAMPLE
        if small:
            return self.equal(got, self.t(key, lambda: want))
        for part in ("#sha256", "#shape", "#maxabs", "#sample"):
            assert key + part not in self.rec, key
        if self.live:
            flat = want.reshape(-1)
            self.rec[key + "#sha256"] = np.array(hashlib.sha256(want.numpy().tobytes()).hexdigest())
            self.rec[key + "#shape"] = np.array(list(want.shape), dtype=np.int64)
            self.rec[key + "#maxabs"] = np.array(flat.double().nan_to_num().abs().max().item())
            self.rec[key + "#sample"] = flat[_sample_index(flat.numel())].numpy()
            return torch.equal(got, want)
        for part in ("#sha256", "#shape", "#maxabs", "#sample"):
            self.rec[key + part] = None
        st = self.stored
        if list(got.shape) != st[key + "#shape"].tolist() or got.numpy().dtype != st[key + "#sample"].dtype:
            return False
        if hashlib.sha256(got.numpy().tobytes()).hexdigest() == str(st[key + "#sha256"]):
            return True
        a, b = got.reshape(-1)[_sample_index(got.numel())], torch.from_numpy(st[key + "#sample"].copy())
        if not a.is_floating_point():
            return torch.equal(a, b)
        a, b = a.double(), b.double()
        return bool(torch.equal(a.isnan(), b.isnan()) and
                    (a - b).nan_to_num().abs().max() <= REPLAY_RTOL * float(st[key + "#maxabs"]) + REPLAY_ATOL)

    def obj(self, key, fn):
        """A JSON-representable value (numbers, strings, lists, dicts) the reference side produced."""
        assert key not in self.rec, key
        if self.live:
            v = fn()
            self.rec[key] = np.array(json.dumps(v, sort_keys=True))
            return v
        self.rec[key] = None
        return json.loads(str(self.stored[key]))

    def _close(self):
        arrays = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in self.rec.items()}
        if os.environ.get("PULSE_REF_RECORD"):
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            np.savez_compressed(self.path, **arrays)
            return
        assert os.path.exists(self.path), f"reference values not recorded yet: run with PULSE_REF_RECORD=1 ({self.path})"
        with np.load(self.path, allow_pickle=False) as z:
            assert set(z.files) == set(arrays), f"recorded keys differ: {sorted(set(z.files) ^ set(arrays))}"
            for k, a in arrays.items():
                s = z[k]
                assert s.dtype == a.dtype and s.shape == a.shape and np.array_equal(s, a, equal_nan=a.dtype.kind in "fc"), \
                    f"{self.path}::{k}: the reference computes something else than the recorded value"
