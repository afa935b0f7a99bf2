"""The host checks of the four normalising entries (csrc/rms_normalize.hip: the shared checks, the one wide-row predicate, each entry's own
extras) as ONE table of "refused or not", called through ctypes.  The expected letters are what the library returned before the entries shared
their checks: the plain entry falls back to the wide and narrow kernels where the others refuse, _b16 takes 8-byte aligned output rows, _planes
alone looks at the planes' pitch and _copy alone at raw_out.

Not marked gpu: without a device an accepted call gets as far as the launch and returns PULSE_ERR_LAUNCH, a refused one never touches the
device.  Where a device is present the buffers are device memory with room for every accepted shape, so an accepted call is a small valid
launch (a kernel handed host addresses would fault)."""
import pytest
import torch

from pulse_amd import _lib

OK, INVALID, LAUNCH = 0, -1, -2
ENTRIES = ("pulse_rms_normalize", "pulse_rms_normalize_copy", "pulse_rms_normalize_planes", "pulse_rms_normalize_b16")
BASE = dict(rows=4, cols=934, x_stride=960, y_stride=960, y_cols=960, num_blocks=1, null_x=False, x_off=0, y_off=0, raw_off=0, planes_ld=960)
# case, what differs from the 4 x 934 -> pitch 960 base, and per entry (plain, _copy, _planes, _b16): A accepted, R refused, 0 = empty problem (PULSE_OK)
CASES = [
    ("base shape", {}, "AAAA"),
    ("rows 0", dict(rows=0), "0000"),
    ("rows -1", dict(rows=-1), "RRRR"),
    ("null x", dict(null_x=True), "RRRR"),
    ("num_blocks 0", dict(num_blocks=0), "RRRR"),
    ("y_stride < y_cols", dict(y_stride=956), "RRRR"),
    ("cols 63", dict(cols=63), "ARRR"),
    ("x off by 4 bytes", dict(x_off=4), "ARRR"),
    ("y off by 4 bytes", dict(y_off=4), "ARRR"),
    ("y off by 8 bytes", dict(y_off=8), "ARRA"),
    ("x_stride 961", dict(x_stride=961), "ARRR"),
    ("y_cols 958", dict(y_cols=958), "ARRR"),
    ("y_cols 3104 with cols 3000", dict(cols=3000, x_stride=3104, y_stride=3104, y_cols=3104), "RRRR"),
    ("raw_out off by 4 bytes", dict(raw_off=4), "ARAA"),
    ("planes_ld 8", dict(planes_ld=8), "AARA"),
]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def bufs():
    """x, y, raw_out: 16384 floats each (4 rows of pitch 3104 and 12 bytes of offset fit); planes: 3 x 4 x 960 bf16 and the bf16 y; mean / var."""
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    b = {k: torch.zeros(16384, dtype=torch.float32, device=dev) for k in ("x", "y", "raw")}
    b["planes"] = torch.zeros(16384, dtype=torch.int16, device=dev)
    b["mean"] = torch.zeros(3072, dtype=torch.float64, device=dev)
    b["var"] = torch.ones(3072, dtype=torch.float64, device=dev)
    assert all(t.data_ptr() % 16 == 0 for t in b.values())
    return b


@pytest.mark.parametrize("name,change,expected", CASES, ids=[c[0] for c in CASES])
def test_normalising_entries_refuse_what_they_refused(lib, bufs, name, change, expected):
    c = dict(BASE, **change)
    x = None if c["null_x"] else bufs["x"].data_ptr() + c["x_off"]
    y = bufs["y"].data_ptr() + c["y_off"]
    head = (x, c["x_stride"], None, c["rows"], c["cols"], bufs["mean"].data_ptr(), bufs["var"].data_ptr(), 1e-5, 5.0)
    tail = (y, c["y_stride"], c["y_cols"], None, c["num_blocks"])
    calls = {
        "pulse_rms_normalize": lambda: lib.pulse_rms_normalize(*head, 0, *tail, None),
        "pulse_rms_normalize_copy": lambda: lib.pulse_rms_normalize_copy(*head, *tail, bufs["raw"].data_ptr() + c["raw_off"], 960, None),
        "pulse_rms_normalize_planes": lambda: lib.pulse_rms_normalize_planes(*head, *tail, bufs["planes"].data_ptr(), 4 * 960, c["planes_ld"], None),
        "pulse_rms_normalize_b16": lambda: lib.pulse_rms_normalize_b16(*head, *tail, None),
    }
    accepted = OK if torch.cuda.is_available() else LAUNCH
    for entry, want in zip(ENTRIES, expected):
        rc = calls[entry]()
        assert rc == {"A": accepted, "R": INVALID, "0": OK}[want], (name, entry, rc, lib.pulse_last_error())
        if want == "R":
            assert (entry + ":").encode() in lib.pulse_last_error(), (name, entry, lib.pulse_last_error())
    if torch.cuda.is_available():
        torch.cuda.synchronize()
