"""CPU: the host-only workspace queries s3od_linear_wgrad_ws / s3od_conv_wgrad_ws answer from the same route functions
the weight-gradient entries switch on (linear_wgrad_route in csrc/linear_ops.hip, conv_wgrad_route in csrc/conv_ops.hip),
so their bytes pin the routing without a GPU.  The table below was recorded from the library before the dispatch was
split out of the kernels' file; a refactor of the routing must reproduce it.  The knob cases run in a child process with
S3OD_AB=1 (knobs re-read per call, csrc/common.hpp); the default row also runs in a child without it (read once)."""
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
F32, BF16 = 0, 1

# (dtype, Nout, Kin, rows, split)
LINEAR = [
    (BF16, 3072, 768, 65616, 0),
    (BF16, 768, 3072, 65616, 0),
    (BF16, 2304, 768, 65616, 0),
    (BF16, 768, 768, 65616, 0),
    (BF16, 1024, 768, 65536, 0),
    (F32, 3072, 768, 65616, 0),
    (BF16, 3072, 768, 65616, 3),
]
# (dtype, B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, split)
CONV = [
    (BF16, 16, 256, 256, 256, 256, 256, 256, 3, 3, 1, 1, 0),
    (BF16, 16, 128, 128, 512, 128, 128, 256, 3, 3, 1, 1, 0),
    (BF16, 16, 64, 64, 1024, 64, 64, 256, 3, 3, 1, 1, 0),
    (BF16, 16, 64, 64, 256, 64, 64, 256, 3, 3, 1, 1, 0),
    (BF16, 16, 1024, 1024, 64, 1024, 1024, 64, 3, 3, 1, 1, 0),
    (BF16, 16, 1024, 1024, 64, 512, 512, 128, 4, 4, 2, 1, 0),
    (BF16, 1, 20, 64, 512, 20, 64, 256, 3, 3, 1, 1, 0),          # H % 8 != 0: the ping-pong path by default
    (F32, 16, 256, 256, 256, 256, 256, 256, 3, 3, 1, 1, 0),
    (BF16, 16, 256, 256, 256, 256, 256, 256, 3, 3, 1, 1, 3),
    (BF16, 1, 20, 64, 512, 20, 64, 256, 3, 3, 1, 1, 3),
]
ENVS = {
    "default": {},
    "dma0": {"S3OD_WGRAD_DMA": "0"},
    "dma0_slab0": {"S3OD_WGRAD_DMA": "0", "S3OD_WGRAD_SLAB": "0"},
    "dma0_pp0": {"S3OD_WGRAD_DMA": "0", "S3OD_WGRAD_PP": "0"},
}
KNOBS = sorted({k for e in ENVS.values() for k in e})

# bytes per case, in the order of LINEAR then CONV
EXPECTED = {
    "default": [66060288, 66060288, 63700992, 0, 0, 0, 28311552,
                0, 0, 0, 0, 0, 0, 9437184, 0, 0, 14155776],
    "dma0": [66060288, 66060288, 63700992, 0, 0, 0, 28311552,
             66060288, 66060288, 66060288, 0, 0, 0, 9437184, 0, 7077888, 14155776],
    "dma0_slab0": [0] * 17,
    "dma0_pp0": [66060288, 66060288, 63700992, 0, 0, 0, 28311552,
                 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
}

SCRIPT = r'''
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
from s3od_amd._lib import lib
spec = json.loads(sys.argv[2])
out = {}
for name, env in spec["envs"].items():
    for k in spec["knobs"]:
        os.environ.pop(k, None)
    os.environ.update(env)
    row = []
    nb = ctypes.c_long(-1)
    for c in spec["linear"]:
        lib()("s3od_linear_wgrad_ws", *c, ctypes.addressof(nb))
        row.append(nb.value)
    for c in spec["conv"]:
        lib()("s3od_conv_wgrad_ws", *c, ctypes.addressof(nb))
        row.append(nb.value)
    out[name] = row
print("ROUTES " + json.dumps(out))
'''


def _query(envs, ab):
    env = {k: v for k, v in os.environ.items() if k != "S3OD_AB" and k not in KNOBS}
    if ab:
        env["S3OD_AB"] = "1"
    spec = json.dumps({"envs": envs, "knobs": KNOBS, "linear": LINEAR, "conv": CONV})
    p = subprocess.run([sys.executable, "-c", SCRIPT, str(REPO), spec], env=env, check=True, capture_output=True,
                       text=True, timeout=240)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROUTES ")][-1]
    return json.loads(line[len("ROUTES "):])


def test_workspace_queries_per_knob():
    got = _query(ENVS, ab=True)
    for name in ENVS:
        print(name, got[name])
        assert got[name] == EXPECTED[name], (name, got[name])


def test_workspace_queries_read_once_default():
    got = _query({"default": {}}, ab=False)
    print(got["default"])
    assert got["default"] == EXPECTED["default"]
