"""Per-inference time of the SARNN step's two halves at 1024 envs, HIP kernels against the torch modules
(SARNN table).

    python scripts/prof_sarnn.py time [ncam]   # one JSON line: medians of 5 windows of 20 calls per
                                               # route, the routes alternated window by window
    rocprofv3 --pmc FETCH_SIZE -d <dir> -o run --output-format csv -- python scripts/prof_sarnn.py pmc
    rocprofv3 --pmc WRITE_SIZE -d <dir> -o run --output-format csv -- python scripts/prof_sarnn.py pmc
                                               # one counter per pass; three 256 MiB copies first, whose
                                               # known traffic gives the counters' units, then three calls
                                               # of each kernel
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robomanipbaselines_amd import kernels as K  # noqa: E402
from robomanipbaselines_amd.policy.sarnn.sarnn_model import SarnnModel  # noqa: E402

mode = sys.argv[1]
n, ncam, S, Kp, hd, sd = 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 1, 64, 5, 50, 7
torch.backends.cudnn.allow_tf32 = False
torch.backends.cuda.matmul.allow_tf32 = False
torch.backends.cudnn.benchmark = True
torch.manual_seed(0)
m = SarnnModel(sd, ncam, [S, S], Kp, hd).eval().requires_grad_(False).to("cuda:0")
images = torch.rand(n, ncam, 3, S, S, device="cuda:0")
state = torch.rand(n, sd, device="cuda:0")
h = torch.zeros(n, hd, device="cuda:0")
c = torch.zeros(n, hd, device="cuda:0")
packed = m._packed()
lin = m.state_decoder[0]
lw = (m.lstm.weight_ih, m.lstm.weight_hh, m.lstm.bias_ih, m.lstm.bias_hh, lin.weight, lin.bias)


def att_fused():
    return K.sarnn_attention(images, packed, m.temperature)


def att_torch():
    return m.attention_points(images)


keys = att_fused()
kv = keys.view(n, -1)


def lstm_fused():
    return K.sarnn_lstm_step(state, kv, h, c, *lw)


def lstm_torch():
    hn, cn = m.lstm(torch.cat([state, kv], dim=-1), (h, c))
    h.copy_(hn)
    c.copy_(cn)
    return lin(hn)


if mode == "pmc":
    buf = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device="cuda:0")  # 256 MiB
    for _ in range(3):
        buf.clone()
    for _ in range(3):
        att_fused()
        lstm_fused()
    torch.cuda.synchronize()
    sys.exit(0)

fns = {"attention_fused": att_fused, "attention_torch": att_torch, "lstm_fused": lstm_fused, "lstm_torch": lstm_torch}
with torch.no_grad():
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for rep in range(5):  # alternate the routes; 20 calls per timing window
        for name, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                f()
            e1.record()
            e1.synchronize()
            res[name].append(e0.elapsed_time(e1) / 20)
flop = 2 * 9 * (3 * 16 * 62 * 62 + 16 * 32 * 60 * 60 + 32 * Kp * 58 * 58) * n * ncam
out = {"n_env": n, "ncam": ncam, "S": S, "K": Kp, "attention_flop": flop,
       "attention_min_bytes": n * ncam * (3 * S * S * 4 + Kp * 2 * 4),
       "ms_per_call": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
                       for k, v in res.items()}}
out["attention_fused_tflops"] = flop / (out["ms_per_call"]["attention_fused"]["median"] * 1e-3) / 1e12
print(json.dumps(out), flush=True)
