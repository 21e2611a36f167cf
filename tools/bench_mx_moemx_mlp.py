#!/usr/bin/env python3
"""
Measure the whole MXFP4 expert MLP on the block-scaled MFMA (`moe_mlp_mxfp4_scaled`, libmbnb_moemx.so) in the same
process against (a) `moe_mlp_mxfp4` on its grouped route and (b) the route composed by hand from §34's projection: scaled gate / up
to bf16, the gated activation as torch ops, scaled down (which quantises T * A rows), a torch weighted sum.

Whole Python calls, bf16, top-k 4, H = I = 2880; the method of tools/bench_mx_moemx.py: events around `--steps` calls after
`--warmup`, the median of 5 repetitions and their spread.  Per shape also the relative Frobenius error of each route against the
f32 MLP over the dequantised weights, on the tokens whose slots all lie in the first experts.

One JSON line per (E, T), printed and written to `--out` (default profiles/moemx_mlp_bench.jsonl).

    python tools/bench_mx_moemx_mlp.py [--steps 20] [--warmup 5] [--tokens 256,1024,4096,8192] [--experts 32,128] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mps_bitsandbytes_amd import _moemx_native, functional as F, synthetic  # noqa: E402
from tools.bench_mx_moegemm import HIDDEN, INTER, SLOTS, time_us  # noqa: E402

ALPHA, LIMIT = 1.702, 7.0


def torch_glu(pre):
    g, u = pre[..., 0::2].float().clamp(max=LIMIT), pre[..., 1::2].float().clamp(-LIMIT, LIMIT)
    return (u + 1) * (g * torch.sigmoid(ALPHA * g))


def composed(x, gw, gs, dw, ds, ids, rw, fmt):
    """the route a caller of §34 composes by hand"""
    h = torch_glu(F.matmul_mxfp4_experts_scaled(x, gw, gs, ids, act_format=fmt)).to(x.dtype)
    y = F.matmul_mxfp4_experts_scaled(h, dw, ds, ids, dtype=torch.float32, act_format=fmt)
    return (y * rw.unsqueeze(-1)).sum(dim=1).to(x.dtype)


def rel_error(y, x, gw, gs, dw, ds, ids, rw, tokens=64):
    """|y - ref| / |ref| over the first `tokens` tokens; ref = the MLP in f32 over the dequantised weights"""
    num = den = 0.0
    for t in range(min(tokens, x.shape[0])):
        ref = torch.zeros(dw.shape[1], device=x.device)
        for a in range(ids.shape[1]):
            e = int(ids[t, a])
            h = torch_glu(x[t].float() @ F.dequantize_mx(gw[e], gs[e], "fp4", torch.float32).t())
            ref += rw[t, a] * (h @ F.dequantize_mx(dw[e], ds[e], "fp4", torch.float32).t())
        num += float((y[t].float() - ref).pow(2).sum())
        den += float(ref.pow(2).sum())
    return (num / den) ** 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tokens", default="256,1024,4096,8192", help="comma-separated T")
    ap.add_argument("--experts", default="32,128", help="comma-separated E")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moemx_mlp_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _moemx_native.lib()
    H, I, A = HIDDEN, INTER, SLOTS
    lines = []
    for E in (int(v) for v in args.experts.split(",")):
        gw, gs = F.quantize_mx(synthetic.normal_device((E * 2 * I, H), torch.bfloat16, seed=3 * E + 1, device=dev) * 0.02, "fp4")
        dw, ds = F.quantize_mx(synthetic.normal_device((E * H, I), torch.bfloat16, seed=3 * E + 2, device=dev) * 0.02, "fp4")
        gw, gs, dw, ds = gw.view(E, 2 * I, -1), gs.view(E, 2 * I, -1), dw.view(E, H, -1), ds.view(E, H, -1)
        for T in (int(v) for v in args.tokens.split(",")):
            rng = np.random.default_rng(1000 * E + T)
            ids = torch.from_numpy(np.stack([rng.permutation(E)[:A] for _ in range(T)]).astype(np.int32)).to(dev)
            rw = torch.softmax(synthetic.normal_device((T, A), torch.float32, seed=7, device=dev), dim=1)
            x = synthetic.normal_device((T, H), torch.bfloat16, seed=8, device=dev)
            flop = 2.0 * T * A * 3 * I * H
            line = {"E": E, "shape": [T, A, H, I], "pairs": T * A, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup}
            routes = {"grouped": lambda: F.moe_mlp_mxfp4(x, gw, gs, None, dw, ds, None, ids, rw)}
            for fmt in ("fp8", "fp4"):
                routes[f"composed_{fmt}"] = lambda fmt=fmt: composed(x, gw, gs, dw, ds, ids, rw, fmt)
                routes[f"scaled_{fmt}"] = lambda fmt=fmt: F.moe_mlp_mxfp4_scaled(x, gw, gs, None, dw, ds, None, ids, rw, act_format=fmt)
            with torch.no_grad():
                for name, fn in routes.items():
                    us, spread = time_us(fn, args.steps, args.warmup)
                    line[name] = {"us": round(us, 1), "tflops": round(flop / us * 1e-6, 1), "spread": round(spread, 3),
                                  "rel_error": round(rel_error(fn(), x, gw, gs, dw, ds, ids, rw), 4)}
            for fmt in ("fp8", "fp4"):
                line[f"scaled_{fmt}"]["to_grouped"] = round(line[f"scaled_{fmt}"]["us"] / line["grouped"]["us"], 3)
                line[f"scaled_{fmt}"]["to_composed"] = round(line[f"scaled_{fmt}"]["us"] / line[f"composed_{fmt}"]["us"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
        del gw, gs, dw, ds
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
