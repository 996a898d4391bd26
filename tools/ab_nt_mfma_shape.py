"""A/B of the two main loops of the persistent NT kernel's plain bf16-output launches (gemm_nt5.hip): ocn_set_gemm_variant NT value 6 =
v_mfma_f32_32x32x16_bf16, 7 = v_mfma_f32_16x16x32_bf16, interleaved in ONE process on the step's eight bf16-out shapes (ViT-B-32, local batch 4096,
packed text: the QKV projection and the three dgrads of each tower's blocks).  Random Gaussian operands (never zeros: the clock a power-limited loop
holds depends on the data); >= 2 s of back-to-back launches before the first sample of a shape, then alternating rounds of event-timed launches.
Per arm: median, min, max; the ratio of the medians counts as a difference only outside the larger of the two arms' min-max spreads.  One JSON
document on stdout:

    python tools/ab_nt_mfma_shape.py > nt5_mfma_shape_ab.json"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open_clip_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
Mi, Mt = 4096 * 50, 177803  # image rows; text rows of the packed tower at the bench's caption lengths
SHAPES = [  # (name, M, N, K, bias): out[M, N] = a[M, K] . b[N, K]^T
    ("img qkv", Mi, 2304, 768, True), ("img d c_fc", Mi, 768, 3072, False), ("img d out_proj", Mi, 768, 768, False), ("img d qkv", Mi, 768, 2304, False),
    ("txt qkv", Mt, 1536, 512, True), ("txt d c_fc", Mt, 512, 2048, False), ("txt d out_proj", Mt, 512, 512, False), ("txt d qkv", Mt, 512, 1536, False),
]
ARMS = (6, 7)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def ab(fn, launches, warm_s):
    """{arm: [ms, ...]} of ``launches`` event-timed launches per arm in alternating rounds of 4, behind ``warm_s`` seconds of alternating launches"""
    t0 = time.time()
    while time.time() - t0 < warm_s:
        for arm in ARMS:
            _lib.call("ocn_set_gemm_variant", arm)
            for _ in range(8):
                fn()
        torch.cuda.synchronize()
    ms = {arm: [] for arm in ARMS}
    for rnd in range((launches + 3) // 4):
        for arm in (ARMS if rnd % 2 == 0 else ARMS[::-1]):
            _lib.call("ocn_set_gemm_variant", arm)
            fn()  # (the first launch behind a switch is not a sample)
            ms[arm] += [event_ms(fn) for _ in range(4)]
    _lib.call("ocn_set_gemm_variant", 0)
    return ms


def summary(ms, flop):
    out = {}
    for arm, v in ms.items():
        med = statistics.median(v)
        out[f"v{arm}"] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v), "tflops": round(flop / med / 1e9, 1)}
    a, b = out["v6"], out["v7"]
    ratio = b["median_ms"] / a["median_ms"]
    spread = max((a["max_ms"] - a["min_ms"]) / a["median_ms"], (b["max_ms"] - b["min_ms"]) / b["median_ms"])
    out["ratio_v7_over_v6"] = round(ratio, 4)
    out["larger_spread"] = round(spread, 4)
    out["outside_spread"] = abs(ratio - 1.0) > spread
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warm", type=float, default=2.0)
    args = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "arms": {"v6": "32x32x16 main loop", "v7": "16x16x32 main loop"}, "launches_per_arm": args.launches,
           "warm_seconds": args.warm, "operands": "randn bf16", "shapes": {}}
    g = torch.Generator(device=dev).manual_seed(1)
    tot = {"v6": 0.0, "v7": 0.0}
    for name, M, N, K, bias in SHAPES:
        a, b = torch.randn(M, K, device=dev, generator=g).bfloat16(), torch.randn(N, K, device=dev, generator=g).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        bv = torch.randn(N, device=dev, generator=g) if bias else None
        fn = lambda: ops.gemm_nt(ops.EPI_BF16, a, b, out, bias=bv)  # noqa: E731
        r = summary(ab(fn, args.launches, args.warm), 2.0 * M * N * K)
        r["shape"] = [M, N, K]
        doc["shapes"][name] = r
        for arm in tot:
            tot[arm] += r[arm]["median_ms"]
        print(name, r, file=sys.stderr, flush=True)
        del a, b, out
    doc["sum_of_medians_ms"] = {k: round(v, 4) for k, v in tot.items()}
    doc["sum_ratio_v7_over_v6"] = round(tot["v7"] / tot["v6"], 4)
    # the step's bf16-out launches: 12 blocks per tower, each shape once per block
    doc["step_bf16_out_launches_ms"] = {k: round(12 * v, 3) for k, v in tot.items()}
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
