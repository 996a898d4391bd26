"""A/B of the two main loops of the hand-scheduled wgrad kernel (gemm_tn5.hip): ocn_set_gemm_variant TN field 6 = v_mfma_f32_32x32x16_bf16,
7 = v_mfma_f32_16x16x32_bf16, interleaved in ONE process on the step's eight wgrad shapes and its two paired launches (ViT-B-32, local batch
4096, packed text).  Random Gaussian operands (never zeros: the clock a power-limited loop holds depends on the data); >= 2 s of back-to-back
launches before the first sample of a shape, then alternating rounds of event-timed launches.  Per arm: median, min, max; the ratio of the medians
counts as a difference only outside the larger of the two arms' min-max spreads.  ``--epilogue`` adds the epilogue share of both forms (developer
knob 4 = 1 skips the atomics) on the out-proj + QKV pairs and on text out-proj.  ``--stamps`` (developer build only: OCN_LIB_PATH =
libopenclip_hip_dev.so) adds the shader clock each form held inside its main loop, from the kernel's own s_memtime / s_memrealtime stamps
(knob 4 = 4).  One JSON document on stdout:

    python tools/ab_tn_mfma_shape.py --epilogue > tn5_mfma_shape_ab.json"""
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
SINGLE = [  # (name, M, N, K, dbias): dW[N, K] over M rows
    ("img qkv", Mi, 2304, 768, True), ("img out", Mi, 768, 768, True), ("img fc", Mi, 3072, 768, True), ("img proj", Mi, 768, 3072, True),
    ("txt qkv", Mt, 1536, 512, True), ("txt out", Mt, 512, 512, True), ("txt fc", Mt, 2048, 512, True), ("txt proj", Mt, 512, 2048, True),
]
PAIRS = [("img out+qkv", Mi, 768), ("txt out+qkv", Mt, 512)]  # (name, M, C): dW[C, C] and dW[3C, C] in one launch
ARMS = (6, 7)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def ab(fn, launches, warm_s, knob4=0):
    """{arm: [ms, ...]} of ``launches`` event-timed launches per arm in alternating rounds of 4, behind ``warm_s`` seconds of alternating launches"""
    _lib.call("ocn_set_tuning", 4, knob4)
    t0 = time.time()
    while time.time() - t0 < warm_s:
        for arm in ARMS:
            _lib.call("ocn_set_gemm_variant", arm << 4)
            for _ in range(8):
                fn()
        torch.cuda.synchronize()
    ms = {arm: [] for arm in ARMS}
    for rnd in range((launches + 3) // 4):
        for arm in (ARMS if rnd % 2 == 0 else ARMS[::-1]):
            _lib.call("ocn_set_gemm_variant", arm << 4)
            fn()  # (the first launch behind a switch is not a sample)
            ms[arm] += [event_ms(fn) for _ in range(4)]
    _lib.call("ocn_set_gemm_variant", 0)
    _lib.call("ocn_set_tuning", 4, 0)
    return ms


def loop_clock(fn):
    """{arm: median MHz over the stamped workgroups} of the main loop (developer build: delta s_memtime / delta s_memrealtime, 100 MHz ticks)"""
    import ctypes
    out = {}
    buf = (ctypes.c_longlong * 1024)()
    _lib.call("ocn_set_tuning", 4, 4)
    for arm in ARMS:
        _lib.call("ocn_set_gemm_variant", arm << 4)
        for _ in range(16):
            fn()
        torch.cuda.synchronize()
        _lib.call("ocn_debug_nt5_trace", ctypes.addressof(buf))
        mhz = [100.0 * buf[2 * w] / buf[2 * w + 1] for w in range(512) if buf[2 * w + 1] > 0]
        out[f"v{arm}"] = {"median_mhz": round(statistics.median(mhz), 1), "min_mhz": round(min(mhz), 1), "max_mhz": round(max(mhz), 1), "workgroups": len(mhz)}
    _lib.call("ocn_set_gemm_variant", 0)
    _lib.call("ocn_set_tuning", 4, 0)
    return out


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
    ap.add_argument("--epilogue", action="store_true")
    ap.add_argument("--stamps", action="store_true")
    args = ap.parse_args()
    doc = {"device": torch.cuda.get_device_name(0), "arms": {"v6": "32x32x16 main loop", "v7": "16x16x32 main loop"}, "launches_per_arm": args.launches,
           "warm_seconds": args.warm, "operands": "randn bf16", "single": {}, "pair": {}, "epilogue_share": {}}
    g = torch.Generator(device=dev).manual_seed(1)
    tot = {"v6": 0.0, "v7": 0.0}
    for name, M, N, K, bias in SINGLE:
        a, b = torch.randn(M, N, device=dev, generator=g).bfloat16(), torch.randn(M, K, device=dev, generator=g).bfloat16()
        dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        fn = lambda: ops.gemm_tn_accum(a, b, dw, db if bias else None)  # noqa: E731
        r = summary(ab(fn, args.launches, args.warm), 2.0 * M * N * K)
        r["shape"] = [M, N, K]
        if args.stamps:
            r["main_loop_clock"] = loop_clock(fn)
        doc["single"][name] = r
        for arm in tot:
            tot[arm] += r[arm]["median_ms"]
        print(name, r, file=sys.stderr, flush=True)
        if args.epilogue and name == "txt out":
            e = summary(ab(fn, args.launches, 0.5, knob4=1), 2.0 * M * N * K)
            doc["epilogue_share"][name] = {arm: round(1.0 - e[arm]["median_ms"] / r[arm]["median_ms"], 4) for arm in ("v6", "v7")}
        del a, b
    doc["sum_of_medians_single_ms"] = {k: round(v, 4) for k, v in tot.items()}
    for name, M, C in PAIRS:
        a1, b1 = torch.randn(M, C, device=dev, generator=g).bfloat16(), torch.randn(M, C, device=dev, generator=g).bfloat16()
        a2, b2 = torch.randn(M, 3 * C, device=dev, generator=g).bfloat16(), torch.randn(M, C, device=dev, generator=g).bfloat16()
        dw1, dw2, db1, db2 = torch.zeros(C, C, device=dev), torch.zeros(3 * C, C, device=dev), torch.zeros(C, device=dev), torch.zeros(3 * C, device=dev)
        fn = lambda: ops.gemm_tn_accum2(a1, b1, dw1, db1, a2, b2, dw2, db2)  # noqa: E731
        r = summary(ab(fn, args.launches, args.warm), 2.0 * M * 4 * C * C)
        r["shape"] = [M, C]
        if args.stamps:
            r["main_loop_clock"] = loop_clock(fn)
        doc["pair"][name] = r
        print(name, r, file=sys.stderr, flush=True)
        if args.epilogue:
            e = summary(ab(fn, args.launches, 0.5, knob4=1), 2.0 * M * 4 * C * C)
            doc["epilogue_share"][name] = {arm: round(1.0 - e[arm]["median_ms"] / r[arm]["median_ms"], 4) for arm in ("v6", "v7")}
        del a1, b1, a2, b2
    # the step's wgrad launches: fc, proj and the out + qkv pair of each tower's blocks (12 layers each)
    step = {arm: 12 * sum(doc["single"][n][arm]["median_ms"] for n in ("img fc", "img proj", "txt fc", "txt proj"))
            + 12 * sum(doc["pair"][n][arm]["median_ms"] for n in ("img out+qkv", "txt out+qkv")) for arm in ("v6", "v7")}
    doc["step_wgrad_launches_ms"] = {k: round(v, 3) for k, v in step.items()}
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
