"""Times the native validation metrics on one MI355X and writes profiles/retrieval_metrics.json.

    python tools/retrieval_metrics_bench.py [--n 32768] [--e 512] [--reps 7] [--out profiles/retrieval_metrics.json]

One process.  ``open_clip_amd.metrics.get_clip_metrics`` on N paired unit-norm features of width E, in both precisions ("fp32" = the three-term bf16 split,
"bf16" = one term), against the REFERENCE'S FORMULA restated in torch on the same GPU: fp32 features, chunks of 4096, per chunk pair one ``matmul``, the two
compare-and-count passes of both directions, then the same ten reductions (open_clip_train/metrics.py:95-176 describes the arithmetic; the loop below is
written from that description, not imported).  Every figure is the MEDIAN of ``reps`` calls, each between its own pair of HIP events after two warm-up
calls; a call ends with the host reading the ten values, as the reference's does, so the interval holds the whole metric.  The two sides' ranks are compared
too: rows where they differ are counted (fp32 matmul and the split product round differently; near-ties may swap).
Needs the GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 4096


def features(n, e, dev):
    gen = torch.Generator().manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(n, e, generator=gen), dim=-1)
    y = torch.nn.functional.normalize(0.35 * x + torch.nn.functional.normalize(torch.randn(n, e, generator=gen), dim=-1), dim=-1)
    return x.to(dev), y.to(dev)


def chunked_torch_ranks(image, text, scale=100.0, chunk=CHUNK):
    """the reference's evaluation order in plain torch: targets from the paired chunks' diagonals, then every chunk pair once for both directions"""
    n = image.shape[0]
    idx = torch.arange(n, device=image.device)
    targets = torch.empty(n, device=image.device, dtype=torch.float32)
    for a in range(0, n, chunk):
        targets[a:a + chunk] = (scale * (image[a:a + chunk] @ text[a:a + chunk].t())).diagonal()
    i2t = torch.zeros(n, device=image.device, dtype=torch.long)
    t2i = torch.zeros(n, device=image.device, dtype=torch.long)
    for a in range(0, n, chunk):
        ti, qi = targets[a:a + chunk, None], idx[a:a + chunk, None]
        for b in range(0, n, chunk):
            s = scale * (image[a:a + chunk] @ text[b:b + chunk].t())
            tt, qt = targets[None, b:b + chunk], idx[None, b:b + chunk]
            i2t[a:a + chunk] += ((s > ti) | ((s == ti) & (qt < qi))).sum(dim=1)
            t2i[b:b + chunk] += ((s > tt) | ((s == tt) & (qi < qt))).sum(dim=0)
    return i2t, t2i


def chunked_torch_metrics(image, text):
    from open_clip_amd.metrics import _add_rank_metrics
    i2t, t2i = chunked_torch_ranks(image, text)
    out = {}
    _add_rank_metrics(out, "image_to_text", i2t)
    _add_rank_metrics(out, "text_to_image", t2i)
    return out


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 3), "min_ms": round(times[0], 3), "max_ms": round(times[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_metrics.json"))
    args = ap.parse_args()
    from open_clip_amd import metrics

    dev = torch.device("cuda")
    x, y = features(args.n, args.e, dev)
    native = {p: median_ms(lambda p=p: metrics.get_clip_metrics(x, y, 100.0, retrieval_dtype=p), args.reps) for p in ("fp32", "bf16")}
    torch_fp32 = median_ms(lambda: chunked_torch_metrics(x, y), args.reps)

    ref_ranks = chunked_torch_ranks(x, y)
    differ = {}
    for p in ("fp32", "bf16"):
        got = metrics.paired_retrieval_ranks(x, y, precision=p)
        differ[p] = {name: int((g != r).sum()) for name, g, r in zip(("image_to_text", "text_to_image"), got, ref_ranks)}
    flops = {"fp32": 2 * 2.0 * args.n * args.n * 3 * args.e, "bf16": 2 * 2.0 * args.n * args.n * args.e}  # two directions; executed MFMA work
    ratio = torch_fp32["median_ms"] / native["fp32"]["median_ms"]
    result = {
        "host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "n": args.n, "e": args.e, "reps": args.reps,
        "native_get_clip_metrics": native,
        "torch_chunked_fp32": dict(torch_fp32, chunk=CHUNK),
        "native_tflops": {p: round(flops[p] / (native[p]["median_ms"] * 1e-3) / 1e12, 1) for p in native},
        "rows_ranked_differently_from_torch_fp32": differ,
        "torch_over_native_fp32": round(ratio, 3),
        "verdict": ("native fp32 mode is faster than the chunked torch formula" if ratio > 1 else
                    "native fp32 mode is SLOWER than the chunked torch formula (its main loop: DESIGN.md section 4, row label_rank_kernel)"),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
