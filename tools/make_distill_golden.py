"""Records the REFERENCE's ``DistillClipLoss`` under gloo and writes tests/golden/distill_loss_w{2,3}.npz (CPU; needs the reference tree).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_distill_golden.py

The reference is imported through ``oracle.ref_shim.import_reference``; nothing of it is copied.  Every rank of a world of 2 and of 3 evaluates
``DistillClipLoss(rank, world_size, **mode)(img, txt, scale, dist_img, dist_txt, dist_scale)`` on seeded unit features -- student [B = 5, E = 32],
teacher [5, E_t = 48]: the widths differ on purpose -- in the three modes oracle/make_golden.py records for ``ClipLoss`` (global, local_loss with and
without gather_with_grad) and in the global gather_with_grad mode, and differentiates ``contrastive_loss + distill_loss``.
Each file holds: ``feats`` [W, 2, B, E], ``dist_feats`` [W, 2, B, E_t], ``scale``, ``dist_scale`` and, per rank and mode,
``r{rank}/{mode}/contrastive``, ``/distill`` (the two losses) and ``/dimg``, ``/dtxt``, ``/dscale`` (gradients of their sum).  Data only, a few KiB."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_shim import import_reference  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
B, E, E_T = 5, 32, 48
SCALE, DIST_SCALE = 9.5, 14.0
MODES = (("global", dict(local_loss=False, gather_with_grad=False)),
         ("local_gwg", dict(local_loss=True, gather_with_grad=True)),
         ("local_nograd", dict(local_loss=True, gather_with_grad=False)),
         ("global_gwg", dict(local_loss=False, gather_with_grad=True)))


def features(world):
    g = torch.Generator().manual_seed(777 + world)
    feats = torch.nn.functional.normalize(torch.randn(world, 2, B, E, generator=g), dim=-1)
    dist_feats = torch.nn.functional.normalize(torch.randn(world, 2, B, E_T, generator=g), dim=-1)
    return feats, dist_feats


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import_reference()
    from open_clip.loss import DistillClipLoss

    feats, dist_feats = features(world)
    res = {}
    for name, kw in MODES:
        img = feats[rank, 0].clone().requires_grad_(True)
        txt = feats[rank, 1].clone().requires_grad_(True)
        s = torch.tensor(SCALE, requires_grad=True)
        c, d = DistillClipLoss(rank=rank, world_size=world, **kw)(img, txt, s, dist_feats[rank, 0], dist_feats[rank, 1], torch.tensor(DIST_SCALE))
        (c + d).backward()
        res[f"{name}/contrastive"] = c.detach().numpy()
        res[f"{name}/distill"] = d.detach().numpy()
        res[f"{name}/dimg"] = img.grad.numpy()
        res[f"{name}/dtxt"] = txt.grad.numpy()
        res[f"{name}/dscale"] = s.grad.numpy()
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def make(world, port):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join()
    feats, dist_feats = features(world)
    out = {"feats": feats.numpy(), "dist_feats": dist_feats.numpy(), "scale": np.float32(SCALE), "dist_scale": np.float32(DIST_SCALE)}
    for rank, res in got:
        for k, v in res.items():
            out[f"r{rank}/{k}"] = v
    path = os.path.join(GOLD, f"distill_loss_w{world}.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes", {k: round(float(v), 6) for k, v in out.items() if k.endswith("/distill")})


if __name__ == "__main__":
    torch.use_deterministic_algorithms(True)
    make(2, 29741)
    make(3, 29742)
