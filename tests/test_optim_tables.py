"""CPU: the host layer of the multi-tensor launches (open_clip_amd/tables.py) -- the chunk-list builder against literal values, the AdamEntry plan on
the shapes of tests/optim_util.py with stand-in operand copies, the per-step mode decision address by address, and NativeMuon's arrangement (flat
records, the update walks the fallback tensors only).  Nothing here touches a device: the plan is a pure host function."""
import numpy as np
import torch

from open_clip_amd import tables
from tests.optim_util import ADAM_SHAPES, MUON_N_MATRICES, MUON_SHAPES


def test_chunk_list_against_literal_values():
    c = tables.chunk_list([1, 1, 1, 1, 2])
    assert c.dtype == np.int32 and c.shape == (6, 2)
    assert c.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [4, 1]]
    assert tables.chunk_list([0, 4]).tolist() == [[1, 0], [1, 1], [1, 2], [1, 3]]  # an entry with count 0 owns no chunk
    assert tables.chunk_list([2, 0, 0, 3, 0]).tolist() == [[0, 0], [0, 1], [3, 0], [3, 1], [3, 2]]
    for empty in ([], [0], [0, 0]):
        c = tables.chunk_list(empty)
        assert c.dtype == np.int32 and c.shape == (0, 2)
    assert tables.chunk_list(np.asarray([3], dtype=np.int32)).tolist() == [[0, 0], [0, 1], [0, 2]]
    assert tables.CHUNK == 8192


def _params_and_copies(shapes, cached):
    params = [torch.zeros(sh) for sh in shapes]
    copies = []
    for i, p in enumerate(params):
        if i in cached:
            rows = p.shape[0]
            copies.append((torch.zeros(rows, p.numel() // rows, dtype=torch.bfloat16), torch.zeros(p.numel() // rows, rows, dtype=torch.bfloat16)))
        else:
            copies.append((None, None))
    return params, copies


def test_adam_plan_on_cpu_tensors():
    cached = [i for i, sh in enumerate(ADAM_SHAPES) if len(sh) in (2, 4)]
    params, copies = _params_and_copies(ADAM_SHAPES, cached)
    ent, counts, kept = tables.adam_plan(params, copies)
    assert ent.dtype == tables.ADAM_ENTRY and ent.dtype.itemsize == 88
    got = [(int(e["rows"]), int(e["cols"]), int(e["mode"]), k, bool(e["w16n"]), bool(e["w16t"])) for e, k in zip(ent, counts)]
    assert got == [(64, 128, 1, 2, True, True),    # tile mode: one chunk per 64x64 tile
                   (128, 64, 1, 2, True, True),
                   (64, 64, 1, 1, True, True),     # (64, 1, 8, 8) as [64, 64]
                   (50, 72, 0, 1, True, False),    # not 64-divisible: the transposed copy stays on the cast path
                   (1, 8199, 0, 2, False, False),
                   (1, 8197, 0, 2, False, False),
                   (1, 1, 0, 1, False, False),
                   (1, 40, 0, 1, False, False)]
    assert ent["numel"].tolist() == [p.numel() for p in params]
    for e, (n16, t16), (kn, kt) in zip(ent, copies, kept):
        assert kn is n16 and int(e["w16n"]) == (0 if n16 is None else n16.data_ptr())
        assert kt is (t16 if e["mode"] == 1 else None) and int(e["w16t"]) == (0 if kt is None else kt.data_ptr())
    # without a cached transposed copy there is no tile mode, whatever the shape
    ent, counts, kept = tables.adam_plan(params[:1], [(copies[0][0], None)])
    assert (int(ent["mode"][0]), counts, int(ent["w16t"][0]), kept[0][1]) == (0, [1], 0, None) and int(ent["w16n"][0]) == copies[0][0].data_ptr()
    plan = tables.AdamTables("test", params, copies)
    assert plan.chunks.shape == (12, 2) and plan.update_chunks.tolist() == plan.chunks.tolist()
    assert plan.chunks.tolist() == tables.chunk_list([2, 2, 1, 1, 2, 2, 1, 1]).tolist()


def _slot(n, off):
    """n floats whose address is ``off`` floats past the 16-byte grid"""
    buf = torch.zeros(n + 8)
    lead = (-buf.data_ptr() // 4) % 4  # floats up to the next 16-byte boundary
    t = buf[lead + off:lead + off + n]
    assert t.data_ptr() % 16 == 4 * off
    return t


def _refreshed_mode(shape, copies, offs):
    """the mode of the one record after a refresh with p, g, m, v at the given float offsets from the 16-byte grid"""
    n = int(np.prod(shape))
    p, g, m, v = (_slot(n, o).view(shape) for o in offs)
    p = torch.nn.Parameter(p)
    p.grad = g
    plan = tables.AdamTables("test", [p], [copies])
    st = {"step": 4, "exp_avg": m, "exp_avg_sq": v}
    filled = []
    grads = plan.refresh([("group", p)], {p: st}, {"step": (0, int)}, lambda *a: filled.append(a) or (0.5, 0.25, 2.0, 4.0), "shared")
    e = plan.records[0]
    assert grads[0] is g and st["step"] == 5 and filled == [("group", st, "shared")]
    assert [float(e[k]) for k in ("lr", "wd", "bc1", "bc2_sqrt")] == [0.5, 0.25, 2.0, 4.0]
    assert [int(e[k]) for k in "wgmv"] == [t.data_ptr() for t in (p, g, m, v)]
    return int(e["mode"])


def test_mode_decision_address_by_address():
    assert _refreshed_mode((40,), (None, None), (0, 0, 0, 0)) == 0
    for k in range(4):  # each of p, g, m, v off the 16-byte grid in turn
        for off in (1, 2, 3):
            offs = [0] * 4
            offs[k] = off
            assert _refreshed_mode((40,), (None, None), offs) == 2, offs
    n16, t16 = torch.zeros(64, 128, dtype=torch.bfloat16), torch.zeros(128, 64, dtype=torch.bfloat16)
    assert _refreshed_mode((64, 128), (n16, t16), (0, 0, 0, 0)) == 1
    assert _refreshed_mode((64, 128), (n16, t16), (0, 1, 0, 0)) == 1  # tile mode stays: the kernel reads an unaligned gradient element by element
    assert _refreshed_mode((64, 128), (n16, None), (0, 0, 0, 0)) == 0
    assert _refreshed_mode((64, 128), (n16, None), (0, 1, 0, 0)) == 2
    # a tensor the clip alone reads: the gradient's address decides
    p = torch.nn.Parameter(_slot(40, 0))
    for off, mode in ((0, 0), (1, 2)):
        p.grad = _slot(40, off)
        plan = tables.AdamTables("test", [p], [(None, None)], update=[False])
        state = {p: {}}
        plan.refresh([({}, p)], state, {"step": (0, int)}, None, None)
        e = plan.records[0]
        assert int(e["mode"]) == mode and int(e["g"]) == p.grad.data_ptr() and int(e["m"]) == 0 and state == {p: {}}


def test_muon_arrangement():
    """every active parameter enters flat, never in tile mode; the update chunk list covers exactly the fallback entries; a fallback weight's
    transposed copy stays on the cast path"""
    from open_clip_amd.optim import NativeMuon
    shapes = MUON_SHAPES + [(64, 128)]  # the last one: a 2-D weight on the fallback side (use_fallback), both copies cached
    is_muon = [i < MUON_N_MATRICES for i in range(len(shapes))]
    params, copies = _params_and_copies(shapes, [2, len(shapes) - 1])
    groups = {True: {"lr": 0.02}, False: {"lr": 0.01, "use_fallback": True}}
    plan = NativeMuon._adam_tables([(groups[m], p) for m, p in zip(is_muon, params)], copies)  # the call NativeMuon._build_plan makes
    ent = plan.records
    assert ent["mode"].tolist() == [0] * len(shapes) and ent["rows"].tolist() == [1] * len(shapes)
    assert ent["cols"].tolist() == ent["numel"].tolist() == [p.numel() for p in params]
    counts = [-(-p.numel() // 8192) for p in params]
    assert plan.chunks.tolist() == tables.chunk_list(counts).tolist() and sorted(set(plan.chunks[:, 0].tolist())) == list(range(len(shapes)))
    fallback = [i for i, m in enumerate(is_muon) if not m]
    assert sorted(set(plan.update_chunks[:, 0].tolist())) == fallback
    assert plan.update_chunks.tolist() == [[i, k] for i in fallback for k in range(counts[i])]
    assert ent["w16t"].tolist() == [0] * len(shapes)
    assert [bool(x) for x in ent["w16n"]] == [False] * (len(shapes) - 1) + [True]
    assert plan.copies[-1] == (copies[-1][0], None) and plan.copies[2] == (None, None)
