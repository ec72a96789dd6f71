"""CPU: the host-side pieces of eprecon_amd.train and eprecon_amd.optim — learning-rate schedule, rank blocks, checkpoint
names, the optimiser's chunk table and its table structs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_order_lrs(lr, lrepochs, start_epoch, epochs, seed_lr):
    """main.py:250-258: MultiStepLR constructed with last_epoch = start_epoch - 1 on an optimiser whose lr (and initial_lr,
    on resume) is seed_lr, then .step() at the top of every epoch -> the lr of every epoch run"""
    from eprecon_amd.train import parse_lrepochs
    milestones, gamma = parse_lrepochs(lrepochs)
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=seed_lr)
    if start_epoch > 0:
        opt.param_groups[0]["initial_lr"] = seed_lr
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones, gamma=gamma, last_epoch=start_epoch - 1)
    out = []
    for _ in range(start_epoch, epochs):
        opt.step()
        sched.step()
        out.append(opt.param_groups[0]["lr"])
    return out


@pytest.mark.parametrize("lrepochs,epochs,resume_at", [("70,90:10", 100, 50), ("70,90:10", 100, 80), ("12,24,36:2", 40, 20),
                                                       ("12,24,36:2", 40, 30)])
def test_lr_at_is_the_reference_schedule(lrepochs, epochs, resume_at):
    from eprecon_amd.train import lr_at
    lr = 1e-4
    fresh = reference_order_lrs(lr, lrepochs, 0, epochs, lr)
    assert fresh == pytest.approx([lr_at(e, lr, lrepochs) for e in range(epochs)], rel=1e-12)
    assert fresh[0] == lr and len(set(fresh)) == len(lrepochs.split(":")[0].split(",")) + 1
    # the schedule stands one epoch ahead of its milestones: the top-of-epoch step
    first = int(lrepochs.split(",")[0])
    assert lr_at(first - 2, lr, lrepochs) == lr and lr_at(first - 1, lr, lrepochs) < lr
    # a resumed run: the reference seeds the scheduler with the checkpoint's lr, the one of the epoch before
    resumed = reference_order_lrs(lr, lrepochs, resume_at, epochs, fresh[resume_at - 1])
    assert resumed == pytest.approx([lr_at(e, lr, lrepochs) for e in range(resume_at, epochs)], rel=1e-12)


def test_rank_indices_are_contiguous_blocks_of_the_wrapped_list():
    from eprecon_amd.train import rank_indices
    want = {(10, 4): [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 0, 1]],
            (8, 4): [[0, 1], [2, 3], [4, 5], [6, 7]],
            (3, 4): [[0], [1], [2], [0]],
            (1, 1): [[0]]}
    for (n, world), blocks in want.items():
        got = [rank_indices(n, world, r) for r in range(world)]
        assert got == blocks, (n, world)
        assert len({len(b) for b in got}) == 1


def test_checkpoint_names_and_latest():
    from eprecon_amd.train import checkpoint_name, latest_checkpoint
    assert checkpoint_name(0) == "model_000000.ckpt" and checkpoint_name(99) == "model_000099.ckpt"
    assert checkpoint_name(1234567) == "model_1234567.ckpt"
    names = ["model_000009.ckpt", "model_000010.ckpt", "model_000002.ckpt", "train_scalars.jsonl", "model_best.ckpt", "model_000011.ckpt.tmp"]
    assert latest_checkpoint(names) == "model_000010.ckpt"
    assert latest_checkpoint(names + ["model_1000000.ckpt", "model_999999.ckpt"]) == "model_1000000.ckpt"
    assert latest_checkpoint(["notes.txt"]) is None and latest_checkpoint([]) is None


def test_chunk_table_covers_every_element_once():
    from eprecon_amd import _lib
    from eprecon_amd.optim import CHUNK, build_chunk_table
    sizes = [1, 4095, 4096, 4097, 248832, 1000]
    base = 0x7F0000000000
    ptrs = [(base + 0x100000 * (4 * s), base + 0x100000 * (4 * s + 1), base + 0x100000 * (4 * s + 2), base + 0x100000 * (4 * s + 3))
            for s in range(len(sizes))]
    ptrs[-1] = (ptrs[-1][0] + 4,) + ptrs[-1][1:]          # the last parameter is a view one float into its storage
    ptrs[1] = (ptrs[1][0], ptrs[1][1] + 4) + ptrs[1][2:]  # ... and this one's gradient is
    table = build_chunk_table(sizes, ptrs)
    assert CHUNK == 4096 and len(table) == sum(-(-n // CHUNK) for n in sizes)
    for s, n in enumerate(sizes):
        rows = table[table["segment"] == s]
        covered = np.zeros(n, dtype=np.int64)
        for r in rows:
            assert 0 < r["count"] <= CHUNK and r["start"] % CHUNK == 0 and r["start"] + r["count"] <= n   # inside its segment
            covered[r["start"]:r["start"] + r["count"]] += 1
        assert (covered == 1).all(), s
        all_aligned = all(p % 16 == 0 for p in ptrs[s])
        want = (_lib.ADAM_ALL_ALIGNED if all_aligned else 0) | (_lib.ADAM_GRAD_ALIGNED if ptrs[s][1] % 16 == 0 else 0)
        assert (rows["flags"] == want).all(), s
    assert (table[table["segment"] == 5]["flags"] == _lib.ADAM_GRAD_ALIGNED).all()       # scalar update, vector norm
    assert (table[table["segment"] == 1]["flags"] == 0).all()
    assert (table[table["segment"] == 4]["flags"] == 3).all() and (table["segment"] == 4).sum() == 61
    assert list(table["segment"]) == sorted(table["segment"])
    with pytest.raises(ValueError):
        build_chunk_table([0], [ptrs[0]])


@pytest.mark.parametrize("c_name,py_name,np_name", [("eprecon_adam_segment", "AdamSegment", "SEGMENT_DTYPE"),
                                                    ("eprecon_adam_chunk", "AdamChunk", "CHUNK_DTYPE")])
def test_optimizer_table_layouts_match_header(tmp_path, c_name, py_name, np_name):
    """the ctypes mirrors and the numpy records the tables are built in have the C compiler's size and field offsets"""
    from eprecon_amd import _lib, optim
    mirror, record = getattr(_lib, py_name), getattr(optim, np_name)
    fields = [f[0] for f in mirror._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "eprecon_hip.h"', 'int main(void) {',
           f'  printf("%zu\\n", sizeof({c_name}));']
    src += [f'  printf("%zu\\n", offsetof({c_name}, {name}));' for name in fields]
    src += ['  printf("%d %d\\n", EPRECON_ADAM_ALL_ALIGNED, EPRECON_ADAM_GRAD_ALIGNED);', '  return 0;', '}']
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(mirror) == record.itemsize
    assert out[1:-2] == [getattr(mirror, name).offset for name in fields] == [record.fields[name][1] for name in fields]
    assert list(record.names) == fields
    assert out[-2:] == [_lib.ADAM_ALL_ALIGNED, _lib.ADAM_GRAD_ALIGNED]


def test_freeze_choices_and_defaults():
    from eprecon_amd import train
    args = train.parse_args(["--data_path", "d", "--logdir", "l"])
    assert (args.batch_size, args.accumulation_steps, args.lr, args.wd, args.lrepochs, args.freeze) == (4, 8, 1e-4, 0.0, "70,90:10", "init")
    assert args.optimizer in ("fused", "torch") and args.epochs == 100 and args.n_views == 9
    assert train.MAX_READERS <= 9
