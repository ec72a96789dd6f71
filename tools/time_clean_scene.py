"""One timing of the scene clean-up (eprecon_amd/clean_scene.py, csrc/components.hip) next to a torch composition of the same
rule on the same rows in the same process.

    python tools/time_clean_scene.py [--voxel 0.04] [--floaters 400] [--reps 20] [--connectivity 26] [--out FILE.json]

The rows: the cells with |tsdf| < 1 of the analytic room of eprecon_amd/synthetic.py at --voxel (tools/eval_scene_timing.py's
volume: 96^3 voxels at 4 cm, a 3-voxel truncation), labelled in 16^3-cell blocks (semantic 1..5, instance 1..6), plus
--floaters seeded single rows and pairs in free space and a seeded 1 % of rows with a spurious id; in a seeded random order.
HIP events around each call, [median, min, max] ms of --reps after warm-up, the calls alternating rep by rep:

    components        clean_scene.components on the geometry rows: table, self map, the three launches, the one read
    labelling         eprecon_components_async alone on a map built once (no read)
    clean_rows        the rule with every option on (min_voxels 50, min_segment_voxels 10, split_instances)
    torch_components  the yardstick: the same labels as an iterated neighbour-minimum with pointer jumping over the same map,
                      until nothing changes (one host read per round)
    torch_clean_rows  the same rule with that labelling in place of the kernel's

`rounds` is how often the yardstick iterated; `labels_equal` / `rows_equal` say that both ways gave the same integers.
Writes nothing into the repository unless --out is given.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def self_map(torch, coords):
    """the library's table and symmetric map of int32[M,3] rows -> nbr int32[27,M]"""
    from eprecon_amd import _lib
    from eprecon_amd.sparse import HashGrid
    m, dev = coords.shape[0], coords.device
    rows = torch.zeros((m, 4), dtype=torch.int32, device=dev)
    rows[:, 1:] = coords
    grid = HashGrid(m, dev).build(rows)
    nbr = torch.empty((27, m), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().eprecon_kernel_map_self_async(_lib.ptr(grid.mem), grid.capacity, _lib.ptr(rows), m, 1, _lib.ptr(nbr),
                                                         _lib.current_stream()), "eprecon_kernel_map_self_async")
    return nbr


def torch_labels(torch, nbr, keys, connectivity, rounds=None):
    """label int32[M] by neighbour-minimum rounds with one pointer jump each, until a round changes nothing"""
    m = nbr.shape[1]
    if m == 0:
        return torch.empty(0, dtype=torch.int32, device=nbr.device)
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    ks = [k for k in range(27) if k != 13 and (k % 3 != 1) + ((k // 3) % 3 != 1) + (k // 9 != 1) <= limit]
    nb = nbr[ks].long()
    linked = nb >= 0
    nb = nb.clamp(min=0)
    if keys is not None:
        linked &= (keys[nb] == keys[None]) & (keys[None] >= 0)
    label = torch.arange(m, device=nbr.device)
    big = torch.full_like(nb, m)
    n_rounds = 0
    while True:
        new = torch.minimum(label, torch.where(linked, label[nb], big).min(0).values)
        new = new[new]
        n_rounds += 1
        if torch.equal(new, label):
            break
        label = new
    if rounds is not None:
        rounds.append(n_rounds)
    if keys is not None:
        label = torch.where(keys < 0, torch.full_like(label, -1), label)
    return label.to(torch.int32)


def room_rows(torch, np, voxel, floaters):
    from eprecon_amd import synthetic as S
    origin = np.array([-1.92, 0.2, -0.4])
    dims = [int(round(3.84 / voxel))] * 3
    ax = [origin[a] + np.arange(dims[a]) * voxel for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    tsdf = np.clip(S.scene_sdf(x, y, z) / (3 * voxel), -1, 1).astype(np.float32)
    rng = np.random.default_rng(0)
    free = np.argwhere(tsdf == 1)
    for c in free[rng.choice(len(free), min(floaters, len(free)), replace=False)]:
        tsdf[c[0], c[1], c[2]] = 0.0
        if rng.random() < 0.5 and c[0] + 1 < dims[0] and tsdf[c[0] + 1, c[1], c[2]] == 1:
            tsdf[c[0] + 1, c[1], c[2]] = 0.25
    coords = np.argwhere(np.abs(tsdf) < 1)
    coords = coords[rng.permutation(len(coords))]
    b = coords // 16
    sem = 1 + (b[:, 0] + 3 * b[:, 1]) % 5
    ins = 1 + b[:, 2] % 6
    spurious = rng.random(len(coords)) < 0.01
    ins[spurious] = 100 + rng.integers(0, 50, spurious.sum())
    to = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    return (to(coords, torch.int32), to(tsdf[tuple(coords.T)], torch.float32), to(sem, torch.int64), to(ins, torch.int64)), dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--floaters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--connectivity", type=int, default=26, choices=[6, 18, 26])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from time_render import event_ms
    from eprecon_amd import _lib
    from eprecon_amd import clean_scene as CS

    (coords, tsdf, sem, ins), dims = room_rows(torch, np, args.voxel, args.floaters)
    m, conn = coords.shape[0], args.connectivity
    rule = dict(min_voxels=50, min_segment_voxels=10, split_instances=True, connectivity=conn)
    lib = _lib.load()
    nbr = self_map(torch, coords)
    label = torch.empty(m, dtype=torch.int32, device="cuda")
    status = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.eprecon_components_workspace_bytes(m)), dtype=torch.uint8, device="cuda")
    labelling = lambda: lib.eprecon_components_async(_lib.ptr(nbr), m, None, conn, _lib.ptr(label), _lib.ptr(status), _lib.ptr(ws),
                                                     ws.numel(), _lib.current_stream())
    rounds = []
    kernel_components = CS.components

    def torch_rule():
        CS.components = lambda c, keys=None, connectivity=26: torch_labels(torch, self_map(torch, c), keys, connectivity)
        try:
            return CS.clean_rows(coords, tsdf, sem, ins, **rule)
        finally:
            CS.components = kernel_components

    ms = event_ms(torch, {
        "components": lambda: CS.components(coords, None, conn),
        "labelling": labelling,
        "clean_rows": lambda: CS.clean_rows(coords, tsdf, sem, ins, **rule),
        "torch_components": lambda: torch_labels(torch, self_map(torch, coords), None, conn, rounds),
        "torch_clean_rows": torch_rule,
    }, args.reps)
    got = CS.components(coords, None, conn)
    want = torch_labels(torch, nbr, None, conn)
    a, b = CS.clean_rows(coords, tsdf, sem, ins, **rule), torch_rule()
    sizes = torch.bincount(got.long())
    res = {"voxel": args.voxel, "dims": dims, "rows": int(m), "connectivity": conn, "reps": args.reps, "ms": ms,
           "components_found": int((sizes > 0).sum()), "largest_component": int(sizes.max()), "rounds": rounds[-1] if rounds else None,
           "status": int(status.item()), "labels_equal": bool(torch.equal(got, want)),
           "rows_equal": bool(all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]), "report": a[4],
           "ns_per_row_labelling": 1e6 * ms["labelling"][0] / max(m, 1),
           "torch_over_components": ms["torch_components"][0] / ms["components"][0],
           "torch_over_clean_rows": ms["torch_clean_rows"][0] / ms["clean_rows"][0]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
